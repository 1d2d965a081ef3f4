// mpcqp_policy.hip — the policy stage of the control tick, batched on the device: the reference's Go1 RL
// controller (src/go1_rl_ctrl_cpp).  Per robot and per tick:
//   observation   observation/Go1Observation.hpp:152-166, float32 cast and previous action  Go1RLController.cpp:95-96
//   network       TorchEigen::run (Go1RLController.cpp:98): 48 -> hidden -> 12 MLP, ELU, float32
//   action        clip, prev_action, scale + default pose, pose limits                        :99-109
//   servo stand   advance_servo                                                                :121-146
//   motor law     tau = Kp (target - q) - Kd dq with the gains of the mode that ran (:79-86, :125-132).  The
//                 reference fills a LowCmd with q = target, dq = 0, tau = 0 (send_cmd, :149-166) and leaves this
//                 line to the motor controller; the tick's output is joint torques, so the stage applies it.
// What Go1RLController keeps between ticks lives in a per-robot slot (MPCQP_PS_*).
//
// One launch, one workgroup of 4 waves per tile of 32 consecutive robots.
//   prologue  thread (robot r = t & 31, part = t >> 5) forms six of the 48 observation entries in binary64
//             (contraction off: bitwise tests/policy_reference.py), checks its inputs, and writes the tile's
//             [32][48] float32 input to LDS; part 0 also reads the slot's scalars and decides update / hold.
//   network   Y[robot][neuron] = X[robot][k] W^T[k][neuron] on v_mfma_f32_32x32x2_f32: A = activations from LDS
//             (lane l: robot l & 31), B = packed weights from global memory (lane l: neuron l & 31), the 32x32
//             result has the neuron on the lane and the robots in the 16 registers.  A lane loads 16 bytes of
//             A and of B per four MFMAs: in k-block kb (8 inputs) lane half h = l >> 5 holds k = 8 kb + 4 h + t
//             for MFMA t = 0..3, the same k for both operands, so an output is one fmaf chain over a fixed
//             permutation of k with the bias as its start.  The waves split a layer's 32-neuron tiles
//             (tile = wave + 4 i, up to 4 accumulators each); ELU (expm1f) runs on the result registers, which
//             then go to the other LDS buffer.  A tile in which no robot runs the network this tick
//             (workgroup-uniform) skips it.
//   epilogue  thread per (robot, joint): clip, targets, slot, torque in binary64.
// Rows are independent in the product; a robot that is not selected, past the batch or has a non-finite input
// enters as a zero row and nothing of it is written.
#pragma clang fp contract(off)

#include "mpcqp_internal.h"

#include <cstring>
#include <vector>

namespace mpcqp {
namespace pol {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int TILE = 32;      // robots per workgroup = rows of one MFMA
constexpr int THREADS = 256;  // 4 waves
constexpr int WAVES = THREADS / 64;
constexpr int ROW_PAD = 4;    // floats: a lane's 16-byte A reads of 16 consecutive rows fall on distinct banks

static_assert(MPCQP_PS_SIZE == 28 && MPCQP_PS_PREV_ACTION == 4 && MPCQP_PS_TARGET == 16, "policy slot layout");
static_assert(MPCQP_PY_OBS == 0 && MPCQP_PY_SIZE == 100, "policy output row layout");

enum : int { F_OK = 1, F_DUE = 2, F_WALK = 4, F_BAD = 8 };

// rot^T v, entry i = (R0i v0 + R1i v1) + R2i v2 (Go1Observation.hpp:152, :154)
__device__ __forceinline__ double rt_v(const double* r, int i, double v0, double v1, double v2) {
  return (r[i] * v0 + r[3 + i] * v1) + r[6 + i] * v2;
}

// One layer for the NT tiles of this wave: acc = bias; acc += A B over K; ELU; to LDS.
template <int NT>
__device__ __forceinline__ void layer(const float* __restrict__ w, const float* __restrict__ bias, const int K,
                                      const int ntiles, const float* in, const int in_stride, float* out,
                                      const int out_stride, const bool elu, const int wave, const int lane) {
  const int r = lane & 31, h = lane >> 5;
  const int kblocks = K >> 3;
  f32x16 acc[NT];
#pragma unroll
  for (int i = 0; i < NT; ++i) {
    const int tile = wave + WAVES * i;
    const float b = tile < ntiles ? bias[tile * 32 + r] : 0.0f;
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[i][e] = b;
  }
  const float4* ap = reinterpret_cast<const float4*>(in + r * in_stride + 4 * h);
  const float4* wp = reinterpret_cast<const float4*>(w) + lane;
  for (int kb = 0; kb < kblocks; ++kb) {
    const float4 a = ap[2 * kb];
#pragma unroll
    for (int i = 0; i < NT; ++i) {
      const int tile = wave + WAVES * i;
      if (tile < ntiles) {
        const float4 b = wp[(size_t)(tile * kblocks + kb) * 64];
        acc[i] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, b.x, acc[i], 0, 0, 0);
        acc[i] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, b.y, acc[i], 0, 0, 0);
        acc[i] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, b.z, acc[i], 0, 0, 0);
        acc[i] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, b.w, acc[i], 0, 0, 0);
      }
    }
  }
#pragma unroll
  for (int i = 0; i < NT; ++i) {
    const int tile = wave + WAVES * i;
    if (tile < ntiles) {
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int row = (e & 3) + 8 * (e >> 2) + 4 * h;  // the 32x32 C/D map: column on the lane
        float v = acc[i][e];
        if (elu) v = v > 0.0f ? v : expm1f(v);
        out[row * out_stride + tile * 32 + r] = v;
      }
    }
  }
}

__global__ __launch_bounds__(THREADS) void policy_kernel(
    const PolicyImage* __restrict__ img, const float* __restrict__ wts, const int stride0, const int stride1,
    const double* __restrict__ sensors, const double* __restrict__ states, const double* __restrict__ plan_in,
    const double* __restrict__ cmds, const int batch, double* __restrict__ slots, const int* __restrict__ type,
    const int want, double* __restrict__ torques, double* __restrict__ outs) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  __shared__ double s_tick[TILE], s_servo[TILE];
  __shared__ int s_flags[TILE], s_bad[TILE];
  float* buf0 = lds;
  float* buf1 = lds + TILE * stride0;
  const mpcqp_policy_params& P = img->p;

  const int t = threadIdx.x;
  const int r = t & 31, part = t >> 5;
  const int base = blockIdx.x * TILE;
  const int b = base + r;
  const bool sel = b < batch && (type == nullptr || type[b] == want);
  if (t < TILE) s_bad[t] = 0;
  __syncthreads();

  // ---- prologue: six observation entries per thread
  double v[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  bool fin = true;
  double mode_in = 0.0;
  if (sel) {
    const double* sn = sensors + (size_t)MPCQP_SN_SIZE * b;
    const double* st = states + (size_t)MPCQP_ST_SIZE * b;
    const double* pl = plan_in + (size_t)MPCQP_PL_SIZE * b;
    const double* cm = cmds + (size_t)MPCQP_CM_SIZE * b;
    if (part == 0) {
      // base linear velocity in the yaw frame (:152), base angular velocity (:153)
      double rz[9];
#pragma unroll
      for (int i = 0; i < 9; ++i) {
        rz[i] = pl[MPCQP_PL_ROT_Z + i];
        fin = fin && isfinite(rz[i]);
      }
      const double l0 = st[MPCQP_ST_LIN_VEL], l1 = st[MPCQP_ST_LIN_VEL + 1], l2 = st[MPCQP_ST_LIN_VEL + 2];
      fin = fin && isfinite(l0) && isfinite(l1) && isfinite(l2);
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        v[i] = rt_v(rz, i, l0, l1, l2);
        v[3 + i] = sn[MPCQP_SN_IMU_ANG_VEL + i];
        fin = fin && isfinite(v[3 + i]);
      }
      mode_in = pl[MPCQP_PL_MOVEMENT_MODE];
    } else if (part == 1) {
      // projected gravity (:154), command (:155)
      double rm[9];
#pragma unroll
      for (int i = 0; i < 9; ++i) {
        rm[i] = st[MPCQP_ST_ROT + i];
        fin = fin && isfinite(rm[i]);
      }
#pragma unroll
      for (int i = 0; i < 3; ++i) v[i] = rt_v(rm, i, 0.0, 0.0, -1.0);
      v[3] = cm[MPCQP_CM_VEL];
      v[4] = cm[MPCQP_CM_VEL + 1];
      v[5] = cm[MPCQP_CM_RATE + 2];
      fin = fin && isfinite(v[3]) && isfinite(v[4]) && isfinite(v[5]);
    } else if (part < 4) {
      // joint_pos - default_joint_pos (:156)
#pragma unroll
      for (int i = 0; i < 6; ++i) {
        const int j = 6 * (part - 2) + i;
        const double q = sn[MPCQP_SN_JOINT_POS + j];
        fin = fin && isfinite(q);
        v[i] = q - P.default_joint_pos[j];
      }
    } else if (part < 6) {
      // joint_vel (:157)
#pragma unroll
      for (int i = 0; i < 6; ++i) {
        v[i] = sn[MPCQP_SN_JOINT_VEL + 6 * (part - 4) + i];
        fin = fin && isfinite(v[i]);
      }
    } else {
      // the previous action (Go1RLController.cpp:96)
#pragma unroll
      for (int i = 0; i < 6; ++i) v[i] = slots[(size_t)MPCQP_PS_SIZE * b + MPCQP_PS_PREV_ACTION + 6 * (part - 6) + i];
    }
    if (part < 6) {
      // scale (:161-163) and clip (:166)
      const double c = P.clip_obs;
#pragma unroll
      for (int i = 0; i < 6; ++i) {
        double x = v[i] * P.obs_scale[6 * part + i];
        x = x < c ? x : c;
        x = x > -c ? x : -c;
        v[i] = x;
      }
    }
    if (!fin) s_bad[r] = 1;
  }
  __syncthreads();
  const bool ok = sel && s_bad[r] == 0;
  {
    float* x = buf0 + r * stride0 + 6 * part;
#pragma unroll
    for (int i = 0; i < 6; ++i) {
      const float f = ok ? (float)v[i] : 0.0f;
      x[i] = f;
      if (ok && outs) outs[(size_t)MPCQP_PY_SIZE * b + MPCQP_PY_OBS + 6 * part + i] = (double)f;
    }
  }
  int need = 0;
  if (part == 0) {
    int f = sel ? F_BAD : 0;
    if (ok) {
      const double* sl = slots + (size_t)MPCQP_PS_SIZE * b;
      const double tick = sl[MPCQP_PS_TICK], servo = sl[MPCQP_PS_SERVO_TIME], last = sl[MPCQP_PS_MODE];
      const bool due = fmod(tick, (double)P.decimation) == 0.0;
      const bool walk = due ? mode_in == 1.0 : last == 1.0;  // MainGazebo.cpp:74-83
      f = F_OK | (due ? F_DUE : 0) | (walk ? F_WALK : 0);
      s_tick[r] = tick;
      s_servo[r] = due && !walk ? servo + 1.0 : servo;  // servo_motion_time_ += 1.0 (:136)
      need = due && walk;
    }
    s_flags[r] = f;
  }
  // ---- network
  const int n_layers = img->n_layers;
  if (__syncthreads_or(need)) {
    const int wave = t >> 6, lane = t & 63;
    for (int l = 0; l < n_layers; ++l) {
      const float* in = (l & 1) ? buf1 : buf0;
      float* out = (l & 1) ? buf0 : buf1;
      const int is = (l & 1) ? stride1 : stride0, os = (l & 1) ? stride0 : stride1;
      const int K = img->in[l], ntiles = img->out[l] >> 5;
      const float* w = wts + img->woff[l];
      const float* bias = wts + img->boff[l];
      const bool elu = l + 1 < n_layers;
      switch ((ntiles + WAVES - 1) / WAVES) {
        case 1: layer<1>(w, bias, K, ntiles, in, is, out, os, elu, wave, lane); break;
        case 2: layer<2>(w, bias, K, ntiles, in, is, out, os, elu, wave, lane); break;
        case 3: layer<3>(w, bias, K, ntiles, in, is, out, os, elu, wave, lane); break;
        default: layer<4>(w, bias, K, ntiles, in, is, out, os, elu, wave, lane); break;
      }
      __syncthreads();
    }
  }
  const float* y = (n_layers & 1) ? buf1 : buf0;
  const int ys = (n_layers & 1) ? stride1 : stride0;

  // ---- epilogue: one (robot, joint) per thread
  for (int item = t; item < TILE * 12; item += THREADS) {
    const int rr = item / 12, j = item - 12 * rr;
    const int f = s_flags[rr];
    const int bb = base + rr;
    if (!(f & F_OK)) {
      if ((f & F_BAD) && outs && j == 0) {
        outs[(size_t)MPCQP_PY_SIZE * bb + MPCQP_PY_STATUS] = 1.0;
        outs[(size_t)MPCQP_PY_SIZE * bb + MPCQP_PY_UPDATED] = 0.0;
      }
      continue;
    }
    const double q = sensors[(size_t)MPCQP_SN_SIZE * bb + MPCQP_SN_JOINT_POS + j];
    const double dq = sensors[(size_t)MPCQP_SN_SIZE * bb + MPCQP_SN_JOINT_VEL + j];
    double* sl = slots + (size_t)MPCQP_PS_SIZE * bb;
    const bool due = f & F_DUE, walk = f & F_WALK;
    double raw = 0.0, act, tgt;
    if (due && walk) {
      raw = (double)y[rr * ys + j];  // action_.cast<double>() (:99)
      const double ca = P.clip_action;
      act = raw < ca ? raw : ca;     // :102
      act = act > -ca ? act : -ca;
      tgt = act * P.action_scale;    // :106
      tgt = tgt + P.default_joint_pos[j];  // :107
      const double hi = P.pose_upper[j], lo = P.pose_lower[j];
      tgt = tgt < hi ? tgt : hi;     // :109
      tgt = tgt > lo ? tgt : lo;
      sl[MPCQP_PS_PREV_ACTION + j] = act;  // :103
      sl[MPCQP_PS_TARGET + j] = tgt;
    } else if (due) {
      double percent = s_servo[rr] / P.servo_ticks;  // :139
      if (P.servo_clamp && percent > 1.0) percent = 1.0;
      tgt = q * (1.0 - percent) + P.stand_pos[j] * percent;  // :141
      act = sl[MPCQP_PS_PREV_ACTION + j];
      sl[MPCQP_PS_TARGET + j] = tgt;
    } else {
      act = sl[MPCQP_PS_PREV_ACTION + j];
      tgt = sl[MPCQP_PS_TARGET + j];
    }
    const double kp = walk ? P.kp_walk[j] : P.kp_servo[j];
    const double kd = walk ? P.kd_walk[j] : P.kd_servo[j];
    const double tau = kp * (tgt - q) - kd * dq;
    torques[(size_t)12 * bb + j] = tau;
    if (outs) {
      double* o = outs + (size_t)MPCQP_PY_SIZE * bb;
      o[MPCQP_PY_RAW + j] = raw;
      o[MPCQP_PY_ACTION + j] = act;
      o[MPCQP_PY_TARGET + j] = tgt;
      o[MPCQP_PY_TORQUE + j] = tau;
      if (j == 0) {
        o[MPCQP_PY_STATUS] = 0.0;
        o[MPCQP_PY_UPDATED] = due ? 1.0 : 0.0;
      }
    }
    if (j == 0) {
      sl[MPCQP_PS_INIT] = 1.0;
      sl[MPCQP_PS_TICK] = s_tick[rr] + 1.0;
      sl[MPCQP_PS_SERVO_TIME] = s_servo[rr];
      sl[MPCQP_PS_MODE] = walk ? 1.0 : 0.0;
    }
  }
}

}  // namespace pol

bool policy_layout(const mpcqp_policy_params& p, PolicyImage* img, size_t* n_floats, int* stride0, int* stride1) {
  if (p.n_hidden < 1 || p.n_hidden > 3) return false;
  int chain[5] = {48, 0, 0, 0, 0};
  for (int i = 0; i < p.n_hidden; ++i) {
    if (p.hidden[i] < 32 || p.hidden[i] > 512 || p.hidden[i] % 32) return false;
    chain[1 + i] = p.hidden[i];
  }
  chain[1 + p.n_hidden] = 32;  // the 12 outputs, padded to one tile
  std::memset(img, 0, sizeof(*img));
  img->p = p;
  img->n_layers = p.n_hidden + 1;
  size_t off = 0;
  int cap[2] = {0, 0};
  for (int i = 0; i <= img->n_layers; ++i) cap[i & 1] = chain[i] > cap[i & 1] ? chain[i] : cap[i & 1];
  for (int l = 0; l < img->n_layers; ++l) {
    img->in[l] = chain[l];
    img->out[l] = chain[l + 1];
    img->woff[l] = (int)off;
    off += (size_t)chain[l] * chain[l + 1];
    img->boff[l] = (int)off;
    off += (size_t)chain[l + 1];
  }
  *n_floats = off;
  *stride0 = cap[0] + pol::ROW_PAD;
  *stride1 = cap[1] + pol::ROW_PAD;
  return true;
}

size_t policy_lds_bytes(int stride0, int stride1) { return sizeof(float) * pol::TILE * (size_t)(stride0 + stride1); }

// The B-operand order of pol::layer: float4 number (tile * K/8 + kb) * 64 + lane holds
// W[tile * 32 + (lane & 31)][8 kb + 4 (lane >> 5) + 0..3]; rows past the real outputs and their biases are 0.
void policy_pack(const PolicyImage& img, const float* const* h_weights, const float* const* h_biases, float* dst) {
  for (int l = 0; l < img.n_layers; ++l) {
    const int K = img.in[l], Np = img.out[l];
    const int N = l + 1 < img.n_layers ? Np : 12;
    float* w = dst + img.woff[l];
    float* bias = dst + img.boff[l];
    const int kblocks = K / 8;
    for (int tile = 0; tile < Np / 32; ++tile)
      for (int kb = 0; kb < kblocks; ++kb)
        for (int lane = 0; lane < 64; ++lane)
          for (int t = 0; t < 4; ++t) {
            const int n = tile * 32 + (lane & 31), k = 8 * kb + 4 * (lane >> 5) + t;
            w[((size_t)(tile * kblocks + kb) * 64 + lane) * 4 + t] = n < N ? h_weights[l][(size_t)n * K + k] : 0.0f;
          }
    for (int n = 0; n < Np; ++n) bias[n] = n < N ? h_biases[l][n] : 0.0f;
  }
}

hipError_t policy_reserve_lds() {
  // the widest admissible network: both buffers [32][512 + pad]
  return hipFuncSetAttribute(reinterpret_cast<const void*>(pol::policy_kernel),
                             hipFuncAttributeMaxDynamicSharedMemorySize,
                             (int)policy_lds_bytes(512 + pol::ROW_PAD, 512 + pol::ROW_PAD));
}

hipError_t launch_policy(const PolicyImage* d_img, const float* d_wts, int stride0, int stride1, const double* sensors,
                         const double* states, const double* plan_in, const double* cmds, int batch, double* slots,
                         const int* type, int want, double* torques, double* outs, void* stream) {
  hipLaunchKernelGGL(pol::policy_kernel, dim3((batch + pol::TILE - 1) / pol::TILE), dim3(pol::THREADS),
                     policy_lds_bytes(stride0, stride1), (hipStream_t)stream, d_img, d_wts, stride0, stride1, sensors,
                     states, plan_in, cmds, batch, slots, type, want, torques, outs);
  return hipGetLastError();
}

}  // namespace mpcqp
