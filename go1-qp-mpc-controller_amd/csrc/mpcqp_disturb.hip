// mpcqp_disturb.hip — the disturbance stage, the first stage of a tick that has the plant and the episode stage:
// per robot it draws this tick's push, the weight of the episode's payload, and the sensor noise with the
// episode's IMU biases (include/mpcqp.h has the statement).  The push and the load go into the wrench row that
// mpcqp_plant_step_wrench_device applies; the noise goes into a second sensor row, written out of place.
//
// The stage keeps no state: every draw is Philox4x32-10 under the key `seed` at the counter (robot, episode,
// stream, index), with the episode index and the episode tick read from the robot's episode slot.
//
// The mapping of mpcqp_plant.hip and mpcqp_episode.hip: one thread per (robot, leg), the four legs of a robot
// are one DPP quad, 16 robots per wave.  The per-episode and per-window draws are computed alike on the four
// lanes (nothing crosses lanes, so a quad always decides together); each lane noises its leg's three joint angles
// and three joint rates, lanes 0..2 one IMU axis each, lane 3 copies the quaternion and the pad; lane k stores
// block k of the wrench row (force 0, point 0, force 1, point 1), leg 0 the output row.  No LDS and no scratch:
// every array is indexed statically and per-lane values are select chains.
//
// Integer and binary64 multiplies and adds with contraction off and no libm call, in the statement order of
// tests/disturb_reference.py: the two agree bitwise.
#include "mpcqp_device.h"

namespace mpcqp {
namespace disturb {

static_assert(MPCQP_DO_BIAS_GYRO + 3 <= MPCQP_DO_SIZE && MPCQP_SN_IMU_ANG_VEL + 3 <= MPCQP_SN_SIZE &&
                  MPCQP_SN_JOINT_POS + 30 == MPCQP_SN_IMU_ANG_VEL + 3 && MPCQP_PW_POINT1 + 3 == MPCQP_PW_SIZE,
              "disturbance layouts");

constexpr double SQRT3 = 1.7320508075688772;  // the Irwin-Hall sum of four has variance 1/3

// Philox4x32-10 (Salmon et al., SC'11), all four output words
__device__ __forceinline__ void philox4(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1,
                                        uint32_t (&w)[4]) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint32_t h0 = __umulhi(0xD2511F53u, c0), l0 = 0xD2511F53u * c0;
    const uint32_t h1 = __umulhi(0xCD9E8D57u, c2), l1 = 0xCD9E8D57u * c2;
    c0 = h1 ^ c1 ^ k0;
    c1 = l1;
    c2 = h0 ^ c3 ^ k1;
    c3 = l0;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  w[0] = c0;
  w[1] = c1;
  w[2] = c2;
  w[3] = c3;
}

// (w + 0.5) 2^-32 in (0, 1) and (w + 0.5) 2^-31 - 1 in (-1, 1); every step is exact
__device__ __forceinline__ double unit(uint32_t w) {
#pragma clang fp contract(off)
  return ((double)w + 0.5) * 0x1p-32;
}
__device__ __forceinline__ double sym(uint32_t w) {
#pragma clang fp contract(off)
  return ((double)w + 0.5) * 0x1p-31 - 1.0;
}

__device__ __forceinline__ double pick(double a0, double a1, double a2, double a3, int leg) {
  return leg == 0 ? a0 : (leg == 1 ? a1 : (leg == 2 ? a2 : a3));
}

// one noisy sensor value: stream 16 + j at index t
__device__ __forceinline__ double noisy(double clean, double bias, double sg, uint32_t b, uint32_t e, int j,
                                        uint32_t t, uint32_t k0, uint32_t k1) {
#pragma clang fp contract(off)
  uint32_t w[4];
  philox4(b, e, 16u + (uint32_t)j, t, k0, k1, w);
  const double z = ((unit(w[0]) + unit(w[1])) + (unit(w[2]) + unit(w[3]))) - 2.0;
  const double d = bias + sg * z;
  return d == 0.0 ? clean : clean + d;  // a zero perturbation leaves the clean value's bits (-0.0 stays -0.0)
}

__global__ __launch_bounds__(256) void disturb_kernel(const mpcqp_disturb_params dp, const mpcqp_disturb_buffers bf,
                                                      const int batch) {
#pragma clang fp contract(off)
  const int gid = blockIdx.x * blockDim.x + threadIdx.x;
  const int b = gid >> 2, leg = gid & 3;
  if (b >= batch) return;  // whole quads leave together
  const double* es = bf.d_episode_state + (size_t)MPCQP_ES_SIZE * b;
  const bool running = es[MPCQP_ES_PHASE] == 1.0;
  const int t = max((int)es[MPCQP_ES_TICK], 0);
  const uint32_t ub = (uint32_t)b, ue = (uint32_t)(int)es[MPCQP_ES_EPISODE], ut = (uint32_t)t;
  const uint32_t k0 = dp.seed[0], k1 = dp.seed[1];

  double f0[3] = {0.0, 0.0, 0.0}, p0[3] = {0.0, 0.0, 0.0}, f1[3] = {0.0, 0.0, 0.0}, p1[3] = {0.0, 0.0, 0.0};
  double ba[3] = {0.0, 0.0, 0.0}, bg[3] = {0.0, 0.0, 0.0};
  double active = 0.0, window = 0.0, mag = 0.0, dir = 0.0, weight = 0.0;
  double pp[3] = {0.0, 0.0, 0.0};  // the window's push point, active or not
  if (running) {
    uint32_t w[4];
    // ---- once per episode: the payload and the IMU biases ----
    philox4(ub, ue, 1u, 0u, k0, k1, w);
    weight = (dp.load_mass_max * unit(w[0])) * dp.gravity;
    f1[2] = 0.0 - weight;
#pragma unroll
    for (int i = 0; i < 3; ++i) p1[i] = dp.load_point[i] * sym(w[i + 1]);
    philox4(ub, ue, 1u, 1u, k0, k1, w);
#pragma unroll
    for (int i = 0; i < 3; ++i) ba[i] = dp.bias_acc * sym(w[i]);
    philox4(ub, ue, 1u, 2u, k0, k1, w);
#pragma unroll
    for (int i = 0; i < 3; ++i) bg[i] = dp.bias_gyro * sym(w[i]);
    // ---- this tick's window: one push, somewhere inside it ----
    if (dp.push_interval > 0 && t >= dp.push_start) {
      const int r = t - dp.push_start;
      const int k = r / dp.push_interval, ph = r - k * dp.push_interval;
      philox4(ub, ue, 2u, (uint32_t)k, k0, k1, w);
      const int jitter = (int)(((uint64_t)w[0] * (uint64_t)(uint32_t)(dp.push_interval - dp.push_duration + 1)) >> 32);
      const int di = (int)(((uint64_t)w[2] * (uint64_t)(uint32_t)dp.dir_count) >> 32);
      mag = dp.push_force[0] + (dp.push_force[1] - dp.push_force[0]) * unit(w[1]);
      window = (double)k;
      dir = (double)di;
      const bool on = jitter <= ph && ph < jitter + dp.push_duration;
      active = on ? 1.0 : 0.0;
      const double* dv = bf.d_dirs + (size_t)4 * di;
      philox4(ub, ue, 3u, (uint32_t)k, k0, k1, w);
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        pp[i] = dp.push_point[i] * sym(w[i]);
        const double fi = mag * dv[i];
        f0[i] = on ? fi : 0.0;
        p0[i] = on ? pp[i] : 0.0;
      }
    }
  }

  // ---- the wrench row: lane k stores block k ----
  {
    double* wr = bf.d_wrench + (size_t)MPCQP_PW_SIZE * b + 3 * leg;
#pragma unroll
    for (int i = 0; i < 3; ++i) wr[i] = pick(f0[i], p0[i], f1[i], p1[i], leg);
  }
  if (bf.d_disturb_out && leg == 0) {
    double* o = bf.d_disturb_out + (size_t)MPCQP_DO_SIZE * b;
    o[MPCQP_DO_PUSH_ACTIVE] = active;
    o[MPCQP_DO_PUSH_WINDOW] = window;
    o[MPCQP_DO_PUSH_FORCE] = mag;
    o[MPCQP_DO_PUSH_DIR] = dir;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      o[MPCQP_DO_PUSH_POINT + i] = pp[i];
      o[MPCQP_DO_LOAD_POINT + i] = p1[i];
      o[MPCQP_DO_BIAS_ACC + i] = ba[i];
      o[MPCQP_DO_BIAS_GYRO + i] = bg[i];
    }
    o[MPCQP_DO_LOAD_FORCE] = weight;
#pragma unroll
    for (int i = MPCQP_DO_BIAS_GYRO + 3; i < MPCQP_DO_SIZE; ++i) o[i] = 0.0;
  }

  // ---- the noisy sensor row, out of place ----
  if (!bf.d_sensors_noisy) return;
  const double* sn = bf.d_sensors + (size_t)MPCQP_SN_SIZE * b;
  double* sy = bf.d_sensors_noisy + (size_t)MPCQP_SN_SIZE * b;
  double qp[3], qv[3], ia = 0.0, ig = 0.0, cp[6];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    qp[i] = sn[MPCQP_SN_JOINT_POS + 3 * leg + i];
    qv[i] = sn[MPCQP_SN_JOINT_VEL + 3 * leg + i];
  }
  if (leg < 3) {
    ia = sn[MPCQP_SN_IMU_ACC + leg];
    ig = sn[MPCQP_SN_IMU_ANG_VEL + leg];
  } else {
#pragma unroll
    for (int i = 0; i < 4; ++i) cp[i] = sn[MPCQP_SN_QUAT + i];
    cp[4] = sn[MPCQP_SN_IMU_ANG_VEL + 3];
    cp[5] = sn[MPCQP_SN_IMU_ANG_VEL + 4];
  }
  if (running) {
    const double sp = dp.sigma[MPCQP_DS_JOINT_POS] * SQRT3, sv = dp.sigma[MPCQP_DS_JOINT_VEL] * SQRT3;
    const double sa = dp.sigma[MPCQP_DS_IMU_ACC] * SQRT3, sg = dp.sigma[MPCQP_DS_IMU_ANG_VEL] * SQRT3;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      qp[i] = noisy(qp[i], 0.0, sp, ub, ue, 3 * leg + i, ut, k0, k1);
      qv[i] = noisy(qv[i], 0.0, sv, ub, ue, 12 + 3 * leg + i, ut, k0, k1);
    }
    if (leg < 3) {
      ia = noisy(ia, pick(ba[0], ba[1], ba[2], 0.0, leg), sa, ub, ue, 24 + leg, ut, k0, k1);
      ig = noisy(ig, pick(bg[0], bg[1], bg[2], 0.0, leg), sg, ub, ue, 27 + leg, ut, k0, k1);
    }
  }
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    sy[MPCQP_SN_JOINT_POS + 3 * leg + i] = qp[i];
    sy[MPCQP_SN_JOINT_VEL + 3 * leg + i] = qv[i];
  }
  if (leg < 3) {
    sy[MPCQP_SN_IMU_ACC + leg] = ia;
    sy[MPCQP_SN_IMU_ANG_VEL + leg] = ig;
  } else {
#pragma unroll
    for (int i = 0; i < 4; ++i) sy[MPCQP_SN_QUAT + i] = cp[i];
    sy[MPCQP_SN_IMU_ANG_VEL + 3] = cp[4];
    sy[MPCQP_SN_IMU_ANG_VEL + 4] = cp[5];
  }
}

}  // namespace disturb

hipError_t launch_disturb(const mpcqp_disturb_params& dp, const mpcqp_disturb_buffers& bf, int batch, void* stream) {
  const int threads = 4 * batch;
  hipLaunchKernelGGL(disturb::disturb_kernel, dim3((threads + 255) / 256), dim3(256), 0, (hipStream_t)stream, dp, bf,
                     batch);
  return hipGetLastError();
}

}  // namespace mpcqp
