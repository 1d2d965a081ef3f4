// mpcqp_episode.hip — the episode stage, the last stage of a tick that ends with the plant: per robot it
// accumulates the episode's metrics, decides when the episode ends, writes the episode into the robot's log
// ring and totals, and restarts the robot over two ticks from a pool row drawn on the device, under a command
// script that restarts with it (include/mpcqp.h has the statement).
//
// The mapping of mpcqp_plant.hip: one thread per (robot, leg), the four legs of a robot are one DPP quad, 16
// robots per wave.  Each lane takes its leg's three joints; sums over the legs move with quad_perm in the fixed
// order (l0 + l1) + (l2 + l3), so the four lanes hold the same bits and a quad always decides together; leg 0
// stores the robot's scalars.  The rare, heavy part of a restart is the zero-fill of the robot's slot rows
// (about 20 KB, the plan slot alone is 940 doubles): the wave ballots which of its robots restart and loops over
// them wave-uniformly, all 64 lanes clearing each row with coalesced 16-byte stores (8-byte ones for a row of an
// odd number of doubles).  No lane leaves early, so the 64 lanes are there for that.  No LDS and no scratch.
//
// Binary64 with contraction off and no libm call, in the statement order of tests/episode_reference.py: the
// two agree bitwise.
#include "mpcqp_device.h"

namespace mpcqp {
namespace episode {

constexpr int RESULT_DOUBLES = (int)(sizeof(mpcqp_result) / sizeof(double));
static_assert(sizeof(mpcqp_result) % 16 == 0, "result rows are cleared with 16-byte stores");
static_assert(MPCQP_ES_METRICS + MPCQP_EM_SIZE <= MPCQP_ES_SIZE && MPCQP_EL_METRICS + MPCQP_EM_SIZE <= MPCQP_EL_SIZE &&
                  MPCQP_ET_REASON + MPCQP_EP_END_COUNT <= MPCQP_ET_SIZE &&
                  MPCQP_EP_POOL_POS_D + 3 <= MPCQP_EP_POOL_SIZE && MPCQP_EP_POOL_EULER_D == MPCQP_PI_SIZE,
              "episode layouts");

__device__ __forceinline__ double quad_sum(double x) {
  const double s = x + dpp<0xB1>(x);
  return s + dpp<0x4E>(s);
}

// A NaN metric is stored as the one quiet NaN 0x7FF8000000000000: IEEE 754 leaves the sign and payload of a NaN
// result open (a - b negates b here, and with it a NaN's sign), and the stored rows are compared bitwise.
__device__ __forceinline__ double canon(double x) { return x != x ? __longlong_as_double(0x7FF8000000000000ll) : x; }

// Philox4x32-10 (Salmon et al., SC'11); the first two output words
__device__ __forceinline__ void philox2(uint32_t c0, uint32_t c1, uint32_t k0, uint32_t k1, uint32_t& w0,
                                        uint32_t& w1) {
  uint32_t c2 = 0u, c3 = 0u;
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
  w0 = c0;
  w1 = c1;
}

// all 64 lanes clear row[0 .. n); n and row are wave-uniform
__device__ __forceinline__ void wave_zero(double* row, int n, int lane) {
  if (n & 1) {
    for (int i = lane; i < n; i += 64) row[i] = 0.0;
  } else {
    double2* r2 = reinterpret_cast<double2*>(row);
    for (int i = lane; i < (n >> 1); i += 64) r2[i] = make_double2(0.0, 0.0);
  }
}

// the script's next segment into the cmd row if it starts at `tick` (leg 0 writes); returns the next segment
__device__ __forceinline__ double segment(const mpcqp_episode_params& ep, const mpcqp_episode_buffers& bf, int b,
                                          int leg, double script, double seg, double tick) {
  if (!bf.d_cmd || !bf.d_scripts) return seg;
  const int sgi = (int)seg;
  if (sgi < 0 || sgi >= ep.script_segments) return seg;
  const int sc = min(max((int)script, 0), ep.script_count - 1);  // (a slot the caller wrote)
  const double* sg = bf.d_scripts + ((size_t)sc * ep.script_segments + sgi) * MPCQP_EP_SEG_SIZE;
  if (!(sg[MPCQP_EP_SEG_TICK] == tick)) return seg;
  if (leg == 0) {
    double* cm = bf.d_cmd + (size_t)MPCQP_CM_SIZE * b;
#pragma unroll
    for (int k = 0; k < 7; ++k) cm[k] = sg[MPCQP_EP_SEG_CMD + k];
  }
  return (double)(sgi + 1);
}

__global__ __launch_bounds__(256) void episode_kernel(const mpcqp_episode_params ep, const mpcqp_episode_buffers bf,
                                                      const int batch, double* slots) {
#pragma clang fp contract(off)
  const int gid = blockIdx.x * blockDim.x + threadIdx.x;
  const int b = gid >> 2, leg = gid & 3, lane = threadIdx.x & 63;
  const bool valid = b < batch;  // whole quads; nobody leaves before the wave-cooperative part
  bool ending = false, priming = false;

  if (valid) {
    double* es = slots + (size_t)MPCQP_ES_SIZE * b;
    double* m = es + MPCQP_ES_METRICS;
    const double* po = bf.d_plant_out + (size_t)MPCQP_PT_SIZE * b;
    const double* pool = ep.pool_count > 0 ? bf.d_pool : nullptr;
    const double roll = po[MPCQP_PT_EULER], pitch = po[MPCQP_PT_EULER + 1], yaw = po[MPCQP_PT_EULER + 2];
    const double tilt2 = roll * roll + pitch * pitch;
    const double x = po[MPCQP_PT_POS], y = po[MPCQP_PT_POS + 1], z = po[MPCQP_PT_POS + 2];
    const double phase = es[MPCQP_ES_PHASE];  // the four lanes read it before leg 0 stores it

    if (phase == 2.0) {
      // ---- priming: the rows are cleared below, by the wave ----
      priming = true;
      const int pi = min(max((int)es[MPCQP_ES_POOL], 0), max(ep.pool_count - 1, 0));  // (a slot the caller wrote)
      const double script = es[MPCQP_ES_SCRIPT];
      if (pool && bf.d_states && leg == 0) {
        double* st = bf.d_states + (size_t)MPCQP_ST_SIZE * b;
        const double* pr = pool + (size_t)MPCQP_EP_POOL_SIZE * pi;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          st[MPCQP_ST_EULER_D + k] = pr[MPCQP_EP_POOL_EULER_D + k];
          st[MPCQP_ST_POS_D + k] = pr[MPCQP_EP_POOL_POS_D + k];
        }
      }
      if (bf.d_est_state && bf.d_states && leg == 0) {
        // the estimator's first tick leaves root_pos and root_lin_vel as they are (A1CtrlStates::reset zeroes them)
        double* st = bf.d_states + (size_t)MPCQP_ST_SIZE * b;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          st[MPCQP_ST_POS + k] = 0.0;
          st[MPCQP_ST_LIN_VEL + k] = 0.0;
        }
      }
      const double seg = segment(ep, bf, b, leg, script, 0.0, 0.0);
      if (leg == 0) {
        es[MPCQP_ES_SEG] = seg;
#pragma unroll
        for (int k = 0; k < MPCQP_EM_SIZE; ++k) m[k] = 0.0;
        m[MPCQP_EM_TILT2_MAX] = canon(tilt2);
        m[MPCQP_EM_Z_MIN] = canon(z);
        m[MPCQP_EM_Z_MAX] = canon(z);
        m[MPCQP_EM_START] = canon(x);
        m[MPCQP_EM_START + 1] = canon(y);
        m[MPCQP_EM_START + 2] = canon(yaw);
        m[MPCQP_EM_END] = canon(x);
        m[MPCQP_EM_END + 1] = canon(y);
        m[MPCQP_EM_END + 2] = canon(yaw);
        es[MPCQP_ES_TICK] = 0.0;
        es[MPCQP_ES_PHASE] = 1.0;
      }
    } else {
      const bool fresh = phase == 0.0;
      const double tick = es[MPCQP_ES_TICK];
      double mm[MPCQP_EM_SIZE];
#pragma unroll
      for (int k = 0; k < MPCQP_EM_SIZE; ++k) mm[k] = m[k];
      if (!fresh) {
        // ---- this tick's metrics, alike on the four lanes ----
        mm[MPCQP_EM_TILT2_MAX] = tilt2 > mm[MPCQP_EM_TILT2_MAX] ? tilt2 : mm[MPCQP_EM_TILT2_MAX];
        mm[MPCQP_EM_Z_MIN] = z < mm[MPCQP_EM_Z_MIN] ? z : mm[MPCQP_EM_Z_MIN];
        mm[MPCQP_EM_Z_MAX] = z > mm[MPCQP_EM_Z_MAX] ? z : mm[MPCQP_EM_Z_MAX];
        if (bf.d_joint_torques) {
          const double* tq = bf.d_joint_torques + (size_t)12 * b + 3 * leg;
          const double t0 = tq[0], t1 = tq[1], t2 = tq[2];
          mm[MPCQP_EM_TAU2] = mm[MPCQP_EM_TAU2] + quad_sum((t0 * t0 + t1 * t1) + t2 * t2);
          if (bf.d_sensors) {
            const double* qd = bf.d_sensors + (size_t)MPCQP_SN_SIZE * b + MPCQP_SN_JOINT_VEL + 3 * leg;
            mm[MPCQP_EM_ENERGY] = mm[MPCQP_EM_ENERGY] + quad_sum((t0 * qd[0] + t1 * qd[1]) + t2 * qd[2]) * ep.dt;
          }
        }
        {
          // body-frame velocity R(quat)' v, R as in Eigen::Quaterniond::toRotationMatrix
          const double qw = po[MPCQP_PT_QUAT], qx = po[MPCQP_PT_QUAT + 1], qy = po[MPCQP_PT_QUAT + 2],
                       qz = po[MPCQP_PT_QUAT + 3];
          const double tx = 2.0 * qx, ty = 2.0 * qy, tz = 2.0 * qz;
          const double twx = tx * qw, twy = ty * qw, twz = tz * qw;
          const double txx = tx * qx, txy = ty * qx, txz = tz * qx;
          const double tyy = ty * qy, tyz = tz * qy, tzz = tz * qz;
          const double r0 = 1.0 - (tyy + tzz), r3 = txy + twz, r6 = txz - twy;
          const double r1 = txy - twz, r4 = 1.0 - (txx + tzz), r7 = tyz + twx;
          const double v0 = po[MPCQP_PT_LIN_VEL], v1 = po[MPCQP_PT_LIN_VEL + 1], v2 = po[MPCQP_PT_LIN_VEL + 2];
          const double vbx = (r0 * v0 + r3 * v1) + r6 * v2;
          const double vby = (r1 * v0 + r4 * v1) + r7 * v2;
          const double wz = po[MPCQP_PT_ANG_VEL + 2];
          double cvx = 0.0, cvy = 0.0, cwz = 0.0;
          if (bf.d_cmd) {
            const double* cm = bf.d_cmd + (size_t)MPCQP_CM_SIZE * b;
            cvx = cm[MPCQP_CM_VEL];
            cvy = cm[MPCQP_CM_VEL + 1];
            cwz = cm[MPCQP_CM_RATE + 2];
          }
          const double ex = vbx - cvx, ey = vby - cvy, ew = wz - cwz;
          mm[MPCQP_EM_ERR_V] = mm[MPCQP_EM_ERR_V] + ex * ex;
          mm[MPCQP_EM_ERR_V + 1] = mm[MPCQP_EM_ERR_V + 1] + ey * ey;
          mm[MPCQP_EM_ERR_V + 2] = mm[MPCQP_EM_ERR_V + 2] + ew * ew;
        }
        if (bf.d_results) {
          const mpcqp_result* r = bf.d_results + b;
          mm[MPCQP_EM_ITERS] = mm[MPCQP_EM_ITERS] + (double)r->iters;
          mm[MPCQP_EM_NOT_SOLVED] = mm[MPCQP_EM_NOT_SOLVED] + (r->status == MPCQP_STATUS_SOLVED ? 0.0 : 1.0);
        }
        const double nc = quad_sum(po[MPCQP_PT_CONTACTS + leg]);
        mm[MPCQP_EM_LOW_CONTACT] = mm[MPCQP_EM_LOW_CONTACT] + (nc < 2.0 ? 1.0 : 0.0);
        mm[MPCQP_EM_END] = x;
        mm[MPCQP_EM_END + 1] = y;
        mm[MPCQP_EM_END + 2] = yaw;
#pragma unroll
        for (int k = 0; k < MPCQP_EM_SIZE; ++k) mm[k] = canon(mm[k]);
      }

      // ---- the end reasons, in their order ----
      int reason = -1;
      {
        const double ps = po[MPCQP_PT_STATUS];
        bool pose_ok = true;
#pragma unroll
        for (int k = MPCQP_PT_POS; k < MPCQP_PT_EULER + 3; ++k) pose_ok = pose_ok && __builtin_isfinite(po[k]);
        const bool env =
            tilt2 > ep.tilt_max * ep.tilt_max || z < ep.height_min || z > ep.height_max || !pose_ok;
        if (fresh) reason = MPCQP_EP_END_FRESH;
        else if (ps == 1.0) reason = MPCQP_EP_END_OUT_OF_REACH;
        else if (ps == 2.0) reason = MPCQP_EP_END_FALLEN;
        else if (ps == 3.0) reason = MPCQP_EP_END_BAD_TORQUE;
        else if (env) reason = MPCQP_EP_END_ENVELOPE;
        else if (tick + 1.0 >= (double)ep.max_ticks) reason = MPCQP_EP_END_TIMEOUT;
      }

      if (reason < 0) {
        // ---- the episode goes on: the next tick's command ----
        const double seg = segment(ep, bf, b, leg, es[MPCQP_ES_SCRIPT], es[MPCQP_ES_SEG], tick + 1.0);
        if (leg == 0) {
#pragma unroll
          for (int k = 0; k < MPCQP_EM_SIZE; ++k) m[k] = mm[k];
          es[MPCQP_ES_SEG] = seg;
          es[MPCQP_ES_TICK] = tick + 1.0;
        }
      } else {
        // ---- the episode ends ----
        ending = true;
        double episode = es[MPCQP_ES_EPISODE];
        double* tot = bf.d_totals ? bf.d_totals + (size_t)MPCQP_ET_SIZE * b : nullptr;
        if (!fresh) {
          const double length = tick + 1.0;
          if (leg == 0) {
            if (bf.d_log) {
              const int at = max((int)episode, 0) % ep.log_len;
              double* row = bf.d_log + ((size_t)ep.log_len * b + at) * MPCQP_EL_SIZE;
              row[MPCQP_EL_EPISODE] = episode;
              row[MPCQP_EL_POOL] = es[MPCQP_ES_POOL];
              row[MPCQP_EL_SCRIPT] = es[MPCQP_ES_SCRIPT];
              row[MPCQP_EL_LENGTH] = length;
              row[MPCQP_EL_REASON] = (double)reason;
#pragma unroll
              for (int k = 0; k < MPCQP_EM_SIZE; ++k) row[MPCQP_EL_METRICS + k] = mm[k];
            }
            if (tot) {
              tot[MPCQP_ET_EPISODES] = tot[MPCQP_ET_EPISODES] + 1.0;
              tot[MPCQP_ET_TICKS] = tot[MPCQP_ET_TICKS] + length;
            }
          }
          episode = episode + 1.0;
        }
        if (tot && leg == 0) tot[MPCQP_ET_REASON + reason] = tot[MPCQP_ET_REASON + reason] + 1.0;
        uint32_t w0, w1;
        philox2((uint32_t)b, (uint32_t)(int)episode, ep.seed[0], ep.seed[1], w0, w1);
        const int pcount = pool ? ep.pool_count : 0, scount = bf.d_scripts ? max(ep.script_count, 0) : 0;
        const int pi = (int)(((uint64_t)w0 * (uint64_t)(uint32_t)pcount) >> 32);
        const int si = (int)(((uint64_t)w1 * (uint64_t)(uint32_t)scount) >> 32);
        if (pool && bf.d_plant_init) {
          // the init part of the pool row, five doubles per lane
          const double* pr = pool + (size_t)MPCQP_EP_POOL_SIZE * pi + MPCQP_EP_POOL_INIT;
          double* in = bf.d_plant_init + (size_t)MPCQP_PI_SIZE * b;
#pragma unroll
          for (int k = 0; k < MPCQP_PI_SIZE / 4; ++k) in[MPCQP_PI_SIZE / 4 * leg + k] = pr[MPCQP_PI_SIZE / 4 * leg + k];
        }
        if (leg == 0) {
#pragma unroll
          for (int k = 0; k < MPCQP_EM_SIZE; ++k) m[k] = mm[k];
          es[MPCQP_ES_EPISODE] = episode;
          es[MPCQP_ES_POOL] = (double)pi;
          es[MPCQP_ES_SCRIPT] = (double)si;
          es[MPCQP_ES_PHASE] = 2.0;
        }
      }
    }
  }

  // ---- the zero-fill, by the whole wave: an ending robot's plant slot and torque row, a priming robot's
  // controller slots, result row and counter.  (The lanes above read their torque and result rows before.)
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  const int rb0 = (gid - lane) >> 2;
  unsigned long long me = __ballot(ending && leg == 0);
  while (me) {
    const int rb = rb0 + ((__ffsll((long long)me) - 1) >> 2);
    me &= me - 1;
    wave_zero(bf.d_plant_state + (size_t)MPCQP_PN_SIZE * rb, MPCQP_PN_SIZE, lane);
    if (bf.d_joint_torques) wave_zero(bf.d_joint_torques + (size_t)12 * rb, 12, lane);
  }
  unsigned long long mp = __ballot(priming && leg == 0);
  while (mp) {
    const int rb = rb0 + ((__ffsll((long long)mp) - 1) >> 2);
    mp &= mp - 1;
    if (bf.d_est_state) wave_zero(bf.d_est_state + (size_t)bf.est_state_size * rb, bf.est_state_size, lane);
    if (bf.d_plan_state) wave_zero(bf.d_plan_state + (size_t)bf.plan_state_size * rb, bf.plan_state_size, lane);
    if (bf.d_cmd_state) wave_zero(bf.d_cmd_state + (size_t)bf.cmd_state_size * rb, bf.cmd_state_size, lane);
    if (bf.d_policy_state)
      wave_zero(bf.d_policy_state + (size_t)bf.policy_state_size * rb, bf.policy_state_size, lane);
    if (bf.d_warm) wave_zero(bf.d_warm + (size_t)bf.warm_size * rb, bf.warm_size, lane);
    if (bf.d_results) wave_zero(reinterpret_cast<double*>(bf.d_results + rb), RESULT_DOUBLES, lane);
    if (bf.d_counter && lane == 0) bf.d_counter[rb] = 0;
  }
}

}  // namespace episode

hipError_t launch_episode(const mpcqp_episode_params& ep, const mpcqp_episode_buffers& bf, int batch, double* slots,
                          void* stream) {
  const int threads = 4 * batch;
  hipLaunchKernelGGL(episode::episode_kernel, dim3((threads + 255) / 256), dim3(256), 0, (hipStream_t)stream, ep, bf,
                     batch, slots);
  return hipGetLastError();
}

}  // namespace mpcqp
