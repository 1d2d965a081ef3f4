// mpcqp_legplan.hip — the upstream leg plan of the control tick, batched on the device:
//   A1RobotControl::update_plan               src/a1_cpp/src/A1RobotControl.cpp:148-202
//   A1RobotControl::generate_swing_legs_ctrl  src/a1_cpp/src/A1RobotControl.cpp:204-287
//   terrain adaptation of compute_grf         src/a1_cpp/src/A1RobotControl.cpp:335-376, :566-582
// in that order, per robot and per tick.  It produces the fields the assemble / solve / torque-map
// kernels consume (contacts, the swing-leg PD force, the terrain-adapted root_euler_d[1]).
//
// One thread per (robot, leg); the four legs of a robot are the four lanes of one DPP quad, 16
// robots per wave (as mpcqp_torque.hip).  The cross-leg values of the terrain fit (the four recent
// contact points) move with quad broadcasts; the fit is then computed by all four lanes alike and
// leg 0 stores it.  The controller's persistent state lives in a per-robot slot (PS_* below): a tick
// reads and writes one ring element per moving-window filter, never a whole ring.
//
// Binary64 with contraction off, in the reference's operation order: everything up to
// foot_pos_recent_contact is bitwise tests/legplan_reference.py.  One stated deviation: the Bezier
// powers t^i, (1-t)^k are repeated multiplications from 1.0, not pow().  The terrain fit takes
// pinv(W'W) from a cyclic Jacobi eigen-decomposition (the reference: Eigen's JacobiSVD,
// Utils.cpp:44-52) and is compared with a conditioning-based tolerance.
#include "mpcqp_device.h"

namespace mpcqp {
namespace lp {

// ---- slot layout (doubles; integers are stored as exact doubles) -----------------------------
constexpr int CW = MPCQP_PLAN_CONTACT_WINDOW, TW = MPCQP_PLAN_TERRAIN_WINDOW;
constexpr int PS_INIT = 0;     // 0.0: fresh reset() controller, gait_counter not loaded yet
constexpr int PS_COUNTER = 1;  // state.counter
constexpr int PS_TFILT = 2;    // terrain_angle_filter: sum, correction, head, count
constexpr int PS_LEG = 8;      // [4] per-leg blocks of PS_LEG_SIZE
constexpr int PL_GC = 0;       //   gait_counter(i)
constexpr int PL_EARLY = 1;    //   early_contacts[i]
constexpr int PL_START = 2;    //   [3] foot_pos_start column i
constexpr int PL_REL_LAST = 5;   // [3] foot_pos_rel_last_time column i
constexpr int PL_TGT_LAST = 8;   // [3] foot_pos_target_last_time column i
constexpr int PL_RECENT = 11;    // [3] foot_pos_recent_contact column i
constexpr int PL_FILT = 14;      // [3] recent_contact_{x,y,z}_filter[i]: sum, correction, head, count
constexpr int PS_LEG_SIZE = 28;  // 26 used
constexpr int PS_RING = PS_LEG + 4 * PS_LEG_SIZE;  // [4][3][CW] rings of the contact filters
constexpr int PS_TRING = PS_RING + 12 * CW;        // [TW] ring of the terrain filter
constexpr int PS_SIZE = (PS_TRING + TW + 3) / 4 * 4;

// MovingWindowFilter::CalculateAverage (utils/filter.hpp:26-62): Neumaier moving sum over a ring.
// f = {sum, correction, head, count}; while the window fills head == count, so the slot written is
// always ring[head] and the value leaving a full window is the one it overwrites.
__device__ __forceinline__ void neumaier(double& sum, double& corr, double value) {
#pragma clang fp contract(off)
  const double new_sum = sum + value;
  if (dabs(sum) >= dabs(value))
    corr += (sum - new_sum) + value;
  else
    corr += (value - new_sum) + sum;
  sum = new_sum;
}
template <int W>
__device__ __forceinline__ double window_average(double* __restrict__ f, double* __restrict__ ring, double value) {
#pragma clang fp contract(off)
  double sum = f[0], corr = f[1];
  const int head = min(max((int)f[2], 0), W - 1), count = (int)f[3];  // in range whatever the slot holds
  if (count >= W) neumaier(sum, corr, -ring[head]);
  neumaier(sum, corr, value);
  ring[head] = value;
  f[0] = sum;
  f[1] = corr;
  f[2] = (double)(head + 1 == W ? 0 : head + 1);
  f[3] = (double)(count < W ? count + 1 : W);
  return (sum + corr) / (double)W;
}

// Per-leg parameters for a per-lane leg: select chains over the wave-uniform kernel arguments.  Each
// element passes through an empty asm first, so the chain stays a chain of values (left alone, the
// optimizer folds it back into one load at a per-lane address, which sends the whole by-value struct
// through scratch memory).
__device__ __forceinline__ double uniform(double v) {
  asm volatile("" : "+s"(v));
  return v;
}
__device__ __forceinline__ double pick4(const double (&a)[4], int leg) {
  const double a0 = uniform(a[0]), a1 = uniform(a[1]), a2 = uniform(a[2]), a3 = uniform(a[3]);
  return leg == 0 ? a0 : (leg == 1 ? a1 : (leg == 2 ? a2 : a3));
}
// element 3*leg + k of a leg-major [4][3] parameter
__device__ __forceinline__ double pick43(const double (&a)[12], int leg, int k) {
  const double a0 = uniform(a[k]), a1 = uniform(a[3 + k]), a2 = uniform(a[6 + k]), a3 = uniform(a[9 + k]);
  return leg == 0 ? a0 : (leg == 1 ? a1 : (leg == 2 ? a2 : a3));
}

// One Jacobi rotation of the symmetric 3x3 in the (p, q) plane; r is the third index.
__device__ __forceinline__ void jacobi_rot(double& app, double& aqq, double& apq, double& arp, double& arq,
                                           double* __restrict__ V, int p, int q) {
#pragma clang fp contract(off)
  if (apq == 0.0) return;
  const double tau = (aqq - app) / (2.0 * apq);
  const double t = (tau >= 0.0 ? 1.0 : -1.0) / (dabs(tau) + sqrt(1.0 + tau * tau));
  const double c = 1.0 / sqrt(1.0 + t * t), s = t * c;
  app = app - t * apq;
  aqq = aqq + t * apq;
  apq = 0.0;
  const double rp = arp, rq = arq;
  arp = c * rp - s * rq;
  arq = s * rp + c * rq;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const double vp = V[3 * k + p], vq = V[3 * k + q];
    V[3 * k + p] = c * vp - s * vq;
    V[3 * k + q] = s * vp + c * vq;
  }
}

constexpr int JACOBI_SWEEPS = 8;  // cyclic Jacobi converges quadratically; 3x3 needs 4-5 sweeps

// a = pinv(A) b for symmetric A = {a00, a01, a02, a11, a12, a22}: A = V diag(w) V', eigenvalues with
// |w| <= eps * 3 * max|w| inverted to 0 (Utils.cpp:46-50).
__device__ __forceinline__ void pinv3_apply(double a00, double a01, double a02, double a11, double a12, double a22,
                                            const double (&b)[3], double (&x)[3]) {
#pragma clang fp contract(off)
  double V[9] = {1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0};
  for (int sweep = 0; sweep < JACOBI_SWEEPS; ++sweep) {
    jacobi_rot(a00, a11, a01, a02, a12, V, 0, 1);
    jacobi_rot(a00, a22, a02, a01, a12, V, 0, 2);
    jacobi_rot(a11, a22, a12, a01, a02, V, 1, 2);
  }
  const double w[3] = {a00, a11, a22};
  const double tol = 2.220446049250313e-16 * 3.0 * dmax(dmax(dabs(w[0]), dabs(w[1])), dabs(w[2]));
  double y[3];
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    const double proj = (V[j] * b[0] + V[3 + j] * b[1]) + V[6 + j] * b[2];
    y[j] = dabs(w[j]) > tol ? proj / w[j] : 0.0;
  }
#pragma unroll
  for (int i = 0; i < 3; ++i) x[i] = (V[3 * i] * y[0] + V[3 * i + 1] * y[1]) + V[3 * i + 2] * y[2];
}

__global__ __launch_bounds__(256) void plan_kernel(const mpcqp_plan_params pp, const double dt,
                                                   double* __restrict__ states, const double* __restrict__ plan_in,
                                                   const int batch, double* __restrict__ slots,
                                                   double* __restrict__ tq, double* __restrict__ out,
                                                   const int* __restrict__ type) {
#pragma clang fp contract(off)
  const int gid = blockIdx.x * blockDim.x + threadIdx.x;
  const int b = gid >> 2, leg = gid & 3;
  if (b >= batch) return;  // whole quads leave together
  double* st = states + (size_t)MPCQP_ST_SIZE * b;
  const double* in = plan_in + (size_t)MPCQP_PL_SIZE * b;
  double* slot = slots + (size_t)PS_SIZE * b;
  double* sl = slot + PS_LEG + PS_LEG_SIZE * leg;
  double* o = out ? out + (size_t)MPCQP_PO_SIZE * b : nullptr;

  // ---- update_plan: gait (:149-165) ----
  const bool fresh = slot[PS_INIT] == 0.0;
  const double gc_init = pick4(pp.gait_counter_init, leg);
  const double speed = pick4(pp.gait_counter_speed, leg);
  const double cps = pp.counter_per_swing;
  double gc = fresh ? gc_init : sl[PL_GC];
  bool plan;
  if (in[MPCQP_PL_MOVEMENT_MODE] == 0.0) {
    plan = true;
    gc = gc_init;  // gait_counter_reset()
  } else {
    gc = fmod(gc + speed, pp.counter_per_gait);
    plan = gc <= cps;
  }
  if (leg == 0) {
    slot[PS_COUNTER] = slot[PS_COUNTER] + 1.0;
    slot[PS_INIT] = 1.0;
  }
  sl[PL_GC] = gc;

  // ---- update_plan: Raibert foothold (:168-201) ----
  double rz[9], R[9];
#pragma unroll
  for (int e = 0; e < 9; ++e) {
    rz[e] = in[MPCQP_PL_ROT_Z + e];
    R[e] = st[MPCQP_ST_ROT + e];
  }
  const double v0 = st[MPCQP_ST_LIN_VEL], v1 = st[MPCQP_ST_LIN_VEL + 1], v2 = st[MPCQP_ST_LIN_VEL + 2];
  const double vd0 = st[MPCQP_ST_LIN_VEL_D], vd1 = st[MPCQP_ST_LIN_VEL_D + 1];
  const double rel0 = (rz[0] * v0 + rz[3] * v1) + rz[6] * v2;  // root_rot_mat_z^T root_lin_vel
  const double rel1 = (rz[1] * v0 + rz[4] * v1) + rz[7] * v2;
  const double kr = sqrt(dabs(pp.default_foot_pos[2]) / 9.8);  // linear index 2: FL's z, for every leg
  const double half_swing = ((cps / speed) * pp.control_dt) / 2.0;
  double dx = kr * (rel0 - vd0) + half_swing * vd0;
  double dy = kr * (rel1 - vd1) + half_swing * vd1;
  if (dx < -pp.foot_delta_x_limit) dx = -pp.foot_delta_x_limit;
  if (dx > pp.foot_delta_x_limit) dx = pp.foot_delta_x_limit;
  if (dy < -pp.foot_delta_y_limit) dy = -pp.foot_delta_y_limit;
  if (dy > pp.foot_delta_y_limit) dy = pp.foot_delta_y_limit;
  double trel[3], tabs[3], tworld[3];
  trel[0] = pick43(pp.default_foot_pos, leg, 0) + dx;
  trel[1] = pick43(pp.default_foot_pos, leg, 1) + dy;
  trel[2] = pick43(pp.default_foot_pos, leg, 2);
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    tabs[k] = (R[3 * k] * trel[0] + R[3 * k + 1] * trel[1]) + R[3 * k + 2] * trel[2];
    tworld[k] = tabs[k] + st[MPCQP_ST_POS + k];
  }

  // ---- generate_swing_legs_ctrl: swing target and PD force (:223-253) ----
  double fabs3[3], cur[3], start[3], tgt[3], fkin[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) fabs3[k] = st[MPCQP_ST_FEET + 3 * leg + k];
#pragma unroll
  for (int k = 0; k < 3; ++k) cur[k] = (rz[k] * fabs3[0] + rz[3 + k] * fabs3[1]) + rz[6 + k] * fabs3[2];
  float spline_time = 0.0f;
  if (gc <= cps) {
#pragma unroll
    for (int k = 0; k < 3; ++k) start[k] = cur[k];  // stance keeps refreshing foot_pos_start
  } else {
#pragma unroll
    for (int k = 0; k < 3; ++k) start[k] = sl[PL_START + k];
    spline_time = (float)(gc - cps) / (float)cps;
  }
  {
    // BezierUtils::get_foot_pos_curve / bezier_curve (Utils.cpp:64-107), pitch argument 0
    const double t = (double)spline_time, u = 1.0 - t;
    double tp[5], up[5];
    tp[0] = 1.0;
    up[0] = 1.0;
#pragma unroll
    for (int i = 1; i < 5; ++i) {
      tp[i] = tp[i - 1] * t;
      up[i] = up[i - 1] * u;
    }
    const double coef[5] = {1.0, 4.0, 6.0, 4.0, 1.0};
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      double P[5] = {start[k], start[k], trel[k], trel[k], trel[k]};
      if (k == 2) {
        P[1] += pp.swing_clearance1;
        P[2] += pp.swing_clearance2;
      }
      double y = 0.0;
#pragma unroll
      for (int i = 0; i < 5; ++i) y += coef[i] * tp[i] * up[4 - i] * P[i];
      tgt[k] = y;
    }
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const double vel_cur = (cur[k] - sl[PL_REL_LAST + k]) / dt;
    const double vel_tgt = (tgt[k] - sl[PL_TGT_LAST + k]) / dt;
    const double pos_err = tgt[k] - cur[k];
    const double vel_err = vel_tgt - vel_cur;
    fkin[k] = pos_err * pick43(pp.kp_foot, leg, k) + vel_err * pick43(pp.kd_foot, leg, k);
    sl[PL_START + k] = start[k];
    sl[PL_REL_LAST + k] = cur[k];
    sl[PL_TGT_LAST + k] = tgt[k];
  }

  // ---- generate_swing_legs_ctrl: early contact, recent contact points (:259-282) ----
  bool early = sl[PL_EARLY] != 0.0;
  if (gc <= cps * 1.5) early = false;
  if (!plan && gc > cps * 1.5 && in[MPCQP_PL_FOOT_FORCE + leg] > pp.foot_force_low) early = true;
  const bool contact = plan || early;
  sl[PL_EARLY] = early ? 1.0 : 0.0;
  double recent[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) recent[k] = sl[PL_RECENT + k];
  if (contact) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      recent[k] = window_average<CW>(sl + PL_FILT + 4 * k, slot + PS_RING + (3 * leg + k) * CW, fabs3[k]);
      sl[PL_RECENT + k] = recent[k];
    }
  }

  // ---- outputs of the two plan functions ----
  const double cflag = contact ? 1.0 : 0.0;
  st[MPCQP_ST_CONTACTS + leg] = cflag;
  if (tq) {
    double* r = tq + (size_t)MPCQP_TQ_SIZE * b;
#pragma unroll
    for (int k = 0; k < 3; ++k) r[MPCQP_TQ_FKIN + 3 * leg + k] = fkin[k];
    r[MPCQP_TQ_CONTACTS + leg] = cflag;
  }
  if (o) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      o[MPCQP_PO_TARGET_REL + 3 * leg + k] = trel[k];
      o[MPCQP_PO_TARGET_ABS + 3 * leg + k] = tabs[k];
      o[MPCQP_PO_TARGET_WORLD + 3 * leg + k] = tworld[k];
      o[MPCQP_PO_FOOT_CUR + 3 * leg + k] = cur[k];
      o[MPCQP_PO_BEZIER + 3 * leg + k] = tgt[k];
      o[MPCQP_PO_FKIN + 3 * leg + k] = fkin[k];
      o[MPCQP_PO_RECENT + 3 * leg + k] = recent[k];
    }
    o[MPCQP_PO_GAIT + leg] = gc;
    o[MPCQP_PO_PLAN + leg] = plan ? 1.0 : 0.0;
    o[MPCQP_PO_EARLY + leg] = early ? 1.0 : 0.0;
    o[MPCQP_PO_CONTACTS + leg] = cflag;
  }

  // ---- compute_grf: terrain adaptation (:335-376) ----
  double coef[3] = {0.0, 0.0, 0.0}, angle_cos = 0.0, angle = 0.0;
  // the reference adapts the terrain only under stance_leg_control_type == 1 (:335): with a type array the
  // branch is per robot, i.e. uniform over the quad its four legs share, which is all the broadcasts need
  if (pp.terrain && (!type || type[b] == 1)) {
    // the four recent contact points, to every lane of the quad (quad_perm broadcasts)
    const double x[4] = {dpp<0x00>(recent[0]), dpp<0x55>(recent[0]), dpp<0xAA>(recent[0]), dpp<0xFF>(recent[0])};
    const double y[4] = {dpp<0x00>(recent[1]), dpp<0x55>(recent[1]), dpp<0xAA>(recent[1]), dpp<0xFF>(recent[1])};
    const double z[4] = {dpp<0x00>(recent[2]), dpp<0x55>(recent[2]), dpp<0xAA>(recent[2]), dpp<0xFF>(recent[2])};
    // compute_walking_surface (:566-582): W = [1, x_i, y_i], a = pinv(W'W) W'z
    double sx = 0.0, sy = 0.0, sxx = 0.0, sxy = 0.0, syy = 0.0, bz[3] = {0.0, 0.0, 0.0};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      sx += x[i];
      sy += y[i];
      sxx += x[i] * x[i];
      sxy += x[i] * y[i];
      syy += y[i] * y[i];
      bz[0] += z[i];
      bz[1] += x[i] * z[i];
      bz[2] += y[i] * z[i];
    }
    pinv3_apply(4.0, sx, sy, sxx, sxy, syy, bz, coef);
    // cal_dihedral_angle((0, 0, 1), (a1, a2, -1)) (Utils.cpp:54-62)
    angle_cos = 1.0 / (1.0 * sqrt((coef[1] * coef[1] + coef[2] * coef[2]) + 1.0));
    const double raw = acos(angle_cos);
    const double f_r_diff = ((z[0] + z[1]) - z[2]) - z[3];
    if (leg == 0) {
      // only record the terrain angle when the body is high (:341)
      if (st[MPCQP_ST_POS + 2] > 0.1) angle = window_average<TW>(slot + PS_TFILT, slot + PS_TRING, raw);
      if (angle > 0.5) angle = 0.5;
      if (angle < -0.5) angle = -0.5;
      if (pp.use_terrain_adapt) st[MPCQP_ST_EULER_D + 1] = f_r_diff > 0.05 ? -angle : angle;
    }
  }
  if (o && leg == 0) {
    o[MPCQP_PO_PLANE] = coef[0];
    o[MPCQP_PO_PLANE + 1] = coef[1];
    o[MPCQP_PO_PLANE + 2] = coef[2];
    o[MPCQP_PO_COS] = angle_cos;
    o[MPCQP_PO_ANGLE] = angle;
  }
}

}  // namespace lp

int plan_state_doubles() { return lp::PS_SIZE; }

hipError_t launch_leg_plan(const mpcqp_plan_params& pp, double dt, double* states, const double* plan_in, int batch,
                           double* slots, double* tq, double* out, const int* type, void* stream) {
  const int threads = 4 * batch;
  hipLaunchKernelGGL(lp::plan_kernel, dim3((threads + 255) / 256), dim3(256), 0, (hipStream_t)stream, pp, dt, states,
                     plan_in, batch, slots, tq, out, type);
  return hipGetLastError();
}

}  // namespace mpcqp
