// mpcqp_estimate.hip — the state front end of the control tick, batched on the device:
//   pose callback    src/a1_cpp/src/GazeboA1ROS.cpp:242-289 (frames :265-269 with Utils::quat_to_euler,
//                    utils/Utils.cpp:7-33; legs :272-285 with legKinematics/A1Kinematics.cpp:39-130)
//   IMU callback     src/a1_cpp/src/GazeboA1ROS.cpp:306
//   A1BasicEKF       init_state / update_estimation, src/a1_cpp/src/A1BasicEKF.cpp:55-164
// in that order, per robot and per tick.  It produces the fields the plan / assemble / solve / torque-map
// kernels consume (root_euler, root_rot_mat, root_ang_vel, root_pos, root_lin_vel, foot_pos_abs,
// root_rot_mat_z, j_foot).
//
// Ordering: the reference runs the estimator after update_plan / generate_swing_legs_ctrl inside
// main_update (GazeboA1ROS.cpp:190-198) while compute_grf reads whatever is latest from a thread of its
// own.  Here the stage runs FIRST in the tick, so the plan and the solve both see this tick's estimate.
//
// Half a wavefront (32 lanes) per robot, two robots per one-wave block; everything a robot's lanes
// exchange goes through that robot's LDS image, ordered by wave_sync (one wave: LDS runs in order), so
// there is no block barrier.  The filter update works on the augmented rows [S | C Pbar | y - C xbar]
// (28 x 47), one row per lane in registers.  C, A and B are selections and differences: S, C Pbar and
// A P A' are formed with adds of P entries read from LDS, never with products against stored matrices.
// S is positive definite (R is), so it is eliminated without pivoting (LDL'): step k broadcasts pivot row
// k through LDS and every row below takes one fused multiply-add per remaining column.  That leaves
// Z = L^-1 [C Pbar | e] and the pivots d; with W = D^-1/2 Z
//   x = xbar + W(:, :18)' W(:, 18),   P = Pbar - W(:, :18)' W(:, :18)
// (the symmetric form; the reference solves twice with fullPivHouseholderQr, A1BasicEKF.cpp:134-139),
// one row of P per lane.  Pbar and S are formed with associations that are symmetric in their two indices,
// so both are exactly symmetric and S needs no transposed pass for the reference's 0.5 (S + S').  Register arrays are indexed statically throughout; global rows and the slot
// move as consecutive doubles on consecutive lanes.
//
// Binary64.  Contraction is off except the explicit fma of the elimination and of W'W: the frames and
// the leg kinematics are the arithmetic of tests/estimator_reference.py operation for operation (ST_ROT
// is bitwise; the rest differs by the device's sin / cos / atan2 / asin).
#include "mpcqp_device.h"

namespace mpcqp {
namespace est {

constexpr int NS = 18, NM = 28;   // STATE_SIZE, MEAS_SIZE (A1BasicEKF.h:14-15)
constexpr int NA = NM + NS + 1;   // columns of the augmented row
constexpr int NW = NS + 1;        // columns of W
// ---- slot layout (doubles) ----
constexpr int ES_INIT = 0;  // 0.0: is_inited() == false
constexpr int ES_X = 4;     // [18] x
constexpr int ES_P = 24;    // [18][18] P, row-major
constexpr int ES_SIZE = ES_P + NS * NS;  // 348
static_assert(ES_SIZE % 4 == 0, "slot padded to a multiple of 4 doubles");

constexpr int CHUNK = 16;  // doubles of the pivot row loaded ahead of their multiply-adds
constexpr int HALF = 32;  // lanes per robot
constexpr int RPB = 2;    // robots per block (one wave)
// offsets inside Lds::so, the image of the MPCQP_ST_* fields the stage writes
constexpr int SO_FEET = 21;  // ST 0..20 (euler, pos, ang_vel, lin_vel, rot) then the 12 feet doubles

struct Lds {
  union {
    double slot[ES_SIZE];        // the slot: old x, P on entry, new on exit ...
    double W[NM * NW];           // ... and W [28][19] in between (P is in Pb by then, old x is used up)
  };
  double Pb[NS * NS];            // Pbar
  double piv[NA + 1];            // the pivot row of the current elimination step
  double sn[MPCQP_SN_SIZE];      // the sensor row
  double pl[MPCQP_PL_SIZE];      // the plan input row
  double prm[32];                // rho_fix [4][5], rho_opt [4][3]
  double so[SO_FEET + 12 + 3];   // outputs to the MPCQP_ST_* row
  double rz[12];                 // root_rot_mat_z
  double jf[36];                 // j_foot blocks, row-major
  double eo[MPCQP_EO_SIZE];      // the optional output row
  double xbar[NS + 2];
  double sc[26];                 // sin, cos of the 12 leg angles (q0, q1, q1 + q2 per leg) and of the yaw
  double cw[4];                  // estimated_contacts
};

__global__ __launch_bounds__(HALF* RPB) void estimate_kernel(const mpcqp_est_params pp, const double dt,
                                                             const double* __restrict__ sensors,
                                                             double* __restrict__ plan_in,
                                                             double* __restrict__ states, const int batch,
                                                             double* __restrict__ slots, double* __restrict__ tq,
                                                             double* __restrict__ out) {
#pragma clang fp contract(off)
  __shared__ Lds lds[RPB];
  const int l = threadIdx.x & (HALF - 1), half = threadIdx.x >> 5;
  const int b = blockIdx.x * RPB + half;
  if (b >= batch) return;  // a whole half-wave leaves; nothing below crosses the halves
  Lds& s = lds[half];
  const double* sn_g = sensors + (size_t)MPCQP_SN_SIZE * b;
  double* pl_g = plan_in + (size_t)MPCQP_PL_SIZE * b;
  double* st_g = states + (size_t)MPCQP_ST_SIZE * b;
  double* slot_g = slots + (size_t)ES_SIZE * b;
  const double qnan = __builtin_nan("");

  // ---- loads: sensor row, plan row, slot, parameters ----
  bool bad;
  {
    const double v0 = sn_g[l];
    s.sn[l] = v0;
    bad = !__builtin_isfinite(v0);
    if (l < 2) {  // 34 used
      const double v1 = sn_g[HALF + l];
      s.sn[HALF + l] = v1;
      bad = bad || !__builtin_isfinite(v1);
    }
  }
  if (l < MPCQP_PL_SIZE) s.pl[l] = pl_g[l];
  for (int e = l; e < ES_SIZE; e += HALF) s.slot[e] = slot_g[e];
  if (l == 0) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
#pragma unroll
      for (int k = 0; k < 5; ++k) s.prm[5 * i + k] = pp.rho_fix[i][k];
#pragma unroll
      for (int k = 0; k < 3; ++k) s.prm[20 + 3 * i + k] = pp.rho_opt[i][k];
    }
  }
  for (int e = MPCQP_EO_CONTACT_W + l; e < MPCQP_EO_SIZE; e += HALF) s.eo[e] = 0.0;  // first tick: weights, det 0
  const unsigned long long ballot = __ballot(bad);
  const bool sensor_bad = ((ballot >> (HALF * half)) & 0xffffffffull) != 0ull;
  wave_sync();

  // ---- a. frames (every lane alike) ----
  double R[9];
  {
    // Eigen::Quaterniond::toRotationMatrix
    const double qw = s.sn[MPCQP_SN_QUAT], qx = s.sn[MPCQP_SN_QUAT + 1], qy = s.sn[MPCQP_SN_QUAT + 2],
                 qz = s.sn[MPCQP_SN_QUAT + 3];
    const double tx = 2.0 * qx, ty = 2.0 * qy, tz = 2.0 * qz;
    const double twx = tx * qw, twy = ty * qw, twz = tz * qw;
    const double txx = tx * qx, txy = ty * qx, txz = tz * qx;
    const double tyy = ty * qy, tyz = tz * qy, tzz = tz * qz;
    R[0] = 1.0 - (tyy + tzz);
    R[1] = txy - twz;
    R[2] = txz + twy;
    R[3] = txy + twz;
    R[4] = 1.0 - (txx + tzz);
    R[5] = tyz - twx;
    R[6] = txz - twy;
    R[7] = tyz + twx;
    R[8] = 1.0 - (txx + tyy);
    // Utils::quat_to_euler (Utils.cpp:7-33): the two atan2 side by side on lanes 0 and 1, asin on lane 2
    {
      const double y_sqr = qy * qy;
      const double t0 = 2.0 * (qw * qx + qy * qz);
      const double t1 = 1.0 - 2.0 * (qx * qx + y_sqr);
      double t2 = 2.0 * (qw * qy - qz * qx);
      t2 = t2 > 1.0 ? 1.0 : t2;
      t2 = t2 < -1.0 ? -1.0 : t2;
      const double t3 = 2.0 * (qw * qz + qx * qy);
      const double t4 = 1.0 - 2.0 * (y_sqr + qz * qz);
      if (l < 2) s.so[MPCQP_ST_EULER + 2 * l] = atan2(l == 0 ? t0 : t3, l == 0 ? t1 : t4);
      if (l == 2) s.so[MPCQP_ST_EULER + 1] = asin(t2);
    }
    wave_sync();
    // every sine and cosine of the tick in one pass: lanes 0..11 the leg angles, lane 12 the yaw
    if (l < 13) {
      double ang = s.so[MPCQP_ST_EULER + 2];
      if (l < 12) {
        ang = s.sn[MPCQP_SN_JOINT_POS + l];
        if (l % 3 == 2) ang = s.sn[MPCQP_SN_JOINT_POS + l - 1] + ang;  // q1 + q2
      }
      s.sc[2 * l] = sin(ang);
      s.sc[2 * l + 1] = cos(ang);
    }
    wave_sync();
    if (l == 0) {
      // Eigen::AngleAxisd(yaw, UnitZ()).toRotationMatrix()
      const double cy = s.sc[25], sy = s.sc[24];
      s.rz[0] = cy;
      s.rz[1] = -sy;
      s.rz[2] = 0.0;
      s.rz[3] = sy;
      s.rz[4] = cy;
      s.rz[5] = 0.0;
      s.rz[6] = 0.0;
      s.rz[7] = 0.0;
      s.rz[8] = (1.0 - cy) + cy;
#pragma unroll
      for (int e = 0; e < 9; ++e) s.so[MPCQP_ST_ROT + e] = R[e];
      // ---- c. root_ang_vel = R imu_ang_vel (GazeboA1ROS.cpp:306) ----
      const double w0 = s.sn[MPCQP_SN_IMU_ANG_VEL], w1 = s.sn[MPCQP_SN_IMU_ANG_VEL + 1],
                   w2 = s.sn[MPCQP_SN_IMU_ANG_VEL + 2];
#pragma unroll
      for (int r = 0; r < 3; ++r) s.so[MPCQP_ST_ANG_VEL + r] = (R[3 * r] * w0 + R[3 * r + 1] * w1) + R[3 * r + 2] * w2;
    }
  }

  // ---- b. legs: lanes 0..3, one leg each ----
  if (l < 4) {
    const int leg = l;
    const double qd[3] = {s.sn[MPCQP_SN_JOINT_VEL + 3 * leg], s.sn[MPCQP_SN_JOINT_VEL + 3 * leg + 1],
                          s.sn[MPCQP_SN_JOINT_VEL + 3 * leg + 2]};
    const double ox = s.prm[5 * leg], oy = s.prm[5 * leg + 1], d = s.prm[5 * leg + 2], lt = s.prm[5 * leg + 3],
                 lc = s.prm[5 * leg + 4];
    const double a0 = s.prm[20 + 3 * leg], a1 = s.prm[20 + 3 * leg + 1], a2 = s.prm[20 + 3 * leg + 2];
    // The leg: hip at (ox, oy, 0) turning about x by q0; the thigh hangs from a point dd along the hip's
    // y axis and swings in the hip's x-z plane by q1, the calf by q1 + q2.  rho_opt shifts the foot along
    // the calf's normal (a0), lengthens the lateral offset (a1) and shortens the calf (a2).
    const double s0 = s.sc[6 * leg], c0 = s.sc[6 * leg + 1], s1 = s.sc[6 * leg + 2], c1 = s.sc[6 * leg + 3];
    const double s12 = s.sc[6 * leg + 4], c12 = s.sc[6 * leg + 5];
    const double dd = d + a1, le = lc - a2;
    const double h2 = le * c12 + a0 * s12;  // the calf's drop below the knee
    const double x2 = a0 * c12 - le * s12;  // and its forward reach
    const double hh = lt * c1 + h2;         // the foot's drop below the hip axis
    const double xx = x2 - lt * s1;         // and its forward reach
    const double py = dd * c0 + hh * s0, pz = dd * s0 - hh * c0;
    const double fk[3] = {ox + xx, oy + py, pz};
    const double J[9] = {0.0, -hh, -h2, hh * c0 - dd * s0, xx * s0, x2 * s0, py, -(xx * c0), -(x2 * c0)};
    double fv[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) fv[r] = (J[3 * r] * qd[0] + J[3 * r + 1] * qd[1]) + J[3 * r + 2] * qd[2];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      s.eo[MPCQP_EO_FOOT_POS_REL + 3 * leg + r] = fk[r];
      s.eo[MPCQP_EO_FOOT_VEL_REL + 3 * leg + r] = fv[r];
      s.so[SO_FEET + 3 * leg + r] = (R[3 * r] * fk[0] + R[3 * r + 1] * fk[1]) + R[3 * r + 2] * fk[2];
      s.eo[MPCQP_EO_FOOT_VEL_ABS + 3 * leg + r] = (R[3 * r] * fv[0] + R[3 * r + 1] * fv[1]) + R[3 * r + 2] * fv[2];
    }
#pragma unroll
    for (int e = 0; e < 9; ++e) s.jf[9 * leg + e] = J[e];
  }
  wave_sync();

  // ---- d. the filter ----
  const bool inited = s.slot[ES_INIT] != 0.0;
  bool fail = sensor_bad;
  bool write_pv = true;
  if (sensor_bad) {
    // nothing: the slot stays untouched
  } else if (!inited) {
    // init_state (A1BasicEKF.cpp:55-68)
    write_pv = false;
    for (int e = l; e < NS * NS; e += HALF) s.slot[ES_P + e] = (e / NS == e % NS) ? pp.init_cov : 0.0;
    if (l < NS) {
      const double x0 = l == 2 ? pp.init_height : 0.0;  // x.segment<3>(0)
      double xv = l < 3 ? x0 : 0.0;
      if (l >= 6) {
        const int r = (l - 6) % 3;
        xv = s.so[SO_FEET + (l - 6)] + (r == 2 ? pp.init_height : 0.0);
      }
      s.slot[ES_X + l] = xv;
      s.eo[MPCQP_EO_X + l] = xv;
      s.eo[MPCQP_EO_DIAG_P + l] = pp.init_cov;
    }
    if (l == 0) s.slot[ES_INIT] = 1.0;
  } else {
    // update_estimation (A1BasicEKF.cpp:70-164)
    const int m = l;                      // measurement row of this lane (m < 28) ...
    const int a = l < NS ? l : NS - 1;    // ... and its state row (l < 18); idle lanes read a valid row
    if (l < 4) {
      double c = 1.0;
      if (s.pl[MPCQP_PL_MOVEMENT_MODE] != 0.0) {
        c = s.pl[MPCQP_PL_FOOT_FORCE + l] / pp.contact_force_scale;
        c = c < 0.0 ? 0.0 : c;   // std::max(c, 0.0)
        c = 1.0 < c ? 1.0 : c;   // std::min(c, 1.0)
      }
      s.cw[l] = c;
      s.eo[MPCQP_EO_CONTACT_W + l] = c;
    }
    wave_sync();
    // xbar = A x + B u, u = R imu_acc + (0, 0, -g)
    {
      const double a0 = s.sn[MPCQP_SN_IMU_ACC], a1 = s.sn[MPCQP_SN_IMU_ACC + 1], a2 = s.sn[MPCQP_SN_IMU_ACC + 2];
      const double u0 = ((R[0] * a0 + R[1] * a1) + R[2] * a2) + 0.0;
      const double u1 = ((R[3] * a0 + R[4] * a1) + R[5] * a2) + 0.0;
      const double u2 = ((R[6] * a0 + R[7] * a1) + R[8] * a2) + (-pp.gravity);
      const double xo = s.slot[ES_X + a];
      double xb = xo;
      if (a < 3) xb = xo + dt * s.slot[ES_X + a + 3];
      else if (a < 6) xb = xo + dt * sel3(a - 3, u0, u1, u2);
      if (l < NS) s.xbar[l] = xb;
    }
    // Pbar = A P A' + Q: row a
    {
      double qd;
      if (a < 3) qd = pp.process_noise_pimu * dt / 20.0;
      else if (a < 6) qd = pp.process_noise_vimu * dt * 9.8 / 20.0;
      else qd = (1.0 + (1.0 - s.cw[(a - 6) / 3]) * 1e3) * dt * pp.process_noise_pfoot;
      // entry (a, c) = P[a][c] + (dt P[a+3][c] + dt P[a][c+3]) + dt^2 P[a+3][c+3], the terms that A has:
      // the same value at (c, a) bit for bit when P is symmetric, so Pbar is exactly symmetric
      const int a3 = a < 3 ? a + 3 : a;
      double Pr[NS], P3[NS];
#pragma unroll
      for (int c = 0; c < NS; ++c) {
        Pr[c] = s.slot[ES_P + NS * a + c];
        P3[c] = s.slot[ES_P + NS * a3 + c];
      }
      if (l < NS) {
#pragma unroll
        for (int c = 0; c < NS; ++c) {
          const double u = a < 3 ? dt * P3[c] : 0.0;
          double v = Pr[c];
          if (c < 3) v = (v + (u + dt * Pr[c + 3])) + (a < 3 ? (dt * dt) * P3[c + 3] : 0.0);
          else v = v + (u + 0.0);
          if (c == a) v = v + qd;
          s.Pb[NS * a + c] = v;
        }
      }
    }
    wave_sync();
    // the augmented row M = [S | C Pbar | y - C xbar] of measurement m
    double M[NA];
    const int mm = m < NM ? m : 0;
    const int leg = mm < 12 ? mm / 3 : (mm < 24 ? (mm - 12) / 3 : mm - 24);
    const int r3 = mm < 24 ? mm % 3 : 2;
    const double cl = s.cw[leg];
    {
      const int ia = mm < 12 ? 6 + mm : (mm < 24 ? 3 + r3 : 8 + 3 * leg);
      // rows ia and (position rows) r3 of Pbar: C's +1 and -1 of this measurement
      double pa[NS], pb[NS];
#pragma unroll
      for (int c = 0; c < NS; ++c) {
        pa[c] = s.Pb[NS * ia + c];
        pb[c] = mm < 12 ? s.Pb[NS * r3 + c] : 0.0;
        M[NM + c] = pa[c] - pb[c];
      }
      const double scale = 1.0 + (1.0 - cl) * 1e3;
      double rd;
      if (mm < 12) rd = scale * pp.sensor_noise_pimu_rel_foot;
      else if (mm < 24) rd = scale * pp.sensor_noise_vimu_rel_foot;
      else rd = pp.assume_flat_ground ? scale * pp.sensor_noise_zfoot : pp.height_noise_no_flat;
#pragma unroll
      for (int n = 0; n < NM; ++n) {
        double v;
        // S[m][n] = (Pbar[am][an] + Pbar[bm][bn]) - (Pbar[bm][an] + Pbar[am][bn]): with Pbar symmetric the
        // same two sums at [n][m], so S is exactly symmetric, which is what the reference's
        // S = 0.5 (S + S') (A1BasicEKF.cpp:131) provides
        if (n < 12) v = (pa[6 + n] + pb[n % 3]) - (pb[6 + n] + pa[n % 3]);
        else if (n < 24) v = M[NM + 3 + n % 3];
        else v = M[NM + 8 + 3 * (n - 24)];
        if (n == mm) v = v + rd;
        M[n] = v;
      }
    }
    {
      // y (A1BasicEKF.cpp:119-128) and yhat = C xbar
      const double fk0 = s.eo[MPCQP_EO_FOOT_POS_REL + 3 * leg], fk1 = s.eo[MPCQP_EO_FOOT_POS_REL + 3 * leg + 1],
                   fk2 = s.eo[MPCQP_EO_FOOT_POS_REL + 3 * leg + 2];
      double y, yhat;
      if (mm < 12) {
        y = s.so[SO_FEET + mm];
        yhat = s.xbar[6 + mm] - s.xbar[r3];
      } else if (mm < 24) {
        const double w0 = s.sn[MPCQP_SN_IMU_ANG_VEL], w1 = s.sn[MPCQP_SN_IMU_ANG_VEL + 1],
                     w2 = s.sn[MPCQP_SN_IMU_ANG_VEL + 2];
        const double lv0 = -s.eo[MPCQP_EO_FOOT_VEL_REL + 3 * leg] - ((-w2) * fk1 + w1 * fk2);
        const double lv1 = -s.eo[MPCQP_EO_FOOT_VEL_REL + 3 * leg + 1] - (w2 * fk0 + (-w0) * fk2);
        const double lv2 = -s.eo[MPCQP_EO_FOOT_VEL_REL + 3 * leg + 2] - ((-w1) * fk0 + w0 * fk1);
        const double r0 = s.so[MPCQP_ST_ROT + 3 * r3], r1 = s.so[MPCQP_ST_ROT + 3 * r3 + 1],
                     r2 = s.so[MPCQP_ST_ROT + 3 * r3 + 2];
        y = (1.0 - cl) * s.slot[ES_X + 3 + r3] + (((cl * r0) * lv0 + (cl * r1) * lv1) + (cl * r2) * lv2);
        yhat = s.xbar[3 + r3];
      } else {
        y = (1.0 - cl) * (s.slot[ES_X + 2] + fk2) + cl * 0.0;
        yhat = s.xbar[8 + 3 * leg];
      }
      M[NA - 1] = y - yhat;
    }
    // LDL' elimination, pivot row through LDS
    double dm = 1.0;
#pragma unroll
    for (int k = 0; k < NM; ++k) {
      if (m == k) {
#pragma unroll
        for (int j = k; j < NA; ++j) s.piv[j] = M[j];
      }
      wave_sync();
      const double dk = s.piv[k];
      if (!(dk > 0.0) || !__builtin_isfinite(dk)) fail = true;
      if (m == k) dm = dk;
      // rows at or above the pivot take a zero multiplier (M + 0 * piv = M), so the step has no branch;
      // the pivot row comes in chunks, all loads of a chunk issued before its first multiply-add
      const double f = (m > k && m < NM) ? -(M[k] / dk) : 0.0;
#pragma unroll
      for (int j0 = k + 1; j0 < NA; j0 += CHUNK) {
        double pr[CHUNK];
#pragma unroll
        for (int j = j0; j < NA && j < j0 + CHUNK; ++j) pr[j - j0] = s.piv[j];
        asm volatile("" ::: "memory");
#pragma unroll
        for (int j = j0; j < NA && j < j0 + CHUNK; ++j) M[j] = __builtin_fma(f, pr[j - j0], M[j]);
      }
      wave_sync();
    }
    // W = D^-1/2 Z
    if (m < NM) {
      const double isd = 1.0 / sqrt(dm);
#pragma unroll
      for (int c = 0; c < NW; ++c) s.W[NW * m + c] = M[NM + c] * isd;
    }
    wave_sync();
    // row a of W'W, then x and P
    double acc[NW];
#pragma unroll
    for (int c = 0; c < NW; ++c) acc[c] = 0.0;
#pragma unroll 1
    for (int i = 0; i < NM; ++i) {
      const double wa = s.W[NW * i + a];
      double wr[NW];
#pragma unroll
      for (int c = 0; c < NW; ++c) wr[c] = s.W[NW * i + c];
      asm volatile("" ::: "memory");  // the row's loads all issue before the first multiply-add waits
#pragma unroll
      for (int c = 0; c < NW; ++c) acc[c] = __builtin_fma(wa, wr[c], acc[c]);
    }
    const double xn = s.xbar[a] + acc[NS];
    double Pn[NS];
#pragma unroll
    for (int c = 0; c < NS; ++c) Pn[c] = 0.5 * ((s.Pb[NS * a + c] - acc[c]) + (s.Pb[NS * c + a] - acc[c]));
    // reduce position drift (A1BasicEKF.cpp:143-147)
    if (l < 2) {
      s.piv[2 * l] = Pn[0];
      s.piv[2 * l + 1] = Pn[1];
    }
    wave_sync();
    const double det = s.piv[0] * s.piv[3] - s.piv[2] * s.piv[1];
    if (det > pp.drift_threshold) {
#pragma unroll
      for (int c = 0; c < NS; ++c) {
        if (a < 2) Pn[c] = c < 2 ? Pn[c] / pp.drift_divisor : 0.0;
        else if (c < 2) Pn[c] = 0.0;
      }
    }
    if (l < NS) {
      double dg = Pn[0];
#pragma unroll
      for (int c = 0; c < NS; ++c) {
        s.slot[ES_P + NS * a + c] = Pn[c];
        dg = c == a ? Pn[c] : dg;
      }
      s.slot[ES_X + a] = xn;
      s.eo[MPCQP_EO_X + a] = xn;
      s.eo[MPCQP_EO_DIAG_P + a] = dg;
      // root_pos = x[0:3], root_lin_vel = x[3:6] (:162-163)
      if (a < 3) s.so[MPCQP_ST_POS + a] = xn;
      else if (a < 6) s.so[MPCQP_ST_LIN_VEL + a - 3] = xn;
    }
    if (l == 0) s.eo[MPCQP_EO_DET] = det;
    // W lay over the slot image: its header and padding again
    if (l < ES_X) s.slot[l] = l == ES_INIT ? 1.0 : 0.0;
    if (l < ES_P - ES_X - NS) s.slot[ES_X + NS + l] = 0.0;
  }
  wave_sync();
  if (fail) {  // robot-uniform: every lane read the same pivots / the same ballot
    for (int e = MPCQP_EO_X + l; e <= MPCQP_EO_DET; e += HALF) s.eo[e] = qnan;
    if (l < 3) {
      s.so[MPCQP_ST_POS + l] = qnan;
      s.so[MPCQP_ST_LIN_VEL + l] = qnan;
    }
    wave_sync();
  }

  // ---- stores: consecutive lanes, consecutive doubles ----
  if (l < SO_FEET) {
    const bool pv = (l >= MPCQP_ST_POS && l < MPCQP_ST_POS + 3) || (l >= MPCQP_ST_LIN_VEL && l < MPCQP_ST_LIN_VEL + 3);
    if (!pv || write_pv) st_g[l] = s.so[l];
  }
  if (l < 12) st_g[MPCQP_ST_FEET + l] = s.so[SO_FEET + l];
  if (l < 9) pl_g[MPCQP_PL_ROT_Z + l] = s.rz[l];
  if (tq) {
    double* tq_g = tq + (size_t)MPCQP_TQ_SIZE * b + MPCQP_TQ_JFOOT;
    tq_g[l] = s.jf[l];
    if (l < 4) tq_g[HALF + l] = s.jf[HALF + l];
  }
  if (out) {
    double* o = out + (size_t)MPCQP_EO_SIZE * b;
    for (int e = l; e < MPCQP_EO_SIZE; e += HALF) o[e] = s.eo[e];
  }
  if (!fail) {
    for (int e = l; e < ES_SIZE; e += HALF) slot_g[e] = s.slot[e];
  }
}

}  // namespace est

int estimator_state_doubles() { return est::ES_SIZE; }

hipError_t launch_state_estimate(const mpcqp_est_params& pp, double dt, const double* sensors, double* plan_in,
                                 double* states, int batch, double* slots, double* tq, double* out, void* stream) {
  hipLaunchKernelGGL(est::estimate_kernel, dim3((batch + est::RPB - 1) / est::RPB), dim3(est::HALF * est::RPB), 0,
                     (hipStream_t)stream, pp, dt, sensors, plan_in, states, batch, slots, tq, out);
  return hipGetLastError();
}

}  // namespace mpcqp
