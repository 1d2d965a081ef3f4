// mpcqp_plant.hip — the plant stage of the control tick: a rigid-body model that turns the tick's joint
// torques back into the next tick's sensor rows, batched on the device, so a fleet closes its loop with
// no host round trip.  The reference closed its loop through Gazebo; this model has no counterpart there.
//
// The model (include/mpcqp.h has the statement): a single rigid trunk, massless stance legs whose held
// feet turn the joint torques into ground reactions f = -R J^-T tau (the inverse of mpcqp_torque.hip's
// tau = J^T (-f_grf)), joint-space swing legs that exert nothing on the trunk, flat ground z = 0,
// semi-implicit Euler in `substeps` substeps per tick; optionally two external forces on the trunk (the wrench
// row of mpcqp_plant_step_wrench_device), and optionally a per-robot inclined ground with its own friction
// coefficient (the terrain row of mpcqp_plant_step_terrain_device), or a bilinear height field: steps, stairs,
// rough ground (the header row and the tile of mpcqp_plant_step_field_device).  A held foot does not slip.  Left
// out: leg mass, the swing legs' reaction on the trunk, foot slip, overhangs, a riser's vertical face as anything
// but one steep cell, trunk-ground contact, joint limits, and impact dynamics beyond zeroing the landing foot's
// velocity.  The joint inertias are the model's own choice, not identified from a robot description.
//
// One thread per (robot, leg); the four legs of a robot are the four lanes of one DPP quad, 16 robots
// per wave (as mpcqp_torque.hip and mpcqp_legplan.hip).  The trunk state is held, and its update is
// computed, alike on the four lanes; the wrench sums move with quad_perm in the fixed order
// (l0 + l1) + (l2 + l3); leg 0 stores the trunk.  No LDS and no scratch: every array is indexed
// statically, and per-leg parameters are select chains over the wave-uniform kernel arguments.
//
// Binary64 with contraction off, in the statement order of tests/plant_reference.py: the two differ only
// by their sin / cos / atan2 / acos / asin / sqrt.
#include "mpcqp_device.h"
#include "mpcqp_lu3.h"

namespace mpcqp {
namespace plant {

using lu3::lu3_solve;

constexpr int SUBSTEPS_MAX = 16;

// Per-leg parameters for a per-lane leg (mpcqp_legplan.hip has the reason for the empty asm).
__device__ __forceinline__ double uniform(double v) {
  asm volatile("" : "+s"(v));
  return v;
}
__device__ __forceinline__ double pick(double a0, double a1, double a2, double a3, int leg) {
  a0 = uniform(a0);
  a1 = uniform(a1);
  a2 = uniform(a2);
  a3 = uniform(a3);
  return leg == 0 ? a0 : (leg == 1 ? a1 : (leg == 2 ? a2 : a3));
}

// (l0 + l1) + (l2 + l3) over the four legs of a robot; every step adds the same two operands on both
// partners, so the four lanes end with the same bits.
__device__ __forceinline__ double quad_sum(double x) {
  const double s = x + dpp<0xB1>(x);
  return s + dpp<0x4E>(s);
}
__device__ __forceinline__ bool quad_any(bool f) {
  int v = f ? 1 : 0;
  v |= __builtin_amdgcn_mov_dpp(v, 0xB1, 0xF, 0xF, true);
  v |= __builtin_amdgcn_mov_dpp(v, 0x4E, 0xF, 0xF, true);
  return v != 0;
}

// The leg of mpcqp_estimate.hip: hip at (ox, oy, 0), lateral offset dd, thigh lt, calf le with the foot
// shifted a0 along its normal; lce and phi are the calf's length and angle to the foot.
struct Leg {
  double ox, oy, dd, lt, le, a0, lce, phi;
};

// Eigen::Quaterniond::toRotationMatrix, the estimator's arithmetic
__device__ __forceinline__ void rotation(const double (&q)[4], double (&R)[9]) {
#pragma clang fp contract(off)
  const double qw = q[0], qx = q[1], qy = q[2], qz = q[3];
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
}
__device__ __forceinline__ void mat_vec(const double (&R)[9], const double (&v)[3], double (&o)[3]) {
#pragma clang fp contract(off)
#pragma unroll
  for (int r = 0; r < 3; ++r) o[r] = (R[3 * r] * v[0] + R[3 * r + 1] * v[1]) + R[3 * r + 2] * v[2];
}
__device__ __forceinline__ void mat_t_vec(const double (&R)[9], const double (&v)[3], double (&o)[3]) {
#pragma clang fp contract(off)
#pragma unroll
  for (int k = 0; k < 3; ++k) o[k] = (R[k] * v[0] + R[3 + k] * v[1]) + R[6 + k] * v[2];
}
__device__ __forceinline__ void cross(const double (&a)[3], const double (&b)[3], double (&o)[3]) {
#pragma clang fp contract(off)
  o[0] = a[1] * b[2] - a[2] * b[1];
  o[1] = a[2] * b[0] - a[0] * b[2];
  o[2] = a[0] * b[1] - a[1] * b[0];
}

// foot position in the body frame and its Jacobian, the estimator's grouping
__device__ __forceinline__ void fk_jac(const Leg& g, const double (&q)[3], double (&p)[3], double (&J)[9]) {
#pragma clang fp contract(off)
  const double s0 = sin(q[0]), c0 = cos(q[0]), s1 = sin(q[1]), c1 = cos(q[1]);
  const double q12 = q[1] + q[2];
  const double s12 = sin(q12), c12 = cos(q12);
  const double h2 = g.le * c12 + g.a0 * s12;
  const double x2 = g.a0 * c12 - g.le * s12;
  const double hh = g.lt * c1 + h2;
  const double xx = x2 - g.lt * s1;
  const double py = g.dd * c0 + hh * s0, pz = g.dd * s0 - hh * c0;
  p[0] = g.ox + xx;
  p[1] = g.oy + py;
  p[2] = pz;
  J[0] = 0.0;
  J[1] = -hh;
  J[2] = -h2;
  J[3] = hh * c0 - g.dd * s0;
  J[4] = xx * s0;
  J[5] = x2 * s0;
  J[6] = py;
  J[7] = -(xx * c0);
  J[8] = -(x2 * c0);
}

// the analytic inverse of fk on the branch foot drop hh >= 0, knee angle negative; false: out of reach
// (a NaN compares false both times)
__device__ __forceinline__ bool ik(const Leg& g, const double (&p)[3], double (&q)[3]) {
#pragma clang fp contract(off)
  const double x = p[0] - g.ox, y = p[1] - g.oy, z = p[2];
  const double arg = (y * y + z * z) - g.dd * g.dd;
  const double hh = sqrt(arg);
  q[0] = atan2(z, y) - atan2(-hh, g.dd);
  const double c = (((x * x + hh * hh) - g.lt * g.lt) - g.lce * g.lce) / ((2.0 * g.lt) * g.lce);
  const double qk = -acos(c);
  q[1] = atan2(-x, hh) - atan2(g.lce * sin(qk), g.lt + g.lce * cos(qk));
  q[2] = qk + g.phi;
  return arg >= 0.0 && dabs(c) <= 1.0;
}

struct State {
  double pos[3], quat[4], v[3], w[3];  // the trunk, alike on the four lanes
  double q[3], qd[3], foot[3];         // this lane's leg
  bool st;                             // its foot is held
};

// Step 1: a stance leg follows its held foot (q from the inverse kinematics, qd from the trunk's motion),
// a swing foot follows its joints.  false: the leg is out of reach.
__device__ __forceinline__ bool kinematics(const Leg& g, State& s, double (&R)[9], double (&p_b)[3],
                                           double (&J)[9]) {
#pragma clang fp contract(off)
  bool ok = true;
  rotation(s.quat, R);
  if (s.st) {
    const double d[3] = {s.foot[0] - s.pos[0], s.foot[1] - s.pos[1], s.foot[2] - s.pos[2]};
    double held[3];
    mat_t_vec(R, d, held);
    ok = ik(g, held, s.q);
  }
  fk_jac(g, s.q, p_b, J);
  if (s.st) {
    double rtv[3], wp[3], rhs[3], A[9];
    mat_t_vec(R, s.v, rtv);
    cross(s.w, p_b, wp);
#pragma unroll
    for (int k = 0; k < 3; ++k) rhs[k] = (-rtv[k]) - wp[k];
#pragma unroll
    for (int e = 0; e < 9; ++e) A[e] = J[e];
    lu3_solve(A, rhs, s.qd);
  } else {
    double rp[3];
    mat_vec(R, p_b, rp);
#pragma unroll
    for (int k = 0; k < 3; ++k) s.foot[k] = s.pos[k] + rp[k];
  }
  return ok;
}

// The ground of a terrain row: {p : n.p = d}, friction mu.  hgt and dot in the grouping of the statement.
struct Ground {
  double n[3], d, mu;
};
__device__ __forceinline__ double dot(const Ground& t, const double (&v)[3]) {
#pragma clang fp contract(off)
  return (t.n[0] * v[0] + t.n[1] * v[1]) + t.n[2] * v[2];
}
__device__ __forceinline__ double hgt(const Ground& t, const double (&p)[3]) {
#pragma clang fp contract(off)
  return dot(t, p) - t.d;
}

// The ground of a height-field header row: the tile H[ny][nx] (x the fast index) with node (i, j) at
// (x0 + i cell, y0 + j cell), friction mu.  The row was checked before this is filled: the tile lies inside the
// heights array.
struct Field {
  double x0, y0, cell, mu;
  int nx, ny;
  const double* H;
};
// The cell index along one axis and the position inside it.  The clamp is on the double, before the conversion:
// whatever u is (NaN and +-inf included) the index lies in [0, n - 2].
__device__ __forceinline__ int field_cell(double u, int n, double& f_raw) {
#pragma clang fp contract(off)
  double c = floor(u);
  c = c > 0.0 ? c : 0.0;  // a NaN ends as 0
  const double hi = (double)(n - 2);
  c = c < hi ? c : hi;
  f_raw = u - c;
  return (int)c;
}
// hgt(p) and the normal n under p, in the grouping of the statement (include/mpcqp.h).  The four corner loads
// are one batch: their addresses depend on p and the header alone.
__device__ __forceinline__ double field_lookup(const Field& fd, const double (&p)[3], double (&n)[3]) {
#pragma clang fp contract(off)
  double fu_raw, fv_raw;
  const int i = field_cell((p[0] - fd.x0) / fd.cell, fd.nx, fu_raw);
  const int j = field_cell((p[1] - fd.y0) / fd.cell, fd.ny, fv_raw);
  const double* c = fd.H + ((size_t)j * fd.nx + i);
  const double h00 = c[0], h10 = c[1], h01 = c[fd.nx], h11 = c[fd.nx + 1];
  const double fu = fmin(fmax(fu_raw, 0.0), 1.0), fv = fmin(fmax(fv_raw, 0.0), 1.0);
  const double d0 = h10 - h00, d1 = h11 - h01;
  const double a = h00 + fu * d0;
  const double b = h01 + fu * d1;
  const double ba = b - a;
  const double h = a + fv * ba;
  const double gx = (fu_raw < 0.0 || fu_raw > 1.0) ? 0.0 : (d0 + fv * (d1 - d0)) / fd.cell;
  const double gy = (fv_raw < 0.0 || fv_raw > 1.0) ? 0.0 : ba / fd.cell;
  const double s = sqrt((gx * gx + gy * gy) + 1.0);
  n[0] = (-gx) / s;
  n[1] = (-gy) / s;
  n[2] = 1.0 / s;
  return (p[2] - h) * n[2];
}

enum : int { FLAT = 0, PLANE = 1, FIELD = 2 };

// WRENCH: the external forces of a wrench row act on the trunk (include/mpcqp.h has the statement).  Without it
// the row is never read, and the instantiation is the kernel as it was before the wrench existed.
// GROUND == PLANE: the ground is the inclined plane of the robot's terrain row, with the row's friction coefficient:
// the four places marked "terrain" below (include/mpcqp.h has the statement).  GROUND == FLAT: neither the table
// nor the episode slot is read, and the instantiation is the kernel as it was before the terrain existed.
// GROUND == FIELD: `terrain` is the table of header rows, and at the same four places every point has the hgt and
// the normal of its own lookup in its tile of `heights`; a held foot's normal is looked up again each substep (the
// foot does not move, so it is the same one).  Without FIELD no header and no height is read.
template <bool WRENCH, int GROUND>
__global__ __launch_bounds__(256) void plant_kernel(const mpcqp_plant_params pp, const double dt,
                                                    const double* __restrict__ torques, const int batch,
                                                    double* __restrict__ slots, const double* __restrict__ init,
                                                    double* __restrict__ sensors, double* __restrict__ plan_in,
                                                    double* __restrict__ states, double* __restrict__ tq,
                                                    double* __restrict__ out, const double* __restrict__ wrench,
                                                    const double* __restrict__ terrain, const int terrain_rows,
                                                    const double* __restrict__ episode_state,
                                                    const double* __restrict__ heights, const int heights_len) {
#pragma clang fp contract(off)
  constexpr bool TERRAIN = GROUND == PLANE;
  const int gid = blockIdx.x * blockDim.x + threadIdx.x;
  const int b = gid >> 2, leg = gid & 3;
  if (b >= batch) return;  // whole quads leave together
  double* slot = slots + (size_t)MPCQP_PN_SIZE * b;
  double* o = out ? out + (size_t)MPCQP_PT_SIZE * b : nullptr;
  // a frozen robot: nothing is written (the four lanes read the same double, so the quad leaves together;
  // they read it before leg 0 stores it below)
  if (slot[MPCQP_PN_STATUS] != 0.0) return;
  double tau[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) tau[k] = torques[(size_t)12 * b + 3 * leg + k];
  bool finite = __builtin_isfinite(tau[0]) && __builtin_isfinite(tau[1]) && __builtin_isfinite(tau[2]);
  // the wrench row, alike on the four lanes: forces F0, F1 (world) at the points P0, P1 (body)
  double F0[3] = {0.0, 0.0, 0.0}, P0[3] = {0.0, 0.0, 0.0}, F1[3] = {0.0, 0.0, 0.0}, P1[3] = {0.0, 0.0, 0.0};
  if constexpr (WRENCH) {
    const double* wr = wrench + (size_t)MPCQP_PW_SIZE * b;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      F0[k] = wr[MPCQP_PW_FORCE0 + k];
      P0[k] = wr[MPCQP_PW_POINT0 + k];
      F1[k] = wr[MPCQP_PW_FORCE1 + k];
      P1[k] = wr[MPCQP_PW_POINT1 + k];
      finite = finite && __builtin_isfinite(F0[k]) && __builtin_isfinite(P0[k]) && __builtin_isfinite(F1[k]) &&
               __builtin_isfinite(P1[k]);
    }
  }
  // the terrain row, alike on the four lanes and read once per tick: the robot's own, or with an episode slot
  // the one of its pool index.  An index outside the table is a non-finite row, and nothing is read there.
  Ground gr = {{0.0, 0.0, 1.0}, 0.0, pp.mu};
  if constexpr (TERRAIN) {
    double idx = (double)b;
    if (episode_state) idx = episode_state[(size_t)MPCQP_ES_SIZE * b + MPCQP_ES_POOL];
    const bool inside = idx > -1.0 && idx < (double)terrain_rows;  // (int) truncates towards zero; a NaN is outside
    finite = finite && inside;
    if (inside) {
      const double* tr = terrain + (size_t)MPCQP_TR_SIZE * (int)idx;
#pragma unroll
      for (int k = 0; k < 3; ++k) gr.n[k] = tr[MPCQP_TR_NORMAL + k];
      gr.d = tr[MPCQP_TR_OFFSET];
      gr.mu = tr[MPCQP_TR_MU];
      finite = finite && __builtin_isfinite(gr.n[0]) && __builtin_isfinite(gr.n[1]) && __builtin_isfinite(gr.n[2]) &&
               __builtin_isfinite(gr.d) && __builtin_isfinite(gr.mu);
    }
  }
  // the header row, chosen as the terrain row is.  A row that is non-finite, or whose tile is degenerate or not
  // inside the heights array, is a non-finite row too: no height is read for it.
  Field fd = {0.0, 0.0, 1.0, pp.mu, 2, 2, heights};
  if constexpr (GROUND == FIELD) {
    double idx = (double)b;
    if (episode_state) idx = episode_state[(size_t)MPCQP_ES_SIZE * b + MPCQP_ES_POOL];
    const bool inside = idx > -1.0 && idx < (double)terrain_rows;
    finite = finite && inside;
    if (inside) {
      const double* hr = terrain + (size_t)MPCQP_HF_SIZE * (int)idx;
      fd.x0 = hr[MPCQP_HF_X0];
      fd.y0 = hr[MPCQP_HF_Y0];
      fd.cell = hr[MPCQP_HF_CELL];
      fd.mu = hr[MPCQP_HF_MU];
      const double nx = hr[MPCQP_HF_NX], ny = hr[MPCQP_HF_NY], off = hr[MPCQP_HF_OFFSET];
      const bool good = __builtin_isfinite(fd.x0) && __builtin_isfinite(fd.y0) && __builtin_isfinite(fd.cell) &&
                        __builtin_isfinite(fd.mu) && __builtin_isfinite(nx) && __builtin_isfinite(ny) &&
                        __builtin_isfinite(off) && fd.cell > 0.0 && nx >= 2.0 && ny >= 2.0 && off >= 0.0 &&
                        off + nx * ny <= (double)heights_len;
      finite = finite && good;
      if (good) {  // (nx, ny >= 2 and nx ny <= heights_len: all three fit an int)
        fd.nx = (int)nx;
        fd.ny = (int)ny;
        fd.H = heights + (size_t)off;
      }
    }
    gr.mu = fd.mu;
  }
  if (quad_any(!finite)) {
    if (o && leg == 0) o[MPCQP_PT_STATUS] = 3.0;
    return;
  }

  Leg g;
  {
    const double d = pick(pp.rho_fix[0][2], pp.rho_fix[1][2], pp.rho_fix[2][2], pp.rho_fix[3][2], leg);
    const double lc = pick(pp.rho_fix[0][4], pp.rho_fix[1][4], pp.rho_fix[2][4], pp.rho_fix[3][4], leg);
    const double a1 = pick(pp.rho_opt[0][1], pp.rho_opt[1][1], pp.rho_opt[2][1], pp.rho_opt[3][1], leg);
    const double a2 = pick(pp.rho_opt[0][2], pp.rho_opt[1][2], pp.rho_opt[2][2], pp.rho_opt[3][2], leg);
    g.ox = pick(pp.rho_fix[0][0], pp.rho_fix[1][0], pp.rho_fix[2][0], pp.rho_fix[3][0], leg);
    g.oy = pick(pp.rho_fix[0][1], pp.rho_fix[1][1], pp.rho_fix[2][1], pp.rho_fix[3][1], leg);
    g.lt = pick(pp.rho_fix[0][3], pp.rho_fix[1][3], pp.rho_fix[2][3], pp.rho_fix[3][3], leg);
    g.a0 = pick(pp.rho_opt[0][0], pp.rho_opt[1][0], pp.rho_opt[2][0], pp.rho_opt[3][0], leg);
    g.dd = d + a1;
    g.le = lc - a2;
    g.lce = sqrt(g.le * g.le + g.a0 * g.a0);
    g.phi = atan2(g.a0, g.le);
  }

  State s;
  double acc[3] = {0.0, 0.0, 0.0}, f[3] = {0.0, 0.0, 0.0};
  double R[9], p_b[3], J[9];
  bool fail = false;
  const bool fresh = slot[MPCQP_PN_INIT] == 0.0;  // robot-uniform
  if (fresh) {
    // ---- initialisation: no integration on this tick ----
    if (init) {
      const double* in = init + (size_t)MPCQP_PI_SIZE * b;
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        s.pos[k] = in[MPCQP_PI_POS + k];
        s.q[k] = in[MPCQP_PI_JOINT_POS + 3 * leg + k];
      }
#pragma unroll
      for (int k = 0; k < 4; ++k) s.quat[k] = in[MPCQP_PI_QUAT + k];
    } else {
#pragma unroll
      for (int k = 0; k < 3; ++k)
        s.q[k] = pick(pp.default_joint_pos[k], pp.default_joint_pos[3 + k], pp.default_joint_pos[6 + k],
                      pp.default_joint_pos[9 + k], leg);
      fk_jac(g, s.q, p_b, J);
      s.pos[0] = 0.0;
      s.pos[1] = 0.0;
      s.pos[2] = -dpp<0x00>(p_b[2]);  // leg 0's foot at z = 0
      s.quat[0] = 1.0;
      s.quat[1] = 0.0;
      s.quat[2] = 0.0;
      s.quat[3] = 0.0;
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      s.v[k] = 0.0;
      s.w[k] = 0.0;
      s.qd[k] = 0.0;
    }
    s.st = false;
    kinematics(g, s, R, p_b, J);  // as a swing leg: the foot from the joints
    if constexpr (GROUND == FIELD) {  // field 1: held iff on or under the surface, and put on it
      double n[3];
      const double hf = field_lookup(fd, s.foot, n);
      s.st = hf <= 0.0;
      if (s.st) {
#pragma unroll
        for (int k = 0; k < 3; ++k) s.foot[k] = s.foot[k] - hf * n[k];
      }
    } else if constexpr (TERRAIN) {  // terrain 1: held iff on or under the plane, and put on it
      const double hf = hgt(gr, s.foot);
      s.st = hf <= 0.0;
      if (s.st) {
#pragma unroll
        for (int k = 0; k < 3; ++k) s.foot[k] = s.foot[k] - hf * gr.n[k];
      }
    } else {
      s.st = s.foot[2] <= 0.0;
      if (s.st) s.foot[2] = 0.0;
    }
  } else {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      s.pos[k] = slot[MPCQP_PN_POS + k];
      s.v[k] = slot[MPCQP_PN_LIN_VEL + k];
      s.w[k] = slot[MPCQP_PN_ANG_VEL + k];
      s.q[k] = slot[MPCQP_PN_JOINT_POS + 3 * leg + k];
      s.qd[k] = slot[MPCQP_PN_JOINT_VEL + 3 * leg + k];
      s.foot[k] = slot[MPCQP_PN_FOOT + 3 * leg + k];
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) s.quat[k] = slot[MPCQP_PN_QUAT + k];
    s.st = slot[MPCQP_PN_CONTACT + leg] != 0.0;

    const int n = min(max(pp.substeps, 1), SUBSTEPS_MAX);
    const double h = dt / (double)n;
#pragma unroll 1
    for (int it = 0; it < n; ++it) {
      // 1.
      fail = !kinematics(g, s, R, p_b, J) || fail;
      // 2. the ground reaction of a massless leg; a leg pulled off the ground lets go
#pragma unroll
      for (int k = 0; k < 3; ++k) f[k] = 0.0;
      if (s.st) {
        double At[9], bt[3], gl[3], fw[3];
#pragma unroll
        for (int i = 0; i < 3; ++i) {
          bt[i] = tau[i];
#pragma unroll
          for (int j = 0; j < 3; ++j) At[3 * i + j] = J[3 * j + i];
        }
        lu3_solve(At, bt, gl);
        mat_vec(R, gl, fw);
        if constexpr (GROUND == FIELD) {  // field 2: terrain 2 with the normal under the held foot
          field_lookup(fd, s.foot, gr.n);
        }
        if constexpr (GROUND != FLAT) {  // terrain 2: the normal part decides, the tangential part is scaled onto the cone
          const double fg[3] = {-fw[0], -fw[1], -fw[2]};
          const double fn = dot(gr, fg);
          if (fn < 0.0) {
            s.st = false;
          } else {
            double t[3];
#pragma unroll
            for (int k = 0; k < 3; ++k) t[k] = fg[k] - fn * gr.n[k];
            const double ft = sqrt((t[0] * t[0] + t[1] * t[1]) + t[2] * t[2]), lim = gr.mu * fn;
            const double sc = ft > lim ? lim / ft : 1.0;
#pragma unroll
            for (int k = 0; k < 3; ++k) f[k] = fn * gr.n[k] + sc * t[k];
          }
        } else {
          const double fz = -fw[2];
          if (fz < 0.0) {
            s.st = false;
          } else {
            const double fx = -fw[0], fy = -fw[1];
            const double ft = sqrt(fx * fx + fy * fy), lim = pp.mu * fz;
            const double sc = ft > lim ? lim / ft : 1.0;
            f[0] = fx * sc;
            f[1] = fy * sc;
            f[2] = fz;
          }
        }
      }
      if (!s.st) {
#pragma unroll
        for (int k = 0; k < 3; ++k)
          s.qd[k] = s.qd[k] + h * (tau[k] - pp.joint_damping[k] * s.qd[k]) / pp.joint_inertia[k];
      }
      // 3. the wrench on the trunk
      double F[3], M[3];
      {
        const double r[3] = {s.foot[0] - s.pos[0], s.foot[1] - s.pos[1], s.foot[2] - s.pos[2]};
        double m[3];
        cross(r, f, m);
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          F[k] = quad_sum(f[k]);
          M[k] = quad_sum(s.st ? m[k] : 0.0);
        }
      }
      double ce[3] = {0.0, 0.0, 0.0};  // the external forces' moment, body frame
      if constexpr (WRENCH) {
        double fb0[3], fb1[3], c0[3], c1[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          // a zero term is skipped, not added: x + 0.0 would turn a sum of -0.0 into +0.0, and a zero row must
          // leave every bit of the kernel without a wrench
          const double fe = F0[k] + F1[k];
          F[k] = fe == 0.0 ? F[k] : F[k] + fe;
        }
        mat_t_vec(R, F0, fb0);
        mat_t_vec(R, F1, fb1);
        cross(P0, fb0, c0);
        cross(P1, fb1, c1);
#pragma unroll
        for (int k = 0; k < 3; ++k) ce[k] = c0[k] + c1[k];
      }
      double a[3], wd[3];
      {
#pragma unroll
        for (int k = 0; k < 3; ++k) a[k] = F[k] / pp.mass;
        a[2] = a[2] + (-pp.gravity);
        double Ib[9], Iw[3], rm[3], wi[3], rhs[3];
#pragma unroll
        for (int e = 0; e < 9; ++e) Ib[e] = pp.inertia[e];
        mat_vec(Ib, s.w, Iw);
        mat_t_vec(R, M, rm);
        if constexpr (WRENCH) {
#pragma unroll
          for (int k = 0; k < 3; ++k) rm[k] = ce[k] == 0.0 ? rm[k] : rm[k] + ce[k];
        }
        cross(s.w, Iw, wi);
#pragma unroll
        for (int k = 0; k < 3; ++k) rhs[k] = rm[k] - wi[k];
        lu3_solve(Ib, rhs, wd);
      }
      // 4. semi-implicit Euler; the quaternion is renormalised
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        s.v[k] = s.v[k] + h * a[k];
        s.w[k] = s.w[k] + h * wd[k];
        s.pos[k] = s.pos[k] + h * s.v[k];
        acc[k] = a[k];
      }
      {
        const double qw = s.quat[0], qx = s.quat[1], qy = s.quat[2], qz = s.quat[3];
        const double w0 = s.w[0], w1 = s.w[1], w2 = s.w[2];
        const double dq[4] = {((-(qx * w0)) - qy * w1) - qz * w2, (qw * w0 + qy * w2) - qz * w1,
                              (qw * w1 + qz * w0) - qx * w2, (qw * w2 + qx * w1) - qy * w0};
        double qn[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) qn[k] = s.quat[k] + (h * 0.5) * dq[k];
        const double nrm = sqrt(((qn[0] * qn[0] + qn[1] * qn[1]) + qn[2] * qn[2]) + qn[3] * qn[3]);
#pragma unroll
        for (int k = 0; k < 4; ++k) s.quat[k] = qn[k] / nrm;
      }
      // 5. swing legs: joints, feet, touchdown
      if (!s.st) {
#pragma unroll
        for (int k = 0; k < 3; ++k) s.q[k] = s.q[k] + h * s.qd[k];
        double R2[9], p2[3], J2[9], rp[3], wp[3], jq[3], u[3];
        rotation(s.quat, R2);
        fk_jac(g, s.q, p2, J2);
        mat_vec(R2, p2, rp);
#pragma unroll
        for (int k = 0; k < 3; ++k) s.foot[k] = s.pos[k] + rp[k];
        cross(s.w, p2, wp);
        mat_vec(J2, s.qd, jq);
#pragma unroll
        for (int k = 0; k < 3; ++k) u[k] = wp[k] + jq[k];
        if constexpr (GROUND != FLAT) {  // terrain 3: lands on or under the ground while moving into it
          double ru[3], fv[3];
          mat_vec(R2, u, ru);
#pragma unroll
          for (int k = 0; k < 3; ++k) fv[k] = s.v[k] + ru[k];
          double hf;
          if constexpr (GROUND == FIELD) {  // field 3: hgt and the normal under the swing foot
            hf = field_lookup(fd, s.foot, gr.n);
          } else {
            hf = hgt(gr, s.foot);
          }
          if (hf <= 0.0 && dot(gr, fv) < 0.0) {
#pragma unroll
            for (int k = 0; k < 3; ++k) s.foot[k] = s.foot[k] - hf * gr.n[k];
            s.st = true;
          }
        } else {
          const double fvz = s.v[2] + ((R2[6] * u[0] + R2[7] * u[1]) + R2[8] * u[2]);
          if (s.foot[2] <= 0.0 && fvz < 0.0) {
            s.foot[2] = 0.0;
            s.st = true;
          }
        }
      }
    }
  }
  // step 1 once more, so the rows are consistent with the state
  fail = !kinematics(g, s, R, p_b, J) || fail;

  if (quad_any(fail)) {
    // a leg out of reach undoes the tick: the status alone is written, and the robot is frozen
    if (leg == 0) {
      slot[MPCQP_PN_STATUS] = 1.0;
      if (o) o[MPCQP_PT_STATUS] = 1.0;
    }
    return;
  }
  double status;
  if constexpr (GROUND == FIELD) {  // field 4: the trunk's height over the ground under it
    double n[3];
    status = field_lookup(fd, s.pos, n) < pp.min_height ? 2.0 : 0.0;
  } else if constexpr (TERRAIN) {  // terrain 4: the trunk's height over the plane
    status = hgt(gr, s.pos) < pp.min_height ? 2.0 : 0.0;
  } else {
    status = s.pos[2] < pp.min_height ? 2.0 : 0.0;
  }

  // ---- stores: each lane its leg, leg 0 the trunk ----
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    slot[MPCQP_PN_JOINT_POS + 3 * leg + k] = s.q[k];
    slot[MPCQP_PN_JOINT_VEL + 3 * leg + k] = s.qd[k];
    slot[MPCQP_PN_FOOT + 3 * leg + k] = s.foot[k];
  }
  const double cflag = s.st ? 1.0 : 0.0;
  slot[MPCQP_PN_CONTACT + leg] = cflag;
  double fa[3];  // foot_pos_abs: world-aligned, body origin
  mat_vec(R, p_b, fa);
  const double ffz = s.st ? f[2] : 0.0;
  if (sensors) {
    double* sn = sensors + (size_t)MPCQP_SN_SIZE * b;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      sn[MPCQP_SN_JOINT_POS + 3 * leg + k] = s.q[k];
      sn[MPCQP_SN_JOINT_VEL + 3 * leg + k] = s.qd[k];
    }
  }
  if (plan_in) plan_in[(size_t)MPCQP_PL_SIZE * b + MPCQP_PL_FOOT_FORCE + leg] = ffz;
  if (states) {
#pragma unroll
    for (int k = 0; k < 3; ++k) states[(size_t)MPCQP_ST_SIZE * b + MPCQP_ST_FEET + 3 * leg + k] = fa[k];
  }
  if (tq) {
#pragma unroll
    for (int e = 0; e < 9; ++e) tq[(size_t)MPCQP_TQ_SIZE * b + MPCQP_TQ_JFOOT + 9 * leg + e] = J[e];
  }
  if (o) {
    o[MPCQP_PT_CONTACTS + leg] = cflag;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      o[MPCQP_PT_GRF + 3 * leg + k] = f[k];
      o[MPCQP_PT_FOOT + 3 * leg + k] = s.foot[k];
    }
  }
  if (leg != 0) return;
  slot[MPCQP_PN_INIT] = 1.0;
  slot[MPCQP_PN_STATUS] = status;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    slot[MPCQP_PN_POS + k] = s.pos[k];
    slot[MPCQP_PN_LIN_VEL + k] = s.v[k];
    slot[MPCQP_PN_ANG_VEL + k] = s.w[k];
    slot[MPCQP_PN_ACC + k] = acc[k];
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) slot[MPCQP_PN_QUAT + k] = s.quat[k];
  // Utils::quat_to_euler (Utils.cpp:7-33), as the estimator
  double euler[3];
  {
    const double qw = s.quat[0], qx = s.quat[1], qy = s.quat[2], qz = s.quat[3];
    const double y_sqr = qy * qy;
    const double t0 = 2.0 * (qw * qx + qy * qz);
    const double t1 = 1.0 - 2.0 * (qx * qx + y_sqr);
    double t2 = 2.0 * (qw * qy - qz * qx);
    t2 = t2 > 1.0 ? 1.0 : t2;
    t2 = t2 < -1.0 ? -1.0 : t2;
    const double t3 = 2.0 * (qw * qz + qx * qy);
    const double t4 = 1.0 - 2.0 * (y_sqr + qz * qz);
    euler[0] = atan2(t0, t1);
    euler[1] = asin(t2);
    euler[2] = atan2(t3, t4);
  }
  if (sensors) {
    double* sn = sensors + (size_t)MPCQP_SN_SIZE * b;
    const double ag[3] = {acc[0] + 0.0, acc[1] + 0.0, acc[2] + pp.gravity};
    double ia[3];
    mat_t_vec(R, ag, ia);  // reads +g at rest (A1BasicEKF.cpp:76)
#pragma unroll
    for (int k = 0; k < 4; ++k) sn[MPCQP_SN_QUAT + k] = s.quat[k];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      sn[MPCQP_SN_IMU_ACC + k] = ia[k];
      sn[MPCQP_SN_IMU_ANG_VEL + k] = s.w[k];
    }
  }
  if (plan_in) {
    // Eigen::AngleAxisd(yaw, UnitZ()).toRotationMatrix(), as the estimator
    double* rz = plan_in + (size_t)MPCQP_PL_SIZE * b + MPCQP_PL_ROT_Z;
    const double cy = cos(euler[2]), sy = sin(euler[2]);
    rz[0] = cy;
    rz[1] = -sy;
    rz[2] = 0.0;
    rz[3] = sy;
    rz[4] = cy;
    rz[5] = 0.0;
    rz[6] = 0.0;
    rz[7] = 0.0;
    rz[8] = (1.0 - cy) + cy;
  }
  if (states) {
    double* st = states + (size_t)MPCQP_ST_SIZE * b;
    double ww[3];
    mat_vec(R, s.w, ww);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      st[MPCQP_ST_EULER + k] = euler[k];
      st[MPCQP_ST_POS + k] = s.pos[k];
      st[MPCQP_ST_ANG_VEL + k] = ww[k];
      st[MPCQP_ST_LIN_VEL + k] = s.v[k];
    }
#pragma unroll
    for (int e = 0; e < 9; ++e) st[MPCQP_ST_ROT + e] = R[e];
  }
  if (o) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      o[MPCQP_PT_POS + k] = s.pos[k];
      o[MPCQP_PT_EULER + k] = euler[k];
      o[MPCQP_PT_LIN_VEL + k] = s.v[k];
      o[MPCQP_PT_ANG_VEL + k] = s.w[k];
      o[MPCQP_PT_ACC + k] = acc[k];
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) o[MPCQP_PT_QUAT + k] = s.quat[k];
    o[MPCQP_PT_STATUS] = status;
  }
}

}  // namespace plant

hipError_t launch_plant(const mpcqp_plant_params& pp, double dt, const double* torques, int batch, double* slots,
                        const double* init, double* sensors, double* plan_in, double* states, double* tq,
                        double* out, void* stream) {
  const int threads = 4 * batch;
  hipLaunchKernelGGL((plant::plant_kernel<false, plant::FLAT>), dim3((threads + 255) / 256), dim3(256), 0,
                     (hipStream_t)stream, pp, dt, torques, batch, slots, init, sensors, plan_in, states, tq, out,
                     (const double*)nullptr, (const double*)nullptr, 0, (const double*)nullptr, (const double*)nullptr,
                     0);
  return hipGetLastError();
}

hipError_t launch_plant_wrench(const mpcqp_plant_params& pp, double dt, const double* torques, const double* wrench,
                               int batch, double* slots, const double* init, double* sensors, double* plan_in,
                               double* states, double* tq, double* out, void* stream) {
  if (!wrench) return launch_plant(pp, dt, torques, batch, slots, init, sensors, plan_in, states, tq, out, stream);
  const int threads = 4 * batch;
  hipLaunchKernelGGL((plant::plant_kernel<true, plant::FLAT>), dim3((threads + 255) / 256), dim3(256), 0,
                     (hipStream_t)stream, pp, dt, torques, batch, slots, init, sensors, plan_in, states, tq, out, wrench,
                     (const double*)nullptr, 0, (const double*)nullptr, (const double*)nullptr, 0);
  return hipGetLastError();
}

hipError_t launch_plant_terrain(const mpcqp_plant_params& pp, double dt, const double* torques, const double* wrench,
                                const double* terrain, int terrain_rows, const double* episode_state, int batch,
                                double* slots, const double* init, double* sensors, double* plan_in, double* states,
                                double* tq, double* out, void* stream) {
  if (!terrain)
    return launch_plant_wrench(pp, dt, torques, wrench, batch, slots, init, sensors, plan_in, states, tq, out, stream);
  const int threads = 4 * batch;
  const dim3 grid((threads + 255) / 256), block(256);
  if (wrench)
    hipLaunchKernelGGL((plant::plant_kernel<true, plant::PLANE>), grid, block, 0, (hipStream_t)stream, pp, dt, torques, batch,
                       slots, init, sensors, plan_in, states, tq, out, wrench, terrain, terrain_rows, episode_state,
                       (const double*)nullptr, 0);
  else
    hipLaunchKernelGGL((plant::plant_kernel<false, plant::PLANE>), grid, block, 0, (hipStream_t)stream, pp, dt, torques, batch,
                       slots, init, sensors, plan_in, states, tq, out, (const double*)nullptr, terrain, terrain_rows,
                       episode_state, (const double*)nullptr, 0);
  return hipGetLastError();
}

hipError_t launch_plant_field(const mpcqp_plant_params& pp, double dt, const double* torques, const double* wrench,
                              const double* field, int field_rows, const double* heights, int heights_len,
                              const double* episode_state, int batch, double* slots, const double* init,
                              double* sensors, double* plan_in, double* states, double* tq, double* out, void* stream) {
  if (!field)
    return launch_plant_wrench(pp, dt, torques, wrench, batch, slots, init, sensors, plan_in, states, tq, out, stream);
  const int threads = 4 * batch;
  const dim3 grid((threads + 255) / 256), block(256);
  if (wrench)
    hipLaunchKernelGGL((plant::plant_kernel<true, plant::FIELD>), grid, block, 0, (hipStream_t)stream, pp, dt, torques,
                       batch, slots, init, sensors, plan_in, states, tq, out, wrench, field, field_rows, episode_state,
                       heights, heights_len);
  else
    hipLaunchKernelGGL((plant::plant_kernel<false, plant::FIELD>), grid, block, 0, (hipStream_t)stream, pp, dt, torques,
                       batch, slots, init, sensors, plan_in, states, tq, out, (const double*)nullptr, field, field_rows,
                       episode_state, heights, heights_len);
  return hipGetLastError();
}

}  // namespace mpcqp
