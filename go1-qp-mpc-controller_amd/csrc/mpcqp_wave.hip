// mpcqp_wave.hip — one WAVEFRONT per robot: the OSQP 0.6 solve of ConvexMpc's QP with the KKT
// system solved through the problem's state-space (LQR) structure, all of it inside one 64-lane
// wave, so that several robots share a CU (the dense path, mpcqp_kernels.hip, runs one workgroup of
// 16 lanes per foot step per robot: 10 waves at N = 10).
//
// Reference path: A1RobotControl::compute_grf (src/a1_cpp/src/A1RobotControl.cpp:446-562) ->
// ConvexMpc (src/a1_cpp/src/ConvexMpc.cpp:7-245) -> OsqpEigen 0.6.3 / OSQP 0.6 (restated in
// oracle/mpc_oracle.c; the phases below follow it: set_rho_vec, update_xz_tilde, update_x/z/y,
// update_info, check_termination, adapt_rho, store_solution).  OSQP scale_data is a kernel of its
// own, launched before this one (scale_kernel, mpcqp_scale.hip); this file reads its image.
//
// KKT structure.  OSQP scales P = c D H D, A~ = E A D (scaling.c), so its reduced KKT matrix is
//   K = P~ + sigma I + A~' diag(rho) A~ = D (c B'Q̄B + R') D,
//   R' = c R + D^-1 (sigma I + A~' diag(rho) A~) D^-1     (3x3 block-diagonal per foot),
// H = B'Q̄B + R being ConvexMpc's condensed Hessian (B = B_qp, ConvexMpc.cpp:184-211).
// (c B'Q̄B + R') u = w is the normal equation of an LQR problem with dynamics
// x_{k+1} = A x_k + B_k u_k, x_0 = 0, state cost cQ and input cost R'_k.  The gravity state never
// moves (x_0 = 0, B row 12 = 0), so the state is 12-dimensional.  Factorization (once per rho):
//   P_N = cQ, G_k = R'_k + B_k'P_{k+1}B_k, K_k = G_k^-1 B_k'P_{k+1}A, Acl_k = A - B_k K_k,
//   P_k = cQ + A'P_{k+1}A - (B_k'P_{k+1}A)'K_k.
// Solve (every ADMM iteration), with a_k = K_k'w_k, b_k = G_k^-1 w_k:
//   backward  s_{N-1} = -a_{N-1},  s_k = Acl_k' s_{k+1} - a_k         (chain of 12x12 mat-vecs)
//   parallel  g_k = b_k + G_k^-1 B_k' s_{k+1},  h_k = B_k g_k
//   forward   x_1 = h_0,  x_{k+1} = Acl_k x_k + h_k                   (chain of 12x12 mat-vecs)
//   parallel  u_k = g_k - K_k x_k.
//
// Lane layout.  A wave is 4 DPP rows of 16 lanes.  Horizon step k lives in DPP row GRAY(k & 3) of
// register "round" k >> 2; inside a row, lane 4l+a holds component a (fx, fy, fz; state triplets
// likewise) of leg l, lane 4l+3 is padding for variables.  A 12x12 mat-vec whose matrix row i sits
// in the lane of output i is 12 `v_fmac_f64_dpp ... row_newbcast:c` (input element c broadcast
// from its lane) — four horizon steps at once, one per row.  Consecutive steps sit in rows one bit
// apart, so a chain hands its vector to the next step with one v_permlane16/32_swap per dword.
// The four lanes of a leg hold the foot's constraint rows: friction-pyramid rows 0-3 (one per
// lane) and row 4 (fz bounds, replicated), so every per-foot ADMM operation (A~x, A~'y, the
// projection) is a quad-perm DPP.  No barrier exists anywhere: the workgroup is the wave.
// Arithmetic is binary64 throughout.
#include "mpcqp_schur.h"
#include "mpcqp_wave_riccati.h"

namespace mpcqp {
namespace wv {

// The LDS image of one robot: the B_w rows, and the setup image recycled as the KKT form's factors.
template <int N, int KS>
struct WSmem {
  using C = Cfg<N>;
  static constexpr bool SACL = N <= ACL_MAXN;
  alignas(16) double Bw[N][3][ND];  // rows 6-8 of B_d(k) = I_w^-1 skew(foot) dt (rows 9-11: dt/m I)
  union U {
    struct Hs {  // setup: record, Ruiz vectors
      double rec[C::REC];
      double D[C::n], Dt[C::n], q[C::n], E[C::m];
      double lam[N][ND];  // gradient adjoint lambda_k (states 0..11)
      double vec[2][16];  // sequential 13-vectors (gradient forward sweep)
      double qn[C::n];     // this tick's gradient (warm start: q of the Ruiz passes is the old one)
    } h;
    // KS = 0: the Riccati factors; KS = 1: the impulse-space Schur form (mpcqp_schur.h)
    typename std::conditional<KS == 0, RicFactors<N, SACL>, SchurLds<N>>::type f;
  } u;
};

// Phase timing (debug builds with -DMPCQP_PHASE_TIMING): lane 0 of each traced robot appends
// {phase id, s_memtime, s_memrealtime (100 MHz), 0} to the trace buffer instead of check records.
#ifdef MPCQP_PHASE_TIMING
// MPCQP_PHASE_TIMING_ENDS: only the first and last marks (0, 20), with the wave's HW_ID register in
// the fourth word, for per-robot durations and the dispatch timeline at no cost to the solve itself
#ifdef MPCQP_PHASE_TIMING_ENDS
#define WV_MARK_ON(id) ((id) == 0 || (id) == 20)
// HW_ID (hwreg 4: wave, SIMD, CU, SE fields) + 2^32 XCC_ID (hwreg 20)
#define WV_HWID()                                                          \
  ((double)(unsigned)__builtin_amdgcn_s_getreg(4 | (0 << 6) | (31 << 11)) + \
   4294967296.0 * (double)(unsigned)__builtin_amdgcn_s_getreg(20 | (0 << 6) | (3 << 11)))
#else
#define WV_MARK_ON(id) true
#define WV_HWID() 0.0
#endif
#define WV_MARK(id) WV_MARK_AT(id, -1)
// cyc >= 0: a cycle count taken earlier (marks recorded in registers inside straight-line code)
#define WV_MARK_AT(id, cyc) WV_MARK_REC(id, cyc, WV_HWID())
#define WV_MARK_REC(id, cyc, w3)                                                        \
  do {                                                                                  \
    if (WV_MARK_ON(id) && trace && threadIdx.x == 0 && inst < trace_cap && nmark < MPCQP_TRACE_LEN) { \
      double* tm_ = trace + ((size_t)inst * MPCQP_TRACE_LEN + nmark) * 4;                \
      tm_[0] = (id);                                                                    \
      tm_[1] = (cyc) >= 0 ? (double)(cyc) : (double)__builtin_readcyclecounter();       \
      tm_[2] = (double)__builtin_amdgcn_s_memrealtime();                                \
      tm_[3] = (w3);                                                                    \
      ++nmark;                                                                          \
    }                                                                                   \
  } while (0)
// A mark inside a phase that has no registers to spare for a record of its own: WV_STAMP takes the
// cycle count in place, and the next mark carries it in its fourth word (WV_MARK_WITH).  The count is
// waited for at once: a scalar load in flight would turn the LDS waits that follow into full drains.
#define WV_STAMP(id, var)                             \
  do {                                                \
    var = (long long)__builtin_readcyclecounter();    \
    asm volatile("s_waitcnt lgkmcnt(0)" : "+s"(var)); \
  } while (0)
#define WV_MARK_WITH(id, var) WV_MARK_REC(id, -1, (double)(var))
#elif defined(MPCQP_ISA_MARKS)
// static ISA accounting (tools/isa_phases.py): an assembly comment per phase mark
#define WV_MARK(id) asm volatile(";WV_MARK %0" ::"n"(id))
// (the Gauss-Jordan's internal marks are recorded after the fact only in timing builds: never here)
#define WV_MARK_AT(id, cyc) \
  do {                      \
    (void)(cyc);            \
    WV_MARK(id);            \
  } while (0)
#define WV_STAMP(id, var) WV_MARK(id)
#define WV_MARK_WITH(id, var) WV_MARK(id)
#else
#define WV_MARK(id) \
  do {              \
  } while (0)
#define WV_MARK_AT(id, cyc) \
  do {                      \
  } while (0)
#define WV_STAMP(id, var) \
  do {                    \
  } while (0)
#define WV_MARK_WITH(id, var) \
  do {                        \
  } while (0)
#endif

// KS: the KKT solve.  0 = Riccati recursion (chains over the horizon, factors on MFMA; every N),
// 1 = impulse-space Schur form (mpcqp_schur.h; N <= 10, nonnegative state weights).
// The solve of robot `inst` by one wave (wave_kernel: one robot per workgroup).  Returns what the
// solve cost (order_cost of its iterations and rho updates, for the launch-order hint's key), with
// WAVE_HANDOFF set when a KS = 1 solve
// hands the robot to the Riccati form without having written anything: scale_kernel
// flagged it (rank-deficient B6_k), a KKT solve cancelled too much for its core (S_max * amp >
// SCHUR_AMP), or a factorization's max S_ii crossed SCHUR_SMAX; wave_kernel then solves it with
// KS = 0 in the same wave.  fb counts the cases: [0] rank-deficient feet, [1] S_max * amp > SCHUR_AMP,
// [2] S_max > SCHUR_SMAX, [3] unused.
constexpr int WAVE_HANDOFF = 1 << 30;
template <int N, int KS>
__device__ __forceinline__ int wave_solve(const int inst, WSmem<N, KS>& sm, const double* __restrict__ recs,
                                           mpcqp_result* __restrict__ results, double* __restrict__ solution,
                                           double* __restrict__ trace, int trace_cap, double* __restrict__ wstate,
                                           double* __restrict__ img, const mpcqp_params& p,
                                           int* __restrict__ fb) {
  using C = Cfg<N>;
  using WL = WarmLayout<N>;
  constexpr int n = C::n, m = C::m, R = C::R;
  const int t = threadIdx.x;
  const int q = t >> 4, li = t & 15, leg = li >> 2, a = li & 3;
  const bool av = a < 3;
  const int idx = 3 * leg + (av ? a : 2);  // index inside a step (padding lanes alias component 2)
  const int ig = gray(q);                  // this lane's step in round r is 4r + ig
  const double alpha = p.alpha, sigma = p.sigma;
  int nmark = 0;
  (void)nmark;
  // the phase marks of code that lives in the two forms' headers
  auto mark = [&](int id, long long cyc = -1) __attribute__((always_inline)) {
    WV_MARK_AT(id, cyc);
    (void)id;
    (void)cyc;
  };
  WV_MARK(0);

  // ---- 0. record -> LDS, non-finite guard -------------------------------------------------------
  auto& HS = sm.u.h;
  {
    const double* rg = recs + (size_t)inst * C::REC;
    bool bad = false;
    for (int e = t; e < C::REC; e += NT) {
      const double v = rg[e];
      HS.rec[e] = v;
      bad |= !isfinite(v);
    }
    if (__ballot(bad) != 0) {
      if (t == 0) results[inst] = osqp::nan_input_result(p);
      if (solution)
        for (int e = t; e < n; e += NT) solution[(size_t)inst * n + e] = NAN;
      return 0;
    }
  }
  wave_sync();
  WV_MARK(1);
  const double* rec = HS.rec;
  // (record values used after the setup image is recycled are plain register copies: every LDS
  // store of the union aliases them under -fno-strict-aliasing, so no reload can be hoisted past
  // the factorization's stores — see DESIGN §5, "LDS unions and aliasing")
  const double dt = rec[MPCQP_REC_DT], mass = rec[MPCQP_REC_MASS], mu_rec = rec[MPCQP_REC_MU];
  Adisc A;
  {
    const double yaw = rec[MPCQP_REC_EULER + 2];
    A.ad0 = cos(yaw) * dt;
    A.ad1 = sin(yaw) * dt;
    A.dt = dt;
  }
  const double dtm = (1.0 / mass) * dt;
  // what the solve needs from the record after the setup image is recycled (root_rot_mat is read
  // again from HBM by the epilogue)
  const double cont = rec[MPCQP_REC_CONTACTS + leg] != 0.0 ? 1.0 : 0.0;
  const double fzmin = rec[MPCQP_REC_FZMIN], fzmax = rec[MPCQP_REC_FZMAX];

  // ---- 1. B_d(k) rows 6-8 (calculate_B_mat_c, Utils.cpp:35-41), gradient adjoint --------------------
  {
    double Iwinv[9];
    iw_inverse(rec, Iwinv);
    for (int e = t; e < N * 36; e += NT) {
      const int k = e / 36, rr = (e / 12) % 3, cc = e % 12;
      const int lg = cc / 3, c3 = cc % 3;
      const double* fp = rec + MPCQP_REC_FEET(N) + 12 * k + 3 * lg;
      const double sk0 = c3 == 0 ? 0.0 : c3 == 1 ? -fp[2] : fp[1];
      const double sk1 = c3 == 0 ? fp[2] : c3 == 1 ? 0.0 : -fp[0];
      const double sk2 = c3 == 0 ? -fp[1] : c3 == 1 ? fp[0] : 0.0;
      double s = 0.0;
      s += sel3(rr, Iwinv[0], Iwinv[3], Iwinv[6]) * sk0;
      s += sel3(rr, Iwinv[1], Iwinv[4], Iwinv[7]) * sk1;
      s += sel3(rr, Iwinv[2], Iwinv[5], Iwinv[8]) * sk2;
      sm.Bw[k][rr][cc] = s * dt;
    }
  }
  WV_MARK(2);

  WV_MARK(3);

  // ---- 3. OSQP scale_data: the image scale_kernel wrote (D, E, q~, c, branch; raw q if warm) -------
  using SI = ScaleImg<N>;
  // (not const: the Schur form records max S_ii of its latest factorization in the DEGEN slot)
  double* const im = img + (size_t)inst * SI::SIZE;
  const double c_s = im[SI::CS];
  const int mode = (int)im[SI::MODE];  // 0 cold, 1 osqp_update_P, 2 OsqpEigen re-init
  if (KS == 1 && im[SI::DEGEN] != 0.0) {
    // rank-deficient B6_k (collinear / coincident feet: G_k would be singular; the reference QP is
    // still strictly convex, R > 0): the Riccati form (KS = 0) solves this robot.  Nothing of it
    // has been written yet.
    if (t == 0) atomicAdd(fb, 1);
    return WAVE_HANDOFF;
  }
  for (int j = t; j < n; j += NT) {
    HS.D[j] = im[SI::D + j];
    HS.q[j] = im[SI::Q + j];
    if (mode != 0) HS.qn[j] = im[SI::QN + j];
  }
  for (int r = t; r < m; r += NT) HS.E[r] = im[SI::E + r];
  // Warm start (A1RobotControl.h:67 member solver, :522-538): the slot of the previous tick.
  double* const ws = wstate ? wstate + (size_t)inst * WL::SIZE : nullptr;
  // The unscaled constraint entries of row ri (ConvexMpc.cpp:46-58), as scale_kernel used them:
  // [0] on fx (rows 0, 1) / fy (rows 2, 3), [1] on fz.  Set once per solver init (friction pyramid
  // of this tick's mu); osqp_update_P keeps the previous A: unscale_data of the previous A~ with the
  // previous scaling (the same expressions as scale_kernel's, so the same bits).
  auto ap_of = [&](int ri, int which) __attribute__((always_inline)) -> double {
    const int f = ri / 5, k5 = ri % 5;
    if (mode == 1) {
      const double ei = 1. / ws[WL::E + ri];
      if (which == 0) return k5 < 4 ? (ws[WL::AK + ri] * ei) * (1. / ws[WL::D + 3 * f + (k5 >> 1)]) : 0.0;
      return (ws[WL::AK + m + ri] * ei) * (1. / ws[WL::D + 3 * f + 2]);
    }
    if (which == 0) return k5 < 4 ? 1.0 : 0.0;
    return k5 < 4 ? ((k5 & 1) ? -mu_rec : mu_rec) : 1.0;
  };
  wave_sync();
  const double cost_c = c_s, cinv = 1. / c_s;
  WV_MARK(4);

  // ---- 4. lane registers: variables (D, q~) and rows (E, A~, bounds, rho) — set_rho_vec -----------
  // update_P keeps the adapted rho (settings->rho); setup and re-init start from the settings'
  const double rho0 = mode == 1 ? ws[WL::RHO] : dmin(dmax(p.rho, RHO_MIN), RHO_MAX);
  // Dv, Ev, E4 are setup-only arrays: the loop reads D and E from the image again when it needs
  // them (factorizations, termination checks, the epilogue) instead of holding them in registers
  double X[R], Qv[R], Dv[R], DI[R], PX[R], RHS[R];
  double Z[R], Y[R], Ev[R], AK0[R], AK1[R];
  double Z4[R], Y4[R], E4[R], L4[R], U4[R], AK4[R], RHO4[R];
  bool kvr[R], vvr[R];
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const int k = 4 * r + ig;
    const bool kv = k < N, vv = kv && av;
    kvr[r] = kv;
    vvr[r] = vv;
    const int kc = kv ? k : 0;
    const int ci = ND * kc + idx, ri = CD * kc + 5 * leg + a, r4 = CD * kc + 5 * leg + 4;
    const int cf = ND * kc + 3 * leg;  // the leg's three variables
    Dv[r] = vv ? HS.D[ci] : 1.0;
    DI[r] = 1. / Dv[r];
    // warm ticks end with osqp_update_lin_cost (A1RobotControl.cpp:533, after updateHessianMatrix's
    // update_P or re-init): q~ = c (D q) of this tick's gradient; a cold setup scales q pass by pass
    Qv[r] = vv ? (mode != 0 ? (HS.qn[ci] * Dv[r]) * c_s : HS.q[ci]) : 0.0;
    Ev[r] = kv ? HS.E[ri] : 1.0;
    E4[r] = kv ? HS.E[r4] : 1.0;
    // A~ = E A D: row a < 4 has A on fx (a < 2) / fy (a >= 2) and on fz; row 4 on fz
    AK0[r] = kv ? (ap_of(ri, 0) * Ev[r]) * HS.D[cf + (a >> 1)] : 0.0;
    AK1[r] = kv ? (ap_of(ri, 1) * Ev[r]) * HS.D[cf + 2] : 0.0;
    AK4[r] = kv ? (ap_of(r4, 1) * E4[r]) * HS.D[cf + 2] : 0.0;
    // bounds (ConvexMpc.cpp:223-245), clipped to +-OSQP_INFTY, scaled by E
    double l4 = fzmin * cont, u4 = fzmax * cont;
    l4 = dmin(dmax(l4, -OSQP_INF), OSQP_INF);
    u4 = dmin(dmax(u4, -OSQP_INF), OSQP_INF);
    L4[r] = E4[r] * l4;
    U4[r] = E4[r] * u4;
    X[r] = 0.0; PX[r] = 0.0;
    Z[r] = 0.0; Y[r] = 0.0; Z4[r] = 0.0; Y4[r] = 0.0;
    RHS[r] = vv ? sigma * 0.0 - Qv[r] : 0.0;  // cold start: compute_rhs with x = z = y = 0
    if (mode == 1) {  // warm start: the previous scaled iterates as they are
      X[r] = vv ? ws[WL::X + ci] : 0.0;
      Z[r] = kv ? ws[WL::Z + ri] : 0.0;
      Y[r] = kv ? ws[WL::Y + ri] : 0.0;
      Z4[r] = kv ? ws[WL::Z + r4] : 0.0;
      Y4[r] = kv ? ws[WL::Y + r4] : 0.0;
    } else if (mode == 2) {  // re-init: x = D^-1 (D_old x_old), y = c E^-1 ((E_old y_old) c_old^-1)
      const double cinv_o = 1. / ws[WL::C];
      X[r] = vv ? DI[r] * (ws[WL::D + ci] * ws[WL::X + ci]) : 0.0;
      Y[r] = kv ? c_s * ((1. / Ev[r]) * ((ws[WL::E + ri] * ws[WL::Y + ri]) * cinv_o)) : 0.0;
      Y4[r] = kv ? c_s * ((1. / E4[r]) * ((ws[WL::E + r4] * ws[WL::Y + r4]) * cinv_o)) : 0.0;
    }
  }
  if (mode == 2) {  // z = A~ x
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const double xp = dpp<QP_PRIM>(X[r]), xz = dpp<QP_B2>(X[r]);
      Z[r] = AK0[r] * xp + AK1[r] * xz;
      Z4[r] = AK4[r] * xz;
    }
  }
  // osqp::rho_of_row(osqp::row_kind(l4, u4), rho), written out: through the int row class the
  // compiler schedules the setup differently (rows 0-3 are always inequalities: rho itself)
  auto rho4_of = [&](double l4, double u4, double rho) __attribute__((always_inline)) {
    const bool loose = l4 < -OSQP_INF * MIN_SCALING && u4 > OSQP_INF * MIN_SCALING;
    const bool eq = u4 - l4 < RHO_TOL;
    return loose ? RHO_MIN : (eq ? RHO_EQ_OVER_RHO_INEQ * rho : rho);
  };
  double RI4[R];  // 1 / rho of row 4 (OSQP rho_inv_vec), refreshed with rho
#pragma unroll
  for (int r = 0; r < R; ++r) {
    RHO4[r] = rho4_of(L4[r], U4[r], rho0);
    RI4[r] = 1. / RHO4[r];
  }
  if (mode != 0) {
#pragma unroll
    for (int r = 0; r < R; ++r) {
      // compute_rhs from the warm x, z, y: sigma x - q~ + A~'(rho z - y)
      const double at = quad_at(rho0 * Z[r] - Y[r], RHO4[r] * Z4[r] - Y4[r], AK0[r], AK1[r], AK4[r], a);
      RHS[r] = vvr[r] ? (sigma * X[r] - Qv[r]) + at : 0.0;
    }
  }
  // Row 4 of every foot (the fz bounds row; its values are the same on the foot's four lanes) packed
  // four register rounds to a register: lane a of a foot's quad holds round 4p + a's value in P[p].
  // The ADMM update projects row 4 once per packed register instead of once per round, and the loop
  // carries 7 NP doubles for it instead of 7 R (NP = 1 at N <= 12): fewer registers for the
  // allocator to park in AGPRs.  unpack(P, r) is round r's value on all four lanes (a quad
  // broadcast), bitwise the value the per-round arrays held.
  constexpr int NP = (R + 3) / 4;
  auto unpack = [&](const double (&P)[NP], int r) __attribute__((always_inline)) -> double {
    const double v = P[r >> 2];
    switch (r & 3) {
      case 0: return dpp<QP_B0>(v);
      case 1: return dpp<QP_B1>(v);
      case 2: return dpp<QP_B2>(v);
      default: return dpp<QP_B3>(v);
    }
  };
  auto pack_of = [&](auto get, int pr) __attribute__((always_inline)) -> double {
    const int r0 = 4 * pr, rl = R - 1;
    const double v0 = get(r0 < rl ? r0 : rl), v1 = get(r0 + 1 < rl ? r0 + 1 : rl);
    const double v2 = get(r0 + 2 < rl ? r0 + 2 : rl), v3 = get(r0 + 3 < rl ? r0 + 3 : rl);
    return a == 0 ? v0 : (a == 1 ? v1 : (a == 2 ? v2 : v3));
  };
  // (the setup's operands through a register copy: a select among loads of one local array is
  // otherwise folded into one load at a per-lane address, which keeps the array in scratch memory)
  auto reg = [](double v) __attribute__((always_inline)) {
    asm("" : "+v"(v));
    return v;
  };
  double Z4P[NP], Y4P[NP], L4P[NP], U4P[NP], AK4P[NP], RHO4P[NP], RI4P[NP];
#pragma unroll
  for (int pr = 0; pr < NP; ++pr) {
    Z4P[pr] = pack_of([&](int r) { return reg(Z4[r]); }, pr);
    Y4P[pr] = pack_of([&](int r) { return reg(Y4[r]); }, pr);
    L4P[pr] = pack_of([&](int r) { return reg(L4[r]); }, pr);
    U4P[pr] = pack_of([&](int r) { return reg(U4[r]); }, pr);
    AK4P[pr] = pack_of([&](int r) { return reg(AK4[r]); }, pr);
    RHO4P[pr] = pack_of([&](int r) { return reg(RHO4[r]); }, pr);
    RI4P[pr] = pack_of([&](int r) { return reg(RI4[r]); }, pr);
  }
  if (KS == 0 && mode != 0) {
    // P~x of the warm iterate (the Riccati variant carries P~x through the KKT identity from here):
    // P~x = c D H (D x), H v = B_qp' Q B_qp v + R v by the dynamics: x_{i+1} = A x_i + B_i v_i
    // from x_0 = 0, e_i = Q x_{i+1}, lambda_j = e_j + A' lambda_{j+1}, (H v)_j = B_j' lambda_j + R v_j.
#pragma unroll
    for (int r = 0; r < R; ++r)
      if (vvr[r]) HS.Dt[ND * (4 * r + ig) + idx] = Dv[r] * X[r];
    if (t < 16) HS.vec[0][t] = 0.0;
    wave_sync();
    for (int i = 0; i < N; ++i) {
      if (t < ND) {
        const double* pv = HS.vec[i & 1];
        const double* v = HS.Dt + ND * i;
        double s;
        if (t == 0) s = (pv[0] + A.ad0 * pv[6]) + A.ad1 * pv[7];
        else if (t == 1) s = (pv[1] + (-A.ad1) * pv[6]) + A.ad0 * pv[7];
        else if (t == 2) s = pv[2] + dt * pv[8];
        else if (t <= 5) s = pv[t] + dt * pv[t + 6];
        else s = pv[t];
        double bu = 0.0;
        if (t >= 6 && t < 9) {
          const double* bw = sm.Bw[i][t - 6];
          for (int c2 = 0; c2 < ND; ++c2) bu += bw[c2] * v[c2];
        } else if (t >= 9) {
          bu = dtm * (((v[t - 9] + v[t - 6]) + v[t - 3]) + v[t]);
        }
        const double xn = s + bu;
        HS.vec[(i + 1) & 1][t] = xn;
        HS.lam[i][t] = 2 * lane_pick(p.q_weights, t) * xn;
      }
      wave_sync();
    }
    for (int j = N - 2; j >= 0; --j) {
      if (t < ND) HS.lam[j][t] = HS.lam[j][t] + A.atv(t, HS.lam[j + 1]);
      wave_sync();
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const int k = vvr[r] ? 4 * r + ig : 0;
      const double* lm = HS.lam[k];
      const double hv = (((sm.Bw[k][0][idx] * lm[6] + sm.Bw[k][1][idx] * lm[7]) + sm.Bw[k][2][idx] * lm[8]) +
                         dtm * lm[9 + idx % 3]) + (2 * lane_pick(p.r_weights, idx)) * HS.Dt[ND * k + idx];
      PX[r] = vvr[r] ? (c_s * Dv[r]) * hv : 0.0;
    }
  }
  // D and E of the lane's variable / rows, reloaded from the image where they are needed (the
  // factorizations, the checks, the epilogue) instead of being held in loop-carried registers: the
  // element offset goes through an opaque copy, so the loads are neither hoisted out of the loop
  // nor merged across uses.  Plain loads, not volatile ones (each volatile load was followed by its
  // own wait for the memory round trip); unconditional, at a clamped step, the padding value
  // selected after (a load under the lane mask became a branch with its own wait).  A
  // global-address-space pointer: global_load, not flat_load, whose lgkmcnt share would also wait
  // on the LDS traffic in flight.
  using gd = const __attribute__((address_space(1))) double;
  gd* const imv = (gd*)im;
  auto img_at = [&](int e) __attribute__((always_inline)) -> double {
    asm volatile("" : "+v"(e));
    return imv[e];
  };
  auto dv_of = [&](int r) __attribute__((always_inline)) {
    const double v = img_at(SI::D + ND * min(4 * r + ig, N - 1) + idx);
    return vvr[r] ? v : 1.0;
  };
  auto ev_of = [&](int r) __attribute__((always_inline)) {
    const double v = img_at(SI::E + CD * min(4 * r + ig, N - 1) + 5 * leg + a);
    return kvr[r] ? v : 1.0;
  };
  auto e4_of = [&](int r) __attribute__((always_inline)) {
    const double v = img_at(SI::E + CD * min(4 * r + ig, N - 1) + 5 * leg + 4);
    return kvr[r] ? v : 1.0;
  };
  // rows 0-3: l = 0 / u = +inf (rows 0, 2) or l = -inf / u = 0 (rows 1, 3): always inequalities
  auto lo03 = [&](double ev) __attribute__((always_inline)) { return (a & 1) ? ev * -OSQP_INF : ev * 0.0; };
  // the projection onto those bounds needs no E: [0, +inf) for rows 0, 2, (-inf, 0] for rows 1, 3
  // (equal to clamping at E * -+OSQP_INF for every operand below 1e30 E in magnitude)
  const double LO03 = (a & 1) ? -INFINITY : 0.0, HI03 = (a & 1) ? 0.0 : INFINITY;
  auto hi03 = [&](double ev) __attribute__((always_inline)) { return (a & 1) ? ev * 0.0 : ev * OSQP_INF; };
  wave_sync();  // every LDS read of the setup image precedes its reuse by the factorization

  // ---- 5. ADMM (osqp_solve) ------------------------------------------------------------------------
  auto& F = sm.u.f;
  // per-lane weights, selected once (lane_pick: a per-lane index into the kernel parameters is a
  // scratch copy and a memory round trip): 2 r of the lane's variable component, 2 q_(6+c) of its
  // impulse component (KS = 1)
  double R2I = 2.0 * lane_pick(p.r_weights, idx), Q2C = 2.0 * lane_pick(p.q_weights, 6 + (t < 6 * N ? t : 0) % 6);
  keep(R2I);
  keep(Q2C);
  // KS = 0: 2 q_j of the MFMA column j = lane & 15 (factorize_mfma's cQ diagonal)
  double Q2J = KS == 0 ? 2.0 * lane_pick(p.q_weights, li < ND ? li : 0) : 0.0;
  keep(Q2J);
  // KS = 0 without stored Acl: the lane's coefficients of A' on states 0-5 (lane of state i: A[s][i])
  // and of A on states 6-11 (A[i][6 + s]), the off-diagonal part of the discrete A
  constexpr bool NOACL = KS == 0 && !WSmem<N, KS>::SACL;
  double CAT[NOACL ? 6 : 1], CAX[NOACL ? 6 : 1];
  if constexpr (NOACL) {
    const int si = 3 * leg + (a < 3 ? a : 0);  // the lane's state (a = 3: padding)
    const bool sv = a < 3;
#pragma unroll
    for (int e = 0; e < 6; ++e) {
      CAT[e] = sv && si >= 6 ? A.at(e, si) : 0.0;
      CAX[e] = sv && si < 6 ? A.at(si, 6 + e) : 0.0;
    }
  }
  // the LDS address of element c of the lane's row of the packed G_k^-1 in round 0 (step ig)
  unsigned GADR[NOACL ? 12 : 1];
  if constexpr (NOACL) {
    const unsigned gb = lds_off(&sm.u.f.Gp[0][0]) + (unsigned)(sizeof(double) * GPS * ig);
#pragma unroll
    for (int e = 0; e < 12; ++e)
      GADR[e] = gb + (unsigned)sizeof(double) * (unsigned)(e >= idx ? poff(idx) + e - idx : poff(e) + idx - e);
  }
  (void)GADR;
  (void)CAT;
  (void)CAX;
  // KS = 1: the lane's rows of R'^-1 (mpcqp_schur.h), set per rho
  double SRI[KS == 1 ? R : 1][3];
  (void)SRI;
  // KS = 1: P~v computed directly where the checks need it (mpcqp_schur.h schur_px)
  auto px_of = [&](const double (&v)[R], const double (&dd)[R], double (&out)[R]) __attribute__((always_inline)) {
    if constexpr (KS == 1) {
      double dvv[R];
#pragma unroll
      for (int r = 0; r < R; ++r) dvv[r] = dd[r] * v[r];
      schur_px<N, R>(sm, F, p, A, dtm, cost_c, Q2C, R2I, dvv, dd, vvr, out);
    }
  };
  double rho = rho0, rinv = 1. / rho0, pri_res = 0.0, dua_res = 0.0;
  int status = MPCQP_STATUS_UNSOLVED, iters = 0, rho_updates = 0, ntrace = 0;
  double obj_sum = 0.0;  // 1/2 x'P~x + q~'x of the final iterate (scaled), set when the loop ends
  bool need_factor = true;
  osqp::InfoSchedule sched(p);
  bool amp_bad = false;  // the Schur form's cancellation bound was crossed at the last check
  for (int iter = 1; iter <= p.max_iter; ++iter) {
    if (need_factor) {
      WV_MARK(10);
#ifdef MPCQP_FACTOR_REPS  // (measurement builds only: every factorization done this many times)
#pragma nounroll
      for (int frep = 0; frep < MPCQP_FACTOR_REPS; ++frep) {
#endif
      // R'_k foot blocks: c 2r + D^-1 (sigma I + A~' diag(rho) A~) D^-1
#pragma unroll
      for (int r = 0; r < R; ++r) {
        const double k00 = dpp<QP_B0>(AK0[r]), k01 = dpp<QP_B1>(AK0[r]), k02 = dpp<QP_B2>(AK0[r]),
                     k03 = dpp<QP_B3>(AK0[r]);
        const double k10 = dpp<QP_B0>(AK1[r]), k11 = dpp<QP_B1>(AK1[r]), k12 = dpp<QP_B2>(AK1[r]),
                     k13 = dpp<QP_B3>(AK1[r]);
        // D^-1 of the foot's three variables from the lanes' own 1 / D (the same correctly rounded
        // quotients: no reload of D, no division here)
        const double dir = DI[r];
        const double i0 = dpp<QP_B0>(dir), i1 = dpp<QP_B1>(dir), i2 = dpp<QP_B2>(dir);
        const double ak4 = unpack(AK4P, r), r4 = unpack(RHO4P, r);
        // rows of the foot: r0 [k00,0,k10] r1 [k01,0,k11] r2 [0,k02,k12] r3 [0,k03,k13] r4 [0,0,ak4]
        auto coef = [&](int row, int col) __attribute__((always_inline)) {
          if (row == 4) return col == 2 ? ak4 : 0.0;
          const double kp = row == 0 ? k00 : row == 1 ? k01 : row == 2 ? k02 : k03;
          const double kz = row == 0 ? k10 : row == 1 ? k11 : row == 2 ? k12 : k13;
          if (col == 2) return kz;
          return (col == (row >> 1)) ? kp : 0.0;
        };
        const int k = 4 * r + ig;
        const double ia = a == 0 ? i0 : (a == 1 ? i1 : i2);
#pragma unroll
        for (int b = 0; b < 3; ++b) {
          double s = 0.0;
#pragma unroll
          for (int row = 0; row < 5; ++row) s += (coef(row, av ? a : 2) * (row == 4 ? r4 : rho)) * coef(row, b);
          const double ib = b == 0 ? i0 : (b == 1 ? i1 : i2);
          const double rt = (av && a == b ? cost_c * R2I : 0.0) + (ia * ((av && a == b ? sigma : 0.0) + s)) * ib;
          if (kvr[r] && av && b >= a) {
            if constexpr (KS == 0) F.rt(k)[6 * leg + sym6(a, b)] = rt;
            else F.s.Rt[k][leg][sym6(a, b)] = rt;
          }
        }
      }
      wave_sync();
      if constexpr (KS == 0) factorize_mfma<N>(sm, p, A, cost_c, dtm, Q2J);
      else {
        double smax;
        schur_factor<N, R>(sm, F, p, A, cost_c, dtm, SRI, mark, smax);
        // The push-through identity subtracts B'(I - S^-1)B w from R'^-1 w: with S ill-conditioned
        // (large state weights, four feet in contact) the difference loses digits the Riccati form
        // keeps.  Such a robot leaves the loop at the next need_info iteration (one follows every
        // factorization before the next one; an exit right here cost 8 % of the kernel in register
        // allocation) and is handed to the Riccati form (wave_kernel: the same wave), which solves
        // it from the start; nothing of it has been written.  max S_ii of the latest factorization
        // lives in the robot's image slot, not in a loop-carried register.
        if (t == 0) im[SI::DEGEN] = smax;
      }
      wave_sync();
#ifdef MPCQP_FACTOR_REPS
      }
#endif
      need_factor = false;
      WV_MARK(12);
    }

    // ---- KKT solve: u = (c B'Q̄B + R')^-1 D^-1 rhs, x~ = D^-1 u ----
    double U[R];
    double amp = 1.0;  // the Schur form's cancellation at the update_info iteration (schur_solve)
    auto kkt = [&](auto INFO) __attribute__((always_inline)) {
      const bool tm_it = iter == 60;
      // mark 53: q = Q z stored, 53 -> 45 being the Schur form's u phase.  Timing builds take the cycle
      // count there and mark 45 carries it (a record of its own inside the u phase, with every round's
      // columns of B live, is more than the register allocator takes).
      long long cyc_q = 0;
      (void)cyc_q;
      if (tm_it) WV_MARK(40);
      if constexpr (KS == 1) {
        double W[R];
#pragma unroll
        for (int r = 0; r < R; ++r) W[r] = DI[r] * RHS[r];
        schur_solve<N, R, decltype(INFO)::value>(F, W, SRI, vvr, U, amp, [&]() __attribute__((always_inline)) {
          if (tm_it) WV_STAMP(53, cyc_q);
        });
      } else if constexpr (NOACL) {
        riccati_solve_noacl<N, R>(sm, F, DI, RHS, CAT, CAX, GADR, dtm, ig, q, leg, a, idx, tm_it, mark, U);
      } else {
        // LDS operands are loaded one phase ahead of their use; sched_barrier keeps the scheduler from
        // sinking a prefetch back down to its consumer (counted lgkmcnt waits then cover only it).
        double W[R], AKw[R], SMv[R], G[R], Hh[R], XS[R], tt[R];
        // Every phase's rows of all rounds are loaded one phase ahead (48 R VGPRs): Acl is stored only
        // up to ACL_MAXN steps, three rounds.
        static_assert(R <= 3, "the stored-Acl solve holds every round's rows in registers");
        double cA[R][12], cB[R][12], cw[R][3];
        int kc[R], kk[R];
#pragma unroll
        for (int r = 0; r < R; ++r) {
          W[r] = DI[r] * RHS[r];
          SMv[r] = 0.0;
          XS[r] = 0.0;
          kc[r] = min(4 * r + ig, N - 1);
          kk[r] = max(kc[r] - 1, 0);  // slot of K_k (k >= 1)
        }
        double cn[12];
#pragma unroll
        for (int r = 0; r < R; ++r) ldcol(cA[r], &F.K[kk[r]][idx]);
        // The chains load Acl one ROUND at a time: DPP row q takes the matrix of step 4 rr + gray(q) of
        // round rr, the step that row computes (every chain step runs in the row of its step), so one
        // 12-double load per lane serves four chain steps.
        constexpr int NA = RicFactors<N, true>::NA;
        auto aslot = [&](int rr) __attribute__((always_inline)) { return min(max(4 * rr + ig - 1, 0), NA - 1); };
        if constexpr (N >= 3) ldcol(cn, &F.Acl[aslot((N - 2) >> 2)][idx]);
        __builtin_amdgcn_sched_barrier(0);
        // a_k = K_k' w_k (k >= 1)
#pragma unroll
        for (int r = 0; r < R; ++r) lds_wait<N >= 3 ? 12 : 0>(cA[r]);
        mv_rounds<R>(W, cA, AKw);
        __builtin_amdgcn_sched_barrier(0);
        if (tm_it) WV_MARK(41);
        // g_k's G_k^-1 rows and B_k' columns: issued when the backward chain enters its last round
        // (three steps before their use), so they do not hold registers through the whole chain
        auto load_g = [&]() __attribute__((always_inline)) {
#pragma unroll
          for (int r = 0; r < R; ++r) {
            ld12(cB[r], &F.Gi[kc[r]][mo(idx)]);
            cw[r][0] = sm.Bw[kc[r]][0][idx];
            cw[r][1] = sm.Bw[kc[r]][1][idx];
            cw[r][2] = sm.Bw[kc[r]][2][idx];
          }
        };
        constexpr int KG = N - 2 >= 2 ? 2 : N - 2;  // the backward chain's step that issues them
        if constexpr (KG < 1) load_g();
        {  // backward chain: s_{N-1} = -a_{N-1}; s_k = Acl_k' s_{k+1} - a_k; SMv (row of k) = s_{k+1}
          double cur = -AKw[(N - 1) >> 2];
          double cc[12];
          sfor<0, N - 1>([&](auto J) {
            constexpr int k = N - 2 - decltype(J)::value;
            const double mvv = rmove2<row_of(k + 1), row_of(k)>(cur);
            SMv[k >> 2] = (q == row_of(k)) ? mvv : SMv[k >> 2];
            if constexpr (k >= 1) {
              if constexpr (k == N - 2 || (k & 3) == 3) {  // entering round k >> 2 (descending)
                lds_wait<0>(cn);
#pragma unroll
                for (int e = 0; e < 12; ++e) cc[e] = cn[e];
                if constexpr (k >= 4) ldcol(cn, &F.Acl[aslot((k >> 2) - 1)][idx]);  // the next round's columns
              }
              if constexpr (k == KG) load_g();
              __builtin_amdgcn_sched_barrier(0);
              cur = mv12a(mvv, cc, -AKw[k >> 2]);
            }
          });
        }
        if (tm_it) WV_MARK(42);
        // g_k = G_k^-1 (w_k + B_k' s_{k+1})
        auto ttr = [&](int r, double c0, double c1, double c2) __attribute__((always_inline)) {
          const double c6[6] = {c0, c1, c2, a == 0 ? dtm : 0.0, a == 1 ? dtm : 0.0, a == 2 ? dtm : 0.0};
          return W[r] + mv6(SMv[r], c6);
        };
        // h_k = B_k g_k: rows 6-8 (leg-2 lanes) B_w g, rows 9-11 (leg-3 lanes) dt/m times the sum of
        // the legs' matching force component, rows 0-5 zero
        auto hhr = [&](int r, double hb) __attribute__((always_inline)) {
          const double ls = dtm * legsum(G[r]);
          return leg == 2 ? hb : (leg == 3 ? ls : 0.0);
        };
#pragma unroll
        for (int r = 0; r < R; ++r) tt[r] = ttr(r, cw[r][0], cw[r][1], cw[r][2]);
#pragma unroll
        for (int r = 0; r < R; ++r) ld12(cA[r], &sm.Bw[kc[r]][av ? a : 2][0]);  // for h_k
        __builtin_amdgcn_sched_barrier(0);
        mv_rounds<R>(tt, cB, G);
        if constexpr (N >= 3) ld12(cn, &F.Acl[aslot(0)][mo(idx)]);
        __builtin_amdgcn_sched_barrier(0);
        {
          double hb[R];
          mv_rounds<R>(G, cA, hb);
#pragma unroll
          for (int r = 0; r < R; ++r) Hh[r] = hhr(r, hb[r]);
        }
        if (tm_it) WV_MARK(43);
        // u_k's K_k rows: issued three steps before the forward chain ends
        auto load_u = [&]() __attribute__((always_inline)) {
#pragma unroll
          for (int r = 0; r < R; ++r) ld12(cB[r], &F.K[kk[r]][mo(idx)]);
        };
        constexpr int KU = N - 2 >= 1 ? (N - 3 > 1 ? N - 3 : 1) : 0;  // two steps before the end
        if constexpr (KU < 1) load_u();
        {  // forward chain: x_1 = h_0; x_{k+1} = Acl_k x_k + h_k; XS (row of k) = x_k
          double cur = Hh[0];
          double cc[12];
          sfor<1, N>([&](auto K) {
            constexpr int k = decltype(K)::value;
            const double mvv = rmove2<row_of(k - 1), row_of(k)>(cur);
            XS[k >> 2] = (q == row_of(k)) ? mvv : XS[k >> 2];
            if constexpr (k <= N - 2) {
              if constexpr (k == 1 || (k & 3) == 0) {  // entering round k >> 2 (ascending)
#pragma unroll
                for (int e = 0; e < 12; ++e) cc[e] = cn[e];
                if constexpr (4 * ((k >> 2) + 1) <= N - 2) ld12(cn, &F.Acl[aslot((k >> 2) + 1)][mo(idx)]);
              }
              if constexpr (k == KU) load_u();
              __builtin_amdgcn_sched_barrier(0);
              cur = mv12a(mvv, cc, Hh[k >> 2]);
            }
          });
        }
        if (tm_it) WV_MARK(44);
        // u_k = g_k - K_k x_k (x_0 = 0)
        double kx[R];
        mv_rounds<R>(XS, cB, kx);
#pragma unroll
        for (int r = 0; r < R; ++r) U[r] = G[r] - kx[r];
      }
      if (tm_it) WV_MARK_WITH(45, cyc_q);
    };

    // ---- update_x / update_z / update_y, and P~x by the KKT identity P~x~ = rhs - sigma x~ - A~'rho A~x~
    // this iteration's deltas, for the infeasibility tests of a need_info iteration only
    double DX[R], DY[R], DY4P[NP], PXO[R];
    auto update = [&](auto INFO) __attribute__((always_inline)) {
      constexpr bool info = decltype(INFO)::value;
      double xt[R], xz[R], zt[R];
#pragma unroll
      for (int r = 0; r < R; ++r) {
        xt[r] = DI[r] * U[r];
        const double xp = dpp<QP_PRIM>(xt[r]);
        xz[r] = dpp<QP_B2>(xt[r]);
        zt[r] = AK0[r] * xp + AK1[r] * xz[r];
        {  // (fmin/fmax = the reference's c_min/c_max on these non-NaN operands)
          const double zr = alpha * zt[r] + (1.0 - alpha) * Z[r];
          const double zn = fmin(fmax(zr + rinv * Y[r], LO03), HI03);
          const double dyv = rho * (zr - zn);
          Z[r] = zn;
          Y[r] = Y[r] + dyv;
          if constexpr (info) DY[r] = dyv;
        }
      }
      // row 4, packed: lane a projects round 4 pr + a
      double V4P[NP], T4P[NP];
#pragma unroll
      for (int pr = 0; pr < NP; ++pr) {
        const double zt4 = AK4P[pr] * pack_of([&](int r) { return xz[r]; }, pr);
        const double r4 = RHO4P[pr];
        const double zr = alpha * zt4 + (1.0 - alpha) * Z4P[pr];
        const double zn = fmin(fmax(zr + RI4P[pr] * Y4P[pr], L4P[pr]), U4P[pr]);
        const double dyv = r4 * (zr - zn);
        Z4P[pr] = zn;
        Y4P[pr] = Y4P[pr] + dyv;
        if constexpr (info) DY4P[pr] = dyv;
        V4P[pr] = RHO4P[pr] * Z4P[pr] - Y4P[pr];
        T4P[pr] = KS == 0 ? RHO4P[pr] * zt4 : 0.0;
      }
#pragma unroll
      for (int r = 0; r < R; ++r) {
        // every lane updates (values of padding lanes / steps past N are never read unmasked)
        const double xo = X[r];
        const double xn = alpha * xt[r] + (1.0 - alpha) * xo;
        if constexpr (info) DX[r] = xn - xo;
        X[r] = xn;
        const double ak4 = unpack(AK4P, r);
        if constexpr (KS == 0) {  // the Riccati variant carries P~x; the Schur form computes it at checks
          const double kd = quad_at(rho * zt[r], unpack(T4P, r), AK0[r], AK1[r], ak4, a);
          const double pxt = (RHS[r] - sigma * xt[r]) - kd;
          if constexpr (info) PXO[r] = PX[r];
          PX[r] = alpha * pxt + (1.0 - alpha) * PX[r];
        }
        // next right-hand side sigma x - q~ + A~'(rho z - y) (recomputed below when adapt_rho changes rho)
        const double at = quad_at(rho * Z[r] - Y[r], unpack(V4P, r), AK0[r], AK1[r], ak4, a);
        RHS[r] = (sigma * X[r] - Qv[r]) + at;
      }
    };

    // The iterations before the next one that needs update_info (a termination check, an adapt_rho
    // step or the last iteration) run in a loop of their own: the check's registers are then live
    // only outside it, and the allocator keeps the ADMM state of the inner loop in registers.
    {
      const int plain = sched.plain_ahead(p, iter);
      for (int j = 0; j < plain; ++j) {
        kkt(IC<0>{});
        sched.plain_step(p);
        update(IC<0>{});
        if (iter == 60) WV_MARK(46);
        if (iter == 60) WV_MARK(47);
        ++iter;
      }
    }
    const bool tm_it = iter == 60;
    kkt(IC<1>{});  // (with the inner loop above, always an update_info iteration)
    bool is_check, is_adapt, last;
    const bool need_info = sched.info_step(p, iter, is_check, is_adapt, last);

    if (need_info) update(IC<1>{});
    else update(IC<0>{});

    if (tm_it) WV_MARK(46);
    const bool tm_ck = iter == 75;  // (a termination check + adapt_rho iteration, timed)
    if (tm_ck) WV_MARK(48);
    if (need_info) {
      // ---- update_info / check_termination / adapt_rho (osqp.c, auxil.c) ----
      // KS = 1: P~x of this iterate, local to the check (not carried through the loop)
      // D and E of the lane's variables / rows.  The Riccati form loads them for the whole check in
      // one batch (one memory round trip instead of one per round: C4 +1.4 %); the Schur form where
      // they are used (holding them through P~x made its check slower: C2 -2 %, profiles/r05)
      // row 4 per round (the packed registers unpacked for the check)
      double Z4[R], Y4[R], L4[R], U4[R], AK4[R], DY4[R];
#pragma unroll
      for (int r = 0; r < R; ++r) {
        Z4[r] = unpack(Z4P, r);
        Y4[r] = unpack(Y4P, r);
        L4[r] = unpack(L4P, r);
        U4[r] = unpack(U4P, r);
        AK4[r] = unpack(AK4P, r);
        DY4[r] = unpack(DY4P, r);
      }
      double DVc[R], EVc[R], E4c[R];
#pragma unroll
      for (int r = 0; r < R; ++r) {
        if constexpr (KS == 0) {
          DVc[r] = dv_of(r);
          EVc[r] = ev_of(r);
          E4c[r] = e4_of(r);
        } else {
          DVc[r] = EVc[r] = E4c[r] = 0.0;
        }
      }
      auto dvc = [&](int r) __attribute__((always_inline)) { return KS == 0 ? DVc[r] : dv_of(r); };
      auto evc = [&](int r) __attribute__((always_inline)) { return KS == 0 ? EVc[r] : ev_of(r); };
      auto e4c = [&](int r) __attribute__((always_inline)) { return KS == 0 ? E4c[r] : e4_of(r); };
      double PXl[R];
      double (&PXc)[R] = KS == 1 ? PXl : PX;
      if constexpr (KS == 1) {
        double dd[R];
#pragma unroll
        for (int r = 0; r < R; ++r) dd[r] = dvc(r);
        px_of(X, dd, PXc);
      }
      if (tm_ck) WV_MARK(50);
      // The norms of update_info / check_termination / compute_rho_estimate, and the first-level
      // quantities of both infeasibility tests (||E dy||, the support term of dy, ||D dx||, q'dx:
      // needed at nearly every check, since dua_res is rarely small before convergence), reduced
      // in one batch of independent wave reductions.  Norms that enter only as max(a, b) share a
      // slot (a max is exact in any grouping): [0] |E^-1 (A~x - z)|, [1] |A~x - z|,
      // [2] max(|E^-1 z|, |E^-1 A~x|), [3] max(|z|, |A~x|), [4] |D^-1 dual|, [5] |dual|,
      // [6] max(|D^-1 q~|, |D^-1 A~'y|, |D^-1 P~x|), [7] max(|q~|, |A~'y|, |P~x|).
      constexpr int NM = 8;
      double mx[NM];
#pragma unroll
      for (int k = 0; k < NM; ++k) mx[k] = 0.0;
      double nd = 0.0, lh = 0.0, nx = 0.0, qd = 0.0, dyp[R], dyp4[R];
#pragma unroll
      for (int r = 0; r < R; ++r) {
        const double xp = dpp<QP_PRIM>(X[r]), xz = dpp<QP_B2>(X[r]);
        const double ax = AK0[r] * xp + AK1[r] * xz, ax4 = AK4[r] * xz;
        const double aty = quad_at(Y[r], Y4[r], AK0[r], AK1[r], AK4[r], a);
        const double evr = evc(r), e4r = e4c(r);
        if (kvr[r]) {
          const double ei = recip(evr), ei4 = recip(e4r);
          const double pr = ax + (-1.0) * Z[r], pr4 = ax4 + (-1.0) * Z4[r];
          mx[0] = nmax(mx[0], nmax(dabs(ei * pr), dabs(ei4 * pr4)));
          mx[1] = nmax(mx[1], nmax(dabs(pr), dabs(pr4)));
          mx[2] = nmax(mx[2], nmax(nmax(dabs(ei * Z[r]), dabs(ei4 * Z4[r])), nmax(dabs(ei * ax), dabs(ei4 * ax4))));
          mx[3] = nmax(mx[3], nmax(nmax(dabs(Z[r]), dabs(Z4[r])), nmax(dabs(ax), dabs(ax4))));
        }
        if (vvr[r]) {
          const double d = (Qv[r] + 1.0 * PXc[r]) + 1.0 * aty;
          mx[4] = nmax(mx[4], dabs(DI[r] * d));
          mx[5] = nmax(mx[5], dabs(d));
          mx[6] = nmax(mx[6], nmax(nmax(dabs(DI[r] * Qv[r]), dabs(DI[r] * aty)), dabs(DI[r] * PXc[r])));
          mx[7] = nmax(mx[7], nmax(nmax(dabs(Qv[r]), dabs(aty)), dabs(PXc[r])));
        }
        // is_primal_infeasible: ||E dy||_inf and u'max(dy, 0) + l'min(dy, 0) of the projected dy
        const double lo = lo03(evr), hi = hi03(evr);
        const double d = osqp::polar_project(DY[r], lo, hi), d4 = osqp::polar_project(DY4[r], L4[r], U4[r]);
        dyp[r] = d;
        dyp4[r] = d4;
        if (kvr[r]) {
          nd = nmax(nd, nmax(dabs(evr * d), dabs(e4r * d4)));
          lh += hi * dmax(d, 0.0) + lo * dmin(d, 0.0);
          if (a == 0) lh += U4[r] * dmax(d4, 0.0) + L4[r] * dmin(d4, 0.0);
        }
        // is_dual_infeasible: ||D dx||_inf and q~'dx
        if (vvr[r]) {
          nx = nmax(nx, dabs(dvc(r) * DX[r]));
          qd += Qv[r] * DX[r];
        }
      }
      // the 10 max- and 2 sum-reductions level by level (wave_reduce_batch: same bits, no waits)
      double rm[NM + 2], rs[2] = {lh, qd};
#pragma unroll
      for (int k = 0; k < NM; ++k) rm[k] = mx[k];
      rm[NM] = nd;
      rm[NM + 1] = nx;
      wave_reduce_batch(rm, rs);
#pragma unroll
      for (int k = 0; k < NM; ++k) mx[k] = rm[k];
      const double ndy = rm[NM], ndx = rm[NM + 1];
      lh = rs[0];
      qd = rs[1];
      pri_res = mx[0];
      dua_res = cinv * mx[4];
      iters = iter;
      if (tm_ck) WV_MARK(51);
      auto check = [&](bool approx) __attribute__((always_inline)) -> int {
        double eps_abs = p.eps_abs, eps_rel = p.eps_rel, eps_pinf = p.eps_prim_inf, eps_dinf = p.eps_dual_inf;
        if (pri_res > OSQP_INF || dua_res > OSQP_INF) return MPCQP_STATUS_NON_CVX;
        if (approx) { eps_abs *= 10; eps_rel *= 10; eps_pinf *= 10; eps_dinf *= 10; }
        const bool prim_ok = pri_res < osqp::tolerance(eps_abs, eps_rel, mx[2]);
        bool prim_inf = false, dual_inf = false;
        if (!prim_ok && ndy > DIV_TOL && lh < eps_pinf * ndy) {
          double an = 0.0;
#pragma unroll
          for (int r = 0; r < R; ++r) {
            const double atd = quad_at(dyp[r], dyp4[r], AK0[r], AK1[r], AK4[r], a);
            if (vvr[r]) an = nmax(an, dabs(DI[r] * atd));
          }
          an = wave_nmax(an);
          prim_inf = an < eps_pinf * ndy;
        }
        const bool dual_ok = dua_res < osqp::tolerance(eps_abs, eps_rel, cinv * mx[6]);
        if (!dual_ok && ndx > DIV_TOL && qd < cost_c * eps_dinf * ndx) {
          // is_dual_infeasible (P~ delta_x = P~x_new - P~x_old)
          double pd = 0.0, PDX[R];
          if constexpr (KS == 1) {
            double dd[R];
#pragma unroll
            for (int r = 0; r < R; ++r) dd[r] = dvc(r);
            px_of(DX, dd, PDX);
          }
#pragma unroll
          for (int r = 0; r < R; ++r) {
            if constexpr (KS == 0) PDX[r] = PX[r] - PXO[r];
            if (vvr[r]) pd = nmax(pd, dabs(DI[r] * PDX[r]));
          }
          pd = wave_nmax(pd);
          if (pd < cost_c * eps_dinf * ndx) {
            double viol = 0.0;
#pragma unroll
            for (int r = 0; r < R; ++r) {
              const double dp = dpp<QP_PRIM>(DX[r]), dz = dpp<QP_B2>(DX[r]);
              const double evr = evc(r);
              const double v = (1.0 / evr) * (AK0[r] * dp + AK1[r] * dz);
              const double v4 = (1.0 / e4c(r)) * (AK4[r] * dz);
              const double lo = lo03(evr), hi = hi03(evr);
              if (kvr[r]) {
                // osqp::dual_ray_violates, written out (the call costs the Schur kernel 8 SGPR spills)
                if ((hi < OSQP_INF * MIN_SCALING && v > eps_dinf * ndx) ||
                    (lo > -OSQP_INF * MIN_SCALING && v < -eps_dinf * ndx))
                  viol = 1.0;
                if ((U4[r] < OSQP_INF * MIN_SCALING && v4 > eps_dinf * ndx) ||
                    (L4[r] > -OSQP_INF * MIN_SCALING && v4 < -eps_dinf * ndx))
                  viol = 1.0;
              }
            }
            viol = wave_nmax(viol);
            dual_inf = viol == 0.0;
          }
        }
        return osqp::termination_status(prim_ok, dual_ok, prim_inf, dual_inf, approx);
      };
      int st = MPCQP_STATUS_UNSOLVED;
      bool done = false, refactor = false;
      for (int pass = 0; pass < 2 && !done; ++pass) {
        if (pass == 1 && !last) break;
        if (pass == 1 || is_check || last) {
          st = check(pass == 1);
          done = st != MPCQP_STATUS_UNSOLVED;
        }
        if (pass == 1 || done || !is_adapt) continue;
        const double est = osqp::rho_estimate(rho, mx[1], mx[3], mx[5], mx[7]);
        if (osqp::rho_moved(est, rho, p.adaptive_rho_tolerance)) {
          rho = dmin(dmax(est, RHO_MIN), RHO_MAX);  // (adapt_rho clamps the clamped estimate again)
          rho_updates += 1;
          refactor = !last;
        }
      }
      if (tm_ck) WV_MARK(52);
      if (last && st == MPCQP_STATUS_UNSOLVED) st = MPCQP_STATUS_MAX_ITER_REACHED;
      // (an ill-conditioned factorization since the last check, or a KKT solve whose push-through
      // identity cancelled too many digits: leave now, see the factorization)
      if constexpr (KS == 1) amp_bad = !(amp * img_at(SI::DEGEN) <= SCHUR_AMP);
      if (last || (KS == 1 && (amp_bad || !(img_at(SI::DEGEN) <= SCHUR_SMAX)))) done = true;
      status = st;
#ifndef MPCQP_PHASE_TIMING
      if (trace && t == 0 && inst < trace_cap && ntrace < MPCQP_TRACE_LEN && is_check) {
        double* tp = trace + ((size_t)inst * MPCQP_TRACE_LEN + ntrace) * 4;
        tp[0] = iter; tp[1] = pri_res; tp[2] = dua_res; tp[3] = rho;
      }
#endif
      ntrace += is_check ? 1 : 0;
      if (done) {
        // the objective of the final iterate (every exit of the loop is a need_info iteration)
#pragma unroll
        for (int r = 0; r < R; ++r)
          if (vvr[r]) obj_sum += 0.5 * X[r] * PXc[r] + Qv[r] * X[r];
        obj_sum = wave_sum(obj_sum);
        break;
      }
      if (refactor) {
#pragma unroll
        for (int pr = 0; pr < NP; ++pr) {
          RHO4P[pr] = rho4_of(L4P[pr], U4P[pr], rho);
          RI4P[pr] = 1. / RHO4P[pr];
        }
        rinv = 1. / rho;
        need_factor = true;
        // the right-hand side with the new rho vector
#pragma unroll
        for (int r = 0; r < R; ++r) {
          const double at = quad_at(rho * Z[r] - Y[r], unpack(RHO4P, r) * Z4[r] - Y4[r], AK0[r], AK1[r], AK4[r], a);
          RHS[r] = (sigma * X[r] - Qv[r]) + at;
        }
      }
    }
    if (tm_ck) WV_MARK(49);
    if (tm_it) WV_MARK(47);
  }

  WV_MARK(20);
  if (KS == 1 && (amp_bad || !(img_at(SI::DEGEN) <= SCHUR_SMAX))) {  // the Riccati form solves it
    if (t == 0) atomicAdd(fb + (amp_bad ? 1 : 2), 1);
    return WAVE_HANDOFF | order_cost(iters, rho_updates);
  }
  if (ws) {  // the solver persists: scaling, scaled data, iterates and rho for the next tick
    if (t == 0) {
      ws[WL::FLAG] = 1.0;
      ws[WL::RHO] = rho;
      ws[WL::C] = cost_c;
      ws[WL::MU] = mu_rec;
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const int k = 4 * r + ig;
      if (vvr[r]) {
        const int ci = ND * k + idx;
        ws[WL::D + ci] = dv_of(r);
        ws[WL::QT + ci] = Qv[r];
        ws[WL::X + ci] = X[r];
      }
      if (kvr[r]) {
        const int ri = CD * k + 5 * leg + a, r4 = CD * k + 5 * leg + 4;
        ws[WL::E + ri] = ev_of(r);
        ws[WL::AK + ri] = AK0[r];
        ws[WL::AK + m + ri] = AK1[r];
        ws[WL::Z + ri] = Z[r];
        ws[WL::Y + ri] = Y[r];
        const double ak4 = unpack(AK4P, r), z4 = unpack(Z4P, r), y4 = unpack(Y4P, r);
        if (a == 0) {
          ws[WL::E + r4] = e4_of(r);
          ws[WL::AK + r4] = 0.0;
          ws[WL::AK + m + r4] = ak4;
          ws[WL::Z + r4] = z4;
          ws[WL::Y + r4] = y4;
        }
      }
    }
  }
  // ---- 6. store_solution + unscale + compute_grf extraction (A1RobotControl.cpp:555-561) --------
  const bool has_sol = osqp::has_solution(status);
  const double ob = obj_sum;
  double xs0 = 0.0;
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const double xs = has_sol ? dv_of(r) * X[r] : NAN;
    if (r == 0) xs0 = xs;
    if (solution && vvr[r]) solution[(size_t)inst * n + ND * (4 * r + ig) + idx] = xs;
  }
  // u0 = step 0 = round 0, DPP row 0 (lanes 0..15); f_i = R^T u0[3i:3i+3], NaN legs skipped
  mpcqp_result* res = results + inst;
  const volatile double* rotv = recs + (size_t)inst * C::REC + MPCQP_REC_ROT;
  double Rot[9];
#pragma unroll
  for (int e = 0; e < 9; ++e) Rot[e] = rotv[e];
  const double u00 = dpp<QP_B0>(xs0), u01 = dpp<QP_B1>(xs0), u02 = dpp<QP_B2>(xs0);
  const double nrm = sqrt(u00 * u00 + u01 * u01 + u02 * u02);
  const bool nanleg = isnan(nrm);
  const unsigned long long nanmask = __ballot(q == 0 && a == 0 && nanleg);
  if (q == 0 && av) {
    double s = 0.0;
    s += sel3(a, Rot[0], Rot[1], Rot[2]) * u00;
    s += sel3(a, Rot[3], Rot[4], Rot[5]) * u01;
    s += sel3(a, Rot[6], Rot[7], Rot[8]) * u02;
    res->u0[3 * leg + a] = xs0;
    res->f_body[3 * leg + a] = nanleg ? 0.0 : s;
  }
  if (t == 0) {
    int legs = 0;
    for (int l = 0; l < 4; ++l) legs |= ((nanmask >> (4 * l)) & 1ull) ? (1 << l) : 0;
    res->nan_legs = legs;
    // osqp::objective_of(status, ob, cinv), written out on has_sol above (the call changes the
    // kernel's instruction selection)
    double obj;
    if (has_sol) obj = ob * cinv;
    else if (status == MPCQP_STATUS_PRIMAL_INFEASIBLE || status == MPCQP_STATUS_PRIMAL_INFEASIBLE_INACCURATE) obj = OSQP_INF;
    else if (status == MPCQP_STATUS_DUAL_INFEASIBLE || status == MPCQP_STATUS_DUAL_INFEASIBLE_INACCURATE) obj = -OSQP_INF;
    else obj = NAN;
    osqp::store_info(res, obj, pri_res, dua_res, rho, status, iters, rho_updates);
  }
  return order_cost(iters, rho_updates);
}

// (one wave per SIMD: the whole register file; two robots per SIMD, a 256-register budget, was
// measured and rejected, profiles/r06/two_per_simd)
template <int N, int KS>
__global__ __launch_bounds__(NT, 1) void wave_kernel(const double* __restrict__ recs, int batch,
                                                     mpcqp_result* __restrict__ results,
                                                     double* __restrict__ solution, double* __restrict__ trace,
                                                     int trace_cap, double* __restrict__ wstate,
                                                     double* __restrict__ img, mpcqp_params p,
                                                     int* __restrict__ fb, const int* __restrict__ order,
                                                     int* __restrict__ key) {
  // launch order (mpcqp_order.hip): block i solves robot order[i]; everything below follows inst.
  // An index outside the batch solves nothing.
  const int inst = order ? order[blockIdx.x] : (int)blockIdx.x;
  int cost;
  if constexpr (KS == 1) {
    // The Schur form, and in the same wave the Riccati form for the robots it hands over (the two
    // forms' LDS images share one allocation: the Riccati factors fit inside the Schur core's)
    __shared__ union LdsU {
      WSmem<N, 1> s;
      WSmem<N, 0> r;
    } sm;
    if ((unsigned)inst >= (unsigned)batch) return;
    cost = wave_solve<N, 1>(inst, sm.s, recs, results, solution, trace, trace_cap, wstate, img, p, fb);
    if (cost & WAVE_HANDOFF) {
      wave_sync();
      cost = (cost & ~WAVE_HANDOFF) +
             wave_solve<N, 0>(inst, sm.r, recs, results, solution, trace, trace_cap, wstate, img, p, nullptr);
    }
  } else {
    __shared__ WSmem<N, 0> sm;
    if ((unsigned)inst >= (unsigned)batch) return;
    cost = wave_solve<N, 0>(inst, sm, recs, results, solution, trace, trace_cap, wstate, img, p, fb);
  }
  // what the robot cost, for the next call's launch order
  if (key && threadIdx.x == 0) key[inst] = order_key(cost);
}

// Self-test of the cross-lane primitives (mv12 broadcast lanes, rmove directions): out[64*k + lane].
__global__ void wave_selftest_kernel(double* out) {
  const int t = threadIdx.x;
  const double x = 100.0 * (t >> 4) + (t & 15);
  double c[12];
  for (int i = 0; i < 12; ++i) c[i] = (i == (t & 15) % 12) ? 1.0 : 0.0;
  out[t] = mv12(x, c);            // lane 16q+i: x of lane loff(i % 12) of row q
  out[64 + t] = rmove<0, 1>(x);   // row 1 lanes: row 0 values
  out[128 + t] = rmove<1, 0>(x);  // row 0 lanes: row 1 values
  out[192 + t] = rmove<0, 2>(x);  // row 2 lanes: row 0 values
  out[256 + t] = rmove<3, 1>(x);  // row 1 lanes: row 3 values
  out[320 + t] = rmove<3, 2>(x);  // row 2 lanes: row 3 values
}

}  // namespace wv

// The Schur-form KKT solve serves N <= 10 with nonnegative state weights (it factors Q with square
// roots); the Riccati recursion everything else.
static bool schur_ok(const mpcqp_params& p) {
  if (p.horizon > 10) return false;
  for (int i = 0; i < MPCQP_STATE_DIM; ++i)
    if (!(p.q_weights[i] >= 0.0)) return false;
  return true;
}
template <int N>
static hipError_t launch_wave(const LaunchArgs& a) {
  const hipError_t e = launch_scale_any(a);  // scale_kernel first, on the same stream (mpcqp_scale.hip)
  if (e != hipSuccess) return e;
  const int* ord = a.hint.order;  // written by order_kernel on the same stream, or nullptr: input order
  int* key = ord ? a.hint.key : nullptr;
  if constexpr (N <= 10) {
    if (schur_ok(a.p)) {
      hipLaunchKernelGGL((wv::wave_kernel<N, 1>), dim3(a.batch), dim3(wv::NT), 0, (hipStream_t)a.stream, a.recs,
                         a.batch, a.results, a.solution, a.trace, a.trace_cap, a.wstate, a.work, a.p, a.fallback,
                         ord, key);
      return hipGetLastError();
    }
  }
  hipLaunchKernelGGL((wv::wave_kernel<N, 0>), dim3(a.batch), dim3(wv::NT), 0, (hipStream_t)a.stream, a.recs, a.batch,
                     a.results, a.solution, a.trace, a.trace_cap, a.wstate, a.work, a.p, a.fallback, ord, key);
  return hipGetLastError();
}
// occupancy of the wave kernel a handle with these parameters launches (the KS choice of launch_wave)
template <int N>
static hipError_t occupancy_wave(const mpcqp_params& p, int* blocks) {
  if constexpr (N <= 10)
    if (schur_ok(p)) return hipOccupancyMaxActiveBlocksPerMultiprocessor(blocks, wv::wave_kernel<N, 1>, wv::NT, 0);
  return hipOccupancyMaxActiveBlocksPerMultiprocessor(blocks, wv::wave_kernel<N, 0>, wv::NT, 0);
}

hipError_t launch_wave_any(const LaunchArgs& a) {
  switch (a.p.horizon) {
#define CASE(K) \
  case K: return launch_wave<K>(a);
    MPCQP_WAVE_FOR_EACH_N(CASE)
#undef CASE
    default: return hipErrorInvalidValue;
  }
}
hipError_t occupancy_wave_any(const mpcqp_params& p, int* blocks) {
  switch (p.horizon) {
#define CASE(K) \
  case K: return occupancy_wave<K>(p, blocks);
    MPCQP_WAVE_FOR_EACH_N(CASE)
#undef CASE
    default: return hipErrorInvalidValue;
  }
}
hipError_t wave_selftest(double* d_out, void* stream) {
  hipLaunchKernelGGL(wv::wave_selftest_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, d_out);
  return hipGetLastError();
}
}  // namespace mpcqp
