// mpcqp_osqp.h — the OSQP 0.6 rules every solve kernel decides by, written once: when an iteration
// needs update_info, check_termination (osqp.c) with its status precedence, compute_rho_estimate /
// adapt_rho (auxil.c), the rho vector's row classes (set_rho_vec), the cone tests of the two
// infeasibility certificates, and what a result record holds for each status.
//
// Scalar, wave-uniform decision code: no reductions, no memory but the result record.  The kernels
// keep their own reductions and hand the reduced values in.  Plain C++ that a host compiler reads too
// (tests/cpp/osqp_rules_host.cpp runs these rules on the CPU); it includes nothing but the C ABI.
//
// Contraction: this header carries no `fp contract` pragma, so each translation unit's own mode
// applies to the functions it inlines: the compiler default (eps_abs + eps_rel * norm is one FMA) in
// mpcqp_wave.hip, mpcqp_kernels.hip and mpcqp_riccati.hip; contraction off in mpcqp_balance.hip,
// whose pragma stands above its includes for that reason.
#pragma once
#include "../../include/mpcqp.h"

#ifdef __HIPCC__
#define MPCQP_OSQP_FN __host__ __device__ inline __attribute__((always_inline))
#else
#define MPCQP_OSQP_FN inline
#endif

namespace mpcqp {

// OSQP 0.6 constants.h
constexpr double OSQP_INF = MPCQP_OSQP_INFTY;
constexpr double MIN_SCALING = 1e-4, MAX_SCALING = 1e4;
constexpr double RHO_MIN = 1e-6, RHO_MAX = 1e6, RHO_EQ_OVER_RHO_INEQ = 1e3, RHO_TOL = 1e-4;
constexpr double DIV_TOL = 1.0 / OSQP_INF;

namespace osqp {

MPCQP_OSQP_FN double max2(double a, double b) { return a > b ? a : b; }
MPCQP_OSQP_FN double min2(double a, double b) { return a < b ? a : b; }

// ---- rho vector (set_rho_vec) ---------------------------------------------------------------------
// Class of a constraint row from its scaled bounds: -1 loose (both infinite), 1 equality, 0 inequality.
MPCQP_OSQP_FN int row_kind(double l, double u) {
  const bool loose = l < -OSQP_INF * MIN_SCALING && u > OSQP_INF * MIN_SCALING;
  const bool eq = u - l < RHO_TOL;
  return loose ? -1 : (eq ? 1 : 0);
}
MPCQP_OSQP_FN double rho_of_row(int kind, double rho) {
  return kind == -1 ? RHO_MIN : (kind == 1 ? RHO_EQ_OVER_RHO_INEQ * rho : rho);
}

// ---- infeasibility certificates: the cone tests (is_primal_infeasible, is_dual_infeasible) ---------
// delta_y of one row projected onto the polar of the recession cone of [l, u]
MPCQP_OSQP_FN double polar_project(double dy, double l, double u) {
  if (u > OSQP_INF * MIN_SCALING) {
    if (l < -OSQP_INF * MIN_SCALING) dy = 0.0;
    else dy = min2(dy, 0.0);
  } else if (l < -OSQP_INF * MIN_SCALING) {
    dy = max2(dy, 0.0);
  }
  return dy;
}
// (A delta_x)_row = v leaves the recession cone of [l, u] by more than thr = eps_dual_inf ||delta_x||
MPCQP_OSQP_FN bool dual_ray_violates(double v, double l, double u, double thr) {
  return (u < OSQP_INF * MIN_SCALING && v > thr) || (l > -OSQP_INF * MIN_SCALING && v < -thr);
}

// ---- check_termination ------------------------------------------------------------------------------
MPCQP_OSQP_FN double tolerance(double eps_abs, double eps_rel, double norm) { return eps_abs + eps_rel * norm; }
// Status by precedence: solved, then primal infeasible, then dual infeasible; UNSOLVED = go on.
MPCQP_OSQP_FN int termination_status(bool prim_ok, bool dual_ok, bool prim_inf, bool dual_inf, bool approx) {
  if (prim_ok && dual_ok) return approx ? MPCQP_STATUS_SOLVED_INACCURATE : MPCQP_STATUS_SOLVED;
  if (prim_inf) return approx ? MPCQP_STATUS_PRIMAL_INFEASIBLE_INACCURATE : MPCQP_STATUS_PRIMAL_INFEASIBLE;
  if (dual_inf) return approx ? MPCQP_STATUS_DUAL_INFEASIBLE_INACCURATE : MPCQP_STATUS_DUAL_INFEASIBLE;
  return MPCQP_STATUS_UNSOLVED;
}
// The inf-norms of update_info / compute_pri_tol / compute_dua_tol / compute_rho_estimate, already
// reduced over the robot and merged where OSQP takes a max of several.  The first of each pair is of
// the unscaled problem (E^-1 / D^-1 applied), the `_s` one of the scaled problem (the rho estimate).
struct Norms {
  double pri, pri_s;              // |A~x - z|
  double prim_norm, prim_norm_s;  // max(|z|, |A~x|)
  double dua, dua_s;              // |P~x + q~ + A~'y|; dua_res = c^-1 dua
  double dual_norm, dual_norm_s;  // max(|q~|, |A~'y|, |P~x|)
};
// check_termination with the tests of scaled_termination = 0: the NON_CVX guard, every eps x 10 when
// `approx`, then the two residual tests.  prim_infeasible(eps_prim_inf) / dual_infeasible(eps_dual_inf)
// are the kernel's certificate tests; each is called only when its residual test fails.  They hold
// reductions and barriers, so every argument here must be the same in all threads of the robot.
template <class PrimInf, class DualInf>
MPCQP_OSQP_FN int check_termination(const mpcqp_params& p, bool approx, const Norms& nm, double cinv,
                                    PrimInf&& prim_infeasible, DualInf&& dual_infeasible) {
  double eps_abs = p.eps_abs, eps_rel = p.eps_rel, eps_pinf = p.eps_prim_inf, eps_dinf = p.eps_dual_inf;
  const double pri_res = nm.pri, dua_res = cinv * nm.dua;
  if (pri_res > OSQP_INF || dua_res > OSQP_INF) return MPCQP_STATUS_NON_CVX;
  if (approx) { eps_abs *= 10; eps_rel *= 10; eps_pinf *= 10; eps_dinf *= 10; }
  const bool prim_ok = pri_res < tolerance(eps_abs, eps_rel, nm.prim_norm);
  bool prim_inf = false, dual_inf = false;
  if (!prim_ok) prim_inf = prim_infeasible(eps_pinf);
  const bool dual_ok = dua_res < tolerance(eps_abs, eps_rel, cinv * nm.dual_norm);
  if (!dual_ok) dual_inf = dual_infeasible(eps_dinf);
  return termination_status(prim_ok, dual_ok, prim_inf, dual_inf, approx);
}

// ---- adapt_rho --------------------------------------------------------------------------------------
// compute_rho_estimate from the scaled residuals and their norms, clamped to [RHO_MIN, RHO_MAX]
MPCQP_OSQP_FN double rho_estimate(double rho, double pri, double pri_norm, double dua, double dua_norm) {
  const double pr_n = pri / (pri_norm + DIV_TOL);
  const double du_n = dua / (dua_norm + DIV_TOL);
  const double est = rho * __builtin_sqrt(pr_n / (du_n + DIV_TOL));
  return min2(max2(est, RHO_MIN), RHO_MAX);
}
// adapt_rho takes the estimate only when it left (rho / tol, rho tol), bounds excluded
MPCQP_OSQP_FN bool rho_moved(double est, double rho, double tol) { return est > rho * tol || est < rho / tol; }

// ---- when an iteration needs update_info ---------------------------------------------------------------
// Countdowns to the next termination check (iter % check_termination == 0) and the next adapt_rho step
// (iter % adaptive_rho_interval == 0); the last iteration needs update_info too.
struct InfoSchedule {
  // (in this order wave_kernel compiles to the instructions it had with two plain ints; the other
  // way round the allocator swaps the two counters' registers and adds a move)
  int to_adapt, to_check;
  MPCQP_OSQP_FN explicit InfoSchedule(const mpcqp_params& p)
      : to_adapt(p.adaptive_rho_interval), to_check(p.check_termination) {}
  // iterations from `iter` on that need no update_info, before the next one that does
  MPCQP_OSQP_FN int plain_ahead(const mpcqp_params& p, int iter) const {
    int plain = p.max_iter - iter;
    if (p.check_termination) plain = plain < to_check - 1 ? plain : to_check - 1;
    if (p.adaptive_rho) plain = plain < to_adapt - 1 ? plain : to_adapt - 1;
    return plain;
  }
  // one of those iterations has run
  MPCQP_OSQP_FN void plain_step(const mpcqp_params& p) {
    if (p.check_termination) --to_check;
    if (p.adaptive_rho) --to_adapt;
  }
  // iteration `iter` runs: what it is; returns whether it needs update_info
  MPCQP_OSQP_FN bool info_step(const mpcqp_params& p, int iter, bool& is_check, bool& is_adapt, bool& last) {
    is_check = is_adapt = false;
    if (p.check_termination && --to_check == 0) {
      is_check = true;
      to_check = p.check_termination;
    }
    if (p.adaptive_rho && --to_adapt == 0) {
      is_adapt = true;
      to_adapt = p.adaptive_rho_interval;
    }
    last = iter == p.max_iter;
    return is_check || is_adapt || last;
  }
};

// ---- an update_info iteration of osqp_solve ----------------------------------------------------------------
struct Verdict {
  int status;     // UNSOLVED: the loop goes on
  bool refactor;  // rho changed and another iteration follows
};
// The termination check of a check iteration or the last one; adapt_rho if the solve goes on; after the
// last iteration osqp_solve's approximate check, then MAX_ITER_REACHED.  check(approx) is the kernel's
// check_termination; rho and rho_updates are updated in place.
template <class Check>
MPCQP_OSQP_FN Verdict info_iteration(const mpcqp_params& p, bool is_check, bool is_adapt, bool last, const Norms& nm,
                                     double& rho, int& rho_updates, Check&& check) {
  Verdict v = {MPCQP_STATUS_UNSOLVED, false};
  if (is_check || last) v.status = check(false);
  if (v.status != MPCQP_STATUS_UNSOLVED) return v;
  if (is_adapt) {
    const double est = rho_estimate(rho, nm.pri_s, nm.prim_norm_s, nm.dua_s, nm.dual_norm_s);
    if (rho_moved(est, rho, p.adaptive_rho_tolerance)) {
      rho = est;
      rho_updates += 1;
      v.refactor = !last;
    }
  }
  if (last) {
    v.status = check(true);
    if (v.status == MPCQP_STATUS_UNSOLVED) v.status = MPCQP_STATUS_MAX_ITER_REACHED;
  }
  return v;
}

// ---- the result record ----------------------------------------------------------------------------------
MPCQP_OSQP_FN bool has_solution(int status) {
  return status != MPCQP_STATUS_PRIMAL_INFEASIBLE && status != MPCQP_STATUS_PRIMAL_INFEASIBLE_INACCURATE &&
         status != MPCQP_STATUS_DUAL_INFEASIBLE && status != MPCQP_STATUS_DUAL_INFEASIBLE_INACCURATE &&
         status != MPCQP_STATUS_NON_CVX;
}
// info->obj_val: the unscaled objective, +-OSQP_INFTY for an infeasibility certificate, NaN for NON_CVX
MPCQP_OSQP_FN double objective_of(int status, double scaled_obj, double cinv) {
  if (has_solution(status)) return scaled_obj * cinv;
  if (status == MPCQP_STATUS_PRIMAL_INFEASIBLE || status == MPCQP_STATUS_PRIMAL_INFEASIBLE_INACCURATE) return OSQP_INF;
  if (status == MPCQP_STATUS_DUAL_INFEASIBLE || status == MPCQP_STATUS_DUAL_INFEASIBLE_INACCURATE) return -OSQP_INF;
  return __builtin_nan("");
}
// the scalars of a result (everything but u0, f_body and nan_legs)
MPCQP_OSQP_FN void store_info(mpcqp_result* res, double obj_val, double pri_res, double dua_res, double rho, int status,
                              int iters, int rho_updates) {
  res->obj_val = obj_val;
  res->pri_res = pri_res;
  res->dua_res = dua_res;
  res->rho = rho;
  res->status = status;
  res->iters = iters;
  res->rho_updates = rho_updates;
}
// what the MPC kernels report for a record with a NaN or an infinity in it: nothing was solved
MPCQP_OSQP_FN mpcqp_result nan_input_result(const mpcqp_params& p) {
  mpcqp_result r;
  for (int k = 0; k < MPCQP_NUM_DOF; ++k) {
    r.u0[k] = __builtin_nan("");
    r.f_body[k] = 0.0;
  }
  store_info(&r, __builtin_nan(""), __builtin_nan(""), __builtin_nan(""), p.rho, MPCQP_STATUS_NAN_INPUT, 0, 0);
  r.nan_legs = 0xF;
  return r;
}

}  // namespace osqp
}  // namespace mpcqp
