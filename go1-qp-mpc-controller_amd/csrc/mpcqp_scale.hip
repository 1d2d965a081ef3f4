// mpcqp_scale.hip — OSQP scale_data (scaling.c) as a kernel of its own: scale_kernel, one multi-wave
// workgroup per robot (block barriers between its phases), launched before wave_kernel
// (mpcqp_wave.hip) on the same stream.
//
// Ruiz equilibration is embarrassingly parallel over the columns of P~ = c D H D, so it runs with
// one thread per column (NTS threads per robot).  It writes a per-robot image (ScaleImg: D, E, the
// scaled gradient q~, c, the warm-start branch, and for warm slots the raw gradient) that
// wave_kernel reads in place of a setup of its own, and zeroes wave_kernel's hand-off counters.
// H's columns come from a closed form (gen_col), so every norm is binary64.
#include "mpcqp_wave_common.h"

namespace mpcqp {
namespace wv {

template <int N>
struct ScaleCfg {
  static constexpr int n = ND * N, m = CD * N;
  static constexpr int TPC = 1;  // threads per column
  static constexpr int BPT = N;  // horizon blocks of the column per thread: all of them
  // at least two waves: wave 1 runs the degenerate-feet screen (one lane per horizon step) while
  // wave 0 runs the gradient sweep, so N <= 5 (n <= 60) still launches threads 64 .. 64 + N - 1
  static constexpr int NTS = ((n + 63) / 64) * 64 > 64 + N ? ((n + 63) / 64) * 64 : ((64 + N + 63) / 64) * 64;
  static constexpr int NWS = NTS / 64;
  // waves per SIMD the register allocation must allow (launch bounds): two, i.e. 256 VGPRs and no
  // spills.  N = 10: two waves per robot, four robots per CU; N = 20: four waves per robot, two per
  // CU (three per CU spilled 43 VGPRs: the same step time, 21 MB more HBM traffic per C4 solve,
  // profiles/r05/w20; three waves at N = 10 is slower, profiles/r05/sweep_reg)
  static constexpr int WPE = 2;
  static constexpr int RPT = (m + NTS - 1) / NTS;   // constraint rows per thread
};

template <int N>
struct ScaleSmem {
  using C = Cfg<N>;
  alignas(16) double Bw[N][3][ND];
  double rec[C::REC];
  double D[2][C::n], q[C::n], qn[C::n], E[2][C::m];  // D, E double-buffered over the Ruiz passes
  double lam[N][ND];
  double vec[2][16];
  double Ap[2][C::m];
  double red[2][16];
  double cm0[C::n];      // raw column norms of H (the first pass, D = 1)
  double red4[2][5 * 16];  // bound passes: per-wave partials, double-buffered by pass parity
};

// block-wide sum of sv and max of qv in one barrier (wave partials summed in wave order)
template <int NW>
__device__ __forceinline__ void block_sum_max(double& sv, double& qv, double (*red)[16]) {
  sv = wave_sum(sv);
  qv = wave_max(qv);
  if constexpr (NW > 1) {
    if ((threadIdx.x & 63) == 0) {
      red[0][threadIdx.x >> 6] = sv;
      red[1][threadIdx.x >> 6] = qv;
    }
    __syncthreads();
    double s = red[0][0], q = red[1][0];
#pragma unroll
    for (int i = 1; i < NW; ++i) {
      s += red[0][i];
      q = fmax(q, red[1][i]);
    }
    sv = s;
    qv = q;
  }
}

// MPCQP_SCALE_TIMING experiment builds: thread 0 of each robot overwrites the first doubles of its
// own record with {id, s_memtime} pairs (tools/scale_phases.py; the solve that follows is garbage)
#ifdef MPCQP_SCALE_TIMING
#define SC_MARK(id)                                                                     \
  do {                                                                                  \
    if (threadIdx.x == 0) {                                                             \
      double* tm_ = const_cast<double*>(recs) + (size_t)blockIdx.x * Cfg<N>::REC + 2 * (id); \
      tm_[0] = (id);                                                                    \
      tm_[1] = (double)__builtin_readcyclecounter();                                    \
    }                                                                                   \
  } while (0)
#else
#define SC_MARK(id) \
  do {              \
  } while (0)
#endif
template <int N>
__global__ __launch_bounds__(ScaleCfg<N>::NTS, ScaleCfg<N>::WPE) void scale_kernel(const double* __restrict__ recs, int batch,
                                                                 double* __restrict__ wstate,
                                                                 double* __restrict__ img, mpcqp_params p,
                                                                 int* __restrict__ fb, const int* __restrict__ type,
                                                                 int want) {
  using C = Cfg<N>;
  using SC = ScaleCfg<N>;
  using WL = WarmLayout<N>;
  using SI = ScaleImg<N>;
  constexpr int n = C::n, m = C::m, NTS = SC::NTS;
  static_assert(NTS >= 64 + N, "wave 1 screens one horizon step per lane");
  __shared__ ScaleSmem<N> sm;
  const int inst = blockIdx.x;
  if (inst >= batch) return;
  const int t = threadIdx.x;
#ifdef MPCQP_SCALE_TIMING
  const double t_entry = (double)__builtin_readcyclecounter();
#endif
  // wave_kernel's hand-off counters start at zero (stream order): [0] rank-deficient feet, [1] a KKT
  // solve that cancelled too much for its core (S_max * amp > SCHUR_AMP), [2] S_max > SCHUR_SMAX
  if (inst == 0 && t < 3) fb[t] = 0;
  // typed solve: a robot of the other control type keeps its warm slot (the zero-pattern mask below)
  if (type && type[inst] != want) return;
  {
    const double* rg = recs + (size_t)inst * C::REC;
    int bad = 0;
    for (int e = t; e < C::REC; e += NTS) {
      const double v = rg[e];
      sm.rec[e] = v;
      bad |= !isfinite(v);
    }
    if (__syncthreads_or(bad)) return;  // wave_kernel reports the non-finite record
  }
  SC_MARK(0);
#ifdef MPCQP_SCALE_TIMING
  if (t == 0) {  // kernel entry (before the record load), kept until the record's first words are read
    double* tm_ = const_cast<double*>(recs) + (size_t)blockIdx.x * Cfg<N>::REC + 14;
    tm_[0] = 7;
    tm_[1] = t_entry;
  }
#endif
  const double* rec = sm.rec;
  const double dt = rec[MPCQP_REC_DT], mass = rec[MPCQP_REC_MASS], mu = rec[MPCQP_REC_MU];
  Adisc A;
  {
    const double yaw = rec[MPCQP_REC_EULER + 2];
    A.ad0 = cos(yaw) * dt;
    A.ad1 = sin(yaw) * dt;
    A.dt = dt;
  }
  const double dtm = (1.0 / mass) * dt;
  // B_d(k) rows 6-8 (calculate_B_mat_c, Utils.cpp:35-41), gradient adjoint (ConvexMpc.cpp:215-217)
  bool any_degen;
  {
    int degen = 0;
    double Iwinv[9];
    iw_inverse(rec, Iwinv);
    for (int e = t; e < N * 36; e += NTS) {
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
    // forward: a_i = A_d^{i+1} x0 (13 states), e_i = 2q (a_i - x_ref_i); backward: lambda_j = e_j + A' lambda_{j+1}
    // (sequential over the horizon: wave 0 alone, wave-synchronous; one block barrier at the end)
    if (t < 64) {
      if (t < SD) sm.vec[0][t] = rec[MPCQP_REC_X0 + t];
      // 2 q of the lane's state, loaded once (indexed by the lane, it is a memory round trip: inside
      // the sweep it was one per step)
      double q2t = 2 * p.q_weights[t < ND ? t : 0];
      keep(q2t);
      // Branch-free rows of A_d (forward) and A_d' (backward): lane t's row is
      // fma(c2, v[j2], fma(c1, v[j1], v[t])), the unused terms with a zero coefficient (exact: the
      // operands are finite).  Per-lane branches serialized the rows, each with its own LDS wait.
      const int tr = t < SD ? t : 0;
      const int fj1 = tr <= 1 ? 6 : (tr == 2 ? 8 : (tr <= 5 ? tr + 6 : (tr == 11 ? 12 : tr)));
      const double fc1 = tr == 0 ? A.ad0 : (tr == 1 ? -A.ad1 : ((tr <= 5 || tr == 11) ? dt : 0.0));
      const int fj2 = tr <= 1 ? 7 : tr;
      const double fc2 = tr == 0 ? A.ad1 : (tr == 1 ? A.ad0 : 0.0);
      const int bj1 = tr == 6 || tr == 7 ? 0 : (tr == 8 ? 2 : (tr >= 9 && tr < ND ? tr - 6 : tr));
      const double bc1 = tr == 6 ? A.ad0 : (tr == 7 ? A.ad1 : ((tr >= 8 && tr < ND) ? dt : 0.0));
      const int bj2 = tr == 6 || tr == 7 ? 1 : tr;
      const double bc2 = tr == 6 ? -A.ad1 : (tr == 7 ? A.ad0 : 0.0);
      wave_sync();
      for (int i = 0; i < N; ++i) {
        if (t < SD) {
          const double* pv = sm.vec[i & 1];
          const double s = fma(fc2, pv[fj2], fma(fc1, pv[fj1], pv[tr]));
          sm.vec[(i + 1) & 1][t] = s;
          if (t < ND) sm.lam[i][t] = q2t * (s - rec[MPCQP_REC_XREF + SD * i + t]);
        }
        wave_sync();
      }
      for (int j = N - 2; j >= 0; --j) {
        if (t < ND) {
          const double* v = sm.lam[j + 1];
          sm.lam[j][t] = sm.lam[j][t] + fma(bc2, v[bj2], fma(bc1, v[bj1], v[tr]));
        }
        wave_sync();
      }
      SC_MARK(8);
    } else if (N <= 10 && t < 64 + N) {  // (the Schur form serves N <= 10 only: no screen beyond)
      // Degenerate-foot screen for the Schur form (wave_kernel KS = 1), by wave 1 while wave 0 runs
      // the sweep: per step k the Cholesky pivots of the Gram matrix B6_k B6_k' (B6 = rows 6-11 of
      // B_d(k): I_w^-1 [r_l]x dt and dt/m sums) relative to its diagonal.  Collinear feet give rank
      // 5, coincident feet rank 3; a pivot ratio below SCHUR_GRAM_TOL sends the robot to the Riccati
      // form.  (Go1 workloads: smallest ratio ~0.12; with R'^-1 between B6 and B6' (spread <= ~1e3)
      // the Schur form then factors G_k with pivot ratios above ~1e-9.)
      const int k = t - 64;
      double bw[3][ND];
#pragma unroll
      for (int lg = 0; lg < 4; ++lg) {
        const double* fp = rec + MPCQP_REC_FEET(N) + 12 * k + 3 * lg;
#pragma unroll
        for (int rr = 0; rr < 3; ++rr) {  // (I_w^-1 [r]x)[rr][c3] = sum_e Iwinv[rr][e] skew[e][c3]
          const double i0 = Iwinv[3 * rr], i1 = Iwinv[3 * rr + 1], i2 = Iwinv[3 * rr + 2];
          bw[rr][3 * lg + 0] = (i1 * fp[2] - i2 * fp[1]) * dt;
          bw[rr][3 * lg + 1] = (i2 * fp[0] - i0 * fp[2]) * dt;
          bw[rr][3 * lg + 2] = (i0 * fp[1] - i1 * fp[0]) * dt;
        }
      }
      double G[21];  // lower triangle, row-major packed; Cholesky in place
      auto gi = [](int r1, int r2) { return r1 * (r1 + 1) / 2 + r2; };
#pragma unroll
      for (int r1 = 0; r1 < 6; ++r1)
#pragma unroll
        for (int r2 = 0; r2 <= r1; ++r2) {
          double g = 0.0;
          if (r1 < 3) {
#pragma unroll
            for (int b = 0; b < ND; ++b) g += bw[r1][b] * bw[r2][b];
          } else if (r2 < 3) {
#pragma unroll
            for (int l = 0; l < 4; ++l) g += bw[r2][3 * l + (r1 - 3)] * dtm;
          } else {
            g = r1 == r2 ? 4.0 * dtm * dtm : 0.0;
          }
          G[gi(r1, r2)] = g;
        }
#pragma unroll
      for (int c = 0; c < 6; ++c) {
        const double d0 = G[gi(c, c)];
        double sc = d0;
#pragma unroll
        for (int e = 0; e < c; ++e) sc -= G[gi(c, e)] * G[gi(c, e)];
        degen |= !(sc > SCHUR_GRAM_TOL * d0);
        const double dg = sqrt(dmax(sc, 0.0)), di = dg > 0.0 ? 1.0 / dg : 0.0;
        G[gi(c, c)] = dg;
#pragma unroll
        for (int r1 = c + 1; r1 < 6; ++r1) {
          double v = G[gi(r1, c)];
#pragma unroll
          for (int e = 0; e < c; ++e) v -= G[gi(r1, e)] * G[gi(c, e)];
          G[gi(r1, c)] = v * di;
        }
      }
    }
    // (a block-uniform flag: nothing else of the screen stays live through the Ruiz passes)
    any_degen = __syncthreads_or(degen) != 0;
  }
  // thread t: column j0 = t of H, blocks jb .. jb+BPT-1 of it, i.e. all N from jb = 0.  (j0 as a
  // copy of t and jb as an expression in t are kept on purpose: with t and a literal 0 in their
  // places the compiler schedules this kernel differently, and its code is held fixed.)
  constexpr int BPT = SC::BPT;
  const int j0 = t;
  const int jb = (t % SC::TPC) * BPT;
  SC_MARK(1);
  // D and E of the current pass (each pass writes the other buffer: no read-before-write barrier)
  double* Dc = sm.D[0];
  double* Ec = sm.E[0];
  if (j0 < n) {
    const int k = j0 / ND, ii = j0 % ND;
    const double* lm = sm.lam[k];
    const double g = ((sm.Bw[k][0][ii] * lm[6] + sm.Bw[k][1][ii] * lm[7]) + sm.Bw[k][2][ii] * lm[8]) + dtm * lm[9 + ii % 3];
    sm.q[j0] = g;
    sm.qn[j0] = g;
    Dc[j0] = 1.0;
  }
  for (int r = t; r < m; r += NTS) {
    Ec[r] = 1.0;
    const int a5 = r % 5;  // friction pyramid rows (ConvexMpc.cpp:46-58)
    sm.Ap[0][r] = a5 < 4 ? 1.0 : 0.0;
    sm.Ap[1][r] = a5 < 4 ? ((a5 & 1) ? -mu : mu) : 1.0;
  }
  __syncthreads();
  double* const ws = wstate ? wstate + (size_t)inst * WL::SIZE : nullptr;
  const bool had = ws && ws[WL::FLAG] != 0.0;
  // max_i D_i |H_ij0| over the thread's column
  auto colmax = [&]() __attribute__((always_inline)) -> double {
    double mx0 = 0.0, mx1 = 0.0;
    if (j0 < n) {
      gen_col<N, BPT, false>(sm, p, A, dtm, j0, jb, [&](int, int b, int ri, double hv) __attribute__((always_inline)) {
        if (b & 1) mx1 = fmax(mx1, Dc[ri] * dabs(hv));
        else mx0 = fmax(mx0, Dc[ri] * dabs(hv));
      });
    }
    return fmax(mx0, mx1);
  };
  // H's zero pattern (sparseView) of column j0's upper triangle vs the previous tick's: decides
  // between osqp_update_P and OsqpEigen's re-init (oracle ws_update)
  auto pattern = [&]() __attribute__((always_inline)) -> bool {
    unsigned long long zm[WL::MW];
#pragma unroll
    for (int w = 0; w < WL::MW; ++w) zm[w] = 0ull;
    auto put = [&](int, int, int ri, double hv) __attribute__((always_inline)) {
      const unsigned long long bit = (hv == 0.0 && ri <= j0) ? (1ull << (ri & 63)) : 0ull;
#pragma unroll
      for (int w = 0; w < WL::MW; ++w) zm[w] |= (ri >> 6) == w ? bit : 0ull;
    };
    if (j0 < n) gen_col<N, BPT, false>(sm, p, A, dtm, j0, jb, put);
    bool diff = false;
    if (j0 < n) {
      double* slot = ws + WL::MASK + WL::MW * j0;
#pragma unroll
      for (int w = 0; w < WL::MW; ++w) {
        diff |= __double_as_longlong(slot[w]) != (long long)zm[w];
        slot[w] = __longlong_as_double((long long)zm[w]);
      }
    }
    return diff;
  };
  // A~ column / row norms, branch-free (every operand loaded, the case selected after: per-lane
  // branches ran the cases one after another, each with its own LDS wait)
  auto acol = [&](int j) __attribute__((always_inline)) {
    const int f = j / 3, aa = j % 3;
    const double* e = Ec + 5 * f;
    const double* a0 = sm.Ap[0] + 5 * f;
    const double* a1 = sm.Ap[1] + 5 * f;
    const double e0 = e[0], e1 = e[1], e2 = e[2], e3 = e[3], e4 = e[4];
    const double m0 = dmax(e0 * dabs(a0[0]), e1 * dabs(a0[1]));
    const double m1 = dmax(e2 * dabs(a0[2]), e3 * dabs(a0[3]));
    const double m2 = dmax(dmax(dmax(dmax(dabs(a1[0]) * e0, dabs(a1[1]) * e1), dabs(a1[2]) * e2), dabs(a1[3]) * e3),
                           e4 * dabs(a1[4]));
    return sel3(aa, m0, m1, m2) * Dc[j];
  };
  auto arow = [&](int r) __attribute__((always_inline)) {
    const int f = r / 5, k5 = r % 5;
    const double e = Ec[r];
    const double* d = Dc + 3 * f;
    const double a0r = sm.Ap[0][r], a1r = sm.Ap[1][r], dk = d[k5 < 4 ? k5 >> 1 : 0], d2 = d[2];
    const double m4 = (e * dabs(a1r)) * d2;
    const double m03 = dmax((e * dabs(a0r)) * dk, (dabs(a1r) * e) * d2);
    return k5 == 4 ? m4 : m03;
  };
  double c_s = 1.0, cm = 0.0;
  // First column pass (D = 1): the raw norms, and H's zero pattern (warm start only): same pattern
  // -> osqp_update_P (unscale with the old scaling, rescale with the previous A and q, keep iterates
  // and rho); a changed pattern or mu -> re-init (fresh scaling and rho, the previous unscaled x, y)
  bool pattern_changed = false;
  SC_MARK(2);
  // The raw norms only enter the bound-decided passes below, where an upper bound serves as well
  // (their tests then err on the side of the exact passes): for nonnegative weights H is symmetric
  // positive semidefinite, so max_i |H_ij| <= sqrt(H_jj max_i H_ii), from H's diagonal alone (one
  // block of column j instead of N; the margin covers the roundings of the computed entries).  The
  // first pass, which compares the raw norm itself with |A col j|, takes the bound only when the
  // bound already loses that comparison in every column (checked below; else the exact norms).
  bool cm_ub = true;
  for (int i = 0; i < ND; ++i) cm_ub = cm_ub && p.q_weights[i] >= 0.0 && p.r_weights[i % MPCQP_NUM_DOF] >= 0.0;
  auto colmax_ub = [&]() __attribute__((always_inline)) -> double {
    double hd = 0.0;
    if (j0 < n) {
      const int a2 = j0 % ND;
      gen_col<N, 1, true>(sm, p, A, dtm, j0, j0 / ND, [&](int, int b, int, double hv) __attribute__((always_inline)) {
        hd = b == a2 ? hv : hd;
      });
    }
    double unused = 0.0, hm = hd;
    block_sum_max<SC::NWS>(unused, hm, sm.red);
    return sqrt(dmax(hd, 0.0) * hm) * (1.0 + 0x1p-20);
  };
  if (p.scaling > 0 || ws) {
    cm = cm_ub ? colmax_ub() : colmax();
    if (ws) pattern_changed = __syncthreads_or(pattern()) != 0;
  }
  // A is set once per solver init (A1RobotControl.cpp:526-530); a changed mu re-initializes
  const bool mu_changed = had && ws[WL::MU] != mu;
  const int mode = !had ? 0 : ((pattern_changed || mu_changed) ? 2 : 1);  // 0 cold, 1 update_P, 2 re-init
  if (mode == 1) {
    // unscale_data with the previous scaling: q = D^-1 (c^-1 q~), A = (E^-1 A~) D^-1
    const double cinv_o = 1. / ws[WL::C];
    if (j0 < n) sm.q[j0] = (1. / ws[WL::D + j0]) * (cinv_o * ws[WL::QT + j0]);
    for (int r = t; r < m; r += NTS) {
      const int f = r / 5, k5 = r % 5;
      const double ei = 1. / ws[WL::E + r];
      const double d2 = 1. / ws[WL::D + 3 * f + 2];
      sm.Ap[0][r] = k5 < 4 ? (ws[WL::AK + r] * ei) * (1. / ws[WL::D + 3 * f + (k5 >> 1)]) : 0.0;
      sm.Ap[1][r] = (ws[WL::AK + m + r] * ei) * d2;
    }
    __syncthreads();
  }
  SC_MARK(3);
  // Ruiz passes decided by bounds.  A pass uses the column norms cm_j = max_i D_i |H_ij| of the
  // D-scaled P twice: in the cost normalization (c_temp = 1 / max(mean_j c D_j cm_j, |q|_inf)) and
  // in the next pass's fmax(c D_j cm_j, |A~ col j|).  With cm0_j = max_i |H_ij| (the raw pass,
  // D = 1) and Dmax = max_i D_i, fl(D_i |H_ij|) <= fl(Dmax cm0_j) (rounding is monotone); where
  // these bounds, with a margin for the roundings of the sums and products, already let |q|_inf win
  // the normalization and the A~ norm win every column's fmax, the exact norms cannot change a bit
  // of the result.  Such a pass is per-foot work — A is block diagonal over the feet (5 rows x 3
  // columns) — done by one thread per foot in place, plus one block reduction (sum c D_j cm0_j,
  // max |q_j|, max D_j, min_j |A~ col j| / (D_j cm0_j)).  The first pass the bounds cannot decide
  // and all after it run the exact passes below.  (Go1 workloads: every pass of every robot is
  // decided by the bounds, H's entries being far below A's unit entries.)
  if (j0 < n) sm.cm0[j0] = cm;
  __syncthreads();
  if (cm_ub && p.scaling > 0) {
    // the first pass's fmax(c D_j cm_j, |A~ col j| D_j) with c = D_j = E_i = 1: the bound must lose it
    // (then the raw norm, at most the bound, loses it too and the pass is the same)
    bool wins = false;
    if (t < 4 * N) {
      const double* a0 = sm.Ap[0] + 5 * t;
      const double* a1 = sm.Ap[1] + 5 * t;
      const double* cz = sm.cm0 + 3 * t;
      const double m0 = dmax(Ec[5 * t] * dabs(a0[0]), Ec[5 * t + 1] * dabs(a0[1]));
      const double m1 = dmax(Ec[5 * t + 2] * dabs(a0[2]), Ec[5 * t + 3] * dabs(a0[3]));
      const double m2 = dmax(dmax(dmax(dmax(dabs(a1[0]) * Ec[5 * t], dabs(a1[1]) * Ec[5 * t + 1]),
                                       dabs(a1[2]) * Ec[5 * t + 2]), dabs(a1[3]) * Ec[5 * t + 3]),
                             Ec[5 * t + 4] * dabs(a1[4]));
      wins = !(cz[0] <= m0 * Dc[3 * t]) || !(cz[1] <= m1 * Dc[3 * t + 1]) || !(cz[2] <= m2 * Dc[3 * t + 2]);
    }
    if (__syncthreads_or(wins)) {
      cm = colmax();
      if (j0 < n) sm.cm0[j0] = cm;
      __syncthreads();
    }
  }
  int pass = 0;
  bool resume = false;  // the bound passes stopped after the D, E, q update of `pass`
  {
    constexpr int NF = 4 * N;
    constexpr double EPS = 2.220446049250313e-16;
    constexpr double M1 = 1.0 + 4.0 * (n + 8) * EPS;  // sum / product margin of the normalization test
    constexpr double M2 = 1.0 + 16.0 * EPS;           // product margin of the fmax test
    double dmax_prev = 1.0;                           // Dmax of the previous pass (ub_j = Dmax cm0_j)
    for (; pass < p.scaling; ++pass) {
      if (pass == 1) SC_MARK(4);
      double s0 = 0.0, qm = 0.0, dm = 0.0, rmin = INFINITY, moved = 0.0;
      if (t < NF) {
        const int f = t;
        double e[5], a0[5], a1[5], d[3], cz[3];
#pragma unroll
        for (int i = 0; i < 5; ++i) {
          e[i] = Ec[5 * f + i];
          a0[i] = sm.Ap[0][5 * f + i];
          a1[i] = sm.Ap[1][5 * f + i];
        }
#pragma unroll
        for (int i = 0; i < 3; ++i) {
          d[i] = Dc[3 * f + i];
          cz[i] = sm.cm0[3 * f + i];
        }
        // |A~ col| of the foot's fx, fy, fz columns without D (acol above, same operations)
        auto acol3 = [&](const double (&ee)[5], double (&mc)[3]) __attribute__((always_inline)) {
          mc[0] = dmax(ee[0] * dabs(a0[0]), ee[1] * dabs(a0[1]));
          mc[1] = dmax(ee[2] * dabs(a0[2]), ee[3] * dabs(a0[3]));
          mc[2] = dmax(dmax(dmax(dmax(dabs(a1[0]) * ee[0], dabs(a1[1]) * ee[1]), dabs(a1[2]) * ee[2]),
                            dabs(a1[3]) * ee[3]),
                       ee[4] * dabs(a1[4]));
        };
        double mc[3];
        acol3(e, mc);
        double dtv[3], et[5];
#pragma unroll
        for (int i = 0; i < 3; ++i) {
          const double cmj = pass == 0 ? cz[i] : dmax_prev * cz[i];
          const double pc = (c_s * d[i]) * cmj;
          dtv[i] = limit_scaling(fmax(pc, mc[i] * d[i]));
        }
#pragma unroll
        for (int i = 0; i < 5; ++i) {  // arow above
          const double dk = d[i < 4 ? i >> 1 : 0], d2 = d[2];
          const double m4 = (e[i] * dabs(a1[i])) * d2;
          const double m03 = dmax((e[i] * dabs(a0[i])) * dk, (dabs(a1[i]) * e[i]) * d2);
          et[i] = limit_scaling(i == 4 ? m4 : m03);
        }
        // 1 / sqrt of the limited norms; 1 / sqrt(1) = 1 exactly, and on the Go1 workloads every
        // norm is 1 (unit friction-pyramid entries, D = E = 1): the wave skips the divisions then
        bool ne1 = false;
#pragma unroll
        for (int i = 0; i < 3; ++i) ne1 |= dtv[i] != 1.0;
#pragma unroll
        for (int i = 0; i < 5; ++i) ne1 |= et[i] != 1.0;
        if (__any(ne1)) {
#pragma unroll
          for (int i = 0; i < 3; ++i) dtv[i] = 1.0 / sqrt(dtv[i]);
#pragma unroll
          for (int i = 0; i < 5; ++i) et[i] = 1.0 / sqrt(et[i]);
        }
        moved = ne1 ? 1.0 : 0.0;
#pragma unroll
        for (int i = 0; i < 5; ++i) {
          e[i] = e[i] * et[i];
          Ec[5 * f + i] = e[i];
        }
#pragma unroll
        for (int i = 0; i < 3; ++i) {
          const double qj = dtv[i] * sm.q[3 * f + i];
          sm.q[3 * f + i] = qj;
          d[i] = d[i] * dtv[i];
          Dc[3 * f + i] = d[i];
          s0 += (c_s * d[i]) * cz[i];
          qm = dmax(qm, dabs(qj));
          dm = dmax(dm, d[i]);
        }
        acol3(e, mc);  // the next pass's A~ norms
#pragma unroll
        for (int i = 0; i < 3; ++i) {
          const double den = d[i] * cz[i];
          rmin = fmin(rmin, den > 0.0 ? (mc[i] * d[i]) / den : INFINITY);
        }
      }
      {  // one block reduction; partials double-buffered by pass parity (no second barrier)
        s0 = wave_sum(s0);
        qm = wave_max(qm);
        dm = wave_max(dm);
        rmin = -wave_max(-rmin);
        moved = wave_max(moved);
        double* pr = sm.red4[pass & 1];
        if ((t & 63) == 0) {
          pr[5 * (t >> 6) + 0] = s0;
          pr[5 * (t >> 6) + 1] = qm;
          pr[5 * (t >> 6) + 2] = dm;
          pr[5 * (t >> 6) + 3] = rmin;
          pr[5 * (t >> 6) + 4] = moved;
        }
        __syncthreads();
        s0 = pr[0];
        qm = pr[1];
        dm = pr[2];
        rmin = pr[3];
        moved = pr[4];
#pragma unroll
        for (int w = 1; w < SC::NWS; ++w) {
          s0 += pr[5 * w];
          qm = dmax(qm, pr[5 * w + 1]);
          dm = dmax(dm, pr[5 * w + 2]);
          rmin = fmin(rmin, pr[5 * w + 3]);
          moved = dmax(moved, pr[5 * w + 4]);
        }
      }
      const double inf_norm_q = limit_scaling(qm);
      const double c_temp = 1. / limit_scaling(inf_norm_q);
      const double c_new = c_s * c_temp;
      const bool ok1 = ((dm * s0) * M1) / n <= inf_norm_q;
      const bool ok2 = pass + 1 == p.scaling || (c_new * dm) * M2 <= rmin;
      if (!(ok1 && ok2)) {  // (block-uniform)
        resume = true;
        break;
      }
      if (t < NF) {
#pragma unroll
        for (int i = 0; i < 3; ++i) sm.q[3 * t + i] *= c_temp;
      }
      // A pass that moved nothing (every 1/sqrt factor 1, c_temp 1, the same Dmax) leaves the next
      // pass exactly the same inputs: every remaining pass is the identity.  (Go1 workloads: from
      // the second or third pass on.)
      const bool fixed = moved == 0.0 && c_temp == 1.0 && dm == dmax_prev;
      c_s = c_new;
      dmax_prev = dm;
      if (fixed) {
        pass = p.scaling;
        break;
      }
    }
  }
  // exact passes: H's columns regenerated for the norms
  for (; pass < p.scaling; ++pass) {
    if (!resume) {
      if (pass == 1) SC_MARK(4);
      // new scaling factors from the current D, E (every thread reads before anyone writes)
      double dtv = 1.0;
      if (j0 < n) {
        const double pc = (c_s * Dc[j0]) * cm;
        dtv = 1.0 / sqrt(limit_scaling(fmax(pc, acol(j0))));
      }
      double et[SC::RPT];
#pragma unroll
      for (int rr = 0; rr < SC::RPT; ++rr) {
        const int r = t + NTS * rr;
        et[rr] = r < m ? 1.0 / sqrt(limit_scaling(arow(r))) : 1.0;
      }
      double* const Dn = Dc == sm.D[0] ? sm.D[1] : sm.D[0];
      double* const En = Ec == sm.E[0] ? sm.E[1] : sm.E[0];
#pragma unroll
      for (int rr = 0; rr < SC::RPT; ++rr) {
        const int r = t + NTS * rr;
        if (r < m) En[r] = Ec[r] * et[rr];
      }
      if (j0 < n) {
        sm.q[j0] = dtv * sm.q[j0];
        Dn[j0] = Dc[j0] * dtv;
      }
      Dc = Dn;
      Ec = En;
    }
    resume = false;
    __syncthreads();
    cm = colmax();  // column norms of the D-scaled P (cost normalization)
    double sv = 0.0, qv = 0.0;
    if (j0 < n) {
      sv = (c_s * Dc[j0]) * cm;
      qv = dabs(sm.q[j0]);
    }
    block_sum_max<SC::NWS>(sv, qv, sm.red);
    double c_temp = sv / n;
    const double inf_norm_q = limit_scaling(qv);
    c_temp = dmax(c_temp, inf_norm_q);
    c_temp = limit_scaling(c_temp);
    c_temp = 1. / c_temp;
    if (j0 < n) sm.q[j0] *= c_temp;  // own column only: no barrier before the next pass
    c_s *= c_temp;
  }
  __syncthreads();
  SC_MARK(5);
  double* out = img + (size_t)inst * SI::SIZE;
  // (the A entries the passes used are not handed over: wave_kernel derives them from mu or the
  // warm slot as above; this tick's raw gradient only matters to osqp_update_P, i.e. warm slots)
  if (j0 < n) {
    out[SI::D + j0] = Dc[j0];
    out[SI::Q + j0] = sm.q[j0];
    if (ws) out[SI::QN + j0] = sm.qn[j0];
  }
  for (int r = t; r < m; r += NTS) out[SI::E + r] = Ec[r];
  // The Schur form's hand-off flag: 1 for rank-deficient B6_k (the screen above).  (Evaluating max
  // S_ii at the initial rho here as well was measured and dropped: at rho = 0.1 no C5 or heavy-weight
  // robot crosses SCHUR_SMAX -- with OSQP's cost scaling S barely grows with the state weights; the
  // crossings come after adapt_rho lowers rho -- and it cost scale_kernel 11 %, profiles/r05.)
  const double flag = any_degen ? 1.0 : 0.0;
  if (t == 0) {
    out[SI::CS] = c_s;
    out[SI::MODE] = (double)mode;
    out[SI::DEGEN] = flag;
  }
  SC_MARK(6);
}
#undef SC_MARK

}  // namespace wv

template <int N>
static hipError_t launch_scale(const LaunchArgs& a) {
  if (!a.fallback) return hipErrorInvalidValue;
  hipLaunchKernelGGL((wv::scale_kernel<N>), dim3(a.batch), dim3(wv::ScaleCfg<N>::NTS), 0, (hipStream_t)a.stream,
                     a.recs, a.batch, a.wstate, a.work, a.p, a.fallback, a.type, a.want);
  return hipGetLastError();
}
hipError_t launch_scale_any(const LaunchArgs& a) {
  switch (a.p.horizon) {
#define CASE(K) \
  case K: return launch_scale<K>(a);
    MPCQP_WAVE_FOR_EACH_N(CASE)
#undef CASE
    default: return hipErrorInvalidValue;
  }
}

}  // namespace mpcqp
