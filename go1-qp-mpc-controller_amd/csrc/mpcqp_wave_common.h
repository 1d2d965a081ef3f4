// mpcqp_wave_common.h — device pieces that at least two of the scaling kernel (mpcqp_scale.hip), the
// two forms of the solve kernel's KKT solve (mpcqp_schur.h, mpcqp_wave_riccati.h) and the solve
// kernel itself (mpcqp_wave.hip) use: lane layout, cross-lane primitives, the discrete dynamics, the
// MFMA tile layout, the thresholds, H's columns (gen_col) and the scale_kernel image layout.
// Not installed.
#pragma once
#include <type_traits>

#include "mpcqp_device.h"

namespace mpcqp {
namespace wv {

constexpr int NT = 64;
__host__ __device__ constexpr int gray(int v) { return v == 2 ? 3 : (v == 3 ? 2 : v); }  // own inverse
__host__ __device__ constexpr int row_of(int k) { return gray(k & 3); }  // DPP row of horizon step k

template <int N>
struct Cfg {
  static constexpr int n = ND * N, m = CD * N, R = (N + 3) / 4, NH = n * (n + 1) / 2;
  static constexpr int REC = MPCQP_REC_SIZE(N);
};

// Warm-start slot of one robot (binary64, caller-owned device memory): everything the reference's
// persistent OsqpEigen solver carries from one tick to the next.  Scaled quantities are stored as
// the kernel used them; the zero pattern of H's upper triangle (one bit per entry, MW words per
// column) and the friction coefficient mu the constraint matrix was built with decide between
// osqp_update_P and OsqpEigen's re-init on the next tick.
template <int N>
struct WarmLayout {
  static constexpr int n = ND * N, m = CD * N, MW = (n + 63) / 64;
  static constexpr int FLAG = 0, RHO = 1, C = 2, MU = 3, D = 4, E = D + n, QT = E + m, AK = QT + n, X = AK + 2 * m,
                       Z = X + n, Y = Z + m, MASK = Y + m, SIZE = MASK + MW * n;
  static_assert(SIZE == warm_state_doubles(N), "warm-start slot layout");
};

// ---- DPP wait states in the inline-asm blocks -------------------------------------------------
// A DPP instruction reads its src0 at least 2 wait states after a VALU write of it, and at least 5
// after a VALU write of EXEC (v_cmpx, which these kernels never emit; tools/isa_hazards.py checks
// both in the compiled code).  An s_nop is not free for a lone wave: s_nop 1 costs 8.4 cycles on
// MI355X, as much as two f64 FMAs (tools/mb/mb_valu).  The compiler cannot see into an asm block, so
// each block that may follow the VALU write of its src0 starts with a wait: WV_NOP_HEAD (2 states).
// A block whose src0 an earlier block of the same sequence already read (the sources of a sequence are
// materialized together before its first block) waits for nothing (WV_NOP_INNER).  tools/isa_hazards.py
// verifies the placement on the compiled product kernels (tests/test_isa_hazards.py).  Against the
// round-4 placement (s_nop 4 / s_nop 1 at every block): C2 1.737 -> 1.677 ms, C4 6.75 -> 6.20 ms,
// bitwise equal results (profiles/r05/nop_lean).
#define WV_NOP_HEAD "s_nop 1\n\t"
#define WV_NOP_INNER ""
#define WV_NOP_HEAD1 "s_nop 1\n\t"
#define WV_NOP_INNER1 ""
#define WV_NOP_PERM "s_nop 0\n\t"

// ---- cross-lane primitives ---------------------------------------------------------------------
// quad_perm DPP of a double
constexpr int QP_PRIM = 0x50;  // [0,0,1,1]: row lane a reads variable a>>1 (fx: rows 0,1; fy: rows 2,3)
constexpr int QP_B0 = 0x00, QP_B1 = 0x55, QP_B2 = 0xAA, QP_B3 = 0xFF;  // quad broadcasts
constexpr int QP_02 = 0x08;  // [0,2,0,0]
constexpr int QP_13 = 0x5D;  // [1,3,1,1]
constexpr int QP_X1 = 0xB1, QP_X2 = 0x4E;

// Move a per-row vector from DPP row FROM to row TO (rows one bit apart).  permlane16_swap(v, v)
// returns {v with odd rows := even rows, v with even rows := odd rows}; permlane32_swap likewise
// for row pairs (0,2), (1,3).
template <int FROM, int TO>
__device__ __forceinline__ double rmove(double v) {
  static_assert((FROM ^ TO) == 1 || (FROM ^ TO) == 2, "rows must differ in one bit");
  const unsigned lo = (unsigned)__double2loint(v), hi = (unsigned)__double2hiint(v);
  if constexpr ((FROM ^ TO) == 1) {
    const auto l2 = __builtin_amdgcn_permlane16_swap(lo, lo, false, false);
    const auto h2 = __builtin_amdgcn_permlane16_swap(hi, hi, false, false);
    return FROM < TO ? __hiloint2double((int)h2[0], (int)l2[0]) : __hiloint2double((int)h2[1], (int)l2[1]);
  } else {
    const auto l2 = __builtin_amdgcn_permlane32_swap(lo, lo, false, false);
    const auto h2 = __builtin_amdgcn_permlane32_swap(hi, hi, false, false);
    return FROM < TO ? __hiloint2double((int)h2[0], (int)l2[0]) : __hiloint2double((int)h2[1], (int)l2[1]);
  }
}

// rmove without register copies: one permlane swap per dword (the source's other rows are
// clobbered, the result's other rows are undefined).
template <int FROM, int TO>
__device__ __forceinline__ double rmove2(double v) {
  static_assert((FROM ^ TO) == 1 || (FROM ^ TO) == 2, "rows must differ in one bit");
  unsigned lo = (unsigned)__double2loint(v), hi = (unsigned)__double2hiint(v), ol, oh;
  if constexpr ((FROM ^ TO) == 1) {
    if constexpr (FROM < TO)  // vdst.odd <- src.even
      asm volatile(WV_NOP_PERM "v_permlane16_swap_b32 %0, %2\n\tv_permlane16_swap_b32 %1, %3"
                   : "=&v"(ol), "=&v"(oh), "+&v"(lo), "+&v"(hi));
    else  // src.even <- vdst.odd
      asm volatile(WV_NOP_PERM "v_permlane16_swap_b32 %2, %0\n\tv_permlane16_swap_b32 %3, %1"
                   : "=&v"(ol), "=&v"(oh), "+&v"(lo), "+&v"(hi));
  } else {
    if constexpr (FROM < TO)  // vdst rows 2-3 <- src rows 0-1
      asm volatile(WV_NOP_PERM "v_permlane32_swap_b32 %0, %2\n\tv_permlane32_swap_b32 %1, %3"
                   : "=&v"(ol), "=&v"(oh), "+&v"(lo), "+&v"(hi));
    else  // src rows 0-1 <- vdst rows 2-3
      asm volatile(WV_NOP_PERM "v_permlane32_swap_b32 %2, %0\n\tv_permlane32_swap_b32 %3, %1"
                   : "=&v"(ol), "=&v"(oh), "+&v"(lo), "+&v"(hi));
  }
  return __hiloint2double((int)oh, (int)ol);
}
// sum of a lane's value over the four quads of its DPP row (component a of every leg)
__device__ __forceinline__ double legsum(double v) {
  v = v + dpp<0x128>(v);  // row_ror:8
  return v + dpp<0x124>(v);  // row_ror:4
}

template <int V>
struct IC {
  static constexpr int value = V;
};
template <int B, int E, class Fn>
__device__ __forceinline__ void sfor(Fn&& f) {
  if constexpr (B < E) {
    f(IC<B>{});
    sfor<B + 1, E>(f);
  }
}

// The 12x12 discrete A = I + A_c dt (calculate_A_mat_c + state_space_discretization,
// ConvexMpc.cpp:110-156) restricted to states 0..11: off-diagonals (0,6)=cy dt, (0,7)=sy dt,
// (1,6)=-sy dt, (1,7)=cy dt, (2,8)=dt, (3..5, 9..11)=dt.
struct Adisc {
  double ad0, ad1, dt;
  __device__ __forceinline__ double atv(int i, const double* v) const {  // (A'v)_i
    double s = v[i];
    if (i == 6) s = (s + ad0 * v[0]) + (-ad1) * v[1];
    else if (i == 7) s = (s + ad1 * v[0]) + ad0 * v[1];
    else if (i == 8) s = s + dt * v[2];
    else if (i >= 9) s = s + dt * v[i - 6];
    return s;
  }
  __device__ __forceinline__ double ma(const double* M, int r, int j) const {  // (M A)_{rj}
    const double* mr = M + 12 * r;
    double s = mr[j];
    if (j == 6) s = (s + mr[0] * ad0) + mr[1] * (-ad1);
    else if (j == 7) s = (s + mr[0] * ad1) + mr[1] * ad0;
    else if (j == 8) s = s + mr[2] * dt;
    else if (j >= 9) s = s + mr[j - 6] * dt;
    return s;
  }
  __device__ __forceinline__ double atm(const double* M, int i, int j) const {  // (A'M)_{ij}
    double s = M[12 * i + j];
    if (i == 6) s = (s + ad0 * M[j]) + (-ad1) * M[12 + j];
    else if (i == 7) s = (s + ad1 * M[j]) + ad0 * M[12 + j];
    else if (i == 8) s = s + dt * M[24 + j];
    else if (i >= 9) s = s + dt * M[12 * (i - 6) + j];
    return s;
  }
  __device__ __forceinline__ double at(int u, int j) const {  // A[u][j]
    if (u == j) return 1.0;
    if (j == 6) return u == 0 ? ad0 : (u == 1 ? -ad1 : 0.0);
    if (j == 7) return u == 0 ? ad1 : (u == 1 ? ad0 : 0.0);
    if (j == 8) return u == 2 ? dt : 0.0;
    if (j >= 9) return u == j - 6 ? dt : 0.0;
    return 0.0;
  }
};

// I_w^-1, I_w = R I_b R' (calculate_B_mat_c, ConvexMpc.cpp:132-138; Eigen's cofactor inverse)
__device__ __forceinline__ void iw_inverse(const double* rec, double (&Iwinv)[9]) {
  const double* R = rec + MPCQP_REC_ROT;
  const double* Ib = rec + MPCQP_REC_INERTIA;
  double tmp[9], Iw[9];
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      double s = 0.0;
#pragma unroll
      for (int k = 0; k < 3; ++k) s += R[i * 3 + k] * Ib[k * 3 + j];
      tmp[i * 3 + j] = s;
    }
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      double s = 0.0;
#pragma unroll
      for (int k = 0; k < 3; ++k) s += tmp[i * 3 + k] * R[j * 3 + k];
      Iw[i * 3 + j] = s;
    }
  auto cof = [&](int i, int j) {
    const int i1 = (i + 1) % 3, i2 = (i + 2) % 3, j1 = (j + 1) % 3, j2 = (j + 2) % 3;
    return Iw[i1 * 3 + j1] * Iw[i2 * 3 + j2] - Iw[i1 * 3 + j2] * Iw[i2 * 3 + j1];
  };
  const double det = (cof(0, 0) * Iw[0] + cof(1, 0) * Iw[3]) + cof(2, 0) * Iw[6];
  const double invdet = 1.0 / det;
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) Iwinv[j * 3 + i] = cof(i, j) * invdet;
}

// A~'v for the three variables of a leg, from the quad's rows (lane a: row a, v4: row 4).
// Lane a < 3 returns component a.  AK0: row a's coefficient on fx (a < 2) / fy (a >= 2);
// AK1: row a's coefficient on fz; AK4: row 4's coefficient on fz.
__device__ __forceinline__ double quad_at(double v, double v4, double AK0, double AK1, double AK4, int a) {
  const double p0 = AK0 * v, p1 = AK1 * v;
  const double s01 = dpp<QP_02>(p0) + dpp<QP_13>(p0);
  const double tt = p1 + dpp<QP_X1>(p1);
  const double s2 = (tt + dpp<QP_X2>(tt)) + AK4 * v4;
  return a < 2 ? s01 : s2;
}

// index of (r, c) in a symmetric 3x3 stored as its upper triangle 00 01 02 11 12 22
__device__ __forceinline__ int sym6(int r, int c) {
  const int lo = r < c ? r : c, hi = r < c ? c : r;
  return lo == 0 ? hi : (lo == 1 ? 2 + hi : 5);
}

// ---- 16x16 tiles on the matrix cores (factorize_mfma, the Schur form's Gauss-Jordan) ---------------
// Every 12x12 product of the Riccati step runs as 16x16 (zero-padded) v_mfma_f64_16x16x4f64 (IEEE
// binary64 FMAs).  Matrices live in the MFMA result ("D") layout: lane j + 16 g, register v holds
// row 4v + g, column j.  In that layout register kb of a matrix X is exactly the B operand of K-block
// kb (X[4kb + kk][j] at lane j + 16 kk) and the A operand of K-block kb of X' (X'[i][4kb + kk] at
// lane i + 16 kk), so products chain without any data movement: C = A X takes A' and X in D layout.
typedef double mf4 __attribute__((ext_vector_type(4)));

// C (+)= (Aᵀ given as `at`)ᵀ X over K-blocks KB0..KB1-1
template <int KB0, int KB1>
__device__ __forceinline__ mf4 mfma_chain(const mf4& at, const mf4& x, mf4 c) {
#pragma unroll
  for (int kb = KB0; kb < KB1; ++kb) c = __builtin_amdgcn_mfma_f64_16x16x4f64(at[kb], x[kb], c, 0, 0, 0);
  return c;
}
// lane L of the lane's DPP row
template <int L>
__device__ __forceinline__ double rbcast(double x) {
  // one v_mov_b64_dpp; the compiler sees it and inserts the DPP wait states itself
  return __builtin_amdgcn_update_dpp(0.0, x, 0x150 + L, 0xF, 0xF, false);
}
// 1 / d: hardware reciprocal + two Newton steps (correct to the last bit or one ulp; the pivots of
// an SPD matrix are positive and normal)
__device__ __forceinline__ double recip(double d) {
  double r = __builtin_amdgcn_rcp(d);
  double e = __builtin_fma(-d, r, 1.0);
  r = __builtin_fma(r, e, r);
  e = __builtin_fma(-d, r, 1.0);
  return __builtin_fma(r, e, r);
}

// ---- what scale_kernel (mpcqp_scale.hip) and wave_kernel share: thresholds, the image, H's columns --
// B6_k Gram pivot ratio below which a robot is handed to the Riccati form (scale_kernel's screen)
#ifndef MPCQP_SCHUR_GRAM_TOL
#define MPCQP_SCHUR_GRAM_TOL 1e-6
#endif
constexpr double SCHUR_GRAM_TOL = MPCQP_SCHUR_GRAM_TOL;
// The Schur form's hand-off to the Riccati form (mpcqp_schur.h), decided at every update_info
// iteration from the latest factorization's max_i S_ii (a lower bound on the condition of S) and that
// iteration's observed cancellation of the push-through identity, schur_solve's
// amp = max|R'^-1 w| / max|u|: one KKT solve then loses about eps * S_max * amp of relative accuracy.
// A robot leaves when S_max * amp > SCHUR_AMP or S_max > SCHUR_SMAX (a hard cap).
// History: round 4 handed over on S_max > 1e4 (four feet in contact, state weights x 5 / x 100: u0 off
// the oracle by 4e-4 / 1e-3 without a hand-off, 9e-7 with it); round 5 lowered that to 3e3 after a
// loop change moved FMA contraction and the mixed-gait golden set from 1.0e-9 to 1.3e-7.  Round 6
// (profiles/r06/cancel: 7,254 robots — stance / mixed at weights x 1, 5, 100, the golden sets, C2 and
// C5 samples — solved to the end by the Schur form in builds with -ffp-contract=fast and =on): the
// worst u0 error of the robots a bound keeps, S_max <= 3e3: 8.3e-9 (fast) / 6.8e-9 (on), 52 handed
// over; S_max * amp <= 5e4: 2.4e-9 / 2.0e-9, 69 handed over (C2: 0 of 2048, C5: 14 of 2048);
// <= 3e4: 1.1e-9 / 8.1e-10 but C5 hands over 101 of 8192 robots and takes 3.15 ms instead of 2.91
// (profiles/r06/cancel/ab.txt: a few late hand-offs re-solved from the start end the batch).
#ifndef MPCQP_SCHUR_SMAX
#define MPCQP_SCHUR_SMAX 1e4
#endif
constexpr double SCHUR_SMAX = MPCQP_SCHUR_SMAX;
#ifndef MPCQP_SCHUR_AMP
#define MPCQP_SCHUR_AMP 5e4
#endif
constexpr double SCHUR_AMP = MPCQP_SCHUR_AMP;
template <int N>
struct ScaleImg {
  static constexpr int n = ND * N, m = CD * N;
  static constexpr int D = 0, E = D + n, Q = E + m, QN = Q + n, CS = QN + n, MODE = CS + 1, DEGEN = MODE + 1,
                       SIZE = DEGEN + 1;
  static_assert(SIZE == scale_image_doubles(N), "scale image layout");
};

// Column c of H = B'Q̄B + R in closed form (A_c is nilpotent on the 12 moving states, A_c^2 = 0,
// so A^m = I + m Ac with Ac := dt A_c, and
//   S_j = sum_{m=0}^{M_j} (A^m)' Q A^m = (M_j+1) Q + T1_j (Q Ac + Ac'Q) + T2_j Ac'Q Ac,
//   M_j = N-1-j, T1 = M(M+1)/2, T2 = M(M+1)(2M+1)/6.  With y = B_k e_a (column c = 12k + a):
//   block j <= k:  H_jk e_a = B_j' (A')^{k-j} S_k y = B_j' (g + (k-j) Ac'g),   g = S_k y
//   block j >  k:  H_jk e_a = B_j' S_j A^{j-k} y   = B_j' S_j (y + (j-k) Ac y)
// where only rows 6-11 of the 12-vector inside B_j' matter).  Blocks jb .. jb+NB-1 (< N) only;
// sink(jj, b, ri, hv) receives entry ri = 12 j + b of block j = jb + jj, jj and b compile-time.
// SM: any LDS image with the B_w rows (Bw[N][3][ND]).
template <int N, int NB, bool UNROLL, class SM, class Sink>
__device__ __forceinline__ void gen_col(const SM& sm, const mpcqp_params& p, const Adisc& A, double dtm,
                                        int c, int jb, Sink&& sink) {
  const double dt = A.dt;
  const int k = c / ND, a2 = c % ND;
  double y[12], w[12];
#pragma unroll
  for (int s2 = 0; s2 < 12; ++s2) y[s2] = 0.0;
  y[6] = sm.Bw[k][0][a2];
  y[7] = sm.Bw[k][1][a2];
  y[8] = sm.Bw[k][2][a2];
  y[9 + a2 % 3] = dtm;
  w[0] = A.ad0 * y[6] + A.ad1 * y[7];
  w[1] = (-A.ad1) * y[6] + A.ad0 * y[7];
  w[2] = dt * y[8];
  w[3] = dt * y[9];
  w[4] = dt * y[10];
  w[5] = dt * y[11];
#pragma unroll
  for (int s2 = 6; s2 < 12; ++s2) w[s2] = 0.0;
  double qy[12], qw[12];
#pragma unroll
  for (int s2 = 0; s2 < 12; ++s2) {
    qy[s2] = 2 * p.q_weights[s2] * y[s2];
    qw[s2] = 2 * p.q_weights[s2] * w[s2];
  }
  auto actv = [&](const double (&v)[12], double (&o)[6]) __attribute__((always_inline)) {
    o[0] = A.ad0 * v[0] + (-A.ad1) * v[1];
    o[1] = A.ad1 * v[0] + A.ad0 * v[1];
    o[2] = dt * v[2];
    o[3] = dt * v[3];
    o[4] = dt * v[4];
    o[5] = dt * v[5];
  };
  double u1[6], u2[6];
  actv(qy, u1);
  actv(qw, u2);
  const double Mk = (double)(N - 1 - k);
  const double T1k = Mk * (Mk + 1) / 2, T2k = Mk * (Mk + 1) * (2 * Mk + 1) / 6;
  double g[12];
#pragma unroll
  for (int s2 = 0; s2 < 12; ++s2) {
    const double ac = s2 >= 6 ? u1[s2 - 6] : 0.0, ac2 = s2 >= 6 ? u2[s2 - 6] : 0.0;
    g[s2] = ((Mk + 1) * qy[s2] + T1k * (qw[s2] + ac)) + T2k * ac2;
  }
  double h[6];
  actv(g, h);
  auto block = [&](int jj) __attribute__((always_inline)) {
    const int j = jb + jj;
    if (j >= N) return;
    const bool up = j <= k;
    const double d = (double)(j - k);
    const double Mj = (double)(N - 1 - j);
    const double T1j = Mj * (Mj + 1) / 2, T2j = Mj * (Mj + 1) * (2 * Mj + 1) / 6;
    const double cg = up ? 1.0 : 0.0, ch = up ? -d : 0.0;
    const double cqy = up ? 0.0 : Mj + 1, cqw = up ? 0.0 : (Mj + 1) * d + T1j;
    const double cu1 = up ? 0.0 : T1j, cu2 = up ? 0.0 : T1j * d + T2j;
    double v[6];
#pragma unroll
    for (int s2 = 0; s2 < 6; ++s2)
      v[s2] = ((((cg * g[6 + s2] + ch * h[s2]) + cqy * qy[6 + s2]) + cqw * qw[6 + s2]) + cu1 * u1[s2]) + cu2 * u2[s2];
    const double* bw0 = sm.Bw[j][0];
    const double* bw1 = sm.Bw[j][1];
    const double* bw2 = sm.Bw[j][2];
#pragma unroll
    for (int b = 0; b < 12; ++b) {
      double hv = ((bw0[b] * v[0] + bw1[b] * v[1]) + bw2[b] * v[2]) + dtm * v[3 + b % 3];
      if (j == k && b == a2) hv += 2 * p.r_weights[b];
      sink(jj, b, ND * j + b, hv);
    }
  };
  if constexpr (UNROLL) {
    sfor<0, NB>([&](auto JJ) __attribute__((always_inline)) { block(decltype(JJ)::value); });
  } else {
#pragma unroll 1
    for (int jj = 0; jj < NB; ++jj) block(jj);
  }
}

}  // namespace wv
}  // namespace mpcqp
