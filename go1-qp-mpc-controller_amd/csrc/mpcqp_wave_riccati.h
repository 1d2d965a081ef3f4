// mpcqp_wave_riccati.h — the Riccati form of the wave kernel's KKT solve (KS = 0, every horizon),
// the counterpart of mpcqp_schur.h: the LDS image of the factors, the DPP mat-vec and chain helpers,
// the LDS column loads, the factorization on the matrix cores (factorize_mfma) and the per-iteration
// solve without stored Acl (riccati_solve_noacl, N > ACL_MAXN).  The recursion itself is derived at the
// top of mpcqp_wave.hip, which keeps the stored-Acl solve (N <= ACL_MAXN) and the warm iterate's P~x
// sweep written out in wave_solve: as functions here they moved its code generation and cost time
// (profiles/wave_phases).  (mpcqp_riccati.hip is another thing: the debug library's workgroup
// kernel.)  Not installed.
#pragma once
#include "mpcqp_wave_common.h"

namespace mpcqp {
namespace wv {

// Stored 12x12 factors (G_k^-1, K_k, Acl_k): row r starts at double mo(r) = 12 r + 2 [r >= 4] (a
// 16-B gap after row 3) and matrices are MS = 146 doubles apart.  The DPP rows of a wave read 12
// distinct rows of one matrix (chains) or rows {0-2, 9-11} of one matrix with rows {3-8} of the
// next (parallel phases); with this layout both land on 12 distinct 16-B bank slots of every
// ds_read_b128 lane group (row-major 12 x 12 at stride 144 put rows r and r + 8 on one slot:
// 2-way conflicts, 449 extra LDS cycles per iteration measured with SQ_LDS_BANK_CONFLICT).
constexpr int MS = 146;
__host__ __device__ constexpr int mo(int r) { return 12 * r + (r >= 4 ? 2 : 0); }

// Riccati factors (KS = 0; the factorization itself runs in registers).  With SACL the closed-loop
// matrices Acl_k = A - B_k K_k are stored for the chains; without (long horizons: the three factor
// families would leave room for only two robots per CU) the chains apply A and B_k K_k separately,
// and the R'_k foot blocks share G_k^-1's slot (read by factorization step k before it writes G_k^-1).
constexpr int ACL_MAXN = 12;
template <int N, bool SACL>
struct RicFactors;
template <int N>
struct RicFactors<N, true> {
  static constexpr bool HAS_ACL = true;
  static constexpr int NK = N > 1 ? N - 1 : 1;  // K_k stored for k = 1..N-1
  static constexpr int NA = N > 2 ? N - 2 : 1;  // Acl_k stored for k = 1..N-2
  alignas(16) double Gi[N][MS];
  alignas(16) double K[NK][MS];
  alignas(16) double Acl[NA][MS];
  double Rt[N][4][6];  // R'_k foot blocks, upper triangle (00 01 02 11 12 22)
  __device__ double* rt(int k) { return &Rt[k][0][0]; }
};
// Without Acl, G_k^-1 (symmetric) is kept as its upper triangle, rows packed (row r at poff(r)),
// GPS doubles per step and 4R steps (whole register rounds, so that every lane's row can be read
// at a compile-time offset from a per-lane base): the three families then need 40.7 KB at N = 20,
// four robots per CU.
__host__ __device__ constexpr int poff(int r) { return 12 * r - r * (r - 1) / 2; }
constexpr int GPS = 80;
static_assert(poff(11) + 1 <= GPS, "packed 12 x 12 upper triangle");
template <int N>
struct RicFactors<N, false> {
  static constexpr bool HAS_ACL = false;
  static constexpr int NK = N > 1 ? N - 1 : 1;
  alignas(16) double Gp[4 * ((N + 3) / 4)][GPS];
  alignas(16) double K[NK][MS];
  __device__ double* rt(int k) { return &Gp[k][0]; }
};

// ---- DPP mat-vecs (the wait states of the blocks: mpcqp_wave_common.h) ---------------------------
#define WV_FM(A, M, L) "v_fmac_f64_dpp " A ", %[x], " M " row_newbcast:" #L " row_mask:0xf bank_mask:0xf\n\t"
// y_i = sum_c M[i][c] x_c, x_c broadcast from lane 4(c/3)+c%3 of each DPP row, M row i in `c`.
// One accumulator per mat-vec, the terms in column order: a dependent v_fmac_f64_dpp chain issues as
// fast as independent ones for a lone wave (4.4 against 5.35 cycles, tools/mb/mb_valu), so rotating
// accumulators only cost the zeroing moves and the closing adds (the round-4 form).
// Each FMA reads the accumulator its predecessor just wrote.  The DPP wait-state requirement (VALU
// write, then a DPP read of that VGPR: 2 states) concerns the operand read through the lane permute,
// src0 (here x, written before the block's head wait); the accumulator is an ordinary dependent VALU
// operand.  LLVM's hazard recognizer applies the rule to every operand of a DPP instruction, so this
// reading is not the compiler's: tools/mb/mb_valu checks the chain numerically on MI355X (bitwise the
// host's fma chain) beside the src0 case it does not cover.
#define WV_OPS12(P, C) [P##0] "v"(C[0]), [P##1] "v"(C[1]), [P##2] "v"(C[2]), [P##3] "v"(C[3]), [P##4] "v"(C[4]), \
    [P##5] "v"(C[5]), [P##6] "v"(C[6]), [P##7] "v"(C[7]), [P##8] "v"(C[8]), [P##9] "v"(C[9]),                \
    [P##10] "v"(C[10]), [P##11] "v"(C[11])
#define WV_OPS6(P, C) [P##0] "v"(C[0]), [P##1] "v"(C[1]), [P##2] "v"(C[2]), [P##3] "v"(C[3]), [P##4] "v"(C[4]), \
    [P##5] "v"(C[5])
#define WV_M12(A) WV_FM(A, "%[c0]", 0) WV_FM(A, "%[c1]", 1) WV_FM(A, "%[c2]", 2) WV_FM(A, "%[c3]", 4)  \
    WV_FM(A, "%[c4]", 5) WV_FM(A, "%[c5]", 6) WV_FM(A, "%[c6]", 8) WV_FM(A, "%[c7]", 9)                 \
    WV_FM(A, "%[c8]", 10) WV_FM(A, "%[c9]", 12) WV_FM(A, "%[c10]", 13) WV_FM(A, "%[c11]", 14)
#define WV_M6HI(A) WV_FM(A, "%[c0]", 8) WV_FM(A, "%[c1]", 9) WV_FM(A, "%[c2]", 10) WV_FM(A, "%[c3]", 12) \
    WV_FM(A, "%[c4]", 13) WV_FM(A, "%[c5]", 14)
#define WV_M6LO(A) WV_FM(A, "%[c0]", 0) WV_FM(A, "%[c1]", 1) WV_FM(A, "%[c2]", 2) WV_FM(A, "%[c3]", 4)  \
    WV_FM(A, "%[c4]", 5) WV_FM(A, "%[c5]", 6)
__device__ __forceinline__ double mv12(double x, const double (&c)[12]) {
  double a = 0.0;
  asm(WV_NOP_HEAD WV_M12("%[a]") : [a] "+&v"(a) : [x] "v"(x), WV_OPS12(c, c));
  return a;
}
// sum over states 6..11 (lanes 8, 9, 10, 12, 13, 14) of c[s-6] x_s
__device__ __forceinline__ double mv6(double x, const double (&c)[6]) {
  double a = 0.0;
  asm(WV_NOP_HEAD WV_M6HI("%[a]") : [a] "+&v"(a) : [x] "v"(x), WV_OPS6(c, c));
  return a;
}
// Two / three independent mat-vecs interleaved in one block (each has its own x and rows)
#define WV_FX(A, X, M, L) "v_fmac_f64_dpp " A ", " X ", " M " row_newbcast:" #L " row_mask:0xf bank_mask:0xf\n\t"
#define WV_T2(L, I) WV_FX("%[a]", "%[x0]", "%[p" #I "]", L) WV_FX("%[b]", "%[x1]", "%[q" #I "]", L)
#define WV_T3(L, I) WV_T2(L, I) WV_FX("%[d]", "%[x2]", "%[r" #I "]", L)
__device__ __forceinline__ void mv12x2(double x0, double x1, const double (&c0)[12], const double (&c1)[12],
                                       double& y0, double& y1) {
  double a = 0.0, b = 0.0;
  asm(WV_NOP_HEAD
      WV_T2(0, 0) WV_T2(1, 1) WV_T2(2, 2) WV_T2(4, 3) WV_T2(5, 4) WV_T2(6, 5)
      WV_T2(8, 6) WV_T2(9, 7) WV_T2(10, 8) WV_T2(12, 9) WV_T2(13, 10) WV_T2(14, 11)
      : [a] "+&v"(a), [b] "+&v"(b)
      : [x0] "v"(x0), [x1] "v"(x1), WV_OPS12(p, c0), WV_OPS12(q, c1));
  y0 = a;
  y1 = b;
}
__device__ __forceinline__ void mv12x3(double x0, double x1, double x2, const double (&c0)[12],
                                       const double (&c1)[12], const double (&c2)[12], double& y0, double& y1,
                                       double& y2) {
  double a = 0.0, b = 0.0, d = 0.0;
  asm(WV_NOP_HEAD
      WV_T3(0, 0) WV_T3(1, 1) WV_T3(2, 2) WV_T3(4, 3) WV_T3(5, 4) WV_T3(6, 5)
      WV_T3(8, 6) WV_T3(9, 7) WV_T3(10, 8) WV_T3(12, 9) WV_T3(13, 10) WV_T3(14, 11)
      : [a] "+&v"(a), [b] "+&v"(b), [d] "+&v"(d)
      : [x0] "v"(x0), [x1] "v"(x1), [x2] "v"(x2), WV_OPS12(p, c0), WV_OPS12(q, c1), WV_OPS12(r, c2));
  y0 = a;
  y1 = b;
  y2 = d;
}
#undef WV_T2
#undef WV_T3
#undef WV_FX
// y[r] = M_r x[r] for the R register rounds of a parallel phase, interleaved.
template <int R>
__device__ __forceinline__ void mv_rounds(const double (&x)[R], const double (&c)[R][12], double (&y)[R]) {
  if constexpr (R == 1) {
    y[0] = mv12(x[0], c[0]);
  } else if constexpr (R == 2) {
    mv12x2(x[0], x[1], c[0], c[1], y[0], y[1]);
  } else if constexpr (R == 3) {
    mv12x3(x[0], x[1], x[2], c[0], c[1], c[2], y[0], y[1], y[2]);
  } else {
#pragma unroll
    for (int r = 0; r < R; ++r) y[r] = mv12(x[r], c[r]);
  }
}
// init + sum_c M[c] x_c: the chains' "- a_k" / "+ h_k" as the accumulator's start
__device__ __forceinline__ double mv12a(double x, const double (&c)[12], double init) {
  double a = init;
  asm(WV_NOP_HEAD WV_M12("%[a]") : [a] "+&v"(a) : [x] "v"(x), WV_OPS12(c, c));
  return a;
}
// init + sum over states 6..11 (lanes 8, 9, 10, 12, 13, 14) of c[s-6] x_s
__device__ __forceinline__ double mv6a(double x, const double (&c)[6], double init) {
  double a = init;
  asm(WV_NOP_HEAD WV_M6HI("%[a]") : [a] "+&v"(a) : [x] "v"(x), WV_OPS6(c, c));
  return a;
}
// init + sum over states 0..5 (lanes 0, 1, 2, 4, 5, 6) of c[s] x_s
__device__ __forceinline__ double mv6lo_a(double x, const double (&c)[6], double init) {
  double a = init;
  asm(WV_NOP_HEAD WV_M6LO("%[a]") : [a] "+&v"(a) : [x] "v"(x), WV_OPS6(c, c));
  return a;
}
// One middle step of each chain of the Acl-free Riccati form (N > 12) in one block, so that the
// step's wait states come from its own independent FMAs instead of s_nop (8.4 cycles for 2 states):
// only m, the row-moved chain value, is a fresh VALU result at the block's start.  Every accumulator
// takes the same FMAs in the same order as the separate helpers (bitwise the same results).
//   backward: tk = w + sum_hi bcast(m) bc (mv6a);  s = m + sum_lo bcast(m) cat (mv6lo_a), then
//             s += sum bcast(tk) kc (mv12a(tk, kc, s)): s is the chain's next value
//   forward:  nu = -g + sum bcast(m) kc (mv12a);  ax = m + sum_hi bcast(m) cax (mv6a);
//             hb = sum bcast(nu) bc (mv12)
#define WV_FY(A, X, M, L) "v_fmac_f64_dpp %[" A "], %[" X "], %[" M "] row_newbcast:" #L " row_mask:0xf bank_mask:0xf\n\t"
__device__ __forceinline__ void chain_bwd(double m, const double (&bc)[6], const double (&cat)[6],
                                          const double (&kc)[12], double& tk, double& s) {
  asm(WV_NOP_HEAD
      WV_FY("t", "m", "b0", 8) WV_FY("s", "m", "a0", 0) WV_FY("t", "m", "b1", 9) WV_FY("s", "m", "a1", 1)
      WV_FY("t", "m", "b2", 10) WV_FY("s", "m", "a2", 2) WV_FY("t", "m", "b3", 12) WV_FY("s", "m", "a3", 4)
      WV_FY("t", "m", "b4", 13) WV_FY("t", "m", "b5", 14) WV_FY("s", "m", "a4", 5) WV_FY("s", "m", "a5", 6)
      // (tk's last write is two instructions back)
      WV_FY("s", "t", "k0", 0) WV_FY("s", "t", "k1", 1) WV_FY("s", "t", "k2", 2) WV_FY("s", "t", "k3", 4)
      WV_FY("s", "t", "k4", 5) WV_FY("s", "t", "k5", 6) WV_FY("s", "t", "k6", 8) WV_FY("s", "t", "k7", 9)
      WV_FY("s", "t", "k8", 10) WV_FY("s", "t", "k9", 12) WV_FY("s", "t", "k10", 13) WV_FY("s", "t", "k11", 14)
      : [t] "+&v"(tk), [s] "+&v"(s)
      : [m] "v"(m), WV_OPS6(b, bc), WV_OPS6(a, cat), WV_OPS12(k, kc));
}
__device__ __forceinline__ void chain_fwd(double m, const double (&kc)[12], const double (&cax)[6],
                                          const double (&bc)[12], double& nu, double& ax, double& hb) {
  asm(WV_NOP_HEAD
      WV_FY("n", "m", "k0", 0) WV_FY("x", "m", "c0", 8) WV_FY("n", "m", "k1", 1) WV_FY("x", "m", "c1", 9)
      WV_FY("n", "m", "k2", 2) WV_FY("x", "m", "c2", 10) WV_FY("n", "m", "k3", 4) WV_FY("x", "m", "c3", 12)
      WV_FY("n", "m", "k4", 5) WV_FY("n", "m", "k5", 6) WV_FY("n", "m", "k6", 8) WV_FY("n", "m", "k7", 9)
      WV_FY("n", "m", "k8", 10) WV_FY("n", "m", "k9", 12) WV_FY("n", "m", "k10", 13) WV_FY("n", "m", "k11", 14)
      WV_FY("x", "m", "c4", 13) WV_FY("x", "m", "c5", 14)
      // (nu's last write is two instructions back)
      WV_FY("h", "n", "d0", 0) WV_FY("h", "n", "d1", 1) WV_FY("h", "n", "d2", 2) WV_FY("h", "n", "d3", 4)
      WV_FY("h", "n", "d4", 5) WV_FY("h", "n", "d5", 6) WV_FY("h", "n", "d6", 8) WV_FY("h", "n", "d7", 9)
      WV_FY("h", "n", "d8", 10) WV_FY("h", "n", "d9", 12) WV_FY("h", "n", "d10", 13) WV_FY("h", "n", "d11", 14)
      : [n] "+&v"(nu), [x] "+&v"(ax), [h] "+&v"(hb)
      : [m] "v"(m), WV_OPS12(k, kc), WV_OPS6(c, cax), WV_OPS12(d, bc));
}
#undef WV_FY
#undef WV_OPS12
#undef WV_OPS6
#undef WV_M12
#undef WV_M6HI
#undef WV_M6LO
#undef WV_FM

// ---- LDS loads of the factors' rows and columns ---------------------------------------------------
__device__ __forceinline__ void ld12(double (&c)[12], const double* p) {  // 12 contiguous, 16-B aligned
  const double2* p2 = reinterpret_cast<const double2*>(p);
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    const double2 v = p2[i];
    c[2 * i] = v.x;
    c[2 * i + 1] = v.y;
  }
}
// A column of a stored factor (c[i] = p[mo(i)]) as 12 separate ds_read_b64, issued without waiting:
// the compiler pairs plain loads of it into ds_read2_b64, which moves 16 B per lane in 8 LDS-array
// cycles against 2 x 2 for two ds_read_b64.  The compiler does not track these loads: the values are
// valid only after
// lds_wait<n>(c), n = the number of LDS instructions issued after them that may stay in flight
// (LDS returns in order; lgkmcnt holds at most 15).
__device__ __forceinline__ unsigned lds_off(const double* p) {
  return (unsigned)(uintptr_t)(const __attribute__((address_space(3))) double*)p;
}
__device__ __forceinline__ void ldcol(double (&c)[12], const double* p) {
  static_assert(mo(11) * 8 == 1072 && mo(4) * 8 == 400, "column offsets below");
  const unsigned ad = lds_off(p);
  asm volatile(
      "ds_read_b64 %0, %12\n\t"
      "ds_read_b64 %1, %12 offset:96\n\t"
      "ds_read_b64 %2, %12 offset:192\n\t"
      "ds_read_b64 %3, %12 offset:288\n\t"
      "ds_read_b64 %4, %12 offset:400\n\t"
      "ds_read_b64 %5, %12 offset:496\n\t"
      "ds_read_b64 %6, %12 offset:592\n\t"
      "ds_read_b64 %7, %12 offset:688\n\t"
      "ds_read_b64 %8, %12 offset:784\n\t"
      "ds_read_b64 %9, %12 offset:880\n\t"
      "ds_read_b64 %10, %12 offset:976\n\t"
      "ds_read_b64 %11, %12 offset:1072"
      : "=&v"(c[0]), "=&v"(c[1]), "=&v"(c[2]), "=&v"(c[3]), "=&v"(c[4]), "=&v"(c[5]), "=&v"(c[6]),
        "=&v"(c[7]), "=&v"(c[8]), "=&v"(c[9]), "=&v"(c[10]), "=&v"(c[11])
      : "v"(ad));
}
template <int CNT>
__device__ __forceinline__ void lds_wait(double (&c)[12]) {
  static_assert(CNT >= 0 && CNT <= 15, "lgkmcnt range");
  asm volatile("s_waitcnt lgkmcnt(%12)"
               : "+&v"(c[0]), "+&v"(c[1]), "+&v"(c[2]), "+&v"(c[3]), "+&v"(c[4]), "+&v"(c[5]), "+&v"(c[6]),
                 "+&v"(c[7]), "+&v"(c[8]), "+&v"(c[9]), "+&v"(c[10]), "+&v"(c[11])
               : "n"(CNT));
}

// ---- factorization on the matrix cores (the tile layout: mpcqp_wave_common.h) --------------------
// value of lane group GP (same lane within the group) in every group
template <int GP>
__device__ __forceinline__ double bcast_group(double x) {
  const int g = threadIdx.x >> 4;
  const double y = xor16(x);  // group g ^ 1
  const double z = ((g & 1) == (GP & 1)) ? x : y;
  const double w = xor32(z);  // group g ^ 2
  return ((g & 2) == (GP & 2)) ? z : w;
}
// In-place Gauss-Jordan inverse of the symmetric positive definite leading 12x12 block (scalar
// pivots, no pivoting: stable for SPD).  Pad rows / columns 12-15 must hold the identity.
__device__ __forceinline__ void gj_inverse12(mf4& g) {
  const int j = threadIdx.x & 15, grp = threadIdx.x >> 4;
  sfor<0, 12>([&](auto P) __attribute__((always_inline)) {
    constexpr int p = decltype(P)::value, vp = p / 4, gp = p % 4;
    const double rowp = bcast_group<gp>(g[vp]);  // G[p][j]
    const double piv = rbcast<p>(rowp);     // G[p][p]
    const double pinv = recip(piv);
    const double rs = rowp * pinv;
    const bool jp = j == p;
    // register 3 holds the pad rows 12-15: identity, zero in every pivot column, never changes
#pragma unroll
    for (int v = 0; v < 3; ++v) {
      const double col = rbcast<p>(g[v]);  // G[4v + grp][p]
      const double upd = jp ? -col * pinv : g[v] - col * rs;
      if (v == vp) g[v] = (grp == gp) ? (jp ? pinv : rs) : upd;  // row p
      else g[v] = upd;
    }
  });
}

// The Riccati recursion of c B'Q̄B + R' (R'_k foot blocks in F.Rt) -> G_k^-1, K_k, Acl_k in LDS.
template <int N, class SM>
// q2j: 2 q_j of the lane's column j = lane & 15 (j < 12), loaded once by the caller (a per-lane index
// into the parameters is a memory round trip)
__device__ void factorize_mfma(SM& sm, const mpcqp_params& p, const Adisc& A, double c, double dtm, double q2j) {
  auto& F = sm.u.f;
  const int j = threadIdx.x & 15, grp = threadIdx.x >> 4;
  mf4 Ad, At, cQ, P;
#pragma unroll
  for (int v = 0; v < 4; ++v) {
    const int u = 4 * v + grp;
    const bool in = u < 12 && j < 12;
    Ad[v] = in ? A.at(u, j) : 0.0;
    At[v] = in ? A.at(j, u) : 0.0;
    cQ[v] = (in && u == j) ? c * q2j : 0.0;
    P[v] = cQ[v];
  }
  for (int k = N - 1; k >= 0; --k) {
    // B_k (rows 6-8: B_w, rows 9-11: dt/m on the matching force component) and B_k', D layout
    mf4 Bk, Bt, G;
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      const int u = 4 * v + grp;
      auto bsc = [&](int s, int cc) __attribute__((always_inline)) {  // B_k[s][cc]
        if (cc >= 12) return 0.0;
        if (s >= 6 && s < 9) return sm.Bw[k][s - 6][cc];
        if (s >= 9 && s < 12) return (cc % 3 == s - 9) ? dtm : 0.0;
        return 0.0;
      };
      Bk[v] = bsc(u, j);
      Bt[v] = bsc(j, u);
      // R'_k: 3x3 foot blocks (upper triangle stored); identity on the pad
      double rv = 0.0;
      if (u < 12 && j < 12 && u / 3 == j / 3) rv = F.rt(k)[6 * (u / 3) + sym6(u % 3, j % 3)];
      if (u >= 12 && u == j) rv = 1.0;
      G[v] = rv;
    }
    const mf4 zero = {0.0, 0.0, 0.0, 0.0};
    // G = R' + B'(P B): P B needs only B's rows 6-11 (K-blocks 1, 2); B' P B likewise
    const mf4 PB = mfma_chain<1, 3>(P, Bk, zero);
    G = mfma_chain<1, 3>(Bk, PB, G);
    // the products that do not need G^-1 go to the matrix cores before the (VALU) inverse, so
    // they run under it (step 0 computes them for nothing)
    const mf4 PA = mfma_chain<0, 3>(P, Ad, zero);   // P A
    const mf4 Fm = mfma_chain<1, 3>(Bk, PA, zero);  // F = B' P A
    const mf4 Pq = mfma_chain<0, 3>(Ad, PA, cQ);    // cQ + A'P A
    gj_inverse12(G);
    if constexpr (std::remove_reference_t<decltype(F)>::HAS_ACL) {
      if (j < 12)
#pragma unroll
        for (int v = 0; v < 3; ++v) F.Gi[k][mo(4 * v + grp) + j] = G[v];
    } else {
#pragma unroll
      for (int v = 0; v < 3; ++v) {  // upper triangle (row <= column), rows packed
        const int row = 4 * v + grp;
        if (j < 12 && row <= j) F.Gp[k][poff(row) + j - row] = G[v];
      }
    }
    if (k >= 1) {
      const mf4 K = mfma_chain<0, 3>(G, Fm, zero);          // K = G^-1 F
      if (j < 12)
#pragma unroll
        for (int v = 0; v < 3; ++v) F.K[k - 1][mo(4 * v + grp) + j] = K[v];
      if constexpr (std::remove_reference_t<decltype(F)>::HAS_ACL) {
        if (k <= N - 2) {
          mf4 nBt;
#pragma unroll
          for (int v = 0; v < 4; ++v) nBt[v] = -Bt[v];
          const mf4 Acl = mfma_chain<0, 3>(nBt, K, Ad);       // A - B K
          if (j < 12)
#pragma unroll
            for (int v = 0; v < 3; ++v) F.Acl[k - 1][mo(4 * v + grp) + j] = Acl[v];
        }
      }
      mf4 nF;
#pragma unroll
      for (int v = 0; v < 4; ++v) nF[v] = -Fm[v];
      P = mfma_chain<0, 3>(nF, K, Pq);  // cQ + A'PA - F'K
    }
  }
  wave_sync();
}

// ---- the per-iteration solve: U = (c B'Q̄B + R')^-1 D^-1 RHS --------------------------------------
// The lane's place comes in as the caller computed it: ig = gray(q) (its step in round r is 4r + ig),
// q its DPP row, leg / a its foot and component, idx its index inside a step.  DI: 1 / D of the
// lane's variable.  tm_it: the timed iteration of phase-timing builds, whose marks 41-44 go to `mark`.

// Riccati form without Acl (N > ACL_MAXN; sigma_k = -s_k):
//   backward  t_k = w_k - B_k' sigma_{k+1},  sigma_k = K_k' t_k + A' sigma_{k+1}  (sigma_N = 0)
//   parallel  g_k = G_k^-1 t_k
//   forward   u_k = g_k - K_k x_k,  x_{k+1} = A x_k + B_k u_k                    (x_0 = 0)
// (the same recursion: s_k = Acl_k' s_{k+1} - K_k' w_k, x_{k+1} = Acl_k x_k + B_k g_k)
// CAT / CAX: the lane's coefficients of A' on states 0-5 and of A on states 6-11; GADR: the LDS
// address of element c of the lane's row of the packed G_k^-1 in round 0.
template <int N, int R, class SM, class Mark>
__device__ __forceinline__ void riccati_solve_noacl(SM& sm, RicFactors<N, false>& F, const double (&DI)[R],
                                                    const double (&RHS)[R], const double (&CAT)[6],
                                                    const double (&CAX)[6], const unsigned (&GADR)[12],
                                                    const double& dtm, const int& ig, const int& q, const int& leg,
                                                    const int& a, const int& idx, const bool& tm_it, Mark&& mark,
                                                    double (&U)[R]) {
  const bool av = a < 3;
  double W[R], TT[R], G[R];
  int kc[R], kk[R];
#pragma unroll
  for (int r = 0; r < R; ++r) {
    W[r] = DI[r] * RHS[r];
    TT[r] = 0.0;
    U[r] = 0.0;
    kc[r] = min(4 * r + ig, N - 1);
    kk[r] = max(kc[r] - 1, 0);  // slot of K_k (k >= 1)
  }
  if (tm_it) mark(41);
  {  // backward chain; a round's K_k columns (rows of K_k') serve its four steps, one per row
    double kn[12], kcur[12], bcur[6];
    ldcol(kn, &F.K[kk[(N - 1) >> 2]][idx]);
    double cur = 0.0;
    sfor<0, N>([&](auto J) {
      constexpr int k = N - 1 - decltype(J)::value;
      constexpr int r = k >> 2;
      if constexpr (k == N - 1 || (k & 3) == 3) {  // entering round r (descending)
        lds_wait<0>(kn);
#pragma unroll
        for (int e = 0; e < 12; ++e) kcur[e] = kn[e];
        if constexpr (r >= 1) ldcol(kn, &F.K[kk[r - 1]][idx]);
        bcur[0] = -sm.Bw[kc[r]][0][idx];
        bcur[1] = -sm.Bw[kc[r]][1][idx];
        bcur[2] = -sm.Bw[kc[r]][2][idx];
        bcur[3] = a == 0 ? -dtm : 0.0;
        bcur[4] = a == 1 ? -dtm : 0.0;
        bcur[5] = a == 2 ? -dtm : 0.0;
      }
      __builtin_amdgcn_sched_barrier(0);
      if constexpr (k >= 1 && k < N - 1) {  // a middle step: one block (chain_bwd)
        const double m = rmove2<row_of(k + 1), row_of(k)>(cur);
        double tk = W[r], sn = m;
        chain_bwd(m, bcur, CAT, kcur, tk, sn);
        TT[r] = (q == row_of(k)) ? tk : TT[r];
        cur = sn;
        return;
      }
      double m = 0.0, tk = W[r];
      if constexpr (k < N - 1) {
        m = rmove2<row_of(k + 1), row_of(k)>(cur);
        tk = mv6a(m, bcur, W[r]);
      }
      TT[r] = (q == row_of(k)) ? tk : TT[r];
      if constexpr (k >= 1) {
        const double as = k < N - 1 ? mv6lo_a(m, CAT, m) : 0.0;
        cur = mv12a(tk, kcur, as);
      }
    });
  }
  if (tm_it) mark(42);
  // g_k = G_k^-1 t_k: row idx of the packed upper triangle, element c at (min, max) of (idx, c);
  // per-lane LDS addresses (constant) plus the round's compile-time offset
  {
    using lds_d = __attribute__((address_space(3))) const double;
    double c0[12], c1[12];
    auto ldg = [&](int r, double (&c)[12]) __attribute__((always_inline)) {
#pragma unroll
      for (int e = 0; e < 12; ++e)
        c[e] = *(lds_d*)(uintptr_t)(GADR[e] + (unsigned)(sizeof(double) * GPS * 4 * r));
    };
    ldg(0, c0);
    sfor<0, R>([&](auto RR) {
      constexpr int r = decltype(RR)::value;
      if constexpr (r + 1 < R) ldg(r + 1, (r & 1) ? c0 : c1);
      G[r] = mv12(TT[r], (r & 1) ? c1 : c0);
    });
  }
  if (tm_it) mark(43);
  {  // forward chain; a round's K_k rows and B_w rows serve its four steps
    double kn[12], kcur[12], bn[12], bcu[12];
    ld12(kn, &F.K[kk[0]][mo(idx)]);
    ld12(bn, &sm.Bw[kc[0]][av ? a : 2][0]);
    double cur = 0.0;
    sfor<0, N>([&](auto K) {
      constexpr int k = decltype(K)::value;
      constexpr int r = k >> 2;
      if constexpr ((k & 3) == 0) {  // entering round r (ascending)
#pragma unroll
        for (int e = 0; e < 12; ++e) {
          kcur[e] = kn[e];
          bcu[e] = bn[e];
        }
        if constexpr (r + 1 < R) {
          ld12(kn, &F.K[kk[r + 1]][mo(idx)]);
          ld12(bn, &sm.Bw[kc[r + 1]][av ? a : 2][0]);
        }
      }
      __builtin_amdgcn_sched_barrier(0);
      if constexpr (k >= 1 && k <= N - 2) {  // a middle step: one block (chain_fwd)
        const double m = rmove2<row_of(k - 1), row_of(k)>(cur);
        double nu = -G[r], ax = m, hb = 0.0;
        chain_fwd(m, kcur, CAX, bcu, nu, ax, hb);
        U[r] = (q == row_of(k)) ? -nu : U[r];
        const double ls = dtm * legsum(nu);
        const double bnu = leg == 2 ? hb : (leg == 3 ? ls : 0.0);
        cur = ax - bnu;
        return;
      }
      double m = 0.0, nu = -G[r];  // nu = -u_k = K_k x_k - g_k
      if constexpr (k >= 1) {
        m = rmove2<row_of(k - 1), row_of(k)>(cur);
        nu = mv12a(m, kcur, -G[r]);
      }
      U[r] = (q == row_of(k)) ? -nu : U[r];
      if constexpr (k <= N - 2) {
        // B_k nu: rows 6-8 (leg-2 lanes) B_w nu, rows 9-11 (leg-3 lanes) dt/m times the legs' sum
        const double hb = mv12(nu, bcu);
        const double ls = dtm * legsum(nu);
        const double bnu = leg == 2 ? hb : (leg == 3 ? ls : 0.0);
        const double ax = k >= 1 ? mv6a(m, CAX, m) : 0.0;  // A x_k
        cur = ax - bnu;
      }
    });
  }
  if (tm_it) mark(44);
}

}  // namespace wv
}  // namespace mpcqp
