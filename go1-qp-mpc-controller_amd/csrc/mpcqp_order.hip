// mpcqp_order.hip — the launch order of wave_kernel (mpcqp_wave.hip): order_kernel, one workgroup per
// batch part, launched ahead of the part's scale_kernel and wave_kernel on the same stream.
//
// One wave solves one robot and cannot migrate, and robots take 25 to 350 iterations, so in input
// order the last robots dispatched leave most SIMD slots idle (the dispatch tail).  A
// controller solves the same robots every tick: wave_kernel's epilogue leaves each robot's cost key
// (order_key, mpcqp_internal.h) and this kernel sorts the part's robots by
//   1. contact mask of this call's record differs from the one stored by the previous call, first
//      (a changed contact set is the one indicator of a long warm-started solve that is known at
//      launch time),
//   2. stored key, descending,
//   3. batch index
// — a stable counting sort over 2 (ORDER_KEY_MAX + 1) bins — into order[], and stores this call's
// masks.  Whether the stored state belongs to this call's batch is decided here, on the device (the
// host's view would be frozen into a captured graph): each part's state carries {whole batch, parts,
// first robot, robots}, and a part whose layout differs gets the identity order.
//
// A typed solve (LaunchArgs::type) selects robots here: a robot whose type differs from the wanted one is
// left out of the sort, its key[] and contacts[] entries are not touched, and the places behind the
// selected robots get the index -1, for which wave_kernel solves nothing.  With the hint off such a call
// still needs an order[]: identity_kernel writes the identity with holes and reads or writes no state.
#include "mpcqp_internal.h"

namespace mpcqp {
namespace ord {

constexpr int ONT = 1024, ONW = ONT / 64;
constexpr int NBIN = 2 * (ORDER_KEY_MAX + 1);
static_assert(NBIN <= 128, "order_kernel matches bins over 7 bits");

__global__ __launch_bounds__(ONT) void order_kernel(const double* __restrict__ recs, int rec_doubles, int robots,
                                                    int* __restrict__ order, const int* __restrict__ key,
                                                    int* __restrict__ contacts, int* __restrict__ layout,
                                                    int whole, int parts, int part, int first, int kmax,
                                                    const int* __restrict__ type, int want) {
  __shared__ int start[NBIN];        // pass A: robots per bin; pass B: the bin's next free place
  __shared__ int total;              // selected robots (all of them without a type array)
  __shared__ int wcount[ONW][NBIN];  // pass B: robots per bin of each wave of the current chunk
  const int t = threadIdx.x, w = t >> 6, lane = t & 63;
  const bool valid = layout[0] == whole && layout[1] == parts && layout[2] == first && layout[3] == robots;
  if (t < NBIN) start[t] = 0;
  for (int e = t; e < ONW * NBIN; e += ONT) (&wcount[0][0])[e] = 0;
  __syncthreads();  // (every thread has read the layout)
  if (t == 0) {
    layout[0] = whole;
    layout[1] = parts;
    layout[2] = first;
    layout[3] = robots;
  }
  // layouts of parts this call does not have: stale from now on (part 0's layout is the array's base)
  if (part == 0 && t >= parts && t < kmax) layout[ORDER_LAYOUT_INTS * t] = -1;
  auto mask_of = [&](int r) {
    const double* c = recs + (size_t)r * rec_doubles + MPCQP_REC_CONTACTS;
    int m = 0;
#pragma unroll
    for (int l = 0; l < MPCQP_NUM_LEG; ++l) m |= (c[l] != 0.0) ? (1 << l) : 0;
    return m;
  };
  auto selected = [&](int r) { return !type || type[r] == want; };
  if (!valid) {
    for (int r = t; r < robots; r += ONT) {
      const bool sel = selected(r);
      order[r] = sel ? r : -1;
      if (sel) contacts[r] = mask_of(r);
    }
    return;
  }
  auto bin_of = [&](int r, int m) {
    const int k = key[r];
    const int kc = k < 0 ? 0 : k > ORDER_KEY_MAX ? ORDER_KEY_MAX : k;
    return (m != contacts[r] ? 0 : ORDER_KEY_MAX + 1) + (ORDER_KEY_MAX - kc);
  };
  // pass A: robots per bin, then each bin's first place
  for (int r = t; r < robots; r += ONT)
    if (selected(r)) atomicAdd(&start[bin_of(r, mask_of(r))], 1);
  __syncthreads();
  int before = 0;
  if (t < NBIN)
    for (int b = 0; b < t; ++b) before += start[b];
  if (t == NBIN - 1) total = before + start[t];
  __syncthreads();
  if (t < NBIN) start[t] = before;
  __syncthreads();
  // pass B: chunks of ONT robots in batch order; a robot's place is its bin's next free place, plus
  // the bin's robots in the chunk's earlier waves, plus those in earlier lanes of its own wave
  for (int c0 = 0; c0 < robots; c0 += ONT) {
    const int r = c0 + t;
    const bool act = r < robots && selected(r);
    const int m = act ? mask_of(r) : 0;
    const int bin = act ? bin_of(r, m) : 0;
    unsigned long long peers = __ballot(act);  // the wave's lanes in the same bin
#pragma unroll
    for (int bit = 0; bit < 7; ++bit) {
      const bool set = (bin >> bit) & 1;
      const unsigned long long bl = __ballot(act && set);
      peers &= set ? bl : ~bl;
    }
    const int rank = __popcll(peers & ((1ull << lane) - 1ull));
    if (act && rank == 0) wcount[w][bin] = __popcll(peers);
    __syncthreads();
    if (act) {
      int pos = start[bin] + rank;
      for (int v = 0; v < w; ++v) pos += wcount[v][bin];
      if ((unsigned)pos < (unsigned)robots) order[pos] = r;
      contacts[r] = m;
    }
    __syncthreads();
    if (t < NBIN) {
      int s = 0;
#pragma unroll
      for (int v = 0; v < ONW; ++v) s += wcount[v][t];
      start[t] += s;
    }
    __syncthreads();
    for (int e = t; e < ONW * NBIN; e += ONT) (&wcount[0][0])[e] = 0;
    __syncthreads();
  }
  // the places behind the selected robots: nothing to solve
  for (int pos = total + t; pos < robots; pos += ONT) order[pos] = -1;
}

// A typed solve without the hint: the identity with holes.
__global__ __launch_bounds__(256) void identity_kernel(int robots, int* __restrict__ order,
                                                       const int* __restrict__ type, int want) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r < robots) order[r] = type[r] == want ? r : -1;
}

}  // namespace ord

hipError_t launch_order(const LaunchArgs& a, int kmax) {
  const OrderHint& o = a.hint;
  if (o.identity) {
    if (!o.order || !a.type || a.batch < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(ord::identity_kernel, dim3((a.batch + 255) / 256), dim3(256), 0, (hipStream_t)a.stream,
                       a.batch, o.order, a.type, a.want);
    return hipGetLastError();
  }
  if (!o.order || !o.key || !o.contacts || !o.layout || a.batch < 1 || o.parts < 1 || kmax > ord::ONT)
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(ord::order_kernel, dim3(1), dim3(ord::ONT), 0, (hipStream_t)a.stream, a.recs,
                     MPCQP_REC_SIZE(a.p.horizon), a.batch, o.order, o.key, o.contacts, o.layout, o.whole, o.parts,
                     o.part, o.first, kmax, a.type, a.want);
  return hipGetLastError();
}

}  // namespace mpcqp
