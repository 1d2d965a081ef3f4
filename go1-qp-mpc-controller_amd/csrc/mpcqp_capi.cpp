// mpcqp_capi.cpp — extern "C" boundary (include/mpcqp.h) over the HIP kernels.
//
// Replaces, per batch of robots, the OsqpEigen::Solver lifecycle of the reference
// (A1RobotControl.h:67, A1RobotControl.cpp:522-555) and ConvexMpc's construction
// (ConvexMpc.cpp:7-68).  No exception crosses this boundary.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <new>

#include "../../include/mpcqp.h"
#include "../../include/mpcqp_debug.h"
#include "mpcqp_internal.h"

struct mpcqp_handle {
  mpcqp_params p;
  int device = 0;
  int slots = 0;             // resident workgroups per device (occupancy x CUs), informational
  int cus = 0;               // compute units of the device
  double* work = nullptr;    // per-robot 12N x 16*ceil(12N/16) binary64 workspace (scaled Hessian)
  size_t work_cap = 0;       // instances the workspace can hold
  size_t work_per = 0;       // doubles per instance the workspace was sized for
  int* fb = nullptr;         // wave path: Schur -> Riccati hand-off counters, [4] ints per batch part
  // The wave path splits a batch into parts solved concurrently on internal streams (forked from
  // and joined to the caller's stream by events): one part's scale_kernel runs beside another
  // part's wave_kernel and the parts' dispatch tails interleave (split_parts; tools/split_exp.py,
  // profiles/r05/split).  Results are bitwise those of one launch.
  static constexpr int KMAX = 8;
  int split = 0;             // parts per solve: 0 = auto (split_parts), else MPCQP_SPLIT / mpcqp_set_split
  int fb_parts = 1;          // parts of the last solve (hand-off counters to sum)
  int split_w[KMAX] = {};    // relative part sizes (MPCQP_SPLIT_W="w0,w1,..."); all 0 = equal parts
  // sub[i] / ev_join[i] serve part i >= 1 (part 0 runs on the caller's stream), created lazily: only
  // the parts - 1 streams a split of that size uses, the first time it runs or at mpcqp_reserve
  hipStream_t sub[KMAX] = {};
  hipEvent_t ev_fork = nullptr;
  hipEvent_t ev_join[KMAX] = {};
  // Launch-order hint of the wave path (mpcqp_order.hip; mpcqp_internal.h OrderHint): per robot the
  // cost key and contact mask of its last solve and this solve's order, per part the layout the state
  // was written for.  Sized and zero-filled with the workspace; validity is decided on the device.
  int order_hint = -1;       // -1 per-path default (order_hint_default), 0 off, 1 on: MPCQP_ORDER_HINT / mpcqp_set_order_hint
  int* ord_order = nullptr;
  int* ord_key = nullptr;
  int* ord_contacts = nullptr;
  int* ord_layout = nullptr;  // [KMAX][ORDER_LAYOUT_INTS]
  // the last wave-path solve, for mpcqp_debug_launch_order
  int last_batch = 0, last_parts = 0;
  bool last_hint = false;
  int last_bnd[KMAX + 1] = {};
  int path = 0;              // 0 auto (= 3), 3 Riccati wave; debug library only: 1 dense K^-1, 2 Riccati workgroup
  // host wrapper: device buffers, a private stream and two pinned staging chunks
  hipStream_t hstream = nullptr;
  char* pin[2] = {nullptr, nullptr};
  hipEvent_t pin_ev[2] = {nullptr, nullptr};
  bool pin_busy[2] = {false, false};
  double* d_recs = nullptr;
  mpcqp_result* d_res = nullptr;
  double* d_sol = nullptr;
  size_t cap = 0;
  double* d_bal_recs = nullptr;  // balance host wrapper staging
  mpcqp_result* d_bal_res = nullptr;
  size_t bal_cap = 0;
  char err[256] = {0};
};

// One packed policy network on one device (mpcqp_policy.hip): the loaded TorchScript modules of
// Go1RLController::loadNNparams (Go1RLController.cpp:66-76) together with the controller's constants.
struct mpcqp_policy {
  int device = 0;
  mpcqp::PolicyImage* d_img = nullptr;  // parameters + layer table
  float* d_wts = nullptr;               // packed weights and biases
  int stride0 = 0, stride1 = 0;         // row strides of the two LDS activation buffers, floats
};

namespace {

// Makes the handle's device current for one entry point and restores the caller's current device
// on every return path (a multi-GPU caller such as torch keeps its own device selection).
struct DeviceGuard {
  int prev = -1;
  hipError_t err;
  explicit DeviceGuard(int device) {
    if (hipGetDevice(&prev) != hipSuccess) prev = -1;
    err = hipSetDevice(device);
  }
  ~DeviceGuard() {
    if (prev >= 0) (void)hipSetDevice(prev);
  }
  DeviceGuard(const DeviceGuard&) = delete;
  DeviceGuard& operator=(const DeviceGuard&) = delete;
};

int set_hip_error(mpcqp_handle* h, hipError_t e, const char* where) {
  if (h) snprintf(h->err, sizeof(h->err), "%s: %s", where, hipGetErrorString(e));
  return MPCQP_ERR_HIP;
}

bool params_valid(const mpcqp_params* p) {
  if (!p) return false;
  if (p->horizon < 1 || p->horizon > MPCQP_MAX_HORIZON) return false;
  if (p->max_iter < 1 || p->scaling < 0 || p->check_termination < 0) return false;
  if (p->adaptive_rho && p->adaptive_rho_interval <= 0) return false;  // wall-clock interval unsupported
  if (!(p->rho > 0) || !(p->sigma > 0) || !(p->alpha > 0 && p->alpha < 2)) return false;
  if (!(p->eps_abs >= 0) || !(p->eps_rel >= 0)) return false;
  if (p->scaled_termination != 0) return false;  // reference uses the default (0)
  for (int i = 0; i < MPCQP_STATE_DIM; ++i)
    if (!isfinite(p->q_weights[i])) return false;
  for (int i = 0; i < MPCQP_NUM_DOF; ++i)
    if (!isfinite(p->r_weights[i])) return false;
  return true;
}

// 3 = scale_kernel + wave_kernel (the product path); 1, 2 = cross-check solvers of the debug build
int effective_path(const mpcqp_handle* h) { return h->path != 0 ? h->path : 3; }
size_t work_per_instance(const mpcqp_handle* h) {
  switch (effective_path(h)) {
#ifdef MPCQP_DEBUG_PATHS
    case 1: return mpcqp::workspace_doubles(h->p.horizon);
    case 2: return mpcqp::riccati_workspace_doubles(h->p.horizon);
#endif
    default: return mpcqp::scale_image_doubles(h->p.horizon);  // scale_kernel -> wave_kernel hand-off
  }
}
hipError_t occupancy_for(const mpcqp_handle* h, int* per_cu) {
  switch (effective_path(h)) {
#ifdef MPCQP_DEBUG_PATHS
    case 1: return mpcqp::occupancy_any(h->p.horizon, per_cu);
    case 2: return mpcqp::occupancy_riccati_any(h->p.horizon, per_cu);
#endif
    default: return mpcqp::occupancy_wave_any(h->p, per_cu);
  }
}
// (Re)size the per-instance workspace for `batch` instances of the current path.
hipError_t ensure_workspace(mpcqp_handle* h, int32_t batch, void* stream) {
  const size_t per = work_per_instance(h);
  if (per == 0) return hipSuccess;
  if ((size_t)batch <= h->work_cap && per <= h->work_per) return hipSuccess;
  hipError_t e = hipStreamSynchronize((hipStream_t)stream);
  if (e == hipSuccess) e = hipFree(h->work);
  if (e == hipSuccess) e = hipFree(h->fb);
  if (e == hipSuccess) e = hipFree(h->ord_order);  // (one allocation: order, key, contacts, layout)
  h->work = nullptr;
  h->fb = nullptr;
  h->ord_order = h->ord_key = h->ord_contacts = h->ord_layout = nullptr;
  const size_t cap = (size_t)batch > h->work_cap ? (size_t)batch : h->work_cap;
  h->work_cap = 0;
  h->work_per = 0;
  if (e == hipSuccess) e = hipMalloc(&h->work, sizeof(double) * per * cap);
  if (e == hipSuccess) e = hipMalloc(&h->fb, sizeof(int) * 4 * mpcqp_handle::KMAX);
  if (e == hipSuccess) e = hipMemset(h->fb, 0, sizeof(int) * 4 * mpcqp_handle::KMAX);
  // the launch-order state starts zero-filled: no part's layout matches a batch of zero robots
  const size_t ord_ints = 3 * cap + (size_t)mpcqp::ORDER_LAYOUT_INTS * mpcqp_handle::KMAX;
  if (e == hipSuccess) e = hipMalloc(&h->ord_order, sizeof(int) * ord_ints);
  if (e == hipSuccess) e = hipMemset(h->ord_order, 0, sizeof(int) * ord_ints);
  if (e == hipSuccess) {
    h->ord_key = h->ord_order + cap;
    h->ord_contacts = h->ord_key + cap;
    h->ord_layout = h->ord_contacts + cap;
  }
  if (e == hipSuccess) {
    h->work_cap = cap;
    h->work_per = per;
  }
  return e;
}

// Parts a wave-path solve of `batch` robots is split into.  Auto: three from 3072 robots, two from
// 2048 (measured, tools/split_exp.py, profiles/r05/split: three parts C2 1.630 -> 1.582 ms, C5
// 3.186 -> 2.971 ms, C4 5.44 -> 5.26 ms, C3's 8192-robot shard and 65536 robots unchanged; four
// parts are slower everywhere: the caller's stream plus three internal ones already fill the
// process's four hardware queues, and a fifth stream shares one in order).
int split_parts(const mpcqp_handle* h, int32_t batch) {
  int k = h->split > 0 ? h->split : (batch >= 3072 ? 3 : batch >= 2048 ? 2 : 1);
  if (k > mpcqp_handle::KMAX) k = mpcqp_handle::KMAX;
  if (k > batch) k = batch;
  return k < 1 ? 1 : k;
}

// Whether a wave-path solve (cold, or warm-started from slots) takes its launch order from the
// handle's hint state.  The built-in defaults are per path and set by measurement on records that
// change every call (tools/order_hint_ab.py, profiles/order_hint; DESIGN 5 "Launch order"): 4096
// robots over 40 consecutive ticks, median ms per tick, cold 1.327 -> 1.259 and 1.342 -> 1.250,
// warm 0.691 -> 0.647 and 0.654 -> 0.618 (swing_ticks 5 and 40), each gain several times the
// hint-off repetitions' spread.  A path whose gain falls inside that spread goes back to false.
constexpr bool ORDER_HINT_DEFAULT_COLD = true;
constexpr bool ORDER_HINT_DEFAULT_WARM = true;
bool order_hint_on(const mpcqp_handle* h, bool warm) {
  if (h->order_hint >= 0) return h->order_hint != 0;
  return warm ? ORDER_HINT_DEFAULT_WARM : ORDER_HINT_DEFAULT_COLD;
}

// The internal streams and events of a split into `parts` parts: parts 1 .. parts-1 each get a stream
// and a join event the first time a split of that size runs (or at mpcqp_reserve, for callers that
// capture the solve into a graph).  Nothing is created for an unsplit solve, so a process's hardware
// queues (GPU_MAX_HW_QUEUES = 4) are not filled with streams it never uses: a C3 rank holds the
// caller's stream, RCCL's and the split's two.
hipError_t ensure_split_streams(mpcqp_handle* h, int parts) {
  hipError_t e = hipSuccess;
  if (parts < 2) return e;
  if (!h->ev_fork) e = hipEventCreateWithFlags(&h->ev_fork, hipEventDisableTiming);
  for (int i = 1; i < parts && i < mpcqp_handle::KMAX && e == hipSuccess; ++i) {
    if (!h->sub[i]) e = hipStreamCreateWithFlags(&h->sub[i], hipStreamNonBlocking);
    if (e == hipSuccess && !h->ev_join[i]) e = hipEventCreateWithFlags(&h->ev_join[i], hipEventDisableTiming);
  }
  return e;
}

constexpr size_t PIN_CHUNK = (size_t)2 << 20;  // bytes per pinned staging chunk

bool host_pinned(const void* p) {
  hipPointerAttribute_t at;
  if (hipPointerGetAttributes(&at, p) != hipSuccess) {
    (void)hipGetLastError();
    return false;
  }
  return at.type == hipMemoryTypeHost;
}

// The host wrappers' private stream and pinned staging, created on first use.  The stream is a
// BLOCKING one (hipStreamDefault): it is ordered after work the caller queued on the legacy null
// stream (e.g. hipMemset / torch zeroing of warm slots), as the null-stream wrappers were before.
hipError_t ensure_host_io(mpcqp_handle* h) {
  hipError_t e = hipSuccess;
  if (!h->hstream) e = hipStreamCreateWithFlags(&h->hstream, hipStreamDefault);
  for (int i = 0; i < 2 && e == hipSuccess; ++i) {
    if (!h->pin[i]) e = hipHostMalloc((void**)&h->pin[i], PIN_CHUNK, hipHostMallocDefault);
    if (e == hipSuccess && !h->pin_ev[i]) e = hipEventCreateWithFlags(&h->pin_ev[i], hipEventDisableTiming);
  }
  return e;
}

// Host -> device on the wrapper stream.  A pinned source goes by one DMA; a pageable one through
// the two staging chunks, the host copy of chunk c + 1 overlapping the DMA of chunk c.
hipError_t copy_h2d(mpcqp_handle* h, void* dst, const void* src, size_t bytes) {
  if (host_pinned(src)) return hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, h->hstream);
  hipError_t e = hipSuccess;
  for (size_t off = 0, c = 0; off < bytes && e == hipSuccess; off += PIN_CHUNK, ++c) {
    const int s = (int)(c & 1);
    const size_t len = bytes - off < PIN_CHUNK ? bytes - off : PIN_CHUNK;
    if (h->pin_busy[s]) e = hipEventSynchronize(h->pin_ev[s]);
    if (e != hipSuccess) break;
    memcpy(h->pin[s], (const char*)src + off, len);
    e = hipMemcpyAsync((char*)dst + off, h->pin[s], len, hipMemcpyHostToDevice, h->hstream);
    if (e == hipSuccess) e = hipEventRecord(h->pin_ev[s], h->hstream);
    h->pin_busy[s] = e == hipSuccess;
  }
  return e;
}

// Device -> host on the wrapper stream, synchronous on return (same staging scheme as copy_h2d).
hipError_t copy_d2h(mpcqp_handle* h, void* dst, const void* src, size_t bytes) {
  hipError_t e;
  if (host_pinned(dst)) {
    e = hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, h->hstream);
    return e == hipSuccess ? hipStreamSynchronize(h->hstream) : e;
  }
  // chunk c is copied into staging slot c & 1 while chunk c - 1 is copied out of the other slot
  e = hipSuccess;
  const size_t nch = (bytes + PIN_CHUNK - 1) / PIN_CHUNK;
  for (size_t c = 0; c <= nch && e == hipSuccess; ++c) {
    if (c < nch) {
      const size_t off = c * PIN_CHUNK, len = bytes - off < PIN_CHUNK ? bytes - off : PIN_CHUNK;
      e = hipMemcpyAsync(h->pin[c & 1], (const char*)src + off, len, hipMemcpyDeviceToHost, h->hstream);
      if (e == hipSuccess) e = hipEventRecord(h->pin_ev[c & 1], h->hstream);
    }
    if (e == hipSuccess && c > 0) {
      const size_t off = (c - 1) * PIN_CHUNK, len = bytes - off < PIN_CHUNK ? bytes - off : PIN_CHUNK;
      e = hipEventSynchronize(h->pin_ev[(c - 1) & 1]);
      if (e == hipSuccess) memcpy((char*)dst + off, h->pin[(c - 1) & 1], len);
    }
  }
  h->pin_busy[0] = h->pin_busy[1] = false;
  return e;
}

}  // namespace

extern "C" {

void mpcqp_default_params(mpcqp_params* p, int32_t horizon) {
  if (!p) return;
  memset(p, 0, sizeof(*p));
  p->horizon = horizon;
  p->max_iter = 4000;
  p->scaling = 10;
  p->check_termination = 25;
  p->adaptive_rho = 1;
  p->adaptive_rho_interval = 25;
  p->scaled_termination = 0;
  p->warm_start = 0;
  // Go1CtrlStates.hpp:203-249 defaults
  const double q[13] = {80.0, 80.0, 1.0, 0.0, 0.0, 270.0, 1.0, 1.0, 20.0, 20.0, 20.0, 20.0, 0.0};
  const double r[12] = {1e-5, 1e-5, 1e-6, 1e-5, 1e-5, 1e-6, 1e-5, 1e-5, 1e-6, 1e-5, 1e-5, 1e-6};
  memcpy(p->q_weights, q, sizeof(q));
  memcpy(p->r_weights, r, sizeof(r));
  p->rho = 0.1;
  p->sigma = 1e-6;
  p->alpha = 1.6;
  p->eps_abs = 1e-3;
  p->eps_rel = 1e-3;
  p->eps_prim_inf = 1e-4;
  p->eps_dual_inf = 1e-4;
  p->adaptive_rho_tolerance = 5.0;
}

int32_t mpcqp_record_size(int32_t horizon) {
  if (horizon < 1) return 0;
  return MPCQP_REC_SIZE(horizon);
}

int32_t mpcqp_create(const mpcqp_params* params, int32_t device, mpcqp_handle** out) {
  if (!out) return MPCQP_ERR_INVALID_ARG;
  *out = nullptr;
  if (!params_valid(params)) return MPCQP_ERR_INVALID_ARG;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return MPCQP_ERR_NO_DEVICE;
  if (device < 0 || device >= ndev) return MPCQP_ERR_INVALID_ARG;
  mpcqp_handle* h = new (std::nothrow) mpcqp_handle();
  if (!h) return MPCQP_ERR_ALLOC;
  h->p = *params;
  h->device = device;
  DeviceGuard dg(device);
  hipError_t e = dg.err;
  if (e != hipSuccess) { delete h; return MPCQP_ERR_HIP; }
  int cus = 0, per_cu = 0;
  e = hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device);
  if (e == hipSuccess) e = occupancy_for(h, &per_cu);
  if (e != hipSuccess || cus <= 0) { delete h; return MPCQP_ERR_HIP; }
  if (per_cu < 1) per_cu = 1;
  h->slots = cus * per_cu;
  h->cus = cus;
  if (const char* sp = getenv("MPCQP_SPLIT")) h->split = atoi(sp);
  if (const char* oh = getenv("MPCQP_ORDER_HINT")) {
    const int v = atoi(oh);
    h->order_hint = v < 0 ? -1 : v != 0;
  }
  if (const char* sw = getenv("MPCQP_SPLIT_W")) {
    for (int i = 0; i < mpcqp_handle::KMAX && *sw; ++i) {
      char* end = nullptr;
      const long v = strtol(sw, &end, 10);
      if (end == sw) break;
      h->split_w[i] = v > 0 && v < 1000 ? (int)v : 0;
      sw = *end == ',' ? end + 1 : end;
    }
  }
  *out = h;
  return MPCQP_OK;
}

int32_t mpcqp_destroy(mpcqp_handle* h) {
  if (!h) return MPCQP_ERR_INVALID_ARG;
  DeviceGuard dg(h->device);
  (void)hipFree(h->work);
  (void)hipFree(h->fb);
  (void)hipFree(h->ord_order);
  (void)hipFree(h->d_recs);
  (void)hipFree(h->d_res);
  (void)hipFree(h->d_sol);
  (void)hipFree(h->d_bal_recs);
  (void)hipFree(h->d_bal_res);
  if (h->hstream) (void)hipStreamSynchronize(h->hstream);
  for (int i = 0; i < 2; ++i) {
    if (h->pin_ev[i]) (void)hipEventDestroy(h->pin_ev[i]);
    (void)hipHostFree(h->pin[i]);
  }
  if (h->hstream) (void)hipStreamDestroy(h->hstream);
  for (int i = 0; i < mpcqp_handle::KMAX; ++i) {
    if (h->sub[i]) (void)hipStreamSynchronize(h->sub[i]);
    if (h->sub[i]) (void)hipStreamDestroy(h->sub[i]);
    if (h->ev_join[i]) (void)hipEventDestroy(h->ev_join[i]);
  }
  if (h->ev_fork) (void)hipEventDestroy(h->ev_fork);
  delete h;
  return MPCQP_OK;
}

static int32_t solve_device_impl(mpcqp_handle* h, const double* d_records, int32_t batch,
                                 mpcqp_result* d_results, double* d_solution, double* d_trace,
                                 int32_t trace_cap, void* stream, double* d_state = nullptr,
                                 const int32_t* d_type = nullptr, int32_t type = 0) {
  if (!h || batch < 0 || (batch > 0 && (!d_records || !d_results))) return MPCQP_ERR_INVALID_ARG;
  if (d_state && effective_path(h) != 3) return MPCQP_ERR_INVALID_ARG;  // warm start: the wave path
  if (d_type && effective_path(h) != 3) return MPCQP_ERR_INVALID_ARG;   // typed solve: the wave path
  if (batch == 0) return MPCQP_OK;
  DeviceGuard dg(h->device);
  hipError_t e = dg.err;
  if (e != hipSuccess) return set_hip_error(h, e, "hipSetDevice");
  // grow-only; a capture-safe caller pre-sizes with mpcqp_reserve()
  e = ensure_workspace(h, batch, stream);
  if (e != hipSuccess) return set_hip_error(h, e, "workspace hipMalloc");
  mpcqp::LaunchArgs a;
  a.recs = d_records;
  a.batch = batch;
  a.results = d_results;
  a.solution = d_solution;
  a.work = h->work;
  a.trace = d_trace;
  a.trace_cap = d_trace ? trace_cap : 0;
  a.wstate = d_state;
  a.fallback = h->fb;
  a.grid = batch;
  a.stream = stream;
  a.p = h->p;
  a.hint = mpcqp::OrderHint{};  // input order (the cross-check paths ignore the hint)
  a.type = d_type;
  a.want = type;
  switch (effective_path(h)) {
#ifdef MPCQP_DEBUG_PATHS
    case 1: e = mpcqp::launch_solve_any(a); break;
    case 2: e = mpcqp::launch_riccati_any(a); break;
#endif
    default: {
      const int parts = split_parts(h, batch);
      h->fb_parts = parts;
      const bool hint = order_hint_on(h, d_state != nullptr);
      h->last_batch = batch;
      h->last_parts = parts;
      h->last_hint = hint || d_type;
      // part i's order_kernel, ahead of its scale_kernel and wave_kernel on the part's stream
      auto order_part = [&](mpcqp::LaunchArgs& ai, int i, int b0) {
        if (!hint && !d_type) return hipSuccess;
        if (!hint) {  // a typed solve still needs an order[]: the identity with holes, no stored state
          ai.hint.order = h->ord_order + b0;
          ai.hint.identity = true;
          return mpcqp::launch_order(ai, mpcqp_handle::KMAX);
        }
        ai.hint.order = h->ord_order + b0;
        ai.hint.key = h->ord_key + b0;
        ai.hint.contacts = h->ord_contacts + b0;
        ai.hint.layout = h->ord_layout + mpcqp::ORDER_LAYOUT_INTS * i;
        ai.hint.whole = batch;
        ai.hint.parts = parts;
        ai.hint.part = i;
        ai.hint.first = b0;
        return mpcqp::launch_order(ai, mpcqp_handle::KMAX);
      };
      if (parts == 1) {
        h->last_bnd[0] = 0;
        h->last_bnd[1] = batch;
        e = order_part(a, 0, 0);
        if (e == hipSuccess) e = mpcqp::launch_wave_any(a);
        break;
      }
      // fork: part 0 runs on the caller's stream, every other part on an internal stream that waits
      // for the work queued on the caller's stream so far (parts - 1 streams more: a process has
      // few hardware queues, GPU_MAX_HW_QUEUES = 4, and streams beyond them share one in order)
      e = ensure_split_streams(h, parts);
      if (e == hipSuccess) e = hipEventRecord(h->ev_fork, (hipStream_t)stream);
      const size_t rs = (size_t)MPCQP_REC_SIZE(h->p.horizon), n = (size_t)MPCQP_NUM_DOF * h->p.horizon;
      const size_t ws = (size_t)mpcqp::warm_state_doubles(h->p.horizon);
      // part boundaries: equal parts, or relative sizes split_w when every part gets a robot
      int bnd[mpcqp_handle::KMAX + 1];
      int64_t wsum = 0;
      for (int i = 0; i < parts; ++i) wsum = h->split_w[i] > 0 && wsum >= 0 ? wsum + h->split_w[i] : -1;
      bool weighted = wsum > 0;
      for (int i = 0, wc = 0; i <= parts; ++i) {
        bnd[i] = (int)(weighted ? (int64_t)batch * wc / wsum : (int64_t)batch * i / parts);
        if (i < parts && weighted) wc += h->split_w[i];
      }
      for (int i = 0; i < parts && weighted; ++i) weighted = bnd[i + 1] > bnd[i];
      for (int i = 0; i <= parts && !weighted; ++i) bnd[i] = (int)((int64_t)batch * i / parts);
      for (int i = 0; i <= parts; ++i) h->last_bnd[i] = bnd[i];
      for (int i = 0; i < parts && e == hipSuccess; ++i) {
        const int b0 = bnd[i], b1 = bnd[i + 1];
        mpcqp::LaunchArgs ai = a;
        ai.recs = d_records + rs * b0;
        ai.batch = b1 - b0;
        ai.grid = b1 - b0;
        ai.results = d_results + b0;
        ai.solution = d_solution ? d_solution + n * b0 : nullptr;
        ai.work = h->work + h->work_per * b0;
        ai.trace = d_trace ? d_trace + (size_t)b0 * MPCQP_TRACE_LEN * 4 : nullptr;
        ai.trace_cap = d_trace && trace_cap > b0 ? trace_cap - b0 : 0;
        ai.wstate = d_state ? d_state + ws * b0 : nullptr;
        ai.fallback = h->fb + 4 * i;
        ai.type = d_type ? d_type + b0 : nullptr;
        if (i == 0) {
          ai.stream = stream;
          e = order_part(ai, i, b0);
          if (e == hipSuccess) e = mpcqp::launch_wave_any(ai);
          continue;
        }
        ai.stream = h->sub[i];
        e = hipStreamWaitEvent(h->sub[i], h->ev_fork, 0);
        if (e == hipSuccess) e = order_part(ai, i, b0);
        if (e == hipSuccess) e = mpcqp::launch_wave_any(ai);
        if (e == hipSuccess) e = hipEventRecord(h->ev_join[i], h->sub[i]);
      }
      // join: the caller's stream waits for every other part
      for (int i = 1; i < parts && e == hipSuccess; ++i) e = hipStreamWaitEvent((hipStream_t)stream, h->ev_join[i], 0);
      break;
    }
  }
  if (e != hipSuccess) return set_hip_error(h, e, "solve_kernel launch");
  return MPCQP_OK;
}

int32_t mpcqp_solve_batch_device(mpcqp_handle* h, const double* d_records, int32_t batch,
                                 mpcqp_result* d_results, double* d_solution, void* stream) {
  return solve_device_impl(h, d_records, batch, d_results, d_solution, nullptr, 0, stream);
}

int32_t mpcqp_debug_solve_trace_device(mpcqp_handle* h, const double* d_records, int32_t batch,
                                       mpcqp_result* d_results, double* d_solution,
                                       double* d_trace, int32_t trace_cap, void* stream) {
  return solve_device_impl(h, d_records, batch, d_results, d_solution, d_trace, trace_cap, stream);
}

int32_t mpcqp_warm_state_size(int32_t horizon) {
  if (horizon < 1 || horizon > mpcqp::WAVE_MAX_HORIZON) return 0;
  return mpcqp::warm_state_doubles(horizon);
}

int32_t mpcqp_solve_batch_warm_device(mpcqp_handle* h, const double* d_records, int32_t batch, double* d_state,
                                      mpcqp_result* d_results, double* d_solution, void* stream) {
  if (batch > 0 && !d_state) return MPCQP_ERR_INVALID_ARG;
  return solve_device_impl(h, d_records, batch, d_results, d_solution, nullptr, 0, stream, d_state);
}

int32_t mpcqp_solve_batch_warm_typed_device(mpcqp_handle* h, const double* d_records, int32_t batch, double* d_state,
                                            const int32_t* d_type, int32_t type, mpcqp_result* d_results,
                                            double* d_solution, void* stream) {
  if (batch > 0 && !d_state) return MPCQP_ERR_INVALID_ARG;
  return solve_device_impl(h, d_records, batch, d_results, d_solution, nullptr, 0, stream, d_state, d_type, type);
}

static int32_t solve_host_impl(mpcqp_handle* h, const double* h_records, int32_t batch, double* d_state,
                               mpcqp_result* h_results, double* h_solution) {
  if (!h || batch < 0 || (batch > 0 && (!h_records || !h_results))) return MPCQP_ERR_INVALID_ARG;
  if (batch == 0) return MPCQP_OK;
  if (d_state && effective_path(h) != 3) return MPCQP_ERR_INVALID_ARG;  // warm start: the wave path
  DeviceGuard dg(h->device);
  hipError_t e = dg.err;
  if (e != hipSuccess) return set_hip_error(h, e, "hipSetDevice");
  e = ensure_host_io(h);
  if (e != hipSuccess) return set_hip_error(h, e, "host staging");
  const size_t rs = (size_t)MPCQP_REC_SIZE(h->p.horizon);
  const size_t n = (size_t)MPCQP_NUM_DOF * h->p.horizon;
  if ((size_t)batch > h->cap) {
    (void)hipStreamSynchronize(h->hstream);
    (void)hipFree(h->d_recs);
    (void)hipFree(h->d_res);
    (void)hipFree(h->d_sol);
    h->d_recs = nullptr; h->d_res = nullptr; h->d_sol = nullptr; h->cap = 0;
    e = hipMalloc(&h->d_recs, sizeof(double) * rs * batch);
    if (e == hipSuccess) e = hipMalloc(&h->d_res, sizeof(mpcqp_result) * batch);
    if (e == hipSuccess) e = hipMalloc(&h->d_sol, sizeof(double) * n * batch);
    if (e != hipSuccess) return set_hip_error(h, e, "hipMalloc");
    h->cap = batch;
  }
  e = copy_h2d(h, h->d_recs, h_records, sizeof(double) * rs * batch);
  if (e != hipSuccess) return set_hip_error(h, e, "records H2D");
  int32_t rc = solve_device_impl(h, h->d_recs, batch, h->d_res, h_solution ? h->d_sol : nullptr,
                                 nullptr, 0, h->hstream, d_state);
  if (rc != MPCQP_OK) return rc;
  e = copy_d2h(h, h_results, h->d_res, sizeof(mpcqp_result) * batch);
  if (e == hipSuccess && h_solution) e = copy_d2h(h, h_solution, h->d_sol, sizeof(double) * n * batch);
  if (e != hipSuccess) return set_hip_error(h, e, "results D2H");
  return MPCQP_OK;
}

int32_t mpcqp_solve_batch_host(mpcqp_handle* h, const double* h_records, int32_t batch,
                               mpcqp_result* h_results, double* h_solution) {
  return solve_host_impl(h, h_records, batch, nullptr, h_results, h_solution);
}

int32_t mpcqp_solve_batch_warm_host(mpcqp_handle* h, const double* h_records, int32_t batch, double* d_state,
                                    mpcqp_result* h_results, double* h_solution) {
  if (batch > 0 && !d_state) return MPCQP_ERR_INVALID_ARG;
  return solve_host_impl(h, h_records, batch, d_state, h_results, h_solution);
}

int32_t mpcqp_build_qp_device(mpcqp_handle* h, const double* d_records, int32_t batch, double* d_P,
                              double* d_q, double* d_l, double* d_u, void* stream) {
  if (!h || batch < 0 || (batch > 0 && (!d_records || !d_P || !d_q || !d_l || !d_u)))
    return MPCQP_ERR_INVALID_ARG;
  if (batch == 0) return MPCQP_OK;
  DeviceGuard dg(h->device);
  hipError_t e = dg.err;
  if (e != hipSuccess) return set_hip_error(h, e, "hipSetDevice");
  mpcqp::LaunchArgs a;
  memset(&a, 0, sizeof(a));
  a.recs = d_records;
  a.batch = batch;
  a.stream = stream;
  a.p = h->p;
  e = mpcqp::launch_build_any(a, d_P, d_q, d_l, d_u);
  if (e != hipSuccess) return set_hip_error(h, e, "build_qp_kernel launch");
  return MPCQP_OK;
}

int32_t mpcqp_assemble_records_device(int32_t horizon, const double* d_states, int32_t batch, double* d_records,
                                      void* stream) {
  if (horizon < 1 || horizon > MPCQP_MAX_HORIZON || batch < 0 || (batch > 0 && (!d_states || !d_records)))
    return MPCQP_ERR_INVALID_ARG;
  if (batch == 0) return MPCQP_OK;
  return mpcqp::launch_assemble(horizon, d_states, batch, d_records, stream) == hipSuccess ? MPCQP_OK : MPCQP_ERR_HIP;
}

int32_t mpcqp_copy_warm_slots_device(int32_t horizon, const double* d_src, const int32_t* d_src_idx, double* d_dst,
                                     const int32_t* d_dst_idx, int32_t count, void* stream) {
  if (horizon < 1 || horizon > MPCQP_MAX_HORIZON || count < 0 || (count > 0 && (!d_src || !d_dst)))
    return MPCQP_ERR_INVALID_ARG;
  if (count == 0) return MPCQP_OK;
  return mpcqp::launch_copy_slots(d_src, d_src_idx, d_dst, d_dst_idx, count, mpcqp_warm_state_size(horizon), stream) ==
                 hipSuccess
             ? MPCQP_OK
             : MPCQP_ERR_HIP;
}

void mpcqp_plan_default_params(mpcqp_plan_params* p) {
  if (!p) return;
  const double sx[4] = {0.17, 0.17, -0.17, -0.17}, sy[4] = {0.15, -0.15, 0.15, -0.15};  // A1CtrlStates.h:45-47
  const double kp[3] = {300.0, 400.0, 400.0}, kd[3] = {8.0, 8.0, 8.0};                  // :105-111
  const double gc0[4] = {0.0, 120.0, 120.0, 0.0};                                       // :325
  for (int i = 0; i < 4; ++i) {
    p->default_foot_pos[3 * i] = sx[i];
    p->default_foot_pos[3 * i + 1] = sy[i];
    p->default_foot_pos[3 * i + 2] = -0.35;
    for (int k = 0; k < 3; ++k) {
      p->kp_foot[3 * i + k] = kp[k];
      p->kd_foot[3 * i + k] = kd[k];
    }
    p->gait_counter_speed[i] = 2.0;  // :103
    p->gait_counter_init[i] = gc0[i];
  }
  p->counter_per_gait = 120 * 2;     // :24
  p->counter_per_swing = 120;        // :25
  p->control_dt = 0.5 / 1000.0;      // :333, MAIN_UPDATE_FREQUENCY (A1Params.h:11)
  p->foot_force_low = 30.0;          // A1Params.h:38
  p->foot_delta_x_limit = 0.1;       // A1Params.h:44
  p->foot_delta_y_limit = 0.1;       // A1Params.h:45
  p->swing_clearance1 = (double)0.0f;  // A1Params.h:41
  p->swing_clearance2 = (double)0.4f;  // A1Params.h:42
  p->terrain = 1;                    // stance_leg_control_type, A1CtrlStates.h:21
  p->use_terrain_adapt = 1;          // A1CtrlStates.h:22
}

int32_t mpcqp_plan_state_size(void) { return mpcqp::plan_state_doubles(); }

int32_t mpcqp_leg_plan_typed_device(const mpcqp_plan_params* pp, double dt, double* d_states,
                                    const double* d_plan_in, int32_t batch, double* d_plan_state,
                                    double* d_tq_records, double* d_plan_out, const int32_t* d_type, void* stream) {
  if (!pp || batch < 0 || !(dt > 0.0) || !isfinite(dt)) return MPCQP_ERR_INVALID_ARG;
  if (batch > 0 && (!d_states || !d_plan_in || !d_plan_state)) return MPCQP_ERR_INVALID_ARG;
  if (batch == 0) return MPCQP_OK;
  return mpcqp::launch_leg_plan(*pp, dt, d_states, d_plan_in, batch, d_plan_state, d_tq_records, d_plan_out, d_type,
                                stream) == hipSuccess
             ? MPCQP_OK
             : MPCQP_ERR_HIP;
}

int32_t mpcqp_leg_plan_device(const mpcqp_plan_params* pp, double dt, double* d_states, const double* d_plan_in,
                              int32_t batch, double* d_plan_state, double* d_tq_records, double* d_plan_out,
                              void* stream) {
  return mpcqp_leg_plan_typed_device(pp, dt, d_states, d_plan_in, batch, d_plan_state, d_tq_records, d_plan_out,
                                     nullptr, stream);
}

void mpcqp_command_default_params(mpcqp_command_params* p) {
  if (!p) return;
  p->body_height_init = 0.2;     // GazeboA1ROS.h:133
  p->body_height_max = 0.32;     // A1Params.h:16
  p->body_height_min = 0.1;      // A1Params.h:17
  p->vel_lock_threshold = 0.05;  // GazeboA1ROS.cpp:180
  p->kp_linear[0] = 100.0;       // Go1CtrlStates.hpp:279-281
  p->kp_linear[1] = 100.0;
  p->kp_linear[2] = 300.0;
  p->kp_linear_lock_x = 100.0;   // Go1CtrlStates.hpp:304-305
  p->kp_linear_lock_y = 100.0;
}

int32_t mpcqp_command_state_size(void) { return MPCQP_CS_SIZE; }

int32_t mpcqp_command_device(const mpcqp_command_params* cp, double dt, double* d_cmd, double* d_states,
                             double* d_plan_in, int32_t batch, double* d_cmd_state, void* stream) {
  if (!cp || batch < 0 || !isfinite(dt)) return MPCQP_ERR_INVALID_ARG;
  if (batch > 0 && (!d_cmd || !d_states || !d_plan_in || !d_cmd_state)) return MPCQP_ERR_INVALID_ARG;
  if (batch == 0) return MPCQP_OK;
  return mpcqp::launch_command(*cp, dt, d_cmd, d_states, d_plan_in, batch, d_cmd_state, stream) == hipSuccess
             ? MPCQP_OK
             : MPCQP_ERR_HIP;
}

void mpcqp_policy_default_params(mpcqp_policy_params* p) {
  if (!p) return;
  memset(p, 0, sizeof(*p));
  p->n_hidden = 3;  // cpp_model.pt: 48 -> 512 -> 256 -> 128 -> 12
  p->hidden[0] = 512;
  p->hidden[1] = 256;
  p->hidden[2] = 128;
  p->servo_clamp = 0;  // Go1RLController.cpp:139-142 never clamps percent
  p->decimation = 1;
  for (int i = 0; i < 36; ++i) p->obs_scale[i] = 1.0;  // gravityScale_, dofPosScale_ (Go1Observation.hpp:54, :59)
  for (int i = 0; i < 3; ++i) {
    p->obs_scale[i] = 2.0;       // linVelScale_ (:52)
    p->obs_scale[3 + i] = 0.25;  // angVelScale_ (:53)
  }
  p->obs_scale[9] = 2.0;  // commandScale_ (:55)
  p->obs_scale[10] = 2.0;
  p->obs_scale[11] = 0.25;
  for (int i = 24; i < 36; ++i) p->obs_scale[i] = 0.05;  // dofVelScale_ (:60)
  p->clip_obs = 100.0;      // Go1Observation.hpp:449
  p->clip_action = 100.0;   // Go1RLController.hpp:84
  p->action_scale = 0.25;   // Go1RLController.hpp:88
  const double lo[3] = {-0.9425, -0.4817, -2.6285}, hi[3] = {0.9425, 2.7855, -0.9320};  // Go1RLController.cpp:36-37
  const double kpw[3] = {20.0, 50.0, 50.0}, kdw[3] = {1.0, 2.0, 2.0};                    // :79-86
  const double kpf[3] = {20.0, 30.0, 60.0}, kpr[3] = {20.0, 80.0, 140.0}, kds[3] = {5.0, 8.0, 12.0};  // :125-132
  for (int leg = 0; leg < 4; ++leg) {
    const double side = (leg & 1) ? -0.1 : 0.1;
    p->default_joint_pos[3 * leg] = side;  // Go1CtrlStates.hpp:75-78
    p->default_joint_pos[3 * leg + 1] = leg < 2 ? 0.8 : 1.0;
    p->default_joint_pos[3 * leg + 2] = -1.5;
    p->stand_pos[3 * leg] = side;  // Go1RLController.cpp:122-123
    p->stand_pos[3 * leg + 1] = 0.6;
    p->stand_pos[3 * leg + 2] = -1.3;
    for (int k = 0; k < 3; ++k) {
      p->pose_lower[3 * leg + k] = lo[k];
      p->pose_upper[3 * leg + k] = hi[k];
      p->kp_walk[3 * leg + k] = kpw[k];
      p->kd_walk[3 * leg + k] = kdw[k];
      p->kp_servo[3 * leg + k] = leg < 2 ? kpf[k] : kpr[k];
      p->kd_servo[3 * leg + k] = kds[k];
    }
  }
  p->servo_ticks = 1000.0;  // :139
}

int32_t mpcqp_policy_params_size(void) { return (int32_t)sizeof(mpcqp_policy_params); }

int32_t mpcqp_policy_state_size(void) { return MPCQP_PS_SIZE; }

int32_t mpcqp_policy_create(const mpcqp_policy_params* params, const float* const* h_weights,
                            const float* const* h_biases, int32_t device, mpcqp_policy** out) {
  if (!out) return MPCQP_ERR_INVALID_ARG;
  *out = nullptr;
  if (!params || !h_weights || !h_biases) return MPCQP_ERR_INVALID_ARG;
  mpcqp::PolicyImage img;
  size_t n_floats = 0;
  int s0 = 0, s1 = 0;
  if (!mpcqp::policy_layout(*params, &img, &n_floats, &s0, &s1)) return MPCQP_ERR_INVALID_ARG;
  if (params->decimation < 1 || !(params->servo_ticks > 0.0) || !isfinite(params->servo_ticks))
    return MPCQP_ERR_INVALID_ARG;
  for (int l = 0; l < img.n_layers; ++l)
    if (!h_weights[l] || !h_biases[l]) return MPCQP_ERR_INVALID_ARG;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return MPCQP_ERR_NO_DEVICE;
  if (device < 0 || device >= ndev) return MPCQP_ERR_INVALID_ARG;
  mpcqp_policy* pol = new (std::nothrow) mpcqp_policy();
  float* host = new (std::nothrow) float[n_floats];
  if (!pol || !host) {
    delete pol;
    delete[] host;
    return MPCQP_ERR_ALLOC;
  }
  mpcqp::policy_pack(img, h_weights, h_biases, host);
  pol->device = device;
  pol->stride0 = s0;
  pol->stride1 = s1;
  DeviceGuard dg(device);
  hipError_t e = dg.err;
  if (e == hipSuccess) e = mpcqp::policy_reserve_lds();
  if (e == hipSuccess) e = hipMalloc(&pol->d_img, sizeof(img));
  if (e == hipSuccess) e = hipMalloc(&pol->d_wts, sizeof(float) * n_floats);
  if (e == hipSuccess) e = hipMemcpy(pol->d_img, &img, sizeof(img), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(pol->d_wts, host, sizeof(float) * n_floats, hipMemcpyHostToDevice);
  delete[] host;
  if (e != hipSuccess) {
    (void)hipFree(pol->d_img);
    (void)hipFree(pol->d_wts);
    delete pol;
    return MPCQP_ERR_HIP;
  }
  *out = pol;
  return MPCQP_OK;
}

int32_t mpcqp_policy_destroy(mpcqp_policy* p) {
  if (!p) return MPCQP_ERR_INVALID_ARG;
  DeviceGuard dg(p->device);
  (void)hipFree(p->d_img);
  (void)hipFree(p->d_wts);
  delete p;
  return MPCQP_OK;
}

int32_t mpcqp_policy_device(const mpcqp_policy* policy, const double* d_sensors, const double* d_states,
                            const double* d_plan_in, const double* d_cmd, int32_t batch, double* d_policy_state,
                            const int32_t* d_type, int32_t type, double* d_joint_torques, double* d_policy_out,
                            void* stream) {
  if (!policy || batch < 0) return MPCQP_ERR_INVALID_ARG;
  if (batch > 0 && (!d_sensors || !d_states || !d_plan_in || !d_cmd || !d_policy_state || !d_joint_torques))
    return MPCQP_ERR_INVALID_ARG;
  if (batch == 0) return MPCQP_OK;
  return mpcqp::launch_policy(policy->d_img, policy->d_wts, policy->stride0, policy->stride1, d_sensors, d_states,
                              d_plan_in, d_cmd, batch, d_policy_state, d_type, type, d_joint_torques, d_policy_out,
                              stream) == hipSuccess
             ? MPCQP_OK
             : MPCQP_ERR_HIP;
}

void mpcqp_est_default_params(mpcqp_est_params* p) {
  if (!p) return;
  const double ox[4] = {0.1881, 0.1881, -0.1881, -0.1881};    // GazeboA1ROS.cpp:76-79
  const double oy[4] = {0.04675, -0.04675, 0.04675, -0.04675};  // :80-83
  const double mo[4] = {0.08, -0.08, 0.08, -0.08};            // :84-87
  for (int i = 0; i < 4; ++i) {
    p->rho_fix[i][0] = ox[i];
    p->rho_fix[i][1] = oy[i];
    p->rho_fix[i][2] = mo[i];
    p->rho_fix[i][3] = 0.213;  // :88
    p->rho_fix[i][4] = 0.213;  // :89
    for (int k = 0; k < 3; ++k) p->rho_opt[i][k] = 0.0;  // :95
  }
  p->process_noise_pimu = 0.01;           // A1BasicEKF.h:16
  p->process_noise_vimu = 0.01;           // :17
  p->process_noise_pfoot = 0.01;          // :18
  p->sensor_noise_pimu_rel_foot = 0.001;  // :19
  p->sensor_noise_vimu_rel_foot = 0.1;    // :20
  p->sensor_noise_zfoot = 0.001;          // :21
  p->height_noise_no_flat = 1e5;          // A1BasicEKF.cpp:51
  p->init_height = 0.09;                  // :63
  p->init_cov = 3.0;                      // :59
  p->gravity = 9.81;                      // :76
  p->contact_force_scale = 100.0;         // :83
  p->drift_threshold = 1e-6;              // :143
  p->drift_divisor = 10.0;                // :146
  p->assume_flat_ground = 1;              // :40
  p->pad_ = 0;
}

int32_t mpcqp_est_params_size(void) { return (int32_t)sizeof(mpcqp_est_params); }

int32_t mpcqp_estimator_state_size(void) { return mpcqp::estimator_state_doubles(); }

int32_t mpcqp_state_estimate_device(const mpcqp_est_params* pp, double dt, const double* d_sensors,
                                    double* d_plan_in, double* d_states, int32_t batch, double* d_est_state,
                                    double* d_tq_records, double* d_est_out, void* stream) {
  if (!pp || batch < 0 || !(dt > 0.0) || !isfinite(dt)) return MPCQP_ERR_INVALID_ARG;
  if (batch > 0 && (!d_sensors || !d_plan_in || !d_states || !d_est_state)) return MPCQP_ERR_INVALID_ARG;
  if (batch == 0) return MPCQP_OK;
  return mpcqp::launch_state_estimate(*pp, dt, d_sensors, d_plan_in, d_states, batch, d_est_state, d_tq_records,
                                      d_est_out, stream) == hipSuccess
             ? MPCQP_OK
             : MPCQP_ERR_HIP;
}

void mpcqp_plant_default_params(mpcqp_plant_params* p) {
  if (!p) return;
  mpcqp_est_params e;
  mpcqp_est_default_params(&e);  // the same leg geometry, so the estimator's kinematics and the plant's agree
  for (int i = 0; i < 4; ++i) {
    for (int k = 0; k < 5; ++k) p->rho_fix[i][k] = e.rho_fix[i][k];
    for (int k = 0; k < 3; ++k) p->rho_opt[i][k] = e.rho_opt[i][k];
    p->default_joint_pos[3 * i] = 0.0;
    p->default_joint_pos[3 * i + 1] = 0.8;
    p->default_joint_pos[3 * i + 2] = -1.6;
  }
  p->mass = 13.0;  // Go1CtrlStates.hpp:145-195
  for (int k = 0; k < 9; ++k) p->inertia[k] = 0.0;
  p->inertia[0] = 0.0168352186;
  p->inertia[4] = 0.0656071082;
  p->inertia[8] = 0.0742720659;
  p->mu = 0.6;
  p->gravity = 9.81;
  p->joint_inertia[0] = 0.03;  // the model's own choice, not identified from a robot description
  p->joint_inertia[1] = 0.03;
  p->joint_inertia[2] = 0.01;
  for (int k = 0; k < 3; ++k) p->joint_damping[k] = 0.0;
  p->min_height = 0.05;
  p->substeps = 4;
  p->pad_ = 0;
}

int32_t mpcqp_plant_params_size(void) { return (int32_t)sizeof(mpcqp_plant_params); }

int32_t mpcqp_plant_state_size(void) { return MPCQP_PN_SIZE; }

int32_t mpcqp_plant_step_device(const mpcqp_plant_params* pp, double dt, const double* d_joint_torques,
                                int32_t batch, double* d_plant_state, const double* d_plant_init,
                                double* d_sensors, double* d_plan_in, double* d_states, double* d_tq_records,
                                double* d_plant_out, void* stream) {
  if (!pp || batch < 0 || !(dt > 0.0) || !isfinite(dt)) return MPCQP_ERR_INVALID_ARG;
  if (pp->substeps < 1 || pp->substeps > 16) return MPCQP_ERR_INVALID_ARG;
  if (batch > 0 && (!d_joint_torques || !d_plant_state)) return MPCQP_ERR_INVALID_ARG;
  if (batch == 0) return MPCQP_OK;
  return mpcqp::launch_plant(*pp, dt, d_joint_torques, batch, d_plant_state, d_plant_init, d_sensors, d_plan_in,
                             d_states, d_tq_records, d_plant_out, stream) == hipSuccess
             ? MPCQP_OK
             : MPCQP_ERR_HIP;
}

int32_t mpcqp_plant_step_wrench_device(const mpcqp_plant_params* pp, double dt, const double* d_joint_torques,
                                       const double* d_wrench, int32_t batch, double* d_plant_state,
                                       const double* d_plant_init, double* d_sensors, double* d_plan_in,
                                       double* d_states, double* d_tq_records, double* d_plant_out, void* stream) {
  if (!pp || batch < 0 || !(dt > 0.0) || !isfinite(dt)) return MPCQP_ERR_INVALID_ARG;
  if (pp->substeps < 1 || pp->substeps > 16) return MPCQP_ERR_INVALID_ARG;
  if (batch > 0 && (!d_joint_torques || !d_plant_state)) return MPCQP_ERR_INVALID_ARG;
  if (batch == 0) return MPCQP_OK;
  return mpcqp::launch_plant_wrench(*pp, dt, d_joint_torques, d_wrench, batch, d_plant_state, d_plant_init, d_sensors,
                                    d_plan_in, d_states, d_tq_records, d_plant_out, stream) == hipSuccess
             ? MPCQP_OK
             : MPCQP_ERR_HIP;
}

int32_t mpcqp_plant_step_terrain_device(const mpcqp_plant_params* pp, double dt, const double* d_joint_torques,
                                        const double* d_wrench, const double* d_terrain, int32_t terrain_rows,
                                        const double* d_episode_state, int32_t batch, double* d_plant_state,
                                        const double* d_plant_init, double* d_sensors, double* d_plan_in,
                                        double* d_states, double* d_tq_records, double* d_plant_out, void* stream) {
  if (!pp || batch < 0 || !(dt > 0.0) || !isfinite(dt)) return MPCQP_ERR_INVALID_ARG;
  if (pp->substeps < 1 || pp->substeps > 16) return MPCQP_ERR_INVALID_ARG;
  if (batch > 0 && (!d_joint_torques || !d_plant_state)) return MPCQP_ERR_INVALID_ARG;
  if (d_terrain && (terrain_rows < 1 || (!d_episode_state && terrain_rows < batch))) return MPCQP_ERR_INVALID_ARG;
  if (batch == 0) return MPCQP_OK;
  return mpcqp::launch_plant_terrain(*pp, dt, d_joint_torques, d_wrench, d_terrain, terrain_rows, d_episode_state,
                                     batch, d_plant_state, d_plant_init, d_sensors, d_plan_in, d_states, d_tq_records,
                                     d_plant_out, stream) == hipSuccess
             ? MPCQP_OK
             : MPCQP_ERR_HIP;
}

int32_t mpcqp_plant_step_field_device(const mpcqp_plant_params* pp, double dt, const double* d_joint_torques,
                                      const double* d_wrench, const double* d_field, int32_t field_rows,
                                      const double* d_heights, int32_t heights_len, const double* d_episode_state,
                                      int32_t batch, double* d_plant_state, const double* d_plant_init,
                                      double* d_sensors, double* d_plan_in, double* d_states, double* d_tq_records,
                                      double* d_plant_out, void* stream) {
  if (!pp || batch < 0 || !(dt > 0.0) || !isfinite(dt)) return MPCQP_ERR_INVALID_ARG;
  if (pp->substeps < 1 || pp->substeps > 16) return MPCQP_ERR_INVALID_ARG;
  if (batch > 0 && (!d_joint_torques || !d_plant_state)) return MPCQP_ERR_INVALID_ARG;
  if (d_field && (field_rows < 1 || (!d_episode_state && field_rows < batch) || !d_heights || heights_len < 4))
    return MPCQP_ERR_INVALID_ARG;
  if (batch == 0) return MPCQP_OK;
  return mpcqp::launch_plant_field(*pp, dt, d_joint_torques, d_wrench, d_field, field_rows, d_heights, heights_len,
                                   d_episode_state, batch, d_plant_state, d_plant_init, d_sensors, d_plan_in,
                                   d_states, d_tq_records, d_plant_out, stream) == hipSuccess
             ? MPCQP_OK
             : MPCQP_ERR_HIP;
}

void mpcqp_disturb_default_params(mpcqp_disturb_params* p) {
  if (!p) return;
  p->load_mass_max = 0.0;
  p->gravity = 9.81;
  p->bias_acc = 0.0;
  p->bias_gyro = 0.0;
  p->push_force[0] = p->push_force[1] = 0.0;
  for (int k = 0; k < 3; ++k) p->load_point[k] = p->push_point[k] = 0.0;
  for (int k = 0; k < 4; ++k) p->sigma[k] = 0.0;
  p->seed[0] = 0u;
  p->seed[1] = 0u;
  p->push_start = 0;
  p->push_interval = 0;
  p->push_duration = 1;
  p->dir_count = 0;
}

int32_t mpcqp_disturb_params_size(void) { return (int32_t)sizeof(mpcqp_disturb_params); }

int32_t mpcqp_disturb_buffers_size(void) { return (int32_t)sizeof(mpcqp_disturb_buffers); }

int32_t mpcqp_disturb_device(const mpcqp_disturb_params* dp, const mpcqp_disturb_buffers* buf, int32_t batch,
                             void* stream) {
  if (!dp || !buf || batch < 0) return MPCQP_ERR_INVALID_ARG;
  if (dp->push_interval < 0) return MPCQP_ERR_INVALID_ARG;
  if (dp->push_interval > 0) {
    if (dp->push_duration < 1 || dp->push_duration > dp->push_interval || dp->push_start < 0)
      return MPCQP_ERR_INVALID_ARG;
    if (!buf->d_dirs || dp->dir_count < 1) return MPCQP_ERR_INVALID_ARG;
  }
  if (!buf->d_episode_state || !buf->d_wrench) return MPCQP_ERR_INVALID_ARG;
  if ((buf->d_sensors == nullptr) != (buf->d_sensors_noisy == nullptr)) return MPCQP_ERR_INVALID_ARG;
  if (buf->d_sensors && buf->d_sensors == buf->d_sensors_noisy) return MPCQP_ERR_INVALID_ARG;
  if (batch == 0) return MPCQP_OK;
  return mpcqp::launch_disturb(*dp, *buf, batch, stream) == hipSuccess ? MPCQP_OK : MPCQP_ERR_HIP;
}

void mpcqp_episode_default_params(mpcqp_episode_params* p) {
  if (!p) return;
  p->dt = 0.0025;
  p->tilt_max = 0.5;
  p->height_min = 0.12;
  p->height_max = 0.6;
  p->seed[0] = 0u;
  p->seed[1] = 0u;
  p->max_ticks = 2000;
  p->pool_count = 0;
  p->script_count = 0;
  p->script_segments = 0;
  p->log_len = 4;
  p->pad_ = 0;
}

int32_t mpcqp_episode_params_size(void) { return (int32_t)sizeof(mpcqp_episode_params); }

int32_t mpcqp_episode_buffers_size(void) { return (int32_t)sizeof(mpcqp_episode_buffers); }

int32_t mpcqp_episode_state_size(void) { return MPCQP_ES_SIZE; }

int32_t mpcqp_episode_device(const mpcqp_episode_params* ep, const mpcqp_episode_buffers* buf, int32_t batch,
                             double* d_episode_state, void* stream) {
  if (!ep || !buf || batch < 0) return MPCQP_ERR_INVALID_ARG;
  if (batch == 0) return MPCQP_OK;
  if (!d_episode_state || !buf->d_plant_out || !buf->d_plant_state) return MPCQP_ERR_INVALID_ARG;
  if (!(ep->dt > 0.0) || !isfinite(ep->dt) || ep->max_ticks < 1 || ep->pool_count < 0) return MPCQP_ERR_INVALID_ARG;
  if (buf->d_scripts && (ep->script_count < 1 || ep->script_segments < 1)) return MPCQP_ERR_INVALID_ARG;
  if (buf->d_log && ep->log_len < 1) return MPCQP_ERR_INVALID_ARG;
  if (buf->est_state_size < 0 || buf->plan_state_size < 0 || buf->cmd_state_size < 0 || buf->policy_state_size < 0 ||
      buf->warm_size < 0)
    return MPCQP_ERR_INVALID_ARG;
  // the rows are cleared with 16-byte stores
  const void* ptrs[] = {d_episode_state,     buf->d_plant_out,  buf->d_plant_state, buf->d_plant_init,
                        buf->d_joint_torques, buf->d_sensors,    buf->d_cmd,         buf->d_results,
                        buf->d_pool,          buf->d_scripts,    buf->d_states,
                        buf->d_log,         buf->d_totals,     buf->d_est_state,   buf->d_plan_state,
                        buf->d_cmd_state,     buf->d_policy_state, buf->d_warm};
  for (const void* p : ptrs)
    if ((reinterpret_cast<uintptr_t>(p) & 15u) != 0) return MPCQP_ERR_INVALID_ARG;
  return mpcqp::launch_episode(*ep, *buf, batch, d_episode_state, stream) == hipSuccess ? MPCQP_OK : MPCQP_ERR_HIP;
}

void mpcqp_balance_default_params(mpcqp_balance_params* p) {
  if (!p) return;
  const double q[6] = {1.0, 1.0, 1.0, 400.0, 400.0, 100.0};  // A1RobotControl.cpp:11
  for (int i = 0; i < 6; ++i) p->q_diag[i] = q[i];
  p->r = 1e-3;  // :12
  p->mu = 0.7;  // :13
  p->f_min = 0.0;
  p->f_max = 180.0;  // :14-15
}

int32_t mpcqp_balance_solve_typed_device(mpcqp_handle* h, const mpcqp_balance_params* bp, const double* d_records,
                                         int32_t batch, const int32_t* d_type, int32_t type, mpcqp_result* d_results,
                                         void* stream) {
  if (!h || !bp || batch < 0 || (batch > 0 && (!d_records || !d_results))) return MPCQP_ERR_INVALID_ARG;
  if (batch == 0) return MPCQP_OK;
  DeviceGuard dg(h->device);
  hipError_t e = dg.err;
  if (e != hipSuccess) return set_hip_error(h, e, "hipSetDevice");
  e = mpcqp::launch_balance(*bp, h->p, d_records, batch, d_type, type, d_results, stream);
  if (e != hipSuccess) return set_hip_error(h, e, "balance_kernel launch");
  return MPCQP_OK;
}

int32_t mpcqp_balance_solve_device(mpcqp_handle* h, const mpcqp_balance_params* bp, const double* d_records,
                                   int32_t batch, mpcqp_result* d_results, void* stream) {
  return mpcqp_balance_solve_typed_device(h, bp, d_records, batch, nullptr, 0, d_results, stream);
}

void mpcqp_balance_default_gains(mpcqp_balance_gains* g) {
  if (!g) return;
  const double kp[3] = {100.0, 100.0, 300.0}, kd[3] = {70.0, 70.0, 120.0};  // Go1CtrlStates.hpp:279-288
  const double ap[3] = {150.0, 150.0, 1.0}, ad[3] = {4.5, 4.5, 30.0};       // :293-302
  for (int i = 0; i < 3; ++i) {
    g->kp_linear[i] = kp[i];
    g->kd_linear[i] = kd[i];
    g->kp_angular[i] = ap[i];
    g->kd_angular[i] = ad[i];
  }
}

int32_t mpcqp_assemble_balance_device(const mpcqp_balance_gains* gains, const double* d_states,
                                      const double* d_plan_in, const double* d_cmd_state, int32_t batch,
                                      double* d_bal_records, void* stream) {
  if (!gains || batch < 0 || (batch > 0 && (!d_states || !d_plan_in || !d_bal_records))) return MPCQP_ERR_INVALID_ARG;
  if (batch == 0) return MPCQP_OK;
  return mpcqp::launch_assemble_balance(*gains, d_states, d_plan_in, d_cmd_state, batch, d_bal_records, stream) ==
                 hipSuccess
             ? MPCQP_OK
             : MPCQP_ERR_HIP;
}

int32_t mpcqp_balance_solve_host(mpcqp_handle* h, const mpcqp_balance_params* bp, const double* h_records,
                                 int32_t batch, mpcqp_result* h_results) {
  if (!h || !bp || batch < 0 || (batch > 0 && (!h_records || !h_results))) return MPCQP_ERR_INVALID_ARG;
  if (batch == 0) return MPCQP_OK;
  DeviceGuard dg(h->device);
  hipError_t e = dg.err;
  if (e != hipSuccess) return set_hip_error(h, e, "hipSetDevice");
  e = ensure_host_io(h);
  if (e != hipSuccess) return set_hip_error(h, e, "host staging");
  if ((size_t)batch > h->bal_cap) {
    (void)hipStreamSynchronize(h->hstream);
    (void)hipFree(h->d_bal_recs);
    (void)hipFree(h->d_bal_res);
    h->d_bal_recs = nullptr; h->d_bal_res = nullptr; h->bal_cap = 0;
    e = hipMalloc(&h->d_bal_recs, sizeof(double) * MPCQP_BAL_SIZE * batch);
    if (e == hipSuccess) e = hipMalloc(&h->d_bal_res, sizeof(mpcqp_result) * batch);
    if (e != hipSuccess) return set_hip_error(h, e, "hipMalloc");
    h->bal_cap = batch;
  }
  e = copy_h2d(h, h->d_bal_recs, h_records, sizeof(double) * MPCQP_BAL_SIZE * batch);
  if (e != hipSuccess) return set_hip_error(h, e, "records H2D");
  int32_t rc = mpcqp_balance_solve_device(h, bp, h->d_bal_recs, batch, h->d_bal_res, h->hstream);
  if (rc != MPCQP_OK) return rc;
  e = copy_d2h(h, h_results, h->d_bal_res, sizeof(mpcqp_result) * batch);
  if (e != hipSuccess) return set_hip_error(h, e, "results D2H");
  return MPCQP_OK;
}

int32_t mpcqp_joint_torques_device(const double* d_tq_records, const mpcqp_result* d_grf, int32_t batch,
                                   int32_t* d_counter, double* d_joint_torques, void* stream) {
  if (batch < 0 || (batch > 0 && (!d_tq_records || !d_grf || !d_counter || !d_joint_torques)))
    return MPCQP_ERR_INVALID_ARG;
  if (batch == 0) return MPCQP_OK;
  return mpcqp::launch_torques(d_tq_records, d_grf, batch, d_counter, d_joint_torques, stream) == hipSuccess
             ? MPCQP_OK
             : MPCQP_ERR_HIP;
}

const char* mpcqp_status_str(int32_t s) {
  switch (s) {
    case MPCQP_STATUS_SOLVED: return "solved";
    case MPCQP_STATUS_SOLVED_INACCURATE: return "solved inaccurate";
    case MPCQP_STATUS_PRIMAL_INFEASIBLE_INACCURATE: return "primal infeasible inaccurate";
    case MPCQP_STATUS_DUAL_INFEASIBLE_INACCURATE: return "dual infeasible inaccurate";
    case MPCQP_STATUS_MAX_ITER_REACHED: return "maximum iterations reached";
    case MPCQP_STATUS_PRIMAL_INFEASIBLE: return "primal infeasible";
    case MPCQP_STATUS_DUAL_INFEASIBLE: return "dual infeasible";
    case MPCQP_STATUS_NON_CVX: return "problem non convex";
    case MPCQP_STATUS_NAN_INPUT: return "non-finite input";
    case MPCQP_STATUS_UNSOLVED: return "unsolved";
    default: return "unknown status";
  }
}

const char* mpcqp_error_str(int32_t err) {
  switch (err) {
    case MPCQP_OK: return "ok";
    case MPCQP_ERR_INVALID_ARG: return "invalid argument";
    case MPCQP_ERR_HIP: return "HIP runtime error";
    case MPCQP_ERR_NO_DEVICE: return "no HIP device";
    case MPCQP_ERR_ALLOC: return "device allocation failed";
    default: return "unknown error";
  }
}

const char* mpcqp_last_error(mpcqp_handle* h) { return h ? h->err : "null handle"; }

int32_t mpcqp_abi_sizes(int32_t* params_size, int32_t* result_size) {
  if (params_size) *params_size = (int32_t)sizeof(mpcqp_params);
  if (result_size) *result_size = (int32_t)sizeof(mpcqp_result);
  return MPCQP_OK;
}

int32_t mpcqp_handle_slots(mpcqp_handle* h) { return h ? h->slots : 0; }

int32_t mpcqp_handoff_counts(mpcqp_handle* h, int32_t counts[3]) {
  if (!h || !counts) return MPCQP_ERR_INVALID_ARG;
  counts[0] = counts[1] = counts[2] = 0;
  if (!h->fb) return MPCQP_OK;  // no wave solve yet
  DeviceGuard g(h->device);
  hipError_t e = g.err;
  if (e == hipSuccess) e = hipDeviceSynchronize();
  int32_t all[4 * mpcqp_handle::KMAX];
  if (e == hipSuccess) e = hipMemcpy(all, h->fb, sizeof(int32_t) * 4 * h->fb_parts, hipMemcpyDeviceToHost);
  for (int i = 0; i < h->fb_parts && e == hipSuccess; ++i)
    for (int j = 0; j < 3; ++j) counts[j] += all[4 * i + j];
  return e == hipSuccess ? MPCQP_OK : set_hip_error(h, e, "mpcqp_handoff_counts");
}

int32_t mpcqp_debug_set_split(mpcqp_handle* h, int32_t parts) {
  if (!h || parts < 0 || parts > mpcqp_handle::KMAX) return -MPCQP_ERR_INVALID_ARG;
  const int32_t old = h->split;
  h->split = parts;
  return old;
}

int32_t mpcqp_set_order_hint(mpcqp_handle* h, int32_t on) {
  if (!h || on < -1 || on > 1) return -2;
  const int32_t old = h->order_hint;
  h->order_hint = on;
  return old;
}

int32_t mpcqp_debug_launch_order(mpcqp_handle* h, int32_t* host_out, int32_t cap) {
  if (!h || cap < 0 || (cap > 0 && !host_out)) return -MPCQP_ERR_INVALID_ARG;
  const int32_t nout = h->last_batch < cap ? h->last_batch : cap;
  for (int32_t i = 0; i < nout; ++i) host_out[i] = i;
  if (!h->last_hint || !h->ord_order || nout == 0) return nout;
  DeviceGuard g(h->device);
  hipError_t e = g.err;
  if (e == hipSuccess) e = hipDeviceSynchronize();
  if (e == hipSuccess) e = hipMemcpy(host_out, h->ord_order, sizeof(int32_t) * nout, hipMemcpyDeviceToHost);
  if (e != hipSuccess) return -set_hip_error(h, e, "mpcqp_debug_launch_order");
  // a part's order holds part-local indices
  for (int i = 0; i < h->last_parts; ++i)
    for (int b = h->last_bnd[i]; b < h->last_bnd[i + 1] && b < nout; ++b)
      if (host_out[b] >= 0) host_out[b] += h->last_bnd[i];  // (-1: a place a typed solve left empty)
  return nout;
}

int32_t mpcqp_debug_split_parts(mpcqp_handle* h, int32_t batch) {
  if (!h || batch < 1) return 0;
  return effective_path(h) == 3 ? split_parts(h, batch) : 1;
}

int32_t mpcqp_reserve(mpcqp_handle* h, int32_t batch) {
  if (!h || batch < 0) return MPCQP_ERR_INVALID_ARG;
  DeviceGuard dg(h->device);
  hipError_t e = dg.err;
  if (e == hipSuccess && ((size_t)batch > h->work_cap || work_per_instance(h) > h->work_per))
    e = hipDeviceSynchronize();
  if (e == hipSuccess) e = ensure_workspace(h, batch, nullptr);
  if (e != hipSuccess) return set_hip_error(h, e, "workspace hipMalloc");
  if (effective_path(h) == 3) e = ensure_split_streams(h, split_parts(h, batch));
  if (e != hipSuccess) return set_hip_error(h, e, "split streams");
  return MPCQP_OK;
}
int32_t mpcqp_solve_threads(int32_t horizon) {
  if (horizon < 1 || horizon > MPCQP_MAX_HORIZON) return 0;
  return 64;  // one wavefront per robot
}

int32_t mpcqp_debug_set_solver(mpcqp_handle* h, int32_t path) {
  if (!h) return MPCQP_ERR_INVALID_ARG;
#ifdef MPCQP_DEBUG_PATHS
  if (path < 0 || path > 3) return MPCQP_ERR_INVALID_ARG;
  if (path == 1 && h->p.horizon > mpcqp::DENSE_MAX_HORIZON) return MPCQP_ERR_INVALID_ARG;
#else
  if (path != 0 && path != 3) return MPCQP_ERR_INVALID_ARG;  // cross-check paths: libmpcqp_debug.so
#endif
  DeviceGuard dg(h->device);
  hipError_t e = dg.err;
  if (e != hipSuccess) return set_hip_error(h, e, "hipSetDevice");
  const int old = h->path;
  h->path = path;
  int per_cu = 0;
  e = occupancy_for(h, &per_cu);
  if (e != hipSuccess) {
    h->path = old;
    return set_hip_error(h, e, "occupancy query");
  }
  h->slots = per_cu * h->cus;
  return MPCQP_OK;
}

int32_t mpcqp_debug_scale_image_doubles(int32_t horizon) {
  if (horizon < 1 || horizon > MPCQP_MAX_HORIZON) return 0;
  return mpcqp::scale_image_doubles(horizon);
}

int32_t mpcqp_debug_scale_image_device(mpcqp_handle* h, const double* d_records, int32_t batch, double* d_state,
                                       double* d_img, void* stream) {
#ifdef MPCQP_DEBUG_PATHS
  if (!h || batch < 0 || (batch > 0 && (!d_records || !d_img))) return MPCQP_ERR_INVALID_ARG;
  if (batch == 0) return MPCQP_OK;
  DeviceGuard dg(h->device);
  hipError_t e = dg.err;
  if (e != hipSuccess) return set_hip_error(h, e, "hipSetDevice");
  e = ensure_workspace(h, batch, stream);  // (the fallback list the kernel resets)
  if (e != hipSuccess) return set_hip_error(h, e, "workspace hipMalloc");
  mpcqp::LaunchArgs a;
  memset(&a, 0, sizeof(a));
  a.recs = d_records;
  a.batch = batch;
  a.work = d_img;
  a.wstate = d_state;
  a.fallback = h->fb;
  a.stream = stream;
  a.p = h->p;
  e = mpcqp::launch_scale_any(a);
  if (e != hipSuccess) return set_hip_error(h, e, "scale_kernel launch");
  return MPCQP_OK;
#else
  (void)h; (void)d_records; (void)batch; (void)d_state; (void)d_img; (void)stream;
  return MPCQP_ERR_INVALID_ARG;  // libmpcqp_debug.so only
#endif
}

int32_t mpcqp_debug_wave_selftest(double* d_out, void* stream) {
  if (!d_out) return MPCQP_ERR_INVALID_ARG;
  return mpcqp::wave_selftest(d_out, stream) == hipSuccess ? MPCQP_OK : MPCQP_ERR_HIP;
}

}  // extern "C"
