// mpcqp_internal.h — shared between the kernels and the C-ABI layer (not installed).
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/mpcqp.h"

#define MPCQP_TRACE_LEN 64  // termination-check records kept per instance by the debug trace

namespace mpcqp {


// Launch-order hint of the wave path (mpcqp_order.hip), handle-owned device state.  The arrays are
// indexed by global batch index; a part of a split solve gets them offset to its first robot, and
// its order[] holds part-local indices.  order == nullptr: robots are dispatched in input order and
// nothing of the state is read or written.
constexpr int ORDER_KEY_MAX = 63;     // cost keys are clamped to 0 .. ORDER_KEY_MAX
constexpr int ORDER_KEY_SHIFT = 3;    // key = cost >> ORDER_KEY_SHIFT
constexpr int ORDER_RHO_WEIGHT = 15;  // one rho update (refactorization) costs about 15 iterations
constexpr int ORDER_COST_MAX = 1 << 20;
constexpr int ORDER_LAYOUT_INTS = 4;  // per part: {whole batch, parts, first robot, robots}
// what a solve cost, in iterations (a robot handed from the Schur to the Riccati form: both added)
__host__ __device__ constexpr int order_cost(int iters, int rho_updates) {
  const int it = iters < 0 ? 0 : iters > ORDER_COST_MAX ? ORDER_COST_MAX : iters;
  const int ru = rho_updates < 0 ? 0 : rho_updates > ORDER_COST_MAX ? ORDER_COST_MAX : rho_updates;
  return it + ORDER_RHO_WEIGHT * ru;  // < 2^25
}
__host__ __device__ constexpr int order_key(int cost) {
  const int k = cost >> ORDER_KEY_SHIFT;
  return k < 0 ? 0 : k > ORDER_KEY_MAX ? ORDER_KEY_MAX : k;
}
struct OrderHint {
  int* order;     // [robots] written by order_kernel, read by wave_kernel: block i solves robot order[i]
  int* key;       // [robots] cost key of the robot's last solve, written by wave_kernel's epilogue
  int* contacts;  // [robots] contact mask (bit l = leg l) the robot was last solved with (order_kernel)
  int* layout;    // this part's ORDER_LAYOUT_INTS: the batch and part layout the state was written for
  int whole, parts, part, first;  // this call's layout: whole batch, parts, this part, its first robot
  bool identity;  // a typed solve with the hint off: order[] = the identity with holes, no stored state used
};

// One (part of a) solve.  recs .. wstate and hint.order/key/contacts point at the part's first robot
// and batch / grid count the part's robots; fallback and hint.layout are the part's own.
struct LaunchArgs {
  const double* recs;
  int batch;
  mpcqp_result* results;
  double* solution;
  double* work;
  double* trace;
  int trace_cap;
  double* wstate;  // warm-start slots [batch][warm_state_doubles(N)] (wave path) or nullptr
  int* fallback;   // wave path: 4 hand-off counters (handle-owned): [0] rank-deficient feet,
                   // [1] S_max * amp > SCHUR_AMP, [2] S_max > SCHUR_SMAX, [3] unused
  int grid;
  void* stream;
  mpcqp_params p;
  OrderHint hint;  // wave path: launch order (hint.order == nullptr: input order)
  // typed solve (mpcqp_solve_batch_warm_typed_device): robot b is solved iff !type || type[b] == want.
  // order_kernel gives the others' places an index outside the batch, which wave_kernel skips, and
  // scale_kernel leaves them alone; type points at the part's first robot.
  const int* type;
  int want;
};

// Formulation only (mpcqp_build.hip): ConvexMpc::calculate_qp_mats, horizons 1..20
hipError_t launch_build_any(const LaunchArgs& a, double* P, double* q, double* l, double* u);

// The solve: scale_kernel (mpcqp_scale.hip), then the one-wave-per-robot wave_kernel
// (mpcqp_wave.hip), horizons 1..WAVE_MAX_HORIZON
hipError_t launch_wave_any(const LaunchArgs& a);
hipError_t occupancy_wave_any(const mpcqp_params& p, int* blocks);
hipError_t wave_selftest(double* d_out, void* stream);
hipError_t launch_scale_any(const LaunchArgs& a);  // scale_kernel alone (the image in a.work)
// order_kernel (mpcqp_order.hip): a.hint.order for this part from the stored keys and contact masks,
// the identity when the state was written for another layout; kmax = layout slots the handle owns
hipError_t launch_order(const LaunchArgs& a, int kmax);
constexpr int WAVE_MAX_HORIZON = 20;
// the horizons both files instantiate their kernels for (static ISA tools build a single one)
#ifndef MPCQP_WAVE_FOR_EACH_N
#define MPCQP_WAVE_FOR_EACH_N(X) \
  X(1) X(2) X(3) X(4) X(5) X(6) X(7) X(8) X(9) X(10) X(11) X(12) X(13) X(14) X(15) X(16) X(17) X(18) X(19) X(20)
#endif

#ifdef MPCQP_DEBUG_PATHS
// Cross-check solvers, built only into libmpcqp_debug.so (mpcqp_debug_set_solver 1, 2):
// dense K^-1 workgroup (mpcqp_kernels.hip, N <= DENSE_MAX_HORIZON) and workgroup Riccati
// (mpcqp_riccati.hip).
hipError_t launch_solve_any(const LaunchArgs& a);
hipError_t occupancy_any(int horizon, int* blocks);
size_t workspace_doubles(int horizon);  // per robot
hipError_t launch_riccati_any(const LaunchArgs& a);
hipError_t occupancy_riccati_any(int horizon, int* blocks);
size_t riccati_workspace_doubles(int horizon);  // per robot
#endif
constexpr int DENSE_MAX_HORIZON = 10;
// doubles per robot of the warm-start slot (mpcqp_wave_common.h WarmLayout)
__host__ __device__ constexpr int warm_state_doubles(int N) {
  return 4 + 3 * 12 * N + 5 * 20 * N + ((12 * N + 63) / 64) * 12 * N;
}

// doubles per robot of the scaling image scale_kernel hands to wave_kernel (mpcqp_wave_common.h ScaleImg)
__host__ __device__ constexpr int scale_image_doubles(int N) { return 3 * 12 * N + 20 * N + 3; }

// Downstream torque map (mpcqp_torque.hip)
hipError_t launch_torques(const double* recs, const mpcqp_result* grf, int batch, int* counter, double* tau,
                          void* stream);

// Input assembly from raw robot state (mpcqp_assemble.hip)
hipError_t launch_assemble(int horizon, const double* states, int batch, double* recs, void* stream);
// Indexed copy of fixed-size slots (warm-start slots of mixed-mode batches; mpcqp_assemble.hip)
hipError_t launch_copy_slots(const double* src, const int* sidx, double* dst, const int* didx, int count, int slot,
                             void* stream);

// Upstream leg plan: gait, footholds, swing-leg PD force, contacts, terrain fit (mpcqp_legplan.hip)
hipError_t launch_leg_plan(const mpcqp_plan_params& pp, double dt, double* states, const double* plan_in, int batch,
                           double* slots, double* tq, double* out, const int* type, void* stream);
int plan_state_doubles();  // doubles per robot of the plan slot

// State front end: frames, leg kinematics, Kalman estimator (mpcqp_estimate.hip)
hipError_t launch_state_estimate(const mpcqp_est_params& pp, double dt, const double* sensors, double* plan_in,
                                 double* states, int batch, double* slots, double* tq, double* out, void* stream);
int estimator_state_doubles();  // doubles per robot of the estimator slot

// Single-step QP balance controller (mpcqp_balance.hip)
hipError_t launch_balance(const mpcqp_balance_params& bp, const mpcqp_params& p, const double* recs, int batch,
                          const int* type, int want, mpcqp_result* out, void* stream);
// Balance records from the raw robot state (mpcqp_assemble.hip)
hipError_t launch_assemble_balance(const mpcqp_balance_gains& g, const double* states, const double* plan_in,
                                   const double* cmd_state, int batch, double* recs, void* stream);

// Command stage: the joystick command block of main_update (mpcqp_command.hip)
hipError_t launch_command(const mpcqp_command_params& cp, double dt, double* cmds, double* states, double* plan_in,
                          int batch, double* slots, void* stream);

// Plant stage: rigid-body model from joint torques to the next tick's sensor rows (mpcqp_plant.hip)
hipError_t launch_plant(const mpcqp_plant_params& pp, double dt, const double* torques, int batch, double* slots,
                        const double* init, double* sensors, double* plan_in, double* states, double* tq,
                        double* out, void* stream);
// the same with the external forces of a wrench row (wrench != nullptr), another instantiation of the kernel
hipError_t launch_plant_wrench(const mpcqp_plant_params& pp, double dt, const double* torques, const double* wrench,
                               int batch, double* slots, const double* init, double* sensors, double* plan_in,
                               double* states, double* tq, double* out, void* stream);
// the same on the inclined ground of a terrain table (terrain != nullptr), two more instantiations; robot b's row
// is its episode slot's pool index, or b without an episode slot
hipError_t launch_plant_terrain(const mpcqp_plant_params& pp, double dt, const double* torques, const double* wrench,
                                const double* terrain, int terrain_rows, const double* episode_state, int batch,
                                double* slots, const double* init, double* sensors, double* plan_in, double* states,
                                double* tq, double* out, void* stream);
// the same on the bilinear height field of a header table and a heights array (field != nullptr), two more
// instantiations; the row is chosen as the terrain row is
hipError_t launch_plant_field(const mpcqp_plant_params& pp, double dt, const double* torques, const double* wrench,
                              const double* field, int field_rows, const double* heights, int heights_len,
                              const double* episode_state, int batch, double* slots, const double* init,
                              double* sensors, double* plan_in, double* states, double* tq, double* out, void* stream);

// Disturbance stage: pushes, payload weight, sensor noise and IMU biases drawn on the device (mpcqp_disturb.hip)
hipError_t launch_disturb(const mpcqp_disturb_params& dp, const mpcqp_disturb_buffers& bf, int batch, void* stream);

// Episode stage: metrics, episode ends, log and on-device restarts (mpcqp_episode.hip)
hipError_t launch_episode(const mpcqp_episode_params& ep, const mpcqp_episode_buffers& bf, int batch, double* slots,
                          void* stream);

// Policy stage: the Go1 RL controller and its servo stand (mpcqp_policy.hip).  The device-resident
// description of one policy: the parameters (read with vector loads at a lane's joint index) and, per layer,
// the input width, the output width padded to a multiple of 32, and the float offsets of its packed weights and
// biases in the weight image.
struct PolicyImage {
  mpcqp_policy_params p;
  int n_layers;  // n_hidden + 1
  int in[4], out[4], woff[4], boff[4];
};
// Fills everything of *img but the device data from p (false: inadmissible widths); the image's float count and
// the row strides of the two LDS activation buffers.
bool policy_layout(const mpcqp_policy_params& p, PolicyImage* img, size_t* n_floats, int* stride0, int* stride1);
size_t policy_lds_bytes(int stride0, int stride1);
void policy_pack(const PolicyImage& img, const float* const* h_weights, const float* const* h_biases, float* dst);
hipError_t policy_reserve_lds();  // once per device before the first launch (not capture safe)
hipError_t launch_policy(const PolicyImage* d_img, const float* d_wts, int stride0, int stride1, const double* sensors,
                         const double* states, const double* plan_in, const double* cmds, int batch, double* slots,
                         const int* type, int want, double* torques, double* outs, void* stream);

}  // namespace mpcqp
