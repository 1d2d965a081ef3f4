/*
 * mpcqp.h — C ABI of the MI355X-native batched convex-MPC QP engine.
 *
 * Drop-in boundary for the per-control-cycle ground-reaction-force (GRF) solve of
 * zerenluo123/Go1-QP-MPC-Controller.  The reference performs, per robot and per tick:
 *
 *   ConvexMpc ctor/reset                      src/a1_cpp/src/ConvexMpc.cpp:7-108
 *   calculate_A_mat_c / calculate_B_mat_c     src/a1_cpp/src/ConvexMpc.cpp:110-143
 *   state_space_discretization                src/a1_cpp/src/ConvexMpc.cpp:145-156
 *   calculate_qp_mats (A_qp, B_qp, H, g, l/u) src/a1_cpp/src/ConvexMpc.cpp:158-245
 *   OsqpEigen setup + solve (OSQP 0.6.x)      src/a1_cpp/src/A1RobotControl.cpp:522-555
 *   extraction f_i = R^T u[3i:3i+3]           src/a1_cpp/src/A1RobotControl.cpp:555-561
 *
 * Every entry point below replaces one of those interfaces for a whole *batch* of robots.
 * The header is plain C: no HIP, Eigen or torch types.  Streams are passed as opaque
 * `void*` (a hipStream_t; NULL = the default stream).
 *
 * Arithmetic is IEEE binary64 (the reference computes in double everywhere).
 *
 * Threading: a handle is bound to one device and is not thread-safe; use one handle per
 * host thread / stream.  Inputs are read once per call (snapshot semantics).
 * Errors never throw across this boundary: every function returns an mpcqp_error code.
 */
#ifndef MPCQP_H_
#define MPCQP_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- dimensions (reference: src/a1_cpp/src/A1Params.h:26-34) ------------------------ */
#define MPCQP_STATE_DIM 13      /* MPC_STATE_DIM: [rpy, p, w, v, g]                       */
#define MPCQP_NUM_LEG 4         /* NUM_LEG (FL, FR, RL, RR)                               */
#define MPCQP_NUM_DOF 12        /* NUM_DOF: 3 GRF components x 4 legs per horizon step     */
#define MPCQP_CONSTRAINT_DIM 20 /* MPC_CONSTRAINT_DIM: 5 friction-pyramid rows x 4 legs    */
#define MPCQP_MAX_HORIZON 20    /* 1..20: one wavefront per robot (Schur form N<=10, Riccati N>10) */
#define MPCQP_OSQP_INFTY 1e30   /* OsqpEigen::INFTY == OSQP_INFTY (OSQP 0.6 constants.h)  */

/* ---- per-instance problem record (all binary64, contiguous) ----------------------------
 * One record describes exactly the inputs ConvexMpc::calculate_qp_mats and the MPC branch
 * of A1RobotControl::compute_grf consume.  Offsets are in doubles.                        */
#define MPCQP_REC_X0 0        /* [13] mpc_states x0 (A1RobotControl.cpp:452-456)                 */
#define MPCQP_REC_EULER 13    /* [3]  euler given to calculate_A_mat_c (only yaw is used, :116)  */
#define MPCQP_REC_ROT 16      /* [9]  root_rot_mat, row-major (calculate_B_mat_c arg)            */
#define MPCQP_REC_INERTIA 25  /* [9]  trunk inertia, body frame, row-major                       */
#define MPCQP_REC_MASS 34     /* robot_mass                                                       */
#define MPCQP_REC_MU 35       /* friction coefficient (ConvexMpc.cpp:8 hard-codes 0.3)            */
#define MPCQP_REC_FZMIN 36    /* fz_min (ConvexMpc.cpp:223: 0)                                    */
#define MPCQP_REC_FZMAX 37    /* fz_max (ConvexMpc.cpp:224: 180)                                  */
#define MPCQP_REC_DT 38       /* mpc_dt used by state_space_discretization (A1RobotControl:462)  */
#define MPCQP_REC_CONTACTS 39 /* [4]  contacts[i] as 0.0 / 1.0 (bounds, ConvexMpc.cpp:225-241)    */
#define MPCQP_REC_XREF 44     /* [13N] mpc_states_d                                               */
/* feet: [N][4][3] foot_pos used for B_c at horizon step i (foot_pos_abs in compute_grf, the
 * per-step shifted foot_pos_abs_mpc in test_mpc.cpp:105-115), at MPCQP_REC_XREF + 13N           */
#define MPCQP_REC_FEET(N) (MPCQP_REC_XREF + 13 * (N))
#define MPCQP_REC_SIZE(N) (MPCQP_REC_XREF + 25 * (N) + ((N)&1))

/* ---- solver settings: OSQP 0.6 defaults + the reference's overrides -------------------
 * (A1RobotControl.cpp:522-538 sets only verbosity=false and warm_start; everything else
 * is osqp_set_default_settings).  adaptive_rho_interval: OSQP's 0 means "derive from
 * wall-clock" (non-reproducible); the engine requires a fixed interval (default 25).      */
typedef struct mpcqp_params {
  int32_t horizon;                /* N, 1..MPCQP_MAX_HORIZON (PLAN_HORIZON = 10)            */
  int32_t max_iter;               /* 4000                                                   */
  int32_t scaling;                /* 10 Ruiz passes                                          */
  int32_t check_termination;      /* 25                                                      */
  int32_t adaptive_rho;           /* 1                                                       */
  int32_t adaptive_rho_interval;  /* 25 (fixed; see above)                                   */
  int32_t scaled_termination;     /* 0                                                       */
  int32_t warm_start;             /* 0: cold start every solve (test_mpc.cpp:133)            */
  double q_weights[MPCQP_STATE_DIM]; /* ConvexMpc ctor arg; Q = diag(2 q) tiled (:16-23)    */
  double r_weights[MPCQP_NUM_DOF];   /* ConvexMpc ctor arg; R = diag(2 r) tiled (:37-44)    */
  double rho;                     /* 0.1                                                     */
  double sigma;                   /* 1e-6                                                    */
  double alpha;                   /* 1.6                                                     */
  double eps_abs, eps_rel;        /* 1e-3, 1e-3                                              */
  double eps_prim_inf, eps_dual_inf; /* 1e-4, 1e-4                                           */
  double adaptive_rho_tolerance;  /* 5                                                       */
} mpcqp_params;

/* ---- per-instance result --------------------------------------------------------------- */
typedef struct mpcqp_result {
  double u0[MPCQP_NUM_DOF];     /* solution.segment(0,12): world-frame GRF of horizon step 0 */
  double f_body[MPCQP_NUM_DOF]; /* compute_grf output: R^T u0[3i:3i+3] per leg (leg-major);
                                   legs whose norm is NaN are left 0 and flagged in nan_legs  */
  double obj_val;               /* unscaled objective 1/2 x'Px + q'x (OSQP info->obj_val)     */
  double pri_res, dua_res;      /* unscaled residuals at the last termination check          */
  double rho;                   /* final rho                                                  */
  int32_t status;               /* MPCQP_STATUS_* (numerically equal to OSQP 0.6 status_val)  */
  int32_t iters;                /* OSQP info->iter                                            */
  int32_t rho_updates;          /* OSQP info->rho_updates                                     */
  int32_t nan_legs;             /* bit i set: leg i solution had a NaN norm                   */
} mpcqp_result;

/* OSQP 0.6 status values (constants.h) */
enum {
  MPCQP_STATUS_SOLVED = 1,
  MPCQP_STATUS_SOLVED_INACCURATE = 2,
  MPCQP_STATUS_PRIMAL_INFEASIBLE_INACCURATE = 3,
  MPCQP_STATUS_DUAL_INFEASIBLE_INACCURATE = 4,
  MPCQP_STATUS_MAX_ITER_REACHED = -2,
  MPCQP_STATUS_PRIMAL_INFEASIBLE = -3,
  MPCQP_STATUS_DUAL_INFEASIBLE = -4,
  MPCQP_STATUS_NON_CVX = -7,
  MPCQP_STATUS_NAN_INPUT = -100, /* engine-specific: a NaN/inf in the instance's record      */
  MPCQP_STATUS_UNSOLVED = -10
};

/* call-level error codes */
enum {
  MPCQP_OK = 0,
  MPCQP_ERR_INVALID_ARG = 1,
  MPCQP_ERR_HIP = 2,
  MPCQP_ERR_NO_DEVICE = 3,
  MPCQP_ERR_ALLOC = 4
};

typedef struct mpcqp_handle mpcqp_handle;

/* Fill *p with the reference's settings for horizon N (OSQP 0.6 defaults, Go1 weights from
 * src/go1_rl_ctrl_cpp/src/Go1CtrlStates.hpp:203-249, fixed adaptive-rho interval 25). */
void mpcqp_default_params(mpcqp_params* p, int32_t horizon);

/* Number of doubles in one problem record for horizon N. */
int32_t mpcqp_record_size(int32_t horizon);

/* Replaces the ConvexMpc ctor + OsqpEigen::Solver construction (ConvexMpc.cpp:7-68,
 * A1RobotControl.h:67): uploads weights/settings to `device`. */
int32_t mpcqp_create(const mpcqp_params* params, int32_t device, mpcqp_handle** out);
int32_t mpcqp_destroy(mpcqp_handle* h);

/* Pre-size the handle's device workspace — the scaling image scale_kernel hands to wave_kernel,
 * 56N + 3 binary64 per robot (3.5 KB at N = 10) — and create the internal streams a solve of `batch`
 * robots splits over, so that later mpcqp_solve_batch_device calls with batch <= `batch` neither
 * allocate nor create streams (hipGraph-capture safe). */
int32_t mpcqp_reserve(mpcqp_handle* h, int32_t batch);

/* Replaces calculate_A/B_mat_c + discretization + calculate_qp_mats + OSQP initSolver/solve
 * + extraction (A1RobotControl.cpp:446-561) for `batch` robots.  All pointers are DEVICE
 * pointers; asynchronous on `stream`.
 *   d_records  [batch][mpcqp_record_size(N)]
 *   d_results  [batch] mpcqp_result
 *   d_solution [batch][12N] full unscaled primal solution, or NULL                       */
int32_t mpcqp_solve_batch_device(mpcqp_handle* h, const double* d_records, int32_t batch,
                                 mpcqp_result* d_results, double* d_solution, void* stream);

/* Warm start across control ticks: the reference keeps one OsqpEigen::Solver per controller
 * (A1RobotControl.h:67) with setWarmStart(true) (A1RobotControl.cpp:524); its first tick runs
 * initSolver, later ticks updateHessianMatrix / updateGradient / updateLowerBound /
 * updateUpperBound and solve from the previous x, z, y and adapted rho (:522-540).  The engine
 * keeps that solver state per robot in a caller-owned DEVICE buffer
 *   d_state [batch][mpcqp_warm_state_size(N)] binary64, zero-filled = "not initialized yet",
 * so a robot's slot must follow it from tick to tick (same batch index).  Robots whose record
 * is non-finite leave their slot untouched.  Default (wave) solver path only. */
int32_t mpcqp_warm_state_size(int32_t horizon);
int32_t mpcqp_solve_batch_warm_device(mpcqp_handle* h, const double* d_records, int32_t batch, double* d_state,
                                      mpcqp_result* d_results, double* d_solution, void* stream);

/* Launch-order hint.  One wavefront solves one robot and robots differ several-fold in iterations,
 * so the order in which a batch's robots are dispatched decides how long the last ones leave the
 * device partly idle.  The handle remembers, per batch index, what the robot cost in the handle's
 * previous solve and the contact set it was solved with; the next solve of the same batch size
 * dispatches robots whose contact set changed first, then the costliest first.  Results do not
 * depend on it by a bit.  The only contract is the warm slots' one: batch index b is the same robot
 * as in the previous call on this handle; a caller that shuffles its robots loses the gain, nothing
 * else.  The state lives on the device and is read when the solve runs, so replays of a solve
 * captured into a hipGraph follow it too.
 *   on: 1 both solves, 0 neither, -1 the built-in default of each (cold and warm-started solves
 * have their own).  The environment variable MPCQP_ORDER_HINT sets the
 * initial value at mpcqp_create.  Returns the previous setting, or -2 for a bad argument. */
int32_t mpcqp_set_order_hint(mpcqp_handle* h, int32_t on);

/* The warm-started solve for the robots of one control type (a fleet in which each robot takes the
 * stance_leg_control_type branch of its own, A1RobotControl.cpp:377 / :446): robot b is solved iff
 * d_type == NULL || d_type[b] == type.  d_type is a DEVICE int32 [batch], read when the kernels run, so
 * a captured graph follows changes made between replays.  Of a robot that is not selected nothing is
 * written: not its mpcqp_result row, its d_solution row or its warm slot (the reference does not touch
 * its member solver on QP ticks, :377-444), not the handle's launch-order state for it, and the hand-off
 * counters do not count it.  A selected robot's outputs are bitwise those of
 * mpcqp_solve_batch_warm_device on the same batch. */
int32_t mpcqp_solve_batch_warm_typed_device(mpcqp_handle* h, const double* d_records, int32_t batch, double* d_state,
                                            const int32_t* d_type, int32_t type, mpcqp_result* d_results,
                                            double* d_solution, void* stream);

/* Indexed copy of warm-start slots between DEVICE buffers, for callers whose solved robots are a
 * subset of their slots (a mixed-mode batch: the MPC robots' slots gathered into a compact buffer
 * for the warm solve and scattered back after it, as the reference's controller keeps its member
 * solver untouched on QP ticks, A1RobotControl.cpp:377-444).  For i < count:
 *   slot d_dst[d_dst_idx ? d_dst_idx[i] : i] = slot d_src[d_src_idx ? d_src_idx[i] : i],
 * slots of mpcqp_warm_state_size(horizon) doubles, index arrays DEVICE int32 (NULL = identity).
 * Destination slots must be distinct.  Async on `stream`. */
int32_t mpcqp_copy_warm_slots_device(int32_t horizon, const double* d_src, const int32_t* d_src_idx, double* d_dst,
                                     const int32_t* d_dst_idx, int32_t count, void* stream);

/* Host-pointer convenience wrapper (copies in, solves, copies out, synchronizes) on a stream of the
 * handle's own.  That stream is a blocking stream: it waits for work queued before the call on the
 * legacy NULL stream (zeroing warm slots with hipMemset(..) / on torch's default stream is ordered
 * before the solve), but NOT for work on other non-blocking streams — synchronize those first.  One
 * handle must not run a device-pointer solve on another stream concurrently with a host-wrapper
 * call (they share the handle's workspace).  Pinned host buffers (hipHostMalloc / registered) move by one DMA each way;
 * pageable ones through two pinned 2-MiB staging chunks of the handle, host copies overlapping the
 * DMA.  Not for concurrent use of one handle from several threads. */
int32_t mpcqp_solve_batch_host(mpcqp_handle* h, const double* h_records, int32_t batch,
                               mpcqp_result* h_results, double* h_solution);

/* Host-pointer variant of the warm-started solve: records and results on the host (as in
 * mpcqp_solve_batch_host), the solver slots d_state in DEVICE memory (as in
 * mpcqp_solve_batch_warm_device).  This is the per-tick call of a persistent controller-owned
 * solver (A1RobotControl.h:67 member OsqpEigen::Solver, warm start on: A1RobotControl.cpp:522-540);
 * synchronous. */
int32_t mpcqp_solve_batch_warm_host(mpcqp_handle* h, const double* h_records, int32_t batch, double* d_state,
                                    mpcqp_result* h_results, double* h_solution);

/* Formulation only (ConvexMpc::calculate_qp_mats): dense Hessian (full symmetric, row-major
 * [12N][12N]), gradient [12N], bounds l/u [20N] per instance.  DEVICE pointers. */
int32_t mpcqp_build_qp_device(mpcqp_handle* h, const double* d_records, int32_t batch,
                              double* d_P, double* d_q, double* d_l, double* d_u, void* stream);

/* ---- on-device input assembly from raw robot state --------------------
 * One binary64 record per robot holding the A1CtrlStates / Go1CtrlStates fields the MPC branch of
 * compute_grf reads (A1RobotControl.cpp:446-514); matrices row-major, vectors world frame unless
 * noted.  Offsets in doubles.                                                                  */
#define MPCQP_ST_EULER 0      /* [3] root_euler                                                  */
#define MPCQP_ST_POS 3        /* [3] root_pos                                                    */
#define MPCQP_ST_ANG_VEL 6    /* [3] root_ang_vel (world)                                        */
#define MPCQP_ST_LIN_VEL 9    /* [3] root_lin_vel (world)                                        */
#define MPCQP_ST_ROT 12       /* [9] root_rot_mat                                                */
#define MPCQP_ST_EULER_D 21   /* [3] root_euler_d (after terrain adaptation, :335-376)           */
#define MPCQP_ST_POS_D 24     /* [3] root_pos_d                                                  */
#define MPCQP_ST_ANG_VEL_D 27 /* [3] root_ang_vel_d                                              */
#define MPCQP_ST_LIN_VEL_D 30 /* [3] root_lin_vel_d (body frame; :470 rotates it to world)       */
#define MPCQP_ST_FEET 33      /* [4][3] foot_pos_abs column i                                     */
#define MPCQP_ST_MASS 45      /* robot_mass                                                      */
#define MPCQP_ST_INERTIA 46   /* [9] trunk_inertia                                               */
#define MPCQP_ST_MU 55        /* friction coefficient (ConvexMpc.cpp:8: 0.3)                      */
#define MPCQP_ST_FZMIN 56     /* 0                                                               */
#define MPCQP_ST_FZMAX 57     /* 180                                                             */
#define MPCQP_ST_DT 58        /* mpc_dt (:462, 0.0025)                                           */
#define MPCQP_ST_CONTACTS 59  /* [4] contacts[i] as 0.0 / 1.0                                    */
#define MPCQP_ST_SIZE 64      /* 63 used, padded to a multiple of 4 doubles                      */

/* Replaces the host-side x0 / x_ref / horizon-feet assembly of compute_grf (A1RobotControl.cpp:
 * 452-514: mpc_states, root_lin_vel_d_world, mpc_states_d, B_mat_d_list feet) for `batch` robots:
 * d_states [batch][MPCQP_ST_SIZE] -> d_records [batch][mpcqp_record_size(horizon)], DEVICE
 * pointers, async on `stream`.  Chain it before mpcqp_solve_batch_device on the same stream. */
int32_t mpcqp_assemble_records_device(int32_t horizon, const double* d_states, int32_t batch, double* d_records,
                                      void* stream);

/* ---- downstream torque map: A1RobotControl::compute_joint_torques (A1RobotControl.cpp:289-319)
 * One binary64 record per robot (offsets in doubles); FL, FR, RL, RR leg order.             */
#define MPCQP_TQ_JFOOT 0      /* [4][9] j_foot.block<3,3>(3i,3i), row-major (A1CtrlStates.h:410) */
#define MPCQP_TQ_FKIN 36      /* [4][3] foot_forces_kin column i (swing-leg PD force, :220-286)  */
#define MPCQP_TQ_KM 48        /* [3]    km_foot                                                    */
#define MPCQP_TQ_GRAV 51      /* [12]   torques_gravity                                            */
#define MPCQP_TQ_CONTACTS 63  /* [4]    contacts[i] as 0.0 / 1.0                                   */
#define MPCQP_TQ_SIZE 68      /* 67 used, padded to a multiple of 4 doubles                       */

/* Replaces compute_joint_torques for `batch` robots (DEVICE pointers, async on `stream`):
 *   d_counter[b] += 1 (mpc_init_counter); while it is < 10 the robot's torques are zeroed;
 *   otherwise stance legs get tau = J^T (-f_grf), swing legs J tau = km .* f_kin (Eigen
 *   PartialPivLU), plus torques_gravity, and non-NaN entries overwrite d_joint_torques[b][12].
 * f_grf is taken from d_grf[b].f_body — the solve's output, so the MPC result never leaves the
 * device (a NaN leg's f_body is 0 there; the reference leaves that column uninitialised). */
int32_t mpcqp_joint_torques_device(const double* d_tq_records, const mpcqp_result* d_grf, int32_t batch,
                                   int32_t* d_counter, double* d_joint_torques, void* stream);

/* ---- upstream leg plan: A1RobotControl::update_plan (A1RobotControl.cpp:148-202), then
 * generate_swing_legs_ctrl (:204-287), then the terrain adaptation of compute_grf (:335-376 with
 * compute_walking_surface, :566-582), in that order, per robot and per tick.  The stage produces the
 * fields the rest of the tick consumes — MPCQP_ST_CONTACTS, MPCQP_ST_EULER_D[1], MPCQP_TQ_FKIN,
 * MPCQP_TQ_CONTACTS — and keeps the controller's persistent state (gait counters, swing start points,
 * the 13 moving-window filters) in a caller-owned device slot per robot.                          */
#define MPCQP_PLAN_CONTACT_WINDOW 60   /* recent_contact_{x,y,z}_filter (A1RobotControl.cpp:54-56) */
#define MPCQP_PLAN_TERRAIN_WINDOW 100  /* terrain_angle_filter (A1RobotControl.cpp:52)             */

typedef struct mpcqp_plan_params {
  double default_foot_pos[12];  /* [leg][xyz] (A1CtrlStates.h:45-47: x +-0.17, y +-0.15, z -0.35)      */
  double kp_foot[12];           /* [leg][xyz] 300, 400, 400 (A1CtrlStates.h:105-116)                  */
  double kd_foot[12];           /* [leg][xyz] 8, 8, 8 (A1CtrlStates.h:109-120)                        */
  double gait_counter_speed[4]; /* 2, 2, 2, 2 (A1CtrlStates.h:103)                                    */
  double gait_counter_init[4];  /* gait_counter_reset(): 0, 120, 120, 0 (A1CtrlStates.h:323-327)      */
  double counter_per_gait;      /* 240 (A1CtrlStates.h:24)                                            */
  double counter_per_swing;     /* 120 (A1CtrlStates.h:25)                                            */
  double control_dt;            /* MAIN_UPDATE_FREQUENCY / 1000 = 0.0005 (A1CtrlStates.h:333)         */
  double foot_force_low;        /* FOOT_FORCE_LOW 30 (A1Params.h:38)                                  */
  double foot_delta_x_limit;    /* FOOT_DELTA_X_LIMIT 0.1 (A1Params.h:44)                             */
  double foot_delta_y_limit;    /* FOOT_DELTA_Y_LIMIT 0.1 (A1Params.h:45)                             */
  double swing_clearance1;      /* (double)0.0f, FOOT_SWING_CLEARANCE1 (A1Params.h:41)                */
  double swing_clearance2;      /* (double)0.4f = 0.4000000059604645, FOOT_SWING_CLEARANCE2 (:42)     */
  int32_t terrain;              /* stance_leg_control_type == 1 (A1CtrlStates.h:21): fit the terrain  */
  int32_t use_terrain_adapt;    /* 1 (A1CtrlStates.h:22): write root_euler_d[1]                       */
} mpcqp_plan_params;

/* Fill *p with A1CtrlStates::reset() (A1CtrlStates.h:20-122) and the A1Params.h:38-45 constants. */
void mpcqp_plan_default_params(mpcqp_plan_params* p);

/* Per-tick plan input row: the fields of the controller state the MPCQP_ST_* row lacks.           */
#define MPCQP_PL_ROT_Z 0          /* [9] root_rot_mat_z (yaw-only rotation), row-major               */
#define MPCQP_PL_FOOT_FORCE 9     /* [4] foot_force (contact sensor, :265)                            */
#define MPCQP_PL_MOVEMENT_MODE 13 /* movement_mode as 0.0 (standstill) / 1.0 (walk) (:150)            */
#define MPCQP_PL_SIZE 16          /* 14 used, padded to a multiple of 4 doubles                       */

/* Optional per-robot output row ([leg][xyz] where 12 wide, flags as 0.0 / 1.0).                   */
#define MPCQP_PO_TARGET_REL 0     /* [4][3] foot_pos_target_rel (:172-197)                            */
#define MPCQP_PO_TARGET_ABS 12    /* [4][3] foot_pos_target_abs (:199)                                */
#define MPCQP_PO_TARGET_WORLD 24  /* [4][3] foot_pos_target_world (:200)                              */
#define MPCQP_PO_FOOT_CUR 36      /* [4][3] foot_pos_cur (:224)                                       */
#define MPCQP_PO_BEZIER 48        /* [4][3] foot_pos_target, the Bezier point (:238)                  */
#define MPCQP_PO_FKIN 60          /* [4][3] foot_forces_kin (:251)                                    */
#define MPCQP_PO_RECENT 72        /* [4][3] foot_pos_recent_contact (:277-280)                        */
#define MPCQP_PO_GAIT 84          /* [4] gait_counter                                                 */
#define MPCQP_PO_PLAN 88          /* [4] plan_contacts                                                */
#define MPCQP_PO_EARLY 92         /* [4] early_contacts                                               */
#define MPCQP_PO_CONTACTS 96      /* [4] contacts                                                     */
#define MPCQP_PO_PLANE 100        /* [3] a of compute_walking_surface (:578); 0 with terrain off      */
#define MPCQP_PO_COS 103          /* angle_cos of cal_dihedral_angle, unfiltered (Utils.cpp:57-60)    */
#define MPCQP_PO_ANGLE 104        /* terrain_pitch_angle (:375): filtered and clamped                 */
#define MPCQP_PO_SIZE 108         /* 105 used, padded to a multiple of 4 doubles                      */

/* Doubles per robot of the plan slot, a caller-owned DEVICE buffer d_plan_state [batch][size] that
 * must follow its robot from tick to tick.  Zero-filled = a freshly reset() controller (the first
 * tick loads gait_counter from gait_counter_init), the convention of the warm-start slots. */
int32_t mpcqp_plan_state_size(void);

/* One plan tick for `batch` robots (DEVICE pointers, async on `stream`, no allocation and no
 * synchronization: hipGraph-capture safe).  Chain it before mpcqp_assemble_records_device on the
 * same stream.  `dt` is the argument of update_plan / generate_swing_legs_ctrl (the foot velocities
 * divide by it).  Reads d_states [batch][MPCQP_ST_SIZE] and d_plan_in [batch][MPCQP_PL_SIZE];
 * writes, in place, MPCQP_ST_CONTACTS and (terrain and use_terrain_adapt set) MPCQP_ST_EULER_D + 1
 * of d_states, MPCQP_TQ_FKIN and MPCQP_TQ_CONTACTS of d_tq_records [batch][MPCQP_TQ_SIZE] (NULL:
 * skipped), the slot, and d_plan_out [batch][MPCQP_PO_SIZE] (NULL: skipped).  The reference runs
 * compute_grf on a thread of its own at the same 0.5 ms period; here it is the same tick. */
int32_t mpcqp_leg_plan_device(const mpcqp_plan_params* pp, double dt, double* d_states, const double* d_plan_in,
                              int32_t batch, double* d_plan_state, double* d_tq_records, double* d_plan_out,
                              void* stream);

/* The same with the terrain adaptation per robot: the reference adapts the terrain only under
 * stance_leg_control_type == 1 (A1RobotControl.cpp:335).  d_type is a DEVICE int32 [batch] read when
 * the kernel runs; robot b runs the terrain block iff pp->terrain && d_type[b] == 1.  A robot that
 * skips it neither advances its terrain filter nor writes MPCQP_ST_EULER_D + 1, as with terrain = 0.
 * d_type == NULL is mpcqp_leg_plan_device. */
int32_t mpcqp_leg_plan_typed_device(const mpcqp_plan_params* pp, double dt, double* d_states,
                                    const double* d_plan_in, int32_t batch, double* d_plan_state,
                                    double* d_tq_records, double* d_plan_out, const int32_t* d_type, void* stream);

/* ---- command stage: the joystick command block at the top of main_update
 * (src/a1_cpp/src/GazeboA1ROS.cpp:122-188; the same block is HardwareA1ROS.cpp:104-158): body height
 * with its clamp, the walk / stand toggle, root_lin_vel_d / root_ang_vel_d, the root_euler_d integration,
 * root_pos_d, movement_mode and the position lock of kp_linear.  It runs FIRST in the tick, as in the
 * reference: the estimator sees this tick's movement_mode, and the position lock reads the previous
 * tick's root_pos (the reference runs the estimator after this block, GazeboA1ROS.cpp:190-198).      */
typedef struct mpcqp_command_params {
  double body_height_init;   /* joy_cmd_body_height = 0.2 (GazeboA1ROS.h:133)                         */
  double body_height_max;    /* JOY_CMD_BODY_HEIGHT_MAX 0.32 (A1Params.h:16)                          */
  double body_height_min;    /* JOY_CMD_BODY_HEIGHT_MIN 0.1 (A1Params.h:17)                           */
  double vel_lock_threshold; /* 0.05 (GazeboA1ROS.cpp:180)                                            */
  double kp_linear[3];       /* 100, 100, 300 (Go1CtrlStates.hpp:279-281)                             */
  double kp_linear_lock_x;   /* 100 (Go1CtrlStates.hpp:304)                                           */
  double kp_linear_lock_y;   /* 100 (Go1CtrlStates.hpp:305)                                           */
} mpcqp_command_params;

void mpcqp_command_default_params(mpcqp_command_params* p);

/* Command row, one per robot, written by the caller (offsets in doubles).  The values are the joy_cmd_*
 * members, already scaled by the JOY_CMD_*_MAX constants as joy_callback does at sensor rate
 * (GazeboA1ROS.cpp:390-416); that scaling stays with the caller, like the IMU moving averages.      */
#define MPCQP_CM_VEL 0           /* [3] joy_cmd_velx, joy_cmd_vely, joy_cmd_velz                      */
#define MPCQP_CM_RATE 3          /* [3] joy_cmd_roll_rate, joy_cmd_pitch_rate, joy_cmd_yaw_rate       */
#define MPCQP_CM_MODE_REQUEST 6  /* joy_cmd_ctrl_state_change_request as 0.0 / 1.0; the stage writes
                                    0.0 back after consuming it (:146), so one press toggles once     */
#define MPCQP_CM_SIZE 8          /* 7 used, padded to a multiple of 4 doubles                         */

/* Command slot, a caller-owned DEVICE buffer d_cmd_state [batch][mpcqp_command_state_size()] that must
 * follow its robot from tick to tick.  Zero-filled = fresh: the first tick loads body_height_init,
 * control state 0 and kp_linear from the parameters.  The offsets are public because
 * mpcqp_assemble_balance_device reads MPCQP_CS_KP_LINEAR.                                           */
#define MPCQP_CS_INIT 0             /* 0.0: fresh                                                     */
#define MPCQP_CS_BODY_HEIGHT 1      /* joy_cmd_body_height                                            */
#define MPCQP_CS_CTRL_STATE 2       /* joy_cmd_ctrl_state as 0.0 (stand) / 1.0 (walk)                 */
#define MPCQP_CS_PREV_CTRL_STATE 3  /* prev_joy_cmd_ctrl_state                                        */
#define MPCQP_CS_KP_LINEAR 4        /* [3] a1_ctrl_states.kp_linear                                   */
#define MPCQP_CS_SIZE 8             /* 7 used, padded to a multiple of 4 doubles                      */
int32_t mpcqp_command_state_size(void);

/* One command tick for `batch` robots (DEVICE pointers, async on `stream`, no allocation and no
 * synchronization: hipGraph-capture safe).  Chain it before mpcqp_state_estimate_device on the same
 * stream.  In the reference's statement order (GazeboA1ROS.cpp:124-188): height += velz * dt and the two
 * clamps; prev = state and the toggle; MPCQP_ST_LIN_VEL_D and MPCQP_ST_ANG_VEL_D from the row;
 * MPCQP_ST_EULER_D += rate * dt IN PLACE (root_euler_d lives in the caller's row from tick to tick, so
 * the plan stage's terrain write of MPCQP_ST_EULER_D + 1 is what the next tick integrates from, as in
 * the reference); MPCQP_ST_POS_D + 2 = height; movement_mode into MPCQP_PL_MOVEMENT_MODE of d_plan_in;
 * the leave-walking lock (:167-173) and the walking-mode lock (:179-188), which refresh
 * MPCQP_ST_POS_D[0:2] from MPCQP_ST_POS and switch kp_linear[0:2] of the slot; 0.0 into
 * MPCQP_CM_MODE_REQUEST of d_cmd.  Nothing else is written.  Multiplies and adds are not contracted.
 * A robot whose command row (its 7 used doubles) is non-finite keeps its slot, its command row, its
 * movement_mode, MPCQP_ST_EULER_D, _POS_D and _ANG_VEL_D, and gets NaN in MPCQP_ST_LIN_VEL_D only, a
 * field rewritten every tick: that tick's solve reports MPCQP_STATUS_NAN_INPUT for it alone and the
 * next finite row recovers. */
int32_t mpcqp_command_device(const mpcqp_command_params* cp, double dt, double* d_cmd, double* d_states,
                             double* d_plan_in, int32_t batch, double* d_cmd_state, void* stream);

/* ---- state front end: what the reference computes between the sensor callbacks and the plan,
 *   pose callback   src/a1_cpp/src/GazeboA1ROS.cpp:242-289 (root_rot_mat, root_euler, root_rot_mat_z:
 *                   :265-269 with Utils::quat_to_euler, utils/Utils.cpp:7-33; leg forward kinematics,
 *                   Jacobian, foot positions and velocities: :272-285, legKinematics/A1Kinematics.cpp:39-130)
 *   IMU callback    GazeboA1ROS.cpp:291-307 (root_ang_vel = root_rot_mat * imu_ang_vel, :306)
 *   A1BasicEKF      init_state / update_estimation, src/a1_cpp/src/A1BasicEKF.cpp:55-164 (18 states,
 *                   28 measurements; root_pos and root_lin_vel are its outputs, :162-163)
 * per robot and per tick, in that order.  The stage runs FIRST in the tick, so the plan and the solve of
 * a tick see that tick's estimate (the reference runs the estimator after the plan inside main_update,
 * GazeboA1ROS.cpp:190-198, while compute_grf reads whatever is latest from its own thread).
 *
 * Sensor row, one per robot (offsets in doubles).  The IMU callback's five-sample moving averages
 * (GazeboA1ROS.cpp:296-305) run at sensor rate outside the tick: the row holds the filtered values.
 * foot_force and movement_mode are read from the MPCQP_PL_* row.                                  */
#define MPCQP_SN_QUAT 0          /* [4] root_quat as w, x, y, z (GazeboA1ROS.cpp:244-247)             */
#define MPCQP_SN_JOINT_POS 4     /* [12] joint_pos, FL FR RL RR x (hip, thigh, calf) (:310-318)       */
#define MPCQP_SN_JOINT_VEL 16    /* [12] joint_vel                                                    */
#define MPCQP_SN_IMU_ACC 28      /* [3] imu_acc, body frame (:296-300)                                */
#define MPCQP_SN_IMU_ANG_VEL 31  /* [3] imu_ang_vel, body frame (:301-305)                            */
#define MPCQP_SN_SIZE 36         /* 34 used, padded to a multiple of 4 doubles                        */

typedef struct mpcqp_est_params {
  double rho_fix[4][5];  /* per leg: hip offset x, y, motor offset, upper, lower link (GazeboA1ROS.cpp:76-93) */
  double rho_opt[4][3];  /* per leg: calibration offsets, 0 (GazeboA1ROS.cpp:94-95)                       */
  double process_noise_pimu;         /* PROCESS_NOISE_PIMU 0.01 (A1BasicEKF.h:16)                        */
  double process_noise_vimu;         /* PROCESS_NOISE_VIMU 0.01 (A1BasicEKF.h:17)                        */
  double process_noise_pfoot;        /* PROCESS_NOISE_PFOOT 0.01 (A1BasicEKF.h:18)                       */
  double sensor_noise_pimu_rel_foot; /* SENSOR_NOISE_PIMU_REL_FOOT 0.001 (A1BasicEKF.h:19)               */
  double sensor_noise_vimu_rel_foot; /* SENSOR_NOISE_VIMU_REL_FOOT 0.1 (A1BasicEKF.h:20)                 */
  double sensor_noise_zfoot;         /* SENSOR_NOISE_ZFOOT 0.001 (A1BasicEKF.h:21)                       */
  double height_noise_no_flat;       /* 1e5: R of the height rows without flat ground (A1BasicEKF.cpp:51) */
  double init_height;                /* 0.09 (A1BasicEKF.cpp:63)                                         */
  double init_cov;                   /* 3 (A1BasicEKF.cpp:59)                                            */
  double gravity;                    /* 9.81 (A1BasicEKF.cpp:76)                                         */
  double contact_force_scale;        /* 100 (A1BasicEKF.cpp:83)                                          */
  double drift_threshold;            /* 1e-6 (A1BasicEKF.cpp:143)                                        */
  double drift_divisor;              /* 10 (A1BasicEKF.cpp:146)                                          */
  int32_t assume_flat_ground;        /* 1 (A1BasicEKF.cpp:40)                                            */
  int32_t pad_;
} mpcqp_est_params;

/* Fill *p from GazeboA1ROS.cpp:72-98 (A1 leg geometry) and A1BasicEKF.h:16-21 / A1BasicEKF.cpp:40-63. */
void mpcqp_est_default_params(mpcqp_est_params* p);
int32_t mpcqp_est_params_size(void); /* sizeof(mpcqp_est_params), for bindings                          */

/* Optional per-robot output row ([leg][xyz] where 12 wide).                                          */
#define MPCQP_EO_FOOT_POS_REL 0   /* [4][3] foot_pos_rel (GazeboA1ROS.cpp:273)                         */
#define MPCQP_EO_FOOT_VEL_REL 12  /* [4][3] foot_vel_rel (:281)                                        */
#define MPCQP_EO_FOOT_VEL_ABS 24  /* [4][3] foot_vel_abs (:284)                                        */
#define MPCQP_EO_CONTACT_W 36     /* [4] estimated_contacts, continuous (A1BasicEKF.cpp:79-86); the
                                     thresholded flags (:151-157) are CONTACT_W >= 0.5; 0 on the first tick */
#define MPCQP_EO_X 40             /* [18] x after the tick                                             */
#define MPCQP_EO_DIAG_P 58        /* [18] diagonal of P after the tick                                 */
#define MPCQP_EO_DET 76           /* det P[0:2,0:2] as tested before the reset (:143); 0 on the first tick */
#define MPCQP_EO_SIZE 80          /* 77 used, padded to a multiple of 4 doubles                        */

/* Doubles per robot of the estimator slot, a caller-owned DEVICE buffer d_est_state [batch][size] that
 * must follow its robot from tick to tick: the init flag, x and P of A1BasicEKF (A1BasicEKF.h:33-38).
 * Zero-filled = is_inited() == false, the convention of the warm-start and plan slots. */
int32_t mpcqp_estimator_state_size(void);

/* One front-end tick for `batch` robots (DEVICE pointers, async on `stream`, no allocation and no
 * synchronization: hipGraph-capture safe).  Chain it before mpcqp_leg_plan_device on the same stream.
 * `dt` is update_estimation's argument.  Reads d_sensors [batch][MPCQP_SN_SIZE] and MPCQP_PL_FOOT_FORCE /
 * MPCQP_PL_MOVEMENT_MODE of d_plan_in [batch][MPCQP_PL_SIZE]; writes, in place, MPCQP_ST_EULER, _POS,
 * _ANG_VEL, _LIN_VEL, _ROT and _FEET of d_states [batch][MPCQP_ST_SIZE], MPCQP_PL_ROT_Z of d_plan_in,
 * MPCQP_TQ_JFOOT of d_tq_records [batch][MPCQP_TQ_SIZE] (NULL: skipped), the slot, and d_est_out
 * [batch][MPCQP_EO_SIZE] (NULL: skipped); nothing else.  A robot's first tick (zero slot) runs init_state
 * only and leaves MPCQP_ST_POS / _LIN_VEL as the caller wrote them (A1BasicEKF.cpp:55-68 does not touch
 * state.root_pos).  The innovation covariance S = C Pbar C' + R is factored without pivoting (LDL'; the
 * reference: fullPivHouseholderQr, :134-138).  A robot whose sensor row is non-finite, or whose
 * factorization meets a pivot that is not positive and finite, keeps its slot untouched and gets NaN in
 * MPCQP_ST_POS / _LIN_VEL, so the solve reports MPCQP_STATUS_NAN_INPUT for that robot alone. */
int32_t mpcqp_state_estimate_device(const mpcqp_est_params* pp, double dt, const double* d_sensors,
                                    double* d_plan_in, double* d_states, int32_t batch, double* d_est_state,
                                    double* d_tq_records, double* d_est_out, void* stream);

/* ---- single-step QP balance controller: the stance_leg_control_type == 0 branch of
 * A1RobotControl::compute_grf (A1RobotControl.cpp:321-332 euler error, :377-444 QP), constants
 * from the A1RobotControl ctor (:7-48).  12 variables (world-frame GRF), 20 rows (4 fz bounds,
 * 16 friction-pyramid rows), a fresh OsqpEigen::Solver every tick (warm start off, :420).
 * One binary64 record per robot (offsets in doubles; matrices row-major).                    */
#define MPCQP_BAL_POS 0        /* [3] root_pos (world)                                       */
#define MPCQP_BAL_POS_D 3      /* [3] root_pos_d                                             */
#define MPCQP_BAL_ROT 6        /* [9] root_rot_mat                                           */
#define MPCQP_BAL_ROT_Z 15     /* [9] root_rot_mat_z (yaw-only rotation)                     */
#define MPCQP_BAL_LIN_VEL 24   /* [3] root_lin_vel (world)                                   */
#define MPCQP_BAL_LIN_VEL_D 27 /* [3] root_lin_vel_d (body, as :382 reads it)                */
#define MPCQP_BAL_ANG_VEL 30   /* [3] root_ang_vel (world)                                   */
#define MPCQP_BAL_ANG_VEL_D 33 /* [3] root_ang_vel_d (body)                                  */
#define MPCQP_BAL_EULER 36     /* [3] root_euler                                             */
#define MPCQP_BAL_EULER_D 39   /* [3] root_euler_d                                           */
#define MPCQP_BAL_KP_LIN 42    /* [3] kp_linear                                              */
#define MPCQP_BAL_KD_LIN 45    /* [3] kd_linear                                              */
#define MPCQP_BAL_KP_ANG 48    /* [3] kp_angular                                             */
#define MPCQP_BAL_KD_ANG 51    /* [3] kd_angular                                             */
#define MPCQP_BAL_MASS 54      /* robot_mass                                                 */
#define MPCQP_BAL_FEET 55      /* [4][3] foot_pos_abs column i (world-aligned, body origin)   */
#define MPCQP_BAL_CONTACTS 67  /* [4] contacts[i] as 0.0 / 1.0                               */
#define MPCQP_BAL_SIZE 72      /* 71 used, padded to a multiple of 4 doubles                 */

typedef struct mpcqp_balance_params {
  double q_diag[6]; /* Q.diagonal() = 1, 1, 1, 400, 400, 100 (A1RobotControl.cpp:11)   */
  double r;         /* R = 1e-3 (:12)                                                    */
  double mu;        /* 0.7 (:13)                                                         */
  double f_min;     /* F_min = 0 (:14)                                                   */
  double f_max;     /* F_max = 180 (:15)                                                 */
} mpcqp_balance_params;

void mpcqp_balance_default_params(mpcqp_balance_params* p);

/* Replaces the QP branch of compute_grf for `batch` robots (DEVICE pointers, async on `stream`):
 * root_acc, H = R I + M'QM, g = -M'Q root_acc, bounds from contacts, OSQP setup + solve with the
 * handle's OSQP settings (warm_start ignored: the reference builds a new solver each tick).
 * d_results[b].u0 = QPSolution (world), .f_body = root_rot_mat^T QPSolution per leg (no NaN
 * guard in this branch, :440-443: a NaN solution stays NaN and sets nan_legs). */
int32_t mpcqp_balance_solve_device(mpcqp_handle* h, const mpcqp_balance_params* bp, const double* d_records,
                                   int32_t batch, mpcqp_result* d_results, void* stream);
/* The same for the robots of one control type: robot b is solved iff d_type == NULL || d_type[b] == type
 * (d_type a DEVICE int32 [batch], read when the kernel runs).  The mpcqp_result row of a robot that is
 * not selected is not written; a selected robot's row is bitwise mpcqp_balance_solve_device's. */
int32_t mpcqp_balance_solve_typed_device(mpcqp_handle* h, const mpcqp_balance_params* bp, const double* d_records,
                                         int32_t batch, const int32_t* d_type, int32_t type, mpcqp_result* d_results,
                                         void* stream);

/* The PD gains of the balance branch's root_acc (A1RobotControl.cpp:380-390). */
typedef struct mpcqp_balance_gains {
  double kp_linear[3];  /* 100, 100, 300 (Go1CtrlStates.hpp:279-281)  */
  double kd_linear[3];  /* 70, 70, 120 (Go1CtrlStates.hpp:286-288)    */
  double kp_angular[3]; /* 150, 150, 1 (Go1CtrlStates.hpp:293-295)    */
  double kd_angular[3]; /* 4.5, 4.5, 30 (Go1CtrlStates.hpp:300-302)   */
} mpcqp_balance_gains;

void mpcqp_balance_default_gains(mpcqp_balance_gains* g);

/* Replaces the host packing of the MPCQP_BAL_* record (the fields A1RobotControl.cpp:321-332, :377-444
 * read from the controller state) for `batch` robots: d_states [batch][MPCQP_ST_SIZE], MPCQP_PL_ROT_Z of
 * d_plan_in [batch][MPCQP_PL_SIZE], the gains, and kp_linear from MPCQP_CS_KP_LINEAR of d_cmd_state
 * [batch][MPCQP_CS_SIZE] (NULL: gains->kp_linear) -> d_bal_records [batch][MPCQP_BAL_SIZE].  Pure copies
 * (contacts as given; the padding is written 0).  DEVICE pointers, async on `stream`, capture safe.
 * Chain it before mpcqp_balance_solve_device on the same stream. */
int32_t mpcqp_assemble_balance_device(const mpcqp_balance_gains* gains, const double* d_states,
                                      const double* d_plan_in, const double* d_cmd_state, int32_t batch,
                                      double* d_bal_records, void* stream);

/* Host-pointer convenience wrapper of mpcqp_balance_solve_device (copies in, solves, copies out, synchronizes). */
int32_t mpcqp_balance_solve_host(mpcqp_handle* h, const mpcqp_balance_params* bp, const double* h_records,
                                 int32_t batch, mpcqp_result* h_results);

/* ---- policy stage: the reference's third controller, the Go1 learned walking policy with its servo
 * stand (src/go1_rl_ctrl_cpp): per robot and per tick
 *   observation     observation/Go1Observation.hpp:152-166, cast to float32 with the previous action
 *                   appended (Go1RLController.cpp:95-96)
 *   network         the TorchScript MLP of TorchEigen::run (Go1RLController.cpp:98), 48 -> hidden -> 12,
 *                   ELU, float32
 *   action          clip, prev_action, scale, default pose, pose limits (:99-109)
 *   servo stand     advance_servo (:121-146)
 *   motor law       tau = Kp (target - q) - Kd dq with the gains of the mode that ran (:79-86, :125-132).
 *                   The reference sends the LowCmd (q = target, dq = 0, tau = 0, :149-166) and leaves this
 *                   line to the motor controller; the tick's output is joint torques, so the stage applies it.
 * The robot's mode is MPCQP_PL_MOVEMENT_MODE, as SwitchController's toggle sets it (MainGazebo.cpp:74-83):
 * 1.0 runs advance, anything else advance_servo.  The hardware variant's observation, the C++ call surface
 * and the ROS debug topics are not built; updateHistory (Go1Observation.hpp:172-181) is dead code there.  */
typedef struct mpcqp_policy mpcqp_policy; /* device-resident packed weights and parameters */

typedef struct mpcqp_policy_params {
  int32_t n_hidden;             /* hidden layers, 1..3; 3 (cpp_model.pt)                                  */
  int32_t hidden[3];            /* their widths, each a multiple of 32 and <= 512; 512, 256, 128          */
  int32_t servo_clamp;          /* 0 (the reference: percent grows past 1, :139-142); 1 clamps it to 1   */
  int32_t decimation;           /* ticks per action update; 1 (parameters.yaml:9-11 is 2)                 */
  double obs_scale[36];         /* scaleFactor_: 2 x3, 0.25 x3, 1 x3, (2, 2, 0.25), 1 x12, 0.05 x12
                                   (Go1Observation.hpp:52-63)                                             */
  double clip_obs;              /* clipObs_ = 100 (Go1Observation.hpp:449)                                */
  double clip_action;           /* clipAction_ = 100 (Go1RLController.hpp:84)                             */
  double action_scale;          /* actionScale_ = 0.25 (Go1RLController.hpp:88)                           */
  double default_joint_pos[12]; /* (+-0.1, 0.8 front / 1.0 rear, -1.5) (Go1CtrlStates.hpp:75-78)          */
  double pose_lower[12];        /* clipPoseLower_ (-0.9425, -0.4817, -2.6285) (Go1RLController.cpp:36)    */
  double pose_upper[12];        /* clipPoseUpper_ (0.9425, 2.7855, -0.9320) (:37)                         */
  double kp_walk[12];           /* (20, 50, 50) per leg (:79-82)                                          */
  double kd_walk[12];           /* (1, 2, 2) per leg (:83-86)                                             */
  double kp_servo[12];          /* (20, 30, 60) front, (20, 80, 140) rear (:125-128)                      */
  double kd_servo[12];          /* (5, 8, 12) per leg (:129-132)                                          */
  double stand_pos[12];         /* (+-0.1, 0.6, -1.3) per leg (:122-123)                                  */
  double servo_ticks;           /* 1000 (:139)                                                            */
} mpcqp_policy_params;

void mpcqp_policy_default_params(mpcqp_policy_params* p);
int32_t mpcqp_policy_params_size(void); /* sizeof(mpcqp_policy_params), for binding checks */

/* Packs the network for the device once.  h_weights[l] is layer l's HOST matrix [out][in], row-major as
 * torch.nn.Linear stores it, h_biases[l] its [out] vector, l = 0 .. n_hidden; layer 0 has 48 inputs and
 * the last layer 12 outputs (Go1RLController.cpp:95, :34).  Allocates and copies (synchronous); the
 * parameters are copied with the weights, so later changes to *params do not reach the policy.      */
int32_t mpcqp_policy_create(const mpcqp_policy_params* params, const float* const* h_weights,
                            const float* const* h_biases, int32_t device, mpcqp_policy** out);
int32_t mpcqp_policy_destroy(mpcqp_policy* p);

/* Policy slot, a caller-owned DEVICE buffer d_policy_state [batch][mpcqp_policy_state_size()] that must
 * follow its robot from tick to tick: the members Go1RLController keeps (offsets in doubles).
 * Zero-filled = fresh, as the constructor leaves them (Go1RLController.cpp:34-35, :50).             */
#define MPCQP_PS_INIT 0         /* 0.0: fresh; 1.0 once the robot has run                             */
#define MPCQP_PS_TICK 1         /* ticks run so far: an update is due when tick % decimation == 0     */
#define MPCQP_PS_SERVO_TIME 2   /* servo_motion_time_ (:136; never reset, as in the reference)        */
#define MPCQP_PS_MODE 3         /* the mode the last update ran: 1.0 advance, 0.0 advance_servo       */
#define MPCQP_PS_PREV_ACTION 4  /* [12] prevActionDouble_ (:103)                                      */
#define MPCQP_PS_TARGET 16      /* [12] targetPoses_ (:109, :141)                                     */
#define MPCQP_PS_SIZE 28        /* a multiple of 4 doubles                                            */
int32_t mpcqp_policy_state_size(void);

/* Optional output row d_policy_out [batch][MPCQP_PY_SIZE] (NULL = skipped), offsets in doubles. */
#define MPCQP_PY_OBS 0      /* [48] the observation the network saw, float32 values widened (:95-96)  */
#define MPCQP_PY_RAW 48     /* [12] action_, the raw network output (:98); 0 unless this tick ran advance */
#define MPCQP_PY_ACTION 60  /* [12] the clipped action = prev_action after this tick (:102-103)       */
#define MPCQP_PY_TARGET 72  /* [12] targetPoses_ in force                                             */
#define MPCQP_PY_TORQUE 84  /* [12] what was written to d_joint_torques                               */
#define MPCQP_PY_STATUS 96  /* 0.0 ran; 1.0 a non-finite input: only this and MPCQP_PY_UPDATED are written */
#define MPCQP_PY_UPDATED 97 /* 1.0 if this tick ran advance / advance_servo, 0.0 if it held the targets */
#define MPCQP_PY_SIZE 100   /* 98 used, padded to a multiple of 4 doubles                             */

/* One policy tick for `batch` robots (DEVICE pointers, async on `stream`, no allocation and no
 * synchronization: hipGraph-capture safe; one kernel).  Robot b runs iff d_type == NULL || d_type[b] ==
 * type (d_type a DEVICE int32 [batch], read when the kernel runs); of a robot that is not selected not a
 * bit of its slot, its torques row or its output row is written.  Reads, per selected robot,
 * MPCQP_SN_JOINT_POS, _JOINT_VEL and _IMU_ANG_VEL of d_sensors [batch][MPCQP_SN_SIZE], MPCQP_ST_LIN_VEL and
 * MPCQP_ST_ROT of d_states [batch][MPCQP_ST_SIZE], MPCQP_PL_ROT_Z and MPCQP_PL_MOVEMENT_MODE of d_plan_in
 * [batch][MPCQP_PL_SIZE], and joy_cmd_velx, joy_cmd_vely (MPCQP_CM_VEL) and joy_cmd_yaw_rate (MPCQP_CM_RATE
 * + 2) of d_cmd [batch][MPCQP_CM_SIZE] (Go1Observation.hpp:152-157).
 *   On a tick with MPCQP_PS_TICK % decimation == 0 the robot updates: mode 1.0 builds the observation in
 * binary64 (unfused, left to right; scale, clip, cast to float32, previous action appended), runs the
 * network in float32 (a k-ordered fused multiply-add chain per output with the bias as its start, expm1f
 * for ELU), clips the action, stores it as prev_action and forms the targets (:99-109); any other mode
 * advances servo_motion_time and interpolates the targets (:136-142) and keeps prev_action.  The mode
 * that ran is stored.  On EVERY tick tau_j = Kp_j (target_j - q_j) - Kd_j dq_j with the stored targets and
 * the stored mode's gains goes to d_joint_torques [batch][12], and the tick counter advances.
 *   A robot with a non-finite value among the fields read above (the movement mode excepted, which is
 * only compared with 1.0) keeps its slot and its torques row, gets MPCQP_PY_STATUS 1.0, and enters the
 * network as a zero row, so the robots that share its tile are unaffected.                           */
int32_t mpcqp_policy_device(const mpcqp_policy* policy, const double* d_sensors, const double* d_states,
                            const double* d_plan_in, const double* d_cmd, int32_t batch, double* d_policy_state,
                            const int32_t* d_type, int32_t type, double* d_joint_torques, double* d_policy_out,
                            void* stream);

/* ---- plant stage: a rigid-body model of the robot that turns the tick's joint torques back into the next
 * tick's sensor rows, so a fleet closes its loop on the device (the reference closed its loop through Gazebo;
 * this model has no counterpart there).  A single rigid trunk on massless stance legs, joint-space swing legs,
 * flat ground z = 0:
 *   stance leg   its foot is held where it touched down (a held foot does not slip); the joint angles follow
 *                from the analytic inverse of the estimator's leg kinematics, the joint rates from
 *                J^-1 (-R' v - w x p), and the joint torques act on the trunk as the ground reaction
 *                f = -R J^-T tau (the inverse of the torque map's tau = J' (-f_grf)).  A leg whose f_z < 0
 *                lets go; f_x, f_y are scaled onto the friction cone mu f_z.
 *   swing leg    every joint is a free inertia, qdd = (tau - b qd) / I_j; the foot follows from the forward
 *                kinematics and lands when it reaches z <= 0 moving down (its z is set to 0).
 *   trunk        a = sum f / m - g, wd = I^-1 (R' sum r x f - w x I w), semi-implicit Euler in `substeps`
 *                substeps per tick with the torque row held; the quaternion is renormalised every substep.
 * mpcqp_plant_step_terrain_device (below) replaces the flat ground by a per-robot inclined plane with its own
 * friction coefficient, and mpcqp_plant_step_field_device by a bilinear height field (steps, stairs, rough ground).
 * Left out: leg mass, the swing legs' reaction on the trunk, foot slip, overhangs, a riser's vertical face as
 * anything but one steep cell, trunk-ground contact, joint limits, and impact dynamics beyond zeroing the landing
 * foot's velocity.  Only the feet touch the ground: a trunk that sinks to min_height is reported as fallen, it does
 * not come to rest.  Binary64, multiplies and adds not contracted, in the statement order of
 * tests/plant_reference.py.                                                                                */
typedef struct mpcqp_plant_params {
  double rho_fix[4][5];         /* leg geometry, as mpcqp_est_params (the estimator's kinematics and the       */
  double rho_opt[4][3];         /* plant's agree when these do)                                                */
  double mass;                  /* 13 (Go1CtrlStates.hpp:145-195)                                              */
  double inertia[9];            /* trunk inertia, body frame, row-major: diag(0.0168352186, 0.0656071082,
                                   0.0742720659)                                                               */
  double mu;                    /* ground friction, 0.6                                                        */
  double gravity;               /* 9.81                                                                        */
  double joint_inertia[3];      /* hip, thigh, calf: 0.03, 0.03, 0.01 kg m^2.  Chosen for the model's swing legs
                                   to settle under the policy stage's walk gains; NOT identified from a robot
                                   description                                                                 */
  double joint_damping[3];      /* 0                                                                           */
  double default_joint_pos[12]; /* (0, 0.8, -1.6) per leg: the pose of a fresh slot without an init row        */
  double min_height;            /* 0.05: a trunk below it has fallen (status 2)                                */
  int32_t substeps;             /* 4; 1..16                                                                    */
  int32_t pad_;
} mpcqp_plant_params;

void mpcqp_plant_default_params(mpcqp_plant_params* p);
int32_t mpcqp_plant_params_size(void); /* sizeof(mpcqp_plant_params), for bindings */

/* Plant slot, a caller-owned DEVICE buffer d_plant_state [batch][mpcqp_plant_state_size()] that must follow
 * its robot from tick to tick (offsets in doubles; FL FR RL RR leg order).  Zero-filled = fresh, the
 * convention of every other slot: the first tick initialises it and does not integrate.  Zeroing a robot's
 * slots (this one and the controller's) is how a fleet resets a fallen robot; mpcqp_episode_device (below)
 * does that on the device, in the two ticks a restart needs.                                              */
#define MPCQP_PN_INIT 0        /* 0.0: fresh                                                             */
#define MPCQP_PN_POS 1         /* [3] trunk position, world                                              */
#define MPCQP_PN_QUAT 4        /* [4] trunk attitude as w, x, y, z                                       */
#define MPCQP_PN_LIN_VEL 8     /* [3] trunk linear velocity, world                                       */
#define MPCQP_PN_ANG_VEL 11    /* [3] trunk angular velocity, body                                       */
#define MPCQP_PN_JOINT_POS 14  /* [12] joint angles                                                      */
#define MPCQP_PN_JOINT_VEL 26  /* [12] joint rates                                                       */
#define MPCQP_PN_FOOT 38       /* [4][3] foot positions, world                                           */
#define MPCQP_PN_CONTACT 50    /* [4] 1.0: the foot is held on the ground                                */
#define MPCQP_PN_ACC 54        /* [3] trunk acceleration of the last substep, world                      */
#define MPCQP_PN_STATUS 57     /* 0.0 fine; 1.0 a leg out of reach; 2.0 fallen: frozen until zeroed      */
#define MPCQP_PN_SIZE 64       /* 58 used, padded to a multiple of 4 doubles                             */
int32_t mpcqp_plant_state_size(void);

/* Optional init row d_plant_init [batch][MPCQP_PI_SIZE], read on a fresh slot's first tick only. */
#define MPCQP_PI_POS 0         /* [3] trunk position, world                                              */
#define MPCQP_PI_QUAT 3        /* [4] trunk attitude as w, x, y, z (unit)                                */
#define MPCQP_PI_JOINT_POS 7   /* [12] joint angles                                                      */
#define MPCQP_PI_SIZE 20       /* 19 used, padded to a multiple of 4 doubles                             */

/* Optional output row d_plant_out [batch][MPCQP_PT_SIZE], for logging and rewards. */
#define MPCQP_PT_POS 0         /* [3] trunk position, world                                              */
#define MPCQP_PT_QUAT 3        /* [4] trunk attitude as w, x, y, z                                       */
#define MPCQP_PT_EULER 7       /* [3] roll, pitch, yaw (Utils::quat_to_euler)                            */
#define MPCQP_PT_LIN_VEL 10    /* [3] world                                                              */
#define MPCQP_PT_ANG_VEL 13    /* [3] body                                                               */
#define MPCQP_PT_CONTACTS 16   /* [4] 0.0 / 1.0                                                          */
#define MPCQP_PT_GRF 20        /* [4][3] ground reactions of the last substep, world; 0 for a leg off the ground */
#define MPCQP_PT_FOOT 32       /* [4][3] foot positions, world                                           */
#define MPCQP_PT_ACC 44        /* [3] trunk acceleration of the last substep, world                      */
#define MPCQP_PT_STATUS 47     /* 0.0 .. 2.0 as MPCQP_PN_STATUS; 3.0 a non-finite torque row (this tick only) */
#define MPCQP_PT_SIZE 48

/* One plant tick for `batch` robots (DEVICE pointers, async on `stream`, no allocation and no
 * synchronization: hipGraph-capture safe; one kernel).  Chain it last in the tick, after
 * mpcqp_joint_torques_device / mpcqp_policy_device on the same stream.  Reads d_joint_torques [batch][12] and
 * the slot, and on a fresh slot d_plant_init (NULL: identity attitude, x = y = 0, default_joint_pos, and the
 * height at which leg 0's foot is at z = 0; all velocities zero; a foot at z <= 0 starts held at z = 0, the
 * others in swing).  A fresh slot's tick initialises and does not integrate; every other tick runs `substeps`
 * substeps of dt / substeps.  Each output pointer may be NULL, which skips it:
 *   d_sensors [batch][MPCQP_SN_SIZE]   MPCQP_SN_QUAT, _JOINT_POS, _JOINT_VEL, _IMU_ACC = R' (a + (0, 0, g)) with
 *                                      the last substep's a (+g at rest, as A1BasicEKF.cpp:76 expects),
 *                                      _IMU_ANG_VEL = w
 *   d_plan_in [batch][MPCQP_PL_SIZE]   MPCQP_PL_FOOT_FORCE = f_z of a held foot, else 0; MPCQP_PL_ROT_Z
 *   d_states [batch][MPCQP_ST_SIZE]    the ground truth of what mpcqp_state_estimate_device estimates:
 *                                      MPCQP_ST_EULER, _POS, _ANG_VEL (world), _LIN_VEL, _ROT, _FEET
 *   d_tq_records [batch][MPCQP_TQ_SIZE] MPCQP_TQ_JFOOT
 *   d_plant_out [batch][MPCQP_PT_SIZE]
 * so a tick without the estimator can run on d_states / d_tq_records, and one with it on d_sensors.
 *   A robot whose MPCQP_PN_STATUS is not 0 is frozen: not one of its doubles, in the slot or in a row, is
 * written until its slot is zeroed.  A leg that leaves its reach (y^2 + z^2 < dd^2 or |cos knee| > 1 in the
 * inverse kinematics) during a tick undoes that tick: the slot and the rows keep their values and status 1.0
 * goes to MPCQP_PN_STATUS and MPCQP_PT_STATUS.  A trunk that ends a tick below min_height is written as it
 * is, with status 2.0.  A robot whose torque row is non-finite gets 3.0 in MPCQP_PT_STATUS and nothing else
 * written that tick, and carries on with the next finite row.                                            */
int32_t mpcqp_plant_step_device(const mpcqp_plant_params* pp, double dt, const double* d_joint_torques,
                                int32_t batch, double* d_plant_state, const double* d_plant_init,
                                double* d_sensors, double* d_plan_in, double* d_states, double* d_tq_records,
                                double* d_plant_out, void* stream);

/* ---- episode stage: the last stage of a tick that ends with the plant.  Per robot it accumulates the
 * episode's metrics from the tick's rows, decides when the episode ends, writes the episode into a per-robot
 * log ring and per-robot totals, and restarts the robot from a start state drawn on the device out of a
 * caller-built pool, under a command script that restarts with it.  T replays of a tick that ends with it are
 * a Monte-Carlo evaluation of the fleet with no host write in between.
 *
 * A robot's phase (MPCQP_ES_PHASE) is 0 fresh, 1 running or 2 priming.  A restart takes two ticks, because a
 * fresh plant slot initialises at the END of its tick: the controller stages of that tick still run on the
 * fallen robot's stale rows and initialise their slots from them.
 *   ending tick (phase 0 or 1).  A running robot first adds this tick to its metrics, then tests the end
 *     reasons in the order of MPCQP_EP_END_*.  A fresh robot ends at once with reason 0 and writes no log row
 *     (so a tick built with the stage needs no init rows and no separate plant launch).  On an end of a running
 *     robot the stage writes the log row at ring position episode % log_len, adds the episode to the totals
 *     and increments the episode index; on every end it counts the reason in the totals, draws the next
 *     episode's pool and script indices, zero-fills the robot's plant slot row and torque row (the plant's
 *     non-finite-torque rule must not block the initialisation), writes the pool row's init part to
 *     d_plant_init and sets phase 2.
 *   priming tick (phase 2), the next one: its plant stage has just initialised the fresh slot and written
 *     clean sensor rows.  The stage zero-fills the robot's row of every controller slot given, of d_results and
 *     of d_counter, writes MPCQP_ST_EULER_D / MPCQP_ST_POS_D from the pool row and, if an estimator slot is
 *     given, zero into MPCQP_ST_POS / _LIN_VEL (the estimator's first tick leaves them as they are; zero is
 *     A1CtrlStates::reset, A1CtrlStates.h:62-67), writes script segment 0 into the cmd row if its start tick is 0, takes the start pose from d_plant_out, clears the sums, sets tick 0 and
 *     phase 1.  No tick is added to the metrics.
 * Whatever the controller stages wrote between the two from stale rows is zeroed or rewritten by the priming
 * tick.  A running robot that does not end and whose next script segment starts at tick + 1 gets that segment
 * written to its cmd row (the stage runs last: it writes the next tick's command), then tick += 1.  A script
 * should start with a segment at tick 0: otherwise the cmd row keeps the previous episode's last command until
 * the first segment.
 *
 * Draws: Philox4x32-10 with key = seed[0], seed[1] and counter = (robot, episode index, 0, 0); pool index =
 * (uint64(w0) * pool_count) >> 32, script index = (uint64(w1) * script_count) >> 32.  Integers only.
 *
 * Metrics: binary64, multiplies and adds not contracted, no libm call, in the statement order of
 * tests/episode_reference.py; sums over the four legs are (l0 + l1) + (l2 + l3); a NaN metric is stored as the
 * quiet NaN 0x7FF8000000000000, so the rows are bitwise those of the restatement.  No atomics: the totals are
 * per-robot rows the host sums, so no number depends on scheduling.                                        */
typedef struct mpcqp_episode_params {
  double dt;               /* control period: the energy is sum(power) * dt.  0.0025                       */
  double tilt_max;         /* envelope: roll^2 + pitch^2 > tilt_max^2 ends the episode.  0.5                */
  double height_min;       /* envelope: trunk z < height_min or > height_max ends it.  0.12, 0.6            */
  double height_max;
  uint32_t seed[2];        /* the Philox key                                                               */
  int32_t max_ticks;       /* an episode of this many ticks ends with MPCQP_EP_END_TIMEOUT.  2000          */
  int32_t pool_count;      /* rows of d_pool                                                               */
  int32_t script_count;    /* scripts of d_scripts                                                         */
  int32_t script_segments; /* segments per script                                                          */
  int32_t log_len;         /* rows per robot of the d_log ring.  4                                         */
  int32_t pad_;
} mpcqp_episode_params;

void mpcqp_episode_default_params(mpcqp_episode_params* p);
int32_t mpcqp_episode_params_size(void); /* sizeof(mpcqp_episode_params), for bindings */

/* End reasons, in the order they are tested. */
#define MPCQP_EP_END_FRESH 0       /* the slot was fresh: the first start                                  */
#define MPCQP_EP_END_OUT_OF_REACH 1 /* MPCQP_PT_STATUS 1.0                                                 */
#define MPCQP_EP_END_FALLEN 2      /* MPCQP_PT_STATUS 2.0                                                  */
#define MPCQP_EP_END_BAD_TORQUE 3  /* MPCQP_PT_STATUS 3.0                                                  */
#define MPCQP_EP_END_ENVELOPE 4    /* tilt, height, or a non-finite entry of MPCQP_PT_POS, _QUAT, _EULER   */
#define MPCQP_EP_END_TIMEOUT 5     /* tick + 1 >= max_ticks                                                */
#define MPCQP_EP_END_COUNT 6

/* Pool row d_pool [pool_count][MPCQP_EP_POOL_SIZE]: a plant init row and the desired values that live in the
 * caller's state row from tick to tick.  The host builds it, so no kinematics or trigonometry runs here.  */
#define MPCQP_EP_POOL_INIT 0     /* [MPCQP_PI_SIZE] the plant init row                                     */
#define MPCQP_EP_POOL_EULER_D 20 /* [3] root_euler_d                                                       */
#define MPCQP_EP_POOL_POS_D 23   /* [3] root_pos_d                                                         */
#define MPCQP_EP_POOL_SIZE 28    /* 26 used, padded to a multiple of 4 doubles                             */

/* Script segment, d_scripts [script_count][script_segments][MPCQP_EP_SEG_SIZE], sorted by start tick; a start
 * tick < 0 ends the list. */
#define MPCQP_EP_SEG_TICK 0      /* the episode tick at which the segment takes effect                     */
#define MPCQP_EP_SEG_CMD 1       /* [7] MPCQP_CM_VEL, MPCQP_CM_RATE, MPCQP_CM_MODE_REQUEST                 */
#define MPCQP_EP_SEG_SIZE 8

/* Episode slot d_episode_state [batch][mpcqp_episode_state_size()]; zero-filled = fresh. */
#define MPCQP_ES_PHASE 0         /* 0.0 fresh, 1.0 running, 2.0 priming                                    */
#define MPCQP_ES_TICK 1          /* ticks of the episode so far                                            */
#define MPCQP_ES_EPISODE 2       /* index of the episode that runs (or is being primed)                    */
#define MPCQP_ES_POOL 3          /* its pool row                                                           */
#define MPCQP_ES_SCRIPT 4        /* its script                                                             */
#define MPCQP_ES_SEG 5           /* the script's next segment                                              */
#define MPCQP_ES_METRICS 6       /* [MPCQP_EM_SIZE] the metrics so far                                     */
#define MPCQP_ES_SIZE 24         /* 23 used, padded to a multiple of 4 doubles                             */
int32_t mpcqp_episode_state_size(void);

/* The metrics block of the slot and of a log row. */
#define MPCQP_EM_TILT2_MAX 0     /* max of roll^2 + pitch^2, the start included                            */
#define MPCQP_EM_Z_MIN 1         /* min and max trunk z, the start included                                */
#define MPCQP_EM_Z_MAX 2
#define MPCQP_EM_ENERGY 3        /* sum over ticks of (sum_j tau_j qd_j) * dt                              */
#define MPCQP_EM_TAU2 4          /* sum of tau_j^2                                                         */
#define MPCQP_EM_ERR_V 5         /* [3] sum of squared body-frame tracking error: v_x, v_y, yaw rate       */
#define MPCQP_EM_ITERS 8         /* sum of mpcqp_result.iters                                              */
#define MPCQP_EM_NOT_SOLVED 9    /* ticks whose mpcqp_result.status is not MPCQP_STATUS_SOLVED             */
#define MPCQP_EM_LOW_CONTACT 10  /* ticks with fewer than two contacts                                     */
#define MPCQP_EM_START 11        /* [3] x, y, yaw at the start                                             */
#define MPCQP_EM_END 14          /* [3] x, y, yaw at the last tick                                         */
#define MPCQP_EM_SIZE 17

/* Log row d_log [batch][log_len][MPCQP_EL_SIZE], the ring of a robot's last log_len episodes. */
#define MPCQP_EL_EPISODE 0
#define MPCQP_EL_POOL 1
#define MPCQP_EL_SCRIPT 2
#define MPCQP_EL_LENGTH 3        /* ticks                                                                  */
#define MPCQP_EL_REASON 4        /* MPCQP_EP_END_*                                                         */
#define MPCQP_EL_METRICS 5       /* [MPCQP_EM_SIZE]                                                        */
#define MPCQP_EL_SIZE 24         /* 22 used, padded to a multiple of 4 doubles                             */

/* Totals row d_totals [batch][MPCQP_ET_SIZE]; the host sums the rows. */
#define MPCQP_ET_EPISODES 0      /* episodes completed (the fresh start is none)                           */
#define MPCQP_ET_TICKS 1         /* their ticks                                                            */
#define MPCQP_ET_REASON 2        /* [MPCQP_EP_END_COUNT] ends per reason                                   */
#define MPCQP_ET_SIZE 8

/* The stage's buffers: DEVICE pointers and the row sizes, in doubles, of the controller slots.  Every pointer
 * except d_plant_out and d_plant_state may be NULL, which skips what it serves: without d_joint_torques the
 * energy and the torque sum stay 0, without d_sensors the energy, without d_results the iteration and
 * not-solved counts; without d_cmd the tracking error is taken against a zero command and no script is written.
 * Every pointer of doubles must be 16-byte aligned (MPCQP_ERR_INVALID_ARG otherwise). */
typedef struct mpcqp_episode_buffers {
  const double* d_plant_out;  /* [batch][MPCQP_PT_SIZE]  read                                              */
  double* d_plant_state;      /* [batch][MPCQP_PN_SIZE]  zero-filled on an end                             */
  double* d_plant_init;       /* [batch][MPCQP_PI_SIZE]  written on an end                                 */
  double* d_joint_torques;    /* [batch][12]             read; zero-filled on an end                       */
  const double* d_sensors;    /* [batch][MPCQP_SN_SIZE]  MPCQP_SN_JOINT_VEL read, for the energy           */
  double* d_cmd;              /* [batch][MPCQP_CM_SIZE]  read (tracking error); script segments written    */
  mpcqp_result* d_results;    /* [batch]                 status and iters read; zero-filled when priming   */
  const double* d_pool;       /* [pool_count][MPCQP_EP_POOL_SIZE]                                          */
  const double* d_scripts;    /* [script_count][script_segments][MPCQP_EP_SEG_SIZE]                        */
  double* d_states;           /* [batch][MPCQP_ST_SIZE]  MPCQP_ST_EULER_D, _POS_D written when priming      */
  int32_t* d_counter;         /* [batch]                 the torque map's counter, zeroed when priming     */
  double* d_log;              /* [batch][log_len][MPCQP_EL_SIZE]                                           */
  double* d_totals;           /* [batch][MPCQP_ET_SIZE]                                                    */
  double* d_est_state;        /* the controller slots, zero-filled when priming, with their row sizes      */
  double* d_plan_state;
  double* d_cmd_state;
  double* d_policy_state;
  double* d_warm;             /* row size mpcqp_warm_state_size(horizon); may be odd                       */
  int32_t est_state_size, plan_state_size, cmd_state_size, policy_state_size, warm_size;
  int32_t pad_;
} mpcqp_episode_buffers;
int32_t mpcqp_episode_buffers_size(void); /* sizeof(mpcqp_episode_buffers), for bindings */

/* One episode tick for `batch` robots (DEVICE pointers, async on `stream`, no allocation and no
 * synchronization: hipGraph-capture safe; one kernel).  Chain it last in the tick, after
 * mpcqp_plant_step_device on the same stream, and give the plant stage the same d_plant_init.  The structs are
 * read when the call is made. */
int32_t mpcqp_episode_device(const mpcqp_episode_params* ep, const mpcqp_episode_buffers* buf, int32_t batch,
                             double* d_episode_state, void* stream);

/* ---- disturbance stage: the first stage of a tick that has the plant and the episode stage.  It draws, on the
 * device, what the world does to each robot this tick: a push, the weight of a payload, and sensor noise with
 * IMU biases.  The plant takes the first two through a wrench row; the estimator and the policy stage read the
 * third as a second, noisy sensor row.
 *
 * Wrench row d_wrench [batch][MPCQP_PW_SIZE]: two applied forces, each a world-frame force and a body-frame
 * application point relative to the trunk's centre of mass.                                                 */
#define MPCQP_PW_FORCE0 0        /* [3] force 0, world (the disturbance stage: the push)                   */
#define MPCQP_PW_POINT0 3        /* [3] its application point, body frame                                  */
#define MPCQP_PW_FORCE1 6        /* [3] force 1, world (the disturbance stage: the payload's weight)       */
#define MPCQP_PW_POINT1 9        /* [3] its application point, body frame                                  */
#define MPCQP_PW_SIZE 12

/* mpcqp_plant_step_device with external forces.  d_wrench == NULL is mpcqp_plant_step_device, bit for bit.  With
 * a row F0, p0, F1, p1, step 3 of every substep becomes, with that substep's R and contraction off,
 *     Fe   = F0 + F1                              (per component)
 *     F    = ((f_0 + f_1) + (f_2 + f_3)) + Fe     (the legs' sum first, as without a wrench)
 *     Fb_i = R' F_i,  c_i = p_i x Fb_i            (R' v and a x b as everywhere in the plant)
 *     Ce   = c_0 + c_1                            (per component)
 *     Mb   = R' M + Ce                            (M the legs' moment sum, as without a wrench)
 *     wd   = I^-1 (Mb - w x I w)
 * and nothing else changes.  A component of Fe or Ce that compares equal to zero is skipped, not added (x + 0.0
 * would turn a sum that is exactly -0.0, which a robot standing under zero torques produces, into +0.0): so an
 * all-zero row, too, leaves every bit as mpcqp_plant_step_device computes it.  The row is held over the tick's
 * substeps, like the torque row.  A non-finite wrench row is treated like a non-finite torque row: 3.0 in
 * MPCQP_PT_STATUS and nothing else written that tick.  The forces model what pushes or loads the trunk; they
 * carry no mass, so a payload's weight is modelled and its inertia is not.                                  */
int32_t mpcqp_plant_step_wrench_device(const mpcqp_plant_params* pp, double dt, const double* d_joint_torques,
                                       const double* d_wrench, int32_t batch, double* d_plant_state,
                                       const double* d_plant_init, double* d_sensors, double* d_plan_in,
                                       double* d_states, double* d_tq_records, double* d_plant_out, void* stream);

/* ---- inclined ground and per-robot friction.  Terrain row d_terrain [terrain_rows][MPCQP_TR_SIZE]: the ground
 * of a robot is the plane {p : n.p = d} with its own friction coefficient.                                    */
#define MPCQP_TR_NORMAL 0        /* [3] unit normal n, world, with n_z > 0                                  */
#define MPCQP_TR_OFFSET 3        /* d; the ground is {p : n.p = d}                                          */
#define MPCQP_TR_MU 4            /* friction coefficient (mpcqp_plant_params.mu is not read)                */
#define MPCQP_TR_SIZE 8          /* 5 used, padded to a multiple of 4 doubles                               */

/* mpcqp_plant_step_wrench_device on the ground of a terrain row.  d_terrain == NULL is
 * mpcqp_plant_step_wrench_device, bit for bit (and with d_wrench == NULL too, mpcqp_plant_step_device).  With
 *     hgt(p) = ((n0 p0 + n1 p1) + n2 p2) - d,    dot(n, v) = (n0 v0 + n1 v1) + n2 v2
 * (contraction off, as everywhere in the plant) exactly four places of the model change and nothing else does:
 *   1. fresh slot       a foot is held iff hgt(foot) <= 0, and a held foot is put on the plane,
 *                       foot_k = foot_k - hgt n_k.
 *   2. ground reaction  with f = -R J^-T tau and fn = dot(n, f): a leg whose fn < 0 lets go.  Otherwise
 *                       t_k = f_k - fn n_k, ft = sqrt((t0^2 + t1^2) + t2^2), lim = mu fn with the row's mu,
 *                       sc = ft > lim ? lim / ft : 1, and f_k = fn n_k + sc t_k.
 *   3. touchdown        a swing foot lands iff hgt(foot) <= 0 && dot(n, v_foot) < 0, and is then put on the
 *                       plane as in 1.
 *   4. fallen           status 2.0 iff hgt(pos) < min_height.
 * The level row n = (0, 0, 1), d = 0, mu = pp->mu gives what the flat ground gives up to the sign of zeros.
 * Unchanged: a held foot does not slip, and MPCQP_PL_FOOT_FORCE is still the world f_z of a held foot, which
 * the controller's contact detection thresholds; on the slopes this is meant for (up to 0.3 rad) the cosine
 * between f_z and the normal force is >= 0.95.  The row is read once per tick and held over its substeps.
 *   The robot's row: with d_episode_state [batch][MPCQP_ES_SIZE] (the episode stage's slot, read only), robot b
 * takes row (int) d_episode_state[b][MPCQP_ES_POOL]: the terrain table is parallel to the episode pool, so a
 * robot's ground restarts with its start pose, and MPCQP_EL_POOL of a log row names the ground the episode ran
 * on.  With d_episode_state == NULL robot b takes row b, and terrain_rows >= batch is required.  A non-finite
 * terrain row, or a row index outside [0, terrain_rows), is treated like a non-finite torque row: 3.0 in
 * MPCQP_PT_STATUS and nothing else written that tick, and nothing is read outside the table.
 *   MPCQP_ERR_INVALID_ARG, and nothing launched: what mpcqp_plant_step_device rejects; with d_terrain,
 * terrain_rows < 1, or terrain_rows < batch without d_episode_state.
 * Left out: foot slip, trunk-ground contact (uneven ground is mpcqp_plant_step_field_device's).  The episode stage's height envelope
 * (height_min / height_max) stays the world z of the trunk, so a long walk uphill leaves it by height_max:
 * a caller who walks robots on slopes widens the bounds.                                                    */
int32_t mpcqp_plant_step_terrain_device(const mpcqp_plant_params* pp, double dt, const double* d_joint_torques,
                                        const double* d_wrench, const double* d_terrain, int32_t terrain_rows,
                                        const double* d_episode_state, int32_t batch, double* d_plant_state,
                                        const double* d_plant_init, double* d_sensors, double* d_plan_in,
                                        double* d_states, double* d_tq_records, double* d_plant_out, void* stream);

/* ---- bilinear height-field ground: steps, stairs, rough terrain.  A tile is a grid of heights H[ny][nx], x the
 * fast index, node (i, j) at (x0 + i cell, y0 + j cell).  The tiles of a call lie in one array
 * d_heights [heights_len]; the header rows d_field [field_rows][MPCQP_HF_SIZE] describe them.  Several header rows
 * may name the same MPCQP_HF_OFFSET (many start poses on one tile), and tiles may differ in size.             */
#define MPCQP_HF_X0 0            /* world x of node column 0                                                */
#define MPCQP_HF_Y0 1            /* world y of node row 0                                                   */
#define MPCQP_HF_CELL 2          /* node spacing, > 0                                                       */
#define MPCQP_HF_MU 3            /* friction coefficient (mpcqp_plant_params.mu is not read)                */
#define MPCQP_HF_NX 4            /* nodes along x, >= 2 (an integer held as a double, as NY and OFFSET)     */
#define MPCQP_HF_NY 5            /* nodes along y, >= 2                                                     */
#define MPCQP_HF_OFFSET 6        /* index of H[0][0] in d_heights                                           */
#define MPCQP_HF_SIZE 8          /* 7 used, padded to a multiple of 4 doubles                               */

/* mpcqp_plant_step_wrench_device on the ground of a height field.  d_field == NULL is
 * mpcqp_plant_step_wrench_device, bit for bit.  The lookup at a world point p (contraction off):
 *     u = (p_x - x0) / cell,  i = floor(u) clamped to [0, nx - 2],  fu_raw = u - i,  fu = min(max(fu_raw, 0), 1)
 * and v, j, fv likewise along y; h00 = H[j][i], h10 = H[j][i+1], h01 = H[j+1][i], h11 = H[j+1][i+1];
 *     a = h00 + fu (h10 - h00),  b = h01 + fu (h11 - h01),  h = a + fv (b - a)
 *     gx = ((h10 - h00) + fv ((h11 - h01) - (h10 - h00))) / cell      (0 where fu_raw < 0 or fu_raw > 1)
 *     gy = (b - a) / cell                                             (0 where fv_raw < 0 or fv_raw > 1)
 *     s = sqrt((gx^2 + gy^2) + 1),  n = (-gx / s, -gy / s, 1 / s),  hgt(p) = (p_z - h) n_z.
 * The ground continues flat beyond a tile's border.  The clamp of i and j is made on the double, before the
 * conversion to an integer: no address outside the tile is formed for any p, finite or not.  hgt is the
 * first-order normal distance; on a tile sampled from a plane it is the plane's own hgt, so the terrain entry
 * cross-checks this one.  With each point's own hgt and n the four places of the terrain entry read:
 *   1. fresh slot       a foot is held iff hgt(foot) <= 0, and a held foot is put at foot - hgt n.
 *   2. ground reaction  fn = dot(n, f) with n at the held foot (a held foot keeps its position, so its normal is
 *                       constant while it is held); the let-go rule and the cone scaling as on the plane, with
 *                       the header row's mu.
 *   3. touchdown        a swing foot lands iff hgt(foot) <= 0 && dot(n, v_foot) < 0, and is then put on the
 *                       surface as in 1.
 *   4. fallen           status 2.0 iff hgt(pos) < min_height, with h and n under the trunk.
 * Unchanged: a held foot does not slip; MPCQP_PL_FOOT_FORCE is the world f_z; the row is chosen once per tick, as
 * the terrain row is (robot b takes row (int) d_episode_state[b][MPCQP_ES_POOL], or row b without an episode
 * slot); the episode stage's height envelope stays the world z, so a caller who climbs stairs widens it.
 *   A bad row is treated like a non-finite torque row: 3.0 in MPCQP_PT_STATUS, nothing else written that tick,
 * nothing read outside the two arrays, and the robot carries on at the next good row.  A row is bad when its
 * index is outside [0, field_rows), when a header entry is non-finite, or when cell <= 0, nx < 2, ny < 2,
 * OFFSET < 0 or OFFSET + nx ny > heights_len.  The heights themselves are not checked on the device: a
 * non-finite height gives non-finite results for the robots that step on it.  The host packer
 * (mpcqp.pack_height_field) rejects non-finite heights.
 *   MPCQP_ERR_INVALID_ARG, and nothing launched: what mpcqp_plant_step_wrench_device rejects; with d_field,
 * field_rows < 1, field_rows < batch without d_episode_state, d_heights == NULL, or heights_len < 4.
 * Left out: overhangs, a riser's vertical face as anything but one steep cell (a step is a cell-wide ramp), foot
 * slip, trunk-ground contact.                                                                               */
int32_t mpcqp_plant_step_field_device(const mpcqp_plant_params* pp, double dt, const double* d_joint_torques,
                                      const double* d_wrench, const double* d_field, int32_t field_rows,
                                      const double* d_heights, int32_t heights_len, const double* d_episode_state,
                                      int32_t batch, double* d_plant_state, const double* d_plant_init,
                                      double* d_sensors, double* d_plan_in, double* d_states, double* d_tq_records,
                                      double* d_plant_out, void* stream);

/* The stage is stateless: every draw is a function of the Philox key `seed`, the robot index, and
 * MPCQP_ES_EPISODE / MPCQP_ES_TICK of the robot's episode slot, which it only reads.  So a restart needs no
 * zero-fill, and the host can recompute what any logged episode was subjected to.  Philox4x32-10 with
 * key = seed[0], seed[1] and counter = (robot, episode, stream, index); the episode stage's own draw is stream
 * 0, index 0.  With the output words w0..w3, u(w) = (w + 0.5) 2^-32 in (0, 1) and s(w) = (w + 0.5) 2^-31 - 1 in
 * (-1, 1), both exact, and t = MPCQP_ES_TICK, a robot in phase 1 gets:
 *   load     (stream 1, index 0; once per episode) the downward force m g, m = load_mass_max u(w0), g = gravity,
 *            computed as (load_mass_max u(w0)) gravity, at the body point load_point[i] s(w_{i+1}); force slot 1
 *            of the wrench row is (0, 0, 0 - m g).  The payload's weight only, not its inertia.
 *   biases   (stream 1, index 1 and 2; once per episode) bias_acc s(w_i) and bias_gyro s(w_i), i = 0..2.
 *   push     (stream 2, index k) if push_interval > 0 and t >= push_start: r = t - push_start, window
 *            k = r / push_interval, jitter = (uint64(w0) (push_interval - push_duration + 1)) >> 32; the push is
 *            active while jitter <= r % push_interval < jitter + push_duration, so a window holds one push and
 *            pushes never overlap.  Magnitude push_force[0] + (push_force[1] - push_force[0]) u(w1); direction
 *            row (uint64(w2) dir_count) >> 32 of d_dirs [dir_count][4], unit vectors in the world frame that the
 *            host builds (no trigonometry runs here); application point (stream 3, index k)
 *            push_point[i] s(w_i).  Force slot 0 of the wrench row is magnitude * direction at that point while
 *            the push is active, and zero otherwise.
 *   noise    (stream 16 + j, index t, j = 0..29 over the sensor doubles MPCQP_SN_JOINT_POS + j: 12 joint
 *            angles, 12 joint rates, imu_acc, imu_ang_vel) z = ((u(w0) + u(w1)) + (u(w2) + u(w3))) - 2, an
 *            Irwin-Hall variate of variance 1/3, so no log, sin or cos is needed; d = (sigma 1.7320508075688772) z
 *            for a joint value and bias + (sigma 1.7320508075688772) z for an IMU value, sigma the value's group
 *            (MPCQP_DS_*); the noisy value is clean + d, and the clean value's own bits when d == 0.  Written out
 *            of place: d_sensors is read, d_sensors_noisy written, the quaternion and the pad copied.  The clean
 *            row stays what the plant wrote (the episode stage's energy keeps reading the truth, and a robot
 *            whose plant tick wrote nothing is not noised twice).
 * A robot whose phase is not 1 (fresh or priming) gets a zero wrench row, a zero output row and a plain copy of
 * its sensor row.  Integer and binary64 multiplies and adds only, not contracted, no libm call, in the
 * statement order of tests/disturb_reference.py: the two agree bitwise.
 * Left out: noise on the quaternion and on MPCQP_PL_FOOT_FORCE (the plant writes the foot force in place and two
 * stages read it), the payload's inertia, per-robot plant mass, foot slip.  (Per-robot friction and inclined
 * ground are rows of mpcqp_plant_step_terrain_device, chosen per episode through the pool index, not drawn
 * here; uneven ground is the tiles of mpcqp_plant_step_field_device.)                                        */
#define MPCQP_DS_JOINT_POS 0     /* indices of mpcqp_disturb_params.sigma                                  */
#define MPCQP_DS_JOINT_VEL 1
#define MPCQP_DS_IMU_ACC 2
#define MPCQP_DS_IMU_ANG_VEL 3
typedef struct mpcqp_disturb_params {
  double load_mass_max;    /* kg; the payload's mass is uniform in (0, load_mass_max).  0                    */
  double gravity;          /* 9.81                                                                         */
  double load_point[3];    /* half-extents of the box, body frame, the payload's point is drawn from.  0    */
  double bias_acc;         /* IMU biases, uniform in (-bias, bias) per axis.  0                             */
  double bias_gyro;
  double push_force[2];    /* N, lowest and highest push magnitude.  0, 0                                   */
  double push_point[3];    /* half-extents of the box the push's application point is drawn from.  0        */
  double sigma[4];         /* standard deviations of the noise, per group MPCQP_DS_*.  0                    */
  uint32_t seed[2];        /* the Philox key (the episode stage's, for one stream of draws per fleet)       */
  int32_t push_start;      /* first episode tick of window 0.  0                                           */
  int32_t push_interval;   /* ticks per window; 0: no pushes.  0                                           */
  int32_t push_duration;   /* ticks per push, 1 .. push_interval.  1                                       */
  int32_t dir_count;       /* rows of d_dirs.  0                                                           */
} mpcqp_disturb_params;

void mpcqp_disturb_default_params(mpcqp_disturb_params* p); /* everything off */
int32_t mpcqp_disturb_params_size(void);  /* sizeof(mpcqp_disturb_params), for bindings */

/* Optional output row d_disturb_out [batch][MPCQP_DO_SIZE]: what the robot was subjected to this tick. */
#define MPCQP_DO_PUSH_ACTIVE 0   /* 1.0 while a push acts                                                  */
#define MPCQP_DO_PUSH_WINDOW 1   /* k; this and the next three describe the window's push, active or not,  */
#define MPCQP_DO_PUSH_FORCE 2    /* its magnitude                 and are 0 before push_start / without pushes */
#define MPCQP_DO_PUSH_DIR 3      /* its row of d_dirs                                                      */
#define MPCQP_DO_PUSH_POINT 4    /* [3] its application point                                              */
#define MPCQP_DO_LOAD_POINT 7    /* [3] the payload's point                                                */
#define MPCQP_DO_LOAD_FORCE 10   /* the payload's weight m g (the wrench row holds 0 - m g in z)           */
#define MPCQP_DO_BIAS_ACC 11     /* [3]                                                                    */
#define MPCQP_DO_BIAS_GYRO 14    /* [3]                                                                    */
#define MPCQP_DO_SIZE 20         /* 17 used, padded to a multiple of 4 doubles                             */

/* The stage's buffers (DEVICE pointers).  d_sensors and d_sensors_noisy may both be NULL (a truth-fed tick:
 * pushes and load only), d_dirs may be NULL when push_interval == 0, d_disturb_out may be NULL.             */
typedef struct mpcqp_disturb_buffers {
  const double* d_episode_state; /* [batch][MPCQP_ES_SIZE]  MPCQP_ES_PHASE, _TICK, _EPISODE read; a stand-alone
                                    caller hands a hand-made row                                           */
  double* d_wrench;              /* [batch][MPCQP_PW_SIZE]  written                                        */
  const double* d_sensors;       /* [batch][MPCQP_SN_SIZE]  read                                           */
  double* d_sensors_noisy;       /* [batch][MPCQP_SN_SIZE]  written; must not be d_sensors                 */
  const double* d_dirs;          /* [dir_count][4]          x, y, z, 0                                     */
  double* d_disturb_out;         /* [batch][MPCQP_DO_SIZE]  written                                        */
} mpcqp_disturb_buffers;
int32_t mpcqp_disturb_buffers_size(void); /* sizeof(mpcqp_disturb_buffers), for bindings */

/* One disturbance tick for `batch` robots (DEVICE pointers, async on `stream`, no allocation and no
 * synchronization: hipGraph-capture safe; one kernel).  Chain it first in the tick, and give the plant stage
 * d_wrench through mpcqp_plant_step_wrench_device.  The structs are read when the call is made.
 * MPCQP_ERR_INVALID_ARG, and nothing launched: a NULL episode slot or wrench row; one of d_sensors /
 * d_sensors_noisy without the other, or the two equal; push_interval < 0; with push_interval > 0,
 * push_duration outside 1 .. push_interval, push_start < 0, d_dirs NULL or dir_count < 1.                    */
int32_t mpcqp_disturb_device(const mpcqp_disturb_params* dp, const mpcqp_disturb_buffers* buf, int32_t batch,
                             void* stream);

const char* mpcqp_status_str(int32_t status);
const char* mpcqp_error_str(int32_t err);
/* Last HIP error string recorded by the handle (for MPCQP_ERR_HIP). */
const char* mpcqp_last_error(mpcqp_handle* h);

#ifdef __cplusplus
}
#endif
#endif /* MPCQP_H_ */
