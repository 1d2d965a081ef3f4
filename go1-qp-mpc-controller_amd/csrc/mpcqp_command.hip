// mpcqp_command.hip — the command stage of the control tick, batched on the device: the joystick command
// block at the top of main_update (src/a1_cpp/src/GazeboA1ROS.cpp:122-188; the same block is
// HardwareA1ROS.cpp:104-158).  Per robot and per tick, in the reference's statement order:
//   body height and its clamp                        :124-130
//   prev_joy_cmd_ctrl_state, the walk / stand toggle :140-147
//   root_lin_vel_d, root_ang_vel_d                   :150-157
//   root_euler_d += rate * dt, root_pos_d[2]         :158-161
//   movement_mode and the leave-walking lock         :164-176
//   the walking-mode position lock of kp_linear      :179-188
// The members the block keeps between ticks (joy_cmd_body_height, joy_cmd_ctrl_state,
// prev_joy_cmd_ctrl_state, kp_linear) live in a per-robot slot (MPCQP_CS_*); root_euler_d and root_pos_d
// live in the caller's MPCQP_ST_* row and are updated in place.
//
// One thread per robot: about 25 doubles moved per robot, launch-bound like plan_kernel.  The command row
// and the slot are 64-byte rows read and written as double2; the state-row fields the stage touches are
// offsets 21..32 of a 512-byte row.  Contraction is off, so a += b * dt is a multiply and an add and the
// stage is bitwise tests/command_reference.py.
#pragma clang fp contract(off)

#include "mpcqp_internal.h"

namespace mpcqp {
namespace cmd {

static_assert(MPCQP_CM_SIZE == 8 && MPCQP_CS_SIZE == 8, "rows are read as four double2");
static_assert(MPCQP_CM_VEL == 0 && MPCQP_CM_RATE == 3 && MPCQP_CM_MODE_REQUEST == 6, "command row layout");
static_assert(MPCQP_CS_INIT == 0 && MPCQP_CS_BODY_HEIGHT == 1 && MPCQP_CS_CTRL_STATE == 2 &&
                  MPCQP_CS_PREV_CTRL_STATE == 3 && MPCQP_CS_KP_LINEAR == 4,
              "command slot layout");

__global__ __launch_bounds__(256) void command_kernel(const mpcqp_command_params cp, const double dt,
                                                      double* __restrict__ cmds, double* __restrict__ states,
                                                      double* __restrict__ plan_in, const int batch,
                                                      double* __restrict__ slots) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= batch) return;
  double2* crow = reinterpret_cast<double2*>(cmds + (size_t)MPCQP_CM_SIZE * b);
  double2* srow = reinterpret_cast<double2*>(slots + (size_t)MPCQP_CS_SIZE * b);
  double* st = states + (size_t)MPCQP_ST_SIZE * b;
  const double2 c0 = crow[0], c1 = crow[1], c2 = crow[2], c3 = crow[3];
  const double velx = c0.x, vely = c0.y, velz = c1.x;
  const double roll_rate = c1.y, pitch_rate = c2.x, yaw_rate = c2.y, request = c3.x;
  if (!(isfinite(velx) && isfinite(vely) && isfinite(velz) && isfinite(roll_rate) && isfinite(pitch_rate) &&
        isfinite(yaw_rate) && isfinite(request))) {
    // the solve reports the robot (MPCQP_STATUS_NAN_INPUT); nothing that persists is touched
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    st[MPCQP_ST_LIN_VEL_D] = nan;
    st[MPCQP_ST_LIN_VEL_D + 1] = nan;
    st[MPCQP_ST_LIN_VEL_D + 2] = nan;
    return;
  }
  const double2 s0 = srow[0], s1 = srow[1], s2 = srow[2], s3 = srow[3];
  const bool fresh = s0.x == 0.0;
  double height = fresh ? cp.body_height_init : s0.y;
  double state = fresh ? 0.0 : s1.x;
  double kp0 = fresh ? cp.kp_linear[0] : s2.x;
  double kp1 = fresh ? cp.kp_linear[1] : s2.y;
  const double kp2 = fresh ? cp.kp_linear[2] : s3.x;

  // body height (:124-130)
  height = height + velz * dt;
  if (height >= cp.body_height_max) height = cp.body_height_max;
  if (height <= cp.body_height_min) height = cp.body_height_min;
  // the toggle (:140-147)
  const double prev = state;
  if (request != 0.0) state = state == 0.0 ? 1.0 : 0.0;  // (joy_cmd_ctrl_state + 1) % 2
  // movement mode and the two locks (:164-188)
  const bool walk = state == 1.0;
  const bool leave = !walk && prev == 1.0;
  bool refresh = leave;
  if (leave) {
    kp0 = cp.kp_linear_lock_x;
    kp1 = cp.kp_linear_lock_y;
  }
  if (walk) {
    if (sqrt(velx * velx + vely * vely) > cp.vel_lock_threshold) {
      refresh = true;
      kp0 = 0.0;
      kp1 = 0.0;
    } else {
      kp0 = cp.kp_linear_lock_x;
      kp1 = cp.kp_linear_lock_y;
    }
  }

  // the state row: root_euler_d (:158-160), root_pos_d (:161, :171, :182), root_ang_vel_d (:155-157),
  // root_lin_vel_d (:150-152): offsets 21 .. 32
  const double e0 = st[MPCQP_ST_EULER_D], e1 = st[MPCQP_ST_EULER_D + 1], e2 = st[MPCQP_ST_EULER_D + 2];
  st[MPCQP_ST_EULER_D] = e0 + roll_rate * dt;
  st[MPCQP_ST_EULER_D + 1] = e1 + pitch_rate * dt;
  st[MPCQP_ST_EULER_D + 2] = e2 + yaw_rate * dt;
  if (refresh) {
    const double p0 = st[MPCQP_ST_POS], p1 = st[MPCQP_ST_POS + 1];
    st[MPCQP_ST_POS_D] = p0;
    st[MPCQP_ST_POS_D + 1] = p1;
  }
  st[MPCQP_ST_POS_D + 2] = height;
  st[MPCQP_ST_ANG_VEL_D] = roll_rate;
  st[MPCQP_ST_ANG_VEL_D + 1] = pitch_rate;
  st[MPCQP_ST_ANG_VEL_D + 2] = yaw_rate;
  st[MPCQP_ST_LIN_VEL_D] = velx;
  st[MPCQP_ST_LIN_VEL_D + 1] = vely;
  st[MPCQP_ST_LIN_VEL_D + 2] = velz;
  plan_in[(size_t)MPCQP_PL_SIZE * b + MPCQP_PL_MOVEMENT_MODE] = walk ? 1.0 : 0.0;
  // the request is consumed (:146); the padding double keeps what the caller left there
  crow[3] = make_double2(0.0, c3.y);
  srow[0] = make_double2(1.0, height);
  srow[1] = make_double2(state, prev);
  srow[2] = make_double2(kp0, kp1);
  srow[3] = make_double2(kp2, s3.y);
}

}  // namespace cmd

hipError_t launch_command(const mpcqp_command_params& cp, double dt, double* cmds, double* states, double* plan_in,
                          int batch, double* slots, void* stream) {
  hipLaunchKernelGGL(cmd::command_kernel, dim3((batch + 255) / 256), dim3(256), 0, (hipStream_t)stream, cp, dt, cmds,
                     states, plan_in, batch, slots);
  return hipGetLastError();
}

}  // namespace mpcqp
