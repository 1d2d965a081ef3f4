"""One fused control tick for a fleet of robots, entirely on the device:

    raw *CtrlStates rows --assemble--> MPC records --warm solve--> mpcqp_result --torque map--> tau

i.e. the MPC branch of A1RobotControl::compute_grf (A1RobotControl.cpp:446-561, with the
persistent warm-started solver of A1RobotControl.h:67) followed by compute_joint_torques
(:289-319), three kernels on one stream with no host round trip.  ``capture()`` records the tick
as a HIP graph (torch.cuda.CUDAGraph is hipGraph on ROCm), so a simulator steps with one replay.
torch is used only to own device buffers and the capture stream.

With ``plan`` (a PlanParams) the tick starts one stage earlier, with the leg plan (update_plan,
generate_swing_legs_ctrl and the terrain adaptation of compute_grf, A1RobotControl.cpp:148-287,
:335-376): it fills the contacts, the swing-leg force and root_euler_d[1] of ``states`` /
``tq_records`` on the device from ``plan_in``.

With ``estimator`` (an EstimatorParams) it starts another stage earlier, with the state front end (pose
and IMU callbacks, GazeboA1ROS.cpp:242-307, and A1BasicEKF::update_estimation, A1BasicEKF.cpp:55-164):
root_euler, root_pos, root_ang_vel, root_lin_vel, root_rot_mat and foot_pos_abs of ``states``,
root_rot_mat_z of ``plan_in`` and j_foot of ``tq_records`` are computed on the device from ``sensors``
(quaternion, joint angles and rates, IMU sample) and the foot forces of ``plan_in``, so the caller writes
only sensor-level state.  The estimator runs before the plan: the plan and the solve see this tick's estimate.

With ``command`` (a CommandParams) it starts with the command stage (the joystick command block of
main_update, GazeboA1ROS.cpp:122-188): the desired velocities, root_euler_d, root_pos_d and movement_mode
of ``states`` / ``plan_in`` and the position-locked kp_linear of ``cmd_state`` are computed on the device
from the joystick-level rows ``cmd``.  It runs first, as in the reference: the estimator sees this tick's
movement_mode, and the position lock reads the previous tick's root_pos.

With ``control_type`` each robot takes the stance_leg_control_type branch of its own (A1RobotControl.cpp:377
QP balance controller, :446 MPC): the tick assembles both kinds of record and runs the balance solve of the
type-0 robots and the warm MPC solve of the type-1 robots into the one ``results`` buffer, so the stage order
is command -> estimate -> plan -> assemble (MPC and balance) -> balance solve -> warm MPC solve -> torque map.

With ``policy`` (a Policy) the tick ends with the policy stage, the reference's third controller (the Go1 RL
policy and its servo stand, src/go1_rl_ctrl_cpp/src/Go1RLController.cpp:78-166): after the torque map has run
for every robot, the stage overwrites the ``torques`` row of the robots whose control type is 2 from ``sensors``,
``states``, ``plan_in`` and ``cmd``.  Robots of type 0 and 1 are untouched by it.

With ``plant`` (a PlantParams) the tick ends with the plant stage, which the reference left to Gazebo: a
rigid-body model (single trunk, massless stance legs, joint-space swing legs, flat ground) moves every robot
one control period on under the final ``torques`` row and writes the next tick's ``sensors`` and foot forces,
so T replays are a T-tick closed-loop rollout with no host write in between.  Without ``estimator`` it also
writes the ground truth of the estimator's fields into ``states`` / ``plan_in`` / ``tq_records``.

With ``episode`` (an EpisodeParams; needs ``plant``) the tick ends with the episode stage: per robot it accumulates
the episode's metrics, ends the episode on a plant status, the envelope or the time-out, writes it into
``episode_log`` / ``episode_totals`` and restarts the robot over two ticks from a row of ``episode_pool`` drawn on
the device, under one of ``episode_scripts``, so T replays are a Monte-Carlo evaluation of the fleet.

With ``disturb`` (a DisturbParams; needs ``plant`` and ``episode``) the tick starts with the disturbance stage: per
robot it draws this tick's push, the weight of the episode's payload and the sensor noise with the episode's IMU
biases, all functions of the seed, the robot and the episode slot's episode index and tick.  The plant applies
``wrench``; the estimator and the policy stage read ``sensors_noisy``, while the plant keeps writing, and the
episode stage keeps reading, the clean ``sensors``.
"""
from . import _lib
from .balance import assemble_balance_device, default_balance_gains
from .command import command_device, command_state_size
from .disturb import DO_SIZE, PW_SIZE, DisturbParams, disturb_buffers, disturb_device, plant_step_wrench_device
from .episode import (EL_SIZE, ET_SIZE, POOL_INIT, POOL_SIZE, SEG_SIZE, EpisodeParams, episode_buffers, episode_device,
                      episode_state_size)
from .estimator import estimator_state_size, state_estimate_device
from .legplan import leg_plan_device, leg_plan_typed_device, plan_state_size
from .plant import plant_state_size, plant_step_device
from .policy import policy_device, policy_state_size
from .solver import MpcQpSolver
from .torques import joint_torques_device


class ControlTick:
    def __init__(self, batch, params=None, device=0, plan=None, dt=None, estimator=None, command=None,
                 control_type=None, balance=None, gains=None, policy=None, plant=None, plant_init=None,
                 episode=None, episode_pool=None, episode_scripts=None, episode_log_len=4, disturb=None,
                 disturb_dirs=None):
        """control_type: None = the MPC-only tick; 0 / 1 = every robot takes the balance / the MPC branch;
        2 (with ``policy``) = every robot takes the policy branch;
        "per_robot" = the tick owns ``self.control_type``, an int32 [B] device tensor the caller writes
        (initialised to 1) and every kernel reads when it runs, so a replayed graph follows it.  A robot whose
        type is neither 0 nor 1 is solved by neither branch and keeps its previous ``results`` row.
        ``balance`` (BalanceParams) and ``gains`` (BalanceGains) default to the reference's.
        ``policy`` (a Policy; needs control_type "per_robot" or 2): robots of type 2 get their torques from the
        policy stage.  The tick then owns ``policy_state`` and ``policy_out``, and ``sensors`` / ``cmd`` exist
        even without ``estimator`` / ``command`` and are then caller-written.
        ``plant`` (a PlantParams): the tick ends with the plant stage and owns ``plant_state``, ``plant_out`` and
        ``plant_init`` (from the rows ``plant_init`` [B, PI_SIZE], or None: the default stance); the caller then
        writes commands and desired values only.  Zeroing a robot's rows of ``plant_state`` and of the
        controller's slots resets it.
        ``episode`` (an EpisodeParams; needs ``plant`` and ``episode_pool``, rows [P, POOL_SIZE] of
        pack_episode_pool): the tick ends with the episode stage and owns ``episode_state``, ``episode_log``
        [B, episode_log_len, EL_SIZE], ``episode_totals``, ``episode_pool``, ``episode_scripts`` (from
        pack_episode_scripts, or None) and ``plant_init`` (pool row 0 until the first draw, unless ``plant_init``
        is given).  Every robot starts fresh, so neither ``plant_init`` nor ``prime_plant()`` is needed: tick 1
        draws, tick 2 primes, tick 3 is episode tick 0.  The counts, ``dt`` and ``log_len`` of the params are
        set by the tick.
        ``disturb`` (a DisturbParams; needs ``plant`` and ``episode``; ``disturb_dirs``, rows [D, 4] of
        pack_push_dirs, when it pushes): the tick starts with the disturbance stage and owns ``wrench``,
        ``disturb_out`` and, when it has ``sensors``, ``sensors_noisy``, which the estimator and the policy stage
        then read.  ``dir_count`` of the params is set by the tick; the seed is the params' own.  With the
        default (all-off) params every buffer is bitwise that of the tick without ``disturb``."""
        import torch
        self.torch = torch
        self.B = int(batch)
        self.solver = MpcQpSolver(params if params is not None else _lib.default_params(10), device=device)
        self.solver.reserve(self.B)
        N = self.solver.horizon
        dev = f"cuda:{device}"
        f64 = dict(dtype=torch.float64, device=dev)
        self.states = torch.zeros((self.B, _lib.ST_SIZE), **f64)        # caller writes robot states here
        self.tq_records = torch.zeros((self.B, _lib.TQ_SIZE), **f64)    # and Jacobians / swing forces here
        self.records = torch.zeros((self.B, _lib.rec_size(N)), **f64)
        self.warm = torch.zeros((self.B, self.solver.warm_state_size), **f64)
        self.results = torch.zeros((self.B, _lib.RESULT_DOUBLES), **f64)
        self.counter = torch.zeros((self.B,), dtype=torch.int32, device=dev)
        self.torques = torch.zeros((self.B, 12), **f64)
        self.plan = plan
        if plan is not None:
            self.dt = float(plan.control_dt if dt is None else dt)  # update_plan's dt argument
            self.plan_in = torch.zeros((self.B, _lib.PL_SIZE), **f64)   # caller writes rot_z / foot_force / mode
            self.plan_state = torch.zeros((self.B, plan_state_size()), **f64)  # zero = reset() controller
            self.plan_out = torch.zeros((self.B, _lib.PO_SIZE), **f64)
        self.estimator = estimator
        if estimator is not None:
            if plan is None:
                if dt is None:
                    raise ValueError("ControlTick(estimator=...) without plan= needs dt")
                self.dt = float(dt)  # update_estimation's dt argument
                self.plan_in = torch.zeros((self.B, _lib.PL_SIZE), **f64)  # caller writes foot_force / mode
            self.sensors = torch.zeros((self.B, _lib.SN_SIZE), **f64)    # caller writes quat / joints / IMU here
            self.est_state = torch.zeros((self.B, estimator_state_size()), **f64)  # zero = not initialized
            self.est_out = torch.zeros((self.B, _lib.EO_SIZE), **f64)
        self.command = command
        if command is not None:
            if plan is None and estimator is None:
                if dt is None:
                    raise ValueError("ControlTick(command=...) without plan= needs dt")
                self.dt = float(dt)  # main_update's dt argument
                self.plan_in = torch.zeros((self.B, _lib.PL_SIZE), **f64)  # movement_mode is written here
            self.cmd = torch.zeros((self.B, _lib.CM_SIZE), **f64)       # caller writes joystick-level commands here
            self.cmd_state = torch.zeros((self.B, command_state_size()), **f64)  # zero = fresh
        if control_type not in (None, 0, 1, "per_robot") and not (control_type == 2 and policy is not None):
            raise ValueError('control_type must be None, 0, 1 or "per_robot" (or 2 with policy=)')
        if policy is not None and control_type not in ("per_robot", 2):
            raise ValueError('ControlTick(policy=...) needs control_type="per_robot" or 2')
        self.typed = control_type is not None
        if self.typed:
            self.control_type = torch.full((self.B,), 1 if control_type == "per_robot" else int(control_type),
                                           dtype=torch.int32, device=dev)
            self.balance = balance if balance is not None else _lib.default_balance_params()
            self.gains = gains if gains is not None else default_balance_gains()
            self.bal_records = torch.zeros((self.B, _lib.BAL_SIZE), **f64)
            if not hasattr(self, "plan_in"):
                self.plan_in = torch.zeros((self.B, _lib.PL_SIZE), **f64)  # caller writes rot_z here
        self.policy = policy
        if policy is not None:
            if estimator is None:
                self.sensors = torch.zeros((self.B, _lib.SN_SIZE), **f64)  # caller writes joints / IMU rate here
            if command is None:
                self.cmd = torch.zeros((self.B, _lib.CM_SIZE), **f64)      # caller writes the joystick velocities
            self.policy_state = torch.zeros((self.B, policy_state_size()), **f64)  # zero = fresh
            self.policy_out = torch.zeros((self.B, _lib.PY_SIZE), **f64)
        self.plant = plant
        if plant is not None:
            if not hasattr(self, "dt"):
                if dt is None:
                    raise ValueError("ControlTick(plant=...) without plan= / estimator= / command= needs dt")
                self.dt = float(dt)  # the plant's control period
            if not hasattr(self, "plan_in"):
                self.plan_in = torch.zeros((self.B, _lib.PL_SIZE), **f64)  # the foot forces are written here
            self.plant_state = torch.zeros((self.B, plant_state_size()), **f64)  # zero = fresh
            self.plant_out = torch.zeros((self.B, _lib.PT_SIZE), **f64)
            self.plant_init = None
            if plant_init is not None:
                rows = torch.as_tensor(plant_init, dtype=torch.float64).reshape(self.B, _lib.PI_SIZE)
                self.plant_init = rows.to(dev).contiguous()
        self.episode = None
        if episode is not None:
            if plant is None or episode_pool is None:
                raise ValueError("ControlTick(episode=...) needs plant= and episode_pool=")
            pool = torch.as_tensor(episode_pool, dtype=torch.float64).reshape(-1, POOL_SIZE)
            ep = EpisodeParams.from_buffer_copy(episode)
            ep.dt, ep.pool_count, ep.log_len = self.dt, pool.shape[0], int(episode_log_len)
            ep.script_count = ep.script_segments = 0
            self.episode_pool = pool.to(dev).contiguous()
            self.episode_scripts = None
            if episode_scripts is not None:
                sc = torch.as_tensor(episode_scripts, dtype=torch.float64)
                sc = sc.reshape(sc.shape[0], -1, SEG_SIZE)
                ep.script_count, ep.script_segments = sc.shape[0], sc.shape[1]
                self.episode_scripts = sc.to(dev).contiguous()
            if self.plant_init is None:
                self.plant_init = self.episode_pool[:1, POOL_INIT:POOL_INIT + _lib.PI_SIZE].repeat(self.B, 1)
            self.episode_state = torch.zeros((self.B, episode_state_size()), **f64)  # zero = fresh
            self.episode_log = torch.zeros((self.B, ep.log_len, EL_SIZE), **f64)
            self.episode_totals = torch.zeros((self.B, ET_SIZE), **f64)
            ptr = lambda name: getattr(self, name).data_ptr() if getattr(self, name, None) is not None else 0
            size = lambda name: getattr(self, name).shape[1] if hasattr(self, name) else 0
            self.episode_buffers = episode_buffers(
                ptr("plant_out"), ptr("plant_state"), ptr("plant_init"), ptr("torques"), ptr("sensors"), ptr("cmd"),
                ptr("results"), ptr("episode_pool"), ptr("episode_scripts"), ptr("states"), ptr("counter"),
                ptr("episode_log"), ptr("episode_totals"), ptr("est_state"), size("est_state"), ptr("plan_state"),
                size("plan_state"), ptr("cmd_state"), size("cmd_state"), ptr("policy_state"), size("policy_state"),
                ptr("warm"), size("warm"))
            self.episode = ep
        self.disturb = None
        if disturb is not None:
            if plant is None or self.episode is None:
                raise ValueError("ControlTick(disturb=...) needs plant= and episode=")
            dp = DisturbParams.from_buffer_copy(disturb)
            self.disturb_dirs = None
            dp.dir_count = 0
            if disturb_dirs is not None:
                dirs = torch.as_tensor(disturb_dirs, dtype=torch.float64).reshape(-1, 4)
                dp.dir_count = dirs.shape[0]
                self.disturb_dirs = dirs.to(dev).contiguous()
            self.wrench = torch.zeros((self.B, PW_SIZE), **f64)
            self.disturb_out = torch.zeros((self.B, DO_SIZE), **f64)
            if hasattr(self, "sensors"):
                self.sensors_noisy = torch.zeros((self.B, _lib.SN_SIZE), **f64)
            ptr = lambda name: getattr(self, name).data_ptr() if getattr(self, name, None) is not None else 0
            self.disturb_buffers = disturb_buffers(ptr("episode_state"), ptr("wrench"), ptr("sensors"),
                                                   ptr("sensors_noisy"), ptr("disturb_dirs"), ptr("disturb_out"))
            self.disturb = dp
        self.graph = None

    def step(self, stream=None, episode=True):
        """Enqueue one tick on `stream` (default: torch's current stream).  ``episode=False`` leaves the episode
        stage out, for a caller that reads the tick's rows before enqueueing it with ``episode_stage()``."""
        s = stream if stream is not None else self.torch.cuda.current_stream().cuda_stream
        if self.disturb is not None:
            self.disturb_stage(s)
        if self.command is not None:
            command_device(self.command, self.dt, self.cmd.data_ptr(), self.states.data_ptr(),
                           self.plan_in.data_ptr(), self.B, self.cmd_state.data_ptr(), s)
        if self.estimator is not None:
            state_estimate_device(self.estimator, self.dt, self._sensed().data_ptr(), self.plan_in.data_ptr(),
                                  self.states.data_ptr(), self.B, self.est_state.data_ptr(),
                                  self.tq_records.data_ptr(), self.est_out.data_ptr(), s)
        if self.typed:
            return self._step_typed(s, episode)
        if self.plan is not None:
            leg_plan_device(self.plan, self.dt, self.states.data_ptr(), self.plan_in.data_ptr(), self.B,
                            self.plan_state.data_ptr(), self.tq_records.data_ptr(), self.plan_out.data_ptr(), s)
        _lib.assemble_records_device(self.solver.horizon, self.states.data_ptr(), self.B, self.records.data_ptr(), s)
        self.solver.solve_warm_device(self.records.data_ptr(), self.B, self.warm.data_ptr(), self.results.data_ptr(),
                                      0, s)
        joint_torques_device(self.tq_records.data_ptr(), self.results.data_ptr(), self.B, self.counter.data_ptr(),
                             self.torques.data_ptr(), s)
        if self.plant is not None:
            self._step_plant(s)
        if self.episode is not None and episode:
            self.episode_stage(s)

    def disturb_stage(self, stream=None):
        """Enqueue the disturbance stage alone: first in the tick (``disturb_buffers``)."""
        s = stream if stream is not None else self.torch.cuda.current_stream().cuda_stream
        disturb_device(self.disturb, self.disturb_buffers, self.B, s)

    def _sensed(self):
        """The sensor row the controller's stages read: the noisy one with the disturbance stage."""
        return self.sensors_noisy if self.disturb is not None else self.sensors

    def episode_stage(self, stream=None):
        """Enqueue the episode stage alone: last in the tick, on whichever of the sensors, cmd and slot buffers
        the tick has (``episode_buffers``)."""
        s = stream if stream is not None else self.torch.cuda.current_stream().cuda_stream
        episode_device(self.episode, self.episode_buffers, self.B, self.episode_state.data_ptr(), s)

    def _step_plant(self, s):
        """The plant stage, last in the tick: the final ``torques`` row moves every robot one control period on.
        With the estimator it writes what sensors would deliver; without it, also the truth image of what the
        estimator would write."""
        truth = self.estimator is None
        rows = (self.B, self.plant_state.data_ptr(), self.plant_init.data_ptr() if self.plant_init is not None else 0,
                self.sensors.data_ptr() if hasattr(self, "sensors") else 0, self.plan_in.data_ptr(),
                self.states.data_ptr() if truth else 0, self.tq_records.data_ptr() if truth else 0,
                self.plant_out.data_ptr(), s)
        if self.disturb is not None:
            plant_step_wrench_device(self.plant, self.dt, self.torques.data_ptr(), self.wrench.data_ptr(), *rows)
        else:
            plant_step_device(self.plant, self.dt, self.torques.data_ptr(), *rows)

    def prime_plant(self, stream=None):
        """Enqueue the plant stage alone.  On fresh slots (after construction or a reset) it initialises them from
        ``plant_init`` and writes the rows of the start without integrating, so the first tick's estimator, plan
        and solve see the robot where it stands instead of zero rows.  (On a slot that is not fresh it is one
        more step under the current ``torques``.)"""
        self._step_plant(stream if stream is not None else self.torch.cuda.current_stream().cuda_stream)

    def _step_typed(self, s, episode=True):
        """plan -> both assemblies -> balance solve of the type-0 robots -> warm MPC solve of the type-1
        robots -> torque map -> policy stage of the type-2 robots; every kernel reads ``control_type`` when it
        runs."""
        ty = self.control_type.data_ptr()
        if self.plan is not None:
            leg_plan_typed_device(self.plan, self.dt, self.states.data_ptr(), self.plan_in.data_ptr(), self.B,
                                  self.plan_state.data_ptr(), self.tq_records.data_ptr(), self.plan_out.data_ptr(),
                                  ty, s)
        _lib.assemble_records_device(self.solver.horizon, self.states.data_ptr(), self.B, self.records.data_ptr(), s)
        assemble_balance_device(self.gains, self.states.data_ptr(), self.plan_in.data_ptr(),
                                self.cmd_state.data_ptr() if self.command is not None else 0, self.B,
                                self.bal_records.data_ptr(), s)
        self.solver.balance_solve_typed_device(self.balance, self.bal_records.data_ptr(), self.B, ty, 0,
                                               self.results.data_ptr(), s)
        self.solver.solve_warm_typed_device(self.records.data_ptr(), self.B, self.warm.data_ptr(), ty, 1,
                                            self.results.data_ptr(), 0, s)
        joint_torques_device(self.tq_records.data_ptr(), self.results.data_ptr(), self.B, self.counter.data_ptr(),
                             self.torques.data_ptr(), s)
        if self.policy is not None:
            policy_device(self.policy, self._sensed().data_ptr(), self.states.data_ptr(), self.plan_in.data_ptr(),
                          self.cmd.data_ptr(), self.B, self.policy_state.data_ptr(), self.torques.data_ptr(),
                          self.policy_out.data_ptr(), ty, 2, s)
        if self.plant is not None:
            self._step_plant(s)
        if self.episode is not None and episode:
            self.episode_stage(s)

    def capture(self):
        """Record step() as a graph.  Estimator, plan and warm slots, counters and torques keep evolving on replay,
        exactly as with eager steps; capture itself launches nothing.  The estimator and plan parameters and dt are
        kernel arguments, so the graph keeps the values they had at capture."""
        torch = self.torch
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            self.step()
        self.graph = g
        return g

    def replay(self):
        self.graph.replay()

    def close(self):
        self.solver.close()
