"""One fused control tick for a fleet of robots, entirely on the device:

    raw *CtrlStates rows --assemble--> MPC records --warm solve--> mpcqp_result --torque map--> tau

i.e. the MPC branch of A1RobotControl::compute_grf (A1RobotControl.cpp:446-561, with the
persistent warm-started solver of A1RobotControl.h:67) followed by compute_joint_torques
(:289-319), three kernels on one stream with no host round trip.  ``capture()`` records the tick
as a HIP graph (torch.cuda.CUDAGraph is hipGraph on ROCm), so a simulator steps with one replay.
torch is used only to own device buffers and the capture stream.

The constructor's options add stages around those three.  A tick is the ordered list

    disturb, command, estimate, plan, assemble, assemble_balance, balance, solve, torques, policy, plant, episode

of the stages its options switch on (``stages()``); ``step()`` walks it, and nothing else enqueues a tick.

disturb (``disturb``, a DisturbParams; needs ``plant`` and ``episode``): per robot this tick's push, the weight of
the episode's payload and the sensor noise with the episode's IMU biases, all functions of the seed, the robot and
the episode slot's episode index and tick.  The plant applies ``wrench``; the estimator and the policy stage read
``sensors_noisy``, while the plant keeps writing, and the episode stage keeps reading, the clean ``sensors``.

command (``command``, a CommandParams; the joystick command block of main_update, GazeboA1ROS.cpp:122-188): the
desired velocities, root_euler_d, root_pos_d and movement_mode of ``states`` / ``plan_in`` and the position-locked
kp_linear of ``cmd_state`` from the joystick-level rows ``cmd``.  Before the estimator, as in the reference: the
estimator sees this tick's movement_mode, and the position lock reads the previous tick's root_pos.

estimate (``estimator``, an EstimatorParams; pose and IMU callbacks, GazeboA1ROS.cpp:242-307, and
A1BasicEKF::update_estimation, A1BasicEKF.cpp:55-164): root_euler, root_pos, root_ang_vel, root_lin_vel,
root_rot_mat and foot_pos_abs of ``states``, root_rot_mat_z of ``plan_in`` and j_foot of ``tq_records`` from
``sensors`` (quaternion, joint angles and rates, IMU sample) and the foot forces of ``plan_in``, so the caller
writes only sensor-level state.  Before the plan: the plan and the solve see this tick's estimate.

plan (``plan``, a PlanParams; update_plan, generate_swing_legs_ctrl and the terrain adaptation of compute_grf,
A1RobotControl.cpp:148-287, :335-376): the contacts, the swing-leg force and root_euler_d[1] of ``states`` /
``tq_records`` from ``plan_in``.

assemble_balance, balance (``control_type``): each robot takes the stance_leg_control_type branch of its own
(A1RobotControl.cpp:377 QP balance controller, :446 MPC).  The tick assembles both kinds of record and runs the
balance solve of the type-0 robots and the warm MPC solve of the type-1 robots into the one ``results`` buffer.
Without ``control_type`` the plan and the solve get a null type pointer, which is the untyped entry point.

policy (``policy``, a Policy; the reference's third controller, the Go1 RL policy and its servo stand,
src/go1_rl_ctrl_cpp/src/Go1RLController.cpp:78-166): after the torque map has run for every robot, the stage
overwrites the ``torques`` row of the robots whose control type is 2 from ``sensors``, ``states``, ``plan_in`` and
``cmd``.  Robots of type 0 and 1 are untouched by it.

plant (``plant``, a PlantParams; what the reference left to Gazebo): a rigid-body model (single trunk, massless
stance legs, joint-space swing legs, flat ground, with ``terrain`` a per-robot inclined plane with its own
friction, or with ``field`` a bilinear height field) moves every robot one control period on under the final ``torques`` row and writes the next tick's ``sensors`` and foot forces, so T replays are a T-tick closed-loop
rollout with no host write in between.  Without ``estimator`` it also writes the ground truth of the estimator's
fields into ``states`` / ``plan_in`` / ``tq_records``.

episode (``episode``, an EpisodeParams; needs ``plant``): per robot it accumulates the episode's metrics, ends the
episode on a plant status, the envelope or the time-out, writes it into ``episode_log`` / ``episode_totals`` and
restarts the robot over two ticks from a row of ``episode_pool`` drawn on the device, under one of
``episode_scripts``, so T replays are a Monte-Carlo evaluation of the fleet.
"""
from . import _lib
from .balance import assemble_balance_device, default_balance_gains
from .command import command_device, command_state_size
from .disturb import DO_SIZE, PW_SIZE, DisturbParams, disturb_buffers, disturb_device, plant_step_wrench_device
from .episode import (EL_SIZE, ET_SIZE, POOL_INIT, POOL_SIZE, SEG_SIZE, EpisodeParams, episode_buffers, episode_device,
                      episode_state_size)
from .estimator import estimator_state_size, state_estimate_device
from .legplan import leg_plan_typed_device, plan_state_size
from .plant import plant_state_size, plant_step_device, plant_step_field_device, plant_step_terrain_device
from .policy import policy_device, policy_state_size
from .solver import MpcQpSolver
from .torques import joint_torques_device

# the stages a caller can leave out (``without=``), and the constructor option each stands for
_OPTION_OF = dict(disturb="disturb", command="command", estimate="estimator", plan="plan",
                  assemble_balance="control_type", balance="control_type", policy="policy", plant="plant",
                  episode="episode")


class ControlTick:
    def __init__(self, batch, params=None, device=0, plan=None, dt=None, estimator=None, command=None,
                 control_type=None, balance=None, gains=None, policy=None, plant=None, plant_init=None,
                 episode=None, episode_pool=None, episode_scripts=None, episode_log_len=4, disturb=None,
                 disturb_dirs=None, terrain=None, field=None):
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
        default (all-off) params every buffer is bitwise that of the tick without ``disturb``.
        ``terrain`` (rows of pack_terrain / terrain_from_slope; needs ``plant``): an option of the plant stage, not a
        stage of its own.  The plant stage runs on the inclined ground and the friction of the rows the tick then
        owns as ``terrain``: [B, TR_SIZE], robot b on row b, or with ``episode`` [P, TR_SIZE] parallel to
        ``episode_pool``, each robot on the row of its episode's pool index, so the ground restarts with the start
        pose.  ``without=("terrain",)`` gives the tick on flat ground.
        ``field`` ((rows, heights) of pack_height_field; needs ``plant``, exclusive with ``terrain``): the same kind
        of option for a bilinear height-field ground (steps, stairs, rough terrain).  The tick then owns ``field``
        [B, HF_SIZE] (with ``episode`` [P, HF_SIZE], parallel to ``episode_pool``) and ``heights``, the tiles.
        ``without=("field",)`` gives the tick on flat ground.
        A buffer the tick does not own is an absent attribute (``_buffers`` has the rule)."""
        import torch
        self.torch = torch
        self.B = int(batch)
        o = dict(disturb=disturb, command=command, estimator=estimator, plan=plan, control_type=control_type,
                 policy=policy, plant=plant, episode=episode, terrain=terrain, field=field)
        tick_dt = self._check(o, dt, episode_pool)
        if tick_dt is not None:
            self.dt = tick_dt
        self.solver = MpcQpSolver(params if params is not None else _lib.default_params(10), device=device)
        self.solver.reserve(self.B)
        dev = f"cuda:{device}"
        given = lambda rows: torch.as_tensor(rows, dtype=torch.float64)  # a caller's rows, before their reshape
        self.plan, self.estimator, self.command, self.policy, self.plant = plan, estimator, command, policy, plant
        self.typed = control_type is not None
        if self.typed:
            self.control_type = torch.full((self.B,), 1 if control_type == "per_robot" else int(control_type),
                                           dtype=torch.int32, device=dev)
            self.balance = balance if balance is not None else _lib.default_balance_params()
            self.gains = gains if gains is not None else default_balance_gains()
        if plant is not None:
            self.plant_init = None
            if plant_init is not None:
                self.plant_init = given(plant_init).reshape(self.B, _lib.PI_SIZE).to(dev).contiguous()
        self.episode = self.disturb = None
        if episode is not None:
            self.episode_pool = given(episode_pool).reshape(-1, POOL_SIZE).to(dev).contiguous()
            ep = EpisodeParams.from_buffer_copy(episode)
            ep.dt, ep.pool_count, ep.log_len = self.dt, self.episode_pool.shape[0], int(episode_log_len)
            ep.script_count = ep.script_segments = 0
            self.episode_scripts = None
            if episode_scripts is not None:
                sc = given(episode_scripts)
                sc = sc.reshape(sc.shape[0], -1, SEG_SIZE)
                ep.script_count, ep.script_segments = sc.shape[0], sc.shape[1]
                self.episode_scripts = sc.to(dev).contiguous()
            if self.plant_init is None:
                self.plant_init = self.episode_pool[:1, POOL_INIT:POOL_INIT + _lib.PI_SIZE].repeat(self.B, 1)
            self.episode = o["episode"] = ep
        if disturb is not None:
            dp = DisturbParams.from_buffer_copy(disturb)
            self.disturb_dirs = None
            dp.dir_count = 0
            if disturb_dirs is not None:
                self.disturb_dirs = given(disturb_dirs).reshape(-1, 4).to(dev).contiguous()
                dp.dir_count = self.disturb_dirs.shape[0]
            self.disturb = o["disturb"] = dp
        if terrain is not None:
            rows = given(terrain).reshape(-1, _lib.TR_SIZE)
            want = self.episode_pool.shape[0] if episode is not None else self.B
            if rows.shape[0] != want:
                raise ValueError(f"ControlTick(terrain=...) has {rows.shape[0]} rows; it needs {want}, one per "
                                 f"{'row of episode_pool' if episode is not None else 'robot'}")
            self.terrain = o["terrain"] = rows.to(dev).contiguous()
        if field is not None:
            rows, heights = field
            rows = given(rows).reshape(-1, _lib.HF_SIZE)
            want = self.episode_pool.shape[0] if episode is not None else self.B
            if rows.shape[0] != want:
                raise ValueError(f"ControlTick(field=...) has {rows.shape[0]} rows; it needs {want}, one per "
                                 f"{'row of episode_pool' if episode is not None else 'robot'}")
            self.field = o["field"] = rows.to(dev).contiguous()
            self.heights = given(heights).reshape(-1).to(dev).contiguous()
        self.counter = torch.zeros((self.B,), dtype=torch.int32, device=dev)
        for name, width in self._buffers(o).items():  # zero = a fresh slot, an uninitialised filter, a reset controller
            if width is not None:
                setattr(self, name, torch.zeros((self.B, *width) if isinstance(width, tuple) else (self.B, width),
                                                dtype=torch.float64, device=dev))
        self._options, self._dt_arg = o, dt
        self._tick = self._stage_list(o, tick_dt)
        if self.episode is not None:
            self.episode_buffers = self._episode_buffers(o)
        if self.disturb is not None:
            self.disturb_buffers = self._disturb_buffers(o)
        self.graph = None

    @staticmethod
    def _check(o, dt, pool):
        """Reject the combinations of options the constructor rejects.  Returns the tick's dt: the argument of
        update_plan, update_estimation and main_update and the plant's control period (None: no stage takes one)."""
        on = lambda name: o[name] is not None
        ct = o["control_type"]
        if on("plan"):
            dt = o["plan"].control_dt if dt is None else dt
        for name in ("estimator", "command"):
            if on(name) and dt is None:
                raise ValueError(f"ControlTick({name}=...) without plan= needs dt")
        if ct not in (None, 0, 1, "per_robot") and not (ct == 2 and on("policy")):
            raise ValueError('control_type must be None, 0, 1 or "per_robot" (or 2 with policy=)')
        if on("policy") and ct not in ("per_robot", 2):
            raise ValueError('ControlTick(policy=...) needs control_type="per_robot" or 2')
        if on("plant") and dt is None:
            raise ValueError("ControlTick(plant=...) without plan= / estimator= / command= needs dt")
        if on("episode") and (not on("plant") or pool is None):
            raise ValueError("ControlTick(episode=...) needs plant= and episode_pool=")
        if on("disturb") and not (on("plant") and on("episode")):
            raise ValueError("ControlTick(disturb=...) needs plant= and episode=")
        if on("terrain") and not on("plant"):
            raise ValueError("ControlTick(terrain=...) needs plant=")
        if on("field") and not on("plant"):
            raise ValueError("ControlTick(field=...) needs plant=")
        if on("field") and on("terrain"):
            raise ValueError("ControlTick(field=...) and terrain= exclude each other")
        return float(dt) if on("plan") or on("estimator") or on("command") or on("plant") else None

    def _buffers(self, o):
        """name -> row width in doubles of every buffer a tick with the options `o` owns.  A width is an int or,
        for rows of more than one dimension, a tuple; None marks a buffer that is not a zero-filled float64
        [B, width] tensor: the constructor builds it from an argument, and it may be None."""
        on = {name for name, v in o.items() if v is not None}
        sensors = on & {"estimator", "policy"}  # the estimator's input, else the policy stage's (caller-written)
        t = dict(states=_lib.ST_SIZE,        # caller writes robot states here
                 tq_records=_lib.TQ_SIZE,    # and Jacobians / swing forces here
                 records=_lib.rec_size(self.solver.horizon), warm=self.solver.warm_state_size,
                 results=_lib.RESULT_DOUBLES, torques=12, counter=None)
        if "plan" in on:
            t.update(plan_state=plan_state_size(), plan_out=_lib.PO_SIZE)
        if on & {"plan", "estimator", "command", "control_type", "plant"}:
            t["plan_in"] = _lib.PL_SIZE      # rot_z / foot_force / movement_mode, whichever the stages leave the caller
        if "estimator" in on:
            t.update(est_state=estimator_state_size(), est_out=_lib.EO_SIZE)
        if sensors:
            t["sensors"] = _lib.SN_SIZE      # quat / joints / IMU: the caller's, or the plant's
        if "command" in on:
            t["cmd_state"] = command_state_size()
        if on & {"command", "policy"}:
            t["cmd"] = _lib.CM_SIZE          # caller writes joystick-level commands here
        if "control_type" in on:
            t.update(control_type=None, bal_records=_lib.BAL_SIZE)
        if "policy" in on:
            t.update(policy_state=policy_state_size(), policy_out=_lib.PY_SIZE)
        if "plant" in on:
            t.update(plant_state=plant_state_size(), plant_out=_lib.PT_SIZE, plant_init=None)
        if "terrain" in on:
            t["terrain"] = None
        if "field" in on:
            t.update(field=None, heights=None)
        if "episode" in on:
            t.update(episode_state=episode_state_size(), episode_log=(o["episode"].log_len, EL_SIZE),
                     episode_totals=ET_SIZE, episode_pool=None, episode_scripts=None)
        if "disturb" in on:
            t.update(wrench=PW_SIZE, disturb_out=DO_SIZE, disturb_dirs=None)
            if sensors:
                t["sensors_noisy"] = _lib.SN_SIZE
        return t

    def _ptr(self, o):
        """ptr(name): the device pointer of a buffer the tick of the options `o` owns, else 0."""
        own = self._buffers(o)

        def ptr(name):
            t = getattr(self, name) if name in own else None
            return t.data_ptr() if t is not None else 0
        return ptr

    def _episode_buffers(self, o):
        p, w = self._ptr(o), self._buffers(o)
        return episode_buffers(
            p("plant_out"), p("plant_state"), p("plant_init"), p("torques"), p("sensors"), p("cmd"), p("results"),
            p("episode_pool"), p("episode_scripts"), p("states"), p("counter"), p("episode_log"), p("episode_totals"),
            p("est_state"), w.get("est_state", 0), p("plan_state"), w.get("plan_state", 0), p("cmd_state"),
            w.get("cmd_state", 0), p("policy_state"), w.get("policy_state", 0), p("warm"), w["warm"])

    def _disturb_buffers(self, o):
        p = self._ptr(o)
        return disturb_buffers(p("episode_state"), p("wrench"), p("sensors"), p("sensors_noisy"), p("disturb_dirs"),
                               p("disturb_out"))

    def _stage_list(self, o, dt):
        """The tick of the options `o` on this tick's buffers: its ordered (name, enqueue(stream)) pairs.  The
        untyped tick passes a null type pointer to the typed plan and warm solve, which is what
        mpcqp_leg_plan_device and mpcqp_solve_batch_warm_device do themselves."""
        on = lambda name: o[name] is not None
        p, B, solver = self._ptr(o), self.B, self.solver
        sensed = "sensors_noisy" if on("disturb") else "sensors"  # the row the controller's stages read
        truth = not on("estimator")  # the plant then also writes what the estimator would
        st = []
        if on("disturb"):
            dbf = self._disturb_buffers(o)
            st.append(("disturb", lambda s: disturb_device(o["disturb"], dbf, B, s)))
        if on("command"):
            st.append(("command", lambda s: command_device(
                o["command"], dt, p("cmd"), p("states"), p("plan_in"), B, p("cmd_state"), s)))
        if on("estimator"):
            st.append(("estimate", lambda s: state_estimate_device(
                o["estimator"], dt, p(sensed), p("plan_in"), p("states"), B, p("est_state"), p("tq_records"),
                p("est_out"), s)))
        if on("plan"):
            st.append(("plan", lambda s: leg_plan_typed_device(
                o["plan"], dt, p("states"), p("plan_in"), B, p("plan_state"), p("tq_records"), p("plan_out"),
                p("control_type"), s)))
        st.append(("assemble", lambda s: _lib.assemble_records_device(
            solver.horizon, p("states"), B, p("records"), s)))
        if on("control_type"):
            st.append(("assemble_balance", lambda s: assemble_balance_device(
                self.gains, p("states"), p("plan_in"), p("cmd_state"), B, p("bal_records"), s)))
            st.append(("balance", lambda s: solver.balance_solve_typed_device(
                self.balance, p("bal_records"), B, p("control_type"), 0, p("results"), s)))
        st.append(("solve", lambda s: solver.solve_warm_typed_device(
            p("records"), B, p("warm"), p("control_type"), 1, p("results"), 0, s)))
        st.append(("torques", lambda s: joint_torques_device(
            p("tq_records"), p("results"), B, p("counter"), p("torques"), s)))
        if on("policy"):
            st.append(("policy", lambda s: policy_device(
                o["policy"], p(sensed), p("states"), p("plan_in"), p("cmd"), B, p("policy_state"), p("torques"),
                p("policy_out"), p("control_type"), 2, s)))
        if on("plant"):
            rows = lambda s: (B, p("plant_state"), p("plant_init"), p("sensors"), p("plan_in"),
                              p("states") if truth else 0, p("tq_records") if truth else 0, p("plant_out"), s)
            if on("terrain"):  # the wrench row and the episode slot are null pointers in a tick without them
                st.append(("plant", lambda s: plant_step_terrain_device(
                    o["plant"], dt, p("torques"), p("wrench"), p("terrain"), o["terrain"].shape[0],
                    p("episode_state"), *rows(s))))
            elif on("field"):
                st.append(("plant", lambda s: plant_step_field_device(
                    o["plant"], dt, p("torques"), p("wrench"), p("field"), o["field"].shape[0], p("heights"),
                    self.heights.numel(), p("episode_state"), *rows(s))))
            elif on("disturb"):
                st.append(("plant", lambda s: plant_step_wrench_device(
                    o["plant"], dt, p("torques"), p("wrench"), *rows(s))))
            else:
                st.append(("plant", lambda s: plant_step_device(o["plant"], dt, p("torques"), *rows(s))))
        if on("episode"):
            ebf = self._episode_buffers(o)
            st.append(("episode", lambda s: episode_device(o["episode"], ebf, B, p("episode_state"), s)))
        return st

    def _stages_of(self, without):
        """This tick's stage list, or the one the constructor would have built, on the same buffers, had the
        options of the stages `without` been None (a constructor option's own name is accepted as well)."""
        if not without:
            return self._tick
        o = dict(self._options)
        for name in without:
            option = _OPTION_OF.get(name, name)
            if option not in o:
                raise ValueError(f"ControlTick: {name!r} is not a stage that can be left out "
                                 f"(one of {', '.join(_OPTION_OF)})")
            o[option] = None
        return self._stage_list(o, self._check(o, self._dt_arg, getattr(self, "episode_pool", None)))

    def _stream(self, stream):
        return stream if stream is not None else self.torch.cuda.current_stream().cuda_stream

    def _enqueue(self, name, stream):
        dict(self._tick)[name](self._stream(stream))

    def stages(self, without=()):
        """The names of the tick's stages in the order they are enqueued; ``without`` as in ``capture``."""
        return tuple(name for name, _ in self._stages_of(without))

    def _step(self, stages, stream, episode):
        s = self._stream(stream)
        for name, enqueue in stages:
            if episode or name != "episode":
                enqueue(s)

    def step(self, stream=None, episode=True):
        """Enqueue one tick on `stream` (default: torch's current stream).  ``episode=False`` leaves the episode
        stage out, for a caller that reads the tick's rows before enqueueing it with ``episode_stage()``."""
        self._step(self._tick, stream, episode)

    def disturb_stage(self, stream=None):
        """Enqueue the disturbance stage alone: first in the tick (``disturb_buffers``)."""
        self._enqueue("disturb", stream)

    def episode_stage(self, stream=None):
        """Enqueue the episode stage alone: last in the tick, on whichever of the sensors, cmd and slot buffers
        the tick has (``episode_buffers``)."""
        self._enqueue("episode", stream)

    def prime_plant(self, stream=None):
        """Enqueue the plant stage alone.  On fresh slots (after construction or a reset) it initialises them from
        ``plant_init`` and writes the rows of the start without integrating, so the first tick's estimator, plan
        and solve see the robot where it stands instead of zero rows.  (On a slot that is not fresh it is one
        more step under the current ``torques``.)"""
        self._enqueue("plant", stream)

    def capture(self, without=()):
        """Record step() as a graph.  Estimator, plan and warm slots, counters and torques keep evolving on replay,
        exactly as with eager steps; capture itself launches nothing.  The estimator and plan parameters and dt are
        kernel arguments, so the graph keeps the values they had at capture.
        ``without`` (stage names) records instead the tick the constructor would have built had those stages'
        options been None, on the same buffers: without ``disturb`` the estimator and the policy stage read
        ``sensors`` and the plant runs without the wrench row; without ``estimate`` the plant also writes the
        truth image; without ``terrain`` or ``field`` (options, not stages) the plant runs on flat ground.  A combination the constructor rejects raises its ValueError (``plant`` under an episode
        stage).  Only the full tick's graph becomes ``self.graph``."""
        torch = self.torch
        stages = self._stages_of(without)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            self._step(stages, None, True)
        if not without:
            self.graph = g
        return g

    def replay(self):
        self.graph.replay()

    def close(self):
        self.solver.close()
