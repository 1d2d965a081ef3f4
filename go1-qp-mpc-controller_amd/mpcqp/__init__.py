"""mpcqp — MI355X-native batched convex-MPC QP engine (host-side Python plumbing).

The compute path is libmpcqp.so (hand-written gfx950 HIP kernels behind the C ABI in
include/mpcqp.h); this package only packs records, owns handles and calls the ABI.
"""
from . import _lib
from ._lib import (assemble_records_device, EXPORTED, LIB_PATH, RESULT_DTYPE, MpcQpError, Params, Result, default_params,
                   load, rec_feet, rec_size, status_str)
from .balance import assemble_balance, assemble_balance_device, default_balance_gains, default_balance_params
from .command import (CMD_STATE_DTYPE, CommandParams, command_device, command_state_size, default_command_params,
                      pack_commands)
from .disturb import (DISTURB_OUT_DTYPE, DisturbBuffers, DisturbParams, default_disturb_params, disturb_buffers,
                      disturb_device, disturbance_of, pack_push_dirs, plant_step_wrench_device)
from .episode import (EPISODE_LOG_DTYPE, EPISODE_STATE_DTYPE, EPISODE_TOTALS_DTYPE, EpisodeBuffers, EpisodeParams,
                      default_episode_params, episode_buffers, episode_device, episode_state_size,
                      pack_episode_pool, pack_episode_scripts)
from .estimator import (EST_OUT_DTYPE, EstimatorParams, default_estimator_params, estimator_state_size,
                        pack_estimator_slot, pack_sensors, state_estimate_device, unpack_estimator_slot)
from .legplan import (PLAN_OUT_DTYPE, PlanParams, default_plan_params, leg_plan_device, leg_plan_typed_device,
                      pack_plan_inputs, plan_state_size)
from .policy import (POLICY_OUT_DTYPE, POLICY_STATE_DTYPE, Policy, PolicyParams, default_policy_params,
                     load_policy_weights, policy_device, policy_state_size)
from .plant import (PLANT_OUT_DTYPE, PLANT_STATE_DTYPE, PlantParams, default_plant_params, pack_plant_init,
                    field_lookup, pack_height_field, pack_terrain, place_on_field, place_on_terrain, plant_state_size,
                    plant_step_device, plant_step_field_device, plant_step_terrain_device, terrain_from_slope,
                    terrain_height)
from .records import (GO1_Q, GO1_R, RobotStates, assemble_compute_grf, assemble_test_mpc,
                      pack_states, synthetic_go1)
from .robot_control import Go1RobotControl, RobotControl
from .solver import MpcQpSolver
from .torques import assemble_torque_records, joint_torques_device

__all__ = [
    "EXPORTED", "LIB_PATH", "RESULT_DTYPE", "MpcQpError", "Params", "Result", "default_params", "load",
    "rec_feet", "rec_size", "status_str", "GO1_Q", "GO1_R", "RobotStates", "assemble_compute_grf",
    "assemble_test_mpc", "synthetic_go1", "Go1RobotControl", "RobotControl", "MpcQpSolver",
    "assemble_torque_records", "joint_torques_device", "pack_states", "assemble_records_device",
    "PLAN_OUT_DTYPE", "PlanParams", "default_plan_params", "leg_plan_device", "pack_plan_inputs", "plan_state_size",
    "EST_OUT_DTYPE", "EstimatorParams", "default_estimator_params", "estimator_state_size", "pack_estimator_slot",
    "pack_sensors", "state_estimate_device", "unpack_estimator_slot",
    "CMD_STATE_DTYPE", "CommandParams", "command_device", "command_state_size", "default_command_params",
    "pack_commands", "assemble_balance", "assemble_balance_device", "default_balance_gains",
    "default_balance_params", "leg_plan_typed_device",
    "POLICY_OUT_DTYPE", "POLICY_STATE_DTYPE", "Policy", "PolicyParams", "default_policy_params",
    "load_policy_weights", "policy_device", "policy_state_size",
    "PLANT_OUT_DTYPE", "PLANT_STATE_DTYPE", "PlantParams", "default_plant_params", "pack_plant_init",
    "plant_state_size", "plant_step_device", "pack_terrain", "place_on_terrain", "plant_step_terrain_device",
    "terrain_from_slope", "terrain_height", "field_lookup", "pack_height_field", "place_on_field",
    "plant_step_field_device",
    "EPISODE_LOG_DTYPE", "EPISODE_STATE_DTYPE", "EPISODE_TOTALS_DTYPE", "EpisodeBuffers", "EpisodeParams",
    "default_episode_params", "episode_buffers", "episode_device", "episode_state_size", "pack_episode_pool",
    "pack_episode_scripts",
    "DISTURB_OUT_DTYPE", "DisturbBuffers", "DisturbParams", "default_disturb_params", "disturb_buffers",
    "disturb_device", "disturbance_of", "pack_push_dirs", "plant_step_wrench_device",
]
