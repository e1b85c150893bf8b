"""bc_gym_planning_env_amd: MI355X-native batched PlanEnv.step() behind the reference's Observation / Action / State
API.  The compute lives in libbcplan.so (hand-written HIP for gfx950, C ABI in include/bcplan.h); this package is the
thin Python host side.  Importing the package never touches the GPU; creating an env without the built library or
without a GPU raises."""
from .api import (Action, Box, ContinuousRewardProviderState, CostMap2D, DiffdriveRobotState, EnvParams,  # noqa: F401
                  INDUSTRIAL_DIFFDRIVE_V1, INDUSTRIAL_TRICYCLE_V1, Observation, RewardParams, State,
                  TricycleRobotState)

__all__ = ["Action", "Box", "ContinuousRewardProviderState", "CostMap2D", "DiffdriveRobotState", "EnvParams",
           "INDUSTRIAL_DIFFDRIVE_V1", "INDUSTRIAL_TRICYCLE_V1", "Observation", "RewardParams", "State",
           "TricycleRobotState", "BatchedPlanEnv", "BatchedRandomAisleTurnEnv", "NativeOps", "Lookahead", "ShootingPlanner",
           "constant_command_library", "Mppi", "MPPIPlanner", "Track", "TrackingPlanner", "pursuit_gain_library",
           "BatchedRangeScan", "BatchedGoalField", "GoalField", "SpeedProfile"]


def __getattr__(name):
    # torch is imported lazily so that `import bc_gym_planning_env_amd` stays cheap for host-only users
    if name in ("BatchedPlanEnv", "BatchedState", "BatchedObservation", "Lookahead", "Mppi", "Track"):
        from . import batched_env
        return getattr(batched_env, name)
    if name == "BatchedRandomAisleTurnEnv":
        from .aisle_env import BatchedRandomAisleTurnEnv
        return BatchedRandomAisleTurnEnv
    if name in ("ShootingPlanner", "constant_command_library", "MPPIPlanner", "TrackingPlanner",
                "pursuit_gain_library"):
        from . import planning
        return getattr(planning, name)
    if name == "BatchedRangeScan":
        from .range_scan import BatchedRangeScan
        return BatchedRangeScan
    if name in ("BatchedGoalField", "GoalField"):
        from . import goal_field
        return getattr(goal_field, name)
    if name == "SpeedProfile":
        from .speed_profile import SpeedProfile
        return SpeedProfile
    if name == "NativeOps":
        from .ops import NativeOps
        return NativeOps
    raise AttributeError(name)
