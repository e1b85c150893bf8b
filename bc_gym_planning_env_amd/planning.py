"""A shooting planner on top of BatchedPlanEnv.lookahead(): the `.act(obs) -> Action` of the reference's motion planning
challenge (README, bc_gym_planning_env/run_the_challange.py), for N envs at once.  A worked example, not a planning framework: every
tick each env scores a fixed library of candidate plans with the noise-free forward model and takes the first action of
the best one (no collision within the horizon first, then the largest return)."""
import numpy as np
import torch


def constant_command_library(action_space, n_v, n_angle, horizon):
    """[horizon, n_v * n_angle, 2] float32: every candidate holds ONE command for the whole horizon; the commands form
    a regular grid over the action box (both ends included; a single value sits in the middle of its range).
    Candidate k = iv * n_angle + ia."""
    low, high = np.asarray(action_space.low, np.float64), np.asarray(action_space.high, np.float64)

    def axis(lo, hi, count):
        return np.linspace(lo, hi, count) if count > 1 else np.array([0.5 * (lo + hi)])

    if n_v < 1 or n_angle < 1 or horizon < 1:
        raise ValueError("n_v, n_angle and horizon must be at least 1")
    v, a = np.meshgrid(axis(low[0], high[0], n_v), axis(low[1], high[1], n_angle), indexing="ij")
    commands = np.stack([v.ravel(), a.ravel()], axis=1).astype(np.float32)
    # (float32 rounding may step outside a float64 bound by an ulp: stay inside the box as the space's dtype sees it)
    commands = np.clip(commands, low.astype(np.float32), high.astype(np.float32))
    return np.ascontiguousarray(np.broadcast_to(commands, (horizon,) + commands.shape))


class ShootingPlanner(object):
    """Picks, for every env, the first action of the best candidate of `library` ([H, K, 2]) under env.lookahead().

    :param env: a BatchedPlanEnv (or a wrapper that forwards lookahead); delays must be 0
    :param library: [H, K, 2] candidate plans shared by all envs, e.g. constant_command_library(env.action_space, 5, 9, 16)
    """

    def __init__(self, env, library):
        self.env = env
        device = getattr(env, "device", None) or env.unwrapped.device
        lib = library if isinstance(library, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(library))
        if lib.dim() != 3 or lib.shape[2] != 2:
            raise ValueError("library must have shape (H, K, 2), got %s" % (tuple(lib.shape),))
        self.library = lib.to(device).contiguous()
        self.last = None   # the Lookahead of the latest act()

    def act(self, observation=None):
        """actions [N, 2] (device tensor, dtype of the library) for env.step().  The observation is not needed: the
        look-ahead reads the env's own state, which is what the challenge allows ("explicit information about the
        forward model of the robot")."""
        self.last = self.env.lookahead(self.library, want=("best", "best_action"))
        return self.last.best_action
