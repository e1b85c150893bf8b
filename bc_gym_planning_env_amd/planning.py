"""Planners on top of BatchedPlanEnv: the `.act(obs) -> Action` of the reference's motion planning challenge (README,
bc_gym_planning_env/run_the_challange.py), for N envs at once.  Worked examples, not a planning framework.
ShootingPlanner: every tick each env scores a fixed library of candidate plans with the noise-free forward model
(lookahead()) and takes the first action of the best one (no collision within the horizon first, then the largest return).
MPPIPlanner: every tick each env refines its own plan by sampling around it (mppi(), one kernel launch) and takes the
plan's first action; the rest of the plan is the next tick's warm start.
TrackingPlanner: every tick each env rolls a pure-pursuit tracker out under K gain settings (track(), one kernel launch) and
takes the first command of the best one; its plan can seed MPPIPlanner (nominal=)."""
import numpy as np
import torch

from . import _lib


class Lookahead(object):
    """What BatchedPlanEnv.lookahead() returns: device tensors over [N, K] candidates (no sync).  `ret` float64 return of
    the steps taken, `steps` int32, `reason` uint8 DONE_* bits (0: not done within the horizon); optional, None unless
    asked for: `final_pose` [N, K, 3], `final_target_idx`, `err`, `best` int32 [N], `best_action` [N, 2].  The tensors
    are the env's cached buffers for this (H, K): the next lookahead() with the same shape overwrites them."""

    FIELDS = ("ret", "steps", "reason", "final_pose", "final_target_idx", "err", "best", "best_action")

    def __init__(self, horizon, n_candidates, **tensors):
        self.horizon, self.n_candidates = horizon, n_candidates
        for name in self.FIELDS:
            setattr(self, name, tensors.get(name))

    def collided(self):
        """bool [N, K]: the candidate ends in a collision"""
        return (self.reason & _lib.DONE_COLLIDED) != 0

    def timed_out(self):
        return (self.reason & _lib.DONE_TIMEOUT) != 0

    def reached_goal(self):
        return (self.reason & _lib.DONE_GOAL) != 0


class Mppi(object):
    """What BatchedPlanEnv.mppi() returns (device tensors, no sync): `mean` [N, H, 2] float64, the refined plan; `action`
    [N, 2] = mean[:, 0], ready for step(); optional, None unless asked for: `eps` [I, N, K, H, 2] float32 (the
    perturbations used), `iter_mean` [I, N, H, 2] (the mean going into each iteration), `iter_ret` / `iter_reason`
    [I, N, K], `err` int32 [N]; with a goal field (bcp_mppi_field) also `iter_value` int32 [I, N, K], the field value read at
    each candidate's final pose (GOAL_NONE = none), and `iter_score` float64 [I, N, K], the scores as weighted; with
    adapt (bcp_mppi_adapt) `sigma` [N, H, 2] float64, the refined widths, and optionally `iter_sigma` [I, N, H, 2], the widths
    going into each iteration.  Everything but `mean` and `sigma` is a cached buffer of the env for this (H, K, I)."""

    FIELDS = ("eps", "iter_mean", "iter_ret", "iter_reason", "err", "iter_sigma", "iter_value", "iter_score")
    TERMINAL_FIELDS = ("iter_value", "iter_score")   # need a goal field

    def __init__(self, horizon, n_candidates, iterations, mean, action, sigma=None, **tensors):
        self.horizon, self.n_candidates, self.iterations = horizon, n_candidates, iterations
        self.mean, self.action, self.sigma = mean, action, sigma
        for name in self.FIELDS:
            setattr(self, name, tensors.get(name))


class Track(Lookahead):
    """What BatchedPlanEnv.track() returns: device tensors over [N, K] gain settings (no sync).  `actions` [N, K, H, 2]
    float64, the commands the tracker took (after a setting's done step its last command repeated); `ret`, `steps`,
    `reason` as in Lookahead; optional, None unless asked for: `final_pose`, `final_target_idx`, `err`, `trace`
    [N, K, H, 6] (x, y, th, wheel angle, target_idx, carrot index as the law read them at step t; zeros after the done
    step), `best` int32 [N], `best_plan` [N, H, 2] = actions[i, best[i]], `best_action` [N, 2].  The tensors are the env's
    cached buffers for this (H, K): the next track() with the same shape overwrites them."""

    FIELDS = ("actions", "ret", "steps", "reason", "final_pose", "final_target_idx", "err", "trace", "best", "best_plan",
              "best_action")
    REQUIRED = FIELDS[:4]


def pursuit_gain_library(action_space, n_speed, reaches):
    """[n_speed * len(reaches), 2] float64 gain settings (speed, reach) for BatchedPlanEnv.track(): the speeds spread evenly
    over (0, action_space.high[0]] -- high[0] * (i + 1) / n_speed --, every one with every reach (metres, > 0).
    Setting k = i_speed * len(reaches) + i_reach."""
    reaches = np.asarray(reaches, np.float64).reshape(-1)
    if n_speed < 1 or reaches.size < 1 or not (reaches > 0).all():
        raise ValueError("n_speed must be at least 1 and reaches positive")
    top = float(np.asarray(action_space.high, np.float64)[0])
    speeds = top * (np.arange(n_speed, dtype=np.float64) + 1.0) / n_speed
    v, r = np.meshgrid(speeds, reaches, indexing="ij")
    return np.ascontiguousarray(np.stack([v.ravel(), r.ravel()], axis=1))


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
    :param goal_field: optional goal_field.GoalField of the env (env.goal_field()): the candidates' final poses are then
        scored by their distance to go through free space -- what the H steps of the look-ahead cannot see
    :param terminal_weight: reward per metre of that distance; the key of a candidate is
        (not collided, ret - terminal_weight * distance to go), the largest wins, ties go to the lowest k.  A final pose
        without a route counts as the longest distance a field can hold (GOAL_FAR cells)
    """

    def __init__(self, env, library, goal_field=None, terminal_weight=0.0):
        self.env = env
        device = getattr(env, "device", None) or env.unwrapped.device
        lib = library if isinstance(library, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(library))
        if lib.dim() != 3 or lib.shape[2] != 2:
            raise ValueError("library must have shape (H, K, 2), got %s" % (tuple(lib.shape),))
        self.library = lib.to(device).contiguous()
        self.goal_field, self.terminal_weight = goal_field, float(terminal_weight)
        self._row_env = None
        self.last = None        # the Lookahead of the latest act()
        self.last_best = None   # with a goal field: int64 [N], the candidates chosen by the latest act()

    def act(self, observation=None):
        """actions [N, 2] (device tensor, dtype of the library) for env.step().  The observation is not needed: the
        look-ahead reads the env's own state, which is what the challenge allows ("explicit information about the
        forward model of the robot")."""
        if self.goal_field is None:
            self.last = self.env.lookahead(self.library, want=("best", "best_action"))
            return self.last.best_action
        la = self.last = self.env.lookahead(self.library, want=("final_pose",))
        n, k = la.ret.shape
        if self._row_env is None or self._row_env.numel() != n * k:
            self._row_env = torch.arange(n, dtype=torch.int32, device=la.ret.device).repeat_interleave(k)
        field = self.goal_field
        farthest = _lib.GOAL_FAR * field.resolution / _lib.GOAL_ORTHO
        out3 = field.sample(la.final_pose.reshape(n * k, 3), row_env=self._row_env, carrot_cells=1, max_dist=farthest)
        score = la.ret - self.terminal_weight * out3[:, 0].to(torch.float64).reshape(n, k)
        # the largest key (not collided, score), ties to the lowest k: the eligible candidates are the ones that do not
        # collide, or all of them where every one collides; among those with the best score the lowest index wins
        free = ~la.collided()
        eligible = free | ~free.any(dim=1, keepdim=True)
        top = torch.where(eligible, score, torch.full_like(score, -float("inf"))).amax(dim=1, keepdim=True)
        index = torch.arange(k, device=score.device).expand(n, k)
        self.last_best = torch.where(eligible & (score == top), index, torch.full_like(index, k)).amin(dim=1)
        return self.library[0, self.last_best]


class TrackingPlanner(object):
    """A pure-pursuit path follower per env on BatchedPlanEnv.track(): every tick the K gain settings of `gains` are rolled
    out over `horizon` steps of the noise-free forward model, and the env takes the first command of the best one (no
    collision within the horizon first, then the largest return).

    :param env: a BatchedPlanEnv (or a wrapper that forwards track); delays must be 0, the reward provider the continuous one
    :param gains: [K, 2] settings (speed, reach) shared by all envs, e.g. pursuit_gain_library(env.action_space, 3,
        (0.4, 0.8, 1.6)), or [N, K, 2] settings per env
    :param horizon: steps H of a roll-out
    :param max_curvature: the clamp of the arc's curvature in 1/m; None: what the robot can turn (BatchedPlanEnv.track)
    :param speed_profile: None, or a SpeedProfile of the env's bound paths (env.speed_profile()): every setting's speed is
        capped by it, so the tracker slows for corners (bcp_track_profile); also settable later as self.speed_profile, e.g.
        after route_paths(), which makes an earlier profile stale
    """

    def __init__(self, env, gains, horizon, max_curvature=None, speed_profile=None):
        self.env = env
        base = env
        while not hasattr(base, "n_envs"):
            base = base.unwrapped() if callable(base.unwrapped) else base.unwrapped
        g = gains if isinstance(gains, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(gains, dtype=np.float64))
        self.base = base   # the BatchedPlanEnv under the wrappers
        self.gains = g.to(base.device).to(torch.float64).contiguous()
        self.horizon, self.max_curvature, self.speed_profile = int(horizon), max_curvature, speed_profile
        self.last = None   # the Track of the latest act() or plan()

    def _extra(self):
        """(speed_profile=None is the call as it always was, also through wrappers that know no such keyword)"""
        return {} if self.speed_profile is None else dict(speed_profile=self.speed_profile)

    def act(self, observation=None):
        """actions [N, 2] (float64 device tensor) for env.step(): step 0 of the best setting.  The observation is not needed
        (as for ShootingPlanner): the roll-outs start from the env's own state."""
        self.last = self.env.track(self.gains, self.horizon, self.max_curvature, want=("best", "best_action"), **self._extra())
        return self.last.best_action

    def plan(self, mask=None):
        """[N, H, 2] float64: the commands of the best setting over the horizon -- a cached buffer of the env, overwritten by
        the next call.  mask: optional [N]; rows of envs with mask 0 keep what the buffer held."""
        self.last = self.env.track(self.gains, self.horizon, self.max_curvature, mask=mask, want=("best", "best_plan"),
                                   **self._extra())
        return self.last.best_plan


class MPPIPlanner(object):
    """Model-predictive path integral control per env on BatchedPlanEnv.mppi(): a receding-horizon plan `mean` [N, H, 2]
    (float64, on the device) refined every tick and shifted by one step afterwards.

    :param env: a BatchedPlanEnv (or a wrapper that forwards mppi); delays must be 0
    :param horizon: steps H of the plan
    :param n_candidates: samples K per iteration, a power of two in [8, 1024] (candidate 0 is the plan itself)
    :param iterations: refinement rounds I per tick
    :param sigma: standard deviations (v, w) of the perturbations
    :param lam: temperature of the weights softmax(score / lam)
    :param collision_penalty: subtracted from the return of a candidate that collides within the horizon
    :param seed: of the perturbation stream (tick j uses draw index j; the env's noise stream is not involved)
    :param goal_field: optional goal_field.GoalField of the env (env.goal_field()): every candidate's score then loses
        terminal_weight * its final pose's distance to go through free space, inside the same launch (bcp_mppi_field) --
        what the H steps of the roll-out cannot see.  A final pose without a route counts as GOAL_FAR cells
    :param terminal_weight: reward per metre of that distance, finite and >= 0; 0 plans exactly as without a field
    :param adapt_rate: None: every step of every plan is sampled with `sigma`, tick after tick.  A rate in [0, 1]: the planner
        owns a width per env, step and component, `self.sigma` [N, H, 2], which every iteration moves by that share of the
        way to the weighted spread of the commands (bcp_mppi_adapt, the same launch) and which shifts with the plan
    :param sigma_min, sigma_max: the clamps of the widths, two values each; default sigma / 8 and 2 * sigma
    :param sigma_recover: after the shift every width relaxes towards `sigma` by this share of the difference

    :param nominal: None, or a TrackingPlanner of the same env and horizon: a new plan is then the tracker's best plan
        (TrackingPlanner.plan()) from the env's state at that moment, not the centre of the box; reset_plans() then
        launches the tracker for the envs it names

    A new plan -- at the start, and for the envs named by reset_plans() -- holds the centre of the action box,
    (low + high) / 2, at every step (or, with `nominal`, the tracker's plan), and with adapt_rate `sigma` as its widths."""

    def __init__(self, env, horizon, n_candidates, iterations, sigma, lam, collision_penalty, seed=0, goal_field=None,
                 terminal_weight=0.0, adapt_rate=None, sigma_min=None, sigma_max=None, sigma_recover=0.0, nominal=None):
        self.env = env
        self.goal_field, self.terminal_weight = goal_field, float(terminal_weight)
        base = env
        while not hasattr(base, "n_envs"):   # wrappers forward mppi(); the sizes and the device are the batched env's
            base = base.unwrapped() if callable(base.unwrapped) else base.unwrapped
        device = base.device
        self.horizon, self.n_candidates, self.iterations = int(horizon), int(n_candidates), int(iterations)
        self.sigma, self.lam, self.collision_penalty, self.seed = tuple(sigma), float(lam), float(collision_penalty), int(seed)
        space = base.action_space
        centre = 0.5 * (np.asarray(space.low, np.float64) + np.asarray(space.high, np.float64))
        self.default = torch.from_numpy(centre).to(device)
        self.mean = self.default.expand(base.n_envs, self.horizon, 2).contiguous()
        self.adapt_rate, self.sigma_recover = adapt_rate, float(sigma_recover)
        if adapt_rate is not None:   # self.sigma becomes the widths [N, H, 2]; the two they start from stay in sigma0
            width = np.asarray(sigma, np.float64).reshape(2)
            self.sigma_min = tuple(width / 8 if sigma_min is None else np.asarray(sigma_min, np.float64).reshape(2))
            self.sigma_max = tuple(2 * width if sigma_max is None else np.asarray(sigma_max, np.float64).reshape(2))
            self.sigma0 = torch.from_numpy(width).to(device)
            self._sigma_call = tuple(width)
            self.sigma = self.sigma0.expand(base.n_envs, self.horizon, 2).contiguous()
        self.nominal = nominal
        if nominal is not None:
            if nominal.base is not base:   # (through whatever wrappers either was given)
                raise ValueError("nominal follows another env than this planner's")
            if nominal.horizon != self.horizon:
                raise ValueError("nominal plans %d steps, this planner %d" % (nominal.horizon, self.horizon))
            self.mean.copy_(nominal.plan())
        self.draw_index = 0
        self._fresh = True    # nothing to shift yet
        self.last = None      # the Mppi of the latest act()

    def reset_plans(self, mask):
        """Call after env.step() with its done mask ([N], non-zero = the env's episode ended and, under auto-reset, it
        starts anew): those envs' plans go back to the default.  With `nominal` that default is the tracker's plan, and
        every call launches bcp_track with this mask (a host check of the mask would synchronise): the lanes of envs with
        mask 0 take no trip, so a call with nothing to reset costs the launch, + 0.02 ms per tick at 4 096 envs."""
        mask = mask if isinstance(mask, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(mask))
        mask = mask.to(self.mean.device) != 0
        fresh = self.default if self.nominal is None else self.nominal.plan(mask=mask.to(torch.uint8))
        self.mean.copy_(torch.where(mask[:, None, None], fresh, self.mean))
        if self.adapt_rate is not None:
            self.sigma.copy_(torch.where(mask[:, None, None], self.sigma0, self.sigma))

    def act(self, observation=None):
        """actions [N, 2] (float64 device tensor) for env.step().  The observation is not needed (as for ShootingPlanner):
        the roll-outs start from the env's own state."""
        if not self._fresh:   # receding horizon: drop the step just taken, repeat the last row
            self.mean.copy_(torch.cat([self.mean[:, 1:], self.mean[:, -1:]], dim=1))
            if self.adapt_rate is not None:   # the widths go with their steps; the new last step starts from sigma0
                shifted = torch.cat([self.sigma[:, 1:], self.sigma0.expand(self.sigma.shape[0], 1, 2)], dim=1)
                self.sigma.copy_(shifted + self.sigma_recover * (self.sigma0 - shifted))
        self._fresh = False
        extra = {} if self.goal_field is None else dict(goal_field=self.goal_field, terminal_weight=self.terminal_weight)
        sigma = self.sigma
        if self.adapt_rate is not None:
            sigma = self._sigma_call
            extra["adapt"] = dict(sigma=self.sigma, rate=self.adapt_rate, sigma_min=self.sigma_min, sigma_max=self.sigma_max)
        self.last = self.env.mppi(self.mean, sigma, self.iterations, self.n_candidates, self.lam, self.collision_penalty,
                                  seed=self.seed, draw_index=self.draw_index, **extra)
        self.draw_index += 1
        return self.last.action
