"""The episode record of BatchedPlanEnv.enable_episode_record(): what every episode end leaves behind under
auto-reset, as device tensors the step kernel fills."""
import torch

from . import _lib
from .state import BatchedState, reference_state


class EpisodeEnds(object):
    """The episodes that ended in the last step (libbcplan's episode record, bcp_bind_episode_record): what a caller of the
    reference's PlanEnv sees from step() before it calls reset() (envs/base/env.py:334-361, 293-303), kept although the
    step has already auto-reset the env.  Device tensors, filled by the step kernel itself (no sync, no extra launch):

      reason        uint8 [N]          BCP_DONE_* bits of every env (GOAL | TIMEOUT | COLLIDED, env.py:400-419), 0 = not done
      count         int32 [1]          envs that ended in the last step (may exceed `capacity`: overflow)
      env_ids       int32 [capacity]   slot j < count: which env ended (order unspecified)
      geom          int32 [capacity]   the geometry-pool entry the episode ran on (-1 without a pool)
      final_state   BatchedState over the slots: the state the env held after its last step, before the reset
                    (robot, reward-provider state, current_iter = episode length, robot_collided; the seen pose / robot
                    state with delays; no queues)
      final_return  float64 [capacity] the episode's return, the float64 sum of its rewards in step order
      ret           float64 [N]        every env's running return (zeroed by every reset; set_state / fan_out leave it)

    The running returns start at 0 when the record is bound: bound in the middle of episodes, each env's first
    final_return covers only the steps since then (bind right after a reset() for whole-episode returns).
    """

    GOAL, TIMEOUT, COLLIDED = _lib.DONE_GOAL, _lib.DONE_TIMEOUT, _lib.DONE_COLLIDED

    def __init__(self, env, capacity):
        n, dev, cap = env.n_envs, env.device, int(capacity)
        if cap < 1:
            raise ValueError("capacity must be positive")
        self._env, self.capacity = env, cap

        def zeros(*shape, dtype=torch.float64):
            return torch.zeros(*shape, dtype=dtype, device=dev)

        self.reason = zeros(n, dtype=torch.uint8)
        self.ret = zeros(n)
        self.count = zeros(1, dtype=torch.int32)
        self.env_ids = zeros(cap, dtype=torch.int32)
        self.geom = torch.full((cap,), -1, dtype=torch.int32, device=dev)
        self.final_return = zeros(cap)
        pd, sd = int(env.params.pose_delay), int(env.params.state_delay)
        self.final_state = BatchedState(zeros(7, cap), zeros(cap), zeros(cap, dtype=torch.int32),
                                        zeros(cap, dtype=torch.int32), zeros(cap, dtype=torch.uint8),
                                        pose_seen=zeros(3, cap) if pd else None,
                                        robot_state_seen=zeros(7, cap) if sd else None)

    def _c_struct(self):
        rec = _lib.BcpEpisodeRecord()
        rec.capacity = self.capacity
        rec.reason, rec.ret, rec.count = self.reason.data_ptr(), self.ret.data_ptr(), self.count.data_ptr()
        rec.env_id, rec.geom, rec.final_ret = self.env_ids.data_ptr(), self.geom.data_ptr(), self.final_return.data_ptr()
        self.final_state.fill_pointers(rec.final)
        return rec

    @property
    def length(self):
        """int32 [capacity]: the episodes' lengths in steps (final_state.current_iter)."""
        return self.final_state.current_iter

    def terminated(self):
        """bool [N]: the episode ended in a terminal state -- goal reached or collided (a time-out together with one
        of them counts as terminal)."""
        return (self.reason & (self.GOAL | self.COLLIDED)) != 0

    def truncated(self):
        """bool [N]: the episode was cut by the time limit alone (gymnasium's `truncated`, SB3's TimeLimit.truncated):
        bootstrap V(final observation) there."""
        return self.reason == self.TIMEOUT

    def overflowed(self):
        """True if more envs ended in the last step than there are slots (synchronises)."""
        return int(self.count[0]) > self.capacity

    def slots(self):
        """Number of filled slots of the last step, min(count, capacity) (synchronises)."""
        return min(int(self.count[0]), self.capacity)

    def to_host(self):
        """The last step's episode ends as a list of (env id, reference State, reason bits, return, length); the States
        hold no delay queues.  Synchronises -- for debugging and tests."""
        e = self._env
        m = self.slots()
        ids = self.env_ids[:m].cpu().numpy()
        geom = self.geom[:m].cpu().numpy()
        reason = self.reason.cpu().numpy()
        ret = self.final_return[:m].cpu().numpy()
        f = self.final_state
        robot = f.robot[:, :m].cpu().numpy()
        md = f.min_spat_dist_so_far[:m].cpu().numpy()
        ti = f.target_idx[:m].cpu().numpy()
        it = f.current_iter[:m].cpu().numpy()
        time = e.time_of(f.current_iter[:m]).cpu().numpy()
        col = f.robot_collided[:m].cpu().numpy()
        ps = f.pose_seen[:, :m].cpu().numpy() if f.pose_seen is not None else None
        rs = f.robot_state_seen[:, :m].cpu().numpy() if f.robot_state_seen is not None else None
        out = []
        for j in range(m):
            i, g = int(ids[j]), int(geom[j])
            # (the entry the episode ran on, not the one the auto-reset moved the env to)
            st = reference_state(e, e._path_host.of_env(i, g), e._map_host.of_env(i, g), md[j], ti[j], it[j], time[j], col[j],
                                 ps[:, j].copy() if ps is not None else robot[:3, j].copy(),
                                 rs[:, j] if rs is not None else robot[:, j])
            out.append((i, st, int(reason[i]), float(ret[j]), int(it[j])))
        return out
