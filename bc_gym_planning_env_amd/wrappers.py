"""The base of the observation wrappers around a BatchedPlanEnv (egocentric.py, range_scan.py): everything but what
an observation kind draws."""
import ctypes as C

import torch


class BatchedObservationWrapper(object):
    """step() / reset() return observation(), an OrderedDict of device tensors over the N envs that the subclass draws.
    final_observation=True: the env's episode record is enabled (env.enable_episode_record) and step() adds
    info["final_observation"], the observation of every episode that ended in the step, drawn from its final state
    before the auto-reset (SB3's terminal_observation, gymnasium's final_obs): the same keys with leading dimension
    `capacity`, row j belongs to env info["episode_ends"].env_ids[j] for j < count.

    A subclass provides observation() (draw and return the current observation), _alloc_final(capacity) (make the final
    buffers, return their OrderedDict) and _draw_final(stream) (fill them from the record's slots), and calls
    _init_final() at the end of its constructor, when its shapes are known."""

    def __init__(self, env):
        self.env = env
        self.action_space = env.action_space
        self._lib = env._lib
        self.n_state = 6 if env.is_tricycle else 5
        self._final = None

    def _init_final(self, final_observation):
        if final_observation:
            env = self.env
            ends = env.episode_ends if env.episode_ends is not None else env.enable_episode_record()
            self._final = self._alloc_final(ends.capacity)

    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.env.device).cuda_stream)

    def _goal_vector(self, rows):
        """goal_n_state for `rows` envs / slots: float32 [rows, 3 + n_state, 1]"""
        return torch.zeros((rows, 3 + self.n_state, 1), dtype=torch.float32, device=self.env.device)

    def _final_buffers(self):
        """The buffers follow the env's record: a record bound again with another capacity gets buffers of that size."""
        ends = self.env.episode_ends
        if ends is None:
            raise RuntimeError("final_observation=True needs the env's episode record (env.disable_episode_record() "
                               "was called)")
        if next(iter(self._final.values())).shape[0] != ends.capacity:
            self._final = self._alloc_final(ends.capacity)
        return self._final

    def step(self, actions, **kw):
        _o, reward, done, info = self.env.step(actions, **kw)
        if self._final is not None:
            # drawn now, on the step's stream: a pool refresh after this step may release the worlds the envs just left
            final = self._final_buffers()
            self._draw_final(self._stream())
            info = dict(info, final_observation=final)   # (a copy: the env's own info dict stays as the env keeps it)
        return self.observation(), reward, done, info

    def reset(self, mask=None):
        self.env.reset(mask)
        return self.observation()

    def unwrapped(self):
        return self.env

    def seed(self, seed=None):
        self.env.seed(seed)

    def lookahead(self, actions, **kw):
        return self.env.lookahead(actions, **kw)

    def mppi(self, mean, *args, **kw):
        return self.env.mppi(mean, *args, **kw)

    def track(self, gains, horizon, *args, **kw):
        return self.env.track(gains, horizon, *args, **kw)

    def speed_profile(self, *args, **kw):
        return self.env.speed_profile(*args, **kw)

    def path_speed(self, paths, lens, *args, **kw):
        return self.env.path_speed(paths, lens, *args, **kw)

    def get_state(self):
        return self.env.get_state()

    def set_state(self, state):
        self.env.set_state(state)

    def render(self, mode='human'):
        return self.env.render(mode)

    def close(self):
        self.env.close()
