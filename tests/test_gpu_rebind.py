"""One handle bound to geometry after geometry, and handles created and destroyed over and over: the library's own device
buffers must grow, be reused with stale tails behind the live part, and be given back, without a trace in the results."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N = 64
STEPS = 20
SEED = 11
RES = 0.1
X0 = 1.4   # where the paths start: the tricycle (0.37 m behind to 1.35 m ahead of its pose) stands clear of the left wall
# (map rows, map cols, way points): small, then everything larger, then the small one again in the larger buffers
PRIVATE = [(24, 40, 12), (72, 104, 60), (24, 40, 12)]
SHARED = [(40, 40, 12), (96, 96, 60), (40, 40, 12)]


def _geometry(rows, cols, n_pts, shared, count=N, x0=X0):
    """Walled rooms with a short wall across the robot's way.  Its distance from the robot's front differs from env to env:
    private maps put it 0.05, 0.25, ... 0.85 m ahead, on a shared map the envs start 0.05, 0.15, ... 0.75 m before it.  In
    STEPS steps of 0.05 s under the 0.4 m/s^2 acceleration limit a robot gets 0.15 to 0.2 m far: the nearest ones hit the
    wall, the others never reach it."""
    from bc_gym_planning_env_amd import CostMap2D
    y0 = 0.5 * rows * RES
    front = int((x0 + 1.348) / RES)   # the cell the front of a tricycle at x0 is in
    spacing = (cols * RES - x0 - 0.3) / n_pts

    def room(i):
        m = np.zeros((rows, cols), dtype=np.uint8)
        m[0, :] = m[-1, :] = m[:, 0] = m[:, -1] = 254
        m[rows // 2 - 2:rows // 2 + 3, front + 1 + 2 * (i % 5)] = 254
        m[1 + i % (rows - 2), cols - 2] = 254   # (no two private maps alike)
        return CostMap2D(m, RES, np.zeros(2))

    def path(i):
        start = x0 - (0.1 * (i % 8) if shared else 0.0)
        p = np.zeros((n_pts, 3))
        p[:, 0] = start + spacing * np.arange(n_pts)
        p[:, 1] = y0
        return p

    return (room(0) if shared else [room(i) for i in range(count)]), [path(i) for i in range(N if shared else count)]


def _actions(torch):
    a = torch.zeros((N, 2), dtype=torch.float64, device="cuda")
    a[:, 0] = torch.linspace(0.2, 0.5, N, dtype=torch.float64)
    a[:, 1] = torch.linspace(-0.5, 0.5, N, dtype=torch.float64)
    return a


def _fresh(geometry, shared, defer):
    from bc_gym_planning_env_amd import BatchedPlanEnv, EnvParams
    maps, paths = _geometry(*geometry, shared=shared)
    params = EnvParams(goal_spat_dist=0.2, goal_ang_dist=np.pi / 8, resolution=RES, refine_path=False)
    env = BatchedPlanEnv(maps, paths, params, n_envs=N, auto_reset=True, seed=SEED)
    if defer is not None:
        env.set_tuning(defer=defer)
    return env


def _rebind(env, geometry, shared):
    maps, paths = _geometry(*geometry, shared=shared)
    env._set_costmaps(maps)
    env._set_paths(paths)
    env._initial_state = env._make_initial_state()
    env._bind(env._initial_state, env._lib.bcp_bind_initial_state)


def _run(torch, env):
    """reset, STEPS steps, one egocentric observation -> everything the caller can see, as one dict of tensors"""
    from bc_gym_planning_env_amd.egocentric import BatchedEgocentricCostmap
    env.seed(SEED)
    env.reset()
    actions = _actions(torch)
    reward, done, collided = [], [], []
    for _ in range(STEPS):
        _o, r, d, _i = env.step(actions)
        reward.append(r.clone())
        done.append(d.clone())
        collided.append(env.collided_now.clone())
    ego = BatchedEgocentricCostmap(env, border_value=0)
    obs = ego.observation()
    out = dict(reward=torch.stack(reward), done=torch.stack(done), collided_now=torch.stack(collided),
               image=obs["env"].clone(), goal_n_state=obs["goal_n_state"].clone())
    state = env.get_state()
    for name in state.FIELDS:
        if getattr(state, name) is not None:
            out["state." + name] = getattr(state, name)
    torch.cuda.synchronize()
    return out, ego.route()["kernel"]


_REFERENCE = {}


def _reference(torch, geometry, shared, defer):
    """what a fresh env built directly on the geometry gives: computed once per configuration and left alone"""
    key = (geometry, shared, defer)
    if key not in _REFERENCE:
        env = _fresh(geometry, shared, defer)
        _REFERENCE[key] = _run(torch, env)
        env.close()
    return _REFERENCE[key]


@pytest.mark.parametrize("shared,defer", [(False, None), (False, 0), (True, None)],
                         ids=["private-default", "private-defer0", "shared-default"])
def test_grow_shrink_grow_on_one_handle(torch_cuda, shared, defer):
    torch = torch_cuda
    geometries = SHARED if shared else PRIVATE
    env = _fresh(geometries[0], shared, defer)
    for k, geometry in enumerate(geometries):
        if k:
            _rebind(env, geometry, shared)
        got, route = _run(torch, env)
        want, want_route = _reference(torch, geometry, shared, defer)
        hits = int(want["collided_now"].any(dim=0).sum())
        assert 0 < hits < N, "the scenario should drive some envs into the wall, not all: %d" % hits
        assert route == want_route == "ego_sparse_kernel", (route, want_route)
        assert sorted(got) == sorted(want)
        for name in sorted(want):
            assert torch.equal(got[name], want[name]), "bind %d (%r): %s differs from a fresh env" % (k, geometry, name)
    env.close()


# One handle across kinds of binding: a shared map, a geometry pool of three private maps, the shared map again.  What an
# owner inside the handle could carry over from the binding before -- a plan, a coarse copy, stale marks, parking slots,
# counters -- would show as a difference from a handle that has only ever seen the one geometry.
WIDE_ROOM = (24, 40, 12)     # rows, cols, way points: the shared map
SMALL_ROOM = (17, 33, 12)    # ... and each of the pool's three
POOL = 3
X0_SMALL = 0.6               # the tricycle's rear (0.37 m behind its pose) clears the left wall, its front stops short of column 20


def _pool_geometry():
    return _geometry(*SMALL_ROOM, shared=False, count=POOL, x0=X0_SMALL)


def _bind_pool(env):
    maps, paths = _pool_geometry()
    env._set_geometry_pool(POOL, np.arange(N) % POOL, None)
    env._set_from_templates(maps, paths, None)
    env._initial_state = env._make_initial_state()
    env._bind(env._initial_state, env._lib.bcp_bind_initial_state)


def _bind_shared(env):
    from bc_gym_planning_env_amd import _lib
    _lib.check(env._lib.bcp_set_geometry_pool(env._h, 0, None, None))
    env.geom_of_env = None
    _rebind(env, WIDE_ROOM, True)


def _fresh_kind(kind, **tuning):
    from bc_gym_planning_env_amd import BatchedPlanEnv, EnvParams
    params = EnvParams(goal_spat_dist=0.2, goal_ang_dist=np.pi / 8, resolution=RES, refine_path=False)
    if kind == "pool":
        maps, paths = _pool_geometry()
        env = BatchedPlanEnv(maps, paths, params, n_envs=N, auto_reset=True, seed=SEED, geom_of_env=np.arange(N) % POOL)
    else:
        maps, paths = _geometry(*WIDE_ROOM, shared=True)
        env = BatchedPlanEnv(maps, paths, params, n_envs=N, auto_reset=True, seed=SEED)
    env.set_tuning(**tuning)
    return env


def _run_steps(torch, env):
    """reset, STEPS steps -> state, reward, done and collided_now of every step, as one dict of tensors"""
    env.seed(SEED)
    env.reset()
    actions = _actions(torch)
    reward, done, collided = [], [], []
    for _ in range(STEPS):
        _o, r, d, _i = env.step(actions)
        reward.append(r.clone())
        done.append(d.clone())
        collided.append(env.collided_now.clone())
    out = dict(reward=torch.stack(reward), done=torch.stack(done), collided_now=torch.stack(collided))
    state = env.get_state()
    for name in state.FIELDS:
        if getattr(state, name) is not None:
            out["state." + name] = getattr(state, name)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("fused", [None, 0], ids=["default", "fused0"])
def test_shared_pool_shared_on_one_handle(torch_cuda, fused):
    """shared 40 x 24 map -> pool of three private 33 x 17 maps -> the shared map again, 20 steps after each bind, bit for
    bit what a fresh handle bound once to that geometry with the same tuning gives.  Between the first two binds culling is
    switched off and on again; before the third BCP_TUNE_NEAR_SHIFT is set to 0 (in force from that bind on; a shared map
    has no coarse copy, so the pool's copy at a quarter of the resolution must be left behind)."""
    torch = torch_cuda
    form = {} if fused is None else dict(fused=fused)
    env = _fresh_kind("shared", **form)
    want_form = "step_local_kernel" if fused is None else "step_fast_pair_kernel + step_pending_kernel"
    for k, kind in enumerate(("shared", "pool", "shared")):
        tuning = dict(form)
        if k == 1:
            env.set_tuning(cull=0)
            env.set_tuning(cull=1)
            _bind_pool(env)
        elif k == 2:
            env.set_tuning(near_shift=0)
            tuning["near_shift"] = 0
            _bind_shared(env)
        got = _run_steps(torch, env)
        assert env.step_kernels().startswith(want_form), (kind, env.step_kernels())
        fresh = _fresh_kind(kind, **tuning)
        want = _run_steps(torch, fresh)
        fresh.close()
        hits = int(want["collided_now"].any(dim=0).sum())
        assert 0 < hits < N, "the scenario should drive some envs into the wall, not all: %d" % hits
        assert sorted(got) == sorted(want)
        for name in sorted(want):
            assert torch.equal(got[name], want[name]), "bind %d (%s): %s differs from a fresh handle" % (k, kind, name)
    env.close()


def test_create_destroy_gives_the_memory_back(torch_cuda):
    torch = torch_cuda
    from bc_gym_planning_env_amd.mini_env import BatchedRandomMiniEnv, sample_pool_device
    from bc_gym_planning_env_amd.egocentric import BatchedEgocentricCostmap

    def free_now():
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        return torch.cuda.mem_get_info()[0]

    pool = sample_pool_device(seeds=range(16), episodes=2)   # (a small pool, sampled once: the cycles are about the handle)

    def cycle(alive=None):
        env = BatchedRandomMiniEnv(256, pool=pool, auto_reset=True, seed=3)
        env.enable_episode_record()
        actions = torch.zeros((256, 2), dtype=torch.float64, device="cuda")
        actions[:, 0] = 0.3
        for _ in range(4):
            env.step(actions)
        BatchedEgocentricCostmap(env).observation()
        side = C.c_void_p()
        assert env._lib.bcp_side_stream(env._h, 50, C.byref(side)) == 0 and side.value
        torch.cuda.synchronize()
        if alive is not None:
            alive.append(torch.cuda.mem_get_info()[0])
        env.close()
        del env, actions
        return free_now()

    cycle()   # (the process's one-time allocations: code objects, the caching allocator's first blocks)
    before, alive = free_now(), []
    free = {1: cycle(alive)}
    footprint = before - alive[0]
    assert footprint > 0, "an env that is alive takes device memory: %d" % footprint
    for k in range(2, 21):
        free[k] = cycle()
    print("footprint %d bytes, free after cycle 2: %d, after cycle 20: %d" % (footprint, free[2], free[20]))
    # a handle that leaked all of it would lose 18 footprints between the two, one that leaks nothing loses none
    assert free[20] >= free[2] - footprint, (free[2], free[20], footprint)
