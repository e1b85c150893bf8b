"""Resets from a declared uniform initial state (bcp_declare_uniform_initial_state): the finishing pass of step_local_kernel's
shared-geometry variant then takes the initial state from the LDS copy of the parameter block instead of loading the eleven
initial-state arrays.

What can go wrong there: two fields of the block swapped or one left out (the stock initial state has six zero fields, so the
test binds one of its own), the tricycle's two values restored for a diff-drive robot, the block read by a launch that was not
declared, a stale snapshot after a re-bind, lanes that reset beside lanes that do not.  g8_traj_mini_00 geometry, 293 envs (one
full workgroup and a ragged one) and 1 env, 48 steps, iteration_timeout 40; envs 64 .. 95 start on the last four way points, so
that episodes end for every reason -- time-out, collision, goal -- and waves hold resetting and non-resetting lanes side by
side.  Declared against undeclared against the generic variant bit for bit, and against the oracle fed the device's normals."""
import os

import numpy as np
import pytest

from util import ATOL, GOLDEN, random_batch, z_in

pytestmark = pytest.mark.gpu

NAME = "g8_traj_mini_00.npz"
SIZES, STEPS, TIMEOUT = (293, 1), 48, 40
SP, AP = 0.2, np.pi / 8
# (the suite also runs with smaller workgroups for every handle, BCP_LOCAL_PAIRS = 1 | 2: those have the generic variant only)
LARGE_WORKGROUPS = os.environ.get("BCP_LOCAL_PAIRS", "4") not in ("1", "2")
STATE_KEYS = ("robot", "min_dist", "target_idx", "current_iter", "robot_collided")


def make_env(g, n, model):
    from bc_gym_planning_env_amd import BatchedPlanEnv, CostMap2D, EnvParams
    res = float(g["resolution"])
    extra = {} if model == "tricycle" else dict(robot_name='industrial_diffdrive_v1')
    params = EnvParams(goal_spat_dist=SP, goal_ang_dist=AP, resolution=res, refine_path=False, iteration_timeout=TIMEOUT, **extra)
    return BatchedPlanEnv(CostMap2D(g["costmap"], res, g["origin"]), g["path"], params, n_envs=n,
                          noise_parameters='planenv' if model == "tricycle" else None, auto_reset=True, seed=123)


def start_states(oracle, g, n):
    """util.random_batch with the time-out of this test; envs 64 .. 95 on the path's last four way points, moving"""
    st, md, tgt, it = random_batch(oracle, np.random.RandomState(7), n, g, NAME, timeout=TIMEOUT)
    path = g["path"]
    last = len(path)
    for k in range(64, min(96, n)):
        wp = last - 1 - (k % 4)
        st[:, k] = 0.0
        st[0:3, k] = path[wp]
        st[3, k] = 0.3
        tgt[k], md[k], it[k] = wp, 0.0, 0
    return st, md, tgt, it


class World(object):
    """one handle of n envs with its start state and the 48 actions, float64 and rounded to float32"""

    def __init__(self, torch, oracle, n, model):
        self.n, self.model = n, model
        self.g = np.load(os.path.join(GOLDEN, NAME))
        self.env = make_env(self.g, n, model)
        self.start = start_states(oracle, self.g, n)
        rng = np.random.RandomState(11)
        a64 = np.stack([self.env.action_space.sample_batch(n, rng) for _ in range(STEPS)])
        self.actions = {"float64": torch.from_numpy(a64).cuda(), "float32": torch.from_numpy(a64.astype(np.float32)).cuda()}
        self.refs = {}

    def put(self, torch):
        env = self.env
        st, md, tgt, it = self.start
        env.state.robot.copy_(torch.from_numpy(st))
        env.state.min_spat_dist_so_far.copy_(torch.from_numpy(md))
        env.state.target_idx.copy_(torch.from_numpy(tgt))
        env.state.current_iter.copy_(torch.from_numpy(it))
        env.state.robot_collided.zero_()
        env.seed(123)


def _state_row(env):
    return dict(robot=env.state.robot.clone(), min_dist=env.state.min_spat_dist_so_far.clone(),
                target_idx=env.state.target_idx.clone(), current_iter=env.state.current_iter.clone(),
                robot_collided=env.state.robot_collided.clone())


def _run(torch, w, dtype, declared, shared=1, steps=STEPS):
    """`steps` steps from the start state -> per step the state arrays, reward, done, collided_now, err and the drawn normals"""
    env, n = w.env, w.n
    env.set_tuning(local_shared=shared)
    env.declare_uniform_initial_state(declared)
    w.put(torch)
    z = torch.full((n, 3), float("nan"), dtype=torch.float64, device="cuda")
    rows = []
    for t in range(steps):
        _, rew, done, _ = env.step(w.actions[dtype][t], noise_z_out=z)
        assert env.step_uniform_reset() == (bool(declared) and bool(shared) and LARGE_WORKGROUPS)
        assert env.step_shared_variant() == (bool(shared) and LARGE_WORKGROUPS)
        rows.append(dict(_state_row(env), reward=rew.clone(), done=done.clone(), collided_now=env.collided_now.clone(),
                         err=env.err.clone(), z=z.clone()))
    env.check_errors()
    return rows


def _same(torch, rows, want, what):
    assert len(rows) == len(want)
    for t, (s, g) in enumerate(zip(rows, want)):
        for key in s:
            a, b = s[key], g[key]
            if a.dtype == torch.float64:   # (NaN marks a normal that was not drawn, and -0.0 is not 0.0: compare the bits)
                a, b = a.view(torch.int64), b.view(torch.int64)
            assert torch.equal(a, b), ("%s step %d" % (what, t), key)


def _oracle_rows(oracle, w, dtype, zs):
    """the oracle's 48 steps from the same start, fed the normals the device drew"""
    g, n = w.g, w.n
    p = oracle.make_params(w.model, noise=oracle.PLANENV_NOISE if w.model == "tricycle" else None, spatial_precision=SP,
                           angular_precision=AP, iteration_timeout=TIMEOUT)
    ref = oracle.OracleBatch(p, n, g["costmap"], g["origin"], float(g["resolution"]), g["path"])
    ref.reset_from_paths()
    st, md, tgt, it = w.start
    for f in range(7):
        ref.st[f][:] = st[f]
    ref.min_dist[:], ref.target_idx[:], ref.cur_iter[:] = md, tgt, it
    rows = []
    acts = w.actions[dtype].cpu().numpy().astype(np.float64)
    for t in range(STEPS):
        ref.step(acts[t], z_in(zs[t]), auto_reset=True, threads=8)
        rows.append(dict(robot=np.stack(ref.st).copy(), min_dist=ref.min_dist.copy(), target_idx=ref.target_idx.copy(),
                         current_iter=ref.cur_iter.copy(), robot_collided=ref.collided.copy(), reward=ref.reward.copy(),
                         done=ref.done.copy(), collided_now=ref.collided_now.copy()))
    return rows


def _against_oracle(w, rows, ref, what):
    live = 7 if w.model == "tricycle" else 5   # (a diff-drive robot has no steering column: rows 5 and 6 are nobody's)
    for t, (s, o) in enumerate(zip(rows, ref)):
        msg = "%s step %d" % (what, t)
        for key in ("done", "collided_now", "target_idx", "current_iter", "robot_collided"):
            np.testing.assert_array_equal(s[key].cpu().numpy(), o[key], err_msg="%s %s" % (msg, key))
        np.testing.assert_allclose(s["robot"].cpu().numpy()[:live], o["robot"][:live], rtol=0, atol=ATOL, err_msg=msg)
        for key in ("reward", "min_dist"):
            np.testing.assert_allclose(s[key].cpu().numpy(), o[key], rtol=0, atol=ATOL, err_msg="%s %s" % (msg, key))
        assert not bool(s["err"].any()), msg


def _ends(w, rows):
    """-> (time-out ends, collision ends, goal ends, waves that hold resetting and non-resetting lanes) over the run"""
    it = w.start[3].copy()
    sticky = np.zeros(w.n, dtype=bool)
    timeouts = collisions = goals = mixed = 0
    for s in rows:
        done = s["done"].cpu().numpy() != 0
        hit = (s["collided_now"].cpu().numpy() != 0) | sticky
        late = it + 1 >= TIMEOUT
        timeouts += int((done & late).sum())
        collisions += int((done & hit).sum())
        goals += int((done & ~late & ~hit).sum())
        for lo in range(0, w.n, 64):
            lanes = done[lo:lo + 64]
            mixed += int(0 < lanes.sum() < len(lanes))
        it = s["current_iter"].cpu().numpy().copy()
        sticky = s["robot_collided"].cpu().numpy() != 0
    return timeouts, collisions, goals, mixed


@pytest.fixture(scope="module")
def worlds(torch_cuda, oracle):
    made = {}

    def get(n, model):
        if (n, model) not in made:
            made[(n, model)] = World(torch_cuda, oracle, n, model)
        return made[(n, model)]
    return get


def _reference(torch, oracle, w, dtype):
    """(undeclared rows of the shared variant, oracle's rows): computed once per world and action type, shared, never written to"""
    if dtype not in w.refs:
        undeclared = _run(torch, w, dtype, False)
        w.refs[dtype] = (undeclared, _oracle_rows(oracle, w, dtype, [r["z"].cpu().numpy() for r in undeclared]))
    return w.refs[dtype]


# ---- case 1
@pytest.mark.parametrize("model,dtype", [("tricycle", "float64"), ("tricycle", "float32"), ("diffdrive", "float64")])
def test_declared_against_undeclared_the_generic_variant_and_the_oracle(torch_cuda, oracle, worlds, model, dtype):
    torch = torch_cuda
    for n in SIZES:
        w = worlds(n, model)
        undeclared, ref = _reference(torch, oracle, w, dtype)
        what = "%s %s n=%d" % (model, dtype, n)
        if n > 1:
            timeouts, collisions, goals, mixed = _ends(w, undeclared)
            print("%s: %d time-out ends, %d collision ends, %d goal ends, %d mixed waves" % (what, timeouts, collisions, goals, mixed))
            assert timeouts >= 300 and collisions >= 30 and goals >= 3 and mixed >= 100
        declared = _run(torch, w, dtype, True)
        _same(torch, declared, undeclared, what + " declared")
        generic = _run(torch, w, dtype, True, shared=0)   # (declared: the flag never reaches the generic variant)
        _same(torch, generic, undeclared, what + " generic")
        _against_oracle(w, declared, ref, what)
        if model == "diffdrive":   # steering command and wheel angle are not the robot's: whatever the arrays held stays
            for s in declared:
                assert torch.equal(s["robot"][5:7], torch.from_numpy(w.start[0][5:7]).cuda())
            if n > 1:
                assert int((w.start[0][6] != 0.0).sum()) > 200   # (the wheel row is not the snapshot's 0.0 for most envs)


# ---- cases 2 and 3: an initial state of the test's own
def own_initial_state(torch, w, collided=0, per_env=False):
    """every field non-zero and distinct from every other (the stock state has six zeros: a swapped pair would not show);
    per_env: a different state for every env"""
    from bc_gym_planning_env_amd.state import BatchedState
    n, path = w.n, w.g["path"]
    robot = np.zeros((7, n))
    robot[0:3] = (path[5] + np.array([0.031, -0.017, 0.052]))[:, None]
    robot[3], robot[4], robot[5], robot[6] = 0.21, -0.13, 0.07, 0.11
    md, tgt, it = np.full(n, 0.37), np.full(n, 7, dtype=np.int32), np.full(n, 2, dtype=np.int32)
    if per_env:
        k = np.arange(n)
        robot[0] += 0.001 * k
        robot[3] += 0.0003 * k
        robot[6] -= 0.0002 * k
        md += 0.0005 * k
        tgt += (k % 3).astype(np.int32)
        it += (k % 5).astype(np.int32)
    return BatchedState(torch.from_numpy(robot).cuda(), torch.from_numpy(md).cuda(), torch.from_numpy(tgt).cuda(),
                        torch.from_numpy(it).cuda(), torch.full((n,), collided, dtype=torch.uint8, device="cuda"))


def _bind_own(w, state):
    w.env._bind(state, w.env._lib.bcp_bind_initial_state)   # (a plain bind: drops any declaration)


def _restore(w):
    w.env._bind_initial_state()
    w.env.set_tuning(local_shared=1)


def _resets_restore(torch, w, rows, init):
    """wherever an env was done, the state after the step is its entry of `init`; -> how many"""
    live = 7 if w.model == "tricycle" else 5
    count = 0
    for t, s in enumerate(rows):
        done = s["done"] != 0
        count += int(done.sum())
        assert torch.equal(s["robot"][:live][:, done].view(torch.int64), init.robot[:live][:, done].view(torch.int64)), t
        assert torch.equal(s["min_dist"][done], init.min_spat_dist_so_far[done]) and torch.equal(s["target_idx"][done], init.target_idx[done])
        assert torch.equal(s["current_iter"][done], init.current_iter[done]) and torch.equal(s["robot_collided"][done], init.robot_collided[done])
    return count


@pytest.mark.parametrize("model", ["tricycle", "diffdrive"])
def test_a_non_stock_initial_state(torch_cuda, oracle, worlds, model):
    torch = torch_cuda
    for n in SIZES:
        w = worlds(n, model)
        init = own_initial_state(torch, w)
        try:
            _bind_own(w, init)
            undeclared = _run(torch, w, "float64", False)
            declared = _run(torch, w, "float64", True)
            _same(torch, declared, undeclared, "%s n=%d" % (model, n))
            ended = _resets_restore(torch, w, declared, init)
            assert ended > (300 if n > 1 else 0)
        finally:
            _restore(w)


def test_an_initial_state_that_has_collided(torch_cuda, oracle):
    """a second handle whose every env ends again in the step after its reset: all eleven fields non-zero and distinct"""
    torch = torch_cuda
    w = World(torch, oracle, SIZES[0], "tricycle")
    init = own_initial_state(torch, w, collided=1)
    _bind_own(w, init)
    undeclared = _run(torch, w, "float64", False)
    declared = _run(torch, w, "float64", True)
    _same(torch, declared, undeclared, "collided")
    _resets_restore(torch, w, declared, init)
    for t in range(1, STEPS):   # whoever ended ends again
        assert bool(declared[t]["done"][declared[t - 1]["done"] != 0].all()), t
    assert int(declared[-1]["done"].sum()) > 200


# ---- case 4
def test_the_life_cycle_of_a_declaration(torch_cuda, oracle, worlds):
    from bc_gym_planning_env_amd import _lib
    torch = torch_cuda
    n = SIZES[0]
    w = worlds(n, "tricycle")
    env = w.env
    try:
        # (a) an array that is not uniform is refused, the handle stays undeclared and steps on the arrays
        init = own_initial_state(torch, w)
        init.robot[0, 100] += 1e-9
        _bind_own(w, init)
        with pytest.raises(_lib.BcpError) as refusal:
            env.declare_uniform_initial_state(True)
        assert "error -1" in str(refusal.value) and "env 100 " in str(refusal.value) and " in x " in str(refusal.value)
        env.set_tuning(local_shared=1)
        w.put(torch)
        rows = []
        for t in range(STEPS):
            _, rew, done, _ = env.step(w.actions["float64"][t])
            assert not env.step_uniform_reset()
            rows.append(dict(_state_row(env), done=done.clone()))
        assert _resets_restore(torch, w, rows, init) > 300
        assert any(bool(s["done"][100]) for s in rows)
        #     ... a refusal also drops a declaration that stood
        init.robot[0, 100] = init.robot[0, 0]
        env.declare_uniform_initial_state(True)
        init.current_iter[n - 1] += 1
        with pytest.raises(_lib.BcpError) as refusal:
            env.declare_uniform_initial_state(True)
        assert "env %d " % (n - 1) in str(refusal.value) and " in current_iter " in str(refusal.value)
        env.step(w.actions["float64"][0])
        assert not env.step_uniform_reset()
        #     ... words, not values: a NaN of another payload, a zero of the other sign (arrays that no step ever reads)
        odd = own_initial_state(torch, w)
        _bind_own(w, odd)
        odd.robot[4].fill_(float("nan"))
        env.declare_uniform_initial_state(True)
        odd.robot[4].view(torch.int64)[17] ^= 1
        assert bool(torch.isnan(odd.robot[4]).all())
        with pytest.raises(_lib.BcpError) as refusal:
            env.declare_uniform_initial_state(True)
        assert "env 17 " in str(refusal.value) and " in w " in str(refusal.value)
        odd.robot[4].fill_(0.0)
        env.declare_uniform_initial_state(True)
        odd.robot[4, n - 1] = -0.0
        with pytest.raises(_lib.BcpError) as refusal:
            env.declare_uniform_initial_state(True)
        assert "env %d " % (n - 1) in str(refusal.value) and " in w " in str(refusal.value)

        # (b) a plain re-bind to a state per env after a declaration: the next steps use the arrays
        _bind_own(w, own_initial_state(torch, w))
        env.declare_uniform_initial_state(True)
        env.step(w.actions["float64"][0])
        assert env.step_uniform_reset() == LARGE_WORKGROUPS
        distinct = own_initial_state(torch, w, per_env=True)
        _bind_own(w, distinct)
        w.put(torch)
        rows = []
        for t in range(STEPS):
            _, rew, done, _ = env.step(w.actions["float64"][t])
            assert not env.step_uniform_reset()
            rows.append(dict(_state_row(env), done=done.clone()))
        assert _resets_restore(torch, w, rows, distinct) > 300
        with pytest.raises(_lib.BcpError):
            env.declare_uniform_initial_state(True)

        # (c) declared, the arrays rewritten in place, declared again: the new values are used
        init = own_initial_state(torch, w)
        _bind_own(w, init)
        env.declare_uniform_initial_state(True)
        init.robot[0] += 0.01
        init.robot[3].fill_(0.17)
        init.min_spat_dist_so_far.fill_(0.29)
        init.target_idx.fill_(9)
        init.current_iter.fill_(3)
        rows = _run(torch, w, "float64", True)   # (declares again)
        assert _resets_restore(torch, w, rows, init) > 300

        # (d) on = 0
        off = _run(torch, w, "float64", False)
        _same(torch, off, rows, "on = 0")
        env.step(w.actions["float64"][0])
        assert not env.step_uniform_reset()
    finally:
        _restore(w)

    # (e) a handle with a geometry pool is refused
    from bc_gym_planning_env_amd import BatchedPlanEnv, CostMap2D, EnvParams
    g = w.g
    res = float(g["resolution"])
    cm = CostMap2D(g["costmap"], res, g["origin"])
    params = EnvParams(goal_spat_dist=SP, goal_ang_dist=AP, resolution=res, refine_path=False, iteration_timeout=TIMEOUT)
    pool = BatchedPlanEnv([cm, cm], [g["path"], g["path"]], params, n_envs=4, geom_of_env=[0, 1, 0, 1], auto_reset=True)
    with pytest.raises(_lib.BcpError) as refusal:
        pool.declare_uniform_initial_state(True)
    assert "error -4" in str(refusal.value)
    pool.step(w.actions["float64"][0][:4].contiguous())
    assert not pool.step_uniform_reset()
    pool.check_errors()


# ---- case 5
def test_with_an_episode_record_bound(torch_cuda, oracle, worlds):
    torch = torch_cuda
    for n in SIZES:
        w = worlds(n, "tricycle")
        undeclared, _ref = _reference(torch, oracle, w, "float64")
        env = w.env
        ends = env.enable_episode_record()
        try:
            per_run = []
            for declared in (True, False):
                env.set_tuning(local_shared=1)
                env.declare_uniform_initial_state(declared)
                w.put(torch)
                ends.ret.zero_()
                seen = []
                for t in range(STEPS):
                    _, rew, done, info = env.step(w.actions["float64"][t])
                    assert info["episode_ends"] is ends
                    assert env.step_uniform_reset() == (declared and LARGE_WORKGROUPS)
                    k = int(ends.count[0])
                    order = torch.argsort(ends.env_ids[:k])
                    fin = ends.final_state
                    seen.append(dict(_state_row(env), reward=rew.clone(), done=done.clone(), reason=ends.reason.clone(),
                                     ret=ends.ret.clone(), count=ends.count.clone(), env_ids=ends.env_ids[:k][order].clone(),
                                     final_robot=fin.robot[:, :k][:, order].clone(),
                                     final_min_dist=fin.min_spat_dist_so_far[:k][order].clone(),
                                     final_target=fin.target_idx[:k][order].clone(), final_iter=fin.current_iter[:k][order].clone(),
                                     final_collided=fin.robot_collided[:k][order].clone(),
                                     final_return=ends.final_return[:k][order].clone()))
                env.check_errors()
                per_run.append(seen)
            _same(torch, per_run[0], per_run[1], "record n=%d" % n)
            for t, s in enumerate(per_run[0]):
                for key in STATE_KEYS + ("reward", "done"):
                    assert torch.equal(s[key], undeclared[t][key]), (n, t, key)   # (... and the record changes no result)
                assert int(s["count"][0]) == int(s["done"].sum())
            if n > 1:
                reasons = torch.stack([s["reason"] for s in per_run[0]])
                for bit in (ends.GOAL, ends.TIMEOUT, ends.COLLIDED):
                    assert int((reasons & bit != 0).sum()) > 0
        finally:
            env.disable_episode_record()
            _restore(w)


# ---- case 6
def test_eight_steps_captured_into_one_graph(torch_cuda, oracle, worlds):
    torch = torch_cuda
    n, k = SIZES[0], 8
    w = worlds(n, "tricycle")
    env = w.env
    try:
        live = _run(torch, w, "float64", True, steps=k)
        a_static = w.actions["float64"][:k].clone()
        ring = torch.full((k, n), 9, dtype=torch.uint8, device="cuda")
        env.step(a_static[0])                              # an ordinary step first: uploads the parameter block
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.stream(side):
            with torch.cuda.graph(graph, stream=side):
                for t in range(k):
                    env.step(a_static[t], done_out=ring[t])
        torch.cuda.current_stream().wait_stream(side)
        assert env.step_uniform_reset() == LARGE_WORKGROUPS
        w.put(torch)                                       # (capture does not execute)
        graph.replay()
        torch.cuda.synchronize()
        row = dict(_state_row(env), reward=env.reward, collided_now=env.collided_now)
        for key in row:
            assert torch.equal(row[key], live[k - 1][key]), key
        assert torch.equal(ring, torch.stack([r["done"] for r in live]))
        assert int(ring.sum()) > 0
        env.check_errors()
    finally:
        _restore(w)
