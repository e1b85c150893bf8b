"""The finishing pass of step_local_kernel's shared-geometry variant: it takes the launch's output pointers and flags from
a copy in LDS and the state arrays from the LDS copy of the parameter block, read in one batch ahead of the verdicts.

What can go wrong there: an optional output treated as present (or the other way round), a pointer of an earlier launch
used again, the flags of the launch misread (action type, auto-reset, episode record), a captured launch that replays
stale words.  293 envs (one full workgroup and a ragged one) and 1 env on the g8_traj_mini_00 geometry, 48 steps, bit for
bit against the generic variant (BCP_TUNE_LOCAL_SHARED = 0) and against the oracle fed the normals the device drew."""
import itertools
import os

import numpy as np
import pytest

from util import ATOL, GOLDEN, env_from_traj, oracle_params_for, random_batch, z_in

pytestmark = pytest.mark.gpu

NAME = "g8_traj_mini_00.npz"
SIZES, STEPS = (293, 1), 48
# (the suite also runs with smaller workgroups for every handle, BCP_LOCAL_PAIRS = 1 | 2: those have the generic variant only)
LARGE_WORKGROUPS = os.environ.get("BCP_LOCAL_PAIRS", "4") not in ("1", "2")
STATE_KEYS = ("robot", "min_dist", "target_idx", "current_iter", "robot_collided")


class World(object):
    """one handle of n envs with its start state and the 48 actions, float64 and rounded to float32"""

    def __init__(self, torch, oracle, n):
        self.n = n
        self.g = np.load(os.path.join(GOLDEN, NAME))
        self.env = env_from_traj(self.g, NAME, n_envs=n, auto_reset=True, seed=123)
        self.start = random_batch(oracle, np.random.RandomState(7), n, self.g, NAME)
        rng = np.random.RandomState(11)
        a64 = np.stack([self.env.action_space.sample_batch(n, rng) for _ in range(STEPS)])
        self.actions = {"float64": torch.from_numpy(a64).cuda(), "float32": torch.from_numpy(a64.astype(np.float32)).cuda()}
        self.refs = {}

    def put(self, torch, env=None):
        env = env or self.env
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


def _run(torch, w, dtype, shared, collided_now=True, err=True, zout=True, done_ring=None):
    """STEPS steps from the start state -> per step, the state arrays and the outputs that were asked for (device tensors).
    An output that is left out must stay as it was: its buffer holds a sentinel throughout."""
    env, n = w.env, w.n
    env.set_tuning(local_shared=shared)
    w.put(torch)
    z = torch.full((n, 3), float("nan"), dtype=torch.float64, device="cuda") if zout else None
    env.collided_now.fill_(7)
    env.err.fill_(-5)
    # (BatchedPlanEnv always binds the two: the library takes either as absent when its pointer is null)
    env._io.collided_now = env.collided_now.data_ptr() if collided_now else None
    env._io.err = env.err.data_ptr() if err else None
    if done_ring is not None:
        env.done.fill_(5)
    rows = []
    try:
        for t in range(STEPS):
            _, rew, done, _ = env.step(w.actions[dtype][t], noise_z_out=z, done_out=None if done_ring is None else done_ring[t])
            assert env.step_shared_variant() == (bool(shared) and LARGE_WORKGROUPS)
            row = _state_row(env)
            row.update(reward=rew.clone(), done=done.clone())
            if collided_now:
                row["collided_now"] = env.collided_now.clone()
            if err:
                row["err"] = env.err.clone()
            if zout:
                row["z"] = z.clone()
            rows.append(row)
        if not collided_now:
            assert bool((env.collided_now == 7).all())
        if not err:
            assert bool((env.err == -5).all())
        if done_ring is not None:
            assert bool((env.done == 5).all())
    finally:
        env._io.collided_now = env.collided_now.data_ptr()
        env._io.err = env.err.data_ptr()
    if not err:
        env.err.zero_()   # (the sentinel is no error word)
    env.check_errors()
    return rows


def _oracle_rows(oracle, w, dtype, zs):
    """the oracle's 48 steps from the same start, fed the normals the device drew"""
    g, n = w.g, w.n
    ref = oracle.OracleBatch(oracle_params_for(oracle, NAME), n, g["costmap"], g["origin"], float(g["resolution"]), g["path"])
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


@pytest.fixture(scope="module")
def worlds(torch_cuda, oracle):
    return dict((n, World(torch_cuda, oracle, n)) for n in SIZES)


def _reference(torch, oracle, w, dtype):
    """(generic variant's rows, oracle's rows) for this world and action type: computed once, shared, never written to"""
    if dtype not in w.refs:
        generic = _run(torch, w, dtype, 0)
        w.refs[dtype] = (generic, _oracle_rows(oracle, w, dtype, [r["z"].cpu().numpy() for r in generic]))
    return w.refs[dtype]


def _check(torch, rows, generic, ref, what):
    for t, (s, g, o) in enumerate(zip(rows, generic, ref)):
        msg = "%s step %d" % (what, t)
        for key in s:
            if key == "z":   # (NaN marks a slot that was not drawn: compare the bits)
                assert torch.equal(s[key].view(torch.int64), g[key].view(torch.int64)), (msg, key)
            else:
                assert torch.equal(s[key], g[key]), (msg, key)
        for key in ("done", "collided_now", "target_idx", "current_iter", "robot_collided"):
            if key in s:
                np.testing.assert_array_equal(s[key].cpu().numpy(), o[key], err_msg="%s %s" % (msg, key))
        for key in ("robot", "reward", "min_dist"):
            np.testing.assert_allclose(s[key].cpu().numpy(), o[key], rtol=0, atol=ATOL, err_msg="%s %s" % (msg, key))
        if "err" in s:
            assert not bool(s["err"].any()), msg


OPTIONAL = list(itertools.product((False, True), repeat=3))


@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("collided_now,err,zout", OPTIONAL, ids=["".join("cez"[k] if on else "-" for k, on in enumerate(c)) for c in OPTIONAL])
def test_every_combination_of_optional_outputs(torch_cuda, oracle, worlds, dtype, collided_now, err, zout):
    torch = torch_cuda
    for n in SIZES:
        w = worlds[n]
        generic, ref = _reference(torch, oracle, w, dtype)
        rows = _run(torch, w, dtype, 1, collided_now=collided_now, err=err, zout=zout)
        _check(torch, rows, generic, ref, "n=%d %s" % (n, dtype))
        if n > 1:   # (episodes end and poses are rolled back, so resets and hits go through the pass)
            assert sum(int(r["done"].sum()) for r in generic) > 0 and sum(int(r["collided_now"].sum()) for r in generic) > 0
            assert w.env.parked_poses() > 0


def test_done_written_to_a_different_row_every_step(torch_cuda, oracle, worlds):
    """bench.py's sharded runs hand a row of a ring to every step: each row holds exactly its step's mask"""
    torch = torch_cuda
    for n in SIZES:
        w = worlds[n]
        generic, ref = _reference(torch, oracle, w, "float64")
        ring = torch.full((STEPS, n), 9, dtype=torch.uint8, device="cuda")
        rows = _run(torch, w, "float64", 1, done_ring=ring)   # (asserts env.done untouched)
        _check(torch, rows, generic, ref, "ring n=%d" % n)
        assert torch.equal(ring, torch.stack([r["done"] for r in generic]))
        for t in range(STEPS):
            np.testing.assert_array_equal(ring[t].cpu().numpy(), ref[t]["done"], err_msg="row %d" % t)


def test_with_an_episode_record_bound(torch_cuda, oracle, worlds):
    """the record is reached through the launch's flags and the parameter block in global memory"""
    torch = torch_cuda
    for n in SIZES:
        w = worlds[n]
        generic, ref = _reference(torch, oracle, w, "float64")
        ends = w.env.enable_episode_record()
        try:
            per_variant = []
            for shared in (1, 0):
                w.env.set_tuning(local_shared=shared)
                w.put(torch)
                ends.ret.zero_()
                seen = []
                for t in range(STEPS):
                    _, rew, done, info = w.env.step(w.actions["float64"][t])
                    assert info["episode_ends"] is ends
                    assert w.env.step_shared_variant() == (bool(shared) and LARGE_WORKGROUPS)
                    k = int(ends.count[0])
                    order = torch.argsort(ends.env_ids[:k])
                    seen.append(dict(_state_row(w.env), reward=rew.clone(), done=done.clone(), reason=ends.reason.clone(),
                                     ret=ends.ret.clone(), env_ids=ends.env_ids[:k][order].clone(),
                                     final_robot=ends.final_state.robot[:, :k][:, order].clone(),
                                     final_iter=ends.length[:k][order].clone(), final_return=ends.final_return[:k][order].clone()))
                w.env.check_errors()
                per_variant.append(seen)
            for t, (s, g) in enumerate(zip(*per_variant)):
                for key in s:
                    assert torch.equal(s[key], g[key]), (n, t, key)
                for key in STATE_KEYS + ("reward", "done"):
                    assert torch.equal(s[key], generic[t][key]), (n, t, key)   # (... and the record changes no result)
                want = np.nonzero(ref[t]["done"])[0]
                np.testing.assert_array_equal(s["env_ids"].cpu().numpy(), want, err_msg="step %d" % t)
                np.testing.assert_array_equal(s["reason"].cpu().numpy() != 0, ref[t]["done"] != 0, err_msg="step %d" % t)
        finally:
            w.env.disable_episode_record()


def test_a_step_replayed_from_a_captured_graph(torch_cuda, oracle, worlds):
    """A captured launch carries its arguments with it: replays write this launch's outputs, step after step, exactly as
    launched steps of the generic variant do."""
    torch = torch_cuda
    n = SIZES[0]
    w = worlds[n]
    generic, ref = _reference(torch, oracle, w, "float64")
    env = w.env
    env.set_tuning(local_shared=1)
    a_static = w.actions["float64"][0].clone()
    env.step(a_static)                                 # an ordinary step first: uploads the parameter block
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            env.step(a_static)
    torch.cuda.current_stream().wait_stream(side)
    w.put(torch)                                       # (capture does not execute)
    for t in range(STEPS):
        a_static.copy_(w.actions["float64"][t])
        graph.replay()
        torch.cuda.synchronize()
        row = dict(_state_row(env), reward=env.reward, done=env.done, collided_now=env.collided_now)
        for key in row:
            assert torch.equal(row[key], generic[t][key]), (t, key)
    assert env.step_shared_variant() == LARGE_WORKGROUPS
    env.check_errors()
