"""The step kernels at the limits of their LDS staging: shared paths of 38 .. 615 way points (one double per stager, the strided
"long paths" loop of 16-, 8- and 4-wave workgroups from its first trip to its fourth, the 24 KB limit from both sides, the 512
register-staged doubles of step_fast_pair_kernel from both sides), shared maps of 2 305 .. 4 097 bitmap words whose lethal
cells lie in the late words only (the fourth to sixth slice of the unrolled map staging, kLocalMapWords from both sides), the
largest LDS request the launch can make, a path dense enough for the flat scan list to overflow in every step, the rollout
kernel on the same worlds, and one handle re-bound across the limits.  tests/staging.py builds the worlds; what they have to be
like for any of this to bite is asserted on the CPU in test_staging_host.py (and the cheap part of it again here, on the
oracle's run with the device's normals).

Every case runs 24 steps of 256 + 37 envs (one full workgroup, one ragged one) from the same start states under each kernel:
16-wave workgroups with the shared-geometry variant and without, 8- and 4-wave workgroups, the two-launch form.  One oracle run,
fed the normals the device drew, serves all of them: flags and counters equal, poses / rewards / distances within util.ATOL;
the kernels agree with each other bit for bit, drawn normals included.

What stays uncovered, and why:
  * private maps and private paths are not staged at all; test_gpu_parity and test_gpu_rollout have them.
  * the 2 305-word map has no row wholly beyond word 2 304 (461 x 150: five words per row), so its only lethal cells there are
    the bottom wall's last 21; the 4 095- and 4 096-word maps are the ones that fill slices four to six with speckles.
  * with BCP_LOCAL_PAIRS = 1 | 2 in the environment the "16-wave" runs are 4- or 8-wave runs (as everywhere in the suite), and
    the rollout falls back to its own 16-wave kernel either way.
  * LDS that a stager failed to write still holds what an earlier workgroup left there: a dropped slice shows only where the
    earlier launch staged another map, which the order of the cases (a different map each) arranges but cannot force.
  * the pure-pursuit reward never takes the flat scan list (non-PLAIN kernels scan per lane); test_gpu_delays has it."""
import os

import numpy as np
import pytest

import staging as S
from test_gpu_rollout import _roll_and_compare
from util import ATOL, z_in

pytestmark = pytest.mark.gpu

N = S.N
# (the suite also runs with smaller workgroups for every handle, BCP_LOCAL_PAIRS = 1 | 2: those have the generic variant only)
LARGE_WORKGROUPS = os.environ.get("BCP_LOCAL_PAIRS", "4") not in ("1", "2")
LOCAL, PAIR = "step_local_kernel", "step_fast_pair_kernel + step_pending_kernel"
# (label, tuning, the step form, may run the shared-geometry variant); in this order on one handle: the first two leave the
# workgroup size as the handle was created with
KERNELS = [("shared", dict(local_shared=1), LOCAL, True), ("generic", dict(local_shared=0), LOCAL, False),
           ("pairs2", dict(local_shared=1, local_pairs=2), LOCAL, False), ("pairs1", dict(local_pairs=1), LOCAL, False),
           ("two-launch", dict(fused=0), PAIR, False)]


def _put(torch, env, start):
    st, md, tgt, it = start
    env.state.robot.copy_(torch.from_numpy(st.copy()))
    env.state.min_spat_dist_so_far.copy_(torch.from_numpy(md.copy()))
    env.state.target_idx.copy_(torch.from_numpy(tgt.copy()))
    env.state.current_iter.copy_(torch.from_numpy(it.copy()))
    env.state.robot_collided.zero_()
    if env.state.pose_seen is not None:             # (delay queues: every env is at iteration 0, the queues are not read yet)
        env.state.pose_seen.copy_(env.state.robot[0:3])
    if env.state.robot_state_seen is not None:
        env.state.robot_state_seen.copy_(env.state.robot)


def _run(torch, env, c, tuning, form, expect_shared):
    """the case's steps from its start states under `tuning` -> per step, every state array and output as numpy"""
    env.set_tuning(**tuning)
    env.reset()
    _put(torch, env, c.start)
    env.seed(123)
    zout = torch.full((N, 3), float("nan"), dtype=torch.float64, device="cuda") if c.noisy else None
    rows = []
    for a in [torch.from_numpy(a.copy()).cuda() for a in c.actions]:
        env.step(a, noise_z_out=zout)
        assert env.step_kernels().startswith(form), (c.name, tuning, env.step_kernels())
        assert env.step_shared_variant() == expect_shared, (c.name, tuning)
        rows.append(dict(robot=env.state.robot.cpu().numpy(), min_dist=env.state.min_spat_dist_so_far.cpu().numpy(),
                         target_idx=env.state.target_idx.cpu().numpy(), current_iter=env.state.current_iter.cpu().numpy(),
                         robot_collided=env.state.robot_collided.cpu().numpy(), reward=env.reward.cpu().numpy(),
                         done=env.done.cpu().numpy(), collided_now=env.collided_now.cpu().numpy(), err=env.err.cpu().numpy(),
                         z=zout.cpu().numpy() if c.noisy else np.zeros((N, 3))))
    env.check_errors()
    return rows


def _same_bits(a, b, what):
    for t, (x, y) in enumerate(zip(a, b)):
        for key in x:
            np.testing.assert_array_equal(x[key].view(np.uint8), y[key].view(np.uint8), err_msg="%s, step %d: %s" % (what, t, key))


def _against_oracle(oracle, c, got):
    """test_shared_variant_equals_generic_and_oracle's comparison, step by step -> the oracle's rows"""
    want = S.run_oracle(oracle, c, [z_in(g["z"]) for g in got])
    for t, (g, w) in enumerate(zip(got, want)):
        msg = "%s step %d" % (c.name, t)
        for key in ("done", "collided_now", "target_idx", "current_iter", "robot_collided"):
            np.testing.assert_array_equal(g[key], w[key], err_msg=msg + ": " + key)
        for key in ("robot", "reward", "min_dist"):
            np.testing.assert_allclose(g[key], w[key], rtol=0, atol=ATOL, err_msg=msg + ": " + key)
        assert not g["err"].any(), msg
    return want


def _expect_shared(c, may):
    return bool(may and LARGE_WORKGROUPS and c.staged_path and c.staged_map)


@pytest.mark.parametrize("name", S.STEP_CASES)
def test_every_kernel_at_the_staging_limits(torch_cuda, oracle, name):
    torch = torch_cuda
    c = S.case(oracle, name)
    env = c.make_env()
    assert env.step_kernels() == LOCAL
    runs = {}
    for label, tuning, form, may in KERNELS:
        runs[label] = _run(torch, env, c, tuning, form, _expect_shared(c, may))
        if label == "shared":
            assert env.parked_poses() > 0                   # (some poses went through the exact test: the bitmap was read)
    want = _against_oracle(oracle, c, runs["shared"])
    for label in runs:
        if label != "shared":
            _same_bits(runs["shared"], runs[label], "%s: shared against %s" % (name, label))
    # what the host tests assert of the inputs holds for this run, too (the device's normals are not the host's)
    at_tail, goals, resets = S.path_conditions(c, want)
    hits = sum(int(w["collided_now"].sum()) for w in want)
    print(name, "words", c.words, "way points", c.n_way, "| at the last way point", at_tail, "goal ends", goals, "reset", resets,
          "collisions", hits)
    assert at_tail >= 10 and goals >= 5 and resets >= 10 and hits > 0
    if name == "dense":
        counts = S.scan_candidates(oracle, c, want)
        assert (counts.max(axis=1) > S.SCAN_ITEMS).all() and counts.max() > 3 * S.SCAN_ITEMS, counts
    env.close()


@pytest.mark.parametrize("name", ["max-delays", "max-diffdrive", "max-wide", "dense"])
def test_rollout_stages_once_per_launch(torch_cuda, oracle, name):
    """bcp_rollout, 7 steps per launch (staged on the first trip only), against 7 bcp_step calls on a twin, bit for bit"""
    torch = torch_cuda
    c = S.case(oracle, name)

    def make():
        env = c.make_env(seed=77)
        _put(torch, env, c.start)
        return env
    hits, dones = _roll_and_compare(torch, make, 7, rounds=3, scale=c.v_scale)
    print(name, "collisions", hits, "episode ends", dones)
    assert hits > 0 and dones > 0


def _rebind(env, c):
    from bc_gym_planning_env_amd import CostMap2D
    env._set_costmaps(CostMap2D(c.cm.copy(), c.res, c.origin.copy()))
    env._set_paths(c.path.copy())
    env._initial_state = env._make_initial_state()
    env._bind(env._initial_state, env._lib.bcp_bind_initial_state)


def test_one_handle_across_the_limits(torch_cuda, oracle):
    """4 096 words / 614 way points -> 4 097 / 615 -> 4 095 / 153 -> the first again, 12 steps after each binding against a fresh
    oracle: the variant follows the limits (shared, generic, shared, shared) and the last binding repeats the first bit for bit"""
    torch = torch_cuda
    cases = [S.case(oracle, n) for n in S.BIND_CASES]
    assert [(c.words, c.n_way) for c in cases] == [(4096, 614), (4097, 615), (4095, 153), (4096, 614)]
    env = cases[0].make_env()
    runs = []
    for k, c in enumerate(cases):
        if k:
            _rebind(env, c)
        expect = _expect_shared(c, True)
        assert expect == ((True, False, True, True)[k] and LARGE_WORKGROUPS)
        runs.append(_run(torch, env, c, {}, LOCAL, expect))
        _against_oracle(oracle, c, runs[-1])
    _same_bits(runs[0], runs[3], "the fourth binding against the first")
    assert env.parked_poses() > 0
    env.close()
