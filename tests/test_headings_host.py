"""What the GPU tests with headings outside [-pi, pi) (tests/test_gpu_headings.py) stand on, checked without a GPU: their
batches (tests/headings.py), stepped on the CPU oracle alone, really start thousands of env-steps from un-normalised
headings, really contain flagged env-steps on and off the knife edge, and whole-turn shifts of the path angles change no
flag of the oracle."""
import numpy as np
import pytest

import headings as HD
import lookahead_ref as LR
import mppi_ref as MR
import offstock as OS

IDS = ["%s-row%d" % wr for wr in HD.WORLDS]


def _run(oracle, world, row, kind, shifted=True):
    b = HD.Batch(oracle, world, row, kind, shifted=shifted)
    assert b.n == 600 and b.n % 256 == 88
    flags, errs = [], []
    for _ in range(OS.STEPS):
        b.injection()
        b.step_oracle(b.next_actions())
        flags.append((b.ref.done.copy(), b.ref.collided_now.copy(), b.ref.target_idx.copy()))
        errs.append(b.ref.err.copy())
    return b, flags, np.stack(errs)


def test_shift_path_moves_what_it_claims():
    path = np.zeros((20, 3))
    path[:, 2] = np.linspace(-3, 3, 20)
    got = HD.shift_path(path)
    assert got[0, 2] == path[0, 2] and (got[:, :2] == path[:, :2]).all()
    turns = (got[:, 2] - path[:, 2]) / HD.TWO_PI
    np.testing.assert_allclose(turns[1:], HD.TURNS[np.arange(1, 20) % 8], rtol=0, atol=1e-9)
    assert np.abs(got[:, 2]).max() > 6000 and (np.abs(got[1:, 2]) >= 4 * np.pi).sum() >= 6
    both = HD.shift_path(np.stack([path, path]))
    assert (both[0] == got).all() and (both[1] == got).all()


@pytest.mark.parametrize("world,row", HD.WORLDS, ids=IDS)
def test_wrapped_batches_on_the_oracle_alone(oracle, world, row):
    """offstock's floors; >= 2 000 env-steps start outside [-pi, pi]; no error word; done, collided_now and target_idx are those
    of the same batch on the unshifted path, for every env and step"""
    b, flags, errs = _run(oracle, world, row, "wrapped")
    print(world, row, b.counts)
    assert (errs == 0).all()
    b.assert_floors()
    plain, plain_flags, plain_errs = _run(oracle, world, row, "wrapped", shifted=False)
    assert (plain_errs == 0).all() and np.abs(plain.paths[..., 2]).max() < 4 * np.pi <= np.abs(b.paths[..., 2]).max()
    for t, (got, want) in enumerate(zip(flags, plain_flags)):
        for name, g, w in zip(("done", "collided_now", "target_idx"), got, want):
            np.testing.assert_array_equal(g, w, err_msg="%s, step %d: shifted against unshifted path angles" % (name, t))


@pytest.mark.parametrize("world,row", HD.WORLDS, ids=IDS)
def test_jumping_batches_on_the_oracle_alone(oracle, world, row):
    """offstock's floors; >= 300 flagged env-steps; on the knife edge >= 50 flagged and >= 50 unflagged; a flag appears only on
    a step that started from an un-normalised heading, and every heading two turns or more out is flagged unless the robot
    still spins from an earlier flagged step (its measured w was a whole turn per dt, and with |w| dt > 0.2 rad the new heading
    may wrap once more and land within pi of the old one)"""
    b = HD.Batch(oracle, world, row, "jumping")
    for _ in range(OS.STEPS):
        b.injection()
        before, calm = b.ref.st[2].copy(), np.abs(b.ref.st[4]) * b.cfg.dt < 0.1
        b.step_oracle(b.next_actions())
        flagged = b.ref.err != 0
        assert (np.abs(before[flagged]) > np.pi).all()
        assert flagged[calm & (np.abs(before) >= 3 * np.pi + 0.2)].all() and set(np.unique(b.ref.err)) <= {0, oracle.ERR_ANGLE_JUMP}
        assert np.abs(before).max() <= 51 * HD.TWO_PI
    print(world, row, b.counts)
    b.assert_floors()


@pytest.mark.parametrize("world,row", HD.PLAN_WORLDS, ids=["%s-row%d" % wr for wr in HD.PLAN_WORLDS])
def test_planner_scenarios_tell_candidates_apart(oracle, world, row):
    """a third of the envs on the knife edge, a third at +-1 turn, the rest two turns or more out; with a shared and with a
    per-env library at least half of the knife-edge envs hold flagged and unflagged candidates; legal envs hold no flag, far
    ones only flags; the MPPI reference flags an env exactly when one of its candidates of one of its iterations is, and with
    the plan of headings.plan_mean some envs are flagged by a single candidate and some by odd-numbered candidates only"""
    b, start, world_d, p, cat = HD.planning_start(oracle, world, row)
    assert [(cat == c).sum() for c in (HD.KNIFE, HD.LEGAL, HD.FAR)] == [32, 32, 32]
    rng = np.random.RandomState(17)
    for shape in ((16,), (b.n, 16)):
        exp = LR.oracle_lookahead(oracle, p, world_d, start, HD.box_library(rng, shape), threads=8)
        err = exp["err"]
        share = HD.mixed_share(err, cat)
        print(world, shape, "knife-edge envs with mixed candidates: %.2f" % share, "flagged candidates", int((err != 0).sum()))
        assert share >= 0.5
        assert (err[cat == HD.LEGAL] == 0).all() and (err[cat == HD.FAR] != 0).all()
    box = OS.action_box()
    low, high = box.low.astype(np.float64), box.high.astype(np.float64)
    for k in (8, 64):
        eps = MR.host_eps(MR.EPS_SEED, HD.MPPI["iterations"], b.n, k, HD.PLAN_H)
        ref = MR.mppi_ref(oracle, p, world_d, start, HD.plan_mean(start), HD.MPPI["sigma"], low, high, HD.MPPI["lam"],
                          HD.MPPI["penalty"], eps)
        np.testing.assert_array_equal(ref["err"] != 0, (ref["iter_err"] != 0).any(axis=(0, 2)))
        flagged, single, odd_only = HD.rare_flags(ref["iter_err"], cat)
        print(world, "mppi K = %d: %d of 32 knife-edge envs flagged, %d by a single candidate, %d by odd-numbered ones only"
              % (k, flagged, single, odd_only))
        assert (ref["err"][cat == HD.LEGAL] == 0).all() and (ref["err"][cat == HD.FAR] != 0).all()
        assert flagged >= 5 and single >= 1 and odd_only >= 2
        if k == 8:
            assert 32 - flagged >= 5
