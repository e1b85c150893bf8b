"""The HIP path with headings outside [-pi, pi): robot headings and path angles whole turns away from it, headings two turns
or more out (the reference raises "Path has missing/corrupted angle data": BCP_ERR_ANGLE_JUMP) and headings a few
milliradians short of +-3 pi, where the command decides whether it raises.  Against a fixture made with the genuine
reference (tests/golden/g17_headings.npz, which tests/test_oracle_golden.py pins the oracle to first) and against the CPU
oracle on the batches of tests/headings.py: 600 envs (two 256-env workgroups and a tail), shown to be non-vacuous on the
oracle alone by tests/test_headings_host.py; every run asserts the same floors on what it saw itself.
err, flags, target_idx and current_iter are compared exactly, state / reward / min_dist within ATOL; no env-step is left
out, flagged ones included (the oracle defines the pose and the measured w there)."""

import numpy as np
import pytest

import headings as HD
import lookahead_ref as LR
import mppi_ref as MR
import offstock as OS
from test_gpu_offstock import FORMS, _form_id, _make_env, _put_start, replay_recorded
from util import ATOL

pytestmark = pytest.mark.gpu

STEP_FORMS = FORMS + [dict(local_pairs=1)]
MESSAGE = "Path has missing/corrupted angle data at env indices: %s"


def _g17():
    return OS._golden("g17_headings.npz")


# ---------------------------------------------------------------------------------------------- a. single robot steps
@pytest.mark.parametrize("name", ["tri_dyn_pid", "tri_kin_nopid", "dd"])
def test_robot_step_vs_reference_from_unnormalised_headings(torch_cuda, name):
    """bcp_robot_step on every row of g17: the state within ATOL where the reference stepped, the error word exactly where it
    raised"""
    from bc_gym_planning_env_amd import EnvParams, NativeOps, _lib
    g = _g17()
    tri = name != "dd"
    ops = NativeOps('industrial_tricycle_v1' if tri else 'industrial_diffdrive_v1', noise_parameters=None,
                    params=EnvParams(dt=float(g["dt"])), dynamic_model=(name == "tri_dyn_pid"), model_front_column_pid=(name == "tri_dyn_pid"))
    st = g["state"].copy()
    if not tri:
        st[:, 5:] = 0.0
    out, err = ops.robot_step(st, g["cmd"])
    out, err = out.cpu().numpy(), err.cpu().numpy()
    raised = g[name + "_raised"] != 0
    assert raised.sum() >= 150 and (~raised).sum() >= 100
    print("%s: max |out - reference| = %.3g over %d rows, %d raised" % (name, np.abs(out - g[name + "_out"])[~raised].max(), (~raised).sum(), raised.sum()))
    np.testing.assert_array_equal(err != 0, raised)
    assert set(np.unique(err)) == {0, _lib.ERR_ANGLE_JUMP}
    np.testing.assert_allclose(out[~raised], g[name + "_out"][~raised], rtol=0, atol=ATOL)


# ---------------------------------------------------------------------------------------------- b. recorded trajectories
@pytest.mark.parametrize("form", FORMS[:3], ids=_form_id)
@pytest.mark.parametrize("tag", ["mini", "aisle"])
def test_recorded_trajectories_on_shifted_path_angles(torch_cuda, tag, form):
    """PlanEnv.step recorded on paths whose angles are up to 1000 turns out: the assertions of
    test_recorded_trajectories_at_other_parameters"""
    g17 = _g17()
    g = dict((k[len("traj_%s_" % tag):], g17[k]) for k in g17 if k.startswith("traj_%s_" % tag))
    world = OS._golden(str(g["world"]))
    g.update(costmap=world["costmap"], origin=world["origin"], resolution=world["resolution"])
    assert np.abs(g["path"][:, 2]).max() > 6000
    replay_recorded(torch_cuda, g, form)


# ---------------------------------------------------------------------------------------------- c, d. batches against the oracle
def _run_against_oracle(torch, oracle, world, row, kind, form):
    b = HD.Batch(oracle, world, row, kind)
    env = _make_env(b, form)
    ref, n = b.ref, b.n
    _put_start(torch, env, b)
    noisy = b.cfg.alpha is not None
    zout = torch.zeros(n, 3, dtype=torch.float64, device="cuda") if noisy else None
    worst, checked = 0.0, 0
    for t in range(OS.STEPS):
        new = b.injection()
        if new is not None:     # the same doubles on both sides
            env.state.robot[2].copy_(torch.from_numpy(new))
        a = b.next_actions()
        before_state, before_target = np.stack(ref.st), ref.target_idx.copy()
        if noisy:
            env.step(a, noise_z_out=zout)
        else:
            env.step(a)
        z = zout.cpu().numpy() if noisy else None
        b.step_oracle(a, z)
        gpu_state = env.state.robot.cpu().numpy()
        flags = [("err", env.err, ref.err), ("done", env.done, ref.done), ("collided_now", env.collided_now, ref.collided_now),
                 ("target_idx", env.state.target_idx, ref.target_idx), ("current_iter", env.state.current_iter, ref.cur_iter),
                 ("robot_collided", env.state.robot_collided, ref.collided)]
        bad = set()
        for name, got, want in flags:
            bad |= set(np.nonzero(got.cpu().numpy() != want)[0].tolist())
        if bad:    # a finding: the two headings, and where the oracle itself stands relative to the limits the flags sit on
            lines = [", ".join("%s %d / %d" % (name, int(got[i]), int(want[i])) for name, got, want in flags) + " (GPU / oracle), heading "
                     "before %r, after %r / %r: " % (before_state[2, i], gpu_state[2, i], ref.st[2][i]) +
                     OS.describe_flag_difference(b, i, before_state, before_target, a, z, gpu_state) for i in sorted(bad)[:8]]
            pytest.fail("%s row %d %s %s, step %d: %d envs differ in a flag\n%s" % (world, row, kind, form, t, len(bad), "\n".join(lines)))
        np.testing.assert_allclose(gpu_state, np.stack(ref.st), rtol=0, atol=ATOL, err_msg="step %d" % t)
        np.testing.assert_allclose(env.reward.cpu().numpy(), ref.reward, rtol=0, atol=ATOL, err_msg="step %d" % t)
        np.testing.assert_allclose(env.state.min_spat_dist_so_far.cpu().numpy(), ref.min_dist, rtol=0, atol=ATOL, err_msg="step %d" % t)
        worst = max(worst, np.abs(gpu_state - np.stack(ref.st)).max())
        flagged = np.nonzero(ref.err)[0]
        if len(flagged) == 0:
            env.check_errors()
        else:       # the reference raised in exactly these envs on this step
            with pytest.raises(Exception) as raised:
                env.check_errors()
            assert str(raised.value) == MESSAGE % flagged, "step %d" % t
            checked += 1
    print("%s row %d %s %s: max |state - oracle| = %.3g, %s" % (world, row, kind, form, worst, b.counts))
    b.assert_floors()
    assert (kind == "wrapped") == (checked == 0)


CASES = [(world, row, form) for world, row in HD.WORLDS for form in STEP_FORMS]
CASE_IDS = ["%s-row%d-%s" % (w, r, _form_id(f)) for w, r, f in CASES]


@pytest.mark.parametrize("world,row,form", CASES, ids=CASE_IDS)
def test_wrapped_headings_vs_oracle(torch_cuda, oracle, world, row, form):
    """path angles up to 1000 turns out, robot headings re-injected one turn out on every third step: the second branch of
    py_mod_two_pi in the movers and the far one in the way-point scans; no error word, check_errors() silent"""
    _run_against_oracle(torch_cuda, oracle, world, row, "wrapped", form)


@pytest.mark.parametrize("world,row,form", CASES, ids=CASE_IDS)
def test_jumping_headings_vs_oracle(torch_cuda, oracle, world, row, form):
    """robot headings 2, 3 and 50 turns out and on the knife edge below +-3 pi: the error word of every env-step is the
    oracle's, check_errors() raises after every flagged step and names exactly the flagged envs"""
    _run_against_oracle(torch_cuda, oracle, world, row, "jumping", form)


# ---------------------------------------------------------------------------------------------- e. bcp_rollout
@pytest.mark.parametrize("outputs", [True, False], ids=["with-err_out", "without"])
@pytest.mark.parametrize("world,row", HD.WORLDS, ids=["%s-row%d" % wr for wr in HD.WORLDS])
def test_rollout_reports_every_flagged_step(torch_cuda, oracle, world, row, outputs):
    """the 'jumping' batch, K = 8 steps per call with a heading injection before each call, bit for bit against a twin stepped
    launch by launch; with and without err_out / collided_out, check_errors() raises for every env that any of the 8 rows
    flagged (the injected heading is flagged on the first row, not the last), and collided_now is the last row"""
    from test_gpu_rollout import _compare_envs, _same
    torch = torch_cuda
    k_steps = 8
    b = HD.Batch(oracle, world, row, "jumping")
    env, twin = _make_env(b, None, seed=77), _make_env(b, None, seed=77)
    for e in (env, twin):
        _put_start(torch, e, b)
    n = b.n
    flagged_rounds = 0
    for r in range(OS.STEPS // k_steps):
        new, _ = HD.inject(b.inject_rng, env.state.robot[2].cpu().numpy(), "jumping")
        for e in (env, twin):
            e.state.robot[2].copy_(torch.from_numpy(new))
        a = torch.from_numpy(np.stack([b.next_actions() for _ in range(k_steps)])).cuda()
        coll = torch.zeros(k_steps, n, dtype=torch.uint8, device="cuda")
        err = torch.zeros(k_steps, n, dtype=torch.int32, device="cuda")
        if outputs:
            rew, done = env.rollout(a, collided_out=coll, err_out=err)
        else:
            rew, done = env.rollout(a)
        any_err = torch.zeros(n, dtype=torch.int32, device="cuda")
        for k in range(k_steps):
            twin.step(a[k])
            _same(torch, rew[k], twin.reward, "reward, round %d step %d" % (r, k))
            _same(torch, done[k], twin.done, "done, round %d step %d" % (r, k))
            if outputs:
                _same(torch, coll[k], twin.collided_now, "collided_now, round %d step %d" % (r, k))
                _same(torch, err[k], twin.err, "err, round %d step %d" % (r, k))
            any_err |= twin.err
        _compare_envs(torch, env, twin, "round %d" % r)
        _same(torch, env.collided_now, twin.collided_now, "collided_now after round %d is the last row" % r)
        _same(torch, env.err, any_err, "err after round %d is the OR over the %d rows" % (r, k_steps))
        flagged = torch.nonzero(any_err).flatten().cpu().numpy()
        assert len(flagged) >= 100 and int((twin.err != 0).sum()) < len(flagged), (r, len(flagged))
        with pytest.raises(Exception) as raised:
            env.check_errors()
        assert str(raised.value) == MESSAGE % flagged, "round %d" % r
        flagged_rounds += 1
    assert flagged_rounds == 4


# ---------------------------------------------------------------------------------------------- f. bcp_lookahead, bcp_mppi
def _planning_case(torch, oracle, world, row):
    b, start, world_d, p, cat = HD.planning_start(oracle, world, row)
    env = _make_env(b, auto_reset=False)
    from test_gpu_lookahead import _set_start
    _set_start(torch, env, start)
    return b, env, start, world_d, p, cat


PLAN_IDS = ["%s-row%d" % wr for wr in HD.PLAN_WORLDS]


@pytest.mark.parametrize("per_env", [False, True], ids=["shared-library", "per-env-library"])
@pytest.mark.parametrize("world,row", HD.PLAN_WORLDS, ids=PLAN_IDS)
def test_lookahead_flags_candidates_one_by_one(torch_cuda, oracle, world, row, per_env):
    """a third of the envs on the knife edge (the candidate decides), a third one turn out (never flagged), the rest two turns
    or more out (always): err per candidate is the oracle's; ret, steps, reason, final_pose and best as the look-ahead tests
    compare them"""
    from test_gpu_lookahead import _check
    torch = torch_cuda
    b, env, start, world_d, p, cat = _planning_case(torch, oracle, world, row)
    library = HD.box_library(np.random.RandomState(17), (b.n, 16) if per_env else (16,))
    exp = LR.oracle_lookahead(oracle, p, world_d, start, library, threads=16)
    la = env.lookahead(torch.from_numpy(library).cuda(), want=("err", "final_pose", "final_target_idx", "best"))
    _check(la, exp, HD.PLAN_H, tag="%s row %d %s" % (world, row, library.shape))
    err = la.err.cpu().numpy()
    np.testing.assert_array_equal(err, exp["err"])
    share = HD.mixed_share(err, cat)
    print("knife-edge envs with flagged and unflagged candidates: %.2f; %d flagged candidates" % (share, (err != 0).sum()))
    assert share >= 0.5 and (err[cat == HD.LEGAL] == 0).all() and (err[cat == HD.FAR] != 0).all()


@pytest.mark.parametrize("k", [8, 64])
@pytest.mark.parametrize("world,row", HD.PLAN_WORLDS, ids=PLAN_IDS)
def test_mppi_flags_an_env_for_a_single_candidate(torch_cuda, oracle, world, row, k):
    """the same start states, a plan that steers away from the edge: few candidates cross it -- in some envs none, in some one,
    in some only odd-numbered ones.  err per env is the reference's: the OR over iterations and candidates; returns and
    reasons of every iteration as the MPPI tests compare them"""
    import mppi_check as MC
    torch = torch_cuda
    b, env, start, world_d, p, cat = _planning_case(torch, oracle, world, row)
    m = HD.MPPI
    eps = MR.host_eps(MR.EPS_SEED, m["iterations"], b.n, k, HD.PLAN_H)
    res = env.mppi(HD.plan_mean(start), m["sigma"], m["iterations"], k, m["lam"], m["penalty"], eps=eps,
                   want=("eps", "iter_mean", "iter_ret", "iter_reason", "err"))
    assert torch.equal(res.eps, torch.from_numpy(eps).cuda())
    MC.teacher_forced(torch, env, res, m["sigma"], m["lam"], m["penalty"], oracle_args=(oracle, p, world_d, start),
                      tag="%s K=%d" % (world, k))
    # the reference's word, teacher-forced like the rest: each iteration's candidates made from the GPU's own mean of that iteration
    low, high = (np.asarray(v, np.float64) for v in (env.action_space.low, env.action_space.high))
    iter_err = []
    for j in range(m["iterations"]):
        u = MR.candidates(res.iter_mean[j].cpu().numpy(), m["sigma"], eps[j], low, high)
        iter_err.append(LR.oracle_lookahead(oracle, p, world_d, start, MR.as_lookahead_actions(u), threads=16)["err"])
    want = np.bitwise_or.reduce(np.stack(iter_err), axis=(0, 2))
    np.testing.assert_array_equal(res.err.cpu().numpy(), want)
    flagged, single, odd_only = HD.rare_flags(iter_err, cat)
    print("K = %d: %d of 32 knife-edge envs flagged, %d by a single candidate, %d by odd-numbered ones only" % (k, flagged, single, odd_only))
    assert flagged >= 5 and single >= 1 and odd_only >= 2
    assert (want[cat == HD.LEGAL] == 0).all() and (want[cat == HD.FAR] != 0).all()
    # and the free-running reference (its own means from iteration to iteration) names the same envs
    ref = MR.mppi_ref(oracle, p, world_d, start, HD.plan_mean(start), m["sigma"], low, high, m["lam"], m["penalty"], eps)
    np.testing.assert_array_equal(res.err.cpu().numpy(), ref["err"])
