"""Host-side checks of the look-ahead (bcp_lookahead): the C struct and its ctypes mirror, the candidate library of
planning.py, the `best` rule, and -- on the CPU oracle alone -- the expectation the GPU tests compare against: it must
reproduce the recorded reference trajectories, and the scenarios the GPU tests run must really contain collisions,
time-outs, reached goals, envs with mixed outcomes and many distinct winners."""
import os
import subprocess
import sys
import tempfile

import numpy as np

import lookahead_ref as LR
from util import ATOL, GOLDEN, oracle_params_for

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

FIELDS = ["actions", "noise_z", "mask", "horizon", "n_candidates", "ret", "steps", "reason", "final_pose",
          "final_target_idx", "err", "best", "best_action"]


def test_lookahead_struct_matches_header_and_symbol_is_bound():
    """sizeof / offsetof of bcp_lookahead_io as the C compiler lays it out from include/bcplan.h == the ctypes mirror"""
    import ctypes as C
    from bc_gym_planning_env_amd import _lib, build
    assert [f[0] for f in _lib.BcpLookaheadIO._fields_] == FIELDS
    src = ['#include <stddef.h>', '#include <stdio.h>', '#include "bcplan.h"', 'int main(void) {',
           '  printf("%zu", sizeof(bcp_lookahead_io));']
    src += ['  printf(" %%zu", offsetof(bcp_lookahead_io, %s));' % f for f in FIELDS]
    src += ['  printf(" %d %d %d\\n", BCP_LOOKAHEAD_PER_ENV, BCP_STEP_ACTIONS_F32, BCP_ABI_VERSION);', '  return 0; }']
    with tempfile.TemporaryDirectory() as d:
        c_file, exe = os.path.join(d, "probe.c"), os.path.join(d, "probe")
        open(c_file, "w").write("\n".join(src))
        subprocess.check_call([os.environ.get("CC", "gcc"), "-I", os.path.join(ROOT, "include"), c_file, "-o", exe])
        got = [int(v) for v in subprocess.check_output([exe]).split()]
    want = [C.sizeof(_lib.BcpLookaheadIO)] + [getattr(_lib.BcpLookaheadIO, f).offset for f in FIELDS]
    assert got[:-3] == want
    assert got[-3:] == [_lib.LOOKAHEAD_PER_ENV, _lib.STEP_ACTIONS_F32, _lib.ABI_VERSION] == [256, 2, 2]
    assert _lib.LOOKAHEAD_PER_ENV & (_lib.STEP_AUTO_RESET | _lib.STEP_ACTIONS_F32) == 0
    build.build()
    lib = _lib.load()
    assert "bcp_lookahead" in _lib.SYMBOLS and lib.bcp_lookahead.argtypes[1]._type_ is _lib.BcpLookaheadIO


def test_constant_command_library():
    from bc_gym_planning_env_amd import constant_command_library
    from bc_gym_planning_env_amd.api import Box
    space = Box(low=np.array([0.1, -np.pi / 2]), high=np.array([0.5, np.pi / 2]), dtype=np.float32)
    lib = constant_command_library(space, 5, 9, 16)
    assert lib.shape == (16, 45, 2) and lib.dtype == np.float32 and lib.flags["C_CONTIGUOUS"]
    assert (lib == lib[0]).all(), "every candidate holds one command for the whole horizon"
    assert (lib >= space.low.astype(np.float32)).all() and (lib <= space.high.astype(np.float32)).all()
    assert all(space.contains(c) for c in lib[0])
    assert len({tuple(c) for c in lib[0]}) == 45
    assert lib[0, :, 0].min() == np.float32(0.1) and lib[0, :, 0].max() == np.float32(0.5)
    one = constant_command_library(space, 1, 1, 3)
    assert one.shape == (3, 1, 2) and abs(one[0, 0, 0] - 0.3) < 1e-6 and abs(one[0, 0, 1]) < 1e-6


def test_best_rule_on_hand_made_tables():
    C = LR.DONE_COLLIDED
    ret = np.array([[1.0, 5.0, 3.0, 3.0],      # the collided 5.0 loses to any free candidate; 3.0 twice -> lowest k
                    [2.0, 2.0, 2.0, 2.0],      # all equal, all free -> 0
                    [1.0, 7.0, 7.0, 0.0],      # all collided -> largest ret among them, lowest k
                    [-1.0, -5.0, 9.0, 9.5],    # one free candidate with the worst return still wins
                    [0.0, 0.0, 1.0, 1.0]])     # goal / timeout bits do not matter
    reason = np.array([[0, C, 0, 0],
                       [0, 0, 0, 0],
                       [C, C, C | LR.DONE_TIMEOUT, C],
                       [C, 0, C, C | LR.DONE_GOAL],
                       [LR.DONE_GOAL, LR.DONE_TIMEOUT, LR.DONE_TIMEOUT, LR.DONE_GOAL]], dtype=np.uint8)
    np.testing.assert_array_equal(LR.select_best(ret, reason), [2, 0, 1, 1, 2])


def test_expectation_reproduces_recorded_reference_windows(oracle):
    """windows of g8_traj_aisle_default (PlanEnv noise, recorded normals replayed, poison in undrawn slots): the masked
    sum until the first done step equals the sum of the recorded rewards, and the windows from 420 and 440 end with the
    recorded collision at step 444"""
    name = "g8_traj_aisle_default.npz"
    g = np.load(os.path.join(GOLDEN, name))
    starts, horizon = [0, 100, 300, 420, 440], 32
    start, actions, z = LR.recorded_windows(g, starts, horizon)
    got = LR.oracle_lookahead(oracle, oracle_params_for(oracle, name), LR.shared_world(g), start, actions, z)
    want = LR.recorded_expectation(g, starts, horizon)
    print("steps", got["steps"][:, 0], "ret", got["ret"][:, 0], "recorded", want["ret"])
    assert int(np.argmax(g["done"])) == 444 and g["collided"][444]
    np.testing.assert_array_equal(got["steps"][:, 0], [32, 32, 32, 25, 5])
    np.testing.assert_array_equal(got["steps"][:, 0], want["steps"])
    np.testing.assert_array_equal(got["reason"][:, 0], [0, 0, 0, LR.DONE_COLLIDED, LR.DONE_COLLIDED])
    np.testing.assert_array_equal(got["ret"][:, 0], want["ret"])
    np.testing.assert_array_equal(got["final_target_idx"][:, 0], want["final_target_idx"])
    np.testing.assert_allclose(got["final_pose"][:, 0], want["final_pose"], rtol=0, atol=ATOL)


def scenario_outcomes(oracle, n=64, k=64, horizon=48):
    """The three scenarios of the GPU tests on the oracle: {kind: (StartState, library, expectation)}"""
    g = LR.mini_fixture()
    params = oracle.make_params("tricycle", noise=None, spatial_precision=0.2, angular_precision=np.pi / 8)
    library = LR.random_library(np.random.RandomState(11), k, horizon)
    out = {}
    for kind in ("scatter", "timeout", "goal"):
        start = LR.scenario_start(g, n, kind)
        out[kind] = (start, library, LR.oracle_lookahead(oracle, params, LR.shared_world(g), start, library))
    return g, out


def test_scenarios_are_not_vacuous(oracle):
    """>= 100 collided, >= 100 timed-out and >= 50 goal candidates, >= 16 envs with a colliding AND a free candidate,
    >= 8 distinct winners -- on the oracle's result, before any GPU is involved"""
    _, out = scenario_outcomes(oracle)
    scatter, timeout, goal = out["scatter"][2], out["timeout"][2], out["goal"][2]
    hit = (scatter["reason"] & LR.DONE_COLLIDED) != 0
    mixed = int((hit.any(axis=1) & ~hit.all(axis=1)).sum())
    winners = len(set(scatter["best"].tolist()))
    timed = int(((timeout["reason"] & LR.DONE_TIMEOUT) != 0).sum())
    goals = int(((goal["reason"] & LR.DONE_GOAL) != 0).sum())
    print("collided %d of %d, mixed envs %d, distinct winners %d, timed out %d, goal %d"
          % (hit.sum(), hit.size, mixed, winners, timed, goals))
    assert hit.sum() >= 100 and timed >= 100 and goals >= 50
    assert mixed >= 16 and winners >= 8
    assert (scatter["steps"][hit] < 48).any() and (scatter["steps"][~hit] == 48).all()
