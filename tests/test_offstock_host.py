"""What the GPU tests away from the stock parameters (tests/test_gpu_offstock.py) stand on, checked without a GPU:
  * their batches, stepped on the CPU oracle alone, really contain dones, collisions, way points reached, time-outs and
    drawn noise slots;
  * div_by_const (csrc/bcp_device.h), restated with an exactly rounded fma, is the IEEE quotient for every dt and wheel
    base the tests use;
  * robots.make_bcp_params(robot_constants=...) puts each constant into its own field."""
import ctypes as C
import math
from fractions import Fraction

import numpy as np
import pytest

import offstock as OS

GRID = [("mini", r) for r in range(1, 15)] + [("dd64", 1), ("dd64", 7)] + [("aisle", r) for r in (7, 8, 9, 11)]


@pytest.mark.parametrize("world,row", GRID, ids=["%s-row%d" % wr for wr in GRID])
def test_grid_rows_are_not_vacuous_on_the_oracle_alone(oracle, world, row):
    """>= 20 dones, >= 20 collisions, >= 10 env-steps onto a new way point; row 10: >= 500 time-outs; row 6: every noise slot
    drawn in >= 100 env-steps; rows 13 and 14: slot 0 in >= 100 env-steps, the others never (tests/offstock.Batch.assert_floors, which the GPU tests call on their own runs too)."""
    b = OS.Batch(oracle, world, row)
    assert b.n == 600 and b.n % 256 == 88
    for _ in range(OS.STEPS):
        b.step_oracle(b.next_actions(), count_drawn=(row in (6, 13, 14)))
    print(world, row, b.counts)
    assert (b.ref.err == 0).all()
    b.assert_floors()


def test_grid_moves_what_it_claims():
    short, long_ = OS.robot_constants("short"), OS.robot_constants("long")
    assert short["front_wheel_from_axis"] == 0.5 and long_["front_wheel_from_axis"] == 1.7
    assert set(short) == set(long_) and len(short) == 6 and all(short[k] != long_[k] for k in short)
    six = OS.alpha_set("all_six")
    assert all(a > 0 for a in six) and OS.PLANENV_ALPHA[0] == OS.PLANENV_ALPHA[1] == 0.0
    c11, c12 = OS.Config(11, (0.2, 0.4, 0.0)), OS.Config(12, (0.2, 0.4, 0.0))
    assert (c11.dt, c11.constants, c11.alpha, (c11.sp, c11.ap, c11.mult)) == (0.1, short, six, OS.REACH_MID)
    assert (c12.dt, c12.constants, c12.dynamic_model, c12.model_front_column_pid) == (0.02, long_, False, False)
    assert c12.ap >= math.pi > c11.ap


# ---- div_by_const in exact arithmetic ---------------------------------------------------------------------------
def _fma(a, b, c):
    """a * b + c rounded once: Fraction arithmetic is exact and float(Fraction) rounds correctly"""
    return float(Fraction(a) * Fraction(b) + Fraction(c))


def div_by_const(x, d, rd):
    """csrc/bcp_device.h: q = x * rd; fma(fma(-q, d, x), rd, q)"""
    q = x * rd
    return _fma(_fma(-q, d, x), rd, q)


def _divisors():
    g = OS._golden("g16_robot_step_params.npz")
    wheel_bases = sorted(set(g["constants"][:, list(g["constant_keys"]).index("front_wheel_from_axis")].tolist()))
    dts = sorted(set(g["dt"].tolist()) | set(spec["dt"] for spec in OS.ROWS.values() if "dt" in spec) | {0.05})
    assert {0.02, 1. / 30., 0.1, 0.25} <= set(dts) and {0.5, 0.964, 1.7} <= set(wheel_bases)
    return dts + wheel_bases + [math.pi, 1. / 60., 0.9, 1.1]


@pytest.mark.parametrize("d", _divisors(), ids=lambda d: "%.6g" % d)
def test_div_by_const_is_the_ieee_quotient(d):
    """2 000 dividends per divisor: random in +-4, random in +-1e-3, whole multiples of the divisor, values around 1e-8"""
    rng = np.random.RandomState(int(d * 1e6) % 2 ** 31)
    xs = np.concatenate([rng.uniform(-4, 4, 800), rng.uniform(-1e-3, 1e-3, 500), np.arange(1, 401) * d * rng.choice([-1.0, 1.0], 400),
                         rng.uniform(-1e-8, 1e-8, 300)])
    assert len(xs) == 2000
    rd = 1.0 / d
    differ = [x for x in xs.tolist() if div_by_const(x, d, rd) != x / d]
    assert len(differ) == 0, (d, len(differ), differ[:3])


def test_div_by_const_loses_the_sign_of_a_negative_zero():
    """The one known exception (documented at div_by_const): -0.0 / d is -0.0, the sequence returns +0.0 -- its residual
    fma(-q, d, x) = (+0.0) + (-0.0) is +0.0 and the correction adds it to q = -0.0.  Equal under ==, invisible to the reference's
    outputs; not changed here."""
    for d in (0.05, 0.1, 0.964, 1.7, math.pi):
        got = div_by_const(-0.0, d, 1.0 / d)
        assert got == 0.0 == -0.0 / d
        assert math.copysign(1.0, got) == 1.0 and math.copysign(1.0, -0.0 / d) == -1.0
        assert math.copysign(1.0, div_by_const(0.0, d, 1.0 / d)) == 1.0


# ---- robot_constants= ---------------------------------------------------------------------------------------------
def _bytes(p):
    return C.string_at(C.addressof(p), C.sizeof(p))


def test_robot_constants_reach_their_fields():
    from bc_gym_planning_env_amd import EnvParams, robots
    stock = robots.make_bcp_params(EnvParams(), 'industrial_tricycle_v1', None)
    assert _bytes(robots.make_bcp_params(EnvParams(), 'industrial_tricycle_v1', None, robot_constants=None)) == _bytes(stock)
    assert _bytes(robots.make_bcp_params(EnvParams(), 'industrial_tricycle_v1', None, robot_constants={})) == _bytes(stock)
    keys = sorted(robots.ROBOT_CONSTANTS)
    assert keys == sorted(OS.robot_constants("short"))
    for k in keys:
        assert getattr(stock, k) == robots.ROBOT_CONSTANTS[k]
    for j, key in enumerate(keys):       # one key at a time: that field alone changes
        p = robots.make_bcp_params(EnvParams(), 'industrial_tricycle_v1', None, robot_constants={key: 10.0 + j})
        for k in keys:
            assert getattr(p, k) == (10.0 + j if k == key else robots.ROBOT_CONSTANTS[k]), (key, k)
        setattr(p, key, robots.ROBOT_CONSTANTS[key])
        assert _bytes(p) == _bytes(stock)
    for robot in ("short", "long"):      # all six at once, with distinct values
        want = OS.robot_constants(robot)
        p = robots.make_bcp_params(EnvParams(), 'industrial_tricycle_v1', None, robot_constants=want)
        assert {k: getattr(p, k) for k in keys} == want
    with pytest.raises(KeyError):
        robots.make_bcp_params(EnvParams(), 'industrial_tricycle_v1', None, robot_constants=dict(wheel_base=1.0))
    with pytest.raises(KeyError):
        robots.make_bcp_params(EnvParams(), 'industrial_tricycle_v1', None,
                               robot_constants=dict(front_wheel_from_axis=1.0, dt=0.1))


def test_time_table_is_dt_accumulated_step_by_step(golden_dir):
    """Observation.time of the reference is current_time + dt once per step (envs/base/env.py:382), not iter * dt: the host's
    table must hold the recorded times of every g16 trajectory exactly, past the time-out as well"""
    import glob
    import os
    from bc_gym_planning_env_amd import host_init
    paths = sorted(glob.glob(os.path.join(golden_dir, "g16_traj_*.npz")))
    assert len(paths) == 6
    for path in paths:
        g = np.load(path)
        t = g["time"]
        table = host_init.time_table(float(g["dt"]), len(t) + 1)
        assert table[0] == 0.0
        np.testing.assert_array_equal(table[1:len(t) + 1], t, err_msg=os.path.basename(path))
