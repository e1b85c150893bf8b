"""The host half of bcp_declare_uniform_initial_state (csrc/bcp_init_uniform.h: init_uniform_pack) as a stand-alone program under
AddressSanitizer and UBSan.  tests/c_abi/init_uniform_main.cpp includes that header alone -- it has no HIP in it -- and calls the
very function the entry point calls, on heap blocks of exactly n entries (the two tricycle arrays are null pointers for the
diff-drive model, so reading them faults).  Checked against the rule restated here: entries are compared with entry 0 bit for
bit, the first differing env and, within it, the first differing field (in bcp_state's order) are named, and the snapshot is
entry 0 packed as StepStatic::init_uniform (eight float64, four int32: 80 bytes).  And the C ABI: the two new symbols are
declared, exported and typed, and the version did not move."""
import os
import struct

import numpy as np
import pytest

import host_program

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ("x", "y", "angle", "v", "w", "steering_motor_command", "wheel_angle", "min_spat_dist_so_far", "target_idx",
          "current_iter", "robot_collided")
STEER, WHEEL = 5, 6


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    return host_program.build(tmp_path_factory, "init_uniform_main.cpp")


def uniform(n, seed=0):
    """eleven arrays of n equal entries: eight float64 (all non-zero and distinct), two int32, one uint8"""
    rng = np.random.RandomState(seed)
    f64 = [np.full(n, v) for v in rng.uniform(-3.0, 3.0, 8)]
    return f64 + [np.full(n, 17, dtype=np.int32), np.full(n, 2, dtype=np.int32), np.full(n, 1, dtype=np.uint8)]


def expected(arrays, tri):
    """-> (env, field) of the first difference (-1, -1: none) and the 80 bytes of the snapshot"""
    n = len(arrays[0])
    first = (-1, -1)
    for i in range(1, n):
        for f, a in enumerate(arrays):
            if f in (STEER, WHEEL) and not tri:
                continue
            if a[i:i + 1].tobytes() != a[0:1].tobytes():
                first = (i, f)
                break
        if first[0] >= 0:
            break
    raw = b"".join(arrays[f][0:1].tobytes() if not (f in (STEER, WHEEL) and not tri) else struct.pack("<d", 0.0) for f in range(8))
    assert len(raw) == 64
    raw += struct.pack("<4i", int(arrays[8][0]), int(arrays[9][0]), int(arrays[10][0]), 1)
    return first, raw


def run_cases(exe, tmp_path, cases):
    """cases: [(arrays, tri)] -> runs them in ONE start of the program and compares every line"""
    paths = []
    for k, (arrays, tri) in enumerate(cases):
        n = len(arrays[0])
        p = str(tmp_path / ("case%04d.bin" % k))
        with open(p, "wb") as f:
            f.write(struct.pack("<qii", n, 1 if tri else 0, 0))
            for a, dt in zip(arrays, [np.float64] * 8 + [np.int32, np.int32, np.uint8]):
                assert a.dtype == dt and a.shape == (n,)
                f.write(np.ascontiguousarray(a).tobytes())
        paths.append(p)
    lines = host_program.run(exe, paths)
    assert lines[len(cases)] == "init uniform ok"
    for k, (arrays, tri) in enumerate(cases):
        (env, field), raw = expected(arrays, tri)
        got = lines[k].split(" ")
        assert (int(got[0]), int(got[1])) == (env, field), (k, lines[k], env, field)
        assert got[2] == (FIELDS[field] if env >= 0 else "-")
        assert bytes.fromhex(got[3]) == raw, (k, got[3], raw.hex())
    return lines[:len(cases)]


def changed(arrays, field, env, value=None):
    out = [a.copy() for a in arrays]
    a = out[field]
    if value is not None:
        a[env] = value
    elif a.dtype == np.float64:
        a[env] = np.nextafter(a[env], np.inf)   # one unit in the last place
    else:
        a[env] = a[env] + 1
    return out


def test_uniform_arrays(program, tmp_path):
    cases = [(uniform(n, seed), tri) for n, seed in ((2, 0), (293, 1), (4096, 2)) for tri in (True, False)]
    special = uniform(65, 3)
    special[0][:] = np.nan
    special[1][:] = -0.0
    special[3][:] = np.inf
    special[7][:] = 5e-324
    cases.append((special, True))
    lines = run_cases(program, tmp_path, cases)
    assert all(ln.startswith("-1 -1 - ") for ln in lines)


def test_a_difference_in_each_field_at_the_first_a_middle_and_the_last_env(program, tmp_path):
    n = 293
    base = uniform(n, 4)
    cases = [(changed(base, f, env), True) for f in range(11) for env in (1, 146, n - 1)]
    lines = run_cases(program, tmp_path, cases)
    assert [tuple(int(v) for v in ln.split(" ")[:2]) for ln in lines] == [(env, f) for f in range(11) for env in (1, 146, n - 1)]
    # env 0 itself differs from everybody else: env 1 is then the first that is not entry 0, in that field
    cases = [(changed(base, f, 0), True) for f in range(11)]
    lines = run_cases(program, tmp_path, cases)
    assert [tuple(int(v) for v in ln.split(" ")[:2]) for ln in lines] == [(1, f) for f in range(11)]


def test_the_first_env_and_within_it_the_first_field_are_named(program, tmp_path):
    base = uniform(100, 5)
    two_envs = changed(changed(base, 2, 70), 9, 31)          # a late field in an early env wins over an early field later
    two_fields = changed(changed(base, 10, 50), 4, 50)
    lines = run_cases(program, tmp_path, [(two_envs, True), (two_fields, True)])
    assert lines[0].startswith("31 9 current_iter ") and lines[1].startswith("50 4 w ")


def test_words_not_values_a_nan_payload_and_minus_zero(program, tmp_path):
    n = 40
    nans = uniform(n, 6)
    nans[2][:] = np.nan
    quiet_other = [a.copy() for a in nans]
    quiet_other[2].view(np.uint64)[17] ^= np.uint64(1)       # still a NaN, another payload
    assert np.isnan(quiet_other[2][17])
    zeros = uniform(n, 7)
    zeros[4][:] = 0.0
    minus = changed(zeros, 4, n - 1, -0.0)                   # equal as values
    assert minus[4][n - 1] == zeros[4][0]
    lines = run_cases(program, tmp_path, [(nans, True), (quiet_other, True), (zeros, True), (minus, True)])
    assert lines[0].startswith("-1 ") and lines[1].startswith("17 2 angle ")
    assert lines[2].startswith("-1 ") and lines[3].startswith("%d 4 w " % (n - 1))


def test_one_env(program, tmp_path):
    lines = run_cases(program, tmp_path, [(uniform(1, 8), True), (uniform(1, 9), False)])
    assert all(ln.startswith("-1 -1 - ") for ln in lines)


def test_the_diff_drive_model_leaves_the_tricycle_arrays_out(program, tmp_path):
    n = 64
    base = uniform(n, 10)
    steer, wheel = changed(base, STEER, 9), changed(base, WHEEL, n - 1)
    both = changed(changed(base, STEER, 3), 7, 40)
    lines = run_cases(program, tmp_path, [(steer, False), (wheel, False), (steer, True), (wheel, True), (both, False), (both, True)])
    assert lines[0].startswith("-1 ") and lines[1].startswith("-1 ")
    assert lines[2].startswith("9 5 steering_motor_command ") and lines[3].startswith("%d 6 wheel_angle " % (n - 1))
    assert lines[4].startswith("40 7 min_spat_dist_so_far ") and lines[5].startswith("3 5 ")
    # the snapshot of a diff-drive robot holds 0.0 in both places (run_cases compared the bytes)
    snap = bytes.fromhex(lines[0].split(" ")[3])
    assert struct.unpack("<8d", snap[:64])[STEER:WHEEL + 1] == (0.0, 0.0) and struct.unpack("<4i", snap[64:])[3] == 1


def test_header_library_and_binding_agree_and_the_abi_stays():
    import ctypes as C
    from bc_gym_planning_env_amd import _lib, build
    build.build()
    raw = C.CDLL(_lib.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "bcplan.h")).read()
    for name in ("bcp_declare_uniform_initial_state", "bcp_step_uniform_reset"):
        assert hasattr(raw, name) and name in _lib.SYMBOLS
    assert "int bcp_declare_uniform_initial_state(bcp_handle *h, int on, void *stream);" in header
    assert "int bcp_step_uniform_reset(bcp_handle *h);" in header
    lib = _lib.load()
    assert lib.bcp_declare_uniform_initial_state.argtypes == [C.c_void_p, C.c_int, C.c_void_p]
    assert lib.bcp_declare_uniform_initial_state.restype is C.c_int
    assert lib.bcp_step_uniform_reset.argtypes == [C.c_void_p] and lib.bcp_step_uniform_reset.restype is C.c_int
    assert lib.bcp_declare_uniform_initial_state(None, 1, None) == -1 and lib.bcp_step_uniform_reset(None) == -1   # BCP_E_INVALID
    assert _lib.ABI_VERSION == 2 and raw.bcp_abi_version() == 2
    assert "#define BCP_ABI_VERSION 2" in header.replace("  ", " ")
