"""The plan of a goal field launch (csrc/bcp_goal_plan.h: plan_goal, which every launch of goal_field_kernel asks for its
route, threads, grid, dynamic LDS and scratch) as a stand-alone host program under AddressSanitizer and UBSan, against the
rules restated here.  tests/c_abi/goal_plan_main.cpp includes that header alone -- it has no HIP in it.  Nothing below is
taken from the program's output: the squares at which the LDS route ends are searched for with the restated formula."""
import itertools

import pytest

import host_program

LDS_LIMIT = 150 * 1024
FIXED = (128 + 4) * 4            # half-widths [128], pass flags [3], counter
LDS_GRID, BOUND_GRID, GLOBAL_GRID, SCRATCH_BYTES = 16384, 1024, 512, 256 << 20
TRIPS = (0, 1, 1024, 1025, 16384, 16385)


def lds_bytes(rows, cols, in_lds, cost):
    wpr, cells = (cols + 31) // 32, rows * cols
    plain = FIXED + (2 * rows * wpr * 4 + ((cells * 2 + 3) & ~3) if in_lds else 0)
    return plain + (512 + (((cells + 3) & ~3) if in_lds else 0) if cost else 0)


def expected(rows, cols, trips, bound, cost, forced):
    """-> (in_lds, threads, grid, lds_bytes, scratch_words)"""
    in_lds = lds_bytes(rows, cols, True, cost) <= LDS_LIMIT and not forced
    threads = 1024 if rows * cols >= 128 * 128 else 256
    if in_lds:
        return 1, threads, min(trips, BOUND_GRID if bound else LDS_GRID), lds_bytes(rows, cols, True, cost), 0
    mask_words = 2 * rows * ((cols + 31) // 32)
    grid = min(trips, GLOBAL_GRID, max(1, SCRATCH_BYTES // (mask_words * 4)))
    return 0, threads, grid, lds_bytes(rows, cols, False, cost), grid * mask_words


def last_square(cost):
    """the largest s whose s x s map takes the LDS route"""
    fits = [s for s in range(1, 2049) if lds_bytes(s, s, True, cost) <= LDS_LIMIT]
    assert fits == list(range(1, fits[-1] + 1)) and fits[-1] < 2048        # (one threshold: the bytes grow with s)
    return fits[-1]


SHAPES = [(1, 1), (127, 128), (128, 128), (2048, 2048), (1, 2048), (2048, 1), (183, 183), (256, 141)]
SHAPES += [(s + d, s + d) for cost in (False, True) for s in (last_square(cost),) for d in (0, 1)]
CASES = list(itertools.product(SHAPES, TRIPS, (0, 1), (0, 1), (0, 1)))     # shape, trips, bound, cost, forced


@pytest.fixture(scope="module")
def plans(tmp_path_factory):
    """every case through ONE start of the program -> {case: the five numbers it printed}"""
    exe = host_program.build(tmp_path_factory, "goal_plan_main.cpp", opt=())
    args = ["%d,%d,%d,%d,%d,%d" % (r, c, t, b, k, f) for (r, c), t, b, k, f in CASES]
    lines = host_program.run(exe, args, "goal plan ok")
    assert lines[len(CASES)] == "limits %d %d %d %d %d %d" % (LDS_LIMIT, LDS_GRID, BOUND_GRID, GLOBAL_GRID, SCRATCH_BYTES, FIXED // 4)
    assert lines[len(CASES) + 1] == "goal plan ok"
    return {case: tuple(int(v) for v in ln.split()) for case, ln in zip(CASES, lines)}


def test_every_plan_is_the_rules(plans):
    assert len(plans) == len(CASES) == 12 * 6 * 8
    for ((rows, cols), trips, bound, cost, forced), got in plans.items():
        assert got == expected(rows, cols, trips, bound, cost, forced), (rows, cols, trips, bound, cost, forced, got)


def test_the_cases_reach_every_rule(plans):
    """what the table is for, stated on the expectations and on the program's answers alike"""
    for source in (lambda *case: expected(case[0][0], case[0][1], *case[1:]), lambda *case: plans[case]):
        # the thread switch at 128 x 128 cells
        assert source((127, 128), 1, 0, 0, 0)[1] == 256 and source((128, 128), 1, 0, 0, 0)[1] == 1024
        assert source((1, 1), 1, 0, 0, 0) == (1, 256, 1, FIXED + 2 * 4 + 4, 0)
        # the last square in LDS and the first beyond it, plain and with cost
        for cost in (0, 1):
            s = last_square(bool(cost))
            assert source((s, s), 1, 0, cost, 0)[0] == 1 and source((s + 1, s + 1), 1, 0, cost, 0)[0] == 0
            assert source((s, s), 1, 0, cost, 0)[3] <= LDS_LIMIT and source((s + 1, s + 1), 1, 0, cost, 0)[3] == FIXED + 512 * cost
        assert last_square(True) < last_square(False)
        # the LDS route's grid: 16 384, or 1 024 in the bound form
        assert [source((128, 128), t, 0, 0, 0)[2] for t in TRIPS] == [0, 1, 1024, 1025, 16384, 16384]
        assert [source((128, 128), t, 1, 0, 0)[2] for t in TRIPS] == [0, 1, 1024, 1024, 1024, 1024]
        # the global route: 512 workgroups, fewer where 256 MiB of masks hold fewer -- 2048 x 2048 has 1 MiB per workgroup
        assert [source((2048, 2048), t, b, 0, 0)[2] for t in TRIPS for b in (0, 1)] == [0, 0, 1, 1, 256, 256, 256, 256, 256, 256, 256, 256]
        assert source((2048, 2048), 16385, 0, 0, 0)[4] * 4 == SCRATCH_BYTES
        s = last_square(False) + 1
        assert [source((s, s), t, 1, 0, 0)[2] for t in TRIPS] == [0, 1, 512, 512, 512, 512]
        # the forced global route: a map that fits LDS, in scratch all the same
        forced = source((128, 128), 1025, 0, 0, 1)
        assert forced == (0, 1024, 512, FIXED, 512 * 2 * 128 * 4) and source((128, 128), 1025, 0, 1, 1)[3] == FIXED + 512
