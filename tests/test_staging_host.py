"""What makes test_gpu_step_staging.py mean something, asserted on its inputs with the oracle alone (no GPU): the worlds of
tests/staging.py really put lethal cells under colliding footprints in the late words of the bitmap, really walk envs over
the last way points, into the goal and through resets, and the dense path really overfills the flat scan list of every
step; and the limits those worlds were built around are still the ones the headers state -- read from a program that includes
csrc/bcp_step_layout.h, not from the headers' text -- with the LDS layouts that header plans for the step kernels."""
import itertools
import os

import numpy as np
import pytest

import host_program
import footprints as F
import staging as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIMIT_WORLD_CASES = [n for n in S.STEP_CASES + S.BIND_CASES if n.startswith(("map-", "max-", "bind-"))]


# every plan the tests below look at, asked of ONE start of the program
LOCAL_TUPLES = list(itertools.product((3, 4, 17), (0, 5, 3070), (0, 1, 4095, 4096), (0, 1), (1, 2, 4)))   # n_verts, path doubles, map words, plain, pairs
PAIR_TUPLES = list(itertools.product((3, 4, 17), (0, 5, 3070)))
COLLISION_TUPLES = list(itertools.product((3, 4, 17), (0, 1, 4095, 4096)))


@pytest.fixture(scope="module")
def layout(tmp_path_factory):
    """tests/c_abi/step_layout_main.cpp, which includes csrc/bcp_step_layout.h alone, built with a host compiler under
    AddressSanitizer and UBSan and run once -> (limits {name: value}, plans {argument: {region: bytes}})"""
    exe = host_program.build(tmp_path_factory, "step_layout_main.cpp")
    args = (["local:%d,%d,%d,%d,%d" % t for t in LOCAL_TUPLES] + ["pair:%d,%d" % t for t in PAIR_TUPLES] +
            ["pending:0", "pending:1"] + ["collision:%d,%d" % t for t in COLLISION_TUPLES])
    lines = host_program.run(exe, args)
    assert lines[-2] == "step layout ok"
    limits = {ln.split(" ")[1]: int(ln.split(" ")[2]) for ln in lines if ln.startswith("limit ")}
    plans = {ln.split(" ")[0]: {kv.split("=")[0]: int(kv.split("=")[1]) for kv in ln.split(" ")[1:]}
             for ln in lines if ":" in ln.split(" ")[0]}
    assert sorted(plans) == sorted(args)
    return limits, plans


@pytest.mark.parametrize("name,value", [
    ("kLocalMapWords", S.LOCAL_MAP_WORDS),
    ("kScanItems", S.SCAN_ITEMS),
    ("local_stagers(4)", S.STAGERS),
    # step_fast_pair_kernel: four doubles per thread of 2 * kBlock = 128 from registers, the loop takes over at 512
    ("kPairStageRegs", 4),
    ("kPairStageDoubles", S.PAIR_STAGE_DOUBLES),
    ("kBlock", 64),
], ids=["map-words", "scan-items", "stagers", "pair-registers", "pair-loop", "block"])
def test_headers_still_state_the_limits(layout, name, value):
    """the edges below are derived from these numbers: if one of them moves, a test fails instead of the edges moving away"""
    limits = layout[0]
    assert limits[name] == value, (name, limits[name], value)
    assert (limits["local_stagers(4)"], limits["local_stagers(2)"], limits["local_stagers(1)"]) == (768, 384, 192)
    assert limits["kPairStageDoubles"] == limits["kPairStageRegs"] * 2 * limits["kBlock"]


def test_headers_still_stage_24_kb_of_path(layout):
    limits = layout[0]
    assert limits["kPathLdsBytes"] == 24 * 1024 == S.PATH_LDS_BYTES
    assert limits["kWayPointDoubles"] * 8 == S.WAY_POINT_BYTES
    assert S.MAX_STAGED_WAY_POINTS * S.WAY_POINT_BYTES <= S.PATH_LDS_BYTES < (S.MAX_STAGED_WAY_POINTS + 1) * S.WAY_POINT_BYTES
    # launch, kernel and local_step_shared ask one function whether the bitmap is staged: up to kLocalMapWords, shared maps only
    assert limits["staged_map_words(1,256,16)"] == 4096 == S.LOCAL_MAP_WORDS
    assert limits["staged_map_words(1,241,17)"] == 0 and limits["staged_map_words(0,8,8)"] == 0


def _regions_hold(plan, order, sizes):
    """the regions follow one another in `order` (the last name is the end of the allocation); each is at least sizes[region]
    bytes long, so a region that holds anything begins strictly before the next one"""
    for name, nxt in zip(order, order[1:]):
        assert plan[nxt] - plan[name] >= sizes[name], (name, nxt, plan, sizes[name])
        assert plan[nxt] > plan[name] or sizes[name] == 0, (name, nxt, plan)


@pytest.mark.parametrize("pairs", [1, 2, 4])
@pytest.mark.parametrize("plain", [0, 1])
def test_the_plan_of_the_single_launch_step(layout, plain, pairs):
    """local_lds_plan, which sizes step_local_kernel's allocation and carves it up: regions in the kernel's order, each as
    large as what the kernel stores there, the 16-byte pieces aligned, and as many bytes as the sum the launcher used to add up"""
    limits, plans = layout
    block, parked, sparse = limits["kBlock"], limits["parked_pose_bytes"], limits["sparse_lds_words"]
    chunks, finish = limits["static_chunks"], limits["finish_slot_bytes"]
    assert finish >= 48 and finish % 16 == 0           # sizeof(FinishWords): five pointers, flags, pad
    order = ("footprint", "path", "hand", "box", "index", "ctl", "rec", "cells", "map", "stat", "finish", "stash", "bytes")
    seen = 0
    for n_verts, path, words, pl, pr in LOCAL_TUPLES:
        if (pl, pr) != (plain, pairs):
            continue
        seen += 1
        p = plans["local:%d,%d,%d,%d,%d" % (n_verts, path, words, pl, pr)]
        sizes = {"footprint": 2 * n_verts * 8, "path": path * 8, "hand": pairs * limits["kHandDoubles"] * block * 8, "box": 8 * 8,
                 "index": 2 * block * 4, "ctl": limits["kCtlWords"] * 4, "rec": pairs * block * parked,
                 "cells": 4 * pairs * sparse * 4, "map": words * 4, "stat": chunks * 16, "finish": finish,
                 "stash": 0 if plain else 10 * pairs * block * 8}
        assert p["footprint"] == 0
        _regions_hold(p, order, sizes)
        assert p["rec"] % 16 == 0 and p["stat"] % 16 == 0 and p["finish"] % 16 == 0 and p["stash"] % 8 == 0
        assert all(p[k] % 8 == 0 for k in ("path", "hand", "box")) and p["index"] % 4 == 0 and p["ctl"] % 4 == 0
        # the sum local_step_lds_bytes added up before the plan existed
        b = (2 * n_verts + path + pairs * 8 * 64 + 8) * 8 + 2 * 64 * 4 + 16 * 4
        b = (b + 15) & ~15
        b += pairs * 64 * parked + 4 * pairs * sparse * 4 + words * 4
        b = (b + 15) & ~15
        b += chunks * 16 + finish + (0 if plain else 10 * pairs * 64 * 8)
        assert p["bytes"] == b, (p, b)
    assert seen == 3 * 3 * 4
    # the flat scan list of a pair (64 results, 64 {lo, first} words, kScanItems bytes) lies in the score part of its hand-off block
    assert (2 * block + limits["kScanItems"] // 4) * 4 <= 3 * block * 8 and limits["kHandDoubles"] == 8


def test_the_plans_of_the_other_step_kernels(layout):
    """the same for step_fast_pair_kernel, step_pending_kernel and step_kernel, against the sums launch_step and
    collision_lds_bytes used to hold"""
    limits, plans = layout
    sparse = limits["sparse_lds_words"]
    for n_verts, path in PAIR_TUPLES:
        p = plans["pair:%d,%d" % (n_verts, path)]
        sizes = {"footprint": 2 * n_verts * 8, "path": path * 8, "hand_pose": 3 * 64 * 8, "hand_score": 3 * 64 * 8, "box": 8 * 8,
                 "index": 2 * 64 * 4}
        assert p["footprint"] == 0
        _regions_hold(p, ("footprint", "path", "hand_pose", "hand_score", "box", "index", "bytes"), sizes)
        assert p["bytes"] == (2 * n_verts + path) * 8 + (6 * 64 + 8) * 8 + 2 * 64 * 4
    assert limits["kPendingWaves"] == 4
    assert plans["pending:0"]["bytes"] == 2 * 4 * 3 * 64 * 4 and plans["pending:1"]["bytes"] == 2 * 4 * 8 * 64 * 4
    for n_verts, words in COLLISION_TUPLES:
        p = plans["collision:%d,%d" % (n_verts, words)]
        sizes = {"map": words * 4, "qverts": 2 * n_verts * 8, "scratch": 2 * n_verts * 64 * 4, "cells": sparse * 4}
        assert p["map"] == 0 and p["qverts"] % 8 == 0
        _regions_hold(p, ("map", "qverts", "scratch", "cells", "bytes"), sizes)
        assert p["bytes"] == (((words + 1) & ~1) + 4 * n_verts + 2 * n_verts * 64 + sparse) * 4


def test_the_edges_are_where_the_cases_stand():
    """what each path length and map size was chosen for"""
    # one double per stager: 768 / 384 / 192 stagers hold 153 / 76 / 38 way points, the loop's first trip starts one later
    for stagers, last in ((768, 153), (384, 76), (192, 38)):
        assert last * 5 <= stagers < (last + 1) * 5 and last in S.PATH_LENGTHS and last + 1 in S.PATH_LENGTHS
    # 16-wave workgroups: 614 way points take the loop's fourth trip (3 070 doubles = 3 * 768 + 766)
    assert 3 * S.STAGERS < 614 * 5 <= 4 * S.STAGERS
    # step_fast_pair_kernel: 102 way points fit its 512 register-staged doubles, 103 do not
    assert 102 * 5 <= S.PAIR_STAGE_DOUBLES < 103 * 5 and 102 in S.PATH_LENGTHS and 103 in S.PATH_LENGTHS
    assert 614 in S.PATH_LENGTHS and 615 in S.PATH_LENGTHS
    for words, shape in S.LIMIT_SHAPES.items():
        assert S.bitmap_words(shape) == words and shape[1] % 32
    assert S.FOURTH_SLICE + 1 in S.LIMIT_SHAPES and {4095, 4096, 4097} <= set(S.LIMIT_SHAPES)


@pytest.mark.parametrize("words", sorted(S.LIMIT_SHAPES))
def test_limit_map_is_what_it_says(oracle, words):
    w = S.limit_map(oracle, words)
    cm, (sr, sc), sw = w["cm"], w["speckles"], w["speckle_words"]
    assert cm.shape == S.LIMIT_SHAPES[words] and S.bitmap_words(cm.shape) == words
    assert (cm[0] == 254).all() and (cm[-1] == 254).all() and (cm[:, 0] == 254).all() and (cm[:, -1] == 254).all()
    assert (cm[sr, sc] == 254).all() and (S.word_of(cm.shape)[sr, sc] == sw).all() and (sw >= S.FOURTH_SLICE).all()
    inner = cm[1:-1, 1:-1] == 254
    if words == S.FOURTH_SLICE + 1:
        assert not inner.any() and (sw == words - 1).all() and (sr == cm.shape[0] - 1).all()
        return
    ir, ic = np.nonzero(inner)
    assert sorted(zip(ir + 1, ic + 1)) == sorted(zip(sr, sc))                     # every inner lethal cell is a listed speckle
    wpr = (cm.shape[1] + 31) // 32
    assert (sr * wpr >= S.FOURTH_SLICE).all()                                     # ... in a row that lies wholly in the late words
    pad = np.pad(inner, 1)
    neighbours = sum(np.roll(np.roll(pad, dy, 0), dx, 1) for dy in (-1, 0, 1) for dx in (-1, 0, 1)) - pad
    assert not (neighbours[pad] > 0).any()                                        # isolated
    assert 3 * (sw >= words - S.STAGERS).sum() >= len(sw)                         # a third in the last 768 words
    assert (sw < S.FOURTH_SLICE + S.STAGERS).sum() >= len(sw) // 4                # ... and the fourth slice has its share
    # about one speckle under every second footprint of the speckled rows
    area = int(np.count_nonzero(oracle.pixel_footprint(0.3, w["verts"], w["res"])))
    band = (cm.shape[0] - 1 - sr.min()) * (cm.shape[1] - 2)
    assert 0.3 < len(sw) * area / band < 0.9, (len(sw), area, band)


@pytest.mark.parametrize("name", S.STEP_CASES + S.BIND_CASES)
def test_paths_are_what_they_say(oracle, name):
    c = S.case(oracle, name)
    want = {"path": lambda: int(name[5:]), "map": lambda: 154, "max": lambda: 154 if name == "max-wide" else 614,
            "dense": lambda: 600, "bind": lambda: (614, 615, 153, 614)[int(name[5:])]}[name.partition("-")[0]]()
    assert c.n_way == len(c.path) == want
    step = np.hypot(np.diff(c.path[:, 0]), np.diff(c.path[:, 1]))
    assert 0 < step.min() and step.max() < S.SP
    assert np.hypot(*(c.path[-1, :2] - c.path[0, :2])) > S.SP
    ti = oracle.initial_reward_state(c.path, S.SP, S.AP)[1]
    assert 1 <= ti <= c.n_way - 1                                                 # the in-kernel reset starts an episode that is not over
    # start states: scattered along the whole path, the last five way points included
    st, md, tgt, it = c.start
    assert tgt.min() >= 1 and tgt.max() == c.n_way - 1 and (tgt >= c.n_way - 5).sum() >= 10
    assert (tgt < c.n_way // 4).any() and ((tgt > c.n_way // 2) & (tgt < c.n_way - 5)).any()


@pytest.mark.parametrize("name", S.STEP_CASES + S.BIND_CASES)
def test_tail_of_the_path(oracle, name):
    """envs arrive at the last way point, episodes end at the goal, and envs are reset onto way point 0"""
    c = S.case(oracle, name)
    rows = S.run_oracle(oracle, c)
    at_tail, goals, resets = S.path_conditions(c, rows)
    hits = sum(int(r["collided_now"].sum()) for r in rows)
    print(name, "envs at the last way point", at_tail, "goal ends", goals, "envs reset", resets, "collisions", hits)
    assert at_tail >= 10 and goals >= 5 and resets >= 10 and hits > 0


@pytest.mark.parametrize("name", LIMIT_WORLD_CASES)
def test_tail_of_the_map(oracle, name):
    """colliding footprints cover lethal cells of the last 768 words of the bitmap, and of words 2 304 .. 3 071"""
    c = S.case(oracle, name)
    in_tail, in_fourth = S.map_conditions(oracle, c, S.run_oracle(oracle, c))
    print(name, "colliding poses over the last 768 words:", in_tail, "over words 2304 .. 3071:", in_fourth)
    assert in_tail >= 10 and in_fourth >= 10


def test_dense_path_overfills_the_scan_list(oracle):
    """in every one of the first 8 steps some block of 64 envs has more than kScanItems candidates, one of them three times as many"""
    c = S.case(oracle, "dense")
    counts = S.scan_candidates(oracle, c, S.run_oracle(oracle, c))
    print("candidates per step and block of 64 envs:\n", counts)
    assert (counts.max(axis=1) > S.SCAN_ITEMS).all() and counts.max() > 3 * S.SCAN_ITEMS
    # ... while the other staged paths keep some blocks on the flat list (their way points are 0.06 m apart and more)
    other = S.case(oracle, "path-614")
    assert (S.scan_candidates(oracle, other, S.run_oracle(oracle, other), steps=2) <= S.SCAN_ITEMS).any()
