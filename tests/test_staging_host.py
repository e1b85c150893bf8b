"""What makes test_gpu_step_staging.py mean something, asserted on its inputs with the oracle alone (no GPU): the worlds of
tests/staging.py really put lethal cells under colliding footprints in the late words of the bitmap, really walk envs over
the last way points, into the goal and through resets, and the dense path really overfills the flat scan list of every
step; and the limits those worlds were built around are still the ones the headers state."""
import os
import re

import numpy as np
import pytest

import footprints as F
import staging as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIMIT_WORLD_CASES = [n for n in S.STEP_CASES + S.BIND_CASES if n.startswith(("map-", "max-", "bind-"))]


def _header(name):
    with open(os.path.join(ROOT, "bc_gym_planning_env_amd", "csrc", name)) as f:
        return f.read()


@pytest.mark.parametrize("name,pattern,value", [
    ("bcp_step.h", r"constexpr int kLocalMapWords\s*=\s*(\d+)\s*;", S.LOCAL_MAP_WORDS),
    ("bcp_step.h", r"constexpr int kScanItems\s*=\s*(\d+)\s*;", S.SCAN_ITEMS),
    ("bcp_step.h", r"kStagers = \(kLocalWaves - kLocalPairs\) \* kBlock;\s*// (\d+) / 384 / 192 threads", S.STAGERS),
    # step_fast_pair_kernel: four doubles per thread of 2 * kBlock = 128 from registers, the loop takes over at 512
    ("bcp_step.h", r"for \(int u = 0; u < (\d+); \+\+u\) \{\s*const int k = u \* 2 \* kBlock \+ tid;\s*t\[u\] =", 4),
    ("bcp_step.h", r"for \(int k = (\d+) \+ tid; k < a\.hot\.lds_path_doubles; k \+= 2 \* kBlock\)", S.PAIR_STAGE_DOUBLES),
    ("bcp_step.h", r"constexpr int kBlock\s*=\s*(\d+)\s*;", 64),
], ids=["map-words", "scan-items", "stagers", "pair-registers", "pair-loop", "block"])
def test_headers_still_state_the_limits(name, pattern, value):
    """the edges below are derived from these numbers: if one of them moves, a test fails instead of the edges moving away"""
    found = re.findall(pattern, _header(name))
    assert found and all(int(v) == value for v in found), (name, pattern, found, value)


def test_headers_still_stage_24_kb_of_path():
    body = re.search(r"static int upload_step_static\(.*?\n\}", _header("bcp_step_host.h"), re.S).group(0)
    found = re.findall(r"h->path\.max_len \* 5 \* sizeof\(double\) <= (\d+) \* (\d+)\)", body)
    assert found == [("24", "1024")], found
    assert S.MAX_STAGED_WAY_POINTS * S.WAY_POINT_BYTES <= S.PATH_LDS_BYTES < (S.MAX_STAGED_WAY_POINTS + 1) * S.WAY_POINT_BYTES
    # the launch asks the same question of the bitmap as the kernel and as local_step_shared
    assert len(re.findall(r"bitmap_words <= kLocalMapWords", _header("bcp_step_host.h"))) == 2


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
