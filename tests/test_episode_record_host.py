"""Host side of the episode record (include/bcplan.h: bcp_episode_record, BCP_DONE_*): constants, the ctypes layout, and
the terminated / truncated split of EpisodeEnds (no GPU needed)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "bcplan.h")


def test_done_reasons_match_header():
    from bc_gym_planning_env_amd import _lib
    text = open(HEADER).read()
    vals = dict((k, int(v)) for k, v in re.findall(r"\b(BCP_DONE_[A-Z]+)\s*=\s*(\d+)", text))
    assert vals == {"BCP_DONE_GOAL": _lib.DONE_GOAL, "BCP_DONE_TIMEOUT": _lib.DONE_TIMEOUT,
                    "BCP_DONE_COLLIDED": _lib.DONE_COLLIDED}


def test_terminated_truncated_truth_table():
    """goal / collision are terminal (with or without a time-out); a time-out alone is a truncation (env.py:400-419)"""
    import torch
    from bc_gym_planning_env_amd.batched_env import EpisodeEnds
    ends = EpisodeEnds.__new__(EpisodeEnds)
    ends.reason = torch.arange(8, dtype=torch.uint8)   # every combination of GOAL(1) TIMEOUT(2) COLLIDED(4)
    term = ends.terminated().numpy()
    trunc = ends.truncated().numpy()
    r = np.arange(8)
    goal, timeout, collided = (r & 1) != 0, (r & 2) != 0, (r & 4) != 0
    np.testing.assert_array_equal(term, goal | collided)
    np.testing.assert_array_equal(trunc, timeout & ~goal & ~collided)
    assert term[1 | 2] and not trunc[1 | 2]   # goal reached on the time-out step: terminated
    assert not (term & trunc).any() and not term[0] and not trunc[0]


def test_record_layout_matches_header(tmp_path):
    """BcpEpisodeRecord has the C layout: offsets and size as a hipcc-compiled probe of the header reports them"""
    from bc_gym_planning_env_amd import _lib, build
    fields = [f[0] for f in _lib.BcpEpisodeRecord._fields_]
    src = tmp_path / "probe.cpp"
    lines = ['#include <cstddef>', '#include <cstdio>', '#include "bcplan.h"', 'int main() {']
    for f in fields:
        lines.append('    std::printf("%%s %%zu\\n", "%s", offsetof(bcp_episode_record, %s));' % (f, f))
    lines.append('    std::printf("sizeof %zu\\n", sizeof(bcp_episode_record));')
    lines.append('    return 0;\n}')
    src.write_text("\n".join(lines) + "\n")
    exe = tmp_path / "probe"
    subprocess.check_call([build.hipcc(), "-x", "c++", "-std=c++17", "-I", os.path.join(ROOT, "include"), str(src),
                           "-o", str(exe)])
    out = dict(line.split() for line in subprocess.check_output([str(exe)]).decode().splitlines())
    for f in fields:
        assert int(out[f]) == getattr(_lib.BcpEpisodeRecord, f).offset, f
    assert int(out["sizeof"]) == C.sizeof(_lib.BcpEpisodeRecord)
