"""Host-side checks of the pooled egocentric observation: the three symbols are exported and bound, and the numpy helper the
GPU tests take their expectations from (tests/ego_pooled_ref.py) is right -- against a double loop, and on the reference's
recorded images.  CPU only."""
import os

import numpy as np
import pytest

from ego_pooled_ref import block_max
from util import GOLDEN

NEW_SYMBOLS = ["bcp_egocentric_pooled_shape", "bcp_egocentric_costmaps_pooled", "bcp_final_egocentric_costmaps_pooled"]


def test_library_exports_the_pooled_symbols_and_lib_binds_them():
    import ctypes as C
    from bc_gym_planning_env_amd import _lib, build
    build.build()
    raw = C.CDLL(_lib.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert hasattr(raw, name), name
        assert name in _lib.SYMBOLS, name
    lib = _lib.load()
    assert lib.bcp_egocentric_pooled_shape.argtypes[2] is C.c_int32
    assert lib.bcp_egocentric_costmaps_pooled.argtypes[5:7] == [C.c_uint8, C.c_int32]
    assert lib.bcp_final_egocentric_costmaps_pooled.argtypes[3:5] == [C.c_int32, C.c_int32]
    assert _lib.EGO_KERNELS[6] == "ego_pooled_sparse_kernel" and _lib.EGO_KERNELS[7] == "ego_pooled_sampled_kernel"
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "bcplan.h")).read()
    assert "BCP_EGO_POOLED_SPARSE = 6" in header and "BCP_EGO_POOLED_SAMPLED = 7" in header


def _double_loop(img, pool):
    h, w = img.shape
    out = np.zeros((-(-h // pool), -(-w // pool)), dtype=img.dtype)
    for r in range(out.shape[0]):
        for c in range(out.shape[1]):
            best = 0
            for y in range(r * pool, min((r + 1) * pool, h)):
                for x in range(c * pool, min((c + 1) * pool, w)):
                    best = max(best, int(img[y, x]))
            out[r, c] = best
    return out


@pytest.mark.parametrize("shape", [(7, 5), (133, 117), (1, 1)])
@pytest.mark.parametrize("pool", [1, 2, 3, 8, 64])
def test_block_max_agrees_with_a_double_loop(shape, pool):
    rng = np.random.RandomState(shape[0] * 100 + pool)
    img = rng.randint(0, 256, shape).astype(np.uint8)
    img[rng.uniform(size=shape) < 0.6] = 0        # (zeros dominate, as in the images it is used on)
    got = block_max(img, pool)
    want = _double_loop(img, pool)
    assert got.shape == want.shape == (-(-shape[0] // pool), -(-shape[1] // pool)) and got.dtype == np.uint8
    assert (got == want).all()
    if pool == 1:
        assert (got == img).all()
    # a leading batch dimension is pooled image by image
    assert (block_max(np.stack([img, img[::-1]]), pool)[1] == _double_loop(img[::-1], pool)).all()


def test_block_max_of_oracle_image_equals_block_max_of_fixture_image(oracle):
    """g10_ego_mini_00: the helper on real data -- pooling the oracle's images and pooling the reference's recorded ones
    give the same thing, and some pooled cells are lit"""
    g = np.load(os.path.join(GOLDEN, "g10_ego_mini_00.npz"))
    res, org = float(g["resolution"]), g["origin"]
    rows, cols = [int(v) for v in g["image_shape"]]
    lit = 0
    for t in range(len(g["states"])):
        img = oracle.extract_egocentric(g["costmap"], org, res, g["states"][t][:3], g["window_origin"], g["window_size"])
        recorded = np.unpackbits(g["images"][t], axis=1)[:, :cols].astype(np.uint8) * 254
        assert img.shape == recorded.shape == (rows, cols)
        for pool in (2, 7, 8):
            a, b = block_max(img, pool), block_max(recorded, pool)
            assert a.shape == (-(-rows // pool), -(-cols // pool)) and (a == b).all(), (t, pool)
            lit += int((a != 0).sum())
    assert lit > 0
