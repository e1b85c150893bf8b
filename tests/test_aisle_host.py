"""Host side of the aisle-turn pool (bc_gym_planning_env_amd/aisle_env.py) against the reference's own worlds: the
AisleTurnEnv trajectories of g8 (fixed turns), the RandomAisleTurnEnv chains of g14 and the coloured egocentric
recording of g12 (tools/gen_aisle_golden.py, oracle/gen_golden.py, both from the genuine reference).  CPU only."""
import os

import numpy as np
import pytest

from bc_gym_planning_env_amd import aisle_env, host_init
from bc_gym_planning_env_amd.api import EnvParams

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")

G8 = [("default", dict(), dict()),
      ("c4_00", dict(resolution=10. / 256), dict()),
      ("c4_10", dict(resolution=10. / 256), dict(flip_arnd_oy=True)),
      ("c4_01", dict(resolution=10. / 256), dict(flip_arnd_ox=True)),
      ("c4_11", dict(resolution=10. / 256), dict(flip_arnd_oy=True, flip_arnd_ox=True))]


def g14():
    return np.load(os.path.join(GOLDEN, "g14_aisle_worlds.npz"))


def lethal_of(g, k):
    rows, cols = [int(v) for v in g["shape"].reshape(-1, 2)[k]]
    bits = g["lethal"][g["lethal_offset"][k]:g["lethal_offset"][k + 1]].reshape(rows, -1)
    return np.unpackbits(bits, axis=1)[:, :cols].astype(bool)


@pytest.mark.parametrize("tag,ekw,tkw", G8, ids=[v[0] for v in G8])
def test_path_and_costmap_reproduce_g8_aisle(tag, ekw, tkw):
    g = np.load(os.path.join(GOLDEN, "g8_traj_aisle_%s.npz" % tag))
    ep = EnvParams(**ekw)
    path, costmap = aisle_env.path_and_costmap_from_config(
        aisle_env.AisleTurnEnvParams(env_params=ep, turn_params=aisle_env.TurnParams(**tkw)))
    assert path.shape == (4, 3)
    assert costmap.get_data().shape == g["costmap"].shape
    assert (costmap.get_data() == g["costmap"]).all()
    assert (costmap.get_origin() == g["origin"]).all()
    refined = host_init.refine_path(path, ep.path_delta)
    assert refined.shape == g["path"].shape and (refined == g["path"]).all()


def test_draw_random_turn_params_consumes_eight_doubles():
    a, b = np.random.RandomState(5), np.random.RandomState(5)
    aisle_env.draw_random_turn_params(a)
    b.random_sample(8)
    assert a.random_sample() == b.random_sample()


def test_host_sampler_reproduces_g14():
    g = g14()
    seeds, K = [int(s) for s in g["seeds"]], g["turn_params"].shape[1]
    assert len(seeds) >= 12 and K >= 4
    pool = aisle_env.sample_aisle_pool(EnvParams(), seeds, K)
    assert len(pool) == len(seeds) * K
    for k in range(len(pool)):
        s, e = divmod(k, K)
        w = pool.worlds[k]
        mine = np.array([w.main_corridor_length, w.turn_corridor_length, w.turn_corridor_angle, w.main_corridor_width,
                         w.turn_corridor_width, w.flip_arnd_oy, w.flip_arnd_ox, w.rot_theta], dtype=np.float64)
        assert (mine == g["turn_params"][s, e]).all(), k
        cm = pool.costmaps[k]
        assert cm.get_data().shape == tuple(g["shape"][s, e])
        assert (cm.get_origin() == g["origin"][s, e]).all()
        assert ((cm.get_data() == 254) == lethal_of(g, k)).all(), k
        assert set(np.unique(cm.get_data())) <= {0, 254}
        assert (pool.paths[k] == g["coarse_path"][s, e]).all()
        refined = host_init.refine_path(pool.paths[k], 0.05)
        want = g["path"][g["path_offset"][k]:g["path_offset"][k + 1]]
        assert refined.shape == want.shape and (refined == want).all(), k
        md, ti = host_init.initial_reward_state(refined, EnvParams().reward_provider_params)
        assert md == g["init"][s, e, 0] and ti == g["init"][s, e, 1]
    nxt = pool.next_geom.reshape(len(seeds), K)
    assert (nxt[:, :-1] == np.arange(1, K) + np.arange(len(seeds))[:, None] * K).all()
    assert (nxt[:, -1] == np.arange(len(seeds)) * K).all()


def test_seed_3_world_0_is_g12():
    """g12 was recorded as ColoredEgoCostmapRandomAisleTurnEnv(); seed(3); reset(): world 0 of chain 3."""
    g = np.load(os.path.join(GOLDEN, "g12_colored_ego.npz"))
    pool = aisle_env.sample_aisle_pool(EnvParams(), [3], 1)
    cm = pool.costmaps[0]
    assert cm.get_data().shape == g["costmap"].shape and (cm.get_data() == g["costmap"]).all()
    assert (cm.get_origin() == g["origin"]).all()
    assert (host_init.refine_path(pool.paths[0], 0.05) == g["path"]).all()


def test_thick_walls_are_refused():
    cfg = aisle_env.AisleTurnEnvParams(env_params=EnvParams(resolution=0.02))
    with pytest.raises(NotImplementedError):
        aisle_env.path_and_costmap_from_config(cfg)
