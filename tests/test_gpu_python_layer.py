"""Seams of the Python layer that no comparison with the oracle crosses: every geometry mode refuses mixed resolutions, the
observation wrappers' final buffers follow the env's episode record through their common base, and the host copies of the
bound geometry follow world edits made one after the other."""
import numpy as np
import pytest

from bc_gym_planning_env_amd import CostMap2D, EnvParams

pytestmark = pytest.mark.gpu


def _map(resolution=0.05, side=40):
    data = np.zeros((side, side), dtype=np.uint8)
    data[0, 0] = 254   # (one lethal cell, in a corner the robot never comes near: no episode ends in these tests)
    return CostMap2D(data, resolution, np.array([0.0, 0.0]))


PATH = np.array([[0.5, 1.0, 0.0], [1.5, 1.0, 0.0]])


def test_templates_of_mixed_resolution_are_refused(torch_cuda):
    from bc_gym_planning_env_amd import BatchedPlanEnv
    with pytest.raises(ValueError, match="all costmaps must share one resolution"):
        BatchedPlanEnv([_map(0.05), _map(0.1)], [PATH, PATH], EnvParams(), n_envs=4, template_of_env=[0, 1, 0, 1])


def test_final_buffers_of_both_wrapper_families_follow_the_record(torch_cuda):
    torch = torch_cuda
    from bc_gym_planning_env_amd import BatchedPlanEnv, BatchedRangeScan
    from bc_gym_planning_env_amd.egocentric import BatchedEgocentricCostmap
    n = 4
    env = BatchedPlanEnv(_map(), PATH, EnvParams(), n_envs=n, auto_reset=True)
    wraps = [BatchedEgocentricCostmap(env, final_observation=True), BatchedRangeScan(env, n_beams=8, final_observation=True)]
    assert env.episode_ends is not None and env.episode_ends.capacity == n
    actions = torch.tensor([[float(env.action_space.low[0]), 0.0]] * n, dtype=torch.float64, device=env.device)
    for w in wraps:
        _obs, _r, _d, info = w.step(actions)
        assert all(t.shape[0] == n for t in info["final_observation"].values())
        assert "final_observation" not in env._info   # (a copy: the env's own info dict stays as it was)
    env.disable_episode_record()
    for w in wraps:
        with pytest.raises(RuntimeError) as raised:
            w.step(actions)
        assert str(raised.value) == ("final_observation=True needs the env's episode record (env.disable_episode_record() "
                                     "was called)")
    env.enable_episode_record(capacity=2)
    ego, scan = wraps
    for w in wraps:
        _obs, _r, _d, info = w.step(actions)
        assert [t.shape[0] for t in info["final_observation"].values()] == [2, 2]
    assert ego.final_images.shape == (2,) + ego.image_shape + (1,) and ego.final_vector.shape == (2, 9, 1)
    assert scan.final_scan.shape == (2, 8, 1) and scan.final_vector.shape == (2, 9, 1)
    assert list(ego._final_buffers().keys()) == ["env", "goal_n_state"] and ego._final_buffers()["env"] is ego.final_images
    assert list(scan._final_buffers().keys()) == ["scan", "goal_n_state"] and scan._final_buffers()["scan"] is scan.final_scan
    env.check_errors()


def _host_copies_follow_the_binding(env):
    """every env's host costmap and path -- costmap_of, path_of, and the State of its view -- hold the bytes of the tensors
    the library has bound, within the entry's valid shape and length"""
    maps, pts, lens = (env._keep[name].cpu().numpy() for name in ("map", "path", "lens"))
    vr, vc = (env._keep[name].cpu().numpy() if env._keep.get(name) is not None else np.full(len(maps), maps.shape[axis])
              for name, axis in (("vr", 1), ("vc", 2)))
    geom = env.geom_of_env.cpu().numpy() if env.geom_of_env is not None else np.arange(env.n_envs)
    for i, k in enumerate(geom):
        state = env.envs[i].get_state()
        for cm in (env.costmap_of(i), state.costmap):
            assert cm.get_data().shape == (vr[k], vc[k]) and (cm.get_data() == maps[k, :vr[k], :vc[k]]).all(), i
        for path in (env.path_of(i), state.original_path):
            assert path.shape == (lens[k], 3) and path.tobytes() == pts[k, :lens[k]].tobytes(), i
    return maps, pts, lens, vr, vc


def _edit_worlds_in_sequence(env, after):
    before = env._keep["map"].clone()
    env.scatter_obstacles(n_boxes=2, half_size=(0.2, 0.4), seed=3)
    assert not bool((env._keep["map"] == before).all())   # (the sequence does edit the worlds)
    after()
    env.inflate_costmaps(3.0)
    after()
    straight = env._keep["path"].clone()
    status = env.route_paths(cost_weight=2)
    assert bool((status == 0).any()) and not bool((env._keep["path"] == straight).all())
    after()


def test_world_edits_in_sequence_keep_the_host_copies(torch_cuda):
    """scatter_obstacles, inflate_costmaps, route_paths one after the other: on expanded templates the host copies become one
    per env with the first edit and stay so; on a device-resident pool they are copies of the pool's own tensors"""
    import goal_field_ref as GR
    import goal_route_ref as RR
    from bc_gym_planning_env_amd import BatchedPlanEnv, mini_env
    worlds, of = (0, 17), np.array([0, 1, 1, 0])
    maps, paths = [], []
    for w in worlds:
        data, origin, res, _g, _s = GR.mini_world(w)
        maps.append(CostMap2D(data.copy(), res, origin))
        paths.append(np.stack(RR.mini_world_poses(w)))
    params = EnvParams(goal_ang_dist=np.pi / 8., goal_spat_dist=0.2)
    env = BatchedPlanEnv(maps, paths, params, n_envs=4, template_of_env=of)
    _host_copies_follow_the_binding(env)
    _edit_worlds_in_sequence(env, lambda: _host_copies_follow_the_binding(env))
    assert len(env._costmaps) == len(env._paths) == 4

    pool_env = mini_env.BatchedRandomMiniEnv(4, mini_env.RandomMiniEnvParams(env_params=params), seeds=[1, 2], episodes=2,
                                             sampler="device_resident", auto_reset=True, seed=2)
    dp = pool_env.pool
    assert pool_env._device_pool is dp and len(dp) == 4

    def pool_entries_follow():
        assert pool_env._keep["map"] is dp.maps and pool_env._keep["path"] is dp.path_points and pool_env._keep["lens"] is dp.lens
        data, pts, lens, vr, vc = _host_copies_follow_the_binding(pool_env)
        assert len(pool_env._costmaps) == len(pool_env._paths) == 4
        for k in range(4):
            assert (pool_env._costmaps[k].get_data() == data[k, :vr[k], :vc[k]]).all()
            assert pool_env._paths[k].tobytes() == pts[k, :lens[k]].tobytes()

    pool_entries_follow()
    _edit_worlds_in_sequence(pool_env, pool_entries_follow)
