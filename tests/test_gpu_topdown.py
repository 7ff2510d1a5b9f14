"""md_topdown on the device (include/md_topdown.h; csrc/parts/topdown.inc rasterises in primitive order into an LDS image) against the host
build of the same header (tests/topdown_host.c, pixel order): after every step the state and the history arrays are downloaded, the
host build runs on them and the WHOLE tensor and the history it leaves are compared bit for bit.  Every env auto-resets inside the
run; an env whose episode ended in a step is rendered on the map and the route it had in that step (MdWorld.env_map and
MdState.route_roads read before the step: the swap of a walk, which follows md_topdown, hands the env its next scene's).
The history on the device: a stacked traffic channel is the newest channel of frame_skip steps ago, a reset observation repeats
the current frame and holds one past position."""
import numpy as np
import pytest

import topdown_host as th
from helpers import scripted_actions

pytestmark = pytest.mark.gpu

BASE = dict(num_envs=8, num_scenarios=8, map=3, traffic_density=0.3, horizon=25)


def _run(cls_name, user, steps, compare=True):
    """-> (per-step images, per-step episode lengths, resets seen per env)"""
    import torch
    from metadrive_ped_amd import envs
    env = getattr(envs, cls_name)(dict(BASE, **user))
    cfg = env.config
    E, skip, stack = cfg["num_envs"], cfg["frame_skip"], cfg["frame_stack"]
    obs, _ = env.reset()
    eng = env.engine
    host = th.HostTopDown.of_config(eng.host, cfg)
    assert tuple(obs.shape) == env.observation_space.shape[:0] + (E, ) + env.observation_space.shape
    assert obs.dtype == (torch.float32 if cfg["norm_pixel"] else torch.uint8) and obs.device == eng.device

    def env_map():
        return eng.world_dev["env_map"].view(torch.int32).cpu().numpy().copy()

    def steps_of(st):
        return st["nav"]["steps"].reshape(E, -1)[:, 0].copy()

    st = eng.download_state()
    assert (steps_of(st) == 0).all()
    imgs, lens = [obs.cpu().numpy().copy()], [steps_of(st)]
    hist = eng.topdown_history()
    assert (hist["cursor"] == 0).all()
    for ch in range(3, 2 + stack):      # the reset observation: every traffic channel the current frame, one past position
        assert np.array_equal(imgs[0][..., ch], imgs[0][..., 2])
    assert ((imgs[0][..., 1] != 0).reshape(E, -1).sum(1) == 1).all()
    resets = np.zeros(E, int)
    for t in range(steps):
        before_map, before_hist = env_map(), eng.topdown_history()
        before_route = eng.state_dev["route_roads"].cpu().numpy().copy()
        a = torch.from_numpy(scripted_actions(E, 1, t).reshape(E, 2)).to(eng.device)
        obs, _, _, _, _ = env.step(a)
        img = obs.cpu().numpy().copy()
        st = eng.download_state()
        if compare:
            seen = dict(st, route_roads=before_route.view(st["route_roads"].dtype).reshape(st["route_roads"].shape))
            want = host.observe(seen, env_map=before_map, hist=before_hist)
            after = eng.topdown_history()
            bad = np.argwhere(img != want)
            assert bad.size == 0, ("step %d" % t, len(bad), bad[:5], img[tuple(bad[0])], want[tuple(bad[0])])
            for k in after:
                assert np.array_equal(after[k], host.hist[k]), (t, k)
        n = steps_of(st)
        for e in range(E):
            if n[e] == 0:       # this step returned env e's reset observation
                resets[e] += 1
                for ch in range(3, 2 + stack):
                    assert np.array_equal(img[e, ..., ch], img[e, ..., 2]), (t, e, ch)
                assert (img[e, ..., 1] != 0).sum() == 1, (t, e)
            elif stack > 1 and n[e] >= skip:      # no reset since the frame of frame_skip steps ago
                assert np.array_equal(img[e, ..., 3], imgs[-skip][e, ..., 2]), (t, e)
        imgs.append(img)
        lens.append(n)
    if cfg["norm_pixel"]:
        assert min(i.min() for i in imgs) >= 0.0 and max(i.max() for i in imgs) <= 1.0
    assert (resets >= 1).all(), resets
    assert all((i[..., 0] != 0).any() for i in imgs)
    env.close()
    return imgs


def test_default_sizes_bit_exact_and_repeatable():
    """R = 84, distance 30, stack 3, skip 5, float32 (the 16-byte store path); a second run gives identical tensors"""
    first = _run("BatchedTopDownMetaDrive", {}, 40)
    second = _run("BatchedTopDownMetaDrive", {}, 40, compare=False)
    assert len(first) == len(second) == 41
    for a, b in zip(first, second):
        assert np.array_equal(a, b)


def test_traffic_in_view():
    """With the trigger traffic of the runs above no vehicle comes inside 30 m within an episode of 25 steps; the respawn mode's
    traffic drives all over the map, so here the traffic channels carry vehicles in every frame"""
    imgs = _run("BatchedTopDownMetaDrive", dict(traffic_mode="respawn"), 40)
    assert all((i[..., 2] != 0).reshape(8, -1).any(1).sum() >= 4 for i in imgs)
    assert any((i[..., 3] != i[..., 2]).any() for i in imgs)


def test_small_odd_sizes_bytes_lidar_off():
    """R = 33, distance 20, stack 2, skip 3, uint8 (a block that is no multiple of 16 bytes: the scalar store path), in the V2 env"""
    imgs = _run("BatchedTopDownMetaDriveEnvV2", dict(resolution_size=33, distance=20, frame_stack=2, frame_skip=3, norm_pixel=False), 40)
    assert imgs[0].shape == (8, 33, 33, 4) and imgs[0].dtype == np.uint8
    assert set(np.unique(np.concatenate([i[..., 2].ravel() for i in imgs]))) <= {0, 176}
    assert set(np.unique(np.concatenate([i[..., 1].ravel() for i in imgs]))) == {0, 255}


def test_odd_size_whose_bit_planes_are_an_odd_number_of_words():
    """R = 85: a plane of 85 * 3 words; the parts of the LDS image behind the planes (the waves' queues and piece lists, written 16
    bytes at a time, the staged frames) must still start on 16 bytes.  Respawn traffic, so that lines, lanes and movers are all drawn"""
    imgs = _run("BatchedTopDownMetaDrive", dict(resolution_size=85, traffic_mode="respawn"), 30)
    assert imgs[0].shape == (8, 85, 85, 5) and any((i[..., 2] != 0).any() for i in imgs)


def test_checkpoint_carries_the_image_history():
    """get_state() / set_state(): after a detour of 7 steps the restored batch replays the same images, stacked frames and past
    positions included"""
    import torch
    from metadrive_ped_amd.envs import BatchedTopDownMetaDrive
    env = BatchedTopDownMetaDrive(dict(BASE, traffic_mode="respawn", resolution_size=40))
    env.reset()
    act = lambda t: torch.from_numpy(scripted_actions(8, 1, t).reshape(8, 2)).to(env.engine.device)
    for t in range(12):
        env.step(act(t))
    ck = env.get_state()
    want = [env.step(act(t))[0].cpu().numpy().copy() for t in range(12, 19)]
    env.set_state(ck)
    got = [env.step(act(t))[0].cpu().numpy().copy() for t in range(12, 19)]
    for a, b in zip(want, got):
        assert np.array_equal(a, b)
    assert any((a[..., 3] != a[..., 2]).any() for a in want)
    del ck["__topdown_cursor__"]
    with pytest.raises(ValueError, match="top-down history"):
        env.set_state(ck)


def test_walking_envs_are_rendered_on_the_map_of_the_episode_that_ended():
    _run("BatchedTopDownMetaDrive", dict(walk_scenarios=True, num_scenarios=16, norm_pixel=False), 30)      # uint8 through the 16-byte store path
