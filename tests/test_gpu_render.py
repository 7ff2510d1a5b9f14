"""env.render(mode="topdown") on the device (include/md_render.h; csrc/parts/render.inc rasterises tile by tile in primitive order and settles
the painter's order through ranks) against the host build of the same header (tests/render_host.c, pixel order): after every call
the state, MdWorld.env_map and the viewer's history are downloaded, the host build runs on them and the WHOLE output tensor, the
ring and the cursors are compared bit for bit."""
import numpy as np
import pytest

import render_host as rh
from helpers import scripted_actions
from metadrive_ped_amd import abi

pytestmark = pytest.mark.gpu

GREEN, PROP, CONTOUR, WHITE = (2, 158, 115), (235, 84, 42), (60, 60, 60), (255, 255, 255)
PALETTE = [(1, 115, 178), (222, 143, 5), (213, 94, 0), (204, 120, 188), (202, 145, 97), (251, 175, 228), (148, 148, 148), (236, 225, 51),
           (86, 180, 233)]


def _colours(img):
    return {tuple(int(v) for v in c) for c in np.unique(img.reshape(-1, 3), axis=0)}


def _run(env, steps, act, compare=True, **opts):
    """reset, then `steps` steps, a render call after the reset and after every step -> (pictures, cursors after every call,
    downloaded states)"""
    import torch
    env.reset()
    eng = env.engine
    host = rh.HostRender(eng.host, **{k: v for k, v in opts.items() if k != "mode"})
    n = len(opts.get("envs", (0, )))
    W, H = opts.get("screen_size", (512, 512))
    imgs, cursors, states = [], [], []
    for t in range(steps + 1):
        if t > 0:
            env.step(act(t - 1))
        before = env.top_down_renderer.history() if env.top_down_renderer is not None else None
        out = env.render(mode="topdown", **opts)
        assert tuple(out.shape) == (n, H, W, 3) and out.dtype == torch.uint8 and out.device == eng.device
        img = out.cpu().numpy().copy()
        after = env.top_down_renderer.history()
        st = eng.download_state()
        if compare:
            env_map = eng.world_dev["env_map"].view(torch.int32).cpu().numpy().copy()
            want = host.render(st, env_map=env_map, hist=before)
            bad = np.argwhere(img != want)
            assert bad.size == 0, ("call %d" % t, len(bad), bad[:5], img[tuple(bad[0])], want[tuple(bad[0])])
            assert after["ring"].tobytes() == host.hist["ring"].tobytes(), t
            assert np.array_equal(after["cursor"], host.hist["cursor"]), (t, after["cursor"], host.hist["cursor"])
        imgs.append(img)
        cursors.append(after["cursor"])
        states.append(st)
    return imgs, cursors, states


def _single_actions(env):
    import torch
    E = env.num_envs
    return lambda t: torch.from_numpy(scripted_actions(E, 1, t).reshape(E, 2)).to(env.engine.device)


def test_single_agent_unordered_envs_partial_tiles_and_auto_resets():
    from metadrive_ped_amd.envs import BatchedMetaDriveEnv
    env = BatchedMetaDriveEnv(dict(num_envs=8, map=3, traffic_mode="respawn", traffic_density=0.3, horizon=12))
    ids = [6, 1, 3]
    imgs, cursors, states = _run(env, 30, _single_actions(env), envs=ids, screen_size=(96, 80), scaling=2, num_stack=4)
    cap = env.engine.cap
    resets = np.zeros(3, int)
    movers = 0
    for t, (img, cur, st) in enumerate(zip(imgs, cursors, states)):
        clock = st["nav"]["steps"].reshape(8, cap)[ids, 0]
        sh = st["shape"].reshape(8, cap)
        for i, e in enumerate(ids):
            if clock[i] == 0:      # the reset step: the history starts again with this frame
                resets[i] += t > 0
                assert cur[i].tolist() == [0, 1, 0, 0], (t, e, cur[i])
            assert cur[i, 2] == clock[i] and 1 <= cur[i, 1] <= 4
            # a traffic vehicle whose centre lies in the window shows there (its own colour, a contour, or a box above it)
            for j in range(1, cap):
                fl = int(sh["flags"][e, j])
                if not (fl & abi.F_ALIVE) or (fl & abi.KIND_MASK) != abi.KIND_VEHICLE:
                    continue
                row = int(np.floor(40 - (float(sh["cy"][e, j]) - float(sh["cy"][e, 0])) * 2))
                col = int(np.floor(48 + (float(sh["cx"][e, j]) - float(sh["cx"][e, 0])) * 2))
                if 1 <= row < 79 and 1 <= col < 95:
                    assert tuple(int(v) for v in img[i, row, col]) in set(PALETTE) | {CONTOUR, PROP}, (t, e, j)
                    movers += 1
    assert (resets >= 1).all(), resets
    assert max(c[:, 1].max() for c in cursors) == 4
    assert movers > 0
    lib = rh.lib()
    green = GREEN[0] | (GREEN[1] << 8) | (GREEN[2] << 16)
    faded = {rh.rgb(lib.hx_rd_fade(green, n, k)) for n in (2, 3, 4) for k in range(n - 1)} - {WHITE}
    assert any(faded & _colours(img) for img in imgs)
    assert all(CONTOUR in _colours(img) for img in imgs)
    env.close()


def test_one_tile_heading_up_smoothed_history_no_contour():
    from metadrive_ped_amd.envs import BatchedMetaDriveEnv
    env = BatchedMetaDriveEnv(dict(num_envs=4, map=3, traffic_mode="respawn", traffic_density=0.3, horizon=12))
    imgs, cursors, _ = _run(env, 15, _single_actions(env), envs=[2], screen_size=(64, 64), target_vehicle_heading_up=True, history_smooth=2,
                            draw_contour=False)
    assert all(tuple(int(v) for v in img[0, 31, 32]) == GREEN for img in imgs)      # the tracked agent, at the centre, looking up
    assert all(CONTOUR not in _colours(img) for img in imgs)
    # the horizon of 12 ends every episode inside the run: the history grows past two frames (so that frames are skipped) and starts again
    assert max(c[0, 1] for c in cursors) > 2 and any(c[0].tolist()[:2] == [0, 1] for c in cursors[1:])
    env.close()


def test_odd_width_takes_the_scalar_store_path():
    """W = 50 is no multiple of 16: the rows are written byte by byte; H = 70 has a partial tile below a full one"""
    from metadrive_ped_amd.envs import BatchedMetaDriveEnv
    env = BatchedMetaDriveEnv(dict(num_envs=2, map=3, traffic_mode="respawn", traffic_density=0.3, horizon=12))
    _run(env, 5, _single_actions(env), envs=[1, 0], screen_size=(50, 70), scaling=1.5, num_stack=3)
    env.close()


def _roundabout(compare, **look):
    import torch
    from metadrive_ped_amd.envs import BatchedMultiAgentRoundaboutEnv
    env = BatchedMultiAgentRoundaboutEnv(dict(num_envs=2))
    E, A = 2, env.num_agents
    env.lazy_init()
    q = env.engine.host.world.arrays["quads"].reshape(-1, 8)
    centre = (float(q[:, 0::2].min() + q[:, 0::2].max()) / 2.0, float(q[:, 1::2].min() + q[:, 1::2].max()) / 2.0)
    act = lambda t: torch.from_numpy(scripted_actions(E, A, t)).to(env.engine.device)
    imgs, cursors, states = _run(env, 20, act, compare=compare, envs=[0, 1], camera_position=centre, scaling=1.5, screen_size=(160, 160), **look)
    env.close()
    return imgs, cursors, states


def test_multi_agent_fixed_camera_and_repeatable():
    """At 1.5 pixels per metre a vehicle's 1.8 m are narrower than two contours (2 pixels = 1.33 m each): with contours every agent of
    the current frame is all contour and no pixel is green.  So the run that looks for green draws none; the run with the default
    contours is compared bit for bit all the same and shows them in every frame."""
    first, cursors, states = _roundabout(True, draw_contour=False)
    second, _, _ = _roundabout(False, draw_contour=False)
    assert len(first) == len(second) == 21
    for a, b in zip(first, second):
        assert np.array_equal(a, b)
    assert all(GREEN in _colours(img[i]) for img in first for i in range(2))
    assert cursors[-1][:, 1].tolist() == [15, 15]
    assert cursors[-1][:, 2].tolist() == states[-1]["env_steps"].reshape(-1).tolist()      # MdState.env_steps is the clock
    contoured, _, _ = _roundabout(True)
    assert all(CONTOUR in _colours(img[i]) for img in contoured for i in range(2))


def test_scenario_mode_draws_the_polyline_maps_lines():
    import torch
    from metadrive_ped_amd.envs.scenario_env import BatchedScenarioEnv
    from metadrive_ped_amd.scenario import synthetic_scenarios
    env = BatchedScenarioEnv(dict(num_envs=4, num_scenarios=4), scenarios=synthetic_scenarios(4, 900, T=80))
    act = lambda t: torch.from_numpy(scripted_actions(4, 1, t).reshape(4, 2)).to(env.engine.device)
    imgs, _, _ = _run(env, 10, act, envs=[3, 0], screen_size=(128, 96), scaling=2, num_stack=5)
    lines = {(255, 175, 35), (175, 175, 175), (95, 95, 95)}
    assert all(lines & _colours(img[i]) for img in imgs for i in range(2))
    env.close()


def test_props_and_a_spawned_pedestrian_at_their_table_sizes():
    """an accident scene's cones (4 * RADIUS square, (235, 84, 42)) and a spawned pedestrian (2 * RADIUS square, its slot's palette
    colour), looked at from a fixed camera at 10 pixels per metre, without contours"""
    import torch
    from metadrive_ped_amd.envs import BatchedSafeMetaDriveEnv
    env = BatchedSafeMetaDriveEnv(dict(num_envs=2, num_scenarios=2, start_seed=0, mover_capacity=128))
    env.reset()
    eng = env.engine
    cap = eng.cap
    sh = eng.download_state()["shape"].reshape(2, cap)
    cones = np.nonzero((sh["flags"][0] & abi.KIND_MASK) == abi.KIND_CONE)[0]
    assert len(cones) > 0
    cone = sh[0, cones[0]]
    cam = (float(cone["cx"]) + 1.0, float(cone["cy"]))
    ped_at = (cam[0] + 3.0, cam[1] + 2.0)
    slot = env.spawn_object("pedestrian", [ped_at[0], ped_at[1]], 0.4)
    opts = dict(envs=[0], screen_size=(128, 128), scaling=10, camera_position=cam, draw_contour=False, num_stack=2)
    img = env.render(mode="topdown", **opts).cpu().numpy().copy()[0]
    host = rh.HostRender(eng.host, **opts)
    want = host.render(eng.download_state(), env_map=eng.world_dev["env_map"].view(torch.int32).cpu().numpy().copy())[0]
    assert np.array_equal(img, want)

    def at(x, y):
        return tuple(int(v) for v in img[int(np.floor(64 - (y - cam[1]) * 10)), int(np.floor(64 + (x - cam[0]) * 10))])
    c, s = float(cone["c"]), float(cone["s"])
    assert at(float(cone["cx"]), float(cone["cy"])) == PROP
    for d in (-0.3, 0.3):      # a pixel (0.1 m) beyond the body's RADIUS 0.2, inside the drawn half size 0.4, along both axes of the square
        assert at(float(cone["cx"]) + d * c, float(cone["cy"]) + d * s) == PROP
        assert at(float(cone["cx"]) - d * s, float(cone["cy"]) + d * c) == PROP
    assert at(float(cone["cx"]) + 0.6 * c, float(cone["cy"]) + 0.6 * s) != PROP       # the next cone of the row stands 2 m away
    pc, ps = np.cos(0.4), np.sin(0.4)
    assert at(*ped_at) == PALETTE[slot % 9]
    for d in (-0.25, 0.25):
        assert at(ped_at[0] + d * pc, ped_at[1] + d * ps) == PALETTE[slot % 9]
        assert at(ped_at[0] - d * ps, ped_at[1] + d * pc) == PALETTE[slot % 9]
    for d in (-0.45, 0.45):
        assert at(ped_at[0] + d * pc, ped_at[1] + d * ps) != PALETTE[slot % 9]
    env.close()


def test_rendering_does_not_disturb_the_simulation():
    from metadrive_ped_amd.envs import BatchedMetaDriveEnv
    runs = []
    for render in (False, True):
        env = BatchedMetaDriveEnv(dict(num_envs=8, map=3, traffic_mode="respawn", traffic_density=0.3, horizon=12))
        obs, _ = env.reset()
        act = _single_actions(env)
        out = [obs.cpu().numpy().copy()]
        for t in range(20):
            if render:
                env.render(mode="topdown", envs=[0, 5], screen_size=(96, 80), scaling=2)
            obs, rew, term, trunc, _ = env.step(act(t))
            out += [obs.cpu().numpy().copy(), rew.cpu().numpy().copy(), term.cpu().numpy().copy(), trunc.cpu().numpy().copy()]
        runs.append(out)
        env.close()
    assert len(runs[0]) == len(runs[1])
    for a, b in zip(*runs):
        assert np.array_equal(a, b)


def test_options_are_fixed_by_the_first_call_and_reset_drops_the_renderer():
    from metadrive_ped_amd.envs import BatchedMetaDriveEnv
    env = BatchedMetaDriveEnv(dict(num_envs=2, map=3))
    env.reset()
    assert env.top_down_renderer is None
    a = env.render(mode="bev", screen_size=(64, 64), screen_record=True)
    r = env.top_down_renderer
    assert r is not None and env.render(mode="birdview", screen_size=(64, 64), screen_record=True) is a
    assert len(r.screen_frames) == 2 and r.screen_frames[0].shape == (1, 64, 64, 3)
    with pytest.raises(ValueError, match="scaling, screen_size"):
        env.render(mode="topdown", screen_size=(32, 64), scaling=4, screen_record=True)
    env.reset()
    assert env.top_down_renderer is None
    assert tuple(env.render(mode="top_down", screen_size=(32, 64), scaling=4).shape) == (1, 64, 32, 3)
    env.close()
    assert env.top_down_renderer is None
