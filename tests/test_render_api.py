"""env.render() without a device: the mode names, the refusals by name, render() before reset(), the other modes' message and
the validation of the options (metadrive_ped_amd/render.py: check_options)."""
import pytest

from metadrive_ped_amd import render as rd
from metadrive_ped_amd.envs import BatchedMetaDriveEnv, BatchedMultiAgentRoundaboutEnv
from metadrive_ped_amd.envs.base import BatchedEnvBase


@pytest.fixture(scope="module")
def env():
    return BatchedMetaDriveEnv(dict(num_envs=4))


def test_mode_names_are_the_references():
    assert rd.TOPDOWN_MODES == ("top_down", "topdown", "bev", "birdview")


@pytest.mark.parametrize("mode", rd.TOPDOWN_MODES)
def test_render_before_reset(env, mode):
    assert env.top_down_renderer is None
    with pytest.raises(RuntimeError, match=r"call reset\(\) before render\(\)"):
        env.render(mode=mode)
    assert env.top_down_renderer is None


@pytest.mark.parametrize("args", [dict(), dict(mode=None), dict(mode="rgb_array"), dict(mode="human"), dict(mode="onscreen"), dict(mode="TOPDOWN"),
                                  dict(mode="rgb_array", window=True, text=dict(a=1), semantic_map=True)])
def test_other_modes_keep_their_message(env, args):
    with pytest.raises(NotImplementedError) as err:
        env.render(**args)
    assert str(err.value) == env.RENDER_MESSAGE and env.RENDER_MESSAGE.startswith(BatchedEnvBase.RENDER_MESSAGE)


def test_refusals_by_name(env):
    with pytest.raises(NotImplementedError, match="window=True"):
        env.render(mode="topdown", window=True)
    with pytest.raises(NotImplementedError, match="text"):
        env.render({"speed": 1.0}, mode="topdown")
    for name in ("semantic_map", "draw_target_vehicle_trajectory", "show_agent_name"):
        assert name in rd.REFUSED_OPTIONS
        with pytest.raises(NotImplementedError, match=name):
            env.render(mode="topdown", **{name: True})
        with pytest.raises(RuntimeError, match="reset"):      # unset, they are the reference's defaults
            env.render(mode="topdown", **{name: False})
    with pytest.raises(TypeError, match="no_such_option"):
        env.render(mode="topdown", no_such_option=1)
    with pytest.raises(RuntimeError, match="reset"):          # empty text, no window, a film size: accepted
        env.render(text={}, mode="bev", window=False, film_size=(2000, 2000))


@pytest.mark.parametrize("bad, match", [(dict(envs=[4]), "envs holds 4"), (dict(envs=[0, -1]), "envs holds -1"), (dict(envs=[]), "envs is empty"),
                                        (dict(screen_size=(1025, 100)), "screen_size"), (dict(screen_size=(100, 0)), "screen_size"),
                                        (dict(screen_size=100), "screen_size"), (dict(scaling=0), "scaling"), (dict(scaling=-2.0), "scaling"),
                                        (dict(num_stack=0), "num_stack"), (dict(num_stack=33), "num_stack"),
                                        (dict(history_smooth=-1), "history_smooth"), (dict(track_agent=1), "track_agent"),
                                        (dict(camera_position=(1.0, )), "camera_position"),
                                        (dict(camera_position=(1.0, float("nan"))), "camera_position")])
def test_options_are_validated_before_the_engine_is_asked_for(env, bad, match):
    with pytest.raises(ValueError, match=match):
        env.render(mode="topdown", **bad)


def test_track_agent_counts_the_agent_slots():
    ma = BatchedMultiAgentRoundaboutEnv(dict(num_envs=2, num_agents=6))
    with pytest.raises(ValueError, match="track_agent"):
        ma.render(mode="topdown", track_agent=6)
    with pytest.raises(RuntimeError, match="reset"):
        ma.render(mode="topdown", track_agent=5)


def test_check_options_normalises():
    o = rd.check_options(8, 1)
    assert o == dict(envs=(0, ), screen_size=(512, 512), scaling=5.0, num_stack=15, history_smooth=0, camera_position=None,
                     target_vehicle_heading_up=False, draw_contour=True, track_agent=0, screen_record=False)
    o = rd.check_options(8, 2, envs=[6, 1, 3], screen_size=[96, 80], scaling=2, camera_position=[1, 2], track_agent=1)
    assert o["envs"] == (6, 1, 3) and o["screen_size"] == (96, 80) and o["camera_position"] == (1.0, 2.0) and o["scaling"] == 2.0
    assert o == rd.check_options(8, 2, envs=(6, 1, 3), screen_size=(96, 80), scaling=2.0, camera_position=(1.0, 2.0), track_agent=1)
