"""md_swap_draw's argument check of the PG walk (MdState.walk.mode > 0 with traffic_mode 0 / 1 / 2): the fields the live state and the
pool (`staged`) must have, and the walk's own parameters.  Every call here is refused before any launch (MD_EINVAL and a message that
names what is missing), so dummy pointers never reach a device."""
import ctypes as C

import pytest

from metadrive_ped_amd import _lib, abi

_BUF = C.create_string_buffer(4096)
DUMMY = (C.addressof(_BUF) + 15) & ~15


def _state(null=()):
    s = abi.MdState()
    for f, t in abi.MdState._fields_:
        if t is abi.P:
            setattr(s, f, None if f in null else DUMMY)
    return s


def _config(**kw):
    k = abi.MdConfig()
    for name, v in dict(dict(struct_size=C.sizeof(abi.MdConfig), n_envs=8, agents_per_env=1, cap=32, n_beams=240, obs_dim=259), **kw).items():
        setattr(k, name, v)
    return k


def _swap(live_null=(), staged_null=(), walk=(4, 1, 8, 0, 0), n_draws=4, **cfg):
    lib = _lib.load()
    s, staged, k = _state(live_null), _state(staged_null), _config(**cfg)
    s.walk = abi.MdWalk(*walk)
    rc = lib.md_swap_draw(C.byref(s), C.byref(staged), C.byref(k), n_draws, C.c_void_p(DUMMY), None)
    return rc, lib.md_last_error().decode()


@pytest.mark.parametrize("field", ["scene_of", "walk_ep", "param", "route_nodes", "route_roads", "final_lane", "idm_rand"])
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_live_state_fields_are_required_by_name(field, mode):
    assert _swap(live_null=(field, ), traffic_mode=mode) == (abi.MD_EINVAL, "required pointer s->%s is null" % field)


@pytest.mark.parametrize("field", ["rng", "route_nodes0", "route_roads0", "final_lane0"])
def test_respawn_modes_require_the_stream_and_the_route_twins(field):
    for mode in (1, 2):
        assert _swap(live_null=(field, ), traffic_mode=mode) == (abi.MD_EINVAL, "required pointer s->%s is null" % field)


@pytest.mark.parametrize("field,modes", [("param", (0, 1, 2)), ("route_nodes", (0, 1, 2)), ("route_roads", (0, 1, 2)), ("final_lane", (0, 1, 2)),
                                         ("idm_rand", (0, 1, 2)), ("rng", (1, 2))])
def test_pool_fields_are_required(field, modes):
    for mode in modes:
        rc, msg = _swap(staged_null=(field, ), traffic_mode=mode)
        assert rc == abi.MD_EINVAL and "pool (staged) needs" in msg and field.split("_")[0] in msg, (mode, msg)


@pytest.mark.parametrize("kw", [dict(walk=(4, 3, 8, 0, 0)), dict(walk=(5, 1, 8, 0, 0)), dict(walk=(4, 1, 0, 0, 0)), dict(walk=(4, 2, 8, -1, 0)),
                                dict(agents_per_env=2), dict(is_multi_agent=1)])
def test_walk_parameters_are_checked(kw):
    rc, msg = _swap(**kw)
    assert rc == abi.MD_EINVAL and msg.startswith("md_swap_draw: the PG walk needs mode 1 or 2"), msg


def test_scenario_walk_keeps_its_own_check():
    rc, msg = _swap(live_null=("scene_of", ), traffic_mode=4, track_len=10)
    assert rc == abi.MD_EINVAL and msg.startswith("md_swap_draw: the scenario walk needs mode 1 or 2"), msg
