"""md_ai_protect's argument check (include/md_ai_protect.h): check_common, the required pointers by name, the expert's observation
config and the alignment of the packed weights.  Every call here is refused before any launch (MD_EINVAL and a message that names
what is wrong), so dummy pointers never reach a device."""
import ctypes as C

import pytest

from metadrive_ped_amd import _lib, abi

_BUF = C.create_string_buffer(4096)
DUMMY = (C.addressof(_BUF) + 15) & ~15
ARGS = ("weights", "noise", "actions", "takeover", "expert_takeover", "applied_out", "flags_out", "saver_out")
CONFIG_MESSAGE = ("md_ai_protect: needs a single-agent batch with the expert's lidar (240 beams, 50 m, num_others 0), no side / "
                  "lane-line detector and random_agent_model off (obs_dim 259)")


def _struct(cls, null=()):
    s = cls()
    for f, t in cls._fields_:
        if t is abi.P:
            setattr(s, f, None if f in null else DUMMY)
    return s


def _call(null=(), args=None, save_level=0.5, world=True, **cfg):
    lib = _lib.load()
    w, s, k = _struct(abi.MdWorld, null), _struct(abi.MdState, null), abi.MdConfig()
    for name, v in dict(dict(struct_size=C.sizeof(abi.MdConfig), n_envs=8, agents_per_env=1, cap=32, n_beams=240, obs_dim=259,
                             lidar_range=50.0), **cfg).items():
        setattr(k, name, v)
    w.n_envs = 8
    a = dict({n: DUMMY for n in ARGS}, **(args or {}))
    rc = lib.md_ai_protect(C.byref(w) if world else None, C.byref(s), C.byref(k), a["weights"], a["noise"], a["actions"],
                           C.c_float(save_level), a["takeover"], a["expert_takeover"], a["applied_out"], a["flags_out"], a["saver_out"], None)
    return rc, lib.md_last_error().decode()


def test_entry_point_has_a_table_of_its_own():
    assert "md_ai_protect" in abi.AI_PROTECT_ENTRY_POINTS and "md_ai_protect" not in abi.EXPERT_ENTRY_POINTS
    assert "md_ai_protect" not in abi.ENTRY_POINTS


def test_check_common_comes_first():
    assert _call(world=False) == (abi.MD_EINVAL, "null MdWorld/MdState/MdConfig pointer")
    rc, msg = _call(struct_size=4)
    assert rc == abi.MD_EABI and "struct_size" in msg
    rc, msg = _call(n_envs=0)
    assert rc == abi.MD_EINVAL and msg.startswith("bad sizes"), msg


@pytest.mark.parametrize("name", ["weights", "actions", "takeover", "expert_takeover", "applied_out", "flags_out"])
def test_required_arguments_by_name(name):
    assert _call(args={name: None}) == (abi.MD_EINVAL, "required pointer %s is null" % name)


@pytest.mark.parametrize("field", ["s->obs", "s->detected", "s->dyn", "s->param", "s->nav", "w->env_map", "w->lanes", "w->lane_off",
                                   "w->roads", "w->road_off", "s->need_reset"])
def test_required_fields_by_name(field):
    assert _call(null=(field[3:], )) == (abi.MD_EINVAL, "required pointer %s is null" % field)


@pytest.mark.parametrize("kw", [dict(n_beams=120, obs_dim=139), dict(num_others=4, obs_dim=275), dict(lidar_range=30.0), dict(n_side=4),
                                dict(n_lane_line=2), dict(random_agent_model=1), dict(is_multi_agent=1), dict(agents_per_env=2),
                                dict(traffic_mode=4)])
def test_non_expert_config_is_refused(kw):
    assert _call(**kw) == (abi.MD_EINVAL, CONFIG_MESSAGE)


def test_misaligned_weights_are_refused():
    assert _call(args=dict(weights=DUMMY + 4)) == (abi.MD_EINVAL, "md_ai_protect: the packed weights must be 16-byte aligned")


@pytest.mark.parametrize("level", [-0.01, 1.01, float("nan")])
def test_save_level_outside_the_unit_interval_is_refused(level):
    rc, msg = _call(save_level=level)
    assert rc == abi.MD_EINVAL and msg.startswith("md_ai_protect: save_level="), msg


def test_optional_arguments_may_be_null_but_nothing_is_launched_without_weights():
    # noise and saver_out are optional: with them NULL the first complaint is still about a required argument
    assert _call(args=dict(noise=None, saver_out=None, weights=None)) == (abi.MD_EINVAL, "required pointer weights is null")
