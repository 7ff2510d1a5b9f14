"""md_expert_sense's argument check (include/md_expert_sense.h): check_common, the required pointers and the fields the kernel
reads by name, the alignment of the packed weights and of the beam table, and the two refused modes.  Every call here is refused
before any launch (MD_EINVAL / MD_EABI and a message that names what is wrong), so dummy pointers never reach a device."""
import ctypes as C

import pytest

from metadrive_ped_amd import _lib, abi

_BUF = C.create_string_buffer(4096)
DUMMY = (C.addressof(_BUF) + 15) & ~15
ARGS = ("weights", "beam_cs240", "noise", "action_out", "mlp_out", "obs_out")
# any vehicle config goes: the env's own lidar / detectors / obs_dim are not the expert's business
CONFIG = dict(struct_size=C.sizeof(abi.MdConfig), n_envs=8, agents_per_env=1, cap=32, n_beams=72, obs_dim=19 + 8 + 72 + 12,
              lidar_range=40.0, num_others=2, n_side=12, random_agent_model=1)


def _struct(cls, null=()):
    s = cls()
    for f, t in cls._fields_:
        if t is abi.P:
            setattr(s, f, None if f in null else DUMMY)
    return s


def _call(null=(), args=None, world=True, **cfg):
    lib = _lib.load()
    w, s, k = _struct(abi.MdWorld, null), _struct(abi.MdState, null), abi.MdConfig()
    for name, v in dict(CONFIG, **cfg).items():
        setattr(k, name, v)
    w.n_envs = 8
    a = dict({n: DUMMY for n in ARGS}, **(args or {}))
    rc = lib.md_expert_sense(C.byref(w) if world else None, C.byref(s), C.byref(k), a["weights"], a["beam_cs240"], a["noise"],
                             a["action_out"], a["mlp_out"], a["obs_out"], None)
    return rc, lib.md_last_error().decode()


def test_entry_point_has_a_table_of_its_own():
    assert "md_expert_sense" in abi.EXPERT_SENSE_ENTRY_POINTS
    assert "md_expert_sense" not in abi.EXPERT_ENTRY_POINTS and "md_expert_sense" not in abi.ENTRY_POINTS


def test_check_common_comes_first():
    assert _call(world=False) == (abi.MD_EINVAL, "null MdWorld/MdState/MdConfig pointer")
    rc, msg = _call(struct_size=4, args=dict(weights=None))
    assert rc == abi.MD_EABI and "struct_size" in msg
    rc, msg = _call(n_envs=0, args=dict(weights=None))
    assert rc == abi.MD_EINVAL and msg.startswith("bad sizes"), msg
    assert _call(null=("shape", ), args=dict(weights=None)) == (abi.MD_EINVAL, "MdState.shape is null")


@pytest.mark.parametrize("name", ["weights", "beam_cs240", "action_out"])
def test_required_arguments_by_name(name):
    assert _call(args={name: None}) == (abi.MD_EINVAL, "required pointer %s is null" % name)


@pytest.mark.parametrize("field", ["s->dyn", "s->param", "s->nav", "s->action", "s->final_lane", "s->need_reset", "w->env_map",
                                   "w->lanes", "w->lane_off", "w->roads", "w->road_off"])
def test_required_fields_by_name(field):
    assert _call(null=(field[3:], )) == (abi.MD_EINVAL, "required pointer %s is null" % field)


def test_the_envs_own_observation_is_not_required():
    """MdState.obs / detected are neither read nor written, MdWorld.beam_cs is replaced by beam_cs240: with them null the first
    complaint is still the one about a missing argument"""
    assert _call(null=("obs", "detected", "beam_cs"), args=dict(action_out=None)) == (abi.MD_EINVAL, "required pointer action_out is null")


def test_misaligned_tables_are_refused():
    assert _call(args=dict(weights=DUMMY + 4)) == (abi.MD_EINVAL, "md_expert_sense: the packed weights must be 16-byte aligned")
    assert _call(args=dict(beam_cs240=DUMMY + 8)) == (abi.MD_EINVAL, "md_expert_sense: the beam table beam_cs240 must be 16-byte aligned")


def test_scenario_and_tollgate_are_refused():
    rc, msg = _call(traffic_mode=4)
    assert rc == abi.MD_EINVAL and msg.startswith("md_expert_sense: not in scenario mode"), msg
    rc, msg = _call(is_multi_agent=1, agents_per_env=4, ma_kind=abi.MA_TOLLGATE)
    assert rc == abi.MD_EINVAL and msg.startswith("md_expert_sense: not in the tollgate env"), msg


def test_optional_arguments_may_be_null_but_nothing_is_launched_without_weights():
    assert _call(args=dict(noise=None, mlp_out=None, obs_out=None, weights=None)) == (abi.MD_EINVAL, "required pointer weights is null")
