"""md_topdown's argument check (include/md_topdown.h): check_common first, the required pointers and the fields the kernel reads by
name, MdTopDown.struct_size, the limits the header defines and the two refused configurations.  Every call here is refused before
any launch (MD_EINVAL / MD_EABI and a message that names what is wrong), so dummy pointers never reach a device."""
import ctypes as C

import pytest

from metadrive_ped_amd import _lib, abi

_BUF = C.create_string_buffer(4096)
DUMMY = (C.addressof(_BUF) + 15) & ~15
CONFIG = dict(struct_size=C.sizeof(abi.MdConfig), n_envs=8, agents_per_env=1, cap=32, n_beams=0, obs_dim=19)
TOPDOWN = dict(struct_size=C.sizeof(abi.MdTopDown), resolution=84, distance=30.0, frame_stack=3, frame_skip=5, post_stack=5, norm_pixel=1)


def _struct(cls, null=()):
    s = cls()
    for f, t in cls._fields_:
        if t is abi.P:
            setattr(s, f, None if f in null else DUMMY)
    return s


def _call(null=(), td_null=(), world=True, with_td=True, cfg=None, **td_fields):
    lib = _lib.load()
    w, s, k, td = _struct(abi.MdWorld, null), _struct(abi.MdState, null), abi.MdConfig(), _struct(abi.MdTopDown, td_null)
    for name, v in dict(CONFIG, **(cfg or {})).items():
        setattr(k, name, v)
    for name, v in dict(TOPDOWN, **td_fields).items():
        setattr(td, name, v)
    w.n_envs, w.n_maps = 8, 1
    rc = lib.md_topdown(C.byref(w) if world else None, C.byref(s), C.byref(k), C.byref(td) if with_td else None, None)
    return rc, lib.md_last_error().decode()


def test_entry_point_has_a_table_of_its_own():
    assert list(abi.TOPDOWN_ENTRY_POINTS) == ["md_topdown"]
    for table in (abi.ENTRY_POINTS, abi.EXPERT_ENTRY_POINTS, abi.AI_PROTECT_ENTRY_POINTS, abi.EXPERT_SENSE_ENTRY_POINTS,
                  abi.CURRICULUM_ENTRY_POINTS):
        assert "md_topdown" not in table
    assert abi.MD_ABI_VERSION == 12


def test_check_common_comes_first():
    assert _call(world=False, with_td=False) == (abi.MD_EINVAL, "null MdWorld/MdState/MdConfig pointer")
    rc, msg = _call(cfg=dict(struct_size=4), with_td=False)
    assert rc == abi.MD_EABI and "MdConfig.struct_size" in msg
    rc, msg = _call(cfg=dict(n_envs=0), with_td=False)
    assert rc == abi.MD_EINVAL and msg.startswith("bad sizes"), msg
    assert _call(null=("shape", ), with_td=False) == (abi.MD_EINVAL, "MdState.shape is null")


def test_the_argument_block_and_its_size():
    assert _call(with_td=False) == (abi.MD_EINVAL, "required pointer td is null")
    rc, msg = _call(struct_size=C.sizeof(abi.MdTopDown) - 8, td_null=("out", ))
    assert rc == abi.MD_EABI and msg == "MdTopDown.struct_size=%d, library expects %d" % (C.sizeof(abi.MdTopDown) - 8, C.sizeof(abi.MdTopDown))


@pytest.mark.parametrize("name", ["out", "ring_traffic", "ring_pos", "cursor"])
def test_required_arguments_by_name(name):
    assert _call(td_null=(name, )) == (abi.MD_EINVAL, "required pointer td->%s is null" % name)


@pytest.mark.parametrize("field", ["s->nav", "s->route_roads", "w->env_map", "w->lane_off", "w->lanes", "w->road_off", "w->roads",
                                   "w->quad_off", "w->quads", "w->quad_kind"])
def test_required_fields_by_name(field):
    assert _call(null=(field[3:], )) == (abi.MD_EINVAL, "required pointer %s is null" % field)


def test_what_the_kernel_does_not_read_is_not_required():
    """the vector observation, the dynamics and the optional cull table may be null: the first complaint is still a limit's"""
    rc, msg = _call(null=("obs", "dyn", "quad_ball", "beam_cs", "need_reset"), resolution=129)
    assert rc == abi.MD_EINVAL and "MD_TD_MAX_RES=128" in msg, msg


def test_limits_are_named():
    rc, msg = _call(resolution=abi.MD_TD_MAX_RES + 1)
    assert rc == abi.MD_EINVAL and msg == "md_topdown: resolution=129 is beyond MD_TD_MAX_RES=128"
    rc, msg = _call(frame_stack=14, frame_skip=5)       # 13 * 5 + 1 = 66
    assert rc == abi.MD_EINVAL and "MD_TD_MAX_RING=64" in msg and "=66" in msg, msg
    rc, msg = _call(post_stack=65, frame_skip=1)
    assert rc == abi.MD_EINVAL and "MD_TD_MAX_RING=64" in msg and "=65" in msg, msg
    rc, msg = _call(frame_stack=2, frame_skip=2 ** 30)  # no overflow on the way to the limit
    assert rc == abi.MD_EINVAL and "MD_TD_MAX_RING=64" in msg, msg
    for bad in (dict(frame_stack=0), dict(post_stack=0), dict(frame_skip=0), dict(resolution=0), dict(distance=0.0)):
        rc, msg = _call(**bad)
        assert rc == abi.MD_EINVAL and msg.startswith("md_topdown: frame_stack="), msg


def test_tables_read_16_bytes_at_a_time_must_be_aligned():
    lib = _lib.load()
    for field in ("quads", "quad_ball"):
        w, s, k, td = _struct(abi.MdWorld), _struct(abi.MdState), abi.MdConfig(), _struct(abi.MdTopDown)
        for name, v in CONFIG.items():
            setattr(k, name, v)
        for name, v in TOPDOWN.items():
            setattr(td, name, v)
        w.n_envs, w.n_maps = 8, 1
        setattr(w, field, DUMMY + 8)
        assert lib.md_topdown(C.byref(w), C.byref(s), C.byref(k), C.byref(td), None) == abi.MD_EINVAL
        assert lib.md_last_error().decode() == "md_topdown: MdWorld.%s must be 16-byte aligned" % field


def test_multi_agent_and_scenario_mode_are_refused():
    rc, msg = _call(cfg=dict(agents_per_env=2))
    assert rc == abi.MD_EINVAL and msg.startswith("md_topdown: agents_per_env=2"), msg
    rc, msg = _call(cfg=dict(traffic_mode=4))
    assert rc == abi.MD_EINVAL and msg.startswith("md_topdown: not in scenario mode"), msg
