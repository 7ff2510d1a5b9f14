"""md_render's argument check (include/md_render.h): check_common first, MdRender.struct_size, the required pointers and the fields
the kernels read by name, then every limit and refusal with its message.  Every call here is refused before any launch (MD_EINVAL /
MD_EABI and a message that names what is wrong), so dummy pointers never reach a device."""
import ctypes as C

import pytest

from metadrive_ped_amd import _lib, abi

_BUF = C.create_string_buffer(4096)
DUMMY = (C.addressof(_BUF) + 15) & ~15
CONFIG = dict(struct_size=C.sizeof(abi.MdConfig), n_envs=8, agents_per_env=1, cap=32, n_beams=0, obs_dim=19)
RENDER = dict(struct_size=C.sizeof(abi.MdRender), width=512, height=512, scaling=5.0, num_stack=15, history_smooth=0, track_agent=0,
              heading_up=0, draw_contour=1, fixed_camera=0, n_render=1)


def _struct(cls, null=()):
    s = cls()
    for f, t in cls._fields_:
        if t is abi.P:
            setattr(s, f, None if f in null else DUMMY)
    return s


def _call(null=(), r_null=(), world=True, with_r=True, cfg=None, world_fields=None, **r_fields):
    lib = _lib.load()
    w, s, k, r = _struct(abi.MdWorld, null), _struct(abi.MdState, null), abi.MdConfig(), _struct(abi.MdRender, r_null)
    for name, v in dict(CONFIG, **(cfg or {})).items():
        setattr(k, name, v)
    for name, v in dict(RENDER, **r_fields).items():
        setattr(r, name, v)
    w.n_envs, w.n_maps = 8, 1
    for name, v in (world_fields or {}).items():
        setattr(w, name, v)
    rc = lib.md_render(C.byref(w) if world else None, C.byref(s), C.byref(k), C.byref(r) if with_r else None, None)
    return rc, lib.md_last_error().decode()


def test_entry_point_has_a_table_of_its_own():
    assert list(abi.RENDER_ENTRY_POINTS) == ["md_render"]
    for table in (abi.ENTRY_POINTS, abi.EXPERT_ENTRY_POINTS, abi.AI_PROTECT_ENTRY_POINTS, abi.EXPERT_SENSE_ENTRY_POINTS,
                  abi.CURRICULUM_ENTRY_POINTS, abi.TOPDOWN_ENTRY_POINTS):
        assert "md_render" not in table
    assert abi.MD_ABI_VERSION == 12
    assert (abi.MD_RD_MAX_SIZE, abi.MD_RD_MAX_STACK, abi.MD_RD_TILE) == (1024, 32, 64)


def test_check_common_comes_first():
    assert _call(world=False, with_r=False) == (abi.MD_EINVAL, "null MdWorld/MdState/MdConfig pointer")
    rc, msg = _call(cfg=dict(struct_size=4), with_r=False)
    assert rc == abi.MD_EABI and "MdConfig.struct_size" in msg
    rc, msg = _call(cfg=dict(n_envs=0), with_r=False)
    assert rc == abi.MD_EINVAL and msg.startswith("bad sizes"), msg
    assert _call(null=("shape", ), with_r=False) == (abi.MD_EINVAL, "MdState.shape is null")


def test_the_argument_block_and_its_size():
    assert _call(with_r=False) == (abi.MD_EINVAL, "required pointer r is null")
    rc, msg = _call(struct_size=C.sizeof(abi.MdRender) - 8, r_null=("out", ))
    assert rc == abi.MD_EABI and msg == "MdRender.struct_size=%d, library expects %d" % (C.sizeof(abi.MdRender) - 8, C.sizeof(abi.MdRender))


@pytest.mark.parametrize("name", ["env_ids", "out", "ring", "cursor"])
def test_required_arguments_by_name(name):
    assert _call(r_null=(name, ), width=0) == (abi.MD_EINVAL, "required pointer r->%s is null" % name)


@pytest.mark.parametrize("field", ["s->nav", "w->env_map", "w->quad_off", "w->quads", "w->quad_kind"])
def test_required_fields_by_name(field):
    assert _call(null=(field[3:], ), width=0) == (abi.MD_EINVAL, "required pointer %s is null" % field)


def test_the_multi_agent_clock_is_required_in_multi_agent_batches_only():
    rc, msg = _call(null=("env_steps", ), width=0)
    assert rc == abi.MD_EINVAL and msg.startswith("md_render: width=0"), msg
    assert _call(null=("env_steps", ), cfg=dict(is_multi_agent=1, agents_per_env=4)) == (abi.MD_EINVAL, "required pointer s->env_steps is null")


def test_what_the_kernels_do_not_read_is_not_required():
    """no lane table, no route, no observation: the first complaint is still a limit's"""
    rc, msg = _call(null=("obs", "dyn", "lanes", "lane_off", "roads", "road_off", "route_roads", "quad_ball", "beam_cs", "need_reset"), num_stack=33)
    assert rc == abi.MD_EINVAL and "MD_RD_MAX_STACK=32" in msg, msg


def test_limits_and_refusals_are_named():
    for bad in (0, -3, 65536):
        assert _call(n_render=bad) == (abi.MD_EINVAL, "md_render: n_render=%d must lie in [1, 65535]" % bad)
    for bad in (dict(width=0), dict(height=0), dict(width=1025), dict(height=1025)):
        size = dict(dict(width=512, height=512), **bad)
        assert _call(**bad) == (abi.MD_EINVAL, "md_render: width=%d height=%d must lie in [1, MD_RD_MAX_SIZE=1024]" % (size["width"], size["height"]))
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        rc, msg = _call(scaling=bad)
        assert rc == abi.MD_EINVAL and msg.startswith("md_render: scaling=") and msg.endswith("must be positive and finite"), msg
    for bad in (0, 33):
        assert _call(num_stack=bad) == (abi.MD_EINVAL, "md_render: num_stack=%d must lie in [1, MD_RD_MAX_STACK=32]" % bad)
    assert _call(history_smooth=-1) == (abi.MD_EINVAL, "md_render: history_smooth=-1 must not be negative")
    assert _call(track_agent=1) == (abi.MD_EINVAL, "md_render: track_agent=1 is no agent slot (agents_per_env=1)")
    assert _call(track_agent=-1) == (abi.MD_EINVAL, "md_render: track_agent=-1 is no agent slot (agents_per_env=1)")
    assert _call(track_agent=4, cfg=dict(agents_per_env=4)) == (abi.MD_EINVAL, "md_render: track_agent=4 is no agent slot (agents_per_env=4)")
    assert _call(world_fields=dict(n_maps=0)) == (abi.MD_EINVAL, "md_render: MdWorld.n_maps=0")


@pytest.mark.parametrize("field", ["quads", "quad_ball"])
def test_tables_read_16_bytes_at_a_time_must_be_aligned(field):
    assert _call(world_fields={field: DUMMY + 8}) == (abi.MD_EINVAL, "md_render: MdWorld.%s must be 16-byte aligned" % field)
