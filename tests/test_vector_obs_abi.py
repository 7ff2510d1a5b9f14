"""md_vector_obs's place in the C-ABI (include/md_vector_obs.h) and its argument check, in the order the header states: the four
struct pointers, both struct_size fields, the sizes, every parameter range, the required MdWorld / MdState arrays, then the outputs,
the ring and the cursor by name.  Every call here is refused before any launch; those tests are skipped where a GPU is visible all the
same, since a call that slipped through the checks would launch on dummy pointers."""
import ctypes as C
import os
import re

import pytest

from metadrive_ped_amd import _lib, abi
from metadrive_ped_amd.config import VECTOR_OBS_DEFAULT_CONFIG

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_BUF = C.create_string_buffer(4096)
DUMMY = (C.addressof(_BUF) + 15) & ~15
CONFIG = dict(struct_size=C.sizeof(abi.MdConfig), n_envs=8, agents_per_env=1, cap=32, n_beams=0, obs_dim=19, substeps=5, dt=0.02)
REQUIRED_STATE = ["dyn", "nav", "route_roads", "final_lane"]      # and shape, which the common size check names itself
REQUIRED_WORLD = ["env_map", "lane_off", "lanes", "road_off", "roads"]
ALWAYS_OUT = ["agents", "agents_mask", "agents_meta", "ego", "ego_mask", "ring_pose", "ring_flags", "cursor"]
ROUTE_OUT = ["route", "route_mask"]
LANE_OUT = ["lanes", "lanes_meta", "lanes_mask"]


@pytest.fixture
def no_gpu():
    import torch
    if torch.cuda.device_count() > 0:
        pytest.skip("a GPU is visible: the calls carry dummy pointers")


def _call(null=(), cfg=None, **fields):
    """md_vector_obs with dummy pointers everywhere; `null`: the arguments ("w", "s", "c", "vo"), the MdWorld / MdState arrays ("w->x",
    "s->x") and the MdVectorObs pointers ("vo->x") left null"""
    lib = _lib.load()
    k, s, w = abi.MdConfig(), abi.MdState(), abi.MdWorld()
    for name, v in dict(CONFIG, **(cfg or {})).items():
        setattr(k, name, v)
    w.n_maps, w.n_envs, w.max_lanes, w.max_roads = 1, k.n_envs, 40, 10
    for f in abi.STATE_FIELDS:
        setattr(s, f, None if "s->" + f in null else DUMMY)
    for f in abi.WORLD_FIELDS:
        setattr(w, f, None if "w->" + f in null else DUMMY)
    ptrs = dict(out_stride=4096, hist_stride=4096)
    ptrs.update({f: DUMMY for f in abi.VECTOR_OBS_OUTPUTS + abi.VECTOR_OBS_HISTORY if "vo->" + f not in null})
    vo = abi.make_md_vector_obs(VECTOR_OBS_DEFAULT_CONFIG, ptrs)
    for name, v in fields.items():
        setattr(vo, name, v)
    args = [None if n in null else C.byref(x) for n, x in (("w", w), ("s", s), ("c", k), ("vo", vo))]
    rc = lib.md_vector_obs(*args, None)
    return rc, lib.md_last_error().decode()


def test_entry_point_has_a_header_and_a_table_of_its_own():
    assert list(abi.VECTOR_OBS_ENTRY_POINTS) == ["md_vector_obs"]
    for table in (abi.ENTRY_POINTS, abi.EXPERT_ENTRY_POINTS, abi.AI_PROTECT_ENTRY_POINTS, abi.EXPERT_SENSE_ENTRY_POINTS,
                  abi.CURRICULUM_ENTRY_POINTS, abi.TOPDOWN_ENTRY_POINTS, abi.RENDER_ENTRY_POINTS, abi.BRANCH_ENTRY_POINTS,
                  abi.PED_ENTRY_POINTS, abi.OPTIONAL_ENTRY_POINTS):
        assert "md_vector_obs" not in table
    assert abi.MD_ABI_VERSION == 12
    inc = os.path.join(ROOT, "include")
    declared = [f for f in sorted(os.listdir(inc)) if re.search(r"^int md_vector_obs\(", open(os.path.join(inc, f)).read(), re.M)]
    assert declared == ["md_vector_obs.h"]
    assert len(abi.VECTOR_OBS_ENTRY_POINTS["md_vector_obs"][1]) == 5
    assert hasattr(_lib.load(), "md_vector_obs")


def test_the_binding_has_the_header_s_size():
    import vector_obs_host
    n = C.sizeof(abi.MdVectorObs)
    assert n == vector_obs_host.lib().hx_sizeof_vector_obs() and n % 8 == 0
    assert abi.MdVectorObs._fields_[0][0] == "struct_size" and abi.MdVectorObs.struct_size.offset == 0
    assert abi.make_md_vector_obs(VECTOR_OBS_DEFAULT_CONFIG, dict(out_stride=16, hist_stride=16)).reserved == 0
    # ... and the library's: it accepts exactly this struct_size (test_struct_sizes)


def test_the_abi_structs_are_as_they_were():
    sizes = (C.c_int32 * 11)()
    assert _lib.load().md_abi(sizes, 11) == 12 and list(sizes) == abi.STRUCT_SIZES


@pytest.mark.parametrize("name", ["w", "s", "c", "vo"])
def test_required_arguments_by_name(no_gpu, name):
    assert _call(null=(name, )) == (abi.MD_EINVAL, "required pointer %s is null" % name)


def test_struct_sizes(no_gpu):
    rc, msg = _call(cfg=dict(struct_size=4))
    assert rc == abi.MD_EABI and msg == "MdConfig.struct_size=4, library expects %d" % C.sizeof(abi.MdConfig)
    n = C.sizeof(abi.MdVectorObs)
    assert _call(struct_size=n - 8) == (abi.MD_EABI, "MdVectorObs.struct_size=%d, library expects %d" % (n - 8, n))
    assert _call(struct_size=n + 8) == (abi.MD_EABI, "MdVectorObs.struct_size=%d, library expects %d" % (n + 8, n))
    # before the sizes and the ranges
    assert _call(struct_size=0, cfg=dict(cap=0), num_agents=0)[0] == abi.MD_EABI


def test_sizes_come_before_the_ranges(no_gpu):
    for cfg in (dict(n_envs=0), dict(cap=0), dict(cap=129), dict(agents_per_env=0)):
        rc, msg = _call(cfg=cfg, num_agents=0)
        assert rc == abi.MD_EINVAL and msg.startswith("bad sizes: "), (cfg, msg)


@pytest.mark.parametrize("field,lo,hi,limit", [("num_agents", 1, 16, "MD_VO_MAX_AGENTS"), ("history", 1, 8, "MD_VO_MAX_HISTORY"),
                                               ("route_points", 0, 32, "MD_VO_MAX_ROUTE_POINTS"), ("num_lanes", 0, 16, "MD_VO_MAX_LANES"),
                                               ("lane_points", 2, 16, "MD_VO_MAX_LANE_POINTS")])
def test_every_count_s_range_is_named(no_gpu, field, lo, hi, limit):
    for bad in (lo - 1, hi + 1):
        assert _call(**{field: bad}) == (abi.MD_EINVAL, "md_vector_obs: %s=%d must lie in [%d, %s=%d]" % (field, bad, lo, limit, hi))
    # ... before any array is asked for
    assert _call(null=("s->nav", "vo->agents"), **{field: hi + 1})[1].startswith("md_vector_obs: %s=" % field)


@pytest.mark.parametrize("field", ["radius", "max_jump", "route_spacing"])
def test_every_length_must_be_positive(no_gpu, field):
    for bad in (0.0, -1.0, float("nan")):
        rc, msg = _call(**{field: bad})
        assert rc == abi.MD_EINVAL and msg.startswith("md_vector_obs: %s=" % field) and "must be positive" in msg, msg


def test_strides(no_gpu):
    for bad in (dict(out_stride=0), dict(out_stride=24), dict(hist_stride=-16), dict(hist_stride=8)):
        rc, msg = _call(**bad)
        assert rc == abi.MD_EINVAL and "must be positive multiples of 16" in msg, (bad, msg)


def test_scenario_mode_is_refused(no_gpu):
    rc, msg = _call(cfg=dict(traffic_mode=4))
    assert rc == abi.MD_EINVAL and msg.startswith("md_vector_obs: not in scenario mode")


@pytest.mark.parametrize("name", ["s->" + f for f in REQUIRED_STATE] + ["w->" + f for f in REQUIRED_WORLD])
def test_required_arrays_by_name(no_gpu, name):
    assert _call(null=(name, )) == (abi.MD_EINVAL, "required pointer %s is null" % name)
    # the arrays come before the outputs
    assert _call(null=(name, "vo->agents"))[1] == "required pointer %s is null" % name


def test_the_shape_array_is_required(no_gpu):
    assert _call(null=("s->shape", )) == (abi.MD_EINVAL, "MdState.shape is null")


def test_the_env_clock_is_required_in_a_multi_agent_batch_only(no_gpu):
    assert _call(null=("s->env_steps", ), cfg=dict(is_multi_agent=1)) == (abi.MD_EINVAL, "required pointer s->env_steps is null")
    assert _call(null=("s->env_steps", "vo->cursor"))[1] == "required pointer vo->cursor is null"


def test_only_those_are_required(no_gpu):
    rest = tuple("s->" + f for f in abi.STATE_FIELDS if f not in REQUIRED_STATE + ["shape"]) + \
        tuple("w->" + f for f in abi.WORLD_FIELDS if f not in REQUIRED_WORLD)
    assert _call(null=rest + ("vo->cursor", ))[1] == "required pointer vo->cursor is null"


@pytest.mark.parametrize("name", ALWAYS_OUT + ROUTE_OUT + LANE_OUT)
def test_outputs_ring_and_cursor_by_name(no_gpu, name):
    assert _call(null=("vo->" + name, )) == (abi.MD_EINVAL, "required pointer vo->%s is null" % name)


def test_a_block_s_outputs_are_not_required_at_count_zero(no_gpu):
    # with the route and the lane blocks off and their outputs null, the first complaint is the next output's
    off = tuple("vo->" + f for f in ROUTE_OUT + LANE_OUT)
    assert _call(null=off + ("vo->ring_pose", ), route_points=0, num_lanes=0)[1] == "required pointer vo->ring_pose is null"
    assert _call(null=off, route_points=0)[1] == "required pointer vo->lanes is null"
    assert _call(null=off, num_lanes=0)[1] == "required pointer vo->route is null"
