"""md_scenario_vector_obs's place in the C-ABI (include/md_scenario_vector_obs.h) and its argument check, in the order the header
states: the four struct pointers, the struct_size fields, the sizes, every count and length, the strides, the mode, the required
MdWorld / MdState arrays, then the outputs, the ring, the cursor and the piece table by name, alignment, max_pieces.  Every call here
is refused before any launch; those tests are skipped where a GPU is visible all the same, since a call that slipped through the
checks would launch on dummy pointers."""
import ctypes as C
import os
import re

import pytest

from metadrive_ped_amd import _lib, abi
from metadrive_ped_amd.config import SCENARIO_VECTOR_OBS_DEFAULT_CONFIG, SCENARIO_VECTOR_OBS_RANGES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_BUF = C.create_string_buffer(4096)
DUMMY = (C.addressof(_BUF) + 15) & ~15
CONFIG = dict(struct_size=C.sizeof(abi.MdConfig), n_envs=8, agents_per_env=1, cap=32, n_beams=0, obs_dim=19, substeps=5, dt=0.02,
              traffic_mode=4)
REQUIRED_STATE = ["dyn", "nav"]      # and shape, which the common size check names itself
REQUIRED_WORLD = ["poly_off", "segs"]
SHARED_OUT = ["agents", "agents_mask", "agents_meta", "ego", "ego_mask", "ring_pose", "ring_flags", "cursor"]      # of the embedded vo
ROUTE_OUT = ["route", "route_mask"]
MAP_OUT = ["map", "map_mask", "map_meta"]
TABLES = ["map_off", "map_xy", "map_info", "map_ball"]
VO_FIELDS = [f for f, _ in abi.MdVectorObs._fields_]


@pytest.fixture
def no_gpu():
    import torch
    if torch.cuda.device_count() > 0:
        pytest.skip("a GPU is visible: the calls carry dummy pointers")


def _name(f):
    return ("sv->vo." if f in SHARED_OUT + ROUTE_OUT else "sv->") + f


def _call(null=(), cfg=None, **fields):
    """md_scenario_vector_obs with dummy pointers everywhere; `null`: the arguments ("w", "s", "c", "sv"), the MdWorld / MdState arrays
    ("w->x", "s->x") and the MdScenarioVectorObs pointers ("sv->x", "sv->vo.x") left null; `fields`: set on the struct, or on its
    embedded MdVectorObs where the name is one of that struct's alone"""
    lib = _lib.load()
    k, s, w = abi.MdConfig(), abi.MdState(), abi.MdWorld()
    for name, v in dict(CONFIG, **(cfg or {})).items():
        setattr(k, name, v)
    w.n_maps, w.n_envs = 1, k.n_envs
    for f in abi.STATE_FIELDS:
        setattr(s, f, None if "s->" + f in null else DUMMY)
    for f in abi.WORLD_FIELDS:
        setattr(w, f, None if "w->" + f in null else DUMMY)
    ptrs = dict(out_stride=4096, hist_stride=4096, max_pieces=100)
    ptrs.update({f: DUMMY for f in SHARED_OUT + ROUTE_OUT + MAP_OUT + TABLES if _name(f) not in null})
    sv = abi.make_md_scenario_vector_obs(SCENARIO_VECTOR_OBS_DEFAULT_CONFIG, ptrs)
    for name, v in fields.items():
        if name.startswith("vo_"):
            setattr(sv.vo, name[3:], v)
        elif name in VO_FIELDS and name != "struct_size" and name != "reserved":
            setattr(sv.vo, name, v)
        else:
            setattr(sv, name, v)
    args = [None if n in null else C.byref(x) for n, x in (("w", w), ("s", s), ("c", k), ("sv", sv))]
    rc = lib.md_scenario_vector_obs(*args, None)
    return rc, lib.md_last_error().decode()


def test_entry_point_has_a_header_and_a_table_of_its_own():
    assert list(abi.SCENARIO_VECTOR_OBS_ENTRY_POINTS) == ["md_scenario_vector_obs"]
    for table in (abi.ENTRY_POINTS, abi.EXPERT_ENTRY_POINTS, abi.AI_PROTECT_ENTRY_POINTS, abi.EXPERT_SENSE_ENTRY_POINTS,
                  abi.CURRICULUM_ENTRY_POINTS, abi.TOPDOWN_ENTRY_POINTS, abi.RENDER_ENTRY_POINTS, abi.BRANCH_ENTRY_POINTS,
                  abi.PED_ENTRY_POINTS, abi.VECTOR_OBS_ENTRY_POINTS, abi.CONTACT_RESPONSE_ENTRY_POINTS, abi.OPTIONAL_ENTRY_POINTS):
        assert "md_scenario_vector_obs" not in table
    assert abi.MD_ABI_VERSION == 12
    inc = os.path.join(ROOT, "include")
    declared = [f for f in sorted(os.listdir(inc)) if re.search(r"^int md_scenario_vector_obs\(", open(os.path.join(inc, f)).read(), re.M)]
    assert declared == ["md_scenario_vector_obs.h"]
    assert len(abi.SCENARIO_VECTOR_OBS_ENTRY_POINTS["md_scenario_vector_obs"][1]) == 5
    assert hasattr(_lib.load(), "md_scenario_vector_obs")
    text = open(os.path.join(inc, "md_scenario_vector_obs.h")).read()
    assert '#include "md_vector_obs.h"' in text and '#include "md_scenario.h"' in text


def test_the_binding_has_the_header_s_size_and_ceilings():
    import scenario_vector_obs_host as sh
    lib = sh.lib()
    n = C.sizeof(abi.MdScenarioVectorObs)
    assert n == lib.hx_sizeof_scenario_vector_obs() and n % 8 == 0
    assert abi.MdScenarioVectorObs.vo.offset == lib.hx_offsetof_svo_vo()
    assert abi.MdScenarioVectorObs._fields_[0][0] == "struct_size" and abi.MdScenarioVectorObs.struct_size.offset == 0
    limits = [lib.hx_svo_limit(i) for i in range(6)]
    assert limits == [abi.MD_VO_MAX_AGENTS, abi.MD_VO_MAX_HISTORY, abi.MD_VO_MAX_ROUTE_POINTS, abi.MD_SVO_MAX_MAP_PIECES,
                      abi.MD_SVO_MAX_PIECE_POINTS, abi.MD_SVO_MAX_PIECES] == [16, 8, 32, 64, 16, 4096]
    assert [SCENARIO_VECTOR_OBS_RANGES[k][1] for k in ("num_agents", "history", "route_points", "num_pieces", "piece_points")] == limits[:5]
    sv = abi.make_md_scenario_vector_obs(SCENARIO_VECTOR_OBS_DEFAULT_CONFIG, dict(out_stride=16, hist_stride=16))
    assert sv.reserved == 0 and sv.vo.num_lanes == 0 and sv.vo.struct_size == C.sizeof(abi.MdVectorObs) and sv.max_pieces == 0


def test_the_abi_structs_are_as_they_were():
    sizes = (C.c_int32 * 11)()
    assert _lib.load().md_abi(sizes, 11) == 12 and list(sizes) == abi.STRUCT_SIZES


@pytest.mark.parametrize("name", ["w", "s", "c", "sv"])
def test_required_arguments_by_name(no_gpu, name):
    assert _call(null=(name, )) == (abi.MD_EINVAL, "required pointer %s is null" % name)


def test_struct_sizes(no_gpu):
    rc, msg = _call(cfg=dict(struct_size=4))
    assert rc == abi.MD_EABI and msg == "MdConfig.struct_size=4, library expects %d" % C.sizeof(abi.MdConfig)
    n = C.sizeof(abi.MdScenarioVectorObs)
    assert _call(struct_size=n - 8) == (abi.MD_EABI, "MdScenarioVectorObs.struct_size=%d, library expects %d" % (n - 8, n))
    assert _call(struct_size=n + 8) == (abi.MD_EABI, "MdScenarioVectorObs.struct_size=%d, library expects %d" % (n + 8, n))
    m = C.sizeof(abi.MdVectorObs)
    assert _call(vo_struct_size=m - 8) == (abi.MD_EABI, "MdScenarioVectorObs.vo.struct_size=%d, library expects %d" % (m - 8, m))
    # before the sizes and the ranges
    assert _call(struct_size=0, cfg=dict(cap=0), num_agents=0)[0] == abi.MD_EABI


def test_sizes_come_before_the_ranges(no_gpu):
    for cfg in (dict(n_envs=0), dict(cap=0), dict(cap=129), dict(agents_per_env=0)):
        rc, msg = _call(cfg=cfg, num_agents=0)
        assert rc == abi.MD_EINVAL and msg.startswith("bad sizes: "), (cfg, msg)


@pytest.mark.parametrize("field,lo,hi,limit", [("num_agents", 1, 16, "MD_VO_MAX_AGENTS"), ("history", 1, 8, "MD_VO_MAX_HISTORY"),
                                               ("route_points", 0, 32, "MD_VO_MAX_ROUTE_POINTS"),
                                               ("num_pieces", 0, 64, "MD_SVO_MAX_MAP_PIECES"),
                                               ("piece_points", 2, 16, "MD_SVO_MAX_PIECE_POINTS")])
def test_every_count_s_range_is_named(no_gpu, field, lo, hi, limit):
    for bad in (lo - 1, hi + 1):
        assert _call(**{field: bad}) == (abi.MD_EINVAL, "md_scenario_vector_obs: %s=%d must lie in [%d, %s=%d]" % (field, bad, lo, limit, hi))
    # ... before any array is asked for, and before the mode
    assert _call(null=("s->nav", "sv->vo.agents"), cfg=dict(traffic_mode=0), **{field: hi + 1})[1].startswith(
        "md_scenario_vector_obs: %s=" % field)


def test_the_embedded_struct_has_no_lanes(no_gpu):
    rc, msg = _call(num_lanes=1)
    assert rc == abi.MD_EINVAL and msg.startswith("md_scenario_vector_obs: vo.num_lanes=1 must be 0")


@pytest.mark.parametrize("field", ["radius", "max_jump", "route_spacing", "map_radius"])
def test_every_length_must_be_positive(no_gpu, field):
    for bad in (0.0, -1.0, float("nan")):
        rc, msg = _call(**{field: bad})
        assert rc == abi.MD_EINVAL and msg.startswith("md_scenario_vector_obs: %s=" % field) and "must be positive" in msg, msg


def test_strides(no_gpu):
    for bad in (dict(out_stride=0), dict(out_stride=24), dict(hist_stride=-16), dict(hist_stride=8)):
        rc, msg = _call(**bad)
        assert rc == abi.MD_EINVAL and "must be positive multiples of 16" in msg, (bad, msg)


@pytest.mark.parametrize("mode", [0, 1, 2, 3])
def test_only_in_scenario_mode(no_gpu, mode):
    rc, msg = _call(cfg=dict(traffic_mode=mode))
    assert rc == abi.MD_EINVAL and msg.startswith("md_scenario_vector_obs: only in scenario mode"), msg
    # the mode comes before the arrays
    assert _call(null=("s->nav", ), cfg=dict(traffic_mode=mode))[1].startswith("md_scenario_vector_obs: only in scenario mode")


def test_md_vector_obs_keeps_refusing_scenario_mode(no_gpu):
    lib = _lib.load()
    k, s, w = abi.MdConfig(), abi.MdState(), abi.MdWorld()
    for name, v in CONFIG.items():
        setattr(k, name, v)
    w.n_maps, w.n_envs, w.max_lanes, w.max_roads = 1, k.n_envs, 40, 10
    for f in abi.STATE_FIELDS:
        setattr(s, f, DUMMY)
    for f in abi.WORLD_FIELDS:
        setattr(w, f, DUMMY)
    from metadrive_ped_amd.config import VECTOR_OBS_DEFAULT_CONFIG
    ptrs = dict(out_stride=4096, hist_stride=4096, **{f: DUMMY for f in abi.VECTOR_OBS_OUTPUTS + abi.VECTOR_OBS_HISTORY})
    vo = abi.make_md_vector_obs(VECTOR_OBS_DEFAULT_CONFIG, ptrs)
    assert lib.md_vector_obs(C.byref(w), C.byref(s), C.byref(k), C.byref(vo), None) == abi.MD_EINVAL
    assert lib.md_last_error().decode().startswith("md_vector_obs: not in scenario mode")


def test_one_observer_per_env(no_gpu):
    assert _call(cfg=dict(agents_per_env=2))[1].startswith("md_scenario_vector_obs: agents_per_env=2")
    assert _call(cfg=dict(is_multi_agent=1))[1].startswith("md_scenario_vector_obs: agents_per_env=1 is_multi_agent=1")


@pytest.mark.parametrize("name", ["s->" + f for f in REQUIRED_STATE] + ["w->" + f for f in REQUIRED_WORLD])
def test_required_arrays_by_name(no_gpu, name):
    assert _call(null=(name, )) == (abi.MD_EINVAL, "required pointer %s is null" % name)
    # the arrays come before the outputs
    assert _call(null=(name, "sv->vo.agents"))[1] == "required pointer %s is null" % name


def test_the_shape_array_is_required(no_gpu):
    assert _call(null=("s->shape", )) == (abi.MD_EINVAL, "MdState.shape is null")


def test_only_those_are_required(no_gpu):
    rest = tuple("s->" + f for f in abi.STATE_FIELDS if f not in REQUIRED_STATE + ["shape"]) + \
        tuple("w->" + f for f in abi.WORLD_FIELDS if f not in REQUIRED_WORLD)
    assert _call(null=rest + ("sv->vo.cursor", ))[1] == "required pointer vo->cursor is null"


@pytest.mark.parametrize("name", SHARED_OUT + ROUTE_OUT + MAP_OUT + TABLES)
def test_outputs_ring_cursor_and_tables_by_name(no_gpu, name):
    spelled = ("vo->" if name in SHARED_OUT + ROUTE_OUT else "sv->") + name
    assert _call(null=(_name(name), )) == (abi.MD_EINVAL, "required pointer %s is null" % spelled)


def test_a_block_s_outputs_are_not_required_at_count_zero(no_gpu):
    off = tuple(_name(f) for f in ROUTE_OUT + MAP_OUT + TABLES)
    assert _call(null=off + ("sv->vo.ring_pose", ), route_points=0, num_pieces=0)[1] == "required pointer vo->ring_pose is null"
    assert _call(null=off, route_points=0)[1] == "required pointer sv->map is null"
    assert _call(null=off, num_pieces=0)[1] == "required pointer vo->route is null"
    # the tables come after the ring
    assert _call(null=("sv->map_off", "sv->vo.cursor"))[1] == "required pointer vo->cursor is null"


def test_alignment(no_gpu):
    assert "must be 4-byte aligned" in _call(map=DUMMY + 2)[1]
    assert "must be 4-byte aligned" in _call(agents=DUMMY + 1)[1]
    assert "map_ball must be 16-byte aligned" in _call(map_ball=DUMMY + 4)[1]


def test_max_pieces_and_its_bound(no_gpu):
    for bad in (-1, 4097):
        assert _call(max_pieces=bad) == (abi.MD_EINVAL, "md_scenario_vector_obs: max_pieces=%d must lie in [0, MD_SVO_MAX_PIECES=4096]" % bad)
    # the largest image, 2 x 4 x 4096 + the two short lists, is inside the LDS of a workgroup: the LDS bound never bites below the ceiling
    assert 8 * 4096 + 4 * 16 + 4 * 64 < 64 * 1024
