"""md_traffic_lights's place in the C-ABI (include/md_traffic_lights.h) and its argument check, in the order the header states: the
four struct pointers, the struct_size fields, the sizes, the two counts, the radius, the stride, the mode, the required MdState arrays,
then the tables and the outputs by name, alignment.  Every call here is refused before any launch; those tests are skipped where a GPU
is visible all the same, since a call that slipped through the checks would launch on dummy pointers."""
import ctypes as C
import os
import re

import pytest

from metadrive_ped_amd import _lib, abi
from metadrive_ped_amd.config import TRAFFIC_LIGHTS_DEFAULT_CONFIG, TRAFFIC_LIGHTS_RANGES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_BUF = C.create_string_buffer(4096)
DUMMY = (C.addressof(_BUF) + 15) & ~15
CONFIG = dict(struct_size=C.sizeof(abi.MdConfig), n_envs=8, agents_per_env=1, cap=32, n_beams=0, obs_dim=19, substeps=5, dt=0.02,
              traffic_mode=4)
TABLES = ["tl_off", "tl_box", "tl_info", "tl_status"]
LIGHTS_OUT = ["lights", "lights_mask", "lights_index"]


@pytest.fixture
def no_gpu():
    import torch
    if torch.cuda.device_count() > 0:
        pytest.skip("a GPU is visible: the calls carry dummy pointers")


def _call(null=(), cfg=None, **fields):
    """md_traffic_lights with dummy pointers everywhere; `null`: the arguments ("w", "s", "c", "tl"), the MdWorld / MdState arrays
    ("w->x", "s->x") and the MdTrafficLights pointers ("tl->x") left null; `fields`: set on the struct"""
    lib = _lib.load()
    k, s, w = abi.MdConfig(), abi.MdState(), abi.MdWorld()
    for name, v in dict(CONFIG, **(cfg or {})).items():
        setattr(k, name, v)
    w.n_maps, w.n_envs = 1, k.n_envs
    for f in abi.STATE_FIELDS:
        setattr(s, f, None if "s->" + f in null else DUMMY)
    for f in abi.WORLD_FIELDS:
        setattr(w, f, None if "w->" + f in null else DUMMY)
    ptrs = dict(out_stride=256, max_scene_lights=100)
    ptrs.update({f: DUMMY for f in TABLES + ["agent_light"] + LIGHTS_OUT if "tl->" + f not in null})
    tl = abi.make_md_traffic_lights(TRAFFIC_LIGHTS_DEFAULT_CONFIG, ptrs)
    for name, v in fields.items():
        setattr(tl, name, v)
    args = [None if n in null else C.byref(x) for n, x in (("w", w), ("s", s), ("c", k), ("tl", tl))]
    rc = lib.md_traffic_lights(*args, None)
    return rc, lib.md_last_error().decode()


def test_entry_point_has_a_header_and_a_table_of_its_own():
    assert list(abi.TRAFFIC_LIGHTS_ENTRY_POINTS) == ["md_traffic_lights"]
    for table in (abi.ENTRY_POINTS, abi.EXPERT_ENTRY_POINTS, abi.AI_PROTECT_ENTRY_POINTS, abi.EXPERT_SENSE_ENTRY_POINTS,
                  abi.CURRICULUM_ENTRY_POINTS, abi.TOPDOWN_ENTRY_POINTS, abi.RENDER_ENTRY_POINTS, abi.BRANCH_ENTRY_POINTS,
                  abi.PED_ENTRY_POINTS, abi.VECTOR_OBS_ENTRY_POINTS, abi.SCENARIO_VECTOR_OBS_ENTRY_POINTS, abi.CONTACT_RESPONSE_ENTRY_POINTS,
                  abi.OPTIONAL_ENTRY_POINTS):
        assert "md_traffic_lights" not in table
    assert abi.MD_ABI_VERSION == 12, "no existing struct changed: the ABI version stays"
    inc = os.path.join(ROOT, "include")
    declared = [f for f in sorted(os.listdir(inc)) if re.search(r"^int md_traffic_lights\(", open(os.path.join(inc, f)).read(), re.M)]
    assert declared == ["md_traffic_lights.h"]
    assert len(abi.TRAFFIC_LIGHTS_ENTRY_POINTS["md_traffic_lights"][1]) == 5
    assert hasattr(_lib.load(), "md_traffic_lights")


def test_the_binding_has_the_header_s_size_and_ceilings():
    import traffic_lights_host as th
    lib = th.lib()
    n = C.sizeof(abi.MdTrafficLights)
    assert n == lib.hx_sizeof_traffic_lights() and n % 8 == 0
    assert abi.MdTrafficLights.tl_off.offset == lib.hx_offsetof_tl_tables()
    assert abi.MdTrafficLights._fields_[0][0] == "struct_size" and abi.MdTrafficLights.struct_size.offset == 0
    assert [lib.hx_tl_limit(i) for i in range(2)] == [abi.MD_TL_MAX_LIGHTS, abi.MD_TL_MAX_SCENE_LIGHTS] == [32, 1024]
    assert TRAFFIC_LIGHTS_RANGES["num_lights"] == (0, abi.MD_TL_MAX_LIGHTS)
    tl = abi.make_md_traffic_lights(TRAFFIC_LIGHTS_DEFAULT_CONFIG, dict(out_stride=16))
    assert tl.reserved == 0 and tl.num_lights == 8 and tl.radius == 80.0 and tl.max_scene_lights == 0 and tl.out_stride == 16
    outs, row = abi.traffic_lights_blocks(dict(num_lights=3))
    assert [(k, v[0]) for k, v in outs.items()] == [("agent_light", 0), ("lights", 16), ("lights_mask", 96), ("lights_index", 112)] and row == 128


def test_the_abi_structs_are_as_they_were():
    sizes = (C.c_int32 * 11)()
    assert _lib.load().md_abi(sizes, 11) == 12 and list(sizes) == abi.STRUCT_SIZES


@pytest.mark.parametrize("name", ["w", "s", "c", "tl"])
def test_required_arguments_by_name(no_gpu, name):
    assert _call(null=(name, )) == (abi.MD_EINVAL, "required pointer %s is null" % name)


def test_struct_sizes(no_gpu):
    rc, msg = _call(cfg=dict(struct_size=4))
    assert rc == abi.MD_EABI and msg == "MdConfig.struct_size=4, library expects %d" % C.sizeof(abi.MdConfig)
    n = C.sizeof(abi.MdTrafficLights)
    for bad in (n - 8, n + 8):
        assert _call(struct_size=bad) == (abi.MD_EABI, "MdTrafficLights.struct_size=%d, library expects %d" % (bad, n))
    # before the sizes and the ranges
    assert _call(struct_size=0, cfg=dict(cap=0), num_lights=-1)[0] == abi.MD_EABI


def test_sizes_come_before_the_ranges(no_gpu):
    for cfg in (dict(n_envs=0), dict(cap=0), dict(cap=129), dict(agents_per_env=0)):
        rc, msg = _call(cfg=cfg, num_lights=-1)
        assert rc == abi.MD_EINVAL and msg.startswith("bad sizes: "), (cfg, msg)


@pytest.mark.parametrize("field,hi,limit", [("num_lights", 32, "MD_TL_MAX_LIGHTS"), ("max_scene_lights", 1024, "MD_TL_MAX_SCENE_LIGHTS")])
def test_both_counts_against_their_bounds(no_gpu, field, hi, limit):
    for bad in (-1, hi + 1):
        assert _call(**{field: bad}) == (abi.MD_EINVAL, "md_traffic_lights: %s=%d must lie in [0, %s=%d]" % (field, bad, limit, hi))
    # ... before the radius, the mode and any array
    assert _call(null=("s->nav", "tl->tl_off"), cfg=dict(traffic_mode=0), radius=0.0, **{field: hi + 1})[1].startswith(
        "md_traffic_lights: %s=" % field)


def test_the_radius_must_be_positive(no_gpu):
    for bad in (0.0, -1.0, float("nan"), 1e19):
        rc, msg = _call(radius=bad, out_stride=0)
        assert rc == abi.MD_EINVAL and msg.startswith("md_traffic_lights: radius=") and "must be positive" in msg, msg


def test_the_stride(no_gpu):
    for bad in (0, 24, -16, 8):
        assert _call(out_stride=bad, cfg=dict(traffic_mode=0)) == (
            abi.MD_EINVAL, "md_traffic_lights: out_stride=%d must be a positive multiple of 16" % bad)


@pytest.mark.parametrize("mode", [0, 1, 2, 3])
def test_only_in_scenario_mode(no_gpu, mode):
    rc, msg = _call(cfg=dict(traffic_mode=mode))
    assert rc == abi.MD_EINVAL and msg.startswith("md_traffic_lights: only in scenario mode"), msg
    # the mode comes before the arrays
    assert _call(null=("s->nav", ), cfg=dict(traffic_mode=mode))[1].startswith("md_traffic_lights: only in scenario mode")


def test_one_observer_per_env(no_gpu):
    assert _call(cfg=dict(agents_per_env=2))[1].startswith("md_traffic_lights: agents_per_env=2")
    assert _call(cfg=dict(is_multi_agent=1))[1].startswith("md_traffic_lights: agents_per_env=1 is_multi_agent=1")


def test_required_arrays_by_name(no_gpu):
    assert _call(null=("s->nav", )) == (abi.MD_EINVAL, "required pointer s->nav is null")
    assert _call(null=("s->nav", "tl->tl_off"))[1] == "required pointer s->nav is null", "the arrays come before the tables"
    assert _call(null=("s->shape", )) == (abi.MD_EINVAL, "MdState.shape is null")


def test_only_those_are_required(no_gpu):
    rest = tuple("s->" + f for f in abi.STATE_FIELDS if f not in ("shape", "nav")) + tuple("w->" + f for f in abi.WORLD_FIELDS)
    assert _call(null=rest + ("tl->agent_light", ))[1] == "required pointer tl->agent_light is null"


@pytest.mark.parametrize("name", TABLES + ["agent_light"] + LIGHTS_OUT)
def test_tables_and_outputs_by_name(no_gpu, name):
    assert _call(null=("tl->" + name, )) == (abi.MD_EINVAL, "required pointer tl->%s is null" % name)


def test_tables_come_before_outputs_and_the_lights_block_is_optional_at_zero(no_gpu):
    assert _call(null=("tl->tl_status", "tl->agent_light"))[1] == "required pointer tl->tl_status is null"
    assert _call(null=("tl->agent_light", "tl->lights"))[1] == "required pointer tl->agent_light is null"
    off = tuple("tl->" + f for f in LIGHTS_OUT)
    assert _call(null=off)[1] == "required pointer tl->lights is null"
    assert _call(null=off + ("tl->agent_light", ), num_lights=0)[1] == "required pointer tl->agent_light is null"
    # with L = 0 and the three null, the next check is the alignment
    assert "tl_box must be 16-byte aligned" in _call(null=off, num_lights=0, tl_box=DUMMY + 4)[1]


def test_alignment(no_gpu):
    assert "must be 4-byte aligned" in _call(lights=DUMMY + 2)[1]
    assert "must be 4-byte aligned" in _call(lights_index=DUMMY + 1)[1]
    assert "must be 4-byte aligned" in _call(tl_off=DUMMY + 2)[1]
    assert "tl_box must be 16-byte aligned" in _call(tl_box=DUMMY + 4)[1]
    assert "tl_info must be 16-byte aligned" in _call(tl_info=DUMMY + 8)[1]


def test_the_lds_image_at_the_ceiling_fits_a_workgroup():
    # four waves, each 32 taken entries and two lists of max_scene_lights words
    assert 4 * (4 * 32 + 2 * 4 * 1024) == 33280 < 64 * 1024
