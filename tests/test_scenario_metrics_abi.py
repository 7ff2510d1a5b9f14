"""md_scenario_metrics's place in the C-ABI (include/md_scenario_metrics.h) and its argument check, in the order the header states: the
four struct pointers, the struct_size fields, the sizes, ttc_samples, ttc_dt, the step period, the strides, the mode, the required
MdState arrays, then the outputs and the state rows by name, alignment; and the config key's checks.  Every call here is refused
before any launch; those tests are skipped where a GPU is visible all the same, since a call that slipped through the checks would
launch on dummy pointers."""
import ctypes as C
import os
import re

import pytest

from metadrive_ped_amd import _lib, abi
from metadrive_ped_amd.config import SCENARIO_METRICS_DEFAULT_CONFIG, SCENARIO_METRICS_RANGES, check_scenario_metrics

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_BUF = C.create_string_buffer(4096)
DUMMY = (C.addressof(_BUF) + 15) & ~15
CONFIG = dict(struct_size=C.sizeof(abi.MdConfig), n_envs=8, agents_per_env=1, cap=32, n_beams=0, obs_dim=19, substeps=5, dt=0.02,
              traffic_mode=4, scenario_length=80, track_len=80)
REQUIRED = ["dyn", "nav", "flags", "step_info", "track_shape", "track_dyn"]       # after MdState.shape, which check_common names
OUT = list(abi.SCENARIO_METRICS_OUTPUTS) + ["state"]


@pytest.fixture
def no_gpu():
    import torch
    if torch.cuda.device_count() > 0:
        pytest.skip("a GPU is visible: the calls carry dummy pointers")


def _call(null=(), cfg=None, **fields):
    """md_scenario_metrics with dummy pointers everywhere; `null`: the arguments ("w", "s", "c", "sm"), the MdWorld / MdState arrays
    ("w->x", "s->x") and the MdScenarioMetrics pointers ("sm->x") left null; `fields`: set on the struct"""
    lib = _lib.load()
    k, s, w = abi.MdConfig(), abi.MdState(), abi.MdWorld()
    for name, v in dict(CONFIG, **(cfg or {})).items():
        setattr(k, name, v)
    w.n_maps, w.n_envs = 1, k.n_envs
    for f in abi.STATE_FIELDS:
        setattr(s, f, None if "s->" + f in null else DUMMY)
    for f in abi.WORLD_FIELDS:
        setattr(w, f, None if "w->" + f in null else DUMMY)
    ptrs = dict(out_stride=192, state_stride=144, light_stride=128)
    ptrs.update({f: DUMMY for f in OUT + ["agent_light"] if "sm->" + f not in null})
    sm = abi.make_md_scenario_metrics(SCENARIO_METRICS_DEFAULT_CONFIG, ptrs)
    for name, v in fields.items():
        setattr(sm, name, v)
    args = [None if n in null else C.byref(x) for n, x in (("w", w), ("s", s), ("c", k), ("sm", sm))]
    rc = lib.md_scenario_metrics(*args, None)
    return rc, lib.md_last_error().decode()


def test_entry_point_has_a_header_and_a_table_of_its_own():
    assert list(abi.SCENARIO_METRICS_ENTRY_POINTS) == ["md_scenario_metrics"]
    for table in (abi.ENTRY_POINTS, abi.EXPERT_ENTRY_POINTS, abi.AI_PROTECT_ENTRY_POINTS, abi.EXPERT_SENSE_ENTRY_POINTS,
                  abi.CURRICULUM_ENTRY_POINTS, abi.TOPDOWN_ENTRY_POINTS, abi.RENDER_ENTRY_POINTS, abi.BRANCH_ENTRY_POINTS,
                  abi.PED_ENTRY_POINTS, abi.VECTOR_OBS_ENTRY_POINTS, abi.SCENARIO_VECTOR_OBS_ENTRY_POINTS, abi.TRAFFIC_LIGHTS_ENTRY_POINTS,
                  abi.CONTACT_RESPONSE_ENTRY_POINTS, abi.OPTIONAL_ENTRY_POINTS):
        assert "md_scenario_metrics" not in table
    assert abi.MD_ABI_VERSION == 12, "no existing struct changed: the ABI version stays"
    inc = os.path.join(ROOT, "include")
    declared = [f for f in sorted(os.listdir(inc)) if re.search(r"^int md_scenario_metrics\(", open(os.path.join(inc, f)).read(), re.M)]
    assert declared == ["md_scenario_metrics.h"]
    assert len(abi.SCENARIO_METRICS_ENTRY_POINTS["md_scenario_metrics"][1]) == 5
    assert hasattr(_lib.load(), "md_scenario_metrics")


def test_the_binding_has_the_header_s_size_offsets_and_ceilings():
    import scenario_metrics_host as mh
    lib = mh.lib()
    M = abi.MdScenarioMetrics
    n = C.sizeof(M)
    assert n == lib.hx_sizeof_scenario_metrics() and n % 8 == 0
    assert [lib.hx_sm_offsetof(i) for i in range(4)] == [M.max_lon_accel.offset, M.out_stride.offset, M.agent_light.offset, M.state.offset]
    assert M._fields_[0][0] == "struct_size" and M.struct_size.offset == 0
    assert [lib.hx_sm_limit(i) for i in range(4)] == [abi.MD_SM_MAX_TTC_SAMPLES, abi.MD_SM_STEP_COLS, abi.MD_SM_EPISODE_COLS,
                                                      abi.MD_SM_STATE_COLS] == [64, 12, 24, 12]
    assert SCENARIO_METRICS_RANGES["ttc_samples"] == (0, abi.MD_SM_MAX_TTC_SAMPLES)
    assert len(abi.SCENARIO_METRICS_STEP_COLUMNS) == 12 and len(abi.SCENARIO_METRICS_EPISODE_COLUMNS) == 24
    assert len(abi.SCENARIO_METRICS_HISTORY_COLUMNS) == 12
    assert abi.SCENARIO_METRICS_STEP_COLUMNS[9:11] == ("ttc", "on_red") and abi.SCENARIO_METRICS_EPISODE_COLUMNS[18:20] == (
        "route_completion", "arrive_dest")
    sm = abi.make_md_scenario_metrics(SCENARIO_METRICS_DEFAULT_CONFIG, dict(out_stride=16))
    assert (sm.ttc_samples, sm.out_stride, sm.state_stride, sm.light_stride, sm.agent_light) == (30, 16, 0, 0, None)
    assert abs(sm.ttc_dt - 0.1) < 1e-7 and abs(sm.min_lon_accel + 4.05) < 1e-6 and abs(sm.max_yaw_accel - 1.93) < 1e-6
    outs, row, state, state_row = abi.scenario_metrics_blocks()
    assert [(k, v[0]) for k, v in outs.items()] == [("step", 0), ("step_valid", 48), ("ttc_slot", 64), ("last_episode", 80), ("episodes", 176)]
    assert row == 192 and [(k, v[0]) for k, v in state.items()] == [("history", 0), ("episode", 48)] and state_row == 144


def test_the_abi_structs_are_as_they_were():
    sizes = (C.c_int32 * 11)()
    assert _lib.load().md_abi(sizes, 11) == 12 and list(sizes) == abi.STRUCT_SIZES
    # the sizes the parent commit's library reported for MdWorld, MdState and MdConfig
    assert (C.sizeof(abi.MdWorld), C.sizeof(abi.MdState), C.sizeof(abi.MdConfig)) == tuple(abi.STRUCT_SIZES[8:11])


@pytest.mark.parametrize("name", ["w", "s", "c", "sm"])
def test_required_arguments_by_name(no_gpu, name):
    assert _call(null=(name, )) == (abi.MD_EINVAL, "required pointer %s is null" % name)


def test_struct_sizes(no_gpu):
    rc, msg = _call(cfg=dict(struct_size=4))
    assert rc == abi.MD_EABI and msg == "MdConfig.struct_size=4, library expects %d" % C.sizeof(abi.MdConfig)
    n = C.sizeof(abi.MdScenarioMetrics)
    for bad in (n - 8, n + 8):
        assert _call(struct_size=bad) == (abi.MD_EABI, "MdScenarioMetrics.struct_size=%d, library expects %d" % (bad, n))
    # before the sizes and the ranges
    assert _call(struct_size=0, cfg=dict(cap=0), ttc_samples=-1)[0] == abi.MD_EABI


def test_sizes_come_before_the_ranges(no_gpu):
    for cfg in (dict(n_envs=0), dict(cap=0), dict(cap=129), dict(agents_per_env=0)):
        rc, msg = _call(cfg=cfg, ttc_samples=-1)
        assert rc == abi.MD_EINVAL and msg.startswith("bad sizes: "), (cfg, msg)


def test_the_samples_against_their_bounds(no_gpu):
    for bad in (-1, 65):
        assert _call(ttc_samples=bad) == (abi.MD_EINVAL, "md_scenario_metrics: ttc_samples=%d must lie in [0, MD_SM_MAX_TTC_SAMPLES=64]" % bad)
    # ... before ttc_dt, the mode and any array
    assert _call(null=("s->nav", "sm->step"), cfg=dict(traffic_mode=0), ttc_dt=0.0, ttc_samples=65)[1].startswith(
        "md_scenario_metrics: ttc_samples=")


def test_the_sample_period_must_be_positive(no_gpu):
    for bad in (0.0, -0.1, float("nan"), 1e7):
        rc, msg = _call(ttc_dt=bad, out_stride=0)
        assert rc == abi.MD_EINVAL and msg.startswith("md_scenario_metrics: ttc_dt=") and "must be positive" in msg, msg


def test_the_step_period_must_be_positive(no_gpu):
    for cfg in (dict(dt=0.0), dict(substeps=0), dict(dt=-0.02)):
        rc, msg = _call(cfg=cfg, out_stride=0)
        assert rc == abi.MD_EINVAL and msg.startswith("md_scenario_metrics: the step period dt * substeps"), msg


def test_the_strides(no_gpu):
    for bad in (0, 24, -16, 8):
        assert _call(out_stride=bad, cfg=dict(traffic_mode=0)) == (
            abi.MD_EINVAL, "md_scenario_metrics: out_stride=%d must be a positive multiple of 16" % bad)
    for bad in (0, 128, 152, -144):
        assert _call(state_stride=bad, cfg=dict(traffic_mode=0)) == (
            abi.MD_EINVAL, "md_scenario_metrics: state_stride=%d must be a multiple of 16, at least 144" % bad)
    assert "light_stride=0 must be positive" in _call(light_stride=0)[1]
    # agent_light NULL means no lights configured: the call then passes every check, as the full one does, and fails at the launch
    assert _call(light_stride=0, agent_light=None)[0] == _call()[0] == abi.MD_ELAUNCH


@pytest.mark.parametrize("mode", [0, 1, 2, 3])
def test_only_in_scenario_mode(no_gpu, mode):
    rc, msg = _call(cfg=dict(traffic_mode=mode))
    assert rc == abi.MD_EINVAL and msg.startswith("md_scenario_metrics: only in scenario mode"), msg
    # the mode comes before the arrays
    assert _call(null=("s->nav", ), cfg=dict(traffic_mode=mode))[1].startswith("md_scenario_metrics: only in scenario mode")


def test_one_observer_per_env(no_gpu):
    assert _call(cfg=dict(agents_per_env=2))[1].startswith("md_scenario_metrics: agents_per_env=2")
    assert _call(cfg=dict(is_multi_agent=1))[1].startswith("md_scenario_metrics: agents_per_env=1 is_multi_agent=1")


@pytest.mark.parametrize("name", REQUIRED)
def test_required_arrays_by_name(no_gpu, name):
    assert _call(null=("s->" + name, )) == (abi.MD_EINVAL, "required pointer s->%s is null" % name)
    assert _call(null=("s->" + name, "sm->step"))[1] == "required pointer s->%s is null" % name, "the arrays come before the outputs"


def test_the_shape_array_and_table_order(no_gpu):
    assert _call(null=("s->shape", )) == (abi.MD_EINVAL, "MdState.shape is null")
    assert _call(null=tuple("s->" + f for f in REQUIRED))[1] == "required pointer s->dyn is null"


def test_only_those_are_required(no_gpu):
    rest = tuple("s->" + f for f in abi.STATE_FIELDS if f not in ["shape"] + REQUIRED) + tuple("w->" + f for f in abi.WORLD_FIELDS)
    assert _call(null=rest + ("sm->agent_light", "sm->step"))[1] == "required pointer sm->step is null"


@pytest.mark.parametrize("name", OUT)
def test_outputs_and_state_by_name(no_gpu, name):
    assert _call(null=("sm->" + name, )) == (abi.MD_EINVAL, "required pointer sm->%s is null" % name)


def test_alignment(no_gpu):
    for name in abi.SCENARIO_METRICS_OUTPUTS:
        assert "must be 4-byte aligned" in _call(**{name: DUMMY + 2})[1], name
    assert _call(state=DUMMY + 8)[1] == "md_scenario_metrics: state must be 16-byte aligned"


def test_the_lds_image_fits_a_workgroup():
    # four waves, each a list of at most MD_MAX_CAP movers of eight words
    assert 4 * 128 * 8 * 4 == 16384 < 64 * 1024


# -- the config key -------------------------------------------------------------------------------------------------------------------
def test_defaults_and_the_checks_by_name():
    assert check_scenario_metrics({}) == SCENARIO_METRICS_DEFAULT_CONFIG
    assert SCENARIO_METRICS_DEFAULT_CONFIG == dict(ttc_samples=30, ttc_dt=0.1, ttc_threshold=0.95, max_lon_accel=2.40, min_lon_accel=-4.05,
                                                   max_lat_accel=4.89, max_lon_jerk=4.13, max_jerk=8.37, max_yaw_rate=0.95, max_yaw_accel=1.93)
    assert set(abi.SCENARIO_METRICS_BOUNDS) | {"ttc_samples", "ttc_dt", "ttc_threshold"} == set(SCENARIO_METRICS_DEFAULT_CONFIG)
    got = check_scenario_metrics(dict(ttc_samples=0, max_jerk=9))
    assert got["ttc_samples"] == 0 and got["max_jerk"] == 9.0 and isinstance(got["max_jerk"], float)
    with pytest.raises(ValueError, match="None \\(off\\) or a dict"):
        check_scenario_metrics(True)
    with pytest.raises(ValueError, match="unknown key.*ttc_sample'"):
        check_scenario_metrics(dict(ttc_sample=3))
    for bad in (-1, 65, 3.0, True):
        with pytest.raises(ValueError, match="ttc_samples"):
            check_scenario_metrics(dict(ttc_samples=bad))
    for key, bad in (("ttc_dt", 0), ("ttc_dt", -0.1), ("ttc_dt", "0.1"), ("ttc_threshold", float("nan")), ("max_lon_accel", -1.0),
                     ("min_lon_accel", 0.5), ("max_jerk", None), ("max_yaw_rate", float("inf")), ("max_lat_accel", True)):
        with pytest.raises(ValueError, match="scenario_metrics\\['%s'\\]" % key):
            check_scenario_metrics({key: bad})


def test_the_key_belongs_to_the_scenario_envs():
    from metadrive_ped_amd.config import make_config
    from metadrive_ped_amd.scenario import make_scenario_config
    with pytest.raises(KeyError, match="scenario_metrics"):
        make_config(dict(scenario_metrics={}))
    assert make_scenario_config({})["scenario_metrics"] is None
    assert make_scenario_config(dict(scenario_metrics=dict(ttc_samples=5)))["scenario_metrics"]["ttc_samples"] == 5
    with pytest.raises(ValueError, match="scenario_metrics"):
        make_scenario_config(dict(scenario_metrics=dict(nope=1)))
