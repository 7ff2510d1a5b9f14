"""md_ped's place in the C-ABI (include/md_ped.h) and its argument check: the three struct pointers, MdConfig.struct_size,
MdPed.struct_size, the sizes, the required MdState arrays by name.  Every call here is refused before any launch; those tests are
skipped where a GPU is visible all the same, since a call that slipped through the checks would launch on dummy pointers."""
import ctypes as C
import os
import re

import pytest

from metadrive_ped_amd import _lib, abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_BUF = C.create_string_buffer(4096)
DUMMY = (C.addressof(_BUF) + 15) & ~15
CONFIG = dict(struct_size=C.sizeof(abi.MdConfig), n_envs=8, agents_per_env=1, cap=32, n_beams=0, obs_dim=19, substeps=5, dt=0.02)
REQUIRED = ["shape", "dyn", "nav", "pid", "idm_rand", "need_reset"]


@pytest.fixture
def no_gpu():
    import torch
    if torch.cuda.device_count() > 0:
        pytest.skip("a GPU is visible: the calls carry dummy pointers")


def _call(null=(), cfg=None, **fields):
    """md_ped with dummy pointers everywhere; `null`: the arguments / MdState arrays left null"""
    lib = _lib.load()
    k, s = abi.MdConfig(), abi.MdState()
    for name, v in dict(CONFIG, **(cfg or {})).items():
        setattr(k, name, v)
    for f in abi.STATE_FIELDS:
        setattr(s, f, None if f in null else DUMMY)
    p = abi.make_md_ped(dict(wait_min_steps=10, clear_dist=1.0, margin=1.0, time_margin=1.0, yield_ahead=3.0, yield_time=1.5))
    for name, v in fields.items():
        setattr(p, name, v)
    args = [None if n in null else C.byref(x) for n, x in (("s", s), ("c", k), ("p", p))]
    rc = lib.md_ped(*args, None)
    return rc, lib.md_last_error().decode()


def test_entry_point_has_a_header_and_a_table_of_its_own():
    assert list(abi.PED_ENTRY_POINTS) == ["md_ped"]
    for table in (abi.ENTRY_POINTS, abi.EXPERT_ENTRY_POINTS, abi.AI_PROTECT_ENTRY_POINTS, abi.EXPERT_SENSE_ENTRY_POINTS,
                  abi.CURRICULUM_ENTRY_POINTS, abi.TOPDOWN_ENTRY_POINTS, abi.RENDER_ENTRY_POINTS, abi.BRANCH_ENTRY_POINTS):
        assert "md_ped" not in table
    assert abi.MD_ABI_VERSION == 12
    inc = os.path.join(ROOT, "include")
    declared = [f for f in sorted(os.listdir(inc)) if re.search(r"^int md_ped\(", open(os.path.join(inc, f)).read(), re.M)]
    assert declared == ["md_ped.h"]
    assert len(abi.PED_ENTRY_POINTS["md_ped"][1]) == 4
    assert hasattr(_lib.load(), "md_ped")


def test_the_binding_has_the_header_s_size():
    import ped_host
    assert C.sizeof(abi.MdPed) == ped_host.lib().hx_sizeof_ped() == 32
    # ... and the library's: it accepts exactly this struct_size (test_struct_sizes)


def test_the_phase_values_are_the_header_s():
    text = open(os.path.join(ROOT, "include", "md_ped.h")).read()
    for name in ("OFF", "WAIT_A", "CROSS_AB", "WAIT_B", "CROSS_BA"):
        assert int(re.search(r"#define MD_PED_%s (\d+)" % name, text).group(1)) == getattr(abi, "PED_" + name)


@pytest.mark.parametrize("name", ["s", "c", "p"])
def test_required_arguments_by_name(no_gpu, name):
    assert _call(null=(name, )) == (abi.MD_EINVAL, "required pointer %s is null" % name)


@pytest.mark.parametrize("name", REQUIRED)
def test_required_state_arrays_by_name(no_gpu, name):
    assert _call(null=(name, )) == (abi.MD_EINVAL, "required pointer s->%s is null" % name)


def test_only_those_are_required(no_gpu):
    # everything else null: the first complaint is still about a size, checked before any array
    rest = tuple(f for f in abi.STATE_FIELDS if f not in REQUIRED)
    assert _call(null=rest, cfg=dict(cap=0))[0] == abi.MD_EINVAL
    assert _call(null=rest + ("pid", ))[1] == "required pointer s->pid is null"


def test_struct_sizes(no_gpu):
    rc, msg = _call(cfg=dict(struct_size=4))
    assert rc == abi.MD_EABI and msg == "MdConfig.struct_size=4, library expects %d" % C.sizeof(abi.MdConfig)
    n = C.sizeof(abi.MdPed)
    assert _call(struct_size=n - 4) == (abi.MD_EABI, "MdPed.struct_size=%d, library expects %d" % (n - 4, n))
    assert _call(struct_size=n + 4) == (abi.MD_EABI, "MdPed.struct_size=%d, library expects %d" % (n + 4, n))


def test_sizes_are_named(no_gpu):
    for cfg in (dict(n_envs=0), dict(cap=0), dict(cap=129), dict(substeps=0), dict(dt=0.0)):
        rc, msg = _call(cfg=cfg)
        assert rc == abi.MD_EINVAL and msg.startswith("md_ped: bad sizes: "), (cfg, msg)
    assert _call(wait_min_steps=-1) == (abi.MD_EINVAL, "md_ped: wait_min_steps=-1 must not be negative")
