"""md_contact_response's place in the C-ABI (include/md_contact_response.h) and its argument check: the three struct pointers,
MdConfig.struct_size, MdContactResponse.struct_size, the sizes, the two ranges, scenario mode, the required MdState arrays by name.
Every call here is refused before any launch; those tests are skipped where a GPU is visible all the same, since a call that
slipped through the checks would launch on dummy pointers."""
import ctypes as C
import os
import re

import pytest

from metadrive_ped_amd import _lib, abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_BUF = C.create_string_buffer(4096)
DUMMY = (C.addressof(_BUF) + 15) & ~15
CONFIG = dict(struct_size=C.sizeof(abi.MdConfig), n_envs=8, agents_per_env=1, cap=32, n_beams=0, obs_dim=19, substeps=5, dt=0.02)
REQUIRED = ["shape", "dyn", "need_reset"]


@pytest.fixture
def no_gpu():
    import torch
    if torch.cuda.device_count() > 0:
        pytest.skip("a GPU is visible: the calls carry dummy pointers")


def _call(null=(), cfg=None, **fields):
    """md_contact_response with dummy pointers everywhere; `null`: the arguments / MdState arrays left null"""
    lib = _lib.load()
    k, s = abi.MdConfig(), abi.MdState()
    for name, v in dict(CONFIG, **(cfg or {})).items():
        setattr(k, name, v)
    for f in abi.STATE_FIELDS:
        setattr(s, f, None if f in null else DUMMY)
    cr = abi.make_md_contact_response(dict(skin=0.01, max_push=0.5))
    for name, v in fields.items():
        setattr(cr, name, v)
    args = [None if n in null else C.byref(x) for n, x in (("s", s), ("c", k), ("cr", cr))]
    rc = lib.md_contact_response(*args, None)
    return rc, lib.md_last_error().decode()


def test_entry_point_has_a_header_and_a_table_of_its_own():
    assert list(abi.CONTACT_RESPONSE_ENTRY_POINTS) == ["md_contact_response"]
    for table in (abi.ENTRY_POINTS, abi.EXPERT_ENTRY_POINTS, abi.AI_PROTECT_ENTRY_POINTS, abi.EXPERT_SENSE_ENTRY_POINTS,
                  abi.CURRICULUM_ENTRY_POINTS, abi.TOPDOWN_ENTRY_POINTS, abi.RENDER_ENTRY_POINTS, abi.BRANCH_ENTRY_POINTS,
                  abi.PED_ENTRY_POINTS, abi.VECTOR_OBS_ENTRY_POINTS, abi.OPTIONAL_ENTRY_POINTS):
        assert "md_contact_response" not in table
    assert abi.MD_ABI_VERSION == 12
    inc = os.path.join(ROOT, "include")
    declared = [f for f in sorted(os.listdir(inc)) if re.search(r"^int md_contact_response\(", open(os.path.join(inc, f)).read(), re.M)]
    assert declared == ["md_contact_response.h"]
    assert len(abi.CONTACT_RESPONSE_ENTRY_POINTS["md_contact_response"][1]) == 4
    assert hasattr(_lib.load(), "md_contact_response")


def test_the_binding_has_the_header_s_size_and_defaults():
    import contact_response_host as ch
    assert C.sizeof(abi.MdContactResponse) == ch.lib().hx_sizeof_contact_response() == 16
    cr = ch.params()
    assert (cr.struct_size, cr.reserved) == (16, 0) and abs(cr.skin - 0.01) < 1e-9 and cr.max_push == 0.5
    text = open(os.path.join(ROOT, "include", "md_contact_response.h")).read()
    assert "0.01 m" in text and "0.5 m" in text
    # ... and the library's: it accepts exactly this struct_size (test_struct_sizes)


def test_the_abi_structs_are_as_they_were():
    sizes = (C.c_int32 * 11)()
    assert _lib.load().md_abi(sizes, 11) == 12 and list(sizes) == abi.STRUCT_SIZES


@pytest.mark.parametrize("name", ["s", "c", "cr"])
def test_required_arguments_by_name(no_gpu, name):
    assert _call(null=(name, )) == (abi.MD_EINVAL, "required pointer %s is null" % name)


@pytest.mark.parametrize("name", REQUIRED)
def test_required_state_arrays_by_name(no_gpu, name):
    assert _call(null=(name, )) == (abi.MD_EINVAL, "required pointer s->%s is null" % name)


def test_only_those_are_required(no_gpu):
    # everything else null: the first complaint is still about a size, checked before any array
    rest = tuple(f for f in abi.STATE_FIELDS if f not in REQUIRED)
    assert _call(null=rest, cfg=dict(cap=0))[0] == abi.MD_EINVAL
    assert _call(null=rest + ("dyn", ))[1] == "required pointer s->dyn is null"


def test_struct_sizes(no_gpu):
    rc, msg = _call(cfg=dict(struct_size=4))
    assert rc == abi.MD_EABI and msg == "MdConfig.struct_size=4, library expects %d" % C.sizeof(abi.MdConfig)
    n = C.sizeof(abi.MdContactResponse)
    assert _call(struct_size=n - 4) == (abi.MD_EABI, "MdContactResponse.struct_size=%d, library expects %d" % (n - 4, n))
    assert _call(struct_size=n + 4) == (abi.MD_EABI, "MdContactResponse.struct_size=%d, library expects %d" % (n + 4, n))
    # before the sizes and the ranges
    assert _call(struct_size=0, cfg=dict(cap=0), skin=-1.0)[0] == abi.MD_EABI


def test_sizes_and_ranges_are_named(no_gpu):
    for cfg in (dict(n_envs=0), dict(cap=0), dict(cap=129)):
        rc, msg = _call(cfg=cfg)
        assert rc == abi.MD_EINVAL and msg.startswith("md_contact_response: bad sizes: "), (cfg, msg)
    for bad in (-0.01, float("nan")):
        rc, msg = _call(skin=bad)
        assert rc == abi.MD_EINVAL and msg.startswith("md_contact_response: skin=") and msg.endswith("must not be negative"), msg
    for bad in (0.0, -0.5, float("nan")):
        rc, msg = _call(max_push=bad)
        assert rc == abi.MD_EINVAL and msg.startswith("md_contact_response: max_push=") and msg.endswith("must be positive"), msg
    # ... before any array is asked for
    assert _call(null=("dyn", ), max_push=0.0)[1].startswith("md_contact_response: max_push=")


def test_scenario_mode_is_refused(no_gpu):
    rc, msg = _call(cfg=dict(traffic_mode=4))
    assert rc == abi.MD_EINVAL and msg.startswith("md_contact_response: not in scenario mode (traffic_mode 4)")
    for mode in (0, 1, 2, 3):       # every other mode passes the checks: the next complaint is the null array's
        assert _call(null=("need_reset", ), cfg=dict(traffic_mode=mode))[1] == "required pointer s->need_reset is null"
