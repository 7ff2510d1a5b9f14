"""md_branch's argument check (include/md_branch.h): the four struct pointers, MdConfig.struct_size, MdBranch.struct_size, the two
index arrays, the sizes, the pair count, the extras table and its entries.  Every call here is refused before any launch; skipped
where a GPU is visible all the same, since a call that slipped through the checks would launch on dummy pointers."""
import ctypes as C

import pytest

from metadrive_ped_amd import _lib, abi

_BUF = C.create_string_buffer(4096)
DUMMY = (C.addressof(_BUF) + 15) & ~15
CONFIG = dict(struct_size=C.sizeof(abi.MdConfig), n_envs=8, agents_per_env=1, cap=32, n_beams=0, obs_dim=19)
BRANCH = dict(struct_size=C.sizeof(abi.MdBranch), n_pairs=2, src_n_envs=8, dst_n_envs=8, n_extras=0)


@pytest.fixture(autouse=True)
def _no_gpu():
    import torch
    if torch.cuda.device_count() > 0:
        pytest.skip("a GPU is visible: the calls carry dummy pointers")


def _state():
    s = abi.MdState()
    for f in abi.STATE_FIELDS:
        setattr(s, f, DUMMY)
    return s


def _call(null=(), cfg=None, extras=(), **fields):
    """md_branch with dummy pointers everywhere; `null`: the arguments / MdBranch pointers left null; extras = [(dst, src, row_bytes)]"""
    lib = _lib.load()
    k, b = abi.MdConfig(), abi.MdBranch()
    for name, v in dict(CONFIG, **(cfg or {})).items():
        setattr(k, name, v)
    b.src_row, b.dst_row = DUMMY, DUMMY
    for name, v in dict(BRANCH, **fields).items():
        setattr(b, name, v)
    for name in ("src_row", "dst_row"):
        if name in null:
            setattr(b, name, None)
    for i, (d, s, rb) in enumerate(extras):
        b.extra[i].dst, b.extra[i].src, b.extra[i].row_bytes = d, s, rb
    dst, src = _state(), _state()
    args = [None if n in null else C.byref(x) for n, x in (("dst", dst), ("src", src), ("c", k), ("b", b))]
    rc = lib.md_branch(*args, None)
    return rc, lib.md_last_error().decode()


def test_entry_point_has_a_table_of_its_own():
    assert list(abi.BRANCH_ENTRY_POINTS) == ["md_branch"]
    for table in (abi.ENTRY_POINTS, abi.EXPERT_ENTRY_POINTS, abi.AI_PROTECT_ENTRY_POINTS, abi.EXPERT_SENSE_ENTRY_POINTS,
                  abi.CURRICULUM_ENTRY_POINTS, abi.TOPDOWN_ENTRY_POINTS, abi.RENDER_ENTRY_POINTS):
        assert "md_branch" not in table
    assert abi.MD_ABI_VERSION == 12


def test_the_binding_has_the_header_s_sizes():
    import hostlib
    lib = hostlib.build("branch_host")
    assert C.sizeof(abi.MdBranch) == lib.hx_sizeof_branch()
    assert abi.MD_BR_MAX_EXTRAS == lib.hx_max_extras()


@pytest.mark.parametrize("name", ["dst", "src", "c", "b"])
def test_required_arguments_by_name(name):
    assert _call(null=(name, )) == (abi.MD_EINVAL, "required pointer %s is null" % name)


@pytest.mark.parametrize("name", ["src_row", "dst_row"])
def test_required_index_arrays_by_name(name):
    assert _call(null=(name, )) == (abi.MD_EINVAL, "required pointer b->%s is null" % name)


def test_struct_sizes():
    rc, msg = _call(cfg=dict(struct_size=4))
    assert rc == abi.MD_EABI and msg == "MdConfig.struct_size=4, library expects %d" % C.sizeof(abi.MdConfig)
    n = C.sizeof(abi.MdBranch)
    assert _call(struct_size=n - 8) == (abi.MD_EABI, "MdBranch.struct_size=%d, library expects %d" % (n - 8, n))
    assert _call(struct_size=n + 8) == (abi.MD_EABI, "MdBranch.struct_size=%d, library expects %d" % (n + 8, n))


def test_sizes_and_counts_are_named():
    assert _call(n_pairs=0) == (abi.MD_EINVAL, "md_branch: n_pairs=0 must be positive")
    assert _call(n_pairs=-3) == (abi.MD_EINVAL, "md_branch: n_pairs=-3 must be positive")
    assert _call(src_n_envs=0) == (abi.MD_EINVAL, "md_branch: src_n_envs=0 and dst_n_envs=8 must be positive")
    assert _call(dst_n_envs=-1) == (abi.MD_EINVAL, "md_branch: src_n_envs=8 and dst_n_envs=-1 must be positive")
    rc, msg = _call(cfg=dict(cap=129))
    assert rc == abi.MD_EINVAL and msg.startswith("md_branch: bad sizes: cap=129 "), msg
    rc, msg = _call(cfg=dict(agents_per_env=0))
    assert rc == abi.MD_EINVAL and msg.startswith("md_branch: bad sizes: cap=32 agents_per_env=0 "), msg


def test_the_extras_table():
    m = abi.MD_BR_MAX_EXTRAS
    assert _call(n_extras=m + 1) == (abi.MD_EINVAL, "md_branch: n_extras=%d must lie in [0, MD_BR_MAX_EXTRAS=%d]" % (m + 1, m))
    assert _call(n_extras=-1) == (abi.MD_EINVAL, "md_branch: n_extras=-1 must lie in [0, MD_BR_MAX_EXTRAS=%d]" % m)
    ok = (DUMMY, DUMMY, 1)
    assert _call(n_extras=2, extras=[ok, (DUMMY, DUMMY, 0)]) == (abi.MD_EINVAL, "md_branch: extra[1].row_bytes=0 must be positive")
    assert _call(n_extras=1, extras=[(DUMMY, DUMMY, -4)]) == (abi.MD_EINVAL, "md_branch: extra[0].row_bytes=-4 must be positive")
    assert _call(n_extras=2, extras=[ok, (None, DUMMY, 4)]) == (abi.MD_EINVAL, "required pointer b->extra[1].dst is null")
    assert _call(n_extras=1, extras=[(DUMMY, None, 4)]) == (abi.MD_EINVAL, "required pointer b->extra[0].src is null")
    # an entry beyond n_extras is not looked at: the first complaint is still the pair count's
    assert _call(n_extras=1, n_pairs=0, extras=[ok, (None, None, 0)]) == (abi.MD_EINVAL, "md_branch: n_pairs=0 must be positive")
