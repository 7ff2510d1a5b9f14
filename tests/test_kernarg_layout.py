"""The lean workgroup kernel reads its arguments straight from the kernel-argument segment, at offsetof(MdStepArgs, field)
(include/md_lean_view.h, csrc/parts/lean_view.inc).  MdStepArgs only DESCRIBES the step kernels' parameter list, so a member out of
step with it would be a wild pointer on the device.  No GPU: a device-only compile with the hipcc line of tools/kernel_regs.sh, the
`.args` (`.offset`, `.size`) of every step kernel read from the code object's metadata and held against the header's offsets as
the host compiler sees them (tests/kernarg_layout_host.c), for every member and every field the kernel reads."""
import ctypes as C
import os
import re
import subprocess

import pytest

import hostlib

ROOT = hostlib.ROOT
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
LLVM = os.environ.get("LLVM", "/opt/rocm/lib/llvm/bin")
STEP_KERNELS = ("env_kernel", "wave_step_kernel", "scenario_step_kernel")


@pytest.fixture(scope="module")
def kernel_args(tmp_path_factory):
    """-> {kernel symbol: [(offset, size, value_kind), ...]} of the device code object"""
    d = tmp_path_factory.mktemp("kernarg")
    obj, co = str(d / "md_dev.o"), str(d / "md_dev.co")
    subprocess.check_call([HIPCC, "-O3", "--offload-arch=gfx950", "-ffp-contract=off", "-std=c++17", "-I" + os.path.join(ROOT, "include"),
                           "--cuda-device-only", "-c", os.path.join(ROOT, "metadrive_ped_amd", "csrc", "mdstep.hip"), "-o", obj],
                          stderr=subprocess.DEVNULL)
    subprocess.check_call([os.path.join(LLVM, "clang-offload-bundler"), "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950",
                           "--input=" + obj, "--output=" + co, "--unbundle"])
    notes = subprocess.check_output([os.path.join(LLVM, "llvm-readelf"), "--notes", co], text=True)
    # the metadata as llvm-readelf prints it: a kernel's record opens with "  - .key:", its own keys stand at column 4, an
    # argument's record opens with "      - .key:" and its keys stand at column 8
    kernels, args = {}, []
    for line in notes.splitlines():
        m = re.match(r"^( *)(- )?\.(\w+):\s*(.*)$", line)
        if not m:
            continue
        col, dash, key, val = len(m.group(1)) + (2 if m.group(2) else 0), m.group(2), m.group(3), m.group(4).strip()
        if col == 4 and dash:
            args = []
        if col == 8:
            if dash:
                args.append({})
            args[-1][key] = val
        elif col == 4 and key == "name":
            kernels[val] = [(int(a["offset"]), int(a["size"]), a.get("value_kind", "")) for a in args]
    assert kernels, "no kernel metadata in the code object"
    return kernels


@pytest.fixture(scope="module")
def layout():
    """-> (members, fields) of MdStepArgs as the host compiler lays it out: lists of (name, offset, size)"""
    lib = hostlib.build("kernarg_layout_host")
    lib.hx_kernarg_layout.restype = C.c_int
    lib.hx_kernarg_layout.argtypes = [C.c_char_p, C.c_int]
    buf = C.create_string_buffer(1 << 14)
    n = lib.hx_kernarg_layout(buf, len(buf))
    assert n > 0
    members, fields = [], []
    into = members
    for line in buf.value.decode().splitlines():
        if line == "--":
            into = fields
            continue
        name, off, size = line.split()
        into.append((name, int(off), int(size)))
    assert [m[0] for m in members] == ["w", "g", "c", "lidar_out", "lidar_stride", "lidar_offset"]
    assert len(fields) >= 30
    return members, fields


def _step_kernels(kernel_args):
    return {k: v for k, v in kernel_args.items() if any(s in k for s in STEP_KERNELS)}


def test_every_step_kernel_is_found(kernel_args):
    ks = _step_kernels(kernel_args)
    for stem in STEP_KERNELS:
        assert any(stem in k for k in ks), stem
    # the two lean non-staged workgroup kernels, the ones that read the segment: the narrow form and its sibling
    assert any("env_kernelILi511ELb0ELb0ELb0ELi256ELb1EE" in k for k in ks)
    assert any("env_kernelILi511ELb0ELb0ELb0ELi256ELb0EE" in k for k in ks)


def test_members_are_the_kernels_parameters(kernel_args, layout):
    members, _ = layout
    for name, args in _step_kernels(kernel_args).items():
        explicit = [a for a in args if not a[2].startswith("hidden")]
        assert len(explicit) == len(members), (name, explicit)
        for (m, off, size), (a_off, a_size, _) in zip(members, explicit):
            assert (off, size) == (a_off, a_size), "%s: MdStepArgs.%s at %d size %d, the kernel's parameter at %d size %d" % (
                name, m, off, size, a_off, a_size)


def test_every_field_read_lies_in_its_parameter(kernel_args, layout):
    members, fields = layout
    by_name = {m: (off, size) for m, off, size in members}
    for name, args in _step_kernels(kernel_args).items():
        at = {a[0]: a[1] for a in args}
        for f, off, size in fields:
            m_off, m_size = by_name[f.split(".")[0]]
            assert at.get(m_off) == m_size, (name, f)
            assert m_off <= off and off + size <= m_off + m_size and off % size == 0, "%s: field %s at %d size %d outside [%d, %d)" % (
                name, f, off, size, m_off, m_off + m_size)
            assert size in (4, 8), (f, size)

