"""Loader of the HIP product library (metadrive_ped_amd/lib/libmdstep.so) through its C-ABI.

There is NO fallback: if the library is missing or its ABI does not match the binding, importing
the engine raises.  (The CPU oracle under oracle/ is test infrastructure and is never imported from
here.)  torch is imported first on purpose: its bundled libamdhip64.so.7 then satisfies the
library's DT_NEEDED entry by soname, so the tensors' device pointers, the torch stream handle and
our kernel launches all live in ONE HIP runtime instance.
"""
import ctypes as C
import os

from metadrive_ped_amd import abi

_LIB = None
# MD_LIB_PATH: tuning experiments only (A/B of differently compiled builds of the same source)
LIB_PATH = os.environ.get("MD_LIB_PATH") or os.path.join(os.path.dirname(os.path.abspath(__file__)), "lib", "libmdstep.so")


class MdStepError(RuntimeError):
    pass


def load():
    global _LIB
    if _LIB is not None:
        return _LIB
    import torch  # noqa: F401  (see module docstring)
    if not os.path.exists(LIB_PATH):
        raise MdStepError(
            "HIP library not found: {}\nBuild it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950).  There is no CPU fallback.".format(LIB_PATH))
    lib = C.CDLL(LIB_PATH)
    optional = {n: sig for n, sig in abi.OPTIONAL_ENTRY_POINTS.items() if hasattr(lib, n)}
    for name, (restype, argtypes) in dict(abi.ENTRY_POINTS, **abi.EXPERT_ENTRY_POINTS, **abi.AI_PROTECT_ENTRY_POINTS,
                                          **abi.EXPERT_SENSE_ENTRY_POINTS, **abi.CURRICULUM_ENTRY_POINTS, **abi.TOPDOWN_ENTRY_POINTS, **abi.RENDER_ENTRY_POINTS,
                                          **abi.BRANCH_ENTRY_POINTS, **abi.PED_ENTRY_POINTS, **abi.VECTOR_OBS_ENTRY_POINTS, **abi.SCENARIO_VECTOR_OBS_ENTRY_POINTS,
                                          **abi.TRAFFIC_LIGHTS_ENTRY_POINTS, **abi.SCENARIO_METRICS_ENTRY_POINTS,
                                          **abi.CONTACT_RESPONSE_ENTRY_POINTS, **optional).items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = restype, argtypes
    abi.check_abi(lib.md_abi, LIB_PATH)
    _LIB = lib
    return lib


def check(rc, what):
    if rc != abi.MD_OK:
        msg = load().md_last_error().decode("utf8", "replace")
        raise MdStepError("{} failed with code {}: {}".format(what, rc, msg))
