"""Argument-checking corpus of the C-ABI: which pointers each entry point requires, and which arguments it refuses.

Every entry point the headers declare, except md_abi / md_last_error, is called once per profile with every pointer set
(a non-null, 16-byte aligned host address; struct pointer fields included) and then once per pointer with just that one
null.  The profiles set the config, world sizes and scalar arguments so that every branch of the library's checks is
reached.  Each call's outcome is [rc, md_last_error()] when the library refuses it, or "passed" when it gets as far as
the launch: on a machine without a GPU that launch fails with MD_ELAUNCH and the runtime's message, which is not ours.

A passed call would launch a kernel on dummy pointers wherever a GPU is present, so run() is only for machines without
one (tests/test_abi_requirements.py skips otherwise).  The stream argument stays NULL throughout.
tools/gen_abi_requirements.py records run() into tests/golden/abi_requirements.json.
"""
import ctypes as C
import json
import math
import os
import re

from metadrive_ped_amd import abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADERS = ("mdstep.h", "md_expert.h")
SKIP = ("md_abi", "md_last_error")

_CTYPES = {"int": C.c_int, "float": C.c_float, "uint32_t": C.c_uint32, "size_t": C.c_size_t}


def declarations():
    """{name: [(C type, argument name), ...]} of the functions the C-ABI headers declare, in header order."""
    out = {}
    for h in HEADERS:
        src = open(os.path.join(ROOT, "include", h)).read()
        src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
        for name, args in re.findall(r"^(?:int|const char\*)\s+(md_\w+)\s*\(([^)]*)\)\s*;", src, flags=re.M):
            args = [] if args.strip() == "void" else [a.strip() for a in args.split(",")]
            out[name] = [tuple(re.match(r"(.*?)\s*(\w+)$", a, flags=re.S).groups()) for a in args]
    return out


BASE_CONFIG = dict(struct_size=C.sizeof(abi.MdConfig), n_envs=8, agents_per_env=1, cap=32, n_beams=240, obs_dim=259,
                   substeps=5, horizon=1000, dt=0.02, lidar_range=50.0)
BASE_WORLD = dict(n_maps=1, n_envs=8, max_lanes=16, max_roads=8, n_dest=1, n_vclass=1)
BASE_ARGS = dict(out_stride=259, out_offset=19, n_beams=12, range=50.0, kind_mask=0x1E, n_beams0=12, range0=50.0,
                 kind_mask0=0x1E, out_offset0=0, n_beams1=12, range1=50.0, kind_mask1=0x1E, out_offset1=12, n_draws=2,
                 op=0, n=4, nbytes=64)
MISALIGNED = "misaligned"   # the dummy address + 4
SCENE = dict(traffic_mode=4, track_len=10, obs_dim=31 + 240)
MULTI = dict(is_multi_agent=1, agents_per_env=4)

# (name, {"config": MdConfig fields, "world": MdWorld fields, "null": pointers null in every call, "args": scalar arguments})
# A profile with "config" or "world" applies to the entry points that take an MdConfig, one with "args" to those that
# take one of its arguments; "base" applies to all.
PROFILES = [
    ("base", {}),
    ("wave_kernel", dict(config=dict(step_kernel=1))),
    ("agent_idm", dict(config=dict(agent_idm=1))),
    ("traffic_respawn", dict(config=dict(traffic_mode=1))),
    ("traffic_hybrid", dict(config=dict(traffic_mode=2))),
    ("replay", dict(config=dict(traffic_mode=3, track_len=10))),
    ("replay_no_track", dict(config=dict(traffic_mode=3))),
    ("traffic_mode_5", dict(config=dict(traffic_mode=5))),
    ("traffic_mode_neg", dict(config=dict(traffic_mode=-1))),
    ("scenario", dict(config=SCENE, null=["s->route_n"])),
    ("scenario_route", dict(config=dict(SCENE, route_seg_cap=4, route_vert_cap=8))),
    ("scenario_route_no_segs", dict(config=dict(SCENE, route_seg_cap=0, route_vert_cap=8))),
    ("scenario_route_few_verts", dict(config=dict(SCENE, route_seg_cap=4, route_vert_cap=7))),
    ("scenario_no_track", dict(config=dict(SCENE, track_len=0), null=["s->route_n"])),
    ("scenario_two_agents", dict(config=dict(SCENE, agents_per_env=2), null=["s->route_n"])),
    ("scenario_obs_dim_off", dict(config=dict(SCENE, obs_dim=31 + 239), null=["s->route_n"])),
    ("scenario_big_lds", dict(config=dict(SCENE, cap=128, route_seg_cap=4096, route_vert_cap=8))),
    ("marl", dict(config=MULTI)),
    ("marl_respawn", dict(config=dict(MULTI, allow_respawn=1))),
    ("marl_respawn_no_dest", dict(config=dict(MULTI, allow_respawn=1), world=dict(n_dest=0))),
    ("marl_no_dest", dict(config=MULTI, world=dict(n_dest=0))),
    ("marl_traffic", dict(config=dict(MULTI, traffic_mode=1))),
    ("marl_wide", dict(config=dict(MULTI, agents_per_env=16))),
    ("marl_tollgate", dict(config=dict(MULTI, ma_kind=abi.MA_TOLLGATE, obs_dim=9 + 240 + 2))),
    ("two_agents", dict(config=dict(agents_per_env=2))),
    ("no_lidar", dict(config=dict(n_beams=0, obs_dim=19))),
    ("others_4", dict(config=dict(num_others=4, obs_dim=19 + 16 + 240))),
    ("others_17", dict(config=dict(num_others=17, obs_dim=19 + 68 + 240))),
    ("others_no_lidar", dict(config=dict(num_others=4, n_beams=0, obs_dim=19 + 16))),
    ("struct_size", dict(config=dict(struct_size=4))),
    ("n_envs_0", dict(config=dict(n_envs=0), world=dict(n_envs=0))),
    ("cap_0", dict(config=dict(cap=0))),
    ("cap_129", dict(config=dict(cap=129))),
    ("agents_0", dict(config=dict(agents_per_env=0))),
    ("agents_over_cap", dict(config=dict(MULTI, agents_per_env=33))),
    ("n_beams_neg", dict(config=dict(n_beams=-1))),
    ("n_beams_1025", dict(config=dict(n_beams=1025, obs_dim=19 + 1025))),
    ("world_n_envs", dict(world=dict(n_envs=7))),
    ("obs_dim_plus_1", dict(config=dict(obs_dim=260))),
    ("obs_dim_18", dict(config=dict(obs_dim=18))),
    ("max_lanes_0", dict(world=dict(max_lanes=0))),
    ("max_roads_0", dict(world=dict(max_roads=0))),
    ("unstaged_map", dict(world=dict(max_lanes=65))),
    ("big_lds", dict(config=dict(cap=128), world=dict(max_lanes=64, max_roads=2048))),
    ("big_lds_wave", dict(config=dict(cap=128, step_kernel=1), world=dict(max_lanes=64, max_roads=2048))),
    ("expert_refused", dict(config=dict(lidar_range=40.0))),
    ("expert_random_model", dict(config=dict(random_agent_model=1, obs_dim=261))),
    ("stride_20", dict(args=dict(out_stride=20))),
    ("offset_neg", dict(args=dict(out_offset=-1))),
    ("offset0_neg", dict(args=dict(out_offset0=-1))),
    ("offset1_neg", dict(args=dict(out_offset1=-1))),
    ("beams_0", dict(args=dict(n_beams=0, n_beams0=0))),
    ("beams_1025", dict(args=dict(n_beams=1025, n_beams0=1025, out_stride=2048))),
    ("beams_over_255", dict(args=dict(n_beams=256, n_beams0=250, out_stride=512))),
    ("beams1_0", dict(args=dict(n_beams1=0))),
    ("range_0", dict(args=dict(range=0.0, range0=0.0))),
    ("range_neg", dict(args=dict(range=-1.0, range0=-1.0))),
    ("range_nan", dict(args=dict(range=math.nan, range0=math.nan))),
    ("range1_0", dict(args=dict(range1=0.0))),
    ("draws_0", dict(args=dict(n_draws=0))),
    ("weights_misaligned", dict(args=dict(weights=MISALIGNED))),
    ("n_0", dict(args=dict(n=0))),
    ("nbytes_0", dict(args=dict(nbytes=0))),
    ("nbytes_8", dict(args=dict(nbytes=8))),
    ("dst_misaligned", dict(args=dict(dst=MISALIGNED))),
    ("src_misaligned", dict(args=dict(src=MISALIGNED))),
]

_STRUCTS = {"MdWorld": abi.MdWorld, "MdState": abi.MdState, "MdConfig": abi.MdConfig}


def _struct_of(ctype):
    m = re.match(r"(?:const\s+)?(Md\w+)\s*\*$", ctype)
    return m and _STRUCTS.get(m.group(1))


def _applies(decl, prof):
    names = {a for _, a in decl}
    if not prof:
        return True
    if "args" in prof:
        return bool(names & set(prof["args"]))
    return "c" in names


def _call(lib, name, decl, prof, dummy, null):
    """One call of `name` under profile `prof` with the pointers in `null` null."""
    keep = []
    args = []
    pargs = dict(BASE_ARGS, **prof.get("args", {}))
    for ctype, arg in decl:
        st = _struct_of(ctype)
        if st is not None:
            if arg in null:
                args.append(None)
                continue
            v = st()
            if st is abi.MdConfig:
                for k, x in dict(BASE_CONFIG, **prof.get("config", {})).items():
                    setattr(v, k, x)
            else:
                fields = [f for f, t in st._fields_ if t is abi.P]
                for f in fields:
                    setattr(v, f, None if "%s->%s" % (arg, f) in null else dummy)
                if st is abi.MdWorld:
                    for k, x in dict(BASE_WORLD, **prof.get("world", {})).items():
                        setattr(v, k, x)
            keep.append(v)
            args.append(C.addressof(v))
        elif arg == "stream":
            args.append(None)
        elif "*" in ctype:
            v = pargs.get(arg)
            args.append(None if arg in null else dummy + 4 if v == MISALIGNED else dummy)
        else:
            args.append(pargs[arg])
    fn = getattr(lib, name)
    rc = fn(*args)
    if rc == abi.MD_ELAUNCH:
        return "passed"
    return [rc, lib.md_last_error().decode()]


def _pointers(decl, st_null):
    """Every pointer an entry point reads: its pointer arguments (not the stream) and the pointer fields of its
    MdWorld / MdState arguments."""
    out = []
    for ctype, arg in decl:
        if arg == "stream" or "*" not in ctype:
            continue
        out.append(arg)
        st = _struct_of(ctype)
        if st in (abi.MdWorld, abi.MdState):
            out += ["%s->%s" % (arg, f) for f, t in st._fields_ if t is abi.P and "%s->%s" % (arg, f) not in st_null]
    return out


def open_lib(path):
    lib = C.CDLL(path)
    for name, decl in declarations().items():
        fn = getattr(lib, name)
        fn.restype = C.c_char_p if name == "md_last_error" else C.c_int
        fn.argtypes = [C.c_void_p if "*" in t else _CTYPES[t] for t, _ in decl]
    return lib


def dumps(res):
    """The fixture's text: one line per (entry, profile)."""
    lines = []
    for name, profs in res.items():
        body = ",\n".join("  %s: %s" % (json.dumps(p), json.dumps(r, sort_keys=True)) for p, r in profs.items())
        lines.append("%s: {\n%s\n}" % (json.dumps(name), body))
    return "{\n" + ",\n".join(lines) + "\n}\n"


def _required(p, r):
    return r == [abi.MD_EINVAL, "required pointer %s is null" % p]


def run(path):
    """{entry: {profile: outcomes}} of the library at `path`, where outcomes is "base" when they equal the entry's base
    profile's, else {"all": outcome with every pointer set, "required": the pointers refused alone with "required pointer
    <p> is null", in the order the library checks them, "null": {pointer: outcome} of the others whose nulling changes
    "all"}.  The order comes from nulling all required pointers and setting them back one by one as they are reported;
    if some other outcome interrupts that, it is "order_stop" and the rest of "required" is sorted.
    Only on a machine without a GPU (see the module docstring)."""
    lib = open_lib(path)
    buf = C.create_string_buffer(4096)
    dummy = (C.addressof(buf) + 15) & ~15
    res = {}
    for name, decl in declarations().items():
        if name in SKIP:
            continue
        res[name] = {}
        for pname, prof in PROFILES:
            if not _applies(decl, prof):
                continue
            null = set(prof.get("null", ()))
            out = dict(all=_call(lib, name, decl, prof, dummy, null))
            diff, req = {}, set()
            for p in _pointers(decl, null):
                r = _call(lib, name, decl, prof, dummy, null | {p})
                if _required(p, r):
                    req.add(p)
                elif r != out["all"]:
                    diff[p] = r
            order = []
            while req:
                r = _call(lib, name, decl, prof, dummy, null | req)
                p = next((p for p in req if _required(p, r)), None)
                if p is None:
                    out["order_stop"] = r
                    break
                order.append(p)
                req.remove(p)
            if order or req:
                out["required"] = order + sorted(req)
            if diff:
                out["null"] = diff
            res[name][pname] = "base" if pname != "base" and out == res[name]["base"] else out
    return res
