"""Device-side env snapshots (include/md_branch.h): env.snapshot() / env.restore() / env.branch() of every batched env family
(envs/base.py), the opaque EnvSnapshot they pass around, the checks both share, and apply_host -- the numpy restatement of one
md_branch launch that the tests and the oracle comparison use.

What travels with an env is every per-env row of every MdState array the batch has (the table MD_BRANCH_FIELDS of the header, read
here as text: a snapshot's storage is sized from it), MdWorld.env_map[e], the top-down history and image, the AIProtect takeover
bytes, the staged-draw index and the env's scenario seed.  What does not: the lidar-noise and expert-noise generators (one stream
per batch, not per env), the viewer's render history and a recording buffer."""
import ctypes as C
import os
import re

import numpy as np

from metadrive_ped_amd import abi

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "md_branch.h")
UNITS = ("MD_BR_SLOT", "MD_BR_AGENT", "MD_BR_ENV")
SCALES = ("MD_BR_ONE", "MD_BR_OBS_DIM", "MD_BR_SEG_CAP", "MD_BR_VERT_CAP")
# per-env arrays of the host state that are arguments of other entry points, not MdState fields: name -> bytes per env
EXTRA_STATE_ROWS = {"takeover": 1, "expert_takeover": 1}
_TABLE = None


def read_table():
    """-> (fields, not_per_env) of include/md_branch.h: fields = [(MdState field, unit, bytes per unit, scale)] in the header's
    order, unit / scale as the names in UNITS / SCALES; not_per_env = the pointer fields that hold no per-env rows."""
    global _TABLE
    if _TABLE is None:
        with open(HEADER) as fh:
            src = re.sub(r"/\*.*?\*/", "", fh.read(), flags=re.S)
        fields = [(n, u, int(b), s) for n, u, b, s in re.findall(r"^\s*X\((\w+),\s*(\w+),\s*(\d+),\s*(\w+)\)", src, flags=re.M)]
        rest = re.findall(r"^\s*Y\((\w+)\)", src, flags=re.M)
        if not fields or any(u not in UNITS or s not in SCALES for _, u, _, s in fields):
            raise RuntimeError("{}: the table of per-env extents could not be read".format(HEADER))
        _TABLE = (fields, rest)
    return _TABLE


def row_bytes(unit, nbytes, scale, cap, agents, obs_dim, seg_cap=0, vert_cap=0):
    """md_branch_row_bytes: bytes of one env's row of a field of the table"""
    units = {"MD_BR_SLOT": cap, "MD_BR_AGENT": agents, "MD_BR_ENV": 1}[unit]
    mul = {"MD_BR_ONE": 1, "MD_BR_OBS_DIM": obs_dim, "MD_BR_SEG_CAP": seg_cap, "MD_BR_VERT_CAP": vert_cap}[scale]
    return int(units) * int(nbytes) * int(mul)


def field_rows(cap, agents, obs_dim, seg_cap=0, vert_cap=0):
    """{MdState field: bytes per env} for a batch of these sizes"""
    return {n: row_bytes(u, b, s, cap, agents, obs_dim, seg_cap, vert_cap) for n, u, b, s in read_table()[0]}


# -- index arguments: host integers or sequences, checked without touching the device.  Everything here is numpy on whole index
#    arrays: a call on 4096 envs must cost far less than the launch it prepares ------------------------------------------------------
def as_indices(x, what):
    """One host integer or a sequence of them (list, tuple, range, numpy) -> 1-D int64 array.  Device tensors are refused:
    reading them would synchronise."""
    if hasattr(x, "device") and hasattr(x, "data_ptr"):
        raise TypeError("{} must be host integers (an int, list, tuple or numpy array), not a tensor: the indices are checked on the "
                        "host without a sync".format(what))
    if isinstance(x, range):
        return np.arange(x.start, x.stop, x.step, dtype=np.int64)
    a = np.asarray(x)
    if a.size == 0 and a.ndim == 1:
        return np.zeros(0, np.int64)
    if a.dtype == bool or not np.issubdtype(a.dtype, np.integer) or a.ndim > 1:
        raise TypeError("{} must be an integer or a 1-D sequence of integers, got {!r}".format(what, x))
    return a.reshape(-1).astype(np.int64, copy=False)


def pair_key(x):
    """A cheap hashable name of an index argument, or None where making one would cost as much as checking it: the envs keep
    the latest checked pair lists under these, so that a rollout loop that names the same envs again checks nothing twice."""
    if x is None or isinstance(x, (int, np.integer)):
        return ("i", None if x is None else int(x))
    if isinstance(x, range):
        return ("r", x.start, x.stop, x.step)
    if isinstance(x, np.ndarray) and x.ndim == 1 and x.dtype != bool and np.issubdtype(x.dtype, np.integer):
        return ("a", x.dtype.str, x.tobytes())
    if isinstance(x, (list, tuple)) and len(x) <= 64 and all(isinstance(v, (int, np.integer)) and not isinstance(v, bool) for v in x):
        return ("t", tuple(int(v) for v in x))
    return None


def check_range(idx, n, what, noun="env"):
    bad = (idx < 0) | (idx >= n)
    if bad.any():
        raise ValueError("{}: {} {} is out of range [0, {})".format(what, noun, int(idx[np.argmax(bad)]), n))


def check_distinct(idx, n, what):
    """idx within [0, n) already"""
    count = np.bincount(idx, minlength=n)
    if count.size and count.max() > 1:
        raise ValueError("{}: env {} is named twice; every destination env takes one row".format(what, int(np.argmax(count > 1))))


def check_branch_pairs(src, dst, n_envs):
    """env.branch(src, dst) -> (src, dst) index arrays of equal length; ValueError names the offending env"""
    s, d = as_indices(src, "src"), as_indices(dst, "dst")
    if d.size == 0:
        raise ValueError("branch: dst names no env")
    if s.size == 1 and np.ndim(src) == 0:
        s = np.full(d.size, s[0], np.int64)
    if s.size != d.size:
        raise ValueError("branch: src must be one env or as many envs as dst ({} != {})".format(s.size, d.size))
    check_range(s, n_envs, "branch: src")
    check_range(d, n_envs, "branch: dst")
    check_distinct(d, n_envs, "branch: dst")
    is_dst = np.zeros(n_envs, bool)
    is_dst[d] = True
    both = is_dst[s]
    if both.any():
        raise ValueError("branch: env {} is both a source and a destination; the pairs are copied concurrently".format(int(s[both].min())))
    return s, d


def check_restore_pairs(snap, envs, rows, n_envs):
    """env.restore(snap, envs, rows) -> (rows, envs) index arrays: snapshot row rows[i] goes to env envs[i].  Defaults: every row
    (a one-row snapshot: that row for every env named), to the envs the rows came from."""
    e = None if envs is None else as_indices(envs, "envs")
    if rows is None:
        n = snap.num_envs if e is None else e.size
        if snap.num_envs == 1:
            r = np.zeros(max(n, 1), np.int64)
        elif n != snap.num_envs:
            raise ValueError("restore: {} envs named for a snapshot of {} rows; say which with rows=".format(n, snap.num_envs))
        else:
            r = np.arange(snap.num_envs, dtype=np.int64)
    else:
        r = as_indices(rows, "rows")
    check_range(r, snap.num_envs, "restore: rows", noun="snapshot row")
    if e is None:
        e = snap._source[r]
    if r.size == 1 and e.size > 1:
        r = np.full(e.size, r[0], np.int64)
    if e.size == 0 or e.size != r.size:
        raise ValueError("restore: {} rows for {} envs".format(r.size, e.size))
    check_range(e, n_envs, "restore: envs")
    check_distinct(e, n_envs, "restore: envs")
    return r, e


# -- scope -------------------------------------------------------------------------------------------------------------------------
def staged_draws(config):
    """BatchedEngine.n_traffic_draws from the config alone"""
    if config.get("scenario_mode") or config["is_multi_agent"] or not (config["random_traffic"] and config["auto_reset"]):
        return 1
    return max(1, int(config.get("traffic_draws", 1)))


def check_scope(config, what, engine=None):
    """The configurations snapshots are not built for, refused by the option's name (NotImplementedError)"""
    if config.get("scenario_mode"):
        raise NotImplementedError("{}: BatchedScenarioEnv (scenario_mode) is not built: its per-scene tables are indexed by scene, "
                                  "not reached through env_map alone".format(what))
    if config.get("walk_scenarios"):
        raise NotImplementedError("{} with walk_scenarios=True is not built: the walk's position belongs to the env's worker".format(what))
    if config.get("traffic_mode") == "replay" or (engine is not None and engine._tracks is not None):
        raise NotImplementedError("{} with traffic_mode='replay' / loaded tracks is not built: the recorded frames are indexed by "
                                  "env".format(what))
    if engine is not None and engine._rec is not None:
        raise NotImplementedError("{} while a recording is running (start_recording) is not built: the recorded frames would mix "
                                  "two histories; stop_recording() first".format(what))


def check_staged_draws(config, pairs, what):
    """random_traffic with more than one staged draw: the pool is indexed by env, so a row may only go back to the env it came
    from.  pairs = (source envs, destination envs), two index arrays."""
    if staged_draws(config) > 1:
        src, dst = np.asarray(pairs[0]), np.asarray(pairs[1])
        moved = src != dst
        if moved.any():
            i = int(np.argmax(moved))
            raise NotImplementedError("{}: random_traffic with traffic_draws={} stages the draws per env; env {}'s state cannot "
                                      "go to env {} (its next auto-reset would take a draw built for another map)".format(
                                          what, staged_draws(config), int(src[i]), int(dst[i])))


def batch_signature(family, cap, agents, obs_dim, topdown=None, arrays=()):
    """What a snapshot and a batch must share: the env class family, the mover capacity, agents per env, obs_dim, the ABI version,
    the top-down sizes (None without the top-down observation) and the names of the arrays that travel."""
    return (str(family), int(cap), int(agents), int(obs_dim), abi.MD_ABI_VERSION, None if topdown is None else tuple(topdown),
            tuple(arrays))


class EnvSnapshot:
    """A device-resident copy of chosen envs of a batch, made by env.snapshot().  Opaque: hand it to env.restore().  It stays valid
    across step() and a plain reset(); reset(seed=...), a rebuild of the engine and close() invalidate it."""
    def __init__(self, source_envs, seeds, signature, token, storage=None, state=None, extras=None, nbytes=0, owner=None):
        self._source = np.asarray(source_envs, np.int64).reshape(-1)      # the env each row came from
        self._seeds = np.asarray(seeds, np.int64).reshape(-1)             # and the scenario seed it played
        self.batch_signature = signature
        self.nbytes = int(nbytes)
        self._token = token          # the engine build the rows belong to
        self._owner = owner          # names the engine itself, whatever its build
        self._storage = storage      # ONE uint8 device tensor
        self._state = state          # abi.MdState over the storage
        self._extras = extras or {}  # name -> (address, bytes per env)

    @property
    def num_envs(self):
        return int(self._source.size)

    @property
    def source_envs(self):
        return tuple(self._source.tolist())

    @property
    def seeds(self):
        return tuple(self._seeds.tolist())

    def __repr__(self):
        return "EnvSnapshot(num_envs={}, nbytes={})".format(self.num_envs, self.nbytes)


def check_snapshot(snap, signature, token, what="restore", owner=None):
    """ValueError unless `snap` fits the batch (signature) and belongs to this build of it (token).  A snapshot of this very
    engine (owner) from before a rebuild is reported as invalidated even where the rebuild also changed the batch's sizes."""
    if not isinstance(snap, EnvSnapshot):
        raise TypeError("{}: expected an EnvSnapshot from env.snapshot(), got {!r}".format(what, type(snap).__name__))
    stale = snap._token is None or snap._token is not token
    if snap.batch_signature != signature and not (stale and owner is not None and snap._owner is owner):
        raise ValueError("{}: the snapshot was taken from another kind of batch (env family, mover capacity, agents per env, obs_dim, "
                         "ABI version, top-down sizes, arrays): {} != {}".format(what, snap.batch_signature, signature))
    if stale:
        raise ValueError("{}: the snapshot is no longer valid: reset(seed=...), a rebuild of the engine or close() came after "
                         "it".format(what))


def layout(present, extras, n_rows):
    """The storage of an n_rows snapshot: {name: (offset, bytes per env)} for the MdState fields `present` ({field: bytes per env})
    and the extras ([(name, bytes per env)]), every part 16-byte aligned -> (state offsets, extra offsets, total bytes)"""
    at, st, ex = 0, {}, {}
    for name, rb in present.items():
        st[name] = (at, rb)
        at = (at + n_rows * rb + 15) // 16 * 16
    for name, rb in extras:
        ex[name] = (at, rb)
        at = (at + n_rows * rb + 15) // 16 * 16
    return st, ex, max(at, 16)


def fill_branch(src_ptr, dst_ptr, n_pairs, src_n, dst_n, extras):
    """abi.MdBranch of one launch; extras = [(dst address, src address, bytes per env)]"""
    if len(extras) > abi.MD_BR_MAX_EXTRAS:
        raise ValueError("md_branch: {} extra arrays, the table holds {}".format(len(extras), abi.MD_BR_MAX_EXTRAS))
    b = abi.MdBranch()
    b.struct_size, b.n_pairs, b.src_n_envs, b.dst_n_envs, b.n_extras = C.sizeof(abi.MdBranch), n_pairs, src_n, dst_n, len(extras)
    b.src_row, b.dst_row = src_ptr, dst_ptr
    for k, (d, s, rb) in enumerate(extras):
        b.extra[k].dst, b.extra[k].src, b.extra[k].row_bytes = d, s, rb
    return b


# -- the numpy restatement ---------------------------------------------------------------------------------------------------------
def _rows(a, n):
    b = a.view(np.uint8).reshape(-1)
    assert b.size % n == 0, (a.shape, n)
    return b.reshape(n, b.size // n)


def apply_host(state, env_map, pairs, src_state=None):
    """One md_branch launch on host arrays, in place: for every (source row, destination row) of `pairs`, the row of every per-env
    array of `src_state` (None: `state` itself, an env -> env branch) goes to the row of `state`, and env_map likewise (from
    src_state["env_map"] when the source is another state and has one).  `state`: a dict of C-contiguous numpy arrays keyed like
    HostScene.state; an array missing on either side is skipped, like a NULL field.  Row counts come from need_reset."""
    fields = {n for n, _, _, _ in read_table()[0]} | set(EXTRA_STATE_ROWS)
    src = state if src_state is None else src_state
    n_dst, n_src = state["need_reset"].size, src["need_reset"].size
    pairs = [(int(s), int(d)) for s, d in pairs]
    for s, d in pairs:
        if not (0 <= s < n_src and 0 <= d < n_dst):
            raise ValueError("apply_host: pair ({}, {}) is out of range".format(s, d))
    for k in state:
        if k not in fields or src.get(k) is None or state[k] is None:
            continue
        dv, sv = _rows(state[k], n_dst), _rows(src[k], n_src)
        taken = sv[[s for s, _ in pairs]].copy()
        dv[[d for _, d in pairs]] = taken
    src_map = env_map if src_state is None else src.get("env_map")
    if env_map is not None and src_map is not None:
        taken = np.asarray(src_map)[[s for s, _ in pairs]].copy()
        env_map[[d for _, d in pairs]] = taken
    return state
