"""Who stores a slot at the end of a step of the lean non-staged workgroup kernels (include/md_write_back_own.h), on the host
(tests/write_back_own_host.c, the same text the library compiles).  EVERY combination of kind (all 16 values of the mask) x ALIVE x
STATIC x PENDING x AGENT x SPAWNED x removed-in-this-step, not a sample:

  - a slot that the write-back behind the last barrier stores (md_moves or removed: `dirty`) has an owner;
  - the three places that store -- wave 0 behind an agent's observe, an IDM wave behind a vehicle's decision, the last wave's rest
    pass -- never take the same slot, spelled here as csrc/mdstep.hip spells them: the IDM waves' rank walk deals out md_drives
    without AGENT, whatever the rule says, and must agree with it."""
import itertools

import numpy as np

import hostlib
from metadrive_ped_amd import abi

F_SPAWNED = 0x200


def _declare(lib):
    import ctypes as C
    lib.hx_wb_owner.restype = None
    lib.hx_wb_owner.argtypes = [C.c_int, C.c_void_p, C.c_void_p]
    lib.hx_wb_names.restype = None
    lib.hx_wb_names.argtypes = [C.c_void_p]


def _lib():
    return hostlib.build("write_back_own_host", _declare)


def _all_rows():
    rows = []
    for kind, alive, static, pending, agent, spawned, removed in itertools.product(range(16), *[(0, 1)] * 6):
        flags = kind | alive * abi.F_ALIVE | static * abi.F_STATIC | pending * abi.F_PENDING | agent * abi.F_AGENT | spawned * F_SPAWNED
        rows.append((flags, removed))
    return np.ascontiguousarray(rows, np.int32)


def _ask(rows):
    out = np.full((len(rows), 4), -7, np.int32)
    _lib().hx_wb_owner(len(rows), hostlib.ptr(rows), hostlib.ptr(out))
    names = np.zeros(4, np.int32)
    _lib().hx_wb_names(hostlib.ptr(names))
    assert len(set(names.tolist())) == 4
    return out, dict(zip(("nobody", "wave0", "idm", "rest"), names.tolist()))


def test_flag_bits_are_the_ones_enumerated():
    assert (abi.KIND_MASK, abi.F_ALIVE, abi.F_AGENT, abi.F_PENDING, abi.F_STATIC) == (0xF, 0x10, 0x20, 0x40, 0x80)


def test_every_dirty_slot_has_an_owner():
    rows = _all_rows()
    assert len(rows) == 16 * 64
    out, who = _ask(rows)
    owner, dirty, moves = out[:, 0], out[:, 1] != 0, out[:, 3] != 0
    assert set(owner.tolist()) == set(who.values()), "every answer occurs"
    assert (dirty == (moves | (rows[:, 1] != 0))).all(), "dirty: it moves or was removed, as the write-back behind the barrier asks"
    bad = rows[dirty & (owner == who["nobody"])]
    assert len(bad) == 0, "dirty slots without an owner: %r" % bad.tolist()
    # the superset is small: nobody stores a slot that is neither dirty nor driving
    assert not (~dirty & (owner != who["nobody"])).any()


def test_no_slot_has_two_owners():
    rows = _all_rows()
    out, who = _ask(rows)
    owner, drives = out[:, 0], out[:, 2] != 0
    agent = (rows[:, 0] & abi.F_AGENT) != 0
    for observed in (True, False):      # the slot is one of the agents_per_env that wave 0 observes, or lies beyond them
        wave0 = (owner == who["wave0"]) & observed
        idm = drives & ~agent                                               # the rank walk's ballot
        rest = (owner == who["rest"]) | ((owner == who["wave0"]) & (not observed))
        stores = wave0.astype(int) + idm.astype(int) + rest.astype(int)
        assert stores.max() == 1, "stored twice: %r" % rows[stores > 1].tolist()
        assert (stores[out[:, 1] != 0] == 1).all(), "a dirty slot is stored exactly once"
        assert (idm == (owner == who["idm"])).all(), "the rule and the rank walk name the same IDM slots"
    # a slot that an IDM wave is still planning is never the rest pass's, whatever its removed word holds
    assert not ((owner == who["rest"]) & drives).any()
