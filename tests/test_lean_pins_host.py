"""The launch predicate of md_step's lean kernels (include/md_lean_pins.h), on the host (tests/lean_pins_host.c, the same text the
library compiles): the lean pins alone choose between the lean kernels and the RESPAWN variant; the size pins -- one agent per env,
at most 64 mover slots -- join them for the narrow form of the lean non-staged kernel, and never send a lean batch anywhere else."""
import ctypes as C

import numpy as np

import hostlib


def _declare(lib):
    lib.hx_lean_pins.restype = None
    lib.hx_lean_pins.argtypes = [C.c_int, C.c_void_p, C.c_void_p]


def _ask(rows):
    rows = np.ascontiguousarray(rows, np.int32)
    out = np.full((len(rows), 3), -7, np.int32)
    hostlib.build("lean_pins_host", _declare).hx_lean_pins(len(rows), hostlib.ptr(rows), hostlib.ptr(out))
    return out


# (cap, agents_per_env) -> the size pins hold
SIZES = [((1, 1), True), ((8, 1), True), ((16, 1), True), ((24, 1), True), ((48, 1), True), ((63, 1), True), ((64, 1), True),
         ((65, 1), False), ((72, 1), False), ((128, 1), False),
         ((24, 2), False), ((64, 2), False), ((65, 2), False), ((24, 0), False), ((24, 40), False), ((128, 40), False)]
# (is_multi_agent, traffic_mode, agent_idm, num_others, detected set) -> the lean pins hold
PINS = [((0, 0, 0, 0, 0), True), ((1, 0, 0, 0, 0), False), ((0, 1, 0, 0, 0), False), ((0, 2, 0, 0, 0), False), ((0, 3, 0, 0, 0), False),
        ((0, 0, 1, 0, 0), False), ((0, 0, 2, 0, 0), False), ((0, 0, 0, 4, 0), False), ((0, 0, 0, 0, 1), False), ((0, 0, 0, 4, 1), False)]


def test_size_pins_join_the_lean_pins():
    rows, want = [], []
    for size, size_ok in SIZES:
        for pins, pins_ok in PINS:
            rows.append(size + pins)
            want.append((pins_ok, size_ok, pins_ok and size_ok))
    got = _ask(rows)
    for r, w, g in zip(rows, want, got.tolist()):
        assert tuple(bool(x) for x in g) == w and set(g) <= {0, 1}, "row %r: (lean, sizes, narrow) = %r, wanted %r" % (r, g, w)
    # the table holds every class: narrow, lean but wide, not lean at a narrow size, neither
    classes = {(w[0], w[1]) for w in want}
    assert classes == {(True, True), (True, False), (False, True), (False, False)}


def test_sizes_never_change_the_lean_answer():
    """a batch that holds the lean pins keeps a lean kernel at every size: the size pins only choose its form"""
    caps = list(range(1, 129))
    for agents in (1, 2):
        got = _ask([(cap, agents, 0, 0, 0, 0, 0) for cap in caps])
        assert (got[:, 0] == 1).all()
        assert got[:, 1].tolist() == [int(agents == 1 and cap <= 64) for cap in caps]
        assert (got[:, 2] == got[:, 1]).all()
