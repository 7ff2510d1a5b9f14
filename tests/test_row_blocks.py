"""abi.row_blocks, the ONE layout of the side features' per-env rows ("Per-env row blocks"): the four *_blocks functions
against tables recorded from the copy-and-paste versions they replace (tests/golden/row_blocks.json: name order, offset, shape,
dtype and row bytes, for the default configs, the tests' small shapes, the ceilings and the zero-count configs), and the rule itself
on the helpers beside it.  CPU only, no library."""
import json
import os

import numpy as np
import pytest

import hostlib
from metadrive_ped_amd import abi

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "row_blocks.json")) as fh:
    CASES = json.load(fh)
f4, i4, u1 = np.float32, np.int32, np.uint8


def _tables(result):
    """(table, row bytes, ...) as the *_blocks functions return them -> the pairs"""
    return list(zip(result[0::2], result[1::2]))


@pytest.mark.parametrize("case", CASES, ids=["{}-{}".format(c["fn"], c["label"]) for c in CASES])
def test_blocks_as_recorded(case):
    got = getattr(abi, case["fn"])(case["cfg"], *case["args"])
    assert len(got) == len(case["result"])
    for (table, row_bytes), (want, want_bytes) in zip(_tables(got), _tables(case["result"])):
        assert [[name, off, list(shape), dt.str] for name, (off, shape, dt) in table.items()] == want
        assert all(isinstance(dt, np.dtype) for _, _, dt in table.values())
        assert row_bytes == want_bytes


def test_recorded_configs():
    """the configurations the record has to hold"""
    import scenario_vector_obs_host as sh
    import vector_obs_host as vh
    from metadrive_ped_amd import config
    have = {(c["fn"], json.dumps(c["cfg"], sort_keys=True), tuple(c["args"])) for c in CASES}
    key = lambda fn, cfg, keys, *args: (fn, json.dumps({k: int(cfg[k]) for k in keys}, sort_keys=True), args)
    vo, svo = sorted(vh.SMALL), sorted(sh.SMALL)
    assert key("vector_obs_blocks", config.VECTOR_OBS_DEFAULT_CONFIG, vo, 1, 8) in have
    assert key("vector_obs_blocks", vh.SMALL, vo, 1, 8) in have and key("vector_obs_blocks", vh.SMALL, vo, 2, 8) in have
    assert key("vector_obs_blocks", dict(vh.SMALL, route_points=0), vo, 2, 8) in have
    assert key("vector_obs_blocks", dict(vh.SMALL, num_lanes=0), vo, 2, 8) in have
    assert key("scenario_vector_obs_blocks", config.SCENARIO_VECTOR_OBS_DEFAULT_CONFIG, svo, 8) in have
    assert key("scenario_vector_obs_blocks", sh.SMALL, svo, 8) in have and key("scenario_vector_obs_blocks", sh.CEILINGS, svo, 8) in have
    assert key("scenario_vector_obs_blocks", dict(sh.SMALL, route_points=0), svo, 8) in have
    assert key("scenario_vector_obs_blocks", dict(sh.SMALL, num_pieces=0), svo, 8) in have
    assert key("traffic_lights_blocks", config.TRAFFIC_LIGHTS_DEFAULT_CONFIG, ["num_lights"]) in have
    assert key("traffic_lights_blocks", dict(num_lights=0), ["num_lights"]) in have
    assert key("scenario_metrics_blocks", config.SCENARIO_METRICS_DEFAULT_CONFIG, ["ttc_samples"]) in have


# an odd byte count, a zero-count block in the middle and one at the end, an item size of 1 behind one of 4, a scalar
BLOCKS = [("a", (3, 5), f4), ("m", (3, ), u1), ("none", (0, 4), f4), ("i", (2, 3), i4), ("one", (), u1), ("tail", (7, 0), u1)]


def test_row_blocks_rule():
    table, row_bytes = abi.row_blocks(BLOCKS)
    assert list(table) == [name for name, _, _ in BLOCKS]
    assert {name: off for name, (off, _, _) in table.items()} == dict(a=0, m=64, none=80, i=80, one=112, tail=128)
    assert row_bytes == 128
    assert all(off % 16 == 0 for off, _, _ in table.values()) and row_bytes % 16 == 0
    for (name, shape, dt), (off, got_shape, got_dt) in zip(BLOCKS, table.values()):
        assert got_shape == shape and got_dt == np.dtype(dt) and abi.block_bytes(table, name) == int(np.prod(shape)) * np.dtype(dt).itemsize
    offs = [off for off, _, _ in table.values()] + [row_bytes]
    for at, name in enumerate(table):       # a zero-count block has no bytes and shares its offset with its successor
        assert (offs[at + 1] == offs[at]) == (abi.block_bytes(table, name) == 0)
    assert abi.row_blocks([]) == ({}, 0)


@pytest.mark.parametrize("case", CASES, ids=["{}-{}".format(c["fn"], c["label"]) for c in CASES])
def test_every_table_keeps_the_rule(case):
    for table, row_bytes in _tables(getattr(abi, case["fn"])(case["cfg"], *case["args"])):
        end = 0
        for name, (off, shape, dt) in table.items():
            assert off % 16 == 0 and off == (end + 15) // 16 * 16
            end = off + abi.block_bytes(table, name)
        assert row_bytes % 16 == 0 and row_bytes == (end + 15) // 16 * 16


def test_block_ptrs_omits_the_empty_blocks():
    table, _ = abi.row_blocks(BLOCKS)
    base = 0x7f0000001000
    assert abi.block_ptrs(table, base) == {"a": base, "m": base + 64, "i": base + 80, "one": base + 112}
    rows = hostlib.HostRows(table, 128, 2)
    assert rows.ptrs() == abi.block_ptrs(table, rows.rows.ctypes.data)


@pytest.mark.parametrize("E", [2, 1])       # E = 1: a one-row slice is contiguous as it is, and block_of still returns a copy
def test_block_round_trip(E):
    """block_of -> HostRows.set -> block_of: exact for the f4, i4 and u1 blocks, and no byte outside the block moves"""
    table, row_bytes = abi.row_blocks(BLOCKS)
    rng = np.random.RandomState(7)
    rows = hostlib.HostRows(table, row_bytes, E)
    rows.rows[:] = rng.randint(0, 256, rows.rows.shape)
    for name in ("a", "i", "m", "one", "none"):
        off, shape, dt = table[name]
        before = rows.rows.copy()
        was = abi.block_of(rows.rows, table, name)
        assert was.shape == (E, ) + shape and was.dtype == dt
        value = rng.randint(0, 256, (E, abi.block_bytes(table, name))).astype(u1).view(dt).reshape((E, ) + shape)
        rows.set(name, value)
        got = rows.out(name)
        assert got.tobytes() == value.tobytes() and got.shape == value.shape and got.dtype == dt
        untouched = np.ones(row_bytes, bool)
        untouched[off:off + abi.block_bytes(table, name)] = False
        assert (rows.rows[:, untouched] == before[:, untouched]).all()
        rows.set(name, was)
        assert (rows.rows == before).all()
        got[...] = 0                                 # a copy: the rows do not follow it
        assert (rows.rows == before).all()
