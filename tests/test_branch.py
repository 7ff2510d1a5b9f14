"""Device-side env snapshots without a GPU (include/md_branch.h, metadrive_ped_amd/branch.py): the one table of per-env extents
against md_env_view and the fields of MdState, the host-built C copy against the numpy restatement apply_host, a branched oracle
run against one that was never branched, and the checks of env.snapshot() / restore() / branch() that need no device."""
import ctypes as C
import types

import numpy as np
import pytest

import hostlib
from helpers import scripted_actions
from metadrive_ped_amd import abi, branch


def _declare(lib):
    lib.hx_field_name.restype = C.c_char_p
    lib.hx_not_per_env_name.restype = C.c_char_p
    lib.hx_field_offset.restype = C.c_longlong
    lib.hx_field_row_bytes.restype = C.c_longlong
    lib.hx_field_row_bytes.argtypes = [C.POINTER(abi.MdConfig), C.c_int]
    lib.hx_env_view.argtypes = [C.POINTER(abi.MdState), C.POINTER(abi.MdConfig), C.c_int, C.POINTER(abi.MdState)]
    lib.hx_branch.argtypes = [C.POINTER(abi.MdState), C.POINTER(abi.MdState), C.POINTER(abi.MdConfig), C.POINTER(abi.MdBranch)]


def _lib():
    return hostlib.build("branch_host", _declare)


def _config(E, A, cap, obs_dim, seg_cap=0, vert_cap=0):
    k = abi.MdConfig()
    k.struct_size = C.sizeof(abi.MdConfig)
    k.n_envs, k.agents_per_env, k.cap, k.obs_dim, k.route_seg_cap, k.route_vert_cap = E, A, cap, obs_dim, seg_cap, vert_cap
    return k


# -- 1. the table ------------------------------------------------------------------------------------------------------------------
def test_every_state_field_is_in_the_table_or_listed_as_not_per_env():
    fields, rest = branch.read_table()
    names = [n for n, _, _, _ in fields]
    assert len(set(names)) == len(names) and not set(names) & set(rest)
    assert sorted(names + rest) == sorted(abi.STATE_FIELDS)
    lib = _lib()      # the C compiler reads the same table as branch.py does
    assert [lib.hx_field_name(i).decode() for i in range(lib.hx_n_fields())] == names
    assert [lib.hx_not_per_env_name(i).decode() for i in range(lib.hx_n_not_per_env())] == rest
    offsets = {f: getattr(abi.MdState, f).offset for f in abi.STATE_FIELDS}
    assert [lib.hx_field_offset(i) for i in range(lib.hx_n_fields())] == [offsets[n] for n in names]


def test_the_table_gives_the_offsets_md_env_view_applies():
    lib = _lib()
    E, A, cap, obs_dim, seg_cap, vert_cap = 3, 2, 5, 23, 6, 9
    k = _config(E, A, cap, obs_dim, seg_cap, vert_cap)
    rows = branch.field_rows(cap, A, obs_dim, seg_cap, vert_cap)
    g = abi.MdState()
    for i, f in enumerate(abi.STATE_FIELDS):      # small fake base addresses: md_env_view only advances them ...
        setattr(g, f, 0x100000 * (i + 1))
    scene_of = np.arange(E, dtype=np.int32)        # ... except scene_of, which it reads
    g.scene_of = scene_of.ctypes.data
    for i, (name, _, _, _) in enumerate(branch.read_table()[0]):
        assert lib.hx_field_row_bytes(C.byref(k), i) == rows[name], name
    for e in range(E):
        v = abi.MdState()
        lib.hx_env_view(C.byref(g), C.byref(k), e, C.byref(v))
        for name, rb in rows.items():
            assert getattr(v, name) - getattr(g, name) == e * rb, (name, e)


# -- 2. the host-built C copy against apply_host -----------------------------------------------------------------------------------
ABSENT = ("detected", "idle_ring")      # left NULL: skipped like copy_draw_rows does


def _random_state(rng, n, A, cap, obs_dim):
    st = {name: rng.randint(0, 256, size=n * rb).astype(np.uint8) for name, rb in branch.field_rows(cap, A, obs_dim).items()
          if rb > 0 and name not in ABSENT}
    st["need_reset"] = st["need_reset"].view(np.int32)
    st["takeover"] = rng.randint(0, 2, size=n).astype(np.uint8)      # a 1-byte extra
    return st


def _c_branch(lib, k, dst, dst_map, pairs, src=None, src_map=None):
    """hx_branch of `pairs` on copies of the host arrays -> (state, env_map)"""
    dst = {n: a.copy() for n, a in dst.items()}
    dst_map = dst_map.copy()
    src_d, src_m = (dst, dst_map) if src is None else (src, src_map)
    structs = []
    for d in (dst, src_d):
        s = abi.MdState()
        abi.fill_struct(s, abi.STATE_FIELDS, d, hostlib.ptr)
        structs.append(s)
    idx = np.ascontiguousarray(np.asarray(pairs, np.int32).T)
    extras = [(hostlib.ptr(dst["takeover"]), hostlib.ptr(src_d["takeover"]), 1), (hostlib.ptr(dst_map), hostlib.ptr(src_m), 4)]
    b = branch.fill_branch(hostlib.ptr(idx[0]), hostlib.ptr(idx[1]), len(pairs), src_d["need_reset"].size, dst["need_reset"].size, extras)
    assert lib.hx_branch(C.byref(structs[0]), C.byref(structs[1]), C.byref(k), C.byref(b)) == 0
    return dst, dst_map


@pytest.mark.parametrize("cap,A,obs_dim", [(1, 1, 19), (7, 1, 259), (7, 3, 19), (7, 3, 259)])
def test_host_copy_equals_the_numpy_restatement(cap, A, obs_dim):
    lib = _lib()
    E = 5
    rng = np.random.RandomState(cap * 1000 + A * 100 + obs_dim)
    k = _config(E, A, cap, obs_dim)
    base, base_map = _random_state(rng, E, A, cap, obs_dim), rng.randint(0, 9, size=E).astype(np.int32)
    small, small_map = _random_state(rng, 3, A, cap, obs_dim), rng.randint(0, 9, size=3).astype(np.int32)
    perm = rng.permutation(E)
    cases = [("fan-out", [(3, d) for d in (0, 1, 2, 4)], None),            # an odd source, odd and even destinations
             ("split permutation", [(int(perm[0]), int(perm[2])), (int(perm[1]), int(perm[3]))], None),
             ("single pair", [(1, 4)], None), ("single pair, odd destination", [(2, 3)], None),
             ("another row count", [(1, 3), (2, 0), (0, 4)], (small, small_map))]     # src_n_envs = 3, dst_n_envs = 5
    for what, pairs, other in cases:
        src, src_map = other if other is not None else (None, None)
        got, got_map = _c_branch(lib, k, base, base_map, pairs, src, src_map)
        want, want_map = {n: a.copy() for n, a in base.items()}, base_map.copy()
        branch.apply_host(want, want_map, pairs, None if src is None else dict(src, env_map=src_map))
        assert sorted(got) == sorted(want)
        taken = [d for _, d in pairs]
        kept = [e for e in range(E) if e not in taken]
        for name in list(want) + ["env_map"]:
            g, w, b0 = (got_map, want_map, base_map) if name == "env_map" else (got[name], want[name], base[name])
            assert g.tobytes() == w.tobytes(), (what, name)
            rows = lambda a: a.view(np.uint8).reshape(E, -1)
            assert np.array_equal(rows(g)[kept], rows(b0)[kept]), (what, name, "rows not named were touched")
            from_rows = rows(b0) if src is None else (src_map if name == "env_map" else src[name]).view(np.uint8).reshape(3, -1)
            assert np.array_equal(rows(g)[taken], from_rows[[s for s, _ in pairs]]), (what, name)


def test_apply_host_refuses_a_pair_out_of_range():
    st = _random_state(np.random.RandomState(0), 2, 1, 1, 19)
    with pytest.raises(ValueError):
        branch.apply_host(st, np.zeros(2, np.int32), [(0, 2)])


# -- 3. a branched oracle run ------------------------------------------------------------------------------------------------------
def test_branched_envs_continue_like_their_source_on_the_oracle():
    import oracle_binding as ob
    from metadrive_ped_amd.config import make_config
    from metadrive_ped_amd.engine import HostScene
    host = HostScene(make_config(dict(num_envs=4, num_scenarios=4, map="SC", traffic_density=0.15, horizon=25)))
    E, A = 4, 1
    keys = ("obs", "reward", "flags", "done_out")
    rows = lambda st, k: st[k].view(np.uint8).reshape(E, -1)

    def actions(t):
        return scripted_actions(E, A, t) if t < 10 else np.broadcast_to(scripted_actions(1, A, t), (E, A, 2)).copy()

    plain = ob.OracleWorld(host)
    plain.reset()
    want = []
    for t in range(50):
        plain.step(actions(t))
        want.append({k: rows(plain.state, k)[2].copy() for k in keys})

    o = ob.OracleWorld(host)
    env_map = host.world.arrays["env_map"].copy()      # the branched run's own copy: the scene's table stays as built
    o.w.env_map = env_map.ctypes.data
    o.reset()
    for t in range(10):
        o.step(actions(t))
    assert len(set(env_map.tolist())) == 4
    branch.apply_host(o.state, env_map, [(2, 0), (2, 1), (2, 3)])
    assert env_map.tolist() == [env_map[2]] * 4
    resets = 0
    for t in range(10, 50):
        o.step(actions(t))
        resets += int(o.state["need_reset"].any())
        for k in keys:
            r = rows(o.state, k)
            assert all(np.array_equal(r[e], r[2]) for e in range(E)), (t, k)
            assert np.array_equal(r[2], want[t][k]), (t, k, "env 2 differs from the run that was never branched")
    assert resets >= 1, "the run must pass a truncation and an auto-reset"


# -- 4. the checks that need no device ---------------------------------------------------------------------------------------------
def _env(**kw):
    from metadrive_ped_amd.envs import BatchedMetaDriveEnv
    return BatchedMetaDriveEnv(dict(dict(num_envs=4, num_scenarios=4, map="SC"), **kw))


def _snapshot(n=2, signature=("pg", 8, 1, 259, 12, None, ()), token=None):
    return branch.EnvSnapshot(list(range(1, n + 1)), [100 + e for e in range(n)], signature, token)


def test_index_errors_name_the_env():
    env = _env()
    for call, text in ((lambda: env.branch(4, [0]), "env 4 is out of range"), (lambda: env.branch(0, [1, -1]), "env -1 is out of range"),
                       (lambda: env.branch(0, [1, 2, 1]), "env 1 is named twice"), (lambda: env.branch(2, [1, 2]), "env 2 is both"),
                       (lambda: env.branch([0, 1], [2, 0]), "env 0 is both"), (lambda: env.branch([0, 1], [2]), "as many envs as dst"),
                       (lambda: env.branch(0, []), "names no env"), (lambda: env.snapshot([0, 7]), "env 7 is out of range"),
                       (lambda: env.snapshot([3, 3]), "env 3 is named twice"),
                       (lambda: env.restore(_snapshot(), envs=[0, 4]), "env 4 is out of range"),
                       (lambda: env.restore(_snapshot(), envs=[2, 2]), "env 2 is named twice"),
                       (lambda: env.restore(_snapshot(), rows=[2]), "snapshot row 2 is out of range"),
                       (lambda: env.restore(_snapshot(), envs=[0, 1, 2]), "say which with rows=")):
        with pytest.raises(ValueError) as err:
            call()
        assert text in str(err.value), (text, str(err.value))
    with pytest.raises(TypeError):
        env.branch(0, [1.5])
    with pytest.raises(TypeError):
        env.restore("not a snapshot")
    # the indices are fine: what is missing is the engine
    with pytest.raises(RuntimeError):
        env.branch(0, [1, 2, 3])
    with pytest.raises(RuntimeError):
        env.snapshot(np.asarray([0, 2]))
    with pytest.raises(ValueError) as err:
        env.restore(_snapshot())
    assert "no longer valid" in str(err.value)


def test_restore_pairs_defaults():
    two, one = _snapshot(2), _snapshot(1)
    pairs = lambda got: tuple(x.tolist() for x in got)
    assert pairs(branch.check_restore_pairs(two, None, None, 4)) == ([0, 1], [1, 2])          # back where the rows came from
    assert pairs(branch.check_restore_pairs(two, [3, 0], None, 4)) == ([0, 1], [3, 0])
    assert pairs(branch.check_restore_pairs(two, [3], [1], 4)) == ([1], [3])
    assert pairs(branch.check_restore_pairs(one, [0, 2, 3], None, 4)) == ([0, 0, 0], [0, 2, 3])   # a one-row snapshot broadcasts
    assert pairs(branch.check_restore_pairs(two, (0, 3), (1, ), 4)) == ([1, 1], [0, 3])
    assert pairs(branch.check_branch_pairs(3, range(0, 3), 4)) == ([3, 3, 3], [0, 1, 2])
    assert pairs(branch.check_branch_pairs(np.int64(1), np.asarray([0]), 4)) == ([1], [0])
    assert pairs(branch.check_branch_pairs([2, 3], (1, 0), 4)) == ([2, 3], [1, 0])
    assert (two.num_envs, two.source_envs, two.seeds) == (2, (1, 2), (100, 101))


def test_out_of_scope_configurations_are_refused_by_name():
    for cfg, text in ((dict(walk_scenarios=True), "walk_scenarios=True"), (dict(traffic_mode="replay"), "traffic_mode='replay'")):
        env = _env(**cfg)
        for call in (lambda: env.snapshot(), lambda: env.branch(0, [1]), lambda: env.restore(_snapshot())):
            with pytest.raises(NotImplementedError) as err:
                call()
            assert text in str(err.value)
    with pytest.raises(NotImplementedError) as err:
        branch.check_scope(dict(scenario_mode=True), "snapshot")
    assert "BatchedScenarioEnv" in str(err.value)
    cfg = _env().config
    with pytest.raises(NotImplementedError) as err:
        branch.check_scope(cfg, "branch", types.SimpleNamespace(_tracks=None, _rec=dict(n=0)))
    assert "recording" in str(err.value)
    with pytest.raises(NotImplementedError) as err:
        branch.check_scope(cfg, "branch", types.SimpleNamespace(_tracks=dict(), _rec=None))
    assert "loaded tracks" in str(err.value)
    branch.check_scope(cfg, "branch", types.SimpleNamespace(_tracks=None, _rec=None))
    # random_traffic with several staged draws: a row may only go back to the env it came from
    env = _env(random_traffic=True, traffic_draws=3)
    with pytest.raises(NotImplementedError) as err:
        env.branch(0, [1])
    assert "random_traffic" in str(err.value) and "traffic_draws=3" in str(err.value)
    with pytest.raises(NotImplementedError):
        env.restore(_snapshot(), envs=[2, 1])
    with pytest.raises(ValueError):          # the same envs: allowed as far as the scope goes; there is no engine yet
        env.restore(_snapshot())
    assert branch.staged_draws(_env(random_traffic=True, traffic_draws=1, auto_reset=False).config) == 1


def test_signature_mismatch_and_invalidated_snapshots():
    token = object()
    sig = branch.batch_signature("pg", 8, 1, 259, None, ("shape", "env_map"))
    assert sig[4] == abi.MD_ABI_VERSION == 12
    snap = branch.EnvSnapshot([0, 1], [5, 6], sig, token, nbytes=64)
    assert (snap.num_envs, snap.source_envs, snap.seeds, snap.nbytes, snap.batch_signature) == (2, (0, 1), (5, 6), 64, sig)
    branch.check_snapshot(snap, sig, token)
    for other in (branch.batch_signature("marl:roundabout", 8, 1, 259, None, ("shape", "env_map")),
                  branch.batch_signature("pg", 16, 1, 259, None, ("shape", "env_map")),
                  branch.batch_signature("pg", 8, 2, 259, None, ("shape", "env_map")),
                  branch.batch_signature("pg", 8, 1, 19, None, ("shape", "env_map")),
                  branch.batch_signature("pg", 8, 1, 259, (84, 3, 5, 5, 1), ("shape", "env_map")),
                  branch.batch_signature("pg", 8, 1, 259, None, ("shape", "detected", "env_map"))):
        with pytest.raises(ValueError) as err:
            branch.check_snapshot(snap, other, token)
        assert "another kind of batch" in str(err.value)
    with pytest.raises(ValueError) as err:      # reset(seed=...), a rebuild or close() came after it
        branch.check_snapshot(snap, sig, object())
    assert "no longer valid" in str(err.value)
    # the engine's own snapshot from before a rebuild that also changed the batch's sizes: invalidated, not "another kind"
    owner = object()
    mine = branch.EnvSnapshot([0], [5], sig, token, owner=owner)
    with pytest.raises(ValueError) as err:
        branch.check_snapshot(mine, branch.batch_signature("pg", 16, 1, 259, None, ("shape", "env_map")), object(), owner=owner)
    assert "no longer valid" in str(err.value)
    with pytest.raises(ValueError) as err:
        branch.check_snapshot(mine, branch.batch_signature("pg", 16, 1, 259, None, ("shape", "env_map")), object(), owner=object())
    assert "another kind of batch" in str(err.value)
    with pytest.raises(TypeError):
        branch.check_snapshot(dict(), sig, token)


def test_snapshot_layout_is_sized_from_the_table():
    rows = branch.field_rows(cap=8, agents=1, obs_dim=259)
    assert rows["obs"] == 1036 and rows["shape"] == 256 and rows["route_nodes"] == 8 * 192 and rows["need_reset"] == 4
    present = {k: rows[k] for k in ("shape", "obs", "need_reset")}
    st, ex, total = branch.layout(present, [("env_map", 4), ("takeover", 1)], 3)
    assert st == {"shape": (0, 256), "obs": (768, 1036), "need_reset": (768 + 3120, 4)}      # 3 * 1036 = 3108 -> 3120
    assert ex == {"env_map": (3904, 4), "takeover": (3920, 1)} and total == 3936
    assert all(off % 16 == 0 for off, _ in list(st.values()) + list(ex.values()))
