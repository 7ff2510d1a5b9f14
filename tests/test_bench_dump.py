"""bench.py --dump-outputs: the step outputs as float32 .npy files, within the size cap, with a fixed env sample above it.
Host logic only: a stand-in engine with CPU tensors of the engine's shapes and dtypes."""
import os
import types

import numpy as np
import torch

import bench


def fake_engine(E=512, A=2, D=19):
    g = torch.Generator().manual_seed(0)
    done = torch.zeros(E, A, 4, dtype=torch.bool)
    done[3, 1, 0] = done[7, 0, 1] = True
    done.view(torch.int16).view(E, A, 2)[:, :, 1] = torch.randint(0, 1 << 12, (E, A), generator=g, dtype=torch.int16)
    return types.SimpleNamespace(
        E=E, device=torch.device("cpu"), obs=torch.randn(E, A, D, generator=g), reward=torch.randn(E, A, generator=g),
        cost=torch.randn(E, A, generator=g), done_tt=done[:, :, 0:2], step_flags=done.view(torch.int16).view(E, A, 2)[:, :, 1],
        step_info=torch.randn(E, A, 8, generator=g))


def load_dir(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in os.listdir(d)}


def test_dump_writes_every_output_whole_when_it_fits(tmp_path):
    eng = fake_engine()
    bench.dump_outputs(eng, str(tmp_path), 0, 1)
    got = load_dir(str(tmp_path))
    assert sorted(got) == ["cost", "env_index", "obs", "reward", "step_flags", "step_info", "terminated", "truncated"]
    assert all(a.dtype in (np.float32, np.float64) for a in got.values())
    assert np.array_equal(got["env_index"], np.arange(eng.E))
    assert np.array_equal(got["obs"], eng.obs.numpy())
    assert np.array_equal(got["terminated"], eng.done_tt[..., 0].numpy().astype(np.float32))
    assert np.array_equal(got["truncated"], eng.done_tt[..., 1].numpy().astype(np.float32))
    assert np.array_equal(got["step_flags"], eng.step_flags.numpy().astype(np.float32))


def test_dump_samples_a_fixed_set_of_envs_above_the_cap(tmp_path, monkeypatch):
    eng = fake_engine()
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 64 << 10)
    for run in ("a", "b"):
        bench.dump_outputs(eng, str(tmp_path / run), 0, 1)
    a, b = load_dir(str(tmp_path / "a")), load_dir(str(tmp_path / "b"))
    total = sum(os.path.getsize(os.path.join(str(tmp_path / "a"), f)) for f in os.listdir(str(tmp_path / "a")))
    assert total <= 64 << 10
    idx = a["env_index"].astype(np.int64)
    assert 0 < len(idx) < eng.E and np.all(np.diff(idx) > 0)
    for k in a:
        assert np.array_equal(a[k], b[k])             # the same sample every run
    assert np.array_equal(a["obs"], eng.obs.numpy()[idx])
    assert np.array_equal(a["step_info"], eng.step_info.numpy()[idx])
