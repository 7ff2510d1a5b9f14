"""bench.py's command line and its --host-cache file: host logic only."""
import sys

import bench


def parse(monkeypatch, *argv):
    monkeypatch.setattr(sys, "argv", ["bench.py"] + list(argv))
    return bench.parse()


def test_a_plain_run_is_the_default(monkeypatch):
    a = parse(monkeypatch, "--gpus", "1", "--steps", "5", "--warmup", "2")
    assert not a.full and (a.gpus, a.steps, a.warmup) == (1, 5, 2)
    assert parse(monkeypatch, "--full").full


def test_host_cache_key_tells_a_plain_run_from_a_full_one(monkeypatch):
    plain = bench.host_cache_key(parse(monkeypatch), 0, 1)
    full = bench.host_cache_key(parse(monkeypatch, "--full"), 0, 1)
    assert plain != full and dict(plain, full=True) == full


def test_host_cache_round_trip_and_stale_key(tmp_path, capsys):
    path = str(tmp_path / "sub" / "hosts.pkl")
    assert bench.read_host_cache("", dict(k=1)) is None
    assert bench.read_host_cache(path, dict(k=1)) is None
    bench.write_host_cache(path, dict(k=1), dict(main=[1, 2, 3]))
    assert bench.read_host_cache(path, dict(k=1)) == dict(main=[1, 2, 3])
    assert bench.read_host_cache(path, dict(k=2)) is None
    assert "rebuilding" in capsys.readouterr().err
