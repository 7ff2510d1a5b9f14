#!/usr/bin/env python
"""Generate tests/golden/expert_policy.npz: the reference's own numpy expert (examples/ppo_expert/numpy_expert.py,
expert(vehicle, deterministic=True, need_obs=True)) on 256 raw 275-dim observations.  TEST INFRASTRUCTURE.

Run where the reference tree is (it imports it through oracle/gen/refshim.py, read-only; nothing under oracle/ changes):

    PYTHONDONTWRITEBYTECODE=1 python tools/gen_expert_golden.py

Inputs: float32 rows of oracle rollouts (the host expert driving the three configs of the reference's
test_expert_performance.py, every lane) plus all-zeros, all-ones and uniform [0, 1) rows.  The generator hands the
reference's expert its weights (`_expert_weights`, the npz of tests/golden) and an observation stub whose observe()
returns the row, so the correction, the matmuls, tanh and the split are the reference's own arithmetic.  Recorded: the
input row (raw), the corrected obs the expert returns (obs), `mean`, and `log_std` of the same forward pass, as float32
arrays in one compressed npz.
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle", "gen")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402

import expert_host as eh  # noqa: E402

OUT = os.environ.get("MD_GOLDEN_OUT") or os.path.join(ROOT, "tests", "golden")
N_ROLLOUT = 240


def rollout_rows():
    w = eh.packed_weights()
    rows = []
    for name in eh.PERF_CONFIGS:
        for lane in range(3):
            rec = []
            eh.oracle_episode(w, name, lane, record=rec)
            rows.append(np.asarray(rec, np.float32))
    per = N_ROLLOUT // len(rows)
    picked = [r[np.linspace(0, len(r) - 1, per).astype(int)] for r in rows]
    return np.concatenate(picked)


def main():
    rows = rollout_rows()
    rng = np.random.RandomState(2024)
    extra = [np.zeros(275, np.float32), np.ones(275, np.float32)] + \
        [rng.uniform(0, 1, 275).astype(np.float32) for _ in range(256 - len(rows) - 2)]
    rows = np.concatenate([rows, np.asarray(extra, np.float32)])
    assert rows.shape == (256, 275)

    import refshim
    refshim.install()
    from metadrive.examples.ppo_expert import numpy_expert as ne

    class _Stub:
        row = None

        def observe(self, vehicle):
            return self.row.copy()

    class _Vehicle:
        def __init__(self):
            self.config = {}

    weights = dict(np.load(eh.WEIGHTS))
    stub = _Stub()
    ne._expert_weights = weights
    ne._expert_observation = stub
    out = dict(raw=rows, obs=np.zeros_like(rows), mean=np.zeros((len(rows), 2), np.float32),
               log_std=np.zeros((len(rows), 2), np.float32))
    for i, r in enumerate(rows):
        stub.row = r
        mean, obs = ne.expert(_Vehicle(), deterministic=True, need_obs=True)
        x = obs.reshape(1, -1)
        # log_std of the same weights: the forward pass of expert() (numpy_expert.py:64-70), second half of the split
        h = np.tanh(np.matmul(x, weights["default_policy/fc_1/kernel"]) + weights["default_policy/fc_1/bias"])
        h = np.tanh(np.matmul(h, weights["default_policy/fc_2/kernel"]) + weights["default_policy/fc_2/bias"])
        o = (np.matmul(h, weights["default_policy/fc_out/kernel"]) + weights["default_policy/fc_out/bias"]).reshape(-1)
        assert np.array_equal(o[:2], mean)
        refshim.assert_plain([float(v) for v in mean], "mean")
        assert mean.dtype == np.float32 and obs.dtype == np.float32
        out["obs"][i], out["mean"][i], out["log_std"][i] = obs.reshape(-1), mean, o[2:]
    np.savez_compressed(os.path.join(OUT, "expert_policy.npz"), **out)
    print("wrote {} cases".format(len(rows)))


if __name__ == "__main__":
    main()
