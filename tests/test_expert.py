"""The PPO expert (metadrive_ped_amd/expert.py, include/md_expert.h) without a GPU: the host build of the kernel's
arithmetic against the reference's own numpy expert, its tanh / exp, the config rules, the weight file checks, and the
reference's expert performance test (tests/test_policy/test_expert_performance.py) restated on the CPU oracle."""
import os

import numpy as np
import pytest

import expert_host as eh

GOLDEN = os.path.join(eh.GOLDEN, "expert_policy.npz")


@pytest.fixture(scope="module")
def weights():
    return eh.packed_weights()


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as f:
        g = {k: f[k] for k in ("raw", "obs", "mean", "log_std")}
    assert g["raw"].shape == (256, 275)
    return g


def _f64_expert(x):
    f = np.load(eh.WEIGHTS)
    x = np.asarray(x, np.float64)
    h = np.tanh(x @ f["default_policy/fc_1/kernel"] + f["default_policy/fc_1/bias"])
    h = np.tanh(h @ f["default_policy/fc_2/kernel"] + f["default_policy/fc_2/bias"])
    return h @ f["default_policy/fc_out/kernel"] + f["default_policy/fc_out/bias"]


def test_host_build_reproduces_reference_expert(weights, golden):
    corr, out = eh.expert(weights, golden["raw"])
    assert np.array_equal(corr.view(np.uint32), golden["obs"].view(np.uint32)), "corrected obs differs from numpy_expert's"
    # the reference sums in its BLAS's order, the kernel in k order: the same float32 products, a different rounding path
    assert np.abs(out[:, :2] - golden["mean"]).max() < 1e-5
    assert np.abs(out[:, 2:] - golden["log_std"]).max() < 1e-5
    assert np.abs(out - _f64_expert(golden["obs"])).max() < 1e-5


def test_packing_matches_header_index(weights):
    f = np.load(eh.WEIGHTS)
    L = eh.lib()
    from metadrive_ped_amd.expert import IN_PAD, HID, N_PACKED
    assert weights.size == N_PACKED
    W1 = f["default_policy/fc_1/kernel"]
    rng = np.random.RandomState(0)
    for k, n in zip(rng.randint(0, 275, 500), rng.randint(0, 256, 500)):
        assert weights[L.hx_widx(IN_PAD, int(k), int(n))] == W1[k, n]
    # the padded rows of W1 are zero
    assert all(weights[L.hx_widx(IN_PAD, k, n)] == 0.0 for k in range(275, IN_PAD) for n in (0, 17, 255))
    W3 = f["default_policy/fc_out/kernel"]
    off = IN_PAD * HID + HID + HID * HID + HID
    assert weights[off + L.hx_widx(HID, 200, 3)] == W3[200, 3]
    assert weights[off + L.hx_widx(HID, 200, 9)] == 0.0


def test_tanh_exp_accuracy():
    """md_tanh / md_exp (the kernel's, + - * / only) against float64 numpy over [-20, 20]: within 2 ulp of the float32
    result, and tanh is exactly +-1 where float32 tanh saturates."""
    x = np.linspace(-20, 20, 400001).astype(np.float32)
    t = eh.unary("tanh", x).astype(np.float64)
    ref = np.tanh(x.astype(np.float64))
    ulp = np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64)
    assert (np.abs(t - ref) <= 2.0 * ulp).all()
    sat = np.abs(x) >= 9.0
    assert (t[sat] == np.sign(x[sat])).all()
    assert eh.unary("tanh", np.float32([0.0]))[0] == 0.0
    e = eh.unary("exp", x).astype(np.float64)
    ref = np.exp(x.astype(np.float64))
    assert (np.abs(e - ref) <= 2.0 * np.spacing(ref.astype(np.float32)).astype(np.float64)).all()


def test_sample_is_mean_plus_std_noise(weights, golden):
    out = eh.mlp(weights, golden["obs"][:8])
    noise = np.random.RandomState(1).standard_normal((8, 2)).astype(np.float32)
    a = eh.sample(out, noise)
    assert np.allclose(a, out[:, :2] + np.exp(out[:, 2:].astype(np.float64)) * noise, atol=1e-6)
    assert np.array_equal(eh.sample(out, np.zeros((8, 2), np.float32)), out[:, :2])


# -- config ------------------------------------------------------------------------------------------------------------
def test_expert_policy_accepted():
    from metadrive_ped_amd.config import make_config
    from metadrive_ped_amd.envs.metadrive_env import BatchedMetaDriveEnv, BatchedSafeMetaDriveEnv, BatchedVaryingDynamicsEnv
    for cls in (BatchedMetaDriveEnv, BatchedSafeMetaDriveEnv, BatchedVaryingDynamicsEnv):
        env = cls(dict(agent_policy="ExpertPolicy", expert_weights=eh.WEIGHTS))
        assert env.config["agent_policy"] == "ExpertPolicy"
        assert env.observation_space.shape == (259, )

    class ExpertPolicy:     # the reference passes the class
        pass

    assert make_config(dict(agent_policy=ExpertPolicy))["agent_policy"] == "ExpertPolicy"
    assert make_config({})["expert_weights"] is None


@pytest.mark.parametrize("user, what", [
    (dict(vehicle_config=dict(lidar=dict(num_others=4))), "num_others"),
    (dict(vehicle_config=dict(lidar=dict(gaussian_noise=0.1))), "gaussian_noise"),
    (dict(vehicle_config=dict(lidar=dict(dropout_prob=0.1))), "dropout_prob"),
    (dict(vehicle_config=dict(lidar=dict(num_lasers=120))), "num_lasers"),
    (dict(vehicle_config=dict(lidar=dict(distance=30))), "distance"),
    (dict(vehicle_config=dict(side_detector=dict(num_lasers=120))), "side_detector"),
    (dict(vehicle_config=dict(lane_line_detector=dict(num_lasers=120))), "lane_line_detector"),
    (dict(random_agent_model=True), "random_agent_model"),
])
def test_expert_policy_refused_with_other_obs(user, what):
    from metadrive_ped_amd.config import make_config
    with pytest.raises(ValueError, match=what) as ei:
        make_config(dict(user, agent_policy="ExpertPolicy"))
    assert "numpy_expert.py" in str(ei.value)


def test_expert_policy_refused_in_other_envs():
    from metadrive_ped_amd.envs.marl_env import BatchedMultiAgentMetaDrive, BatchedMultiAgentRoundaboutEnv
    from metadrive_ped_amd.envs.scenario_env import BatchedScenarioEnv
    with pytest.raises((ValueError, NotImplementedError), match="ExpertPolicy.*multi-agent"):
        BatchedMultiAgentRoundaboutEnv(dict(agent_policy="ExpertPolicy"))
    with pytest.raises((ValueError, NotImplementedError), match="ExpertPolicy.*multi-agent"):
        BatchedMultiAgentMetaDrive(dict(agent_policy="ExpertPolicy"))
    with pytest.raises((ValueError, NotImplementedError), match="ExpertPolicy.*BatchedScenarioEnv"):
        BatchedScenarioEnv(dict(agent_policy="ExpertPolicy"))


def test_expert_refuses_env_config():
    from metadrive_ped_amd.envs.metadrive_env import BatchedMetaDriveEnv
    from metadrive_ped_amd.expert import expert
    env = BatchedMetaDriveEnv(dict(vehicle_config=dict(lidar=dict(num_lasers=120))))
    with pytest.raises(ValueError, match="num_lasers"):
        expert(env)


def test_bad_weight_files(tmp_path):
    from metadrive_ped_amd.expert import load_expert_weights
    f = dict(np.load(eh.WEIGHTS))
    missing = dict(f)
    missing.pop("default_policy/fc_2/bias")
    np.savez(tmp_path / "missing.npz", **missing)
    with pytest.raises(ValueError, match="fc_2/bias"):
        load_expert_weights(str(tmp_path / "missing.npz"))
    bad = dict(f)
    bad["default_policy/fc_1/kernel"] = bad["default_policy/fc_1/kernel"][:259]
    np.savez(tmp_path / "shape.npz", **bad)
    with pytest.raises(ValueError, match=r"fc_1/kernel.*\(259, 256\)"):
        load_expert_weights(str(tmp_path / "shape.npz"))
    assert load_expert_weights(eh.WEIGHTS).dtype == np.float32


def test_missing_reference_names_the_key(monkeypatch):
    import importlib.util
    from metadrive_ped_amd import expert as ex
    real = importlib.util.find_spec
    monkeypatch.setattr(importlib.util, "find_spec", lambda name, *a: None if name == "metadrive" else real(name, *a))
    with pytest.raises(FileNotFoundError, match="expert_weights"):
        ex.load_expert_weights(None)


# -- the reference's expert performance test on the CPU oracle ----------------------------------------------------------
def _evaluate(weights, name, need_on_same_lane):
    """_evaluate of test_expert_performance.py: 10 episodes in its spawn-lane order, deterministic expert."""
    eps = [eh.oracle_episode(weights, name, lane) for lane in eh.LANE_ORDER]
    from metadrive_ped_amd import abi
    success = [1 if e["flags"] & abi.FL_ARRIVE_DEST else 0 for e in eps]
    if need_on_same_lane:
        assert all(e["on_lane"] for e in eps), "Not one the same lane"
    return sum(e["reward"] for e in eps) / len(eps), sum(success) / len(success), eps


def test_expert_without_traffic(weights):
    reward, success, _ = _evaluate(weights, "ccc", need_on_same_lane=True)
    assert success == 1.0, success
    assert 300 <= reward <= 350, reward


def test_expert_in_intersection(weights):
    reward, success, _ = _evaluate(weights, "xtxts", need_on_same_lane=True)
    assert success == 1.0, success
    assert reward > 400, reward


def test_expert_with_traffic(weights):
    reward, _, _ = _evaluate(weights, "ccc_traffic", need_on_same_lane=False)
    assert 300 < reward < 350, reward
