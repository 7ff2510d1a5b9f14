"""ctypes binding of tests/expert_host.c, the host build of include/md_expert.h (compiled on first use into a temporary
directory by tests/hostlib.py).  TEST INFRASTRUCTURE."""
import ctypes as C
import os

import numpy as np

import hostlib
from hostlib import lane_index, ptr as _p

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
WEIGHTS = os.path.join(GOLDEN, "expert_weights.npz")


def _declare(L):
    P = C.c_void_p
    L.hx_expert.argtypes = [P, P, C.c_int, P, P]
    L.hx_mlp.argtypes = [P, P, C.c_int, P]
    L.hx_sample.argtypes = [P, P, C.c_int, P]
    L.hx_tanh.argtypes = [P, C.c_int, P]
    L.hx_exp.argtypes = [P, C.c_int, P]
    L.hx_widx.argtypes = [C.c_int, C.c_int, C.c_int]
    L.hx_widx.restype = C.c_int


def lib():
    return hostlib.build("expert_host", _declare)


def packed_weights(path=WEIGHTS):
    from metadrive_ped_amd.expert import load_expert_weights
    return np.ascontiguousarray(load_expert_weights(path))


def expert(w, raw):
    """raw [n, 275] float32 (uncorrected) -> (corrected obs [n, 275], mean | log_std [n, 4])"""
    raw = np.ascontiguousarray(raw, np.float32).reshape(-1, 275)
    corr = np.zeros_like(raw)
    out = np.zeros((len(raw), 4), np.float32)
    lib().hx_expert(_p(w), _p(raw), len(raw), _p(corr), _p(out))
    return corr, out


def mlp(w, x):
    x = np.ascontiguousarray(x, np.float32).reshape(-1, 275)
    out = np.zeros((len(x), 4), np.float32)
    lib().hx_mlp(_p(w), _p(x), len(x), _p(out))
    return out


def sample(out4, noise):
    out4 = np.ascontiguousarray(out4, np.float32)
    noise = np.ascontiguousarray(noise, np.float32)
    a = np.zeros((len(out4), 2), np.float32)
    lib().hx_sample(_p(out4), _p(noise), len(out4), _p(a))
    return a


def unary(name, x):
    x = np.ascontiguousarray(x, np.float32)
    y = np.zeros_like(x)
    getattr(lib(), "hx_" + name)(_p(x), x.size, _p(y))
    return y


# -- the reference's performance test (tests/test_policy/test_expert_performance.py) on the CPU oracle ------------------
LANE_ORDER = (0, 1, 2, 0, 1, 2, 0, 1, 2, 0)     # spawn lane of episode i: 0, then len(reward_list) % 3
PERF_CONFIGS = {
    "ccc": dict(map="CCC", traffic_density=0.0),
    "xtxts": dict(map="XTXTS", traffic_density=0.0),
    "ccc_traffic": dict(map="CCC", traffic_density=0.1),
}


def perf_config(name, lane, **extra):
    """_evaluate's env config (num_scenarios=1, start_seed=2, random_traffic=False, random_spawn_lane_index=False) on
    spawn lane `lane`; extra keys (e.g. the expert's num_others=4 for the oracle) are laid over it."""
    from metadrive_ped_amd.config import make_config
    cfg = dict(num_envs=1, num_scenarios=1, start_seed=2, random_traffic=False, random_spawn_lane_index=False,
               agent_configs={"default_agent": dict(spawn_lane_index=(">", ">>", lane))}, build_workers=1)
    cfg.update(PERF_CONFIGS[name])
    cfg.update(extra)
    return make_config(cfg)


def oracle_episode(w, name, lane, max_steps=3000, record=None):
    """One episode of the host expert (deterministic) driving the oracle with the expert's own observation config (lidar
    num_others=4, so the oracle's obs row IS the expert's raw observation).  -> dict(reward, flags, steps, on_lane)
    reward: float64 sum of the float32 step rewards; flags: the flag word of the last step; on_lane: the agent was on its
    spawn lane after every step.  record: a list that gets the raw observation rows."""
    import oracle_binding as ob
    from metadrive_ped_amd import abi
    from metadrive_ped_amd.engine import HostScene
    host = HostScene(perf_config(name, lane, vehicle_config=dict(lidar=dict(num_others=4))))
    o = ob.OracleWorld(host)
    o.reset()
    total, on_lane = 0.0, True
    for t in range(max_steps):
        raw = o.obs[0].copy()
        if record is not None:
            record.append(raw)
        _, out = expert(w, raw)
        o.step(out[:, :2].reshape(1, 1, 2))
        total += float(o.state["reward"][0])
        on_lane = on_lane and lane_index(host, o.state) == lane
        fl = int(o.state["flags"][0])
        if fl & (abi.FL_TERMINATED | abi.FL_TRUNCATED):
            return dict(reward=total, flags=fl & 0xFFFF, steps=t + 1, on_lane=on_lane)
    raise AssertionError("episode did not end in {} steps".format(max_steps))
