"""The reference's PPO driving expert for a whole batch: metadrive.examples.expert (examples/ppo_expert/numpy_expert.py:34-77)
and ExpertPolicy (policy/expert_policy.py), with the MLP in HIP (md_expert, include/md_expert.h).

    from metadrive_ped_amd.expert import expert
    env = BatchedMetaDriveEnv(dict(num_envs=4096, expert_weights="expert_weights.npz"))
    obs, info = env.reset()
    for _ in range(1000):
        obs, reward, terminated, truncated, info = env.step(expert(env, deterministic=True))

or agent_policy="ExpertPolicy", which runs the expert inside step() (stochastic, like ExpertPolicy.act).

The weights are the reference's asset (examples/ppo_expert/expert_weights.npz) and are not shipped here: pass the file
(config["expert_weights"] or load_expert_weights(path)), or have the reference package installed, where it is found
without importing it.

The expert observes the agent with its own LidarStateObservation (240 beams, 50 m, num_others=4) and, on every call,
rewrites the vehicle's lidar config to (240, 50, num_others=0) with random_agent_model=False (numpy_expert.py:58-62).
By default only configs where that rewrite changes nothing are accepted (config.expert_config_problem); there the env's own
259-dim observation is the expert's state block and cloud, and only the 16 "others" dims are added, by the kernel.

With config["expert_own_sensors"]=True (or expert(env, own_sensors=True) for one call) the expert observes for itself, as in the
reference: md_expert_sense (include/md_expert_sense.h) builds the 275-vector of every agent from the live state -- state and
navigation dims, a 240-beam / 50 m lidar cast with its own detected sets, the four nearest detected vehicles -- in the same launch
as the MLP.  Any vehicle_config goes, and so do the multi-agent envs (all but tollgate), where the tensors are [E, A, ...].  The
env's own lidar noise and dropout belong to the env's observation and never touch the expert's.  An env that is about to restore
itself (its episode just ended) is not sensed: its rows are zeros, and the step ignores its action anyway.
"""
import importlib.util
import os

import numpy as np

from metadrive_ped_amd.config import expert_config_problem

IN, IN_PAD, HID, OUT, OUT_PAD = 275, 288, 256, 4, 16
LAYERS = (("fc_1", (IN, HID)), ("fc_2", (HID, HID)), ("fc_out", (HID, OUT)))
N_PACKED = IN_PAD * HID + HID + HID * HID + HID + HID * OUT_PAD + OUT_PAD     # MD_EXPERT_NW


def reference_weights_path():
    """metadrive/examples/ppo_expert/expert_weights.npz of an installed reference package (located, not imported)."""
    spec = importlib.util.find_spec("metadrive")
    if spec is None or not spec.submodule_search_locations:
        return None
    for root in spec.submodule_search_locations:
        p = os.path.join(root, "examples", "ppo_expert", "expert_weights.npz")
        if os.path.exists(p):
            return p
    return None


def _pack_matrix(W, K, N):
    """W [k][n] -> the kernel's B-operand order (md_expert_widx): zero-padded to [K][N], tiles (n/16, k/16) of
    64 lanes x 4 floats, lane = (k % 4) * 16 + n % 16, float = (k % 16) / 4."""
    P = np.zeros((K, N), np.float32)
    P[:W.shape[0], :W.shape[1]] = W
    # [nt][g][s][r][c] with k = 16 g + 4 s + r, n = 16 nt + c  ->  [nt][g][r][c][s]
    t = P.reshape(K // 16, 4, 4, N // 16, 16).transpose(3, 0, 2, 4, 1)
    return np.ascontiguousarray(t).reshape(-1)


def pack_expert_weights(w):
    """dict of the npz arrays -> the packed fp32 buffer of include/md_expert.h (W1 | b1 | W2 | b2 | W3 | b3)."""
    g = lambda n, p: np.asarray(w["default_policy/{}/{}".format(n, p)], np.float32)
    b3 = np.zeros(OUT_PAD, np.float32)
    b3[:OUT] = g("fc_out", "bias")
    out = np.concatenate([_pack_matrix(g("fc_1", "kernel"), IN_PAD, HID), g("fc_1", "bias"),
                          _pack_matrix(g("fc_2", "kernel"), HID, HID), g("fc_2", "bias"),
                          _pack_matrix(g("fc_out", "kernel"), HID, OUT_PAD), b3])
    assert out.size == N_PACKED
    return out


def load_expert_weights(path=None):
    """Read and check the expert's npz (the default_policy/fc_1|fc_2|fc_out/kernel|bias arrays of the reference's
    expert_weights.npz; other arrays, e.g. the critic's, are ignored) and pack it -> float32 [MD_EXPERT_NW]."""
    if path is None:
        path = reference_weights_path()
        if path is None:
            raise FileNotFoundError("the expert's weights were not found: pass the path of the reference's "
                                    "examples/ppo_expert/expert_weights.npz (load_expert_weights(path) or config "
                                    "['expert_weights']); they are not shipped with this package")
    with np.load(path) as f:
        w = {}
        for name, (k, n) in LAYERS:
            for part, shape in (("kernel", (k, n)), ("bias", (n, ))):
                key = "default_policy/{}/{}".format(name, part)
                if key not in f.files:
                    raise ValueError("{}: expert weights need '{}' (missing)".format(path, key))
                a = f[key]
                if tuple(a.shape) != shape:
                    raise ValueError("{}: '{}' has shape {}, the expert needs {}".format(path, key, tuple(a.shape), shape))
                if not np.isfinite(a).all():
                    raise ValueError("{}: '{}' is not finite".format(path, key))
                w[key] = a
    return pack_expert_weights(w)


def _engine_of(env):
    eng = getattr(env, "engine", env)
    if eng is None or not hasattr(eng, "expert_forward"):
        raise RuntimeError("expert(env): call env.reset() first")
    return eng


def expert(env, deterministic=False, need_obs=False, own_sensors=None):
    """The batched metadrive.examples.expert: -> action [E, 2] (and the corrected expert observation [E, 275] with
    need_obs), device tensors on the env's stream, no host synchronisation.  deterministic=False draws
    N(mean, exp(log_std)) from the engine's expert stream (a device generator seeded with start_seed + env_seed_offset;
    the reference draws from the global numpy stream).  The returned tensors are fresh (not views of engine buffers).
    own_sensors: None = config["expert_own_sensors"]; True = the expert observes through its own sensors in this call, on an
    env built without the key too.  Multi-agent envs (own sensors only): [E, A, 2] and [E, A, 275]."""
    cfg = getattr(env, "config", None) or getattr(env, "cfg")
    own = bool(cfg.get("expert_own_sensors")) if own_sensors is None else bool(own_sensors)
    problem = expert_config_problem(cfg, own_sensors=own)
    if problem:
        raise ValueError(problem)
    eng = _engine_of(env)
    out = eng.expert_forward(deterministic=deterministic, need_obs=need_obs, own_sensors=own)
    if not own or eng.A == 1:
        return out
    shape = lambda t: t.view(eng.E, eng.A, t.shape[-1])
    return (shape(out[0]), shape(out[1])) if need_obs else shape(out)
