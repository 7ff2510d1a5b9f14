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
Only configs where that rewrite changes nothing are accepted (config.expert_config_problem); there the env's own
259-dim observation is the expert's state block and cloud, and only the 16 "others" dims are added, by the kernel.
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


def expert(env, deterministic=False, need_obs=False):
    """The batched metadrive.examples.expert: -> action [E, 2] (and the corrected expert observation [E, 275] with
    need_obs), device tensors on the env's stream, no host synchronisation.  deterministic=False draws
    N(mean, exp(log_std)) from the engine's expert stream (a device generator seeded with start_seed + env_seed_offset;
    the reference draws from the global numpy stream).  The returned tensors are fresh (not views of engine buffers)."""
    cfg = getattr(env, "config", None) or getattr(env, "cfg")
    problem = expert_config_problem(cfg)
    if problem:
        raise ValueError(problem)
    eng = _engine_of(env)
    return eng.expert_forward(deterministic=deterministic, need_obs=need_obs)
