"""One sha256 per host scene of a fixed list of small batches: everything a host scene hands to the device (world tables, state,
scene pool, recorded tracks, the MdConfig bytes).  Run it on two commits on the same machine and diff the outputs: a refactor of
the host layer must leave every line as it was.  The output is no fixture: map geometry goes through libm and need not hash alike
on another CPU.

    python tools/host_scene_digest.py > digest.txt
"""
import hashlib
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from metadrive_ped_amd.config import make_config                      # noqa: E402
from metadrive_ped_amd.engine import HostScene                        # noqa: E402
from metadrive_ped_amd.envs import marl_env, metadrive_env           # noqa: E402
from metadrive_ped_amd.scenario import ScenarioHostScene, make_scenario_config, synthetic_scenarios      # noqa: E402

E = 8
BASE = dict(num_envs=E, num_scenarios=E, build_workers=1)


def _single(**kw):
    return lambda: HostScene(make_config(dict(BASE, **kw)))


def _env(cls, **kw):
    return lambda: HostScene(cls(dict(BASE, **kw)).config)


def _scenario(n_scenes, **kw):
    def build():
        cfg = make_scenario_config(dict(BASE, num_scenarios=n_scenes, **kw))
        return ScenarioHostScene(cfg, synthetic_scenarios(n_scenes, 0, T=60))
    return build


SCENES = [
    ("single/trigger", _single(map=3, traffic_density=0.1)),
    ("single/respawn", _single(map=3, traffic_density=0.1, traffic_mode="respawn")),
    ("single/hybrid", _single(map=3, traffic_density=0.1, traffic_mode="hybrid")),
    ("single/replay", _single(map=3, traffic_density=0.1, traffic_mode="replay", horizon=200)),
    ("safe", _env(metadrive_env.BatchedSafeMetaDriveEnv)),
    ("varying_dynamics", _env(metadrive_env.BatchedVaryingDynamicsEnv)),
    ("pg_walk", _single(map=2, traffic_density=0.1, walk_scenarios=True, num_scenarios=12)),
    ("policy/idm", _single(map=2, agent_policy="IDMPolicy")),
    ("policy/lane_change", _single(map=2, agent_policy="LaneChangePolicy", discrete_action=True, use_multi_discrete=True)),
    ("policy/expert", _single(map=2, agent_policy="ExpertPolicy")),
    ("policy/ai_protect", _single(map=2, agent_policy="AIProtectPolicy")),
    ("policy/expert_own_sensors", _single(map=2, agent_policy="ExpertPolicy", expert_own_sensors=True)),
    ("marl/roundabout", _env(marl_env.BatchedMultiAgentRoundaboutEnv)),
    ("marl/intersection", _env(marl_env.BatchedMultiAgentIntersectionEnv)),
    ("marl/bottleneck", _env(marl_env.BatchedMultiAgentBottleneckEnv)),
    ("marl/tollgate", _env(marl_env.BatchedMultiAgentTollgateEnv)),
    ("marl/parking_lot", _env(marl_env.BatchedMultiAgentParkingLotEnv)),
    ("marl/racing", _env(marl_env.BatchedMultiAgentRacingEnv, map_config=dict(exit_length=60))),
    ("marl/pg", _env(marl_env.BatchedMultiAgentMetaDrive)),
    ("scenario/fixed", _scenario(E)),
    ("scenario/reactive", _scenario(E, reactive_traffic=True)),
    ("scenario/walk", _scenario(16, walk_scenarios=True)),
    ("scenario/walk_curriculum", _scenario(24, walk_scenarios=True, curriculum_level=3, sequential_seed=True)),
]


def _feed(h, name, value):
    h.update(name.encode())
    if isinstance(value, np.ndarray):
        h.update(str((value.dtype.str, value.shape)).encode())
        h.update(np.ascontiguousarray(value).tobytes())
    else:
        h.update(repr(value).encode())


def digest(host):
    h = hashlib.sha256()
    groups = [("world", host.world.arrays), ("state", host.state), ("pool", getattr(host, "pool", None)),
              ("tracks", getattr(host, "tracks", None))]
    for group, arrays in groups:
        for k in sorted(arrays or {}):
            _feed(h, group + "." + k, arrays[k])
    h.update(bytes(host.md_config))
    return h.hexdigest()


def main():
    only = sys.argv[1:]
    n = 0
    for name, build in SCENES:
        if only and not any(o in name for o in only):
            continue
        host = build()
        print("{:28s} E={} A={:<3d} cap={:<3d} obs_dim={:<4d} {}".format(name, host.E, host.A, host.cap, host.obs_dim, digest(host)),
              flush=True)
        n += 1
    print("{} scenes".format(n))


if __name__ == "__main__":
    main()
