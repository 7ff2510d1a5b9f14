"""A population of expert drivers: the multi-agent roundabout with every agent driven by the reference's PPO expert, which observes
each vehicle through its own sensors (240 lasers at 50 m, num_others=4) whatever the env's own lidar is -- here 72 lasers at 40 m.
agent_policy="ExpertPolicy" with expert_own_sensors=True acts inside step(); expert(env, own_sensors=True) gives the actions (and the
expert's observations) of any env, e.g. to collect demonstrations.

    python examples/marl_expert_rollout.py [expert_weights.npz]      (needs an MI355X; builds the library on first use)
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    from metadrive_ped_amd import hostpool
    hostpool.start()                                     # host build workers: before the first GPU call
    import torch
    from metadrive_ped_amd import abi
    from metadrive_ped_amd.envs import BatchedMultiAgentRoundaboutEnv
    from metadrive_ped_amd.expert import expert
    weights = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "expert_weights.npz")
    E = 64
    env = BatchedMultiAgentRoundaboutEnv(dict(num_envs=E, agent_policy="ExpertPolicy", expert_own_sensors=True, expert_weights=weights))
    obs, info = env.reset()
    print("env obs", tuple(obs.shape), "agents per env", env.num_agents)
    act, xobs = expert(env, deterministic=True, need_obs=True)          # what the expert sees and would do now
    print("expert obs", tuple(xobs.shape), "actions", tuple(act.shape))
    total = torch.zeros(E, env.num_agents, device=obs.device)
    arrived = crashed = 0
    for t in range(400):
        obs, reward, terminated, truncated, info = env.step(None)       # the experts drive: actions are ignored
        total += reward
        done = terminated | truncated
        arrived += int((done & info["arrive_dest"]).sum())
        crashed += int((done & info["crash_vehicle"]).sum())
        if t % 100 == 99:
            print("step %3d: mean step reward %.3f, arrived %d, crashed %d, applied |steer| %.3f" % (
                t + 1, float(total.mean()) / (t + 1), arrived, crashed, float(info["action"][..., 0].abs().mean())))
    env.close()
    hostpool.stop()


if __name__ == "__main__":
    main()
