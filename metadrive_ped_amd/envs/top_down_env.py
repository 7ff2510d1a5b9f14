"""The top-down observation envs: TopDownMetaDrive and TopDownMetaDriveEnvV2 of the reference (envs/top_down_env.py:33-74) for E
lock-stepped environments.  reset() / step() return the bird's-eye observation of TopDownMultiChannel.observe
(obs/top_down_obs_multi_channel.py:237-280) as ONE device tensor [E, R, R, 2 + frame_stack], channels [road_network, past_pos,
traffic(t), traffic(t - frame_skip), ...]: float32 in [0, 1], or uint8 with norm_pixel=False.  The image is rasterised on the device
by md_topdown (include/md_topdown.h) right after md_step; no host sync.  It is the geometry the reference draws, sampled exactly --
not pygame's pixels.  The vector observation md_step computes stays at env.engine.obs.

Config keys of these classes only (any other class given one raises KeyError, as the reference's would): frame_skip=5,
frame_stack=3, post_stack=5, norm_pixel=True, resolution_size=84, distance=30.  Single-agent PG envs: the PG walk, random_traffic,
agent_policy = IDMPolicy / ExpertPolicy / LaneChangePolicy / AIProtectPolicy and spawn_object participants all work, since they only
change the state the kernel reads.  sharding.gather_step_slab and envs/pipeline.py carry the vector observation only."""
import numpy as np

from metadrive_ped_amd.envs.metadrive_env import BatchedMetaDriveEnv
from metadrive_ped_amd.envs.spaces import Box


class BatchedTopDownMetaDrive(BatchedMetaDriveEnv):
    """TopDownMetaDrive (envs/top_down_env.py:33-44): the multi-channel top-down observation, the vehicle's lidar kept."""
    TOP_DOWN = True

    def __init__(self, config=None):
        super().__init__(config)
        c = self.config
        shape = (c["resolution_size"], c["resolution_size"], 2 + c["frame_stack"])
        # TopDownMultiChannel.observation_space (obs/top_down_obs_multi_channel.py:301-307)
        self.observation_space = Box(-0.0, 1.0, shape, np.float32) if c["norm_pixel"] else Box(0, 255, shape, np.uint8)

    def _obs(self):
        return self.engine.topdown

    # -- checkpoints: the image's history (the traffic frames, the past positions, the cursors) travels with the state, so that the
    #    stacked channels and past_pos after set_state() are those of the run the checkpoint was taken from --------------------------
    HISTORY_KEYS = ("ring_traffic", "ring_pos", "cursor")

    def get_state(self):
        st = super().get_state()
        for k, v in self.engine.topdown_history().items():
            st["__topdown_" + k + "__"] = v
        return st

    def set_state(self, state):
        hist = {k: state.get("__topdown_" + k + "__") for k in self.HISTORY_KEYS}
        dev = self.engine.topdown_dev if self.engine is not None else {}
        for k, v in hist.items():
            if v is None or (k in dev and tuple(np.asarray(v).shape) != tuple(dev[k].shape)):
                raise ValueError("the checkpoint holds no top-down history {!r} of this batch's sizes (resolution_size, frame_stack, "
                                 "frame_skip, post_stack)".format(k))
        super().set_state(state)
        self.engine.upload_topdown_history(hist)


class BatchedTopDownMetaDriveEnvV2(BatchedTopDownMetaDrive):
    """TopDownMetaDriveEnvV2 (envs/top_down_env.py:47-74): the same observation with the lidar removed."""
    DEFAULTS = dict(vehicle_config=dict(lidar=dict(num_lasers=0, distance=0)))

    def __init__(self, config=None):
        config = dict(config or {})
        vc = dict(config.get("vehicle_config") or {})
        vc["lidar"] = dict(dict(num_lasers=0, distance=0), **(vc.get("lidar") or {}))     # "Remove lidar" (:51); the user's own wins
        config["vehicle_config"] = vc
        super().__init__(config)


class BatchedTopDownSingleFrameMetaDriveEnv:
    """TopDownSingleFrameMetaDriveEnv (envs/top_down_env.py:7-30), a colour rendering of the whole map: not built."""
    def __init__(self, config=None):
        raise NotImplementedError("TopDownSingleFrameMetaDriveEnv (TopDownObservation, a colour rendering of the whole map) is not built; "
                                  "built are BatchedTopDownMetaDrive and BatchedTopDownMetaDriveEnvV2, the multi-channel observation")
