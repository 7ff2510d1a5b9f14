"""BatchedMetaDriveEnv: the reset()/step() surface of the reference's MetaDriveEnv for E lock-stepped
environments on one MI355X.

Mirrors (same names, argument meaning, return structure and error behaviour, with a leading env
dimension): BaseEnv.reset / step / close / observation_space / action_space
(metadrive/envs/base_env.py:269,426-431,502-537,678-700), MetaDriveEnv.default_config
(envs/metadrive_env.py:16-99).  Single-agent returns are unwrapped like the reference's
(_wrap_as_single_agent, base_env.py:618-623): obs [E, 259], reward [E], terminated [E], truncated [E],
info = dict of [E] tensors with the reference's info keys (base_vehicle.py:243-252,
metadrive_env.py:132-152,203-211,269; base_env.py:614-616).

Everything returned is a torch tensor on the engine's device (views of the engine's buffers: copy
them if you keep them across steps).  With config auto_reset=True an env that terminated or was
truncated at step t is restored from its reset snapshot during step t+1, which then returns the
reset observation with reward 0 (gymnasium's NEXT_STEP autoreset convention).

walk_scenarios=True (the PG walk): an env whose episode ends moves on, on the device (md_swap_draw), to another scenario seed of
[start_seed, start_seed + num_scenarios) -- its map, spawn, route, traffic, props and vehicle parameters -- as the reference draws
a new seed at every reset (BaseEnv._reset_global_seed, envs/base_env.py:886-891).  Every seed of the slice is built once into a
scene pool.  sequential_seed=False: a uniform draw per (global env index, episode) from a reproducible stream; True: env e is worker
w = (env_seed_offset + e) % num_scenarios of walk_stride workers and plays start_seed + w + k * walk_stride.  info["env_seed"],
current_seeds and info["scenario_index"] (the position in the slice) follow each env's current scenario as device tensors;
reset() restarts every env at episode 0 of its walk; get_state() / set_state() carry the walk.
"""
import copy

import numpy as np

from metadrive_ped_amd import abi
from metadrive_ped_amd.config import make_config
from metadrive_ped_amd.envs.base import SINGLE_AGENT_FLAG_INFO, BatchedEnvBase, ObjectSpawnMixin
from metadrive_ped_amd.envs.spaces import Box, LazyInfo, Discrete, MultiDiscrete


def steering_dim(cfg):
    """Steering grid size of the discrete action space: LaneChangePolicy has 3 (left, keep, right) whatever
    discrete_steering_dim says (policy/lange_change_policy.py:22,57)."""
    return 3 if cfg["agent_policy"] == "LaneChangePolicy" else int(cfg["discrete_steering_dim"])


def make_action_space(cfg):
    """EnvInputPolicy.get_input_space (policy/env_input_policy.py:50-69); LaneChangePolicy.get_input_space
    (policy/lange_change_policy.py:50-62) with steering_dim(cfg) = 3."""
    if not cfg["discrete_action"]:
        return Box(-1.0, 1.0, (2, ), np.float32)
    if cfg["use_multi_discrete"]:
        return MultiDiscrete([steering_dim(cfg), cfg["discrete_throttle_dim"]])
    return Discrete(steering_dim(cfg) * cfg["discrete_throttle_dim"])


def discrete_to_continuous(torch, cfg, actions, lead_shape, device):
    """EnvInputPolicy.convert_to_continuous_action (policy/env_input_policy.py:40-48) for a batch: Discrete
    index -> (index % steering_dim, index // steering_dim), MultiDiscrete -> (a[0], a[1]); each grid index i
    maps to i * 2/(dim-1) - 1.  Returns float32 [*lead_shape, 2] on `device`.  Under LaneChangePolicy the steering
    grid has 3 values, so the steering is exactly -1 (right), 0 (keep) or +1 (left)."""
    sd, td = steering_dim(cfg), int(cfg["discrete_throttle_dim"])
    a = actions if torch.is_tensor(actions) else torch.as_tensor(np.asarray(actions))
    if a.is_floating_point():
        raise TypeError("discrete_action=True expects integer actions, got dtype {}".format(a.dtype))
    a = a.to(device)
    if cfg["use_multi_discrete"]:
        if tuple(a.shape) == (2, ):
            a = a.expand(*lead_shape, 2)
        if tuple(a.shape) != tuple(lead_shape) + (2, ):
            raise ValueError("actions must have shape {}, got {}".format(tuple(lead_shape) + (2, ), tuple(a.shape)))
        si, ti = a[..., 0], a[..., 1]
    else:
        if a.dim() == 0:
            a = a.expand(*lead_shape)
        if tuple(a.shape) != tuple(lead_shape):
            raise ValueError("actions must have shape {}, got {}".format(tuple(lead_shape), tuple(a.shape)))
        si, ti = a % sd, torch.div(a, sd, rounding_mode="floor")
    if cfg["action_check"]:
        ok = (si >= 0) & (si < sd) & (ti >= 0) & (ti < td)
        assert bool(ok.all()), "Input is not compatible with action space {}!".format(make_action_space(cfg))
    steering = si.to(torch.float32) * (2.0 / (sd - 1)) - 1.0
    throttle = ti.to(torch.float32) * (2.0 / (td - 1)) - 1.0
    return torch.stack([steering, throttle], dim=-1)


class BatchedMetaDriveEnv(ObjectSpawnMixin, BatchedEnvBase):
    metadata = {"render_modes": []}
    DEFAULTS = {}         # a subclass's own defaults, under the user's config (top-level keys)
    TOP_DOWN = False      # the top-down observation envs: their own config keys exist (config.TOP_DOWN_DEFAULT_CONFIG)
    FLAG_INFO = SINGLE_AGENT_FLAG_INFO + (("on_lane", abi.FL_ON_LANE), ("on_broken_line", abi.FL_ON_BROKEN))
    RENDER_MESSAGE = BatchedEnvBase.RENDER_MESSAGE + (": export_scenarios() gives the episode in the reference's scenario format "
                                                      "for its own top-down renderer; "
                                                      "BatchedTopDownMetaDrive / BatchedTopDownMetaDriveEnvV2 return the bird's-eye "
                                                      "observation as an image tensor")

    @classmethod
    def default_config(cls):
        return make_config(copy.deepcopy(cls.DEFAULTS), top_down=cls.TOP_DOWN)

    def __init__(self, config=None):
        super().__init__(make_config(dict(copy.deepcopy(self.DEFAULTS), **(config or {})), top_down=self.TOP_DOWN))
        if self.config["num_agents"] != 1 or self.config["is_multi_agent"]:
            raise NotImplementedError("BatchedMetaDriveEnv is the single-agent env; multi-agent envs are separate classes")
        if self.config["random_traffic"] and self.config["auto_reset"] and int(self.config.get("traffic_draws", 1)) <= 1:
            # the reference draws other traffic in EVERY episode (traffic_manager.py:335-337: the stream is not re-seeded at
            # reset); here a new draw happens at an explicit reset() only, and episodes that auto-reset restore the latest one
            import warnings
            warnings.warn("random_traffic=True with auto_reset=True and traffic_draws=1: traffic is re-drawn by env.reset() only; episodes that "
                          "auto-reset in between replay the latest draw (call reset() between episodes, or set auto_reset=False, "
                          "for a new draw per episode)", stacklevel=2)
        self.action_space = make_action_space(self.config)
        self.start_seed = self.config["start_seed"]
        self.episode_rewards = None

    def reset(self, seed=None):
        """seed: None keeps the scenario assignment; an int re-bases it (env e gets scenario
        seed + (env_seed_offset + e) % num_scenarios), regenerating maps/traffic on the host."""
        if seed is not None:
            if not (isinstance(seed, (int, np.integer)) and seed >= 0):
                raise ValueError("seed must be a non-negative int, got {!r}".format(seed))
            if self.engine is not None and int(seed) != self.config["start_seed"]:
                self.config["start_seed"] = int(seed)
                self.engine.rebuild(self.config)
            self.config["start_seed"] = int(seed)
        if self.config["random_traffic"] and self.engine is not None:
            # new traffic for the coming episodes (PGTrafficManager with random_traffic: the stream is not re-seeded at
            # reset); episodes that auto-reset in between restart from the latest draw
            self.config["traffic_epoch"] = int(self.config.get("traffic_epoch", 0)) + 1
            self.engine.rebuild(self.config)
        self.top_down_renderer = None      # BaseEnv.reset clears the top-down renderer (base_env.py:526-528)
        self.lazy_init()
        self.engine.reset()        # a walk: every env back to episode 0 of its walk
        if self.config["agent_policy"] == "AIProtectPolicy":     # BaseVehicle.reset (base_vehicle.py:361,367)
            self.engine.state_dev["takeover"].zero_()
            self.engine.state_dev["expert_takeover"].zero_()
            if self.engine.protect_flags is not None:
                self.engine.protect_flags.zero_()
        return self._obs(), self._info()

    def step(self, actions):
        self._require_engine("step")
        if self.config["agent_policy"] in ("IDMPolicy", "ExpertPolicy"):     # the agents drive themselves; `actions` is ignored
            self.engine.step(None)
        else:
            self.engine.step(self._coerce_actions(actions, (self.num_envs, ), self.config["discrete_action"]))
        terminated, truncated = self._done_flags()
        return self._obs(), self.engine.reward[:, 0], terminated, truncated, self._info()

    # -- agent_policy = AIProtectPolicy: vehicle.expert_takeover of every env (include/md_ai_protect.h) --------------------
    @property
    def expert_takeover(self):
        """[E] bool tensor on the device (a copy): the envs whose wheel the expert holds outright.  Cleared by reset() and by an
        env's auto-reset."""
        self._require_protect("expert_takeover")
        return self.engine.state_dev["expert_takeover"].bool()

    def set_expert_takeover(self, mask, envs=None):
        """vehicle.expert_takeover = mask (ManualControlPolicy.toggle_takeover sets it in the reference): one bool, or one per
        chosen env; `envs`: indices (None: every env)."""
        self._require_protect("set_expert_takeover")
        torch = self.engine.torch
        m = torch.as_tensor(mask, device=self.engine.device).to(torch.uint8).ne(0).to(torch.uint8)
        et = self.engine.state_dev["expert_takeover"]
        if envs is None:
            et.copy_(m.expand(self.num_envs))
        else:
            idx = torch.as_tensor(envs, dtype=torch.long, device=self.engine.device).reshape(-1)
            et[idx] = m.expand(idx.numel())

    def _require_protect(self, what):
        if self.config["agent_policy"] != "AIProtectPolicy":
            raise ValueError("{} belongs to agent_policy='AIProtectPolicy'".format(what))
        self._require_engine(what)

    # -- record / replay of the traffic (RecordManager / ReplayManager / ReplayTrafficParticipantPolicy) ------------
    def start_recording(self, max_steps):
        """Right after reset(): keep the pose of every mover for the next `max_steps` steps (device memory)."""
        self.engine.start_recording(max_steps)

    def stop_recording(self):
        return self.engine.stop_recording()

    def export_scenarios(self, tracks, envs=None):
        """BaseEnv.export_scenarios (envs/base_env.py:775-836) for a recorded batch: one scenario description (the
        reference's unified dict format, see scenario_export.py) per env of `envs` from stop_recording()'s tracks."""
        from metadrive_ped_amd.scenario_export import tracks_to_scenarios
        return tracks_to_scenarios(tracks, self.engine.host, envs)

    def load_scenarios(self, scenarios):
        """traffic_mode='replay' from scenario descriptions written by export_scenarios() (one per env, same scenario
        seeds): ScenarioEnv-style replay of data recorded here."""
        from metadrive_ped_amd.scenario_export import scenarios_to_tracks
        self._refuse_tracks_while_walking("load_scenarios")
        self.lazy_init()
        tracks = scenarios_to_tracks(scenarios, self.engine.host)
        torch = self.engine.torch
        self.load_tracks(dict(shape=torch.from_numpy(tracks["shape"].view(np.uint8).reshape(tracks["shape"].shape[0], -1)),
                              dyn=torch.from_numpy(tracks["dyn"]), seeds=tracks["seeds"], cap=tracks["cap"]))

    def load_tracks(self, tracks):
        """For an env built with traffic_mode='replay': the traffic follows `tracks` (from stop_recording() of an env
        with the same scenarios) instead of reacting; call before reset()."""
        self._refuse_tracks_while_walking("load_tracks")
        if self.config["traffic_mode"] != "replay":
            raise ValueError("load_tracks needs config traffic_mode='replay'")
        self.lazy_init()
        self.engine.set_tracks(tracks)

    def _refuse_tracks_while_walking(self, what):
        if self.config["walk_scenarios"]:
            raise NotImplementedError("{} with walk_scenarios=True is not built: recorded traffic belongs to one scenario assignment; "
                                      "replay a batch without the walk".format(what))

    # -- state checkpoint (the role of BaseEngine/BaseManager get_state / set_state, manager/base_manager.py:116-135,
    #    and of BaseVehicle.get_state / set_state, component/vehicle/base_vehicle.py:808-846: everything that
    #    evolves is already a flat array here, so a checkpoint is a dict of numpy arrays) -----------------------
    def get_state(self):
        """Every evolving array of the batch (poses, dynamics, navigation, PID, flags, obs, RNG ...) as host numpy
        arrays, plus the scenario assignment.  set_state() of the result resumes bit-identically."""
        self._require_engine("get_state")
        st = self.engine.download_state()
        st["__seeds__"] = np.asarray(self.engine.host.seeds, dtype=np.int64)     # a walk: the slice
        if self.engine.host.walk:       # each env's scene and walk position travel in scene_of / walk_ep; which walk it is, here
            st["__walk__"] = np.asarray(self.engine.host.walk_params, dtype=np.int64)
        elif getattr(self.engine, "_staged", None) is not None:       # random_traffic: which staged draw every env is on
            st["__draw_idx__"] = self.engine.draw_idx.cpu().numpy().copy()
        return st

    def set_state(self, state):
        self._require_engine("set_state")
        arrays = self._check_checkpoint(state)
        if self.engine.host.walk != ("scene_of" in arrays):
            raise ValueError("the checkpoint was taken with walk_scenarios={}, this batch has walk_scenarios={}".format(
                "scene_of" in arrays, self.engine.host.walk))
        if self.engine.host.walk and np.asarray(state.get("__walk__", ())).tolist() != list(self.engine.host.walk_params):
            # the same slice walked in another order (sequential_seed), by other workers (walk_stride, env_seed_offset): walk_ep
            # would continue a different schedule
            raise ValueError("the checkpoint was taken on another walk (num_scenarios, sequential_seed, walk_stride, env_seed_offset, "
                             "start_seed = {}, this batch has {})".format(np.asarray(state.get("__walk__", ())).tolist(),
                                                                          list(self.engine.host.walk_params)))
        draw_idx = state.get("__draw_idx__")
        if draw_idx is not None and getattr(self.engine, "_staged", None) is not None and not self.engine.host.walk:
            self.engine.draw_idx.copy_(self.engine.torch.from_numpy(np.asarray(draw_idx, dtype=np.int32)))
        self.engine.upload_state(arrays)
        self.engine.vector_obs_forget()     # a checkpoint does not carry the vector observation's history
        if self.engine.host.walk:     # the walk: each env's line map is its scene's
            self.engine.world_dev["env_map"].copy_(self.engine.state_dev["scene_of"])

    # -- helpers --------------------------------------------------------------------------------
    def _obs(self):
        return self.engine.obs[:, 0, :]

    def _info(self):
        e = self.engine
        fl = e.flags[:, 0]
        si = e.step_info[:, 0, :]
        eager = {
            "velocity": si[:, 1], "steering": e.dyn_f[:, 0, 2], "acceleration": e.dyn_f[:, 0, 3],
            "step_energy": si[:, 2], "episode_energy": si[:, 3], "step_reward": si[:, 0], "episode_reward": si[:, 4],
            "episode_length": e.nav_i[:, 0, 8], "cost": e.cost[:, 0], "total_cost": si[:, 5],
            "raw_action": e.action[:, 0, :], "action": e.action[:, 0, :],
        }
        lazy = self._flag_info(fl)
        lazy["env_seed"] = self._env_seed_tensor
        if self.config["agent_policy"] == "AIProtectPolicy":     # AIProtectPolicy.action_info (AI_protect_policy.py:54-58)
            for k, bit in (("takeover", abi.AIP_TAKEOVER), ("takeover_start", abi.AIP_TAKEOVER_START), ("takeover_end", abi.AIP_TAKEOVER_END)):
                lazy[k] = (lambda bit=bit: self._protect_flags() & bit != 0)
        lazy["scenario_index"] = self._scenario_index
        return LazyInfo(eager, lazy)

    def _protect_flags(self):
        e = self.engine
        fl = e.protect_flags      # None before the first step: nothing reported yet
        return fl if fl is not None else e.torch.zeros(self.num_envs, dtype=e.torch.uint8, device=e.device)

    def _scenario_index(self):
        """[E] int64: each env's position in the slice [start_seed, start_seed + num_scenarios).  A walk: MdState.scene_of, on the
        device (an env whose episode ended in this step has already been moved on: it names the scenario of its reset)."""
        e = self.engine
        if e.host.walk:
            return e.state_dev["scene_of"].view(e.torch.int32).long()
        return self._env_seed_tensor() - int(e.cfg["start_seed"])

    def _env_seed_tensor(self):
        e = self.engine
        if e.host.walk:     # follows the env's current scenario: no host copy to cache
            return self._scenario_index() + int(e.cfg["start_seed"])
        key = tuple(e.host.seeds)
        if getattr(self, "_seed_cache", (None, None))[0] != key:
            self._seed_cache = (key, e.torch.as_tensor(np.asarray(e.host.seeds, dtype=np.int64), device=e.device))
        return self._seed_cache[1]

    # -- small parts of BaseEnv's surface that user loops touch (envs/base_env.py:618-700) --------------------------
    @property
    def current_seed(self):
        """The scenario seed of env 0 (BaseEnv.current_seed)."""
        return self.current_seeds[0]

    @property
    def episode_step(self):
        """[E] steps taken in the running episode of every env (BaseEnv.episode_step)."""
        return self.engine.nav_i[:, 0, 8]

    @property
    def num_scenarios(self):
        return self.config["num_scenarios"]

    @property
    def current_seeds(self):
        """The scenario seed of every env: a list; under walk_scenarios the [E] device tensor start_seed + scene_of."""
        if self.engine.host.walk:
            return self._env_seed_tensor()
        return list(self.engine.host.seeds)


class BatchedSafeMetaDriveEnv(BatchedMetaDriveEnv):
    """SafeMetaDriveEnv (metadrive/envs/safe_metadrive_env.py:7-35): accident scenes on the road (cones,
    broken-down vehicle + warning tripod, barrier), crashes cost but do not terminate, info["total_cost"]
    accumulates the episode cost."""
    SAFE_DEFAULTS = DEFAULTS = dict(num_scenarios=100, accident_prob=0.8, traffic_density=0.05, crash_vehicle_done=False,
                                    crash_object_done=False)


class BatchedVaryingDynamicsEnv(BatchedMetaDriveEnv):
    """VaryingDynamicsEnv (metadrive/envs/varying_dynamics_env.py:14-60): the agent's engine force, brake force,
    wheel friction, maximum steering angle and mass are drawn per scenario seed from config["random_dynamics"]
    ({parameter: (min, max) | None}); like there, the same scenario seed always gives the same dynamics, so use
    num_scenarios > 1 for a spread.  `dynamics_parameters()` is the batch form of agent.get_dynamics_parameters()."""
    VARYING_DEFAULTS = DEFAULTS = dict(
        vehicle_config=dict(vehicle_model="varying_dynamics"),
        random_dynamics=dict(max_engine_force=(100, 3000), max_brake_force=(20, 600), wheel_friction=(0.1, 2.5),
                             max_steering=(10, 80), mass=(300, 3000)))

    def __init__(self, config=None):
        config = dict(config or {})
        if "vehicle_config" in config:      # on top of the class's vehicle_config; every other key replaces its default whole
            config["vehicle_config"] = dict(self.DEFAULTS["vehicle_config"], **config["vehicle_config"])
        super().__init__(config)

    def dynamics_parameters(self):
        """-> list (one dict per env) of the agent's max_engine_force / max_brake_force / wheel_friction / max_steering
        / mass, as sampled for its scenario."""
        self.lazy_init()
        keys = ("max_engine_force", "max_brake_force", "wheel_friction", "max_steering", "mass")
        h = self.engine.host
        seeds = h.seeds
        if h.walk:      # the scenario each env is on now (one device read)
            seeds = [int(s) for s in self.current_seeds.cpu().numpy()]
        return [{k: h.scenes[s].vehicle_cfgs[0][k] for k in keys if k in h.scenes[s].vehicle_cfgs[0]} for s in seeds]
