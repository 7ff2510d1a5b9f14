"""BatchedScenarioEnv: the reset()/step() surface of the reference's ScenarioEnv (envs/scenario_env.py) for E
lock-stepped scenes on one MI355X.  Scene e replays scenario description e: read from `data_directory` (a ScenarioNet
dataset folder, as the reference's ScenarioDataManager reads it: metadrive_ped_amd/scenario_data.py), or handed in as dicts
of the same format (e.g. from BatchedMetaDriveEnv.export_scenarios()), or metadrive_ped_amd.scenario.synthetic_scenarios().

Returns like the single-agent env: obs [E, obs_dim] (side cloud | state | 22 navigation dims | lidar), reward [E],
terminated [E], truncated [E], info = dict of [E] tensors with ScenarioEnv's keys (route_completion, cost, crash_*,
out_of_road, arrive_dest, max_step, ..., and scenario_index: the dataset index each env plays).

walk_scenarios=True: the envs walk through the dataset slice [start_scenario_index, start_scenario_index + num_scenarios), a new
scenario whenever an episode ends (the reference's ScenarioEnv picks one at every reset, envs/scenario_env.py:359-380).  Every
scenario of the slice is built once into a scene pool; the device moves an env that has finished its episode on to its next
scene (md_swap_draw), so a walk step costs what a fixed-scene step does.  The order:
  sequential_seed=True: env e is worker w = (env_seed_offset + e) % num_scenarios of W = walk_stride workers (default num_envs;
    sharding.shard_config sets it to the env count over all shards, so the shards split the slice as RLlib workers do).  It plays
    start + w, then adds W after every episode, and goes back to start + w once the seed reaches start + num_scenarios: env e
    plays only start + w + k * W, never the seeds in between.  (One worker of the reference's multi-worker rule, not one
    single-env walk spread over the batch.)
  sequential_seed=False: a uniform draw over the slice per (env, episode), from a stream keyed by start_seed and the global env
    index -- reproducible, where the reference's draw is unseeded.
reset() starts every env again at the first scenario of its walk; get_state() / set_state() carry each env's scene and walk
position (MdState.scene_of / walk_ep) with the rest of the state.

The curriculum of a walk (ScenarioEnv's curriculum manager, one per env as one per worker in the reference): curriculum_level=L > 1
sorts the slice by difficulty (scenario.difficulty_score) and splits it into L windows of num_scenarios / L; each env plays its
worker's scenarios of its window and moves one window up at an episode end once its recent success rate reaches
target_success_rate (include/md_curriculum.h, md_curriculum after every step).  Walk batches report curriculum_level,
scenario_difficulty, data_coverage, curriculum_success and curriculum_route_completion as [E] tensors; with L > 1
scenario_index is the position in the sorted slice.  reset() keeps levels, queues and coverage and restarts each env at its
worker's first scenario of its level."""
import numpy as np

from metadrive_ped_amd import abi
from metadrive_ped_amd.envs.base import SINGLE_AGENT_FLAG_INFO, BatchedEnvBase
from metadrive_ped_amd.envs.spaces import Box, LazyInfo
from metadrive_ped_amd.scenario import ScenarioHostScene, make_scenario_config, synthetic_scenarios


def scenario_bench_config(common):
    """bench.py --workload scenario: reactive traffic, 240-beam lidar, 200-frame synthetic scenes"""
    cfg = make_scenario_config(dict(common, reactive_traffic=True, horizon=400,
                                    vehicle_config=dict(lidar=dict(num_lasers=240, distance=50))))
    return cfg


class BatchedScenarioEnv(BatchedEnvBase):
    metadata = {"render_modes": []}
    FLAG_INFO = SINGLE_AGENT_FLAG_INFO
    ASSIGNMENT = ("start_scenario_index", "tracks")

    @classmethod
    def default_config(cls):
        return make_scenario_config({})

    def __init__(self, config=None, scenarios=None):
        super().__init__(make_scenario_config(config), scenario=True)
        walk = bool(self.config["walk_scenarios"])
        if scenarios is None and self.config["data_directory"] is not None:
            from metadrive_ped_amd.scenario_data import load_scenarios
            # scene e = scenario start_scenario_index + (offset + e) % num_scenarios; a walk: the whole slice, in order
            scenarios = load_scenarios(self.config, pool=walk)
        if scenarios is None and walk:
            scenarios = synthetic_scenarios(self.config["num_scenarios"], self.config["start_scenario_index"])
        if scenarios is None:
            scenarios = synthetic_scenarios(self.num_envs, self.config["start_scenario_index"] + self.config["env_seed_offset"])
        self.scenarios = scenarios
        self.host = None
        self.action_space = Box(-1.0, 1.0, (2, ), np.float32)

    def _build_host(self):
        return ScenarioHostScene(self.config, self.scenarios)

    def lazy_init(self, host=None):
        super().lazy_init(host)
        self.host = self.engine.host

    def reset(self, seed=None):
        self.top_down_renderer = None      # BaseEnv.reset clears the top-down renderer (base_env.py:526-528)
        self.lazy_init()
        self.engine.scenario_metrics_forget()      # last_episode / episodes too: a reset() starts the evaluation afresh
        self.engine.reset()
        return self.engine.obs[:, 0, :], self._info()

    def step(self, actions):
        self._require_engine("step")
        if actions is None and self.config["agent_policy"] == "ReplayEgoCarPolicy":
            actions = np.zeros((self.num_envs, 2), np.float32)      # the agent replays the SDC track: actions are ignored
        self.engine.step(self._coerce_actions(actions, (self.num_envs, ), False))
        terminated, truncated = self._done_flags()
        return self.engine.obs[:, 0, :], self.engine.reward[:, 0], terminated, truncated, self._info()

    # -- the vector scene observation (include/md_scenario_vector_obs.h) ----------------------------------------------------------
    def _vector_obs_config(self, what):
        vo = self.config.get("scenario_vector_obs")
        if vo is None:
            raise RuntimeError("{}(): config['scenario_vector_obs'] is None; give it a dict ({{}} takes the defaults) to turn the "
                               "vector scene observation on".format(what))
        return vo

    def vector_obs_spec(self):
        """{name: (shape, numpy dtype)} of vector_obs()'s tensors, leading axis [E]"""
        outs = abi.scenario_vector_obs_blocks(self._vector_obs_config("vector_obs_spec"), 1)[0]
        return {name: ((self.num_envs, ) + tuple(shape), dt.type) for name, (_, shape, dt) in outs.items()}

    def vector_obs(self):
        """The vector scene observation of the state the last step() / reset() left, a dict of device tensors in the ego frame, metres:
        agents [E, K, T, 4] (x, y, cos, sin per frame, frame 0 = now), agents_mask, agents_meta [E, K, 4] (length, width, speed, kind),
        ego [E, T, 4], ego_mask, route [E, M, 4] (x, y, dx, dy of the recorded trajectory ahead), route_mask, map [E, P, S, 2] (the
        nearest map polyline pieces), map_mask [E, P, S], map_meta [E, P, 4] (class 0 lane / 1 line / 2 edge, type code -- the index
        into scenario.MAP_FEATURE_TYPES --, points, squared distance).  Views of the engine's buffers, valid until the next step() /
        reset(); no host sync."""
        self._vector_obs_config("vector_obs")
        self._require_engine("vector_obs")
        return dict(self.engine.vector_obs_out)

    # -- the traffic lights (include/md_traffic_lights.h) ----------------------------------------------------------------------------
    def _traffic_lights_config(self, what):
        tl = self.config.get("traffic_lights")
        if tl is None:
            raise RuntimeError("{}(): config['traffic_lights'] is None; give it a dict ({{}} takes the defaults) to turn the traffic "
                               "lights on".format(what))
        return tl

    def traffic_lights_spec(self):
        """{name: (shape, numpy dtype)} of traffic_lights()'s tensors, leading axis [E]"""
        outs = abi.traffic_lights_blocks(self._traffic_lights_config("traffic_lights_spec"))[0]
        return {name: ((self.num_envs, ) + tuple(shape), dt.type) for name, (_, shape, dt) in outs.items()}

    def traffic_lights(self):
        """The traffic lights as the last step() / reset() left them, a dict of device tensors: agent_light [E] uint8 (bit 0 green,
        bit 1 yellow, bit 2 red: the walls the ego's chassis overlapped in this step, by the status they had during it), lights
        [E, L, 6] (x, y of the stop point and dx, dy of the lane direction in the ego frame, metres; the status now on show -- 0
        unknown, 1 green, 2 yellow, 3 red --; the squared distance), lights_mask [E, L], lights_index [E, L] int32 (the light's place
        in traffic_light_ids(scenario), -1 for an empty rank).  Views of the engine's buffers, valid until the next step() / reset();
        no host sync."""
        self._traffic_lights_config("traffic_lights")
        self._require_engine("traffic_lights")
        return dict(self.engine.traffic_lights_out)

    def traffic_light_ids(self, scenario_index):
        """The keys of dynamic_map_states that became lights of scenario `scenario_index` (its position in the batch, or in the walk's
        pool), in the order lights_index counts them (host list)"""
        self._traffic_lights_config("traffic_light_ids")
        self._require_engine("traffic_light_ids")
        return list(self.engine.host.traffic_light_ids[int(scenario_index)])

    # -- the closed-loop driving metrics (include/md_scenario_metrics.h) ---------------------------------------------------------------
    def _scenario_metrics_config(self, what):
        sm = self.config.get("scenario_metrics")
        if sm is None:
            raise RuntimeError("{}(): config['scenario_metrics'] is None; give it a dict ({{}} takes the defaults) to turn the driving "
                               "metrics on".format(what))
        return sm

    def scenario_metrics_spec(self):
        """{name: (shape, numpy dtype)} of scenario_metrics()'s tensors, leading axis [E]"""
        outs, _, state, _ = abi.scenario_metrics_blocks(self._scenario_metrics_config("scenario_metrics_spec"))
        return {name: ((self.num_envs, ) + tuple(shape), dt.type) for table in (outs, state) for name, (_, shape, dt) in table.items()}

    def scenario_metrics(self):
        """The driving metrics as the last step() / reset() left them, a dict of device tensors: step [E, 12] (the columns
        abi.SCENARIO_METRICS_STEP_COLUMNS: divergence from the recorded drive, speed and its finite differences, time to collision,
        on_red), step_valid [E] int32 (bit i: column i means something), ttc_slot [E] int32 (the mover of the first overlap, -1
        without one), episode [E, 24] (abi.SCENARIO_METRICS_EPISODE_COLUMNS over the running episode), last_episode [E, 24] (the same
        of the env's last finished episode, kept through the auto-reset), episodes [E] int32 (how many it has finished since
        reset()), history [E, 12] (the kernel's own row).  Views of the engine's buffers, valid until the next step() / reset(); no
        host sync.  step()'s info carries three of them as lazy [E] tensors: log_divergence and time_to_collision (the step columns;
        0 where step_valid says the column means nothing) and comfortable (the running episode has no comfort violation so far)."""
        self._scenario_metrics_config("scenario_metrics")
        self._require_engine("scenario_metrics")
        return dict(self.engine.scenario_metrics_out)

    # -- checkpoints (envs/base_env.py:775-836 get_state / set_state through the managers): a dict of numpy arrays; the routes the
    #    device cut at later spawn frames are state too and travel with it -----------------------------------------------------
    def get_state(self):
        self._require_engine("get_state")
        st = self.engine.download_state()
        st["__seeds__"] = np.asarray(self.engine.host.seeds, dtype=np.int64)
        st["__scenario_ids__"] = np.asarray(self.engine.host.scenario_ids)
        st["__abi__"] = np.asarray([abi.MD_ABI_VERSION], dtype=np.int64)
        return st

    def set_state(self, state):
        self._require_engine("set_state")
        if "__abi__" in state and int(np.asarray(state["__abi__"])[0]) != abi.MD_ABI_VERSION:
            raise ValueError("the checkpoint was written by ABI v{}, this library is v{}: the record layouts differ".format(
                int(np.asarray(state["__abi__"])[0]), abi.MD_ABI_VERSION))
        arrays = self._check_checkpoint(state)
        if "__scenario_ids__" in state and [str(x) for x in np.asarray(state["__scenario_ids__"]).tolist()] != list(self.engine.host.scenario_ids):
            raise ValueError("the checkpoint was taken on other scenarios (their ids differ): tracks and routes would not match")
        self.engine.upload_state(arrays)
        if "scene_of" in arrays:     # the walk: each env's line map is its scene
            self.engine.world_dev["env_map"].copy_(self.engine.state_dev["scene_of"])
        self.engine.vector_obs_forget()     # a checkpoint does not carry the vector observation's history
        self.engine.scenario_metrics_forget()   # ... nor the driving metrics

    def _info(self):
        e = self.engine
        fl = e.flags[:, 0]
        si = e.step_info[:, 0, :]
        eager = {"velocity": si[:, 1], "step_energy": si[:, 2], "episode_energy": si[:, 3], "step_reward": si[:, 0],
                 "episode_reward": si[:, 4], "episode_length": e.nav_i[:, 0, 8], "cost": e.cost[:, 0], "total_cost": si[:, 5],
                 "route_completion": si[:, 6], "action": e.action[:, 0, :], "raw_action": e.action[:, 0, :]}
        lazy = self._flag_info(fl)
        lazy["scenario_index"] = self._scenario_index
        if e.traffic_lights_out is not None:   # vehicle.red_light / yellow_light / green_light (base_vehicle.py:720-733), device ops only
            al = e.traffic_lights_out["agent_light"]
            lazy.update(green_light=lambda: (al & abi.TL_BIT_GREEN) != 0, yellow_light=lambda: (al & abi.TL_BIT_YELLOW) != 0,
                        red_light=lambda: (al & abi.TL_BIT_RED) != 0)
        if self.config.get("scenario_metrics") is not None:  # this step's headline metrics, device ops only (scenario_metrics() has the rest)
            step, col = e.scenario_metrics_out["step"], abi.SCENARIO_METRICS_STEP_COLUMNS.index
            comfort = e.scenario_metrics_out["episode"][:, abi.SCENARIO_METRICS_EPISODE_COLUMNS.index("comfort_violation_steps")]
            lazy.update(log_divergence=lambda: step[:, col("log_divergence")], time_to_collision=lambda: step[:, col("ttc")],
                        comfortable=lambda: comfort == 0)
        if e.host.walk:     # the curriculum's keys (envs/scenario_env.py:279-285), as md_curriculum reported them for this step
            torch = e.torch
            rep_i = e.state_dev["cur_rep_i"].view(torch.int32).view(self.num_envs, 2)
            rep_f = e.state_dev["cur_rep_f"].view(torch.float64).view(self.num_envs, 3)
            eager.update(curriculum_level=rep_i[:, 0], curriculum_success=rep_f[:, 0], curriculum_route_completion=rep_f[:, 1],
                         data_coverage=rep_f[:, 2])
            lazy["scenario_difficulty"] = lambda: self._difficulty()[rep_i[:, 1].long()]
        return LazyInfo(eager, lazy)

    def _difficulty(self):
        e = self.engine
        if e._difficulty_dev is None:
            e._difficulty_dev = e.torch.as_tensor(e.host.difficulty, device=e.device)
        return e._difficulty_dev

    def _scenario_index(self):
        """[E] int64: the dataset index each env plays in this step (step_info["scenario_index"], envs/scenario_env.py:281).  In
        a walk the scene of the episode that this step belongs to: an env whose episode ended here has already been moved on
        (need_reset set, walk_ep advanced), so it reports episode walk_ep - need_reset."""
        e = self.engine
        torch = e.torch
        if not e.host.walk:
            return torch.as_tensor(np.asarray(e.host.seeds, np.int64), device=e.device)
        if e.host.curriculum[0] > 1:    # engine.current_seed: the position in the difficulty-sorted slice
            seed = e.state_dev["cur_rep_i"].view(torch.int32).view(self.num_envs, 2)[:, 1]
            return seed.long() + int(self.config["start_scenario_index"])
        from metadrive_ped_amd.scenario import walk_scene
        ep = e.state_dev["walk_ep"].view(torch.int32).cpu().numpy().astype(np.int64) - e.need_reset.cpu().numpy()
        p = walk_scene(self.config, np.arange(self.num_envs), np.maximum(ep, 0))
        return torch.as_tensor(int(self.config["start_scenario_index"]) + p, device=e.device)
