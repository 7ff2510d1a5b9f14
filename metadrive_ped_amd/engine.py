"""BatchedEngine: the host side of the batched step().  Owns every table and state array as
PyTorch-ROCm tensors (device memory + streams are torch's job; arithmetic is the HIP library's) and
drives the C-ABI.  Plays the role of BaseEngine + the manager chain for E lock-stepped worlds
(metadrive/engine/base_engine.py:306-478): reset() builds the scenes on the host with numpy
RandomState streams, step() is ONE md_step launch.

Sharding: an engine owns envs [env_seed_offset, env_seed_offset + num_envs) of the global batch;
env g uses scenario seed start_seed + g % num_scenarios, so results do not depend on how many
GPUs the batch is split over.
"""
import copy
import ctypes as C
import os
from collections import OrderedDict

import numpy as np

from metadrive_ped_amd import abi, hostpool
from metadrive_ped_amd.mapgen.pg import PGMap
from metadrive_ped_amd.mapgen.tables import MapTables, WorldTables, beam_table
from metadrive_ped_amd.obs_layout import ObsLayout
from metadrive_ped_amd.scene import EnvScene, HostSceneBase, step_state

STATE_ARRAY_SPECS = None  # filled below


# One wave per env beats the 4-wave workgroup when a LARGE batch shares few distinct maps: the lane / grid tables stay in L2, so
# the wave's serial chain of map reads is short, and all envs are resident at once.  Measured on the MI355X
# (tools/locality_probe.py, profiles/r03_step_kernel_by_maps.txt): 4096 envs on 1 / 8 / 16 / 32 maps 70-72 us against 83-86 us;
# even at 64 maps, behind at 512 (82.6 vs 79.2) and with a map per env (94 vs 87); at 1024 envs and below the workgroup kernel's
# shorter chain wins whatever the maps (38 vs 60 us).  The reference's default is num_scenarios = 1.
WAVE_KERNEL_MAX_MAPS = 32
WAVE_KERNEL_MIN_ENVS = 3072


def pick_step_kernel(cfg, n_maps):
    """config["step_kernel"] -> "wg" | "wave".  "auto": by the batch size and the number of distinct maps; MD_STEP_KERNEL in the
    environment overrides "auto" only (A/B runs) -- read HERE, once per engine, never inside the library."""
    want = cfg.get("step_kernel", "auto")
    if cfg.get("is_multi_agent") or cfg.get("scenario_mode"):
        return "wg"
    if want == "auto":
        env = os.environ.get("MD_STEP_KERNEL", "")
        if env in ("wg", "wave"):
            return env
        return "wave" if (n_maps <= WAVE_KERNEL_MAX_MAPS and int(cfg["num_envs"]) >= WAVE_KERNEL_MIN_ENVS) else "wg"
    return want


def _build_marl(cfg, scene_cfg, uniq):
    """Multi-agent maps (roundabout, intersection): one shared map, one scene per env seed."""
    from metadrive_ped_amd.mapgen.pg import (MABidirectionMap, MABottleneckMap, MAIntersectionMap, MAParkingLotMap, MARoundaboutMap,
                                             MATollGateMap)
    from metadrive_ped_amd.marl import FIXED_DESTINATION, SPAWN_ROADS, RoundaboutScene
    from metadrive_ped_amd.mapgen.tables import spawn_tables
    mc = cfg["map_config"]
    kind = cfg["marl_map"]
    if kind not in SPAWN_ROADS:
        raise NotImplementedError("multi-agent map {!r} is not built (built: {})".format(kind, sorted(SPAWN_ROADS)))
    if kind in ("bottleneck", "bidirection"):
        pg = (MABottleneckMap if kind == "bottleneck" else MABidirectionMap)(lane_num=mc["lane_num"], lane_width=mc["lane_width"], exit_length=mc["exit_length"],
                             neck_lane_num=mc["neck_lane_num"], neck_length=mc["neck_length"])
    elif kind == "parking_lot":
        pg = MAParkingLotMap(lane_num=mc["lane_num"], lane_width=mc["lane_width"], exit_length=mc["exit_length"],
                             parking_space_num=cfg["parking_space_num"])
    elif kind == "racing":
        from metadrive_ped_amd.mapgen.pg import RacingMap
        pg = RacingMap(lane_num=mc["lane_num"], lane_width=mc["lane_width"], exit_length=mc["exit_length"])
    elif kind == "tollgate":
        pg = MATollGateMap(lane_num=mc["lane_num"], lane_width=mc["lane_width"], exit_length=mc["exit_length"],
                           toll_lane_num=mc["toll_lane_num"], toll_length=mc["toll_length"])
    else:
        cls = dict(roundabout=MARoundaboutMap, intersection=MAIntersectionMap)[kind]
        kw = dict(radius=mc.get("radius")) if kind == "intersection" else {}
        pg = cls(lane_num=mc["lane_num"], lane_width=mc["lane_width"], exit_length=mc["exit_length"], **kw)
    mt = MapTables(pg)
    sc_cfg = dict(scene_cfg, exit_length=mc["exit_length"])
    fixed = FIXED_DESTINATION[kind]
    roads = _user_spawn_roads(cfg, mt) or SPAWN_ROADS[kind]
    parking, dests = None, None
    if kind == "parking_lot":
        from metadrive_ped_amd.marl import PARKING_IN_ROADS, parking_lot_roads
        if cfg.get("spawn_roads"):
            raise NotImplementedError("spawn_roads: the parking-lot env fills them itself (marl_parking_lot.py:194-203)")
        roads, dests = parking_lot_roads(cfg["parking_space_num"])
        assert [tuple(r) for r in pg.parking_space] == [(d[:-2] + "1_", d) for d in dests[:cfg["parking_space_num"]]]
        parking = (len(PARKING_IN_ROADS), cfg["parking_space_num"], dests)
    # MAIntersectionSpawnManager(disable_u_turn = lane_num < 2) (marl_intersection.py:73-85, :104): on the one-lane intersection a
    # vehicle is never sent back out of the arm it came in by
    no_u_turn = kind == "intersection" and mc["lane_num"] < 2
    sc_cfg["exclude_own_road"] = no_u_turn
    scenes = {s: RoundaboutScene(s, mt, sc_cfg, roads, fixed, parking) for s in uniq}
    return mt, scenes, spawn_tables(mt, roads, mc["lane_num"], fixed, dests, exclude_own_road=no_u_turn)


def _user_spawn_roads(cfg, mt):
    """config["spawn_roads"] (multi_agent_metadrive.py:27,84-92): the user's own list of (start node, end node) roads."""
    if not cfg.get("spawn_roads"):
        return None
    roads = [tuple(r) for r in cfg["spawn_roads"]]
    for r in roads:
        if len(r) != 2 or r not in mt.road_id:
            raise ValueError("spawn_roads: {!r} is not a road of this map".format(r))
    return roads


def _build_one_marl_pg(job):
    """MultiAgentMetaDrive on procedurally generated maps (envs/marl_envs/multi_agent_metadrive.py:12-61): one PG map per
    scenario seed like the single-agent env, agents spawn on the first block's exit road, destination = the far end."""
    from metadrive_ped_amd.mapgen.tables import spawn_tables
    from metadrive_ped_amd.marl import PG_SPAWN_ROADS, RoundaboutScene
    s, mc, dist, scene_cfg = job
    mt = copy.copy(_map_tables_for(s, mc, dist))   # the cached tables stay as generated
    roads = [tuple(r) for r in scene_cfg["spawn_roads"]] if scene_cfg.get("spawn_roads") else PG_SPAWN_ROADS
    mt.respawn = spawn_tables(mt, roads, mc["lane_num"], fixed_destination=True)   # stacked per map by WorldTables
    sc_cfg = dict(scene_cfg, exit_length=mc["exit_length"])
    return mt, RoundaboutScene(s, mt, sc_cfg, roads, True)


# Maps built by THIS process, by what they were generated from: a rebuild that only changes the scenes on them (random_traffic: new
# traffic at every env.reset(); another traffic density) does not generate them again.  The build workers are persistent and
# build_all keeps a job on the same worker (sticky), so their caches hit as well.
_MAP_CACHE = OrderedDict()
_MAP_CACHE_MAX = 512
MAPS_GENERATED = [0]          # what the cache did not have (tests read it)


def _map_tables_for(s, mc, dist):
    import pickle
    key = pickle.dumps((s, sorted(mc.items(), key=lambda kv: str(kv[0])), dist), protocol=4)
    mt = _MAP_CACHE.get(key)
    if mt is not None:
        _MAP_CACHE.move_to_end(key)
        return mt
    pg = PGMap(s, lane_num=mc["lane_num"], lane_width=mc["lane_width"], exit_length=mc["exit_length"],
               generate_type=mc["type"], generate_config=mc["config"], block_dist=dist)
    mt = MapTables(pg)
    MAPS_GENERATED[0] += 1
    _MAP_CACHE[key] = mt
    while len(_MAP_CACHE) > _MAP_CACHE_MAX:
        _MAP_CACHE.popitem(last=False)
    return mt


def _build_one(job):
    """One scenario seed -> (MapTables, EnvScene).  Module-level so that a fork pool can run it."""
    s, mc, dist, scene_cfg = job
    if scene_cfg.get("random_lane_width") or scene_cfg.get("random_lane_num"):
        # PGMapManager.add_random_to_map (manager/pg_map_manager.py:68-74): the map manager's stream, re-seeded with
        # the scenario index at every reset; width first, then the lane count
        from metadrive_ped_amd.rng import get_np_random
        rng = get_np_random(s)
        mc = dict(mc)
        if scene_cfg.get("random_lane_width"):
            mc["lane_width"] = float(rng.rand() * (4.5 - 3.0) + 3.0)     # MAX_LANE_WIDTH / MIN_LANE_WIDTH (base_map.py:38-39)
        if scene_cfg.get("random_lane_num"):
            mc["lane_num"] = int(rng.randint(2, 3 + 1))                   # MIN_LANE_NUM .. MAX_LANE_NUM (base_map.py:40-41)
    mt = _map_tables_for(s, mc, dist)
    if scene_cfg["traffic_mode"] in ("respawn", "hybrid") and abs(scene_cfg["traffic_density"]) >= 1e-2:
        from metadrive_ped_amd.mapgen.tables import respawn_tables
        mt = copy.copy(mt)                      # the cached tables stay as generated
        mt.respawn = respawn_tables(mt, s)
    return mt, EnvScene(s, mt, scene_cfg)


# what a scene hands to the batch per mover slot: (state array, EnvScene / RoundaboutScene field).  These are also the arrays
# md_swap_draw copies into an env that takes the next traffic draw or moves on to the next scene of a walk (BatchedEngine.DRAW_ARRAYS).
DRAW_FIELDS = (("shape0", "shape"), ("dyn0", "dyn"), ("nav0", "nav"), ("pid0", "pid"), ("param", "param"), ("route_nodes", "route_nodes"),
               ("route_roads", "route_roads"), ("final_lane", "final_lane"), ("idm_rand", "idm_rand"))


def _traffic_rng(of_seeds):
    """MdState.rng of the scenes `of_seeds`: xorshift32 needs a non-zero state; derive it from the scenario seed"""
    return np.asarray([((s * 2654435761) ^ 0x9E3779B9) & 0xFFFFFFFF or 1 for s in of_seeds], np.uint32)


class HostScene(HostSceneBase):
    """Host (numpy) copy of everything: world tables + reset snapshot.  Also what the tests hand to
    the CPU oracle."""
    def __init__(self, cfg):
        self.cfg = cfg
        self.E, self.A = cfg["num_envs"], cfg["num_agents"]
        ObsLayout(cfg, scenario=False).export_to(self)     # self.layout, and n_beams / n_side / n_ll / obs_base / ... / obs_dim
        self.cap = self._build_capacity()
        seeds, uniq, env_scene = self._assign_seeds()
        tables, map_of_seed = self._build(uniq, self._scene_config())
        if not cfg["is_multi_agent"]:
            self._trim_capacity()
        self._world_tables(tables, [map_of_seed[s] for s in seeds])
        self._state(seeds, env_scene)
        if self.walk:
            self._walk_pool(uniq)
        self._md_config(len(tables))
        self.set_detector_beams()

    def _build_capacity(self):
        """The slot count the scenes are built with.  Single-agent scenes are always generated with the maximum and cut to size
        afterwards (_trim_capacity); multi-agent ones with mover_capacity, or (0 = auto) a slot per agent."""
        cfg, A = self.cfg, self.A
        if not cfg["is_multi_agent"]:
            return abi.MD_MAX_CAP
        if cfg["mover_capacity"]:
            return cfg["mover_capacity"]
        if self.tollgate:     # + the toll booths (one on every odd lane of both directions), slots in multiples of 8
            return min(abi.MD_MAX_CAP, (A + 2 * (cfg["map_config"]["toll_lane_num"] // 2) + 7) // 8 * 8)
        return A

    def _assign_seeds(self):
        """-> (the scenario seed of every env, the seeds to build, the pool scene of every env or None).  The PG walk
        (walk_scenarios): the scene pool is every seed of the slice, built once whatever the env count; env e starts at the first
        scene of its walk (scenario.walk_scene), and md_swap_draw moves it on through the pool on the device."""
        cfg, E = self.cfg, self.E
        self.walk, self.pool, self.walk_params = bool(cfg.get("walk_scenarios")), None, (0, 0, 0, 0, 0)
        if not self.walk:
            self.seeds = [cfg["start_seed"] + ((cfg["env_seed_offset"] + e) % cfg["num_scenarios"]) for e in range(E)]
            return self.seeds, sorted(set(self.seeds)), None
        from metadrive_ped_amd.scenario import walk_params, walk_scene
        self.walk_params = walk_params(cfg)
        self.seeds = [cfg["start_seed"] + p for p in range(cfg["num_scenarios"])]   # names the slice, like ScenarioHostScene.seeds of a walk
        env_scene = [int(p) for p in walk_scene(cfg, np.arange(E), 0)]
        return [self.seeds[p] for p in env_scene], self.seeds, env_scene

    def _scene_config(self):
        """What EnvScene / RoundaboutScene read of the config (picklable: it travels to the build workers with the job)"""
        cfg, vc = self.cfg, self.cfg["vehicle_config"]
        scene_cfg = dict(cap=self.cap, agents_per_env=self.A, spawn_lane_index=cfg["agent_configs"]["default_agent"]["spawn_lane_index"],
                         agent_vehicle_model=vc["vehicle_model"], agent_size_mass={k: vc[k] for k in ("width", "length", "height", "mass")},
                         traffic_epoch=cfg.get("traffic_epoch", 0))
        scene_cfg.update({k: vc[k] for k in ("spawn_longitude", "spawn_lateral", "spawn_velocity", "spawn_velocity_car_frame", "destination")})
        scene_cfg.update({k: cfg[k] for k in (
            "physics_world_step_size", "random_spawn_lane_index", "traffic_density", "traffic_mode", "accident_prob",
            "static_traffic_object", "need_inverse_traffic", "random_lane_width", "random_lane_num", "random_agent_model",
            "random_dynamics", "initial_agents", "agent_policy", "spawn_roads", "random_traffic")})
        if cfg.get("num_pedestrians"):     # only then: a scene without pedestrians is built (and memoised) from the same job as before
            scene_cfg.update(num_pedestrians=int(cfg["num_pedestrians"]), pedestrian_config=dict(cfg["pedestrian_config"]))
        return scene_cfg

    def _build(self, uniq, scene_cfg):
        """Maps and scenes of the seeds `uniq` -> (the map tables, seed -> its map's index); sets self.scenes / map_tables / spawn.
        Reset-time host work goes to the persistent build workers (metadrive_ped_amd/hostpool.py): they are started before this
        process touches the GPU and kept; a process that already has a GPU context and no workers builds serially (it must not
        fork).  build_workers = 1 forces the serial path."""
        cfg = self.cfg
        self.spawn = None
        if cfg["is_multi_agent"] and cfg["marl_map"] != "pg":      # one shared map, one scene per seed
            mt, marl_scenes, self.spawn = _build_marl(cfg, scene_cfg, uniq)
            tables, map_of_seed, self.scenes = [mt], {s: 0 for s in uniq}, {s: marl_scenes[s] for s in uniq}
        else:
            build_fn = _build_one
            if cfg["is_multi_agent"]:
                build_fn = _build_one_marl_pg
                self.spawn = dict(n_dest=1)          # per-map spawn tables travel with the map tables
            jobs = [(s, dict(cfg["map_config"]), cfg["block_dist_config"], scene_cfg) for s in uniq]
            built = hostpool.build_all(build_fn, jobs, workers=int(cfg.get("build_workers", 0)), cache=bool(cfg.get("build_cache", False)),
                                       sticky=True)
            tables, map_of_seed = [mt for mt, _ in built], {s: i for i, s in enumerate(uniq)}
            self.scenes = {s: sc for s, (_, sc) in zip(uniq, built)}
        self.map_tables = tables
        return tables, map_of_seed

    def _trim_capacity(self):
        """Single-agent scenes are always generated with the maximum slot count and cut to size here (vehicles keep their low
        slots, props the top ones: the same arrays as a build at that size), so that one built scene serves every capacity -- the
        build memo keys on the job."""
        need = max(self.A + sc.n_traffic + sc.n_props for sc in self.scenes.values())
        cap = self.cfg["mover_capacity"] or min(abi.MD_MAX_CAP, max(8, (need + 7) // 8 * 8))
        if need > cap:
            raise ValueError("more than cap={} movers in an env ({}); raise `mover_capacity`".format(cap, need))
        for sc in self.scenes.values():
            sc.trim(cap)
        self.cap = cap

    def _world_tables(self, tables, env_map):
        cfg = self.cfg
        self.world = WorldTables(tables, env_map, beam_table(self.n_beams))
        a = self.world.arrays
        if self.spawn is not None and "spawn_lane" in self.spawn:      # the shared map's spawn tables
            a["spawn_off"] = np.asarray([0, len(self.spawn["spawn_lane"])], np.int32)
            for k in ("spawn_place", "spawn_lane", "spawn_route", "spawn_route_meta"):
                a[k] = np.ascontiguousarray(self.spawn[k])
        self.traffic_respawns = "spawn_off" in a and not cfg["is_multi_agent"]
        if cfg["is_multi_agent"] and cfg["random_agent_model"]:
            from metadrive_ped_amd.marl import vehicle_class_table
            a["vclass"] = vehicle_class_table(cfg["physics_world_step_size"])

    def _draw_rows(self, of_seeds):
        """The snapshot rows and per-slot constants (DRAW_FIELDS) of the scenes `of_seeds`, cap slots each"""
        d = {k: np.concatenate([getattr(self.scenes[s], field) for s in of_seeds], axis=0) for k, field in DRAW_FIELDS}
        # MdNav.road0 / road1: the road ids under the two route cursors, kept beside them (ABI v7) so that the per-step
        # logic never indexes the route arrays
        n = len(of_seeds) * self.cap
        rr = d["route_roads"].reshape(n, abi.MD_ROUTE_LEN)
        for road, ck in (("road0", "ck0"), ("road1", "ck1")):
            d["nav0"][road] = rr[np.arange(n), np.clip(d["nav0"][ck], 0, abi.MD_ROUTE_LEN - 1)]
        return d

    def _state(self, seeds, env_scene):
        cfg, E, A, cap = self.cfg, self.E, self.A, self.cap
        st = step_state(E, A, cap, self.obs_dim, self._draw_rows(seeds), env_scene)
        if cfg["is_multi_agent"] or self.traffic_respawns:
            # respawns (agents in MARL, traffic in the respawn / hybrid modes) rewrite routes and draw random numbers
            for k in ("route_nodes", "route_roads", "final_lane"):
                st[k + "0"] = st[k].copy()
            st["rng"] = _traffic_rng(seeds)
        if cfg["is_multi_agent"] and cfg["random_agent_model"]:
            st["param0"] = st["param"].copy()
        if cfg["is_multi_agent"]:
            st["env_steps"] = np.zeros(E, np.int32)
            st["agent_id"] = np.tile(np.arange(cap, dtype=np.int32), E)
            st["next_agent_id"] = np.full(E, cfg["initial_agents"] or A, np.int32)   # names agent0 .. agent{n-1} are taken
        if self.num_others > 0 or (cfg["agent_policy"] in ("ExpertPolicy", "AIProtectPolicy") and not cfg.get("expert_own_sensors")):
            # ExpertPolicy / AIProtectPolicy: the expert's own "others" block (num_others=4) is computed by md_expert from these sets; the env's
            # obs keeps its 259 dims (md_step tracks the sets whenever the array is there)
            st["detected"] = np.zeros((E * A, 2), np.uint64)
        if cfg["agent_policy"] == "AIProtectPolicy":
            # vehicle.takeover / vehicle.expert_takeover (base_vehicle.py:361,367), one byte per env: md_ai_protect's arguments, not MdState's
            st["takeover"] = np.zeros(E, np.uint8)
            st["expert_takeover"] = np.zeros(E, np.uint8)
        if cfg["is_multi_agent"] and cfg["marl_map"] == "racing":
            st["idle_ring"] = np.zeros((E * A, abi.MD_IDLE_WINDOW), np.float32)     # movement_between_steps of every agent
        self.state = st

    def _walk_pool(self, pool_seeds):
        """What md_swap_draw copies into an env that moves on to pool scene p: its rows at p * cap, and the scene's traffic
        stream (the reference re-seeds the traffic manager with the scenario seed at every reset)"""
        cfg = self.cfg
        self.pool = self._draw_rows(pool_seeds)
        if "rng" in self.state:
            self.pool["rng"] = _traffic_rng(pool_seeds)
        dev_bytes = sum(v.nbytes for v in self.world.arrays.values()) + sum(v.nbytes for v in self.pool.values())
        if dev_bytes > int(cfg["scenario_pool_max_bytes"]):
            raise ValueError("walk_scenarios: the pool of num_scenarios={} scenes needs {:.2f} GiB on the device (maps and snapshot "
                             "rows, mover capacity {}), more than scenario_pool_max_bytes={:.2f} GiB: walk a smaller slice".format(
                                 len(pool_seeds), dev_bytes / 2 ** 30, self.cap, int(cfg["scenario_pool_max_bytes"]) / 2 ** 30))
        print("walk_scenarios: scene pool of num_scenarios={} scenes (mover capacity {}): {:.1f} MiB on the device".format(
            len(pool_seeds), self.cap, dev_bytes / 2 ** 20), flush=True)

    def _md_config(self, n_maps):
        cfg = self.cfg
        k = make_md_config(cfg, self.layout, self.E, self.A, self.cap)
        k.random_agent_model = int(bool(cfg["random_agent_model"]))
        k.enable_reverse = int(bool(cfg["vehicle_config"]["enable_reverse"]))
        self.step_kernel = pick_step_kernel(cfg, n_maps)
        k.step_kernel = {"wg": 0, "wave": 1}[self.step_kernel]
        self.md_config = k


def make_md_config(cfg, layout, E, A, cap):
    """MdConfig of a batch: the sizes, the observation layout's counts (`layout`: the scene's ObsLayout) and what both env
    families read from the config; a host scene sets its own family's fields afterwards."""
    k = abi.MdConfig()
    k.struct_size = C.sizeof(abi.MdConfig)
    k.n_envs, k.agents_per_env, k.cap = E, A, cap
    k.n_beams, k.n_side, k.n_lane_line, k.obs_dim = layout.n_beams, layout.n_side, layout.n_ll, layout.obs_dim
    k.num_others, k.add_others_navi = layout.num_others, int(layout.add_others_navi)
    k.agent_idm = {"IDMPolicy": abi.AGENT_IDM, "LaneChangePolicy": abi.AGENT_LANE_CHANGE}.get(cfg["agent_policy"], abi.AGENT_INPUT)
    k.substeps = int(cfg["decision_repeat"])
    k.horizon = int(cfg["horizon"]) if cfg["horizon"] else 0
    k.dt = float(cfg["physics_world_step_size"])
    k.lidar_range = float(cfg["vehicle_config"]["lidar"]["distance"])
    for name in ("success_reward", "out_of_road_penalty", "crash_vehicle_penalty", "crash_object_penalty",
                 "driving_reward", "speed_reward", "crash_vehicle_cost", "crash_object_cost", "out_of_road_cost"):
        setattr(k, name, float(cfg[name]))
    for name in ("use_lateral_reward", "out_of_route_done", "on_continuous_line_done", "crash_vehicle_done",
                 "crash_object_done", "crash_human_done", "truncate_as_terminate", "enable_idm_lane_change",
                 "auto_reset"):
        setattr(k, name, int(bool(cfg[name])))
    # density ~ 0: PGTrafficManager.reset returns before any mode-specific set-up (traffic_manager.py:62-63)
    k.traffic_mode = {"trigger": 0, "respawn": 1, "hybrid": 2, "replay": 3}[cfg["traffic_mode"]] \
        if abs(cfg["traffic_density"]) >= 1e-2 else 0
    k.max_lane_width = 4.5      # BaseMap.MAX_LANE_WIDTH (component/map/base_map.py:38)
    k.total_width = (3 + 1) * 4.5  # (MAX_LANE_NUM + 1) * MAX_LANE_WIDTH (obs/state_obs.py:92)
    k.curve_radius_max = 60.0   # BlockParameterSpace.CURVE radius max
    k.curve_angle_max = 135.0
    k.is_multi_agent = int(bool(cfg["is_multi_agent"]))
    k.delay_done = int(cfg["delay_done"])
    k.allow_respawn = int(bool(cfg["allow_respawn"]))
    k.crash_done = int(bool(cfg["crash_done"]))
    k.out_of_road_done = int(bool(cfg["out_of_road_done"]))
    if cfg["is_multi_agent"] and cfg["marl_map"] == "parking_lot":
        k.ma_kind = abi.MA_PARKING_LOT
        k.n_parking = int(cfg["parking_space_num"])
    if cfg["is_multi_agent"] and cfg["marl_map"] == "racing":
        k.ma_kind = abi.MA_RACING
        k.crash_sidewalk_penalty, k.idle_penalty = float(cfg["crash_sidewalk_penalty"]), float(cfg["idle_penalty"])
        k.idle_done, k.crash_sidewalk_done = int(bool(cfg["idle_done"])), int(bool(cfg["crash_sidewalk_done"]))
    if cfg["is_multi_agent"] and cfg["marl_map"] == "tollgate":
        k.ma_kind = abi.MA_TOLLGATE
        k.min_pass_steps = int(cfg["vehicle_config"]["min_pass_steps"])
        k.overspeed_penalty = float(cfg["overspeed_penalty"])
        k.on_continuous_line_done = int(bool(cfg["cross_yellow_line_done"]))   # _is_out_of_road (marl_tollgate.py:241-247)
    return k


def make_structs(world_arrays, state_arrays, md_config, n_maps, n_envs, ptr_of):
    """(MdWorld, MdState, MdConfig) over the arrays wherever they live (ptr_of(array) -> address); `world_arrays` also holds the
    host scene's world_scalars()."""
    w = abi.MdWorld()
    w.n_maps, w.n_envs = n_maps, n_envs
    abi.fill_struct(w, abi.WORLD_FIELDS, world_arrays, ptr_of)
    lane_off = np.asarray(world_arrays["lane_off_host"])
    road_off = np.asarray(world_arrays["road_off_host"])
    w.max_lanes = int(np.diff(lane_off).max())
    w.max_roads = int(np.diff(road_off).max())
    w.n_dest = int(world_arrays.get("n_dest_host", 0))
    w.n_vclass = int(world_arrays.get("n_vclass_host", 0))
    s = abi.MdState()
    abi.fill_struct(s, abi.STATE_FIELDS, state_arrays, ptr_of)
    return w, s, md_config


class _NullCtx:
    def __enter__(self):
        return self

    def __exit__(self, *a):
        return False


_NULL_CTX = _NullCtx()
# the row blocks' numpy dtypes -> the torch dtype of their views, by name (torch is imported with the first engine)
_TORCH_DTYPE = {np.dtype(np.float32): "float32", np.dtype(np.int32): "int32", np.dtype(np.uint8): "uint8"}


def _ptr(t):
    """A tensor's address as a C-ABI pointer argument; None -> NULL"""
    return C.c_void_p(t.data_ptr() if t is not None else None)


class BatchedEngine:
    def __init__(self, cfg, host=None):
        import torch
        from metadrive_ped_amd import _lib
        self.torch = torch
        self.lib = _lib.load()
        self._check = _lib.check
        self.cfg = cfg
        self.device = torch.device(cfg["device"])
        self._dev_index = self.device.index if self.device.index is not None else 0
        if self.device.type != "cuda":
            raise _lib.MdStepError("BatchedEngine needs a ROCm device (config['device']={!r}); there is no CPU "
                                   "fallback".format(cfg["device"]))
        self.host = host
        self._noise_gen = None
        self._expert_gen = None
        self._expert_w = None
        self._expert_beams = None
        self._track_det = False
        self._clear_buffers()
        self._rec = None
        self._branch_owner = object()    # names this engine in the env snapshots it makes (branch.py), across rebuilds
        self._tracks = None
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
            self._dev_index = self.device.index
        self.build()

    def _clear_buffers(self):
        """Per-engine buffers made on first use; a build() drops them with the batch they were sized for."""
        self._expert_action = None      # step(): the expert's action, ExpertPolicy
        self._protect_action = None     # ai_protect_forward: the applied action ...
        self.protect_flags = None       # ... and its flag bytes; None before the first protected step
        self._difficulty_dev = None     # BatchedScenarioEnv: the pool's difficulty scores on the device

    # -- upload helpers ---------------------------------------------------------------------------
    def _to_dev(self, arr):
        t = self.torch.from_numpy(np.ascontiguousarray(arr).view(np.uint8).reshape(-1))
        return t.to(self.device)

    DRAW_ARRAYS = tuple(k for k, _ in DRAW_FIELDS)
    DRAW_EPOCH_STRIDE = 4099          # traffic_epoch of draw k = the env's epoch + k * stride

    def n_traffic_draws(self):
        """random_traffic with envs that reset themselves: how many traffic draws are staged on the device (md_swap_draw)."""
        c = self.cfg
        if c.get("scenario_mode") or c["is_multi_agent"] or not (c["random_traffic"] and c["auto_reset"]):
            return 1
        return max(1, int(c.get("traffic_draws", 1)))

    def _draw_cfg(self, k, cap=None):
        c = dict(self.host.cfg if self.host is not None else self.cfg)
        c["traffic_epoch"] = int(c.get("traffic_epoch", 0)) + k * self.DRAW_EPOCH_STRIDE
        if cap is not None:
            c["mover_capacity"] = cap
        return c

    def rebuild(self, cfg):
        """Drop the host scene and build() again from `cfg` (a new start_seed, a new traffic draw)."""
        self.host = None
        self.cfg = cfg
        self.build()

    def build(self):
        """(Re)generate maps + scenes on the host and upload.  BaseEnv.reset's map/agent/traffic managers."""
        torch = self.torch
        self._clear_buffers()
        self._branch_token = object()    # env snapshots (branch.py) belong to one build of the batch
        self._branch_idx = OrderedDict() # their latest index lists, on the device
        K = self.n_traffic_draws()
        draws = None
        if self.host is None:
            self.host = HostScene(self.cfg)
            if K > 1 and not self.cfg["mover_capacity"]:
                # the draws share one capacity: the largest any of them needs (the maps are cached per process, the scenes are cheap)
                draws = [HostScene(self._draw_cfg(k)) for k in range(1, K)]
                need = max([self.host.cap] + [d.cap for d in draws])
                if self.host.cap != need:
                    self.host = HostScene(dict(self.cfg, mover_capacity=need))
                draws = [d if d.cap == need else HostScene(self._draw_cfg(k + 1, need)) for k, d in enumerate(draws)]
        if K > 1 and draws is None:      # a host handed in, or a fixed capacity: every draw must fit it (ValueError names the capacity)
            draws = [HostScene(self._draw_cfg(k, self.host.cap)) for k in range(1, K)]
        self.draw_hosts_ = [self.host] + (draws or [])
        h = self.host
        if self._track_det and "detected" not in h.state:       # expert() was called on this engine before a rebuild
            h.state["detected"] = np.zeros((h.E * h.A, 2), np.uint64)
        self.E, self.A, self.cap = h.E, h.A, h.cap
        self.n_beams, self.obs_dim = h.n_beams, h.obs_dim
        self.world_dev = {k: self._to_dev(v) for k, v in h.world.arrays.items()}
        self.state_dev = {k: self._to_dev(v) for k, v in h.state.items()}
        self._pack_step_outputs()
        ptr = lambda t: t.data_ptr()
        wd = dict(self.world_dev, **h.world_scalars())
        self._side_beams = self._to_dev(h.side_beams) if h.side_beams is not None else None
        self._ll_beams = self._to_dev(h.ll_beams) if h.ll_beams is not None else None
        # scenario mode: md_step runs the side / lane-line detectors itself (MdWorld.side_beam_cs / ll_beam_cs) on waves that
        # idle while the agent is observed; the other modes call md_line_detector after md_step
        self._fused_detectors = bool(self.cfg.get("scenario_mode")) and (h.n_side > 0 or h.n_ll > 0)
        if self._fused_detectors:
            vc = self.cfg["vehicle_config"]
            if self._side_beams is not None:
                wd["side_beam_cs"] = self._side_beams
            if self._ll_beams is not None:
                wd["ll_beam_cs"] = self._ll_beams
            h.md_config.side_range = float(vc["side_detector"]["distance"])
            h.md_config.ll_range = float(vc["lane_line_detector"]["distance"])
            h.md_config.side_mask, h.md_config.ll_mask = self.SIDE_MASK, self.LANE_LINE_MASK
        self.w, self.s, self.k = make_structs(wd, self.state_dev, h.md_config, h.world.n_maps, h.E, ptr)
        # random_traffic: the staged draws (md_swap_draw after every step hands an env that finished its episode the next one)
        self._staged = None
        if K > 1:
            hosts = self.draw_hosts_
            names = [k for k in self.DRAW_ARRAYS if k in h.state]
            self._staged_dev = {k: self._to_dev(np.stack([np.ascontiguousarray(x.state[k]).view(np.uint8).reshape(-1) for x in hosts])) for k in names}
            self._staged = abi.MdState()
            abi.fill_struct(self._staged, abi.STATE_FIELDS, self._staged_dev, ptr)
            self.draw_idx = torch.zeros(self.E, dtype=torch.int32, device=self.device)
        # the scenario walk: the staged "draws" are the scene pool's snapshot rows; the env's scene index is its line map
        # (MdWorld.env_map), which md_swap_draw rewrites together with MdState.scene_of / walk_ep
        self._walk = getattr(h, "pool", None) is not None
        if self._walk:
            self.s.walk = abi.MdWalk(*h.walk_params)
            self._staged_dev = {k: self._to_dev(v) for k, v in h.pool.items()}
            self._staged = abi.MdState()
            abi.fill_struct(self._staged, abi.STATE_FIELDS, self._staged_dev, ptr)
            self.draw_idx = self.world_dev["env_map"]
            self._n_draws = int(h.walk_params[0])
        elif self._staged is not None:
            self._n_draws = len(self.draw_hosts_)
        # the curriculum of a walk (include/md_curriculum.h): md_curriculum after every step; with more than one level it moves
        # the envs itself, instead of md_swap_draw
        self._cur = None
        if self._walk and getattr(h, "curriculum", None) is not None:     # scenario mode; the PG walk has no curriculum
            L, per, Q, target = h.curriculum
            n, _, W, off, _ = h.walk_params
            cu = abi.MdCurriculum()
            abi.fill_struct(cu, abi.CURRICULUM_FIELDS, {f: self.state_dev["cur_" + f] for f in abi.CURRICULUM_FIELDS}, ptr)
            cu.n_levels, cu.per_level, cu.eval, cu.n_scenes, cu.stride, cu.offset = L, per, Q, n, W, off
            cu.cover_words, cu.target = (n + 31) // 32, target
            self._cur = cu
        sd = self.state_dev
        # typed views for the env API
        self.obs = sd["obs"].view(torch.float32).view(self.E, self.A, self.obs_dim)
        self.reward = sd["reward"].view(torch.float32).view(self.E, self.A)
        self.cost = sd["cost"].view(torch.float32).view(self.E, self.A)
        self.flags = sd["flags"].view(torch.int32).view(self.E, self.cap)
        self.action = sd["action"].view(torch.float32).view(self.E, self.cap, 2)
        self.step_info = sd["step_info"].view(torch.float32).view(self.E, self.A, 8)
        self.done_tt = sd["done_out"].view(torch.bool).view(self.E, self.A, 4)[:, :, 0:2] if "done_out" in sd else None
        self.step_flags = sd["done_out"].view(torch.int16).view(self.E, self.A, 2)[:, :, 1] if "done_out" in sd else None   # MD_FL_* of the step
        self.need_reset = sd["need_reset"].view(torch.int32)
        self.shape_f = sd["shape"].view(torch.float32).view(self.E, self.cap, 8)
        self.dyn_f = sd["dyn"].view(torch.float32).view(self.E, self.cap, 8)
        self.nav_i = sd["nav"].view(torch.int32).view(self.E, self.cap, 16)
        # crossing pedestrians (include/md_ped.h): md_ped's argument block; None = no launch
        self._ped = abi.make_md_ped(self.cfg["pedestrian_config"]) if self.cfg.get("num_pedestrians") else None
        # contact response (include/md_contact_response.h): md_contact_response's argument block; None = no launch
        self._cr = abi.make_md_contact_response(self.cfg["contact_response_config"]) if self.cfg.get("contact_response") else None
        self.agent_id = sd["agent_id"].view(torch.int32).view(self.E, self.cap) if "agent_id" in sd else None
        self._topdown_setup()
        self._vector_obs_setup()
        self._scenario_vector_obs_setup()
        self._traffic_lights_setup()
        self._scenario_metrics_setup()
        if getattr(h, "tracks", None) is not None:     # scenario mode: the scenes' recorded frames come with the host scene
            tr = h.tracks
            self.set_tracks(dict(shape=torch.from_numpy(np.ascontiguousarray(tr["shape"]).view(np.uint8).reshape(tr["shape"].shape[0], -1)),
                                 dyn=torch.from_numpy(np.ascontiguousarray(tr["dyn"])), seeds=tr["seeds"], cap=tr["cap"]))

    def _topdown_setup(self):
        """The top-down observation envs (config keys resolution_size ...; include/md_topdown.h): the image tensor
        [E, R, R, 2 + frame_stack] and the engine-owned history -- the 1-bit traffic frames, the past positions and the cursors --
        md_topdown's arguments, not MdState's.  self.topdown is None for every other env."""
        torch, cfg = self.torch, self.cfg
        self._td = self.topdown = self.topdown_dev = None
        if "resolution_size" not in cfg:
            return
        if cfg.get("scenario_mode") or self.A != 1:
            raise NotImplementedError("the top-down observation is built for the single-agent PG envs")
        R, stack, skip = int(cfg["resolution_size"]), int(cfg["frame_stack"]), int(cfg["frame_skip"])
        norm = bool(cfg["norm_pixel"])
        Lt, Lp = abi.td_ring_len(stack, skip), abi.td_ring_len(int(cfg["post_stack"]), skip)
        self.topdown = torch.zeros((self.E, R, R, 2 + stack), dtype=torch.float32 if norm else torch.uint8, device=self.device)
        self.topdown_dev = dict(ring_traffic=torch.zeros((self.E, Lt, R, abi.td_row_words(R)), dtype=torch.int32, device=self.device),
                                ring_pos=torch.zeros((self.E, Lp, 2), dtype=torch.float32, device=self.device),
                                cursor=torch.zeros((self.E, 4), dtype=torch.int32, device=self.device))
        td = abi.MdTopDown()
        td.struct_size, td.resolution, td.distance = C.sizeof(abi.MdTopDown), R, float(cfg["distance"])
        td.frame_stack, td.frame_skip, td.post_stack, td.norm_pixel = stack, skip, int(cfg["post_stack"]), int(norm)
        td.out = self.topdown.data_ptr()
        for k, t in self.topdown_dev.items():
            setattr(td, k, t.data_ptr())
        self._td = td

    def _row_blocks(self, table, row_bytes):
        """One zeroed [E, row_bytes] uint8 device tensor laid out by `table` (abi.row_blocks) -> (the tensor, name -> typed view
        [E, ...] of its block, name -> device address of env 0's block).  A block without bytes has an empty view and no address."""
        rows = self.torch.zeros((self.E, row_bytes), dtype=self.torch.uint8, device=self.device)
        views = OrderedDict()
        for name, (off, shape, dt) in table.items():
            block = rows[:, off:off + abi.block_bytes(table, name)]
            views[name] = block.view(getattr(self.torch, _TORCH_DTYPE[dt])).view((self.E, ) + shape)
        return rows, views, abi.block_ptrs(table, rows.data_ptr())

    def _vector_obs_setup(self):
        """The vector scene observation (config vector_obs; include/md_vector_obs.h): TWO allocations with one row per env -- the ten
        output blocks, and the engine-owned history (pose ring, flag ring, cursor) -- md_vector_obs's arguments, not MdState's.
        self.vector_obs_out holds the blocks as typed views [E, A, ...] of the output rows.  All None when the key is None."""
        vo = self.cfg.get("vector_obs")
        self._vo = self.vector_obs_out = self.vector_obs_rows = self.vector_obs_hist = None
        if vo is None:
            return
        if self.cfg.get("scenario_mode"):
            raise NotImplementedError("vector_obs is not built for BatchedScenarioEnv")
        outs, out_bytes, hist, hist_bytes = abi.vector_obs_blocks(vo, self.A, self.cap)
        self.vector_obs_rows, self.vector_obs_out, ptrs = self._row_blocks(outs, out_bytes)
        self.vector_obs_hist, _, hist_ptrs = self._row_blocks(hist, hist_bytes)
        self._vo_blocks = (outs, hist)
        self._vo = abi.make_md_vector_obs(vo, dict(ptrs, out_stride=out_bytes, hist_stride=hist_bytes, **hist_ptrs))

    def _scenario_vector_obs_setup(self):
        """The vector scene observation of scenario mode (config scenario_vector_obs; include/md_scenario_vector_obs.h): the same TWO
        allocations with one row per env as _vector_obs_setup makes -- the ten output blocks (self.vector_obs_out: typed views [E, ...]),
        and the engine-owned history -- plus the per-scene map piece table the host scene built (ScenarioHostScene.map_pieces),
        uploaded once.  md_scenario_vector_obs's arguments, not MdState's or MdWorld's.  self._svo is None when the key is None."""
        vo = self.cfg.get("scenario_vector_obs")
        self._svo = self.scenario_map_dev = None
        if vo is None:
            return
        outs, out_bytes, hist, hist_bytes = abi.scenario_vector_obs_blocks(vo, self.cap)
        self.vector_obs_rows, self.vector_obs_out, ptrs = self._row_blocks(outs, out_bytes)
        self.vector_obs_hist, _, hist_ptrs = self._row_blocks(hist, hist_bytes)
        ptrs.update(hist_ptrs, out_stride=out_bytes, hist_stride=hist_bytes, max_pieces=0)
        pieces = getattr(self.host, "map_pieces", None)
        if int(vo["num_pieces"]) > 0:
            if pieces is None:
                raise RuntimeError("scenario_vector_obs: the host scene carries no map piece table (it was built without the key)")
            self.scenario_map_dev = {k: self._to_dev(pieces[k]) for k in abi.SCENARIO_VECTOR_OBS_TABLES}
            ptrs.update({k: t.data_ptr() for k, t in self.scenario_map_dev.items()}, max_pieces=pieces["max_pieces"])
        self._vo_blocks = (outs, hist)
        self._svo = abi.make_md_scenario_vector_obs(vo, ptrs)

    def _traffic_lights_setup(self):
        """The traffic lights of scenario mode (config traffic_lights; include/md_traffic_lights.h): ONE allocation with one row per env
        for the four output blocks (self.traffic_lights_out: typed views [E, ...]) and the per-scene light tables the host scene built
        (ScenarioHostScene.traffic_lights), uploaded once.  md_traffic_lights's arguments, not MdState's or MdWorld's.  self._tl is
        None, and nothing is allocated, when the key is None."""
        tl = self.cfg.get("traffic_lights")
        self._tl = self.traffic_lights_rows = self.traffic_lights_out = self.traffic_lights_dev = None
        if tl is None or not self.cfg.get("scenario_mode"):
            return
        tables = getattr(self.host, "traffic_lights", None)
        if tables is None:
            raise RuntimeError("traffic_lights: the host scene carries no light tables (it was built without the key)")
        outs, out_bytes = abi.traffic_lights_blocks(tl)
        self.traffic_lights_rows, self.traffic_lights_out, ptrs = self._row_blocks(outs, out_bytes)
        self.traffic_lights_dev = {k: self._to_dev(tables[k]) for k in abi.TRAFFIC_LIGHTS_TABLES}
        ptrs.update({k: t.data_ptr() for k, t in self.traffic_lights_dev.items()}, out_stride=out_bytes,
                    max_scene_lights=tables["max_scene_lights"])
        self._tl = abi.make_md_traffic_lights(tl, ptrs)

    def _scenario_metrics_setup(self):
        """The closed-loop driving metrics of scenario mode (config scenario_metrics; include/md_scenario_metrics.h): ONE allocation with
        one row per env for the output blocks and ONE for the history with the running episode's accumulators
        (self.scenario_metrics_out: typed views [E, ...] of both).  md_scenario_metrics's arguments, not MdState's or MdWorld's; it reads
        md_traffic_lights' agent_light where the lights are configured.  self._sm is None, and nothing is allocated, when the key is
        None."""
        sm = self.cfg.get("scenario_metrics")
        self._sm = self.scenario_metrics_rows = self.scenario_metrics_state = self.scenario_metrics_out = None
        if sm is None or not self.cfg.get("scenario_mode"):
            return
        outs, out_bytes, state, state_bytes = abi.scenario_metrics_blocks(sm)
        self.scenario_metrics_rows, self.scenario_metrics_out, ptrs = self._row_blocks(outs, out_bytes)
        self.scenario_metrics_state, state_views, _ = self._row_blocks(state, state_bytes)
        self.scenario_metrics_out.update(state_views)
        ptrs.update(out_stride=out_bytes, state_stride=state_bytes, state=self.scenario_metrics_state.data_ptr())
        if self._tl is not None:
            ptrs.update(agent_light=self.traffic_lights_out["agent_light"].data_ptr(), light_stride=self._tl.out_stride)
        self._sm = abi.make_md_scenario_metrics(sm, ptrs)

    def scenario_metrics_forget(self):
        """Zero the metrics: the step columns, the history, the accumulators, last_episode and episodes (env.reset; env.set_state: a
        checkpoint does not carry them)"""
        if self._sm is not None:
            self.scenario_metrics_rows.zero_()
            self.scenario_metrics_state.zero_()

    def vector_obs_history(self):
        """The vector observation's history as host numpy copies: ring_pose [E, T, cap, 4], ring_flags [E, T, cap], cursor [E, 4]
        (the tests compare them)"""
        rows = self.vector_obs_hist.cpu().numpy()
        return {name: abi.block_of(rows, self._vo_blocks[1], name) for name in self._vo_blocks[1]}

    def vector_obs_forget(self):
        """Empty every env's history (env.set_state: a checkpoint does not carry it, like the renderer's)"""
        if self.vector_obs_hist is not None:
            self.vector_obs_hist.zero_()

    def topdown_history(self):
        """The top-down history arrays as host numpy copies: ring_traffic, ring_pos, cursor (the tests compare them; the top-down
        envs' get_state() carries them and set_state() puts them back through upload_topdown_history)"""
        return {k: t.cpu().numpy().copy() for k, t in self.topdown_dev.items()}

    def upload_topdown_history(self, arrays):
        """The arrays of topdown_history(), back onto the device (env.set_state)"""
        for k, v in arrays.items():
            t = self.topdown_dev[k]
            t.copy_(self.torch.from_numpy(np.ascontiguousarray(v)).to(t.dtype).view_as(t))

    def _pack_step_outputs(self):
        """obs | reward | done_out (terminated, truncated, step flags) of this rank in ONE allocation, in that order, each part
        16-byte aligned: the kernel writes the three arrays where it always did, and the whole step output of the shard is one
        contiguous slab -- the single collective of SURVEY 8(e) (sharding.gather_step_slab) moves it as it lies."""
        torch = self.torch
        sd = self.state_dev
        names = [k for k in ("obs", "reward", "done_out") if k in sd]
        layout, at = {}, 0
        for k in names:
            layout[k] = (at, sd[k].numel())
            at = (at + sd[k].numel() + 15) // 16 * 16
        slab = torch.zeros(at, dtype=torch.uint8, device=self.device)
        for k in names:
            o, n = layout[k]
            view = slab[o:o + n]
            view.copy_(sd[k])
            sd[k] = view
        self.out_slab, self.out_layout = slab, layout

    def _stream(self):
        return C.c_void_p(self.torch.cuda.current_stream(self.device).cuda_stream)

    def _launch(self, name, *args):
        """One C-ABI launch on the engine's batch: md_<name>(&world, &state, &config, *args, stream), checked.  The caller is
        inside _on_device()."""
        self._check(getattr(self.lib, name)(C.byref(self.w), C.byref(self.s), C.byref(self.k), *args, self._stream()), name)

    def _on_device(self):
        """Context in which HIP's current device is the engine's (config["device"]): a no-op object when it already is
        (the usual one-process-per-GPU case), torch.cuda.device(...) otherwise -- a launch must not land on another
        device's stream because the caller's current device differs."""
        cuda = self.torch.cuda
        if cuda.current_device() == self._dev_index:
            return _NULL_CTX
        return cuda.device(self._dev_index)

    def reset(self):
        """All envs back to their reset snapshot; returns after the reset observation is computed.
        (BaseEnv.reset -> engine.reset -> _get_reset_return, envs/base_env.py:502-584)"""
        self.need_reset.fill_(1)
        if self._walk:     # every env back to the first scene of its walk (episode 0), then the reset step
            self.state_dev["walk_ep"].view(self.torch.int32).fill_(-1)
            with self._on_device():
                if self._cur is None or self._cur.n_levels == 1:
                    self._swap()
                if self._cur is not None:
                    self._curriculum(1)     # the level check; more than one level: the first scene of the env's level
        self.step_raw()

    def _curriculum(self, reset):
        self._check(self.lib.md_curriculum(C.byref(self.s), C.byref(self._staged), C.byref(self.k), C.byref(self._cur),
                                           C.c_void_p(self.draw_idx.data_ptr()), int(reset), self._stream()), "md_curriculum")

    def _swap(self):
        self._check(self.lib.md_swap_draw(C.byref(self.s), C.byref(self._staged), C.byref(self.k), self._n_draws,
                                          C.c_void_p(self.draw_idx.data_ptr()), self._stream()), "md_swap_draw")

    SIDE_MASK = (1 << abi.Q_LINE_WHITE_CONT) | (1 << abi.Q_LINE_YELLOW_CONT)      # CollisionGroup.ContinuousLaneLine
    LANE_LINE_MASK = SIDE_MASK | (1 << abi.Q_LINE_BROKEN)                         # ... | BrokenLaneLine

    def step_raw(self):
        with self._on_device():
            self._step_raw()

    def _step_raw(self):
        if self._cr is not None:         # vehicles out of what the previous step drove them into; the pedestrians judge the corrected ones
            self._check(self.lib.md_contact_response(C.byref(self.s), C.byref(self.k), C.byref(self._cr), self._stream()), "md_contact_response")
        if self._ped is not None:       # the pedestrians' policy on the state the previous step left, then the world steps
            self._check(self.lib.md_ped(C.byref(self.s), C.byref(self.k), C.byref(self._ped), self._stream()), "md_ped")
        self._launch("md_step")
        L = self.host.layout
        vc = self.cfg["vehicle_config"]
        obs = self.state_dev["obs"]
        if self._fused_detectors:        # md_step ran them itself
            pass
        elif L.n_side and L.n_ll and L.n_side + L.n_ll <= 255:
            # both detector clouds in ONE launch and one pass over the line pieces (md_line_detectors)
            self._launch("md_line_detectors",
                         _ptr(self._side_beams), L.n_side, C.c_float(float(vc["side_detector"]["distance"])), C.c_uint32(self.SIDE_MASK), L.side_off,
                         _ptr(self._ll_beams), L.n_ll, C.c_float(float(vc["lane_line_detector"]["distance"])), C.c_uint32(self.LANE_LINE_MASK),
                         L.ll_off, _ptr(obs), L.obs_dim)
        else:
            if L.n_side:     # SideDetector cloud replaces obs[0:2] (obs/state_obs.py:77-86)
                self.line_detector(self._side_beams, L.n_side, float(vc["side_detector"]["distance"]), self.SIDE_MASK, obs, L.obs_dim, L.side_off)
            if L.n_ll:       # LaneLineDetector cloud replaces the lateral dim (obs/state_obs.py:129-140)
                self.line_detector(self._ll_beams, L.n_ll, float(vc["lane_line_detector"]["distance"]), self.LANE_LINE_MASK, obs, L.obs_dim,
                                   L.ll_off)
        self._lidar_noise()
        if self._td is not None:         # the top-down image of the state this step left, on the map of the episode it belongs to
            self._launch("md_topdown", C.byref(self._td))
        if self._vo is not None:         # the vector scene observation, likewise: a walking env's last frame is traced on the old map
            self._launch("md_vector_obs", C.byref(self._vo))
        if self._svo is not None:        # scenario mode's: before the walk's swap and the curriculum move an env on to another scene
            self._launch("md_scenario_vector_obs", C.byref(self._svo))
        if self._tl is not None:         # the traffic lights, likewise: a walking env's last frame is read on its own scene's lights
            self._launch("md_traffic_lights", C.byref(self._tl))
        if self._sm is not None:         # the driving metrics: after the lights (they read agent_light), and before an env moves on, so
            self._launch("md_scenario_metrics", C.byref(self._sm))     # that its last frame is scored on its own scene's SDC track
        # Only now, with the step's observation complete, do the envs whose episode just ended move on: the swap of a walk rewrites
        # MdWorld.env_map, and the detector launches above trace the map of the episode that ended
        if self._cur is not None:        # the scenario walk: the curriculum's step, and the envs whose episode just ended move on
            if self._cur.n_levels == 1:
                self._swap()
            self._curriculum(0)
        elif self._staged is not None:   # random_traffic / the PG walk: the envs whose episode just ended get the next draw / scene
            self._swap()
        if self._rec is not None:
            self._record_frame()

    # -- record / replay of the traffic (the role of RecordManager / ReplayManager for the movers of the batch,
    #    manager/record_manager.py:35-135, manager/replay_manager.py:21-195, policy/replay_policy.py:43-67) ---------
    def start_recording(self, max_steps):
        """Call right after reset(): frame 0 is the reset state, frame k the state after the k-th step.  Frames are
        device tensors (32 + 8 bytes per slot and step); recording stops by itself when the buffer is full."""
        torch = self.torch
        if self._walk and not self.cfg.get("scenario_mode"):
            raise NotImplementedError("start_recording with walk_scenarios=True: the recorded frames belong to one scenario assignment; "
                                      "record a batch without the walk")
        n = self.E * self.cap
        self._rec = dict(shape=torch.empty((max_steps + 1, n * 32), dtype=torch.uint8, device=self.device),
                         dyn=torch.empty((max_steps + 1, n, 2), dtype=torch.float32, device=self.device), n=0)
        self._record_frame()

    def _record_frame(self):
        r = self._rec
        if r["n"] >= r["shape"].shape[0]:
            return
        r["shape"][r["n"]].copy_(self.state_dev["shape"])
        r["dyn"][r["n"], :, 0].copy_(self.dyn_f.reshape(-1, 8)[:, 0])      # heading
        r["dyn"][r["n"], :, 1].copy_(self.dyn_f.reshape(-1, 8)[:, 1])      # speed
        r["n"] += 1

    def stop_recording(self):
        """-> dict(shape=[T, E*cap*32] uint8, dyn=[T, E*cap, 2] float32, seeds=...) of the T recorded frames."""
        r, self._rec = self._rec, None
        return dict(shape=r["shape"][:r["n"]].contiguous(), dyn=r["dyn"][:r["n"]].contiguous(),
                    seeds=list(self.host.seeds), cap=self.cap)

    def set_tracks(self, tracks):
        """traffic_mode 'replay': every non-agent slot follows these recorded frames (episode step k -> frame k; the
        last frame is held afterwards).  The tracks must come from the same scenario assignment and capacity."""
        if list(tracks["seeds"]) != list(self.host.seeds) or tracks["cap"] != self.cap:
            raise ValueError("tracks were recorded with another scenario assignment or mover capacity")
        self._tracks = dict(shape=tracks["shape"].to(self.device).contiguous(), dyn=tracks["dyn"].to(self.device).contiguous())
        self.s.track_shape = self._tracks["shape"].data_ptr()
        self.s.track_dyn = self._tracks["dyn"].data_ptr()
        self.k.track_len = int(self._tracks["shape"].shape[0])

    def _lidar_noise(self):
        """LidarStateObservation._add_noise_to_cloud_points (obs/state_obs.py:234-244) and the same call on the side /
        lane-line detector clouds (state_obs.py:82-85,134-137): gaussian noise (clipped to [0,1]) then dropout to 0,
        each cloud with its own detector's `gaussian_noise` / `dropout_prob`.  The reference draws from the global,
        unseeded numpy stream, so no stream can be 'the' stream; this one is a device generator seeded with
        start_seed + env_seed_offset (reproducible, shard-dependent)."""
        vc = self.cfg["vehicle_config"]
        L = self.host.layout
        clouds = [(vc["lidar"], L.lidar_off, L.n_beams), (vc["side_detector"], L.side_off, L.n_side),
                  (vc["lane_line_detector"], L.ll_off, L.n_ll)]
        torch = self.torch
        for dc, off, n in clouds:
            g, p = float(dc["gaussian_noise"]), float(dc["dropout_prob"])
            if (g <= 0.0 and p <= 0.0) or n <= 0:
                continue
            if self._noise_gen is None:
                self._noise_gen = self._seeded_generator()
            cloud = self.obs[..., off:off + n]
            if g > 0.0:
                noise = torch.empty_like(cloud).normal_(0.0, g, generator=self._noise_gen)
                cloud.copy_((cloud + noise).clamp_(0.0, 1.0))
            if p > 0.0:
                assert p <= 1.0
                drop = torch.empty_like(cloud).uniform_(0.0, 1.0, generator=self._noise_gen) < p
                cloud.masked_fill_(drop, 0.0)

    def line_detector(self, beams, n, dist, mask, out, stride, offset):
        self._launch("md_line_detector", _ptr(beams), n, C.c_float(dist), C.c_uint32(mask), _ptr(out), stride, offset)

    # -- the PPO expert (metadrive_ped_amd/expert.py, md_expert) -----------------------------------------------------------
    def _track_detected(self):
        """expert() on an engine that does not keep the lidar's detected sets (agent_policy other than ExpertPolicy): from
        now on md_step keeps them (its general variant: same results), and md_lidar_detect fills them for the current state."""
        if "detected" in self.state_dev:
            return
        self._track_det = True
        h = self.host
        h.state["detected"] = np.zeros((h.E * h.A, 2), np.uint64)
        self.state_dev["detected"] = self._to_dev(h.state["detected"])
        self.s.detected = self.state_dev["detected"].data_ptr()
        scratch = self.torch.empty((self.E * self.A, self.n_beams), dtype=self.torch.float32, device=self.device)
        with self._on_device():
            self._launch("md_lidar_detect", _ptr(scratch), self.n_beams, 0, _ptr(self.state_dev["detected"]))

    def expert_weights(self):
        """The packed expert weights on the device (uploaded once per engine)."""
        if self._expert_w is None:
            from metadrive_ped_amd.expert import load_expert_weights
            self._expert_w = self.torch.from_numpy(load_expert_weights(self.cfg.get("expert_weights"))).to(self.device)
        return self._expert_w

    def expert_beams(self):
        """The expert's 240-beam table on the device (md_expert_sense's beam_cs240): the env's own MdWorld.beam_cs when that is
        the 240-beam one, else uploaded once per engine."""
        if self.n_beams == 240:
            return self.world_dev["beam_cs"]
        if self._expert_beams is None:
            self._expert_beams = self._to_dev(beam_table(240))
        return self._expert_beams

    def _seeded_generator(self):
        """A device generator seeded with start_seed + env_seed_offset (reproducible, shard-dependent): the lidar noise and the
        expert's draws each have one of their own."""
        g = self.torch.Generator(device=self.device)
        g.manual_seed(int(self.cfg["start_seed"]) + int(self.cfg["env_seed_offset"]))
        return g

    def _expert_noise(self, rows):
        """One [rows, 2] N(0, 1) draw of the engine's expert generator"""
        if self._expert_gen is None:
            self._expert_gen = self._seeded_generator()
        return self.torch.randn((rows, 2), dtype=self.torch.float32, device=self.device, generator=self._expert_gen)

    def _check_f32(self, name, t, rows, cols):
        """A caller's tensor that a kernel reads or writes as rows x cols floats (leading dims may be split: [E, A, cols])"""
        if (t.numel() != rows * cols or t.shape[-1] != cols or t.dtype != self.torch.float32 or t.device != self.device
                or not t.is_contiguous()):
            raise ValueError("{} must be a contiguous float32 [{}, {}] tensor on the engine's device".format(name, rows, cols))

    def expert_forward(self, deterministic=False, need_obs=False, action_out=None, mlp_out=None, noise=None, own_sensors=None):
        """ONE md_expert launch on the current observation -> action [E, 2] (+ the corrected expert obs [E, 275] with
        need_obs).  deterministic=False: action = mean + exp(log_std) * N(0, 1), one [E, 2] draw of the engine's expert
        generator (seeded with start_seed + env_seed_offset), or `noise` [E, 2] float32 on the device when given.
        own_sensors (None: config["expert_own_sensors"]): ONE md_expert_sense launch on the live state instead -- [E * A, 2]
        (+ [E * A, 275]), row e * A + a = agent a of env e, one [E * A, 2] draw; rows of an env about to restore itself are zeros."""
        torch = self.torch
        own = bool(self.cfg.get("expert_own_sensors")) if own_sensors is None else bool(own_sensors)
        if own:      # md_expert_sense reads the live state through the expert's own beam table
            rows, name, extra = self.E * self.A, "md_expert_sense", (_ptr(self.expert_beams()), )
        else:        # md_expert reads the env's observation row and the lidar's detected sets
            if self.A != 1:
                raise ValueError("the expert drives single-agent envs")
            self._track_detected()
            rows, name, extra = self.E, "md_expert", ()
        if deterministic:
            noise = None
        for what, t, cols in (("noise", noise, 2), ("action_out", action_out, 2), ("mlp_out", mlp_out, 4)):
            if t is not None:
                self._check_f32(what, t, rows, cols)
        if noise is None and not deterministic:
            noise = self._expert_noise(rows)
        if action_out is None:
            action_out = torch.empty((rows, 2), dtype=torch.float32, device=self.device)
        obs = torch.empty((rows, 275), dtype=torch.float32, device=self.device) if need_obs else None
        with self._on_device():
            self._launch(name, _ptr(self.expert_weights()), *extra, _ptr(noise), _ptr(action_out), _ptr(mlp_out), _ptr(obs))
        return (action_out, obs) if need_obs else action_out

    def ai_protect_forward(self, actions, noise=None, saver_out=None):
        """agent_policy = AIProtectPolicy (include/md_ai_protect.h): ONE md_ai_protect launch on the current observation -- the expert's
        draw (the weights, the generator and the one [E, 2] draw per step of expert_forward) and the saver's rule on the agents'
        decoded `actions` [E, 2].  -> the applied action [E, 2] (an engine buffer, rewritten by the next call); the flag bytes are left
        in self.protect_flags, the vehicles' takeover / expert_takeover bytes updated in place.  `noise`: the draw to use instead."""
        torch = self.torch
        if "takeover" not in self.state_dev:
            raise ValueError("ai_protect_forward needs agent_policy='AIProtectPolicy'")
        if noise is None:
            noise = self._expert_noise(self.E)
        a = actions
        if tuple(a.shape) != (self.E, 2):
            raise ValueError("actions must have shape [{}, 2], got {}".format(self.E, tuple(a.shape)))
        if a.dtype != torch.float32 or a.device != self.device or not a.is_contiguous():
            a = a.to(self.device, torch.float32).contiguous()
        self._check_f32("noise", noise, self.E, 2)
        self._protect_buffers()
        with self._on_device():
            self._launch("md_ai_protect", _ptr(self.expert_weights()), _ptr(noise), _ptr(a), C.c_float(float(self.cfg["save_level"])),
                         _ptr(self.state_dev["takeover"]), _ptr(self.state_dev["expert_takeover"]), _ptr(self._protect_action),
                         _ptr(self.protect_flags), _ptr(saver_out))
        return self._protect_action

    def _protect_buffers(self):
        """ai_protect_forward's applied action and flag bytes, made on first use"""
        if self._protect_action is None:
            self._protect_action = self.torch.empty((self.E, 2), dtype=self.torch.float32, device=self.device)
            self.protect_flags = self.torch.zeros(self.E, dtype=self.torch.uint8, device=self.device)

    def step(self, actions, noise=None):
        """actions: tensor [E, A, 2] (or [E, 2] when A == 1), float32, on the engine's device.  With agent_policy =
        IDMPolicy the agents drive themselves: `actions` is ignored (None is fine), as the reference's IDMPolicy ignores
        what env.step() is given.  With agent_policy = ExpertPolicy likewise: the expert acts on the state the previous
        step left (ExpertPolicy.act in before_step), then the world steps with that action.  With agent_policy = LaneChangePolicy
        `actions` are the decoded discrete actions (steering -1 / 0 / +1 = right / keep / left): md_step turns the steering into the
        lane-change PIDs' output before it integrates the agents (include/md_lane_change.h).  An env that auto-resets in
        this step discards it (md_step restores the env instead of moving it); its next action comes from the reset state.
        With agent_policy = AIProtectPolicy `actions` are the agents' own (decoded) actions and ai_protect_forward decides what the world
        is stepped with; `noise` [E, 2]: the expert's draw of this step instead of the generator's (that policy only)."""
        if self.k.agent_idm == abi.AGENT_IDM:
            self.s.agent_action = None
            self.step_raw()
            return
        if self.cfg["agent_policy"] == "ExpertPolicy":
            rows = self.E * self.A if self.cfg.get("expert_own_sensors") else self.E
            if self._expert_action is None:
                self._expert_action = self.torch.empty((rows, 2), dtype=self.torch.float32, device=self.device)
            actions = self.expert_forward(deterministic=False, action_out=self._expert_action).view(self.E, -1, 2)
        if self.cfg["agent_policy"] == "AIProtectPolicy":     # the saver looks at the agents' actions on the state the previous step left
            actions = self.ai_protect_forward(actions.reshape(self.E, 2) if actions.dim() == 3 else actions, noise=noise)
        a = actions
        if a.dim() == 2:
            a = a.unsqueeze(1)
        if tuple(a.shape) != (self.E, self.A, 2):
            raise ValueError("actions must have shape [{}, {}, 2], got {}".format(self.E, self.A, tuple(a.shape)))
        if a.dtype != self.torch.float32 or a.device != self.device or not a.is_contiguous():
            a = a.to(self.device, self.torch.float32).contiguous()
        # zero-copy: the kernel reads the agents' actions from the caller's tensor (MdState.agent_action) and
        # writes the sanitised values into the per-slot `action` array itself.  The struct is passed by value at
        # launch, so the pointer is cleared again right away; the tensor is kept alive until the next step.
        self._held_actions = a
        self.s.agent_action = a.data_ptr()
        try:
            self.step_raw()
        finally:
            self.s.agent_action = None

    def call(self, name):
        """Single-phase entry points (parity tests): md_integrate, md_localize, ..."""
        with self._on_device():
            self._launch(name)

    def lidar(self, out, stride, offset):
        with self._on_device():
            self._lidar(out, stride, offset)

    def _lidar(self, out, stride, offset):
        self._launch("md_lidar", _ptr(out), stride, offset)

    # -- user-spawned traffic participants (engine.spawn_object(Pedestrian, ...) + set_velocity of the reference,
    #    tests/test_functionality/test_pedestrian.py:38-55); see participants.py ---------------------------------
    def _edit_participants(self, fn):
        names = ("shape", "shape0", "dyn", "flags")
        st = {k: self.state_dev[k].cpu().numpy().view(self.host.state[k].dtype).reshape(self.host.state[k].shape).copy()
              for k in names}
        out = fn(st)
        self.upload_state({k: st[k] for k in ("shape", "dyn", "flags")})
        return out

    def spawn_object(self, kind, position, heading_theta=0.0, envs=None):
        """-> slot handle.  The participant lives until its env resets (auto-reset included)."""
        from metadrive_ped_amd import participants as P
        return self._edit_participants(lambda st: P.spawn(st, self.E, self.cap, self.A, kind, position, heading_theta, envs))

    def set_velocity(self, slot, direction, value=None, in_local_frame=False, envs=None):
        from metadrive_ped_amd import participants as P
        self._edit_participants(lambda st: P.set_velocity(st, self.E, self.cap, slot, direction, value, in_local_frame, envs))

    def clear_objects(self, slots, envs=None):
        from metadrive_ped_amd import participants as P
        self._edit_participants(lambda st: [P.clear(st, self.E, self.cap, s, envs) for s in slots])

    def object_positions(self, slot):
        """[E, 2] tensor view of the slot's centre in every env."""
        return self.shape_f[:, slot, 0:2]

    def pedestrian_state(self):
        """The policy-driven pedestrians of every env, as device tensors: positions [E, P, 2] float32, phase [E, P] and slot
        [E, P] int32 (abi.PED_*; ascending slot order), P = config num_pedestrians; an env that holds fewer (a map without
        enough straight roads; clear_objects) is padded with -1.  Read from the live state: no host sync."""
        torch = self.torch
        P_ = int(self.cfg.get("num_pedestrians") or 0)
        flags = self.state_dev["shape"].view(torch.int32).view(self.E, self.cap, 8)[:, :, 6]
        phase = self.nav_i[:, :, 13]
        driven = ((flags & abi.KIND_MASK) == abi.KIND_PEDESTRIAN) & ((flags & abi.F_ALIVE) != 0) & ((flags & abi.F_STATIC) == 0) & (phase != 0)
        slots = torch.arange(self.cap, device=self.device, dtype=torch.int64).expand(self.E, self.cap)
        first = torch.where(driven, slots, torch.full_like(slots, self.cap)).sort(dim=1).values[:, :P_]
        if first.shape[1] < P_:          # more pedestrians asked for than slots
            first = torch.nn.functional.pad(first, (0, P_ - first.shape[1]), value=self.cap)
        have = first < self.cap
        at = first.clamp(max=self.cap - 1)
        pos = torch.gather(self.shape_f[:, :, 0:2], 1, at.unsqueeze(-1).expand(-1, -1, 2))
        pos = torch.where(have.unsqueeze(-1), pos, torch.full_like(pos, -1.0))
        ph = torch.where(have, torch.gather(phase, 1, at), torch.full_like(at, -1, dtype=torch.int32))
        return pos, ph, torch.where(have, at, torch.full_like(at, -1)).to(torch.int32)

    def download_state(self):
        """Device state -> dict of numpy arrays with the host dtypes (tests / checkpoints)."""
        out = {}
        for k, v in self.host.state.items():
            out[k] = self.state_dev[k].cpu().numpy().view(v.dtype).reshape(v.shape).copy()
        return out

    # -- device-side env snapshots (include/md_branch.h, metadrive_ped_amd/branch.py) ----------------------------------------
    def branch_fields(self):
        """{MdState field: bytes per env} of the per-env arrays this batch has, in the header table's order; each is checked against
        the array's real size, so a table that drifted from the state builder fails here and not in the kernel."""
        from metadrive_ped_amd import branch
        rows = branch.field_rows(self.cap, self.A, self.obs_dim, int(self.k.route_seg_cap), int(self.k.route_vert_cap))
        out = OrderedDict()
        for name, rb in rows.items():
            t = self.state_dev.get(name)
            if t is None or not getattr(self.s, name):
                continue
            if t.numel() != self.E * rb:
                raise RuntimeError("md_branch: MdState.{} holds {} bytes, the table of per-env extents says {} x {}".format(
                    name, t.numel(), self.E, rb))
            out[name] = rb
        return out

    def branch_extras(self):
        """[(name, tensor, bytes per env)]: the per-env arrays the engine owns outside MdState -- MdWorld.env_map, the top-down
        history and image, the AIProtect bytes, the staged-draw index of random_traffic, the vector observation's history and rows"""
        ex = [("env_map", self.world_dev["env_map"])]
        if self.topdown_dev is not None:
            ex += [(k, self.topdown_dev[k]) for k in ("ring_traffic", "ring_pos", "cursor")] + [("topdown", self.topdown)]
        if "takeover" in self.state_dev:
            self._protect_buffers()
            ex += [("takeover", self.state_dev["takeover"]), ("expert_takeover", self.state_dev["expert_takeover"]),
                   ("protect_flags", self.protect_flags)]
        if self._staged is not None and not self._walk:
            ex.append(("draw_idx", self.draw_idx))
        if self.vector_obs_rows is not None:
            ex += [("vector_obs_hist", self.vector_obs_hist), ("vector_obs", self.vector_obs_rows)]
        out = []
        for name, t in ex:
            nbytes = t.numel() * t.element_size()
            assert t.is_contiguous() and nbytes % self.E == 0, name
            out.append((name, t, nbytes // self.E))
        return out

    def _branch_indices(self, src, dst):
        """The pair lists on the device, [2, n] int32 (a pinned host copy and an asynchronous upload: no sync); the latest few
        lists are kept, so a rollout loop that branches the same envs again uploads nothing."""
        torch = self.torch
        host = np.stack([src, dst]).astype(np.int32)
        key = host.tobytes()
        t = self._branch_idx.get(key)
        if t is None:
            t = torch.from_numpy(host).pin_memory().to(self.device, non_blocking=True)
            self._branch_idx[key] = t
            while len(self._branch_idx) > 8:
                self._branch_idx.popitem(last=False)
        else:
            self._branch_idx.move_to_end(key)
        return t

    def branch_rows(self, dst_state, src_state, src, dst, src_n, dst_n, extras):
        """ONE md_branch launch on torch's current stream: row src[i] of every per-env array of `src_state` (an abi.MdState: this
        engine's self.s or a snapshot's) -> row dst[i] of `dst_state`; extras = [(dst address, src address, bytes per env)].
        src / dst: host integer arrays, already checked by the caller (ranges, no destination twice, no overlap); the kernel
        itself only guards the rows against the two row counts."""
        from metadrive_ped_amd import branch
        src, dst = np.asarray(src, dtype=np.int64).reshape(-1), np.asarray(dst, dtype=np.int64).reshape(-1)
        if src.size != dst.size or src.size == 0:
            raise ValueError("md_branch: {} source rows for {} destination rows".format(src.size, dst.size))
        idx = self._branch_indices(src, dst)
        n = len(src)
        b = branch.fill_branch(idx.data_ptr(), idx.data_ptr() + 4 * n, n, src_n, dst_n, extras)
        with self._on_device():
            self._check(self.lib.md_branch(C.byref(dst_state), C.byref(src_state), C.byref(self.k), C.byref(b), self._stream()), "md_branch")

    def upload_state(self, arrays):
        for k, v in arrays.items():
            self.state_dev[k].copy_(self.torch.from_numpy(np.ascontiguousarray(v).view(np.uint8).reshape(-1)))
