"""Configuration of the batched envs: the reference's config keys for this path, same defaults.

Mirrors the layering BASE_DEFAULT_CONFIG -> METADRIVE_DEFAULT_CONFIG -> user dict
(metadrive/envs/base_env.py:32-266, envs/metadrive_env.py:16-99) and the Config class's contract
(utils/config.py:23-38,125): an unknown key raises KeyError, a value whose type differs from the
default's raises TypeError.  Keys of the reference that belong to subsystems outside the hot path
(rendering, cameras, recording ...) are accepted only at their default "off" value and rejected
loudly otherwise, so a reference config either behaves the same or fails -- never silently differs.
Batched-engine extras are grouped at the end.
"""
import copy

from metadrive_ped_amd.mapgen.pg import BlockDist

DEFAULT_AGENT = "default_agent"

BASE_DEFAULT_CONFIG = dict(
    # ===== agent =====
    random_agent_model=False,
    num_agents=1,
    is_multi_agent=False,
    allow_respawn=False,
    delay_done=0,
    # ===== action =====
    agent_policy="EnvInputPolicy",   # or "IDMPolicy" / "ExpertPolicy" / "LaneChangePolicy" / "AIProtectPolicy" (the class of that name is accepted too): envs/base_env.py:53
    discrete_action=False,
    use_multi_discrete=False,
    discrete_steering_dim=5,
    discrete_throttle_dim=5,
    action_check=False,
    # ===== termination =====
    horizon=None,
    truncate_as_terminate=False,
    marl_map=None,          # None | "pg" | "roundabout" | "intersection" | "bottleneck" | "bidirection" | "tollgate" | "parking_lot" | "racing" (set by the multi-agent env classes)
    # ===== vehicle =====
    vehicle_config=dict(
        vehicle_model="default",
        enable_reverse=False,
        spawn_lane_index=None,
        destination=None,
        spawn_longitude=5.0,
        spawn_lateral=0.0,
        width=None, length=None, height=None, mass=None,   # read by vehicle_model="varying_dynamics" only (vehicle_type.py:168-187)
        spawn_velocity=None,             # [vx, vy] m/s at reset (base_vehicle.py:371-372); its component along the heading is kept
        spawn_velocity_car_frame=False,  # True: [forward, left] of the vehicle instead of world axes
        lidar=dict(num_lasers=240, distance=50, num_others=0, gaussian_noise=0.0, dropout_prob=0.0,
                   add_others_navi=False),
        side_detector=dict(num_lasers=0, distance=50, gaussian_noise=0.0, dropout_prob=0.0),
        lane_line_detector=dict(num_lasers=0, distance=20, gaussian_noise=0.0, dropout_prob=0.0),
        min_pass_steps=30,               # MultiAgentTollgateEnv: steps an agent has to spend inside the toll block (marl_tollgate.py:28)
    ),
    # ===== engine =====
    use_render=False,
    image_observation=False,
    physics_world_step_size=2e-2,
    decision_repeat=5,
    map_region_size=1024,
    log_level=20,
)

METADRIVE_DEFAULT_CONFIG = dict(
    start_seed=0,
    num_scenarios=1,
    map=3,
    block_dist_config=None,  # None -> BLOCK_TYPE_DISTRIBUTION_V2
    random_lane_width=False,
    random_lane_num=False,
    map_config=dict(type="block_num", config=None, lane_width=3.5, lane_num=3, exit_length=50,
                    neck_lane_num=1, neck_length=20,    # multi-agent bottleneck map only (marl_bottleneck.py:13)
                    toll_lane_num=8, toll_length=10,    # multi-agent tollgate map only (marl_tollgate.py:19)
                    radius=None),                       # multi-agent intersection maps only (tinyinter.py:349-351)
    store_map=True,
    traffic_density=0.1,
    need_inverse_traffic=False,
    traffic_mode="trigger",
    random_traffic=False,
    accident_prob=0.0,
    static_traffic_object=True,
    random_spawn_lane_index=True,
    agent_configs={DEFAULT_AGENT: dict(spawn_lane_index=(">", ">>", 0))},
    success_reward=10.0,
    out_of_road_penalty=5.0,
    crash_vehicle_penalty=5.0,
    crash_object_penalty=5.0,
    driving_reward=1.0,
    speed_reward=0.1,
    use_lateral_reward=False,
    crash_vehicle_cost=1.0,
    crash_object_cost=1.0,
    out_of_road_cost=1.0,
    out_of_route_done=False,
    on_continuous_line_done=True,
    crash_vehicle_done=True,
    crash_object_done=True,
    crash_human_done=True,
    enable_idm_lane_change=True,
    # multi-agent keys (envs/marl_envs/multi_agent_metadrive.py:12-61); inert for single-agent envs
    crash_done=True,
    out_of_road_done=True,
    force_seed_spawn_manager=False,
    spawn_roads=None,
    cross_yellow_line_done=True,   # bottleneck / bidirection / tollgate envs (marl_bottleneck.py:17,129-135, marl_tollgate.py:22,241-247)
    overspeed_penalty=0.5,         # tollgate env (marl_tollgate.py:25)
    parking_space_num=8,           # parking-lot env (marl_parking_lot.py:31): an even number >= 4
    # racing env (RACING_CONFIG, marl_racing_env.py:46-63)
    crash_sidewalk_penalty=1.0, idle_penalty=1.0, idle_done=True, crash_sidewalk_done=False,
    # VaryingDynamicsEnv (envs/varying_dynamics_env.py:14-25): None = off, else {parameter: (min, max) | None}
    random_dynamics=None,
)

# batched-engine keys (no counterpart in the reference: it steps one world per process)
BATCH_DEFAULT_CONFIG = dict(
    num_envs=1,             # E: environments stepped in lockstep by this process (this GPU's shard)
    env_seed_offset=0,      # global index of this shard's first env (seed = start_seed + (offset + e) % num_scenarios)
    mover_capacity=0,       # slots per env (agents + traffic + props); 0 = smallest multiple of 8 that fits every env
    auto_reset=True,        # restore an env from its reset snapshot on the step after it finished
    device="cuda:0",
    build_workers=0,        # 1 = generate maps in this process; otherwise the persistent workers of hostpool.py do it
    build_cache=False,      # memoise built (map, scene) pairs by scenario seed + config (sub-batches / copies of the same envs)
    traffic_epoch=0,        # random_traffic=True: bumped by every explicit env.reset(); part of the traffic stream's seed
    traffic_draws=4,        # random_traffic=True with auto_reset: traffic draws staged on the device; an env takes the next one
                            # at every reset (an episode meets its n-th predecessor's traffic again); 1 = one draw per env.reset()
    initial_agents=0,       # set by num_agents=-1 (multi-agent): agents present at reset; the other slots start free
    step_kernel="auto",     # single-agent md_step: "wg" = one 4-wave workgroup per env, "wave" = one wave per env, "auto" = by
                            # the number of distinct maps the batch shares (engine.WAVE_KERNEL_MAX_MAPS) (same
                            # results bit for bit; a machine-mapping choice)
    # the PG walk (no key of the reference's: it draws a new scenario seed at every reset by itself, envs/base_env.py:886-891):
    # True = an env moves on to another seed of [start_seed, start_seed + num_scenarios) whenever its episode ends, on the device
    walk_scenarios=False,
    walk_stride=None,       # W, the envs over all shards / sub-batches (sharding.shard_config and SubBatchedEnvs set it); None: num_envs
    sequential_seed=False,  # walk order: False = a uniform draw over the slice per (global env index, episode), the reference's PG
                            # rule from a reproducible stream; True = worker w = (env_seed_offset + e) % num_scenarios plays w, w + W, ...
    scenario_pool_max_bytes=64 << 30,   # a walk's scene pool (maps + snapshot rows, device bytes) larger than this is refused
    expert_weights=None,    # agent_policy="ExpertPolicy" / expert.expert(): path of the reference's ppo_expert/expert_weights.npz;
                            # None = found in an installed reference package (metadrive_ped_amd/expert.py)
    expert_own_sensors=False,   # True: the expert observes through its own sensors (240 lasers at 50 m, num_others=4, no noise, no
                            # detectors: numpy_expert.py:39-62) from the live state (md_expert_sense), so agent_policy="ExpertPolicy"
                            # and expert() take any vehicle_config and the multi-agent envs (all but tollgate); False: from the
                            # env's own obs row (md_expert), which only the 259-dim default vehicle config allows
    # crossing pedestrians driven on the device (include/md_ped.h; no key of the reference's, the numbers are a design choice):
    # placed per scenario seed at scene build, restored by the env's own reset, one md_ped launch before every md_step
    num_pedestrians=0,      # per env; a map with fewer straight roads than that holds fewer (env.pedestrian_state() reports them)
    pedestrian_config=dict(
        speed=1.2,              # m/s (Pedestrian.SPEED_LIST[1])
        wait_min_steps=10,      # a wait at the kerb lasts this + a draw of randint(0, 25) steps
        clear_dist=1.0,         # m: a vehicle this close to the crossing line (beyond its half length) occupies it
        margin=1.0,             # m: the strip a waiting pedestrian watches reaches this far beyond both kerbs
        time_margin=1.0,        # s: a gap is taken if no vehicle arrives within the crossing time + this
        yield_ahead=3.0,        # m: a crossing pedestrian looks this far ahead along its walk ...
        yield_time=1.5,         # s: ... and stops for a vehicle that arrives there within this
        kerb_offset=1.0,        # m: the end points lie this far outside the outermost lanes' edges
        min_road_length=20.0,   # m: shorter roads hold no crossing
        spawn_clearance=15.0),  # m: no crossing closer than this to the agent's spawn position
    # contact response (include/md_contact_response.h; no key of the reference's, the numbers are a design choice): True = a driving
    # vehicle that overlaps another body is pushed out of it and loses the speed that closes on it, one md_contact_response launch
    # before every md_step (and before md_ped); False = no launch: vehicles pass through what they hit, as before
    contact_response=False,
    contact_response_config=dict(
        skin=0.01,              # m: the gap a resolved pair is left with
        max_push=0.5),          # m: the longest displacement of a vehicle in one step
    # the vector scene observation (include/md_vector_obs.h; no key of the reference's, the numbers are a design choice): None = off,
    # no launch and no array; a dict (an empty one too) is laid over VECTOR_OBS_DEFAULT_CONFIG and env.vector_obs() returns the blocks
    vector_obs=None,
)

VECTOR_OBS_DEFAULT_CONFIG = dict(
    num_agents=8,           # K nearest movers, 1 .. 16
    history=5,              # T frames of pose history, the current one included, 1 .. 8
    radius=50.0,            # m: movers farther from the observer than this are no neighbours
    max_jump=8.0,           # m: a displacement between two frames beyond this ends a slot's history (a respawn in the slot)
    route_points=16,        # M waypoints along the route ahead, 0 .. 32
    route_spacing=4.0,      # m between them
    num_lanes=8,            # P nearest lane centre-lines, 0 .. 16
    lane_points=8,          # S points per lane, 2 .. 16
)
# key -> (lowest, highest): MD_VO_MAX_* of include/md_vector_obs.h
VECTOR_OBS_RANGES = dict(num_agents=(1, 16), history=(1, 8), route_points=(0, 32), num_lanes=(0, 16), lane_points=(2, 16))


def check_vector_obs(user):
    """config["vector_obs"] (a dict) laid over its defaults -> the finished dict; a ValueError names the key at fault"""
    if not isinstance(user, dict):
        raise ValueError("vector_obs={!r}: None (off) or a dict of {}".format(user, sorted(VECTOR_OBS_DEFAULT_CONFIG)))
    unknown = sorted(set(user) - set(VECTOR_OBS_DEFAULT_CONFIG))
    if unknown:
        raise ValueError("vector_obs: unknown key(s) {} (known: {})".format(unknown, sorted(VECTOR_OBS_DEFAULT_CONFIG)))
    vo = dict(VECTOR_OBS_DEFAULT_CONFIG, **user)
    for k, (lo, hi) in VECTOR_OBS_RANGES.items():
        if isinstance(vo[k], bool) or not isinstance(vo[k], int) or not lo <= vo[k] <= hi:
            raise ValueError("vector_obs['{}']={!r}: an int in [{}, {}]".format(k, vo[k], lo, hi))
    for k in ("radius", "max_jump", "route_spacing"):
        if isinstance(vo[k], bool) or not isinstance(vo[k], (int, float)) or not 0 < vo[k] <= 1e18:
            raise ValueError("vector_obs['{}']={!r}: a positive number of metres".format(k, vo[k]))
        vo[k] = float(vo[k])
    return vo


# BatchedScenarioEnv's vector scene observation (config scenario_vector_obs; include/md_scenario_vector_obs.h).  Like the numbers
# above, every default here is a design choice, not a value of the reference's.
SCENARIO_VECTOR_OBS_DEFAULT_CONFIG = dict(
    num_agents=8,           # K nearest movers, 1 .. 16
    history=5,              # T frames of pose history, the current one included, 1 .. 8
    radius=50.0,            # m: movers farther from the observer than this are no neighbours
    max_jump=8.0,           # m: a displacement between two frames beyond this ends a slot's history
    route_points=16,        # M waypoints along the recorded trajectory ahead, 0 .. 32
    route_spacing=4.0,      # m between them
    num_pieces=32,          # P nearest map polyline pieces, 0 .. 64
    piece_points=8,         # S points per piece, 2 .. 16
    map_radius=50.0,        # m: pieces without a point this close to the observer are not taken
    map_spacing=2.0,        # m between the samples of a map polyline (the host resamples every feature once per scene)
)
# key -> (lowest, highest): MD_VO_MAX_* of include/md_vector_obs.h, MD_SVO_MAX_* of include/md_scenario_vector_obs.h
SCENARIO_VECTOR_OBS_RANGES = dict(num_agents=(1, 16), history=(1, 8), route_points=(0, 32), num_pieces=(0, 64), piece_points=(2, 16))
SCENARIO_VECTOR_OBS_LENGTHS = ("radius", "max_jump", "route_spacing", "map_radius", "map_spacing")


def check_scenario_vector_obs(user):
    """config["scenario_vector_obs"] (a dict) laid over its defaults -> the finished dict; a ValueError names the key at fault"""
    known = sorted(SCENARIO_VECTOR_OBS_DEFAULT_CONFIG)
    if not isinstance(user, dict):
        raise ValueError("scenario_vector_obs={!r}: None (off) or a dict of {}".format(user, known))
    unknown = sorted(set(user) - set(SCENARIO_VECTOR_OBS_DEFAULT_CONFIG))
    if unknown:
        raise ValueError("scenario_vector_obs: unknown key(s) {} (known: {})".format(unknown, known))
    vo = dict(SCENARIO_VECTOR_OBS_DEFAULT_CONFIG, **user)
    for k, (lo, hi) in SCENARIO_VECTOR_OBS_RANGES.items():
        if isinstance(vo[k], bool) or not isinstance(vo[k], int) or not lo <= vo[k] <= hi:
            raise ValueError("scenario_vector_obs['{}']={!r}: an int in [{}, {}]".format(k, vo[k], lo, hi))
    for k in SCENARIO_VECTOR_OBS_LENGTHS:
        if isinstance(vo[k], bool) or not isinstance(vo[k], (int, float)) or not 0 < vo[k] <= 1e18:
            raise ValueError("scenario_vector_obs['{}']={!r}: a positive number of metres".format(k, vo[k]))
        vo[k] = float(vo[k])
    return vo


# BatchedScenarioEnv's traffic lights (config traffic_lights; include/md_traffic_lights.h).  The walls, their statuses and the flags
# are the reference's; the two numbers of the nearest-lights block are design choices, not values of the reference's.
TRAFFIC_LIGHTS_DEFAULT_CONFIG = dict(
    num_lights=8,           # L nearest lights in the observation block, 0 .. 32 (MD_TL_MAX_LIGHTS)
    radius=80.0,            # m: lights whose stop point is farther from the observer than this are not taken
)
TRAFFIC_LIGHTS_RANGES = dict(num_lights=(0, 32))


def check_traffic_lights(user):
    """config["traffic_lights"] (a dict) laid over its defaults -> the finished dict; a ValueError names the key at fault"""
    known = sorted(TRAFFIC_LIGHTS_DEFAULT_CONFIG)
    if not isinstance(user, dict):
        raise ValueError("traffic_lights={!r}: None (off) or a dict of {}".format(user, known))
    unknown = sorted(set(user) - set(TRAFFIC_LIGHTS_DEFAULT_CONFIG))
    if unknown:
        raise ValueError("traffic_lights: unknown key(s) {} (known: {})".format(unknown, known))
    tl = dict(TRAFFIC_LIGHTS_DEFAULT_CONFIG, **user)
    for k, (lo, hi) in TRAFFIC_LIGHTS_RANGES.items():
        if isinstance(tl[k], bool) or not isinstance(tl[k], int) or not lo <= tl[k] <= hi:
            raise ValueError("traffic_lights['{}']={!r}: an int in [{}, {}]".format(k, tl[k], lo, hi))
    if isinstance(tl["radius"], bool) or not isinstance(tl["radius"], (int, float)) or not 0 < tl["radius"] <= 1e18:
        raise ValueError("traffic_lights['radius']={!r}: a positive number of metres".format(tl["radius"]))
    tl["radius"] = float(tl["radius"])
    return tl


# BatchedScenarioEnv's closed-loop driving metrics (config scenario_metrics; include/md_scenario_metrics.h).  The reference has no
# counterpart: every number here is a design choice -- the sweep's sampling, and comfort bounds as planning benchmarks commonly set them.
SCENARIO_METRICS_DEFAULT_CONFIG = dict(
    ttc_samples=30,         # J: the sweep tests the samples 0 .. J, 0 .. 64 (MD_SM_MAX_TTC_SAMPLES)
    ttc_dt=0.1,             # s between two samples
    ttc_threshold=0.95,     # s: a step with a smaller time to collision counts in ttc_violation_steps
    max_lon_accel=2.40, min_lon_accel=-4.05,      # m/s^2
    max_lat_accel=4.89,     # m/s^2, against |lat_accel|
    max_lon_jerk=4.13,      # m/s^3, against |lon_jerk|
    max_jerk=8.37,          # m/s^3
    max_yaw_rate=0.95,      # rad/s, against |yaw_rate|
    max_yaw_accel=1.93,     # rad/s^2, against |yaw_accel|
)
SCENARIO_METRICS_RANGES = dict(ttc_samples=(0, 64))


def check_scenario_metrics(user):
    """config["scenario_metrics"] (a dict) laid over its defaults -> the finished dict; a ValueError names the key at fault"""
    known = sorted(SCENARIO_METRICS_DEFAULT_CONFIG)
    if not isinstance(user, dict):
        raise ValueError("scenario_metrics={!r}: None (off) or a dict of {}".format(user, known))
    unknown = sorted(set(user) - set(SCENARIO_METRICS_DEFAULT_CONFIG))
    if unknown:
        raise ValueError("scenario_metrics: unknown key(s) {} (known: {})".format(unknown, known))
    sm = dict(SCENARIO_METRICS_DEFAULT_CONFIG, **user)
    for k, (lo, hi) in SCENARIO_METRICS_RANGES.items():
        if isinstance(sm[k], bool) or not isinstance(sm[k], int) or not lo <= sm[k] <= hi:
            raise ValueError("scenario_metrics['{}']={!r}: an int in [{}, {}]".format(k, sm[k], lo, hi))
    for k in sorted(set(sm) - set(SCENARIO_METRICS_RANGES)):
        if isinstance(sm[k], bool) or not isinstance(sm[k], (int, float)) or not -1e18 <= sm[k] <= 1e18:     # a NaN fails both
            raise ValueError("scenario_metrics['{}']={!r}: a finite number".format(k, sm[k]))
        sm[k] = float(sm[k])
    if not 0 < sm["ttc_dt"] <= 1e6:
        raise ValueError("scenario_metrics['ttc_dt']={!r}: a positive number of seconds (at most 1e6)".format(sm["ttc_dt"]))
    for k in ("max_lon_accel", "max_lat_accel", "max_lon_jerk", "max_jerk", "max_yaw_rate", "max_yaw_accel"):
        if sm[k] < 0:
            raise ValueError("scenario_metrics['{}']={!r}: an upper bound, not negative".format(k, sm[k]))
    if sm["min_lon_accel"] > 0:
        raise ValueError("scenario_metrics['min_lon_accel']={!r}: a lower bound, not positive".format(sm["min_lon_accel"]))
    return sm

# The top-down observation envs' own keys (envs/top_down_env.py:12-21,54-61 of the reference): they exist for BatchedTopDownMetaDrive /
# BatchedTopDownMetaDriveEnvV2 only (make_config(top_down=True)); any other class given one raises KeyError, as the reference's would.
# norm_pixel is on the cosmetic list below for every other class; for these two it decides the image's dtype.
TOP_DOWN_DEFAULT_CONFIG = dict(frame_skip=5, frame_stack=3, post_stack=5, norm_pixel=True, resolution_size=84, distance=30)
TOP_DOWN_MAX_RES, TOP_DOWN_MAX_RING = 128, 64      # MD_TD_MAX_RES / MD_TD_MAX_RING (include/md_topdown.h)

# Keys of the reference's BASE_DEFAULT_CONFIG (envs/base_env.py:32-266) that only concern rendering, cameras, the GUI,
# debugging displays or asset handling: nothing on this path reads them, so any value is accepted and kept.
COSMETIC_DEFAULT_CONFIG = dict(
    controller="keyboard", norm_pixel=True, stack_size=3, use_chase_camera_follow_lane=False, camera_height=2.2, camera_dist=7.5,
    camera_pitch=None, camera_smooth=True, camera_smooth_buffer_size=20, camera_fov=65, prefer_track_agent=None,
    top_down_camera_initial_x=0, top_down_camera_initial_y=0, top_down_camera_initial_z=200, window_size=(1200, 900),
    image_on_cuda=False, _render_mode="none", force_render_fps=None, force_destroy=False, num_buffering_objects=200,
    render_pipeline=False, daytime="19:00", shadow_range=50, multi_thread_render=True, multi_thread_render_mode="Cull",
    preload_models=True, disable_model_compression=True, cull_lanes_outside_map=False, drivable_area_extension=7,
    height_scale=50, use_mesh_terrain=False, full_size_mesh=True, show_crosswalk=True, show_sidewalk=True, pstats=False,
    debug=False, debug_panda3d=False, debug_physics_world=False, debug_static_world=False, show_coordinates=False,
    show_fps=True, show_logo=True, show_mouse=True, show_skybox=True, show_terrain=True, show_interface=True,
    show_policy_mark=False, show_interface_navi_mark=True, interface_panel=["dashboard"], force_reuse_object_name=False,
    traffic_vehicle_config=dict(show_navi_mark=False, show_dest_mark=False, enable_reverse=False, show_lidar=False,
                                show_lane_line_detector=False, show_side_detector=False),
)
COSMETIC_VEHICLE_CONFIG = dict(show_navi_mark=True, show_dest_mark=False, show_line_to_dest=False, show_line_to_navi_mark=False,
                               use_special_color=False, image_source="rgb_camera", overtake_stat=False, random_color=False,
                               top_down_width=None, top_down_length=None, show_lidar=False, show_side_detector=False,
                               show_lane_line_detector=False)

# Behavioural keys of subsystems that are not built: accepted at the reference's default, rejected loudly otherwise.
_OFF_ONLY = dict(use_render=False, image_observation=False, manual_control=False, agent_observation=None,
                 sensors=None, record_episode=False, replay_episode=None, only_reset_when_replay=False, use_AI_protector=False,
                 save_level=0.5)
_OFF_ONLY_VEHICLE = dict(no_wheel_friction=False, navigation_module=None, spawn_position_heading=None, light=False)
_OFF_HINT = dict(record_episode="use env.start_recording() / stop_recording() / export_scenarios()",
                 replay_episode="use traffic_mode='replay' with env.load_tracks()",
                 use_AI_protector="the saver is built as agent_policy='AIProtectPolicy' (with config['save_level'])",
                 save_level="any value in [0, 1] is read by agent_policy='AIProtectPolicy' only")
# the policies whose step runs the PPO expert (expert_config_problem applies)
EXPERT_POLICIES = ("ExpertPolicy", "AIProtectPolicy")


def _merge(dst, src, path=""):
    for k, v in src.items():
        if k not in dst:
            raise KeyError("'{}{}' does not exist in existing config. Please use config.update(..., allow_add_new_key="
                           "True) to allow new keys -- unknown config key".format(path, k))
        if isinstance(dst[k], dict) and isinstance(v, dict) and k != "agent_configs":
            _merge(dst[k], v, path + k + ".")
        else:
            old = dst[k]
            cosmetic = k in COSMETIC_DEFAULT_CONFIG or k in COSMETIC_VEHICLE_CONFIG
            if old is not None and v is not None and not isinstance(old, dict) and not cosmetic:
                # utils/config.py:241-250: int <-> float are interchangeable
                ok = isinstance(v, type(old)) or (isinstance(old, float) and isinstance(v, int)) or \
                    (isinstance(old, int) and not isinstance(old, bool) and isinstance(v, float)) or \
                    (k == "map" and isinstance(v, (int, str))) or (k == "horizon") or (k == "agent_policy")
                if not ok:
                    raise TypeError("Attempting to update '{}{}' with type {}, expected {}".format(
                        path, k, type(v).__name__, type(old).__name__))
            dst[k] = v


OWN_SENSORS_HINT = "; expert_own_sensors=True lets the expert observe through its own sensors instead"


def expert_config_problem(cfg, own_sensors=None):
    """None if the PPO expert can drive envs of this config, else why not.  numpy_expert.py:58-62 rewrites the vehicle's
    config to lidar (240 beams, 50 m, num_others=0, no noise, no dropout) and random_agent_model=False on every call, and
    its observation must be 275-dim (:48): reading the env's own obs row, only the configs where that rewrite changes
    nothing are taken.  own_sensors (None: config["expert_own_sensors"]): the expert observes for itself (md_expert_sense),
    whatever the vehicle config, in every env whose vehicles navigate a road network with the plain observation layout."""
    why = "the reference's expert (examples/ppo_expert/numpy_expert.py) rewrites the vehicle config to this on every call"
    own = bool(cfg.get("expert_own_sensors")) if own_sensors is None else bool(own_sensors)
    if cfg.get("scenario_mode"):
        return "agent_policy=ExpertPolicy / expert(): not in BatchedScenarioEnv (single-agent PG envs only)"
    if own:
        if cfg["is_multi_agent"] and cfg["marl_map"] == "tollgate":
            return ("agent_policy=ExpertPolicy / expert(): not in the tollgate env, with expert_own_sensors=True either (its "
                    "observation has no navigation dims)")
        return None
    problem = _obs_row_expert_problem(cfg, why)
    return problem + OWN_SENSORS_HINT if problem else None


def _obs_row_expert_problem(cfg, why):
    if cfg["is_multi_agent"]:
        return "agent_policy=ExpertPolicy / expert(): not in the multi-agent envs (single-agent PG envs only)"
    vc = cfg["vehicle_config"]
    li = vc["lidar"]
    want = dict(num_lasers=240, distance=50, num_others=0, gaussian_noise=0.0, dropout_prob=0.0, add_others_navi=False)
    for k, v in want.items():
        if li[k] != v:
            return "vehicle_config['lidar']['{}']={!r}: the expert needs {!r} ({})".format(k, li[k], v, why)
    for det in ("side_detector", "lane_line_detector"):
        if vc[det]["num_lasers"] > 0 and vc[det]["distance"] > 0:
            return ("vehicle_config['{}'] is on: the expert's observation would not be 275-dim ('Observation not match', "
                    "numpy_expert.py:48)".format(det))
    if cfg["random_agent_model"]:
        return "random_agent_model=True: the expert needs False ({})".format(why)
    return None


def _check_top_down(cfg):
    """The top-down keys' types and the limits of include/md_topdown.h, refused by name"""
    for k in ("frame_skip", "frame_stack", "post_stack", "resolution_size"):
        if isinstance(cfg[k], bool) or not isinstance(cfg[k], int) or cfg[k] < 1:
            raise ValueError("config['{}']={!r}: an int >= 1".format(k, cfg[k]))
    if not isinstance(cfg["norm_pixel"], bool):
        raise TypeError("Attempting to update 'norm_pixel' with type {}, expected bool".format(type(cfg["norm_pixel"]).__name__))
    if isinstance(cfg["distance"], bool) or not cfg["distance"] > 0:
        raise ValueError("config['distance']={!r}: a positive number of metres".format(cfg["distance"]))
    if cfg["resolution_size"] > TOP_DOWN_MAX_RES:
        raise ValueError("config['resolution_size']={} is beyond the top-down kernel's limit {}".format(cfg["resolution_size"], TOP_DOWN_MAX_RES))
    for k in ("frame_stack", "post_stack"):
        if (cfg[k] - 1) * cfg["frame_skip"] + 1 > TOP_DOWN_MAX_RING:
            raise ValueError("({0} - 1) * frame_skip + 1 = {1} is beyond the top-down kernel's ring limit {2}".format(
                k, (cfg[k] - 1) * cfg["frame_skip"] + 1, TOP_DOWN_MAX_RING))
    if cfg["is_multi_agent"] or cfg["num_agents"] != 1:
        raise NotImplementedError("Don't support multi-agent top-down observation yet! (top_down_obs_multi_channel.py:151)")


def make_config(user=None, top_down=False):
    """top_down: the config of a top-down observation env (TOP_DOWN_DEFAULT_CONFIG's keys exist)"""
    cfg = copy.deepcopy(BASE_DEFAULT_CONFIG)
    cfg.update(copy.deepcopy(METADRIVE_DEFAULT_CONFIG))
    cfg.update(copy.deepcopy(BATCH_DEFAULT_CONFIG))
    cfg.update(copy.deepcopy(COSMETIC_DEFAULT_CONFIG))
    if top_down:
        cfg.update(copy.deepcopy(TOP_DOWN_DEFAULT_CONFIG))
    cfg["vehicle_config"].update(copy.deepcopy(COSMETIC_VEHICLE_CONFIG))
    for k, off in _OFF_ONLY.items():
        cfg.setdefault(k, off)
    for k, off in _OFF_ONLY_VEHICLE.items():
        cfg["vehicle_config"].setdefault(k, off)
    user = dict(user or {})
    if isinstance(user.get("sensors"), dict) and not user["sensors"]:
        user["sensors"] = None                                  # an empty sensor table is the default
    _merge(cfg, user)
    if top_down:
        _check_top_down(cfg)
    # agent_policy: the reference takes a policy CLASS; here its name (or a class of that name)
    pol = cfg["agent_policy"]
    pol = pol if isinstance(pol, str) else getattr(pol, "__name__", repr(pol))
    for where, table in ((cfg, _OFF_ONLY), (cfg["vehicle_config"], _OFF_ONLY_VEHICLE)):
        for k, off in table.items():
            if k == "save_level" and pol == "AIProtectPolicy":      # the saver's grade (policy/AI_protect_policy.py:15)
                if isinstance(where[k], bool) or not isinstance(where[k], (int, float)) or not 0.0 <= where[k] <= 1.0:
                    raise ValueError("config['save_level']={!r}: a number in [0, 1]".format(where[k]))
                continue
            if where[k] != off:
                raise NotImplementedError("config['{}']={!r}: this option lies outside the batched step() path built so far "
                                          "(only {!r} is accepted){}".format(k, where[k], off,
                                                                             "; " + _OFF_HINT[k] if k in _OFF_HINT else ""))
    # parse_map_config (component/map/pg_map.py:17-36): `map` shorthand fills map_config
    m = cfg["map"]
    if isinstance(m, int):
        cfg["map_config"]["type"], cfg["map_config"]["config"] = "block_num", m
    elif isinstance(m, str):
        cfg["map_config"]["type"], cfg["map_config"]["config"] = "block_sequence", m
    else:
        raise ValueError("Unknown easy map config: {}".format(m))
    if cfg["block_dist_config"] is None:
        cfg["block_dist_config"] = BlockDist()
    elif isinstance(cfg["block_dist_config"], dict):
        cfg["block_dist_config"] = BlockDist(cfg["block_dist_config"])
    if cfg["is_multi_agent"] and abs(cfg["traffic_density"]) >= 1e-2:
        raise NotImplementedError("traffic_density > 0 in a multi-agent env is not built (the reference's multi-agent "
                                  "envs run without traffic: multi_agent_metadrive.py:58)")
    if cfg["is_multi_agent"] and cfg["random_dynamics"]:
        raise NotImplementedError("random_dynamics: 'Only supporting single-agent now!' (varying_dynamics_env.py:46)")
    if cfg["random_dynamics"]:
        unknown = set(cfg["random_dynamics"]) - {"max_engine_force", "max_brake_force", "wheel_friction", "max_steering", "mass"}
        if unknown:
            raise KeyError("random_dynamics: unknown parameter(s) {}".format(sorted(unknown)))
    if cfg["is_multi_agent"] and abs(cfg["accident_prob"]) >= 1e-2:
        raise NotImplementedError("accident scenes in a multi-agent env are not built")
    if pol not in ("EnvInputPolicy", "IDMPolicy", "ExpertPolicy", "LaneChangePolicy", "AIProtectPolicy"):
        raise NotImplementedError("agent_policy={!r}: built are EnvInputPolicy (actions from step()), IDMPolicy, ExpertPolicy, "
                                  "LaneChangePolicy, AIProtectPolicy and, in BatchedScenarioEnv only, ReplayEgoCarPolicy".format(pol))
    cfg["agent_policy"] = pol
    if pol == "LaneChangePolicy":
        # LaneChangePolicy.__init__ (policy/lange_change_policy.py:16)
        assert cfg["discrete_action"], "Must set discrete_action=True for using this control policy"
    if pol == "AIProtectPolicy" and cfg["expert_own_sensors"]:
        raise NotImplementedError("agent_policy=AIProtectPolicy with expert_own_sensors=True is not built: the saver's rule reads the "
                                  "env's own lidar cloud (use ExpertPolicy / expert(), or the default vehicle config without the key)")
    if pol in EXPERT_POLICIES:
        problem = expert_config_problem(cfg)
        if problem:
            raise ValueError(problem if pol == "ExpertPolicy" else problem.replace("agent_policy=ExpertPolicy", "agent_policy=" + pol))
    if cfg["num_agents"] == -1:
        # "infinite agents" (spawn_manager.py:74-78, agent_manager.py:272-279, multi_agent_metadrive.py:86-92): every spawn
        # point holds an agent at reset and a new agent enters whenever a spawn region is clear, whatever the number on
        # the road.  With fixed slots: capacity = all spawn points, and as many slots again for vehicles still on the
        # road (active or dying) -- a respawn needs a free slot too, which is the one bound the reference does not have.
        if not cfg["is_multi_agent"] or cfg["marl_map"] is None:
            raise ValueError("num_agents=-1 (infinite agents) is a multi-agent env option")
        import math
        from metadrive_ped_amd.marl import PG_SPAWN_ROADS, SPAWN_ROADS
        roads = cfg["spawn_roads"] or (PG_SPAWN_ROADS if cfg["marl_map"] == "pg" else SPAWN_ROADS[cfg["marl_map"]])
        slots = int(math.floor((cfg["map_config"]["exit_length"] - 10) / 8.0))      # max_capacity (spawn_manager.py:108-115)
        if slots <= 0:
            raise ValueError("The exist length {} should greater than minimal longitude interval {}.".format(
                cfg["map_config"]["exit_length"] - 10, 18))
        cfg["initial_agents"] = cfg["map_config"]["lane_num"] * len(roads) * slots
        cfg["num_agents"] = min(128, 2 * cfg["initial_agents"])
    if cfg["spawn_roads"] is not None and not cfg["is_multi_agent"]:
        raise ValueError("spawn_roads is a multi-agent env option")
    if cfg["is_multi_agent"] and cfg["marl_map"] is None:
        raise NotImplementedError("multi-agent configs are built through the multi-agent env classes (marl_map)")
    if cfg["marl_map"] == "parking_lot":
        n = cfg["parking_space_num"]
        assert n % 2 == 0, "number of parking spaces must be multiples of 2"          # marl_parking_lot.py:198-199
        assert n >= 4, "minimal number of parking space is 4"
        if n > 20:
            raise ValueError("parking_space_num > 20: the spawn tables hold 32 places")
    if not cfg["cross_yellow_line_done"] and cfg["marl_map"] not in ("tollgate", "racing"):
        raise NotImplementedError("cross_yellow_line_done=False is built for the tollgate env only")
    if cfg["walk_scenarios"]:
        # the PG walk: what this change does not build is refused by name
        if cfg["is_multi_agent"]:
            raise NotImplementedError("walk_scenarios=True in a multi-agent env is not built (marl_map='pg' included): the walk moves "
                                      "single-agent PG envs")
        if cfg["random_traffic"]:
            raise NotImplementedError("walk_scenarios=True with random_traffic=True is not built: the staged traffic draws would "
                                      "multiply the scenario pool")
        if cfg["traffic_mode"] == "replay":
            raise NotImplementedError("walk_scenarios=True with traffic_mode='replay' is not built: recorded traffic (load_tracks / "
                                      "load_scenarios) belongs to one scenario assignment")
        if not cfg["auto_reset"]:
            raise ValueError("walk_scenarios=True needs auto_reset=True: an env moves on when it resets itself")
        if cfg["walk_stride"] is not None and int(cfg["walk_stride"]) < 1:
            raise ValueError("walk_stride must be >= 1 (the env count over all shards), got {!r}".format(cfg["walk_stride"]))
    if cfg["num_pedestrians"]:
        # crossing pedestrians: built for the single-agent PG envs; everything else is refused by name
        n, pc = cfg["num_pedestrians"], cfg["pedestrian_config"]
        if isinstance(n, bool) or n < 0:
            raise ValueError("num_pedestrians={!r}: an int >= 0".format(n))
        if cfg["is_multi_agent"]:
            raise NotImplementedError("num_pedestrians > 0 in a multi-agent env is not built: crossing pedestrians are placed by the "
                                      "single-agent PG scene builder")
        if cfg["traffic_mode"] == "replay":
            raise NotImplementedError("num_pedestrians > 0 with traffic_mode='replay' is not built: replayed slots take their poses from "
                                      "the recorded frames")
        for k in ("speed", "min_road_length"):
            if not pc[k] > 0:
                raise ValueError("pedestrian_config['{}']={!r}: a positive number".format(k, pc[k]))
        for k in ("wait_min_steps", "clear_dist", "margin", "time_margin", "yield_ahead", "yield_time", "kerb_offset", "spawn_clearance"):
            if pc[k] < 0:
                raise ValueError("pedestrian_config['{}']={!r} must not be negative".format(k, pc[k]))
        if pc["min_road_length"] < 10:
            raise ValueError("pedestrian_config['min_road_length']={!r}: at least 10 m (a crossing keeps 5 m from both road ends)".format(
                pc["min_road_length"]))
    if not isinstance(cfg["contact_response"], bool):
        raise ValueError("contact_response={!r}: True or False".format(cfg["contact_response"]))
    rc = cfg["contact_response_config"]
    for k, ok, what in (("skin", lambda v: v >= 0, "must not be negative"), ("max_push", lambda v: v > 0, "a positive number")):
        if isinstance(rc[k], bool) or not isinstance(rc[k], (int, float)) or not ok(rc[k]):
            raise ValueError("contact_response_config['{}']={!r}: {}".format(k, rc[k], what))
    if cfg["vector_obs"] is not None:
        cfg["vector_obs"] = check_vector_obs(cfg["vector_obs"])
    if cfg["step_kernel"] not in ("auto", "wg", "wave"):
        raise ValueError("step_kernel must be 'auto', 'wg' or 'wave', got {!r}".format(cfg["step_kernel"]))
    if cfg["mover_capacity"] != 0 and (cfg["mover_capacity"] > 128 or cfg["mover_capacity"] < cfg["num_agents"]):
        raise ValueError("mover_capacity must be 0 (auto) or in [num_agents, 128]")
    return cfg
