"""ctypes / numpy mirror of include/mdstep.h.

Every struct of the C-ABI exists here twice: as a numpy structured dtype (for the table arrays the
host builds and uploads) and as a ctypes.Structure (for the three by-pointer argument blocks
MdWorld / MdState / MdConfig).  `check_abi(lib)` compares sizeof() with what the loaded library
reports through md_abi(), so a header/ binding drift fails loudly at import time.
"""
import ctypes as C

import numpy as np

MD_ABI_VERSION = 12
MD_POLY_GROUP = 8     # pieces per MdWorld.poly_ball group
MD_OK, MD_EINVAL, MD_ELAUNCH, MD_ENODEV, MD_EABI = 0, -1, -2, -3, -4
MD_MAX_CAP = 128
MD_MAX_BEAMS = 1024
MD_ROUTE_LEN = 48
MD_IDM_RAND = 8
# MdConfig.agent_idm: the agents' policy on the device
AGENT_INPUT, AGENT_IDM, AGENT_LANE_CHANGE = 0, 1, 2

# mover kinds / flags
KIND_NONE, KIND_VEHICLE, KIND_CONE, KIND_WARNING, KIND_BARRIER, KIND_PEDESTRIAN, KIND_CYCLIST, KIND_BUILDING = range(8)
KIND_MASK = 0xF
F_ALIVE, F_AGENT, F_PENDING, F_STATIC, F_CRASHED_ONCE, F_SPAWNED = 0x10, 0x20, 0x40, 0x80, 0x100, 0x200

# per-step flag word
FL_CRASH_VEHICLE = 0x0001
FL_CRASH_OBJECT = 0x0002
FL_CRASH_HUMAN = 0x0004
FL_CRASH_BUILDING = 0x0008
FL_CRASH_SIDEWALK = 0x0010
FL_ON_WHITE_CONT = 0x0020
FL_ON_YELLOW_CONT = 0x0040
FL_ON_BROKEN = 0x0080
FL_ON_CROSSWALK = 0x0100
FL_ON_LANE = 0x0200
FL_OUT_OF_ROUTE = 0x0400
FL_OUT_OF_ROAD = 0x0800
FL_ARRIVE_DEST = 0x1000
FL_MAX_STEP = 0x2000
FL_TERMINATED = 0x4000
FL_TRUNCATED = 0x8000

Q_LINE_WHITE_CONT, Q_LINE_YELLOW_CONT, Q_LINE_BROKEN, Q_SIDEWALK, Q_CROSSWALK = 1, 2, 3, 4, 5

f4, i4, u1 = np.float32, np.int32, np.uint8

SHAPE_DT = np.dtype([("cx", f4), ("cy", f4), ("c", f4), ("s", f4), ("hl", f4), ("hw", f4), ("flags", i4), ("aux", i4)])
DYN_DT = np.dtype([("heading", f4), ("speed", f4), ("steering", f4), ("throttle", f4), ("last_x", f4),
                   ("last_y", f4), ("last_c", f4), ("last_s", f4)])
PARAM_DT = np.dtype([("max_steer", f4), ("accel_gain", f4), ("brake_gain", f4), ("roll_decel", f4),
                     ("max_speed_kmh", f4), ("lf", f4), ("lr", f4), ("fric_decel", f4)])
NAV_DT = np.dtype([("lane", i4), ("ck0", i4), ("ck1", i4), ("route_len", i4), ("target_lane", i4), ("timer", i4),
                   ("trigger_road", i4), ("trigger_order", i4), ("steps", i4), ("rand_cursor", i4), ("done", i4),
                   ("road0", i4), ("road1", i4), ("toll_state", i4), ("toll_entry", i4), ("toll_exit", i4)])
PID_DT = np.dtype([("hp", f4), ("hi", f4), ("hd", f4), ("lp", f4), ("li", f4), ("ld", f4), ("target_speed", f4),
                   ("energy", f4)])
LANE_DT = np.dtype([("type", i4), ("road", i4), ("idx", i4), ("n_in_road", i4), ("ax", f4), ("ay", f4), ("bx", f4),
                    ("by", f4), ("length", f4), ("width", f4), ("end_phase", f4), ("dirsign", f4), ("angle", f4),
                    ("heading", f4), ("sx", f4), ("sy", f4), ("ex", f4), ("ey", f4), ("x0", f4), ("y0", f4),
                    ("x1", f4), ("y1", f4), ("hull_off", i4), ("hull_n", i4), ("end_phase_w", f4), ("speed_limit", f4),
                    ("elx", f4), ("ely", f4), ("spare", f4, (4, )), ("hull4", f4, (8, ))])
ROAD_DT = np.dtype([("first_lane", i4), ("n_lanes", i4), ("start_node", i4), ("end_node", i4), ("negative", i4),
                    ("block", i4), ("block_kind", i4), ("spare", i4)])
SEG_DT = np.dtype([("sx", f4), ("sy", f4), ("ex", f4), ("ey", f4), ("dx", f4), ("dy", f4), ("len", f4), ("heading", f4),
                   ("cum", f4), ("spare", f4, (3, ))])
MA_DEFAULT, MA_TOLLGATE, MA_PARKING_LOT, MA_RACING = 0, 1, 2, 3
MD_IDLE_WINDOW = 100
FL_IDLE = 0x10000
TM_MOVING, TM_LENGTH_OK, TM_NEVER = 1, 2, 4
SC_ABSENT, SC_REPLAY, SC_IDM, SC_ARRIVED = 0, 1, 2, 3
GRID_DT = np.dtype([("x0", f4), ("y0", f4), ("inv_cell", f4), ("nx", i4), ("ny", i4), ("cell_base", i4),
                    ("spare", i4, (2, ))])

assert SHAPE_DT.itemsize == 32 and DYN_DT.itemsize == 32 and PARAM_DT.itemsize == 32
assert NAV_DT.itemsize == 64 and PID_DT.itemsize == 32 and LANE_DT.itemsize == 160
assert ROAD_DT.itemsize == 32 and GRID_DT.itemsize == 32 and SEG_DT.itemsize == 48

P = C.c_void_p


class MdWorld(C.Structure):
    _fields_ = [
        ("n_maps", C.c_int32), ("n_envs", C.c_int32),
        ("env_map", P), ("lane_off", P), ("lanes", P), ("hull_xy", P), ("road_off", P), ("roads", P),
        ("quad_off", P), ("quads", P), ("quad_kind", P), ("grid", P), ("cell_start", P), ("cell_items", P),
        ("node_adj_off", P), ("node_adj", P), ("node_off", P), ("beam_cs", P),
        ("max_lanes", C.c_int32), ("max_roads", C.c_int32),
        ("spawn_off", P), ("spawn_place", P), ("spawn_lane", P), ("spawn_route", P), ("spawn_route_meta", P),
        ("n_dest", C.c_int32), ("n_vclass", C.c_int32),
        ("poly_off", P), ("segs", P), ("polyv_off", P), ("polyv", P), ("ckpt_off", P), ("ckpt_xy", P), ("track_meta", P), ("vclass", P), ("poly_aux", P), ("side_beam_cs", P), ("ll_beam_cs", P), ("quad_ball", P), ("run_off", P), ("runs", P),
        ("poly_ball", P), ("poly_ball_off", P),
    ]


class MdWalk(C.Structure):
    _fields_ = [("n_scenes", C.c_int32), ("mode", C.c_int32), ("stride", C.c_int32), ("offset", C.c_int32), ("seed", C.c_uint32),
                ("reserved", C.c_int32)]


class MdCurriculum(C.Structure):
    """include/md_curriculum.h: ScenarioEnv's curriculum manager, per env"""
    _fields_ = [("level", P), ("seed", P), ("q_len", P), ("q_key", P), ("q_success", P), ("q_route", P), ("cover", P),
                ("cover_n", P), ("rep_i", P), ("rep_f", P),
                ("n_levels", C.c_int32), ("per_level", C.c_int32), ("eval", C.c_int32), ("n_scenes", C.c_int32),
                ("stride", C.c_int32), ("offset", C.c_int32), ("cover_words", C.c_int32), ("reserved", C.c_int32),
                ("target", C.c_double)]


CURRICULUM_FIELDS = [f for f, t in MdCurriculum._fields_ if t is P]

# include/md_topdown.h: the limits, and md_topdown's argument block
MD_TD_MAX_RES, MD_TD_MAX_RING = 128, 64


class MdTopDown(C.Structure):
    """include/md_topdown.h: the top-down observation's sizes, output and engine-owned history arrays"""
    _fields_ = [("struct_size", C.c_int32), ("resolution", C.c_int32), ("distance", C.c_float), ("frame_stack", C.c_int32),
                ("frame_skip", C.c_int32), ("post_stack", C.c_int32), ("norm_pixel", C.c_int32), ("reserved", C.c_int32),
                ("out", P), ("ring_traffic", P), ("ring_pos", P), ("cursor", P)]


def td_row_words(R):
    """MD_TD_ROW_WORDS: 32-bit words per row of a 1-bit frame"""
    return (R + 31) >> 5


def td_ring_len(stack, skip):
    """md_td_ring_len: the length of stack_traffic_flow / stack_past_pos"""
    return (stack - 1) * skip + 1

# include/md_render.h: the limits, and md_render's argument block
MD_RD_MAX_SIZE, MD_RD_MAX_STACK, MD_RD_TILE = 1024, 32, 64


class MdRender(C.Structure):
    """include/md_render.h: the top-down renderer's window, options, rendered envs, output and engine-owned history arrays"""
    _fields_ = [("struct_size", C.c_int32), ("width", C.c_int32), ("height", C.c_int32), ("scaling", C.c_float),
                ("num_stack", C.c_int32), ("history_smooth", C.c_int32), ("track_agent", C.c_int32), ("heading_up", C.c_int32),
                ("draw_contour", C.c_int32), ("fixed_camera", C.c_int32), ("cam_x", C.c_float), ("cam_y", C.c_float),
                ("n_render", C.c_int32), ("reserved", C.c_int32), ("env_ids", P), ("out", P), ("ring", P), ("cursor", P)]


# include/md_branch.h: the extras table's size, and md_branch's argument block
MD_BR_MAX_EXTRAS = 12


class MdBranchExtra(C.Structure):
    _fields_ = [("dst", P), ("src", P), ("row_bytes", C.c_int64)]


class MdBranch(C.Structure):
    """include/md_branch.h: the (source row, destination row) pairs of one md_branch launch, the row counts of the two states and
    the engine-owned per-env arrays outside MdState"""
    _fields_ = [("struct_size", C.c_int32), ("n_pairs", C.c_int32), ("src_n_envs", C.c_int32), ("dst_n_envs", C.c_int32),
                ("n_extras", C.c_int32), ("reserved", C.c_int32), ("src_row", P), ("dst_row", P),
                ("extra", MdBranchExtra * MD_BR_MAX_EXTRAS)]


# include/md_ped.h: the phases (MdNav.toll_state of a policy-driven pedestrian), and md_ped's argument block
PED_OFF, PED_WAIT_A, PED_CROSS_AB, PED_WAIT_B, PED_CROSS_BA = range(5)


class MdPed(C.Structure):
    """include/md_ped.h: the constants of the crossing rule that all pedestrians share (config pedestrian_config)"""
    _fields_ = [("struct_size", C.c_int32), ("wait_min_steps", C.c_int32), ("clear_dist", C.c_float), ("margin", C.c_float),
                ("time_margin", C.c_float), ("yield_ahead", C.c_float), ("yield_time", C.c_float), ("reserved", C.c_int32)]


def make_md_ped(pedestrian_config):
    p = MdPed()
    p.struct_size, p.wait_min_steps = C.sizeof(MdPed), int(pedestrian_config["wait_min_steps"])
    for k in ("clear_dist", "margin", "time_margin", "yield_ahead", "yield_time"):
        setattr(p, k, float(pedestrian_config[k]))
    return p


class MdContactResponse(C.Structure):
    """include/md_contact_response.h: the two lengths of the contact response rule (config contact_response_config)"""
    _fields_ = [("struct_size", C.c_int32), ("skin", C.c_float), ("max_push", C.c_float), ("reserved", C.c_int32)]


def make_md_contact_response(contact_response_config):
    cr = MdContactResponse()
    cr.struct_size = C.sizeof(MdContactResponse)
    cr.skin, cr.max_push = float(contact_response_config["skin"]), float(contact_response_config["max_push"])
    return cr


def row_blocks(blocks):
    """The per-env row layout ("Per-env row blocks"): blocks = (name, shape after the env axis, dtype), ... -> (table, row
    bytes) with table[name] = (byte offset in an env's row, shape, numpy dtype).  Every block starts 16-byte aligned; a block whose
    count is 0 has no bytes and shares its offset with its successor."""
    table, at = {}, 0
    for name, shape, dt in blocks:
        table[name] = (at, tuple(shape), np.dtype(dt))
        at = (at + int(np.prod(shape)) * np.dtype(dt).itemsize + 15) // 16 * 16
    return table, at


def block_bytes(table, name):
    _, shape, dt = table[name]
    return int(np.prod(shape)) * dt.itemsize


def block_ptrs(table, base):
    """name -> address of env 0's block in rows that start at `base`; a block without bytes is left out (its pointer stays NULL)"""
    return {name: base + table[name][0] for name in table if block_bytes(table, name)}


def block_of(rows, table, name):
    """a typed copy [E, ...] of the block `name` of the [E, row bytes] uint8 array `rows`"""
    off, shape, dt = table[name]
    return rows[:, off:off + block_bytes(table, name)].copy().view(dt).reshape((rows.shape[0], ) + shape)     # (E = 1: a slice is contiguous)


# include/md_vector_obs.h: the ceilings MD_VO_MAX_*, and md_vector_obs's argument block
MD_VO_MAX_AGENTS, MD_VO_MAX_HISTORY, MD_VO_MAX_ROUTE_POINTS, MD_VO_MAX_LANES, MD_VO_MAX_LANE_POINTS = 16, 8, 32, 16, 16
VECTOR_OBS_OUTPUTS = ("agents", "agents_mask", "agents_meta", "ego", "ego_mask", "route", "route_mask", "lanes", "lanes_meta", "lanes_mask")
VECTOR_OBS_HISTORY = ("ring_pose", "ring_flags", "cursor")


class MdVectorObs(C.Structure):
    """include/md_vector_obs.h: the vector scene observation's counts and lengths, the per-env strides, its outputs and the
    engine-owned history arrays"""
    _fields_ = [("struct_size", C.c_int32), ("num_agents", C.c_int32), ("history", C.c_int32), ("route_points", C.c_int32),
                ("num_lanes", C.c_int32), ("lane_points", C.c_int32), ("radius", C.c_float), ("max_jump", C.c_float),
                ("route_spacing", C.c_float), ("reserved", C.c_int32), ("out_stride", C.c_int32), ("hist_stride", C.c_int32)] + \
        [(k, P) for k in VECTOR_OBS_OUTPUTS + VECTOR_OBS_HISTORY]


def _history_blocks(T, cap):
    """the engine-owned history both vector observations keep: the pose ring, the flag ring, the cursor"""
    return [("ring_pose", (T, cap, 4), f4), ("ring_flags", (T, cap), i4), ("cursor", (4, ), i4)]


def vector_obs_blocks(vo_cfg, A, cap):
    """-> (outputs, output row bytes, history, history row bytes); outputs / history: name -> (byte offset in an env's row, shape
    after the env axis, numpy dtype), laid out by row_blocks.  One output row and one history row per env."""
    K, T, M, Pn, S = (int(vo_cfg[k]) for k in ("num_agents", "history", "route_points", "num_lanes", "lane_points"))
    outs = [("agents", (A, K, T, 4), f4), ("agents_mask", (A, K, T), u1), ("agents_meta", (A, K, 4), f4), ("ego", (A, T, 4), f4),
            ("ego_mask", (A, T), u1), ("route", (A, M, 4), f4), ("route_mask", (A, M), u1), ("lanes", (A, Pn, S, 2), f4),
            ("lanes_meta", (A, Pn, 4), f4), ("lanes_mask", (A, Pn), u1)]
    return row_blocks(outs) + row_blocks(_history_blocks(T, cap))


def make_md_vector_obs(vo_cfg, tensors):
    """MdVectorObs of the finished config["vector_obs"]; `tensors`: out_stride, hist_stride and name -> device address of env 0's
    block (None / missing: NULL)"""
    v = MdVectorObs()
    v.struct_size = C.sizeof(MdVectorObs)
    for k in ("num_agents", "history", "route_points", "num_lanes", "lane_points"):
        setattr(v, k, int(vo_cfg[k]))
    for k in ("radius", "max_jump", "route_spacing"):
        setattr(v, k, float(vo_cfg[k]))
    v.out_stride, v.hist_stride = int(tensors["out_stride"]), int(tensors["hist_stride"])
    for k in VECTOR_OBS_OUTPUTS + VECTOR_OBS_HISTORY:
        setattr(v, k, tensors.get(k))
    return v


# include/md_scenario_vector_obs.h: the ceilings MD_SVO_MAX_*, and md_scenario_vector_obs's argument block
MD_SVO_MAX_MAP_PIECES, MD_SVO_MAX_PIECE_POINTS, MD_SVO_MAX_PIECES = 64, 16, 4096
SCENARIO_VECTOR_OBS_OUTPUTS = ("agents", "agents_mask", "agents_meta", "ego", "ego_mask", "route", "route_mask", "map", "map_mask", "map_meta")
SCENARIO_VECTOR_OBS_MAP_OUTPUTS = ("map", "map_mask", "map_meta")
SCENARIO_VECTOR_OBS_TABLES = ("map_off", "map_xy", "map_info", "map_ball")


class MdScenarioVectorObs(C.Structure):
    """include/md_scenario_vector_obs.h: the map block's counts and radius, md_vector_obs.h's struct (num_lanes = 0) for everything
    the two observations share, the map outputs and the engine-owned per-scene piece table"""
    _fields_ = [("struct_size", C.c_int32), ("num_pieces", C.c_int32), ("piece_points", C.c_int32), ("max_pieces", C.c_int32),
                ("map_radius", C.c_float), ("reserved", C.c_int32), ("vo", MdVectorObs)] + \
        [(k, P) for k in SCENARIO_VECTOR_OBS_MAP_OUTPUTS + SCENARIO_VECTOR_OBS_TABLES]


def scenario_vector_obs_blocks(vo_cfg, cap):
    """-> (outputs, output row bytes, history, history row bytes), like vector_obs_blocks: name -> (byte offset in an env's row, shape
    after the env axis, numpy dtype).  One observer per env, so the shapes have no agent axis."""
    K, T, M, Pn, S = (int(vo_cfg[k]) for k in ("num_agents", "history", "route_points", "num_pieces", "piece_points"))
    outs = [("agents", (K, T, 4), f4), ("agents_mask", (K, T), u1), ("agents_meta", (K, 4), f4), ("ego", (T, 4), f4), ("ego_mask", (T, ), u1),
            ("route", (M, 4), f4), ("route_mask", (M, ), u1), ("map", (Pn, S, 2), f4), ("map_mask", (Pn, S), u1), ("map_meta", (Pn, 4), f4)]
    return row_blocks(outs) + row_blocks(_history_blocks(T, cap))


def make_md_scenario_vector_obs(vo_cfg, tensors):
    """MdScenarioVectorObs of the finished config["scenario_vector_obs"]; `tensors`: out_stride, hist_stride, max_pieces and name ->
    address of env 0's block / of the table (None / missing: NULL)"""
    v = MdScenarioVectorObs()
    v.struct_size = C.sizeof(MdScenarioVectorObs)
    v.num_pieces, v.piece_points = int(vo_cfg["num_pieces"]), int(vo_cfg["piece_points"])
    v.max_pieces, v.map_radius = int(tensors.get("max_pieces", 0)), float(vo_cfg["map_radius"])
    shared = dict(vo_cfg, num_lanes=0, lane_points=2)
    v.vo = make_md_vector_obs(shared, {k: tensors.get(k) for k in ("out_stride", "hist_stride") + VECTOR_OBS_OUTPUTS + VECTOR_OBS_HISTORY
                                       if not k.startswith("lanes")})
    for k in SCENARIO_VECTOR_OBS_MAP_OUTPUTS + SCENARIO_VECTOR_OBS_TABLES:
        setattr(v, k, tensors.get(k))
    return v


# include/md_traffic_lights.h: the ceilings MD_TL_MAX_*, the status codes, and md_traffic_lights's argument block
MD_TL_MAX_LIGHTS, MD_TL_MAX_SCENE_LIGHTS = 32, 1024
TL_UNKNOWN, TL_GREEN, TL_YELLOW, TL_RED = 0, 1, 2, 3
TL_BIT_GREEN, TL_BIT_YELLOW, TL_BIT_RED = 1, 2, 4
TRAFFIC_LIGHTS_OUTPUTS = ("agent_light", "lights", "lights_mask", "lights_index")
TRAFFIC_LIGHTS_TABLES = ("tl_off", "tl_box", "tl_info", "tl_status")


class MdTrafficLights(C.Structure):
    """include/md_traffic_lights.h: L, the radius, the largest scene, the stride, the engine-owned per-scene light tables, the outputs"""
    _fields_ = [("struct_size", C.c_int32), ("num_lights", C.c_int32), ("radius", C.c_float), ("max_scene_lights", C.c_int32),
                ("out_stride", C.c_int32), ("reserved", C.c_int32)] + [(k, P) for k in TRAFFIC_LIGHTS_TABLES + TRAFFIC_LIGHTS_OUTPUTS]


def traffic_lights_blocks(tl_cfg):
    """-> (outputs, output row bytes): name -> (byte offset in an env's row, shape after the env axis, numpy dtype), laid out by
    row_blocks.  agent_light is one byte per env."""
    L = int(tl_cfg["num_lights"])
    return row_blocks([("agent_light", (), u1), ("lights", (L, 6), f4), ("lights_mask", (L, ), u1), ("lights_index", (L, ), i4)])


def make_md_traffic_lights(tl_cfg, tensors):
    """MdTrafficLights of the finished config["traffic_lights"]; `tensors`: out_stride, max_scene_lights and name -> address of env 0's
    block / of the table (None / missing: NULL)"""
    v = MdTrafficLights()
    v.struct_size = C.sizeof(MdTrafficLights)
    v.num_lights, v.radius = int(tl_cfg["num_lights"]), float(tl_cfg["radius"])
    v.max_scene_lights, v.out_stride = int(tensors.get("max_scene_lights", 0)), int(tensors.get("out_stride", 0))
    for k in TRAFFIC_LIGHTS_TABLES + TRAFFIC_LIGHTS_OUTPUTS:
        setattr(v, k, tensors.get(k))
    return v


# include/md_scenario_metrics.h: the ceiling MD_SM_MAX_TTC_SAMPLES, the columns by name, and md_scenario_metrics's argument block
MD_SM_MAX_TTC_SAMPLES, MD_SM_STEP_COLS, MD_SM_EPISODE_COLS, MD_SM_STATE_COLS = 64, 12, 24, 12
SCENARIO_METRICS_STEP_COLUMNS = ("log_divergence", "log_heading_error", "speed", "lon_accel", "yaw_rate", "lat_accel", "lon_jerk",
                                 "yaw_accel", "jerk", "ttc", "on_red", "reserved")
SCENARIO_METRICS_EPISODE_COLUMNS = ("steps", "ade", "max_divergence", "fde", "max_heading_error", "min_ttc", "ttc_violation_steps",
                                    "max_lon_accel", "min_lon_accel", "max_abs_lat_accel", "max_abs_lon_jerk", "max_jerk",
                                    "max_abs_yaw_rate", "max_abs_yaw_accel", "comfort_violation_steps", "red_light_steps",
                                    "collision_steps", "out_of_road_steps", "route_completion", "arrive_dest") + ("reserved", ) * 4
SCENARIO_METRICS_HISTORY_COLUMNS = ("v", "h", "lon_accel", "yaw_rate", "lat_accel", "clock", "rates", "latched", "divergence_sum",
                                    "divergence_steps", "reserved", "reserved")
SCENARIO_METRICS_BOUNDS = ("max_lon_accel", "min_lon_accel", "max_lat_accel", "max_lon_jerk", "max_jerk", "max_yaw_rate", "max_yaw_accel")
SCENARIO_METRICS_OUTPUTS = ("step", "step_valid", "ttc_slot", "last_episode", "episodes")


class MdScenarioMetrics(C.Structure):
    """include/md_scenario_metrics.h: the sweep's J and period, the thresholds, the strides, agent_light, the outputs, the state rows"""
    _fields_ = ([("struct_size", C.c_int32), ("ttc_samples", C.c_int32), ("ttc_dt", C.c_float), ("ttc_threshold", C.c_float)] +
                [(k, C.c_float) for k in SCENARIO_METRICS_BOUNDS] +
                [("out_stride", C.c_int32), ("state_stride", C.c_int32), ("light_stride", C.c_int32), ("agent_light", P)] +
                [(k, P) for k in SCENARIO_METRICS_OUTPUTS + ("state", )])


def scenario_metrics_blocks(sm_cfg=None):
    """-> (outputs, output row bytes, state, state row bytes): name -> (byte offset in an env's row, shape after the env axis, numpy
    dtype), the outputs laid out by row_blocks.  The layout is the same for every config (`sm_cfg` is taken as the sibling *_blocks take
    theirs).  step_valid, a uint32 of 11 bits in the header, is viewed as int32, torch's own word type.  The state row is the history
    (MD_SM_STATE_COLS words) with the running episode behind it."""
    outs = [("step", (MD_SM_STEP_COLS, ), f4), ("step_valid", (), i4), ("ttc_slot", (), i4), ("last_episode", (MD_SM_EPISODE_COLS, ), f4),
            ("episodes", (), i4)]
    state = {"history": (0, (MD_SM_STATE_COLS, ), np.dtype(f4)), "episode": (4 * MD_SM_STATE_COLS, (MD_SM_EPISODE_COLS, ), np.dtype(f4))}
    return row_blocks(outs) + (state, 4 * (MD_SM_STATE_COLS + MD_SM_EPISODE_COLS))


def make_md_scenario_metrics(sm_cfg, tensors):
    """MdScenarioMetrics of the finished config["scenario_metrics"]; `tensors`: out_stride, state_stride, light_stride and name ->
    address of env 0's block (None / missing: NULL)"""
    v = MdScenarioMetrics()
    v.struct_size = C.sizeof(MdScenarioMetrics)
    v.ttc_samples, v.ttc_dt, v.ttc_threshold = int(sm_cfg["ttc_samples"]), float(sm_cfg["ttc_dt"]), float(sm_cfg["ttc_threshold"])
    for k in SCENARIO_METRICS_BOUNDS:
        setattr(v, k, float(sm_cfg[k]))
    for k in ("out_stride", "state_stride", "light_stride"):
        setattr(v, k, int(tensors.get(k, 0)))
    for k in ("agent_light", "state") + SCENARIO_METRICS_OUTPUTS:
        setattr(v, k, tensors.get(k))
    return v


class MdState(C.Structure):
    _fields_ = [
        ("shape", P), ("dyn", P), ("param", P), ("nav", P), ("pid", P), ("action", P), ("route_nodes", P),
        ("route_roads", P), ("final_lane", P), ("idm_rand", P), ("flags", P), ("obs", P), ("reward", P), ("cost", P),
        ("step_info", P), ("need_reset", P), ("shape0", P), ("dyn0", P), ("nav0", P), ("pid0", P),
        ("route_nodes0", P), ("route_roads0", P), ("final_lane0", P), ("rng", P), ("env_steps", P), ("agent_id", P),
        ("next_agent_id", P),
        ("agent_action", P),
        ("track_shape", P),
        ("track_dyn", P),
        ("detected", P),
        ("scratch", P),
        ("param0", P),
        ("done_out", P),
        ("route_n", P), ("route_segs", P), ("route_verts", P), ("route_aux", P), ("idle_ring", P),
        ("scene_of", P), ("walk_ep", P),
        ("walk", MdWalk),
    ]


class MdConfig(C.Structure):
    _fields_ = [
        ("struct_size", C.c_int32), ("n_envs", C.c_int32), ("agents_per_env", C.c_int32), ("cap", C.c_int32),
        ("n_beams", C.c_int32), ("obs_dim", C.c_int32), ("substeps", C.c_int32), ("horizon", C.c_int32),
        ("dt", C.c_float), ("lidar_range", C.c_float),
        ("success_reward", C.c_float), ("out_of_road_penalty", C.c_float), ("crash_vehicle_penalty", C.c_float),
        ("crash_object_penalty", C.c_float), ("driving_reward", C.c_float), ("speed_reward", C.c_float),
        ("crash_vehicle_cost", C.c_float), ("crash_object_cost", C.c_float), ("out_of_road_cost", C.c_float),
        ("use_lateral_reward", C.c_int32), ("out_of_route_done", C.c_int32), ("on_continuous_line_done", C.c_int32),
        ("crash_vehicle_done", C.c_int32), ("crash_object_done", C.c_int32), ("crash_human_done", C.c_int32),
        ("truncate_as_terminate", C.c_int32), ("traffic_mode", C.c_int32), ("enable_idm_lane_change", C.c_int32),
        ("auto_reset", C.c_int32),
        ("max_lane_width", C.c_float), ("total_width", C.c_float), ("curve_radius_max", C.c_float),
        ("curve_angle_max", C.c_float),
        ("is_multi_agent", C.c_int32), ("delay_done", C.c_int32), ("allow_respawn", C.c_int32),
        ("crash_done", C.c_int32), ("out_of_road_done", C.c_int32), ("n_side", C.c_int32), ("n_lane_line", C.c_int32),
        ("num_others", C.c_int32),
        ("add_others_navi", C.c_int32),
        ("track_len", C.c_int32),
        ("random_agent_model", C.c_int32),
        ("agent_idm", C.c_int32),
        ("enable_reverse", C.c_int32),
        ("on_lane_line_penalty", C.c_float), ("crash_human_penalty", C.c_float), ("steering_range_penalty", C.c_float),
        ("heading_penalty", C.c_float), ("lateral_penalty", C.c_float), ("max_lateral_dist", C.c_float),
        ("crash_human_cost", C.c_float),
        ("no_negative_reward", C.c_int32), ("relax_out_of_road_done", C.c_int32), ("reactive_traffic", C.c_int32),
        ("filter_overlapping_car", C.c_int32), ("no_static_vehicles", C.c_int32), ("allowed_more_steps", C.c_int32),
        ("scenario_length", C.c_int32),
        ("step_kernel", C.c_int32),
        ("ma_kind", C.c_int32), ("min_pass_steps", C.c_int32), ("overspeed_penalty", C.c_float), ("n_parking", C.c_int32),
        ("side_range", C.c_float), ("ll_range", C.c_float), ("side_mask", C.c_uint32), ("ll_mask", C.c_uint32),
        ("route_seg_cap", C.c_int32), ("route_vert_cap", C.c_int32), ("ego_replay", C.c_int32),
        ("crash_sidewalk_penalty", C.c_float), ("idle_penalty", C.c_float), ("idle_done", C.c_int32), ("crash_sidewalk_done", C.c_int32),
    ]


STRUCT_SIZES = [SHAPE_DT.itemsize, DYN_DT.itemsize, PARAM_DT.itemsize, NAV_DT.itemsize, PID_DT.itemsize,
                LANE_DT.itemsize, ROAD_DT.itemsize, GRID_DT.itemsize, C.sizeof(MdWorld), C.sizeof(MdState),
                C.sizeof(MdConfig)]
STRUCT_NAMES = ["MdShape", "MdDyn", "MdParam", "MdNav", "MdPid", "MdLane", "MdRoad", "MdGrid", "MdWorld", "MdState",
                "MdConfig"]

WORLD_FIELDS = [f for f, t in MdWorld._fields_ if t is P]
STATE_FIELDS = [f for f, t in MdState._fields_ if t is P]

_W, _S, _K = C.POINTER(MdWorld), C.POINTER(MdState), C.POINTER(MdConfig)
_i, _f, _u = C.c_int, C.c_float, C.c_uint32
_PHASE = (_i, [_W, _S, _K, P])
# the C-ABI's functions, name -> (restype, argtypes), one table per header; _lib.load() sets them all
# include/mdstep.h
ENTRY_POINTS = {
    "md_abi": (_i, [C.POINTER(C.c_int32), _i]),
    "md_last_error": (C.c_char_p, []),
    "md_probe_math": (_i, [_i, P, P, P, _i, P]),
    "md_probe_stream_copy": (_i, [P, P, C.c_size_t, P]),
    "md_lidar": (_i, [_W, _S, _K, P, _i, _i, P]),
    "md_lidar_detect": (_i, [_W, _S, _K, P, _i, _i, P, P]),
    "md_line_detector": (_i, [_W, _S, _K, P, _i, _f, _u, P, _i, _i, P]),
    "md_line_detectors": (_i, [_W, _S, _K, P, _i, _f, _u, _i, P, _i, _f, _u, _i, P, _i, P]),
    "md_swap_draw": (_i, [_S, _S, _K, _i, P, P]),
    "md_integrate": _PHASE, "md_localize": _PHASE, "md_contacts": _PHASE, "md_observe": _PHASE, "md_idm": _PHASE,
    "md_traffic_after_step": _PHASE, "md_lifecycle": _PHASE, "md_step": _PHASE,
}
# include/md_expert.h
EXPERT_ENTRY_POINTS = {"md_expert": (_i, [_W, _S, _K, P, P, P, P, P, P])}
# include/md_ai_protect.h: (w, s, c, weights, noise, actions, save_level, takeover, expert_takeover, applied_out, flags_out, saver_out, stream)
AI_PROTECT_ENTRY_POINTS = {"md_ai_protect": (_i, [_W, _S, _K, P, P, P, _f, P, P, P, P, P, P])}
# include/md_expert_sense.h: (w, s, c, weights, beam_cs240, noise, action_out, mlp_out, obs_out, stream)
EXPERT_SENSE_ENTRY_POINTS = {"md_expert_sense": (_i, [_W, _S, _K, P, P, P, P, P, P, P])}
AIP_TAKEOVER, AIP_TAKEOVER_START, AIP_TAKEOVER_END = 1, 2, 4      # md_ai_protect's flag byte
# include/md_curriculum.h
CURRICULUM_ENTRY_POINTS = {"md_curriculum": (_i, [_S, _S, _K, C.POINTER(MdCurriculum), P, _i, P])}
# include/md_topdown.h: (w, s, c, td, stream)
TOPDOWN_ENTRY_POINTS = {"md_topdown": (_i, [_W, _S, _K, C.POINTER(MdTopDown), P])}
# include/md_render.h: (w, s, c, r, stream)
RENDER_ENTRY_POINTS = {"md_render": (_i, [_W, _S, _K, C.POINTER(MdRender), P])}
# include/md_branch.h: (dst, src, c, b, stream)
BRANCH_ENTRY_POINTS = {"md_branch": (_i, [_S, _S, _K, C.POINTER(MdBranch), P])}
# include/md_ped.h: (s, c, p, stream)
PED_ENTRY_POINTS = {"md_ped": (_i, [_S, _K, C.POINTER(MdPed), P])}
# include/md_contact_response.h: (s, c, cr, stream)
CONTACT_RESPONSE_ENTRY_POINTS = {"md_contact_response": (_i, [_S, _K, C.POINTER(MdContactResponse), P])}
# include/md_vector_obs.h: (w, s, c, vo, stream)
VECTOR_OBS_ENTRY_POINTS = {"md_vector_obs": (_i, [_W, _S, _K, C.POINTER(MdVectorObs), P])}
# include/md_scenario_vector_obs.h: (w, s, c, sv, stream)
SCENARIO_VECTOR_OBS_ENTRY_POINTS = {"md_scenario_vector_obs": (_i, [_W, _S, _K, C.POINTER(MdScenarioVectorObs), P])}
# include/md_traffic_lights.h: (w, s, c, tl, stream)
TRAFFIC_LIGHTS_ENTRY_POINTS = {"md_traffic_lights": (_i, [_W, _S, _K, C.POINTER(MdTrafficLights), P])}
# include/md_scenario_metrics.h: (w, s, c, sm, stream)
SCENARIO_METRICS_ENTRY_POINTS = {"md_scenario_metrics": (_i, [_W, _S, _K, C.POINTER(MdScenarioMetrics), P])}
# declared in no header: the hooks of diagnostic (-DMD_STAMP) builds, and md_localize through the lean step's road-first path
# (the parity tests call it; a -DMD_LOC_ROAD_FIRST=0 build runs the plain walk under that name)
OPTIONAL_ENTRY_POINTS = {"md_debug_set_stamp_buffer": (_i, [P]), "md_debug_set_env_order": (_i, [P]),
                         "md_localize_road_first": _PHASE}


def check_abi(abi_fn, what):
    sizes = (C.c_int32 * 11)()
    ver = abi_fn(sizes, 11)
    if ver != MD_ABI_VERSION:
        raise RuntimeError("%s: ABI version %d, binding expects %d" % (what, ver, MD_ABI_VERSION))
    for name, mine, theirs in zip(STRUCT_NAMES, STRUCT_SIZES, list(sizes)):
        if mine != theirs:
            raise RuntimeError("%s: sizeof(%s) = %d in the library but %d in the Python binding" %
                               (what, name, theirs, mine))


def fill_struct(struct, fields, arrays, ptr_of):
    """Set every pointer field of `struct` from `arrays[field]` (None -> NULL) using ptr_of(array)."""
    for f in fields:
        a = arrays.get(f)
        setattr(struct, f, None if a is None else ptr_of(a))
    return struct
