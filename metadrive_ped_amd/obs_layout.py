"""ObsLayout: which dims sit where in one observation row.

The authority is the C header: md_obs_base / md_obs_mid / md_obs_ll / md_obs_navi / md_navi_dims / md_obs_others /
md_others_width / md_obs_lidar / md_obs_tail in include/md_entity.h, and md_sc_obs_navi / md_sc_obs_lidar in
include/md_scenario.h (obs/state_obs.py:64-151, marl_tollgate.py:62-110 of the reference).  This class is their Python
mirror, member for member, and the only place in the host layer that does this arithmetic: the host scenes size their obs
arrays with it, the env classes their observation_space, the engine its detector launches.

    [length, width] | side cloud (or 2 dims) | 6 state dims | lane-line cloud (or 1 dim) | navi | others | lidar | tail
    0        obs_base=side_off              mid_off         ll_off                       navi_off others_off lidar_off
"""

SCENARIO_NAVI_DIMS = 22       # MD_TRAJ_NAVI_DIM


def _beams(detector):
    """A detector's beam count; a detector with distance <= 0 is off, whatever its num_lasers says."""
    return int(detector["num_lasers"]) if detector["distance"] > 0 else 0


class ObsLayout:
    """Counts and offsets only, from a finished config.  `scenario`: the layout of BatchedScenarioEnv (22 trajectory
    navigation dims, no [length, width], no others block); None reads config["scenario_mode"]."""
    def __init__(self, cfg, scenario=None):
        vc = cfg["vehicle_config"]
        scenario = bool(cfg.get("scenario_mode")) if scenario is None else scenario
        self.tollgate = not scenario and bool(cfg["is_multi_agent"]) and cfg["marl_map"] == "tollgate"
        self.n_beams, self.n_side, self.n_ll = _beams(vc["lidar"]), _beams(vc["side_detector"]), _beams(vc["lane_line_detector"])
        self.obs_base = 2 if cfg["random_agent_model"] and not scenario else 0      # [length, width] lead the state dims
        self.side_off = self.obs_base                      # SideDetector cloud replaces 2 dims (obs/state_obs.py:77-86)
        self.mid_off = self.side_off + (self.n_side or 2)
        self.ll_off = self.mid_off + 6                     # LaneLineDetector cloud replaces the lateral dim (:129-140)
        self.navi_off = self.ll_off + (self.n_ll or 1)
        # the tollgate env's state observation has no navigation dims (marl_tollgate.py:62-74)
        self.navi_dims = SCENARIO_NAVI_DIMS if scenario else 0 if self.tollgate else 10
        self.others_off = self.state_dim = self.navi_off + self.navi_dims       # 19 with everything off
        # the "others" block only exists with the lidar on (obs/state_obs.py:172-183)
        self.num_others = int(vc["lidar"]["num_others"]) if self.n_beams > 0 and not scenario else 0
        self.add_others_navi = bool(vc["lidar"]["add_others_navi"]) and self.num_others > 0
        self.others_dim = self.num_others * (8 if self.add_others_navi else 4)
        self.lidar_off = self.others_off + self.others_dim
        self.tail = 2 if self.tollgate else 0              # [in toll block, stayed long enough] after the cloud
        self.obs_dim = self.lidar_off + self.n_beams + self.tail

    # what HostScene / ScenarioHostScene keep as attributes of their own (bench.py, the oracle binding and the tests read them)
    HOST_ATTRS = ("n_beams", "n_side", "n_ll", "obs_base", "tollgate", "state_dim", "num_others", "add_others_navi",
                  "others_dim", "obs_dim")

    def export_to(self, host):
        host.layout = self
        for k in self.HOST_ATTRS:
            setattr(host, k, getattr(self, k))
