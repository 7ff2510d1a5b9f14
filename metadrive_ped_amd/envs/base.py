"""BatchedEnvBase: what the three env families (BatchedMetaDriveEnv, BatchedMultiAgentRoundaboutEnv, BatchedScenarioEnv) share --
the engine's lifecycle, action coercion, the done flags, the flag-bit entries of the lazy info and the checkpoint validation.
Each family keeps its own reset() (they differ in what a seed means) and its own step() result shape."""
import numpy as np

from metadrive_ped_amd import abi
from metadrive_ped_amd.envs.spaces import Box
from metadrive_ped_amd.obs_layout import ObsLayout

# info key -> flag bits, for every family; the single-agent families add SINGLE_AGENT_FLAG_INFO
FLAG_INFO = (("crash_vehicle", abi.FL_CRASH_VEHICLE), ("crash_object", abi.FL_CRASH_OBJECT), ("crash_sidewalk", abi.FL_CRASH_SIDEWALK),
             ("out_of_road", abi.FL_OUT_OF_ROAD), ("arrive_dest", abi.FL_ARRIVE_DEST), ("max_step", abi.FL_MAX_STEP))
SINGLE_AGENT_FLAG_INFO = FLAG_INFO + (
    ("crash_building", abi.FL_CRASH_BUILDING), ("crash_human", abi.FL_CRASH_HUMAN),
    ("crash", abi.FL_CRASH_VEHICLE | abi.FL_CRASH_OBJECT | abi.FL_CRASH_BUILDING | abi.FL_CRASH_SIDEWALK | abi.FL_CRASH_HUMAN))


class BatchedEnvBase:
    FLAG_INFO = FLAG_INFO
    RENDER_MESSAGE = "rendering lies outside this build (DESIGN.md section 1)"
    # the checkpoint's seeds differ from the batch's: (the config key that bases them, what would not match)
    ASSIGNMENT = ("start_seed", "maps")

    def __init__(self, config, scenario=False):
        """`config`: the finished config.  The observation space comes from the one ObsLayout, like the host scene's obs_dim."""
        self.config = config
        self.num_envs = config["num_envs"]
        self.observation_space = Box(-0.0, 1.0, (ObsLayout(self.config, scenario=scenario).obs_dim, ), np.float32)
        self.engine = None
        self.top_down_renderer = None      # the BatchedTopDownRenderer of render(mode="topdown"), None before the first call

    # -- lifecycle ----------------------------------------------------------------------------
    def _build_host(self):
        """The host scene of a new engine; None: BatchedEngine builds a HostScene from the config."""
        return None

    def lazy_init(self, host=None):
        """`host`: a host scene already built from this env's config (e.g. before the GPU was touched)."""
        if self.engine is None:
            from metadrive_ped_amd.engine import BatchedEngine
            self.engine = BatchedEngine(self.config, host=host or self._build_host())

    def close(self):
        self.engine = None
        self.top_down_renderer = None

    def seed(self, seed=None):
        """BaseEnv.seed: scenario seeds are set through reset(seed=...); kept as a no-op like the gymnasium API."""

    def render(self, text=None, mode=None, envs=None, screen_size=(512, 512), scaling=5, num_stack=15, history_smooth=0, camera_position=None,
               target_vehicle_heading_up=False, draw_contour=True, track_agent=0, screen_record=False, window=False, film_size=None, **refused):
        """BaseEnv.render (envs/base_env.py:482-492) for the modes "top_down" | "topdown" | "bev" | "birdview": the reference's
        TopDownRenderer, rasterised on the device (include/md_render.h) -> uint8 device tensor [len(envs), H, W, 3], RGB, of the envs
        `envs` (None: env 0); screen_size is (width, height), `scaling` pixels per metre.  The tensor is rewritten by the next call.
        The first call after reset() fixes the options, as the reference's first call of an episode does; a later call with other
        options raises ValueError, and reset() drops the renderer (env.top_down_renderer) with its history.  The history of an env
        that auto-resets empties itself; a caller that renders less often than every step can miss a reset, and in a walking batch
        the one frame between an episode's end and its reset step is drawn on the next scene's map (the swap happens inside step()).
        `film_size` is accepted and has nothing to act on: there is no film canvas, the window is sampled from the geometry itself.
        Not built, refused by name: window=True, a non-empty `text`, semantic_map, draw_target_vehicle_trajectory, show_agent_name.
        Every other mode: NotImplementedError(RENDER_MESSAGE)."""
        from metadrive_ped_amd import render as rd
        if mode not in rd.TOPDOWN_MODES:
            raise NotImplementedError(self.RENDER_MESSAGE)
        if window:
            raise NotImplementedError("render(window=True): there is no on-screen window; the frames are device tensors")
        if text:
            raise NotImplementedError("render(text=...): the text overlay is not built")
        for k, v in refused.items():
            if k not in rd.REFUSED_OPTIONS:
                raise TypeError("render() got an unexpected keyword argument {!r}".format(k))
            if v:
                raise NotImplementedError("render({}=True) is not built".format(k))
        options = rd.check_options(self.num_envs, int(self.config["num_agents"]), envs=envs, screen_size=screen_size, scaling=scaling,
                                   num_stack=num_stack, history_smooth=history_smooth, camera_position=camera_position,
                                   target_vehicle_heading_up=target_vehicle_heading_up, draw_contour=draw_contour, track_agent=track_agent,
                                   screen_record=screen_record)
        self._require_engine("render")
        if self.top_down_renderer is None:
            self.top_down_renderer = rd.BatchedTopDownRenderer(self.engine, options)
        elif self.top_down_renderer.options != options:
            changed = sorted(k for k, v in options.items() if self.top_down_renderer.options[k] != v)
            raise ValueError("render: the first call after reset() fixed the renderer's options; {} changed (reset() drops the "
                             "renderer)".format(", ".join(changed)))
        return self.top_down_renderer.render()

    def _require_engine(self, what):
        if self.engine is None:
            raise RuntimeError("call reset() before {}()".format(what))

    # -- step() helpers -----------------------------------------------------------------------
    def _coerce_actions(self, actions, lead_shape, discrete):
        """-> float tensor [*lead_shape, 2]: a tensor is taken as it is, anything else goes through numpy; ONE action [2] is
        given to every vehicle; `discrete`: grid indices, through discrete_to_continuous."""
        torch = self.engine.torch
        if discrete:
            from metadrive_ped_amd.envs.metadrive_env import discrete_to_continuous
            a = discrete_to_continuous(torch, self.config, actions, lead_shape, self.engine.device)
        else:
            a = actions if torch.is_tensor(actions) else torch.as_tensor(np.asarray(actions, dtype=np.float32))
            if a.dim() == 1:
                a = a.expand(*lead_shape, 2)
        if tuple(a.shape) != tuple(lead_shape) + (2, ):
            raise ValueError("actions must have shape [{}, 2], got {}".format(", ".join(map(str, lead_shape)), tuple(a.shape)))
        return a

    def _done_flags(self, agents=0):
        """(terminated, truncated) of slot(s) `agents` (0: the single agent; a slice: the agent slots).  Written by md_step itself
        (MdState.done_out): no device op at all -- every eager torch op costs ~5 us, several percent of a step.  Like obs and
        reward these are views of the engine's buffers: the next step() overwrites them, .clone() what has to outlive it.
        Without done_out: the two bits of the flag word."""
        e = self.engine
        if e.done_tt is not None:
            return e.done_tt[:, agents, 0], e.done_tt[:, agents, 1]
        fl = e.flags[:, agents]
        return (fl & abi.FL_TERMINATED) != 0, (fl & abi.FL_TRUNCATED) != 0

    def _flag_info(self, fl):
        """The lazy info entries that test bits of the flag words `fl`: this family's FLAG_INFO."""
        return {k: (lambda m=m: (fl & m) != 0) for k, m in self.FLAG_INFO}

    # -- checkpoints --------------------------------------------------------------------------
    def _check_checkpoint(self, state):
        """-> the arrays of `state` (its "__...__" keys dropped), once the checkpoint is known to fit this batch: taken with the
        same scenario assignment, every array known and of this batch's size."""
        host = self.engine.host
        if np.asarray(state["__seeds__"]).tolist() != list(host.seeds):
            raise ValueError("the checkpoint was taken with another scenario assignment ({} / num_scenarios / env_seed_offset "
                             "differ): {} and routes would not match".format(*self.ASSIGNMENT))
        arrays = {k: v for k, v in state.items() if not k.startswith("__")}
        for k, v in arrays.items():
            if k not in host.state or np.asarray(v).nbytes != host.state[k].nbytes:
                raise ValueError("checkpoint array {!r} does not fit this batch".format(k))
        return arrays


class ObjectSpawnMixin:
    """Traffic participants spawned by the user (engine.spawn_object(Pedestrian, ...) of the reference).  In a multi-agent env
    this needs mover_capacity > num_agents: the agents' slots are never handed out."""
    def spawn_object(self, kind, position, heading_theta=0.0, envs=None):
        """kind "pedestrian" | "cyclist" at `position` (one [x, y] or one per chosen env) -> handle.  It is hit by
        lidar beams, crashing into it sets crash_human, it moves with the velocity given by set_velocity and it is
        gone when its env resets."""
        return self.engine.spawn_object(kind, position, heading_theta, envs)

    def set_velocity(self, handle, direction, value=None, in_local_frame=False, envs=None):
        self.engine.set_velocity(handle, direction, value, in_local_frame, envs)

    def clear_objects(self, handles, envs=None):
        self.engine.clear_objects(list(handles), envs)
