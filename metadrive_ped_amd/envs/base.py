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

    # -- the vector scene observation (include/md_vector_obs.h) ---------------------------------
    def _vector_obs_config(self, what):
        vo = self.config.get("vector_obs")
        if vo is None:
            raise RuntimeError("{}(): config['vector_obs'] is None; give it a dict ({{}} takes the defaults) to turn the vector "
                               "scene observation on".format(what))
        return vo

    def vector_obs_spec(self):
        """{name: (shape, numpy dtype)} of vector_obs()'s tensors: [E, A, ...] in a multi-agent env, [E, ...] in a single-agent one"""
        from metadrive_ped_amd import abi as _abi
        vo = self._vector_obs_config("vector_obs_spec")
        multi = bool(self.config["is_multi_agent"])
        outs = _abi.vector_obs_blocks(vo, int(self.config["num_agents"]) if multi else 1, 1)[0]
        return {name: ((self.num_envs, ) + (tuple(shape) if multi else tuple(shape[1:])), dt.type) for name, (_, shape, dt) in outs.items()}

    def vector_obs(self):
        """The vector scene observation of the state the last step() / reset() left, a dict of device tensors in the observer's ego
        frame, metres: agents [.., K, T, 4] (x, y, cos, sin per frame, frame 0 = now), agents_mask, agents_meta [.., K, 4] (length,
        width, speed, kind), ego [.., T, 4], ego_mask, route [.., M, 4], route_mask, lanes [.., P, S, 2], lanes_meta [.., P, 4]
        (width, length, on_route, distance), lanes_mask.  Views of the engine's buffers, valid until the next step() / reset();
        no host sync.  Leading axes [E, A] in a multi-agent env, [E] in a single-agent one."""
        self._vector_obs_config("vector_obs")
        self._require_engine("vector_obs")
        out = self.engine.vector_obs_out
        return dict(out) if self.config["is_multi_agent"] else {k: t[:, 0] for k, t in out.items()}

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

    # -- device-side snapshots (metadrive_ped_amd/branch.py, include/md_branch.h) ---------------
    def _branch_plan(self):
        """(batch signature, {MdState field: bytes per env}, the engine's extras) of the batch as it is now"""
        from metadrive_ped_amd import branch
        e, c = self.engine, self.config
        key = (e._branch_token, len(e.state_dev), e.protect_flags is None)
        if getattr(self, "_branch_cache", (None, ))[0] != key:
            fields, extras = e.branch_fields(), e.branch_extras()
            td = None
            if e.topdown_dev is not None:
                td = tuple(int(c[k]) for k in ("resolution_size", "frame_stack", "frame_skip", "post_stack", "norm_pixel"))
            family = "marl:{}".format(c["marl_map"]) if c["is_multi_agent"] else "pg"
            sig = branch.batch_signature(family, e.cap, e.A, e.obs_dim, td, tuple(fields) + tuple(n for n, _, _ in extras))
            self._branch_cache = (key, sig, fields, extras)
        return self._branch_cache[1:]

    def _checked_pairs(self, what, a, b, check, keep=None):
        """check() -> the checked (a, b) index arrays, remembered under the arguments' cheap names (branch.pair_key) for the
        latest few calls.  `keep`: an object the memo entry belongs to (a snapshot, named by id in `what`): held weakly, and the
        entry is only used while it is that very object."""
        import weakref
        from metadrive_ped_amd import branch
        ka, kb = branch.pair_key(a), branch.pair_key(b)
        if ka is None or kb is None:
            return check()
        memo = self.__dict__.setdefault("_pair_memo", {})
        key = what + (ka, kb, self.num_envs)
        hit = memo.get(key)
        if hit is not None and (hit[1] is None or hit[1]() is keep):
            return hit[0]
        out = check()
        if len(memo) >= 8:
            memo.pop(next(iter(memo)))
        memo[key] = (out, None if keep is None else weakref.ref(keep))
        return out

    def _seeds_np(self):
        """The host scene's seed list as an int64 array, kept beside it (the list is only ever rewritten here and by a build)"""
        seeds = self.engine.host.seeds
        m = getattr(self, "_seeds_mirror", None)
        if m is None or m[0] is not seeds:
            m = self._seeds_mirror = (seeds, np.asarray(seeds, dtype=np.int64))
        return m[1]

    def _seeds_moved(self, seeds, dst):
        """The scenario seeds follow the rows: env dst[i] now plays seeds[i].  Host-side, from the host-side indices: no sync."""
        arr = self._seeds_np()
        if np.array_equal(arr[dst], seeds):      # the usual case of a rollout loop: nothing to rewrite
            return
        arr[dst] = seeds
        self.engine.host.seeds[:] = arr.tolist()
        self._seed_cache = (None, None)

    def snapshot(self, envs=None):
        """-> EnvSnapshot: a device-resident copy of the envs `envs` (host integers; None: all), made by ONE md_branch launch on
        torch's current stream, no host sync.  It holds everything that makes an env's next step() bit-identical: every per-env
        row of every state array (live, reset snapshot rows, step outputs, RNG), the env's map, the top-down history and image,
        the AIProtect takeover bytes and the scenario seed.  It does NOT hold the lidar-noise and expert-noise generators (one
        stream per batch), the viewer's render history or a recording buffer.  Valid across step() and a plain reset(); not
        across reset(seed=...), a rebuild of the engine or close()."""
        from metadrive_ped_amd import abi as _abi, branch
        branch.check_scope(self.config, "snapshot", self.engine)
        if envs is None:
            envs = np.arange(self.num_envs, dtype=np.int64)
        else:
            envs = branch.as_indices(envs, "envs")
            if envs.size == 0:
                raise ValueError("snapshot: envs names no env")
            branch.check_range(envs, self.num_envs, "snapshot: envs")
            branch.check_distinct(envs, self.num_envs, "snapshot: envs")
        self._require_engine("snapshot")
        e, n = self.engine, int(envs.size)
        sig, fields, extras = self._branch_plan()
        st_off, ex_off, total = branch.layout(fields, [(name, rb) for name, _, rb in extras], n)
        storage = e.torch.empty(total, dtype=e.torch.uint8, device=e.device)
        base = storage.data_ptr()
        s = _abi.MdState()
        for name, (off, _) in st_off.items():
            setattr(s, name, base + off)
        e.branch_rows(s, e.s, envs, np.arange(n, dtype=np.int64), e.E, n, [(base + ex_off[name][0], t.data_ptr(), rb) for name, t, rb in extras])
        return branch.EnvSnapshot(envs, self._seeds_np()[envs], sig, e._branch_token, storage, s,
                                  {name: (base + off, rb) for name, (off, rb) in ex_off.items()}, total, owner=e._branch_owner)

    def restore(self, snap, envs=None, rows=None):
        """Snapshot row rows[i] -> env envs[i], ONE md_branch launch on torch's current stream, no host sync.  Defaults: every row,
        to the env it came from; a one-row snapshot goes to every env named.  The envs' scenario seeds follow (current_seeds,
        info["env_seed"], get_state()["__seeds__"]), so a set_state() of a checkpoint from before is refused as another
        assignment.  What a snapshot does not hold (the noise generators, render history, recordings) is not touched.
        ValueError: an index out of range or an env named twice (names the env), a snapshot of another kind of batch, or one
        invalidated by reset(seed=...) / a rebuild / close()."""
        from metadrive_ped_amd import branch
        branch.check_scope(self.config, "restore", self.engine)
        if not isinstance(snap, branch.EnvSnapshot):
            raise TypeError("restore: expected an EnvSnapshot from env.snapshot(), got {!r}".format(type(snap).__name__))
        rows, envs = self._checked_pairs(("restore", id(snap)), rows, envs,
                                         lambda: branch.check_restore_pairs(snap, envs, rows, self.num_envs), keep=snap)
        branch.check_staged_draws(self.config, (snap._source[rows], envs), "restore")
        if self.engine is None:
            raise ValueError("restore: the snapshot is no longer valid: this env has no engine (close() came after it, or reset() "
                             "was never called)")
        e = self.engine
        sig, _, extras = self._branch_plan()
        branch.check_snapshot(snap, sig, e._branch_token, owner=e._branch_owner)
        e.branch_rows(e.s, snap._state, rows, envs, snap.num_envs, e.E, [(t.data_ptr(), snap._extras[name][0], rb) for name, t, rb in extras])
        self._seeds_moved(snap._seeds[rows], envs)

    def branch(self, src, dst):
        """Live env -> live env(s) in ONE md_branch launch on torch's current stream, no host sync: `src` one env or as many as
        `dst`.  Everything a snapshot holds travels (see snapshot()); reset() without a new seed keeps the branched assignment,
        since the reset snapshot rows travel too.  ValueError names an env that is out of range, twice in dst, or both a source
        and a destination (the pairs are copied concurrently)."""
        from metadrive_ped_amd import branch
        branch.check_scope(self.config, "branch", self.engine)
        src, dst = self._checked_pairs(("branch", ), src, dst, lambda: branch.check_branch_pairs(src, dst, self.num_envs))
        branch.check_staged_draws(self.config, (src, dst), "branch")
        self._require_engine("branch")
        e = self.engine
        _, _, extras = self._branch_plan()
        e.branch_rows(e.s, e.s, src, dst, e.E, e.E, [(t.data_ptr(), t.data_ptr(), rb) for _, t, rb in extras])
        self._seeds_moved(self._seeds_np()[src], dst)

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
        """On a policy-driven pedestrian (config num_pedestrians; its slot from pedestrian_state()) the velocity holds until the
        next step() at most: md_ped rewrites the walker's velocity at the start of every step."""
        self.engine.set_velocity(handle, direction, value, in_local_frame, envs)

    def clear_objects(self, handles, envs=None):
        """A policy-driven pedestrian cleared here is back when its env resets (its snapshot rows are untouched)."""
        self.engine.clear_objects(list(handles), envs)

    def pedestrian_state(self):
        """The crossing pedestrians of config num_pedestrians (include/md_ped.h) as device tensors: positions [E, P, 2], phase
        [E, P] (0 .. 4: abi.PED_*) and slot [E, P], padded with -1 where an env holds fewer than P.  No host sync."""
        return self.engine.pedestrian_state()
