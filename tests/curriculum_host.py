"""ctypes binding of tests/curriculum_host.c (the curriculum of include/md_curriculum.h, compiled on first use into a temporary
directory) and the host model of md_curriculum on an oracle: CurriculumOracle steps the walk's oracle and runs the same state
machine after every step, moving the envs itself when there is more than one level.  TEST INFRASTRUCTURE."""
import ctypes as C

import numpy as np

import hostlib
import walk_host as wh
from metadrive_ped_amd.scenario import curriculum_state as new_state      # noqa: F401  (the per-env arrays cur_* of a batch before its first reset)

FIELDS = ("level", "seed", "q_len", "q_key", "q_success", "q_route", "cover", "cover_n", "rep_i", "rep_f")


def _declare(L):
    P = C.c_void_p
    L.hx_cur_after_step.argtypes = [P, P, C.c_double, C.c_int, C.c_int, C.c_float, C.c_int, C.c_int]
    L.hx_cur_restart.argtypes = [P, P, C.c_double, C.c_int, C.c_int]
    L.hx_cur_next.argtypes = [P, C.c_int, P, C.c_int, C.c_int, P]


def lib():
    return hostlib.build("curriculum_host", _declare)


class Curriculum:
    """md_curriculum's state machine on the arrays `st` (keys cur_*, modified in place)"""
    def __init__(self, st, n_levels, per_level, eval_, n_scenes, stride, offset, target):
        self.st = st
        for f in FIELDS:
            assert st["cur_" + f].flags.c_contiguous
        self.k = np.asarray([n_levels, per_level, eval_, n_scenes, stride, offset], np.int32)
        self.target = float(target)

    def _ptrs(self):
        return (C.c_void_p * 10)(*[self.st["cur_" + f].ctypes.data for f in FIELDS])

    def after_step(self, e, success, route, ended, follow=-1):
        return lib().hx_cur_after_step(self._ptrs(), self.k.ctypes.data, self.target, int(e), int(success), float(route),
                                       int(ended), int(follow))

    def restart(self, e, follow=-1):
        return lib().hx_cur_restart(self._ptrs(), self.k.ctypes.data, self.target, int(e), int(follow))

    def report(self, e):
        """(level, scene, success, route completion, coverage) of env e's last step"""
        ri, rf = self.st["cur_rep_i"][e], self.st["cur_rep_f"][e]
        return int(ri[0]), int(ri[1]), float(rf[0]), float(rf[1]), float(rf[2])


def next_seeds(n_levels, per_level, n_scenes, stride, w, cur, level):
    cur = np.ascontiguousarray(cur, np.int32)
    out = np.zeros_like(cur)
    k = np.asarray([n_levels, per_level, 1, n_scenes, stride, 0], np.int32)
    lib().hx_cur_next(k.ctypes.data, int(w), cur.ctypes.data, int(level), cur.size, out.ctypes.data)
    return out


def host_curriculum(host, st):
    L, per, Q, target = host.curriculum
    n, _, W, off, _ = host.walk_params
    return Curriculum(st, L, per, Q, n, W, off, target)


class CurriculumOracle(wh.WalkOracle):
    """The walk's oracle with the host model of md_curriculum after every step, in the engine's launch order: one level,
    md_swap_draw's move then the curriculum following it; more levels, the curriculum's own move (scene_of, walk_ep, env_map and
    the snapshot rows from the pool)."""
    def __init__(self, host, state=None):
        super().__init__(host, state)
        self.cur = host_curriculum(host, self.state)
        self.levels = host.curriculum[0]

    def _move(self, e, p, reset):
        h, st, cap = self.host, self.state, self.host.cap
        st["walk_ep"][e] = 0 if reset else st["walk_ep"][e] + 1
        st["scene_of"][e], self.env_map[e] = p, p
        for k in self.ROWS:
            st[k][e * cap:(e + 1) * cap] = h.pool[k][p * cap:(p + 1) * cap]

    def _after_step(self):
        st = self.state
        if self.levels == 1:
            self.swap()
        for e in range(self.host.E):
            follow = int(st["scene_of"][e]) if self.levels == 1 else -1
            p = self.cur.after_step(e, (int(st["flags"][e * self.host.cap]) & wh.abi.FL_ARRIVE_DEST) != 0, st["step_info"][e][6],
                                    st["need_reset"][e] != 0, follow)
            if p >= 0 and self.levels > 1:
                self._move(e, p, False)

    def step(self, actions=None, threads=1):
        wh.ob.OracleWorld.step(self, actions, threads)
        self._after_step()

    def reset(self):
        st = self.state
        st["walk_ep"][:] = -1
        st["need_reset"][:] = 1
        if self.levels == 1:
            self.swap()
        for e in range(self.host.E):
            p = self.cur.restart(e, int(st["scene_of"][e]) if self.levels == 1 else -1)
            if self.levels > 1:
                self._move(e, p, True)
        wh.ob.OracleWorld.reset(self)
        self._after_step()
