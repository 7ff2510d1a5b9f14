/*
 * md_ped.h -- crossing pedestrians driven on the device (config num_pedestrians; metadrive_ped_amd/scene.py places them,
 * BatchedEngine launches md_ped before every md_step).  No reference counterpart: the reference's pedestrians move with the
 * constant velocity the user set (tests/test_functionality/test_pedestrian.py); here a walker crosses its road back and forth,
 * waits at the kerb for a gap in the traffic and stops for a vehicle bearing down on it.  Shared by the kernel (csrc/parts/ped.inc:
 * ped_kernel) and the host restatement of the tests (tests/ped_host.c): float32, only + - * /, md_sqrt / md_norm / md_sincos of
 * md_math.h, no libm, so that a gcc -ffp-contract=off build reproduces the device bit for bit.
 *
 * A policy-driven pedestrian is a mover of kind MD_KIND_PEDESTRIAN whose OWN rows carry its policy data; no per-env array is
 * added and MdState / MdConfig / MdWorld stay as they are.  No stage of any md_step variant reads or writes the MdPid row or
 * the integer fields of the MdNav row of a slot that is no vehicle (the IDM, the localiser, the traffic stages and the observe
 * stage all ask md_drives / MD_F_AGENT first; the write-back stores a walker's staged rows as they were loaded), and the slot's
 * idm_rand row is read by IDMPolicy vehicles only.  The assignment:
 *
 *   MdPid.hp, hi          A: the crossing's first end point, world coordinates
 *   MdPid.hd, lp          B: its second end point
 *   MdPid.li              walking speed, m/s
 *   MdPid.ld              heading of A -> B, radians
 *   MdPid.target_speed    heading of B -> A, radians
 *   MdNav.toll_state      phase: MD_PED_OFF (0: not policy-driven -- what the untouched row of a user-spawned participant
 *                         holds; md_ped leaves it alone), MD_PED_WAIT_A, MD_PED_CROSS_AB, MD_PED_WAIT_B, MD_PED_CROSS_BA
 *   MdNav.timer           wait countdown, steps
 *   MdNav.rand_cursor     cursor into the slot's idm_rand row (the wait draws, consumed cyclically)
 *
 * The snapshot rows shape0 / dyn0 / nav0 / pid0 hold the same, so the env's own reset inside md_step starts an episode's
 * pedestrians over; md_swap_draw and md_curriculum swap whole slot ranges of those rows and of idm_rand, and md_branch copies
 * them: the PG walk, random_traffic and env snapshots carry the pedestrians with no code of their own.
 *
 * The rule, once per pedestrian and step, BEFORE md_step, on the state the previous step left.  u = (B - A) / |B - A|,
 * L = |B - A|, n = perp(u); the pedestrian stands at along = (p - A).u.  A vehicle j counts if md_drives(flags); for it
 * a_j = (c_j - A).u, lon_j = (c_j - A).n, vlon_j = speed_j * ((cos_j, sin_j).n).  It OCCUPIES the strip if |lon_j| <= hl_j +
 * clear_dist and ARRIVES WITHIN t if lon_j * vlon_j < 0 and (|lon_j| - hl_j) / |vlon_j| < t.
 *   waiting   velocity 0; the countdown decrements; once it is 0 and no counting vehicle with -margin <= a_j <= L + margin
 *             occupies the strip or arrives within L / speed + time_margin the pedestrian starts to cross (in this step);
 *   crossing  heading along the walk; velocity 0 if a vehicle lies ahead within yield_ahead metres of `along` in walking
 *             direction and occupies the strip or arrives within yield_time; else speed * (+-u), on the last step remaining /
 *             step_dt so that the walker lands on the end point.  Arrival is remaining <= 1e-3 m: the phase becomes the wait
 *             at that end with countdown wait_min_steps + idm_rand[cursor++ mod MD_IDM_RAND].
 * The velocity goes into MdDyn.steering / throttle / speed, where md_walk_mover (md_entity.h) reads it.  A pedestrian's verdicts
 * depend on the vehicles only, never on other pedestrians, so the order of the pedestrians does not matter.
 */
#ifndef MD_PED_H
#define MD_PED_H

#include "md_entity.h"

#define MD_PED_OFF 0
#define MD_PED_WAIT_A 1
#define MD_PED_CROSS_AB 2
#define MD_PED_WAIT_B 3
#define MD_PED_CROSS_BA 4

#define MD_PED_HOLD 1    /* a vehicle keeps the waiting pedestrian at the kerb */
#define MD_PED_YIELD 2   /* a vehicle stops the crossing pedestrian */
#define MD_PED_ARRIVE_EPS 1.0e-3f

/* md_ped's argument block: the constants of the rule that are the same for every pedestrian (config pedestrian_config; a
 * design choice with no reference counterpart) */
typedef struct MdPed {
    int32_t struct_size;     /* sizeof(MdPed) as the caller sees it */
    int32_t wait_min_steps;  /* 10 */
    float clear_dist;        /* 1.0 m */
    float margin;            /* 1.0 m */
    float time_margin;       /* 1.0 s */
    float yield_ahead;       /* 3.0 m */
    float yield_time;        /* 1.5 s */
    int32_t reserved;        /* 0 */
} MdPed;

/* one pedestrian's crossing as the vehicle tests read it */
typedef struct MdPedGeom {
    float ax, ay;     /* A */
    float ux, uy;     /* unit vector A -> B */
    float L;          /* |B - A| */
    float along;      /* (p - A).u */
    float dir;        /* +1 walking (or about to walk) A -> B, -1 B -> A */
    float t_cross;    /* L / speed + time_margin */
} MdPedGeom;

/* policy-driven: an alive, non-static pedestrian whose phase is set */
MD_HD int md_ped_driven(int flags, const MdNav* nav) {
    return md_walks(flags) && md_kind_of(flags) == MD_KIND_PEDESTRIAN && nav->toll_state != MD_PED_OFF;
}

MD_HD MdPedGeom md_ped_geom(const MdShape* sh, const MdNav* nav, const MdPid* pid, const MdPed* p) {
    MdPedGeom g;
    const float dx = pid->hd - pid->hp, dy = pid->lp - pid->hi;
    g.ax = pid->hp;
    g.ay = pid->hi;
    g.L = md_norm(dx, dy);
    g.ux = dx / g.L;
    g.uy = dy / g.L;
    g.along = (sh->cx - g.ax) * g.ux + (sh->cy - g.ay) * g.uy;
    g.dir = nav->toll_state <= MD_PED_CROSS_AB ? 1.0f : -1.0f;
    g.t_cross = g.L / pid->li + p->time_margin;
    return g;
}

MD_HD int md_ped_arrives_within(float lon, float vlon, float hl, float t) {
    return lon * vlon < 0.0f && (md_fabs(lon) - hl) / md_fabs(vlon) < t;
}

/* what the vehicle `v` with forward speed `speed` means to the pedestrian of `g`: MD_PED_HOLD | MD_PED_YIELD bits */
MD_HD int md_ped_vehicle(const MdPedGeom* g, const MdPed* p, const MdShape* v, float speed) {
    if (!md_drives(v->flags)) return 0;
    const float rx = v->cx - g->ax, ry = v->cy - g->ay;
    const float nx = -g->uy, ny = g->ux;
    const float a = rx * g->ux + ry * g->uy;
    const float lon = rx * nx + ry * ny;
    const float vlon = speed * (v->c * nx + v->s * ny);
    const int occupies = md_fabs(lon) <= v->hl + p->clear_dist;
    int bits = 0;
    if (a >= -p->margin && a <= g->L + p->margin && (occupies || md_ped_arrives_within(lon, vlon, v->hl, g->t_cross))) bits |= MD_PED_HOLD;
    const float ahead = (a - g->along) * g->dir;
    if (ahead >= 0.0f && ahead <= p->yield_ahead && (occupies || md_ped_arrives_within(lon, vlon, v->hl, p->yield_time))) bits |= MD_PED_YIELD;
    return bits;
}

/* The scalar part of the rule for the pedestrian in slot j of the env view `s`, given the OR of md_ped_vehicle over the env's
 * slots: phase, countdown, cursor, heading and velocity. */
MD_HD void md_ped_apply(const MdState* s, const MdConfig* c, const MdPed* p, int j, const MdPedGeom* g, int bits) {
    MdShape* sh = &s->shape[j];
    MdDyn* d = &s->dyn[j];
    MdNav* nav = &s->nav[j];
    const MdPid* pid = &s->pid[j];
    float v = 0.0f;
    if (nav->toll_state == MD_PED_WAIT_A || nav->toll_state == MD_PED_WAIT_B) {
        if (nav->timer > 0) nav->timer -= 1;
        if (nav->timer == 0 && !(bits & MD_PED_HOLD)) nav->toll_state += 1;
    }
    if (nav->toll_state == MD_PED_CROSS_AB || nav->toll_state == MD_PED_CROSS_BA) {
        const float step_dt = c->dt * (float)c->substeps;
        const float remaining = g->dir > 0.0f ? g->L - g->along : g->along;
        if (remaining <= MD_PED_ARRIVE_EPS) {
            nav->toll_state = nav->toll_state == MD_PED_CROSS_AB ? MD_PED_WAIT_B : MD_PED_WAIT_A;
            const int cur = nav->rand_cursor;
            nav->timer = p->wait_min_steps + s->idm_rand[(size_t)j * MD_IDM_RAND + (size_t)(cur & (MD_IDM_RAND - 1))];
            nav->rand_cursor = cur + 1;
        } else {
            d->heading = g->dir > 0.0f ? pid->ld : pid->target_speed;
            md_sincos(d->heading, &sh->s, &sh->c);
            if (!(bits & MD_PED_YIELD)) v = remaining <= pid->li * step_dt ? remaining / step_dt : pid->li;
        }
    }
    d->steering = v * g->dir * g->ux;
    d->throttle = v * g->dir * g->uy;
    d->speed = v;
}

/* md_ped for one env (view `s`) as a plain loop: what the kernel computes with a wave per env */
MD_HD void md_ped_env(const MdState* s, const MdConfig* c, const MdPed* p) {
    if (s->need_reset[0] != 0) return;   /* its rows are about to be replaced by the snapshot */
    for (int j = 0; j < c->cap; ++j) {
        if (!md_ped_driven(s->shape[j].flags, &s->nav[j])) continue;
        const MdPedGeom g = md_ped_geom(&s->shape[j], &s->nav[j], &s->pid[j], p);
        int bits = 0;
        for (int k = 0; k < c->cap; ++k) bits |= md_ped_vehicle(&g, p, &s->shape[k], s->dyn[k].speed);
        md_ped_apply(s, c, p, j, &g, bits);
    }
}

#ifdef __cplusplus
extern "C" {
#endif

/* The rule above for every policy-driven pedestrian of every env whose need_reset is 0: ONE launch, one wave per env,
 * asynchronous on `stream`; call it before md_step, on the same stream.  Requires s->shape, dyn, nav, pid, idm_rand,
 * need_reset; reads c->n_envs, cap, dt, substeps. */
int md_ped(const MdState* s, const MdConfig* c, const MdPed* p, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MD_PED_H */
