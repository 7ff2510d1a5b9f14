/*
 * md_contact_response.h -- contact response of the kinematic engine (config contact_response; BatchedEngine launches
 * md_contact_response before md_ped and md_step).  No reference counterpart: the reference resolves contacts inside Bullet
 * (impulses, friction, chassis rotation), which cannot be restated, and trajectories against Bullet are unpinned by construction
 * (DESIGN.md section 5).  This is a small deterministic rule instead: a driving vehicle that overlaps another body is pushed out
 * of it and loses the part of its speed that closes on it.  The heading never changes, nothing but vehicles is ever moved, and
 * static map bodies (sidewalk strips, guardrails, lane lines) take no part.  Shared by the kernel (csrc/parts/
 * contact_response.inc: contact_response_kernel) and the host restatement of the tests (tests/contact_response_host.c): float32,
 * only + - * /, comparisons and md_sqrt / md_norm / md_fabs of md_math.h, no libm, so that a gcc -ffp-contract=off build
 * reproduces the device bit for bit.  The rule keeps no state: MdState / MdConfig / MdWorld stay as they are.
 *
 * The rule, once per env and step, BEFORE md_step (and before md_ped), on the state the previous step left; an env whose
 * need_reset is set is skipped, its rows are about to be replaced by the snapshot.
 *
 *   responders   slots i with md_drives(flags_i): agents and driving traffic
 *   obstacles    every other slot j != i with md_present(flags_j): props, pending / static / replayed vehicles, buildings,
 *                walkers, other driving vehicles.  Weight w = 0.5 if the obstacle drives too (an equal-mass pair: each is the
 *                other's obstacle), w = 1 otherwise (the obstacle is immovable and is never written)
 *   velocity     of the obstacle: speed_j (c_j, s_j) if it drives, (dyn_j.steering, dyn_j.throttle) if md_walks, else 0
 *
 * Every read is of the ENTRY state of the env: no responder sees another responder's update.
 *
 * Contact of a pair, evaluated canonically for (lo, hi) = (min(i, j), max(i, j)) so that both members of a vehicle pair get the
 * same depth bits and opposite normals:
 *   box vs box     the four axes of md_obb_obb in its order (A.u, A.v, B.u, B.v; A = lo) with its exact limit expressions;
 *                  overlap_k = limit_k - |t . axis_k|, t = centre(hi) - centre(lo); a hit iff no axis separates (exactly when
 *                  md_obb_obb returns 1 on the same floats); depth = the smallest overlap, the first one on ties; the normal
 *                  that moves lo away is -sgn(t . axis_k) axis_k with sgn(0) = +1
 *   box vs circle  (md_is_circle_kind; the circle is always the obstacle) a hit iff md_obb_circle says so.  Centre outside the
 *                  box: the normal runs along centre minus closest point, depth = r - dist (md_sqrt).  Centre inside: the
 *                  nearer face (u on ties), depth = r + the distance to it.
 *
 * A responder's contacts are folded in ASCENDING obstacle slot order (md_cr_fold):
 *       push += w (depth + skin) n
 *       hn = (c_i, s_i) . n
 *       closing = speed hn - v_j . n           speed: the value folded so far
 *       if closing < 0: speed -= w closing hn
 * then a push longer than max_push is scaled to max_push, cx += push.x, cy += push.y, dyn.speed = speed.  Nothing else is
 * written: not the heading, not last_*, not MdNav or MdPid, no other slot; a responder without a hit is not written at all.
 * So a head-on hit on a barrier ends at speed 0, a 45 degree scrape keeps half the speed and slides, a rear-end hit at 10 on
 * 4 m/s leaves both at 7, and two cones hit at once stop the car instead of reversing it (the fold is sequential for that).
 *
 * Before the step and not after it: md_integrate_mover takes last_x, last_y from the pose it starts with, so the step's
 * distance, energy and velocity direction never contain the push; the observation md_step writes belongs to the pose it wrote;
 * an env that is about to reset is simply skipped.
 *
 * skin and max_push are design choices with no reference counterpart.
 */
#ifndef MD_CONTACT_RESPONSE_H
#define MD_CONTACT_RESPONSE_H

#include "md_entity.h"

/* md_contact_response's argument block (config contact_response_config) */
typedef struct MdContactResponse {
    int32_t struct_size;   /* sizeof(MdContactResponse) as the caller sees it */
    float skin;            /* 0.01 m: the gap a resolved pair is left with, so that the next step's contact test is clear */
    float max_push;        /* 0.5 m: the longest displacement of a vehicle in one step */
    int32_t reserved;      /* 0 */
} MdContactResponse;

/* one contact as the responder sees it: (nx, ny) moves the responder out of the obstacle */
typedef struct MdCrHit {
    int hit;
    float depth, nx, ny;
} MdCrHit;

/* what a responder's contacts fold into */
typedef struct MdCrAcc {
    float px, py, speed;
} MdCrAcc;

/* Box A vs box B with the axes, limits and order of md_obb_obb: hit, depth and the normal that moves A away from B. */
MD_HD MdCrHit md_cr_box_box(const MdShape* A, const MdShape* B) {
    MdCrHit h;
    h.hit = 0;
    h.depth = h.nx = h.ny = 0.0f;
    const float ac = A->c, as = A->s, bc = B->c, bs = B->s;
    const float tx = B->cx - A->cx, ty = B->cy - A->cy;
    const float cc = md_fabs(ac * bc + as * bs);
    const float cs = md_fabs(ac * bs - as * bc);
    const float d0 = tx * ac + ty * as, l0 = A->hl + B->hl * cc + B->hw * cs;
    if (md_fabs(d0) > l0) return h;
    const float d1 = ty * ac - tx * as, l1 = A->hw + B->hl * cs + B->hw * cc;
    if (md_fabs(d1) > l1) return h;
    const float d2 = tx * bc + ty * bs, l2 = B->hl + A->hl * cc + A->hw * cs;
    if (md_fabs(d2) > l2) return h;
    const float d3 = ty * bc - tx * bs, l3 = B->hw + A->hl * cs + A->hw * cc;
    if (md_fabs(d3) > l3) return h;
    h.hit = 1;
    const float o0 = l0 - md_fabs(d0), o1 = l1 - md_fabs(d1), o2 = l2 - md_fabs(d2), o3 = l3 - md_fabs(d3);
    float depth = o0, d = d0, ax = ac, ay = as;            /* A.u */
    if (o1 < depth) { depth = o1; d = d1; ax = -as; ay = ac; }   /* A.v */
    if (o2 < depth) { depth = o2; d = d2; ax = bc; ay = bs; }    /* B.u */
    if (o3 < depth) { depth = o3; d = d3; ax = -bs; ay = bc; }   /* B.v */
    h.depth = depth;
    h.nx = d < 0.0f ? ax : -ax;
    h.ny = d < 0.0f ? ay : -ay;
    return h;
}

/* Box A vs the circle (bx, by, r): hit as md_obb_circle, depth and the normal that moves A away from the circle. */
MD_HD MdCrHit md_cr_box_circle(const MdShape* A, float bx, float by, float r) {
    MdCrHit h;
    h.hit = 0;
    h.depth = h.nx = h.ny = 0.0f;
    const float ac = A->c, as = A->s;
    const float tx = bx - A->cx, ty = by - A->cy;
    const float u = tx * ac + ty * as, v = ty * ac - tx * as;
    float lx = md_fabs(u) - A->hl, ly = md_fabs(v) - A->hw;
    const float fu = -lx, fv = -ly;     /* distances to the faces, read where the centre is inside */
    if (lx < 0.0f) lx = 0.0f;
    if (ly < 0.0f) ly = 0.0f;
    const float d2 = lx * lx + ly * ly;
    if (!(d2 <= r * r)) return h;
    h.hit = 1;
    const float su = u < 0.0f ? -1.0f : 1.0f, sv = v < 0.0f ? -1.0f : 1.0f;
    float mu, mv;                       /* the normal in A's frame */
    if (lx > 0.0f || ly > 0.0f) {       /* centre outside: away from (centre - closest point) */
        const float dist = md_sqrt(d2);
        h.depth = r - dist;
        mu = -(su * lx) / dist;
        mv = -(sv * ly) / dist;
    } else if (fu <= fv) {              /* centre inside, the front / rear face is the nearer one */
        h.depth = r + fu;
        mu = -su;
        mv = 0.0f;
    } else {
        h.depth = r + fv;
        mu = 0.0f;
        mv = -sv;
    }
    h.nx = mu * ac - mv * as;
    h.ny = mu * as + mv * ac;
    return h;
}

/* What an obstacle can reach from its centre, generously: hl + hw >= the box's circumradius, 2 r >= r */
MD_HD float md_cr_reach(const MdShape* J) {
    return md_is_circle_kind(md_kind_of(J->flags)) ? J->hl + J->hl : J->hl + J->hw;
}

/* Conservative centre-distance cull in front of md_cr_contact: 0 only where the pair cannot hit.  A hit has |t . axis| <= limit
 * on both axes of one body in float32; with the bodies' reaches R = md_cr_reach the limits are at most R_i + R_j (1 + 1e-6)
 * (|c|, |s| <= 1 + 1e-7 from md_sincos, a few roundings), so |t|^2 <= 2 (R_i + R_j)^2 (1 + 1e-5): the bound below, 2.1 (R_i +
 * R_j)^2 + 1e-6, lies above that by 5 %, ten thousand times what the roundings of the two sides can add up to.  t is the same
 * difference of centres the tests form, up to its sign. */
MD_HD int md_cr_near(const MdShape* I, const MdShape* J) {
    const float tx = J->cx - I->cx, ty = J->cy - I->cy;
    const float R = md_cr_reach(I) + md_cr_reach(J);
    return !(tx * tx + ty * ty > 2.1f * (R * R) + 1.0e-6f);
}

/* The contact of responder slot i (a box: md_drives) with obstacle slot j != i, as the responder sees it */
MD_HD MdCrHit md_cr_contact(const MdShape* I, int i, const MdShape* J, int j) {
    if (md_is_circle_kind(md_kind_of(J->flags))) return md_cr_box_circle(I, J->cx, J->cy, J->hl);
    if (i < j) return md_cr_box_box(I, J);
    MdCrHit h = md_cr_box_box(J, I);    /* the normal that moves lo = j away: the responder gets the opposite one */
    h.nx = -h.nx;
    h.ny = -h.ny;
    return h;
}

/* obstacle j's weight and velocity */
MD_HD float md_cr_weight(int flags) { return md_drives(flags) ? 0.5f : 1.0f; }
MD_HD void md_cr_velocity(const MdShape* J, float speed, float wvx, float wvy, float* vx, float* vy) {
    *vx = *vy = 0.0f;
    if (md_drives(J->flags)) {
        *vx = speed * J->c;
        *vy = speed * J->s;
    } else if (md_walks(J->flags)) {
        *vx = wvx;
        *vy = wvy;
    }
}

/* one contact folded into the responder's push and speed; (hc, hs) the responder's heading */
MD_HD void md_cr_fold(MdCrAcc* a, float depth, float nx, float ny, float w, float vx, float vy, float hc, float hs, float skin) {
    const float m = w * (depth + skin);
    a->px = a->px + m * nx;
    a->py = a->py + m * ny;
    const float hn = hc * nx + hs * ny;
    const float closing = a->speed * hn - (vx * nx + vy * ny);
    if (closing < 0.0f) a->speed = a->speed - (w * closing) * hn;
}

/* after the fold: the push no longer than max_push */
MD_HD void md_cr_clamp(MdCrAcc* a, float max_push) {
    const float len = md_norm(a->px, a->py);
    if (len > max_push) {
        const float k = max_push / len;
        a->px = a->px * k;
        a->py = a->py * k;
    }
}

/* md_contact_response for one env (view `s`) as plain loops: what the kernel computes with a wave per env.  The results are
 * kept aside until every responder has read the entry state.  `e` names the env for the caller; the view is env-local already. */
MD_HD void md_contact_response_env(const MdState* s, const MdConfig* c, const MdContactResponse* cr, int e) {
    (void)e;
    if (s->need_reset[0] != 0) return;   /* its rows are about to be replaced by the snapshot */
    float out_x[MD_MAX_CAP], out_y[MD_MAX_CAP], out_v[MD_MAX_CAP];
    int had[MD_MAX_CAP];
    for (int i = 0; i < c->cap; ++i) {
        had[i] = 0;
        const MdShape* I = &s->shape[i];
        if (!md_drives(I->flags)) continue;
        MdCrAcc a;
        a.px = a.py = 0.0f;
        a.speed = s->dyn[i].speed;
        for (int j = 0; j < c->cap; ++j) {
            const MdShape* J = &s->shape[j];
            if (j == i || !md_present(J->flags)) continue;
            const MdCrHit h = md_cr_contact(I, i, J, j);
            if (!h.hit) continue;
            float vx, vy;
            md_cr_velocity(J, s->dyn[j].speed, s->dyn[j].steering, s->dyn[j].throttle, &vx, &vy);
            md_cr_fold(&a, h.depth, h.nx, h.ny, md_cr_weight(J->flags), vx, vy, I->c, I->s, cr->skin);
            had[i] = 1;
        }
        if (!had[i]) continue;
        md_cr_clamp(&a, cr->max_push);
        out_x[i] = I->cx + a.px;
        out_y[i] = I->cy + a.py;
        out_v[i] = a.speed;
    }
    for (int i = 0; i < c->cap; ++i)
        if (had[i]) {
            s->shape[i].cx = out_x[i];
            s->shape[i].cy = out_y[i];
            s->dyn[i].speed = out_v[i];
        }
}

#ifdef __cplusplus
extern "C" {
#endif

/* The rule above for every env whose need_reset is 0: ONE launch, one wave per env, asynchronous on `stream`; call it before
 * md_ped and md_step, on the same stream.  With no contact in the batch it writes nothing.  Requires s->shape, dyn, need_reset;
 * reads c->n_envs, cap, traffic_mode (4, scenario mode, is refused: replayed and trajectory-bound vehicles take their poses from
 * data); cr->skin >= 0, cr->max_push > 0. */
int md_contact_response(const MdState* s, const MdConfig* c, const MdContactResponse* cr, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MD_CONTACT_RESPONSE_H */
