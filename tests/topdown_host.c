/* Host build of include/md_topdown.h (the top-down observation), loaded by the tests through tests/hostlib.py.  Compiled with
 * gcc -O2 -ffp-contract=off: the rules are the header's, so the results are the md_topdown kernel's to the last bit.  Where the
 * kernel rasterises in primitive order into an LDS image, this walks the image in PIXEL order and tests every sample against every
 * primitive near the window (a world-space bounding box per primitive is the only cull). */
#include <stdlib.h>
#include <string.h>

#include "md_topdown.h"

#define EXPORT __attribute__((visibility("default")))

EXPORT int hx_sizeof_topdown(void) { return (int)sizeof(MdTopDown); }
EXPORT void hx_window(float px, float py, float hc, float hs, int R, float distance, float fr, float fc, float* xy) {
    md_td_window(px, py, hc, hs, R, md_td_metres_per_pixel(R, distance), fr, fc, &xy[0], &xy[1]);
}
EXPORT int hx_stack_indices(int length, int skip, int* out) {
    const int n = md_td_stack_count(length, skip);
    for (int i = 0; i < n; ++i) out[i] = md_td_stack_index(length, skip, i);
    return n;
}
EXPORT int hx_past_dot(float ox, float oy, float px, float py, float c, float s, int R, float distance, int* rc) {
    return md_td_past_dot(ox, oy, px, py, c, s, R, distance, &rc[0], &rc[1]);
}
EXPORT float hx_line_half_width(int R, float distance) { return md_td_line_half_width(md_td_metres_per_pixel(R, distance)); }
EXPORT float hx_road_float(int sum4) { return md_td_road_float(sum4); }
EXPORT int hx_road_byte(int sum4) { return md_td_road_byte(sum4); }
EXPORT float hx_traffic_float(void) { return md_td_traffic_float(); }
EXPORT int hx_traffic_byte(void) { return md_td_traffic_byte(); }

typedef struct Box { float x0, y0, x1, y1; int id; } Box;
static int in_box(const Box* b, float x, float y) { return x >= b->x0 && x <= b->x1 && y >= b->y0 && y <= b->y1; }

/* One md_topdown launch restated: every env of the batch on the state md_step left (global arrays, cap slots per env, one
 * agent); td's pointers are host arrays, advanced in place like the device's. */
EXPORT void hx_topdown(const MdWorld* w, const MdState* g, const MdConfig* c, const MdTopDown* td) {
    const int R = td->resolution, wpr = MD_TD_ROW_WORDS(R), FW = R * wpr, C = 2 + td->frame_stack;
    const int Lt = md_td_ring_len(td->frame_stack, td->frame_skip), Lp = md_td_ring_len(td->post_stack, td->frame_skip);
    const float m = md_td_metres_per_pixel(R, td->distance), hw = md_td_line_half_width(m);
    const float reach = td->distance * 1.5f + 4.0f * m + 1.0f;       /* beyond the window's circumscribed circle */
    uint32_t* traffic = (uint32_t*)malloc(sizeof(uint32_t) * (size_t)FW);
    uint32_t* past = (uint32_t*)malloc(sizeof(uint32_t) * (size_t)FW);
    int* sum4 = (int*)malloc(sizeof(int) * (size_t)R * R);
    for (int e = 0; e < c->n_envs; ++e) {
        const size_t b0 = (size_t)e * (size_t)c->cap;
        const MdShape* shape = g->shape + b0;
        const MdNav* nav0 = g->nav + b0;
        const int32_t* route = g->route_roads + b0 * MD_ROUTE_LEN;
        const int map = w->env_map[e];
        const MdLane* lanes = w->lanes + w->lane_off[map];
        const MdRoad* roads = w->roads + w->road_off[map];
        const float px = shape[0].cx, py = shape[0].cy, hc = shape[0].c, hs = shape[0].s;
        const int reset = md_td_is_reset(nav0);
        /* the primitives near the window */
        int n_lane = 0, n_quad = 0, n_mover = 0;
        const int qa = w->quad_off[map], qb = w->quad_off[map + 1];
        Box* lane_box = (Box*)malloc(sizeof(Box) * (size_t)(MD_ROUTE_LEN * 16 + 1));
        Box* quad_box = (Box*)malloc(sizeof(Box) * (size_t)(qb - qa + 1));
        Box mover_box[MD_MAX_CAP];
        for (int j = 0; j < nav0->route_len - 1 && j < MD_ROUTE_LEN; ++j) {
            if (route[j] < 0) continue;
            const MdRoad* rd = &roads[route[j]];
            for (int l = 0; l < rd->n_lanes && n_lane < MD_ROUTE_LEN * 16; ++l) {
                const MdLane* L = &lanes[rd->first_lane + l];
                /* MdLane.x0 .. y1 is the AABB of the lane's hull, built (mapgen/lanes.py) from a densely sampled outline with tangent
                 * extensions: chords of an arc miss it by centimetres, so 1.0 m is a wide margin.  The kernel culls on the same AABB
                 * with 1.5 m: should the hull ever be sampled coarsely, BOTH margins have to grow, or the two sides would miss the
                 * same part of an arc and still agree (the float64 restatement of tests/test_topdown.py culls nothing and knows arcs) */
                Box b = {L->x0 - 1.0f, L->y0 - 1.0f, L->x1 + 1.0f, L->y1 + 1.0f, rd->first_lane + l};
                if (b.x0 > px + reach || b.x1 < px - reach || b.y0 > py + reach || b.y1 < py - reach) continue;
                lane_box[n_lane++] = b;
            }
        }
        for (int q = qa; q < qb; ++q) {
            if (!md_td_is_line_kind(w->quad_kind[q])) continue;
            const float* v = w->quads + 8 * (size_t)q;
            Box b = {v[0], v[1], v[0], v[1], q};
            for (int i = 1; i < 4; ++i) {
                b.x0 = md_min(b.x0, v[2 * i]); b.x1 = md_max(b.x1, v[2 * i]);
                b.y0 = md_min(b.y0, v[2 * i + 1]); b.y1 = md_max(b.y1, v[2 * i + 1]);
            }
            b.x0 -= hw + 0.01f; b.y0 -= hw + 0.01f; b.x1 += hw + 0.01f; b.y1 += hw + 0.01f;
            if (b.x0 > px + reach || b.x1 < px - reach || b.y0 > py + reach || b.y1 < py - reach) continue;
            quad_box[n_quad++] = b;
        }
        for (int j = 0; j < c->cap; ++j) {
            if (!md_td_drawn(shape[j].flags, j)) continue;
            const float ext = md_fabs(shape[j].hl) + md_fabs(shape[j].hw) + 0.01f;
            Box b = {shape[j].cx - ext, shape[j].cy - ext, shape[j].cx + ext, shape[j].cy + ext, j};
            mover_box[n_mover++] = b;
        }
        memset(traffic, 0, sizeof(uint32_t) * (size_t)FW);
        memset(past, 0, sizeof(uint32_t) * (size_t)FW);
        for (int r = 0; r < R; ++r)
            for (int cc = 0; cc < R; ++cc) {
                int sum = 0;
                for (int k = 0; k < 4; ++k) {
                    float x, y;
                    md_td_window(px, py, hc, hs, R, m, (float)r + 0.25f + 0.5f * (float)(k >> 1), (float)cc + 0.25f + 0.5f * (float)(k & 1), &x, &y);
                    int nav = 0, line = 0;
                    for (int i = 0; i < n_quad && !line; ++i)
                        line = in_box(&quad_box[i], x, y) && md_td_on_line(w->quads + 8 * (size_t)quad_box[i].id, hw, x, y);
                    for (int i = 0; i < n_lane && !line && !nav; ++i) nav = in_box(&lane_box[i], x, y) && md_td_on_lane(&lanes[lane_box[i].id], x, y);
                    sum += line ? MD_TD_LINE : (nav ? MD_TD_NAV : 0);
                }
                sum4[r * R + cc] = sum;
                float x, y;
                md_td_window(px, py, hc, hs, R, m, (float)r + 0.5f, (float)cc + 0.5f, &x, &y);
                for (int i = 0; i < n_mover; ++i)
                    if (in_box(&mover_box[i], x, y) && md_td_in_box(&shape[mover_box[i].id], x, y)) {
                        traffic[r * wpr + (cc >> 5)] |= 1u << (cc & 31);
                        break;
                    }
            }
        free(lane_box);
        free(quad_box);
        /* the rings */
        int* cursor = td->cursor + 4 * (size_t)e;
        const int tcur_old = (int)((unsigned)cursor[0] % (unsigned)Lt), pcur_old = (int)((unsigned)cursor[1] % (unsigned)Lp);
        const int pcnt_old = cursor[2] < 0 ? 0 : (cursor[2] > Lp ? Lp : cursor[2]);
        const int pcur = reset ? 0 : (pcur_old + 1) % Lp, pcnt = reset ? 1 : (pcnt_old + 1 > Lp ? Lp : pcnt_old + 1);
        float* ring_pos = td->ring_pos + (size_t)e * (size_t)Lp * 2;
        ring_pos[2 * pcur] = px;
        ring_pos[2 * pcur + 1] = py;
        float sc, ss;
        md_td_snap(hc, hs, &sc, &ss);
        for (int i = 0; i < md_td_stack_count(pcnt, td->frame_skip); ++i) {
            const int back = pcnt - 1 - md_td_stack_index(pcnt, td->frame_skip, i);
            const int slot = (pcur + Lp - back) % Lp;
            int row, col;
            if (md_td_past_dot(ring_pos[2 * slot], ring_pos[2 * slot + 1], px, py, sc, ss, R, td->distance, &row, &col))
                past[row * wpr + (col >> 5)] |= 1u << (col & 31);
        }
        const int tcur = reset ? 0 : (tcur_old + 1) % Lt;
        uint32_t* ring = td->ring_traffic + (size_t)e * (size_t)Lt * (size_t)FW;
        for (int sl = 0; sl < Lt; ++sl)
            if (reset || sl == tcur) memcpy(ring + (size_t)sl * FW, traffic, sizeof(uint32_t) * (size_t)FW);
        cursor[0] = tcur;
        cursor[1] = pcur;
        cursor[2] = reset ? 0 : pcnt;
        cursor[3] = 0;
        /* the block */
        for (int pix = 0; pix < R * R; ++pix) {
            const int r = pix / R, cc = pix - r * R, wi = r * wpr + (cc >> 5);
            for (int ch = 0; ch < C; ++ch) {
                const size_t o = ((size_t)e * R * R + (size_t)pix) * C + ch;
                float vf;
                int vb;
                if (ch == 0) {
                    vf = md_td_road_float(sum4[pix]);
                    vb = md_td_road_byte(sum4[pix]);
                } else {
                    const uint32_t* frame = ch == 1 ? past : ring + (size_t)((tcur + Lt - (ch - 2) * td->frame_skip) % Lt) * FW;
                    const int on = (frame[wi] >> (cc & 31)) & 1u;
                    vf = on ? (ch == 1 ? 1.0f : md_td_traffic_float()) : 0.0f;
                    vb = on ? (ch == 1 ? 255 : md_td_traffic_byte()) : 0;
                }
                if (td->norm_pixel) ((float*)td->out)[o] = vf;
                else ((uint8_t*)td->out)[o] = (uint8_t)vb;
            }
        }
    }
    free(traffic);
    free(past);
    free(sum4);
}
