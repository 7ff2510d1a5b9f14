/* Host build of include/md_render.h (env.render(mode="topdown")), loaded by the tests through tests/hostlib.py.  Compiled with
 * gcc -O2 -ffp-contract=off: the rules are the header's, so the results are the md_render kernels' to the last bit.  Where the
 * kernel works tile by tile in primitive order and settles the painter's order through ranks, this walks the image in PIXEL order
 * and paints every pixel the painter's way: the lines, then every held frame from the oldest, every slot ascending, each one
 * overwriting the colour before it.  No tile, no rank; the only culls are a world-space bounding box per primitive and, per row of
 * pixels, the line pieces whose box meets the row's. */
#include <stdlib.h>
#include <string.h>

#include "md_render.h"

#define EXPORT __attribute__((visibility("default")))

EXPORT int hx_sizeof_render(void) { return (int)sizeof(MdRender); }
EXPORT void hx_rd_window(float px, float py, float uc, float us, int W, int H, float scaling, float fr, float fc, float* xy) {
    md_rd_window(px, py, uc, us, W, H, scaling, fr, fc, &xy[0], &xy[1]);
}
EXPORT float hx_rd_line_half_width(float scaling) { return md_rd_line_half_width(scaling); }
EXPORT int hx_rd_line_rgb(int kind) { return md_rd_line_rgb(md_rd_line_order(kind)); }
EXPORT int hx_rd_line_order(int kind) { return md_rd_line_order(kind); }
EXPORT int hx_rd_base_rgb(int flags, int slot) { return md_rd_base_rgb(flags, slot); }
EXPORT void hx_rd_drawn_size(int flags, float hl, float hw, float* out) { md_rd_drawn_size(flags, hl, hw, &out[0], &out[1]); }
EXPORT int hx_rd_fade(int rgb, int n, int k) { return md_rd_fade(rgb, md_rd_alpha(n, k)); }
EXPORT int hx_rd_frame_skipped(int n, int k, int smooth) { return md_rd_frame_skipped(n, k, smooth); }
EXPORT int hx_rd_contour_rgb(void) { return MD_RD_CONTOUR_RGB; }

typedef struct Box { float x0, y0, x1, y1; int id; } Box;
static int in_box(const Box* b, float x, float y) { return x >= b->x0 && x <= b->x1 && y >= b->y0 && y <= b->y1; }

/* One md_render call restated: r's pointers are host arrays, the ring and the cursors advanced in place like the device's. */
EXPORT void hx_render(const MdWorld* w, const MdState* g, const MdConfig* c, const MdRender* r) {
    const int W = r->width, H = r->height, cap = c->cap, S = r->num_stack;
    const float hw = md_rd_line_half_width(r->scaling), cw = MD_RD_CONTOUR_PIXELS / r->scaling;
    for (int ri = 0; ri < r->n_render; ++ri) {
        int e = r->env_ids[ri];
        e = e < 0 ? 0 : (e >= c->n_envs ? c->n_envs - 1 : e);
        const size_t b0 = (size_t)e * (size_t)cap;
        /* the push */
        int32_t* cursor = r->cursor + 4 * (size_t)ri;
        const int clock = md_rd_clock(g, c, e, g->nav + b0);
        int newest, held;
        md_rd_advance(cursor, S, clock, &newest, &held);
        MdShape* ring = r->ring + (size_t)ri * (size_t)S * (size_t)cap;
        for (int j = 0; j < cap; ++j) ring[(size_t)newest * cap + j] = md_rd_box_of(&g->shape[b0 + j], j);
        cursor[0] = newest;
        cursor[1] = held;
        cursor[2] = clock;
        cursor[3] = 0;
        /* the picture */
        float px, py, uc, us;
        md_rd_camera(r, &g->shape[b0 + r->track_agent], &px, &py, &uc, &us);
        int map = w->env_map[e];
        if (map < 0 || map >= w->n_maps) map = 0;
        const int qa = w->quad_off[map], qb = w->quad_off[map + 1];
        Box* quad_box = (Box*)malloc(sizeof(Box) * (size_t)(qb - qa + 1));
        int n_quad = 0;
        for (int q = qa; q < qb; ++q) {
            if (!md_rd_line_order(w->quad_kind[q])) continue;
            const float* v = w->quads + 8 * (size_t)q;
            Box b = {v[0], v[1], v[0], v[1], q};
            for (int i = 1; i < 4; ++i) {
                b.x0 = md_min(b.x0, v[2 * i]); b.x1 = md_max(b.x1, v[2 * i]);
                b.y0 = md_min(b.y0, v[2 * i + 1]); b.y1 = md_max(b.y1, v[2 * i + 1]);
            }
            b.x0 -= hw + 0.01f; b.y0 -= hw + 0.01f; b.x1 += hw + 0.01f; b.y1 += hw + 0.01f;
            quad_box[n_quad++] = b;
        }
        uint8_t* out = r->out + (size_t)ri * (size_t)H * (size_t)W * 3;
        int* row_quads = (int*)malloc(sizeof(int) * (size_t)(n_quad + 1));
        for (int row = 0; row < H; ++row) {
            /* the line pieces whose box meets the world-space box of this row of pixel centres (a straight segment) */
            float ax, ay, bx, by;
            md_rd_window(px, py, uc, us, W, H, r->scaling, (float)row + 0.5f, 0.5f, &ax, &ay);
            md_rd_window(px, py, uc, us, W, H, r->scaling, (float)row + 0.5f, (float)(W - 1) + 0.5f, &bx, &by);
            const float pad = 1.0f / r->scaling + 0.01f;
            const Box rb = {md_min(ax, bx) - pad, md_min(ay, by) - pad, md_max(ax, bx) + pad, md_max(ay, by) + pad, 0};
            int n_row = 0;
            for (int i = 0; i < n_quad; ++i)
                if (!(quad_box[i].x0 > rb.x1 || quad_box[i].x1 < rb.x0 || quad_box[i].y0 > rb.y1 || quad_box[i].y1 < rb.y0)) row_quads[n_row++] = i;
            for (int col = 0; col < W; ++col) {
                float x, y;
                md_rd_window(px, py, uc, us, W, H, r->scaling, (float)row + 0.5f, (float)col + 0.5f, &x, &y);
                int32_t rgb = MD_RD_WHITE;
                int best = 0;
                for (int t = 0; t < n_row; ++t) {
                    const int i = row_quads[t];
                    const int order = md_rd_line_order(w->quad_kind[quad_box[i].id]);
                    if (order > best && in_box(&quad_box[i], x, y) && md_td_on_line(w->quads + 8 * (size_t)quad_box[i].id, hw, x, y)) best = order;
                }
                if (best) rgb = md_rd_line_rgb(best);
                for (int k = 0; k < held; ++k) {
                    if (md_rd_frame_skipped(held, k, r->history_smooth)) continue;
                    const MdShape* frame = ring + (size_t)md_rd_ring_slot(newest, S, held, k) * cap;
                    const float alpha = md_rd_alpha(held, k);
                    for (int j = 0; j < cap; ++j) {
                        const MdShape* b = &frame[j];
                        if (b->flags == 0) continue;
                        const float ext = md_fabs(b->hl) + md_fabs(b->hw) + 0.01f;
                        if (!(md_fabs(x - b->cx) <= ext && md_fabs(y - b->cy) <= ext) || !md_td_in_box(b, x, y)) continue;
                        rgb = (k == held - 1 && r->draw_contour && md_rd_on_contour(b, cw, x, y)) ? MD_RD_CONTOUR_RGB : md_rd_fade(b->aux, alpha);
                    }
                }
                uint8_t* o = out + ((size_t)row * W + col) * 3;
                o[0] = (uint8_t)(rgb & 255);
                o[1] = (uint8_t)((rgb >> 8) & 255);
                o[2] = (uint8_t)((rgb >> 16) & 255);
            }
        }
        free(row_quads);
        free(quad_box);
    }
}
