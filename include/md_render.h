/*
 * md_render.h -- env.render(mode="topdown"): the bird's-eye picture of TopDownRenderer (obs/top_down_renderer.py, reached through
 * envs/base_env.py:482-492,756 -> engine.render_topdown), one RGB frame per chosen env of the batch.
 *
 * What this is NOT: pygame's pixels.  The reference paints polygons with pygame.draw on a canvas of the whole map, blits a window
 * out of it and, heading up, turns it with a bilinear rotozoom; its edges are anti-aliased by nothing and rounded by everything.
 * Built here is the GEOMETRY the reference draws, sampled exactly: one sample per pixel, at its centre.  Every rule below names the
 * reference's file and line.  Parity is pinned like md_topdown.h: this header is the single source of the md_render kernels
 * (csrc/parts/render.inc: tiled, primitive order, painter's order through ranks) and of the host build of the tests (tests/render_host.c: brute
 * force in pixel order); the rules use + - * /, comparisons and the shared md_math.h / md_geom.h formulas only, so a
 * gcc -ffp-contract=off build reproduces the device bit for bit.  Left out: the red dots the reference leaves where an agent
 * finished (:476-492); and heading up the whole window is sampled, where the reference turns a canvas that reaches 100 * sqrt(2) m
 * from the agent (:268-271) and shows nothing beyond it.
 *
 * Window (W x H pixels, `scaling` pixels per metre; the reference's defaults are scaling=5, screen_size=(1000, 1000)):
 *   the camera is the position of the tracked agent (slot track_agent of the env: current_track_agent) or, with fixed_camera, the
 *   point (cam_x, cam_y) (camera_position, top_down_renderer.py:497-504).  The centre of output row r, column c is the world point
 *     cam + up * (uc, us) + right * (us, -uc),  up = (H/2 - (r + 0.5)) / scaling,  right = ((c + 0.5) - W/2) / scaling
 *   with the up vector (uc, us) = (0, 1): world x to the right, world y up (WorldSurface.pos2pix flips y,
 *   top_down_obs_impl.py:136-146).  With heading_up (target_vehicle_heading_up, :505-527: rotation by heading + 90 deg about the
 *   tracked agent, whose position is then the camera whatever camera_position says) the up vector is the tracked agent's UNSNAPPED
 *   heading vector: it looks up the image.  The tracked slot is read as it is, alive or not.
 *
 * Background: white (WorldSurface.fill(WHITE)); over it the map's line pieces (MdWorld.quads of the kinds MD_Q_LINE_*), the centre
 *   strip of a piece as md_td_on_line has it, of width max(MD_TD_LINE_WIDTH, one pixel); coloured by kind as
 *   LaneGraphics.display(use_line_color=True) does (top_down_obs_impl.py:294-300): yellow continuous (255, 175, 35), broken
 *   (175, 175, 175), white continuous (95, 95, 95) -- the SIDE colour; a quad's kind cannot tell a side line from the toll block's
 *   white separators, which the reference draws (175, 175, 175): a declared deviation.  Sidewalk and crosswalk
 *   strips are not drawn (the non-semantic renderer draws none).  Where kinds overlap: broken < white < yellow.  No lane table is
 *   read, so a scenario's polyline map, whose road lines and boundaries are quads too, is drawn by the same rule.
 *
 * Movers: every slot with md_present(flags), of every kind (get_objects(not map related), top_down_renderer.py:309), a box at its
 *   snapped heading (|h| <= 2 deg -> 0, :463) of the size top_down_length x top_down_width of its kind (md_rd_drawn_size).
 *   Colour (md_rd_base_rgb): MD_F_AGENT slots the special green (2, 158, 115), entry 2 of the colorblind palette
 *   (base_vehicle.py:968-973); cones, warnings and barriers (235, 84, 42) (traffic_object.py:75-76); everything else entry slot % 9
 *   of the nine remaining palette colours -- the reference draws a random one per object (base_object.py:154-158), the slot index is
 *   the stand-in (declared).  With draw_contour the pixels inside a box of the CURRENT frame within 2 pixels of
 *   its edge are (60, 60, 60) (ObjectGraphics.BLACK, contour_width=2, :469-471).
 *
 * History (history_objects, :239-240,311): the boxes of the last num_stack render calls, the current one included.  Of the n frames
 *   held, frame k (k = 0 the oldest, k = n - 1 the current one) is painted before the newer ones; a history frame (k < n - 1) has
 *   no contour, is skipped when history_smooth != 0 and (n - k) % history_smooth != 0, and is faded towards white by
 *   alpha = (float)(n - k) / (float)n: c + alpha * (255 - c) per channel, truncated to a byte (:417-433; the oldest of a full
 *   history is therefore white).  The current frame is painted last, at alpha 0.
 *   PAINTER'S ORDER: lines (broken, white, yellow), then the frames oldest -> newest, within a frame ascending slot index; the last
 *   painter of a pixel wins.  Both builds give the same pixel wherever boxes overlap.
 *
 * Episode boundaries: the reference clears its renderer at reset (base_env.py:526-528).  The episode clock of a rendered env is
 *   MdNav.steps of its slot 0 in a single-agent batch and MdState.env_steps[e] in a multi-agent one; a call that finds the clock 0
 *   or smaller than at the env's previous call empties the history before the current frame is pushed.  A caller who renders less
 *   often than every step can miss a reset.  In a walking batch the swap to the next scene happens inside step(): the one frame
 *   between an episode's end and its reset step is drawn on the next scene's map.
 *
 * Engine-owned arrays of MdRender (MdState is read only; a checkpoint does not carry the viewer's history):
 *   ring    [n_render][num_stack][cap] MdShape: what a box needs -- cx, cy, the UNSNAPPED heading vector c, s (md_td_in_box snaps),
 *           hl, hw the DRAWN half sizes, flags (0: nothing to draw), aux the base colour 0xBBGGRR
 *   cursor  [n_render][4] int32: ring slot of the newest frame, frames held, the episode clock at the previous call, 0
 */
#ifndef MD_RENDER_H
#define MD_RENDER_H

#include "md_topdown.h"

#define MD_RD_MAX_SIZE 1024     /* W and H at most */
#define MD_RD_MAX_STACK 32      /* num_stack at most */
#define MD_RD_TILE 64           /* the kernel's tile: MD_RD_TILE x MD_RD_TILE pixels per workgroup */
#define MD_RD_CONTOUR_PIXELS 2.0f   /* contour_width=2, top_down_renderer.py:470 */
#define MD_RD_WHITE 0xFFFFFF
#define MD_RD_CONTOUR_RGB 0x3C3C3C  /* ObjectGraphics.BLACK = (60, 60, 60) */

#define MD_RD_RGB(r, g, b) ((int32_t)(r) | ((int32_t)(g) << 8) | ((int32_t)(b) << 16))

typedef struct MdRender {
    int32_t struct_size;      /* sizeof(MdRender) as the caller sees it */
    int32_t width, height;    /* W, H */
    float scaling;            /* pixels per metre */
    int32_t num_stack, history_smooth;
    int32_t track_agent;      /* agent slot whose position (and heading, heading_up) is the camera */
    int32_t heading_up, draw_contour, fixed_camera;
    float cam_x, cam_y;       /* fixed_camera and not heading_up: the camera */
    int32_t n_render;         /* envs rendered by this call */
    int32_t reserved;         /* 0 */
    const int32_t* env_ids;   /* [n_render], each in [0, n_envs) (clamped on the device) */
    uint8_t* out;             /* [n_render][H][W][3] */
    MdShape* ring;            /* [n_render][num_stack][cap] */
    int32_t* cursor;          /* [n_render][4] */
} MdRender;

/* the world point of the (fractional) image coordinate (fr, fc) -- a pixel centre is (r + 0.5, c + 0.5) -- for a camera at
 * (px, py) whose up vector is (uc, us) */
MD_HD void md_rd_window(float px, float py, float uc, float us, int W, int H, float scaling, float fr, float fc, float* x, float* y) {
    const float up = (0.5f * (float)H - fr) / scaling;
    const float right = (fc - 0.5f * (float)W) / scaling;
    *x = px + up * uc + right * us;
    *y = py + up * us - right * uc;
}

/* the camera and the up vector of a rendered env; `tracked`: the shape of slot track_agent */
MD_HD void md_rd_camera(const MdRender* r, const MdShape* tracked, float* px, float* py, float* uc, float* us) {
    const int fixed = r->fixed_camera && !r->heading_up;
    *px = fixed ? r->cam_x : tracked->cx;
    *py = fixed ? r->cam_y : tracked->cy;
    /* a slot that never held a mover has no heading vector: the window would collapse into one point */
    const float l2 = tracked->c * tracked->c + tracked->s * tracked->s;
    const int turn = r->heading_up && l2 > 0.5f && l2 < 2.0f;
    *uc = turn ? tracked->c : 0.0f;
    *us = turn ? tracked->s : 1.0f;
}

/* half the drawn line width: half of max(MD_TD_LINE_WIDTH, one pixel) */
MD_HD float md_rd_line_half_width(float scaling) { return md_max(MD_TD_LINE_WIDTH, 1.0f / scaling) / 2.0f; }

/* a line kind's place in the painter's order (0: not drawn) and its colour */
MD_HD int md_rd_line_order(int kind) {
    return kind == MD_Q_LINE_BROKEN ? 1 : (kind == MD_Q_LINE_WHITE_CONT ? 2 : (kind == MD_Q_LINE_YELLOW_CONT ? 3 : 0));
}
MD_HD int32_t md_rd_line_rgb(int order) {
    return order == 3 ? MD_RD_RGB(255, 175, 35) : (order == 2 ? MD_RD_RGB(95, 95, 95) : MD_RD_RGB(175, 175, 175));
}

/* top_down_length / 2, top_down_width / 2 of a mover whose shape record holds (hl, hw): vehicles and cyclists as they are; the cone
 * 4 * RADIUS square and the warning 2 * RADIUS square (traffic_object.py:67-72,110-115; RADIUS 0.2 / 0.5), the barrier with its
 * sides swapped, 2 * WIDTH x LENGTH = 0.6 x 2.0 (:170-177), the pedestrian 2 * RADIUS square (pedestrian.py:113-118; RADIUS 0.35),
 * the toll booth BUILDING_LENGTH x 3 (tollgate_building.py:36-41) */
MD_HD void md_rd_drawn_size(int flags, float hl, float hw, float* dl, float* dw) {
    const int k = md_kind_of(flags);
    *dl = k == MD_KIND_CONE ? 0.4f : (k == MD_KIND_WARNING ? 0.5f : (k == MD_KIND_BARRIER ? 0.3f : (k == MD_KIND_PEDESTRIAN ? 0.35f : (k == MD_KIND_BUILDING ? 5.0f : hl))));
    *dw = k == MD_KIND_CONE ? 0.4f : (k == MD_KIND_WARNING ? 0.5f : (k == MD_KIND_BARRIER ? 1.0f : (k == MD_KIND_PEDESTRIAN ? 0.35f : (k == MD_KIND_BUILDING ? 1.5f : hw))));
}

/* sns.color_palette("colorblind") without its entry 2, as bytes (base_object.py:154-155) */
MD_HD int32_t md_rd_palette(int i) {
    switch (i) {
    case 0: return MD_RD_RGB(1, 115, 178);
    case 1: return MD_RD_RGB(222, 143, 5);
    case 2: return MD_RD_RGB(213, 94, 0);
    case 3: return MD_RD_RGB(204, 120, 188);
    case 4: return MD_RD_RGB(202, 145, 97);
    case 5: return MD_RD_RGB(251, 175, 228);
    case 6: return MD_RD_RGB(148, 148, 148);
    case 7: return MD_RD_RGB(236, 225, 51);
    default: return MD_RD_RGB(86, 180, 233);
    }
}
MD_HD int32_t md_rd_base_rgb(int flags, int slot) {
    const int k = md_kind_of(flags);
    if (flags & MD_F_AGENT) return MD_RD_RGB(2, 158, 115);
    if (k == MD_KIND_CONE || k == MD_KIND_WARNING || k == MD_KIND_BARRIER) return MD_RD_RGB(235, 84, 42);
    return md_rd_palette(slot % 9);
}

/* what the ring keeps of the mover in `slot` (flags 0: nothing to draw) */
MD_HD MdShape md_rd_box_of(const MdShape* sh, int slot) {
    MdShape b = *sh;
    if (!md_present(sh->flags)) {
        b.flags = 0;
        b.aux = 0;
        return b;
    }
    md_rd_drawn_size(sh->flags, sh->hl, sh->hw, &b.hl, &b.hw);
    b.aux = md_rd_base_rgb(sh->flags, slot);
    return b;
}

/* history: is frame k of n skipped, its alpha, a faded colour */
MD_HD int md_rd_frame_skipped(int n, int k, int smooth) { return k < n - 1 && smooth != 0 && (n - k) % smooth != 0; }
MD_HD float md_rd_alpha(int n, int k) { return k == n - 1 ? 0.0f : (float)(n - k) / (float)n; }
MD_HD int md_rd_fade_byte(int c, float alpha) { return (int)((float)c + alpha * (float)(255 - c)); }
MD_HD int32_t md_rd_fade(int32_t rgb, float alpha) {
    return MD_RD_RGB(md_rd_fade_byte(rgb & 255, alpha), md_rd_fade_byte((rgb >> 8) & 255, alpha), md_rd_fade_byte((rgb >> 16) & 255, alpha));
}

/* (x, y), inside the box b, lies within cw metres of its edge (cw = MD_RD_CONTOUR_PIXELS / scaling) */
MD_HD int md_rd_on_contour(const MdShape* b, float cw, float x, float y) {
    float c, s;
    md_td_snap(b->c, b->s, &c, &s);
    const float dx = x - b->cx, dy = y - b->cy;
    return b->hl - md_fabs(dx * c + dy * s) < cw || b->hw - md_fabs(dy * c - dx * s) < cw;
}

/* the episode clock of env e (nav0: its slot 0) and the history's fate: (clock, the clock at the previous call) -> emptied first */
MD_HD int md_rd_clock(const MdState* s, const MdConfig* c, int e, const MdNav* nav0) { return c->is_multi_agent ? s->env_steps[e] : nav0->steps; }
MD_HD int md_rd_new_episode(int clock, int prev) { return clock <= 0 || clock < prev; }

/* the cursors as a call finds them, sanitised (they index the ring), and as it leaves them */
MD_HD void md_rd_advance(const int32_t* cursor, int num_stack, int clock, int* newest, int* held) {
    const int old_newest = (int)((uint32_t)cursor[0] % (uint32_t)num_stack);
    const int old_held = cursor[1] < 0 ? 0 : (cursor[1] > num_stack ? num_stack : cursor[1]);
    const int fresh = md_rd_new_episode(clock, cursor[2]) || old_held == 0;
    *newest = fresh ? 0 : (old_newest + 1) % num_stack;
    *held = fresh ? 1 : (old_held + 1 > num_stack ? num_stack : old_held + 1);
}
/* the ring slot of frame k of n (k = n - 1 the newest) */
MD_HD int md_rd_ring_slot(int newest, int num_stack, int n, int k) { return (newest + num_stack - (n - 1 - k)) % num_stack; }

/* C-ABI entry point (libmdstep.so).  One call = a small launch that pushes the current boxes into each rendered env's ring and
 * advances its cursor, then the raster launch, one workgroup per (tile, rendered env), which writes r->out; stream order makes the
 * first visible to the second.  Reads the state as md_step (and whatever follows it in a step) left it; MdState is not written.
 * Refused, by name and before any launch: a wrong struct_size, null required pointers, n_render < 1, W or H outside
 * [1, MD_RD_MAX_SIZE], scaling <= 0, num_stack outside [1, MD_RD_MAX_STACK], history_smooth < 0, track_agent outside the agent slots,
 * misaligned MdWorld.quads / quad_ball (read 16 bytes at a time).  r->out may have any alignment (a 16-byte aligned one with
 * W a multiple of 16 gets the wide stores).  Returns MD_OK or an error (md_last_error). */
#ifdef __cplusplus
extern "C" {
#endif
int md_render(const MdWorld* w, const MdState* s, const MdConfig* c, const MdRender* r, void* stream);
#ifdef __cplusplus
}
#endif

#endif /* MD_RENDER_H */
