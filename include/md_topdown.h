/*
 * md_topdown.h -- the top-down observation of TopDownMetaDrive / TopDownMetaDriveEnvV2 (envs/top_down_env.py:33-74):
 * TopDownMultiChannel.observe (obs/top_down_obs_multi_channel.py:237-280), an ego-centred R x R raster with the channels
 * [road_network, past_pos, traffic(t), traffic(t - frame_skip), ...], 2 + frame_stack of them.
 *
 * What this is NOT: the reference's pixels.  There the image is a chain of pygame blits on a 2000 x 2000 canvas whose scale is
 * rounded per map, a bilinear rotozoom and a smoothscale; nobody can restate that bit for bit.  Built here is the GEOMETRY the
 * reference draws, sampled exactly; every rule below names the reference's file and line.  Parity is pinned like md_ai_protect.h:
 * this header is the single source of the md_topdown kernel (csrc/parts/topdown.inc, rasterised in primitive order) and of the host build
 * of the tests (tests/topdown_host.c, brute force in pixel order); the rules use + - * /, comparisons and the shared md_math.h /
 * md_geom.h formulas only, so a gcc -ffp-contract=off build reproduces the device bit for bit.
 *
 * Window (ObservationWindow treats max_range as a RADIUS, obs/top_down_obs_impl.py:37-44: the window spans +-distance):
 *   m = 2 * distance / R metres per pixel; the centre of output row r, column c is the ego-frame point
 *   forward = (R/2 - (r + 0.5)) * m, left = (R/2 - (c + 0.5)) * m, i.e. the world point
 *   pos + forward * (cos h, sin h) + left * (-sin h, cos h): the ego looks UP the image and its left is the image's left
 *   (WorldSurface.pos2pix flips y, top_down_obs_impl.py:136-146; _rotate turns by heading + 90 deg, :58-74; observe transposes,
 *   top_down_obs_multi_channel.py:280).  h is the UNSNAPPED heading (render(heading=vehicle.heading_theta), :203).
 *
 * Channels:
 *   road_network  2 x 2 sub-samples per pixel (the reference renders this channel at twice the resolution and smoothscales it
 *                 down, :240).  A sub-sample is 64 on a lane of a road of the agent's route (draw_navigation_node, :119,282-287:
 *                 route_roads[0 .. route_len - 2] of slot 0, every lane, 0 <= s <= length and |lat| <= width / 2), and, over
 *                 that, 35 within half a line width of the centre segment of a line piece (MdWorld.quads of the kinds
 *                 MD_Q_LINE_*: the bodies built from the line_types LaneGraphics.display draws, :126-133; LANE_LINE_COLOR).
 *                 Line width = max(MD_TD_LINE_WIDTH, one sub-sample), so a line never falls between samples.  The pixel is the
 *                 mean g of its four sub-samples; float clip(2 g / 255, 0, 1), byte min(255, 2 floor(g)) (:229-234,255).
 *   traffic       a pixel CENTRE inside a mover's box hl x hw (circles as their bounding square: ObjectGraphics.display draws
 *                 LENGTH x WIDTH for everything, top_down_obs_impl.py:215-262); the movers are those the env's lidar sees
 *                 (md_present) of the kinds vehicle, pedestrian, cyclist (:167), minus the ego; a heading with |h| <= 2 deg is
 *                 drawn at 0 (:171-172).  Value (0.299 * 100 + 0.587 * 200 + 0.114 * 255) / 255 (ObjectGraphics.BLUE), byte 176.
 *   past_pos      one pixel of value 1 (byte 255) per stacked past ego position, :175-192 as they are: scaling =
 *                 resolution / max_distance (TWICE the window's scale, a quirk that is kept), the SNAPPED ego heading, no y
 *                 flip (so the dots are mirrored left / right against the window, kept too), the clip to +-R, the truncation
 *                 of the fill rectangle's origin towards zero.  A dot outside [0, R) is not drawn.
 *
 * History (engine-owned arrays of MdTopDown, like md_ai_protect's takeover bytes; MdState is not touched):
 *   ring_traffic  [n_envs][Lt][R][MD_TD_ROW_WORDS(R)] uint32, Lt = (frame_stack - 1) * frame_skip + 1: stack_traffic_flow (:54)
 *                 as 1-bit masks (bit c & 31 of word c >> 5 of a row).  A stacked frame is the image as it was rendered then, in
 *                 the ego frame of then; it is not re-projected.
 *   ring_pos      [n_envs][Lp][2] float, Lp = (post_stack - 1) * frame_skip + 1: stack_past_pos (:55)
 *   cursor        [n_envs][4] int32: slot of the newest traffic frame, slot of the newest position, positions held, 0
 * The step that returns an env's reset observation is recognised by MdNav.steps == 0 of slot 0 in the state md_step leaves
 * (md_observe counts the episode's steps from the step after the restore): the traffic ring is filled with the current frame
 * (_should_fill_stack, :246-251) and past_pos is the one dot of the current position, at (R/2, R/2); as in the reference the
 * position ring is left EMPTY by that step (observe clears it after the dot is drawn, :247), so the reset position itself is
 * never a past position.
 */
#ifndef MD_TOPDOWN_H
#define MD_TOPDOWN_H

#include "md_entity.h"

#define MD_TD_MAX_RES 128        /* resolution_size R at most */
#define MD_TD_MAX_RING 64        /* (frame_stack - 1) * frame_skip + 1 and (post_stack - 1) * frame_skip + 1 at most */
#define MD_TD_LINE_WIDTH 0.3f    /* 2 * PGDrivableAreaProperty.LANE_LINE_WIDTH (0.15 m), the width LaneGraphics draws a line at */
#define MD_TD_NAV 64             /* draw_navigation_node's grey (64, 64, 64) */
#define MD_TD_LINE 35            /* LANE_LINE_COLOR */
#define MD_TD_SNAP_SIN 0.0348994967f /* sin(2 deg): |h| <= 2 deg  <=>  cos h > 0 and |sin h| <= this */
#define MD_TD_ROW_WORDS(R) (((R) + 31) >> 5)

typedef struct MdTopDown {
    int32_t struct_size;   /* sizeof(MdTopDown) as the caller sees it */
    int32_t resolution;    /* resolution_size R */
    float distance;        /* m: the window spans +-distance */
    int32_t frame_stack, frame_skip, post_stack;
    int32_t norm_pixel;    /* 1: out is float32 in [0, 1]; 0: uint8 */
    int32_t reserved;      /* 0 */
    void* out;             /* [n_envs][R][R][2 + frame_stack] float32 or uint8 */
    uint32_t* ring_traffic;
    float* ring_pos;
    int32_t* cursor;
} MdTopDown;

MD_HD int md_td_ring_len(int stack, int skip) { return (stack - 1) * skip + 1; }
MD_HD float md_td_metres_per_pixel(int R, float distance) { return 2.0f * distance / (float)R; }

/* the world point of the (fractional) image coordinate (fr, fc) -- a pixel centre is (r + 0.5, c + 0.5), its sub-sample (i, j)
 * (r + 0.25 + 0.5 i, c + 0.25 + 0.5 j) -- for an ego at (px, py) with heading vector (hc, hs) */
MD_HD void md_td_window(float px, float py, float hc, float hs, int R, float m, float fr, float fc, float* x, float* y) {
    const float fwd = (0.5f * (float)R - fr) * m;
    const float left = (0.5f * (float)R - fc) * m;
    *x = px + fwd * hc - left * hs;
    *y = py + fwd * hs + left * hc;
}

/* a heading with |h| <= 2 deg is drawn at 0 (top_down_obs_multi_channel.py:165,172): (c, s) -> the drawn heading vector */
MD_HD void md_td_snap(float c, float s, float* oc, float* os) {
    const int snap = c > 0.0f && md_fabs(s) <= MD_TD_SNAP_SIN;
    *oc = snap ? 1.0f : c;
    *os = snap ? 0.0f : s;
}

/* road_network: on the drivable area of a lane (LaneGraphics.draw_drivable_area, top_down_obs_impl.py:430-458) */
MD_HD int md_td_on_lane(const MdLane* L, float x, float y) {
    float s, lat;
    md_lane_local(L, x, y, &s, &lat);
    return s >= 0.0f && s <= L->length && md_fabs(lat) <= L->width / 2.0f;
}

/* half the drawn line width: half of max(MD_TD_LINE_WIDTH, one sub-sample = m / 2) */
MD_HD float md_td_line_half_width(float m) { return md_max(MD_TD_LINE_WIDTH, m / 2.0f) / 2.0f; }

/* road_network: within hw of the centre segment of the line piece q (x0, y0 .. x3, y3; built as [p0 -+ n, p1 -+ n, p1 +- n,
 * p0 +- n], mapgen/tables.py: the centre segment runs from the middle of v0 v3 to the middle of v1 v2).  A strip with square
 * ends; no division and no root: t in [0, |d|^2], cross^2 <= hw^2 |d|^2. */
MD_HD int md_td_on_line(const float* q, float hw, float x, float y) {
    const float ax = (q[0] + q[6]) / 2.0f, ay = (q[1] + q[7]) / 2.0f;
    const float bx = (q[2] + q[4]) / 2.0f, by = (q[3] + q[5]) / 2.0f;
    const float dx = bx - ax, dy = by - ay;
    const float rx = x - ax, ry = y - ay;
    const float l2 = dx * dx + dy * dy;
    const float t = rx * dx + ry * dy;
    const float cr = rx * dy - ry * dx;
    return t >= 0.0f && t <= l2 && cr * cr <= hw * hw * l2;
}
MD_HD int md_td_is_line_kind(int kind) { return kind == MD_Q_LINE_WHITE_CONT || kind == MD_Q_LINE_YELLOW_CONT || kind == MD_Q_LINE_BROKEN; }

/* traffic: is the mover in `slot` drawn (isinstance BaseVehicle or BaseTrafficParticipant, not the ego; :167-170) */
MD_HD int md_td_drawn(int flags, int slot) {
    const int k = md_kind_of(flags);
    return slot != 0 && md_present(flags) && (k == MD_KIND_VEHICLE || k == MD_KIND_PEDESTRIAN || k == MD_KIND_CYCLIST);
}
/* traffic: (x, y) inside the mover's box, drawn at its snapped heading */
MD_HD int md_td_in_box(const MdShape* sh, float x, float y) {
    float c, s;
    md_td_snap(sh->c, sh->s, &c, &s);
    const float dx = x - sh->cx, dy = y - sh->cy;
    return md_fabs(dx * c + dy * s) <= sh->hl && md_fabs(dy * c - dx * s) <= sh->hw;
}

/* _get_stack_indices (top_down_obs_multi_channel.py:293-299): ceil(length / skip) indices, the i-th is length - 1 - i * skip */
MD_HD int md_td_stack_count(int length, int skip) { return (length + skip - 1) / skip; }
MD_HD int md_td_stack_index(int length, int skip, int i) { return length - 1 - i * skip; }

/* past_pos (:175-192): the dot of the past position (ox, oy) seen from the ego at (px, py) with the SNAPPED heading vector
 * (c, s).  diff * scaling, swapped, rotated by heading + 90 deg (cos = -s, sin = c), swapped back, + R/2, clipped to +-R, the
 * rectangle's origin truncated towards zero (pygame.Rect of floats).  -> 1 and (row, col) when the dot lies on the image. */
MD_HD int md_td_past_dot(float ox, float oy, float px, float py, float c, float s, int R, float distance, int* row, int* col) {
    const float scaling = (float)R / distance;
    const float vx = (oy - py) * scaling, vy = (ox - px) * scaling;    /* diff = (diff[1], diff[0]) */
    const float rx = vx * (0.0f - s) - vy * c;                          /* Vector2.rotate(deg(h) + 90) */
    const float ry = vx * c + vy * (0.0f - s);
    const float p0 = md_clip(ry + (float)R / 2.0f, (float)(-R), (float)R);   /* p = (p[1], p[0]) */
    const float p1 = md_clip(rx + (float)R / 2.0f, (float)(-R), (float)R);
    const int x = (int)p0, y = (int)p1;     /* fill((255, 255, 255), (p, (1, 1))); array3d is [x][y], observe transposes */
    *row = y;
    *col = x;
    return x >= 0 && x < R && y >= 0 && y < R;
}

/* value mapping.  road: sum4 = the sum of the pixel's four sub-samples (each 0, MD_TD_NAV or MD_TD_LINE), g = sum4 / 4 */
MD_HD float md_td_road_float(int sum4) { return md_clip(2.0f * ((float)sum4 * 0.25f) / 255.0f, 0.0f, 1.0f); }
MD_HD int md_td_road_byte(int sum4) {
    const int v = 2 * (sum4 / 4);
    return v > 255 ? 255 : v;
}
MD_HD float md_td_traffic_grey(void) { return 0.299f * 100.0f + 0.587f * 200.0f + 0.114f * 255.0f; }   /* _transform, :229 */
MD_HD float md_td_traffic_float(void) { return md_clip(md_td_traffic_grey() / 255.0f, 0.0f, 1.0f); }
MD_HD int md_td_traffic_byte(void) { return (int)md_td_traffic_grey(); }                                 /* astype(uint8): 176 */

/* the step returns the env's reset observation (nav: the env's slot 0) */
MD_HD int md_td_is_reset(const MdNav* nav) { return nav->steps == 0; }

/* C-ABI entry point (libmdstep.so).  ONE launch, one workgroup per env, on the state md_step left (after the detectors: the
 * image belongs to the map of MdWorld.env_map, so it goes before md_swap_draw / md_curriculum move an env on): rasterises the
 * env's road and traffic, advances the two rings and writes td->out.  Refused: agents_per_env != 1 (the reference asserts the
 * same, :151), traffic_mode 4 (scenario mode: its trajectory navigation and polyline map lines are not built), sizes beyond the
 * MD_TD_* limits, frame_stack / post_stack / frame_skip < 1, distance <= 0.  MdWorld.quads and, where set, MdWorld.quad_ball are read
 * 16 bytes at a time and must be 16-byte aligned (refused otherwise); td->out may have any alignment (a 16-byte aligned one whose
 * per-env block is a multiple of 16 bytes gets the wide stores).  Returns MD_OK or an error (md_last_error). */
#ifdef __cplusplus
extern "C" {
#endif
int md_topdown(const MdWorld* w, const MdState* s, const MdConfig* c, const MdTopDown* td, void* stream);
#ifdef __cplusplus
}
#endif

#endif /* MD_TOPDOWN_H */
