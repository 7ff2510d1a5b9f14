// parts/topdown.inc -- part of mdstep.hip, included there and not compiled on its own.
// Provides: MD_TD_SKIP, the LDS layout topdown_lds / topdown_staged and topdown_kernel<NORM> (include/md_topdown.h).
// Relies on: mdstep.hip (align_up, bcast_*, wave_lds_sync, QuadBall, quad_ball_of).

namespace {

// ---- md_topdown (include/md_topdown.h): the top-down observation, one workgroup per env -------------------------------------
// Rasterised in PRIMITIVE order into an LDS image: every route lane, line piece and mover that survives its cull touches only the
// pixels of its own bounding box in the image.  The road plane holds one byte per pixel, two bits per sub-sample (bit 0: on a
// route lane, bit 1: on a line, which wins), so that navigation and lines are set with ds_or and need no order between them; the
// traffic and past_pos planes hold one bit per pixel.  The epilogue composes the env's R x R x C block and writes it with 16-byte
// non-temporal stores wherever the block is 16-byte aligned.
// Diagnostic builds only (tools/topdown_bench.py under MD_LIB_PATH): phases of topdown_kernel left out, each by one #if around it,
// to read their cost off the launch time (1 route lanes, 2 line pieces, 4 movers, 8 compose + write).  0 in the product.
#ifndef MD_TD_SKIP
#define MD_TD_SKIP 0
#endif
struct TopdownLds { uint32_t road, traffic, past, queue, pieces, stage, bytes; };
constexpr int kTdQueue = 128;     // pixels a wave keeps between its cull and its exact test (two passes' worth)
// `staged`: the older traffic frames (frame_stack - 1 of them) the epilogue reads, copied into LDS first
__host__ __device__ constexpr TopdownLds topdown_lds(int R, int staged) {
    // a plane is R * ceil(R / 32) words, an odd count for many an odd R: rounded up so that every part below starts on 16 bytes
    // (the piece lists are written with 16-byte LDS stores)
    const uint32_t plane = align_up((uint32_t)R * (uint32_t)MD_TD_ROW_WORDS(R) * 4u, 16);
    const uint32_t traffic = align_up((uint32_t)R * (uint32_t)R, 16);
    const uint32_t queue = traffic + 2u * plane, pieces = queue + 4u * kTdQueue * 2u, stage = pieces + 4u * 64u * 32u;
    return TopdownLds{0u, traffic, traffic + plane, queue, pieces, stage, stage + (uint32_t)staged * plane};
}
// the older frames are staged while the image fits the 64 KB of LDS a launch may ask for without more ado; beyond (R and
// frame_stack both near their limits) the epilogue reads them from the ring
__host__ __device__ constexpr int topdown_staged(int R, int frame_stack) {
    return topdown_lds(R, frame_stack - 1).bytes <= 64u * 1024u ? frame_stack - 1 : 0;
}
// the two sizes tests/test_gpu_topdown_placed.py stands on: the largest staged image, and the first that reads the ring
static_assert(topdown_staged(128, 18) == 17 && topdown_staged(128, 19) == 0 && topdown_lds(128, 17).bytes == 64512);

struct TdView { float px, py, hc, hs, m, inv_m, half; int R; };
struct TdBox { int r0, c0, w, h; };

// the pixels that can hold a sample of the convex hull of the four world points xy, grown by `grow` pixels
__device__ __forceinline__ TdBox td_bbox(const TdView& v, const float* xy, int grow) {
    float rmin = 3.0e38f, rmax = -3.0e38f, cmin = 3.0e38f, cmax = -3.0e38f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const float dx = xy[2 * i] - v.px, dy = xy[2 * i + 1] - v.py;
        const float fr = v.half - (dx * v.hc + dy * v.hs) * v.inv_m;
        const float fc = v.half - (dy * v.hc - dx * v.hs) * v.inv_m;
        rmin = md_min(rmin, fr); rmax = md_max(rmax, fr);
        cmin = md_min(cmin, fc); cmax = md_max(cmax, fc);
    }
    const float lo = -8.0f, hi = (float)v.R + 8.0f;     // keeps the conversions to int in range (NaN -> lo)
    const int r0 = (int)md_floor(md_clip(rmin, lo, hi)) - grow, r1 = (int)md_floor(md_clip(rmax, lo, hi)) + grow;
    const int c0 = (int)md_floor(md_clip(cmin, lo, hi)) - grow, c1 = (int)md_floor(md_clip(cmax, lo, hi)) + grow;
    TdBox b;
    b.r0 = r0 < 0 ? 0 : r0;
    b.c0 = c0 < 0 ? 0 : c0;
    const int r1c = r1 > v.R - 1 ? v.R - 1 : r1, c1c = c1 > v.R - 1 ? v.R - 1 : c1;
    b.h = r1c >= b.r0 ? r1c - b.r0 + 1 : 0;
    b.w = c1c >= b.c0 ? c1c - b.c0 + 1 : 0;
    return b;
}

// One wave: the four sub-samples of every pixel of `b` against test(x, y); hits are OR-ed into the road plane as `code`.  The
// pixels first pass near(x, y) of their CENTRE -- a cheap conservative test: it may only reject a pixel none of whose samples (at
// most 0.36 m pixels from the centre) can hit -- and the survivors are compacted through the wave's `queue`, so that the exact
// test runs on full waves: a curved lane's bounding box is mostly empty.
template <typename Near, typename Test>
__device__ __forceinline__ void td_raster_road(const TdView& v, const TdBox& b, uint32_t* road, unsigned code, int lane_id, uint16_t* queue,
                                               Near near, Test test) {
    const int n = b.w * b.h;
    auto exact = [&](int p, int r, int cc) {
        unsigned bits = 0u;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            float x, y;
            md_td_window(v.px, v.py, v.hc, v.hs, v.R, v.m, (float)r + 0.25f + 0.5f * (float)(k >> 1), (float)cc + 0.25f + 0.5f * (float)(k & 1), &x, &y);
            if (test(x, y)) bits |= code << (2 * k);
        }
        if (bits) atomicOr(&road[p >> 2], bits << (8 * (p & 3)));
    };
    if (n <= 64) {      // one pass: no compaction to gain
        if (lane_id < n) {
            const int dr = lane_id / b.w;
            const int r = b.r0 + dr, cc = b.c0 + (lane_id - dr * b.w);
            exact(r * v.R + cc, r, cc);
        }
        return;
    }
    int qn = 0;
    for (int base = 0; base < n; base += 64) {
        const int idx = base + lane_id;
        bool keep = false;
        int pix = 0;
        if (idx < n) {
            const int dr = idx / b.w;
            const int r = b.r0 + dr, cc = b.c0 + (idx - dr * b.w);
            float x, y;
            md_td_window(v.px, v.py, v.hc, v.hs, v.R, v.m, (float)r + 0.5f, (float)cc + 0.5f, &x, &y);
            keep = near(x, y);
            pix = r * v.R + cc;
        }
        const unsigned long long mask = __ballot(keep);
        if (keep) queue[qn + __popcll(mask & ((1ull << lane_id) - 1ull))] = (uint16_t)pix;
        qn += __popcll(mask);
        const bool last = base + 64 >= n;
        while (qn >= 64 || (last && qn > 0)) {
            wave_lds_sync();
            const int take = qn < 64 ? qn : 64;
            if (lane_id < take) {
                const int p = queue[qn - take + lane_id];
                const int r = p / v.R;
                exact(p, r, p - r * v.R);
            }
            qn -= take;
            wave_lds_sync();
        }
    }
}

template <bool NORM>
__global__ __launch_bounds__(256) void topdown_kernel(const MdWorld w, const MdState g, const MdConfig c, const MdTopDown td, const int vec) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int e = blockIdx.x, tid = threadIdx.x, lane_id = tid & 63, wave = tid >> 6;
    const int R = td.resolution, wpr = MD_TD_ROW_WORDS(R), FW = R * wpr;
    const int staged = topdown_staged(R, td.frame_stack);
    const TopdownLds lds = topdown_lds(R, staged);
    uint32_t* road = reinterpret_cast<uint32_t*>(smem + lds.road);
    uint32_t* traffic = reinterpret_cast<uint32_t*>(smem + lds.traffic);
    uint32_t* past = reinterpret_cast<uint32_t*>(smem + lds.past);
    uint16_t* queue = reinterpret_cast<uint16_t*>(smem + lds.queue) + wave * kTdQueue;
    float* pieces = reinterpret_cast<float*>(smem + lds.pieces) + wave * 64 * 8;
    uint32_t* stage = reinterpret_cast<uint32_t*>(smem + lds.stage);
    for (int i = tid; i < (int)(lds.queue >> 2); i += 256) road[i] = 0u;

    const size_t b0 = (size_t)e * (size_t)c.cap;
    const MdShape ego = g.shape[b0];
    const MdNav nav0 = g.nav[b0];
    const bool reset = md_td_is_reset(&nav0);
    const int Lt = md_td_ring_len(td.frame_stack, td.frame_skip), Lp = md_td_ring_len(td.post_stack, td.frame_skip);
    int* cursor = td.cursor + 4 * (size_t)e;
    // the cursors as the previous launch left them (sanitised: they index the rings)
    const int tcur_old = (int)((unsigned)cursor[0] % (unsigned)Lt), pcur_old = (int)((unsigned)cursor[1] % (unsigned)Lp);
    const int pcnt_old = cursor[2] < 0 ? 0 : (cursor[2] > Lp ? Lp : cursor[2]);
    TdView v;
    v.px = ego.cx; v.py = ego.cy; v.hc = ego.c; v.hs = ego.s; v.R = R;
    v.m = md_td_metres_per_pixel(R, td.distance);
    v.inv_m = 1.0f / v.m;
    v.half = 0.5f * (float)R;
    const float hw = md_td_line_half_width(v.m);
    const float rwin = td.distance * 1.41422f + 2.0f * v.m;     // the window's circumscribed circle, with a margin
    int map = w.env_map[e];
    if (map < 0 || map >= w.n_maps) map = 0;
    __syncthreads();

    // ---- road_network: the route's lanes (a wave per road), then the line pieces (64 culled per wave and pass) ----
    const int lane_a = w.lane_off[map], n_lanes = w.lane_off[map + 1] - lane_a;
    const int road_a = w.road_off[map], n_roads = w.road_off[map + 1] - road_a;
    int n_route = nav0.route_len - 1;
    n_route = n_route > MD_ROUTE_LEN ? MD_ROUTE_LEN : n_route;
    const float pad = 0.36f * v.m + 0.01f;      // a pixel's samples lie within 0.25 * sqrt(2) pixels of its centre
    // the route's roads, one per lane of the wave (two dependent loads for all of them at once), then handed round
    int my_first = 0, my_n = 0;
    if (lane_id < n_route) {
        const int rid = g.route_roads[b0 * MD_ROUTE_LEN + lane_id];
        if (rid >= 0 && rid < n_roads) {
            const MdRoad rd = w.roads[road_a + rid];
            my_first = rd.first_lane;
            my_n = rd.n_lanes;
        }
    }
#if !(MD_TD_SKIP & 1)
    int item = 0;                               // the route's lanes, dealt to the waves in turn
    for (int j = 0; j < n_route; ++j) {
        const int first_lane = bcast_i(my_first, j), road_lanes = min(bcast_i(my_n, j), n_lanes);
        for (int l = 0; l < road_lanes; ++l) {
            if (((item++) & 3) != wave) continue;
            const int id = first_lane + l;
            if (id < 0 || id >= n_lanes) continue;
            const MdLane* L = &w.lanes[lane_a + id];
            // the lane's AABB against the window's circle
            const float ex = md_max(md_max(L->x0 - v.px, v.px - L->x1), 0.0f), ey = md_max(md_max(L->y0 - v.py, v.py - L->y1), 0.0f);
            // MdLane.x0 .. y1 is the AABB of the lane's hull, which mapgen/lanes.py builds from a densely sampled polygon of the lane's
            // outline with tangent extensions: chords of an arc miss it by centimetres, so 1.5 m (here and for the box below) is a wide
            // margin.  tests/topdown_host.c culls on the same AABB with 1.0 m: should the hull ever be sampled coarsely, BOTH margins
            // have to grow -- the two sides would otherwise miss the same part of an arc and still agree
            if (ex * ex + ey * ey > (rwin + 1.5f) * (rwin + 1.5f)) continue;
            float pts[8];
            if (L->type == 0 && L->hull_n == 4) {
#pragma unroll
                for (int i = 0; i < 8; ++i) pts[i] = L->hull4[i];
            } else {      // the AABB of the hull, grown beyond what a polygon of chords can miss of the arc
                const float gx = 1.5f;
                pts[0] = L->x0 - gx; pts[1] = L->y0 - gx; pts[2] = L->x1 + gx; pts[3] = L->y0 - gx;
                pts[4] = L->x1 + gx; pts[5] = L->y1 + gx; pts[6] = L->x0 - gx; pts[7] = L->y1 + gx;
            }
            const TdBox b = td_bbox(v, pts, 2);
            const float half = L->width / 2.0f + pad;
            if (L->type == 0) {
                td_raster_road(v, b, road, 1u, lane_id, queue,
                               [&](float x, float y) {
                                   const float dx = x - L->ax, dy = y - L->ay;
                                   const float sl = dx * L->bx + dy * L->by, lat = dx * L->by - dy * L->bx;
                                   return sl >= -pad && sl <= L->length + pad && md_fabs(lat) <= half;
                               },
                               [&](float x, float y) { return md_td_on_lane(L, x, y) != 0; });
            } else {      // the ring of the arc's radius: no angle, no root
                const float lo = md_max(L->bx - half, 0.0f), hi = L->bx + half;
                td_raster_road(v, b, road, 1u, lane_id, queue,
                               [&](float x, float y) {
                                   const float dx = x - L->ax, dy = y - L->ay, r2 = dx * dx + dy * dy;
                                   return r2 >= lo * lo && r2 <= hi * hi;
                               },
                               [&](float x, float y) { return md_td_on_lane(L, x, y) != 0; });
            }
        }
    }
#endif
#if !(MD_TD_SKIP & 2)
    const int qa = w.quad_off[map], qb = w.quad_off[map + 1];
    const int line_grow = 1 + (int)(hw * v.inv_m + 0.5f);      // a sample on the strip lies within hw of the piece's own extent: at least half a pixel to spare
    for (int q0 = qa + wave * 64; q0 < qb; q0 += 4 * 64) {
        bool keep = false;
        if (q0 + lane_id < qb) {
            const QuadBall qbl = quad_ball_of(w, q0 + lane_id);
            const float dx = qbl.mx - v.px, dy = qbl.my - v.py, reach = qbl.rr + rwin + hw;
            keep = md_td_is_line_kind(qbl.kind) && dx * dx + dy * dy <= reach * reach;
        }
        // The pieces kept go into the wave's list (fetched by all lanes at once); then 16 lanes take a piece, four pieces at a
        // time: a stripe's box is a dozen pixels, a whole wave on it would idle
        const unsigned long long mask = __ballot(keep);
        const int kept = __popcll(mask);
        if (keep) {
            const float4* qp = reinterpret_cast<const float4*>(w.quads) + 2 * (size_t)(q0 + lane_id);
            float4* dst = reinterpret_cast<float4*>(pieces) + 2 * __popcll(mask & ((1ull << lane_id) - 1ull));
            dst[0] = qp[0];
            dst[1] = qp[1];
        }
        wave_lds_sync();
        for (int k = lane_id >> 4; k < kept; k += 4) {
            float q[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) q[i] = pieces[8 * k + i];
            const TdBox b = td_bbox(v, q, line_grow);
            const int n = b.w * b.h;
            for (int idx = lane_id & 15; idx < n; idx += 16) {
                const int dr = idx / b.w;
                const int r = b.r0 + dr, cc = b.c0 + (idx - dr * b.w);
                unsigned bits = 0u;
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    float x, y;
                    md_td_window(v.px, v.py, v.hc, v.hs, R, v.m, (float)r + 0.25f + 0.5f * (float)(u >> 1), (float)cc + 0.25f + 0.5f * (float)(u & 1), &x, &y);
                    if (md_td_on_line(q, hw, x, y)) bits |= 2u << (2 * u);
                }
                const int pix = r * R + cc;
                if (bits) atomicOr(&road[pix >> 2], bits << (8 * (pix & 3)));
            }
        }
        wave_lds_sync();      // the list is rewritten by the next pass
    }
#endif
#if !(MD_TD_SKIP & 4)
    // ---- traffic(t): the drawn movers (64 culled per wave and pass), pixel centres ----
    for (int j0 = wave * 64; j0 < c.cap; j0 += 4 * 64) {
        bool keep = false;
        MdShape mine = ego;
        if (j0 + lane_id < c.cap) {
            mine = g.shape[b0 + j0 + lane_id];
            const float dx = mine.cx - v.px, dy = mine.cy - v.py, reach = md_fabs(mine.hl) + md_fabs(mine.hw) + rwin;
            keep = md_td_drawn(mine.flags, j0 + lane_id) && dx * dx + dy * dy <= reach * reach;
        }
        unsigned long long mask = __ballot(keep);
        while (mask) {
            const int k = __ffsll((long long)mask) - 1;
            mask &= mask - 1ull;
            MdShape o;
            o.cx = bcast_f(mine.cx, k); o.cy = bcast_f(mine.cy, k); o.c = bcast_f(mine.c, k); o.s = bcast_f(mine.s, k);
            o.hl = bcast_f(mine.hl, k); o.hw = bcast_f(mine.hw, k); o.flags = bcast_i(mine.flags, k); o.aux = 0;
            float oc, os;
            md_td_snap(o.c, o.s, &oc, &os);
            float pts[8];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const float sl = (i == 0 || i == 3) ? o.hl : -o.hl, sw = (i < 2) ? o.hw : -o.hw;
                pts[2 * i] = o.cx + sl * oc - sw * os;
                pts[2 * i + 1] = o.cy + sl * os + sw * oc;
            }
            const TdBox b = td_bbox(v, pts, 1);
            const int n = b.w * b.h;
            for (int idx = lane_id; idx < n; idx += 64) {
                const int dr = idx / b.w;
                const int r = b.r0 + dr, cc = b.c0 + (idx - dr * b.w);
                float x, y;
                md_td_window(v.px, v.py, v.hc, v.hs, R, v.m, (float)r + 0.5f, (float)cc + 0.5f, &x, &y);
                if (md_td_in_box(&o, x, y)) atomicOr(&traffic[r * wpr + (cc >> 5)], 1u << (cc & 31));
            }
        }
    }
#endif
    // ---- past_pos: the position ring moves on, one dot per stacked position ----
    const int pcur = reset ? 0 : (pcur_old + 1) % Lp;
    const int pcnt = reset ? 1 : (pcnt_old + 1 > Lp ? Lp : pcnt_old + 1);
    float* ring_pos = td.ring_pos + (size_t)e * (size_t)Lp * 2;
    if (tid == 0) {
        ring_pos[2 * pcur] = v.px;
        ring_pos[2 * pcur + 1] = v.py;
    }
    if (tid < md_td_stack_count(pcnt, td.frame_skip)) {
        const int back = pcnt - 1 - md_td_stack_index(pcnt, td.frame_skip, tid);    // positions back from the newest: tid * skip < pcnt
        float ox = v.px, oy = v.py;
        if (back > 0) {      // a slot an earlier launch wrote (back < Lp: never the slot written above)
            const int slot = (pcur + Lp - back) % Lp;
            ox = ring_pos[2 * slot];
            oy = ring_pos[2 * slot + 1];
        }
        float sc, ss;
        md_td_snap(v.hc, v.hs, &sc, &ss);
        int row, col;
        if (md_td_past_dot(ox, oy, v.px, v.py, sc, ss, R, td.distance, &row, &col)) atomicOr(&past[row * wpr + (col >> 5)], 1u << (col & 31));
    }
    __syncthreads();

    // ---- the traffic ring moves on: the newest frame into its slot (every slot on a reset observation) ----
    const int tcur = reset ? 0 : (tcur_old + 1) % Lt;
    uint32_t* ring = td.ring_traffic + (size_t)e * (size_t)Lt * (size_t)FW;
    for (int i = tid; i < FW; i += 256) {
        const uint32_t word = traffic[i];
        if (reset) {
            for (int sl = 0; sl < Lt; ++sl) ring[(size_t)sl * FW + i] = word;
        } else {
            ring[(size_t)tcur * FW + i] = word;
        }
    }
    // the older frames the epilogue reads (slots earlier launches wrote), into LDS with coalesced loads
    if (!reset)
        for (int i = tid; i < staged * FW; i += 256) {
            const int f = i / FW;
            stage[i] = ring[(size_t)((tcur + Lt - (f + 1) * td.frame_skip) % Lt) * FW + (i - f * FW)];
        }
    __syncthreads();
    // ---- epilogue: compose and write the env's block ----
    const int C = 2 + td.frame_stack, n = R * R * C;
    typedef typename std::conditional<NORM, float, uint8_t>::type T;
    const T t_on = NORM ? (T)md_td_traffic_float() : (T)md_td_traffic_byte();
    const T p_on = NORM ? (T)1.0f : (T)255;
    // the value of channel ch of pixel pix = (r, cc)
    auto value = [&](int pix, int r, int cc, int ch) -> T {
        if (ch == 0) {
            const unsigned byte = (road[pix >> 2] >> (8 * (pix & 3))) & 0xFFu;
            int sum4 = 0;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const unsigned code = (byte >> (2 * k)) & 3u;
                sum4 += (code & 2u) ? MD_TD_LINE : ((code & 1u) ? MD_TD_NAV : 0);
            }
            return NORM ? (T)md_td_road_float(sum4) : (T)md_td_road_byte(sum4);
        }
        const int wi = r * wpr + (cc >> 5);
        uint32_t word;
        if (ch == 1) word = past[wi];
        else if (ch == 2 || reset) word = traffic[wi];
        else if (staged) word = stage[(ch - 3) * FW + wi];
        else word = ring[(size_t)((tcur + Lt - (ch - 2) * td.frame_skip) % Lt) * FW + wi];    // a slot of an earlier launch: (ch - 2) * skip < Lt
        return ((word >> (cc & 31)) & 1u) ? (ch == 1 ? p_on : t_on) : (T)0;
    };
    T* out = (T*)td.out + (size_t)e * (size_t)n;
    constexpr int VE = 16 / (int)sizeof(T);
#if !(MD_TD_SKIP & 8)
    if (vec) {      // n * sizeof(T) is a multiple of 16 and td.out is 16-byte aligned: so is every env's block
        md_u32x4* out4 = reinterpret_cast<md_u32x4*>(out);
        for (int q = tid; q < n / VE; q += 256) {      // consecutive lanes, consecutive 16 bytes
            int pix = (q * VE) / C, ch = q * VE - pix * C;
            int r = pix / R, cc = pix - r * R;
            union { md_u32x4 q4; T t[VE]; } u;
#pragma unroll
            for (int j = 0; j < VE; ++j) {
                u.t[j] = value(pix, r, cc, ch);
                if (++ch == C) {
                    ch = 0;
                    ++pix;
                    if (++cc == R) {
                        cc = 0;
                        ++r;
                    }
                }
            }
            __builtin_nontemporal_store(u.q4, &out4[q]);
        }
    } else {
        for (int i = tid; i < n; i += 256) {
            const int pix = i / C, r = pix / R;
            out[i] = value(pix, r, pix - r * R, i - pix * C);
        }
    }
#endif
    if (tid == 0) {      // every thread read the cursors before the first barrier
        cursor[0] = tcur;
        cursor[1] = pcur;
        cursor[2] = reset ? 0 : pcnt;     // the reference clears stack_past_pos after the reset observation's dot is drawn
        cursor[3] = 0;
    }
}

}  // namespace
