// parts/render.inc -- part of mdstep.hip, included there and not compiled on its own.
// Provides: the LDS layout render_lds, render_push_kernel and render_kernel (include/md_render.h),
// and the entry point md_render with its argument checks.
// Relies on: mdstep.hip (align_up, bcast_*, wave_lds_sync, QuadBall, quad_ball_of), entry_checks.

namespace {

// ---- md_render (include/md_render.h): env.render(mode="topdown"), one workgroup per (tile, rendered env) ----------------------
// A tile is MD_RD_TILE x MD_RD_TILE pixels, one LDS word each.  The word holds a RANK, not a colour: 0 the white ground, 1 .. 3 the
// line kinds in their order, 4 + 2 * (k * cap + slot) + contour the box of `slot` in held frame k.  Ranks grow along the painter's
// order, so every primitive is rasterised over its own bounding box in the tile with an LDS atomicMax and no order between
// primitives is needed; the epilogue turns ranks into colours (the faded colour of every (frame, slot) sits in an LDS table) and
// writes the tile's rows.  Nothing here depends on the order in which waves run: the image is a function of the ring alone.
struct RenderLds { uint32_t pix, palette, pieces, kinds, bytes; };
__host__ __device__ constexpr RenderLds render_lds(int num_stack, int cap) {
    const uint32_t palette = 4u * MD_RD_TILE * MD_RD_TILE;
    const uint32_t pieces = palette + align_up(4u * (uint32_t)num_stack * (uint32_t)cap, 16);      // written with 16-byte LDS stores
    const uint32_t kinds = pieces + 4u * 64u * 32u;
    return RenderLds{0u, palette, pieces, kinds, kinds + 4u * 64u * 4u};
}

// the launch before the raster: the current boxes into the ring of every rendered env, its cursor moved on
__global__ __launch_bounds__(MD_MAX_CAP) void render_push_kernel(const MdState g, const MdConfig c, const MdRender r) {
    const int ri = blockIdx.x, j = threadIdx.x;
    int e = r.env_ids[ri];
    e = e < 0 ? 0 : (e >= c.n_envs ? c.n_envs - 1 : e);
    const size_t b0 = (size_t)e * (size_t)c.cap;
    int32_t* cursor = r.cursor + 4 * (size_t)ri;
    const int clock = md_rd_clock(&g, &c, e, &g.nav[b0]);
    int newest, held;
    md_rd_advance(cursor, r.num_stack, clock, &newest, &held);
    __syncthreads();      // every thread has read the cursors
    if (j < c.cap) r.ring[((size_t)ri * (size_t)r.num_stack + (size_t)newest) * (size_t)c.cap + j] = md_rd_box_of(&g.shape[b0 + j], j);
    if (j == 0) {
        cursor[0] = newest;
        cursor[1] = held;
        cursor[2] = clock;
        cursor[3] = 0;
    }
}

struct RdView { float px, py, uc, us, scaling; int W, H, r0, c0, th, tw; };      // the window, and this workgroup's tile of it
struct RdBox { int r0, c0, w, h; };                                              // in the tile's own rows and columns

// the pixels of the tile that can hold the centre of a sample of the convex hull of the four world points xy, grown by `grow` pixels
__device__ __forceinline__ RdBox rd_bbox(const RdView& v, const float* xy, int grow) {
    float rmin = 3.0e38f, rmax = -3.0e38f, cmin = 3.0e38f, cmax = -3.0e38f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const float dx = xy[2 * i] - v.px, dy = xy[2 * i + 1] - v.py;
        const float fr = 0.5f * (float)v.H - (dx * v.uc + dy * v.us) * v.scaling;
        const float fc = 0.5f * (float)v.W + (dx * v.us - dy * v.uc) * v.scaling;
        rmin = md_min(rmin, fr); rmax = md_max(rmax, fr);
        cmin = md_min(cmin, fc); cmax = md_max(cmax, fc);
    }
    const float lo = -8.0f, hr = (float)v.H + 8.0f, hc = (float)v.W + 8.0f;     // keeps the conversions to int in range (NaN -> lo)
    const int r0 = (int)md_floor(md_clip(rmin, lo, hr)) - grow - v.r0, r1 = (int)md_floor(md_clip(rmax, lo, hr)) + grow - v.r0;
    const int c0 = (int)md_floor(md_clip(cmin, lo, hc)) - grow - v.c0, c1 = (int)md_floor(md_clip(cmax, lo, hc)) + grow - v.c0;
    RdBox b;
    b.r0 = r0 < 0 ? 0 : r0;
    b.c0 = c0 < 0 ? 0 : c0;
    const int r1c = r1 > v.th - 1 ? v.th - 1 : r1, c1c = c1 > v.tw - 1 ? v.tw - 1 : c1;
    b.h = r1c >= b.r0 ? r1c - b.r0 + 1 : 0;
    b.w = c1c >= b.c0 ? c1c - b.c0 + 1 : 0;
    return b;
}

__global__ __launch_bounds__(256) void render_kernel(const MdWorld w, const MdState g, const MdConfig c, const MdRender r, const int tiles_x,
                                                     const int vec) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int ri = blockIdx.y, tid = threadIdx.x, lane_id = tid & 63, wave = tid >> 6;
    const RenderLds lds = render_lds(r.num_stack, c.cap);
    uint32_t* pix = reinterpret_cast<uint32_t*>(smem + lds.pix);
    uint32_t* palette = reinterpret_cast<uint32_t*>(smem + lds.palette);
    float* pieces = reinterpret_cast<float*>(smem + lds.pieces) + wave * 64 * 8;
    int* kinds = reinterpret_cast<int*>(smem + lds.kinds) + wave * 64;
    for (int i = tid; i < MD_RD_TILE * MD_RD_TILE; i += 256) pix[i] = 0u;

    int e = r.env_ids[ri];
    e = e < 0 ? 0 : (e >= c.n_envs ? c.n_envs - 1 : e);
    const size_t b0 = (size_t)e * (size_t)c.cap;
    const MdShape tracked = g.shape[b0 + r.track_agent];
    RdView v;
    md_rd_camera(&r, &tracked, &v.px, &v.py, &v.uc, &v.us);
    v.scaling = r.scaling; v.W = r.width; v.H = r.height;
    const int ty = blockIdx.x / tiles_x;
    v.r0 = ty * MD_RD_TILE;
    v.c0 = (blockIdx.x - ty * tiles_x) * MD_RD_TILE;
    v.th = min(MD_RD_TILE, v.H - v.r0);
    v.tw = min(MD_RD_TILE, v.W - v.c0);
    // the tile's circumscribed circle, with a margin of two pixels
    float tcx, tcy;
    md_rd_window(v.px, v.py, v.uc, v.us, v.W, v.H, v.scaling, (float)v.r0 + 0.5f * (float)v.th, (float)v.c0 + 0.5f * (float)v.tw, &tcx, &tcy);
    const float rtile = (0.70711f * (float)MD_RD_TILE + 2.0f) / v.scaling;
    const int32_t* cursor = r.cursor + 4 * (size_t)ri;      // as render_push_kernel left them
    const int newest = (int)((uint32_t)cursor[0] % (uint32_t)r.num_stack);
    const int held = cursor[1] < 1 ? 1 : (cursor[1] > r.num_stack ? r.num_stack : cursor[1]);
    int map = w.env_map[e];
    if (map < 0 || map >= w.n_maps) map = 0;
    __syncthreads();

    // ---- the map's line pieces: 64 culled per wave and pass, then 16 lanes to a piece ----
    const float hw = md_rd_line_half_width(v.scaling);
    const int line_grow = 2 + (int)(hw * v.scaling);      // a sample on the strip lies within hw of the piece's own extent
    const int qa = w.quad_off[map], qb = w.quad_off[map + 1];
    for (int q0 = qa + wave * 64; q0 < qb; q0 += 4 * 64) {
        bool keep = false;
        int order = 0;
        if (q0 + lane_id < qb) {
            const QuadBall qbl = quad_ball_of(w, q0 + lane_id);
            const float dx = qbl.mx - tcx, dy = qbl.my - tcy, reach = qbl.rr + rtile + hw;
            order = md_rd_line_order(qbl.kind);
            keep = order != 0 && dx * dx + dy * dy <= reach * reach;
        }
        const unsigned long long mask = __ballot(keep);
        const int kept = __popcll(mask);
        if (keep) {
            const int at = __popcll(mask & ((1ull << lane_id) - 1ull));
            const float4* qp = reinterpret_cast<const float4*>(w.quads) + 2 * (size_t)(q0 + lane_id);
            float4* dst = reinterpret_cast<float4*>(pieces) + 2 * at;
            dst[0] = qp[0];
            dst[1] = qp[1];
            kinds[at] = order;
        }
        wave_lds_sync();
        for (int k = lane_id >> 4; k < kept; k += 4) {
            float q[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) q[i] = pieces[8 * k + i];
            const unsigned rank = (unsigned)kinds[k];
            const RdBox b = rd_bbox(v, q, line_grow);
            const int n = b.w * b.h;
            for (int idx = lane_id & 15; idx < n; idx += 16) {
                const int dr = idx / b.w;
                const int lr = b.r0 + dr, lc = b.c0 + (idx - dr * b.w);
                float x, y;
                md_rd_window(v.px, v.py, v.uc, v.us, v.W, v.H, v.scaling, (float)(v.r0 + lr) + 0.5f, (float)(v.c0 + lc) + 0.5f, &x, &y);
                if (md_td_on_line(q, hw, x, y)) atomicMax(&pix[lr * MD_RD_TILE + lc], rank);
            }
        }
        wave_lds_sync();      // the list is rewritten by the next pass
    }

    // ---- the movers of every held frame: item i = (frame k, slot), 64 culled per wave and pass, then the wave on each kept box ----
    const int n_items = held * c.cap;
    const float cw = MD_RD_CONTOUR_PIXELS / v.scaling;
    for (int i0 = wave * 64; i0 < n_items; i0 += 4 * 64) {
        bool keep = false;
        MdShape mine = tracked;
        const int i = i0 + lane_id;
        if (i < n_items) {
            const int k = i / c.cap, slot = i - k * c.cap;
            mine = r.ring[((size_t)ri * (size_t)r.num_stack + (size_t)md_rd_ring_slot(newest, r.num_stack, held, k)) * (size_t)c.cap + slot];
            if (mine.flags != 0 && !md_rd_frame_skipped(held, k, r.history_smooth)) {
                palette[i] = (uint32_t)md_rd_fade(mine.aux, md_rd_alpha(held, k));
                const float dx = mine.cx - tcx, dy = mine.cy - tcy, reach = md_fabs(mine.hl) + md_fabs(mine.hw) + rtile;
                keep = dx * dx + dy * dy <= reach * reach;
            }
        }
        unsigned long long mask = __ballot(keep);
        while (mask) {
            const int src = __ffsll((long long)mask) - 1;
            mask &= mask - 1ull;
            MdShape o;
            o.cx = bcast_f(mine.cx, src); o.cy = bcast_f(mine.cy, src); o.c = bcast_f(mine.c, src); o.s = bcast_f(mine.s, src);
            o.hl = bcast_f(mine.hl, src); o.hw = bcast_f(mine.hw, src); o.flags = bcast_i(mine.flags, src); o.aux = 0;
            const int item = i0 + src;
            const bool contour = r.draw_contour && item / c.cap == held - 1;
            float oc, os;
            md_td_snap(o.c, o.s, &oc, &os);
            float pts[8];
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const float sl = (t == 0 || t == 3) ? o.hl : -o.hl, sw = (t < 2) ? o.hw : -o.hw;
                pts[2 * t] = o.cx + sl * oc - sw * os;
                pts[2 * t + 1] = o.cy + sl * os + sw * oc;
            }
            const RdBox b = rd_bbox(v, pts, 1);
            const int n = b.w * b.h;
            for (int idx = lane_id; idx < n; idx += 64) {
                const int dr = idx / b.w;
                const int lr = b.r0 + dr, lc = b.c0 + (idx - dr * b.w);
                float x, y;
                md_rd_window(v.px, v.py, v.uc, v.us, v.W, v.H, v.scaling, (float)(v.r0 + lr) + 0.5f, (float)(v.c0 + lc) + 0.5f, &x, &y);
                if (md_td_in_box(&o, x, y)) {
                    const unsigned edge = (contour && md_rd_on_contour(&o, cw, x, y)) ? 1u : 0u;
                    atomicMax(&pix[lr * MD_RD_TILE + lc], 4u + 2u * (unsigned)item + edge);
                }
            }
        }
    }
    __syncthreads();

    // ---- epilogue: ranks to colours, in place; then the tile's rows ----
    for (int p = tid; p < MD_RD_TILE * MD_RD_TILE; p += 256) {
        const uint32_t rank = pix[p];
        pix[p] = rank == 0u ? (uint32_t)MD_RD_WHITE
                            : (rank < 4u ? (uint32_t)md_rd_line_rgb((int)rank) : ((rank & 1u) ? (uint32_t)MD_RD_CONTOUR_RGB : palette[(rank - 4u) >> 1]));
    }
    __syncthreads();
    uint8_t* out = r.out + (((size_t)ri * (size_t)v.H + (size_t)v.r0) * (size_t)v.W + (size_t)v.c0) * 3;      // the tile's first byte
    const int row_bytes = v.tw * 3;
    auto byte_of = [&](int lr, int b) -> uint32_t {
        const int p = b / 3;
        return (pix[lr * MD_RD_TILE + p] >> (8 * (b - 3 * p))) & 255u;
    };
    if (vec) {      // W is a multiple of 16 and r.out 16-byte aligned: so are every tile row's first byte and length
        const int cpr = row_bytes >> 4;
        for (int q = tid; q < v.th * cpr; q += 256) {      // consecutive lanes, consecutive 16 bytes of a row
            const int lr = q / cpr, b = (q - lr * cpr) << 4;
            md_u32x4 t;
#pragma unroll
            for (int j = 0; j < 4; ++j)
                t[j] = byte_of(lr, b + 4 * j) | (byte_of(lr, b + 4 * j + 1) << 8) | (byte_of(lr, b + 4 * j + 2) << 16) | (byte_of(lr, b + 4 * j + 3) << 24);
            __builtin_nontemporal_store(t, reinterpret_cast<md_u32x4*>(out + (size_t)lr * (size_t)v.W * 3 + b));
        }
    } else {
        for (int q = tid; q < v.th * row_bytes; q += 256) {
            const int lr = q / row_bytes, b = q - lr * row_bytes;
            out[(size_t)lr * (size_t)v.W * 3 + b] = (uint8_t)byte_of(lr, b);
        }
    }
}

}  // namespace

extern "C" {

__attribute__((visibility("default"))) int md_render(const MdWorld* w, const MdState* s, const MdConfig* c, const MdRender* r, void* stream) {
    TRY(check_common(w, s, c));
    NEED(r);
    TRY(check_arg_size("MdRender", r->struct_size, sizeof(MdRender)));
    NEED(r->env_ids); NEED(r->out); NEED(r->ring); NEED(r->cursor);
    TRY(need_fields(kRenderEntry, ALWAYS | MULTI, w, s, c));
    if (r->n_render < 1 || r->n_render > 65535) {
        snprintf(g_err, sizeof g_err, "md_render: n_render=%d must lie in [1, 65535]", r->n_render);
        return MD_EINVAL;
    }
    if (r->width < 1 || r->height < 1 || r->width > MD_RD_MAX_SIZE || r->height > MD_RD_MAX_SIZE) {
        snprintf(g_err, sizeof g_err, "md_render: width=%d height=%d must lie in [1, MD_RD_MAX_SIZE=%d]", r->width, r->height, MD_RD_MAX_SIZE);
        return MD_EINVAL;
    }
    if (!(r->scaling > 0.0f) || !(r->scaling <= 3.0e38f)) {
        snprintf(g_err, sizeof g_err, "md_render: scaling=%g must be positive and finite", (double)r->scaling);
        return MD_EINVAL;
    }
    if (r->num_stack < 1 || r->num_stack > MD_RD_MAX_STACK) {
        snprintf(g_err, sizeof g_err, "md_render: num_stack=%d must lie in [1, MD_RD_MAX_STACK=%d]", r->num_stack, MD_RD_MAX_STACK);
        return MD_EINVAL;
    }
    if (r->history_smooth < 0) {
        snprintf(g_err, sizeof g_err, "md_render: history_smooth=%d must not be negative", r->history_smooth);
        return MD_EINVAL;
    }
    if (r->track_agent < 0 || r->track_agent >= c->agents_per_env) {
        snprintf(g_err, sizeof g_err, "md_render: track_agent=%d is no agent slot (agents_per_env=%d)", r->track_agent, c->agents_per_env);
        return MD_EINVAL;
    }
    if (((uintptr_t)w->quads & 15) || ((uintptr_t)w->quad_ball & 15)) {     // read as float4 (quad_ball may be NULL)
        snprintf(g_err, sizeof g_err, "md_render: MdWorld.%s must be 16-byte aligned", ((uintptr_t)w->quads & 15) ? "quads" : "quad_ball");
        return MD_EINVAL;
    }
    if (w->n_maps <= 0) {
        snprintf(g_err, sizeof g_err, "md_render: MdWorld.n_maps=%d", w->n_maps);
        return MD_EINVAL;
    }
    const int tiles_x = (r->width + MD_RD_TILE - 1) / MD_RD_TILE, tiles_y = (r->height + MD_RD_TILE - 1) / MD_RD_TILE;
    const int vec = (r->width % 16 == 0) && (((uintptr_t)r->out & 15) == 0);
    hipLaunchKernelGGL(render_push_kernel, dim3(r->n_render), dim3(MD_MAX_CAP), 0, (hipStream_t)stream, *s, *c, *r);
    hipLaunchKernelGGL(render_kernel, dim3(tiles_x * tiles_y, r->n_render), dim3(256), render_lds(r->num_stack, c->cap).bytes, (hipStream_t)stream,
                       *w, *s, *c, *r, tiles_x, vec);
    return launch_status();
}

}  // extern "C"
