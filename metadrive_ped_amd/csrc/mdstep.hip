// mdstep.hip -- gfx950 (MI355X / CDNA4) kernels + C-ABI launchers of the batched MetaDrive step().
//
// One workgroup (256 threads = 4 wave64) owns one environment for the whole step; phases are
// separated by workgroup barriers and never talk to other workgroups, so a step is ONE launch with
// no inter-workgroup traffic, no atomics and no grid-level synchronisation:
//
//   reset -> IDM(+trigger) -> integrate -> localize -> contacts -> traffic removal -> observe -> lidar
//
// Work shapes (wave64-native, none of this is a warp-32 tiling):
//   * lidar     : one wave per (agent, 64-beam sector).  Each LANE first loads ONE mover record
//                 (32 B, coalesced), culls it against range + the sector's cone, the survivors are
//                 collected with a 64-bit ballot and broadcast lane->wave with v_readlane; each lane
//                 then tests ITS beam against the surviving shapes.  No LDS, no atomics.
//   * localize  : one wave per vehicle; candidate lanes come from the static grid cell under the
//                 vehicle; the convex-hull containment test spreads hull edges over the 64 lanes and
//                 votes with a ballot.
//   * contacts  : one wave per vehicle; lanes = the other movers (SAT each), then lanes = quads of
//                 the grid cells under the chassis AABB; flag words are OR-combined by ballots.
//   * trigger   : wavefront min-reduce (DPP shuffles) over the pending traffic blocks.
//   * integrate / observe / IDM : one thread per entity over include/md_entity.h.
//
// There is no dense contraction on the step path, hence no MFMA there; the one exception is md_expert (the PPO expert's
// MLP, include/md_expert.h), which runs on v_mfma_f32_16x16x4_f32.  The arithmetic formulas are the shared
// include/md_geom.h / md_entity.h ones (bit-exact vs the CPU oracle, -ffp-contract=off).
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <type_traits>

#include "md_curriculum.h"
#include "md_expert.h"
#include "md_expert_sense.h"
#include "md_ai_protect.h"
#include "md_scenario.h"
#include "md_topdown.h"
#include "md_render.h"
#include "md_branch.h"
#include "md_ped.h"
#include "md_vector_obs.h"

namespace {

constexpr int kBlock = 256;  // block size of the auxiliary kernels; env_kernel is templated on its own

enum Phase : int {
    PH_RESET = 1,
    PH_IDM = 2,
    PH_INTEGRATE = 4,
    PH_LOCALIZE = 8,
    PH_CONTACTS = 16,
    PH_TRAFFIC = 32,
    PH_OBSERVE = 64,
    PH_LIDAR = 128,
    PH_LIFECYCLE = 256,
    PH_ALL = 511,
    // md_localize_road_first: PH_LOCALIZE whose localize_vehicle tries the road-first path (a bit above every entry-point mask)
    PH_LOCALIZE_ROAD_FIRST = PH_LOCALIZE | (1 << 20),
};

thread_local char g_err[256] = "ok";

// In-kernel phase stamps: DIAGNOSTIC BUILD ONLY (-DMD_STAMP, tools/stamp_profile.py).  The stamp
// values go to a buffer of their own that no kernel code reads; the production build contains none.
#ifdef MD_STAMP
__device__ unsigned long long* g_stamp_buf = nullptr;
__device__ const int* g_env_order = nullptr;
// slots 0..11: shader-cycle stamps; 12 / 13: s_memrealtime (100 MHz, one time base for the whole chip) at the first / last
// stamp; 14: HW_ID | XCC_ID << 32 (which CU the workgroup ran on) -- tools/timeline_probe.py rebuilds the occupancy timeline;
// 15 (fine slot -1) / fine slot 14: start / end of the trigger's search (trigger_search_wave)
#define MD_STAMP_AT(i)                                                                         \
    do {                                                                                       \
        if (threadIdx.x == 0 && g_stamp_buf) {                                                 \
            unsigned long long* sb_ = g_stamp_buf + (size_t)blockIdx.x * 32;                   \
            sb_[(i)] = __builtin_readcyclecounter();                                           \
            if ((i) == 0) {                                                                    \
                sb_[12] = __builtin_amdgcn_s_memrealtime();                                    \
                sb_[14] = (unsigned long long)__builtin_amdgcn_s_getreg(63492) |               \
                          ((unsigned long long)__builtin_amdgcn_s_getreg(63508) << 32);        \
            }                                                                                  \
            if ((i) == 11) sb_[13] = __builtin_amdgcn_s_memrealtime();                         \
        }                                                                                      \
    } while (0)
#define MD_FINE_STAMP(cond, i)                                                                 \
    do {                                                                                       \
        if ((cond) && g_stamp_buf) g_stamp_buf[(size_t)blockIdx.x * 32 + 16 + (i)] = __builtin_readcyclecounter(); \
    } while (0)
// fine slots 12 / 13: the workgroup's localisations so far / those the road-first path answered (tools/stamp_profile.py)
#define MD_LOC_COUNT(cond, hit)                                                                \
    do {                                                                                       \
        if ((cond) && g_stamp_buf) {                                                           \
            atomicAdd(&g_stamp_buf[(size_t)blockIdx.x * 32 + 16 + 12], 1ull);                  \
            if (hit) atomicAdd(&g_stamp_buf[(size_t)blockIdx.x * 32 + 16 + 13], 1ull);         \
        }                                                                                      \
    } while (0)
#else
#define MD_STAMP_AT(i) do { } while (0)
#define MD_FINE_STAMP(cond, i) do { } while (0)
#define MD_LOC_COUNT(cond, hit) do { } while (0)
#endif
// Diagnostic builds only (tools/ab/env_knockout.sh): stages of the fused env kernel left out to read their marginal cost off the
// launch time.  0 in the product.
#ifndef MD_ENV_SKIP
#define MD_ENV_SKIP 0
#endif

// LDS images: every kernel with dynamic LDS has ONE layout function (<kernel>_lds below) that both its launcher (for the size)
// and the kernel (to carve smem) call.  Offsets are in bytes from the start of the dynamic LDS, which is 16-B aligned.
__host__ __device__ constexpr uint32_t align_up(uint32_t b, uint32_t a) { return (b + a - 1) & ~(a - 1); }

__device__ __forceinline__ float bcast_f(float v, int src) { return __shfl(v, src, 64); }
__device__ __forceinline__ int bcast_i(int v, int src) { return __shfl(v, src, 64); }

// One wave's LDS hand-over: what its lanes wrote before is visible to all of its lanes after.  The LDS unit executes a wave's
// ds_write / ds_read in order; the fences keep the compiler from moving reads above the other lanes' writes.
__device__ __forceinline__ void wave_lds_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// The env state is read once and written once per step: streaming accesses (the nt hint keeps them from displacing the map
// tables -- read again next step by the same env, on the same XCD -- from L2).  Measured: workgroup kernel 88.6 -> 86.7 us,
// wave kernel on 4096 distinct maps 93.5 -> 89.0 us (-DMD_NT_STAGE=0 switches the hint off).
#ifndef MD_NT_STAGE
#define MD_NT_STAGE 1
#endif
typedef unsigned int md_u32x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ uint4 ld_stream(const uint4* p) {
#if MD_NT_STAGE
    const md_u32x4 v = __builtin_nontemporal_load(reinterpret_cast<const md_u32x4*>(p));
    return make_uint4(v.x, v.y, v.z, v.w);
#else
    return *p;
#endif
}
__device__ __forceinline__ void st_stream(uint4* p, const uint4 v) {
#if MD_NT_STAGE
    md_u32x4 t;
    t.x = v.x; t.y = v.y; t.z = v.z; t.w = v.w;
    __builtin_nontemporal_store(t, reinterpret_cast<md_u32x4*>(p));
#else
    *p = v;
#endif
}
__device__ __forceinline__ void st_stream_f(float* p, float v) {
#if MD_NT_STAGE
    __builtin_nontemporal_store(v, p);
#else
    *p = v;
#endif
}

// Wavefront min-reduce over the lanes whose `valid` is set; returns `none` when no lane is valid.
// Built from a 64-bit ballot + v_readlane walks over the set bits: on gfx950 __shfl_xor lowers to
// ds_bpermute (an LDS-crossbar round trip of ~100+ cycles per step), and the candidate sets here are
// sparse (a handful of lanes), so walking the ballot is several times faster than a 6-step butterfly.
__device__ __forceinline__ int wave_min_i(int v, bool valid, int none) {
    unsigned long long m = __ballot(valid);
    int best = none;
    while (m) {
        const int l = __ffsll((long long)m) - 1;
        m &= m - 1;
        const int o = __shfl(v, l, 64);
        best = o < best ? o : best;
    }
    return best;
}

// ------------------------------------------------------------------------------------------------
// Lidar for one (agent, sector) work item, executed by one wave.
// ------------------------------------------------------------------------------------------------
// det: LDS words [2] of agent a's detected set (nullptr = not tracked)
// kLdsRow: out_row is a row in LDS (md_expert_sense): a plain store instead of the streaming one meant for HBM
template <bool kLdsRow = false>
__device__ __forceinline__ void lidar_item(const MdWorld& w, const MdState& s, const MdConfig& c, int a, int sec, int lane,
                           float* __restrict__ out_row, unsigned long long* det) {
    const MdShape me = s.shape[a];  // wave-uniform (s is the env-local, LDS-staged view)
    const int beam = sec * 64 + lane;
    const bool valid = beam < c.n_beams;
    if (!md_present(me.flags)) {
        if (valid) out_row[beam] = 1.0f;
        return;
    }
    float bc = 1.0f, bs = 0.0f;
    if (valid) {
        bc = w.beam_cs[2 * beam];
        bs = w.beam_cs[2 * beam + 1];
    }
    const float dirx = (bc * me.c - bs * me.s) * c.lidar_range;
    const float diry = (bs * me.c + bc * me.s) * c.lidar_range;

    // Sector cone for culling: axis = middle of the sector's beam fan, half-span h.  The cull is only ever
    // CONSERVATIVE (2e-3 slack on the cosine, 1 cm on the radii), so it runs on the hardware's approximate
    // rcp / rsq / sqrt / sin / cos (1 ulp, v_sin/v_cos take revolutions); the cast below stays exact.
    const int nb = min(64, c.n_beams - sec * 64);
    const float inv_n = __builtin_amdgcn_rcpf((float)c.n_beams);
    const float mid_rev = ((float)(sec * 64) + 0.5f * (float)(nb - 1)) * inv_n;   // axis angle, in revolutions, ego frame
    const float half_rev = 0.5f * (float)(nb - 1) * inv_n;
    const float ax = __builtin_amdgcn_cosf(mid_rev), ay = __builtin_amdgcn_sinf(mid_rev);
    const float cos_h = __builtin_amdgcn_cosf(half_rev), sin_h = __builtin_amdgcn_sinf(half_rev);
    const float half_span = MD_TWO_PI_F * half_rev;
    // cone test is meaningful only while h + asin(rb/dist) < pi; asin <= pi/2, so narrow sectors never need the check
    const bool narrow = half_span < MD_HALF_PI_F - 0.02f;
    const float wax = ax * me.c - ay * me.s;  // axis in world frame
    const float way = ay * me.c + ax * me.s;

    float best = 1.0f;
    int best_j = -1;  // slot of the body this beam hits first (tracked only when det != nullptr)
    for (int j0 = 0; j0 < c.cap; j0 += 64) {
        const int j = j0 + lane;
        MdShape o;
        o.flags = 0;
        if (j < c.cap) o = s.shape[j];
        bool keep = (j < c.cap) && (j != a) && md_present(o.flags);
        if (keep) {
            const float ddx = o.cx - me.cx, ddy = o.cy - me.cy;
            const float d2 = ddx * ddx + ddy * ddy;
            const int k = md_kind_of(o.flags);
            const float rb = (md_is_circle_kind(k) ? o.hl : __builtin_amdgcn_sqrtf(o.hl * o.hl + o.hw * o.hw)) + 0.01f;
            const float reach = c.lidar_range + rb;
            if (d2 > reach * reach * 1.0001f) keep = false;
            else if (d2 > rb * rb) {
                // cone test: angle(d, axis) <= h + alpha, sin(alpha) = rb / dist
                const float inv = __builtin_amdgcn_rsqf(d2);
                const float sin_a = rb * inv;
                const float cos_a = __builtin_amdgcn_sqrtf(md_max(0.0f, 1.0f - sin_a * sin_a));
                if (narrow || half_span + md_asin(md_min(sin_a, 1.0f)) < MD_PI_F - 0.01f) {
                    const float cos_lim = cos_h * cos_a - sin_h * sin_a;  // cos(h + alpha)
                    const float cos_t = (ddx * wax + ddy * way) * inv;
                    if (cos_t < cos_lim - 2e-3f) keep = false;
                }
            }
        }
        unsigned long long mask = __ballot(keep);
        while (mask) {
            const int k = __ffsll((long long)mask) - 1;
            mask &= mask - 1;
            const float ocx = bcast_f(o.cx, k), ocy = bcast_f(o.cy, k);
            const float oc = bcast_f(o.c, k), os = bcast_f(o.s, k);
            const float ohl = bcast_f(o.hl, k), ohw = bcast_f(o.hw, k);
            const int ofl = bcast_i(o.flags, k);
            const float t = md_ray_shape(me.cx, me.cy, dirx, diry, ocx, ocy, oc, os, ohl, ohw, md_kind_of(ofl));
            if (t < best) {
                best = t;
                best_j = j0 + k;  // candidates come in ascending slot order: equal fractions keep the lowest slot
            }
        }
    }
    if (valid) {
        if (kLdsRow) out_row[beam] = best;
        else st_stream_f(&out_row[beam], best);
    }
    if (det) {
        // union of the 64 beams' first hits: peel one distinct slot per iteration (<= a handful)
        unsigned long long todo = __ballot(valid && best_j >= 0);
        unsigned long long lo = 0ull, hi = 0ull;
        while (todo) {
            const int k = __ffsll((long long)todo) - 1;
            const int jj = bcast_i(best_j, k);
            todo &= ~__ballot(best_j == jj);
            if (jj < 64) lo |= 1ull << jj;
            else hi |= 1ull << (jj - 64);
        }
        if (lane == 0) {
            if (lo) atomicOr(&det[0], lo);
            if (hi) atomicOr(&det[1], hi);
        }
    }
}

// (Keeping the sectors off the wave that runs the agent's observe chain was tried: 154 vs 145 us, worse.)
// `tickets` (LDS counter, zeroed by the caller behind a barrier) = the waves take the (agent, sector) items as they get free -- the
// multi-agent kernels, whose workgroups are all resident at once so that a launch lasts as long as its slowest env; nullptr = dealt
// round-robin.  The items are independent: the order changes nothing.
__device__ __forceinline__ void phase_lidar(const MdWorld& w, const MdState& s, const MdConfig& c, int e, int tid, int kWaves,
                            float* out, int out_stride, int out_offset, unsigned long long* l_det, int* tickets = nullptr) {  // `out` is the GLOBAL output base
    const int wave = tid >> 6, lane = tid & 63;
    const int nsec = (c.n_beams + 63) >> 6;
    const int items = c.agents_per_env * nsec;
    if (tickets) {
        for (int guard = 0; guard < items; ++guard) {
            int it = 0;
            if (lane == 0) it = atomicAdd(tickets, 1);
            it = __builtin_amdgcn_readfirstlane(it);
            if (it < 0 || it >= items) break;
            const int a = it / nsec, sec = it - a * nsec;
            float* row = out + (size_t)(e * c.agents_per_env + a) * out_stride + out_offset;
            lidar_item(w, s, c, a, sec, lane, row, l_det ? l_det + 2 * a : nullptr);
        }
        return;
    }
    for (int it = wave; it < items; it += kWaves) {
        const int a = it / nsec, sec = it - a * nsec;
        float* row = out + (size_t)(e * c.agents_per_env + a) * out_stride + out_offset;
        lidar_item(w, s, c, a, sec, lane, row, l_det ? l_det + 2 * a : nullptr);
    }
}

// The detectors' cull record of quad q: centre, radius of a circle around it, kind -- from MdWorld.quad_ball (16 bytes) or,
// without that table, from the quad itself.
struct QuadBall { float mx, my, rr; int kind; };
__device__ __forceinline__ QuadBall quad_ball_of(const MdWorld& w, int q) {
    QuadBall b;
    if (w.quad_ball) {
        const float4 t = reinterpret_cast<const float4*>(w.quad_ball)[q];
        b.mx = t.x;
        b.my = t.y;
        b.rr = t.z;
        b.kind = __float_as_int(t.w);
    } else {
        const float4* quads4 = reinterpret_cast<const float4*>(w.quads);
        const float4 lo = quads4[2 * (size_t)q], hi = quads4[2 * (size_t)q + 1];
        b.mx = 0.25f * (lo.x + lo.z + hi.x + hi.z);
        b.my = 0.25f * (lo.y + lo.w + hi.y + hi.w);
        const float r2 = md_max(md_max((lo.x - b.mx) * (lo.x - b.mx) + (lo.y - b.my) * (lo.y - b.my),
                                       (lo.z - b.mx) * (lo.z - b.mx) + (lo.w - b.my) * (lo.w - b.my)),
                                md_max((hi.x - b.mx) * (hi.x - b.mx) + (hi.y - b.my) * (hi.y - b.my),
                                       (hi.z - b.mx) * (hi.z - b.mx) + (hi.w - b.my) * (hi.w - b.my)));
        b.rr = md_sqrt(r2) * 1.01f + 1.0e-3f;
        b.kind = w.quad_kind[q];
    }
    return b;
}

// One detector fan of one agent against the quads [qa, qb) of its map by ONE wave, in two phases so that the expensive
// slab tests run on full wavefronts: (1) lanes = quads: kind, reach, then every beam against the quad's bounding circle
// (a dozen instructions); the (quad, beam) pairs that survive -- a few per hundred -- are appended to `pairs` (LDS,
// kDetPairs ints of this wave) through ballot prefix counts; (2) lanes = pairs: fetch the quad, cast, atomicMin on the
// fraction's bit pattern in `best` (initialised to 1.0).  The list is drained whenever a pass could overflow it.  Same
// arithmetic and the same minima as line_detector_kernel and the oracle's serial loop.
constexpr int kDetPairs = 512;
__device__ __forceinline__ void detector_drain(const MdWorld& w, const MdShape& me, const float* beam_cs, float range, const int* pairs, int n,
                               int qa, int* best, int lane_id) {   // a pair = (quad - qa) << 8 | beam
    const float4* quads4 = reinterpret_cast<const float4*>(w.quads);
    for (int k = lane_id; k < n; k += 64) {
        const int pr = pairs[k];
        const int q = qa + (pr >> 8), i = pr & 255;
        const float4 lo = quads4[2 * (size_t)q], hi = quads4[2 * (size_t)q + 1];
        const float v[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
        const float bc = beam_cs[2 * i], bs = beam_cs[2 * i + 1];
        const float ux = bc * me.c - bs * me.s, uy = bs * me.c + bc * me.s;
        const float t = md_ray_quad(me.cx, me.cy, ux * range, uy * range, v);
        if (t < 1.0f) atomicMin(&best[i], __float_as_int(t));
    }
}

// is the table a uniform fan?  beam i = (cos, sin)(phase0 + i 2 pi / n): one lane per beam compares
__device__ __forceinline__ bool detector_uniform_fan(const float* beam_cs, int n_beams, int lane_id, float* phase0_out) {
    const float phase0 = atan2f(beam_cs[1], beam_cs[0]);
    const float dphi = 6.283185307179586f / (float)n_beams;
    bool fan_ok = true;
    for (int i = lane_id; i < n_beams; i += 64) {
        float sn, cs;
        sincosf(phase0 + (float)i * dphi, &sn, &cs);
        fan_ok = fan_ok && md_fabs(cs - beam_cs[2 * i]) < 1.0e-3f && md_fabs(sn - beam_cs[2 * i + 1]) < 1.0e-3f;
    }
    *phase0_out = phase0;
    return __ballot(!fan_ok) == 0ull && n_beams >= 4;
}

// Which beams can meet a quad at all?  For a uniform fan (beam i at phase0 + i dphi from the heading -- every detector table
// is one; the callers check, else all beams are tried) only those within asin(r / d) of the direction to the quad's centre
// (px, py from the agent, circle radius rr): a handful instead of all 12 ... 72, n_try of them from beam i_lo on, cyclically.
// Hardware atan2 / asin are good enough here, a margin covers them and the exact circle test follows anyway.  An agent
// inside the circle keeps the all-beams window that the caller set.
__device__ __forceinline__ void detector_beam_window(const MdShape& me, float px, float py, float rr, float phase0, float inv_dphi,
                                                     int n_beams, int& i_lo, int& n_try) {
    const float d2 = px * px + py * py;
    if (d2 > rr * rr * 1.0201f) {
        const float lx = px * me.c + py * me.s, ly = py * me.c - px * me.s;   // the centre in the agent's frame
        const float half = asinf(md_min(rr * 1.01f * rsqrtf(d2), 1.0f)) + 0.02f;
        float rel = atan2f(ly, lx) - phase0;
        const float lo = (rel - half) * inv_dphi, hi = (rel + half) * inv_dphi;
        i_lo = (int)floorf(lo);
        n_try = min((int)ceilf(hi) - i_lo + 1, n_beams);
        i_lo = ((i_lo % n_beams) + n_beams) % n_beams;
    }
}

__device__ __forceinline__ void detector_wave(const MdWorld& w, const MdShape& me, int qa, int qb, const float* beam_cs, int n_beams,
                              float range, uint32_t kind_mask, int* best, int* pairs, int lane_id) {
    const float reach = range * 1.001f;
    float phase0 = 0.0f;
    const bool uniform_fan = detector_uniform_fan(beam_cs, n_beams, lane_id, &phase0);
    const float inv_dphi = 1.0f / (6.283185307179586f / (float)n_beams);
    int cnt = 0;   // wave-uniform
    // the 16-byte records of the NEXT 64 quads are requested before this round's are worked on: the rounds are a dependent chain
    // (ballot, pair list), and a cold fetch per round was most of the phase
    QuadBall nb;
    nb.mx = nb.my = nb.rr = 0.0f;
    nb.kind = 0;
    if (qa + lane_id < qb) nb = quad_ball_of(w, qa + lane_id);
    for (int q0 = qa; q0 < qb; q0 += 64) {
        const int q = q0 + lane_id;
        bool near = false;
        float px = 0.0f, py = 0.0f, rr = 0.0f;
        const QuadBall b = nb;
        if (q + 64 < qb) nb = quad_ball_of(w, q + 64);
        if (q < qb) {
            px = b.mx - me.cx;
            py = b.my - me.cy;
            rr = b.rr;
            const float far = reach + rr;
            near = ((kind_mask >> b.kind) & 1u) && !(px * px + py * py > far * far);
        }
        if (__ballot(near) == 0ull) continue;
        int i_lo = 0, n_try = n_beams;   // the beams that can meet this quad
        if (uniform_fan && near) detector_beam_window(me, px, py, rr, phase0, inv_dphi, n_beams, i_lo, n_try);
        int max_try = near ? n_try : 0;
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) max_try = max(max_try, __shfl_xor(max_try, off, 64));
        for (int k = 0; k < max_try; ++k) {
            int i = i_lo + k;
            if (i >= n_beams) i -= n_beams;
            const bool mine_ = near && k < n_try;
            const float bc = beam_cs[2 * i], bs = beam_cs[2 * i + 1];
            const float ux = bc * me.c - bs * me.s, uy = bs * me.c + bc * me.s;
            const float perp = ux * py - uy * px, along = ux * px + uy * py;
            const bool pass = mine_ && !(md_fabs(perp) > rr * 1.001f + 1.0e-3f || along < -rr || along > reach + rr);
            const unsigned long long m = __ballot(pass);
            if (m == 0ull) continue;
            if (cnt + 64 > kDetPairs) {   // keep room for a whole ballot
                wave_lds_sync();
                detector_drain(w, me, beam_cs, range, pairs, cnt, qa, best, lane_id);
                __builtin_amdgcn_wave_barrier();
                cnt = 0;
            }
            if (pass) pairs[cnt + __popcll(m & ((1ull << lane_id) - 1ull))] = ((q - qa) << 8) | i;
            cnt += __popcll(m);
        }
    }
    wave_lds_sync();
    detector_drain(w, me, beam_cs, range, pairs, cnt, qa, best, lane_id);
    __builtin_amdgcn_wave_barrier();
}

// One or TWO detector fans of one agent (side detector + lane-line detector: different beam tables, ranges and line kinds) against
// the quads [qa, qb) of its map by ONE wave, in ONE pass over the quads' cull records, in two phases so that the expensive slab
// tests run on full wavefronts: (1) lanes = quads: per fan kind, reach, then the beams that can meet the quad's bounding circle (a
// dozen instructions each); the (quad, beam) pairs that survive -- a few per hundred -- are appended to `pairs` (LDS, kDetPairs
// ints of this wave) through ballot prefix counts, the second fan's beams numbered behind the first's; (2) lanes = pairs: fetch
// the quad, cast, atomicMin on the fraction's bit pattern in the fan's `best` (initialised to 1.0).  The list is drained whenever
// a pass could overflow it.  Same arithmetic and the same minima as the oracle's serial loop per detector.
constexpr int kAllBeamsMax = 8;
struct DetFan2 {
    const float* cs0; int n0; float range0; uint32_t mask0; int* best0;
    const float* cs1; int n1; float range1; uint32_t mask1; int* best1;   // n1 == 0: one fan only
};
__device__ __forceinline__ void detector_drain2(const MdWorld& w, const MdShape& me, const DetFan2& f, const int* pairs, int n, int qa,
                               int lane_id) {   // a pair = (quad - qa) << 8 | beam (fan 1's beams from n0 on)
    const float4* quads4 = reinterpret_cast<const float4*>(w.quads);
    for (int k = lane_id; k < n; k += 64) {
        const int pr = pairs[k];
        const int q = qa + (pr >> 8), ig = pr & 255;
        const bool second = ig >= f.n0;
        const int i = second ? ig - f.n0 : ig;
        const float* cs = second ? f.cs1 : f.cs0;
        const float range = second ? f.range1 : f.range0;
        const float4 lo = quads4[2 * (size_t)q], hi = quads4[2 * (size_t)q + 1];
        const float v[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
        const float bc = cs[2 * i], bs = cs[2 * i + 1];
        const float ux = bc * me.c - bs * me.s, uy = bs * me.c + bc * me.s;
        const float t = md_ray_quad(me.cx, me.cy, ux * range, uy * range, v);
        if (t < 1.0f) atomicMin(second ? &f.best1[i] : &f.best0[i], __float_as_int(t));
    }
}

__device__ __forceinline__ void detector_wave2(const MdWorld& w, const MdShape& me, int qa, int qb, const DetFan2& f, int* pairs, int lane_id) {
    float ph0 = 0.0f, ph1 = 0.0f;
    const bool uni0 = detector_uniform_fan(f.cs0, f.n0, lane_id, &ph0);
    const bool uni1 = f.n1 > 0 ? detector_uniform_fan(f.cs1, f.n1, lane_id, &ph1) : false;
    const float reach_max = md_max(f.range0, f.n1 > 0 ? f.range1 : 0.0f) * 1.001f;
    int cnt = 0;   // wave-uniform
    // the 16-byte records of the NEXT 64 quads are requested before this round's are worked on: the rounds are a dependent chain
    // (ballot, pair list), and a cold fetch per round was most of the phase
    QuadBall nb;
    nb.mx = nb.my = nb.rr = 0.0f;
    nb.kind = 0;
    if (qa + lane_id < qb) nb = quad_ball_of(w, qa + lane_id);
    // Two passes: (a) lanes = quads, reach only, the quads within reach COMPACTED onto a list (the first half of `pairs`); (b) lanes =
    // listed quads, dense: kinds, beam ranges, circle tests.  In one pass (b)'s work ran for the whole wave as soon as one of a
    // round's 64 quads was within reach, and the quads within reach (a third of a map's) are spread over most rounds.
    constexpr int kNear = kDetPairs / 2, kPairs = kDetPairs - kNear;
    int* near_list = pairs;            // [kNear]  quad - qa
    int* pair_list = pairs + kNear;    // [kPairs]
    int n_near = 0;                    // wave-uniform
    const bool across_rounds = f.n0 > kAllBeamsMax || f.n1 > kAllBeamsMax;
    auto work_off = [&]() {
    wave_lds_sync();
    for (int t0 = 0; t0 < n_near; t0 += 64) {
        const bool in_reach = t0 + lane_id < n_near;
        const int q0 = qa + (in_reach ? near_list[t0 + lane_id] : 0);   // this lane's quad (no longer q0 + lane)
        float px = 0.0f, py = 0.0f, rr = 0.0f;
        QuadBall b;
        b.mx = b.my = b.rr = 0.0f;
        b.kind = 0;
        if (in_reach) {
            b = quad_ball_of(w, q0);
            px = b.mx - me.cx;
            py = b.my - me.cy;
            rr = b.rr;
        }
        // one fan after the other against this round's quads (the second only where there is one)
        for (int fan = 0; fan < (f.n1 > 0 ? 2 : 1); ++fan) {
            const float* beam_cs = fan ? f.cs1 : f.cs0;
            const int n_beams = fan ? f.n1 : f.n0;
            const float reach = (fan ? f.range1 : f.range0) * 1.001f;
            const uint32_t kind_mask = fan ? f.mask1 : f.mask0;
            const float phase0 = fan ? ph1 : ph0;
            const bool uniform_fan = fan ? uni1 : uni0;
            const int beam_base = fan ? f.n0 : 0;
            const float inv_dphi = 1.0f / (6.283185307179586f / (float)n_beams);
            const float far = reach + rr;
            const bool near = in_reach && ((kind_mask >> b.kind) & 1u) && !(px * px + py * py > far * far);
            if (__ballot(near) == 0ull) continue;
            int i_lo = 0, n_try = n_beams;   // the beams that can meet this quad
            if (uniform_fan && near && n_beams > kAllBeamsMax)   // a handful of beams: trying all costs less than asin + atan2
                detector_beam_window(me, px, py, rr, phase0, inv_dphi, n_beams, i_lo, n_try);
            // The (quad, beam) candidates of this round, FLAT: lane t of a pass takes candidate t -- beam k of the quad in the lane l
            // that owns it (the largest l whose exclusive prefix count is <= t: a six-step search through the wave's registers).
            // A loop over k as long as the NEAREST quad needs (up to all 72 beams, one lane busy) ran 5x as many passes.
            const int nt = near ? n_try : 0;
            int pin = nt;   // inclusive prefix count
#pragma unroll
            for (int off = 1; off < 64; off <<= 1) {
                const int v = __shfl_up(pin, off, 64);
                if (lane_id >= off) pin += v;
            }
            const int total = __shfl(pin, 63, 64);   // wave-uniform
            const int pex = pin - nt;
            for (int t0 = 0; t0 < total; t0 += 64) {
                const int t = t0 + lane_id;
                int l = 0;
#pragma unroll
                for (int step = 32; step >= 1; step >>= 1) {
                    const int cnd = l + step;
                    const int pc = __shfl(pex, cnd & 63, 64);
                    if (cnd < 64 && pc <= t) l = cnd;
                }
                const bool mine_ = t < total;
                const int k = t - __shfl(pex, l, 64);
                const float px_ = __shfl(px, l, 64), py_ = __shfl(py, l, 64), rr_ = __shfl(rr, l, 64);
                int i = __shfl(i_lo, l, 64) + k;
                if (i >= n_beams) i -= n_beams;
                if (!mine_) i = 0;
                const int q_ = __shfl(q0, l, 64);
                const float bc = beam_cs[2 * i], bs = beam_cs[2 * i + 1];
                const float ux = bc * me.c - bs * me.s, uy = bs * me.c + bc * me.s;
                const float perp = ux * py_ - uy * px_, along = ux * px_ + uy * py_;
                const bool pass = mine_ && !(md_fabs(perp) > rr_ * 1.001f + 1.0e-3f || along < -rr_ || along > reach + rr_);
                const unsigned long long m = __ballot(pass);
                if (m == 0ull) continue;
                if (cnt + 64 > kPairs) {   // keep room for a whole ballot
                    wave_lds_sync();
                    detector_drain2(w, me, f, pair_list, cnt, qa, lane_id);
                    __builtin_amdgcn_wave_barrier();
                    cnt = 0;
                }
                if (pass) pair_list[cnt + __popcll(m & ((1ull << lane_id) - 1ull))] = ((q_ - qa) << 8) | (beam_base + i);
                cnt += __popcll(m);
            }
        }
    }
    __builtin_amdgcn_wave_barrier();   // the list is free again
    n_near = 0;
    };
    for (int q0 = qa; q0 < qb; q0 += 64) {
        const int q = q0 + lane_id;
        const QuadBall b = nb;
        if (q + 64 < qb) nb = quad_ball_of(w, q + 64);
        bool in_reach = false;
        if (q < qb) {
            const float px = b.mx - me.cx, py = b.my - me.cy;
            const float far = reach_max + b.rr;
            in_reach = !(px * px + py * py > far * far);
        }
        const unsigned long long m = __ballot(in_reach);
        if (m == 0ull) continue;
        if (n_near + 64 > kNear) work_off();
        if (in_reach) near_list[n_near + __popcll(m & ((1ull << lane_id) - 1ull))] = q - qa;
        n_near += __popcll(m);
        if (!across_rounds) work_off();   // fans of a few beams: round by round (measured: collecting across rounds costs them 1 %)
    }
    work_off();
    wave_lds_sync();
    detector_drain2(w, me, f, pair_list, cnt, qa, lane_id);
    __builtin_amdgcn_wave_barrier();
}

// Side / lane-line detector as an entry point of its own (md_line_detector).  Work items = (agent, part of the map's quads),
// one WAVE each running detector_wave above; with four or more agents per env an item is a whole agent, with fewer the quads
// are split four ways.  A workgroup takes FOUR consecutive items of one env (grid = n_envs x ceil(items / 4)): the 40-agent
// tollgate batch of 512 envs is 5 120 workgroups -- the first form of this launch, one workgroup per env walking its ten
// rounds of agents in turn, left the chip at two workgroups per CU (174 us per launch there).  One thread per beam walking
// all quads, the very first form, took 1 ms on a scenario scene's ~1100 line pieces.
__device__ __host__ inline int detector_parts(int A) { return (A >= kBlock / 64) ? 1 : kBlock / 64; }
__device__ __host__ inline int detector_groups(int A) { return (A * detector_parts(A) + kBlock / 64 - 1) / (kBlock / 64); }

// LDS image of line_detector_kernel for nb beams (both fans)
struct LineDetectorLds { uint32_t best, beams, pairs, bytes; };
__host__ __device__ inline LineDetectorLds line_detector_lds(int nb) {
    constexpr int kW = kBlock / 64;
    LineDetectorLds L;
    L.best = 0;                                                  // [kW][nb] bit patterns of the closest fractions
    L.beams = L.best + (uint32_t)kW * nb * sizeof(int);            // [nb][2] the beam tables, fan 0 then fan 1
    L.pairs = L.beams + (uint32_t)nb * 2 * sizeof(float);          // [kW][kDetPairs] each wave's pair list
    L.bytes = L.pairs + (uint32_t)kW * kDetPairs * sizeof(int);
    return L;
}

__global__ __launch_bounds__(kBlock) void line_detector_kernel(MdWorld w, MdState s, MdConfig c,
                                                               const float* __restrict__ beam_cs, int n_beams,
                                                               float range, uint32_t kind_mask, float* out,
                                                               int out_stride, int out_offset,
                                                               const float* __restrict__ beam_cs1, int n_beams1, float range1,
                                                               uint32_t kind_mask1, int out_offset1) {
    // (beam_cs1, n_beams1 > 0, ...): a SECOND fan evaluated in the same pass over the quads (md_line_detectors)
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr int kW = kBlock / 64;
    const int A = c.agents_per_env;
    const int nb = n_beams + n_beams1;
    const int parts = detector_parts(A), groups = detector_groups(A);
    const LineDetectorLds L = line_detector_lds(nb);
    int* l_best = reinterpret_cast<int*>(smem + L.best);
    float* l_bm = reinterpret_cast<float*>(smem + L.beams);
    int* l_pairs = reinterpret_cast<int*>(smem + L.pairs);
    const int e = blockIdx.x / groups, grp = blockIdx.x - e * groups;
    if (e >= c.n_envs) return;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int m = w.env_map[e];
    const int q0 = w.quad_off[m], q1 = w.quad_off[m + 1];
    const int a_first = (grp * kW) / parts;                          // first agent this workgroup serves
    const int n_here = min(A - a_first, kW / parts);                 // agents it serves (4, or 1 when the quads are split)
    for (int it = tid; it < n_here * nb; it += kBlock) l_best[it] = __float_as_int(1.0f);
    for (int it = tid; it < 2 * n_beams; it += kBlock) l_bm[it] = beam_cs[it];
    for (int it = tid; it < 2 * n_beams1; it += kBlock) l_bm[2 * n_beams + it] = beam_cs1[it];
    __syncthreads();
    const int per = (q1 - q0 + parts - 1) / parts;
    const int it = grp * kW + wave;
    if (it < A * parts) {
        const int a = it / parts, part = it - a * parts;
        const MdShape me = s.shape[e * c.cap + a];
        if (md_present(me.flags)) {
            const int qa = q0 + part * per, qb = min(qa + per, q1);
            DetFan2 f;
            f.cs0 = l_bm; f.n0 = n_beams; f.range0 = range; f.mask0 = kind_mask; f.best0 = l_best + (a - a_first) * nb;
            f.cs1 = l_bm + 2 * n_beams; f.n1 = n_beams1; f.range1 = range1; f.mask1 = kind_mask1; f.best1 = f.best0 + n_beams;
            detector_wave2(w, me, qa, qb, f, l_pairs + wave * kDetPairs, lane);
        }
    }
    __syncthreads();
    for (int k = tid; k < n_here * nb; k += kBlock) {
        const int al = k / nb, i = k - al * nb;
        float* row = out + (size_t)(e * A + a_first + al) * out_stride;
        if (i < n_beams) row[out_offset + i] = __int_as_float(l_best[k]);
        else row[out_offset1 + (i - n_beams)] = __int_as_float(l_best[k]);
    }
}

// ------------------------------------------------------------------------------------------------
// Grid helpers
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ int grid_clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// ------------------------------------------------------------------------------------------------
// Localisation, one wave per vehicle.
// ------------------------------------------------------------------------------------------------
// pass B for one candidate lane L that contains the point (cx, cy; heading c, s): Frenet coordinates, heading filter, L1
// distance.  dist / road stay as the caller set them (3.0e38f / -1) for a lane that fails the heading filter.
__device__ __forceinline__ void localize_candidate(const MdLane* L, float cx, float cy, float c, float s, float& dist, float& ls,
                                                   int& road) {
    float llat;
    md_lane_local(L, cx, cy, &ls, &llat);
    if (md_lane_heading_dot(L, cx, cy, c, s) > 0.0f) {
        dist = md_lane_distance(L, ls, llat);
        road = L->road;
    }
}

// Commit of vehicle n by ONE lane: its lane (the caller's choice by preference, ls the longitudinal on it; -1: the previous lane
// stays) and the route cursors' advance within the first 5 m of a lane whose road starts at a later route node.  nav_*: the
// vehicle's MdNav fields before the step; rroads / rnodes: its route (global: read only when the cursors advance).
__device__ __forceinline__ void localize_commit(const MdLane* lanes, const MdRoad* roads, const MdState& s, int n, int lane, float ls,
                                                float cx, float cy, int nav_lane, int nav_ck0, int nav_ck1,
                                                int nav_route_len, const int32_t* rroads, const int32_t* rnodes) {
    const bool kept = lane < 0;  // found nothing: the previous lane stays, its longitudinal was not evaluated above
    if (kept) lane = nav_lane;
    s.nav[n].lane = lane;
    if (lane < 0) return;
    if (nav_ck0 == nav_ck1) return;
    if (kept) {
        float llat;
        md_lane_local(&lanes[lane], cx, cy, &ls, &llat);
    }
    if (!(ls < 5.0f)) return;
    const int start_node = roads[lanes[lane].road].start_node;
    const int k = nav_route_len;
    int idx = -1;
    for (int j = nav_ck1; j < k - 1; ++j) {
        if (rnodes[j] == start_node) { idx = j; break; }
    }
    if (idx < 0) return;
    const int nck1 = (idx + 1 == k - 1) ? idx : idx + 1;
    s.nav[n].ck0 = idx;
    s.nav[n].ck1 = nck1;
    s.nav[n].road0 = rroads[idx];
    s.nav[n].road1 = rroads[nck1];
}

// pass A for one candidate lane L, the share of lane hl of the GW lanes that test it: the hull's edges hl, hl + GW, ... (4-vertex
// hulls come inline from the lane record).  true: (cx, cy) is outside one of them; hn: the hull's vertex count.
template <int GW>
__device__ __forceinline__ bool hull_edges_outside(const MdLane* L, const float* hull_xy, float cx, float cy, int hl, int& hn) {
    hn = L->hull_n;
    const float* xy = md_lane_hull(L, hull_xy);
    bool outside = false;
    for (int i = hl; i < hn; i += GW) {
        const int j = (i + 1 == hn) ? 0 : i + 1;
        const float ex = xy[2 * j] - xy[2 * i], ey = xy[2 * j + 1] - xy[2 * i + 1];
        const float cr = ex * (cy - xy[2 * i + 1]) - ey * (cx - xy[2 * i]);
        if (cr < 0.0f) outside = true;
    }
    return outside;
}

// pass A by the whole wave, ballot vote.  Wave-uniform result: L's hull contains (cx, cy).
__device__ __forceinline__ bool hull_contains_wave(const MdLane* L, const float* hull_xy, float cx, float cy, int lane_id) {
    int hn;
    const bool outside = hull_edges_outside<64>(L, hull_xy, cx, cy, lane_id, hn);
    return __ballot(outside) == 0ull && hn >= 3;
}

// A/B builds: -DMD_LOC_ROAD_FIRST=0 compiles every kernel without the road-first localisation below
#ifndef MD_LOC_ROAD_FIRST
#define MD_LOC_ROAD_FIRST 1
#endif
// The road-first window: the lane records nav_lane - kLocWindow .. nav_lane + kLocWindow, one per wave lane.  A road's lanes are
// contiguous (first = lane - idx), so 3 covers every road of up to four lanes wherever in it the vehicle was; PG roads have 1-4.
constexpr int kLocWindow = 3;

// Localisation on the lanes of the vehicle's CURRENT road, before any table: the wave loads the records around the previous lane
// in one trip (no grid header, cell range or item list), the lanes of road cur_road test their own record in parallel (box, hull,
// Frenet + heading filter: localize_vehicle's predicates in its order) and the nearest one wins, the lowest lane id on ties.
// A lane of the current road that contains the point and passes the heading filter is what localize_vehicle's selection takes
// whenever there is one (best_cur), and the grid cell's list holds every lane whose box contains the point, so a hit here is the
// walk's result.  false (nothing written): no previous lane, the previous lane is not on cur_road, the road does not fit the
// window, or none of its lanes qualifies -- the caller runs the grid walk as if nothing had happened.
__device__ __forceinline__ bool localize_road_first(const MdLane* lanes, int n_lanes, const float* hull_xy, int nav_lane, int cur_road,
                                                    float cx, float cy, float c, float s, int lane_id, int& best, float& best_ls) {
    if (nav_lane < 0 || nav_lane >= n_lanes) return false;
    const int li = nav_lane - kLocWindow + lane_id;
    const bool valid = lane_id <= 2 * kLocWindow && li >= 0 && li < n_lanes;   // no load leaves the map's slice
    const MdLane* L = &lanes[valid ? li : nav_lane];
    int road = -1, idx = 0, nr = 0, hn = 0;
    float x0 = 0.0f, y0 = 0.0f, x1 = 0.0f, y1 = 0.0f;
    float h[8] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    if (valid) {
        road = L->road; idx = L->idx; nr = L->n_in_road;
        x0 = L->x0; y0 = L->y0; x1 = L->x1; y1 = L->y1;
        hn = L->hull_n;
#pragma unroll
        for (int i = 0; i < 8; ++i) h[i] = L->hull4[i];
    }
    // the previous lane's record is in wave lane kLocWindow
    const int first = nav_lane - bcast_i(idx, kLocWindow), n_road = bcast_i(nr, kLocWindow);
    if (bcast_i(road, kLocWindow) != cur_road || first < nav_lane - kLocWindow || first + n_road > nav_lane + kLocWindow + 1) return false;
    const bool mine = valid && road == cur_road && li >= first && li < first + n_road;
    const bool pass = mine && !(cx < x0 || cx > x1 || cy < y0 || cy > y1);
    bool contains = false;
    if (pass && hn == 4) {   // straight lanes: the four edges in this lane
        bool outside = false;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int j = (i + 1) & 3;
            const float ex = h[2 * j] - h[2 * i], ey = h[2 * j + 1] - h[2 * i + 1];
            const float cr = ex * (cy - h[2 * i + 1]) - ey * (cx - h[2 * i]);
            if (cr < 0.0f) outside = true;
        }
        contains = !outside;
    }
    unsigned long long wide = __ballot(pass && hn != 4);   // other hulls (circular lanes): the wave's vote, one candidate at a time
    while (wide) {
        const int k = __ffsll((long long)wide) - 1;
        wide &= wide - 1;
        const bool in = hull_contains_wave(&lanes[nav_lane - kLocWindow + k], hull_xy, cx, cy, lane_id);
        if (k == lane_id) contains = in;
    }
    float my_dist = 3.0e38f, my_ls = 0.0f;
    int my_road = -1;
    if (contains) localize_candidate(L, cx, cy, c, s, my_dist, my_ls, my_road);
    unsigned long long sel = __ballot(my_road >= 0);   // contained and past the heading filter
    float d = 3.0e38f;
    int k_best = -1;
    while (sel) {   // ascending lane id, strict <: the first minimum
        const int k = __ffsll((long long)sel) - 1;
        sel &= sel - 1;
        const float dist = bcast_f(my_dist, k);
        if (dist < d) { d = dist; k_best = k; }
    }
    if (k_best < 0) return false;
    best = nav_lane - kLocWindow + k_best;
    best_ls = bcast_f(my_ls, k_best);
    return true;
}

// onlane_out: nullptr = write the ON_LANE bit into s.flags[n] (stand-alone phase); otherwise store the bare
// decision there and leave s.flags alone (fused step: contacts run concurrently and own the other bits).
// kRoadFirst: try localize_road_first before the grid walk (the lean fused step; the other kernels keep the walk alone).
template <bool kRoadFirst = false>
__device__ __forceinline__ void localize_vehicle(const MdWorld& w, const MdLane* lanes, const MdRoad* roads, const MdState& s, int e,
                                 int n, int lane_id, uint32_t* onlane_out = nullptr) {
    // n = slot inside the env-local view; lanes / roads = this env's map tables (LDS copies)
    const MdShape sh = s.shape[n];
    if (!md_drives(sh.flags)) return;
    MdNav nav = s.nav[n];
    const int m = w.env_map[e];
    const int32_t* rroads = s.route_roads + (size_t)n * MD_ROUTE_LEN;   // global: read only when the cursors advance
    const int32_t* rnodes = s.route_nodes + (size_t)n * MD_ROUTE_LEN;
    const int cur_road = nav.road0;
    const bool has_next = nav.ck1 != nav.ck0;
    const int next_road = has_next ? nav.road1 : -1;

    MD_FINE_STAMP(n == 0 && lane_id == 0, 0);
    int on_lane = 0;
    int best_any = -1, best_cur = -1, best_next = -1;
    float d_any = 3.0e38f, d_cur = 3.0e38f, d_next = 3.0e38f;
    float ls_any = 0.0f, ls_cur = 0.0f, ls_next = 0.0f;
    if (MD_LOC_ROAD_FIRST && kRoadFirst &&
        localize_road_first(lanes, w.lane_off[m + 1] - w.lane_off[m], w.hull_xy, nav.lane, cur_road, sh.cx, sh.cy, sh.c, sh.s, lane_id,
                            best_cur, ls_cur))
        on_lane = 1;
    MD_LOC_COUNT(lane_id == 0, on_lane);
    // a hit leaves the walk nothing to do: the grid header and the cell's range are loaded behind the miss
    int it0 = 0, it1 = 0;
    if (!on_lane) {
        const MdGrid g = w.grid[m];
        const int gx = (int)md_floor((sh.cx - g.x0) * g.inv_cell);
        const int gy = (int)md_floor((sh.cy - g.y0) * g.inv_cell);
        if (gx >= 0 && gx < g.nx && gy >= 0 && gy < g.ny) {
            const int cell = g.cell_base + gy * g.nx + gx;
            it0 = w.cell_start[cell];
            it1 = w.cell_start[cell + 1];
        }
    }
    MD_FINE_STAMP(n == 0 && lane_id == 0 && it1 >= 0, 1);
    // Candidate lanes of the cell: each LANE fetches one cell item and tests its lane record's hull
    // AABB (records are in LDS); survivors are visited in ascending lane id through the ballot mask
    // (ties in distance resolve to the lowest lane id, like the oracle's ascending scan).
    //   pass A  hull containment of every surviving candidate (edges spread over the 64 lanes, ballot
    //           vote; 4-vertex hulls come inline from the lane record, no second lookup)
    //   pass B  ONE batched Frenet evaluation: lane k evaluates the k-th contained candidate
    //   pass C  uniform selection over the (few) contained candidates
    for (int itb = it0; itb < it1; itb += 64) {
        const int it = itb + lane_id;
        int l = -1;
        bool pass = false;
        if (it < it1) {
            l = w.cell_items[it];
            if (l >= 0) {
                const MdLane* L = &lanes[l];
                pass = !(sh.cx < L->x0 || sh.cx > L->x1 || sh.cy < L->y0 || sh.cy > L->y1);
            }
        }
        unsigned long long mask = __ballot(pass);
        MD_FINE_STAMP(n == 0 && lane_id == 0, 2);
#ifdef MD_STAMP
        if (n == 0 && lane_id == 0 && g_stamp_buf)
            g_stamp_buf[(size_t)blockIdx.x * 32 + 16 + 15] = (unsigned long long)__popcll(mask) | ((unsigned long long)(it1 - it0) << 32);
#endif
        unsigned long long inside = 0ull;  // bit k: candidate held by lane k contains the point
        while (mask) {
            const int k = __ffsll((long long)mask) - 1;
            mask &= mask - 1;
            if (hull_contains_wave(&lanes[bcast_i(l, k)], w.hull_xy, sh.cx, sh.cy, lane_id)) inside |= 1ull << k;
        }
        if (inside == 0ull) continue;
        on_lane = 1;
        // pass B: my lane's candidate (if contained): Frenet coordinates, heading filter, L1 distance
        float my_dist = 3.0e38f, my_ls = 0.0f;
        int my_road = -1;
        if ((inside >> lane_id) & 1ull) localize_candidate(&lanes[l], sh.cx, sh.cy, sh.c, sh.s, my_dist, my_ls, my_road);
        // pass C (the winner's longitudinal is kept: the checkpoint update below needs it)
        while (inside) {
            const int k = __ffsll((long long)inside) - 1;
            inside &= inside - 1;
            const float dist = bcast_f(my_dist, k);
            const int road = bcast_i(my_road, k);
            const int lk = bcast_i(l, k);
            if (road < 0) continue;  // failed the heading filter
            const float lsk = bcast_f(my_ls, k);
            if (dist < d_any) { d_any = dist; best_any = lk; ls_any = lsk; }
            if (road == cur_road && dist < d_cur) { d_cur = dist; best_cur = lk; ls_cur = lsk; }
            if (has_next && road == next_road && dist < d_next) { d_next = dist; best_next = lk; ls_next = lsk; }
        }
    }
    MD_FINE_STAMP(n == 0 && lane_id == 0, 3);
    if (lane_id != 0) return;  // everything below is wave-uniform; lane 0 commits
    int lane = -1;
    float ls = 0.0f;
    if (best_cur >= 0) { lane = best_cur; ls = ls_cur; }
    else if (!has_next) { lane = best_any; ls = ls_any; }
    else if (best_next >= 0) { lane = best_next; ls = ls_next; }
    else { lane = best_any; ls = ls_any; }
    if (onlane_out) {
        onlane_out[n] = on_lane ? MD_FL_ON_LANE : 0u;
    } else {
        uint32_t fl = s.flags[n] & ~(uint32_t)MD_FL_ON_LANE;
        if (on_lane) fl |= MD_FL_ON_LANE;
        s.flags[n] = fl;
    }
    localize_commit(lanes, roads, s, n, lane, ls, sh.cx, sh.cy, nav.lane, nav.ck0, nav.ck1, nav.route_len, rroads, rnodes);
}

// localize_road_first for the groups of localize_group<GW> (one vehicle per GW lanes; every argument but lanes / n_lanes / hull_xy is
// uniform within a group): the same window, predicates, order and tie-break, votes through the group's part of the ballot.
// true in the lanes of a group whose vehicle was found (best / best_ls set there).
template <int GW>
__device__ __forceinline__ bool localize_road_first_group(const MdLane* lanes, int n_lanes, const float* hull_xy, bool act, int nav_lane,
                                                          int cur_road, float cx, float cy, float c, float s, int lane_id, int& best,
                                                          float& best_ls) {
    constexpr unsigned kGroupMask = (GW == 32) ? 0xFFFFFFFFu : 0xFFFFu;
    const int hl = lane_id & (GW - 1), hbase = lane_id - hl;
    const auto part_of = [&](unsigned long long b) { return (unsigned)(b >> hbase) & kGroupMask; };
    const bool any = act && nav_lane >= 0 && nav_lane < n_lanes;
    const int li = nav_lane - kLocWindow + hl;
    const bool valid = any && hl <= 2 * kLocWindow && li >= 0 && li < n_lanes;   // no load leaves the map's slice
    const MdLane* L = &lanes[valid ? li : 0];
    int road = -1, idx = 0, nr = 0, hn = 0;
    float x0 = 0.0f, y0 = 0.0f, x1 = 0.0f, y1 = 0.0f;
    float h[8] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    if (valid) {
        road = L->road; idx = L->idx; nr = L->n_in_road;
        x0 = L->x0; y0 = L->y0; x1 = L->x1; y1 = L->y1;
        hn = L->hull_n;
#pragma unroll
        for (int i = 0; i < 8; ++i) h[i] = L->hull4[i];
    }
    const int first = nav_lane - __shfl(idx, hbase + kLocWindow, 64), n_road = __shfl(nr, hbase + kLocWindow, 64);
    const bool elig = any && __shfl(road, hbase + kLocWindow, 64) == cur_road && first >= nav_lane - kLocWindow &&
                      first + n_road <= nav_lane + kLocWindow + 1;
    const bool mine = elig && valid && road == cur_road && li >= first && li < first + n_road;
    const bool pass = mine && !(cx < x0 || cx > x1 || cy < y0 || cy > y1);
    bool contains = false;
    if (pass && hn == 4) {
        bool outside = false;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int j = (i + 1) & 3;
            const float ex = h[2 * j] - h[2 * i], ey = h[2 * j + 1] - h[2 * i + 1];
            const float cr = ex * (cy - h[2 * i + 1]) - ey * (cx - h[2 * i]);
            if (cr < 0.0f) outside = true;
        }
        contains = !outside;
    }
    unsigned wide = part_of(__ballot(pass && hn != 4));   // other hulls: the group's vote, one candidate at a time
    while (__ballot(wide != 0u) != 0ull) {
        const bool on = wide != 0u;
        const int k = on ? (__ffs((int)wide) - 1) : 0;
        if (on) wide &= wide - 1;
        bool outside = false;
        int hk = 0;
        if (on) outside = hull_edges_outside<GW>(&lanes[nav_lane - kLocWindow + k], hull_xy, cx, cy, hl, hk);
        const unsigned out_h = part_of(__ballot(outside));
        if (on && k == hl) contains = out_h == 0u && hk >= 3;
    }
    float my_dist = 3.0e38f, my_ls = 0.0f;
    int my_road = -1;
    if (contains) localize_candidate(L, cx, cy, c, s, my_dist, my_ls, my_road);
    unsigned sel = part_of(__ballot(my_road >= 0));
    float d = 3.0e38f;
    int k_best = -1;
    while (__ballot(sel != 0u) != 0ull) {   // ascending lane id, strict <: the first minimum
        const bool on = sel != 0u;
        const int k = on ? (__ffs((int)sel) - 1) : 0;
        if (on) sel &= sel - 1;
        const float dist = __shfl(my_dist, hbase + k, 64);
        if (on && dist < d) { d = dist; k_best = k; }
    }
    const float ls = __shfl(my_ls, hbase + (k_best < 0 ? 0 : k_best), 64);
    if (k_best < 0) return false;
    best = nav_lane - kLocWindow + k_best;
    best_ls = ls;
    return true;
}

// ------------------------------------------------------------------------------------------------
// Localisation of TWO vehicles by one wave (lanes 0-31: slot_a, lanes 32-63: slot_b; -1 = half idle): the form the
// fused step uses when more vehicles drive than the workgroup has waves.  Same arithmetic, same candidate order and
// tie-breaks as localize_vehicle; the per-vehicle data are per-lane values here (uniform within a half), cross-lane
// reads go through __shfl, votes through the matching half of a 64-bit ballot.  Results go to onlane_out.
// ------------------------------------------------------------------------------------------------
// GW = lanes per vehicle: 32 (two vehicles per wave) or 16 (four; the one-wave-per-env kernel's form when three or more
// vehicles drive).  slot_c / slot_d are only read with GW == 16.
template <int GW, bool kRoadFirst = false>
__device__ __forceinline__ void localize_group(const MdWorld& w, const MdLane* lanes, const MdRoad* roads, const MdState& s, int e,
                              int slot_a, int slot_b, int slot_c, int slot_d, int lane_id, uint32_t* onlane_out) {
    constexpr unsigned kGroupMask = (GW == 32) ? 0xFFFFFFFFu : 0xFFFFu;
    const int h = lane_id / GW, hl = lane_id & (GW - 1), hbase = h * GW;
    const int n = (h == 0) ? slot_a : ((h == 1) ? slot_b : ((h == 2) ? slot_c : slot_d));
    const bool act = n >= 0;  // (slots handed in always drive)
    const int nn = act ? n : 0;
    struct { float cx, cy, c, s; } sh;   // only what the search needs, per lane
    sh.cx = s.shape[nn].cx;
    sh.cy = s.shape[nn].cy;
    sh.c = s.shape[nn].c;
    sh.s = s.shape[nn].s;
    struct { int lane, ck0, ck1, route_len; } nav;
    nav.lane = s.nav[nn].lane;
    nav.ck0 = s.nav[nn].ck0;
    nav.ck1 = s.nav[nn].ck1;
    nav.route_len = s.nav[nn].route_len;
    const int m = w.env_map[e];
    const int32_t* rroads = s.route_roads + (size_t)nn * MD_ROUTE_LEN;   // global: read only when the cursors advance
    const int32_t* rnodes = s.route_nodes + (size_t)nn * MD_ROUTE_LEN;
    const int cur_road = s.nav[nn].road0;
    const bool has_next = nav.ck1 != nav.ck0;
    const int next_road = has_next ? s.nav[nn].road1 : -1;
    int on_lane = 0;
    int best_any = -1, best_cur = -1, best_next = -1;
    float d_any = 3.0e38f, d_cur = 3.0e38f, d_next = 3.0e38f;
    float ls_any = 0.0f, ls_cur = 0.0f, ls_next = 0.0f;
    if (MD_LOC_ROAD_FIRST && kRoadFirst &&
        localize_road_first_group<GW>(lanes, w.lane_off[m + 1] - w.lane_off[m], w.hull_xy, act, nav.lane, cur_road, sh.cx, sh.cy, sh.c,
                                      sh.s, lane_id, best_cur, ls_cur))
        on_lane = 1;
    const bool road_first_hit = on_lane != 0;
    (void)road_first_hit;
    // a group that was answered above leaves the walk nothing to do; the grid header is loaded only if some group walks
    int it0 = 0, it1 = 0;
    if (!(MD_LOC_ROAD_FIRST && kRoadFirst) || __ballot(act && !on_lane) != 0ull) {
        const MdGrid g = w.grid[m];
        const int gx = (int)md_floor((sh.cx - g.x0) * g.inv_cell);
        const int gy = (int)md_floor((sh.cy - g.y0) * g.inv_cell);
        if (act && !on_lane && gx >= 0 && gx < g.nx && gy >= 0 && gy < g.ny) {
            const int cell = g.cell_base + gy * g.nx + gx;
            it0 = w.cell_start[cell];
            it1 = w.cell_start[cell + 1];
        }
    }
    const auto part_of = [&](unsigned long long b) { return (unsigned)(b >> hbase) & kGroupMask; };
    for (int itb = it0; __ballot(itb < it1) != 0ull; itb += GW) {
        const int it = itb + hl;
        int l = -1;
        bool pass = false;
        if (it < it1) {
            l = w.cell_items[it];
            if (l >= 0) {
                const MdLane* L = &lanes[l];
                pass = !(sh.cx < L->x0 || sh.cx > L->x1 || sh.cy < L->y0 || sh.cy > L->y1);
            }
        }
        unsigned mask = part_of(__ballot(pass));
        unsigned inside = 0u;  // bit k: candidate held by lane k of MY group contains the point
        while (__ballot(mask != 0u) != 0ull) {
            const bool mine = mask != 0u;
            const int k = mine ? (__ffs((int)mask) - 1) : 0;
            if (mine) mask &= mask - 1;
            const int lk = __shfl(l, hbase + k, 64);
            bool outside = false;
            int hn = 0;
            if (mine) outside = hull_edges_outside<GW>(&lanes[lk], w.hull_xy, sh.cx, sh.cy, hl, hn);
            const unsigned out_h = part_of(__ballot(outside));
            if (mine && out_h == 0u && hn >= 3) inside |= 1u << k;
        }
        if (inside != 0u) on_lane = 1;
        float my_dist = 3.0e38f, my_ls = 0.0f;
        int my_road = -1;
        if ((inside >> hl) & 1u) localize_candidate(&lanes[l], sh.cx, sh.cy, sh.c, sh.s, my_dist, my_ls, my_road);
        while (__ballot(inside != 0u) != 0ull) {
            const bool mine = inside != 0u;
            const int k = mine ? (__ffs((int)inside) - 1) : 0;
            if (mine) inside &= inside - 1;
            const float dist = __shfl(my_dist, hbase + k, 64);
            const int road = __shfl(my_road, hbase + k, 64);
            const int lk = __shfl(l, hbase + k, 64);
            const float lsk = __shfl(my_ls, hbase + k, 64);
            if (!mine || road < 0) continue;
            if (dist < d_any) { d_any = dist; best_any = lk; ls_any = lsk; }
            if (road == cur_road && dist < d_cur) { d_cur = dist; best_cur = lk; ls_cur = lsk; }
            if (has_next && road == next_road && dist < d_next) { d_next = dist; best_next = lk; ls_next = lsk; }
        }
    }
    if (hl != 0 || !act) return;  // lane 0 of each group commits its vehicle
    MD_LOC_COUNT(true, road_first_hit);
    int lane = -1;
    float ls = 0.0f;
    if (best_cur >= 0) { lane = best_cur; ls = ls_cur; }
    else if (!has_next) { lane = best_any; ls = ls_any; }
    else if (best_next >= 0) { lane = best_next; ls = ls_next; }
    else { lane = best_any; ls = ls_any; }
    onlane_out[n] = on_lane ? MD_FL_ON_LANE : 0u;
    localize_commit(lanes, roads, s, n, lane, ls, sh.cx, sh.cy, nav.lane, nav.ck0, nav.ck1, nav.route_len, rroads, rnodes);
}

template <bool kRoadFirst = false>
__device__ __forceinline__ void localize_pair(const MdWorld& w, const MdLane* lanes, const MdRoad* roads, const MdState& s, int e,
                              int slot_a, int slot_b, int lane_id, uint32_t* onlane_out) {
    localize_group<32, kRoadFirst>(w, lanes, roads, s, e, slot_a, slot_b, -1, -1, lane_id, onlane_out);
}

// ------------------------------------------------------------------------------------------------
// Contacts, one wave per vehicle.
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ void contacts_vehicle(const MdWorld& w, const MdState& s, const MdConfig& c, int e, int slot, int lane_id,
                                 uint32_t* cfl_out = nullptr) {
    const int base = 0;  // env-local view
    const int n = slot;
    const MdShape me = s.shape[n];
    if (!md_drives(me.flags)) return;
    if (!(me.flags & MD_F_AGENT)) {  // traffic: nothing reads its crash / line flags (see the oracle's contacts_mover)
        if (lane_id == 0) {
            if (cfl_out) cfl_out[n] = 0u;
            else s.flags[n] &= MD_FL_ON_LANE;
        }
        return;
    }
    uint32_t fl = 0;
    for (int j0 = 0; j0 < c.cap; j0 += 64) {
        const int j = j0 + lane_id;
        if (j >= c.cap || j == slot) continue;
        const MdShape o = s.shape[base + j];
        if (!md_present(o.flags)) continue;
        const int k = md_kind_of(o.flags);
        int hit;
        if (md_is_circle_kind(k)) hit = md_obb_circle(me.cx, me.cy, me.c, me.s, me.hl, me.hw, o.cx, o.cy, o.hl);
        else hit = md_obb_obb(me.cx, me.cy, me.c, me.s, me.hl, me.hw, o.cx, o.cy, o.c, o.s, o.hl, o.hw);
        if (!hit) continue;
        if (k == MD_KIND_VEHICLE) fl |= MD_FL_CRASH_VEHICLE;
        else if (k == MD_KIND_CONE || k == MD_KIND_WARNING || k == MD_KIND_BARRIER) fl |= MD_FL_CRASH_OBJECT;
        else if (k == MD_KIND_PEDESTRIAN || k == MD_KIND_CYCLIST) fl |= MD_FL_CRASH_HUMAN;
        else if (k == MD_KIND_BUILDING) fl |= MD_FL_CRASH_BUILDING;
    }
    // static quads through the grid: cells under the chassis AABB (+ margin)
    const int m = w.env_map[e];
    const MdGrid g = w.grid[m];
    const float ext_x = md_fabs(me.c) * me.hl + md_fabs(me.s) * me.hw + 0.05f;
    const float ext_y = md_fabs(me.s) * me.hl + md_fabs(me.c) * me.hw + 0.05f;
    int gx0 = (int)md_floor((me.cx - ext_x - g.x0) * g.inv_cell);
    int gx1 = (int)md_floor((me.cx + ext_x - g.x0) * g.inv_cell);
    int gy0 = (int)md_floor((me.cy - ext_y - g.y0) * g.inv_cell);
    int gy1 = (int)md_floor((me.cy + ext_y - g.y0) * g.inv_cell);
    if (!(gx1 < 0 || gy1 < 0 || gx0 >= g.nx || gy0 >= g.ny)) {
        gx0 = grid_clampi(gx0, 0, g.nx - 1);
        gx1 = grid_clampi(gx1, 0, g.nx - 1);
        gy0 = grid_clampi(gy0, 0, g.ny - 1);
        gy1 = grid_clampi(gy1, 0, g.ny - 1);
        const float* quads = w.quads + 8 * (size_t)w.quad_off[m];
        const int32_t* qkind = w.quad_kind + w.quad_off[m];
        for (int gy = gy0; gy <= gy1; ++gy)
            for (int gx = gx0; gx <= gx1; ++gx) {
                const int cell = g.cell_base + gy * g.nx + gx;
                const int it0 = w.cell_start[cell], it1 = w.cell_start[cell + 1];
                for (int it = it0 + lane_id; it < it1; it += 64) {
                    const int item = w.cell_items[it];
                    if (item >= 0) continue;  // lane item
                    const int q = ~item;
                    if (!md_obb_quad(me.cx, me.cy, me.c, me.s, me.hl, me.hw, quads + 8 * (size_t)q)) continue;
                    switch (qkind[q]) {
                        case MD_Q_LINE_WHITE_CONT: fl |= MD_FL_ON_WHITE_CONT; break;
                        case MD_Q_LINE_YELLOW_CONT: fl |= MD_FL_ON_YELLOW_CONT; break;
                        case MD_Q_LINE_BROKEN: fl |= MD_FL_ON_BROKEN; break;
                        case MD_Q_SIDEWALK: fl |= MD_FL_CRASH_SIDEWALK; break;
                        case MD_Q_CROSSWALK: fl |= MD_FL_ON_CROSSWALK; break;
                        default: break;
                    }
                }
            }
    }
    // wave OR-reduce of the flag word: one ballot per flag bit that can be set here
    uint32_t all = 0;
#pragma unroll
    for (int b = 0; b < 9; ++b) {
        const uint32_t bit = 1u << b;
        if (__ballot((fl & bit) != 0) != 0ull) all |= bit;
    }
    if (lane_id == 0) {
        if (cfl_out) cfl_out[n] = all;
        else s.flags[n] = (s.flags[n] & MD_FL_ON_LANE) | all;
    }
}

// ------------------------------------------------------------------------------------------------
// IDM for one traffic vehicle, executed by one wave: lanes = candidate objects; the lead / rear
// vehicle gap scan is a wavefront min-reduction (key = gap, tie -> lowest slot), which is the
// order-independent form of FrontBackObjects.get_find_front_back_objs (policy/idm_policy.py:82-132).
// Stages A (route bookkeeping) and C (lane-change policy, PID steering, IDM acceleration) are
// scalar and run on lane 0.
// ------------------------------------------------------------------------------------------------
// The scan's LDS words, after the compacted candidate list (wave_list[0..20]): the six gap minima, (scanned lane i,
// front / back) at 64-bit word i * 2 + {0, 1}, and the ego's Frenet data on the scanned lanes for stage C.
constexpr int kIdmKeyWord = 24;       // int index of the first 64-bit key (8-B aligned: the scratch is 16-B aligned)
constexpr int kIdmLatWord = 40;       // + k: lateral offset on scanned lane k
constexpr int kIdmHeadWord = 44;      // + k: the lane's heading 1 m ahead of the ego's longitudinal on it
constexpr unsigned long long kNoGap = ~0ull;

// (gap, slot) as one unsigned key: the gap's bits mapped so that unsigned order is float order across the sign (a connected
// lane's back gap can be negative), +-0 alike, the slot in the low word so that equal gaps keep the lowest slot.
__device__ __forceinline__ unsigned long long gap_key(float g, int slot) {
    const unsigned u = __float_as_uint(g);
    const unsigned o = (g == 0.0f) ? 0x80000000u : ((u & 0x80000000u) ? ~u : (u | 0x80000000u));
    return ((unsigned long long)o << 32) | (unsigned)slot;
}
__device__ __forceinline__ float gap_of_key(unsigned long long k) {
    const unsigned o = (unsigned)(k >> 32);
    return __uint_as_float((o & 0x80000000u) ? (o & 0x7fffffffu) : ~o);
}

// Reads the six minima back into fb (wave-uniform); returns bit i*2 (front) / i*2+1 (back) for every bucket that holds one.
__device__ __forceinline__ int gap_keys_read(const unsigned long long* keys, FrontBack& fb) {
    int found = 0;
#pragma unroll
    for (int b = 0; b < 6; ++b) {
        const unsigned long long k = keys[b];
        if (k != kNoGap) {
            found |= 1 << b;
            if (b & 1) { fb.back_d[b >> 1] = gap_of_key(k); fb.back[b >> 1] = (int)(unsigned)k; }
            else { fb.front_d[b >> 1] = gap_of_key(k); fb.front[b >> 1] = (int)(unsigned)k; }
        }
    }
    return found;
}

// arg-min of (key, slot) over the wave; lanes holding kInf do not take part.  Ascending lane order
// == ascending slot order, so the strict `<` keeps the lowest slot among equal keys.
__device__ __forceinline__ void wave_argmin(float& key, int& slot) {
    unsigned long long m = __ballot(key < 3.0e38f);
    float bk = 3.0e38f;
    int bs = 0x7fffffff;
    while (m) {
        const int l = __ffsll((long long)m) - 1;
        m &= m - 1;
        const float k = __shfl(key, l, 64);
        const int sl = __shfl(slot, l, 64);
        if (k < bk) {
            bk = k;
            bs = sl;
        }
    }
    key = bk;
    slot = bs;
}

// Nothing found on any scanned lane, and no lane scanned yet (the scans set exist[] from their plan).
__device__ __forceinline__ void front_back_clear(FrontBack& fb) {
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        fb.front[i] = fb.back[i] = -1;
        fb.exist[i] = 0;
        fb.front_d[i] = fb.back_d[i] = IDM_MAX_LONG_DIST;
    }
}

// The candidate objects of the vehicle in `slot` at (px, py) (get_surrounding_objects: within 50 m, present, not the vehicle
// itself), compacted in ascending slot order into wave_list: usually a handful, whatever the slot capacity is.  Returns their
// number (wave-uniform); only the first 21 are listed.  The caller syncs the wave's LDS before it reads wave_list.
__device__ __forceinline__ int idm_candidates_wave(const MdState& s, const MdConfig& c, int slot, int lane_id, float px, float py,
                                                   int* wave_list, MdIdmPlan& plan) {
    int n_cand = 0;
    bool sees_participant = false;  // a pedestrian / cyclist among them: the reference's object loop raises (md_idm_sees_participant)
    for (int j0 = 0; j0 < c.cap; j0 += 64) {
        const int j = j0 + lane_id;
        const bool is_c = j < c.cap && j != slot && md_idm_is_candidate(&s.shape[j < c.cap ? j : 0], px, py);
        const unsigned long long mk = __ballot(is_c);
        if (__ballot(is_c && md_is_participant_kind(md_kind_of(s.shape[j < c.cap ? j : 0].flags))) != 0ull) sees_participant = true;
        const int rank = n_cand + __popcll(mk & ((1ull << lane_id) - 1ull));
        if (is_c && rank < 21) wave_list[rank] = j;
        n_cand += __popcll(mk);
    }
    if (sees_participant) {  // wave-uniform: bare-except fallback, nothing is scanned
        plan.fail = 1;
        n_cand = 0;
    }
    return n_cand;
}

// More than 21 candidates (three pairs each no longer fit the wave), the general capacity: per scanned lane, lanes = objects
// (two passes, chunks of 64 objects), arg-min walks.
__device__ __forceinline__ void idm_scan_walks(const MdLane* lanes, const MdState& s, const MdConfig& c, int slot, int lane_id, float px,
                                               float py, const MdIdmPlan& plan, const float (&cur_long)[3],
                                               const float (&left_long)[3], FrontBack& fb) {
    constexpr float kInf = 3.0e38f;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        if (plan.ids[i] < 0) continue;  // wave-uniform
        const MdLane* L = &lanes[plan.ids[i]];
        int found_front = 0, found_back = 0;
        for (int j0 = 0; j0 < c.cap; j0 += 64) {
            const int j = j0 + lane_id;
            float kf = kInf, kb = kInf;
            if (j < c.cap && j != slot && md_idm_is_candidate(&s.shape[j], px, py) &&
                md_obj_lane_of(&s, j) == plan.ids[i]) {
                const float lg = md_fb_same_lane_gap(L, cur_long[i], &s.shape[j]);
                if (lg > 0.0f && lg < IDM_MAX_LONG_DIST) kf = lg;
                if (lg < 0.0f && md_fabs(lg) < IDM_MAX_LONG_DIST) kb = md_fabs(lg);
            }
            int jf = j, jb = j;
            wave_argmin(kf, jf);
            wave_argmin(kb, jb);
            if (kf < fb.front_d[i]) { fb.front_d[i] = kf; fb.front[i] = jf; found_front = 1; }
            if (kb < fb.back_d[i]) { fb.back_d[i] = kb; fb.back[i] = jb; found_back = 1; }
        }
        if (found_front && found_back) continue;
        for (int j0 = 0; j0 < c.cap; j0 += 64) {
            const int j = j0 + lane_id;
            float kf = kInf, kb = kInf;
            if (j < c.cap && j != slot && md_idm_is_candidate(&s.shape[j], px, py)) {
                const int ol = md_obj_lane_of(&s, j);
                if (ol >= 0 && ol != plan.ids[i]) {
                    float lg;
                    const int cls = md_fb_neighbour(L, &lanes[ol], cur_long[i], left_long[i], &s.shape[j],
                                                    !found_front, !found_back, &lg);
                    if (cls == 1 && lg > 0.0f && lg < IDM_MAX_LONG_DIST) kf = lg;
                    if (cls == 2 && lg < IDM_MAX_LONG_DIST) kb = lg;
                }
            }
            int jf = j, jb = j;
            wave_argmin(kf, jf);
            wave_argmin(kb, jb);
            if (kf < fb.front_d[i]) { fb.front_d[i] = kf; fb.front[i] = jf; }
            if (kb < fb.back_d[i]) { fb.back_d[i] = kb; fb.back[i] = jb; }
        }
    }
}

// The object scan of one vehicle by the whole wave.  `plan` is wave-uniform (may come back with fail = 1: a traffic
// participant among the candidates), `fb` is the wave-uniform result.
// wave_list: >= 24 ints of LDS private to this wave (the compacted candidate list)
__device__ __forceinline__ void idm_scan_wave(const MdLane* lanes, const MdState& s, const MdConfig& c, int slot, int lane_id,
                              int* wave_list, MdIdmPlan& plan, FrontBack& fb) {
    constexpr float kInf = 3.0e38f;
    front_back_clear(fb);
#pragma unroll
    for (int i = 0; i < 3; ++i) fb.exist[i] = plan.ids[i] >= 0 && !plan.fail;
    if (!plan.fail) {
        const float px = s.shape[slot].cx, py = s.shape[slot].cy;
        // (1) ego longitudinal on the three scanned lanes: lanes 0..2 evaluate one each, then broadcast
        float my_cur = 0.0f;
        {
            const int my_id = (lane_id == 0) ? plan.ids[0] : ((lane_id == 1) ? plan.ids[1] : ((lane_id == 2) ? plan.ids[2] : -1));
            if (my_id >= 0) {
                float tmp;
                md_lane_local(&lanes[my_id], px, py, &my_cur, &tmp);
            }
        }
        float cur_long[3], left_long[3];
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            cur_long[i] = bcast_f(my_cur, i);
            left_long[i] = (plan.ids[i] >= 0) ? lanes[plan.ids[i]].length - cur_long[i] : 0.0f;
        }
        const int n_cand = idm_candidates_wave(s, c, slot, lane_id, px, py, wave_list, plan);
        wave_lds_sync();
        const int npairs = n_cand * 3;
        if (npairs <= 63) {
            // (2) every (scanned lane i, candidate j) pair on its own lane of the wave: ONE Frenet evaluation
            //     per pair (on lane i for a same-lane object, on the object's lane for a connected one)
            float val = 0.0f;
            int meta = 0;  // bit0 same-lane, bit1 lane i precedes obj lane, bit2 obj lane precedes lane i, bits 4-5 i, bits 8.. j
            if (n_cand > 0) {
                const int p = lane_id;
                const int i = p / n_cand;
                const int j = (p < npairs) ? wave_list[p - i * n_cand] : 0;
                const int id_i = (i == 0) ? plan.ids[0] : ((i == 1) ? plan.ids[1] : plan.ids[2]);
                const float cur_i = (i == 0) ? cur_long[0] : ((i == 1) ? cur_long[1] : cur_long[2]);
                if (p < npairs && id_i >= 0) {
                    const int ol = md_obj_lane_of(&s, j);
                    const MdLane* L = &lanes[id_i];
                    int mt = (i << 4) | (j << 8);
                    // one Frenet evaluation per pair: on lane i for a same-lane object, else on the object's lane
                    const MdLane* EL = L;
                    if (ol == id_i) mt |= 1;
                    else if (ol >= 0) {
                        EL = &lanes[ol];
                        mt |= (md_lane_is_previous_of(L, EL) ? 2 : 0) | (md_lane_is_previous_of(EL, L) ? 4 : 0);
                    }
                    if (mt & 7) {
                        float os, ot;
                        md_lane_local(EL, s.shape[j].cx, s.shape[j].cy, &os, &ot);
                        val = (mt & 1) ? os - cur_i : os;
                    }
                    meta = mt;
                }
            }
            // (3) per scanned lane: arg-min reductions (same-lane objects first, connected lanes only if none)
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                if (plan.ids[i] < 0) continue;  // wave-uniform
                int found_front = 0, found_back = 0;
                const bool mine = ((meta >> 4) & 3) == i;
                {
                    const bool same = mine && (meta & 1);
                    float kf = (same && val > 0.0f && val < IDM_MAX_LONG_DIST) ? val : kInf;
                    float kb = (same && val < 0.0f && md_fabs(val) < IDM_MAX_LONG_DIST) ? md_fabs(val) : kInf;
                    int jf = meta >> 8, jb = meta >> 8;
                    wave_argmin(kf, jf);
                    wave_argmin(kb, jb);
                    if (kf < fb.front_d[i]) { fb.front_d[i] = kf; fb.front[i] = jf; found_front = 1; }
                    if (kb < fb.back_d[i]) { fb.back_d[i] = kb; fb.back[i] = jb; found_back = 1; }
                }
                if (found_front && found_back) continue;
                float kf = kInf, kb = kInf;
                if (mine && !(meta & 1) && (meta & 6)) {
                    // md_fb_neighbour's choice: front if (need_front && L precedes OL), else back if (need_back && OL precedes L)
                    if (!found_front && (meta & 2)) {
                        const float lg = val + left_long[i];
                        if (lg > 0.0f && lg < IDM_MAX_LONG_DIST) kf = lg;
                    } else if (!found_back && (meta & 4)) {
                        const float lg = lanes[md_obj_lane_of(&s, meta >> 8)].length - val + cur_long[i];
                        if (lg < IDM_MAX_LONG_DIST) kb = lg;
                    }
                }
                int jf = meta >> 8, jb = meta >> 8;
                wave_argmin(kf, jf);
                wave_argmin(kb, jb);
                if (kf < fb.front_d[i]) { fb.front_d[i] = kf; fb.front[i] = jf; }
                if (kb < fb.back_d[i]) { fb.back_d[i] = kb; fb.back[i] = jb; }
            }
        } else {
            idm_scan_walks(lanes, s, c, slot, lane_id, px, py, plan, cur_long, left_long, fb);   // more than 21 candidates
        }
    }
}

// The same scan in the one-vehicle form (idm_vehicle_wave of the lean single-agent kernel): the minima of each round
// (same-lane objects, then connected-lane objects for the buckets left empty) are LDS atomic mins of gap_key, one per wave
// lane at most, instead of arg-min walks; and the ego's lateral offset and the lane heading 1 m ahead on each scanned lane
// are left at kIdmLatWord / kIdmHeadWord for stage C (its steering lane is one of them), evaluated before the participant
// check so that the fallback has them.  More than 21 candidates (three pairs each no longer fit the wave): the walks.
// wave_list: >= 48 ints of LDS private to this wave (the compacted candidate list, the keys, the carried Frenet data)
__device__ __forceinline__ void idm_scan_wave_keys(const MdLane* lanes, const MdState& s, const MdConfig& c, int slot, int lane_id,
                                   int* wave_list, MdIdmPlan& plan, FrontBack& fb) {
    unsigned long long* keys = reinterpret_cast<unsigned long long*>(wave_list + kIdmKeyWord);
    front_back_clear(fb);
#pragma unroll
    for (int i = 0; i < 3; ++i) fb.exist[i] = plan.ids[i] >= 0 && !plan.fail;
    if (!plan.fail) {
        const float px = s.shape[slot].cx, py = s.shape[slot].cy;
        // (1) ego Frenet coordinates on the three scanned lanes: lanes 0..2 evaluate one each, then broadcast
        float my_cur = 0.0f, my_left = 0.0f;
        {
            const int my_id = (lane_id == 0) ? plan.ids[0] : ((lane_id == 1) ? plan.ids[1] : ((lane_id == 2) ? plan.ids[2] : -1));
            if (my_id >= 0) {
                const MdLane* L = &lanes[my_id];
                float lat;
                md_lane_local(L, px, py, &my_cur, &lat);
                my_left = L->length - my_cur;
                reinterpret_cast<float*>(wave_list)[kIdmLatWord + lane_id] = lat;
                reinterpret_cast<float*>(wave_list)[kIdmHeadWord + lane_id] = md_lane_heading_at(L, my_cur + 1.0f);
            }
            if (lane_id < 6) keys[lane_id] = kNoGap;
        }
        float cur_long[3], left_long[3];
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            cur_long[i] = bcast_f(my_cur, i);
            left_long[i] = (plan.ids[i] >= 0) ? bcast_f(my_left, i) : 0.0f;
        }
        const int n_cand = idm_candidates_wave(s, c, slot, lane_id, px, py, wave_list, plan);
        wave_lds_sync();
        if (n_cand == 0) return;
        const int npairs = n_cand * 3;
        if (npairs <= 63) {
            // (2) every (scanned lane i, candidate j) pair on its own lane of the wave: ONE Frenet evaluation
            //     per pair (on lane i for a same-lane object, on the object's lane for a connected one).  va: the
            //     same-lane gap, or the connected lane's front gap; vb: the connected lane's back gap.
            float va = 0.0f, vb = 0.0f;
            int meta = 0;  // bit0 same-lane, bit1 lane i precedes obj lane, bit2 obj lane precedes lane i, bits 4-5 i, bits 8.. j
            {
                const int p = lane_id;
                const int i = p / n_cand;
                const int j = (p < npairs) ? wave_list[p - i * n_cand] : 0;
                const int id_i = (i == 0) ? plan.ids[0] : ((i == 1) ? plan.ids[1] : plan.ids[2]);
                const float cur_i = (i == 0) ? cur_long[0] : ((i == 1) ? cur_long[1] : cur_long[2]);
                const float left_i = (i == 0) ? left_long[0] : ((i == 1) ? left_long[1] : left_long[2]);
                if (p < npairs && id_i >= 0) {
                    const int ol = md_obj_lane_of(&s, j);
                    const MdLane* L = &lanes[id_i];
                    int mt = (i << 4) | (j << 8);
                    const MdLane* EL = L;
                    if (ol == id_i) mt |= 1;
                    else if (ol >= 0) {
                        EL = &lanes[ol];
                        mt |= (md_lane_is_previous_of(L, EL) ? 2 : 0) | (md_lane_is_previous_of(EL, L) ? 4 : 0);
                    }
                    if (mt & 7) {
                        float os, ot;
                        md_lane_local(EL, s.shape[j].cx, s.shape[j].cy, &os, &ot);
                        if (mt & 1) va = os - cur_i;
                        else {
                            va = os + left_i;                 // md_fb_neighbour's front gap
                            vb = EL->length - os + cur_i;     // and its back gap
                        }
                    }
                    meta = mt;
                }
            }
            {
                const int b0 = ((meta >> 4) & 3) * 2;  // this pair's front bucket; + 1: back
                // (3) round 1: same-lane objects, one gap per pair
                if (meta & 1) {
                    if (va > 0.0f && va < IDM_MAX_LONG_DIST) atomicMin(&keys[b0], gap_key(va, meta >> 8));
                    else if (va < 0.0f && md_fabs(va) < IDM_MAX_LONG_DIST) atomicMin(&keys[b0 + 1], gap_key(md_fabs(va), meta >> 8));
                }
                wave_lds_sync();
                const int found = gap_keys_read(keys, fb);
                // round 2: connected-lane objects, for the buckets of a scanned lane that round 1 did not fill both of
                // (md_fb_neighbour's choice: front if (need_front && L precedes OL), else back if (need_back && OL precedes L))
                bool more = false;
                if (!(meta & 1) && (meta & 6)) {
                    const bool ff = (found >> b0) & 1, fbk = (found >> (b0 + 1)) & 1;
                    if (!(ff && fbk)) {
                        if (!ff && (meta & 2)) {
                            if (va > 0.0f && va < IDM_MAX_LONG_DIST) { atomicMin(&keys[b0], gap_key(va, meta >> 8)); more = true; }
                        } else if (!fbk && (meta & 4)) {
                            if (vb < IDM_MAX_LONG_DIST) { atomicMin(&keys[b0 + 1], gap_key(vb, meta >> 8)); more = true; }
                        }
                    }
                }
                if (__ballot(more) != 0ull) {
                    wave_lds_sync();
                    gap_keys_read(keys, fb);
                }
            }
        } else {
            idm_scan_walks(lanes, s, c, slot, lane_id, px, py, plan, cur_long, left_long, fb);   // more than 21 candidates
        }
    }
}

// One vehicle at a time: plan on lane 0, scan by the wave, decide on lane 0 (the workgroup-per-env kernels' form).
// kKeys (the lean single-agent kernel; the other variants keep the walk form, which their registers prefer): the scan is
// idm_scan_wave_keys and stage C steers by the ego's Frenet data that it carried for the scanned lanes, with no lane record
// load or projection of its own.
template <bool kKeys>
__device__ __forceinline__ void idm_vehicle_wave(const MdWorld& w, const MdLane* lanes, const MdRoad* roads, const MdState& s,
                                 const MdConfig& c, int m, int slot, int lane_id, int* wave_list) {
    MdIdmPlan plan;
    plan.success = plan.use_ref = plan.fail = 0;
    plan.ids[0] = plan.ids[1] = plan.ids[2] = -1;
    const bool st_ = (slot == c.agents_per_env) && lane_id == 0;
    (void)st_;
    MD_FINE_STAMP(st_, 4);
    if (lane_id == 0) md_idm_plan(&w, lanes, roads, &s, &c, m, slot, &plan);
    if constexpr (!kKeys) {
        plan.success = bcast_i(plan.success, 0);
        plan.use_ref = bcast_i(plan.use_ref, 0);
        plan.fail = bcast_i(plan.fail, 0);
        plan.ids[0] = bcast_i(plan.ids[0], 0);
        plan.ids[1] = bcast_i(plan.ids[1], 0);
        plan.ids[2] = bcast_i(plan.ids[2], 0);
        MD_FINE_STAMP(st_, 5);
        FrontBack fb;
        idm_scan_wave(lanes, s, c, slot, lane_id, wave_list, plan, fb);
        MD_FINE_STAMP(st_, 6);
        if (lane_id == 0) md_idm_decide(lanes, roads, &s, slot, &plan, &fb);
    } else {
        plan.success = __builtin_amdgcn_readlane(plan.success, 0);
        plan.use_ref = __builtin_amdgcn_readlane(plan.use_ref, 0);
        plan.fail = __builtin_amdgcn_readlane(plan.fail, 0);
        plan.ids[0] = __builtin_amdgcn_readlane(plan.ids[0], 0);
        plan.ids[1] = __builtin_amdgcn_readlane(plan.ids[1], 0);
        plan.ids[2] = __builtin_amdgcn_readlane(plan.ids[2], 0);
        MD_FINE_STAMP(st_, 5);
        FrontBack fb;
        idm_scan_wave_keys(lanes, s, c, slot, lane_id, wave_list, plan, fb);
        MD_FINE_STAMP(st_, 6);
        if (lane_id == 0) {
            int front_obj;
            float front_dist;
            const float speed_kmh = md_fabs(s.dyn[slot].speed) * 3.6f;
            const int steer = md_idm_policy(lanes, roads, &s, slot, &plan, &fb, &front_obj, &front_dist);
            if (steer < 0) {  // never localised: coast straight
                s.action[2 * slot] = 0.0f;
                s.action[2 * slot + 1] = 0.0f;
            } else {
                // md_idm_policy steers on one of the scanned lanes, so k = 2 below stands for ids[2]: every branch that steers
                // to tidx -/+ 1 needs fb.exist[0 / 2], or a lane inside [avail_lo, avail_hi] with avail_lo >= 0 and
                // avail_hi <= ncur - 1, which md_idm_plan scanned.  A policy that steered anywhere else would need the
                // projection of md_idm_decide here (it costs this kernel 8 more spilled SGPRs, so it is not kept as a fallback).
                const int k = (steer == plan.ids[0]) ? 0 : ((steer == plan.ids[1]) ? 1 : 2);
                const float* wf = reinterpret_cast<const float*>(wave_list);
                md_idm_act(&s, slot, speed_kmh, front_obj, front_dist, wf[kIdmLatWord + k], wf[kIdmHeadWord + k]);
            }
        }
    }
    MD_FINE_STAMP(st_, 7);
}

// All vehicles of `mask` (bit j = slot j0 + j; <= 64 of them): stage A (route bookkeeping) and stage C (lane-change
// policy, PID steering, IDM acceleration) are per-vehicle scalar code, so every vehicle runs them on ITS OWN lane, all
// at once; only the object scans in between go vehicle by vehicle, each by the whole wave.  Same arithmetic per
// vehicle; the decisions do not depend on each other (a decision reads poses / speeds / lanes, and writes only its
// own action, PID and lane-change state).  The one-wave-per-env kernel's form.
__device__ __forceinline__ void idm_group_wave(const MdWorld& w, const MdLane* lanes, const MdRoad* roads, const MdState& s,
                               const MdConfig& c, int m, int j0, unsigned long long mask, int lane_id, int* wave_list) {
    const int my_slot = j0 + lane_id;
    const bool mine = (mask >> lane_id) & 1ull;
    MdIdmPlan plan;
    plan.success = plan.use_ref = plan.fail = 0;
    plan.ids[0] = plan.ids[1] = plan.ids[2] = -1;
    if (mine) md_idm_plan(&w, lanes, roads, &s, &c, m, my_slot, &plan);
    FrontBack fb;
    front_back_clear(fb);
    unsigned long long todo = mask;
    while (todo) {
        const int v = __ffsll((long long)todo) - 1;
        todo &= todo - 1;
        MdIdmPlan up;   // vehicle v's plan, wave-uniform
        up.success = bcast_i(plan.success, v);
        up.use_ref = bcast_i(plan.use_ref, v);
        up.fail = bcast_i(plan.fail, v);
        up.ids[0] = bcast_i(plan.ids[0], v);
        up.ids[1] = bcast_i(plan.ids[1], v);
        up.ids[2] = bcast_i(plan.ids[2], v);
        FrontBack ufb;
        idm_scan_wave(lanes, s, c, j0 + v, lane_id, wave_list, up, ufb);
        wave_lds_sync();   // the next scan reuses wave_list
        if (lane_id == v) {
            plan.fail = up.fail;
            fb = ufb;
        }
    }
    if (mine) md_idm_decide(lanes, roads, &s, my_slot, &plan, &fb);
}

// ------------------------------------------------------------------------------------------------
// Observation / reward / done of one agent by one wave: the nine independent geometric evaluations
// (md_observe_task) run on lanes 0..8 at once, lane 0 gathers them with v_readlane and combines.
// ------------------------------------------------------------------------------------------------
// A/B builds: -DMD_OBS_LOCKSTEP=0 compiles the lean kernel with the serial tasks (md_observe_task) like every other kernel
#ifndef MD_OBS_LOCKSTEP
#define MD_OBS_LOCKSTEP 1
#endif
// One agent per wave (`a` wave-uniform: its context lives in scalar registers) -- the single-agent envs' form.
// kLockstep (the lean kernel): the tasks as md_observe_lane, sixteen lanes on one straight-line sequence of three square
// roots and three quotients instead of nine lanes on four bodies run one after the other; same 45 words in the scratch.
template <bool kLockstep = false>
__device__ __forceinline__ void observe_agent_wave1(const MdLane* lanes, const MdRoad* roads, const MdState& s, const MdConfig& c, int a,
                                    int just_reset, int lane_id, float* wave_scratch /* LDS, MD_OBS_TASKS*5 floats */) {
    MdObsCtx k;
    MD_FINE_STAMP(a == 0 && lane_id == 0, 8);
    md_observe_ctx(lanes, roads, &s, a, &k);
    MD_FINE_STAMP(a == 0 && lane_id == 0, 9);
    if constexpr (kLockstep) {
        // the lanes write one or two words each: the rest of the 45 are zeros (an LDS unit runs a wave's writes in order)
        if (lane_id < MD_OBS_TASKS * 5) wave_scratch[lane_id] = 0.0f;
        md_observe_lane(lane_id, &k, &s, &c, a, wave_scratch);   // lanes 0 .. MD_OBS_LANES - 1 write
    } else if (lane_id < MD_OBS_TASKS) {
        float mine[5];
        md_observe_task(lane_id, &k, &s, &c, a, mine);
#pragma unroll
        for (int i = 0; i < 5; ++i) wave_scratch[lane_id * 5 + i] = mine[i];
    }
    wave_lds_sync();
    MD_FINE_STAMP(a == 0 && lane_id == 0, 10);
    if (lane_id == 0) md_observe_combine(&k, &s, &c, a, just_reset, (const float (*)[5])wave_scratch);
    __builtin_amdgcn_wave_barrier();
    MD_FINE_STAMP(a == 0 && lane_id == 0, 11);
}

// Up to FOUR agents per wave: 16-lane group g serves agent a_base + g (tasks on its lanes 0..8, combine on its
// lane 0): a 40-agent env finishes in 3 rounds of 4 waves instead of 10 (multi-agent kernels only).
constexpr int kObsGroups = 4;
constexpr int kObsScratch = kObsGroups * 48;  // floats of LDS per wave: MD_OBS_TASKS * 5 (= 45) per group, padded

__device__ __forceinline__ void observe_agent_wave(const MdLane* lanes, const MdRoad* roads, const MdState& s, const MdConfig& c, int a_base,
                                   int just_reset, int lane_id, float* wave_scratch /* LDS, kObsScratch floats */) {
    const int g = lane_id >> 4, sub = lane_id & 15;
    const int a = a_base + g;
    const bool live = a < c.agents_per_env;
    float* scratch = wave_scratch + g * 48;
    MdObsCtx k;
    if (live) md_observe_ctx(lanes, roads, &s, a, &k);
    if (live && sub < MD_OBS_TASKS) {
        float mine[5];
        md_observe_task(sub, &k, &s, &c, a, mine);
#pragma unroll
        for (int i = 0; i < 5; ++i) scratch[sub * 5 + i] = mine[i];
    }
    // same wave: the LDS unit executes a wave's ds_write / ds_read in order; the fence keeps the
    // compiler from moving the combining lanes' reads above the other lanes' writes
    wave_lds_sync();
    if (live && sub == 0) md_observe_combine(&k, &s, &c, a, just_reset, (const float (*)[5])scratch);
    __builtin_amdgcn_wave_barrier();
}

// ------------------------------------------------------------------------------------------------
// Traffic trigger (one wave) -- PGTrafficManager.before_step, manager/traffic_manager.py:80-88
// In two halves: the lean kernel runs the search beside the integration and only the fire in its traffic stage.
// ------------------------------------------------------------------------------------------------
// A/B builds: -DMD_TRIGGER_EARLY=0 compiles the lean kernel with both halves in its traffic stage (trigger_env)
#ifndef MD_TRIGGER_EARLY
#define MD_TRIGGER_EARLY 1
#endif
// The search: the lowest pending trigger_order of the env and the trigger road of its block (0x7fffffff: nothing is pending).
// Reads only the PENDING / ALIVE bits and trigger_order / trigger_road of slots that do not drive: nothing a step computes.
constexpr int kNoTrigger = 0x7fffffff;
__device__ __forceinline__ void trigger_search_wave(const MdState& s, const MdConfig& c, int lane_id, int* min_order_out, int* trig_road_out) {
    const int base = 0;  // env-local view
    MD_FINE_STAMP(lane_id == 0, -1);
    *min_order_out = kNoTrigger;
    *trig_road_out = -1;
    int my_min = 0x7fffffff;
    for (int j = lane_id; j < c.cap; j += 64) {
        const int f = s.shape[base + j].flags;
        if ((f & MD_F_PENDING) && (f & MD_F_ALIVE)) {
            const int o = s.nav[base + j].trigger_order;
            my_min = o < my_min ? o : my_min;
        }
    }
    const int min_order = wave_min_i(my_min, my_min != 0x7fffffff, 0x7fffffff);  // wavefront min-reduce
    if (min_order == 0x7fffffff) return;
    // trigger road of that block: lowest slot carrying min_order
    int my_slot = 0x7fffffff;
    for (int j = lane_id; j < c.cap; j += 64) {
        const int f = s.shape[base + j].flags;
        if ((f & MD_F_PENDING) && (f & MD_F_ALIVE) && s.nav[base + j].trigger_order == min_order)
            my_slot = j < my_slot ? j : my_slot;
    }
    const int first_slot = wave_min_i(my_slot, my_slot != 0x7fffffff, 0x7fffffff);
    *min_order_out = min_order;
    *trig_road_out = s.nav[base + first_slot].trigger_road;
    MD_FINE_STAMP(lane_id == 0, 14);
}

// The fire: an agent on the trigger road wakes the block's vehicles (clears their PENDING bits)
__device__ __forceinline__ void trigger_fire_wave(const MdLane* lanes, const MdState& s, const MdConfig& c, int lane_id, int min_order, int trig_road) {
    const int base = 0;  // env-local view
    if (min_order == kNoTrigger) return;
    bool fire = false;
    for (int a = lane_id; a < c.agents_per_env; a += 64) {
        if (!md_drives(s.shape[base + a].flags)) continue;
        const int al = s.nav[base + a].lane;
        if (al >= 0 && lanes[al].road == trig_road) fire = true;
    }
    if (__ballot(fire) == 0ull) return;
    for (int j = lane_id; j < c.cap; j += 64) {
        const int f = s.shape[base + j].flags;
        if ((f & MD_F_PENDING) && (f & MD_F_ALIVE) && s.nav[base + j].trigger_order == min_order)
            s.shape[base + j].flags = f & ~MD_F_PENDING;
    }
}

__device__ __forceinline__ void trigger_env(const MdLane* lanes, const MdState& s, const MdConfig& c, int lane_id) {
    int min_order, trig_road;
    trigger_search_wave(s, c, lane_id, &min_order, &trig_road);
    trigger_fire_wave(lanes, s, c, lane_id, min_order, trig_road);
}

// ------------------------------------------------------------------------------------------------
// Multi-agent lifecycle of one env by the whole workgroup: the block-parallel form of md_lifecycle_env
// (include/md_entity.h, which the oracle runs serially).  Per-agent state machine: one thread per agent; the
// search for a safe spawn place -- (place, vehicle) overlap tests, 8 x 40 of them -- spread over all threads with
// an LDS OR per place; the respawn itself (RNG draws, slot rewrite) on thread 0.  md_lifecycle_env re-scans
// after a respawn; that second scan can never find a place (every safe place of the first scan is marked used,
// the unsafe ones are still occupied), so one scan is exact.  scratch: >= 4 ints of LDS.
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ void lifecycle_block(const MdWorld& w, const MdState& s, const MdConfig& c, int m, int tid, int nthreads,
                                int* scratch) {
    const int A = c.agents_per_env;
    int* cnt_active = scratch;      // agents that keep driving
    int* cnt_dying = scratch + 1;   // bodies waiting out delay_done
    int* hit_mask = scratch + 2;    // bit p: spawn place p is occupied
    int* reserved = scratch + 3;    // parking lot env: bit d: an active agent holds parking space d (md_lifecycle_env)
    int* new_slot = scratch + 4;    // slot refilled in this step (-1: none) and its row of the spawn-route table: the
    int* new_ri = scratch + 5;      //   96 words of its route are copied by the whole workgroup, not by the one thread
    const bool parking = c.ma_kind == MD_MA_PARKING_LOT;
    if (tid == 0) {
        s.env_steps[0] += 1;
        *cnt_active = 0;
        *cnt_dying = 0;
        *hit_mask = 0;
        *reserved = 0;
        *new_slot = -1;
    }
    __syncthreads();
    for (int a = tid; a < A; a += nthreads) {
        MdShape* sh = &s.shape[a];
        MdNav* nav = &s.nav[a];
        if (!(sh->flags & MD_F_ALIVE)) continue;
        bool count_down = true;
        if (!(sh->flags & MD_F_STATIC)) {
            const uint32_t fl = s.flags[a];
            if (nav->done || (fl & MD_FL_TRUNCATED)) {
                if ((fl & MD_FL_ARRIVE_DEST) || c.delay_done <= 0) {
                    sh->flags &= ~MD_F_ALIVE;
                    count_down = false;
                } else {
                    sh->flags |= MD_F_STATIC;
                    nav->timer = c.delay_done;
                    s.dyn[a].speed = 0.0f;
                }
            } else {
                atomicAdd(cnt_active, 1);
                if (parking && nav->toll_entry > 0) atomicOr(reserved, 1 << (nav->toll_entry - 1));
                count_down = false;
            }
        }
        if (count_down) {
            nav->timer -= 1;
            if (nav->timer <= 0) sh->flags &= ~MD_F_ALIVE;
            else atomicAdd(cnt_dying, 1);
        }
    }
    __syncthreads();
    const bool horizon_open = !(c.horizon > 0 && s.env_steps[0] >= c.horizon);
    const bool may_respawn = c.allow_respawn && horizon_open && w.spawn_off != nullptr && (*cnt_active + *cnt_dying < A);
    if (may_respawn) {  // block-uniform
        const int p0 = w.spawn_off[m];
        const int np_ = min(w.spawn_off[m + 1] - p0, 32);
        for (int idx = tid; idx < np_ * c.cap; idx += nthreads) {
            const int p = idx / c.cap, j = idx - p * c.cap;
            const MdShape o = s.shape[j];
            if (!md_present(o.flags) || md_kind_of(o.flags) != MD_KIND_VEHICLE) continue;
            const float* pl = w.spawn_place + 8 * (size_t)(p0 + p);
            if (md_obb_obb(pl[0], pl[1], pl[2], pl[3], MD_RESPAWN_HALF_LEN, MD_RESPAWN_HALF_WID, o.cx, o.cy, o.c, o.s, o.hl, o.hw))
                atomicOr(hit_mask, 1 << p);
        }
        __syncthreads();
        if (tid == 0) {
            const uint32_t all = np_ >= 32 ? 0xFFFFFFFFu : ((1u << np_) - 1u);
            uint32_t safe = ~(uint32_t)(*hit_mask) & all;
            const int n_in = parking ? np_ - c.n_parking : 0;
            uint32_t avail = parking ? (((1u << c.n_parking) - 1u) & ~(uint32_t)(*reserved)) : 0u;
            if (parking && avail == 0u) safe &= ~((1u << n_in) - 1u);   // no free space: the entrances stay shut
            const int n_safe = __popc(safe);
            int slot = -1;
            for (int a = 0; a < A; ++a)
                if (!(s.shape[a].flags & MD_F_ALIVE)) { slot = a; break; }
            if (n_safe > 0) {
                int k = (int)(md_rng_next(s.rng) % (uint32_t)n_safe);   // ascending place order, like the serial `safe[]`
                while (k-- > 0) safe &= safe - 1;
                const int p = __ffs((int)safe) - 1;
                if (slot >= 0) {
                    const float* pl = w.spawn_place + 8 * (size_t)(p0 + p);
                    int dest = 0, space = 0;
                    if (!parking) dest = (int)(md_rng_next(s.rng) % (uint32_t)w.n_dest);
                    else if (p < n_in) {
                        dest = md_kth_set_bit(avail, (int)(md_rng_next(s.rng) % (uint32_t)__popc(avail)));
                        space = dest + 1;
                    } else dest = c.n_parking + (int)(md_rng_next(s.rng) % (uint32_t)(w.n_dest - c.n_parking));
                    const size_t ri = ((size_t)(p0 + p) * w.n_dest + dest);
                    const int32_t* rt = w.spawn_route + ri * 2 * MD_ROUTE_LEN;
                    MdShape* sh = &s.shape[slot];
                    sh->cx = pl[0];
                    sh->cy = pl[1];
                    sh->c = pl[2];
                    sh->s = pl[3];
                    sh->flags = MD_KIND_VEHICLE | MD_F_ALIVE | MD_F_AGENT | MD_F_SPAWNED;
                    sh->aux = -1;
                    MdDyn* d = &s.dyn[slot];
                    d->heading = pl[4];
                    d->speed = 0.0f;
                    d->steering = 0.0f;
                    d->throttle = 0.0f;
                    d->last_x = pl[0];
                    d->last_y = pl[1];
                    d->last_c = pl[2];
                    d->last_s = pl[3];
                    MdNav* nav = &s.nav[slot];
                    nav->lane = w.spawn_lane[p0 + p];
                    nav->route_len = w.spawn_route_meta[2 * ri];
                    nav->ck0 = 0;
                    nav->ck1 = (nav->route_len <= 2) ? 0 : 1;
                    nav->target_lane = -1;
                    nav->timer = 0;
                    nav->steps = 0;
                    nav->done = 0;
                    nav->toll_state = nav->toll_entry = nav->toll_exit = 0;
                    nav->toll_entry = space;
                    md_agent_policy_init(&s, &c, slot);
                    if (c.random_agent_model && w.n_vclass > 0) md_draw_vehicle_class(&w, &s, slot);
                    s.final_lane[slot] = w.spawn_route_meta[2 * ri + 1];
                    *new_slot = slot;
                    *new_ri = (int)ri;
                    nav->road0 = rt[MD_ROUTE_LEN + nav->ck0];
                    nav->road1 = rt[MD_ROUTE_LEN + nav->ck1];
                    s.pid[slot].energy = 0.0f;
                    s.flags[slot] = 0;
                    s.action[2 * slot] = 0.0f;
                    s.action[2 * slot + 1] = 0.0f;
                    s.agent_id[slot] = s.next_agent_id[0];
                    s.next_agent_id[0] += 1;
                    *cnt_active += 1;
                }
            }
        }
        __syncthreads();
        if (*new_slot >= 0) {   // block-uniform
            const int slot = *new_slot;
            const int32_t* rt = w.spawn_route + (size_t)(*new_ri) * 2 * MD_ROUTE_LEN;
            for (int q = tid; q < 2 * MD_ROUTE_LEN; q += nthreads) {
                if (q < MD_ROUTE_LEN) s.route_nodes[(size_t)slot * MD_ROUTE_LEN + q] = rt[q];
                else s.route_roads[(size_t)slot * MD_ROUTE_LEN + (q - MD_ROUTE_LEN)] = rt[q];
            }
        }
    }
    // episode over: nobody left and nobody can come back
    if (tid == 0 && c.auto_reset && *cnt_active == 0 && !(c.allow_respawn && horizon_open)) s.need_reset[0] = 1;
    __syncthreads();
}

// ------------------------------------------------------------------------------------------------
// The per-env kernel.  PH selects the phases (a compile-time mask: the single-phase entry points
// instantiate it with one bit, md_step with all of them).
// ------------------------------------------------------------------------------------------------
// Cooperative 16-byte copy (both sides 16-byte aligned, nbytes a multiple of 16).
__device__ __forceinline__ void copy16(void* dst, const void* src, int nbytes, int tid, int nthreads) {
    uint4* d = reinterpret_cast<uint4*>(dst);
    const uint4* s = reinterpret_cast<const uint4*>(src);
    for (int i = tid; i < (nbytes >> 4); i += nthreads) d[i] = s[i];
}

// STAGE_MAP: copy the env's lane + road tables into LDS (small maps: <= kStageMaxLanes lanes); big maps
// (intersections, roundabouts: 100-200 lanes) are read through L1/L2 instead -- staging 30 KB per env per
// step would cost more HBM traffic and LDS occupancy than it saves in latency.
constexpr int kStageMaxLanes = 64;
constexpr int kWideMaxEnvs = 640;   // multi-agent batches up to this many envs step with eight waves per env (see launch<>)
constexpr uint32_t kRemovedMark = 0xFFFFFFFFu;  // l_cfl value of a traffic slot removed in this step

// k-th set bit of (hi:lo), -1 if there is none
__device__ __forceinline__ int kth_bit(unsigned long long lo, unsigned long long hi, int k) {
    int slot = -1;
    while (k >= 0) {
        if (lo) {
            slot = __ffsll((long long)lo) - 1;
            lo &= lo - 1;
        } else if (hi) {
            slot = 64 + __ffsll((long long)hi) - 1;
            hi &= hi - 1;
        } else {
            return -1;
        }
        --k;
    }
    return slot;
}

// The staged records of one env in LDS, at the offsets of the kernel's layout (env_lds, wave_env_lds, scenario_lds).
struct EnvImage {
    MdShape* shape;
    MdDyn* dyn;
    MdPid* pid;
    MdParam* param;
    MdNav* nav;
    float* action;  // [cap][2]
    uint32_t* flags;
    int32_t* final_lane;  // nullptr where the kernel does not stage it (scenes)
};

// The env-local view of the state: gv with its hot arrays in the image
__device__ __forceinline__ MdState local_view(const MdState& gv, const EnvImage& img) {
    MdState s = gv;
    s.shape = img.shape;
    s.dyn = img.dyn;
    s.nav = img.nav;
    s.pid = img.pid;
    s.action = img.action;
    s.flags = img.flags;
    s.param = img.param;
    s.final_lane = img.final_lane;
    return s;
}

// The slots that drive (md_drives), as a mask of up to 128 slots (hi:lo), the same in every lane of the wave
struct SlotMask { unsigned long long lo, hi; };
static_assert(MD_MAX_CAP <= 128, "drive_mask: two 64-bit words per env");
__device__ __forceinline__ SlotMask drive_mask(const MdShape* shape, int cap, int lane) {
    SlotMask m = {0ull, 0ull};
    for (int j0 = 0; j0 < cap; j0 += 64) {
        const int j = j0 + lane;
        const unsigned long long mk = __ballot(j < cap && md_drives(shape[j < cap ? j : 0].flags));
        if (j0 == 0) m.lo = mk;
        else m.hi = mk;
    }
    return m;
}
// ... its agents' share (slots [0, agents): the ones whose contacts are tested)
__device__ __forceinline__ SlotMask agent_share(SlotMask m, int agents) {
    m.lo &= agents >= 64 ? ~0ull : ((1ull << agents) - 1ull);
    m.hi &= agents <= 64 ? 0ull : (agents >= 128 ? ~0ull : ((1ull << (agents - 64)) - 1ull));
    return m;
}
__device__ __forceinline__ int popc(SlotMask m) { return __popcll(m.lo) + __popcll(m.hi); }

// RESPAWN: the variant for everything off the headline path -- traffic modes respawn / hybrid / replay, detected
// sets for the `num_others` block (compiled apart: its slot-rewriting code costs the common trigger-mode
// kernel 8 VGPRs and one wave of occupancy when it is merely branched around).
// Threads per env workgroup.  256 = 4 waves: measured best (tools/run_blocks.sh rebuilds with -DMD_ENV_BLOCK=128/64).
#ifndef MD_ENV_BLOCK
#define MD_ENV_BLOCK 256
#endif
#ifndef MD_ENV_WAVES_EU
#define MD_ENV_WAVES_EU 7
#endif
// ---- what a lean launch pins ----
// The lean kernels of md_step -- env_kernel<PH_ALL, *, false, false> and wave_step_kernel<false> -- are launched only while every
// field listed here has its pinned value: variant<PH_ALL>() (the launch predicate) asks lean_pins_hold(), and the kernels overwrite
// their by-value copies of the arguments with the same list (lean_pins_fold; all but the staged-map env_kernel, see there), so the
// branches on these fields fold away instead of riding along in SGPRs.  ONE list for both sides: a field taken out of the predicate
// is no longer folded.  Only fields the predicate itself tests belong here; a field that merely happens to be unused in these
// configs does not.
//   zero(int32 MdConfig field): the field is 0;  null(MdState pointer): the pointer is null
template <class Config, class State, class Zero, class Null>
__host__ __device__ inline void lean_pins(Config& c, State& s, Zero zero, Null null) {
    zero(c.is_multi_agent);   // the multi-agent envs have their own variant (MULTI)
    zero(c.traffic_mode);     // trigger mode; respawn / hybrid / replay: the RESPAWN variant (scenario mode: its own kernel)
    zero(c.agent_idm);        // the caller's actions; IDMPolicy / LaneChangePolicy agents: the RESPAWN variant
    zero(c.num_others);       // the `others` block needs the detected sets
    null(s.detected);         // tracked by the RESPAWN / MULTI variants only
}
__host__ __device__ inline bool lean_pins_hold(const MdState& s, const MdConfig& c) {
    bool ok = true;
    lean_pins(c, s, [&ok](const int32_t& v) { ok = ok && v == 0; }, [&ok](const void* p) { ok = ok && p == nullptr; });
    return ok;
}
__host__ __device__ inline void lean_pins_fold(MdState& s, MdConfig& c) {
    lean_pins(c, s, [](int32_t& v) { v = 0; }, [](auto*& p) { p = nullptr; });
}

// MULTI: multi-agent envs (lifecycle phase, reference order of the IDM); single-agent envs plan the traffic ahead.
// Register budget: the single-agent fused step is compiled for 7 waves per SIMD (72 VGPRs / 96 SGPRs): measured
// 123 us against 133 us at the compiler's own choice (6 waves) and 131 us at 8 (64 VGPRs, more spills) --
// the step is latency-bound, so resident workgroups per CU count.  Other instantiations keep the default.
template <int PH, bool RESPAWN, bool MULTI>
constexpr int env_waves_per_eu() { return (PH == PH_ALL && !RESPAWN && !MULTI && MD_ENV_BLOCK >= 128) ? MD_ENV_WAVES_EU : 0; }

// LDS image of one env in env_kernel: its dynamic state, the staged map tables (n_lanes / n_roads: 0 when not staged) and the
// stages' scratch.  The lidar-only kernel stages nothing but the shapes: asking for the full image would cost it occupancy.
struct EnvLds { uint32_t shape, dyn, nav, pid, action, flags, lanes, roads, scratch, param, final_lane, det, onlane, cfl, tk, bytes; };
__host__ __device__ inline EnvLds env_lds(int cap, int agents, int n_lanes, int n_roads, int waves, bool multi, bool lidar_only) {
    EnvLds L;
    L.shape = 0;                                                     // the 16-B records are staged as uint4
    L.dyn = L.shape + (uint32_t)cap * sizeof(MdShape);
    L.nav = L.dyn + (uint32_t)cap * sizeof(MdDyn);
    L.pid = L.nav + (uint32_t)cap * sizeof(MdNav);
    L.action = L.pid + (uint32_t)cap * sizeof(MdPid);                  // [cap][2] floats
    L.flags = L.action + (uint32_t)cap * 2 * sizeof(float);
    L.lanes = align_up(L.flags + (uint32_t)cap * sizeof(uint32_t), 16);  // map tables: copy16
    L.roads = L.lanes + (uint32_t)n_lanes * sizeof(MdLane);
    L.scratch = L.roads + (uint32_t)n_roads * sizeof(MdRoad);         // [waves][kObsScratch or 48] floats: per-wave observe results
    L.param = L.scratch + (uint32_t)waves * (multi ? kObsScratch : 48) * sizeof(float);   // 16-B aligned like the map tables
    L.final_lane = L.param + (uint32_t)cap * sizeof(MdParam);
    L.det = L.final_lane + align_up(cap, 2) * sizeof(int32_t);      // [agents][2] detected sets (8-B aligned)
    // the fused step's localize / contacts results ([cap] each, merged into flags afterwards) share their words with the
    // lifecycle's 8 scratch words, which run before them (MULTI)
    L.onlane = L.det + (uint32_t)agents * 2 * sizeof(unsigned long long);
    L.cfl = L.onlane + (uint32_t)cap * sizeof(uint32_t);
    const uint32_t shared_words = 2 * cap > 8 ? 2 * cap : 8;
    L.tk = L.onlane + shared_words * sizeof(uint32_t);               // ticket counters of the locate / observe / lidar stages
    L.bytes = lidar_only ? L.dyn : L.tk + 3 * sizeof(int);
    return L;
}

// BLK: threads of the workgroup (MD_ENV_BLOCK; multi-agent batches small enough to stay resident are also instantiated with 512:
// eight waves share an env's 20-40 agents -- lifecycle search, contacts, observe groups, lidar sectors -- instead of four).
template <int PH, bool STAGE_MAP, bool RESPAWN = false, bool MULTI = false, int BLK = MD_ENV_BLOCK>
__global__ __launch_bounds__(BLK)
__attribute__((amdgpu_waves_per_eu(env_waves_per_eu<PH, RESPAWN, MULTI>() ? env_waves_per_eu<PH, RESPAWN, MULTI>() : 1,
                                   env_waves_per_eu<PH, RESPAWN, MULTI>() ? env_waves_per_eu<PH, RESPAWN, MULTI>() : 8)))
void env_kernel(MdWorld w, MdState g, MdConfig c, float* lidar_out,
                                                  int lidar_stride, int lidar_offset) {
    constexpr int kBlock = BLK;
    constexpr int kWaves = kBlock / 64;
    // the IDM's one-vehicle form with LDS gap keys: the lean kernel only; the staged-map, respawn and multi-agent variants
    // keep the walk form (the keys cost them registers)
    constexpr bool kIdmKeys = !STAGE_MAP && !RESPAWN && !MULTI;
    // the road-first localisation: the lean kernel's one- and two-vehicles-per-wave forms (and the test entry point md_localize_road_first)
    constexpr bool kLocRoadFirst = PH == PH_ALL ? kIdmKeys : PH == PH_LOCALIZE_ROAD_FIRST;
    // the agent's observation tasks in lock-step (md_observe_lane): the lean kernel only
    constexpr bool kObsLockstep = MD_OBS_LOCKSTEP && PH == PH_ALL && kIdmKeys;
    // The lean launch: variant<PH_ALL>() guarantees the pins.  Not in the staged-map kernel: folded, its scratch grows from 16 to
    // 80 B per lane (EXPERIMENTS.md, "Lean kernels fold what their launch pins"), so it keeps reading the fields.
    if constexpr (PH == PH_ALL && !RESPAWN && !MULTI && !STAGE_MAP) lean_pins_fold(g, c);
    if ((int)blockIdx.x >= c.n_envs) return;
#ifdef MD_STAMP
    const int e = g_env_order ? g_env_order[blockIdx.x] : (int)blockIdx.x;   // diagnostic: launch-order experiments
#else
    const int e = blockIdx.x;
#endif
    const int tid = threadIdx.x;
    const int wave = tid >> 6, lane = tid & 63;
    const int cap = c.cap;

    // ---- LDS image of this env (env_lds) ----
    // static tables of this env's map: read many times by the serial per-vehicle logic, so (small maps) they sit in
    // LDS too (a dependent chain of HBM/L2 round trips otherwise).  The movers' routes stay in global memory: the two
    // road ids the step needs are cached in MdNav (road0 / road1), the arrays are touched only when a cursor advances.
    const int n_stage_lanes = STAGE_MAP ? w.max_lanes : 0, n_stage_roads = STAGE_MAP ? w.max_roads : 0;
    constexpr bool kLidarOnly = (PH == PH_LIDAR);
    const EnvLds L = env_lds(cap, c.agents_per_env, n_stage_lanes, n_stage_roads, kWaves, MULTI, kLidarOnly);
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    MdShape* l_shape = reinterpret_cast<MdShape*>(smem + L.shape);
    MdDyn* l_dyn = reinterpret_cast<MdDyn*>(smem + L.dyn);
    MdNav* l_nav = reinterpret_cast<MdNav*>(smem + L.nav);
    MdPid* l_pid = reinterpret_cast<MdPid*>(smem + L.pid);
    float* l_action = reinterpret_cast<float*>(smem + L.action);
    uint32_t* l_flags = reinterpret_cast<uint32_t*>(smem + L.flags);
    MdLane* l_lanes = reinterpret_cast<MdLane*>(smem + L.lanes);
    MdRoad* l_roads = reinterpret_cast<MdRoad*>(smem + L.roads);
    float* l_scratch = reinterpret_cast<float*>(smem + L.scratch) + wave * (MULTI ? kObsScratch : 48);
    MdParam* l_param = reinterpret_cast<MdParam*>(smem + L.param);
    int32_t* l_final = reinterpret_cast<int32_t*>(smem + L.final_lane);
    unsigned long long* l_det = reinterpret_cast<unsigned long long*>(smem + L.det);
    const EnvImage img = {l_shape, l_dyn, l_pid, l_param, l_nav, l_action, l_flags, l_final};
    uint32_t* l_onlane = reinterpret_cast<uint32_t*>(smem + L.onlane);
    uint32_t* l_cfl = reinterpret_cast<uint32_t*>(smem + L.cfl);
    int* l_tk = reinterpret_cast<int*>(smem + L.tk);
    // detected sets: only the RESPAWN ("everything else") and MULTI variants carry the tracking code; launch<> picks
    // one of them whenever MdState.detected is set, so the lean trigger-mode kernel pays nothing for it
    const bool track_det = (PH == PH_ALL) && (RESPAWN || MULTI) && g.detected != nullptr;

    const MdState gv = md_env_view(&g, &c, e);  // this env's slices of the global arrays
    // The reset flag is loaded first but nothing below waits for it: the live state is staged
    // unconditionally (one round trip) and only a resetting env re-stages from the snapshot.
    const int reset_flag = (PH & PH_RESET) ? gv.need_reset[0] : 0;

    MD_STAMP_AT(0);
    const bool kFusedAct = (PH == PH_ALL) && gv.agent_action != nullptr;  // md_step only: agents' actions from the caller's buffer
    const MdLane* lanes;
    const MdRoad* roads;
    if (STAGE_MAP) {
        lanes = l_lanes;
        roads = l_roads;
    } else {
        lanes = w.lanes + w.lane_off[w.env_map[e]];
        roads = w.roads + w.road_off[w.env_map[e]];
    }
    if (kLidarOnly) {
        copy16(l_shape, gv.shape, cap * (int)sizeof(MdShape), tid, kBlock);
    } else if (kBlock >= 256) {
        // Fast path: ALL global loads of the stage-in are issued before the first LDS store, so the whole image
        // arrives in one memory round trip (a chain of copy loops waits for each loop's loads in turn: 7 trips,
        // ~9 k cycles per env).  16-B units per array at cap <= 128: shape/dyn/pid/param <= 256 (one per thread),
        // nav <= 512, routes <= 1536: the first 256 / 512 units go through registers, the rest (cap > 64 / > 42) in tail loops.
        const int n32 = cap * 2, n64 = cap * 4;
        const uint4* g_shape = reinterpret_cast<const uint4*>(gv.shape);
        const uint4* g_dyn = reinterpret_cast<const uint4*>(gv.dyn);
        const uint4* g_pid = reinterpret_cast<const uint4*>(gv.pid);
        const uint4* g_param = reinterpret_cast<const uint4*>(gv.param);
        const uint4* g_nav = reinterpret_cast<const uint4*>(gv.nav);
        uint4 r_shape, r_dyn, r_pid, r_param, r_nav0;
        float2 r_act;
        uint32_t r_fl;
        int r_fin;
        const bool p32 = tid < n32, pc = tid < cap;
        if (p32) {
            r_shape = ld_stream(&g_shape[tid]);
            r_dyn = ld_stream(&g_dyn[tid]);
            r_pid = ld_stream(&g_pid[tid]);
            r_param = ld_stream(&g_param[tid]);
        }
        if (tid < n64) r_nav0 = ld_stream(&g_nav[tid]);
        if (pc) {
            r_act = (kFusedAct && tid < c.agents_per_env) ? reinterpret_cast<const float2*>(gv.agent_action)[tid]
                                                          : reinterpret_cast<const float2*>(gv.action)[tid];
            r_fl = gv.flags[tid];
            r_fin = gv.final_lane ? gv.final_lane[tid] : 0;
        }
        if (STAGE_MAP) {
            const int m = w.env_map[e];
            const int lo = w.lane_off[m], ro = w.road_off[m];
            copy16(l_lanes, w.lanes + lo, (w.lane_off[m + 1] - lo) * (int)sizeof(MdLane), tid, kBlock);
            copy16(l_roads, w.roads + ro, (w.road_off[m + 1] - ro) * (int)sizeof(MdRoad), tid, kBlock);
        }
        if (p32) {
            reinterpret_cast<uint4*>(l_shape)[tid] = r_shape;
            reinterpret_cast<uint4*>(l_dyn)[tid] = r_dyn;
            reinterpret_cast<uint4*>(l_pid)[tid] = r_pid;
            reinterpret_cast<uint4*>(l_param)[tid] = r_param;
        }
        if (tid < n64) reinterpret_cast<uint4*>(l_nav)[tid] = r_nav0;
        for (int i = tid + kBlock; i < n64; i += kBlock) reinterpret_cast<uint4*>(l_nav)[i] = g_nav[i];
        if (pc) {
            reinterpret_cast<float2*>(l_action)[tid] = r_act;
            l_flags[tid] = r_fl;
            l_final[tid] = r_fin;
        }
        if (track_det)
            for (int j = tid; j < 2 * c.agents_per_env; j += kBlock) l_det[j] = 0ull;
    } else {
        copy16(l_shape, gv.shape, cap * (int)sizeof(MdShape), tid, kBlock);
        if (STAGE_MAP) {
            const int m = w.env_map[e];
            const int lo = w.lane_off[m], ro = w.road_off[m];
            copy16(l_lanes, w.lanes + lo, (w.lane_off[m + 1] - lo) * (int)sizeof(MdLane), tid, kBlock);
            copy16(l_roads, w.roads + ro, (w.road_off[m + 1] - ro) * (int)sizeof(MdRoad), tid, kBlock);
        }
        copy16(l_dyn, gv.dyn, cap * (int)sizeof(MdDyn), tid, kBlock);
        copy16(l_nav, gv.nav, cap * (int)sizeof(MdNav), tid, kBlock);
        copy16(l_pid, gv.pid, cap * (int)sizeof(MdPid), tid, kBlock);
        copy16(l_param, gv.param, cap * (int)sizeof(MdParam), tid, kBlock);
        for (int j = tid; j < cap; j += kBlock) {
            const float* src = (kFusedAct && j < c.agents_per_env) ? gv.agent_action : gv.action;
            l_action[2 * j] = src[2 * j];
            l_action[2 * j + 1] = src[2 * j + 1];
            l_flags[j] = gv.flags[j];
            l_final[j] = gv.final_lane ? gv.final_lane[j] : 0;
        }
        if (track_det)
            for (int j = tid; j < 2 * c.agents_per_env; j += kBlock) l_det[j] = 0ull;
    }
    const bool do_reset = reset_flag != 0;  // block-uniform
    const int just_reset = do_reset ? 1 : 0;
    if (do_reset && !kLidarOnly) {
        __syncthreads();
        copy16(l_shape, gv.shape0, cap * (int)sizeof(MdShape), tid, kBlock);
        copy16(l_dyn, gv.dyn0, cap * (int)sizeof(MdDyn), tid, kBlock);
        copy16(l_nav, gv.nav0, cap * (int)sizeof(MdNav), tid, kBlock);
        copy16(l_pid, gv.pid0, cap * (int)sizeof(MdPid), tid, kBlock);
        if (MULTI && c.random_agent_model && gv.param0)   // respawns drew new vehicle classes: back to the reset ones
            copy16(l_param, gv.param0, cap * (int)sizeof(MdParam), tid, kBlock);
        for (int j = tid; j < cap; j += kBlock) {
            l_action[2 * j] = 0.0f;
            l_action[2 * j + 1] = 0.0f;
            l_flags[j] = 0u;
        }
        if (MULTI || (RESPAWN && (c.traffic_mode == 1 || c.traffic_mode == 2))) {  // respawns rewrote the routes: restore them too
            for (int i = tid; i < cap * MD_ROUTE_LEN; i += kBlock) {
                gv.route_nodes[i] = gv.route_nodes0[i];
                gv.route_roads[i] = gv.route_roads0[i];
            }
            for (int j = tid; j < cap; j += kBlock) l_final[j] = gv.final_lane0[j];
        }
        if (MULTI) {
            for (int j = tid; j < cap; j += kBlock) gv.agent_id[j] = j;
            if (tid == 0) {
                gv.env_steps[0] = 0;
                int n0 = 0;  // agents present at reset: all slots, or one per spawn point with num_agents = -1
                for (int j = 0; j < c.agents_per_env; ++j) n0 += (gv.shape0[j].flags & MD_F_ALIVE) ? 1 : 0;
                gv.next_agent_id[0] = n0;
            }
        }
    }
    MdState s = local_view(gv, img);  // env-local view whose hot arrays live in LDS
    if (kLidarOnly) {   // the lidar-only image holds the shapes alone
        s = gv;
        s.shape = l_shape;
    }
    if ((MULTI || PH == PH_ALL) && tid == 0) l_tk[0] = l_tk[1] = l_tk[2] = 0;
    __syncthreads();
    MD_STAMP_AT(1);
    // Lean kernel: the search half of the next step's trigger runs here, on the last wave, which owns no slot of the integrate
    // stage below.  It reads PENDING / ALIVE and trigger_order / trigger_road of waiting slots only, which no stage before the
    // traffic stage writes (the reset step's too: the snapshot is staged by now).  The same wave fires, behind the locate
    // stage's barrier; nothing stays in registers in between.
    constexpr bool kTriggerEarly = MD_TRIGGER_EARLY && PH == PH_ALL && kIdmKeys && kWaves > 1;
    // its two words (min order, trigger road): words 46 / 47 of the last wave's own scratch (env_lds: 48 per wave), which the observe
    // tasks (45 floats) never touch and the wave's IDM (ints 0 .. 35) uses only after the fire has read them
    constexpr int kTrigWord = (kWaves - 1) * 48 + 46;
    if (kTriggerEarly && wave == kWaves - 1) {
        int min_order, trig_road;
        trigger_search_wave(s, c, lane, &min_order, &trig_road);
        if (lane == 0) {
            int* l_trig = reinterpret_cast<int*>(smem + L.scratch) + kTrigWord;
            l_trig[0] = min_order;
            l_trig[1] = trig_road;
        }
    }

    if ((PH & PH_LIFECYCLE) && MULTI && !just_reset) {
        lifecycle_block(w, s, c, w.env_map[e], tid, kBlock, reinterpret_cast<int*>(l_onlane));
    }

    // Single-agent envs plan the traffic one step AHEAD (see the observe stage below): the IDM decision of step
    // t+1 depends only on the state at the end of step t, so it is taken there, on the waves that would
    // otherwise idle behind the agent's observe chain.  Multi-agent envs keep the reference order (the
    // lifecycle at the start of a step may respawn agents the IDM would have to see).
    constexpr bool kFused = (PH == PH_ALL);
    // agent_policy = IDMPolicy (single-agent envs): the agents are planned like the traffic, in the reference's order
    // (decide, then move): the observation reports the action applied in THIS step.  Never in the lean fused variant:
    // the launcher sends such configs to the RESPAWN one.
    const bool agent_idm = (kFused && !RESPAWN && !MULTI) ? false : (c.agent_idm == MD_AGENT_IDM);
    // agent_policy = LaneChangePolicy: each agent's decoded action is turned into the lane-change PIDs' steering just before it
    // is integrated (md_lane_change_act, same thread as the integration).  Only the RESPAWN and MULTI variants carry the code.
    const bool lane_change = (RESPAWN || MULTI) && c.agent_idm == MD_AGENT_LANE_CHANGE;
    constexpr bool kPlanAhead = kFused && kWaves > 1 && !MULTI;
    const bool plan_ahead = kPlanAhead && !agent_idm;
    if ((PH & PH_IDM) && !just_reset && !plan_ahead) {
        if (wave == 0) trigger_env(lanes, s, c, lane);
        __syncthreads();
        MD_STAMP_AT(2);
        for (int j = (agent_idm ? 0 : c.agents_per_env) + wave; j < cap; j += kWaves) {
            const int f = s.shape[j].flags;  // wave-uniform
            if (md_drives(f) && (agent_idm || !(f & MD_F_AGENT))) idm_vehicle_wave<kIdmKeys>(w, lanes, roads, s, c, w.env_map[e], j, lane, reinterpret_cast<int*>(l_scratch));
        }
        __syncthreads();
    }
    MD_STAMP_AT(3);
    if ((PH & PH_INTEGRATE) && !just_reset) {
        for (int j = tid; j < cap; j += kBlock) {
            if (lane_change && j < c.agents_per_env) {
                const int f = s.shape[j].flags;   // not on the step the slot was (re)spawned: it is not integrated then
                if (md_drives(f) && !(f & MD_F_SPAWNED)) md_lane_change_act(lanes, roads, &s, j);
            }
            if (RESPAWN) md_advance_mover(&s, &c, j);  // the non-trigger traffic modes' kernel (respawn / hybrid / replay)
            else md_integrate_mover(&s, &c, j);
        }
        if (!RESPAWN)  // user-spawned pedestrians / cyclists (a loop of its own: inside the one above it costs spills)
            for (int j = tid; j < cap; j += kBlock) md_walk_mover(&s, &c, j);
        __syncthreads();
    }
    MD_STAMP_AT(4);
    unsigned long long drv_lo = 0ull, drv_hi = 0ull;  // fused step: the slots that drive in this step (wave-uniform)
    if (kFused) {
        // Localisation and contacts of a vehicle are independent of each other (both only read the integrated
        // poses and the map), so they share ONE stage: work items = [localize of every driving vehicle, then
        // contacts of every driving vehicle], dealt round-robin to the waves.  With the usual 1-3 driving
        // vehicles per env everything fits one round instead of two phases behind two barriers.
        const SlotMask drv = drive_mask(s.shape, cap, lane);
        drv_lo = drv.lo;
        drv_hi = drv.hi;
        // contacts only for agents (traffic's crash flags are never read): their slots are the first A
        const SlotMask adrv = agent_share(drv, c.agents_per_env);
        const unsigned long long adrv_lo = adrv.lo, adrv_hi = adrv.hi;
        const int nd = popc(drv), na = popc(adrv);
        if (MULTI) {
            // every workgroup of a multi-agent batch is resident at once: the launch lasts as long as its slowest env, and inside
            // an env as long as the wave with the most expensive items -- the waves take the items by ticket, contacts (the
            // expensive ones in a crowd) first
            const int npair = (nd + 1) >> 1;
            for (int guard = 0; guard < npair + na; ++guard) {
                int item = 0;
                if (lane == 0) item = atomicAdd(&l_tk[0], 1);
                item = __builtin_amdgcn_readfirstlane(item);
                if (item < 0 || item >= npair + na) break;
                if (item < na) contacts_vehicle(w, s, c, e, kth_bit(adrv_lo, adrv_hi, item), lane, l_cfl);
                else localize_pair(w, lanes, roads, s, e, kth_bit(drv_lo, drv_hi, 2 * (item - na)), kth_bit(drv_lo, drv_hi, 2 * (item - na) + 1), lane, l_onlane);
            }
        } else if (nd + na <= kWaves) {
            // everything fits one round: one wave per job, the vehicle's data in scalar registers
            for (int item = wave; item < nd + na; item += kWaves) {
                if (item < nd) {
                    if (!(MD_ENV_SKIP & 4)) localize_vehicle<kLocRoadFirst>(w, lanes, roads, s, e, kth_bit(drv_lo, drv_hi, item), lane, l_onlane);
                } else if (!(MD_ENV_SKIP & 8)) contacts_vehicle(w, s, c, e, kth_bit(adrv_lo, adrv_hi, item - nd), lane, l_cfl);
            }
        } else {
            // many vehicles awake: two localisations per wave (32 lanes each), halving the rounds
            const int npair = (nd + 1) >> 1;
            for (int item = wave; item < npair + na; item += kWaves) {
                if (item < npair) {
                    if (!(MD_ENV_SKIP & 4)) localize_pair<kLocRoadFirst>(w, lanes, roads, s, e, kth_bit(drv_lo, drv_hi, 2 * item), kth_bit(drv_lo, drv_hi, 2 * item + 1), lane, l_onlane);
                } else if (!(MD_ENV_SKIP & 8))
                    contacts_vehicle(w, s, c, e, kth_bit(adrv_lo, adrv_hi, item - npair), lane, l_cfl);
            }
        }
        __syncthreads();
    } else {
        if (PH & PH_LOCALIZE) {
            for (int j = wave; j < cap; j += kWaves) localize_vehicle<kLocRoadFirst>(w, lanes, roads, s, e, j, lane);
            __syncthreads();
        }
        MD_STAMP_AT(5);
        if (PH & PH_CONTACTS) {
            for (int j = wave; j < cap; j += kWaves) contacts_vehicle(w, s, c, e, j, lane);
            __syncthreads();
        }
    }
    MD_STAMP_AT(6);
    if (PH & PH_TRAFFIC) {
        for (int j = tid; j < cap; j += kBlock) {
            // Fused step: "drives" comes from the masks built BEFORE the localisation, never from a re-read of the slot's
            // flags: the last wave may already be inside trigger_env below, clearing MD_F_PENDING of slots that did
            // not drive in this step (their l_onlane / l_cfl entries were never written).  Those slots are skipped
            // here by construction, and the read-modify-write of a driving slot's flags cannot collide with the
            // trigger's, which only touches PENDING slots.
            const bool drove = kFused ? ((((j < 64) ? (drv_lo >> j) : (drv_hi >> (j - 64))) & 1ull) != 0ull) : false;
            if (kFused && !drove) continue;
            const int f = s.shape[j].flags;
            if (kFused)  // traffic slots carry no contact flags (l_cfl is written for agents only)
                s.flags[j] = l_onlane[j] | ((f & MD_F_AGENT) ? l_cfl[j] : 0u);
            if (md_drives(f) && !(f & MD_F_AGENT) && !(s.flags[j] & MD_FL_ON_LANE)) {
                s.shape[j].flags = f & ~MD_F_ALIVE;
                if (kFused) l_cfl[j] = kRemovedMark;  // the slot's last write-back (see the dirty-slot write-back)
            }
        }
        // next step's trigger: reads the agents' final lanes and the PENDING slots, which the removal above
        // (slots that drove in this step only) does not touch
        if (plan_ahead && wave == kWaves - 1) {
            if (kTriggerEarly) {   // searched beside the integration
                const int* l_trig = reinterpret_cast<const int*>(smem + L.scratch) + kTrigWord;
                trigger_fire_wave(lanes, s, c, lane, __builtin_amdgcn_readfirstlane(l_trig[0]), __builtin_amdgcn_readfirstlane(l_trig[1]));
            } else trigger_env(lanes, s, c, lane);
        }
        __syncthreads();
        if (RESPAWN) {  // respawn / hybrid: the removed vehicle re-enters on a respawn lane (rare; serial)
            if (tid == 0) md_traffic_respawn_env(&w, lanes, &s, &c, w.env_map[e]);
            __syncthreads();
        }
    }
    MD_STAMP_AT(7);
    if (plan_ahead) {
        // wave 0: the agents' observe chain.  waves 1..: IDM of every driving traffic vehicle for the NEXT step
        // (reads poses / lanes / speeds, writes the traffic slots' action, IDM timer / target lane and PID state:
        // disjoint from what observe writes -- obs, reward, the agent's flags / steps / energy).
        if (wave == 0) {
            if (!(MD_ENV_SKIP & 16))
                for (int a = 0; a < c.agents_per_env; ++a) observe_agent_wave1<kObsLockstep>(lanes, roads, s, c, a, just_reset, lane, l_scratch);
        } else if (!(MD_ENV_SKIP & 2)) {
            // the driving traffic vehicles by RANK, not by slot: dealt by slot (j = A + wave - 1, + kWaves - 1, ...) two of an env's
            // two or three vehicles meet on one wave in every third env while another wave idles
            int rank = 0;
            for (int j0 = 0; j0 < cap; j0 += 64) {
                const int jl = j0 + lane;
                const int fl = (jl < cap) ? s.shape[jl].flags : 0;
                unsigned long long mk = __ballot(jl < cap && md_drives(fl) && !(fl & MD_F_AGENT));
                while (mk) {
                    const int j = j0 + __ffsll((long long)mk) - 1;
                    mk &= mk - 1;
                    if (rank % (kWaves - 1) == wave - 1) idm_vehicle_wave<kIdmKeys>(w, lanes, roads, s, c, w.env_map[e], j, lane, reinterpret_cast<int*>(l_scratch));
                    ++rank;
                }
            }
        }
        MD_STAMP_AT(8);
    } else if (PH & PH_OBSERVE) {
        if (MULTI) {
            const int n_grp = (c.agents_per_env + kObsGroups - 1) / kObsGroups;
            for (int guard = 0; guard < n_grp; ++guard) {
                int gi = 0;
                if (lane == 0) gi = atomicAdd(&l_tk[1], 1);
                gi = __builtin_amdgcn_readfirstlane(gi);
                if (gi < 0 || gi >= n_grp) break;
                observe_agent_wave(lanes, roads, s, c, gi * kObsGroups, just_reset, lane, l_scratch);
            }
        } else {
            for (int a = wave; a < c.agents_per_env; a += kWaves) observe_agent_wave1(lanes, roads, s, c, a, just_reset, lane, l_scratch);
        }
        MD_STAMP_AT(8);
        // lidar only reads shapes; observe writes obs[0:19] / flags / nav / pid -- no barrier needed in between
    }
    if ((PH & PH_LIDAR) && !(PH == PH_ALL && (MD_ENV_SKIP & 1))) {
        if (c.n_beams > 0) phase_lidar(w, s, c, e, tid, kWaves, lidar_out, lidar_stride, lidar_offset, track_det ? l_det : nullptr, PH == PH_ALL ? &l_tk[2] : nullptr);
    }

    MD_STAMP_AT(9);
    // ---- write the modified arrays back (coalesced 16-byte stores) ----
    if (!kLidarOnly) {
        __syncthreads();
        MD_STAMP_AT(10);
        constexpr bool respawns = (PH & PH_TRAFFIC) && RESPAWN;  // traffic respawn rewrites a whole slot
        if (kFused && !MULTI && !do_reset) {
            // Single-agent fused step: only slots that drive now (agents, traffic incl. the just triggered /
            // respawned) or were removed this step can differ from what HBM already holds -- props, waiting and
            // dead traffic are never written by any phase.  Writing just those cuts the store traffic ~4x.
            const bool replay = c.traffic_mode == 3;  // replayed slots move without "driving"
            auto dirty = [&](int j) { return replay || md_moves(l_shape[j].flags) || l_cfl[j] == kRemovedMark; };
            for (int i = tid; i < cap * 2; i += kBlock)
                if (dirty(i >> 1)) {
                    st_stream(&reinterpret_cast<uint4*>(gv.shape)[i], reinterpret_cast<const uint4*>(l_shape)[i]);
                    st_stream(&reinterpret_cast<uint4*>(gv.dyn)[i], reinterpret_cast<const uint4*>(l_dyn)[i]);
                    st_stream(&reinterpret_cast<uint4*>(gv.pid)[i], reinterpret_cast<const uint4*>(l_pid)[i]);
                }
            for (int i = tid; i < cap * 4; i += kBlock)
                if (dirty(i >> 2)) st_stream(&reinterpret_cast<uint4*>(gv.nav)[i], reinterpret_cast<const uint4*>(l_nav)[i]);
            for (int j = tid; j < cap; j += kBlock)
                if (dirty(j)) {
                    reinterpret_cast<float2*>(gv.action)[j] = reinterpret_cast<const float2*>(l_action)[j];
                    gv.flags[j] = l_flags[j];
                    if (RESPAWN) gv.final_lane[j] = l_final[j];
                }
            if (track_det)
                for (int j = tid; j < 2 * c.agents_per_env; j += kBlock) gv.detected[j] = l_det[j];
            MD_STAMP_AT(11);
            return;
        }
        if (PH & (PH_RESET | PH_IDM | PH_INTEGRATE | PH_TRAFFIC | PH_OBSERVE | PH_LIFECYCLE)) copy16(gv.shape, l_shape, cap * (int)sizeof(MdShape), tid, kBlock);
        if (MULTI && (PH & (PH_RESET | PH_LIFECYCLE)) && c.random_agent_model && c.is_multi_agent)
            copy16(gv.param, l_param, cap * (int)sizeof(MdParam), tid, kBlock);   // a respawn / reset rewrote vehicle classes
        if ((PH & (PH_RESET | PH_INTEGRATE | PH_LIFECYCLE)) || respawns) copy16(gv.dyn, l_dyn, cap * (int)sizeof(MdDyn), tid, kBlock);
        if ((PH & (PH_RESET | PH_IDM | PH_LOCALIZE | PH_OBSERVE | PH_LIFECYCLE)) || respawns) copy16(gv.nav, l_nav, cap * (int)sizeof(MdNav), tid, kBlock);
        if ((PH & (PH_RESET | PH_IDM | PH_OBSERVE | PH_LIFECYCLE)) || respawns || (lane_change && (PH & PH_INTEGRATE)))
            copy16(gv.pid, l_pid, cap * (int)sizeof(MdPid), tid, kBlock);
        if (((PH & (PH_RESET | PH_LIFECYCLE)) && MULTI) || ((PH & (PH_RESET | PH_TRAFFIC)) && RESPAWN)) {
            for (int j = tid; j < cap; j += kBlock) gv.final_lane[j] = l_final[j];
        }
        for (int j = tid; j < cap; j += kBlock) {
            if ((PH & (PH_RESET | PH_IDM | PH_INTEGRATE | PH_LIFECYCLE)) || respawns) {
                gv.action[2 * j] = l_action[2 * j];
                gv.action[2 * j + 1] = l_action[2 * j + 1];
            }
            if ((PH & (PH_RESET | PH_LOCALIZE | PH_CONTACTS | PH_OBSERVE | PH_LIFECYCLE)) || respawns) gv.flags[j] = l_flags[j];
        }
        if (track_det)
            for (int j = tid; j < 2 * c.agents_per_env; j += kBlock) gv.detected[j] = l_det[j];
        if (do_reset && tid == 0) gv.need_reset[0] = 0;
    }
    MD_STAMP_AT(11);
}

// ------------------------------------------------------------------------------------------------
// wave_step_kernel: the fused step of the SINGLE-AGENT envs with ONE WAVE PER ENVIRONMENT.
//
// env_kernel above gives an env a 4-wave workgroup and orders its phases with workgroup barriers; with one agent and two
// or three driving vehicles per env most of those waves spend most of the step parked at the next barrier (PMC:
// SQ_WAIT_ANY 79 % of the wave-cycles) while holding a wave slot and a share of the LDS, and everything wave-uniform
// (stage-in addressing, masks, flag merges) is executed four times.  Here one wave64 walks through ALL phases of its
// env: the work items that env_kernel deals to waves (localise a vehicle, the agent's contacts, one IDM scan, one
// 64-beam lidar sector) are taken one after the other by the same wave, with the SAME wave-level device functions --
// identical arithmetic, candidate order and tie-breaks, so the results stay bit-identical to the oracle.  What changes
// is the machine mapping:
//   * no workgroup barrier anywhere: phases are ordered by program order inside the wave (LDS operations of one wave
//     execute in order; a compiler fence + wave barrier keeps the compiler from reordering across the lanes' roles);
//   * every resident wave issues useful instructions: 4096 envs = 4096 waves = 4 per SIMD, all of them busy, instead
//     of 1 792 resident workgroups x 4 waves of which ~1.3 per SIMD issue;
//   * a workgroup is kWaveEnvs independent envs (they share nothing but the launch), the LDS image of an env is
//     ~5.4 KB at 24 slots (no routes, no map tables), so LDS never limits the residency.
// Multi-agent envs (40 agents per env) keep env_kernel: there the parallelism inside one env pays.
// ------------------------------------------------------------------------------------------------
#ifndef MD_WAVE_ENVS
#define MD_WAVE_ENVS 4
#endif
constexpr int kWaveEnvs = MD_WAVE_ENVS;   // envs (= waves) per workgroup

// LDS image of one env (= one wave) in wave_step_kernel; the images of a workgroup's envs follow each other every `bytes`
struct WaveEnvLds { uint32_t shape, dyn, pid, param, nav, action, flags, final_lane, onlane, cfl, scratch, det, bytes; };
__host__ __device__ inline WaveEnvLds wave_env_lds(int cap, int agents) {
    WaveEnvLds L;
    L.shape = 0;                                                     // the 16-B records are staged as uint4
    L.dyn = L.shape + (uint32_t)cap * sizeof(MdShape);
    L.pid = L.dyn + (uint32_t)cap * sizeof(MdDyn);
    L.param = L.pid + (uint32_t)cap * sizeof(MdPid);
    L.nav = L.param + (uint32_t)cap * sizeof(MdParam);
    L.action = L.nav + (uint32_t)cap * sizeof(MdNav);                  // [cap][2] floats
    L.flags = L.action + (uint32_t)cap * 2 * sizeof(float);
    L.final_lane = L.flags + (uint32_t)cap * sizeof(uint32_t);
    L.onlane = L.final_lane + (uint32_t)cap * sizeof(int32_t);         // localize / contacts results, merged into flags afterwards
    L.cfl = L.onlane + (uint32_t)cap * sizeof(uint32_t);
    L.scratch = L.cfl + (uint32_t)cap * sizeof(uint32_t);             // 48 floats: the wave's observe results
    L.det = L.scratch + 48 * sizeof(float);                         // [agents][2] detected sets: 8-B aligned (see below)
    L.bytes = align_up(L.det + (uint32_t)agents * 2 * sizeof(unsigned long long), 16);   // the next env's shapes: uint4
    return L;
}
static_assert((sizeof(MdShape) + sizeof(MdDyn) + sizeof(MdPid) + sizeof(MdParam) + sizeof(MdNav) + 6 * 4) % 8 == 0 && 48 * 4 % 8 == 0,
              "wave_env_lds: the detected sets need 8-B alignment");

template <bool RESPAWN>
__global__ __launch_bounds__(64 * kWaveEnvs) void wave_step_kernel(MdWorld w, MdState g, MdConfig c, float* lidar_out,
                                                                  int lidar_stride, int lidar_offset) {
    if constexpr (!RESPAWN) lean_pins_fold(g, c);   // the lean launch: variant<PH_ALL>() guarantees them
    const int lane = threadIdx.x & 63;
    const int e = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);   // blockDim.x / 64 envs per workgroup (<= kWaveEnvs)
    if (e >= c.n_envs) return;   // whole wave
    const int cap = c.cap;
    const int A = c.agents_per_env;

    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const WaveEnvLds L = wave_env_lds(cap, A);
    unsigned char* base = smem + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6) * L.bytes;   // wave-uniform: kept in SGPRs
    MdShape* l_shape = reinterpret_cast<MdShape*>(base + L.shape);
    MdDyn* l_dyn = reinterpret_cast<MdDyn*>(base + L.dyn);
    MdPid* l_pid = reinterpret_cast<MdPid*>(base + L.pid);
    MdParam* l_param = reinterpret_cast<MdParam*>(base + L.param);
    MdNav* l_nav = reinterpret_cast<MdNav*>(base + L.nav);
    float* l_action = reinterpret_cast<float*>(base + L.action);
    uint32_t* l_flags = reinterpret_cast<uint32_t*>(base + L.flags);
    int32_t* l_final = reinterpret_cast<int32_t*>(base + L.final_lane);
    uint32_t* l_onlane = reinterpret_cast<uint32_t*>(base + L.onlane);
    uint32_t* l_cfl = reinterpret_cast<uint32_t*>(base + L.cfl);
    float* l_scratch = reinterpret_cast<float*>(base + L.scratch);
    unsigned long long* l_det = reinterpret_cast<unsigned long long*>(base + L.det);
    const EnvImage img = {l_shape, l_dyn, l_pid, l_param, l_nav, l_action, l_flags, l_final};
    const bool track_det = RESPAWN && g.detected != nullptr;

    const MdState gv = md_env_view(&g, &c, e);
    const int reset_flag = gv.need_reset[0];
    MD_STAMP_AT(0);
    const int m = w.env_map[e];
    const MdLane* lanes = w.lanes + w.lane_off[m];
    const MdRoad* roads = w.roads + w.road_off[m];
    const bool fused_act = gv.agent_action != nullptr;

    // ---- stage-in: every global load is issued before the first LDS store (one memory round trip) ----
    {
        const int n32 = cap * 2, n64 = cap * 4;   // 16-byte units
        const uint4* g_shape = reinterpret_cast<const uint4*>(gv.shape);
        const uint4* g_dyn = reinterpret_cast<const uint4*>(gv.dyn);
        const uint4* g_pid = reinterpret_cast<const uint4*>(gv.pid);
        const uint4* g_param = reinterpret_cast<const uint4*>(gv.param);
        const uint4* g_nav = reinterpret_cast<const uint4*>(gv.nav);
        uint4 r_shape, r_dyn, r_pid, r_param, r_nav0, r_nav1;
        float2 r_act;
        uint32_t r_fl;
        int r_fin;
        const bool p32 = lane < n32, pc = lane < cap;
        if (p32) {
            r_shape = ld_stream(&g_shape[lane]);
            r_dyn = ld_stream(&g_dyn[lane]);
            r_pid = ld_stream(&g_pid[lane]);
            r_param = ld_stream(&g_param[lane]);
        }
        if (lane < n64) r_nav0 = ld_stream(&g_nav[lane]);
        if (lane + 64 < n64) r_nav1 = ld_stream(&g_nav[lane + 64]);
        if (pc) {
            r_act = (fused_act && lane < A) ? reinterpret_cast<const float2*>(gv.agent_action)[lane]
                                            : reinterpret_cast<const float2*>(gv.action)[lane];
            r_fl = gv.flags[lane];
            r_fin = gv.final_lane ? gv.final_lane[lane] : 0;
        }
        if (p32) {
            reinterpret_cast<uint4*>(l_shape)[lane] = r_shape;
            reinterpret_cast<uint4*>(l_dyn)[lane] = r_dyn;
            reinterpret_cast<uint4*>(l_pid)[lane] = r_pid;
            reinterpret_cast<uint4*>(l_param)[lane] = r_param;
        }
        if (lane < n64) reinterpret_cast<uint4*>(l_nav)[lane] = r_nav0;
        if (lane + 64 < n64) reinterpret_cast<uint4*>(l_nav)[lane + 64] = r_nav1;
        if (pc) {
            reinterpret_cast<float2*>(l_action)[lane] = r_act;
            l_flags[lane] = r_fl;
            l_final[lane] = r_fin;
        }
        // capacities beyond 32 slots (accident scenes with many props): the tails, in plain loops
        for (int i = lane + 64; i < n32; i += 64) {
            reinterpret_cast<uint4*>(l_shape)[i] = g_shape[i];
            reinterpret_cast<uint4*>(l_dyn)[i] = g_dyn[i];
            reinterpret_cast<uint4*>(l_pid)[i] = g_pid[i];
            reinterpret_cast<uint4*>(l_param)[i] = g_param[i];
        }
        for (int i = lane + 128; i < n64; i += 64) reinterpret_cast<uint4*>(l_nav)[i] = g_nav[i];
        for (int j = lane + 64; j < cap; j += 64) {
            const float* src = (fused_act && j < A) ? gv.agent_action : gv.action;
            l_action[2 * j] = src[2 * j];
            l_action[2 * j + 1] = src[2 * j + 1];
            l_flags[j] = gv.flags[j];
            l_final[j] = gv.final_lane ? gv.final_lane[j] : 0;
        }
        if (track_det)
            for (int j = lane; j < 2 * A; j += 64) l_det[j] = 0ull;
    }
    const bool do_reset = reset_flag != 0;   // wave-uniform
    const int just_reset = do_reset ? 1 : 0;
    if (do_reset) {
        wave_lds_sync();
        const uint4* s0 = reinterpret_cast<const uint4*>(gv.shape0);
        const uint4* d0 = reinterpret_cast<const uint4*>(gv.dyn0);
        const uint4* p0 = reinterpret_cast<const uint4*>(gv.pid0);
        const uint4* n0 = reinterpret_cast<const uint4*>(gv.nav0);
        for (int i = lane; i < cap * 2; i += 64) {
            reinterpret_cast<uint4*>(l_shape)[i] = s0[i];
            reinterpret_cast<uint4*>(l_dyn)[i] = d0[i];
            reinterpret_cast<uint4*>(l_pid)[i] = p0[i];
        }
        for (int i = lane; i < cap * 4; i += 64) reinterpret_cast<uint4*>(l_nav)[i] = n0[i];
        for (int j = lane; j < cap; j += 64) {
            l_action[2 * j] = 0.0f;
            l_action[2 * j + 1] = 0.0f;
            l_flags[j] = 0u;
        }
        if (RESPAWN && (c.traffic_mode == 1 || c.traffic_mode == 2)) {   // respawns rewrote the routes: restore them too
            for (int i = lane; i < cap * MD_ROUTE_LEN; i += 64) {
                gv.route_nodes[i] = gv.route_nodes0[i];
                gv.route_roads[i] = gv.route_roads0[i];
            }
            for (int j = lane; j < cap; j += 64) l_final[j] = gv.final_lane0[j];
        }
    }
    MdState s = local_view(gv, img);   // env-local view whose hot arrays live in this wave's LDS image
    wave_lds_sync();
    MD_STAMP_AT(1);

    // agent_policy = IDMPolicy: the agents are planned like the traffic, in the reference's order (decide, then move);
    // otherwise the traffic is planned one step AHEAD, at the end of the step (see env_kernel)
    const bool agent_idm = RESPAWN && c.agent_idm == MD_AGENT_IDM;
    const bool plan_ahead = !agent_idm;
    const bool lane_change = RESPAWN && c.agent_idm == MD_AGENT_LANE_CHANGE;   // LaneChangePolicy: see env_kernel
    if (!just_reset && !plan_ahead) {
        trigger_env(lanes, s, c, lane);
        wave_lds_sync();
        for (int j0 = 0; j0 < cap; j0 += 64) {
            const int jj = j0 + lane;
            const unsigned long long mk = __ballot(jj < cap && md_drives(s.shape[jj < cap ? jj : 0].flags));
            if (mk) idm_group_wave(w, lanes, roads, s, c, m, j0, mk, lane, reinterpret_cast<int*>(l_scratch));
        }
        wave_lds_sync();
    }
    MD_STAMP_AT(3);
    // the slots that drive in this step (the integration does not change any slot's flags)
    const SlotMask drv = drive_mask(s.shape, cap, lane);
    const unsigned long long drv_lo = drv.lo, drv_hi = drv.hi;
    if (!just_reset) {
        for (int j = lane; j < cap; j += 64) {
            if (lane_change && j < A) {
                const int f = s.shape[j].flags;
                if (md_drives(f) && !(f & MD_F_SPAWNED)) md_lane_change_act(lanes, roads, &s, j);
            }
            if (RESPAWN) md_advance_mover(&s, &c, j);
            else md_integrate_mover(&s, &c, j);
        }
        if (!RESPAWN)
            for (int j = lane; j < cap; j += 64) md_walk_mover(&s, &c, j);
        wave_lds_sync();
    }
    MD_STAMP_AT(4);
    // ---- localisation of every driving vehicle, contacts of every driving agent ----
    {
        const SlotMask adrv = agent_share(drv, A);
        const unsigned long long adrv_lo = adrv.lo, adrv_hi = adrv.hi;
        const int nd = popc(drv), na = popc(adrv);
        // one vehicle: the whole wave, its data in scalar registers; two: 32 lanes each; more: 16 lanes each, four per pass
        if (nd == 1) localize_vehicle(w, lanes, roads, s, e, kth_bit(drv_lo, drv_hi, 0), lane, l_onlane);
        else if (nd == 2) localize_pair(w, lanes, roads, s, e, kth_bit(drv_lo, drv_hi, 0), kth_bit(drv_lo, drv_hi, 1), lane, l_onlane);
        else
            for (int item = 0; item < nd; item += 4)
                localize_group<16>(w, lanes, roads, s, e, kth_bit(drv_lo, drv_hi, item), kth_bit(drv_lo, drv_hi, item + 1),
                                   kth_bit(drv_lo, drv_hi, item + 2), kth_bit(drv_lo, drv_hi, item + 3), lane, l_onlane);
        for (int k = 0; k < na; ++k) contacts_vehicle(w, s, c, e, kth_bit(adrv_lo, adrv_hi, k), lane, l_cfl);
    }
    wave_lds_sync();
    MD_STAMP_AT(6);
    // ---- flags of the slots that drove; traffic that left every lane is removed ----
    for (int j = lane; j < cap; j += 64) {
        const bool drove = (((j < 64) ? (drv_lo >> j) : (drv_hi >> (j - 64))) & 1ull) != 0ull;
        if (!drove) continue;
        const int f = s.shape[j].flags;
        s.flags[j] = l_onlane[j] | ((f & MD_F_AGENT) ? l_cfl[j] : 0u);
        if (!(f & MD_F_AGENT) && !(s.flags[j] & MD_FL_ON_LANE)) {
            s.shape[j].flags = f & ~MD_F_ALIVE;
            l_cfl[j] = kRemovedMark;
        }
    }
    wave_lds_sync();
    if (plan_ahead) {   // next step's trigger: the agents' final lanes, the PENDING slots
        trigger_env(lanes, s, c, lane);
        wave_lds_sync();
    }
    if (RESPAWN) {   // respawn / hybrid: the removed vehicle re-enters on a respawn lane (rare; serial)
        if (lane == 0) md_traffic_respawn_env(&w, lanes, &s, &c, m);
        wave_lds_sync();
    }
    MD_STAMP_AT(7);
    // ---- next step's traffic decisions, then the agents' observations (disjoint data: either order gives the same) ----
    if (plan_ahead) {
        for (int j0 = 0; j0 < cap; j0 += 64) {
            const int jj = j0 + lane;
            const unsigned long long mk = __ballot(jj < cap && jj >= A && md_drives(s.shape[jj < cap ? jj : 0].flags) &&
                                                   !(s.shape[jj < cap ? jj : 0].flags & MD_F_AGENT));
            if (mk) idm_group_wave(w, lanes, roads, s, c, m, j0, mk, lane, reinterpret_cast<int*>(l_scratch));
            wave_lds_sync();
        }
    }
    MD_STAMP_AT(8);
    for (int a = 0; a < A; ++a) observe_agent_wave1(lanes, roads, s, c, a, just_reset, lane, l_scratch);
    MD_STAMP_AT(9);
    // ---- lidar: the sectors of every agent, one after the other ----
    if (c.n_beams > 0) {
        const int nsec = (c.n_beams + 63) >> 6;
        for (int a = 0; a < A; ++a) {
            float* row = lidar_out + (size_t)(e * A + a) * lidar_stride + lidar_offset;
            for (int sec = 0; sec < nsec; ++sec) lidar_item(w, s, c, a, sec, lane, row, track_det ? l_det + 2 * a : nullptr);
        }
    }
    wave_lds_sync();
    MD_STAMP_AT(10);
    // ---- write-back (16-byte stores) ----
    if (!do_reset) {
        // only slots that move now (agents, traffic incl. the just triggered / respawned, walking participants) or were
        // removed in this step can differ from what HBM already holds
        const bool replay = RESPAWN && c.traffic_mode == 3;   // replayed slots move without "driving"
        auto dirty = [&](int j) { return replay || md_moves(l_shape[j].flags) || l_cfl[j] == kRemovedMark; };
        for (int i = lane; i < cap * 2; i += 64)
            if (dirty(i >> 1)) {
                st_stream(&reinterpret_cast<uint4*>(gv.shape)[i], reinterpret_cast<const uint4*>(l_shape)[i]);
                st_stream(&reinterpret_cast<uint4*>(gv.dyn)[i], reinterpret_cast<const uint4*>(l_dyn)[i]);
                st_stream(&reinterpret_cast<uint4*>(gv.pid)[i], reinterpret_cast<const uint4*>(l_pid)[i]);
            }
        for (int i = lane; i < cap * 4; i += 64)
            if (dirty(i >> 2)) st_stream(&reinterpret_cast<uint4*>(gv.nav)[i], reinterpret_cast<const uint4*>(l_nav)[i]);
        for (int j = lane; j < cap; j += 64)
            if (dirty(j)) {
                reinterpret_cast<float2*>(gv.action)[j] = reinterpret_cast<const float2*>(l_action)[j];
                gv.flags[j] = l_flags[j];
                if (RESPAWN) gv.final_lane[j] = l_final[j];
            }
    } else {
        for (int i = lane; i < cap * 2; i += 64) {
            reinterpret_cast<uint4*>(gv.shape)[i] = reinterpret_cast<const uint4*>(l_shape)[i];
            reinterpret_cast<uint4*>(gv.dyn)[i] = reinterpret_cast<const uint4*>(l_dyn)[i];
            reinterpret_cast<uint4*>(gv.pid)[i] = reinterpret_cast<const uint4*>(l_pid)[i];
        }
        for (int i = lane; i < cap * 4; i += 64) reinterpret_cast<uint4*>(gv.nav)[i] = reinterpret_cast<const uint4*>(l_nav)[i];
        for (int j = lane; j < cap; j += 64) {
            reinterpret_cast<float2*>(gv.action)[j] = reinterpret_cast<const float2*>(l_action)[j];
            gv.flags[j] = l_flags[j];
            if (RESPAWN && gv.final_lane) gv.final_lane[j] = l_final[j];
        }
        if (lane == 0) gv.need_reset[0] = 0;
    }
    if (track_det)
        for (int j = lane; j < 2 * A; j += 64) gv.detected[j] = l_det[j];
    MD_STAMP_AT(11);
}

// ------------------------------------------------------------------------------------------------
// Scenario mode (MdConfig.traffic_mode 4): one ScenarioEnv step per launch, one 4-wave workgroup per scene.
//   stage-in     the scene's mover state -> LDS
//   decide       one WAVE per reactive vehicle (TrajectoryIDMPolicy): projection on its own path with one LANE per
//                polyline segment + wavefront arg-min; arrival; every fifth step (staggered by policy_index) the
//                front search: one lane per candidate object (20 m, any chassis corner inside the path's outline),
//                arg-min of the gaps; PID steering + IDM acceleration on lane 0
//   integrate    one thread per mover (agent + reactive vehicles; replayed ones are kinematic)
//   after_step   wave 0: one lane per track slot -- replay pose of frame k / removal / spawn; the spawns that get a
//                reactive policy take consecutive policy indices through a ballot prefix count (slot order, as the
//                reference's dict order)
//   agent        wave 0 projects the agent on the reference trajectory (lanes = segments) while wave 1 runs its contacts
//   observe      lane 0 of wave 0: state + 22 navigation dims + ScenarioEnv reward / cost / done; lidar sectors on all waves
// The scalar logic is include/md_scenario.h, shared with the oracle (which runs the serial forms).
// ------------------------------------------------------------------------------------------------
// InterpolatingLine.local_coordinates by one wave: lanes = segments (chunks of 64), first minimum wins like np.argmin.
// Every lane first keeps the best of ITS segments (lane, lane + 64, ...: a strict < keeps the earliest), then ONE dense
// wave reduction: the minimum distance by a 6-step butterfly, and among the lanes that hold it the lowest segment index
// (a sparse set, usually one lane: ballot walk).
// EXACT cull of a projection's pieces through MdWorld.poly_ball (a circle per group of MD_POLY_GROUP pieces, lanes = groups, at most
// 64 of them): a piece of the group with the smallest "farthest point of the circle" U is at most U away, so the arg-min lies in a
// group whose circle comes within U; every other group's pieces are farther than the minimum by more than the margin (the radii are
// rounded up by >= 1e-3 m, the test adds 0.02 m + 1e-5 U against the rounding of the distances computed here), so neither the arg-min
// nor a tie can sit in them.  Returns the mask of the groups to evaluate (never empty for n >= 1).
constexpr int kPolyGroup = MD_POLY_GROUP;
static_assert(kPolyGroup == 8, "the lane <-> (group, piece) mapping below packs eight groups of eight pieces into a wave");
__device__ __forceinline__ unsigned long long poly_cull_wave(const float4* balls, int n, float px, float py, int lane_id) {
    const int n_g = (n + kPolyGroup - 1) / kPolyGroup;
    float lb = 3.0e38f, ub = 3.0e38f;
    if (lane_id < n_g) {
        const float4 b = balls[lane_id];
        const float d = md_norm(px - b.x, py - b.y);
        lb = d - b.z;
        ub = d + b.z;
    }
    float U = ub;
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) U = md_min(U, __shfl_xor(U, off, 64));
    return __ballot(lane_id < n_g && lb <= U + (0.02f + 1.0e-5f * U));
}
// lane -> the piece it evaluates: piece (lane & 7) of the (lane >> 3)-th lowest group of `cand` (-1: none).  Lanes in ascending order
// hold pieces in ascending order.
__device__ __forceinline__ int cull_piece_of(unsigned long long cand, int n, int lane_id) {
    int grp = -1;
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        const int g = cand ? (__ffsll((long long)cand) - 1) : -1;   // wave-uniform
        cand &= cand - 1;
        if ((lane_id >> 3) == q) grp = g;
    }
    const int i = grp * kPolyGroup + (lane_id & 7);
    return (grp >= 0 && i < n) ? i : -1;
}
__device__ __forceinline__ bool poly_can_cull(const float4* balls, int n) { return balls != nullptr && n > 2 * kPolyGroup && n <= 64 * kPolyGroup; }

__device__ __forceinline__ int poly_local_wave(const MdPoly& p, const float4* balls, float px, float py, int lane_id, float* lng, float* lat) {
    // The coordinates come WITHOUT a second trip to memory (arg-min, then md_poly_local_at of that piece): every lane keeps the
    // coordinates w.r.t. the best of its own pieces (the expressions of md_poly_local_at), the winner's are read from its lane.
    float bd = 3.0e38f, bl = 0.0f, bt = 0.0f;
    int bi = 0x7fffffff;
    auto eval = [&](int i) {
        const MdSeg g = p.segs[i];
        const float d = md_seg_dist(&g, px, py);
        if (d < bd) {   // a lane meets its pieces in ascending order: the strict < keeps the earliest of its minima
            const float ddx = px - g.sx, ddy = py - g.sy;
            bd = d;
            bi = i;
            bl = g.cum + (ddx * g.dx + ddy * g.dy);
            bt = ddx * g.dy - ddy * g.dx;
        }
    };
    if (poly_can_cull(balls, p.n)) {
        unsigned long long cand = poly_cull_wave(balls, p.n, px, py, lane_id);
        while (cand) {   // eight groups per pass, ascending
            const int i = cull_piece_of(cand, p.n, lane_id);
#pragma unroll
            for (int q = 0; q < 8; ++q) cand &= cand - 1;
            if (i >= 0) eval(i);
        }
    } else {
        for (int i = lane_id; i < p.n; i += 64) eval(i);
    }
    float m = bd;
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) m = md_min(m, __shfl_xor(m, off, 64));
    const int best = wave_min_i(bi, bd == m, 0x7fffffff);
    const int src = __ffsll((long long)__ballot(bd == m && bi == best)) - 1;   // the one lane that holds it
    *lng = bcast_f(bl, src);
    *lat = bcast_f(bt, src);
    return best;
}

// What a decision needs to know about a slot's route before it touches a piece: staged into LDS with the scene's state (one memory
// round trip for the whole scene) instead of three dependent ones per vehicle (route_n -> poly_off -> aux).  md_route_of + aux.
struct __attribute__((aligned(16))) RouteDesc {
    const MdSeg* segs;
    const float* verts;
    const float4* balls;  // MdWorld.poly_ball of the slot's static polyline; nullptr: none (cut routes, tables not supplied)
    int pad_[2];
    int n;
    int n_verts;          // bit 30: no aux record (end point / outline box are derived by the decision)
    float end_x, end_y;
    float bx0, by0, bx1, by1;
};
constexpr int kDescNoAux = 1 << 30;
__device__ __forceinline__ int uni_i(int v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ __forceinline__ float uni_f(float v) { return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(v))); }
template <typename T>
__device__ __forceinline__ const T* uni_p(const T* q) {
    const unsigned long long u = reinterpret_cast<unsigned long long>(q);
    const unsigned lo = (unsigned)__builtin_amdgcn_readfirstlane((int)(u & 0xffffffffull));
    const unsigned hi = (unsigned)__builtin_amdgcn_readfirstlane((int)(u >> 32));
    return reinterpret_cast<const T*>(((unsigned long long)hi << 32) | lo);
}

// crossing number of the ray from (px, py) over the polygon's edges, lanes = edges: odd = inside (md_point_in_polygon)
__device__ __forceinline__ bool point_in_polygon_wave(const float* xy, int n, float px, float py, int lane_id) {
    int cnt = 0;
    for (int i0 = 0; i0 < n; i0 += 64) {
        const int i = i0 + lane_id;
        cnt += __popcll(__ballot(i < n && md_polygon_edge_crosses(xy, n, i, px, py)));
    }
    return (cnt & 1) != 0;
}

// first segment (ascending) for which `pred` holds, else the last one; pred evaluated by one lane per segment
template <typename F>
__device__ __forceinline__ int poly_first_wave(const MdPoly& p, int lane_id, F pred) {
    for (int i0 = 0; i0 < p.n; i0 += 64) {
        const int i = i0 + lane_id;
        const unsigned long long m = __ballot(i < p.n && pred(p.segs[i]));
        if (m) return i0 + __ffsll((long long)m) - 1;
    }
    return p.n - 1;
}

// The agent on its reference trajectory (md_traj_locate) and the trajectory's length (md_poly_of's) in TWO trips to memory for up to
// 256 pieces: every lane keeps the end longitudinals of its (<= 4) pieces, so the two "first piece that ends beyond" look-ups are
// ballots over registers; then the two pieces they name are read together.
__device__ __forceinline__ void traj_locate_wave(const MdPoly& p, float px, float py, int lane_id, MdTrajLoc* o, float* length) {
    constexpr int kChunks = 4;
    if (p.n > 0 && p.n <= 64 * kChunks) {   // wave-uniform
        float ce[kChunks];
        float bd = 3.0e38f, bl = 0.0f, bt = 0.0f;
        int bi = 0x7fffffff;
#pragma unroll
        for (int q = 0; q < kChunks; ++q) {
            const int i = lane_id + 64 * q;
            ce[q] = -3.0e38f;     // never "ends beyond" anything
            if (i < p.n) {
                const MdSeg g = p.segs[i];
                const float d = md_seg_dist(&g, px, py);
                if (d < bd) {
                    const float ddx = px - g.sx, ddy = py - g.sy;
                    bd = d;
                    bi = i;
                    bl = g.cum + (ddx * g.dx + ddy * g.dy);
                    bt = ddx * g.dy - ddy * g.dx;
                }
                ce[q] = g.cum + g.len;
            }
        }
        float m = bd;
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) m = md_min(m, __shfl_xor(m, off, 64));
        const int best = wave_min_i(bi, bd == m, 0x7fffffff);
        const float lng = bcast_f(bl, best & 63);
        o->lng = lng;
        o->lat = bcast_f(bt, best & 63);
        const int il = p.n - 1;
        int ih = il, is = il;
        bool fh = false, fs = false;
        float len = 0.0f;
#pragma unroll
        for (int q = 0; q < kChunks; ++q) {
            const unsigned long long mh = __ballot(ce[q] > lng), ms = __ballot(ce[q] + 0.1f >= lng);
            if (!fh && mh) {
                ih = 64 * q + __ffsll((long long)mh) - 1;
                fh = true;
            }
            if (!fs && ms) {
                is = 64 * q + __ffsll((long long)ms) - 1;
                fs = true;
            }
            if ((il >> 6) == q) len = bcast_f(ce[q], il & 63);
        }
        *length = len;
        const float hh = p.segs[ih].heading;
        const MdSeg gs = p.segs[is];
        o->heading_at = hh;
        o->lat_dx = gs.dy;
        o->lat_dy = -gs.dx;
        return;
    }
    *length = (p.n > 0) ? p.segs[p.n - 1].cum + p.segs[p.n - 1].len : 0.0f;
    poly_local_wave(p, nullptr, px, py, lane_id, &o->lng, &o->lat);
    const float lng = o->lng;
    const int ih = poly_first_wave(p, lane_id, [lng](const MdSeg& g) { return g.cum + g.len > lng; });
    const int is = poly_first_wave(p, lane_id, [lng](const MdSeg& g) { return g.cum + g.len + 0.1f >= lng; });
    o->heading_at = p.segs[ih].heading;
    o->lat_dx = p.segs[is].dy;
    o->lat_dy = -p.segs[is].dx;
}

// Four points against one polygon in one pass over its edges (lanes = edges): bit c of the result = point c is inside
// (odd crossing number, md_point_in_polygon).  `want`: the points worth testing (wave-uniform).
__device__ __forceinline__ int points_in_polygon_wave4(const float* xy, int n, const float* px, const float* py, int want, int lane_id) {
    int c0 = 0, c1 = 0, c2 = 0, c3 = 0;
    for (int i0 = 0; i0 < n; i0 += 64) {
        const int i = i0 + lane_id;
        const bool v = i < n;
        const int ii = v ? i : 0;
        const int j = (ii == 0) ? n - 1 : ii - 1;
        const float xi = xy[2 * ii], yi = xy[2 * ii + 1], xj = xy[2 * j], yj = xy[2 * j + 1];
        // md_polygon_edge_crosses, the same expression for each point
        // the division only where an edge of this chunk straddles the point's y at all (two edges of the whole outline, usually)
#define MD_CROSS(q, cnt)                                                                                       \
        if (want & (1 << q)) {                                                                                 \
            const bool st = v && ((yi > py[q]) != (yj > py[q]));                                               \
            if (__ballot(st)) cnt += __popcll(__ballot(st && (px[q] < (xj - xi) * (py[q] - yi) / (yj - yi) + xi))); \
        }
        MD_CROSS(0, c0)
        MD_CROSS(1, c1)
        MD_CROSS(2, c2)
        MD_CROSS(3, c3)
#undef MD_CROSS
    }
    return (c0 & 1) | ((c1 & 1) << 1) | ((c2 & 1) << 2) | ((c3 & 1) << 3);
}

// TrajectoryIDMPolicy.act of the vehicle in `slot` by one wave (md_tidm_vehicle is the serial form).
// The route's pieces are read ONCE: every lane keeps the end longitudinal and the heading of its (<= 4) pieces in
// registers, so the look-ahead heading after the projection needs no second pass over memory; the end point and the
// outline's bounding box come precomputed (MdWorld.poly_aux); the four chassis corners of a candidate are tested in
// one pass over the outline's edges, and only those inside its bounding box.
// Scratch of the decision stage in LDS (over the route builder's scratch, which the traffic manager uses later in the step).
struct DecideLds {
    unsigned long long* key;   // [cap] (gap bits << 32 | slot) of the front object found so far; kNoFront = none
    float* cur_long;           // [cap] own longitudinal; NaN = arrived (no decision)
    float* heading;            // [cap] heading of the route one metre ahead
    uint32_t* pairs;           // [kPairCap] (vehicle | candidate << 8 | corners-in-box << 16); kNullPair = nothing
    int* ctl;                  // [0] pairs reserved, [1] pair tickets
};
constexpr int kPairCap = 256;
constexpr uint32_t kNullPair = 0xffffffffu;
constexpr unsigned long long kNoFront = ~0ull;

// One (speed-control vehicle, near mover) pair of get_find_front_back_objs_single_lane (md_tidm_front_gap), by one wave: the chassis
// corners inside the outline's bounding box against the outline (lanes = polygon edges, all corners in one pass), then the
// projection on the route with lanes = pieces.  A mover that counts enters the vehicle's key by an LDS atomic min: the smallest gap,
// among equal gaps the lowest slot -- what the serial search's ascending order and strict < leave.
__device__ __forceinline__ void tidm_pair_wave(const MdState& s, int slot, int j, int want, int lane_id, const RouteDesc* l_desc,
                                               const DecideLds& dl) {
    const RouteDesc rd = l_desc[slot];
    MdPoly route;
    route.segs = uni_p(rd.segs);
    route.n = uni_i(rd.n);
    route.length = 0.0f;
    const float* pv = uni_p(rd.verts);
    const int n_v = uni_i(rd.n_verts) & ~kDescNoAux;
    const float4* balls = uni_p(rd.balls);
    const MdShape o = s.shape[j];   // wave-uniform
    const float ex = o.c * o.hl, ey = o.s * o.hl, fx = -o.s * o.hw, fy = o.c * o.hw;
    const float qx[4] = {o.cx + ex + fx, o.cx + ex - fx, o.cx - ex - fx, o.cx - ex + fx};
    const float qy[4] = {o.cy + ey + fy, o.cy + ey - fy, o.cy - ey - fy, o.cy - ey + fy};
    if (points_in_polygon_wave4(pv, n_v, qx, qy, want, lane_id) == 0) return;
    float lg, lt;
    poly_local_wave(route, balls, o.cx, o.cy, lane_id, &lg, &lt);
    const float gap = lg - dl.cur_long[slot];
    if (lane_id == 0 && gap > 0.0f && gap < MD_TIDM_MAX_DIST)
        atomicMin(&dl.key[slot], ((unsigned long long)__float_as_uint(gap) << 32) | (unsigned)j);
}

// TrajectoryIDMPolicy.act of the vehicle in `slot`, everything BEFORE the front search's candidates are looked at, by one wave
// (md_tidm_vehicle is the serial form): arrival, own projection, the heading ahead; a vehicle due for speed control leaves its
// (vehicle, near mover) pairs on the scene's pair list, which ALL waves then work off (tidm_pair_wave) -- a crowded vehicle's
// search was the tail of the stage when one wave walked its movers alone.
__device__ __forceinline__ void tidm_prepare_wave(const MdWorld& w, const MdState& s, const MdConfig& c, int e, int slot, int k,
                                  int lane_id, const RouteDesc* l_desc, const DecideLds& dl) {
#ifdef MD_STAMP
    bool st_ = lane_id == 0;   // diagnostic: the scene's first reactive vehicle, apart for its speed-control steps (slots 16.. / 24..)
    for (int q = c.agents_per_env; q < slot; ++q) st_ = st_ && !(s.nav[q].ck0 == MD_SC_IDM && md_present(s.shape[q].flags));
    const int so_ = ((k % MD_TIDM_BATCH) == s.nav[slot].timer) ? 8 : 0;
#endif
    MD_FINE_STAMP(st_, so_ + 0);
    // the slot's static polyline or the route cut at its spawn frame (md_route_of), end point and outline box (aux): the record the
    // stage-in left in LDS -- wave-uniform, kept in scalar registers
    const RouteDesc rd = l_desc[slot];
    MdPoly route;
    route.segs = uni_p(rd.segs);
    route.n = uni_i(rd.n);
    route.length = 0.0f;   // only the fallback below needs it: a dependent load of the last piece
    const int nvf = uni_i(rd.n_verts);
    const float4* balls = uni_p(rd.balls);
    const float px = s.shape[slot].cx, py = s.shape[slot].cy;
    float end_x, end_y, bx0 = -3.0e38f, by0 = -3.0e38f, bx1 = 3.0e38f, by1 = 3.0e38f;
    if (!(nvf & kDescNoAux)) {
        end_x = uni_f(rd.end_x);
        end_y = uni_f(rd.end_y);
        bx0 = uni_f(rd.bx0);
        by0 = uni_f(rd.by0);
        bx1 = uni_f(rd.bx1);
        by1 = uni_f(rd.by1);
    } else {
        route.length = (route.n > 0) ? route.segs[route.n - 1].cum + route.segs[route.n - 1].len : 0.0f;
        const float length = route.length;
        const int ie = poly_first_wave(route, lane_id, [length](const MdSeg& g) { return g.cum + g.len + 0.1f >= length; });
        const MdSeg ge = route.segs[ie];
        end_x = ge.sx + (length - ge.cum) * ge.dx;
        end_y = ge.sy + (length - ge.cum) * ge.dy;
    }
    if (md_norm(px - end_x, py - end_y) < MD_TIDM_DEST_RADIUS) {
        if (lane_id == 0) {
            s.nav[slot].ck0 = MD_SC_ARRIVED;   // no action this step: the vehicle rolls on with its previous one
            dl.cur_long[slot] = __int_as_float(0x7fc00000);
        }
        return;
    }
    MD_FINE_STAMP(st_, so_ + 1);
    const int do_speed_control = (k % MD_TIDM_BATCH) == s.nav[slot].timer;
    // ---- projection on the own route; the pieces' end longitudinals / headings stay in registers ----
    constexpr int kChunks = 4;
    // (1) with the route's group circles (poly_cull_wave) and at most eight groups left: ONE pass, a lane per surviving piece -- the
    // usual case, ~20 of 100 pieces; (2) up to 256 pieces: all of them, (<= 4) per lane; (3) anything else: the generic loops
    unsigned long long cand = 0ull;
    if (poly_can_cull(balls, route.n)) cand = poly_cull_wave(balls, route.n, px, py, lane_id);
    const bool culled = cand != 0ull && __popcll(cand) <= 8;   // wave-uniform
    const bool small = !culled && route.n <= 64 * kChunks;      // wave-uniform
    float ce[kChunks], hd[kChunks];
    int best;
    float cur_long;
    int my_i = -1;             // (1): this lane's piece, its end longitudinal and heading
    float my_ce = -3.0e38f, my_hd = 0.0f;
    if (culled) {
        my_i = cull_piece_of(cand, route.n, lane_id);
        float bd = 3.0e38f, bl = 0.0f;
        if (my_i >= 0) {
            const MdSeg g = route.segs[my_i];
            bd = md_seg_dist(&g, px, py);
            bl = g.cum + ((px - g.sx) * g.dx + (py - g.sy) * g.dy);   // md_poly_local_at w.r.t. this piece
            my_ce = g.cum + g.len;
            my_hd = g.heading;
        }
        float m = bd;
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) m = md_min(m, __shfl_xor(m, off, 64));
        const unsigned long long mm = __ballot(bd == m);   // lanes ascend with the pieces: the lowest lane = the lowest index
        const int src = __ffsll((long long)mm) - 1;
        best = bcast_i(my_i, src);
        cur_long = bcast_f(bl, src);
    } else if (small) {
        float bd = 3.0e38f, bl = 0.0f;
        int bi = 0x7fffffff;
#pragma unroll
        for (int q = 0; q < kChunks; ++q) {
            const int i = lane_id + 64 * q;
            ce[q] = -3.0e38f;     // never "ends beyond" anything
            hd[q] = 0.0f;
            if (i < route.n) {
                const MdSeg g = route.segs[i];
                const float d = md_seg_dist(&g, px, py);
                if (d < bd) {
                    bd = d;
                    bi = i;
                    bl = g.cum + ((px - g.sx) * g.dx + (py - g.sy) * g.dy);   // md_poly_local_at w.r.t. this piece
                }
                ce[q] = g.cum + g.len;
                hd[q] = g.heading;
            }
        }
        float m = bd;
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) m = md_min(m, __shfl_xor(m, off, 64));
        best = wave_min_i(bi, bd == m, 0x7fffffff);
        cur_long = bcast_f(bl, best & 63);   // the lane of piece `best`; its own best is that piece (strict <)
    } else {
        float tmp;
        best = poly_local_wave(route, balls, px, py, lane_id, &cur_long, &tmp);
    }
    MD_FINE_STAMP(st_, so_ + 2);
    if (do_speed_control) {
        // md_tidm_front_gap's filters that need no route: lanes = movers -- present, within 20 m, and a chassis corner inside the
        // outline's bounding box (a point outside it is outside the outline).  The survivors go on the pair list; when the list
        // is full (never in practice: kPairCap pairs per scene) this wave works its pairs off itself, after publishing cur_long.
        if (lane_id == 0) dl.cur_long[slot] = cur_long;
        wave_lds_sync();
        for (int j0 = 0; j0 < c.cap; j0 += 64) {
            const int jl = j0 + lane_id;
            int want = 0;
            if (jl < c.cap && jl != slot) {
                const MdShape o = s.shape[jl];
                if (md_present(o.flags) && !(md_norm(o.cx - px, o.cy - py) > MD_TIDM_MAX_DIST)) {
                    const float ex = o.c * o.hl, ey = o.s * o.hl, fx = -o.s * o.hw, fy = o.c * o.hw;
                    const float qx[4] = {o.cx + ex + fx, o.cx + ex - fx, o.cx - ex - fx, o.cx - ex + fx};
                    const float qy[4] = {o.cy + ey + fy, o.cy + ey - fy, o.cy - ey - fy, o.cy - ey + fy};
#pragma unroll
                    for (int q = 0; q < 4; ++q)
                        if (!(qx[q] < bx0 || qx[q] > bx1 || qy[q] < by0 || qy[q] > by1)) want |= 1 << q;
                }
            }
            unsigned long long mk = __ballot(want != 0);
            if (mk == 0) continue;
            const int cnt = __popcll(mk);
            int r0 = 0;
            if (lane_id == 0) r0 = atomicAdd(&dl.ctl[0], cnt);
            r0 = uni_i(r0);
            if (r0 + cnt <= kPairCap) {
                if (want != 0) dl.pairs[r0 + __popcll(mk & ((1ull << lane_id) - 1ull))] = (uint32_t)slot | ((uint32_t)jl << 8) | ((uint32_t)want << 16);
            } else {
                for (int i = r0 + lane_id; i < kPairCap; i += 64) dl.pairs[i] = kNullPair;   // the part of the reservation inside the list
                while (mk) {
                    const int b = __ffsll((long long)mk) - 1;
                    mk &= mk - 1;
                    tidm_pair_wave(s, slot, j0 + b, uni_i(__shfl(want, b, 64)), lane_id, l_desc, dl);
                }
            }
        }
    }
    MD_FINE_STAMP(st_, so_ + 3);
    // heading of the route one metre ahead: the first piece that ends beyond it (md_poly_seg_heading), else the last one
    const float ahead = cur_long + 1.0f;
    float lane_heading = 0.0f;
    bool have_heading = false;
    if (culled) {
        // the first piece that ends beyond `ahead`, among the pieces in the lanes: it is THE first one when the piece before it is in
        // the lanes too (and does not end beyond) or there is none before it -- every piece but a route's last is longer than 1 m,
        // so the end longitudinals ascend.  Otherwise (the look-ahead leaves the surviving groups) the generic search below.
        const unsigned long long mf = __ballot(my_i >= 0 && my_ce > ahead);
        if (mf) {
            const int src = __ffsll((long long)mf) - 1;
            const int ih = bcast_i(my_i, src);
            const int prev = (src > 0) ? bcast_i(my_i, src - 1) : -2;
            if (ih == 0 || prev == ih - 1) {
                lane_heading = bcast_f(my_hd, src);
                have_heading = true;
            }
        }
    }
    if (have_heading) {
    } else if (small) {
        int ih = route.n - 1;
        bool found = false;
#pragma unroll
        for (int q = 0; q < kChunks; ++q) {
            const unsigned long long m = __ballot(ce[q] > ahead);
            if (!found && m) {
                ih = 64 * q + __ffsll((long long)m) - 1;
                found = true;
            }
        }
        lane_heading = 0.0f;
#pragma unroll
        for (int q = 0; q < kChunks; ++q)
            if ((ih >> 6) == q) lane_heading = bcast_f(hd[q], ih & 63);
    } else {
        const int ih = poly_first_wave(route, lane_id, [ahead](const MdSeg& g) { return g.cum + g.len > ahead; });
        lane_heading = route.segs[ih].heading;
    }
    MD_FINE_STAMP(st_, so_ + 4);
    if (lane_id == 0) {
        dl.cur_long[slot] = cur_long;
        dl.heading[slot] = lane_heading;
    }
    MD_FINE_STAMP(st_, so_ + 5);
}

// The route cut at a spawn frame, built by one wave from the positions staged in LDS (md_build_route is the serial form; the element
// functions are the same, so the results are bit-identical): the chain of kept points with lanes = candidate points (one ballot per
// piece), the pieces with lanes = pieces (dropped ones squeezed out by ballot prefix counts), the running length on lane 0 (a sum in
// a fixed order), the outline with lanes = vertices.  A few per scene and episode; ~3 us instead of ~40 on one lane.
//   l_link [seg_cap] ints, l_len [seg_cap + 1] doubles: LDS scratch.  rn = the slot's route_n[4].
__device__ __forceinline__ void build_route_wave(int32_t* rn, MdSeg* segs, int seg_cap, float* verts, int vert_cap, float* aux,
                                 const float* l_pts, int n_pts, int* l_link, double* l_len, int lane) {
    int nl = 0, i = 0;
    while (i < n_pts - 1 && nl < seg_cap) {
        int j = n_pts - 1;
        for (int q0 = i + 1; q0 < n_pts; q0 += 64) {
            const int q = q0 + lane;
            const unsigned long long m = __ballot(q < n_pts && md_route_far(l_pts, 2, i, q));
            if (m) {
                j = q0 + __ffsll((long long)m) - 1;
                break;
            }
        }
        if (lane == 0) l_link[nl] = i | (j << 16);
        ++nl;
        i = j;
    }
    wave_lds_sync();
    int ns = 0;
    for (int p0 = 0; p0 < nl; p0 += 64) {
        const int p = p0 + lane;
        MdSeg g;
        double L = -1.0;
        if (p < nl) {
            const int lk = l_link[p];
            L = md_route_piece(l_pts, 2, lk & 0xffff, lk >> 16, &g);
        }
        const bool keep = !(L < 0.0);
        const unsigned long long m = __ballot(keep);
        const int at = ns + __popcll(m & ((1ull << lane) - 1ull));
        if (keep) {
            segs[at] = g;
            l_len[at] = L;
        }
        ns += __popcll(m);
    }
    __threadfence_block();
    wave_lds_sync();
    const int never_moved = ns == 0;
    if (lane == 0) {
        if (never_moved) {
            md_route_still_piece(l_pts, &segs[0]);
            l_len[seg_cap] = 0.1;
        } else {
            double cum = 0.0;
            for (int p = 0; p < ns; ++p) {
                segs[p].cum = (float)cum;
                cum += l_len[p];
            }
            l_len[seg_cap] = cum;
        }
    }
    if (never_moved) ns = 1;
    __threadfence_block();
    wave_lds_sync();
    const int n_long = md_route_n_long(l_len[seg_cap]);
    const int nv = 2 * (n_long + 2);
    if (nv > vert_cap) {   // (the host sizes the buffers by the longest run: never) the slot keeps its static polyline
        if (lane == 0) rn[0] = rn[1] = rn[3] = 0;
        return;
    }
    float bx0 = 3.0e38f, by0 = 3.0e38f, bx1 = -3.0e38f, by1 = -3.0e38f;
    for (int o0 = 0; o0 < nv; o0 += 64) {
        const int o = o0 + lane;
        if (o < nv) {
            float fx, fy;
            md_route_outline_vertex(segs, ns, never_moved, n_long, o, &fx, &fy);
            verts[2 * o] = fx;
            verts[2 * o + 1] = fy;
            bx0 = md_min(bx0, fx);
            by0 = md_min(by0, fy);
            bx1 = md_max(bx1, fx);
            by1 = md_max(by1, fy);
        }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        bx0 = md_min(bx0, __shfl_xor(bx0, off, 64));
        by0 = md_min(by0, __shfl_xor(by0, off, 64));
        bx1 = md_max(bx1, __shfl_xor(bx1, off, 64));
        by1 = md_max(by1, __shfl_xor(by1, off, 64));
    }
    if (lane == 0) {
        md_route_end_point(segs, ns, aux);
        aux[2] = bx0;
        aux[3] = by0;
        aux[4] = bx1;
        aux[5] = by1;
        aux[6] = aux[7] = 0.0f;
        rn[0] = ns;
        rn[1] = nv;
        rn[3] = 0;
    }
}

// Register budget of the scenario kernel: 8 waves per SIMD (64 VGPRs, one spilled) -- 2048 scenes = 256 CUs x 8 workgroups
// are then resident at once, one round instead of two (measured 148 vs 173 us at the compiler's own choice)
// Diagnostic builds only (tools/ab/sc_knockout.sh): stages left out to read their marginal cost off the launch time.  0 in the product.
#ifndef MD_SC_SKIP
#define MD_SC_SKIP 0
#endif
#ifndef MD_SC_WAVES_EU
#define MD_SC_WAVES_EU 8
#endif
// LDS image of one scene in scenario_step_kernel.  n_det = n_side + n_lane_line (the detectors' share is there whenever the
// config has beams); routes: the scene builds routes (MdState.route_n set), each of at most seg_cap pieces.
struct ScenarioLds {
    uint32_t shape, dyn, pid, param, nav, action, flags, cfl, loc, count, dbest, beams, pairs;
    uint32_t key, cur_long, heading, dpairs, ctl;   // the decision stage's scratch (DecideLds) ...
    uint32_t len, pts, link;                        // ... and the route builder's, at the same offset (the traffic manager builds later)
    uint32_t rn, shape_ct, desc, bytes;
};
__host__ __device__ inline ScenarioLds scenario_lds(int cap, int agents, int n_det, bool routes, int seg_cap) {
    ScenarioLds L;
    L.shape = 0;                                                     // the 16-B records are staged as uint4
    L.dyn = L.shape + (uint32_t)cap * sizeof(MdShape);
    L.pid = L.dyn + (uint32_t)cap * sizeof(MdDyn);
    L.param = L.pid + (uint32_t)cap * sizeof(MdPid);
    L.nav = L.param + (uint32_t)cap * sizeof(MdParam);
    L.action = L.nav + (uint32_t)cap * sizeof(MdNav);                  // [cap][2] floats
    L.flags = L.action + (uint32_t)cap * 2 * sizeof(float);
    L.cfl = L.flags + (uint32_t)cap * sizeof(uint32_t);
    L.loc = L.cfl + (uint32_t)((cap + 3) & ~3) * sizeof(uint32_t);    // [agents]
    L.count = L.loc + (uint32_t)agents * sizeof(MdTrajLoc);           // 4 ints: next_agent_id, the traffic manager's two counters, route length
    L.dbest = L.count + 4 * sizeof(int);                             // [agents][n_det] detector fractions (bit patterns)
    L.beams = L.dbest + (uint32_t)agents * n_det * sizeof(int);        // [n_det][2] the beam tables
    L.pairs = L.beams + (uint32_t)n_det * 2 * sizeof(float);           // [2][kDetPairs] pair lists of the two detector waves
    const uint32_t shared = align_up(L.pairs + (n_det > 0 ? 2 * (uint32_t)kDetPairs * sizeof(int) : 0), 8);
    L.key = shared;                                                  // [cap] unsigned long long
    L.cur_long = L.key + (uint32_t)cap * sizeof(unsigned long long);
    L.heading = L.cur_long + (uint32_t)cap * sizeof(float);
    L.dpairs = L.heading + (uint32_t)cap * sizeof(float);              // [kPairCap]
    L.ctl = L.dpairs + (uint32_t)kPairCap * sizeof(uint32_t);          // 2 ints
    const uint32_t decide_end = L.ctl + 2 * sizeof(int);
    L.len = shared;                                                  // [seg_cap + 1] doubles
    L.pts = L.len + (uint32_t)(seg_cap + 1) * sizeof(double);          // [seg_cap][2] floats
    L.link = L.pts + (uint32_t)seg_cap * 2 * sizeof(float);            // [seg_cap] ints
    const uint32_t build_end = routes ? L.link + (uint32_t)seg_cap * sizeof(int) : shared;
    L.rn = decide_end > build_end ? decide_end : build_end;          // [cap][4] route_n of the scene, when it builds routes
    L.shape_ct = align_up(L.rn + (routes ? (uint32_t)cap * 4 * sizeof(int32_t) : 0), 16);   // [cap], copied as uint4
    L.desc = L.shape_ct + (uint32_t)cap * sizeof(MdShape);             // [cap] RouteDesc (16-B aligned)
    L.bytes = L.desc + (uint32_t)cap * sizeof(RouteDesc);
    return L;
}
// kPool: the batch plays scenes of a pool (MdState.scene_of, the scenario walk).  Without it the walk fields are constants here, so
// that the per-scene lookups of the shared headers fold to scene = env and the kernel is the one of a batch without a walk.
template <bool kPool>
__global__ __launch_bounds__(256)
#if MD_SC_WAVES_EU
__attribute__((amdgpu_waves_per_eu(MD_SC_WAVES_EU, MD_SC_WAVES_EU)))
#endif
void scenario_step_kernel(MdWorld w, MdState g, MdConfig c, float* lidar_out, int lidar_stride,
                                                           int lidar_offset) {
    constexpr int kBlock = 256, kWaves = 4;
    if (!kPool) {
        g.scene_of = nullptr;
        g.walk_ep = nullptr;
        g.walk = MdWalk{};
    }
    const int e = blockIdx.x;
    if (e >= c.n_envs) return;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int cap = c.cap, A = c.agents_per_env;
    const bool fused_det = (w.side_beam_cs != nullptr && c.n_side > 0) || (w.ll_beam_cs != nullptr && c.n_lane_line > 0);
    const int n_det = (w.side_beam_cs ? c.n_side : 0) + (w.ll_beam_cs ? c.n_lane_line : 0);
    const ScenarioLds L = scenario_lds(cap, A, c.n_side + c.n_lane_line, g.route_n != nullptr, c.route_seg_cap);
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    MdShape* l_shape = reinterpret_cast<MdShape*>(smem + L.shape);
    MdDyn* l_dyn = reinterpret_cast<MdDyn*>(smem + L.dyn);
    MdPid* l_pid = reinterpret_cast<MdPid*>(smem + L.pid);
    MdParam* l_param = reinterpret_cast<MdParam*>(smem + L.param);
    MdNav* l_nav = reinterpret_cast<MdNav*>(smem + L.nav);
    float* l_action = reinterpret_cast<float*>(smem + L.action);
    uint32_t* l_flags = reinterpret_cast<uint32_t*>(smem + L.flags);
    uint32_t* l_cfl = reinterpret_cast<uint32_t*>(smem + L.cfl);
    const EnvImage img = {l_shape, l_dyn, l_pid, l_param, l_nav, l_action, l_flags, nullptr};   // a scene stages no final lanes
    MdTrajLoc* l_loc = reinterpret_cast<MdTrajLoc*>(smem + L.loc);
    int* l_count = reinterpret_cast<int*>(smem + L.count);
    int* l_dbest = reinterpret_cast<int*>(smem + L.dbest);   // [A][n_det] when md_step runs the detectors
    float* l_beams = reinterpret_cast<float*>(smem + L.beams);   // [n_det][2]: read n_beams times per quad
    int* l_det_pairs = reinterpret_cast<int*>(smem + L.pairs);
    // the positions, lengths and links a route cut at a spawn frame is built from
    double* l_len = reinterpret_cast<double*>(smem + L.len);
    float* l_pts = reinterpret_cast<float*>(smem + L.pts);
    int* l_link = reinterpret_cast<int*>(smem + L.link);
    DecideLds dl;   // on the builder's words
    dl.key = reinterpret_cast<unsigned long long*>(smem + L.key);
    dl.cur_long = reinterpret_cast<float*>(smem + L.cur_long);
    dl.heading = reinterpret_cast<float*>(smem + L.heading);
    dl.pairs = reinterpret_cast<uint32_t*>(smem + L.dpairs);
    dl.ctl = reinterpret_cast<int*>(smem + L.ctl);
    int32_t* l_rn = reinterpret_cast<int32_t*>(smem + L.rn);   // [cap][4]: route_n of the scene (the decisions read it first: not a global round trip)
    // [cap] the movers as the agent's contact test sees them: after the integration, BEFORE the traffic manager's after_step
    MdShape* l_shape_ct = reinterpret_cast<MdShape*>(smem + L.shape_ct);
    RouteDesc* l_desc = reinterpret_cast<RouteDesc*>(smem + L.desc);   // [cap] what the decisions know about each slot's route

    MD_STAMP_AT(0);
    const MdState gv = md_env_view(&g, &c, e);
    const int reset_flag = gv.need_reset[0];
    const bool fused_act = gv.agent_action != nullptr;
    const bool do_reset = reset_flag != 0;
    {
        // ONE memory round trip: every global load of the live state is issued before the first LDS store, and nothing waits for
        // the reset flag (a chain of copy loops waits for each loop's loads in turn: ~15 k cycles per scene); only a scene that
        // resets re-stages from the snapshot below.  16-byte units: shape / dyn / pid / param cap * 2 each, nav cap * 4.
        const int n32 = cap * 2, n64 = cap * 4;
        const uint4* g_shape = reinterpret_cast<const uint4*>(gv.shape);
        const uint4* g_dyn = reinterpret_cast<const uint4*>(gv.dyn);
        const uint4* g_pid = reinterpret_cast<const uint4*>(gv.pid);
        const uint4* g_param = reinterpret_cast<const uint4*>(gv.param);
        const uint4* g_nav = reinterpret_cast<const uint4*>(gv.nav);
        uint4 r_shape, r_dyn, r_pid, r_param, r_nav0, r_nav1;
        float2 r_act;
        uint32_t r_fl;
        int po0 = 0, po1 = 0, pv0 = 0, pv1 = 0, pb0 = 0, rn0 = 0, rn1 = 0, rn2 = 0, rn3 = 0, r_cnt = 0;
        const bool has_balls = w.poly_ball != nullptr && w.poly_ball_off != nullptr;
        float ax[6];
        const bool p32 = tid < n32, pc = tid < cap;
        if (p32) {
            r_shape = g_shape[tid];
            r_dyn = g_dyn[tid];
            r_pid = g_pid[tid];
            r_param = g_param[tid];
        }
        if (tid < n64) r_nav0 = g_nav[tid];
        if (tid + kBlock < n64) r_nav1 = g_nav[tid + kBlock];
        if (pc) {
            r_act = (fused_act && tid < A) ? reinterpret_cast<const float2*>(gv.agent_action)[tid] : reinterpret_cast<const float2*>(gv.action)[tid];
            r_fl = gv.flags[tid];
            // the slot's route record (md_route_of + MdWorld.poly_aux): every address is known here
            const size_t ng = (size_t)md_scene_of_env(&g, e) * cap + tid;   // the scene this env plays (MdState.scene_of)
            po0 = w.poly_off[ng];
            po1 = w.poly_off[ng + 1];
            pv0 = w.polyv_off[ng];
            pv1 = w.polyv_off[ng + 1];
            if (has_balls) pb0 = w.poly_ball_off[ng];
            if (w.poly_aux) {
#pragma unroll
                for (int q = 0; q < 6; ++q) ax[q] = w.poly_aux[8 * ng + q];
            }
            if (gv.route_n) {
                rn0 = gv.route_n[4 * tid];
                rn1 = gv.route_n[4 * tid + 1];
                rn2 = gv.route_n[4 * tid + 2];
                rn3 = gv.route_n[4 * tid + 3];
            }
        }
        if (tid == 0) r_cnt = gv.next_agent_id[0];
        if (p32) {
            reinterpret_cast<uint4*>(l_shape)[tid] = r_shape;
            reinterpret_cast<uint4*>(l_dyn)[tid] = r_dyn;
            reinterpret_cast<uint4*>(l_pid)[tid] = r_pid;
            reinterpret_cast<uint4*>(l_param)[tid] = r_param;
        }
        if (tid < n64) reinterpret_cast<uint4*>(l_nav)[tid] = r_nav0;
        if (tid + kBlock < n64) reinterpret_cast<uint4*>(l_nav)[tid + kBlock] = r_nav1;
        if (pc) {
            reinterpret_cast<float2*>(l_action)[tid] = r_act;
            l_flags[tid] = r_fl;
            if (do_reset) rn0 = rn1 = rn2 = rn3 = 0;   // a reset leaves no cut routes
            if (gv.route_n) {
                l_rn[4 * tid] = rn0;
                l_rn[4 * tid + 1] = rn1;
                l_rn[4 * tid + 2] = rn2;
                l_rn[4 * tid + 3] = rn3;
            }
            RouteDesc d;
            d.pad_[0] = d.pad_[1] = 0;
            if (rn0 > 0 && tid >= A) {   // a route cut at a spawn frame (rare; never an agent's: its slot keeps the reference trajectory): its record lives in the state, one more trip for this lane
                d.segs = gv.route_segs + (size_t)tid * c.route_seg_cap;
                d.verts = gv.route_verts + 2 * (size_t)tid * c.route_vert_cap;
                d.balls = nullptr;
                d.n = rn0;
                d.n_verts = rn1;
                const float* ra = gv.route_aux + 8 * (size_t)tid;
                d.end_x = ra[0];
                d.end_y = ra[1];
                d.bx0 = ra[2];
                d.by0 = ra[3];
                d.bx1 = ra[4];
                d.by1 = ra[5];
            } else {
                d.segs = w.segs + po0;
                d.verts = w.polyv + 2 * (size_t)pv0;
                d.balls = has_balls ? reinterpret_cast<const float4*>(w.poly_ball) + pb0 : nullptr;
                d.n = po1 - po0;
                d.n_verts = (pv1 - pv0) | (w.poly_aux ? 0 : kDescNoAux);
                d.end_x = w.poly_aux ? ax[0] : 0.0f;
                d.end_y = w.poly_aux ? ax[1] : 0.0f;
                d.bx0 = w.poly_aux ? ax[2] : 0.0f;
                d.by0 = w.poly_aux ? ax[3] : 0.0f;
                d.bx1 = w.poly_aux ? ax[4] : 0.0f;
                d.by1 = w.poly_aux ? ax[5] : 0.0f;
            }
            l_desc[tid] = d;
        }
        if (tid == 0) *l_count = do_reset ? 0 : r_cnt;   // idm_policy_count
    }
    if (do_reset) {   // block-uniform, rare: the snapshot over what was just staged (same threads wrote the same words: no barrier needed
                      // between a thread's own stores, and the barrier below orders everything before the first read)
        __syncthreads();
        copy16(l_shape, gv.shape0, cap * (int)sizeof(MdShape), tid, kBlock);
        copy16(l_dyn, gv.dyn0, cap * (int)sizeof(MdDyn), tid, kBlock);
        copy16(l_pid, gv.pid0, cap * (int)sizeof(MdPid), tid, kBlock);
        copy16(l_nav, gv.nav0, cap * (int)sizeof(MdNav), tid, kBlock);
        for (int j = tid; j < cap; j += kBlock) {
            l_action[2 * j] = 0.0f;
            l_action[2 * j + 1] = 0.0f;
            l_flags[j] = 0u;
        }
    }
    if (fused_det) {
        const int ns = w.side_beam_cs ? c.n_side : 0;
        for (int it = tid; it < A * n_det; it += kBlock) l_dbest[it] = __float_as_int(1.0f);
        for (int it = tid; it < 2 * n_det; it += kBlock)
            l_beams[it] = (it < 2 * ns) ? w.side_beam_cs[it] : w.ll_beam_cs[it - 2 * ns];
    }
    MdState s = local_view(gv, img);
    s.final_lane = gv.final_lane;   // not staged
    if (gv.route_n) s.route_n = l_rn;
    s.next_agent_id = l_count;
    __syncthreads();
    MD_STAMP_AT(1);
    const int just_reset = do_reset ? 1 : 0;
    const int k = just_reset ? 0 : s.nav[0].steps + 1;   // engine.episode_step of this step
    constexpr int kSkip = MD_SC_SKIP;
    if (!just_reset) {
        // Work list of the reactive vehicles, those due for speed control in this step FIRST (their front search makes them
        // ~2.5x as expensive as the others); the waves then take vehicles off the list one by one through an LDS counter,
        // so a wave that drew a cheap vehicle moves on instead of waiting at the barrier (every wave leaves the loop as
        // soon as the counter passes the list's end: no waiting inside).  The decisions are independent of each other,
        // so the order changes nothing in the results.
        int* l_list = reinterpret_cast<int*>(l_cfl);   // free until the contacts stage writes its flags
        int* l_ctr = l_count + 1;
        int* l_n = l_count + 2;
        if (wave == 0) {
            int n = 0;
            for (int pass = 0; pass < 2; ++pass)
                for (int j0 = A; j0 < cap; j0 += 64) {
                    const int j = j0 + lane;
                    bool take = false;
                    if (j < cap && s.nav[j].ck0 == MD_SC_IDM && md_present(s.shape[j].flags)) {
                        const bool sc = (k % MD_TIDM_BATCH) == s.nav[j].timer;
                        take = (pass == 0) ? sc : !sc;
                    }
                    const unsigned long long m = __ballot(take);
                    if (take) l_list[n + __popcll(m & ((1ull << lane) - 1ull))] = j;
                    n += __popcll(m);
                }
            if (lane == 0) {
                *l_n = n;
                *l_ctr = 0;
            }
        }
        for (int j = tid; j < cap; j += kBlock) dl.key[j] = kNoFront;
        if (tid == 64) dl.ctl[0] = dl.ctl[1] = 0;
        __syncthreads();
        const int n_list = __builtin_amdgcn_readfirstlane(*l_n);
        // (A) per vehicle: arrival, own projection, heading ahead, the speed-control vehicles' candidate pairs
        for (int guard = 0; guard < cap; ++guard) {   // at most cap tickets per wave: the loop ends whatever the counter holds
            int i = 0;
            if (lane == 0) i = atomicAdd(l_ctr, 1);
            i = __builtin_amdgcn_readfirstlane(i);     // lane 0's ticket, in a scalar register
            if (i < 0 || i >= n_list) break;
            const int slot = __builtin_amdgcn_readfirstlane(l_list[i]);
            if (slot < A || slot >= cap) break;        // never index with anything but a mover slot
            if (kSkip & 32) {
                if (lane == 0) dl.cur_long[slot] = __int_as_float(0x7fc00000);
                continue;
            }
            tidm_prepare_wave(w, s, c, e, slot, k, lane, l_desc, dl);
        }
        __syncthreads();
        // (B) the pairs, one per ticket
        const int n_pairs = min(__builtin_amdgcn_readfirstlane(dl.ctl[0]), kPairCap);
        for (int guard = 0; guard < kPairCap; ++guard) {
            int i = 0;
            if (lane == 0) i = atomicAdd(&dl.ctl[1], 1);
            i = __builtin_amdgcn_readfirstlane(i);
            if (i < 0 || i >= n_pairs) break;
            const uint32_t pr = (uint32_t)__builtin_amdgcn_readfirstlane((int)dl.pairs[i]);
            if (pr == kNullPair || (kSkip & 16)) continue;
            const int slot = pr & 0xff, j = (pr >> 8) & 0xff, want = (pr >> 16) & 0xf;
            if (slot < A || slot >= cap || j >= cap) break;
            tidm_pair_wave(s, slot, j, want, lane, l_desc, dl);
        }
        __syncthreads();
        // (C) steering + acceleration (md_tidm_decide): one lane per vehicle
        for (int i = tid; i < n_list; i += kBlock) {
            const int slot = l_list[i];
            const float cl = dl.cur_long[slot];
            if (slot >= A && slot < cap && cl == cl) {   // NaN: arrived
                const unsigned long long key = dl.key[slot];
                const int front = (key == kNoFront) ? -1 : (int)(key & 0xffffffffull);
                const float front_dist = (key == kNoFront) ? MD_TIDM_MAX_DIST : __uint_as_float((unsigned)(key >> 32));
                const int do_speed_control = (k % MD_TIDM_BATCH) == s.nav[slot].timer;
                md_tidm_decide(nullptr, &s, slot, do_speed_control, front, front_dist, dl.heading[slot]);
            }
        }
        __syncthreads();
        MD_STAMP_AT(2);
        for (int j = tid; j < cap; j += kBlock) {
            if (c.ego_replay && j < A) md_scenario_replay_ego(&s, &c, j, k);   // agent_policy = ReplayEgoCarPolicy
            else if (!(kSkip & 128)) md_integrate_mover(&s, &c, j);
            l_shape_ct[j] = l_shape[j];   // what the contact test below sees
        }
        __syncthreads();
    }
    MD_STAMP_AT(3);
    // The agent's contact flags come from BaseVehicle.after_step (a contact test at the bodies' present poses), which the agent
    // manager runs BEFORE the traffic manager's after_step: replayed bodies are still at frame k-1, bodies removed / spawned in
    // this step are still / not yet there.  Wave 1 tests against a snapshot of the shapes while wave 0 runs after_step and the
    // agent's projection, and waves 2 / 3 the detectors: one stage, one barrier.
    if (just_reset) {
        copy16(l_shape_ct, l_shape, cap * (int)sizeof(MdShape), tid, kBlock);
        __syncthreads();
    }
    if (wave == 1 && !(kSkip & 4)) {
        MdState sc = s;
        sc.shape = l_shape_ct;
        for (int a = 0; a < A; ++a) contacts_vehicle(w, sc, c, e, a, lane, l_cfl);
    }
    // ---- after_step of the traffic manager: lanes = track slots, in slot order ----
    if (wave == 0 && !(kSkip & 64)) {
        for (int j0 = A; j0 < cap; j0 += 64) {
            const int j = j0 + lane;
            const bool in = j < cap;
            const int wants = in ? md_scenario_slot_after_step(&w, &s, &c, e, j, k, 0, 1) : 0;
            const unsigned long long m = __ballot(wants != 0);
            const int before = *l_count + __popcll(m & ((1ull << lane) - 1ull));
            if (in) md_scenario_slot_after_step(&w, &s, &c, e, j, k, before, 0);
            __builtin_amdgcn_wave_barrier();
            if (lane == 0) *l_count += __popcll(m);
            wave_lds_sync();
            // a reactive policy created at a frame other than its first run's start: its route is cut at this frame.  Rare
            // (a few per scene and episode): the wave stages the run's remaining positions, lane 0 builds (md_build_route).
            unsigned long long mb = __ballot(in && s.route_n != nullptr && s.route_n[4 * (in ? j : 0) + 3] > 0);
            while (mb) {
                const int jb = j0 + __ffsll((long long)mb) - 1;
                mb &= mb - 1;
                const int kb = s.route_n[4 * jb + 2];
                const int nb = min(s.route_n[4 * jb + 3], c.route_seg_cap);
                for (int i = lane; i < nb; i += 64) {
                    const MdShape fr = s.track_shape[(size_t)(kb + i) * md_track_stride(&s, &c) + (size_t)jb];
                    l_pts[2 * i] = fr.cx;
                    l_pts[2 * i + 1] = fr.cy;
                }
                wave_lds_sync();
                build_route_wave(s.route_n + 4 * jb, s.route_segs + (size_t)jb * c.route_seg_cap, c.route_seg_cap,
                                 s.route_verts + 2 * (size_t)jb * c.route_vert_cap, c.route_vert_cap, s.route_aux + 8 * (size_t)jb, l_pts, nb,
                                 l_link, l_len, lane);
                wave_lds_sync();
            }
        }
    }
    MD_STAMP_AT(4);
    // ---- the agents, in the same stage (nothing below reads a slot after_step writes: the agent's own pose is final after the
    // integration): projection on the reference trajectory (wave 0, after its after_step); waves 2, 3: the detectors ----
    for (int a = 0; a < A; ++a) {
        if (wave == 0) {
            // the reference trajectory = the agent slot's static polyline (md_poly_of): its record is in LDS already
            MdPoly ref;
            ref.segs = uni_p(l_desc[a].segs);
            ref.n = uni_i(l_desc[a].n);
            ref.length = 0.0f;
            MdTrajLoc L;
            float ref_len;
            if (kSkip & 8) {
                L.lng = L.lat = L.heading_at = L.lat_dy = 0.0f;
                L.lat_dx = 1.0f;
                ref_len = 100.0f;
            } else
                traj_locate_wave(ref, s.shape[a].cx, s.shape[a].cy, lane, &L, &ref_len);
            if (lane == 0) {
                l_loc[a] = L;
                l_count[3] = __float_as_int(ref_len);   // single-agent scenes (md_step refuses others): one length
            }
        } else if (wave >= 2 && fused_det && !(kSkip & 2)) {
            // waves 2 and 3 have nothing to do in this stage and the next: the side / lane-line detectors of the agent,
            // each wave one half of the scene's line pieces (the poses are final here)
            const MdShape me = s.shape[a];
            if (md_present(me.flags)) {
                const int mq = w.env_map[e];
                const int q0 = w.quad_off[mq], q1 = w.quad_off[mq + 1];
                const int half = (q1 - q0 + 1) >> 1;
                const int qa = q0 + (wave - 2) * half, qb = min(qa + half, q1);
                int* best = l_dbest + a * n_det;
                const int ns = w.side_beam_cs ? c.n_side : 0;
                int* pairs = l_det_pairs + (wave - 2) * kDetPairs;   // this wave's pair list
                if (w.side_beam_cs && c.n_side > 0)
                    detector_wave(w, me, qa, qb, l_beams, c.n_side, c.side_range, c.side_mask, best, pairs, lane);
                if (w.ll_beam_cs && c.n_lane_line > 0)
                    detector_wave(w, me, qa, qb, l_beams + 2 * ns, c.n_lane_line, c.ll_range, c.ll_mask, best + ns, pairs, lane);
            }
        }
    }
    __syncthreads();
    MD_STAMP_AT(5);
    // the nine way points of the navigation vector: one lane each (wave 0), both slots of a way point get the value
    if (wave == 0 && lane < MD_TRAJ_NUM_WAY_POINT - 1) {
        const int sc = md_scene_of_env(&g, e);
        const int k0 = w.ckpt_off[sc], n_ck = w.ckpt_off[sc + 1] - k0;
        const float* ck = w.ckpt_xy + 2 * (size_t)k0;
        for (int a = 0; a < A; ++a) {
            const MdTrajLoc L = l_loc[a];
            const MdShape sh = s.shape[a];
            const float v = md_traj_navi_point(ck, n_ck, md_traj_next_idx(&L, n_ck), lane, sh.cx, sh.cy, sh.c, sh.s);
            float* o = s.obs + (size_t)a * c.obs_dim + md_sc_obs_navi(&c);
            o[2 * lane] = v;
            o[2 * lane + 1] = v;
        }
    }
    if (tid < A) {
        const int a = tid;
        s.flags[a] = l_cfl[a];
        md_scenario_observe_at(&w, &s, &c, e, a, just_reset, &l_loc[a], __int_as_float(l_count[3]), 0);
    }
    MD_STAMP_AT(6);
    if (c.n_beams > 0 && !(kSkip & 1)) phase_lidar(w, s, c, e, tid, kWaves, lidar_out, lidar_stride, lidar_offset, nullptr);
    __syncthreads();
    MD_STAMP_AT(7);
    if (fused_det) {   // after the observation (whose lane 0 filled these dims with "nothing seen")
        const int ns = w.side_beam_cs ? c.n_side : 0;
        for (int it = tid; it < A * n_det; it += kBlock) {
            const int a = it / n_det, i = it - a * n_det;
            float* o = s.obs + (size_t)a * c.obs_dim;
            if (i < ns) o[md_obs_base(&c) + i] = __int_as_float(l_dbest[it]);
            else o[md_obs_ll(&c) + (i - ns)] = __int_as_float(l_dbest[it]);
        }
    }
    copy16(gv.shape, l_shape, cap * (int)sizeof(MdShape), tid, kBlock);
    copy16(gv.dyn, l_dyn, cap * (int)sizeof(MdDyn), tid, kBlock);
    copy16(gv.pid, l_pid, cap * (int)sizeof(MdPid), tid, kBlock);
    copy16(gv.nav, l_nav, cap * (int)sizeof(MdNav), tid, kBlock);
    for (int j = tid; j < cap; j += kBlock) {
        gv.action[2 * j] = l_action[2 * j];
        gv.action[2 * j + 1] = l_action[2 * j + 1];
        gv.flags[j] = l_flags[j];
    }
    if (gv.route_n)
        for (int j = tid; j < 4 * cap; j += kBlock) gv.route_n[j] = l_rn[j];
    if (tid == 0) {
        gv.next_agent_id[0] = *l_count;
        if (do_reset) gv.need_reset[0] = 0;
    }
    MD_STAMP_AT(11);
}

// Lidar.perceive as a sensor on its own (md_lidar_detect): cloud points AND the detected-object sets, from nothing but
// the shape table.  One workgroup per env, shapes + sets in LDS, (agent, sector) items dealt to the waves.
struct LidarDetectLds { uint32_t shape, det, bytes; };
__host__ __device__ inline LidarDetectLds lidar_detect_lds(int cap, int agents) {
    LidarDetectLds L;
    L.shape = 0;                                                     // copy16
    L.det = L.shape + (uint32_t)cap * sizeof(MdShape);                 // [agents][2] detected sets
    L.bytes = L.det + (uint32_t)agents * 2 * sizeof(unsigned long long);
    return L;
}
__global__ __launch_bounds__(256) void lidar_detect_kernel(MdWorld w, MdState g, MdConfig c, float* out, int out_stride, int out_offset,
                                                          unsigned long long* detected) {
    const int e = blockIdx.x;
    if (e >= c.n_envs) return;
    const int tid = threadIdx.x;
    const LidarDetectLds L = lidar_detect_lds(c.cap, c.agents_per_env);
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    MdShape* l_shape = reinterpret_cast<MdShape*>(smem + L.shape);
    unsigned long long* l_det = reinterpret_cast<unsigned long long*>(smem + L.det);
    copy16(l_shape, g.shape + (size_t)e * c.cap, c.cap * (int)sizeof(MdShape), tid, 256);
    for (int j = tid; j < 2 * c.agents_per_env; j += 256) l_det[j] = 0ull;
    __syncthreads();
    MdState s = g;
    s.shape = l_shape;
    phase_lidar(w, s, c, e, tid, 4, out, out_stride, out_offset, l_det);
    __syncthreads();
    for (int j = tid; j < 2 * c.agents_per_env; j += 256) detected[(size_t)e * c.agents_per_env * 2 + j] = l_det[j];
}

// The move of an env onto a staged draw / pool scene: the snapshot rows and per-slot constants of live slots [row, + cap) from
// staged slots [from, + cap), by threads tid of nthr (swap_draw_kernel, curriculum_kernel).
__device__ void copy_draw_rows(const MdState& live, const MdState& staged, int cap, size_t row, size_t from, int tid, int nthr) {
    auto words = [&](void* dst, const void* src, size_t elem_words) {   // cap slots of elem_words 4-byte words each
        if (dst == nullptr || src == nullptr) return;
        uint32_t* d = reinterpret_cast<uint32_t*>(dst) + row * elem_words;
        const uint32_t* q = reinterpret_cast<const uint32_t*>(src) + from * elem_words;
        for (size_t i = tid; i < (size_t)cap * elem_words; i += nthr) d[i] = q[i];
    };
    words(const_cast<MdShape*>(live.shape0), staged.shape0, sizeof(MdShape) / 4);
    words(const_cast<MdDyn*>(live.dyn0), staged.dyn0, sizeof(MdDyn) / 4);
    words(const_cast<MdNav*>(live.nav0), staged.nav0, sizeof(MdNav) / 4);
    words(const_cast<MdPid*>(live.pid0), staged.pid0, sizeof(MdPid) / 4);
    words(live.param, staged.param, sizeof(MdParam) / 4);
    words(const_cast<MdParam*>(live.param0), staged.param, sizeof(MdParam) / 4);
    words(live.route_nodes, staged.route_nodes, MD_ROUTE_LEN);
    words(const_cast<int32_t*>(live.route_nodes0), staged.route_nodes, MD_ROUTE_LEN);
    words(live.route_roads, staged.route_roads, MD_ROUTE_LEN);
    words(const_cast<int32_t*>(live.route_roads0), staged.route_roads, MD_ROUTE_LEN);
    words(live.final_lane, staged.final_lane, 1);
    words(const_cast<int32_t*>(live.final_lane0), staged.final_lane, 1);
    words(const_cast<int32_t*>(live.idm_rand), staged.idm_rand, MD_IDM_RAND);
}

// random_traffic with auto-reset (PGTrafficManager with `random_traffic`: the traffic stream is not re-seeded at reset, every episode
// sees other traffic, manager/traffic_manager.py:335-337): the caller stages n_draws host-built traffic draws on the device; an env
// that has just finished its episode (need_reset != 0: md_step restores it from the snapshot at the NEXT step) takes the next draw --
// the snapshot rows and the per-slot constants of the traffic (parameters, routes, pre-drawn lane-change timers) of that env are
// replaced.  One workgroup per env, a no-op for the envs that go on.
// The scenario walk (traffic_mode 4, MdState.walk.mode > 0) is the same move with the scenes for draws: `staged` holds the snapshot rows
// of the n_draws = n_scenes scenes of the pool (scene p at p * cap), `draw_idx` is MdWorld.env_map (the scene's line map); the env
// takes scene md_walk_scene(c, e, walk_ep[e] + 1) and scene_of / walk_ep / env_map follow.  The per-scene tables are only redirected.
// The PG walk (traffic_mode 0 / 1 / 2 with MdState.walk.mode > 0) is that move over a pool of PG scenes: scene p = scenario seed
// start_seed + p, env_map[e] = p picks its map, and the scene's traffic stream state (MdState.rng, the respawn modes) comes along
// with the rows -- the reference re-seeds the traffic manager with the scenario seed at every reset.
__global__ __launch_bounds__(256) void swap_draw_kernel(MdState live, MdState staged, MdConfig c, int n_draws, int32_t* draw_idx) {
    const int e = blockIdx.x;
    if (e >= c.n_envs || live.need_reset[e] == 0) return;   // block-uniform
    const int tid = threadIdx.x;
    const bool walk = live.walk.mode != 0;
    const int ep = walk ? live.walk_ep[e] + 1 : 0;
    const int k = walk ? md_walk_scene(&live.walk, e, ep) : (draw_idx[e] + 1) % n_draws;
    __syncthreads();   // every thread has read the index
    if (tid == 0) {
        draw_idx[e] = k;
        if (walk) {
            live.scene_of[e] = k;
            live.walk_ep[e] = ep;
            if (live.rng && staged.rng) live.rng[e] = staged.rng[k];
        }
    }
    const size_t row = (size_t)e * c.cap, from = walk ? (size_t)k * c.cap : ((size_t)k * c.n_envs + e) * c.cap;
    copy_draw_rows(live, staged, c.cap, row, from, tid, 256);
}

// ScenarioEnv's curriculum manager (include/md_curriculum.h), one wave per env: lane 0 runs the env's state machine, and when the
// env moves on (n_levels > 1) the whole wave copies the new scene's snapshot rows from the pool (`staged`, scene p at p * cap).
// reset = 1: an env reset (every env restarts at its worker's first scene of its level; no report, no put).
__global__ __launch_bounds__(64) void curriculum_kernel(MdState live, MdState staged, MdConfig c, MdCurriculum cu, int32_t* env_map,
                                                        int reset) {
    const int e = blockIdx.x;
    if (e >= c.n_envs) return;
    const int lane = threadIdx.x;
    const bool moves = cu.n_levels > 1;
    int p = -1;
    if (lane == 0) {
        const int follow = moves ? -1 : live.scene_of[e];   // one level: md_swap_draw has moved the env already
        if (reset) {
            p = md_cur_restart(&cu, e, follow);
        } else {
            const size_t a = (size_t)e * c.agents_per_env;
            const int success = (live.flags[(size_t)e * c.cap] & MD_FL_ARRIVE_DEST) != 0;
            p = md_cur_after_step(&cu, e, success, live.step_info[8 * a + 6], live.need_reset[e] != 0, follow);
        }
    }
    p = __shfl(p, 0);
    if (!moves || p < 0) return;   // wave-uniform
    if (lane == 0) {
        live.scene_of[e] = p;
        live.walk_ep[e] = reset ? 0 : live.walk_ep[e] + 1;
        env_map[e] = p;
    }
    copy_draw_rows(live, staged, c.cap, (size_t)e * c.cap, (size_t)p * c.cap, lane, 64);
}

// md_branch (include/md_branch.h): the copy of whole envs between two states, one workgroup per (source row, destination row) pair.
// A pure gather-copy: the workgroup walks the table of per-env extents, then the extras.  Per field the row is moved with the widest
// access both row bases and the length allow -- 16 bytes (the 32 / 64-byte records always), else 4 (an obs row of 259 floats is no
// multiple of 16 bytes), else single bytes (the 1-byte extras) -- decided block-uniformly, and a thread issues up to four loads before
// their stores, so that a field costs one memory round trip, not one per word.  A fan-out reads its one source row from L2.
// No LDS, no atomics; the pairs never meet (the caller keeps destination rows distinct and apart from the source rows).
template <typename T>
__device__ __forceinline__ void branch_copy_as(char* d, const char* s, size_t n, int tid) {
    T* dp = reinterpret_cast<T*>(d);
    const T* sp = reinterpret_cast<const T*>(s);
    for (size_t i = tid; i < n; i += 4 * 256) {
        T v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            v[u] = T{};
            if (i + u * 256 < n) v[u] = sp[i + u * 256];
        }
#pragma unroll
        for (int u = 0; u < 4; ++u)
            if (i + u * 256 < n) dp[i + u * 256] = v[u];
    }
}

// One copy of the three loops for all ~50 call sites (called, not inlined: the kernel stays a few KB of code instead of ~40).
__device__ __noinline__ void branch_rows(void* dst, const void* src, size_t row_bytes, int srow, int drow, int tid) {
    if (dst == nullptr || src == nullptr || row_bytes == 0) return;   // an array this batch does not have
    const char* s = reinterpret_cast<const char*>(src) + (size_t)srow * row_bytes;
    char* d = reinterpret_cast<char*>(dst) + (size_t)drow * row_bytes;
    const uintptr_t bits = (uintptr_t)s | (uintptr_t)d | (uintptr_t)row_bytes;   // block-uniform
    if ((bits & 15) == 0) branch_copy_as<md_u32x4>(d, s, row_bytes >> 4, tid);
    else if ((bits & 3) == 0) branch_copy_as<uint32_t>(d, s, row_bytes >> 2, tid);
    else branch_copy_as<uint8_t>(d, s, row_bytes, tid);
}

__global__ __launch_bounds__(256) void branch_kernel(MdState dst, MdState src, MdConfig c, MdBranch b) {
    const int p = blockIdx.x;
    if (p >= b.n_pairs) return;
    const int srow = b.src_row[p], drow = b.dst_row[p];
    if (srow < 0 || srow >= b.src_n_envs || drow < 0 || drow >= b.dst_n_envs) return;   // block-uniform; the host refuses such a pair
    const int tid = threadIdx.x;
#define MD_BR_COPY(field, unit, bytes, scale) \
    branch_rows((void*)dst.field, (const void*)src.field, md_branch_row_bytes(&c, unit, bytes, scale), srow, drow, tid);
    MD_BRANCH_FIELDS(MD_BR_COPY)
#undef MD_BR_COPY
#pragma unroll
    for (int k = 0; k < MD_BR_MAX_EXTRAS; ++k)
        if (k < b.n_extras) branch_rows(b.extra[k].dst, b.extra[k].src, (size_t)b.extra[k].row_bytes, srow, drow, tid);
}

// ---- crossing pedestrians (include/md_ped.h): ONE WAVE PER ENV, kPedEnvs envs per workgroup ----
// The wave's lanes each load one mover's shape record and speed (two rounds when cap > 64); a lane whose mover is a policy-driven
// pedestrian also loads that walker's nav / pid rows and keeps its crossing (md_ped_geom) in registers, so every global load of
// the launch is issued in the first round trip.  A ballot finds the pedestrians; for each of them in slot order its crossing is
// broadcast from the lane that owns it, every lane tests ITS vehicle(s) (md_ped_vehicle) and two ballots give the hold / yield
// verdicts, which the owner keeps.  After the loop the owners evaluate the scalar part (md_ped_apply) side by side and store their
// walkers' rows: the first version did that on lane 0 inside the loop, one dependent chain of loads per pedestrian (9.5 / 15.3 us
// at 4096 envs x 4 / 8 pedestrians; EXPERIMENTS "Crossing pedestrians").  A pedestrian is no vehicle and reads no other
// pedestrian, so the order of the stores does not matter.  No LDS, no atomics, plain vector stores.
constexpr int kPedEnvs = 4;
static_assert(MD_MAX_CAP <= 128, "ped_kernel: two lane rounds per env");
__device__ __forceinline__ MdPedGeom bcast_ped_geom(const MdPedGeom& g, int src) {
    MdPedGeom o;
    o.ax = bcast_f(g.ax, src);
    o.ay = bcast_f(g.ay, src);
    o.ux = bcast_f(g.ux, src);
    o.uy = bcast_f(g.uy, src);
    o.L = bcast_f(g.L, src);
    o.along = bcast_f(g.along, src);
    o.dir = bcast_f(g.dir, src);
    o.t_cross = bcast_f(g.t_cross, src);
    return o;
}

__global__ __launch_bounds__(64 * kPedEnvs) void ped_kernel(MdState g, MdConfig c, MdPed p) {
    const int lane = threadIdx.x & 63;
    const int e = blockIdx.x * kPedEnvs + (threadIdx.x >> 6);
    if (e >= c.n_envs) return;              // wave-uniform, as everything below that is not a lane's own mover
    if (g.need_reset[e] != 0) return;       // md_step replaces this env's rows by the snapshot
    const int cap = c.cap;
    const size_t b = (size_t)e * (size_t)cap;
    MdState s = g;                          // the env view of the arrays the rule touches
    s.shape = g.shape + b;
    s.dyn = g.dyn + b;
    s.nav = g.nav + b;
    s.pid = g.pid + b;
    s.idm_rand = g.idm_rand + b * MD_IDM_RAND;
    s.need_reset = g.need_reset + e;
    MdShape vs[2] = {};
    float vspeed[2] = {0.0f, 0.0f};
    MdPedGeom mine[2] = {};                 // the crossing of this lane's own pedestrian
    int verdict[2] = {0, 0};
    unsigned long long peds[2] = {0ull, 0ull};
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        if (r * 64 >= cap) break;
        const int j = r * 64 + lane;
        bool driven = false;
        if (j < cap) {
            vs[r] = s.shape[j];
            vspeed[r] = s.dyn[j].speed;
            driven = md_ped_driven(vs[r].flags, &s.nav[j]);
            if (driven) mine[r] = md_ped_geom(&vs[r], &s.nav[j], &s.pid[j], &p);
        }
        peds[r] = __ballot(driven);
    }
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        unsigned long long m = peds[r];
        while (m) {
            const int k = __ffsll((long long)m) - 1;
            m &= m - 1;
            const MdPedGeom gm = bcast_ped_geom(mine[r], k);
            int bits = md_ped_vehicle(&gm, &p, &vs[0], vspeed[0]);
            if (cap > 64) bits |= md_ped_vehicle(&gm, &p, &vs[1], vspeed[1]);
            const int hold = __ballot((bits & MD_PED_HOLD) != 0) != 0ull ? MD_PED_HOLD : 0;
            const int yield = __ballot((bits & MD_PED_YIELD) != 0) != 0ull ? MD_PED_YIELD : 0;
            if (lane == k) verdict[r] = hold | yield;
        }
    }
#pragma unroll
    for (int r = 0; r < 2; ++r)
        if ((peds[r] >> lane) & 1ull) md_ped_apply(&s, &c, &p, r * 64 + lane, &mine[r], verdict[r]);
}

// ---- the vector scene observation (include/md_vector_obs.h): ONE WORKGROUP PER ENV, one wave per (observer, block) ----
// The workgroup first pushes the env's frame into the history ring: every wave reads the cursor as the previous call left it,
// a barrier, the threads store the slots of the newest frame and thread 0 the new cursor, a second barrier.  So the push happens
// once per env and is ordered before every read of the ring.  Then the 3 * A work items (observer a, block: agents + ego | route |
// lanes) are dealt to the waves -- a single-agent env keeps three waves busy, a 40-agent env loops.  Within a wave:
//   agents  lanes take the slots (two per lane at cap > 64) and pack (float bits of d2) << 32 | slot: d2 >= 0, so the key orders
//           as an unsigned integer and the slot breaks ties.  A candidate's rank is the number of candidates with a smaller key,
//           counted over a ballot walk (the candidates inside the radius are few); ranks below K go to an LDS list.  The (K + 1) x T
//           items (the ego is group K) are dealt to the lanes in whole groups of T: a lane evaluates ITS link and a ballot gives the
//           prefix "links 0 .. t all hold" with one mask compare.
//   route   lane i fetches the chain's i-th road, its chain lane and length (three dependent loads in all); the cumulative sum is
//           the serial loop the header states, at most 47 additions over broadcast lengths, during which lane m keeps the first
//           chain lane that reaches waypoint m; the M rows are then evaluated side by side.
//   lanes   the candidate lanes are strided over the wave and their distances kept in LDS, so md_atan2 runs once per (observer,
//           lane); a candidate's rank is counted over the LDS distances, ranks below P go to an LDS list, and the P x S points
//           are dealt to the lanes.
// No atomics, plain vector stores.
constexpr int kVoWaves = 4;
struct VectorObsLds { uint32_t sel, taken, dist, per_wave; };
__host__ __device__ constexpr VectorObsLds vector_obs_lds(int max_lanes) {
    const uint32_t taken = 4u * MD_VO_MAX_AGENTS, dist = taken + 4u * MD_VO_MAX_LANES;
    return VectorObsLds{0u, taken, dist, align_up(dist + 4u * (uint32_t)(max_lanes > 0 ? max_lanes : 0), 16)};
}
__device__ __forceinline__ unsigned long long vo_key(float d, int id) {
    return ((unsigned long long)__float_as_uint(d) << 32) | (unsigned long long)(unsigned)id;
}

// the chain's roads, one per lane of the wave (lane i < *n_chain holds road i; -1 elsewhere)
__device__ __forceinline__ int vo_chain_roads(const MdState& s, const MdObsCtx& k, int a, int lane, int* n_chain) {
    const MdNav* nav = &s.nav[a];
    int n = k.valid ? md_vo_chain_len(nav) : 0;
    int road = -1;
    if (lane < n) road = s.route_roads[(size_t)a * MD_ROUTE_LEN + nav->ck0 + lane];
    const unsigned long long cut = __ballot(lane < n && road < 0);
    if (cut) n = __ffsll((long long)cut) - 1;
    *n_chain = n;
    return lane < n ? road : -1;
}

__device__ __forceinline__ void vo_agents_block(const MdState& s, const MdConfig& c, const MdVectorObs& vo, const MdVoHist& h,
                                                const MdObsCtx& k, const MdVoEgo& ego, const MdVoOut& o, int a, int lane, int* l_sel) {
    const int K = vo.num_agents, T = vo.history, cap = c.cap;
    const float radius2 = vo.radius * vo.radius, max_jump2 = vo.max_jump * vo.max_jump;
    const MdShape me = s.shape[a];
    unsigned long long key[2] = {~0ull, ~0ull};
    bool cand[2] = {false, false};
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        const int j = r * 64 + lane;
        if (k.valid && j < cap && j != a) {
            const MdShape other = s.shape[j];
            float d2;
            cand[r] = md_vo_candidate(&me, &other, radius2, &d2);
            key[r] = vo_key(d2, j);
        }
    }
    if (lane < MD_VO_MAX_AGENTS) l_sel[lane] = -1;
    int rank[2] = {0, 0};
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        unsigned long long m = __ballot(cand[q]);
        while (m) {
            const int l = __ffsll((long long)m) - 1;
            m &= m - 1;
            const unsigned long long kq = __shfl(key[q], l, 64);
            rank[0] += kq < key[0];
            rank[1] += kq < key[1];
        }
    }
#pragma unroll
    for (int r = 0; r < 2; ++r)
        if (cand[r] && rank[r] < K) l_sel[rank[r]] = r * 64 + lane;
    wave_lds_sync();
    const int per = 64 / T;                 // whole groups of T items per round
    for (int g0 = 0; g0 < K + 1; g0 += per) {
        const int gi = lane / T, t = lane - gi * T, r = g0 + gi;
        const bool act = gi < per && r <= K;
        int j = -1;
        if (act) j = r < K ? l_sel[r] : (k.valid ? a : -1);
        const bool link = act && j >= 0 && md_vo_link(&h, max_jump2, j, t);
        const unsigned long long links = __ballot(link);
        if (act) {
            const unsigned long long need = ((2ull << t) - 1ull) << (gi * T);    // links 0 .. t of this group
            const int valid = (links & need) == need;
            if (r < K) {
                md_vo_agent_item(&h, &ego, &o, r, t, j, valid);
                if (t == 0) md_vo_agent_meta(&s, &o, r, j);
            } else {
                md_vo_ego_item(&h, &ego, &o, t, j, valid);
            }
        }
    }
}

__device__ __forceinline__ void vo_route_block(const MdLane* lanes, const MdRoad* roads, const MdVectorObs& vo, const MdObsCtx& k,
                                               const MdVoEgo& ego, const MdVoOut& o, int lane, int my_road, int n_chain) {
    const int M = vo.route_points;
    int my_lane = 0;
    float my_len = 0.0f;
    if (lane < n_chain) {
        my_lane = md_vo_chain_lane(roads, my_road, k.rl->idx);
        my_len = lanes[my_lane].length;
    }
    float cum = 0.0f;
    if (n_chain > 0) cum = 0.0f - md_vo_chain_start(&lanes[bcast_i(my_lane, 0)], ego.cx, ego.cy);
    const float d = md_vo_waypoint_d(&vo, lane);
    int at = -1;
    float lng = 0.0f;
    for (int i = 0; i < n_chain; ++i) {       // serial, in the header's order: the sum is bit-exact
        const float next = cum + bcast_f(my_len, i);
        if (at < 0 && d <= next) {
            at = i;
            lng = d - cum;
        }
        cum = next;
    }
    const int at_lane = __shfl(my_lane, at < 0 ? 0 : at, 64);
    if (lane < M) md_vo_route_item(&o, lane, at >= 0 ? &lanes[at_lane] : nullptr, lng, &ego);
}

__device__ __forceinline__ void vo_lanes_block(const MdLane* lanes, int n_lanes, const MdVectorObs& vo, const MdObsCtx& k,
                                               const MdVoEgo& ego, const MdVoOut& o, int lane, int my_road, int n_chain, int* l_taken,
                                               float* l_dist) {
    const int P = vo.num_lanes, S = vo.lane_points;
    if (lane < MD_VO_MAX_LANES) l_taken[lane] = -1;
    if (k.valid)
        for (int l = lane; l < n_lanes; l += 64) l_dist[l] = md_vo_lane_dist(&lanes[l], ego.cx, ego.cy);
    wave_lds_sync();
    if (k.valid)
        for (int l = lane; l < n_lanes; l += 64) {
            const unsigned long long mine = vo_key(l_dist[l], l);
            int rank = 0;
            for (int q = 0; q < n_lanes && rank < P; ++q) rank += vo_key(l_dist[q], q) < mine;
            if (rank < P) l_taken[rank] = l;
        }
    wave_lds_sync();
    for (int it = lane; it < P * S; it += 64) {
        const int p = it / S, i = it - p * S;
        const int tl = l_taken[p];
        md_vo_lane_item(&o, S, p, i, tl >= 0 ? &lanes[tl] : nullptr, &ego);
    }
    const int tl = lane < P ? l_taken[lane] : -1;
    const int road = tl >= 0 ? lanes[tl].road : -2;
    int on_route = 0;
    for (int i = 0; i < n_chain; ++i) on_route |= bcast_i(my_road, i) == road;
    if (lane < P) md_vo_lane_meta(&o, lane, tl >= 0 ? &lanes[tl] : nullptr, on_route, tl >= 0 ? l_dist[tl] : 0.0f);
}

__global__ __launch_bounds__(64 * kVoWaves) void vector_obs_kernel(const MdWorld w, const MdState g, const MdConfig c, const MdVectorObs vo) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int e = blockIdx.x;                       // the grid is n_envs workgroups
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, n_waves = blockDim.x >> 6;
    const VectorObsLds LD = vector_obs_lds(w.max_lanes);
    unsigned char* base = smem + wave * LD.per_wave;
    int* l_sel = reinterpret_cast<int*>(base + LD.sel);
    int* l_taken = reinterpret_cast<int*>(base + LD.taken);
    float* l_dist = reinterpret_cast<float*>(base + LD.dist);
    const MdState s = md_env_view(&g, &c, e);
    const int clock = md_rd_clock(&g, &c, e, &s.nav[0]);
    const MdVoHist h = md_vo_hist_of(&vo, &c, e, clock);   // the cursor as the previous call left it, advanced in registers
    __syncthreads();                                       // ... by every wave, before it is rewritten
    for (int j = tid; j < c.cap; j += blockDim.x) md_vo_push_slot(&h, j, &s.shape[j]);
    if (tid == 0) md_vo_push_cursor(&h, clock);
    __threadfence_block();
    __syncthreads();                                       // the newest frame is in the ring for every wave of the env
    const int m = w.env_map[e];
    const MdLane* lanes = w.lanes + w.lane_off[m];
    const MdRoad* roads = w.roads + w.road_off[m];
    const int map_lanes = w.lane_off[m + 1] - w.lane_off[m];
    const int n_lanes = map_lanes < w.max_lanes ? map_lanes : w.max_lanes;     // l_dist holds max_lanes entries
    for (int item = wave; item < 3 * c.agents_per_env; item += n_waves) {   // wave-uniform
        const int a = item / 3, block = item - 3 * a;
        const MdVoOut o = md_vo_out_of(&vo, e, a);
        MdObsCtx k;
        md_observe_ctx(lanes, roads, &s, a, &k);
        const MdVoEgo ego = {s.shape[a].cx, s.shape[a].cy, s.shape[a].c, s.shape[a].s};
        if (block == 0) {
            vo_agents_block(s, c, vo, h, k, ego, o, a, lane, l_sel);
        } else if ((block == 1 && vo.route_points > 0) || (block == 2 && vo.num_lanes > 0)) {
            int n_chain;
            const int my_road = vo_chain_roads(s, k, a, lane, &n_chain);
            if (block == 1) vo_route_block(lanes, roads, vo, k, ego, o, lane, my_road, n_chain);
            else vo_lanes_block(lanes, n_lanes, vo, k, ego, o, lane, my_road, n_chain, l_taken, l_dist);
        }
        wave_lds_sync();                                   // the lists are reused by the wave's next item
    }
}

// "Others" block of the observation (Lidar.get_surrounding_vehicles_info): one thread per agent, after the
// step kernel has written the detected sets and the new state back.  Off in the headline configs.
__global__ __launch_bounds__(64) void others_kernel(MdWorld w, MdState g, MdConfig c) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= c.n_envs * c.agents_per_env) return;
    const int e = i / c.agents_per_env, a = i - e * c.agents_per_env;
    const MdState s = md_env_view(&g, &c, e);
    const int m = w.env_map[e];
    md_others_block(w.lanes + w.lane_off[m], w.roads + w.road_off[m], &s, &c, a, s.detected[2 * a], s.detected[2 * a + 1],
                    s.obs + (size_t)a * c.obs_dim + md_obs_others(&c));
}

// ----------------------------------------------------------------------------------------------------------------------------
// md_expert: the PPO expert (numpy_expert.py:34-77) over the batch.  One workgroup of 4 waves per tile of 16 envs:
//   1. x = the expert's 275-vector of each env in LDS (the env's obs row + the "others" block of md_others_block with
//      num_others = 4), corrected; rows past the last env stay zero and are never written out;
//   2. h1 = tanh(x W1 + b1), h2 = tanh(h1 W2 + b2): wave w owns the output columns [64w, 64w + 64) as four 16x16 tiles,
//      every tile ONE accumulator chained over the k-steps in order (A = 16 env rows from LDS, B = one 16-byte load per
//      lane per four k-steps from the packed weights, which stay in L2), bias as the accumulator's start value;
//   3. out = h2 W3 + b3 on wave 0 (one tile, N padded to 16), then mean / log_std / action.
// Each output element is the k-ordered fmaf chain of include/md_expert.h: v_mfma_f32_16x16x4_f32 rounds once per product
// in k order, and nothing else touches the accumulator.
constexpr int kExpM = 16;                                  // envs per workgroup (the MFMA's M)
constexpr int kExpXS = MD_EXPERT_IN_PAD + 4;               // LDS row strides: = 4 mod 32, so the 16 rows x 4 k of one
constexpr int kExpHS = MD_EXPERT_HID + 4;                  //   A-operand read spread over the banks
typedef float f32x4 __attribute__((ext_vector_type(4)));

// acc[j] (+)= A[16 rows][K] . W[K][tile nt0 + j], j < NT; A row r at a + r * lda, W packed (md_expert_widx)
template <int NT>
__device__ __forceinline__ void expert_tiles(const float* __restrict__ W, int K, int nt0, const float* a, int lda, int lane,
                                             f32x4* acc) {
    const int G = K >> 4;
    const float* arow = a + (lane & 15) * lda + (lane >> 4);
    const f32x4* wp[NT];
#pragma unroll
    for (int j = 0; j < NT; ++j) wp[j] = reinterpret_cast<const f32x4*>(W + (size_t)(nt0 + j) * G * 256) + lane;
    f32x4 cur[NT], nxt[NT];
#pragma unroll
    for (int j = 0; j < NT; ++j) cur[j] = wp[j][0];
    for (int g = 0; g < G; ++g) {
        if (g + 1 < G) {
#pragma unroll
            for (int j = 0; j < NT; ++j) nxt[j] = wp[j][(size_t)(g + 1) * 64];
        }
#pragma unroll
        for (int st = 0; st < 4; ++st) {
            const float av = arow[16 * g + 4 * st];
#pragma unroll
            for (int j = 0; j < NT; ++j) acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, cur[j][st], acc[j], 0, 0, 0);
        }
#pragma unroll
        for (int j = 0; j < NT; ++j) cur[j] = nxt[j];
    }
}

// one hidden layer: out[r][n] = tanh(in[r] . W[:, n] + b[n]) for the 64 columns of this wave
__device__ __forceinline__ void expert_hidden(const float* __restrict__ W, const float* __restrict__ b, int K, const float* in,
                                              int lds_in, float* out, int wave, int lane) {
    f32x4 acc[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const float bv = b[(4 * wave + j) * 16 + (lane & 15)];
        acc[j] = f32x4{bv, bv, bv, bv};
    }
    expert_tiles<4>(W, K, 4 * wave, in, lds_in, lane, acc);
    // C/D layout of the 16x16 MFMAs: column = lane & 15, row = (lane >> 4) * 4 + register
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r) out[((lane >> 4) * 4 + r) * kExpHS + (4 * wave + j) * 16 + (lane & 15)] = md_tanh(acc[j][r]);
}

// Stage 1 of md_expert for the tile of envs [e0, e0 + n_here): x from the env's obs row (state 19 | cloud 240) and the "others"
// block of md_others_block on the env's detected sets, corrected, in l_x [kExpM * kExpXS]; behind a barrier.
__device__ __forceinline__ void expert_fill_x(const MdWorld& w, const MdState& g, const MdConfig& c, float* l_x, int e0, int n_here) {
    const int tid = threadIdx.x;
    const int od = c.obs_dim;   // 259: state 19 | cloud 240
    for (int i = tid; i < kExpM * kExpXS; i += 256) {
        const int r = i / kExpXS, k = i - r * kExpXS;
        float v = 0.0f;
        if (r < n_here && k < MD_EXPERT_IN) {
            const float* o = g.obs + (size_t)(e0 + r) * od;
            if (k < MD_EXPERT_STATE) v = o[k];
            else if (k >= MD_EXPERT_STATE + 4 * MD_EXPERT_OTHERS) v = o[k - 4 * MD_EXPERT_OTHERS];
        }
        l_x[i] = v;
    }
    __syncthreads();
    if (tid < n_here) {
        MdConfig cc = c;                          // the expert's lidar: num_others = 4, no navigation dims of the others
        cc.num_others = MD_EXPERT_OTHERS;
        cc.add_others_navi = 0;
        const int e = e0 + tid;
        const MdState s = md_env_view(&g, &c, e);
        const int m = w.env_map[e];
        float* x = l_x + tid * kExpXS;
        md_others_block(w.lanes + w.lane_off[m], w.roads + w.road_off[m], &s, &cc, 0, s.detected[0], s.detected[1],
                        x + MD_EXPERT_STATE);
        md_expert_correct(x);
    }
    __syncthreads();
}

// Stages 2-3 for the tile of rows [row0, row0 + n_here) whose x stands in l_x (expert_fill_x, or md_expert_sense's own): obs_out rows,
// then the MLP; leaves mean | log_std of row r in l_out[r * MD_EXPERT_OUT ...], behind a barrier.
// l_x [kExpM * kExpXS] (x; later h2 at stride kExpHS), l_h [kExpM * kExpHS] (h1) and l_out are the calling kernel's LDS.
__device__ __forceinline__ void expert_tile_forward(const float* __restrict__ wts, float* __restrict__ obs_out, float* l_x, float* l_h,
                                                    float* l_out, int row0, int n_here) {
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    if (obs_out)
        for (int i = tid; i < n_here * MD_EXPERT_IN; i += 256) {
            const int r = i / MD_EXPERT_IN, k = i - r * MD_EXPERT_IN;
            obs_out[(size_t)row0 * MD_EXPERT_IN + i] = l_x[r * kExpXS + k];
        }
    // 2. hidden layers
    expert_hidden(wts + MD_EXPERT_W1, wts + MD_EXPERT_B1, MD_EXPERT_IN_PAD, l_x, kExpXS, l_h, wave, lane);
    __syncthreads();
    expert_hidden(wts + MD_EXPERT_W2, wts + MD_EXPERT_B2, MD_EXPERT_HID, l_h, kExpHS, l_x, wave, lane);
    __syncthreads();
    // 3. output layer (one 16x16 tile; columns 4..15 are zero padding)
    if (wave == 0) {
        const float bv = wts[MD_EXPERT_B3 + (lane & 15)];
        f32x4 acc[1] = {f32x4{bv, bv, bv, bv}};
        expert_tiles<1>(wts + MD_EXPERT_W3, MD_EXPERT_HID, 0, l_x, kExpHS, lane, acc);
        if ((lane & 15) < MD_EXPERT_OUT)
#pragma unroll
            for (int r = 0; r < 4; ++r) l_out[((lane >> 4) * 4 + r) * MD_EXPERT_OUT + (lane & 15)] = acc[0][r];
    }
    __syncthreads();
}

// The tile's results from l_out: mlp_out rows and the action (mean, or the draw with `noise`) of rows [row0, row0 + n_here).  Rows
// whose bit in `skip` is set (md_expert_sense: rows that were not sensed) get zeros.
__device__ __forceinline__ void expert_tile_emit(const float* l_out, const float* __restrict__ noise, float* __restrict__ action_out,
                                                 float* __restrict__ mlp_out, int row0, int n_here, unsigned skip) {
    const int tid = threadIdx.x;
    if (tid < n_here * MD_EXPERT_OUT) {
        const int r = tid >> 2, q = tid & 3;
        const size_t e = (size_t)(row0 + r);
        const bool off = ((skip >> r) & 1u) != 0u;
        if (mlp_out) mlp_out[e * MD_EXPERT_OUT + q] = off ? 0.0f : l_out[tid];
        if (q < 2) {
            const float mean = l_out[r * MD_EXPERT_OUT + q];
            const float act = noise ? md_expert_sample(mean, l_out[r * MD_EXPERT_OUT + 2 + q], noise[e * 2 + q]) : mean;
            action_out[e * 2 + q] = off ? 0.0f : act;
        }
    }
}

__global__ __launch_bounds__(256) void expert_kernel(MdWorld w, MdState g, MdConfig c, const float* __restrict__ wts,
                                                     const float* __restrict__ noise, float* __restrict__ action_out,
                                                     float* __restrict__ mlp_out, float* __restrict__ obs_out) {
    __shared__ __attribute__((aligned(16))) float l_x[kExpM * kExpXS];   // x; later h2 (stride kExpHS)
    __shared__ __attribute__((aligned(16))) float l_h[kExpM * kExpHS];   // h1
    __shared__ float l_out[kExpM * MD_EXPERT_OUT];
    const int tid = threadIdx.x;
    const int e0 = blockIdx.x * kExpM;
    const int n_here = min(kExpM, c.n_envs - e0);
    expert_fill_x(w, g, c, l_x, e0, n_here);
    expert_tile_forward(wts, obs_out, l_x, l_h, l_out, e0, n_here);
    expert_tile_emit(l_out, noise, action_out, mlp_out, e0, n_here, 0u);
}

// md_expert_sense (include/md_expert_sense.h): the expert observes for itself.  Tile of kExpM rows, row i = agent i % A of env i / A.
//   1. wave w, 16-lane group q: the state dims of row 4 w + q (md_observe_ctx, the six tasks the obs dims read on lanes of the group,
//      md_observe_state_dims on its lane 0) into the row in LDS;
//   2. the 16 rows x 4 sectors of the 240-beam cast by LDS ticket: lidar_item against the env's shape table, cloud straight into the
//      row, the detected set into the row's two LDS words;
//   3. behind a barrier, one thread per row: md_others_block on the row's own set, md_expert_correct;
//   4. expert_tile_forward / expert_tile_emit, as expert_kernel.
// The shape tables are read through L2, not staged: the 16 rows of a single-agent tile belong to 16 envs, and 16 tables of up to 128
// slots x 32 B (64 KB) cannot stand in LDS beside x and h1; a row's four sectors read the same 4 KB at most, which stays in L2 / the
// vector cache between them.  Static LDS: x 18.3 KB + h1 16.3 KB + 3 KB of task results + 0.6 KB = 38.3 KB at every capacity.
// Rows of an env with need_reset != 0 and rows past the last stay zero in LDS and are written out as zeros (expert_tile_emit).
__global__ __launch_bounds__(256) void expert_sense_kernel(MdWorld w, MdState g, MdConfig c, const float* __restrict__ wts,
                                                           const float* __restrict__ beam_cs240, const float* __restrict__ noise,
                                                           float* __restrict__ action_out, float* __restrict__ mlp_out,
                                                           float* __restrict__ obs_out) {
    __shared__ __attribute__((aligned(16))) float l_x[kExpM * kExpXS];
    __shared__ __attribute__((aligned(16))) float l_h[kExpM * kExpHS];
    __shared__ float l_out[kExpM * MD_EXPERT_OUT];
    __shared__ float l_task[kExpM * 48];                 // MD_OBS_TASKS * 5 (= 45) task results per row, padded
    __shared__ unsigned long long l_det[kExpM * 2];      // the rows' detected sets
    __shared__ int l_env[kExpM];                         // the row's env, -1 = not sensed
    __shared__ int l_tk;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int A = c.agents_per_env;
    const int rows = c.n_envs * A;
    const int row0 = blockIdx.x * kExpM;
    const int n_here = min(kExpM, rows - row0);
    // the expert's sensor config (numpy_expert.py:39-46) over the env's
    c.n_beams = MD_EXPERT_BEAMS;
    c.lidar_range = MD_EXPERT_RANGE;
    c.n_side = 0;
    c.n_lane_line = 0;
    c.random_agent_model = 0;
    c.num_others = MD_EXPERT_OTHERS;
    c.add_others_navi = 0;
    c.obs_dim = MD_EXPERT_IN;
    w.beam_cs = beam_cs240;
    for (int i = tid; i < kExpM * kExpXS; i += 256) l_x[i] = 0.0f;
    if (tid < kExpM) {
        int e = -1;
        if (tid < n_here) {
            e = (row0 + tid) / A;
            if (g.need_reset[e] != 0) e = -1;
        }
        l_env[tid] = e;
        l_det[2 * tid] = 0ull;
        l_det[2 * tid + 1] = 0ull;
    }
    if (tid == 0) l_tk = 0;
    __syncthreads();
    // the slices of env e that the sensors read (md_env_view without the arrays nothing here touches)
    auto view_of = [&](int e) {
        MdState s = g;
        const size_t b = (size_t)e * (size_t)c.cap;
        s.shape = g.shape + b;
        s.dyn = g.dyn + b;
        s.param = g.param + b;
        s.nav = g.nav + b;
        s.action = g.action + 2 * b;
        s.final_lane = g.final_lane + b;
        return s;
    };
    unsigned skip = 0u;
#pragma unroll
    for (int r = 0; r < kExpM; ++r) skip |= (l_env[r] < 0 ? 1u : 0u) << r;
    // 1. state dims
    {
        const int q = lane >> 4, sub = lane & 15;
        const int r = 4 * wave + q;
        const int e = l_env[r];
        float* scratch = l_task + r * 48;
        MdObsCtx k;
        MdState s = g;
        int a = 0;
        if (e >= 0) {
            a = row0 + r - e * A;
            s = view_of(e);
            const int m = w.env_map[e];
            md_observe_ctx(w.lanes + w.lane_off[m], w.roads + w.road_off[m], &s, a, &k);
            if (sub < 5 || sub == 8) {     // the tasks whose results the obs dims read
                float mine[5];
                md_observe_task(sub, &k, &s, &c, a, mine);
#pragma unroll
                for (int i = 0; i < 5; ++i) scratch[sub * 5 + i] = mine[i];
            }
        }
        wave_lds_sync();
        // a slot without a driving agent keeps its zeros
        if (e >= 0 && sub == 0 && k.valid) md_observe_state_dims(&k, &s, &c, a, (const float (*)[5])scratch, l_x + r * kExpXS);
    }
    // 2. cloud and detected sets
    constexpr int kSectors = (MD_EXPERT_BEAMS + 63) / 64;
    for (int guard = 0; guard < kExpM * kSectors; ++guard) {
        int it = 0;
        if (lane == 0) it = atomicAdd(&l_tk, 1);
        it = __builtin_amdgcn_readfirstlane(it);
        if (it < 0 || it >= kExpM * kSectors) break;
        const int r = it / kSectors, sec = it - r * kSectors;
        const int e = l_env[r];
        if (e < 0) continue;
        MdState s = g;
        s.shape = g.shape + (size_t)e * (size_t)c.cap;
        lidar_item<true>(w, s, c, row0 + r - e * A, sec, lane, l_x + r * kExpXS + MD_EXPERT_STATE + 4 * MD_EXPERT_OTHERS, l_det + 2 * r);
    }
    __syncthreads();
    // 3. others, correction: row r on lane 0 of its 16-lane group
    if ((tid & 15) == 0) {
        const int r = tid >> 4;
        const int e = l_env[r];
        if (e >= 0) {
            const MdState s = view_of(e);
            const int m = w.env_map[e];
            float* x = l_x + r * kExpXS;
            md_others_block(w.lanes + w.lane_off[m], w.roads + w.road_off[m], &s, &c, row0 + r - e * A, l_det[2 * r], l_det[2 * r + 1],
                            x + MD_EXPERT_STATE);
            md_expert_correct(x);
        }
    }
    __syncthreads();
    expert_tile_forward(wts, obs_out, l_x, l_h, l_out, row0, n_here);
    expert_tile_emit(l_out, noise, action_out, mlp_out, row0, n_here, skip);
}

// md_ai_protect: AIProtectPolicy (include/md_ai_protect.h) in one launch.  The expert's draw exactly as expert_kernel computes it (the
// same tile, the same chains), then the rule as an epilogue, one thread per env: obs[0], obs[1] and the four lidar windows come from
// the env's obs row in HBM (l_x holds h2 by now), speed / heading / lane from the env's state and the map tables.  No LDS beyond
// expert_kernel's.
__global__ __launch_bounds__(256) void ai_protect_kernel(MdWorld w, MdState g, MdConfig c, const float* __restrict__ wts,
                                                         const float* __restrict__ noise, const float* __restrict__ actions,
                                                         float save_level, unsigned char* __restrict__ takeover,
                                                         unsigned char* __restrict__ expert_takeover, float* __restrict__ applied_out,
                                                         unsigned char* __restrict__ flags_out, float* __restrict__ saver_out) {
    __shared__ __attribute__((aligned(16))) float l_x[kExpM * kExpXS];
    __shared__ __attribute__((aligned(16))) float l_h[kExpM * kExpHS];
    __shared__ float l_out[kExpM * MD_EXPERT_OUT];
    const int tid = threadIdx.x;
    const int e0 = blockIdx.x * kExpM;
    const int n_here = min(kExpM, c.n_envs - e0);
    expert_fill_x(w, g, c, l_x, e0, n_here);
    expert_tile_forward(wts, nullptr, l_x, l_h, l_out, e0, n_here);
    if (tid >= n_here) return;
    const int e = e0 + tid;
    const float* o4 = l_out + tid * MD_EXPERT_OUT;
    float sv[2];
#pragma unroll
    for (int q = 0; q < 2; ++q) sv[q] = noise ? md_expert_sample(o4[q], o4[2 + q], noise[(size_t)e * 2 + q]) : o4[q];
    if (saver_out) {
        saver_out[(size_t)e * 2] = sv[0];
        saver_out[(size_t)e * 2 + 1] = sv[1];
    }
    const float raw[2] = {actions[(size_t)e * 2], actions[(size_t)e * 2 + 1]};
    float applied[2];
    unsigned char tk = takeover[e], et = expert_takeover[e];
    unsigned fl;
    if (g.need_reset[e] != 0) {
        fl = md_ai_protect_reset(raw, &tk, &et, applied);
    } else {
        const MdState s = md_env_view(&g, &c, e);
        MdProtectIn in;
        md_ai_protect_inputs(w.lanes + w.lane_off[w.env_map[e]], &s, &c, &in);
        fl = md_ai_protect_act(raw, sv, &in, save_level, et != 0, &tk, applied);
    }
    takeover[e] = tk;
    expert_takeover[e] = et;
    applied_out[(size_t)e * 2] = applied[0];
    applied_out[(size_t)e * 2 + 1] = applied[1];
    flags_out[e] = (unsigned char)fl;
}

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

__global__ void probe_kernel(int op, const float* a, const float* b, float* out, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = md_probe_eval(op, a[i], b[i]);
}

// return from the calling entry point unless x is MD_OK
#define TRY(x)                       \
    do {                             \
        const int _r = (x);          \
        if (_r != MD_OK) return _r;  \
    } while (0)
#define NEED(p) TRY(need((const void*)(p), #p))

int check_struct_size(const MdConfig* c) {
    if (c->struct_size == (int32_t)sizeof(MdConfig)) return MD_OK;
    snprintf(g_err, sizeof g_err, "MdConfig.struct_size=%d, library expects %d", c->struct_size, (int)sizeof(MdConfig));
    return MD_EABI;
}

int check_common(const MdWorld* w, const MdState* s, const MdConfig* c) {
    if (!w || !s || !c) {
        snprintf(g_err, sizeof g_err, "null MdWorld/MdState/MdConfig pointer");
        return MD_EINVAL;
    }
    TRY(check_struct_size(c));
    if (c->n_envs <= 0 || c->cap <= 0 || c->cap > MD_MAX_CAP || c->agents_per_env <= 0 || c->agents_per_env > c->cap) {
        snprintf(g_err, sizeof g_err, "bad sizes: n_envs=%d cap=%d agents_per_env=%d (cap<=%d)", c->n_envs, c->cap,
                 c->agents_per_env, MD_MAX_CAP);
        return MD_EINVAL;
    }
    if (c->n_beams < 0 || c->n_beams > MD_MAX_BEAMS) {
        snprintf(g_err, sizeof g_err, "n_beams=%d out of range [0,%d]", c->n_beams, MD_MAX_BEAMS);
        return MD_EINVAL;
    }
    if (!s->shape) {
        snprintf(g_err, sizeof g_err, "MdState.shape is null");
        return MD_EINVAL;
    }
    if (w->n_envs != c->n_envs) {
        snprintf(g_err, sizeof g_err, "MdWorld.n_envs=%d != MdConfig.n_envs=%d", w->n_envs, c->n_envs);
        return MD_EINVAL;
    }
    return MD_OK;
}

int need(const void* p, const char* name) {
    if (p) return MD_OK;
    snprintf(g_err, sizeof g_err, "required pointer %s is null", name);
    return MD_EINVAL;
}

// ---- the MdWorld / MdState pointers each entry point requires ----
// A row: the entry points that require its fields (their PH_* bits: PH_RESET is md_step's alone; the k*Entry bits stand for
// the entry points that run no phase), the condition under which they do, and the fields.  An entry point checks the rows of
// a few conditions at a time (need_fields), each group where its code has validated what the condition reads; within a
// group, table order is check order, so the first null field is the one the message names.
enum When : unsigned {
    ALWAYS = 1, LIDAR_ON = 2, MULTI = 4, RESPAWN = 8,   // check_phase, before anything but check_common
    REPLAY = 16, SPAWN_TRAFFIC = 32,                     // check_phase, after traffic_mode is validated
    SCENARIO = 64, ROUTE = 128, OTHERS = 256,            // md_step, each after the config checks of its branch
};
constexpr int kLidarEntry = 1 << 9, kDetectorEntry = 1 << 10, kExpertEntry = 1 << 11, kPgWalkEntry = 1 << 12, kProtectEntry = 1 << 13,
              kSenseEntry = 1 << 14, kTopDownEntry = 1 << 15, kRenderEntry = 1 << 16, kPedEntry = 1 << 17, kVectorObsEntry = 1 << 18;
constexpr int kMapPhases = PH_LOCALIZE | PH_CONTACTS | PH_OBSERVE | PH_IDM | PH_LIFECYCLE;
constexpr int kTrafficPhases = PH_INTEGRATE | PH_TRAFFIC;

struct Field { const char* name; bool world; size_t off; };   // "w->x" / "s->x" as the message spells it, MdWorld?, offset
#define FW(f) Field{"w->" #f, true, offsetof(MdWorld, f)}
#define FS(f) Field{"s->" #f, false, offsetof(MdState, f)}
#define MAP_FIELDS FW(env_map), FW(lane_off), FW(lanes), FW(hull_xy), FW(road_off), FW(roads), FW(quad_off), FW(quads), \
                   FW(quad_kind), FW(grid), FW(cell_start), FW(cell_items)
struct Need { int entries; When when; Field fields[12]; };   // fields: up to 12, the unused tail has name == nullptr
const Need kNeeds[] = {
    {PH_ALL, ALWAYS, {FS(dyn), FS(param), FS(nav), FS(pid), FS(action), FS(flags), FS(route_nodes), FS(route_roads), FS(need_reset)}},
    {kMapPhases, ALWAYS, {MAP_FIELDS}},
    {PH_OBSERVE, ALWAYS, {FS(final_lane)}},
    {PH_IDM, ALWAYS, {FS(idm_rand)}},
    {PH_OBSERVE, ALWAYS, {FS(obs), FS(reward), FS(cost), FS(step_info)}},
    {PH_IDM, ALWAYS, {FW(node_adj_off), FW(node_adj), FW(node_off)}},
    {PH_RESET, LIDAR_ON, {FW(beam_cs)}},
    {PH_RESET, ALWAYS, {FS(shape0), FS(dyn0), FS(nav0), FS(pid0)}},
    {PH_LIFECYCLE, MULTI, {FS(rng), FS(env_steps), FS(agent_id), FS(next_agent_id), FS(route_nodes0), FS(route_roads0), FS(final_lane0),
                           FS(final_lane)}},
    {PH_LIFECYCLE, RESPAWN, {FW(spawn_off), FW(spawn_place), FW(spawn_lane), FW(spawn_route), FW(spawn_route_meta)}},
    {kTrafficPhases, REPLAY, {FS(track_shape), FS(track_dyn)}},
    {kTrafficPhases, SPAWN_TRAFFIC, {MAP_FIELDS}},
    {kTrafficPhases, SPAWN_TRAFFIC, {FS(rng), FS(route_nodes0), FS(route_roads0), FS(final_lane0), FS(final_lane), FW(spawn_off),
                                     FW(spawn_lane), FW(spawn_route), FW(spawn_route_meta)}},
    {PH_RESET, SCENARIO, {FW(poly_off), FW(segs), FW(polyv_off), FW(polyv), FW(ckpt_off), FW(ckpt_xy), FW(track_meta), FS(track_shape),
                          FS(track_dyn), FS(next_agent_id)}},
    {PH_RESET, ROUTE, {FS(route_segs), FS(route_verts), FS(route_aux), FW(run_off), FW(runs)}},
    {PH_RESET, OTHERS, {FS(detected)}},
    {kLidarEntry, ALWAYS, {FW(beam_cs)}},
    {kDetectorEntry, ALWAYS, {FW(env_map), FW(quad_off), FW(quads), FW(quad_kind)}},
    {kExpertEntry, ALWAYS, {FS(obs), FS(detected), FS(dyn), FS(param), FS(nav), FW(env_map), FW(lanes), FW(lane_off), FW(roads),
                            FW(road_off)}},
    {kProtectEntry, ALWAYS, {FS(shape), FS(need_reset)}},
    {kSenseEntry, ALWAYS, {FS(dyn), FS(param), FS(nav), FS(action), FS(final_lane), FS(need_reset), FW(env_map), FW(lanes), FW(lane_off),
                           FW(roads), FW(road_off)}},
    {kTopDownEntry, ALWAYS, {FS(nav), FS(route_roads), FW(env_map), FW(lane_off), FW(lanes), FW(road_off), FW(roads), FW(quad_off), FW(quads),
                             FW(quad_kind)}},
    {kRenderEntry, ALWAYS, {FS(nav), FW(env_map), FW(quad_off), FW(quads), FW(quad_kind)}},
    {kRenderEntry, MULTI, {FS(env_steps)}},
    {kPgWalkEntry, ALWAYS, {FS(scene_of), FS(walk_ep), FS(param), FS(route_nodes), FS(route_roads), FS(final_lane), FS(idm_rand)}},
    {kPgWalkEntry, SPAWN_TRAFFIC, {FS(rng), FS(route_nodes0), FS(route_roads0), FS(final_lane0)}},
    {kPedEntry, ALWAYS, {FS(shape), FS(dyn), FS(nav), FS(pid), FS(idm_rand), FS(need_reset)}},
    {kVectorObsEntry, ALWAYS, {FS(shape), FS(dyn), FS(nav), FS(route_roads), FS(final_lane), FW(env_map), FW(lane_off), FW(lanes),
                               FW(road_off), FW(roads)}},
    {kVectorObsEntry, MULTI, {FS(env_steps)}},
};
#undef FW
#undef FS
#undef MAP_FIELDS

bool holds(When when, const MdState* s, const MdConfig* c) {
    switch (when) {
    case ALWAYS: return true;
    case LIDAR_ON: return c->n_beams > 0;
    case MULTI: return c->is_multi_agent;
    case RESPAWN: return c->is_multi_agent && c->allow_respawn;
    case REPLAY: return c->traffic_mode == 3;
    case SPAWN_TRAFFIC: return c->traffic_mode == 1 || c->traffic_mode == 2;   // respawn / hybrid
    case SCENARIO: return c->traffic_mode == 4;
    case ROUTE: return c->traffic_mode == 4 && s->route_n;
    case OTHERS: return c->num_others > 0;
    }
    return false;
}

// MD_OK, or MD_EINVAL naming the first null field that `entry` requires under the conditions `whens`
int need_fields(int entry, unsigned whens, const MdWorld* w, const MdState* s, const MdConfig* c) {
    for (const Need& n : kNeeds) {
        if (!(n.entries & entry) || !(n.when & whens) || !holds(n.when, s, c)) continue;
        for (const Field& f : n.fields) {
            if (f.name && !*(void* const*)((const char*)(f.world ? (const void*)w : (const void*)s) + f.off)) return need(nullptr, f.name);
        }
    }
    return MD_OK;
}

// what the eight phase entry points check before they launch (md_step goes on checking)
int check_phase(int ph, const MdWorld* w, const MdState* s, const MdConfig* c) {
    TRY(check_common(w, s, c));
    TRY(need_fields(ph, ALWAYS | LIDAR_ON | MULTI | RESPAWN, w, s, c));
    if ((ph & PH_LIFECYCLE) && c->is_multi_agent && c->allow_respawn && w->n_dest <= 0) {
        snprintf(g_err, sizeof g_err, "multi-agent respawn needs MdWorld.n_dest > 0");
        return MD_EINVAL;
    }
    // traffic_mode 4 (scenario) is validated by md_step itself
    const int tm = c->traffic_mode;
    if ((ph & kTrafficPhases) && tm != 0 && tm != 4 && (tm < 0 || tm > 3 || c->is_multi_agent)) {
        snprintf(g_err, sizeof g_err, "traffic_mode=%d is not valid here (0 trigger, 1 respawn, 2 hybrid, 3 replay; "
                 "single-agent envs)", tm);
        return MD_EINVAL;
    }
    TRY(need_fields(ph, REPLAY | SPAWN_TRAFFIC, w, s, c));
    if ((ph & kTrafficPhases) && tm == 3 && c->track_len <= 0) {
        snprintf(g_err, sizeof g_err, "traffic_mode 3 (replay) needs MdConfig.track_len > 0");
        return MD_EINVAL;
    }
    if (ph == PH_OBSERVE && c->obs_dim < md_obs_lidar(c)) {
        snprintf(g_err, sizeof g_err, "obs_dim=%d < %d", c->obs_dim, md_obs_lidar(c));
        return MD_EINVAL;
    }
    return MD_OK;
}

// after a hipLaunchKernelGGL: MD_OK, or MD_ELAUNCH with the HIP error in g_err
int launch_status() {
    const hipError_t err = hipGetLastError();
    if (err == hipSuccess) return MD_OK;
    snprintf(g_err, sizeof g_err, "kernel launch failed: %s", hipGetErrorString(err));
    return MD_ELAUNCH;
}

// The kernel a phase launches.  md_step of the single-agent envs has two: env_kernel (one 4-wave workgroup per env) and
// wave_step_kernel (one wave per env), chosen by MdConfig.step_kernel alone (0 = workgroup, 1 = wave): the host decides -- it
// knows how many distinct maps the batch shares, which is what tips the balance (metadrive_ped_amd/engine.py) -- and the
// library reads no environment variable.  The wave kernel is wave_step_kernel<respawn>; the workgroup kernel is
// env_kernel<PH, stage, respawn, multi>, or <PH_ALL, stage, false, true, 512> when wide.
struct Variant {
    bool wave, stage, respawn, multi, wide;
};

template <int PH>
Variant variant(const MdWorld* w, const MdState* s, const MdConfig* c) {
    Variant v;
    v.wave = PH == PH_ALL && !c->is_multi_agent && c->step_kernel == 1;
    v.stage = w->max_lanes <= kStageMaxLanes;
    v.multi = (PH & (PH_LIFECYCLE | PH_RESET)) && c->is_multi_agent;
    // agent_idm != 0: IDMPolicy and LaneChangePolicy agents are driven by code that only this variant (and MULTI) carries
    // md_step (PH_ALL): whatever breaks one of the lean pins (lean_pins: the list the lean kernels fold) -- so does num_others > 0,
    // which md_step accepts with the detected sets only.  The phase entry points track no detected sets.
    v.respawn = !v.multi && (PH & (PH_TRAFFIC | PH_RESET | PH_INTEGRATE)) &&
                (PH == PH_ALL ? !lean_pins_hold(*s, *c) : (c->traffic_mode != 0 || c->agent_idm != 0));
    // Multi-agent md_step: eight waves per env while every workgroup of the batch is resident at once at that size (the MULTI
    // kernel's 92 VGPRs allow 5 waves per SIMD = 640 eight-wave workgroups on the 256 CUs); larger batches keep four, which
    // then fill the chip by themselves.  Measured: 512 tollgate envs x 40 agents, 1024 roundabout envs (profiles/r03_*).
    v.wide = PH == PH_ALL && v.multi && c->n_envs <= kWideMaxEnvs && MD_ENV_BLOCK == 256 && c->agents_per_env > 8;
    return v;
}

template <int PH, bool RESPAWN, bool MULTI, int BLK = MD_ENV_BLOCK>
void launch_env(bool stage, size_t lds, hipStream_t st, const MdWorld* w, const MdState* s, const MdConfig* c, float* lidar_out,
                int stride, int offset) {
    if (stage) hipLaunchKernelGGL((env_kernel<PH, true, RESPAWN, MULTI, BLK>), dim3(c->n_envs), dim3(BLK), lds, st, *w, *s, *c, lidar_out, stride, offset);
    else hipLaunchKernelGGL((env_kernel<PH, false, RESPAWN, MULTI, BLK>), dim3(c->n_envs), dim3(BLK), lds, st, *w, *s, *c, lidar_out, stride, offset);
}

template <int PH>
int launch(const MdWorld* w, const MdState* s, const MdConfig* c, float* lidar_out, int stride, int offset, void* stream) {
    const Variant v = variant<PH>(w, s, c);
    const hipStream_t st = (hipStream_t)stream;
    if (v.wave) {
        const size_t per_env = wave_env_lds(c->cap, c->agents_per_env).bytes;
        int per_wg = kWaveEnvs;   // envs per workgroup: as many as fit 64 KB of LDS (capacity-128 accident scenes: 2)
        while (per_wg > 1 && per_wg * per_env > 64 * 1024) per_wg >>= 1;
        const size_t lds = per_wg * per_env;
        if (lds > 64 * 1024) {
            snprintf(g_err, sizeof g_err, "LDS image of one env needs %zu B (cap=%d); limit 65536", lds, c->cap);
            return MD_EINVAL;
        }
        const dim3 grid((c->n_envs + per_wg - 1) / per_wg), block(64 * per_wg);
        if (v.respawn) hipLaunchKernelGGL((wave_step_kernel<true>), grid, block, lds, st, *w, *s, *c, lidar_out, stride, offset);
        else hipLaunchKernelGGL((wave_step_kernel<false>), grid, block, lds, st, *w, *s, *c, lidar_out, stride, offset);
        return launch_status();
    }
    const size_t lds = env_lds(c->cap, c->agents_per_env, v.stage ? w->max_lanes : 0, v.stage ? w->max_roads : 0,
                               (v.wide ? 512 : MD_ENV_BLOCK) / 64, v.multi, PH == PH_LIDAR).bytes;
    if (lds > 64 * 1024 || ((PH != PH_LIDAR) && (w->max_lanes <= 0 || w->max_roads <= 0))) {
        snprintf(g_err, sizeof g_err, "LDS image of one env needs %zu B (cap=%d, max_lanes=%d, max_roads=%d); limit 65536",
                 lds, c->cap, w->max_lanes, w->max_roads);
        return MD_EINVAL;
    }
    // the instantiations: PH_ALL all four; the phases that can be multi-agent or respawn two; the others one (per stage)
    constexpr bool kAll = PH == PH_ALL, kMulti = (PH & (PH_LIFECYCLE | PH_RESET)) != 0;
    constexpr bool kRespawn = (PH & (PH_TRAFFIC | PH_RESET | PH_INTEGRATE)) != 0;
    if (v.wide) launch_env<PH, false, kAll, kAll ? 512 : MD_ENV_BLOCK>(v.stage, lds, st, w, s, c, lidar_out, stride, offset);
    else if (v.multi) launch_env<PH, false, kMulti>(v.stage, lds, st, w, s, c, lidar_out, stride, offset);
    else if (v.respawn) launch_env<PH, kRespawn, false>(v.stage, lds, st, w, s, c, lidar_out, stride, offset);
    else launch_env<PH, false, false>(v.stage, lds, st, w, s, c, lidar_out, stride, offset);
    return launch_status();
}

}  // namespace

extern "C" {

__attribute__((visibility("default"))) int md_abi(int32_t* sizes, int n) {
    const int32_t v[11] = {sizeof(MdShape), sizeof(MdDyn), sizeof(MdParam), sizeof(MdNav), sizeof(MdPid), sizeof(MdLane),
                           sizeof(MdRoad), sizeof(MdGrid), sizeof(MdWorld), sizeof(MdState), sizeof(MdConfig)};
    for (int i = 0; sizes && i < n && i < 11; ++i) sizes[i] = v[i];
    return MD_ABI_VERSION;
}

__attribute__((visibility("default"))) const char* md_last_error(void) { return g_err; }

#ifdef MD_STAMP
// diagnostic build only: buffer of n_envs * 16 uint64 device words, or NULL to stop stamping
__attribute__((visibility("default"))) int md_debug_set_stamp_buffer(void* dev_ptr) {
    unsigned long long* p = (unsigned long long*)dev_ptr;
    return hipMemcpyToSymbol(HIP_SYMBOL(g_stamp_buf), &p, sizeof(p)) == hipSuccess ? MD_OK : MD_ELAUNCH;
}
// diagnostic build only: a permutation of the envs (workgroup b steps env order[b]), or NULL
__attribute__((visibility("default"))) int md_debug_set_env_order(const void* dev_ptr) {
    const int* p = (const int*)dev_ptr;
    return hipMemcpyToSymbol(HIP_SYMBOL(g_env_order), &p, sizeof(p)) == hipSuccess ? MD_OK : MD_ELAUNCH;
}
#endif

// 4 x 16 B per thread in flight (loads issued before the stores), non-temporal both ways, 2048 workgroups
// striding over 16 KB tiles: the usual shape of a bandwidth probe on this part.
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
__global__ __launch_bounds__(256) void stream_copy_kernel(u32x4* __restrict__ dst, const u32x4* __restrict__ src, size_t n16) {
    constexpr int U = 4;
    const size_t tile = (size_t)256 * U;
    const size_t n_tiles = n16 / tile;
    for (size_t t = blockIdx.x; t < n_tiles; t += gridDim.x) {
        const size_t base = t * tile + threadIdx.x;
        u32x4 v[U];
#pragma unroll
        for (int u = 0; u < U; ++u) v[u] = __builtin_nontemporal_load(&src[base + (size_t)u * 256]);
#pragma unroll
        for (int u = 0; u < U; ++u) __builtin_nontemporal_store(v[u], &dst[base + (size_t)u * 256]);
    }
    // tail (< one tile): first workgroup
    if (blockIdx.x == 0)
        for (size_t i = n_tiles * tile + threadIdx.x; i < n16; i += 256) dst[i] = src[i];
}

__attribute__((visibility("default"))) int md_probe_stream_copy(void* dst, const void* src, size_t nbytes, void* stream) {
    if (!dst || !src || nbytes == 0 || (nbytes & 15) || ((uintptr_t)dst & 15) || ((uintptr_t)src & 15)) {
        snprintf(g_err, sizeof g_err, "md_probe_stream_copy: null / unaligned pointer or size not a multiple of 16");
        return MD_EINVAL;
    }
    const size_t n16 = nbytes >> 4;
    size_t blocks = (n16 + 1023) / 1024;
    if (blocks > 2048u) blocks = 2048u;  // 8 workgroups per CU, tile-stride beyond
    hipLaunchKernelGGL(stream_copy_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, (u32x4*)dst,
                       (const u32x4*)src, n16);
    return launch_status();
}

__attribute__((visibility("default"))) int md_probe_math(int op, const float* a, const float* b, float* out, int n,
                                                        void* stream) {
    if (!a || !b || !out || n <= 0) {
        snprintf(g_err, sizeof g_err, "md_probe_math: null pointer or n<=0");
        return MD_EINVAL;
    }
    hipLaunchKernelGGL(probe_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, op, a, b, out, n);
    return launch_status();
}

__attribute__((visibility("default"))) int md_lidar(const MdWorld* w, const MdState* s, const MdConfig* c, float* out,
                                                   int out_stride, int out_offset, void* stream) {
    TRY(check_common(w, s, c));
    NEED(out);
    TRY(need_fields(kLidarEntry, ALWAYS, w, s, c));
    if (c->n_beams <= 0 || out_stride < c->n_beams + out_offset || out_offset < 0) {
        snprintf(g_err, sizeof g_err, "md_lidar: n_beams=%d stride=%d offset=%d", c->n_beams, out_stride, out_offset);
        return MD_EINVAL;
    }
    return launch<PH_LIDAR>(w, s, c, out, out_stride, out_offset, stream);
}

__attribute__((visibility("default"))) int md_lidar_detect(const MdWorld* w, const MdState* s, const MdConfig* c, float* out,
                                                          int out_stride, int out_offset, uint64_t* detected, void* stream) {
    TRY(check_common(w, s, c));
    NEED(out); NEED(detected);
    TRY(need_fields(kLidarEntry, ALWAYS, w, s, c));
    if (c->n_beams <= 0 || out_stride < c->n_beams + out_offset || out_offset < 0) {
        snprintf(g_err, sizeof g_err, "md_lidar_detect: n_beams=%d stride=%d offset=%d", c->n_beams, out_stride, out_offset);
        return MD_EINVAL;
    }
    hipLaunchKernelGGL(lidar_detect_kernel, dim3(c->n_envs), dim3(256), lidar_detect_lds(c->cap, c->agents_per_env).bytes, (hipStream_t)stream, *w, *s, *c, out, out_stride,
                       out_offset, (unsigned long long*)detected);
    return launch_status();
}

static int line_detector_launch(const MdWorld* w, const MdState* s, const MdConfig* c, const float* beam_cs, int n_beams, float range,
                                uint32_t kind_mask, int out_offset, const float* beam_cs1, int n_beams1, float range1, uint32_t kind_mask1,
                                int out_offset1, float* out, int out_stride, void* stream, const char* who) {
    TRY(check_common(w, s, c));
    NEED(out); NEED(beam_cs);
    TRY(need_fields(kDetectorEntry, ALWAYS, w, s, c));
    if (n_beams <= 0 || n_beams > MD_MAX_BEAMS || out_stride < n_beams + out_offset || out_offset < 0 || !(range > 0.0f) ||
        (n_beams1 > 0 && (!beam_cs1 || out_stride < n_beams1 + out_offset1 || out_offset1 < 0 || !(range1 > 0.0f)))) {
        snprintf(g_err, sizeof g_err, "%s: n_beams=%d/%d stride=%d offset=%d/%d range=%f/%f", who, n_beams, n_beams1, out_stride, out_offset,
                 out_offset1, (double)range, (double)range1);
        return MD_EINVAL;
    }
    const size_t nb = (size_t)n_beams + (size_t)(n_beams1 > 0 ? n_beams1 : 0);
    if (nb > 255) {   // a (quad, beam) pair keeps the beam in eight bits
        snprintf(g_err, sizeof g_err, "%s: %zu beams > 255", who, nb);
        return MD_EINVAL;
    }
    hipLaunchKernelGGL(line_detector_kernel, dim3(c->n_envs * detector_groups(c->agents_per_env)), dim3(kBlock), line_detector_lds((int)nb).bytes, (hipStream_t)stream, *w, *s, *c, beam_cs,
                       n_beams, range, kind_mask, out, out_stride, out_offset, beam_cs1, n_beams1 > 0 ? n_beams1 : 0, range1, kind_mask1, out_offset1);
    return launch_status();
}

__attribute__((visibility("default"))) int md_line_detector(const MdWorld* w, const MdState* s, const MdConfig* c,
                                                           const float* beam_cs, int n_beams, float range,
                                                           uint32_t kind_mask, float* out, int out_stride,
                                                           int out_offset, void* stream) {
    return line_detector_launch(w, s, c, beam_cs, n_beams, range, kind_mask, out_offset, nullptr, 0, 0.0f, 0u, 0, out, out_stride, stream,
                                "md_line_detector");
}

// Two detector fans (the side detector and the lane-line detector of one observation) in ONE launch and one pass over the map's
// line pieces: what SideDetector.perceive + LaneLineDetector.perceive cost twice (obs/state_obs.py:77-86,129-140).
__attribute__((visibility("default"))) int md_swap_draw(const MdState* s, const MdState* staged, const MdConfig* c, int n_draws,
                                                        int32_t* draw_idx, void* stream) {
    if (!s || !staged || !c || !draw_idx) {
        snprintf(g_err, sizeof g_err, "md_swap_draw: null MdState / staged MdState / MdConfig / draw_idx");
        return MD_EINVAL;
    }
    TRY(check_struct_size(c));
    if (n_draws < 1 || c->n_envs <= 0 || c->cap <= 0 || c->cap > MD_MAX_CAP) {
        snprintf(g_err, sizeof g_err, "md_swap_draw: n_draws=%d n_envs=%d cap=%d", n_draws, c->n_envs, c->cap);
        return MD_EINVAL;
    }
    if (!s->need_reset || !s->shape0 || !s->dyn0 || !s->nav0 || !s->pid0 || !staged->shape0 || !staged->dyn0 || !staged->nav0 || !staged->pid0) {
        snprintf(g_err, sizeof g_err, "md_swap_draw: need_reset and the snapshot arrays shape0 / dyn0 / nav0 / pid0 (live and staged) are required");
        return MD_EINVAL;
    }
    const MdWalk& wk = s->walk;
    if (wk.mode != 0 && c->traffic_mode >= 0 && c->traffic_mode <= 2) {   // the PG walk: n_draws PG scenes, draw_idx = MdWorld.env_map
        if (wk.mode < 0 || wk.mode > 2 || c->is_multi_agent || c->agents_per_env != 1 || wk.n_scenes != n_draws || wk.stride < 1 ||
            wk.offset < 0) {
            snprintf(g_err, sizeof g_err, "md_swap_draw: the PG walk needs mode 1 or 2 (got %d), a single-agent batch (agents=%d), "
                     "n_scenes == n_draws (%d, %d), stride >= 1 (%d) and offset >= 0 (%d)", wk.mode, c->agents_per_env, wk.n_scenes,
                     n_draws, wk.stride, wk.offset);
            return MD_EINVAL;
        }
        // the live batch and the pool hold the same per-slot constants: what the in-kernel reset of the next step reads
        TRY(need_fields(kPgWalkEntry, ALWAYS | SPAWN_TRAFFIC, nullptr, s, c));
        const bool spawn = c->traffic_mode == 1 || c->traffic_mode == 2;
        if (!staged->param || !staged->route_nodes || !staged->route_roads || !staged->final_lane || !staged->idm_rand ||
            (spawn && !staged->rng)) {
            snprintf(g_err, sizeof g_err, "md_swap_draw: the PG walk's pool (staged) needs param / route_nodes / route_roads / "
                     "final_lane / idm_rand, and rng in the respawn / hybrid modes");
            return MD_EINVAL;
        }
    } else if (wk.mode != 0) {   // the scenario walk: n_draws scenes, draw_idx = MdWorld.env_map
        if (wk.mode < 0 || wk.mode > 2 || c->traffic_mode != 4 || wk.n_scenes != n_draws || wk.stride < 1 || wk.offset < 0 ||
            !s->scene_of || !s->walk_ep) {
            snprintf(g_err, sizeof g_err, "md_swap_draw: the scenario walk needs mode 1 or 2 (got %d), traffic_mode 4, n_scenes == "
                     "n_draws (%d, %d), stride >= 1 (%d), offset >= 0 (%d) and MdState.scene_of / walk_ep", wk.mode, wk.n_scenes,
                     n_draws, wk.stride, wk.offset);
            return MD_EINVAL;
        }
    }
    hipLaunchKernelGGL(swap_draw_kernel, dim3(c->n_envs), dim3(256), 0, (hipStream_t)stream, *s, *staged, *c, n_draws, draw_idx);
    return launch_status();
}

// include/md_curriculum.h
__attribute__((visibility("default"))) int md_curriculum(const MdState* s, const MdState* staged, const MdConfig* c,
                                                         const MdCurriculum* cu, int32_t* env_map, int reset, void* stream) {
    if (!s || !staged || !c || !cu || !env_map) {
        snprintf(g_err, sizeof g_err, "md_curriculum: null MdState / staged MdState / MdConfig / MdCurriculum / env_map");
        return MD_EINVAL;
    }
    TRY(check_struct_size(c));
    if (c->n_envs <= 0 || c->cap <= 0 || c->cap > MD_MAX_CAP || c->agents_per_env != 1 || c->traffic_mode != 4) {
        snprintf(g_err, sizeof g_err, "md_curriculum: a single-agent scenario batch is required (n_envs=%d cap=%d agents=%d "
                 "traffic_mode=%d)", c->n_envs, c->cap, c->agents_per_env, c->traffic_mode);
        return MD_EINVAL;
    }
    const MdWalk& wk = s->walk;
    if (wk.mode == 0 || wk.n_scenes != cu->n_scenes || wk.stride != cu->stride || wk.offset != cu->offset || !s->scene_of ||
        !s->walk_ep || !s->need_reset || !s->flags || !s->step_info) {
        snprintf(g_err, sizeof g_err, "md_curriculum: needs the scenario walk (MdState.walk mode %d, n_scenes %d / %d, stride %d / %d, "
                 "offset %d / %d), MdState.scene_of / walk_ep / need_reset / flags / step_info", wk.mode, wk.n_scenes, cu->n_scenes,
                 wk.stride, cu->stride, wk.offset, cu->offset);
        return MD_EINVAL;
    }
    if (cu->n_levels < 1 || cu->n_scenes < 1 || cu->per_level * cu->n_levels != cu->n_scenes || cu->eval < 1 || cu->stride < 1 ||
        cu->offset < 0 || cu->cover_words != (cu->n_scenes + 31) / 32 || (cu->n_levels > 1 && wk.mode != 1)) {
        snprintf(g_err, sizeof g_err, "md_curriculum: n_levels=%d per_level=%d n_scenes=%d eval=%d stride=%d offset=%d cover_words=%d "
                 "walk mode %d (levels > 1 need the sequential walk)", cu->n_levels, cu->per_level, cu->n_scenes, cu->eval, cu->stride,
                 cu->offset, cu->cover_words, wk.mode);
        return MD_EINVAL;
    }
    if (!cu->level || !cu->seed || !cu->q_len || !cu->q_key || !cu->q_success || !cu->q_route || !cu->cover || !cu->cover_n ||
        !cu->rep_i || !cu->rep_f) {
        snprintf(g_err, sizeof g_err, "md_curriculum: every MdCurriculum array is required");
        return MD_EINVAL;
    }
    if (cu->n_levels > 1 && (!s->shape0 || !s->dyn0 || !s->nav0 || !s->pid0 || !staged->shape0 || !staged->dyn0 || !staged->nav0 ||
                             !staged->pid0)) {
        snprintf(g_err, sizeof g_err, "md_curriculum: the snapshot arrays shape0 / dyn0 / nav0 / pid0 (live and staged) are required");
        return MD_EINVAL;
    }
    hipLaunchKernelGGL(curriculum_kernel, dim3(c->n_envs), dim3(64), 0, (hipStream_t)stream, *s, *staged, *c, *cu, env_map, reset);
    return launch_status();
}

__attribute__((visibility("default"))) int md_line_detectors(const MdWorld* w, const MdState* s, const MdConfig* c,
                                                            const float* beam_cs0, int n_beams0, float range0, uint32_t kind_mask0,
                                                            int out_offset0, const float* beam_cs1, int n_beams1, float range1,
                                                            uint32_t kind_mask1, int out_offset1, float* out, int out_stride,
                                                            void* stream) {
    return line_detector_launch(w, s, c, beam_cs0, n_beams0, range0, kind_mask0, out_offset0, beam_cs1, n_beams1, range1, kind_mask1,
                                out_offset1, out, out_stride, stream, "md_line_detectors");
}

// the eight phase entry points: check_phase, then launch<PH>
#define MD_PHASE_ENTRY(name, PH)                                                                                          \
    __attribute__((visibility("default"))) int name(const MdWorld* w, const MdState* s, const MdConfig* c, void* stream) { \
        TRY(check_phase(PH, w, s, c));                                                                                    \
        return launch<PH>(w, s, c, nullptr, 0, 0, stream);                                                                \
    }
MD_PHASE_ENTRY(md_integrate, PH_INTEGRATE)
MD_PHASE_ENTRY(md_localize, PH_LOCALIZE)
MD_PHASE_ENTRY(md_contacts, PH_CONTACTS)
MD_PHASE_ENTRY(md_observe, PH_OBSERVE)
MD_PHASE_ENTRY(md_idm, PH_IDM)
MD_PHASE_ENTRY(md_traffic_after_step, PH_TRAFFIC)
MD_PHASE_ENTRY(md_lifecycle, PH_LIFECYCLE)
#undef MD_PHASE_ENTRY

// md_localize through the road-first path (the lean md_step's localisation on its own): for the parity tests, declared in no header
__attribute__((visibility("default"))) int md_localize_road_first(const MdWorld* w, const MdState* s, const MdConfig* c, void* stream) {
    TRY(check_phase(PH_LOCALIZE, w, s, c));
    return launch<PH_LOCALIZE_ROAD_FIRST>(w, s, c, nullptr, 0, 0, stream);
}

__attribute__((visibility("default"))) int md_step(const MdWorld* w, const MdState* s, const MdConfig* c, void* stream) {
    TRY(check_phase(PH_ALL, w, s, c));
    if (c->agent_idm < MD_AGENT_INPUT || c->agent_idm > MD_AGENT_LANE_CHANGE) {
        snprintf(g_err, sizeof g_err, "agent_idm=%d: 0 (the caller's actions), 1 (IDMPolicy) or 2 (LaneChangePolicy)", c->agent_idm);
        return MD_EINVAL;
    }
    if (c->agent_idm == MD_AGENT_LANE_CHANGE && c->traffic_mode == 4) {
        snprintf(g_err, sizeof g_err, "agent_idm=2 (LaneChangePolicy) steers along the road network's lanes: not in scenario mode "
                 "(traffic_mode 4)");
        return MD_EINVAL;
    }
    if (c->traffic_mode == 4) {   // scenario mode: its own kernel (ScenarioEnv step)
        TRY(need_fields(PH_ALL, SCENARIO, w, s, c));
        if (c->is_multi_agent || c->agents_per_env != 1 || c->track_len <= 0) {
            snprintf(g_err, sizeof g_err, "scenario mode: single-agent scenes with track_len > 0 (got agents=%d track_len=%d)",
                     c->agents_per_env, c->track_len);
            return MD_EINVAL;
        }
        if (c->obs_dim != md_sc_obs_lidar(c) + c->n_beams) {
            snprintf(g_err, sizeof g_err, "scenario mode: obs_dim=%d != %d state/navi dims + n_beams=%d", c->obs_dim,
                     md_sc_obs_lidar(c), c->n_beams);
            return MD_EINVAL;
        }
        if (s->walk.n_scenes < 0 || (s->walk.n_scenes > 0 && !s->scene_of)) {   // a scene pool: scene_of says which scene
            snprintf(g_err, sizeof g_err, "scenario mode: MdState.walk.n_scenes=%d needs MdState.scene_of", s->walk.n_scenes);
            return MD_EINVAL;
        }
        const size_t lds = scenario_lds(c->cap, c->agents_per_env, c->n_side + c->n_lane_line, s->route_n != nullptr, c->route_seg_cap).bytes;
        if (s->route_n) {
            TRY(need_fields(PH_ALL, ROUTE, w, s, c));
            if (c->route_seg_cap < 1 || c->route_vert_cap < 8) {
                snprintf(g_err, sizeof g_err, "scenario mode: route buffers need route_seg_cap >= 1 and route_vert_cap >= 8 (got %d, %d)",
                         c->route_seg_cap, c->route_vert_cap);
                return MD_EINVAL;
            }
        }
        if (lds > 64 * 1024) {
            snprintf(g_err, sizeof g_err, "scenario mode: LDS image needs %zu B (cap=%d)", lds, c->cap);
            return MD_EINVAL;
        }
        if (s->scene_of)
            hipLaunchKernelGGL(scenario_step_kernel<true>, dim3(c->n_envs), dim3(256), lds, (hipStream_t)stream, *w, *s, *c, s->obs,
                               c->obs_dim, md_sc_obs_lidar(c));
        else
            hipLaunchKernelGGL(scenario_step_kernel<false>, dim3(c->n_envs), dim3(256), lds, (hipStream_t)stream, *w, *s, *c, s->obs,
                               c->obs_dim, md_sc_obs_lidar(c));
        return launch_status();
    }
    if (c->obs_dim != md_obs_lidar(c) + c->n_beams + md_obs_tail(c)) {
        snprintf(g_err, sizeof g_err, "obs_dim=%d != %d state/navi dims + n_beams=%d + %d", c->obs_dim, md_obs_lidar(c), c->n_beams,
                 md_obs_tail(c));
        return MD_EINVAL;
    }
    if (!c->is_multi_agent && c->agents_per_env != 1) {   // the single-agent kernels schedule ONE agent's observation per env
        snprintf(g_err, sizeof g_err, "single-agent envs step one agent per env (agents_per_env=%d): use the multi-agent configs", c->agents_per_env);
        return MD_EINVAL;
    }
    if (c->num_others < 0 || c->num_others > 16 || (c->num_others > 0 && c->n_beams <= 0)) {
        snprintf(g_err, sizeof g_err, "num_others=%d needs 0..16 and the lidar on", c->num_others);
        return MD_EINVAL;
    }
    TRY(need_fields(PH_ALL, OTHERS, w, s, c));
    const int r = launch<PH_ALL>(w, s, c, s->obs, c->obs_dim, md_obs_lidar(c), stream);
    if (r != MD_OK || c->num_others <= 0) return r;
    const int n = c->n_envs * c->agents_per_env;
    hipLaunchKernelGGL(others_kernel, dim3((n + 63) / 64), dim3(64), 0, (hipStream_t)stream, *w, *s, *c);
    return launch_status();
}

// the configs where the reference's rewrite of the vehicle config (numpy_expert.py:58-62) changes nothing
static int check_expert_config(const MdConfig* c, const char* who) {
    if (c->is_multi_agent || c->agents_per_env != 1 || c->traffic_mode == 4 || c->n_beams != 240 || c->lidar_range != 50.0f ||
        c->num_others != 0 || c->n_side != 0 || c->n_lane_line != 0 || c->random_agent_model != 0 ||
        c->obs_dim != MD_EXPERT_IN - 4 * MD_EXPERT_OTHERS) {
        snprintf(g_err, sizeof g_err, "%s: needs a single-agent batch with the expert's lidar (240 beams, 50 m, num_others 0), "
                 "no side / lane-line detector and random_agent_model off (obs_dim 259)", who);
        return MD_EINVAL;
    }
    return MD_OK;
}

__attribute__((visibility("default"))) int md_expert(const MdWorld* w, const MdState* s, const MdConfig* c, const float* weights,
                                                    const float* noise, float* action_out, float* mlp_out, float* obs_out,
                                                    void* stream) {
    TRY(check_common(w, s, c));
    NEED(weights); NEED(action_out);
    TRY(need_fields(kExpertEntry, ALWAYS, w, s, c));
    TRY(check_expert_config(c, "md_expert"));
    if ((uintptr_t)weights & 15) {
        snprintf(g_err, sizeof g_err, "md_expert: the packed weights must be 16-byte aligned");
        return MD_EINVAL;
    }
    hipLaunchKernelGGL(expert_kernel, dim3((c->n_envs + kExpM - 1) / kExpM), dim3(256), 0, (hipStream_t)stream, *w, *s, *c, weights,
                       noise, action_out, mlp_out, obs_out);
    return launch_status();
}

__attribute__((visibility("default"))) int md_ai_protect(const MdWorld* w, const MdState* s, const MdConfig* c, const float* weights,
                                                        const float* noise, const float* actions, float save_level,
                                                        unsigned char* takeover, unsigned char* expert_takeover, float* applied_out,
                                                        unsigned char* flags_out, float* saver_out, void* stream) {
    TRY(check_common(w, s, c));
    NEED(weights); NEED(actions); NEED(takeover); NEED(expert_takeover); NEED(applied_out); NEED(flags_out);
    TRY(need_fields(kExpertEntry | kProtectEntry, ALWAYS, w, s, c));
    TRY(check_expert_config(c, "md_ai_protect"));
    if ((uintptr_t)weights & 15) {
        snprintf(g_err, sizeof g_err, "md_ai_protect: the packed weights must be 16-byte aligned");
        return MD_EINVAL;
    }
    if (!(save_level >= 0.0f && save_level <= 1.0f)) {
        snprintf(g_err, sizeof g_err, "md_ai_protect: save_level=%g is not in [0, 1]", (double)save_level);
        return MD_EINVAL;
    }
    hipLaunchKernelGGL(ai_protect_kernel, dim3((c->n_envs + kExpM - 1) / kExpM), dim3(256), 0, (hipStream_t)stream, *w, *s, *c, weights,
                       noise, actions, save_level, takeover, expert_takeover, applied_out, flags_out, saver_out);
    return launch_status();
}

__attribute__((visibility("default"))) int md_expert_sense(const MdWorld* w, const MdState* s, const MdConfig* c, const float* weights,
                                                          const float* beam_cs240, const float* noise, float* action_out, float* mlp_out,
                                                          float* obs_out, void* stream) {
    TRY(check_common(w, s, c));
    NEED(weights); NEED(beam_cs240); NEED(action_out);
    TRY(need_fields(kSenseEntry, ALWAYS, w, s, c));
    if (((uintptr_t)weights & 15) || ((uintptr_t)beam_cs240 & 15)) {
        snprintf(g_err, sizeof g_err, "md_expert_sense: %s must be 16-byte aligned",
                 ((uintptr_t)weights & 15) ? "the packed weights" : "the beam table beam_cs240");
        return MD_EINVAL;
    }
    if (c->traffic_mode == 4) {
        snprintf(g_err, sizeof g_err, "md_expert_sense: not in scenario mode (traffic_mode 4): the expert's observation needs a road "
                 "network's navigation");
        return MD_EINVAL;
    }
    if (c->is_multi_agent && c->ma_kind == MD_MA_TOLLGATE) {
        snprintf(g_err, sizeof g_err, "md_expert_sense: not in the tollgate env (ma_kind 1): its observation has no navigation dims");
        return MD_EINVAL;
    }
    const int rows = c->n_envs * c->agents_per_env;
    hipLaunchKernelGGL(expert_sense_kernel, dim3((rows + kExpM - 1) / kExpM), dim3(256), 0, (hipStream_t)stream, *w, *s, *c, weights,
                       beam_cs240, noise, action_out, mlp_out, obs_out);
    return launch_status();
}

__attribute__((visibility("default"))) int md_topdown(const MdWorld* w, const MdState* s, const MdConfig* c, const MdTopDown* td, void* stream) {
    TRY(check_common(w, s, c));
    NEED(td);
    if (td->struct_size != (int32_t)sizeof(MdTopDown)) {
        snprintf(g_err, sizeof g_err, "MdTopDown.struct_size=%d, library expects %d", td->struct_size, (int)sizeof(MdTopDown));
        return MD_EABI;
    }
    NEED(td->out); NEED(td->ring_traffic); NEED(td->ring_pos); NEED(td->cursor);
    TRY(need_fields(kTopDownEntry, ALWAYS, w, s, c));
    if (td->frame_stack < 1 || td->post_stack < 1 || td->frame_skip < 1 || !(td->distance > 0.0f) || td->resolution < 1) {
        snprintf(g_err, sizeof g_err, "md_topdown: frame_stack=%d post_stack=%d frame_skip=%d resolution=%d distance=%g: the counts must be "
                 ">= 1 and the distance positive", td->frame_stack, td->post_stack, td->frame_skip, td->resolution, (double)td->distance);
        return MD_EINVAL;
    }
    if (td->resolution > MD_TD_MAX_RES) {
        snprintf(g_err, sizeof g_err, "md_topdown: resolution=%d is beyond MD_TD_MAX_RES=%d", td->resolution, MD_TD_MAX_RES);
        return MD_EINVAL;
    }
    // checked in 64 bits: (stack - 1) * skip + 1 of two ints
    const long long lt = (long long)(td->frame_stack - 1) * td->frame_skip + 1, lp = (long long)(td->post_stack - 1) * td->frame_skip + 1;
    if (lt > MD_TD_MAX_RING || lp > MD_TD_MAX_RING) {
        snprintf(g_err, sizeof g_err, "md_topdown: ring lengths (frame_stack-1)*frame_skip+1=%lld and (post_stack-1)*frame_skip+1=%lld must "
                 "not exceed MD_TD_MAX_RING=%d", lt, lp, MD_TD_MAX_RING);
        return MD_EINVAL;
    }
    if (c->agents_per_env != 1) {
        snprintf(g_err, sizeof g_err, "md_topdown: agents_per_env=%d: the top-down observation is single-agent (the reference asserts "
                 "the same)", c->agents_per_env);
        return MD_EINVAL;
    }
    if (c->traffic_mode == 4) {
        snprintf(g_err, sizeof g_err, "md_topdown: not in scenario mode (traffic_mode 4): its trajectory navigation and polyline map "
                 "lines are not built");
        return MD_EINVAL;
    }
    if (((uintptr_t)w->quads & 15) || ((uintptr_t)w->quad_ball & 15)) {     // read as float4 (quad_ball may be NULL)
        snprintf(g_err, sizeof g_err, "md_topdown: MdWorld.%s must be 16-byte aligned", ((uintptr_t)w->quads & 15) ? "quads" : "quad_ball");
        return MD_EINVAL;
    }
    if (w->n_maps <= 0) {
        snprintf(g_err, sizeof g_err, "md_topdown: MdWorld.n_maps=%d", w->n_maps);
        return MD_EINVAL;
    }
    const size_t lds = topdown_lds(td->resolution, topdown_staged(td->resolution, td->frame_stack)).bytes;
    const size_t block_bytes = (size_t)td->resolution * td->resolution * (2 + td->frame_stack) * (td->norm_pixel ? 4 : 1);
    const int vec = (block_bytes % 16 == 0) && (((uintptr_t)td->out & 15) == 0);
    if (td->norm_pixel) hipLaunchKernelGGL((topdown_kernel<true>), dim3(c->n_envs), dim3(256), lds, (hipStream_t)stream, *w, *s, *c, *td, vec);
    else hipLaunchKernelGGL((topdown_kernel<false>), dim3(c->n_envs), dim3(256), lds, (hipStream_t)stream, *w, *s, *c, *td, vec);
    return launch_status();
}

__attribute__((visibility("default"))) int md_render(const MdWorld* w, const MdState* s, const MdConfig* c, const MdRender* r, void* stream) {
    TRY(check_common(w, s, c));
    NEED(r);
    if (r->struct_size != (int32_t)sizeof(MdRender)) {
        snprintf(g_err, sizeof g_err, "MdRender.struct_size=%d, library expects %d", r->struct_size, (int)sizeof(MdRender));
        return MD_EABI;
    }
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

__attribute__((visibility("default"))) int md_branch(const MdState* dst, const MdState* src, const MdConfig* c, const MdBranch* b, void* stream) {
    NEED(dst); NEED(src); NEED(c); NEED(b);
    TRY(check_struct_size(c));
    if (b->struct_size != (int32_t)sizeof(MdBranch)) {
        snprintf(g_err, sizeof g_err, "MdBranch.struct_size=%d, library expects %d", b->struct_size, (int)sizeof(MdBranch));
        return MD_EABI;
    }
    NEED(b->src_row); NEED(b->dst_row);
    if (c->cap <= 0 || c->cap > MD_MAX_CAP || c->agents_per_env <= 0 || c->agents_per_env > c->cap || c->obs_dim < 0 ||
        c->route_seg_cap < 0 || c->route_vert_cap < 0) {
        snprintf(g_err, sizeof g_err, "md_branch: bad sizes: cap=%d agents_per_env=%d obs_dim=%d route_seg_cap=%d route_vert_cap=%d (cap<=%d)",
                 c->cap, c->agents_per_env, c->obs_dim, c->route_seg_cap, c->route_vert_cap, MD_MAX_CAP);
        return MD_EINVAL;
    }
    if (b->n_pairs <= 0) {
        snprintf(g_err, sizeof g_err, "md_branch: n_pairs=%d must be positive", b->n_pairs);
        return MD_EINVAL;
    }
    if (b->src_n_envs <= 0 || b->dst_n_envs <= 0) {
        snprintf(g_err, sizeof g_err, "md_branch: src_n_envs=%d and dst_n_envs=%d must be positive", b->src_n_envs, b->dst_n_envs);
        return MD_EINVAL;
    }
    if (b->n_extras < 0 || b->n_extras > MD_BR_MAX_EXTRAS) {
        snprintf(g_err, sizeof g_err, "md_branch: n_extras=%d must lie in [0, MD_BR_MAX_EXTRAS=%d]", b->n_extras, MD_BR_MAX_EXTRAS);
        return MD_EINVAL;
    }
    for (int k = 0; k < b->n_extras; ++k) {
        if (!b->extra[k].dst || !b->extra[k].src) {
            snprintf(g_err, sizeof g_err, "required pointer b->extra[%d].%s is null", k, b->extra[k].dst ? "src" : "dst");
            return MD_EINVAL;
        }
        if (b->extra[k].row_bytes <= 0) {
            snprintf(g_err, sizeof g_err, "md_branch: extra[%d].row_bytes=%lld must be positive", k, (long long)b->extra[k].row_bytes);
            return MD_EINVAL;
        }
    }
    hipLaunchKernelGGL(branch_kernel, dim3(b->n_pairs), dim3(256), 0, (hipStream_t)stream, *dst, *src, *c, *b);
    return launch_status();
}

__attribute__((visibility("default"))) int md_ped(const MdState* s, const MdConfig* c, const MdPed* p, void* stream) {
    NEED(s); NEED(c); NEED(p);
    TRY(check_struct_size(c));
    if (p->struct_size != (int32_t)sizeof(MdPed)) {
        snprintf(g_err, sizeof g_err, "MdPed.struct_size=%d, library expects %d", p->struct_size, (int)sizeof(MdPed));
        return MD_EABI;
    }
    if (c->n_envs <= 0 || c->cap <= 0 || c->cap > MD_MAX_CAP || c->substeps <= 0 || !(c->dt > 0.0f)) {
        snprintf(g_err, sizeof g_err, "md_ped: bad sizes: n_envs=%d cap=%d substeps=%d dt=%g (cap<=%d)", c->n_envs, c->cap, c->substeps,
                 (double)c->dt, MD_MAX_CAP);
        return MD_EINVAL;
    }
    if (p->wait_min_steps < 0) {
        snprintf(g_err, sizeof g_err, "md_ped: wait_min_steps=%d must not be negative", p->wait_min_steps);
        return MD_EINVAL;
    }
    TRY(need_fields(kPedEntry, ALWAYS, nullptr, s, c));
    hipLaunchKernelGGL(ped_kernel, dim3((c->n_envs + kPedEnvs - 1) / kPedEnvs), dim3(64 * kPedEnvs), 0, (hipStream_t)stream, *s, *c, *p);
    return launch_status();
}

__attribute__((visibility("default"))) int md_vector_obs(const MdWorld* w, const MdState* s, const MdConfig* c, const MdVectorObs* vo,
                                                        void* stream) {
    NEED(w); NEED(s); NEED(c); NEED(vo);
    TRY(check_struct_size(c));
    if (vo->struct_size != (int32_t)sizeof(MdVectorObs)) {
        snprintf(g_err, sizeof g_err, "MdVectorObs.struct_size=%d, library expects %d", vo->struct_size, (int)sizeof(MdVectorObs));
        return MD_EABI;
    }
    TRY(check_common(w, s, c));
    const struct { const char* name; int v, lo, hi; const char* limit; } counts[] = {
        {"num_agents", vo->num_agents, 1, MD_VO_MAX_AGENTS, "MD_VO_MAX_AGENTS"},
        {"history", vo->history, 1, MD_VO_MAX_HISTORY, "MD_VO_MAX_HISTORY"},
        {"route_points", vo->route_points, 0, MD_VO_MAX_ROUTE_POINTS, "MD_VO_MAX_ROUTE_POINTS"},
        {"num_lanes", vo->num_lanes, 0, MD_VO_MAX_LANES, "MD_VO_MAX_LANES"},
        {"lane_points", vo->lane_points, 2, MD_VO_MAX_LANE_POINTS, "MD_VO_MAX_LANE_POINTS"},
    };
    for (const auto& r : counts)
        if (r.v < r.lo || r.v > r.hi) {
            snprintf(g_err, sizeof g_err, "md_vector_obs: %s=%d must lie in [%d, %s=%d]", r.name, r.v, r.lo, r.limit, r.hi);
            return MD_EINVAL;
        }
    const struct { const char* name; float v; } lengths[] = {{"radius", vo->radius}, {"max_jump", vo->max_jump},
                                                             {"route_spacing", vo->route_spacing}};
    for (const auto& r : lengths)
        if (!(r.v > 0.0f) || !(r.v <= 1.0e18f)) {      // its square stays finite
            snprintf(g_err, sizeof g_err, "md_vector_obs: %s=%g must be positive (and at most 1e18)", r.name, (double)r.v);
            return MD_EINVAL;
        }
    if (vo->out_stride <= 0 || vo->out_stride % 16 || vo->hist_stride <= 0 || vo->hist_stride % 16) {
        snprintf(g_err, sizeof g_err, "md_vector_obs: out_stride=%d and hist_stride=%d must be positive multiples of 16", vo->out_stride,
                 vo->hist_stride);
        return MD_EINVAL;
    }
    if (c->traffic_mode == 4) {
        snprintf(g_err, sizeof g_err, "md_vector_obs: not in scenario mode (traffic_mode 4): it has no lane table and its routes are polylines");
        return MD_EINVAL;
    }
    TRY(need_fields(kVectorObsEntry, ALWAYS | MULTI, w, s, c));
    NEED(vo->agents); NEED(vo->agents_mask); NEED(vo->agents_meta); NEED(vo->ego); NEED(vo->ego_mask);
    if (vo->route_points > 0) { NEED(vo->route); NEED(vo->route_mask); }
    if (vo->num_lanes > 0) { NEED(vo->lanes); NEED(vo->lanes_meta); NEED(vo->lanes_mask); }
    NEED(vo->ring_pose); NEED(vo->ring_flags); NEED(vo->cursor);
    const void* const words[] = {vo->agents, vo->agents_meta, vo->ego, vo->route, vo->lanes, vo->lanes_meta, vo->ring_pose, vo->ring_flags,
                                 vo->cursor};
    for (const void* p : words)
        if ((uintptr_t)p & 3) {
            snprintf(g_err, sizeof g_err, "md_vector_obs: the float and int32 arrays of MdVectorObs must be 4-byte aligned");
            return MD_EINVAL;
        }
    if (w->n_maps <= 0 || w->max_lanes <= 0) {
        snprintf(g_err, sizeof g_err, "md_vector_obs: MdWorld.n_maps=%d max_lanes=%d", w->n_maps, w->max_lanes);
        return MD_EINVAL;
    }
    const int n_waves = 3 * c->agents_per_env < kVoWaves ? 3 * c->agents_per_env : kVoWaves;
    const size_t lds = (size_t)n_waves * vector_obs_lds(w->max_lanes).per_wave;
    if (lds > 64 * 1024) {
        snprintf(g_err, sizeof g_err, "md_vector_obs: the lane distances of %d waves need %zu B of LDS (max_lanes=%d); limit 65536", n_waves, lds,
                 w->max_lanes);
        return MD_EINVAL;
    }
    hipLaunchKernelGGL(vector_obs_kernel, dim3(c->n_envs), dim3(64 * n_waves), lds, (hipStream_t)stream, *w, *s, *c, *vo);
    return launch_status();
}

}  // extern "C"
