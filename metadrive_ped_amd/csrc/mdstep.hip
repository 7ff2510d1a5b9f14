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

#include <initializer_list>
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
#include "md_contact_response.h"
#include "md_vector_obs.h"
#include "md_scenario_vector_obs.h"
#include "md_traffic_lights.h"
#include "md_scenario_metrics.h"
#include "md_lean_pins.h"
#include "md_lean_view.h"
#include "md_write_back_own.h"

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
// a wave's end where the waves of an env end apart (the lean kernels' own write-back): slot 11 / 13 keep the LATEST wave's
#define MD_STAMP_WAVE_END(cond)                                                                \
    do {                                                                                       \
        if ((cond) && g_stamp_buf) {                                                           \
            atomicMax(&g_stamp_buf[(size_t)blockIdx.x * 32 + 11], (unsigned long long)__builtin_readcyclecounter()); \
            atomicMax(&g_stamp_buf[(size_t)blockIdx.x * 32 + 13], (unsigned long long)__builtin_amdgcn_s_memrealtime()); \
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
// the lean kernel's observation ahead (observe_ahead_wave): start / end of the evaluation in stamp slots 2 / 5, which that kernel does
// not write otherwise, by the lane that `cond` picks; its counts per env above the localisations in fine slot 12, a byte each
#define MD_AHEAD_STAMP(cond, i)                                                                \
    do {                                                                                       \
        if ((cond) && g_stamp_buf) g_stamp_buf[(size_t)blockIdx.x * 32 + (i)] = __builtin_readcyclecounter(); \
    } while (0)
enum : int { MD_AHEAD_EVALUATED = 32, MD_AHEAD_HIT = 40, MD_AHEAD_MISS = 48 };
#define MD_AHEAD_COUNT(cond, what)                                                             \
    do {                                                                                       \
        if ((cond) && g_stamp_buf) atomicAdd(&g_stamp_buf[(size_t)blockIdx.x * 32 + 16 + 12], 1ull << (what)); \
    } while (0)
// the contacts of the agent in slot 0 (contacts_vehicle), in a buffer of their own (md_debug_set_contacts_buffer: 8 words per env; the 32
// above are all taken; zeroed by the caller before the stamped step): 0 / 1 start / end of the mover loop, 2 the end of the quads part
// (grid header to the last cell's items), 4 the grid cells under the chassis, 5 the cell items read (both added up, by one lane)
__device__ unsigned long long* g_contacts_buf = nullptr;
#define MD_CONTACTS_STAMP(cond, i)                                                             \
    do {                                                                                       \
        if ((cond) && g_contacts_buf) g_contacts_buf[(size_t)blockIdx.x * 8 + (i)] = __builtin_readcyclecounter(); \
    } while (0)
#define MD_CONTACTS_COUNT(cond, cells, items)                                                  \
    do {                                                                                       \
        if ((cond) && g_contacts_buf) {                                                        \
            g_contacts_buf[(size_t)blockIdx.x * 8 + 4] += (unsigned long long)(cells);         \
            g_contacts_buf[(size_t)blockIdx.x * 8 + 5] += (unsigned long long)(items);         \
        }                                                                                      \
    } while (0)
#else
#define MD_CONTACTS_STAMP(cond, i) do { } while (0)
#define MD_CONTACTS_COUNT(cond, cells, items) do { } while (0)
#define MD_STAMP_AT(i) do { } while (0)
#define MD_STAMP_WAVE_END(cond) do { } while (0)
#define MD_FINE_STAMP(cond, i) do { } while (0)
#define MD_LOC_COUNT(cond, hit) do { } while (0)
#define MD_AHEAD_STAMP(cond, i) do { } while (0)
#define MD_AHEAD_COUNT(cond, what) do { } while (0)
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

// ------------------------------------------------------------------------------------------------
// Lidar for one agent's WHOLE cloud by one wave, FLAT over the (mover, beam) pairs that can meet: the two lean non-staged workgroup
// kernels (no detected sets, the cloud goes to HBM).  lidar_item casts all 64 beams of a sector at every mover its cone cull keeps,
// and derives the cull once per sector; a vehicle 20 m away meets a dozen of 240 beams.  Here:
//   (1) lanes = slots: md_lidar_beam_span gives each present mover the cyclic range of beams that can come within its bounding
//       radius (correctly rounded, conservative: tests/test_lidar_span_host.py), once per cloud;
//   (2) lanes = pairs: lane t of a pass takes pair t of the movers' spans laid end to end.  The owner is found by walking the
//       movers' ballot with a running count in scalar registers (a handful of movers: cheaper than a prefix scan and a search
//       through ds_bpermute); movers that lie wholly before or behind the pass are stepped over;
//   (3) the lane casts its beam at its mover with the same md_ray_shape and, under lidar_item's predicate t < 1.0f, lowers the
//       beam's word in `row` (LDS, n_beams words of this wave, set to the bits of 1.0f) with atomicMin on the float's bits: t lies
//       in (0, 1), where unsigned order is float order; a NaN fails the predicate in both forms.
// A beam's value is the minimum of the same fractions over a superset of the movers that can hit it, and a minimum does not depend
// on the order: the same bits as lidar_item's.
// ------------------------------------------------------------------------------------------------
#ifndef MD_LIDAR_FLAT
#define MD_LIDAR_FLAT 1
#endif
__device__ __forceinline__ void lidar_agent_flat(const MdWorld& w, const MdState& s, const MdConfig& c, int a, int lane,
                                                 float* __restrict__ out_row, uint32_t* row) {
    const MdShape me = s.shape[a];  // wave-uniform
    const int nb = c.n_beams;
    if (!md_present(me.flags)) {
        for (int b = lane; b < nb; b += 64) st_stream_f(&out_row[b], 1.0f);
        return;
    }
    for (int b = lane; b < nb; b += 64) row[b] = 0x3f800000u;
    wave_lds_sync();
    for (int j0 = 0; j0 < c.cap; j0 += 64) {
        const int j = j0 + lane;
        int first = 0, cnt = 0;
        if (j < c.cap && j != a) {
            const MdShape o = s.shape[j];
            if (md_present(o.flags)) md_lidar_beam_span(me.cx, me.cy, me.c, me.s, c.lidar_range, nb, &o, &first, &cnt);
        }
        const unsigned long long movers = __ballot(cnt > 0);
#if MD_LIDAR_FLAT == 2
        // the other form: one pass per mover that can be met, over its own span alone -- no owner search, and since a pass holds a
        // beam once, a plain read-min-write of the row's words
        for (unsigned long long m = movers; m;) {
            const int k = __ffsll((long long)m) - 1;
            m &= m - 1;
            const int ck = __builtin_amdgcn_readlane(cnt, k), fk = __builtin_amdgcn_readlane(first, k);
            const MdShape o = s.shape[j0 + k];
            for (int i = lane; i < ck; i += 64) {
                int beam = fk + i;
                if (beam >= nb) beam -= nb;
                const float bc = w.beam_cs[2 * beam], bs = w.beam_cs[2 * beam + 1];
                const float dirx = (bc * me.c - bs * me.s) * c.lidar_range;
                const float diry = (bs * me.c + bc * me.s) * c.lidar_range;
                const float tt = md_ray_shape(me.cx, me.cy, dirx, diry, o.cx, o.cy, o.c, o.s, o.hl, o.hw, md_kind_of(o.flags));
                if (tt < 1.0f && __float_as_uint(tt) < row[beam]) row[beam] = __float_as_uint(tt);
            }
            wave_lds_sync();
        }
#else
        int total = 1;   // wave-uniform; known after the first pass
        for (int t0 = 0; t0 < total; t0 += 64) {
            const int t = t0 + lane;
            int owner = -1, beam = 0;
            int run = 0;   // pairs of the movers before this one
            for (unsigned long long m = movers; m;) {
                const int k = __ffsll((long long)m) - 1;
                m &= m - 1;
                const int ck = __builtin_amdgcn_readlane(cnt, k);
                const int at = run;
                run += ck;
                if (run <= t0 || at >= t0 + 64) continue;   // wholly before / behind this pass (the count goes on for `total`)
                const int fk = __builtin_amdgcn_readlane(first, k);
                if ((unsigned)(t - at) < (unsigned)ck) {
                    owner = k;
                    beam = fk + (t - at);
                }
            }
            total = run;
            if (owner >= 0) {
                if (beam >= nb) beam -= nb;
                const MdShape o = s.shape[j0 + owner];
                const float bc = w.beam_cs[2 * beam], bs = w.beam_cs[2 * beam + 1];
                const float dirx = (bc * me.c - bs * me.s) * c.lidar_range;
                const float diry = (bs * me.c + bc * me.s) * c.lidar_range;
                const float tt = md_ray_shape(me.cx, me.cy, dirx, diry, o.cx, o.cy, o.c, o.s, o.hl, o.hw, md_kind_of(o.flags));
                if (tt < 1.0f) atomicMin(&row[beam], __float_as_uint(tt));
            }
        }
#endif
    }
    wave_lds_sync();
    for (int b = lane; b < nb; b += 64) st_stream_f(&out_row[b], __uint_as_float(row[b]));
    __builtin_amdgcn_wave_barrier();   // the row is free again
}

// The waves take the AGENTS as they get free (`tickets`: LDS counter, zeroed by the caller behind a barrier); `rows`: n_beams words
// of LDS per wave (env_lds_lidar_rows).
__device__ __forceinline__ void phase_lidar_flat(const MdWorld& w, const MdState& s, const MdConfig& c, int e, int tid, float* out,
                                                 int out_stride, int out_offset, int* tickets, uint32_t* rows) {
    // the wave's number is made again from an opaque copy of tid, in a scalar register: carried from the kernel's entry it is one
    // more VGPR live across every stage, and the lean kernels have none to spare (narrow: v3 and 16 B of scratch instead of v2 and
    // 12 B).  This steers the register allocator of ONE compiler: after a toolchain change read the two lean kernels' lines of
    // tools/kernel_regs.sh again -- nothing else guards the register rule here.
    int tid_here = tid;
    asm("" : "+v"(tid_here));
    const int wave = __builtin_amdgcn_readfirstlane(tid_here >> 6), lane = tid & 63;
    for (int guard = 0; guard < c.agents_per_env; ++guard) {
        int a = 0;
        if (lane == 0) a = atomicAdd(tickets, 1);
        a = __builtin_amdgcn_readfirstlane(a);
        if (a < 0 || a >= c.agents_per_env) break;
        float* row = out + (size_t)(e * c.agents_per_env + a) * out_stride + out_offset;
        lidar_agent_flat(w, s, c, a, lane, row, rows + (size_t)wave * c.n_beams);
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

}  // namespace

// The wave-level stages of the step, one part each: a part is included here and not compiled on its own, opens its own namespace
// and names what it provides and relies on in its first lines.  Cuts of this file's text, in its order.
#include "parts/localize.inc"     // grid_clampi, localize_*, hull_*; MD_LOC_ROAD_FIRST
#include "parts/contacts.inc"     // contacts_quad_bits, contacts_vehicle; MD_CONTACTS_FLAT
#include "parts/idm.inc"          // gap keys, wave_argmin, idm_*
#include "parts/observe.inc"      // observe_*; MD_OBS_LOCKSTEP, MD_OBS_AHEAD
#include "parts/trigger.inc"      // trigger_*; MD_TRIGGER_EARLY
#include "parts/lifecycle.inc"    // lifecycle_block (multi-agent envs)
#include "parts/lean_view.inc"    // lean_args_here, LEAN_ARG, lean_view_*; MD_LEAN_VIEW

namespace {

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
// field of MD_LEAN_PINS (include/md_lean_pins.h) has its pinned value: variant<PH_ALL>() (the launch predicate) asks
// md_lean_pins_hold(), and the kernels overwrite their by-value copies of the arguments from the same list (lean_pins_fold; all but
// the staged-map env_kernel, see there), so the branches on these fields fold away instead of riding along in SGPRs.  ONE list for
// both sides: a field taken out of the predicate is no longer folded.
__device__ __forceinline__ void lean_pins_fold(MdState& s, MdConfig& c) {
#define MD_PIN_ZERO(f) c.f = 0;
#define MD_PIN_NUL(p) s.p = nullptr;
    MD_LEAN_PINS(MD_PIN_ZERO, MD_PIN_NUL)
#undef MD_PIN_ZERO
#undef MD_PIN_NUL
}
// The size pins (MD_LEAN_SIZE_PINS, same header): variant<PH_ALL>() sends a lean batch to the NARROW instantiation of the
// non-staged env_kernel only while md_lean_size_pins_hold(), and that instantiation alone folds them.  A pinned value overwrites
// the argument in `c`.  A bound goes into `c_scan`, the copy that the whole-wave slot scans read (lidar, IDM candidates and gap
// keys, trigger search and fire), as min(field, bound): a no-op under the predicate that tells the compiler the scan is one pass.
// `c` itself keeps the field as it came: with the bound on the contacts' mover loop, the mask scans or the per-thread loops the
// kernel breaks the register rule (EXPERIMENTS.md, "Size pins"); the masks drop their second word in the kernel itself.
__device__ __forceinline__ void lean_size_pins_fold(MdConfig& c, MdConfig& c_scan) {
#define MD_PIN_EQUALS(f, v) c.f = (v);
#define MD_PIN_AT_MOST(f, v)
    MD_LEAN_SIZE_PINS(MD_PIN_EQUALS, MD_PIN_AT_MOST)
#undef MD_PIN_EQUALS
#undef MD_PIN_AT_MOST
    c_scan = c;
#define MD_PIN_EQUALS(f, v)
#define MD_PIN_AT_MOST(f, v) c_scan.f = min(c.f, (v));
    MD_LEAN_SIZE_PINS(MD_PIN_EQUALS, MD_PIN_AT_MOST)
#undef MD_PIN_EQUALS
#undef MD_PIN_AT_MOST
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
                                                                     // (lean kernel: wave 0's 48 also carry the observation ahead's hand-over, ObsAheadWord)
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

// The result words of the flat lidar pass (lidar_agent_flat): n_beams words per wave BEHIND the image -- in the dynamic size of the
// launches that use them (launch<PH_ALL>, behind its fit check), not in env_lds().bytes, which the entry points' messages quote.
// -> their offset.  The entry checks bound n_beams by 1024: four waves' words are at most 16 KB.
__host__ __device__ inline uint32_t env_lds_lidar_rows(uint32_t image_bytes) { return align_up(image_bytes, 16); }

// BLK: threads of the workgroup (MD_ENV_BLOCK; multi-agent batches small enough to stay resident are also instantiated with 512:
// eight waves share an env's 20-40 agents -- lifecycle search, contacts, observe groups, lidar sectors -- instead of four).
// NARROW: the lean non-staged kernel of a batch that holds the size pins too (lean_size_pins_fold): one agent, at most 64 slots.
template <int PH, bool STAGE_MAP, bool RESPAWN = false, bool MULTI = false, int BLK = MD_ENV_BLOCK, bool NARROW = false>
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
    // ... and ahead, by a wave that the locate stage leaves without an item (observe_ahead_wave): the lean kernel only
    constexpr bool kObsAhead = MD_OBS_AHEAD && kObsLockstep && kWaves > 1;
    // the agent's contacts with the quads in one flat pass over the cells under the chassis (contacts_vehicle): the lean kernel only
    constexpr bool kContactsFlat = MD_CONTACTS_FLAT && PH == PH_ALL && kIdmKeys;
    // the env's pointers derived where they are used, from the kernel-argument segment (parts/lean_view.inc): the lean kernel only.
    // It reads NOTHING from its by-value arguments: they are cleared here and refilled, the stage-in's few fields now, the rest of
    // `w` and `c` behind the stage-in's loads, each cold group of `g` at the head of its stage.
    constexpr bool kLeanView = MD_LEAN_VIEW && PH == PH_ALL && kIdmKeys && BLK >= 256;
    // each wave stores the slots it finished and leaves; no last barrier but in a reset step (parts/lean_view.inc, include/
    // md_write_back_own.h): the same two kernels.  Not in a knockout build, where a stage that owns slots is compiled out.
    constexpr bool kWriteBackOwn = MD_WRITE_BACK_OWN && kLeanView && MD_ENV_SKIP == 0;
    LeanStageIn lean_in;
    if constexpr (kLeanView) {
        lean_in = lean_stage_in_args(lean_args_entry());
        w = MdWorld{};
        g = MdState{};
        c = MdConfig{};
        c.n_envs = lean_in.n_envs;
        c.cap = lean_in.cap;
        c.agents_per_env = lean_in.agents;
    }
    // The lean launch: variant<PH_ALL>() guarantees the pins.  Not in the staged-map kernel: folded, its scratch grows from 16 to
    // 80 B per lane (EXPERIMENTS.md, "Lean kernels fold what their launch pins"), so it keeps reading the fields.
    if constexpr (PH == PH_ALL && !RESPAWN && !MULTI && !STAGE_MAP) lean_pins_fold(g, c);
    static_assert(!NARROW || (PH == PH_ALL && !RESPAWN && !MULTI && !STAGE_MAP), "NARROW: a form of the lean non-staged kernel only");
    MdConfig c_scan = c;   // what the whole-wave slot scans read: `c`, but for the NARROW kernel's bounds
    if constexpr (NARROW) lean_size_pins_fold(c, c_scan);   // variant<PH_ALL>() guarantees them
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

    MdState gv = md_env_view(&g, &c, e);  // this env's slices of the global arrays (kLeanView: all null here)
    const MdLane* lanes;
    const MdRoad* roads;
    if constexpr (kLeanView) lean_view_stage_in(gv, lean_in, e, cap, c.agents_per_env);
    // The reset flag is loaded first but nothing below waits for it: the live state is staged
    // unconditionally (one round trip) and only a resetting env re-stages from the snapshot.
    const int reset_flag = (PH & PH_RESET) ? gv.need_reset[0] : 0;

    MD_STAMP_AT(0);
    const bool kFusedAct = (PH == PH_ALL) && gv.agent_action != nullptr;  // md_step only: agents' actions from the caller's buffer
    if (STAGE_MAP) {
        lanes = l_lanes;
        roads = l_roads;
    } else if constexpr (!kLeanView) {
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
        if constexpr (kLeanView) {
            // behind the stage-in's loads, while they are in flight: what the stages below read of `w` and `c` (the three fields
            // above stay the values the image was laid out with), the env's map tables and the routes, which the locate stage may follow at once
            lean_view_map(&lanes, &roads, lean_args_entry(), e);   // before the asm below, or its loads could not be scalar ones
            const LeanArgs kb = lean_args_here();
            const int n_envs = c.n_envs, agents = c.agents_per_env;
            lean_arg_copy(w, kb, offsetof(MdStepArgs, w));
            lean_arg_copy(c, kb, offsetof(MdStepArgs, c));
            c.n_envs = n_envs;
            c.cap = cap;
            c.agents_per_env = agents;
            lean_pins_fold(g, c);
            c_scan = c;
            if constexpr (NARROW) lean_size_pins_fold(c, c_scan);
            lean_view_routes(gv, kb, e, cap);
        }
        if (STAGE_MAP) {
            const int m = w.env_map[e];
            const int lo = w.lane_off[m], ro = w.road_off[m];
            copy16(l_lanes, w.lanes + lo, (w.lane_off[m + 1] - lo) * (int)sizeof(MdLane), tid, kBlock);
            copy16(l_roads, w.roads + ro, (w.road_off[m + 1] - ro) * (int)sizeof(MdRoad), tid, kBlock);
        }
        // kLeanView: the stores' predicates are made again from an opaque copy of tid (a v_cmp each), not carried from the loads
        // in SGPR pairs that the argument copy above pushes into VGPR lanes ahead of the first load
        int tid_st = tid;
        if constexpr (kLeanView) asm("" : "+v"(tid_st));
        if (tid_st < n32) {
            reinterpret_cast<uint4*>(l_shape)[tid] = r_shape;
            reinterpret_cast<uint4*>(l_dyn)[tid] = r_dyn;
            reinterpret_cast<uint4*>(l_pid)[tid] = r_pid;
            reinterpret_cast<uint4*>(l_param)[tid] = r_param;
        }
        if (tid_st < n64) reinterpret_cast<uint4*>(l_nav)[tid] = r_nav0;
        for (int i = tid + kBlock; i < n64; i += kBlock) reinterpret_cast<uint4*>(l_nav)[i] = g_nav[i];
        if (tid_st < cap) {
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
        if constexpr (kLeanView) lean_view_reset(gv, e, cap);
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
    if (kObsAhead && tid == 0) reinterpret_cast<int*>(smem + L.scratch)[kAhMark] = 0;   // wave 0's scratch: nothing evaluated ahead yet
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
        trigger_search_wave(s, c_scan, lane, &min_order, &trig_road);
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
        drv_hi = NARROW ? 0ull : drv.hi;   // NARROW: at most 64 slots, every mask is its low word (the k-th-bit walks and the flag merge fold)
        // contacts only for agents (traffic's crash flags are never read): their slots are the first A
        const SlotMask adrv = agent_share(drv, c.agents_per_env);
        const unsigned long long adrv_lo = adrv.lo, adrv_hi = NARROW ? 0ull : adrv.hi;
        const int nd = NARROW ? __popcll(drv_lo) : popc(drv), na = NARROW ? __popcll(adrv_lo) : popc(adrv);
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
                } else if (!(MD_ENV_SKIP & 8)) contacts_vehicle<kContactsFlat>(w, s, c, e, kth_bit(adrv_lo, adrv_hi, item - nd), lane, l_cfl);
            }
            // the first wave without an item: agent 0's observation context and tasks from the navigation words as they stand,
            // into wave 0's scratch (the last wave is free here too: its trigger fires behind this stage's barrier)
            if constexpr (kObsAhead) {
                if (nd + na < kWaves && wave == nd + na && !(MD_ENV_SKIP & 16))
                    observe_ahead_wave(lanes, roads, s, c, lane, reinterpret_cast<float*>(smem + L.scratch));
            }
        } else {
            // many vehicles awake: two localisations per wave (32 lanes each), halving the rounds
            const int npair = (nd + 1) >> 1;
            for (int item = wave; item < npair + na; item += kWaves) {
                if (item < npair) {
                    if (!(MD_ENV_SKIP & 4)) localize_pair<kLocRoadFirst>(w, lanes, roads, s, e, kth_bit(drv_lo, drv_hi, 2 * item), kth_bit(drv_lo, drv_hi, 2 * item + 1), lane, l_onlane);
                } else if (!(MD_ENV_SKIP & 8))
                    contacts_vehicle<kContactsFlat>(w, s, c, e, kth_bit(adrv_lo, adrv_hi, item - npair), lane, l_cfl);
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
                trigger_fire_wave(lanes, s, c_scan, lane, __builtin_amdgcn_readfirstlane(l_trig[0]), __builtin_amdgcn_readfirstlane(l_trig[1]));
            } else trigger_env(lanes, s, c_scan, lane);
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
            if constexpr (kLeanView) {
                // wave 0 alone reads the outputs and the reward / cost / done scheme: both from the argument segment, here
                const LeanArgs ko = lean_args_here();
                MdConfig co;
                lean_arg_copy(co, ko, offsetof(MdStepArgs, c));
                co.n_envs = c.n_envs;
                co.cap = cap;
                co.agents_per_env = c.agents_per_env;
                MdConfig co_scan;
                lean_pins_fold(g, co);
                if constexpr (NARROW) lean_size_pins_fold(co, co_scan);
                MdState so = s;
                lean_view_observe(so, ko, e, co.agents_per_env, co.obs_dim);
                if (!(MD_ENV_SKIP & 16))
                    for (int a = 0; a < co.agents_per_env; ++a) {
                        observe_agent_wave1<kObsLockstep, kObsAhead>(lanes, roads, so, co, a, just_reset, lane, l_scratch);
                        if (kWriteBackOwn && !do_reset) {   // the agent's slot is final: nothing but this observe writes it behind the traffic stage
                            wave_lds_sync();
                            const int fa = l_shape[a].flags;
                            if (md_wb_owner(fa, fa & MD_F_AGENT, l_cfl[a] == kRemovedMark) == MD_WB_WAVE0)
                                lean_store_slot(l_shape, l_dyn, l_pid, l_nav, l_action, l_flags, e, cap, a, lane);
                        }
                    }
            } else if (!(MD_ENV_SKIP & 16))
                for (int a = 0; a < c.agents_per_env; ++a) observe_agent_wave1<kObsLockstep, kObsAhead>(lanes, roads, s, c, a, just_reset, lane, l_scratch);
        } else if (!(MD_ENV_SKIP & 2)) {
            // the driving traffic vehicles by RANK, not by slot: dealt by slot (j = A + wave - 1, + kWaves - 1, ...) two of an env's
            // two or three vehicles meet on one wave in every third env while another wave idles
            int rank = 0;
            for (int j0 = 0; j0 < cap; j0 += 64) {
                const int jl = j0 + lane;
                const int fl = (jl < cap) ? s.shape[jl].flags : 0;
                unsigned long long mk = __ballot(jl < cap && md_drives(fl) && !(fl & MD_F_AGENT));
                if (kWriteBackOwn && !do_reset && wave == kWaves - 1) {
                    // the rest pass: slots that no wave writes behind the traffic stage's barrier (removed in this step, walkers).
                    // An agent's slot beyond the agents that wave 0 observes is nobody's to write either: taken here too.
                    const int own = jl < cap ? md_wb_owner(fl, fl & MD_F_AGENT, l_cfl[jl] == kRemovedMark) : MD_WB_NOBODY;
                    unsigned long long rest = __ballot(own == MD_WB_REST || (own == MD_WB_WAVE0 && jl >= c.agents_per_env));
                    while (rest) {   // usually none
                        const int j = j0 + __ffsll((long long)rest) - 1;
                        rest &= rest - 1;
                        lean_store_slot(l_shape, l_dyn, l_pid, l_nav, l_action, l_flags, e, cap, j, lane);
                    }
                }
                while (mk) {
                    const int j = j0 + __ffsll((long long)mk) - 1;
                    mk &= mk - 1;
                    if (rank % (kWaves - 1) == wave - 1) {
                        idm_vehicle_wave<kIdmKeys>(w, lanes, roads, s, c_scan, w.env_map[e], j, lane, reinterpret_cast<int*>(l_scratch));
                        if (kWriteBackOwn && !do_reset) {   // the vehicle's slot is final: other vehicles' IDM only read it
                            wave_lds_sync();
                            lean_store_slot(l_shape, l_dyn, l_pid, l_nav, l_action, l_flags, e, cap, j, lane);
                        }
                    }
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
        if constexpr (kLeanView) {   // where the cloud goes: read here
            const LeanArgs kl = lean_args_here();
            lidar_out = LEAN_ARG(kl, lidar_out);
            lidar_stride = LEAN_ARG(kl, lidar_stride);
            lidar_offset = LEAN_ARG(kl, lidar_offset);
        }
        // the two lean non-staged kernels: one wave per agent, flat over the (mover, beam) pairs (lidar_agent_flat)
        constexpr bool kLidarFlat = MD_LIDAR_FLAT && PH == PH_ALL && kIdmKeys;
        if constexpr (kLidarFlat) {
            const uint32_t rows_at = env_lds_lidar_rows(env_lds(cap, c.agents_per_env, 0, 0, kWaves, false, false).bytes);
            if (c.n_beams > 0) phase_lidar_flat(w, s, c_scan, e, tid, lidar_out, lidar_stride, lidar_offset, &l_tk[2], reinterpret_cast<uint32_t*>(smem + rows_at));
        } else if (c.n_beams > 0) phase_lidar(w, s, c_scan, e, tid, kWaves, lidar_out, lidar_stride, lidar_offset, track_det ? l_det : nullptr, PH == PH_ALL ? &l_tk[2] : nullptr);
    }

    MD_STAMP_AT(9);
    // ---- write the modified arrays back (coalesced 16-byte stores) ----
    if (!kLidarOnly) {
        if constexpr (kWriteBackOwn) {
            if (!do_reset) {   // every slot is stored by the wave that finished it (see the observe || IDM stage): the waves end apart
                MD_STAMP_AT(10);
                MD_STAMP_WAVE_END(lane == 0);
                return;
            }
        }
        __syncthreads();
        MD_STAMP_AT(10);
        constexpr bool respawns = (PH & PH_TRAFFIC) && RESPAWN;  // traffic respawn rewrites a whole slot
        if constexpr (kLeanView) lean_view_write_back(gv, e, cap);   // its targets: derived again here, not carried from the entry
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

}  // namespace

// Everything above is the step path: the wave-level stages, the three step kernels and the sensors they share.  What follows
// it is one part per side feature: kernel, LDS layout and, beside them, the extern "C" entry point with its argument checks;
// entry_checks (host only) stands before them.  A part is included here and not compiled on its own; it opens its own namespace.
#include "parts/entry_checks.inc" // host only: TRY / NEED, check_struct_size, check_common, need, the kNeeds table, need_fields, launch_status
#include "parts/draws.inc"        // lidar_detect_kernel, swap_draw_kernel, curriculum_kernel; md_swap_draw, md_curriculum
#include "parts/branch.inc"       // branch_kernel; md_branch (env snapshots)
#include "parts/ped.inc"          // ped_kernel; md_ped (crossing pedestrians)
#include "parts/contact_response.inc" // contact_response_kernel; md_contact_response
#include "parts/vector_obs.inc"   // vector_obs_kernel; md_vector_obs
#include "parts/scenario_vector_obs.inc" // scenario_vector_obs_kernel; md_scenario_vector_obs (after vector_obs: it reuses vo_agents_block)
#include "parts/traffic_lights.inc" // traffic_lights_kernel; md_traffic_lights (after vector_obs: it reuses vo_key)
#include "parts/scenario_metrics.inc" // scenario_metrics_kernel; md_scenario_metrics
#include "parts/others.inc"       // others_kernel: the observation's "others" block, launched by md_step
#include "parts/expert.inc"       // expert_kernel, expert_sense_kernel, ai_protect_kernel; md_expert, md_ai_protect, md_expert_sense
#include "parts/topdown.inc"      // topdown_kernel (its entry point md_topdown stays below: see DESIGN.md section 4)
#include "parts/render.inc"       // render_push_kernel, render_kernel; md_render

namespace {

__global__ void probe_kernel(int op, const float* a, const float* b, float* out, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = md_probe_eval(op, a[i], b[i]);
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

// The kernel a phase launches.  md_step of the single-agent envs has two: env_kernel (one 4-wave workgroup per env) and
// wave_step_kernel (one wave per env), chosen by MdConfig.step_kernel alone (0 = workgroup, 1 = wave): the host decides -- it
// knows how many distinct maps the batch shares, which is what tips the balance (metadrive_ped_amd/engine.py) -- and the
// library reads no environment variable.  The wave kernel is wave_step_kernel<respawn>; the workgroup kernel is
// env_kernel<PH, stage, respawn, multi>, or <PH_ALL, stage, false, true, 512> when wide.
struct Variant {
    bool wave, stage, respawn, multi, wide, narrow;
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
                (PH == PH_ALL ? !md_lean_pins_hold(s, c) : (c->traffic_mode != 0 || c->agent_idm != 0));
    // Multi-agent md_step: eight waves per env while every workgroup of the batch is resident at once at that size (the MULTI
    // kernel's 92 VGPRs allow 5 waves per SIMD = 640 eight-wave workgroups on the 256 CUs); larger batches keep four, which
    // then fill the chip by themselves.  Measured: 512 tollgate envs x 40 agents, 1024 roundabout envs (profiles/r03_*).
    v.wide = PH == PH_ALL && v.multi && c->n_envs <= kWideMaxEnvs && MD_ENV_BLOCK == 256 && c->agents_per_env > 8;
    // the lean non-staged workgroup kernel has a narrow form for the batches that hold the size pins as well; a lean batch that
    // does not keeps the lean kernel itself (never the RESPAWN variant: no gap keys, no road-first localisation there)
    v.narrow = PH == PH_ALL && !v.wave && !v.stage && !v.multi && !v.respawn && md_lean_size_pins_hold(c);
    return v;
}

template <int PH, bool RESPAWN, bool MULTI, int BLK = MD_ENV_BLOCK>
void launch_env(bool stage, size_t lds, hipStream_t st, const MdWorld* w, const MdState* s, const MdConfig* c, float* lidar_out,
                int stride, int offset) {
    if (stage) hipLaunchKernelGGL((env_kernel<PH, true, RESPAWN, MULTI, BLK>), dim3(c->n_envs), dim3(BLK), lds, st, *w, *s, *c, lidar_out, stride, offset);
    else hipLaunchKernelGGL((env_kernel<PH, false, RESPAWN, MULTI, BLK>), dim3(c->n_envs), dim3(BLK), lds, st, *w, *s, *c, lidar_out, stride, offset);
}

// md_step alone has the narrow form (variant<PH>().narrow is false for every other PH)
template <int PH>
void launch_narrow(size_t lds, hipStream_t st, const MdWorld* w, const MdState* s, const MdConfig* c, float* lidar_out, int stride, int offset) {
    if constexpr (PH == PH_ALL)
        hipLaunchKernelGGL((env_kernel<PH_ALL, false, false, false, MD_ENV_BLOCK, true>), dim3(c->n_envs), dim3(MD_ENV_BLOCK), lds, st, *w, *s, *c, lidar_out, stride, offset);
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
    size_t lds_launch = lds;   // the lean non-staged kernels' flat lidar pass: its result words behind the image, where they fit
    if (PH == PH_ALL && MD_LIDAR_FLAT && !v.stage && !v.multi && !v.respawn) {
        if (c->n_beams > 0) lds_launch = env_lds_lidar_rows((uint32_t)lds) + (size_t)(MD_ENV_BLOCK / 64) * c->n_beams * sizeof(uint32_t);
        if (lds_launch > 64 * 1024) {
            snprintf(g_err, sizeof g_err, "LDS image of one env and its lidar rows need %zu B (cap=%d, n_beams=%d); limit 65536", lds_launch, c->cap, c->n_beams);
            return MD_EINVAL;
        }
    }
    // the instantiations: PH_ALL all four; the phases that can be multi-agent or respawn two; the others one (per stage)
    constexpr bool kAll = PH == PH_ALL, kMulti = (PH & (PH_LIFECYCLE | PH_RESET)) != 0;
    constexpr bool kRespawn = (PH & (PH_TRAFFIC | PH_RESET | PH_INTEGRATE)) != 0;
    if (v.wide) launch_env<PH, false, kAll, kAll ? 512 : MD_ENV_BLOCK>(v.stage, lds, st, w, s, c, lidar_out, stride, offset);
    else if (v.multi) launch_env<PH, false, kMulti>(v.stage, lds, st, w, s, c, lidar_out, stride, offset);
    else if (v.respawn) launch_env<PH, kRespawn, false>(v.stage, lds, st, w, s, c, lidar_out, stride, offset);
    else if (kAll && v.narrow) launch_narrow<PH>(lds_launch, st, w, s, c, lidar_out, stride, offset);
    else launch_env<PH, false, false>(v.stage, lds_launch, st, w, s, c, lidar_out, stride, offset);
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
// diagnostic build only: buffer of n_envs * 8 uint64 device words for the agent's contacts (the workgroup kernels: one env per
// workgroup), or NULL
__attribute__((visibility("default"))) int md_debug_set_contacts_buffer(void* dev_ptr) {
    unsigned long long* p = (unsigned long long*)dev_ptr;
    return hipMemcpyToSymbol(HIP_SYMBOL(g_contacts_buf), &p, sizeof(p)) == hipSuccess ? MD_OK : MD_ELAUNCH;
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

__attribute__((visibility("default"))) int md_topdown(const MdWorld* w, const MdState* s, const MdConfig* c, const MdTopDown* td, void* stream) {
    TRY(check_common(w, s, c));
    NEED(td);
    TRY(check_arg_size("MdTopDown", td->struct_size, sizeof(MdTopDown)));
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

}  // extern "C"
