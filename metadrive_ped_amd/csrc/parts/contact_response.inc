// parts/contact_response.inc -- part of mdstep.hip, included there and not compiled on its own.
// Provides: kCrEnvs and contact_response_kernel (include/md_contact_response.h),
// and the entry point md_contact_response with its argument checks.
// Relies on: mdstep.hip (bcast_f), entry_checks.

namespace {

// ---- contact response (include/md_contact_response.h): ONE WAVE PER ENV, kCrEnvs envs per workgroup ----
// The wave's lanes each load one mover's shape record and the first half of its dyn record -- speed and, for a walker, its velocity
// -- (two rounds when cap > 64), so every global load of the launch is issued in the first round trip; each lane works out its
// movers' role as an obstacle (weight, velocity, reach) once.  A ballot finds the responders; for each of them in slot order its
// record is broadcast from the lane that owns it and every lane tests ITS mover(s) against it: the centre-distance cull
// (md_cr_near, which can never drop a hit), then the canonical pair test (md_cr_contact).  A ballot per round collects the hits:
// a responder without one costs nothing more.  The hits are folded in ascending slot order, each broadcast from the lane that
// holds it (md_cr_fold on wave-uniform values), and the owner keeps the result.  After the loop the owners store cx, cy and speed
// -- three dwords, plain vector stores, only for responders that had a hit; every read was of the entry state, in registers by
// then.  No LDS, no atomics.  With no contact in the batch the launch writes nothing.
constexpr int kCrEnvs = 4;
static_assert(MD_MAX_CAP <= 128, "contact_response_kernel: two lane rounds per env");

__global__ __launch_bounds__(64 * kCrEnvs) void contact_response_kernel(MdState g, MdConfig c, MdContactResponse cr) {
    const int lane = threadIdx.x & 63;
    const int e = blockIdx.x * kCrEnvs + (threadIdx.x >> 6);
    if (e >= c.n_envs) return;              // wave-uniform, as everything below that is not a lane's own mover
    if (g.need_reset[e] != 0) return;       // md_step replaces this env's rows by the snapshot
    const int cap = c.cap;
    const size_t b = (size_t)e * (size_t)cap;
    MdShape* const shape = g.shape + b;
    MdDyn* const dyn = g.dyn + b;
    MdShape vs[2] = {};                     // flags 0: not present
    float vspeed[2] = {0.0f, 0.0f};
    float ow[2] = {1.0f, 1.0f}, ovx[2] = {0.0f, 0.0f}, ovy[2] = {0.0f, 0.0f};   // this lane's movers as obstacles
    unsigned long long responders[2] = {0ull, 0ull};
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        if (r * 64 >= cap) break;
        const int j = r * 64 + lane;
        if (j < cap) {
            vs[r] = shape[j];
            const float4 d = *reinterpret_cast<const float4*>(&dyn[j]);   // heading, speed, steering, throttle
            vspeed[r] = d.y;
            ow[r] = md_cr_weight(vs[r].flags);
            md_cr_velocity(&vs[r], d.y, d.z, d.w, &ovx[r], &ovy[r]);
        }
        responders[r] = __ballot(md_drives(vs[r].flags));
    }
    MdCrAcc res[2] = {};
    bool had[2] = {false, false};
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        unsigned long long m = responders[r];
        while (m) {
            const int k = __ffsll((long long)m) - 1;
            m &= m - 1;
            const int i = r * 64 + k;
            MdShape I;
            I.cx = bcast_f(vs[r].cx, k);
            I.cy = bcast_f(vs[r].cy, k);
            I.c = bcast_f(vs[r].c, k);
            I.s = bcast_f(vs[r].s, k);
            I.hl = bcast_f(vs[r].hl, k);
            I.hw = bcast_f(vs[r].hw, k);
            I.flags = MD_KIND_VEHICLE | MD_F_ALIVE;   // a responder: a box
            I.aux = -1;
            MdCrHit h[2] = {};
            unsigned long long hits[2] = {0ull, 0ull};
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                if (q * 64 >= cap) break;
                const int j = q * 64 + lane;
                if (j != i && md_present(vs[q].flags) && md_cr_near(&I, &vs[q])) h[q] = md_cr_contact(&I, i, &vs[q], j);
                hits[q] = __ballot(h[q].hit != 0);
            }
            if ((hits[0] | hits[1]) == 0ull) continue;
            MdCrAcc a;
            a.px = a.py = 0.0f;
            a.speed = bcast_f(vspeed[r], k);
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                unsigned long long hm = hits[q];
                while (hm) {
                    const int src = __ffsll((long long)hm) - 1;
                    hm &= hm - 1;
                    md_cr_fold(&a, bcast_f(h[q].depth, src), bcast_f(h[q].nx, src), bcast_f(h[q].ny, src), bcast_f(ow[q], src),
                               bcast_f(ovx[q], src), bcast_f(ovy[q], src), I.c, I.s, cr.skin);
                }
            }
            md_cr_clamp(&a, cr.max_push);
            if (lane == k) {
                res[r].px = vs[r].cx + a.px;
                res[r].py = vs[r].cy + a.py;
                res[r].speed = a.speed;
                had[r] = true;
            }
        }
    }
#pragma unroll
    for (int r = 0; r < 2; ++r)
        if (had[r]) {                       // only an owner of a responder with a hit: r * 64 + lane < cap
            const int j = r * 64 + lane;
            shape[j].cx = res[r].px;
            shape[j].cy = res[r].py;
            dyn[j].speed = res[r].speed;
        }
}

}  // namespace

extern "C" {

__attribute__((visibility("default"))) int md_contact_response(const MdState* s, const MdConfig* c, const MdContactResponse* cr, void* stream) {
    NEED(s); NEED(c); NEED(cr);
    TRY(check_struct_size(c));
    TRY(check_arg_size("MdContactResponse", cr->struct_size, sizeof(MdContactResponse)));
    if (c->n_envs <= 0 || c->cap <= 0 || c->cap > MD_MAX_CAP) {
        snprintf(g_err, sizeof g_err, "md_contact_response: bad sizes: n_envs=%d cap=%d (cap<=%d)", c->n_envs, c->cap, MD_MAX_CAP);
        return MD_EINVAL;
    }
    if (!(cr->skin >= 0.0f)) {
        snprintf(g_err, sizeof g_err, "md_contact_response: skin=%g must not be negative", (double)cr->skin);
        return MD_EINVAL;
    }
    if (!(cr->max_push > 0.0f)) {
        snprintf(g_err, sizeof g_err, "md_contact_response: max_push=%g must be positive", (double)cr->max_push);
        return MD_EINVAL;
    }
    if (c->traffic_mode == 4) {
        snprintf(g_err, sizeof g_err, "md_contact_response: not in scenario mode (traffic_mode 4): replayed and trajectory-bound vehicles take "
                                      "their poses from data");
        return MD_EINVAL;
    }
    TRY(need_fields(kContactResponseEntry, ALWAYS, nullptr, s, c));
    hipLaunchKernelGGL(contact_response_kernel, dim3((c->n_envs + kCrEnvs - 1) / kCrEnvs), dim3(64 * kCrEnvs), 0, (hipStream_t)stream, *s, *c, *cr);
    return launch_status();
}

}  // extern "C"
