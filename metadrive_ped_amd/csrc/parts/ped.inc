// parts/ped.inc -- part of mdstep.hip, included there and not compiled on its own.
// Provides: kPedEnvs and ped_kernel (include/md_ped.h),
// and the entry point md_ped with its argument checks.
// Relies on: mdstep.hip (bcast_f), entry_checks.

namespace {

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

}  // namespace

extern "C" {

__attribute__((visibility("default"))) int md_ped(const MdState* s, const MdConfig* c, const MdPed* p, void* stream) {
    NEED(s); NEED(c); NEED(p);
    TRY(check_struct_size(c));
    TRY(check_arg_size("MdPed", p->struct_size, sizeof(MdPed)));
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

}  // extern "C"
