// parts/scenario_metrics.inc -- part of mdstep.hip, included there and not compiled on its own.
// Provides: kSmWaves, scenario_metrics_kernel (include/md_scenario_metrics.h), and the entry point md_scenario_metrics with its
// argument checks.
// Relies on: mdstep.hip (wave_lds_sync), entry_checks.

namespace {

// ---- the closed-loop metrics of scenario mode (include/md_scenario_metrics.h): ONE WAVE PER ENV, kSmWaves ENVS PER WORKGROUP ----
// The waves of a workgroup share nothing: each has its own slice of LDS and there is no workgroup barrier, so a wave past the last
// env simply leaves.  The sweep: the env's slots are strided over the lanes, 64 at a time; a lane reads its mover's shape record whole
// and its speed, and the movers that are md_present and not culled are appended to an LDS list (cx, cy, c, s, hl, hw, speed, slot) at
// the ballot's prefix count, so the list is in slot order.  The (sample, mover) pairs p = j * count + i are then strided over the
// lanes in ascending order of their key (j << 16) | slot; a lane's overlap (the header's md_sm_overlap_at) becomes that key, and the
// first round of 64 pairs with any overlap holds the smallest key of all -- the wave stops there and takes the minimum by shuffles,
// so the result does not depend on scheduling.  One lane then runs the header's md_sm_finish: the finite differences, the
// accumulators and the latch.  No atomics, plain vector stores.
//
// THE CULL is conservative.  A mover can overlap the ego at some sample only if the distance of their centres then is at most the
// sum of the half diagonals; each centre moves at most |speed| * J * ttc_dt along a unit vector, so a pair whose centres NOW are
// farther apart than both half diagonals plus (|v_e| + |v_n|) * J * ttc_dt cannot meet.  The bound is taken with a slack of 1 m plus
// 1e-5 of the coordinates' magnitudes -- four orders of magnitude above the float32 rounding of any term of it and of md_obb_obb's
// projections (a few ulp of the coordinates) -- and the test is written so that a NaN or an infinite bound keeps the pair.
constexpr int kSmWaves = 4;

__device__ __forceinline__ bool sm_cannot_meet(const MdShape& me, float vm, const MdShape& o, float vo, float reach) {
    const float dist = md_norm(o.cx - me.cx, o.cy - me.cy);
    const float bound = md_norm(me.hl, me.hw) + md_norm(o.hl, o.hw) + (md_fabs(vm) + md_fabs(vo)) * reach + 1.0f +
                        1.0e-5f * (md_fabs(me.cx) + md_fabs(me.cy) + md_fabs(o.cx) + md_fabs(o.cy));
    return dist > bound;
}

__global__ __launch_bounds__(64 * kSmWaves) void scenario_metrics_kernel(const MdState g, const MdConfig c, const MdScenarioMetrics sm) {
    __shared__ __attribute__((aligned(16))) float l_all[kSmWaves][8 * MD_MAX_CAP];   // 16 KB: check_common holds cap <= MD_MAX_CAP
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int e = blockIdx.x * kSmWaves + wave;
    if (e >= c.n_envs) return;                       // wave-uniform, and the kernel has no workgroup barrier
    float* l_box = l_all[wave];
    const MdState s = md_env_view(&g, &c, e);
    const MdShape me = s.shape[0];
    const float vm = s.dyn[0].speed;
    const int J = sm.ttc_samples;
    int count = 0;
    if (md_present(me.flags)) {                      // wave-uniform
        const float reach = (float)J * sm.ttc_dt;
        for (int n0 = 0; n0 < c.cap; n0 += 64) {     // wave-uniform
            const int n = n0 + lane;
            bool cand = false;
            float4 b0 = make_float4(0.0f, 0.0f, 0.0f, 0.0f), b1 = b0;
            if (n >= 1 && n < c.cap) {
                b0 = *reinterpret_cast<const float4*>(&s.shape[n]);
                b1 = *reinterpret_cast<const float4*>(&s.shape[n].hl);
                const MdShape o = {b0.x, b0.y, b0.z, b0.w, b1.x, b1.y, __float_as_int(b1.z), __float_as_int(b1.w)};
                if (md_present(o.flags)) {
                    b1.z = s.dyn[n].speed;
                    cand = !sm_cannot_meet(me, vm, o, b1.z, reach);
                }
            }
            const unsigned long long mask = __ballot(cand);
            if (cand) {
                const int at = count + __popcll(mask & ((1ull << lane) - 1ull));
                b1.w = __int_as_float(n);
                *reinterpret_cast<float4*>(l_box + 8 * at) = b0;
                *reinterpret_cast<float4*>(l_box + 8 * at + 4) = b1;
            }
            count += __popcll(mask);
        }
    }
    wave_lds_sync();
    int key = MD_SM_NO_HIT;
    const int pairs = (J + 1) * count;               // at most 65 * 127
    for (int p0 = 0; p0 < pairs; p0 += 64) {         // wave-uniform
        const int p = p0 + lane;
        if (p < pairs) {
            const int j = p / count, i = p - j * count;
            const float4 b0 = *reinterpret_cast<const float4*>(l_box + 8 * i);
            const float4 b1 = *reinterpret_cast<const float4*>(l_box + 8 * i + 4);
            const MdShape o = {b0.x, b0.y, b0.z, b0.w, b1.x, b1.y, 0, 0};
            if (md_sm_overlap_at(&me, vm, &o, b1.z, j, sm.ttc_dt)) key = (j << 16) | __float_as_int(b1.w);
        }
        if (__ballot(key != MD_SM_NO_HIT)) break;    // every later pair has a larger key
    }
    for (int off = 32; off >= 1; off >>= 1) {
        const int other = __shfl_xor(key, off, 64);
        key = other < key ? other : key;
    }
    if (lane == 0) md_sm_finish(&g, &c, &sm, e, key);
}

}  // namespace

extern "C" {

__attribute__((visibility("default"))) int md_scenario_metrics(const MdWorld* w, const MdState* s, const MdConfig* c,
                                                              const MdScenarioMetrics* sm, void* stream) {
    NEED(w); NEED(s); NEED(c); NEED(sm);
    TRY(check_struct_size(c));
    TRY(check_arg_size("MdScenarioMetrics", sm->struct_size, sizeof(MdScenarioMetrics)));
    TRY(check_common(w, s, c));
    TRY(check_counts("md_scenario_metrics", {{"ttc_samples", sm->ttc_samples, 0, MD_SM_MAX_TTC_SAMPLES, "MD_SM_MAX_TTC_SAMPLES"}}));
    if (!(sm->ttc_dt > 0.0f) || !(sm->ttc_dt <= 1.0e6f)) {
        snprintf(g_err, sizeof g_err, "md_scenario_metrics: ttc_dt=%g must be positive (and at most 1e6)", (double)sm->ttc_dt);
        return MD_EINVAL;
    }
    if (!(c->dt * (float)c->substeps > 0.0f)) {
        snprintf(g_err, sizeof g_err, "md_scenario_metrics: the step period dt * substeps = %g * %d must be positive", (double)c->dt,
                 c->substeps);
        return MD_EINVAL;
    }
    TRY(check_stride("md_scenario_metrics", sm->out_stride));
    const int row = 4 * (MD_SM_STATE_COLS + MD_SM_EPISODE_COLS);
    if (sm->state_stride < row || sm->state_stride % 16) {
        snprintf(g_err, sizeof g_err, "md_scenario_metrics: state_stride=%d must be a multiple of 16, at least %d", sm->state_stride, row);
        return MD_EINVAL;
    }
    TRY(check_scenario_observer("md_scenario_metrics", c));
    TRY(need_fields(kScenarioMetricsEntry, ALWAYS, w, s, c));
    NEED(sm->step); NEED(sm->step_valid); NEED(sm->ttc_slot); NEED(sm->last_episode); NEED(sm->episodes); NEED(sm->state);
    if (sm->agent_light && sm->light_stride <= 0) {
        snprintf(g_err, sizeof g_err, "md_scenario_metrics: light_stride=%d must be positive with agent_light set", sm->light_stride);
        return MD_EINVAL;
    }
    TRY(check_word_aligned("md_scenario_metrics", "the output arrays of MdScenarioMetrics",
                           {sm->step, sm->step_valid, sm->ttc_slot, sm->last_episode, sm->episodes}));
    if ((uintptr_t)sm->state & 15) {
        snprintf(g_err, sizeof g_err, "md_scenario_metrics: state must be 16-byte aligned");
        return MD_EINVAL;
    }
    hipLaunchKernelGGL(scenario_metrics_kernel, dim3((c->n_envs + kSmWaves - 1) / kSmWaves), dim3(64 * kSmWaves), 0, (hipStream_t)stream,
                       *s, *c, *sm);
    return launch_status();
}

}  // extern "C"
