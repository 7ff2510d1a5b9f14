// parts/traffic_lights.inc -- part of mdstep.hip, included there and not compiled on its own.
// Provides: kTlWaves, the LDS layout traffic_lights_lds and traffic_lights_kernel (include/md_traffic_lights.h), and the entry point
// md_traffic_lights with its argument checks.
// Relies on: mdstep.hip (align_up, wave_lds_sync), entry_checks, vector_obs.inc (vo_key).

namespace {

// ---- the traffic lights of scenario mode (include/md_traffic_lights.h): ONE WAVE PER ENV, kTlWaves ENVS PER WORKGROUP ----
// The waves of a workgroup share nothing: each has its own slice of LDS and there is no workgroup barrier, so a wave past the last
// env simply leaves.  The scene's lights are strided over the lanes, 64 at a time: a lane reads its light's box and info records
// whole, raises the header's md_tl_light_bits into its own word (OR-ed over the wave by shuffles at the end) and computes the
// header's md_tl_d2.  The candidates of a round are appended to an LDS list (ordinal, d2) at the ballot's prefix count; a
// candidate's rank is the number of candidates with a smaller key (float bits of d2) << 32 | ordinal (d2 >= 0: the key orders as an
// unsigned integer, the ordinal breaks ties -- md_vo_before's order), counted over the list only; ranks below L go to a taken list
// and lane r writes row r with the header's md_tl_row.  No atomics, plain vector stores; the result does not depend on scheduling.
constexpr int kTlWaves = 4;
struct TrafficLightsLds { uint32_t taken, at, d2, per_wave, bytes; };
__host__ __device__ constexpr TrafficLightsLds traffic_lights_lds(int max_scene_lights) {
    const uint32_t n = (uint32_t)(max_scene_lights > 0 ? max_scene_lights : 0);
    const uint32_t at = 4u * MD_TL_MAX_LIGHTS, d2 = at + 4u * n, per_wave = align_up(d2 + 4u * n, 16);
    return TrafficLightsLds{0u, at, d2, per_wave, per_wave * (uint32_t)kTlWaves};
}

__global__ __launch_bounds__(64 * kTlWaves) void traffic_lights_kernel(const MdState g, const MdConfig c, const MdTrafficLights tl) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int e = blockIdx.x * kTlWaves + wave;
    if (e >= c.n_envs) return;                       // wave-uniform, and the kernel has no workgroup barrier
    const TrafficLightsLds LD = traffic_lights_lds(tl.max_scene_lights);
    unsigned char* mine = smem + (size_t)wave * LD.per_wave;
    int* l_taken = reinterpret_cast<int*>(mine + LD.taken);
    int* l_at = reinterpret_cast<int*>(mine + LD.at);
    float* l_d2 = reinterpret_cast<float*>(mine + LD.d2);
    const MdState s = md_env_view(&g, &c, e);
    const int t = md_rd_clock(&g, &c, e, &s.nav[0]);
    const MdShape me = s.shape[0];
    const bool observer = md_present(me.flags);
    const MdVoEgo ego = {me.cx, me.cy, me.c, me.s};
    const MdTlOut o = md_tl_out_of(&tl, e);
    int p0;
    const int in_scene = md_tl_scene(&tl, md_scene(&s, e), &p0);      // at most max_scene_lights: the lists hold that many
    const int n = observer ? in_scene : 0;
    const int L = tl.num_lights;
    const float radius2 = tl.radius * tl.radius;
    if (lane < MD_TL_MAX_LIGHTS) l_taken[lane] = -1;
    int bits = 0, count = 0;
    for (int q0 = 0; q0 < n; q0 += 64) {             // wave-uniform
        const int q = q0 + lane;
        bool cand = false;
        float d2 = 0.0f;
        if (q < n) {
            const size_t at = (size_t)(p0 + q);
            const float4 b0 = *reinterpret_cast<const float4*>(tl.tl_box + 8 * at);
            const float4 b1 = *reinterpret_cast<const float4*>(tl.tl_box + 8 * at + 4);
            const int4 i0 = *reinterpret_cast<const int4*>(tl.tl_info + 4 * at);
            const float box[8] = {b0.x, b0.y, b0.z, b0.w, b1.x, b1.y, b1.z, b1.w};
            const int32_t info[4] = {i0.x, i0.y, i0.z, i0.w};
            bits |= md_tl_light_bits(&tl, &me, box, info, t);
            d2 = md_tl_d2(box, me.cx, me.cy);
            cand = L > 0 && d2 <= radius2;
        }
        const unsigned long long mask = __ballot(cand);
        if (cand) {
            const int slot = count + __popcll(mask & ((1ull << lane) - 1ull));
            l_at[slot] = q;
            l_d2[slot] = d2;
        }
        count += __popcll(mask);
    }
    for (int off = 32; off >= 1; off >>= 1) bits |= __shfl_xor(bits, off, 64);
    if (lane == 0) o.agent_light[0] = (uint8_t)bits;
    if (L <= 0) return;                              // wave-uniform
    wave_lds_sync();
    for (int i = lane; i < count; i += 64) {
        const unsigned long long key = vo_key(l_d2[i], tl.tl_info[4 * (size_t)(p0 + l_at[i]) + 2]);
        int rank = 0;
        for (int j = 0; j < count && rank < L; ++j) rank += vo_key(l_d2[j], tl.tl_info[4 * (size_t)(p0 + l_at[j]) + 2]) < key;
        if (rank < L) l_taken[rank] = i;
    }
    wave_lds_sync();
    if (lane < L) {
        const int k = l_taken[lane];
        const size_t at = (size_t)(p0 + (k >= 0 ? l_at[k] : 0));
        md_tl_row(&tl, &o, lane, k >= 0 ? tl.tl_box + 8 * at : nullptr, k >= 0 ? tl.tl_info + 4 * at : nullptr, t, k >= 0 ? l_d2[k] : 0.0f,
                  &ego);
    }
}

}  // namespace

extern "C" {

__attribute__((visibility("default"))) int md_traffic_lights(const MdWorld* w, const MdState* s, const MdConfig* c, const MdTrafficLights* tl,
                                                            void* stream) {
    NEED(w); NEED(s); NEED(c); NEED(tl);
    TRY(check_struct_size(c));
    TRY(check_arg_size("MdTrafficLights", tl->struct_size, sizeof(MdTrafficLights)));
    TRY(check_common(w, s, c));
    TRY(check_counts("md_traffic_lights", {{"num_lights", tl->num_lights, 0, MD_TL_MAX_LIGHTS, "MD_TL_MAX_LIGHTS"},
                                           {"max_scene_lights", tl->max_scene_lights, 0, MD_TL_MAX_SCENE_LIGHTS, "MD_TL_MAX_SCENE_LIGHTS"}}));
    TRY(check_lengths("md_traffic_lights", {{"radius", tl->radius}}));
    TRY(check_stride("md_traffic_lights", tl->out_stride));
    TRY(check_scenario_observer("md_traffic_lights", c));
    TRY(need_fields(kTrafficLightsEntry, ALWAYS, w, s, c));
    NEED(tl->tl_off); NEED(tl->tl_box); NEED(tl->tl_info); NEED(tl->tl_status); NEED(tl->agent_light);
    if (tl->num_lights > 0) { NEED(tl->lights); NEED(tl->lights_mask); NEED(tl->lights_index); }
    TRY(check_word_aligned("md_traffic_lights", "the float and int32 arrays of MdTrafficLights", {tl->tl_off, tl->lights, tl->lights_index}));
    if (((uintptr_t)tl->tl_box & 15) || ((uintptr_t)tl->tl_info & 15)) {
        snprintf(g_err, sizeof g_err, "md_traffic_lights: %s must be 16-byte aligned (its records are read whole)",
                 ((uintptr_t)tl->tl_box & 15) ? "tl_box" : "tl_info");
        return MD_EINVAL;
    }
    const size_t lds = traffic_lights_lds(tl->max_scene_lights).bytes;     // 33280 B at the ceiling: inside a workgroup's 64 KB
    hipLaunchKernelGGL(traffic_lights_kernel, dim3((c->n_envs + kTlWaves - 1) / kTlWaves), dim3(64 * kTlWaves), lds, (hipStream_t)stream,
                       *s, *c, *tl);
    return launch_status();
}

}  // extern "C"
