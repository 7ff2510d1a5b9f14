// parts/expert.inc -- part of mdstep.hip, included there and not compiled on its own.
// Provides: kExpM and the expert's tiles, expert_kernel (include/md_expert.h), expert_sense_kernel (include/md_expert_sense.h)
// and ai_protect_kernel (include/md_ai_protect.h),
// and their entry points md_expert, md_ai_protect and md_expert_sense (check_expert_config) with their argument checks.
// Relies on: mdstep.hip (wave_lds_sync, lidar_item), entry_checks.

namespace {

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

}  // namespace

extern "C" {

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

}  // extern "C"
