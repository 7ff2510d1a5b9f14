/*
 * md_expert.h -- the reference's PPO driving expert (metadrive/examples/ppo_expert/numpy_expert.py:34-77): a
 * 275 -> 256 -> 256 -> 4 tanh MLP on the LidarStateObservation of the agent, shared by the HIP kernel (md_expert in
 * csrc/parts/expert.inc) and its host restatement (tests), so that the GPU result is reproducible on the host to the last bit.
 *
 * Reproducibility contract (what both builds compute, output element by output element):
 *   - every pre-activation is ONE k-ordered fmaf chain that starts from the bias:
 *         acc = b[n];  for k = 0 .. K_pad-1:  acc = fmaf(x[k], W[k][n], acc)
 *     with K padded by zeros to a multiple of 16 (275 -> 288; the padded x and W entries are both 0, so the host and
 *     the device take the same extra steps).  v_mfma_f32_16x16x4_f32 is bit for bit such a chain over its 4 k, so
 *     chaining its accumulator over the k-steps in order gives exactly this.  No split-K, no atomics: an env's bits
 *     depend on nothing but its own input row.
 *   - tanh and exp are md_tanh / md_exp below (+ - * / only), not the device library's, which does not round like glibc.
 *
 * Packed weights (one fp32 buffer, built by metadrive_ped_amd/expert.py:pack_expert_weights): each weight matrix W [K][N]
 * is stored in the MFMA B-operand order of the kernel, 16x16 tiles of (k, n) as
 *     tile (n / 16, k / 16) of 64 lanes x 4 floats;  lane = ((k % 16) % 4) * 16 + n % 16,  float = (k % 16) / 4
 * so that one 16-byte load per lane feeds four consecutive 16x16x4 k-steps (md_expert_widx).  Layer 3 (N = 4) is padded
 * to N = 16 with zero columns.  Order: W1 | b1 | W2 | b2 | W3 | b3 (b3 padded to 16).
 */
#ifndef MD_EXPERT_H
#define MD_EXPERT_H

#include <stddef.h>

#include "md_math.h"
#include "mdstep.h"

#define MD_EXPERT_IN 275          /* state 19 + others 4 x 4 + cloud 240 (numpy_expert.py:64) */
#define MD_EXPERT_IN_PAD 288      /* K of layer 1, padded to a multiple of 16 */
#define MD_EXPERT_HID 256
#define MD_EXPERT_OUT 4           /* mean (2) | log_std (2) */
#define MD_EXPERT_OUT_PAD 16      /* N of layer 3, padded to one MFMA tile */
#define MD_EXPERT_STATE 19        /* dims of the state block, first in both the env's obs and the expert's */
#define MD_EXPERT_OTHERS 4        /* num_others of the expert's lidar */

#define MD_EXPERT_W1 0
#define MD_EXPERT_B1 (MD_EXPERT_W1 + MD_EXPERT_IN_PAD * MD_EXPERT_HID)
#define MD_EXPERT_W2 (MD_EXPERT_B1 + MD_EXPERT_HID)
#define MD_EXPERT_B2 (MD_EXPERT_W2 + MD_EXPERT_HID * MD_EXPERT_HID)
#define MD_EXPERT_W3 (MD_EXPERT_B2 + MD_EXPERT_HID)
#define MD_EXPERT_B3 (MD_EXPERT_W3 + MD_EXPERT_HID * MD_EXPERT_OUT_PAD)
#define MD_EXPERT_NW (MD_EXPERT_B3 + MD_EXPERT_OUT_PAD)   /* floats in the packed buffer */

/* offset of W[k][n] inside a packed matrix of K rows (K a multiple of 16) */
MD_HD int md_expert_widx(int K, int k, int n) {
    const int tile = (n >> 4) * (K >> 4) + (k >> 4);
    const int kk = k & 15;
    return tile * 256 + ((kk & 3) * 16 + (n & 15)) * 4 + (kk >> 2);
}

/* tanh from md_exp: 1 - 2 / (exp(2x) + 1), odd-symmetric; |x| >= 9 is +-1 (tanh(9) rounds to 1 in float32). */
MD_HD float md_tanh(float x) {
    const float ax = md_fabs(x);
    if (!(ax < 9.0f)) return x < 0.0f ? -1.0f : (x > 0.0f ? 1.0f : x);   /* NaN passes through */
    float t;
    if (ax < 0.625f) {
        /* Cephes tanhf kernel: x + x^3 P(x^2) */
        const float z = ax * ax;
        t = ((((-5.70498872745e-3f * z + 2.06390887954e-2f) * z - 5.37397155531e-2f) * z + 1.33314422036e-1f) * z
             - 3.33332819422e-1f) * z * ax + ax;
    } else {
        t = 1.0f - 2.0f / (md_exp(ax + ax) + 1.0f);
    }
    return x < 0.0f ? -t : t;
}

/* obs_correction (numpy_expert.py:30-34) */
MD_HD void md_expert_correct(float* obs) {
    obs[15] = 1.0f - obs[15];
    obs[10] = 1.0f - obs[10];
}

/* one pre-activation: the k-ordered chain of the contract (host restatement; the kernel runs it on the matrix cores) */
MD_HD float md_expert_dot(const float* W, int K, const float* x, float bias, int n) {
    float acc = bias;
    for (int k = 0; k < K; ++k) acc = __builtin_fmaf(x[k], W[md_expert_widx(K, k, n)], acc);
    return acc;
}

/* action = mean + exp(log_std) * noise (np.random.normal(mean, std), numpy_expert.py:72-73); noise = N(0, 1) */
MD_HD float md_expert_sample(float mean, float log_std, float noise) { return mean + md_exp(log_std) * noise; }

/* The whole MLP on one corrected 275-vector `x` (host form): out[0:2] = mean, out[2:4] = log_std. */
MD_HD void md_expert_mlp(const float* w, const float* x, float* out) {
    float xin[MD_EXPERT_IN_PAD], h1[MD_EXPERT_HID], h2[MD_EXPERT_HID];
    for (int k = 0; k < MD_EXPERT_IN_PAD; ++k) xin[k] = k < MD_EXPERT_IN ? x[k] : 0.0f;
    for (int n = 0; n < MD_EXPERT_HID; ++n)
        h1[n] = md_tanh(md_expert_dot(w + MD_EXPERT_W1, MD_EXPERT_IN_PAD, xin, w[MD_EXPERT_B1 + n], n));
    for (int n = 0; n < MD_EXPERT_HID; ++n)
        h2[n] = md_tanh(md_expert_dot(w + MD_EXPERT_W2, MD_EXPERT_HID, h1, w[MD_EXPERT_B2 + n], n));
    for (int n = 0; n < MD_EXPERT_OUT; ++n)
        out[n] = md_expert_dot(w + MD_EXPERT_W3, MD_EXPERT_HID, h2, w[MD_EXPERT_B3 + n], n);
}

/* C-ABI entry point (libmdstep.so; declared here rather than in mdstep.h, which the CPU oracle is built from).
 * One launch over all envs of a single-agent batch whose observation is the expert's minus the "others" block: lidar
 * 240 beams / 50 m, num_others = 0, side and lane-line detectors off, random_agent_model off (obs_dim 259), with the
 * detected sets tracked (MdState.detected).  For every env e:
 *   x = obs[e][0:19] | md_others_block(num_others = 4) | obs[e][19:259]  -> corrected (md_expert_correct) -> MLP
 *   action_out[e][0:2] = mean + exp(log_std) * noise[e][0:2]   (noise = NULL: mean)
 *   mlp_out[e][0:4]    = mean | log_std                        (may be NULL)
 *   obs_out[e][0:275]  = the corrected x                       (may be NULL)
 * weights: MD_EXPERT_NW packed floats (16-byte aligned device buffer).  Returns MD_OK or an error (md_last_error). */
#ifdef __cplusplus
extern "C" {
#endif
int md_expert(const MdWorld* w, const MdState* s, const MdConfig* c, const float* weights, const float* noise, float* action_out,
              float* mlp_out, float* obs_out, void* stream);
#ifdef __cplusplus
}
#endif

#endif /* MD_EXPERT_H */
