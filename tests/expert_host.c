/* Host build of include/md_expert.h (the PPO expert's MLP, tanh, exp), loaded by tests/expert_host.py.  Compiled with
 * gcc -O2 -ffp-contract=off: the same k-ordered fmaf chains as the md_expert kernel, so its results are the kernel's bits. */
#include "md_expert.h"

#define EXPORT __attribute__((visibility("default")))

/* raw 275-vectors (the env's obs with the others block) -> corrected obs + mean | log_std, n rows */
EXPORT void hx_expert(const float* w, const float* raw, int n, float* corrected, float* out4) {
    for (int i = 0; i < n; ++i) {
        float* x = corrected + (long)i * MD_EXPERT_IN;
        for (int k = 0; k < MD_EXPERT_IN; ++k) x[k] = raw[(long)i * MD_EXPERT_IN + k];
        md_expert_correct(x);
        md_expert_mlp(w, x, out4 + 4L * i);
    }
}

/* already corrected 275-vectors -> mean | log_std */
EXPORT void hx_mlp(const float* w, const float* x, int n, float* out4) {
    for (int i = 0; i < n; ++i) md_expert_mlp(w, x + (long)i * MD_EXPERT_IN, out4 + 4L * i);
}

EXPORT void hx_sample(const float* out4, const float* noise, int n, float* action) {
    for (int i = 0; i < n; ++i)
        for (int q = 0; q < 2; ++q) action[2 * i + q] = md_expert_sample(out4[4 * i + q], out4[4 * i + 2 + q], noise[2 * i + q]);
}

EXPORT void hx_tanh(const float* x, int n, float* y) {
    for (int i = 0; i < n; ++i) y[i] = md_tanh(x[i]);
}

EXPORT void hx_exp(const float* x, int n, float* y) {
    for (int i = 0; i < n; ++i) y[i] = md_exp(x[i]);
}

EXPORT int hx_widx(int K, int k, int n) { return md_expert_widx(K, k, n); }
