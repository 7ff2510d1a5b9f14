/* Host build of include/md_ai_protect.h (AIProtectPolicy's saver and takeover flags), loaded by tests/ai_protect_host.py.  Compiled
 * with gcc -O2 -ffp-contract=off like tests/expert_host.c: the rule is + - * /, md_fabs, md_min and comparisons, so its results
 * are the md_ai_protect kernel's to the last bit. */
#include <string.h>

#include "md_entity.h"
#include "md_ai_protect.h"

#define EXPORT __attribute__((visibility("default")))

EXPORT float hx_heading_diff(const MdLane* lanes, int lane, float x, float y, float hc, float hs) {
    return md_ai_protect_heading_diff(lanes, lane, x, y, hc, hs);
}

EXPORT void hx_windows(const float* cloud, int n, float* lat_min, float* lon_min) { md_ai_protect_windows(cloud, n, lat_min, lon_min); }

/* n independent calls of AIProtectPolicy.act: raw / sv [n][2], in [n], save_level / expert_takeover [n]; takeover [n] in and out */
EXPORT void hx_act(int n, const float* raw, const float* sv, const MdProtectIn* in, const float* save_level, const unsigned char* expert_takeover,
                   unsigned char* takeover, float* applied, unsigned char* flags) {
    for (int i = 0; i < n; ++i)
        flags[i] = (unsigned char)md_ai_protect_act(raw + 2 * i, sv + 2 * i, in + i, save_level[i], expert_takeover[i], takeover + i, applied + 2 * i);
}

/* One md_ai_protect launch restated: every env of a batch on the state and observation the previous step left (global arrays,
 * cap slots per env, one agent, obs rows of c->obs_dim floats).  sv [E][2]: the expert's draws. */
EXPORT void hx_batch(const MdLane* lanes, const int32_t* lane_off, const int32_t* env_map, const MdShape* shape, const MdDyn* dyn,
                     const MdParam* param, const MdNav* nav, const float* obs, const int32_t* need_reset, const MdConfig* c,
                     const float* raw, const float* sv, float save_level, unsigned char* takeover, unsigned char* expert_takeover,
                     float* applied, unsigned char* flags, MdProtectIn* in_out) {
    for (int e = 0; e < c->n_envs; ++e) {
        const size_t b = (size_t)e * (size_t)c->cap;
        if (need_reset[e]) {
            flags[e] = (unsigned char)md_ai_protect_reset(raw + 2 * e, takeover + e, expert_takeover + e, applied + 2 * e);
            continue;
        }
        MdState s;
        memset(&s, 0, sizeof s);
        s.shape = (MdShape*)shape + b;
        s.dyn = (MdDyn*)dyn + b;
        s.param = (MdParam*)param + b;
        s.nav = (MdNav*)nav + b;
        s.obs = (float*)obs + (size_t)e * c->obs_dim;
        MdProtectIn in;
        md_ai_protect_inputs(lanes + lane_off[env_map[e]], &s, c, &in);
        if (in_out) in_out[e] = in;
        flags[e] = (unsigned char)md_ai_protect_act(raw + 2 * e, sv + 2 * e, &in, save_level, expert_takeover[e], takeover + e, applied + 2 * e);
    }
}
