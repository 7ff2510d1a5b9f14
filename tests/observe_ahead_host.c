/* Host build of the agent's observation evaluated AHEAD, as the lean step kernel does it (csrc/parts/observe.inc: observe_ahead_wave and the
 * hit path of observe_agent_wave1), loaded by tests/test_observe_ahead.py through tests/hostlib.py.  Per case two runs on copies of the
 * same state:
 *   direct  md_observe_ctx from the slot's MdNav, the nine tasks in lock-step, md_observe_combine;
 *   ahead   a copy of the key, then the MdNav's five words POISONED while md_observe_ctx_of and the tasks run (they may read the copy
 *           alone), the 45 words, the key and the hand-over words through a 48-word array laid out like wave 0's scratch, and
 *           md_observe_combine_of from that array.
 * Compiled with gcc -O2 -ffp-contract=off: the header's arithmetic to the last bit. */
#include <string.h>

#include "md_entity.h"

#define EXPORT __attribute__((visibility("default")))

/* the scratch words of the hand-over: ObsAheadWord of csrc/parts/observe.inc */
enum { AH_MARK = 45, AH_LANE = 46, AH_ROAD0 = 47, AH_ROAD1 = 2, AH_CK0 = 3, AH_CK1 = 4,
       AH_VALID = 6, AH_CUR_W = 7, AH_CUR_N = 8, AH_POS_ROAD = 9, AH_FIN_LEN = 12 };

#define HX_OBS_DIM 19
#define HX_OUT_WORDS 40   /* obs 19 | reward | cost | info 8 | flags | done word | steps | done | energy | need_reset | shape flags */

EXPORT int hx_key_words(void) { return MD_OBS_KEY_WORDS; }
EXPORT int hx_out_words(void) { return HX_OUT_WORDS; }

/* 1 iff the key copied from `from` equals the five words of `nav` */
EXPORT int hx_key_same(const MdNav* from, const MdNav* nav) {
    MdObsKey q;
    md_obs_key_of(from, &q);
    return md_obs_key_same(&q, nav);
}

typedef struct HxRun {
    MdShape shape;
    MdDyn dyn;
    MdNav nav;
    MdPid pid;
    MdParam param;
    float action[2], obs[HX_OBS_DIM], info[8], reward, cost;
    uint32_t flags, done_word;
    int32_t need_reset, final_lane;
    MdState s;
} HxRun;

static void hx_config(MdConfig* c, const float* cfg2) {
    memset(c, 0, sizeof *c);
    c->curve_radius_max = cfg2[0];
    c->curve_angle_max = cfg2[1];
    c->obs_dim = HX_OBS_DIM;
    c->agents_per_env = 1;
    c->cap = 1;
    c->total_width = 50.0f;
    c->max_lane_width = 4.5f;
    c->driving_reward = 1.0f;
    c->speed_reward = 0.1f;
    c->use_lateral_reward = 1;
    c->success_reward = 10.0f;
    c->out_of_road_penalty = 5.0f;
    c->crash_vehicle_penalty = 5.0f;
    c->crash_object_penalty = 5.0f;
    c->out_of_road_cost = 1.0f;
    c->crash_vehicle_cost = 1.0f;
    c->crash_object_cost = 1.0f;
    c->crash_vehicle_done = 1;
    c->out_of_route_done = 1;
    c->horizon = 60;
    c->auto_reset = 1;
}

static void hx_run_init(HxRun* r, const MdShape* shape, const MdDyn* dyn, const MdNav* nav, int32_t final_lane, uint32_t flags, int i) {
    memset(r, 0, sizeof *r);
    r->shape = *shape;
    r->dyn = *dyn;
    r->nav = *nav;
    r->final_lane = final_lane;
    r->flags = flags;
    r->param.max_speed_kmh = 80.0f + (float)(i % 40);
    r->pid.energy = 0.25f * (float)(i % 7);
    r->action[0] = (float)((i % 21) - 10) / 10.0f;
    r->action[1] = (float)((i % 13) - 6) / 6.0f;
    r->info[4] = 1.5f;
    r->info[5] = 0.5f;
    r->s.shape = &r->shape;
    r->s.dyn = &r->dyn;
    r->s.nav = &r->nav;
    r->s.pid = &r->pid;
    r->s.param = &r->param;
    r->s.action = r->action;
    r->s.obs = r->obs;
    r->s.step_info = r->info;
    r->s.reward = &r->reward;
    r->s.cost = &r->cost;
    r->s.flags = &r->flags;
    r->s.done_out = (void*)&r->done_word;
    r->s.need_reset = &r->need_reset;
    r->s.final_lane = &r->final_lane;
}

static void hx_run_out(const HxRun* r, uint32_t* out) {
    memcpy(out, r->obs, sizeof r->obs);
    memcpy(out + 19, &r->reward, 4);
    memcpy(out + 20, &r->cost, 4);
    memcpy(out + 21, r->info, sizeof r->info);
    out[29] = r->flags;
    out[30] = r->done_word;
    out[31] = (uint32_t)r->nav.steps;
    out[32] = (uint32_t)r->nav.done;
    memcpy(out + 33, &r->pid.energy, 4);
    out[34] = (uint32_t)r->need_reset;
    out[35] = (uint32_t)r->shape.flags;
}

/* Case i as in tests/observe_host.c (its own little map, one vehicle in slot 0), plus flags[i] = the slot's step flags as the
 * traffic stage left them and reset[i] = the env's just_reset.  words_*: 45 per case, out_*: HX_OUT_WORDS per case. */
EXPORT void hx_ahead_cases(int n, const MdLane* lanes, int lanes_per, const MdRoad* roads, int roads_per, const MdShape* shape,
                           const MdDyn* dyn, const MdNav* nav, const int32_t* final_lane, const float* cfg2, const uint32_t* flags,
                           const int32_t* reset, float* words_direct, float* words_ahead, uint32_t* out_direct, uint32_t* out_ahead,
                           int32_t* valid) {
    for (int i = 0; i < n; ++i) {
        MdConfig c;
        hx_config(&c, cfg2 + 2 * i);
        const MdLane* L = lanes + (size_t)i * lanes_per;
        const MdRoad* R = roads + (size_t)i * roads_per;
        memset(out_direct + (size_t)i * HX_OUT_WORDS, 0, 4 * HX_OUT_WORDS);
        memset(out_ahead + (size_t)i * HX_OUT_WORDS, 0, 4 * HX_OUT_WORDS);
        {
            HxRun r;
            hx_run_init(&r, shape + i, dyn + i, nav + i, final_lane[i], flags[i], i);
            MdObsCtx k;
            float w[48];
            memset(w, 0, sizeof w);
            md_observe_ctx(L, R, &r.s, 0, &k);
            for (int l = 0; l < MD_OBS_LANES; ++l) md_observe_lane(l, &k, &r.s, &c, 0, w);
            memcpy(words_direct + (size_t)i * 45, w, 4 * 45);
            md_observe_combine(&k, &r.s, &c, 0, reset[i], (const float (*)[5])w);
            hx_run_out(&r, out_direct + (size_t)i * HX_OUT_WORDS);
            valid[i] = k.valid;
        }
        {
            HxRun r;
            hx_run_init(&r, shape + i, dyn + i, nav + i, final_lane[i], flags[i], i);
            float w[48];
            int32_t* wi = (int32_t*)w;
            memset(w, 0xff, sizeof w);
            /* the ahead wave: the key read once, everything from the copy */
            MdObsKey q;
            md_obs_key_of(&r.nav, &q);
            const MdNav kept = r.nav;
            r.nav.lane = r.nav.road0 = r.nav.road1 = r.nav.ck0 = r.nav.ck1 = 0x7fffff00;   /* an index that would fault if it were read */
            MdObsCtx k;
            md_observe_ctx_of(L, R, &r.s, 0, &q, &k);
            for (int l = 0; l < MD_OBS_TASKS * 5; ++l) w[l] = 0.0f;
            for (int l = 0; l < MD_OBS_LANES; ++l) md_observe_lane(l, &k, &r.s, &c, 0, w);
            memcpy(words_ahead + (size_t)i * 45, w, 4 * 45);
            wi[AH_LANE] = q.lane;
            wi[AH_ROAD0] = q.road0;
            wi[AH_ROAD1] = q.road1;
            wi[AH_CK0] = q.ck0;
            wi[AH_CK1] = q.ck1;
            wi[AH_VALID] = k.valid;
            w[AH_CUR_W] = k.cur_w;
            w[AH_CUR_N] = k.cur_n;
            w[AH_POS_ROAD] = k.positive_road;
            w[AH_FIN_LEN] = k.fin->length;
            wi[AH_MARK] = 1;
            r.nav = kept;
            /* wave 0: the stored key against the committed words, then the combine from the array alone */
            const MdObsKey stored = {wi[AH_LANE], wi[AH_ROAD0], wi[AH_ROAD1], wi[AH_CK0], wi[AH_CK1]};
            if (wi[AH_MARK] && md_obs_key_same(&stored, &r.nav)) {
                const MdObsHand h = {wi[AH_VALID], w[AH_CUR_W], w[AH_CUR_N], w[AH_POS_ROAD], 0, &w[AH_FIN_LEN], 0};
                md_observe_combine_of(&h, &r.s, &c, 0, reset[i], (const float (*)[5])w);
                hx_run_out(&r, out_ahead + (size_t)i * HX_OUT_WORDS);
            }
        }
    }
}
