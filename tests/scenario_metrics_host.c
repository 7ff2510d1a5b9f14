/* Host build of include/md_scenario_metrics.h (the closed-loop driving metrics of scenario mode), loaded by the tests through
 * tests/hostlib.py: one md_scenario_metrics launch restated as a plain loop over the envs (all pointers host arrays), and
 * sizeof(MdScenarioMetrics), two of its offsets and the ceilings as the C compiler sees them. */
#include "md_scenario_metrics.h"

#define EXPORT __attribute__((visibility("default")))

EXPORT int hx_sizeof_scenario_metrics(void) { return (int)sizeof(MdScenarioMetrics); }
EXPORT int hx_sm_offsetof(int which) {
    const int at[4] = {(int)offsetof(MdScenarioMetrics, max_lon_accel), (int)offsetof(MdScenarioMetrics, out_stride),
                       (int)offsetof(MdScenarioMetrics, agent_light), (int)offsetof(MdScenarioMetrics, state)};
    return which >= 0 && which < 4 ? at[which] : -1;
}
EXPORT int hx_sm_limit(int which) {
    const int limits[4] = {MD_SM_MAX_TTC_SAMPLES, MD_SM_STEP_COLS, MD_SM_EPISODE_COLS, MD_SM_STATE_COLS};
    return which >= 0 && which < 4 ? limits[which] : -1;
}

/* md_scenario_metrics without the launch */
EXPORT int hx_scenario_metrics(const MdWorld* w, const MdState* s, const MdConfig* c, const MdScenarioMetrics* sm) {
    for (int e = 0; e < c->n_envs; ++e) md_scenario_metrics_env(w, s, c, sm, e);
    return 0;
}
