/* Host build of include/md_traffic_lights.h (the traffic lights of scenario mode), loaded by the tests through tests/hostlib.py: one
 * md_traffic_lights launch restated as a plain loop over the envs (all pointers host arrays), and sizeof(MdTrafficLights), the
 * ceilings and the wall's constants as the C compiler sees them. */
#include "md_traffic_lights.h"

#define EXPORT __attribute__((visibility("default")))

EXPORT int hx_sizeof_traffic_lights(void) { return (int)sizeof(MdTrafficLights); }
EXPORT int hx_offsetof_tl_tables(void) { return (int)offsetof(MdTrafficLights, tl_off); }
EXPORT int hx_tl_limit(int which) {
    const int limits[2] = {MD_TL_MAX_LIGHTS, MD_TL_MAX_SCENE_LIGHTS};
    return which >= 0 && which < 2 ? limits[which] : -1;
}
EXPORT float hx_tl_constant(int which) {
    const float k[3] = {MD_TL_AIR_WALL_LENGTH, MD_TL_LANE_WIDTH, MD_TL_PLACE_LONGITUDE};
    return which >= 0 && which < 3 ? k[which] : -1.0f;
}

/* md_traffic_lights without the launch */
EXPORT int hx_traffic_lights(const MdWorld* w, const MdState* s, const MdConfig* c, const MdTrafficLights* tl) {
    for (int e = 0; e < c->n_envs; ++e) md_traffic_lights_env(w, s, c, tl, e);
    return 0;
}
