/* Host build of the scenario walk of include/md_scenario.h (md_walk_scene), loaded by tests/walk_host.py: the schedule md_swap_draw
 * runs on the device, for the oracle's host-side swap and the schedule tests. */
#include <stddef.h>
#include <string.h>

#include "md_scenario.h"

#define EXPORT __attribute__((visibility("default")))

/* out[i] = md_walk_scene(walk, e[i], ep[i]) for an MdState.walk with the given fields */
EXPORT void hx_walk_scene(int n_scenes, int walk, int stride, int offset, uint32_t seed, const int* e, const int* ep, int n, int* out) {
    MdWalk c = {0};
    c.n_scenes = n_scenes;
    c.mode = walk;
    c.stride = stride;
    c.offset = offset;
    c.seed = seed;
    for (int i = 0; i < n; ++i) out[i] = md_walk_scene(&c, e[i], ep[i]);
}
