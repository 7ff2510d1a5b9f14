/* Host driver of tests/test_lidar_span_host.py: md_lidar_beam_span (include/md_geom.h, the text the lean step kernels compile)
 * against md_ray_shape over every beam of the fan, the beams built as lidar_item builds them.  TEST INFRASTRUCTURE. */
#include <stddef.h>

#include "md_geom.h"

#define EXPORT __attribute__((visibility("default")))

/* n cases: ego[i] the observer's record, body[i] the mover's, range[i], the fan of case i = beams + 2 * beam_off[i], n_beams[i]
 * beams of (cos, sin).  Out per case: first / count = the span, hits = beams with md_ray_shape < 1, bad = those of them outside
 * the span (the property: 0), first_bad = the first such beam or -1. */
EXPORT void hx_lidar_span(int n, const MdShape* ego, const MdShape* body, const float* range, const float* beams, const int* beam_off,
                   const int* n_beams, int* first, int* count, int* hits, int* bad, int* first_bad) {
    for (int i = 0; i < n; ++i) {
        const MdShape* me = &ego[i];
        const MdShape* o = &body[i];
        const int nb = n_beams[i];
        const float* cs = beams + 2 * (long)beam_off[i];
        md_lidar_beam_span(me->cx, me->cy, me->c, me->s, range[i], nb, o, &first[i], &count[i]);
        hits[i] = 0;
        bad[i] = 0;
        first_bad[i] = -1;
        for (int b = 0; b < nb; ++b) {
            const float bc = cs[2 * b], bs = cs[2 * b + 1];
            const float dirx = (bc * me->c - bs * me->s) * range[i];
            const float diry = (bs * me->c + bc * me->s) * range[i];
            const float t = md_ray_shape(me->cx, me->cy, dirx, diry, o->cx, o->cy, o->c, o->s, o->hl, o->hw, o->flags & MD_KIND_MASK);
            if (!(t < 1.0f)) continue;
            ++hits[i];
            int k = b - first[i];
            if (k < 0) k += nb;
            if (k >= count[i]) {
                if (first_bad[i] < 0) first_bad[i] = b;
                ++bad[i];
            }
        }
    }
}
