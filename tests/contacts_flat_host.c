/* Host build of md_flat_cell_item (include/md_geom.h), the index mapping of the lean step kernel's flat pass over the grid cells
 * under the agent's chassis (csrc/parts/contacts.inc: contacts_vehicle, kFlat), loaded by tests/test_contacts_flat_host.py through
 * tests/hostlib.py.  The same text the kernel compiles. */
#include <stddef.h>

#include "md_geom.h"

#define EXPORT __attribute__((visibility("default")))

/* cases of four range lengths each; per case the walk flat = 0 .. total - 1, (cell, offset) pairs into out[2 * k], at most `room`
 * pairs per case -> pairs[i] = the pairs written; past[i] = what the helper answers at flat = total, before[i] at flat = -1 */
EXPORT void hx_flat_walk(int n, const int* len4, int room, int* out, int* pairs, int* past, int* before) {
    for (int i = 0; i < n; ++i) {
        const int* L = len4 + 4 * i;
        const int total = L[0] + L[1] + L[2] + L[3];
        int k = 0, off = 0;
        for (int flat = 0; flat < total && k < room; ++flat, ++k) {
            out[((size_t)i * room + k) * 2] = md_flat_cell_item(L[0], L[1], L[2], L[3], flat, &off);
            out[((size_t)i * room + k) * 2 + 1] = off;
        }
        pairs[i] = k;
        past[i] = md_flat_cell_item(L[0], L[1], L[2], L[3], total, &off);
        before[i] = md_flat_cell_item(L[0], L[1], L[2], L[3], -1, &off);
    }
}
