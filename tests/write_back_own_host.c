/* Host build of the owner rule of the lean kernels' per-wave write-back (include/md_write_back_own.h), loaded by
 * tests/test_write_back_own_host.py through tests/hostlib.py.  The same text the library compiles. */
#include "md_write_back_own.h"

#define EXPORT __attribute__((visibility("default")))

/* n rows of (shape flags, removed in this step) -> out[4 * i] = md_wb_owner, [4 * i + 1] = md_wb_dirty, [4 * i + 2] = md_drives,
 * [4 * i + 3] = md_moves.  The slot is an agent's iff its flags say so, as the kernel asks. */
EXPORT void hx_wb_owner(int n, const int* rows, int* out) {
    for (int i = 0; i < n; ++i) {
        const int flags = rows[2 * i], removed = rows[2 * i + 1];
        out[4 * i] = md_wb_owner(flags, flags & MD_F_AGENT, removed);
        out[4 * i + 1] = md_wb_dirty(flags, removed);
        out[4 * i + 2] = md_drives(flags);
        out[4 * i + 3] = md_moves(flags);
    }
}

EXPORT void hx_wb_names(int* out) {
    out[0] = MD_WB_NOBODY;
    out[1] = MD_WB_WAVE0;
    out[2] = MD_WB_IDM;
    out[3] = MD_WB_REST;
}
