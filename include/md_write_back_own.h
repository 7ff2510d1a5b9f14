/*
 * md_write_back_own.h -- who stores a slot of an env at the end of a step of the lean non-staged workgroup kernels (csrc/mdstep.hip:
 * env_kernel with parts/lean_view.inc, MD_WRITE_BACK_OWN).  Plain C, so the CPU tests read the same text
 * (tests/write_back_own_host.c).
 *
 * Those kernels no longer meet at a last barrier to write the dirty slots back: each wave stores the slots that IT was the last
 * to touch, straight from the LDS image, and leaves.  Which wave that is follows from the stage structure alone:
 *   - an agent's slot is final when wave 0's observe returns (it writes the slot's flag word, nav.steps / done, pid.energy and the
 *     SPAWNED bit);
 *   - a driving traffic slot is final when the IDM wave that plans it returns (the slot's action, nav and pid; other vehicles'
 *     IDM only read it);
 *   - every other dirty slot -- removed in this step, or a walking participant -- is final behind the traffic stage's barrier: the
 *     rest pass of the last wave.
 * "Dirty" is md_wb_dirty below, what the write-back behind the last barrier stores (and every other step kernel still does).
 */
#ifndef MD_WRITE_BACK_OWN_H
#define MD_WRITE_BACK_OWN_H

#include "md_entity.h"

enum { MD_WB_NOBODY = 0, MD_WB_WAVE0 = 1, MD_WB_IDM = 2, MD_WB_REST = 3 };

/* the slot's LDS image may differ from HBM: it moves, or the traffic stage removed it in this step */
MD_HD int md_wb_dirty(int flags, int removed) { return md_moves(flags) || removed; }

/* flags: the slot's shape flags behind the traffic stage's barrier (an agent's: behind its observe, which changes none of the
 * bits read here but SPAWNED, which nothing here reads); is_agent: its MD_F_AGENT bit; removed: the traffic stage's mark.
 * A driving traffic slot is asked first: its `removed` word is not written by any stage (only an agent's contacts and a removal
 * write it), and whatever it holds the slot belongs to the wave that is still planning it. */
MD_HD int md_wb_owner(int flags, int is_agent, int removed) {
    if (!is_agent && md_drives(flags)) return MD_WB_IDM;   /* exactly the slots the IDM waves' rank walk deals out */
    if (!md_wb_dirty(flags, removed)) return MD_WB_NOBODY;
    return is_agent ? MD_WB_WAVE0 : MD_WB_REST;
}

#endif
