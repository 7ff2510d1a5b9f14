/*
 * md_lean_pins.h -- what a lean launch of md_step pins: ONE list for the launch predicate (host) and for the kernels that fold it
 * (csrc/mdstep.hip: variant<PH_ALL>(), lean_pins_fold, lean_size_pins_fold).  Plain C, so the CPU tests read the same text
 * (tests/lean_pins_host.c).
 *
 * A requirement taken out of a list is no longer assumed by any kernel; only fields the predicate itself tests belong here, a field
 * that merely happens to be unused in these configs does not.
 */
#ifndef MD_LEAN_PINS_H
#define MD_LEAN_PINS_H

#include "mdstep.h"
#include "md_math.h"

/* The lean kernels of md_step -- env_kernel<PH_ALL, *, false, false> and wave_step_kernel<false> -- are launched only while every
 * field listed here has its pinned value.
 *   ZERO(int32 MdConfig field): the field is 0;  NUL(MdState pointer): the pointer is null */
#define MD_LEAN_PINS(ZERO, NUL)                                                                                              \
    ZERO(is_multi_agent) /* the multi-agent envs have their own variant (MULTI) */                                             \
    ZERO(traffic_mode)   /* trigger mode; respawn / hybrid / replay: the RESPAWN variant (scenario mode: its own kernel) */    \
    ZERO(agent_idm)      /* the caller's actions; IDMPolicy / LaneChangePolicy agents: the RESPAWN variant */                  \
    ZERO(num_others)     /* the `others` block needs the detected sets */                                                     \
    NUL(detected)        /* tracked by the RESPAWN / MULTI variants only */

/* The size pins: a lean batch that holds them too takes the NARROW instantiation of the non-staged env_kernel, in which a slot
 * mask is one 64-bit word, a slot scan one pass, a per-thread loop one `if`, and the agent is slot 0.  A lean batch that does not
 * (capacity 65..128: the accident scenes; more than one agent per env through the C ABI) runs the lean kernel as before.
 *   EQUALS(int32 MdConfig field, value);  AT_MOST(int32 MdConfig field, bound) */
#define MD_LEAN_SIZE_PINS(EQUALS, AT_MOST)                                                                                   \
    EQUALS(agents_per_env, 1) /* one agent: slot 0 */                                                                          \
    AT_MOST(cap, 64)          /* every slot of an env in one wave's lanes, one mask word */

MD_HD int md_lean_pins_hold(const MdState* s, const MdConfig* c) {
    int ok = 1;
#define MD_PIN_ZERO(f) ok = ok && c->f == 0;
#define MD_PIN_NUL(p) ok = ok && s->p == 0;
    MD_LEAN_PINS(MD_PIN_ZERO, MD_PIN_NUL)
#undef MD_PIN_ZERO
#undef MD_PIN_NUL
    return ok;
}

MD_HD int md_lean_size_pins_hold(const MdConfig* c) {
    int ok = 1;
#define MD_PIN_EQUALS(f, v) ok = ok && c->f == (v);
#define MD_PIN_AT_MOST(f, v) ok = ok && c->f <= (v);
    MD_LEAN_SIZE_PINS(MD_PIN_EQUALS, MD_PIN_AT_MOST)
#undef MD_PIN_EQUALS
#undef MD_PIN_AT_MOST
    return ok;
}

/* The narrow launch: every lean pin and every size pin */
MD_HD int md_lean_narrow_hold(const MdState* s, const MdConfig* c) { return md_lean_pins_hold(s, c) && md_lean_size_pins_hold(c); }

#endif
