/* Host build of the launch predicate of md_step's lean kernels (include/md_lean_pins.h: the lists that csrc/mdstep.hip's
 * variant<PH_ALL>() asks and its kernels fold), loaded by tests/test_lean_pins_host.py through tests/hostlib.py.  The same text
 * the library compiles. */
#include <string.h>

#include "md_lean_pins.h"

#define EXPORT __attribute__((visibility("default")))

/* n rows of (cap, agents_per_env, is_multi_agent, traffic_mode, agent_idm, num_others, detected set?) ->
 * out[3 * i] = lean pins hold, [3 * i + 1] = size pins hold, [3 * i + 2] = the narrow launch */
EXPORT void hx_lean_pins(int n, const int* rows, int* out) {
    static uint64_t some_set[2];
    for (int i = 0; i < n; ++i) {
        const int* r = rows + 7 * i;
        MdConfig c;
        MdState s;
        memset(&c, 0, sizeof c);
        memset(&s, 0, sizeof s);
        c.cap = r[0];
        c.agents_per_env = r[1];
        c.is_multi_agent = r[2];
        c.traffic_mode = r[3];
        c.agent_idm = r[4];
        c.num_others = r[5];
        s.detected = r[6] ? some_set : 0;
        out[3 * i] = md_lean_pins_hold(&s, &c);
        out[3 * i + 1] = md_lean_size_pins_hold(&c);
        out[3 * i + 2] = md_lean_narrow_hold(&s, &c);
    }
}
