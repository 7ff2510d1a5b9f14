/* Host build of include/md_lean_view.h (MdStepArgs, the step kernels' parameter list as one struct, and the lists of its fields that
 * the lean kernel reads from the kernel-argument segment), loaded by tests/test_kernarg_layout.py through tests/hostlib.py.  The same
 * text the library compiles. */
#include <stdio.h>

#include "md_lean_view.h"

#define EXPORT __attribute__((visibility("default")))

/* one line per entry, "name offset size": first the members of MdStepArgs (MD_STEP_ARGS), a line "--", then every field of
 * MD_LEAN_ARGS.  -> the characters written, or -1 if `cap` is too small */
EXPORT int hx_kernarg_layout(char* out, int cap) {
    int n = 0;
#define LINE(f)                                                                                                          \
    if (n >= 0) {                                                                                                        \
        const int k = snprintf(out + n, (size_t)(cap - n), "%s %zu %zu\n", #f, offsetof(MdStepArgs, f), sizeof(((MdStepArgs*)0)->f)); \
        n = (k < 0 || k >= cap - n) ? -1 : n + k;                                                                        \
    }
    MD_STEP_ARGS(LINE)
    if (n >= 0) {
        const int k = snprintf(out + n, (size_t)(cap - n), "--\n");
        n = (k < 0 || k >= cap - n) ? -1 : n + k;
    }
    MD_LEAN_ARGS(LINE)
#undef LINE
    return n;
}
