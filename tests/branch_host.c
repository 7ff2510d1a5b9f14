/* Host build of include/md_branch.h (device-side env snapshots), loaded by the tests through tests/hostlib.py: the table of per-env
 * extents as the C compiler sees it, md_env_view for the comparison with it, and one md_branch launch restated as a loop over the
 * pairs, the table and the extras (all pointers host arrays; the rows are moved with memcpy, the pairs one after the other). */
#include <string.h>

#include "md_branch.h"
#include "md_entity.h"

#define EXPORT __attribute__((visibility("default")))

typedef struct Field { const char* name; size_t offset; int unit, bytes, scale; } Field;
#define ROW(field, unit, bytes, scale) {#field, offsetof(MdState, field), unit, bytes, scale},
static const Field kFields[] = {MD_BRANCH_FIELDS(ROW)};
#undef ROW
#define NAME(field) #field,
static const char* const kNotPerEnv[] = {MD_BRANCH_NOT_PER_ENV(NAME)};
#undef NAME
enum { kNumFields = sizeof kFields / sizeof kFields[0], kNumNotPerEnv = sizeof kNotPerEnv / sizeof kNotPerEnv[0] };

EXPORT int hx_sizeof_branch(void) { return (int)sizeof(MdBranch); }
EXPORT int hx_max_extras(void) { return MD_BR_MAX_EXTRAS; }
EXPORT int hx_n_fields(void) { return kNumFields; }
EXPORT const char* hx_field_name(int i) { return kFields[i].name; }
EXPORT long long hx_field_offset(int i) { return (long long)kFields[i].offset; }
EXPORT long long hx_field_row_bytes(const MdConfig* c, int i) {
    return (long long)md_branch_row_bytes(c, kFields[i].unit, kFields[i].bytes, kFields[i].scale);
}
EXPORT int hx_n_not_per_env(void) { return kNumNotPerEnv; }
EXPORT const char* hx_not_per_env_name(int i) { return kNotPerEnv[i]; }

EXPORT void hx_env_view(const MdState* g, const MdConfig* c, int e, MdState* out) { *out = md_env_view(g, c, e); }

static void copy_row(void* dst, const void* src, size_t row_bytes, int srow, int drow) {
    if (dst == NULL || src == NULL || row_bytes == 0) return;
    memcpy((char*)dst + (size_t)drow * row_bytes, (const char*)src + (size_t)srow * row_bytes, row_bytes);
}

/* md_branch without the launch: 0, or -1 for a pair out of range */
EXPORT int hx_branch(const MdState* dst, const MdState* src, const MdConfig* c, const MdBranch* b) {
    for (int p = 0; p < b->n_pairs; ++p) {
        const int srow = b->src_row[p], drow = b->dst_row[p];
        if (srow < 0 || srow >= b->src_n_envs || drow < 0 || drow >= b->dst_n_envs) return -1;
        for (int i = 0; i < kNumFields; ++i) {
            void* d = *(void* const*)((const char*)dst + kFields[i].offset);
            const void* s = *(const void* const*)((const char*)src + kFields[i].offset);
            copy_row(d, s, md_branch_row_bytes(c, kFields[i].unit, kFields[i].bytes, kFields[i].scale), srow, drow);
        }
        for (int k = 0; k < b->n_extras; ++k) copy_row(b->extra[k].dst, b->extra[k].src, (size_t)b->extra[k].row_bytes, srow, drow);
    }
    return 0;
}
