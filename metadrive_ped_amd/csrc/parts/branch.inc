// parts/branch.inc -- part of mdstep.hip, included there and not compiled on its own.
// Provides: branch_copy_as, branch_rows and branch_kernel (include/md_branch.h),
// and the entry point md_branch with its argument checks.
// Relies on: mdstep.hip (md_u32x4), entry_checks.

namespace {

// md_branch (include/md_branch.h): the copy of whole envs between two states, one workgroup per (source row, destination row) pair.
// A pure gather-copy: the workgroup walks the table of per-env extents, then the extras.  Per field the row is moved with the widest
// access both row bases and the length allow -- 16 bytes (the 32 / 64-byte records always), else 4 (an obs row of 259 floats is no
// multiple of 16 bytes), else single bytes (the 1-byte extras) -- decided block-uniformly, and a thread issues up to four loads before
// their stores, so that a field costs one memory round trip, not one per word.  A fan-out reads its one source row from L2.
// No LDS, no atomics; the pairs never meet (the caller keeps destination rows distinct and apart from the source rows).
template <typename T>
__device__ __forceinline__ void branch_copy_as(char* d, const char* s, size_t n, int tid) {
    T* dp = reinterpret_cast<T*>(d);
    const T* sp = reinterpret_cast<const T*>(s);
    for (size_t i = tid; i < n; i += 4 * 256) {
        T v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            v[u] = T{};
            if (i + u * 256 < n) v[u] = sp[i + u * 256];
        }
#pragma unroll
        for (int u = 0; u < 4; ++u)
            if (i + u * 256 < n) dp[i + u * 256] = v[u];
    }
}

// One copy of the three loops for all ~50 call sites (called, not inlined: the kernel stays a few KB of code instead of ~40).
__device__ __noinline__ void branch_rows(void* dst, const void* src, size_t row_bytes, int srow, int drow, int tid) {
    if (dst == nullptr || src == nullptr || row_bytes == 0) return;   // an array this batch does not have
    const char* s = reinterpret_cast<const char*>(src) + (size_t)srow * row_bytes;
    char* d = reinterpret_cast<char*>(dst) + (size_t)drow * row_bytes;
    const uintptr_t bits = (uintptr_t)s | (uintptr_t)d | (uintptr_t)row_bytes;   // block-uniform
    if ((bits & 15) == 0) branch_copy_as<md_u32x4>(d, s, row_bytes >> 4, tid);
    else if ((bits & 3) == 0) branch_copy_as<uint32_t>(d, s, row_bytes >> 2, tid);
    else branch_copy_as<uint8_t>(d, s, row_bytes, tid);
}

__global__ __launch_bounds__(256) void branch_kernel(MdState dst, MdState src, MdConfig c, MdBranch b) {
    const int p = blockIdx.x;
    if (p >= b.n_pairs) return;
    const int srow = b.src_row[p], drow = b.dst_row[p];
    if (srow < 0 || srow >= b.src_n_envs || drow < 0 || drow >= b.dst_n_envs) return;   // block-uniform; the host refuses such a pair
    const int tid = threadIdx.x;
#define MD_BR_COPY(field, unit, bytes, scale) \
    branch_rows((void*)dst.field, (const void*)src.field, md_branch_row_bytes(&c, unit, bytes, scale), srow, drow, tid);
    MD_BRANCH_FIELDS(MD_BR_COPY)
#undef MD_BR_COPY
#pragma unroll
    for (int k = 0; k < MD_BR_MAX_EXTRAS; ++k)
        if (k < b.n_extras) branch_rows(b.extra[k].dst, b.extra[k].src, (size_t)b.extra[k].row_bytes, srow, drow, tid);
}

}  // namespace

extern "C" {

__attribute__((visibility("default"))) int md_branch(const MdState* dst, const MdState* src, const MdConfig* c, const MdBranch* b, void* stream) {
    NEED(dst); NEED(src); NEED(c); NEED(b);
    TRY(check_struct_size(c));
    TRY(check_arg_size("MdBranch", b->struct_size, sizeof(MdBranch)));
    NEED(b->src_row); NEED(b->dst_row);
    if (c->cap <= 0 || c->cap > MD_MAX_CAP || c->agents_per_env <= 0 || c->agents_per_env > c->cap || c->obs_dim < 0 ||
        c->route_seg_cap < 0 || c->route_vert_cap < 0) {
        snprintf(g_err, sizeof g_err, "md_branch: bad sizes: cap=%d agents_per_env=%d obs_dim=%d route_seg_cap=%d route_vert_cap=%d (cap<=%d)",
                 c->cap, c->agents_per_env, c->obs_dim, c->route_seg_cap, c->route_vert_cap, MD_MAX_CAP);
        return MD_EINVAL;
    }
    if (b->n_pairs <= 0) {
        snprintf(g_err, sizeof g_err, "md_branch: n_pairs=%d must be positive", b->n_pairs);
        return MD_EINVAL;
    }
    if (b->src_n_envs <= 0 || b->dst_n_envs <= 0) {
        snprintf(g_err, sizeof g_err, "md_branch: src_n_envs=%d and dst_n_envs=%d must be positive", b->src_n_envs, b->dst_n_envs);
        return MD_EINVAL;
    }
    TRY(check_counts("md_branch", {{"n_extras", b->n_extras, 0, MD_BR_MAX_EXTRAS, "MD_BR_MAX_EXTRAS"}}));
    for (int k = 0; k < b->n_extras; ++k) {
        if (!b->extra[k].dst || !b->extra[k].src) {
            snprintf(g_err, sizeof g_err, "required pointer b->extra[%d].%s is null", k, b->extra[k].dst ? "src" : "dst");
            return MD_EINVAL;
        }
        if (b->extra[k].row_bytes <= 0) {
            snprintf(g_err, sizeof g_err, "md_branch: extra[%d].row_bytes=%lld must be positive", k, (long long)b->extra[k].row_bytes);
            return MD_EINVAL;
        }
    }
    hipLaunchKernelGGL(branch_kernel, dim3(b->n_pairs), dim3(256), 0, (hipStream_t)stream, *dst, *src, *c, *b);
    return launch_status();
}

}  // extern "C"
