/*
 * md_branch.h -- device-side env snapshots: copy the WHOLE per-env state of chosen envs between two MdState blocks in one
 * launch (env -> env of one batch: BatchedEnvBase.branch; batch -> snapshot storage and back: snapshot / restore).  No
 * reference counterpart: the reference can only pickle one whole engine; this is what per-env state control looks like when
 * everything that evolves is a flat array (metadrive_ped_amd/branch.py is the Python surface).
 *
 * ONE table of per-env extents, MD_BRANCH_FIELDS below: every pointer field of MdState that holds rows per env, as
 * (unit, bytes per unit, scale).  An env's row of a field is  units * bytes * scale  bytes long and starts at  env * that:
 *   unit   MD_BR_SLOT  = MdConfig.cap units per env, MD_BR_AGENT = MdConfig.agents_per_env, MD_BR_ENV = one
 *   scale  MD_BR_ONE, or the MdConfig size the unit is multiplied by (obs_dim, route_seg_cap, route_vert_cap)
 * The bytes are literal numbers so that branch.py reads this table as text (it sizes a snapshot's storage from it); the
 * static assertions below hold them to the struct sizes.  The fields that are NOT per env -- borrowed caller buffers, the
 * recorded frames, the reserved work space -- are listed in MD_BRANCH_NOT_PER_ENV and never copied.  md_env_view
 * (md_entity.h) advances the same pointers by the same extents; tests/test_branch.py holds the two together, and both lists
 * to the fields of MdState, so a field added later cannot be silently left out of a snapshot.
 *
 * The md_branch kernel (csrc/parts/branch.inc: branch_kernel), the host build of the tests (tests/branch_host.c) and branch.py all walk
 * this table.  What the engine owns outside MdState (MdWorld.env_map, the top-down history and image, the takeover bytes,
 * the staged-draw index) travels through MdBranch.extra: up to MD_BR_MAX_EXTRAS arrays of row_bytes bytes per env.
 */
#ifndef MD_BRANCH_H
#define MD_BRANCH_H

#include <stddef.h>

#include "md_math.h"
#include "mdstep.h"

#define MD_BR_SLOT 0
#define MD_BR_AGENT 1
#define MD_BR_ENV 2

#define MD_BR_ONE 0
#define MD_BR_OBS_DIM 1
#define MD_BR_SEG_CAP 2
#define MD_BR_VERT_CAP 3

#define MD_BR_MAX_EXTRAS 12

/* X(field of MdState, unit, bytes per unit, scale) */
#define MD_BRANCH_FIELDS(X)                   \
    X(shape, MD_BR_SLOT, 32, MD_BR_ONE)       \
    X(dyn, MD_BR_SLOT, 32, MD_BR_ONE)         \
    X(param, MD_BR_SLOT, 32, MD_BR_ONE)       \
    X(nav, MD_BR_SLOT, 64, MD_BR_ONE)         \
    X(pid, MD_BR_SLOT, 32, MD_BR_ONE)         \
    X(action, MD_BR_SLOT, 8, MD_BR_ONE)       \
    X(route_nodes, MD_BR_SLOT, 192, MD_BR_ONE)  \
    X(route_roads, MD_BR_SLOT, 192, MD_BR_ONE)  \
    X(final_lane, MD_BR_SLOT, 4, MD_BR_ONE)   \
    X(idm_rand, MD_BR_SLOT, 32, MD_BR_ONE)    \
    X(flags, MD_BR_SLOT, 4, MD_BR_ONE)        \
    X(obs, MD_BR_AGENT, 4, MD_BR_OBS_DIM)     \
    X(reward, MD_BR_AGENT, 4, MD_BR_ONE)      \
    X(cost, MD_BR_AGENT, 4, MD_BR_ONE)        \
    X(step_info, MD_BR_AGENT, 32, MD_BR_ONE)  \
    X(need_reset, MD_BR_ENV, 4, MD_BR_ONE)    \
    X(shape0, MD_BR_SLOT, 32, MD_BR_ONE)      \
    X(dyn0, MD_BR_SLOT, 32, MD_BR_ONE)        \
    X(nav0, MD_BR_SLOT, 64, MD_BR_ONE)        \
    X(pid0, MD_BR_SLOT, 32, MD_BR_ONE)        \
    X(route_nodes0, MD_BR_SLOT, 192, MD_BR_ONE) \
    X(route_roads0, MD_BR_SLOT, 192, MD_BR_ONE) \
    X(final_lane0, MD_BR_SLOT, 4, MD_BR_ONE)  \
    X(rng, MD_BR_ENV, 4, MD_BR_ONE)           \
    X(env_steps, MD_BR_ENV, 4, MD_BR_ONE)     \
    X(agent_id, MD_BR_SLOT, 4, MD_BR_ONE)     \
    X(next_agent_id, MD_BR_ENV, 4, MD_BR_ONE) \
    X(detected, MD_BR_AGENT, 16, MD_BR_ONE)   \
    X(param0, MD_BR_SLOT, 32, MD_BR_ONE)      \
    X(done_out, MD_BR_AGENT, 4, MD_BR_ONE)    \
    X(route_n, MD_BR_SLOT, 16, MD_BR_ONE)     \
    X(route_segs, MD_BR_SLOT, 48, MD_BR_SEG_CAP) \
    X(route_verts, MD_BR_SLOT, 8, MD_BR_VERT_CAP) \
    X(route_aux, MD_BR_SLOT, 32, MD_BR_ONE)   \
    X(idle_ring, MD_BR_AGENT, 400, MD_BR_ONE) \
    X(scene_of, MD_BR_ENV, 4, MD_BR_ONE)      \
    X(walk_ep, MD_BR_ENV, 4, MD_BR_ONE)

/* Y(field of MdState): pointer fields that hold no rows of their own per env */
#define MD_BRANCH_NOT_PER_ENV(Y)                                                          \
    Y(agent_action) /* the caller's action buffer of one step, borrowed for that launch */ \
    Y(track_shape)  /* recorded frames, indexed by frame and scene */                      \
    Y(track_dyn)                                                                          \
    Y(scratch)      /* reserved, NULL */

/* the literal sizes above against the structs and limits they stand for */
typedef char md_br_assert_sizes[(sizeof(MdShape) == 32 && sizeof(MdDyn) == 32 && sizeof(MdParam) == 32 && sizeof(MdNav) == 64 &&
                                 sizeof(MdPid) == 32 && sizeof(MdSeg) == 48 && 4 * MD_ROUTE_LEN == 192 && 4 * MD_IDM_RAND == 32 &&
                                 4 * MD_IDLE_WINDOW == 400) ? 1 : -1];

typedef struct MdBranchExtra {
    void* dst;             /* [dst_n_envs][row_bytes] */
    const void* src;       /* [src_n_envs][row_bytes] */
    int64_t row_bytes;     /* bytes per env, >= 1 */
} MdBranchExtra;

typedef struct MdBranch {
    int32_t struct_size;   /* sizeof(MdBranch) as the caller sees it */
    int32_t n_pairs;       /* >= 1 */
    int32_t src_n_envs;    /* rows of the arrays of `src` (a snapshot holds only its own rows) */
    int32_t dst_n_envs;    /* rows of the arrays of `dst` */
    int32_t n_extras;      /* 0 .. MD_BR_MAX_EXTRAS */
    int32_t reserved;      /* 0 */
    const int32_t* src_row; /* [n_pairs] device: row of `src` that pair i reads */
    const int32_t* dst_row; /* [n_pairs] device: row of `dst` that pair i writes; no row twice, and -- where src and dst are
                              the same arrays -- no row that is also read (the pairs run concurrently) */
    MdBranchExtra extra[MD_BR_MAX_EXTRAS];
} MdBranch;

/* units of `unit` per env */
MD_HD size_t md_branch_units(const MdConfig* c, int unit) {
    return unit == MD_BR_SLOT ? (size_t)c->cap : (unit == MD_BR_AGENT ? (size_t)c->agents_per_env : (size_t)1);
}
MD_HD size_t md_branch_scale(const MdConfig* c, int scale) {
    return scale == MD_BR_OBS_DIM ? (size_t)c->obs_dim
                                  : (scale == MD_BR_SEG_CAP ? (size_t)c->route_seg_cap : (scale == MD_BR_VERT_CAP ? (size_t)c->route_vert_cap : (size_t)1));
}
/* bytes of one env's row of a field of the table */
MD_HD size_t md_branch_row_bytes(const MdConfig* c, int unit, int bytes, int scale) {
    return md_branch_units(c, unit) * (size_t)bytes * md_branch_scale(c, scale);
}

#ifdef __cplusplus
extern "C" {
#endif

/* For every pair i: the row src_row[i] of every per-env array of `src` (MD_BRANCH_FIELDS; c gives cap, agents_per_env, obs_dim
 * and the route capacities) and of every b->extra[k].src is copied to the row dst_row[i] of the same array of `dst` /
 * b->extra[k].dst.  A field that is NULL in either state is skipped.  ONE launch, one workgroup per pair, asynchronous on
 * `stream`; no world is read.  The caller keeps the destination rows distinct and apart from the source rows. */
int md_branch(const MdState* dst, const MdState* src, const MdConfig* c, const MdBranch* b, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MD_BRANCH_H */
