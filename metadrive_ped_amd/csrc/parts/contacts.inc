// parts/contacts.inc -- part of mdstep.hip, included there and not compiled on its own.
// Provides: MD_CONTACTS_FLAT, contacts_quad_bits and contacts_vehicle<kFlat>.
// Relies on: mdstep.hip (MD_CONTACTS_STAMP / MD_CONTACTS_COUNT), localize (grid_clampi).

namespace {

// ------------------------------------------------------------------------------------------------
// Contacts, one wave per vehicle.
// ------------------------------------------------------------------------------------------------
// Two jobs, one after the other: the movers in LDS, then the static quads through the grid.  The flag word is an OR over the hits.
// kFlat (the lean kernel only; -DMD_CONTACTS_FLAT=0 compiles it out): the quads of the up to four cells under the chassis in ONE
// pass -- lanes 0 .. 3 fetch their cell's cell_start pair in one trip, then wave lane t takes item t of the ranges laid end to end
// (md_flat_cell_item), so the cell_items / quad / kind loads are made once for the whole set: four dependent round trips where
// the nested loops make three or four per cell, each cell's behind the one before.  A box of more than four cells (no vehicle of
// the reference's sizes on the 8 m grid) takes the nested loops.
#ifndef MD_CONTACTS_FLAT
#define MD_CONTACTS_FLAT 1
#endif
// the flag a static quad raises under the chassis `me` (0: clear of it, or a kind without a flag)
__device__ __forceinline__ uint32_t contacts_quad_bits(const MdShape& me, const float* quads, const int32_t* qkind, int q) {
    if (!md_obb_quad(me.cx, me.cy, me.c, me.s, me.hl, me.hw, quads + 8 * (size_t)q)) return 0u;
    switch (qkind[q]) {
        case MD_Q_LINE_WHITE_CONT: return MD_FL_ON_WHITE_CONT;
        case MD_Q_LINE_YELLOW_CONT: return MD_FL_ON_YELLOW_CONT;
        case MD_Q_LINE_BROKEN: return MD_FL_ON_BROKEN;
        case MD_Q_SIDEWALK: return MD_FL_CRASH_SIDEWALK;
        case MD_Q_CROSSWALK: return MD_FL_ON_CROSSWALK;
        default: return 0u;
    }
}

template <bool kFlat = false>
__device__ __forceinline__ void contacts_vehicle(const MdWorld& w, const MdState& s, const MdConfig& c, int e, int slot, int lane_id,
                                 uint32_t* cfl_out = nullptr) {
    const int base = 0;  // env-local view
    const int n = slot;
    const MdShape me = s.shape[n];
    if (!md_drives(me.flags)) return;
    if (!(me.flags & MD_F_AGENT)) {  // traffic: nothing reads its crash / line flags (see the oracle's contacts_mover)
        if (lane_id == 0) {
            if (cfl_out) cfl_out[n] = 0u;
            else s.flags[n] &= MD_FL_ON_LANE;
        }
        return;
    }
    uint32_t fl = 0;
    MD_CONTACTS_STAMP(n == 0 && lane_id == 0, 0);
    for (int j0 = 0; j0 < c.cap; j0 += 64) {
        const int j = j0 + lane_id;
        if (j >= c.cap || j == slot) continue;
        const MdShape o = s.shape[base + j];
        if (!md_present(o.flags)) continue;
        const int k = md_kind_of(o.flags);
        int hit;
        if (md_is_circle_kind(k)) hit = md_obb_circle(me.cx, me.cy, me.c, me.s, me.hl, me.hw, o.cx, o.cy, o.hl);
        else hit = md_obb_obb(me.cx, me.cy, me.c, me.s, me.hl, me.hw, o.cx, o.cy, o.c, o.s, o.hl, o.hw);
        if (!hit) continue;
        if (k == MD_KIND_VEHICLE) fl |= MD_FL_CRASH_VEHICLE;
        else if (k == MD_KIND_CONE || k == MD_KIND_WARNING || k == MD_KIND_BARRIER) fl |= MD_FL_CRASH_OBJECT;
        else if (k == MD_KIND_PEDESTRIAN || k == MD_KIND_CYCLIST) fl |= MD_FL_CRASH_HUMAN;
        else if (k == MD_KIND_BUILDING) fl |= MD_FL_CRASH_BUILDING;
    }
    MD_CONTACTS_STAMP(n == 0 && lane_id == 0, 1);
    // static quads through the grid: cells under the chassis AABB (+ margin)
    const int m = w.env_map[e];
    const MdGrid g = w.grid[m];
    const float ext_x = md_fabs(me.c) * me.hl + md_fabs(me.s) * me.hw + 0.05f;
    const float ext_y = md_fabs(me.s) * me.hl + md_fabs(me.c) * me.hw + 0.05f;
    int gx0 = (int)md_floor((me.cx - ext_x - g.x0) * g.inv_cell);
    int gx1 = (int)md_floor((me.cx + ext_x - g.x0) * g.inv_cell);
    int gy0 = (int)md_floor((me.cy - ext_y - g.y0) * g.inv_cell);
    int gy1 = (int)md_floor((me.cy + ext_y - g.y0) * g.inv_cell);
    if (!(gx1 < 0 || gy1 < 0 || gx0 >= g.nx || gy0 >= g.ny)) {
        gx0 = grid_clampi(gx0, 0, g.nx - 1);
        gx1 = grid_clampi(gx1, 0, g.nx - 1);
        gy0 = grid_clampi(gy0, 0, g.ny - 1);
        gy1 = grid_clampi(gy1, 0, g.ny - 1);
        const float* quads = w.quads + 8 * (size_t)w.quad_off[m];
        const int32_t* qkind = w.quad_kind + w.quad_off[m];
        const int ncx = gx1 - gx0 + 1, n_cells = ncx * (gy1 - gy0 + 1);
        if (kFlat && n_cells <= 4) {
            // lanes 0 .. n_cells - 1: their cell's range, the cells in the nested loops' order (the box row by row, gx ascending)
            int my0 = 0, myn = 0;
            if (lane_id < n_cells) {
                const int cell = g.cell_base + (gy0 + lane_id / ncx) * g.nx + gx0 + lane_id % ncx;
                my0 = w.cell_start[cell];
                myn = w.cell_start[cell + 1] - my0;
                if (myn < 0) myn = 0;
            }
            const int s0 = __builtin_amdgcn_readlane(my0, 0), s1 = __builtin_amdgcn_readlane(my0, 1);
            const int s2 = __builtin_amdgcn_readlane(my0, 2), s3 = __builtin_amdgcn_readlane(my0, 3);
            const int n0 = __builtin_amdgcn_readlane(myn, 0), n1 = __builtin_amdgcn_readlane(myn, 1);
            const int n2 = __builtin_amdgcn_readlane(myn, 2), n3 = __builtin_amdgcn_readlane(myn, 3);
            const int total = n0 + n1 + n2 + n3;   // the loop's bound: wave-uniform, known before it starts
            MD_CONTACTS_COUNT(n == 0 && lane_id == 0, n_cells, total);
            for (int t = lane_id; t < total; t += 64) {
                int off;
                const int k = md_flat_cell_item(n0, n1, n2, n3, t, &off);
                const int item = w.cell_items[(k == 0 ? s0 : k == 1 ? s1 : k == 2 ? s2 : s3) + off];
                if (item >= 0) continue;  // lane item
                fl |= contacts_quad_bits(me, quads, qkind, ~item);
            }
        } else
        for (int gy = gy0; gy <= gy1; ++gy)
            for (int gx = gx0; gx <= gx1; ++gx) {
                const int cell = g.cell_base + gy * g.nx + gx;
                const int it0 = w.cell_start[cell], it1 = w.cell_start[cell + 1];
                MD_CONTACTS_COUNT(n == 0 && lane_id == 0, 1, it1 > it0 ? it1 - it0 : 0);
                for (int it = it0 + lane_id; it < it1; it += 64) {
                    const int item = w.cell_items[it];
                    if (item >= 0) continue;  // lane item
                    const int q = ~item;
                    if (!md_obb_quad(me.cx, me.cy, me.c, me.s, me.hl, me.hw, quads + 8 * (size_t)q)) continue;
                    switch (qkind[q]) {   // (contacts_quad_bits in words: through the helper, seven other kernels' register lines move)
                        case MD_Q_LINE_WHITE_CONT: fl |= MD_FL_ON_WHITE_CONT; break;
                        case MD_Q_LINE_YELLOW_CONT: fl |= MD_FL_ON_YELLOW_CONT; break;
                        case MD_Q_LINE_BROKEN: fl |= MD_FL_ON_BROKEN; break;
                        case MD_Q_SIDEWALK: fl |= MD_FL_CRASH_SIDEWALK; break;
                        case MD_Q_CROSSWALK: fl |= MD_FL_ON_CROSSWALK; break;
                        default: break;
                    }
                }
            }
    }
    MD_CONTACTS_STAMP(n == 0 && lane_id == 0, 2);
    // wave OR-reduce of the flag word: one ballot per flag bit that can be set here
    uint32_t all = 0;
#pragma unroll
    for (int b = 0; b < 9; ++b) {
        const uint32_t bit = 1u << b;
        if (__ballot((fl & bit) != 0) != 0ull) all |= bit;
    }
    if (lane_id == 0) {
        if (cfl_out) cfl_out[n] = all;
        else s.flags[n] = (s.flags[n] & MD_FL_ON_LANE) | all;
    }
}

}  // namespace
