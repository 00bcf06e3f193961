/*
 * dyn_pos.h -- the dynamic rect placed and sized per stream and per frame
 * (scroll_batch_set_dyn_rect_moving, DESIGN.md §3m;
 * scroll_batch_set_dyn_rect_size_at, §3p): the row-group count of a
 * placement, the position table's word, and the one place where a kernel
 * turns the batch's geometry into its frame's.
 */
#ifndef SCROLL_DYN_POS_H
#define SCROLL_DYN_POS_H

#include <stdint.h>

#include "engine.h"

/* row groups of a NAL whose h-row rect starts at MB row y0 of an mbh-row
 * picture: the static groups above (DYN_STATIC_ROWS rows each; the first
 * holds the slice header and exists even with no rows), the rect rows, the
 * static groups below (the last holds the stop bit and exists likewise) */
__host__ __device__ inline int dyn_groups_at(int y0, int h, int mbh)
{
    const int sr = DYN_STATIC_ROWS;
    const int na = (y0 + sr - 1) / sr, nb = (mbh - y0 - h + sr - 1) / sr;
    return (na > 1 ? na : 1) + h + (nb > 1 ? nb : 1);
}

/* the most of them over every legal y0 */
inline int dyn_groups_max(int h, int mbh)
{
    int m = 0;
    for (int y0 = 0; y0 + h <= mbh; ++y0) {
        const int n = dyn_groups_at(y0, h, mbh);
        m = n > m ? n : m;
    }
    return m;
}

/* With frames sized on their own (§3p) a frame's rect is h_f <= h rows at an
 * origin that is legal for the batch's h (y0 + h <= mbh).  Over every such
 * (y0, h_f): the most row groups, the most static row groups, and the most
 * row-stage words of a frame's region when a static group takes sw words and
 * a rect row rw -- computed, not assumed to lie at h_f = h */
struct DynSizedMax {
    int groups, statics;
    uint64_t words;
};
inline DynSizedMax dyn_sized_max(int h, int mbh, uint64_t sw, uint64_t rw)
{
    DynSizedMax m{0, 0, 0};
    for (int hf = 1; hf <= h; ++hf)
        for (int y0 = 0; y0 + h <= mbh; ++y0) {
            const int n = dyn_groups_at(y0, hf, mbh);
            const uint64_t wd = (uint64_t)(n - hf) * sw + (uint64_t)hf * rw;
            m.groups = n > m.groups ? n : m.groups;
            m.statics = n - hf > m.statics ? n - hf : m.statics;
            m.words = wd > m.words ? wd : m.words;
        }
    return m;
}

/* the position table's word of a frame at (x0, y0) whose rect is dw columns
 * and dh rows short of the batch's (0, 0: the batch's size -- the word every
 * table held before frames had sizes) */
__host__ __device__ inline uint32_t dyn_pos_pack(uint32_t x0, uint32_t y0, uint32_t dw, uint32_t dh)
{
    return x0 | dw << 8 | y0 << 16 | dh << 24;
}

/* what a word says under pos_mask (DynGeom: 0xff where origins fit a byte
 * and the high bytes are the size's, else 0xffff and no sizes) */
struct DynPosWord {
    int x0, y0, dw, dh;
};
__host__ __device__ inline DynPosWord dyn_pos_unpack(uint32_t e, uint32_t pos_mask)
{
    const uint32_t lo = e & 0xffffu, hi = e >> 16;
    DynPosWord p;
    p.x0 = (int)(lo & pos_mask);
    p.y0 = (int)(hi & pos_mask);
    p.dw = (int)((lo & ~pos_mask) >> 8);
    p.dh = (int)((hi & ~pos_mask) >> 8);
    return p;
}

#ifdef __HIPCC__
/* frame nb = s ld_fr + f of a kernel's copy of the geometry: with a position
 * table, x0, y0, w, h and ngroups become the frame's (one uniform load: a
 * scalar one where nb is uniform).  A frame without a rect has no dynamic NAL
 * (k_plan: DynFrame.nal = -1) and is coded by nobody; its entry reads as the
 * picture's origin at the batch's size, so that nothing computed before that
 * test leaves the picture. */
__device__ inline void dyn_frame_geom(DynGeom &g, size_t nb)
{
    if (!g.dpos) return;
    const uint32_t e = __builtin_amdgcn_readfirstlane(g.dpos[nb]);
    const DynPosWord p = dyn_pos_unpack(e == DYN_POS_NONE ? 0u : e, g.pos_mask);
    g.x0 = p.x0;
    g.y0 = p.y0;
    g.w = g.ld_w - p.dw;
    g.h = g.ld_h - p.dh;
    g.ngroups = dyn_groups_at(g.y0, g.h, g.ph / 16);
}
#endif

#endif
