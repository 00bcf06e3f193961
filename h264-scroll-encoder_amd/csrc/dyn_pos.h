/*
 * dyn_pos.h -- the dynamic rect placed per stream and per frame
 * (scroll_batch_set_dyn_rect_moving): the row-group count of a
 * placement, and the one place where a kernel turns the batch's geometry into
 * its frame's.
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

#ifdef __HIPCC__
/* frame nb = s ld_fr + f of a kernel's copy of the geometry: with a position
 * table, x0, y0 and ngroups become the frame's (one uniform load: a scalar
 * one where nb is uniform).  A frame without a rect has no dynamic NAL
 * (k_plan: DynFrame.nal = -1) and is coded by nobody; its entry reads as the
 * picture's origin, so that nothing computed before that test leaves the
 * picture. */
__device__ inline void dyn_frame_geom(DynGeom &g, size_t nb)
{
    if (!g.dpos) return;
    const uint32_t e = __builtin_amdgcn_readfirstlane(g.dpos[nb]);
    const bool none = e == DYN_POS_NONE;
    g.x0 = none ? 0 : (int)(e & 0xffffu);
    g.y0 = none ? 0 : (int)(e >> 16);
    g.ngroups = dyn_groups_at(g.y0, g.h, g.ph / 16);
}
#endif

#endif
