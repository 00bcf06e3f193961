/*
 * damage_device.h -- the rule by which the dynamic rect is located from the
 * renderer's surfaces (scroll_batch_dyn_locate): the per-MB
 * damage map and the placement of the rect over the damaged MBs.
 *
 * Pure integer functions: k_dmg_rows, k_dyn_damage and k_dyn_place
 * (damage_kernels.hip) run them, tests/hostsim/damage_sim.cpp compiles them
 * for the CPU and tests/test_damage_hostsim.py checks them against the numpy
 * restatement of tests/damagehelp.py.
 *
 * The map.  For frame f of stream s and MB (mx, my) of the picture
 *     D = sum over the MB's 256 pixels of (Ysrc - Ypred)^2          (uint32)
 * Ysrc: csc_device.h's luma of the surface pixel (luma_px) under the caller's
 * format / matrix / range.  Ypred: the luma a decoder shows at that pixel for
 * a scroll MB without residual, the frame's scroll NAL being the one a
 * compose at scroll_batch_set_offsets' offsets would write.  Luma motion is
 * full-pel and vertical, so Ypred of picture row Y is a row of reference
 * picture A or B, the one luma_row() (dyn_device.h) resolves through the
 * waypoint chain from the region's reference and motion (pred_row below: the
 * luma branch of k_dyn_rows over the whole picture); the column is the
 * pixel's own.
 *
 * Luma only: chroma prediction is 1/8-pel bilinear and may run through
 * half-pel waypoint chains (chroma_px_any), so a change of colour that leaves
 * the luma as it was is NOT detected.
 * Against the prediction, not the decoder's picture: on a stream whose loop
 * filter is on (an ingested one without
 * deblocking_filter_control_present_flag) the decoded picture can differ from
 * this prediction at the seam between the two regions.
 *
 * The rule.  Per frame, from its map, the rect size w x h, the picture size
 * mbw x mbh (all in MBs) and the caller's mb_sse and margin:
 *   an MB is damaged iff D > mb_sse (mb_sse = 0: any difference);
 *   n_mb damaged MBs; their bounding box grown by margin MBs (0..4) on each
 *   side and clipped to the picture is [bx0, bx1) x [by0, by1)
 *   (docs/MASTER_DESIGN.md §7.1);
 *   n_mb = 0:                 SCROLL_DYN_LOC_NONE, no rect (x0 = y0 = -1), box 0;
 *   box at most w x h:        SCROLL_DYN_LOC_FIT,  x0 = min(bx0, mbw - w),
 *                                                  y0 = min(by0, mbh - h);
 *   a larger box:             SCROLL_DYN_LOC_OVER, the same position: the rect
 *                             covers the box's top-left part;
 *   a frame without a scroll NAL (experiment mode's waypoint frame):
 *                             SCROLL_DYN_LOC_NOFRAME, no rect, zero map entries;
 *   sse_all = sum of D over the picture, sse_out = sum of D over the MBs
 *   outside the placed rect (= sse_all without one), max_sse = the largest D.
 * Every value is a sum, a count, a minimum or a maximum: independent of the
 * order in which the MBs are visited.
 *
 * With size = 1 (ScrollDynLocate.size) the placed rect is also
 * sized: from the same origin it reaches to the box's end or to the batch
 * size, whichever comes first,
 *   w_f = min(bx1, x0 + w) - x0,   h_f = min(by1, y0 + h) - y0
 * so a FIT rect covers exactly origin-to-box-end and an OVER rect is w x h in
 * the dimension that is over.  The record's reserved word then holds
 * (w_f - 1) | (h_f - 1) << 8 (0 without a rect), sse_out is summed outside
 * the sized rect, and the table's entry carries w - w_f, h - h_f
 * (dyn_pos_pack).  size = 0: every value as before, reserved 0.
 */
#ifndef SCROLL_DAMAGE_DEVICE_H
#define SCROLL_DAMAGE_DEVICE_H

#include <stdint.h>

#include "composer_batch.h"     /* ScrollDynDamage, SCROLL_DYN_LOC_* */
#include "csc_device.h"
#include "dyn_device.h"         /* scroll::dyn::luma_row, WpTab; scroll::Regions */

namespace scroll {
namespace damage {

constexpr uint32_t MAX_MARGIN = 4u;

/* ---- the map ---- */

/* picture row Y (MB row Y / 16) of the frame whose regions are rg and whose
 * region A ends before MB row a_end = (h - off) / 16: reference picture 0 (A)
 * or 1 (B), its row in yo */
__host__ __device__ inline int pred_row(const dyn::WpTab &T, const Regions &rg, int a_end, int Y, int &yo)
{
    const bool cA = (Y >> 4) < a_end;
    return dyn::luma_row(T, cA ? rg.ra : rg.rb, Y + (cA ? rg.mva : rg.mvb), yo);
}

__host__ __device__ inline uint32_t sq_diff(uint32_t a, uint32_t b)
{
    const int32_t d = (int32_t)a - (int32_t)b;
    return (uint32_t)(d * d);
}

/* four surface pixels (memory order) against four prediction bytes (a
 * little-endian word, the first pixel lowest): their squared differences added to acc */
__host__ __device__ inline uint32_t sq4(const csc::Coef &k, uint32_t p0, uint32_t p1, uint32_t p2, uint32_t p3,
                                        uint32_t ref, uint32_t acc)
{
    acc += sq_diff(csc::luma_px(k, p0), ref & 255u);
    acc += sq_diff(csc::luma_px(k, p1), (ref >> 8) & 255u);
    acc += sq_diff(csc::luma_px(k, p2), (ref >> 16) & 255u);
    acc += sq_diff(csc::luma_px(k, p3), ref >> 24);
    return acc;
}

/* ---- the rule ---- */

/* what a walk over (part of) a frame's map gathers; merge() joins two parts */
struct Acc {
    uint32_t n, max;
    uint32_t x0, y0, x1, y1;    /* the damaged MBs' box, [x0, x1) x [y0, y1); n = 0: x0 = y0 = ~0, x1 = y1 = 0 */
    uint64_t sum;
};

__host__ __device__ inline Acc acc_init() { return Acc{0u, 0u, 0xFFFFFFFFu, 0xFFFFFFFFu, 0u, 0u, 0u}; }

__host__ __device__ inline uint32_t minu(uint32_t a, uint32_t b) { return a < b ? a : b; }
__host__ __device__ inline uint32_t maxu(uint32_t a, uint32_t b) { return a > b ? a : b; }

__host__ __device__ inline void acc_add(Acc &a, uint32_t D, uint32_t mx, uint32_t my, uint32_t mb_sse)
{
    a.sum += D;
    a.max = maxu(a.max, D);
    if (D > mb_sse) {
        ++a.n;
        a.x0 = minu(a.x0, mx);
        a.y0 = minu(a.y0, my);
        a.x1 = maxu(a.x1, mx + 1u);
        a.y1 = maxu(a.y1, my + 1u);
    }
}

__host__ __device__ inline void acc_merge(Acc &a, const Acc &b)
{
    a.n += b.n;
    a.max = maxu(a.max, b.max);
    a.x0 = minu(a.x0, b.x0);
    a.y0 = minu(a.y0, b.y0);
    a.x1 = maxu(a.x1, b.x1);
    a.y1 = maxu(a.y1, b.y1);
    a.sum += b.sum;
}

/* the record of a frame without a scroll NAL */
__host__ __device__ inline ScrollDynDamage noframe()
{
    ScrollDynDamage r{};
    r.x0 = r.y0 = -1;
    r.status = SCROLL_DYN_LOC_NOFRAME;
    return r;
}

/* the record of a frame from its whole map's Acc, all but sse_out, which is
 * sse_all until outside() has been summed (finish) */
__host__ __device__ inline ScrollDynDamage place(const Acc &a, uint32_t w, uint32_t h, uint32_t mbw, uint32_t mbh,
                                                 uint32_t margin, uint32_t size = 0u)
{
    ScrollDynDamage r{};
    r.n_mb = a.n;
    r.max_sse = a.max;
    r.sse_all = r.sse_out = a.sum;
    r.x0 = r.y0 = -1;
    r.status = SCROLL_DYN_LOC_NONE;
    if (a.n == 0u) return r;
    const uint32_t bx0 = a.x0 > margin ? a.x0 - margin : 0u, by0 = a.y0 > margin ? a.y0 - margin : 0u;
    const uint32_t bx1 = minu(a.x1 + margin, mbw), by1 = minu(a.y1 + margin, mbh);
    r.bx0 = (uint16_t)bx0;
    r.by0 = (uint16_t)by0;
    r.bx1 = (uint16_t)bx1;
    r.by1 = (uint16_t)by1;
    r.status = bx1 - bx0 <= w && by1 - by0 <= h ? SCROLL_DYN_LOC_FIT : SCROLL_DYN_LOC_OVER;
    r.x0 = (int16_t)minu(bx0, mbw - w);
    r.y0 = (int16_t)minu(by0, mbh - h);
    if (size) {
        const uint32_t x0 = (uint32_t)r.x0, y0 = (uint32_t)r.y0;
        const uint32_t wf = minu(bx1, x0 + w) - x0, hf = minu(by1, y0 + h) - y0;
        r.reserved = (uint16_t)((wf - 1u) | (hf - 1u) << 8);
    }
    return r;
}

/* the size of the rect a record places: the batch's w x h, or with size = 1 its own */
__host__ __device__ inline uint32_t placed_w(const ScrollDynDamage &r, uint32_t w, uint32_t size)
{
    return size && r.x0 >= 0 ? (r.reserved & 255u) + 1u : w;
}
__host__ __device__ inline uint32_t placed_h(const ScrollDynDamage &r, uint32_t h, uint32_t size)
{
    return size && r.x0 >= 0 ? (uint32_t)(r.reserved >> 8) + 1u : h;
}

/* MB (mx, my) lies inside the w x h rect the record places (w, h: placed_w, placed_h) */
__host__ __device__ inline bool covered(const ScrollDynDamage &r, uint32_t w, uint32_t h, uint32_t mx, uint32_t my)
{
    if (r.x0 < 0) return false;
    const uint32_t x0 = (uint32_t)r.x0, y0 = (uint32_t)r.y0;
    return mx >= x0 && mx < x0 + w && my >= y0 && my < y0 + h;
}

/* the sum of D over the covered MBs taken off */
__host__ __device__ inline void finish(ScrollDynDamage &r, uint64_t sse_in) { r.sse_out = r.sse_all - sse_in; }

/* the position table's entry (DynGeom.dpos) of a record */
__host__ __device__ inline uint32_t pos_entry(const ScrollDynDamage &r)
{
    return r.x0 < 0 ? 0xFFFFFFFFu : (uint32_t)r.x0 | (uint32_t)r.y0 << 16;
}
/* ... of a record placed with size = 1 in a batch whose rect is w x h: the
 * columns and rows the frame's rect is short of it in bits 8-15 and 24-31 */
__host__ __device__ inline uint32_t pos_entry_sized(const ScrollDynDamage &r, uint32_t w, uint32_t h)
{
    if (r.x0 < 0) return 0xFFFFFFFFu;
    return pos_entry(r) | (w - placed_w(r, w, 1u)) << 8 | (h - placed_h(r, h, 1u)) << 24;
}

/* one frame, serially: the rule as a whole, for the CPU and for reading */
__host__ __device__ inline ScrollDynDamage locate_frame(const uint32_t *map, uint32_t w, uint32_t h, uint32_t mbw,
                                                        uint32_t mbh, uint32_t mb_sse, uint32_t margin,
                                                        uint32_t size = 0u)
{
    Acc a = acc_init();
    for (uint32_t my = 0; my < mbh; ++my)
        for (uint32_t mx = 0; mx < mbw; ++mx) acc_add(a, map[(size_t)my * mbw + mx], mx, my, mb_sse);
    ScrollDynDamage r = place(a, w, h, mbw, mbh, margin, size);
    const uint32_t wf = placed_w(r, w, size), hf = placed_h(r, h, size);
    uint64_t in = 0;
    for (uint32_t my = 0; my < mbh; ++my)
        for (uint32_t mx = 0; mx < mbw; ++mx)
            if (covered(r, wf, hf, mx, my)) in += map[(size_t)my * mbw + mx];
    finish(r, in);
    return r;
}

}  // namespace damage
}  // namespace scroll

#endif
