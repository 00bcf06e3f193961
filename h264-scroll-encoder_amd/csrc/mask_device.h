/*
 * mask_device.h -- the rule of the dynamic rect's per-MB source mask
 * (scroll_batch_dyn_mask): which MBs of the rect changed, which
 * are kept, and what the frame's record says of the rest.
 *
 * Pure integer functions: k_dyn_mask_diff, k_dyn_mask_fill and k_dyn_mask_rec
 * (mask_kernels.hip) run them, tests/hostsim/mask_sim.cpp compiles them for
 * the CPU and tests/test_mask_hostsim.py checks them against the numpy
 * restatement of tests/maskhelp.py.
 *
 * The map.  For frame f of stream s and MB (mx, my) of its w x h rect, two
 * uint32:
 *     Dy = sum over the MB's 256 luma samples of (src - pred)^2
 *     Dc = the same over its 64 Cb + 64 Cr samples, bit 31 (KEPT): the MB is kept
 * src: the rect's source (d_src); pred: the sample k_dyn_row subtracts there,
 * which the kernels take from the coder's own predictor (k_dyn_rows'
 * prediction rows through RowPred / chroma_pred_any, recon_pred.h) -- this
 * file never forms a prediction.  Dy <= 256 * 255^2 < 2^24, Dc <= 128 * 255^2
 * < 2^24: bit 31 is free.
 *
 * The rule.  changed iff Dy > mb_sse_y || Dc > mb_sse_c; kept iff a changed
 * MB of the same rect lies within grow MBs (0..2) in both directions.  The
 * record: n_changed, n_kept, sse_drop[Y, Cb, Cr] = the planes' parts of D over
 * the MBs not kept (Y from the map; Cb and Cr apart from the samples, since
 * the map holds their sum).  Sums and counts only: independent of order.
 */
#ifndef SCROLL_MASK_DEVICE_H
#define SCROLL_MASK_DEVICE_H

#include <stddef.h>
#include <stdint.h>

#include "composer_batch.h"     /* ScrollDynMask, ScrollDynMaskRule, SCROLL_DYN_MASK_* */

#if !defined(__HIPCC__) && !defined(__device__)
#define __device__
#define __host__
#endif

namespace scroll {
namespace mask {

constexpr uint32_t MAX_GROW = 2u;
constexpr uint32_t KEPT = SCROLL_DYN_MASK_KEPT;

/* ---- the map ---- */

/* four source bytes against four prediction bytes (packed words, any byte
 * order as long as it is the same): their squared differences added to acc */
__host__ __device__ inline uint32_t sq4b(uint32_t a, uint32_t b, uint32_t acc)
{
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int32_t d = (int32_t)((a >> (8 * k)) & 255u) - (int32_t)((b >> (8 * k)) & 255u);
        acc += (uint32_t)(d * d);
    }
    return acc;
}

/* ---- the rule ---- */

__host__ __device__ inline bool changed(uint32_t dy, uint32_t dc, const ScrollDynMaskRule &r)
{
    return dy > r.mb_sse_y || (dc & ~KEPT) > r.mb_sse_c;
}

/* is MB (mx, my) of the w x h rect kept?  The (2 grow + 1)^2 neighbours are
 * numbered row by row; this call looks at numbers part, part + nparts, ...:
 * the results of parts 0 .. nparts - 1 OR-ed are the answer (a lane quad
 * shares one MB's neighbours; part 0 of 1 is the whole).  map: the frame's
 * entries, two words per MB; the KEPT bit of a neighbour is not looked at. */
__host__ __device__ inline bool kept_part(const uint32_t *map, uint32_t w, uint32_t h, uint32_t mx, uint32_t my,
                                          const ScrollDynMaskRule &r, uint32_t part, uint32_t nparts)
{
    const int32_t g = (int32_t)r.grow, side = 2 * g + 1;
    bool k = false;
    for (int32_t i = (int32_t)part; i < side * side; i += (int32_t)nparts) {
        const int32_t dy = i / side, dx = i - dy * side;
        const int32_t x = (int32_t)mx + dx - g, y = (int32_t)my + dy - g;
        if (x < 0 || y < 0 || x >= (int32_t)w || y >= (int32_t)h) continue;
        const uint32_t *e = map + 2 * ((size_t)y * w + (size_t)x);
        k |= changed(e[0], e[1], r);
    }
    return k;
}

/* what a walk over (part of) a frame's map gathers; acc_merge joins two parts */
struct Acc {
    uint32_t n_changed, n_kept;
    uint64_t drop[3];
};

__host__ __device__ inline Acc acc_init() { return Acc{0u, 0u, {0u, 0u, 0u}}; }

/* MB (mx, my): counted, its Dy dropped unless kept; returns its entry's second word with the KEPT bit as it now is */
__host__ __device__ inline uint32_t acc_mb(Acc &a, const uint32_t *map, uint32_t w, uint32_t h, uint32_t mx,
                                           uint32_t my, const ScrollDynMaskRule &r)
{
    const uint32_t *e = map + 2 * ((size_t)my * w + mx);
    const uint32_t dy = e[0], dc = e[1] & ~KEPT;
    const bool kp = kept_part(map, w, h, mx, my, r, 0u, 1u);
    a.n_changed += changed(dy, dc, r) ? 1u : 0u;
    a.n_kept += kp ? 1u : 0u;
    if (!kp) a.drop[0] += dy;
    return dc | (kp ? KEPT : 0u);
}

__host__ __device__ inline void acc_merge(Acc &a, const Acc &b)
{
    a.n_changed += b.n_changed;
    a.n_kept += b.n_kept;
    for (int k = 0; k < 3; ++k) a.drop[k] += b.drop[k];
}

__host__ __device__ inline ScrollDynMask record(const Acc &a)
{
    ScrollDynMask m{};
    m.status = SCROLL_DYN_MASK_OK;
    m.n_changed = a.n_changed;
    m.n_kept = a.n_kept;
    for (int k = 0; k < 3; ++k) m.sse_drop[k] = a.drop[k];
    return m;
}

/* the record of a frame without a dynamic NAL */
__host__ __device__ inline ScrollDynMask noframe()
{
    ScrollDynMask m{};
    m.status = SCROLL_DYN_MASK_NOFRAME;
    return m;
}

/* one frame, serially: the rule as a whole, for the CPU and for reading.
 * map: in with any KEPT bits, out with the rule's; dcb: per MB the Cb part of
 * Dc (the Cr part is the rest) */
__host__ __device__ inline ScrollDynMask mask_frame(uint32_t *map, const uint32_t *dcb, uint32_t w, uint32_t h,
                                                    const ScrollDynMaskRule &r)
{
    Acc a = acc_init();
    for (uint32_t my = 0; my < h; ++my)
        for (uint32_t mx = 0; mx < w; ++mx) {
            const size_t i = (size_t)my * w + mx;
            /* (a neighbour's KEPT bit is masked off wherever it is read, so writing as we go changes nothing) */
            const uint32_t e1 = acc_mb(a, map, w, h, mx, my, r);
            if (!(e1 & KEPT)) {
                a.drop[1] += dcb[i];
                a.drop[2] += (e1 & ~KEPT) - dcb[i];
            }
            map[2 * i + 1] = e1;
        }
    return record(a);
}

}  // namespace mask
}  // namespace scroll

#endif
