/*
 * csc_engine.h -- engine-internal launcher of k_csc (csc_kernels.hip), used
 * by the batch engine (batch_surface.hip).
 */
#ifndef SCROLL_CSC_ENGINE_H
#define SCROLL_CSC_ENGINE_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "csc_device.h"

/* One conversion: for every item (s, f), s < S, f < nframes, the w x h pixel
 * window (multiples of 16) of the surface at src + s src_ld + f src_fr, at
 * pixel (16 x0, 16 y0) -- or at 16 x pos[2 (s nframes + f)], +1 when pos is
 * given (device memory; x < 0: the item is skipped) -- goes to the I420 block
 * at dst + s dst_ld + f dst_fr: luma w x h, then Cb, Cr w/2 x h/2.  src,
 * pitch, src_fr and src_ld multiples of 16, dst, dst_fr and dst_ld of 8. */
typedef struct {
    const uint8_t *src;
    uint64_t pitch, src_fr, src_ld;
    uint8_t *dst;
    uint64_t dst_fr, dst_ld;
    const int32_t *pos;
    /* or, in place of pos, the batch's packed position table (DynGeom.dpos's
     * form: x0 | y0 << 16, DYN_POS_NONE: skipped), item (s, f) at dpos[s dpos_ld + f] */
    const uint32_t *dpos;
    uint32_t dpos_ld;
    /* DynGeom.pos_mask of that table (0: as 0xffff).  At 0xff an entry's high
     * bytes hold (w - w_f) / 16 and (h - h_f) / 16: the item
     * then crops w_f x h_f pixels into the layout of a w_f x h_f picture at
     * the head of its block, whose stride stays dst_fr */
    uint32_t pos_mask;
    int32_t x0, y0;
    uint32_t w, h;
    uint32_t S, nframes;
    uint32_t cropped;           /* 1: every window starts at its surface's origin; pos only says which items to skip */
    scroll::csc::Coef k;
} CscJob;

/* the job's patches of 8 x 2 pixels: one launch takes at most CSC_MAX_TASKS
 * (2^35 pixels), so that the task index and its grid stride stay 32-bit */
#define CSC_MAX_TASKS ((uint64_t)1 << 31)
static inline uint64_t csc_tasks(const CscJob *job)
{
    return (uint64_t)job->S * job->nframes * (job->h / 2u) * (job->w / 8u);
}

/* Returns 0, or -1 when the job is larger than that or the launch failed. */
int csc_launch(hipStream_t hs, const CscJob *job);

#endif
