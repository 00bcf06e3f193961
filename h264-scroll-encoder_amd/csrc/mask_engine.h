/*
 * mask_engine.h -- engine-internal launcher of the source-mask kernels
 * (mask_kernels.hip), used by the batch engine (batch_mask.hip).
 */
#ifndef SCROLL_MASK_ENGINE_H
#define SCROLL_MASK_ENGINE_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "engine.h"
#include "composer_batch.h"

/* One mask: frames [0, nframes) of S streams, after a dry plan (nal, pend,
 * dfr) and k_dyn_rows (rows, ctr: the general-path frames listed) into the
 * mask's own buffers.  For every MB of every frame's g.w x g.h rect the pair
 * { Dy, Dc | kept } goes to map[((s ld_fr + f) g.h + my) g.w + mx][2]; with
 * rule.apply the source of the MBs not kept (src + s g.src_ld + f g.src_fr,
 * the rect as I420) is overwritten by their prediction; part[(s ld_fr + f)
 * g.h + r][2]: the Cb / Cr squared error of rect row r's MBs not kept;
 * res[s ld_fr + f]: the record.  Frames whose dfr[].nal < 0: zero entries,
 * a NOFRAME record, nothing else touched.
 * A frame sized on its own (g.dpos) is, inside its own
 * blocks, a batch whose rect is w_f x h_f: its map block starts at (s ld_fr
 * + f) g.ld_h g.ld_w pairs and holds [my w_f + mx], its part rows start at
 * (s ld_fr + f) g.ld_h; the rest of either block is not written.  g.w, g.h
 * here are the batch's (= g.ld_w, g.ld_h): they size the launch. */
typedef struct {
    const DevStream *st;
    const NalDesc *nal;
    const PlanPending *pend;
    const DynFrame *dfr;
    const uint32_t *rows;
    const uint32_t *ctr;
    uint8_t *src;
    const uint8_t *refs;
    uint32_t *map;
    unsigned long long *part;
    ScrollDynMask *res;
    DynGeom g;
    int32_t ld_nal, ld_fr;
    uint32_t S, nframes;
    ScrollDynMaskRule rule;
} MaskJob;

/* the difference kernel's tasks (a span of 16 MBs of one rect row each): one
 * launch takes fewer than 2^31, so that the task index stays 32-bit */
static inline uint64_t mask_tasks(const MaskJob *job)
{
    return (uint64_t)job->S * job->nframes * (uint32_t)job->g.h * (((uint32_t)job->g.w + 15u) / 16u);
}
#define MASK_MAX_TASKS ((uint64_t)1 << 31)

#pragma GCC visibility push(hidden)

/* k_dyn_mask_diff, k_dyn_mask_fill (both in their two instantiations: plain
 * rows, rows behind a half-pel waypoint chain) and k_dyn_mask_rec; ev0 / ev1
 * (or NULL) are recorded around k_dyn_mask_diff.  0, or -1 when a launch
 * failed or the job is too large */
int mask_launch(hipStream_t hs, const MaskJob *job, hipEvent_t ev0, hipEvent_t ev1);

#pragma GCC visibility pop

#endif
