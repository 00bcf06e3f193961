/*
 * detect_engine.h -- engine-internal launchers of the offset detector's
 * kernels (detect_kernels.hip), used by the batch engine (batch_detect.hip).
 */
#ifndef SCROLL_DETECT_ENGINE_H
#define SCROLL_DETECT_ENGINE_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "composer_batch.h"
#include "csc_device.h"

/* One detection: for every item (s, f), s < S, f < nframes, the pw x ph
 * surface at src + s src_ld + f src_fr (rows pitch bytes apart; all multiples
 * of 16) against the stream's reference pair at refs + s ref_ld (luma of A at
 * 0, of B at pic bytes; ref_ld 0: one pair for every stream).
 *   sig_s  [(s ld_fr + f) ph + Y][nuse]  uint16, the surface signatures
 *   sig_r  [s' nuse + cu][2 ph]          uint16, the reference signatures,
 *          segment-major; s' = s, or 0 with a shared pair
 *   scores [(s ld_fr + f)][ph + 1], res [s ld_fr + f]; off [s ld_fr + f] is
 *   the estimate and, with rule.apply, where a FOUND frame's offset goes */
typedef struct {
    const uint8_t *src;
    uint64_t pitch, src_fr, src_ld;
    const uint8_t *refs;
    uint64_t ref_ld, pic;
    uint16_t *sig_s, *sig_r;
    uint32_t *scores;
    ScrollOffsetFound *res;
    int32_t *off;
    uint32_t ld_fr;
    uint32_t pw, ph;
    uint32_t S, nframes;
    uint32_t nuse;
    ScrollDetect rule;
    scroll::csc::Coef k;
} DetJob;

/* the surface kernel's tasks (four used segments x 16 rows each): one launch
 * takes fewer than 2^31, which the caller's bound of 2^35 pixels implies (a
 * task covers at least 16 x 16 of them) */
static inline uint64_t det_tasks(const DetJob *job)
{
    return (uint64_t)job->S * job->nframes * (job->ph / 16u) * ((job->nuse + 3u) / 4u);
}
#define DET_MAX_PIXELS ((uint64_t)1 << 35)

#pragma GCC visibility push(hidden)

/* each returns 0, or -1 when the launch failed */
int det_launch_refs(hipStream_t hs, const DetJob *job);     /* k_det_refs: sig_r */
int det_launch_surf(hipStream_t hs, const DetJob *job);     /* k_det_surf: sig_s */
int det_launch_score(hipStream_t hs, const DetJob *job);    /* k_det_score: scores inside the windows */
int det_launch_pick(hipStream_t hs, const DetJob *job);     /* k_det_pick: res, scores outside the windows, off */

#pragma GCC visibility pop

#endif
