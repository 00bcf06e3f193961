/*
 * pick_engine.h -- engine-internal launcher of k_dyn_pick (pick_kernels.hip),
 * used by the batch engine (batch_rate.hip).
 */
#ifndef SCROLL_PICK_ENGINE_H
#define SCROLL_PICK_ENGINE_H

#include <hip/hip_runtime.h>
#include "engine.h"

/* what k_dyn_pick leaves per (stream, frame) [s ld_fr + f] beside the table entry */
typedef struct {
    uint8_t k;                      /* the chosen candidate (status 0 / 1) */
    uint8_t qp;                     /* its QP */
    uint8_t status;                 /* PICK_* (pick_device.h) */
    uint8_t pad;
} PickOut;

/* k_dyn_pick over the first nframes frames of S streams, from the last plain
 * probe's results (res, SCROLL_DYN_PROBE_MAX_QPS per frame), its DynFrames
 * (dfr: nal < 0, no dynamic NAL) and row counters (done; h rows complete a
 * frame), at the probe's nq candidates qps.  fb: frame_bits per stream, or
 * NULL for rate->frame_bits; level: the buckets' levels per stream (bucket
 * mode reads and writes them).  Writes qpf[s ld_fr + f] (the chosen QP, or
 * 0xFF) and out.  Returns 0, or -1 when the launch failed. */
int pick_launch(hipStream_t hs, int nframes, int S, const DevStream *st, const DynFrame *dfr, int ld_fr,
                const ScrollDynProbe *res, const uint32_t *done, int h, const uint8_t *qps, int nq,
                const ScrollDynRate *rate, const uint32_t *fb, long long *level, uint8_t *qpf, PickOut *out);

#endif
