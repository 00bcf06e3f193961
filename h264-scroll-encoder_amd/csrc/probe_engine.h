/*
 * probe_engine.h -- engine-internal launcher of the dynamic rect's QP probe
 * (probe_kernels.hip), used by the batch engine (batch_dyn.hip) for
 * scroll_batch_dyn_probe.
 */
#ifndef SCROLL_PROBE_ENGINE_H
#define SCROLL_PROBE_ENGINE_H

#include <hip/hip_runtime.h>
#include "engine.h"

/* the candidate QPs of one probe, by value into the kernel */
typedef struct {
    int32_t n;
    uint8_t qp[SCROLL_DYN_PROBE_MAX_QPS];
} ProbeQps;

/* zeroes res ([S][ld_fr][SCROLL_DYN_PROBE_MAX_QPS]) and done ([S][ld_fr]) and
 * runs k_dyn_probe over frames [0, nframes) of S streams on hs, after
 * k_dyn_rows wrote rows[] and listed the general-path frames in ctr there:
 * per frame and candidate the squared error, bits and non-zero levels of
 * the rect (ScrollDynProbe), and in done[] the rect rows counted (g->h when
 * the frame is complete).  ev0 / ev1 != NULL: recorded right before / after
 * the kernels.  Returns 0, or -1 when a launch failed. */
int probe_launch(hipStream_t hs, int nframes, int S, const DevStream *st, const NalDesc *nal, int ld_nal,
                 const PlanPending *pend, const DynFrame *dfr, int ld_fr, const DynGeom *g,
                 const uint32_t *rows, const uint8_t *src, const uint8_t *refs, const ProbeQps *q,
                 ScrollDynProbe *res, uint32_t *done, const uint32_t *ctr, hipEvent_t ev0, hipEvent_t ev1);

#endif
