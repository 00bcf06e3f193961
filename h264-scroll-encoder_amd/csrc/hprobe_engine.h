/*
 * hprobe_engine.h -- engine-internal launcher of the QP probe of the dynamic
 * rect under UI hints (hprobe_kernels.hip), used by the batch engine
 * (batch_dyn.hip) for scroll_batch_dyn_probe_hinted.
 */
#ifndef SCROLL_HPROBE_ENGINE_H
#define SCROLL_HPROBE_ENGINE_H

#include <hip/hip_runtime.h>
#include "engine.h"
#include "probe_engine.h"
#include "splice_engine.h"

/* k_hprobe_class's answer per frame: what the next compose would make of it */
#define HPROBE_NONE 0               /* no dynamic NAL, no rect, or a dormant fallback region: nothing to probe */
#define HPROBE_HINT 1               /* the rect under its hint rects */
#define HPROBE_FB 2                 /* the frame falls back: the whole-picture region, no hint rects */
#define HPROBE_FAIL 3               /* a hint rect names a reference the frame lacks, the fallback off */

/* zeroes res ([S][ld_fr][SCROLL_DYN_PROBE_MAX_QPS]) and done ([S][ld_fr]),
 * classes every frame [0, nframes) of S streams into cls ([S][ld_fr];
 * k_hprobe_class: HintFrame.mode is read, never written) and runs
 * k_hdyn_probe over the HPROBE_HINT / HPROBE_FB frames on hs: per frame and
 * candidate the squared error, bits and non-zero levels of the rect at its
 * hinted motion, and in done[] the rect rows counted (g->h when the frame is
 * complete).  hf, pool, spf as k_hdyn_code takes them; nal, pend, dfr from a
 * k_plan state pass.  ev1 != NULL: recorded right after the kernels.
 * Returns 0, or -1 when a launch failed. */
int hprobe_launch(hipStream_t hs, int nframes, int S, const DevStream *st, const NalDesc *nal, int ld_nal,
                  const PlanPending *pend, const DynFrame *dfr, int ld_fr, const HintFrame *hf,
                  const ScrollHintRect *pool, const SpliceFrame *spf, int fallback, const DynGeom *g,
                  const uint8_t *src, const uint8_t *refs, const ProbeQps *q, uint8_t *cls, ScrollDynProbe *res,
                  uint32_t *done, hipEvent_t ev1);

#endif
