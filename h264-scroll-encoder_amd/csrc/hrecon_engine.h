/*
 * hrecon_engine.h -- engine-internal launcher of the dynamic rect's
 * reconstruction under UI hints (hrecon_kernels.hip), used by the batch
 * engine (batch_core.hip) when scroll_batch_set_dyn_recon_hinted is on.
 */
#ifndef SCROLL_HRECON_ENGINE_H
#define SCROLL_HRECON_ENGINE_H

#include <hip/hip_runtime.h>
#include "engine.h"
#include "splice_engine.h"

/* zeroes sse ([S][ld_fr][3], Y / Cb / Cr) and runs k_hdyn_recon over frames
 * [0, nframes) of S streams on hs, after k_hint_fb set the frames' fallback
 * bits there: the decoded rect of every frame k_hdyn_code codes (hf, pool,
 * spf as it takes them) into rec (the source's layout and strides,
 * DynGeom.src_ld / src_fr) and its squared error against src.  ev0 / ev1 !=
 * NULL: recorded right before / after the kernels.  Returns 0, or -1 when a
 * launch failed. */
int hrecon_launch(hipStream_t hs, int nframes, int S, const DevStream *st, const NalDesc *nal, int ld_nal,
                  const PlanPending *pend, const DynFrame *dfr, int ld_fr, const HintFrame *hf,
                  const ScrollHintRect *pool, const SpliceFrame *spf, const DynGeom *g, const uint8_t *src,
                  const uint8_t *refs, uint8_t *rec, unsigned long long *sse, hipEvent_t ev0, hipEvent_t ev1);

#endif
