/*
 * recon_engine.h -- engine-internal launcher of the dynamic rect's
 * reconstruction kernel (recon_kernels.hip), used by the batch engine
 * (batch_core.hip) when scroll_batch_set_dyn_recon is on.
 */
#ifndef SCROLL_RECON_ENGINE_H
#define SCROLL_RECON_ENGINE_H

#include <hip/hip_runtime.h>
#include "engine.h"

/* zeroes sse ([S][ld_fr][3], Y / Cb / Cr) and runs k_dyn_recon over frames
 * [0, nframes) of S streams on hs, after k_dyn_rows wrote rows[] there: the
 * decoded rect of every dynamic NAL into rec (the source's layout and
 * strides, DynGeom.src_ld / src_fr) and its squared error against src.
 * ctr: DynScratch.ctr, the general-path frames k_dyn_rows listed (the rows
 * with a half-pel waypoint chain run in a second instantiation over them).
 * ev0 / ev1 != NULL: recorded right before / after the kernels.  Returns 0,
 * or -1 when a launch failed. */
int recon_launch(hipStream_t hs, int nframes, int S, const DevStream *st, const NalDesc *nal, int ld_nal,
                 const PlanPending *pend, const DynFrame *dfr, int ld_fr, const DynGeom *g,
                 const uint32_t *rows, const uint8_t *src, const uint8_t *refs, uint8_t *rec,
                 unsigned long long *sse, const uint32_t *ctr, hipEvent_t ev0, hipEvent_t ev1);

#endif
