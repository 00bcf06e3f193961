/*
 * scroll_engine.h -- engine-internal launchers of the plan, emit and
 * host-delivery kernels (scroll_kernels.hip), used by the batch engine
 * (batch_core.hip, batch_dyn.hip).
 */
#ifndef SCROLL_SCROLL_ENGINE_H
#define SCROLL_SCROLL_ENGINE_H

#include <hip/hip_runtime.h>
#include "engine.h"

/* k_plan's flags, above the SCROLL_DEBUG_* bits they are or-ed with */
constexpr int PLAN_REWIND = 1 << 8;   /* k_plan flag: arena restarts at 0 */
constexpr int PLAN_STATE = 1 << 9;    /* phase 1 only -> PlanPending (dynamic rect)   */
constexpr int PLAN_SIZE = 1 << 10;    /* phase 2 only, from PlanPending              */
constexpr int PLAN_DYN = 1 << 11;     /* scroll NALs carry the dynamic rect          */

#pragma GCC visibility push(hidden)

/* they launch and leave the launch's error to the caller (hipGetLastError) */
/* k_plan, one workgroup per stream.  The plain call stops at ld_fr; the
 * state pass (PLAN_STATE) names in ctr_zero the dynamic rect's counters to
 * zero; the size pass (PLAN_SIZE) names them in pool_ctr, with the pools'
 * caps, to fail the compose that ran out of one.  dpos (both passes of a
 * compose with moving rects, DynGeom.dpos): the frames whose entry is
 * DYN_POS_NONE get no dynamic NAL (DynFrame.nal = -1, their scroll NAL plain) */
void scroll_launch_plan(hipStream_t hs, int S, DevStream *st, const int32_t *offs, int ld_off, NalDesc *nal,
                        int ld_nal, int nframes, int mode, int flags, PlanPending *pend, DynFrame *dfr, int ld_fr,
                        const uint32_t *pool_ctr = nullptr, uint32_t spill_cap = 0, uint32_t gen_cap = 0,
                        uint32_t *ctr_zero = nullptr, const uint32_t *dpos = nullptr);
/* k_emit over up to nal_max NALs per stream; nothing when that is none */
void scroll_launch_emit(hipStream_t hs, int S, int nal_max, const DevStream *st, const NalDesc *nal, int ld_nal,
                        uint8_t *arena, uint64_t ld_arena, int flags, uint64_t *dbg);
/* 8-word stamp slots that launch fills in dbg under SCROLL_DEBUG_EMIT_STAMPS */
size_t scroll_emit_stamp_slots(int nal_max, int S);
/* k_out_table (one workgroup), then k_out_copy over S > 0 streams */
void scroll_launch_out_table(hipStream_t hs, DevStream *st, int S, uint64_t cap, uint64_t *dtab, uint64_t *htab);
void scroll_launch_out_copy(hipStream_t hs, const DevStream *st, int S, const uint8_t *arena, uint64_t ld_arena,
                            uint64_t arena_end, const uint64_t *dtab, uint8_t *dst);

#pragma GCC visibility pop

#endif
