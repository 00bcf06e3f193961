/*
 * damage_engine.h -- engine-internal launchers of the locate kernels
 * (damage_kernels.hip), used by the batch engine (batch_damage.hip).
 */
#ifndef SCROLL_DAMAGE_ENGINE_H
#define SCROLL_DAMAGE_ENGINE_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "engine.h"
#include "csc_device.h"

/* One damage map: for every item (s, f), s < S, f < nframes, and every MB of
 * the mbw x mbh picture, the squared luma difference between the surface at
 * src + s src_ld + f src_fr (rows pitch bytes apart; all multiples of 16) and
 * the prediction rows[(s ld_fr + f) 16 mbh + Y] (byte offsets into the
 * stream's reference pair at refs + s ref_ld) goes to map[((s ld_fr + f) mbh
 * + my) mbw + mx]; items whose dfr[s ld_fr + f].nal < 0 get zeroes. */
typedef struct {
    const uint8_t *src;
    uint64_t pitch, src_fr, src_ld;
    const uint8_t *refs;
    uint64_t ref_ld;
    const uint32_t *rows;
    const DynFrame *dfr;
    uint32_t *map;
    uint32_t ld_fr;
    uint32_t mbw, mbh;
    uint32_t S, nframes;
    scroll::csc::Coef k;
} DmgJob;

/* the job's tasks (a span of 16 MBs of one MB row each): one launch takes
 * fewer than 2^31, so that the task index and its grid stride stay 32-bit */
static inline uint64_t dmg_tasks(const DmgJob *job)
{
    return (uint64_t)job->S * job->nframes * job->mbh * ((job->mbw + 15u) / 16u);
}
#define DMG_MAX_TASKS ((uint64_t)1 << 31)

#pragma GCC visibility push(hidden)

/* each returns 0, or -1 when the launch failed (dmg_launch_damage: or the job is too large) */
/* k_dmg_rows: rows[(s ld_fr + f) ph + Y], Y < ph, of every frame with a scroll NAL of the dry plan (nal, pend, dfr) */
int dmg_launch_rows(hipStream_t hs, int nframes, int S, const DevStream *st, const NalDesc *nal, int ld_nal,
                    const PlanPending *pend, const DynFrame *dfr, int ld_fr, int ph, uint32_t *rows);
int dmg_launch_damage(hipStream_t hs, const DmgJob *job);
/* k_dyn_place: res[s ld_fr + f] by the rule of damage_device.h for the w x h
 * rect; dpos (or NULL): the position table's entries of the same frames */
int dmg_launch_place(hipStream_t hs, int nframes, int S, const DynFrame *dfr, int ld_fr, const uint32_t *map,
                     uint32_t mbw, uint32_t mbh, uint32_t w, uint32_t h, const ScrollDynLocate *rule,
                     ScrollDynDamage *res, uint32_t *dpos);

#pragma GCC visibility pop

#endif
