/*
 * batch_damage.hip -- the batch engine's locate (batch.h): the dynamic rect's
 * position found on the device from the renderer's surfaces
 * (scroll_batch_dyn_locate; k_dmg_rows, k_dyn_damage, k_dyn_place,
 * damage_kernels.hip; the rule: damage_device.h), its results, and the
 * read-back of positions the device has written.
 */
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "batch.h"
#include "csc_device.h"
#include "damage_engine.h"
#include "dyn_pos.h"            /* dyn_pos_unpack: the position table's word */

using namespace scroll::batch;

namespace scroll {
namespace batch {

void locate_release(ScrollBatch *b)
{
    ScrollBatch::Locate &l = b->lc;
    pass_release(&l.run);
    dry_plan_free(&l.plan);
    (void)hipFree(l.rows);
    (void)hipFree(l.map);
    (void)hipFree(l.res);
    l = ScrollBatch::Locate{};
    b->dpos_dev = 0;
}

/* the per-frame QP table's precedent (batch_rate.hip, table_refresh): the
 * device wrote, so the host's copy is read back before anything reads it */
int dyn_pos_refresh(ScrollBatch *b)
{
    if (!b->dpos_dev) return SCROLL_OK;
    HIPCHK(hipSetDevice(b->device));
    HIPCHK(hipEventSynchronize(b->dpos_ev));            /* the locate that wrote last */
    const size_t n = (size_t)b->max_streams * b->max_frames;
    b->h_dpos.resize(n);
    HIPCHK(hipMemcpy(b->h_dpos.data(), b->d_dpos, n * sizeof(uint32_t), hipMemcpyDeviceToHost));
    bool any = false;
    size_t sized = 0;
    for (size_t i = 0; i < n; ++i) {
        const uint32_t e = b->h_dpos[i];
        const DynPosWord p = dyn_pos_unpack(e == DYN_POS_NONE ? 0u : e, b->geo.pos_mask);
        const int32_t x = e == DYN_POS_NONE ? -1 : p.x0, y = e == DYN_POS_NONE ? -1 : p.y0;
        b->h_dyn_pos[2 * i] = x;
        b->h_dyn_pos[2 * i + 1] = y;
        any |= x != b->geo.x0 || (x >= 0 && y != b->geo.y0);
        /* the size a locate with size = 1 gave the frame (only a batch whose
         * row stage is sized for it gets such entries: dsz_on) */
        if (!b->h_dyn_dsz.empty()) {
            b->h_dyn_dsz[2 * i] = (uint8_t)p.dw;
            b->h_dyn_dsz[2 * i + 1] = (uint8_t)p.dh;
            sized += (p.dw | p.dh) != 0 ? 1 : 0;
        }
    }
    b->dsz_nz = sized;
    b->dsz_any = sized ? 1 : 0;
    any |= sized != 0;
    /* host and device agree again: nothing to upload */
    b->dyn_pos_custom = any ? 1 : 0;
    b->dpos_any = any ? 1 : 0;
    b->dpos_stale = 0;
    b->dpos_dev = 0;
    b->hd_dirty = 1;
    b->hint_dirty = 1;
    return SCROLL_OK;
}

}  // namespace batch
}  // namespace scroll

static int locate_alloc(ScrollBatch *b, const char *who)
{
    ScrollBatch::Locate &l = b->lc;
    if (l.res) return SCROLL_OK;
    const size_t NF = (size_t)b->max_streams * (size_t)b->max_frames;
    const size_t nmb = (size_t)(b->dyn_pw / 16) * (b->dyn_ph / 16);
    hipError_t e = dry_plan_alloc(b, &l.plan);
    if (e == hipSuccess) e = hipMalloc(&l.rows, NF * (size_t)b->dyn_ph * sizeof(uint32_t));
    if (e == hipSuccess) e = hipMalloc(&l.map, NF * nmb * sizeof(uint32_t));
    if (e == hipSuccess) e = hipMalloc(&l.res, NF * sizeof(ScrollDynDamage));
    if (e == hipSuccess) e = hipMemset(l.map, 0, NF * nmb * sizeof(uint32_t));
    if (e == hipSuccess) e = hipMemset(l.res, 0, NF * sizeof(ScrollDynDamage));
    if (e == hipSuccess) e = hipEventCreateWithFlags(&l.run.fin, hipEventDisableTiming);
    if (e != hipSuccess) {
        locate_release(b);
        return hip_fail(who, e, true);
    }
    return SCROLL_OK;
}

extern "C" {

int scroll_batch_dyn_locate(ScrollBatch *b, int nframes, const ScrollSurfaces *surf, const ScrollDynLocate *rule,
                            void *hip_stream)
{
    const char *who = "scroll_batch_dyn_locate";
    if (!b || !rule) {
        set_err("%s: no batch or no rule", who);
        return SCROLL_ERR_ARG;
    }
    if (!b->dyn_on || !b->dyn_refs) {
        set_err("%s: needs a dynamic rect with reference pictures "
                "(scroll_batch_set_dyn_rect, scroll_batch_set_dyn_refs)", who);
        return SCROLL_ERR_CONFIG;
    }
    if (b->hint_on) {
        set_err("%s: locates the plain dynamic rect, not the rect under UI hints: clear the hints", who);
        return SCROLL_ERR_CONFIG;
    }
    if (nframes < 0 || nframes > b->max_frames) {
        set_err("%s: nframes %d out of range", who, nframes);
        return SCROLL_ERR_ARG;
    }
    if (rule->margin > 4u || rule->apply > 1u) {
        set_err("%s: margin %u above 4 or apply %u not 0 / 1", who, rule->margin, rule->apply);
        return SCROLL_ERR_ARG;
    }
    if (rule->size > 1u || (rule->size && !rule->apply)) {
        set_err("%s: size %u not 0 / 1, or size = 1 without apply = 1 (a size is placed with its origin)", who,
                rule->size);
        return SCROLL_ERR_ARG;
    }
    const int rc = surf_args(who, surf, (uint64_t)b->dyn_pw, true);
    if (rc) return rc;
    if (surf->cropped) {
        set_err("%s: the surfaces are whole pictures (cropped = 1: there is nothing outside the rect to look at)", who);
        return SCROLL_ERR_ARG;
    }
    if (rule->apply && !b->dyn_moving) {
        set_err("%s: apply = 1 places the rect per frame: needs scroll_batch_set_dyn_rect_moving", who);
        return SCROLL_ERR_CONFIG;
    }
    if (rule->size) {
        /* the row stage for every h_f, once (no later locate allocates) */
        const int sr = dyn_sizes_enable(b, who);
        if (sr) return sr;
    }
    const int S = b->nstreams, ld_fr = b->max_frames;
    const uint32_t mbw = (uint32_t)b->dyn_pw / 16u, mbh = (uint32_t)b->dyn_ph / 16u;
    DmgJob job{};
    job.src = surf->base;
    job.pitch = surf->pitch;
    job.src_fr = surf->frame_stride;
    job.src_ld = surf->stream_stride;
    job.refs = b->d_refs;
    job.ref_ld = b->geo.ref_ld;
    job.ld_fr = (uint32_t)ld_fr;
    job.mbw = mbw;
    job.mbh = mbh;
    job.S = (uint32_t)S;
    job.nframes = (uint32_t)nframes;
    job.k = scroll::csc::coef(surf->format, surf->matrix, surf->full_range);
    if (dmg_tasks(&job) >= DMG_MAX_TASKS) {
        set_err("%s: more than 2^31 spans of 16 MBs in one call: locate fewer frames at a time", who);
        return SCROLL_ERR_ARG;
    }
    if (nframes == 0 || S == 0) return SCROLL_OK;
    HIPCHK(hipSetDevice(b->device));
    int rr = locate_alloc(b, who);
    if (rr) return rr;
    ScrollBatch::Locate &l = b->lc;
    hipStream_t hs = hip_stream ? (hipStream_t)hip_stream : b->own;
    if ((rr = pass_begin(b, &l.run, 4, hs))) return rr;

    uint32_t *dpos = nullptr;
    if (rule->apply) {
        /* the table the kernel writes into must hold the host's entries from
         * nframes on: unless the device owns it already, it is packed and
         * uploaded whole (dyn_pos_table uploads only a table that differs) */
        if (!b->dpos_dev) {
            if (b->dpos_hs) HIPCHK(hipEventSynchronize(b->dpos_ev));   /* the last upload has read its source */
            const size_t n = (size_t)b->max_streams * b->max_frames;
            b->h_dpos.resize(n);
            for (size_t i = 0; i < n; ++i) {
                b->h_dpos[i] = dyn_pos_word(b, i);
            }
            HIPCHK(hipMemcpyAsync(b->d_dpos, b->h_dpos.data(), n * sizeof(uint32_t), hipMemcpyHostToDevice, hs));
        } else if (hs != b->dpos_hs) {
            HIPCHK(hipStreamWaitEvent(hs, b->dpos_ev, 0));             /* the last locate, on another stream */
        }
        dpos = b->d_dpos;
    }

    /* the compose's state pass, dry, as the QP probe runs it (probe_run):
     * into the locate's own DryPlan, nothing committed.  No position table:
     * every frame with a scroll NAL has DynFrame.nal >= 0, wherever its rect
     * was before */
    if ((rr = dry_plan_launch(b, hs, nframes, l.plan))) return rr;
    if (dmg_launch_rows(hs, nframes, S, b->d_st, l.plan.nal, b->ld_nal, l.plan.pend, l.plan.dfr, ld_fr, b->dyn_ph,
                        l.rows)) {
        set_err("k_dmg_rows launch: %s", hipGetErrorString(hipGetLastError()));
        return SCROLL_ERR_HIP;
    }
    job.rows = l.rows;
    job.dfr = l.plan.dfr;
    job.map = l.map;
    if ((rr = pass_mark(b, &l.run, 1, hs))) return rr;
    if (dmg_launch_damage(hs, &job)) {
        set_err("k_dyn_damage launch: %s", hipGetErrorString(hipGetLastError()));
        return SCROLL_ERR_HIP;
    }
    if ((rr = pass_mark(b, &l.run, 2, hs))) return rr;
    if (dmg_launch_place(hs, nframes, S, l.plan.dfr, ld_fr, l.map, mbw, mbh, (uint32_t)b->geo.w, (uint32_t)b->geo.h,
                         rule, l.res, dpos)) {
        set_err("k_dyn_place launch: %s", hipGetErrorString(hipGetLastError()));
        return SCROLL_ERR_HIP;
    }
    if ((rr = pass_end(b, &l.run, hs, nframes, S))) return rr;
    if (dpos) {
        /* from here the device's table is the truth (dyn_pos_table hands it
         * out as it is; dyn_pos_refresh brings the host's copy up to date) */
        HIPCHK(hipEventRecord(b->dpos_ev, hs));
        b->dpos_hs = hs;
        b->dpos_any = 1;
        b->dpos_stale = 0;
        b->dpos_dev = 1;
    }
    return SCROLL_OK;
}

int scroll_batch_dyn_locate_result(ScrollBatch *b, int s, int f, ScrollDynDamage *out)
{
    if (!b || !out) return SCROLL_ERR_ARG;
    int rc = pass_frame_arg(b, &b->lc.run, s, f, "scroll_batch_dyn_locate_result", "locate", "scroll_batch_dyn_locate");
    if (rc) return rc;
    HIPCHK(hipMemcpy(out, b->lc.res + (size_t)s * b->max_frames + f, sizeof(*out), hipMemcpyDeviceToHost));
    return SCROLL_OK;
}

const ScrollDynDamage *scroll_batch_dyn_locate_device(ScrollBatch *b, size_t *stream_stride)
{
    if (!b || !b->lc.res) return nullptr;
    if (stream_stride) *stream_stride = (size_t)b->max_frames * sizeof(ScrollDynDamage);
    return b->lc.res;
}

int scroll_batch_dyn_damage_map(ScrollBatch *b, int s, int f, uint32_t *dst)
{
    if (!b || !dst) return SCROLL_ERR_ARG;
    int rc = pass_frame_arg(b, &b->lc.run, s, f, "scroll_batch_dyn_damage_map", "locate", "scroll_batch_dyn_locate");
    if (rc) return rc;
    const size_t nmb = (size_t)(b->dyn_pw / 16) * (b->dyn_ph / 16);
    HIPCHK(hipMemcpy(dst, b->lc.map + ((size_t)s * b->max_frames + f) * nmb, nmb * sizeof(uint32_t),
                     hipMemcpyDeviceToHost));
    return SCROLL_OK;
}

const uint32_t *scroll_batch_dyn_damage_map_device(ScrollBatch *b, size_t *stream_stride, size_t *frame_stride)
{
    if (!b || !b->lc.map) return nullptr;
    const size_t fr = (size_t)(b->dyn_pw / 16) * (b->dyn_ph / 16) * sizeof(uint32_t);
    if (frame_stride) *frame_stride = fr;
    if (stream_stride) *stream_stride = (size_t)b->max_frames * fr;
    return b->lc.map;
}

float scroll_batch_dyn_locate_ms(ScrollBatch *b) { return b ? pass_span_ms(b, &b->lc.run, 0, 3) : -1.0f; }

float scroll_batch_dyn_locate_kernel_ms(ScrollBatch *b) { return b ? pass_span_ms(b, &b->lc.run, 1, 2) : -1.0f; }

}  // extern "C"
