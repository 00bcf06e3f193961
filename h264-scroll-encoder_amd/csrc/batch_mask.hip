/*
 * batch_mask.hip -- the batch engine's per-MB source mask (batch.h): the
 * dynamic rect's MBs compared with the prediction a decoder forms for them,
 * and the source of the unchanged ones replaced by it
 * (scroll_batch_dyn_mask; k_dyn_mask_diff, k_dyn_mask_fill, k_dyn_mask_rec,
 * mask_kernels.hip; the rule: mask_device.h), and its results.
 */
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "batch.h"
#include "mask_device.h"
#include "mask_engine.h"

using namespace scroll::batch;

namespace scroll {
namespace batch {

void mask_release(ScrollBatch *b)
{
    ScrollBatch::Mask &m = b->mk;
    pass_release(&m.run);
    dry_plan_free(&m.plan);
    pred_rows_free(&m.pr);
    (void)hipFree(m.map);
    (void)hipFree(m.part);
    (void)hipFree(m.res);
    m = ScrollBatch::Mask{};
}

}  // namespace batch
}  // namespace scroll

static size_t mask_frame_words(const ScrollBatch *b) { return (size_t)2 * b->geo.w * b->geo.h; }

static int mask_alloc(ScrollBatch *b, const char *who)
{
    ScrollBatch::Mask &m = b->mk;
    if (m.res) return SCROLL_OK;
    const size_t NF = (size_t)b->max_streams * (size_t)b->max_frames, h = (size_t)b->geo.h;
    hipError_t e = dry_plan_alloc(b, &m.plan);
    if (e == hipSuccess) e = pred_rows_alloc(b, &m.pr);
    if (e == hipSuccess) e = hipMalloc(&m.map, NF * mask_frame_words(b) * sizeof(uint32_t));
    if (e == hipSuccess) e = hipMalloc(&m.part, NF * h * 2 * sizeof(unsigned long long));
    if (e == hipSuccess) e = hipMalloc(&m.res, NF * sizeof(ScrollDynMask));
    if (e == hipSuccess) e = hipMemset(m.map, 0, NF * mask_frame_words(b) * sizeof(uint32_t));
    if (e == hipSuccess) e = hipMemset(m.res, 0, NF * sizeof(ScrollDynMask));
    if (e == hipSuccess) e = hipEventCreateWithFlags(&m.run.fin, hipEventDisableTiming);
    if (e != hipSuccess) {
        mask_release(b);
        return hip_fail(who, e, true);
    }
    return SCROLL_OK;
}

extern "C" {

int scroll_batch_dyn_mask(ScrollBatch *b, int nframes, const ScrollDynMaskRule *rule, void *hip_stream)
{
    const char *who = "scroll_batch_dyn_mask";
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
        set_err("%s: masks the plain dynamic rect, not the rect under UI hints: clear the hints", who);
        return SCROLL_ERR_CONFIG;
    }
    if (nframes < 0 || nframes > b->max_frames) {
        set_err("%s: nframes %d out of range", who, nframes);
        return SCROLL_ERR_ARG;
    }
    if (rule->grow > scroll::mask::MAX_GROW || rule->apply > 1u) {
        set_err("%s: grow %u above 2 or apply %u not 0 / 1", who, rule->grow, rule->apply);
        return SCROLL_ERR_ARG;
    }
    const int S = b->nstreams, ld_fr = b->max_frames;
    MaskJob job{};
    job.g = b->geo;
    job.S = (uint32_t)S;
    job.nframes = (uint32_t)nframes;
    if (mask_tasks(&job) >= MASK_MAX_TASKS) {
        set_err("%s: more than 2^31 spans of 16 MBs in one call: mask fewer frames at a time", who);
        return SCROLL_ERR_ARG;
    }
    if (nframes == 0 || S == 0) return SCROLL_OK;
    HIPCHK(hipSetDevice(b->device));
    int rc = mask_alloc(b, who);
    if (rc) return rc;
    ScrollBatch::Mask &m = b->mk;
    hipStream_t hs = hip_stream ? (hipStream_t)hip_stream : b->own;
    const bool timed = b->timing != 0;
    if ((rc = pass_begin(b, &m.run, 4, hs))) return rc;

    /* the compose's state pass, dry, and k_dyn_rows after it, as the QP probe
     * runs them (probe_run): into the mask's own DryPlan and PredRows, nothing
     * committed.  Moving rects: the frames' own origins, and no dynamic NAL
     * where there is no rect */
    DynGeom G = b->geo;
    G.debug = b->debug;
    if ((rc = dyn_pos_table(b, hs, &G.dpos))) return rc;
    if ((rc = dry_plan_launch(b, hs, nframes, m.plan, 0, m.pr.ctr, G.dpos))) return rc;
    /* (no per-frame QP table: the prediction does not depend on the QP) */
    if ((rc = pred_rows_launch(b, hs, nframes, m.plan, m.pr, &G))) return rc;
    job.st = b->d_st;
    job.nal = m.plan.nal;
    job.pend = m.plan.pend;
    job.dfr = m.plan.dfr;
    job.rows = m.pr.rows;
    job.ctr = m.pr.ctr;
    job.src = b->d_src;
    job.refs = b->d_refs;
    job.map = m.map;
    job.part = m.part;
    job.res = m.res;
    job.g = G;
    job.ld_nal = b->ld_nal;
    job.ld_fr = ld_fr;
    job.rule = *rule;
    if (mask_launch(hs, &job, timed ? m.run.ev[1] : nullptr, timed ? m.run.ev[2] : nullptr)) {
        set_err("k_dyn_mask launch: %s", hipGetErrorString(hipGetLastError()));
        return SCROLL_ERR_HIP;
    }
    return pass_end(b, &m.run, hs, nframes, S);
}

int scroll_batch_dyn_mask_result(ScrollBatch *b, int s, int f, ScrollDynMask *out)
{
    if (!b || !out) return SCROLL_ERR_ARG;
    int rc = pass_frame_arg(b, &b->mk.run, s, f, "scroll_batch_dyn_mask_result", "mask", "scroll_batch_dyn_mask");
    if (rc) return rc;
    HIPCHK(hipMemcpy(out, b->mk.res + (size_t)s * b->max_frames + f, sizeof(*out), hipMemcpyDeviceToHost));
    return SCROLL_OK;
}

const ScrollDynMask *scroll_batch_dyn_mask_device(ScrollBatch *b, size_t *stream_stride)
{
    if (!b || !b->mk.res) return nullptr;
    if (stream_stride) *stream_stride = (size_t)b->max_frames * sizeof(ScrollDynMask);
    return b->mk.res;
}

int scroll_batch_dyn_mask_map(ScrollBatch *b, int s, int f, uint32_t *dst)
{
    if (!b || !dst) return SCROLL_ERR_ARG;
    int rc = pass_frame_arg(b, &b->mk.run, s, f, "scroll_batch_dyn_mask_map", "mask", "scroll_batch_dyn_mask");
    if (rc) return rc;
    const size_t n = mask_frame_words(b);
    HIPCHK(hipMemcpy(dst, b->mk.map + ((size_t)s * b->max_frames + f) * n, n * sizeof(uint32_t),
                     hipMemcpyDeviceToHost));
    return SCROLL_OK;
}

const uint32_t *scroll_batch_dyn_mask_map_device(ScrollBatch *b, size_t *stream_stride, size_t *frame_stride)
{
    if (!b || !b->mk.map) return nullptr;
    const size_t fr = mask_frame_words(b) * sizeof(uint32_t);
    if (frame_stride) *frame_stride = fr;
    if (stream_stride) *stream_stride = (size_t)b->max_frames * fr;
    return b->mk.map;
}

float scroll_batch_dyn_mask_ms(ScrollBatch *b) { return b ? pass_span_ms(b, &b->mk.run, 0, 3) : -1.0f; }

float scroll_batch_dyn_mask_kernel_ms(ScrollBatch *b) { return b ? pass_span_ms(b, &b->mk.run, 1, 2) : -1.0f; }

}  // extern "C"
