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
#include "scroll_engine.h"
#include "dyn_engine.h"
#include "mask_device.h"
#include "mask_engine.h"

using namespace scroll::batch;

namespace scroll {
namespace batch {

void mask_release(ScrollBatch *b)
{
    ScrollBatch::Mask &m = b->mk;
    if (m.fin) {
        (void)hipEventSynchronize(m.fin);
        (void)hipEventDestroy(m.fin);
    }
    for (hipEvent_t e : m.ev)
        if (e) (void)hipEventDestroy(e);
    (void)hipFree(m.nal);
    (void)hipFree(m.dfr);
    (void)hipFree(m.pend);
    (void)hipFree(m.rows);
    (void)hipFree(m.ctr);
    (void)hipFree(m.heads);
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
    const size_t S = (size_t)b->max_streams, NF = S * (size_t)b->max_frames, h = (size_t)b->geo.h;
    hipError_t e = hipMalloc(&m.nal, S * (size_t)b->ld_nal * sizeof(NalDesc));
    if (e == hipSuccess) e = hipMalloc(&m.dfr, NF * sizeof(DynFrame));
    if (e == hipSuccess) e = hipMalloc(&m.pend, S * sizeof(PlanPending));
    if (e == hipSuccess) e = hipMalloc(&m.rows, NF * 32 * h * sizeof(uint32_t));
    /* the general-frame list holds every frame: it can never run out */
    if (e == hipSuccess) e = hipMalloc(&m.ctr, (DYN_CTR_LIST + NF) * sizeof(uint32_t));
    if (e == hipSuccess) e = hipMalloc(&m.heads, NF * DYN_HEAD_VECS * sizeof(uint4));
    if (e == hipSuccess) e = hipMalloc(&m.map, NF * mask_frame_words(b) * sizeof(uint32_t));
    if (e == hipSuccess) e = hipMalloc(&m.part, NF * h * 2 * sizeof(unsigned long long));
    if (e == hipSuccess) e = hipMalloc(&m.res, NF * sizeof(ScrollDynMask));
    if (e == hipSuccess) e = hipMemset(m.map, 0, NF * mask_frame_words(b) * sizeof(uint32_t));
    if (e == hipSuccess) e = hipMemset(m.res, 0, NF * sizeof(ScrollDynMask));
    if (e == hipSuccess) e = hipEventCreateWithFlags(&m.fin, hipEventDisableTiming);
    if (e != hipSuccess) {
        mask_release(b);
        return hip_fail(who, e, true);
    }
    return SCROLL_OK;
}

/* the frame of the last mask that a result call names; the mask has finished on return */
static int mask_frame_arg(ScrollBatch *b, int s, int f, const char *who)
{
    if (!b) return SCROLL_ERR_ARG;
    ScrollBatch::Mask &m = b->mk;
    if (!m.res || m.nframes < 0) {
        set_err("%s: no mask to read (scroll_batch_dyn_mask; scroll_batch_set_dyn_rect drops it)", who);
        return SCROLL_ERR_CONFIG;
    }
    if (s < 0 || s >= m.nstreams || f < 0 || f >= m.nframes) {
        set_err("%s: stream %d / frame %d outside the last mask", who, s, f);
        return SCROLL_ERR_ARG;
    }
    HIPCHK(hipSetDevice(b->device));
    HIPCHK(hipEventSynchronize(m.fin));
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
    m.timed = 0;
    if (timed && !m.ev[0])
        for (hipEvent_t &e : m.ev) HIPCHK(hipEventCreate(&e));
    if (timed) HIPCHK(hipEventRecord(m.ev[0], hs));

    /* the compose's state pass, dry, and k_dyn_rows after it, as the QP probe
     * runs them (probe_run): into the mask's own NalDesc / DynFrame /
     * PlanPending / rows / heads / ctr, nothing committed.  Moving rects: the
     * frames' own origins, and no dynamic NAL where there is no rect */
    DynGeom G = b->geo;
    G.debug = b->debug;
    G.gen_cap = (uint32_t)((size_t)b->max_streams * ld_fr);
    if ((rc = dyn_pos_table(b, hs, &G.dpos))) return rc;
    const int plan = b->mode == SCROLL_MODE_EXPERIMENT ? SCROLL_PLAN_EXPERIMENT : SCROLL_PLAN_COMPOSER;
    scroll_launch_plan(hs, S, b->d_st, b->d_off, b->max_frames, m.nal, b->ld_nal, nframes, plan,
                       b->debug | PLAN_STATE | PLAN_DYN, m.pend, m.dfr, ld_fr, nullptr, 0u, 0u, m.ctr, G.dpos);
    HIPCHK(hipGetLastError());
    /* (no per-frame QP table: the prediction does not depend on the QP) */
    if (dyn_launch_rows(hs, nframes, S, b->d_st, m.nal, b->ld_nal, m.pend, m.dfr, ld_fr, &G, m.rows, m.ctr, m.heads,
                        nullptr)) {
        set_err("k_dyn_rows launch: %s", hipGetErrorString(hipGetLastError()));
        return SCROLL_ERR_HIP;
    }
    job.st = b->d_st;
    job.nal = m.nal;
    job.pend = m.pend;
    job.dfr = m.dfr;
    job.rows = m.rows;
    job.ctr = m.ctr;
    job.src = b->d_src;
    job.refs = b->d_refs;
    job.map = m.map;
    job.part = m.part;
    job.res = m.res;
    job.g = G;
    job.ld_nal = b->ld_nal;
    job.ld_fr = ld_fr;
    job.rule = *rule;
    if (mask_launch(hs, &job, timed ? m.ev[1] : nullptr, timed ? m.ev[2] : nullptr)) {
        set_err("k_dyn_mask launch: %s", hipGetErrorString(hipGetLastError()));
        return SCROLL_ERR_HIP;
    }
    if (timed) {
        HIPCHK(hipEventRecord(m.ev[3], hs));
        m.timed = 1;
    }
    HIPCHK(hipEventRecord(m.fin, hs));
    m.nframes = nframes;
    m.nstreams = S;
    return SCROLL_OK;
}

int scroll_batch_dyn_mask_result(ScrollBatch *b, int s, int f, ScrollDynMask *out)
{
    if (!out) return SCROLL_ERR_ARG;
    int rc = mask_frame_arg(b, s, f, "scroll_batch_dyn_mask_result");
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
    if (!dst) return SCROLL_ERR_ARG;
    int rc = mask_frame_arg(b, s, f, "scroll_batch_dyn_mask_map");
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

static float mask_span_ms(ScrollBatch *b, int from, int to)
{
    if (!b || !b->mk.res || !b->mk.timed) return -1.0f;
    if (hipSetDevice(b->device) != hipSuccess || hipEventSynchronize(b->mk.ev[3]) != hipSuccess) {
        (void)hipGetLastError();
        return -1.0f;
    }
    float ms = -1.0f;
    if (hipEventElapsedTime(&ms, b->mk.ev[from], b->mk.ev[to]) != hipSuccess) {
        (void)hipGetLastError();
        return -1.0f;
    }
    return ms;
}

float scroll_batch_dyn_mask_ms(ScrollBatch *b) { return mask_span_ms(b, 0, 3); }

float scroll_batch_dyn_mask_kernel_ms(ScrollBatch *b) { return mask_span_ms(b, 1, 2); }

}  // extern "C"
