/*
 * batch_detect.hip -- the batch engine's offset detector (batch.h): each
 * frame's scroll offset found on the device from the renderer's surfaces and
 * the stacked reference pictures (scroll_batch_detect_offsets; k_det_refs,
 * k_det_surf, k_det_score, k_det_pick, detect_kernels.hip; the rule:
 * detect_device.h) and its results.
 */
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "batch.h"
#include "csc_device.h"
#include "detect_device.h"
#include "detect_engine.h"

using namespace scroll::batch;

namespace scroll {
namespace batch {

void detect_release(ScrollBatch *b)
{
    ScrollBatch::Detect &d = b->dt;
    pass_release(&d.run);
    (void)hipFree(d.sig_s);
    (void)hipFree(d.sig_r);
    (void)hipFree(d.scores);
    (void)hipFree(d.res);
    d = ScrollBatch::Detect{};
}

}  // namespace batch
}  // namespace scroll

static int detect_alloc(ScrollBatch *b, const char *who)
{
    ScrollBatch::Detect &d = b->dt;
    if (d.res) return SCROLL_OK;
    /* for every seg_step: the signatures of all nseg segments */
    const size_t S = (size_t)b->max_streams, NF = S * (size_t)b->max_frames, ph = (size_t)b->dyn_ph;
    const size_t ns = scroll::detect::nseg((uint32_t)b->dyn_pw);
    hipError_t e = hipMalloc(&d.sig_s, NF * ph * ns * sizeof(uint16_t));
    if (e == hipSuccess) e = hipMalloc(&d.sig_r, S * 2u * ph * ns * sizeof(uint16_t));
    if (e == hipSuccess) e = hipMalloc(&d.scores, NF * (ph + 1u) * sizeof(uint32_t));
    if (e == hipSuccess) e = hipMalloc(&d.res, NF * sizeof(ScrollOffsetFound));
    if (e == hipSuccess) e = hipMemset(d.scores, 0xFF, NF * (ph + 1u) * sizeof(uint32_t));
    if (e == hipSuccess) e = hipMemset(d.res, 0, NF * sizeof(ScrollOffsetFound));
    if (e == hipSuccess) e = hipEventCreateWithFlags(&d.run.fin, hipEventDisableTiming);
    if (e != hipSuccess) {
        detect_release(b);
        return hip_fail(who, e, true);
    }
    return SCROLL_OK;
}

extern "C" {

int scroll_batch_detect_offsets(ScrollBatch *b, int nframes, const ScrollSurfaces *surf, const ScrollDetect *rule,
                                void *hip_stream)
{
    const char *who = "scroll_batch_detect_offsets";
    if (!b || !rule) {
        set_err("%s: no batch or no rule", who);
        return SCROLL_ERR_ARG;
    }
    if (!b->dyn_on || !b->dyn_refs) {
        set_err("%s: needs a dynamic rect with reference pictures "
                "(scroll_batch_set_dyn_rect, scroll_batch_set_dyn_refs)", who);
        return SCROLL_ERR_CONFIG;
    }
    if (nframes < 0 || nframes > b->max_frames) {
        set_err("%s: nframes %d out of range", who, nframes);
        return SCROLL_ERR_ARG;
    }
    const uint32_t pw = (uint32_t)b->dyn_pw, ph = (uint32_t)b->dyn_ph;
    if (rule->seg_step == 0u || rule->seg_step > scroll::detect::nseg(pw) || rule->apply > 1u) {
        set_err("%s: seg_step %u outside 1..%u (the picture's segments of 64 columns) or apply %u not 0 / 1", who,
                rule->seg_step, scroll::detect::nseg(pw), rule->apply);
        return SCROLL_ERR_ARG;
    }
    const int rc = surf_args(who, surf, (uint64_t)pw, true);
    if (rc) return rc;
    if (surf->cropped) {
        set_err("%s: the surfaces are whole pictures (cropped = 1: a rect's rows say nothing of the scroll)", who);
        return SCROLL_ERR_ARG;
    }
    if (ph >= 0xFFFFu) {
        set_err("%s: a picture of %u rows: the window's ends are 16-bit", who, ph);
        return SCROLL_ERR_CONFIG;
    }
    const int S = b->nstreams;
    if ((uint64_t)S * (uint64_t)nframes * pw * ph > DET_MAX_PIXELS) {
        set_err("%s: more than 2^35 pixels in one call: detect fewer frames at a time", who);
        return SCROLL_ERR_ARG;
    }
    if (nframes == 0 || S == 0) return SCROLL_OK;
    HIPCHK(hipSetDevice(b->device));
    const int ar = detect_alloc(b, who);
    if (ar) return ar;
    ScrollBatch::Detect &d = b->dt;
    DetJob job{};
    job.src = surf->base;
    job.pitch = surf->pitch;
    job.src_fr = surf->frame_stride;
    job.src_ld = surf->stream_stride;
    job.refs = b->d_refs;
    job.ref_ld = b->geo.ref_ld;
    job.pic = (uint64_t)pw * ph * 3u / 2u;
    job.sig_s = d.sig_s;
    job.sig_r = d.sig_r;
    job.scores = d.scores;
    job.res = d.res;
    job.off = b->d_off;
    job.ld_fr = (uint32_t)b->max_frames;
    job.pw = pw;
    job.ph = ph;
    job.S = (uint32_t)S;
    job.nframes = (uint32_t)nframes;
    job.nuse = scroll::detect::nuse(pw, rule->seg_step);
    job.rule = *rule;
    job.k = scroll::csc::coef(surf->format, surf->matrix, surf->full_range);

    hipStream_t hs = hip_stream ? (hipStream_t)hip_stream : b->own;
    int tr = pass_begin(b, &d.run, 5, hs);
    if (tr) return tr;
    /* the references' signatures every call: a cache would have to be
     * invalidated by every call that writes a reference picture */
    if (det_launch_refs(hs, &job)) {
        set_err("k_det_refs launch: %s", hipGetErrorString(hipGetLastError()));
        return SCROLL_ERR_HIP;
    }
    if ((tr = pass_mark(b, &d.run, 1, hs))) return tr;
    if (det_launch_surf(hs, &job)) {
        set_err("k_det_surf launch: %s", hipGetErrorString(hipGetLastError()));
        return SCROLL_ERR_HIP;
    }
    if ((tr = pass_mark(b, &d.run, 2, hs))) return tr;
    if (det_launch_score(hs, &job)) {
        set_err("k_det_score launch: %s", hipGetErrorString(hipGetLastError()));
        return SCROLL_ERR_HIP;
    }
    if ((tr = pass_mark(b, &d.run, 3, hs))) return tr;
    if (det_launch_pick(hs, &job)) {
        set_err("k_det_pick launch: %s", hipGetErrorString(hipGetLastError()));
        return SCROLL_ERR_HIP;
    }
    return pass_end(b, &d.run, hs, nframes, S);
}

int scroll_batch_detect_result(ScrollBatch *b, int s, int f, ScrollOffsetFound *out)
{
    if (!b || !out) return SCROLL_ERR_ARG;
    int rc = pass_frame_arg(b, &b->dt.run, s, f, "scroll_batch_detect_result", "detect", "scroll_batch_detect_offsets");
    if (rc) return rc;
    HIPCHK(hipMemcpy(out, b->dt.res + (size_t)s * b->max_frames + f, sizeof(*out), hipMemcpyDeviceToHost));
    return SCROLL_OK;
}

const ScrollOffsetFound *scroll_batch_detect_device(ScrollBatch *b, size_t *stream_stride)
{
    if (!b || !b->dt.res) return nullptr;
    if (stream_stride) *stream_stride = (size_t)b->max_frames * sizeof(ScrollOffsetFound);
    return b->dt.res;
}

int scroll_batch_detect_scores(ScrollBatch *b, int s, int f, uint32_t *dst)
{
    if (!b || !dst) return SCROLL_ERR_ARG;
    int rc = pass_frame_arg(b, &b->dt.run, s, f, "scroll_batch_detect_scores", "detect", "scroll_batch_detect_offsets");
    if (rc) return rc;
    const size_t n = (size_t)b->dyn_ph + 1u;
    HIPCHK(hipMemcpy(dst, b->dt.scores + ((size_t)s * b->max_frames + f) * n, n * sizeof(uint32_t),
                     hipMemcpyDeviceToHost));
    return SCROLL_OK;
}

const uint32_t *scroll_batch_detect_scores_device(ScrollBatch *b, size_t *stream_stride, size_t *frame_stride)
{
    if (!b || !b->dt.scores) return nullptr;
    const size_t fr = ((size_t)b->dyn_ph + 1u) * sizeof(uint32_t);
    if (frame_stride) *frame_stride = fr;
    if (stream_stride) *stream_stride = (size_t)b->max_frames * fr;
    return b->dt.scores;
}

float scroll_batch_detect_ms(ScrollBatch *b) { return b ? pass_span_ms(b, &b->dt.run, 0, 4) : -1.0f; }

float scroll_batch_detect_kernel_ms(ScrollBatch *b) { return b ? pass_span_ms(b, &b->dt.run, 1, 2) : -1.0f; }

/* the score stage alone (k_det_score and k_det_pick): what tools/detect_bench.py reports beside the kernel */
float scroll_batch_detect_score_ms(ScrollBatch *b) { return b ? pass_span_ms(b, &b->dt.run, 2, 4) : -1.0f; }

}  // extern "C"
