/*
 * batch_surface.hip -- the batch engine's pixel entry (batch.h): windows of a
 * renderer's RGBA / BGRA surfaces become the dynamic rect's source or whole
 * I420 pictures on the device (k_csc, csc_kernels.hip; the rule:
 * csc_device.h), and the rect's references are set from device pictures.
 */
#include <hip/hip_runtime.h>

#include <stdint.h>

#include <vector>

#include "batch.h"
#include "csc_device.h"
#include "csc_engine.h"

using namespace scroll::batch;

namespace scroll {
namespace batch {

void surface_release(ScrollBatch *b, bool all)
{
    ScrollBatch::Surf &sf = b->sf;
    if (sf.fin) {
        (void)hipEventSynchronize(sf.fin);
        (void)hipEventDestroy(sf.fin);
        sf.fin = nullptr;
    }
    (void)hipFree(sf.pos);
    sf.pos = nullptr;
    sf.h_pos.clear();
    if (all) pass_release(&sf.run);
}

/* what every surface call asks of the surfaces: w pixels of every row lie inside the pitch */
int surf_args(const char *who, const ScrollSurfaces *surf, uint64_t w, bool streams)
{
    if (!surf || !surf->base) {
        set_err("%s: no surfaces", who);
        return SCROLL_ERR_ARG;
    }
    if ((surf->format != SCROLL_SURF_RGBA && surf->format != SCROLL_SURF_BGRA) ||
        (surf->matrix != SCROLL_SURF_BT601 && surf->matrix != SCROLL_SURF_BT709) || surf->full_range > 1u ||
        surf->cropped > 1u) {
        set_err("%s: format %u / matrix %u / full_range %u / cropped %u: not a SCROLL_SURF_* value or 0 / 1", who,
                surf->format, surf->matrix, surf->full_range, surf->cropped);
        return SCROLL_ERR_ARG;
    }
    if (((uintptr_t)surf->base | surf->pitch | surf->frame_stride | (streams ? surf->stream_stride : 0u)) & 15u) {
        set_err("%s: the surfaces' base, pitch and strides must be multiples of 16 bytes", who);
        return SCROLL_ERR_ARG;
    }
    if (surf->pitch < 4u * w) {
        set_err("%s: pitch %llu is smaller than a row of %llu pixels", who, (unsigned long long)surf->pitch,
                (unsigned long long)w);
        return SCROLL_ERR_ARG;
    }
    return SCROLL_OK;
}

}  // namespace batch
}  // namespace scroll

/* the launches of one conversion, between the timing events when timing is on */
static int surf_run(ScrollBatch *b, hipStream_t hs, const CscJob &job, const char *who)
{
    const int rc = pass_begin(b, &b->sf.run, 2, hs);
    if (rc) return rc;
    if (csc_launch(hs, &job)) {
        set_err("%s: k_csc launch: %s", who, hipGetErrorString(hipGetLastError()));
        return SCROLL_ERR_HIP;
    }
    /* (the timing only: sf.fin is not the end of a run) */
    return pass_stop(b, &b->sf.run, hs);
}

extern "C" {

int scroll_batch_dyn_source_from_surfaces(ScrollBatch *b, int nframes, const ScrollSurfaces *surf, void *hip_stream)
{
    const char *who = "scroll_batch_dyn_source_from_surfaces";
    if (!b) return SCROLL_ERR_ARG;
    if (!b->dyn_on) {
        set_err("%s: needs a dynamic rect (scroll_batch_set_dyn_rect)", who);
        return SCROLL_ERR_CONFIG;
    }
    if (nframes < 0 || nframes > b->max_frames) {
        set_err("%s: nframes %d out of range", who, nframes);
        return SCROLL_ERR_ARG;
    }
    const DynGeom &g = b->geo;
    const uint32_t w = 16u * (uint32_t)g.w, h = 16u * (uint32_t)g.h;
    const int rc = surf_args(who, surf, surf && surf->cropped ? w : (uint32_t)b->dyn_pw, true);
    if (rc) return rc;
    const int S = b->nstreams;
    if (nframes == 0 || S == 0) return SCROLL_OK;
    HIPCHK(hipSetDevice(b->device));
    hipStream_t hs = hip_stream ? (hipStream_t)hip_stream : b->own;
    ScrollBatch::Surf &sf = b->sf;

    CscJob job{};
    job.src = surf->base;
    job.pitch = surf->pitch;
    job.src_fr = surf->frame_stride;
    job.src_ld = surf->stream_stride;
    job.dst = b->d_src;
    job.dst_fr = g.src_fr;
    job.dst_ld = g.src_ld;
    job.x0 = g.x0;
    job.y0 = g.y0;
    job.w = w;
    job.h = h;
    job.S = (uint32_t)S;
    job.nframes = (uint32_t)nframes;
    job.cropped = surf->cropped;
    job.k = scroll::csc::coef(surf->format, surf->matrix, surf->full_range);
    if (csc_tasks(&job) > CSC_MAX_TASKS) {
        set_err("%s: more than 2^35 pixels in one call: convert fewer frames at a time", who);
        return SCROLL_ERR_ARG;
    }
    /* positions a locate placed on the device (scroll_batch_dyn_locate with
     * apply): the plain moving rect reads them in place, no host step; any
     * other configuration first brings the host's copy up to date */
    const bool located = b->dpos_dev && b->dyn_moving && !b->hint_on && !b->fallback;
    if (b->dpos_dev && !located) {
        const int pr = dyn_pos_refresh(b);
        if (pr) return pr;
    }
    job.pos_mask = g.pos_mask;
    if (located) {
        if (hs != b->dpos_hs) HIPCHK(hipStreamWaitEvent(hs, b->dpos_ev, 0));   /* located on another stream */
        job.dpos = b->d_dpos;
        job.dpos_ld = (uint32_t)b->max_frames;
    } else if (b->dsz_any && b->dyn_moving && !b->hint_on) {
        /* frames sized on their own: origins and sizes in the
         * packed table the coder's kernels read, uploaded here when stale */
        const uint32_t *dp = nullptr;
        const int pr = dyn_pos_table(b, hs, &dp);
        if (pr) return pr;
        job.dpos = dp;
        job.dpos_ld = (uint32_t)b->max_frames;
    } else if (b->dyn_pos_custom) {
        /* the origins of this call's frames, compact; the table is the
         * batch's, so the previous call's kernel must have read it.  With
         * the fallback on, a frame without the rect keeps a dormant
         * whole-picture region at (0, 0) (hd_upload) that is coded from its
         * source block if the frame falls back: it gets its pixels too */
        if (!sf.fin) {
            hipError_t e = hipMalloc(&sf.pos, (size_t)2 * b->max_streams * b->max_frames * sizeof(int32_t));
            if (e == hipSuccess) e = hipEventCreateWithFlags(&sf.fin, hipEventDisableTiming);
            if (e != hipSuccess) {
                surface_release(b, false);
                return hip_fail(who, e, true);
            }
        }
        HIPCHK(hipEventSynchronize(sf.fin));
        sf.h_pos.resize((size_t)2 * S * nframes);
        for (int s = 0; s < S; ++s)
            for (int f = 0; f < nframes; ++f) {
                const size_t i = (size_t)s * b->max_frames + f, o = (size_t)s * nframes + f;
                const bool dormant = b->h_dyn_pos[2 * i] < 0 && b->fallback;
                sf.h_pos[2 * o] = dormant ? 0 : b->h_dyn_pos[2 * i];
                sf.h_pos[2 * o + 1] = dormant ? 0 : b->h_dyn_pos[2 * i + 1];
            }
        HIPCHK(hipMemcpyAsync(sf.pos, sf.h_pos.data(), sf.h_pos.size() * sizeof(int32_t), hipMemcpyHostToDevice, hs));
        job.pos = sf.pos;
    }
    const int rr = surf_run(b, hs, job, who);
    if (job.pos) HIPCHK(hipEventRecord(sf.fin, hs));
    return rr;
}

int scroll_batch_surfaces_to_i420(ScrollBatch *b, int n, int w, int h, const ScrollSurfaces *surf, uint8_t *d_pics,
                                  size_t pic_stride, void *hip_stream)
{
    const char *who = "scroll_batch_surfaces_to_i420";
    if (!b) return SCROLL_ERR_ARG;
    if (n < 0 || w <= 0 || h <= 0 || (w & 15) || (h & 15) || w > 65536 || h > 65536) {
        set_err("%s: n >= 0 pictures of w x h pixels, both multiples of 16", who);
        return SCROLL_ERR_ARG;
    }
    const int rc = surf_args(who, surf, (uint64_t)w, false);
    if (rc) return rc;
    const size_t pic = (size_t)w * h * 3 / 2;
    if (!d_pics || (((uintptr_t)d_pics | pic_stride) & 15u) || (n > 1 && pic_stride < pic)) {
        set_err("%s: d_pics and pic_stride multiples of 16, pic_stride at least a picture's %zu bytes", who, pic);
        return SCROLL_ERR_ARG;
    }
    if (n == 0) return SCROLL_OK;
    HIPCHK(hipSetDevice(b->device));
    hipStream_t hs = hip_stream ? (hipStream_t)hip_stream : b->own;
    CscJob job{};
    job.src = surf->base;
    job.pitch = surf->pitch;
    job.src_fr = surf->frame_stride;
    job.dst = d_pics;
    job.dst_fr = pic_stride;
    job.w = (uint32_t)w;
    job.h = (uint32_t)h;
    job.S = 1u;
    job.nframes = (uint32_t)n;
    job.k = scroll::csc::coef(surf->format, surf->matrix, surf->full_range);
    if (csc_tasks(&job) > CSC_MAX_TASKS) {
        set_err("%s: more than 2^35 pixels in one call: convert fewer pictures at a time", who);
        return SCROLL_ERR_ARG;
    }
    return surf_run(b, hs, job, who);
}

int scroll_batch_set_dyn_refs_device(ScrollBatch *b, int s, const uint8_t *d_ref_a, const uint8_t *d_ref_b)
{
    return dyn_set_refs(b, s, d_ref_a, d_ref_b, hipMemcpyDeviceToDevice);
}

float scroll_batch_surface_ms(ScrollBatch *b) { return b ? pass_span_ms(b, &b->sf.run, 0, 1) : -1.0f; }

}  // extern "C"
