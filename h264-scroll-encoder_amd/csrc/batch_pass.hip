/*
 * batch_pass.hip -- what the batch engine's side passes share (batch.h): the
 * record of a pass's last run with its timing events, the checks and the wait
 * of the calls that read a run's results, and the compose's state pass run
 * dry into a pass's own buffers, with k_dyn_rows after it.
 */
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "batch.h"
#include "scroll_engine.h"
#include "dyn_engine.h"

namespace scroll {
namespace batch {

void pass_release(PassRun *r)
{
    if (r->fin) {
        (void)hipEventSynchronize(r->fin);
        (void)hipEventDestroy(r->fin);
    }
    for (hipEvent_t e : r->ev)
        if (e) (void)hipEventDestroy(e);
    *r = PassRun{};
}

int pass_begin(ScrollBatch *b, PassRun *r, int n, hipStream_t hs)
{
    r->timed = 0;
    if (!b->timing) return SCROLL_OK;
    /* (every missing one: a creation that failed part-way is made up for here) */
    for (int i = 0; i < n; ++i)
        if (!r->ev[i]) HIPCHK(hipEventCreate(&r->ev[i]));
    r->nev = n;
    HIPCHK(hipEventRecord(r->ev[0], hs));
    return SCROLL_OK;
}

int pass_mark(ScrollBatch *b, PassRun *r, int i, hipStream_t hs)
{
    if (b->timing) HIPCHK(hipEventRecord(r->ev[i], hs));
    return SCROLL_OK;
}

int pass_stop(ScrollBatch *b, PassRun *r, hipStream_t hs)
{
    if (!b->timing || !r->nev) return SCROLL_OK;
    HIPCHK(hipEventRecord(r->ev[r->nev - 1], hs));
    r->timed = 1;
    return SCROLL_OK;
}

int pass_end(ScrollBatch *b, PassRun *r, hipStream_t hs, int nframes, int nstreams)
{
    const int rc = pass_stop(b, r, hs);
    if (rc) return rc;
    HIPCHK(hipEventRecord(r->fin, hs));
    r->nframes = nframes;
    r->nstreams = nstreams;
    return SCROLL_OK;
}

int pass_have(const PassRun *r, const char *who, const char *noun, const char *entry)
{
    if (r->nframes >= 0) return SCROLL_OK;
    set_err("%s: no %s to read (%s; scroll_batch_set_dyn_rect drops it)", who, noun, entry);
    return SCROLL_ERR_CONFIG;
}

int pass_frame_arg(ScrollBatch *b, PassRun *r, int s, int f, const char *who, const char *noun, const char *entry)
{
    const int rc = pass_have(r, who, noun, entry);
    if (rc) return rc;
    if (s < 0 || s >= r->nstreams || f < 0 || f >= r->nframes) {
        set_err("%s: stream %d / frame %d outside the last %s", who, s, f, noun);
        return SCROLL_ERR_ARG;
    }
    HIPCHK(hipSetDevice(b->device));
    HIPCHK(hipEventSynchronize(r->fin));
    return SCROLL_OK;
}

float pass_span_ms(ScrollBatch *b, const PassRun *r, int from, int to)
{
    float ms = -1.0f;
    if (!r->timed) return ms;
    if (hipSetDevice(b->device) != hipSuccess || hipEventSynchronize(r->ev[r->nev - 1]) != hipSuccess ||
        hipEventElapsedTime(&ms, r->ev[from], r->ev[to]) != hipSuccess) {
        (void)hipGetLastError();
        return -1.0f;
    }
    return ms;
}

hipError_t dry_plan_alloc(const ScrollBatch *b, DryPlan *d)
{
    const size_t S = (size_t)b->max_streams, NF = S * (size_t)b->max_frames;
    hipError_t e = hipMalloc(&d->nal, S * (size_t)b->ld_nal * sizeof(NalDesc));
    if (e == hipSuccess) e = hipMalloc(&d->dfr, NF * sizeof(DynFrame));
    if (e == hipSuccess) e = hipMalloc(&d->pend, S * sizeof(PlanPending));
    return e;
}

void dry_plan_free(DryPlan *d)
{
    (void)hipFree(d->nal);
    (void)hipFree(d->dfr);
    (void)hipFree(d->pend);
    *d = DryPlan{};
}

int dry_plan_launch(ScrollBatch *b, hipStream_t hs, int nframes, const DryPlan &d, int flags_extra, uint32_t *ctr,
                    const uint32_t *dpos)
{
    const int plan = b->mode == SCROLL_MODE_EXPERIMENT ? SCROLL_PLAN_EXPERIMENT : SCROLL_PLAN_COMPOSER;
    /* the debug bits below k_plan's own flags only, as the compose passes them (launch, batch_core.hip) */
    scroll_launch_plan(hs, b->nstreams, b->d_st, b->d_off, b->max_frames, d.nal, b->ld_nal, nframes, plan,
                       (b->debug & (PLAN_REWIND - 1)) | PLAN_STATE | PLAN_DYN | flags_extra, d.pend, d.dfr,
                       b->max_frames, nullptr, 0u, 0u, ctr, dpos);
    HIPCHK(hipGetLastError());
    return SCROLL_OK;
}

hipError_t pred_rows_alloc(const ScrollBatch *b, PredRows *p)
{
    const size_t NF = (size_t)b->max_streams * (size_t)b->max_frames;
    hipError_t e = hipMalloc(&p->rows, NF * 32 * (size_t)b->geo.h * sizeof(uint32_t));
    /* the general-frame list holds every frame: it can never run out */
    if (e == hipSuccess) e = hipMalloc(&p->ctr, (DYN_CTR_LIST + NF) * sizeof(uint32_t));
    if (e == hipSuccess) e = hipMalloc(&p->heads, NF * DYN_HEAD_VECS * sizeof(uint4));
    return e;
}

void pred_rows_free(PredRows *p)
{
    (void)hipFree(p->rows);
    (void)hipFree(p->ctr);
    (void)hipFree(p->heads);
    *p = PredRows{};
}

int pred_rows_launch(ScrollBatch *b, hipStream_t hs, int nframes, const DryPlan &d, const PredRows &p, DynGeom *G)
{
    G->gen_cap = (uint32_t)((size_t)b->max_streams * b->max_frames);
    if (dyn_launch_rows(hs, nframes, b->nstreams, b->d_st, d.nal, b->ld_nal, d.pend, d.dfr, b->max_frames, G, p.rows,
                        p.ctr, p.heads, nullptr)) {
        set_err("k_dyn_rows launch: %s", hipGetErrorString(hipGetLastError()));
        return SCROLL_ERR_HIP;
    }
    return SCROLL_OK;
}

}  // namespace batch
}  // namespace scroll
