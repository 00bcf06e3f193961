/*
 * batch_rate.hip -- the batch engine's per-frame QP of the plain dynamic rect
 * (batch.h): the device table k_dyn_rows resolves every frame's QP from, its
 * host setters and read-back, and the pick that fills it from the QP probe's
 * device results (k_dyn_pick, pick_kernels.hip) with its per-stream buckets.
 */
#include <hip/hip_runtime.h>

#include <stdint.h>

#include <algorithm>
#include <vector>

#include "batch.h"
#include "pick_device.h"
#include "pick_engine.h"
#include "dyn_device.h"         /* scroll::dyn::QP_MIN: below it a NAL takes a general-path record slot */

using namespace scroll::batch;
using namespace scroll::pick;

namespace scroll {
namespace batch {

void rate_release(ScrollBatch *b)
{
    ScrollBatch::Rate &r = b->rt;
    pass_release(&r.run);
    (void)hipFree(r.level);
    (void)hipFree(r.fb);
    (void)hipFree(r.out);
    r = ScrollBatch::Rate{};
    b->h_qpf.clear();
    b->qpf_dev = 0;
}

}  // namespace batch
}  // namespace scroll

static size_t table_bytes(const ScrollBatch *b) { return (size_t)b->max_streams * (size_t)b->max_frames; }

/* the table on the device and its host copy, every entry 0xFF */
static int table_alloc(ScrollBatch *b, const char *who)
{
    if (b->dx.qpf) return SCROLL_OK;
    HIPCHK(hipSetDevice(b->device));
    uint8_t *t = nullptr;
    hipError_t e = hipMalloc(&t, table_bytes(b));
    if (e == hipSuccess) e = hipMemset(t, 0xFF, table_bytes(b));
    if (e != hipSuccess) {
        (void)hipFree(t);
        return hip_fail(who, e, true);
    }
    b->dx.qpf = t;
    b->h_qpf.assign(table_bytes(b), 0xFFu);
    b->qpf_dev = 0;
    return SCROLL_OK;
}

/* everything that may write the table has finished; the host copy is current */
static int table_refresh(ScrollBatch *b)
{
    int rc = batch_host_sync(b);
    if (rc) return rc;
    if (!b->dx.qpf || !b->qpf_dev) return SCROLL_OK;
    HIPCHK(hipSetDevice(b->device));
    if (b->rt.run.fin) HIPCHK(hipEventSynchronize(b->rt.run.fin));
    HIPCHK(hipMemcpy(b->h_qpf.data(), b->dx.qpf, table_bytes(b), hipMemcpyDeviceToHost));
    /* (a pointer handed out stays with the caller: its kernels may write again) */
    return SCROLL_OK;
}

/* the pick's buffers: the levels (zero), frame_bits per stream, the choices */
static int rate_alloc(ScrollBatch *b, const char *who)
{
    ScrollBatch::Rate &r = b->rt;
    if (r.level) return SCROLL_OK;
    HIPCHK(hipSetDevice(b->device));
    const size_t S = (size_t)b->max_streams;
    hipError_t e = hipMalloc(&r.level, S * sizeof(long long));
    if (e == hipSuccess) e = hipMemset(r.level, 0, S * sizeof(long long));
    if (e == hipSuccess) e = hipMalloc(&r.fb, S * sizeof(uint32_t));
    if (e == hipSuccess) e = hipMalloc(&r.out, table_bytes(b) * sizeof(PickOut));
    if (e == hipSuccess) e = hipEventCreateWithFlags(&r.run.fin, hipEventDisableTiming);
    if (e != hipSuccess) {
        rate_release(b);
        return hip_fail(who, e, true);
    }
    return SCROLL_OK;
}

namespace scroll {
namespace batch {

int qp_frames_any(ScrollBatch *b, bool *any)
{
    *any = false;
    if (!b->dx.qpf) return SCROLL_OK;
    int rc = table_refresh(b);
    if (rc) return rc;
    for (uint8_t q : b->h_qpf) *any |= q != 0xFFu;
    return SCROLL_OK;
}

}  // namespace batch
}  // namespace scroll

extern "C" {

int scroll_batch_set_dyn_qp_frames(ScrollBatch *b, int s, int f0, int n, const int8_t *qps)
{
    const char *who = "scroll_batch_set_dyn_qp_frames";
    if (!b || (!qps && n > 0) || s < -1 || s >= b->nstreams || f0 < 0 || n < 0 || f0 > b->max_frames ||
        n > b->max_frames - f0) {
        set_err("%s: stream or frame range out of bounds", who);
        return SCROLL_ERR_ARG;
    }
    for (int i = 0; i < n; ++i)
        if (qps[i] < -1 || qps[i] > SCROLL_DYN_QP_MAX) {
            set_err("%s: entry %d: QP %d outside -1, 0..%d", who, i, qps[i], SCROLL_DYN_QP_MAX);
            return SCROLL_ERR_ARG;
        }
    if (!b->dyn_on || b->hint_on) {
        set_err("%s: needs the dynamic rect without UI hints (under hints: scroll_batch_set_dyn_qp_at)", who);
        return SCROLL_ERR_CONFIG;
    }
    const int s0 = s < 0 ? 0 : s, s1 = s < 0 ? b->nstreams : s + 1;
    for (int k = s0; k < s1; ++k)
        for (int i = 0; i < n; ++i)
            if (qps[i] >= 0 && qps[i] != 26 && !b->h_st[k].deblock) {
                set_err("%s: stream %d has the deblocking filter on: its rect codes at QP 26", who, k);
                return SCROLL_ERR_CONFIG;
            }
    int rc = table_alloc(b, who);
    if (rc || (rc = table_refresh(b))) return rc;
    if (n == 0 || s0 == s1) return SCROLL_OK;
    const size_t F = (size_t)b->max_frames;
    for (int k = s0; k < s1; ++k)
        for (int i = 0; i < n; ++i) b->h_qpf[(size_t)k * F + f0 + i] = qps[i] < 0 ? 0xFFu : (uint8_t)qps[i];
    HIPCHK(hipMemcpy2D(b->dx.qpf + (size_t)s0 * F + f0, F, b->h_qpf.data() + (size_t)s0 * F + f0, F, (size_t)n,
                       (size_t)(s1 - s0), hipMemcpyHostToDevice));
    /* frames below QP_MIN take a general-path record slot each, on top of
     * what typical content takes (set_dyn_rect's allowance) */
    size_t low = 0;
    for (uint8_t q : b->h_qpf) low += q < (uint8_t)scroll::dyn::QP_MIN;
    if (low) rc = dyn_reserve_gen(b, low + std::max<size_t>(32, table_bytes(b) / 64));
    return rc;
}

int scroll_batch_clear_dyn_qp_frames(ScrollBatch *b)
{
    if (!b) return SCROLL_ERR_ARG;
    if (!b->dx.qpf) return SCROLL_OK;
    int rc = batch_host_sync(b);
    if (rc) return rc;
    HIPCHK(hipSetDevice(b->device));
    if (b->rt.run.fin) HIPCHK(hipEventSynchronize(b->rt.run.fin));
    HIPCHK(hipMemset(b->dx.qpf, 0xFF, table_bytes(b)));
    HIPCHK(hipDeviceSynchronize());
    std::fill(b->h_qpf.begin(), b->h_qpf.end(), (uint8_t)0xFFu);
    return SCROLL_OK;
}

int scroll_batch_dyn_qp_frames(ScrollBatch *b, int s, int f0, int n, int8_t *out)
{
    if (!b || (!out && n > 0) || s < 0 || s >= b->nstreams || f0 < 0 || n < 0 || f0 > b->max_frames ||
        n > b->max_frames - f0) {
        set_err("scroll_batch_dyn_qp_frames: stream or frame range out of bounds");
        return SCROLL_ERR_ARG;
    }
    for (int i = 0; i < n; ++i) out[i] = -1;
    if (!b->dx.qpf || n == 0) return SCROLL_OK;
    int rc = table_refresh(b);
    if (rc) return rc;
    for (int i = 0; i < n; ++i) {
        const uint8_t q = b->h_qpf[(size_t)s * b->max_frames + f0 + i];
        out[i] = q > SCROLL_DYN_QP_MAX ? -1 : (int8_t)q;
    }
    return SCROLL_OK;
}

uint8_t *scroll_batch_dyn_qp_frames_device(ScrollBatch *b, size_t *stream_stride)
{
    if (!b || !b->dyn_on || table_alloc(b, "scroll_batch_dyn_qp_frames_device")) return nullptr;
    if (stream_stride) *stream_stride = (size_t)b->max_frames;
    b->qpf_dev = 1;                    /* from here on the caller's kernels may write it */
    return b->dx.qpf;
}

int scroll_batch_dyn_pick(ScrollBatch *b, int nframes, const ScrollDynRate *rate,
                          const uint32_t *frame_bits_per_stream, void *hip_stream)
{
    const char *who = "scroll_batch_dyn_pick";
    if (!b || !rate || (rate->mode != SCROLL_DYN_RATE_FRAME && rate->mode != SCROLL_DYN_RATE_BUCKET) ||
        nframes < 0) {
        set_err("%s: a rate with mode SCROLL_DYN_RATE_FRAME or _BUCKET, nframes >= 0", who);
        return SCROLL_ERR_ARG;
    }
    ScrollBatch::Probe &p = b->pb;
    if (p.run.nframes < 0 || p.hinted || nframes > p.run.nframes || p.run.nstreams != b->nstreams) {
        set_err("%s: needs a scroll_batch_dyn_probe (the plain one) of at least %d frames of the batch's streams "
                "before it", who, nframes);
        return SCROLL_ERR_CONFIG;
    }
    if (b->hint_on || !b->dyn_on) {
        set_err("%s: picks for the plain dynamic rect: clear the UI hints (under hints: "
                "scroll_batch_set_dyn_qp_at)", who);
        return SCROLL_ERR_CONFIG;
    }
    HIPCHK(hipSetDevice(b->device));
    int rc = table_alloc(b, who);
    if (rc || (rc = rate_alloc(b, who))) return rc;
    /* a candidate below QP_MIN: any frame may take a general-path record
     * slot, and only the device will know which -- slots for all, now */
    bool low = false;
    for (int k = 0; k < p.nq; ++k) low |= p.qps[k] < scroll::dyn::QP_MIN;
    if (low && b->geo.gen_cap < table_bytes(b)) {
        if ((rc = batch_host_sync(b)) || (rc = dyn_reserve_gen(b, table_bytes(b)))) return rc;
    }
    hipStream_t hs = hip_stream ? (hipStream_t)hip_stream : b->own;
    ScrollBatch::Rate &r = b->rt;
    const int S = b->nstreams;
    if (frame_bits_per_stream && S > 0)
        HIPCHK(hipMemcpyAsync(r.fb, frame_bits_per_stream, (size_t)S * sizeof(uint32_t), hipMemcpyHostToDevice, hs));
    if (pick_launch(hs, nframes, S, b->d_st, p.plan.dfr, b->max_frames, p.res, p.done, b->geo.h, p.qps, p.nq, rate,
                    frame_bits_per_stream ? r.fb : nullptr, r.level, b->dx.qpf, r.out)) {
        set_err("k_dyn_pick launch: %s", hipGetErrorString(hipGetLastError()));
        return SCROLL_ERR_HIP;
    }
    if ((rc = pass_end(b, &r.run, hs, nframes, S))) return rc;
    b->qpf_dev = 1;
    return SCROLL_OK;
}

int scroll_batch_dyn_pick_result(ScrollBatch *b, int s, int f, int *k, int *qp)
{
    if (!b) return SCROLL_ERR_ARG;
    const int rc = pass_frame_arg(b, &b->rt.run, s, f, "scroll_batch_dyn_pick_result", "pick", "scroll_batch_dyn_pick");
    if (rc) return rc;
    PickOut o;
    HIPCHK(hipMemcpy(&o, b->rt.out + (size_t)s * b->max_frames + f, sizeof(o), hipMemcpyDeviceToHost));
    if (k) *k = -1;
    if (qp) *qp = -1;
    if (o.status == PICK_SHORT) {
        set_err("scroll_batch_dyn_pick_result: stream %d frame %d: the probe did not count every rect row", s, f);
        return SCROLL_ERR_DEVICE;
    }
    if (o.status == PICK_NONE) return 2;
    if (k) *k = o.k;
    if (qp) *qp = o.qp;
    return o.status == PICK_OVER ? 1 : 0;
}

int scroll_batch_dyn_rate_level(ScrollBatch *b, int s, int64_t *level, int set)
{
    const char *who = "scroll_batch_dyn_rate_level";
    if (!b || !level || s < 0 || s >= b->nstreams) {
        set_err("%s: stream out of range", who);
        return SCROLL_ERR_ARG;
    }
    if (!b->dyn_on) {
        set_err("%s: needs the dynamic rect", who);
        return SCROLL_ERR_CONFIG;
    }
    int rc = rate_alloc(b, who);
    if (rc) return rc;
    HIPCHK(hipEventSynchronize(b->rt.run.fin)); /* (never recorded: complete) */
    long long v = (long long)*level;
    if (set) {
        HIPCHK(hipMemcpy(b->rt.level + s, &v, sizeof(v), hipMemcpyHostToDevice));
    } else {
        HIPCHK(hipMemcpy(&v, b->rt.level + s, sizeof(v), hipMemcpyDeviceToHost));
        *level = (int64_t)v;
    }
    return SCROLL_OK;
}

}  // extern "C"
