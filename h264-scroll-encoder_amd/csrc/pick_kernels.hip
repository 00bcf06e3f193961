/*
 * pick_kernels.hip -- MI355X (gfx950) kernel of the rect's per-frame QP pick
 * (scroll_batch_dyn_pick): from the QP probe's device results
 * straight into the per-frame QP table k_dyn_rows reads, without the host.
 *
 * The work is one comparison chain over at most 8 candidates of 32 bytes per
 * frame, so the kernel is as plain as its rule (pick_device.h): one thread
 * per (stream, frame) in SCROLL_DYN_RATE_FRAME; one thread per stream in
 * SCROLL_DYN_RATE_BUCKET, whose level makes a stream's frames sequential.
 */
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "pick_device.h"
#include "pick_engine.h"

using namespace scroll::pick;

namespace {

constexpr int PICK_T = 256;

struct PickQps {
    uint8_t qp[SCROLL_DYN_PROBE_MAX_QPS];
};

__device__ inline void pick_one(const DevStream *__restrict__ st, const DynFrame *__restrict__ dfr, int ld_fr,
                                const ScrollDynProbe *__restrict__ res, const uint32_t *__restrict__ done, int h,
                                const PickQps &Q, int nq, uint32_t mode, uint32_t frame_bits, uint32_t bucket_bits,
                                int s, int f, int64_t *level, uint8_t *__restrict__ qpf, PickOut *__restrict__ out)
{
    const size_t nb = (size_t)s * ld_fr + f;
    uint32_t status = PICK_NONE;
    /* no dynamic NAL in the frame, or a stream whose deblocking filter is on
     * (it keeps QP 26): nothing to choose; a frame whose rows the probe did
     * not all count: no choice over partial sums */
    if (dfr[nb].nal >= 0 && st[s].deblock) status = done[nb] == (uint32_t)h ? PICK_OK : PICK_SHORT;
    const Choice c = pick_frame(mode, res + nb * SCROLL_DYN_PROBE_MAX_QPS, Q.qp, nq, status == PICK_OK, frame_bits,
                                bucket_bits, level);
    PickOut o{0, 0, (uint8_t)status, 0};
    uint8_t q = 0xFFu;
    if (c.k >= 0) {
        q = Q.qp[c.k];
        o.k = (uint8_t)c.k;
        o.qp = q;
        o.status = (uint8_t)(c.over ? PICK_OVER : PICK_OK);
    }
    qpf[nb] = q;
    out[nb] = o;
}

__global__ __launch_bounds__(PICK_T) void k_dyn_pick(const DevStream *__restrict__ st,
                                                     const DynFrame *__restrict__ dfr, int ld_fr, int nframes,
                                                     int S, const ScrollDynProbe *__restrict__ res,
                                                     const uint32_t *__restrict__ done, int h, PickQps Q, int nq,
                                                     ScrollDynRate rate, const uint32_t *__restrict__ fb,
                                                     long long *__restrict__ level, uint8_t *__restrict__ qpf,
                                                     PickOut *__restrict__ out)
{
    const int i = (int)(blockIdx.x * (uint32_t)PICK_T + threadIdx.x);
    if (rate.mode == SCROLL_DYN_RATE_BUCKET) {
        if (i >= S) return;
        const uint32_t fbits = fb ? fb[i] : rate.frame_bits;
        int64_t lv = level[i];
        for (int f = 0; f < nframes; ++f)
            pick_one(st, dfr, ld_fr, res, done, h, Q, nq, rate.mode, fbits, rate.bucket_bits, i, f, &lv, qpf, out);
        level[i] = lv;
    } else {
        if (i >= S * nframes) return;
        const int s = i / nframes, f = i - s * nframes;
        int64_t lv = 0;
        pick_one(st, dfr, ld_fr, res, done, h, Q, nq, rate.mode, fb ? fb[s] : rate.frame_bits, rate.bucket_bits, s, f,
                 &lv, qpf, out);
    }
}

}  // namespace

int pick_launch(hipStream_t hs, int nframes, int S, const DevStream *st, const DynFrame *dfr, int ld_fr,
                const ScrollDynProbe *res, const uint32_t *done, int h, const uint8_t *qps, int nq,
                const ScrollDynRate *rate, const uint32_t *fb, long long *level, uint8_t *qpf, PickOut *out)
{
    if (nframes <= 0 || S <= 0) return 0;
    PickQps Q{};
    for (int k = 0; k < nq; ++k) Q.qp[k] = qps[k];
    const int n = rate->mode == SCROLL_DYN_RATE_BUCKET ? S : S * nframes;
    hipLaunchKernelGGL(k_dyn_pick, dim3((n + PICK_T - 1) / PICK_T), dim3(PICK_T), 0, hs, st, dfr, ld_fr, nframes, S,
                       res, done, h, Q, nq, *rate, fb, level, qpf, out);
    return hipGetLastError() != hipSuccess ? -1 : 0;
}
