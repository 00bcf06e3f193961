/*
 * pick_device.h -- the rule by which the rect's per-frame QP is picked from
 * the QP probe's results (scroll_batch_dyn_pick).
 *
 * Pure integer functions: k_dyn_pick (pick_kernels.hip) runs them per
 * (stream, frame) or per stream, tests/hostsim/pick_sim.cpp compiles them
 * for the CPU and tests/test_pick_hostsim.py checks them against a numpy
 * restatement and against h264scroll.pick_qp.
 *
 * The cost of candidate k of a frame is the QP-dependent part of its dynamic
 * NAL's RBSP bits (composer_batch.h, "From bits to a size"):
 *     cost(k) = bits[k] + len(se(qp[k] - 26)),
 * the frame's constant C(frame) left out: it is the same for every
 * candidate.
 */
#ifndef SCROLL_PICK_DEVICE_H
#define SCROLL_PICK_DEVICE_H

#include <stdint.h>

#include "composer_batch.h"     /* ScrollDynProbe, ScrollDynRate */

#if !defined(__HIPCC__) && !defined(__device__)
#define __device__
#define __host__
#endif

namespace scroll {
namespace pick {

/* what a frame of the pick got (PickOut.status; scroll_batch_dyn_pick_result) */
constexpr uint32_t PICK_OK = 0u;        /* the best candidate within the allowance */
constexpr uint32_t PICK_OVER = 1u;      /* none fitted: the cheapest, over the allowance */
constexpr uint32_t PICK_NONE = 2u;      /* nothing chosen: the frame keeps the stream's QP */
constexpr uint32_t PICK_SHORT = 3u;     /* the probe did not count every rect row of it */

/* bits of se(v) (H.264 9.1.1): codeNum 2|v| - (v > 0) */
__host__ __device__ inline uint32_t se_len(int v)
{
    const uint32_t code = v > 0 ? 2u * (uint32_t)v - 1u : 2u * (uint32_t)(-v);
    return 2u * (31u - (uint32_t)__builtin_clz(code + 1u)) + 1u;
}

__host__ __device__ inline uint32_t cost_of(uint32_t bits, int qp) { return bits + se_len(qp - 26); }

struct Choice {
    int k;              /* the candidate */
    uint32_t cost;      /* its cost */
    uint32_t over;      /* 1: none fitted, k is the cheapest */
};

/* Among the nq candidates r[0..nq) at QPs qp[] whose cost is at most allow:
 * the smallest sse[0] + sse[1] + sse[2], ties to the smaller cost, then to
 * the earlier candidate (h264scroll.pick_qp's rule on cost).  None fits: the
 * smallest cost, ties to the smaller error, then to the earlier one, over = 1. */
__host__ __device__ inline Choice pick(const ScrollDynProbe *r, const uint8_t *qp, int nq, uint64_t allow)
{
    int fit = -1, low = 0;
    uint64_t fit_e = 0, low_e = 0;
    uint32_t fit_c = 0, low_c = 0;
    for (int k = 0; k < nq; ++k) {
        const uint64_t e = r[k].sse[0] + r[k].sse[1] + r[k].sse[2];
        const uint32_t c = cost_of(r[k].bits, qp[k]);
        if (c <= allow && (fit < 0 || e < fit_e || (e == fit_e && c < fit_c))) {
            fit = k;
            fit_e = e;
            fit_c = c;
        }
        if (k == 0 || c < low_c || (c == low_c && e < low_e)) {
            low = k;
            low_e = e;
            low_c = c;
        }
    }
    if (fit >= 0) return Choice{fit, fit_c, 0u};
    return Choice{low, low_c, 1u};
}

/* The leaky bucket of SCROLL_DYN_RATE_BUCKET, one frame of one stream:
 * bucket_allow is what the frame may cost before the clamp at 0 that the pick
 * itself applies; bucket_next the level after a frame of that cost (0: a
 * frame that codes nothing of the rect, or that keeps the stream's QP).  The
 * debt stops at one bucket. */
__host__ __device__ inline int64_t bucket_allow(int64_t level, uint32_t frame_bits, uint32_t bucket_bits)
{
    const int64_t a = level + (int64_t)frame_bits;
    return a < (int64_t)bucket_bits ? a : (int64_t)bucket_bits;
}

__host__ __device__ inline int64_t bucket_next(int64_t allow, uint32_t cost, uint32_t bucket_bits)
{
    const int64_t l = allow - (int64_t)cost;
    return l > -(int64_t)bucket_bits ? l : -(int64_t)bucket_bits;
}

/* what the pick may spend on a frame: frame_bits, or the bucket's allowance clamped at 0 */
__host__ __device__ inline uint64_t pick_allow(uint32_t mode, int64_t level, uint32_t frame_bits,
                                               uint32_t bucket_bits)
{
    if (mode != SCROLL_DYN_RATE_BUCKET) return frame_bits;
    const int64_t a = bucket_allow(level, frame_bits, bucket_bits);
    return a > 0 ? (uint64_t)a : 0u;
}

/* One frame, both modes.  has: the frame has a dynamic NAL, its stream may
 * leave QP 26 and every rect row was counted (else nothing is chosen and it
 * costs 0).  *level moves in bucket mode only.  Returns the choice; k = -1:
 * none. */
__host__ __device__ inline Choice pick_frame(uint32_t mode, const ScrollDynProbe *r, const uint8_t *qp, int nq,
                                             bool has, uint32_t frame_bits, uint32_t bucket_bits, int64_t *level)
{
    Choice c{-1, 0u, 0u};
    if (has) c = pick(r, qp, nq, pick_allow(mode, *level, frame_bits, bucket_bits));
    if (mode == SCROLL_DYN_RATE_BUCKET)
        *level = bucket_next(bucket_allow(*level, frame_bits, bucket_bits), c.cost, bucket_bits);
    return c;
}

}  // namespace pick
}  // namespace scroll

#endif
