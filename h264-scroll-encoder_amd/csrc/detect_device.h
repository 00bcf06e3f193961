/*
 * detect_device.h -- the rule by which a frame's scroll offset is detected
 * from the renderer's surfaces (scroll_batch_detect_offsets).
 *
 * Pure integer functions: k_det_surf, k_det_refs, k_det_score and k_det_pick
 * (detect_kernels.hip) run them, tests/hostsim/detect_sim.cpp compiles them
 * for the CPU and tests/test_detect_hostsim.py checks them against the numpy
 * restatement of tests/detecthelp.py.
 *
 * The picture is pw x ph luma samples.  It is cut into segments of SEG = 64
 * columns, nseg = ceil(pw / 64) of them, the last one 16, 32 or 48 wide when
 * pw is no multiple of 64; of these the segments 0, seg_step, 2 seg_step, ...
 * are used, nuse of them.
 *
 * The stacked reference R[r], r < 2 ph: luma row r of reference picture A
 * for r < ph, row r - ph of B otherwise -- a scroll at offset o shows R[Y + o]
 * in picture row Y (the tearing of the one MB row that straddles A and B and
 * the waypoint chain are the decoder's business: the locate that follows at
 * the detected offset accounts for them as damage).
 *
 * Signatures, both at most 64 * 255 = 16,320 (uint16):
 *     sigR[r][c] = the sum of R[r][x] over segment c
 *     sigS[Y][c] = the sum of csc::luma_px(k, pixel) over segment c of surface row Y
 * The window around the caller's estimate e (the frame's entry of the offsets):
 *     c0 = clamp(e, 0, ph), lo = max(c0 - radius, 0), hi = min(c0 + radius, ph)
 * The score of candidate o, lo <= o <= hi:
 *     score(o) = #{ (Y, used c) : sigS[Y][c] == sigR[Y + o][c] },  Y < ph
 * out of n_sig = ph nuse.  A count of exact agreements: the rows the dynamic
 * rect covers do not vote, where a sum of differences would pull the estimate.
 * The choice: off is the candidate that is largest under (score descending,
 * |o - c0| ascending, o ascending) -- one lexicographic maximum, packed into
 * one uint64 (key()) and max-reduced, so independent of the order of the
 * walk; second / second_off are the score and the offset of the largest of
 * the other candidates under the same key (0 and -1 without another one).
 *     SCROLL_DET_LOW    score < min_match
 *     SCROLL_DET_FOUND  score >= min_match and score > second
 *     SCROLL_DET_TIED   score >= min_match and score == second (a flat or
 *                       periodic page: the offsets cannot be told apart)
 */
#ifndef SCROLL_DETECT_DEVICE_H
#define SCROLL_DETECT_DEVICE_H

#include <stdint.h>

#include "composer_batch.h"     /* ScrollOffsetFound, SCROLL_DET_* */
#include "csc_device.h"

namespace scroll {
namespace detect {

constexpr uint32_t SEG = 64u;
constexpr uint32_t NO_SCORE = 0xFFFFFFFFu;  /* a scores entry outside the window */

/* ---- segments ---- */

__host__ __device__ inline uint32_t nseg(uint32_t pw) { return (pw + SEG - 1u) / SEG; }
__host__ __device__ inline uint32_t nuse(uint32_t pw, uint32_t seg_step) { return (nseg(pw) + seg_step - 1u) / seg_step; }

/* ---- signatures ---- */

/* four surface pixels (memory order): their lumas' sum */
__host__ __device__ inline uint32_t sig4(const csc::Coef &k, uint32_t p0, uint32_t p1, uint32_t p2, uint32_t p3)
{
    return csc::luma_px(k, p0) + csc::luma_px(k, p1) + csc::luma_px(k, p2) + csc::luma_px(k, p3);
}

/* four reference luma bytes (a word): their sum */
__host__ __device__ inline uint32_t ref4(uint32_t v)
{
    return (v & 255u) + ((v >> 8) & 255u) + ((v >> 16) & 255u) + (v >> 24);
}

/* ---- the window ---- */

struct Window {
    int32_t c0, lo, hi;
};

__host__ __device__ inline Window window(int32_t estimate, uint32_t radius, uint32_t ph)
{
    Window w;
    w.c0 = estimate < 0 ? 0 : estimate > (int32_t)ph ? (int32_t)ph : estimate;
    /* radius >= ph: every offset (and no overflow for any uint32 radius) */
    const int32_t r = radius > ph ? (int32_t)ph : (int32_t)radius;
    w.lo = w.c0 - r < 0 ? 0 : w.c0 - r;
    w.hi = w.c0 + r > (int32_t)ph ? (int32_t)ph : w.c0 + r;
    return w;
}

/* ---- the choice ---- */

/* never 0 for a candidate: o <= ph < 0xFFFF */
__host__ __device__ inline uint64_t key(uint32_t score, int32_t o, int32_t c0)
{
    const uint32_t d = (uint32_t)(o < c0 ? c0 - o : o - c0);
    return (uint64_t)score << 32 | (uint64_t)(0xFFFFu - d) << 16 | (uint64_t)(0xFFFFu - (uint32_t)o);
}

__host__ __device__ inline uint32_t key_score(uint64_t k) { return (uint32_t)(k >> 32); }
__host__ __device__ inline int32_t key_off(uint64_t k) { return (int32_t)(0xFFFFu - (uint32_t)(k & 0xFFFFu)); }

/* the two largest keys of the candidates seen; 0: none */
struct Top2 {
    uint64_t a, b;
};

__host__ __device__ inline Top2 top2_init() { return Top2{0u, 0u}; }

__host__ __device__ inline uint64_t max64(uint64_t x, uint64_t y) { return x > y ? x : y; }
__host__ __device__ inline uint64_t min64(uint64_t x, uint64_t y) { return x < y ? x : y; }

__host__ __device__ inline void top2_add(Top2 &t, uint64_t k)
{
    t.b = max64(t.b, min64(t.a, k));
    t.a = max64(t.a, k);
}

/* two walks over disjoint candidates */
__host__ __device__ inline void top2_merge(Top2 &t, const Top2 &u)
{
    const uint64_t b = max64(min64(t.a, u.a), max64(t.b, u.b));
    t.a = max64(t.a, u.a);
    t.b = b;
}

/* the record of a frame from its whole window's Top2 */
__host__ __device__ inline ScrollOffsetFound found(const Top2 &t, const Window &w, uint32_t n_sig, uint32_t min_match)
{
    ScrollOffsetFound r{};
    r.off = key_off(t.a);
    r.centre = w.c0;
    r.score = key_score(t.a);
    r.second = t.b ? key_score(t.b) : 0u;
    r.second_off = t.b ? key_off(t.b) : -1;
    r.n_sig = n_sig;
    r.lo = (uint16_t)w.lo;
    r.hi = (uint16_t)w.hi;
    r.status = (uint16_t)(r.score < min_match ? SCROLL_DET_LOW
                          : t.b && r.score == r.second ? SCROLL_DET_TIED : SCROLL_DET_FOUND);
    return r;
}

/* ---- one frame, serially: the rule as a whole, for the CPU and for reading ----
 * sigS [ph][nu], sigR [2 ph][nu] (the used segments only); scores [ph + 1] */
__host__ __device__ inline uint32_t score_at(const uint16_t *sigS, const uint16_t *sigR, uint32_t ph, uint32_t nu,
                                             uint32_t o)
{
    uint32_t n = 0;
    for (uint32_t Y = 0; Y < ph; ++Y)
        for (uint32_t c = 0; c < nu; ++c) n += sigS[(size_t)Y * nu + c] == sigR[(size_t)(Y + o) * nu + c] ? 1u : 0u;
    return n;
}

__host__ __device__ inline ScrollOffsetFound detect_frame(const uint16_t *sigS, const uint16_t *sigR, uint32_t ph,
                                                          uint32_t nu, int32_t estimate, uint32_t radius,
                                                          uint32_t min_match, uint32_t *scores)
{
    const Window w = window(estimate, radius, ph);
    Top2 t = top2_init();
    for (int32_t o = 0; o <= (int32_t)ph; ++o) {
        if (o < w.lo || o > w.hi) {
            scores[o] = NO_SCORE;
            continue;
        }
        scores[o] = score_at(sigS, sigR, ph, nu, (uint32_t)o);
        top2_add(t, key(scores[o], o, w.c0));
    }
    return found(t, w, ph * nu, min_match);
}

}  // namespace detect
}  // namespace scroll

#endif
