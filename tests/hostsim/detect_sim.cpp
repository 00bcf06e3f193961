/*
 * detect_sim.cpp -- TEST-ONLY CPU harness around the rule of the offset
 * detector (h264-scroll-encoder_amd/csrc/detect_device.h), compiled by
 * tests/test_detect_hostsim.py:
 *   dtsim_sig_surface(): a surface -> sigS, four pixels at a time through
 *                        sig4 as k_det_surf's lanes run it;
 *   dtsim_sig_refs():    luma rows -> sigR through ref4, as k_det_refs;
 *   dtsim_detect():      one frame's signatures -> scores and record,
 *                        serially (detect_frame);
 *   dtsim_walk():        the same the way the kernels walk: the scores in
 *                        tiles of 128 rows x 16 segments with k_det_score's
 *                        padding values, 256 candidates a group; the choice
 *                        through 256 partial Top2 merged by a tree, as
 *                        k_det_pick's workgroup does it.
 * With -DDETECT_SIM_MAIN it is a program of its own (random pictures through
 * every entry point, the two walks compared, a checksum printed) for a run
 * under the host sanitizers.
 */
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "detect_device.h"

using namespace scroll;
using namespace scroll::detect;

extern "C" {

int dtsim_record_size(void) { return (int)sizeof(ScrollOffsetFound); }
int dtsim_rule_size(void) { return (int)sizeof(ScrollDetect); }
uint32_t dtsim_nuse(uint32_t pw, uint32_t seg_step) { return nuse(pw, seg_step); }

/* px [h][w] little-endian pixel words -> out [h][nuse] */
void dtsim_sig_surface(int w, int h, const uint32_t *px, uint32_t format, uint32_t matrix, uint32_t full_range,
                       uint32_t seg_step, uint16_t *out)
{
    const csc::Coef k = csc::coef(format, matrix, full_range);
    const uint32_t nu = nuse((uint32_t)w, seg_step);
    for (int y = 0; y < h; ++y)
        for (uint32_t cu = 0; cu < nu; ++cu) {
            uint32_t sum = 0;
            for (uint32_t q = 0; q < 16; ++q) {                 /* the segment's 16 lanes */
                const uint32_t x = cu * seg_step * SEG + 4u * q;
                if (x >= (uint32_t)w) continue;                 /* a partial last segment */
                const uint32_t *p = px + (size_t)y * w + x;
                sum += sig4(k, p[0], p[1], p[2], p[3]);
            }
            out[(size_t)y * nu + cu] = (uint16_t)sum;
        }
}

/* luma [rows][w] -> out [rows][nuse] */
void dtsim_sig_refs(int w, int rows, const uint8_t *luma, uint32_t seg_step, uint16_t *out)
{
    const uint32_t nu = nuse((uint32_t)w, seg_step);
    for (int y = 0; y < rows; ++y)
        for (uint32_t cu = 0; cu < nu; ++cu) {
            uint32_t sum = 0;
            for (uint32_t q = 0; q < 16; ++q) {
                const uint32_t x = cu * seg_step * SEG + 4u * q;
                if (x >= (uint32_t)w) continue;
                uint32_t v;
                memcpy(&v, luma + (size_t)y * w + x, 4);
                sum += ref4(v);
            }
            out[(size_t)y * nu + cu] = (uint16_t)sum;
        }
}

void dtsim_detect(const uint16_t *sigS, const uint16_t *sigR, uint32_t ph, uint32_t nu, int32_t estimate,
                  uint32_t radius, uint32_t min_match, uint32_t *scores, ScrollOffsetFound *out)
{
    *out = detect_frame(sigS, sigR, ph, nu, estimate, radius, min_match, scores);
}

void dtsim_walk(const uint16_t *sigS, const uint16_t *sigR, uint32_t ph, uint32_t nu, int32_t estimate,
                uint32_t radius, uint32_t min_match, uint32_t *scores, ScrollOffsetFound *out)
{
    const uint32_t T = 256, TY = 128, TC = 16, TR = TY + T;
    const Window w = window(estimate, radius, ph);
    for (uint32_t o = 0; o <= ph; ++o) scores[o] = NO_SCORE;
    std::vector<uint16_t> sR((size_t)TC * TR), sS((size_t)TY * TC);
    for (uint32_t o0 = (uint32_t)w.lo; o0 <= (uint32_t)w.hi; o0 += T) {
        std::vector<uint32_t> cnt(T, 0u);
        for (uint32_t y0 = 0; y0 < ph; y0 += TY) {
            const uint32_t ty = TY < ph - y0 ? TY : ph - y0;
            for (uint32_t c0 = 0; c0 < nu; c0 += TC) {
                const uint32_t ncc = TC < nu - c0 ? TC : nu - c0, ncc4 = (ncc + 3u) & ~3u;
                for (uint32_t i = 0; i < ncc4 * TR; ++i) {
                    const uint32_t cc = i / TR, k = i % TR, r = y0 + o0 + k;
                    sR[(size_t)cc * TR + k] = cc < ncc && r < 2u * ph ? sigR[(size_t)r * nu + c0 + cc] : 0xFFFFu;
                }
                for (uint32_t i = 0; i < ty * TC; ++i) {
                    const uint32_t y = i / TC, cc = i % TC;
                    sS[(size_t)y * TC + cc] = cc < ncc ? sigS[(size_t)(y0 + y) * nu + c0 + cc] : 0xFFFEu;
                }
                for (uint32_t t = 0; t < T && o0 + t <= (uint32_t)w.hi; ++t)
                    for (uint32_t y = 0; y < ty; ++y)
                        for (uint32_t cc = 0; cc < ncc4; ++cc)
                            cnt[t] += sS[(size_t)y * TC + cc] == sR[(size_t)cc * TR + y + t] ? 1u : 0u;
            }
        }
        for (uint32_t t = 0; t < T && o0 + t <= (uint32_t)w.hi; ++t) scores[o0 + t] = cnt[t];
    }
    std::vector<Top2> part(T, top2_init());
    for (uint32_t t = 0; t < T; ++t)
        for (uint32_t o = t; o <= ph; o += T)
            if ((int32_t)o >= w.lo && (int32_t)o <= w.hi) top2_add(part[t], key(scores[o], (int32_t)o, w.c0));
    for (uint32_t n = T / 2; n > 0; n >>= 1)
        for (uint32_t t = 0; t < n; ++t) top2_merge(part[t], part[t + n]);
    *out = found(part[0], w, ph * nu, min_match);
}

}  // extern "C"

#ifdef DETECT_SIM_MAIN
int main()
{
    uint64_t x = 0x9e3779b97f4a7c15ull, sum = 0;
    auto rnd = [&]() {
        x ^= x << 13;
        x ^= x >> 7;
        x ^= x << 17;
        return x;
    };
    for (int it = 0; it < 60; ++it) {
        const int w = 16 * (1 + (int)(rnd() % 24)), h = 16 * (1 + (int)(rnd() % 12));
        const uint32_t step = 1u + (uint32_t)(rnd() % nseg((uint32_t)w)), nu = nuse((uint32_t)w, step);
        const int off = (int)(rnd() % (unsigned)(h + 1));
        std::vector<uint8_t> st((size_t)2 * h * w);
        const int mode = it % 3;                                /* noise, flat, bands of 8 rows */
        for (int y = 0; y < 2 * h; ++y)
            for (int c = 0; c < w; ++c)
                st[(size_t)y * w + c] = mode == 0 ? (uint8_t)rnd() : mode == 1 ? 50 : (uint8_t)(y / 8 * 37);
        std::vector<uint32_t> px((size_t)w * h);
        for (int y = 0; y < h; ++y)
            for (int c = 0; c < w; ++c) {
                const uint32_t v = st[(size_t)(y + off) * w + c];
                px[(size_t)y * w + c] = v | v << 8 | v << 16 | (uint32_t)(rnd() & 255u) << 24;
            }
        std::vector<uint16_t> sS((size_t)h * nu), sR((size_t)2 * h * nu);
        dtsim_sig_surface(w, h, px.data(), 0, 0, 1, step, sS.data());     /* grey, full range: luma = v */
        dtsim_sig_refs(w, 2 * h, st.data(), step, sR.data());
        const int32_t est = (int32_t)(rnd() % (unsigned)(h + 40)) - 20;
        const uint32_t radius = it % 5 == 0 ? 0u : it % 5 == 1 ? 100000u : (uint32_t)(rnd() % 300);
        const uint32_t min_match = (uint32_t)(rnd() % (h * nu + 2));
        std::vector<uint32_t> s1((size_t)h + 1), s2((size_t)h + 1);
        ScrollOffsetFound a, b;
        dtsim_detect(sS.data(), sR.data(), (uint32_t)h, nu, est, radius, min_match, s1.data(), &a);
        dtsim_walk(sS.data(), sR.data(), (uint32_t)h, nu, est, radius, min_match, s2.data(), &b);
        if (memcmp(&a, &b, sizeof(a)) != 0 || s1 != s2) {
            printf("detect_sim: serial and tiled walks differ at %d\n", it);
            return 1;
        }
        if (mode == 0 && off >= a.lo && off <= a.hi && a.off != off) {
            printf("detect_sim: noise picture %d found %d, not %d\n", it, a.off, off);
            return 1;
        }
        sum = sum * 31 + (uint32_t)a.off + 3u * a.score + 5u * a.second + 7u * a.status + (uint32_t)a.second_off;
    }
    printf("detect_sim: checksum %016llx\n", (unsigned long long)sum);
    return 0;
}
#endif
