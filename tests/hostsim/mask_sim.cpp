/*
 * mask_sim.cpp -- TEST-ONLY CPU harness around the rule of the dynamic rect's
 * per-MB source mask (h264-scroll-encoder_amd/csrc/mask_device.h), compiled by
 * tests/test_mask_hostsim.py:
 *   mksim_frame():  one frame's map -> its KEPT bits and record, serially
 *                   (mask_frame);
 *   mksim_parts():  the same the way the kernels walk it: an MB's neighbours
 *                   in four parts OR-ed (k_dyn_mask_fill's lane quad), the
 *                   record through 256 partial walks merged by a tree, the
 *                   chroma split from per-row partials (k_dyn_mask_rec);
 *   mksim_map():    a rect-layout source against its prediction -> the map
 *                   and the Cb part, through sq4b four bytes at a time as the
 *                   lanes of k_dyn_mask_diff run it.
 * With -DMASK_SIM_MAIN it is a program of its own (random maps and rects
 * through every entry point, the two walks compared, a checksum printed) for
 * a run under the host sanitizers.
 */
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "mask_device.h"

using namespace scroll::mask;

static ScrollDynMaskRule rule_of(uint32_t ty, uint32_t tc, uint32_t grow)
{
    ScrollDynMaskRule r{};
    r.mb_sse_y = ty;
    r.mb_sse_c = tc;
    r.grow = (uint8_t)grow;
    r.apply = 1;
    return r;
}

extern "C" {

int mksim_record_size(void) { return (int)sizeof(ScrollDynMask); }
int mksim_rule_size(void) { return (int)sizeof(ScrollDynMaskRule); }

void mksim_frame(uint32_t *map, const uint32_t *dcb, uint32_t w, uint32_t h, uint32_t ty, uint32_t tc, uint32_t grow,
                 ScrollDynMask *out)
{
    *out = mask_frame(map, dcb, w, h, rule_of(ty, tc, grow));
}

void mksim_noframe(ScrollDynMask *out) { *out = noframe(); }

/* 0, or 0xDEAD when the quad's four parts disagree with the whole */
uint32_t mksim_parts(uint32_t *map, const uint32_t *dcb, uint32_t w, uint32_t h, uint32_t ty, uint32_t tc,
                     uint32_t grow, ScrollDynMask *out)
{
    const ScrollDynMaskRule r = rule_of(ty, tc, grow);
    const uint32_t T = 256, nmb = w * h;
    /* k_dyn_mask_fill: per rect row the Cb / Cr error of the MBs its quads do not keep */
    std::vector<uint64_t> part(2 * (size_t)h, 0);
    for (uint32_t my = 0; my < h; ++my)
        for (uint32_t mx = 0; mx < w; ++mx) {
            bool kp = false;
            for (uint32_t q = 0; q < 4; ++q) kp |= kept_part(map, w, h, mx, my, r, q, 4u);
            if (kp != kept_part(map, w, h, mx, my, r, 0u, 1u)) return 0xDEADu;
            if (!kp) {
                const size_t i = (size_t)my * w + mx;
                part[2 * my] += dcb[i];
                part[2 * my + 1] += (map[2 * i + 1] & ~KEPT) - dcb[i];
            }
        }
    /* k_dyn_mask_rec: thread t takes MBs t, t + 256, ... and rows t, t + 256, ... */
    std::vector<Acc> acc(T);
    std::vector<uint32_t> e1(nmb);
    for (uint32_t t = 0; t < T; ++t) {
        Acc a = acc_init();
        for (uint32_t i = t; i < nmb; i += T) e1[i] = acc_mb(a, map, w, h, i % w, i / w, r);
        for (uint32_t y = t; y < h; y += T) {
            a.drop[1] += part[2 * y];
            a.drop[2] += part[2 * y + 1];
        }
        acc[t] = a;
    }
    for (uint32_t i = 0; i < nmb; ++i) map[2 * i + 1] = e1[i];
    for (uint32_t n = T / 2; n > 0; n >>= 1)
        for (uint32_t t = 0; t < n; ++t) acc_merge(acc[t], acc[t + n]);
    *out = record(acc[0]);
    return 0;
}

/* src, pred: [384 w h] in the source layout -> map [h][w][2], dcb [h][w] */
void mksim_map(const uint8_t *src, const uint8_t *pred, uint32_t w, uint32_t h, uint32_t *map, uint32_t *dcb)
{
    const size_t n = (size_t)w * h;
    for (size_t i = 0; i < n; ++i) map[2 * i] = map[2 * i + 1] = dcb[i] = 0;
    auto word = [](const uint8_t *p) {
        uint32_t v;
        memcpy(&v, p, 4);
        return v;
    };
    for (uint32_t y = 0; y < 16 * h; ++y)
        for (uint32_t x = 0; x < 16 * w; x += 4) {
            const size_t at = (size_t)y * 16 * w + x;
            uint32_t &m = map[2 * ((size_t)(y / 16) * w + x / 16)];
            m = sq4b(word(src + at), word(pred + at), m);
        }
    for (int p = 0; p < 2; ++p)
        for (uint32_t y = 0; y < 8 * h; ++y)
            for (uint32_t x = 0; x < 8 * w; x += 4) {
                const size_t at = 256 * n + (size_t)p * 64 * n + (size_t)y * 8 * w + x;
                const size_t i = (size_t)(y / 8) * w + x / 8;
                const uint32_t d = sq4b(word(src + at), word(pred + at), 0u);
                map[2 * i + 1] += d;
                if (p == 0) dcb[i] += d;
            }
}

}  // extern "C"

#ifdef MASK_SIM_MAIN
int main()
{
    uint64_t x = 0x9e3779b97f4a7c15ull, sum = 0;
    auto rnd = [&]() {
        x ^= x << 13;
        x ^= x >> 7;
        x ^= x << 17;
        return x;
    };
    for (int it = 0; it < 400; ++it) {
        const uint32_t w = 1 + (uint32_t)(rnd() % 20), h = 1 + (uint32_t)(rnd() % 14);
        const size_t n = (size_t)w * h;
        std::vector<uint32_t> map(2 * n, 0u), dcb(n, 0u);
        const int k = it % 5 == 0 ? (int)n : (int)(rnd() % 6);
        for (int i = 0; i < k; ++i) {
            const size_t at = it % 5 == 0 ? (size_t)i : (size_t)(rnd() % n);
            map[2 * at] = (uint32_t)(rnd() % 16646401u);
            map[2 * at + 1] = (uint32_t)(rnd() % 8323201u) | (rnd() & 1 ? KEPT : 0u);     /* stale KEPT bits */
            dcb[at] = (uint32_t)(rnd() % ((map[2 * at + 1] & ~KEPT) + 1u));
        }
        const uint32_t ty = (uint32_t)(rnd() % 3 ? 0 : rnd() % 9000000), tc = (uint32_t)(rnd() % 3 ? 0 : rnd() % 5000000);
        const uint32_t grow = (uint32_t)(rnd() % 3);
        std::vector<uint32_t> m1 = map, m2 = map;
        ScrollDynMask a, b;
        mksim_frame(m1.data(), dcb.data(), w, h, ty, tc, grow, &a);
        if (mksim_parts(m2.data(), dcb.data(), w, h, ty, tc, grow, &b) || memcmp(&a, &b, sizeof(a)) != 0 || m1 != m2) {
            printf("mask_sim: serial and kernel walks differ at %d\n", it);
            return 1;
        }
        sum = sum * 31 + a.n_changed + 3u * a.n_kept + a.sse_drop[0] + 5u * a.sse_drop[1] + 7u * a.sse_drop[2];
        for (uint32_t v : m1) sum = sum * 33 + v;
    }
    for (int it = 0; it < 40; ++it) {
        const uint32_t w = 1 + (uint32_t)(rnd() % 5), h = 1 + (uint32_t)(rnd() % 4);
        const size_t n = (size_t)w * h;
        std::vector<uint8_t> src(384 * n), pred(384 * n);
        for (auto &v : src) v = (uint8_t)rnd();
        for (auto &v : pred) v = (uint8_t)rnd();
        std::vector<uint32_t> map(2 * n), dcb(n);
        mksim_map(src.data(), pred.data(), w, h, map.data(), dcb.data());
        for (uint32_t v : map) sum = sum * 33 + v;
        for (uint32_t v : dcb) sum = sum * 35 + v;
    }
    ScrollDynMask nf;
    mksim_noframe(&nf);
    printf("mask_sim: checksum %016llx\n", (unsigned long long)(sum + (uint64_t)nf.status));
    return 0;
}
#endif
