/*
 * csc_sim.cpp -- TEST-ONLY CPU harness around the surface entry's conversion
 * rule (h264-scroll-encoder_amd/csrc/csc_device.h), compiled by
 * tests/test_csc_hostsim.py:
 *   cssim_luma():    n pixels (4 bytes each, memory order) -> n luma bytes;
 *   cssim_chroma():  n quads (4 pixels each: top left, top right, bottom
 *                    left, bottom right) -> n Cb and n Cr bytes;
 *   cssim_coef():    the coefficients coef() hands the kernel;
 *   cssim_window():  a w x h window of a pitched surface -> its I420 block,
 *                    patch by patch through the flat task index as k_csc
 *                    walks it (divmod by the magic multiplier included).
 * With -DCSC_SIM_MAIN it is a program of its own (random surfaces through all
 * three, every variant, a checksum printed) for a run under the host
 * sanitizers.
 */
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "csc_device.h"

using namespace scroll::csc;

static uint32_t px_at(const uint8_t *p)
{
    uint32_t v;
    memcpy(&v, p, 4);
    return v;           /* (little-endian hosts, as the device) */
}

extern "C" {

void cssim_luma(uint32_t format, uint32_t matrix, uint32_t full, const uint8_t *px, size_t n, uint8_t *y)
{
    const Coef k = coef(format, matrix, full);
    for (size_t i = 0; i < n; ++i) y[i] = (uint8_t)luma_px(k, px_at(px + 4 * i));
}

void cssim_chroma(uint32_t format, uint32_t matrix, uint32_t full, const uint8_t *quads, size_t n, uint8_t *cb,
                  uint8_t *cr)
{
    const Coef k = coef(format, matrix, full);
    for (size_t i = 0; i < n; ++i) {
        const uint8_t *q = quads + 16 * i;
        uint32_t s02, s1;
        quad_sums(px_at(q), px_at(q + 4), px_at(q + 8), px_at(q + 12), &s02, &s1);
        cb[i] = (uint8_t)chroma_quad(k.cb, s02, s1);
        cr[i] = (uint8_t)chroma_quad(k.cr, s02, s1);
    }
}

/* w, h multiples of 16; out: w h 3 / 2 bytes */
void cssim_window(uint32_t format, uint32_t matrix, uint32_t full, const uint8_t *src, size_t pitch, uint32_t w,
                  uint32_t h, uint8_t *out)
{
    const Coef k = coef(format, matrix, full);
    const uint32_t cw = w / 8u, tpi = (h / 2u) * cw, m_cw = magic(cw);
    uint8_t *cbp = out + (size_t)w * h, *crp = cbp + (size_t)w * h / 4;
    for (uint32_t t = 0; t < tpi; ++t) {
        uint32_t cg;
        const uint32_t rp = divmod(t, cw, m_cw, &cg);
        for (uint32_t row = 0; row < 2; ++row)
            for (uint32_t i = 0; i < 8; ++i)
                out[(size_t)(2 * rp + row) * w + 8 * cg + i] =
                    (uint8_t)luma_px(k, px_at(src + (size_t)(2 * rp + row) * pitch + 4 * (size_t)(8 * cg + i)));
        for (uint32_t q = 0; q < 4; ++q) {
            const uint8_t *t0 = src + (size_t)(2 * rp) * pitch + 4 * (size_t)(8 * cg + 2 * q), *b0 = t0 + pitch;
            uint32_t s02, s1;
            quad_sums(px_at(t0), px_at(t0 + 4), px_at(b0), px_at(b0 + 4), &s02, &s1);
            cbp[(size_t)rp * (w / 2) + 4 * cg + q] = (uint8_t)chroma_quad(k.cb, s02, s1);
            crp[(size_t)rp * (w / 2) + 4 * cg + q] = (uint8_t)chroma_quad(k.cr, s02, s1);
        }
    }
}

/* the header's coefficients by byte position: y[3], yoff, cb[3], cr[3] */
void cssim_coef(uint32_t format, uint32_t matrix, uint32_t full, int32_t out[10])
{
    const Coef k = coef(format, matrix, full);
    for (int i = 0; i < 3; ++i) {
        out[i] = k.y[i];
        out[4 + i] = k.cb[i];
        out[7 + i] = k.cr[i];
    }
    out[3] = k.yoff;
}

/* n / d and n % d by csc_device.h's divmod */
uint32_t cssim_divmod(uint32_t n, uint32_t d, uint32_t *rem) { return divmod(n, d, magic(d), rem); }

}  // extern "C"

#ifdef CSC_SIM_MAIN
int main()
{
    uint64_t x = 0x9e3779b97f4a7c15ull, sum = 0;
    auto rnd = [&]() {
        x ^= x << 13;
        x ^= x >> 7;
        x ^= x << 17;
        return x;
    };
    for (int it = 0; it < 64; ++it) {
        const uint32_t fmt = it & 1, mat = (it >> 1) & 1, full = (it >> 2) & 1;
        const uint32_t w = 16u * (1u + (uint32_t)(rnd() % 5)), h = 16u * (1u + (uint32_t)(rnd() % 3));
        const size_t pitch = 4 * (size_t)w + 16 * (size_t)(rnd() % 3);
        std::vector<uint8_t> src(pitch * h), out((size_t)w * h * 3 / 2), y((size_t)w), cb(w / 4), cr(w / 4);
        for (auto &b : src) b = (uint8_t)rnd();
        cssim_window(fmt, mat, full, src.data(), pitch, w, h, out.data());
        cssim_luma(fmt, mat, full, src.data(), w, y.data());
        cssim_chroma(fmt, mat, full, src.data(), w / 4, cb.data(), cr.data());
        for (uint8_t b : out) sum = sum * 31 + b;
        for (uint8_t b : y) sum = sum * 31 + b;
        for (size_t i = 0; i < cb.size(); ++i) sum = sum * 31 + cb[i] + 3u * cr[i];
        if (memcmp(y.data(), out.data(), w)) {
            printf("csc_sim: the window's first luma row differs from cssim_luma\n");
            return 1;
        }
    }
    for (int it = 0; it < 100000; ++it) {
        const uint32_t n = (uint32_t)rnd(), d = 1u + (uint32_t)(rnd() % (it & 1 ? 100000u : 0xFFFFFFFFu));
        uint32_t r;
        const uint32_t q = cssim_divmod(n, d, &r);
        if (q != n / d || r != n % d) {
            printf("csc_sim: divmod(%u, %u) = %u r %u\n", n, d, q, r);
            return 1;
        }
    }
    printf("csc_sim: checksum %016llx\n", (unsigned long long)sum);
    return 0;
}
#endif
