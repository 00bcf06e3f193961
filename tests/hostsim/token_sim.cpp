/*
 * token_sim.cpp -- TEST-ONLY CPU harness around k_dyn_row's token-first
 * CAVLC body (cavlc_body_t with nC and the coeff_token tables,
 * h264-scroll-encoder_amd/csrc/dyn_device.h), compiled by
 * tests/test_token_fold.py as a library and, with -DTOKEN_SIM_MAIN, as a
 * stand-alone program for the sanitizers:
 *   tsim_piece(): one block (int8 levels in scan order) at context nC through
 *                 the tokened cavlc_body_t and through cavlc_body<CapSink,
 *                 true>: each one's 128 bits, length, TotalCoeff,
 *                 TrailingOnes, ok; then the token length the kernel looks up
 *                 again for a piece over 128 bits and which of its three
 *                 forms the piece takes.
 */
#include <cstdint>
#include <cstdio>
#include <cstring>
#include "scroll_device.h"
#include "dyn_device.h"

using namespace scroll;

static const dyn::Tabs g_tabs = SCROLL_DYN_TABS;

extern "C" {

/* out[0..8]: hi (2 words), lo (2 words), n, TotalCoeff, TrailingOnes, ok, 0 of
 * the tokened cavlc_body_t; out[9..17] the same of cavlc_body<CapSink, true>
 * (the body alone); out[18] the token's length from the packed table (the
 * kernel's piece_token); out[19] the piece's form as the kernel's body lane
 * decides it: 0 token in front (n <= 128), 1 the body alone kept (n > 128,
 * n - tl <= 128), 2 the body over 128 bits.  Returns 0, or -1 for a level
 * outside int8 */
int tsim_piece(const int *coef, int maxc, int nC, uint32_t *out)
{
    static dyn::PTabs P;
    static bool init = false;
    if (!init) {
        dyn::build_ptabs(g_tabs, P, 0, 1);
        init = true;
    }
    static constexpr dyn::LvTab lvt = dyn::make_lvt();
    int8_t lb[17] = {0};
    lb[0] = 77;                                       /* the guard byte: any value */
    uint32_t nz = 0, pw[4] = {0, 0, 0, 0};
    for (int i = 0; i < maxc; ++i) {
        if (coef[i] < -128 || coef[i] > 127) return -1;
        lb[1 + i] = (int8_t)coef[i];
        if (coef[i]) nz |= 1u << i;
        pw[i >> 2] |= ((uint32_t)coef[i] & 255u) << (8 * (i & 3));
    }
    uint32_t ntok = 0;
    int tct = 0, t1t = 0;
    for (int which = 0; which < 2; ++which) {
        dyn::CapSink cap{0, 0, 0};
        int t1 = -1, tc;
        bool ok = false;
        if (which == 0)
            tc = dyn::cavlc_body_t(cap, lb + 1, nz, dyn::tzrb_entry(g_tabs, nz, maxc), t1, ok, lvt.e, nC, P.ct);
        else
            tc = dyn::cavlc_body<dyn::CapSink, true>(cap, P, make_uint4(pw[0], pw[1], pw[2], pw[3]), maxc, t1, ok, lb + 1);
        uint32_t *o = out + 9 * which;
        o[0] = (uint32_t)(cap.hi >> 32), o[1] = (uint32_t)cap.hi;
        o[2] = (uint32_t)(cap.lo >> 32), o[3] = (uint32_t)cap.lo;
        o[4] = cap.n, o[5] = (uint32_t)tc, o[6] = (uint32_t)t1, o[7] = ok ? 1u : 0u, o[8] = 0u;
        if (which == 0) ntok = cap.n, tct = tc, t1t = t1;
    }
    /* piece_token (dyn_kernels.hip) from the meta the body lane keeps */
    const uint32_t tl = nC >= 8 ? 6u : (uint32_t)(P.ct[nC < 2 ? 0 : (nC < 4 ? 1 : 2)][4 * tct + t1t] >> 8);
    out[18] = tl;
    out[19] = ntok <= 128u ? 0u : (ntok - tl <= 128u ? 1u : 2u);
    return 0;
}

}  // extern "C"

#ifdef TOKEN_SIM_MAIN
/* every TotalCoeff / level size / context over a fixed pseudo-random walk:
 * the sanitizers' run; the comparisons are test_token_fold.py's */
int main()
{
    uint32_t x = 12345u, out[20];
    long n = 0, forms[3] = {0, 0, 0};
    for (int it = 0; it < 200000; ++it) {
        int coef[16] = {0};
        x = x * 1664525u + 1013904223u;
        const int maxc = (x >> 8) & 1 ? 16 : 15, nC = (int)((x >> 10) % 18u);
        const int big = 1 + (int)((x >> 16) % 127u), fill = 1 + (int)((x >> 24) % 16u);
        for (int i = 0; i < maxc; ++i) {
            x = x * 1664525u + 1013904223u;
            if ((int)((x >> 12) % 16u) < fill) coef[i] = (int)((x >> 16) % (2u * big + 1u)) - big;
        }
        if (it % 97 == 0)
            for (int i = 0; i < maxc; ++i) coef[i] = it % 2 ? -128 : 127;
        if (tsim_piece(coef, maxc, nC, out)) return 2;
        if (out[5] != out[14] || out[6] != out[15]) return 3;
        ++forms[out[19]];
        ++n;
    }
    std::printf("token_sim: %ld blocks, forms %ld / %ld / %ld\n", n, forms[0], forms[1], forms[2]);
    return forms[0] && forms[1] && forms[2] ? 0 : 4;
}
#endif
