/*
 * body_sim.cpp -- TEST-ONLY CPU harness around k_dyn_row's CAVLC phase
 * (h264-scroll-encoder_amd/csrc/dyn_device.h), compiled by
 * tests/test_body_schedule.py the way sim.cpp is:
 *   bsim_bodies(): one block (int8 levels in scan order) through
 *                 cavlc_body_t and through cavlc_body<CapSink, true>: each
 *                 one's 128 body bits, length, TotalCoeff, TrailingOnes, ok.
 */
#include <cstdint>
#include <cstring>
#include "scroll_device.h"
#include "dyn_device.h"

using namespace scroll;

static const dyn::Tabs g_tabs = SCROLL_DYN_TABS;

extern "C" {

/* out[2][9]: hi (2 words), lo (2 words), n, TotalCoeff, TrailingOnes, ok, 0
 * of cavlc_body_t (row 0) and cavlc_body<CapSink, true> (row 1); returns 0,
 * or -1 for a level outside int8 */
int bsim_bodies(const int *coef, int maxc, uint32_t *out)
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
    for (int which = 0; which < 2; ++which) {
        dyn::CapSink cap{0, 0, 0};
        int t1 = -1, tc;
        bool ok = false;
        if (which == 0)
            tc = dyn::cavlc_body_t(cap, lb + 1, nz, dyn::tzrb_entry(g_tabs, nz, maxc), t1, ok, lvt.e);
        else
            tc = dyn::cavlc_body<dyn::CapSink, true>(cap, P, make_uint4(pw[0], pw[1], pw[2], pw[3]), maxc, t1, ok, lb + 1);
        uint32_t *o = out + 9 * which;
        o[0] = (uint32_t)(cap.hi >> 32), o[1] = (uint32_t)cap.hi;
        o[2] = (uint32_t)(cap.lo >> 32), o[3] = (uint32_t)cap.lo;
        o[4] = cap.n, o[5] = (uint32_t)tc, o[6] = (uint32_t)t1, o[7] = ok ? 1u : 0u, o[8] = 0u;
    }
    return 0;
}

}  // extern "C"
