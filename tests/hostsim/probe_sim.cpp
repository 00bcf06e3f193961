/*
 * probe_sim.cpp -- TEST-ONLY CPU harness around the QP probe's device
 * functions (h264-scroll-encoder_amd/csrc/probe_device.h), compiled by
 * tests/test_probe_hostsim.py with the hostsim shim:
 *   psim_block(): one block's TotalCoeff, TrailingOnes, coeff_token and
 *                 body lengths from levels in scan order;
 *   psim_mb():    one MB's bits from given levels and neighbour TotalCoeffs;
 *   psim_rect():  a whole rect from source and prediction pixels at one QP:
 *                 bits, nonzero and squared error, composed as k_dyn_probe
 *                 composes them (levels of the coder, nC across the rect's
 *                 MBs, outside MBs available with 0, picture edges not).
 */
#include <cstdint>
#include <vector>
#include "scroll_device.h"
#include "recon_device.h"
#include "probe_device.h"

using namespace scroll;
using namespace scroll::dyn;
using namespace scroll::recon;
using namespace scroll::probe;

namespace {

constexpr Tabs k_tabs = SCROLL_DYN_TABS;
const PLens g_pl = make_plens(k_tabs);

/* maxc coefficients in scan order -> the raster levels block_len<maxc> takes */
void to_raster(const int *coef, int maxc, int lv[16])
{
    for (int i = 0; i < 16; ++i) lv[i] = 0;
    for (int i = 0; i < maxc; ++i) lv[maxc == 4 ? i : ZZ[maxc == 15 ? i + 1 : i]] = coef[i];
}

int body_of(const int lv[16], int maxc, int &tc, int &t1)
{
    return maxc == 16 ? block_len<16>(g_pl, lv, tc, t1)
                      : maxc == 15 ? block_len<15>(g_pl, lv, tc, t1) : block_len<4>(g_pl, lv, tc, t1);
}

/* one MB's 24 blocks + 2 DC blocks: tt, the bodies' sum, the DC blocks'
 * bits, any_dc, TotalCoeff sum */
struct MbStat {
    uint8_t tt[24];
    int body, dc_bits, nonzero;
    bool any_dc;
};

}  // namespace

extern "C" {

void psim_block(const int *coef, int maxc, int nC, int *tc, int *t1, int *token, int *body)
{
    int lv[16];
    to_raster(coef, maxc, lv);
    *body = body_of(lv, maxc, *tc, *t1);
    *token = token_len(g_pl, *tc, *t1, nC);
}

/* levels as or_dyn_mb_levels_bits takes them: luma[16][16] (raster block,
 * scan order), cdc[2][4], cac[2][4][15]; left / top: 24 TotalCoeffs each */
int psim_mb(const int *luma, const int *cdc, const int *cac, const int *left, const int *top, int avail_l,
            int avail_t, int *nonzero, int *tc_out)
{
    MbStat m{};
    for (int r = 0; r < 24; ++r) {
        int lv[16], tc, t1;
        if (r < 16) to_raster(luma + 16 * r, 16, lv);
        else to_raster(cac + 15 * (r - 16), 15, lv);
        m.body += body_of(lv, r < 16 ? 16 : 15, tc, t1);
        m.tt[r] = (uint8_t)(tc << 2 | t1);
        m.nonzero += tc;
        tc_out[r] = tc;
    }
    for (int p = 0; p < 2; ++p) {
        int lv[16], tc, t1;
        to_raster(cdc + 4 * p, 4, lv);
        m.dc_bits += body_of(lv, 4, tc, t1) + token_len(g_pl, tc, t1, -1);
        m.any_dc |= tc != 0;
        m.nonzero += tc;
    }
    uint8_t l8[24], t8[24];
    for (int i = 0; i < 24; ++i) {
        l8[i] = (uint8_t)left[i];
        t8[i] = (uint8_t)top[i];
    }
    *nonzero = m.nonzero;
    return mb_len(g_pl, m.tt, m.body, m.dc_bits, m.any_dc, avail_l ? l8 : nullptr, avail_t ? t8 : nullptr);
}

/* src, pred: a w x h MB rect in the source layout (384 w h bytes); avail_l /
 * avail_t: the rect does not touch the picture's left / top edge */
void psim_rect(const uint8_t *src, const uint8_t *pred, int w, int h, int qp, int avail_l, int avail_t,
               uint64_t *sse, uint32_t *bits, uint32_t *nonzero)
{
    const int qpc = qp_chroma(qp);
    const QParams ql = qparams_rt(qp), qc = qparams_rt(qpc);
    const DQParams dl = dqparams_rt(qp), dc = dqparams_rt(qpc);
    const int ls = 16 * w, cs = 8 * w;
    std::vector<MbStat> mb((size_t)w * h);
    sse[0] = sse[1] = sse[2] = 0;
    *bits = *nonzero = 0;
    for (int my = 0; my < h; ++my)
        for (int mx = 0; mx < w; ++mx) {
            MbStat &m = mb[(size_t)my * w + mx];
            m = MbStat{};
            for (int r = 0; r < 16; ++r) {
                int s[16], p[16], W[16], lv[16], o[16], tc, t1;
                for (int k = 0; k < 16; ++k) {
                    const size_t at = (size_t)(16 * my + 4 * (r >> 2) + (k >> 2)) * ls + 16 * mx + 4 * (r & 3) + (k & 3);
                    s[k] = src[at];
                    p[k] = pred[at];
                }
                residual_fwd(s, p, W);
                quant4x4<false>(W, lv, ql);
                m.body += block_len<16>(g_pl, lv, tc, t1);
                m.tt[r] = (uint8_t)(tc << 2 | t1);
                m.nonzero += tc;
                sse[0] += recon_coefs<false>(W, 0, s, p, o, ql, dl);
            }
            for (int pl = 0; pl < 2; ++pl) {
                const size_t base = (size_t)256 * w * h + (size_t)pl * 64 * w * h;
                int s[4][16], p[4][16], W[4][16], o[16];
                for (int b = 0; b < 4; ++b) {
                    for (int k = 0; k < 16; ++k) {
                        const size_t at = base + (size_t)(8 * my + 4 * (b >> 1) + (k >> 2)) * cs + 8 * mx + 4 * (b & 1) + (k & 3);
                        s[b][k] = src[at];
                        p[b][k] = pred[at];
                    }
                    residual_fwd(s[b], p[b], W[b]);
                }
                const int w0[4] = {W[0][0], W[1][0], W[2][0], W[3][0]};
                int ld[16] = {quant_dc(w0[0] + w0[1] + w0[2] + w0[3], qc), quant_dc(w0[0] - w0[1] + w0[2] - w0[3], qc),
                              quant_dc(w0[0] + w0[1] - w0[2] - w0[3], qc), quant_dc(w0[0] - w0[1] - w0[2] + w0[3], qc)};
                int dcs[4], tcd, t1d;
                chroma_dc(ld, dcs, dc);
                m.dc_bits += block_len<4>(g_pl, ld, tcd, t1d);
                m.dc_bits += token_len(g_pl, tcd, t1d, -1);
                m.any_dc |= tcd != 0;
                m.nonzero += tcd;
                for (int b = 0; b < 4; ++b) {
                    int lv[16], tc, t1;
                    quant4x4<true>(W[b], lv, qc);
                    m.body += block_len<15>(g_pl, lv, tc, t1);
                    m.tt[16 + 4 * pl + b] = (uint8_t)(tc << 2 | t1);
                    m.nonzero += tc;
                    sse[1 + pl] += recon_coefs<true>(W[b], dcs[b], s[b], p[b], o, qc, dc);
                }
            }
        }
    const uint8_t zero[24] = {};
    for (int my = 0; my < h; ++my)
        for (int mx = 0; mx < w; ++mx) {
            const MbStat &m = mb[(size_t)my * w + mx];
            uint8_t l8[24], t8[24];
            const uint8_t *lp = mx > 0 ? l8 : avail_l ? zero : nullptr;
            const uint8_t *tp = my > 0 ? t8 : avail_t ? zero : nullptr;
            for (int i = 0; i < 24; ++i) {
                if (mx > 0) l8[i] = mb[(size_t)my * w + mx - 1].tt[i] >> 2;
                if (my > 0) t8[i] = mb[(size_t)(my - 1) * w + mx].tt[i] >> 2;
            }
            *bits += (uint32_t)mb_len(g_pl, m.tt, m.body, m.dc_bits, m.any_dc, lp, tp);
            *nonzero += (uint32_t)m.nonzero;
        }
}

}  // extern "C"
