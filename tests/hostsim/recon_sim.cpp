/*
 * recon_sim.cpp -- TEST-ONLY CPU harness around the reconstruction's device
 * functions (h264-scroll-encoder_amd/csrc/recon_device.h), compiled by
 * tests/test_recon_hostsim.py with the hostsim shim:
 *   rsim_recon_mb():   one MB from given levels (the decoder's half);
 *   rsim_recon_rect(): a whole rect from source and prediction pixels (the
 *                      coder's levels, then the decoder's half) + its SSE.
 */
#include <cstdint>
#include "scroll_device.h"
#include "recon_device.h"

using namespace scroll;
using namespace scroll::dyn;
using namespace scroll::recon;

extern "C" {

/* QPc of QP as the kernels take it (Table 8-15) */
int rsim_qpc(int qp) { return qp_chroma(qp); }

/* levels as the slice parser delivers them: luma[16][16] (raster block, scan
 * order), cdc[2][4], cac[2][4][15] (scan order from index 1); predictions
 * py[16][16], pu / pv[8][8]; luma at qp, chroma at QPc of qp */
void rsim_recon_mb(const int *luma, const int *cdc, const int *cac, const uint8_t *py, const uint8_t *pu,
                   const uint8_t *pv, int qp, uint8_t *ry, uint8_t *ru, uint8_t *rv)
{
    const DQParams dl = dqparams_rt(qp), dc = dqparams_rt(qp_chroma(qp));
    for (int r = 0; r < 16; ++r) {
        const int bx = 4 * (r & 3), by = 4 * (r >> 2);
        int lv[16], pred[16], out[16];
        for (int k = 0; k < 16; ++k) lv[ZZ[k]] = luma[16 * r + k];
        for (int p = 0; p < 16; ++p) pred[p] = py[(by + (p >> 2)) * 16 + bx + (p & 3)];
        recon_levels<false>(lv, 0, pred, out, dl);
        for (int p = 0; p < 16; ++p) ry[(by + (p >> 2)) * 16 + bx + (p & 3)] = (uint8_t)out[p];
    }
    for (int pl = 0; pl < 2; ++pl) {
        const uint8_t *pp = pl ? pv : pu;
        uint8_t *rp = pl ? rv : ru;
        int dcs[4];
        chroma_dc(cdc + 4 * pl, dcs, dc);
        for (int k = 0; k < 4; ++k) {
            const int bx = 4 * (k & 1), by = 4 * (k >> 1);
            int lv[16], pred[16], out[16];
            lv[0] = 0;
            for (int i = 1; i < 16; ++i) lv[ZZ[i]] = cac[(4 * pl + k) * 15 + i - 1];
            for (int p = 0; p < 16; ++p) pred[p] = pp[(by + (p >> 2)) * 8 + bx + (p & 3)];
            recon_levels<true>(lv, dcs[k], pred, out, dc);
            for (int p = 0; p < 16; ++p) rp[(by + (p >> 2)) * 8 + bx + (p & 3)] = (uint8_t)out[p];
        }
    }
}

/* src, pred, out: a w x h MB rect in the source layout (384 w h bytes: luma
 * 16w x 16h, then Cb, Cr 8w x 8h); sse: Y, Cb, Cr */
void rsim_recon_rect(const uint8_t *src, const uint8_t *pred, int w, int h, int qp, uint8_t *out, uint64_t *sse)
{
    const QParams ql = qparams_rt(qp), qc = qparams_rt(qp_chroma(qp));
    const DQParams dl = dqparams_rt(qp), dc = dqparams_rt(qp_chroma(qp));
    const int ls = 16 * w, cs = 8 * w;
    sse[0] = sse[1] = sse[2] = 0;
    for (int by = 0; by < 4 * h; ++by)
        for (int bx = 0; bx < 4 * w; ++bx) {
            int s[16], p[16], o[16];
            for (int k = 0; k < 16; ++k) {
                const size_t at = (size_t)(4 * by + (k >> 2)) * ls + 4 * bx + (k & 3);
                s[k] = src[at];
                p[k] = pred[at];
            }
            sse[0] += recon_luma4x4(s, p, o, ql, dl);
            for (int k = 0; k < 16; ++k) out[(size_t)(4 * by + (k >> 2)) * ls + 4 * bx + (k & 3)] = (uint8_t)o[k];
        }
    for (int pl = 0; pl < 2; ++pl) {
        const size_t base = (size_t)256 * w * h + (size_t)pl * 64 * w * h;
        for (int my = 0; my < h; ++my)
            for (int mx = 0; mx < w; ++mx) {
                int s[4][16], p[4][16], o[4][16];
                for (int b = 0; b < 4; ++b)
                    for (int k = 0; k < 16; ++k) {
                        const size_t at = base + (size_t)(8 * my + 4 * (b >> 1) + (k >> 2)) * cs + 8 * mx + 4 * (b & 1) + (k & 3);
                        s[b][k] = src[at];
                        p[b][k] = pred[at];
                    }
                sse[1 + pl] += recon_chroma8x8(s, p, o, qc, dc);
                for (int b = 0; b < 4; ++b)
                    for (int k = 0; k < 16; ++k)
                        out[base + (size_t)(8 * my + 4 * (b >> 1) + (k >> 2)) * cs + 8 * mx + 4 * (b & 1) + (k & 3)] = (uint8_t)o[b][k];
            }
    }
}

}  // extern "C"
