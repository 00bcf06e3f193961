/*
 * hrecon_sim.cpp -- TEST-ONLY CPU harness around the prediction fetch of the
 * reconstruction under UI hints (h264-scroll-encoder_amd/csrc/
 * hrecon_device.h), compiled by tests/test_hrecon_hostsim.py with the hostsim
 * shim:
 *   hsim_pred_mb():    one MB's prediction at a motion (ref, mvx, mvy), block
 *                      by block as k_hdyn_recon's lanes fetch it;
 *   hsim_recon_rect(): a whole rect from source pixels and per-MB motion to
 *                      the reconstruction and its SSE (recon_device.h on that
 *                      prediction).
 * refs: pictures A and B as I420, one after the other (the device layout).
 */
#include <cstdint>
#include "scroll_device.h"
#include "hrecon_device.h"

using namespace scroll;
using namespace scroll::dyn;
using namespace scroll::recon;
using namespace scroll::hrecon;

namespace {

void unpack_rows(const uint32_t pv[4], int o[16])
{
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) o[4 * i + j] = (int)byte_of(pv[i], j);
}

/* the MB's prediction as raster blocks: luma[16][16], chroma[2][4][16].
 * Returns chroma_needs_gen, which picks the instantiation as the kernel does */
bool pred_mb(const WpTab &T, const Pics &P, int ref, int mvx, int mvy, int mbx, int mby, int luma[16][16],
             int chroma[2][4][16])
{
    const bool gen = chroma_needs_gen(T, ref, mvy, mby);
    for (int k = 0; k < 16; ++k) {
        uint32_t pv[4];
        pred_luma4x4(T, P, ref, mvx, mvy, 16 * mbx + 4 * (k & 3), 16 * mby + 4 * (k >> 2), pv);
        unpack_rows(pv, luma[k]);
    }
    for (int p = 0; p < 2; ++p)
        for (int k = 0; k < 4; ++k) {
            uint32_t pv[4];
            const int X = 8 * mbx + 4 * (k & 1), Y = 8 * mby + 4 * (k >> 1);
            if (gen) pred_chroma4x4<true>(T, P, ref, p, mvx, mvy, X, Y, pv);
            else pred_chroma4x4<false>(T, P, ref, p, mvx, mvy, X, Y, pv);
            unpack_rows(pv, chroma[p][k]);
        }
    return gen;
}

}  // namespace

extern "C" {

/* py[16][16], pu / pv[8][8]; returns 1 when the chroma went through the
 * half-pel waypoint path (GEN) */
int hsim_pred_mb(const uint8_t *refs, int w, int h, const int32_t *wo, const int32_t *wv, int ref, int mvx, int mvy,
                 int mbx, int mby, uint8_t *py, uint8_t *pu, uint8_t *pv)
{
    const WpTab T{wo, wv, h};
    const Pics P{refs, w, h};
    int luma[16][16], chroma[2][4][16];
    const bool gen = pred_mb(T, P, ref, mvx, mvy, mbx, mby, luma, chroma);
    for (int k = 0; k < 16; ++k)
        for (int q = 0; q < 16; ++q) py[(4 * (k >> 2) + (q >> 2)) * 16 + 4 * (k & 3) + (q & 3)] = (uint8_t)luma[k][q];
    for (int p = 0; p < 2; ++p)
        for (int k = 0; k < 4; ++k)
            for (int q = 0; q < 16; ++q)
                (p ? pv : pu)[(4 * (k >> 1) + (q >> 2)) * 8 + 4 * (k & 1) + (q & 3)] = (uint8_t)chroma[p][k][q];
    return gen ? 1 : 0;
}

/* motion[3 (ly rw + lx)] = (ref, mvx, mvy) of the rect's MBs; src, out: the
 * rw x rh MB rect in the source layout (384 rw rh bytes); sse: Y, Cb, Cr */
void hsim_recon_rect(const uint8_t *refs, int w, int h, const int32_t *wo, const int32_t *wv, const int32_t *motion,
                     int x0, int y0, int rw, int rh, const uint8_t *src, int qp, uint8_t *out, uint64_t *sse)
{
    const WpTab T{wo, wv, h};
    const Pics P{refs, w, h};
    const QParams ql = qparams_rt(qp), qc = qparams_rt(qp_chroma(qp));
    const DQParams dl = dqparams_rt(qp), dc = dqparams_rt(qp_chroma(qp));
    const int ls = 16 * rw, cs = 8 * rw;
    sse[0] = sse[1] = sse[2] = 0;
    for (int ly = 0; ly < rh; ++ly)
        for (int lx = 0; lx < rw; ++lx) {
            const int32_t *m = motion + 3 * (ly * rw + lx);
            int luma[16][16], chroma[2][4][16];
            pred_mb(T, P, m[0], m[1], m[2], x0 + lx, y0 + ly, luma, chroma);
            for (int k = 0; k < 16; ++k) {
                int s[16], o[16];
                const size_t at = (size_t)(16 * ly + 4 * (k >> 2)) * ls + 16 * lx + 4 * (k & 3);
                for (int q = 0; q < 16; ++q) s[q] = src[at + (size_t)(q >> 2) * ls + (q & 3)];
                sse[0] += recon_luma4x4(s, luma[k], o, ql, dl);
                for (int q = 0; q < 16; ++q) out[at + (size_t)(q >> 2) * ls + (q & 3)] = (uint8_t)o[q];
            }
            for (int p = 0; p < 2; ++p) {
                const size_t base = (size_t)256 * rw * rh + (size_t)p * 64 * rw * rh;
                int s[4][16], o[4][16];
                for (int k = 0; k < 4; ++k)
                    for (int q = 0; q < 16; ++q)
                        s[k][q] = src[base + (size_t)(8 * ly + 4 * (k >> 1) + (q >> 2)) * cs + 8 * lx + 4 * (k & 1) + (q & 3)];
                sse[1 + p] += recon_chroma8x8(s, chroma[p], o, qc, dc);
                for (int k = 0; k < 4; ++k)
                    for (int q = 0; q < 16; ++q)
                        out[base + (size_t)(8 * ly + 4 * (k >> 1) + (q >> 2)) * cs + 8 * lx + 4 * (k & 1) + (q & 3)] = (uint8_t)o[k][q];
            }
        }
}

}  // extern "C"
