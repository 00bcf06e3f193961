/*
 * pick_sim.cpp -- TEST-ONLY CPU harness around the rule of the rect's
 * per-frame QP pick (h264-scroll-encoder_amd/csrc/pick_device.h), compiled by
 * tests/test_pick_hostsim.py:
 *   pksim_pick():    one frame's candidates at an allowance -> the choice;
 *   pksim_stream():  one stream's frames in either mode, as k_dyn_pick walks
 *                    them (the table byte and the status per frame, the
 *                    bucket's level across them).
 * With -DPICK_SIM_MAIN it is a program of its own (random tables through
 * both entry points, a checksum printed) for a run under the host sanitizers.
 */
#include <cstdint>
#include <cstdio>
#include <vector>

#include "pick_device.h"

using namespace scroll::pick;

extern "C" {

int pksim_se_len(int v) { return (int)se_len(v); }

int pksim_pick(const ScrollDynProbe *r, const uint8_t *qp, int nq, uint64_t allow, int *over, uint32_t *cost)
{
    const Choice c = pick(r, qp, nq, allow);
    *over = (int)c.over;
    *cost = c.cost;
    return c.k;
}

/* frames [F] of SCROLL_DYN_PROBE_MAX_QPS candidates each; has[f]: the frame
 * can be chosen for.  entry[f]: the table byte; status[f]: PICK_*; k[f] */
void pksim_stream(uint32_t mode, const ScrollDynProbe *r, const uint8_t *qp, int nq, const uint8_t *has, int F,
                  uint32_t frame_bits, uint32_t bucket_bits, int64_t *level, int *k, int *status, uint8_t *entry)
{
    for (int f = 0; f < F; ++f) {
        const Choice c = pick_frame(mode, r + (size_t)f * SCROLL_DYN_PROBE_MAX_QPS, qp, nq, has[f] != 0, frame_bits,
                                    bucket_bits, level);
        k[f] = c.k;
        status[f] = c.k < 0 ? (int)PICK_NONE : c.over ? (int)PICK_OVER : (int)PICK_OK;
        entry[f] = c.k < 0 ? 0xFFu : qp[c.k];
    }
}

}  // extern "C"

#ifdef PICK_SIM_MAIN
int main()
{
    uint64_t x = 0x9e3779b97f4a7c15ull, sum = 0;
    auto rnd = [&]() {
        x ^= x << 13;
        x ^= x >> 7;
        x ^= x << 17;
        return x;
    };
    for (int it = 0; it < 2000; ++it) {
        const int F = 1 + (int)(rnd() % 12), nq = 1 + (int)(rnd() % SCROLL_DYN_PROBE_MAX_QPS);
        std::vector<ScrollDynProbe> r((size_t)F * SCROLL_DYN_PROBE_MAX_QPS);
        std::vector<uint8_t> has(F), entry(F);
        std::vector<int> k(F), st(F);
        uint8_t qp[SCROLL_DYN_PROBE_MAX_QPS];
        for (int i = 0; i < nq; ++i) qp[i] = (uint8_t)(rnd() % 52);
        for (auto &p : r) {
            for (auto &e : p.sse) e = rnd() % 5000;
            p.bits = (uint32_t)(rnd() % 3000);
            p.nonzero = 0;
        }
        for (auto &h : has) h = rnd() % 5 != 0;
        int64_t level = (int64_t)(rnd() % 4000) - 2000;
        const uint32_t mode = it & 1 ? SCROLL_DYN_RATE_BUCKET : SCROLL_DYN_RATE_FRAME;
        pksim_stream(mode, r.data(), qp, nq, has.data(), F, (uint32_t)(rnd() % 3000), (uint32_t)(rnd() % 6000),
                     &level, k.data(), st.data(), entry.data());
        for (int f = 0; f < F; ++f) sum = sum * 31 + (uint64_t)(k[f] + 1) * 7 + (uint64_t)st[f] + entry[f];
        sum += (uint64_t)level;
    }
    printf("pick_sim: checksum %016llx\n", (unsigned long long)sum);
    return 0;
}
#endif
