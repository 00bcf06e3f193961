/*
 * size_sim.cpp -- TEST-ONLY CPU harness around the host and rule code of the
 * dynamic rect sized per frame (scroll_batch_set_dyn_rect_size_at, DESIGN.md
 * §3p), compiled by tests/test_dyn_size_hostsim.py:
 *   szsim_pack() / szsim_unpack():  the position table's word (dyn_pos.h);
 *   szsim_groups_at():              the row groups of a placement with h_f;
 *   szsim_sized_max():              the most groups / static groups / region
 *                                   words over every legal (y0, h_f);
 *   szsim_place():                  one frame's map -> its record and table
 *                                   entry, with and without size
 *                                   (damage_device.h: locate_frame, and
 *                                   k_dyn_place's walk over the sized rect).
 * With -DSIZE_SIM_MAIN it is a program of its own (random pictures through
 * every entry point, a checksum printed) for a run under the host sanitizers.
 */
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "scroll_device.h"
#include "damage_device.h"
#include "dyn_pos.h"

using namespace scroll;
using namespace scroll::damage;

extern "C" {

uint32_t szsim_pack(uint32_t x0, uint32_t y0, uint32_t dw, uint32_t dh) { return dyn_pos_pack(x0, y0, dw, dh); }

void szsim_unpack(uint32_t e, uint32_t pos_mask, int32_t *out)
{
    const DynPosWord p = dyn_pos_unpack(e, pos_mask);
    out[0] = p.x0;
    out[1] = p.y0;
    out[2] = p.dw;
    out[3] = p.dh;
}

int szsim_static_rows(void) { return DYN_STATIC_ROWS; }

int szsim_groups_at(int y0, int h, int mbh) { return dyn_groups_at(y0, h, mbh); }

int szsim_groups_max(int h, int mbh) { return dyn_groups_max(h, mbh); }

void szsim_sized_max(int h, int mbh, uint64_t sw, uint64_t rw, uint64_t *out)
{
    const DynSizedMax m = dyn_sized_max(h, mbh, sw, rw);
    out[0] = (uint64_t)m.groups;
    out[1] = (uint64_t)m.statics;
    out[2] = m.words;
}

/* the record through locate_frame, and again as k_dyn_place makes it: place,
 * then the sum over the placed (sized) rect's own MBs.  Returns the table
 * entry, 0xDEAD0000 if the two records differ */
uint32_t szsim_place(const uint32_t *map, uint32_t w, uint32_t h, uint32_t mbw, uint32_t mbh, uint32_t mb_sse,
                     uint32_t margin, uint32_t size, ScrollDynDamage *out)
{
    *out = locate_frame(map, w, h, mbw, mbh, mb_sse, margin, size);
    Acc a = acc_init();
    for (uint32_t i = 0; i < mbw * mbh; ++i) acc_add(a, map[i], i % mbw, i / mbw, mb_sse);
    ScrollDynDamage r = place(a, w, h, mbw, mbh, margin, size);
    const uint32_t wf = placed_w(r, w, size), hf = placed_h(r, h, size);
    uint64_t in = 0;
    if (r.x0 >= 0)
        for (uint32_t i = 0; i < wf * hf; ++i)
            in += map[((uint32_t)r.y0 + i / wf) * mbw + (uint32_t)r.x0 + i % wf];
    finish(r, in);
    if (memcmp(&r, out, sizeof(r)) != 0) return 0xDEAD0000u;
    return size ? pos_entry_sized(r, w, h) : pos_entry(r);
}

}  // extern "C"

#ifdef SIZE_SIM_MAIN
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
        const uint32_t mbw = 1 + (uint32_t)(rnd() % 40), mbh = 1 + (uint32_t)(rnd() % 30);
        const uint32_t w = 1 + (uint32_t)(rnd() % mbw), h = 1 + (uint32_t)(rnd() % mbh);
        std::vector<uint32_t> map((size_t)mbw * mbh, 0u);
        const int n = (int)(rnd() % 6);
        for (int i = 0; i < n; ++i) map[rnd() % map.size()] = (uint32_t)(rnd() % 100000);
        ScrollDynDamage a, b;
        const uint32_t margin = (uint32_t)(rnd() % 5);
        const uint32_t e0 = szsim_place(map.data(), w, h, mbw, mbh, 0, margin, 0, &a);
        const uint32_t e1 = szsim_place(map.data(), w, h, mbw, mbh, 0, margin, 1, &b);
        if (e0 == 0xDEAD0000u || e1 == 0xDEAD0000u || a.reserved != 0) {
            printf("size_sim: the two walks differ at %d\n", it);
            return 1;
        }
        if (b.x0 >= 0) {
            int32_t p[4];
            szsim_unpack(e1, 0xffu, p);
            const uint32_t wf = w - (uint32_t)p[2], hf = h - (uint32_t)p[3];
            if (p[0] != b.x0 || p[1] != b.y0 || wf < 1 || wf > w || hf < 1 || hf > h ||
                (uint32_t)b.x0 + wf > mbw || (uint32_t)b.y0 + hf > mbh || (e0 & 0xff00ff00u) != 0) {
                printf("size_sim: a sized rect leaves its bounds at %d\n", it);
                return 1;
            }
        }
        sum = sum * 31 + e0 + 7u * e1 + a.sse_out + 3u * b.sse_out;
    }
    for (int mbh = 1; mbh <= 60; ++mbh)
        for (int h = 1; h <= mbh; ++h) {
            uint64_t o[3];
            szsim_sized_max(h, mbh, 100 + (uint64_t)(rnd() % 50), 300 + (uint64_t)(rnd() % 900), o);
            if ((int)o[0] < szsim_groups_max(h, mbh)) {
                printf("size_sim: fewer groups than the unsized maximum\n");
                return 1;
            }
            sum = sum * 31 + o[0] + o[1] + o[2];
        }
    printf("size_sim checksum %llu\n", (unsigned long long)sum);
    return 0;
}
#endif
