/*
 * damage_sim.cpp -- TEST-ONLY CPU harness around the rule of the dynamic
 * rect's locate (h264-scroll-encoder_amd/csrc/damage_device.h), compiled by
 * tests/test_damage_hostsim.py:
 *   dmsim_locate():  one frame's map -> its record, serially (locate_frame);
 *   dmsim_parts():   the same through 256 partial walks merged by a tree, as
 *                    k_dyn_place's workgroup does it;
 *   dmsim_ypred():   the prediction luma of a whole picture through pred_row
 *                    (regions + luma_row), as k_dmg_rows resolves it;
 *   dmsim_map():     a surface against that prediction -> the map, through
 *                    sq4 as k_dyn_damage's lanes run it.
 * With -DDAMAGE_SIM_MAIN it is a program of its own (random maps and
 * pictures through every entry point, a checksum printed) for a run under
 * the host sanitizers.
 */
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "scroll_device.h"
#include "damage_device.h"

using namespace scroll;
using namespace scroll::damage;

extern "C" {

int dmsim_record_size(void) { return (int)sizeof(ScrollDynDamage); }

void dmsim_locate(const uint32_t *map, uint32_t w, uint32_t h, uint32_t mbw, uint32_t mbh, uint32_t mb_sse,
                  uint32_t margin, ScrollDynDamage *out)
{
    *out = locate_frame(map, w, h, mbw, mbh, mb_sse, margin);
}

void dmsim_noframe(ScrollDynDamage *out, uint32_t *entry)
{
    *out = noframe();
    *entry = pos_entry(*out);
}

/* k_dyn_place's walk: thread t takes MBs t, t + 256, ...; the partial results merge pairwise */
uint32_t dmsim_parts(const uint32_t *map, uint32_t w, uint32_t h, uint32_t mbw, uint32_t mbh, uint32_t mb_sse,
                     uint32_t margin, ScrollDynDamage *out)
{
    const uint32_t T = 256, nmb = mbw * mbh;
    std::vector<Acc> part(T);
    for (uint32_t t = 0; t < T; ++t) {
        Acc a = acc_init();
        for (uint32_t i = t; i < nmb; i += T) acc_add(a, map[i], i % mbw, i / mbw, mb_sse);
        part[t] = a;
    }
    for (uint32_t n = T / 2; n > 0; n >>= 1)
        for (uint32_t t = 0; t < n; ++t) acc_merge(part[t], part[t + n]);
    ScrollDynDamage r = place(part[0], w, h, mbw, mbh, margin);
    uint64_t in = 0;
    if (r.x0 >= 0)
        for (uint32_t i = 0; i < w * h; ++i) {
            const uint32_t mx = (uint32_t)r.x0 + i % w, my = (uint32_t)r.y0 + i / w;
            if (!covered(r, w, h, mx, my)) return 0xDEADu;     /* the rect's own MBs are covered */
            in += map[my * mbw + mx];
        }
    finish(r, in);
    *out = r;
    return pos_entry(r);
}

/* a scroll NAL at offset off with the waypoint table (wo, wv)[nwp]: the luma of pictures a, b ([h][w]) it predicts */
void dmsim_ypred(int w, int h, int off, int nwp, const int32_t *wo, const int32_t *wv, const uint8_t *a,
                 const uint8_t *b, uint8_t *out)
{
    NalCtx c{};
    c.w = w;
    c.h = h;
    c.kind = 0;
    c.off = off;
    c.nwp = nwp;
    c.wp_off = wo;
    c.wp_lt = wo;                  /* regions() does not read the long-term indices */
    c.wp_valid = wv;
    const Regions rg = regions(c);
    const int a_end = (h - off) / 16;
    const dyn::WpTab T{wo, wv, h};
    for (int Y = 0; Y < h; ++Y) {
        int yo;
        const int p = pred_row(T, rg, a_end, Y, yo);
        memcpy(out + (size_t)Y * w, (p ? b : a) + (size_t)yo * w, (size_t)w);
    }
}

/* surface pixels [h][w] (little-endian words) against yp [h][w] -> map [h / 16][w / 16], 4 pixels at a time */
void dmsim_map(int w, int h, const uint32_t *px, const uint8_t *yp, uint32_t format, uint32_t matrix,
               uint32_t full_range, uint32_t *map)
{
    const csc::Coef k = csc::coef(format, matrix, full_range);
    const int mbw = w / 16;
    for (int i = 0; i < mbw * (h / 16); ++i) map[i] = 0;
    for (int y = 0; y < h; ++y)
        for (int x = 0; x < w; x += 4) {
            const uint32_t *p = px + (size_t)y * w + x;
            uint32_t ref;
            memcpy(&ref, yp + (size_t)y * w + x, 4);
            uint32_t &m = map[(y / 16) * mbw + x / 16];
            m = sq4(k, p[0], p[1], p[2], p[3], ref, m);
        }
}

}  // extern "C"

#ifdef DAMAGE_SIM_MAIN
int main()
{
    uint64_t x = 0x9e3779b97f4a7c15ull, sum = 0;
    auto rnd = [&]() {
        x ^= x << 13;
        x ^= x >> 7;
        x ^= x << 17;
        return x;
    };
    for (int it = 0; it < 600; ++it) {
        const uint32_t mbw = 1 + (uint32_t)(rnd() % 40), mbh = 1 + (uint32_t)(rnd() % 30);
        const uint32_t w = 1 + (uint32_t)(rnd() % mbw), h = 1 + (uint32_t)(rnd() % mbh);
        std::vector<uint32_t> map((size_t)mbw * mbh, 0u);
        const int n = (int)(rnd() % 6);
        for (int i = 0; i < n; ++i) map[rnd() % map.size()] = (uint32_t)(rnd() % 100000);
        if (it % 7 == 0)
            for (auto &m : map) m = (uint32_t)(rnd() % 16646400u);
        ScrollDynDamage a, b;
        const uint32_t mb_sse = (uint32_t)(rnd() % 3 ? 0 : rnd() % 50000), margin = (uint32_t)(rnd() % 5);
        dmsim_locate(map.data(), w, h, mbw, mbh, mb_sse, margin, &a);
        const uint32_t e = dmsim_parts(map.data(), w, h, mbw, mbh, mb_sse, margin, &b);
        if (memcmp(&a, &b, sizeof(a)) != 0 || e == 0xDEADu) {
            printf("damage_sim: serial and tree walks differ at %d\n", it);
            return 1;
        }
        sum = sum * 31 + a.status + 3u * (uint32_t)(a.x0 + 1) + 5u * (uint32_t)(a.y0 + 1) + a.sse_out + e;
    }
    for (int it = 0; it < 40; ++it) {
        const int w = 16 * (1 + (int)(rnd() % 3)), h = 16 * (2 + (int)(rnd() % 40));
        std::vector<uint8_t> a((size_t)w * h), b((size_t)w * h), yp((size_t)w * h);
        std::vector<uint32_t> px((size_t)w * h), map((size_t)(w / 16) * (h / 16));
        for (auto &v : a) v = (uint8_t)rnd();
        for (auto &v : b) v = (uint8_t)rnd();
        for (auto &v : px) v = (uint32_t)rnd();
        int32_t wo[8] = {496, 992, 0, 0, 0, 0, 0, 0}, wv[8] = {1, (int32_t)(rnd() & 1), 0, 0, 0, 0, 0, 0};
        const int nwp = (int)(rnd() % 3), off = (int)(rnd() % (unsigned)(h + 1));
        dmsim_ypred(w, h, off, nwp, wo, wv, a.data(), b.data(), yp.data());
        dmsim_map(w, h, px.data(), yp.data(), (uint32_t)(rnd() & 1), (uint32_t)(rnd() & 1), (uint32_t)(rnd() & 1),
                  map.data());
        for (uint32_t m : map) sum = sum * 33 + m;
    }
    printf("damage_sim: checksum %016llx\n", (unsigned long long)sum);
    return 0;
}
#endif
