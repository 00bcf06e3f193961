"""The designed corpus (tests/designed.py) proves itself: every oracle NAL of
the corpus is parsed by the independent decoder tests/h264_pslice.py with its
cavlc_block wrapped as a tally, and the tallies must show every CAVLC table
entry, every reachable level triple, the block-length edges and the extreme
levels that tests/test_gpu_designed.py then demands byte for byte of the
kernels.  The expected sets come from the standard's tables as h264_pslice.py
holds them and from the standard's level rule; what no source picture can
produce is on a named list with its reason.  No GPU."""
import pytest

import designed as dz
import h264_pslice as hp
from dynhelp import split_nals

MB_BITS_MAX = 16384                       # dyn_device.h


# ------------------------------------------------------------- the tally -----
class Tally:
    """hp.cavlc_block with a record of every call: (nC, maxc, coefficients,
    coded bits by the parser's position before and after)"""

    def __init__(self):
        self.orig, self.blocks = hp.cavlc_block, []

    def __call__(self, bits, nC, maxc):
        p0 = bits.p
        coef, tc = self.orig(bits, nC, maxc)
        self.blocks.append((nC, maxc, tuple(coef), bits.p - p0))
        return coef, tc


def column(nC):
    return -1 if nC == -1 else (8 if nC >= 8 else (4 if nC >= 4 else (2 if nC >= 2 else 0)))


def level_triples(levels, tc, t1):
    """the standard's level rule (9.2.2.1, as hp.cavlc_block states it) from
    the encoder's side: levels in coding order after the trailing ones ->
    [(suffixLength when coded, first-level adjustment, level_prefix, level)]"""
    out = []
    sl = 1 if (tc > 10 and t1 < 3) else 0
    for i, v in enumerate(levels):
        code = 2 * v - 2 if v > 0 else -2 * v - 1
        adj = i == 0 and t1 < 3
        if adj:
            code -= 2
        if sl == 0:
            prefix = code if code < 14 else (14 if code < 30 else 15)
        else:
            prefix = min(15, code >> sl)
        out.append((sl, adj, prefix, v))
        if sl == 0:
            sl = 1
        if abs(v) > (3 << (sl - 1)) and sl < 6:
            sl += 1
    return out


def analyse(nC, maxc, coef):
    """-> dict(ct, tz, rb: table entries; triples)"""
    nz = [k for k, v in enumerate(coef) if v]
    tc = len(nz)
    lv = [coef[k] for k in reversed(nz)]
    t1 = 0
    while t1 < min(3, tc) and abs(lv[t1]) == 1:
        t1 += 1
    d = dict(ct=(column(nC), tc, t1), tz=None, rb=[], triples=level_triples(lv[t1:], tc, t1), tc=tc, t1=t1)
    if tc and tc < maxc:
        tz = nz[-1] + 1 - tc
        d["tz"] = (tc, tz)
        zl = tz
        for hi, lo in zip(reversed(nz), list(reversed(nz))[1:]):
            if zl <= 0:
                break
            run = hi - lo - 1
            d["rb"].append((min(zl, 7), run))
            zl -= run
    return d


def reachable_triples(vmax):
    """every (suffixLength, adjusted, level_prefix) the standard's rule gives a
    level 1 .. vmax of either sign in any context: the first level after t1
    trailing ones with TotalCoeff <= 10 (suffixLength 0; adjusted unless t1 = 3,
    and then never +-1) or above 10 with t1 < 3 (suffixLength 1, adjusted), and
    a later level at suffixLength 1 .. 6"""
    out = set()
    for v in range(1, vmax + 1):
        for s in (v, -v):
            if v >= 2:
                out.add(level_triples([s], 1, 0)[0][:3])
                out.add(level_triples([s], 11, 0)[0][:3])
            out.add(level_triples([s], 4, 3)[0][:3])
            for sl in range(1, 7):
                code = 2 * s - 2 if s > 0 else -2 * s - 1
                out.add((sl, False, min(15, code >> sl)))
    return out


# entries of the expected sets that no source picture can produce
UNREACHABLE_RUN_BEFORE_15 = {
    # a 15-coefficient block codes a run_before only with TotalCoeff >= 2, which
    # leaves at most 13 zeros: run_before 14 needs zerosLeft 14
    (7, 14),
}


@pytest.fixture(scope="module")
def tallies(oracle):
    """per case: the blocks of stream 0's NALs, per frame and in parse order,
    and per frame the levels of every rect MB"""
    out = {}
    t = Tally()
    hp.cavlc_block = t
    try:
        for name, c in dz.cases(oracle).items():
            nals = split_nals(dz.want_of(oracle, name)[0])
            assert len(nals) == c.F
            frames = []
            for nal in nals:
                t.blocks = []
                mbs = {}

                def on_mb(x, y, ref, mvd, cbp, luma, cdc, cac):
                    if dz.X0 <= x < dz.X0 + c.rw and dz.Y0 <= y < dz.Y0 + c.rh:
                        mbs[(x - dz.X0, y - dz.Y0)] = (cbp, luma, cdc, cac, len(t.blocks))
                    else:
                        assert cbp == 0

                H, n = hp.parse_p_slice(nal, c.w, c.h, on_mb=on_mb)
                assert H["qp_delta"] == c.qp - 26 and len(mbs) == c.rw * c.rh
                frames.append((t.blocks, mbs))
            out[name] = frames
    finally:
        hp.cavlc_block = t.orig
    return out


def blocks_of(tallies, oracle, groups):
    for name, frames in tallies.items():
        c = dz.cases(oracle)[name]
        if c.group in groups:
            for blocks, _ in frames:
                for b in blocks:
                    yield c, b


def test_group_a_round_trip(tallies, oracle):
    """the designed levels of the table-walk cases come back exactly: all of
    group a (QP 28); the share of its QP-20 redesign and of the level walks is
    printed (their conditions are on what the parser finds)"""
    share = {}
    for name, frames in tallies.items():
        c = dz.cases(oracle)[name]
        same = total = 0
        for fr, (_, mbs) in zip(c.frames, frames):
            for key, (luma, cdc, cac) in fr.design.items():
                _, gl, gdc, gac, _ = mbs[key]
                for a, b in zip(luma, gl):
                    total += 1
                    same += list(a) == list(b)
                for p in range(2):
                    total += 1
                    same += list(cdc[p]) == list(gdc[p])
                    for a, b in zip(cac[p], gac[p]):
                        total += 1
                        same += list(a) == list(b)
        if total:
            g = share.setdefault(c.group, [0, 0])
            g[0] += same
            g[1] += total
    for g, (same, total) in sorted(share.items()):
        print(f"group {g} round trip: {same} of {total} designed blocks came back exactly "
              f"({100.0 * same / total:.2f} %)")
    assert share["a"][0] == share["a"][1]


def test_table_entries(tallies, oracle):
    """coeff_token, total_zeros and run_before: every entry, on the int8 path
    (groups a-d, QP >= 22) and again on the general path (below 22)"""
    for label, groups in (("QP >= 22", ("a", "b", "c", "d")), ("QP < 22", ("a20", "e"))):
        ct, tz, rb = {16: set(), 15: set(), 4: set()}, {16: set(), 15: set(), 4: set()}, {16: set(), 15: set()}
        for c, (nC, maxc, coef, _) in blocks_of(tallies, oracle, groups):
            d = analyse(nC, maxc, coef)
            ct[maxc].add(d["ct"])
            if d["tz"]:
                tz[maxc].add(d["tz"])
            if maxc != 4:
                rb[maxc].update(d["rb"])
        want_ct16 = {(col, tc, t1) for col in (0, 2, 4, 8) for tc, t1 in dz.token_entries(16)}
        want_ct15 = {(col, tc, t1) for col in (0, 2, 4, 8) for tc, t1 in dz.token_entries(15)}
        want_dc = {(-1, tc, t1) for tc, t1 in hp.CT_TABLES[-1].values()}
        want_tz16 = {(tc, z) for tc, row in hp.TZ.items() for z in row.values()}
        want_tz15 = {(tc, z) for tc, z in want_tz16 if tc + z <= 15 and tc < 15}
        want_tzdc = {(tc, z) for tc, row in hp.TZDC.items() for z in row.values()}
        want_rb = {(zl, r) for zl, row in hp.RB.items() for r in row.values()}
        assert len(want_ct16) == 248 and len(want_dc) == 14 and len(want_tz16) == 135 and len(want_rb) == 42
        print(f"{label}: coeff_token {len(ct[16])}/248 luma, {len(ct[15])}/{len(want_ct15)} chroma AC, "
              f"{len(ct[4])}/14 chroma DC; total_zeros {len(tz[16])}/135, {len(tz[15])}/{len(want_tz15)}, "
              f"{len(tz[4])}/{len(want_tzdc)}; run_before {len(rb[16])}/42 luma, "
              f"{len(rb[15])}/{len(want_rb - UNREACHABLE_RUN_BEFORE_15)} chroma AC")
        assert ct[16] == want_ct16, sorted(want_ct16 - ct[16])
        assert ct[15] == want_ct15, sorted(want_ct15 - ct[15])
        assert ct[4] == want_dc, sorted(want_dc - ct[4])
        assert tz[16] == want_tz16, sorted(want_tz16 - tz[16])
        assert tz[15] == want_tz15, sorted(want_tz15 - tz[15])
        assert tz[4] == want_tzdc, sorted(want_tzdc - tz[4])
        assert rb[16] == want_rb, sorted(want_rb - rb[16])
        assert rb[15] == want_rb - UNREACHABLE_RUN_BEFORE_15, sorted(want_rb - rb[15])


def test_level_triples(tallies, oracle):
    """every reachable (suffixLength, adjustment, level_prefix) occurs, both
    signs of |v| = 47, 48, 127 (and 2063 below QP 22), 127 at QP 22"""
    for label, groups, vmax, marks in (("QP >= 22", ("a", "b", "c", "d"), 127, (47, 48, 127)),
                                       ("QP < 22", ("a20", "e"), 2063, (47, 48, 127, 2063))):
        seen, levels, at22, big = {16: set(), 15: set(), 4: set()}, set(), set(), 0
        for c, (nC, maxc, coef, _) in blocks_of(tallies, oracle, groups):
            d = analyse(nC, maxc, coef)
            for sl, adj, prefix, v in d["triples"]:
                seen[maxc].add((sl, adj, prefix))
                levels.add(v)
                if c.qp == 22 and maxc != 4:
                    at22.add(v)
            if maxc != 4:
                big = max(big, max((abs(v) for v in coef), default=0))
        want = reachable_triples(vmax)
        both = seen[16] | seen[15] | seen[4]
        print(f"{label}: level triples {len(both & want)}/{len(want)} (luma {len(seen[16] & want)}, "
              f"chroma AC {len(seen[15] & want)}, chroma DC {len(seen[4] & want)}); "
              f"largest luma / chroma AC |level| {big}, largest of all {max(abs(v) for v in levels)}")
        for m in marks:
            assert m in levels and -m in levels, m
        if vmax == 127:
            assert 127 in at22 and -127 in at22 and big == 127
        missing = want - both - UNREACHABLE_TRIPLES[label]
        assert not missing, sorted(missing)
        assert not (UNREACHABLE_TRIPLES[label] & both), sorted(UNREACHABLE_TRIPLES[label] & both)


UNREACHABLE_TRIPLES = {"QP >= 22": set(), "QP < 22": set()}


def test_block_length_edges(tallies, oracle):
    """blocks of exactly 64, 65, 128 and 129 coded bits, luma and chroma AC,
    on both paths; the same for the bits after coeff_token (the kernels'
    accumulator holds those); the largest chroma DC block and MB"""
    ctlen = {}
    for col, table in hp.CT_TABLES.items():
        for code, e in table.items():
            ctlen[(col,) + e] = len(code)
    for label, groups in (("QP >= 22", ("a", "b", "c", "d")), ("QP < 22", ("a20", "e"))):
        total, body, dcmax = {16: set(), 15: set()}, {16: set(), 15: set()}, 0
        edge = {16: set(), 15: set()}
        for c, (nC, maxc, coef, n) in blocks_of(tallies, oracle, groups):
            if maxc == 4:
                dcmax = max(dcmax, n)
                continue
            d = analyse(nC, maxc, coef)
            total[maxc].add(n)
            body[maxc].add(n - ctlen.get(d["ct"], 6))
            assert dz.body_pushes(coef, maxc)[1][-1:] in ([], [n - ctlen.get(d["ct"], 6)])
            edge[maxc].add(dz.accumulator_edge(coef, maxc))
        print(f"{label}: longest block luma {max(total[16])}, chroma AC {max(total[15])}, chroma DC {dcmax} bits")
        for maxc in (16, 15):
            for n in (64, 65, 128, 129):
                assert n in total[maxc], (label, maxc, n, "coded bits")
                assert n in body[maxc], (label, maxc, n, "bits after coeff_token")
        if label == "QP >= 22":
            # k_dyn_row's 64-bit accumulator: a codeword that fills it to exactly 64, 65 and 66
            # bits while its top bit is a one (a spill one bit late would lose that bit)
            print(f"accumulator edges: luma {sorted(e for e in edge[16] if e)}, "
                  f"chroma AC {sorted(e for e in edge[15] if e)}")
            assert {64, 65, 66} <= edge[16] and {64, 65, 66} <= edge[15]
        assert dcmax <= 118                       # 6 bits of coeff_token + 4 x 28: never past 128


def test_largest_mb(tallies, oracle):
    """the residual bits of the largest MB of the corpus, next to MB_BITS_MAX"""
    best = (0, None)
    for name, frames in tallies.items():
        for f, (blocks, mbs) in enumerate(frames):
            starts = sorted((v[4], k) for k, v in mbs.items())       # blocks parsed before the MB's callback
            prev = 0
            for end, key in starts:
                bits = sum(b[3] for b in blocks[prev:end])
                prev = end
                best = max(best, (bits, (name, f, key)))
    print(f"largest MB: {best[0]} residual bits ({best[1]}), MB_BITS_MAX {MB_BITS_MAX}")
    assert 4000 < best[0] < MB_BITS_MAX


def test_all_zero_rect_between_coded_frames(tallies, oracle):
    for name, frames in tallies.items():
        if "extremes" in name:
            assert all(v[0] == 0 for v in frames[1][1].values())
            assert any(v[0] for v in frames[0][1].values()) and any(v[0] for v in frames[2][1].values())


def test_chroma_dc_clamp(tallies, oracle):
    """+-2063 in each of the four chroma DC positions at QP 0-5, and mixed
    signs within a block"""
    for qp in range(6):
        pos, mixed, top = set(), False, 0
        for blocks, _ in tallies[f"e_clamp_qp{qp}"]:
            for nC, maxc, coef, _ in blocks:
                if maxc == 4:
                    pos.update((k, v) for k, v in enumerate(coef) if abs(v) == 2063)
                    mixed = mixed or (min(coef) < 0 < max(coef))
                    top = max(top, max(abs(v) for v in coef))
        # 8.5-style forward chroma DC of the largest sum, 64 x 255, before the clamp
        unclamped = (16320 * dz._MF[qp % 6][0] + 2 * ((1 << 15) // 6)) >> 16
        print(f"QP {qp}: largest chroma DC level {top} (unclamped {unclamped})")
        assert top == min(unclamped, 2063)
        if unclamped < 2063:                      # QP 4 and 5: 2040 and 1813, the clamp is out of reach
            assert qp in (4, 5)
            continue
        assert pos == {(k, s * 2063) for k in range(4) for s in (1, -1)}, (qp, sorted(pos))
        assert mixed


def test_level_table_edge(tallies, oracle):
    """k_dyn_row's level table ends at |v| = 47 (LVT_V); 47 and 48 of both
    signs are coded in each of its nine classes -- suffixLength 0 .. 6, and
    the adjusted first level at suffixLength 0 and 1 -- in luma and chroma AC
    blocks of the int8 path"""
    seen = set()
    for c, (nC, maxc, coef, _) in blocks_of(tallies, oracle, ("a", "b", "c", "d")):
        if maxc != 4:
            for sl, adj, _, v in analyse(nC, maxc, coef)["triples"]:
                if abs(v) in (47, 48):
                    seen.add((sl, adj, v))
    classes = [(sl, False) for sl in range(7)] + [(0, True), (1, True)]
    want = {(sl, adj, v) for sl, adj in classes for v in (47, -47, 48, -48)}
    print(f"level table edge: {len(seen & want)}/{len(want)} (class, +-47 / +-48)")
    assert want <= seen, sorted(want - seen)


def split_t_mismatch(hostsim, oracle, tallies, groups=("a", "b", "c", "d")):
    """the corpus's int8 blocks through the CPU build of k_dyn_row's block
    coder (sim_cavlc_split_t: cavlc_body_t + coeff_token, or cavlc_block where
    the body passes 128 bits) against or_cavlc_block -> (blocks compared, the
    first (case, nC, maxc, coefficients) that differs or None)"""
    import ctypes
    words = (ctypes.c_uint32 * 64)()
    tc = ctypes.c_int()
    seen, n = set(), 0
    for c, (nC, maxc, coef, nbits) in blocks_of(tallies, oracle, groups):
        if maxc == 4 or (nC, maxc, coef) in seen:
            continue
        seen.add((nC, maxc, coef))
        ob = (ctypes.c_uint8 * 128)()
        bits = dz.OrBits()
        oracle.or_bits_init(ctypes.byref(bits), ob, len(ob))
        ca = (ctypes.c_int * 16)(*coef)
        oracle.or_cavlc_block(ctypes.byref(bits), ca, maxc, nC)
        assert bits.nbits == nbits                    # the restatement's bits are what the parser read
        n += 1
        for fn in (hostsim.sim_cavlc_split_t, hostsim.sim_cavlc_split):     # k_dyn_row's form, k_dyn_code's
            ctypes.memset(words, 0, ctypes.sizeof(words))
            got = fn(ca, maxc, nC, 5, words, ctypes.byref(tc))
            same = got == nbits and all(((words[(5 + i) >> 5] >> (31 - ((5 + i) & 31))) & 1) ==
                                        ((ob[i >> 3] >> (7 - (i & 7))) & 1) for i in range(nbits))
            if not same:
                return n, (c.name, nC, maxc, coef)
    return n, None


def test_cpu_build_codes_the_corpus(tallies, oracle, hostsim):
    """every distinct luma / chroma AC block of the int8 cases through the CPU
    build of k_dyn_row's block coder: the level table, the re-code of a block
    with a level past 47, the 64-bit accumulator's spill and the 128-bit
    overflow give or_cavlc_block's bits"""
    n, bad = split_t_mismatch(hostsim, oracle, tallies)
    print(f"CPU build: {n} distinct designed blocks equal or_cavlc_block")
    assert bad is None, bad
    assert n > 5000


def test_chroma_dc_block_bound(oracle):
    """a chroma DC block never passes 118 bits: 6 of coeff_token and four
    28-bit escapes (or_cavlc_block over every 4-vector of the extreme and
    threshold levels), so the coders' branch for a chroma DC block over 128
    bits (M_OVF in k_dyn_code_general and k_dyn_row) cannot be taken"""
    import itertools
    vals = [0, 1, -1, 2, -2, 8, -8, 16, -16, 17, -17, 2063, -2063]
    longest = max(dz.coded_bits(oracle, list(v), 4, -1) for v in itertools.product(vals, repeat=4))
    print(f"longest chroma DC block: {longest} bits")
    assert longest == 6 + 4 * 28 == 118
