"""The designed splice corpus (tests/splicedesign.py) proves itself: every
external slice of the corpus and every NAL the oracle composes from it is
parsed by the independent decoder tests/h264_pslice.py with its cavlc_block
wrapped as a tally.  The tallies must show every CAVLC table entry parsed in
every nC class, every entry re-coded for every reachable (external, composed)
class pair, every level triple, the length and phase edges, the motion and QP
limits and the emulation-prevention positions that
tests/test_gpu_splice_designed.py then demands byte for byte of
k_splice_parse, k_splice_lanes and k_splice_stage.  Conditions are on what
the parser finds, never on the design's intent; what cannot occur is on a
named list with its reason.  No GPU."""
import ctypes
import itertools

import pytest

import h264_pslice as hp
import splicedesign as sd
import designed as dz
from dynhelp import OrCfg, split_nals, splice_of
from test_designed_oracle import column, analyse, reachable_triples
from test_splice_oracle import SpliceMb

EXACT, PSKIP, SPEC = 0, 1, 2

CTLEN = {(col,) + e: len(code) for col, table in hp.CT_TABLES.items() for code, e in table.items()}
TZLEN = {tc: {z: len(code) for code, z in row.items()} for tc, row in hp.TZ.items()}
TZDCLEN = {tc: {z: len(code) for code, z in row.items()} for tc, row in hp.TZDC.items()}
RBLEN = {zl: {r: len(code) for code, r in row.items()} for zl, row in hp.RB.items()}


def codes(nC, maxc, coef):
    """the codewords of a block by the standard's rule and tables:
    [(kind, bit offset in the block, length)], kind ct / t1 / lv / tz / rb"""
    d = analyse(nC, maxc, coef)
    out = [("ct", 0, CTLEN.get(d["ct"], 6))]
    p = out[0][2]
    if d["tc"] == 0:
        return out, p
    if d["t1"]:
        out.append(("t1", p, d["t1"]))
        p += d["t1"]
    for sl, adj, prefix, v in d["triples"]:
        if prefix >= 15:
            n = 28
        elif sl == 0:
            n = 19 if prefix == 14 else prefix + 1
        else:
            n = prefix + 1 + sl
        out.append(("lv", p, n))
        p += n
    if d["tz"]:
        n = (TZDCLEN if maxc == 4 else TZLEN)[d["tz"][0]][d["tz"][1]]
        out.append(("tz", p, n))
        p += n
    for zl, run in d["rb"]:
        out.append(("rb", p, RBLEN[zl][run]))
        p += RBLEN[zl][run]
    return out, p


class Tally:
    """hp.cavlc_block with a record of every call (MB by the decoder's trace,
    nC, maxc, coefficients, bit position in the slice's RBSP, coded bits) and
    hp.Bits.se with a record of every value, its code length and the number of
    blocks parsed before it"""

    def __init__(self):
        self.orig, self.orig_se = hp.cavlc_block, hp.Bits.se
        self.blocks, self.trace, self.se = [], [], []

    def block(self, bits, nC, maxc):
        p0 = bits.p
        coef, tc = self.orig(bits, nC, maxc)
        self.blocks.append((self.trace[-1][0], nC, maxc, tuple(coef), p0, bits.p - p0))
        return coef, tc

    def decode(self, nal, w, h, predictor, **kw):
        t = self
        self.blocks, self.trace, self.se = [], [], []

        def se(b):
            p0 = b.p
            v = t.orig_se(b)
            t.se.append((v, b.p - p0, len(t.blocks)))
            return v
        hp.cavlc_block, hp.Bits.se = self.block, se
        try:
            H, mbs = hp.decode_p_slice(nal, w, h, predictor, trace=self.trace, **kw)
        finally:
            hp.cavlc_block, hp.Bits.se = self.orig, self.orig_se
        return H, mbs, self.blocks, self.se


def mb_pieces(d):
    """decoded MB -> {piece: coefficients} of its coded pieces"""
    out = {}
    if d["skip"] or d["intra"] == 3:
        return out
    i16 = d["intra"] == 2
    for r in range(16):
        out[r] = d["luma"][r][1:] if i16 else d["luma"][r]
    for p in range(2):
        out[16 + p] = d["cdc"][p]
        for k in range(4):
            out[18 + 4 * p + k] = d["cac"][p][k]
    if i16:
        out[26] = d["dc16"]
    return out


def tc_t1(coef):
    lv = [v for v in reversed(coef) if v]
    t1 = 0
    while t1 < min(3, len(lv)) and abs(lv[t1]) == 1:
        t1 += 1
    return len(lv), t1


class Rec:
    """what the decoder found in one (case, picture, shape)"""


@pytest.fixture(scope="module")
def corpus(oracle):
    """every picture of every case in every shape: the external slices decoded
    and parsed by the oracle, the oracle's composed NAL (one mode per picture,
    the three modes in turn) decoded"""
    out = []
    t = Tally()
    buf = (ctypes.c_uint8 * (4 << 20))()
    err = ctypes.c_int()
    for case in sd.cases().values():
        for si, shape in enumerate(case.shapes):
            c = sd.cfg_of(oracle, case.w, case.h)
            for ti, (pic, off) in enumerate(zip(case.pics, case.offs)):
                r = Rec()
                r.case, r.pic, r.shape, r.ti = case, pic, shape, ti
                r.nal = pic.nal(oracle, shape)
                r.mode = case.modes[(ti + si) % len(case.modes)]
                sp = splice_of(pic.at[0], pic.at[1], pic.W, pic.H, r.nal)
                c2 = OrCfg.from_buffer_copy(c)
                k = oracle.or_compose_splice(buf, len(buf), ctypes.byref(c), off, 0, None, 0, r.mode,
                                             ctypes.byref(sp), ctypes.byref(err))
                r.status = err.value
                assert r.status == pic.status, (case.name, shape, ti, err.value)
                mbs = (SpliceMb * (pic.W * pic.H))()
                rb = (ctypes.c_uint8 * (len(r.nal) + 8))()
                rn = ctypes.c_size_t()
                # the parse sees the references of the frame: after the waypoint, if one was due
                cp = OrCfg.from_buffer_copy(c)
                assert oracle.or_splice_parse(ctypes.byref(cp), ctypes.byref(sp), mbs, rb, ctypes.byref(rn)) == pic.status
                r.parsed = mbs
                if pic.status:
                    assert k == 0 and bytes(c) == bytes(c2)          # nothing committed
                    r.ext = None
                    out.append(r)
                    continue
                r.nrefs = 2 + c.nwp
                r.H, r.ext, r.eblocks, r.ese = t.decode(r.nal, 16 * pic.W, 16 * pic.H, "spec")
                r.comp_nal = split_nals(bytes(buf[:k]))[-1]
                r.CH, r.comp, r.cblocks, r.cse = t.decode(r.comp_nal, case.w, case.h, "ref" if r.mode == EXACT else "spec")
                out.append(r)
    return out


def good(corpus, *groups):
    return [r for r in corpus if r.ext is not None and (not groups or r.case.group in groups)]


# ------------------------------------------------- the oracle against the decoder
def test_size_and_routes(corpus):
    routes = sd.route_mbs()
    print("designed MBs per parse route:", routes, "total", sum(routes.values()))
    assert all(v > 1000 for v in routes.values())
    assert sum(routes.values()) == sum(c.n_mbs() for c in sd.cases().values())


def test_oracle_parse_reports_what_the_decoder_finds(corpus):
    """or_splice_parse: ref, motion, cbp, QP, TotalCoeff and TrailingOnes of
    every MB and piece"""
    n = 0
    for r in good(corpus):
        W = r.pic.W
        for y in range(r.pic.H):
            for x in range(W):
                d, m = r.ext[y][x], r.parsed[y * W + x]
                key = (r.case.name, r.shape, r.ti, x, y)
                assert (m.ref, m.mx, m.my, m.cbp, bool(m.skip), m.intra) == \
                    (d["ref"], d["mx"], d["my"], d["cbp"], d["skip"], d["intra"]), key
                if d["intra"]:
                    assert m.mbt == d["mbt"], key
                else:
                    assert [(m.bref[k], m.bmx[k], m.bmy[k]) for k in range(16)] == d["blocks"], key
                    assert m.part == min(d["mbt"], 3), key
                if m.hasqpd:
                    assert m.qp == d["qp"], key
                assert bool(m.hasqpd) == bool(d["intra"] == 2 or (d["cbp"] and d["intra"] != 3)), key
                for i, coef in mb_pieces(d).items():
                    assert (m.tc[i], m.t1[i]) == tc_t1(coef), key + (i,)
                    n += 1
    print(f"or_splice_parse: {n} pieces equal the decoder's TotalCoeff and TrailingOnes")


def test_designed_blocks_come_back_exactly(corpus):
    n = 0
    for r in good(corpus):
        for y in range(r.pic.H):
            for x in range(r.pic.W):
                want, got = r.pic.mb(x, y), r.ext[y][x]
                assert (want["kind"] == sd.SKIP) == got["skip"]
                if want["kind"] == sd.PCM:
                    assert got["intra"] == 3 and got["pcm"] == want["pcm"]
                if want["kind"] in (sd.SKIP, sd.PCM):
                    continue
                assert got["qp"] == want["qp"] or not (want["cbp"] or want["kind"] == sd.I16)
                pieces = mb_pieces(got)
                for i, coef in pieces.items():
                    w = list(want["coef"].get(i, ()))
                    assert list(coef) == w + [0] * (len(coef) - len(w)), (r.case.name, r.shape, x, y, i)
                    n += 1
    print(f"{n} designed pieces came back exactly")


def test_spliced_mbs_decode_to_the_external_mbs(corpus):
    """every spliced MB of the composed NAL: the external MB's ref, motion,
    cbp, QP and every level (tests/test_splice_oracle.py _check_frame); every
    other MB without residual"""
    n = 0
    for r in good(corpus):
        assert r.CH["nrefs"] == r.nrefs and r.CH["qp"] == 26
        x0, y0 = r.pic.at
        for y in range(r.case.h // 16):
            for x in range(r.case.w // 16):
                g = r.comp[y][x]
                key = (r.case.name, r.shape, r.ti, r.mode, x, y)
                if not (x0 <= x < x0 + r.pic.W and y0 <= y < y0 + r.pic.H):
                    assert g["cbp"] == 0 and not g["intra"], key
                    continue
                e = r.ext[y - y0][x - x0]
                n += 1
                assert (g["ref"], g["mx"], g["my"], g["cbp"]) == (e["ref"], e["mx"], e["my"], e["cbp"]), key
                if e["intra"]:
                    assert (g["intra"], g["mbt"], g["modes"], g["cmode"], g["dc16"], g["pcm"]) == \
                        (e["intra"], e["mbt"], e["modes"], e["cmode"], e["dc16"], e["pcm"]), key
                    if e["intra"] == 2 or e["cbp"]:
                        assert g["qp"] == e["qp"], key
                    assert (g["luma"], g["cdc"], g["cac"]) == (e["luma"], e["cdc"], e["cac"]), key
                    continue
                assert (g["mbt"], g["sub"]) == (min(e["mbt"], 3), e["sub"]) or (e["skip"] and g["mbt"] == 0), key
                assert g["blocks"] == e["blocks"], key
                if e["cbp"]:
                    assert g["qp"] == e["qp"], key
                    assert (g["luma"], g["cdc"], g["cac"]) == (e["luma"], e["cdc"], e["cac"]), key
    print(f"{n} spliced MBs decode to their external MBs")


# ----------------------------------------------------------------- table walk ---
WANT_CT = {16: {(col, tc, t1) for col in (0, 2, 4, 8) for tc, t1 in dz.token_entries(16)},
           15: {(col, tc, t1) for col in (0, 2, 4, 8) for tc, t1 in dz.token_entries(15)},
           4: {(-1, tc, t1) for tc, t1 in hp.CT_TABLES[-1].values()}}


def test_coeff_token_parsed_in_every_class(corpus):
    """every coeff_token entry in every class of the external nC, in each
    slice shape (each parse route reads the shape of its own): 62 per class
    for 16-coefficient blocks, 58 for 15-coefficient ones, 14 chroma DC"""
    assert (len(WANT_CT[16]), len(WANT_CT[15]), len(WANT_CT[4])) == (248, 232, 14)
    for shape in sd.SHAPES:
        seen = {16: set(), 15: set(), 4: set()}
        for r in good(corpus):
            if r.shape == shape:
                for _, nC, maxc, coef, _, _ in r.eblocks:
                    seen[maxc].add((column(nC),) + tc_t1(coef))
        print(f"{shape}: coeff_token parsed {len(seen[16])}/248 of 16, {len(seen[15])}/232 of 15, "
              f"{len(seen[4])}/14 chroma DC")
        for maxc in (16, 15, 4):
            assert seen[maxc] == WANT_CT[maxc], (shape, maxc, sorted(WANT_CT[maxc] - seen[maxc]))


def reachable_pairs():
    """(external class, composed class) of a re-coded block by the nC rule: a
    neighbour block unavailable in the external picture becomes an available
    one of TotalCoeff 0 .. 16 (an MB of the rect above the slice's first row)
    or 0 (an MB outside the rect); an available one stays as it is"""
    def nc(a, b):
        return hp._nc(-1 if a is None else a, -1 if b is None else b)
    out = set()
    rng = list(range(17))
    for a, b in itertools.product([None] + rng, repeat=2):
        for a2 in (rng if a is None else [a]):
            for b2 in (rng if b is None else [b]):
                out.add((column(nc(a, b)), column(nc(a2, b2))))
    return out


# the composed nC is never below half the external one: the external nC is the
# one available neighbour's TotalCoeff n, the composed one at least (n + 0 + 1) >> 1
UNREACHABLE_PAIRS = {(4, 0), (8, 0), (8, 2)}


def test_coeff_token_recoded_for_every_reachable_pair(corpus):
    """k_splice_stage re-codes the tokens of an MB whose left or top neighbour
    is available in the composed picture only: every entry x every reachable
    (external class, composed class), 16- and 15-coefficient blocks; the chroma
    DC token (one class) re-coded too"""
    pairs = reachable_pairs()
    classes = (0, 2, 4, 8)
    assert pairs == {(e, c) for e in classes for c in classes if c >= e or (e, c) in ((2, 0), (4, 2), (8, 4))}
    assert {(e, c) for e in classes for c in classes} - pairs == UNREACHABLE_PAIRS
    seen = {16: set(), 15: set(), 4: set()}
    verbatim = {16: set(), 15: set()}
    corner = {16: set(), 15: set()}
    for r in good(corpus):
        W, (x0, y0) = r.pic.W, r.pic.at
        firsts = set(r.pic.firsts(r.shape)) | {0}
        eb, cb = {}, {}
        for b in r.eblocks:
            eb.setdefault(b[0], []).append(b)
        for b in r.cblocks:
            cb.setdefault(b[0], []).append(b)
        mbw = r.case.w // 16
        for m, blocks in eb.items():
            x, y = m % W, m // W
            top_slice = any(f <= m < f + W and f > m - W for f in firsts) and y > 0    # the MB above: another slice
            new_left = x == 0 and x0 > 0
            new_top = (y == 0 and y0 > 0) or top_slice
            got = cb[(y0 + y) * mbw + x0 + x]
            assert [b[2:4] for b in got] == [b[2:4] for b in blocks]
            for e, c in zip(blocks, got):
                ent = (column(e[1]), column(c[1]), e[2]) + tc_t1(e[3])
                if new_left or new_top:
                    seen[e[2]].add(ent)
                else:
                    assert e[1] == c[1]
                    if e[2] != 4:
                        (corner if (x == 0 or y == 0) else verbatim)[e[2]].add((ent[0],) + ent[3:])
    for maxc in (16, 15):
        want = {(e, c, maxc, tc, t1) for e, c in pairs for tc, t1 in dz.token_entries(maxc)}
        assert not {(e, c) for e, c, *_ in seen[maxc]} & UNREACHABLE_PAIRS
        print(f"re-coded coeff_token, {maxc}-coefficient blocks: {len(seen[maxc] & want)}/{len(want)} "
              f"(entry x pair) over {len(pairs)} reachable pairs; verbatim path {len(verbatim[maxc])}/"
              f"{len(WANT_CT[maxc])}, picture-edge path {len(corner[maxc])}/{len(WANT_CT[maxc])} (entry x class)")
        assert want <= seen[maxc], sorted(want - seen[maxc])[:20]
        assert verbatim[maxc] == WANT_CT[maxc]
        # the MBs on the picture's left column and top row, the rect in its corner: nbsame is
        # set by the picture's edge, not by a neighbour in the rect
        assert corner[maxc] == WANT_CT[maxc], sorted(WANT_CT[maxc] - corner[maxc])
    assert {(e[3], e[4]) for e in seen[4]} == {(tc, t1) for _, tc, t1 in WANT_CT[4]}


def test_total_zeros_and_run_before(corpus):
    for shape in sd.SHAPES:
        tz, rb = {16: set(), 15: set(), 4: set()}, {16: set(), 15: set()}
        for r in good(corpus):
            if r.shape != shape:
                continue
            for _, nC, maxc, coef, _, _ in r.eblocks:
                d = analyse(nC, maxc, coef)
                if d["tz"]:
                    tz[maxc].add(d["tz"])
                if maxc != 4:
                    rb[maxc].update(d["rb"])
        want_tz16 = {(tc, z) for tc, row in hp.TZ.items() for z in row.values()}
        want_tz15 = {(tc, z) for tc, z in want_tz16 if tc + z <= 15 and tc < 15}
        want_tzdc = {(tc, z) for tc, row in hp.TZDC.items() for z in row.values()}
        want_rb = {(zl, run) for zl, row in hp.RB.items() for run in row.values()}
        # a 15-coefficient block codes a run_before only with TotalCoeff >= 2, which
        # leaves at most 13 zeros: run_before 14 needs zerosLeft 14
        unreachable_rb15 = {(7, 14)}
        print(f"{shape}: total_zeros {len(tz[16])}/{len(want_tz16)}, {len(tz[15])}/{len(want_tz15)}, "
              f"{len(tz[4])}/{len(want_tzdc)}; run_before {len(rb[16])}/{len(want_rb)}, "
              f"{len(rb[15])}/{len(want_rb - unreachable_rb15)}")
        assert tz[16] == want_tz16 and tz[15] == want_tz15 and tz[4] == want_tzdc
        assert rb[16] == want_rb and rb[15] == want_rb - unreachable_rb15
        assert (7, 14) in rb[16]


def test_intra_pieces(corpus):
    """the Intra16x16DCLevel piece with TotalCoeff 0, 1, 15 and 16 on every
    route; I_16x16 AC and I_4x4 blocks at TotalCoeff = maxc (with one slice per
    MB row I_4x4 sits in row 0 of a rect on the picture's top edge: no MB above
    in either picture); I slices and IDR pictures from the scripted writer"""
    for shape in sd.SHAPES:
        dc, ac, i4, kinds = set(), set(), set(), set()
        for r in good(corpus):
            if r.shape != shape:
                continue
            kinds.add((r.H["slice_type"], hp.nal_units(r.nal)[0][0] & 31))
            if r.H["slice_type"] == 7:               # every MB intra; se() only as slice_qp_delta and mb_qp_delta
                assert all(d["intra"] for row in r.ext for d in row) and len(r.ese) == \
                    1 + len(r.pic.firsts(shape)) + sum(d["intra"] == 2 or (d["intra"] == 1 and d["cbp"] > 0) for row in r.ext for d in row)
            for row in r.ext:
                for d in row:
                    if d["intra"] == 2:
                        dc.add(tc_t1(d["dc16"])[0])
                        ac.update(tc_t1(b[1:])[0] for b in d["luma"])
                    if d["intra"] == 1:
                        i4.update(tc_t1(b)[0] for b in d["luma"])
        print(f"{shape}: Intra16x16DCLevel TotalCoeff {sorted(dc)}, largest AC {max(ac)}, largest I_4x4 {max(i4, default=None)}")
        assert {0, 1, 15, 16} <= dc and 15 in ac and 16 in i4
        assert kinds == {(0, 1), (7, 1), (7, 5)}, kinds      # P, I and IDR slices


# --------------------------------------------------------------------- levels ---
def test_levels(corpus):
    """every reachable (suffixLength, adjustment, level_prefix) for |level|
    1 .. 2063 on every route; |level| 8 .. 15 first with and without the
    adjustment and 16 with it (level_prefix 14 at suffixLength 0); each
    threshold of the suffixLength chain met and passed by one; TotalCoeff 11
    with 2 and 3 trailing ones"""
    want = reachable_triples(2063)
    for shape in sd.SHAPES:
        seen, esc14, chain, start, top = set(), set(), set(), set(), 0
        for r in good(corpus):
            if r.shape != shape:
                continue
            for _, nC, maxc, coef, _, _ in r.eblocks:
                d = analyse(nC, maxc, coef)
                tr = d["triples"]
                for i, (sl, adj, prefix, v) in enumerate(tr):
                    seen.add((sl, adj, prefix))
                    top = max(top, abs(v))
                    if sl == 0 and prefix == 14:
                        esc14.add((abs(v), adj))
                    if i + 1 < len(tr) and sl >= 1:
                        chain.add((sl, abs(v), tr[i + 1][0]))
                if d["tc"] == 11 and tr:
                    start.add((d["t1"], tr[0][0]))
        print(f"{shape}: level triples {len(seen & want)}/{len(want)}, largest |level| {top}, "
              f"level_prefix 14 at suffixLength 0: {sorted(esc14)}")
        assert want <= seen, sorted(want - seen)
        assert top == 2063
        assert {(v, False) for v in range(8, 16)} | {(v, True) for v in range(9, 17)} <= esc14
        for sl, thr in enumerate(sd.THRESHOLDS, 1):
            assert (sl, thr, sl) in chain and (sl, thr + 1, sl + 1) in chain, (shape, sl)
        assert {(2, 1), (3, 0)} <= start              # suffixLength starts at 1 only with fewer than 3 trailing ones


def test_level_prefix_16_is_refused(corpus):
    """a level_prefix 16 code, in each slice shape: the decoder finds 16 zeros
    before the one where the picture's one escape stood, the slice is still
    whole, and the oracle's parse and compose refuse it (checked where the
    corpus is built) with nothing committed"""
    t = Tally()
    recs = [r for r in corpus if r.case.name == "l_prefix16"]
    assert [r.shape for r in recs] == list(sd.SHAPES)
    for r in recs:
        assert r.status == sd.ERR_SYNTAX and r.ext is None
        _, mbs, blocks, _ = t.decode(r.nal, 16 * r.pic.W, 16 * r.pic.H, "spec")      # consumed to the stop bit
        (m, nC, maxc, coef, p0, n), = [b for b in blocks if any(b[3])]
        k, at = r.pic.patched[r.shape]
        # the 6-bit coeff_token of (1, 0) at nC 0, the 30-bit level, total_zeros "1"
        assert (m, nC, maxc, n) == (9, 0, 16, 6 + 30 + 1) and at == p0 + 6
        rb = hp.ebsp_to_rbsp(hp.nal_units(r.nal)[k][1:])
        bits = "".join(format(x, "08b") for x in rb)
        assert bits[at:at + 17] == "0" * 16 + "1"


# --------------------------------------------------------- lengths and phases ---
def test_longest_body_and_mb(corpus, oracle):
    """the longest body the syntax allows under level_prefix <= 15 (the bits
    after coeff_token): sixteen 28-bit escapes, 448 bits, found with
    or_cavlc_block over the block families that could pass it; the corpus
    holds it, and whole MBs of such blocks fit the record's fields"""
    best = 0
    B = sd.BIG
    for maxc in (16, 15):
        for tc in range(1, maxc + 1):
            # tc escapes, the last coefficient behind the longest total_zeros / run_before codes
            for pos in (list(range(tc)), list(range(tc - 1)) + [maxc - 1], [0] + list(range(maxc - tc + 1, maxc))):
                if len(set(pos)) != tc:
                    continue
                for first in (B, 1):
                    coef = dz.place([first] + [B] * (tc - 1), pos, maxc)
                    n = dz.coded_bits(oracle, coef, maxc, 0)
                    assert n == codes(0, maxc, coef)[1]
                    best = max(best, n - codes(0, maxc, coef)[0][0][2])
    assert best == 16 * 28 == 448
    longest, mb_body, piece = 0, 0, 0
    for r in good(corpus):
        per_mb = {}
        for m, nC, maxc, coef, p0, n in r.eblocks:
            cs, total = codes(nC, maxc, coef)
            assert total == n                       # the rule's lengths are what the parser read
            body = n - cs[0][2]
            longest = max(longest, body)
            per_mb[m] = per_mb.get(m, 0) + body
            piece = max(piece, body)
        mb_body = max([mb_body] + list(per_mb.values()))
    print(f"longest body {longest} bits; largest MB body sum {mb_body} bits (16-bit field), "
          f"largest piece {piece} bits (11-bit field)")
    assert longest == 448 and piece < 1 << 11
    assert 16 * 448 + 2 * 112 + 8 * 420 + 448 - 16 * 28 <= mb_body < 1 << 16


def test_bit_phases(corpus):
    """28-bit escapes, 16-bit coeff_tokens, 9-bit total_zeros and 11-bit
    run_before codes start at every bit position modulo 32 of the external
    RBSP, on every route (a reader refill one bit late has a place to show)"""
    for shape in sd.SHAPES:
        ph = {("lv", 28): set(), ("ct", 16): set(), ("tz", 9): set(), ("rb", 11): set()}
        for r in good(corpus):
            if r.shape != shape:
                continue
            for _, nC, maxc, coef, p0, _ in r.eblocks:
                for kind, off, n in codes(nC, maxc, coef)[0]:
                    if (kind, n) in ph:
                        ph[(kind, n)].add((p0 + off) % 32)
        print(f"{shape}: phases", {f"{k[1]}-bit {k[0]}": len(v) for k, v in ph.items()})
        for k, v in ph.items():
            assert v == set(range(32)), (shape, k, sorted(set(range(32)) - v))


# --------------------------------------------------------------------- motion ---
def test_motion_limits(corpus):
    """mvd +-32766 as a 31-bit code in the external slices and in the composed
    NALs of each mode; motion at +-16383 in P_L0_16x16, 16x8, 8x16, P_8x8 and
    P_8x8ref0 and through a P_Skip; |mv| 16384 refused; ref_idx as one bit and
    as ue; a slice that is one mb_skip_run, a slice that ends in one"""
    E = sd.MAX_MV
    ext_mvd, comp_mvd, kinds, skip_at_bound, refbits = set(), {}, set(), 0, set()
    for r in good(corpus, "m"):
        ext_mvd.update(v for v, n, _ in r.ese if n == 31)
        comp_mvd.setdefault(r.mode, set()).update(v for v, n, _ in r.cse if n == 31)
        refbits.add(r.H["nrefs"])
        for row in r.ext:
            for d in row:
                if any(abs(b[1]) == E or abs(b[2]) == E for b in d["blocks"]):
                    kinds.add("skip" if d["skip"] else d["mbt"])
                    skip_at_bound += d["skip"]
        for row in r.comp:
            assert all(abs(b[1]) <= E and abs(b[2]) <= E for d in row for b in d["blocks"])
    print(f"31-bit mvd: external {sorted(ext_mvd)}, composed {({k: sorted(v) for k, v in comp_mvd.items()})}; "
          f"MB kinds at +-16383: {sorted(map(str, kinds))}; references {sorted(refbits)}")
    assert {32766, -32766} <= ext_mvd
    for mode in (EXACT, PSKIP, SPEC):
        assert {32766, -32766} <= comp_mvd[mode], mode
    assert kinds == {0, 1, 2, 3, 4, "skip"}
    assert refbits == {2} | set(range(3, 3 + sd.WAYPOINTS)), refbits
    for r in good(corpus, "m"):
        if r.case.name == "m_refs":
            assert r.nrefs == 3 and {b[0] for row in r.comp for d in row for b in d["blocks"]} >= {0, 1, 2}
    # a scroll over every waypoint: each frame's list is 2 + its waypoints long, the last one
    # 2 + all eight, and the largest index occurs in each partition shape, external and composed
    allwp = [r for r in good(corpus, "m") if r.case.name == "m_refs_all"]
    assert len(allwp) == 3 * len(sd.ALL_WP_OFFS)
    for r in allwp:
        n = min(3 + r.ti, 2 + sd.WAYPOINTS)
        assert r.nrefs == r.CH["nrefs"] == r.H["nrefs"] == n, (r.shape, r.ti)
        x0, y0 = r.pic.at
        spliced = [r.comp[y0 + y][x0 + x] for y in range(r.pic.H) for x in range(r.pic.W)]
        for mbs in ([d for row in r.ext for d in row], spliced):
            top = {d["mbt"] for d in mbs if any(b[0] == n - 1 for b in d["blocks"])}
            assert top == {0, 1, 2, 3}, (r.shape, r.ti, top)
    assert {r.nrefs for r in allwp if r.ti == len(sd.ALL_WP_OFFS) - 1} == {2 + sd.WAYPOINTS} == {10}
    refused = [r for r in corpus if r.case.name == "m_refused"]
    assert len(refused) == 3 and all(r.status == sd.ERR_SYNTAX for r in refused)
    # the mb_skip_run picture, slice by slice: a slice that is one run where a slice is at most
    # two MB rows (rows 0-1 are all skipped; one slice per picture has coded MBs), and in every
    # shape a slice with coded MBs that ends in a run
    runs = [r for r in good(corpus, "m") if r.case.name == "m_motion" and r.ti == 1]
    assert [r.shape for r in runs] == list(sd.SHAPES)
    for r in runs:
        flat = [d["skip"] for row in r.ext for d in row]
        firsts = [0] + r.pic.firsts(r.shape) + [len(flat)]
        slices = [flat[a:b] for a, b in zip(firsts, firsts[1:])]
        assert any(all(sl) for sl in slices) == (r.shape != "one"), r.shape
        assert any(not all(sl) and sl[-1] for sl in slices), r.shape


# ------------------------------------------------------------------- QP chain ---
def test_qp_chain(corpus):
    """MB QPs 0 -> 51 -> 0 -> 26 -> 51 in one slice, slice QPs 0 and 51, a
    slice that ends at QP 51 before one that starts at 0 and the reverse, the
    first spliced MB of a NAL at QP 0 and at 51; the composed NAL keeps every QP
    (test_spliced_mbs_decode_to_the_external_mbs)"""
    for shape in sd.SHAPES:
        chain, slice_qp, edges, first, deltas = False, set(), set(), set(), set()
        for r in good(corpus, "q"):
            if r.shape != shape:
                continue
            slice_qp.add(r.H["qp"])
            firsts = [0] + r.pic.firsts(shape) + [r.pic.W * r.pic.H]
            flat = [d for row in r.ext for d in row]
            prev_last = None
            for a, b in zip(firsts, firsts[1:]):
                qps = [d["qp"] for d in flat[a:b] if d["cbp"] or d["intra"] == 2]
                s = ",".join(map(str, qps))
                chain = chain or ",".join(map(str, sd.QP_CHAIN)) in s
                if prev_last is not None:
                    edges.add((prev_last, qps[0]))
                prev_last = qps[-1]
            # mb_qp_delta as written: the last se() before an MB's first block
            first_block = {}
            for i, blk in enumerate(r.eblocks):
                first_block.setdefault(blk[0], i)
            for a, b in zip(firsts, firsts[1:]):
                prev = r.H["qp"]
                for m in range(a, b):
                    if m not in first_block:
                        continue
                    d = [v for v, _, nb in r.ese if nb == first_block[m]][-1]
                    assert -26 <= d <= 25 and (prev + d) % 52 == flat[m]["qp"], (shape, r.ti, m, d)
                    deltas.add((prev, flat[m]["qp"], d))
                    prev = flat[m]["qp"]
            x0, y0 = r.pic.at
            g = r.comp[y0][x0]
            assert g["qp"] == flat[0]["qp"]
            first.add(g["qp"])
        print(f"{shape}: slice QPs {sorted(slice_qp)}, slice edges (last, first) {sorted(edges)}, first MB {sorted(first)}, "
              f"mb_qp_delta {min(d for _, _, d in deltas)} .. {max(d for _, _, d in deltas)}")
        assert chain and {0, 51} <= slice_qp and {0, 51} <= first
        # the wrap: 0 -> 51 is written as -1, 51 -> 0 as +1; the range's ends -26 and +25 occur
        assert {(0, 51, -1), (51, 0, 1), (26, 0, -26), (26, 51, 25)} <= deltas
        if shape == "rows":
            assert {(51, 0), (0, 51)} <= edges


# ------------------------------------------------------ emulation prevention ---
def ep_positions(nal):
    return [i for i in range(2, len(nal)) if nal[i] == 3 and nal[i - 1] == 0 and nal[i - 2] == 0
            and i + 1 < len(nal) and nal[i + 1] <= 3 and i > 5]


def test_emulation_prevention_positions(corpus):
    """the external NALs of the EP case carry emulation prevention bytes whose
    03 falls at every byte position modulo 16 of the buffer handed over, in
    each picture alone, with its start code and (the one-slice pictures, as
    the GPU test hands one over) without; the composed NALs carry their own"""
    for shape in sd.SHAPES:
        n, comp = 0, 0
        for r in good(corpus, "e"):
            if r.shape == shape:
                ep = ep_positions(r.nal)
                n += len(ep)
                comp += len(ep_positions(r.comp_nal))
                # per picture: as handed over with its start code, and (a one-slice picture
                # only) without it, four bytes earlier
                with_sc = {i % 16 for i in ep}
                assert with_sc == set(range(16)), (shape, r.ti, sorted(with_sc))
                if shape == "one":
                    assert r.nal[:4] == b"\x00\x00\x00\x01"
                    without = {i % 16 for i in ep_positions(r.nal[4:])}
                    assert without == set(range(16)) and len(ep_positions(r.nal[4:])) == len(ep), (r.ti, sorted(without))
        print(f"{shape}: {n} EP bytes in the external NALs, every picture at 16/16 positions, {comp} in the composed NALs")
        assert n > 1000 and comp > 1000
