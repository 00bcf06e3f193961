"""The rule of scroll_batch_detect_offsets, restated in numpy from its
definition (include/composer_batch.h) -- not from
csrc/detect_device.h, which the tests check against this.

  segments   64 columns, nseg = ceil(pw / 64), the used ones 0, step, 2 step ...
  sigS       cschelp.luma_np of the surface pixels, summed per segment and row
  sigR       the stacked reference rows (A's, then B's), summed the same way
  window     c0 = clamp(estimate, 0, ph), lo / hi = c0 -/+ radius clipped to 0..ph
  score(o)   the number of (row, used segment) pairs with sigS[Y] == sigR[Y + o]
  choice     max under (score, -|o - c0|, -o); second: the same over the others
  status     LOW / FOUND / TIED

For tests/test_detect_hostsim.py and tests/test_gpu_detect.py; device memory
and surfaces through damagehelp's Hip / Surfaces / grey_surface / paint."""
import numpy as np

from cschelp import BT601, RGBA, luma_np, rgb_of
from damagehelp import grey_surface, paint

LOW, FOUND, TIED = 0, 1, 2
SEG = 64
NO_SCORE = 0xFFFFFFFF
DETECT_DTYPE = np.dtype([("off", np.int32), ("centre", np.int32), ("score", np.uint32), ("second", np.uint32),
                         ("second_off", np.int32), ("n_sig", np.uint32), ("lo", np.uint16), ("hi", np.uint16),
                         ("status", np.uint16), ("reserved", np.uint16)])
assert DETECT_DTYPE.itemsize == 32


def used_segments(pw, seg_step=1):
    return list(range(0, -(-pw // SEG), seg_step))


def sig_rows(y, seg_step=1):
    """[rows][pw] luma -> [rows][nuse] sums over the used segments"""
    y = np.asarray(y).astype(np.int64)
    pw = y.shape[1]
    return np.stack([y[:, SEG * c:min(SEG * c + SEG, pw)].sum(axis=1) for c in used_segments(pw, seg_step)], axis=1)


def sig_surface(img, v, seg_step=1):
    """[ph][pw][4] u8 surface under the variant v = (format, matrix, full_range)"""
    fmt, matrix, full = v
    return sig_rows(luma_np(*rgb_of(img, fmt), matrix, full), seg_step)


def stacked(ya, yb):
    """[2 ph][pw]: reference picture A's luma rows, then B's"""
    return np.concatenate([np.asarray(ya), np.asarray(yb)], axis=0)


def detect_np(sig_s, sig_r, estimate, radius, min_match=1):
    """one frame: (record as a dict of DETECT_DTYPE's fields, scores [ph + 1] uint32)"""
    ph = sig_s.shape[0]
    assert sig_r.shape == (2 * ph, sig_s.shape[1])
    c0 = min(max(int(estimate), 0), ph)
    lo, hi = max(c0 - radius, 0), min(c0 + radius, ph)
    scores = np.full(ph + 1, NO_SCORE, np.uint32)
    for o in range(lo, hi + 1):
        scores[o] = int((sig_s == sig_r[o:o + ph]).sum())
    order = lambda o: (int(scores[o]), -abs(o - c0), -o)
    cands = list(range(lo, hi + 1))
    off = max(cands, key=order)
    rest = [o for o in cands if o != off]
    second_off = max(rest, key=order) if rest else -1
    score, second = int(scores[off]), int(scores[second_off]) if rest else 0
    status = LOW if score < min_match else TIED if rest and score == second else FOUND
    return dict(off=off, centre=c0, score=score, second=second, second_off=second_off, n_sig=ph * sig_s.shape[1],
                lo=lo, hi=hi, status=status, reserved=0), scores


def record_tuple(r):
    """a dict of detect_np or a numpy record -> a plain tuple in DETECT_DTYPE's order"""
    return tuple(int(r[n]) for n in DETECT_DTYPE.names)


# ------------------------------------------------------------- the pictures
def noise_luma(pw, ph, rng):
    """(A, B): random luma, every row of the stack distinct"""
    return rng.integers(0, 256, (ph, pw), dtype=np.uint8), rng.integers(0, 256, (ph, pw), dtype=np.uint8)


def tiled_luma(pw, ph, rng):
    """(A, B): flat 48 x 32 tiles, each of its own grey level, on a 64 x 48
    grid over one background level: most rows agree with many others in some
    segment, so the scores curve is not trivial"""
    st = np.full((2 * ph, pw), 90, np.uint8)
    for y in range(0, 2 * ph, 48):
        for x in range(0, pw, 64):
            st[y:y + 32, x:x + 48] = rng.integers(0, 256)
    return st[:ph].copy(), st[ph:].copy()


def flat_luma(pw, ph, va=77, vb=77):
    return np.full((ph, pw), va, np.uint8), np.full((ph, pw), vb, np.uint8)


def i420(y):
    """the I420 picture with luma y and grey chroma, as set_dyn_refs takes it"""
    return np.concatenate([np.asarray(y, np.uint8).reshape(-1), np.full(y.size // 2, 128, np.uint8)]).tobytes()


def quarter(pw, ph):
    """the MBs of a quarter of the picture (half its width, half its height), from its middle down and right"""
    mbw, mbh = pw // 16, ph // 16
    return [(x, y) for y in range(mbh // 2, mbh) for x in range(mbw // 2, mbw)]


def painted(name, pw, ph):
    """the damage test's patterns, as lists of MBs"""
    mbw, mbh = pw // 16, ph // 16
    return {"none": [], "2x2": [(mbw - 2, mbh - 2), (mbw - 1, mbh - 2), (mbw - 2, mbh - 1), (mbw - 1, mbh - 1)],
            "corners": [(0, 0), (mbw - 1, 0), (0, mbh - 1), (mbw - 1, mbh - 1)], "quarter": quarter(pw, ph)}[name]


# ------------------------------------------------------- the designed cases
# Shared by the CPU test, which asserts that the helper alone finds the truth
# in each of them, and the GPU test, which compares the device with the helper.
GREY = (RGBA, BT601, 1)             # the variant under which a grey surface's luma is its grey level
EDGE_W, EDGE_H, EDGE_S, EDGE_F = 96, 368, 3, 6
EDGE_OFFS = [0, 1, 15, 16, 17, 184, 351, 367, 368]
EDGE_PATTERNS = ["none", "2x2", "corners", "quarter"]
EDGE_RADII = [0, 8, 400]


def scroll_surface(stack, off, ph, rng, mbs=()):
    """the grey full-range surface that shows the stack at offset off, the listed MBs painted over"""
    return paint(grey_surface(stack[off:off + ph], RGBA, rng), mbs, rng)


def edge_case(shared):
    """96x368: two segments, the second 32 wide; 369 candidates.  3 streams x
    6 frames over EDGE_OFFS (each twice) and EDGE_PATTERNS; references per
    stream (noise, tiled, noise) or one shared noise pair.
    -> (lumas [(A, B)] per stream or one, img [S][F][ph][pw][4], truth [S][F])"""
    rng = np.random.default_rng(61 + int(shared))
    pw, ph = EDGE_W, EDGE_H
    lumas = [noise_luma(pw, ph, rng)] if shared else [noise_luma(pw, ph, rng), tiled_luma(pw, ph, rng),
                                                      noise_luma(pw, ph, rng)]
    truth = np.array(EDGE_OFFS * 2, np.int32).reshape(EDGE_S, EDGE_F)
    img = np.empty((EDGE_S, EDGE_F, ph, pw, 4), np.uint8)
    for s in range(EDGE_S):
        st = stacked(*lumas[0 if shared else s])
        for f in range(EDGE_F):
            name = EDGE_PATTERNS[(s * EDGE_F + f) % len(EDGE_PATTERNS)]
            img[s, f] = scroll_surface(st, int(truth[s, f]), ph, rng, painted(name, pw, ph))
    return lumas, img, truth


def estimates(truth, radius):
    """the caller's estimates for a search of `radius`: off the truth by 0, +5,
    -5, +radius, -radius in turn (by 0 throughout for radius 0; never by more
    than the radius), not clamped: the window does that"""
    deltas = [0, 5, -5, radius, -radius]
    t = np.asarray(truth)
    d = np.array([deltas[i % 5] for i in range(t.size)], np.int32).reshape(t.shape)
    return (t + np.clip(d, -radius, radius)).astype(np.int32)


def width_case(pw, ph):
    """272x48 (four segments and one 16 wide) and 320x240 (five): 2 streams x
    2 frames on one noise pair, a 2x2 painted"""
    rng = np.random.default_rng(63 + pw)
    lumas = [noise_luma(pw, ph, rng)]
    truth = np.array([[3, ph], [ph // 2 + 1, 0]], np.int32)
    st = stacked(*lumas[0])
    img = np.stack([np.stack([scroll_surface(st, int(truth[s, f]), ph, rng, painted("2x2", pw, ph))
                              for f in range(2)]) for s in range(2)])
    return lumas, img, truth


def expect(lumas, img, est, v=GREY, radius=8, seg_step=1, min_match=1):
    """the helper's (records [S][F] of dicts, scores [S][F][ph + 1]); lumas one pair (shared) or one per stream"""
    ns, nf = est.shape
    recs, scores = [], []
    for s in range(ns):
        sr = sig_rows(stacked(*lumas[s if len(lumas) > 1 else 0]), seg_step)
        out = [detect_np(sig_surface(img[s if img.shape[0] > 1 else 0, f], v, seg_step), sr, int(est[s, f]), radius,
                         min_match) for f in range(nf)]
        recs.append([o[0] for o in out])
        scores.append(np.stack([o[1] for o in out]))
    return recs, np.stack(scores)
