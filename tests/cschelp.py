"""The surface entry's conversion rule, restated in numpy from the table of its
definition (include/composer_batch.h) -- not from
csrc/csc_device.h, which the tests check against this.

    Y = (yr R + yg G + yb B + yoff) >> 16                               per pixel
    C = clamp((cr Sr + cg Sg + cb Sb + (128 << 18) + (1 << 17)) >> 18, 0, 255)
per 2x2 quad, Sr Sg Sb the quad's channel sums; alpha ignored."""
import numpy as np

RGBA, BGRA = 0, 1
BT601, BT709 = 0, 1

# (matrix, full_range) -> (yr, yg, yb, yoff), (Cb r, g, b), (Cr r, g, b); Q16
TABLE = {
    (BT601, 0): ((16829, 33039, 6416, 1081344), (-9714, -19070, 28784), (28784, -24103, -4681)),
    (BT601, 1): ((19595, 38470, 7471, 32768), (-11058, -21710, 32768), (32768, -27439, -5329)),
    (BT709, 0): ((11966, 40254, 4064, 1081344), (-6596, -22188, 28784), (28784, -26145, -2639)),
    (BT709, 1): ((13933, 46871, 4732, 32768), (-7509, -25259, 32768), (32768, -29763, -3005)),
}
VARIANTS = [(fmt, m, fr) for fmt in (RGBA, BGRA) for m in (BT601, BT709) for fr in (0, 1)]

# the real-valued matrices the table rounds: Kr, Kb
KRKB = {BT601: (0.299, 0.114), BT709: (0.2126, 0.0722)}


def rgb_of(px, fmt):
    """[..., 4] u8 pixels in memory order -> R, G, B as int64"""
    p = np.asarray(px).astype(np.int64)
    return (p[..., 2], p[..., 1], p[..., 0]) if fmt == BGRA else (p[..., 0], p[..., 1], p[..., 2])


def luma_np(r, g, b, matrix, full):
    yr, yg, yb, yoff = TABLE[(matrix, int(full))][0]
    return (yr * r + yg * g + yb * b + yoff) >> 16


def chroma_np(sr, sg, sb, matrix, full):
    """quad sums -> (Cb, Cr)"""
    out = []
    for cr, cg, cb in TABLE[(matrix, int(full))][1:]:
        out.append(np.clip((cr * sr + cg * sg + cb * sb + (128 << 18) + (1 << 17)) >> 18, 0, 255))
    return out


def convert(img, fmt, matrix, full):
    """[h][w][4] u8 (h, w even) -> (Y [h][w], Cb, Cr [h/2][w/2]) u8"""
    r, g, b = rgb_of(img, fmt)
    y = luma_np(r, g, b, matrix, full)
    h, w = y.shape
    q = lambda c: c.reshape(h // 2, 2, w // 2, 2).sum(axis=(1, 3))
    cb, cr = chroma_np(q(r), q(g), q(b), matrix, full)
    return y.astype(np.uint8), cb.astype(np.uint8), cr.astype(np.uint8)


def i420_bytes(img, fmt, matrix, full):
    """the I420 block of the window: luma, then Cb, then Cr"""
    return b"".join(p.tobytes() for p in convert(img, fmt, matrix, full))


def real_luma(r, g, b, matrix, full):
    kr, kb = KRKB[matrix]
    y = kr * r + (1.0 - kr - kb) * g + kb * b
    return y if full else 16.0 + y * 219.0 / 255.0


def real_chroma(r, g, b, matrix, full):
    """mean channel values (floats) -> (Cb, Cr), unclamped (at most 255.5: full-range pure blue or red)"""
    kr, kb = KRKB[matrix]
    y = kr * r + (1.0 - kr - kb) * g + kb * b
    s = 1.0 if full else 224.0 / 255.0
    cb = 128.0 + s * (b - y) / (2.0 * (1.0 - kb))
    cr = 128.0 + s * (r - y) / (2.0 * (1.0 - kr))
    return cb, cr
