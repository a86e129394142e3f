"""YCbCr VarDCT frames: the streams of tests/test_ycbcr.py and tests/test_ycbcr_gpu.py and a numpy restatement of the tail kernel
(device/ycbcr_dev.h), float32 throughout and in the order the kernel computes (TEST INFRASTRUCTURE)."""
import numpy as np

from streams import synth

U8X4, U16X4 = 0x0F33, 0x0F35
F = np.float32
SEED = 5

# (hshift, vshift) of Cb, Y, Cr for every layout jpeg_upsampling can give here
SHIFTS = {"444": ((0, 0), (0, 0), (0, 0)), "420": ((1, 1), (0, 0), (1, 1)), "422": ((1, 0), (0, 0), (1, 0)), "440": ((0, 1), (0, 0), (0, 1))}


def ycbcr_stream(w, h, sub="444", **opts):
    if sub != "444":
        opts = dict(opts, subsampling=sub)
    return synth("vardct", w, h, SEED, ycbcr=1, **opts)


def twin_stream(w, h, **opts):
    """the same options with noxyb=1 and do_ycbcr = 0"""
    return synth("vardct", w, h, SEED, noxyb=1, fullheader=1, **opts)


def plane_shapes(w, h, sub):
    """(rows, columns) of the planes Cb, Y, Cr: the frame's size, or the block grid padded to whole MCUs at each channel's resolution"""
    sh = SHIFTS[sub]
    if sub == "444":
        return [(h, w)] * 3
    mh, mv = max(s[0] for s in sh), max(s[1] for s in sh)
    fw = -(-w // (8 << mh)) << (mh + 3)
    fh = -(-h // (8 << mv)) << (mv + 3)
    return [(fh >> s[1], fw >> s[0]) for s in sh]


def _up(a, axis):
    """by 2 along `axis`: out[2i] = 0.75 a[i] + 0.25 a[i-1], out[2i+1] = 0.75 a[i] + 0.25 a[i+1], the plane's border repeated"""
    a = np.moveaxis(np.asarray(a, F), axis, -1)
    before = np.concatenate([a[..., :1], a[..., :-1]], -1)
    after = np.concatenate([a[..., 1:], a[..., -1:]], -1)
    out = np.empty(a.shape[:-1] + (2 * a.shape[-1],), F)
    out[..., 0::2] = F(0.75) * a + F(0.25) * before
    out[..., 1::2] = F(0.75) * a + F(0.25) * after
    return np.moveaxis(out, -1, axis)


def upsampled(plane, hshift, vshift, w, h):
    """plane at the picture's resolution, cut to w x h: horizontal first, then vertical on the horizontally upsampled values"""
    a = np.asarray(plane, F)
    if hshift:
        a = _up(a, 1)
    if vshift:
        a = _up(a, 0)
    return a[:h, :w]


def restatement(planes, shifts, w, h, bpp, fmt):
    """(pixels [h, w, 4], sure [h, w, 3]): what k_ycbcr_tail makes of the planes Cb, Y, Cr, and where the scaled value is farther than
    1e-3 from a rounding boundary, so that the level cannot depend on how a tie falls"""
    cb, y, cr = (upsampled(p, s[0], s[1], w, h) for p, s in zip(planes, shifts))
    k = F(128.0) / F(255.0)
    r = y + F(1.402) * cr + k
    g = y - F(0.344136286) * cb - F(0.714136286) * cr + k
    b = y + F(1.772) * cb + k
    maxv = F(255.0 if fmt == U8X4 else (1 << bpp) - 1)
    out = np.zeros((h, w, 4), np.uint16 if fmt == U16X4 else np.uint8)
    sure = np.zeros((h, w, 3), bool)
    for i, v in enumerate((r, g, b)):
        s = v * maxv + F(0.5)
        level = np.clip(np.floor(s), 0, maxv).astype(np.int64)
        frac = s.astype(np.float64) - np.floor(s.astype(np.float64))
        sure[..., i] = np.minimum(frac, 1.0 - frac) > 1e-3
        if fmt == U16X4:
            maxpixel = (1 << bpp) - 1
            level = (level * 65535 + (1 << (bpp - 1))) // maxpixel
        out[..., i] = level
    out[..., 3] = 65535 if fmt == U16X4 else 255
    return out, sure


def levels(px, bpp, fmt):
    """the samples back on their level scale (u16: p = (u16 * maxpixel + 32767) / 65535, INTEGRATION.md's 16-bit rule)"""
    px = np.asarray(px, np.int64)
    return px if fmt == U8X4 else (px * ((1 << bpp) - 1) + 32767) // 65535


def check_against_restatement(got, planes, shifts, w, h, bpp, fmt, exact):
    """within +-1 level everywhere; exact: equal wherever the restatement is sure (the inputs are the same floats on both sides)"""
    want, sure = restatement(planes, shifts, w, h, bpp, fmt)
    assert got.shape == want.shape and got.dtype == want.dtype
    assert (got[..., 3] == want[..., 3]).all(), "A is opaque"
    d = np.abs(levels(got[..., :3], bpp, fmt) - levels(want[..., :3], bpp, fmt))
    print("max |delta| = %d level(s), %d of %d samples differ, %d of them where a tie decides" % (d.max(), int((d > 0).sum()), d.size, int(((d > 0) & ~sure).sum())))
    assert d.max() <= 1
    if exact:
        assert np.array_equal(got[..., :3][sure], want[..., :3][sure]), "a difference may only come from a tie"
    return d


FWD = dict(forward=1, hfmul=5, dct8only=1, nocfl=1, nosmooth=1)   # what a subsampled stream has anyway, for its 4:4:4 twins


def code4(c):
    c &= 0xffffffff
    return "".join(chr((c >> s) & 0xff) for s in (24, 16, 8, 0)) if c else ""


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def tail_cases():
    """the tail kernel's known-answer cases: (width, height, layout, format, bpp)"""
    for w, h in ((1, 1), (7, 5), (33, 17), (264, 9)):
        for sub in ("444", "420", "422", "440"):
            for fmt in (U8X4, U16X4):
                for bpp in (8, 12):
                    yield w, h, sub, fmt, bpp


def random_planes(rng, w, h, sub):
    """chroma in [-0.6, 0.6], Y in [-0.1, 1.1], the planes as large as the padded-grid rule makes them"""
    return [rng.uniform(-0.1, 1.1, s).astype(np.float32) if c == 1 else rng.uniform(-0.6, 0.6, s).astype(np.float32) for c, s in enumerate(plane_shapes(w, h, sub))]
