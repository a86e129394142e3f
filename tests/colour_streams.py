"""helpers shared by tests/test_colour.py and tests/test_colour_gpu.py (TEST INFRASTRUCTURE): the streams with a signalled colour encoding,
the CPU build of the colour tail (tests/hostsim/colour_sim.cpp) and the float64 model of the colour mode written out in numpy -- the
standards' formulas as include/j40hip.h states them, nothing of the library's own."""
import ctypes as C
import os

import numpy as np

from streams import synth, ROOT

SEED = 11
U8X4, U16X4 = 0x0F33, 0x0F35   # (j40_amd.J40_U8X4 / J40_U16X4)

# name -> (the cenc= options of the stream writer, intensity_target or None for the default 255, tone= option)
CURVES = {
    "linear": (dict(tf=8), None),
    "srgb_p3": (dict(tf=13, primaries=11), None),
    "bt709": (dict(tf=1), None),
    "dci": (dict(tf=17, white=11, primaries=11), None),
    "gamma": (dict(gamma=4545455), None),
    "pq": (dict(tf=16, primaries=9), 4000),
    "hlg": (dict(tf=18, primaries=9), 1000),
}


def stream(mode, w, h, curve, **more):
    """a VarDCT (two passes: the writer's smallest) or Modular XYB stream with the curve's encoding; curve None: the same stream without cenc="""
    opts = dict(more)
    if mode == "vardct":
        opts.setdefault("passes", 2)
    else:
        opts.setdefault("xyb", 1)
    it = None
    if curve is not None:
        cenc, it = CURVES[curve]
        opts.update(cenc)
    if it is not None:
        opts["tone"] = "%d,0.5" % it
    return synth(mode, w, h, SEED, **opts)


def enc_words(white=1, primaries=1, tf=13, gamma=0, whitexy=None, primxy=None):
    """the 16 words of j40hip_frame_colour_encoding for an RGB encoding"""
    wxy = {1: (312700, 329000), 10: (333333, 333333), 11: (314000, 351000)}.get(white, whitexy)
    pxy = {1: (640000, 330000, 300000, 600000, 150000, 60000), 9: (708000, 292000, 170000, 797000, 131000, 46000),
           11: (680000, 320000, 265000, 690000, 150000, 60000)}.get(primaries, primxy)
    return np.array([0, white, wxy[0], wxy[1], primaries] + list(pxy) + [1 if gamma else 0, gamma, tf, 1, 0], np.int32)


class ColourSim:
    def __init__(self):
        self.L = C.CDLL(os.path.join(ROOT, "build", "libhostsim_colour.so"))
        vp, i32, i64, sz = C.c_void_p, C.c_int32, C.c_int64, C.c_size_t
        self.L.colour_sim_tail.restype = i32
        self.L.colour_sim_tail.argtypes = [vp, i32, i32, vp, vp, vp, i32, i32, i32, vp, sz]
        self.L.colour_sim_levels.restype = None
        self.L.colour_sim_levels.argtypes = [vp, C.c_float, vp, i64, i32, vp]
        self.L.colour_sim_hlg_ootf.restype = None
        self.L.colour_sim_hlg_ootf.argtypes = [vp, C.c_float, vp, vp, i64]
        self.L.colour_sim_pow.restype = None
        self.L.colour_sim_pow.argtypes = [vp, vp, i64, vp]
        self.L.colour_sim_table_check.restype = None
        self.L.colour_sim_table_check.argtypes = [vp, C.c_float, i32, i32, vp, vp]

    def tail(self, xyb, cc15, enc, lum, bpp, fmt=U8X4, use_table=True):
        xyb = np.ascontiguousarray(xyb, np.float32)
        _, h, w = xyb.shape
        pb = 8 if fmt == U16X4 else 4
        out = np.zeros((h, w * pb), np.uint8)
        cc = np.ascontiguousarray(cc15, np.float32); e = np.ascontiguousarray(enc, np.int32); lm = np.ascontiguousarray(lum, np.float32)
        r = self.L.colour_sim_tail(xyb.ctypes.data, w, h, cc.ctypes.data, e.ctypes.data, lm.ctypes.data, bpp, 1 if use_table else 0, 1 if pb == 8 else 0, out.ctypes.data, w * pb)
        assert r >= 0
        return (out.view(np.uint16) if pb == 8 else out).reshape(h, w, 4), r == 1

    def levels(self, enc, it, v, bpp):
        v = np.ascontiguousarray(v, np.float32); e = np.ascontiguousarray(enc, np.int32)
        out = np.zeros(v.size, np.int32)
        self.L.colour_sim_levels(e.ctypes.data, float(it), v.ctypes.data, v.size, bpp, out.ctypes.data)
        return out.reshape(v.shape)

    def hlg_ootf(self, enc, it, lum, v):
        v = np.array(v, np.float32, order="C"); e = np.ascontiguousarray(enc, np.int32); lm = np.ascontiguousarray(lum, np.float32)
        self.L.colour_sim_hlg_ootf(e.ctypes.data, float(it), lm.ctypes.data, v.ctypes.data, v.size // 3)
        return v

    def pow(self, x, p):
        x = np.ascontiguousarray(x, np.float64); p = np.ascontiguousarray(np.broadcast_to(p, x.shape), np.float64)
        out = np.zeros(x.shape, np.float64)
        self.L.colour_sim_pow(x.ctypes.data, p.ctypes.data, x.size, out.ctypes.data)
        return out

    def table_check(self, enc, it, step=1, threads=8):
        e = np.ascontiguousarray(enc, np.int32)
        out = np.zeros(6, np.int64); thr = np.zeros(258, np.float32)
        self.L.colour_sim_table_check(e.ctypes.data, float(it), step, threads, out.ctypes.data, thr.ctypes.data)
        return {"table": bool(out[0]), "blo": int(out[1]), "bhi": int(out[2]), "compared": int(out[3]), "differ": int(out[4]), "first": int(out[5]), "thr": thr}


# ---------------------------------------------------------------- the float64 model

def model_transfer(enc, it, v):
    """f in [0, 1] of linear values v (float64; 1.0 = intensity_target nits) by the encoding's curve: the formulas of include/j40hip.h. For
    HLG, v is what the inverse OOTF left"""
    v = np.asarray(v, np.float64)
    pos = v > 0
    x = np.where(pos, v, 1.0)
    have_gamma, gamma, tf = int(enc[11]), int(enc[12]), int(enc[13])
    if have_gamma:
        f = x ** (gamma / 1e7)
    elif tf == 8:
        f = x
    elif tf == 13:
        f = np.where(x <= 0.0031308, 12.92 * x, 1.055 * x ** (1 / 2.4) - 0.055)
    elif tf == 1:
        f = np.where(x < 0.018, 4.5 * x, 1.099 * x ** 0.45 - 0.099)
    elif tf == 17:
        f = x ** (1 / 2.6)
    elif tf == 16:
        m1, m2, c1, c2, c3 = 2610 / 16384, 2523 / 32, 3424 / 4096, 2413 / 128, 2392 / 128
        ym = np.minimum(x * (float(it) / 10000.0), 1e6) ** m1   # (f is 1 from Y = 1 on: the cap changes nothing and keeps inf / inf out)
        f = ((c1 + c2 * ym) / (1 + c3 * ym)) ** m2
    elif tf == 18:
        a = 0.17883277; b = 1 - 4 * a; c = 0.5 - a * np.log(4 * a)
        f = np.where(x <= 1 / 12, np.sqrt(3 * x), a * np.log(np.maximum(12 * x - b, 1e-300)) + c)
    else:
        raise ValueError(tf)
    return np.where(pos, np.clip(f, 0.0, 1.0), 0.0)


def model_level(enc, it, v, bpp):
    """(level, u): level = clamp(floor(u), 0, maxpixel) with u = maxpixel * f + 0.5, float64"""
    maxpixel = (1 << bpp) - 1
    u = maxpixel * model_transfer(enc, it, v) + 0.5
    return np.clip(np.floor(u), 0, maxpixel).astype(np.int64), u


def hlg_gamma(it):
    return 1.2 * 1.111 ** np.log2(float(it) / 1000.0)


def model_hlg_ootf(it, lum, v):
    """BT.2100's inverse OOTF on [..., 3] target-space values, float64"""
    v = np.asarray(v, np.float64)
    yd = (v * np.asarray(lum, np.float64)).sum(-1, keepdims=True)
    s = np.where(yd > 0, np.where(yd > 0, yd, 1.0) ** (1 / hlg_gamma(it) - 1), 1.0)
    return v * s


def to_u8(level, bpp):
    maxpixel = (1 << bpp) - 1
    return (level * 255 + (1 << (bpp - 1))) // maxpixel


def to_u16(level, bpp):
    maxpixel = (1 << bpp) - 1
    return (level * 65535 + (1 << (bpp - 1))) // maxpixel


def folded_matrix(P, opsin_inv_mat):
    """m' = float32(P . m), the product in float64"""
    return (np.asarray(P, np.float64) @ np.asarray(opsin_inv_mat, np.float64)).astype(np.float32)


def model_interval(xyb, m_folded, opsin_bias, it, enc, lum, bpp):
    """The interval test of a whole decode. xyb [3, h, w] float32 (the frame's own planes). In float64: the linear values v of the tail
    and the forward bound of its float32 mixing e = 16 * 2^-24 * sum_j |m'_cj| (|pp_j|^3 + |bias_j|) * itscale, per sample; the level at
    v - e and at v + e (the curves are monotone; HLG: the OOTF's scale taken at the same end). Returns (lo, hi) [h, w, 3] levels."""
    x, y, b = (xyb[c].astype(np.float64) for c in range(3))
    bias = np.asarray(opsin_bias, np.float64)
    cb = np.cbrt(bias.astype(np.float32)).astype(np.float64)   # (cbrtf on the host, as the frame constants are made)
    itscale = float(np.float32(255.0) / np.float32(it))
    pp = np.stack([y + x - cb[0], y - x - cb[1], b - cb[2]], -1)
    s = (pp ** 3 + bias) * itscale
    mag = (np.abs(pp) ** 3 + np.abs(bias)) * itscale
    m = np.asarray(m_folded, np.float64)
    v = s @ m.T
    e = 16 * 2.0 ** -24 * (mag @ np.abs(m).T)
    lo_v, hi_v = v - e, v + e
    if int(enc[13]) == 18 and not int(enc[11]):
        # the three values move together through the OOTF: its scale is monotone in Yd, and Yd's own bound is e's luminance
        lumv = np.asarray(lum, np.float64)
        g = 1 / hlg_gamma(it) - 1   # (negative for every intensity_target above ~ 50 nits: a larger Yd scales down)
        yd = (v * lumv).sum(-1, keepdims=True); ye = (e * np.abs(lumv)).sum(-1, keepdims=True) + 4 * 2.0 ** -24 * (np.abs(v) * np.abs(lumv)).sum(-1, keepdims=True)
        def scale(q):
            return np.where(q > 0, np.where(q > 0, q, 1.0) ** g, 1.0)
        s_a, s_b = scale(yd - ye), scale(yd + ye)
        s_lo, s_hi = np.minimum(s_a, s_b) * (1 - 4 * 2.0 ** -24), np.maximum(s_a, s_b) * (1 + 4 * 2.0 ** -24)
        # (a Yd interval that straddles 0 also holds scale 1: "nothing where Yd <= 0")
        straddle = (yd - ye <= 0) & (yd + ye > 0)
        s_lo = np.where(straddle, np.minimum(s_lo, 1.0), s_lo); s_hi = np.where(straddle, np.maximum(s_hi, 1.0), s_hi)
        cands = [lo_v * s_lo, lo_v * s_hi, hi_v * s_lo, hi_v * s_hi]
        lo_v, hi_v = np.minimum.reduce(cands), np.maximum.reduce(cands)
    return model_level(enc, it, lo_v, bpp)[0], model_level(enc, it, hi_v, bpp)[0]
