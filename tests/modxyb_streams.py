"""Modular frames of XYB images (TEST INFRASTRUCTURE, for tests/test_modular_xyb.py and tests/test_modular_xyb_gpu.py): the generator's
xyb=1 streams, the rule's statement in numpy, the float64 model of the colour tail and the host restatement's wrapper.

The rule (PARITY UNPINNED). c0, c1, c2: the colour planes after every inverse transform; m = m_lf_scaled:
    Y = float32(c0) * m[1]    X = float32(c1) * m[0]    B = float32(c2 + c0) * m[2]     (integer sum, one conversion, one multiply)
and from X, Y, B on what a VarDCT frame's colour tail makes of them."""
import ctypes as C
import os
import subprocess

import numpy as np

from streams import synth, ROOT, SYNTH, CACHE

SEED = 11
PARSE_WIDE = 8
M_DEFAULT = np.array([1.0 / 4096, 1.0 / 512, 1.0 / 256], np.float32)
LFDEQUANT = "0.00048828125,0.00390625,0.0078125"       # 1/2048, 1/256, 1/128: twice the default steps, each times 128 an f16
M_LFDEQUANT = np.array([1.0 / 2048, 1.0 / 256, 1.0 / 128], np.float32)
# 2^-20, 2^-17, 2^-16: steps 256 times finer than the default, so that a picture's integers leave int16 (wide frames)
LFDEQUANT_FINE = "9.5367431640625e-07,7.62939453125e-06,1.52587890625e-05"
M_LFDEQUANT_FINE = np.array([2.0 ** -20, 2.0 ** -17, 2.0 ** -16], np.float32)
# tone= and opsin= as tests/tone_streams.py writes them
TONE = "64,1"


def opsin_option():
    import tone_streams as T
    return T.written_options(T.ROW["bias_distinct"][1])["opsin"]


def xyb_stream(w, h, seed=SEED, **opts):
    """a Modular frame of an XYB image: the procedural picture's integers read as quantised Y, X, B - Y"""
    return synth("modular", w, h, seed, xyb=1, **opts)


def xybpic_stream(w, h, seed=SEED, **opts):
    """(stream, source picture float32 [h, w, 3], sRGB samples in [0, 1]): xybpic=1, the picture itself quantised to XYB integers"""
    os.makedirs(CACHE, exist_ok=True)
    key = "modular_%d_%d_%d_%s" % (w, h, seed, "_".join("%s-%s" % kv for kv in sorted(opts.items())))
    path, rgb = os.path.join(CACHE, key + ".xybpic.jxl"), os.path.join(CACHE, key + ".xybpic.f32")
    if not (os.path.exists(path) and os.path.exists(rgb)):
        tmp, tmp_rgb = path + ".tmp%d" % os.getpid(), rgb + ".tmp%d" % os.getpid()
        subprocess.run([SYNTH, "modular", str(w), str(h), str(seed), tmp, "xyb=1", "xybpic=1", "dumprgb=" + tmp_rgb] + ["%s=%s" % kv for kv in sorted(opts.items())],
                       check=True, stderr=subprocess.DEVNULL)
        os.replace(tmp_rgb, rgb)
        os.replace(tmp, path)
    with open(path, "rb") as fp:
        data = fp.read()
    return data, np.fromfile(rgb, np.float32).reshape(h, w, 3)


def statement(c, m):
    """the planes X, Y, B [3, h, w] float32 of integer planes c [3, h, w] (int16 or int32): numpy's float32 arithmetic, the integer
    sum first in a type that holds it"""
    m = np.asarray(m, np.float32)
    c = np.asarray(c)
    wide_t = np.int64 if c.dtype == np.int32 else np.int32
    total = c[2].astype(wide_t) + c[0].astype(wide_t)
    return np.stack([c[1].astype(np.float32) * m[0], c[0].astype(np.float32) * m[1], total.astype(np.float32) * m[2]])


def consts15(matrix, bias, intensity_target):
    return np.concatenate([np.asarray(matrix, np.float32).reshape(9), np.asarray(bias, np.float32), [np.float32(intensity_target), 0, 0]]).astype(np.float32)


def float64_model(c, m, cc15, bpp=8):
    """the rule, the inverse opsin transform and the sRGB transfer in float64, from the 15 constants j40hip_frame_colour_consts returns:
    (u [h, w, 3]: maxpixel * t + 0.5, the level's value before it is truncated; the 8-bit pixels [h, w, 3] that follow from it)"""
    c = np.asarray(c).astype(np.int64)
    m = np.asarray(m, np.float32).astype(np.float64)
    cc = np.asarray(cc15, np.float32).astype(np.float64)
    y, x, b = c[0] * m[1], c[1] * m[0], (c[2] + c[0]) * m[2]
    mat, bias, it = cc[:9].reshape(3, 3), cc[9:12], cc[12]
    p = np.stack([y + x, y - x, b])
    s = ((p - np.cbrt(bias)[:, None, None]) ** 3 + bias[:, None, None]) * (255.0 / it)
    v = np.einsum("ck,khw->hwc", mat, s)
    t = np.where(v <= 0.0031308, 12.92 * v, 1.055 * np.power(np.abs(v), 1.0 / 2.4) - 0.055)
    maxpixel = (1 << bpp) - 1
    u = float(maxpixel) * t + 0.5
    # the level as the VarDCT colour tail makes it (j40.h:7213-7240): truncation, the reference's (int16_t) conversion -- which wraps from
    # 32768 on, so at 16 bits the upper half of the range comes out as 0 -- then the clamp
    i = np.trunc(np.where(np.abs(u) >= 2.0 ** 31, 0.0, u)).astype(np.int64)
    i16 = ((i & 0xFFFF) ^ 0x8000) - 0x8000
    level = np.clip(i16, 0, maxpixel)
    return u, ((level * 255 + (1 << (bpp - 1))) // maxpixel).astype(np.uint8)


def boundary_exempt(u, bpp=8, eps=1e-3):
    """samples whose unrounded value lies within eps of a level of a rounding boundary: level k - 1 turns into level k at u = k, for
    k = 1 .. maxpixel (below 1 and above maxpixel the clamp holds the level whatever u is)"""
    maxpixel = (1 << bpp) - 1
    k = np.round(u)
    return (np.abs(u - k) < eps) & (k >= 1) & (k <= maxpixel)


def alpha_u8(a, bpp=8):
    maxpixel = (1 << bpp) - 1
    return ((np.clip(np.asarray(a).astype(np.int64), 0, maxpixel) * 255 + (1 << (bpp - 1))) // maxpixel).astype(np.uint8)


def alpha_u16(a, bpp=8):
    maxpixel = (1 << bpp) - 1
    return ((np.clip(np.asarray(a).astype(np.int64), 0, maxpixel) * 65535 + (1 << (bpp - 1))) // maxpixel).astype(np.uint16)


class XybSim:
    """build/libhostsim_modxyb.so: device/modular_xyb_dev.h's lane functions on the CPU"""

    def __init__(self):
        L = self.L = C.CDLL(os.path.join(ROOT, "build", "libhostsim_modxyb.so"))
        L.modxyb_sim_planes.restype = C.c_int32
        L.modxyb_sim_planes.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_size_t]
        L.modxyb_sim_pack.restype = C.c_int32
        L.modxyb_sim_pack.argtypes = [C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_size_t]

    @staticmethod
    def _ptrs(planes):
        planes = [np.ascontiguousarray(p) for p in planes]
        return planes, (C.c_void_p * 3)(*[p.ctypes.data for p in planes])

    def planes(self, c, m, rect=None):
        """k_modular_to_xyb over planes c [3, h, w] (the rectangle (x0, y0, rw, rh), or all of them): [3, rh, rw] float32"""
        c = np.ascontiguousarray(c)
        _, h, w = c.shape
        x0, y0, rw, rh = rect or (0, 0, w, h)
        keep, ptrs = self._ptrs([c[0], c[1], c[2]])
        out = np.full((3, rh, rw), -1.0, np.float32)
        outs = (C.c_void_p * 3)(*[out[k].ctypes.data for k in range(3)])
        mm = np.ascontiguousarray(m, np.float32)
        assert self.L.modxyb_sim_planes(ptrs, c.dtype.itemsize, w, x0, y0, rw, rh, mm.ctypes.data, outs, rw) == 0
        return out

    def pack(self, c, alpha, m, cc15, bpp=8, u16=False, on=True, rect=None):
        """decode_modular's last step over planes c [3, h, w]: [h, w, 4] uint8 / uint16 (pixels outside the rectangle stay 0)"""
        c = np.ascontiguousarray(c)
        _, h, w = c.shape
        x0, y0, rw, rh = rect or (0, 0, w, h)
        keep, ptrs = self._ptrs([c[0], c[1], c[2]])
        a = None if alpha is None else np.ascontiguousarray(alpha, c.dtype)
        out = np.zeros((h, w, 4), np.uint16 if u16 else np.uint8)
        mm = np.ascontiguousarray(m, np.float32); cc = np.ascontiguousarray(cc15, np.float32)
        assert self.L.modxyb_sim_pack(1 if on else 0, ptrs, a.ctypes.data if a is not None else None, c.dtype.itemsize, w, x0, y0, rw, rh, mm.ctypes.data, cc.ctypes.data,
                                      bpp, 1 if u16 else 0, out.ctypes.data, w * (8 if u16 else 4)) == 0
        return out


def host_consts(j40, data, wide=False):
    """(m [3] float32, the 15 colour constants, info) of a stream by the host parser alone (no device)"""
    fr = j40.Frame(data, wide=wide)
    try:
        a = np.zeros(15, np.float32)
        j40.lib().j40hip_frame_colour_consts(fr.h, a.ctypes.data)
        return fr.lf_dequant(), a, dict(fr.info)
    finally:
        fr.close()
