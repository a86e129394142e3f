"""Upsampling streams for tests/test_upsampling.py and tests/test_upsampling_gpu.py (TEST INFRASTRUCTURE): the generator's upsampling=
streams and their twins, the numpy statement of the rule in j40_amd/csrc/device/upsample_dev.h (float32, one rounding per operation,
the 25 products added in source order, the clamp to the window's range), and the shapes, weights and inputs the tests share.

The VarDCT frame is 300 x 270 coded (the generator cannot write a one-group XYB VarDCT frame), the Modular one 200 x 136. Shown sizes:
K * coded, and one cut on both axes (ceil and the crop: 599 x 537 at K = 2)."""
import hashlib
import os
import subprocess

import numpy as np

from streams import SYNTH, CACHE

SEED = 7
VW, VH = 300, 270            # the VarDCT frame as coded
MW, MH = 200, 136            # the Modular frame as coded
COUNT = {2: 15, 4: 55, 8: 210}
# coded (w, h): planes narrower than the halo, one past a tile (the kernel's is 32 x 8), one tile's multiple exactly
KAT_SHAPES = [(1, 1), (2, 1), (1, 3), (5, 5), (33, 9), (64, 32), (67, 35)]
F = np.float32


def up_synth(mode, w, h, seed=SEED, **opts):
    """the generator's stream for these options (cached by a hash of them: a weight list is long)"""
    args = [SYNTH, mode, str(w), str(h), str(seed)]
    tail = ["%s=%s" % kv for kv in sorted(opts.items())]
    os.makedirs(CACHE, exist_ok=True)
    path = os.path.join(CACHE, "up2_%s_%d_%d_%d_%s.jxl" % (mode, w, h, seed, hashlib.sha256(" ".join(tail).encode()).hexdigest()[:24]))
    if not os.path.exists(path):
        tmp = path + ".tmp%d" % os.getpid()
        subprocess.run(args + [tmp] + tail, check=True, stderr=subprocess.DEVNULL)
        os.replace(tmp, path)
    with open(path, "rb") as fp:
        return fp.read()


def cut_size(k, w, h):
    """a shown size that is no multiple of K on either axis and still codes at w x h"""
    return k * w - 1, k * h - (k - 1)


def weights_text(w):
    return ",".join(repr(float(v)) for v in w)


def pair(mode, w, h, k, weights="nearest", shown=None, **opts):
    """(the upsampled stream, its twin: the same coded frame with upsampling = 1 and no table)"""
    if mode == "modular":
        opts.setdefault("xyb", 1)
    if not isinstance(weights, str):
        weights = weights_text(weights)
    if shown is not None:
        opts["upshown"] = "%d,%d" % shown
    return up_synth(mode, w, h, upsampling=k, upweights=weights, **opts), up_synth(mode, w, h, upsampling=k, upweights=weights, uptwin=1, **opts)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def f16(w):
    """what a decoder reads back of values written as F16"""
    return np.asarray(w, np.float32).astype(np.float16).astype(np.float32)


# ---------------------------------------------------------------- weights and inputs

def centre_heavy(k):
    """about 0.6 at the centre taps (M[i][j] with i % 5 == 2 and j % 5 == 2), small distinct values elsewhere, a third of them negative:
    every value m / 32768 with m below 2048 is an F16 as it stands; 0.6 is not, its F16 is what a decoder holds"""
    n5 = 5 * k // 2
    out, t = [], 0
    for y in range(n5):
        for x in range(y, n5):
            if y % 5 == 2 and x % 5 == 2:
                out.append(0.6)
            else:
                m = 40 + (t * 37) % 211          # (211 is prime: 210 distinct values)
                out.append((-4 * m if t % 3 == 0 else (7 if k == 2 else 6) * m) / 32768.0)   # (K = 2 has one kernel: a little more, so that its sum leaves 1 as far as the others' do)
            t += 1
    return f16(out)


def distinct_table(k):
    """every packed weight different from every other (a transposed or flipped index shows)"""
    return np.arange(1, COUNT[k] + 1, dtype=np.float32) / F(256.0)


def nearest_table(k):
    n5 = 5 * k // 2
    return np.array([1.0 if y % 5 == 2 and x % 5 == 2 else 0.0 for y in range(n5) for x in range(y, n5)], np.float32)


def kat_planes(w, h, seed=SEED):
    """a gradient plus seeded noise, [3, h, w] float32"""
    rng = np.random.default_rng(seed * 100003 + w * 1009 + h)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float32)
    grad = (xx * F(0.03) + yy * F(0.02)).astype(np.float32)
    return np.stack([grad * F(s) + rng.normal(0.0, 0.05, (h, w)).astype(np.float32) for s in (0.1, 1.0, 0.7)]).astype(np.float32)


# ---------------------------------------------------------------- the rule in numpy

def mirror(x, n):
    while x < 0 or x >= n:
        x = -x - 1 if x < 0 else 2 * n - 1 - x
    return x


def expand(k, w):
    """E[oy, ox, ky', kx']: the weight output phase (ox, oy) gives the coded sample at (kx' - 2, ky' - 2), by the rule's three steps"""
    n = k // 2
    n5 = 5 * n
    w = np.asarray(w, np.float32)
    assert w.size == COUNT[k]
    M = np.zeros((n5, n5), np.float32)
    for i in range(n5):
        for j in range(n5):
            y, x = min(i, j), max(i, j)
            M[i][j] = w[n5 * y - y * (y - 1) // 2 + x - y]
    kernel = np.zeros((n, n, 5, 5), np.float32)
    for i in range(n5):
        for j in range(n5):
            kernel[j // 5][i // 5][j % 5][i % 5] = M[i][j]
    E = np.zeros((k, k, 5, 5), np.float32)
    for oy in range(k):
        for ox in range(k):
            kern = kernel[oy if oy < n else k - 1 - oy][ox if ox < n else k - 1 - ox]
            for ky in range(5):
                for kx in range(5):
                    # tap (ky, kx) is applied to source (kx', ky') with ky' = ky or 4 - ky, kx' likewise
                    E[oy, ox, ky if oy < n else 4 - ky, kx if ox < n else 4 - kx] = kern[ky][kx]
    return E


def upsample(planes, k, w, out_w=None, out_h=None, want_clamped=False):
    """the statement: planes [3, h, w] float32 -> [3, out_h, out_w] (default K * h, K * w); with want_clamped also how many samples of
    the uncut picture the clamp changed"""
    planes = np.asarray(planes, np.float32)
    _, h, wd = planes.shape
    E = expand(k, w)
    iy = [mirror(y, h) for y in range(-2, h + 2)]
    ix = [mirror(x, wd) for x in range(-2, wd + 2)]
    p = planes[:, iy][:, :, ix]
    views = [[p[:, sy:sy + h, sx:sx + wd] for sx in range(5)] for sy in range(5)]
    lo = views[0][0].copy(); hi = views[0][0].copy()
    for sy in range(5):
        for sx in range(5):
            v = views[sy][sx]
            lo = np.where(v < lo, v, lo); hi = np.where(v > hi, v, hi)
    out = np.zeros((3, k * h, k * wd), np.float32)
    clamped = 0
    for oy in range(k):
        for ox in range(k):
            acc = np.zeros((3, h, wd), np.float32)
            for sy in range(5):
                for sx in range(5):
                    acc = acc + F(E[oy, ox, sy, sx]) * views[sy][sx]
            r = np.where(acc < lo, lo, acc)
            r = np.where(r > hi, hi, r).astype(np.float32)
            clamped += int((bits(r) != bits(acc)).sum())
            out[:, oy::k, ox::k] = r
    out = np.ascontiguousarray(out[:, :(k * h if out_h is None else out_h), :(k * wd if out_w is None else out_w)])
    return (out, clamped) if want_clamped else out


def repeat(px, k, out_w, out_h):
    """np.repeat on both axes, cut to the shown size: what upweights=nearest makes of the twin's picture"""
    return np.ascontiguousarray(np.repeat(np.repeat(px, k, axis=0), k, axis=1)[:out_h, :out_w])
