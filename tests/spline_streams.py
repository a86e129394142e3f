"""Spline streams for tests/test_splines.py and tests/test_splines_gpu.py (TEST INFRASTRUCTURE): the generator's splines= streams and
their twins, and the numpy statements of the rule in j40_amd/csrc/device/spline_dev.h -- the dequantisation into segments in float64
(Python floats: one rounding per operation, in the stated order) and the splat in float32.

The Modular frame is 96 x 80: 2 x 3 tiles of 64 x 32 with partial ones at the right and at the bottom. The generator cannot write a
one-group XYB VarDCT frame, so the VarDCT frame is 288 x 80: two groups, 5 x 3 tiles, the right and the bottom ones partial."""
import hashlib
import math
import os
import subprocess

import numpy as np

from streams import SYNTH, CACHE

SEED = 7
MW, MH = 96, 80
VW, VH = 288, 80
TILE_W, TILE_H = 64, 32
F = np.float32
WEIGHT = (0.0042, 0.075, 0.07, 0.3333)


def spline_synth(mode, w, h, seed=SEED, **opts):
    """the generator's stream for these options (cached by a hash of them)"""
    args = [SYNTH, mode, str(w), str(h), str(seed)]
    tail = ["%s=%s" % kv for kv in sorted(opts.items())]
    os.makedirs(CACHE, exist_ok=True)
    path = os.path.join(CACHE, "spline_%s_%d_%d_%d_%s.jxl" % (mode, w, h, seed, hashlib.sha256(" ".join(tail).encode()).hexdigest()[:24]))
    if not os.path.exists(path):
        tmp = path + ".tmp%d" % os.getpid()
        subprocess.run(args + [tmp] + tail, check=True, stderr=subprocess.DEVNULL)
        os.replace(tmp, path)
    with open(path, "rb") as fp:
        return fp.read()


def spline(points, coef):
    """a spline as the tests state it: its control points (absolute, integers) and its non-zero quantised coefficients {(c, i): v},
    c = 0 X, 1 Y, 2 B, 3 sigma"""
    return {"points": [(int(x), int(y)) for x, y in points], "coef": dict(coef)}


def double_deltas(points):
    out, delta, cur = [], (0, 0), points[0]
    for p in points[1:]:
        step = (p[0] - cur[0], p[1] - cur[1])
        out.append((step[0] - delta[0], step[1] - delta[1]))
        delta, cur = step, p
    return out


def text_of(splines):
    """the generator's description: x,y[:dx,dy...][|c:i=v,...] per spline, '/' between splines"""
    parts = []
    for s in splines:
        pts = ["%d,%d" % s["points"][0]] + ["%d,%d" % d for d in double_deltas(s["points"])]
        one = ":".join(pts)
        if s["coef"]:
            one += "|" + ",".join("%d:%d=%d" % (c, i, v) for (c, i), v in sorted(s["coef"].items()))
        parts.append(one)
    return "/".join(parts)


def pair(mode, w, h, splines, **opts):
    """(the stream with the splines, its twin without the flag and the data)"""
    if mode == "modular":
        opts.setdefault("xyb", 1)
    t = text_of(splines)
    return spline_synth(mode, w, h, splines=t, **opts), spline_synth(mode, w, h, splines=t, splinetwin=1, **opts)


def coef_array(s):
    a = np.zeros((4, 32), np.int32)
    for (c, i), v in s["coef"].items():
        a[c, i] = v
    return a


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---------------------------------------------------------------- the dequantisation in float64

def catmull_rom(pts):
    pts = [(float(x), float(y)) for x, y in pts]
    if len(pts) == 1:
        return [pts[0]]
    e = [(pts[0][0] + (pts[0][0] - pts[1][0]), pts[0][1] + (pts[0][1] - pts[1][1]))] + pts
    e.append((pts[-1][0] + (pts[-1][0] - pts[-2][0]), pts[-1][1] + (pts[-1][1] - pts[-2][1])))
    out = []
    for w in range(len(e) - 3):
        p = e[w:w + 4]
        out.append(p[1])
        t = [0.0]
        for i in range(1, 4):
            dx, dy = p[i][0] - p[i - 1][0], p[i][1] - p[i - 1][1]
            t.append(t[i - 1] + math.sqrt(math.sqrt(dx * dx + dy * dy)))
        for j in range(1, 16):
            tt = t[1] + (j / 16.0) * (t[2] - t[1])
            A = []
            for i in range(3):
                f = (tt - t[i]) / (t[i + 1] - t[i])
                A.append((p[i][0] + f * (p[i + 1][0] - p[i][0]), p[i][1] + f * (p[i + 1][1] - p[i][1])))
            B = []
            for i in range(2):
                f = (tt - t[i]) / (t[i + 2] - t[i])
                B.append((A[i][0] + f * (A[i + 1][0] - A[i][0]), A[i][1] + f * (A[i + 1][1] - A[i][1])))
            f = (tt - t[1]) / (t[2] - t[1])
            out.append((B[0][0] + f * (B[1][0] - B[0][0]), B[0][1] + f * (B[1][1] - B[0][1])))
    out.append(pts[-1])
    return out


def equal_spacing(poly):
    """-> (points, multipliers, the smallest |acc + len - 1| met: how far the walk stayed from a tie)"""
    pts, mult = [poly[0]], [1.0]
    cur, acc, margin = poly[0], 0.0, math.inf
    for q in poly[1:]:
        dx, dy = q[0] - cur[0], q[1] - cur[1]
        ln = math.sqrt(dx * dx + dy * dy)
        margin = min(margin, abs(acc + ln - 1.0))
        while acc + ln >= 1.0:
            f = (1.0 - acc) / ln
            cur = (cur[0] + f * dx, cur[1] + f * dy)
            pts.append(cur); mult.append(1.0)
            acc = 0.0
            dx, dy = q[0] - cur[0], q[1] - cur[1]
            ln = math.sqrt(dx * dx + dy * dy)
            margin = min(margin, abs(acc + ln - 1.0))
        acc += ln
        cur = q
    pts.append(poly[-1]); mult.append(acc)
    return pts, mult, margin


def model_segments(splines, quant_adjust, ytox, ytob, w, h):
    """the float64 statement: -> (rows, margins). A row: dict with the box (x0, x1, y0, y1), and cx, cy, mult, inv_sigma, s4, col in
    float64 before they are stored as float32. margins: the smallest distance of a box edge's v + 1/2 from an integer, and of a
    spacing step from a tie -- the tests assert both are well away from zero before they compare boxes and counts"""
    qa = float(quant_adjust)
    inv_q = 1.0 / (1.0 + qa / 8.0) if quant_adjust >= 0 else 1.0 - qa / 8.0
    sqrt2, ln = math.sqrt(2.0), 5.0 * math.log(10.0)
    rows, edge_margin, tie_margin = [], math.inf, math.inf
    for s in splines:
        q = coef_array(s)
        coef = [[((float(q[c, i]) * (math.sqrt(0.5) if i == 0 else 1.0)) * WEIGHT[c]) * inv_q for i in range(32)] for c in range(4)]
        for i in range(32):
            coef[0][i] += float(F(ytox)) * coef[1][i]
            coef[2][i] += float(F(ytob)) * coef[1][i]
        pts, mult, margin = equal_spacing(catmull_rom(s["points"]))
        tie_margin = min(tie_margin, margin)
        arc = float(len(pts) - 2) + mult[-1]
        if not arc > 0.0:
            continue
        for k, (px, py) in enumerate(pts):
            t = 31.0 * min(1.0, float(k) / arc)
            val = []
            for c in range(4):
                acc = 0.0
                for i in range(32):
                    if coef[c][i] != 0.0:
                        acc += (coef[c][i] * sqrt2) * math.cos(((math.pi / 32.0) * float(i)) * (t + 0.5))
                val.append(acc)
            sigma, m1 = val[3], mult[k]
            if sigma == 0.0 or not math.isfinite(sigma) or not math.isfinite(1.0 / sigma) or not math.isfinite(m1):
                continue
            m = max([0.01] + [abs(val[c] * m1) for c in range(3)])
            d = math.sqrt(((2.0 * sigma) * sigma) * (ln + math.log(m)))
            box, empty = [], False
            for centre, n in ((px, w), (py, h)):
                lo, hi = (centre - d) + 0.5, (centre + d) + 0.5
                for v in (lo, hi):
                    edge_margin = min(edge_margin, abs(v - round(v)))
                a, b = max(math.floor(lo), 0), min(math.floor(hi), n - 1)
                empty = empty or a > b
                box += [a, b]
            if empty:
                continue
            rows.append({"box": tuple(box), "cx": px, "cy": py, "mult": m1, "inv_sigma": 1.0 / sigma, "s4": (0.25 * sigma) * m1, "col": tuple(val[:3])})
    return rows, (edge_margin, tie_margin)


def pack_segments(rows):
    """model rows -> the [n, 12] uint32 words of the layout (float32 fields rounded from the float64 values)"""
    a = np.zeros((len(rows), 12), np.uint32)
    for k, r in enumerate(rows):
        a[k, 0:4] = np.array(r["box"], np.int32).view(np.uint32)
        a[k, 4:11] = np.array([r["cx"], r["cy"], r["inv_sigma"], r["s4"], r["col"][0], r["col"][1], r["col"][2]], np.float64).astype(np.float32).view(np.uint32)
    return a


def make_segment(x0, x1, y0, y1, cx, cy, sigma, mult, col):
    """one record of the layout from float values"""
    a = np.zeros(12, np.uint32)
    a[0:4] = np.array([x0, x1, y0, y1], np.int32).view(np.uint32)
    a[4:11] = np.array([cx, cy, 1.0 / sigma, 0.25 * sigma * mult, col[0], col[1], col[2]], np.float32).view(np.uint32)
    return a


# ---------------------------------------------------------------- the splat in float32

def erf_r(x):
    x = np.asarray(x, np.float32)
    a = np.abs(x)
    with np.errstate(over="ignore"):   # (a huge argument: p is infinite and r is 1, as in the kernel)
        p = (((F(0.078108) * a + F(0.000972)) * a + F(0.230389)) * a + F(0.278393)) * a + F(1.0)
        r = F(1.0) - F(1.0) / ((p * p) * (p * p))
    return np.copysign(r, x).astype(np.float32)


def apply_segments(planes, segs):
    """the statement: planes [3, h, w] float32 -> the planes with the segments [n, 12] drawn, in their order"""
    out = np.array(planes, np.float32)
    segs = np.ascontiguousarray(segs, np.uint32).reshape(-1, 12)
    for g in segs:
        x0, x1, y0, y1 = (int(v) for v in g[0:4].view(np.int32))
        cx, cy, inv_sigma, s4, c0, c1, c2 = (F(v) for v in g[4:11].view(np.float32))
        dx = (np.arange(x0, x1 + 1).astype(np.float32) - cx)[None, :]
        dy = (np.arange(y0, y1 + 1).astype(np.float32) - cy)[:, None]
        dist = np.sqrt(dx * dx + dy * dy).astype(np.float32)
        f = erf_r((F(0.5) * dist + F(0.35355339)) * inv_sigma) - erf_r((F(0.5) * dist - F(0.35355339)) * inv_sigma)
        v = (s4 * f * f).astype(np.float32)
        for c, col in enumerate((c0, c1, c2)):
            out[c, y0:y1 + 1, x0:x1 + 1] = out[c, y0:y1 + 1, x0:x1 + 1] + col * v
    return out


def touched_tiles(segs, w):
    """the tiles the boxes touch and the longest list of one tile"""
    tiles_x = (w + TILE_W - 1) // TILE_W
    count = {}
    for g in np.ascontiguousarray(segs, np.uint32).reshape(-1, 12):
        x0, x1, y0, y1 = (int(v) for v in g[0:4].view(np.int32))
        for ty in range(y0 // TILE_H, y1 // TILE_H + 1):
            for tx in range(x0 // TILE_W, x1 // TILE_W + 1):
                count[ty * tiles_x + tx] = count.get(ty * tiles_x + tx, 0) + 1
    return len(count), max(count.values()) if count else 0


# ---------------------------------------------------------------- the shapes the CPU build and the kernel are both held to

STRAIGHT = spline([(12, 14), (70, 52)], {(1, 0): 40, (0, 0): 9, (2, 0): -12, (3, 0): 9})
CURVED = spline([(8, 60), (30, 15), (52, 48), (75, 22), (90, 66)], {(0, 0): 30, (0, 2): -6, (1, 0): -25, (1, 1): 11, (2, 0): 18, (2, 3): 5, (3, 0): 8, (3, 1): 3})
# (the first spline's starting point is unsigned in the stream: this one starts inside, leaves at the left, the bottom and the right)
OUTSIDE = spline([(30, 20), (-35, 50), (40, 95), (130, 41)], {(1, 0): 33, (2, 1): -9, (3, 0): 12})
ONE_POINT = spline([(40, 40)], {(1, 0): 40, (3, 0): 9})
CROSS_A = spline([(10, 10), (85, 70)], {(0, 0): 21, (1, 0): 37, (2, 0): -15, (3, 0): 7})
CROSS_B = spline([(12, 72), (84, 9)], {(0, 0): -17, (1, 0): 29, (2, 0): 23, (3, 0): 11})
ZIGZAG = spline([(5, 3), (57, 7), (6, 11), (56, 15), (5, 19), (57, 23), (6, 27)], {(1, 0): 31, (0, 1): 8, (2, 0): -14, (3, 0): 5})


def kat_cases():
    """name -> (w, h, segments [n, 12]): the cases of the kernel alone, shared by the CPU build's test and the device's"""
    cases = {}
    cases["one_segment_one_tile"] = (MW, MH, np.stack([make_segment(10, 31, 4, 26, 20.3, 15.2, 2.1, 1.0, (0.05, 0.31, -0.12))]))
    cases["box_over_four_tiles"] = (MW, MH, np.stack([make_segment(50, 80, 20, 45, 64.4, 31.7, 3.4, 0.83, (0.11, -0.2, 0.07))]))
    cases["clipped_at_four_edges"] = (MW, MH, np.stack([
        make_segment(0, 7, 30, 50, -2.2, 40.1, 2.0, 1.0, (0.2, 0.1, 0.3)), make_segment(88, 95, 30, 50, 97.6, 39.4, 2.0, 1.0, (0.2, -0.1, 0.3)),
        make_segment(40, 60, 0, 6, 50.5, -1.8, 1.7, 1.0, (-0.2, 0.1, 0.1)), make_segment(40, 60, 73, 79, 49.1, 81.3, 1.9, 0.6, (0.2, 0.4, -0.3))]))
    crossing = pack_segments(model_segments([CROSS_A, CROSS_B], 0, 0.0, 1.0, MW, MH)[0])
    cases["two_splines_crossing"] = (MW, MH, crossing)
    cases["zigzag_beyond_one_chunk"] = (MW, MH, pack_segments(model_segments([ZIGZAG], 1, 0.0, 1.0, MW, MH)[0]))
    cases["frame_65x33_spills"] = (65, 33, np.stack([make_segment(57, 64, 25, 32, 63.6, 31.7, 1.5, 1.0, (0.3, 0.2, -0.1)), make_segment(0, 64, 0, 32, 30.2, 16.9, 9.0, 0.4, (0.02, -0.03, 0.05))]))
    return cases


def kat_planes(w, h, seed=11):
    rng = np.random.default_rng(seed)
    return rng.uniform(-0.6, 0.9, (3, h, w)).astype(np.float32)
