"""Splines on the host (include/j40hip.h, J40HIP_PARSE_SPLINES): the switch, the parse of the spline data, what is refused, the segments
the dequantisation makes against a float64 statement in Python (tests/spline_streams.py), and device/spline_dev.h's erf_r, binning and
lane function compiled for the CPU (tests/hostsim/spline_sim.cpp), held bit for bit against numpy's float32. PARITY UNPINNED: the
reference holds no code for splines; tests/test_splines_gpu.py has the device and the anchors that reach the reference."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import spline_streams as S
from spline_streams import spline_synth, pair, text_of, spline
from streams import ROOT


@pytest.fixture(scope="module")
def j40(built):
    import j40_amd
    return j40_amd


def parse_code(j40, data, **kw):
    try:
        j40.Frame(data, **kw).close()
        return ""
    except j40.J40Error as e:
        return e.code


def sequence_codes(j40, data, **kw):
    """per coded frame: the row's code, else what its handle's parse answers; a sequence that does not open: its code alone"""
    try:
        seq = j40.Sequence(data, **kw)
    except j40.J40Error as e:
        return e.code
    try:
        out = []
        for k in range(seq.num_frames):
            code = seq.frame_info(k)["code"]
            if not code:
                try:
                    seq.frame(k)
                except j40.J40Error as e:
                    code = e.code
            out.append(code)
        return out
    finally:
        seq.close()


FRAMES = [("vardct", S.VW, S.VH), ("modular", S.MW, S.MH)]
GIVEN = [S.STRAIGHT, S.CURVED]


# ---------------------------------------------------------------- 1. the switch, the parse, the twin

@pytest.mark.parametrize("mode,w,h", FRAMES)
def test_switch_off_is_todo_and_switch_on_parses_what_was_written(j40, monkeypatch, mode, w, h):
    """this is a test that fails without the feature: the keyword does not exist"""
    monkeypatch.delenv("J40HIP_SPLINES", raising=False)
    with_splines, twin = pair(mode, w, h, GIVEN, qadj=-3)
    assert parse_code(j40, with_splines) == "TODO"
    fr = j40.Frame(with_splines, splines=True)
    got = fr.splines()
    assert got["quant_adjust"] == -3 and len(got["splines"]) == len(GIVEN)
    for g, s in zip(got["splines"], GIVEN):
        assert g["start"] == s["points"][0]
        assert g["deltas"].tolist() == [list(d) for d in S.double_deltas(s["points"])]
        assert np.array_equal(g["coef"], S.coef_array(s))
    assert fr.spline_segments().shape[0] > 0 and fr.spline_launches() == 0
    fr.close()
    # the twin parses either way, to the same fields
    a, b = j40.Frame(twin), j40.Frame(twin, splines=True)
    assert a.splines() is None and b.splines() is None
    assert (a.width, a.height) == (b.width, b.height) == (w, h)
    assert a.spline_segments().shape == (0, 12) and b.spline_bins() == (0, 0)
    a.close(); b.close()
    # the environment asks for every parse
    monkeypatch.setenv("J40HIP_SPLINES", "1")
    assert parse_code(j40, with_splines) == ""


def test_positive_adjustment_and_later_splines_left_of_earlier_ones(j40):
    given = [S.CURVED, S.STRAIGHT, S.OUTSIDE]   # (starting points that go down as well as up: signed differences)
    fr = j40.Frame(pair("modular", S.MW, S.MH, given, qadj=5)[0], splines=True)
    got = fr.splines()
    assert got["quant_adjust"] == 5
    assert [g["start"] for g in got["splines"]] == [s["points"][0] for s in given]
    fr.close()


# ---------------------------------------------------------------- 2. damaged streams

def damaged():
    w, h = S.MW, S.MH
    ok = text_of([S.STRAIGHT])
    lim = 1 << 23
    # (the first spline's starting point is unsigned in the stream: these start inside the frame and leave it)
    long_text = text_of([spline([(0, 40), (8000000, 41)], {(1, 0): 10, (3, 0): 9})])
    # 3 000 000 segments whose boxes all cover the frame's six tiles (sigma 942 700, a reach of 3.5 million samples): 18 000 000 pairs
    wide_text = text_of([spline([(0, 40), (3000000, 41)], {(3, 0): 4000000})])
    return [
        ("too_many_splines", dict(splines=ok, splinecount=w * h // 4 + 1)),
        ("too_many_control_points", dict(splines=ok, splinen=w * h // 2 + 1)),
        ("starting_coordinate", dict(splines=text_of([spline([(lim + 1, 10), (20, 20)], {(3, 0): 9})]))),
        ("control_point_coordinate", dict(splines=text_of([spline([(10, 10), (20, -lim - 1)], {(3, 0): 9})]))),
        ("equal_control_points", dict(splines=text_of([spline([(10, 10), (20, 20), (20, 20)], {(3, 0): 9})]))),
        ("too_many_segments", dict(splines=long_text)),
        ("too_many_tile_pairs", dict(splines=wide_text)),
    ]


@pytest.mark.parametrize("name,how", damaged(), ids=[d[0] for d in damaged()])
def test_damaged_streams_are_spln(j40, name, how):
    assert parse_code(j40, spline_synth("modular", S.MW, S.MH, xyb=1, **how), splines=True) == "spln"
    # a sequence: the refusal comes when the index is built -- a second frame's ends the index there, a first frame's fails the open
    second = dict(how, splines=";" + how["splines"])
    assert sequence_codes(j40, spline_synth("modular", S.MW, S.MH, xyb=1, frames=2, **second), splines=True, modular_xyb=True) == ["", "spln"]
    first = dict(how, splines=how["splines"] + ";")
    assert sequence_codes(j40, spline_synth("modular", S.MW, S.MH, xyb=1, frames=2, **first), splines=True, modular_xyb=True) == "spln"


def test_the_bounds_themselves_are_served(j40):
    """coordinates of magnitude 1 << 23 itself parse, as a starting point and as a control point: the refusals above are the bound"""
    lim = 1 << 23
    edge = [spline([(lim, 10), (lim - 30, 40)], {(3, 0): 9}), spline([(lim - 30, 12), (lim, 50)], {(3, 0): 9})]
    assert parse_code(j40, spline_synth("modular", S.MW, S.MH, xyb=1, splines=text_of(edge)), splines=True) == ""


def test_the_segment_bound_itself(j40):
    """1 << 22 points along a curve are served, one more is "spln". A straight spline from (0, 40) to (dx, 40 + 2048) is
    sqrt(dx^2 + 2048^2) = dx + 0.5000001 long for dx near 1 << 22 (the next term of the root is 3e-8): floor(length) + 2 points, the first,
    one per unit of arc and the last with the remaining half -- far from a tie. Sigma is zero, so every point is dropped as a segment:
    the bound counts the points, which are the work"""
    for dx, code in (((1 << 22) - 2, ""), ((1 << 22) - 1, "spln")):
        one = [spline([(0, 40), (dx, 40 + 2048)], {(1, 0): 10})]
        assert parse_code(j40, spline_synth("modular", S.MW, S.MH, xyb=1, splines=text_of(one)), splines=True) == code, dx


def test_spline_data_cut_short(j40):
    data = spline_synth("vardct", S.VW, S.VH, splines=text_of(GIVEN), splinecut=1)
    assert parse_code(j40, data, splines=True) == "shrt"
    assert parse_code(j40, data) == "TODO"


# ---------------------------------------------------------------- 3. what stays TODO

def test_refusals_at_parse(j40, monkeypatch):
    t = text_of(GIVEN)
    for env in (None, "1"):
        monkeypatch.delenv("J40HIP_SPLINES", raising=False)
        if env:
            monkeypatch.setenv("J40HIP_SPLINES", env)
        # an image with xyb_encoded = 0, VarDCT and Modular
        assert parse_code(j40, spline_synth("vardct", S.VW, S.VH, noxyb=1, fullheader=1, splines=t), splines=True) == "TODO"
        assert parse_code(j40, spline_synth("vardct", S.VW, S.VH, noxyb=1, fullheader=1, splines=t, splinetwin=1), splines=True) == ""
        assert parse_code(j40, spline_synth("modular", S.MW, S.MH, splines=t), splines=True) == "TODO"
        # an LF-only parse
        assert parse_code(j40, pair("vardct", S.VW, S.VH, GIVEN)[0], splines=True, lf_only=True) == "TODO"
        assert parse_code(j40, pair("vardct", S.VW, S.VH, GIVEN)[1], splines=True, lf_only=True) == ""
        # an LF frame (type 1) with has_splines; the same stream with the splines on the main frame alone parses
        lf = dict(lflevels=1, splines=t)
        assert sequence_codes(j40, spline_synth("vardct", 2060, 70, splinelf=1, **lf), lf_frames=True, splines=True) == ["TODO", ""]
        assert sequence_codes(j40, spline_synth("vardct", 2060, 70, **lf), lf_frames=True, splines=True) == ["", ""]
        assert sequence_codes(j40, spline_synth("vardct", 2060, 70, **lf), lf_frames=True) == ["", "" if env else "TODO"]
        # a reference-only frame (type 2) with has_splines
        ref = dict(frames=2, types="2,0", crops="0,0,264,40;", saves="1,0")
        assert sequence_codes(j40, spline_synth("vardct", S.VW, S.VH, splines=t + ";", **ref), patches=True, splines=True) == ["TODO", ""]
        assert sequence_codes(j40, spline_synth("vardct", S.VW, S.VH, splines=";" + t, **ref), patches=True, splines=True) == ["", ""]


# ---------------------------------------------------------------- 4. the segments against the float64 statement

def ulps(a, b):
    """the distance of two float32 arrays in units in the last place"""
    def key(v):
        i = np.ascontiguousarray(v, np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    return np.abs(key(a) - key(b))


SEGMENT_CASES = [
    ("straight", [S.STRAIGHT], 0, {}),
    ("curved", [S.CURVED], 0, {}),
    ("outside_both_sides", [S.OUTSIDE], 0, {}),
    ("one_point", [S.ONE_POINT], 0, {}),
    ("positive_adjustment", [S.CURVED, S.STRAIGHT], 3, {}),
    ("negative_adjustment", [S.OUTSIDE, S.CURVED], -5, {}),
    ("base_correlations", [S.CURVED, S.ZIGZAG], 1, dict(cfl=1)),
]


@pytest.mark.parametrize("name,given,qadj,extra", SEGMENT_CASES, ids=[c[0] for c in SEGMENT_CASES])
def test_segments_equal_the_model(j40, sim, name, given, qadj, extra):
    """count and boxes equal (the model's margins first); cx, cy and the multiplier -- + - x / sqrt alone -- bit for bit; colours,
    inv_sigma and s4 within one float32 ulp: the only slack is the two libms' cos and ln in float64"""
    mode, w, h = ("vardct", S.VW, S.VH) if extra else ("modular", S.MW, S.MH)
    ytox, ytob = (0.125, 0.75) if extra else (0.0, 1.0)   # (the generator's cfl=1: base_corr_x 0.125, base_corr_b 0.75; a Modular frame: 0 and 1)
    fr = j40.Frame(pair(mode, w, h, given, qadj=qadj, **extra)[0], splines=True)
    rows, (edge_margin, tie_margin) = S.model_segments(given, qadj, ytox, ytob, w, h)
    assert edge_margin > 1e-6 and tie_margin > 1e-6, "the case's coordinates sit on a rounding edge: choose others"
    got = fr.spline_segments()
    fr.close()
    want = S.pack_segments(rows)
    assert got.shape == want.shape
    if name == "one_point":
        assert got.shape[0] == 0
        return
    assert got.shape[0] > 0
    assert np.array_equal(got[:, 0:4], want[:, 0:4]), "boxes"
    assert np.array_equal(got[:, 4:6], want[:, 4:6]), "cx, cy"
    assert np.array_equal(got[:, 11], np.zeros(len(got), np.uint32))
    gf, wf = got[:, 6:11].view(np.float32), want[:, 6:11].view(np.float32)
    assert ulps(gf, wf).max() <= 1, ulps(gf, wf).max()
    # the multiplier is not a word of the record (s4 holds it times sigma / 4): the CPU build of the same dequantisation hands it out,
    # spline by spline, and it equals the model's in every bit of its float64 -- 1 along the curve, the remaining arc at its end
    at = 0
    for s in given:
        n, words, mults = sim.segments(s, qadj, ytox, ytob, w, h)
        assert n >= 0 and np.array_equal(words, got[at:at + n])
        model = np.array([r["mult"] for r in rows[at:at + n]], np.float64)
        assert np.array_equal(mults.view(np.uint64), model.view(np.uint64))
        assert ((mults > 0.0) & (mults <= 1.0)).all() and (mults[:-1] == 1.0).all()   # (only a curve's last point has less than 1)
        at += n
    assert at == got.shape[0]


# ---------------------------------------------------------------- 5. erf_r and the CPU build of the splat

class SplineSim:
    def __init__(self):
        self.lib = C.CDLL(os.path.join(ROOT, "build", "libhostsim_splines.so"))
        self.lib.spline_sim_erf.argtypes = [C.c_void_p, C.c_int64, C.c_void_p]
        self.lib.spline_sim_draw.restype = C.c_int64
        self.lib.spline_sim_draw.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p]
        self.lib.spline_sim_chunk.restype = C.c_int32
        self.lib.spline_sim_segments.restype = C.c_int64
        self.lib.spline_sim_segments.argtypes = [C.c_int64, C.c_int64, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_float, C.c_float, C.c_int32, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p]

    def segments(self, s, qadj, ytox, ytob, w, h, cap=1 << 16):
        """one spline's segments by the CPU build of the dequantisation: (count or -1, the records [n, 12], their multipliers float64)"""
        dd = np.array(S.double_deltas(s["points"]), np.int64).reshape(-1, 2)
        coef = S.coef_array(s)
        out = np.zeros((cap, 12), np.uint32); mult = np.zeros(cap, np.float64)
        n = int(self.lib.spline_sim_segments(s["points"][0][0], s["points"][0][1], dd.ctypes.data if dd.size else None, dd.shape[0], coef.ctypes.data, qadj, ytox, ytob, w, h,
                                             out.ctypes.data, cap, mult.ctypes.data))
        assert n <= cap
        return n, out[:max(n, 0)], mult[:max(n, 0)]

    def erf(self, x):
        x = np.ascontiguousarray(x, np.float32)
        out = np.zeros_like(x)
        self.lib.spline_sim_erf(x.ctypes.data, x.size, out.ctypes.data)
        return out

    def draw(self, planes, segs):
        planes = np.array(planes, np.float32)
        segs = np.ascontiguousarray(segs, np.uint32)
        most = C.c_int64(0)
        tiles = self.lib.spline_sim_draw(planes.ctypes.data, planes.shape[2], planes.shape[1], segs.ctypes.data, segs.shape[0], C.byref(most))
        return tiles, int(most.value), planes


@pytest.fixture(scope="module")
def sim(built):
    return SplineSim()


def test_erf_r(sim):
    rng = np.random.default_rng(5)
    x = np.concatenate([rng.uniform(-6, 6, 9000), rng.normal(0, 0.3, 990), [0.0, -0.0, 1e-30, -1e-30, 40.0, -40.0, 3.4e38, -3.4e38, 0.35355339, 1.0]]).astype(np.float32)
    assert x.size == 10000
    got = sim.erf(x)
    assert np.array_equal(S.bits(got), S.bits(S.erf_r(x)))
    exact = np.array([math.erf(float(v)) for v in x])
    # Abramowitz-Stegun 7.1.27: 5e-4 in exact arithmetic; 1e-5 more for the float32 evaluation
    assert np.abs(got.astype(np.float64) - exact).max() <= 5e-4 + 1e-5


@pytest.mark.parametrize("name", list(S.kat_cases()))
def test_cpu_build_of_the_splat_equals_numpy(sim, name):
    w, h, segs = S.kat_cases()[name]
    planes = S.kat_planes(w, h)
    want = S.apply_segments(planes, segs)
    tiles, most, got = sim.draw(planes, segs)
    assert (tiles, most) == S.touched_tiles(segs, w)
    assert np.array_equal(S.bits(got), S.bits(want))
    assert not np.array_equal(S.bits(got), S.bits(planes))
    if name == "zigzag_beyond_one_chunk":
        assert most == 310 and most > 2 * sim.lib.spline_sim_chunk()          # 310 segments on one tile: three LDS chunks of 128
    if name == "two_splines_crossing":
        # the order of the additions is visible in the bits: the second spline drawn first gives other samples
        a = S.model_segments([S.CROSS_A], 0, 0.0, 1.0, w, h)[0]
        swapped = np.concatenate([segs[len(a):], segs[:len(a)]])
        assert not np.array_equal(S.bits(S.apply_segments(planes, swapped)), S.bits(want))


# ---------------------------------------------------------------- 6. the stand-alone program

@pytest.mark.parametrize("program", ["spline_main", "spline_main_san"])
def test_stand_alone_program_plain_and_sanitised(built, program):
    """the tiled, chunked draw against the rule sample by sample over planes in allocations of exactly their size, and the
    dequantisation over splines that leave the frame, are refused or draw nothing (tests/hostsim/spline_main.cpp)"""
    r = subprocess.run([os.path.join(ROOT, "build", program)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    assert r.returncode == 0, r.stdout.decode()
    assert b"0 failure(s)" in r.stdout
