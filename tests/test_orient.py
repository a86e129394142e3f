"""Oriented output (j40hip_frame_set_orientation, include/j40hip.h), without a device.

The oriented picture is an exact permutation of the pixels a handle writes in stored order. orient() below states it in index form --
output pixel (i, j) of orientation o is stored pixel (x, y), the table of include/j40hip.h -- and is the oracle of every test here and
in tests/test_orient_gpu.py. Here: orient() against numpy's own flips and rotations (and Pillow's, where it is installed); the
arithmetic k_orient runs (device/orient_dev.h) compiled for the CPU by build/libhostsim_orient.so (tests/hostsim/orient_sim.cpp) --
the row function of orientations 2 to 4, the tile functions of 5 to 8 with every lane's load before every lane's store --, the same as
a stand-alone program plain and under the host sanitizers; the rectangle maps; the parser, against the reference's decode of the same
stream; the setter's rules on parsed frames; and the generator, whose streams without orientation= are byte for byte what they were."""
import ctypes as C
import hashlib
import itertools
import os
import subprocess
import sys

import numpy as np
import pytest

from streams import synth, ROOT

U8X4, U16X4 = 0x0F33, 0x0F35
SEED = 7
TILE = 32    # ORIENT_TILE of device/orient_dev.h (asserted against the library below)

# o: (x, y) of output pixel (i, j) over a stored W x H image
SOURCE = {
    1: lambda W, H, i, j: (i, j),
    2: lambda W, H, i, j: (W - 1 - i, j),
    3: lambda W, H, i, j: (W - 1 - i, H - 1 - j),
    4: lambda W, H, i, j: (i, H - 1 - j),
    5: lambda W, H, i, j: (j, i),
    6: lambda W, H, i, j: (j, H - 1 - i),
    7: lambda W, H, i, j: (W - 1 - j, H - 1 - i),
    8: lambda W, H, i, j: (W - 1 - j, i),
}


def orient(a, o):
    """the definition: a [H, W, ...] in stored order -> the picture in orientation o, [H, W, ...] up to 4 and [W, H, ...] from 5 on"""
    H, W = a.shape[:2]
    ow, oh = (H, W) if o >= 5 else (W, H)
    jj, ii = np.mgrid[0:oh, 0:ow]
    x, y = SOURCE[o](W, H, ii, jj)
    return np.ascontiguousarray(a[y, x])


NUMPY_FORMS = {
    1: lambda a: a, 2: lambda a: a[:, ::-1], 3: lambda a: a[::-1, ::-1], 4: lambda a: a[::-1],
    5: lambda a: a.transpose(1, 0, 2), 6: lambda a: np.rot90(a, -1), 7: lambda a: a[::-1, ::-1].transpose(1, 0, 2), 8: lambda a: np.rot90(a, 1),
}


def all_differ(a):
    """the test's own test: the eight oriented forms of `a` are pairwise different (a mixed-up map cannot pass by symmetry)"""
    forms = [orient(a, o) for o in range(1, 9)]
    return all(x.shape != y.shape or not np.array_equal(x, y) for x, y in itertools.combinations(forms, 2))


def test_orient_is_the_definition():
    rng = np.random.default_rng(1)
    a = rng.integers(0, 256, (7, 5, 4), dtype=np.uint8)    # a 5 x 7 picture
    for o in range(1, 9):
        got = orient(a, o)
        assert got.shape == ((5, 7, 4) if o >= 5 else (7, 5, 4))
        assert np.array_equal(got, NUMPY_FORMS[o](a)), o
        for j in range(got.shape[0]):       # ... and pixel by pixel, without numpy's index arrays
            for i in range(got.shape[1]):
                x, y = SOURCE[o](5, 7, i, j)
                assert np.array_equal(got[j, i], a[y, x])
    assert all_differ(a)


def test_orient_is_pillows_exif_transpose():
    Image = pytest.importorskip("PIL.Image")
    T = getattr(Image, "Transpose", Image)
    exif = {2: T.FLIP_LEFT_RIGHT, 3: T.ROTATE_180, 4: T.FLIP_TOP_BOTTOM, 5: T.TRANSPOSE, 6: T.ROTATE_270, 7: T.TRANSVERSE, 8: T.ROTATE_90}
    rng = np.random.default_rng(2)
    a = rng.integers(0, 256, (7, 5, 4), dtype=np.uint8)
    for o, method in exif.items():
        assert np.array_equal(orient(a, o), np.asarray(Image.fromarray(a, "RGBA").transpose(method))), o


# ---------------------------------------------------------------- the kernel's arithmetic on the CPU

@pytest.fixture(scope="module")
def sim(built):
    L = C.CDLL(os.path.join(ROOT, "build", "libhostsim_orient.so"))
    L.orient_sim.restype = None
    L.orient_sim.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t] + [C.c_int32] * 5
    L.orient_sim_size.restype = None
    L.orient_sim_size.argtypes = [C.c_int32] * 3 + [C.c_void_p]
    L.orient_sim_source.restype = None
    L.orient_sim_source.argtypes = [C.c_int32] * 5 + [C.c_void_p]
    L.orient_sim_rect.restype = None
    L.orient_sim_rect.argtypes = [C.c_int32] * 4 + [C.c_void_p, C.c_void_p]
    L.orient_sim_tile.restype = C.c_int32
    L.orient_sim_tile.argtypes = []
    assert L.orient_sim_tile() == TILE
    return L


def run_sim(L, a, o, lanes=5, pad=24):
    """the CPU build of k_orient's functions over `a`; the output's rows carry `pad` guard bytes that must stay 0xA5"""
    H, W = a.shape[:2]
    pb = 4 * a.dtype.itemsize
    size = (C.c_int32 * 2)()
    L.orient_sim_size(W, H, o, size)
    ow, oh = size[0], size[1]
    assert (ow, oh) == ((H, W) if o >= 5 else (W, H))
    stride = ow * pb + pad
    out = np.full((oh, stride), 0xA5, np.uint8)
    src = np.ascontiguousarray(a)
    L.orient_sim(out.ctypes.data, stride, src.ctypes.data, W * pb, W, H, o, pb, lanes)
    assert (out[:, ow * pb:] == 0xA5).all(), "bytes behind the rows' pixels were written"
    return np.ascontiguousarray(out[:, :ow * pb]).view(a.dtype).reshape(oh, ow, 4)


SIM_SIZES = [(w, h) for w in range(1, 10) for h in range(1, 10)] + [(w, h) for w in (TILE - 1, TILE, TILE + 1, 2 * TILE + 3) for h in (TILE - 1, TILE, TILE + 1, 2 * TILE + 3)]


@pytest.mark.parametrize("dtype", [np.uint8, np.uint16], ids=["u8x4", "u16x4"])
def test_kernel_arithmetic_equals_orient(sim, dtype):
    rng = np.random.default_rng(100 + np.dtype(dtype).itemsize)
    top = np.iinfo(dtype).max
    checked = 0
    for w, h in SIM_SIZES:
        a = rng.integers(0, top + 1, (h, w, 4)).astype(dtype)
        if w != h and w * h >= 6 and min(w, h) >= 2:
            assert all_differ(a), (w, h)
            checked += 1
        for o in range(1, 9):
            got = run_sim(sim, a, o)
            assert got.dtype == a.dtype and np.array_equal(got, orient(a, o)), (w, h, o)
    assert checked >= 60
    # the lanes along a row of orientations 2 to 4: one, a few, more than the row has pixels
    a = rng.integers(0, top + 1, (9, 70, 4)).astype(dtype)
    for lanes in (1, 7, 64, 256):
        for o in (2, 3, 4):
            assert np.array_equal(run_sim(sim, a, o, lanes), orient(a, o)), (lanes, o)


def test_source_pixel_function(sim):
    out = (C.c_int32 * 2)()
    for W, H in ((5, 7), (1, 4), (6, 1)):
        for o in range(1, 9):
            ow, oh = (H, W) if o >= 5 else (W, H)
            for j in range(oh):
                for i in range(ow):
                    sim.orient_sim_source(W, H, o, i, j, out)
                    assert (out[0], out[1]) == SOURCE[o](W, H, i, j)


@pytest.mark.parametrize("program", ["orient_main", "orient_main_san"])
def test_stand_alone_program_plain_and_sanitised(built, program):
    """the same sweep outside Python, source and output in blocks of exactly their size; the second build under
    -fsanitize=address,undefined"""
    r = subprocess.run([os.path.join(ROOT, "build", program)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    assert " 0 mismatches, 0 guard bytes damaged" in r.stdout and "orient_main: %d cases" % (len(SIM_SIZES) * 16) in r.stdout, r.stdout


# ---------------------------------------------------------------- rectangles

def random_rects(rng, lw, lh, n):
    for _ in range(n):
        x0, y0 = int(rng.integers(0, lw)), int(rng.integers(0, lh))
        yield x0, y0, int(rng.integers(1, lw - x0 + 1)), int(rng.integers(1, lh - y0 + 1))


@pytest.mark.parametrize("o", range(1, 9))
def test_orient_rect(sim, built, o):
    """device/orient_dev.h's maps and, for the same rectangles, j40hip_frame_orient_rect of a parsed 11 x 7 frame"""
    import j40_amd
    W, H = 11, 7
    rng = np.random.default_rng(o)
    full = rng.integers(0, 256, (H, W, 4), dtype=np.uint8)
    shown = orient(full, o)
    oh, ow = shown.shape[:2]
    fr = j40_amd.Frame(synth("modular", W, H, SEED, orientation=o))
    assert fr.orientation()["orientation"] == o
    rin, rout = (C.c_int32 * 4)(), (C.c_int32 * 4)()
    for rect in random_rects(rng, ow, oh, 300):
        rin[:] = rect
        sim.orient_sim_rect(W, H, o, 1, rin, rout)
        stored = tuple(rout)
        x, y, w, h = stored
        assert x >= 0 and y >= 0 and w > 0 and h > 0 and x + w <= W and y + h <= H
        rin[:] = stored
        sim.orient_sim_rect(W, H, o, 0, rin, rout)
        assert tuple(rout) == rect, "displayed -> stored -> displayed"
        i0, j0, dw, dh = rect
        assert np.array_equal(shown[j0:j0 + dh, i0:i0 + dw], orient(full[y:y + h, x:x + w], o)), (rect, stored)
        assert fr.orient_rect(rect, to_stored=True) == ("", stored)
        assert fr.orient_rect(stored, to_stored=False) == ("", rect)
    for rect in random_rects(rng, W, H, 100):   # ... and starting from stored coordinates
        code, disp = fr.orient_rect(rect, to_stored=False)
        assert code == "" and fr.orient_rect(disp, to_stored=True) == ("", rect)
    # outside the frame the rectangle is given in: "rnge"
    for bad in ((0, 0, ow + 1, 1), (0, 0, 1, oh + 1), (-1, 0, 1, 1), (0, 0, 0, 1), (ow, 0, 1, 1), (0, 0, 2 ** 31 - 1, 1)):
        assert fr.orient_rect(bad, to_stored=True) == ("rnge", None), bad
    assert fr.orient_rect((0, 0, W + 1, 1), to_stored=False) == ("rnge", None)
    if o >= 5:
        assert fr.orient_rect((0, 0, W, H), to_stored=True)[0] == "rnge" and fr.orient_rect((0, 0, H, W), to_stored=True) == ("", (0, 0, W, H))
    fr.close()


# ---------------------------------------------------------------- the parser

PARSER_STREAMS = [("vardct", 40, 24, dict(passes=2)),   # (the generator writes no single-section VarDCT frame)
                  ("modular", 37, 21, dict(alpha=1))]


@pytest.mark.parametrize("mode,w,h,opts", PARSER_STREAMS, ids=[c[0] for c in PARSER_STREAMS])
def test_parser_reports_the_orientation(built, ref, mode, w, h, opts):
    """... and the reference decodes the stream to the pixels of the stream without the option: stored order is what it pins"""
    import j40_amd
    plain = synth(mode, w, h, SEED, **opts)
    fr = j40_amd.Frame(plain)
    assert fr.orientation()["orientation"] == 1 and (fr.width, fr.height) == (w, h)
    fr.close()
    rerr, want = ref.decode(plain)
    assert rerr == ""
    for n in range(1, 9):
        data = synth(mode, w, h, SEED, orientation=n, **opts)
        assert data != plain
        fr = j40_amd.Frame(data)
        assert fr.orientation()["orientation"] == n, n
        assert (fr.width, fr.height) == (w, h), "the frame's size is the stored one"
        fr.close()
        rerr, got = ref.decode(data)
        assert rerr == "" and np.array_equal(got, want), n


def test_parser_inside_an_animation_and_a_container(built):
    """an animation's extra fields carry the orientation too (only those three bits change); a container changes nothing"""
    import j40_amd
    opts = dict(passes=2, frames=2, anim=1, durations="1,1")
    plain, turned = synth("vardct", 40, 24, SEED, **opts), synth("vardct", 40, 24, SEED, orientation=6, **opts)
    assert len(plain) == len(turned)
    diff = [k for k in range(len(plain)) if plain[k] != turned[k]]
    assert len(diff) <= 2 and sum(bin(plain[k] ^ turned[k]).count("1") for k in diff) <= 3, diff
    fr = j40_amd.Frame(synth("modular", 37, 21, SEED, orientation=8, container=1))
    assert fr.orientation()["orientation"] == 8
    fr.close()


# ---------------------------------------------------------------- the setter's rules, on parsed frames

SETTER_CHILD = r"""
import sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import j40_amd
from streams import synth
w, h = 40, 24
for o in (3, 6):
    fr = j40_amd.Frame(synth("vardct", w, h, 7, orientation=o, passes=2))
    ow, oh = (h, w) if o >= 5 else (w, h)
    want_env = int(sys.argv[2])
    q = fr.orientation()
    assert (q["orientation"], q["applied"]) == (o, want_env), q                       # mode -1, the default: the environment
    assert (q["width"], q["height"]) == ((ow, oh) if want_env else (w, h)), q
    assert fr.set_orientation(1) == "" and fr.orientation()["applied"] == 1
    assert fr.set_orientation(0) == "" and fr.orientation()["applied"] == 0
    assert fr.set_orientation(-1) == "" and fr.orientation()["applied"] == want_env
    fr.close()
fr = j40_amd.Frame(synth("vardct", w, h, 7, passes=2))
assert fr.orientation()["applied"] == 0 and fr.set_orientation(1) == "" and fr.orientation()["applied"] == 0   # o = 1: nothing to apply
fr.close()
print("ok")
"""


@pytest.mark.parametrize("env", ["", "0", "1"], ids=["unset", "set_to_0", "set_to_1"])
def test_setter_modes_and_the_environment(built, env):
    e = dict(os.environ)
    e.pop("J40HIP_ORIENT", None)
    if env:
        e["J40HIP_ORIENT"] = env
    r = subprocess.run([sys.executable, "-c", SETTER_CHILD, ROOT, "1" if env == "1" else "0"], env=e, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip() == "ok", (r.stdout[-2000:], r.stderr[-2000:])


@pytest.mark.parametrize("mode,w,h", [("vardct", 777, 523), ("modular", 601, 303)])
@pytest.mark.parametrize("o", [3, 6])
def test_sizes_with_a_region_and_a_scale(built, mode, w, h, o):
    import j40_amd
    assert os.environ.get("J40HIP_ORIENT", "") in ("", "0"), "this test sets the mode itself"
    turn = (lambda a, b: (b, a)) if o >= 5 else (lambda a, b: (a, b))
    fr = j40_amd.Frame(synth(mode, w, h, SEED, orientation=o))
    blank = dict(orientation=o, applied=0, width=w, height=h, went_through_k_orient=0, staging_bytes=0)
    assert fr.orientation() == blank
    assert fr.set_orientation(1) == ""
    assert fr.orientation() == dict(blank, applied=1, width=turn(w, h)[0], height=turn(w, h)[1])
    assert fr.set_region(8, 16, 100, 50) == ""                     # a region stays a rectangle in stored coordinates
    assert (fr.orientation()["width"], fr.orientation()["height"]) == turn(100, 50)
    assert fr.set_orientation(0) == "" and (fr.orientation()["width"], fr.orientation()["height"]) == (100, 50)
    assert fr.clear_region() == "" and fr.set_orientation(1) == ""
    for k in (1, 2):
        s = 1 << k
        assert fr.set_scale(k) == ""
        assert (fr.orientation()["width"], fr.orientation()["height"]) == turn(-(-w // s), -(-h // s))
    assert fr.set_scale(0) == "" and fr.set_orientation(-1) == ""
    assert fr.orientation() == blank
    fr.close()


def test_sequence_frames_refuse_mode_1(built):
    import j40_amd
    seq = j40_amd.Sequence(synth("vardct", 300, 200, SEED, passes=2, frames=2, crops=";37,21,130,90"))
    for k in range(2):
        f = seq.frame(k)
        assert f.set_orientation(1) == "Uor?" and f.orientation()["applied"] == 0
        assert f.set_orientation(0) == "" and f.set_orientation(-1) == ""
    seq.close()


# ---------------------------------------------------------------- the generator

# SHA-256 of what the generator wrote for these option sets before it knew orientation= (recorded from a build of the commit before)
GENERATOR_PINS = [
    ("vardct", 520, 264, 1, dict(), "1308dbdf0ecb08241c4c8830a788bb21a01bb97a83f13886fa3a12d9971e7e39"),
    ("modular", 600, 300, 7, dict(tree=3, alpha=1), "e6f88b24eed516852d2d476f12777204cd22fa3b86e9f160848ed74a607717df"),
]


@pytest.mark.parametrize("mode,w,h,seed,opts,want", GENERATOR_PINS, ids=[c[0] for c in GENERATOR_PINS])
def test_generator_without_the_option_is_unchanged(built, tmp_path, mode, w, h, seed, opts, want):
    """written afresh (build/streams caches by options), not read from the cache"""
    out = str(tmp_path / "s.jxl")
    subprocess.run([os.path.join(ROOT, "build", "jxlsynth"), mode, str(w), str(h), str(seed), out] + ["%s=%s" % kv for kv in sorted(opts.items())], check=True, stderr=subprocess.DEVNULL)
    with open(out, "rb") as fp:
        data = fp.read()
    assert hashlib.sha256(data).hexdigest() == want
    assert data == synth(mode, w, h, seed, **opts), "the cache holds the same bytes"


def test_generator_refuses_orientations_outside_1_to_8(built, tmp_path):
    for bad in ("0", "9", "-1"):
        r = subprocess.run([os.path.join(ROOT, "build", "jxlsynth"), "vardct", "40", "24", "1", str(tmp_path / "x.jxl"), "orientation=" + bad, "passes=2"], capture_output=True)
        assert r.returncode != 0, bad
