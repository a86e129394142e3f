"""YCbCr VarDCT frames against real JPEG data: the quantised integers of baseline JPEG files written by a real encoder
(tests/golden/jpeg/NAME.jpg, Pillow / libjpeg; tools/make_jpeg_fixtures.py) go through tools/jxlsynth's jpegdata= into a YCbCr VarDCT
stream, and what this decoder makes of that stream is held against tests/jpeg_ref.py -- a float64 decoder written from the JPEG
definition, itself held against the real decoder's picture (NAME.rgb.npy) -- and against that picture directly.

What this pins that tests/test_ycbcr*.py cannot (they compare the decoder with restatements of itself): which slot is Cb and which Cr,
the upsampling's phase and taps, the 128/255 offset and the matrix constants, which dequantisation matrix a subsampled channel gets and
its orientation (custom_420_264x40 has two tables that are not symmetric), the MCU padding at ragged edges (17 x 9; 40, 264 and 24 of 16), blocks landing
in the right place across a group border (x = 256, y = 256).

What it does not pin ("YCbCr frames"): libjxl's own transcoding conventions. Two things a JPEG decoder does and this decoder
(like the format) does not, both found while writing these tests:
  * the quantisation bias (q - 0.145 / q, q * 0.93..0.95 for |q| = 1) is applied to every VarDCT frame and a frame that is not XYB cannot
    signal another; the streams here carry q times a large integer so that it vanishes below float32's resolution;
  * T.81 clamps every reconstructed sample to [0, 255] before upsampling and conversion, a float pipeline does not. The float64
    reference has both forms; (d) leaves out the pixels where they differ.

Numbers measured on the development machine (manifest.json holds them, the tests assert them):
  (a) max |round(float64, clamp, edge="libjpeg") - Pillow| per fixture, histogram of |delta| = 0, 1, 2, 3 over all samples:
        q90_444_8x8 2 [125, 66, 1]            q75_420_16x16 2 [464, 291, 13]        q75_420_17x9 2 [242, 206, 11]
        q75_422_40x24 2 [1722, 1107, 51]      q30_444_40x24 2 [1893, 978, 9]        q98_420_40x24 2 [1714, 1122, 44]
        custom_420_264x40 2 [20450, 10795, 435]                                     q75_420_24x264 3 [12542, 6201, 264, 1]
      The one 3 is a B sample (float64 235.53, libjpeg 233): libjpeg rounds after its inverse DCT, after upsampling and after the
      conversion, and a chroma error enters B with gain 1.772 -- worst case 1 + 1.772 * 1.5 + 0.5 = 4.2 levels in B, 3.6 in R, 3.1 in G.
      Differences of 2 occur in R and B only, never in G.
  (b) max |float32 plane - float64 plane| over all fixtures, CPU build of the device code: 2.4562e-07 (planes in units of 1/255 of a
      level, values within about [-0.6, 0.6]). Asserted: four times that, 9.8248e-07.
"""
import ctypes as C
import functools
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import jpeg_ref
from streams import ROOT, CACHE

U8X4, U16X4 = 0x0F33, 0x0F35

with open(os.path.join(jpeg_ref.GOLDEN, "manifest.json")) as _fp:
    MANIFEST = json.load(_fp)
FIXTURES = {f["name"]: f for f in MANIFEST["fixtures"]}
NAMES = list(FIXTURES)
PLANE_BOUND = 4 * MANIFEST["plane_max_abs_f32_minus_f64"]
# (c): the plane bound in levels through the conversion's largest row gain (B = Y + 1.772 Cb)
MARGIN = PLANE_BOUND * (1 + 1.772) * 255
WHOLE_MCUS = [n for n, f in FIXTURES.items() if f["width"] % (8 if f["subsampling"] in ("444", "440") else 16) == 0 and f["height"] % (8 if f["subsampling"] in ("444", "422") else 16) == 0]


def test_the_fixture_set_is_the_issues():
    assert NAMES == ["q90_444_8x8", "q75_420_16x16", "q75_420_17x9", "q75_422_40x24", "q30_444_40x24", "q98_420_40x24", "custom_420_264x40", "q75_420_24x264"]
    assert WHOLE_MCUS == ["q90_444_8x8", "q75_420_16x16", "q30_444_40x24"]
    for name, f in FIXTURES.items():
        for ext, key in ((".jpg", "sha256_jpg"), (".rgb.npy", "sha256_rgb_npy")):
            with open(os.path.join(jpeg_ref.GOLDEN, name + ext), "rb") as fp:
                assert hashlib.sha256(fp.read()).hexdigest() == f[key], (name, ext)


# ---------------------------------------------------------------- shared, computed once

@functools.lru_cache(maxsize=None)
def case(name):
    """(parsed file, Pillow's picture, float64 decode with the padded-grid edge rule: (rgb, u8, planes))"""
    if name == "q75_422_40x24_transposed":   # (e): the 4:2:2 file with x and y exchanged, a 24 x 40 4:4:0 picture
        parsed = jpeg_ref.transposed(case("q75_422_40x24")[0])
        return parsed, None, jpeg_ref.decode_f64(parsed, "padded")
    data, rgb = jpeg_ref.fixture(name)
    parsed = jpeg_ref.parse(data)
    return parsed, rgb, jpeg_ref.decode_f64(parsed, "padded")


def stream(name):
    return jpeg_ref.transcoded(case(name)[0], name)


def code4(c):
    c &= 0xffffffff
    return "".join(chr((c >> s) & 0xff) for s in (24, 16, 8, 0)) if c else ""


@pytest.fixture(scope="module")
def sim(built):
    L = C.CDLL(os.path.join(ROOT, "build", "libhostsim_ycbcr.so"))
    L.ycbcr_sim_info.restype = None
    L.ycbcr_sim_info.argtypes = [C.c_char_p, C.c_size_t, C.c_int32, C.c_void_p]
    L.ycbcr_sim_decode.restype = C.c_uint32
    L.ycbcr_sim_decode.argtypes = [C.c_char_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_int32]
    cache = {}

    def decode(name, fmt=U8X4):
        """(planes Cb, Y, Cr as the tail reads them, pixels) of the CPU decode of the fixture's stream with the switch on"""
        if (name, fmt) not in cache:
            data = stream(name)
            a = np.zeros(24, np.int32)
            L.ycbcr_sim_info(data, len(data), 1, a.ctypes.data)
            assert code4(int(a[0])) == "" and int(a[1]) == 1, (name, code4(int(a[0])))
            planes = [np.zeros((int(a[9 + 2 * c]), int(a[8 + 2 * c])), np.float32) for c in range(3)]
            w, h = int(a[14]), int(a[15])
            px = np.zeros((h, w, 4), np.uint16 if fmt == U16X4 else np.uint8)
            code = L.ycbcr_sim_decode(data, len(data), planes[0].ctypes.data, planes[1].ctypes.data, planes[2].ctypes.data, px.ctypes.data, px.strides[0], 1 if fmt == U16X4 else 0)
            assert code4(code) == "", (name, code4(code))
            cache[(name, fmt)] = (planes, px)
        return cache[(name, fmt)]
    return decode


@pytest.fixture(scope="module")
def gpu(built):
    import j40_amd
    assert j40_amd.device_count() > 0, "the gpu tests need a HIP device"
    assert os.environ.get("J40HIP_YCBCR", "") in ("", "0"), "these tests set the switch themselves (and J40HIP_YCBCR in a child process)"
    return j40_amd


# ---------------------------------------------------------------- the checks, for either build

def check_planes(name, planes):
    """(b): each channel's plane against the float64 plane in the decoder's units, (sample - 128) / 255; slots Cb, Y, Cr"""
    parsed, _, (_, _, ref) = case(name)
    worst = 0.0
    for slot, comp in ((0, 1), (1, 0), (2, 2)):
        want = (ref[comp] - 128.0) / 255.0
        assert planes[slot].shape == want.shape and planes[slot].dtype == np.float32, (name, slot, planes[slot].shape, want.shape)
        worst = max(worst, float(np.abs(planes[slot].astype(np.float64) - want).max()))
    print("%s: max |float32 - float64| over the planes = %.4e (bound %.4e)" % (name, worst, PLANE_BOUND))
    assert worst <= PLANE_BOUND, (name, worst)
    return worst


def levels_of(px, fmt):
    """R, G, B on the 8-bit level scale; A is opaque; an 8-bit frame's 16-bit sample is its level times 257"""
    if fmt == U16X4:
        assert px.dtype == np.uint16 and (px[..., 3] == 65535).all() and (px[..., :3] % 257 == 0).all()
        return (px[..., :3] // 257).astype(np.int64)
    assert px.dtype == np.uint8 and (px[..., 3] == 255).all()
    return px[..., :3].astype(np.int64)


def inside_margin(rgb):
    """where the float64 value is within MARGIN of a rounding boundary (v + 0.5 an integer)"""
    frac = (rgb + 0.5) - np.floor(rgb + 0.5)
    return np.minimum(frac, 1.0 - frac) <= MARGIN


def check_pixels(name, px, fmt):
    """(c): within one level of the float64 decode everywhere, equal wherever the float64 value is farther than MARGIN from a rounding
    boundary; at most 4 * MARGIN of the samples are that close (uniform fractions give 2 * MARGIN)"""
    parsed, _, (rgb, u8, _) = case(name)
    got = levels_of(px, fmt)
    assert got.shape == u8.shape
    d = np.abs(got - u8.astype(np.int64))
    unsure = inside_margin(rgb)
    print("%s: %d of %d samples differ from the float64 decode (max %d), %d within %.2e of a boundary" % (name, int((d > 0).sum()), d.size, int(d.max()), int(unsure.sum()), MARGIN))
    assert d.max() <= 1, name
    assert unsure.mean() <= 4 * MARGIN, (name, float(unsure.mean()))
    assert np.array_equal(got[~unsure], u8.astype(np.int64)[~unsure]), "%s: a difference may only come from a value on a rounding boundary" % name
    assert len(np.unique(got.reshape(-1, 3), axis=0)) > 16, "a picture, not a flat field"


def check_against_pillow(name, px, fmt):
    """(d): the decode against what the real JPEG decoder shows, within the rounding (a) recorded for the fixture plus one level --
    wherever T.81's clamp of the reconstructed samples changes nothing (this decoder, a float pipeline, has none)"""
    parsed, pillow, (rgb, _, _) = case(name)
    free = (jpeg_ref.decode_f64(parsed, "padded", clamp=True)[0] == rgb).all(-1)
    assert free.mean() >= 0.9, (name, float(free.mean()))
    d = np.abs(levels_of(px, fmt) - pillow.astype(np.int64))[free]
    print("%s: max |decode - Pillow| = %d over %d of %d pixels" % (name, int(d.max()), int(free.sum()), free.size))
    assert d.max() <= FIXTURES[name]["f64_vs_pillow_max"] + 1, (name, int(d.max()))


# ---------------------------------------------------------------- CPU

@pytest.mark.parametrize("name", NAMES)
def test_a_parser_and_reference_against_the_real_decoder(name):
    """every sample of every fixture: the float64 decode (T.81's clamp, libjpeg's edge rule), rounded, against Pillow's decode of the same
    file, within the maximum recorded for the fixture (the module's docstring has the histograms and why a 3 can occur in B)"""
    data, pillow = jpeg_ref.fixture(name)
    parsed = jpeg_ref.parse(data)
    f = FIXTURES[name]
    assert (parsed.width, parsed.height, parsed.subsampling) == (f["width"], f["height"], f["subsampling"]) and pillow.shape == (f["height"], f["width"], 3)
    _, u8, planes = jpeg_ref.decode_f64(parsed, "libjpeg", clamp=True)
    d = np.abs(u8.astype(np.int64) - pillow.astype(np.int64))
    hist = [int((d == k).sum()) for k in range(int(d.max()) + 1)]
    print("%s: max %d, histogram %s (recorded: max %d, %s)" % (name, d.max(), hist, f["f64_vs_pillow_max"], f["f64_vs_pillow_histogram"]))
    assert d.max() <= f["f64_vs_pillow_max"] <= 3, (name, hist)
    assert (d > 2).sum() * 1000 < d.size and d[..., 1].max() <= 2
    for c in parsed.components:   # the whole-MCU block grid
        assert c.coef.dtype == np.int16 and c.coef.shape == (-(-f["height"] // (8 * parsed.vmax)) * c.v, -(-f["width"] // (8 * parsed.hmax)) * c.h, 8, 8)


def test_a_edge_rules_differ_only_at_a_ragged_edge():
    """edge="padded" and edge="libjpeg" are the same decode but for the picture's last column (row) where a halved component's last
    sample lies inside the block grid AND the last pixel is the odd one of its pair, the one that looks right (down): an even size that
    is no multiple of the MCU (40, 264 and 24 of 16). At 17 x 9 the last pixels look left and up, and the two rules agree"""
    for name in NAMES:
        parsed = case(name)[0]
        a, b = jpeg_ref.decode_f64(parsed, "libjpeg")[0], case(name)[2][0]
        f = FIXTURES[name]
        col = f["subsampling"] in ("420", "422") and f["width"] % 2 == 0 and f["width"] % 16 != 0
        row = f["subsampling"] in ("420", "440") and f["height"] % 2 == 0 and f["height"] % 16 != 0
        assert np.array_equal(a[:-1, :-1], b[:-1, :-1]), name
        assert np.array_equal(a[:-1, -1], b[:-1, -1]) != col and np.array_equal(a[-1, :-1], b[-1, :-1]) != row, (name, col, row)
    assert [n for n in NAMES if not np.array_equal(jpeg_ref.decode_f64(case(n)[0], "libjpeg")[0], case(n)[2][0])] == ["q75_422_40x24", "q98_420_40x24", "custom_420_264x40", "q75_420_24x264"]
    tables = [c.table for c in case("custom_420_264x40")[0].components]
    assert not np.array_equal(tables[0], tables[0].T) and not np.array_equal(tables[1], tables[1].T) and not np.array_equal(tables[0], tables[1])


@pytest.mark.parametrize("name", NAMES)
def test_b_planes_on_the_cpu(sim, name):
    check_planes(name, sim(name)[0])


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("fmt", [U8X4, U16X4], ids=["u8", "u16"])
def test_c_pixels_on_the_cpu(sim, name, fmt):
    check_pixels(name, sim(name, fmt)[1], fmt)


@pytest.mark.parametrize("name", NAMES)
def test_c_the_reference_alone_keeps_the_margin(name):
    """no more than 4 * MARGIN of a fixture's float64 samples lie within MARGIN of a rounding boundary: the equality of (c) is asked of
    nearly every sample"""
    rgb = case(name)[2][0]
    assert inside_margin(rgb).mean() <= 4 * MARGIN, (name, int(inside_margin(rgb).sum()), rgb.size)
    assert 0 < MARGIN < 1e-3


@pytest.mark.parametrize("name", WHOLE_MCUS)
def test_d_the_real_decoders_picture_on_the_cpu(sim, name):
    check_against_pillow(name, sim(name)[1], U8X4)


def test_e_440_by_transposition_on_the_cpu(sim):
    """the 4:2:2 file's data with x and y exchanged is a 24 x 40 4:4:0 picture: its float64 decode is the transposed decode to the bit (a
    check of jpeg_ref.py itself), its stream's decode the transposed decode within one level, and checks (b) and (c) hold for it"""
    t = "q75_422_40x24_transposed"
    parsed, _, (rgb, u8, planes) = case(t)
    assert (parsed.width, parsed.height, parsed.subsampling) == (24, 40, "440")
    want = case("q75_422_40x24")[2]
    assert np.array_equal(rgb, want[0].transpose(1, 0, 2)) and all(np.array_equal(a, b.T) for a, b in zip(planes, want[2]))
    got_planes, got = sim(t)
    check_planes(t, got_planes)
    check_pixels(t, got, U8X4)
    assert np.abs(got.astype(np.int64) - sim("q75_422_40x24")[1].transpose(1, 0, 2).astype(np.int64)).max() <= 1


def test_f_files_outside_the_parsers_scope_raise():
    grey = b"\xff\xd8" + b"\xff\xc0\x00\x0b\x08\x00\x08\x00\x08\x01\x01\x11\x00"
    with pytest.raises(ValueError, match="grey"):
        jpeg_ref.parse(grey)
    data = jpeg_ref.fixture("q90_444_8x8")[0]
    at = data.index(b"\xff\xc0")
    for patch, words in ((b"\xff\xc2", "progressive"), (b"\xff\xc9", "arithmetic"), (b"\xff\xc1", "baseline")):
        with pytest.raises(ValueError, match=words):
            jpeg_ref.parse(data[:at] + patch + data[at + 2:])
    with pytest.raises(ValueError, match="12|bit"):
        jpeg_ref.parse(data[:at + 4] + b"\x0c" + data[at + 5:])
    sos = data.index(b"\xff\xda")
    with pytest.raises(ValueError, match="restart"):
        jpeg_ref.parse(data[:sos] + b"\xff\xdd\x00\x04\x00\x02" + data[sos:])


# ---------------------------------------------------------------- GPU

def staged(gpu, data, fmt=U8X4):
    f = gpu.Frame(data, ycbcr=True)
    try:
        assert f.set_ycbcr(1) == ""
        f.set_output_format(fmt)
        f.upload(0)
        err, px = f.decode_to_host()
        assert err == "", err
        return [f.read_ycbcr(c) for c in range(3)], px
    finally:
        f.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_g_gpu_planes_are_the_cpu_builds(gpu, sim, name):
    """the planes read after a GPU decode are bit-equal to those of the device code built for the host (both builds pass
    -ffp-contract=off), which (b) holds against float64"""
    planes, px = staged(gpu, stream(name))
    want, want_px = sim(name)
    for c in range(3):
        assert planes[c].shape == want[c].shape and np.array_equal(np.ascontiguousarray(planes[c], np.float32).view(np.uint32), want[c].view(np.uint32)), (name, c)
    check_planes(name, [np.ascontiguousarray(p, np.float32) for p in planes])
    assert np.abs(px.astype(np.int64) - want_px.astype(np.int64)).max() <= 1


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("fmt", [U8X4, U16X4], ids=["u8", "u16"])
def test_h_gpu_pixels(gpu, name, fmt):
    err, px = gpu.decode(stream(name), fmt, ycbcr=True)
    assert err == ""
    check_pixels(name, px, fmt)
    if name in WHOLE_MCUS:
        check_against_pillow(name, px, fmt)


@pytest.mark.gpu
def test_i_440_by_transposition_on_the_gpu(gpu):
    t = "q75_422_40x24_transposed"
    planes, px = staged(gpu, stream(t))
    check_planes(t, [np.ascontiguousarray(p, np.float32) for p in planes])
    check_pixels(t, px, U8X4)
    err, other = gpu.decode(stream("q75_422_40x24"), ycbcr=True)
    assert err == "" and np.abs(px.astype(np.int64) - other.transpose(1, 0, 2).astype(np.int64)).max() <= 1


@pytest.mark.gpu
def test_j_ten_function_api_in_a_fresh_process(gpu):
    """a fresh process with J40HIP_YCBCR=1: j40_next_frame + j40_frame_pixels_u8x4 on the ragged 4:2:0 fixture give the bytes of
    j40_amd.decode(..., ycbcr=True)"""
    name = "q75_420_17x9"
    data = stream(name)
    err, want = gpu.decode(data, ycbcr=True)
    assert err == ""
    check_pixels(name, want, U8X4)
    path = os.path.join(CACHE, "jpeg_api_420_17x9.jxl"); out = os.path.join(CACHE, "jpeg_api_420_17x9.npy")
    with open(path, "wb") as fp:
        fp.write(data)
    prog = ("import sys, os\nsys.path.insert(0, %r)\nimport numpy as np, j40_amd\n"
            "img = j40_amd.from_memory(open(%r, 'rb').read())\nassert img.next_frame(), img.error()\n"
            "px = img.frame_pixels_u8x4()[0]\nassert img.error() == ''\nnp.save(%r, px)\nimg.free()\nj40_amd.shutdown()\n" % (ROOT, path, out))
    r = subprocess.run([sys.executable, "-c", prog], env=dict(os.environ, J40HIP_YCBCR="1"), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    assert np.array_equal(np.load(out), want)
    os.remove(out)
