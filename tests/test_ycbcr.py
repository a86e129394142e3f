"""YCbCr VarDCT frames (recompressed JPEGs; j40hip_frame_set_ycbcr, include/j40hip.h) without a GPU: the host parser's geometry of
subsampled frames, the plan, and the device code built for the host (tests/hostsim/ycbcr_sim.cpp: hf_dev.h's subsampled entropy
decode, the pixel stage into planes, ycbcr_dev.h's tail -- the functions k_ycbcr_tail runs).

The reference refuses such frames, so nothing here is pinned to it directly. What is pinned: a 4:4:4 frame's planes are bit-equal to
those of its twin coded without do_ycbcr, which the rest of the suite ties to the reference; the tail against a numpy restatement
(tests/ycbcr_ref.py); a subsampled frame's planes against the 4:4:4 frames of the same pictures."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from streams import ROOT, CACHE
from ycbcr_ref import U8X4, U16X4, SHIFTS, FWD, ycbcr_stream, twin_stream, plane_shapes, check_against_restatement, code4, bits, tail_cases, random_planes


@pytest.fixture(scope="module")
def sim(built):
    L = C.CDLL(os.path.join(ROOT, "build", "libhostsim_ycbcr.so"))
    L.ycbcr_sim_tail.restype = C.c_int32
    L.ycbcr_sim_tail.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_size_t]
    L.ycbcr_sim_info.restype = None
    L.ycbcr_sim_info.argtypes = [C.c_char_p, C.c_size_t, C.c_int32, C.c_void_p]
    L.ycbcr_sim_decode.restype = C.c_uint32
    L.ycbcr_sim_decode.argtypes = [C.c_char_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_int32]
    return L


def info(sim, data, allow=1):
    a = np.zeros(24, np.int32)
    sim.ycbcr_sim_info(data, len(data), allow, a.ctypes.data)
    return dict(parse=code4(int(a[0])), ycbcr=int(a[1]), shifts=tuple((int(a[2 + 2 * c]), int(a[3 + 2 * c])) for c in range(3)),
                planes=[(int(a[9 + 2 * c]), int(a[8 + 2 * c])) for c in range(3)], width=int(a[14]), height=int(a[15]), scope=code4(int(a[16])),
                lf_group=tuple(int(v) for v in a[17:21]), plan_on=code4(int(a[21])), plan_off=code4(int(a[22])))


def decode(sim, data, fmt=U8X4):
    """(code, planes as the tail reads them, pixels) of the CPU decode with the switch on"""
    i = info(sim, data)
    assert i["parse"] == "", i
    planes = [np.zeros(s, np.float32) for s in i["planes"]]
    w, h = i["width"], i["height"]
    px = np.zeros((h, w, 4), np.uint16 if fmt == U16X4 else np.uint8)
    code = sim.ycbcr_sim_decode(data, len(data), planes[0].ctypes.data, planes[1].ctypes.data, planes[2].ctypes.data, px.ctypes.data, px.strides[0], 1 if fmt == U16X4 else 0)
    return code4(code), planes, px


# ---------------------------------------------------------------- the parser's geometry and the switch

def test_geometry_of_subsampled_frames(sim):
    """jpeg_upsampling to shifts (coded order Cb, Y, Cr; 4:2:0 = 4, 4:2:2 = 8, 4:4:0 = 12), the block grid padded to whole MCUs, every
    plane at its channel's resolution; group and LfGroup counts stay the picture's"""
    for sub in ("420", "422", "440"):
        i = info(sim, ycbcr_stream(24, 24, sub))
        assert i["parse"] == "" and i["ycbcr"] == 1 and i["shifts"] == SHIFTS[sub] and i["scope"] == "" and i["plan_on"] == "", (sub, i)
        mh, mv = SHIFTS[sub][0]
        w8, h8 = (4 if mh else 3), (4 if mv else 3)   # 3 blocks padded to 4 along a subsampled axis
        assert i["lf_group"] == (w8, h8, 1, 1)
        assert i["planes"] == [(h8 * 8 >> mv, w8 * 8 >> mh), (h8 * 8, w8 * 8), (h8 * 8 >> mv, w8 * 8 >> mh)] == plane_shapes(24, 24, sub)
    i = info(sim, ycbcr_stream(264, 40, "420"))
    assert i["lf_group"] == (34, 6, 5, 1) and i["planes"] == [(24, 136), (48, 272), (24, 136)]   # 33 x 5 blocks padded to 34 x 6, two groups
    i = info(sim, ycbcr_stream(40, 24))
    assert i["shifts"] == SHIFTS["444"] and i["lf_group"] == (5, 3, 1, 1) and i["planes"] == [(24, 40)] * 3


def test_switch_off_is_todo_as_before(sim):
    """without the switch a subsampled frame fails where it always did -- before its LF image is read -- and a 4:4:4 one at the plan"""
    assert info(sim, ycbcr_stream(24, 24, "420"), allow=0)["parse"] == "TODO"
    assert info(sim, ycbcr_stream(264, 40, "420"), allow=0)["parse"] == "TODO"
    i = info(sim, ycbcr_stream(40, 24), allow=0)
    assert i["parse"] == "" and i["plan_off"] == "TODO" and i["plan_on"] == ""
    i = info(sim, ycbcr_stream(24, 24, "420"))
    assert i["plan_off"] == "TODO" and i["plan_on"] == ""


def test_refusals_with_the_switch_on(sim):
    """still TODO: a subsampled frame with a DCT16 block, one without skip_adapt_lf_smooth, one that signals Gaborish; a grey image"""
    for name, data in (("dct16", ycbcr_stream(40, 24, "420", subdct16=1)), ("smoothing", ycbcr_stream(40, 24, "420", nosmooth=0)),
                       ("gaborish", ycbcr_stream(40, 24, "420", gab=1)), ("grey", ycbcr_stream(40, 24, grey=1)), ("grey 420", ycbcr_stream(40, 24, "420", grey=1))):
        i = info(sim, data)
        assert i["parse"] == "" and i["scope"] == "TODO" and i["plan_on"] == "TODO", (name, i)
        assert decode(sim, data)[0] == "TODO", name
    # layouts jpeg_upsampling can say that are not 4:4:4, 4:2:0, 4:2:2 or 4:4:0 (Y coarser than chroma: 1, 17; Cb and Cr differing: 2, 50)
    # are refused before anything of the frame is read, with the switch on too
    for v in (1, 17, 2, 50, 6):
        assert info(sim, ycbcr_stream(40, 24, jpegup=v))["parse"] == "TODO", v
    assert info(sim, ycbcr_stream(40, 24, jpegup=21))["scope"] == ""   # three equal modes: no subsampling
    # ... each of which is served without what makes it one
    assert decode(sim, ycbcr_stream(40, 24, "420"))[0] == ""
    assert decode(sim, ycbcr_stream(40, 24, gab=1))[0] == ""   # a 4:4:4 frame may signal the filters


def test_geometry_under_the_host_sanitizers(sim):
    """the parse and the plan of the subsampled 24 x 24 and 264 x 40 streams (and their decode on the CPU) as a program of its own
    built with -fsanitize=address,undefined"""
    prog = os.path.join(ROOT, "build", "ycbcr_main_san")
    paths = []
    for k, (w, h, sub) in enumerate(((24, 24, "420"), (264, 40, "420"), (264, 40, "422"), (264, 40, "440"))):
        path = os.path.join(CACHE, "ycbcr_san_%d.jxl" % k)
        with open(path, "wb") as fp:
            fp.write(ycbcr_stream(w, h, sub))
        paths.append(path)
    r = subprocess.run([prog] + paths, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    assert r.stdout.count("code 00000000") == 2 * len(paths)


# ---------------------------------------------------------------- the tail's functions

def test_tail_against_the_restatement(sim):
    """ycbcr_dev.h's chunk function over random planes, every size, layout, format and depth: within one level of the numpy restatement,
    equal wherever no tie decides; bytes outside width x height of a wider destination stay"""
    rng = np.random.default_rng(11)
    for w, h, sub, fmt, bpp in tail_cases():
        planes = random_planes(rng, w, h, sub)
        pb = 8 if fmt == U16X4 else 4
        stride = w * pb + 24
        given = rng.integers(0, 256, (h, stride), dtype=np.uint8)
        out = given.copy()
        dims = np.array([v for p in planes for v in (p.shape[1], p.shape[1], p.shape[0])], np.int32)
        shifts = np.array([v for s in SHIFTS[sub] for v in s], np.int32)
        assert sim.ycbcr_sim_tail(planes[0].ctypes.data, planes[1].ctypes.data, planes[2].ctypes.data, dims.ctypes.data, shifts.ctypes.data, w, h, bpp, 1 if fmt == U16X4 else 0, out.ctypes.data, stride) == 0
        assert np.array_equal(out[:, w * pb:], given[:, w * pb:]), "bytes behind the rows"
        got = np.ascontiguousarray(out[:, :w * pb]).view(np.uint16 if fmt == U16X4 else np.uint8).reshape(h, w, 4)
        check_against_restatement(got, planes, SHIFTS[sub], w, h, bpp, fmt, exact=True)
    small = np.zeros((1, 4), np.float32)
    dims = np.array([4, 4, 1] * 3, np.int32); shifts = np.zeros(6, np.int32); out = np.zeros(64, np.uint8)
    assert sim.ycbcr_sim_tail(small.ctypes.data, small.ctypes.data, small.ctypes.data, dims.ctypes.data, shifts.ctypes.data, 5, 1, 8, 0, out.ctypes.data, 32) == 1   # a plane narrower than the picture


def test_upsampling_taps_and_border():
    """A check of the REFERENCE, not of the product (it passes without the feature): tests/ycbcr_ref.py's restatement on a ramp gives
    the taps the issue writes down -- 0.75 / 0.25, the plane's own border repeated, horizontal before vertical -- so that the tests
    which hold the product against it hold it against the right thing"""
    from ycbcr_ref import upsampled
    a = np.array([[0.0, 4.0, 8.0]], np.float32)
    assert upsampled(a, 1, 0, 6, 1).tolist() == [[0.0, 1.0, 3.0, 5.0, 7.0, 8.0]]
    b = np.array([[0.0], [4.0]], np.float32)
    assert upsampled(b, 0, 1, 1, 4).tolist() == [[0.0], [1.0], [3.0], [4.0]]
    c = np.array([[0.0, 4.0], [8.0, 12.0]], np.float32)
    assert upsampled(c, 1, 1, 4, 4).tolist() == [[0.0, 1.0, 3.0, 4.0], [2.0, 3.0, 5.0, 6.0], [6.0, 7.0, 9.0, 10.0], [8.0, 9.0, 11.0, 12.0]]


# ---------------------------------------------------------------- whole frames on the CPU

@pytest.mark.parametrize("w,h,opts", [(40, 24, dict()), (264, 136, dict(cfl=1, passes=2))], ids=["40x24", "264x136_cfl_two_passes"])
def test_444_planes_equal_the_twin_without_do_ycbcr(sim, w, h, opts):
    """the planes a 4:4:4 YCbCr frame hands its tail are bit-equal to the samples of the same stream coded with noxyb=1 and
    do_ycbcr = 0 ahead of ITS colour conversion: dequantisation, chroma-from-luma and the inverse transforms are any VarDCT frame's"""
    code, planes, _ = decode(sim, ycbcr_stream(w, h, **opts))
    tcode, tplanes, _ = decode(sim, twin_stream(w, h, **opts))
    assert code == tcode == ""
    for c in range(3):
        assert planes[c].shape == (h, w) and np.array_equal(bits(planes[c]), bits(tplanes[c])), c
    assert np.abs(planes[1]).max() > 0.05 and np.abs(planes[0]).max() > 0


@pytest.mark.parametrize("w,h,sub", [(40, 24, "444"), (24, 24, "420"), (264, 40, "420"), (40, 24, "422"), (40, 24, "440")])
@pytest.mark.parametrize("fmt", [U8X4, U16X4], ids=["u8", "u16"])
def test_whole_frame_is_the_restatement_of_its_planes(sim, w, h, sub, fmt):
    code, planes, px = decode(sim, ycbcr_stream(w, h, sub), fmt)
    assert code == ""
    check_against_restatement(px, planes, SHIFTS[sub], w, h, 8, fmt, exact=True)
    assert len(np.unique(px[..., :3])) > 16, "a picture, not a flat field"


def test_subsampled_luma_equals_the_444_stream_of_the_same_picture(sim):
    """flat chroma: the Y plane of the 4:2:0, 4:2:2 and 4:4:0 streams at 264 x 40 is bit-equal to that of the 4:4:4 stream over
    width x height -- the presence rule keeps the entropy decode in step, every Y block lands where it belongs"""
    w, h = 264, 40
    code, want, wpx = decode(sim, ycbcr_stream(w, h, flatchroma=1, **FWD))
    assert code == "" and want[1].std() > 0.01
    for sub in ("420", "422", "440"):
        code, planes, px = decode(sim, ycbcr_stream(w, h, sub, flatchroma=1, **FWD))
        assert code == "", sub
        assert np.array_equal(bits(planes[1][:h, :w]), bits(want[1])), sub
        for c in (0, 2):   # flat planes stay flat through the upsampling: the same pixels too
            assert np.ptp(planes[c]) < 1e-3
        assert np.abs(px.astype(np.int32) - wpx.astype(np.int32)).max() <= 1


@pytest.mark.parametrize("w,h", [(24, 16), (264, 40)])
def test_subsampled_chroma_equals_the_444_stream_of_half_the_size(sim, w, h):
    """the chroma planes of the 4:2:0 stream of 2w x 2h are bit-equal to those of the 4:4:4 stream of w x h (the generator evaluates
    its picture per plane at the plane's own coordinates): the chroma blocks are read at the right places of the stream, with
    non-zero maps of their own, and land at (bx >> 1, by >> 1) of their planes"""
    code, want, _ = decode(sim, ycbcr_stream(w, h, **FWD))
    code2, planes, _ = decode(sim, ycbcr_stream(2 * w, 2 * h, "420", **FWD))
    assert code == code2 == ""
    for c in (0, 2):
        assert want[c].std() > 1e-3
        assert np.array_equal(bits(planes[c][:h, :w]), bits(want[c])), c
