"""YCbCr VarDCT frames (recompressed JPEGs) on the GPU: j40hip_frame_set_ycbcr / J40HIP_YCBCR, j40_amd.decode(..., ycbcr=True),
k_ycbcr_tail (device/ycbcr_kernels.hip) and the subsampled forms of the entropy and pixel kernels. tests/test_ycbcr.py holds the same
properties against the device code built for the host; tests/ycbcr_ref.py the numpy restatement of the tail.

The reference refuses such frames (j40.h:7867, 6749): the feature is opt-in and PARITY UNPINNED past the inverse transforms. What ties
it down: with the switch off everything is "TODO" as before; a 4:4:4 frame's planes are bit-equal to those of its twin coded without
do_ycbcr (read with j40hip_frame_read_xyb ahead of ITS colour conversion), which the rest of the suite holds against the
reference; the tail kernel against the restatement; subsampled frames against the 4:4:4 frames of the same pictures. The +-1 on
pixels is the project's VarDCT pixel tolerance."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from streams import ROOT, CACHE
from ycbcr_ref import U8X4, U16X4, SHIFTS, FWD, ycbcr_stream, twin_stream, plane_shapes, check_against_restatement, tail_cases, random_planes, bits, code4


@pytest.fixture(scope="module")
def gpu(built):
    import j40_amd
    assert j40_amd.device_count() > 0, "the gpu tests need a HIP device"
    assert os.environ.get("J40HIP_YCBCR", "") in ("", "0"), "these tests set the switch themselves (and J40HIP_YCBCR in a child process)"
    return j40_amd


def staged(gpu, data, fmt=U8X4, restoration=0):
    """(code, planes as the tail read them, pixels, what j40hip_frame_ycbcr says) of a decode through the thin C-ABI with the switch on"""
    f = gpu.Frame(data, ycbcr=True)
    try:
        assert f.set_ycbcr(1) == ""
        f.set_output_format(fmt)
        f.set_restoration(restoration)
        f.upload(0)
        err, px = f.decode_to_host()
        if err:
            return err, None, None, f.ycbcr()
        return "", [f.read_ycbcr(c) for c in range(3)], px, f.ycbcr()
    except gpu.J40Error as e:
        return e.code, None, None, None
    finally:
        f.close()


# 1
@pytest.mark.gpu
def test_switch_off_is_todo_as_before(gpu):
    """no switch, no environment: a ycbcr=1 stream, 4:4:4 or 4:2:0, is "TODO" from the ten-function API (which is what j40_amd.decode
    goes through) and from the thin C-ABI, where the 4:2:0 one fails in its parse and the 4:4:4 one at the upload, as ever"""
    for data in (ycbcr_stream(40, 24), ycbcr_stream(24, 24, "420"), ycbcr_stream(264, 40, "420")):
        err, px = gpu.decode(data)
        assert err == "TODO" and px is None
        err, px = gpu.decode(data, U16X4)
        assert err == "TODO"
    with pytest.raises(gpu.J40Error) as e:
        gpu.Frame(ycbcr_stream(24, 24, "420"))
    assert e.value.code == "TODO"
    f = gpu.Frame(ycbcr_stream(40, 24))
    assert f.ycbcr() == {"ycbcr": 1, "shifts": SHIFTS["444"], "used": 0}
    with pytest.raises(gpu.J40Error) as e:
        f.upload(0)
    assert e.value.code == "TODO"
    assert f.set_ycbcr(0) == ""
    with pytest.raises(gpu.J40Error):
        f.upload(0)
    f.close()
    f = gpu.Frame(ycbcr_stream(24, 24, "420"), ycbcr=True)   # parsed for YCbCr, but not asked to serve it
    assert f.ycbcr()["shifts"] == SHIFTS["420"]
    with pytest.raises(gpu.J40Error) as e:
        f.upload(0)
    assert e.value.code == "TODO"
    f.close()


# 2
@pytest.mark.gpu
@pytest.mark.parametrize("w,h,opts", [(40, 24, dict(gab=1)), (264, 136, dict(gab=1, cfl=1, passes=2))], ids=["40x24", "264x136_all_transforms_cfl_two_passes"])
def test_444_planes_equal_the_twin_without_do_ycbcr(gpu, w, h, opts):
    """stream S (ycbcr=1) and its twin S0 (the same options, noxyb=1, do_ycbcr = 0): the planes S hands k_ycbcr_tail are bit-equal to
    what the pixel kernels leave of S0 ahead of its colour conversion (j40hip_frame_read_xyb, stage 0; the streams signal Gaborish so
    that the twin's decode with the filters on leaves its planes) -- and with the filters on for S too, to the twin's filtered planes"""
    s, s0 = ycbcr_stream(w, h, **opts), twin_stream(w, h, **opts)
    f0 = gpu.Frame(s0)
    f0.set_restoration(1); f0.upload(0)
    err, _ = f0.decode_to_host()
    assert err == ""
    want, want_filtered = f0.read_xyb(0), f0.read_xyb(1)
    f0.close()
    err, planes, px, st = staged(gpu, s)
    assert err == "" and st["used"] == 1 and st["ycbcr"] == 1
    for c in range(3):
        assert planes[c].shape == (h, w) and np.array_equal(bits(planes[c]), bits(want[c])), c
    check_against_restatement(px, planes, SHIFTS["444"], w, h, 8, U8X4, exact=False)
    err, planes, px, _ = staged(gpu, s, restoration=1)
    assert err == ""
    for c in range(3):
        assert np.array_equal(bits(planes[c]), bits(want_filtered[c])), c
    check_against_restatement(px, planes, SHIFTS["444"], w, h, 8, U8X4, exact=False)


# 3
@pytest.mark.gpu
def test_tail_kernel_known_answers(gpu):
    """k_ycbcr_tail alone (j40hip_kat_device_ycbcr_tail) on random planes: sizes 1 x 1, 7 x 5, 33 x 17, 264 x 9, every layout, both
    formats, bpp 8 and 12. Within one level of the numpy restatement everywhere, EQUAL wherever the restatement's scaled value is
    farther than 1e-3 from a rounding boundary; bytes outside width x height of a wider destination stay. Destinations on a 16-byte
    boundary (the kernel's wide stores) and off it (pixel by pixel)"""
    import torch
    L = gpu.lib()
    rng = np.random.default_rng(12)
    stream = torch.cuda.current_stream().cuda_stream
    for k, (w, h, sub, fmt, bpp) in enumerate(tail_cases()):
        planes = random_planes(rng, w, h, sub)
        assert [p.shape for p in planes] == plane_shapes(w, h, sub)
        pb = 8 if fmt == U16X4 else 4
        stride = w * pb + (32 if k % 2 else 24)
        lead = 0 if k % 2 else pb   # even cases: rows off the 16-byte boundary
        given = rng.integers(0, 256, (h, stride), dtype=np.uint8)
        flat = torch.zeros(h * stride + 64, dtype=torch.uint8, device="cuda:0")
        base = (-flat.data_ptr()) % 16 + lead
        flat[base:base + h * stride] = torch.from_numpy(given.reshape(-1)).to("cuda:0")
        d_planes = [torch.from_numpy(p).to("cuda:0") for p in planes]
        ptrs = (C.c_void_p * 3)(*[p.data_ptr() for p in d_planes])
        dims = (C.c_int32 * 9)(*[v for p in planes for v in (p.shape[1], p.shape[1], p.shape[0])])
        shifts = (C.c_int32 * 6)(*[v for s in SHIFTS[sub] for v in s])
        assert L.j40hip_kat_device_ycbcr_tail(ptrs, dims, shifts, w, h, bpp, fmt, flat.data_ptr() + base, stride, stream) == 0
        torch.cuda.synchronize()
        out = flat.cpu().numpy()[base:base + h * stride].reshape(h, stride)
        assert np.array_equal(out[:, w * pb:], given[:, w * pb:]), "bytes behind the rows"
        assert np.array_equal(flat.cpu().numpy()[:base], np.zeros(base, np.uint8)) and not flat.cpu().numpy()[base + h * stride:].any(), "bytes around the image"
        got = np.ascontiguousarray(out[:, :w * pb]).view(np.uint16 if fmt == U16X4 else np.uint8).reshape(h, w, 4)
        check_against_restatement(got, planes, SHIFTS[sub], w, h, bpp, fmt, exact=True)
    ptrs = (C.c_void_p * 3)(256, 256, 256); dims = (C.c_int32 * 9)(4, 4, 1, 4, 4, 1, 4, 4, 1); shifts = (C.c_int32 * 6)(0, 0, 0, 0, 0, 0)
    assert code4(L.j40hip_kat_device_ycbcr_tail(ptrs, dims, shifts, 5, 1, 8, U8X4, 256, 64, None)) == "rnge"    # a plane narrower than the picture
    assert code4(L.j40hip_kat_device_ycbcr_tail(ptrs, dims, shifts, 4, 1, 16, U8X4, 256, 64, None)) == "rnge"   # bpp
    assert code4(L.j40hip_kat_device_ycbcr_tail(ptrs, dims, shifts, 4, 1, 8, 0x0F34, 256, 64, None)) == "Ufm?"


# 4
WHOLE = [(40, 24, "444"), (24, 24, "420"), (264, 40, "420"), (40, 24, "422"), (40, 24, "440")]


@pytest.mark.gpu
@pytest.mark.parametrize("w,h,sub", WHOLE, ids=["%s_%dx%d" % (s, w, h) for w, h, s in WHOLE])
@pytest.mark.parametrize("fmt", [U8X4, U16X4], ids=["u8", "u16"])
def test_whole_frame_is_the_restatement_of_its_planes(gpu, w, h, sub, fmt):
    """j40_amd.decode(..., ycbcr=True) against the numpy restatement run on the planes of the staged hook: within +-1; the planes have
    the padded grid's size at each channel's resolution"""
    data = ycbcr_stream(w, h, sub)
    err, planes, px, st = staged(gpu, data, fmt)
    assert err == "" and st == {"ycbcr": 1, "shifts": SHIFTS[sub], "used": 1}
    assert [p.shape for p in planes] == plane_shapes(w, h, sub)
    err, got = gpu.decode(data, fmt, ycbcr=True)
    assert err == "" and got.shape == (h, w, 4) and np.array_equal(got, px)
    check_against_restatement(got, planes, SHIFTS[sub], w, h, 8, fmt, exact=False)
    assert len(np.unique(got[..., :3])) > 16, "a picture, not a flat field"


# 5 (a)
@pytest.mark.gpu
def test_subsampled_luma_equals_the_444_stream_of_the_same_picture(gpu):
    w, h = 264, 40
    err, want, wpx, _ = staged(gpu, ycbcr_stream(w, h, flatchroma=1, **FWD))
    assert err == "" and want[1].std() > 0.01
    for sub in ("420", "422", "440"):
        err, planes, px, _ = staged(gpu, ycbcr_stream(w, h, sub, flatchroma=1, **FWD))
        assert err == "", sub
        assert np.array_equal(bits(planes[1][:h, :w]), bits(want[1])), sub
        assert np.abs(px.astype(np.int32) - wpx.astype(np.int32)).max() <= 1


# 5 (b)
@pytest.mark.gpu
@pytest.mark.parametrize("w,h", [(24, 16), (264, 40)])
def test_subsampled_chroma_equals_the_444_stream_of_half_the_size(gpu, w, h):
    err, want, _, _ = staged(gpu, ycbcr_stream(w, h, **FWD))
    err2, planes, _, _ = staged(gpu, ycbcr_stream(2 * w, 2 * h, "420", **FWD))
    assert err == err2 == ""
    for c in (0, 2):
        assert want[c].std() > 1e-3
        assert np.array_equal(bits(planes[c][:h, :w]), bits(want[c])), c


# kept alpha (j40hip_frame_set_alpha) through the YCbCr path
@pytest.mark.gpu
@pytest.mark.parametrize("sub", ["444", "420"])
def test_kept_alpha_is_merged_into_the_ycbcr_pixels(gpu, sub):
    """a ycbcr=1 alpha=1 stream of two groups: with alpha kept R, G, B are those of the opaque decode and A is the A the keep-mode
    decode of the twin without do_ycbcr gives (the same alpha sub-images; tests/test_alpha.py pins that one to the reference's plane)"""
    w, h = 264, 40
    # (alpharange=1: alpha samples that are a function of the position alone, so that both streams carry the same channel)
    data = ycbcr_stream(w, h, sub, alpha=1, alpharange=1)
    twin = twin_stream(w, h, alpha=1, alpharange=1)
    f0 = gpu.Frame(twin)
    assert f0.set_alpha(1) == ""
    f0.upload(0)
    err, want = f0.decode_to_host()
    f0.close()
    assert err == "" and len(np.unique(want[..., 3])) > 16
    for fmt in (U8X4, U16X4):
        err, opaque = gpu.decode(data, fmt, ycbcr=True)
        assert err == "" and (opaque[..., 3] == (65535 if fmt == U16X4 else 255)).all()
        err, kept = gpu.decode(data, fmt, alpha=True, ycbcr=True)
        assert err == "" and np.array_equal(kept[..., :3], opaque[..., :3])
        a = want[..., 3].astype(np.uint16) * 257 if fmt == U16X4 else want[..., 3]
        assert np.array_equal(kept[..., 3], a)


# 6
@pytest.mark.gpu
def test_refusals_with_the_switch_on(gpu):
    """a subsampled stream with a DCT16 block, one without skip_adapt_lf_smooth, one with Gaborish signalled, a grey YCbCr image: "TODO";
    and the entries that keep refusing YCbCr frames: a region, a scale, a group range, a batch"""
    for name, data in (("dct16", ycbcr_stream(40, 24, "420", subdct16=1)), ("smoothing", ycbcr_stream(40, 24, "420", nosmooth=0)),
                       ("gaborish", ycbcr_stream(40, 24, "420", gab=1)), ("grey", ycbcr_stream(40, 24, grey=1))):
        err, px = gpu.decode(data, ycbcr=True)
        assert err == "TODO" and px is None, name
    data = ycbcr_stream(264, 40)
    f = gpu.Frame(data, ycbcr=True)
    assert f.set_ycbcr(1) == ""
    f.upload(0)
    assert f.decode_to_host()[0] == ""
    assert f.set_region(8, 8, 16, 16) == "" and f.decode_to_host()[0] == "TODO"
    assert f.clear_region() == "" and f.set_scale(1) == "" and f.decode_to_host()[0] == "TODO"
    assert f.set_scale(0) == ""
    f.set_group_range(0, 1)
    assert f.decode_to_host()[0] == "TODO"
    f.set_group_range(0, 2)
    assert f.decode_to_host()[0] == ""
    err = C.c_uint32()
    frames = (C.c_void_p * 1)(f.h)
    assert not gpu.lib().j40hip_batch_create(frames, 1, C.byref(err)) and code4(err.value) == "TODO"
    assert f.set_ycbcr(0) == "" and f.decode_to_host()[0] == "TODO"   # the switch taken back: nothing is served any more
    f.close()


# 7
@pytest.mark.gpu
def test_ten_function_api_follows_the_environment(gpu):
    """a fresh process with J40HIP_YCBCR=1: j40_next_frame + j40_frame_pixels_u8x4 on the 4:2:0 24 x 24 stream give the pixels of
    j40_amd.decode(..., ycbcr=True)"""
    data = ycbcr_stream(24, 24, "420")
    err, want = gpu.decode(data, ycbcr=True)
    assert err == ""
    path = os.path.join(CACHE, "ycbcr_api_420.jxl"); out = os.path.join(CACHE, "ycbcr_api_420.npy")
    with open(path, "wb") as fp:
        fp.write(data)
    prog = ("import sys, os\nsys.path.insert(0, %r)\nimport numpy as np, j40_amd\n"
            "img = j40_amd.from_memory(open(%r, 'rb').read())\nassert img.next_frame(), img.error()\n"
            "px = img.frame_pixels_u8x4()[0]\nassert img.error() == ''\nnp.save(%r, px)\nimg.free()\nj40_amd.shutdown()\n" % (ROOT, path, out))
    r = subprocess.run([sys.executable, "-c", prog], env=dict(os.environ, J40HIP_YCBCR="1"), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    assert np.array_equal(np.load(out), want)
    os.remove(out)
