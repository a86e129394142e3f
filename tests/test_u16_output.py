"""16-bit RGBA output (J40_U16X4): the public API, the frame C-ABI and the device's 16-bit pixel kernels.

Every 16-bit sample is pinned to the reference: with bpp the image's bit depth, maxpixel = 2^bpp - 1 and p the reference's int16
level clamped to [0, maxpixel] (alpha: the alpha plane's, clamped the same way),

    u16 = (p * 65535 + 2^(bpp - 1)) / maxpixel

-- the reference's 8-bit render (j40.h:7947-7953) with 255 replaced by 65535. For bit depths 8-16 the map is injective and
p = (u16 * maxpixel + 32767) / 65535 recovers the level; the 8-bit output is then (p * 255 + 2^(bpp - 1)) / maxpixel."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from streams import synth, VARDCT_CASES, MODULAR_CASES, ROOT

GOLDEN = os.path.join(ROOT, "tests", "golden")
U16X4 = 0x0F35


def scale_u16(p, bpp):
    maxpixel = (1 << bpp) - 1
    p = np.clip(np.asarray(p, np.int64), 0, maxpixel)
    return ((p * 65535 + (1 << (bpp - 1))) // maxpixel).astype(np.uint16)


def level_of(u16, bpp):
    maxpixel = (1 << bpp) - 1
    return (u16.astype(np.int64) * maxpixel + 32767) // 65535


def reduce_u8(p, bpp):
    maxpixel = (1 << bpp) - 1
    return ((np.asarray(p, np.int64) * 255 + (1 << (bpp - 1))) // maxpixel).astype(np.uint8)


# ---------------------------------------------------------------- without a GPU

def test_output_format_accepts_u16(built):
    import j40_amd
    assert j40_amd.J40_U16X4 == U16X4
    img = j40_amd.from_memory(synth("vardct", 264, 200, 11))
    assert img.output_format(j40_amd.J40_RGBA, j40_amd.J40_U16X4) == ""
    assert img.error() == ""
    assert img.output_format(j40_amd.J40_RGBA, j40_amd.J40_U8X4) == ""   # (before the first frame: the last call wins)
    img.free()


def test_output_format_refuses_other_formats_and_channels(built):
    import j40_amd
    data = synth("vardct", 264, 200, 11)
    for fmt in (0, 0x0F2B, 0x0F36, 0x0F39, 0x0F34):
        img = j40_amd.from_memory(data)
        assert img.output_format(j40_amd.J40_RGBA, fmt) == "Ufm?", hex(fmt)
        assert "during j40_output_format" in img.error_string()
        img.free()
    for ch in (0x1756, 0x174E, 0):
        img = j40_amd.from_memory(data)
        assert img.output_format(ch, j40_amd.J40_U16X4) == "Uch?", hex(ch)
        img.free()


def test_frame_output_format_setter(built):
    import j40_amd
    fr = j40_amd.Frame(synth("vardct", 264, 200, 11))
    assert fr.output_format() == j40_amd.J40_U8X4
    fr.set_output_format(j40_amd.J40_U16X4)
    assert fr.output_format() == j40_amd.J40_U16X4
    for bad in (0, 0x0F36, -1):
        with pytest.raises(j40_amd.J40Error) as e:
            fr.set_output_format(bad)
        assert e.value.code == "Ufm?"
        assert fr.output_format() == j40_amd.J40_U16X4   # left as it was
    fr.set_output_format(j40_amd.J40_U8X4)
    assert fr.output_format() == j40_amd.J40_U8X4
    fr.close()


def test_pixels_u16x4_structure_and_scaling_rule():
    """j40_pixels_u16x4 is the 24-byte layout of j40_pixels_u8x4; the rule's properties the GPU tests rely on"""
    import j40_amd
    assert C.sizeof(j40_amd._PixelsU16) == 24
    for bpp in range(8, 17):
        maxpixel = (1 << bpp) - 1
        p = np.arange(maxpixel + 1)
        u = scale_u16(p, bpp)
        assert u[0] == 0 and u[-1] == 65535 and np.all(np.diff(u.astype(np.int64)) > 0)   # injective
        assert np.array_equal(level_of(u, bpp), p)
    assert np.array_equal(scale_u16(np.arange(256), 8), np.arange(256) * 257)


def test_u16_image_fails_loudly_without_gpu(built):
    import j40_amd
    if j40_amd.device_count() > 0:
        pytest.skip("a GPU is present")
    data = synth("vardct", 264, 200, 11)
    err, px = j40_amd.decode(data, j40_amd.J40_U16X4)
    assert err == "!gpu" and px is None
    img = j40_amd.from_memory(data)
    assert img.output_format(j40_amd.J40_RGBA, j40_amd.J40_U16X4) == ""
    assert not img.next_frame()
    px16, stride16, _ = img.frame_pixels_u16x4()
    px8, stride8, _ = img.frame_pixels_u8x4()
    assert px16.dtype == np.uint16 and px16.shape == (7, 21, 4) and stride16 == 168
    assert px8.shape == (7, 21, 4) and stride8 == 84
    assert np.array_equal(px16, px8.astype(np.uint16) * 257)
    img.free()


# ---------------------------------------------------------------- on the GPU

@pytest.fixture(scope="module")
def gpu(built):
    import j40_amd
    assert j40_amd.device_count() > 0, "the gpu tests need a HIP device"
    return j40_amd


def ref_planes(ref, data):
    """the reference's int16 planes after combine(): (bpp, [h, w, 3] levels, alpha plane or None); None when the staged decode
    does not take the stream (it mirrors j40__advance for a single regular frame only)"""
    from refdec import RefStage
    try:
        rs = RefStage(ref, data)
    except RuntimeError as e:
        assert "TODO" in str(e)
        return None
    assert rs.combine() == ""
    w, h, bpp = rs.info["width"], rs.info["height"], rs.info["bpp"]
    n = ref.lib.ref_stage_num_planes(rs.h)
    planes = [rs.plane_i16(c)[:h, :w] for c in range(n)]
    rgba8 = rs.rgba()
    rs.close()
    alpha = None
    for c in range(3, n):   # the first extra channel whose render is the reference's alpha (j40.h:7926-7935)
        if planes[c].shape == (h, w) and np.array_equal(reduce_u8(np.clip(planes[c], 0, (1 << bpp) - 1), bpp), rgba8[..., 3]):
            alpha = planes[c]
            break
    if alpha is None:
        assert np.all(rgba8[..., 3] == 255)
    return bpp, np.stack(planes[:3], -1), alpha


def golden(kind):
    manifest = json.load(open(os.path.join(GOLDEN, "manifest.json")))
    return [(n, open(os.path.join(GOLDEN, n + ".jxl"), "rb").read()) for n, e in sorted(manifest.items()) if e["mode"] == kind and "error" not in e]


@pytest.mark.gpu
def test_device_srgb_u16_tail_matches_reference(gpu, ref):
    """j40hip_kat_device_srgb_u16 = the scaling rule on the clamped ref_kat_srgb_i16(v, bpp): exactly on a sample of the values
    against the reference's own line, and on the whole sweep of test_device_srgb_tail_matches_correctly_rounded_powf against
    that line with a correctly rounded powf (the same two-sample allowance for glibc's powf as there)"""
    rng = np.random.default_rng(5)
    v = np.concatenate([np.linspace(0.0, 1.2, 3000001, dtype=np.float32), rng.uniform(0.9, 70000.0, 2000000).astype(np.float32),
                        np.float32(2.0) ** rng.uniform(-20, 120, 500000).astype(np.float32), np.array([np.inf, np.nan, -1.0, 0.0031308, 0.00313081], np.float32)])
    P = np.float64(np.float32(1.0) / np.float32(2.4))
    with np.errstate(all="ignore"):
        p = np.power(v.astype(np.float64), P).astype(np.float32)
        t = np.where(v <= np.float32(0.0031308), np.float32(12.92) * v, np.float32(1.055) * p - np.float32(0.055)).astype(np.float32)
    pick = np.concatenate([rng.choice(v.size, 20000, replace=False), np.arange(v.size - 5, v.size)])
    for bpp in range(8, 16):
        err, out = gpu.kat_device_srgb_u16(v, bpp)
        assert err == ""
        # the reference's own line, value by value
        lv = np.array([ref.lib.ref_kat_srgb_i16(float(v[i]), bpp) for i in pick], np.int64)
        assert np.array_equal(out[pick], scale_u16(lv, bpp)), bpp
        # the whole sweep
        with np.errstate(all="ignore"):
            y = (np.float32((1 << bpp) - 1) * t + np.float32(0.5)).astype(np.float32)
            ok = np.isfinite(y) & (np.abs(y) < 2147483648.0)
            i32 = np.where(ok, np.trunc(np.where(ok, y, 0)).astype(np.int64), -2147483648)
        i16 = ((i32 & 0xFFFF) ^ 0x8000) - 0x8000
        bad = np.nonzero(out != scale_u16(i16, bpp))[0]
        assert bad.size <= 2, (bpp, bad.size, v[bad[:5]])


MODULAR_STREAMS = [("golden_" + n, d) for n, d in golden("modular")] + [(n, (w, h, o)) for n, w, h, o in MODULAR_CASES]


@pytest.mark.gpu
@pytest.mark.parametrize("name,src", MODULAR_STREAMS, ids=[s[0] for s in MODULAR_STREAMS])
def test_modular_u16_bit_exact(gpu, ref, name, src):
    data = src if isinstance(src, bytes) else synth("modular", src[0], src[1], 71, **src[2])
    err, px = gpu.decode(data, gpu.J40_U16X4)
    assert err == "" and px.dtype == np.uint16
    staged = ref_planes(ref, data)
    if staged is None:   # the reference's 8-bit output then pins the levels: exactly for 8-bit images, where u16 = u8 * 257
        rerr, expect = ref.decode(data)
        if rerr != "":   # (streams the reference refuses, Squeeze among them: the library's own bit-exact 8-bit output instead)
            rerr, expect = gpu.decode(data)
        fr = gpu.Frame(data)
        bpp = fr.info["bpp"]
        fr.close()
        assert rerr == "" and np.array_equal(reduce_u8(level_of(px, bpp), bpp), expect)
        if bpp == 8:
            assert np.array_equal(px, expect.astype(np.uint16) * 257)
        return
    bpp, rgb, alpha = staged
    assert np.array_equal(px[..., :3], scale_u16(rgb, bpp))
    assert np.array_equal(px[..., 3], scale_u16(alpha, bpp) if alpha is not None else np.full(px.shape[:2], 65535, np.uint16))
    err8, px8 = gpu.decode(data)
    assert err8 == "" and np.array_equal(px8, reduce_u8(level_of(px, bpp), bpp))


def check_vardct(gpu, ref, data, max_ndiff=None):
    err, px = gpu.decode(data, gpu.J40_U16X4)
    assert err == "" and px.dtype == np.uint16
    staged = ref_planes(ref, data)
    if staged is None:   # (the reference's 8-bit output instead: within one 8-bit level)
        fr = gpu.Frame(data)
        bpp = fr.info["bpp"]
        fr.close()
        rerr, expect = ref.decode(data)
        p = level_of(px[..., :3], bpp)
        assert rerr == "" and np.abs(reduce_u8(p, bpp).astype(np.int32) - expect[..., :3].astype(np.int32)).max() <= 1
    else:
        bpp, rgb, _ = staged
        p = level_of(px[..., :3], bpp)
        check_levels(p, rgb, bpp, px.size, max_ndiff)
    assert np.all(px[..., 3] == 65535)
    err8, px8 = gpu.decode(data)
    assert err8 == "" and np.array_equal(px8[..., :3], reduce_u8(p, bpp)) and np.all(px8[..., 3] == 255)
    return px


def check_levels(p, rgb, bpp, size, max_ndiff):
    d = np.abs(p - np.clip(rgb.astype(np.int64), 0, (1 << bpp) - 1))
    ndiff = int((d > 0).sum())
    assert d.max() <= 1, (d.max(), ndiff)
    assert ndiff <= (max_ndiff if max_ndiff is not None else size // 10000 + 4), ndiff


VARDCT_STREAMS = [(n, (520, 264, o)) for n, o in VARDCT_CASES] + [("golden_" + n, d) for n, d in golden("vardct") if "bit_depth" in n or "forward" in n]


@pytest.mark.gpu
@pytest.mark.parametrize("name,src", VARDCT_STREAMS, ids=[s[0] for s in VARDCT_STREAMS])
def test_vardct_u16_against_reference_levels(gpu, ref, name, src):
    check_vardct(gpu, ref, src if isinstance(src, bytes) else synth("vardct", src[0], src[1], 41, **src[2]))


@pytest.mark.gpu
def test_vardct_u16_8k_frame(gpu, ref):
    check_vardct(gpu, ref, synth("vardct", 7680, 4320, 3), max_ndiff=12000)


@pytest.mark.gpu
def test_u16_device_decode_equals_host_decode(gpu):
    import torch
    for data in (synth("vardct", 520, 264, 41, bpp=12, cfl=1), synth("modular", 600, 300, 71, bpp=10, tree=1)):
        fr = gpu.Frame(data)
        fr.set_output_format(gpu.J40_U16X4)
        fr.upload(0)
        err, host = fr.decode_to_host()
        assert err == "" and host.dtype == np.uint16
        out = torch.zeros((fr.height, fr.width * 8), dtype=torch.uint8, device="cuda:0")
        fr.decode(out.data_ptr(), fr.width * 8, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        assert fr.status() == ""
        dev = out.cpu().numpy().view(np.uint16).reshape(fr.height, fr.width, 4)
        assert np.array_equal(dev, host)
        assert np.array_equal(host, gpu.decode(data, gpu.J40_U16X4)[1])
        fr.close()


def child(code, env_extra, timeout=600):
    env = dict(os.environ, **env_extra)
    prog = "import sys, os\nsys.path.insert(0, %r); sys.path.insert(0, os.path.join(%r, 'tests'))\n" % (ROOT, ROOT) + code
    r = subprocess.run([sys.executable, "-c", prog], env=env, timeout=timeout, capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    return r.stdout


TWO_PHASE_CASES = [(4096, 2304, 72, dict()), (3840, 2160, 13, dict()), (2600, 2100, 71, dict(forward=1))]


@pytest.mark.gpu
def test_u16_two_phase_decode_equals_one_phase(gpu):
    out = os.path.join(ROOT, "build", "u16_one_phase_%d.npy")
    child("""
import numpy as np, j40_amd
from streams import synth
for i, (w, h, seed, opts) in enumerate(CASES):
    fr = j40_amd.Frame(synth("vardct", w, h, seed, **opts)); fr.set_output_format(j40_amd.J40_U16X4); fr.upload(0)
    err, px = fr.decode_to_host()
    assert err == "" and fr.two_phase_sections() == 0, (err, fr.two_phase_sections())
    np.save(OUT % i, px)
""".replace("CASES", repr(TWO_PHASE_CASES)).replace("OUT", repr(out)), {"J40HIP_TWO_PHASE": "0"})
    used = 0
    for i, (w, h, seed, opts) in enumerate(TWO_PHASE_CASES):
        data = synth("vardct", w, h, seed, **opts)
        fr = gpu.Frame(data)
        fr.set_output_format(gpu.J40_U16X4)
        fr.upload(0)
        err, two = fr.decode_to_host()                # into pageable memory: the long sections' rectangles by 2-D copies
        assert err == ""
        used += fr.two_phase_sections() > 0
        fr.close()
        err, api = gpu.decode(data, gpu.J40_U16X4)    # the public API's pinned plane: the rectangles by k_store_group_rects
        assert err == "" and np.array_equal(api, two)
        assert np.array_equal(np.load(out % i), two), (w, h)
    assert used >= 1


@pytest.mark.gpu
def test_u16_dense_fallback_after_evof(gpu, ref):
    out = os.path.join(ROOT, "build", "u16_evof.npy")
    child("""
import numpy as np, torch, j40_amd
from streams import synth
data = synth("vardct", 520, 264, 71)
fr = j40_amd.Frame(data); fr.set_output_format(j40_amd.J40_U16X4); fr.upload(0)
out = torch.zeros((264, 520 * 8), dtype=torch.uint8, device="cuda:0")
fr.decode(out.data_ptr(), 520 * 8, torch.cuda.current_stream().cuda_stream); torch.cuda.synchronize()
assert fr.status() == "evof", fr.status()
err, px = j40_amd.decode(data, j40_amd.J40_U16X4)
assert err == "", err
np.save(OUT, px)
""".replace("OUT", repr(out)), {"J40HIP_EVENTS_PER_BYTE": "0"})
    data = synth("vardct", 520, 264, 71)
    assert np.array_equal(np.load(out), gpu.decode(data, gpu.J40_U16X4)[1])


@pytest.mark.gpu
def test_u16_restoration_mode_2_consistent_with_u8(gpu):
    for w, h, opts in ((264, 200, dict(fullheader=1, gab=1, epf=2, maxlog=3)), (776, 520, dict(fullheader=1, gab=2, epf=3, epfw=1, epfs=1, maxlog=8, bctx=1))):
        data = synth("vardct", w, h, 31, **opts)
        fr = gpu.Frame(data)
        fr.upload(0)
        fr.set_restoration(2)
        err, px8 = fr.decode_to_host()
        assert err == ""
        fr.set_output_format(gpu.J40_U16X4)
        err, px16 = fr.decode_to_host()
        assert err == "" and px16.dtype == np.uint16
        bpp = fr.info["bpp"]
        assert np.array_equal(px8[..., :3], reduce_u8(level_of(px16[..., :3], bpp), bpp)) and np.all(px16[..., 3] == 65535)
        fr.set_restoration(0)
        err, plain16 = fr.decode_to_host()
        assert err == "" and not np.array_equal(plain16, px16)   # the filters did run in the 16-bit decode
        fr.close()


@pytest.mark.gpu
def test_u16_batch_equals_single_frames(gpu):
    import torch
    sizes = [(520, 264, dict()), (776, 520, dict(maxlog=8, bctx=1, presets=2, orders=1)), (264, 200, dict(bpp=12, cfl=1)), (1000, 257, dict(bpp=15))]
    frames, alone = [], []
    for i, (w, h, o) in enumerate(sizes):
        data = synth("vardct", w, h, 50 + i, **o)
        fr = gpu.Frame(data)
        fr.set_output_format(gpu.J40_U16X4)
        fr.upload(0)
        err, px = fr.decode_to_host()
        assert err == ""
        frames.append(fr); alone.append(px)
    outs = [torch.zeros((f.height, f.width * 8), dtype=torch.uint8, device="cuda:0") for f in frames]
    b = gpu.Batch(frames)
    b.decode([o.data_ptr() for o in outs], [f.width * 8 for f in frames], torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    for f, o, px in zip(frames, outs, alone):
        assert f.status() == ""
        assert np.array_equal(o.cpu().numpy().view(np.uint16).reshape(f.height, f.width, 4), px)
    # a stride below 8 * width for a 16-bit member: "rnge", nothing launched
    with pytest.raises(gpu.J40Error) as e:
        b.decode([o.data_ptr() for o in outs], [f.width * 8 - 8 for f in frames], torch.cuda.current_stream().cuda_stream)
    assert e.value.code == "rnge"
    # members that disagree on the format: "Uof?", nothing launched
    frames[1].set_output_format(gpu.J40_U8X4)
    with pytest.raises(gpu.J40Error) as e:
        b.decode([o.data_ptr() for o in outs], [f.width * 8 for f in frames], torch.cuda.current_stream().cuda_stream)
    assert e.value.code == "Uof?"
    b.close()
    for f in frames:
        f.close()


@pytest.mark.gpu
def test_u16_stride_too_small_is_refused(gpu):
    import torch
    L = gpu.lib()
    for data in (synth("vardct", 520, 264, 41), synth("modular", 256, 256, 71)):
        fr = gpu.Frame(data)
        fr.set_output_format(gpu.J40_U16X4)
        fr.upload(0)
        w = fr.width
        out = torch.full((fr.height, w * 8), 7, dtype=torch.uint8, device="cuda:0")
        assert gpu.err4(L.j40hip_frame_decode(fr.h, out.data_ptr(), w * 8 - 1, None)) == "rnge"
        assert gpu.err4(L.j40hip_frame_decode_timed(fr.h, out.data_ptr(), w * 4, None, np.zeros(3, np.float32).ctypes.data)) == "rnge"
        host = np.zeros((fr.height, w * 8), np.uint8)
        assert gpu.err4(L.j40hip_frame_decode_to_host(fr.h, host.ctypes.data, w * 4)) == "rnge"
        torch.cuda.synchronize()
        assert bool((out == 7).all()) and not host.any()   # nothing was written
        fr.close()


@pytest.mark.gpu
def test_u16_public_api_format_rules(gpu):
    data = synth("vardct", 520, 264, 41, bpp=12, cfl=1)
    img = gpu.from_memory(data)
    assert img.output_format(gpu.J40_RGBA, gpu.J40_U16X4) == ""
    assert img.next_frame()
    px, stride, _ = img.frame_pixels_u16x4()
    assert px.shape == (264, 520, 4) and stride == (8 * 520 + 1 + 31) // 32 * 32
    ph, _, _ = img.frame_pixels_u8x4()               # the format that was not decoded: the placeholder and "Ufm?"
    assert ph.shape == (7, 21, 4) and img.error() == "Ufm?"
    assert "during j40_frame_pixels_*" in img.error_string()
    img.free()
    img = gpu.from_memory(data)
    assert img.next_frame()
    assert img.output_format(gpu.J40_RGBA, gpu.J40_U16X4) == "Uof?"   # after the decode: refused, nothing changes
    assert img.error() == "" and img.frame_pixels_u8x4()[0].shape == (264, 520, 4)
    img.free()


@pytest.mark.gpu
def test_u16_public_api_from_threads_while_serving(gpu):
    """several threads through the public API in u16 with J40HIP_SERVE=1 (16-bit images take the single-frame path): the
    pixels of the lone call"""
    out = os.path.join(ROOT, "build", "u16_threads.npy")
    child("""
import threading, numpy as np, j40_amd
from streams import synth
datas = [synth("vardct", 520, 264, 41, bpp=12, cfl=1), synth("modular", 600, 300, 71, bpp=10, tree=1), synth("vardct", 264, 200, 11)]
res = [None] * 9
def call(i):
    res[i] = j40_amd.decode(datas[i % 3], j40_amd.J40_U16X4)
ts = [threading.Thread(target=call, args=(i,)) for i in range(9)]
[t.start() for t in ts]; [t.join() for t in ts]
for i, (e, px) in enumerate(res):
    assert e == "" and px.dtype == np.uint16, (i, e)
    assert np.array_equal(px, res[i % 3][1]), i
np.save(OUT, np.concatenate([res[k][1].reshape(-1) for k in range(3)]))
""".replace("OUT", repr(out)), {"J40HIP_SERVE": "1"})
    lone = [gpu.decode(d, gpu.J40_U16X4)[1] for d in (synth("vardct", 520, 264, 41, bpp=12, cfl=1), synth("modular", 600, 300, 71, bpp=10, tree=1), synth("vardct", 264, 200, 11))]
    assert np.array_equal(np.load(out), np.concatenate([p.reshape(-1) for p in lone]))
