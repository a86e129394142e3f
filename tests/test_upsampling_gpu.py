"""Upsampling on the device (include/j40hip.h, J40HIP_PARSE_UPSAMPLING; k_upsample<2|4|8>). PARITY UNPINNED: the reference refuses every
such frame (j40.h:3297-3306, 5244-5249, 3638), so the feature is pinned piece by piece, every piece bit for bit or byte for byte:
  - the kernel alone (j40hip_kat_device_upsample) against the CPU build of the same functions and numpy's float32 statement of the rule
    (tests/upsample_streams.py), over planes narrower than the halo, one past a tile and a tile's multiple, whole and cut;
  - the planes a decode leaves (j40hip_frame_read_xyb, stage 5) against that statement applied to planes the library makes WITHOUT the
    feature: the same coded frame written with upsampling = 1 (uptwin=1) and decoded alone;
  - the pixels against k_xyb_to_rgba (or k_colour_tail) alone over those expected planes, u8 and u16;
  - the anchor that reaches the reference: with upweights=nearest the picture is np.repeat of the twin's pixels, cut to the shown size,
    and the reference decodes the VarDCT twin at the suite's bar (within one level, A equal).
tests/test_upsampling.py has the switch, the sizes, the refusals at parse and the CPU build."""
import numpy as np
import pytest

import upsample_streams as U
from upsample_streams import up_synth, pair, bits, KAT_SHAPES
from test_scale import box
from test_orient import orient
from test_colour_gpu import tail_inputs
from test_frames_gpu import public_api_frames

pytestmark = pytest.mark.gpu
U8X4, U16X4 = 0x0F33, 0x0F35
GAB = dict(gab=1)     # the VarDCT frames signal Gaborish: a decode with the restoration filters on leaves its planes readable (stages 0 and 1)


@pytest.fixture(scope="module")
def gpu(built):
    import j40_amd
    assert j40_amd.device_count() > 0, "the gpu tests need a HIP device"
    return j40_amd


def cc15(fr):
    m, bias, it, kx, kb = fr.colour_consts()
    return np.concatenate([m.reshape(9), bias, [it, kx, kb]]).astype(np.float32)


def vardct_planes_alone(gpu, data):
    """a one-frame VarDCT stream decoded alone with the filters on: (planes before the filters = what a decode without them makes, after)"""
    fr = gpu.Frame(data)
    fr.set_restoration(1)
    fr.upload(0)
    err, _ = fr.decode_to_host()
    assert err == ""
    before, after = fr.read_xyb(0), fr.read_xyb(1)
    fr.close()
    return before, after


def modular_planes_alone(gpu, data):
    fr = gpu.Frame(data)
    assert fr.set_modular_xyb(1) == ""
    fr.upload(0)
    err, _ = fr.decode_to_host()
    assert err == ""
    planes = fr.read_xyb(0)
    fr.close()
    return planes


def open_up(gpu, data, fmt=U8X4, modular=False, restoration=None, colour=False):
    fr = gpu.Frame(data, upsampling=True)
    if modular:
        assert fr.set_modular_xyb(1) == ""
    if restoration is not None:
        fr.set_restoration(restoration)
    if colour:
        assert fr.set_colour(1) == ""
    fr.set_output_format(fmt)
    fr.upload(0)
    return fr


KINDS = {
    "vardct": dict(mode="vardct", w=U.VW, h=U.VH, more=GAB),
    "modular": dict(mode="modular", w=U.MW, h=U.MH, more={}),
}
_cache = {}


def twin_planes(gpu, kind, restoration=0):
    """the twin's planes from a decode that does not involve the feature (every K's twin is the same coded frame), made once"""
    key = ("own", kind, restoration)
    if key not in _cache:
        K = KINDS[kind]
        twin = pair(K["mode"], K["w"], K["h"], 2, weights=U.centre_heavy(2), **K["more"])[1]
        _cache[key] = vardct_planes_alone(gpu, twin)[1 if restoration else 0] if kind == "vardct" else modular_planes_alone(gpu, twin)
    return _cache[key]


def case(gpu, kind, k, restoration=0):
    """the stream of `kind` coded at 1:k with the centre-heavy weights and a cut shown size, and everything the feature is held against,
    made once: numpy's rule over the twin's planes, and k_xyb_to_rgba's pixels of the result"""
    key = (kind, k, restoration)
    if key in _cache:
        return _cache[key]
    K = KINDS[kind]
    weights = U.centre_heavy(k)
    shown = U.cut_size(k, K["w"], K["h"])
    data, twin = pair(K["mode"], K["w"], K["h"], k, weights=weights, shown=shown, **K["more"])
    own = twin_planes(gpu, kind, restoration)
    want, clamped = U.upsample(own, k, weights, shown[0], shown[1], want_clamped=True)
    fr = gpu.Frame(twin)
    consts = cc15(fr)
    fr.close()
    pixels = {}
    for fmt in (U8X4, U16X4):
        code, px = gpu.kat_device_xyb_to_rgba(want, consts, 8, fmt)
        assert code == ""
        pixels[fmt] = px
    _cache[key] = dict(K, k=k, data=data, twin=twin, own=own, planes=want, pixels=pixels, consts=consts, shown=shown, weights=weights, clamped=clamped / (3.0 * k * k * K["w"] * K["h"]))
    return _cache[key]


# ---------------------------------------------------------------- 1. the kernel alone

@pytest.mark.parametrize("k", [2, 4, 8])
def test_kernel_alone_equals_the_cpu_build(gpu, k):
    """this is a test that fails without the feature: the symbol does not exist. Every known-answer shape, whole and cut on both axes"""
    weights = U.centre_heavy(k)
    for (w, h) in KAT_SHAPES:
        planes = U.kat_planes(w, h)
        code, want = gpu.kat_host_upsample(planes, k, weights)
        assert code == "" and np.array_equal(bits(want), bits(U.upsample(planes, k, weights)))
        code, got = gpu.kat_device_upsample(planes, k, weights)
        assert code == "" and np.array_equal(bits(got), bits(want)), "%d x %d: %d samples differ" % (w, h, int((bits(got) != bits(want)).sum()))
        ow, oh = U.cut_size(k, w, h)
        code, got = gpu.kat_device_upsample(planes, k, weights, ow, oh)
        assert code == "" and got.shape == (3, oh, ow) and np.array_equal(bits(got), bits(want[:, :oh, :ow])), (w, h)
    assert gpu.kat_device_upsample(U.kat_planes(5, 5), k, weights, 5 * k + 1, 5 * k)[0] == "rnge"
    assert gpu.kat_device_upsample(U.kat_planes(5, 5), k, weights[:-1])[0] == "rnge"


@pytest.mark.parametrize("k", [2, 4, 8])
def test_kernel_nearest_repeats_and_flat_stays_flat(gpu, k):
    """nearest: every output is its coded sample. A flat plane under the centre-heavy weights, whose kernels do not sum to 1, stays
    flat: lo = hi, the clamp makes it exact"""
    planes = U.kat_planes(67, 35)
    code, got = gpu.kat_device_upsample(planes, k, U.nearest_table(k))
    assert code == "" and np.array_equal(bits(got), bits(np.repeat(np.repeat(planes, k, axis=1), k, axis=2)))
    flat = np.stack([np.full((35, 67), v, np.float32) for v in (0.0123, 0.4321, -0.2)])
    code, got = gpu.kat_device_upsample(flat, k, U.centre_heavy(k))
    assert code == "" and np.array_equal(bits(got), bits(np.repeat(np.repeat(flat, k, axis=1), k, axis=2)))


# ---------------------------------------------------------------- 2. planes and pixels

@pytest.mark.parametrize("k", [2, 4, 8])
@pytest.mark.parametrize("kind", ["vardct", "modular"])
def test_planes_and_pixels(gpu, kind, k):
    c = case(gpu, kind, k)
    # (the clamp neither vanishes nor swallows the stencil here either. The bound is wider than the known-answer inputs' 1 % .. 50 %:
    # a generated picture has flat runs, where lo = hi and every output counts as clamped whatever the weights are)
    assert 0.01 <= c["clamped"] <= 0.9, c["clamped"]
    fr = open_up(gpu, c["data"], modular=kind == "modular")
    try:
        assert (fr.width, fr.height) == c["shown"] and fr.coded_size() == (c["w"], c["h"])
        err, px = fr.decode_to_host()
        assert err == ""
        got = fr.read_xyb(5)
        assert got.shape == (3, c["shown"][1], c["shown"][0])
        assert np.array_equal(bits(got), bits(c["planes"])), "%d samples differ" % int((bits(got) != bits(c["planes"])).sum())
        assert px.shape == (c["shown"][1], c["shown"][0], 4) and np.array_equal(px, c["pixels"][U8X4])
        if kind == "modular":       # stage 0 keeps the coded size
            assert np.array_equal(bits(fr.read_xyb(0)), bits(c["own"]))
        # two decodes of one handle are identical
        err, again = fr.decode_to_host()
        assert err == "" and np.array_equal(again, px) and np.array_equal(bits(fr.read_xyb(5)), bits(c["planes"]))
    finally:
        fr.close()
    fr = open_up(gpu, c["data"], fmt=U16X4, modular=kind == "modular")
    try:
        err, px16 = fr.decode_to_host()
        assert err == "" and px16.dtype == np.uint16 and np.array_equal(px16, c["pixels"][U16X4])
    finally:
        fr.close()
    # the twin, parsed with the switch: nothing to stretch, stage 5 is not answered
    fr = open_up(gpu, c["twin"], modular=kind == "modular")
    try:
        err, plain = fr.decode_to_host()
        assert err == "" and plain.shape == (c["h"], c["w"], 4)
        with pytest.raises(gpu.J40Error):
            fr.read_xyb(5)
    finally:
        fr.close()
    kw = dict(modular_xyb=True) if kind == "modular" else {}
    err, whole = gpu.decode(c["data"], upsampling=True, **kw)
    assert err == "" and np.array_equal(whole, px)
    assert gpu.decode(c["data"], **kw)[0] == "TODO"


@pytest.mark.parametrize("kind", ["vardct", "modular"])
def test_region_scale_and_orientation(gpu, kind):
    """a region is the crop of the shown-size picture, 1:2 and 1:4 its box mean, an orientation its permutation"""
    c = case(gpu, kind, 2)
    px = c["pixels"][U8X4]
    W, H = c["shown"]
    fr = open_up(gpu, c["data"], modular=kind == "modular")
    try:
        for (x, y, w, h) in ((0, 0, 64, 32), (257, 131, 183, 171), (W - 31, H - 17, 31, 17)):
            x, y = min(x, W - w), min(y, H - h)
            assert fr.set_region(x, y, w, h) == ""
            err, part = fr.decode_to_host()
            assert err == "" and np.array_equal(part, px[y:y + h, x:x + w]), (x, y, w, h)
        assert fr.clear_region() == ""
        for shift in (1, 2):
            assert fr.set_scale(shift) == ""
            err, small = fr.decode_to_host()
            assert err == "" and np.array_equal(small, box(px, shift)), shift
        assert fr.set_scale(0) == ""
    finally:
        fr.close()
    if kind == "vardct":
        err, part = gpu.decode_region(c["data"], 257, 131, 183, 171, upsampling=True)
        assert err == "" and np.array_equal(part, px[131:302, 257:440])
    K = KINDS[kind]
    for o in (3, 6):
        data = pair(K["mode"], K["w"], K["h"], 2, weights=c["weights"], shown=c["shown"], orientation=o, **K["more"])[0]
        fr = open_up(gpu, data, modular=kind == "modular")      # (the option changes no stored pixel)
        try:
            assert fr.set_orientation(1) == ""
            err, turned = fr.decode_to_host()
            assert err == "" and np.array_equal(turned, orient(px, o)), o
        finally:
            fr.close()


def test_restoration_on(gpu):
    """the stretch reads the FILTERED planes: behind the filters, ahead of the tail; stages 0 and 1 keep the coded size"""
    c, plain = case(gpu, "vardct", 2, 1), case(gpu, "vardct", 2, 0)
    assert not np.array_equal(c["own"], plain["own"])
    fr = open_up(gpu, c["data"], restoration=1)
    try:
        err, px = fr.decode_to_host()
        assert err == "" and np.array_equal(bits(fr.read_xyb(5)), bits(c["planes"]))
        assert np.array_equal(px, c["pixels"][U8X4]) and not np.array_equal(px, plain["pixels"][U8X4])
        assert np.array_equal(bits(fr.read_xyb(1)), bits(c["own"])) and np.array_equal(bits(fr.read_xyb(0)), bits(plain["own"]))
    finally:
        fr.close()


@pytest.mark.parametrize("kind", ["vardct", "modular"])
def test_colour_mode(gpu, kind):
    """the signalled colour space: the same planes, k_colour_tail alone over them (Display P3 primaries, PQ)"""
    K = KINDS[kind]
    plain = case(gpu, kind, 2)     # (the encoding changes no coefficient: the planes are the sRGB stream's)
    data = pair(K["mode"], K["w"], K["h"], 2, weights=plain["weights"], shown=plain["shown"], primaries=11, tf=16, **K["more"])[0]
    fr = open_up(gpu, data, modular=kind == "modular", colour=True)
    try:
        err, px = fr.decode_to_host()
        assert err == "" and np.array_equal(bits(fr.read_xyb(5)), bits(plain["planes"]))
        cc, enc, lum, _, bpp, _, _ = tail_inputs(gpu, fr)
        code, want = gpu.kat_device_colour_tail(plain["planes"], cc, enc, lum, bpp, U8X4)
        assert code == "" and np.array_equal(px, want)
        assert not np.array_equal(px, plain["pixels"][U8X4])
    finally:
        fr.close()


# ---------------------------------------------------------------- 3. the anchor that reaches the reference

@pytest.mark.parametrize("k", [2, 4, 8])
@pytest.mark.parametrize("kind", ["vardct", "modular"])
def test_anchor_nearest_is_repeat_of_the_twin(gpu, ref, kind, k):
    K = KINDS[kind]
    shown = U.cut_size(k, K["w"], K["h"])
    data, twin = pair(K["mode"], K["w"], K["h"], k, weights="nearest", shown=shown, **K["more"])
    fr = gpu.Frame(twin)
    if kind == "modular":
        assert fr.set_modular_xyb(1) == ""
    fr.upload(0)
    err, alone = fr.decode_to_host()
    fr.close()
    assert err == "" and alone.shape == (K["h"], K["w"], 4)
    for fmt in (U8X4, U16X4):
        fr = open_up(gpu, data, fmt=fmt, modular=kind == "modular")
        try:
            err, px = fr.decode_to_host()
            assert err == "" and px.shape == (shown[1], shown[0], 4)
            if fmt == U8X4:
                assert np.array_equal(px, U.repeat(alone, k, shown[0], shown[1]))
            else:
                tw = gpu.Frame(twin)
                if kind == "modular":
                    assert tw.set_modular_xyb(1) == ""
                tw.set_output_format(U16X4)
                tw.upload(0)
                err, alone16 = tw.decode_to_host()
                tw.close()
                assert err == "" and np.array_equal(px, U.repeat(alone16, k, shown[0], shown[1]))
        finally:
            fr.close()
    if kind == "vardct":
        rerr, want = ref.decode(twin)
        assert rerr == ""
        d = int(np.abs(alone[..., :3].astype(np.int32) - want[..., :3].astype(np.int32)).max())
        print("against the reference: max |delta| =", d)
        assert d <= 1 and np.array_equal(alone[..., 3], want[..., 3])


# ---------------------------------------------------------------- 4. what is refused, alpha, and the ten functions

def test_alpha_is_dropped_and_kept_alpha_refused(gpu):
    data, twin = pair("vardct", U.VW, U.VH, 2, weights=U.centre_heavy(2), shown=U.cut_size(2, U.VW, U.VH), alpha=1, **GAB)
    fr = open_up(gpu, data)
    try:
        assert fr.set_alpha(1) == "TODO"
        err, px = fr.decode_to_host()
        assert err == "" and (px[..., 3] == 255).all()
        want = U.upsample(vardct_planes_alone(gpu, twin)[0], 2, U.centre_heavy(2), px.shape[1], px.shape[0])
        assert np.array_equal(bits(fr.read_xyb(5)), bits(want))
    finally:
        fr.close()
    assert gpu.decode(data, alpha=True, upsampling=True)[0] == "TODO"


def test_coarser_extra_channels_are_decoded_at_their_own_size_and_dropped(gpu):
    """a 600 x 540 VarDCT frame at 1:2 whose alpha channel has ec_upsampling = 4: ceil(1199 / 4) x ceil(1077 / 4) samples, the groups'
    rectangles halved. Its sections are decoded and checked like any extra channel's, the pixels are those of the same frame with the
    alpha channel at the frame's own factor, A = 255. The same beside upsampling = 1 (ec_upsampling = 2)"""
    w, h, k = 600, 540, 2
    shown = U.cut_size(k, w, h)
    base = dict(upsampling=k, upweights="nearest", upshown="%d,%d" % shown, alpha=1)
    fine, coarse = up_synth("vardct", w, h, **base), up_synth("vardct", w, h, ecup=4, **base)
    assert fine != coarse
    out = []
    for data in (fine, coarse):
        fr = open_up(gpu, data)
        try:
            err, px = fr.decode_to_host()
            assert err == "" and fr.status() == "" and px.shape == (shown[1], shown[0], 4) and (px[..., 3] == 255).all()
            assert fr.set_alpha(1) == "TODO"
            out.append(px)
        finally:
            fr.close()
    assert np.array_equal(out[0], out[1])
    twin_fine, twin_coarse = up_synth("vardct", w, h, uptwin=1, **base), up_synth("vardct", w, h, uptwin=1, ecup=2, **base)
    fr = gpu.Frame(twin_fine)
    fr.upload(0)
    err, want = fr.decode_to_host()
    fr.close()
    assert err == "" and np.array_equal(out[0], U.repeat(want, k, shown[0], shown[1]))
    fr = open_up(gpu, twin_coarse)
    try:
        err, px = fr.decode_to_host()
        assert err == "" and fr.status() == "" and np.array_equal(px, want)
        assert fr.set_alpha(1) == "TODO"          # (a coarser alpha channel is dropped only)
    finally:
        fr.close()
    # a damaged sub-image of the coarser channel is reported, as any extra channel's is
    bad = bytearray(coarse); bad[-40] ^= 0x55
    fr = open_up(gpu, bytes(bad))
    try:
        err, _ = fr.decode_to_host()
        assert err != "" and fr.status() == err, (err, fr.status())
    finally:
        fr.close()


def test_a_flat_frame_stays_flat(gpu):
    """a Modular XYB frame of constant samples under the centre-heavy weights, whose kernels do not sum to 1: lo = hi everywhere, the
    clamp makes every output the coded sample, so the picture is the twin's repeated -- through the decode's own table and planes,
    twice from one handle"""
    for k in (2, 4, 8):
        shown = U.cut_size(k, U.MW, U.MH)
        data, twin = pair("modular", U.MW, U.MH, k, weights=U.centre_heavy(k), shown=shown, range="100,100")
        own = modular_planes_alone(gpu, twin)
        assert all(len(np.unique(own[c])) == 1 for c in range(3))
        fr = open_up(gpu, data, modular=True)
        try:
            for _ in range(2):
                err, px = fr.decode_to_host()
                assert err == ""
                got = fr.read_xyb(5)
                assert all(np.array_equal(bits(got[c]), bits(np.full((shown[1], shown[0]), own[c, 0, 0], np.float32))) for c in range(3))
            assert len(np.unique(px.reshape(-1, 4), axis=0)) == 1
        finally:
            fr.close()
        tw = gpu.Frame(twin)
        assert tw.set_modular_xyb(1) == ""
        tw.upload(0)
        err, alone = tw.decode_to_host()
        tw.close()
        assert err == "" and np.array_equal(px, U.repeat(alone, k, shown[0], shown[1]))


def test_what_an_upsampled_frame_refuses(gpu):
    """a partial group range, a batch and the many-frames LF preview are "TODO" for an upsampled frame; its twin takes all three"""
    import torch
    c = case(gpu, "vardct", 2)
    out = torch.zeros((c["shown"][1], c["shown"][0] * 4), dtype=torch.uint8, device="cuda:0")
    for stream, code in ((c["data"], "TODO"), (c["twin"], "")):
        fr = open_up(gpu, stream)
        try:
            try:
                fr.set_group_range(0, 1)
                got = ""
            except gpu.J40Error as e:
                got = e.code
            assert got == code
            if not code:
                fr.set_group_range(0, 4)     # (every group again)
            try:
                gpu.Batch([fr]).close()
                got = ""
            except gpu.J40Error as e:
                got = e.code
            assert got == code
            assert gpu.frames_decode_lf([fr], [out.data_ptr()], [c["shown"][0] * 4]) == code
            torch.cuda.synchronize()
            err, px = fr.decode_to_host()
            assert err == "" and (not code or np.array_equal(px, c["pixels"][U8X4]))
        finally:
            fr.close()


def test_route_refusals_at_the_decode(gpu):
    """a Modular frame without the Modular XYB switch; a frame that also has noise (a shown-size operation: a follow-up)"""
    c = case(gpu, "modular", 2)
    fr = gpu.Frame(c["data"], upsampling=True)
    try:
        fr.upload(0)
        assert fr.decode_to_host()[0] == "TODO"
        assert fr.set_modular_xyb(1) == ""
        err, px = fr.decode_to_host()
        assert err == "" and np.array_equal(px, c["pixels"][U8X4])
    finally:
        fr.close()
    # a Modular frame with an alpha plane: the plane has the coded size, the tail would read it at the shown one
    data, twin = pair("modular", U.MW, U.MH, 2, alpha=1)
    for stream, code in ((data, "TODO"), (twin, "")):
        fr = gpu.Frame(stream, upsampling=True)
        try:
            assert fr.set_modular_xyb(1) == ""
            fr.upload(0)
            assert fr.decode_to_host()[0] == code
        finally:
            fr.close()
    # a YCbCr plan
    data, twin = pair("vardct", 304, 272, 2, ycbcr=1)
    for stream, code in ((data, "TODO"), (twin, "")):
        fr = gpu.Frame(stream, upsampling=True, ycbcr=True)
        try:
            assert fr.set_ycbcr(1) == ""
            fr.upload(0)
            assert fr.decode_to_host()[0] == code
        finally:
            fr.close()
    # a frame that also has noise
    noisy = up_synth("vardct", U.VW, U.VH, upsampling=2, upweights="nearest", noise="100,200,300,400,500,600,700,1023", **GAB)
    fr = gpu.Frame(noisy, upsampling=True, noise=True)
    try:
        fr.upload(0)
        assert fr.decode_to_host()[0] == "TODO"
    finally:
        fr.close()


def test_public_api(gpu, monkeypatch):
    """J40HIP_UPSAMPLING=1 serves such a stream through the ten functions, at the shown size; without it they say what they always said"""
    c = case(gpu, "vardct", 2)
    monkeypatch.delenv("J40HIP_UPSAMPLING", raising=False)
    frames, err, _ = public_api_frames(gpu, c["data"])
    assert frames == [] and err == "TODO"
    monkeypatch.setenv("J40HIP_UPSAMPLING", "1")
    for fmt in (U8X4, U16X4):
        frames, err, _ = public_api_frames(gpu, c["data"], fmt)
        assert err == "" and len(frames) == 1 and frames[0].shape == (c["shown"][1], c["shown"][0], 4) and np.array_equal(frames[0], c["pixels"][fmt])
    # a pipeline under the variable: its front parse leaves such a frame to the single-frame route, which serves it at the shown size
    # (what it does with a frame that has noise); without the variable the ticket answers "TODO"
    W, H = c["shown"]
    for env, code in (("1", ""), (None, "TODO")):
        if env is None:
            monkeypatch.delenv("J40HIP_UPSAMPLING")
        out = np.zeros((H, W, 4), np.uint8)
        pipe = gpu.Pipeline(device=0, host_threads=2, batch_frames=4, max_in_flight=2, lf_streams="device")
        try:
            t = pipe.submit(c["data"], out.ctypes.data, W * 4, device_output=False)
            pipe.drain()
            assert pipe.result(t) == code
        finally:
            pipe.close()
        assert not code or not out.any()
        assert code or np.array_equal(out, c["pixels"][U8X4])
    monkeypatch.setenv("J40HIP_UPSAMPLING", "1")
    frames, err, _ = public_api_frames(gpu, c["twin"])
    monkeypatch.delenv("J40HIP_UPSAMPLING")
    want, err2, _ = public_api_frames(gpu, c["twin"])
    assert err == err2 == "" and np.array_equal(frames[0], want[0])
