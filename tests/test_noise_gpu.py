"""Photon noise on the device (include/j40hip.h, J40HIP_PARSE_NOISE; k_noise_fill, k_noise_add). PARITY UNPINNED: the reference holds no
code for noise (j40.h:6264), so the feature is pinned piece by piece, every piece bit for bit or byte for byte:
  - the two kernels alone (j40hip_kat_device_noise), raw planes and result, against numpy's float32 statement of the rule
    (tests/noise_streams.py);
  - the planes a decode leaves (j40hip_frame_read_xyb, stage 4) against that statement applied to planes the library makes WITHOUT the
    feature: the same frame written without the flag and the parameters (noisetwin=1) and decoded alone;
  - the pixels against k_xyb_to_rgba (or k_colour_tail) alone over those expected planes;
  - the anchor that reaches the reference: a LUT of eight zeros changes nothing and launches nothing, so the pixels are the twin's, which
    the reference decodes at the suite's bar for VarDCT frames (within one level, A equal).
tests/test_noise.py has the switch, the refusals at parse, the seed counters and the CPU build."""
import numpy as np
import pytest

import noise_streams as N
from noise_streams import noise_synth, pair, lut_text, lut_of, bits, LUT, ZERO
from test_scale import box
from test_orient import orient
from test_colour_gpu import tail_inputs
from test_frames_gpu import public_api_frames
import patch_streams as P

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


def open_noisy(gpu, data, fmt=U8X4, modular=False, restoration=None, colour=False, alpha=False):
    fr = gpu.Frame(data, noise=True)
    if modular:
        assert fr.set_modular_xyb(1) == ""
    if restoration is not None:
        fr.set_restoration(restoration)
    if colour:
        assert fr.set_colour(1) == ""
    if alpha:
        assert fr.set_alpha(1) == ""
    fr.set_output_format(fmt)
    fr.upload(0)
    return fr


KINDS = {
    # (the VarDCT writer's chroma-from-luma base correlations are LfGlobal's defaults, 0 and 1: what the Modular frame has too)
    "vardct": dict(mode="vardct", w=N.VW, h=N.VH, gdim=256, more=GAB),
    "modular": dict(mode="modular", w=N.MW, h=N.MH, gdim=256, more={}),
}
_cache = {}


def case(gpu, kind, restoration=0):
    """the noisy stream of `kind` and its twin, and everything the feature is held against, made once: the twin's planes from a decode
    that does not involve noise, numpy's noise over them, and k_xyb_to_rgba's pixels of the result"""
    key = (kind, restoration)
    if key in _cache:
        return _cache[key]
    K = KINDS[kind]
    data, twin = pair(K["mode"], K["w"], K["h"], **K["more"])
    own = vardct_planes_alone(gpu, twin)[1 if restoration else 0] if kind == "vardct" else modular_planes_alone(gpu, twin)
    raw = N.raw_planes(K["w"], K["h"], K["gdim"], 0, 0)
    want = N.apply_noise(own, lut_of(LUT), 0.0, 1.0, raw=raw)
    assert not np.array_equal(want, own)
    fr = gpu.Frame(twin)
    consts = cc15(fr)
    fr.close()
    pixels = {}
    for fmt in (U8X4, U16X4):
        code, px = gpu.kat_device_xyb_to_rgba(want, consts, 8, fmt)
        assert code == ""
        pixels[fmt] = px
    _cache[key] = dict(K, data=data, twin=twin, own=own, raw=raw, planes=want, pixels=pixels, consts=consts)
    return _cache[key]


# ---------------------------------------------------------------- 1. the kernels alone

@pytest.mark.parametrize("w,h", N.KAT_SHAPES, ids=["%dx%d" % s for s in N.KAT_SHAPES])
def test_kernels_alone_equal_numpy(gpu, w, h):
    """this is a test that fails without the feature: the symbol does not exist. Raw planes and result, bit for bit, for every clipped
    group shape and a frame aligned to the 64 x 32 tile; a LUT that interpolates past 1, and both base correlations off their defaults"""
    rng = np.random.default_rng(w * 1000 + h)
    planes = np.stack([rng.uniform(-0.03, 0.03, (h, w)), rng.uniform(-0.1, 1.3, (h, w)), rng.uniform(-0.1, 1.3, (h, w))]).astype(np.float32)
    raw = N.raw_planes(w, h, N.GDIM, 3, 1)
    for lut, ytox, ytob in ((lut_of(LUT), 0.0, 1.0), (np.array([0.5, 0.9, 1.4, 1.1, 0.2, 1.9, 0.0, 1.3], np.float32), 0.125, 0.75)):
        code, got, got_raw = gpu.kat_device_noise(planes, N.GDIM, lut, ytox, ytob, 3, 1)
        assert code == ""
        assert np.array_equal(bits(got_raw), bits(raw)), "%d raw samples differ" % int((bits(got_raw) != bits(raw)).sum())
        want = N.apply_noise(planes, lut, ytox, ytob, raw=raw)
        assert np.array_equal(bits(got), bits(want)), "%d samples differ" % int((bits(got) != bits(want)).sum())
    # a LUT of zeros: nothing is launched, nothing changes
    code, got, got_raw = gpu.kat_device_noise(planes, N.GDIM, lut_of(ZERO), 0.0, 1.0)
    assert code == "" and np.array_equal(bits(got), bits(planes)) and not got_raw.any()


def test_kernels_hook_refusals_and_seeds(gpu):
    planes = np.zeros((3, 40, 70), np.float32)
    for gdim in (0, 8, 24, 2048):
        assert gpu.kat_device_noise(planes, gdim, lut_of(LUT), 0.0, 1.0)[0] == "rnge"
    a = gpu.kat_device_noise(planes, 16, lut_of(LUT), 0.0, 1.0, 0, 0)[2]
    b = gpu.kat_device_noise(planes, 16, lut_of(LUT), 0.0, 1.0, 1, 0)[2]
    c = gpu.kat_device_noise(planes, 16, lut_of(LUT), 0.0, 1.0, 0, 1)[2]
    assert np.array_equal(bits(a), bits(N.raw_planes(70, 40, 16, 0, 0))) and np.array_equal(bits(b), bits(N.raw_planes(70, 40, 16, 1, 0)))
    assert not np.array_equal(a, b) and not np.array_equal(a, c) and not np.array_equal(b, c)


# ---------------------------------------------------------------- 2. planes and pixels

@pytest.mark.parametrize("kind", ["vardct", "modular"])
def test_planes_and_pixels(gpu, kind):
    c = case(gpu, kind)
    fr = open_noisy(gpu, c["data"], modular=kind == "modular")
    try:
        err, px = fr.decode_to_host()
        assert err == "" and fr.noise_launches() == 1
        got = fr.read_xyb(4)
        assert np.array_equal(bits(got), bits(c["planes"])), "%d samples differ" % int((bits(got) != bits(c["planes"])).sum())
        assert px.shape == (c["h"], c["w"], 4) and np.array_equal(px, c["pixels"][U8X4])
        with pytest.raises(gpu.J40Error):
            fr.read_xyb(3)
        # two decodes of one handle are identical
        err, again = fr.decode_to_host()
        assert err == "" and np.array_equal(again, px) and fr.noise_launches() == 2
        assert np.array_equal(bits(fr.read_xyb(4)), bits(c["planes"]))
        # a region is the crop of the whole, 1:2 and 1:4 are box of the whole
        for (x, y, w, h) in ((0, 0, 64, 32), (57, 31, 83, 71), (c["w"] - 31, c["h"] - 17, 31, 17)):
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
    # the twin, parsed with the switch: no noise, stage 4 is not answered
    fr = open_noisy(gpu, c["twin"], modular=kind == "modular")
    try:
        err, plain = fr.decode_to_host()
        assert err == "" and fr.noise_launches() == 0 and not np.array_equal(plain, px)
        with pytest.raises(gpu.J40Error):
            fr.read_xyb(4)
    finally:
        fr.close()
    kw = dict(modular_xyb=True) if kind == "modular" else {}
    err, whole = gpu.decode(c["data"], noise=True, **kw)
    assert err == "" and np.array_equal(whole, px)
    err, part = gpu.decode_region(c["data"], 57, 31, 83, 71, noise=True) if kind == "vardct" else ("", px[31:102, 57:140])
    assert err == "" and np.array_equal(part, px[31:102, 57:140])
    assert gpu.decode(c["data"], **kw)[0] == "TODO"


@pytest.mark.parametrize("kind", ["vardct", "modular"])
def test_u16_pixels(gpu, kind):
    c = case(gpu, kind)
    fr = open_noisy(gpu, c["data"], fmt=U16X4, modular=kind == "modular")
    try:
        err, px = fr.decode_to_host()
        assert err == "" and px.dtype == np.uint16 and np.array_equal(px, c["pixels"][U16X4])
    finally:
        fr.close()


def test_modular_frame_needs_the_modular_xyb_switch(gpu):
    c = case(gpu, "modular")
    fr = gpu.Frame(c["data"], noise=True)
    try:
        fr.upload(0)
        assert fr.decode_to_host()[0] == "TODO"
        assert fr.set_modular_xyb(1) == ""
        err, px = fr.decode_to_host()
        assert err == "" and np.array_equal(px, c["pixels"][U8X4])
    finally:
        fr.close()


def test_restoration_on(gpu):
    """the noise goes onto the FILTERED planes: after the filters, before the tail"""
    c, plain = case(gpu, "vardct", 1), case(gpu, "vardct", 0)
    assert not np.array_equal(c["own"], plain["own"])
    fr = open_noisy(gpu, c["data"], restoration=1)
    try:
        err, px = fr.decode_to_host()
        assert err == "" and np.array_equal(bits(fr.read_xyb(4)), bits(c["planes"]))
        assert np.array_equal(px, c["pixels"][U8X4]) and not np.array_equal(px, plain["pixels"][U8X4])
    finally:
        fr.close()


@pytest.mark.parametrize("kind", ["vardct", "modular"])
def test_colour_mode(gpu, kind):
    """the signalled colour space: the same planes, k_colour_tail alone over them (Display P3 primaries, PQ)"""
    K = KINDS[kind]
    data, _ = pair(K["mode"], K["w"], K["h"], primaries=11, tf=16, **K["more"])
    plain = case(gpu, kind)     # (the encoding changes no coefficient: the planes are the sRGB stream's)
    fr = open_noisy(gpu, data, modular=kind == "modular", colour=True)
    try:
        err, px = fr.decode_to_host()
        assert err == "" and np.array_equal(bits(fr.read_xyb(4)), bits(plain["planes"]))
        cc, enc, lum, _, bpp, _, _ = tail_inputs(gpu, fr)
        code, want = gpu.kat_device_colour_tail(plain["planes"], cc, enc, lum, bpp, U8X4)
        assert code == "" and np.array_equal(px, want)
        assert not np.array_equal(px, plain["pixels"][U8X4])
    finally:
        fr.close()


# ---------------------------------------------------------------- 3. the anchor that reaches the reference

def test_anchor_a_lut_of_zeros_changes_nothing(gpu, ref):
    data, twin = pair("vardct", N.VW, N.VH, values=ZERO, **GAB)
    assert twin == case(gpu, "vardct")["twin"]
    fr = open_noisy(gpu, data)
    try:
        err, px = fr.decode_to_host()
        assert err == "" and fr.noise_launches() == 0 and fr.noise_params()["lut"].tolist() == [0.0] * 8
        assert np.array_equal(bits(fr.read_xyb(4)), bits(case(gpu, "vardct")["own"]))
    finally:
        fr.close()
    fr = gpu.Frame(twin)
    fr.upload(0)
    err, alone = fr.decode_to_host()
    fr.close()
    assert err == "" and np.array_equal(px, alone)
    rerr, want = ref.decode(twin)
    assert rerr == ""
    d = int(np.abs(alone[..., :3].astype(np.int32) - want[..., :3].astype(np.int32)).max())
    print("against the reference: max |delta| =", d)
    assert d <= 1 and np.array_equal(alone[..., 3], want[..., 3])


# ---------------------------------------------------------------- 4. composition

@pytest.mark.parametrize("o", range(2, 9))
def test_every_orientation_is_the_permutation(gpu, o):
    data, _ = pair("vardct", N.VW, N.VH, orientation=o, **GAB)
    px = case(gpu, "vardct")["pixels"][U8X4]      # (the option changes no stored pixel)
    fr = open_noisy(gpu, data)
    try:
        assert fr.set_orientation(1) == ""
        err, turned = fr.decode_to_host()
        assert err == "" and np.array_equal(turned, orient(px, o))
    finally:
        fr.close()


def test_kept_alpha(gpu):
    """the noise goes onto the colour samples, the kept alpha channel is the twin's"""
    data, twin = pair("vardct", N.VW, N.VH, alpha=1, **GAB)
    out = []
    for stream in (data, twin):
        fr = open_noisy(gpu, stream, alpha=True)
        try:
            err, px = fr.decode_to_host()
            assert err == ""
            out.append((px, fr.read_xyb(4) if stream is data else None))
        finally:
            fr.close()
    (noisy, planes), (plain, _) = out
    assert np.array_equal(noisy[..., 3], plain[..., 3]) and len(np.unique(plain[..., 3])) > 1
    want = N.apply_noise(vardct_planes_alone(gpu, twin)[0], lut_of(LUT), 0.0, 1.0, gdim=256)
    assert np.array_equal(bits(planes), bits(want))
    fr = gpu.Frame(twin)
    code, rgb = gpu.kat_device_xyb_to_rgba(want, cc15(fr), 8, U8X4)
    fr.close()
    assert code == "" and np.array_equal(noisy[..., :3], rgb[..., :3])


def test_a_replace_patch_lies_under_the_noise(gpu):
    """the order: filters, patches, noise, tail. A reference-only frame, then a frame with one Replace patch and noise: its planes are
    numpy's noise over numpy's patches over the twin's planes; its counters are (0, 1), behind one frame that is not shown"""
    refs = [(1, 2, 3, 100, 24, [(70, 40, P.REPLACE, 0)])]
    opts = P.seq_opts("v", refs, [P.REF_V], ["v"], noise=";" + lut_text(LUT), **GAB)
    data = noise_synth("vardct", N.VW, N.VH, **opts)
    seq = gpu.Sequence(data, patches=True, noise=True)
    try:
        seq.upload(0)
        err, px = seq.next_to_host()
        assert err == "" and seq.status() == ("", -1)
        fr = seq.frame(1)
        assert fr.noise_params()["seeds"] == (0, 1) and fr.noise_launches() == 1 and seq.frame_patches(1)["launches"] == 1
        planes = fr.read_xyb(4)
        slot = seq.read_ref_slot(1)
        with pytest.raises(gpu.J40Error):
            fr.read_xyb(3)
    finally:
        seq.close()
    twin = noise_synth("vardct", N.VW, N.VH, **dict(opts, only=1, patchtwin=1, noisetwin=1))
    own = vardct_planes_alone(gpu, twin)[0]
    patched = P.apply_patches(own, {1: slot}, P.flat(refs))
    want = N.apply_noise(patched, lut_of(LUT), 0.0, 1.0, gdim=256, visible=0, nonvisible=1)
    assert np.array_equal(bits(planes), bits(want))
    assert not np.array_equal(bits(want), bits(P.apply_patches(N.apply_noise(own, lut_of(LUT), 0.0, 1.0, gdim=256, visible=0, nonvisible=1), {1: slot}, P.flat(refs))))
    fr = gpu.Frame(twin)
    code, pixels = gpu.kat_device_xyb_to_rgba(want, cc15(fr), 8, U8X4)
    fr.close()
    assert code == "" and np.array_equal(px, pixels)


def test_two_shown_frames_get_different_fields_and_a_rewind_replays_them(gpu):
    """two frames with the same picture (the writer's seed moves with the frame: the fields are compared through their twins)"""
    per = lut_text(LUT) + ";" + lut_text(LUT)
    opts = dict(frames=2, anim=1, **GAB)
    data, twin = noise_synth("vardct", N.VW, N.VH, noise=per, **opts), noise_synth("vardct", N.VW, N.VH, noise=per, noisetwin=1, **opts)
    seq = gpu.Sequence(data, noise=True)
    plain = gpu.Sequence(twin)
    try:
        seq.upload(0); plain.upload(0)
        shown = [seq.next_to_host() for _ in range(2)]
        assert [e for e, _ in shown] == ["", ""] and seq.status() == ("", -1)
        fields = []
        for k in range(2):
            assert seq.frame(k).noise_params()["seeds"] == (k, 0)
            own = vardct_planes_alone(gpu, noise_synth("vardct", N.VW, N.VH, noise=per, noisetwin=1, only=k, **opts))[0]
            got = seq.frame(k).read_xyb(4)
            assert np.array_equal(bits(got), bits(N.apply_noise(own, lut_of(LUT), 0.0, 1.0, gdim=256, visible=k, nonvisible=0))), k
            fields.append(got - own)
        assert not np.array_equal(fields[0], fields[1]) and abs(np.corrcoef(fields[0][1].ravel(), fields[1][1].ravel())[0, 1]) < 0.05
        seq.rewind()
        again = [seq.next_to_host() for _ in range(2)]
        assert all(e == "" and np.array_equal(a, b) for (e, a), (_, b) in zip(again, shown))
        assert not np.array_equal(shown[0][1], plain.next_to_host()[1])
    finally:
        seq.close(); plain.close()
    frames, _ = gpu.decode_frames(data, noise=True)
    assert len(frames) == 2 and all(np.array_equal(f[0], s[1]) for f, s in zip(frames, shown))


@pytest.mark.parametrize("blend", [1, 2, 4], ids=["add", "blend", "mul"])
def test_a_blended_noisy_crop_composes_as_ever(gpu, blend):
    """a full frame saved into slot 0, then a noisy crop blended onto it: the canvas is what the composition makes of the crop's own
    (noisy) pixels, whatever the mode"""
    from test_blend import blend_expected
    x0, y0, w, h = 20, 10, 264, 200
    opts = dict(frames=2, crops=";%d,%d,%d,%d" % (x0, y0, w, h), saves="0,0", srcs="0,0", blends="0,%d" % blend, noise=";" + lut_text(LUT), alpha=1 if blend == 2 else 0, **GAB)
    data = noise_synth("vardct", N.VW, N.VH, **opts)
    seq = gpu.Sequence(data, blend=True, noise=True)
    try:
        seq.upload(0)
        err, px = seq.next_to_host()
        assert err == "" and seq.status() == ("", -1)
        err, under = seq.frame(0).decode_to_host()
        assert err == ""
        err, own = seq.frame(1).decode_to_host()
        assert err == "" and own.shape == (h, w, 4) and seq.frame(1).noise_launches() == 2
        info = seq.frame_blend(1)
    finally:
        seq.close()
    assert info["blended"] == 1
    assert np.array_equal(px, blend_expected(under, own, N.VW, N.VH, x0, y0, 4, False, info["mode"], info["alpha_mode"]))


# ---------------------------------------------------------------- 5. what is refused, and the ten functions

def test_what_a_frame_with_noise_refuses(gpu):
    """a partial group range, a batch and the many-frames LF preview are "TODO" for a frame with noise; its twin takes all three"""
    import torch
    c = case(gpu, "vardct")
    out = torch.zeros((c["h"], c["w"] * 4), dtype=torch.uint8, device="cuda:0")
    for stream, code in ((c["data"], "TODO"), (c["twin"], "")):
        fr = open_noisy(gpu, stream)
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
            assert gpu.frames_decode_lf([fr], [out.data_ptr()], [c["w"] * 4]) == code
            torch.cuda.synchronize()
            err, px = fr.decode_to_host()
            assert err == "" and (not code or np.array_equal(px, c["pixels"][U8X4]))
        finally:
            fr.close()


def test_public_api(gpu, monkeypatch):
    """J40HIP_NOISE=1 serves such a stream through the ten functions; without it they say what they always said"""
    c = case(gpu, "vardct")
    monkeypatch.delenv("J40HIP_NOISE", raising=False)
    frames, err, _ = public_api_frames(gpu, c["data"])
    assert frames == [] and err == "TODO"
    monkeypatch.setenv("J40HIP_NOISE", "1")
    for fmt in (U8X4, U16X4):
        frames, err, _ = public_api_frames(gpu, c["data"], fmt)
        assert err == "" and len(frames) == 1 and np.array_equal(frames[0], c["pixels"][fmt])
    frames, err, _ = public_api_frames(gpu, c["twin"])
    monkeypatch.delenv("J40HIP_NOISE")
    want, err2, _ = public_api_frames(gpu, c["twin"])
    assert err == err2 == "" and np.array_equal(frames[0], want[0])
