"""Splines on the device (include/j40hip.h, J40HIP_PARSE_SPLINES; k_spline_draw). PARITY UNPINNED: the reference holds no code for
splines (j40.h:6263), so the feature is pinned piece by piece, every piece bit for bit or byte for byte:
  - the kernel alone (j40hip_kat_device_splines) against numpy's float32 statement of the rule (tests/spline_streams.py);
  - the planes a decode leaves (j40hip_frame_read_xyb, stage 6) against that statement applied to the library's own segments
    (tests/test_splines.py holds those against the float64 model) and to planes the library makes WITHOUT the feature: the same frame
    written without the flag and the data (splinetwin=1) and decoded alone, with the restoration filters on for the VarDCT frame;
  - the pixels against k_xyb_to_rgba (or k_colour_tail) alone over those expected planes;
  - the anchors that reach the reference: splines whose colours are all zero change no pixel though the kernel runs, splines whose
    sigmas are all zero launch nothing, and the twin is decoded by the reference at the suite's bar.
tests/test_splines.py has the switch, the refusals at parse, the segments and the CPU build."""
import numpy as np
import pytest

import spline_streams as S
from spline_streams import spline_synth, pair, text_of, bits, spline
from test_scale import box
from test_orient import orient
from test_colour_gpu import tail_inputs
import noise_streams as N
import patch_streams as P

pytestmark = pytest.mark.gpu
U8X4, U16X4 = 0x0F33, 0x0F35
GAB = dict(gab=1)     # the VarDCT frames signal Gaborish: the decodes run with the restoration filters on, the splines go onto the filtered planes
WIDE = spline([(20, 10), (150, 70), (270, 20)], {(0, 0): 14, (1, 0): 30, (1, 2): -8, (2, 0): -20, (3, 0): 10, (3, 1): -2})   # across both groups of the VarDCT frame


@pytest.fixture(scope="module")
def gpu(built):
    import j40_amd
    assert j40_amd.device_count() > 0, "the gpu tests need a HIP device"
    return j40_amd


def cc15(fr):
    m, bias, it, kx, kb = fr.colour_consts()
    return np.concatenate([m.reshape(9), bias, [it, kx, kb]]).astype(np.float32)


def planes_alone(gpu, data, modular):
    """a one-frame stream decoded alone, without the feature: the planes its tail reads (a VarDCT frame: after the filters)"""
    fr = gpu.Frame(data)
    if modular:
        assert fr.set_modular_xyb(1) == ""
    else:
        fr.set_restoration(1)
    fr.upload(0)
    err, px = fr.decode_to_host()
    assert err == ""
    planes = fr.read_xyb(0 if modular else 1)
    fr.close()
    return planes, px


def open_splined(gpu, data, fmt=U8X4, modular=False, colour=False, **kw):
    fr = gpu.Frame(data, splines=True, **kw)
    if modular:
        assert fr.set_modular_xyb(1) == ""
    else:
        fr.set_restoration(1)
    if colour:
        assert fr.set_colour(1) == ""
    fr.set_output_format(fmt)
    fr.upload(0)
    return fr


KINDS = {
    "vardct": dict(mode="vardct", w=S.VW, h=S.VH, given=[S.CURVED, WIDE, S.OUTSIDE], more=GAB),
    "modular": dict(mode="modular", w=S.MW, h=S.MH, given=[S.CURVED, S.STRAIGHT, S.OUTSIDE], more={}),
}
_cache = {}


def case(gpu, kind):
    """the stream with splines of `kind` and its twin, and everything the feature is held against, made once: the twin's planes from a
    decode that does not involve splines, numpy's splat of the library's own segments over them, and k_xyb_to_rgba's pixels of the result"""
    if kind in _cache:
        return _cache[kind]
    K = KINDS[kind]
    data, twin = pair(K["mode"], K["w"], K["h"], K["given"], qadj=1, **K["more"])
    own, twin_px = planes_alone(gpu, twin, kind == "modular")
    fr = gpu.Frame(data, splines=True)
    segs = fr.spline_segments()
    fr.close()
    assert segs.shape[0] > 100
    want = S.apply_segments(own, segs)
    assert not np.array_equal(want, own)
    fr = gpu.Frame(twin)
    consts = cc15(fr)
    fr.close()
    pixels = {}
    for fmt in (U8X4, U16X4):
        code, px = gpu.kat_device_xyb_to_rgba(want, consts, 8, fmt)
        assert code == ""
        pixels[fmt] = px
    _cache[kind] = dict(K, data=data, twin=twin, own=own, twin_px=twin_px, segs=segs, planes=want, pixels=pixels, consts=consts)
    return _cache[kind]


# ---------------------------------------------------------------- 1. the kernel alone

@pytest.mark.parametrize("name", list(S.kat_cases()))
def test_kernel_alone_equals_numpy(gpu, name):
    """this is a test that fails without the feature: the symbol does not exist. Random planes, bit for bit: one segment inside one
    tile; a box over four tiles; boxes clipped at all four frame edges; two splines crossing; a zigzag that puts 310 segments on one
    tile, three LDS chunks of 128; a 65 x 33 frame whose last column and row spill into second tiles"""
    w, h, segs = S.kat_cases()[name]
    planes = S.kat_planes(w, h)
    want = S.apply_segments(planes, segs)
    code, got, tiles = gpu.kat_device_splines(planes, segs)
    assert code == ""
    count, most = S.touched_tiles(segs, w)
    assert tiles == count
    assert np.array_equal(bits(got), bits(want)), "%d samples differ" % int((bits(got) != bits(want)).sum())
    assert not np.array_equal(bits(got), bits(planes))
    if name == "zigzag_beyond_one_chunk":
        assert most == 310
    if name == "two_splines_crossing":
        # the order of the additions is visible in the bits, and the kernel keeps the order it is given
        a = len(S.model_segments([S.CROSS_A], 0, 0.0, 1.0, w, h)[0])
        swapped = np.concatenate([segs[a:], segs[:a]])
        other = S.apply_segments(planes, swapped)
        assert not np.array_equal(bits(other), bits(want))
        code, got, _ = gpu.kat_device_splines(planes, swapped)
        assert code == "" and np.array_equal(bits(got), bits(other))


def test_kernel_hook_refusals_and_nothing_to_draw(gpu):
    planes = S.kat_planes(70, 40)
    for box_ in ((-1, 5, 0, 5), (0, 70, 0, 5), (0, 5, 0, 40), (6, 5, 0, 5), (0, 5, 9, 8)):
        seg = S.make_segment(box_[0], box_[1], box_[2], box_[3], 3.0, 3.0, 2.0, 1.0, (0.1, 0.1, 0.1))
        assert gpu.kat_device_splines(planes, np.stack([seg]))[0] == "rnge", box_
    code, got, tiles = gpu.kat_device_splines(planes, np.zeros((0, 12), np.uint32))
    assert code == "" and tiles == 0 and np.array_equal(bits(got), bits(planes))


# ---------------------------------------------------------------- 2. planes, pixels and the routes

@pytest.mark.parametrize("kind", ["vardct", "modular"])
def test_planes_pixels_and_routes(gpu, kind):
    c = case(gpu, kind)
    fr = open_splined(gpu, c["data"], modular=kind == "modular")
    try:
        err, px = fr.decode_to_host()
        assert err == "" and fr.spline_launches() == 1
        got = fr.read_xyb(6)
        assert np.array_equal(bits(got), bits(c["planes"])), "%d samples differ" % int((bits(got) != bits(c["planes"])).sum())
        assert px.shape == (c["h"], c["w"], 4) and np.array_equal(px, c["pixels"][U8X4])
        assert not np.array_equal(px, c["twin_px"])
        with pytest.raises(gpu.J40Error):
            fr.read_xyb(4)
        # two decodes of one handle are identical: the planes are made anew, the segments are uploaded once
        err, again = fr.decode_to_host()
        assert err == "" and np.array_equal(again, px) and fr.spline_launches() == 2
        # a region straddling a tile corner is the crop of the whole, 1:2 is the mean of the whole
        for (x, y, w, h) in ((57, 25, 20, 15), (0, 0, 64, 32), (c["w"] - 31, c["h"] - 17, 31, 17)):
            assert fr.set_region(x, y, w, h) == ""
            err, part = fr.decode_to_host()
            assert err == "" and np.array_equal(part, px[y:y + h, x:x + w]), (x, y, w, h)
        assert fr.clear_region() == ""
        assert fr.set_scale(1) == ""
        err, small = fr.decode_to_host()
        assert err == "" and np.array_equal(small, box(px, 1))
        assert fr.set_scale(0) == ""
    finally:
        fr.close()
    kw = dict(modular_xyb=True) if kind == "modular" else {}
    assert gpu.decode(c["data"], **kw)[0] == "TODO"
    if kind == "modular":
        err, whole = gpu.decode(c["data"], splines=True, **kw)
        assert err == "" and np.array_equal(whole, px)


@pytest.mark.parametrize("kind", ["vardct", "modular"])
def test_u16_pixels(gpu, kind):
    c = case(gpu, kind)
    fr = open_splined(gpu, c["data"], fmt=U16X4, modular=kind == "modular")
    try:
        err, px = fr.decode_to_host()
        assert err == "" and px.dtype == np.uint16 and np.array_equal(px, c["pixels"][U16X4])
    finally:
        fr.close()


@pytest.mark.parametrize("kind", ["vardct", "modular"])
def test_a_frame_without_splines_is_unchanged_by_the_switch(gpu, kind):
    c = case(gpu, kind)
    fr = open_splined(gpu, c["twin"], modular=kind == "modular")
    try:
        err, plain = fr.decode_to_host()
        assert err == "" and fr.spline_launches() == 0 and np.array_equal(plain, c["twin_px"])
        with pytest.raises(gpu.J40Error):
            fr.read_xyb(6)
    finally:
        fr.close()


def test_modular_frame_needs_the_modular_xyb_switch(gpu):
    c = case(gpu, "modular")
    fr = gpu.Frame(c["data"], splines=True)
    try:
        fr.upload(0)
        assert fr.decode_to_host()[0] == "TODO"
        assert fr.set_modular_xyb(1) == ""
        err, px = fr.decode_to_host()
        assert err == "" and np.array_equal(px, c["pixels"][U8X4])
    finally:
        fr.close()


@pytest.mark.parametrize("kind", ["vardct", "modular"])
def test_colour_mode(gpu, kind):
    """the signalled colour space: the same planes, k_colour_tail alone over them (Display P3 primaries, PQ)"""
    K = KINDS[kind]
    data, _ = pair(K["mode"], K["w"], K["h"], K["given"], qadj=1, primaries=11, tf=16, **K["more"])
    plain = case(gpu, kind)     # (the encoding changes no coefficient: the planes are the sRGB stream's)
    fr = open_splined(gpu, data, modular=kind == "modular", colour=True)
    try:
        err, px = fr.decode_to_host()
        assert err == "" and np.array_equal(bits(fr.read_xyb(6)), bits(plain["planes"]))
        cc, enc, lum, _, bpp, _, _ = tail_inputs(gpu, fr)
        code, want = gpu.kat_device_colour_tail(plain["planes"], cc, enc, lum, bpp, U8X4)
        assert code == "" and np.array_equal(px, want)
        assert not np.array_equal(px, plain["pixels"][U8X4])
    finally:
        fr.close()


def test_an_orientation_is_the_turn_of_the_whole(gpu):
    K = KINDS["vardct"]
    data, _ = pair("vardct", K["w"], K["h"], K["given"], qadj=1, orientation=6, **GAB)
    px = case(gpu, "vardct")["pixels"][U8X4]      # (the option changes no stored pixel)
    fr = open_splined(gpu, data)
    try:
        assert fr.set_orientation(1) == ""
        err, turned = fr.decode_to_host()
        assert err == "" and np.array_equal(turned, orient(px, 6))
    finally:
        fr.close()


# ---------------------------------------------------------------- 3. the order: patches, splines, noise

def test_patches_then_splines_then_noise(gpu):
    """a reference-only frame, then a frame with one Replace patch under a spline, and noise: its planes are numpy's noise over numpy's
    splat over numpy's patches over the twin's planes, and no other order gives them"""
    refs = [(1, 2, 3, 100, 24, [(70, 40, P.REPLACE, 0)])]
    over = [spline([(60, 30), (120, 52), (190, 45)], {(0, 0): 12, (1, 0): 35, (2, 0): -18, (3, 0): 11})]   # across the patch at (70, 40), 100 x 24
    opts = P.seq_opts("v", refs, [P.REF_V], ["v"], splines=";" + text_of(over), noise=";" + N.lut_text(N.LUT), **GAB)
    data = spline_synth("vardct", P.VW, P.VH, **opts)
    seq = gpu.Sequence(data, patches=True, splines=True, noise=True)
    try:
        seq.upload(0)
        err, px = seq.next_to_host()
        assert err == "" and seq.status() == ("", -1)
        fr = seq.frame(1)
        assert fr.spline_launches() == 1 and fr.noise_launches() == 1 and seq.frame_patches(1)["launches"] == 1
        planes = fr.read_xyb(4)
        segs = fr.spline_segments()
        slot = seq.read_ref_slot(1)
        before_splines = fr.read_xyb(3)      # (the sequence's stage 3: the planes between k_patch_blend and k_spline_draw)
        with pytest.raises(gpu.J40Error):    # (noise follows: what stood between k_spline_draw and k_noise_add is gone)
            fr.read_xyb(6)
    finally:
        seq.close()
    twin = spline_synth("vardct", P.VW, P.VH, **dict(opts, only=1, patchtwin=1, splinetwin=1, noisetwin=1))
    fr = gpu.Frame(twin)
    fr.set_restoration(1)
    fr.upload(0)
    assert fr.decode_to_host()[0] == ""
    own = fr.read_xyb(0)        # (a sequence's frames decode with the filters off unless asked: the planes before them)
    fr.close()
    lut = N.lut_of(N.LUT)
    noise = lambda p: N.apply_noise(p, lut, 0.0, 1.0, gdim=256, visible=0, nonvisible=1)
    patch = lambda p: P.apply_patches(p, {1: slot}, P.flat(refs))
    draw = lambda p: S.apply_segments(p, segs)
    assert np.array_equal(bits(before_splines), bits(patch(own))), "stage 3 does not hold the pre-spline planes"
    assert not np.array_equal(bits(before_splines), bits(own)) and not np.array_equal(bits(before_splines), bits(draw(patch(own))))
    want = noise(draw(patch(own)))
    assert np.array_equal(bits(planes), bits(want)), "%d samples differ" % int((bits(planes) != bits(want)).sum())
    for other in (noise(patch(draw(own))), draw(noise(patch(own))), patch(noise(draw(own)))):
        assert not np.array_equal(bits(other), bits(want))


def test_patches_then_splines_without_noise(gpu):
    """the same frame without noise: stage 3 the patched planes, stage 6 the splat over them"""
    refs = [(1, 2, 3, 100, 24, [(70, 40, P.REPLACE, 0)])]
    over = [spline([(60, 30), (120, 52), (190, 45)], {(0, 0): 12, (1, 0): 35, (2, 0): -18, (3, 0): 11})]
    opts = P.seq_opts("v", refs, [P.REF_V], ["v"], splines=";" + text_of(over), **GAB)
    seq = gpu.Sequence(spline_synth("vardct", P.VW, P.VH, **opts), patches=True, splines=True)
    try:
        seq.upload(0)
        err, _ = seq.next_to_host()
        assert err == "" and seq.status() == ("", -1)
        fr = seq.frame(1)
        stage3, stage6, segs, slot = fr.read_xyb(3), fr.read_xyb(6), fr.spline_segments(), seq.read_ref_slot(1)
    finally:
        seq.close()
    fr = gpu.Frame(spline_synth("vardct", P.VW, P.VH, **dict(opts, only=1, patchtwin=1, splinetwin=1)))
    fr.set_restoration(1)
    fr.upload(0)
    assert fr.decode_to_host()[0] == ""
    own = fr.read_xyb(0)
    fr.close()
    patched = P.apply_patches(own, {1: slot}, P.flat(refs))
    assert np.array_equal(bits(stage3), bits(patched))
    assert np.array_equal(bits(stage6), bits(S.apply_segments(patched, segs))) and not np.array_equal(bits(stage6), bits(stage3))


def test_kept_alpha(gpu):
    """the splines go onto the colour samples, the kept alpha channel is the twin's"""
    K = KINDS["vardct"]
    data, twin = pair("vardct", K["w"], K["h"], K["given"], qadj=1, alpha=1, **GAB)
    out = []
    for stream in (data, twin):
        fr = gpu.Frame(stream, splines=True)
        assert fr.set_alpha(1) == ""
        fr.upload(0)
        try:
            err, px = fr.decode_to_host()
            assert err == ""
            out.append((px, fr.read_xyb(6) if stream is data else None, fr.spline_segments()))
        finally:
            fr.close()
    (drawn, planes, segs), (plain, _, _) = out
    assert np.array_equal(drawn[..., 3], plain[..., 3]) and len(np.unique(plain[..., 3])) > 1
    fr = gpu.Frame(twin)
    fr.set_restoration(1)
    fr.upload(0)
    assert fr.decode_to_host()[0] == ""
    own = fr.read_xyb(0)      # (the filters are off in the decodes above: the planes before them)
    consts = cc15(fr)
    fr.close()
    want = S.apply_segments(own, segs)
    assert np.array_equal(bits(planes), bits(want))
    code, rgb = gpu.kat_device_xyb_to_rgba(want, consts, 8, U8X4)
    assert code == "" and np.array_equal(drawn[..., :3], rgb[..., :3]) and not np.array_equal(drawn[..., :3], plain[..., :3])


def test_what_a_frame_with_splines_refuses(gpu):
    """a partial group range, a batch and the many-frames LF preview are "TODO" for a frame with splines; its twin takes all three"""
    import torch
    c = case(gpu, "vardct")
    out = torch.zeros((c["h"], c["w"] * 4), dtype=torch.uint8, device="cuda:0")
    for stream, code in ((c["data"], "TODO"), (c["twin"], "")):
        fr = open_splined(gpu, stream)
        try:
            try:
                fr.set_group_range(0, 1)
                got = ""
            except gpu.J40Error as e:
                got = e.code
            assert got == code
            if not code:
                fr.set_group_range(0, 2)     # (every group again)
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


def test_an_upsampled_frame_with_splines_is_todo(gpu):
    """its splines belong on the coded planes ahead of the stretch: a follow-up. The same frame without them decodes"""
    opts = dict(upsampling=2, upweights="nearest", splines=text_of([S.CURVED]), **GAB)
    for more, code in ((dict(), "TODO"), (dict(splinetwin=1), "")):
        fr = gpu.Frame(spline_synth("vardct", 2 * S.VW, 2 * S.VH, **opts, **more), upsampling=True, splines=True)
        try:
            fr.upload(0)
            assert fr.decode_to_host()[0] == code
        finally:
            fr.close()


# ---------------------------------------------------------------- 4. the anchors that reach the reference

def test_anchor_zero_colours_draw_nothing_visible_and_zero_sigmas_launch_nothing(gpu, ref):
    c = case(gpu, "vardct")
    no_colour = [spline(s["points"], {k: v for k, v in s["coef"].items() if k[0] == 3}) for s in c["given"]]
    no_sigma = [spline(s["points"], {k: v for k, v in s["coef"].items() if k[0] != 3}) for s in c["given"]]
    data, twin = pair("vardct", S.VW, S.VH, no_colour, qadj=1, **GAB)
    assert twin == c["twin"]      # (the twin holds no spline data: any description gives the same bytes)
    fr = open_splined(gpu, data)
    try:
        err, px = fr.decode_to_host()
        assert err == "" and fr.spline_launches() == 1 and fr.spline_bins()[0] > 0
        assert np.array_equal(px, c["twin_px"])
    finally:
        fr.close()
    data, _ = pair("vardct", S.VW, S.VH, no_sigma, qadj=1, **GAB)
    fr = open_splined(gpu, data)
    try:
        err, px = fr.decode_to_host()
        assert err == "" and fr.spline_launches() == 0 and fr.spline_segments().shape[0] == 0 and fr.spline_bins() == (0, 0)
        assert np.array_equal(px, c["twin_px"])
        assert np.array_equal(bits(fr.read_xyb(6)), bits(c["own"]))
    finally:
        fr.close()
    # the twin without the filters, as the reference decodes it
    fr = gpu.Frame(c["twin"])
    fr.upload(0)
    err, alone = fr.decode_to_host()
    fr.close()
    rerr, want = ref.decode(c["twin"])
    assert err == "" and rerr == ""
    d = int(np.abs(alone[..., :3].astype(np.int32) - want[..., :3].astype(np.int32)).max())
    print("against the reference: max |delta| =", d)
    assert d <= 1 and np.array_equal(alone[..., 3], want[..., 3])
