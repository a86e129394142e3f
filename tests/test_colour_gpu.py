"""The colour mode on the device (include/j40hip.h: j40hip_frame_set_colour, J40HIP_SEQ_COLOUR; k_colour_tail). PARITY UNPINNED: the
reference renders every XYB image as sRGB, so it pins the switch-off bytes alone; everything else is held against the CPU build of the
same functions (byte for byte), a float64 model of the standards' formulas (an interval, below) and the library's own whole decode
(composition). tests/test_colour.py has the CPU half.

The whole-decode bar. From the frame's own XYB planes (j40hip_frame_read_xyb) the model computes in float64 the linear value v of every
sample and the forward bound of the tail's float32 mixing, e = 16 * 2^-24 * sum_j |m'_cj| (|pp_j|^3 + |bias_j|) * itscale; every curve is
monotone, so the sample must lie between the model's level at v - e and at v + e. No measured tolerance enters. (A fixed +-1 level is
not valid near black under PQ: the mixing's float32 noise is several levels there.)"""
import os
import subprocess
import sys

import numpy as np
import pytest

from streams import synth, ROOT
from test_scale import box
from test_orient import orient
import colour_streams as X

pytestmark = pytest.mark.gpu
U8X4, U16X4 = X.U8X4, X.U16X4
SIZES = ((37, 21), (65, 24), (300, 70))   # the last crosses a 256 group and the tail's 64 x 4 block edges
CURVES = sorted(X.CURVES)


@pytest.fixture(scope="module")
def gpu(built):
    import j40_amd
    assert j40_amd.device_count() > 0, "the gpu tests need a HIP device"
    assert (j40_amd.J40_U8X4, j40_amd.J40_U16X4) == (U8X4, U16X4)
    return j40_amd


@pytest.fixture(scope="module")
def sim(built):
    return X.ColourSim()


def tail_inputs(gpu, fr):
    """what k_colour_tail takes for a frame, by the host's getters: (cc15 with the folded matrix, encoding words, lum, intensity_target, bpp, bias)"""
    m, bias, it, _, _ = fr.colour_consts()
    enc = fr.colour_encoding(words=True)
    code, P, lum = gpu.colour_gamut_matrix(enc)
    assert code == ""
    info = np.zeros(21, np.int64)
    gpu.lib().j40hip_frame_info(fr.h, info.ctypes.data)
    folded = X.folded_matrix(P, m)
    cc = np.concatenate([folded.reshape(9), bias, [it, 0, 0]]).astype(np.float32)
    return cc, enc, lum.astype(np.float32), float(it), int(info[18]), bias, folded


def open_frame(gpu, data, fmt=U8X4, colour=1, alpha=False, restoration=None, modular_xyb=False):
    fr = gpu.Frame(data)
    if modular_xyb:
        assert fr.set_modular_xyb(1) == ""
    if alpha:
        assert fr.set_alpha(1) == ""
    if restoration is not None:
        fr.set_restoration(restoration)
    assert fr.set_colour(colour) == ""
    fr.set_output_format(fmt)
    fr.upload(0)
    return fr


# ---------------------------------------------------------------- 1. the kernel alone

def kat_planes(w, h, seed):
    rng = np.random.default_rng(seed)
    xyb = np.stack([rng.uniform(-0.03, 0.03, (h, w)), rng.uniform(0.0, 0.9, (h, w)), rng.uniform(0.0, 0.9, (h, w))]).astype(np.float32)
    flat = xyb.reshape(3, -1)
    odd = np.array([np.nan, np.inf, -np.inf, 1e38, -1e38, 0.0, -0.0, 1e-30, 0.155, 0.1551], np.float32)   # (0.155: the cube root of the bias, black)
    n = min(len(odd), flat.shape[1] // 3)
    for c in range(3):
        flat[c, c:3 * n:3] = odd[:n]
    flat[:, -1] = 0.155
    return xyb


@pytest.mark.parametrize("fmt", [U8X4, U16X4], ids=["u8", "u16"])
@pytest.mark.parametrize("curve", CURVES)
def test_kernel_equals_the_cpu_build(gpu, sim, curve, fmt):
    cenc, it = X.CURVES[curve]
    enc = X.enc_words(white=cenc.get("white", 1), primaries=cenc.get("primaries", 1), tf=cenc.get("tf", 13), gamma=cenc.get("gamma", 0))
    code, P, lum = gpu.colour_gamut_matrix(enc)
    assert code == ""
    default_m = [[11.031566901960783, -9.866943921568629, -0.16462299647058826], [-3.254147380392157, 4.418770392156863, -0.16462299647058826],
                 [-3.6588512862745097, 2.7129230470588235, 1.9459282392156863]]
    cc = np.concatenate([X.folded_matrix(P, np.array(default_m, np.float32)).reshape(9), [-0.0037930732552754493] * 3, [it or 255, 0, 0]]).astype(np.float32)
    for i, (w, h) in enumerate(SIZES):
        xyb = kat_planes(w, h, 40 + i)
        for bpp in (8, 10):
            want, tabled = sim.tail(xyb, cc, enc, lum, bpp, fmt)
            assert tabled == (bpp == 8)
            code, got = gpu.kat_device_colour_tail(xyb, cc, enc, lum, bpp, fmt, pad=5)
            assert code == ""
            assert np.array_equal(got, want), "%s %dx%d bpp %d: %d pixels differ" % (curve, w, h, bpp, int((got != want).any(axis=2).sum()))
            assert (got[..., 3] == (255 if fmt == U8X4 else 65535)).all()
        # an 8-bit frame by the curve instead of the table: the same bytes
        code, long_way = gpu.kat_device_colour_tail(xyb, cc, enc, lum, 8, fmt, use_table=False)
        assert code == "" and np.array_equal(long_way, sim.tail(xyb, cc, enc, lum, 8, fmt)[0])


def test_kat_hook_refusals(gpu):
    xyb = kat_planes(8, 8, 1)
    cc = np.array(list(np.eye(3).ravel()) + [0, 0, 0, 255, 0, 0], np.float32)
    lum = [0.2, 0.7, 0.1]
    assert gpu.kat_device_colour_tail(xyb, cc, X.enc_words(), lum, 8, 0x1234)[0] == "Ufm?"
    assert gpu.kat_device_colour_tail(xyb, cc, X.enc_words(), lum, 7)[0] == "rnge"
    assert gpu.kat_device_colour_tail(xyb, cc, X.enc_words(tf=2), lum, 8)[0] == "Ucs?"


# ---------------------------------------------------------------- 2. whole decodes against the float64 model

@pytest.mark.parametrize("fmt", [U8X4, U16X4], ids=["u8", "u16"])
@pytest.mark.parametrize("bpp", [8, 10])
@pytest.mark.parametrize("curve", CURVES)
def test_whole_vardct_decode_within_the_model_interval(gpu, curve, bpp, fmt):
    for w, h in SIZES:
        data = X.stream("vardct", w, h, curve, **(dict(bpp=bpp) if bpp != 8 else {}))
        fr = open_frame(gpu, data, fmt)
        try:
            q = fr.colour()
            assert q["applies"] and q["in_force"]
            err, px = fr.decode_to_host()
            assert err == "" and fr.colour()["used"]
            # (8-bit frames take their curve's threshold table; the linear curve has none on purpose and says so)
            assert fr.colour()["curve_evaluated_at_8_bits"] == (bpp == 8 and curve == "linear")
            xyb = fr.read_xyb(0)
            cc, enc, lum, it, fbpp, bias, folded = tail_inputs(gpu, fr)
            assert fbpp == bpp
        finally:
            fr.close()
        lo, hi = X.model_interval(xyb, folded, bias, it, enc, lum, bpp)
        conv = X.to_u8 if fmt == U8X4 else X.to_u16
        got = px[..., :3].astype(np.int64)
        below, above = got < conv(lo, bpp), got > conv(hi, bpp)
        width = (hi - lo)
        print("%s %dx%d bpp %d: outside the interval %d of %d; interval width in levels: median %d, max %d; levels used %d..%d" %
              (curve, w, h, bpp, int(below.sum() + above.sum()), got.size, int(np.median(width)), int(width.max()), int(lo.min()), int(hi.max())))
        assert not below.any() and not above.any()
        assert (px[..., 3] == (255 if fmt == U8X4 else 65535)).all()
        assert hi.max() - lo.min() > (1 << bpp) // 8, "a picture that uses an eighth of the range proves little: pick another stream"


# ---------------------------------------------------------------- 3. the default stays

def test_switch_on_default_encoding_is_the_usual_decode(gpu):
    for w, h in SIZES:
        for opts in (dict(), dict(cenc=1)):   # all_default, and the sRGB encoding written out
            data = synth("vardct", w, h, X.SEED, passes=2, **opts)
            for fmt in (U8X4, U16X4):
                off = open_frame(gpu, data, fmt, colour=0); on = open_frame(gpu, data, fmt, colour=1)
                e0, p0 = off.decode_to_host(); e1, p1 = on.decode_to_host()
                assert e0 == "" and e1 == "" and np.array_equal(p0, p1)
                assert not on.colour()["in_force"] and not on.colour()["used"]
                off.close(); on.close()


@pytest.mark.parametrize("curve", CURVES)
def test_switch_off_any_encoding_is_todays_decode(gpu, curve):
    """passes on the parent commit too: it guards the default"""
    cenc, it = X.CURVES[curve]
    tone = dict(tone="%d,0.5" % it) if it else {}
    for w, h in SIZES:
        for fmt in (U8X4, U16X4):
            a = open_frame(gpu, X.stream("vardct", w, h, curve), fmt, colour=0)
            b = open_frame(gpu, synth("vardct", w, h, X.SEED, passes=2, **tone), fmt, colour=0)
            ea, pa = a.decode_to_host(); eb, pb = b.decode_to_host()
            assert ea == "" and eb == "" and np.array_equal(pa, pb)
            assert not a.colour()["used"]
            a.close(); b.close()
    err, px = gpu.decode(X.stream("vardct", 65, 24, curve))   # the public API, nothing in the environment
    assert err == "" and np.array_equal(px, gpu.decode(synth("vardct", 65, 24, X.SEED, passes=2, **tone))[1])


# ---------------------------------------------------------------- 4. composition, 65 x 24, PQ / BT.2100

W, H = 65, 24
_whole = {}


def whole(gpu, fmt=U8X4, **opts):
    key = (fmt, tuple(sorted(opts.items())))
    if key not in _whole:
        fr = open_frame(gpu, X.stream("vardct", W, H, "pq", **opts), fmt)
        err, px = fr.decode_to_host()
        assert err == "" and fr.colour()["used"]
        fr.close()
        px.setflags(write=False)
        _whole[key] = px
    return _whole[key]


@pytest.mark.parametrize("fmt", [U8X4, U16X4], ids=["u8", "u16"])
def test_region_scale_orientation(gpu, fmt):
    full = whole(gpu, fmt)
    off = open_frame(gpu, X.stream("vardct", W, H, "pq"), fmt, colour=0)
    assert not np.array_equal(off.decode_to_host()[1], full), "the switch changes nothing for this stream: it proves nothing"
    off.close()
    data = X.stream("vardct", W, H, "pq")
    for rect in ((0, 0, 65, 24), (3, 5, 40, 11), (64, 23, 1, 1), (10, 0, 55, 24)):
        err, px = gpu.decode_region(data, *rect, fmt=fmt, colour=True)
        x, y, w, h = rect
        assert err == "" and np.array_equal(px, full[y:y + h, x:x + w]), rect
    for k in (1, 2):
        err, px = gpu.decode(data, fmt=fmt, scale=k, colour=True)
        assert err == "" and np.array_equal(px, box(full, k)), k
    turned = X.stream("vardct", W, H, "pq", orientation=6)
    fr = open_frame(gpu, turned, fmt)
    assert fr.set_orientation(1) == ""
    err, px = fr.decode_to_host()
    assert err == "" and fr.colour()["used"] and np.array_equal(px, orient(full, 6))
    fr.close()


def test_kept_alpha(gpu):
    data = X.stream("vardct", 300, 70, "pq", alpha=1, passes=1)   # (the writer makes alpha with one pass: two groups, then)
    srgb = open_frame(gpu, data, colour=0, alpha=True); col = open_frame(gpu, data, colour=1, alpha=True)
    e0, p0 = srgb.decode_to_host(); e1, p1 = col.decode_to_host()
    assert e0 == "" and e1 == "" and col.colour()["used"] and col.alpha()["written"] == 1
    assert np.array_equal(p0[..., 3], p1[..., 3]) and p0[..., 3].min() < 255, "alpha is the kept channel, untouched by the colour tail"
    opaque = open_frame(gpu, data, colour=1)
    e2, p2 = opaque.decode_to_host()
    assert e2 == "" and np.array_equal(p1[..., :3], p2[..., :3]) and (p2[..., 3] == 255).all()
    for f in (srgb, col, opaque):
        f.close()


@pytest.mark.parametrize("fmt", [U8X4, U16X4], ids=["u8", "u16"])
def test_restoration_then_the_tail(gpu, fmt):
    data = X.stream("vardct", W, H, "pq", fullheader=1, gab=1, epf=2)
    fr = open_frame(gpu, data, fmt, restoration=1)
    err, px = fr.decode_to_host()
    assert err == "" and fr.colour()["used"] and fr.restoration().as_list() is not None
    filtered, before = fr.read_xyb(1), fr.read_xyb(0)
    assert not np.array_equal(filtered, before), "the filters ran"
    cc, enc, lum, it, bpp, _, _ = tail_inputs(gpu, fr)
    fr.close()
    code, want = gpu.kat_device_colour_tail(filtered, cc, enc, lum, bpp, fmt)
    assert code == "" and np.array_equal(px, want)
    plain = open_frame(gpu, data, fmt)   # the same stream without the filters: another picture
    assert not np.array_equal(plain.decode_to_host()[1], px)
    plain.close()


@pytest.mark.parametrize("fmt", [U8X4, U16X4], ids=["u8", "u16"])
@pytest.mark.parametrize("alpha", [0, 1])
def test_modular_xyb_frame(gpu, fmt, alpha):
    opts = dict(alpha=1) if alpha else {}
    data = X.stream("modular", W, H, "pq", **opts)
    fr = open_frame(gpu, data, fmt, modular_xyb=True)
    err, px = fr.decode_to_host()
    assert err == "" and fr.colour()["used"] and fr.modular_xyb()["used"] == 1
    planes = fr.read_xyb(0)
    cc, enc, lum, it, bpp, _, _ = tail_inputs(gpu, fr)
    # the switch off on the same handle: the fused Modular XYB kernel's sRGB pixels, the same alpha
    assert fr.set_colour(0) == ""
    err0, srgb = fr.decode_to_host()
    assert err0 == "" and not fr.colour()["used"]
    fr.close()
    code, want = gpu.kat_device_colour_tail(planes, cc, enc, lum, bpp, fmt)
    assert code == "" and np.array_equal(px[..., :3], want[..., :3])
    assert np.array_equal(px[..., 3], srgb[..., 3]) and not np.array_equal(px[..., :3], srgb[..., :3])
    if alpha:
        assert srgb[..., 3].min() < (255 if fmt == U8X4 else 65535)
    # a region and a scale of it go through the full-size staging image
    reg = open_frame(gpu, data, fmt, modular_xyb=True)
    assert reg.set_region(3, 5, 40, 11) == ""
    err, part = reg.decode_to_host()
    assert err == "" and np.array_equal(part, px[5:16, 3:43])
    assert reg.set_region(0, 0, 0, 0) == "" and reg.set_scale(1) == ""
    err, small = reg.decode_to_host()
    assert err == "" and np.array_equal(small, box(px, 1))
    reg.close()


def test_sequence(gpu):
    """a two-frame Replace animation with J40HIP_SEQ_COLOUR: every canvas is its frame's own decode, in the signalled space"""
    data = X.stream("vardct", W, H, "pq", frames=2, anim=1, durations="1,1")
    on, _ = gpu.decode_frames(data, colour=True)
    off, _ = gpu.decode_frames(data)
    assert len(on) == len(off) == 2
    seq = gpu.Sequence(data, colour=True)
    seq.upload(0)
    plain = gpu.Sequence(data)
    assert not plain.frame(0).colour()["in_force"]
    plain.close()
    for k, (canvas, _) in enumerate(on):
        fr = seq.frame(k)
        assert fr.colour()["in_force"]
        e, alone = fr.decode_to_host()
        assert e == "" and fr.colour()["used"] and np.array_equal(canvas, alone), k
        assert not np.array_equal(canvas, off[k][0])
        xyb = fr.read_xyb(0)
        cc, enc, lum, it, bpp, _, _ = tail_inputs(gpu, fr)
        code, want = gpu.kat_device_colour_tail(xyb, cc, enc, lum, bpp, U8X4)
        assert code == "" and np.array_equal(canvas, want), k
    seq.close()


# ---------------------------------------------------------------- 5. refusals

def test_refusals_on_the_device(gpu):
    pq = dict(primaries=9, tf=16)
    # a batch member with the mode in force; the frame still decodes
    fr = open_frame(gpu, synth("vardct", 300, 260, X.SEED, **pq))
    err, px = fr.decode_to_host()
    assert err == "" and fr.colour()["used"]
    with pytest.raises(gpu.J40Error) as e:
        gpu.Batch([fr])
    assert e.value.code == "Ucs?"
    err, again = fr.decode_to_host()
    assert err == "" and np.array_equal(px, again)
    # a partial group range and the mode exclude each other, whichever comes first
    with pytest.raises(gpu.J40Error) as e:
        fr.set_group_range(0, 1)
    assert e.value.code == "Ucs?"
    assert fr.set_colour(0) == ""
    batch = gpu.Batch([fr]); batch.close()
    fr.set_group_range(0, 1)
    assert fr.set_colour(1) == "Ucs?" and not fr.colour()["in_force"]
    fr.close()
    # the setter's list, after an upload as before it
    for data, kw, prepare in ((synth("vardct", 300, 260, X.SEED, icc=700), {}, None), (synth("vardct", 37, 21, X.SEED, passes=2, tf=2), {}, None),
                              (synth("modular", 37, 21, X.SEED, xyb=1, grey=1), {}, None), (synth("vardct", 64, 64, X.SEED, ycbcr=1), dict(ycbcr=True), None),
                              (synth("modular", 37, 21, X.SEED, xyb=1, **pq), {}, None)):
        f = gpu.Frame(data, **kw)   # (parses: nothing here is "TODO")
        if prepare:
            assert f.set_modular_xyb(1) == ""
        if kw:
            assert f.set_ycbcr(1) == ""
        f.upload(0)
        assert f.set_colour(1) == "Ucs?" and not f.colour()["in_force"]
        err, _ = f.decode_to_host()
        assert err == "" and not f.colour()["used"]
        f.close()
    # xyb_encoded = 0: accepted, nothing changes
    data = synth("modular", 37, 21, X.SEED, **pq)
    a = open_frame(gpu, data, colour=1); b = open_frame(gpu, data, colour=0)
    assert np.array_equal(a.decode_to_host()[1], b.decode_to_host()[1]) and not a.colour()["used"]
    a.close(); b.close()
    # j40hip_frame_decode_xyb's planes and the LF preview are not the mode's business: the preview of an LF-only handle refuses it
    lf = gpu.Frame(synth("vardct", 300, 260, X.SEED, **pq), lf_only=True)
    assert lf.set_colour(1) == "Ucs?"
    lf.close()


def test_lf_preview_is_refused_while_the_mode_is_in_force(gpu):
    """the preview's tail renders sRGB: a full handle with the colour mode in force gets "Ucs?" from the single-frame preview entries
    and from the many-frames one alike, and its preview again once the mode is off; the float planes are not the mode's business"""
    import torch
    data = X.stream("vardct", 300, 70, "pq")
    fr = open_frame(gpu, data, colour=0)
    want = fr.decode_lf_to_host()
    plane = fr.read_lf(1)
    w8, h8 = fr.lf_size()
    buf = torch.zeros((h8, w8 * 4), dtype=torch.uint8, device="cuda:0")
    assert fr.set_colour(1) == "" and fr.colour()["in_force"]
    with pytest.raises(gpu.J40Error) as e:
        fr.decode_lf_to_host()
    assert e.value.code == "Ucs?"
    with pytest.raises(gpu.J40Error) as e:
        fr.decode_lf(buf.data_ptr(), w8 * 4, torch.cuda.current_stream(0).cuda_stream)
    assert e.value.code == "Ucs?"
    assert gpu.frames_decode_lf([fr], [buf.data_ptr()], [w8 * 4], torch.cuda.current_stream(0).cuda_stream) == "Ucs?"
    torch.cuda.synchronize()
    assert int(buf.count_nonzero()) == 0, "a refused preview writes nothing"
    assert np.array_equal(fr.read_lf(1), plane)
    err, px = fr.decode_to_host()          # the full decode is served as ever
    assert err == "" and fr.colour()["used"]
    assert fr.set_colour(0) == ""
    assert np.array_equal(fr.decode_lf_to_host(), want)
    assert gpu.frames_decode_lf([fr], [buf.data_ptr()], [w8 * 4], torch.cuda.current_stream(0).cuda_stream) == ""
    torch.cuda.synchronize()
    assert np.array_equal(buf.cpu().numpy().reshape(h8, w8, 4), want)
    fr.close()
    # the default encoding with the switch on: the mode is not in force, the preview is served
    fr = open_frame(gpu, synth("vardct", 300, 70, X.SEED, passes=2), colour=1)
    assert fr.decode_lf_to_host().shape == (h8, w8, 4)
    fr.close()


def test_sequence_holds_one_colour_space(gpu):
    """with the flag, a Modular XYB frame that would be composed as sRGB among frames in the signalled space is refused; with the
    Modular XYB switch as well it is served through k_modular_to_xyb and the tail"""
    data = X.stream("modular", W, H, "pq", frames=2, anim=1, durations="1,1")
    seq = gpu.Sequence(data, colour=True)
    with pytest.raises(gpu.J40Error) as e:
        seq.frame(0)
    assert e.value.code == "Ucs?"
    seq.close()
    on, _ = gpu.decode_frames(data, colour=True, modular_xyb=True)
    off, _ = gpu.decode_frames(data, modular_xyb=True)
    assert len(on) == 2 and not np.array_equal(on[0][0], off[0][0])
    plain, _ = gpu.decode_frames(data)     # neither switch: R, G, B as ever
    assert len(plain) == 2
    with pytest.raises(gpu.J40Error) as e:   # an image the mode refuses as a whole fails the open
        gpu.Sequence(synth("vardct", W, H, X.SEED, passes=2, frames=2, anim=1, durations="1,1", tf=2), colour=True)
    assert e.value.code == "Ucs?"


CHILD = r"""
import os, sys
import numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
import j40_amd
import colour_streams as X
data = X.stream("vardct", 65, 24, "pq")
err, px = j40_amd.decode(data)
assert err == "", err
np.save(sys.argv[2], px)
j40_amd.shutdown()
"""


def test_environment_variable_in_a_fresh_process(gpu, tmp_path):
    """J40HIP_COLOUR=1 applies the mode to the ten-function API (the single-frame route); without it the same call renders sRGB"""
    outs = {}
    for tag, env in (("on", {"J40HIP_COLOUR": "1"}), ("off", {})):
        path = str(tmp_path / (tag + ".npy"))
        r = subprocess.run([sys.executable, "-c", CHILD, ROOT, path], env=dict(os.environ, **env), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
        assert r.returncode == 0, r.stdout.decode()
        outs[tag] = np.load(path)
    assert np.array_equal(outs["on"], whole(gpu))
    fr = open_frame(gpu, X.stream("vardct", W, H, "pq"), colour=0)
    assert np.array_equal(outs["off"], fr.decode_to_host()[1])
    fr.close()
