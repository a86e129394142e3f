"""Modular frames of XYB images through the XYB colour tail on the device (include/j40hip.h: j40hip_frame_set_modular_xyb,
J40HIP_SEQ_MODULAR_XYB; k_modular_xyb_pack, k_modular_to_xyb). PARITY UNPINNED: the reference renders such a frame's integers as R, G, B,
so it pins the switch-off bytes and, through the twin of an LF-frame stream, the Modular LF frame's leg; everything else is held against
the rule's statement in numpy (bit for bit), the two-kernel route through the VarDCT colour tail's own kernel (byte for byte) and a
float64 model (within one level). tests/test_modular_xyb.py has the CPU half and the bars' reasons."""
import os
import subprocess
import sys

import numpy as np
import pytest

from streams import synth
import modxyb_streams as X
from lf_streams import WIDE, TALL, lf_stream, lf_twin, lf_stats, lf_size

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U8X4, U16X4 = 0x0F33, 0x0F35
DEFAULT_CC = X.consts15([[11.031566901960783, -9.866943921568629, -0.16462299647058826], [-3.254147380392157, 4.418770392156863, -0.16462299647058826],
                         [-3.6588512862745097, 2.7129230470588235, 1.9459282392156863]], [-0.0037930732552754493] * 3, 255.0)


@pytest.fixture(scope="module")
def gpu(built):
    import j40_amd
    assert j40_amd.device_count() > 0, "the gpu tests need a HIP device"
    assert (j40_amd.J40_U8X4, j40_amd.J40_U16X4) == (U8X4, U16X4)
    return j40_amd


# ---------------------------------------------------------------- 1. the kernels alone

def kat_planes(dtype, w, h, seed):
    rng = np.random.default_rng(seed)
    info = np.iinfo(dtype)
    c = np.stack([rng.integers(0, 500, (h, w)), rng.integers(-130, 130, (h, w)), rng.integers(-400, 300, (h, w))]).astype(dtype)
    alpha = rng.integers(-20, 300, (h, w)).astype(dtype)
    special = [info.min, info.max, 0, -1] + ([2 ** 24 + 1, -(2 ** 24) - 1, 2 ** 30 + 12345] if dtype == np.int32 else [32767, -32768])
    flat, k = c.reshape(3, -1), 0
    for a in special:                       # the extremes, as far as the shape has room for them
        for b in special:
            if k < flat.shape[1] and k % 3 == 0:
                flat[0, k] = a; flat[2, k] = b; flat[1, k] = special[(k // 3) % len(special)]
            k += 1
    alpha.reshape(-1)[::7] = info.max
    alpha.reshape(-1)[3::11] = info.min
    return c, alpha


@pytest.mark.parametrize("with_alpha", [False, True], ids=["opaque", "alpha"])
@pytest.mark.parametrize("dtype,bpp", [(np.int16, 8), (np.int16, 12), (np.int32, 8), (np.int32, 16)], ids=["int16_8", "int16_12", "int32_8", "int32_16"])
@pytest.mark.parametrize("fmt", [U8X4, U16X4], ids=["u8", "u16"])
def test_fused_kernel_equals_the_two_kernel_route(gpu, fmt, dtype, bpp, with_alpha):
    for i, (w, h) in enumerate(((1, 1), (63, 5), (65, 4), (257, 9))):
        c, alpha = kat_planes(dtype, w, h, 100 + i)
        for m in (X.M_DEFAULT, X.M_LFDEQUANT):
            err, fused, two, xyb, guard = gpu.kat_device_modular_xyb(c, alpha if with_alpha else None, m, DEFAULT_CC, bpp, fmt, pad=24)
            assert err == "" and guard, (w, h)
            assert np.array_equal(xyb.view(np.uint32), X.statement(c, m).view(np.uint32)), (w, h)
            assert np.array_equal(fused, two), "%d x %d: %d pixels differ" % (w, h, int((fused != two).any(axis=2).sum()))
            full = 65535 if fmt == U16X4 else 255
            want_a = (X.alpha_u16 if fmt == U16X4 else X.alpha_u8)(alpha, bpp) if with_alpha else np.full((h, w), full)
            assert np.array_equal(fused[..., 3], want_a)


def test_kat_hook_refusals(gpu):
    c, _ = kat_planes(np.int16, 8, 8, 1)
    assert gpu.kat_device_modular_xyb(c, None, X.M_DEFAULT, DEFAULT_CC, 8, 0x1234)[0] == "Ufm?"
    assert gpu.kat_device_modular_xyb(c, None, X.M_DEFAULT, DEFAULT_CC, 7)[0] == "rnge"
    assert gpu.kat_device_modular_xyb(c, None, X.M_DEFAULT, DEFAULT_CC, 16)[0] == "rnge"   # (16-bit levels do not fit int16 planes)


# ---------------------------------------------------------------- 2. whole frames with the switch on

FRAME_CASES = [
    ("one_section_rct", 37, 21, dict()),
    ("one_section_alpha", 37, 21, dict(alpha=1)),
    ("nine_groups_rct", 300, 270, dict(groupshift=7)),
    ("nine_groups_palette", 300, 270, dict(groupshift=7, palette=1)),
    ("nine_groups_alpha", 300, 270, dict(groupshift=7, alpha=1)),
    ("nine_groups_two_passes", 300, 270, dict(groupshift=7, passes=2, tree=1)),
    ("nine_groups_picture_lfdequant", 300, 270, dict(groupshift=7, xybpic=1, lfdequant=X.LFDEQUANT)),
    # wide frames: a picture quantised with steps 256 times finer than the default, so that its integers leave int16. (The generator's
    # other pictures, 16-bit integers read as XYB, are Y = 128 and the like: values past 2^24 before the integer conversion, where a
    # float32 tail and a float64 model have nothing in common.)
    ("one_section_wide_16", 37, 21, dict(wide=1, bpp=16, xybpic=1, lfdequant=X.LFDEQUANT_FINE)),
    ("nine_groups_wide_16_alpha", 300, 270, dict(groupshift=7, wide=1, bpp=16, alpha=1, xybpic=1, lfdequant=X.LFDEQUANT_FINE)),
]
FRAME_IDS = [c[0] for c in FRAME_CASES]


def open_frame(gpu, data, opts, fmt=U8X4, on=True):
    fr = gpu.Frame(data, wide=bool(opts.get("wide")))
    if on:
        assert fr.set_modular_xyb(1) == ""
    fr.set_output_format(fmt)
    fr.upload(0)
    return fr


_whole = {}


def whole_decode(gpu, w, h, opts, fmt=U8X4):
    """the full decode with the switch on, once per stream and format"""
    key = (w, h, tuple(sorted(opts.items())), fmt)
    if key not in _whole:
        fr = open_frame(gpu, X.xyb_stream(w, h, **opts), opts, fmt)
        err, px = fr.decode_to_host()
        assert err == "" and fr.modular_xyb()["used"] == 1
        fr.close()
        px.setflags(write=False)
        _whole[key] = px
    return _whole[key]


@pytest.mark.parametrize("name,w,h,opts", FRAME_CASES, ids=FRAME_IDS)
def test_whole_frames(gpu, name, w, h, opts):
    data = X.xyb_stream(w, h, **opts)
    wide, bpp, nch = bool(opts.get("wide")), opts.get("bpp", 8), 4 if opts.get("alpha") else 3
    fr = open_frame(gpu, data, opts)
    try:
        said = fr.modular_xyb()
        assert said["applies"] == 1 and said["on"] == 1 and said["sample_bytes"] == (4 if wide else 2)
        err, px = fr.decode_to_host()
        assert err == "" and fr.status() == "" and fr.modular_xyb()["used"] == 1
        read = fr.read_plane_i32 if wide else fr.read_plane_i16
        c = np.stack([read(k, (h, w)) for k in range(nch)])
        xyb = fr.read_xyb(0)
        m, cc = fr.lf_dequant(), np.concatenate([fr.colour_consts()[0].reshape(9), fr.colour_consts()[1], [fr.colour_consts()[2], 0, 0]]).astype(np.float32)
        assert np.array_equal(m, {None: X.M_DEFAULT, X.LFDEQUANT: X.M_LFDEQUANT, X.LFDEQUANT_FINE: X.M_LFDEQUANT_FINE}[opts.get("lfdequant")])
        # the planes are the statement over the decoded integers
        assert np.array_equal(xyb.view(np.uint32), X.statement(c[:3], m).view(np.uint32))
        for fmt in (U8X4, U16X4):
            if fmt == U16X4:
                fr.set_output_format(U16X4)
                err, px16 = fr.decode_to_host()
                assert err == ""
            got = px if fmt == U8X4 else px16
            # the pixels are the kernel's for those planes
            kerr, fused, two, _, guard = gpu.kat_device_modular_xyb(c[:3], c[3] if nch == 4 else None, m, cc, bpp, fmt)
            assert kerr == "" and guard and np.array_equal(fused, two)
            assert np.array_equal(got, fused)
        # ... and within one level of the float64 model
        u, model = X.float64_model(c[:3], m, cc, bpp)
        d = np.abs(px[..., :3].astype(np.int32) - model.astype(np.int32))
        print("%s: against the float64 model max |delta| %d, differing %d of %d" % (name, d.max(), int((d > 0).sum()), d.size))
        assert d.max() <= 1
        assert np.array_equal(px[..., 3], X.alpha_u8(c[3], bpp) if nch == 4 else np.full((h, w), 255))
    finally:
        fr.close()


# ---------------------------------------------------------------- 3. the switch off, and the public API

@pytest.mark.parametrize("name,w,h,opts", [c for c in FRAME_CASES if not c[3].get("wide")], ids=[c[0] for c in FRAME_CASES if not c[3].get("wide")])
def test_switch_off_equals_the_reference(gpu, ref, name, w, h, opts):
    """the narrow cases only: the reference refuses an image with 32-bit buffers ("fm32"), so the two wide cases of FRAME_CASES have no
    reference bytes and are NOT covered here; what a wide frame decodes to with the switch off is tests/test_wide_modular.py's"""
    data = X.xyb_stream(w, h, **opts)
    rerr, want = ref.decode(data)
    assert rerr == ""
    for mode in (None, 0):
        fr = open_frame(gpu, data, opts, on=False)
        if mode is not None:
            assert fr.set_modular_xyb(mode) == ""
        err, px = fr.decode_to_host()
        assert err == "" and fr.modular_xyb()["used"] == 0 and fr.modular_xyb()["on"] == 0
        fr.close()
        assert np.array_equal(px, want)
    err, px = gpu.decode(data)
    assert err == "" and np.array_equal(px, want)
    assert not np.array_equal(whole_decode(gpu, w, h, opts)[..., :3], want[..., :3])


CHILD = r"""
import sys, numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import j40_amd
data = open(sys.argv[2], "rb").read()
err, px = j40_amd.decode(data)
assert err == "", err
np.save(sys.argv[3], px)
j40_amd.shutdown()
"""


def test_public_api_under_the_environment_variable(gpu, tmp_path):
    w, h, opts = 300, 270, dict(groupshift=7, alpha=1)
    data = X.xyb_stream(w, h, **opts)
    (tmp_path / "s.jxl").write_bytes(data)
    out = str(tmp_path / "px.npy")
    env = dict(os.environ, J40HIP_MODULAR_XYB="1")
    subprocess.run([sys.executable, "-c", CHILD, ROOT, str(tmp_path / "s.jxl"), out], check=True, env=env, timeout=300)
    assert np.array_equal(np.load(out), whole_decode(gpu, w, h, opts))
    err, px = gpu.decode(data, modular_xyb=True)
    assert err == "" and np.array_equal(px, whole_decode(gpu, w, h, opts))
    assert gpu.decode(synth("modular", 37, 21, X.SEED), modular_xyb=True)[0] == "Umx?"


# ---------------------------------------------------------------- 4. region, group range, scale, orientation

REGION_STREAM = (300, 270, dict(groupshift=7, alpha=1))
# groups of 128: borders at 128 and 256 both ways. Straddling one border, both, all four corners' groups; touching each edge; one pixel
RECTS = [(100, 90, 60, 70), (120, 120, 140, 140), (0, 0, 300, 1), (0, 269, 300, 1), (0, 0, 1, 270), (299, 0, 1, 270), (255, 255, 45, 15), (127, 127, 2, 2), (13, 7, 1, 1), (1, 1, 298, 268)]


@pytest.mark.parametrize("fmt", [U8X4, U16X4], ids=["u8", "u16"])
def test_region_equals_the_crop(gpu, fmt):
    w, h, opts = REGION_STREAM
    whole = whole_decode(gpu, w, h, opts, fmt)
    fr = open_frame(gpu, X.xyb_stream(w, h, **opts), opts, fmt)
    try:
        for x, y, rw, rh in RECTS:
            assert fr.set_region(x, y, rw, rh) == ""
            err, px = fr.decode_to_host()
            assert err == "" and px.shape == (rh, rw, 4) and fr.modular_xyb()["used"] == 1
            assert np.array_equal(px, whole[y:y + rh, x:x + rw]), (x, y, rw, rh)
        # the planes read-back answers for a decode of the whole frame only: after one group's decode the other groups' planes are stale
        assert fr.set_region(13, 7, 1, 1) == "" and fr.decode_to_host()[0] == ""
        with pytest.raises(gpu.J40Error) as e:
            fr.read_xyb(0)
        assert e.value.code == "rnge"
        assert fr.clear_region() == "" and fr.decode_to_host()[0] == "" and fr.read_xyb(0).shape == (3, h, w)
    finally:
        fr.close()


def test_group_range_halves_make_the_whole(gpu):
    import torch
    from j40_amd import sharding
    w, h, opts = REGION_STREAM
    whole = whole_decode(gpu, w, h, opts)
    fr = open_frame(gpu, X.xyb_stream(w, h, **opts), opts)
    try:
        out = torch.full((h, w, 4), 9, dtype=torch.uint8, device="cuda:0")
        stream = torch.cuda.current_stream().cuda_stream
        for first, count in ((0, 4), (4, 5)):     # the split falls in the middle of the second row of groups
            fr.set_group_range(first, count)
            before = out.clone()
            fr.decode(out.data_ptr(), w * 4, stream)
            torch.cuda.synchronize()
            assert fr.status() == "" and fr.modular_xyb()["used"] == 1
            mine = torch.zeros((h, w), dtype=torch.bool, device="cuda:0")
            for x0, y0, x1, y1 in sharding.range_rectangles(first, count, w, h, fr.info["group_size_shift"]):
                mine[y0:y1, x0:x1] = True
            assert torch.equal(out[~mine], before[~mine]), "a range wrote outside its own groups"
            assert np.array_equal(out[mine].cpu().numpy(), whole[mine.cpu().numpy()])
        assert np.array_equal(out.cpu().numpy(), whole)
    finally:
        fr.close()


@pytest.mark.parametrize("fmt", [U8X4, U16X4], ids=["u8", "u16"])
def test_scale_is_the_mean_of_the_full_decodes_bytes(gpu, fmt):
    from test_scale import box
    w, h, opts = 301, 271, dict(groupshift=7, alpha=1)
    whole = whole_decode(gpu, w, h, opts, fmt)
    fr = open_frame(gpu, X.xyb_stream(w, h, **opts), opts, fmt)
    try:
        for k in (1, 2):
            assert fr.set_scale(k) == ""
            err, px = fr.decode_to_host()
            assert err == "" and fr.modular_xyb()["used"] == 1 and fr.scale()["staged"] == 1
            assert np.array_equal(px, box(np.asarray(whole), k)), k
    finally:
        fr.close()


@pytest.mark.parametrize("o", [2, 5, 8])
def test_orientation_is_the_permutation(gpu, o):
    from test_orient import orient
    w, h, opts = 300, 270, dict(groupshift=7, alpha=1, orientation=o)
    stored = whole_decode(gpu, w, h, opts)
    fr = open_frame(gpu, X.xyb_stream(w, h, **opts), opts)
    try:
        assert fr.set_orientation(1) == ""
        err, px = fr.decode_to_host()
        assert err == "" and fr.orientation()["went_through_k_orient"] == 1
        assert np.array_equal(px, orient(np.asarray(stored), o))
    finally:
        fr.close()


# ---------------------------------------------------------------- 5. a sequence

@pytest.mark.parametrize("blend", [0, 2], ids=["replace", "blend"])
def test_cropped_modular_xyb_frame_over_a_vardct_frame(gpu, blend):
    from test_blend import blend_expected
    cw, ch, crop = 520, 264, (100, 30, 300, 200)
    opts = dict(frames=2, modes="v,m", xyb=1, alpha=1, alpharange=1, groupshift=7, crops=";%d,%d,%d,%d" % crop, blends="0,%d" % blend)
    data = synth("vardct", cw, ch, X.SEED, **opts)
    alone = []
    for k in range(2):
        fr = gpu.Frame(synth("vardct", cw, ch, X.SEED, **dict(opts, only=k)))
        if k == 1:
            assert fr.set_modular_xyb(1) == ""
        fr.upload(0)
        err, px = fr.decode_to_host()
        assert err == "" and fr.modular_xyb()["used"] == k
        fr.close()
        alone.append(px)
    assert alone[0].shape == (ch, cw, 4) and alone[1].shape == (crop[3], crop[2], 4)
    assert (alone[0][..., 3] == 255).all() and len(np.unique(alone[1][..., 3])) > 2   # the VarDCT frame in drop mode; the Modular frame's own alpha
    seq = gpu.Sequence(data, blend=True, modular_xyb=True)
    try:
        rows, blends = [seq.frame_info(k) for k in range(2)], [seq.frame_blend(k) for k in range(2)]
        assert [r["code"] for r in rows] == ["", ""] and rows[0]["saved"] and rows[1]["shown"] and blends[1]["mode"] == blend
        assert seq.frame(1).modular_xyb()["on"] == 1
        seq.upload(0)
        err, canvas = seq.next_to_host()
        assert err == "" and seq.status() == ("", -1)
    finally:
        seq.close()
    want = blend_expected(alone[0], alone[1], cw, ch, crop[0], crop[1], 4, False, blends[1]["mode"], blends[1]["alpha_mode"])
    assert np.array_equal(canvas, want)
    if blend:
        inside = canvas[crop[1]:crop[1] + crop[3], crop[0]:crop[0] + crop[2]]
        assert not np.array_equal(inside, alone[1]) and not np.array_equal(inside, alone[0][crop[1]:crop[1] + crop[3], crop[0]:crop[0] + crop[2]])


# ---------------------------------------------------------------- 6. Modular LF frames

LF_OPTS = dict(global_scale=4096, quant_lf=16, nocfl=1)
LF_CASES = [("wide", WIDE, dict()), ("tall", TALL, dict()), ("wide_bctx", WIDE, dict(bctx=1))]


def play(gpu, data, **switches):
    seq = gpu.Sequence(data, lf_frames=True, **switches)
    seq.upload(0)
    err, px = seq.next_to_host()
    assert err == "" and seq.status() == ("", -1)
    return seq, px


@pytest.mark.parametrize("name,size,more", LF_CASES, ids=[c[0] for c in LF_CASES])
def test_modular_lf_frame(gpu, ref, name, size, more):
    opts = dict(LF_OPTS, **more)
    if more.get("bctx"):
        assert lf_stats(size, **opts)["lfidx_distinct"] > 1   # some LF threshold splits the cells: k_lf_frame_bctx has work
    lw, lh = lf_size(size)
    # the VarDCT-LF-frame stream with the same options: slot and canvas
    seq, vardct_canvas = play(gpu, lf_stream(size, **opts))
    vardct_slot = seq.read_lf_slot(1, lw, lh)
    seq.close()
    data = lf_stream(size, lfmodular=1, **opts)
    seq, canvas = play(gpu, data, modular_xyb=True)
    try:
        assert seq.frame(0).info["is_modular"] == 1 and seq.frame(0).modular_xyb()["used"] == 1
        slot = seq.read_lf_slot(1, lw, lh)
    finally:
        seq.close()
    assert np.array_equal(slot.view(np.uint32), vardct_slot.view(np.uint32)), "%d of %d slot floats differ" % (int((slot.view(np.uint32) != vardct_slot.view(np.uint32)).sum()), slot.size)
    assert np.array_equal(canvas, vardct_canvas)
    # the twin: the ordinary stream with the same LF integers, the one leg the reference pins
    twin = lf_twin(size, **opts)
    fr = gpu.Frame(twin)
    fr.upload(0)
    err, twin_px = fr.decode_to_host()
    fr.close()
    rerr, want = ref.decode(twin)
    assert err == "" and rerr == ""
    d = int(np.abs(twin_px[..., :3].astype(np.int32) - want[..., :3].astype(np.int32)).max())
    print("twin against the reference: max |delta| =", d)
    assert d <= 1 and np.array_equal(twin_px[..., 3], want[..., 3])
    assert np.array_equal(canvas, twin_px)
    # the Python entries and the environment's route
    err, px = gpu.decode(data, lf_frames=True, modular_xyb=True)
    assert err == "" and np.array_equal(px, canvas)
    assert gpu.decode(data, lf_frames=True)[0] == "TODO"


def test_modular_lf_frame_through_the_environment(gpu, tmp_path):
    data = lf_stream(WIDE, lfmodular=1, **LF_OPTS)
    (tmp_path / "s.jxl").write_bytes(data)
    out = str(tmp_path / "px.npy")
    env = dict(os.environ, J40HIP_MODULAR_XYB="1", J40HIP_LFFRAME="1")
    subprocess.run([sys.executable, "-c", CHILD, ROOT, str(tmp_path / "s.jxl"), out], check=True, env=env, timeout=300)
    seq, canvas = play(gpu, data, modular_xyb=True)
    seq.close()
    assert np.array_equal(np.load(out), canvas)
