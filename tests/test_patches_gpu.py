"""Patches on the device (include/j40hip.h, J40HIP_SEQ_PATCHES; k_patch_blend). PARITY UNPINNED: the reference holds no code for patches
(j40.h:6262), so the feature is pinned piece by piece, every piece byte for byte:
  - the kernel alone and the planes a sequence leaves (j40hip_frame_read_xyb, stage 3) against numpy's float32 statement of the rule,
    applied to planes the library makes WITHOUT the feature: the main frame written without its dictionary (patchtwin=1) and decoded alone,
    and the reference-only frames written as regular frames (only=k) and decoded alone;
  - the pixels against k_xyb_to_rgba (or k_colour_tail) alone over those expected planes;
  - two anchors that reach the reference: placements of mode None change nothing, so the canvas is the twin's, which the reference
    decodes; one Replace patch over the whole frame shows the reference frame, whose only=k stream the reference decodes. Both at the
    suite's bar for VarDCT frames (within one level, A equal).
tests/test_patches.py has the index, the refusals and the CPU build."""
import numpy as np
import pytest

import patch_streams as P
from patch_streams import patch_synth, seq_opts, main_refs, flat, bits, NONE, REPLACE, ADD, MUL
from test_scale import box
from test_blend import blend_expected
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


def open_seq(gpu, data, fmt=U8X4, restoration=None, **kw):
    seq = gpu.Sequence(data, patches=True, modular_xyb=True, **kw)
    seq.set_output_format(fmt)
    if restoration is not None:
        for k in range(seq.num_frames):
            seq.frame(k).set_restoration(restoration)
    seq.upload(0)
    return seq


def play(seq):
    err, px = seq.next_to_host()
    assert err == "" and seq.status() == ("", -1)
    assert seq.next_to_host()[0] == "Useq"
    return px


KINDS = {
    "vardct": dict(main="v", mode="vardct", w=P.VW, h=P.VH, sizes=[P.REF_V, P.REF_M], modes=["v", "m"], more=GAB),
    "modular": dict(main="m", mode="modular", w=P.MW, h=P.MH, sizes=[P.REF_M, (60, 34)], modes=["m", "m"], more={}),
}
_cache = {}


def case(gpu, kind, restoration=0):
    """the stream of `kind` with the shared dictionary, and everything the feature is held against, made once: the slots' planes and the
    main frame's planes from decodes that do not involve patches, numpy's patches over them, and k_xyb_to_rgba's pixels of the result"""
    key = (kind, restoration)
    if key in _cache:
        return _cache[key]
    K = KINDS[kind]
    refs = main_refs(K["w"], K["h"], K["sizes"][0], K["sizes"][1])
    opts = seq_opts(K["main"], refs, K["sizes"], K["modes"], **K["more"])
    data = patch_synth(K["mode"], K["w"], K["h"], **opts)
    slots = {}
    for k, m in enumerate(K["modes"]):
        alone = patch_synth(K["mode"], K["w"], K["h"], **dict(opts, only=k))
        slots[k + 1] = vardct_planes_alone(gpu, alone)[1 if restoration else 0] if m == "v" else modular_planes_alone(gpu, alone)
    twin = patch_synth(K["mode"], K["w"], K["h"], **dict(opts, only=len(K["modes"]), patchtwin=1))
    own = vardct_planes_alone(gpu, twin)[1 if restoration else 0] if K["main"] == "v" else modular_planes_alone(gpu, twin)
    want = P.apply_patches(own, slots, flat(refs))
    assert not np.array_equal(want, own)
    fr = gpu.Frame(twin)
    consts = cc15(fr)
    fr.close()
    pixels = {}
    for fmt in (U8X4, U16X4):
        code, px = gpu.kat_device_xyb_to_rgba(want, consts, 8, fmt)
        assert code == ""
        pixels[fmt] = px
    _cache[key] = dict(K, refs=refs, opts=opts, data=data, slots=slots, own=own, planes=want, pixels=pixels, twin=twin, consts=consts)
    return _cache[key]


# ---------------------------------------------------------------- 1. the kernel alone

def test_kernel_alone_equals_numpy(gpu):
    rng = np.random.default_rng(11)
    slots, cases = P.kat_cases(rng)
    planes = rng.uniform(-1.0, 2.0, (3, P.MH, P.MW)).astype(np.float32)
    results = {}
    for name, placements in cases:
        code, got, tiles = gpu.kat_device_patches(planes, [slots.get(k) for k in range(4)], placements)
        assert code == "" and tiles == len(P.tiles_touched(placements, P.MW, P.MH)), name
        assert np.array_equal(bits(got), bits(P.apply_patches(planes, slots, placements))), name
        results[name] = got
    assert not np.array_equal(results["replace_then_add"], results["add_then_replace"])
    # the host's check stands in front of the kernel: an empty slot, a rectangle past its slot, a placement past the planes
    none = [slots.get(k) for k in range(4)]
    assert gpu.kat_device_patches(planes, none, [(0, 0, 8, 8, 0, 0, 1, REPLACE, 0)])[0] == "ptno"
    assert gpu.kat_device_patches(planes, none, [(0, 0, 8, 8, 40, 26, 3, REPLACE, 0)])[0] == "ptch"
    assert gpu.kat_device_patches(planes, none, [(P.MW - 7, 0, 8, 8, 0, 0, 3, ADD, 0)])[0] == "ptch"


# ---------------------------------------------------------------- 2. the reference slots

@pytest.mark.parametrize("restoration", [0, 1], ids=["plain", "filters_on"])
def test_reference_slots_hold_the_frames_planes(gpu, restoration):
    """a VarDCT and a Modular reference-only frame: what the slot holds is what the same frame makes written as a regular frame and decoded alone"""
    c = case(gpu, "vardct", restoration)
    seq = open_seq(gpu, c["data"], restoration=restoration)
    try:
        play(seq)
        for slot, size in ((1, P.REF_V), (2, P.REF_M)):
            got = seq.read_ref_slot(slot)
            assert got.shape == (3, size[1], size[0])
            assert np.array_equal(bits(got), bits(c["slots"][slot])), slot
        with pytest.raises(gpu.J40Error):
            seq.read_ref_slot(0)
        assert [seq.frame_patches(k)["xyb_slot"] for k in range(3)] == [1, 2, -1]
    finally:
        seq.close()


# ---------------------------------------------------------------- 3. planes and pixels through the sequence

@pytest.mark.parametrize("kind", ["vardct", "modular"])
def test_planes_and_pixels_through_the_sequence(gpu, kind):
    c = case(gpu, kind)
    seq = open_seq(gpu, c["data"])
    try:
        px = play(seq)
        fr = seq.frame(2)
        got = fr.read_xyb(3)
        assert np.array_equal(bits(got), bits(c["planes"])), "%d samples differ" % int((bits(got) != bits(c["planes"])).sum())
        assert px.shape == (c["h"], c["w"], 4) and np.array_equal(px, c["pixels"][U8X4])
        pt = seq.frame_patches(2)
        assert pt["launches"] == 1 and pt["tiles"] == len(P.tiles_touched(flat(c["refs"]), c["w"], c["h"]))
        # a region and 1:2 of the frame's own handle, which keeps its slots: cut from, and averaged over, the full-size picture
        for (x, y, w, h) in ((0, 0, 64, 32), (57, 31, 83, 71), (c["w"] - 31, c["h"] - 17, 31, 17)):
            assert fr.set_region(x, y, w, h) == ""
            err, part = fr.decode_to_host()
            assert err == "" and np.array_equal(part, c["pixels"][U8X4][y:y + h, x:x + w]), (x, y, w, h)
        assert fr.clear_region() == "" and fr.set_scale(1) == ""
        err, half = fr.decode_to_host()
        assert err == "" and np.array_equal(half, box(c["pixels"][U8X4], 1))
        assert fr.set_scale(0) == ""
        # rewind, and a second playback: the same bytes (the handle alone is "ptno" in between: its slots are unbound)
        seq.rewind()
        assert fr.decode_to_host()[0] == "ptno"
        assert np.array_equal(play(seq), px)
        assert seq.frame_patches(2)["launches"] >= 2
    finally:
        seq.close()
    assert np.array_equal(gpu.decode_frames(c["data"], patches=True, modular_xyb=True)[0][0][0], px)
    err, again = gpu.decode(c["data"], patches=True, modular_xyb=True)
    assert err == "" and np.array_equal(again, px)
    err, half2 = gpu.decode(c["data"], patches=True, modular_xyb=True, scale=1)
    assert err == "" and np.array_equal(half2, half)


@pytest.mark.parametrize("kind", ["vardct", "modular"])
def test_u16_pixels(gpu, kind):
    c = case(gpu, kind)
    seq = open_seq(gpu, c["data"], fmt=U16X4)
    try:
        px = play(seq)
        assert px.dtype == np.uint16 and np.array_equal(px, c["pixels"][U16X4])
    finally:
        seq.close()


def test_restoration_on(gpu):
    """the patches go onto the FILTERED planes (and the slots hold filtered planes): after the filters, before the tail"""
    c, plain = case(gpu, "vardct", 1), case(gpu, "vardct", 0)
    assert not np.array_equal(c["own"], plain["own"])
    seq = open_seq(gpu, c["data"], restoration=1)
    try:
        px = play(seq)
        assert np.array_equal(bits(seq.frame(2).read_xyb(3)), bits(c["planes"]))
        assert np.array_equal(px, c["pixels"][U8X4]) and not np.array_equal(px, plain["pixels"][U8X4])
    finally:
        seq.close()


@pytest.mark.parametrize("kind", ["vardct", "modular"])
def test_colour_mode(gpu, kind):
    """the signalled colour space: the same planes, k_colour_tail alone over them (Display P3 primaries, PQ)"""
    K = KINDS[kind]
    refs = main_refs(K["w"], K["h"], K["sizes"][0], K["sizes"][1])
    opts = seq_opts(K["main"], refs, K["sizes"], K["modes"], primaries=11, tf=16, **K["more"])
    data = patch_synth(K["mode"], K["w"], K["h"], **opts)
    plain = case(gpu, kind)     # (the encoding changes no coefficient: the planes are the sRGB stream's)
    seq = open_seq(gpu, data, colour=True)
    try:
        px = play(seq)
        fr = seq.frame(2)
        assert np.array_equal(bits(fr.read_xyb(3)), bits(plain["planes"]))
        cc, enc, lum, _, bpp, _, _ = tail_inputs(gpu, fr)
        code, want = gpu.kat_device_colour_tail(plain["planes"], cc, enc, lum, bpp, U8X4)
        assert code == "" and np.array_equal(px, want)
        assert not np.array_equal(px, plain["pixels"][U8X4])
    finally:
        seq.close()


# ---------------------------------------------------------------- 4. the anchors that reach the reference

def against_the_reference(ref, data, px):
    rerr, want = ref.decode(data)
    assert rerr == ""
    d = int(np.abs(px[..., :3].astype(np.int32) - want[..., :3].astype(np.int32)).max())
    print("against the reference: max |delta| =", d)
    assert d <= 1 and np.array_equal(px[..., 3], want[..., 3])


def test_anchor_placements_of_mode_none_change_nothing(gpu, ref):
    c = case(gpu, "vardct")
    refs = [r[:5] + ([(x, y, NONE, 0) for (x, y, _, _) in r[5]],) for r in c["refs"]]
    opts = seq_opts("v", refs, c["sizes"], c["modes"], **GAB)
    seq = open_seq(gpu, patch_synth("vardct", P.VW, P.VH, **opts))
    try:
        px = play(seq)
        pt = seq.frame_patches(2)
        assert pt["has_patches"] == 1 and pt["placements"] == len(flat(refs)) and pt["tiles"] == 0 and pt["launches"] == 0
        assert np.array_equal(bits(seq.frame(2).read_xyb(3)), bits(c["own"]))
    finally:
        seq.close()
    twin = patch_synth("vardct", P.VW, P.VH, **dict(opts, only=2, patchtwin=1))
    assert twin == c["twin"]
    fr = gpu.Frame(twin)
    fr.upload(0)
    err, alone = fr.decode_to_host()
    fr.close()
    assert err == "" and np.array_equal(px, alone)
    against_the_reference(ref, twin, alone)


def test_anchor_one_replace_patch_shows_the_reference_frame(gpu, ref):
    refs = [(1, 0, 0, P.VW, P.VH, [(0, 0, REPLACE, 0)])]
    opts = seq_opts("v", refs, [(P.VW, P.VH)], ["v"], **GAB)
    seq = open_seq(gpu, patch_synth("vardct", P.VW, P.VH, **opts))
    try:
        px = play(seq)
        assert seq.frame_patches(1)["tiles"] == ((P.VW + 63) // 64) * ((P.VH + 31) // 32)
    finally:
        seq.close()
    against_the_reference(ref, patch_synth("vardct", P.VW, P.VH, **dict(opts, only=0)), px)


# ---------------------------------------------------------------- 5. composition, and streams without patches

def test_a_blended_crop_composes_as_ever(gpu):
    """reference-only frame, a full frame saved into slot 0, then a cropped frame with patches added onto it: the canvas is what the
    composition makes of the frame's own (patched) pixels"""
    x0, y0, w, h = 20, 10, 264, 200
    refs = [(1, 2, 3, 16, 24, [(70, 40, REPLACE, 0), (5, 8, ADD, 0), (w - 16, h - 24, MUL, 1)])]
    opts = dict(frames=3, types="2,0,0", crops="0,0,264,40;;%d,%d,%d,%d" % (x0, y0, w, h), saves="1,0,0", srcs="0,0,0", blends="0,0,1",
                patches=";;" + P.dictionary(refs), **GAB)
    data = patch_synth("vardct", P.VW, P.VH, **opts)
    seq = open_seq(gpu, data, blend=True)
    try:
        px = play(seq)
        assert seq.frame_blend(2)["blended"] == 1 and seq.frame_patches(2)["launches"] == 1
        err, under = seq.frame(1).decode_to_host()
        assert err == ""
        err, own = seq.frame(2).decode_to_host()
        assert err == "" and own.shape == (h, w, 4)
        slot = seq.read_ref_slot(1)
        planes = seq.frame(2).read_xyb(3)
    finally:
        seq.close()
    assert np.array_equal(px, blend_expected(under, own, P.VW, P.VH, x0, y0, 4, False, 1, 0))
    # ... and those pixels are the patched planes': the frame written alone without its dictionary, numpy's patches, k_xyb_to_rgba
    twin = patch_synth("vardct", P.VW, P.VH, **dict(opts, only=2, patchtwin=1))
    want = P.apply_patches(vardct_planes_alone(gpu, twin)[0], {1: slot}, flat(refs))
    assert np.array_equal(bits(planes), bits(want))
    fr = gpu.Frame(twin)
    code, pixels = gpu.kat_device_xyb_to_rgba(want, cc15(fr), 8, U8X4)
    fr.close()
    assert code == "" and np.array_equal(own, pixels)


@pytest.mark.parametrize("mode,w,h,more", [("vardct", P.VW, P.VH, {}), ("modular", P.MW, P.MH, dict(xyb=1))], ids=["vardct", "modular"])
def test_a_stream_without_patches_is_untouched_by_the_switch(gpu, mode, w, h, more):
    data = patch_synth(mode, w, h, frames=2, crops=";10,20,%d,100" % (w - 30), saves="0,0", **more)
    canvases = []
    for patches in (False, True):
        seq = gpu.Sequence(data, patches=patches, modular_xyb=True)
        try:
            seq.upload(0)
            canvases.append(play(seq))
            for k in range(seq.num_frames):
                pt = seq.frame_patches(k)
                assert (pt["has_patches"], pt["stored_xyb"], pt["tiles"], pt["launches"]) == (0, 0, 0, 0)
                with pytest.raises(gpu.J40Error):
                    seq.frame(k).read_xyb(3)
        finally:
            seq.close()
    assert np.array_equal(canvases[0], canvases[1])


def test_what_a_frame_with_patches_refuses(gpu):
    """a partial group range, a batch and the many-frames LF preview are "TODO" for the handle of a frame with patches; the handle of a
    frame without a dictionary in the same sequence takes all three"""
    import torch
    c = case(gpu, "vardct")
    seq = open_seq(gpu, c["data"])
    try:
        px = play(seq)
        patched, plain = seq.frame(2), seq.frame(0)
        out = torch.zeros((c["h"], c["w"] * 4), dtype=torch.uint8, device="cuda:0")
        for fr, code in ((patched, "TODO"), (plain, "")):
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
        # nothing of that changed what the handle decodes
        err, again = patched.decode_to_host()
        assert err == "" and np.array_equal(again, px)
    finally:
        seq.close()


def test_public_api(gpu, monkeypatch):
    """J40HIP_PATCHES=1 sends such a stream through a sequence; without it the ten-function API says what it always said"""
    c = case(gpu, "vardct")
    for name in ("J40HIP_PATCHES", "J40HIP_MODULAR_XYB", "J40HIP_FRAMES"):
        monkeypatch.delenv(name, raising=False)
    frames, err, _ = public_api_frames(gpu, c["data"])
    assert frames == [] and err == "TODO"
    monkeypatch.setenv("J40HIP_PATCHES", "1")
    monkeypatch.setenv("J40HIP_MODULAR_XYB", "1")
    for fmt in (U8X4, U16X4):
        frames, err, _ = public_api_frames(gpu, c["data"], fmt)
        assert err == "" and len(frames) == 1 and np.array_equal(frames[0], c["pixels"][fmt])
    # a stream without a reference-only frame or patches stays on its usual route
    plain = patch_synth("vardct", P.VW, P.VH, **GAB)
    frames, err, _ = public_api_frames(gpu, plain)
    monkeypatch.delenv("J40HIP_PATCHES")
    monkeypatch.delenv("J40HIP_MODULAR_XYB")
    want, err2, _ = public_api_frames(gpu, plain)
    assert err == err2 == "" and np.array_equal(frames[0], want[0])
