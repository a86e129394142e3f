"""Blend modes of frame sequences on the device (J40HIP_SEQ_BLEND, k_frame_blend; include/j40hip.h).

The kernel alone goes through the table and the exact cases of tests/test_blend.py, byte for byte: both sides are IEEE float32 with no
contraction and correctly rounded division. The playback follows tests/test_frames_gpu.py: every coded frame is decoded alone by this
library and held against the reference (equal for Modular, within one level for VarDCT), the frames are then composed by
test_blend.blend_expected, and the canvases of next_to_host equal the result byte for byte. The composition itself has no reference
code behind it: PARITY UNPINNED (tests/test_blend.py's docstring)."""
import numpy as np
import pytest

from streams import synth
from test_frames import SEED, CROPS, U8X4, U16X4, assert_same_sections, compose_cases, Guarded
from test_frames_gpu import decode_alone, stream_opts, public_api_frames, VARDCT_ALPHA, VARDCT_ALPHA_CROPS
from test_blend import (REPLACE, BLEND, MULADD, blend_expected, run_blend_case, table_pairs, assert_table_covers, exact_cases, hand_pixel)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu(built):
    import j40_amd
    assert j40_amd.device_count() > 0, "the gpu tests need a HIP device"
    return j40_amd


# ---------------------------------------------------------------- 5. the kernel alone

def test_blend_kernel_alone(gpu):
    import torch

    class OnDevice(Guarded):
        def place(self):
            self.dev = torch.empty(len(self.raw), dtype=torch.uint8, device="cuda:0")
            return self.dev.data_ptr()

        def send(self):
            self.dev.copy_(torch.from_numpy(self.raw))

        def fetch(self):
            self.raw[:] = self.dev.cpu().numpy()

    L = gpu.lib()
    stream = torch.cuda.current_stream().cuda_stream

    def call(out, out_stride, src, src_stride, frm, frm_stride, cw, ch, x0, y0, w, h, lo, hi, pb, cmode, amode):
        assert L.j40hip_kat_device_blend(out, out_stride, src, src_stride, frm, frm_stride, cw, ch, x0, y0, w, h, lo, hi, U16X4 if pb == 8 else U8X4, cmode, amode, stream) == 0
        torch.cuda.synchronize()

    cases = compose_cases()
    assert_table_covers(cases)
    for n, (case, (cmode, amode)) in enumerate(zip(cases, table_pairs(cases))):
        run_blend_case(case, call, n, cmode, amode, OnDevice)
    for cmode, amode in ((BLEND, BLEND), (MULADD, REPLACE)):
        for n, case in enumerate(cases):
            run_blend_case(case, call, n, cmode, amode, OnDevice)

    def call_arrays(out, out_stride, src, src_stride, frm, frm_stride, *rest):
        """the exact cases hand numpy arrays over: copies in device memory, the output's doubling as the source where they are one"""
        d_out, d_frm = torch.from_numpy(out).to("cuda:0"), torch.from_numpy(frm).to("cuda:0")
        d_src = None if src is None else d_out if src is out else torch.from_numpy(src).to("cuda:0")
        call(d_out.data_ptr(), out_stride, None if d_src is None else d_src.data_ptr(), src_stride, d_frm.data_ptr(), frm_stride, *rest)
        out[:] = d_out.cpu().numpy()

    for pb in (4, 8):
        exact_cases(call_arrays, pb)
    hand_pixel(call_arrays)
    # what the hook refuses before anything is launched: j40hip_kat_device_compose's list, and a mode outside 0..4
    buf = torch.zeros(4096, dtype=torch.uint8, device="cuda:0")
    p = buf.data_ptr()
    bad = [(p, 64, None, 0, p + 2048, 64, 16, 4, 0, 0, 4, 4, 0, 0, 0x1234, 2, 2, stream), (p, 63, None, 0, p + 2048, 64, 16, 4, 0, 0, 4, 4, 0, 0, U8X4, 2, 2, stream),
           (p, 64, None, 0, p + 2048, 12, 16, 4, 0, 0, 4, 4, 0, 0, U8X4, 2, 2, stream), (p + 2, 64, None, 0, p + 2048, 64, 16, 4, 0, 0, 4, 4, 0, 0, U8X4, 2, 2, stream),
           (p, 128, p, 256, p + 2048, 64, 16, 4, 0, 0, 4, 4, 0, 0, U8X4, 2, 2, stream), (p, 64, None, 0, None, 64, 16, 4, 0, 0, 4, 4, 0, 0, U8X4, 2, 2, stream),
           (p, 64, None, 0, p + 2048, 64, 16, 4, 0, 0, 4, 4, 0, 0, U8X4, 5, 0, stream), (p, 64, None, 0, p + 2048, 64, 16, 4, 0, 0, 4, 4, 0, 0, U8X4, 0, -1, stream)]
    assert [gpu.err4(L.j40hip_kat_device_blend(*a)) for a in bad] == ["Ufm?", "rnge", "rnge", "rnge", "rnge", "rnge", "rnge", "rnge"]


# ---------------------------------------------------------------- 6. playback

def numpy_play(rows, blends, alone, cw, ch, pb, a0):
    """the displayed canvases as the header and the formulas define them: [(coded frame, canvas)]"""
    slots, shown = {}, []
    for k, (r, b, px) in enumerate(zip(rows, blends, alone)):
        raw = px.view(np.uint8).reshape(px.shape[0], px.shape[1], pb)
        canvas = blend_expected(slots.get(b["src"]), raw, cw, ch, r["x0"], r["y0"], pb, a0, b["mode"], b["alpha_mode"])
        if r["saved"]:
            slots[r["save_as_reference"]] = canvas
        if r["shown"]:
            shown.append((k, canvas))
    return shown


def play_and_check(gpu, ref, mode, cw, ch, opts, fmt=U8X4, alpha=False, a0=False, blended=None):
    """test_frames_gpu.play_and_check's scheme with the switch on; returns the rows' blend entries and the canvases"""
    pb = 8 if fmt == U16X4 else 4
    data = synth(mode, cw, ch, SEED, **opts)
    seq = gpu.Sequence(data, blend=True)
    rows = [seq.frame_info(k) for k in range(seq.num_frames)]
    blends = [seq.frame_blend(k) for k in range(seq.num_frames)]
    assert len(rows) == opts["frames"] and all(r["code"] == "" for r in rows)
    assert blended is None or [b["blended"] for b in blends] == blended
    for k, r in enumerate(rows):
        assert_same_sections(data, r, mode, cw, ch, opts, k)
    alone = [decode_alone(gpu, mode, cw, ch, opts, k, fmt, alpha, ref) for k in range(len(rows))]
    want = numpy_play(rows, blends, alone, cw, ch, pb, a0)
    assert len(want) == seq.num_shown
    seq.set_output_format(fmt)
    if alpha:
        for k in range(seq.num_frames):
            assert seq.frame(k).set_alpha(1) == ""
    seq.upload(0)
    got = []
    for turn in range(2):   # ... and again after a rewind
        for k, canvas in want:
            err, px = seq.next_to_host()
            assert err == "", (k, err)
            assert np.array_equal(px.view(np.uint8).reshape(ch, cw, pb), canvas), "the canvas of coded frame %d (turn %d)" % (k, turn)
            got.append(px)
        assert seq.next_to_host()[0] == "Useq"
        assert seq.status() == ("", -1)
        seq.rewind()
    seq.close()
    return blends, got[:len(want)]


# alpharange=1: the alpha plane holds 0, full scale and everything between
MODULAR = dict(groupshift=7, alpha=1, alpharange=1)
VARDCT_KEEP = dict(VARDCT_ALPHA, alpharange=1)
KINDS = {"modular": ("modular", MODULAR, 300, 200, CROPS, False), "vardct": ("vardct", VARDCT_KEEP, 520, 264, VARDCT_ALPHA_CROPS, True)}


def kind_opts(kind, colour, ec=None):
    """frame 0 replaces and is saved into slot 1; frame 1 is blended over slot 1 into slot 2, frame 2 over slot 2 into slot 1, a fourth
    one over slot 1; every frame is shown"""
    mode, base, cw, ch, crops, alpha = KINDS[kind]
    n = len(crops)
    o = dict(blends=",".join(["0"] + [str(colour)] * (n - 1)), saves=",".join(str(s) for s in [1, 2, 1][:n - 1] + [0]), srcs=",".join(str(s) for s in [0, 1, 2, 1][:n]))
    if ec is not None:
        o["ecblends"] = ",".join(["0"] + [str(ec)] * (n - 1))
    return mode, cw, ch, stream_opts(base, crops, **o), alpha


@pytest.mark.parametrize("blend", [1, 2, 3, 4], ids=["add", "blend", "muladd", "mul"])
@pytest.mark.parametrize("kind", ["modular", "vardct"])
def test_every_mode(gpu, ref, kind, blend):
    mode, cw, ch, opts, alpha = kind_opts(kind, blend)
    blends, got = play_and_check(gpu, ref, mode, cw, ch, opts, alpha=alpha, a0=True, blended=[0] + [1] * (opts["frames"] - 1))
    assert all((b["mode"], b["alpha_mode"]) == (blend, blend) for b in blends[1:])
    a = np.concatenate([g[..., 3].ravel() for g in got])
    assert a.min() == 0 and a.max() == 255 and ((a > 0) & (a < 255)).any()   # transparent, opaque and in between all met


@pytest.mark.parametrize("kind", ["modular", "vardct"])
def test_colour_blend_alpha_replace(gpu, ref, kind):
    mode, cw, ch, opts, alpha = kind_opts(kind, BLEND, ec=REPLACE)
    blends, _ = play_and_check(gpu, ref, mode, cw, ch, opts, alpha=alpha, a0=True)
    assert all((b["mode"], b["alpha_mode"], b["blended"]) == (BLEND, REPLACE, 1) for b in blends[1:])


@pytest.mark.parametrize("kind", ["modular", "vardct"])
def test_full_frame_layers(gpu, ref, kind):
    """a layer stack without animation: every layer covers the canvas exactly and is blended over the slot it is saved into -- the
    staging image for an exact frame"""
    mode, base, cw, ch, _, alpha = KINDS[kind]
    opts = stream_opts(base, [None, None, None], anim=False, saves="0,0,0", blends="0,2,2")
    blends, got = play_and_check(gpu, ref, mode, cw, ch, opts, alpha=alpha, a0=True, blended=[0, 1, 1])
    assert len(got) == 1
    top = decode_alone(gpu, mode, cw, ch, opts, 2, alpha=alpha)
    assert not np.array_equal(got[0], top) and np.array_equal(got[0][top[..., 3] == 255], top[top[..., 3] == 255])


@pytest.mark.parametrize("kind", ["modular", "vardct"])
def test_aliased_and_never_saved(gpu, ref, kind):
    mode, base, cw, ch, crops, alpha = KINDS[kind]
    # frame 1 is blended over slot 1 while it is saved into slot 1: k_frame_blend's out == src
    play_and_check(gpu, ref, mode, cw, ch, stream_opts(base, crops[:3], saves="1,1,0", srcs="0,1,1", blends="0,2,2"), alpha=alpha, a0=True, blended=[0, 1, 1])
    # the source slot was never saved: blended over the empty pixel (0, 0, 0, 0), which gives the frame's pixel where its alpha is not 0
    opts = stream_opts(base, crops[1:3], srcs="2,2", blends="2,2")
    _, got = play_and_check(gpu, ref, mode, cw, ch, opts, alpha=alpha, a0=True, blended=[1, 1])
    assert tuple(got[0][ch - 1, cw - 1]) == (0, 0, 0, 0)


def test_u16(gpu, ref):
    mode, cw, ch, opts, alpha = kind_opts("modular", BLEND)
    play_and_check(gpu, ref, mode, cw, ch, opts, a0=True)   # (the frames alone against the reference, at 8 bits)
    _, got = play_and_check(gpu, ref, mode, cw, ch, opts, fmt=U16X4, a0=True)
    assert got[-1].dtype == np.uint16 and got[-1][..., 3].max() == 65535
    mode, cw, ch, opts, alpha = kind_opts("vardct", MULADD, ec=BLEND)
    play_and_check(gpu, ref, mode, cw, ch, opts, alpha=alpha, a0=True)
    play_and_check(gpu, ref, mode, cw, ch, opts, fmt=U16X4, alpha=alpha, a0=True)


def test_vardct_drop_mode_blend_is_replace(gpu, ref):
    """an alpha that is not rendered is full scale everywhere: Blend gives the canvases of the same stream written with Replace"""
    mode, cw, ch, opts, _ = kind_opts("vardct", BLEND)
    _, got = play_and_check(gpu, ref, mode, cw, ch, opts, blended=[0, 1, 1])
    _, replaced = play_and_check(gpu, ref, mode, cw, ch, dict(opts, blends="0,0,0"), blended=[0, 0, 0])
    assert len(got) == len(replaced) == 3
    for a, b in zip(got, replaced):
        assert np.array_equal(a, b) and a[..., 3].min() == 255


# ---------------------------------------------------------------- 7. public API and Python

def test_public_api_and_python(gpu, ref, monkeypatch):
    mode, cw, ch, opts, _ = kind_opts("modular", BLEND)
    data = synth(mode, cw, ch, SEED, **opts)
    monkeypatch.delenv("J40HIP_BLEND", raising=False)
    _, want = play_and_check(gpu, ref, mode, cw, ch, opts, a0=True)
    frames, (num, den, loops) = gpu.decode_frames(data, blend=True)
    assert (num, den, loops) == (10, 1, 0) and len(frames) == len(want) == 4
    for (px, _), b in zip(frames, want):
        assert np.array_equal(px, b)
    with pytest.raises(gpu.J40Error) as e:
        gpu.decode_frames(data)
    assert e.value.code == "TODO"
    monkeypatch.setenv("J40HIP_FRAMES", "1")
    frames, err, _ = public_api_frames(gpu, data)   # without the blend switch: frame 0, then TODO at the blended frame
    assert len(frames) == 1 and err == "TODO" and np.array_equal(frames[0], want[0])
    monkeypatch.setenv("J40HIP_BLEND", "1")
    frames, err, _ = public_api_frames(gpu, data)
    assert err == "" and len(frames) == 4
    for a, b in zip(frames, want):
        assert np.array_equal(a, b)
