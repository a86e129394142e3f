"""Frame sequences on the device (j40hip_sequence_next, k_frame_compose; include/j40hip.h): every displayed canvas of an animation or a
layered still equals, bit for bit, the numpy composition of THIS library's decodes of the frames alone (the generator's only=k streams),
and those decodes hold against the reference at the bar the suite uses everywhere: equal for Modular, within one level for VarDCT.
Together the two pin the composed canvases to the reference. tests/test_frames.py has the index and the CPU build of the composition."""
import ctypes as C

import numpy as np
import pytest

from streams import synth
from test_frames import (SEED, CROPS, DURATIONS, U8X4, U16X4, crops_opt, only_stream, assert_same_sections, compose_cases, compose_expected,
                         run_compose_case, Guarded)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu(built):
    import j40_amd
    assert j40_amd.device_count() > 0, "the gpu tests need a HIP device"
    return j40_amd


def stream_opts(base, crops, anim=True, durations=None, **more):
    o = dict(base, frames=len(crops), crops=crops_opt(crops))
    if anim:
        o.update(anim=1, durations=",".join(str(d) for d in (durations or [1] * len(crops))))
    o.update(more)
    return o


_alone = {}


def decode_alone(gpu, mode, w, h, opts, k, fmt=U8X4, alpha=False, ref=None):
    """this library's decode of coded frame k written alone (cached); with `ref`, held against the reference first: (ii)"""
    key = (mode, w, h, tuple(sorted((kk, v) for kk, v in opts.items() if kk != "container")), k, fmt, alpha)
    if key not in _alone:
        data = only_stream(mode, w, h, opts, k)
        fr = gpu.Frame(data)
        if alpha:
            assert fr.set_alpha(1) == ""
        fr.set_output_format(fmt)
        fr.upload(0)
        err, px = fr.decode_to_host()
        fr.close()
        assert err == ""
        if ref is not None and fmt == U8X4:
            rerr, want = ref.decode(data)
            assert rerr == ""
            d = np.abs(px[..., :3].astype(np.int32) - want[..., :3].astype(np.int32)).max()
            print("frame %d alone against the reference: max |delta| = %d" % (k, d))
            assert d <= (0 if mode == "modular" else 1)
            if not alpha:
                assert np.array_equal(px[..., 3], want[..., 3])
        _alone[key] = px
    return _alone[key]


def numpy_play(rows, alone, cw, ch, pb, a0):
    """the displayed canvases as the header defines them: [(coded frame, canvas)]"""
    slots, shown = {}, []
    for k, (r, px) in enumerate(zip(rows, alone)):
        raw = px.view(np.uint8).reshape(px.shape[0], px.shape[1], pb)
        canvas = compose_expected(slots.get(r["src"]), raw, cw, ch, r["x0"], r["y0"], pb, a0)
        if r["saved"]:
            slots[r["save_as_reference"]] = canvas
        if r["shown"]:
            shown.append((k, canvas))
    return shown


def play_and_check(gpu, ref, mode, cw, ch, opts, fmt=U8X4, alpha=False, a0=False):
    """(i) and (ii) for one stream; returns the sequence's rows and the canvases"""
    pb = 8 if fmt == U16X4 else 4
    data = synth(mode, cw, ch, SEED, **opts)
    seq = gpu.Sequence(data)
    rows = [seq.frame_info(k) for k in range(seq.num_frames)]
    assert all(r["code"] == "" for r in rows)
    for k, r in enumerate(rows):
        assert_same_sections(data, r, mode, cw, ch, opts, k)
    alone = [decode_alone(gpu, mode, cw, ch, opts, k, fmt, alpha, ref) for k in range(len(rows))]
    want = numpy_play(rows, alone, cw, ch, pb, a0)
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
    return rows, got[:len(want)]


MODULAR = dict(groupshift=7, alpha=1)
VARDCT = dict(passes=2)          # (a frame of one group gets several sections: the generator does not write single-section VarDCT frames)
VARDCT_ALPHA = dict(alpha=1)     # one pass, so every frame is at least two groups wide


def test_animation_modular(gpu, ref):
    opts = stream_opts(MODULAR, CROPS, durations=DURATIONS)
    rows, got = play_and_check(gpu, ref, "modular", 300, 200, opts, a0=True)
    assert [r["shown"] for r in rows] == [1, 0, 1, 1]
    # the frame of duration 0 is never returned, and lies under the next one: a pixel of its rectangle outside frame 2's
    f1 = decode_alone(gpu, "modular", 300, 200, opts, 1)
    x, y = 120, 90
    assert np.array_equal(got[1][y, x], f1[y - 21, x - 37]) and not np.array_equal(got[0][y, x], got[1][y, x])


def test_animation_modular_u16_at_12_bits(gpu, ref):
    """(no alpha here, A0 is full scale: the reference refuses an alpha channel whose depth differs from the colour channels', the
    generator writes an 8-bit one, so a 12-bit Modular animation with alpha has no oracle. u16 output with alpha is checked at 8 bits
    in test_public_api.)"""
    opts = stream_opts(dict(groupshift=7, bpp=12), CROPS, durations=DURATIONS)
    play_and_check(gpu, ref, "modular", 300, 200, opts, fmt=U16X4)
    play_and_check(gpu, ref, "modular", 300, 200, opts, fmt=U8X4)


VARDCT_CROPS = [None, (8, 8, 256, 128), (37, 21, 131, 77)]            # full; on block boundaries; off them
VARDCT_ALPHA_CROPS = [None, (8, 8, 264, 128), (37, 21, 331, 77)]      # ... two groups wide


@pytest.mark.parametrize("fmt", [U8X4, U16X4], ids=["u8", "u16"])
def test_animation_vardct_drop_mode(gpu, ref, fmt):
    play_and_check(gpu, ref, "vardct", 520, 264, stream_opts(VARDCT, VARDCT_CROPS), fmt=fmt)


def test_animation_vardct_keep_alpha(gpu, ref):
    opts = stream_opts(VARDCT_ALPHA, VARDCT_ALPHA_CROPS)
    play_and_check(gpu, ref, "vardct", 520, 264, opts, alpha=True, a0=True)
    play_and_check(gpu, ref, "vardct", 520, 264, opts)   # the same stream in drop mode: opaque
    # no full frame under the crops: the empty pixel shows, A0 = 0 in keep mode and full scale in drop mode; alpha comes from the frame inside
    opts = stream_opts(VARDCT_ALPHA, VARDCT_ALPHA_CROPS[1:], srcs="0,1")
    rows, kept = play_and_check(gpu, ref, "vardct", 520, 264, opts, alpha=True, a0=True)
    assert tuple(kept[0][0, 0]) == (0, 0, 0, 0) and tuple(kept[1][263, 519]) == (0, 0, 0, 0)
    inside = decode_alone(gpu, "vardct", 520, 264, opts, 0, alpha=True)
    assert np.array_equal(kept[0][8:136, 8:272, 3], inside[..., 3]) and inside[..., 3].min() < 255
    rows, dropped = play_and_check(gpu, ref, "vardct", 520, 264, opts)
    assert tuple(dropped[0][0, 0]) == (0, 0, 0, 255) and dropped[0][..., 3].min() == 255


def test_layers(gpu, ref):
    for mode, base, cw, ch, crops in (("modular", MODULAR, 300, 200, CROPS[:3]), ("vardct", VARDCT, 520, 264, VARDCT_CROPS)):
        rows, got = play_and_check(gpu, ref, mode, cw, ch, stream_opts(base, crops, anim=False, saves="0,0,0"), a0=mode == "modular")
        assert len(got) == 1 and [r["saved"] for r in rows] == [1, 1, 0]
    # a slot never saved gives the empty pixel: frame 1 draws over slot 2, which nobody wrote
    rows, got = play_and_check(gpu, ref, "modular", 300, 200, stream_opts(MODULAR, CROPS[1:3], srcs="0,2"), a0=True)
    assert tuple(got[1][199, 299]) == (0, 0, 0, 0) and tuple(got[1][150, 150]) == (0, 0, 0, 0)


def test_slots_and_aliasing(gpu, ref):
    three = [None, (37, 21, 130, 90), (-20, -10, 100, 80)]
    # frame 1 reads slot 1 and is saved into slot 2; frame 2 reads slot 2
    play_and_check(gpu, ref, "modular", 300, 200, stream_opts(MODULAR, three, durations=[0, 0, 1], saves="1,2,0", srcs="0,1,2"), a0=True)
    # frame 1 reads slot 1 while it is saved into slot 1: the compose kernel's out == src
    play_and_check(gpu, ref, "modular", 300, 200, stream_opts(MODULAR, three, durations=[0, 0, 1], saves="1,1,0", srcs="0,1,1"), a0=True)
    # shown and saved at once, drawing over its own slot, in both formats
    for fmt in (U8X4, U16X4):
        play_and_check(gpu, ref, "vardct", 520, 264, stream_opts(VARDCT, VARDCT_CROPS, durations=[2, 2, 2], saves="3,3,0", srcs="0,3,3"), fmt=fmt)


def test_compose_kernel_alone(gpu):
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

    def call(out, out_stride, src, src_stride, frm, frm_stride, cw, ch, x0, y0, w, h, lo, hi, pb):
        assert L.j40hip_kat_device_compose(out, out_stride, src, src_stride, frm, frm_stride, cw, ch, x0, y0, w, h, lo, hi, U16X4 if pb == 8 else U8X4, stream) == 0
        torch.cuda.synchronize()

    for n, case in enumerate(compose_cases()):
        run_compose_case(case, call, n, OnDevice)
    # what the hook refuses before anything is launched
    buf = torch.zeros(4096, dtype=torch.uint8, device="cuda:0")
    p = buf.data_ptr()
    bad = [(p, 64, None, 0, p + 2048, 64, 16, 4, 0, 0, 4, 4, 0, 0, 0x1234, stream), (p, 63, None, 0, p + 2048, 64, 16, 4, 0, 0, 4, 4, 0, 0, U8X4, stream),
           (p, 64, None, 0, p + 2048, 12, 16, 4, 0, 0, 4, 4, 0, 0, U8X4, stream), (p + 2, 64, None, 0, p + 2048, 64, 16, 4, 0, 0, 4, 4, 0, 0, U8X4, stream),
           (p, 128, p, 256, p + 2048, 64, 16, 4, 0, 0, 4, 4, 0, 0, U8X4, stream), (p, 64, None, 0, None, 64, 16, 4, 0, 0, 4, 4, 0, 0, U8X4, stream)]
    assert [gpu.err4(L.j40hip_kat_device_compose(*a)) for a in bad] == ["Ufm?", "rnge", "rnge", "rnge", "rnge", "rnge"]


def test_all_coded_frames_in_one_batch(gpu):
    import torch
    seq = gpu.Sequence(synth("vardct", 520, 264, SEED, **stream_opts(VARDCT, VARDCT_CROPS)))
    seq.upload(0)
    frames = [seq.frame(k) for k in range(seq.num_frames)]
    singles = []
    for fr in frames:
        err, px = fr.decode_to_host()
        assert err == ""
        singles.append(px)
    outs = [torch.zeros((fr.height, fr.width, 4), dtype=torch.uint8, device="cuda:0") for fr in frames]
    batch = gpu.Batch(frames)
    batch.decode([o.data_ptr() for o in outs], [o.shape[1] * 4 for o in outs], torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    for k, (fr, o, px) in enumerate(zip(frames, outs, singles)):
        assert fr.status() == "" and px.shape == ((264, 520, 4) if k == 0 else (VARDCT_CROPS[k][3], VARDCT_CROPS[k][2], 4))
        assert np.array_equal(o.cpu().numpy(), px), k
    batch.close()
    seq.close()


def public_api_frames(gpu, data, fmt=U8X4):
    """j40_next_frame until it returns 0: (the canvases, the error code, the error string)"""
    img = gpu.from_memory(data)
    img.output_format(gpu.J40_RGBA, fmt)
    out = []
    while img.next_frame():
        out.append((img.frame_pixels_u16x4 if fmt == U16X4 else img.frame_pixels_u8x4)()[0].copy())
        assert len(out) < 64
    assert img.next_frame() == 0
    err, text = img.error(), img.error_string()
    img.free()
    return out, err, text


def test_public_api(gpu, ref, monkeypatch):
    opts = stream_opts(MODULAR, CROPS, durations=DURATIONS)
    data = synth("modular", 300, 200, SEED, **opts)
    monkeypatch.delenv("J40HIP_FRAMES", raising=False)
    frames, err, text = public_api_frames(gpu, data)
    assert frames == [] and err == "TODO" and text == ref.error_string(data)
    monkeypatch.setenv("J40HIP_FRAMES", "1")
    for fmt in (U8X4, U16X4):
        rows, want = play_and_check(gpu, ref, "modular", 300, 200, opts, fmt=fmt, a0=True)
        frames, err, text = public_api_frames(gpu, data, fmt)
        assert err == "" and len(frames) == len(want) == 3
        for a, b in zip(frames, want):
            assert np.array_equal(a, b)
    # a stream whose first frame is its last takes the single-frame route, switch or not: crop-sized pixels for a cropped one
    alone = only_stream("modular", 300, 200, opts, 1)
    frames, err, _ = public_api_frames(gpu, alone)
    assert err == "" and len(frames) == 1 and np.array_equal(frames[0], decode_alone(gpu, "modular", 300, 200, opts, 1))
    # the format cannot change between frames
    img = gpu.from_memory(data)
    assert img.next_frame() == 1
    assert img.output_format(gpu.J40_RGBA, U16X4) == "Uof?" and img.next_frame() == 1
    img.free()


def test_python_decode_frames(gpu, ref):
    opts = stream_opts(MODULAR, CROPS, durations=DURATIONS)
    rows, want = play_and_check(gpu, ref, "modular", 300, 200, opts, a0=True)
    frames, (num, den, loops) = gpu.decode_frames(synth("modular", 300, 200, SEED, **opts))
    assert (num, den, loops) == (10, 1, 0) and [d for _, d in frames] == [3, 2, 1]
    for (px, _), b in zip(frames, want):
        assert np.array_equal(px, b)
    with pytest.raises(gpu.J40Error) as e:
        gpu.decode_frames(synth("modular", 300, 200, SEED, **MODULAR))
    assert e.value.code == "Usq?"


def test_a_damaged_section_in_frame_2(gpu, ref, monkeypatch):
    opts = stream_opts(VARDCT, [None, (8, 8, 256, 128), (37, 21, 131, 77), None], durations=[1, 1, 1, 1])
    data = bytearray(synth("vardct", 520, 264, SEED, **opts))
    rows, want = play_and_check(gpu, ref, "vardct", 520, 264, opts)
    seq = gpu.Sequence(bytes(data))
    r = seq.frame_info(2)
    seq.close()
    for at in range(r["end"] - 40, r["end"] - 8):   # the tail of frame 2's last pass-group section
        data[at] ^= 0x5A
    seq = gpu.Sequence(bytes(data))
    seq.upload(0)
    for k in range(2):
        err, px = seq.next_to_host()
        assert err == "" and np.array_equal(px, want[k]), k
    err, px = seq.next_to_host()
    assert err != "" and err != "Useq" and px is None
    code, frame = seq.status()
    assert frame == 2 and code == err
    seq.close()
    monkeypatch.setenv("J40HIP_FRAMES", "1")
    frames, api_err, _ = public_api_frames(gpu, bytes(data))
    assert len(frames) == 2 and api_err == err
    assert np.array_equal(frames[0], want[0]) and np.array_equal(frames[1], want[1])


@pytest.mark.parametrize("mode,base,cw,ch", [("modular", MODULAR, 300, 200), ("vardct", VARDCT, 520, 264)], ids=["modular", "vardct"])
def test_a_frame_that_does_not_parse_ends_the_index_at_upload(gpu, ref, mode, base, cw, ch):
    """the index reads headers and TOCs only, so a frame whose first section is damaged is found when it is parsed, at the upload: the
    index then ends at its row as it does for a refused frame, the frames before it play, and Frames handed out for the rows behind it
    (and, at close, every one) lose their handles"""
    crops = [None, (37, 21, 130, 90), (-20, -10, 100, 80), None]
    opts = stream_opts(base, crops, durations=[1, 1, 1, 1])
    data = bytearray(synth(mode, cw, ch, SEED, **opts))
    rows, want = play_and_check(gpu, ref, mode, cw, ch, opts, a0=mode == "modular")
    for at in range(rows[1]["first_section"], rows[1]["first_section"] + 8):
        data[at] = 0xFF
    seq = gpu.Sequence(bytes(data))
    assert (seq.num_frames, seq.num_shown) == (4, 4) and [seq.frame_info(k)["code"] for k in range(4)] == [""] * 4
    first, behind = seq.frame(0), seq.frame(2)
    with pytest.raises(gpu.J40Error) as e:
        seq.frame(1)
    code = e.value.code
    assert code not in ("", "TODO")
    seq.upload(0)
    assert (seq.num_frames, seq.num_shown) == (2, 1)
    assert seq.frame_info(1)["code"] == code and not seq.frame_info(1)["shown"] and seq.frame_info(2)["end"] == 0
    assert behind.h is None and first.h is not None
    err, px = seq.next_to_host()
    assert err == "" and np.array_equal(px, want[0])
    assert seq.next_to_host() == (code, None)
    seq.close()
    assert first.h is None
