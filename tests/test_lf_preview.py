"""The LF preview: the 1:8 image of a VarDCT frame decoded from its LF sections alone (include/j40hip.h, INTEGRATION.md "LF preview").

Pinned to the reference: for a cell whose varblock covers only that cell, the reference keeps the cell's dequantised, smoothed LF
sample unchanged as the block's LLF coefficient (j40.h:6669-6670), llfcoeffs[c][coeffoff >> 6] with coeffoff = coeffoff_qfidx & ~15
(j40.h:6924). The pixels are the reference's colour tail (j40.h:7208-7235) and 8-bit render (j40.h:7941-7953) on that sample,
restated here in numpy float32 in the reference's operation order."""
import ctypes as C

import numpy as np
import pytest

from streams import synth, VARDCT_CASES

U16X4 = 0x0F35


def stream(name, opts):
    if name == "several_lf_groups":
        return synth("vardct", 2600, 2100, 41)
    if name == "maxlog8":
        return synth("vardct", 776, 520, 31, maxlog=8, bctx=1)
    return synth("vardct", 520, 264, 41, **opts)


STREAMS = [(n, o) for n, o in VARDCT_CASES] + [("several_lf_groups", None), ("maxlog8", None)]
IDS = [s[0] for s in STREAMS]


def ref_single_cells(ref, data):
    """{(row, col) of the frame's LF grid: [X, Y, B] float32} from the reference's LLF coefficients, for every cell whose varblock
    covers that cell alone"""
    from refdec import RefStage
    rs = RefStage(ref, data)
    out = {}
    try:
        for gg in range(rs.info["num_lf_groups"]):
            gi = rs.lf_group_info(gg)
            blocks = rs.plane(gg, 0)
            vb = blocks & 0xFFFFF
            coeffoff = rs.varblocks(gg)[0] & ~15
            llf = [rs.llf(gg, c) for c in range(3)]
            ids, counts = np.unique(vb, return_counts=True)
            single = set(ids[counts == 1].tolist())
            for y, x in zip(*np.nonzero(np.isin(vb, list(single)))):
                k = coeffoff[vb[y, x]] >> 6
                out[(gi["top"] // 8 + int(y), gi["left"] // 8 + int(x))] = np.array([llf[c][k] for c in range(3)], np.float32)
    finally:
        rs.close()
    return out


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---------------------------------------------------------------- without a GPU

@pytest.mark.parametrize("name,opts", STREAMS, ids=IDS)
def test_host_lf_plane_matches_reference(built, ref, name, opts):
    import j40_amd
    data = stream(name, opts)
    fr = j40_amd.Frame(data)
    planes = [fr.lf_plane(c) for c in range(3)]
    w8, h8 = fr.lf_size()
    fr.close()
    assert all(p.shape == (h8, w8) for p in planes)
    cells = ref_single_cells(ref, data)
    assert len(cells) > w8 * h8 // 8, len(cells)   # (maxlog8: most cells lie under larger varblocks)
    rows, cols = np.array([k[0] for k in cells]), np.array([k[1] for k in cells])
    expect = np.stack([cells[k] for k in cells])
    got = np.stack([planes[c][rows, cols] for c in range(3)], -1)
    assert np.array_equal(bits(got), bits(expect)), (name, int((bits(got) != bits(expect)).sum()))


def bare(data):
    return data[:2] == b"\xff\x0a"


@pytest.mark.parametrize("name,opts", STREAMS, ids=IDS)
def test_lf_only_parse_of_a_truncated_stream(built, name, opts):
    import j40_amd
    data = stream(name, opts)
    full = j40_amd.Frame(data)
    lf_end = full.lf_end()
    planes = [full.lf_plane(c) for c in range(3)]
    nsec = j40_amd.lib().j40hip_frame_num_sections(full.h)
    cs = full.codestream_size
    full.close()
    assert nsec > 1 and lf_end < cs, (lf_end, cs)
    if not bare(data):   # (containers must be complete; the whole stream with the flag gives the same planes)
        fr = j40_amd.Frame(data, lf_only=True)
        assert fr.lf_end() == lf_end and all(np.array_equal(fr.lf_plane(c), planes[c]) for c in range(3))
        fr.close()
        return
    fr = j40_amd.Frame(data[:lf_end], lf_only=True)
    assert fr.lf_end() == lf_end
    for c in range(3):
        assert np.array_equal(bits(fr.lf_plane(c)), bits(planes[c])), c
    assert lib_after_frame_status(fr) == ""
    fr.close()
    # cut into the last LF section in byte order: "shrt"
    for cut in (16, 64):
        with pytest.raises(j40_amd.J40Error) as e:
            j40_amd.Frame(data[:lf_end - cut], lf_only=True)
        assert e.value.code == "shrt", (cut, e.value.code)
    # the full parse of the prefix still fails -- unless a permuted TOC stored HfGlobal in front of the last LF section: then the host's
    # part passes and the pass groups are what is missing (the GPU tests decode such a frame)
    try:
        j40_amd.Frame(data[:lf_end]).close()
        parsed = True
    except j40_amd.J40Error as e:
        assert e.code == "shrt"
        parsed = False
    assert not parsed or name.startswith("permuted")


def lib_after_frame_status(fr):
    import j40_amd
    return j40_amd.err4(j40_amd.lib().j40hip_frame_after_frame_status(fr.h))


@pytest.mark.parametrize("name,opts", [s for s in STREAMS if bare(stream(*s))], ids=[s[0] for s in STREAMS if bare(stream(*s))])
def test_streamed_lf_only_parse_asks_for_no_more_than_lf_end(built, name, opts):
    import j40_amd
    data = stream(name, opts)
    full = j40_amd.Frame(data)
    lf_end = full.lf_end()
    planes = [full.lf_plane(c) for c in range(3)]
    full.close()
    log = []
    fr = j40_amd.Frame.parse_streamed(data, step=1, flags=j40_amd.PARSE_LF_ONLY, log=log)
    asked = log[:-1]   # (the last entry is parse_streamed's own: the rest of the stream, once the parse has returned)
    assert max(asked) <= lf_end, (max(asked), lf_end)
    assert all(np.array_equal(bits(fr.lf_plane(c)), bits(planes[c])) for c in range(3))
    fr.close()
    log = []   # (without the flag the same parse goes on to HfGlobal)
    fr = j40_amd.Frame.parse_streamed(data, step=1, flags=0, log=log)
    assert max(log[:-1]) > lf_end or name.startswith("permuted")
    fr.close()


def test_lf_only_parse_refuses_modular(built):
    import j40_amd
    for data in (synth("modular", 600, 300, 71), synth("modular", 256, 256, 71)):
        with pytest.raises(j40_amd.J40Error) as e:
            j40_amd.Frame(data, lf_only=True)
        assert e.value.code == "TODO"


def test_single_section_lf_end_is_the_whole_codestream(built):
    """(the generator writes no single-section VarDCT frame -- the reference's section order quirk --, so the rule is shown on a
    single-section Modular frame, whose full parse reports lf_end all the same)"""
    import j40_amd
    data = synth("modular", 256, 256, 71)
    fr = j40_amd.Frame(data)
    assert j40_amd.lib().j40hip_frame_num_sections(fr.h) == 1
    assert fr.lf_end() == fr.codestream_size == len(data)
    fr.close()


def test_lf_size_rounds_up(built):
    import j40_amd
    for w, h in ((521, 263), (520, 264), (257, 129)):
        fr = j40_amd.Frame(synth("vardct", w, h, 41))
        assert fr.lf_size() == ((w + 7) // 8, (h + 7) // 8)
        assert fr.lf_plane(0).shape == ((h + 7) // 8, (w + 7) // 8)
        fr.close()


def test_lf_plane_and_consts_entry_points(built):
    import j40_amd
    fr = j40_amd.Frame(stream("default", {}))
    with pytest.raises(j40_amd.J40Error) as e:
        fr.lf_plane(3)
    assert e.value.code == "rnge"
    m, bias, it, kx, kb = fr.colour_consts()
    assert m.shape == (3, 3) and bias.shape == (3,) and it > 0 and kb == 1.0   # (base_corr_b's default, no factor in this stream)
    fr.close()


def test_lf_only_frame_refuses_the_full_decode_without_gpu(built):
    """the refusal comes before anything needs a device: "Ulf?" on every full-decode entry point"""
    import j40_amd
    L = j40_amd.lib()
    data = stream("default", {})
    fr = j40_amd.Frame(data[:j40_amd.Frame(data).lf_end()], lf_only=True)
    host = np.zeros((fr.height, fr.width, 4), np.uint8)
    assert j40_amd.err4(L.j40hip_frame_decode(fr.h, None, fr.width * 4, None)) == "Ulf?"
    assert j40_amd.err4(L.j40hip_frame_decode_timed(fr.h, None, fr.width * 4, None, np.zeros(3, np.float32).ctypes.data)) == "Ulf?"
    assert j40_amd.err4(L.j40hip_frame_decode_to_host(fr.h, host.ctypes.data, fr.width * 4)) == "Ulf?"
    err = C.c_uint32()
    hs = (C.c_void_p * 1)(fr.h)
    assert not L.j40hip_batch_create(hs, 1, C.byref(err)) and j40_amd.err4(err.value) == "Ulf?"
    assert not host.any()
    fr.close()


# ---------------------------------------------------------------- the colour tail, restated (numpy float32, no contraction)

def restate(ref, planes, consts, bpp):
    """the reference's per-sample tail on LF samples [3][h8, w8]: chroma from luma (j40.h:7158, 7170), XYB -> linear (7208-7220) ->
    sRGB -> level (7221-7235);
    returns the int levels [h8, w8, 3] as the reference's int16 casts leave them, clamped to [0, maxpixel] as its render does"""
    m, bias, it, kx, kb = consts
    f32 = np.float32
    x, y, b = (np.asarray(p, f32) for p in planes)
    x, b = x + y * kx, b + y * kb   # chroma from luma on the LF sample (j40.h:7158, 7170)
    cbrt = [f32(ref.lib.ref_kat_cbrtf(float(bias[c]))) for c in range(3)]
    itscale = f32(255.0) / f32(it)
    p = [y + x, y - x, b]
    s = []
    for c in range(3):
        pp = p[c] - cbrt[c]
        s.append(((pp * pp) * pp + bias[c]) * itscale)
    levels = []
    fn = ref.lib.ref_kat_srgb_i16
    for c in range(3):
        v = (s[0] * m[c, 0] + s[1] * m[c, 1]) + s[2] * m[c, 2]
        lv = np.fromiter((fn(float(t), bpp) for t in v.reshape(-1)), np.int64, v.size).reshape(v.shape)
        levels.append(np.clip(lv, 0, (1 << bpp) - 1))
    return np.stack(levels, -1)


def to_u8(level, bpp):
    maxpixel = (1 << bpp) - 1
    return (level * 255 + (1 << (bpp - 1))) // maxpixel


def to_u16(level, bpp):
    maxpixel = (1 << bpp) - 1
    return (level * 65535 + (1 << (bpp - 1))) // maxpixel


def level_of_u16(u16, bpp):
    return (u16.astype(np.int64) * ((1 << bpp) - 1) + 32767) // 65535


def box_mean_u8(rgba, w8, h8):
    h, w = rgba.shape[:2]
    pad = np.zeros((h8 * 8, w8 * 8, 3), np.float64)
    cnt = np.zeros((h8 * 8, w8 * 8, 1), np.float64)
    pad[:h, :w] = rgba[..., :3]
    cnt[:h, :w] = 1
    s = pad.reshape(h8, 8, w8, 8, 3).sum((1, 3))
    n = cnt.reshape(h8, 8, w8, 8, 1).sum((1, 3))
    return s / n


# the forward-encoded 8K stream of bench.py and the bound on |preview - 8x8 box mean of the reference's full decode|, mean over the
# RGB samples: measured on the CPU from the restatement (0.31 levels), set at twice that
K8 = (7680, 4320, 3)
BOX_MEAN_BOUND = 0.62


def test_restated_preview_against_box_mean_of_reference_decode(built, ref):
    import j40_amd
    data = synth("vardct", *K8, forward=1)
    fr = j40_amd.Frame(data[:j40_amd.Frame(data).lf_end()], lf_only=True)
    w8, h8 = fr.lf_size()
    assert (w8, h8) == (960, 540)
    lv = restate(ref, [fr.lf_plane(c) for c in range(3)], fr.colour_consts(), fr.info["bpp"])
    fr.close()
    err, full = ref.decode(data)
    assert err == ""
    d = np.abs(to_u8(lv, 8) - box_mean_u8(full, w8, h8))
    assert d.mean() <= BOX_MEAN_BOUND, d.mean()


# ---------------------------------------------------------------- on the GPU

@pytest.fixture(scope="module")
def gpu(built):
    import j40_amd
    assert j40_amd.device_count() > 0, "the gpu tests need a HIP device"
    return j40_amd


def check_preview(gpu, ref, fr, data, fmt):
    """read_lf == lf_plane bit for bit; the pixels against the restatement (from lf_plane) and against the reference's LLF on single-cell
    cells: every sample within one level; returns (pixels, unequal samples vs the restatement)"""
    bpp = fr.info["bpp"]
    planes = [fr.lf_plane(c) for c in range(3)]
    for c in range(3):
        assert np.array_equal(bits(fr.read_lf(c)), bits(planes[c])), c
    fr.set_output_format(fmt)
    px = fr.decode_lf_to_host()
    w8, h8 = fr.lf_size()
    assert px.shape == (h8, w8, 4)
    lv = restate(ref, planes, fr.colour_consts(), bpp)
    if fmt == U16X4:
        assert px.dtype == np.uint16 and np.all(px[..., 3] == 65535)
        got = level_of_u16(px[..., :3], bpp)
        assert np.array_equal(to_u16(got, bpp), px[..., :3])   # (every u16 is the rule applied to a level)
        want = lv
    else:
        assert px.dtype == np.uint8 and np.all(px[..., 3] == 255)
        got = px[..., :3].astype(np.int64)
        want = to_u8(lv, bpp)
    d = np.abs(got - want)
    assert d.max() <= 1, (d.max(), int((d > 0).sum()))
    # against the reference's own LLF on single-cell cells
    cells = ref_single_cells(ref, data)
    rows, cols = np.array([k[0] for k in cells]), np.array([k[1] for k in cells])
    vals = np.stack([cells[k] for k in cells])
    rl = restate(ref, [vals[:, 0], vals[:, 1], vals[:, 2]], fr.colour_consts(), bpp)
    rwant = rl if fmt == U16X4 else to_u8(rl, bpp)
    assert np.abs(got[rows, cols] - rwant).max() <= 1
    return px, int((d > 0).sum())


@pytest.mark.gpu
@pytest.mark.parametrize("name,opts", STREAMS, ids=IDS)
def test_device_preview_matches_host_and_reference(gpu, ref, name, opts):
    data = stream(name, opts)
    for fmt in (gpu.J40_U8X4, U16X4):
        fr = gpu.Frame(data)
        fr.upload(0)
        _, ndiff = check_preview(gpu, ref, fr, data, fmt)
        print("%s %s: samples unequal to the restatement: %d" % (name, "u16" if fmt == U16X4 else "u8", ndiff))
        if fmt == gpu.J40_U8X4 and fr.info["bpp"] == 8:
            assert ndiff == 0
        fr.close()


@pytest.mark.gpu
def test_device_preview_8k(gpu, ref):
    data = synth("vardct", *K8, forward=1)
    err, full = ref.decode(data)
    assert err == ""
    for fmt in (gpu.J40_U8X4, U16X4):
        fr = gpu.Frame(data[:gpu.Frame(data).lf_end()], lf_only=True)
        fr.upload(0)
        px, ndiff = check_preview(gpu, ref, fr, data, fmt)
        print("8K %s: samples unequal to the restatement: %d" % ("u16" if fmt == U16X4 else "u8", ndiff))
        assert px.shape == (540, 960, 4)
        if fmt == gpu.J40_U8X4:
            assert ndiff == 0
            assert np.abs(px[..., :3].astype(np.float64) - box_mean_u8(full, 960, 540)).mean() <= BOX_MEAN_BOUND
        fr.close()


@pytest.mark.gpu
def test_truncated_stream_preview_equals_whole_stream_preview(gpu):
    import torch
    for data in (synth("vardct", *K8, forward=1), stream("permuted_toc_two_passes", dict(permute=1, passes=2))):
        whole = gpu.Frame(data)
        lf_end = whole.lf_end()
        whole.upload(0)
        for fmt in (gpu.J40_U8X4, U16X4):
            whole.set_output_format(fmt)
            want = whole.decode_lf_to_host()
            for kw in (dict(), dict(lf_device=0)):
                fr = gpu.Frame(data[:lf_end], lf_only=True, **kw)
                for c in range(3):
                    assert np.array_equal(bits(fr.lf_plane(c)), bits(whole.lf_plane(c))), (kw, c)
                fr.set_output_format(fmt)
                fr.upload(0)
                w8, h8 = fr.lf_size()
                pxb = 8 if fmt == U16X4 else 4
                out = torch.zeros((h8, w8 * pxb), dtype=torch.uint8, device="cuda:0")
                fr.decode_lf(out.data_ptr(), w8 * pxb, torch.cuda.current_stream().cuda_stream)
                torch.cuda.synchronize()
                got = out.cpu().numpy().view(np.uint16 if fmt == U16X4 else np.uint8).reshape(h8, w8, 4)
                assert np.array_equal(got, want), (kw, fmt)
                fr.close()
        whole.close()


@pytest.mark.gpu
def test_many_frames_in_one_launch(gpu):
    import torch
    sizes = [(520, 264, dict()), (776, 520, dict(maxlog=8, bctx=1)), (264, 200, dict(bpp=12, cfl=1)), (1000, 257, dict(bpp=15)),
             (521, 263, dict()), (2600, 2100, dict())]
    datas = [synth("vardct", w, h, 60 + i, **o) for i, (w, h, o) in enumerate(sizes * 3)]
    frames, alone = [], []
    for i, d in enumerate(datas):
        lf_only = i % 2 == 1
        fr = gpu.Frame(d[:gpu.Frame(d).lf_end()] if lf_only else d, lf_only=lf_only)
        fr.upload(0)
        alone.append(fr.decode_lf_to_host())
        frames.append(fr)
    assert len(frames) >= 16
    stream = torch.cuda.current_stream().cuda_stream
    outs = [torch.full((f.lf_size()[1], f.lf_size()[0] * 4), 7, dtype=torch.uint8, device="cuda:0") for f in frames]
    strides = [f.lf_size()[0] * 4 for f in frames]
    assert gpu.frames_decode_lf(frames, [o.data_ptr() for o in outs], strides, stream) == ""
    torch.cuda.synchronize()
    for f, o, a in zip(frames, outs, alone):
        assert np.array_equal(o.cpu().numpy().reshape(a.shape), a)
    # refused calls launch nothing: the sentinel-filled buffers stay as they are
    for o in outs:
        o.fill_(7)
    assert gpu.frames_decode_lf(frames, [o.data_ptr() for o in outs], [s - 4 for s in strides], stream) == "rnge"
    frames[3].set_output_format(U16X4)
    assert gpu.frames_decode_lf(frames, [o.data_ptr() for o in outs], strides, stream) == "Uof?"
    frames[3].set_output_format(gpu.J40_U8X4)
    mod = gpu.Frame(synth("modular", 600, 300, 71))
    mod.upload(0)
    assert gpu.frames_decode_lf(frames[:2] + [mod], [o.data_ptr() for o in outs[:3]], strides[:3], stream) == "TODO"
    notup = gpu.Frame(datas[0])
    assert gpu.frames_decode_lf(frames[:1] + [notup], [o.data_ptr() for o in outs[:2]], strides[:2], stream) == "!gpu"
    torch.cuda.synchronize()
    assert all(bool((o == 7).all()) for o in outs)
    for f in frames + [mod, notup]:
        f.close()
    # the module-level helpers: one launch for many streams, the same pixels
    err, many = gpu.decode_lf_many(datas[:6])
    assert err == "" and all(np.array_equal(m, a) for m, a in zip(many, alone[:6]))
    err, one = gpu.decode_lf(datas[2], U16X4)
    assert err == "" and one.dtype == np.uint16 and one.shape == alone[2].shape
    assert gpu.decode_lf(synth("modular", 600, 300, 71))[0] == "TODO"


@pytest.mark.gpu
def test_preview_does_not_interfere_with_the_full_decode(gpu):
    import torch
    for data in (stream("default", {}), synth("vardct", 4096, 2304, 72), synth("vardct", 2600, 2100, 71, forward=1)):
        for flags_kw in (dict(), dict(lf_device=0)):
            fr = gpu.Frame(data, **flags_kw)
            fr.upload(0)
            err, a = fr.decode_to_host()
            assert err == ""
            w8, h8 = fr.lf_size()
            out = torch.zeros((h8, w8 * 4), dtype=torch.uint8, device="cuda:0")
            fr.decode_lf(out.data_ptr(), w8 * 4, torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            p1 = out.cpu().numpy().copy()
            err, b = fr.decode_to_host()
            assert err == "" and np.array_equal(a, b)
            p2 = fr.decode_lf_to_host()
            assert np.array_equal(p1.reshape(p2.shape), p2)
            fr.close()
    lf = gpu.Frame(stream("default", {}), lf_only=True)
    lf.upload(0)
    assert lf.decode_to_host()[0] == "Ulf?"
    lf.close()
