"""Reduced-size decode on the device (j40hip_frame_set_scale, include/j40hip.h): every 1:2 and 1:4 image equals box() of the full
decode of the same handle, bit for bit -- through the fused pixel kernels (the three VarDCT families, the Modular pack kernel), through
k_downscale where the frame is staged (restoration filters, keep-alpha), in batches, through the pipeline and the public API -- and
box() of the reference's pixels at the bar the full decode has. box() and the CPU side are in tests/test_scale.py."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from streams import synth, ROOT, STRESS_SEED
from test_scale import box, U8X4, U16X4, SEED

pytestmark = pytest.mark.gpu

SIZES = [(779, 517), (774, 518)]     # W mod 4 = 3, H mod 4 = 1; both mod 4 = 2: every edge-cell size at both shifts
VARDCT_STREAMS = [
    ("default", dict()), ("cfl", dict(cfl=1)), ("passes", dict(passes=2)), ("bpp12", dict(bpp=12)), ("dq", dict(dq=2)),
    ("large", dict(density=1, decay=1, global_scale=73728, maxlog=8)),
]
MODULAR_SIZES = [(601, 303), (257, 255)]
MODULAR_STREAMS = [
    ("plain", dict()), ("rgba_prefix_lz77", dict(alpha=1, prefix=1, lz77=1)), ("palette", dict(palette=1)), ("bpp10", dict(bpp=10, tree=1)),
    ("bpp14_wp_rct", dict(bpp=14, tree=2, rct=13)), ("squeeze", dict(squeeze=1, tree=1)),
    ("full_range_noise", dict(rct=-1, noise=40000, range="-32768,32767", tree=4)),   # samples outside [0, maxpixel]: the clamp comes before the mean
]
BATCH_SIZES = [(779, 517), (774, 518), (520, 264), (264, 520), (9, 5)]


def opts_for(w, h):
    """the generator writes no single-section VarDCT frame: the 9 x 5 one has two passes"""
    return dict(passes=2) if (w, h) == (9, 5) else dict()


@pytest.fixture(scope="module")
def gpu(built):
    import j40_amd
    assert j40_amd.device_count() > 0, "the gpu tests need a HIP device"
    return j40_amd


def varied(full):
    """the test's own test: at least a quarter of the 2 x 2 cells of the picture hold two different values in some channel"""
    H, W = full.shape[:2]
    a = full[:H // 2 * 2, :W // 2 * 2].reshape(H // 2, 2, W // 2, 2, 4)
    if a.size == 0:
        return True
    differs = (a.max(axis=(1, 3)) != a.min(axis=(1, 3))).any(axis=-1)
    return differs.mean() >= 0.25


def open_frame(gpu, data, fmt=U8X4, alpha=False, restoration=None):
    fr = gpu.Frame(data)
    if alpha:
        assert fr.set_alpha(1) == ""
    if restoration is not None:
        fr.set_restoration(restoration)
    fr.set_output_format(fmt)
    fr.upload(0)
    return fr


def full_and_scaled(gpu, data, fmt=U8X4, shifts=(1, 2), **mode):
    """one handle: its full decode, then its decode at every shift with scale() afterwards: full, {k: (pixels, scale dict)}"""
    fr = open_frame(gpu, data, fmt, **mode)
    err, full = fr.decode_to_host()
    assert err == "", err
    assert varied(full), "a flat picture proves nothing here: pick another stream"
    got = {}
    for k in shifts:
        assert fr.set_scale(k) == ""
        err, px = fr.decode_to_host()
        assert err == "", err
        got[k] = (px, fr.scale())
    assert fr.set_scale(0) == ""
    err, again = fr.decode_to_host()
    assert err == "" and np.array_equal(again, full), "shift 0 afterwards is the full decode again"
    fr.close()
    return full, got


# ---------------------------------------------------------------- 1, 2: the fused VarDCT kernels

FUSED_CASES = [(n, o, w, h) for n, o in VARDCT_STREAMS for w, h in SIZES] + [("passes", dict(passes=2), 9, 5)]   # ... and a frame smaller than a cell row


@pytest.mark.parametrize("fmt", [U8X4, U16X4], ids=["u8x4", "u16x4"])
@pytest.mark.parametrize("name,opts,w,h", FUSED_CASES, ids=["%s_%dx%d" % (c[0], c[2], c[3]) for c in FUSED_CASES])
def test_fused_vardct_equals_box_of_full(gpu, name, opts, w, h, fmt):
    full, got = full_and_scaled(gpu, synth("vardct", w, h, SEED, **opts), fmt)
    for k, (px, sc) in got.items():
        assert px.shape == box(full, k).shape and px.dtype == full.dtype
        assert np.array_equal(px, box(full, k)), (name, w, h, k)
        assert (sc["shift"], sc["staged"], sc["staging_bytes"]) == (k, 0, 0)
        assert (px[..., 3] == (255 if fmt == U8X4 else 65535)).all()


def test_every_kernel_family_ran(gpu):
    """the streams above put varblocks into k_vardct_dct, the 8x8 specials and k_vardct_large"""
    families = {"dct": 0, "special": 0, "large": 0}
    for name, opts in VARDCT_STREAMS:
        for w, h in SIZES:
            try:
                d = gpu.StageDump(synth("vardct", w, h, SEED, **opts))
            except gpu.J40Error as e:
                assert e.code == "TODO", e.code     # a stream the batched path does not take has no dump
                continue
            cs = d.sorted_varblocks()[2]
            d.close()
            for sel in range(27):
                n = int(cs[sel + 1] - cs[sel])
                families["large" if sel >= 21 else "special" if sel in (1, 2, 3, 12, 13, 14, 15, 16, 17) else "dct"] += n
    print("varblocks per kernel family:", families)
    assert all(v > 0 for v in families.values()), families


@pytest.mark.parametrize("name,opts", VARDCT_STREAMS, ids=[n for n, _ in VARDCT_STREAMS])
def test_vardct_against_the_reference(gpu, ref, name, opts):
    """box(the reference's pixels): within one level, the bar the full decode has (a mean of values within 1 is within 1)"""
    w, h = SIZES[0]
    data = synth("vardct", w, h, SEED, **opts)
    rerr, want = ref.decode(data)
    assert rerr == ""
    _, got = full_and_scaled(gpu, data)
    for k, (px, _) in got.items():
        d = np.abs(px.astype(np.int32) - box(want, k).astype(np.int32)).max()
        print("%s at 1:%d against the reference: max |delta| = %d" % (name, 1 << k, d))
        assert d <= 1


# ---------------------------------------------------------------- 3: nothing else is written

@pytest.mark.parametrize("fmt", [U8X4, U16X4], ids=["u8x4", "u16x4"])
@pytest.mark.parametrize("k", [1, 2])
@pytest.mark.parametrize("mode,w,h", [("vardct", 779, 517), ("vardct", 9, 5), ("modular", 257, 255)])
def test_nothing_outside_the_small_image_is_written(gpu, mode, w, h, k, fmt):
    import torch
    pb = 4 if fmt == U8X4 else 8
    s = 1 << k
    ow, oh = -(-w // s), -(-h // s)
    fr = open_frame(gpu, synth(mode, w, h, SEED, **opts_for(w, h)), fmt)
    err, full = fr.decode_to_host()
    assert err == "" and fr.set_scale(k) == ""
    stride = pb * ow + 64
    buf = torch.full((oh + 8, stride), 0xA5, dtype=torch.uint8, device="cuda:0")
    stream = torch.cuda.current_stream().cuda_stream
    with pytest.raises(gpu.J40Error) as e:
        fr.decode(buf.data_ptr() + 4 * stride, pb * ow - 1, stream)
    assert e.value.code == "rnge"
    torch.cuda.synchronize()
    assert bool((buf == 0xA5).all()), "a refused decode wrote something"
    fr.decode(buf.data_ptr() + 4 * stride, stride, stream)
    torch.cuda.synchronize()
    assert fr.status() == ""
    host = buf.cpu().numpy()
    assert (host[:4] == 0xA5).all() and (host[4 + oh:] == 0xA5).all() and (host[4:4 + oh, pb * ow:] == 0xA5).all()
    px = np.ascontiguousarray(host[4:4 + oh, :pb * ow]).view(full.dtype).reshape(oh, ow, 4)
    assert np.array_equal(px, box(full, k))
    fr.close()


# ---------------------------------------------------------------- 4, 2: Modular

@pytest.mark.parametrize("fmt", [U8X4, U16X4], ids=["u8x4", "u16x4"])
@pytest.mark.parametrize("w,h", MODULAR_SIZES)
@pytest.mark.parametrize("name,opts", MODULAR_STREAMS, ids=[n for n, _ in MODULAR_STREAMS])
def test_modular_equals_box_of_full(gpu, name, opts, w, h, fmt):
    full, got = full_and_scaled(gpu, synth("modular", w, h, SEED, **opts), fmt)
    for k, (px, sc) in got.items():
        assert np.array_equal(px, box(full, k)), (name, w, h, k)
        assert (sc["shift"], sc["staged"], sc["staging_bytes"]) == (k, 0, 0)


@pytest.mark.parametrize("name,opts", MODULAR_STREAMS, ids=[n for n, _ in MODULAR_STREAMS])
def test_modular_against_the_reference(gpu, ref, name, opts):
    w, h = MODULAR_SIZES[0]
    data = synth("modular", w, h, SEED, **opts)
    rerr, want = ref.decode(data)
    if name == "squeeze":   # the reference has no Squeeze ("TODO"): that stream is held to box(full) above, and its full decode to tests/test_squeeze.py
        assert rerr == "TODO"
        return
    assert rerr == ""
    _, got = full_and_scaled(gpu, data)
    for k, (px, _) in got.items():
        assert np.array_equal(px, box(want, k)), (name, k)


# ---------------------------------------------------------------- 5: the staged combinations

@pytest.mark.parametrize("fmt", [U8X4, U16X4], ids=["u8x4", "u16x4"])
@pytest.mark.parametrize("what", ["restoration", "keep_alpha"])
def test_staged_combinations(gpu, what, fmt):
    w, h = SIZES[0]
    if what == "restoration":
        data, mode = synth("vardct", w, h, 3, fullheader=1, gab=1, epf=2), dict(restoration=1)
    else:
        data, mode = synth("vardct", w, h, SEED, alpha=1), dict(alpha=True)
    full, got = full_and_scaled(gpu, data, fmt, **mode)
    plain = full_and_scaled(gpu, data, fmt, shifts=())[0]
    assert not np.array_equal(full, plain), "the mode changes the pixels, or this proves nothing about it"
    for k, (px, sc) in got.items():
        assert np.array_equal(px, box(full, k)), (what, k)
        assert sc["staged"] == 1 and sc["staging_bytes"] >= w * h * (4 if fmt == U8X4 else 8)
    # a second decode of the same handle gives the same bytes
    fr = open_frame(gpu, data, fmt, **mode)
    assert fr.set_scale(1) == ""
    first, second = fr.decode_to_host(), fr.decode_to_host()
    assert first[0] == second[0] == "" and np.array_equal(first[1], second[1]) and np.array_equal(first[1], got[1][0])
    fr.close()


# ---------------------------------------------------------------- 6: batches

def test_batch(gpu):
    import torch
    stream = torch.cuda.current_stream().cuda_stream
    frames = [open_frame(gpu, synth("vardct", w, h, SEED, **opts_for(w, h))) for w, h in BATCH_SIZES]
    fulls = []
    for fr in frames:
        err, px = fr.decode_to_host()
        assert err == "" and varied(px)
        fulls.append(px)
    for k in (1, 2):
        for fr in frames:
            assert fr.set_scale(k) == ""
        batch = gpu.Batch(frames)
        outs = [torch.full((fr.scale()["height"], fr.scale()["width"] * 4 + 32), 0xA5, dtype=torch.uint8, device="cuda:0") for fr in frames]
        batch.decode([o.data_ptr() for o in outs], [o.shape[1] for o in outs], stream)
        torch.cuda.synchronize()
        for fr, o, full in zip(frames, outs, fulls):
            assert fr.status() == ""
            host = o.cpu().numpy()
            want = box(full, k)
            assert (host[:, want.shape[1] * 4:] == 0xA5).all()
            assert np.array_equal(np.ascontiguousarray(host[:, :want.shape[1] * 4]).reshape(want.shape), want), (k, full.shape)
        batch.close()
    # members at shifts 0 and 1 together: "Usc?", nothing is written
    assert frames[0].set_scale(0) == "" and all(fr.set_scale(1) == "" for fr in frames[1:])
    batch = gpu.Batch(frames)
    outs = [torch.full((fr.height, fr.width * 4), 0xA5, dtype=torch.uint8, device="cuda:0") for fr in frames]
    with pytest.raises(gpu.J40Error) as e:
        batch.decode([o.data_ptr() for o in outs], [o.shape[1] for o in outs], stream)
    assert e.value.code == "Usc?"
    torch.cuda.synchronize()
    assert all(bool((o == 0xA5).all()) for o in outs)
    batch.close()
    for fr in frames:
        fr.close()
    # a keep-alpha member at shift 1
    fr = open_frame(gpu, synth("vardct", 520, 264, SEED, alpha=1), alpha=True)
    assert fr.set_scale(1) == ""
    batch = gpu.Batch([fr])
    out = torch.full((132, 260 * 4), 0xA5, dtype=torch.uint8, device="cuda:0")
    with pytest.raises(gpu.J40Error) as e:
        batch.decode([out.data_ptr()], [260 * 4], stream)
    assert e.value.code == "Usc?"
    torch.cuda.synchronize()
    assert bool((out == 0xA5).all())
    batch.close()
    fr.close()


def test_group_range_and_scale_exclude_each_other(gpu):
    """(an uploaded frame: j40hip_frame_set_group_range needs the device state)"""
    for mode, w, h in (("vardct", 779, 517), ("modular", 601, 303)):
        fr = open_frame(gpu, synth(mode, w, h, SEED))
        fr.set_group_range(1, 2)
        assert fr.set_scale(1) == "Usc?" and fr.scale()["shift"] == 0
        fr.set_group_range(0, fr.info["num_groups"])
        assert fr.set_scale(1) == ""
        with pytest.raises(gpu.J40Error) as e:
            fr.set_group_range(1, 2)
        assert e.value.code == "Usc?"
        fr.set_group_range(0, fr.info["num_groups"])      # the whole range is no range
        err, px = fr.decode_to_host()
        assert err == "" and px.shape == (-(-h // 2), -(-w // 2), 4)
        fr.close()


# ---------------------------------------------------------------- 7: the "evof" retry

def test_evof_retry_at_a_scale(gpu):
    data = synth("vardct", 520, 264, STRESS_SEED, flat=1, density=1, decay=1)
    fr = open_frame(gpu, data)
    assert fr.set_scale(1) == ""
    stream = 0
    import torch
    out = torch.zeros((132, 260 * 4), dtype=torch.uint8, device="cuda:0")
    fr.decode(out.data_ptr(), 260 * 4, stream)
    torch.cuda.synchronize()
    assert fr.status() == "evof", "the stream overflows its event region, or the retry is not what this tests"
    err, small = fr.decode_to_host()
    assert err == ""
    assert fr.set_scale(0) == ""
    err, full = fr.decode_to_host()
    assert err == "" and varied(full)
    assert np.array_equal(small, box(full, 1))
    fr.close()


# ---------------------------------------------------------------- 8: damage

def test_status_of_damaged_streams(gpu):
    """one byte changed inside a pass-group section: the code at 1:4 is the full decode's (every section is still entropy-decoded)"""
    base = synth("vardct", 520, 264, SEED)
    fr = gpu.Frame(base)
    first = int(fr.lf_end())
    fr.close()
    rng = np.random.default_rng(2024)
    found = 0
    for at in rng.integers(first, len(base) - 1, 64).tolist():
        data = bytearray(base)
        data[at] ^= 0x5A
        try:
            fr = open_frame(gpu, bytes(data))
        except gpu.J40Error:
            continue
        err0, _ = fr.decode_to_host()
        st0 = fr.status()
        if st0 == "":
            fr.close()
            continue
        assert fr.set_scale(2) == ""
        err2, _ = fr.decode_to_host()
        assert (err2, fr.status()) == (err0, st0), at
        fr.close()
        found += 1
        if found == 5:
            break
    assert found == 5, "fewer than five damaged streams report a code"


# ---------------------------------------------------------------- 9: the pipeline

def test_pipeline(gpu):
    import torch
    sizes = BATCH_SIZES + [(776, 520)] * 3
    streams = [synth("vardct", w, h, SEED + (i if i >= 5 else 0), **opts_for(w, h)) for i, (w, h) in enumerate(sizes)]
    wants = []
    for data in streams:
        full = full_and_scaled(gpu, data, shifts=())[0]
        wants.append((full, box(full, 1)))
    pipe = gpu.Pipeline(device=0, host_threads=2, batch_frames=4, max_in_flight=2)
    assert pipe.set_scale(3) == "rnge" and pipe.set_scale(1) == ""
    # to host memory
    outs = [np.full(w.shape, 0xA5, np.uint8) for _, w in wants]
    tickets = [pipe.submit(d, o.ctypes.data, o.shape[1] * 4) for d, o in zip(streams, outs)]
    assert pipe.set_scale(2) == "Usc?", "jobs are in flight"
    pipe.drain()
    assert [pipe.result(t) for t in tickets] == [""] * len(tickets)
    for o, (_, want) in zip(outs, wants):
        assert np.array_equal(o, want)
    # device output
    douts = [torch.full(w.shape, 0xA5, dtype=torch.uint8, device="cuda:0") for _, w in wants]
    tickets = [pipe.submit(d, o.data_ptr(), o.shape[1] * 4, device_output=True) for d, o in zip(streams, douts)]
    pipe.drain()
    torch.cuda.synchronize()
    assert [pipe.result(t) for t in tickets] == [""] * len(tickets)
    for o, (_, want) in zip(douts, wants):
        assert np.array_equal(o.cpu().numpy(), want)
    # run() hands the small sizes to the allocator
    for i in (0, 4, 5):
        err, px = pipe.run(streams[i])
        assert err == "" and np.array_equal(px, wants[i][1])
    # a stride one byte short of the small image's rows
    bad = np.full(wants[0][1].shape, 0xA5, np.uint8)
    t = pipe.submit(streams[0], bad.ctypes.data, bad.shape[1] * 4 - 1)
    pipe.drain()
    assert pipe.result(t) == "rnge" and (bad == 0xA5).all()
    assert pipe.set_scale(2) == ""
    err, px = pipe.run(streams[1])
    assert err == "" and np.array_equal(px, box(wants[1][0], 2))
    # a second pipeline at shift 0 in the same process still gives full images
    other = gpu.Pipeline(device=0, host_threads=2, batch_frames=4, max_in_flight=2)
    for i in (0, 4, 6):
        err, px = other.run(streams[i])
        assert err == "" and np.array_equal(px, wants[i][0])
    other.close()
    pipe.close()


@pytest.mark.parametrize("name,opts", [("large", VARDCT_STREAMS[5][1]), ("cfl", VARDCT_STREAMS[1][1]), ("dq", VARDCT_STREAMS[4][1])])
def test_pipeline_batch_wide_kernels_every_family(gpu, name, opts):
    """the batch-wide instantiations (what a pipeline launches) of all three kernel families at both shifts: streams with the
    128 / 256-sized transforms and the 8x8 specials, four frames to a launch, against box() of the single-frame full decode"""
    import torch
    streams = [synth("vardct", w, h, SEED, **opts) for w, h in SIZES] * 2
    fulls = [full_and_scaled(gpu, d, shifts=())[0] for d in streams[:2]] * 2
    pipe = gpu.Pipeline(device=0, host_threads=2, batch_frames=4, max_in_flight=2)
    for k in (1, 2):
        pipe.drain()
        assert pipe.set_scale(k) == ""
        wants = [box(f, k) for f in fulls]
        outs = [torch.full(w.shape, 0xA5, dtype=torch.uint8, device="cuda:0") for w in wants]
        tickets = [pipe.submit(d, o.data_ptr(), o.shape[1] * 4, device_output=True) for d, o in zip(streams, outs)]
        assert pipe.set_scale(k) == "", "the shift in force, also with images in flight"
        pipe.drain()
        torch.cuda.synchronize()
        assert [pipe.result(t) for t in tickets] == [""] * 4
        for o, want in zip(outs, wants):
            assert np.array_equal(o.cpu().numpy(), want), (name, k)
    st = pipe.stats()
    assert st["launches"] >= 2 and st["single_frames"] == 0, st    # the frames went through batches, not the single-frame path
    pipe.close()


# ---------------------------------------------------------------- 10: the public API

CHILD = r"""
import os, sys
import numpy as np
sys.path.insert(0, sys.argv[1])
import j40_amd
data = open(sys.argv[2], "rb").read()
out = {}
def one(tag):
    err, px = j40_amd.decode(data)
    out[tag + "_err"] = np.frombuffer(err.encode().ljust(4), np.uint8)
    if px is not None:
        out[tag] = px.copy()
one("scale2")
if os.environ.get("J40HIP_SERVE") != "1":
    os.environ["J40HIP_FRAMES"] = "1"; one("scale2_frames")
    del os.environ["J40HIP_FRAMES"]
    os.environ["J40HIP_SCALE"] = "0"; one("scale0")
    del os.environ["J40HIP_SCALE"]; one("unset")
np.savez(sys.argv[3], **out)
j40_amd.shutdown()
"""


@pytest.mark.parametrize("serve", [0, 1], ids=["latency_path", "served"])
def test_public_api_in_a_fresh_process(gpu, tmp_path, serve):
    w, h = SIZES[0]
    data = synth("vardct", w, h, SEED)
    full = full_and_scaled(gpu, data, shifts=())[0]
    path, res = str(tmp_path / "in.jxl"), str(tmp_path / "out.npz")
    with open(path, "wb") as fp:
        fp.write(data)
    env = dict(os.environ, J40HIP_SCALE="2")
    env.pop("J40HIP_FRAMES", None)
    if serve:
        env["J40HIP_SERVE"] = "1"
    r = subprocess.run([sys.executable, "-c", CHILD, ROOT, path, res], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    got = np.load(res)
    code = lambda tag: bytes(got[tag + "_err"]).decode().strip()
    assert code("scale2") == "" and got["scale2"].shape == (-(-h // 4), -(-w // 4), 4)
    assert np.array_equal(got["scale2"], box(full, 2))
    if not serve:
        assert code("scale2_frames") == "Usc?" and "scale2_frames" not in got
        assert code("scale0") == code("unset") == ""
        assert np.array_equal(got["scale0"], got["unset"]) and np.array_equal(got["unset"], full)


# ---------------------------------------------------------------- 11: k_downscale alone

@pytest.mark.parametrize("fmt", [U8X4, U16X4], ids=["u8x4", "u16x4"])
@pytest.mark.parametrize("k", [1, 2])
@pytest.mark.parametrize("w,h", [(61, 43), (256, 64)])
def test_downscale_kernel_alone(gpu, w, h, k, fmt):
    import torch
    L = gpu.lib()
    dtype = np.uint8 if fmt == U8X4 else np.uint16
    pb = 4 * np.dtype(dtype).itemsize
    rng = np.random.default_rng(w + k)
    full = rng.integers(0, np.iinfo(dtype).max + 1, (h, w, 4)).astype(dtype)
    want = box(full, k)
    oh, ow = want.shape[:2]
    src = torch.from_numpy(full.view(np.uint8).reshape(h, w * pb)).to("cuda:0")
    stride = ow * pb + 16
    out = torch.full((oh, stride), 0xA5, dtype=torch.uint8, device="cuda:0")
    stream = torch.cuda.current_stream().cuda_stream
    call = lambda *a: gpu.err4(L.j40hip_kat_device_downscale(*a))
    assert call(out.data_ptr(), stride, src.data_ptr(), w * pb, w, h, k, 0x1234, stream) == "Ufm?"
    assert call(out.data_ptr(), stride, src.data_ptr(), w * pb, w, h, 3, fmt, stream) == "rnge"
    assert call(out.data_ptr(), stride, src.data_ptr(), w * pb, w, h, 0, fmt, stream) == "rnge"
    assert call(out.data_ptr(), ow * pb - pb, src.data_ptr(), w * pb, w, h, k, fmt, stream) == "rnge"
    assert call(out.data_ptr(), stride, src.data_ptr(), w * pb - pb, w, h, k, fmt, stream) == "rnge"
    torch.cuda.synchronize()
    assert bool((out == 0xA5).all())
    assert call(out.data_ptr(), stride, src.data_ptr(), w * pb, w, h, k, fmt, stream) == ""
    torch.cuda.synchronize()
    host = out.cpu().numpy()
    assert (host[:, ow * pb:] == 0xA5).all()
    assert np.array_equal(np.ascontiguousarray(host[:, :ow * pb]).view(dtype).reshape(oh, ow, 4), want)
