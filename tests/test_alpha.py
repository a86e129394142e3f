"""The kept alpha channel of VarDCT frames (j40hip_frame_set_alpha, J40HIP_ALPHA; include/j40hip.h).

A lossy image with transparency carries its alpha as an extra channel: a Modular sub-image behind the HF coefficients of every
pass-group section. The reference decodes these and drops them when it combines the frame (j40.h:7868), so its pixels -- and this
library's by default -- have A = 255. Its STAGED decode (oracle/ref_harness.c) stops before that: until RefStage.combine() is
called, RefStage.plane_i16(c) is extra channel c as the reference decoded it, sample for sample. Keep mode is pinned to that plane
through the rule the reference renders a Modular frame's alpha with (j40.h:7950-7951):

    p clamped to [0, maxpixel = 2^bpp - 1];  u8: (p * 255 + 2^(bpp - 1)) / maxpixel;  u16: (p * 65535 + 2^(bpp - 1)) / maxpixel

A is exact everywhere; R, G, B are those of drop mode, which the other test files hold against the reference."""
import ctypes as C
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

from streams import synth, ROOT

U8X4, U16X4 = 0x0F33, 0x0F35

# (name, width, height, generator options, index of the alpha extra channel, bit depth)
STREAMS = [
    ("plain_600x300", 600, 300, dict(alpha=1), 0, 8),
    ("hfprefix_257x200", 257, 200, dict(alpha=1, hfprefix=1), 0, 8),                      # a width not divisible by 4
    ("dq2_1000x700", 1000, 700, dict(alpha=1, dq=2), 0, 8),
    ("two_depth_channels_ahead", 600, 300, dict(alpha=1, extra=2), 2, 8),
    ("bpp12_601x300", 601, 300, dict(alpha=1, bpp=12), 0, 12),
    ("forward_522x264", 522, 264, dict(alpha=1, forward=1), 0, 8),
    ("wp_in_both_headers", 600, 300, dict(alpha=1, lftree=4, wp="random", wpat="both", dq=2), 0, 8),
    ("global_code_lz77_prefix", 600, 300, dict(alpha=1, extra=1, glz77=1, gprefix=1), 1, 8),   # LZ77 and prefix codes in the global code
]
SEED = 7
IDS = [s[0] for s in STREAMS]


def stream(case):
    _, w, h, opts, _, _ = case
    return synth("vardct", w, h, SEED, **opts)


def render(p, bpp, fmt):
    """the rule, on the reference's plane"""
    maxpixel = (1 << bpp) - 1
    p = np.clip(np.asarray(p, np.int64), 0, maxpixel)
    return ((p * (65535 if fmt == U16X4 else 255) + (1 << (bpp - 1))) // maxpixel).astype(np.uint16 if fmt == U16X4 else np.uint8)


def oracle(ref, data, index):
    """(the reference's alpha plane before it is dropped, the reference's u8 pixels, bpp)"""
    from refdec import RefStage
    st = RefStage(ref, data)
    try:
        assert st.info["is_modular"] == 0
        n_before = ref.lib.ref_stage_num_planes(st.h)
        plane = st.plane_i16(index)
        bpp = st.info["bpp"]
        assert n_before == st.info["num_extra_channels"] and plane.shape == (st.info["height"], st.info["width"])
    finally:
        st.close()
    err, px = ref.decode(data)
    assert err == "" and (px[..., 3] == 255).all()   # what the reference itself shows: opaque
    return plane, px, bpp


@pytest.fixture(scope="module")
def sim(built):
    L = C.CDLL(os.path.join(ROOT, "build", "libhostsim_alpha.so"))
    L.alpha_sim_scale.restype = C.c_uint32
    L.alpha_sim_scale.argtypes = [C.c_int32, C.c_int32, C.c_int32]
    L.alpha_sim_decode.restype = C.c_uint32
    L.alpha_sim_decode.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_int32]
    return L


def code4(c):
    return "".join(chr((c >> s) & 0xff) for s in (24, 16, 8, 0)) if c else ""


# ---------------------------------------------------------------- without a GPU

def test_scale_is_the_integer_formula_everywhere(sim):
    """device/alpha_dev.h's alpha_value (multiply-high by a per-depth reciprocal and one correction) against the plain division:
    every p in [-2, maxpixel + 2], every bpp 8..15, both formats"""
    for bpp in range(8, 16):
        maxpixel = (1 << bpp) - 1
        for fmt, mult in ((U8X4, 255), (U16X4, 65535)):
            for p in range(-2, maxpixel + 3):
                c = min(max(p, 0), maxpixel)
                assert sim.alpha_sim_scale(p, bpp, fmt) == (c * mult + (1 << (bpp - 1))) // maxpixel, (p, bpp, hex(fmt))
    for p in range(0, 256):   # 8 bits to 8 bits is the identity
        assert sim.alpha_sim_scale(p, 8, U8X4) == p


def aligned_view(nbytes, offset):
    """a byte buffer whose first byte is `offset` past a 16-byte boundary"""
    raw = np.zeros(nbytes + 64, np.uint8)
    start = (-raw.ctypes.data) % 16 + offset
    return raw[start:start + nbytes]


@pytest.mark.parametrize("case", STREAMS, ids=IDS)
def test_cpu_merge_equals_the_reference_plane(sim, ref, case):
    """alpha_sim_decode (tests/hostsim/alpha_sim.cpp): entropy decode, keep-mode trailer plan into frame-wide planes, the merge
    functions k_alpha_merge runs. A exact in u8 and u16, R, G, B as handed in; tight rows on a 16-byte boundary and rows with a
    larger stride starting one pixel past one (so that every row has a head and a tail to take the narrow path)"""
    _, w, h, _, index, bpp_expected = case
    data = stream(case)
    plane, px, bpp = oracle(ref, data, index)
    assert bpp == bpp_expected and plane.min() >= 0 and plane.max() > (1 << bpp) * 3 // 4   # (a channel that is not constant)
    rng = np.random.default_rng(11)
    for fmt, pb, dt in ((U8X4, 4, np.uint8), (U16X4, 8, np.uint16)):
        given = px.copy() if fmt == U8X4 else rng.integers(0, 65536, (h, w, 4), dtype=np.uint16)
        given[..., 3] = 255 if fmt == U8X4 else 65535
        for offset, slack in ((0, 0), (pb, 24 - pb)):
            stride = w * pb + slack
            buf = aligned_view(h * stride, offset)
            buf[:] = 0x5a
            rows = np.lib.stride_tricks.as_strided(buf, (h, w * pb), (stride, 1))
            rows[:] = given.view(np.uint8).reshape(h, w * pb)
            err = sim.alpha_sim_decode(data, len(data), buf.ctypes.data, stride, fmt)
            assert err == 0, code4(err)
            got = np.ascontiguousarray(rows).view(dt).reshape(h, w, 4)
            assert np.array_equal(got[..., 3], render(plane, bpp, fmt)), (hex(fmt), offset)
            assert np.array_equal(got[..., :3], given[..., :3]), (hex(fmt), offset)
            if slack:
                pad = np.lib.stride_tricks.as_strided(buf[w * pb:], (h - 1, slack), (stride, 1))
                assert (pad == 0x5a).all(), "the merge wrote between the rows"


def test_set_alpha_header_logic(built):
    """j40hip_frame_set_alpha / j40hip_frame_alpha on parsed frames, no device involved"""
    import j40_amd
    # nothing to keep: no alpha channel; a Modular frame (its alpha is always rendered)
    for data in (synth("vardct", 264, 200, 11), synth("modular", 300, 200, 4, alpha=1)):
        fr = j40_amd.Frame(data)
        for mode in (1, 0, -1):
            assert fr.set_alpha(mode) == "Ual?"
        assert fr.alpha()["mode"] == 0 and fr.alpha()["written"] == 0
        fr.close()
    fr = j40_amd.Frame(synth("vardct", 264, 200, 11))
    assert fr.alpha()["index"] == -1
    fr.close()
    # outside what keep mode serves: "TODO", the frame left as it was; dropping is always possible
    for opts, bpp in ((dict(alpha=1, alphaassoc=1), 8), (dict(alpha=1, alphabpp=10), 10)):
        fr = j40_amd.Frame(synth("vardct", 300, 260, SEED, **opts))
        assert fr.set_alpha(1) == "TODO"
        assert fr.alpha() == {"index": 0, "bpp": bpp, "mode": 0, "written": 0}
        assert fr.set_alpha(0) == "" and fr.set_alpha(-1) == ""
        fr.close()
    # (passes=2 alpha=1: tools/jxlsynth.cpp refuses to write it -- carrying the sub-image in both passes' sections as they stand
    # gives a stream the reference answers with "shrt" -- so the several-passes refusal, `num_passes != 1` in plan_build.cpp's
    # alpha_keep_scope, has no stream here)
    with pytest.raises(subprocess.CalledProcessError):
        synth("vardct", 300, 260, SEED, alpha=1, passes=2)
    # in scope
    for opts, index in ((dict(alpha=1), 0), (dict(alpha=1, extra=2), 2), (dict(alpha=1, bpp=12), 0)):
        fr = j40_amd.Frame(synth("vardct", 600, 300, SEED, **opts))
        assert fr.alpha()["index"] == index and fr.alpha()["bpp"] == opts.get("bpp", 8)
        assert fr.set_alpha(1) == "" and fr.alpha()["mode"] == 1
        assert fr.set_alpha(0) == "" and fr.alpha()["mode"] == 0
        assert fr.set_alpha(-1) == "" and fr.alpha()["mode"] == (1 if os.environ.get("J40HIP_ALPHA", "0") not in ("", "0") else 0)
        fr.close()


def test_cpu_merge_refuses_what_set_alpha_refuses(sim):
    for opts, want in ((dict(alpha=1, alphaassoc=1), "TODO"), (dict(alpha=1, alphabpp=10), "TODO"), (dict(), "Ual?")):
        data = synth("vardct", 300, 260, SEED, **opts)
        buf = np.full((260, 300, 4), 255, np.uint8)
        assert code4(sim.alpha_sim_decode(data, len(data), buf.ctypes.data, 1200, U8X4)) == want
        assert (buf == 255).all()


# the bytes the generator wrote for these before it learnt extra= / bpp= / alphaassoc= / alphabpp= / glz77= / gprefix= in VarDCT mode
PARENT_STREAMS = [
    ("vardct", 600, 300, 7, {"alpha": 1}, "d8f1a7bdba1647fa18094f54a830f723385c346930d7c9020cc33ff5d41a3ec7"),
    ("vardct", 257, 200, 7, {"alpha": 1, "hfprefix": 1}, "a825e31ac35d5bbe579eb3c4bff9d0a6af48b6db3799e26b2c76c2937158fe85"),
    ("vardct", 1000, 700, 7, {"alpha": 1, "dq": 2}, "eaaf80bb2a8af700c7cd168164e3b158dd2e8e660ff240dcb8a02de04ba4ab40"),
    ("vardct", 520, 264, 1, {}, "1308dbdf0ecb08241c4c8830a788bb21a01bb97a83f13886fa3a12d9971e7e39"),
    ("vardct", 520, 264, 33, {"alpha": 1}, "3e1767c8ba37cc008b3e06fdbc91ebf5578787014ce9353cc9ded095cb977eee"),
    ("vardct", 300, 200, 2, {"bpp": 12}, "32944aa017c07e5c5e6c13472c8eb85639d3255146852308c4239e40b2b0a46f"),
    ("vardct", 600, 300, 7, {"alpha": 1, "lftree": 4, "wp": "random", "wpat": "both", "dq": 2}, "297f0206206a815981b1984a5e3d05ecf5c20843a50bd460a4bd10d2d23b027f"),
    ("vardct", 300, 300, 9, {"alpha": 1, "noxyb": 1, "fullheader": 1}, "5535cac7fc07217a9a8c38ce2b2a9dc07bb1ef47b9fef122c7274ada36a148a9"),
    ("modular", 600, 300, 4, {"extra": 3, "alpha": 1, "tree": 3, "localrct": 7}, "06d1702c200402f4bb3b18e79160d9ebb2ba51e74dd624ed55c5a886c14419f3"),
    ("vardct", 400, 300, 5, {"passes": 2}, "bf6c0887ae8fbaaeccb2027ddab6c6acb2a1ffed932e64246930fdb684a8aaf4"),
]


def test_streams_without_the_new_options_are_unchanged(built, tmp_path):
    for mode, w, h, seed, opts, digest in PARENT_STREAMS:
        out = str(tmp_path / "s.jxl")   # (not through the stream cache: what the generator writes now)
        subprocess.run([os.path.join(ROOT, "build", "jxlsynth"), mode, str(w), str(h), str(seed), out] + ["%s=%s" % kv for kv in sorted(opts.items())],
                       check=True, stderr=subprocess.DEVNULL)
        with open(out, "rb") as fp:
            assert hashlib.sha256(fp.read()).hexdigest() == digest, (mode, w, h, seed, opts)


# ---------------------------------------------------------------- on the GPU

@pytest.fixture(scope="module")
def gpu(built):
    import j40_amd
    assert j40_amd.device_count() > 0, "the gpu tests need a HIP device"
    assert os.environ.get("J40HIP_ALPHA", "") in ("", "0"), "these tests set the mode themselves (and J40HIP_ALPHA in child processes)"
    return j40_amd


def child(code, env_extra, timeout=900):
    env = dict(os.environ, **env_extra)
    prog = "import sys, os\nsys.path.insert(0, %r); sys.path.insert(0, os.path.join(%r, 'tests'))\n" % (ROOT, ROOT) + code
    r = subprocess.run([sys.executable, "-c", prog], env=env, timeout=timeout, capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    return r.stdout


def decode_host(gpu, data, fmt, alpha, restoration=None):
    fr = gpu.Frame(data)
    fr.set_output_format(fmt)
    if alpha is not None:
        assert fr.set_alpha(alpha) == ""
    if restoration is not None:
        fr.set_restoration(restoration)
    fr.upload(0)
    err, px = fr.decode_to_host()
    return fr, err, px


@pytest.mark.gpu
@pytest.mark.parametrize("case", STREAMS, ids=IDS)
def test_gpu_keep_mode_is_exact(gpu, ref, case):
    """Frame.decode_to_host and j40hip_frame_decode into a torch tensor, both formats: A is the reference's plane by the rule, R, G, B
    are drop mode's; a second decode of the same handle (which reuses the plan and the planes kept with the frame) gives the same bytes"""
    import torch
    _, w, h, _, index, _ = case
    data = stream(case)
    plane, _, bpp = oracle(ref, data, index)
    for fmt, pb, dt in ((U8X4, 4, np.uint8), (U16X4, 8, np.uint16)):
        want_a = render(plane, bpp, fmt)
        fd, err, drop = decode_host(gpu, data, fmt, 0)
        assert err == "" and (drop[..., 3] == (255 if fmt == U8X4 else 65535)).all() and fd.alpha()["written"] == 0
        fd.close()
        fr, err, keep = decode_host(gpu, data, fmt, 1)
        assert err == "" and fr.alpha() == {"index": index, "bpp": bpp, "mode": 1, "written": 1}
        assert np.array_equal(keep[..., 3], want_a), hex(fmt)
        assert np.array_equal(keep[..., :3], drop[..., :3]), hex(fmt)
        err, again = fr.decode_to_host()
        assert err == "" and np.array_equal(again, keep)
        # on the device: rows longer than the picture, the first of them one pixel past a 16-byte boundary
        stride = w * pb + 24 - pb
        flat = torch.full((h * stride + 64,), 0x5a, dtype=torch.uint8, device="cuda:0")
        base = (-flat.data_ptr()) % 16 + pb
        for _ in range(2):
            fr.decode(flat.data_ptr() + base, stride, torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            assert fr.status() == ""
            host = flat.cpu().numpy()[base:base + h * stride]
            rows = np.lib.stride_tricks.as_strided(host, (h, w * pb), (stride, 1))
            assert np.array_equal(np.ascontiguousarray(rows).view(dt).reshape(h, w, 4), keep), hex(fmt)
            pad = np.lib.stride_tricks.as_strided(host[w * pb:], (h - 1, 24 - pb), (stride, 1))
            assert (pad == 0x5a).all()
        fr.close()
        err, api = gpu.decode(data, fmt, alpha=True)
        assert err == "" and np.array_equal(api, keep)


@pytest.mark.gpu
def test_gpu_public_api_follows_the_environment(gpu, ref):
    """the public ten functions under J40HIP_ALPHA=1, in a process of its own (the variable is read once): A exact in both formats;
    a frame keep mode does not serve decodes opaque as before, and j40hip_frame_alpha says so"""
    out = os.path.join(ROOT, "build", "alpha_env_%d_%d.npy")
    child("""
import numpy as np, j40_amd
from streams import synth
for i, (name, w, h, opts, index, bpp) in enumerate(CASES):
    data = synth("vardct", w, h, SEED, **opts)
    for k, fmt in enumerate((j40_amd.J40_U8X4, j40_amd.J40_U16X4)):
        err, px = j40_amd.decode(data, fmt)
        assert err == "", err
        np.save(OUT % (i, k), px)
data = synth("vardct", 300, 260, SEED, alpha=1, alphaassoc=1)
err, px = j40_amd.decode(data)
assert err == "" and (px[..., 3] == 255).all()
fr = j40_amd.Frame(data); fr.upload(0)
assert fr.alpha()["mode"] == 0
err, px2 = fr.decode_to_host()
assert err == "" and np.array_equal(px, px2) and fr.alpha()["written"] == 0
fr.close()
fr = j40_amd.Frame(synth("vardct", 600, 300, SEED, alpha=1))
assert fr.alpha()["mode"] == 1 and fr.set_alpha(0) == "" and fr.alpha()["mode"] == 0
fr.close()
j40_amd.shutdown()
""".replace("CASES", repr(STREAMS)).replace("SEED", repr(SEED)).replace("OUT", repr(out)), {"J40HIP_ALPHA": "1"})
    for i, case in enumerate(STREAMS):
        _, w, h, _, index, _ = case
        data = stream(case)
        plane, _, bpp = oracle(ref, data, index)
        for k, fmt in enumerate((U8X4, U16X4)):
            px = np.load(out % (i, k))
            err, drop = gpu.decode(data, fmt)   # (this process: the variable unset)
            assert err == "" and (drop[..., 3] == (255 if fmt == U8X4 else 65535)).all()
            assert np.array_equal(px[..., 3], render(plane, bpp, fmt)), (case[0], hex(fmt))
            assert np.array_equal(px[..., :3], drop[..., :3]), (case[0], hex(fmt))


@pytest.mark.gpu
def test_gpu_drop_mode_and_unset_environment_are_todays_bytes(gpu, ref):
    for case in STREAMS[:2] + STREAMS[3:5]:
        data = stream(case)
        for fmt in (U8X4, U16X4):
            opaque = 255 if fmt == U8X4 else 65535
            f0, err, never = decode_host(gpu, data, fmt, None)   # set_alpha never called
            assert err == "" and (never[..., 3] == opaque).all() and f0.alpha()["mode"] == 0 and f0.alpha()["written"] == 0
            assert f0.set_alpha(0) == ""
            err, dropped = f0.decode_to_host()
            assert err == "" and np.array_equal(dropped, never)
            # keep, then back to the default on the same handle
            assert f0.set_alpha(1) == ""
            err, kept = f0.decode_to_host()
            assert err == "" and not (kept[..., 3] == opaque).all()
            assert f0.set_alpha(-1) == ""
            err, back = f0.decode_to_host()
            assert err == "" and np.array_equal(back, never) and f0.alpha()["written"] == 0
            f0.close()
            err, api = gpu.decode(data, fmt)
            assert err == "" and np.array_equal(api, never)
        if case[5] == 8:
            _, px, _ = oracle(ref, data, case[4])
            err, api = gpu.decode(data)
            assert np.abs(api.astype(np.int32) - px.astype(np.int32)).max() <= 1 and (api[..., 3] == 255).all()


@pytest.mark.gpu
def test_gpu_range_decodes_merge_their_own_groups(gpu):
    """two halves of the groups into one buffer = the whole decode, keep mode; a half touches only its groups' pixels"""
    import torch
    from j40_amd import sharding
    for w, h, opts, fmt, pb in ((1000, 700, dict(alpha=1, dq=2), U8X4, 4), (601, 300, dict(alpha=1, bpp=12), U16X4, 8), (600, 600, dict(alpha=1, extra=2), U8X4, 4)):
        data = synth("vardct", w, h, SEED, **opts)
        fr, err, whole = decode_host(gpu, data, fmt, 1)
        assert err == ""
        n = fr.info["num_groups"]
        out = torch.full((h, w * pb), 9, dtype=torch.uint8, device="cuda:0")
        for first, count in ((0, n // 2), (n // 2, n - n // 2)):
            fr.set_group_range(first, count)
            before = out.clone()
            fr.decode(out.data_ptr(), w * pb, torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            assert fr.status() == "" and fr.alpha()["written"] == 1
            mine = torch.zeros((h, w), dtype=torch.bool, device="cuda:0")
            for x0, y0, x1, y1 in sharding.range_rectangles(first, count, w, h, fr.info["group_size_shift"]):
                mine[y0:y1, x0:x1] = True
            assert torch.equal(out.view(h, w, pb)[~mine], before.view(h, w, pb)[~mine]), "a range wrote outside its own groups"
        got = out.cpu().numpy().view(np.uint16 if fmt == U16X4 else np.uint8).reshape(h, w, 4)
        assert np.array_equal(got, whole)
        # and whole again on the same handle
        fr.set_group_range(0, n)
        err, again = fr.decode_to_host()
        assert err == "" and np.array_equal(again, whole)
        fr.close()


@pytest.mark.gpu
def test_gpu_batch_merges_at_status(gpu, ref):
    """four keep-mode frames and one drop-mode frame in one batch: A is 255 until the status is read, then the reference's plane for
    the keep members and still 255 for the drop member; the codes are the single-frame path's"""
    import torch
    cases = [STREAMS[0], STREAMS[1], STREAMS[3], STREAMS[6], STREAMS[2]]
    modes = [1, 1, 1, 1, 0]
    frames, outs, alone = [], [], []
    for case, mode in zip(cases, modes):
        data = stream(case)
        f1, err, px = decode_host(gpu, data, U8X4, mode)
        assert err == ""
        alone.append(px)
        f1.close()
        fr = gpu.Frame(data)
        assert fr.set_alpha(mode) == ""
        fr.upload(0)
        frames.append(fr)
        outs.append(torch.zeros((fr.height, fr.width, 4), dtype=torch.uint8, device="cuda:0"))
    b = gpu.Batch(frames)
    for _ in range(2):
        b.decode([o.data_ptr() for o in outs], [f.width * 4 for f in frames], torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        for fr, o in zip(frames, outs):
            assert (o[..., 3] == 255).all() and fr.alpha()["written"] == 0
        for case, mode, fr, o, px in zip(cases, modes, frames, outs, alone):
            assert fr.status() == ""
            got = o.cpu().numpy()
            assert np.array_equal(got, px), case[0]
            assert fr.alpha()["written"] == mode
            if mode:
                plane, _, bpp = oracle(ref, stream(case), case[4])
                assert np.array_equal(got[..., 3], render(plane, bpp, U8X4))
            else:
                assert (got[..., 3] == 255).all()
    b.close()
    for fr in frames:
        fr.close()


@pytest.mark.gpu
def test_gpu_alpha_composes_with_restoration(gpu, ref):
    data = synth("vardct", 600, 300, SEED, alpha=1, fullheader=1, gab=1, epf=2)
    plane, _, bpp = oracle(ref, data, 0)
    for fmt in (U8X4, U16X4):
        f0, err, filtered = decode_host(gpu, data, fmt, 0, restoration=1)
        assert err == ""
        f0.close()
        f1, err, plain = decode_host(gpu, data, fmt, 0, restoration=0)
        assert err == "" and not np.array_equal(plain, filtered)   # (the filters did run)
        f1.close()
        fr, err, both = decode_host(gpu, data, fmt, 1, restoration=1)
        assert err == "" and fr.alpha()["written"] == 1
        assert np.array_equal(both[..., 3], render(plane, bpp, fmt))
        assert np.array_equal(both[..., :3], filtered[..., :3])
        fr.close()


@pytest.mark.gpu
def test_gpu_damage_in_the_sub_images_keeps_the_reference_codes(gpu, ref):
    """the 40 single-bit flips of test_gpu_parity.py's test_damage_in_extra_channel_sub_images_is_reported (same stream, seed and
    range) in keep mode: the reference's code for every one; where it accepts, A is its plane of the DAMAGED stream and R, G, B are
    within one level. At least 10 of the 40 must be rejections, or the test says nothing about them."""
    from refdec import RefStage
    data = synth("vardct", 520, 264, 33, alpha=1)
    rng = np.random.default_rng(5)
    seen = {}
    for _ in range(40):
        mutated = bytearray(data)
        pos = int(rng.integers(len(data) // 3, len(data)))
        mutated[pos] ^= 1 << int(rng.integers(0, 8))
        mutated = bytes(mutated)
        rerr, rexp = ref.decode(mutated)
        err, rgba = gpu.decode(mutated, alpha=True)
        print("flip at %d: reference %r, keep mode %r" % (pos, rerr, err))
        assert err == rerr, (pos, rerr, err)
        if rerr == "":
            st = RefStage(ref, mutated)
            plane = st.plane_i16(0)
            st.close()
            assert np.array_equal(rgba[..., 3], render(plane, 8, U8X4)), pos
            assert np.abs(rgba[..., :3].astype(np.int32) - rexp[..., :3].astype(np.int32)).max() <= 1, pos
        seen[rerr] = seen.get(rerr, 0) + 1
    print(seen)
    assert 40 - seen.get("", 0) >= 10, seen


@pytest.mark.gpu
def test_gpu_8k_frame_through_the_public_api(gpu, ref):
    """7680 x 4320, alpha=1 forward=1, the public API with J40HIP_ALPHA=1: every row is 16-byte aligned and a multiple of four
    pixels wide, so the merge takes its wide path throughout"""
    out = os.path.join(ROOT, "build", "alpha_8k.npy")
    child("""
import numpy as np, j40_amd
from streams import synth
err, px = j40_amd.decode(synth("vardct", 7680, 4320, SEED, alpha=1, forward=1))
assert err == "", err
np.save(OUT, px[..., 3])
j40_amd.shutdown()
""".replace("SEED", repr(SEED)).replace("OUT", repr(out)), {"J40HIP_ALPHA": "1"})
    data = synth("vardct", 7680, 4320, SEED, alpha=1, forward=1)
    from refdec import RefStage
    st = RefStage(ref, data)
    plane = st.plane_i16(0)
    st.close()
    assert np.array_equal(np.load(out), render(plane, 8, U8X4))
    os.remove(out)


@pytest.mark.gpu
def test_gpu_merge_kernel_alone(gpu):
    """k_alpha_merge through j40hip_kat_device_alpha_merge on planes no stream would give: samples below 0 and above maxpixel (the
    clamp), depths 8, 10 and 15, a rectangle that starts and ends off every alignment; pixels outside it and R, G, B stay"""
    import torch
    L = gpu.lib()
    rng = np.random.default_rng(3)
    W, H = 203, 37
    for bpp in (8, 10, 15):
        maxpixel = (1 << bpp) - 1
        plane = rng.integers(-40, maxpixel + 41, (H, W)).clip(-32768, 32767).astype(np.int16)
        plane[0, :8] = [-32768, -1, 0, 1, maxpixel - 1, maxpixel, min(maxpixel + 1, 32767), 32767]
        d_plane = torch.from_numpy(plane).to("cuda:0")
        for fmt, pb, dt in ((U8X4, 4, np.uint8), (U16X4, 8, np.uint16)):
            for x0, y0, w, h in ((0, 0, W, H), (3, 2, W - 5, H - 3), (1, 0, 2, H), (W - 1, 5, 1, 7)):
                stride = W * pb + 24 - pb
                given = rng.integers(0, 256, (H, stride), dtype=np.uint8)
                flat = torch.zeros(H * stride + 64, dtype=torch.uint8, device="cuda:0")
                base = (-flat.data_ptr()) % 16 + pb
                flat[base:base + H * stride] = torch.from_numpy(given.reshape(-1)).to("cuda:0")
                code = L.j40hip_kat_device_alpha_merge(flat.data_ptr() + base, stride, d_plane.data_ptr(), W, x0, y0, w, h, bpp, fmt, torch.cuda.current_stream().cuda_stream)
                assert code == 0
                torch.cuda.synchronize()
                got = flat.cpu().numpy()[base:base + H * stride].reshape(H, stride)
                want = given.copy()
                px = np.ascontiguousarray(want[:, :W * pb]).view(dt).reshape(H, W, 4)
                px[y0:y0 + h, x0:x0 + w, 3] = render(plane[y0:y0 + h, x0:x0 + w], bpp, fmt)
                want[:, :W * pb] = px.view(np.uint8).reshape(H, W * pb)
                assert np.array_equal(got, want), (bpp, hex(fmt), x0, y0, w, h)
    assert code4(L.j40hip_kat_device_alpha_merge(1, 16, 1, 4, 0, 0, 4, 1, 16, U8X4, None)) == "rnge"
    assert code4(L.j40hip_kat_device_alpha_merge(1, 16, 1, 4, 0, 0, 4, 1, 8, 0x0F34, None)) == "Ufm?"
