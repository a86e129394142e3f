"""CPU tests of the *device* functions: tests/hostsim compiles j40_amd/csrc/device/*_dev.h for the CPU
and runs them with the kernels' orchestration; results must equal the reference bit for bit
(quantised coefficients) and within 1 u8 level (RGBA; in practice identical)."""
import ctypes as C
import os

import numpy as np
import pytest

from streams import synth, VARDCT_CASES, MODULAR_CASES, ROOT


# libhostsim.so: the device functions compiled with the product's setting of J40_LANE_EV_FLUSH (the coefficient events leave with one store
# each); libhostsim_ring8.so: with the per-lane event rings (the build option EVENT_RING=8). The lane decoder's straight coefficient path
# differs between the two, so every test here runs through both.
@pytest.fixture(scope="module", params=["libhostsim.so", "libhostsim_ring8.so"], ids=["events_as_shipped", "event_rings_of_8"])
def sim(built, request):
    S = C.CDLL(os.path.join(ROOT, "build", request.param))
    S.hostsim_decode.restype = C.c_uint32
    S.hostsim_decode.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_int]
    return S


@pytest.mark.parametrize("name,opts", VARDCT_CASES[:8] + VARDCT_CASES[10:] + [("all_transforms", dict(maxlog=8, bctx=1, presets=2, orders=1))])
def test_device_functions_on_cpu_match_reference(ref, sim, name, opts):
    from refdec import RefStage
    w, h = (776, 520) if name == "all_transforms" else (392, 264)
    data = synth("vardct", w, h, 31, **opts)
    rs = RefStage(ref, data)
    ncells = sum(rs.lf_group_info(g)["width8"] * rs.lf_group_info(g)["height8"] for g in range(rs.info["num_lf_groups"]))
    rgba = np.zeros((h, w, 4), np.uint8)
    co = np.zeros((3, ncells * 64), np.float32)
    buf = C.create_string_buffer(data, len(data))
    assert sim.hostsim_decode(buf, len(data), rgba.ctypes.data, co.ctypes.data, 0) == 0
    base = 0
    for g in range(rs.info["num_lf_groups"]):
        n = rs.lf_group_info(g)["width8"] * rs.lf_group_info(g)["height8"] * 64
        for c in range(3):
            assert np.array_equal(rs.coeffs(g, c), co[c, base:base + n]), "quantised HF coefficients differ"
        base += n
    assert rs.combine() == ""
    d = np.abs(rs.rgba().astype(np.int32) - rgba.astype(np.int32))
    assert d.max() <= 1
    rs.close()


@pytest.mark.parametrize("name,opts", VARDCT_CASES + [("all_transforms", dict(maxlog=8, bctx=1, presets=2, orders=1))])
def test_flat_lane_decoder_matches_nested_decoder(sim, name, opts):
    """decode_hf_section_flat (one section per lane, throughput kernel) == decode_hf_section, coefficients and status"""
    w, h = (776, 520) if name == "all_transforms" else (392, 264)
    data = synth("vardct", w, h, 33, **opts)
    buf = C.create_string_buffer(data, len(data))
    n = ((w + 7) // 8) * ((h + 7) // 8) * 64 * 4   # generous: LF groups pad to whole cells
    a = np.zeros((3, n), np.float32); b = np.zeros((3, n), np.float32)
    rgba = np.zeros((h, w, 4), np.uint8)
    assert sim.hostsim_decode(buf, len(data), rgba.ctypes.data, a.ctypes.data, 1) == 0
    assert sim.hostsim_decode(buf, len(data), rgba.ctypes.data, b.ctypes.data, 3) == 0
    assert np.array_equal(a, b) and np.abs(a).sum() > 0
    # the rANS / no-LZ77 fast path of the throughput kernel (hf_lanes_dev.h); other specs report TODO and take the flat decoder
    c = np.zeros((3, n), np.float32)
    err = sim.hostsim_decode(buf, len(data), rgba.ctypes.data, c.ctypes.data, 5)
    if opts.get("hfprefix") or opts.get("hflz77"):
        assert err == 0x544F444F
    else:
        assert err == 0 and np.array_equal(a, c)
        # ... and with ONE lane taking every section of a pass from a queue, the largest first (k_hf_lanes' lanes take a further
        # section of their frame when they have finished one: decode_hf_sections_lane)
        q = np.zeros((3, n), np.float32)
        assert sim.hostsim_decode(buf, len(data), rgba.ctypes.data, q.ctypes.data, 13) == 0
        assert np.array_equal(a, q)


def test_large_transforms_levels_in_lds_and_64_point_registers_equal_the_sweeps_and_the_reference(ref, sim):
    """k_vardct_large's block function (large_dev.h: the top one or two levels of the recursion over the tile, every 64-point
    sub-vector through Idct1D<64> in a lane's registers; 128x64 tiles live in LDS all three channels at once, 128x128 ones a channel at
    a time with its events scattered per channel, 256-sized ones go through the scratch panel by panel; dense planes of two-pass
    frames) run on the CPU lane by lane: the same bits as the model of round 3's kernel (every level a sweep over a tile in the
    scratch), the reference's pixels, over streams in which every one of the six 128 / 256-sized transforms occurs
    (j40.h:5972-5990, 5802-5841)"""
    from refdec import RefStage
    seen = set()
    for (w, h, seed, opts) in [(1300, 1040, 5, {}), (776, 520, 31, {}), (1040, 1300, 8, {}), (1040, 776, 12, dict(passes=2)), (1040, 776, 13, dict(cfl=1)),
                               (520, 1300, 14, dict(dq=2, bctx=1))]:
        data = synth("vardct", w, h, seed, maxlog=8, **opts)
        rs = RefStage(ref, data)
        for g in range(rs.info["num_lf_groups"]):
            sel = (rs.plane(g, 0) >> 20) & 31
            seen |= set((sel[sel >= 2] - 2).tolist())
        assert rs.combine() == ""
        want = rs.rgba().astype(np.int32)
        rs.close()
        buf = C.create_string_buffer(data, len(data))
        outs = []
        for sweeps in (False, True):
            if sweeps:
                os.environ["HOSTSIM_LARGE_SWEEPS"] = "1"
            try:
                rgba = np.zeros((h, w, 4), np.uint8)
                assert sim.hostsim_decode(buf, len(data), rgba.ctypes.data, None, 0) == 0
            finally:
                os.environ.pop("HOSTSIM_LARGE_SWEEPS", None)
            outs.append(rgba)
        assert np.array_equal(outs[0], outs[1])
        assert np.abs(want - outs[0]).max() <= 1
    assert {21, 22, 23, 24, 25, 26} <= seen, sorted(seen)


def test_persistent_pixel_kernels_take_every_tile_once(sim):
    """k2_iter_dev.h, the walk of a persistent workgroup over its run of tiles (kernels.hip binds a frame's list, count and output
    only when the run enters the frame): over random batches -- frames without a block of the class, fewer tiles than workgroups,
    one workgroup, thousands -- every tile of every frame is taken exactly once with its first varblock and the frame's bindings"""
    sim.hostsim_k2_runs_check.restype = C.c_int32
    sim.hostsim_k2_runs_check.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32]
    rng = np.random.default_rng(4)
    for trial in range(400):
        nframes = int(rng.integers(1, 40))
        counts = rng.integers(0, 2000, nframes).astype(np.int32)
        counts[rng.random(nframes) < 0.3] = 0
        if trial % 7 == 0:
            counts[:] = 0
            counts[int(rng.integers(0, nframes))] = int(rng.integers(1, 5))
        per_wg = int(rng.choice([1, 2, 4, 8, 16, 32]))
        grid = int(rng.choice([1, 2, 3, 64, 257, 1024, 5000]))
        if trial == 3:
            counts[:] = 0   # (a batch without a block of the class: every run is empty)
        assert sim.hostsim_k2_runs_check(counts.ctypes.data, nframes, per_wg, grid) == 0, (counts.tolist(), per_wg, grid)


def test_fast_latency_decoder_matches_nested_decoder(sim, ref):
    """decode_hf_section_fast (hf_uni_dev.h: the latency kernel's fast path -- tables across lanes, the next coefficient's cluster
    fetched for both outcomes of the current one) against decode_hf_section on every single-pass rANS case: coefficients, and on
    damaged streams the same status, which is the reference's"""
    rng = np.random.default_rng(9)
    cases = [(392, 264, 33, o) for _, o in VARDCT_CASES if not (o.get("hfprefix") or o.get("hflz77") or o.get("passes"))]
    cases += [(776, 520, 33, dict(maxlog=8, bctx=1, presets=2, orders=1)), (1920, 1080, 34, dict(forward=1)), (2600, 2100, 35, dict(forward=1))]
    took = 0
    for (w, h, seed, opts) in cases:
        data = synth("vardct", w, h, seed, **opts)
        n = ((w + 7) // 8) * ((h + 7) // 8) * 64 * 4
        a = np.zeros((3, n), np.float32); q = np.zeros((3, n), np.float32); rgba = np.zeros((h, w, 4), np.uint8)
        buf = C.create_string_buffer(data, len(data))
        assert sim.hostsim_decode(buf, len(data), rgba.ctypes.data, a.ctypes.data, 1) == 0
        err = sim.hostsim_decode(buf, len(data), rgba.ctypes.data, q.ctypes.data, 17)
        if err == 0x544F444F:     # (a frame the fast path leaves to the general kernel: extra channels' trailers are fine, prefix codes are not)
            continue
        assert err == 0 and np.array_equal(a, q) and np.abs(a).sum() > 0, opts
        took += 1
        for trial in range(10):
            bad = bytearray(data)
            for _ in range(1 + trial % 2):
                bad[int(rng.integers(len(bad) // 3, len(bad)))] ^= 1 << int(rng.integers(0, 8))
            if trial == 9:
                bad = bad[:len(bad) - 7]
            bb = C.create_string_buffer(bytes(bad), len(bad))
            e1 = sim.hostsim_decode(bb, len(bad), rgba.ctypes.data, a.ctypes.data, 1)
            e2 = sim.hostsim_decode(bb, len(bad), rgba.ctypes.data, q.ctypes.data, 17)
            assert e1 == e2, (opts, trial, hex(e1), hex(e2))
            if w <= 400:
                rerr, _ = ref.decode(bytes(bad))
                assert ("".join(chr((e1 >> s) & 255) for s in (24, 16, 8, 0)) if e1 else "") == rerr
    assert took >= 12


def test_queued_lane_decoder_on_multi_group_frames_and_damage(sim):
    """decode_hf_sections_lane with many sections per lane: a 1920x1080 picture-encoded frame (40 sections, one lane takes them all),
    a three-pass frame, and bit flips -- coefficients and the frame's status equal the nested decoder's, section by section"""
    rng = np.random.default_rng(5)
    for (w, h, seed, opts) in [(1920, 1080, 34, dict(forward=1)), (1300, 776, 32, dict(passes=3)), (776, 520, 3, dict(maxlog=8, bctx=1, presets=2, orders=1))]:
        data = synth("vardct", w, h, seed, **opts)
        n = ((w + 7) // 8) * ((h + 7) // 8) * 64 * 4
        a = np.zeros((3, n), np.float32); q = np.zeros((3, n), np.float32); rgba = np.zeros((h, w, 4), np.uint8)
        buf = C.create_string_buffer(data, len(data))
        assert sim.hostsim_decode(buf, len(data), rgba.ctypes.data, a.ctypes.data, 1) == 0
        assert sim.hostsim_decode(buf, len(data), rgba.ctypes.data, q.ctypes.data, 13) == 0
        assert np.array_equal(a, q) and np.abs(a).sum() > 0
        for trial in range(12):
            bad = bytearray(data)
            bad[int(rng.integers(len(bad) // 3, len(bad)))] ^= 1 << int(rng.integers(0, 8))
            bb = C.create_string_buffer(bytes(bad), len(bad))
            assert sim.hostsim_decode(bb, len(bad), rgba.ctypes.data, a.ctypes.data, 1) == sim.hostsim_decode(bb, len(bad), rgba.ctypes.data, q.ctypes.data, 13)


@pytest.mark.parametrize("name,w,h,opts", MODULAR_CASES)
def test_modular_device_functions_on_cpu_are_bit_exact(ref, sim, name, w, h, opts):
    data = synth("modular", w, h, 61, **opts)
    err, expect = ref.decode(data)
    assert err == ""
    rgba = np.zeros(expect.shape, np.uint8)
    buf = C.create_string_buffer(data, len(data))
    assert sim.hostsim_decode(buf, len(data), rgba.ctypes.data, None, 0) == 0
    assert np.array_equal(rgba, expect)


def test_srgb_power_function_is_correctly_rounded(sim):
    """pow_1_over_2p4 (seeded fp64 root, idct_dev.h) == (float) pow((double) x, 1/2.4f): every 7th float of
    [2^-9, 4) and a coarse sweep of all positive floats"""
    import struct
    sim.hostsim_pow_sweep.restype = C.c_uint64
    sim.hostsim_pow_sweep.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(C.c_float)]
    sim.hostsim_srgb_u8_sweep.restype = C.c_uint64
    sim.hostsim_srgb_u8_sweep.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32]
    bits = lambda x: struct.unpack("<I", struct.pack("<f", x))[0]
    worst = C.c_float()
    n = (bits(4.0) - bits(2.0 ** -9)) // 7
    bad = sim.hostsim_pow_sweep(bits(2.0 ** -9), bits(4.0), 7, C.byref(worst))
    assert bad <= n // 1000000, "%d of %d results differ, e.g. x = %r" % (bad, n, worst.value)
    bad = sim.hostsim_pow_sweep(bits(2.0 ** -9), bits(3.0e38), 4099, C.byref(worst))
    assert bad <= 2, "x = %r" % worst.value
    assert sim.hostsim_srgb_u8_sweep(bits(1e-6), bits(300.0), 13) == 0
    sim.hostsim_srgb_u8_edges.restype = C.c_uint64
    assert sim.hostsim_srgb_u8_edges() == 0, "every threshold and bucket edge of the table path, +- 2 floats"


def test_lane_decoder_reports_the_same_errors_on_corrupt_streams(sim, ref):
    """bit flips in the pass-group sections: the throughput decoder (hf_lanes_dev.h), the nested decoder and the
    reference agree on the 4-char code (or on success)"""
    rng = np.random.default_rng(11)
    data = synth("vardct", 392, 264, 35)
    n = 392 * 264 * 64 // 16
    a = np.zeros((3, n), np.float32); rgba = np.zeros((264, 392, 4), np.uint8)
    seen = set()
    for trial in range(60):
        bad = bytearray(data)
        lo = len(bad) // 3   # past the headers and LF sections: the HF sections make up the tail
        for _ in range(1 + trial % 3):
            pos = int(rng.integers(lo, len(bad)))
            bad[pos] ^= 1 << int(rng.integers(0, 8))
        if trial % 7 == 0:
            bad = bad[:len(bad) - 1 - trial]   # truncated last section
        buf = C.create_string_buffer(bytes(bad), len(bad))
        e1 = sim.hostsim_decode(buf, len(bad), rgba.ctypes.data, a.ctypes.data, 1)
        e2 = sim.hostsim_decode(buf, len(bad), rgba.ctypes.data, a.ctypes.data, 5)
        assert e1 == e2, (trial, hex(e1), hex(e2))
        rerr, _ = ref.decode(bytes(bad))
        code = "".join(chr((e1 >> s) & 255) for s in (24, 16, 8, 0)) if e1 else ""
        assert code == rerr, (trial, code, rerr)
        seen.add(code)
    assert len(seen) >= 3, seen


def test_damage_behind_the_coefficients_of_alpha_frames(sim, ref):
    """VarDCT + alpha: the Modular sub-image behind each section's HF coefficients is decoded for its status (build_trailer_plan +
    the K3 section decoder), so bit flips anywhere in the sections give the reference's code"""
    data = synth("vardct", 520, 264, 33, alpha=1)
    rng = np.random.default_rng(5)
    out = np.zeros((264, 520, 4), np.uint8)
    sim.hostsim_decode.restype = C.c_uint32
    sim.hostsim_decode.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_int]
    rejected = 0
    for _ in range(60):
        mutated = bytearray(data)
        mutated[int(rng.integers(len(data) // 3, len(data)))] ^= 1 << int(rng.integers(0, 8))
        rerr, _ = ref.decode(bytes(mutated))
        buf = C.create_string_buffer(bytes(mutated), len(mutated))
        code = sim.hostsim_decode(buf, len(mutated), out.ctypes.data, None, 0)
        assert ("" if code == 0 else code.to_bytes(4, "big").decode("latin1")) == rerr
        rejected += rerr != ""
    assert rejected >= 30


def test_section_ends_are_checked_the_way_the_reference_checks_them(sim, ref):
    """In frames with several sections the reference notices neither junk behind a section's data nor a section that stops short of
    its end (j40__finish_section_state drops the error of its own j40__no_more_bytes, j40.h:7778-7795); single-section frames get
    `pad0` / `shrt`. Prefix-coded streams have no final-state check, so this decides whether a damaged stream is accepted."""
    sim.hostsim_decode.restype = C.c_uint32
    sim.hostsim_decode.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_int]

    def mine(d, w, h):
        out = np.zeros((h, w, 4), np.uint8)
        buf = C.create_string_buffer(d, len(d))
        code = sim.hostsim_decode(buf, len(d), out.ctypes.data, None, 0)
        return ("" if code == 0 else code.to_bytes(4, "big").decode("latin1")), out

    for mode, w, h, o in [("modular", 600, 300, dict(slack=2)), ("modular", 256, 256, dict(slack=2)), ("vardct", 520, 264, dict(slack=3)),
                          ("vardct", 520, 264, dict(slack=1, alpha=1)), ("modular", 600, 300, dict(slack=1, prefix=1, lz77=1)),
                          ("vardct", 200, 200, dict(slack=2, passes=2)), ("vardct", 392, 264, dict(slack=1, hfprefix=1))]:
        d = synth(mode, w, h, 9, **o)
        rerr, px = ref.decode(d)
        err, out = mine(d, w, h)
        assert err == rerr, (mode, o, rerr, err)
        if rerr == "":
            assert np.abs(px.astype(int) - out).max() <= (0 if mode == "modular" else 1)
    d = synth("modular", 762, 8, 236738, prefix=1, lz77=1)   # prefix codes: a flipped bit desynchronises the rest of the section
    rng = np.random.default_rng(3)
    for _ in range(80):
        b = bytearray(d)
        b[int(rng.integers(len(d) // 4, len(d)))] ^= 1 << int(rng.integers(8))
        rerr, px = ref.decode(bytes(b))
        err, out = mine(bytes(b), 762, 8)
        assert err == rerr and (rerr != "" or np.array_equal(px, out))


def test_every_header_bit_flip_ends_like_in_the_reference(sim, ref):
    """Each bit of the first bytes of small streams flipped in turn (image and frame headers, TOC, the start of LfGlobal): same verdict as the
    reference, error code included. Covers what the sweep found: a single-section frame is read to the end of the codestream and its
    end compared with the TOC entry afterwards (`shrt` / `excs`, j40.h:7884-7896); Squeeze parameters are read before the decoder
    gives up on them (j40.h:3794-3812); the first failing section in FILE order is the one reported when the TOC is permuted
    (j40.h:5608); VarDCT frames of images without xyb_encoded go through the XYB inverse regardless (j40.h:7206)."""
    sim.hostsim_decode.restype = C.c_uint32
    sim.hostsim_decode.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_int]
    beyond_reference = 0
    for mode, w, h, seed, nbytes, o in [("modular", 300, 200, 5, 40, {}), ("modular", 40, 30, 21, 70, dict(tree=2, alpha=1)),
                                        ("vardct", 264, 136, 4, 40, dict(dq=2, alpha=1)), ("vardct", 520, 264, 3, 70, dict(passes=2, permute=1)),
                                        ("modular", 64, 48, 3, 124, dict(icc=60))]:   # (frame header behind an ICC stream: extension skips
                                                                                      # depend on the accumulator's fill, j40.h:1895)
        d = synth(mode, w, h, seed, **o)
        for byte in range(2 if nbytes < 100 else 100, min(len(d), nbytes)):
            for bit in range(8):
                b = bytearray(d); b[byte] ^= 1 << bit; b = bytes(b)
                rerr, px = ref.decode(b)
                if rerr == "" and px.shape[:2] != (h, w): continue   # (a flip in the size header; the buffers here are sized for the clean stream)
                out = np.zeros((h, w, 4), np.uint8)
                buf = C.create_string_buffer(b, len(b))
                code = sim.hostsim_decode(buf, len(b), out.ctypes.data, None, 0)
                err = "" if code == 0 else code.to_bytes(4, "big").decode("latin1")
                if rerr == "TODO" and err != "TODO":
                    # a flip that turns a transform into a Squeeze: the reference stops there (j40.h:3812), this decoder carries on
                    beyond_reference += 1
                    continue
                assert err == rerr, (mode, w, h, seed, o, byte, bit, rerr, err)
                if rerr == "": assert np.abs(px.astype(int) - out).max() <= (0 if mode == "modular" else 1), (mode, byte, bit)
    assert beyond_reference <= 12, beyond_reference


def test_nsym4_simple_prefix_code_follows_the_reference_and_documents_the_rfc_difference(sim, ref):
    """Simple prefix code with four symbols, tree-select 0 (all codes two bits): the reference fills its table with the sorted
    symbols at the index made of the two bits in READ order (template {2,2,2,2}, symref {0,1,2,3}, j40.h:2090 / 2112), which swaps
    the sorted symbols 1 and 2 against RFC 7932's canonical code. The product follows the reference by default (results identical
    to the reference's); J40HIP_RFC_SIMPLE_CODES=1 selects the RFC order. Documented here with the exact differing output:
    a four-valued picture (samples 0..3, zero predictor, so tokens 0 / 2 / 4 / 6) written three ways by tools/jxlsynth --
    simple4=0: tree-select 1 (unaffected); simple4=1: tree-select 0 with the codes the reference reads; simple4=2: tree-select 0
    as an RFC 7932 encoder writes it."""
    import subprocess, sys
    w, h = 64, 48
    streams = [synth("modular", w, h, 3, prefix=1, rct=-1, tree=4, fourvalues=1, simple4=m) for m in (0, 1, 2)]
    sim.hostsim_decode.restype = C.c_uint32
    sim.hostsim_decode.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_int]

    def mine(d):
        out = np.zeros((h, w, 4), np.uint8)
        assert sim.hostsim_decode(C.create_string_buffer(d, len(d)), len(d), out.ctypes.data, None, 0) == 0
        return out
    refs = [ref.decode(d)[1] for d in streams]
    intended = refs[0]
    assert set(np.unique(intended[..., :3])) == {0, 1, 2, 3}
    assert np.array_equal(refs[1], intended)
    for d, r in zip(streams, refs):
        assert np.array_equal(mine(d), r), "default: identical to the reference on every form"
    # the RFC-encoded stream: the reference (and the default here) return the picture with the values 1 and 2 exchanged
    swapped = intended.copy()
    rgb = swapped[..., :3]
    ones, twos = intended[..., :3] == 1, intended[..., :3] == 2
    rgb[ones] = 2; rgb[twos] = 1
    assert np.array_equal(refs[2], swapped) and not np.array_equal(refs[2], intended)
    # ... and with the RFC order selected the same stream decodes to the intended picture
    code = ("import ctypes as C, numpy as np, sys\n"
            "S = C.CDLL(%r); S.hostsim_decode.restype = C.c_uint32\n"
            "S.hostsim_decode.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_int]\n"
            "d = open(sys.argv[1], 'rb').read(); out = np.zeros((%d, %d, 4), np.uint8)\n"
            "assert S.hostsim_decode(C.create_string_buffer(d, len(d)), len(d), out.ctypes.data, None, 0) == 0\n"
            "sys.stdout.buffer.write(out.tobytes())\n") % (os.path.join(ROOT, "build", "libhostsim.so"), h, w)
    path = os.path.join(ROOT, "build", "streams", "nsym4_rfc.jxl")
    open(path, "wb").write(streams[2])
    res = subprocess.run([sys.executable, "-c", code, path], env=dict(os.environ, J40HIP_RFC_SIMPLE_CODES="1"), capture_output=True, check=True)
    rfc = np.frombuffer(res.stdout, np.uint8).reshape(h, w, 4)
    assert np.array_equal(rfc, intended)


@pytest.mark.parametrize("sel", [1, 2, 3, 12, 13, 14, 15, 16, 17])
def test_cooperative_special_transforms_equal_the_reference_bit_for_bit(sim, ref, sel):
    """The nine 8x8 special transforms as k_vardct_special runs them (special8_dev.h: eight lanes per tile, two phases over tiles
    with rows nine floats apart) against the reference's routines (j40.h:5993-6246 via ref_kat_inverse_by_dctsel): identical floats
    -- out of place whatever the order in which the lanes of a phase run, and in place with the lanes in lockstep (the kernel's
    form: every phase loads all it needs before it stores anything)."""
    sim.hostsim_special8.argtypes = [C.c_int, C.c_void_p, C.c_int]
    sim.hostsim_special8_in_place.argtypes = [C.c_int, C.c_void_p]
    rng = np.random.default_rng(sel)
    for trial in range(120):
        a = (rng.standard_normal(64) * (10.0 ** rng.integers(-3, 3))).astype(np.float32)
        if trial % 3 == 0:
            a[rng.integers(0, 64, 40)] = 0
        expect = a.copy()
        scratch = np.zeros(256, np.float32)
        ref.lib.ref_kat_inverse_by_dctsel(expect.ctypes.data, scratch.ctypes.data, sel)
        for order in (0, 1, 2):
            got = a.copy()
            sim.hostsim_special8(sel, got.ctypes.data, order)
            assert np.array_equal(expect.view(np.uint32), got.view(np.uint32)), (sel, trial, order)
        got = a.copy()
        sim.hostsim_special8_in_place(sel, got.ctypes.data)
        assert np.array_equal(expect.view(np.uint32), got.view(np.uint32)), (sel, trial, "in place")


def test_lz77_distance_multiplier_of_lf_global_is_the_whole_images(sim, ref):
    """LfGlobal's stream belongs to the frame-wide Modular image: its LZ77 special distances are scaled by the widest non-meta
    channel of THAT image (j40.h:3840-3844), also when the section itself codes only the palette (multi-group frames). Found by
    tools/fuzz_parity.py: a flipped bit turned a distance token of the palette's stream into a special one, and this decoder
    (multiplier 0: no image channel in the section) read a different palette entry than the reference -- both without an error."""
    data = bytearray(synth("modular", 645, 28, 75417, palette=3, prefix=1, lz77=1, permute=1))
    data[1249] ^= 0x08
    data = bytes(data)
    rerr, expect = ref.decode(data)
    assert rerr == ""
    got = np.zeros((28, 645, 4), np.uint8)
    buf = C.create_string_buffer(data, len(data))
    assert sim.hostsim_decode(buf, len(data), got.ctypes.data, None, 0) == 0
    assert np.array_equal(got, expect)
    D = C.CDLL(os.path.join(ROOT, "build", "liboracle_driver.so"))
    D.oracle_run.restype = C.c_uint32
    D.oracle_run.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
    again = np.zeros((28, 645, 4), np.uint8)
    assert D.oracle_run(buf, len(data), again.ctypes.data, None) == 0
    assert np.array_equal(again, expect)


def test_device_memory_cache_bookkeeping(sim):
    """device/block_cache.hpp (free list, size classes, slabs) driven like device_memory.hip drives it, over a backend with a byte budget:
    random acquire / release / trim sequences keep every invariant (no overlapping blocks, byte counts, slabs freed only when idle,
    a failed allocation retried after a trim), with a roomy and with a tight budget and cache limit"""
    sim.hostsim_block_cache_selftest.restype = C.c_int32
    sim.hostsim_block_cache_selftest.argtypes = [C.c_uint32, C.c_int32, C.c_uint64, C.c_uint64]
    for seed, budget, limit in [(1, 288 << 30, 216 << 30), (2, 8 << 30, 6 << 30), (3, 3 << 30, 1 << 30), (4, 2 << 30, 0), (5, 64 << 30, 1 << 40)]:
        assert sim.hostsim_block_cache_selftest(seed, 4000, budget, limit) == 0, (seed, budget, limit)
