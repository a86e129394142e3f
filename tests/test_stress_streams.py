"""VarDCT streams outside an encoder's d1 statistics (streams.VARDCT_STRESS_CASES): dense blocks, event regions that really overflow,
coefficients beyond the event's int16 and up to the reference's 30-bit hybrid integers, other hybrid-integer configurations, the
quantiser's extremes (global_scale, quant_lf, extra_precision).

Bars. Quantised coefficients, LLF coefficients and error codes: exact. Pixels against the reference: max |delta| <= 1 and at most
size // 10000 + 4 differing samples (the bar of test_vardct_public_api_matches_reference); the one exemption is a sample whose value
before the reference's integer conversion, 255 t + 0.5 (maxpixel for 255 in deeper images), recomputed in float64 from the
restatement's XYB planes, is at or beyond 2^24 in magnitude -- there a float's ulp is 2 levels or more -- and the exempted share
must stay below 1 sample in 10000; it is printed per row. Between two of this project's own paths: identical.

The CPU half runs the device functions compiled for the host (tests/hostsim, both event forms) and the plain-C restatement; the GPU
half (-m gpu) sends every row through every way in: public API, Frame (events, then dense planes), Batch, Pipeline, StageDump, the
LF preview and the 16-bit output."""
import ctypes as C
import os
import signal

import numpy as np
import pytest

from streams import synth, VARDCT_CASES, VARDCT_STRESS_CASES, stress_size, stress_stream, ROOT

ROWS = VARDCT_STRESS_CASES
IDS = [r[0] for r in ROWS]
ROW = {r[0]: r for r in ROWS}
TODO, EVOF = 0x544F444F, 0x65766F66


def err4(code):
    return "".join(chr((code >> s) & 255) for s in (24, 16, 8, 0)) if code else ""


def leaves_the_events(opts, traits):
    """a single-pass frame whose first attempt (event lists) must end in "evof": a region too small, or a value beyond int16"""
    return bool(traits.get("overflows") or traits.get("evof") or traits.get("top_mag", 0) > 32767)


def lanes_todo(opts):
    return bool(opts.get("hfprefix") or opts.get("hflz77"))          # hf_lanes_dev.h: rANS without LZ77 only


def uni_todo(opts):
    return lanes_todo(opts) or opts.get("passes", 1) > 1             # hf_uni_dev.h: ... of single-pass frames


_REFERENCE = {}


def reference(ref, name):
    """the reference's verdict on a row, once per session: err, rgba, coeffs[g][c], llf[g][c], info"""
    if name not in _REFERENCE:
        from refdec import RefStage
        data = stress_stream(ROW[name][2])
        rerr, rgba = ref.decode(data)
        r = dict(err=rerr, rgba=rgba)
        if rerr == "":
            rs = RefStage(ref, data)
            n = rs.info["num_lf_groups"]
            r["info"] = rs.info
            r["cells"] = [rs.lf_group_info(g)["width8"] * rs.lf_group_info(g)["height8"] for g in range(n)]
            r["coeffs"] = [[rs.coeffs(g, c) for c in range(3)] for g in range(n)]
            r["llf"] = [[rs.llf(g, c) for c in range(3)] for g in range(n)]
            rs.close()
        _REFERENCE[name] = r
    return _REFERENCE[name]


def values_before_conversion(data, w, h, bpp):
    """maxpixel * t + 0.5 of j40.h:7208-7235 for every colour sample, in float64 from the restatement's XYB planes: [h, w, 3]"""
    D = C.CDLL(os.path.join(ROOT, "build", "liboracle_driver.so"))
    D.oracle_run_xyb.restype = C.c_uint32
    D.oracle_run_xyb.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p]
    xyb = np.zeros((3, h, w), np.float32)
    assert D.oracle_run_xyb(C.create_string_buffer(data, len(data)), len(data), xyb.ctypes.data) == 0
    import j40_amd
    fr = j40_amd.Frame(data)
    inv, bias, intensity_target, _, _ = fr.colour_consts()
    fr.close()
    x, y, b = xyb.astype(np.float64)
    bias = bias.astype(np.float64)
    p = np.stack([y + x, y - x, b])
    s = ((p - np.cbrt(bias)[:, None, None]) ** 3 + bias[:, None, None]) * (255.0 / float(intensity_target))
    v = np.einsum("ck,khw->hwc", inv.astype(np.float64), s)
    t = np.where(v <= 0.0031308, 12.92 * v, 1.055 * np.power(np.abs(v), 1.0 / 2.4) - 0.055)
    return float((1 << bpp) - 1) * t + 0.5


def check_pixels(name, data, opts, got, expect):
    """the bar of the module's docstring; prints the exempted share"""
    assert got is not None and got.shape == expect.shape and got.dtype == expect.dtype
    d = np.abs(got.astype(np.int32) - expect.astype(np.int32))
    exempted = 0
    if d.max() > 1:
        h, w = got.shape[:2]
        u = values_before_conversion(data, w, h, opts.get("bpp", 8))
        exempt = (d[..., :3] > 1) & (np.abs(u) >= 2.0 ** 24)
        exempted = int(exempt.sum())
        d[..., :3][exempt] = 0
    share = exempted / d.size
    print("%s: max |delta| %d, %d differing samples of %d, exempted (|255 t + 0.5| >= 2^24) %d = %.2e of the samples"
          % (name, int(d.max()), int((d > 0).sum()), d.size, exempted, share))
    assert share < 1e-4, share
    assert d.max() <= 1, "max |delta| %d at %s" % (int(d.max()), np.argwhere(d > 1)[:4].tolist())
    assert int((d > 0).sum()) <= d.size // 10000 + 4, int((d > 0).sum())


def check_coeffs(r, flat3, what):
    """flat3: [3, total cells * 64] in hostsim's / read_coeffs' layout against the reference's planes, bit for bit"""
    base = 0
    for g, cells in enumerate(r["cells"]):
        for c in range(3):
            assert np.array_equal(flat3[c][base:base + cells * 64].view(np.uint32), r["coeffs"][g][c].view(np.uint32)), (what, g, c)
        base += cells * 64


# ---------------------------------------------------------------- the rows themselves

@pytest.mark.parametrize("name", IDS)
def test_row_is_what_it_claims_to_be(built, ref, name):
    """so that a row cannot silently stop doing what it is there for (see streams.py for the traits)"""
    import j40_amd
    _, family, opts, traits = ROW[name]
    data = stress_stream(opts)
    r = reference(ref, name)
    assert r["err"] == traits.get("error", ""), r["err"]
    if r["err"]:
        return
    co = np.concatenate([np.concatenate(r["coeffs"][g]) for g in range(len(r["cells"]))])
    rgb = r["rgba"][..., :3]
    saturated = float(((rgb == 0) | (rgb == 255)).mean())
    fr = j40_amd.Frame(data)
    sizes = fr.section_sizes()
    fr.close()
    nz = int((co != 0).sum())
    print("%s: %d bytes, %d non-zeros, %.2f per section byte, largest magnitude %g, %.0f %% of the reference's colour samples saturated"
          % (name, len(data), nz, nz / sizes.sum(), np.abs(co).max(), 100 * saturated))
    if traits.get("unsaturated"):
        assert saturated < 0.5, saturated
    if traits.get("overflows"):
        # plan_build.cpp gives section i min(worst, 4 * bytes + 256) events: with more non-zeros than the sum of these some region is full
        assert nz > 4 * int(sizes.sum()) + 256 * len(sizes), (nz, int(sizes.sum()), len(sizes))
    if "top_mag" in traits:
        top = traits["top_mag"]
        low = (top + 1) // 2
        assert np.abs(co).max() == np.float32(top)
        for v in (low, -low, top, -top):     # both ends of [2^(k-1), 2^k) with both signs (as floats: exact up to 2^24)
            assert (co == np.float32(v)).any(), v
    if family == "dense":
        assert nz > co.size // 4     # X and B are drawn thinner than Y; default statistics: a few per cent


# ---------------------------------------------------------------- without a GPU

@pytest.fixture(scope="module", params=["libhostsim.so", "libhostsim_ring8.so"], ids=["events_as_shipped", "event_rings_of_8"])
def sim(built, request):
    S = C.CDLL(os.path.join(ROOT, "build", request.param))
    S.hostsim_decode.restype = C.c_uint32
    S.hostsim_decode.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_int]
    S.hostsim_first_attempt_status.restype = C.c_uint32
    return S


def run_sim(sim, data, w, h, mode):
    """(code, status of the attempt with events when a dense one followed, rgba, coefficients [3, cells * 64])"""
    rgba = np.zeros((h, w, 4), np.uint8)
    co = np.zeros((3, ((w + 7) // 8) * ((h + 7) // 8) * 64), np.float32)
    buf = C.create_string_buffer(data, len(data))
    code = sim.hostsim_decode(buf, len(data), rgba.ctypes.data, co.ctypes.data, mode)
    return code, sim.hostsim_first_attempt_status(), rgba, co


def modes_of(opts):
    """hostsim_decode's modes as tests/test_hostsim.py uses them, with the code each must end in on a stream the reference takes"""
    return [(1, 0), (3, 0), (5, TODO if lanes_todo(opts) else 0), (13, TODO if lanes_todo(opts) else 0), (16, TODO if uni_todo(opts) else 0)]


@pytest.mark.parametrize("name", IDS)
def test_device_functions_on_cpu_match_reference(ref, sim, name):
    """mode 0 (entropy decode and pixels as the kernels orchestrate them; "evof" answered with dense planes as the runtime does):
    coefficients, code and pixels against the reference. Modes 1 / 3 (nested and flat section decoder), 5 (hf_lanes fast path), 13
    (one lane taking the sections from a queue), 16 (hf_uni fast path): the coefficients and status of mode 0, or TODO where those
    paths leave a stream to the general decoder"""
    _, _, opts, traits = ROW[name]
    data = stress_stream(opts)
    w, h = stress_size(opts)
    r = reference(ref, name)
    code, first, rgba, co = run_sim(sim, data, w, h, 0)
    assert err4(code) == r["err"]
    if r["err"]:
        for mode, _ in modes_of(opts):
            assert err4(run_sim(sim, data, w, h, mode)[0]) == r["err"], mode
        return
    assert err4(first) == ("evof" if leaves_the_events(opts, traits) else ""), err4(first)
    check_coeffs(r, co, "mode 0")
    check_pixels(name, data, opts, rgba, r["rgba"])
    for mode, want in modes_of(opts):
        code_m, first_m, rgba_m, co_m = run_sim(sim, data, w, h, mode)
        assert code_m == want, (mode, err4(code_m))
        if want == 0:
            assert err4(first_m) == err4(first), (mode, err4(first_m))
            assert np.array_equal(co_m.view(np.uint32), co.view(np.uint32)), mode
            if not mode & 1:
                assert np.array_equal(rgba_m, rgba), mode


@pytest.mark.parametrize("name", IDS)
def test_restatement_matches_reference(built, ref, name):
    """oracle/hotpath_oracle.c, the other checker, has seen none of these streams either: coefficients, code, pixels"""
    _, _, opts, _ = ROW[name]
    data = stress_stream(opts)
    w, h = stress_size(opts)
    r = reference(ref, name)
    D = C.CDLL(os.path.join(ROOT, "build", "liboracle_driver.so"))
    D.oracle_run.restype = C.c_uint32
    D.oracle_run.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
    rgba = np.zeros((h, w, 4), np.uint8)
    cells = sum(r["cells"]) if not r["err"] else ((w + 7) // 8) * ((h + 7) // 8)
    co = np.zeros(3 * cells * 64, np.float32)
    code = D.oracle_run(C.create_string_buffer(data, len(data)), len(data), rgba.ctypes.data, co.ctypes.data)
    assert err4(code) == r["err"]
    if r["err"]:
        return
    off = 0
    for g, n in enumerate(r["cells"]):     # [lf group][channel][cells * 64]
        for c in range(3):
            assert np.array_equal(co[off:off + n * 64].view(np.uint32), r["coeffs"][g][c].view(np.uint32)), (g, c)
            off += n * 64
    check_pixels(name, data, opts, rgba, r["rgba"])


def decode_in_child(ref, data, limit=60):
    """ref.decode's code in a forked child: a damaged stream may crash the reference itself ("CRSH")"""
    rd, wr = os.pipe()
    pid = os.fork()
    if pid == 0:
        try:
            import faulthandler
            faulthandler.disable()     # (pytest's: a crash of the reference in here is an answer, not a report)
            signal.alarm(limit)
            err, _ = ref.decode(data)
            os.write(wr, ("%-4s" % err).encode("latin1"))
        finally:
            os._exit(0)
    os.close(wr)
    with os.fdopen(rd, "rb") as f:
        got = f.read()
    _, status = os.waitpid(pid, 0)
    return "CRSH" if status != 0 or len(got) < 4 else got[:4].decode("latin1").strip()


# one row per family for the damaged variants (the mix without an alpha channel: the lane modes of hostsim_decode do not look at
# the Modular sub-images behind the coefficients, test_damage_behind_the_coefficients_of_alpha_frames does that in mode 0)
DAMAGED = ["dense", "flat_ones", "big_22", "hybrid_720_big_22", "extra_precision_1_bctx", "mix_dense_12_bits_cfl"]


@pytest.mark.parametrize("name", DAMAGED)
def test_damaged_variants_end_like_in_the_reference(ref, sim, name):
    """nine variants with one or two flipped bits inside the pass-group sections and a truncated one: the reference's code (or its
    acceptance) in every mode. A variant that crashes the reference itself is skipped and counted, at most 2 in 10"""
    import j40_amd
    _, _, opts, _ = ROW[name]
    data = stress_stream(opts)
    w, h = stress_size(opts)
    fr = j40_amd.Frame(data)
    tail = int(fr.section_sizes().sum())     # the pass-group sections are the last ones of these streams
    fr.close()
    rng = np.random.default_rng(len(name))
    crashed, rejected = 0, 0
    for trial in range(10):
        bad = bytearray(data)
        for _ in range(1 + trial % 2):
            bad[int(rng.integers(len(bad) - tail, len(bad)))] ^= 1 << int(rng.integers(0, 8))
        if trial == 9:
            bad = bytearray(data[:len(data) - 7])
        bad = bytes(bad)
        rerr = decode_in_child(ref, bad)
        if rerr == "CRSH":
            crashed += 1
            continue
        rejected += rerr != ""
        for mode, want in [(0, 0)] + modes_of(opts):
            if want == TODO:
                continue
            assert err4(run_sim(sim, bad, w, h, mode)[0]) == rerr, (trial, mode, rerr)
    print("%s: %d of 10 variants rejected by the reference, %d crashed it" % (name, rejected, crashed))
    assert crashed <= 2 and rejected >= 1


QUANTISER = [r[0] for r in ROWS if r[1] == "quantiser"] + ["dense_quant_lf_16", "mix_flat_alpha_extra_precision"]


@pytest.mark.parametrize("name", QUANTISER)
def test_host_lf_image_under_the_quantisers_extremes(built, ref, name):
    """mult_lf = m_lf / (global_scale * quant_lf) * (65536 >> extra_precision) on the host (frame.cpp: the plain parse and the streamed
    parse read extra_precision at places of their own): the LLF coefficients of the plain parse bit for bit the reference's, the LF
    preview's plane equal to the reference's LLF on single-cell varblocks, and the streamed parse's plane equal to the plain one's"""
    import j40_amd
    from test_lf_preview import ref_single_cells, bits
    data = stress_stream(ROW[name][2])
    r = reference(ref, name)
    fr = j40_amd.Frame(data)
    for g in range(len(r["cells"])):
        for c in range(3):
            assert np.array_equal(bits(fr.llf(g, c)), bits(r["llf"][g][c])), (g, c)
    planes = [fr.lf_plane(c) for c in range(3)]
    fr.close()
    cells = ref_single_cells(ref, data)
    assert len(cells) > 100
    rows, cols = np.array([k[0] for k in cells]), np.array([k[1] for k in cells])
    expect = np.stack([cells[k] for k in cells])
    got = np.stack([planes[c][rows, cols] for c in range(3)], -1)
    assert np.array_equal(bits(got), bits(expect))
    fr = j40_amd.Frame.parse_streamed(data, step=512)
    for c in range(3):
        assert np.array_equal(bits(fr.lf_plane(c)), bits(planes[c])), c
    for g in range(len(r["cells"])):
        for c in range(3):
            assert np.array_equal(bits(fr.llf(g, c)), bits(r["llf"][g][c])), ("streamed", g, c)
    fr.close()


def test_out_of_range_samples_and_the_reference_s_power_function(built, ref):
    """global_scale=1 quant_lf=1 density=1 decay=1, seed 7: every colour sample is far out of range (the reference's int16 conversion
    wraps, j40.h:7235) and ONE of 411840 comes out two levels off (row 203, column 58, R: reference 40, device functions 38). The cause
    (DESIGN.md section 7): the reference's powf is glibc's, which is not correctly rounded (about 6 results in 10000 are one ulp off
    (float) pow((double) x, 1 / 2.4f)); the device function is correctly rounded. In range one ulp of t = 1.055 p - 0.055 moves
    255 t + 0.5 by 2e-5 levels; at that sample t is 38293, one ulp of it is 2^-8 and 255 ulps are one level, two after the rounding of
    the product and the sum. 255 t + 0.5 is 9.76e6 there: below 2^24, so the exemption of check_pixels does not cover it, and this
    decoder cannot follow a libm's rounding errors. What is asserted: the restatement (same libm) gives the reference's pixels; the
    device functions differ by more than one level only where |t| >= 2^15 (one ulp of t is 1 / 256 or more: at least one level),
    and at fewer than 1 sample in 10000; everywhere else the usual bar."""
    w, h = 520, 264
    data = synth("vardct", w, h, 7, global_scale=1, quant_lf=1, density=1, decay=1)
    rerr, expect = ref.decode(data)
    assert rerr == ""
    S = C.CDLL(os.path.join(ROOT, "build", "libhostsim.so"))
    S.hostsim_decode.restype = C.c_uint32
    S.hostsim_decode.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_int]
    rgba = np.zeros((h, w, 4), np.uint8)
    assert S.hostsim_decode(C.create_string_buffer(data, len(data)), len(data), rgba.ctypes.data, None, 0) == 0
    d = np.abs(rgba.astype(np.int32) - expect.astype(np.int32))
    t = (values_before_conversion(data, w, h, 8) - 0.5) / 255.0
    far = d[..., :3] > 1
    print("samples more than one level off: %d of %d, at |t| = %s" % (int(far.sum()), far.size, np.abs(t[far]).tolist()))
    assert not (far & (np.abs(t) < 2.0 ** 15)).any()
    assert far.sum() < far.size / 10000
    d[..., :3][far] = 0
    assert d.max() <= 1 and int((d > 0).sum()) <= d.size // 10000 + 4


# ---------------------------------------------------------------- on the GPU

@pytest.fixture(scope="module")
def gpu(built):
    import j40_amd
    assert j40_amd.device_count() > 0, "the gpu tests need a HIP device"
    return j40_amd


_PUBLIC = {}


def public_api(gpu, name):
    if name not in _PUBLIC:
        _PUBLIC[name] = gpu.decode(stress_stream(ROW[name][2]))
    return _PUBLIC[name]


def read_all_coeffs(fr, r):
    return [np.concatenate([fr.read_coeffs(g, c) for g in range(len(r["cells"]))]) for c in range(3)]


@pytest.mark.gpu
@pytest.mark.parametrize("name", IDS)
def test_public_api_and_single_frame_paths(gpu, ref, name):
    """j40_amd.decode: the reference's pixels / code. Frame.upload + decode_to_host: the same pixels, read_coeffs bit-exact (a frame
    that leaves the events is decoded again with dense planes by decode_to_host itself); then force_dense + upload + decode: identical"""
    _, _, opts, traits = ROW[name]
    data = stress_stream(opts)
    r = reference(ref, name)
    err, rgba = public_api(gpu, name)
    assert err == r["err"]
    fr = gpu.Frame(data)
    fr.upload(0)
    ferr, first = fr.decode_to_host()
    assert ferr == r["err"]
    if r["err"]:
        fr.close()
        return
    check_pixels(name, data, opts, rgba, r["rgba"])
    assert np.all(rgba[..., 3] == 255)
    assert np.array_equal(first, rgba)
    check_coeffs(r, read_all_coeffs(fr, r), "read_coeffs")
    if opts.get("passes", 1) == 1:
        fr.force_dense(True)
        fr.upload(0)
        derr, dense = fr.decode_to_host()
        assert derr == "" and np.array_equal(dense, rgba)
        check_coeffs(r, read_all_coeffs(fr, r), "read_coeffs, dense planes")
    fr.close()


def batch_of(gpu, ref, names):
    import torch
    frames, outs = [], []
    for name in names:
        opts = ROW[name][2]
        w, h = stress_size(opts)
        fr = gpu.Frame(stress_stream(opts))
        fr.upload(0)
        frames.append(fr)
        outs.append(torch.zeros((h, w, 4), dtype=torch.uint8, device="cuda:0"))
    batch = gpu.Batch(frames)
    batch.decode([o.data_ptr() for o in outs], [o.shape[1] * 4 for o in outs], torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    seen_evof = 0
    for name, fr, o in zip(names, frames, outs):
        _, _, opts, traits = ROW[name]
        r = reference(ref, name)
        err, single = public_api(gpu, name)
        status = fr.status()
        if r["err"]:
            assert status == r["err"] == err, (name, status)
        elif leaves_the_events(opts, traits):
            assert status == "evof", (name, status)
            seen_evof += 1
            fr.force_dense(True)      # include/j40hip.h: callers of the asynchronous entry points do this and upload / decode again
            fr.upload(0)
            derr, dense = fr.decode_to_host()
            assert derr == "" and np.array_equal(dense, single), name
            check_pixels(name, stress_stream(opts), opts, dense, r["rgba"])
        else:
            assert status == "", (name, status)
            assert np.array_equal(o.cpu().numpy(), single), name
    batch.close()
    for fr in frames:
        fr.close()
    return seen_evof


@pytest.mark.gpu
def test_batch_over_all_rows(gpu, ref):
    """one entropy launch over every row (prefix-coded members: the general lane decoder) and one over the rANS rows alone
    (k_hf_lanes' fast form): per frame the single-frame pixels and status; members that leave the events report "evof" and come out
    right after force_dense + upload + decode, their neighbours untouched"""
    assert batch_of(gpu, ref, IDS) >= 10
    rans = [n for n in IDS if not lanes_todo(ROW[n][2])]
    assert batch_of(gpu, ref, rans) >= 10


@pytest.mark.gpu
@pytest.mark.parametrize("lf_streams", ["device", "host"])
@pytest.mark.parametrize("device_output", [True, False], ids=["device_output", "host_output"])
def test_pipeline_over_all_rows(gpu, ref, lf_streams, device_output):
    """every row twice in one run, a plain frame between two rows that leave the events: pixels equal to the public API's, result(t)
    equal to its code, nothing left behind (an "evof" member must neither stall nor poison its batch neighbours)"""
    import torch
    plain = synth("vardct", 520, 264, 41, **VARDCT_CASES[0][1])
    perr, ppx = gpu.decode(plain)
    assert perr == ""
    jobs = []    # (data, expected code, expected pixels, width, height)
    for name in IDS:
        opts = ROW[name][2]
        w, h = stress_size(opts)
        err, px = public_api(gpu, name)
        jobs += [(stress_stream(opts), err, px, w, h)] * 2
    for name in ("flat_ones", None, "flat_ones_all_transforms", None, "big_16"):
        if name is None:
            jobs.append((plain, "", ppx, 520, 264))
        else:
            opts = ROW[name][2]
            w, h = stress_size(opts)
            jobs.append((stress_stream(opts),) + public_api(gpu, name) + (w, h))
    pipe = gpu.Pipeline(device=0, host_threads=4, batch_frames=16, max_in_flight=2, lf_streams=lf_streams)
    outs, tickets = [], []
    for data, _, _, w, h in jobs:
        o = torch.zeros((h, w, 4), dtype=torch.uint8, device="cuda:0") if device_output else np.zeros((h, w, 4), np.uint8)
        outs.append(o)
        tickets.append(pipe.submit(data, o.data_ptr() if device_output else o.ctypes.data, w * 4, device_output=device_output))
    pipe.drain()
    codes = [pipe.result(t) for t in tickets]
    completed = pipe.stats()["completed"]
    pipe.close()
    if device_output:
        torch.cuda.synchronize()
    assert completed == len(jobs), (completed, len(jobs))
    for i, ((data, err, px, w, h), o, code) in enumerate(zip(jobs, outs, codes)):
        assert code == err, (i, code, err)
        if err == "":
            assert np.array_equal(o.cpu().numpy() if device_output else o, px), i


@pytest.mark.gpu
@pytest.mark.parametrize("lf_on_device", [True, False], ids=["lf_on_device", "lf_on_host"])
@pytest.mark.parametrize("name", [n for n in QUANTISER if "alpha" not in n])
def test_device_stages_under_the_quantisers_extremes(gpu, ref, name, lf_on_device):
    """the pipeline's device stages (LfGroup streams, dequantisation and smoothing in lf_tail_kernels.hip, LLF) on the quantiser rows:
    bit-identical to the reference's internals, as test_device_stages.py has it for its cases"""
    from test_device_stages import compare
    compare(ref, stress_stream(ROW[name][2]), lf_on_device)


@pytest.mark.gpu
@pytest.mark.parametrize("name", [n for n in IDS if "extraprec" in ROW[n][2]])
def test_lf_preview_with_extra_precision(gpu, ref, name):
    """decode_lf / read_lf against j40hip_frame_lf_plane and the reference-derived plane, the way tests/test_lf_preview.py compares them"""
    from test_lf_preview import check_preview, U16X4
    data = stress_stream(ROW[name][2])
    for fmt in (gpu.J40_U8X4, U16X4):
        fr = gpu.Frame(data)
        fr.upload(0)
        _, ndiff = check_preview(gpu, ref, fr, data, fmt)
        if fmt == gpu.J40_U8X4:
            assert ndiff == 0
        fr.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["flat_ones", "big_16"])
def test_u16_output_of_frames_that_leave_the_events(gpu, ref, name):
    """J40_U16X4 through the dense fallback, against test_u16_output.py's rule (levels within one of the reference's planes)"""
    from test_u16_output import check_vardct
    check_vardct(gpu, ref, stress_stream(ROW[name][2]))
