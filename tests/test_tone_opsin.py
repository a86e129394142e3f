"""VarDCT decode under an image header that says something: ToneMapping (intensity_target) and the custom-transform block (opsin_inv_mat,
opsin_bias, quant_bias, quant_bias_num). Every other stream of the suite leaves both at their defaults, so a transposed matrix, one
bias used for three channels, a quant bias from the wrong slot or constants kept over from the frame before would pass it. The rows
are in tests/tone_streams.py; each runs as a plain stream, a forward-encoded one, one with every transform size (776 x 520) and, three
of them, at 12 bits.

Bars. Parsed constants, quantised coefficients, error codes: exact. Pixels against the reference: max |delta| <= 1 and at most
size // 10000 + 4 differing samples (test_stress_streams.check_pixels' bar). Pixels against an independent float64 evaluation of the
colour tail from the restatement's XYB planes and the constants THE TEST WROTE: no farther than the reference itself is on that row,
plus one level; the distances are printed per row. Exempt from both, below 1 sample in 10000: samples whose value before the integer
conversion is 2^24 or more in magnitude, or as close to a place where the reference's int16 conversion wraps as a float32 evaluation
can be off (float64_tail). Between two of this project's own paths: identical.

The CPU half runs the host parser, the device functions compiled for the host (both event forms, the dense form) and the plain-C
restatement; the GPU half (-m gpu) walks every way in, every output mode, the LF preview, Batch and the Pipeline with neighbours whose
constants differ -- among them one launch whose workgroups' runs cross frame borders."""
import concurrent.futures
import ctypes as C
import hashlib
import json
import os
import subprocess

import numpy as np
import pytest

from streams import synth, VARDCT_CASES, MODULAR_CASES, ROOT
import tone_streams as T
from test_stress_streams import err4, check_coeffs, run_sim, modes_of, read_all_coeffs

U8X4, U16X4 = 0x0F33, 0x0F35


def driver():
    D = C.CDLL(os.path.join(ROOT, "build", "liboracle_driver.so"))
    D.oracle_run_xyb.restype = C.c_uint32
    D.oracle_run_xyb.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p]
    D.oracle_run.restype = C.c_uint32
    D.oracle_run.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
    D.oracle_colour.restype = C.c_uint32
    D.oracle_colour.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
    D.oracle_view_consts.restype = C.c_uint32
    D.oracle_view_consts.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
    D.seam_roundtrip.restype = C.c_uint32
    D.seam_roundtrip.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_int]
    return D


_REFERENCE = {}


def reference(ref, name, tag):
    """the reference's verdict on a case, once per session: rgba, the twin's rgba, coeffs[g][c], cells, bpp"""
    if (name, tag) not in _REFERENCE:
        from refdec import RefStage
        data = T.stream(name, tag)
        rerr, rgba = ref.decode(data)
        assert rerr == "", "the reference refuses %s: %r" % (name, rerr)
        terr, twin = ref.decode(T.twin(name, tag))
        assert terr == ""
        rs = RefStage(ref, data)
        n = rs.info["num_lf_groups"]
        r = dict(err="", rgba=rgba, twin=twin, bpp=rs.info["bpp"])
        r["cells"] = [rs.lf_group_info(g)["width8"] * rs.lf_group_info(g)["height8"] for g in range(n)]
        r["coeffs"] = [[rs.coeffs(g, c) for c in range(3)] for g in range(n)]
        rs.close()
        _REFERENCE[(name, tag)] = r
    return _REFERENCE[(name, tag)]


_FLOAT64 = {}


def float64_tail(name, tag):
    """the colour tail of j40.h:7208-7235 in float64 on the restatement's XYB planes, with the constants the test wrote (mixed cube,
    bias, itscale, matrix, sRGB): (u = maxpixel * t + 0.5 [h, w, 3], the 8-bit pixels that follow from it [h, w, 3], exempt [h, w, 3])"""
    if (name, tag) not in _FLOAT64:
        data = T.stream(name, tag)
        opts = T.options_of(name, tag)
        w, h = T.size_of(opts)
        bpp = opts.get("bpp", 8)
        xyb = np.zeros((3, h, w), np.float32)
        assert driver().oracle_run_xyb(C.create_string_buffer(data, len(data)), len(data), xyb.ctypes.data) == 0
        m, bias, it, _, _ = T.expected_consts(T.ROW[name][1])
        x, y, b = xyb.astype(np.float64)
        bias = bias.astype(np.float64)
        p = np.stack([y + x, y - x, b])
        s = ((p - np.cbrt(bias)[:, None, None]) ** 3 + bias[:, None, None]) * (255.0 / float(it))
        v = np.einsum("ck,khw->hwc", m.astype(np.float64), s)
        t = np.where(v <= 0.0031308, 12.92 * v, 1.055 * np.power(np.abs(v), 1.0 / 2.4) - 0.055)
        maxpixel = (1 << bpp) - 1
        u = float(maxpixel) * t + 0.5
        big = np.abs(u) >= 2.0 ** 24
        i = np.trunc(np.where(big, 0.0, u)).astype(np.int64)
        i16 = ((i & 0xFFFF) ^ 0x8000) - 0x8000                  # the (int16_t) conversion as the reference's build performs it
        level = np.clip(i16, 0, maxpixel)
        px = (level * 255 + (1 << (bpp - 1))) // maxpixel
        r = np.mod(np.abs(u) - np.where(u >= 0, 32768.0, 32769.0), 65536.0)   # the conversion wraps at 32768 + 65536 k and at -32769 - 65536 k
        # ... where a float32 evaluation and this one may land on different sides of it. What a float32 evaluation can be off by: 32 of
        # its steps at u (the tail is a dozen roundings behind a cube, which triples a relative error), or, where the matrix row
        # cancels (a far negative value is the small difference of two large products), four roundings of the products' magnitudes
        # carried through the curve's slope
        slope = np.where(v <= 0.0031308, 12.92, 1.055 / 2.4 * np.power(np.maximum(np.abs(v), 0.0031308), 1.0 / 2.4 - 1.0))
        mag = np.einsum("ck,khw->hwc", np.abs(m.astype(np.float64)), np.abs(s))
        off = np.maximum(32.0 * np.spacing(np.abs(u).astype(np.float32)).astype(np.float64), float(maxpixel) * slope * mag * 4.0 * 2.0 ** -24)
        near_wrap = np.minimum(r, 65536.0 - r) < off
        _FLOAT64[(name, tag)] = (u, px, big | near_wrap)
    return _FLOAT64[(name, tag)]


def check_pixels(name, tag, got, expect, what=""):
    """the bar against the reference (module docstring); prints the exempted share"""
    assert got is not None and got.shape == expect.shape and got.dtype == expect.dtype
    d = np.abs(got.astype(np.int32) - expect.astype(np.int32))
    exempted = 0
    if d.max() > 1:
        exempt = (d[..., :3] > 1) & float64_tail(name, tag)[2]
        exempted = int(exempt.sum())
        d[..., :3][exempt] = 0
    share = exempted / d.size
    print("%s-%s %s: max |delta| %d, %d differing samples of %d, exempted %d = %.2e of the samples"
          % (name, tag, what, int(d.max()), int((d > 0).sum()), d.size, exempted, share))
    assert share < 1e-4, share
    assert d.max() <= 1, "max |delta| %d at %s" % (int(d.max()), np.argwhere(d > 1)[:4].tolist())
    assert int((d > 0).sum()) <= d.size // 10000 + 4, int((d > 0).sum())


def check_float64(name, tag, got, expect, what):
    """`got` is no farther from the float64 evaluation than the reference's pixels are on this case, plus one level"""
    _, px, exempt = float64_tail(name, tag)
    assert exempt.mean() < 1e-4, exempt.mean()
    ref_d = np.where(exempt, 0, np.abs(expect[..., :3].astype(np.int64) - px))
    got_d = np.where(exempt, 0, np.abs(got[..., :3].astype(np.int64) - px))
    print("%s-%s float64 distance: reference %d (%d samples off), %s %d (%d samples off), exempt %.2e"
          % (name, tag, int(ref_d.max()), int((ref_d > 0).sum()), what, int(got_d.max()), int((got_d > 0).sum()), exempt.mean()))
    assert got_d.max() <= ref_d.max() + 1, (int(got_d.max()), int(ref_d.max()))
    return int(ref_d.max()), int(got_d.max())


# ---------------------------------------------------------------- the rows themselves

@pytest.mark.parametrize("name,tag", T.CASES, ids=T.CASE_IDS)
def test_row_is_what_it_claims_to_be(built, ref, name, tag):
    """from the reference's decode alone, so that a row cannot quietly stop testing anything"""
    r = reference(ref, name, tag)
    rgb, twin = r["rgba"][..., :3].astype(np.int32), r["twin"][..., :3].astype(np.int32)
    saturated = float(((rgb == 0) | (rgb == 255)).mean())
    differing = float((np.abs(rgb - twin) > 1).mean())
    print("%s-%s: %.3f of the reference's colour samples saturated, %.3f more than one level from the twin's, mean level %.1f"
          % (name, tag, saturated, differing, rgb.mean()))
    if name == "tone_255":
        assert np.array_equal(r["rgba"], r["twin"])
        return
    if not name.startswith("tone_half") and name != "tone_max":
        assert saturated < 0.5, saturated
    assert differing >= (0.05 if name == "qbias" else 0.9), differing
    if name == "tone_max":        # the sRGB curve's linear segment ends at level 255 * 12.92 * 0.0031308 = 10.3
        assert (rgb <= 10).mean() > 0.9, (rgb <= 10).mean()
    if name == "tone_half_12_bit":
        u, _, exempt = float64_tail(name, tag)
        wrapped = (rgb == 0) & (u > 4096.0) & ~exempt
        print("%s-%s: %d samples at level 0 whose float64 value lies above the largest level" % (name, tag, int(wrapped.sum())))
        assert wrapped.any()


# ---------------------------------------------------------------- without a GPU: the parsers

def consts_of(D, fr, through_seam=0):
    a = np.zeros(17, np.float32)
    assert D.oracle_view_consts(fr.h, a.ctypes.data, through_seam) == 0
    return a


def expected17(name):
    m, bias, it, qb, qn = T.expected_consts(T.ROW[name][1])
    return np.concatenate([m.reshape(-1), bias, [it], qb, [qn]]).astype(np.float32)


@pytest.mark.parametrize("name", T.NAMES)
def test_parsed_constants_are_the_written_ones(built, name):
    """Frame.colour_consts() and the plan view (quant_bias, quant_bias_num too), of the plain parse, of the streamed parse and of a handle
    built from the view: the table the test wrote, bit for bit (an f16 is exact in a float32)"""
    import j40_amd
    D = driver()
    want = expected17(name)
    for tag in ("plain", "all_transforms"):
        data = T.stream(name, tag)
        whole = j40_amd.Frame(data)
        lf_only = j40_amd.Frame(data[:whole.lf_end()], lf_only=True)     # (the LF preview's parse: it has no plan view)
        for how, fr in (("plain", whole), ("streamed", j40_amd.Frame.parse_streamed(data, step=512)), ("lf_only", lf_only)):
            m, bias, it, _, _ = fr.colour_consts()
            assert np.array_equal(np.concatenate([m.reshape(-1), bias, [it]]).astype(np.float32).view(np.uint32), want[:13].view(np.uint32)), (name, how)
            if how != "lf_only":
                assert np.array_equal(consts_of(D, fr).view(np.uint32), want.view(np.uint32)), (name, how)
                assert np.array_equal(consts_of(D, fr, 1).view(np.uint32), want.view(np.uint32)), (name, how, "through the seam")
            fr.close()


BAD_TONE = [("0,1", "tone"), ("-64,1", "tone"), ("64,0", "tone"), ("64,128", "tone"), ("64,1,1.5,1", "tone"), ("64,1,-1", "tone")]
_OPSIN = T.written_options(T.ROW["swapped_all"][1])["opsin"]
REFUSED = [("tone_" + t.replace(",", "_"), dict(tone=t)) for t, _ in BAD_TONE] + \
          [("cw_mask_%d" % k, dict(opsin=_OPSIN, cwmask=k)) for k in (1, 2, 4)] + \
          [("opsin_field_%d_not_finite" % k, dict(opsin=",".join(bits if i == k else v for i, v in enumerate(_OPSIN.split(",")))))
           for k, bits in ((0, "h7c00"), (10, "hfc00"), (15, "h7e00"))]      # an f16 with exponent 31: +inf, -inf, a NaN


def refused_stream(opts, **more):
    return synth("vardct", 520, 264, T.SEED, **dict(opts, **more))


@pytest.mark.parametrize("what,opts", REFUSED, ids=[r[0] for r in REFUSED])
def test_refusals_without_a_gpu(built, ref, what, opts):
    """headers the reference refuses (a ToneMapping out of range, custom upsampling weights, an f16 that is not finite): its code from
    Frame, from the streamed parse and from the device functions compiled for the host"""
    import j40_amd
    data = refused_stream(opts)
    rerr, _ = ref.decode(data)
    assert rerr != "", "the reference takes this stream"
    if what.startswith("tone_"):
        assert rerr == "tone"
    with pytest.raises(j40_amd.J40Error) as e:
        j40_amd.Frame(data)
    assert e.value.code == rerr
    with pytest.raises(j40_amd.J40Error) as e:
        j40_amd.Frame.parse_streamed(data, step=512)
    assert e.value.code == rerr
    with pytest.raises(j40_amd.J40Error) as e:
        j40_amd.Frame(data, lf_only=True)
    assert e.value.code == rerr
    S = C.CDLL(os.path.join(ROOT, "build", "libhostsim.so"))
    S.hostsim_decode.restype = C.c_uint32
    S.hostsim_decode.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_int]
    rgba = np.zeros((264, 520, 4), np.uint8)
    assert err4(S.hostsim_decode(C.create_string_buffer(data, len(data)), len(data), rgba.ctypes.data, None, 0)) == rerr
    D = driver()
    assert err4(D.oracle_run(C.create_string_buffer(data, len(data)), len(data), rgba.ctypes.data, None)) == rerr


def test_every_header_branch_carries_the_blocks(built, ref):
    """the generator's header branches (plain, bpp=, alpha=1, icc=, frames=, lflevels=; noxyb=1: default_m = 0 and no values): the
    reference takes each stream, its pixels differ from the twin's, and the parsed constants are the written ones"""
    import j40_amd
    consts = T.ROW["swapped_all_tone_1000"][1]
    w = T.written_options(consts)
    want = expected17("swapped_all_tone_1000")
    for extra in (dict(), dict(bpp=12), dict(alpha=1), dict(icc=700), dict(alpha=1, bpp=12), dict(orientation=5), dict(container=1)):
        data = synth("vardct", 520, 264, T.SEED, **dict(extra, **w))
        rerr, px = ref.decode(data)
        terr, tpx = ref.decode(synth("vardct", 520, 264, T.SEED, **extra))
        assert rerr == terr == "", (extra, rerr)
        assert (np.abs(px[..., :3].astype(np.int32) - tpx[..., :3]) > 1).mean() > 0.9, extra
        fr = j40_amd.Frame(data)
        assert np.array_equal(consts_of(driver(), fr).view(np.uint32), want.view(np.uint32)), extra
        fr.close()
    # the generator's two spellings of a value, decimal and f16 bits, write the same bytes; a decimal an f16 does not hold is refused
    decimal = T.written_options(consts, T._num)
    assert decimal["opsin"] != w["opsin"] and synth("vardct", 264, 200, T.SEED, **decimal) == synth("vardct", 264, 200, T.SEED, **w)
    with pytest.raises(subprocess.CalledProcessError):
        synth("vardct", 264, 200, T.SEED, tone="1000.25,1")     # (an f16's steps are 0.5 there)
    # not XYB: the block holds cw_mask alone, the constants stay the defaults, the pixels the twin's
    extra = dict(alpha=1, fullheader=1, noxyb=1)
    data = synth("vardct", 520, 264, T.SEED, **dict(extra, opsin=w["opsin"]))
    twin = synth("vardct", 520, 264, T.SEED, **extra)
    assert len(data) <= len(twin) + 1
    rerr, px = ref.decode(data)
    assert rerr == "" and np.array_equal(px, ref.decode(twin)[1])
    fr = j40_amd.Frame(data)
    assert np.array_equal(consts_of(driver(), fr).view(np.uint32), expected17("tone_255").view(np.uint32))
    fr.close()


def _fresh(args):
    mode, w, h, seed, opts = args
    import tempfile
    with tempfile.TemporaryDirectory() as d:     # (not through the stream cache: what the generator writes now)
        out = os.path.join(d, "s.jxl")
        subprocess.run([os.path.join(ROOT, "build", "jxlsynth"), mode, str(w), str(h), str(seed), out] + ["%s=%s" % kv for kv in sorted(opts.items())],
                       check=True, stderr=subprocess.DEVNULL)
        with open(out, "rb") as fp:
            return hashlib.sha256(fp.read()).hexdigest()


def test_streams_without_the_new_options_are_unchanged(built):
    """every VARDCT_CASES / MODULAR_CASES stream and the benchmark's first one: the bytes the generator wrote before it learnt tone= and
    opsin= (tests/golden/stream_digests.json)"""
    with open(os.path.join(ROOT, "tests", "golden", "stream_digests.json")) as fp:
        want = json.load(fp)
    jobs = {"vardct/" + n: ("vardct", 520, 264, 41, o) for n, o in VARDCT_CASES}
    jobs.update({"modular/" + n: ("modular", w, h, 71, o) for n, w, h, o in MODULAR_CASES})
    jobs["bench/vardct_7680x4320_seed_3_forward"] = ("vardct", 7680, 4320, 3, dict(forward=1))
    assert set(jobs) == set(want)
    keys = sorted(jobs, key=lambda k: -jobs[k][1] * jobs[k][2])
    with concurrent.futures.ThreadPoolExecutor(max_workers=8) as ex:
        got = dict(zip(keys, ex.map(_fresh, [jobs[k] for k in keys])))
    assert got == want, [k for k in keys if got[k] != want[k]]


# ---------------------------------------------------------------- without a GPU: device functions and the restatement

@pytest.fixture(scope="module", params=["libhostsim.so", "libhostsim_ring8.so"], ids=["events_as_shipped", "event_rings_of_8"])
def sim(built, request):
    S = C.CDLL(os.path.join(ROOT, "build", request.param))
    S.hostsim_decode.restype = C.c_uint32
    S.hostsim_decode.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_int]
    S.hostsim_first_attempt_status.restype = C.c_uint32
    S.hostsim_decode_dense.restype = C.c_uint32
    S.hostsim_decode_dense.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_int]
    return S


@pytest.mark.parametrize("name,tag", T.CASES, ids=T.CASE_IDS)
def test_device_functions_on_cpu_match_reference(ref, sim, name, tag):
    """as test_stress_streams.py has it: mode 0 (entropy decode and pixels as the kernels orchestrate them), then the nested and the flat
    section decoder, the lane fast paths and hf_uni: coefficients bit for bit the reference's, pixels within the bar and within the
    float64 bar; J40HIPSIM_DENSE forces the dense planes (the third scatter form, vardct_dev.h)"""
    opts = T.options_of(name, tag)
    data = T.stream(name, tag)
    w, h = T.size_of(opts)
    r = reference(ref, name, tag)
    code, first, rgba, co = run_sim(sim, data, w, h, 0)
    assert code == 0 and first == 0, (err4(code), err4(first))
    check_coeffs(r, co, "mode 0")
    check_pixels(name, tag, rgba, r["rgba"], "device functions")
    check_float64(name, tag, rgba, r["rgba"], "device functions")
    if name == "tone_255":
        tcode, _, trgba, _ = run_sim(sim, T.twin(name, tag), w, h, 0)
        assert tcode == 0 and np.array_equal(rgba, trgba), "written-out defaults: the twin's pixels"
    for mode, want in modes_of(opts):
        code_m, first_m, rgba_m, co_m = run_sim(sim, data, w, h, mode)
        assert code_m == want == 0, (mode, err4(code_m))
        assert np.array_equal(co_m.view(np.uint32), co.view(np.uint32)), mode
        if not mode & 1:
            assert np.array_equal(rgba_m, rgba), mode
    # dense coefficient planes from the start: the dequantiser's third form (vardct_dev.h), the same pixels
    dense = np.zeros((h, w, 4), np.uint8)
    dco = np.zeros_like(co)
    assert sim.hostsim_decode_dense(C.create_string_buffer(data, len(data)), len(data), dense.ctypes.data, dco.ctypes.data, 0) == 0
    assert np.array_equal(dco.view(np.uint32), co.view(np.uint32))
    assert np.array_equal(dense, rgba), "dense planes"


@pytest.mark.parametrize("name,tag", T.CASES, ids=T.CASE_IDS)
def test_restatement_matches_reference(built, ref, name, tag):
    """oracle/hotpath_oracle.c reads the view's constants: coefficients, pixels, and the float64 distances of the module's docstring"""
    opts = T.options_of(name, tag)
    data = T.stream(name, tag)
    w, h = T.size_of(opts)
    r = reference(ref, name, tag)
    D = driver()
    rgba = np.zeros((h, w, 4), np.uint8)
    co = np.zeros(3 * sum(r["cells"]) * 64, np.float32)
    assert D.oracle_run(C.create_string_buffer(data, len(data)), len(data), rgba.ctypes.data, co.ctypes.data) == 0
    off = 0
    for g, n in enumerate(r["cells"]):
        for c in range(3):
            assert np.array_equal(co[off:off + n * 64].view(np.uint32), r["coeffs"][g][c].view(np.uint32)), (g, c)
            off += n * 64
    check_pixels(name, tag, rgba, r["rgba"], "restatement")
    check_float64(name, tag, rgba, r["rgba"], "restatement")


# ---------------------------------------------------------------- on the GPU

@pytest.fixture(scope="module")
def gpu(built):
    import j40_amd
    assert j40_amd.device_count() > 0, "the gpu tests need a HIP device"
    return j40_amd


_PUBLIC = {}


def public_api(gpu, data):
    """j40_amd.decode's pixels of a stream the reference takes, once per session"""
    key = hashlib.sha256(data).digest()
    if key not in _PUBLIC:
        err, px = gpu.decode(data)
        assert err == "", err
        _PUBLIC[key] = px
    return _PUBLIC[key]


@pytest.mark.gpu
@pytest.mark.parametrize("name,tag", T.CASES, ids=T.CASE_IDS)
def test_public_api_and_single_frame_paths(gpu, ref, name, tag):
    """every way in: j40_amd.decode against the reference and the float64 evaluation; Frame with events and after force_dense, and the
    pipeline's device stages (StageDump): the same pixels; read_coeffs bit for bit the reference's"""
    data = T.stream(name, tag)
    r = reference(ref, name, tag)
    rgba = public_api(gpu, data)
    check_pixels(name, tag, rgba, r["rgba"], "public API")
    check_float64(name, tag, rgba, r["rgba"], "public API")
    assert np.all(rgba[..., 3] == 255)
    if name == "tone_255":
        assert np.array_equal(rgba, public_api(gpu, T.twin(name, tag))), "written-out defaults: the twin's pixels"
    fr = gpu.Frame(data)
    fr.upload(0)
    ferr, first = fr.decode_to_host()
    assert ferr == "" and np.array_equal(first, rgba)
    check_coeffs(r, read_all_coeffs(fr, r), "read_coeffs")
    fr.force_dense(True)
    fr.upload(0)
    derr, dense = fr.decode_to_host()
    assert derr == "" and np.array_equal(dense, rgba), "dense planes"
    check_coeffs(r, read_all_coeffs(fr, r), "read_coeffs, dense planes")
    fr.close()
    d = gpu.StageDump(data)
    assert d.verdict == "" and np.array_equal(d.rgba(), rgba), "StageDump"
    d.close()


# the rows whose pictures every output mode is run on: the matrix's orientation with everything else, the sRGB curve's linear segment,
# clamping at the top
MODES = [("swapped_all", "plain"), ("swapped_all", "all_transforms"), ("swapped_all", "twelve"), ("tone_10000", "plain"), ("tone_10000", "all_transforms"),
         ("tone_64", "plain"), ("tone_64", "all_transforms"), ("tone_64", "twelve")]
MODE_IDS = ["%s-%s" % m for m in MODES]


@pytest.mark.gpu
@pytest.mark.parametrize("name,tag", MODES + [("tone_max", "plain")], ids=MODE_IDS + ["tone_max-plain"])
def test_u16_output(gpu, ref, name, tag):
    """J40_U16X4 against the reference's own levels (test_u16_output.check_vardct)"""
    from test_u16_output import check_vardct
    check_vardct(gpu, ref, T.stream(name, tag))


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["tone_10000", "tone_max"])
def test_u16_output_resolves_the_linear_segment(gpu, ref, name):
    """at 12 bits the sRGB curve's linear segment is 166 levels wide (4095 * 12.92 * 0.0031308), which eight bits squeeze into ten: the
    16-bit output keeps them, against the reference's own levels"""
    from test_u16_output import check_vardct, level_of
    px = check_vardct(gpu, ref, T.stream(name, "plain", bpp=12))
    lv = level_of(px[..., :3], 12)
    inside = lv[lv <= 165]
    print("%s at 12 bits: %d of %d samples in the linear segment, %d different levels among them" % (name, inside.size, lv.size, len(np.unique(inside))))
    assert inside.size > lv.size // 10 and len(np.unique(inside)) > 100, (inside.size, len(np.unique(inside)))


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", [U8X4, U16X4], ids=["u8x4", "u16x4"])
@pytest.mark.parametrize("name,tag", MODES, ids=MODE_IDS)
def test_scaled_output_is_the_box_of_the_full_decode(gpu, name, tag, fmt):
    """the fused 1:2 and 1:4 tails of the three kernel families"""
    from test_scale import box
    from test_scale_gpu import full_and_scaled
    full, got = full_and_scaled(gpu, T.stream(name, tag), fmt)
    if fmt == U8X4:
        assert np.array_equal(full, public_api(gpu, T.stream(name, tag)))
    for k, (px, sc) in got.items():
        assert np.array_equal(px, box(full, k)), (name, tag, k)
        assert (sc["shift"], sc["staged"]) == (k, 0)


@pytest.mark.gpu
@pytest.mark.parametrize("name,tag", MODES, ids=MODE_IDS)
def test_region_across_a_group_border(gpu, ref, name, tag):
    from test_region import check_regions
    w, h = T.size_of(T.options_of(name, tag))
    check_regions(gpu, ref, T.stream(name, tag), [(190, 180, 141, h - 180), (250, 0, 13, 9)], False, 1)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("name,tag", [m for m in MODES if m[1] != "twelve"], ids=[i for i in MODE_IDS if "twelve" not in i])
def test_restoration_modes(gpu, ref, name, tag, mode):
    """Gaborish and the edge-preserving filter between the pixel kernels and the colour tail: the samples left in XYB (the dequantiser's
    constants) bit for bit the restatement's, k_xyb_to_rgba on the filtered planes against the restatement's tail on the same planes"""
    D = driver()
    more = dict(fullheader=1, gab=1, epf=2)
    data = T.stream(name, tag, **more)
    w, h = T.size_of(T.options_of(name, tag))
    buf = C.create_string_buffer(data, len(data))
    fr = gpu.Frame(data)
    fr.upload(0)
    err, plain = fr.decode_to_host()
    rerr, expect = ref.decode(data)
    assert err == rerr == ""
    d = np.abs(plain.astype(np.int32) - expect.astype(np.int32))
    assert d.max() <= 1 and int((d > 0).sum()) <= d.size // 10000 + 4
    fr.set_restoration(mode)
    err, rgba = fr.decode_to_host()
    assert err == ""
    xyb0, xyb1 = fr.read_xyb(0), fr.read_xyb(1)
    want0 = np.zeros((3, h, w), np.float32)
    assert D.oracle_run_xyb(buf, len(data), want0.ctypes.data) == 0
    assert np.array_equal(xyb0.view(np.uint32), want0.view(np.uint32))
    want = np.zeros((h, w, 4), np.uint8)
    assert D.oracle_colour(buf, len(data), np.ascontiguousarray(xyb1).ctypes.data, want.ctypes.data) == 0
    assert np.abs(rgba.astype(np.int32) - want.astype(np.int32)).max() <= 1
    assert (rgba != plain).any(), "the filters changed the picture"
    fr.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name,tag", [m for m in MODES if m[1] == "plain"], ids=[i for i in MODE_IDS if "plain" in i])
def test_kept_alpha_orientation_and_the_plan_view_seam(gpu, ref, name, tag):
    D = driver()
    # alpha=1, kept: the colour samples of the drop-mode decode, the alpha plane of the twin
    data, twin = T.stream(name, tag, alpha=1), T.twin(name, tag, alpha=1)
    rerr, expect = ref.decode(data)
    assert rerr == ""
    dropped = public_api(gpu, data)
    d = np.abs(dropped.astype(np.int32) - expect.astype(np.int32))
    assert d.max() <= 1 and int((d > 0).sum()) <= d.size // 10000 + 4
    err, kept = gpu.decode(data, alpha=True)
    terr, tkept = gpu.decode(twin, alpha=True)
    assert err == terr == ""
    assert np.array_equal(kept[..., :3], dropped[..., :3]) and np.array_equal(kept[..., 3], tkept[..., 3]) and kept[..., 3].min() < 255
    # orientation 5
    from test_orient_gpu import stored_oriented_stored, check
    odata = T.stream(name, tag, orientation=5)
    full, turned, said = stored_oriented_stored(gpu, odata, 5)
    check(full, turned, said, 5)
    assert np.array_equal(full, public_api(gpu, T.stream(name, tag))), "the orientation changes no sample"
    # a handle built from the plan view, and from the LF bundle: identical pixels
    for tg in ("plain", "all_transforms"):
        sdata = T.stream(name, tg)
        direct = public_api(gpu, sdata)
        buf = C.create_string_buffer(sdata, len(sdata))
        for m in (1, 3):
            rgba = np.zeros_like(direct)
            assert D.seam_roundtrip(buf, len(sdata), rgba.ctypes.data, m) == 0
            assert np.array_equal(rgba, direct), (tg, m)


# ---------------------------------------------------------------- the LF preview

def written_preview_consts(name, fr):
    """test_lf_preview.restate's constants with matrix, bias and intensity_target as the test wrote them (the chroma-from-luma factors
    are no part of these blocks: as parsed)"""
    m, bias, it, _, _ = T.expected_consts(T.ROW[name][1]) if name else T.expected_consts({})
    _, _, _, kx, kb = fr.colour_consts()
    return m, bias, it, kx, kb


def check_preview_pixels(ref, name, fr, px):
    from test_lf_preview import restate, to_u8
    lv = restate(ref, [fr.lf_plane(c) for c in range(3)], written_preview_consts(name, fr), fr.info["bpp"])
    d = np.abs(px[..., :3].astype(np.int64) - to_u8(lv, fr.info["bpp"]))
    assert d.max() <= 1 and np.all(px[..., 3] == 255), (name, int(d.max()))
    return int((d > 0).sum())


@pytest.mark.gpu
@pytest.mark.parametrize("name", T.NAMES)
def test_lf_preview(gpu, ref, name):
    """decode_lf (runtime_lfp.hip copies the constants by hand) against the restated tail fed with the written constants"""
    data = T.stream(name, "plain")
    fr = gpu.Frame(data)
    fr.upload(0)
    px = fr.decode_lf_to_host()
    ndiff = check_preview_pixels(ref, name, fr, px)
    print("%s: preview samples unequal to the restatement: %d" % (name, ndiff))
    if fr.info["bpp"] == 8:
        assert ndiff == 0
    fr.close()
    err, again = gpu.decode_lf(data)
    assert err == "" and np.array_equal(again, px), "the LF-only parse"


@pytest.mark.gpu
def test_lf_previews_of_frames_with_different_constants_in_one_launch(gpu, ref):
    names = [None, "swapped_all", "tone_10000", "bias_positive"] * 3
    datas = [T.twin("tone_255") if n is None else T.stream(n, "plain") for n in names]
    err, outs = gpu.decode_lf_many(datas)
    assert err == ""
    for n, data, px in zip(names, datas, outs):
        fr = gpu.Frame(data)
        assert check_preview_pixels(ref, n, fr, px) == 0, n
        fr.close()
    assert not np.array_equal(outs[0], outs[1]) and not np.array_equal(outs[1], outs[2]) and not np.array_equal(outs[2], outs[3])


# ---------------------------------------------------------------- batches: neighbours with different constants

def interleaved(tags):
    """(name, tag) so that neighbours always differ in constants: the rows in an order that alternates the two blocks"""
    order = ["tone_255", "swapped_all", "tone_64", "bias_distinct", "tone_1000", "qbias", "tone_10000", "bias_zero", "tone_max", "bias_positive", "tone_half",
             "swapped_all_tone_1000", "tone_half_12_bit"]
    assert sorted(order) == sorted(T.NAMES)
    return [(n, t) for t in tags for n in order]


@pytest.mark.gpu
def test_batch_of_frames_with_different_constants(gpu):
    import torch
    jobs = interleaved(["plain", "all_transforms"])
    frames, outs = [], []
    for name, tag in jobs:
        w, h = T.size_of(T.options_of(name, tag))
        fr = gpu.Frame(T.stream(name, tag))
        fr.upload(0)
        frames.append(fr)
        outs.append(torch.zeros((h, w, 4), dtype=torch.uint8, device="cuda:0"))
    batch = gpu.Batch(frames)
    batch.decode([o.data_ptr() for o in outs], [o.shape[1] * 4 for o in outs], torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    for (name, tag), fr, o in zip(jobs, frames, outs):
        assert fr.status() == "", (name, tag, fr.status())
        assert np.array_equal(o.cpu().numpy(), public_api(gpu, T.stream(name, tag))), (name, tag)
    batch.close()
    for fr in frames:
        fr.close()


@pytest.mark.gpu
@pytest.mark.parametrize("shift", [0, 1], ids=["full", "half"])
@pytest.mark.parametrize("lf_streams", ["device", "host"])
@pytest.mark.parametrize("device_output", [True, False], ids=["device_output", "host_output"])
def test_pipeline_over_all_rows(gpu, lf_streams, device_output, shift):
    """every row twice in one run, neighbours always differing in constants: the public API's pixels (at 1:2, their box), served by the
    batched kernels (the front parse and the device-side plan carry the constants)"""
    import torch
    from test_scale import box
    jobs = interleaved(["plain", "all_transforms", "plain"]) + interleaved(["forward"])[:5]
    pipe = gpu.Pipeline(device=0, host_threads=4, batch_frames=16, max_in_flight=2, lf_streams=lf_streams)
    if shift:
        assert pipe.set_scale(shift) == ""
    outs, tickets = [], []
    for name, tag in jobs:
        w, h = T.size_of(T.options_of(name, tag))
        w, h = (w + (1 << shift) - 1) >> shift, (h + (1 << shift) - 1) >> shift
        o = torch.zeros((h, w, 4), dtype=torch.uint8, device="cuda:0") if device_output else np.zeros((h, w, 4), np.uint8)
        outs.append(o)
        tickets.append(pipe.submit(T.stream(name, tag), o.data_ptr() if device_output else o.ctypes.data, w * 4, device_output=device_output))
    pipe.drain()
    codes = [pipe.result(t) for t in tickets]
    stats = pipe.stats()
    pipe.close()
    if device_output:
        torch.cuda.synchronize()
    assert codes == [""] * len(jobs), codes
    assert stats["completed"] == len(jobs) and stats["single_frames"] == 0 and stats["launch_frames"] == len(jobs), stats
    for (name, tag), o in zip(jobs, outs):
        want = public_api(gpu, T.stream(name, tag))
        assert np.array_equal(o.cpu().numpy() if device_output else o, box(want, shift) if shift else want), (name, tag)


def k2_launch(gpu, l):
    a = np.zeros(5, np.int32)
    L = gpu.lib()
    L.j40hip_debug_k2_launch.restype = C.c_int32
    L.j40hip_debug_k2_launch.argtypes = [C.c_int32, C.c_void_p]
    n = L.j40hip_debug_k2_launch(l, a.ctypes.data)
    return n, dict(zip(("a", "b", "per_wg", "min_cells", "wg_slots"), a.tolist()))


@pytest.mark.gpu
def test_pipeline_runs_that_cross_a_frame_border(gpu, ref):
    """the persistent batch kernels load a frame's constants when a workgroup's run ENTERS the frame. Three 1000 x 1000 streams of 8x8
    DCT blocks alone, with different constants, 36 frames in one launch: more tiles than a launch gets workgroups, so every workgroup
    walks two tiles, and with an odd number of tiles per frame every other frame border lies inside a run. Every output: its stream's
    single-frame pixels exactly, the reference's within the bar"""
    import torch
    W = H = 1000
    FRAMES = 36
    names = ["tone_255", "swapped_all", "tone_1000"]
    datas = [T.twin("tone_255", size=(W, H), dct8only=1)] + [T.stream(n, size=(W, H), dct8only=1) for n in names[1:]]
    want = []
    for n, data in zip(names, datas):
        px = public_api(gpu, data)
        rerr, expect = ref.decode(data)
        assert rerr == ""
        d = np.abs(px.astype(np.int32) - expect.astype(np.int32))
        print("%s 1000 x 1000: max |delta| %d, %d differing samples" % (n, int(d.max()), int((d > 0).sum())))
        assert d.max() <= 1 and int((d > 0).sum()) <= d.size // 10000 + 4
        want.append(px)
    assert not np.array_equal(want[0], want[1]) and not np.array_equal(want[1], want[2]) and not np.array_equal(want[0], want[2])
    # the precondition, from the kernels' own table and the frames' own class counts
    nlaunches, dct8 = k2_launch(gpu, 0)
    assert (dct8["a"], dct8["b"]) == (0, 1) and nlaunches > 1
    tiles = []
    for data in datas:
        d = gpu.StageDump(data)
        cs = d.sorted_varblocks()[2]
        d.close()
        assert int(cs[27]) == int(cs[dct8["b"]]) - int(cs[dct8["a"]]) == ((W + 7) // 8) * ((H + 7) // 8), "8x8 DCT blocks alone"
        tiles.append(-(-(int(cs[dct8["b"]]) - int(cs[dct8["a"]])) // dct8["per_wg"]))
    total = sum(tiles) * (FRAMES // 3)
    chunk = -(-total // dct8["wg_slots"])
    borders = np.cumsum([tiles[k % 3] for k in range(FRAMES)])[:-1]
    inside = int((borders % chunk != 0).sum())
    print("tiles per frame %s, %d in all for %d workgroups: runs of %d tiles, %d of %d frame borders inside a run" % (tiles, total, dct8["wg_slots"], chunk, inside, FRAMES - 1))
    assert total > dct8["wg_slots"] and chunk >= 2 and inside >= (FRAMES - 1) // 3
    pipe = gpu.Pipeline(device=0, host_threads=4, batch_frames=FRAMES, max_in_flight=1, lf_streams="device")
    outs = [torch.zeros((H, W, 4), dtype=torch.uint8, device="cuda:0") for _ in range(FRAMES)]
    tickets = [pipe.submit(datas[k % 3], o.data_ptr(), W * 4, device_output=True) for k, o in enumerate(outs)]
    pipe.drain()
    codes = [pipe.result(t) for t in tickets]
    stats = pipe.stats()
    pipe.close()
    torch.cuda.synchronize()
    assert codes == [""] * FRAMES, codes
    print("launches %d, launch_frames %d, single_frames %d" % (stats["launches"], stats["launch_frames"], stats["single_frames"]))
    assert stats["launches"] == 1 and stats["launch_frames"] == FRAMES and stats["single_frames"] == 0, stats
    for k, o in enumerate(outs):
        assert bool((o == torch.from_numpy(want[k % 3]).to("cuda:0")).all()), "frame %d (%s)" % (k, names[k % 3])


# ---------------------------------------------------------------- frame sequences and LF frames: one row each

@pytest.mark.gpu
def test_animation_with_custom_constants(gpu, ref):
    """frames=3 with swapped_all in the image header: each coded frame alone against the reference, the canvases by
    test_frames_gpu.py's scheme"""
    from test_frames_gpu import play_and_check, stream_opts, VARDCT, VARDCT_CROPS
    w = T.written_options(T.ROW["swapped_all"][1])
    rows, got = play_and_check(gpu, ref, "vardct", 520, 264, stream_opts(dict(VARDCT, **w), VARDCT_CROPS))
    _, plain = play_and_check(gpu, ref, "vardct", 520, 264, stream_opts(VARDCT, VARDCT_CROPS))
    assert len(got) == len(plain) == 3 and all(not np.array_equal(a, b) for a, b in zip(got, plain))
    assert (np.abs(got[0][..., :3].astype(np.int32) - plain[0][..., :3]) > 1).mean() > 0.9, "the first frame covers the canvas"


@pytest.mark.gpu
def test_lf_frame_with_custom_constants(gpu, ref):
    """lflevels=1 with swapped_all_tone_1000 against its twin with the same constants, byte for byte (test_lf_frames_gpu.py's rule)"""
    from lf_streams import WIDE, lf_stream, lf_twin
    from test_lf_frames_gpu import play, twin_pixels
    w = T.written_options(T.ROW["swapped_all_tone_1000"][1])
    want = twin_pixels(gpu, ref, WIDE, dict(w))
    seq, px = play(gpu, lf_stream(WIDE, **w))
    seq.close()
    assert np.array_equal(px, want)
    assert (np.abs(want[..., :3].astype(np.int32) - twin_pixels(gpu, ref, WIDE, dict())[..., :3]) > 1).mean() > 0.9


# ---------------------------------------------------------------- refusals

@pytest.mark.gpu
def test_refusals_on_the_gpu(gpu, ref):
    """the reference's code from the public API and from the pipeline's result(ticket), the refused frames between two good ones"""
    good = T.stream("swapped_all", "plain")
    jobs = [good]
    for _, opts in REFUSED:
        jobs += [refused_stream(opts), good]
    want = [ref.decode(d)[0] for d in jobs]
    assert want[0] == "" and all(c != "" for c in want[1::2])
    for d, code in zip(jobs[1::2], want[1::2]):
        err, px = gpu.decode(d)
        assert err == code and px is None
    pipe = gpu.Pipeline(device=0, host_threads=2, batch_frames=8, max_in_flight=2)
    outs = [np.zeros((264, 520, 4), np.uint8) for _ in jobs]
    tickets = [pipe.submit(d, o.ctypes.data, 520 * 4) for d, o in zip(jobs, outs)]
    pipe.drain()
    codes = [pipe.result(t) for t in tickets]
    pipe.close()
    assert codes == want, (codes, want)
    for o, code in zip(outs, want):
        assert np.array_equal(o, public_api(gpu, good)) if code == "" else not o.any()
