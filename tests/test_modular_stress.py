"""Modular streams outside an encoder's habits (streams.MODULAR_STRESS_CASES): LZ77 copies at every special distance code under
several multipliers, at plain distances up to 2^20, overlapping themselves, crossing row and channel ends, starting before the first
decoded integer and ending behind the last needed one; the header's other LZ77 selectors; weighted-predictor parameters other than
the defaults, in the global header, in the pass-group headers and different in both; predicted palettes with every predictor;
samples over the whole of int16, inverse RCTs that wrap, coarse leaves, residuals that take a sample beyond int16.

Bars. Modular output is bit-exact and error codes are equal: there is no tolerance in this module.

The CPU half runs the device functions compiled for the host (tests/hostsim, either neighbour source on every section) and the
plain-C restatement against the unmodified reference; the GPU half (-m gpu) sends every row and every damaged variant through the
public API, once per kernel switch in a child process of its own (the switches are read once per process), and the deep rows
through the 16-bit output."""
import ctypes as C
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

from streams import synth, synth_stats, stress_size, MODULAR_STRESS_CASES, MODULAR_STRESS_SQUEEZE, VARDCT_STRESS_CASES, STRESS_SEED, ROOT, SYNTH
from test_stress_streams import decode_in_child, err4

ROWS = MODULAR_STRESS_CASES
IDS = [r[0] for r in ROWS]
ROW = {r[0]: r for r in ROWS}
FAMILIES = ["lz_forced", "lz_match", "wp", "palette", "range", "overflow"]


def stream(name):
    _, _, (w, h), opts, _ = ROW[name]
    return synth("modular", w, h, STRESS_SEED, **opts)


_REFERENCE = {}


def reference(ref, name):
    """the reference's verdict on a row, once per session: (code, rgba or None)"""
    if name not in _REFERENCE:
        _REFERENCE[name] = ref.decode(stream(name))
    return _REFERENCE[name]


def test_the_matrix_is_what_the_module_says():
    assert len(set(IDS)) == len(IDS)
    assert sorted({r[1] for r in ROWS}) == sorted(FAMILIES)
    widths = {r[2][0] for r in ROWS}
    assert {1, 2, 7, 8, 63, 64, 65, 1030} <= widths


# ---------------------------------------------------------------- the rows themselves

@pytest.mark.parametrize("name", IDS)
def test_row_is_what_it_claims_to_be(built, ref, name):
    """the traits of streams.py against the generator's own account of the stream, and the reference's code"""
    _, _, (w, h), opts, traits = ROW[name]
    stats, data = synth_stats("modular", w, h, STRESS_SEED, **opts)
    assert data == stream(name), "stats=1 must not change the stream"
    print(name, len(data), "bytes", {k: v for k, v in stats.items() if v not in (0, -1)})
    for key, floor in traits.get("at_least", {}).items():
        assert stats[key] >= floor, (key, stats[key], floor)
    for key, value in traits.get("exactly", {}).items():
        assert stats[key] == value, (key, stats[key], value)
    for key, value in traits.get("every", {}).items():
        assert len(stats[key]) >= 1 and all(v == value for v in stats[key]), (key, stats[key], value)
    assert reference(ref, name)[0] == traits.get("error", "")


VARDCT_ROWS = [r for r in VARDCT_STRESS_CASES if "stats" in r[3]]


@pytest.mark.parametrize("name", [r[0] for r in VARDCT_ROWS])
def test_vardct_row_is_what_it_claims_to_be(built, name):
    """the LZ77 and weighted-predictor rows appended to streams.VARDCT_STRESS_CASES (tests/test_stress_streams.py walks them through
    every decoder, on the CPU and on the GPU, Batch and Pipeline included): the floors of their `stats` trait"""
    _, _, opts, traits = [r for r in VARDCT_ROWS if r[0] == name][0]
    w, h = stress_size(opts)
    stats, data = synth_stats("vardct", w, h, STRESS_SEED, **opts)
    assert data == synth("vardct", w, h, STRESS_SEED, **opts)
    print(name, len(data), "bytes", stats)
    for key, floor in traits["stats"].items():
        assert stats[key] >= floor, (key, stats[key], floor)
    if "hflzmode" in opts:
        assert stats["copies"] > stats["distance_one_copies"] > 0      # distances other than "the value before", and that one too
    if opts.get("wpat") == "global":
        assert stats["wp_headers"] == 1                                 # the header that decodes nothing is the only one with parameters


def test_lz77_rows_cover_the_table_under_a_clamping_multiplier(built):
    """a multiplier below 8 makes max(1, dx + mult * dy) act: in a frame one sample wide no code reaches beyond 8 + 7 = 15, and every
    code with dx + dy < 1 stands for the distance 1"""
    _, _, (w, h), opts, _ = ROW["specials_1x1000_groupshift_10"]
    stats, _ = synth_stats("modular", w, h, STRESS_SEED, **opts)
    assert stats["distinct_special_codes"] == 120 and stats["distance_one_copies"] >= 60 and stats["max_distance"] == 15


# ---------------------------------------------------------------- without a GPU

@pytest.fixture(scope="module")
def sim(built):
    S = C.CDLL(os.path.join(ROOT, "build", "libhostsim.so"))
    S.hostsim_decode.restype = C.c_uint32
    S.hostsim_decode.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_int]
    S.hostsim_set_neighbour_flip.argtypes = [C.c_int32]
    yield S
    S.hostsim_set_neighbour_flip(0)


@pytest.fixture(scope="module")
def oracle(built):
    D = C.CDLL(os.path.join(ROOT, "build", "liboracle_driver.so"))
    D.oracle_run.restype = C.c_uint32
    D.oracle_run.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
    return D


def run_sim(sim, data, w, h, flip):
    rgba = np.zeros((h, w, 4), np.uint8)
    sim.hostsim_set_neighbour_flip(flip)
    code = sim.hostsim_decode(C.create_string_buffer(data, len(data)), len(data), rgba.ctypes.data, None, 0)
    return err4(code), rgba


def run_oracle(oracle, data, w, h):
    rgba = np.zeros((h, w, 4), np.uint8)
    code = oracle.oracle_run(C.create_string_buffer(data, len(data)), len(data), rgba.ctypes.data, None)
    return err4(code), rgba


@pytest.mark.parametrize("name", IDS)
def test_device_functions_on_cpu_match_reference(ref, sim, name):
    """decode_modular_section with either neighbour source on every section: the reference's pixels, or its code"""
    w, h = ROW[name][2]
    rerr, expect = reference(ref, name)
    for flip in (0, 1):
        err, rgba = run_sim(sim, stream(name), w, h, flip)
        assert err == rerr, (flip, err, rerr)
        if rerr == "":
            assert np.array_equal(rgba, expect), (flip, int((rgba != expect).sum()))


@pytest.mark.parametrize("name", IDS)
def test_restatement_matches_reference(ref, oracle, name):
    """oracle/hotpath_oracle.c, the other checker. (early_groups found it keeping one window for all sections of a code: a copy from
    before a later section's first integer read the section before it instead of zeros)"""
    w, h = ROW[name][2]
    rerr, expect = reference(ref, name)
    err, rgba = run_oracle(oracle, stream(name), w, h)
    assert err == rerr
    if rerr == "":
        assert np.array_equal(rgba, expect)


def squeeze_row(ref, name):
    """(stream, the reference's pixels for the same picture coded without Squeeze)"""
    _, (w, h), opts = [r for r in MODULAR_STRESS_SQUEEZE if r[0] == name][0]
    rerr, expect = ref.decode(synth("modular", w, h, STRESS_SEED, **{k: v for k, v in opts.items() if k != "squeeze"}))
    assert rerr == ""
    return synth("modular", w, h, STRESS_SEED, **opts), expect


@pytest.mark.parametrize("name", [r[0] for r in MODULAR_STRESS_SQUEEZE])
def test_lz77_under_squeeze_on_cpu(ref, sim, oracle, name):
    """a section whose channels differ in width: the multiplier is the widest one's. Every special code occurs; the device functions and
    the restatement give the picture the reference decodes from the stream without Squeeze"""
    _, (w, h), opts = [r for r in MODULAR_STRESS_SQUEEZE if r[0] == name][0]
    stats, _ = synth_stats("modular", w, h, STRESS_SEED, **opts)
    assert stats["distinct_special_codes"] == 120 and stats["special_copies"] >= 1000 and stats["sections"] > 1
    data, expect = squeeze_row(ref, name)
    assert ref.decode(data)[0] == "TODO"
    for flip in (0, 1):
        err, rgba = run_sim(sim, data, w, h, flip)
        assert err == "" and np.array_equal(rgba, expect), flip
    err, rgba = run_oracle(oracle, data, w, h)
    assert err == "" and np.array_equal(rgba, expect)


def sections_of(data):
    import j40_amd
    fr = j40_amd.Frame(data)
    coop, total = fr.coop_sections()
    split = fr.split_sections()
    sizes = fr.section_sizes()
    fr.close()
    return coop, split, total, sizes


def test_which_kernels_the_rows_belong_to(built):
    """the forced LZ77 rows are the two-pass decoder's by default (k_modular_tokens: one leaf, no property), so are the matcher's rows
    over position-only trees; some rows are the cooperative kernel's, some the general one's (weighted predictor)"""
    taken = {}
    for name, family, _, opts, traits in ROWS:
        if traits.get("error") == "iovf":
            continue
        coop, split, total, _ = sections_of(stream(name))
        taken[name] = (coop, split, total)
        assert 0 <= coop and coop + split <= total and total >= 1, name
        if family == "lz_forced":     # (LfGlobal's section of a frame of several groups codes no channel: nobody's)
            assert split == (total if total == 1 else total - 1), (name, coop, split, total)
        if opts.get("tree") == 2:
            assert coop == 0 and split == 0, (name, coop, split, total)
    assert taken["match_special"][1] == taken["match_special"][2] - 1 and taken["match_overlap_single_alpha"][1:] == (1, 1)
    assert taken["coarse_leaves_position_tree_prefix_lz77"][1] > 0
    cooperative = [n for n, (coop, _, _) in taken.items() if coop > 0]
    print("cooperative kernel:", cooperative)
    assert {"coarse_leaves_neighbour_tree", "noise_15_bit_wide_tree", "overflow_wide_tree"} <= set(cooperative)


# ---------------------------------------------------------------- damaged variants

# per family one row with prefix codes (a flipped bit desynchronises what follows: often accepted) and one with rANS (its final
# state notices nearly every flip); the overflow family's prefix row has its overflow in the last section only, late in it, so
# that a flip ahead of it can take the section another way
DAMAGED = {
    "lz_forced": ["specials_groups_128_and_44", "specials_200x100_lzminsym_100", "early_groups"],
    "lz_match": ["match_special", "match_plain"],
    "wp": ["match_special_wp_tree_custom_wp", "wp_both"],
    "palette": ["palette_dpred_6_prefix", "local_palette_dpred_6_both", "palette_dpred_6_max"],
    "range": ["noise_15_bit_property_tree_prefix", "noise_15_bit_rct_wraps"],
    "overflow": ["overflow_last_section_prefix", "overflow_last_section_rans", "overflow_matcher"],
}
EXTRA_ROWS = {
    # (rows of the damaged families that are not part of the matrix proper)
    # the overflow in the last section alone, 20000 samples into it; the generator says where the overflowing residual's extra bits
    # lie, and the first six variants are aimed: the residual made small (no overflow left), damage ahead of it and behind it with and
    # without the overflow -- "povf" against a parse error on either side of it, which the two-pass decoder finds in different passes
    "overflow_last_section_prefix": ((300, 200), dict(povf=20000, povfsection=1, povfto=33000, bpp=15, rct=-1, prefix=1)),
    "overflow_last_section_rans": ((300, 200), dict(povf=20000, povfsection=1, povfto=33000, bpp=15, rct=-1)),
}
VARIANTS = 12


def damaged_stream(name):
    if name in EXTRA_ROWS:
        (w, h), opts = EXTRA_ROWS[name]
        return (w, h), synth("modular", w, h, STRESS_SEED, **opts)
    return ROW[name][2], stream(name)


def variants_of(name):
    """VARIANTS damaged copies of a row: one or two flipped bits inside the sections (behind the image and frame headers; the last
    section alone for the row whose overflow sits there), and two truncations. Deterministic in the row's name"""
    _, data = damaged_stream(name)
    sizes = sections_of(data)[3]
    tail = int(sizes[-1]) if name in EXTRA_ROWS else int(sizes.sum())
    rng = np.random.default_rng(sum(name.encode()))
    out = []
    aimed = []
    if name in EXTRA_ROWS:
        (w, h), opts = EXTRA_ROWS[name]
        (bit, nbits, extra), = synth_stats("modular", w, h, STRESS_SEED, **opts)[0]["povf_extra_bits"]
        small = [bit + k for k in range(nbits) if (extra >> k) & 1]      # flipping these clears the residual's extra bits
        aimed = [small, small + [bit + 4000], [bit - 4000], [bit + 4000], [bit - 40], small + [bit - 4000]]
    for trial in range(VARIANTS):
        bad = bytearray(data)
        if trial < len(aimed):
            for b in aimed[trial]:
                bad[b >> 3] ^= 1 << (b & 7)
        elif trial >= VARIANTS - 2:
            bad = bad[:len(bad) - (5 if trial == VARIANTS - 1 else tail // 3)]
        else:
            for _ in range(1 + trial % 2):
                bad[int(rng.integers(len(bad) - tail, len(bad)))] ^= 1 << int(rng.integers(0, 8))
        out.append(bytes(bad))
    return out


_VERDICTS = {}


def verdicts(ref, name):
    """the reference on every variant of a row, in a child each (it may crash on damage): list of (code or "CRSH", sha256 of its pixels)"""
    if name not in _VERDICTS:
        out = []
        for bad in variants_of(name):
            code = decode_in_child(ref, bad)
            digest = ""
            if code == "":
                rerr, px = ref.decode(bad)
                assert rerr == ""
                digest = hashlib.sha256(px.tobytes()).hexdigest()
            out.append((code, digest))
        _VERDICTS[name] = out
    return _VERDICTS[name]


def comparable(code):
    return code not in ("CRSH", "TODO")


@pytest.mark.parametrize("family", FAMILIES)
def test_damaged_variants_end_like_in_the_reference(ref, sim, oracle, family):
    """the reference's code, or its pixels, from the device functions (either neighbour source) and from the restatement. A variant
    is left out only where the reference crashes or answers TODO: at most a quarter of the family's; at least one is accepted and at
    least three are rejected"""
    left_out = accepted = rejected = 0
    codes = {}
    for name in DAMAGED[family]:
        (w, h), _ = damaged_stream(name)
        for trial, (bad, (rcode, digest)) in enumerate(zip(variants_of(name), verdicts(ref, name))):
            codes[rcode] = codes.get(rcode, 0) + 1
            if not comparable(rcode):
                left_out += 1
                continue
            accepted += rcode == ""
            rejected += rcode != ""
            for flip in (0, 1):
                err, rgba = run_sim(sim, bad, w, h, flip)
                assert err == rcode, (name, trial, flip, err, rcode)
                if rcode == "":
                    assert hashlib.sha256(rgba.tobytes()).hexdigest() == digest, (name, trial, flip)
            err, rgba = run_oracle(oracle, bad, w, h)
            assert err == rcode, (name, trial, "restatement", err, rcode)
            if rcode == "":
                assert hashlib.sha256(rgba.tobytes()).hexdigest() == digest, (name, trial, "restatement")
    if family == "overflow":
        # what the aimed variants are aimed at (EXTRA_ROWS), from the reference alone: with the residual's extra bits cleared nothing
        # overflows and nothing else was touched; damage behind the overflow changes nothing, the reference stops at the overflow; a
        # stream that ends at two thirds of its last section ends ahead of the overflow (sample 20000 of 26400): a parse error, not "povf"
        for name in EXTRA_ROWS:
            got = [code for code, _ in verdicts(ref, name)]
            assert got[0] == "" and got[3] == "povf" and got[VARIANTS - 2] not in ("", "povf", "CRSH", "TODO"), (name, got)
    total = left_out + accepted + rejected
    print("%s: %d variants, %d accepted, %d rejected, %d left out; the reference's codes: %s" % (family, total, accepted, rejected, left_out, codes))
    assert 4 * left_out <= total and accepted >= 1 and rejected >= 3


# ---------------------------------------------------------------- the generator's refusals

REFUSALS = [
    (dict(lzmode="special"), "want lz77=1"),
    (dict(lz77=1, lzmode="fancy"), "lzmode=runs|special|plain|overlap"),
    (dict(lz77=1, lzforce="specials"), "zero predictor in one leaf (tree=4)"),
    (dict(lz77=1, lzforce="specials", tree=4, palette=1), "neither palette, squeeze nor local trees"),
    (dict(lz77=1, lzforce="specials", lzmode="plain", tree=4), "lzforce writes its own copies"),
    (dict(lz77=1, lzminsym=512), "wants prefix=1"),
    (dict(lz77=1, lzminsym=5), "lzminsym 224, 512, 4096 or 8 + u(15)"),
    (dict(lz77=1, lzminlen=2), "lzminlen 3..264"),
    (dict(lz77=1, lzlencfg="9,0,0"), "split_exp <= 8"),
    (dict(lz77=1, lzlencfg="4,2,0", lzforce="specials", tree=4, rct=-1), "beyond the alphabet of 256"),
    (dict(lz77=1, lzminsym=8, lzforce="specials", tree=4, rct=-1), "which min_symbol = 8 takes for a copy"),
    (dict(lz77=1, lzmode="special", repeat=2), "do not combine with repeat"),
    (dict(hybrid="8,1,0"), "leaves msb and lsb uncoded"),
    (dict(wp="1,2,3"), "wp=random|max|zero|"),
    (dict(wp="32,0,0,0,0,0,0,0,0,0,0", tree=2), "5-bit and w* 4-bit"),
    (dict(wpat="both"), "wpat places the parameters wp= gives"),
    (dict(wp="max", wpat="everywhere", tree=2), "wpat=global|group|both"),
    (dict(wp="max", squeeze=1), "does not combine with squeeze"),
    (dict(dpred=6), "belongs to a palette with delta entries"),
    (dict(palette=3, dpred=14), "dpred 0..13"),
    (dict(povf=5, povfto=100), "povfto lies outside int16"),
    (dict(povf=5, povfto=1 << 31), "povfto within +-2^30"),
    (dict(noise=70000), "noise 0..65535"),
    (dict(range="5,1"), "range=<lo>,<hi> within int16"),
    (dict(tile="0,4"), "tile=<px>,<py>"),
    (dict(range="-32768,32767", noise=40000), "modular sample out of int16 range"),     # (the RCT's forward half leaves int16: rct=-1 for such samples)
]


@pytest.mark.parametrize("opts,words", REFUSALS, ids=["_".join("%s-%s" % kv for kv in sorted(o.items())).replace(",", ".").replace("|", ".") for o, _ in REFUSALS])
def test_generator_says_why_it_refuses(built, tmp_path, opts, words):
    r = subprocess.run([SYNTH, "modular", "256", "256", "7", str(tmp_path / "x.jxl")] + ["%s=%s" % kv for kv in sorted(opts.items())], capture_output=True, text=True)
    assert r.returncode == 2 and words in r.stderr, r.stderr
    assert not (tmp_path / "x.jxl").exists()


VARDCT_REFUSALS = [
    (dict(hflzmode="plain"), "want hflz77=1"),
    (dict(hflz77=1, hflzmode="special"), "no distance multiplier and so no special distance codes"),
    (dict(hflz77=1, hflzminlen=2), "hflzminlen 3..264"),
    (dict(hflz77=1, hflzdistcfg="8,0,0"), "hflzdistcfg=<split_exp>,<msb>,<lsb> with split_exp < 8"),
    (dict(wp="max"), "unless the tree uses the weighted predictor: lftree=4"),
    (dict(lftree=4, wpat="both"), "wpat places the parameters wp= gives"),
    (dict(lftree=4, wp="max", wpat="both"), "want alpha=1"),
    (dict(lftree=4, wp="1,2"), "wp=random|max|zero|"),
    # jpegdata= (a JPEG file's integers, tests/test_jpeg_transcode.py) fixes everything else about the frame; the combinations are refused
    # before the dump is opened, a dump of another size than the command line's once it is
    (dict(jpegdata="missing.jpgd", forward=1), "forward=1 takes them from the picture"),
    (dict(jpegdata="missing.jpgd", passes=2), "jpegdata= writes one pass"),
    (dict(jpegdata="missing.jpgd", cfl=1), "jpegdata= and cfl=1 exclude each other"),
    (dict(jpegdata="missing.jpgd", maxlog=4), "jpegdata= fixes what maxlog= would say"),
    (dict(jpegdata="missing.jpgd", subsampling="420"), "jpegdata= fixes what subsampling= would say"),
    (dict(jpegdata="missing.jpgd"), "cannot be read"),
    (dict(jpegdata="8x8"), "holds a picture of 8 x 8, the command line says 520 x 264"),
]


@pytest.mark.parametrize("opts,words", VARDCT_REFUSALS, ids=["_".join("%s-%s" % kv for kv in sorted(o.items())).replace(",", ".") for o, _ in VARDCT_REFUSALS])
def test_generator_says_why_it_refuses_vardct_options(built, tmp_path, opts, words):
    if opts.get("jpegdata") == "8x8":   # a real dump: the 8 x 8 fixture's
        import jpeg_ref
        opts = dict(opts, jpegdata=jpeg_ref.dump_path(jpeg_ref.parse(jpeg_ref.fixture("q90_444_8x8")[0]), "q90_444_8x8"))
    r = subprocess.run([SYNTH, "vardct", "520", "264", "7", str(tmp_path / "x.jxl")] + ["%s=%s" % kv for kv in sorted(opts.items())], capture_output=True, text=True)
    assert r.returncode == 2 and words in r.stderr, r.stderr
    assert not (tmp_path / "x.jxl").exists()


def test_generator_refuses_group_parameters_without_groups(built, tmp_path):
    r = subprocess.run([SYNTH, "modular", "200", "200", "7", str(tmp_path / "x.jxl"), "tree=2", "wp=max", "wpat=group"], capture_output=True, text=True)
    assert r.returncode == 2 and "has no pass-group headers" in r.stderr, r.stderr


# ---------------------------------------------------------------- on the GPU

@pytest.fixture(scope="module")
def gpu(built):
    import j40_amd
    assert j40_amd.device_count() > 0, "the gpu tests need a HIP device"
    return j40_amd


@pytest.mark.gpu
@pytest.mark.parametrize("name", IDS)
def test_public_api_matches_reference(gpu, ref, name):
    """j40_amd.decode, kernels as shipped: the reference's pixels or its code; rows deeper than 8 bits through the 16-bit output as
    well, against the reference's int16 planes (tests/test_u16_output.py's rule)"""
    _, _, _, opts, _ = ROW[name]
    data = stream(name)
    rerr, expect = reference(ref, name)
    err, rgba = gpu.decode(data)
    assert err == rerr, (err, rerr)
    if rerr != "":
        assert gpu.decode(data, gpu.J40_U16X4)[0] == rerr
        return
    assert np.array_equal(rgba, expect), int((rgba != expect).sum())
    if opts.get("bpp", 8) > 8 or "range" in opts:
        from test_u16_output import ref_planes, scale_u16
        err, px = gpu.decode(data, gpu.J40_U16X4)
        assert err == "" and px.dtype == np.uint16
        bpp, rgb, alpha = ref_planes(ref, data)
        assert np.array_equal(px[..., :3], scale_u16(rgb, bpp))
        assert np.array_equal(px[..., 3], scale_u16(alpha, bpp) if alpha is not None else np.full(px.shape[:2], 65535, np.uint16))


CHILD = r"""
import sys, hashlib
sys.path.insert(0, %r); sys.path.insert(0, %r)
import j40_amd
import test_modular_stress as T
from streams import synth, MODULAR_STRESS_SQUEEZE, STRESS_SEED
out = {}
for name in T.IDS:
    err, rgba = j40_amd.decode(T.stream(name))
    out[name] = (err, hashlib.sha256(rgba.tobytes()).hexdigest() if err == "" else "")
for name, (w, h), opts in MODULAR_STRESS_SQUEEZE:
    err, rgba = j40_amd.decode(synth("modular", w, h, STRESS_SEED, **opts))
    out[name] = (err, hashlib.sha256(rgba.tobytes()).hexdigest() if err == "" else "")
for name, trials in %r:
    bad = T.variants_of(name)
    for trial in trials:
        err, rgba = j40_amd.decode(bad[trial])
        out[name, trial] = (err, hashlib.sha256(rgba.tobytes()).hexdigest() if err == "" else "")
j40_amd.shutdown()
print(repr(out))
"""

_CHILD_ENDED_BADLY = []     # a child that faulted, aborted or ran out of time: nothing more is started on that card


SWITCHES = [{}, {"J40HIP_NO_SPLIT": "1"}, {"J40HIP_SPLIT_NO_FAST": "1"}, {"J40HIP_NO_COOP": "1"}, {"J40HIP_QUAD_MIN": "1"}]


@pytest.mark.gpu
@pytest.mark.parametrize("switch", SWITCHES, ids=["as_shipped", "no_split", "split_no_fast", "no_coop", "quad_min_1"])
def test_every_kernel_gives_the_reference_s_answer(gpu, ref, switch):
    """the whole matrix and every comparable damaged variant through the public API in ONE child process per switch: the two-pass
    decoder with and without its sixty-four-at-a-time mode, the general kernel in its place, the cooperative kernel off, and four
    sections per wavefront wherever k_modular_quad can take them. Every answer is the reference's: code, or sha256 of the pixels"""
    expect, jobs = {}, []
    for name in IDS:
        rerr, px = reference(ref, name)
        expect[name] = (rerr, hashlib.sha256(px.tobytes()).hexdigest() if rerr == "" else "")
    for name, _, _ in MODULAR_STRESS_SQUEEZE:
        expect[name] = ("", hashlib.sha256(squeeze_row(ref, name)[1].tobytes()).hexdigest())
    for family in FAMILIES:
        for name in DAMAGED[family]:
            trials = [t for t, (code, _) in enumerate(verdicts(ref, name)) if comparable(code)]
            jobs.append((name, trials))
            for t in trials:
                expect[name, t] = verdicts(ref, name)[t]
    script = CHILD % (ROOT, os.path.join(ROOT, "tests"), jobs)
    assert not _CHILD_ENDED_BADLY, "an earlier child ended badly (%s): no further child is started" % _CHILD_ENDED_BADLY[0]
    try:
        r = subprocess.run([sys.executable, "-c", script], env=dict(os.environ, **switch), capture_output=True, text=True, timeout=900)
    except subprocess.TimeoutExpired:
        _CHILD_ENDED_BADLY.append("%s: time limit" % (switch or "as shipped"))
        raise
    if r.returncode != 0:
        _CHILD_ENDED_BADLY.append("%s: exit status %d" % (switch or "as shipped", r.returncode))
    assert r.returncode == 0, r.stderr[-3000:]
    got = eval(r.stdout.strip().splitlines()[-1])
    assert set(got) == set(expect)
    wrong = {k: (got[k], expect[k]) for k in expect if got[k] != expect[k]}
    assert not wrong, "%d of %d answers differ from the reference's: %s" % (len(wrong), len(expect), list(wrong.items())[:6])
