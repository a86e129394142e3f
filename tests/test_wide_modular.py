"""Wide Modular frames: images whose metadata says modular_16bit_buffers = 0 -- every 16-bit lossless image -- decoded with int32
sample planes (J40HIP_PARSE_WIDE / J40HIP_WIDE=1, include/j40hip.h). The reference refuses every such image with "fm32"
(j40.h:3169) and its 32-bit channel decoder still tests the int16 range (j40.h:4225), so it cannot be the oracle: PARITY UNPINNED.
What pins the path here, every comparison exact:

  * without the switch nothing changes: "fm32", as in the reference;
  * narrow equals wide: the generator's wide=1 flips that one metadata bit and nothing else, so at 8, 12 and 15 bits the wide decode
    of a picture must equal the REFERENCE's decode of its narrow twin (u8) and the narrow path's u16 -- which pins the int32
    instantiation to the reference wherever values fit 16 bits;
  * lossless round trip at 16 bits: the decode equals the generator's source samples (dumpsrc=), whose maximum exceeds 40000 and
    whose coded planes leave int16 -- a path that truncates anywhere cannot pass;
  * samples at the ends of int32's upper half round-trip, a sample beyond int32 is "povf";
  * the plan's memory (ModPlanLayout) with guard bytes behind every region comes back untouched;
  * three streams through the stand-alone program, plain and under the host sanitizers.

The CPU tests run the device functions compiled for the host (tests/hostsim/wide_sim.cpp); the GPU tests run the HIP kernels."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from streams import synth, ROOT, SYNTH, CACHE

SEED = 7
PARSE_WIDE = 8
U8, U16 = 0, 1   # wide_sim.cpp's output formats

# (name, width, height, generator options): the smallest shapes that still reach every branch (tests/test_squeeze.py,
# tests/test_modular_stress.py): one group / several, global and per-section trees, every predictor family, previous-channel
# properties, prefix codes + LZ77, RCT and palette global and per section, Squeeze, two passes
CASES = [
    ("one_group", 200, 150, dict()),
    ("one_group_alpha_property_tree", 200, 150, dict(alpha=1, tree=1)),
    ("six_groups_weighted_predictor", 600, 300, dict(tree=2)),
    ("odd_size_ycocg_weighted_predictor", 601, 299, dict(rct=6, tree=2)),     # 18-bit intermediates through the weighted predictor
    ("groups_of_128_prefix_lz77", 520, 520, dict(groupshift=7, prefix=1, lz77=1)),
    ("palette", 300, 200, dict(palette=1)),
    ("palette_predicted_deltas", 300, 200, dict(palette=3)),
    ("local_rct", 300, 200, dict(localrct=4)),
    ("local_palette", 300, 200, dict(localpalette=1)),
    ("local_tree", 300, 200, dict(localtree=1)),
    ("squeeze", 600, 300, dict(squeeze=1)),
    ("squeeze_explicit_list_alpha", 601, 299, dict(squeeze=3, alpha=1)),
    ("two_passes", 600, 300, dict(passes=2, tree=1)),
    ("previous_channel_properties_alpha", 600, 300, dict(tree=3, alpha=1)),
]
IDS = [c[0] for c in CASES]


def err4(code):
    return "".join(chr((code >> s) & 0xff) for s in (24, 16, 8, 0)) if code else ""


def synth_src(w, h, seed, **opts):
    """(stream, source samples int32 [channels, h, w]) of a Modular stream written with dumpsrc= (cached like streams.synth's)"""
    os.makedirs(CACHE, exist_ok=True)
    key = "modular_%d_%d_%d_%s" % (w, h, seed, "_".join("%s-%s" % kv for kv in sorted(opts.items())))
    path, src = os.path.join(CACHE, key + ".src.jxl"), os.path.join(CACHE, key + ".src.i32")
    if not (os.path.exists(path) and os.path.exists(src)):
        tmp = path + ".tmp%d" % os.getpid()
        subprocess.run([SYNTH, "modular", str(w), str(h), str(seed), tmp] + ["%s=%s" % kv for kv in sorted(opts.items())] + ["dumpsrc=" + src + ".tmp%d" % os.getpid()],
                       check=True, stderr=subprocess.DEVNULL)
        os.replace(src + ".tmp%d" % os.getpid(), src)
        os.replace(tmp, path)
    with open(path, "rb") as fp:
        data = fp.read()
    return data, np.fromfile(src, np.int32).reshape(-1, h, w)


def level_to_u16(p, bpp):
    """INTEGRATION.md's rule on clamped levels; at 16 bits the level itself"""
    maxpixel = (1 << bpp) - 1
    return ((np.clip(p, 0, maxpixel).astype(np.int64) * 65535 + (1 << (bpp - 1))) // maxpixel).astype(np.uint16)


def level_to_u8(p, bpp):
    maxpixel = (1 << bpp) - 1
    return ((np.clip(p, 0, maxpixel).astype(np.int64) * 255 + (1 << (bpp - 1))) // maxpixel).astype(np.uint8)


def expected_pixels(src, bpp, fmt):
    """RGBA of the source samples: colour channels 0..2, the last extra channel as alpha where there is one, else opaque"""
    conv = level_to_u16 if fmt == U16 else level_to_u8
    h, w = src.shape[1:]
    out = np.zeros((h, w, 4), np.uint16 if fmt == U16 else np.uint8)
    for c in range(3):
        out[..., c] = conv(src[c], bpp)
    out[..., 3] = conv(src[-1], bpp) if src.shape[0] > 3 else (65535 if fmt == U16 else 255)
    return out


class Sim:
    """build/libwidesim.so: the Modular device functions on the CPU, int32 samples for wide frames, int16 for narrow ones"""

    def __init__(self):
        L = self.L = C.CDLL(os.path.join(ROOT, "build", "libwidesim.so"))
        L.widesim_decode.restype = C.c_uint32
        L.widesim_decode.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_int, C.c_uint32]
        L.widesim_parse.restype = C.c_uint32
        L.widesim_parse.argtypes = [C.c_void_p, C.c_size_t, C.c_uint32, C.c_void_p]
        L.widesim_final_plane.restype = C.c_int64
        L.widesim_final_plane.argtypes = [C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
        L.widesim_guard_damage.restype = C.c_int64
        L.widesim_region_bytes.restype = C.c_int64
        L.widesim_region_bytes.argtypes = [C.c_char_p]
        L.widesim_plan_counts.restype = C.c_uint32
        L.widesim_plan_counts.argtypes = [C.c_void_p, C.c_size_t, C.c_uint32, C.c_void_p]
        L.widesim_coded_range.argtypes = [C.c_void_p]

    def decode(self, data, w, h, fmt, flags=PARSE_WIDE):
        """(code, pixels); every decode must leave the guard bytes of its plan's memory alone (the layout, test 6)"""
        out = np.zeros((h, w, 4), np.uint16 if fmt == U16 else np.uint8)
        code = self.L.widesim_decode(data, len(data), out.ctypes.data, fmt, flags)
        assert self.L.widesim_guard_damage() == 0, "a region of the plan's memory was written past its end"
        return err4(code), out

    def planes(self, n, w, h):
        out = np.zeros((n, h, w), np.int32)
        for c in range(n):
            assert self.L.widesim_final_plane(c, out[c].ctypes.data, None, None) == w * h
        return out

    def coded_range(self):
        a = np.zeros(2, np.int64)
        self.L.widesim_coded_range(a.ctypes.data)
        return int(a[0]), int(a[1])

    def plan(self, data, flags=PARSE_WIDE):
        a = np.zeros(5, np.int32)
        code = self.L.widesim_plan_counts(data, len(data), flags, a.ctypes.data)
        return err4(code), dict(sections=int(a[0]), coop=int(a[1]), quad=int(a[2]), split=int(a[3]), sample_bytes=int(a[4]))


@pytest.fixture(scope="module")
def sim(built):
    return Sim()


# ---------------------------------------------------------------- 1. nothing changes without the switch

def test_default_is_fm32_and_the_switch_serves_modular_frames_only(built, ref, sim):
    import j40_amd
    data = synth("modular", 200, 150, SEED, bpp=16, wide=1)
    with pytest.raises(j40_amd.J40Error) as e:
        j40_amd.Frame(data)
    assert e.value.code == "fm32"
    assert ref.decode(data)[0] == "fm32", "the reference refuses every image with 32-bit buffers (j40.h:3169)"
    assert err4(sim.L.widesim_parse(data, len(data), 0, None)) == "fm32"
    fr = j40_amd.Frame(data, wide=True)
    assert fr.wide() == dict(wide=1, bpp=16, used=0, sample_bytes=0)
    fr.close()
    twelve = synth("modular", 200, 150, SEED, bpp=12, wide=1)
    with pytest.raises(j40_amd.J40Error) as e:
        j40_amd.Frame(twelve)
    assert e.value.code == "fm32"
    # a narrow image says so, with or without the switch
    fr = j40_amd.Frame(synth("modular", 200, 150, SEED, bpp=12), wide=True)
    assert fr.wide()["wide"] == 0 and fr.wide()["bpp"] == 12
    fr.close()
    # a VarDCT frame of such an image: "fm32" without the switch, "TODO" with it
    vardct = synth("vardct", 520, 264, SEED, bpp=12, wide=1)
    assert ref.decode(vardct)[0] == "fm32"
    for flag, want in ((False, "fm32"), (True, "TODO")):
        with pytest.raises(j40_amd.J40Error) as e:
            j40_amd.Frame(vardct, wide=flag)
        assert e.value.code == want
    # sequences take the flag too
    seq = synth("modular", 200, 150, SEED, bpp=16, wide=1, frames=2, anim=1, durations="1,1")
    with pytest.raises(j40_amd.J40Error) as e:
        j40_amd.Sequence(seq)
    assert e.value.code == "fm32"
    s = j40_amd.Sequence(seq, wide=True)
    assert s.num_frames == 2
    s.close()


def test_environment_switch_in_a_fresh_process(built):
    """J40HIP_WIDE=1 serves parses that pass no flag (it is read once per process)"""
    data_path = os.path.join(CACHE, "wide_env_probe.jxl")
    with open(data_path, "wb") as fp:
        fp.write(synth("modular", 200, 150, SEED, bpp=16, wide=1))
    prog = ("import sys; sys.path.insert(0, %r)\nimport j40_amd\nd = open(%r, 'rb').read()\n"
            "try:\n    f = j40_amd.Frame(d); print('ok', f.wide()['wide']); f.close()\nexcept j40_amd.J40Error as e:\n    print('err', e.code)\n") % (ROOT, data_path)
    for env, want in ((dict(J40HIP_WIDE="1"), "ok 1"), (dict(J40HIP_WIDE="0"), "err fm32")):
        r = subprocess.run([sys.executable, "-c", prog], env=dict(os.environ, **env), capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and r.stdout.strip() == want, (r.stdout, r.stderr[-1000:])


def test_generator_wide_changes_one_bit(built):
    """wide=1 at a depth the narrow form has: the same picture, the same sections -- the files differ in the metadata bit alone (what
    follows it keeps its bit positions: the bit is written either way)"""
    for w, h, opts in ((200, 150, dict(bpp=12)), (600, 300, dict(bpp=15, tree=2)), (300, 200, dict(bpp=8, alpha=1, palette=3))):
        narrow, nsrc = synth_src(w, h, SEED, **opts)
        wide, wsrc = synth_src(w, h, SEED, wide=1, **opts)
        assert np.array_equal(nsrc, wsrc)
        assert len(narrow) == len(wide)
        diff = np.nonzero(np.frombuffer(narrow, np.uint8) != np.frombuffer(wide, np.uint8))[0]
        assert len(diff) == 1 and bin(narrow[diff[0]] ^ wide[diff[0]]).count("1") == 1 and diff[0] < 16
    for args in (["bpp=16"], ["bpp=12", "alpha=1"], ["range=0,40000"], ["bias=5"]):
        r = subprocess.run([SYNTH, "modular", "64", "64", "1", os.path.join(CACHE, "never.jxl")] + args, capture_output=True)
        assert r.returncode != 0, "without wide=1 the tool refuses %r" % args


# ---------------------------------------------------------------- 2. narrow equals wide

def narrow_twin(opts):
    """the options of the narrow stream the reference decodes to the same colour picture: no Squeeze (the reference stops there with
    "TODO", tests/test_squeeze.py: the picture without it is what it pins), and above 8 bits no alpha (the narrow generator writes
    the default 8-bit alpha only, which the reference refuses beside deeper colour; the colour samples do not depend on it)"""
    return {k: v for k, v in opts.items() if k != "squeeze" and not (k == "alpha" and opts.get("bpp", 8) != 8)}


def comparable(planes):
    """Narrow and wide can only agree where the wide samples fit int16: the number of leading pixels (raster order) before the first
    sample that does not. Every row below is chosen so that this is the whole picture (fits_narrow)"""
    misfit = ((planes > 32767) | (planes < -32768)).any(0).ravel()
    return int(np.argmax(misfit)) if misfit.any() else misfit.size


def fits_narrow(o):
    """The option set with its samples bounded where the narrow path would otherwise wrap -- the reference's int16 arithmetic wraps
    there and int32 does not, so the two would differ by design. 12-bit palettes: an implicit colour is k * 4095 / 4 + 512 for
    k = index - nb_colours < 64, beyond int16 from k = 32 on; the generator's index is v * 40 >> 8, so samples up to 460 keep
    k below 32 (implicit colours still occur). 15-bit pictures under localrct=: most of its RCT types take the picture as already
    transformed, and two chained inverses on top of the global one sum up to eight samples: samples up to 4000 stay inside int16"""
    if "palette" in o and o["bpp"] == 12:
        return dict(o, range="0,460")
    if "localrct" in o and o["bpp"] == 15:
        return dict(o, range="0,4000")
    return o


@pytest.mark.parametrize("bpp", [8, 12, 15])
@pytest.mark.parametrize("name,w,h,opts", CASES, ids=IDS)
def test_narrow_equals_wide(built, ref, sim, name, w, h, opts, bpp):
    o = fits_narrow(dict(opts, bpp=bpp))
    wide, src = synth_src(w, h, SEED, wide=1, **o)
    narrow = synth("modular", w, h, SEED, **narrow_twin(o))
    rerr, want = ref.decode(narrow)
    assert rerr == "", "the narrow twin is what the reference pins"
    assert ref.decode(wide)[0] == "fm32"
    err, got8 = sim.decode(wide, w, h, U8)
    assert err == "" and sim.L.widesim_sample_bytes() == 4
    planes = sim.planes(3, w, h)
    n = comparable(planes)
    assert n == w * h, "%d leading pixels comparable: the row must be chosen so that nothing leaves int16" % n
    assert np.array_equal(got8.reshape(-1, 4)[:n, :3], want.reshape(-1, 4)[:n, :3]), "u8 against the reference's decode of the narrow twin"
    if "alpha" in narrow_twin(o) or "alpha" not in o:
        assert np.array_equal(got8.reshape(-1, 4)[:n, 3], want.reshape(-1, 4)[:n, 3])
    else:
        assert np.array_equal(got8[..., 3], level_to_u8(src[-1], bpp)), "the deep alpha channel against the source"
    # u16: the narrow path through the same orchestration (int16 instantiation), whose planes the existing tests pin
    err, got16 = sim.decode(wide, w, h, U16)
    assert err == ""
    nerr, narrow16 = sim.decode(narrow, w, h, U16, flags=0)
    assert nerr == "" and sim.L.widesim_sample_bytes() == 2
    assert np.array_equal(got16.reshape(-1, 4)[:n, :3], narrow16.reshape(-1, 4)[:n, :3])
    assert np.array_equal(got16.reshape(-1, 4)[:n, :3], level_to_u16(planes, bpp).transpose(1, 2, 0).reshape(-1, 3)[:n])
    if n == w * h:
        assert np.array_equal(got16, expected_pixels(src, bpp, U16)), "and the source samples"


def narrow_16_bit_stream(w, h, **opts):
    """a 16-bit image with 16-BIT buffers (the reference takes it: samples up to 32767): the wide=1 stream with the metadata bit set
    back. The bit's place is where the 15-bit narrow and wide twins differ (15 and 16 bits are written with the same field widths)"""
    n15, w15 = synth("modular", w, h, SEED, bpp=15, **opts), synth("modular", w, h, SEED, bpp=15, wide=1, **opts)
    at = np.nonzero(np.frombuffer(n15, np.uint8) != np.frombuffer(w15, np.uint8))[0]
    assert len(at) == 1
    data = bytearray(synth("modular", w, h, SEED, bpp=16, wide=1, range="0,32767", **opts))
    data[at[0]] |= n15[at[0]] ^ w15[at[0]]
    return bytes(data)


@pytest.mark.parametrize("opts", [dict(rct=-1, tree=1), dict(tree=2), dict(groupshift=7, prefix=1, lz77=1)], ids=["property_tree", "weighted_predictor", "groups_of_128_prefix_lz77"])
def test_narrow_16_bit_image_is_unchanged(built, ref, sim, opts):
    """existing behaviour: a 16-bit image in 16-bit buffers decodes through the int16 path to the reference's pixels, opaque where it
    has no alpha plane (maxpixel = 65535 does not fit the sample type: the pack kernels' `opaque` must not take it)"""
    w, h = 300, 200
    data = narrow_16_bit_stream(w, h, **opts)
    rerr, want = ref.decode(data)
    assert rerr == "" and (want[..., 3] == 255).all()
    err, got = sim.decode(data, w, h, U8, flags=0)
    assert err == "" and sim.L.widesim_sample_bytes() == 2 and np.array_equal(got, want)


# ---------------------------------------------------------------- 3. the 16-bit round trip (fails without the feature: no such stream, no such parse)

@pytest.mark.parametrize("name,w,h,opts", CASES, ids=IDS)
def test_16_bit_round_trip(built, sim, name, w, h, opts):
    data, src = synth_src(w, h, SEED, bpp=16, wide=1, **opts)
    assert src[:3].max() > 40000, "the picture must span more than int16"
    err, got16 = sim.decode(data, w, h, U16)
    assert err == "" and sim.L.widesim_sample_bytes() == 4
    lo, hi = sim.coded_range()
    planes = sim.planes(src.shape[0], w, h)
    # a plane a truncating path would damage: the coded planes before the inverse RCT -- or, where a palette stands in for the colour
    # channels (indices and entries are small), the planes behind the look-up
    if "palette" in opts:
        assert planes.max() > 32767
    else:
        assert hi > 32767 or lo < -32768, "coded samples %d .. %d" % (lo, hi)
    assert np.array_equal(planes, src), "the planes are the source samples"
    assert np.array_equal(got16, expected_pixels(src, 16, U16)), "at 16 bits the u16 value is the level; A = 65535 without an alpha channel"
    err, got8 = sim.decode(data, w, h, U8)
    assert err == ""
    assert np.array_equal(got8, ((got16.astype(np.int64) * 255 + 32768) // 65535).astype(np.uint8))
    assert np.array_equal(got8, expected_pixels(src, 16, U8))
    if "alpha" not in opts:
        assert (got16[..., 3] == 65535).all() and (got8[..., 3] == 255).all()


def test_both_neighbour_sources(built, sim):
    """decode_modular_section reads neighbours from the row ring or back from the plane: a frame of one section sees both"""
    data, src = synth_src(200, 150, SEED, bpp=16, wide=1, tree=2)
    outs = []
    for flip in (0, 1):
        sim.L.widesim_set_neighbour_flip(flip)
        outs.append(sim.decode(data, 200, 150, U16))
    sim.L.widesim_set_neighbour_flip(0)
    assert outs[0][0] == "" and outs[1][0] == "" and np.array_equal(outs[0][1], outs[1][1]) and np.array_equal(outs[0][1], expected_pixels(src, 16, U16))


# ---------------------------------------------------------------- 5. the sample range is int32

FAR = dict(bpp=16, wide=1, rct=-1, range="-1073741824,1073741823")


@pytest.mark.parametrize("opts", [dict(FAR, bias=1073676288, tree=8), dict(FAR, bias=-1073741824, tree=8), dict(FAR, bias=1073676288, tree=8, groupshift=7)],
                         ids=["plus_2_30", "minus_2_30", "plus_2_30_groups_of_128"])
def test_samples_near_2_30_round_trip(built, sim, opts):
    """read the planes, not the pixels: every sample is clamped to 0 or 65535 on its way out"""
    w, h = 200, 150
    data, src = synth_src(w, h, SEED, **opts)
    assert abs(int(src.astype(np.int64).min())) >= (1 << 30) - 65536 or int(src.max()) >= (1 << 30) - 65536
    err, px = sim.decode(data, w, h, U16)
    assert err == ""
    assert np.array_equal(sim.planes(3, w, h), src)
    assert np.array_equal(px, expected_pixels(src, 16, U16))


@pytest.mark.parametrize("opts", [dict(FAR, bias=1073676288, tree=7, povf=100), dict(FAR, bias=-1073741824, tree=7, povf=5000, povfto=-2147483649, groupshift=7),
                                  dict(FAR, bias=1073676288, tree=7, povf=0, povfto=4294967296)], ids=["above", "below_in_a_group", "first_sample_2_32"])
def test_sample_beyond_int32_is_povf(built, sim, opts):
    data = synth("modular", 200, 150, SEED, **opts)
    assert sim.decode(data, 200, 150, U8)[0] == "povf"


def test_sample_beyond_int16_is_not_povf_in_a_wide_frame(built, sim):
    """the departure from j40.h:4225: the narrow path's overflow streams, flagged wide, decode"""
    data = synth("modular", 300, 200, SEED, rct=-1, noise=40000, range="-70000,70000", tree=4, wide=1)
    narrow_err = sim.decode(synth("modular", 300, 200, SEED, povf=5000), 300, 200, U8, flags=0)[0]
    assert narrow_err == "povf"
    err, _ = sim.decode(data, 300, 200, U8)
    lo, hi = sim.coded_range()
    assert err == "" and lo < -32768 and hi > 32767


# ---------------------------------------------------------------- 6. the layout

def test_layout_regions_take_the_sample_size(built, sim):
    """ModPlanLayout: planes and sub-planes of a wide plan are int32, the weighted predictor's scratch cells int64; every decode in
    this file also checks the guard bytes behind every region (Sim.decode)"""
    for w, h, opts in ((600, 300, dict(tree=2)), (300, 200, dict(localpalette=1)), (600, 300, dict(squeeze=1, tree=2))):
        sizes = []
        for wide in (0, 1):
            data = synth("modular", w, h, SEED, bpp=12, **(dict(opts, wide=1) if wide else opts))
            assert sim.decode(data, w, h, U8, flags=PARSE_WIDE if wide else 0)[0] == ""
            sizes.append({k: sim.L.widesim_region_bytes(k.encode()) for k in ("plane", "sub_plane", "wp_scratch", "status", "tree", "sections")})
        n, wd = sizes
        assert n["plane"] > 0 and wd["plane"] == 2 * n["plane"] and wd["sub_plane"] == 2 * n["sub_plane"] and wd["wp_scratch"] == 2 * n["wp_scratch"]
        assert ("tree" not in opts or opts["tree"] != 2) or n["wp_scratch"] > 0
        assert all(wd[k] == n[k] for k in ("status", "tree", "sections"))


def test_wide_sections_never_go_to_the_int16_only_kernels(built):
    """assign_coop's quad step and the split assignment never pick a section of a wide frame, also under J40HIP_QUAD_MIN=1 (read once
    per process: a child); the cooperative kernel keeps them. The narrow twins show that the streams are the kind those kernels take"""
    paths = []
    for k, (w, h, opts) in enumerate(((600, 300, dict(tree=1)), (600, 300, dict()))):
        for wide in (0, 1):
            p = os.path.join(CACHE, "wide_plan_probe_%d_%d.jxl" % (k, wide))
            with open(p, "wb") as fp:
                fp.write(synth("modular", w, h, SEED, bpp=12, **(dict(opts, wide=1) if wide else opts)))
            paths.append(p)
    prog = ("import sys, os; sys.path.insert(0, os.path.join(%r, 'tests')); sys.path.insert(0, %r)\nfrom test_wide_modular import Sim\ns = Sim()\n"
            "for p in %r:\n    print(s.plan(open(p, 'rb').read()))\n") % (ROOT, ROOT, paths)
    r = subprocess.run([sys.executable, "-c", prog], env=dict(os.environ, J40HIP_QUAD_MIN="1"), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    rows = [eval(line) for line in r.stdout.strip().splitlines()]
    assert all(e == "" for e, _ in rows)
    (n1, w1, n0, w0) = [p for _, p in rows]
    assert n1["quad"] > 0 and n1["sample_bytes"] == 2, n1          # property tree: cooperative, then four to a wavefront
    assert n0["split"] > 0, n0                                     # one gradient leaf: the two-pass decoder
    for wd in (w1, w0):
        assert wd["sample_bytes"] == 4 and wd["quad"] == 0 and wd["split"] == 0 and wd["coop"] == wd["sections"] > 0, wd


# ---------------------------------------------------------------- 7. the stand-alone program, plain and under the host sanitizers

@pytest.mark.parametrize("program", ["wide_main", "wide_main_san"])
def test_stand_alone_program_plain_and_sanitised(built, program):
    """an executable of its own, never loaded into Python: the 18-bit weighted predictor, a predicted palette, Squeeze with alpha"""
    paths = []
    for k, (w, h, opts) in enumerate(((601, 299, dict(rct=6, tree=2)), (300, 200, dict(palette=3)), (601, 299, dict(squeeze=3, alpha=1)))):
        p = os.path.join(CACHE, "wide_main_%d.jxl" % k)
        with open(p, "wb") as fp:
            fp.write(synth("modular", w, h, SEED, bpp=16, wide=1, **opts))
        paths.append(p)
    r = subprocess.run([os.path.join(ROOT, "build", program)] + paths, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 6 and all("4 bytes a sample" in ln and "code 00000000" in ln and " 0 guard bytes damaged" in ln for ln in lines), r.stdout
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]


# ---------------------------------------------------------------- on the GPU

@pytest.fixture(scope="module")
def gpu(built):
    import j40_amd
    assert j40_amd.device_count() > 0, "the gpu tests need a HIP device"
    return j40_amd


def gpu_decode(gpu, data, fmt, **how):
    """through the thin C-ABI with the getter's word on the decode: (pixels, Frame.wide())"""
    fr = gpu.Frame(data, wide=True)
    try:
        fr.set_output_format(gpu.J40_U16X4 if fmt == U16 else gpu.J40_U8X4)
        fr.upload(0)
        err, px = fr.decode_to_host()
        assert err == "", err
        counts = (fr.coop_sections(), fr.quad_sections(), fr.split_sections())
        return px, fr.wide(), counts
    finally:
        fr.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name,w,h,opts", CASES, ids=IDS)
def test_gpu_16_bit_round_trip(gpu, name, w, h, opts):
    data, src = synth_src(w, h, SEED, bpp=16, wide=1, **opts)
    for fmt in (U16, U8):
        px, said, counts = gpu_decode(gpu, data, fmt)
        assert said == dict(wide=1, bpp=16, used=1, sample_bytes=4)
        assert counts[1] == 0 and counts[2] == 0, "no section of a wide frame goes to k_modular_quad or the two-pass decoder"
        assert np.array_equal(px, expected_pixels(src, 16, fmt))
    err, px = gpu.decode(data, gpu.J40_U16X4, wide=True)
    assert err == "" and np.array_equal(px, expected_pixels(src, 16, U16))
    assert gpu.decode(data, gpu.J40_U16X4)[0] == "fm32", "the public API without the switch"


@pytest.mark.gpu
@pytest.mark.parametrize("bpp", [8, 12, 15])
@pytest.mark.parametrize("name,w,h,opts", CASES, ids=IDS)
def test_gpu_narrow_equals_wide(gpu, ref, name, w, h, opts, bpp):
    o = fits_narrow(dict(opts, bpp=bpp))
    wide, src = synth_src(w, h, SEED, wide=1, **o)
    narrow = synth("modular", w, h, SEED, **narrow_twin(o))
    rerr, want = ref.decode(narrow)
    assert rerr == ""
    fr = gpu.Frame(wide, wide=True)
    try:
        fr.upload(0)
        err, got8 = fr.decode_to_host()
        assert err == "" and fr.wide()["used"] == 1 and fr.wide()["sample_bytes"] == 4
        planes = np.stack([fr.read_plane_i32(c, (h, w)) for c in range(3)])
    finally:
        fr.close()
    n = comparable(planes)
    assert n == w * h
    assert np.array_equal(got8.reshape(-1, 4)[:n, :3], want.reshape(-1, 4)[:n, :3])
    nerr, narrow16 = gpu.decode(narrow, gpu.J40_U16X4)
    err, got16 = gpu.decode(wide, gpu.J40_U16X4, wide=True)
    assert nerr == "" and err == ""
    assert np.array_equal(got16.reshape(-1, 4)[:n, :3], narrow16.reshape(-1, 4)[:n, :3])
    if n == w * h:
        assert np.array_equal(got16, expected_pixels(src, bpp, U16))


def child(code, env_extra, timeout=600):
    env = dict(os.environ, **env_extra)
    prog = "import sys, os\nsys.path.insert(0, %r); sys.path.insert(0, os.path.join(%r, 'tests'))\n" % (ROOT, ROOT) + code
    r = subprocess.run([sys.executable, "-c", prog], env=env, timeout=timeout, capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    return r.stdout


@pytest.mark.gpu
@pytest.mark.parametrize("opts", [dict(rct=-1, tree=1), dict(tree=2), dict(groupshift=7, prefix=1, lz77=1)], ids=["property_tree", "weighted_predictor", "groups_of_128_prefix_lz77"])
def test_gpu_narrow_16_bit_image_is_unchanged(gpu, ref, opts):
    """the int16 pack kernels at bpp = 16: A = 255 / 65535 without an alpha plane, as the reference renders it (j40.h:7950); region
    (the _rect kernels) and scale (the K > 0 forms) too"""
    from test_scale import box
    w, h = 300, 200
    data = narrow_16_bit_stream(w, h, **opts)
    rerr, want = ref.decode(data)
    assert rerr == ""
    err, got = gpu.decode(data)
    assert err == "" and np.array_equal(got, want)
    err, got16 = gpu.decode(data, gpu.J40_U16X4)
    assert err == "" and np.array_equal(((got16.astype(np.int64) * 255 + 32768) // 65535).astype(np.uint8), want)
    assert (got16[..., 3] == 65535).all()
    err, part = gpu.decode_region(data, 31, 17, 260, 150)
    assert err == "" and np.array_equal(part, want[17:167, 31:291])
    err, small = gpu.decode(data, scale=1)
    assert err == "" and np.array_equal(small, box(want, 1))


@pytest.mark.gpu
def test_gpu_cooperative_kernel_takes_wide_sections(gpu):
    """a property tree without the weighted predictor, rANS: k_modular_coop's; with J40HIP_NO_COOP=1 (a fresh process) the generic
    kernel decodes the same pixels; under J40HIP_QUAD_MIN=1 no section turns to the int16-only kernels"""
    w, h = 600, 300
    data, src = synth_src(w, h, SEED, bpp=16, wide=1, tree=1)
    px, said, counts = gpu_decode(gpu, data, U16)
    assert counts[0][0] == counts[0][1] > 0 and counts[1] == 0 and counts[2] == 0, counts
    assert np.array_equal(px, expected_pixels(src, 16, U16))
    path, out = os.path.join(CACHE, "wide_coop_probe.jxl"), os.path.join(ROOT, "build", "wide_coop_probe_%s.npy")
    with open(path, "wb") as fp:
        fp.write(data)
    code = """
import numpy as np, j40_amd
fr = j40_amd.Frame(open(%r, 'rb').read(), wide=True)
fr.set_output_format(j40_amd.J40_U16X4); fr.upload(0)
err, px = fr.decode_to_host()
assert err == '', err
print(fr.coop_sections()[0], fr.quad_sections(), fr.split_sections(), fr.wide()['used'])
np.save(%r %% TAG, px)
"""
    said = child(code.replace("TAG", "'nocoop'") % (path, out), dict(J40HIP_NO_COOP="1")).split()
    assert said == ["0", "0", "0", "1"], said
    assert np.array_equal(np.load(out % "nocoop"), px)
    said = child(code.replace("TAG", "'quadmin'") % (path, out), dict(J40HIP_QUAD_MIN="1")).split()
    assert int(said[0]) > 0 and said[1:] == ["0", "0", "1"], said
    assert np.array_equal(np.load(out % "quadmin"), px)


@pytest.mark.gpu
def test_gpu_four_lf_groups_squeeze(gpu):
    """2600 x 2100: 2 x 2 LfGroups, the channels shifted by 3 or more coded in LfGroup sections"""
    w, h = 2600, 2100
    data, src = synth_src(w, h, SEED, bpp=16, wide=1, tree=1, squeeze=1)
    px, said, counts = gpu_decode(gpu, data, U16)
    assert said["used"] == 1 and counts[1] == 0 and counts[2] == 0
    assert np.array_equal(px, expected_pixels(src, 16, U16))


@pytest.mark.gpu
def test_gpu_region_scale_orientation(gpu):
    """composition with the features that work on packed pixels, against numpy on the whole wide decode"""
    from test_scale import box
    from test_orient import orient
    w, h = 600, 300
    data, src = synth_src(w, h, SEED, bpp=16, wide=1, tree=2, alpha=1)
    whole = expected_pixels(src, 16, U16)
    for fmt, full in ((gpu.J40_U16X4, whole), (gpu.J40_U8X4, expected_pixels(src, 16, U8))):
        err, px = gpu.decode_region(data, 251, 37, 290, 231, fmt, wide=True)   # off the group grid, three groups
        assert err == "" and np.array_equal(px, full[37:37 + 231, 251:251 + 290])
        for k in (1, 2):
            err, px = gpu.decode(data, fmt, scale=k, wide=True)
            assert err == "" and np.array_equal(px, box(full, k)), "scale %d" % k
    turned, tsrc = synth_src(w, h, SEED, bpp=16, wide=1, tree=2, alpha=1, orientation=6)
    assert np.array_equal(tsrc, src)
    err, px = gpu.decode(turned, gpu.J40_U16X4, orient=True, wide=True)
    assert err == "" and px.shape == (w, h, 4) and np.array_equal(px, orient(whole, 6))
    err, px = gpu.decode(turned, gpu.J40_U16X4, wide=True)
    assert err == "" and np.array_equal(px, whole)


@pytest.mark.gpu
def test_gpu_group_range(gpu):
    """a partial group range of a wide frame goes through the _rect pack kernels: two ranges written into one buffer give the whole
    picture, and each writes its own groups' pixels only (tests/test_gpu_parity.py's form)"""
    import torch
    from j40_amd import sharding
    w, h = 600, 300
    data, src = synth_src(w, h, SEED, bpp=16, wide=1, tree=1)
    whole = expected_pixels(src, 16, U16)
    fr = gpu.Frame(data, wide=True)
    try:
        fr.set_output_format(gpu.J40_U16X4)
        fr.upload(0)
        out = torch.full((h, w, 4), 9, dtype=torch.int16, device="cuda:0")
        stream = torch.cuda.current_stream().cuda_stream
        for first, count in ((1, 3), (0, 1), (4, 2)):     # groups 1, 2 (first row) and 3 (second row); group 0; groups 4, 5
            fr.set_group_range(first, count)
            before = out.clone()
            fr.decode(out.data_ptr(), w * 8, stream)
            torch.cuda.synchronize()
            assert fr.status() == "" and fr.wide()["used"] == 1
            mine = torch.zeros((h, w), dtype=torch.bool, device="cuda:0")
            for x0, y0, x1, y1 in sharding.range_rectangles(first, count, w, h, fr.info["group_size_shift"]):
                mine[y0:y1, x0:x1] = True
            assert torch.equal(out[~mine], before[~mine]), "a range wrote outside its own groups"
        assert np.array_equal(out.cpu().numpy().view(np.uint16), whole)
    finally:
        fr.close()


@pytest.mark.gpu
def test_gpu_sequence_of_wide_frames(gpu):
    """every coded frame of a sequence is an ordinary handle: two full frames, each the picture of its own seed"""
    w, h = 300, 200
    data = synth("modular", w, h, SEED, bpp=16, wide=1, tree=2, frames=2, anim=1, durations="1,1")
    frames, _ = gpu.decode_frames(data, gpu.J40_U16X4, wide=True)
    assert len(frames) == 2
    for k, (px, _) in enumerate(frames):
        _, src = synth_src(w, h, SEED + k, bpp=16, wide=1, tree=2)
        assert np.array_equal(px, expected_pixels(src, 16, U16)), "frame %d" % k
    with pytest.raises(gpu.J40Error) as e:
        gpu.decode_frames(data, gpu.J40_U16X4)
    assert e.value.code == "fm32"


@pytest.mark.gpu
def test_gpu_narrow_before_and_after_wide(gpu):
    """the device memory caches hand blocks from one frame to the next by size in bytes: a narrow frame decodes to the same pixels
    before and after a wide one of the same picture size"""
    w, h = 600, 300
    narrow = synth("modular", w, h, SEED, bpp=12, tree=2)
    wide, src = synth_src(w, h, SEED, bpp=16, wide=1, tree=2)
    outs = []
    for data in (narrow, wide, narrow, wide):
        err, px = gpu.decode(data, gpu.J40_U16X4, wide=True)
        assert err == ""
        outs.append(px)
    assert np.array_equal(outs[0], outs[2]) and np.array_equal(outs[1], outs[3])
    assert np.array_equal(outs[1], expected_pixels(src, 16, U16))
    assert np.array_equal(outs[0], gpu.decode(narrow, gpu.J40_U16X4)[1])
