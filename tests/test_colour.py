"""The colour mode without a device (include/j40hip.h: j40hip_frame_set_colour): the parse of ColourEncoding, the
gamut matrices, the transfer stage of device/colour_dev.h compiled for the host (tests/hostsim/colour_sim.cpp), the setter's refusals.
PARITY UNPINNED: the reference drops the encoding; the formulas are the standards', written out in colour_streams.py.

Bars. Parse: exact. Matrices: 1e-6 against known answers, rows summing to 1. Threshold lookup: equal to the long way for every float of
the table's range and the samples outside it. The long way at bpp 8, 10, 12, 16 against the float64 formula on the same float32 input:
equal, except where the float64 unrounded level lies within 2^-10 of a half-integer -- there within one level -- and that exception is
taken by at most 1 % of a log-spaced sweep over [2^-24, 2] (the band itself is 2 * 2^-10 = 0.2 % of a smooth sweep)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from streams import synth, ROOT
import colour_streams as X


@pytest.fixture(scope="module")
def sim(built):
    return X.ColourSim()


@pytest.fixture(scope="module")
def j40(built):
    import j40_amd
    j40_amd.lib()
    return j40_amd


def frame_facts(j40, data, **kw):
    """what the parse makes of a stream besides its colour encoding: the frame's info words, its section sizes, the colour constants"""
    fr = j40.Frame(data, **kw)
    try:
        info = np.zeros(21, np.int64)
        j40.lib().j40hip_frame_info(fr.h, info.ctypes.data)
        m, bias, it, kx, kb = fr.colour_consts()
        return info.tolist(), list(fr.section_sizes()), m.tolist(), bias.tolist(), float(it), fr.colour_encoding()
    finally:
        fr.close()


# ---------------------------------------------------------------- 1. parse

P3 = ((680000, 320000), (265000, 690000), (150000, 60000))
BT2100 = ((708000, 292000), (170000, 797000), (131000, 46000))
SRGB = ((640000, 330000), (300000, 600000), (150000, 60000))
WHITES = {1: (312700, 329000), 10: (333333, 333333), 11: (314000, 351000)}
ENUM_CASES = [dict(white=w, primaries=p, tf=t) for w in (1, 10, 11) for p, t in ((1, 8), (9, 16), (11, 18))] + \
             [dict(white=1, primaries=1, tf=t) for t in (1, 2, 13, 17)]
CUSTOM_CASES = [
    dict(white=2, whitexy="345700,358500"),
    dict(primaries=2, primxy="680000,320000,265000,690000,150000,60000"),
    dict(white=2, whitexy="-5,1100000", primaries=2, primxy="734700,265300,0,1000000,100,-77000"),   # (negative and > 1: the sign fold, every selector of the U32)
    dict(gamma=4545455), dict(gamma=1), dict(gamma=10000000),
    dict(white=11, primaries=11, gamma=3846154),
]


@pytest.mark.parametrize("mode", ["vardct", "modular"])
@pytest.mark.parametrize("case", ENUM_CASES + CUSTOM_CASES, ids=lambda c: "_".join("%s%s" % (k[0], str(v)[:9]) for k, v in c.items()))
def test_colour_encoding_is_parsed(j40, mode, case):
    base = dict(passes=2) if mode == "vardct" else dict(xyb=1)
    plain = frame_facts(j40, synth(mode, 37, 21, X.SEED, **base))
    got = frame_facts(j40, synth(mode, 37, 21, X.SEED, **base, **case))
    assert got[:5] == plain[:5]   # the same frame as before: sizes, sections, constants
    ce = got[5]
    assert plain[5] == dict(colour_space=0, white_point=1, white_xy=WHITES[1], primaries=1, primaries_xy=SRGB, have_gamma=False, gamma=0, transfer=13, intent=1, want_icc=False)
    white = case.get("white", 1); prim = case.get("primaries", 1)
    assert ce["colour_space"] == 0 and ce["white_point"] == white and ce["primaries"] == prim and ce["intent"] == 1 and not ce["want_icc"]
    assert ce["white_xy"] == (tuple(int(t) for t in case["whitexy"].split(",")) if white == 2 else WHITES[white])
    if prim == 2:
        v = [int(t) for t in case["primxy"].split(",")]
        assert ce["primaries_xy"] == ((v[0], v[1]), (v[2], v[3]), (v[4], v[5]))
    else:
        assert ce["primaries_xy"] == {1: SRGB, 9: BT2100, 11: P3}[prim]
    assert ce["have_gamma"] == ("gamma" in case) and ce["gamma"] == case.get("gamma", 0)
    assert ce["transfer"] == (13 if "gamma" in case else case.get("tf", 13))


def test_refused_streams_stay_refused(j40):
    """the checks in front of the fields stay: a white point, primaries, transfer function the format does not know, a gamma of 0"""
    for opts, code in ((dict(white=3), "wpt?"), (dict(primaries=3), "prm?"), (dict(tf=3), "tfn?"), (dict(tf=19), "tfn?"), (dict(gamma=10000001), "gama")):
        with pytest.raises(j40.J40Error) as e:
            j40.Frame(synth("vardct", 37, 21, X.SEED, passes=2, cenc=1, **opts))
        assert e.value.code == code


# ---------------------------------------------------------------- 2. gamut matrices

def test_gamut_matrices_known_answers(j40):
    code, p, lum = j40.colour_gamut_matrix(X.enc_words())
    assert code == "" and np.abs(p - np.eye(3)).max() < 1e-12
    assert np.abs(lum - [0.2126390059, 0.7151686788, 0.0721923154]).max() < 1e-6        # (IEC 61966-2-1's Y row from the xy)
    code, p, lum = j40.colour_gamut_matrix(X.enc_words(primaries=9))
    # BT.2087's matrix BT.709 -> BT.2020 (its table rounds to 4 places), from the xy to 1e-6 of the exact quotient
    assert code == "" and np.abs(p - [[0.6274, 0.3293, 0.0433], [0.0691, 0.9195, 0.0114], [0.0164, 0.0880, 0.8956]]).max() < 5e-5
    assert np.abs(p[0] - [0.627403896, 0.329283038, 0.043313066]).max() < 1e-6
    assert np.abs(lum - [0.2627002, 0.6779981, 0.0593017]).max() < 1e-6                 # (BT.2020's luminance coefficients)
    code, p, lum = j40.colour_gamut_matrix(X.enc_words(primaries=11))
    assert code == "" and np.abs(p[0] - [0.822461969, 0.177538031, 0.0]).max() < 1e-6   # (sRGB -> Display P3)


@pytest.mark.parametrize("white", [1, 10, 11, 2])
@pytest.mark.parametrize("primaries", [1, 9, 11, 2])
def test_gamut_matrix_maps_white_to_white(j40, white, primaries):
    enc = X.enc_words(white=white, primaries=primaries, whitexy=(345700, 358500), primxy=(734700, 265300, 274000, 717000, 167000, 9000))
    code, p, lum = j40.colour_gamut_matrix(enc)
    assert code == ""
    assert np.abs(p.sum(1) - 1).max() < 1e-6 and abs(lum.sum() - 1) < 1e-6
    # the long way round in numpy: RGB -> XYZ of both sets, Bradford between the white points
    def xyz(xy):
        return np.array([xy[0] / xy[1], 1.0, (1 - xy[0] - xy[1]) / xy[1]])
    def rgb2xyz(prim, wh):
        m = np.stack([xyz(q) for q in prim], 1)
        return m * np.linalg.solve(m, xyz(wh))
    wh = (1 / 3, 1 / 3) if white == 10 else (enc[2] / 1e6, enc[3] / 1e6)
    prim = [(enc[5 + 2 * c] / 1e6, enc[6 + 2 * c] / 1e6) for c in range(3)]
    d65 = (0.3127, 0.3290)
    B = np.array([[0.8951, 0.2664, -0.1614], [-0.7502, 1.7135, 0.0367], [0.0389, -0.0685, 1.0296]])
    adapt = np.linalg.inv(B) @ np.diag((B @ xyz(wh)) / (B @ xyz(d65))) @ B
    want = np.linalg.inv(rgb2xyz(prim, wh)) @ adapt @ rgb2xyz([(0.64, 0.33), (0.30, 0.60), (0.15, 0.06)], d65)
    assert np.abs(p - want).max() < 1e-9


def test_degenerate_chromaticities_are_refused(j40):
    assert j40.colour_gamut_matrix(X.enc_words(primaries=2, primxy=(100000, 100000, 200000, 200000, 300000, 300000)))[0] == "Ucs?"   # on one line
    assert j40.colour_gamut_matrix(X.enc_words(white=2, whitexy=(300000, 0)))[0] == "Ucs?"


# ---------------------------------------------------------------- 3. the transfer stage

TF_CASES = {   # name -> (encoding words, intensity_target)
    "linear": (X.enc_words(tf=8), 255), "srgb": (X.enc_words(tf=13), 255), "bt709": (X.enc_words(tf=1), 255), "dci": (X.enc_words(tf=17), 255),
    "gamma_0.45": (X.enc_words(gamma=4545455), 255), "gamma_1": (X.enc_words(gamma=10000000), 255), "gamma_0.1": (X.enc_words(gamma=1000000), 255),
    "pq_255": (X.enc_words(tf=16), 255), "pq_4000": (X.enc_words(tf=16), 4000), "pq_10000": (X.enc_words(tf=16), 10000), "hlg": (X.enc_words(tf=18), 1000),
}


NO_TABLE = {"gamma_0.1"}   # x^0.1 has 8-bit levels down to 2^-90: more buckets than the table holds, the tail evaluates the curve


@pytest.mark.parametrize("name", sorted(set(TF_CASES) - NO_TABLE))
def test_threshold_lookup_equals_the_long_way(sim, name):
    enc, it = TF_CASES[name]
    r = sim.table_check(enc, it, step=1, threads=min(8, os.cpu_count() or 1))
    print("%s: buckets %d..%d (2^%d .. 2^%d), %d floats compared, %d differ (first 0x%08x)" % (name, r["blo"], r["bhi"], (r["blo"] >> 7) - 127, (r["bhi"] >> 7) - 127, r["compared"], r["differ"], r["first"]))
    assert r["table"] and r["differ"] == 0
    assert r["compared"] > (r["bhi"] - r["blo"] + 1) << 16
    # the thresholds are the float64 model's to a float's neighbour: level k begins where the model says, one float either way
    thr = r["thr"]
    fin = np.isfinite(thr[1:256])
    t = thr[1:256][fin]
    assert len(t) > 100 and (np.diff(t) > 0).all()
    k = np.arange(1, 256)[fin]
    below = np.nextafter(np.nextafter(t, np.float32(0)), np.float32(0)); above = np.nextafter(t, np.float32(np.inf))
    assert (X.model_level(enc, it, below, 8)[0] < k).all() and (X.model_level(enc, it, above, 8)[0] >= k).all()


def test_a_gamma_too_steep_for_buckets_has_no_table(sim):
    """x^(1e-7): every level within a few floats of 0 -- a bucket would span them all; the tail evaluates the curve instead"""
    r = sim.table_check(X.enc_words(gamma=1), 255)
    assert not r["table"]
    rng = np.random.default_rng(3)
    xyb = rng.uniform(-0.1, 0.6, (3, 5, 9)).astype(np.float32)
    cc = np.array(list(np.eye(3, dtype=np.float32).ravel()) + [0, 0, 0, 255, 0, 0], np.float32)
    px, tabled = sim.tail(xyb, cc, X.enc_words(gamma=1), [0.2, 0.7, 0.1], 8)
    assert not tabled and px[..., 3].min() == 255


SWEEP = np.exp2(np.linspace(-24, 1, 250001)).astype(np.float32)   # log-spaced over [2^-24, 2]


@pytest.mark.parametrize("bpp", [8, 10, 12, 16])
@pytest.mark.parametrize("name", sorted(TF_CASES))
def test_long_way_equals_the_float64_formula(sim, name, bpp):
    enc, it = TF_CASES[name]
    v = np.concatenate([SWEEP, np.array([0, -1, 1, 2, 1e-30, 1e30, 0.0031308, 0.018, 1 / 12, np.inf, -np.inf, np.nan], np.float32)])
    got = sim.levels(enc, it, v, bpp)
    level, u = X.model_level(enc, it, v.astype(np.float64), bpp)
    band = np.abs(u - np.round(u)) < 2.0 ** -10     # the unrounded level maxpixel * f within 2^-10 of a half-integer
    band &= (u > 0.5) & (u < (1 << bpp) - 0.5)        # (where the clamp has not settled it)
    d = np.abs(got - level)
    print("%s bpp %d: differing %d of %d, all in the band: %s, band share %.4f %%" % (name, bpp, int((d > 0).sum()), d.size, bool((d[~band] == 0).all()), 100 * band.mean()))
    assert (d[~band] == 0).all()
    assert d.max() <= 1
    assert band.mean() <= 0.01


def test_pow_is_float64_accurate(sim):
    rng = np.random.default_rng(1)
    x = np.exp2(rng.uniform(-60, 20, 200000)); p = rng.uniform(0.01, 80, x.size)
    p = np.where(np.abs(p * np.log(x)) > 600, 0.1, p)
    rel = np.abs(sim.pow(x, p) / x ** p - 1)
    print("colour_pow: largest relative error %.3g" % rel.max())
    assert rel.max() < 2e-13   # (|p ln x| <= 600 times the 1.1e-16 of its rounding, and the two polynomials' own)


def test_hlg_inverse_ootf(sim):
    rng = np.random.default_rng(2)
    lum = np.array([0.2627, 0.6780, 0.0593], np.float32)
    v = np.exp2(rng.uniform(-20, 1, (5000, 3))).astype(np.float32)
    for it in (255, 1000, 4000):
        got = sim.hlg_ootf(X.enc_words(tf=18), it, lum, v)
        want = X.model_hlg_ootf(it, lum.astype(np.float64), v.astype(np.float64))
        # float32: Yd's three products and two sums, the scale's rounding, the product's (|1 / gamma - 1| < 0.3 of Yd's error goes on)
        assert np.abs(got / want - 1).max() < 4 * 2.0 ** -24
    v[0] = [-1, -1, -1]; v[1] = [0, 0, 0]
    got = sim.hlg_ootf(X.enc_words(tf=18), 1000, lum, v)
    assert np.array_equal(got[:2], v[:2])   # nothing where Yd <= 0


def test_tail_pixels_on_the_host(sim):
    """colour_tail_pixel end to end against the model: identity mixing (the planes are the linear values' cube roots), every curve, u8 and u16"""
    rng = np.random.default_rng(4)
    lin = np.exp2(rng.uniform(-12, 0.5, (3, 21, 37)))
    # X, Y, B with zero bias and the identity as matrix: pp = (Y + X, Y - X, B), s = pp^3
    r, g, b = np.cbrt(lin)
    xyb = np.stack([(r - g) / 2, (r + g) / 2, b]).astype(np.float32)
    cc = np.array(list(np.eye(3, dtype=np.float32).ravel()) + [0, 0, 0, 255, 0, 0], np.float32)
    lum = np.array([0.2627, 0.6780, 0.0593], np.float32)
    for name, (enc, it) in sorted(TF_CASES.items()):
        cc[12] = it
        for bpp in (8, 10, 16):
            pp = np.stack([xyb[1] + xyb[0], xyb[1] - xyb[0], xyb[2]], -1)
            v = ((pp * pp * pp) * (np.float32(255) / np.float32(it))).astype(np.float32)   # (float32 as the tail: two products, the scale)
            if int(enc[13]) == 18 and not int(enc[11]):
                v = sim.hlg_ootf(enc, it, lum, v.reshape(-1, 3)).reshape(v.shape)
            level = sim.levels(enc, it, v, bpp).astype(np.int64)
            for fmt, conv in ((X.U8X4, X.to_u8), (X.U16X4, X.to_u16)):
                px, tabled = sim.tail(xyb, cc, enc, lum, bpp, fmt)
                assert tabled == (bpp == 8 and name not in NO_TABLE)
                assert np.array_equal(px[..., :3], conv(level, bpp)), (name, bpp, fmt)
                assert (px[..., 3] == (255 if fmt == X.U8X4 else 65535)).all()


# ---------------------------------------------------------------- 4. the setter

def test_setter_refusals(j40):
    def verdict(data, mode=1, prepare=None, **kw):
        fr = j40.Frame(data, **kw)
        try:
            if prepare:
                prepare(fr)
            code = fr.set_colour(mode)
            return code, fr.colour()
        finally:
            fr.close()
    pq = dict(primaries=9, tf=16)
    code, c = verdict(synth("vardct", 37, 21, X.SEED, passes=2, **pq))
    assert code == "" and c["applies"] and c["in_force"] and c["transfer"] == 16 and c["primaries"] == 9 and not c["used"]
    # the sRGB default: accepted, and the usual way
    code, c = verdict(synth("vardct", 37, 21, X.SEED, passes=2))
    assert code == "" and c["applies"] and not c["in_force"]
    code, c = verdict(synth("vardct", 37, 21, X.SEED, passes=2, cenc=1))   # (written out, still the default)
    assert code == "" and c["applies"] and not c["in_force"]
    # "Ucs?": the profile is not interpreted, no curve, grey, YCbCr, a Modular frame rendered as R, G, B
    assert verdict(synth("vardct", 300, 260, X.SEED, icc=700))[0] == "Ucs?"
    assert verdict(synth("vardct", 37, 21, X.SEED, passes=2, tf=2))[0] == "Ucs?"
    assert verdict(synth("modular", 37, 21, X.SEED, xyb=1, grey=1))[0] == "Ucs?"
    assert verdict(synth("vardct", 64, 64, X.SEED, ycbcr=1), ycbcr=True)[0] == "Ucs?"
    mod = synth("modular", 37, 21, X.SEED, xyb=1, **pq)
    assert verdict(mod)[0] == "Ucs?"
    code, c = verdict(mod, prepare=lambda fr: fr.set_modular_xyb(1))
    assert code == "" and c["in_force"]
    # refused: the frame is left as it was; modes 0 and -1 are never refused
    assert verdict(synth("vardct", 37, 21, X.SEED, passes=2, tf=2), mode=0)[0] == "" and verdict(synth("vardct", 37, 21, X.SEED, passes=2, tf=2), mode=-1)[0] == ""
    # xyb_encoded = 0: the samples are in their signalled space already -- accepted, nothing changes
    code, c = verdict(synth("modular", 37, 21, X.SEED, **pq))
    assert code == "" and not c["applies"] and not c["in_force"]


def test_sequence_refusals_without_a_device(j40):
    """one canvas holds one colour space: the flag on an image the mode refuses as a whole fails the open; a Modular XYB frame without
    the Modular XYB switch is refused among frames that render in the signalled space; without the flag nothing changes"""
    anim = dict(frames=2, anim=1, durations="1,1")
    for opts in (dict(tf=2), ):
        data = synth("vardct", 65, 24, X.SEED, passes=2, **anim, **opts)
        with pytest.raises(j40.J40Error) as e:
            j40.Sequence(data, colour=True)
        assert e.value.code == "Ucs?"
        j40.Sequence(data).close()
    data = synth("modular", 65, 24, X.SEED, xyb=1, primaries=9, tf=16, **anim)
    seq = j40.Sequence(data, colour=True)
    with pytest.raises(j40.J40Error) as e:
        seq.frame(0)
    assert e.value.code == "Ucs?"
    seq.close()
    seq = j40.Sequence(data, colour=True, modular_xyb=True)
    assert seq.frame(0).colour()["in_force"] and seq.frame(1).colour()["in_force"]
    seq.close()
    seq = j40.Sequence(data)
    assert not seq.frame(0).colour()["in_force"]
    seq.close()
    seq = j40.Sequence(synth("vardct", 65, 24, X.SEED, passes=2, **anim), colour=True)   # the default encoding: nothing to refuse
    assert not seq.frame(0).colour()["in_force"]
    seq.close()


# ---------------------------------------------------------------- 5. the stand-alone programs

@pytest.mark.parametrize("program", ["colour_main", "colour_main_san"])
def test_stand_alone_program(built, program):
    r = subprocess.run([os.path.join(ROOT, "build", program)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    print(r.stdout.decode())
    assert r.returncode == 0
