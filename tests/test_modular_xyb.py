"""Modular frames of XYB images through the XYB colour tail, without a device (include/j40hip.h: j40hip_frame_set_modular_xyb; DESIGN.md
section 4). PARITY UNPINNED: the reference renders such a frame's integers as R, G, B, so nothing here is held against it but the
switch-off bytes. The CPU half runs device/modular_xyb_dev.h compiled for the host (tests/hostsim/modular_xyb_sim.cpp) over the planes
the Modular device functions decode on the CPU (tests/hostsim/wide_sim.cpp).

Bars. Planes: bit for bit numpy's float32(c) * float32(m), the integer sum first. Pixels against the float64 model
(modxyb_streams.float64_model): within one level everywhere, and equal wherever the model's unrounded value is farther than 1e-3 of a
level from a rounding boundary; the excluded share is printed and stays under 1 %. xybpic=1 pictures: the decode's largest distance
from the source picture is at most the model's own plus one level. Index and refusals: exact."""
import os
import subprocess

import numpy as np
import pytest

from streams import synth, ROOT
import modxyb_streams as X
from lf_streams import WIDE, lf_stream

INT32_MIN, INT32_MAX = -2 ** 31, 2 ** 31 - 1


@pytest.fixture(scope="module")
def sim(built):
    return X.XybSim()


@pytest.fixture(scope="module")
def widesim(built):
    from test_wide_modular import Sim
    return Sim()


@pytest.fixture(scope="module")
def j40(built):
    import j40_amd
    j40_amd.lib()
    return j40_amd


def decoded_planes(widesim, data, w, h, nplanes=3, wide=False):
    """(the stream's pixels with the switch off, its planes [nplanes, h, w] after the inverse transforms) by the Modular device functions on the CPU"""
    err, px = widesim.decode(data, w, h, 0, X.PARSE_WIDE if wide else 0)
    assert err == "", err
    c = widesim.planes(nplanes, w, h)
    return px, (c if wide else c.astype(np.int16))


# ---------------------------------------------------------------- 1. planes

def extremes(dtype, rng, shape):
    info = np.iinfo(dtype)
    c = rng.integers(-700, 700, size=(3,) + shape).astype(dtype)
    special = [info.min, info.max, 0, -1, 1] + ([2 ** 24, 2 ** 24 + 1, -(2 ** 24) - 1, 2 ** 30 + 12345, INT32_MIN + 1] if dtype == np.int32 else [32767, -32768])
    flat = c.reshape(3, -1)
    k = 0
    for a in special:                      # every pair of extremes meets in the sum c2 + c0
        for b in special:
            flat[0, k] = a; flat[2, k] = b; flat[1, k] = special[k % len(special)]
            k += 1
    return c


@pytest.mark.parametrize("dtype", [np.int16, np.int32], ids=["int16", "int32"])
@pytest.mark.parametrize("m", [X.M_DEFAULT, X.M_LFDEQUANT], ids=["default_m", "lfdequant_m"])
def test_planes_equal_the_float32_statement(sim, dtype, m):
    rng = np.random.default_rng(5)
    for shape in ((1, 1 + 100), (5, 63), (9, 257)):
        c = extremes(dtype, rng, shape)
        got = sim.planes(c, m)
        want = X.statement(c, m)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
        # a rectangle inside the planes reads its own samples
        h, w = shape
        rect = (w // 3, h // 2, w - w // 3 - 1, h - h // 2)
        assert np.array_equal(sim.planes(c, m, rect).view(np.uint32), want[:, rect[1]:rect[1] + rect[3], rect[0]:rect[0] + rect[2]].view(np.uint32))
    if dtype == np.int32:   # the sum is taken in 64 bits: INT32_MAX + INT32_MAX does not wrap
        c = np.array([[[INT32_MAX]], [[0]], [[INT32_MAX]]], np.int32)
        assert sim.planes(c, m)[2, 0, 0] == np.float32(2 * INT32_MAX) * np.float32(m[2])
    else:                   # ... and an int16 sum in 32
        c = np.array([[[32767]], [[0]], [[32767]]], np.int16)
        assert sim.planes(c, m)[2, 0, 0] == np.float32(65534) * np.float32(m[2])


def test_lfdequant_is_parsed(j40):
    data, _ = X.xybpic_stream(37, 21, lfdequant=X.LFDEQUANT)
    m, _, _ = X.host_consts(j40, data)
    assert np.array_equal(m, X.M_LFDEQUANT)
    m, _, _ = X.host_consts(j40, X.xybpic_stream(37, 21)[0])
    assert np.array_equal(m, X.M_DEFAULT)


# ---------------------------------------------------------------- 2. pixels against the float64 model

MODEL_CASES = [
    ("default_one_section", 37, 21, dict()),
    ("default_nine_groups", 300, 270, dict(groupshift=7)),
    ("lfdequant", 300, 270, dict(groupshift=7, lfdequant=X.LFDEQUANT)),
    ("tone", 300, 270, dict(groupshift=7, tone=X.TONE)),
    ("opsin", 300, 270, dict(groupshift=7, opsin=None)),     # (filled in below: tone_streams' bias_distinct row)
]


def check_against_model(got, c, m, cc, what):
    u, model = X.float64_model(c, m, cc)
    exempt = X.boundary_exempt(u)
    d = np.abs(got[..., :3].astype(np.int32) - model.astype(np.int32))
    share = float(exempt.mean())
    print("%s: max |delta| %d, differing %d of %d, excluded by the boundary clause %.4f %%" % (what, d.max(), int((d > 0).sum()), d.size, 100 * share))
    assert d.max() <= 1
    assert not ((d > 0) & ~exempt).any(), "%d samples differ from the model away from a rounding boundary" % int(((d > 0) & ~exempt).sum())
    assert share < 0.01
    return u, model


@pytest.mark.parametrize("name,w,h,opts", MODEL_CASES, ids=[c[0] for c in MODEL_CASES])
def test_pixels_against_float64_model(sim, widesim, j40, name, w, h, opts):
    opts = dict(opts)
    if "opsin" in opts:
        opts["opsin"] = X.opsin_option()
    data, _ = X.xybpic_stream(w, h, **opts)
    m, cc, _ = X.host_consts(j40, data)
    if name == "tone":
        assert cc[12] == 64.0
    if name == "opsin":
        assert len(set(cc[9:12].tolist())) == 3
    _, c = decoded_planes(widesim, data, w, h)
    got = sim.pack(c, None, m, cc)
    assert (got[..., 3] == 255).all()
    check_against_model(got, c, m, cc, name)
    got16 = sim.pack(c, None, m, cc, u16=True)
    assert np.array_equal(got16, got.astype(np.uint16) * 257)   # an 8-bit frame's 16-bit output


def test_alpha_is_rendered_as_the_pack_kernels_render_it(sim, widesim, j40):
    w, h = 37, 21
    data = X.xyb_stream(w, h, alpha=1)
    m, cc, _ = X.host_consts(j40, data)
    plain, c4 = decoded_planes(widesim, data, w, h, 4)
    got = sim.pack(c4[:3], c4[3], m, cc)
    assert np.array_equal(got[..., 3], plain[..., 3]) and np.array_equal(got[..., 3], X.alpha_u8(c4[3]))
    assert np.array_equal(sim.pack(c4[:3], c4[3], m, cc, u16=True)[..., 3], X.alpha_u16(c4[3]))
    assert np.array_equal(got[..., :3], sim.pack(c4[:3], None, m, cc)[..., :3])


# ---------------------------------------------------------------- 3. xybpic=1 pictures

@pytest.mark.parametrize("w,h,opts", [(37, 21, dict()), (300, 270, dict(groupshift=7)), (300, 270, dict(groupshift=7, lfdequant=X.LFDEQUANT))], ids=["one_section", "nine_groups", "lfdequant"])
def test_xybpic_decodes_to_its_source(sim, widesim, j40, w, h, opts):
    data, src = X.xybpic_stream(w, h, **opts)
    m, cc, _ = X.host_consts(j40, data)
    _, c = decoded_planes(widesim, data, w, h)
    got = sim.pack(c, None, m, cc)[..., :3]
    _, model = X.float64_model(c, m, cc)
    want = src.astype(np.float64) * 255.0
    d_got, d_model = float(np.abs(got - want).max()), float(np.abs(model - want).max())
    print("xybpic %dx%d %s: largest distance from the source picture: decode %.3f levels, float64 model %.3f levels" % (w, h, opts, d_got, d_model))
    assert d_got <= d_model + 1.0
    assert d_model < 32.0   # (a picture, not noise: the quantisation steps are a few levels)


# ---------------------------------------------------------------- 4. index and refusals

def seq_codes(j40, data, **kw):
    try:
        s = j40.Sequence(data, **kw)
    except j40.J40Error as e:
        return e.code
    try:
        return [s.frame_info(k)["code"] for k in range(s.num_frames)]
    finally:
        s.close()


def test_modular_lf_frame_needs_both_switches(j40):
    data = lf_stream(WIDE, lfmodular=1, global_scale=4096, quant_lf=16, nocfl=1)
    assert seq_codes(j40, data) == "TODO"
    assert seq_codes(j40, data, lf_frames=True) == "TODO"
    assert seq_codes(j40, data, modular_xyb=True) == "TODO"
    assert seq_codes(j40, data, lf_frames=True, modular_xyb=True) == ["", ""]
    s = j40.Sequence(data, lf_frames=True, modular_xyb=True)
    try:
        assert s.frame_lf(0)["lf_level"] == 1 and s.frame_info(0)["type"] == 1 and not s.frame_info(0)["shown"] and not s.frame_info(0)["saved"]
        fr = s.frame(0)
        assert fr.info["is_modular"] == 1 and fr.modular_xyb() == dict(applies=1, on=1, sample_bytes=2, used=0)
    finally:
        s.close()
    # a VarDCT LF frame is served with the LF switch alone, as before
    assert seq_codes(j40, lf_stream(WIDE, global_scale=4096, quant_lf=16, nocfl=1), lf_frames=True) == ["", ""]


def test_generator_refuses_lfmodular_outside_its_conditions(built):
    from streams import SYNTH
    for opts in (["nocfl=1"], ["global_scale=4096", "quant_lf=16"], ["global_scale=2048", "quant_lf=16", "nocfl=1"]):
        r = subprocess.run([SYNTH, "vardct", "2060", "70", "7", os.devnull, "lflevels=1", "lfmodular=1"] + opts, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE)
        assert r.returncode != 0 and b"lfmodular=1" in r.stderr


def test_set_modular_xyb_refusals(j40):
    def answer(data, **kw):
        fr = j40.Frame(data, **kw)
        try:
            before = fr.modular_xyb()
            code = fr.set_modular_xyb(1)
            after = fr.modular_xyb()
            assert fr.set_modular_xyb(0) == "" and fr.set_modular_xyb(-1) == ""   # (off and "as the environment says" always pass)
            return code, before, after
        finally:
            fr.close()
    code, before, after = answer(X.xyb_stream(37, 21))
    assert code == "" and before == dict(applies=1, on=0, sample_bytes=2, used=0) and after["on"] == 1
    code, before, after = answer(X.xyb_stream(37, 21, bpp=16, wide=1), wide=True)
    assert code == "" and after == dict(applies=1, on=1, sample_bytes=4, used=0)
    for what, data in (("VarDCT", synth("vardct", 520, 264, 1)), ("not XYB", synth("modular", 37, 21, X.SEED)), ("YCbCr flag", synth("modular", 37, 21, X.SEED, ycbcr=1))):
        code, before, after = answer(data)
        assert code == "Umx?" and before["applies"] == 0 and after["on"] == 0, what


def test_grey_image_is_refused(j40):
    """an XYB image whose colour encoding says grey still codes three channels (j40.h:3619) and parses; the rule does not apply to it"""
    fr = j40.Frame(X.xyb_stream(37, 21, grey=1))
    try:
        assert fr.info["is_modular"] == 1 and fr.info["xyb_encoded"] == 1
        assert fr.modular_xyb()["applies"] == 0 and fr.set_modular_xyb(1) == "Umx?" and fr.modular_xyb()["on"] == 0
    finally:
        fr.close()


@pytest.mark.parametrize("w,h,opts", [(37, 21, dict()), (300, 270, dict(groupshift=7, alpha=1)), (300, 270, dict(groupshift=7, palette=1))], ids=["one_section", "nine_groups_alpha", "palette"])
def test_switch_off_is_todays_decode(sim, widesim, j40, ref, w, h, opts):
    data = X.xyb_stream(w, h, **opts)
    m, cc, _ = X.host_consts(j40, data)
    n = 4 if opts.get("alpha") else 3
    plain, c = decoded_planes(widesim, data, w, h, n)
    rerr, expect = ref.decode(data)
    assert rerr == "" and np.array_equal(plain, expect)
    off = sim.pack(c[:3], c[3] if n == 4 else None, m, cc, on=False)
    assert np.array_equal(off, expect)
    on = sim.pack(c[:3], c[3] if n == 4 else None, m, cc, on=True)
    assert not np.array_equal(on[..., :3], expect[..., :3]) and np.array_equal(on[..., 3], expect[..., 3])


# ---------------------------------------------------------------- 5. the stand-alone programs

@pytest.mark.parametrize("program", ["modular_xyb_main", "modular_xyb_main_san"])
def test_stand_alone_program(built, program):
    r = subprocess.run([os.path.join(ROOT, "build", program)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    print(r.stdout.decode())
    assert r.returncode == 0
