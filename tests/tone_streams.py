"""VarDCT streams whose image header carries a ToneMapping block and / or the custom-transform block (TEST INFRASTRUCTURE, for
tests/test_tone_opsin.py): the generator's tone= and opsin= options, the constants each row writes, and the shapes the tests share.

Every other stream of the suite runs the dequantiser and the colour tails at one point: intensity_target 255, the default
opsin_inv_mat, three equal opsin biases, the default quant biases. A row here is (name, constants); `constants` holds what the test
WROTE -- "tone": (intensity_target, min_nits), "m": the matrix [3][3], "bias", "qbias", "qnum" -- every number rounded to the nearest
f16, which the generator demands (its f16_bits dies otherwise) and which makes the parsed float32 values equal them exactly."""
import numpy as np

from streams import synth

SEED = 31


def f16(x):
    return float(np.float16(x))


# the defaults (j40.h:3109-3143) rounded to f16
D = [[f16(v) for v in row] for row in ((11.031566901960783, -9.866943921568629, -0.16462299647058826),
                                        (-3.254147380392157, 4.418770392156863, -0.16462299647058826),
                                        (-3.6588512862745097, 2.7129230470588235, 1.9459282392156863))]
DB = [f16(-0.0037930732552754493)] * 3
DQ = [f16(1.0 - 0.05465007330715401), f16(1.0 - 0.07005449891748593), f16(1.0 - 0.049935103337343655)]
DQN = f16(0.145)
S = [D[2], D[1], D[0]]      # D with its first and third rows exchanged
_DISTINCT = [f16(-0.002), f16(-0.004), f16(-0.008)]
_QB = [0.5, 0.75, 1.25]


def _opsin(m=D, bias=DB, qbias=DQ, qnum=DQN):
    return dict(m=[list(r) for r in m], bias=list(bias), qbias=list(qbias), qnum=qnum)


def _tone(it, min_nits):
    return dict(tone=(f16(it), f16(min_nits)))


# (name, constants, options every stream of the row carries)
ROWS = [
    ("tone_255", _tone(255, 1), {}),            # written-out defaults: the twin's pixels, byte for byte
    ("tone_64", _tone(64, 1), {}),              # itscale about 4: clamping at the top
    ("tone_1000", _tone(1000, 1), {}),          # dark pictures, the sRGB curve's linear segment
    ("tone_10000", _tone(10000, 1), {}),
    ("tone_max", _tone(65504, 1), {}),          # everything in the linear segment
    ("tone_half", _tone(0.5, 0.25), {}),        # itscale = 510
    ("tone_half_12_bit", _tone(0.5, 0.25), dict(bpp=12)),   # the reference's (int16_t) wrap
    ("bias_distinct", _opsin(bias=_DISTINCT), {}),          # per-channel bias and cube root
    ("bias_zero", _opsin(bias=[0.0, 0.0, 0.0]), {}),        # cbrtf(0)
    ("bias_positive", _opsin(bias=[f16(0.004), f16(0.002), f16(0.001)]), {}),   # sign of the cube root
    ("qbias", _opsin(qbias=_QB, qnum=0.5), {}),             # the dequantiser alone
    ("swapped_all", _opsin(S, _DISTINCT, _QB, 0.5), {}),    # matrix orientation, everything at once
    ("swapped_all_tone_1000", dict(_opsin(S, _DISTINCT, _QB, 0.5), **_tone(1000, 1)), {}),   # both blocks in one header
]
ROW = {r[0]: r for r in ROWS}
NAMES = [r[0] for r in ROWS]

# the option sets every row runs with; `twelve` is added for the rows in TWELVE (tone_half_12_bit carries bpp=12 in all of its sets)
SETS = [("plain", {}), ("forward", dict(forward=1)), ("all_transforms", dict(maxlog=8, bctx=1))]
TWELVE = ("tone_64", "swapped_all")
CASES = [(name, tag) for name in NAMES for tag, _ in SETS] + [(name, "twelve") for name in TWELVE]
CASE_IDS = ["%s-%s" % c for c in CASES]


def set_options(tag):
    return dict(bpp=12) if tag == "twelve" else dict(SETS)[tag]


def size_of(opts):
    return (776, 520) if opts.get("maxlog") == 8 else (520, 264)


def _num(v):
    """nine significant digits name a float32, so an f16, exactly"""
    s = "%.9g" % float(v)
    assert np.float32(s) == np.float32(v) == np.float16(v), v
    return s


def _bits(v):
    """the generator's other spelling of an f16, its bits: sixteen of them keep the stream cache's file names short"""
    assert np.float32(np.float16(v)) == np.float32(v), v
    return "h%04x" % int(np.float16(v).view(np.uint16))


def written_options(consts, spell=_bits):
    """the generator's options that write `consts`"""
    o = {}
    if "tone" in consts:
        o["tone"] = ",".join(_num(v) for v in consts["tone"])
    if "m" in consts:
        o["opsin"] = ",".join(spell(v) for v in [v for r in consts["m"] for v in r] + consts["bias"] + consts["qbias"] + [consts["qnum"]])
    return o


def expected_consts(consts):
    """what a parser must hold after the header: (matrix [3, 3], bias [3], intensity_target, quant_bias [3], quant_bias_num), float32;
    the format's defaults at full float precision (j40.h:3109-3143) where a block is absent"""
    f32 = np.float32
    if "m" in consts:
        m, bias, qb, qn = np.array(consts["m"], f32), np.array(consts["bias"], f32), np.array(consts["qbias"], f32), f32(consts["qnum"])
    else:
        m = np.array([[11.031566901960783, -9.866943921568629, -0.16462299647058826], [-3.254147380392157, 4.418770392156863, -0.16462299647058826],
                      [-3.6588512862745097, 2.7129230470588235, 1.9459282392156863]], f32)
        bias = np.full(3, -0.0037930732552754493, f32)
        qb = np.array([f32(1.0) - f32(0.05465007330715401), f32(1.0) - f32(0.07005449891748593), f32(1.0) - f32(0.049935103337343655)], f32)
        qn = f32(0.145)
    return m, bias, f32(consts["tone"][0] if "tone" in consts else 255.0), qb, qn


def options_of(name, tag, **more):
    _, consts, own = ROW[name]
    return dict(set_options(tag), **own, **written_options(consts), **more)


def twin_options(name, tag, **more):
    return dict(set_options(tag), **ROW[name][2], **more)


def stream(name, tag="plain", size=None, **more):
    opts = options_of(name, tag, **more)
    w, h = size or size_of(opts)
    return synth("vardct", w, h, SEED, **opts)


def twin(name, tag="plain", size=None, **more):
    """the same stream without tone= / opsin="""
    opts = twin_options(name, tag, **more)
    w, h = size or size_of(opts)
    return synth("vardct", w, h, SEED, **opts)
