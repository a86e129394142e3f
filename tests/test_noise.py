"""Photon noise on the host (include/j40hip.h, J40HIP_PARSE_NOISE): the switch, the parse of the NoiseParameters, what is refused, the
seed counters a sequence's index gives its frames, and device/noise_dev.h's generator, jumped fill and tile functions compiled for the
CPU (tests/hostsim/noise_sim.cpp), held bit for bit against numpy's float32 (tests/noise_streams.py) and against a statement of
SplitMix64 and xorshift128+ in Python integers written here. PARITY UNPINNED: the reference holds no code for noise;
tests/test_noise_gpu.py has the device and the anchor that reaches the reference."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import noise_streams as N
from noise_streams import noise_synth, pair, lut_text, lut_of, bits, LUT, ZERO
from streams import ROOT


@pytest.fixture(scope="module")
def j40(built):
    import j40_amd
    return j40_amd


def parse_code(j40, data, **kw):
    try:
        j40.Frame(data, **kw).close()
        return ""
    except j40.J40Error as e:
        return e.code


def sequence_codes(j40, data, **kw):
    """per coded frame: the row's code, else what its handle's parse answers"""
    seq = j40.Sequence(data, **kw)
    try:
        out = []
        for k in range(seq.num_frames):
            code = seq.frame_info(k)["code"]
            if not code:
                try:
                    seq.frame(k)
                except j40.J40Error as e:
                    code = e.code
            out.append(code)
        return out
    finally:
        seq.close()


# ---------------------------------------------------------------- 1. the switch and the refusals

@pytest.mark.parametrize("mode,w,h", [("vardct", N.VW, N.VH), ("modular", N.MW, N.MH)])
def test_switch_and_parameters(j40, monkeypatch, mode, w, h):
    """this is a test that fails without the feature: the keyword does not exist"""
    monkeypatch.delenv("J40HIP_NOISE", raising=False)
    noisy, twin = pair(mode, w, h)
    assert parse_code(j40, noisy) == "TODO"
    assert parse_code(j40, noisy, noise=True) == ""
    assert parse_code(j40, twin) == "" and parse_code(j40, twin, noise=True) == ""
    assert len(noisy) - len(twin) in (10, 11)          # the 80 bits, and what the flag's varint and the section's padding make of them
    monkeypatch.setenv("J40HIP_NOISE", "1")
    assert parse_code(j40, noisy) == ""
    monkeypatch.setenv("J40HIP_NOISE", "0")
    assert parse_code(j40, noisy) == "TODO"
    monkeypatch.delenv("J40HIP_NOISE", raising=False)
    fr = j40.Frame(noisy, noise=True)
    p = fr.noise_params()
    assert np.array_equal(bits(p["lut"]), bits(lut_of(LUT))) and p["seeds"] == (0, 0) and fr.noise_launches() == 0
    assert list((p["lut"] * 1024).astype(int)) == list(LUT)
    fr.close()
    fr = j40.Frame(twin, noise=True)
    assert fr.noise_params() is None
    fr.close()
    # the streamed parse takes the flag too
    fr = j40.Frame.parse_streamed(noisy, flags=j40.PARSE_NOISE)
    assert np.array_equal(fr.noise_params()["lut"], lut_of(LUT))
    fr.close()
    with pytest.raises(j40.J40Error) as e:
        j40.Frame.parse_streamed(noisy)
    assert e.value.code == "TODO"


def test_refusals_at_parse(j40, monkeypatch):
    for env in (None, "1"):
        monkeypatch.delenv("J40HIP_NOISE", raising=False)
        if env:
            monkeypatch.setenv("J40HIP_NOISE", env)
        # an image with xyb_encoded = 0, VarDCT and Modular
        assert parse_code(j40, noise_synth("vardct", N.VW, N.VH, noxyb=1, fullheader=1, noise=lut_text(LUT)), noise=True) == "TODO"
        assert parse_code(j40, noise_synth("vardct", N.VW, N.VH, noxyb=1, fullheader=1, noise=lut_text(LUT), noisetwin=1), noise=True) == ""
        assert parse_code(j40, noise_synth("modular", 64, 64, noise=lut_text(LUT)), noise=True) == "TODO"
        # an LF-only parse of a frame with noise
        assert parse_code(j40, pair("vardct", N.VW, N.VH)[0], noise=True, lf_only=True) == "TODO"
        assert parse_code(j40, pair("vardct", N.VW, N.VH)[1], noise=True, lf_only=True) == ""
        # an LF frame (type 1) with has_noise; the same stream with the noise on the main frame alone parses
        lf = dict(lflevels=1, noise=lut_text(LUT))
        assert sequence_codes(j40, noise_synth("vardct", 2060, 70, noiself=1, **lf), lf_frames=True, noise=True) == ["TODO", ""]
        assert sequence_codes(j40, noise_synth("vardct", 2060, 70, **lf), lf_frames=True, noise=True) == ["", ""]
        assert sequence_codes(j40, noise_synth("vardct", 2060, 70, **lf), lf_frames=True) == ["", "" if env else "TODO"]
        # a reference-only frame (type 2) with has_noise
        ref = dict(frames=2, types="2,0", crops="0,0,264,40;", saves="1,0")
        assert sequence_codes(j40, noise_synth("vardct", N.VW, N.VH, noise=lut_text(LUT) + ";", **ref), patches=True, noise=True) == ["TODO", ""]
        assert sequence_codes(j40, noise_synth("vardct", N.VW, N.VH, noise=";" + lut_text(LUT), **ref), patches=True, noise=True) == ["", ""]


def test_sequence_seed_counters(j40, monkeypatch):
    """visible counts the shown frames before a frame, nonvisible the frames since the last shown one"""
    monkeypatch.delenv("J40HIP_NOISE", raising=False)
    per_frame = ";".join([lut_text(LUT)] * 5)
    data = noise_synth("vardct", N.VW, N.VH, frames=5, anim=1, durations="1,1,0,0,1", saves="0,0,1,2,0", noise=per_frame)
    seq = j40.Sequence(data, noise=True)
    try:
        assert [seq.frame_info(k)["shown"] for k in range(5)] == [1, 1, 0, 0, 1]
        assert [seq.frame(k).noise_params()["seeds"] for k in range(5)] == [(0, 0), (1, 0), (2, 0), (2, 1), (2, 2)]
    finally:
        seq.close()
    assert sequence_codes(j40, data)[0] == "TODO"       # without the switch
    # frames without an entry have no noise
    some = noise_synth("vardct", N.VW, N.VH, frames=3, anim=1, noise=";" + lut_text(LUT) + ";")
    seq = j40.Sequence(some, noise=True)
    try:
        assert [seq.frame(k).noise_params() is None for k in range(3)] == [True, False, True]
        assert seq.frame(1).noise_params()["seeds"] == (1, 0)
    finally:
        seq.close()


# ---------------------------------------------------------------- 2. the generator and the arithmetic on the CPU

class NoiseSim:
    def __init__(self):
        self.L = C.CDLL(os.path.join(ROOT, "build", "libhostsim_noise.so"))
        self.L.noise_sim_pitch.restype = C.c_int64
        self.L.noise_sim_fill.restype = C.c_int32
        self.L.noise_sim_strength.restype = C.c_float
        self.L.noise_sim_strength.argtypes = [C.c_void_p, C.c_float]
        self.L.noise_sim_add.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_float, C.c_float]

    def steps(self, visible, nonvisible, x0, y0, n):
        out = np.zeros(16 * n, np.uint32)
        self.L.noise_sim_steps(C.c_uint32(visible), C.c_uint32(nonvisible), C.c_uint32(x0), C.c_uint32(y0), C.c_int32(n), C.c_void_p(out.ctypes.data))
        return out

    def fill_padded(self, w, h, gdim, visible=0, nonvisible=0, jumped=1):
        pitch = int(self.L.noise_sim_pitch(w))
        raw = np.full((3, h, pitch), -1.0, np.float32)
        assert self.L.noise_sim_fill(C.c_void_p(raw.ctypes.data), w, h, gdim, C.c_uint32(visible), C.c_uint32(nonvisible), jumped) == 0
        return raw

    def fill(self, w, h, gdim, visible=0, nonvisible=0, jumped=1):
        return self.fill_padded(w, h, gdim, visible, nonvisible, jumped)[:, :, :w].copy()

    def add(self, planes, raw_padded, lut, ytox, ytob):
        out = np.array(planes, np.float32, copy=True)
        _, h, w = out.shape
        lut = np.ascontiguousarray(lut, np.float32)
        raw_padded = np.ascontiguousarray(raw_padded, np.float32)
        assert raw_padded.shape == (3, h, int(self.L.noise_sim_pitch(w)))
        self.L.noise_sim_add(out.ctypes.data, raw_padded.ctypes.data, w, h, lut.ctypes.data, ytox, ytob)
        return out

    def strength(self, lut, v):
        lut = np.ascontiguousarray(lut, np.float32)
        return np.float32(self.L.noise_sim_strength(lut.ctypes.data, float(v)))


@pytest.fixture(scope="module")
def sim(built):
    return NoiseSim()


def python_integer_steps(visible, nonvisible, x0, y0, n):
    """SplitMix64 and xorshift128+ in Python integers, sharing no code with either implementation"""
    mask = 0xFFFFFFFFFFFFFFFF

    def mix(z):
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & mask
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & mask
        return z ^ (z >> 31)

    s0 = [mix(((visible << 32) + nonvisible + 0x9E3779B97F4A7C15) & mask)]
    s1 = [mix(((x0 << 32) + y0 + 0x9E3779B97F4A7C15) & mask)]
    for i in range(1, 8):
        s0.append(mix(s0[i - 1])); s1.append(mix(s1[i - 1]))
    out = []
    for _ in range(n):
        for i in range(8):
            a, b = s0[i], s1[i]
            v = (a + b) & mask
            s0[i] = b
            a ^= (a << 23) & mask
            s1[i] = a ^ b ^ (a >> 18) ^ (b >> 5)
            out += [v & 0xFFFFFFFF, v >> 32]
    return np.array(out, np.uint32)


@pytest.mark.parametrize("seeds", [(0, 0, 0, 0), (3, 1, 256, 128), (0xFFFFFFFF, 7, 1024, 0), (1, 0, 0, 2048)])
def test_generator_equals_python_integers(sim, seeds):
    want = python_integer_steps(*seeds, 40)
    assert np.array_equal(sim.steps(*seeds, 40), want)
    # ... and so does the numpy model the other tests lean on: a 16 x 40 group is 40 steps of R's rows
    visible, nonvisible, x0, y0 = seeds
    if visible < (1 << 31):
        field = N.group_field(x0, y0, 16, 40, visible, nonvisible)
        assert np.array_equal(bits(field[0]).ravel(), (want >> 9) | np.uint32(0x3F800000))


@pytest.mark.parametrize("w,h", N.KAT_SHAPES + [(70, 45)])
def test_jumped_fill_equals_sequential_fill_and_numpy(sim, w, h):
    """every clipped group shape: 128 x 128, 44 x 14 (two whole steps and a 12-float tail; 42 rows in blocks of 2), 16 x 1, 17 x 3, 1 x 1;
    45 rows: 135 rows in blocks of 5, the group's height no multiple of the 32 blocks"""
    seq = sim.fill(w, h, N.GDIM, 2, 1, jumped=0)
    jumped = sim.fill(w, h, N.GDIM, 2, 1, jumped=1)
    assert np.array_equal(bits(seq), bits(jumped))
    assert np.array_equal(bits(seq), bits(N.raw_planes(w, h, N.GDIM, 2, 1)))
    assert seq.min() >= 1.0 and seq.max() < 2.0


def test_jumped_fill_with_other_group_sizes(sim):
    for (w, h, gdim) in ((70, 40, 16), (300, 20, 256), (40, 300, 64)):
        assert np.array_equal(bits(sim.fill(w, h, gdim, jumped=0)), bits(sim.fill(w, h, gdim, jumped=1))), (w, h, gdim)
        assert np.array_equal(bits(sim.fill(w, h, gdim, jumped=0)), bits(N.raw_planes(w, h, gdim))), (w, h, gdim)


def test_strength(sim):
    """v < 0, the knots, v = 7/6 exactly, v > 7/6, and a LUT whose values interpolate past 1"""
    luts = [lut_of(LUT), np.array([0.5, 0.9, 1.4, 1.1, 0.2, 1.9, 0.0, 1.3], np.float32), np.array([0.0, -0.5, 0.3, 0, 0, 0, 0.8, -0.2], np.float32)]
    values = [-1.0, -0.0, 0.0, 1e-9, 0.1, 1.0 / 6.0, 0.25, 0.3333, 0.5, 0.99, 1.0, 1.1, np.float32(7.0) / np.float32(6.0), 1.1666666, 1.1666667, 1.17, 2.0, 1e30, float("nan")]
    for lut in luts:
        got = np.array([sim.strength(lut, v) for v in values], np.float32)
        want = N.strength(lut, np.array(values, np.float32))
        assert np.array_equal(bits(got), bits(want)), lut
        assert got.min() >= 0.0 and got.max() <= 1.0
    assert sim.strength(luts[0], -1.0) == luts[0][0] and sim.strength(luts[0], 2.0) == np.float32(luts[0][6] + (luts[0][7] - luts[0][6]) * np.float32(1.0))
    assert sim.strength(luts[1], 0.3) == 1.0            # between 0.9 and 1.4: clamped


@pytest.fixture(scope="module")
def frame_300(sim):
    """the 300 x 270 frame with 128-pixel groups: 3 x 3 groups, narrow right and bottom groups, mirror on all four edges"""
    rng = np.random.default_rng(5)
    planes = np.stack([rng.uniform(-0.03, 0.03, (N.VH, N.VW)), rng.uniform(-0.1, 1.3, (N.VH, N.VW)), rng.uniform(-0.1, 1.3, (N.VH, N.VW))]).astype(np.float32)
    padded = sim.fill_padded(N.VW, N.VH, N.GDIM, 1, 0)
    return planes, padded


@pytest.mark.parametrize("lut,ytox,ytob", [(lut_of(LUT), 0.0, 1.0), (np.array([0.5, 0.9, 1.4, 1.1, 0.2, 1.9, 0.0, 1.3], np.float32), 0.125, 0.75), (lut_of((0, 0, 0, 1023, 0, 0, 0, 0)), -1.5, 2.0)])
def test_fill_convolve_and_add_equal_numpy(sim, frame_300, lut, ytox, ytob):
    planes, padded = frame_300
    raw = padded[:, :, :N.VW]
    assert np.array_equal(bits(raw), bits(N.raw_planes(N.VW, N.VH, N.GDIM, 1, 0)))
    got = sim.add(planes, padded, lut, ytox, ytob)
    want = N.apply_noise(planes, lut, ytox, ytob, raw=raw)
    assert np.array_equal(bits(got), bits(want))
    assert not np.array_equal(got, planes)


@pytest.mark.parametrize("w,h", [(44, 14), (16, 1), (17, 3), (1, 1), (128, 64), (3, 70)])
def test_add_on_small_frames_equals_numpy(sim, w, h):
    """frames narrower or lower than the filter's reach: the mirror folds more than once"""
    rng = np.random.default_rng(w * 100 + h)
    planes = rng.uniform(-0.2, 1.3, (3, h, w)).astype(np.float32)
    padded = sim.fill_padded(w, h, N.GDIM)
    got = sim.add(planes, padded, lut_of(LUT), 0.25, 0.5)
    assert np.array_equal(bits(got), bits(N.apply_noise(planes, lut_of(LUT), 0.25, 0.5, raw=padded[:, :, :w])))


# ---------------------------------------------------------------- 3. statistics: lanes, rows or groups that repeat each other show here

def test_statistics_of_the_reference_model_and_the_jumped_fill(sim):
    """512 x 512: a convolved plane has |mean| < 0.02 and a variance within 10 % of 1.28 = (3.84^2 + 24 * 0.16^2) / 12; about 10^4
    independent 5 x 5 neighbourhoods give a standard error near 1.4 %. The numpy model first, then the jumped fill, which must be it."""
    model = N.raw_planes(512, 512, 256, 0, 0)
    conv = N.convolve(model).astype(np.float64)
    for c in range(3):
        print("plane %d: mean %.5f variance %.5f" % (c, conv[c].mean(), conv[c].var()))
        assert abs(conv[c].mean()) < 0.02
        assert abs(conv[c].var() - 1.28) < 0.128
    assert abs(model.astype(np.float64).mean() - 1.5) < 0.005 and abs(model.astype(np.float64).var() - 1.0 / 12.0) < 0.002
    jumped = sim.fill(512, 512, 256, 0, 0)
    assert np.array_equal(bits(jumped), bits(model))
    # groups, channels and seeds all differ, and so do the rows of a group and the 16-float runs of a row
    groups = [model[:, y:y + 256, x:x + 256] for y in (0, 256) for x in (0, 256)]
    for i in range(4):
        for j in range(i + 1, 4):
            assert not np.array_equal(groups[i], groups[j]) and np.abs(np.corrcoef(groups[i].ravel(), groups[j].ravel())[0, 1]) < 0.02
    for a, b in ((0, 1), (0, 2), (1, 2)):
        assert np.abs(np.corrcoef(model[a].ravel(), model[b].ravel())[0, 1]) < 0.02
    for seeds in ((1, 0), (0, 1)):
        other = sim.fill(512, 512, 256, *seeds)
        assert np.abs(np.corrcoef(other.ravel(), model.ravel())[0, 1]) < 0.02
    g = groups[0][0]
    assert np.abs(np.corrcoef(g[:-1].ravel(), g[1:].ravel())[0, 1]) < 0.02           # a row against the next
    assert np.abs(np.corrcoef(g[:, :-16].ravel(), g[:, 16:].ravel())[0, 1]) < 0.02   # a run against the next
    assert np.abs(np.corrcoef(g[:, 0::2].ravel(), g[:, 1::2].ravel())[0, 1]) < 0.02   # a lane's low half against its high half
    assert len(np.unique(bits(g))) > 0.99 * g.size * (1 - g.size / 2 ** 24)          # 23 random bits a value


# ---------------------------------------------------------------- 4. the stand-alone program

@pytest.mark.parametrize("program", ["noise_main", "noise_main_san"])
def test_stand_alone_program_plain_and_sanitised(built, program):
    """the jumped fill against the sequential one and the tiled addition against the rule, over planes in allocations of exactly
    their size (tests/hostsim/noise_main.cpp)"""
    r = subprocess.run([os.path.join(ROOT, "build", program)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    assert r.returncode == 0, r.stdout.decode()
    assert b"0 failure(s)" in r.stdout
