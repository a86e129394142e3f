"""Reduced-size decode (j40hip_frame_set_scale, include/j40hip.h), without a device.

The 1:2 and 1:4 images are defined as a function of the full decode: sample c of output pixel (i, j) is (S + n // 2) // n over its
cell, clipped at the right and bottom edges. box() below restates that in a dozen lines of numpy and is the oracle of every test here
and in tests/test_scale_gpu.py. Here: the arithmetic every kernel uses (device/scale_dev.h) compiled for the CPU by
build/libhostsim_scale.so (tests/hostsim/scale_sim.cpp) -- every cell size, both formats, the accumulators' fields and the rounding at
their limits --, the same as a stand-alone program plain and under the host sanitizers, and the setter's rules on parsed frames.
(j40hip_frame_set_group_range needs an uploaded frame: its half of the mutual exclusion is in tests/test_scale_gpu.py.)"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from streams import synth, ROOT

U8X4, U16X4 = 0x0F33, 0x0F35
SEED = 7


def box(full, k):
    """the definition: full [H, W, 4] uint8 or uint16 -> [ceil(H / s), ceil(W / s), 4] of the same dtype"""
    s = 1 << k
    H, W = full.shape[:2]
    oh, ow = (H + s - 1) >> k, (W + s - 1) >> k
    S = np.zeros((oh, ow, 4), np.int64)
    n = np.zeros((oh, ow, 1), np.int64)
    for dy in range(s):
        for dx in range(s):
            part = full[dy::s, dx::s].astype(np.int64)     # the cells' sample (dy, dx), where the frame has it
            S[:part.shape[0], :part.shape[1]] += part
            n[:part.shape[0], :part.shape[1]] += 1
    return ((S + n // 2) // n).astype(full.dtype)


@pytest.fixture(scope="module")
def sim(built):
    L = C.CDLL(os.path.join(ROOT, "build", "libhostsim_scale.so"))
    L.scale_sim.restype = None
    L.scale_sim.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32]
    L.scale_sim_cell.restype = None
    L.scale_sim_cell.argtypes = [C.c_int32] * 5 + [C.c_void_p]
    return L


def run_sim(L, full, k, lanes=5, pad=24):
    """the CPU build of k_downscale's row function over `full`; the output's rows carry `pad` guard bytes that must stay 0xA5"""
    H, W = full.shape[:2]
    pb = 4 * full.dtype.itemsize
    s = 1 << k
    oh, ow = (H + s - 1) >> k, (W + s - 1) >> k
    stride = ow * pb + pad
    out = np.full((oh, stride), 0xA5, np.uint8)
    src = np.ascontiguousarray(full)
    L.scale_sim(out.ctypes.data, stride, src.ctypes.data, W * pb, W, H, k, pb, lanes)
    assert (out[:, ow * pb:] == 0xA5).all(), "bytes behind the rows' pixels were written"
    return np.ascontiguousarray(out[:, :ow * pb]).view(full.dtype).reshape(oh, ow, 4)


def test_box_is_the_definition():
    """box() against the definition spelt out sample by sample, on a size with every kind of edge cell"""
    rng = np.random.default_rng(1)
    full = rng.integers(0, 256, (7, 11, 4), dtype=np.uint8)
    for k in (1, 2):
        s = 1 << k
        got = box(full, k)
        for j in range(got.shape[0]):
            for i in range(got.shape[1]):
                cell = full[j * s:min(7, (j + 1) * s), i * s:min(11, (i + 1) * s)].reshape(-1, 4).astype(np.int64)
                n = cell.shape[0]
                assert np.array_equal(got[j, i], (cell.sum(0) + n // 2) // n)


@pytest.mark.parametrize("dtype", [np.uint8, np.uint16], ids=["u8x4", "u16x4"])
@pytest.mark.parametrize("k", [1, 2])
def test_every_small_size(sim, k, dtype):
    """1..9 x 1..9: every n in {1, 2, 3, 4, 6, 8, 9, 12, 16} occurs"""
    rng = np.random.default_rng(100 * k + np.dtype(dtype).itemsize)
    top = np.iinfo(dtype).max
    seen = set()
    out3 = (C.c_int32 * 3)()
    for h in range(1, 10):
        for w in range(1, 10):
            full = rng.integers(0, top + 1, (h, w, 4)).astype(dtype)
            assert np.array_equal(run_sim(sim, full, k), box(full, k)), (w, h)
            for j in range((h + (1 << k) - 1) >> k):
                for i in range((w + (1 << k) - 1) >> k):
                    sim.scale_sim_cell(w, h, k, i, j, out3)
                    assert (out3[0], out3[1]) == ((w + (1 << k) - 1) >> k, (h + (1 << k) - 1) >> k)
                    seen.add(out3[2])
    assert seen == ({1, 2, 4} if k == 1 else {1, 2, 3, 4, 6, 8, 9, 12, 16})


@pytest.mark.parametrize("dtype", [np.uint8, np.uint16], ids=["u8x4", "u16x4"])
@pytest.mark.parametrize("k", [1, 2])
@pytest.mark.parametrize("w,h", [(61, 43), (64, 64)])
def test_random_and_extreme_images(sim, w, h, k, dtype):
    rng = np.random.default_rng(w * h + k)
    top = np.iinfo(dtype).max
    yy, xx = np.mgrid[0:h, 0:w]
    alternating = np.where(((yy + xx) & 1)[..., None].repeat(4, 2) == 1, top, 0).astype(dtype)
    columns = np.where((xx & 1)[..., None].repeat(4, 2) == 1, top, 0).astype(dtype)     # cells whose means round at .5
    for name, full in [("random", rng.integers(0, top + 1, (h, w, 4)).astype(dtype)), ("zeros", np.zeros((h, w, 4), dtype)),
                       ("top", np.full((h, w, 4), top, dtype)), ("alternating", alternating), ("columns", columns)]:
        for lanes in (1, 7, 64):
            assert np.array_equal(run_sim(sim, full, k, lanes), box(full, k)), (name, lanes)
    assert (box(np.full((h, w, 4), top, dtype), k) == top).all()   # the fields hold 16 full-scale samples


@pytest.mark.parametrize("program", ["scale_main", "scale_main_san"])
def test_stand_alone_program_plain_and_sanitised(built, program):
    """the same row function outside Python over the odd sizes, source and output in blocks of exactly their size; the second build
    under -fsanitize=address,undefined"""
    r = subprocess.run([os.path.join(ROOT, "build", program)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    assert " 0 mismatches, 0 guard bytes damaged" in r.stdout and "scale_main: 1328 cases" in r.stdout, r.stdout


# ---------------------------------------------------------------- the setter's rules, on parsed frames

@pytest.mark.parametrize("mode,w,h", [("vardct", 777, 523), ("modular", 601, 303)])
def test_set_scale_and_sizes(built, mode, w, h):
    import j40_amd
    fr = j40_amd.Frame(synth(mode, w, h, SEED))
    assert fr.scale() == dict(shift=0, width=w, height=h, staged=-1, staging_bytes=0)
    for k in (1, 2, 0):
        assert fr.set_scale(k) == ""
        s = 1 << k
        assert fr.scale() == dict(shift=k, width=-(-w // s), height=-(-h // s), staged=-1, staging_bytes=0)
    assert fr.set_scale(2) == ""
    for bad in (-1, 3, 2 ** 31 - 1):
        assert fr.set_scale(bad) == "rnge"
        assert fr.scale()["shift"] == 2, "a refused call leaves the frame as it was"
    fr.close()


@pytest.mark.parametrize("mode,w,h", [("vardct", 777, 523), ("modular", 601, 303)])
def test_region_and_scale_exclude_each_other(built, mode, w, h):
    import j40_amd
    fr = j40_amd.Frame(synth(mode, w, h, SEED))
    assert fr.set_region(8, 8, 100, 50) == ""
    assert fr.set_scale(1) == "Usc?" and fr.scale()["shift"] == 0
    assert fr.set_scale(0) == ""                     # shift 0 always succeeds
    assert fr.clear_region() == "" and fr.set_scale(1) == ""
    assert fr.set_region(8, 8, 100, 50) == "Usc?" and not fr.region()["set"]
    assert fr.set_region(0, 0, w, h) == "" and fr.clear_region() == ""   # clearing a region is no region
    assert fr.set_region(8, 8, 100, 5000) == "rnge"
    assert fr.set_scale(0) == "" and fr.set_region(8, 8, 100, 50) == ""
    fr.close()


def test_lf_only_and_sequence_frames_are_refused(built):
    import j40_amd
    fr = j40_amd.Frame(synth("vardct", 777, 523, SEED), lf_only=True)
    assert fr.set_scale(1) == "Ulf?" and fr.set_scale(2) == "Ulf?" and fr.set_scale(3) == "rnge"
    assert fr.set_scale(0) == "" and fr.scale()["shift"] == 0
    fr.close()
    seq = j40_amd.Sequence(synth("vardct", 300, 200, SEED, passes=2, frames=2, crops=";37,21,130,90"))
    for k in range(2):
        f = seq.frame(k)
        assert f.set_scale(1) == "Usc?" and f.set_scale(0) == "" and f.scale()["shift"] == 0
    seq.close()
