"""LF frames on the host (include/j40hip.h, J40HIP_SEQ_LFFRAME): the index over a stream whose LF image is a frame of its own, what
stays refused, the parse of the frame with use_lf_frame, and device/lf_frame_dev.h -- the functions k_lf_from_frame and k_lf_frame_bctx
run -- compiled for the CPU (tests/hostsim/lf_frame_sim.cpp) against numpy and against the plan of the twin stream.
tests/test_lf_frames_gpu.py has the decodes."""
import ctypes as C
import os

import numpy as np
import pytest

from lf_streams import WIDE, TALL, TWO_LEVELS, lf_stream, lf_twin, lf_stats, lf_size, without_first_frame

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib(built):
    import j40_amd
    return j40_amd


@pytest.fixture(scope="module")
def sim(built):
    s = C.CDLL(os.path.join(ROOT, "build", "libhostsim_lfframe.so"))
    s.lfsim_gather.restype = C.c_int64
    s.lfsim_gather.argtypes = [C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64]
    s.lfsim_twin_check.restype = C.c_uint32
    s.lfsim_twin_check.argtypes = [C.c_char_p, C.c_size_t, C.c_int32, C.c_char_p, C.c_size_t, C.c_void_p]
    return s


def rows_of(seq):
    return [dict(seq.frame_info(k), **seq.frame_lf(k)) for k in range(seq.num_frames)]


def refusal(fn):
    import j40_amd
    with pytest.raises(j40_amd.J40Error) as e:
        fn()
    return e.value.code


@pytest.mark.parametrize("size", [WIDE, TALL], ids=["2060x70", "70x2060"])
def test_index_one_level(lib, size):
    seq = lib.Sequence(lf_stream(size), lf_frames=True)
    rows = rows_of(seq)
    assert seq.num_frames == 2 and seq.num_shown == 1
    lf, main = rows
    assert (lf["type"], lf["w"], lf["h"]) == (1,) + lf_size(size) and (lf["x0"], lf["y0"]) == (0, 0)
    assert (lf["lf_level"], lf["use_lf_frame"], lf["lf_src"]) == (1, 0, -1)
    assert not lf["shown"] and not lf["saved"] and not lf["is_last"] and lf["code"] == ""
    assert (main["type"], main["w"], main["h"]) == (0,) + size and main["shown"] and main["is_last"] and main["code"] == ""
    assert (main["lf_level"], main["use_lf_frame"], main["lf_src"]) == (0, 1, 0)
    # every row is an ordinary frame handle of its own size
    for k, r in enumerate(rows):
        fr = seq.frame(k)
        assert (fr.width, fr.height) == (r["w"], r["h"])
    assert seq.frame_lf(2) == {"lf_level": 0, "use_lf_frame": 0, "lf_src": 0}   # (out of range: zeros)
    seq.close()


def test_index_two_levels(lib):
    seq = lib.Sequence(lf_stream(TWO_LEVELS, lflevels=2), lf_frames=True)
    rows = rows_of(seq)
    assert seq.num_frames == 3 and seq.num_shown == 1
    assert [(r["type"], r["w"], r["h"]) for r in rows] == [(1,) + lf_size(TWO_LEVELS, 2), (1,) + lf_size(TWO_LEVELS, 1), (0,) + TWO_LEVELS]
    assert lf_size(TWO_LEVELS, 2) == (257, 2) and lf_size(TWO_LEVELS, 1) == (2050, 9)
    assert [(r["lf_level"], r["use_lf_frame"], r["lf_src"]) for r in rows] == [(2, 0, -1), (1, 1, 0), (0, 1, 1)]
    assert [bool(r["shown"]) for r in rows] == [False, False, True] and not any(r["saved"] for r in rows)
    for k in range(3):
        seq.frame(k)
    seq.close()


def test_refused_without_the_switch(lib, monkeypatch):
    monkeypatch.delenv("J40HIP_LFFRAME", raising=False)
    data = lf_stream(WIDE)
    assert refusal(lambda: lib.Sequence(data)) == "TODO"
    assert refusal(lambda: lib.Frame(data)) == "TODO"   # (a stand-alone parse stays what it was, switch or not)
    monkeypatch.setenv("J40HIP_LFFRAME", "1")
    assert refusal(lambda: lib.Frame(data)) == "TODO"
    seq = lib.Sequence(data)                            # (the variable is the flag)
    assert seq.num_frames == 2 and seq.frame_lf(1)["use_lf_frame"] == 1
    seq.close()


def test_missing_and_missized_lf_frame(lib):
    # the LF frame cut out: the frame with use_lf_frame is the stream's first, nothing is in its slot
    data = lf_stream(WIDE)
    assert refusal(lambda: lib.Sequence(without_first_frame(lib, data), lf_frames=True)) == "lfno"
    # two levels, the level-2 frame cut out: the level-1 frame finds slot 1 empty; it ends the index
    two = lf_stream(TWO_LEVELS, lflevels=2)
    assert refusal(lambda: lib.Sequence(without_first_frame(lib, two), lf_frames=True)) == "lfno"
    # a main frame that is a crop: the LF frame, sized by the image, is not ceil(w / 8) x ceil(h / 8) of it
    seq = lib.Sequence(lf_stream(WIDE, lfcrop="1000,70"), lf_frames=True)
    assert [seq.frame_info(k)["code"] for k in range(seq.num_frames)] == ["", "lfsz"]
    assert seq.num_shown == 0
    seq.close()


def test_refused_with_the_switch(lib):
    # an image that is not XYB encoded
    assert refusal(lambda: lib.Sequence(lf_stream(WIDE, noxyb=1, alpha=1), lf_frames=True)) == "TODO"
    # an image with extra channels: its LF frame has them too, behind its coefficients. Refused when the index is built, not at playback
    assert refusal(lambda: lib.Sequence(lf_stream(WIDE, alpha=1), lf_frames=True)) == "TODO"
    # a Modular LF frame: the LF frame's header with its is_modular bit set (bit 3 of its first byte: all_default, type (2), is_modular).
    # Whatever the bits behind it then read as, the frame is refused before anything of it is decoded
    data = bytearray(lf_stream(WIDE))
    seq = lib.Sequence(bytes(data), lf_frames=True)
    at = seq.frame_info(0)["offset"]
    seq.close()
    assert data[at] & 0x0f == 0x02   # !all_default, type 1, VarDCT
    data[at] |= 0x08
    assert refusal(lambda: lib.Sequence(bytes(data), lf_frames=True)) == "TODO"


def numpy_gather(src, W, H, thr):
    """the LF planes in the plan's cell layout (LfGroups of 2048 x 2048 pixels row by row, each one's cells row by row) and the LF index
    of every cell: thresholds counted per channel (X, Y, B), combined ((x * (nB + 1)) + b) * (nY + 1) + y -- frame.cpp's order"""
    out, idx = [[], [], []], []
    for gy in range(0, H, 2048):
        for gx in range(0, W, 2048):
            w8, h8 = (min(2048, W - gx) + 7) // 8, (min(2048, H - gy) + 7) // 8
            blk = src[:, gy // 8:gy // 8 + h8, gx // 8:gx // 8 + w8]
            for c in range(3):
                out[c].append(blk[c].reshape(-1))
            cnt = [sum((blk[c] > np.float32(t)).astype(np.int64) for t in thr[c]) if len(thr[c]) else np.zeros(blk[c].shape, np.int64) for c in range(3)]
            idx.append((((cnt[0] * (len(thr[0]) + 1) + cnt[2]) * (len(thr[2]) + 1) + cnt[1]) & 255).reshape(-1))   # (8-bit arithmetic)
    return np.stack([np.concatenate(o) for o in out]), np.concatenate(idx).astype(np.uint8)


@pytest.mark.parametrize("W,H", [(2060, 70), (70, 2060), (4100, 2052)], ids=["2x1", "1x2", "3x2"])
@pytest.mark.parametrize("thr", [([], [], []), ([0.25], [], []), ([-0.1, 0.3], [0.1, 0.5, 0.9], [0.4])], ids=["none", "one", "several"])
def test_gather_against_numpy(sim, W, H, thr):
    w8, h8 = (W + 7) // 8, (H + 7) // 8
    rng = np.random.default_rng(W * 31 + H)
    src = rng.random((3, h8, w8), dtype=np.float32)
    for c in range(3):   # samples that sit on a threshold: > is strict
        for t in thr[c]:
            src[c].reshape(-1)[rng.integers(0, w8 * h8, 50)] = np.float32(t)
    nb = np.array([len(t) for t in thr], np.int32)
    tv = np.zeros((3, 15), np.float32)
    for c in range(3):
        tv[c, :len(thr[c])] = thr[c]
    cells = w8 * h8
    out, idx = np.full((3, cells), -1.0, np.float32), np.full(cells, 255, np.uint8)
    n = sim.lfsim_gather(W, H, src.ctypes.data, nb.ctypes.data, tv.ctypes.data, out.ctypes.data, idx.ctypes.data, cells)
    assert n == cells
    want, want_idx = numpy_gather(src, W, H, thr)
    assert np.array_equal(out.view(np.uint32), want.view(np.uint32))
    assert np.array_equal(idx, want_idx)
    if any(len(t) for t in thr):
        assert len(np.unique(idx)) > 1


TWIN_CASES = [("default", WIDE, dict()), ("bctx", WIDE, dict(bctx=1)), ("bctx_tall_two_passes", TALL, dict(bctx=1, passes=2)), ("two_levels_bctx", TWO_LEVELS, dict(lflevels=2, bctx=1))]


@pytest.mark.parametrize("name,size,opts", TWIN_CASES, ids=[c[0] for c in TWIN_CASES])
def test_main_frame_against_its_twin(sim, name, size, opts):
    """The frame with use_lf_frame parses to the twin's varblocks, quantisation-field indices, chroma-from-luma maps and sharpness; the
    samples (float) q * mult_lf of the flat LF frame gather to exactly the twin's dequantised LF, their LF indices are the twin's
    (rule: sample > (float) t * mult_lf; for |q| < 2^15 the product of two floats keeps q > t), and the block contexts looked up
    again with them are the twin's plan's"""
    data, twin = lf_stream(size, **opts), lf_twin(size, **opts)
    out = np.zeros(6, np.int64)
    code = sim.lfsim_twin_check(data, len(data), opts.get("lflevels", 1), twin, len(twin), out.ctypes.data)
    assert code == 0, code.to_bytes(4, "big")
    mismatched_parse, mismatched_index, distinct, mismatched_ctx, changed, mismatched_sample = out.tolist()
    print(name, "distinct LF indices", distinct, "blocks whose contexts changed", changed)
    assert mismatched_parse == 0 and mismatched_sample == 0 and mismatched_index == 0 and mismatched_ctx == 0
    if opts.get("bctx"):
        # the case is there for the thresholds: some split the cells, and the second look-up has work to do
        assert distinct > 1 and changed > 0
        assert lf_stats(size, **opts)["lfidx_distinct"] == distinct
    else:
        assert distinct == 1 and changed == 0
