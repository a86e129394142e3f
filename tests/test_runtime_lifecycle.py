"""What a frame handle's device side does between decodes, which the parity tests do not reach: the timed entry point against the untimed
one, one handle carried through every owner of a block of the device memory cache (plan, working set, kept alpha, region staging, the
temporaries of decode_to_host) and back, and the two-phase block across a second upload. Every expectation is a fresh handle's result
for the same setting, or the same call once more: these tests describe the runtime as it stands."""
import ctypes as C
import os

import numpy as np
import pytest

from streams import synth, VARDCT_CASES, MODULAR_CASES

SEED = 7
SENTINEL = 0xC3
INTERIOR = (219, 235, 75, 43)   # straddles a four-group corner of 256-pixel groups: its cover is four whole groups, not the rectangle


def stream(name):
    if name in dict(VARDCT_CASES):
        return synth("vardct", 1300, 776, SEED, **dict(VARDCT_CASES)[name])
    _, W, H, opts = [c for c in MODULAR_CASES if c[0] == name][0]
    return synth("modular", W, H, SEED, **opts)


@pytest.fixture(scope="module")
def gpu(built):
    import j40_amd
    assert j40_amd.device_count() > 0, "the gpu tests need a HIP device"
    return j40_amd


def into_sentinel(fr, w, h, timed):
    """one decode through the asynchronous entry point into a padded device image full of SENTINEL; (every byte of it, status, times)"""
    import torch
    stride = (w + 3) * 4
    buf = torch.full(((h + 4) * stride,), SENTINEL, dtype=torch.uint8, device="cuda:0")
    s = torch.cuda.current_stream()
    ms = None
    if timed:
        ms = fr.decode_timed(buf.data_ptr() + 2 * stride, stride, s.cuda_stream)
    else:
        fr.decode(buf.data_ptr() + 2 * stride, stride, s.cuda_stream)
    s.synchronize()
    return buf.cpu().numpy().reshape(h + 4, stride), fr.status(), ms


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["default", "alpha_extra_channel", "multi_group"])
def test_timed_decode_equals_untimed(gpu, name):
    fr = gpu.Frame(stream(name))
    fr.upload(0)
    for rect in (None, INTERIOR):
        if rect:
            assert fr.set_region(*rect) == ""
        w, h = (rect[2], rect[3]) if rect else (fr.width, fr.height)
        plain, code, _ = into_sentinel(fr, w, h, False)
        timed, tcode, ms = into_sentinel(fr, w, h, True)
        assert code == tcode == "", (name, rect, code, tcode)
        assert np.array_equal(plain, timed), (name, rect)
        assert np.all(plain[:2] == SENTINEL) and np.all(plain[-2:] == SENTINEL) and np.all(plain[2:-2, w * 4:] == SENTINEL), (name, rect)
        assert not np.all(plain[2:-2, :w * 4] == SENTINEL), (name, rect)
        print(name, rect, "ms3 =", ms.tolist())
        assert ms.shape == (3,) and np.all(np.isfinite(ms)) and np.all(ms >= 0), (name, rect, ms)
    fr.close()


SMALL, LARGER = INTERIOR, (100, 100, 900, 500)   # covers of 2 x 2 and 4 x 3 groups, both inside the 6 x 4 of the frame


def fresh(gpu, data, alpha, rect):
    fr = gpu.Frame(data)
    if alpha is not None:
        assert fr.set_alpha(alpha) == ""
    fr.upload(0)
    if rect:
        assert fr.set_region(*rect) == ""
    err, px = fr.decode_to_host()
    assert err == "", err
    fr.close()
    return px


def cycle(gpu, data, expect):
    """one handle through every setting that makes the runtime take, grow or give back a block; each result against the fresh handle's"""
    def decode(key):
        err, px = fr.decode_to_host()
        assert err == "", (key, err)
        assert np.array_equal(px, expect[key]), key
    fr = gpu.Frame(data)
    fr.upload(0)
    decode((None, None))
    assert fr.set_alpha(1) == ""
    decode((1, None))
    assert fr.alpha()["written"] == 1
    assert fr.set_region(*SMALL) == ""
    decode((1, SMALL))
    assert fr.region()["widened"] == 1   # (the kept alpha is merged into full-size pixels: the whole frame into staging)
    assert fr.set_alpha(0) == ""
    decode((0, SMALL))
    assert fr.region()["widened"] == 0
    assert fr.set_region(*LARGER) == ""
    decode((0, LARGER))
    assert fr.clear_region() == ""
    fr.set_group_range(5, 7)
    fr.set_group_range(0, fr.info["num_groups"])
    decode((0, None))
    fr.upload(0)
    decode((0, None))
    fr.close()


def cache_mallocs(gpu):
    a = np.zeros(10, np.uint64)
    gpu.lib().j40hip_cache_counters(C.c_void_p(a.ctypes.data))
    return int(a[2] + a[3])   # slab allocations + plain allocations


@pytest.mark.gpu
def test_one_handle_through_every_owner(gpu):
    data = stream("alpha_extra_channel")
    settings = [(None, None), (1, None), (1, SMALL), (0, SMALL), (0, LARGER), (0, None)]
    expect = {k: fresh(gpu, data, *k) for k in settings}
    assert not np.array_equal(expect[(1, None)], expect[(0, None)]), "the stream's alpha channel is not opaque"
    cycle(gpu, data, expect)
    before = cache_mallocs(gpu)
    cycle(gpu, data, expect)
    if os.environ.get("J40HIP_CACHE_GB") != "0":
        assert cache_mallocs(gpu) == before, "a block of the first cycle did not go back to the cache"


@pytest.mark.gpu
def test_two_phase_block_across_uploads(gpu):
    data = synth("vardct", 2600, 2100, 71, forward=1)   # (tests/test_gpu_parity.py: the smallest stream known to take the path)
    saved = os.environ.get("J40HIP_TWO_PHASE")
    try:
        os.environ["J40HIP_TWO_PHASE"] = "1"
        fr = gpu.Frame(data, threads=4)
        fr.upload(0)
        code, px = fr.decode_to_host()
        assert fr.two_phase_sections() > 0
        fr.upload(0)
        code2, px2 = fr.decode_to_host()
        assert fr.two_phase_sections() > 0
        fr.close()
        os.environ["J40HIP_TWO_PHASE"] = "0"
        one = gpu.Frame(data, threads=4)
        one.upload(0)
        code1, px1 = one.decode_to_host()
        assert one.two_phase_sections() <= 0
        one.close()
    finally:
        os.environ.pop("J40HIP_TWO_PHASE", None)
        if saved is not None:
            os.environ["J40HIP_TWO_PHASE"] = saved
    assert code == code2 == code1 == ""
    assert np.array_equal(px, px2) and np.array_equal(px, px1)
