"""Upsampling on the host (include/j40hip.h, J40HIP_PARSE_UPSAMPLING): the switch, the parse of the custom weights and of the frame
header's upsampling fields, the coded and the shown size, what is refused, the defaults an application supplies, the expansion of a
packed table and device/upsample_dev.h's rule compiled for the CPU (j40hip_kat_host_upsample: sample by sample, and the kernel's tile
functions thread by thread), held bit for bit against numpy's float32 statement (tests/upsample_streams.py). PARITY UNPINNED: the
reference refuses all of it; tests/test_upsampling_gpu.py has the device and the anchor that reaches the reference."""
import os
import subprocess

import numpy as np
import pytest

import upsample_streams as U
from upsample_streams import up_synth, pair, bits, KAT_SHAPES
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


STREAMS = [("vardct", U.VW, U.VH), ("modular", U.MW, U.MH)]
EW, EH = 600, 540            # a VarDCT frame whose extra channels, coded twice or four times coarser, still exceed a group


@pytest.fixture(autouse=True)
def no_defaults(j40):
    """the default tables are process-wide: every test starts and ends without any"""
    for k in (2, 4, 8):
        assert j40.set_upsampling_defaults(k, None) == ""
    yield
    for k in (2, 4, 8):
        assert j40.set_upsampling_defaults(k, None) == ""


# ---------------------------------------------------------------- 1. the switch, the sizes, the weights

@pytest.mark.parametrize("mode,w,h", STREAMS)
def test_three_kinds_of_stream_need_the_switch(j40, monkeypatch, mode, w, h):
    """this is a test that fails without the feature: the keyword does not exist. A frame with upsampling, one whose extra channel has
    ec_upsampling (a VarDCT frame's alone, beside upsampling = 1: the one refusal; a Modular frame's beside the frame's own), an image
    with custom weights: "TODO" each, parsed with the switch"""
    monkeypatch.delenv("J40HIP_UPSAMPLING", raising=False)
    j40.set_upsampling_defaults(2, U.nearest_table(2))        # (the first kind carries no table)
    xyb = dict(xyb=1) if mode == "modular" else {}
    kinds = [up_synth(mode, w, h, upsampling=2, upweights="default", **xyb),
             up_synth(mode, EW, EH, upsampling=2, upweights="nearest", alpha=1, ecup=2, uptwin=1) if mode == "vardct" else up_synth(mode, w, h, upsampling=2, upweights="nearest", alpha=1, **xyb),
             up_synth(mode, w, h, upsampling=2, upweights="nearest", uptwin=2, **xyb)]
    for data in kinds:
        assert parse_code(j40, data) == "TODO"
        assert parse_code(j40, data, upsampling=True) == ""
        monkeypatch.setenv("J40HIP_UPSAMPLING", "1")
        assert parse_code(j40, data) == ""
        monkeypatch.setenv("J40HIP_UPSAMPLING", "0")
        assert parse_code(j40, data) == "TODO"
        monkeypatch.delenv("J40HIP_UPSAMPLING")
        with pytest.raises(j40.J40Error) as e:
            j40.Frame.parse_streamed(data)
        assert e.value.code == "TODO"
        j40.Frame.parse_streamed(data, flags=j40.PARSE_UPSAMPLING).close()
    # custom weights beside a frame with upsampling = 1: kept, nothing to stretch
    fr = j40.Frame(kinds[2], upsampling=True)
    assert fr.upsampling()[0] == 1 and fr.upsampling()[1].size == 0 and (fr.width, fr.height) == (w, h) == fr.coded_size()
    fr.close()
    # the plain twin never needed the switch
    twin = pair(mode, w, h, 2)[1]
    assert parse_code(j40, twin) == "" and parse_code(j40, twin, upsampling=True) == ""


@pytest.mark.parametrize("k", [2, 4, 8])
@pytest.mark.parametrize("mode,w,h", STREAMS)
def test_sizes_groups_and_weights(j40, mode, w, h, k):
    """the header's size is the shown one, everything else is sized by ceil(shown / K); the table comes back as its F16s"""
    raw = np.linspace(-0.37, 0.91, U.COUNT[k])          # (values no F16 holds)
    assert not np.array_equal(U.f16(raw), raw.astype(np.float32))
    for shown in ((k * w, k * h), U.cut_size(k, w, h)):
        data, twin = pair(mode, w, h, k, weights=raw, shown=shown)
        fr = j40.Frame(data, upsampling=True)
        tw = j40.Frame(twin)
        try:
            got_k, weights = fr.upsampling()
            assert got_k == k and np.array_equal(bits(weights), bits(U.f16(raw)))
            assert (fr.width, fr.height) == shown and fr.coded_size() == (w, h) == (-(-shown[0] // k), -(-shown[1] // k))
            assert (tw.width, tw.height) == (w, h) == tw.coded_size() and tw.upsampling()[0] == 1
            for key in ("num_groups", "num_lf_groups", "num_passes", "group_size_shift"):
                assert fr.info[key] == tw.info[key], key
            shift = fr.info["group_size_shift"]
            assert fr.info["num_groups"] == (-(-w // (1 << shift))) * (-(-h // (1 << shift)))
            # the region, the scale and the orientation speak of the shown size
            assert fr.region()["w"] == shown[0] and fr.region()["h"] == shown[1]
            assert fr.set_region(shown[0] - 5, shown[1] - 7, 5, 7) == "" and fr.set_region(shown[0] - 5, shown[1] - 7, 6, 7) == "rnge"
            assert fr.clear_region() == ""
            assert fr.set_scale(1) == "" and fr.scale()["width"] == -(-shown[0] // 2) and fr.scale()["height"] == -(-shown[1] // 2)
        finally:
            fr.close(); tw.close()


def test_usmp_updf_and_the_parse_refusals(j40):
    w, h = U.VW, U.VH
    # an extra channel coded finer than the frame: "usmp" (j40.h:3637's rule)
    assert parse_code(j40, up_synth("vardct", w, h, upsampling=4, upweights="nearest", alpha=1, ecup=2), upsampling=True) == "usmp"
    assert parse_code(j40, up_synth("vardct", w, h, upsampling=4, upweights="nearest", alpha=1, ecup=1), upsampling=True) == "usmp"
    assert parse_code(j40, up_synth("vardct", w, h, upsampling=4, upweights="nearest", alpha=1, ecup=4), upsampling=True) == ""
    # coarser, in a VarDCT frame: coded at ceil(shown / ec_upsampling) up to four times the frame's factor, "TODO" from eight times on
    assert parse_code(j40, up_synth("vardct", EW, EH, upsampling=2, upweights="nearest", alpha=1, ecup=4), upsampling=True) == ""
    assert parse_code(j40, up_synth("vardct", EW, EH, upsampling=2, upweights="nearest", alpha=1, ecup=2, uptwin=1), upsampling=True) == ""
    assert parse_code(j40, up_synth("vardct", EW, EH, upsampling=2, upweights="nearest", alpha=1, ecup=8, uptwin=1), upsampling=True) == "TODO"
    # ... in a Modular frame, whose alpha plane is rendered: "TODO"
    assert parse_code(j40, up_synth("modular", U.MW, U.MH, xyb=1, upsampling=2, upweights="nearest", alpha=1, ecup=4), upsampling=True) == "TODO"
    # an image with xyb_encoded = 0 that is no YCbCr frame: "TODO", like noise; a YCbCr frame parses (the route refuses its plan)
    assert parse_code(j40, up_synth("vardct", w, h, upsampling=2, upweights="nearest", noxyb=1, fullheader=1), upsampling=True) == "TODO"
    assert parse_code(j40, up_synth("vardct", w, h, upsampling=2, upweights="nearest", noxyb=1, fullheader=1, uptwin=1), upsampling=True) == ""
    assert parse_code(j40, up_synth("vardct", 304, 272, upsampling=2, upweights="nearest", ycbcr=1), upsampling=True, ycbcr=True) == ""
    # no table for the frame's K anywhere: "updf" until the application supplies one
    data = up_synth("vardct", w, h, upsampling=8, upweights="default")
    assert parse_code(j40, data, upsampling=True) == "updf"
    assert j40.set_upsampling_defaults(8, U.nearest_table(8)) == "" and parse_code(j40, data, upsampling=True) == ""
    assert j40.set_upsampling_defaults(8, None) == "" and parse_code(j40, data, upsampling=True) == "updf"
    # an LF-only parse
    assert parse_code(j40, pair("vardct", w, h, 2)[0], upsampling=True, lf_only=True) == "TODO"
    assert parse_code(j40, pair("vardct", w, h, 2)[1], upsampling=True, lf_only=True) == ""
    # a sequence's flag reads the image's weights; its frames with upsampling stay "TODO"
    with pytest.raises(j40.J40Error) as e:
        j40.Sequence(pair("vardct", w, h, 2)[0], flags=j40.PARSE_UPSAMPLING)
    assert e.value.code == "TODO"
    # (the frame's twin is a one-frame stream: not a sequence, whatever the flag)
    with pytest.raises(j40.J40Error) as e:
        j40.Sequence(pair("vardct", w, h, 2)[1], flags=j40.PARSE_UPSAMPLING)
    assert e.value.code == "Usq?"


def test_defaults_come_from_the_application(j40):
    """nothing here holds the standard's tables: set_upsampling_defaults supplies them, a frame copies its K's at parse"""
    data = up_synth("modular", U.MW, U.MH, xyb=1, upsampling=4, upweights="default")
    assert j40.set_upsampling_defaults(4, np.zeros(15)) == "rnge" and j40.set_upsampling_defaults(3, np.zeros(15)) == "rnge"
    first = U.distinct_table(4)
    assert j40.set_upsampling_defaults(4, first) == ""
    fr = j40.Frame(data, upsampling=True)
    assert fr.upsampling()[0] == 4 and np.array_equal(fr.upsampling()[1], first)
    assert j40.set_upsampling_defaults(4, first * 2) == ""
    assert np.array_equal(fr.upsampling()[1], first)          # (copied at parse)
    fr.close()
    fr = j40.Frame(data, upsampling=True)
    assert np.array_equal(fr.upsampling()[1], first * 2)
    fr.close()
    # the stream's own table for its K wins
    fr = j40.Frame(pair("modular", U.MW, U.MH, 4)[0], upsampling=True)
    assert np.array_equal(fr.upsampling()[1], U.nearest_table(4))
    fr.close()


def test_host_side_route_refusals(j40):
    """what needs no device to refuse: kept alpha (the group range, the batch and the rest need an upload: tests/test_upsampling_gpu.py)"""
    data = pair("vardct", U.VW, U.VH, 2, alpha=1)[0]
    fr = j40.Frame(data, upsampling=True)
    try:
        assert fr.set_alpha(1) == "TODO" and fr.set_alpha(0) == ""
    finally:
        fr.close()
    fr = j40.Frame(pair("vardct", U.VW, U.VH, 2, alpha=1)[1], upsampling=True)
    try:
        assert fr.set_alpha(1) == ""
    finally:
        fr.close()


# ---------------------------------------------------------------- 2. the table and the rule on the CPU

@pytest.mark.parametrize("k", [2, 4, 8])
def test_expanded_table_equals_numpy(j40, k):
    """distinct values: a transposed or flipped index shows"""
    w = U.distinct_table(k)
    code, got = j40.kat_upsampling_kernel(k, w)
    assert code == "" and np.array_equal(bits(got), bits(U.expand(k, w)))
    assert len(np.unique(got)) == U.COUNT[k]
    # mirrored phases are mirrored kernels; the first phase's first row is the packed table's first entries
    assert np.array_equal(got[k - 1, k - 1], got[0, 0, ::-1, ::-1]) and np.array_equal(got[0, k - 1], got[0, 0, :, ::-1])
    assert np.array_equal(got[0, 0, 0], w[:5])
    assert j40.kat_upsampling_kernel(3, w)[0] == "rnge" and j40.kat_upsampling_kernel(k, w[:-1])[0] == "rnge"
    # nearest: every phase takes the centre sample alone
    code, near = j40.kat_upsampling_kernel(k, U.nearest_table(k))
    want = np.zeros((5, 5), np.float32); want[2, 2] = 1
    assert code == "" and all(np.array_equal(near[oy, ox], want) for oy in range(k) for ox in range(k))


@pytest.mark.parametrize("k", [2, 4, 8])
def test_cpu_build_equals_numpy(j40, k):
    """upsample_sample and the tile functions over the known-answer shapes, whole and cut; the clamp neither vanishes nor swallows
    the stencil: numpy itself finds between 1 % and 50 % of the outputs clamped, over all shapes together and in every shape of more
    than one tile"""
    weights = U.centre_heavy(k)
    total = clamped = 0
    for (w, h) in KAT_SHAPES:
        planes = U.kat_planes(w, h)
        want, c = U.upsample(planes, k, weights, want_clamped=True)
        total += want.size; clamped += c
        print("K = %d, %d x %d: %.1f %% clamped" % (k, w, h, 100.0 * c / want.size))
        if w * h > 32 * 8:
            assert 0.01 <= c / want.size <= 0.5
        ow, oh = U.cut_size(k, w, h)
        for tiled in (False, True):
            code, got = j40.kat_host_upsample(planes, k, weights, tiled=tiled)
            assert code == "" and np.array_equal(bits(got), bits(want)), (w, h, tiled)
            code, got = j40.kat_host_upsample(planes, k, weights, ow, oh, tiled=tiled)
            assert code == "" and got.shape == (3, oh, ow) and np.array_equal(bits(got), bits(want[:, :oh, :ow])), (w, h, tiled)
    assert 0.01 <= clamped / total <= 0.5
    assert j40.kat_host_upsample(U.kat_planes(5, 5), k, weights, 5 * k + 1, 5 * k)[0] == "rnge"


def test_nearest_is_repeat_and_flat_stays_flat(j40):
    planes = U.kat_planes(33, 9)
    for k in (2, 4, 8):
        code, got = j40.kat_host_upsample(planes, k, U.nearest_table(k), tiled=True)
        assert code == "" and np.array_equal(bits(got), bits(np.repeat(np.repeat(planes, k, axis=1), k, axis=2)))
        flat = np.full((3, 9, 33), 0.3217, np.float32)
        code, got = j40.kat_host_upsample(flat, k, U.centre_heavy(k), tiled=True)
        assert code == "" and np.array_equal(bits(got), bits(np.full((3, 9 * k, 33 * k), 0.3217, np.float32)))


# ---------------------------------------------------------------- 3. the stand-alone program

@pytest.mark.parametrize("program", ["upsample_main", "upsample_main_san"])
def test_stand_alone_program_plain_and_sanitised(built, program):
    """the tile functions against the rule over planes in allocations of exactly their size (tests/hostsim/upsample_main.cpp)"""
    r = subprocess.run([os.path.join(ROOT, "build", program)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    assert r.returncode == 0, r.stdout.decode()
    assert b"0 failure(s)" in r.stdout
