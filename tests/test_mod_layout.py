"""The layout of a Modular plan's memory (j40_amd/csrc/mod_layout.hpp: ModPlanLayout), checked on the CPU.

The runtime lays out three kinds of block with it: a Modular frame (runtime_upload.hip: upload_modular), and in runtime.hip the
extra-channel sub-images of a VarDCT frame in drop mode (validate_trailers) and in keep mode (keep_alpha). tests/hostsim lays out the same three blocks in host memory
(mod_block.hpp): exactly total_bytes from malloc, 64 guard bytes behind every region, the scratch regions and the guards filled
with 0x5a. A region the layout sizes too small therefore shows here as a damaged guard, or -- in build/mod_layout_main_san, the
same decodes as a program of its own under the address and undefined-behaviour sanitizers -- as a report at the byte it happens.

What the decodes give is pinned twice: by the tests that hold hostsim against the reference (test_hostsim.py, test_alpha.py,
test_squeeze.py, unchanged), and here by the digests of what the same entry points returned before they shared the layout."""
import ctypes as C
import hashlib
import os
import subprocess

import numpy as np
import pytest

from streams import synth, ROOT

SEED = 7
U8X4 = 0x0F33

# (name, width, height, generator options, sha256 of hostsim_decode's pixels before the layout was shared)
MODULAR = [
    # sub-planes, local_rct, the weighted predictor's rows
    ("local_palette_beside_local_rct_local_tree", 300, 200, dict(localpalette=1, localrct=5, localtree=2, groupshift=7),
     "5aac7e9426a81e8b6a95c91b5cb751ecea77d0a2f154a417744a11e0c9c2189b"),
    # LZ77 windows, the weighted predictor in local trees only, alpha
    ("local_tree_wp_prefix_lz77_alpha", 600, 300, dict(localtree=2, prefix=1, lz77=1, alpha=1),
     "fa1cf77d651a7860d0d1d63fe572b8c43da6d05e535b5652b50ae26a5752842c"),
    # a position-only tree: sections decoded in two passes (residuals, split_state)
    ("coarse_leaves_position_tree_prefix_lz77", 300, 200, dict(tree=6, bpp=14, prefix=1, lz77=1, lzmode="special", noise=3000),
     "d3649ae91331edf9847d4aa91e974c38acf158af833b8b37a6a1fb0907869455"),
    ("four_extra_channels_alpha_last", 600, 300, dict(extra=3, alpha=1, tree=3, localrct=7),
     "c6d6eb93b3cc16b710b144d7c6740929f3499a9a04295f2dfdf382f82e8b62ed"),
    # Squeeze: channels of different sizes (chan_rects); six groups
    ("squeeze_six_groups", 600, 300, dict(squeeze=1),
     "d915cbe9a4f0e7ae2f6f785cab076ae08b9b0630718abe5b12543809dc7a9776"),
]
# VarDCT frames with extra channels, from tests/test_alpha.py's STREAMS:
# (name, width, height, options, sha256 of hostsim_decode's pixels, sha256 of alpha_sim_decode's merge over pixels of all 255)
VARDCT = [
    ("two_depth_channels_ahead", 600, 300, dict(alpha=1, extra=2),
     "dfaac1b1a1a675bd60fd6dd013146cb834b33a773d59ba580626bea064c35bf7", "6b903b8b5622dc4b714430b97b61b11a37cf6df8f4a1f7de6586539094acf0ad"),
    ("wp_in_both_headers", 600, 300, dict(alpha=1, lftree=4, wp="random", wpat="both", dq=2),
     "4e74d8559057fa81517da2583256df4a98a6cdbca10b135ffaf2dbb3a1087689", "6b903b8b5622dc4b714430b97b61b11a37cf6df8f4a1f7de6586539094acf0ad"),
    ("global_code_lz77_prefix", 600, 300, dict(alpha=1, extra=1, glz77=1, gprefix=1),
     "dfaac1b1a1a675bd60fd6dd013146cb834b33a773d59ba580626bea064c35bf7", "6b903b8b5622dc4b714430b97b61b11a37cf6df8f4a1f7de6586539094acf0ad"),
    ("hfprefix_257x200", 257, 200, dict(alpha=1, hfprefix=1),
     "423da6445b15bf8be51ec6135d16c0b4a3c5034ac014e94409b8efbfdb96e155", "89b81be0b435f6b434d44f4ebb6fd2556dcdc5c6ed0eccaa99efd693c5ced266"),
]
# the regions only some plans have (ModPlanLayout's names); "plane" in a keep-mode block: the frame-wide planes
OPTIONAL = ["coop_trees", "local_rct", "chan_rects", "sub_plane", "wp_scratch", "lz_window", "residuals", "split_state"]


def sha(a):
    return hashlib.sha256(a.tobytes()).hexdigest()


@pytest.fixture(scope="module")
def sims(built):
    S = C.CDLL(os.path.join(ROOT, "build", "libhostsim.so"))
    S.hostsim_decode.restype = C.c_uint32
    S.hostsim_decode.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_int]
    A = C.CDLL(os.path.join(ROOT, "build", "libhostsim_alpha.so"))
    A.alpha_sim_decode.restype = C.c_uint32
    A.alpha_sim_decode.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_int32]
    for L, prefix in ((S, "hostsim"), (A, "alpha_sim")):
        getattr(L, prefix + "_guard_damage").restype = C.c_int64
        getattr(L, prefix + "_region_bytes").restype = C.c_int64
        getattr(L, prefix + "_region_bytes").argtypes = [C.c_char_p]
    return S, A


def cpu_modular(sims, case):
    """(pixels, guard bytes damaged, {region name: bytes}) of hostsim_decode"""
    S, _ = sims
    _, w, h, opts = case[:4]
    data = synth("modular" if case in MODULAR else "vardct", w, h, SEED, **opts)
    out = np.zeros((h, w, 4), np.uint8)
    assert S.hostsim_decode(data, len(data), out.ctypes.data, None, 0) == 0
    return out, S.hostsim_guard_damage(), {n: S.hostsim_region_bytes(n.encode()) for n in OPTIONAL + ["plane"]}


def cpu_keep(sims, case, given):
    """alpha_sim_decode's merge over a copy of `given`"""
    _, A = sims
    _, w, h, opts = case[:4]
    data = synth("vardct", w, h, SEED, **opts)
    out = np.ascontiguousarray(given).copy()
    assert A.alpha_sim_decode(data, len(data), out.ctypes.data, w * 4, U8X4) == 0
    return out, A.alpha_sim_guard_damage(), {n: A.alpha_sim_region_bytes(n.encode()) for n in OPTIONAL + ["plane"]}


@pytest.fixture(scope="module")
def cpu(sims):
    """every CPU decode once, shared by the tests below: name -> (pixels, damaged guard bytes, region sizes); VarDCT frames under
    name + ":drop" and name + ":keep" (the merge over pixels of all 255)"""
    got = {}
    for case in MODULAR:
        got[case[0]] = cpu_modular(sims, case)
    for case in VARDCT:
        got[case[0] + ":drop"] = cpu_modular(sims, case)
        got[case[0] + ":keep"] = cpu_keep(sims, case, np.full((case[2], case[1], 4), 255, np.uint8))
    return got


def test_cpu_decodes_are_what_they_were_and_leave_the_guards(cpu):
    for case in MODULAR:
        px, damage, _ = cpu[case[0]]
        assert sha(px) == case[4], case[0]
        assert damage == 0, case[0]
    for case in VARDCT:
        for mode, digest in ((":drop", case[4]), (":keep", case[5])):
            px, damage, _ = cpu[case[0] + mode]
            assert sha(px) == digest, (case[0], mode)
            assert damage == 0, (case[0], mode)


def test_every_optional_region_exists_in_some_stream(cpu):
    """or the guards above say nothing about it"""
    for name in OPTIONAL:
        assert any(sizes[name] > 0 for _, _, sizes in cpu.values()), name
    assert all(cpu[case[0] + ":keep"][2]["plane"] >= 2 * case[1] * case[2] for case in VARDCT), "keep mode: frame-wide planes"
    assert all(cpu[case[0] + ":drop"][2]["plane"] == 0 and cpu[case[0] + ":drop"][2]["sub_plane"] > 0 for case in VARDCT), "drop mode: sub-planes only"


@pytest.mark.parametrize("program", ["mod_layout_main", "mod_layout_main_san"])
def test_stand_alone_program_plain_and_sanitised(built, tmp_path, program):
    """the same three decodes outside Python, each plan in a block of exactly total_bytes from malloc; the second build under
    -fsanitize=address,undefined"""
    paths = []
    for case in MODULAR + VARDCT:
        path = str(tmp_path / (case[0] + ".jxl"))
        with open(path, "wb") as fp:
            fp.write(synth("modular" if case in MODULAR else "vardct", case[1], case[2], SEED, **case[3]))
        paths.append(path)
    r = subprocess.run([os.path.join(ROOT, "build", program)] + paths, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    assert r.stdout.count(" decode 00000000, 0 guard bytes damaged") == len(MODULAR) + 2 * len(VARDCT), r.stdout


@pytest.mark.gpu
def test_gpu_blocks_decode_twice_and_equal_the_cpu(built, cpu, sims):
    """Every frame uploaded once and decoded twice per mode: both decodes equal byte for byte, status "". A Modular frame's pixels
    equal hostsim's. A VarDCT frame goes drop, keep, keep over two group ranges, whole again (the kept block reused, laid out
    again, and used as cached): what the Modular block decides there is the status and the A samples, so drop mode is opaque and
    keep mode equals alpha_sim_decode's merge over the drop-mode pixels, all four channels."""
    import torch
    import j40_amd
    assert j40_amd.device_count() > 0, "the gpu tests need a HIP device"
    for case in MODULAR:
        name, w, h, opts = case[:4]
        fr = j40_amd.Frame(synth("modular", w, h, SEED, **opts))
        fr.upload(0)
        for _ in range(2):
            err, px = fr.decode_to_host()
            assert err == "" and fr.status() == "", (name, err)
            assert np.array_equal(px, cpu[name][0]), name
        fr.close()
    for case in VARDCT:
        name, w, h, opts = case[:4]
        fr = j40_amd.Frame(synth("vardct", w, h, SEED, **opts))
        fr.upload(0)
        assert fr.set_alpha(0) == ""
        err, drop = fr.decode_to_host()
        assert err == "" and fr.status() == "" and (drop[..., 3] == 255).all(), (name, err)
        err, again = fr.decode_to_host()
        assert err == "" and np.array_equal(again, drop), name
        want, damage, _ = cpu_keep(sims, case, drop)
        assert damage == 0
        assert fr.set_alpha(1) == ""
        for _ in range(2):
            err, keep = fr.decode_to_host()
            assert err == "" and fr.status() == "" and fr.alpha()["written"] == 1, (name, err)
            assert np.array_equal(keep, want), name
        n = fr.info["num_groups"]
        assert n >= 2
        for _ in range(2):
            out = torch.full((h, w * 4), 9, dtype=torch.uint8, device="cuda:0")
            for first, count in ((0, n // 2), (n // 2, n - n // 2)):
                fr.set_group_range(first, count)
                fr.decode(out.data_ptr(), w * 4, torch.cuda.current_stream().cuda_stream)
                torch.cuda.synchronize()
                assert fr.status() == "", name
            assert np.array_equal(out.cpu().numpy().reshape(h, w, 4), want), name
        fr.set_group_range(0, n)
        for _ in range(2):
            err, keep = fr.decode_to_host()
            assert err == "" and fr.status() == "" and np.array_equal(keep, want), name
        fr.close()
