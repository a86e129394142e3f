"""Patches on the host (include/j40hip.h, J40HIP_SEQ_PATCHES): the switch, the index over reference-only frames and patch dictionaries,
what is refused and with which code, and device/patch_dev.h's lane function and tile binning compiled for the CPU, held bit for bit
against numpy's float32. PARITY UNPINNED: the reference holds no code for patches; tests/test_patches_gpu.py has the device and the two
anchors that reach the reference."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import patch_streams as P
from patch_streams import patch_synth, seq_opts, main_refs, flat, NONE, REPLACE, ADD, MUL
from streams import ROOT


@pytest.fixture(scope="module")
def j40(built):
    import j40_amd
    return j40_amd


def code_of(j40, data, **kw):
    """the code a sequence over `data` ends with: j40hip_sequence_open's, else the first row's that has one, else the first frame's
    that does not parse"""
    try:
        seq = j40.Sequence(data, **kw)
    except j40.J40Error as e:
        return e.code
    try:
        for k in range(seq.num_frames):
            if seq.frame_info(k)["code"]:
                return seq.frame_info(k)["code"]
            try:
                seq.frame(k)
            except j40.J40Error as e:
                return e.code
        return ""
    finally:
        seq.close()


VARDCT = ("v", P.VW, P.VH, [P.REF_V, P.REF_M], ["v", "m"])
MODULAR = ("m", P.MW, P.MH, [P.REF_M, (60, 34)], ["m", "m"])


def stream_of(kind, refs=None, **more):
    main, w, h, sizes, modes = kind
    refs = main_refs(w, h, sizes[0], sizes[1]) if refs is None else refs
    opts = seq_opts(main, refs, sizes, modes, **more)
    return refs, opts, patch_synth("vardct" if main == "v" else "modular", w, h, **opts)


# ---------------------------------------------------------------- 1. the switch

@pytest.mark.parametrize("kind", [VARDCT, MODULAR], ids=["vardct", "modular"])
def test_without_the_switch_it_is_todo(j40, monkeypatch, kind):
    _, opts, data = stream_of(kind)
    for env in (None, "1"):
        monkeypatch.delenv("J40HIP_PATCHES", raising=False)
        if env:
            monkeypatch.setenv("J40HIP_PATCHES", env)
        with pytest.raises(j40.J40Error) as e:
            j40.Frame(data)                       # a stand-alone parse: its first frame is neither the last nor of type 0
        assert e.value.code == "TODO"
        assert code_of(j40, data, modular_xyb=True) == ("" if env else "TODO")
    monkeypatch.delenv("J40HIP_PATCHES", raising=False)
    # the main frame alone (has_patches, last, type 0): "TODO" as a frame and as a member of a sequence without the switch
    n = opts["frames"] - 1
    alone = patch_synth("vardct" if kind[0] == "v" else "modular", kind[1], kind[2], **dict(opts, only=n))
    for env in (None, "1"):
        if env:
            monkeypatch.setenv("J40HIP_PATCHES", env)
        with pytest.raises(j40.J40Error) as e:
            j40.Frame(alone)
        assert e.value.code == "TODO"
    monkeypatch.delenv("J40HIP_PATCHES", raising=False)
    two = dict(frames=2, patches=";" + opts["patches"].lstrip(";"))   # two regular frames, the second with the flag
    if kind[0] == "m":
        two["xyb"] = 1
    assert code_of(j40, patch_synth("vardct" if kind[0] == "v" else "modular", kind[1], kind[2], **two), modular_xyb=True) == "TODO"


def test_modular_reference_frame_needs_the_modular_xyb_switch(j40):
    _, _, data = stream_of(VARDCT)
    assert code_of(j40, data, patches=True) == "TODO"
    assert code_of(j40, data, patches=True, modular_xyb=True) == ""


# ---------------------------------------------------------------- 2. the index

@pytest.mark.parametrize("kind", [VARDCT, MODULAR], ids=["vardct", "modular"])
def test_index(j40, kind):
    """this is a test that fails without the feature: the keyword does not exist"""
    main, w, h, sizes, modes = kind
    refs, opts, data = stream_of(kind)
    said = patch_synth("vardct" if main == "v" else "modular", w, h, stats=True, **opts)
    seq = j40.Sequence(data, patches=True, modular_xyb=True)
    try:
        assert seq.num_frames == 3 and seq.num_shown == 1 and (seq.width, seq.height) == (w, h)
        for k, size in enumerate(sizes):
            info, pt = seq.frame_info(k), seq.frame_patches(k)
            assert (info["type"], info["w"], info["h"], info["x0"], info["y0"]) == (2, size[0], size[1], 0, 0)
            assert (info["shown"], info["saved"], info["save_as_reference"], info["code"]) == (0, 0, k + 1, "")
            assert pt == dict(has_patches=0, num_ref=0, placements=0, slots=0, stored_xyb=1, xyb_slot=k + 1, tiles=0, launches=0)
        info, pt = seq.frame_info(2), seq.frame_patches(2)
        assert (info["type"], info["w"], info["h"], info["shown"], info["saved"], info["code"]) == (0, w, h, 1, 0, "")
        want = flat(refs)
        assert pt == dict(has_patches=1, num_ref=len(refs), placements=len(want), slots=0b110, stored_xyb=0, xyb_slot=-1,
                          tiles=len(P.tiles_touched(want, w, h)), launches=0)
        # every placement as the generator says it wrote it (count > 1, negative deltas among them)
        (row,) = said["patches"]
        assert row["frame"] == 2 and len(row["placements"]) == len(want)
        assert any(b[0] < a[0] and b[1] < a[1] for a, b in zip(want, want[1:]))
        for i, (wrote, src) in enumerate(zip(row["placements"], [r for r, ref in enumerate(refs) for _ in ref[5]])):
            got = seq.frame_patch(2, i)
            assert [got[f] for f in ("x", "y", "w", "h", "x0", "y0", "ref", "mode", "clamp", "source")] == wrote
            assert tuple(wrote[:9]) == want[i] and wrote[9] == src
        with pytest.raises(j40.J40Error):
            seq.frame_patch(2, len(want))
        # the handles parse: a reference-only frame of its own size, the main frame with its dictionary
        assert [(seq.frame(k).width, seq.frame(k).height) for k in range(3)] == [sizes[0], sizes[1], (w, h)]
    finally:
        seq.close()


def test_pixels_saved_into_a_slot_take_the_planes_place(j40):
    """slot 1: a reference-only frame, then a regular frame saved there -- a patch that names slot 1 finds no planes"""
    refs = [(1, 0, 0, 8, 8, [(0, 0, REPLACE, 0)])]
    opts = dict(frames=3, types="2,0,0", crops="0,0,264,40;;", saves="1,1,0", patches=";;" + P.dictionary(refs))
    assert code_of(j40, patch_synth("vardct", P.VW, P.VH, **opts), patches=True) == "ptno"
    opts["saves"] = "1,2,0"
    assert code_of(j40, patch_synth("vardct", P.VW, P.VH, **opts), patches=True) == ""


# ---------------------------------------------------------------- 3. refusals with the switch

def one(slot=1, x0=0, y0=0, w=8, h=8, at=((0, 0, REPLACE, 0),)):
    return [(slot, x0, y0, w, h, list(at))]


REFUSALS = [
    ("mode_4", dict(refs=one(at=((0, 0, 4, 0),))), "TODO"),
    ("mode_7", dict(refs=one(at=((0, 0, 7, 1),))), "TODO"),
    ("mode_8", dict(refs=one(at=((0, 0, 8, 0),))), "ptch"),
    ("ref_4", dict(refs=one(slot=4)), "ptch"),
    ("source_one_past_the_reference_frame_right", dict(refs=one(x0=P.REF_V[0] - 7)), "ptch"),
    ("source_one_past_the_reference_frame_below", dict(refs=one(y0=P.REF_V[1] - 7)), "ptch"),
    ("source_at_the_reference_frames_corner", dict(refs=one(x0=P.REF_V[0] - 8, y0=P.REF_V[1] - 8)), ""),
    ("placement_one_past_the_frame_right", dict(refs=one(at=((P.VW - 7, 0, REPLACE, 0),))), "ptch"),
    ("placement_one_past_the_frame_below", dict(refs=one(at=((0, P.VH - 7, ADD, 0),))), "ptch"),
    ("placement_at_the_frames_corner", dict(refs=one(at=((P.VW - 8, P.VH - 8, ADD, 0),))), ""),
    ("negative_placement", dict(refs=one(at=((4, 4, REPLACE, 0), (-1, 4, REPLACE, 0)))), "ptch"),
    ("negative_placement_y", dict(refs=one(at=((4, 4, REPLACE, 0), (4, -3, REPLACE, 0)))), "ptch"),
    ("empty_slot", dict(refs=one(slot=2)), "ptno"),
    ("save_before_ct_0", dict(refs=one(), sbct=0), "TODO"),
    ("dictionary_cut_short", dict(refs=main_refs(P.VW, P.VH, P.REF_V, P.REF_V), patchcut=1), "shrt"),
]


@pytest.mark.parametrize("name,how,code", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusals(j40, name, how, code):
    how = dict(how)
    refs = how.pop("refs")
    if name == "dictionary_cut_short":
        refs = [r for r in refs if r[0] == 1]
    opts = seq_opts("v", refs, [P.REF_V], ["v"], **how)
    assert code_of(j40, patch_synth("vardct", P.VW, P.VH, **opts), patches=True) == code


def test_extra_channel_entry_is_todo(j40):
    """an image with an alpha channel: the dictionary carries two blend entries a placement; the second one other than None is not served"""
    for mode, ec, code in ((1, 0, ""), (1, 1, "TODO"), (0, 2, "TODO")):
        opts = seq_opts("m", [(1, 0, 0, 8, 8, [(0, 0, mode, 0)])], [P.REF_M], ["m"], alpha=1, patchec=ec)
        assert code_of(j40, patch_synth("modular", P.MW, P.MH, **opts), patches=True, modular_xyb=True) == code, (mode, ec)


def test_reference_frame_of_an_image_that_is_not_xyb_is_todo(j40):
    opts = dict(frames=2, types="2,0", crops="0,0,90,50;", saves="1,0")
    data = patch_synth("modular", P.MW, P.MH, **opts)      # xyb_encoded = 0
    assert code_of(j40, data, patches=True, modular_xyb=True) == "TODO"
    assert code_of(j40, patch_synth("modular", P.MW, P.MH, xyb=1, **opts), patches=True, modular_xyb=True) == ""


def test_more_reference_patches_than_the_frame_allows(j40):
    """1024 + pixels / 4 reference patches at the most: what bounds the host's allocations for a damaged stream"""
    for n, code in ((1024 + 8 * 8 // 4, ""), (1024 + 8 * 8 // 4 + 1, "ptch")):
        refs = [(1, i % 8, 0, 1, 1, [(i % 8, i // 8 % 8, ADD, 0)]) for i in range(n)]
        opts = seq_opts("m", refs, [(8, 8)], ["m"])
        assert code_of(j40, patch_synth("modular", 8, 8, **opts), patches=True, modular_xyb=True) == code, n


def test_more_tile_entries_than_the_frame_allows(j40):
    """a legal dictionary whose placements touch more tiles, summed, than 4096 + 64 a tile (device/patch_dev.h: patch_bin_limit) is
    "ptch" when the index is built: the dictionary bounds the placements, this bounds what is binned, allocated and uploaded for them.
    A 64 x 32 frame is one tile (4160 entries) and may hold 4 * (1024 + 512) = 6144 placements"""
    for each, code in ((4, ""), (5, "ptch")):
        refs = [(1, 0, 0, 1, 1, [((i + j) % 64, i % 32, ADD, 0) for j in range(each)]) for i in range(1040)]
        opts = seq_opts("m", refs, [(8, 8)], ["m"])
        assert code_of(j40, patch_synth("modular", 64, 32, **opts), patches=True, modular_xyb=True) == code, each
    # placements of mode None touch nothing and do not count
    refs = [(1, 0, 0, 1, 1, [((i + j) % 64, i % 32, NONE, 0) for j in range(5)]) for i in range(1040)]
    assert code_of(j40, patch_synth("modular", 64, 32, **seq_opts("m", refs, [(8, 8)], ["m"])), patches=True, modular_xyb=True) == ""


# ---------------------------------------------------------------- 4. the device function and the binning on the CPU

class PatchSim:
    def __init__(self):
        self.L = C.CDLL(os.path.join(ROOT, "build", "libhostsim_patches.so"))
        self.L.patch_sim_apply.restype = C.c_uint32
        self.L.patch_sim_bin.restype = C.c_int32

    def apply(self, planes, slots, placements):
        out = np.array(planes, np.float32, copy=True)
        _, h, w = out.shape
        keep = [None if k not in slots else np.ascontiguousarray(slots[k], np.float32) for k in range(4)]
        ptrs = (C.c_void_p * 4)(*[None if s is None else s.ctypes.data for s in keep])
        sw = (C.c_int32 * 4)(*[0 if s is None else s.shape[2] for s in keep]); sh = (C.c_int32 * 4)(*[0 if s is None else s.shape[1] for s in keep])
        pl = np.ascontiguousarray(placements, np.int32).reshape(-1, 9)
        code = self.L.patch_sim_apply(C.c_void_p(out.ctypes.data), w, h, ptrs, sw, sh, C.c_void_p(pl.ctypes.data), len(pl))
        return code, out

    def bin(self, placements, w, h):
        pl = np.ascontiguousarray(placements, np.int32).reshape(-1, 9)
        cap = 1 << 16
        xy = np.zeros(2, np.int32); ids = np.zeros(cap, np.int32); offs = np.zeros(cap + 1, np.int32); index = np.zeros(cap, np.int32)
        n = self.L.patch_sim_bin(C.c_void_p(pl.ctypes.data), len(pl), w, h, C.c_void_p(xy.ctypes.data), C.c_void_p(ids.ctypes.data), cap, C.c_void_p(offs.ctypes.data), C.c_void_p(index.ctypes.data), cap)
        if n < 0:
            return None, None
        return tuple(xy), {int(ids[b]): index[offs[b]:offs[b + 1]].tolist() for b in range(n)}


@pytest.fixture(scope="module")
def sim(built):
    return PatchSim()


def test_lane_function_equals_numpy(sim):
    rng = np.random.default_rng(11)
    slots, cases = P.kat_cases(rng)
    planes = rng.uniform(-1.0, 2.0, (3, P.MH, P.MW)).astype(np.float32)
    results = {}
    for name, placements in cases:
        code, got = sim.apply(planes, slots, placements)
        want = P.apply_patches(planes, slots, placements)
        assert code == 0 and np.array_equal(P.bits(got), P.bits(want)), name
        results[name] = got
    assert not np.array_equal(results["replace_then_add"], results["add_then_replace"])
    assert np.array_equal(P.bits(results["none_touches_nothing"]), P.bits(planes))
    # clamp matters: the sources reach outside [0, 1]
    a = sim.apply(planes, slots, [(0, 0, 90, 60, 3, 3, 0, MUL, 0)])[1]
    b = sim.apply(planes, slots, [(0, 0, 90, 60, 3, 3, 0, MUL, 1)])[1]
    assert not np.array_equal(a, b)


def test_what_the_check_refuses(sim):
    planes = np.zeros((3, 40, 70), np.float32)
    slots = {0: np.zeros((3, 10, 12), np.float32)}
    ptch, ptno = 0x70746368, 0x70746e6f
    for placement, code in (((0, 0, 12, 10, 0, 0, 0, REPLACE, 0), 0), ((0, 0, 12, 10, 1, 0, 0, REPLACE, 0), ptch), ((0, 0, 12, 10, 0, 1, 0, ADD, 0), ptch),
                            ((59, 0, 12, 10, 0, 0, 0, ADD, 0), ptch), ((0, 31, 12, 10, 0, 0, 0, ADD, 0), ptch), ((-1, 0, 12, 10, 0, 0, 0, ADD, 0), ptch),
                            ((0, 0, 12, 10, 0, 0, 1, ADD, 0), ptno), ((0, 0, 12, 10, 0, 0, 4, ADD, 0), ptch), ((0, 0, 12, 10, 0, 0, 0, 4, 0), ptch), ((0, 0, 0, 10, 0, 0, 0, ADD, 0), ptch)):
        assert sim.apply(planes, slots, [placement])[0] == code, placement


@pytest.mark.parametrize("w,h", [(P.MW, P.MH), (P.VW, P.VH), (64, 32), (65, 33)])
def test_binning(sim, w, h):
    """for every tile the records that touch it, in dictionary order; tiles nothing touches are not listed"""
    rng = np.random.default_rng(w * 1000 + h)
    placements = []
    for i in range(120):
        pw, ph = int(rng.integers(1, min(w, 90) + 1)), int(rng.integers(1, min(h, 70) + 1))
        placements.append((int(rng.integers(0, w - pw + 1)), int(rng.integers(0, h - ph + 1)), pw, ph, 0, 0, 0, int(rng.integers(0, 4)), 0))
    for chosen in (placements[:1], placements[:7], placements, [(0, 0, w, h, 0, 0, 0, NONE, 0)], []):
        xy, got = sim.bin(chosen, w, h)
        assert xy == ((w + 63) // 64, (h + 31) // 32)
        assert got == P.tiles_touched(chosen, w, h)
    slots, cases = P.kat_cases(np.random.default_rng(1))
    for name, chosen in cases:
        assert sim.bin(chosen, P.MW, P.MH)[1] == P.tiles_touched(chosen, P.MW, P.MH), name


def test_binning_is_bounded(sim):
    """the sum over the placements of the tiles each touches may reach 4096 + 64 a tile and no more: a longer list is not binned, and
    the lane function's entry answers "ptch" for it. 200 x 136 is 4 x 5 tiles: 5376 entries, 268 whole-frame placements"""
    whole = (0, 0, P.MW, P.MH, 0, 0, 0, ADD, 0)
    limit = 4096 + 64 * 20
    assert sim.bin([whole] * (limit // 20), P.MW, P.MH)[1] is not None
    assert sim.bin([whole] * (limit // 20 + 1), P.MW, P.MH) == (None, None)
    assert sim.bin([whole] * (limit // 20) + [(0, 0, 1, 1, 0, 0, 0, ADD, 0)] * (limit % 20), P.MW, P.MH)[1] is not None
    assert sim.bin([whole] * (limit // 20) + [(0, 0, 1, 1, 0, 0, 0, ADD, 0)] * (limit % 20 + 1), P.MW, P.MH) == (None, None)
    assert sim.bin([(0, 0, P.MW, P.MH, 0, 0, 0, NONE, 0)] * 1000, P.MW, P.MH)[1] == {}
    planes = np.zeros((3, P.MH, P.MW), np.float32)
    slots = {0: np.ones((3, P.MH, P.MW), np.float32)}
    code, got = sim.apply(planes, slots, [whole] * (limit // 20))
    assert code == 0 and (got == limit // 20).all()
    code, got = sim.apply(planes, slots, [whole] * (limit // 20 + 1))
    assert code == 0x70746368 and (got == 0).all()


@pytest.mark.parametrize("program", ["patch_main", "patch_main_san"])
def test_stand_alone_program_plain_and_sanitised(built, program):
    """random placement lists over planes and slots in allocations of exactly their size (tests/hostsim/patch_main.cpp)"""
    r = subprocess.run([os.path.join(ROOT, "build", program)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    assert r.returncode == 0, r.stdout.decode()
    assert b"0 failure(s)" in r.stdout
