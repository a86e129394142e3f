"""Region decode (j40hip_frame_set_region, include/j40hip.h): a rectangle of a frame from the pass groups that cover it.

The oracle is the simplest there is: the rectangle is the crop of the whole decode of the same handle, bit for bit, and through it the
reference's pixels (exact for Modular frames, within the one level the parity tests allow for VarDCT). What a region decode cost --
sections launched, varblocks through the pixel kernels -- is read from j40hip_frame_region and compared with counts made here by brute
force. Without a device: the header logic on parsed frames, and the device functions of device/region_dev.h (the group-major index of
the varblock list, the gather of a cover, the crop) run on the CPU by build/libhostsim_region.so (tests/hostsim/region_sim.cpp)."""
import ctypes as C
import os

import numpy as np
import pytest

from streams import synth, ROOT, VARDCT_CASES, MODULAR_CASES

U8X4, U16X4 = 0x0F33, 0x0F35
SEED = 7


# ---------------------------------------------------------------- rectangles and covers, restated

def cover_of(x, y, w, h, shift):
    gx0, gy0 = x >> shift, y >> shift
    return gx0, gy0, ((x + w - 1) >> shift) - gx0 + 1, ((y + h - 1) >> shift) - gy0 + 1


def clip(x, y, w, h, W, H):
    x, y = max(0, min(x, W - 1)), max(0, min(y, H - 1))
    return x, y, max(1, min(w, W - x)), max(1, min(h, H - y))


def fixed_rects(W, H, shift):
    """one pixel, a group-aligned block, a rectangle straddling a four-group corner, the bottom-right corner, a full-width band"""
    g = 1 << shift
    return [
        clip(W // 2 + 1, H // 2 + 1, 1, 1, W, H),
        clip(g if W > g else 0, 0, g, g, W, H),
        clip(g - 37, g - 21, 75, 43, W, H),
        clip(W - 33, H - 17, 33, 17, W, H),
        clip(0, H // 3, W, 40, W, H),
    ]


def random_rects(W, H, n, seed):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        x, y = int(rng.integers(0, W)), int(rng.integers(0, H))
        out.append((x, y, int(rng.integers(1, W - x + 1)), int(rng.integers(1, H - y + 1))))
    return out


# ---------------------------------------------------------------- without a device: the header logic

# (kind, width, height, options): group shifts 7 to 10, frames whose last group column and row are partial
HEADER_STREAMS = [
    ("modular", 700, 500, dict(groupshift=7)),
    ("modular", 600, 300, dict()),
    ("modular", 1100, 600, dict(groupshift=9)),
    ("modular", 2100, 1100, dict(groupshift=10)),
    ("vardct", 776, 600, dict()),
]


@pytest.mark.parametrize("kind,W,H,opts", HEADER_STREAMS, ids=["%s_%dx%d_%s" % (k, w, h, o.get("groupshift", 8)) for k, w, h, o in HEADER_STREAMS])
def test_set_region_and_cover_on_a_parsed_frame(built, kind, W, H, opts):
    import j40_amd
    fr = j40_amd.Frame(synth(kind, W, H, SEED, **opts))
    shift = fr.info["group_size_shift"]
    assert shift == opts.get("groupshift", 8)
    gcols, grows = (W + (1 << shift) - 1) >> shift, (H + (1 << shift) - 1) >> shift
    none = dict(x=0, y=0, w=W, h=H, gx0=0, gy0=0, gcols=gcols, grows=grows, set=0, widened=0, sections=0, varblocks=0)
    assert fr.region() == none
    for rect in fixed_rects(W, H, shift) + random_rects(W, H, 20, 11) + [(W - 1, H - 1, 1, 1), (0, 0, W, 1), (0, 0, 1, H), (1, 0, W - 1, H)]:
        assert fr.set_region(*rect) == "", rect
        r = fr.region()
        assert (r["x"], r["y"], r["w"], r["h"]) == rect and r["set"] == 1
        assert (r["gx0"], r["gy0"], r["gcols"], r["grows"]) == cover_of(*rect, shift), rect
        assert r["gx0"] + r["gcols"] <= gcols and r["gy0"] + r["grows"] <= grows
    # refusals leave the frame as it was
    assert fr.set_region(5, 6, 7, 8) == ""
    kept = fr.region()
    for bad in [(-1, 0, 4, 4), (0, -1, 4, 4), (0, 0, 0, 4), (0, 0, 4, 0), (0, 0, -3, 4), (W, 0, 1, 1), (0, H, 1, 1), (W - 3, 0, 4, 1), (0, H - 3, 1, 4),
                (1, 0, W, H), (0, 0, W + 1, H), (0, 0, 2 ** 31 - 1, 1), (2 ** 31 - 1, 0, 2 ** 31 - 1, 1), (1, 1, 0, 0)]:
        assert fr.set_region(*bad) == "rnge", bad
        assert fr.region() == kept
    # clearing; the full rectangle is no region
    assert fr.clear_region() == "" and fr.region() == none
    assert fr.set_region(5, 6, 7, 8) == "" and fr.set_region(0, 0, W, H) == "" and fr.region() == none
    assert fr.set_region(0, 0, W, H - 1) == "" and fr.region()["set"] == 1
    assert fr.set_region(0, 0, 0, 0) == "" and fr.region() == none
    fr.close()


def test_lf_only_frame_refuses_a_region(built):
    import j40_amd
    data = synth("vardct", 776, 600, SEED)
    fr = j40_amd.Frame(data[:j40_amd.Frame(data).lf_end()], lf_only=True)
    assert fr.set_region(0, 0, 8, 8) == "Ulf?" and fr.clear_region() == "Ulf?"
    assert fr.region()["set"] == 0
    fr.close()


# ---------------------------------------------------------------- without a device: the region's varblock list

_sim = None


def region_sim():
    global _sim
    if _sim is None:
        L = C.CDLL(os.path.join(ROOT, "build", "libhostsim_region.so"))
        vp, i32, i64, sz = C.c_void_p, C.c_int32, C.c_int64, C.c_size_t
        L.region_sim_open.restype = vp; L.region_sim_open.argtypes = [vp, sz, C.POINTER(C.c_uint32)]
        L.region_sim_close.argtypes = [vp]
        L.region_sim_info.argtypes = [vp, vp]
        L.region_sim_sorted.argtypes = [vp, vp, vp]
        L.region_sim_gather.restype = i64; L.region_sim_gather.argtypes = [vp, i32, i32, i32, i32, i32, vp, i64, vp, vp, vp]
        L.region_sim_crop.argtypes = [vp, sz, vp, sz, i32, i32, i32, i32]
        _sim = L
    return _sim


class SimStream:
    """a stream's varblock list as the pixel kernels take it (rows: px, py, effw, effh, dctsel, blk, llf_base, coeff_base)"""

    def __init__(self, data):
        L = region_sim()
        self.buf = C.create_string_buffer(data, len(data))
        err = C.c_uint32()
        self.h = L.region_sim_open(self.buf, len(data), C.byref(err))
        assert self.h and err.value == 0, hex(err.value)
        info = np.zeros(6, np.int32)
        L.region_sim_info(self.h, info.ctypes.data)
        self.W, self.H, self.shift, self.gcolumns, self.groups, self.count = info.tolist()
        self.sorted = np.zeros((self.count, 8), np.int32)
        self.class_start = np.zeros(28, np.int32)
        L.region_sim_sorted(self.h, self.sorted.ctypes.data, self.class_start.ctypes.data)

    def gather(self, rect, lanes=64):
        out = np.zeros((self.count, 8), np.int32)
        cs, cover, order = np.zeros(28, np.int32), np.zeros(4, np.int32), np.zeros(self.groups, np.uint32)
        n = region_sim().region_sim_gather(self.h, *rect, lanes, out.ctypes.data, self.count, cs.ctypes.data, cover.ctypes.data, order.ctypes.data)
        assert n >= 0, ("an entry outside the list, written twice or not at all", rect)
        return out[:n], cs, tuple(cover.tolist()), order

    def brute(self, rect):
        """the whole list filtered by the group of each varblock's top-left pixel, rebased to the cover's origin"""
        gx0, gy0, cols, rows = cover_of(*rect, self.shift)
        s = self.sorted
        gx, gy = s[:, 0] >> self.shift, s[:, 1] >> self.shift
        sel = s[(gx >= gx0) & (gx < gx0 + cols) & (gy >= gy0) & (gy < gy0 + rows)].copy()
        sel[:, 0] -= gx0 << self.shift
        sel[:, 1] -= gy0 << self.shift
        return sel

    def close(self):
        region_sim().region_sim_close(self.h)


def brute_varblocks(data, rect):
    s = SimStream(data)
    n = len(s.brute(rect))
    s.close()
    return n


def rows_sorted(a):
    return a[np.lexsort(a.T[::-1])] if len(a) else a


LIST_STREAMS = [
    ("776x600_maxlog8", 776, 600, dict(maxlog=8)),
    ("2600x2100_several_lf_groups", 2600, 2100, dict()),
    ("1300x776_default", 1300, 776, dict(VARDCT_CASES)["default"]),
    ("1300x776_cfl", 1300, 776, dict(VARDCT_CASES)["cfl"]),
]


@pytest.mark.parametrize("name,W,H,opts", LIST_STREAMS, ids=[s[0] for s in LIST_STREAMS])
def test_region_list_equals_the_brute_force_filter(built, name, W, H, opts):
    s = SimStream(synth("vardct", W, H, SEED, **opts))
    assert (s.W, s.H) == (W, H) and s.count == s.class_start[27]
    if "several_lf_groups" in name:
        assert W > 2048 and H > 2048   # (an LfGroup is 2048 pixels wide)
    for rect in fixed_rects(W, H, s.shift) + random_rects(W, H, 50, 2024):
        got, cs, cover, order = s.gather(rect, lanes=64 if rect[0] % 2 else 5)
        want = s.brute(rect)
        gx0, gy0, cols, rows = cover_of(*rect, s.shift)
        assert cover == (gx0, gy0, cols, rows)
        assert order[:cols * rows].tolist() == [(gy0 + i // cols) * s.gcolumns + gx0 + i % cols for i in range(cols * rows)]
        assert len(got) == len(want) == cs[27], rect   # field [11] of j40hip_frame_region
        assert cs[0] == 0 and np.all(np.diff(cs) >= 0)
        for d in range(27):
            a, b = got[cs[d]:cs[d + 1]], want[want[:, 4] == d]
            assert np.all(a[:, 4] == d), (rect, d)   # class-contiguous, as launch_vardct_frame needs
            assert np.array_equal(rows_sorted(a), rows_sorted(b)), (rect, d)
        # rebased: every varblock lies inside the cover's image
        cw, ch = min(W, (gx0 + cols) << s.shift) - (gx0 << s.shift), min(H, (gy0 + rows) << s.shift) - (gy0 << s.shift)
        if len(got):
            assert got[:, 0].min() >= 0 and got[:, 1].min() >= 0
            assert (got[:, 0] + got[:, 2]).max() <= cw and (got[:, 1] + got[:, 3]).max() <= ch
    # the whole frame's cover gives the whole list back
    got, cs, _, _ = s.gather((0, 0, W, H))
    assert np.array_equal(cs, s.class_start) and np.array_equal(rows_sorted(got), rows_sorted(s.sorted))
    s.close()


@pytest.mark.parametrize("pb", [4, 8])
def test_crop_function_is_exact_and_writes_nothing_else(built, pb):
    L = region_sim()
    rng = np.random.default_rng(5)
    SW, SH = 301, 23
    src = rng.integers(0, 256, (SH, SW * pb + 24), np.uint8)
    for x0 in (0, 1, 2, 3, 4, 7, 64):
        for w in (1, 2, 3, 4, 5, 16, 31, 64, 97, SW - x0):
            for pad, shift_dst in ((0, 0), (pb, 0), (24, pb), (16, 3 * pb), (5 * pb, 4)):
                if shift_dst % pb:
                    continue
                h, y0 = SH - 3, 2
                stride = w * pb + pad
                whole = np.full(stride * h + 64, 0xA5, np.uint8)
                # the destination's first pixel at every alignment a pixel-aligned pointer can have within 16 bytes
                base = whole.ctypes.data
                off = (-base) % 16 + shift_dst
                dst = whole[off:off + stride * h]
                sp = src.ctypes.data + y0 * src.strides[0] + x0 * pb
                L.region_sim_crop(sp, src.strides[0], dst.ctypes.data, stride, w, h, pb, 7 if w % 2 else 64)
                rows = dst.reshape(h, stride)
                assert np.array_equal(rows[:, :w * pb], src[y0:y0 + h, x0 * pb:(x0 + w) * pb]), (x0, w, pad, shift_dst)
                assert np.all(rows[:, w * pb:] == 0xA5), "bytes between the rows were written"
                assert np.all(whole[:off] == 0xA5) and np.all(whole[off + stride * h:] == 0xA5)


# ---------------------------------------------------------------- on the GPU

@pytest.fixture(scope="module")
def gpu(built):
    import j40_amd
    assert j40_amd.device_count() > 0, "the gpu tests need a HIP device"
    return j40_amd


def level_to_u8(u16, bpp):
    """a 16-bit sample back to its level at the image's depth, then the 8-bit render (tests/test_u16_output.py's rule)"""
    maxpixel = (1 << bpp) - 1
    p = (u16.astype(np.int64) * maxpixel + 32767) // 65535
    return (p * 255 + (1 << (bpp - 1))) // maxpixel


SENTINEL = 0xC3


def decode_into_sentinel(fr, rect, fmt, pad_pixels=3):
    """the region through the asynchronous entry point into a padded device image full of SENTINEL, two rows of it above and below;
    returns the pixels [h, w, 4] after checking that nothing but the w pixels of the h rows was written"""
    import torch
    x, y, w, h = rect
    pb = 8 if fmt == U16X4 else 4
    stride = (w + pad_pixels) * pb
    buf = torch.full(((h + 4) * stride,), SENTINEL, dtype=torch.uint8, device="cuda:0")
    s = torch.cuda.current_stream()
    fr.decode(buf.data_ptr() + 2 * stride, stride, s.cuda_stream)
    s.synchronize()
    a = buf.cpu().numpy().reshape(h + 4, stride)
    assert np.all(a[:2] == SENTINEL) and np.all(a[-2:] == SENTINEL), "rows outside the region were written"
    assert np.all(a[2:-2, w * pb:] == SENTINEL), "bytes between the rows were written"
    px = np.ascontiguousarray(a[2:-2, :w * pb])
    return px.view(np.uint16).reshape(h, w, 4) if fmt == U16X4 else px.reshape(h, w, 4)


def whole_decode(gpu, data, fmt, prepare=None):
    fr = gpu.Frame(data)
    if prepare:
        prepare(fr)
    fr.set_output_format(fmt)
    fr.upload(0)
    err, full = fr.decode_to_host()
    assert err == "", err
    return fr, full


def check_regions(gpu, ref, data, rects, modular, passes):
    rerr, expect = ref.decode(data)
    assert rerr == ""
    H, W = expect.shape[:2]
    for fmt in (U8X4, U16X4):
        fr, full = whole_decode(gpu, data, fmt)
        shift, bpp = fr.info["group_size_shift"], fr.info["bpp"]
        assert full.shape == (H, W, 4)
        # a Modular frame's lead sections: what its plan holds ahead of the pass groups' sections (LfGlobal's)
        lead = fr.coop_sections()[1] - passes * fr.info["num_groups"] if modular else 0
        assert lead in (0, 1)
        for rect in rects:
            x, y, w, h = rect
            assert fr.set_region(*rect) == ""
            px = decode_into_sentinel(fr, rect, fmt, pad_pixels=3 if w % 2 else 0 if x % 2 else 5)
            assert fr.status() == ""
            assert np.array_equal(px, full[y:y + h, x:x + w]), ("not the crop of the whole decode", rect, fmt)
            got8 = px if fmt == U8X4 else level_to_u8(px, bpp)
            d = np.abs(got8.astype(np.int64) - expect[y:y + h, x:x + w].astype(np.int64))
            assert d.max() <= (0 if modular else 1), (rect, fmt, int(d.max()))
            r = fr.region()
            gx0, gy0, cols, rows = cover_of(*rect, shift)
            assert (r["gx0"], r["gy0"], r["gcols"], r["grows"]) == (gx0, gy0, cols, rows)
            assert r["widened"] == 0
            assert r["sections"] == lead + passes * cols * rows, (rect, r)
            assert r["varblocks"] == (0 if modular else brute_varblocks(data, rect)), (rect, r)
            # the synchronous entry point: the same pixels, only the rectangle's shape
            err, again = fr.decode_to_host()
            assert err == "" and again.shape == (h, w, 4) and np.array_equal(again, px)
        assert fr.clear_region() == ""
        err, again = fr.decode_to_host()
        assert err == "" and np.array_equal(again, full)
        fr.close()


VARDCT_NAMES = ["default", "passes", "hf_prefix_lz77_passes", "permuted_toc_two_passes", "alpha_extra_channel", "bit_depth_12"]


@pytest.mark.gpu
@pytest.mark.parametrize("name", VARDCT_NAMES + ["776x600_maxlog8"])
def test_vardct_region_is_the_crop_of_the_whole_decode(gpu, ref, name):
    if name == "776x600_maxlog8":
        W, H, opts = 776, 600, dict(maxlog=8)
    else:
        W, H, opts = 1300, 776, dict(VARDCT_CASES)[name]
    data = synth("vardct", W, H, SEED, **opts)
    check_regions(gpu, ref, data, fixed_rects(W, H, 8), False, opts.get("passes", 1))


MODULAR_NAMES = ["multi_group", "palette", "local_tree_under_wp_global", "local_rct_local_tree_no_global_rct", "local_palette", "three_passes_local_rct_local_tree_alpha"]


@pytest.mark.gpu
@pytest.mark.parametrize("name", MODULAR_NAMES)
def test_modular_region_is_the_crop_of_the_whole_decode(gpu, ref, name):
    _, W, H, opts = [c for c in MODULAR_CASES if c[0] == name][0]
    shift = opts.get("groupshift", 8)
    assert ((W + (1 << shift) - 1) >> shift) * ((H + (1 << shift) - 1) >> shift) > 1, "several groups"
    chosen = [c[3] for c in MODULAR_CASES if c[0] in MODULAR_NAMES]
    assert len(chosen) == 6 and sum(1 for o in chosen if o.get("groupshift") == 7) >= 2
    assert any(o.get("localpalette") for o in chosen) and any(o.get("passes") == 3 for o in chosen)
    check_regions(gpu, ref, synth("modular", W, H, SEED, **opts), fixed_rects(W, H, shift), True, opts.get("passes", 1))


@pytest.mark.gpu
def test_pan_clear_and_determinism(gpu):
    for kind, W, H, opts in (("vardct", 1300, 776, dict()), ("vardct", 1300, 776, dict(passes=2, hfprefix=1, hflz77=1)), ("modular", 600, 300, dict(localrct=4, alpha=1))):
        data = synth(kind, W, H, SEED, **opts)
        fr, full = whole_decode(gpu, data, U8X4)
        path = [(10 + 97 * k, 5 + 61 * k, 300, 200) for k in range(8)] + [(0, 0, 256, 256), (256, 256, 256, 256), (255, 255, 2, 2), (3, 3, 5, 5)]
        path = [clip(*r, W, H) for r in path]
        for rect in path + path[::-1]:
            x, y, w, h = rect
            assert fr.set_region(*rect) == ""
            err, a = fr.decode_to_host()
            err2, b = fr.decode_to_host()
            assert err == err2 == "" and np.array_equal(a, b), rect
            assert np.array_equal(a, full[y:y + h, x:x + w]), rect
        assert fr.clear_region() == ""
        err, again = fr.decode_to_host()
        assert err == "" and np.array_equal(again, full) and fr.region()["set"] == 0
        fr.close()


@pytest.mark.gpu
def test_damage_outside_the_cover_is_not_seen(gpu, ref):
    W, H = 1300, 776
    data = synth("vardct", W, H, SEED)   # bare, unpermuted, one pass: the pass-group sections are the file's tail
    fr = gpu.Frame(data)
    sizes = fr.section_sizes().tolist()
    gcols, groups = (W + 255) >> 8, fr.info["num_groups"]
    fr.close()
    assert len(sizes) == groups == gcols * ((H + 255) >> 8)
    k = 2 * gcols + 4   # the group at column 4 of row 2
    start = len(data) - sum(sizes[k:])
    assert sizes[k] > 64
    damaged = code = None
    for off, bit in [(sizes[k] // 2, 0), (sizes[k] // 3, 5), (sizes[k] // 4, 2), (16, 7), (sizes[k] - 9, 1), (sizes[k] // 2 + 1, 3), (8, 0), (sizes[k] * 2 // 3, 6)]:
        m = bytearray(data)
        m[start + off] ^= 1 << bit
        rerr, _ = ref.decode(bytes(m))
        if rerr:
            damaged, code = bytes(m), rerr
            break
    assert damaged is not None, "none of the fixed positions makes the reference report an error"
    clean, full = whole_decode(gpu, data, U8X4)
    clean.close()
    fr = gpu.Frame(damaged)
    fr.upload(0)
    err, _ = fr.decode_to_host()
    assert err == code
    gx, gy = (k % gcols) << 8, (k // gcols) << 8
    for rect in [(0, 0, gx, H), (gx + 256, 0, W - gx - 256, H), (gx - 300, gy - 200, 300, 200), (gx, gy + 256, 256, H - gy - 256), (gx + 256, gy + 255, 1, 1)]:
        x, y, w, h = rect
        assert fr.set_region(*rect) == ""
        err, px = fr.decode_to_host()
        assert err == "", (rect, err)
        assert np.array_equal(px, full[y:y + h, x:x + w]), rect
    for rect in [(gx, gy, 1, 1), (gx - 1, gy - 1, 2, 2), (0, gy + 100, W, 8), (gx + 255, 0, 1, H)]:
        assert fr.set_region(*rect) == ""
        err, _ = fr.decode_to_host()
        assert err == code, (rect, err)
    fr.close()


@pytest.mark.gpu
def test_widening_serves_the_region_from_every_group(gpu):
    cases = [
        ("squeeze", synth("modular", 600, 300, SEED, squeeze=1, tree=1), None),
        ("palette_delta_prediction", synth("modular", 300, 200, SEED, palette=3), None),
        ("restoration_on_gaborish", synth("vardct", 776, 600, SEED, fullheader=1, gab=1), lambda fr: fr.set_restoration(1)),
        ("keep_alpha", synth("vardct", 600, 300, SEED, alpha=1), lambda fr: (None, fr.set_alpha(1))[0]),
    ]
    for name, data, prepare in cases:
        for fmt in (U8X4, U16X4):
            fr, full = whole_decode(gpu, data, fmt, prepare)
            H, W = full.shape[:2]
            if name == "keep_alpha":
                assert fr.alpha()["written"] == 1
            # every section of the frame: what the whole decode runs
            all_sections = fr.coop_sections()[1] if fr.info["is_modular"] else fr.info["num_passes"] * fr.info["num_groups"]
            for rect in fixed_rects(W, H, fr.info["group_size_shift"]):
                x, y, w, h = rect
                assert fr.set_region(*rect) == ""
                px = decode_into_sentinel(fr, rect, fmt)
                assert fr.status() == ""
                assert np.array_equal(px, full[y:y + h, x:x + w]), (name, rect, fmt)
                r = fr.region()
                assert r["widened"] == 1, (name, rect)
                assert r["sections"] == all_sections, (name, r)
            fr.close()


@pytest.mark.gpu
def test_refusals_on_the_device(gpu):
    import torch
    data = synth("vardct", 1300, 776, SEED)
    fr = gpu.Frame(data)
    fr.upload(0)
    # a partial group range first: the region is refused, and the other way round
    fr.set_group_range(2, 5)
    assert fr.set_region(10, 10, 100, 100) == "Urg?" and fr.region()["set"] == 0
    assert fr.clear_region() == ""                      # (clearing is no region)
    fr.set_group_range(0, fr.info["num_groups"])
    assert fr.set_region(10, 10, 100, 100) == ""
    with pytest.raises(gpu.J40Error) as e:
        fr.set_group_range(2, 5)
    assert e.value.code == "Urg?"
    fr.set_group_range(0, fr.info["num_groups"])         # the whole range is no range
    err, px = fr.decode_to_host()
    assert err == "" and px.shape == (100, 100, 4)      # ... and the refused range changed nothing
    # a batch member with a region
    other = gpu.Frame(data)
    other.upload(0)
    with pytest.raises(gpu.J40Error) as e:
        gpu.Batch([other, fr])
    assert e.value.code == "Urg?"
    assert fr.clear_region() == ""
    gpu.Batch([other, fr]).close()
    other.close()
    # a stride one byte short, in each format
    s = torch.cuda.current_stream().cuda_stream
    for fmt, pb in ((U8X4, 4), (U16X4, 8)):
        fr.set_output_format(fmt)
        assert fr.set_region(7, 9, 101, 50) == ""
        buf = torch.full((60 * 101 * pb,), SENTINEL, dtype=torch.uint8, device="cuda:0")
        with pytest.raises(gpu.J40Error) as e:
            fr.decode(buf.data_ptr(), 101 * pb - 1, s)
        assert e.value.code == "rnge"
        with pytest.raises(gpu.J40Error) as e:
            fr.decode_timed(buf.data_ptr(), 101 * pb - 1, s)
        assert e.value.code == "rnge"
        host = np.zeros(60 * 101 * pb, np.uint8)
        assert gpu.err4(gpu.lib().j40hip_frame_decode_to_host(fr.h, host.ctypes.data, 101 * pb - 1)) == "rnge"
        torch.cuda.synchronize()
        assert bool((buf == SENTINEL).all()) and not host.any()
        fr.decode(buf.data_ptr(), 101 * pb, s)
        torch.cuda.synchronize()
        assert fr.status() == ""
    fr.close()


def device_region(fr, rect, fmt=U8X4):
    import torch
    x, y, w, h = rect
    out = torch.zeros((h, w, 4), dtype=torch.uint8 if fmt == U8X4 else torch.int16, device="cuda:0")
    assert fr.set_region(*rect) == ""
    s = torch.cuda.current_stream()
    fr.decode(out.data_ptr(), w * (4 if fmt == U8X4 else 8), s.cuda_stream)
    s.synchronize()
    assert fr.status() == ""
    return out


@pytest.mark.gpu
def test_full_size_regions_on_the_device(gpu):
    import torch
    for kind, W, H, seed, opts in (("vardct", 7680, 4320, 3, dict(forward=1)), ("modular", 16384, 16384, 21, dict(tree=1, repeat=16))):
        data = synth(kind, W, H, seed, **opts)
        fr = gpu.Frame(data)
        fr.upload(0)
        full = torch.zeros((H, W, 4), dtype=torch.uint8, device="cuda:0")
        s = torch.cuda.current_stream()
        fr.decode(full.data_ptr(), W * 4, s.cuda_stream)
        s.synchronize()
        assert fr.status() == ""
        central = ((W - 1024) // 2, (H - 1024) // 2, 1024, 1024)
        for rect in (central, (W - 1000, H - 700, 1000, 700), (0, 0, 513, 257)):
            x, y, w, h = rect
            out = device_region(fr, rect)
            assert bool(torch.equal(out, full[y:y + h, x:x + w])), (kind, rect)
            r = fr.region()
            assert r["widened"] == 0
            if kind == "vardct":
                assert r["sections"] == r["gcols"] * r["grows"]
                if rect == central:
                    assert r["sections"] <= 25
                    print("8K central 1024x1024: %d of %d sections, %d of %d varblocks" % (r["sections"], fr.info["num_groups"], r["varblocks"], brute_varblocks(data, (0, 0, W, H))))
                assert r["varblocks"] == brute_varblocks(data, rect)
            else:
                assert r["sections"] == 1 + r["gcols"] * r["grows"] and r["varblocks"] == 0
        assert fr.clear_region() == ""
        again = torch.zeros_like(full)
        fr.decode(again.data_ptr(), W * 4, s.cuda_stream)
        s.synchronize()
        assert fr.status() == "" and bool(torch.equal(again, full))
        fr.close()
        del full, again


@pytest.mark.gpu
def test_python_decode_region(gpu, ref):
    data = synth("vardct", 1300, 776, SEED, bpp=12, cfl=1)
    for fmt in (U8X4, U16X4):
        fr, full = whole_decode(gpu, data, fmt)
        rect = (301, 77, 555, 333)
        assert fr.set_region(*rect) == ""
        err, px = fr.decode_to_host()
        assert err == "" and px.shape == (333, 555, 4) and px.dtype == full.dtype
        fr.close()
        err, out = gpu.decode_region(data, *rect, fmt=fmt)
        assert err == "" and out.dtype == px.dtype and np.array_equal(out, px)
        assert np.array_equal(out, full[77:77 + 333, 301:301 + 555])
    assert gpu.decode_region(data, 1200, 700, 200, 10)[0] == "rnge"
    assert gpu.decode_region(data + b"\0" * 5, 0, 0, 8, 8)[0] == gpu.decode(data + b"\0" * 5)[0]   # the look behind the frame, as decode() has it
    err, out = gpu.decode_region(data, 0, 0, 1300, 776)
    assert err == "" and out.shape == (776, 1300, 4)
