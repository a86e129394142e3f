"""Oriented output on the device (j40hip_frame_set_orientation, include/j40hip.h): k_orient alone against orient(); every kind of frame
decoded on one handle in stored order, then oriented -- bit for bit orient() of the stored-order decode --, then in stored order again;
the orientation applied last to a scaled decode, a region and the LF preview; the entries that refuse; the public API in a child
process under J40HIP_ORIENT=1; and the bookkeeping. orient() and the CPU side are in tests/test_orient.py."""
import os
import subprocess
import sys

import numpy as np
import pytest

from streams import synth, ROOT
from test_orient import orient, all_differ, U8X4, U16X4, SEED, TILE
from test_scale import box

pytestmark = pytest.mark.gpu

SIZES = [(779, 517), (264, 520)]
LARGE = dict(density=1, decay=1, global_scale=73728, maxlog=8)     # the large-block stream of tests/test_scale_gpu.py


@pytest.fixture(scope="module")
def gpu(built):
    import j40_amd
    assert j40_amd.device_count() > 0, "the gpu tests need a HIP device"
    assert os.environ.get("J40HIP_ORIENT", "") in ("", "0"), "these tests set the mode themselves (and J40HIP_ORIENT in a child process)"
    return j40_amd


# ---------------------------------------------------------------- k_orient alone

KAT_SIZES = [(1, 1), (1, 300), (300, 1), (TILE - 1, TILE + 1), (TILE, TILE), (2 * TILE + 3, TILE + 5), (4099, 3)]


@pytest.mark.parametrize("dtype", [np.uint8, np.uint16], ids=["u8x4", "u16x4"])
@pytest.mark.parametrize("w,h", KAT_SIZES, ids=["%dx%d" % s for s in KAT_SIZES])
def test_k_orient_alone(gpu, w, h, dtype):
    rng = np.random.default_rng(w * 7 + h)
    a = rng.integers(0, np.iinfo(dtype).max + 1, (h, w, 4)).astype(dtype)
    if w != h and w * h >= 6 and min(w, h) >= 2:
        assert all_differ(a)
    for o in range(1, 9):
        err, got, guard = gpu.kat_device_orient(a, o, pad=24)
        assert err == "" and guard, (o, err, "guard bytes behind the rows were written" if not guard else "")
        assert got.dtype == a.dtype and got.shape == orient(a, o).shape and np.array_equal(got, orient(a, o)), o


def test_k_orient_hook_refusals(gpu):
    a = np.zeros((3, 5, 4), np.uint8)
    assert gpu.kat_device_orient(a, 0)[0] == "rnge" and gpu.kat_device_orient(a, 9)[0] == "rnge"
    assert gpu.kat_device_orient(a, 6, fmt=0x1234)[0] == "Ufm?"


# ---------------------------------------------------------------- frames

def open_frame(gpu, data, fmt=U8X4, alpha=False, restoration=None, ycbcr=False):
    fr = gpu.Frame(data, ycbcr=True) if ycbcr else gpu.Frame(data)
    if ycbcr:
        assert fr.set_ycbcr(1) == ""
    if alpha:
        assert fr.set_alpha(1) == ""
    if restoration is not None:
        fr.set_restoration(restoration)
    fr.set_output_format(fmt)
    fr.upload(0)
    return fr


def stored_oriented_stored(gpu, data, o, fmt=U8X4, **mode):
    """one handle: mode 0, mode 1, mode 0 again. Returns (full, oriented, what orientation() said after the oriented decode)"""
    fr = open_frame(gpu, data, fmt, **mode)
    assert fr.orientation()["orientation"] == o
    assert fr.set_orientation(0) == ""
    err, full = fr.decode_to_host()
    assert err == "", err
    q = fr.orientation()
    assert (q["went_through_k_orient"], q["staging_bytes"]) == (0, 0)
    assert all_differ(full), "a picture that is symmetric under an orientation proves nothing here: pick another stream"
    assert fr.set_orientation(1) == ""
    err, turned = fr.decode_to_host()
    assert err == "", err
    said = fr.orientation()
    assert fr.set_orientation(0) == ""
    err, again = fr.decode_to_host()
    assert err == "" and np.array_equal(again, full), "mode 0 afterwards is the stored-order decode again"
    q = fr.orientation()
    assert (q["went_through_k_orient"], q["staging_bytes"]) == (0, 0)
    fr.close()
    return full, turned, said


def check(full, turned, said, o):
    pb = 4 * full.dtype.itemsize
    H, W = full.shape[:2]
    assert turned.dtype == full.dtype and turned.shape == orient(full, o).shape
    assert np.array_equal(turned, orient(full, o)), o
    if o == 1:
        assert (said["applied"], said["went_through_k_orient"], said["staging_bytes"]) == (0, 0, 0)
    else:
        assert (said["applied"], said["went_through_k_orient"], said["staging_bytes"]) == (1, 1, pb * W * H)
    assert (said["width"], said["height"]) == (turned.shape[1], turned.shape[0])


@pytest.mark.parametrize("o", range(1, 9))
@pytest.mark.parametrize("w,h", SIZES, ids=["%dx%d" % s for s in SIZES])
def test_default_vardct_every_orientation(gpu, w, h, o):
    full, turned, said = stored_oriented_stored(gpu, synth("vardct", w, h, SEED, orientation=o), o)
    check(full, turned, said, o)
    assert np.array_equal(full, stored_oriented_stored(gpu, synth("vardct", w, h, SEED), 1)[0]), "the option changes no stored pixel"


FRAME_CASES = [
    ("passes", "vardct", dict(passes=2), U8X4, dict()),
    ("bpp12_u16", "vardct", dict(bpp=12), U16X4, dict()),
    ("large", "vardct", LARGE, U8X4, dict()),
    ("modular_alpha", "modular", dict(alpha=1, prefix=1, lz77=1), U8X4, dict()),
    ("modular_alpha_u16", "modular", dict(alpha=1, tree=3), U16X4, dict()),
    ("modular_squeeze", "modular", dict(squeeze=1, tree=1), U8X4, dict()),
    ("keep_alpha", "vardct", dict(alpha=1), U8X4, dict(alpha=True)),
    ("restoration", "vardct", dict(fullheader=1, gab=1, epf=2), U8X4, dict(restoration=1)),
    ("ycbcr_420", "vardct", dict(ycbcr=1, subsampling="420"), U8X4, dict(ycbcr=True)),
]


@pytest.mark.parametrize("o", [6, 7])
@pytest.mark.parametrize("w,h", SIZES, ids=["%dx%d" % s for s in SIZES])
@pytest.mark.parametrize("name,mode,opts,fmt,how", FRAME_CASES, ids=[c[0] for c in FRAME_CASES])
def test_every_kind_of_frame(gpu, name, mode, opts, fmt, how, w, h, o):
    seed = 3 if name == "restoration" else SEED
    full, turned, said = stored_oriented_stored(gpu, synth(mode, w, h, seed, orientation=o, **opts), o, fmt, **how)
    check(full, turned, said, o)
    if name in ("keep_alpha", "modular_alpha", "modular_alpha_u16"):
        assert full[..., 3].min() < np.iinfo(full.dtype).max, "the alpha channel is there"


def test_device_buffer_rows_and_stride(gpu):
    """j40hip_frame_decode into device memory: a stride below the oriented rows is "rnge" before anything is launched; nothing
    outside the ow pixels of each of the oh rows is written"""
    import torch
    w, h, o = 779, 517, 6
    fr = open_frame(gpu, synth("vardct", w, h, SEED, orientation=o))
    err, full = fr.decode_to_host()
    assert err == "" and fr.set_orientation(1) == ""
    ow, oh = h, w
    stride = 4 * ow + 64
    buf = torch.full((oh + 8, stride), 0xA5, dtype=torch.uint8, device="cuda:0")
    stream = torch.cuda.current_stream().cuda_stream
    with pytest.raises(gpu.J40Error) as e:
        fr.decode(buf.data_ptr() + 4 * stride, 4 * ow - 4, stream)
    assert e.value.code == "rnge"
    torch.cuda.synchronize()
    assert bool((buf == 0xA5).all()), "a refused decode wrote something"
    fr.decode(buf.data_ptr() + 4 * stride, stride, stream)
    torch.cuda.synchronize()
    assert fr.status() == ""
    host = buf.cpu().numpy()
    assert (host[:4] == 0xA5).all() and (host[4 + oh:] == 0xA5).all() and (host[4:4 + oh, 4 * ow:] == 0xA5).all()
    assert np.array_equal(np.ascontiguousarray(host[4:4 + oh, :4 * ow]).reshape(oh, ow, 4), orient(full, o))
    ms = fr.decode_timed(buf.data_ptr() + 4 * stride, stride, stream)     # the timed entry goes the same way
    torch.cuda.synchronize()
    assert np.array_equal(np.ascontiguousarray(buf.cpu().numpy()[4:4 + oh, :4 * ow]).reshape(oh, ow, 4), orient(full, o)), ms
    fr.close()


# ---------------------------------------------------------------- composition: the orientation is applied last

@pytest.mark.parametrize("o", [6, 4])
@pytest.mark.parametrize("mode,opts,how", [("vardct", dict(), dict()), ("modular", dict(alpha=1), dict()), ("vardct", dict(alpha=1), dict(alpha=True))], ids=["vardct", "modular", "keep_alpha_staged"])
def test_scaled_and_oriented(gpu, mode, opts, how, o):
    w, h = SIZES[0]
    fr = open_frame(gpu, synth(mode, w, h, SEED, orientation=o, **opts), **how)
    err, full = fr.decode_to_host()
    assert err == "" and all_differ(full)
    assert fr.set_orientation(1) == ""
    for k in (1, 2):
        assert fr.set_scale(k) == ""
        err, px = fr.decode_to_host()
        assert err == ""
        small = box(full, k)
        assert np.array_equal(px, orient(small, o)), k
        q = fr.orientation()
        assert (q["went_through_k_orient"], q["staging_bytes"]) == (1, 4 * small.shape[0] * small.shape[1])
    # (w and h are no multiples of 4: box(orient(full)) has other edge cells for o = 6 -- the order matters)
    if o == 6:
        assert not np.array_equal(orient(box(full, 2), o), box(orient(full, o), 2))
    fr.close()


@pytest.mark.parametrize("o", [6, 4])
@pytest.mark.parametrize("mode", ["vardct", "modular"])
def test_region_and_oriented(gpu, mode, o):
    w, h = SIZES[0]
    data = synth(mode, w, h, SEED, orientation=o)
    fr = open_frame(gpu, data)
    err, full = fr.decode_to_host()
    assert err == ""
    shown = orient(full, o)
    x0, y0, rw, rh = 200, 190, 150, 120     # straddles the four groups that meet at (256, 256)
    assert fr.set_region(x0, y0, rw, rh) == "" and fr.set_orientation(1) == ""
    assert fr.region()["gcols"] == 2 and fr.region()["grows"] == 2
    err, px = fr.decode_to_host()
    assert err == "" and np.array_equal(px, orient(full[y0:y0 + rh, x0:x0 + rw], o))
    q = fr.orientation()
    assert (q["went_through_k_orient"], q["staging_bytes"]) == (1, 4 * rw * rh)
    code, disp = fr.orient_rect((x0, y0, rw, rh), to_stored=False)
    assert code == "" and np.array_equal(px, shown[disp[1]:disp[1] + disp[3], disp[0]:disp[0] + disp[2]]), "a region is a crop of the oriented picture"
    fr.close()
    # decode_region(..., orient=True): the rectangle in displayed coordinates
    dx, dy, dw, dh = 180, 210, 130, 101
    err, px = gpu.decode_region(data, dx, dy, dw, dh, orient=True)
    assert err == "" and np.array_equal(px, shown[dy:dy + dh, dx:dx + dw])
    assert gpu.decode_region(data, 0, 0, shown.shape[1] + 1, 1, orient=True)[0] == "rnge"
    # ... and decode(..., orient=True) the whole picture
    err, px = gpu.decode(data, orient=True)
    assert err == "" and np.array_equal(px, shown)


@pytest.mark.parametrize("o", [6, 4])
@pytest.mark.parametrize("lf_only", [False, True], ids=["full_frame", "lf_only"])
def test_lf_preview_oriented(gpu, o, lf_only):
    import torch
    w, h = SIZES[0]
    fr = gpu.Frame(synth("vardct", w, h, SEED, orientation=o), lf_only=lf_only)
    fr.upload(0)
    assert fr.set_orientation(0) == ""
    stored = fr.decode_lf_to_host()
    assert stored.shape == ((h + 7) // 8, (w + 7) // 8, 4) and all_differ(stored)
    assert fr.set_orientation(1) == ""
    turned = fr.decode_lf_to_host()
    assert np.array_equal(turned, orient(stored, o))
    # j40hip_frame_decode_lf into device memory, guard bytes behind the rows
    oh, ow = turned.shape[:2]
    stride = 4 * ow + 32
    buf = torch.full((oh, stride), 0xA5, dtype=torch.uint8, device="cuda:0")
    stream = torch.cuda.current_stream().cuda_stream
    with pytest.raises(gpu.J40Error) as e:
        fr.decode_lf(buf.data_ptr(), 4 * ow - 4, stream)
    assert e.value.code == "rnge"
    fr.decode_lf(buf.data_ptr(), stride, stream)
    torch.cuda.synchronize()
    host = buf.cpu().numpy()
    assert (host[:, 4 * ow:] == 0xA5).all()
    assert np.array_equal(np.ascontiguousarray(host[:, :4 * ow]).reshape(oh, ow, 4), turned)
    q = fr.orientation()
    assert (q["went_through_k_orient"], q["staging_bytes"]) == (1, 4 * stored.shape[0] * stored.shape[1])
    # the many-frames preview writes stored order: refused while the orientation is in force, served again with the mode off
    assert gpu.frames_decode_lf([fr], [buf.data_ptr()], [stride], stream) == "Uor?"
    assert fr.set_orientation(0) == ""
    buf2 = torch.full((stored.shape[0], 4 * stored.shape[1]), 0xA5, dtype=torch.uint8, device="cuda:0")
    assert gpu.frames_decode_lf([fr], [buf2.data_ptr()], [4 * stored.shape[1]], stream) == ""
    torch.cuda.synchronize()
    assert np.array_equal(buf2.cpu().numpy().reshape(stored.shape), stored)
    fr.close()


def test_unaligned_destination(gpu):
    """pointer and stride need no alignment, as in stored order: pixels that are not aligned to their size still arrive, and nothing
    else is written"""
    import torch
    w, h = 264, 520
    for o, fmt, pb in ((6, U8X4, 4), (3, U16X4, 8)):
        fr = open_frame(gpu, synth("vardct", w, h, SEED, orientation=o), fmt)
        err, full = fr.decode_to_host()
        assert err == "" and fr.set_orientation(1) == ""
        want = orient(full, o)
        oh, ow = want.shape[:2]
        stride = pb * ow + 3
        buf = torch.full((oh * stride + 16,), 0xA5, dtype=torch.uint8, device="cuda:0")
        fr.decode(buf.data_ptr() + 1, stride, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        assert fr.status() == ""
        host = buf.cpu().numpy()
        rows = host[1:1 + oh * stride].reshape(oh, stride)
        assert host[0] == 0xA5 and (host[1 + oh * stride:] == 0xA5).all() and (rows[:, pb * ow:] == 0xA5).all()
        assert np.array_equal(np.ascontiguousarray(rows[:, :pb * ow]).view(full.dtype).reshape(oh, ow, 4), want), (o, fmt)
        fr.close()


# ---------------------------------------------------------------- refusals

@pytest.mark.parametrize("mode,w,h", [("vardct", 779, 517), ("modular", 601, 303)])
def test_group_range_and_orientation_exclude_each_other(gpu, mode, w, h):
    """a partial group range writes its own rectangles of the caller's image: with an orientation in force there is no whole
    stored-order image to turn. Whichever setter comes second is refused, the decode entries refuse the combination too, and nothing
    is written"""
    import torch
    o = 6
    fr = open_frame(gpu, synth(mode, w, h, SEED, orientation=o))
    n = fr.info["num_groups"]
    err, full = fr.decode_to_host()
    assert err == "" and n >= 4
    fr.set_group_range(1, 2)
    assert fr.set_orientation(1) == "Uor?" and fr.orientation()["applied"] == 0, "a refused call leaves the frame as it was"
    stream = torch.cuda.current_stream().cuda_stream
    buf = torch.full((h, w * 4), 0xA5, dtype=torch.uint8, device="cuda:0")
    fr.decode(buf.data_ptr(), w * 4, stream)              # stored order with the range: served as ever, its rectangles only
    torch.cuda.synchronize()
    part = buf.cpu().numpy().reshape(h, w, 4)
    wrote = (part != 0xA5).any(axis=-1)
    assert wrote.any() and not wrote.all() and np.array_equal(part[wrote], full[wrote])
    fr.set_group_range(0, n)                              # the whole range is no range
    assert fr.set_orientation(1) == ""
    with pytest.raises(gpu.J40Error) as e:
        fr.set_group_range(1, 2)
    assert e.value.code == "Uor?"
    err, px = fr.decode_to_host()
    assert err == "" and np.array_equal(px, orient(full, o)), "the refused range left the frame whole"
    fr.close()
    # no orientation to apply (o = 1): mode 1 and a range go together
    fr = open_frame(gpu, synth(mode, w, h, SEED))
    fr.set_group_range(1, 2)
    assert fr.set_orientation(1) == ""
    fr.close()


GROUP_RANGE_CHILD = r"""
import sys
import numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import torch
import j40_amd
from streams import synth
w, h = 779, 517
fr = j40_amd.Frame(synth("vardct", w, h, 7, orientation=6))
fr.upload(0)
assert fr.orientation()["applied"] == 1
codes = []
try:
    fr.set_group_range(1, 2)
except j40_amd.J40Error as e:
    codes.append(e.code)
fr.set_orientation(0)
fr.set_group_range(1, 2)
fr.set_orientation(-1)            # the environment puts the orientation in force behind the range
buf = torch.full((w, h * 4), 0xA5, dtype=torch.uint8, device="cuda:0")
try:
    fr.decode(buf.data_ptr(), h * 4, torch.cuda.current_stream().cuda_stream)
except j40_amd.J40Error as e:
    codes.append(e.code)
torch.cuda.synchronize()
codes.append(fr.decode_to_host()[0])
assert bool((buf == 0xA5).all()), "a refused decode wrote something"
print(",".join(codes))
fr.close()
j40_amd.shutdown()
"""


def test_group_range_under_the_environment_variable(gpu):
    """J40HIP_ORIENT=1 with mode -1: the setter refuses a range, and a range that got in while the mode was off is refused by the
    decode entries, before anything is written"""
    env = dict(os.environ, J40HIP_ORIENT="1")
    r = subprocess.run([sys.executable, "-c", GROUP_RANGE_CHILD, ROOT], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    assert r.stdout.strip().splitlines()[-1] == "Uor?,Uor?,Uor?"


def test_batch_refuses_and_the_frame_still_decodes(gpu):
    w, h, o = 264, 520, 6
    fr = open_frame(gpu, synth("vardct", w, h, SEED, orientation=o))
    err, full = fr.decode_to_host()
    assert err == "" and fr.set_orientation(1) == ""
    with pytest.raises(gpu.J40Error) as e:
        gpu.Batch([fr])
    assert e.value.code == "Uor?"
    assert fr.orientation()["applied"] == 1, "a refused call leaves the frame as it was"
    err, px = fr.decode_to_host()
    assert err == "" and np.array_equal(px, orient(full, o))
    assert fr.set_orientation(0) == ""
    batch = gpu.Batch([fr])      # stored order: served
    batch.close()
    fr.close()


def test_sequence_frame_refuses(gpu):
    seq = gpu.Sequence(synth("vardct", 300, 200, SEED, passes=2, frames=2, crops=";37,21,130,90", orientation=6))
    f = seq.frame(0)
    assert f.orientation()["orientation"] == 6
    assert f.set_orientation(1) == "Uor?" and f.orientation()["applied"] == 0
    seq.upload(0)
    err, px = seq.next_to_host()
    assert err == "" and px.shape[:2] == (200, 300), "the playback writes stored order"
    seq.close()


def test_pipeline_writes_stored_order(gpu):
    w, h = 520, 264
    pipe = gpu.Pipeline(device=0, host_threads=2, batch_frames=4, max_in_flight=2)
    err, plain = pipe.run(synth("vardct", w, h, SEED))
    assert err == ""
    err, px = pipe.run(synth("vardct", w, h, SEED, orientation=6))
    assert err == "" and px.shape == (h, w, 4) and np.array_equal(px, plain)
    pipe.close()


# ---------------------------------------------------------------- the public API

CHILD = r"""
import os, sys
import numpy as np
sys.path.insert(0, sys.argv[1])
import j40_amd
data = open(sys.argv[2], "rb").read()
out = {}
def one(tag, fmt):
    err, px = j40_amd.decode(data, fmt)
    out[tag + "_err"] = np.frombuffer(err.encode().ljust(4), np.uint8)
    if px is not None:
        out[tag] = px.copy()
one("u8", j40_amd.J40_U8X4)
one("u16", j40_amd.J40_U16X4)
os.environ["J40HIP_FRAMES"] = "1"; one("frames", j40_amd.J40_U8X4)
np.savez(sys.argv[3], **out)
j40_amd.shutdown()
"""


@pytest.mark.parametrize("serve", [0, 1], ids=["latency_path", "serve_policy_1"])
def test_public_api_in_a_fresh_process(gpu, tmp_path, serve):
    w, h, o = 779, 517, 8
    data = synth("vardct", w, h, SEED, orientation=o)
    fulls = {}
    for tag, fmt in (("u8", U8X4), ("u16", U16X4)):
        fr = open_frame(gpu, data, fmt)
        err, fulls[tag] = fr.decode_to_host()
        assert err == ""
        fr.close()
    path = str(tmp_path / "in.jxl")
    with open(path, "wb") as fp:
        fp.write(data)
    got = {}
    for var in ("1", None):
        env = dict(os.environ)
        for k in ("J40HIP_FRAMES", "J40HIP_ORIENT", "J40HIP_SERVE"):
            env.pop(k, None)
        if var:
            env["J40HIP_ORIENT"] = var
        if serve:
            env["J40HIP_SERVE"] = "1"
        res = str(tmp_path / ("out%s.npz" % var))
        r = subprocess.run([sys.executable, "-c", CHILD, ROOT, path, res], env=env, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
        got[var] = np.load(res)
    code = lambda g, tag: bytes(g[tag + "_err"]).decode().strip()
    on, off = got["1"], got[None]
    for tag in ("u8", "u16"):
        assert code(on, tag) == "" and on[tag].shape == (w, h, 4), "width and height swapped"
        assert np.array_equal(on[tag], orient(fulls[tag], o))
        assert code(off, tag) == "" and np.array_equal(off[tag], fulls[tag]), "without the variable nothing changes"
    assert code(on, "frames") == "Uor?" and "frames" not in on
    assert code(off, "frames") == "" and np.array_equal(off["frames"], fulls["u8"])


# ---------------------------------------------------------------- bookkeeping

def test_bookkeeping_without_an_orientation(gpu):
    """o = 1 with the mode on, and any o with the mode off: no staging image is taken"""
    w, h = 264, 520
    fr = open_frame(gpu, synth("vardct", w, h, SEED))
    assert fr.set_orientation(1) == ""
    err, full = fr.decode_to_host()
    q = fr.orientation()
    assert err == "" and (q["orientation"], q["applied"], q["went_through_k_orient"], q["staging_bytes"]) == (1, 0, 0, 0)
    fr.close()
    fr = open_frame(gpu, synth("vardct", w, h, SEED, orientation=5))
    err, px = fr.decode_to_host()         # mode -1, no J40HIP_ORIENT: stored order
    q = fr.orientation()
    assert err == "" and np.array_equal(px, full) and (q["applied"], q["went_through_k_orient"], q["staging_bytes"]) == (0, 0, 0)
    fr.close()
