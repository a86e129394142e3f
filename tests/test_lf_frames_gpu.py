"""LF frames on the device (include/j40hip.h, J40HIP_SEQ_LFFRAME; k_lf_from_frame, k_lf_frame_bctx): a stream whose LF image is a frame of
its own decodes, byte for byte, to what its twin decodes to -- the ordinary one-frame stream whose LfCoefficients are the flat LF
frame's integers, a stream the reference decodes and this library's decode of which is held against the reference at the suite's bar
(within one level). Why the twin is an exact pin: a DCT8 block with only its (0, 0) coefficient comes out of the inverse transform
exactly flat at that value, so a flat LF frame's samples are exactly (float) q * mult_lf -- what k_lf_dequant_smooth computes for the
twin without smoothing -- and the LF indices follow (tests/test_lf_frames.py checks both steps on the CPU build).
What an LF frame stores is pinned to the single-frame decode of the same frame written alone; a real LF picture is held against the
ordinary encode of the same source by PSNR. tests/test_lf_frames.py has the index, the refusals and the CPU build."""
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

from streams import synth
from lf_streams import SEED, WIDE, TALL, TWO_LEVELS, lf_stream, lf_twin, lf_stats, lf_size

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U8X4, U16X4 = 0x0F33, 0x0F35


@pytest.fixture(scope="module")
def gpu(built):
    import j40_amd
    assert j40_amd.device_count() > 0, "the gpu tests need a HIP device"
    assert (j40_amd.J40_U8X4, j40_amd.J40_U16X4) == (U8X4, U16X4)
    return j40_amd


def decode_twin(gpu, data, fmt=U8X4, restoration=None, region=None):
    fr = gpu.Frame(data)
    if restoration is not None:
        fr.set_restoration(restoration)
    if region is not None:
        assert fr.set_region(*region) == ""
    fr.set_output_format(fmt)
    fr.upload(0)
    err, px = fr.decode_to_host()
    fr.close()
    assert err == ""
    return px


def play(gpu, data, fmt=U8X4, restoration=None):
    """the one displayed canvas of an LF-frame stream; the sequence stays open for the caller"""
    seq = gpu.Sequence(data, lf_frames=True)
    seq.set_output_format(fmt)
    if restoration is not None:
        for k in range(seq.num_frames):
            seq.frame(k).set_restoration(restoration)
    seq.upload(0)
    err, px = seq.next_to_host()
    assert err == "" and seq.status() == ("", -1)
    assert seq.next_to_host()[0] == "Useq"
    return seq, px


_twins = {}


def twin_pixels(gpu, ref, size, opts):
    """the twin's decode, held against the reference once"""
    key = (size, tuple(sorted(opts.items())))
    if key not in _twins:
        data = lf_twin(size, **opts)
        px = decode_twin(gpu, data)
        rerr, want = ref.decode(data)
        assert rerr == ""
        d = int(np.abs(px[..., :3].astype(np.int32) - want[..., :3].astype(np.int32)).max())
        print("twin against the reference: max |delta| =", d)
        assert d <= 1 and np.array_equal(px[..., 3], want[..., 3])
        _twins[key] = px
    return _twins[key]


FLAT_CASES = [("default", WIDE, dict()), ("bctx", WIDE, dict(bctx=1)), ("two_passes", WIDE, dict(passes=2)),
              ("tall_default", TALL, dict()), ("tall_bctx", TALL, dict(bctx=1)), ("tall_two_passes", TALL, dict(passes=2))]


@pytest.mark.parametrize("name,size,opts", FLAT_CASES, ids=[c[0] for c in FLAT_CASES])
def test_flat_lf_frame_equals_its_twin(gpu, ref, name, size, opts):
    """varblocks up to 64 x 64 (maxlog=6, the default mix with every transform forced once)"""
    if opts.get("bctx"):
        assert lf_stats(size, **opts)["lfidx_distinct"] > 1   # some LF threshold splits the cells: k_lf_frame_bctx has work
    want = twin_pixels(gpu, ref, size, opts)
    seq, px = play(gpu, lf_stream(size, **opts))
    seq.close()
    assert px.shape == want.shape == (size[1], size[0], 4)
    assert np.array_equal(px, want)
    assert np.array_equal(gpu.decode_frames(lf_stream(size, **opts), lf_frames=True)[0][0][0], want)
    err, px = gpu.decode(lf_stream(size, **opts), lf_frames=True)
    assert err == "" and np.array_equal(px, want)


def test_two_levels_equal_their_twin(gpu, ref):
    opts = dict(lflevels=2, bctx=1)
    assert lf_stats(TWO_LEVELS, **opts)["lfidx_distinct"] > 1
    want = twin_pixels(gpu, ref, TWO_LEVELS, opts)
    seq, px = play(gpu, lf_stream(TWO_LEVELS, **opts))
    assert np.array_equal(px, want)
    # the level-1 picture is the level-2 picture, every sample over 8 x 8
    w1, h1 = lf_size(TWO_LEVELS, 1)
    w2, h2 = lf_size(TWO_LEVELS, 2)
    coarse, fine = seq.read_lf_slot(2, w2, h2), seq.read_lf_slot(1, w1, h1)
    seq.close()
    assert np.array_equal(fine.view(np.uint32), np.repeat(np.repeat(coarse, 8, axis=1), 8, axis=2)[:, :h1, :w1].view(np.uint32))


def test_u16_output_equals_the_twin(gpu):
    opts = dict(bctx=1)
    seq, px = play(gpu, lf_stream(WIDE, **opts), fmt=U16X4)
    seq.close()
    want = decode_twin(gpu, lf_twin(WIDE, **opts), fmt=U16X4)
    assert px.dtype == np.uint16 and np.array_equal(px, want)


def test_main_frame_filters_equal_the_twin(gpu):
    """Gaborish and the edge-preserving filter signalled by the main frame, run by the restoration mode: they sit behind the LLF stage"""
    opts = dict(gab=1, epf=2)
    seq, px = play(gpu, lf_stream(WIDE, **opts), restoration=1)
    seq.close()
    want = decode_twin(gpu, lf_twin(WIDE, **opts), restoration=1)
    plain = decode_twin(gpu, lf_twin(WIDE, **opts), restoration=0)
    assert np.array_equal(px, want) and not np.array_equal(px, plain)


def test_region_across_the_lfgroup_seam_equals_the_twin(gpu):
    """the main frame's handle keeps its LF source after the playback: a rectangle over the seam between its two LfGroups (x = 2048)"""
    opts = dict(bctx=1)
    region = (2000, 9, 57, 52)
    seq, px = play(gpu, lf_stream(WIDE, **opts))
    fr = seq.frame(1)
    assert fr.set_region(*region) == ""
    err, part = fr.decode_to_host()
    assert err == ""
    seq.close()
    want = decode_twin(gpu, lf_twin(WIDE, **opts), region=region)
    x, y, w, h = region
    assert part.shape == (h, w, 4) and np.array_equal(part, want) and np.array_equal(part, px[y:y + h, x:x + w])


@pytest.mark.parametrize("size", [WIDE, TALL], ids=["2060x70", "70x2060"])
def test_scale_equals_the_twin(gpu, size):
    """scale=1: the 1:2 image of the still, from the main frame's handle once the LF frame has played -- what the twin gives at that scale"""
    opts = dict(bctx=1)
    err, px = gpu.decode(lf_stream(size, **opts), lf_frames=True, scale=1)
    err2, want = gpu.decode(lf_twin(size, **opts), scale=1)
    assert err == "" and err2 == "" and px.shape == want.shape == ((size[1] + 1) // 2, (size[0] + 1) // 2, 4)
    assert np.array_equal(px, want)
    err, px = gpu.decode(lf_stream(size, **opts), gpu.J40_U16X4, lf_frames=True, scale=2)
    err2, want = gpu.decode(lf_twin(size, **opts), gpu.J40_U16X4, scale=2)
    assert err == "" and err2 == "" and px.dtype == np.uint16 and np.array_equal(px, want)


@pytest.mark.parametrize("orientation", [3, 6], ids=["turned_180", "transposed"])
def test_orient_equals_the_twin(gpu, orientation):
    """orient=True: the still in the orientation its image header carries; with a scale on top"""
    opts = dict(bctx=1, orientation=orientation)
    plain = gpu.decode(lf_stream(WIDE, **opts), lf_frames=True)[1]
    err, px = gpu.decode(lf_stream(WIDE, **opts), lf_frames=True, orient=True)
    err2, want = gpu.decode(lf_twin(WIDE, **opts), orient=True)
    assert err == "" and err2 == "" and np.array_equal(px, want)
    assert px.shape == ((70, 2060, 4) if orientation == 3 else (2060, 70, 4)) and not np.array_equal(px, plain)
    err, px = gpu.decode(lf_stream(WIDE, **opts), lf_frames=True, orient=True, scale=1)
    err2, want = gpu.decode(lf_twin(WIDE, **opts), orient=True, scale=1)
    assert err == "" and err2 == "" and np.array_equal(px, want)


def test_playback_and_handle_rules(gpu):
    """The main frame's handle takes a scale and the orientation only for decodes of its own: the playback refuses it while either is
    set, an LF frame's handle refuses both, and a rewind unbinds the LF source (a decode of its own is then "lfno" until the playback
    has filled the slot again)"""
    data = lf_stream(WIDE, orientation=6)
    seq, px = play(gpu, data)
    lf, main = seq.frame(0), seq.frame(1)
    assert lf.set_scale(1) == "Usc?" and lf.set_orientation(1) == "Uor?"
    assert main.set_scale(1) == ""
    seq.rewind()
    assert seq.next_to_host()[0] == "Usc?"
    assert main.set_scale(0) == "" and main.set_orientation(1) == ""
    seq.rewind()
    assert seq.next_to_host()[0] == "Uor?"
    assert main.set_orientation(0) == ""
    seq.rewind()
    assert main.decode_to_host()[0] == "lfno"
    err, again = seq.next_to_host()
    assert err == "" and np.array_equal(again, px)
    assert main.decode_to_host()[0] == ""
    seq.close()


@pytest.mark.parametrize("mode", [1, 0], ids=["filters_run", "filters_off"])
def test_stored_planes_are_the_single_frame_decodes(gpu, mode):
    """The LF slot holds what j40hip_frame_read_xyb holds for the same frame decoded alone (the generator's only=0 stream): the filtered
    planes (stage 1) where the restoration mode runs the filters the LF frame signals, else the planes as the inverse transforms left
    them (stage 0). Bit for bit."""
    opts = dict(lfkind="picture", forward=1, lfgab=1, lfepf=1)
    w, h = lf_size(WIDE)
    alone = gpu.Frame(lf_stream(WIDE, only=0, **opts))
    assert (alone.width, alone.height) == (w, h)
    alone.set_restoration(1)
    alone.upload(0)
    assert alone.decode_to_host()[0] == ""
    before, after = alone.read_xyb(0), alone.read_xyb(1)
    alone.close()
    assert not np.array_equal(before, after)
    seq, _ = play(gpu, lf_stream(WIDE, **opts), restoration=mode)
    slot = seq.read_lf_slot(1, w, h)
    seq.close()
    assert np.array_equal(slot.view(np.uint32), (after if mode else before).view(np.uint32))


def psnr(a, b):
    d = a[..., :3].astype(np.float64) - b[..., :3].astype(np.float64)
    return 10 * np.log10(255.0 ** 2 / np.mean(d * d))


def test_lf_picture_against_the_ordinary_encode(gpu):
    """A real LF picture: the LF frame forward-codes the 8 x 8 cell means of the procedural picture (lfkind=picture forward=1), the main
    frame codes the same HF as the ordinary forward=1 stream of that picture. Both decodes against the generator's source (dumpsrc);
    the ordinary stream is the yardstick. A misplaced cell, a swapped channel or a wrong scale costs far more than 10 dB; the bound is
    3 dB. Measured on an MI355X: ordinary stream 36.65 dB, LF-frame stream 34.62 dB. The 2.03 dB between them are the generator's, not
    the decoder's: a frame with use_lf_frame is written without chroma from luma (so that the LF frame can hold the B samples
    themselves), and the ordinary stream written that way (nocfl=1) decodes to 34.90 dB in the reference; the remaining 0.28 dB are
    the LF frame's own coding error (HfMul 64) and the missing adaptive LF smoothing. With the LF frame at the main frame's HfMul and
    B - Y in a plane of its own the same stream measured 30.81 dB, which the bound refused."""
    with tempfile.TemporaryDirectory() as d:
        src_path = os.path.join(d, "src.rgb")   # (not through synth(): its cache is keyed by the options, and this path is new every time)
        subprocess.run([os.path.join(ROOT, "build", "jxlsynth"), "vardct", str(WIDE[0]), str(WIDE[1]), str(SEED), os.path.join(d, "o.jxl"), "forward=1", "dumpsrc=" + src_path],
                       check=True, stderr=subprocess.DEVNULL)
        src = np.fromfile(src_path, np.uint8).reshape(WIDE[1], WIDE[0], 3)
        with open(os.path.join(d, "o.jxl"), "rb") as fp:
            ordinary = fp.read()
    seq, px = play(gpu, lf_stream(WIDE, lfkind="picture", forward=1))
    seq.close()
    a, b = psnr(decode_twin(gpu, ordinary), src), psnr(px, src)
    print("PSNR against the source: ordinary stream %.2f dB, LF-frame stream %.2f dB" % (a, b))
    assert b > a - 3.0


CHILD = """
import sys
sys.path.insert(0, %r)
import numpy as np
import j40_amd
data = open(sys.argv[1], "rb").read()
for fmt, name in ((j40_amd.J40_U8X4, "u8"), (j40_amd.J40_U16X4, "u16")):
    err, px = j40_amd.decode(data, fmt)
    print(name, repr(err))
    if px is not None:
        np.save(sys.argv[2] + name + ".npy", px)
j40_amd.shutdown()
"""


def test_public_api_in_a_child_process(gpu, ref):
    """the ten-function API (j40_from_memory .. j40_next_frame, what j40_amd.decode() walks): "TODO" as ever without J40HIP_LFFRAME=1,
    the twin's picture with it"""
    opts = dict(bctx=1)
    want = twin_pixels(gpu, ref, WIDE, opts)
    want16 = decode_twin(gpu, lf_twin(WIDE, **opts), fmt=U16X4)
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "s.jxl")
        with open(path, "wb") as fp:
            fp.write(lf_stream(WIDE, **opts))
        env = {k: v for k, v in os.environ.items() if k not in ("J40HIP_LFFRAME", "J40HIP_FRAMES")}
        out = subprocess.run([sys.executable, "-c", CHILD % ROOT, path, os.path.join(d, "off_")], env=env, check=True, stdout=subprocess.PIPE, timeout=120).stdout.decode()
        assert out.split() == ["u8", "'TODO'", "u16", "'TODO'"] and not os.path.exists(os.path.join(d, "off_u8.npy"))
        out = subprocess.run([sys.executable, "-c", CHILD % ROOT, path, os.path.join(d, "on_")], env=dict(env, J40HIP_LFFRAME="1"), check=True, stdout=subprocess.PIPE, timeout=120).stdout.decode()
        assert out.split() == ["u8", "''", "u16", "''"]
        assert np.array_equal(np.load(os.path.join(d, "on_u8.npy")), want)
        assert np.array_equal(np.load(os.path.join(d, "on_u16.npy")), want16)
