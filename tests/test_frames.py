"""Frame sequences (j40hip_sequence, include/j40hip.h): animations and layered stills, without a device.

The reference decodes one frame. A coded frame of a sequence, written alone as a last frame under the same image header (the
generator's only=k), is a stream it does decode -- crop-sized, the crop's offsets ignored -- and putting a rectangle onto a canvas is
integer work numpy restates. Here: the index over headers and TOCs (every field, for animations and layers, bare and in both container
forms), that frame k of the N-frame stream carries the section bytes of the only=k stream and parses to the same tables, what is
refused and what damage does, and the composition's device functions (device/compose_dev.h) run on the CPU, lane by lane, by
build/libhostsim_compose.so (tests/hostsim/compose_sim.cpp). tests/test_frames_gpu.py decodes."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

from streams import synth, ROOT, SYNTH

U8X4, U16X4 = 0x0F33, 0x0F35
SEED = 7
W, H = 300, 200
CROPS = [None, (37, 21, 130, 90), (-20, -10, 100, 80), (250, 150, 100, 100)]   # full; inside; off the top-left; beyond the bottom-right
DURATIONS = [3, 0, 2, 1]
# Modular: two groups across at groupshift=7, an alpha channel. VarDCT: two passes, so that a frame of one group has several sections (the
# generator does not write the single-section VarDCT frame, whose reading order in the reference is special)
MODES = {"modular": dict(groupshift=7, alpha=1), "vardct": dict(passes=2)}


def crops_opt(crops):
    return ";".join("" if c is None else "%d,%d,%d,%d" % c for c in crops)


def seq_opts(mode, anim, crops=CROPS, durations=DURATIONS, **more):
    o = dict(MODES[mode], frames=len(crops), crops=crops_opt(crops))
    if anim:
        o.update(anim=1, durations=",".join(str(d) for d in durations))
    o.update(more)
    return o


def only_stream(mode, w, h, opts, k):
    """coded frame k alone, as a last frame under the same image header (a stream the reference decodes)"""
    return synth(mode, w, h, SEED, **dict({kk: v for kk, v in opts.items() if kk != "container"}, only=k))


def generator_rows(mode, w, h, opts):
    """what the generator says it wrote (stats=1): {"frames", "shown", "saved_slots", "written": [{"frame", "first_section", "end"}]}"""
    out = os.path.join(ROOT, "build", "streams", "stats_%d.jxl" % os.getpid())
    r = subprocess.run([SYNTH, mode, str(w), str(h), str(SEED), out, "stats=1"] + ["%s=%s" % kv for kv in sorted(opts.items())], check=True, capture_output=True)
    os.remove(out)
    return json.loads(r.stdout)


def expected_flags(anim, n, durations):
    shown = [bool(anim and durations[k] > 0) or k == n - 1 for k in range(n)]
    saved = [k != n - 1 and (not anim or durations[k] == 0) for k in range(n)]   # (save_as_reference is 0 throughout)
    return shown, saved


def assert_same_sections(seq_data, info, mode, w, h, opts, k):
    """frame k's section bytes in the N-frame stream are the only=k stream's"""
    only = only_stream(mode, w, h, opts, k)
    rows = generator_rows(mode, w, h, dict({kk: v for kk, v in opts.items() if kk != "container"}, only=k))
    assert rows["frames"] == 1 and rows["written"][0]["frame"] == k and rows["written"][0]["end"] == len(only)
    a = seq_data[info["first_section"]:info["end"]]
    b = only[rows["written"][0]["first_section"]:]
    assert len(a) > 0 and a == b, "frame %d: the sequence and the only= stream carry different sections" % k


# ---------------------------------------------------------------- the index

@pytest.mark.parametrize("container", [0, 1, 2])
@pytest.mark.parametrize("anim", [1, 0], ids=["animation", "layers"])
@pytest.mark.parametrize("mode", ["modular", "vardct"])
def test_index_rows(built, mode, anim, container):
    import j40_amd
    opts = seq_opts(mode, anim)
    bare = synth(mode, W, H, SEED, **opts)
    data = synth(mode, W, H, SEED, **dict(opts, container=container)) if container else bare
    seq = j40_amd.Sequence(data)
    n = len(CROPS)
    shown, saved = expected_flags(anim, n, DURATIONS)
    assert seq.num_frames == n and seq.num_shown == sum(shown)
    assert (seq.width, seq.height) == (W, H)
    assert (seq.tps, seq.loops) == (((10, 1), 0) if anim else ((0, 0), 0))
    at = None
    for k in range(n):
        i = seq.frame_info(k)
        x0, y0, w, h = CROPS[k] or (0, 0, W, H)
        assert (i["x0"], i["y0"], i["w"], i["h"]) == (x0, y0, w, h)
        assert i["duration"] == (DURATIONS[k] if anim else 0)
        assert i["is_last"] == (k == n - 1) and i["shown"] == shown[k] and i["saved"] == saved[k]
        assert (i["type"], i["blend"], i["src"], i["save_as_reference"], i["code"]) == (0, 0, 0, 0, "")
        assert (i["tps_num"], i["tps_den"], i["loops"], i["canvas_w"], i["canvas_h"]) == ((10, 1, 0, W, H) if anim else (0, 0, 0, W, H))
        assert i["offset"] < i["first_section"] < i["end"]
        assert at is None or i["offset"] == at, "a frame starts where the one before it ends"
        at = i["end"]
        assert_same_sections(bare, i, mode, W, H, opts, k)   # (offsets count in the codestream, container or not)
    assert at == len(bare)
    gen = generator_rows(mode, W, H, opts)
    assert (gen["frames"], gen["shown"], gen["saved_slots"]) == (n, sum(shown), 1 if any(saved) else 0)
    assert [(r["first_section"], r["end"]) for r in gen["written"]] == [(seq.frame_info(k)["first_section"], seq.frame_info(k)["end"]) for k in range(n)]
    assert seq.frame_info(n)["end"] == 0 and seq.frame_info(-1)["end"] == 0   # out of range: zeros
    seq.close()


def tables_of(fr):
    """what the host parse made of a frame, as comparable Python values"""
    t = dict(info=fr.info, sections=fr.section_sizes().tolist())
    if fr.info["is_modular"]:
        planes = [fr.global_plane(c) for c in range(3 + fr.info["num_extra_channels"])]
        t["planes"] = [None if p is None else (p.shape, p.tobytes()) for p in planes]
        t["kernels"] = (fr.coop_sections(), fr.quad_sections(), fr.split_sections())
        return t
    t["bctx"] = fr.block_ctx_map().tobytes()
    t["dq"] = [fr.dq_matrix(i).tobytes() for i in range(17)]
    for gg in range(fr.info["num_lf_groups"]):
        t["gg%d" % gg] = (fr.lf_group_info(gg), [fr.plane(gg, w).tobytes() for w in range(4)], [a.tobytes() for a in fr.varblocks(gg)], [fr.llf(gg, c).tobytes() for c in range(3)])
    return t


@pytest.mark.parametrize("container", [0, 1, 2])
@pytest.mark.parametrize("anim", [1, 0], ids=["animation", "layers"])
@pytest.mark.parametrize("mode", ["modular", "vardct"])
def test_sequence_frame_parses_to_the_tables_of_the_frame_alone(built, mode, anim, container):
    import j40_amd
    opts = seq_opts(mode, anim, **({"container": container} if container else {}))
    seq = j40_amd.Sequence(synth(mode, W, H, SEED, **opts))
    for k in range(seq.num_frames):
        mine = seq.frame(k)
        alone = j40_amd.Frame(only_stream(mode, W, H, opts, k))
        x0, y0, w, h = CROPS[k] or (0, 0, W, H)
        assert (mine.width, mine.height) == (alone.width, alone.height) == (w, h)   # crop-sized, like the reference's decode of the frame alone
        assert tables_of(mine) == tables_of(alone), k
        if not mine.info["is_modular"]:   # ... and as the relocatable blob, up to the codestream's bytes and the offsets into it
            assert j40_amd.Frame.from_lf_bundle(mine.lf_bundle()).info == j40_amd.Frame.from_lf_bundle(alone.lf_bundle()).info
        alone.close()
    assert seq.frame(1).h == seq.frame(1).h   # parsed once, owned by the sequence
    seq.close()


# ---------------------------------------------------------------- the default does not move

@pytest.mark.parametrize("mode", ["modular", "vardct"])
def test_without_the_sequence_entry_points_nothing_changes(built, mode):
    import j40_amd
    data = synth(mode, W, H, SEED, **seq_opts(mode, 1))
    with pytest.raises(j40_amd.J40Error) as e:
        j40_amd.Frame(data)
    assert e.value.code == "TODO"
    one = synth(mode, W, H, SEED, **MODES[mode])
    with pytest.raises(j40_amd.J40Error) as e:
        j40_amd.Sequence(one)
    assert e.value.code == "Usq?"
    # a single cropped last frame is a single frame: crop-sized, through the entry point it always went through
    alone = only_stream(mode, W, H, seq_opts(mode, 1), 1)
    with pytest.raises(j40_amd.J40Error) as e:
        j40_amd.Sequence(alone)
    assert e.value.code == "Usq?"
    fr = j40_amd.Frame(alone)
    assert (fr.width, fr.height) == CROPS[1][2:]
    fr.close()


def test_the_reference_refuses_the_sequence_and_decodes_each_frame_alone(built, ref):
    for mode in MODES:
        opts = seq_opts(mode, 1)
        assert ref.decode(synth(mode, W, H, SEED, **opts))[0] == "TODO"
        for k, c in enumerate(CROPS):
            err, px = ref.decode(only_stream(mode, W, H, opts, k))
            assert err == "" and px.shape[:2] == ((c[3], c[2]) if c else (H, W))


# ---------------------------------------------------------------- refusals

@pytest.mark.parametrize("blend", [1, 2, 3, 4])
@pytest.mark.parametrize("mode,extra", [("modular", dict(alpha=0)), ("modular", dict()), ("vardct", dict())], ids=["colour_only", "colour_and_alpha", "vardct"])
def test_other_blend_modes_are_todo_for_their_frame(built, mode, extra, blend):
    """(blends= is the blend mode of every channel of a frame: with an alpha channel it is the alpha channel's too; the test below
    gives the alpha channel a mode of its own)"""
    import j40_amd
    opts = seq_opts(mode, 1, crops=CROPS[:3], durations=DURATIONS[:3], blends="0,%d,0" % blend, **extra)
    seq = j40_amd.Sequence(synth(mode, W, H, SEED, **opts))
    assert seq.num_frames == 2   # the index ends at the frame it cannot serve
    assert seq.frame_info(0)["code"] == "" and seq.frame_info(1)["code"] == "TODO"
    assert seq.num_shown == 1
    with pytest.raises(j40_amd.J40Error) as e:
        seq.frame(1)
    assert e.value.code == "TODO"
    assert seq.frame(0).width == W
    seq.close()


# an alpha channel in both modes. The generator writes a VarDCT frame's alpha with one pass only, and no single-section VarDCT frame: the
# crops are two groups wide
ALPHA_MODES = {"modular": dict(alpha=1), "vardct": dict(alpha=1, passes=1)}
ALPHA_CROPS = [None, (17, 21, 270, 90), (-20, -10, 290, 80)]


@pytest.mark.parametrize("blend", [1, 2, 3, 4])
@pytest.mark.parametrize("mode", ["modular", "vardct"])
def test_a_blend_mode_on_the_alpha_channel_alone_is_todo(built, mode, blend):
    """Replace on the colour channels, another mode on the alpha channel only (ecblends=): refused for that frame all the same"""
    import j40_amd
    opts = seq_opts(mode, 1, crops=ALPHA_CROPS, durations=DURATIONS[:3], ecblends="0,%d,0" % blend, **ALPHA_MODES[mode])
    seq = j40_amd.Sequence(synth(mode, W, H, SEED, **opts))
    assert seq.num_frames == 2 and seq.num_shown == 1
    assert seq.frame_info(0)["code"] == "" and seq.frame_info(1)["code"] == "TODO"
    assert seq.frame_info(1)["blend"] == 0   # the colour channels' mode is Replace: the refusal is the alpha channel's
    with pytest.raises(j40_amd.J40Error) as e:
        seq.frame(1)
    assert e.value.code == "TODO"
    seq.close()
    # the same stream with Replace throughout is served
    seq = j40_amd.Sequence(synth(mode, W, H, SEED, **dict(opts, ecblends="0,0,0")))
    assert seq.num_frames == 3 and [seq.frame_info(k)["code"] for k in range(3)] == ["", "", ""]
    seq.close()


@pytest.mark.parametrize("mode", ["modular", "vardct"])
def test_a_source_slot_of_the_alpha_channel_alone_is_todo(built, mode):
    """the rendered pixels carry colour and alpha together, so a cropped frame whose alpha channel names another source slot than its
    colour channels (ecsrcs=) is refused; the same slot for both is served"""
    import j40_amd
    opts = seq_opts(mode, 1, crops=ALPHA_CROPS, durations=DURATIONS[:3], srcs="0,1,0", ecsrcs="0,2,0", **ALPHA_MODES[mode])
    seq = j40_amd.Sequence(synth(mode, W, H, SEED, **opts))
    assert seq.num_frames == 2 and seq.num_shown == 1
    assert seq.frame_info(0)["code"] == "" and seq.frame_info(1)["code"] == "TODO"
    assert (seq.frame_info(1)["blend"], seq.frame_info(1)["src"]) == (0, 1)
    seq.close()
    seq = j40_amd.Sequence(synth(mode, W, H, SEED, **dict(opts, ecsrcs="0,1,0")))
    assert seq.num_frames == 3 and [seq.frame_info(k)["code"] for k in range(3)] == ["", "", ""]
    assert seq.frame_info(1)["src"] == 1
    seq.close()


@pytest.mark.parametrize("mode", ["modular", "vardct"])
def test_a_frame_of_type_2_is_todo(built, mode):
    import j40_amd
    data = bytearray(synth(mode, W, H, SEED, **seq_opts(mode, 1)))
    seq = j40_amd.Sequence(bytes(data))
    at = seq.frame_info(1)["offset"]
    seq.close()
    assert data[at] & 7 == 0      # all_default = 0, type = 0 (the frame header's first three bits)
    for ftype, want in ((2, "TODO"), (1, "TODO")):
        damaged = bytearray(data)
        damaged[at] |= ftype << 1
        seq = j40_amd.Sequence(bytes(damaged))
        assert seq.num_frames == 2 and seq.frame_info(1)["code"] == want and seq.frame_info(0)["code"] == ""
        seq.close()


# ---------------------------------------------------------------- damage

@pytest.mark.parametrize("mode", ["modular", "vardct"])
def test_truncation_is_shrt_from_the_frame_it_hits(built, mode):
    import j40_amd
    data = synth(mode, W, H, SEED, **seq_opts(mode, 1))
    seq = j40_amd.Sequence(data)
    rows = [seq.frame_info(k) for k in range(seq.num_frames)]
    seq.close()
    for k, r in enumerate(rows):
        for cut in (r["offset"] + 1, r["first_section"] - 1):   # inside the frame header; inside the TOC
            if k == 0:
                with pytest.raises(j40_amd.J40Error) as e:
                    j40_amd.Sequence(data[:cut])
                assert e.value.code == "shrt"
                continue
            seq = j40_amd.Sequence(data[:cut])
            assert seq.num_frames == k + 1, (k, cut)
            assert [seq.frame_info(j)["code"] for j in range(k + 1)] == [""] * k + ["shrt"]
            assert [seq.frame_info(j) for j in range(k)] == rows[:k]
            seq.close()
    seq = j40_amd.Sequence(data[:-1])   # in the last frame's last section
    assert seq.num_frames == len(rows) and seq.frame_info(len(rows) - 1)["code"] == "shrt"
    assert [seq.frame_info(j) for j in range(len(rows) - 1)] == rows[:-1]
    seq.close()


@pytest.mark.parametrize("mode", ["modular", "vardct"])
def test_bit_flips_in_frame_1_leave_frame_0_alone(built, mode):
    import j40_amd
    data = synth(mode, W, H, SEED, **seq_opts(mode, 1))
    seq = j40_amd.Sequence(data)
    row0, lo, hi = seq.frame_info(0), seq.frame_info(1)["offset"], seq.frame_info(1)["end"]
    table0 = tables_of(seq.frame(0))
    seq.close()
    rng = np.random.default_rng(20)
    for _ in range(20):
        bit = int(rng.integers(lo * 8, hi * 8))
        damaged = bytearray(data)
        damaged[bit >> 3] ^= 1 << (bit & 7)
        seq = j40_amd.Sequence(bytes(damaged))
        assert seq.frame_info(0) == row0, bit
        assert tables_of(seq.frame(0)) == table0, bit
        seq.close()


# ---------------------------------------------------------------- the composition's device functions on the CPU

GUARD = 64


class Guarded:
    """`rows` rows of `stride` bytes whose first byte sits at `align` modulo 16, between guard bytes"""

    def __init__(self, rows, stride, align, fill_rng=None):
        self.n = rows * stride
        self.raw = np.full(self.n + 2 * GUARD + 32, 0xA5, np.uint8)
        self.base = self.place()    # where the bytes of `raw` live for whoever composes: here, or a copy in device memory
        self.off = GUARD + ((align - (self.base + GUARD)) % 16)
        self.view = self.raw[self.off:self.off + self.n]
        if fill_rng is not None:
            self.view[:] = fill_rng.integers(0, 256, self.n, dtype=np.uint8)
        self.rows, self.stride = rows, stride
        self.before = self.raw.copy()
        self.send()

    def place(self):
        return self.raw.ctypes.data

    def send(self):
        pass

    def fetch(self):
        pass

    @property
    def ptr(self):
        return self.base + self.off

    def pixels(self, w, pb):
        return self.view.reshape(self.rows, self.stride)[:, :w * pb].reshape(self.rows, w, pb)

    def untouched_outside(self, w, pb):
        """guards, and the bytes of every row behind its w pixels, are what they were"""
        now, was = self.raw.copy(), self.before.copy()
        for a in (now, was):
            a[self.off:self.off + self.n].reshape(self.rows, self.stride)[:, :w * pb] = 0
        return np.array_equal(now, was)


def compose_cases():
    """(pb, cw, ch, x0, y0, w, h, source, a0, alike): the table both the CPU build and the kernel go through. source: "slot", "none" or
    "same" (the output is the source); a0: the empty pixel's alpha is 0; alike: the three images' rows sit alike modulo 16 bytes"""
    cases = []
    n = 0
    for pb in (4, 8):
        for cw, ch in ((67, 9), (64, 5)):
            for x0 in range(16 // pb):                 # x0 % 4 in 0..3 (u8), x0 % 2 in 0..1 (u16)
                for w in (1, 3, 4, 5, 64):
                    for source in ("slot", "none", "same"):
                        cases.append((pb, cw, ch, 4 + x0, 2, w, 3, source, n % 2 == 0, n % 3 != 0))
                        n += 1
            # off each of the four edges, over a corner, covering everything, entirely outside
            for rect in ((-5, 2, 9, 3), (cw - 4, 1, 9, 3), (3, -2, 7, 4), (3, ch - 2, 7, 5), (-3, -1, 6, 4), (-2, -2, cw + 4, ch + 4), (cw, 0, 5, 5), (-9, 0, 9, 3), (0, ch + 1, 4, 2)):
                for source in ("slot", "none", "same"):
                    cases.append((pb, cw, ch) + rect + (source, n % 2 == 1, n % 3 != 1))
                    n += 1
    return cases


def empty_words(pb, a0):
    return (0 if a0 else 0xFF000000, 0) if pb == 4 else (0, 0 if a0 else 0xFFFF0000)


def compose_expected(canvas_src, frame, cw, ch, x0, y0, pb, a0):
    """the issue's definition, in numpy: inside the rectangle clipped to the canvas the frame's pixel, elsewhere the source's or the empty one"""
    if canvas_src is None:
        lo, hi = empty_words(pb, a0)
        px = np.frombuffer(np.array([lo, hi], "<u4").tobytes()[:pb], np.uint8)
        out = np.tile(px, (ch, cw, 1))
    else:
        out = canvas_src.copy()
    h, w = frame.shape[:2]
    cx0, cy0, cx1, cy1 = max(x0, 0), max(y0, 0), min(x0 + w, cw), min(y0 + h, ch)
    if cx1 > cx0 and cy1 > cy0:
        out[cy0:cy1, cx0:cx1] = frame[cy0 - y0:cy1 - y0, cx0 - x0:cx1 - x0]
    return out


def run_compose_case(case, call, seed, Guarded=Guarded):
    """builds the three images of a case between guards, lets `call` compose them, checks pixels and guards"""
    pb, cw, ch, x0, y0, w, h, source, a0, alike = case
    rng = np.random.default_rng(seed)
    skew = 0 if alike else pb
    out_stride = ((cw * pb + 15) & ~15) + 16
    out = Guarded(ch, out_stride, 0, rng)
    # the frame's pixel that lands on the rectangle's first canvas column sits like that canvas pixel does (or one pixel off)
    fx, cx0 = max(0, -x0), max(0, x0)
    frm = Guarded(h, ((w * pb + 15) & ~15) + 32 + skew, (cx0 - fx) * pb + skew, rng)
    src = out if source == "same" else Guarded(ch, out_stride + 16 + skew, skew, rng) if source == "slot" else None
    frame_px = frm.pixels(w, pb).copy()
    src_px = None if src is None else src.pixels(cw, pb).copy()
    want = compose_expected(src_px, frame_px, cw, ch, x0, y0, pb, a0)
    lo, hi = empty_words(pb, a0)
    call(out.ptr, out.stride, src.ptr if src else None, src.stride if src else 0, frm.ptr, frm.stride, cw, ch, x0, y0, w, h, lo, hi, pb)
    for g in (out, frm, src):
        if g is not None:
            g.fetch()
    assert np.array_equal(out.pixels(cw, pb), want), case
    assert out.untouched_outside(cw, pb), case
    assert np.array_equal(frm.raw, frm.before), case
    assert src is None or src is out or np.array_equal(src.raw, src.before), case


_sim = None


def compose_sim():
    global _sim
    if _sim is None:
        _sim = C.CDLL(os.path.join(ROOT, "build", "libhostsim_compose.so"))
        vp, sz, i32, u32 = C.c_void_p, C.c_size_t, C.c_int32, C.c_uint32
        _sim.compose_sim.argtypes = [vp, sz, vp, sz, vp, sz, i32, i32, i32, i32, i32, i32, u32, u32, i32, i32]
        _sim.compose_sim.restype = None
        _sim.compose_sim_clip.argtypes = [i32] * 6 + [vp]
        _sim.compose_sim_clip.restype = None
    return _sim


@pytest.mark.parametrize("lanes", [1, 3, 64])
def test_compose_rows_on_the_cpu(built, lanes):
    sim = compose_sim()
    cases = compose_cases()
    assert {c[7] for c in cases} == {"slot", "none", "same"} and {c[8] for c in cases} == {True, False} and {c[9] for c in cases} == {True, False}
    for n, case in enumerate(cases):
        run_compose_case(case, lambda *a: sim.compose_sim(*a, lanes), n)


def test_compose_clip(built):
    sim = compose_sim()
    out = np.zeros(6, np.int32)
    for (cw, ch, x0, y0, w, h), want in [
            ((300, 200, 37, 21, 130, 90), (37, 21, 167, 111, 0, 0)), ((300, 200, -20, -10, 100, 80), (0, 0, 80, 70, 20, 10)),
            ((300, 200, 250, 150, 100, 100), (250, 150, 300, 200, 0, 0)), ((300, 200, 300, 0, 10, 10), (0, 0, 0, 0, 0, 0)),
            ((300, 200, -10, -10, 10, 10), (0, 0, 0, 0, 0, 0)), ((300, 200, -5, -5, 400, 400), (0, 0, 300, 200, 5, 5)),
            ((262144, 8, 262000, 0, 262144, 8), (262000, 0, 262144, 8, 0, 0)), ((8, 8, -2147483647, 0, 5, 5), (0, 0, 0, 0, 0, 0))]:
        sim.compose_sim_clip(cw, ch, x0, y0, w, h, out.ctypes.data)
        assert tuple(out.tolist()) == want, (cw, ch, x0, y0, w, h)
