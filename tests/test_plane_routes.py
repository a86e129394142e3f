"""The plane stage ("the plane stage"): every route on which a frame's samples are three float planes (X, Y, B) between the
inverse transforms and the caller's image -- the restoration filters, the colour mode, patches, a 4:4:4 YCbCr frame, the planes a
sequence keeps in its LF and reference slots -- crossed with each other, which no other test does.

Everything compares with a fixture recorded from the commit BEFORE the stage was written once, by this very file:
    python tests/test_plane_routes.py record tests/golden/plane_routes.json.gz COMMIT        (on the MI355X)
with J40HIP_LIB pointing at that commit's build/libj40hip.so. Never record it from the code under test. tests/test_decode_modes.py
is the pattern, and its digest, fixture reader and writer are used here.

Every cell makes its decodes twice on the same handle and the two results must be equal: state a decode fails to reset shows there.
The frames are 261 x 70 (two groups across, a width that is no multiple of 4, a height that is no multiple of 8) unless the stream
helper fixes a size of its own. j40hip_frame_restoration reports the header alone; whether the filters ran is what j40hip_frame_read_xyb
answers for stage 2 (the reciprocal sigmas), recorded with stages 0, 1 and 3 -- as a digest where the frame signals the edge-preserving
filter, else only as "answered": without that filter nothing writes the sigmas."""
import hashlib
import itertools
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))

from test_decode_modes import digest, load_fixture, write_fixture, no_switches, U8X4, U16X4
from colour_streams import stream as colour_stream
from lf_streams import lf_stream, lf_size, WIDE
from ycbcr_ref import ycbcr_stream
import patch_streams as P

FIXTURE = os.path.join(ROOT, "tests", "golden", "plane_routes.json.gz")
W, H = 261, 70
SHAPES = [("whole", None), ("region", (20, 30, 100, 33)), ("scale_1", 1)]
FILTERS = dict(fullheader=1, gab=1, epf=2)
LF_PICTURE = dict(lfkind="picture", forward=1, lfgab=1, lfepf=1)   # (the LF frame signals filters of its own: the slot holds filtered planes)
LF_MODULAR = dict(lfmodular=1, global_scale=4096, quant_lf=16, nocfl=1)
PATCH_KINDS = {   # (tests/test_patches_gpu.py's two, with a signalled encoding so that the colour mode is in force where the sequence asks for it)
    "vardct": dict(main="v", mode="vardct", w=P.VW, h=P.VH, sizes=[P.REF_V, P.REF_M], modes=["v", "m"], more=dict(gab=1)),
    "modular": dict(main="m", mode="modular", w=P.MW, h=P.MH, sizes=[P.REF_M, (60, 34)], modes=["m", "m"], more={}),
}


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def answer(j40, read):
    """a read-back hook's planes as their SHA-256, or the code it refuses with"""
    try:
        return sha(read())
    except j40.J40Error as e:
        return "refused:" + e.code


def last_decode(fr):
    c = fr.colour()
    return [c["used"], c["curve_evaluated_at_8_bits"], fr.ycbcr()["used"], fr.alpha()["written"], fr.modular_xyb()["used"]]


def frame_pass(j40, torch, fr, ycbcr):
    """[decode()'s code, status()'s, digest, getters, read_xyb 0 / 1 / 2 / 3 (, read_ycbcr 0..2)], and the same of decode_to_host()"""
    pb = 8 if fr.output_format() == U16X4 else 4
    o = fr.orientation()
    w, h = o["width"], o["height"]

    def behind():
        planes = [answer(j40, lambda s=s: fr.read_xyb(s)) for s in (0, 1, 2, 3)]
        if not planes[2].startswith("refused") and fr.restoration().epf_iters == 0:
            planes[2] = "answered"   # (no edge-preserving filter: nothing ever writes the sigmas, the bytes are whatever the allocation held)
        if ycbcr:
            planes += [answer(j40, lambda c=c: fr.read_ycbcr(c)) for c in range(3)]
        return [last_decode(fr), planes]

    dev = torch.zeros((h, w * pb), dtype=torch.uint8, device="cuda:0")
    call = j40.err4(j40.lib().j40hip_frame_decode(fr.h, dev.data_ptr(), w * pb, 0))
    torch.cuda.synchronize()
    on_device = [call, "" if call else fr.status(), None if call else digest(dev.cpu().numpy(), False, pb)] + behind()
    code, px = fr.decode_to_host()
    to_host = [code, None if code else digest(px.view(np.uint8).reshape(h, w * pb), False, pb)] + behind()
    return [on_device, to_host]


def frame_cell(j40, torch, fr, c, ycbcr=False):
    """[setter codes, the two entries' results]; both entries are made twice"""
    fr.set_region(0, 0, 0, 0); fr.set_scale(0)
    codes = []
    fr.set_restoration(c["restoration"])
    if c.get("colour") is not None:
        codes.append(fr.set_colour(c["colour"]))
    how = dict(SHAPES)[c["shape"]]
    if isinstance(how, tuple):
        codes.append(fr.set_region(*how))
    elif how:
        codes.append(fr.set_scale(how))
    first, second = frame_pass(j40, torch, fr, ycbcr), frame_pass(j40, torch, fr, ycbcr)
    assert first == second, "the second decode on the same handle answers as the first"
    return [codes, first]


def frame_cells(restorations, colours, shapes):
    return [dict(restoration=r, colour=k, shape=s) for r, k, s in itertools.product(restorations, colours, shapes)]


def frame_cell_id(c):
    return "restoration_%d%s/%s" % (c["restoration"], "" if c["colour"] is None else "/colour_%d" % c["colour"], c["shape"])


def run_frames(j40, torch, data, fmt, cells, ycbcr=False, modular_xyb=False):
    fr = j40.Frame(data, ycbcr=True) if ycbcr else j40.Frame(data)
    if ycbcr:
        assert fr.set_ycbcr(1) == ""
    if modular_xyb:
        assert fr.set_modular_xyb(1) == ""
    fr.set_output_format(fmt)
    fr.upload(0)
    out = {frame_cell_id(c): frame_cell(j40, torch, fr, c, ycbcr) for c in cells}
    fr.close()
    return out


def sequence_pass(j40, seq, main, lf_slot, ref_slots):
    """[next_to_host()'s code, the sequence's status, canvas digest, the main frame's getters, its read_xyb 3, the slots' digests]"""
    code, px = seq.next_to_host()
    status = list(seq.status())
    fr = seq.frame(main)
    slots = [answer(j40, lambda: seq.read_lf_slot(1, *lf_slot))] if lf_slot else [answer(j40, lambda k=k: seq.read_ref_slot(k)) for k in ref_slots]
    return [code, status, None if code else sha(px), last_decode(fr), answer(j40, lambda: fr.read_xyb(3)), slots]


def sequence_cell(j40, data, c, main, lf_slot=None, ref_slots=(), **switches):
    """the playback twice (rewound in between) on the same handles"""
    seq = j40.Sequence(data, colour=bool(c.get("colour")), **switches)
    for k in range(seq.num_frames):
        seq.frame(k).set_restoration(c["restoration"])
    seq.upload(0)
    first = sequence_pass(j40, seq, main, lf_slot, ref_slots)
    seq.rewind()
    second = sequence_pass(j40, seq, main, lf_slot, ref_slots)
    seq.close()
    assert first == second, "the second playback on the same handles answers as the first"
    return [[], first]


def patch_data(kind):
    K = PATCH_KINDS[kind]
    refs = P.main_refs(K["w"], K["h"], K["sizes"][0], K["sizes"][1])
    return P.patch_synth(K["mode"], K["w"], K["h"], **P.seq_opts(K["main"], refs, K["sizes"], K["modes"], primaries=11, tf=16, **K["more"]))


# part -> (its cells, how they run): one stream in one format each
def _vardct(opts, restorations, shapes):
    cells = frame_cells(restorations, (0, 1), shapes)
    return cells, lambda j40, torch, fmt: run_frames(j40, torch, colour_stream("vardct", W, H, "pq", **opts), fmt, cells)


def _ycbcr():
    cells = frame_cells((0, 1), (None,), ("whole",))
    return cells, lambda j40, torch, fmt: run_frames(j40, torch, ycbcr_stream(W, H, gab=1), fmt, cells, ycbcr=True)


def _modular():
    cells = frame_cells((0,), (0, 1), [s for s, _ in SHAPES])
    return cells, lambda j40, torch, fmt: run_frames(j40, torch, colour_stream("modular", W, H, "pq", alpha=1), fmt, cells, modular_xyb=True)


def _patches(kind):
    cells = frame_cells((0, 1) if kind == "vardct" else (0,), (0, 1), ("whole",))
    return cells, lambda j40, torch, fmt: {frame_cell_id(c): sequence_cell(j40, patch_data(kind), c, 2, ref_slots=(1, 2), patches=True, modular_xyb=True) for c in cells}


def _lf_still(opts, **switches):
    cells = frame_cells((0, 1), (None,), ("whole",))
    return cells, lambda j40, torch, fmt: {frame_cell_id(c): sequence_cell(j40, lf_stream(WIDE, **opts), c, 1, lf_slot=lf_size(WIDE), lf_frames=True, **switches) for c in cells}


STREAMS = {
    "vardct_filters": (_vardct(FILTERS, (0, 1, 2), [s for s, _ in SHAPES]), (U8X4, U16X4)),
    "vardct_epf0": (_vardct(dict(FILTERS, epflut=0), (0, 1), ("whole",)), (U8X4,)),      # the filters refuse with "epf0"
    "ycbcr_444": (_ycbcr(), (U8X4, U16X4)),
    "modular_xyb_alpha": (_modular(), (U8X4, U16X4)),
    "patches_vardct": (_patches("vardct"), (U8X4,)),
    "patches_modular": (_patches("modular"), (U8X4,)),
    "lf_still_vardct": (_lf_still(LF_PICTURE), (U8X4,)),
    "lf_still_modular": (_lf_still(LF_MODULAR, modular_xyb=True), (U8X4,)),
}
PARTS = [(name, fmt) for name, (_, fmts) in STREAMS.items() for fmt in fmts]


def part_id(part):
    return "%s-%s" % (part[0], "u16" if part[1] == U16X4 else "u8")


def cell_ids(part):
    return ["%s/%s" % (part_id(part), frame_cell_id(c)) for c in STREAMS[part[0]][0][0]]


def table(j40, parts=PARTS):
    import torch
    no_switches()
    assert os.environ.get("J40HIP_COLOUR", "") in ("", "0") and os.environ.get("J40HIP_PATCHES", "") in ("", "0") and os.environ.get("J40HIP_LFFRAME", "") in ("", "0")
    cells = {}
    for part in parts:
        for key, cell in STREAMS[part[0]][0][1](j40, torch, part[1]).items():
            cells["%s/%s" % (part_id(part), key)] = cell
    return cells


def refused(cells, part=None):
    """cells whose decode (or playback) answered with a code, from the call or from the status behind it"""
    mine = [v for k, v in cells.items() if part is None or k.split("/")[0] == part_id(part)]
    return sum(bool(v[1][0][0] or v[1][0][1]) if isinstance(v[1][0], list) else bool(v[1][0] or v[1][1][0]) for v in mine)


@pytest.fixture(scope="module")
def gpu(built):
    import j40_amd
    assert j40_amd.device_count() > 0, "the gpu tests need a HIP device"
    return j40_amd


@pytest.fixture(scope="module")
def fixture():
    return load_fixture(FIXTURE)


@pytest.mark.gpu
@pytest.mark.parametrize("part", PARTS, ids=part_id)
def test_plane_routes_decode_as_before_the_plane_stage(gpu, fixture, part):
    """the setters' codes, both entries' codes, status, the pixels' SHA-256, the getters' last-decode fields and what the read-back hooks
    answer are the fixture's, twice in a row on one handle. A refusal is an expected value like any other; no cell is missing or extra."""
    want = {k: v for k, v in fixture["cells"].items() if k.split("/")[0] == part_id(part)}
    got = table(gpu, [part])
    assert sorted(got) == sorted(want)
    for key, cell in got.items():
        print(key, cell)
        assert cell == want[key], key
    assert refused(got) <= fixture["header"]["refused_per_part"][part_id(part)], "a run that refuses more is seen"


def test_plane_routes_fixture_is_whole():
    """the fixture's own header: every cell of the matrix is there, the refused ones are counted"""
    fx = load_fixture(FIXTURE)
    ids = [i for p in PARTS for i in cell_ids(p)]
    assert sorted(ids) == sorted(fx["cells"]) and len(ids) == fx["header"]["cells"]
    assert {part_id(p): refused(fx["cells"], p) for p in PARTS} == fx["header"]["refused_per_part"]
    assert refused(fx["cells"]) == fx["header"]["refused"]


# ---------------------------------------------------------------- recording (the commit before, through J40HIP_LIB)

if __name__ == "__main__":
    import j40_amd
    if len(sys.argv) != 4 or sys.argv[1] != "record":
        raise SystemExit("record OUT COMMIT")
    cells = table(j40_amd)
    header = dict(cells=len(cells), refused=refused(cells), refused_per_part={part_id(p): refused(cells, p) for p in PARTS}, recorded_at_commit=sys.argv[3])
    j40_amd.shutdown()
    write_fixture(sys.argv[2], dict(header=header, cells=cells))
    print(header)
