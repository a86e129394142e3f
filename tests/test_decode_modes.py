"""A handle's decode modes, stated once (j40_amd/csrc/decode_route.hpp): which setter refuses what in which order of calls, what
the getters report, and which route every combination of modes takes through the decode entry points.

Both halves compare with fixtures recorded from the commit BEFORE the route existed, by this very file:
    python tests/test_decode_modes.py record-setters tests/golden/decode_modes_setters.json.gz COMMIT      (no device needed)
    python tests/test_decode_modes.py record-routes tests/golden/decode_modes_routes.json.gz COMMIT        (on the MI355X)
with J40HIP_LIB pointing at that commit's build/libj40hip.so. Never record them from the code under test. The fixtures are JSON,
gzipped (300 KB each as text, mostly repetition; `zcat` shows them).

The route cases cross everything the modes can combine into and every cell decodes twice: a minute on the MI355X, in 30 cases
(a stream in one format and one range value) of 5 s at the most."""
import ctypes as C
import gzip
import hashlib
import itertools
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))

from streams import synth
from lf_streams import lf_stream, WIDE

GOLDEN = os.path.join(ROOT, "tests", "golden")
SETTERS_FIXTURE = os.path.join(GOLDEN, "decode_modes_setters.json.gz")
ROUTES_FIXTURE = os.path.join(GOLDEN, "decode_modes_routes.json.gz")
W, H, SEED = 300, 270, 5    # 2 x 2 groups of 256: a region can cover some of them, and be its cover or not
U8X4, U16X4 = 0x0F33, 0x0F35
SWITCHES = ("J40HIP_ORIENT", "J40HIP_ALPHA", "J40HIP_RESTORATION", "J40HIP_MODULAR_XYB", "J40HIP_YCBCR")


def load_fixture(path):
    with gzip.open(path, "rt") as fp:
        return json.load(fp)


def write_fixture(path, table):
    with open(path, "wb") as raw, gzip.GzipFile(filename="", mode="wb", fileobj=raw, mtime=0, compresslevel=9) as fp:   # (no name, no time: the same bytes for the same table)
        fp.write((json.dumps(table, separators=(",", ":"), sort_keys=True) + "\n").encode())


def no_switches():
    for name in SWITCHES:
        assert os.environ.get(name, "") in ("", "0"), "this file sets every mode itself: unset %s" % name


# ---------------------------------------------------------------- 1. the setters and getters (no device)

def setter_handles(j40):
    """name -> handle; the second value keeps the handles' owners alive"""
    keep = []
    plain = synth("vardct", W, H, SEED)
    probe = j40.Frame(plain)
    lf_end = probe.lf_end()
    bundle = probe.lf_bundle()
    probe.close()
    crops = j40.Sequence(synth("vardct", 300, 200, SEED, passes=2, frames=2, crops=";37,21,130,90", orientation=6))
    still = j40.Sequence(lf_stream(WIDE, orientation=6), lf_frames=True)
    keep += [crops, still]
    return {
        "vardct": j40.Frame(plain),
        "vardct_alpha": j40.Frame(synth("vardct", W, H, SEED, alpha=1)),
        "modular": j40.Frame(synth("modular", W, H, SEED)),
        "modular_xyb": j40.Frame(synth("modular", W, H, SEED, xyb=1)),
        "lf_only": j40.Frame(plain[:lf_end], lf_only=True),
        "orientation_6": j40.Frame(synth("vardct", W, H, SEED, orientation=6)),
        "sequence_frame": crops.frame(1),            # a cropped frame of an animation
        "sequence_lf_frame": still.frame(0),         # the LF frame of a still (type 1)
        "sequence_lf_still": still.frame(1),         # ... and its main frame: the one handle of a sequence that takes a scale and the orientation
        "from_view": j40.Frame.from_lf_bundle(bundle),
    }, keep


def setter_ops(fr):
    w, h = fr.width, fr.height
    return [
        ("region_inside", lambda: fr.set_region(w // 8, h // 8, w // 2, h // 2)),
        ("region_outside", lambda: fr.set_region(w // 2, h // 2, w, h)),
        ("region_clear", lambda: fr.set_region(0, 0, 0, 0)),
        ("scale_0", lambda: fr.set_scale(0)), ("scale_1", lambda: fr.set_scale(1)), ("scale_2", lambda: fr.set_scale(2)), ("scale_3", lambda: fr.set_scale(3)),
        ("orientation_default", lambda: fr.set_orientation(-1)), ("orientation_0", lambda: fr.set_orientation(0)), ("orientation_1", lambda: fr.set_orientation(1)),
        ("alpha_1", lambda: fr.set_alpha(1)),
        ("modular_xyb_1", lambda: fr.set_modular_xyb(1)),
    ]


def handle_state(fr):
    return [list(fr.region().values()), list(fr.scale().values()), list(fr.orientation().values()), fr.alpha()["mode"], fr.modular_xyb()["on"]]


def reset_modes(fr):
    fr.set_region(0, 0, 0, 0); fr.set_scale(0); fr.set_orientation(-1); fr.set_alpha(-1); fr.set_modular_xyb(-1)


def setter_table(j40):
    """{"ops": names, "handles": {name: {"outcomes": the distinct [codes, state] seen, "pairs": / "triples": an index into them for every
    ordered pair / triple of ops (repeats included) in itertools.product's order}}}"""
    no_switches()
    handles, keep = setter_handles(j40)
    table = {"ops": None, "handles": {}}
    for name, fr in handles.items():
        ops = setter_ops(fr)
        table["ops"] = [n for n, _ in ops]
        fresh = handle_state(fr)
        outcomes, index = [], {}
        row = {"fresh": fresh}
        for key, n in (("pairs", 2), ("triples", 3)):
            row[key] = []
            for seq in itertools.product(range(len(ops)), repeat=n):
                codes = [ops[k][1]() for k in seq]
                text = json.dumps([codes, handle_state(fr)], separators=(",", ":"))
                if text not in index:
                    index[text] = len(outcomes)
                    outcomes.append(json.loads(text))
                row[key].append(index[text])
                reset_modes(fr)
                assert handle_state(fr) == fresh, "clearing every mode leaves the handle as it was parsed (%s after %s)" % (name, [ops[k][0] for k in seq])
        row["outcomes"] = outcomes
        table["handles"][name] = row
    for fr in handles.values():
        fr.close()
    for s in keep:
        s.close()
    return table


def test_setters_and_getters_answer_as_before_the_route(built):
    """every ordered pair and triple of the mode setters on every kind of handle: each returned code and the getters' full output
    afterwards equal what the commit before the route answered. A missing or an extra case fails."""
    import j40_amd
    want = load_fixture(SETTERS_FIXTURE)
    got = setter_table(j40_amd)
    assert got["ops"] == want["ops"]
    assert sorted(got["handles"]) == sorted(want["handles"])
    n = len(got["ops"])
    cases = 0
    for name, row in got["handles"].items():
        ref = want["handles"][name]
        assert row["fresh"] == ref["fresh"], name
        for key, k in (("pairs", 2), ("triples", 3)):
            assert len(row[key]) == len(ref[key]) == n ** k, (name, key)
            for seq, a, b in zip(itertools.product(got["ops"], repeat=k), row[key], ref[key]):
                assert row["outcomes"][a] == ref["outcomes"][b], (name, seq)
            cases += len(row[key])
    assert cases == want["cases"]


# ---------------------------------------------------------------- 2. the routes (MI355X)

ROUTE_STREAMS = [   # name, generator mode, options (every stream carries orientation 6), the dimensions that apply beyond shape / order / format / range
    ("vardct", "vardct", dict(), ("restoration",)),
    ("vardct_alpha", "vardct", dict(alpha=1), ("restoration", "alpha")),
    ("vardct_filters", "vardct", dict(fullheader=1, gab=1, epf=2), ("restoration",)),
    ("modular", "modular", dict(), ()),
    ("modular_xyb", "modular", dict(xyb=1), ("modular_xyb",)),
]
SHAPES = [
    ("whole", None),
    ("region_is_its_cover", (0, 0, 256, 256)),        # group 0 exactly
    ("region_in_one_group", (20, 30, 100, 80)),
    ("region_in_four_groups", (200, 200, 100, 70)),
    ("scale_1", 1), ("scale_2", 2),
]
# groups 1..2 of the four: uploaded whole, then narrowed -- ahead of the other setters (they see the range) or behind them (it sees them)
RANGES = ["every_group", "range_then_modes", "modes_then_range"]
RANGE = (1, 2)


def route_cells(dims):
    for shape, order, fmt, rng in itertools.product(range(len(SHAPES)), (0, 1), (U8X4, U16X4), RANGES):
        for r, a, x in itertools.product((0, 1) if "restoration" in dims else (None,), (0, 1) if "alpha" in dims else (None,), (0, 1) if "modular_xyb" in dims else (None,)):
            yield dict(shape=shape, order=order, fmt=fmt, range=rng, restoration=r, alpha=a, modular_xyb=x)


def cell_id(stream, c):
    return "%s/%s/%s/%s/%s%s%s%s" % (stream, SHAPES[c["shape"]][0], "oriented" if c["order"] else "stored", "u16" if c["fmt"] == U16X4 else "u8", c["range"],
                                   "" if c["restoration"] is None else "/restoration_%d" % c["restoration"], "" if c["alpha"] is None else "/alpha_%d" % c["alpha"],
                                   "" if c["modular_xyb"] is None else "/modular_xyb_%d" % c["modular_xyb"])


def last_decode(fr):
    return [list(fr.region().values()), list(fr.scale().values()), list(fr.orientation().values()), fr.alpha()["written"], fr.modular_xyb()["used"], fr.ycbcr()["used"], fr.wide()["used"]]


def range_rects(first, count, w, h, gcolumns=2, gdim=256):
    return [((g % gcolumns) * gdim, (g // gcolumns) * gdim, min(w, (g % gcolumns + 1) * gdim), min(h, (g // gcolumns + 1) * gdim)) for g in range(first, first + count)]


def digest(rows, partial, pb):
    """SHA-256 of an image's bytes ([h, w * pb] uint8). A partial group range writes its groups' rectangles and nothing else -- the
    other pixels are the caller's on the device and whatever the block held in decode_to_host --, so only those are hashed"""
    m = hashlib.sha256()
    if not partial:
        m.update(np.ascontiguousarray(rows).tobytes())
    else:
        for x0, y0, x1, y1 in range_rects(RANGE[0], RANGE[1], rows.shape[1] // pb, rows.shape[0]):
            m.update(np.ascontiguousarray(rows[y0:y1, x0 * pb:x1 * pb]).tobytes())
    return m.hexdigest()


def run_cell(j40, torch, fr, c):
    """[setter codes, [decode()'s code, status()'s, digest, last-decode fields], [decode_to_host()'s code, digest, last-decode fields]].
    A code that only status() reports (the restoration filters' "epf0" on a frame whose header leaves them at their defaults) comes with
    pixels on the device, and with none from decode_to_host, which copies nothing back then"""
    L = j40.lib()
    ng = fr.info["num_groups"]
    fr.set_region(0, 0, 0, 0); fr.set_scale(0); fr.set_orientation(0); fr.set_restoration(0); fr.set_alpha(0); fr.set_modular_xyb(0)
    assert L.j40hip_frame_set_group_range(fr.h, 0, ng) == 0
    fr.set_output_format(c["fmt"])
    codes = []
    narrow = lambda: codes.append(j40.err4(L.j40hip_frame_set_group_range(fr.h, RANGE[0], RANGE[1])))
    if c["range"] == "range_then_modes":
        narrow()
    if c["restoration"] is not None:
        fr.set_restoration(c["restoration"])
    if c["alpha"] is not None:
        codes.append(fr.set_alpha(c["alpha"]))
    if c["modular_xyb"] is not None:
        codes.append(fr.set_modular_xyb(c["modular_xyb"]))
    how = SHAPES[c["shape"]][1]
    if isinstance(how, tuple):
        codes.append(fr.set_region(*how))
    elif how:
        codes.append(fr.set_scale(how))
    codes.append(fr.set_orientation(c["order"]))
    if c["range"] == "modes_then_range":
        narrow()
    partial = c["range"] != "every_group" and codes[0 if c["range"] == "range_then_modes" else -1] == ""
    pb = 8 if c["fmt"] == U16X4 else 4
    o = fr.orientation()
    w, h = o["width"], o["height"]
    dev = torch.zeros((h, w * pb), dtype=torch.uint8, device="cuda:0")
    call = j40.err4(L.j40hip_frame_decode(fr.h, dev.data_ptr(), w * pb, 0))
    torch.cuda.synchronize()
    on_device = [call, "" if call else fr.status(), None if call else digest(dev.cpu().numpy(), partial, pb), last_decode(fr)]
    code, px = fr.decode_to_host()
    to_host = [code, None if code else digest(px.view(np.uint8).reshape(h, w * pb), partial, pb), last_decode(fr)]   # (px: zeros where nothing came back)
    return [codes, on_device, to_host]


# One handle serves the cells of a stream in one format and one range value, in route_cells' order (what a getter says of "the last decode
# with a region" outlives the region, so a cell's fields know the cells before it): a part is a test case of a few seconds -- a Modular
# decode of these groups, and of an alpha sub-image, is some 80 ms, and every cell makes two
ROUTE_PARTS = [(s[0], fmt, rng) for s in ROUTE_STREAMS for fmt in (U8X4, U16X4) for rng in RANGES]


def part_id(part):
    return "%s-%s-%s" % (part[0], "u16" if part[1] == U16X4 else "u8", part[2])


def route_table(j40, parts=ROUTE_PARTS):
    import torch
    no_switches()
    cells = {}
    for stream, fmt, rng in parts:
        name, mode, opts, dims = [s for s in ROUTE_STREAMS if s[0] == stream][0]
        fr = j40.Frame(synth(mode, W, H, SEED, orientation=6, **opts))
        fr.upload(0)
        for c in route_cells(dims):
            if (c["fmt"], c["range"]) == (fmt, rng):
                cells[cell_id(name, c)] = run_cell(j40, torch, fr, c)
        fr.close()
    return cells


def agree(cell):
    """decode() + status() and decode_to_host(): one code, and the same pixels wherever both have some"""
    return (cell[1][0] or cell[1][1]) == cell[2][0] and (cell[2][1] is None or cell[2][1] == cell[1][2])


def in_part(key, part):
    k = key.split("/")
    return part is None or (k[0], k[3], k[4]) == (part[0], "u16" if part[1] == U16X4 else "u8", part[2])


def refusals(cells, part=None):
    """[cells in which a setter refused, cells whose decode() refused, cells whose decode ran and status() reports a code]"""
    mine = [v for k, v in cells.items() if in_part(k, part)]
    return [sum(any(v[0]) for v in mine), sum(bool(v[1][0]) for v in mine), sum(bool(v[1][1]) for v in mine)]


def batch_table(j40):
    """the batch entry with two VarDCT handles (plain, and the one with an alpha channel) at scale 0 and 1 in both formats with alpha
    dropped and kept, then the refusals of a membership it does not serve: {case: [create code, decode code, statuses, digests, alpha written]}"""
    import torch
    no_switches()
    a = j40.Frame(synth("vardct", W, H, SEED, orientation=6))
    b = j40.Frame(synth("vardct", W, H, SEED, orientation=6, alpha=1))
    a.upload(0); b.upload(0)

    def run():
        try:
            batch = j40.Batch([a, b])
        except j40.J40Error as e:
            return [e.code, None, None, None, None]
        pb = 8 if a.output_format() == U16X4 else 4
        sizes = [(f.scale()["width"], f.scale()["height"]) for f in (a, b)]
        outs = [torch.zeros((h, w * pb), dtype=torch.uint8, device="cuda:0") for w, h in sizes]
        try:
            batch.decode([t.data_ptr() for t in outs], [w * pb for w, _ in sizes])
            code = ""
        except j40.J40Error as e:
            code = e.code
        torch.cuda.synchronize()
        batch.close()
        if code:
            return ["", code, None, None, None]
        status = [a.status(), b.status()]
        torch.cuda.synchronize()
        return ["", "", status, [digest(t.cpu().numpy(), False, pb) for t in outs], b.alpha()["written"]]

    def modes(fmt=U8X4, scale=(0, 0), alpha=0, region=None, orient=0):
        for f, k in zip((a, b), scale):
            f.set_region(0, 0, 0, 0); f.set_scale(k); f.set_output_format(fmt)
        a.set_orientation(orient)
        if region:
            a.set_region(*region)
        b.set_alpha(alpha)

    table = {}
    for fmt, k, alpha in itertools.product((U8X4, U16X4), (0, 1), (0, 1)):
        modes(fmt, (k, k), alpha)
        table["%s/scale_%d/alpha_%d" % ("u16" if fmt == U16X4 else "u8", k, alpha)] = run()
    modes(scale=(0, 1)); table["scales_differ"] = run()
    modes(region=(20, 30, 100, 80)); table["member_with_a_region"] = run()
    modes(orient=1); table["member_oriented"] = run()
    modes(); b.set_output_format(U16X4); table["formats_differ"] = run()
    a.close(); b.close()
    return table


@pytest.fixture(scope="module")
def gpu(built):
    import j40_amd
    assert j40_amd.device_count() > 0, "the gpu tests need a HIP device"
    return j40_amd


@pytest.fixture(scope="module")
def routes_fixture():
    return load_fixture(ROUTES_FIXTURE)


@pytest.mark.gpu
@pytest.mark.parametrize("part", ROUTE_PARTS, ids=part_id)
def test_routes_decode_as_before_the_route(gpu, routes_fixture, part):
    """every combination of output shape, order, format, restoration, alpha, Modular XYB and group range: decode() + status() and
    decode_to_host() agree on code and pixels, and the setters' codes, the entries' codes, the pixels' SHA-256 and the getters'
    last-decode fields are the fixture's. A refusal is an expected value like any other; no cell is missing or extra."""
    want = {k: v for k, v in routes_fixture["cells"].items() if in_part(k, part)}
    got = route_table(gpu, [part])
    assert sorted(got) == sorted(want)
    for key, cell in got.items():
        assert agree(cell), "decode() + status() and decode_to_host() agree (%s)" % key
        assert cell == want[key], key
    assert refusals(got) == routes_fixture["header"]["refusals_per_part"][part_id(part)], "a run that refuses more is seen"


@pytest.mark.gpu
def test_batch_refusals_and_pixels_as_before_the_route(gpu, routes_fixture):
    got = batch_table(gpu)
    assert sorted(got) == sorted(routes_fixture["batch"])
    for key, row in got.items():
        assert row == routes_fixture["batch"][key], key


def test_routes_fixture_is_whole():
    """the fixture's own header: every cell of the matrix is there, the refused ones are counted"""
    fx = load_fixture(ROUTES_FIXTURE)
    ids = [cell_id(name, c) for name, _, _, dims in ROUTE_STREAMS for c in route_cells(dims)]
    assert sorted(ids) == sorted(fx["cells"]) and len(ids) == fx["header"]["cells"]
    assert {part_id(p): refusals(fx["cells"], p) for p in ROUTE_PARTS} == fx["header"]["refusals_per_part"]
    assert refusals(fx["cells"]) == fx["header"]["refusals"]


# ---------------------------------------------------------------- recording (the commit before, through J40HIP_LIB)

if __name__ == "__main__":
    import j40_amd
    what, out = sys.argv[1], sys.argv[2]
    if what == "record-setters":
        table = setter_table(j40_amd)
        table["cases"] = sum(len(r["pairs"]) + len(r["triples"]) for r in table["handles"].values())
        table["recorded_at_commit"] = sys.argv[3]
    elif what == "record-routes":
        cells = route_table(j40_amd)
        for key, cell in cells.items():
            assert agree(cell), ("the two entries disagree", key, cell)
        # refusals: [setter, decode(), status()] counts, see refusals()
        header = dict(cells=len(cells), refusals=refusals(cells), refusals_per_part={part_id(p): refusals(cells, p) for p in ROUTE_PARTS},
                      recorded_at_commit=sys.argv[3])
        table = dict(header=header, cells=cells, batch=batch_table(j40_amd))
        j40_amd.shutdown()
    else:
        raise SystemExit("record-setters OUT COMMIT | record-routes OUT COMMIT")
    write_fixture(out, table)
    print({k: v for k, v in table.items() if k in ("cases", "header")})
