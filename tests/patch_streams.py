"""Patch streams for tests/test_patches.py and tests/test_patches_gpu.py (TEST INFRASTRUCTURE): the generator's types= / patches= streams,
their twins, the numpy statement of what patches do, and the shapes the tests share.

The generator cannot write a one-group XYB VarDCT frame, so a VarDCT reference-only frame is wider than 256 pixels. The VarDCT main
frame is 300 x 270: four groups, five by nine tiles of 64 x 32 with a partial last column and row. The Modular one is 200 x 136."""
import hashlib
import json
import os
import subprocess
import tempfile

import numpy as np

from streams import SYNTH, CACHE

SEED = 7
VW, VH = 300, 270            # the VarDCT main frame
MW, MH = 200, 136            # the Modular main frame, and the planes of the kernel's known-answer cases
REF_V = (264, 40)            # a VarDCT reference-only frame (two groups), smaller than the frame
REF_M = (90, 50)             # a Modular one
NONE, REPLACE, ADD, MUL = 0, 1, 2, 3
TILE_W, TILE_H = 64, 32      # device/patch_dev.h


def patch_synth(mode, w, h, seed=SEED, stats=False, **opts):
    """the generator's stream for these options (cached by a hash of them: the values hold characters no file name should), or with
    stats=True what it says of the stream (stats=1)"""
    args = [SYNTH, mode, str(w), str(h), str(seed)]
    tail = ["%s=%s" % kv for kv in sorted(opts.items())]
    if stats:
        with tempfile.TemporaryDirectory() as d:
            text = subprocess.run(args + [os.path.join(d, "s.jxl"), "stats=1"] + tail, check=True, stdout=subprocess.PIPE, stderr=subprocess.DEVNULL).stdout.decode()
        return json.loads(text.strip().splitlines()[-1])
    os.makedirs(CACHE, exist_ok=True)
    path = os.path.join(CACHE, "patch_%s_%d_%d_%d_%s.jxl" % (mode, w, h, seed, hashlib.sha256(" ".join(tail).encode()).hexdigest()[:24]))
    if not os.path.exists(path):
        tmp = path + ".tmp%d" % os.getpid()
        subprocess.run(args + [tmp] + tail, check=True, stderr=subprocess.DEVNULL)
        os.replace(tmp, path)
    with open(path, "rb") as fp:
        return fp.read()


def dictionary(refs):
    """patches= text of one frame. refs: [(slot, x0, y0, w, h, [(x, y, mode, clamp), ...]), ...]"""
    return "/".join("%d,%d,%d,%d,%d:" % r[:5] + ":".join("%d,%d,%d,%d" % p for p in r[5]) for r in refs)


def flat(refs):
    """the placements in dictionary order, as the hooks take and give them: rows x, y, w, h, x0, y0, slot, mode, clamp"""
    return [(x, y, r[3], r[4], r[1], r[2], r[0], mode, clamp) for r in refs for (x, y, mode, clamp) in r[5]]


# the main frame's dictionary in most tests: two slots, every mode, count > 1 with negative deltas, overlaps in both orders, a 1 x 1
# patch on a tile corner, one over four tiles, one that ends at the frame's last column and row
def main_refs(w, h, big, small):
    """big: the size of the reference frame in slot 1, small: of the one in slot 2"""
    return [
        (1, 2, 3, 16, 24, [(70, 40, REPLACE, 0), (5, 8, ADD, 0), (60, 20, ADD, 0), (w - 16, h - 24, REPLACE, 0)]),   # the second and third step left / up; the third straddles four tiles
        (2, 0, 0, 1, 1, [(TILE_W, TILE_H, REPLACE, 0), (TILE_W - 1, TILE_H - 1, ADD, 0)]),
        (2, 4, 5, 30, 20, [(100, 60, ADD, 0), (110, 70, REPLACE, 0), (150, 60, REPLACE, 0), (160, 70, ADD, 0)]),      # Add then Replace, Replace then Add
        (1, big[0] - 40, big[1] - 10, 40, 10, [(10, 100, MUL, 0), (10, 115, MUL, 1), (20, 105, NONE, 0)]),
        (2, small[0] - 8, small[1] - 8, 8, 8, [(w - 8, 0, MUL, 1)]),
    ]


def seq_opts(main, refs, ref_sizes, ref_modes, **more):
    """options of a stream with one reference-only frame per entry of ref_sizes (slot k + 1, written by ref_modes[k]: "v" or "m") and then
    the main frame (`main`: "v" or "m") with dictionary `refs`"""
    n = len(ref_sizes)
    opts = dict(frames=n + 1, types=",".join(["2"] * n + ["0"]), crops=";".join("0,0,%d,%d" % s for s in ref_sizes) + ";",
                saves=",".join(str(k + 1) for k in range(n)) + ",0", patches=";" * n + dictionary(refs))
    modes = list(ref_modes) + [main]
    if len(set(modes)) > 1 or modes[0] != main:
        opts["modes"] = ",".join(modes)
    if "m" in modes:
        opts["xyb"] = 1
    opts.update(more)
    return opts


def apply_patches(planes, slots, placements):
    """the statement: planes [3, h, w] float32, slots {slot: [3, sh, sw] float32}, placements as flat() gives them, applied in order, one
    float32 operation per sample and channel"""
    out = np.array(planes, np.float32, copy=True)
    for (x, y, w, h, x0, y0, slot, mode, clamp) in placements:
        s = slots[slot][:, y0:y0 + h, x0:x0 + w]
        assert s.shape == (3, h, w)
        d = out[:, y:y + h, x:x + w]
        if mode == REPLACE:
            d[...] = s
        elif mode == ADD:
            d[...] = d + s
        elif mode == MUL:
            d[...] = d * (np.minimum(np.maximum(s, np.float32(0)), np.float32(1)) if clamp else s)
        else:
            assert mode == NONE
    return out


def tiles_touched(placements, w, h):
    """for every tile (row-major id) a placement other than None touches: the placements' numbers, in dictionary order"""
    tiles = {}
    tx = (w + TILE_W - 1) // TILE_W
    for i, (x, y, pw, ph, _, _, _, mode, _) in enumerate(placements):
        if mode == NONE:
            continue
        for ty in range(y // TILE_H, (y + ph - 1) // TILE_H + 1):
            for txi in range(x // TILE_W, (x + pw - 1) // TILE_W + 1):
                tiles.setdefault(ty * tx + txi, []).append(i)
    return tiles


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def kat_cases(rng):
    """the kernel's known-answer cases on MW x MH planes: (name, slots, placements). Slot 0 is larger than the frame, slot 3 small; the
    sources reach outside [0, 1]"""
    slots = {0: rng.uniform(-1.5, 2.5, (3, MH + 40, MW + 60)).astype(np.float32), 3: rng.uniform(-1.5, 2.5, (3, 33, 47)).astype(np.float32)}
    cases = [
        ("one_sample_on_a_tile_corner", [(TILE_W, TILE_H, 1, 1, 5, 6, 0, REPLACE, 0), (TILE_W - 1, TILE_H - 1, 1, 1, 0, 0, 3, ADD, 0)]),
        ("straddles_four_tiles", [(TILE_W - 7, TILE_H - 5, 20, 11, 100, 90, 0, ADD, 0)]),
        ("ends_at_the_last_column_and_row", [(MW - 47, MH - 33, 47, 33, 0, 0, 3, REPLACE, 0)]),
        ("replace_then_add", [(30, 30, 40, 40, 10, 10, 0, REPLACE, 0), (50, 50, 40, 30, 0, 0, 3, ADD, 0)]),
        ("add_then_replace", [(50, 50, 40, 30, 0, 0, 3, ADD, 0), (30, 30, 40, 40, 10, 10, 0, REPLACE, 0)]),
        ("mul_with_and_without_clamp", [(0, 0, 90, 60, 3, 3, 0, MUL, 0), (100, 0, 90, 60, 3, 3, 0, MUL, 1), (40, 70, 47, 33, 0, 0, 3, MUL, 1)]),
        ("two_slots_one_larger_than_the_frame", [(0, 0, MW, MH, 60, 40, 0, REPLACE, 0), (150, 100, 47, 33, 0, 0, 3, MUL, 0), (0, 0, MW, MH, 0, 0, 0, ADD, 0)]),
        ("none_touches_nothing", [(0, 0, MW, MH, 0, 0, 0, NONE, 0)]),
        ("many_records_in_one_tile", [(3 + i % 9, 2 + i % 7, 20, 12, i % 11, i % 5, 0 if i % 3 else 3, 1 + i % 3, i % 2) for i in range(150)]),   # three chunks of records
    ]
    return slots, cases
