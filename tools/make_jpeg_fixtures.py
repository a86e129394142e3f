#!/usr/bin/env python3
"""Writes tests/golden/jpeg/: real baseline JPEG files from a real encoder and a real decoder's picture of each (TEST INFRASTRUCTURE).

Run by hand where Pillow (with libjpeg) is installed: python tools/make_jpeg_fixtures.py. Nothing else calls it -- the tests, build(),
smoke() and bench.py read the committed files only. For every row of ROWS: NAME.jpg (Pillow's encode of a procedural picture) and
NAME.rgb.npy (Pillow's own decode of that file, u8 [h, w, 3]); manifest.json with sizes, hashes and, per fixture, how far
tests/jpeg_ref.py's float64 decode (edge="libjpeg", clamp=True, rounded) lies from Pillow's (test a of tests/test_jpeg_transcode.py asserts that
maximum). Keys of the manifest this script does not compute (the measured plane bound of test b) are kept when it is run again."""
import hashlib
import io
import json
import os
import sys

import numpy as np
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import jpeg_ref   # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "jpeg")
SEED = 20

# two non-standard tables, [v][u] (row: vertical frequency), NOT symmetric: luma coarser along x, chroma coarser along y
LUMA = [[2 + 2 * u + v + (3 if (u, v) == (1, 0) else 0) for u in range(8)] for v in range(8)]
CHROMA = [[3 + u + 3 * v + (5 if (u, v) == (0, 1) else 0) for u in range(8)] for v in range(8)]

# name, width, height, subsampling, save options
ROWS = [
    ("q90_444_8x8", 8, 8, "4:4:4", dict(quality=90)),
    ("q75_420_16x16", 16, 16, "4:2:0", dict(quality=75)),
    ("q75_420_17x9", 17, 9, "4:2:0", dict(quality=75)),
    ("q75_422_40x24", 40, 24, "4:2:2", dict(quality=75)),
    ("q30_444_40x24", 40, 24, "4:4:4", dict(quality=30, optimize=True)),
    ("q98_420_40x24", 40, 24, "4:2:0", dict(quality=98)),
    ("custom_420_264x40", 264, 40, "4:2:0", dict(qtables="custom")),
    ("q75_420_24x264", 24, 264, "4:2:0", dict(quality=75)),
]


def picture(w, h, seed):
    """smooth gradients, saturated colour edges, texture: u8 [h, w, 3]"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    u, v = x / max(w - 1, 1), y / max(h - 1, 1)
    img = np.stack([40 + 170 * u, 60 + 150 * (1 - v), 90 + 120 * (0.5 * u + 0.5 * v)], -1)
    # saturated rectangles: primaries and their complements, edges that fall inside blocks and across chroma samples
    colours = [(255, 0, 0), (0, 255, 0), (0, 0, 255), (255, 255, 0), (255, 0, 255), (0, 255, 255), (255, 255, 255), (0, 0, 0)]
    for k in range(max(2, (w * h) // 60)):
        cx, cy = rng.integers(0, w), rng.integers(0, h)
        rw, rh = rng.integers(2, max(3, w // 3 + 1)), rng.integers(2, max(3, h // 3 + 1))
        img[cy:cy + rh, cx:cx + rw] = colours[k % 8]
    img += rng.normal(0, 14, (h, w, 1)) + rng.normal(0, 6, (h, w, 3))   # texture: every frequency present
    img += (((x.astype(np.int64) + y.astype(np.int64)) & 1) * 70.0 - 35.0)[..., None] * (((x // 5 + y // 3) % 3) == 0)[..., None]   # patches of the highest frequency
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)


def natural(t):
    """Pillow takes a table as 64 values in natural order, row = vertical frequency (the parse of the file it writes is asserted below)"""
    return [int(v) for v in np.asarray(t).reshape(64)]


def main():
    os.makedirs(OUT, exist_ok=True)
    path = os.path.join(OUT, "manifest.json")
    old = json.load(open(path)) if os.path.exists(path) else {}
    manifest = {k: v for k, v in old.items() if k != "fixtures"}
    manifest["fixtures"] = []
    for i, (name, w, h, sub, opts) in enumerate(ROWS):
        src = picture(w, h, SEED + i)
        assert len(np.unique(src.reshape(-1, 3), axis=0)) > min(32, w * h // 2), "%s: a flat field pins nothing" % name
        opts = dict(opts)
        if opts.get("qtables") == "custom":
            opts["qtables"] = [natural(LUMA), natural(CHROMA)]
        buf = io.BytesIO()
        Image.fromarray(src).save(buf, "JPEG", subsampling=sub, **opts)
        data = buf.getvalue()
        rgb = np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))
        assert rgb.shape == (h, w, 3) and len(data) < 16384
        p = jpeg_ref.parse(data)
        assert p.subsampling == sub.replace(":", ""), (name, p.subsampling)
        for c in p.components:
            ac = np.abs(c.coef).sum() - np.abs(c.coef[..., 0, 0]).sum()
            assert ac > 0 and (np.ptp(c.coef[..., 0, 0]) > 0 or c.coef.shape[:2] == (1, 1)), "%s: component %d is flat" % (name, c.id)
        assert np.abs(p.components[0].coef[..., 4:, 4:]).sum() > 0, "%s: no high frequencies" % name
        if "qtables" in opts:
            assert np.array_equal(p.components[0].table, np.array(LUMA)) and np.array_equal(p.components[1].table, np.array(CHROMA)), "the file's tables are not the ones asked for"
            assert not np.array_equal(p.components[0].table, p.components[0].table.T) and not np.array_equal(p.components[1].table, p.components[1].table.T)
        _, u8, _ = jpeg_ref.decode_f64(p, "libjpeg", clamp=True)
        free = (jpeg_ref.decode_f64(p, "libjpeg")[0] == jpeg_ref.decode_f64(p, "libjpeg", clamp=True)[0]).all(-1)
        d = np.abs(u8.astype(np.int32) - rgb.astype(np.int32))
        hist = [int((d == k).sum()) for k in range(int(d.max()) + 1)]
        # libjpeg rounds three times: after its inverse DCT (whose integer form may itself be one level off, IEEE 1180), after the
        # upsampling of a subsampled component (half a level), after the colour conversion (half a level). A chroma error enters R
        # with gain 1.402, B with 1.772, G with 0.344 + 0.714: worst cases 1 + gain * 1.5 + 0.5 = 3.6, 3.1, 4.2 levels. Beyond that
        # something is wrong with the parser or the reference; typical maxima are 2, with a rare 3 in B.
        worst = [int(d[..., k].max()) for k in range(3)]
        assert worst[0] <= 3 and worst[1] <= 3 and worst[2] <= 4 and (d > 2).sum() * 1000 < d.size, "%s: %s levels from Pillow's decode cannot come from rounding: %s" % (name, worst, hist)
        with open(os.path.join(OUT, name + ".jpg"), "wb") as fp:
            fp.write(data)
        np.save(os.path.join(OUT, name + ".rgb.npy"), rgb)
        manifest["fixtures"].append(dict(
            name=name, width=w, height=h, subsampling=p.subsampling, bytes=len(data),
            sha256_jpg=hashlib.sha256(data).hexdigest(), sha256_rgb_npy=hashlib.sha256(open(os.path.join(OUT, name + ".rgb.npy"), "rb").read()).hexdigest(),
            unclamped_pixel_share=round(float(free.mean()), 4), f64_vs_pillow_max=int(d.max()), f64_vs_pillow_histogram=hist,
            max_table_entry=int(max(c.table.max() for c in p.components)), max_abs_coefficient=int(max(np.abs(c.coef).max() for c in p.components))))
        print("%-20s %4d bytes  |f64 - Pillow| max %d  histogram %s" % (name, len(data), d.max(), hist))
    with open(path, "w") as fp:
        json.dump(manifest, fp, indent=1, sort_keys=True)
        fp.write("\n")


if __name__ == "__main__":
    main()
