#!/usr/bin/env python3
"""What splines cost. One process: a 7680 x 4320 generator stream with splines= and its twin (splinetwin=1),
each parsed and uploaded once and decoded `--rounds` times into device memory, the two in turn, J40HIP_SPLINE_TIMING=1.

    k_spline_draw               the kernel's device time in the splined decode, between HIP events of the decode's own
                                (j40hip_frame_spline_ms)
    splined decode, twin decode j40hip_frame_decode_timed's three stages summed (clear, entropy, pixels)
    parse                       the host's time for j40hip_frame_parse_ex of either stream: the difference is the spline data's
                                entropy decode, the dequantisation into segments and their binning

The workload: `--splines` curves of five control points each, left to right across the frame with a vertical wiggle, sigma about 2.4
samples, colours on all three channels; the segments, the touched tiles and the (tile, segment) pairs are printed with the times.
The first `--warmup` rounds are dropped; the median, the minimum and the maximum of the rest are printed and, with --out, written.

    python tools/spline_probe.py [--width 7680] [--height 4320] [--splines 64] [--rounds 15] [--warmup 3] [--out profiles/spline_probe.json]"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ["J40HIP_SPLINE_TIMING"] = "1"


def description(w, h, count):
    """count curves, each five control points from the left edge to the right one, as the generator takes them (double deltas)"""
    parts = []
    for k in range(count):
        y = (2 * k + 1) * h // (2 * count)
        swing = max(8, h // (3 * count))
        pts = [(40 + i * (w - 80) // 4, y + (swing if i % 2 else -swing) * (1 if k % 2 else -1)) for i in range(5)]
        dd, delta, cur = [], (0, 0), pts[0]
        for p in pts[1:]:
            step = (p[0] - cur[0], p[1] - cur[1])
            dd.append((step[0] - delta[0], step[1] - delta[1]))
            delta, cur = step, p
        parts.append(":".join(["%d,%d" % pts[0]] + ["%d,%d" % d for d in dd]) + "|0:0=%d,1:0=%d,1:1=9,2:0=%d,3:0=10,3:2=1" % (12 + k % 5, 30 + k % 7, -16 + k % 3))
    return "/".join(parts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=7680)
    ap.add_argument("--height", type=int, default=4320)
    ap.add_argument("--splines", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import j40_amd
    assert j40_amd.device_count() > 0, "the probe measures on the GPU"
    w, h = args.width, args.height
    streams = {}
    with tempfile.TemporaryDirectory() as d:
        for name, more in (("splined", []), ("twin", ["splinetwin=1"])):
            path = os.path.join(d, name + ".jxl")
            subprocess.run([os.path.join(ROOT, "build", "jxlsynth"), "vardct", str(w), str(h), "7", path, "splines=" + description(w, h, args.splines)] + more, check=True, stderr=subprocess.DEVNULL)
            with open(path, "rb") as fp:
                streams[name] = fp.read()
    out = torch.zeros((h, w * 4), dtype=torch.uint8, device="cuda:0")
    frames, parse_ms = {}, {}
    for name, data in streams.items():
        t0 = time.perf_counter()
        frames[name] = j40_amd.Frame(data, splines=True)
        parse_ms[name] = (time.perf_counter() - t0) * 1e3
    segments = int(frames["splined"].spline_segments().shape[0])
    tiles, pairs = frames["splined"].spline_bins()
    for fr in frames.values():
        fr.upload(0)
    rows = {"k_spline_draw": [], "splined_decode": [], "twin_decode": []}
    for _ in range(args.rounds):
        for name, fr in frames.items():
            ms = fr.decode_timed(out.data_ptr(), w * 4)
            torch.cuda.synchronize()
            assert fr.status() == ""
            rows[name + "_decode"].append(float(ms.sum()) * 1e3)
            if name == "splined":
                rows["k_spline_draw"].append(fr.spline_ms() * 1e3)
    assert frames["splined"].spline_launches() == args.rounds and frames["twin"].spline_launches() == 0
    for fr in frames.values():
        fr.close()
    result = {"workload": {"width": w, "height": h, "splines": args.splines, "segments": segments, "tiles": tiles, "tile_segment_pairs": pairs,
                           "parse_ms_splined": parse_ms["splined"], "parse_ms_twin": parse_ms["twin"]}}
    print("%d x %d, %d splines: %d segments (the arc length in samples), %d of %d tiles touched, %d (tile, segment) pairs" % (w, h, args.splines, segments, tiles, ((w + 63) // 64) * ((h + 31) // 32), pairs))
    print("parse: %.1f ms with the splines, %.1f ms the twin" % (parse_ms["splined"], parse_ms["twin"]))
    for name, us in rows.items():
        kept = us[args.warmup:] if len(us) > args.warmup else us
        result[name] = {"rounds": len(us), "median_us": statistics.median(kept), "min_us": min(kept), "max_us": max(kept)}
        print("%-15s %3d rounds, median %9.1f us (min %.1f, max %.1f)" % (name, len(us), statistics.median(kept), min(kept), max(kept)))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fp:
            json.dump({"what": "tools/spline_probe.py: %d x %d, %d splines, %d rounds, the first %d dropped; microseconds" % (w, h, args.splines, args.rounds, args.warmup), "rows": result}, fp, indent=1)
            fp.write("\n")
    j40_amd.shutdown()


if __name__ == "__main__":
    main()
