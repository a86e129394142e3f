#!/usr/bin/env python3
"""What photon noise costs. One process: a 7680 x 4320 generator stream with noise= and its twin (noisetwin=1),
each parsed and uploaded once and decoded `--rounds` times into device memory, the two in turn, J40HIP_NOISE_TIMING=1.

    k_noise_fill, k_noise_add   the two kernels' device time in the noisy decode, between HIP events of the decode's own
                                (j40hip_frame_noise_ms)
    noisy decode, twin decode   j40hip_frame_decode_timed's three stages summed (clear, entropy, pixels)
    the kernels alone           j40hip_kat_device_noise over resident planes of the same size, with the frame's group side (256)

The first `--warmup` rounds are dropped; the median, the minimum and the maximum of the rest are printed and, with --out, written.

    python tools/noise_probe.py [--width 7680] [--height 4320] [--rounds 15] [--warmup 3] [--out profiles/noise_probe.json]"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ["J40HIP_NOISE_TIMING"] = "1"

LUT = "100,200,300,400,500,600,700,1023"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=7680)
    ap.add_argument("--height", type=int, default=4320)
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    import j40_amd
    assert j40_amd.device_count() > 0, "the probe measures on the GPU"
    w, h = args.width, args.height
    streams = {}
    with tempfile.TemporaryDirectory() as d:
        for name, more in (("noisy", []), ("twin", ["noisetwin=1"])):
            path = os.path.join(d, name + ".jxl")
            subprocess.run([os.path.join(ROOT, "build", "jxlsynth"), "vardct", str(w), str(h), "7", path, "noise=" + LUT] + more, check=True, stderr=subprocess.DEVNULL)
            with open(path, "rb") as fp:
                streams[name] = fp.read()
    out = torch.zeros((h, w * 4), dtype=torch.uint8, device="cuda:0")
    frames = {name: j40_amd.Frame(data, noise=True) for name, data in streams.items()}
    for fr in frames.values():
        fr.upload(0)
    rows = {"k_noise_fill": [], "k_noise_add": [], "noisy_decode": [], "twin_decode": [], "kat_fill": [], "kat_add": []}
    for _ in range(args.rounds):
        for name, fr in frames.items():
            ms = fr.decode_timed(out.data_ptr(), w * 4)
            torch.cuda.synchronize()
            assert fr.status() == ""
            rows[name + "_decode"].append(float(ms.sum()) * 1e3)
            if name == "noisy":
                fill, add = fr.noise_ms()
                rows["k_noise_fill"].append(fill * 1e3); rows["k_noise_add"].append(add * 1e3)
    assert frames["noisy"].noise_launches() == args.rounds and frames["twin"].noise_launches() == 0
    for fr in frames.values():
        fr.close()
    planes = np.zeros((3, h, w), np.float32)
    planes[1:] = 0.5
    lut = np.array([int(v) for v in LUT.split(",")], np.float32) / np.float32(1024)
    for _ in range(min(args.rounds, 6)):
        code, _, _, ms = j40_amd.kat_device_noise(planes, 256, lut, 0.0, 1.0, want_ms=True)
        assert code == ""
        rows["kat_fill"].append(ms[0] * 1e3); rows["kat_add"].append(ms[1] * 1e3)
    result = {}
    for name, us in rows.items():
        kept = us[args.warmup:] if len(us) > args.warmup else us
        result[name] = {"rounds": len(us), "median_us": statistics.median(kept), "min_us": min(kept), "max_us": max(kept)}
        print("%-14s %3d rounds, median %9.1f us (min %.1f, max %.1f)" % (name, len(us), statistics.median(kept), min(kept), max(kept)))
    moved = 36.0 * w * h     # the fill writes three planes, the addition reads them and reads and writes the frame's three: 36 bytes a pixel
    result["bytes_moved"] = moved
    print("36 bytes a pixel: %.1f MB; at the kernels' median that is %.0f GB/s" % (moved / 1e6, moved / 1e3 / (result["k_noise_fill"]["median_us"] + result["k_noise_add"]["median_us"])))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fp:
            json.dump({"what": "tools/noise_probe.py: %d x %d, %d rounds, the first %d dropped; microseconds" % (w, h, args.rounds, args.warmup), "rows": result}, fp, indent=1)
            fp.write("\n")
    j40_amd.shutdown()


if __name__ == "__main__":
    main()
