#!/usr/bin/env python3
"""What upsampling costs. One process on one device:

    k_upsample<2|4|8>      the kernel alone (j40hip_kat_device_upsample) from resident coded planes of ceil(shown / K) to a shown size
                           of 7680 x 4320, between HIP events of the hook's own
    copy                   a device-to-device copy of the same output bytes (3 * 7680 * 4320 floats): the floor of a kernel that is
                           bound by its stores; the ratio kernel / copy is reported
    decode, twin decode    a VarDCT generator stream coded at 3840 x 2160 with upsampling=2 (shown 7680 x 4320) and its twin
                           (uptwin=1, shown at the coded size), each uploaded once and decoded `--rounds` times into device memory in
                           turn: j40hip_frame_decode_timed's three stages summed; J40HIP_UPSAMPLE_TIMING=1 gives the kernel's share

The first `--warmup` rounds are dropped; the median, the minimum and the maximum of the rest are printed and, with --out, written.

    python tools/upsample_probe.py [--width 7680] [--height 4320] [--rounds 12] [--warmup 3] [--out profiles/upsample_probe.json]"""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ["J40HIP_UPSAMPLE_TIMING"] = "1"


def centre_heavy(k):
    """0.6 at the centre taps, small values elsewhere (the tests' shape of table; the kernel's time does not depend on the values)"""
    n5 = 5 * k // 2
    return [0.6 if y % 5 == 2 and x % 5 == 2 else 0.01 for y in range(n5) for x in range(y, n5)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=7680)
    ap.add_argument("--height", type=int, default=4320)
    ap.add_argument("--rounds", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    import j40_amd
    assert j40_amd.device_count() > 0, "the probe measures on the GPU"
    W, H = args.width, args.height
    L = j40_amd.lib()
    rows = {}
    d_out = torch.zeros(3 * H * W, dtype=torch.float32, device="cuda:0")
    d_copy = torch.zeros(3 * H * W, dtype=torch.float32, device="cuda:0")
    for k in (2, 4, 8):
        w, h = -(-W // k), -(-H // k)
        d_in = torch.rand(3 * h * w, dtype=torch.float32, device="cuda:0")
        wt = np.array(centre_heavy(k), np.float32)
        ms = C.c_float(0.0)
        rows["k_upsample_%d" % k] = []
        for _ in range(args.rounds):
            code = L.j40hip_kat_device_upsample(d_in.data_ptr(), w, h, k, wt.ctypes.data, W, H, d_out.data_ptr(), None, C.byref(ms))
            assert code == 0, j40_amd.err4(code)
            rows["k_upsample_%d" % k].append(ms.value * 1e3)
    rows["copy"] = []
    for _ in range(args.rounds):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); d_copy.copy_(d_out); b.record()
        torch.cuda.synchronize()
        rows["copy"].append(a.elapsed_time(b) * 1e3)
    del d_copy, d_out
    # one whole decode beside its twin at the coded size
    cw, ch = -(-W // 2), -(-H // 2)
    streams = {}
    with tempfile.TemporaryDirectory() as d:
        for name, more in (("decode", []), ("twin_decode", ["uptwin=1"])):
            path = os.path.join(d, name + ".jxl")
            subprocess.run([os.path.join(ROOT, "build", "jxlsynth"), "vardct", str(cw), str(ch), "7", path, "upsampling=2", "upweights=" + ",".join(repr(v) for v in centre_heavy(2)),
                            "upshown=%d,%d" % (W, H)] + more, check=True, stderr=subprocess.DEVNULL)
            with open(path, "rb") as fp:
                streams[name] = fp.read()
    out = torch.zeros((H, W * 4), dtype=torch.uint8, device="cuda:0")
    frames = {name: j40_amd.Frame(data, upsampling=True) for name, data in streams.items()}
    for fr in frames.values():
        fr.upload(0)
    rows.update({"decode": [], "twin_decode": [], "k_upsample_in_decode": []})
    for _ in range(args.rounds):
        for name, fr in frames.items():
            ms3 = fr.decode_timed(out.data_ptr(), W * 4)
            torch.cuda.synchronize()
            assert fr.status() == ""
            rows[name].append(float(ms3.sum()) * 1e3)
            if name == "decode":
                rows["k_upsample_in_decode"].append(fr.upsample_ms() * 1e3)
    for fr in frames.values():
        fr.close()
    result = {}
    for name, us in rows.items():
        kept = us[args.warmup:] if len(us) > args.warmup else us
        result[name] = {"rounds": len(us), "median_us": statistics.median(kept), "min_us": min(kept), "max_us": max(kept)}
        print("%-22s %3d rounds, median %9.1f us (min %.1f, max %.1f)" % (name, len(us), statistics.median(kept), min(kept), max(kept)))
    out_bytes = 12.0 * W * H
    result["output_bytes"] = out_bytes
    for k in (2, 4, 8):
        r = result["k_upsample_%d" % k]["median_us"] / result["copy"]["median_us"]
        result["k_upsample_%d" % k]["over_copy"] = r
        print("k_upsample<%d>: %.2f x the copy of its %.0f MB of output (%.0f GB/s written)" % (k, r, out_bytes / 1e6, out_bytes / 1e3 / result["k_upsample_%d" % k]["median_us"]))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fp:
            json.dump({"what": "tools/upsample_probe.py: shown %d x %d, %d rounds, the first %d dropped; microseconds" % (W, H, args.rounds, args.warmup), "rows": result}, fp, indent=1)
            fp.write("\n")
    j40_amd.shutdown()


if __name__ == "__main__":
    main()
