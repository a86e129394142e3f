#!/usr/bin/env python3
"""Measures the kept alpha channel of VarDCT frames (j40hip_frame_set_alpha) on device 0; one JSON document on stdout.

  decode   j40hip_frame_decode_to_host of one 8K stream with an alpha channel (vardct 7680x4320 seed 7 alpha=1 forward=1), the
           variants -- drop and keep -- alternating in ONE process after a warm-up, every repetition with a device synchronisation
           inside the clock. A build without j40hip_frame_set_alpha (the commit before the feature) measures "drop" alone: run this
           file from that commit's tree for the yardstick and its run-to-run spread.
  merge    k_alpha_merge alone (j40hip_kat_device_alpha_merge) over an 8K image against a device-to-device copy of the same image
           (torch's Tensor.copy_, a hipMemcpyAsync), alternating, timed with events on the stream: the merge moves 10 bytes a
           pixel (u8; 18 for u16), the copy 8 (16).

Usage: python tools/alpha_probe.py [--reps N] [--warmup N] [--skip-decode] [--skip-merge] > profiles/alpha_probe.json
`rocprofv3 --kernel-trace --stats -- python tools/alpha_probe.py --skip-merge --reps 5` gives k_alpha_merge's own time in a decode."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

HBM_PEAK_GB_S = 8000.0   # MI355X: 8 TB/s, the vendor's peak


def summary(ms):
    ms = sorted(ms)
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(ms[0], 4), "max_ms": round(ms[-1], 4),
            "p10_ms": round(ms[len(ms) // 10], 4), "p90_ms": round(ms[(len(ms) * 9) // 10], 4), "n": len(ms)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--skip-decode", action="store_true")
    ap.add_argument("--skip-merge", action="store_true")
    args = ap.parse_args()
    import numpy as np
    import torch
    import j40_amd
    from streams import synth
    L = j40_amd.lib()
    out = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "warmup": args.warmup}
    W, H = 7680, 4320
    if not args.skip_decode:
        data = synth("vardct", W, H, 7, alpha=1, forward=1)
        has_alpha = hasattr(j40_amd.Frame, "set_alpha")
        variants = [("drop", 0)] + ([("keep", 1)] if has_alpha else [])
        frames = {}
        for name, mode in variants:
            fr = j40_amd.Frame(data)
            if has_alpha:
                assert fr.set_alpha(mode) == ""
            fr.upload(0)
            frames[name] = fr
        host = np.zeros((H, W, 4), np.uint8)
        times = {name: [] for name, _ in variants}
        for rep in range(args.warmup + args.reps):
            for name, _ in variants:   # alternating: drift of the machine lands on every variant alike
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                code = L.j40hip_frame_decode_to_host(frames[name].h, host.ctypes.data, W * 4)
                torch.cuda.synchronize()
                dt = (time.perf_counter() - t0) * 1e3
                assert code == 0, code
                if rep >= args.warmup:
                    times[name].append(dt)
            if rep == 0 and has_alpha:
                assert host[..., 3].min() < 255   # (the last variant was keep)
        out["decode_to_host_8k"] = {name: summary(ms) for name, ms in times.items()}
        out["decode_to_host_8k"]["stream_bytes"] = len(data)
        for fr in frames.values():
            fr.close()
    if not args.skip_merge and hasattr(j40_amd.Frame, "set_alpha"):
        stream = torch.cuda.current_stream()
        merge = {}
        for fmt, pb, name in ((j40_amd.J40_U8X4, 4, "u8"), (j40_amd.J40_U16X4, 8, "u16")):
            img = torch.randint(0, 255, (H, W * pb), dtype=torch.uint8, device="cuda:0")
            dst = torch.empty_like(img)
            plane = torch.randint(0, 256, (H, W), dtype=torch.int16, device="cuda:0")
            t_merge, t_copy = [], []
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
            for rep in range(args.warmup + args.reps):
                ev[0].record(stream)
                code = L.j40hip_kat_device_alpha_merge(img.data_ptr(), W * pb, plane.data_ptr(), W, 0, 0, W, H, 8, fmt, stream.cuda_stream)
                ev[1].record(stream)
                dst.copy_(img)
                ev[2].record(stream)
                torch.cuda.synchronize()
                assert code == 0
                if rep >= args.warmup:
                    t_merge.append(ev[0].elapsed_time(ev[1])); t_copy.append(ev[1].elapsed_time(ev[2]))
            m, c = summary(t_merge), summary(t_copy)
            bytes_merge, bytes_copy = W * H * (2 * pb + 2), W * H * 2 * pb
            merge[name] = {"merge": m, "copy": c, "merge_bytes": bytes_merge, "copy_bytes": bytes_copy,
                           "merge_gb_per_s": round(bytes_merge / m["median_ms"] / 1e6, 1), "copy_gb_per_s": round(bytes_copy / c["median_ms"] / 1e6, 1),
                           "merge_share_of_hbm_peak": round(bytes_merge / m["median_ms"] / 1e6 / HBM_PEAK_GB_S, 3), "hbm_peak_gb_per_s": HBM_PEAK_GB_S,
                           "merge_over_copy": round(m["median_ms"] / c["median_ms"], 3), "bytes_ratio": round(bytes_merge / bytes_copy, 3)}
        out["merge_vs_copy_8k"] = merge
    print(json.dumps(out, indent=1))
    j40_amd.shutdown()


if __name__ == "__main__":
    main()
