"""What the LF preview costs on the forward-encoded 8K stream bench.py uses (synth("vardct", 7680, 4320, 3, forward=1)):

  - lf_end as a share of the codestream (the bytes a preview needs);
  - host to host: LF-only parse + upload + decode_lf_to_host, next to the full j40hip_frame_decode_to_host of the same frame;
  - j40hip_frames_decode_lf over N 8K frames in one launch: the launch's device time (HIP events around it) and the bytes it moves
    (6 B read + 4 B written per cell) against the MI355X's HBM peak (8 TB/s).

Prints one JSON line. usage: python tools/lf_preview_probe.py [--frames 256] [--reps 5]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

HBM_PEAK_GBPS = 8000.0   # MI355X: 8 TB/s HBM3E


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    import numpy as np
    import torch
    import j40_amd
    from streams import synth
    data = synth("vardct", 7680, 4320, 3, forward=1)
    full = j40_amd.Frame(data)
    lf_end, cs = full.lf_end(), full.codestream_size
    full.upload(0)
    out = {"stream": "vardct 7680x4320 seed 3 forward=1", "codestream_bytes": cs, "lf_end": lf_end, "lf_end_share": round(lf_end / cs, 4)}

    # host to host, best of reps (the first of each is a warm-up)
    def best(fn):
        fn()
        ts = []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            fn()
            ts.append((time.perf_counter() - t0) * 1e3)
        return round(min(ts), 3), round(float(np.median(ts)), 3)

    prefix = data[:lf_end]

    def preview():
        fr = j40_amd.Frame(prefix, lf_only=True)
        fr.upload(0)
        px = fr.decode_lf_to_host()
        fr.close()
        return px

    def whole():
        err, px = full.decode_to_host()
        assert err == ""
        return px

    out["preview_host_to_host_ms"] = dict(zip(("best", "median"), best(preview)))
    out["full_decode_to_host_ms"] = dict(zip(("best", "median"), best(whole)))
    full.close()

    # many frames, one launch: the kernel alone
    frames = []   # (frames of their own, so that every frame's LF integers come from HBM)
    for _ in range(args.frames):
        fr = j40_amd.Frame(prefix, lf_only=True)
        fr.upload(0)
        frames.append(fr)
    w8, h8 = frames[0].lf_size()
    buf = torch.empty((args.frames, h8, w8 * 4), dtype=torch.uint8, device="cuda:0")
    stream = torch.cuda.current_stream()
    ptrs, strides = [buf[i].data_ptr() for i in range(args.frames)], [w8 * 4] * args.frames
    assert j40_amd.frames_decode_lf(frames, ptrs, strides, stream.cuda_stream) == ""   # warm-up (and the pooled argument buffers)
    ms = []
    for _ in range(args.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        assert j40_amd.frames_decode_lf(frames, ptrs, strides, stream.cuda_stream) == ""
        e1.record(stream)
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    cells = w8 * h8 * args.frames
    moved = cells * (6 + 4)
    kms = min(ms)
    out["batch"] = {"frames": args.frames, "cells": cells, "bytes_moved": moved, "launch_ms_best": round(kms, 4), "launch_ms_median": round(float(np.median(ms)), 4),
                    "gb_per_s": round(moved / kms / 1e6, 1), "share_of_hbm_peak": round(moved / kms / 1e6 / HBM_PEAK_GBPS, 4),
                    "note": "event-timed launch (argument copy + kernel); the kernel's own time comes from rocprofv3 --kernel-trace --stats"}
    for fr in frames:
        fr.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
