#!/usr/bin/env python3
"""Measures the YCbCr path (j40hip_frame_set_ycbcr) on device 0; one JSON document on stdout.

  tail     k_ycbcr_tail alone (j40hip_kat_device_ycbcr_tail) on 7680 x 4320 planes, 4:4:4 and 4:2:0, u8x4: timed with events on
           the stream around runs of 50 launches after a warm-up. Per pixel it moves 3 x 4 + 4 = 16 bytes (4:4:4) or
           4 + 2 x 1 + 4 = 10 bytes (4:2:0); the rate is those bytes over the time. A device-to-device copy of the same output
           image plus as many bytes of input (torch's Tensor.copy_) is timed beside it as the yardstick of what this device
           moves. The launches repeat over the same buffers (531 MB and 332 MB, more than the 256 MiB Infinity Cache).
  decode   j40hip_frame_decode of one 8K stream coded three ways from the same procedural picture (vardct 7680x4320 seed 3
           forward=1): ycbcr=1 (4:4:4: the planes of OutMode::XYB, then the tail), its twin noxyb=1 (the fused colour tail of the
           pixel kernels), and ycbcr=1 subsampling=420 (OutMode::YCC planes, then the tail). Alternating in one process after a
           warm-up, events on the stream. ycbcr minus twin is what going through planes costs against a fused tail.

Usage: python tools/ycbcr_probe.py [--reps N] [--skip-decode] > profiles/ycbcr_probe.json"""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--skip-decode", action="store_true")
    args = ap.parse_args()
    import numpy as np
    import torch
    import j40_amd
    from streams import synth
    from ycbcr_ref import SHIFTS, plane_shapes, U8X4

    L = j40_amd.lib()
    W, H = 7680, 4320
    res = {"width": W, "height": H}
    s = torch.cuda.current_stream().cuda_stream
    rng = np.random.default_rng(1)

    def timed(run, n):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(n):
            run()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / n

    for sub in ("444", "420"):
        shapes = plane_shapes(W, H, sub)
        planes = [torch.from_numpy(rng.uniform(-0.5 if c != 1 else 0.0, 0.5 if c != 1 else 1.0, sh).astype(np.float32)).to("cuda:0") for c, sh in enumerate(shapes)]
        out = torch.zeros((H, W, 4), dtype=torch.uint8, device="cuda:0")
        ptrs = (C.c_void_p * 3)(*[p.data_ptr() for p in planes])
        dims = (C.c_int32 * 9)(*[v for sh in shapes for v in (sh[1], sh[1], sh[0])])
        shifts = (C.c_int32 * 6)(*[v for p in SHIFTS[sub] for v in p])
        bytes_per_pixel = 16 if sub == "444" else 10
        total = W * H * bytes_per_pixel
        src = torch.zeros(total // 2, dtype=torch.uint8, device="cuda:0")   # a copy reads and writes: half the bytes each way
        dst = torch.zeros_like(src)

        def tail():
            assert L.j40hip_kat_device_ycbcr_tail(ptrs, dims, shifts, W, H, 8, U8X4, out.data_ptr(), W * 4, s) == 0

        def copy():
            dst.copy_(src)

        for _ in range(10):
            tail(); copy()
        torch.cuda.synchronize()
        t_tail, t_copy = [], []
        for _ in range(args.reps):
            t_tail.append(timed(tail, 50)); t_copy.append(timed(copy, 50))
        ms, cms = float(np.median(t_tail)), float(np.median(t_copy))
        res["tail_" + sub] = dict(ms=t_tail, median_ms=ms, bytes_per_pixel=bytes_per_pixel, megabytes=total / 1e6, tb_per_s=total / (ms * 1e-3) / 1e12,
                                  copy_same_bytes_ms=t_copy, copy_median_ms=cms, copy_tb_per_s=total / (cms * 1e-3) / 1e12)
        del planes, out, src, dst

    if not args.skip_decode:
        streams = {"ycbcr_444": synth("vardct", W, H, 3, ycbcr=1, forward=1), "twin_noxyb": synth("vardct", W, H, 3, noxyb=1, fullheader=1, forward=1),
                   "ycbcr_420": synth("vardct", W, H, 3, ycbcr=1, subsampling=420, forward=1)}
        out = torch.zeros((H, W, 4), dtype=torch.uint8, device="cuda:0")
        frames = {}
        for k, data in streams.items():
            f = j40_amd.Frame(data, threads=8, ycbcr=True)
            f.set_ycbcr(1)
            f.upload(0)
            frames[k] = f
            for _ in range(3):
                f.decode(out.data_ptr(), W * 4, s)
            torch.cuda.synchronize()
            assert f.status() == "", (k, f.status())
        times = {k: [] for k in frames}
        for _ in range(args.reps):
            for k, f in frames.items():
                times[k].append(timed(lambda: f.decode(out.data_ptr(), W * 4, s), 5))
        for k, f in frames.items():
            res["decode_" + k] = dict(ms=times[k], median_ms=float(np.median(times[k])), codestream_bytes=len(streams[k]))
            f.close()
        res["planes_instead_of_fused_tail_ms"] = res["decode_ycbcr_444"]["median_ms"] - res["decode_twin_noxyb"]["median_ms"]
    print(json.dumps(res, indent=1))
    j40_amd.shutdown()


if __name__ == "__main__":
    main()
