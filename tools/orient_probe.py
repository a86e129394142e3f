#!/usr/bin/env python3
"""What the oriented output costs ("Oriented output"). k_orient alone through j40hip_kat_device_orient on a
7680 x 4320 image: each orientation 2..8, both formats, warm-up then one timed region between two events on the stream, several
regions, the median -- and, in the same run, a device-to-device hipMemcpyAsync of the same bytes between the same buffers: the
copy reads and writes every byte once, as k_orient must, so it is the yardstick (each case also as a fraction of the copy's rate).
Both are taken twice: over one pair of buffers (largely resident in the Infinity Cache) and rotating over several pairs (HBM).
Then one 8K frame through j40hip_frame_decode_to_host, oriented (orientation 6) against the same handle in stored order: the
difference is what the feature costs a caller.

    python tools/orient_probe.py [--iters 2000] [--pairs 5] [--regions 5] [--decodes 7] [--out profiles/orient_probe.json]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def timed_regions(torch, stream, fn, iters, regions, warmup=3):
    """milliseconds per call: the median over `regions` regions of `iters` calls each, each region between two events on `stream`"""
    for _ in range(warmup):
        fn()
    stream.synchronize()
    ms = []
    for _ in range(regions):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        for _ in range(iters):
            fn()
        b.record(stream)
        b.synchronize()
        ms.append(a.elapsed_time(b) / iters)
    return statistics.median(ms), min(ms), max(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=2000)
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--regions", type=int, default=5)
    ap.add_argument("--decodes", type=int, default=7)
    ap.add_argument("--width", type=int, default=7680)
    ap.add_argument("--height", type=int, default=4320)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "orient_probe.json"))
    args = ap.parse_args()
    import numpy as np
    import torch
    import j40_amd
    L = j40_amd.lib()
    W, H = args.width, args.height
    stream = torch.cuda.current_stream(0)
    hip = C.CDLL("libamdhip64.so")     # (the runtime torch and the library have loaded)
    hip.hipMemcpyAsync.restype = C.c_int
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    kernel_rows = []
    for fmt, pb in ((j40_amd.J40_U8X4, 4), (j40_amd.J40_U16X4, 8)):
        nbytes = W * H * pb
        # `pairs` source / destination pairs, together several times the 256 MiB Infinity Cache. "resident": every call on pair 0, the
        # working set (2 x nbytes) largely cache-resident from one call to the next; "rotating": call k on pair k % pairs, so that what
        # a call reads and writes was last touched pairs - 1 calls and more than a gigabyte of traffic ago: HBM rates
        pairs = args.pairs
        srcs = [torch.randint(0, 256, (nbytes,), dtype=torch.uint8, device="cuda:0") for _ in range(pairs)]
        dsts = [torch.empty(nbytes, dtype=torch.uint8, device="cuda:0") for _ in range(pairs)]
        row = {"format": "u8x4" if pb == 4 else "u16x4", "bytes": nbytes, "pairs": pairs, "footprint_bytes": 2 * nbytes * pairs}
        for how in ("resident", "rotating"):
            turn_k = [0]

            def pick():
                k = turn_k[0] % pairs if how == "rotating" else 0
                turn_k[0] += 1
                return srcs[k].data_ptr(), dsts[k].data_ptr()

            def copy():
                s_, d_ = pick()
                assert hip.hipMemcpyAsync(d_, s_, nbytes, 3, stream.cuda_stream) == 0   # 3: hipMemcpyDeviceToDevice, on the same stream

            copy_ms, copy_lo, copy_hi = timed_regions(torch, stream, copy, args.iters, args.regions)
            part = {"copy_ms": round(copy_ms, 4), "copy_ms_min_max": [round(copy_lo, 4), round(copy_hi, 4)],
                    "copy_gb_per_s_read_plus_write": round(2 * nbytes / copy_ms / 1e6, 1), "orientations": []}
            for o in range(2, 9):
                ow = H if o >= 5 else W

                def turn():
                    s_, d_ = pick()
                    assert L.j40hip_kat_device_orient(d_, ow * pb, s_, W * pb, W, H, o, fmt, stream.cuda_stream) == 0

                ms, lo, hi = timed_regions(torch, stream, turn, args.iters, args.regions)
                part["orientations"].append({"orientation": o, "ms": round(ms, 4), "ms_min_max": [round(lo, 4), round(hi, 4)],
                                             "gb_per_s_read_plus_write": round(2 * nbytes / ms / 1e6, 1), "fraction_of_copy_rate": round(copy_ms / ms, 3)})
            row[how] = part
        kernel_rows.append(row)
        print(json.dumps(row), flush=True)
        del srcs, dsts
        torch.cuda.empty_cache()

    # one 8K frame, oriented against stored order, on one handle: wall time of j40hip_frame_decode_to_host into pinned memory
    import bench
    from streams import synth
    bargs = bench.parser().parse_args([])
    mode, w, h, seed, opts = bench.stream_specs(bargs)[0]
    data = synth(mode, w, h, seed, orientation=6, **opts)
    fr = j40_amd.Frame(data)
    fr.upload(0)
    out = torch.empty(w * h * 4, dtype=torch.uint8, pin_memory=True)
    decode = {"width": w, "height": h, "orientation": 6, "decodes": args.decodes}
    pixels = {}
    for tag, mode_, stride in (("stored_order", 0, w * 4), ("oriented", 1, h * 4)):
        assert fr.set_orientation(mode_) == ""
        times = []
        for k in range(args.decodes + 2):
            t0 = time.perf_counter()
            code = L.j40hip_frame_decode_to_host(fr.h, out.data_ptr(), stride)
            t1 = time.perf_counter()
            assert code == 0, j40_amd.err4(code)
            if k >= 2:
                times.append((t1 - t0) * 1e3)
        decode[tag + "_ms"] = round(statistics.median(times), 3)
        decode[tag + "_ms_min_max"] = [round(min(times), 3), round(max(times), 3)]
        decode[tag + "_went_through_k_orient"] = fr.orientation()["went_through_k_orient"]
        pixels[tag] = out.numpy().copy()
    q = fr.orientation()
    decode["staging_bytes"] = q["staging_bytes"]
    decode["difference_ms"] = round(decode["oriented_ms"] - decode["stored_order_ms"], 3)
    decode["pixels_equal_rot90"] = bool(np.array_equal(pixels["oriented"].reshape(w, h, 4), np.rot90(pixels["stored_order"].reshape(h, w, 4), -1)))
    fr.close()
    print(json.dumps(decode), flush=True)
    result = {"width": W, "height": H, "iters_per_region": args.iters, "regions": args.regions, "unit": "milliseconds per call, median of the regions",
              "k_orient_alone": kernel_rows, "decode_to_host_8k": decode}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fp:
        json.dump(result, fp, indent=1)
        fp.write("\n")
    j40_amd.shutdown()


if __name__ == "__main__":
    main()
