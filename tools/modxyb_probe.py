#!/usr/bin/env python3
"""What the Modular XYB colour tail costs ("Modular frames of XYB images"). One process, the planes of a
7680 x 4320 frame resident on the device: three int16 planes of XYB integers, the three float planes k_modular_to_xyb makes of them, one
output image. Timed alone (j40hip_kat_device_modular_xyb_launch), warm: a sample is the time between two device events round `--launches`
launches of ONE kernel, back to back on the stream, divided by their number -- a window of milliseconds, so that the events' own cost
does not decide a comparison of kernels that take a tenth of one --, in rounds that take the kernels one after the other so that whatever
else the machine does falls on all of them alike:

    k_modular_xyb_pack  u8 and u16     the fused kernel: 6 bytes in, 4 / 8 out per pixel
    k_pack_planes       u8 and u16     the same planes rendered as R, G, B (the switch off): the same traffic, no colour tail
    k_xyb_to_rgba       u8 and u16     the VarDCT colour tail's kernel on the float planes: 12 bytes in, 4 / 8 out -- twice per round, so that
                                       the spread between repeats of one kernel is measured beside the differences between kernels

The yardstick is k_xyb_to_rgba: the fused kernel moves fewer bytes and should take no longer than it, beyond that spread.
Per kernel: median, min, max in ms and the achieved GB/s of the bytes the algorithm needs at the median.

The 8K working set (199 MB of integer planes, 398 MB of float planes, 133 / 265 MB of pixels) is of the size of the 256 MB Infinity Cache:
part of every kernel's traffic is served from it, so the GB/s are those of the bytes the algorithm needs, not of HBM alone.

    python tools/modxyb_probe.py [--width 7680] [--height 4320] [--rounds 25] [--warmup 3] [--launches 20] [--out profiles/modxyb_probe.json]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

U8X4, U16X4 = 0x0F33, 0x0F35
CC = [11.031566901960783, -9.866943921568629, -0.16462299647058826, -3.254147380392157, 4.418770392156863, -0.16462299647058826,
      -3.6588512862745097, 2.7129230470588235, 1.9459282392156863, -0.0037930732552754493, -0.0037930732552754493, -0.0037930732552754493, 255.0, 0.0, 0.0]
M = [1.0 / 4096, 1.0 / 512, 1.0 / 256]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=7680)
    ap.add_argument("--height", type=int, default=4320)
    ap.add_argument("--rounds", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--launches", type=int, default=20, help="launches of one kernel between the two events of a sample")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "modxyb_probe.json"))
    args = ap.parse_args()
    import numpy as np
    import torch
    import j40_amd
    assert j40_amd.device_count() > 0, "the probe measures on the GPU"
    L = j40_amd.lib()
    w, h = args.width, args.height
    dev = "cuda:0"
    g = torch.Generator(device=dev)
    g.manual_seed(5)
    # integers of the size a picture's are: Y in [0, 0.85], X in [-0.03, 0.03], B - Y in [-0.6, 0.2]
    c0 = torch.randint(0, 436, (h, w), generator=g, device=dev, dtype=torch.int32)
    c1 = torch.randint(-120, 121, (h, w), generator=g, device=dev, dtype=torch.int32)
    c2 = torch.randint(-300, 100, (h, w), generator=g, device=dev, dtype=torch.int32)
    planes = [t.to(torch.int16).contiguous() for t in (c0, c1, c2)]
    xyb = torch.empty((3, h, w), dtype=torch.float32, device=dev)
    xyb[0] = c1.float() * M[0]; xyb[1] = c0.float() * M[1]; xyb[2] = (c2 + c0).float() * M[2]
    del c0, c1, c2
    out = torch.empty((h, w, 8), dtype=torch.uint8, device=dev)
    frame_dev = torch.zeros(4096, dtype=torch.uint8, device=dev)
    cc, mm = np.array(CC, np.float32), np.array(M, np.float32)
    assert L.j40hip_kat_device_colour_frame(cc.ctypes.data, 8, frame_dev.data_ptr(), 4096) <= 4096
    p_int = (C.c_void_p * 3)(*[p.data_ptr() for p in planes])
    p_flt = (C.c_void_p * 3)(*[xyb[k].data_ptr() for k in range(3)])
    stream = torch.cuda.current_stream(0)
    px = w * h

    def launch(kernel, fmt):
        code = L.j40hip_kat_device_modular_xyb_launch(kernel, p_flt if kernel == 2 else p_int, 2, w, h, mm.ctypes.data, cc.ctypes.data, 8, fmt, out.data_ptr(),
                                                      w * (8 if fmt == U16X4 else 4), frame_dev.data_ptr(), stream.cuda_stream)
        assert code == 0, j40_amd.err4(code)

    # (name, kernel, format, bytes per pixel the algorithm needs)
    series = [("k_modular_xyb_pack_u8", 0, U8X4, 6 + 4), ("k_pack_planes_u8", 1, U8X4, 6 + 4), ("k_xyb_to_rgba_u8", 2, U8X4, 12 + 4), ("k_xyb_to_rgba_u8_repeat", 2, U8X4, 12 + 4),
              ("k_modular_xyb_pack_u16", 0, U16X4, 6 + 8), ("k_pack_planes_u16", 1, U16X4, 6 + 8), ("k_xyb_to_rgba_u16", 2, U16X4, 12 + 8), ("k_xyb_to_rgba_u16_repeat", 2, U16X4, 12 + 8)]
    # the fused kernel's pixels are the yardstick's on these planes: what is timed computes the same thing
    same = True
    for fmt, pb in ((U8X4, 4), (U16X4, 8)):   # (the image's first w * h * pb bytes: the launches write rows of w * pb bytes)
        flat = out.view(-1)[:px * pb]
        launch(0, fmt); torch.cuda.synchronize(); fused = flat.clone()
        flat.zero_()
        launch(2, fmt); torch.cuda.synchronize()
        same = same and bool(torch.equal(fused, flat))
        del fused
    if not same:
        sys.exit("k_modular_xyb_pack and k_xyb_to_rgba disagree on the same planes: nothing worth timing")
    print("k_modular_xyb_pack and k_xyb_to_rgba on the same planes: the same pixels, every byte, both formats")
    times = {name: [] for name, _, _, _ in series}
    for r in range(args.warmup + args.rounds):
        for name, kernel, fmt, _ in series:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(stream)
            for _ in range(args.launches):
                launch(kernel, fmt)
            b.record(stream)
            b.synchronize()
            if r >= args.warmup:
                times[name].append(a.elapsed_time(b) / args.launches)
    rows = {}
    for name, _, _, bpp_moved in series:
        t = sorted(times[name])
        med = statistics.median(t)
        rows[name] = {"median_ms": med, "min_ms": t[0], "max_ms": t[-1], "bytes_per_pixel": bpp_moved, "achieved_GB_per_s": px * bpp_moved / (med * 1e-3) / 1e9}
        print("%-28s median %.4f ms  (min %.4f, max %.4f)  %6.0f GB/s of %d B/pixel" % (name, med, t[0], t[-1], rows[name]["achieved_GB_per_s"], bpp_moved))
    verdict = {}
    for tag in ("u8", "u16"):
        y, yr, f = rows["k_xyb_to_rgba_" + tag]["median_ms"], rows["k_xyb_to_rgba_%s_repeat" % tag]["median_ms"], rows["k_modular_xyb_pack_" + tag]["median_ms"]
        verdict[tag] = {"fused_over_yardstick": f / min(y, yr), "yardstick_repeat_spread": abs(y - yr) / min(y, yr), "fused_no_slower": f <= max(y, yr)}
        print("%s: fused / k_xyb_to_rgba = %.3f, spread between the two series of k_xyb_to_rgba %.3f" % (tag, verdict[tag]["fused_over_yardstick"], verdict[tag]["yardstick_repeat_spread"]))
    result = {"what": "ms per launch: %d launches of one kernel between two device events, %d rounds after %d warm-up rounds, the kernels taken in turn within a round" % (args.launches, args.rounds, args.warmup),
              "device": torch.cuda.get_device_name(0), "size": [w, h], "fused_pixels_equal_the_yardsticks": same, "kernels": rows, "verdict": verdict}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fp:
        json.dump(result, fp, indent=1)
        fp.write("\n")
    print(json.dumps({"modxyb_probe": args.out}))


if __name__ == "__main__":
    main()
