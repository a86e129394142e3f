#!/usr/bin/env python3
"""What k_patch_blend costs. One process, the three float planes of a 4096 x 4096 frame resident on the device, and
three kernels launched `--launches` times each, one after the other (j40hip_kat_device_patches, j40hip_kat_device_modular_xyb_launch):

    k_patch_blend, glyphs       4096 placements of 16 x 24 samples on a 64 x 64 grid, Replace and Add in turn, from a 512 x 384 slot
    k_patch_blend, whole frame  one Replace of all 4096 x 4096 samples from a slot of the frame's size
    k_xyb_to_rgba               the sRGB tail over the same planes, u8: the pass the patches sit in front of

The times are the kernels' own, read from a kernel trace of this run:

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/patch_probe.py
    python tools/patch_probe.py --summarise OUT [--out profiles/patch_probe.json]

--summarise groups the trace's dispatches by kernel name and grid size (the two k_patch_blend cases differ in their grids) and prints
the median, minimum and maximum of each group after dropping its first `--warmup` dispatches."""
import argparse
import csv
import ctypes as C
import glob
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

U8X4 = 0x0F33
M = [[11.031566901960783, -9.866943921568629, -0.16462299647058826], [-3.254147380392157, 4.418770392156863, -0.16462299647058826],
     [-3.6588512862745097, 2.7129230470588235, 1.9459282392156863]]
BIAS = [-0.0037930732552754493] * 3


def summarise(trace_dir, warmup, out):
    files = glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True)
    assert files, "no *kernel_trace.csv under %s (the trace has to be written as CSV: --output-format csv)" % trace_dir
    groups = {}
    for path in files:
        with open(path, newline="") as fp:
            for row in csv.DictReader(fp):
                name = row["Kernel_Name"].split("(")[0]
                if "k_patch_blend" not in name and "k_xyb_to_rgba" not in name:
                    continue
                name = "k_patch_blend" if "k_patch_blend" in name else "k_xyb_to_rgba"
                grid = int(row["Grid_Size_X"]) // max(1, int(row["Workgroup_Size_X"])) if "Grid_Size_X" in row else 0
                groups.setdefault((name, grid), []).append((int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3)
    rows = {}
    for (name, grid), us in sorted(groups.items()):
        kept = us[warmup:] if len(us) > warmup else us
        rows["%s_grid_%d" % (name, grid)] = {"dispatches": len(us), "median_us": statistics.median(kept), "min_us": min(kept), "max_us": max(kept)}
        print("%-16s %6d workgroups along x: %3d dispatches, median %.1f us (min %.1f, max %.1f)" % (name, grid, len(us), statistics.median(kept), min(kept), max(kept)))
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as fp:
            json.dump({"what": "kernel times from rocprofv3 --kernel-trace over tools/patch_probe.py, per kernel and grid, the first %d dispatches of each dropped" % warmup, "kernels": rows}, fp, indent=1)
            fp.write("\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--launches", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--summarise", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.summarise:
        return summarise(args.summarise, args.warmup, args.out)
    import numpy as np
    import torch
    import j40_amd
    assert j40_amd.device_count() > 0, "the probe measures on the GPU"
    L = j40_amd.lib()
    n = args.size
    dev = "cuda:0"
    g = torch.Generator(device=dev)
    g.manual_seed(5)
    planes = torch.rand((3, n, n), generator=g, device=dev) * 0.6 + 0.1
    atlas = torch.rand((3, 384, 512), generator=g, device=dev) * 0.1
    whole = torch.rand((3, n, n), generator=g, device=dev) * 0.6 + 0.1
    out = torch.empty((n, n * 4), dtype=torch.uint8, device=dev)
    step = n // 64
    glyphs = np.array([(gx * step + (gy * 7) % (step - 16), gy * step + (gx * 5) % (step - 24), 16, 24, (gx * 16) % 496, (gy * 24) % 360, 0, 1 + (gx + gy) % 2, 0)
                       for gy in range(64) for gx in range(64)], np.int32)
    frame = np.array([(0, 0, n, n, 0, 0, 1, 1, 0)], np.int32)
    slots = (C.c_void_p * 4)(atlas.data_ptr(), whole.data_ptr(), None, None)
    sw = np.array([512, n, 0, 0], np.int32); sh = np.array([384, n, 0, 0], np.int32)
    tiles = C.c_int32(0)
    torch.cuda.synchronize()
    for name, pl in (("glyphs", glyphs), ("whole frame", frame)):
        for _ in range(args.launches):
            code = L.j40hip_kat_device_patches(planes.data_ptr(), n, n, slots, sw.ctypes.data, sh.ctypes.data, pl.ctypes.data, len(pl), C.byref(tiles), None)
            assert code == 0, j40_amd.err4(code)
        print("k_patch_blend, %s: %d placements, %d workgroups" % (name, len(pl), tiles.value))
    frame_dev = torch.zeros(4096, dtype=torch.uint8, device=dev)
    cc = np.array(sum(M, []) + BIAS + [255.0, 0, 0], np.float32)
    assert L.j40hip_kat_device_colour_frame(cc.ctypes.data, 8, frame_dev.data_ptr(), 4096) <= 4096
    ptrs = (C.c_void_p * 3)(*[planes[k].data_ptr() for k in range(3)])
    mm = np.zeros(3, np.float32)
    torch.cuda.synchronize()
    for _ in range(args.launches):
        code = L.j40hip_kat_device_modular_xyb_launch(2, ptrs, 4, n, n, mm.ctypes.data, cc.ctypes.data, 8, U8X4, out.data_ptr(), n * 4, frame_dev.data_ptr(), None)
        assert code == 0, j40_amd.err4(code)
    torch.cuda.synchronize()
    j40_amd.shutdown()


if __name__ == "__main__":
    main()
