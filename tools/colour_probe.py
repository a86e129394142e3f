#!/usr/bin/env python3
"""What the colour mode costs. One process, the three float planes of a 7680 x 4320 frame resident on the device,
one output image. The kernels alone (j40hip_kat_device_colour_tail, j40hip_kat_device_modular_xyb_launch), warm: a sample is the time
between two device events round `--launches` launches of ONE kernel, back to back on the stream, divided by their number, in rounds that
take the kernels one after the other so that whatever else the machine does falls on all of them alike:

    k_xyb_to_rgba                 u8 and u16   the yardstick: the sRGB tail on the same planes, 12 bytes in, 4 / 8 out per pixel
    k_colour_tail<curve>, 8 bit   u8 and u16   the frame's threshold table in LDS, no curve evaluated
    k_colour_tail<curve>, 10 bit  u8 and u16   the curve in float64 per sample

Per kernel: median, min, max in ms, the achieved GB/s of the bytes the algorithm needs and that as a share of the HBM peak (8 TB/s).
Then one 8K VarDCT decode on the device (pixels left in device memory) with the switch off and on, alternating, host clock round a
synchronised decode. The 8K working set (398 MB of planes, 133 / 265 MB of pixels) is of the size of the 256 MB Infinity Cache: the
GB/s are those of the bytes the algorithm needs, not of HBM alone.

    python tools/colour_probe.py [--width 7680] [--height 4320] [--rounds 15] [--warmup 3] [--launches 10] [--out profiles/colour_probe.json]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

U8X4, U16X4 = 0x0F33, 0x0F35
HBM_PEAK_GB_S = 8000.0
M = [[11.031566901960783, -9.866943921568629, -0.16462299647058826], [-3.254147380392157, 4.418770392156863, -0.16462299647058826],
     [-3.6588512862745097, 2.7129230470588235, 1.9459282392156863]]
BIAS = [-0.0037930732552754493] * 3
# name -> (white, primaries, tf, gamma, intensity_target)
CURVES = {"linear": (1, 1, 8, 0, 255), "srgb_p3": (1, 11, 13, 0, 255), "bt709": (1, 1, 1, 0, 255), "dci": (11, 11, 17, 0, 255), "gamma": (1, 1, 0, 4545455, 255),
          "pq": (1, 9, 16, 0, 4000), "hlg": (1, 9, 18, 0, 1000)}


WHITE_XY = {1: (312700, 329000), 10: (333333, 333333), 11: (314000, 351000)}
PRIM_XY = {1: (640000, 330000, 300000, 600000, 150000, 60000), 9: (708000, 292000, 170000, 797000, 131000, 46000), 11: (680000, 320000, 265000, 690000, 150000, 60000)}


def enc_words(np, white, primaries, tf, gamma):
    """the 16 words of j40hip_frame_colour_encoding for an RGB encoding of enums"""
    return np.array([0, white, *WHITE_XY[white], primaries, *PRIM_XY[primaries], 1 if gamma else 0, gamma, tf, 1, 0], np.int32)


def synth_8k(w, h):
    """the 8K stream of the decode timing, PQ / BT.2100 signalled, by the stream writer (build/jxlsynth)"""
    path = os.path.join(ROOT, "build", "streams", "colour_probe_%d_%d.jxl" % (w, h))
    if not os.path.exists(path):
        os.makedirs(os.path.dirname(path), exist_ok=True)
        subprocess.run([os.path.join(ROOT, "build", "jxlsynth"), "vardct", str(w), str(h), "3", path, "forward=1", "primaries=9", "tf=16", "tone=4000,0.5"], check=True, stderr=subprocess.DEVNULL)
    with open(path, "rb") as fp:
        return fp.read()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=7680)
    ap.add_argument("--height", type=int, default=4320)
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--launches", type=int, default=10, help="launches of one kernel between the two events of a sample")
    ap.add_argument("--decodes", type=int, default=15, help="whole decodes per setting of the switch")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "colour_probe.json"))
    args = ap.parse_args()
    import numpy as np
    import torch
    import j40_amd
    assert j40_amd.device_count() > 0, "the probe measures on the GPU"
    L = j40_amd.lib()
    w, h = args.width, args.height
    px = w * h
    dev = "cuda:0"
    g = torch.Generator(device=dev)
    g.manual_seed(5)
    # XYB samples of the size a picture's are: X in [-0.03, 0.03], Y and B in [0.16, 0.85]
    xyb = torch.empty((3, h, w), dtype=torch.float32, device=dev)
    xyb[0] = (torch.rand((h, w), generator=g, device=dev) - 0.5) * 0.06
    xyb[1] = torch.rand((h, w), generator=g, device=dev) * 0.69 + 0.16
    xyb[2] = torch.rand((h, w), generator=g, device=dev) * 0.69 + 0.16
    out = torch.empty((h, w, 8), dtype=torch.uint8, device=dev)
    stream = torch.cuda.current_stream(0)
    frame_dev = torch.zeros(4096, dtype=torch.uint8, device=dev)
    cc_srgb = np.array(sum(M, []) + BIAS + [255.0, 0, 0], np.float32)
    assert L.j40hip_kat_device_colour_frame(cc_srgb.ctypes.data, 8, frame_dev.data_ptr(), 4096) <= 4096
    p_flt = (C.c_void_p * 3)(*[xyb[k].data_ptr() for k in range(3)])
    mm = np.zeros(3, np.float32)
    keep = []   # (what the launches read from host memory lives as long as they do)

    def yardstick(fmt):
        def launch():
            code = L.j40hip_kat_device_modular_xyb_launch(2, p_flt, 2, w, h, mm.ctypes.data, cc_srgb.ctypes.data, 8, fmt, out.data_ptr(), w * (8 if fmt == U16X4 else 4), frame_dev.data_ptr(), stream.cuda_stream)
            assert code == 0, j40_amd.err4(code)
        return launch

    def tail(curve, bpp, fmt):
        white, prim, tf, gamma, it = CURVES[curve]
        enc = enc_words(np, white, prim, tf or 13, gamma)
        code, P, lum = j40_amd.colour_gamut_matrix(enc)
        assert code == ""
        cc = np.concatenate([(P @ np.array(M, np.float32).astype(np.float64)).astype(np.float32).reshape(9), BIAS, [it, 0, 0]]).astype(np.float32)
        lm = lum.astype(np.float32)
        table, rng = None, np.zeros(2, np.int32)
        if bpp == 8:
            code, t, r = j40_amd.colour_table(enc, it)
            assert code == "", curve
            table = torch.from_numpy(t).to(dev); rng = np.array(r, np.int32)
        keep.extend([enc, cc, lm, table, rng])
        def launch():
            code = L.j40hip_kat_device_colour_tail(xyb.data_ptr(), w, h, cc.ctypes.data, enc.ctypes.data, lm.ctypes.data, bpp, table.data_ptr() if table is not None else None, rng.ctypes.data,
                                                   fmt, out.data_ptr(), w * (8 if fmt == U16X4 else 4), stream.cuda_stream)
            assert code == 0, j40_amd.err4(code)
        return launch

    series = []   # (name, launch, bytes per pixel the algorithm needs)
    for tag, fmt, pb in (("u8", U8X4, 4), ("u16", U16X4, 8)):
        series.append(("k_xyb_to_rgba_" + tag, yardstick(fmt), 12 + pb))
        for curve in CURVES:
            for bpp in (8, 10):
                series.append(("k_colour_tail_%s_bpp%d_%s" % (curve, bpp, tag), tail(curve, bpp, fmt), 12 + pb))
        series.append(("k_xyb_to_rgba_%s_repeat" % tag, yardstick(fmt), 12 + pb))
    times = {name: [] for name, _, _ in series}
    for r in range(args.warmup + args.rounds):
        for name, launch, _ in series:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(stream)
            for _ in range(args.launches):
                launch()
            b.record(stream)
            b.synchronize()
            if r >= args.warmup:
                times[name].append(a.elapsed_time(b) / args.launches)
    rows = {}
    for name, _, moved in series:
        t = sorted(times[name])
        med = statistics.median(t)
        gbs = px * moved / (med * 1e-3) / 1e9
        rows[name] = {"median_ms": med, "min_ms": t[0], "max_ms": t[-1], "bytes_per_pixel": moved, "achieved_GB_per_s": gbs, "share_of_hbm_peak": gbs / HBM_PEAK_GB_S}
        print("%-36s median %.4f ms  (min %.4f, max %.4f)  %6.0f GB/s of %d B/pixel = %.2f of the HBM peak" % (name, med, t[0], t[-1], gbs, moved, gbs / HBM_PEAK_GB_S))
    for tag in ("u8", "u16"):
        y = min(rows["k_xyb_to_rgba_" + tag]["median_ms"], rows["k_xyb_to_rgba_%s_repeat" % tag]["median_ms"])
        for name in rows:
            if name.startswith("k_colour_tail") and name.endswith("_" + tag):
                rows[name]["over_k_xyb_to_rgba"] = rows[name]["median_ms"] / y
    del xyb
    torch.cuda.empty_cache()
    # one 8K decode on the device with the switch off and on: the same coefficients, PQ / BT.2100 signalled
    data = synth_8k(w, h)
    decode = {}
    for bpp_tag, fmt, pb in (("u8", U8X4, 4), ("u16", U16X4, 8)):
        img = torch.empty((h, w * pb), dtype=torch.uint8, device=dev)
        frames = {}
        for mode in (0, 1):
            fr = j40_amd.Frame(data)
            assert fr.set_colour(mode) == ""
            fr.set_output_format(fmt); fr.upload(0)
            frames[mode] = fr
        ms = {0: [], 1: []}
        for r in range(args.warmup + args.decodes):
            for mode in (0, 1):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                frames[mode].decode(img.data_ptr(), w * pb, stream.cuda_stream)
                torch.cuda.synchronize()
                if r >= args.warmup:
                    ms[mode].append((time.perf_counter() - t0) * 1e3)
        assert frames[1].colour()["used"] and not frames[0].colour()["used"] and frames[0].status() == "" and frames[1].status() == ""
        for fr in frames.values():
            fr.close()
        decode[bpp_tag] = {"switch_off_median_ms": statistics.median(ms[0]), "switch_on_median_ms": statistics.median(ms[1]), "switch_off_min_ms": min(ms[0]), "switch_on_min_ms": min(ms[1]),
                           "extra_ms": statistics.median(ms[1]) - statistics.median(ms[0])}
        print("8K decode, %s: switch off %.3f ms, on %.3f ms (medians of %d, alternating)" % (bpp_tag, decode[bpp_tag]["switch_off_median_ms"], decode[bpp_tag]["switch_on_median_ms"], args.decodes))
    result = {"what": "kernels: ms per launch, %d launches of one kernel between two device events, %d rounds after %d warm-up rounds, the kernels taken in turn within a round; decodes: host clock round one synchronised device decode of an 8-bit 8K VarDCT frame (PQ, BT.2100 signalled), the switch off and on in turn" % (args.launches, args.rounds, args.warmup),
              "device": torch.cuda.get_device_name(0), "size": [w, h], "hbm_peak_GB_per_s": HBM_PEAK_GB_S, "kernels": rows, "decode_8k": decode}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fp:
        json.dump(result, fp, indent=1)
        fp.write("\n")
    j40_amd.shutdown()
    print(json.dumps({"colour_probe": args.out}))


if __name__ == "__main__":
    main()
