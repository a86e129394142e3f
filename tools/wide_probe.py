#!/usr/bin/env python3
"""What the wide Modular path costs ("Wide Modular frames"). Two 4096 x 4096 pictures -- tree=1: a property tree
the wave-cooperative kernel takes; tree=2: the weighted predictor, the generic kernel -- each as three streams: the 12-bit narrow
stream, its wide=1 twin (the same sections decoded with int32 planes) and the 16-bit stream. Per stream one handle, uploaded once:
3 warm-up decodes, then 10 timed ones (j40hip_frame_decode_timed: device events around the decode on the stream); the median, the
spread, the stage times of the median run, and the wide / narrow ratios.

    python tools/wide_probe.py [--size 4096] [--decodes 10] [--warmup 3] [--out profiles/wide_probe.json]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--decodes", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "wide_probe.json"))
    args = ap.parse_args()
    import torch
    import j40_amd
    from streams import synth
    assert j40_amd.device_count() > 0, "the probe measures on the GPU"
    n = args.size
    stream = torch.cuda.current_stream(0).cuda_stream
    rows = []
    for picture, tree in (("coop", 1), ("generic_weighted_predictor", 2)):
        row = {"picture": picture, "tree": tree, "size": [n, n]}
        for name, opts in (("narrow_12", dict(bpp=12)), ("wide_12", dict(bpp=12, wide=1)), ("wide_16", dict(bpp=16, wide=1))):
            data = synth("modular", n, n, 7, tree=tree, repeat=4, **opts)   # (a 1024 x 1024 picture tiled: cheap to write, the sections are real)
            fr = j40_amd.Frame(data, wide=True)
            fr.upload(0)
            out = torch.empty((n, n, 4), dtype=torch.uint8, device="cuda:0")
            for _ in range(args.warmup):
                fr.decode_timed(out.data_ptr(), n * 4, stream)
            assert fr.status() == ""
            runs = sorted((float(sum(ms)), [float(v) for v in ms]) for ms in (fr.decode_timed(out.data_ptr(), n * 4, stream) for _ in range(args.decodes)))
            total = [t for t, _ in runs]
            coop, sections = fr.coop_sections()
            row[name] = {"bytes": len(data), "median_ms": statistics.median(total), "min_ms": total[0], "max_ms": total[-1], "stages_ms_of_median_run": runs[len(runs) // 2][1],
                         "sections": sections, "coop_sections": coop, "quad_sections": fr.quad_sections(), "split_sections": fr.split_sections(), "wide": fr.wide()}
            fr.close()
            del out
        row["wide_12_over_narrow_12"] = row["wide_12"]["median_ms"] / row["narrow_12"]["median_ms"]
        row["wide_16_over_narrow_12"] = row["wide_16"]["median_ms"] / row["narrow_12"]["median_ms"]
        rows.append(row)
        print("%s: narrow 12-bit %.3f ms, wide 12-bit %.3f ms (x %.2f), wide 16-bit %.3f ms (x %.2f)" % (
            picture, row["narrow_12"]["median_ms"], row["wide_12"]["median_ms"], row["wide_12_over_narrow_12"], row["wide_16"]["median_ms"], row["wide_16_over_narrow_12"]))
    result = {"what": "j40hip_frame_decode_timed of one uploaded Modular frame, ms: median of %d after %d warm-ups" % (args.decodes, args.warmup),
              "device": torch.cuda.get_device_name(0), "rows": rows}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fp:
        json.dump(result, fp, indent=1)
        fp.write("\n")
    print(json.dumps({"wide_probe": args.out}))


if __name__ == "__main__":
    main()
