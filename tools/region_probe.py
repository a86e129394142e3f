"""What a region decode costs on the forward-encoded 8K stream bench.py uses (synth("vardct", 7680, 4320, 3, forward=1)), uploaded once:

  - the warm median of Frame.decode_to_host for the whole frame and for central 256 x 256, 1024 x 1024 and 2048 x 2048 regions and a
    full-width band of 256 rows, the whole decode and the regions alternated in one process on one handle (the whole decode is the
    only way to a rectangle without j40hip_frame_set_region);
  - the device time of each (j40hip_frame_decode_timed into device memory: entropy decode, pixel kernels + crop);
  - the one-off cost of the group-major varblock index, built at the first region decode of an upload: the first region decode of
    a fresh upload against the warm one of the same region;
  - what each region took: sections launched, varblocks through the pixel kernels, bytes of the longest section inside its cover.

Prints one JSON line and writes it to profiles/region_probe.json. usage: python tools/region_probe.py [--reps 9] [--out PATH]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "region_probe.json"))
    args = ap.parse_args()
    import numpy as np
    import torch
    import j40_amd
    from streams import synth
    W, H = 7680, 4320
    data = synth("vardct", W, H, 3, forward=1)
    fr = j40_amd.Frame(data)
    sizes = fr.section_sizes()
    shift, gcols = fr.info["group_size_shift"], (W + 255) >> 8
    rects = {"whole": None, "central_256": ((W - 256) // 2, (H - 256) // 2, 256, 256), "central_1024": ((W - 1024) // 2, (H - 1024) // 2, 1024, 1024),
             "central_2048": ((W - 2048) // 2, (H - 2048) // 2, 2048, 2048), "band_256_rows": (0, (H - 256) // 2, W, 256)}

    def select(rect):
        assert (fr.clear_region() if rect is None else fr.set_region(*rect)) == ""

    # the index build: the first region decode of a fresh upload against the second
    fr.upload(0)
    select(rects["central_1024"])
    t0 = time.perf_counter(); err, _ = fr.decode_to_host(); first = (time.perf_counter() - t0) * 1e3
    assert err == ""
    t0 = time.perf_counter(); err, _ = fr.decode_to_host(); second = (time.perf_counter() - t0) * 1e3
    out = {"stream": "vardct 7680x4320 seed 3 forward=1", "codestream_bytes": len(data), "sections": int(len(sizes)), "longest_section_bytes": int(sizes.max()),
           "first_region_decode_of_an_upload_ms": round(first, 3), "second_ms": round(second, 3), "index_build_one_off_ms": round(first - second, 3), "reps": args.reps, "regions": {}}

    # host to host, alternated: one round decodes the whole frame and every region once
    host = {k: [] for k in rects}
    for rep in range(args.reps + 1):
        for name, rect in rects.items():
            select(rect)
            t0 = time.perf_counter()
            err, px = fr.decode_to_host()
            dt = (time.perf_counter() - t0) * 1e3
            assert err == ""
            if rep:
                host[name].append(dt)
    # device time, alternated the same way
    dev = {k: [] for k in rects}
    stream = torch.cuda.current_stream()
    bufs = {k: torch.empty(((r[3] if r else H), (r[2] if r else W), 4), dtype=torch.uint8, device="cuda:0") for k, r in rects.items()}
    for rep in range(args.reps + 1):
        for name, rect in rects.items():
            select(rect)
            ms = fr.decode_timed(bufs[name].data_ptr(), bufs[name].shape[1] * 4, stream.cuda_stream)
            assert fr.status() == ""
            if rep:
                dev[name].append([float(v) for v in ms])
    for name, rect in rects.items():
        select(rect)
        r = fr.region()
        cover = [(r["gy0"] + j) * gcols + r["gx0"] + i for j in range(r["grows"]) for i in range(r["gcols"])]
        d = np.median(np.array(dev[name]), axis=0)
        out["regions"][name] = {
            "rect": rect, "output_mb": round((rect[2] * rect[3] if rect else W * H) * 4 / 1e6, 2),
            "decode_to_host_ms_median": round(float(np.median(host[name])), 3), "decode_to_host_ms_min": round(min(host[name]), 3),
            "device_ms_median": {"entropy": round(float(d[0]), 3), "pixels_and_crop": round(float(d[1]), 3), "clear": round(float(d[2]), 3), "sum": round(float(d.sum()), 3)},
            "cover_groups": len(cover), "sections_launched": r["sections"] if rect else int(len(sizes)), "varblocks": r["varblocks"] if rect else None,
            "longest_section_in_cover_bytes": int(sizes[cover].max()),
        }
    whole = out["regions"]["whole"]["decode_to_host_ms_median"]
    for name in rects:
        out["regions"][name]["share_of_whole_decode_to_host"] = round(out["regions"][name]["decode_to_host_ms_median"] / whole, 4)
    fr.close()
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fp:
        fp.write(line + "\n")


if __name__ == "__main__":
    main()
