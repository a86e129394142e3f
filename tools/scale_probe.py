#!/usr/bin/env python3
"""What the reduced-size decode gives ("Reduced-size decode"): the pipeline over bench.py's 8K streams at scale
shifts 0, 1 and 2, to pinned host memory and with the pixels left in device memory, 256 frames per step, in SOURCE Mpixel/s (the
frames' own size: what a caller who wants small pictures of large frames gets through per second). The shift-0 rows are the control
against bench.py's own `value` and `device_output`. Per row also the pipeline's stage times per launch (HIP events on the batches'
streams: LfGroup streams + plan, entropy, pixels), and -- `pixel_stage_alone` -- the pixel stage of one batch in flight with nothing
beside it, shift 1 and 2 against shift 0 (the stores fall to a quarter and a sixteenth).

    python tools/scale_probe.py [--steps 6] [--warmup 2] [--batch 256] [--out profiles/scale_probe.json]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def run_steps(pipe, bufs, sizes, outs, strides, device_output, steps, torch):
    torch.cuda.synchronize()
    pipe.reset_stats()
    t0 = time.perf_counter()
    tickets = []
    for _ in range(steps):
        tickets = [pipe.submit_raw(bufs[i], sizes[i], outs[i].data_ptr(), strides, device_output) for i in range(len(bufs))]
    pipe.drain()
    torch.cuda.synchronize()
    elapsed = time.perf_counter() - t0
    assert all(pipe.result(t) == "" for t in tickets)
    return elapsed


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=6)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scale_probe.json"))
    args = ap.parse_args()
    import torch
    import bench
    import j40_amd
    bargs = bench.parser().parse_args([])
    W, H, B = bargs.width, bargs.height, args.batch
    specs = bench.stream_specs(bargs)
    datas = bench.synth_many(specs, bench.cpu_quota())
    D = len(datas)
    bufs = [C.create_string_buffer(d, len(d)) for d in datas]
    step_bufs = [bufs[i % D] for i in range(B)]
    step_sizes = [len(datas[i % D]) for i in range(B)]
    threads = max(2, min(4, bench.cpu_quota()))
    rows, alone = [], []
    for shift in (0, 1, 2):
        s = 1 << shift
        ow, oh = (W + s - 1) >> shift, (H + s - 1) >> shift
        for device_output in (False, True):
            n = min(D, B, 64) if not device_output else min(B, 256)
            if device_output:
                outs = [torch.empty((oh, ow, 4), dtype=torch.uint8, device="cuda:0") for _ in range(n)]
            else:
                outs = [torch.empty((oh, ow, 4), dtype=torch.uint8, pin_memory=True) for _ in range(n)]
            step_outs = [outs[i % n] for i in range(B)]
            pipe = j40_amd.Pipeline(0, threads, B, bargs.in_flight, lf_streams="device")
            assert pipe.set_scale(shift) == ""
            run_steps(pipe, step_bufs, step_sizes, step_outs, ow * 4, device_output, args.warmup, torch)
            el = run_steps(pipe, step_bufs, step_sizes, step_outs, ow * 4, device_output, args.steps, torch)
            st = pipe.stats()
            pipe.close()
            launches = max(st["launches"], 1)
            rows.append({"shift": shift, "output": "device" if device_output else "host", "out_width": ow, "out_height": oh,
                         "source_mpixels_per_s": round(W * H * B * args.steps / el / 1e6, 2), "ms_per_step": round(el / args.steps * 1e3, 3),
                         "bytes_out_per_step": ow * oh * 4 * B, "frames_per_launch": round(st["launch_frames"] / launches, 1),
                         "lf_plan_ms_per_launch": round(st["lf_plan_ms"] / launches, 3), "entropy_ms_per_launch": round(st["k1_ms"] / launches, 3),
                         "pixels_ms_per_launch": round(st["k2_ms"] / launches, 3), "single_frames": st["single_frames"]})
            print(json.dumps(rows[-1]), flush=True)
            del outs, step_outs
            torch.cuda.empty_cache()
        # the pixel stage with the device to itself: one batch in flight, pixels left in HBM
        outs = [torch.empty((oh, ow, 4), dtype=torch.uint8, device="cuda:0") for _ in range(min(B, 256))]
        step_outs = [outs[i % len(outs)] for i in range(B)]
        pipe = j40_amd.Pipeline(0, threads, B, 1, lf_streams="device")
        assert pipe.set_scale(shift) == ""
        run_steps(pipe, step_bufs, step_sizes, step_outs, ow * 4, True, 2, torch)
        run_steps(pipe, step_bufs, step_sizes, step_outs, ow * 4, True, max(3, args.steps // 2), torch)
        st = pipe.stats()
        pipe.close()
        alone.append({"shift": shift, "pixels_ms_per_launch": round(st["k2_ms"] / max(st["launches"], 1), 3), "entropy_ms_per_launch": round(st["k1_ms"] / max(st["launches"], 1), 3),
                      "frames_per_launch": round(st["launch_frames"] / max(st["launches"], 1), 1)})
        print(json.dumps(alone[-1]), flush=True)
        del outs, step_outs
        torch.cuda.empty_cache()
    base = alone[0]["pixels_ms_per_launch"]
    for a in alone:
        a["ratio_to_shift_0"] = round(a["pixels_ms_per_launch"] / base, 3) if base > 0 else None
    result = {"width": W, "height": H, "frames_per_step": B, "steps": args.steps, "warmup": args.warmup, "distinct_streams": D, "host_threads": threads,
              "in_flight": bargs.in_flight, "unit": "source Mpixels/s (the frames' own size over the wall time)", "rows": rows, "pixel_stage_alone": alone}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fp:
        json.dump(result, fp, indent=1)
        fp.write("\n")
    print(json.dumps(result))
    j40_amd.shutdown()


if __name__ == "__main__":
    main()
