"""What composing the frames of a sequence costs (k_frame_compose, j40hip_sequence_next), in one process, the variants alternating after a
warm-up, with a device synchronisation inside every clock:

  (a) k_frame_compose alone (j40hip_kat_device_compose) over a 7680 x 4320 canvas with a 4096 x 2048 rectangle and a source slot,
      against a device-to-device copy of the canvas, u8x4 and u16x4. The kernel moves at most the copy's 8 (u8) or 16 (u16) bytes a
      pixel, so the bar is the copy's time plus the copy's own run-to-run spread over the session; the ratio and the bytes per second
      are recorded.
  (b) the aliased form (out == src: only the rectangle is written) against a copy of the rectangle alone.
  (d) k_frame_blend alone (j40hip_kat_device_blend, colour and alpha both Blend) on (a)'s and (b)'s case, alternating with them. The
      yardstick is k_frame_compose's bytes per second in this same session; the blend's bytes count the source inside the rectangle
      too (it is read there as well). The bar: the blend's bytes per second (median) fall no further below compose's than compose's
      own min-to-max spread of bytes per second. Recorded under "blend", met or missed per format and form.
  (c) a 16-frame 1920 x 1080 VarDCT animation (frame 0 full, the others cropped): j40hip_sequence_next sixteen times against one
      j40hip_batch over its coded frames plus sixteen composes. Reported, no bar.

Prints one JSON line and writes it to profiles/frames_probe.json. usage: python tools/frames_probe.py [--reps 15] [--out PATH]"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

U8X4, U16X4 = 0x0F33, 0x0F35


def stats(ms):
    import numpy as np
    a = np.sort(np.array(ms))
    return {"median_ms": round(float(np.median(a)), 4), "min_ms": round(float(a[0]), 4), "max_ms": round(float(a[-1]), 4), "spread_ms": round(float(a[-1] - a[0]), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "frames_probe.json"))
    args = ap.parse_args()
    import torch
    import j40_amd
    from streams import SYNTH, CACHE
    L = j40_amd.lib()
    stream = torch.cuda.current_stream().cuda_stream

    def clock(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    out = {"reps": args.reps, "compose": {}, "blend": {}}
    W, H, rw, rh, x0, y0 = 7680, 4320, 4096, 2048, 1792, 1136
    for name, fmt, pb in (("u8x4", U8X4, 4), ("u16x4", U16X4, 8)):
        stride = W * pb
        canvas = torch.randint(0, 255, (H * stride,), dtype=torch.uint8, device="cuda:0")
        slot = torch.randint(0, 255, (H * stride,), dtype=torch.uint8, device="cuda:0")
        frame = torch.randint(0, 255, (rh * rw * pb,), dtype=torch.uint8, device="cuda:0")
        rect_dst = slot.view(H, stride)[y0:y0 + rh, x0 * pb:(x0 + rw) * pb]
        rect_src = frame.view(rh, rw * pb)

        def compose():
            assert L.j40hip_kat_device_compose(canvas.data_ptr(), stride, slot.data_ptr(), stride, frame.data_ptr(), rw * pb, W, H, x0, y0, rw, rh, 0, 0, fmt, stream) == 0

        def compose_aliased():
            assert L.j40hip_kat_device_compose(slot.data_ptr(), stride, slot.data_ptr(), stride, frame.data_ptr(), rw * pb, W, H, x0, y0, rw, rh, 0, 0, fmt, stream) == 0

        def blend():
            assert L.j40hip_kat_device_blend(canvas.data_ptr(), stride, slot.data_ptr(), stride, frame.data_ptr(), rw * pb, W, H, x0, y0, rw, rh, 0, 0, fmt, 2, 2, stream) == 0

        def blend_aliased():
            assert L.j40hip_kat_device_blend(slot.data_ptr(), stride, slot.data_ptr(), stride, frame.data_ptr(), rw * pb, W, H, x0, y0, rw, rh, 0, 0, fmt, 2, 2, stream) == 0

        variants = {"compose": compose, "copy_canvas": lambda: canvas.copy_(slot), "compose_aliased": compose_aliased, "copy_rectangle": lambda: rect_dst.copy_(rect_src),
                    "blend": blend, "blend_aliased": blend_aliased}
        ms = {k: [] for k in variants}
        for rep in range(args.reps + 3):
            for k, fn in variants.items():
                dt = clock(fn)
                if rep >= 3:
                    ms[k].append(dt)
        r = {k: stats(v) for k, v in ms.items()}
        r["canvas_bytes_read_and_written"] = 2 * H * stride
        r["rectangle_bytes_read_and_written"] = 2 * rh * rw * pb
        r["compose_over_copy"] = round(r["compose"]["median_ms"] / r["copy_canvas"]["median_ms"], 4)
        r["compose_gbytes_per_s"] = round(2 * H * stride / r["compose"]["median_ms"] / 1e6, 1)
        r["copy_gbytes_per_s"] = round(2 * H * stride / r["copy_canvas"]["median_ms"] / 1e6, 1)
        r["bar_ms_copy_median_plus_its_spread"] = round(r["copy_canvas"]["median_ms"] + r["copy_canvas"]["spread_ms"], 4)
        r["compose_within_bar"] = r["compose"]["median_ms"] <= r["bar_ms_copy_median_plus_its_spread"]
        r["aliased_over_rectangle_copy"] = round(r["compose_aliased"]["median_ms"] / r["copy_rectangle"]["median_ms"], 4)
        r["aliased_gbytes_per_s"] = round(2 * rh * rw * pb / r["compose_aliased"]["median_ms"] / 1e6, 1)
        b = {}
        for form, kernel, yard, moved, yard_moved in (("canvas", "blend", "compose", 2 * H * stride + rh * rw * pb, 2 * H * stride), ("aliased", "blend_aliased", "compose_aliased", 3 * rh * rw * pb, 2 * rh * rw * pb)):
            rate = lambda nbytes, ms: nbytes / ms / 1e6
            y = r[yard]
            spread = rate(yard_moved, y["min_ms"]) - rate(yard_moved, y["max_ms"])
            b[form] = dict(r.pop(kernel), bytes_moved=moved)
            b[form]["gbytes_per_s"] = round(rate(moved, b[form]["median_ms"]), 1)
            b[form]["compose_gbytes_per_s_this_session"] = round(rate(yard_moved, y["median_ms"]), 1)
            b[form]["compose_gbytes_per_s_spread"] = round(spread, 1)
            b[form]["compose_median_ms_this_session"] = y["median_ms"]
            b[form]["bar_met"] = bool(b[form]["gbytes_per_s"] >= b[form]["compose_gbytes_per_s_this_session"] - b[form]["compose_gbytes_per_s_spread"])
        out["blend"][name] = b
        out["compose"][name] = r
        del canvas, slot, frame

    # (c) sixteen frames of 1080p: the sequence's own playback against a batch over the coded frames plus the composes
    n, aw, ah = 16, 1920, 1080
    crops = [""] + ["%d,%d,%d,%d" % (64 + 40 * k, 32 + 24 * k, 768, 512) for k in range(1, n)]
    path = os.path.join(CACHE, "frames_probe_animation.jxl")   # (the options make too long a file name for synth()'s cache)
    if not os.path.exists(path):
        os.makedirs(CACHE, exist_ok=True)
        subprocess.run([SYNTH, "vardct", str(aw), str(ah), "3", path, "frames=%d" % n, "anim=1", "crops=" + ";".join(crops), "durations=" + ",".join(["1"] * n)], check=True, stderr=subprocess.DEVNULL)
    with open(path, "rb") as fp:
        data = fp.read()
    seq = j40_amd.Sequence(data)
    seq.upload(0)
    frames = [seq.frame(k) for k in range(n)]
    rows = [seq.frame_info(k) for k in range(n)]
    canvas = torch.zeros((ah, aw, 4), dtype=torch.uint8, device="cuda:0")
    outs = [torch.zeros((fr.height, fr.width, 4), dtype=torch.uint8, device="cuda:0") for fr in frames]
    batch = j40_amd.Batch(frames)

    def play():
        seq.rewind()
        for _ in range(n):
            assert seq.next(canvas.data_ptr(), aw * 4, stream) == ""

    def batch_and_compose():
        batch.decode([o.data_ptr() for o in outs], [o.shape[1] * 4 for o in outs], stream)
        for r, o in zip(rows, outs):
            assert L.j40hip_kat_device_compose(canvas.data_ptr(), aw * 4, None, 0, o.data_ptr(), o.shape[1] * 4, aw, ah, r["x0"], r["y0"], r["w"], r["h"], 0xFF000000, 0, U8X4, stream) == 0   # (what the playback does: no slot is ever saved in this stream)

    ms = {"sequence_next_x16": [], "one_batch_plus_16_composes": []}
    for rep in range(args.reps + 2):
        for k, fn in (("sequence_next_x16", play), ("one_batch_plus_16_composes", batch_and_compose)):
            dt = clock(fn)
            if rep >= 2:
                ms[k].append(dt)
    assert seq.status() == ("", -1) and all(fr.status() == "" for fr in frames)
    out["animation_16_frames_1080p"] = dict({k: stats(v) for k, v in ms.items()}, codestream_bytes=len(data), crop="768x512")
    batch.close()
    seq.close()
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fp:
        fp.write(line + "\n")
    j40_amd.shutdown()


if __name__ == "__main__":
    main()
