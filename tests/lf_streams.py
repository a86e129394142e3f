"""LF-frame streams for tests/test_lf_frames.py and tests/test_lf_frames_gpu.py (TEST INFRASTRUCTURE): the generator's lflevels=
streams, their twins, and the shapes the tests share.

The generator cannot write a one-group XYB VarDCT frame, so an LF frame has to be wider than 256 pixels: the main frame is 2060 x 70 --
LF frame 258 x 9, two LfGroups side by side in the main frame, a partial last cell column and row -- or 70 x 2060, the vertical case;
two levels take 16400 x 70: level-1 frame 2050 x 9 (two LfGroups itself), level-2 frame 257 x 2."""
import json
import os
import subprocess
import tempfile

from streams import synth, SYNTH

SEED = 7
WIDE, TALL, TWO_LEVELS = (2060, 70), (70, 2060), (16400, 70)


def lf_stream(size, **opts):
    """LF frame(s) + the main frame with use_lf_frame, under one image header"""
    opts.setdefault("lflevels", 1)
    return synth("vardct", size[0], size[1], SEED, **opts)


def lf_twin(size, **opts):
    """the ordinary one-frame stream whose LF integers are the flat LF frame's, over 8 x 8 (two levels: 64 x 64) cells each"""
    opts.setdefault("lflevels", 1)
    return synth("vardct", size[0], size[1], SEED, lftwin=1, **opts)


def lf_stats(size, **opts):
    """what the generator says of the stream (stats=1): {"frames": coded frames, "lfidx_distinct": values the main frame's LF index takes}"""
    opts.setdefault("lflevels", 1)
    with tempfile.TemporaryDirectory() as d:
        args = [SYNTH, "vardct", str(size[0]), str(size[1]), str(SEED), os.path.join(d, "s.jxl"), "stats=1"] + ["%s=%s" % kv for kv in sorted(opts.items())]
        text = subprocess.run(args, check=True, stdout=subprocess.PIPE, stderr=subprocess.DEVNULL).stdout.decode()
    return json.loads(text.strip().splitlines()[-1])


def lf_size(size, level=1):
    w, h = size
    for _ in range(level):
        w, h = (w + 7) // 8, (h + 7) // 8
    return w, h


def without_first_frame(gpu_or_lib, data):
    """the stream with its first coded frame cut out: image header, then everything from the second frame's header on"""
    seq = gpu_or_lib.Sequence(data, lf_frames=True)
    a, b = seq.frame_info(0)["offset"], seq.frame_info(1)["offset"]
    seq.close()
    return data[:a] + data[b:]
