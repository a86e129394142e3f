"""synthetic stream helpers shared by the tests, smoke() and bench.py (TEST INFRASTRUCTURE)"""
import os
import subprocess
import hashlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYNTH = os.path.join(ROOT, "build", "jxlsynth")
CACHE = os.path.join(ROOT, "build", "streams")


def synth(mode, w, h, seed, **opts):
    """returns the bytes of a generated stream (cached on disk by its parameters)"""
    os.makedirs(CACHE, exist_ok=True)
    key = "%s_%d_%d_%d_%s" % (mode, w, h, seed, "_".join("%s-%s" % kv for kv in sorted(opts.items())))
    path = os.path.join(CACHE, key + ".jxl")
    if not os.path.exists(path):
        if not os.path.exists(SYNTH):
            raise RuntimeError("build/jxlsynth is missing; run __graft_entry__.build()")
        tmp = path + ".tmp%d" % os.getpid()
        subprocess.run([SYNTH, mode, str(w), str(h), str(seed), tmp] + ["%s=%s" % kv for kv in sorted(opts.items())],
                       check=True, stderr=subprocess.DEVNULL)
        os.replace(tmp, path)
    with open(path, "rb") as fp:
        return fp.read()


def sha(a):
    return hashlib.sha256(a.tobytes() if hasattr(a, "tobytes") else a).hexdigest()


# the VarDCT feature matrix every parity test walks (small frames: the reference decodes them in ms)
VARDCT_CASES = [
    ("default", dict()),
    ("bctx", dict(bctx=1)),
    ("presets", dict(presets=2)),
    ("orders", dict(orders=1)),
    ("passes", dict(passes=2)),
    ("fullheader", dict(fullheader=1, xqm=2, bqm=4, nosmooth=1)),
    ("simpleclusters", dict(simpleclusters=1, logalpha=6)),
    ("cfl", dict(cfl=1)),
    ("container_jxlc", dict(container=1)),
    ("container_jxlp", dict(container=2)),
    ("hf_prefix_codes", dict(hfprefix=1)),                  # HF coefficient streams with prefix codes (fast encoders)
    ("hf_lz77", dict(hflz77=1)),                            # ... with LZ77 copies
    ("hf_prefix_lz77_passes", dict(hfprefix=1, hflz77=1, passes=2)),
    ("icc_profile", dict(icc=700)),
    ("permuted_toc_two_passes", dict(permute=1, passes=2)),  # sections stored in a shuffled order, Lehmer-coded permutation in the TOC
    ("alpha_extra_channel", dict(alpha=1)),                 # Modular sub-image after the HF coefficients of every group; the reference outputs opaque pixels                         # want_icc: the ICC stream is decoded and discarded like in the reference
    ("bit_depth_12", dict(bpp=12, cfl=1)),                  # more than 8 bits: the long way through the transfer curve, scaling to 8 bits at the end
    ("bit_depth_15", dict(bpp=15)),
    ("custom_dequant_matrices", dict(dq=2)),                # HfGlobal codes the 8x8 matrices in the Hornuss / DCT2x2 / DCT4x4 / DCT4x8 / AFV / band forms and two larger ones raw (Modular sub-images)
    ("not_xyb_encoded_decoded_as_xyb", dict(alpha=1, fullheader=1, noxyb=1)),   # reference quirk: the XYB inverse runs on any VarDCT frame (j40.h:7206)
]

# the Modular feature matrix (width, height, options); all decode bit-exactly
MODULAR_CASES = [
    ("single_group_gradient", 256, 256, dict()),
    ("fjxl_like_rgba", 256, 256, dict(alpha=1, prefix=1, lz77=1)),          # config 1 shape: single section, alpha, RCT 6, prefix codes + LZ77
    ("multi_group", 600, 300, dict()),
    ("property_tree", 600, 300, dict(tree=1)),
    ("weighted_predictor", 600, 300, dict(tree=2)),
    ("previous_channel_props_alpha", 600, 300, dict(tree=3, alpha=1)),
    ("palette", 600, 300, dict(palette=1)),
    ("palette_deltas_synthetic_alpha", 600, 300, dict(palette=2, alpha=1)),
    ("palette_delta_prediction", 300, 200, dict(palette=3)),
    ("rct_permuted_prefix", 600, 300, dict(rct=13, prefix=1)),
    ("no_rct_group128_lz77", 200, 100, dict(rct=-1, groupshift=7, lz77=1)),
    ("palette_prediction_wp_tree", 160, 120, dict(palette=3, tree=2)),
    ("container", 300, 200, dict(container=1, tree=1)),
    ("icc_profile", 256, 256, dict(icc=500, alpha=1)),
    ("local_tree_copy", 600, 300, dict(localtree=1, tree=1)),               # every other group: use_global_tree = 0, own code spec
    ("local_tree_wp_prefix_lz77_alpha", 600, 300, dict(localtree=2, prefix=1, lz77=1, alpha=1)),  # local tree needs WP, global does not
    ("local_tree_under_wp_global", 520, 520, dict(localtree=2, tree=2, groupshift=7)),
    ("flagged_xyb_rendered_raw", 300, 200, dict(xyb=1)),                     # the reference applies no colour transform to Modular frames
    ("flagged_ycbcr_rendered_raw_alpha", 300, 200, dict(ycbcr=1, alpha=1)),
    ("two_passes_last_one_stays", 600, 300, dict(passes=2, tree=1)),         # every pass codes the groups again (j40.h:7025-7033)
    ("three_passes_local_rct_local_tree_alpha", 520, 300, dict(passes=3, localrct=4, localtree=2, alpha=1)),
    ("permuted_toc", 600, 300, dict(permute=1, tree=1, alpha=1)),
    ("local_rct_per_group", 600, 300, dict(localrct=4, alpha=1)),            # every group lists RCTs of its own (one or two)
    ("local_rct_local_tree_no_global_rct", 520, 520, dict(localrct=13, localtree=2, rct=-1, groupshift=7)),
    ("bit_depth_10", 600, 300, dict(bpp=10, tree=1)),
    ("bit_depth_14_wp_rct", 300, 200, dict(bpp=14, tree=2, rct=13)),
    ("local_palette", 600, 300, dict(localpalette=1, tree=1)),                 # every other group: a palette of its own -> decoded in a sub-image, pasted
    ("local_palette_deltas_alpha_prefix_lz77", 520, 300, dict(localpalette=2, alpha=1, prefix=1, lz77=1, groupshift=7)),
    ("local_palette_predicted_two_passes", 600, 300, dict(localpalette=3, passes=2, tree=2, rct=-1)),
    ("local_palette_beside_local_rct_local_tree", 300, 200, dict(localpalette=1, localrct=5, localtree=2, groupshift=7)),
    ("four_extra_channels_alpha_last", 600, 300, dict(extra=3, alpha=1, tree=3, localrct=7)),   # depth channels ahead of the alpha channel
]


# ---- VarDCT streams outside an encoder's d1 statistics (tests/test_stress_streams.py) ----
# Every VARDCT_CASES stream has sparse blocks, magnitudes <= 40, the hybrid-integer configurations {4,1,1} / {4,2,0} and one quantiser
# (global_scale 8192, quant_lf 4, extra_precision 0). These rows leave that regime one axis at a time. A row is
# (name, family, options, traits); the frame is 776x520 where maxlog=8 asks for the 128 / 256-sized transforms and 520x264 otherwise
# (stress_size), the seed is STRESS_SEED. Traits a test asserts so that a row cannot silently stop doing what it is there for:
#   unsaturated  fewer than half of the reference's colour samples are 0 or 255 (the pixels say something)
#   overflows    more than 4 non-zeros per section byte: the event region of plan_build.cpp cannot hold them (`evof` on the batch path)
#   evof         some section leaves the events (region full or a value beyond int16) without the row promising the density above
#   top_mag      the largest magnitude among the reference's coefficients; it, half of it rounded up (the other end of bigbits' range)
#                and their negatives all occur. Beyond 32767 the frame leaves the events
#   error        the reference's error code for the stream ("" when absent)
STRESS_SEED = 7
_DENSE = dict(density=1, decay=1)
_BASE = dict(density=1, decay=1, global_scale=73728)     # at the default scale a dense picture is three quarters saturated
_BIG = dict(bigshare=0.02)


def _big(k, **more):
    # a magnitude in [2^(k-1), 2^k) packs into k + 1 bits; {4,1,1} and {4,2,0} keep 3 of them in the token: k - 2 extra bits
    return dict(_BIG, bigbits=k, **more), dict(top_mag=(1 << k) - 1)


VARDCT_STRESS_CASES = [
    # dense blocks, small values: non-zero counts at the format's cap, scans that run to the last position, full event rings
    ("dense", "dense", dict(_BASE), dict(unsaturated=1)),
    ("dense_ones", "dense", dict(_BASE, cont=0), dict(unsaturated=1)),
    ("dense_all_transforms", "dense", dict(_BASE, maxlog=8), dict(unsaturated=1)),
    ("dense_two_passes", "dense", dict(_BASE, passes=2), dict(unsaturated=1)),
    ("dense_prefix_codes", "dense", dict(_BASE, hfprefix=1), dict(unsaturated=1)),
    ("dense_lz77", "dense", dict(_BASE, hflz77=1), dict(unsaturated=1)),
    ("dense_quant_lf_16", "dense", dict(_BASE, quant_lf=16), dict(unsaturated=1)),
    ("dense_default_scale", "dense", dict(_DENSE), dict()),                      # mostly saturated: pinned by its coefficients
    # every non-zero the same value: rANS codes it in a fraction of a bit, the event region (4 events per section byte) overflows
    ("flat_ones", "overflow", dict(_DENSE, flat=1), dict(overflows=1)),
    ("flat_ones_all_transforms", "overflow", dict(_DENSE, flat=1, maxlog=8), dict(overflows=1)),
    # value boundaries: int16 (the event's value field; -32768 fits, +32768 does not), 17 / 18 / 20 extra bits around the lane reader's
    # refill, float exactness at 2^24, the largest hybrid integer the reference takes (30 bits) and the first it refuses
    ("big_15", "big") + _big(15),
    ("big_16", "big") + _big(16),
    ("big_19", "big") + _big(19),
    ("big_20", "big") + _big(20),
    ("big_22", "big") + _big(22),
    ("big_24", "big") + _big(24),
    ("big_25", "big") + _big(25),
    ("big_29", "big") + _big(29),
    ("big_30_refused", "big", dict(_BIG, bigbits=30), dict(error="iovf")),
    # hybrid-integer configurations (split_exp, msb, lsb) with long and with ordinary integers
    ("hybrid_000_big_22", "hybrid") + _big(22, hybrid="0,0,0"),
    ("hybrid_000_big_12", "hybrid") + _big(12, hybrid="0,0,0"),
    ("hybrid_400_big_22", "hybrid") + _big(22, hybrid="4,0,0"),
    ("hybrid_400_big_12", "hybrid") + _big(12, hybrid="4,0,0"),
    ("hybrid_720_big_22", "hybrid") + _big(22, hybrid="7,2,0", logalpha=8),
    ("hybrid_720_big_12", "hybrid") + _big(12, hybrid="7,2,0", logalpha=8),
    # (hybrid=8,3,2 cannot be written for rANS: split_exp == log_alpha_size = 8 leaves msb and lsb uncoded and no token beyond the
    # split; prefix codes read the configuration against 15 and have the alphabet for it)
    ("hybrid_832_prefix_big_22", "hybrid") + _big(22, hybrid="8,3,2", hfprefix=1),
    ("hybrid_832_prefix_big_12", "hybrid") + _big(12, hybrid="8,3,2", hfprefix=1),
] + [
    # quantiser extremes: one value per selector of global_scale's and quant_lf's U32 codes (73728 x 257 cannot be written: its LF
    # integers leave the LfGroup's 16-bit channels)
    ("scale_%d_lf_%d" % (gs, qlf), "quantiser", dict(global_scale=gs, quant_lf=qlf), dict(unsaturated=1) if gs >= 2048 else dict())
    for gs in (1, 2048, 2049, 4097, 8193, 73728) for qlf in (1, 16, 33, 257) if (gs, qlf) != (73728, 257)
] + [
    ("extra_precision_1_bctx", "quantiser", dict(extraprec=1, bctx=1), dict(unsaturated=1)),   # the LF thresholds look at the integers
    ("extra_precision_2_nosmooth", "quantiser", dict(extraprec=2, nosmooth=1), dict(unsaturated=1)),
    ("extra_precision_3", "quantiser", dict(extraprec=3), dict(unsaturated=1)),
    # mixes
    ("mix_dense_12_bits_cfl", "mix", dict(_BASE, bpp=12, cfl=1), dict()),
    ("mix_big_16_custom_dequant_alpha", "mix") + _big(16, dq=2, alpha=1),
    ("mix_flat_alpha_extra_precision", "mix", dict(_DENSE, flat=1, alpha=1, extraprec=2), dict(evof=1)),
]


def stress_size(opts):
    return (776, 520) if opts.get("maxlog") == 8 else (520, 264)


def stress_stream(opts):
    w, h = stress_size(opts)
    return synth("vardct", w, h, STRESS_SEED, **opts)
