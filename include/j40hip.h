/*
 * include/j40hip.h -- thin C-ABI between the C host (container / header / TOC / LF parsing) and the
 * HIP hot path, plus stage-level entry points used by the parity tests.
 *
 * The reference has no plugin / FFI layer: its public API (include/j40.h) is the
 * drop-in boundary. This header is the *internal* seam the north star asks for -- "the C host parses
 * the container, frame header and group TOC, then hands the per-group hot path to HIP through a
 * thin C-ABI layer" -- cut where the reference calls j40__pass_group (j40.h:7007, driver loop
 * j40.h:8202-8204), j40__inverse_transform(&f->gmodular) (j40.h:8209), j40__combine_vardct
 * (j40.h:7862 / 8210) and j40__render_to_u8x4_rgba (j40.h:7910 / 8393). Plain pointers and sizes
 * only; every device pointer is a raw HIP device address, every stream a hipStream_t passed as void*.
 */
#ifndef J40HIP_H_
#define J40HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define J40HIP_API __attribute__((visibility("default")))

typedef struct j40hip_frame j40hip_frame;

/* ---- host side: replaces the reference's parse up to the section loop (j40.h:8175-8192 and the
 *      LF-group half of j40__lf_or_pass_group_in_section, j40.h:7840-7846) ---- */

/* Parses container, headers, TOC, LfGlobal, HfGlobal and all LfGroup sections of the single frame
 * in `buf` (borrowed until j40hip_frame_free). `threads` = host threads for LfGroup sections.
 * Returns NULL and sets *err (4-char code, same values as the reference's j40_err) on failure. */
J40HIP_API j40hip_frame *j40hip_frame_parse(const void *buf, size_t size, int threads, uint32_t *err);
/* flags & 1: leave the tail of every LfGroup -- dequantisation of the LF samples, adaptive smoothing, LLF coefficients (j40.h:6544-6590,
 * 6492, 5944) -- to the device: j40hip_frame_upload runs it there (device/lf_tail_kernels.hip). Same results; what the pipeline uses. */
J40HIP_API j40hip_frame *j40hip_frame_parse_ex(const void *buf, size_t size, int threads, uint32_t flags, uint32_t *err);
/* Streaming input (what replaces the reference's refillable source and backing buffer, j40.h:1220-1386, 1676-1812, for a buffer
 * that is still being filled -- a file being read, j40_from_file): `buf` has room for the `size` bytes the stream will have, and
 * the parse runs while they arrive. need(ctx, n) is called -- also from the parse's worker threads -- before any byte below n is
 * read and returns once bytes [0, n) are there (or the source has ended: what is missing is then a truncated stream, "shrt" where
 * the reference raises it); have(ctx) says how many are there now. The parse asks for the signature first; a bare codestream's
 * headers and TOC are parsed on growing prefixes, then LfGlobal, HfGlobal and each LfGroup section as its bytes are due, so the
 * host's part of the decode overlaps the arrival of the pass-group sections (most of the file), which only the device reads:
 * wait for the rest before j40hip_frame_upload. A container is parsed once it is complete. Same frame as j40hip_frame_parse_ex. */
typedef void (*j40hip_need_bytes)(void *ctx, size_t upto);
typedef size_t (*j40hip_have_bytes)(void *ctx);
J40HIP_API j40hip_frame *j40hip_frame_parse_streamed(const void *buf, size_t size, int threads, uint32_t flags, j40hip_need_bytes need, j40hip_have_bytes have, void *ctx, uint32_t *err);
/* ... with the LfGroup streams (LF coefficients, HF metadata: j40.h:6722-6790) decoded on HIP device `device` on `stream` (a
 * hipStream_t) instead of the host; `flags` must include 1. The call sleeps while the device works -- meant for many parsing
 * threads per CPU (the pipeline). Frames outside what the device decoder takes are parsed on the host, same results.
 * j40hip_frame_lf_on_device tells which it was. */
J40HIP_API j40hip_frame *j40hip_frame_parse_on(const void *buf, size_t size, int threads, uint32_t flags, int device, void *stream, uint32_t *err);
J40HIP_API int j40hip_frame_lf_on_device(const j40hip_frame *f);
J40HIP_API void j40hip_frame_free(j40hip_frame *f);

/* ---- the LF preview: the 1:8 image every VarDCT frame carries in its LfGroup sections (one XYB sample per 8x8 cell, the cell's mean),
 *      decoded from those sections alone -- libjxl's progressive "DC" step. INTEGRATION.md, "LF preview". ----
 * flags & J40HIP_PARSE_LF_ONLY (j40hip_frame_parse_ex / _streamed / _on): the parse reads headers, TOC, LfGlobal and every LfGroup
 * section, with the same checks and codes as the full parse, and never reads nor asks for HfGlobal or a pass-group section, so a
 * codestream cut at j40hip_frame_lf_end parses. Such a frame can only be previewed: j40hip_frame_decode / _timed / _decode_to_host and
 * j40hip_batch_create refuse it with "Ulf?". Modular frames: "TODO" (no LF image without Squeeze). */
#define J40HIP_PARSE_LF_ONLY 2u
/* flags & J40HIP_PARSE_YCBCR: YCbCr frames are asked for (see j40hip_frame_set_ycbcr): a frame whose channels are subsampled is parsed
 * instead of refused with "TODO" before its LF image is read, which is where the reference refuses it. J40HIP_YCBCR=1 in the
 * environment does the same for every parse. */
#define J40HIP_PARSE_YCBCR 4u
/* flags & J40HIP_PARSE_WIDE: wide Modular frames are asked for (see j40hip_frame_wide): an image whose metadata says
 * modular_16bit_buffers = 0 -- every 16-bit lossless image, and what libjxl writes for every image deeper than 12 bits -- is parsed
 * instead of refused with "fm32", which is where the reference refuses it (j40.h:3169). A Modular frame of such an image is then decoded
 * with 32-bit sample planes; a VarDCT frame of one is "TODO" at parse. J40HIP_WIDE=1 in the environment does the same for every parse,
 * and j40hip_sequence_open takes the flag too. */
#define J40HIP_PARSE_WIDE 8u
/* flags & J40HIP_PARSE_NOISE: photon noise is asked for. PARITY UNPINNED: the reference stops at has_noise (j40.h:6264, "TODO"), and so
 * does every parse without this flag. With it a frame whose header has has_noise is parsed -- its eight NoiseParameters follow the patch
 * dictionary in LfGlobal (behind the splines, where the frame has them: J40HIP_PARSE_SPLINES) -- and every decode of the frame adds the noise to the
 * frame's XYB samples behind the restoration filters and the patches, ahead of the colour tail (k_noise_fill, k_noise_add;
 * j40_amd/csrc/device/noise_dev.h states the rule). "TODO" at parse even with the flag: an image with xyb_encoded = 0; an LF frame or a
 * reference-only frame (type 1 or 2) with has_noise. A frame with noise decodes whole frames at full size: a region or a scale is cut
 * or averaged from the full-size picture, the orientation, kept alpha, the restoration filters, the colour mode and patches combine
 * with it; a Modular frame needs the Modular XYB switch (j40hip_frame_set_modular_xyb), a YCbCr plan, a group range, a batch, a
 * pipeline, the LF preview and an LF-only parse of such a frame are "TODO". A LUT of eight zeros launches nothing.
 * J40HIP_NOISE=1 in the environment does the same for every parse, and j40hip_sequence_open takes the flag too: the frames of a
 * sequence get the seed counters of their place in it (visible: the shown frames before it, nonvisible: the frames since the last
 * shown one); a stand-alone handle has both 0. */
#define J40HIP_PARSE_NOISE 256u
/* flags & J40HIP_PARSE_SPLINES: splines are asked for. PARITY UNPINNED: the reference stops at has_splines (j40.h:6263, "TODO"), and so
 * does every parse without this flag. With it a frame whose header has has_splines is parsed -- the splines follow the patch dictionary
 * in LfGlobal, ahead of the noise parameters: one entropy-coded stream over six contexts -- and every decode of the frame draws them
 * onto the frame's XYB samples behind the restoration filters and the patches, ahead of the noise and the colour tail (k_spline_draw;
 * j40_amd/csrc/device/spline_dev.h states the rule). A damaged spline stream is "spln": more splines than min(1 << 24, W * H / 4), more
 * control points than min(1 << 20, W * H / 2), a starting or control-point coordinate of magnitude above 1 << 23, two successive
 * control points that are equal, more than 1 << 22 segments (counted along the curves, before any is dropped), more than 1 << 24
 * (tile, segment) pairs; at parse for a handle, at j40hip_sequence_open for a frame of a sequence. "TODO" at parse even with the flag:
 * an image with xyb_encoded = 0; an LF frame or a reference-only frame (type 1 or 2) with has_splines; an LF-only parse. A frame with
 * splines decodes as one with noise does: whole frames at full size, from which a region is cut and a scale averaged; the orientation,
 * kept alpha, the restoration filters, the colour mode, patches and noise combine with it; a Modular frame needs the Modular XYB
 * switch; a YCbCr plan, a group range, a batch, a pipeline, the LF preview and a frame that is upsampled as well are "TODO". A frame
 * whose segments all drop launches nothing. J40HIP_SPLINES=1 in the environment does the same for every parse, and
 * j40hip_sequence_open takes the flag too (J40HIP_SEQ_SPLINES). */
#define J40HIP_PARSE_SPLINES 1024u
#define J40HIP_SEQ_SPLINES 1024u
/* flags & J40HIP_PARSE_UPSAMPLING: upsampling is asked for. PARITY UNPINNED: the reference refuses a frame header with upsampling or an
 * ec_upsampling other than 1 (j40.h:3297-3306, 5244-5249) and custom upsampling weights in the image header (j40.h:3638) with "TODO", and so
 * does every parse without this flag. With it the custom weights are read and kept, and a frame coded at 1:2, 1:4 or 1:8
 * (cjxl --resampling=2|4|8) is parsed: its header's width and height are the SHOWN size, everything up to and including the restoration
 * filters works on the CODED size ceil(shown / K), and every decode stretches the filtered XYB planes K times (k_upsample: a 5 x 5 stencil,
 * K x K outputs a coded sample, each clamped to its neighbourhood's range; j40_amd/csrc/device/upsample_dev.h states the rule) ahead of the
 * colour tail and writes the shown size. j40hip_frame_info, the region, the scale and the orientation speak of the shown size;
 * j40hip_frame_coded_size of the coded one. The weights: the stream's custom table for the frame's K, else the defaults the application
 * supplied (j40hip_set_upsampling_defaults -- nothing here holds the standard's default tables); neither: "updf" at parse. "usmp": an
 * extra channel coded finer than the frame ((ec_upsampling << dim_shift) < upsampling). Served: VarDCT frames of XYB images and, through
 * the Modular XYB switch, Modular ones (an image with xyb_encoded = 0 that is no YCbCr frame: "TODO" at parse); both output formats, the orientation, the restoration filters, the colour mode; a region is cut
 * from and a scale averaged over the shown-size picture. An extra channel of a VarDCT frame coarser than the frame (ec_upsampling up to four
 * times upsampling) is decoded at its own size, ceil(shown / ec_upsampling), and dropped. "TODO" even with the flag: an extra channel
 * from eight times coarser than the frame on, or coarser at all in a Modular frame; frames of types 1 and 2, an LF-only parse, every frame of a sequence (at parse); a partial group range, a batch, a
 * pipeline, the many-frames LF preview, kept alpha (j40hip_frame_set_alpha), a Modular frame with an alpha channel or without the Modular
 * XYB switch, a YCbCr plan, a frame that also has patches or noise (at the setter or the decode, before anything is launched).
 * J40HIP_UPSAMPLING=1 in the environment does the same for every parse, the ten-function API's too. j40hip_sequence_open takes
 * J40HIP_SEQ_UPSAMPLING (the same bit): the image header's custom weights are read; its frames with upsampling > 1 stay "TODO". */
#define J40HIP_PARSE_UPSAMPLING 512u
#define J40HIP_SEQ_UPSAMPLING 512u
/* the shortest prefix of the codestream holding headers, TOC, LfGlobal and every LfGroup section (the largest end among those
 * sections, so a permuted TOC is covered); a bare codestream's file prefix. Single-section frames: the whole codestream. */
J40HIP_API int64_t j40hip_frame_lf_end(const j40hip_frame *f);
/* the preview's size: ceil(width / 8) x ceil(height / 8) */
J40HIP_API void j40hip_frame_lf_size(const j40hip_frame *f, int32_t *w, int32_t *h);
/* channel c (0 X, 1 Y, 2 B) of the LF image on the host: every cell's integer times its LfGroup's dequantisation factor (j40.h:6562),
 * adaptively smoothed within the LfGroup unless the frame skips it (j40.h:6492-6540), over the preview's grid row by row -- the
 * samples the LLF coefficients are made of. 0, "rnge" (c out of range), "TODO" (Modular frames; frames built from a plan view) */
J40HIP_API uint32_t j40hip_frame_lf_plane(const j40hip_frame *f, int c, float *out);
/* the constants of the preview's colour tail as parsed: out15 = opsin_inv_mat[9] (row-major), opsin_bias[3], intensity_target, and the
 * LF chroma-from-luma factors kx_lf, kb_lf (j40.h:7115-7116) */
J40HIP_API void j40hip_frame_colour_consts(const j40hip_frame *f, float *out15);
/* LfGlobal's LF dequantisation as parsed: out3 = m_lf_scaled of X, Y, B (defaults 1/4096, 1/512, 1/256) -- the factors of a VarDCT frame's
 * LF samples and of a Modular frame's samples under j40hip_frame_set_modular_xyb */
J40HIP_API void j40hip_frame_lf_dequant(const j40hip_frame *f, float *out3);

/* out[0..20] = width, height, is_modular, num_lf_groups, num_groups, num_passes, nb_block_ctx,
 * block_ctx_size, num_hf_presets, global_scale, quant_lf, x_qm_scale, b_qm_scale, nb_qf_thr,
 * nb_lf_thr[0..2], group_size_shift, bpp, num_extra_channels, xyb_encoded */
J40HIP_API void j40hip_frame_info(const j40hip_frame *f, int64_t *out);
/* bytes of the (re-assembled) codestream and number of pass-group sections */
J40HIP_API size_t j40hip_frame_codestream_size(const j40hip_frame *f);
J40HIP_API int64_t j40hip_frame_num_sections(const j40hip_frame *f);
/* bytes of every pass-group section as the TOC lists them (j40.h:5529), pass-major; out may be NULL; returns how many */
J40HIP_API int64_t j40hip_frame_section_sizes(const j40hip_frame *f, int64_t *out);
/* Modular frames: sections decoded by the wave-cooperative form of the section kernel (diagnostic; -1 when the frame has no Modular plan) */
J40HIP_API int32_t j40hip_frame_coop_sections(j40hip_frame *f, int32_t *total);
J40HIP_API int32_t j40hip_frame_quad_sections(j40hip_frame *f);   /* ... of those, decoded four to a wavefront */
/* sections whose MA tree looks only at a sample's position (properties 0-3, no weighted predictor -- what fast lossless encoders write): decoded
 * in two passes, the stream's tokens first, the prediction behind them (modular_split.hip); J40HIP_NO_SPLIT=1 leaves them to the one-pass kernels */
J40HIP_API int32_t j40hip_frame_split_sections(j40hip_frame *f);

/* stage accessors for parity tests (mirror j40__lf_group_st, j40.h:6360-6390) */
J40HIP_API void j40hip_frame_lf_group_info(const j40hip_frame *f, int64_t gg, int32_t *out9);
/* which: 0 blocks (i32 w8*h8), 1 lfindices (u8 w8*h8), 2 xfromy (i16 w64*h64), 3 bfromy */
J40HIP_API int j40hip_frame_lf_group_plane(const j40hip_frame *f, int64_t gg, int which, void *out);
J40HIP_API void j40hip_frame_varblocks(const j40hip_frame *f, int64_t gg, int32_t *coeffoff_qfidx, float *hfmul_inv);
J40HIP_API void j40hip_frame_llf(const j40hip_frame *f, int64_t gg, int c, float *out);
J40HIP_API int32_t j40hip_frame_dq_matrix(const j40hip_frame *f, int idx, float *out_n_by_3);
J40HIP_API int32_t j40hip_frame_order(const j40hip_frame *f, int pass, int idx, int c, int32_t *out);
J40HIP_API int32_t j40hip_frame_block_ctx_map(const j40hip_frame *f, uint8_t *out);
/* Modular planes decoded on the host inside LfGlobal (j40.h:6334-6336): returns 0 and fills w*h int16 */
J40HIP_API int j40hip_frame_global_plane(const j40hip_frame *f, int c, int16_t *out, int32_t *w, int32_t *h);

/* ---- plan views: what crosses the seam, as plain C arrays (mirrors of j40__frame_st, j40.h:5061-5122,
 *      j40__lf_group_st, j40.h:6360-6390, j40__code_spec, j40.h:2486-2495, j40__modular, j40.h:3553-3564).
 *      Pointers stay valid until j40hip_frame_free. Used by the CPU oracle (oracle/hotpath_oracle.c) so
 *      that it can be driven behind exactly the same boundary as the HIP kernels. ---- */

typedef struct {
	int32_t split_exp, msb_in_token, lsb_in_token;   /* hybrid integer config (j40.h:2283) */
	const int16_t *D;              /* ANS: distribution, 1 << log_alpha_size entries summing to 4096 */
	const uint8_t *lengths;        /* prefix code: code length per symbol */
	int32_t alphabet_size;         /* prefix code: number of symbols */
} j40hip_cluster_view;

typedef struct {
	int32_t num_dist, num_clusters;
	int32_t lz77_enabled, use_prefix_code, min_symbol, min_length, log_alpha_size;
	int32_t lz_len_split_exp, lz_len_msb, lz_len_lsb;
	const uint8_t *cluster_map;    /* [num_dist] */
	const j40hip_cluster_view *clusters;
} j40hip_codespec_view;

typedef struct {
	int32_t left, top, width, height, width8, height8, width64, height64, nb_varblocks;
	const int32_t *blocks;         /* [height8 * width8], (DctSelect + 2) << 20 | varblock or 1 << 20 | varblock */
	const uint8_t *lfindices;      /* [height8 * width8] */
	const float *llfcoeffs[3];     /* [height8 * width8] */
	const int32_t *coeffoff_qfidx; /* [nb_varblocks] */
	const float *hfmul_inv;        /* [nb_varblocks] */
	const int16_t *xfromy, *bfromy;/* [height64 * width64] */
} j40hip_lf_group_view;

typedef struct { uint32_t byte_off, size, bit_off; int32_t ggidx, gx_in_gg, gy_in_gg, gw, gh; } j40hip_section_view;

typedef struct {
	int32_t width, height, num_passes, num_groups, num_lf_groups;
	int32_t nb_block_ctx, nb_qf_thr, nb_lf_thr[3], num_hf_presets, bpp;
	int32_t sections_have_trailer;   /* extra channels: a Modular sub-image follows the coefficients of each section */
	uint32_t single_declared_end;    /* single-section frames: the TOC's end of the section (byte offset); the section itself is readable to the
	                                    end of the codestream, ending short of this is shrt, past it excs (j40.h:7796-7803) */
	int32_t check_section_end;       /* single-section frames only: zero padding + no bytes left at the section's end (the reference checks
	                                    nothing in frames with several sections, j40.h:7778-7795) */
	int32_t global_scale, x_qm_scale, b_qm_scale, x_factor_lf, b_factor_lf;
	float quant_bias[3], quant_bias_num, base_corr_x, base_corr_b, inv_colour_factor;
	float opsin_inv_mat[9], opsin_bias[3], intensity_target;
	const uint8_t *codestream; size_t codestream_size;
	const uint8_t *block_ctx_map; int32_t block_ctx_size;
	const j40hip_codespec_view *coeff_specs;     /* [num_passes] */
	const int32_t *orders[11 * 13 * 3];           /* [pass][order][channel] -> coefficient order or NULL */
	const float *dq_matrix[17]; int32_t dq_size[17];  /* [size][3] dequantisation weights or NULL */
	const j40hip_lf_group_view *lf_groups;       /* [num_lf_groups] */
	const j40hip_section_view *sections;         /* [num_passes * num_groups] */
} j40hip_vardct_view;

typedef struct { int32_t prop, value, a, b; } j40hip_tree_node;   /* see j40_amd/csrc/modular.hpp */
/* kind 0 RCT, 1 Palette, 2 one Squeeze step (channels [begin_c, begin_c + num_c) halved along rows if `horizontal`, else along
 * columns; residual channels right behind them if `in_place`, else at the end of the list) */
typedef struct { int32_t kind, begin_c, rct_type, num_c, nb_colours, nb_deltas, d_pred, horizontal, in_place; } j40hip_transform_view;
typedef struct {
	uint32_t byte_off, size, bit_off; int32_t gx, gy, gw, gh, sidx, first_channel, num_channels;
	int8_t wp[12];                 /* weighted predictor parameters p1, p2, p3[5], w[4] */
	/* the section's MA tree = tree[tree_off .. tree_off + tree_nodes) and its code spec = codespec[spec_idx]:
	 * the global pair, or the section's own when its header says use_global_tree = 0 (j40.h:3740-3746) */
	uint32_t tree_off; int32_t tree_nodes, spec_idx;
	/* RCTs of the section's own header (j40.h:3757), undone over its rectangle before the global transforms
	 * (j40.h:7030): pairs {begin_c relative to first_channel, rct_type} at local_rct + 2 * local_off */
	int32_t local_off, local_count;
	/* a section whose own header lists a palette decodes into a sub-image of its own (the reference's j40__pass_group does that
	 * for every section, j40.h:7024-7032): num_channels planes sub_w/h/meta[sub_off ..], its transforms
	 * sub_transforms[sub_tr_off .. sub_tr_off + sub_tr_count) undone there, then the channels pasted over the rectangle unless
	 * sub_paste is 0 (an earlier pass of a multi-pass frame). sub_off < 0: no sub-image, channels first_channel ... of the frame */
	int32_t sub_off, sub_tr_off, sub_tr_count, sub_paste;
	uint32_t preset_status;        /* != 0: the section's own Modular header did not parse; this is its status, nothing is decoded */
	/* frames whose channels differ in size (after a Squeeze): the section's channels as explicit rectangles,
	 * chan_rects[6 * (chan_off + i)] = {channel, x0, y0, width, height, hshift | vshift << 8}; -1: first_channel ... over gx, gy, gw, gh */
	int32_t chan_off;
	/* the LZ77 distance multiplier of the section's stream + 1 (j40.h:3840-3844), or 0: the widest non-meta channel among the section's
	 * own channels. LfGlobal's section takes the frame-wide image's, which also counts channels the section does not code */
	int32_t dist_mult_p1;
} j40hip_modular_section_view;

typedef struct {
	int32_t width, height, bpp, num_channels, num_sections, num_transforms, num_tree_nodes, alpha_channel;
	int32_t check_section_end;     /* as in j40hip_vardct_view */
	uint32_t single_declared_end;
	const uint8_t *codestream; size_t codestream_size;
	const j40hip_codespec_view *codespec;     /* [num_codespecs] */
	const j40hip_tree_node *tree;              /* [num_tree_nodes]: every tree in use, back to back */
	int32_t num_codespecs;
	const int32_t *channel_w, *channel_h, *channel_meta;   /* coded channels */
	const j40hip_transform_view *transforms;
	const j40hip_modular_section_view *sections;
	const int32_t *local_rct;
	const int32_t *sub_w, *sub_h, *sub_meta;
	const j40hip_transform_view *sub_transforms;
	int8_t global_wp[12];
	const int32_t *chan_rects;
} j40hip_modular_view;

/* The seam for a host that parses the bitstream itself (a patched j40): a frame handle built from the
 * view instead of from a bitstream; then j40hip_frame_upload / j40hip_frame_decode* as usual. Everything is copied. (The view does
 * not carry the global MA tree, so for frames with extra channels the sub-images behind the coefficients are not validated.) */
J40HIP_API j40hip_frame *j40hip_frame_from_vardct_view(const j40hip_vardct_view *v, uint32_t *err);
/* The same seam across processes (the "LF bundle" one rank parses and the others receive): the view flattened
 * into one relocatable blob. j40hip_frame_lf_bundle returns the bytes it needs and writes them when `capacity` suffices (call it
 * with out = NULL first); j40hip_frame_from_lf_bundle builds a frame handle from a received blob (everything is copied and
 * bounds-checked; "rnge" for a malformed blob). */
J40HIP_API size_t j40hip_frame_lf_bundle(j40hip_frame *f, void *out, size_t capacity, uint32_t *err);
J40HIP_API j40hip_frame *j40hip_frame_from_lf_bundle(const void *blob, size_t size, uint32_t *err);

/* What the reference reports after a frame that decoded cleanly: "excs" when bytes follow the frame and the reference gets to see
 * them -- always for single-section frames; for frames with several sections only if the frame ends within the first 64 KB its main
 * buffer holds (j40__seek_buffer, j40.h:1745-1760: otherwise the buffer is emptied, not refilled, and j40__no_more_bytes passes).
 * Bare codestreams only; 0 otherwise. The public API (api.cpp) applies it after a successful decode. */
J40HIP_API uint32_t j40hip_frame_after_frame_status(const j40hip_frame *f);

/* fill the views for a parsed frame; return 0 or a 4-char code ("TODO" for frames the hot path does not cover) */
J40HIP_API uint32_t j40hip_frame_vardct_view(j40hip_frame *f, j40hip_vardct_view *out);
J40HIP_API uint32_t j40hip_frame_modular_view(j40hip_frame *f, j40hip_modular_view *out);

/* host table builders exposed for known-answer tests against the reference's internals */
J40HIP_API int32_t j40hip_kat_natural_order(int32_t log_rows, int32_t log_columns, int32_t *out);          /* j40.h:4980 */
J40HIP_API int32_t j40hip_kat_library_dq_matrix(int idx, float *out_n_by_3);                              /* j40.h:4828 */
J40HIP_API void j40hip_kat_forward_llf(float *buf, int32_t log_rows, int32_t log_columns);                /* j40.h:5944 */
J40HIP_API float j40hip_kat_half_secant(int i);                                                           /* j40.h:5690 */
J40HIP_API float j40hip_kat_lf2llf_scale(int i);                                                          /* j40.h:5739 */

/* ---- device side ---- */

/* Number of visible HIP devices (0 when there is none); never throws. */
J40HIP_API int j40hip_device_count(void);

/* Uploads the frame plan (codestream, code specs, orders, dequant tables, LF bundle) to `device`
 * and allocates the working buffers. Returns 0 or a 4-char error ("!gpu": no device / HIP error). */
J40HIP_API uint32_t j40hip_frame_upload(j40hip_frame *f, int device);

/* Single-pass frames keep their quantised coefficients as per-block event lists sized from the section sizes. A section
 * with more non-zero coefficients than its region holds reports "evof" (j40hip_frame_status); j40hip_frame_decode_to_host
 * and the public API then repeat the decode with dense planes on their own, callers of the asynchronous entry points
 * call this and upload / decode again. */
J40HIP_API void j40hip_frame_force_dense(j40hip_frame *f, int dense);

/* Section subset decoded by this process (multi-GPU sharding by pass-group section):
 * groups [first_group, first_group + num_groups) of every pass. Default: all. */
J40HIP_API uint32_t j40hip_frame_set_group_range(j40hip_frame *f, int64_t first_group, int64_t num_groups);

/* Runs the hot path on `stream`: entropy decode of every pass-group section, dequantisation,
 * chroma-from-luma, inverse transforms, XYB -> sRGB and RGBA u8x4 packing (or the Modular
 * equivalents) into device memory `rgba_dev` with `stride_bytes` per row. Asynchronous. */
J40HIP_API uint32_t j40hip_frame_decode(j40hip_frame *f, void *rgba_dev, size_t stride_bytes, void *stream);

/* The frame's output format: J40HIP_U8X4 (the default; 4 bytes a pixel) or J40HIP_U16X4 (16-bit RGBA, 8 bytes a pixel: every
 * sample at the image's bit depth p in [0, maxpixel = 2^bpp - 1] as (p * 65535 + 2^(bpp - 1)) / maxpixel; 8-bit images: u8 * 257).
 * Every entry point that writes pixels -- j40hip_frame_decode / _timed / _decode_to_host, j40hip_batch_decode* -- writes the frame's
 * format; a 16-bit frame's stride_bytes below 8 * width is "rnge", a batch whose frames disagree "Uof?", before anything is launched.
 * set: 0, or "Ufm?" for any other value (the frame is left as it was). Pipelines write u8x4 only. */
#define J40HIP_U8X4 0x0f33  /* = J40_U8X4 (include/j40.h) */
#define J40HIP_U16X4 0x0f35 /* = J40_U16X4 */
J40HIP_API uint32_t j40hip_frame_set_output_format(j40hip_frame *f, int32_t format);
J40HIP_API int32_t j40hip_frame_output_format(const j40hip_frame *f);

/* ---- the alpha channel of VarDCT frames. A lossy image with transparency carries its alpha as an extra channel, a Modular sub-image
 *      behind the HF coefficients of every pass-group section. The reference decodes these and drops them (j40__combine_vardct,
 *      j40.h:7868): its pixels have A = 255, and so have this library's by DEFAULT (mode 0, drop). Mode 1, keep: A is the first extra
 *      channel of type alpha, rendered as the reference renders a Modular frame's alpha (j40.h:7950): the sample p clamped to
 *      [0, maxpixel = 2^bpp - 1], then (p * 255 + 2^(bpp - 1)) / maxpixel, or the J40HIP_U16X4 rule for 16-bit output. R, G, B and
 *      every status code are those of drop mode.
 *      Served: frames of one pass and more than one group (the extra channels in the pass-group sections, any number of them, alpha
 *      at any index), 8..15 bits, no transform in the global Modular header, an alpha channel the reference's render accepts (the
 *      image's depth and sample type, not subsampled, not associated). Reversible colour transforms a section's own header lists are
 *      undone; any other transform there makes a keep-mode decode "TODO".
 *      set: mode -1 follows the environment (J40HIP_ALPHA=1 keeps; the default), 0 drops, 1 keeps. Returns 0; "TODO", the frame left
 *      as it was, when mode 1 is asked of a frame outside the above; "Ual?" for a frame without an alpha channel and for a Modular
 *      frame, whose alpha is always rendered. With the environment variable alone a frame outside the above decodes opaque as before.
 *      Every single-frame entry point that writes full-size pixels honours it: j40hip_frame_decode / _timed / _decode_to_host (these
 *      synchronise for such frames anyway), with the restoration filters (the merge comes last), with a group range (only that
 *      range's sub-images and rectangles). In a batch the alpha of a keep-mode member is merged when j40hip_frame_status is read, where
 *      its sub-images are validated: into the buffer and stride given at the batch decode, which must stay valid until then; A is 255
 *      before. LF previews stay opaque (the LF sections carry no alpha).
 *      j40hip_frame_alpha: out[0] the index of the alpha extra channel or -1, out[1] its bpp, out[2] the mode in force (1: the next
 *      decode keeps alpha), out[3] whether the last decode wrote it. ---- */
J40HIP_API uint32_t j40hip_frame_set_alpha(j40hip_frame *f, int mode);
J40HIP_API void j40hip_frame_alpha(const j40hip_frame *f, int32_t out[4]);
/* known-answer / measuring hook: k_alpha_merge alone. plane_dev: int16 samples of an alpha channel of `bpp` bits (8..15), `pitch` of
 * them a row, in device memory; they become the A of rectangle (x0, y0, w, h) of the pixels at rgba_dev (format J40HIP_U8X4 or
 * J40HIP_U16X4, rows pixel-aligned). Asynchronous on `stream`. 0, "rnge" for a bpp or rectangle out of range, "Ufm?". */
J40HIP_API uint32_t j40hip_kat_device_alpha_merge(void *rgba_dev, size_t stride_bytes, const int16_t *plane_dev, int32_t pitch, int32_t x0, int32_t y0, int32_t w, int32_t h, int32_t bpp, int32_t format, void *stream);

/* ---- YCbCr VarDCT frames: losslessly recompressed JPEGs ("YCbCr frames"; DESIGN.md has the rules). Such a frame has
 *      xyb_encoded = 0 and do_ycbcr = 1: its three channels are Cb, Y, Cr in the slots of X, Y, B, 4:4:4 or with chroma at half the
 *      resolution along one or both axes (jpeg_upsampling). The reference refuses them (j40.h:7867, 6749) and so does this library
 *      unless asked: the feature is opt-in, and none of its arithmetic past the inverse transforms is pinned by the reference.
 *      set: mode -1 follows the environment (J40HIP_YCBCR=1 serves; the default), 0 refuses, 1 serves. It holds from the next upload
 *      on. A frame with subsampled channels must also have been PARSED with YCbCr frames asked for (J40HIP_PARSE_YCBCR, or the
 *      environment variable), else its parse has already failed with "TODO".
 *      Served: j40hip_frame_upload + j40hip_frame_decode / _timed / _decode_to_host of 8..15-bit colour images, both output formats,
 *      kept alpha included; 4:4:4 frames with every transform, chroma-from-luma and the restoration filters; subsampled frames
 *      (4:2:0, 4:2:2, 4:4:0) made of DCT8 blocks, with skip_adapt_lf_smooth and without restoration filters signalled.
 *      "TODO": everything else -- grey images, float samples, LF frames, other subsampled frames -- and every other entry: batches,
 *      pipelines, LF previews, a region, a scale, a group range, sequences, plan views.
 *      j40hip_frame_ycbcr: out[0] the frame is a YCbCr VarDCT frame; out[1..6] (hshift, vshift) of Cb, Y, Cr: log2 of how much coarser
 *      than the finest channel it is sampled; out[7] the last decode went through the YCbCr planes and k_ycbcr_tail. ---- */
J40HIP_API uint32_t j40hip_frame_set_ycbcr(j40hip_frame *f, int mode);
J40HIP_API void j40hip_frame_ycbcr(const j40hip_frame *f, int32_t out[8]);
/* ---- wide Modular frames ("16-bit images"): Modular frames of images with 32-bit Modular buffers, integer samples of
 *      8..16 bits, alpha at the same depth. Opt-in at parse (J40HIP_PARSE_WIDE / J40HIP_WIDE=1). Served: everything a narrow Modular frame
 *      is served with -- both output formats, a region, a scale, an orientation, a group range, sequences. "TODO": VarDCT frames of such
 *      images, batches, pipelines. Pinned by lossless round trips and by equality with the narrow path, not by the reference.
 *      j40hip_frame_wide: out[0] the image has 32-bit buffers; out[1] its bit depth; out[2] the last decode ran the int32 kernels;
 *      out[3] bytes per sample of the frame's planes on the device (2 or 4; 0 before an upload). ---- */
J40HIP_API void j40hip_frame_wide(const j40hip_frame *f, int32_t out[4]);
/* ---- Modular frames of XYB images ("Modular frames of XYB images"; DESIGN.md section 4 has the rule). An image with
 *      xyb_encoded = 1 may carry its colour in a Modular frame (lossy Modular, every LF frame a real encoder writes): three planes of
 *      quantised integers Y, X, B - Y. The reference applies no colour transform to a Modular frame (j40.h:7910-7962) and renders those
 *      integers as R, G, B; so does this library unless asked. PARITY UNPINNED: no decoder at hand pins the rule.
 *      set: mode -1 follows the environment (J40HIP_MODULAR_XYB=1 serves; the default), 0 renders R, G, B, 1 renders through the XYB
 *      colour tail: Y = (float) c0 * m[1], X = (float) c1 * m[0], B = (float) (c2 + c0) * m[2] with m = LfGlobal's LF dequantisation
 *      (integer sum, one conversion, one multiply), then what a VarDCT frame's colour tail makes of X, Y, B; A from the alpha plane as
 *      before. Mode 1 is refused with "Umx?" (the frame is left as it was) for a frame the rule does not apply to: VarDCT frames, images
 *      with xyb_encoded = 0, grey images, do_ycbcr, float samples, bpp < 8, handles built from a view. The environment variable alone
 *      leaves such frames as they were. It holds from the next decode on.
 *      Served with the switch on: both output formats, a region, a group range, scale 1 and 2 (through the full-size staging image and
 *      k_downscale), the orientation, wide frames, sequences (Replace and the blend modes). "TODO" or as before: batches and pipelines
 *      (no Modular frames there), restoration filters (a Modular frame applies none), type-2 frames, patches, splines, noise, upsampling.
 *      j40hip_frame_modular_xyb: out[0] the rule applies to the frame; out[1] it is in force; out[2] bytes per sample of the frame's
 *      planes (2 or 4; 0 for a VarDCT frame); out[3] the last decode went through k_modular_xyb_pack / k_modular_to_xyb.
 *      With the switch in force j40hip_frame_read_xyb(f, 0, out) answers for such a frame after a decode: the three planes X, Y, B
 *      ([3][height][width] floats) by k_modular_to_xyb over the decoded integer planes -- "rnge" where that decode covered part of the
 *      frame only (a region's groups, a partial group range): the planes outside it are not this decode's. ---- */
J40HIP_API uint32_t j40hip_frame_set_modular_xyb(j40hip_frame *f, int mode);
J40HIP_API void j40hip_frame_modular_xyb(const j40hip_frame *f, int32_t out[4]);
/* ---- The colour mode ("Colour space"). The image header's ColourEncoding names white point, primaries
 *      and a transfer function or gamma. The reference reads it and renders every XYB image as sRGB primaries, D65, sRGB curve; so does
 *      this library unless asked. PARITY UNPINNED: the formulas are the standards' (BT.709, BT.2100, SMPTE 428 / 431, sRGB, ST 2084); no
 *      decoder at hand pins libjxl's conventions, above all the HLG inverse OOTF and blending in the signalled space.
 *      set: mode -1 follows the environment (J40HIP_COLOUR=1 serves; the default), 0 renders sRGB, 1 renders an XYB image in the signalled
 *      space: the gamut matrix (Bradford-adapted where the white points differ) folded into the inverse opsin matrix, then the signalled
 *      curve -- linear, sRGB, BT.709, DCI (x^(1/2.6)), gamma, PQ (1.0 = intensity_target nits), HLG (BT.2100's inverse OOTF first) -- and
 *      level = floor(maxpixel * f + 0.5) at the frame's bit depth, reduced to u8 / u16 as ever (k_colour_tail). An image whose encoding is
 *      the sRGB default goes the usual way, byte for byte. Mode 1 is refused with "Ucs?" (the frame is left as it was) for: an image that
 *      wants its ICC profile interpreted, transfer function 2 (unknown), a grey image, custom chromaticities that span nothing, a YCbCr
 *      frame, a Modular frame that does not go through the XYB colour tail (j40hip_frame_set_modular_xyb), an LF-only handle, a handle
 *      built from a view. An image with xyb_encoded = 0 holds samples in its signalled space already: accepted, and nothing changes. The
 *      environment variable alone leaves every such frame as it was. It holds from the next decode on.
 *      Served with the mode in force: both output formats, a region and scale 1 and 2 (through the full-size staging image), the
 *      orientation, kept alpha, the restoration filters (the tail runs on the filtered planes), Modular XYB frames, sequences
 *      (J40HIP_SEQ_COLOUR: the canvas holds pixels in the signalled space). "Ucs?" with the mode in force: a partial group range, a
 *      batch member (j40hip_batch_create), the LF preview -- j40hip_frame_decode_lf, j40hip_frame_decode_lf_to_host and
 *      j40hip_frames_decode_lf alike, whose tail renders sRGB (j40hip_frame_read_lf's float planes are served). A pipeline is not
 *      refused: it renders sRGB whatever the mode or the environment says. j40hip_frame_decode_xyb's planes are not affected.
 *      j40hip_frame_colour: out[0] the rule applies to the frame; out[1] it is in force; out[2] white point, out[3] primaries, out[4]
 *      transfer function (-1 with a gamma), out[5] colour space -- the enums as parsed; out[6] the last decode went through
 *      k_colour_tail (2: and it was an 8-bit frame whose curve has no threshold table -- the linear curve, which is cheaper evaluated,
 *      or a gamma so small that its levels span more buckets than a table holds -- so the curve was evaluated per sample, at the cost
 *      of the deeper frames' path); out[7] what mode 1 would be refused with (0: nothing).
 *      j40hip_frame_colour_encoding: out[0] colour space, [1] white point, [2..3] its xy, [4] primaries, [5..10] their xy (R, G, B),
 *      [11] have_gamma, [12] gamma, [13] transfer function, [14] rendering intent, [15] want_icc. xy and gamma are the stream's
 *      integers (1e-6 and 1e-7 units); an enum's xy are the values it stands for.
 *      After a decode that took the tail without the restoration filters, j40hip_frame_read_xyb (stages 0 and 1) answers with the
 *      planes the tail read. ---- */
J40HIP_API uint32_t j40hip_frame_set_colour(j40hip_frame *f, int mode);
J40HIP_API void j40hip_frame_colour(const j40hip_frame *f, int32_t out[8]);
J40HIP_API void j40hip_frame_colour_encoding(const j40hip_frame *f, int32_t out[16]);
/* host known answers (no device): the gamut matrix of an encoding given as j40hip_frame_colour_encoding states it (`enc`), row-major
 * into p[9], the luminance row into lum[3]; 0 or "Ucs?" */
J40HIP_API uint32_t j40hip_colour_gamut_matrix(const int32_t enc[16], double p[9], double lum[3]);
/* host known answer (no device): the threshold table an 8-bit frame's tail uses for the encoding's curve at intensity_target -- 1794
 * floats into `out` (out_floats: its room): 258 thresholds, then the bucket bytes; range[0..1]: the first and last bucket (a float's top
 * 16 bits). 0, "rnge" (no room), "Ucs?": the curve has no table (its levels span more buckets than the table holds), the tail evaluates it. */
J40HIP_API uint32_t j40hip_colour_table(const int32_t enc[16], float intensity_target, float *out, size_t out_floats, int32_t range[2]);
/* known-answer / measuring hook: k_colour_tail on caller-supplied planes in device memory, enqueued on `stream` and not waited for.
 * xyb_dev: three planes X, Y, B of width x height floats, one behind the other; colour_consts: the 15 floats of
 * j40hip_frame_colour_consts ([0..8] the matrix the tail uses as it stands -- the caller folds the gamut matrix in --, [9..11] the opsin
 * bias, [12] intensity_target); enc: the encoding as above (its curve is taken), lum: the luminance row HLG's OOTF uses; bpp 8..16.
 * table_dev: null, or for bpp 8 what j40hip_colour_table made, in device memory (all 1794 floats), with its range: the tail then takes
 * the table instead of the curve. The image in `format`, stride_bytes a row, rows pixel-aligned. 0, "rnge", "Ufm?", "Ucs?". */
J40HIP_API uint32_t j40hip_kat_device_colour_tail(const float *xyb_dev, int32_t width, int32_t height, const float colour_consts[15], const int32_t enc[16], const float lum[3],
		int32_t bpp, const float *table_dev, const int32_t table_range[2], int32_t format, void *out_dev, size_t stride_bytes, void *stream);
/* known-answer / measuring hook: the Modular XYB kernels on caller-supplied planes in device memory. planes_dev: c0, c1, c2 (width x
 * height samples of sample_bytes 2 or 4 each, tightly packed); alpha_dev: the alpha plane of the same kind, or null; m: the three
 * dequantisation factors; colour_consts: the 15 floats of j40hip_frame_colour_consts (the last two are not used); bpp 8..16.
 * fused_dev: k_modular_xyb_pack's pixels. two_kernel_dev: k_modular_to_xyb into xyb_dev (3 * width * height floats: X, Y, B), then the
 * VarDCT colour tail's kernel over those planes, A from the alpha plane by the pack kernels' rule. Both images in `format`
 * (J40HIP_U8X4 or J40HIP_U16X4), stride_bytes a row, rows pixel-aligned. The call waits for `stream`. 0, "rnge", "Ufm?". */
J40HIP_API uint32_t j40hip_kat_device_modular_xyb(const void *const planes_dev[3], const void *alpha_dev, int32_t sample_bytes, int32_t width, int32_t height, const float m[3], const float colour_consts[15],
		int32_t bpp, int32_t format, void *fused_dev, void *two_kernel_dev, size_t stride_bytes, float *xyb_dev, void *stream);
/* measuring hook (tools/modxyb_probe.py): ONE kernel over caller-supplied device memory, enqueued on `stream` and not waited for.
 * kernel 0: k_modular_xyb_pack (in_dev: the planes c0, c1, c2 as above); 1: k_pack_planes on the same planes; 2: k_xyb_to_rgba (in_dev: three
 * float planes X, Y, B of width x height, sample_bytes ignored; frame_dev: what j40hip_kat_device_colour_frame filled). No alpha plane.
 * j40hip_kat_device_colour_frame: the colour tail's frame constants for k_xyb_to_rgba into frame_dev, device memory of at least
 * `bytes` bytes; returns the bytes it needs, writing nothing when `bytes` is less, or 0 when the copy failed (synchronous). */
J40HIP_API uint32_t j40hip_kat_device_modular_xyb_launch(int32_t kernel, const void *const in_dev[3], int32_t sample_bytes, int32_t width, int32_t height, const float m[3], const float colour_consts[15],
		int32_t bpp, int32_t format, void *out_dev, size_t stride_bytes, const void *frame_dev, void *stream);
J40HIP_API size_t j40hip_kat_device_colour_frame(const float colour_consts[15], int32_t bpp, void *frame_dev, size_t bytes);
/* staged hook: plane c (0 Cb, 1 Y, 2 Cr) of the last decode that went through the YCbCr path, as k_ycbcr_tail read it -- the pixel
 * kernels' samples, or the restoration filters' result where those ran -- tightly packed: width x height floats for a 4:4:4 frame;
 * for a subsampled one the block grid padded to whole MCUs, ((ceil(width / (8 << mh)) << mh) * 8 >> hshift[c]) x (likewise with
 * the vertical shifts) floats. 0, "rnge" without such a decode. */
J40HIP_API uint32_t j40hip_frame_read_ycbcr(j40hip_frame *f, int c, float *out);
/* known-answer / measuring hook: k_ycbcr_tail alone on caller-supplied planes in device memory. plane_dims: {pitch, width, height} of
 * plane 0 (Cb), 1 (Y), 2 (Cr) in floats; shifts: {hshift, vshift} of each (0 or 1); every plane must cover width x height at its
 * resolution. The width x height pixels at out_dev (format J40HIP_U8X4 or J40HIP_U16X4, rows pixel-aligned) are written, nothing
 * else. bpp 8..15: the depth of the 16-bit output's levels. Asynchronous on `stream`. 0, "rnge", "Ufm?". */
J40HIP_API uint32_t j40hip_kat_device_ycbcr_tail(const float *const planes_dev[3], const int32_t plane_dims[9], const int32_t shifts[6], int32_t width, int32_t height, int32_t bpp, int32_t format, void *out_dev, size_t stride_bytes, void *stream);

/* ---- region decode: a rectangle of the frame from the pass groups that cover it ("Region decode"). A pass group is
 *      entropy-coded in a section of its own and no varblock straddles a group, so rectangle (x0, y0, w, h) needs the sections and
 *      varblocks of its COVER only: group columns x0 >> shift .. (x0 + w - 1) >> shift, rows likewise (shift = group_size_shift).
 *      set: any parsed frame, uploaded or not; it holds from the next decode on, across uploads. The rectangle must lie inside the
 *      frame with w, h > 0, else "rnge"; (0, 0, 0, 0) and the full-frame rectangle clear the region (the frame then decodes exactly as
 *      without one). An LF-only frame: "Ulf?". A region and a partial group range (j40hip_frame_set_group_range) exclude each other:
 *      whichever setter comes second returns "Urg?". A refused call leaves the frame as it was. j40hip_batch_create refuses a member
 *      with a region ("Urg?"); pipelines own their frames and never see one.
 *      With a region j40hip_frame_decode / _timed / _decode_to_host write w x h pixels of the frame's format, pixel (i, j) being pixel
 *      (x0 + i, y0 + j) of the whole decode, bit for bit; stride_bytes below 4 * w (u8) or 8 * w (u16) is "rnge" for both formats;
 *      nothing outside the w pixels of each of the h rows is written; j40hip_frame_decode_to_host copies only the region back, keeps the
 *      "evof" retry and never decodes in two phases. Only the cover's sections are entropy-decoded (every pass of them; a Modular
 *      frame's LfGlobal section too) and only the cover's varblocks go through the pixel kernels, so j40hip_frame_status is the verdict
 *      over THOSE sections: damage in a section outside the cover is not seen. A partial cover of a VarDCT frame in drop mode does not
 *      validate the extra channels' sub-images (as with a group range).
 *      Where the work cannot be limited to the cover it is widened to every group, and the rectangle cut out of the whole picture: a
 *      Modular frame with a Squeeze step, a palette with predicted deltas or without one section per group; restoration filters in
 *      force on a frame that signals them; keep-alpha mode. A region is served wherever the whole frame is.
 *      j40hip_frame_region: out[0..3] the rectangle (0, 0, width, height without a region), out[4..7] its cover in groups (first
 *      column, first row, columns, rows), out[8] a region is set, and of the last decode with it: out[9] it was widened to the whole
 *      frame, out[10] the pass-group sections it launched (a Modular frame's LfGlobal section included), out[11] the varblocks its
 *      pixel kernels took (0 for Modular frames). ---- */
J40HIP_API uint32_t j40hip_frame_set_region(j40hip_frame *f, int32_t x0, int32_t y0, int32_t w, int32_t h);
J40HIP_API void j40hip_frame_region(const j40hip_frame *f, int32_t out[12]);

/* ---- reduced-size decode: the whole frame at 1:2 or 1:4, averaged in the pixel kernels ("Reduced-size decode"). A frame has
 *      a scale shift k in {0, 1, 2}, s = 1 << k; the default 0 changes nothing. At k > 0 the decode entry points write ow x oh pixels of
 *      the frame's format, ow = (width + s - 1) >> k, oh = (height + s - 1) >> k. Sample c (each of R, G, B, A on its own) of pixel (i, j)
 *      is (S + (n >> 1)) / n in integers: S the sum of sample c of the FULL decode in the same output format -- what the same handle
 *      writes with k = 0 and every other setting equal (alpha mode, restoration mode, format) -- over the cell x in [i * s, min(width,
 *      (i + 1) * s)), y in [j * s, min(height, (j + 1) * s)), n the cell's pixels (only cells on the right and bottom edges have fewer
 *      than s * s). The mean is taken on coded (sRGB) levels, NOT in linear light: that makes the small image an exact function of
 *      pixels the reference pins. An opaque frame stays A = 255 (65535).
 *      set: any parsed frame, uploaded or not; it holds from the next decode on, across uploads. A shift outside 0..2: "rnge". A shift
 *      above 0 is refused with "Usc?" for a frame with a region or a partial group range and for a handle j40hip_sequence_frame handed
 *      out (other than the main frame of an LF-frame still, see J40HIP_SEQ_LFFRAME, and a full-canvas frame with patches, see J40HIP_SEQ_PATCHES), with "Ulf?" for an LF-only frame; j40hip_frame_set_region and j40hip_frame_set_group_range on a frame with a shift above 0
 *      return "Usc?": whichever setter comes second is refused. A refused call leaves the frame as it was. Shift 0 always succeeds.
 *      At a shift above 0 j40hip_frame_decode / _timed / _decode_to_host write ow x oh pixels; stride_bytes below 4 * ow (u8) or 8 * ow
 *      (u16) is "rnge" before anything is launched; nothing outside the ow pixels of each of the oh rows is written;
 *      j40hip_frame_decode_to_host copies only the small image back, keeps the "evof" retry and never decodes in two phases. Every
 *      section is still entropy-decoded: j40hip_frame_status and every error code are those of the full decode.
 *      Fused: the VarDCT pixel kernels and the Modular pack kernel average their samples as they colour-convert them and store the
 *      small image alone -- no full-size pixel is written. Staged: where other kernels write the pixels -- restoration filters in force
 *      on a frame that signals them, keep-alpha mode on a single frame -- the frame decodes into a full-size image in device memory
 *      kept with the frame (one block of the device memory cache, given back with the frame) and k_downscale reduces it. A scale is
 *      served wherever the whole frame is.
 *      Batches: members must agree on the shift, else "Usc?" where "Uof?" is raised, before any launch; each member gets its own
 *      ow x oh at its own stride; a member in keep-alpha mode at a shift above 0: "Usc?".
 *      j40hip_frame_scale: out[0] the shift in force, out[1], out[2] ow, oh at that shift, and of the last decode at a shift above 0:
 *      out[3] 1 if it went through a full-size staging image, 0 if the kernels wrote the small image directly, -1 if there was none,
 *      out[4] the bytes of staging image it held (0 when fused). ---- */
J40HIP_API uint32_t j40hip_frame_set_scale(j40hip_frame *f, int32_t shift);
J40HIP_API void j40hip_frame_scale(const j40hip_frame *f, int32_t out[5]);
/* known-answer / measuring hook: k_downscale alone (device/scale_kernels.hip). The full w x h image at src_dev made 1:2 (shift 1) or
 * 1:4 (shift 2) at out_dev, format J40HIP_U8X4 or J40HIP_U16X4, all rows pixel-aligned. Asynchronous on `stream`. 0, "rnge" (a shift
 * other than 1 or 2, a stride below the rows' pixels), "Ufm?". */
J40HIP_API uint32_t j40hip_kat_device_downscale(void *out_dev, size_t out_stride, const void *src_dev, size_t src_stride, int32_t w, int32_t h, int32_t shift, int32_t format, void *stream);

/* ---- oriented output: the picture turned as the image metadata's orientation says, by k_orient ("Orientation"). The
 *      codestream stores a W x H frame and an orientation o in 1..8 (the EXIF numbering; 1 where the stream has none). Off by default:
 *      every entry point then writes stored order, as the reference does. Applied, the decode entry points write ow x oh pixels, and
 *      pixel (i, j) is P(x, y), P the image the same handle writes with the mode off and every other setting equal (format, alpha mode,
 *      restoration mode, YCbCr mode, a region, a scale shift), W x H that image's size:
 *        o  ow x oh  (x, y)                      o  ow x oh  (x, y)
 *        1  W x H    (i, j)                      5  H x W    (j, i)
 *        2  W x H    (W - 1 - i, j)              6  H x W    (j, H - 1 - i)
 *        3  W x H    (W - 1 - i, H - 1 - j)      7  H x W    (W - 1 - j, H - 1 - i)
 *        4  W x H    (i, H - 1 - j)              8  H x W    (W - 1 - j, i)
 *      The orientation is applied last: a scaled oriented decode is the oriented small image (not the small image of the oriented
 *      one: the two differ in the edge cells), and a region stays a rectangle in stored coordinates (j40hip_frame_orient_rect maps one).
 *      set: mode -1 follows the environment (J40HIP_ORIENT=1 applies the orientation; the default), 0 is stored order, 1 applies it. Any
 *      parsed frame, uploaded or not; it holds from the next decode on, across uploads. A handle j40hip_sequence_frame handed out refuses
 *      mode 1 with "Uor?" (other than the main frame of an LF-frame still, see J40HIP_SEQ_LFFRAME) and is never oriented by the environment; a refused call leaves the frame as it was.
 *      A partial group range (j40hip_frame_set_group_range: the decode writes that range's rectangles and leaves the rest of the
 *      caller's image alone) and an orientation in force exclude each other, since there is no whole stored-order image to turn:
 *      mode 1 on a frame with a partial range and o other than 1 is "Uor?", j40hip_frame_set_group_range with a partial range on a
 *      frame whose orientation is in force is "Uor?" (whichever comes second), and, because the environment can put an orientation
 *      in force behind a range that was already set, the decode entry points themselves return "Uor?" for the combination before
 *      anything is launched or written.
 *      In force (applied, and o other than 1), j40hip_frame_decode / _timed / _decode_to_host and j40hip_frame_decode_lf /
 *      _decode_lf_to_host (the preview: W x H its (width + 7) / 8 x (height + 7) / 8) decode as ever into a stored-order staging image
 *      of exactly W x H pixels in device memory, kept with the frame (one block of the device memory cache, given back with the frame),
 *      and k_orient writes the caller's ow x oh pixels behind it on the same stream. rgba_dev and stride_bytes need no alignment (as in
 *      stored order; pixels that are not aligned to their size are stored byte by byte); stride_bytes below 4 * ow (u8) or 8 * ow (u16)
 *      is "rnge" before anything is launched; nothing outside the ow pixels of each of the oh rows is written. The three figures of
 *      j40hip_frame_decode_timed are the stored-order decode's stages: k_orient runs behind the last mark and is in none of them. j40hip_frame_decode_to_host copies the oriented image back, keeps the "evof" retry and
 *      never decodes in two phases. Status and error codes are the stored-order decode's. With o = 1 or the mode off nothing is staged
 *      and the path is the stored-order one.
 *      Entries that write stored order only refuse a frame whose orientation is in force with "Uor?": j40hip_batch_create /
 *      j40hip_batch_reset and j40hip_frames_decode_lf. Pipelines and sequences write stored order whatever the environment says.
 *      j40hip_frame_orientation: out[0] the stream's orientation 1..8, out[1] 1 if the next decode applies one other than 1, out[2],
 *      out[3] ow, oh the next decode writes (region and scale counted), out[4] 1 if the last decode went through k_orient, out[5] the
 *      bytes of staging image it held (0 otherwise).
 *      j40hip_frame_orient_rect: rectangle in = {x0, y0, w, h} of the whole frame from displayed (oriented by the stream's o, whatever
 *      the mode) to stored coordinates (to_stored != 0) or back; "rnge" if it does not lie inside the frame it is given in. ---- */
J40HIP_API uint32_t j40hip_frame_set_orientation(j40hip_frame *f, int mode);
J40HIP_API void j40hip_frame_orientation(const j40hip_frame *f, int32_t out[6]);
J40HIP_API uint32_t j40hip_frame_orient_rect(const j40hip_frame *f, int to_stored, const int32_t in[4], int32_t out[4]);
/* known-answer / measuring hook: k_orient alone (device/orient_kernels.hip). The w x h image at src_dev written in `orientation` (1..8;
 * 1 is a plain copy) at out_dev, w x h pixels up to 4 and h x w from 5 on, format J40HIP_U8X4 or J40HIP_U16X4, all rows pixel-aligned.
 * The source must be pixel-aligned (pointer and stride); the output may sit anywhere. Asynchronous on `stream`. 0, "rnge" (an orientation
 * outside 1..8, a stride below the rows' pixels, a source that is not pixel-aligned), "Ufm?". */
J40HIP_API uint32_t j40hip_kat_device_orient(void *out_dev, size_t out_stride, const void *src_dev, size_t src_stride, int32_t w, int32_t h, int32_t orientation, int32_t format, void *stream);

/* After the stream has been synchronised: first failing section in TOC order -> its 4-char code
 * ("coef", "shrt", "excs", "ans?" ...), 0 if every section decoded cleanly (j40.h:530-534). */
J40HIP_API uint32_t j40hip_frame_status(j40hip_frame *f);

/* Convenience for the public API: decode + copy to host rows of `stride_bytes`. Synchronous. */
J40HIP_API uint32_t j40hip_frame_decode_to_host(j40hip_frame *f, void *rgba_host, size_t stride_bytes);
/* How j40hip_frame_decode_to_host last decoded the frame: k > 0 -- in two phases, the k longest pass-group sections on a stream of
 * their own beside the others, the image on its way over the link while they finish (device/runtime.hip; J40HIP_TWO_PHASE=0: never);
 * 0: in one; -1: not decoded to the host since its upload. Same pixels, same codes either way. */
J40HIP_API int32_t j40hip_frame_two_phase_sections(const j40hip_frame *f);

/* The LF preview on the device (device/lf_preview.hip): every cell of the LF image through the LF chroma from luma (X += kx_lf * Y,
 * B += kb_lf * Y: what the reference does to every LLF coefficient, j40.h:7158, 7170) and the full decode's colour tail (XYB ->
 * linear -> sRGB -> level at the image's bit depth, then the 8-bit render or the J40_U16X4 rule, whichever the frame's output format
 * is), alpha opaque, into lf_w x lf_h pixels (j40hip_frame_lf_size) of `stride_bytes` per row. No restoration filter, no upsampling.
 * j40hip_frame_upload of an LF-only frame uploads the LF integers, the LfGroups' geometry and dequantisation factors and the colour
 * constants only; a full frame parsed without flags & 1 gets its LF integers uploaded, into an allocation of its own, at its first
 * preview. Checked before anything is launched: a frame not uploaded or on another device "!gpu", Modular "TODO", stride_bytes below
 * 4 * lf_w (u8) or 8 * lf_w (u16) "rnge". Asynchronous on `stream`. */
J40HIP_API uint32_t j40hip_frame_decode_lf(j40hip_frame *f, void *rgba_dev, size_t stride_bytes, void *stream);
/* ... into host memory, synchronously */
J40HIP_API uint32_t j40hip_frame_decode_lf_to_host(j40hip_frame *f, void *rgba_host, size_t stride_bytes);
/* n uploaded frames, LF-only or full, of one device in ONE launch; rgba_dev[i] / stride_bytes[i] belong to frames[i]. The same checks for
 * every member, and members that disagree on the output format: "Uof?" -- nothing is launched then. */
J40HIP_API uint32_t j40hip_frames_decode_lf(j40hip_frame *const *frames, int64_t n, void *const *rgba_dev, const size_t *stride_bytes, void *stream);
/* parity tests: channel c of the device's dequantised, smoothed LF image (j40hip_frame_lf_plane's layout), by the preview kernel */
J40HIP_API uint32_t j40hip_frame_read_lf(j40hip_frame *f, int c, float *out);

/* Stage dumps for parity tests (device -> host copies, synchronous):
 *   quantised HF coefficients of LF group gg, channel c (f32[w8*h8*64], as j40__hf_coeffs leaves them) */
J40HIP_API uint32_t j40hip_frame_read_coeffs(j40hip_frame *f, int64_t gg, int c, float *out);
/*   int16 sample planes (Modular frames) before packing: channel c, w*h */
J40HIP_API uint32_t j40hip_frame_read_plane_i16(j40hip_frame *f, int c, int16_t *out);
/*   the same of a wide frame (int32 planes); each answers "TODO" for a frame of the other kind */
J40HIP_API uint32_t j40hip_frame_read_plane_i32(j40hip_frame *f, int c, int32_t *out);

/* ---- restoration filters: Gaborish and the edge-preserving filter between the inverse transforms and the colour
 *      conversion, over the whole picture. The reference parses the frame header's RestorationFilter bundle (j40.h:5339-5366) and never
 *      looks at it again -- its j40__gaborish (j40.h:7271) and j40__epf (j40.h:7578) are defined and never called -- so by DEFAULT
 *      nothing runs and the decode matches j40. mode 1 (or J40HIP_RESTORATION=1 in the environment): the filters a VarDCT frame
 *      signals run, stated as those two routines state them (j40_amd/csrc/device/restore_dev.h); mode 2 (J40HIP_RESTORATION=j40):
 *      bit for bit what the routines compute as they stand, including the edge-preserving filter's aliased line buffers (X and Y
 *      read the next channel's rows on half of the lines; the routine only runs at all under an allocator with slack). Their own
 *      complaints -- "gab0", "epf0" (the DEFAULT sharpness table starts with 0: every frame that keeps it), "shrp" -- are reported
 *      behind the sections' codes (j40hip_frame_status) and the picture is then left unfiltered. Single-frame entry points and the
 *      public API; a pipeline decodes such frames on its single-frame path. Modular frames: not filtered (the reference's routines
 *      take float planes only). ---- */
typedef struct {
	int32_t gab_enabled; float gab_weights[3][2];
	int32_t epf_iters; float epf_sharp_lut[8], epf_channel_scale[3], epf_quant_mul, epf_pass0_sigma_scale, epf_pass2_sigma_scale, epf_border_sad_mul, epf_sigma_for_modular;
} j40hip_restoration;
J40HIP_API void j40hip_frame_restoration(const j40hip_frame *f, j40hip_restoration *out);   /* as parsed (mirrors j40__frame_st::gab / ::epf, j40.h:5085-5100) */
J40HIP_API void j40hip_frame_set_restoration(j40hip_frame *f, int mode);                    /* -1: as the environment says (default), 0 off, 1 on, 2 as j40's routines stand */
J40HIP_API int j40hip_frame_sharpness(const j40hip_frame *f, int64_t gg, int16_t *out);     /* LfGroup gg's sharpness map as decoded (i16 w8*h8; j40__lf_group_st::sharpness) */
/* after a decode that ran the filters, stream synchronised: stage 0 the XYB samples as the inverse transforms left them, 1 the filtered
 * ones ([3][height][width] floats); 2 the reciprocal-sigma plane of the edge-preserving filter (w8*h8 floats, < 0: the cell is skipped).
 * Stage 3, after any decode of a frame with patches (J40HIP_SEQ_PATCHES): the planes after k_patch_blend, as the tail read them */
J40HIP_API uint32_t j40hip_frame_read_xyb(j40hip_frame *f, int stage, float *out);
/* Stage 6, after any decode of a frame with splines (J40HIP_PARSE_SPLINES) and without noise: the planes after k_spline_draw, as the tail
 * read them. With noise as well stage 6 answers "rnge" and stage 4 has the planes after both. With patches as well stage 3 answers with the
 * planes between k_patch_blend and k_spline_draw, which such a decode copies before the splines are drawn (with or without noise). */
/* Stage 4, after any decode of a frame with noise (J40HIP_PARSE_NOISE): the planes after k_noise_add, as the tail read them. For a
 * frame with both patches and noise stage 3 answers "rnge": the patched planes are noised in place, what stood between the two is gone.
 * A frame whose LUT is all zeros answers stage 4 with the planes the tail read. */
/* Stage 5, after any decode of an upsampled frame (J40HIP_PARSE_UPSAMPLING): the planes k_upsample wrote, [3][shown height][shown width],
 * as the tail read them. Stages 0 and 1 keep the coded size. */
J40HIP_API float j40hip_frame_restoration_ms(const j40hip_frame *f);   /* device time of the filter kernels in the last decode (J40HIP_RESTORATION_TIMING=1) */
/* known-answer hook: the filter kernels on caller-supplied planes (xyb: [3][h][w] floats, host, in place), a w8*h8 sharpness map and the
 * HfMul reciprocal of the varblock covering each cell; mode 1 or 2; sigma_out optional. 0 or "gab0" / "epf0" / "shrp" / "!gpu". */
J40HIP_API uint32_t j40hip_kat_device_restoration(float *xyb, int32_t w, int32_t h, const int16_t *sharpness, const float *hfmul_inv, const j40hip_restoration *r, int mode, int device, float *sigma_out);

/* per-kernel device time of the last j40hip_frame_decode_timed call, measured with HIP events on
 * the launch stream: ms[0] = entropy decode, ms[1] = coefficients -> pixels, ms[2] = other */
J40HIP_API uint32_t j40hip_frame_decode_timed(j40hip_frame *f, void *rgba_dev, size_t stride_bytes, void *stream, float *ms3);

/* known-answer hook for the renderer's per-sample tail on the device: linear sample -> sRGB transfer -> u8
 * (j40.h:7213-7240, 7925-7935); host arrays in and out */
J40HIP_API uint32_t j40hip_kat_device_srgb_u8(const float *v_host, size_t n, uint8_t *out_host);
/* ... and for the 16-bit output at bit depth bpp (8..15): the level (transfer, conversion, clamp) scaled to u16 as above */
J40HIP_API uint32_t j40hip_kat_device_srgb_u16(const float *v_host, size_t n, int32_t bpp, uint16_t *out_host);

/* ---- batches: throughput mode ----
 * A batch is a set of uploaded VarDCT frames decoded together: ONE entropy launch with one pass-group
 * section per wavefront LANE (64 sections per wavefront, every frame's sections side by side), then the
 * coefficients -> pixels kernels. Frames stay owned by the caller and must outlive the batch; the same
 * frame may also be decoded alone (latency mode: one section per wavefront, scalarised) with
 * j40hip_frame_decode. rgba_dev[i] / stride_bytes[i] belong to frames[i]. Per-frame result:
 * j40hip_frame_status(frames[i]) after the stream has been synchronised. */
typedef struct j40hip_batch j40hip_batch;
J40HIP_API j40hip_batch *j40hip_batch_create(j40hip_frame *const *frames, int64_t n, uint32_t *err);
J40HIP_API void j40hip_batch_free(j40hip_batch *b);
J40HIP_API uint32_t j40hip_batch_decode(j40hip_batch *b, void *const *rgba_dev, const size_t *stride_bytes, void *stream);
/* ms3 as j40hip_frame_decode_timed, for the whole batch */
J40HIP_API uint32_t j40hip_batch_decode_timed(j40hip_batch *b, void *const *rgba_dev, const size_t *stride_bytes, void *stream, float *ms3);
/* asynchronous timed decode: records the stage events in `slot` (0..4095) and returns without waiting, so that
 * batches on different streams overlap (one batch's entropy kernel with another's pixel kernels);
 * j40hip_batch_elapsed reads a slot's ms3 once its stream has been synchronised */
J40HIP_API uint32_t j40hip_batch_decode_recorded(j40hip_batch *b, void *const *rgba_dev, const size_t *stride_bytes, void *stream, int32_t slot);
J40HIP_API uint32_t j40hip_batch_elapsed(j40hip_batch *b, int32_t slot, float *ms3);
/* `stream` waits for stage 1 (cleared), 2 (entropy decoded) or 3 (pixels written) of the decode recorded in `slot` */
J40HIP_API uint32_t j40hip_batch_wait_stage(j40hip_batch *b, int32_t slot, int32_t stage, void *stream);

/* a batch object re-used for other members (keeps its device arrays, streams and events); the previous members' decodes must be complete */
J40HIP_API uint32_t j40hip_batch_reset(j40hip_batch *b, j40hip_frame *const *frames, int64_t n);

/* ---- frame sequences: animations and layered stills ("Several frames"). A codestream whose first frame is not its
 *      last holds several coded frames; each one is placed on the canvas -- the image's width x height -- and the canvas is shown
 *      (duration > 0, or the last frame) and/or saved into one of four reference slots for later frames to draw over. Served: frames
 *      of type 0 and 3 whose blend mode is Replace for the colour channels and every extra channel, with any crop (negative offsets,
 *      beyond the canvas), any source slot, any save_as_reference; animations (have_animation, durations; timecodes skipped) and
 *      layers. Refused with "TODO", reported for the frame it comes from: any other blend mode, frame type 2, frame type 1 and
 *      use_lf_frame (these two unless J40HIP_SEQ_LFFRAME is given, below), and whatever a single frame is refused for.
 *      With J40HIP_SEQ_BLEND (or J40HIP_BLEND=1 in the environment) the blend modes Add, Blend, MulAdd and Mul are served as well,
 *      for the colour channels and for the alpha channel the pixels carry (the first extra channel of type alpha), each with a mode
 *      of its own; the entries of the other extra channels are not looked at, `clamp` is read and changes nothing (a rendered alpha
 *      lies in [0, 1]). The arithmetic works on rendered pixels -- the slots' and the frame's, one float32 operation a step,
 *      INTEGRATION.md "Several frames" states it in full -- so every blended layer rounds once: PARITY UNPINNED against a decoder
 *      that keeps unrounded samples in its slots. Still "TODO" then: a Blend or MulAdd, of the colour channels or of that alpha
 *      channel, whose alpha_chan is another channel; a source slot of any extra channel that differs from the colour channels'
 *      (switch or not, for every entry that carries a slot: a cropped frame's, a full frame's with a mode other than Replace).
 *      A shown or saved canvas, per pixel: inside the frame's rectangle (x0, y0, w, h) clipped to the canvas the frame's pixel;
 *      elsewhere the pixel of slot src_ref_frame, or the empty pixel (0, 0, 0, A0) when that slot was never saved -- A0 = 0 when the
 *      decode renders an alpha channel (a Modular image that has one, a VarDCT image in keep-alpha mode), full scale otherwise. It is
 *      saved into slot save_as_reference when !is_last && (duration == 0 || save_as_reference != 0). Slots hold rendered pixels in
 *      the sequence's output format.
 *      j40hip_sequence_open reads the signature, image header and the header and TOC of every coded frame (`buf` is borrowed until
 *      j40hip_sequence_free; a container's boxes are put together once); no device needed. A stream whose first frame is its last is
 *      not a sequence: NULL and "Usq?" (use j40hip_frame_parse). NULL and the code when the image header or the first frame's header
 *      fails. A later frame whose header or TOC fails, or that is refused, ends the index: it is the last row and carries its code.
 *      flags: bit 0 as j40hip_frame_parse_ex's, applied to every frame handle; bit 1 J40HIP_SEQ_BLEND; J40HIP_PARSE_WIDE (8) as
 *      j40hip_frame_parse_ex's: an image with 32-bit Modular buffers is opened and its Modular frames are served.
 *      With J40HIP_SEQ_LFFRAME (or J40HIP_LFFRAME=1 in the environment) LF frames are served: a frame of type 1 with lf_level L in
 *      1..4 is ceil(image / 8^L) in size, is decoded like any VarDCT frame and never shown nor saved into a reference slot; its three
 *      XYB planes (float32, as the inverse transforms or -- where the restoration mode runs them -- the restoration filters leave them)
 *      are kept in LF slot L - 1. A later frame with use_lf_frame (of level L, 0 for the other types) carries no LfCoefficients
 *      stream: the LF sample of its cell (x8, y8) is sample (x8, y8) of slot L, channel by channel, with no dequantisation factor and
 *      no adaptive smoothing (k_lf_from_frame); its LF indices count the thresholds t with sample > (float) t * mult_lf of that
 *      channel at extra_precision 0 (k_lf_frame_bctx then looks the block contexts up again) -- PARITY UNPINNED, like what an LF
 *      frame stores: the reference refuses such streams. "lfno": the slot was never filled (found at j40hip_sequence_open, it ends the
 *      index); "lfsz": the stored picture is not ceil(w / 8) x ceil(h / 8). A Modular LF frame (the only kind libjxl writes) is served when
 *      J40HIP_SEQ_MODULAR_XYB is given as well: its integer planes are decoded and k_modular_to_xyb makes the slot's three planes of
 *      them (j40hip_frame_set_modular_xyb's rule, PARITY UNPINNED); with the LF switch alone it stays "TODO". Still "TODO" with the
 *      switches: an image that is not XYB encoded or has extra channels, use_lf_frame on a YCbCr or Modular frame. The main frame of such a still (a regular frame
 *      with use_lf_frame that covers the canvas) is the one handle of a sequence that takes j40hip_frame_set_scale and
 *      j40hip_frame_set_orientation, for decodes of its own once the playback has filled its LF slot; the playback refuses it
 *      ("Usc?" / "Uor?") while either is set. j40hip_sequence_rewind unbinds the handles from the slots ("lfno" until played again). Outside a sequence (j40hip_frame_parse*, batches, the pipeline) such
 *      streams stay "TODO", and j40hip_frame_decode_lf of a frame with use_lf_frame is "TODO": the LF frame's own handle decodes
 *      that picture. ---- */
#define J40HIP_SEQ_BLEND 2u   /* j40hip_sequence_open: serve the blend modes Add (1), Blend (2), MulAdd (3) and Mul (4) too */
#define J40HIP_SEQ_LFFRAME 16u   /* j40hip_sequence_open: serve LF frames (type 1) and the frames that take their LF image from one (use_lf_frame) */
/* j40hip_sequence_open: the Modular frames of an XYB image go through the XYB colour tail (j40hip_frame_set_modular_xyb's mode 1 on every
 * handle the rule applies to; J40HIP_MODULAR_XYB=1 in the environment does the same). Together with J40HIP_SEQ_LFFRAME a Modular LF frame
 * is served: k_modular_to_xyb fills its LF slot. With either alone such a frame stays "TODO". */
#define J40HIP_SEQ_MODULAR_XYB 32u
/* j40hip_sequence_open: every handle of the sequence renders in the colour space the image header signals (j40hip_frame_set_colour's mode 1
 * wherever the rule applies and the encoding is not the sRGB default; J40HIP_COLOUR=1 in the environment does the same): the canvas and the
 * reference slots then hold pixels in that space, and the blend modes work on them as they are (PARITY UNPINNED). One canvas holds
 * one colour space: with the flag, an image the mode refuses as a whole (want_icc, transfer function 2, grey) fails j40hip_sequence_open
 * with "Ucs?" (under the environment variable alone such a sequence plays as sRGB, every frame of it); and where the image's frames do
 * render in the signalled space, j40hip_sequence_frame answers "Ucs?" for a frame that cannot -- a Modular frame while
 * J40HIP_SEQ_MODULAR_XYB is off -- instead of composing it as sRGB among them. */
#define J40HIP_SEQ_COLOUR 64u
typedef struct j40hip_sequence j40hip_sequence;
J40HIP_API j40hip_sequence *j40hip_sequence_open(const void *buf, size_t size, int threads, uint32_t flags, uint32_t *err);
J40HIP_API void j40hip_sequence_free(j40hip_sequence *s);
J40HIP_API int64_t j40hip_sequence_num_frames(const j40hip_sequence *s);   /* coded frames (rows of the index) */
J40HIP_API int64_t j40hip_sequence_num_shown(const j40hip_sequence *s);    /* displayed frames */
/* out21: [0..3] x0, y0, w, h of the frame on the canvas, [4] duration in ticks, [5] is_last, [6] shown, [7] type, [8] the colour
 * channels' blend mode, [9] source slot, [10] save_as_reference, [11] whether the canvas is saved, [12] byte offset of the frame
 * header in the codestream and [13] of the end of its last section, [14] of its first section, [15] 0 or the code the frame is refused
 * with ("shrt": the stream ends before the frame does), [16] ticks per second numerator and [17] denominator, [18] loops (0: for
 * ever), [19] canvas width, [20] height. k out of range: zeros. */
J40HIP_API void j40hip_sequence_frame_info(const j40hip_sequence *s, int64_t k, int64_t *out21);
/* How coded frame k goes onto the canvas. out8: [0] the colour channels' blend mode (0 Replace, 1 Add, 2 Blend, 3 MulAdd, 4 Mul),
 * [1] the rendered alpha channel's (0 without one), [2] the colour channels' alpha_chan and [3] clamp, [4] the alpha channel's own
 * alpha_chan and [5] clamp, [6] the source slot, [7] whether the frame goes through k_frame_blend (J40HIP_SEQ_BLEND, a mode other
 * than Replace in [0] or [1], and the frame is not refused). k out of range: zeros. */
J40HIP_API void j40hip_sequence_frame_blend(const j40hip_sequence *s, int64_t k, int32_t *out8);
/* LF frames (J40HIP_SEQ_LFFRAME). out4: [0] the row's lf_level (1..4 for an LF frame, else 0), [1] use_lf_frame, [2] the row it takes
 * its LF image from or -1, [3] 0. k out of range: zeros. */
J40HIP_API void j40hip_sequence_frame_lf(const j40hip_sequence *s, int64_t k, int32_t *out4);
/* debug read-back (synchronises the device): plane c (0 X, 1 Y, 2 B) of LF slot `level` - 1 as the playback last filled it, tightly
 * packed floats of the LF frame's size. "rnge": no such slot, or nothing stored in it since the last rewind. */
J40HIP_API uint32_t j40hip_sequence_read_lf_slot(j40hip_sequence *s, int32_t level, int32_t c, float *out);
/* ---- splines (J40HIP_PARSE_SPLINES above) ----
 * j40hip_frame_splines: has_splines of the frame's header; num_splines, quant_adjust (optional): as parsed.
 * j40hip_frame_spline: spline i as the stream holds it -- start2: its starting point, num_points: its further control points, deltas:
 * up to `cap` of their 2 * num_points double deltas (x and y in turn), coef128: the coefficients [4][32] of X, Y, B and sigma. "rnge": no
 * such spline. j40hip_frame_spline_segments: the number of segments the next decode draws, up to `cap` of them copied to `out` -- 12
 * 4-byte words each: x0, x1, y0, y1 (int32, the box, inclusive), cx, cy, 1 / sigma, sigma * multiplier / 4, colour X, Y, B (float), a pad.
 * j40hip_frame_spline_bins: out2[0] the 64 x 32 tiles the segments touch, out2[1] the (tile, segment) pairs.
 * launches: how often decodes of the handle have launched k_spline_draw. j40hip_frame_spline_ms: with J40HIP_SPLINE_TIMING=1 in the
 * environment the kernel's device time in the last decode, which then waits for it; else 0. */
J40HIP_API int j40hip_frame_splines(const j40hip_frame *f, int32_t *num_splines, int32_t *quant_adjust);
J40HIP_API uint32_t j40hip_frame_spline(const j40hip_frame *f, int64_t i, int64_t *start2, int32_t *num_points, int64_t *deltas, int64_t cap, int32_t *coef128);
J40HIP_API int64_t j40hip_frame_spline_segments(const j40hip_frame *f, void *out, int64_t cap);
J40HIP_API void j40hip_frame_spline_bins(const j40hip_frame *f, int64_t *out2);
J40HIP_API int64_t j40hip_frame_spline_launches(const j40hip_frame *f);
J40HIP_API float j40hip_frame_spline_ms(const j40hip_frame *f);
/* known-answer / measuring hook: k_spline_draw alone. planes_dev: three planes (X, Y, B) of width x height floats, one behind the other,
 * changed in place; segments: n records of 12 words in host memory, in drawing order, every box inside the frame ("rnge": one is not),
 * binned here as the parse bins a frame's. tiles_out (optional): the tiles launched. No segments launch nothing. ms (optional): the
 * kernel's device time. Enqueued on `stream` and waited for. */
J40HIP_API uint32_t j40hip_kat_device_splines(float *planes_dev, int32_t width, int32_t height, const void *segments, int64_t n, int64_t *tiles_out, void *stream, float *ms);
/* ---- photon noise (J40HIP_PARSE_NOISE above) ----
 * j40hip_frame_noise: has_noise of the frame's header; lut8 (optional): the eight NoiseParameters / 1024, seeds2 (optional): the seed
 * counters visible, nonvisible the next decode uses. launches: how often decodes of the handle have launched the two kernels.
 * j40hip_frame_noise_ms: with J40HIP_NOISE_TIMING=1 in the environment the device time of k_noise_fill (ms2[0]) and k_noise_add (ms2[1])
 * in the last decode, which then waits for them; else zeros. */
J40HIP_API int j40hip_frame_noise(const j40hip_frame *f, float *lut8, uint32_t *seeds2);
J40HIP_API int64_t j40hip_frame_noise_launches(const j40hip_frame *f);
J40HIP_API void j40hip_frame_noise_ms(const j40hip_frame *f, float *ms2);
/* known-answer / measuring hook: the two kernels alone. planes_dev: three planes (X, Y, B) of width x height floats, one behind the
 * other, changed in place; group_dim: the side of a group (a multiple of 16, 16..1024); lut8, ytox (base_corr_x), ytob (base_corr_b),
 * visible, nonvisible: as the rule takes them. raw_out_dev (optional): the three raw planes the fill made, width x height floats each,
 * tightly packed. A LUT of zeros launches nothing and leaves raw_out_dev alone. ms2 (optional): the two kernels' device time.
 * Enqueued on `stream` and waited for. "rnge": a size the kernels do not take. */
J40HIP_API uint32_t j40hip_kat_device_noise(float *planes_dev, int32_t width, int32_t height, int32_t group_dim, const float *lut8, float ytox, float ytob,
		uint32_t visible, uint32_t nonvisible, float *raw_out_dev, void *stream, float *ms2);
/* ---- upsampling (J40HIP_PARSE_UPSAMPLING above) ----
 * j40hip_set_upsampling_defaults: the standard's default weights for k = 2, 4 or 8 (n = 15, 55, 210: the upper triangle of the symmetric
 * 5k/2 x 5k/2 matrix, row by row), supplied by the application once; process-wide, behind a mutex; frames parsed afterwards without a
 * custom table for their K copy them; n = 0 takes the table back. "rnge": another k or n.
 * j40hip_frame_upsampling: *k = the frame's upsampling (1, 2, 4, 8); weights (optional, room for 210 floats): the table the frame copied at
 * parse, *n (optional) of them (0 for k = 1). j40hip_frame_coded_size: the size the frame is coded at (j40hip_frame_info has the shown one).
 * j40hip_frame_upsample_ms: with J40HIP_UPSAMPLE_TIMING=1 in the environment the device time of k_upsample in the last decode, which then
 * waits for it; else 0. */
J40HIP_API uint32_t j40hip_set_upsampling_defaults(int k, const float *w, int n);
J40HIP_API uint32_t j40hip_frame_upsampling(const j40hip_frame *f, int32_t *k, float *weights, int32_t *n);
J40HIP_API void j40hip_frame_coded_size(const j40hip_frame *f, int32_t *width, int32_t *height);
J40HIP_API float j40hip_frame_upsample_ms(const j40hip_frame *f);
/* known-answer / measuring hooks. j40hip_kat_upsampling_kernel: the expanded table [k][k][25] of the 15 / 55 / 210 weights --
 * out[(oy * k + ox) * 25 + 5 * sy + sx]: what output phase (ox, oy) gives the coded sample at (sx - 2, sy - 2).
 * j40hip_kat_device_upsample: k_upsample alone. planes_dev: three planes of width x height floats, one behind the other; out_dev: three of
 * out_w x out_h (out_w <= k * width, out_h <= k * height: the cut). ms (optional): the kernel's device time. Enqueued on `stream` and waited
 * for. j40hip_kat_host_upsample: the same functions compiled for the CPU over host memory; tiled = 0 the rule sample by sample, 1 the
 * kernel's tile functions thread by thread. "rnge": a factor or a size they do not take. */
J40HIP_API uint32_t j40hip_kat_upsampling_kernel(int32_t k, const float *weights, float *out);
J40HIP_API uint32_t j40hip_kat_device_upsample(const float *planes_dev, int32_t width, int32_t height, int32_t k, const float *weights, int32_t out_w, int32_t out_h, float *out_dev, void *stream, float *ms);
J40HIP_API uint32_t j40hip_kat_host_upsample(const float *planes, int32_t width, int32_t height, int32_t k, const float *weights, int32_t out_w, int32_t out_h, float *out, int tiled);
/* ---- patches: reference-only frames and the patch dictionary. PARITY UNPINNED: the reference holds no code for either (j40.h:6262 is a
 *      TODO); off by default. With J40HIP_SEQ_PATCHES (or J40HIP_PATCHES=1 in the environment) a sequence takes
 *      - a reference-only frame (type 2) with save_before_colour_transform = 1 of an image with xyb_encoded = 1: a frame of its own width
 *        and height, without an origin, never shown. Its three float32 planes X, Y, B -- what the inverse transforms (and, where they are
 *        in force, the restoration filters) leave of it -- are stored in reference slot save_as_reference; a Modular one needs
 *        J40HIP_SEQ_MODULAR_XYB as well. A slot holds such planes or saved pixels, whichever the playback put there last. Type 2 with
 *        save_before_colour_transform = 0, with patches of its own, or in an image with xyb_encoded = 0 stays "TODO";
 *      - a frame with has_patches: the patch dictionary at the head of its LfGlobal names rectangles of those slots and where they go
 *        onto the frame's own XYB samples, in dictionary order, in blend mode None (0), Replace (1), Add (2) or Mul (3; with clamp the
 *        source is clamped to [0, 1]) -- one float32 operation per sample and channel (k_patch_blend), after the restoration filters and
 *        before the colour tail. A dictionary with a mode that uses alpha (4..7), or with an extra channel's entry other than None, is "TODO".
 *      "ptch": a dictionary that is damaged -- a mode above 7, a slot above 3, a rectangle that leaves its reference frame, a placement
 *      that is negative or leaves the frame, more reference patches than 1024 + pixels / 4 (or four times as many placements). "ptno": a
 *      slot that no reference-only frame has filled when the frame is reached. Both are found when the index is built (the row's code).
 *      A frame with patches decodes whole frames at full size: a region or a scale is cut from the full-size picture, a group range, a
 *      batch, a pipeline and the LF preview of such a frame are "TODO". Without the flag every stream is taken or refused as before. ---- */
#define J40HIP_SEQ_PATCHES 128u
/* out8: [0] has_patches, [1] the dictionary's reference patches, [2] its placements, [3] the slots they read (bit k: slot k), [4] whether
 * the row is a reference-only frame stored as XYB planes, [5] the slot it is stored in (-1: none), [6] the tiles of the frame that a
 * placement other than None touches (k_patch_blend's workgroups; 0: it is not launched), [7] how often the decodes of the row's handle
 * have launched k_patch_blend. k out of range: zeros. */
J40HIP_API void j40hip_sequence_frame_patches(const j40hip_sequence *s, int64_t k, int32_t *out8);
/* placement i (dictionary order) of coded frame k as parsed. out10: [0..1] x, y on the frame, [2..3] width, height, [4..5] x0, y0 in the
 * reference frame, [6] the slot, [7] the colour channels' mode, [8] clamp, [9] which reference patch it places. "rnge": no such placement. */
J40HIP_API uint32_t j40hip_sequence_frame_patch(const j40hip_sequence *s, int64_t k, int64_t i, int32_t *out10);
/* debug read-back: the size of the planes in reference slot `slot` as the playback last filled it, and (synchronises the device) plane c
 * (0 X, 1 Y, 2 B) of it, tightly packed floats. "rnge": no such slot, or it holds no reference-only frame since the last rewind. */
J40HIP_API uint32_t j40hip_sequence_ref_slot_size(j40hip_sequence *s, int32_t slot, int32_t *width, int32_t *height);
J40HIP_API uint32_t j40hip_sequence_read_ref_slot(j40hip_sequence *s, int32_t slot, int32_t c, float *out);
/* known-answer / measuring hook: k_patch_blend alone. planes_dev: three planes (X, Y, B) of width x height floats, one behind the other,
 * changed in place; slot_dev[k]: the three planes of slot k, slot_w[k] x slot_h[k] floats each (null: empty); placements: count times
 * nine integers x, y, w, h, x0, y0, slot, mode, clamp, in dictionary order. The list is checked ("ptch", "ptno") and binned on the host;
 * tiles_out (optional): the workgroups launched. Enqueued on `stream` and waited for. */
J40HIP_API uint32_t j40hip_kat_device_patches(float *planes_dev, int32_t width, int32_t height, const float *const slot_dev[4], const int32_t slot_w[4], const int32_t slot_h[4],
		const int32_t *placements, int32_t count, int32_t *tiles_out, void *stream);
/* Coded frame k, fully parsed at the first call: an ordinary frame handle of the frame's own (crop) size over a copy of the frame's
 * own bytes, owned by the sequence (do not free it). Every single-frame and batch entry point takes it -- upload, decode, region,
 * LF preview, alpha mode, status. NULL and the code for a frame that is refused or does not parse. */
J40HIP_API j40hip_frame *j40hip_sequence_frame(j40hip_sequence *s, int64_t k, uint32_t *err);
/* parses and uploads every coded frame to `device` (its own bytes each, not the whole file) and takes the device memory of the
 * playback: every slot the index saves into and one staging image large enough for each cropped frame. A frame that does not parse
 * ends the index there, as a refused one does at j40hip_sequence_open: it becomes the last row and carries its code, the frames
 * before it play. Returns the code of a frame that fails to upload, "!gpu" when the device is out of memory. */
J40HIP_API uint32_t j40hip_sequence_upload(j40hip_sequence *s, int device);
/* J40HIP_U8X4 or J40HIP_U16X4 for every frame and the canvas; "Ufm?" otherwise; "Uof?" once the playback has begun (rewind first).
 * After an upload a change takes the slots and the staging image again and may wait for the device. */
J40HIP_API uint32_t j40hip_sequence_set_output_format(j40hip_sequence *s, int32_t format);
/* Decodes the coded frames up to and including the next displayed one and leaves that frame's canvas in rgba_dev: canvas-sized, rows
 * of stride_bytes (at least 4 or 8 bytes a pixel, else "rnge"), pixel-aligned. Frames that are saved are composed in their slot --
 * where that slot is also the source (out == src for the compose kernel) only the rectangle is written -- and copied out when they
 * are shown; up to four canvas-sized slots and one staging image come from the device memory cache at j40hip_sequence_upload and go
 * back at j40hip_sequence_free. A frame that covers the canvas exactly decodes straight into its destination -- unless it has a blend
 * mode other than Replace: such a frame, whatever it covers, decodes into the staging image and goes through k_frame_blend. Everything is enqueued
 * on `stream`; nothing is waited for and no memory is taken (frames in keep-alpha mode synchronise as j40hip_frame_decode does). Returns 0; "Useq" when no
 * displayed frame is left; the code of a frame that is refused or fails to upload ("!gpu": not uploaded). Section failures surface
 * in j40hip_sequence_status once the stream has been synchronised. */
J40HIP_API uint32_t j40hip_sequence_next(j40hip_sequence *s, void *rgba_dev, size_t stride_bytes, void *stream);
/* ... into host memory, synchronously, every coded frame's status checked as it is decoded (an "evof" frame is decoded again with
 * dense planes): 0, "Useq", or the failing frame's code -- the canvas is then not written */
J40HIP_API uint32_t j40hip_sequence_next_to_host(j40hip_sequence *s, void *rgba_host, size_t stride_bytes);
J40HIP_API void j40hip_sequence_rewind(j40hip_sequence *s);   /* the next j40hip_sequence_next starts over at frame 0 with no slot saved */
/* After the stream has been synchronised: the first failing section over the frames decoded since the last rewind, frame by frame in
 * order -> its code, and in *out_frame (optional) which coded frame; 0 and -1 when all of them decoded cleanly */
J40HIP_API uint32_t j40hip_sequence_status(j40hip_sequence *s, int64_t *out_frame);
/* known-answer / measuring hook: k_frame_compose alone (device/compose_kernels.hip). The frame image frame_dev (w x h pixels, its
 * pixel (0, 0) at canvas pixel (x0, y0)) onto the W x H canvas at out_dev; outside the rectangle the pixels of src_dev or, src_dev
 * NULL, the empty pixel whose bytes are empty_lo (u8x4) or empty_lo, empty_hi (u16x4) as little-endian words. out_dev == src_dev (and
 * equal strides): only the rectangle is written. All rows pixel-aligned. Asynchronous on `stream`. 0, "rnge", "Ufm?". */
J40HIP_API uint32_t j40hip_kat_device_compose(void *out_dev, size_t out_stride, const void *src_dev, size_t src_stride, const void *frame_dev, size_t frame_stride,
		int32_t W, int32_t H, int32_t x0, int32_t y0, int32_t w, int32_t h, uint32_t empty_lo, uint32_t empty_hi, int32_t format, void *stream);

/* ... and k_frame_blend alone: the same arguments and checks, then the colour channels' and the alpha channel's blend mode (0..4,
 * else "rnge"). Inside the rectangle the canvas pixel is the blend of the frame's pixel over src_dev's (or the empty pixel);
 * out_dev == src_dev blends in place. */
J40HIP_API uint32_t j40hip_kat_device_blend(void *out_dev, size_t out_stride, const void *src_dev, size_t src_stride, const void *frame_dev, size_t frame_stride,
		int32_t W, int32_t H, int32_t x0, int32_t y0, int32_t w, int32_t h, uint32_t empty_lo, uint32_t empty_hi, int32_t format, int32_t colour_mode, int32_t alpha_mode, void *stream);

/* ---- building blocks for pipelines ---- */
/* j40hip_frame_upload with the copies enqueued on `stream` (the plan is staged in pinned memory owned by the calling thread, so the
 * copy is a real asynchronous DMA beside other streams' kernels); returns when they have completed */
J40HIP_API uint32_t j40hip_frame_upload_on(j40hip_frame *f, int device, void *stream);
/* frees the calling thread's pinned staging buffer (call before a thread that uploaded frames exits) */
J40HIP_API void j40hip_thread_release(void);
/* Takes the library's process-wide state down: stops and joins its service threads, frees the cached device memory, pooled events
 * and cached tables. Optional (a process may simply end); nothing of the library may be running, and objects created before must
 * have been freed. The library can be used again afterwards. */
J40HIP_API void j40hip_shutdown(void);
/* j40hip_frame_status in two halves: `begin` enqueues the copy of the status words on `stream`, `end` -- once the caller has waited
 * for that stream -- reduces them to the frame's verdict without touching the device. VarDCT frames without extra channels. */
J40HIP_API uint32_t j40hip_frame_status_begin(j40hip_frame *f, void *stream);
J40HIP_API uint32_t j40hip_frame_status_end(j40hip_frame *f);
/* the caller guarantees that nothing is pending on the frame's device memory: j40hip_frame_free then skips its device-wide wait */
J40HIP_API void j40hip_frame_mark_idle(j40hip_frame *f);

/* ---- whole-frame throughput pipeline (j40_amd/csrc/device/pipeline.hip): codestreams in host memory -> RGBA u8x4, every stage of
 *      many frames in flight. `host_threads` workers parse what precedes the LfGroup sections of a frame and copy it to the device
 *      without waiting for it; one thread enqueues, per batch of `batch_frames` frames, the LfGroup streams, the plan build, the
 *      entropy decode and the pixel kernels on the batch's stream, up to `max_in_flight` batches on their own streams; host output
 *      is copied back on the batch's stream behind its kernels. Frames outside that path (Modular, one section, extra channels)
 *      are decoded by a worker through the single-frame entry points. The serving shape of j40_from_memory + j40_next_frame +
 *      j40_frame_pixels_u8x4 for many images. ---- */
typedef struct j40hip_pipeline j40hip_pipeline;
/* host_threads < 1: the container's CPU quota (cgroup cpu.max) less two, at most 16 -- never the visible CPU count. Keep the busy threads
 * of the process below its quota: a cgroup that runs into it throttles every thread of the process, the HIP runtime's included, and
 * the copies back to the host then crawl. With the LfGroup streams on the GPU a frame's host stage is 1-2 ms: two to four threads. */
J40HIP_API j40hip_pipeline *j40hip_pipeline_create(int device, int host_threads, int batch_frames, int max_in_flight, uint32_t *err);
/* flags bits 0-1: who decodes the LfGroup streams (j40.h:6722-6790) of the batched frames: 0 decided frame by frame (the host
 * threads keep them while the device has batches queued up, else the device takes them), 1 always the device (k_lf_groups),
 * 2 always the host threads. Bit 2: tune the process's malloc for many threads freeing multi-megabyte blocks (mallopt: mmap
 * threshold, trim threshold, top pad) -- process-wide, hence opt-in. Bit 3: do not size the device memory cache for the pipeline's full
 * depth at its second full batch (a serving pipeline whose batches fill up only now and then). */
J40HIP_API j40hip_pipeline *j40hip_pipeline_create_ex(int device, int host_threads, int batch_frames, int max_in_flight, uint32_t flags, uint32_t *err);
J40HIP_API int64_t j40hip_pipeline_lf_device_frames(j40hip_pipeline *p);   /* frames whose LfGroup streams the device decoded (since the last reset) */
J40HIP_API void j40hip_pipeline_free(j40hip_pipeline *p);
/* frames still queued when the pipeline is freed are dropped; frames already prepared or in flight are decoded first */
/* queues one image. buf is borrowed until the ticket is done. rgba: `stride_bytes` * height bytes of host memory (pinned memory for
 * full copy speed) or, with device_output != 0, of device memory (no copy back). */
J40HIP_API uint32_t j40hip_pipeline_submit(j40hip_pipeline *p, const void *buf, size_t size, void *rgba, size_t stride_bytes, int device_output, int64_t *ticket);
/* One image, synchronously: queued like a submitted one, the calling thread sleeps until it is done; returns 0 or the image's 4-char
 * code. The pixel memory is asked for through `alloc` once the image's size is known (called once, on a pipeline thread, before
 * anything is written; it returns host memory -- pinned for full copy speed -- of *stride_bytes * height bytes, *stride_bytes >=
 * 4 * width, or NULL: "!mem"). Any number of threads may call this at once: their images share the pipeline's batches. This is what
 * j40_next_frame (include/j40.h) runs on when several threads are inside the public API at once. */
typedef void *(*j40hip_output_alloc)(void *ctx, int64_t width, int64_t height, size_t *stride_bytes);
J40HIP_API uint32_t j40hip_pipeline_run(j40hip_pipeline *p, const void *buf, size_t size, j40hip_output_alloc alloc, void *ctx);
/* The scale shift (0, 1, 2: j40hip_frame_set_scale) of every image submitted afterwards: the caller's rgba / stride_bytes and the
 * width and height j40hip_output_alloc is asked for are then the small image's, and so are the device images, the copies back and a
 * device_output image. "rnge" for a shift outside 0..2, "Usc?" for another shift than the one in force while images are in flight (drain first). */
J40HIP_API uint32_t j40hip_pipeline_set_scale(j40hip_pipeline *p, int32_t shift);
/* > 0: a prepared image waits at most `ms` for its batch to fill up while the device has a free batch slot (serving: images arrive
 * one by one); 0 (default): a partial batch is launched only when nothing else is queued */
J40HIP_API void j40hip_pipeline_set_max_wait_ms(j40hip_pipeline *p, double ms);
/* waits until everything submitted so far is done */
J40HIP_API uint32_t j40hip_pipeline_drain(j40hip_pipeline *p);
/* 0 or the image's 4-char error code, as j40_error would give it ("rnge" for an unknown or unfinished ticket) */
J40HIP_API uint32_t j40hip_pipeline_result(j40hip_pipeline *p, int64_t ticket);
/* out8: [0] ms the worker threads spent in the host stage of batched frames and [1] in whole single-frame decodes (summed over the
 * threads), [2] images completed, [3] ms from first submit to last completion, [4] entropy-stage and [5] pixel-stage ms summed over
 * the batch launches (HIP events on their streams), [6] batch launches, [7] images in them */
J40HIP_API void j40hip_pipeline_stats(j40hip_pipeline *p, double *out8);
/* out12: as above, then [8] ms of the batches' first stage (LfGroup streams + plan build + LfGroup tail), [9] images whose LfGroup
 * streams the device decoded, [10] images decoded on the single-frame path, [11] ms of k_hf_lanes itself summed over the launches,
 * as the device recorded them (first wavefront's start to last one's end: the duration rocprofv3 reports; [4] also counts what the
 * launch waited for behind other kernels) */
J40HIP_API void j40hip_pipeline_stats_ex(j40hip_pipeline *p, double *out12);
/* out5: the launches of the LfGroup lane decoder (k_lf_rows / k_lf_lanes; j40__lf_group's two Modular streams, j40.h:6722-6790) since
 * the last reset: [0] their durations summed, ms, as the device recorded them (first wavefront's start to last one's end), [1]
 * launches, [2] frames, [3] LfGroup sections and [4] wavefronts in them */
J40HIP_API void j40hip_pipeline_lf_stats(j40hip_pipeline *p, double *out5);
J40HIP_API void j40hip_pipeline_reset_stats(j40hip_pipeline *p);

/* The SDMA engine the pipeline's copies back to host memory go to on `device` (hsa_amd_memory_async_copy_on_engine; -1: none, the
 * copies are hipMemcpyAsync). An MI355X has sixteen engines of very different device-to-host rates (57 ... 7 GB/s) and hipMemcpyAsync
 * takes whichever is free; the library measures them once per process and device (32 MB each, at its first pipeline or at this call)
 * and keeps the fastest. gbps16 (optional): the measured GB/s per engine, 0 = not measured, < 0 = failed; masks2 (optional, THREE
 * words): the runtime's masks {free, recommended} for the direction and the engines set aside for the worker threads' uploads (an
 * SDMA engine works on one copy at a time: an upload sharing the engine of the copies back waits behind 133 MB transfers). J40HIP_COPY_ENGINE=hip: never; =<n>: engine n, unmeasured. */
J40HIP_API int j40hip_copy_engine(int device, double *gbps16, uint32_t *masks2);

/* ---- stage dump of the pipeline's DEVICE stages, for parity tests (tests/test_device_stages.py): one image goes through the same
 *      enqueue a batch of one takes -- front parse on the host; the LfGroup streams on the device (k_lf_lanes) when `lf_on_device`
 *      and the frame's tables allow it, else by the host decoder; plan build (k_plan_place / _scan / _emit), LfGroup tail, entropy
 *      decode, pixel kernels, verdict -- and what every stage produced is copied back and handed out in the layout of the reference's
 *      j40__lf_group_st (j40.h:6360-6390), like the j40hip_frame_lf_group_* accessors do for the host parse. NULL + "TODO" for
 *      images the batched path does not take. ---- */
typedef struct j40hip_stage_dump j40hip_stage_dump;
J40HIP_API j40hip_stage_dump *j40hip_stage_dump_create(const void *buf, size_t size, int device, int lf_on_device, uint32_t *err);
J40HIP_API void j40hip_stage_dump_free(j40hip_stage_dump *d);
/* out8: [0] the frame's verdict (k_plan_verdict: 0 or the first failing section's 4-char code, LfGroup and pass-group sections alike),
 * [1] flags: bit 0 an LfGroup section the device decoder leaves to the host, bit 1 an event region overflowed, bit 2 the LfGroup
 * streams were decoded on the device, [2] LfGroups, [3] groups, [4] width, [5] height, [6] union of the DctSelect values placed, [7] varblocks */
J40HIP_API void j40hip_stage_dump_info(const j40hip_stage_dump *d, uint32_t *out8);
/* out10: left, top, width, height, width8, height8, width64, height64, varblocks placed, the section's status (4-char code or 0) */
J40HIP_API int j40hip_stage_dump_lf_group_info(const j40hip_stage_dump *d, int64_t gg, int32_t *out10);
/* which: 0 blocks (i32 w8*h8, the reference's encoding, rebuilt from the device's varblock records), 1 lfindices (u8 w8*h8, from the
 * decoded LF integers with the frame's thresholds, j40.h:6566-6570), 2 xfromy / 3 bfromy (i16 w64*h64), 4 sharpness (i16 w8*h8; only
 * when the device decoded the streams), 5 / 6 / 7 the raw LF integers of X / Y / B (i16 w8*h8) */
J40HIP_API int j40hip_stage_dump_plane(const j40hip_stage_dump *d, int64_t gg, int which, void *out);
/* varblocks in placement order (= the reference's varblock index): coeffoff_qfidx, hfmul.inv, and (optional) x8, y8, DctSelect; returns how many */
J40HIP_API int j40hip_stage_dump_varblocks(const j40hip_stage_dump *d, int64_t gg, int32_t *coeffoff_qfidx, float *hfmul_inv, int32_t *x8_y8_dctsel);
J40HIP_API int j40hip_stage_dump_llf(const j40hip_stage_dump *d, int64_t gg, int c, float *out);
/* the entropy kernel's block list of one group (frame-wide group index), in j40__hf_coeffs' visiting order: per block
 * coeffoff_qfidx, pos_dct (y8 * 32 + x8 inside the group | DctSelect << 10), bctx3 (block context of Y | X << 4 | B << 8); returns the count */
J40HIP_API int64_t j40hip_stage_dump_group_blocks(const j40hip_stage_dump *d, int64_t group, uint32_t *out3, int64_t capacity);
/* the pixel kernels' work list (sorted by DctSelect; class_start28[27] = varblocks): out8 = px, py, effw, effh, dctsel, blk, llf_base,
 * coeff_base; out3 = mult1, kx_hf, kb_hf; returns the count */
J40HIP_API int64_t j40hip_stage_dump_sorted_varblocks(const j40hip_stage_dump *d, int32_t *out8, float *out3, int32_t *class_start28, int64_t capacity);
J40HIP_API int j40hip_stage_dump_rgba(const j40hip_stage_dump *d, uint8_t *out);   /* width * 4 bytes per row */

#ifdef __cplusplus
}
#endif
#endif
