// j40_amd/csrc/frame.hpp -- host-side parse of everything in front of the per-group hot path:
// container, image metadata, frame header, TOC, LfGlobal, HfGlobal/HfPass and the LfGroup sections
// (LF image, varblock layout, LLF coefficients). Produces the tables the HIP kernels consume.
//
// Reference behaviour (all host-only rows of SURVEY.md section 2): j40__container (j40.h:1479),
// j40__image_metadata (3104), j40__frame_header (5163), j40__read_toc (5479), j40__lf_global (6257),
// j40__lf_group (6722), j40__hf_global (6819), j40__load_dq_matrix (4828), j40__natural_order (4980).
#pragma once
#include "modular.hpp"
#include "device/spline_dev.h"
#include <algorithm>
#include <array>

namespace j40hip {

// J40HIP_API_TIMING=1: the single-image path prints where its time goes (parse, upload, decode); read once
inline bool api_timing() { static const bool v = env_str("J40HIP_API_TIMING") != nullptr; return v; }

// J40HIP_ALPHA=1: VarDCT frames keep their alpha channel where j40hip_frame_set_alpha(f, 1) would be taken (include/j40hip.h); read once
inline bool alpha_env() { static const bool v = [] { const char *e = env_str("J40HIP_ALPHA"); return e && atoi(e) > 0; }(); return v; }

// J40HIP_ORIENT=1: single-frame decodes apply the image's orientation where j40hip_frame_set_orientation(f, 1) would be taken (include/j40hip.h); read once
inline bool orient_env() { static const bool v = [] { const char *e = env_str("J40HIP_ORIENT"); return e && atoi(e) > 0; }(); return v; }
// J40HIP_YCBCR=1: YCbCr VarDCT frames (recompressed JPEGs) are served where j40hip_frame_set_ycbcr(f, 1) would be taken (include/j40hip.h); read once
inline bool noise_env() { return env_on("J40HIP_NOISE", false); }   // (read at every parse)
inline bool splines_env() { return env_on("J40HIP_SPLINES", false); }   // J40HIP_SPLINES=1: every parse asks for splines (J40HIP_PARSE_SPLINES); read at every parse
inline bool upsampling_env() { return env_on("J40HIP_UPSAMPLING", false); }   // J40HIP_UPSAMPLING=1: every parse asks for upsampling (J40HIP_PARSE_UPSAMPLING); read at every parse
inline bool wide_env() { static const bool v = [] { const char *e = env_str("J40HIP_WIDE"); return e && atoi(e) > 0; }(); return v; }
inline bool modular_xyb_env() { static const bool v = [] { const char *e = env_str("J40HIP_MODULAR_XYB"); return e && atoi(e) > 0; }(); return v; }
// J40HIP_RESTORATION: 0 off (the default), 1 the filters a frame signals, 2 (`j40`) as j40's routines stand; read once
inline int restoration_env() { static const int v = [] { const char *e = env_str("J40HIP_RESTORATION"); return !e ? 0 : !strcmp(e, "j40") ? 2 : atoi(e) > 0 ? 1 : 0; }(); return v; }
inline bool ycbcr_env() { static const bool v = [] { const char *e = env_str("J40HIP_YCBCR"); return e && atoi(e) > 0; }(); return v; }

struct ExtraChannel { int32_t type = 0, bpp = 8, exp_bits = 0, dim_shift = 0; bool alpha_associated = false; };
enum { EC_ALPHA = 0, EC_SPOT = 2, EC_BLACK = 4, EC_CFA = 5 };

// J40HIP_COLOUR=1: XYB images are rendered in the colour space their header signals where j40hip_frame_set_colour(f, 1) would be taken (include/j40hip.h); read once
inline bool colour_env() { static const bool v = [] { const char *e = env_str("J40HIP_COLOUR"); return e && atoi(e) > 0; }(); return v; }

// ColourEncoding as the stream states it (the defaults: what all_default means -- RGB, D65, sRGB primaries, sRGB transfer, relative intent).
// The reference reads it and drops it; the colour mode (j40hip_frame_set_colour, colour_space.hpp) renders XYB images by it. Custom xy:
// the stream's integers, 1e6 to the unit; filled in for the enums too
struct ColourEncoding {
	int32_t colour_space = 0;                  // 0 RGB, 1 grey, 2 XYB, 3 unknown
	int32_t white_point = 1;                   // 1 D65, 2 custom, 10 E, 11 DCI
	int32_t white_xy[2] = {312700, 329000};
	int32_t primaries = 1;                     // 1 sRGB, 2 custom, 9 BT.2100, 11 P3
	int32_t prim_xy[3][2] = {{640000, 330000}, {300000, 600000}, {150000, 60000}};
	bool have_gamma = false;
	int32_t gamma = 0;                         // with have_gamma: the exponent times 1e7
	int32_t transfer = 13;                     // else: 1 BT.709, 2 unknown, 8 linear, 13 sRGB, 16 PQ, 17 DCI, 18 HLG
	int32_t intent = 1;
	bool srgb_default() const {   // what today's tail renders: nothing for the colour mode to do
		return colour_space == 0 && white_point == 1 && primaries == 1 && !have_gamma && transfer == 13;
	}
};

struct ImageMeta {
	ColourEncoding cenc;
	int32_t width = 0, height = 0;
	int32_t bpp = 8, exp_bits = 0;
	int32_t orientation = 1;   // 1..8, the EXIF numbering (the stream holds orientation - 1 in its extra fields; 1 where it has none)
	bool have_animation = false, anim_have_timecodes = false;
	int32_t anim_tps_num = 0, anim_tps_den = 0; int64_t anim_loops = 0;   // ticks per second as a fraction, repetitions (0: for ever); with have_animation
	bool modular_16bit_buffers = true;
	std::vector<ExtraChannel> ec;
	bool xyb_encoded = true, want_icc = false, grey = false;
	float intensity_target = 255.0f;
	float opsin_inv_mat[3][3];
	float opsin_bias[3];
	float quant_bias[3];
	float quant_bias_num = 0.145f;
	// custom upsampling weights (read with the upsampling switch only, else a non-zero mask is "TODO"): bit 0 of cw_mask: up_weights[0] holds
	// the 15 up2_weight, bit 1: [1] the 55 up4_weight, bit 2: [2] the 210 up8_weight, each as its F16 reads (device/upsample_dev.h)
	int32_t cw_mask = 0;
	std::vector<float> up_weights[3];
};

struct FrameHeader {
	bool is_last = true;
	int32_t type = 0;
	int32_t lf_level = 0;   // 1..4 for an LF frame (type 1), whose size is the image's divided by 8 that many times, rounding up; else 0
	bool is_modular = false;
	bool has_noise = false, has_patches = false, has_splines = false, use_lf_frame = false, skip_adapt_lf_smooth = false;
	bool do_ycbcr = false;
	int32_t jpeg_upsampling = 0;
	// what jpeg_upsampling says of the channels in coded order (slot 0 Cb, 1 Y, 2 Cr): log2 of how much coarser than the finest channel
	// each is sampled, per axis (0 or 1). PARITY UNPINNED (the reference refuses such frames, j40.h:6749): mode (v >> 2c) & 3 of channel c
	// means the sampling factors (h, v) = (1, 1), (2, 2), (2, 1), (1, 2); shift = log2(largest factor / the channel's)
	int8_t hshift[3] = {0, 0, 0}, vshift[3] = {0, 0, 0};
	bool subsampled() const { return hshift[0] | hshift[1] | hshift[2] | vshift[0] | vshift[1] | vshift[2]; }
	// the layouts that are served: luma at full resolution, the two chroma channels alike (4:4:4, 4:2:0, 4:2:2, 4:4:0). jpeg_upsampling can
	// say others -- Y coarser than chroma, Cb and Cr differing --; nothing here was ever made or tested with them, they stay "TODO"
	bool layout_served() const { return !hshift[1] && !vshift[1] && hshift[0] == hshift[2] && vshift[0] == vshift[2]; }
	int32_t max_hshift() const { return std::max<int32_t>(hshift[0], std::max(hshift[1], hshift[2])); }
	int32_t max_vshift() const { return std::max<int32_t>(vshift[0], std::max(vshift[1], vshift[2])); }
	int32_t group_size_shift = 8;
	int32_t x_qm_scale = 3, b_qm_scale = 2;
	int32_t num_passes = 1;
	int32_t x0 = 0, y0 = 0, width = 0, height = 0;
	// Upsampling (read with the upsampling switch only, else anything but 1 is "TODO"; device/upsample_dev.h has the rule): upsampling = K,
	// 1, 2, 4 or 8. width and height above are the CODED size, ceil(shown / K) -- what groups, LF groups, the TOC, varblocks, Modular
	// channels and the filters work on --; up_width and up_height the SHOWN size, what the header states and a decode writes. K = 1: the
	// two agree (a header that was not parsed, a plan view's, has up_width = 0: shown_width() answers for both).
	// WHICH SIZE A READER WANTS: whatever works on coded samples -- groups, sections, varblocks, LF cells, Modular channels, the filters,
	// the planes ahead of k_upsample -- reads width and height (coded_width() says so out loud); whatever speaks of the picture -- the
	// output, its staging images, the region, the scale, the orientation, the tails -- reads shown_width() and shown_height().
	int32_t upsampling = 1, up_width = 0, up_height = 0;
	std::vector<int32_t> ec_upsampling;   // every extra channel's
	int32_t shown_width() const { return up_width > 0 ? up_width : width; }
	int32_t shown_height() const { return up_height > 0 ? up_height : height; }
	int32_t coded_width() const { return width; }
	int32_t coded_height() const { return height; }
	// how the frame goes onto the canvas (j40.h:5297-5336). The reference reads these and drops them; frame sequences (capi.hpp: j40hip_sequence) keep them
	struct Blend { int8_t mode = 0, alpha_chan = 0, clamp = 0, src_ref = 0; };
	Blend blend;                          // the colour channels'
	std::vector<Blend> ec_blend;          // every extra channel's
	bool full_frame = true;               // the frame covers the canvas
	int64_t duration = 0;                 // ticks (animations)
	int32_t save_as_ref = 0;
	bool save_before_ct = false;
	int32_t grows = 0, gcolumns = 0, ggrows = 0, ggcolumns = 0;
	int64_t num_groups = 0, num_lf_groups = 0;
	// RestorationFilter as the reference parses it (defaults j40.h:5196-5208, fields j40.h:5339-5366). The reference reads it and never
	// looks at it again; here it is kept for the restoration filters (device/restore_dev.h), which run only when asked for.
	struct Restoration {
		bool gab = true;
		float gab_weights[3][2] = {{0.115169525f, 0.061248592f}, {0.115169525f, 0.061248592f}, {0.115169525f, 0.061248592f}};
		int32_t epf_iters = 2;
		float sharp_lut[8] = {0.0f / 7.0f, 1.0f / 7.0f, 2.0f / 7.0f, 3.0f / 7.0f, 4.0f / 7.0f, 5.0f / 7.0f, 6.0f / 7.0f, 7.0f / 7.0f};
		float channel_scale[3] = {40.0f, 5.0f, 3.5f};
		float quant_mul = 0.46f, pass0_sigma_scale = 0.9f, pass2_sigma_scale = 6.5f, border_sad_mul = 2.0f / 3.0f, sigma_for_modular = 1.0f;
	} restoration;
};

struct Section { size_t offset = 0, size = 0; };  // byte range inside the codestream

// The patch dictionary at the head of LfGlobal (a frame with has_patches; read with Frame::allow_patches only). PARITY UNPINNED: the
// reference holds no code for it (j40.h:6262). A placement puts the w x h samples at (sx, sy) of the reference-only frame in slot `ref`
// onto the frame's XYB samples at (x, y), in the colour channels' blend mode (0 None, 1 Replace, 2 Add, 3 Mul; 4..7 use alpha)
struct PatchPlacement { int32_t x, y, w, h, sx, sy, ref, mode, clamp, source; };   // source: which reference patch of the dictionary it places
struct PatchDictionary {
	int32_t num_ref = 0;                        // reference patches
	std::vector<PatchPlacement> placements;     // flat, in dictionary order
	uint32_t slots = 0;                         // bit k: a placement reads slot k
	bool unserved = false;                      // a mode 4..7, or an extra channel's entry other than None: parsed, "TODO"
};

struct Toc {
	bool single = false;
	Section single_section;               // when the frame has exactly one section: readable to the end of the codestream like in the
	                                      // reference, which reads such a frame from its main state (no section boundary) ...
	size_t single_declared_end = 0;       // ... and compares where it ended with the TOC entry afterwards (j40__end_of_frame, j40.h:7796)
	Section lf_global, hf_global;
	size_t first_offset = 0;              // where the first stored section starts
	std::vector<Section> lf_groups;       // [num_lf_groups]
	std::vector<Section> pass_groups;     // [num_passes * num_groups], pass-major
	size_t end_offset = 0;
	size_t lf_end = 0;                    // the largest end of LfGlobal and the LfGroup sections as the TOC states them (before clipping);
	                                      // single-section frames: the codestream's size
};

struct DqMatrix {
	int32_t mode = 0;                     // 0 library, 7 raw, else the coded parameter form
	int32_t n = 0, m = 0;
	std::vector<std::array<float, 3>> params;
	bool loaded = false;                  // expanded to one weight per coefficient
};

struct VarblockInfo { int32_t coeffoff_qfidx; float hfmul_inv; int32_t x8, y8, dctsel; };

struct LfGroup {
	int32_t idx = 0, left = 0, top = 0, width = 0, height = 0, width8 = 0, height8 = 0, width64 = 0, height64 = 0;
	std::vector<int32_t> blocks;          // [height8 * width8]: (dctsel + 2) << 20 | varblock, 1 << 20 | varblock
	std::vector<uint8_t> lfindices;       // [height8 * width8]
	std::vector<VarblockInfo> varblocks;
	std::vector<float> llfcoeffs[3];      // [height8 * width8], indexed by coefficient offset / 64
	std::vector<int16_t> xfromy, bfromy;  // [height64 * width64]
	std::vector<int16_t> sharpness;       // [height8 * width8], as decoded (the reference's j40__lf_group_st::sharpness; read by the edge-preserving filter only)
	bool loaded = false;
	// Frame::defer_lf_tail: the quantised LF samples as decoded (channel order X, Y, B) and their dequantisation factors; the
	// dequantisation, the adaptive smoothing and the LLF coefficients (`llfcoeffs`) are then computed on the device at upload
	// (finish_lf_tail does the same on the host when somebody asks for llfcoeffs)
	std::vector<int16_t> lfraw[3];
	float mult_lf[3] = {0.0f, 0.0f, 0.0f};
	bool tail_pending = false;
};

// One LfGroup section handed to a device decoder (Frame::lf_decoder; device/lf_decode.hip): the host has read what precedes the
// LF coefficient stream; the decoder fills in the results (plane pointers stay valid until its next call on the same thread).
struct LfDeviceTask {
	size_t byte_off = 0, size = 0; uint32_t bit_off = 0;
	int32_t w8 = 0, h8 = 0, w64 = 0, h64 = 0, sidx0 = 0, sidx2 = 0, nbvb_bits = 0;
	uint32_t status = 0;          // 0, the stream's 4-char error, or 'lffb': decode this section on the host
	int32_t nb_varblocks = 0;
	const int16_t *lf[3] = {nullptr, nullptr, nullptr};   // streamed order Y, X, B
	const int16_t *xfromy = nullptr, *bfromy = nullptr, *info0 = nullptr, *info1 = nullptr, *sharp = nullptr;
};
// the streams of one LfGroup section as decoded (read_lf_group_raw): LF integers in streamed order Y, X, B; chroma-from-luma
// maps; the varblock-info channel (two rows of nb_varblocks: DctSelect, HfMul - 1); the sharpness map.
struct LfRaw {
	int32_t extra_prec = 0, nb_varblocks = 0;
	std::vector<int16_t> lf[3], xfromy, bfromy, info, sharp;
};
struct Frame;
// returns false when it cannot take the frame (tree / code spec outside what the kernel handles, no device): host path
typedef bool (*LfDeviceDecoder)(void *ctx, const Frame &f, const uint8_t *cs, size_t cs_size, std::vector<LfDeviceTask> &tasks);

struct Frame {
	ImageMeta im;
	FrameHeader fh;
	Toc toc;

	// LfGlobal
	float m_lf_scaled[3] = {1.0f / 4096.0f, 1.0f / 512.0f, 1.0f / 256.0f};
	int32_t global_scale = 0, quant_lf = 0;
	int32_t lf_thr[3][15], qf_thr[15];
	int32_t nb_lf_thr[3] = {0, 0, 0}, nb_qf_thr = 0;
	std::vector<uint8_t> block_ctx_map;
	int32_t nb_block_ctx = 0;
	float inv_colour_factor = 1.0f / 84.0f, base_corr_x = 0.0f, base_corr_b = 1.0f;
	int32_t x_factor_lf = 0, b_factor_lf = 0;
	std::vector<TreeNode> global_tree;
	CodeSpec global_codespec;
	Modular gmodular;                     // frame-sized Modular image (Modular frames, extra channels)
	int32_t num_gm_channels = 0;          // channels already decoded inside LfGlobal
	// where the not-yet-decoded global Modular pixel data would start is irrelevant: it is decoded here

	// HfGlobal / HfPass
	DqMatrix dq_matrix[17];
	int32_t num_hf_presets = 0;
	std::vector<int32_t> order_lehmer[11][13][3];
	bool order_has_lehmer[11][13][3];
	std::vector<int32_t> orders[11][13][3];   // expanded coefficient orders (only those in use)
	CodeSpec coeff_codespec[11];
	uint32_t dct_select_used = 0, order_used = 0;

	std::vector<LfGroup> lf_groups;
	size_t single_pass_group_bitpos = 0;
	// VarDCT frames: leave the tail of every LfGroup (dequantisation, adaptive smoothing, LLF coefficients; j40.h:6544-6590, 6492, 5944)
	// to the device: the host keeps the decoded integers (LfGroup::lfraw). Set before parse_frame.
	bool defer_lf_tail = false;
	// VarDCT frames with several sections: the LfGroup streams are decoded by this (on the device) instead of the host. Set before parse_frame.
	LfDeviceDecoder lf_decoder = nullptr; void *lf_decoder_ctx = nullptr;
	bool lf_decoded_on_device = false;   // out: it was
	// Streaming input (the reference's refillable source, j40.h:1220-1386, 1676-1812): the codestream's bytes arrive
	// while it is parsed. need_bytes(ctx, n) returns once bytes [0, n) of the buffer are there (or the source has ended: what is
	// missing then reads as a truncated stream). parse_frame asks before it touches anything: the headers on growing prefixes, then
	// LfGlobal, HfGlobal and every LfGroup section as their bytes are due -- the pass-group sections, most of the file, are not the
	// host's to read. nullptr: everything is there. Set before parse_frame; called from the LfGroup worker threads too.
	void (*need_bytes)(void *ctx, size_t upto) = nullptr; void *need_ctx = nullptr;
	size_t (*have_bytes)(void *ctx) = nullptr;   // how many bytes are there now (with need_bytes)
	void need(size_t upto) const { if (need_bytes) need_bytes(need_ctx, upto); }
	// The LF preview (J40HIP_PARSE_LF_ONLY): headers, TOC, LfGlobal and the LfGroup sections only -- HfGlobal and the pass groups are
	// never read nor asked for (frames with several sections; a single section is read whole). VarDCT frames only. Set before parse_frame.
	bool lf_only = false;
	// A member of a frame sequence (capi.hpp: j40hip_sequence): the bytes handed to parse_frame start at this frame's header, byte aligned, and the
	// image metadata is this one instead of a parsed one. Frames that are not last, and frames of type 3, are taken; what a sequence
	// does not serve (sequence_refusal) is "TODO". Set before parse_frame.
	const ImageMeta *seq_im = nullptr;
	bool seq_blend = false;   // ... and the sequence serves the blend modes other than Replace (J40HIP_SEQ_BLEND)
	// YCbCr frames are asked for (J40HIP_PARSE_YCBCR or J40HIP_YCBCR=1): a frame with subsampled channels is parsed -- its block grid padded
	// to whole MCUs, every LF channel at its own size -- instead of refused with "TODO" before its LF image is read. Set before parse_frame.
	bool allow_ycbcr = false;
	// Wide Modular frames are asked for (J40HIP_PARSE_WIDE or J40HIP_WIDE=1): an image whose metadata says modular_16bit_buffers = 0 is parsed
	// instead of refused with "fm32" (j40.h:3169), and a Modular frame of it is decoded with int32 sample planes. A VarDCT frame of such an
	// image is "TODO". Set before parse_frame.
	bool allow_wide = false;
	// LF frames are asked for (a sequence opened with J40HIP_SEQ_LFFRAME or J40HIP_LFFRAME=1): a sequence's member of type 1 is taken, and
	// a frame with use_lf_frame is parsed -- its LfGroup sections start at nb_varblocks, its LF integers and LF indices stay zero (the
	// device fills both in from the LF frame's picture, device/lf_tail_kernels.hip) -- instead of refused with "TODO". Set before parse_frame.
	bool allow_lf_frame = false;
	// ... and Modular LF frames among them (the sequence also renders Modular frames of XYB images through the XYB colour tail,
	// J40HIP_SEQ_MODULAR_XYB or J40HIP_MODULAR_XYB=1: k_modular_to_xyb fills the LF slot). Set before parse_frame.
	bool allow_modular_lf = false;
	// Patches are asked for (a sequence opened with J40HIP_SEQ_PATCHES or J40HIP_PATCHES=1): a sequence's member of type 2 is taken, and a
	// frame with has_patches is parsed -- its dictionary into `patches` -- instead of refused with "TODO". Set before parse_frame.
	bool allow_patches = false;
	bool allow_modular_ref = false;   // ... and Modular reference-only frames among them (the sequence has the Modular XYB switch too)
	PatchDictionary patches;
	// Photon noise is asked for (J40HIP_PARSE_NOISE, or J40HIP_NOISE=1): a frame with has_noise is parsed -- its eight NoiseParameters
	// into noise_lut, each u(10) / 1024 -- instead of refused with "TODO"; the frame must be a regular or skip-progressive one (type 0
	// or 3) of an image with xyb_encoded = 1. Set before parse_frame. (device/noise_dev.h has the rule.)
	bool allow_noise = false;
	float noise_lut[8] = {0, 0, 0, 0, 0, 0, 0, 0};
	// Upsampling is asked for (J40HIP_PARSE_UPSAMPLING, or J40HIP_UPSAMPLING=1): custom weights in the image header and a frame header with
	// upsampling > 1 are parsed instead of refused with "TODO". up_table: the 15 / 55 / 210 weights of the frame's K, copied at parse from
	// the stream's custom table for that K, else from the process-wide defaults (set_upsampling_defaults); neither: "updf". Empty for K = 1.
	bool allow_upsampling = false;
	std::vector<float> up_table;
	// Splines are asked for (J40HIP_PARSE_SPLINES, or J40HIP_SPLINES=1): a frame with has_splines is parsed -- its quantised splines into
	// `splines`, behind the patch dictionary and ahead of the noise parameters; the segments every decode draws and their tiles into
	// `spline_plan` once LfGlobal's base correlations are known -- instead of refused with "TODO"; the frame must be a regular or
	// skip-progressive one (type 0 or 3) of an image with xyb_encoded = 1. A damaged stream is "spln". Set before
	// parse_frame. (device/spline_dev.h has the rule.)
	bool allow_splines = false;
	SplineData splines;
	SplinePlan spline_plan;
	bool wide() const { return !im.modular_16bit_buffers; }
	// A fresh Frame with the fields a caller sets BEFORE parse_frame -- the ones declared above, from defer_lf_tail on -- and nothing
	// else (the streaming header parse starts over with one when the prefix it had ran out). A field added to that set goes in here.
	Frame with_same_inputs() const {
		Frame g;
		g.defer_lf_tail = defer_lf_tail; g.lf_decoder = lf_decoder; g.lf_decoder_ctx = lf_decoder_ctx;
		g.need_bytes = need_bytes; g.need_ctx = need_ctx; g.have_bytes = have_bytes;
		g.lf_only = lf_only; g.seq_im = seq_im; g.seq_blend = seq_blend; g.allow_ycbcr = allow_ycbcr; g.allow_wide = allow_wide; g.allow_lf_frame = allow_lf_frame; g.allow_modular_lf = allow_modular_lf;
		g.allow_patches = allow_patches; g.allow_modular_ref = allow_modular_ref; g.allow_noise = allow_noise; g.allow_splines = allow_splines; g.allow_upsampling = allow_upsampling;
		return g;
	}
	// Modular frames: LfGlobal's channel data is left to the device; it starts at this bit of the section
	bool gm_data_pending = false;
	size_t gm_data_bitpos = 0;  // single-section VarDCT frames: where the pass group starts
};

// locates the codestream inside `data` (bare codestream or ISOBMFF container); if the codestream is
// split over several boxes it is reassembled into `storage`
// stray_tail (optional): 1..7 when that many bytes follow the last box of a container -- too few for a box header
void extract_codestream(const uint8_t *data, size_t size, const uint8_t **cs, size_t *cs_size, std::vector<uint8_t> *storage, int *stray_tail = nullptr);

// signature, image metadata and ICC profile of a codestream: everything in front of the first frame header. *first_frame: the byte
// the first frame header starts at
void parse_image_header(const uint8_t *cs, size_t cs_size, ImageMeta *im, size_t *first_frame, bool allow_wide = false, bool allow_upsampling = false);
// The standard's default upsampling weights, which nothing here holds: the application supplies them once (j40hip_set_upsampling_defaults).
// Process-wide, behind a mutex. set: false for a k other than 2, 4, 8 or an n other than 15, 55, 210; get: false while none were supplied
bool set_upsampling_defaults(int32_t k, const float *w, int32_t n);
bool get_upsampling_defaults(int32_t k, std::vector<float> *out);
// header and TOC of the frame that starts at byte `offset` of the codestream, for a sequence's index: nothing behind the TOC is
// read. The TOC's offsets count from `offset`. Raises what the header or the TOC raise, "TODO" for what sequence_refusal refuses.
// blend: the sequence serves the blend modes other than Replace, lf_frames: and LF frames (sequence_refusal).
// patches: and reference-only frames (type 2), modular_ref: Modular ones among them.
void parse_sequence_frame_header(const uint8_t *cs, size_t cs_size, size_t offset, const ImageMeta &im, bool blend, bool lf_frames, FrameHeader *fh, Toc *toc, bool modular_lf = false, bool patches = false, bool modular_ref = false);
// the patch dictionary of a frame with has_patches (`im`: its image's metadata, the size is the frame's own). Raises "shrt", the entropy
// code's errors and "ptch"; a dictionary that parses but is not served comes back with `unserved` set
void read_patch_dictionary(BitReader &br, const ImageMeta &im, const FrameHeader &fh, PatchDictionary *out);
void read_splines(BitReader &br, const FrameHeader &fh, SplineData *out);
void parse_sequence_splines(const uint8_t *cs, size_t cs_size, size_t offset, const ImageMeta &im, const FrameHeader &fh, const Toc &toc, bool allow_patches, bool allow_noise);
// ... of the frame whose header starts at byte `offset` of the codestream and whose TOC (offsets from `offset`) is `toc`, for a sequence's index
void parse_sequence_patches(const uint8_t *cs, size_t cs_size, size_t offset, const ImageMeta &im, const FrameHeader &fh, const Toc &toc, PatchDictionary *out);
// the extra channel whose samples become the pixels' A (plan_build.cpp: alpha_channel): the first one of type alpha; -1: none
int32_t rendered_alpha_channel(const ImageMeta &im);
// 0, or "TODO": the frame is of a kind a sequence does not serve -- types 1 and 2, use_lf_frame, and a blend mode other than Replace
// in any channel. With `blend` the other four modes are served for the colour channels and for extra channel `alpha_ec` (the rendered
// alpha, -1: none; the other extra channels' entries are not looked at), unless a Blend or MulAdd of either names another alpha
// channel than `alpha_ec`. With `lf_frames` type 1 and use_lf_frame pass, unless the LF frame is a Modular one and `modular_lf` is not
// set (without the Modular XYB switch nothing renders Modular samples to XYB floats) or of an image with extra channels, the image is not XYB encoded (`xyb`), or the frame with use_lf_frame is a
// YCbCr or Modular one
// With `patches` a reference-only frame (type 2) passes where it is saved before the colour transform, of an XYB image, has no patches of
// its own and is a VarDCT frame or `modular_ref` is set.
uint32_t sequence_refusal(const FrameHeader &fh, bool blend, int32_t alpha_ec, bool lf_frames = false, bool xyb = true, bool modular_lf = false, bool patches = false, bool modular_ref = false);

// parses headers, TOC, LfGlobal, HfGlobal and every LfGroup section. `threads` > 1 decodes LfGroup
// sections concurrently (they are independent given LfGlobal)
void parse_frame(const uint8_t *cs, size_t cs_size, Frame *f, int threads);
// the pipeline's host stage (see frame.cpp)
bool parse_frame_front(const uint8_t *cs, size_t cs_size, Frame *f, std::vector<LfDeviceTask> *tasks, std::vector<int32_t> *extra_prec, bool *plain);
void read_lf_group_raw(BitReader &br, const Frame &f, const LfGroup &gg, LfRaw *out);
// the LfGroup tail on the host for the groups that still have it pending (dequantise, smooth, LLF): what the device does at upload
void finish_lf_tail(Frame *f);
// channel c (X, Y, B) of the LF image over the frame: the dequantised, smoothed sample of every 8x8 cell, ceil(width / 8) x
// ceil(height / 8) floats row by row -- what the LLF coefficients are made of. Returns false when the frame holds no LF integers.
bool lf_plane(const Frame &f, int c, float *out);

// 0 when the single-frame decode serves this YCbCr VarDCT frame once it is asked to (j40hip_frame_set_ycbcr), else "TODO"
uint32_t ycbcr_scope(const Frame &f);

struct GroupInfo { int32_t ggidx, gx_in_gg, gy_in_gg, gw, gh; };
GroupInfo group_info(const FrameHeader &fh, int64_t gidx);  // j40.h:7734

struct DctSelect { int8_t log_rows, log_columns, param_idx, order_idx; };
extern const DctSelect DCT_SELECT[27];
extern const int8_t LOG_ORDER_SIZE[13][2];

void natural_order(int32_t log_rows, int32_t log_columns, std::vector<int32_t> *out);
void load_dq_matrix(int32_t idx, DqMatrix *dq);
void forward_dct2d_scaled_for_llf(float *buf, float *scratch, int32_t log_rows, int32_t log_columns);

} // namespace j40hip
