// j40_amd/csrc/capi.hpp -- the object behind the opaque j40hip_frame handle
#pragma once
#include "../../include/j40hip.h"
#include "frame.hpp"
#include "plan_build.hpp"
#include "colour_space.hpp"
#include "device/patch_dev.h"
#include <memory>

struct j40hip_device_state;  // defined in device/runtime_state.hpp

// What the last decode of a handle did, for j40hip_frame_status, the getters and the read-back hooks. A decode begins with a fresh one, so
// a field added here is reset with the rest. (What the getters report "of the last decode with a region / scale / orientation" outlives
// the decodes without one and stays on the handle.)
struct LastDecode {
	bool alpha_written = false;       // merged the alpha channel into its pixels
	bool ycbcr_used = false;          // went through the YCbCr planes and k_ycbcr_tail
	bool wide_used = false;           // ran the int32 instantiations of the Modular kernels (a wide frame, j40hip_frame_wide)
	bool modular_xyb_used = false;    // went through k_modular_xyb_pack / k_modular_to_xyb
	bool modular_xyb_whole = false;   // ... and decoded every group: the planes hold the whole frame (j40hip_frame_read_xyb)
	bool colour_used = false;         // went through k_colour_tail
	bool colour_curve_8bit = false;   // ... of an 8-bit frame without a threshold table: the curve was evaluated per sample (the linear curve, or one whose levels no table holds)
	int restore_ran = 0;              // the mode the restoration filters ran in (0: they did not)
	uint32_t restore_err = 0;         // their "gab0" / "epf0" / "shrp" (reported behind the sections' codes)
	bool trailers_pending = false;    // decoded by a batch: j40hip_frame_status validates the extra channels' sub-images before it reports
	const float *tail_planes = nullptr;   // the three XYB planes the tail read, after the filters and the patches (j40hip_frame_read_xyb); device memory of the upload
	const float *coded_planes = nullptr;  // an upsampled frame: the coded planes k_upsample read (tail_planes are the shown-size ones it wrote); else null
	// the upload's device state is released: nothing of it is named or reported any longer
	const float *patched_planes = nullptr;   // a frame with patches and splines: a copy of the planes between k_patch_blend and k_spline_draw (stage 3); else null
	void device_released() { restore_ran = 0; restore_err = 0; trailers_pending = false; tail_planes = nullptr; coded_planes = nullptr; patched_planes = nullptr; }
};

struct j40hip_frame {
	const uint8_t *cs = nullptr;     // codestream bytes (inside the caller's buffer, or cs_storage)
	size_t cs_size = 0;
	std::vector<uint8_t> cs_storage;
	bool bare_codestream = false;    // the input was the codestream itself, no container around it
	bool from_view = false;          // built by j40hip_frame_from_vardct_view: no global MA tree / code spec, so the extra channels'
	                                 // sub-images behind the coefficients cannot be validated (runtime.hip: validate_trailers)
	int container_stray_tail = 0;    // container input: 1..7 bytes behind the last box (not enough for a box header)
	j40hip::Frame frame;
	j40hip_device_state *dev = nullptr;
	bool force_dense = false;        // upload with dense coefficient planes (set after a decode ran out of event space, ERR_EVOF)
	int restoration = -1;            // the restoration filters (j40hip_frame_set_restoration): -1 as J40HIP_RESTORATION says, 0 off, 1 on, 2 as j40's routines stand
	int alpha = -1;                  // the alpha channel of a VarDCT frame (j40hip_frame_set_alpha): -1 as J40HIP_ALPHA says, 0 dropped (A = 255, the reference's pixels), 1 kept
	int ycbcr = -1;                  // YCbCr VarDCT frames (j40hip_frame_set_ycbcr): -1 as J40HIP_YCBCR says, 0 refused ("TODO", the reference's answer), 1 served
	// Modular frames of XYB images (j40hip_frame_set_modular_xyb): -1 as J40HIP_MODULAR_XYB says, 0 rendered as R, G, B (the reference's pixels), 1 through
	// the XYB colour tail
	int modular_xyb = -1;
	// the colour mode (j40hip_frame_set_colour): -1 as J40HIP_COLOUR says, 0 every XYB image rendered as sRGB (the reference's pixels), 1 in the
	// colour space the image header signals
	int colour = -1;
	LastDecode last;                 // what the last decode did: every decode begins with last = LastDecode()
	int32_t output_format = J40HIP_U8X4;   // what the decode entry points write (j40hip_frame_set_output_format): u8x4 or u16x4
	// region decode (j40hip_frame_set_region): the rectangle the decode entry points write instead of the whole frame, and what the last
	// decode with it cost (j40hip_frame_region's fields 9-11)
	bool region_set = false;
	int32_t region[4] = {0, 0, 0, 0};                              // x0, y0, w, h
	int32_t region_widened = 0, region_sections = 0, region_varblocks = 0;
	bool partial_range = false;      // j40hip_frame_set_group_range narrowed the uploaded frame to some of its groups (what the setters know of the upload)
	// reduced-size decode (j40hip_frame_set_scale): the scale shift the decode entry points write at (0: full size, 1: 1:2, 2: 1:4), and of
	// the last decode at a shift above 0 whether it went through a full-size staging image and how large that was (j40hip_frame_scale)
	int32_t scale = 0, scale_staged = -1;
	int64_t scale_staging_bytes = 0;
	bool from_sequence = false;      // handed out by j40hip_sequence_frame: the playback owns its size (no scale, no orientation)
	// oriented output (j40hip_frame_set_orientation): -1 as J40HIP_ORIENT says, 0 stored order, 1 the image's orientation applied; and of
	// the last decode whether it went through k_orient and the bytes of stored-order staging image it held (j40hip_frame_orientation)
	int orient = -1;
	int32_t orient_applied = 0;
	int64_t orient_staging_bytes = 0;
	// a frame with use_lf_frame (a sequence with J40HIP_SEQ_LFFRAME): the LF frame's picture its next decodes take their LF samples from --
	// three device planes of float32 (X, Y, B), lf_src_w x lf_src_h tightly packed, bound by the playback (j40hip_frame_bind_lf_source);
	// null: nothing bound, such a frame's decode is "lfno"
	const float *lf_src[3] = {nullptr, nullptr, nullptr};
	int32_t lf_src_w = 0, lf_src_h = 0;
	// a frame with patches (a sequence with J40HIP_SEQ_PATCHES): the reference slots its next decodes read -- per slot the three device
	// planes (X, Y, B) of a reference-only frame, w x h floats each, one behind the other, bound by the playback (j40hip_frame_bind_patch_source);
	// null: nothing bound, a decode that reads the slot is "ptno". patch_launches: how often a decode of this handle has launched k_patch_blend
	struct PatchSource { const float *base = nullptr; int32_t w = 0, h = 0; } patch_src[4];
	int64_t patch_launches = 0;
	// a frame with noise (J40HIP_PARSE_NOISE): the seed counters its decodes use -- a sequence's index counts them (Row::noise_seeds), a
	// stand-alone handle has zeros; noise_launches: how often a decode of this handle has launched k_noise_fill and k_noise_add
	uint32_t noise_seeds[2] = {0, 0};
	int64_t noise_launches = 0;
	// a frame with splines (J40HIP_PARSE_SPLINES): how often a decode of this handle has launched k_spline_draw
	int64_t spline_launches = 0;
	std::shared_ptr<const j40hip::PatchPlan> patch_plan;   // the placements as records and their tiles, as the sequence's index made them (null: no dictionary)
	int threads = 1;                 // what the frame was parsed with: the plan build at upload may use as many (plan_build.cpp)
	// backing storage of the plan views (include/j40hip.h)
	struct Views {
		std::vector<std::vector<j40hip_cluster_view>> clusters;
		std::vector<j40hip_codespec_view> specs;
		std::vector<j40hip::CodeSpec> host_specs;
		std::vector<j40hip_lf_group_view> lf_groups;
		std::vector<j40hip_section_view> sections;
		std::vector<std::vector<float>> dq;
		std::vector<j40hip_tree_node> tree;
		std::vector<int32_t> ch_w, ch_h, ch_meta;
		std::vector<j40hip_transform_view> transforms;
		std::vector<j40hip_modular_section_view> mod_sections;
		std::vector<int32_t> local_rct, sub_w, sub_h, sub_meta, chan_rects;
		std::vector<j40hip_transform_view> sub_transforms;
		std::vector<std::vector<int32_t>> vb_coeffoff_qfidx;
		std::vector<std::vector<float>> vb_hfmul_inv;
	} views;
};

// the object behind j40hip_sequence (include/j40hip.h): the index over the coded frames of one codestream and, once asked for, their
// frame handles. The device half (canvas slots, staging image, where the playback stands) lives in device/runtime_seq.hip.
struct j40hip_sequence_device;
struct j40hip_sequence {
	const uint8_t *cs = nullptr;     // the codestream (inside the caller's buffer, or cs_storage: a container's boxes put together once)
	size_t cs_size = 0;
	std::vector<uint8_t> cs_storage;
	j40hip::ImageMeta im;
	struct Row {
		j40hip::FrameHeader fh;
		size_t offset = 0, end = 0, first_section = 0;   // bytes of the codestream: the frame header, the end of the last section, the first section
		uint32_t code = 0;           // what the frame is refused with; nothing behind such a frame is known
		bool shown = false, saved = false;
		// blend modes (J40HIP_SEQ_BLEND): the rendered alpha channel's mode, the one source slot of the entries that carry one, and
		// whether the frame goes through k_frame_blend (a mode other than Replace in the colour channels or the rendered alpha)
		int8_t alpha_mode = 0, src = 0;
		bool blended = false;
		int32_t lf_src = -1;         // LF frames (J40HIP_SEQ_LFFRAME): the row whose picture this frame's LF samples are (use_lf_frame), -1: none
		// patches (J40HIP_SEQ_PATCHES): the row is a reference-only frame, stored as three XYB planes in reference slot `xyb_slot` and never
		// shown; or a frame with patches -- its dictionary and, made of it once here, the records and their binning into tiles, which the
		// frame's handle shares (j40hip_frame::patch_plan) and its upload copies to the device
		bool stored_xyb = false;
		int32_t xyb_slot = -1;
		j40hip::PatchDictionary patches;
		std::shared_ptr<const j40hip::PatchPlan> patch_plan;
		// photon noise (J40HIP_PARSE_NOISE): the counters visible, nonvisible when the playback reaches the row -- the shown frames before
		// it, the frames since the last shown one (device/noise_dev.h)
		uint32_t noise_seeds[2] = {0, 0};
	};
	std::vector<Row> rows;
	std::vector<j40hip_frame *> frames;   // [rows.size()], parsed when first asked for
	int threads = 1; uint32_t flags = 0;
	bool blend = false;              // the blend modes other than Replace are served (J40HIP_SEQ_BLEND or J40HIP_BLEND=1)
	bool lf_frames = false;          // LF frames and use_lf_frame are served (J40HIP_SEQ_LFFRAME or J40HIP_LFFRAME=1)
	bool colour = false;             // every handle renders in the signalled colour space (J40HIP_SEQ_COLOUR or J40HIP_COLOUR=1)
	bool colour_asked = false;       // ... by the flag itself: an image the mode refuses as a whole then fails j40hip_sequence_open
	bool modular_xyb = false;        // Modular frames of an XYB image go through the XYB colour tail (J40HIP_SEQ_MODULAR_XYB or J40HIP_MODULAR_XYB=1)
	bool noise = false;              // frames with has_noise are served (J40HIP_PARSE_NOISE or J40HIP_NOISE=1)
	bool splines = false;            // frames with has_splines are served (J40HIP_SEQ_SPLINES or J40HIP_SPLINES=1)
	bool patches = false;            // reference-only frames and patch dictionaries are served (J40HIP_SEQ_PATCHES or J40HIP_PATCHES=1)
	int32_t alpha_ec = -1;           // the extra channel that is rendered as A (rendered_alpha_channel); -1: none
	int32_t output_format = J40HIP_U8X4;
	j40hip_sequence_device *dev = nullptr;
};
extern "C" void j40hip_sequence_release_device(j40hip_sequence *s);   // device/runtime_seq.hip

// a tri-state mode of a handle (-1: as its environment switch says, read only then; else the mode itself)
template <typename Env> inline int mode_on(int mode, Env env) { return mode >= 0 ? mode : (int) env(); }

// the alpha mode in force: kept only where asked for (or J40HIP_ALPHA=1) AND the frame is one keep mode serves (plan_build.cpp:
// alpha_keep_scope) -- with the environment variable alone every other frame decodes opaque as before
inline bool j40hip_alpha_kept(const j40hip_frame *h) {
	int32_t index;
	return mode_on(h->alpha, j40hip::alpha_env) && !h->from_view && j40hip::alpha_keep_scope(h->frame, &index) == 0;
}

// YCbCr frames are served: asked for (or J40HIP_YCBCR=1) on a handle of the single-frame decode -- not one a sequence hands out, not
// one built from a view (whose LF bundle knows nothing of channel sizes)
inline bool j40hip_ycbcr_on(const j40hip_frame *h) {
	return mode_on(h->ycbcr, j40hip::ycbcr_env) && !h->from_view && !h->from_sequence;
}

// Modular frames of XYB images: the frames the rule applies to -- a Modular frame of a colour image with
// xyb_encoded = 1, integer samples of 8 bits or more, no YCbCr -- and whether it is in force: asked for (or J40HIP_MODULAR_XYB=1) on such
// a frame; with the environment variable alone every other frame decodes as before
inline bool j40hip_modular_xyb_applies(const j40hip_frame *h) {
	const j40hip::Frame &f = h->frame;
	return f.fh.is_modular && f.im.xyb_encoded && !f.im.grey && !f.fh.do_ycbcr && !f.im.exp_bits && f.im.bpp >= 8 && !f.lf_only && !h->from_view;
}
inline bool j40hip_modular_xyb_on(const j40hip_frame *h) {
	return mode_on(h->modular_xyb, j40hip::modular_xyb_env) && j40hip_modular_xyb_applies(h);
}

// The colour mode: what the setter refuses ("Ucs?"), the frames the rule applies to -- XYB images it does not refuse --
// and whether it is in force: asked for (or J40HIP_COLOUR=1) on such a frame whose encoding is not the sRGB default; with the environment
// variable alone every other frame decodes as before. An image with xyb_encoded = 0 holds samples in its signalled space already:
// accepted, never in force. A YCbCr frame, a Modular frame that does not go through the XYB colour tail, the LF preview and a handle
// built from a view have no XYB tail to redirect.
inline uint32_t j40hip_colour_refusal(const j40hip_frame *h) {
	const j40hip::Frame &f = h->frame;
	if (f.fh.do_ycbcr) return j40hip::colour::ERR_UCS;
	if (!f.im.xyb_encoded) return 0;
	if (uint32_t e = j40hip::colour::image_refusal(f.im)) return e;
	if (f.lf_only || h->from_view) return j40hip::colour::ERR_UCS;
	return f.fh.is_modular && !j40hip_modular_xyb_on(h) ? j40hip::colour::ERR_UCS : 0;
}
inline bool j40hip_colour_applies(const j40hip_frame *h) { return h->frame.im.xyb_encoded && !j40hip_colour_refusal(h); }
inline bool j40hip_colour_on(const j40hip_frame *h) {
	return mode_on(h->colour, j40hip::colour_env) && !h->frame.im.cenc.srgb_default() && j40hip_colour_applies(h);
}

// A handle a sequence hands out for the main frame of a still whose LF image is a frame of its own: a regular frame with use_lf_frame
// that covers the canvas. Once the playback has filled its LF slot (and bound it) the handle decodes alone like any frame, so it takes
// a scale and the orientation, which every other handle of a sequence refuses; the playback refuses it while either is set
inline bool j40hip_lf_still_handle(const j40hip_frame *h) {
	const j40hip::FrameHeader &fh = h->frame.fh;
	return h->from_sequence && fh.use_lf_frame && fh.type != 1 && fh.x0 == 0 && fh.y0 == 0 && fh.width == h->frame.im.width && fh.height == h->frame.im.height;
}

// Likewise the handle of a frame with patches that covers the canvas: once the playback has bound its reference slots it decodes alone
// like any frame, so it takes a scale (a region it takes anyway); the playback refuses it while one is set. Never an orientation.
inline bool j40hip_patch_still_handle(const j40hip_frame *h) {
	const j40hip::FrameHeader &fh = h->frame.fh;
	return h->from_sequence && fh.has_patches && (fh.type == 0 || fh.type == 3) && fh.x0 == 0 && fh.y0 == 0 && fh.width == h->frame.im.width && fh.height == h->frame.im.height;
}

// the orientation the next decode writes in: the stream's where the mode (or J40HIP_ORIENT=1) applies it, else 1 (stored order). A handle
// a sequence hands out is never oriented: the playback writes stored order -- but for the main frame of an LF-frame still, and that one
// only where the mode was set on the handle itself (the environment never orients a sequence's handles)
inline int32_t j40hip_orientation_in_force(const j40hip_frame *h) {
	if (h->from_sequence) return h->orient == 1 && j40hip_lf_still_handle(h) ? h->frame.im.orientation : 1;
	return mode_on(h->orient, j40hip::orient_env) ? h->frame.im.orientation : 1;
}

// internal (a sequence's playback, device/runtime_seq.hip): the LF frame's picture the next decodes of a frame with use_lf_frame read --
// device planes X, Y, B of w x h floats each, which must stay where they are until those decodes have run
inline void j40hip_frame_bind_lf_source(j40hip_frame *h, const float *const planes[3], int32_t w, int32_t hh) {
	for (int c = 0; c < 3; ++c) h->lf_src[c] = planes[c];
	h->lf_src_w = w; h->lf_src_h = hh;
}

// internal (a sequence's playback): the reference-only frame's planes in slot `slot` that the next decodes of a frame with patches read,
// which must stay where they are until those decodes have run; base null: the slot is empty
inline void j40hip_frame_bind_patch_source(j40hip_frame *h, int32_t slot, const float *base, int32_t w, int32_t hh) {
	h->patch_src[slot].base = base; h->patch_src[slot].w = w; h->patch_src[slot].h = hh;
}

extern "C" j40hip_frame *j40hip_frame_parse_with(const void *buf, size_t size, int threads, uint32_t flags, j40hip::LfDeviceDecoder lf_decoder, void *lf_ctx, uint32_t *err);

// implemented next to the kernels; a no-op when nothing was uploaded
extern "C" void j40hip_release_device(j40hip_frame *f);

// internal to the library (api.cpp <-> the device side): the process-wide serving pipeline of a device (device/pipeline.hip) and
// the pool of pinned host planes the public API hands out as image pixels (device/device_memory.hip)
extern "C" j40hip_pipeline *j40hip_serve_pipeline(int device, uint32_t *err);
extern "C" void j40hip_serve_shutdown(void);
// CPUs' worth of time the process may use: the visible CPUs, or the cgroup's quota (v2 cpu.max, v1 cfs_quota_us) when that is less.
// A process that runs into its quota has ALL its threads throttled, the HIP runtime's included: thread counts are sized from this.
extern "C" int j40hip_cpu_quota();
extern "C" void *j40hip_pinned_acquire(size_t bytes);
extern "C" void j40hip_pinned_release(void *ptr, size_t bytes);
