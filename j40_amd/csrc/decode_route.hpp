// j40_amd/csrc/decode_route.hpp -- the one place that interprets a frame handle's modes (output format, region, scale, orientation, restoration,
// kept alpha, YCbCr, Modular XYB, the group range): resolve_route states what the next decode does, mode_refusal which modes exclude which; the
// setters, the getters and every decode entry read their answers. A further mode is added here. Host code only: no HIP, nothing allocated.
// (A further operation on a frame's XYB planes -- behind the filters, ahead of the tail -- is added in device/runtime.hip: render_planes.)
// Photon noise (a frame parsed with J40HIP_PARSE_NOISE whose header has has_noise) is such an operation, and like patches a property of the
// frame, not a mode of the handle: DecodeRoute::noise sends the decode through the plane stage -- whole frames at full size, from which a
// region is cut and a scale averaged (full_size_first), in one phase --, and refuses what has no full-size XYB planes to add it to: a
// Modular frame without the Modular XYB switch, a YCbCr plan, a partial group range, a batch, many LF previews in one launch (an LF-only parse of such a frame is refused by the parse).
// Splines (a frame parsed with J40HIP_PARSE_SPLINES whose header has has_splines) are such an operation as well, between the patches and the
// noise: DecodeRoute::splines goes wherever patches and noise go.
// Upsampling (a frame parsed with J40HIP_PARSE_UPSAMPLING whose header has upsampling > 1) is such an operation too, the one that changes the
// planes' size: DecodeRoute::upsampling sends the decode through the plane stage, where k_upsample stretches the coded planes to the shown
// size ahead of the tail; stored_w and stored_h come from the shown size, a region is cut from and a scale averaged over the shown-size
// picture, in one phase. Refused ("TODO"): what noise refuses, and kept alpha, a frame that also has patches or noise (shown-size
// operations: a follow-up), a Modular frame with an alpha channel, every frame of a sequence (the parse).
#pragma once
#include "capi.hpp"
#include "device/orient_dev.h"

namespace j40hip {

constexpr uint32_t ERR_URG = E4("Urg?");   // a region (j40hip_frame_set_region) where only whole frames or group ranges are served, or the other way round
constexpr uint32_t ERR_USC = E4("Usc?");   // a scale (j40hip_frame_set_scale) where only full-size frames are served, or the other way round
constexpr uint32_t ERR_UOR = E4("Uor?");   // an orientation in force (j40hip_frame_set_orientation) where only stored order is served
constexpr uint32_t ERR_UCS = colour::ERR_UCS;   // the colour mode (j40hip_frame_set_colour) on an image it does not serve, or in force where only sRGB pixels are served
constexpr uint32_t ERR_ULF = E4("Ulf?");   // an LF-only frame (J40HIP_PARSE_LF_ONLY) has nothing but its LF image: the full decode's entry points refuse it

// ---- which modes exclude which ----
// What is about to be set on a handle (the three setters; GroupRange: a partial one) or about to take the handle as it is (a batch, a
// sequence's playback, many LF previews in one launch). 0, or the code it is refused with for what the handle already has; where two
// apply, the one named first wins. The orientation is asked for last, and only where it decides: it may read J40HIP_ORIENT.
enum class Mode { Region, Scale, Orientation, GroupRange, Batch, Playback, LfPreviewBatch };
inline uint32_t mode_refusal(const j40hip_frame *h, Mode what) {
	const auto oriented = [h] { return j40hip_orientation_in_force(h) != 1; };
	const bool owned = h->from_sequence && !j40hip_lf_still_handle(h);   // the playback owns its size and order (capi.hpp: but for the main frame of an LF-frame still)
	const bool owned_size = owned && !j40hip_patch_still_handle(h);     // ... its size also but for a full-canvas frame with patches
	// (patches go onto whole pictures' planes through one handle's own tail: no batch, no preview of the LF image alone, no partial range)
	// (noise likewise: it is added to whole pictures' planes)
	// (an upsampled frame likewise: its coded planes are stretched whole)
	// (splines likewise: they are drawn onto whole pictures' planes)
	const bool patches = h->frame.fh.has_patches || h->frame.fh.has_splines || h->frame.fh.has_noise || h->frame.fh.upsampling > 1;
	if (patches && (what == Mode::GroupRange || what == Mode::Batch || what == Mode::LfPreviewBatch)) return ERR_TODO;
	switch (what) {
	case Mode::Region:         return h->partial_range ? ERR_URG : h->scale > 0 ? ERR_USC : 0;
	case Mode::Scale:          return h->region_set || h->partial_range || owned_size ? ERR_USC : 0;
	// (a partial group range writes its own rectangles of the stored image: nothing whole to turn)
	case Mode::Orientation:    return owned || (h->partial_range && h->frame.im.orientation != 1) ? ERR_UOR : 0;
	// (the colour tail runs over whole pictures: a partial range has none; batches and pipelines render sRGB only)
	case Mode::GroupRange:     return h->region_set ? ERR_URG : h->scale > 0 ? ERR_USC : oriented() ? ERR_UOR : j40hip_colour_on(h) ? ERR_UCS : 0;
	case Mode::Batch:          return h->region_set ? ERR_URG : oriented() ? ERR_UOR : j40hip_colour_on(h) ? ERR_UCS : 0;   // a batch writes whole frames in stored order, at any one scale
	case Mode::Playback:       return h->scale > 0 ? ERR_USC : oriented() ? ERR_UOR : 0;    // the canvas is full size, stored order
	case Mode::LfPreviewBatch: return oriented() ? ERR_UOR : j40hip_colour_on(h) ? ERR_UCS : 0;
	}
	return 0;
}

// ---- the route ----
inline int32_t scaled_size(int32_t n, int32_t shift) { return (n + (1 << shift) - 1) >> shift; }   // ceil(n / 2^shift) (j40hip_frame_set_scale)
inline bool signals_filters(const FrameHeader &fh) { return fh.restoration.gab || fh.restoration.epf_iters > 0; }   // (whether they run is the restoration mode's business)

// what the decision needs of the upload (j40hip_device_state's): a Modular plan, a VarDCT plan built for a YCbCr frame, sections that go on
// with the extra channels' sub-images, the group range
struct UploadFacts { bool is_modular, ycbcr, has_trailers; int64_t first_group, num_groups; bool modular_alpha = false; };   // modular_alpha: a Modular plan renders A from a plane of its own

struct DecodeRoute {
	uint32_t refusal = 0;              // what every single-frame decode entry answers before anything is launched or allocated (not its concern: xyb_refusal)
	int32_t orientation = 1;           // in force; other than 1: k_orient writes the caller's image from a stored-order staging image
	int32_t stored_w = 0, stored_h = 0, out_w = 0, out_h = 0;   // the stored-order image the decode makes (the region's rectangle, else the frame at its scale shift) and, in the orientation in force, the image written
	size_t pixel_bytes = 4, min_stride = 0;   // of the image written (a whole u8 frame in stored order: 0, the entry points' old contract)
	enum Shape { Whole, Region, Scaled } shape = Whole;
	bool full_size_first = false;      // a region or a scale served from full-size pixels in a staging image: filters in force, merged alpha, the colour mode in force; at a scale a Modular XYB frame (k_modular_xyb_pack writes full-size pixels only, the mean is of rendered bytes)
	int restoration_asked = 0;         // the restoration mode of a VarDCT plan decoding every group (the filters run over whole frames), whatever the frame signals
	int restoration = 0;               // ... and in force: where the frame signals filters
	bool alpha_merged = false;         // the extra channels' sub-images carry an alpha channel that is kept: k_alpha_merge writes it into full-size pixels
	bool modular_xyb = false;          // a Modular plan through the XYB colour tail
	bool patches = false;              // the frame has a patch dictionary: its pixels come from XYB planes (the filtered ones where the filters are in force), k_patch_blend over them, then the tail
	bool splines = false;              // the frame has splines: likewise, k_spline_draw behind the patches, ahead of the noise
	bool noise = false;                // the frame has noise: likewise, k_noise_fill and k_noise_add behind the patches, ahead of the tail
	bool upsampling = false;           // the frame is coded at 1:2, 1:4 or 1:8: k_upsample behind the filters makes the shown-size planes the tail reads
	bool colour = false;               // the colour mode in force: the XYB planes (filtered where the filters are in force; a Modular XYB plan's by k_modular_to_xyb) go through k_colour_tail
	bool every_group = true;           // no partial group range
	bool two_phase = false;            // decode_to_host may try its two phases: a whole frame in stored order that takes no LF frame's picture
	uint32_t xyb_refusal = 0;          // decode_frame_xyb's answer: "TODO" for what keeps the decode from being three full-size XYB planes
};

// `out`, `stride_bytes`: the caller's image (the getters, which want sizes alone, pass none)
inline DecodeRoute resolve_route(const j40hip_frame *h, const UploadFacts *up, bool have_out = true, size_t stride_bytes = SIZE_MAX) {
	DecodeRoute r;
	const Frame &fr = h->frame;
	r.orientation = j40hip_orientation_in_force(h);
	r.shape = h->region_set ? DecodeRoute::Region : h->scale > 0 ? DecodeRoute::Scaled : DecodeRoute::Whole;
	r.stored_w = h->region_set ? h->region[2] : scaled_size(fr.fh.shown_width(), h->scale);
	r.stored_h = h->region_set ? h->region[3] : scaled_size(fr.fh.shown_height(), h->scale);
	orient_out_size(r.stored_w, r.stored_h, r.orientation, &r.out_w, &r.out_h);
	r.pixel_bytes = h->output_format == J40HIP_U16X4 ? 8 : 4;
	const bool old_contract = r.shape == DecodeRoute::Whole && r.orientation == 1 && r.pixel_bytes == 4;
	r.min_stride = old_contract ? 0 : r.pixel_bytes * (size_t) r.out_w;
	if (fr.lf_only) { r.refusal = ERR_ULF; r.xyb_refusal = ERR_TODO; return r; }
	if (!up) { r.refusal = E4("!gpu"); return r; }
	r.every_group = up->first_group == 0 && up->num_groups == fr.fh.num_groups;
	r.restoration_asked = up->is_modular || !r.every_group ? 0 : mode_on(h->restoration, restoration_env);
	r.restoration = signals_filters(fr.fh) ? r.restoration_asked : 0;
	r.alpha_merged = up->has_trailers && j40hip_alpha_kept(h);
	r.modular_xyb = up->is_modular && j40hip_modular_xyb_on(h);
	r.colour = j40hip_colour_on(h);
	r.patches = fr.fh.has_patches;
	r.splines = fr.fh.has_splines;
	r.noise = fr.fh.has_noise;
	r.upsampling = fr.fh.upsampling > 1;
	const bool full_size_only = r.colour || r.patches || r.splines || r.noise || r.upsampling || (up->is_modular ? r.modular_xyb && r.shape == DecodeRoute::Scaled : r.restoration || r.alpha_merged);
	r.full_size_first = r.shape != DecodeRoute::Whole && full_size_only;
	r.two_phase = r.shape == DecodeRoute::Whole && r.orientation == 1 && !fr.fh.use_lf_frame && !r.colour && !r.patches && !r.splines && !r.noise && !r.upsampling;
	r.xyb_refusal = r.patches || r.splines || r.noise || r.upsampling || r.shape != DecodeRoute::Whole || !r.every_group || (up->is_modular ? !r.modular_xyb : up->ycbcr || up->has_trailers) ? (uint32_t) ERR_TODO : 0;
	// in the entry points' order: an orientation over a partial range (no whole stored image to turn), the oriented image's rows, a YCbCr plan
	// (served only while its switch stays on, and whole), the stored image's rows
	if (r.orientation != 1 && !r.every_group) r.refusal = ERR_UOR;
	else if (r.colour && !r.every_group) r.refusal = ERR_UCS;   // (a group range set before the mode: mode_refusal's rule)
	// (a Modular frame's planes reach XYB through the Modular XYB switch alone)
	else if ((r.patches || r.splines || r.noise || r.upsampling) && (!r.every_group || (up->is_modular && !r.modular_xyb) || up->ycbcr)) r.refusal = ERR_TODO;
	// (splines belong on the coded planes ahead of the stretch: a follow-up)
	// (noise is a shown-size operation, the kept alpha and a Modular frame's alpha plane would have to be stretched as well)
	// (a frame with patches exists in sequences alone, whose frames the parse refuses: nothing to ask here)
	else if (r.upsampling && (r.splines || r.noise || r.alpha_merged || (up->is_modular && up->modular_alpha))) r.refusal = ERR_TODO;
	else if (r.orientation != 1 && (!have_out || stride_bytes < r.min_stride)) r.refusal = ERR_RNGE;
	else if (up->ycbcr && (!j40hip_ycbcr_on(h) || r.shape != DecodeRoute::Whole || !r.every_group)) r.refusal = ERR_TODO;
	else if (stride_bytes < r.min_stride) r.refusal = ERR_RNGE;
	return r;
}

} // namespace j40hip
