// j40_amd/csrc/device/kernels.h -- launch entry points of device/kernels.hip and device/modular_kernels.hip
#pragma once
#include <hip/hip_runtime.h>
#include "plan.h"
#include "restore_dev.h"
#include "region_dev.h"
#include "colour_dev.h"
#include "patch_dev.h"
#include "noise_dev.h"
#include "spline_dev.h"
#include "upsample_dev.h"

namespace j40hip {

void upload_constant_tables(const float *half_secants, const float *afv_basis, const float *srgb_thr, hipStream_t stream);
void launch_hf_entropy(const DevPlan &plan, const HfLaunchInfo &info, int32_t first_group, int32_t num_groups, hipStream_t stream);
// the single-image path's two phases (runtime.hip): is the fast entropy kernel the one this frame gets; that kernel over the groups
// order[first .. first + count); the block_events entries of the groups order[0 .. k) copied from `shadow` into the plan's table
bool hf_entropy_fast_path(const DevPlan &plan, const HfLaunchInfo &info);
void launch_hf_entropy_fast_ordered(const DevPlan &plan, const HfLaunchInfo &info, const uint32_t *order, int32_t first, int32_t count, hipStream_t stream);
void launch_merge_block_events(const DevPlan &plan, const uint32_t *order, int32_t k, const uint32_t *shadow, hipStream_t stream);
// the rectangles of the groups order[0 .. k) out of the device image into a host image the device can write (pinned)
void launch_store_group_rects(const uint32_t *order, int32_t k, int32_t gcolumns, int32_t shift, int32_t width, int32_t height, const uint8_t *src, uint8_t *dst_host_mapped, size_t stride_bytes, hipStream_t stream, int32_t pixel_bytes = 4);
uint32_t hf_lanes_lds_bytes(const HfLaunchInfo &info);
void launch_hf_entropy_lanes(const DevPlan *plans, const HfLaneWork *work, int32_t num_work, bool tables_in_lds, uint32_t lds_bytes, hipStream_t stream);
void launch_hf_lanes(const DevPlan *plans, const HfLaneWork *work, int32_t num_work, int32_t waves_per_wg, uint32_t lds_bytes, hipStream_t stream, hipEvent_t started = nullptr, hipEvent_t stopped = nullptr, uint32_t *queue = nullptr);
// every frame of a batch: one persistent launch per class of transforms, spread over `nside` side streams that fork from and join
// `stream` (nside = 0: all on `stream`). tile_prefix_dev: K2_NUM_BATCH_LAUNCHES * (nframes + 1) ints of scratch; totals_dev:
// K2_NUM_BATCH_LAUNCHES ints (out: tiles per launch); grids: workgroups per launch, from k2_batch_grids
enum { K2_NUM_BATCH_LAUNCHES = 16, K2_LARGE_WGS = 256, K2_WG_SLOTS = 32768 };   // K2_WG_SLOTS: the most workgroups a launch gets (k2_batch_grids' wg_slots)
void k2_batch_grids(const int32_t *last_totals, size_t cells_total, int32_t nframes, int32_t wg_slots, int32_t *grids);
void launch_vardct_batch(const K2Frame *frames_dev, int32_t nframes, int32_t *tile_prefix_dev, int32_t *totals_dev, const int32_t *grids, float *large_scratch, hipStream_t stream, hipStream_t *side, int nside, hipEvent_t fork, hipEvent_t *side_done, int32_t shift = 0);
// The pixel stage of one frame. Where its samples go (K2Target): `out` says as what -- RGBA8: u8x4 pixels; RGBA16: the 16-bit output
// (J40_U16X4, 8 bytes a pixel; idct_dev.h xyb_to_rgba16); XYB: left in XYB for the restoration filters and LF frames
// (device/restore_kernels.h, restore_dev.h), three float planes of `stride` bytes per row, one behind the other; YCC: a subsampled
// YCbCr frame (DevFrame::ycc_shifts; it holds DCT8 blocks alone), three float planes one behind the other, each of the padded grid's
// size at its channel's resolution (ycbcr_dev.h: ycc_plane_dims), `stride` unused -- and `shift` is the scale shift (1, 2: the kernels
// write the 1:2 / 1:4 image, scale_dev.h; `base` and `stride` are then the small image's; the pixel forms only).
enum class OutMode { RGBA8, XYB, RGBA16, YCC };
struct K2Target { void *base; size_t stride; OutMode out; int32_t shift; };
void launch_vardct_frame(const DevPlan &plan, const int32_t *class_start, const DevVarblock *sorted, float *large_scratch, const K2Target &to, hipStream_t stream);

// the restoration filters (device/restore_kernels.h, restore_dev.h): the reciprocal-sigma plane, Gaborish + the edge-preserving
// filter's steps between `xyb` and `tmp` (returns where the result lies), the colour tail on planes
void launch_epf_sigma(const DevPlan &plan, int32_t num_lf_groups, const int16_t *sharpness, const RestoreParams &p, float *sigma, uint32_t *sharp_or, hipStream_t stream);
void launch_epf_sigma_cells(const int16_t *sharpness, const float *hfmul_inv, const RestoreParams &p, float *sigma, uint32_t *sharp_or, hipStream_t stream);
float *launch_restoration(float *xyb, float *tmp, size_t pitch, const RestoreParams &p, bool gab, int32_t epf_iters, const float *sigma, hipStream_t stream);
void launch_xyb_to_rgba(const float *xyb, size_t pitch, const DevFrame *frame_dev, int32_t width, int32_t height, uint8_t *rgba, size_t stride_bytes, hipStream_t stream, bool rgba16 = false);

// the colour mode's tail (device/colour_kernels.hip, colour_dev.h): k_colour_tail over three planes laid out as launch_xyb_to_rgba's,
// in the colour space `p` describes; p.table: device memory
void launch_colour_tail(const float *xyb, size_t pitch, const ColourTailParams &p, int32_t width, int32_t height, uint8_t *out, size_t stride_bytes, hipStream_t stream, bool rgba16 = false);

// patches (device/patch_kernels.hip, patch_dev.h): k_patch_blend over the three planes at `planes` (width * height floats each, one behind
// the other), one workgroup per non-empty tile of `p` (device memory); nothing is launched for a list without tiles
void launch_patch_blend(float *planes, int32_t width, int32_t height, const DevPatches &p, const PatchSlots &slots, hipStream_t stream);

// photon noise (device/noise_kernels.hip, noise_dev.h): k_noise_fill makes the three raw planes at `raw` (noise_pitch(W) floats a row, one
// plane behind the other) from the frame's four jump sets in device memory; k_noise_add convolves them and adds the result onto the
// three planes at `planes` (`ppitch` floats a row, one behind the other), in place
void launch_noise_fill(float *raw, const NoiseFillArgs &a, const uint64_t *sets_dev, hipStream_t stream);
void launch_noise_add(float *planes, size_t ppitch, const float *raw, int32_t W, int32_t H, const NoiseParams &p, hipStream_t stream);

// upsampling (device/upsample_kernels.hip, upsample_dev.h): k_upsample<k> stretches the three coded planes at `src` (w x h floats each, one
// behind the other) into the three at `out` (up_w x up_h each, up_w <= k * w, up_h <= k * h) by the expanded table at `table_dev`
// (k * k * 25 floats, device memory). false: a factor or a size it does not take, nothing launched
bool launch_upsample(const float *src, int32_t w, int32_t h, int32_t k, const float *table_dev, float *out, int32_t up_w, int32_t up_h, hipStream_t stream);

// splines (device/spline_kernels.hip, spline_dev.h): k_spline_draw adds the segments of `d` (device memory) onto the three planes at
// `planes` (`pitch` floats a row, one behind the other), in place, one workgroup per touched tile; nothing is launched without tiles
void launch_spline_draw(float *planes, size_t pitch, int32_t W, int32_t H, const DevSplines &d, hipStream_t stream);

// LfGroup tail on the device (device/lf_tail_kernels.hip)
void upload_lf_tail_tables(const float *half_secants, const float *lf2llf, hipStream_t stream);
void launch_lf_tail(const DevPlan &plan, int32_t num_lf_groups, int32_t max_cells, size_t cells, float *lfs, const DevVarblock *sorted, int32_t count, int32_t first_large, int32_t smooth,
		const float inv_m_lf[3], hipStream_t stream);
// ... of a frame with use_lf_frame: k_lf_from_frame (args.src, the thresholds; out and lfindices are filled in here), k_lf_frame_bctx
// where `bctx` (the frame has LF thresholds), then the LLF kernels as above
void launch_lf_frame_tail(const DevPlan &plan, int32_t num_lf_groups, int32_t max_cells, size_t cells, float *lfs, const DevVarblock *sorted, int32_t count, int32_t first_large,
		LfFrameArgs args, bool bctx, int32_t num_groups, hipStream_t stream);

void launch_lf_tail_batch(const DevPlan *plans, const DevPlanBuild *builds, const DevBatchLf *lfs, int32_t nframes, int32_t nlf, int32_t max_lf_cells, size_t max_frame_cells, hipStream_t stream);
// the LF-dependent half of the plan of every frame of a batch (device/plan_kernels.hip)
void launch_plan_build(const DevPlanBuild *builds, const DevBatchLf *lfs, int32_t nframes, int32_t nlf, int32_t max_lf_cells, hipStream_t stream);
void launch_clear_block_events(const DevPlan *plans, const DevPlanBuild *builds, int32_t nframes, size_t max_frame_cells, hipStream_t stream);
void launch_plan_verdict(const DevPlanBuild *builds, const DevPlan *plans, int32_t nframes, hipStream_t stream);

// the LF preview (device/lf_preview.hip): nblocks workgroups of LFP_LANES lanes over the work list (DevLfpWork, plan.h); mode LFP_U8 /
// LFP_U16 writes the pixels, LFP_PLANE channel `channel` of the dequantised, smoothed samples as floats
enum { LFP_U8 = 0, LFP_U16 = 1, LFP_PLANE = 2, LFP_LANES = 256 };
void upload_lf_preview_tables(const float *srgb_thr, hipStream_t stream);
void launch_lf_preview(const DevLfpFrame *frames, const DevLfpWork *work, int32_t nwork, uint32_t nblocks, int32_t mode, int32_t channel, hipStream_t stream);

void launch_kat_srgb_u8(const float *v, size_t n, uint8_t *out, hipStream_t stream);
void launch_kat_srgb_u16(const float *v, size_t n, int32_t bpp, uint16_t *out, hipStream_t stream);

// Modular path (device/modular_kernels.hip)
void launch_modular_sections(const DevModPlan &plan, int32_t first_section, int32_t num_sections, const ModLaunchInfo &info, hipStream_t stream);
void launch_lf_groups(const DevLfTask *tasks, int32_t num_tasks, hipStream_t stream);
// one LfGroup section per lane (lf_lanes_dev.h): pack_lf_waves deals the sections of the sets (host copies) to wavefronts and returns
// the LDS a wavefront needs at most; launch_lf_lanes takes the device copies of both arrays
#include <vector>
uint32_t pack_lf_waves(const DevLfLaneSet *sets_host, int32_t num_sets, std::vector<DevLfWave> *waves, const std::vector<int32_t> *only = nullptr);
void launch_lf_lanes(const DevLfLaneSet *sets, const DevLfWave *waves, int32_t num_waves, uint32_t lds_bytes, hipStream_t stream, hipEvent_t started = nullptr, hipEvent_t stopped = nullptr);
// the same with tree, alias tables and row windows in LDS (lf_rows_dev.h, k_lf_rows): pack_lf_row_waves returns 0 when some frame's
// tables do not fit a wavefront's LDS -- with `oversized`, those frames alone are listed for k_lf_lanes --; lf_rows_enabled: J40HIP_LF_KERNEL != "lanes"
bool lf_rows_enabled();
uint32_t pack_lf_row_waves(const DevLfLaneSet *sets_host, int32_t num_sets, std::vector<DevLfWave> *waves, std::vector<int32_t> *oversized = nullptr);
void launch_lf_rows(const DevLfLaneSet *sets, const DevLfWave *waves, int32_t num_waves, uint32_t lds_bytes, hipStream_t stream, hipEvent_t started = nullptr, hipEvent_t stopped = nullptr);
void launch_modular_quad(const DevModPlan &plan, int32_t first_section, int32_t num_sections, int32_t spec_idx, uint32_t table_span, int32_t max_width, hipStream_t stream);
void launch_modular_split(const DevModPlan &plan, int32_t first_section, int32_t num_sections, const ModLaunchInfo &info, hipStream_t stream);
void launch_modular_coop(const DevModPlan &plan, int32_t first_section, int32_t num_sections, int32_t max_width, hipStream_t stream, bool wide = false);
// the planes arrive as PlanePtr (plan.h): address + bytes per sample; planes of one call have the same sample size, which picks the instantiation
void launch_section_inverse_rcts(const DevModPlan &plan, int32_t first_section, int32_t num_sections, hipStream_t stream, bool wide = false);
void launch_paste_plane(PlanePtr src, int32_t w, int32_t h, PlanePtr dst, int32_t dst_stride, hipStream_t stream);
void launch_inverse_rct(PlanePtr a, PlanePtr b, PlanePtr c, size_t n, int32_t type7, hipStream_t stream);
void launch_inverse_palette_plain(PlanePtr idx, PlanePtr palrow, PlanePtr dst, size_t n, int32_t i, int32_t nb_colours, int32_t bpp, hipStream_t stream);
void launch_inverse_palette_predicted(PlanePtr idx, PlanePtr pal, int32_t pal_stride, void *const *dst_dev, int32_t num_c, int32_t width, int32_t height,
		int32_t nb_colours, int32_t nb_deltas, int32_t d_pred, int32_t bpp, const int8_t *wpp_dev, int32_t *wp_scratch, uint32_t *status, hipStream_t stream);
void launch_inverse_squeeze(PlanePtr avg, PlanePtr res, PlanePtr out, int32_t aw, int32_t ah, int32_t rw, int32_t rh, bool horizontal, hipStream_t stream);
// a: a null address where the frame has no alpha plane
void launch_pack_planes_rect(PlanePtr r, PlanePtr g, PlanePtr b, PlanePtr a, int32_t plane_width, int32_t x0, int32_t y0, int32_t rw, int32_t rh, int32_t bpp, uint8_t *rgba, size_t stride, hipStream_t stream, bool rgba16 = false);
// alpha_kernels.hip: the kept alpha channel of a VarDCT frame into rectangle (x0, y0, w, h) of pixels already written
void launch_alpha_merge(const int16_t *plane, int32_t pitch, int32_t x0, int32_t y0, int32_t w, int32_t h, int32_t bpp, uint8_t *rgba, size_t stride, hipStream_t stream, bool rgba16);
// ycbcr_kernels.hip: the three float planes of a YCbCr VarDCT frame (ycbcr_dev.h: YcbcrTail) to the picture's width x height pixels
struct YcbcrTail;
void launch_ycbcr_tail(const YcbcrTail &t, uint8_t *rgba, size_t stride, hipStream_t stream, bool rgba16);
// shift: the scale shift; 1, 2: ceil(width / s) x ceil(height / s) pixels, each the mean of its cell's rendered samples (scale_dev.h)
void launch_pack_planes(PlanePtr r, PlanePtr g, PlanePtr b, PlanePtr a, int32_t width, int32_t height, int32_t bpp, uint8_t *rgba, size_t stride, hipStream_t stream, bool rgba16 = false, int32_t shift = 0);

// a Modular frame of an XYB image through the XYB colour tail (device/modular_xyb_kernels.hip, modular_xyb_dev.h): c0, c1, c2 the colour
// planes (quantised Y, X, B - Y), a as above; k: the frame's m_lf_scaled and colour constants. The rect form as launch_pack_planes_rect.
// launch_modular_to_xyb: the rectangle's three float planes alone, its sample (0, 0) first, `pitch` floats a row
struct ModXybConsts;
void upload_modular_xyb_tables(const float *srgb_thr, hipStream_t stream);
void launch_modular_xyb_pack(PlanePtr c0, PlanePtr c1, PlanePtr c2, PlanePtr a, int32_t width, int32_t height, const ModXybConsts &k, uint8_t *rgba, size_t stride, hipStream_t stream, bool rgba16 = false);
void launch_modular_xyb_pack_rect(PlanePtr c0, PlanePtr c1, PlanePtr c2, PlanePtr a, int32_t plane_width, int32_t x0, int32_t y0, int32_t rw, int32_t rh, const ModXybConsts &k, uint8_t *rgba, size_t stride, hipStream_t stream, bool rgba16 = false);
// the A of every pixel of a width x height image from the alpha plane, pack_rgba8 / pack_rgba16's sample, into pixels written opaque:
// behind k_colour_tail on a Modular XYB frame under the colour mode, and the known-answer hook's two-kernel route
void launch_alpha_from_plane(PlanePtr a, int32_t width, int32_t height, int32_t bpp, uint8_t *rgba, size_t stride, hipStream_t stream, bool rgba16);
void launch_modular_to_xyb(PlanePtr c0, PlanePtr c1, PlanePtr c2, int32_t plane_width, int32_t x0, int32_t y0, int32_t rw, int32_t rh, const ModXybConsts &k, float *x, float *y, float *b, size_t pitch, hipStream_t stream);

// reduced-size decode (device/scale_kernels.hip, scale_dev.h): the full W x H image at src made 1:2 (shift 1) or 1:4 (shift 2) at dst,
// pixel_bytes 4 or 8, every row pixel-aligned
void launch_downscale(const uint8_t *src, size_t src_stride, uint8_t *dst, size_t dst_stride, int32_t W, int32_t H, int32_t shift, int32_t pixel_bytes, hipStream_t stream);

// oriented output (device/orient_kernels.hip, orient_dev.h): the W x H image at src written in orientation 1..8 (the EXIF numbering) at dst,
// W x H pixels for orientations up to 4 and H x W from 5 on; pixel_bytes 4 or 8, every row of both pixel-aligned
void launch_orient(const uint8_t *src, size_t src_stride, uint8_t *dst, size_t dst_stride, int32_t W, int32_t H, int32_t orientation, int32_t pixel_bytes, hipStream_t stream);

// region decode (device/region_kernels.hip, region_dev.h). launch_region_index: the group-major index of the `count` varblocks of
// `sorted` -- cursor: nkeys = groups * REGION_KEYS words of scratch, seg_start: nkeys + 1 words, index: count words.
// launch_region_gather: the cover's varblocks, class by class from class_start[28], into `list` with their positions counted from the
// cover's origin, and the cover's groups into `order`. launch_region_crop: w x h pixels of pixel_bytes (4 or 8) from src to dst, both
// pointing at the rectangle's first pixel
void launch_region_index(const DevVarblock *sorted, uint32_t count, int32_t shift, int32_t gcolumns, uint32_t nkeys, uint32_t *cursor, uint32_t *seg_start, uint32_t *index, hipStream_t stream);
void launch_region_gather(const DevVarblock *sorted, const uint32_t *index, const uint32_t *seg_start, const RegionCover &cover, const int32_t *class_start, DevVarblock *list, uint32_t *order, hipStream_t stream);
void launch_region_crop(const uint8_t *src, size_t src_stride, uint8_t *dst, size_t dst_stride, int32_t w, int32_t h, int32_t pixel_bytes, hipStream_t stream);

// frame sequences (device/compose_kernels.hip, compose_dev.h): the frame image `frm` (w x h pixels, its pixel (0, 0) canvas pixel
// (x0, y0); any offsets, clipped here) onto the W x H canvas at `out`; outside the rectangle the pixels of `src` or, src null, the empty
// pixel (its bytes as one or two little-endian words). src == out: only the rectangle is written. Every row pixel-aligned.
void launch_frame_compose(uint8_t *out, size_t out_stride, const uint8_t *src, size_t src_stride, const uint8_t *frm, size_t frm_stride, int32_t W, int32_t H,
		int32_t x0, int32_t y0, int32_t w, int32_t h, uint32_t empty_lo, uint32_t empty_hi, int32_t pixel_bytes, hipStream_t stream);
// ... in the blend modes (compose_dev.h: BLEND_*, 0..4) cmode for the colour channels and amode for the alpha: inside the rectangle the
// frame's pixel blended over the source's (or the empty pixel). src == out: the rectangle is blended in place.
void launch_frame_blend(uint8_t *out, size_t out_stride, const uint8_t *src, size_t src_stride, const uint8_t *frm, size_t frm_stride, int32_t W, int32_t H,
		int32_t x0, int32_t y0, int32_t w, int32_t h, uint32_t empty_lo, uint32_t empty_hi, int32_t pixel_bytes, int32_t cmode, int32_t amode, hipStream_t stream);

} // namespace j40hip
