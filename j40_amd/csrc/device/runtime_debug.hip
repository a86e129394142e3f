// j40_amd/csrc/device/runtime_debug.hip -- the small setters and getters of a frame handle, and what the tests read back: stage
// dumps (j40hip_frame_read_*) and the known-answer hooks (j40hip_kat_device_*)
#include "runtime_state.hpp"
#include "ycbcr_dev.h"

extern "C" uint32_t j40hip_frame_set_output_format(j40hip_frame *h, int32_t format) {
	if (!h) return ERR_RNGE;
	if (format != J40HIP_U8X4 && format != J40HIP_U16X4) return ERR4('U', 'f', 'm', '?');
	h->output_format = format;
	return 0;
}
extern "C" uint32_t j40hip_kat_device_alpha_merge(void *rgba_dev, size_t stride_bytes, const int16_t *plane_dev, int32_t pitch, int32_t x0, int32_t y0, int32_t w, int32_t h, int32_t bpp, int32_t format, void *stream) {
	if (format != J40HIP_U8X4 && format != J40HIP_U16X4) return ERR4('U', 'f', 'm', '?');
	if (!rgba_dev || !plane_dev || bpp < 8 || bpp > 15 || x0 < 0 || y0 < 0 || w < 0 || h < 0 || pitch < 0 || (int64_t) x0 + w > pitch) return ERR_RNGE;
	if (stride_bytes < (size_t) (x0 + w) * (format == J40HIP_U16X4 ? 8 : 4)) return ERR_RNGE;
	launch_alpha_merge(plane_dev, pitch, x0, y0, w, h, bpp, (uint8_t *) rgba_dev, stride_bytes, (hipStream_t) stream, format == J40HIP_U16X4);
	return hipGetLastError() == hipSuccess ? 0 : ERR_GPU;
}
extern "C" int32_t j40hip_frame_output_format(const j40hip_frame *h) { return h ? h->output_format : 0; }
extern "C" void j40hip_frame_set_restoration(j40hip_frame *h, int mode) { if (h) h->restoration = mode < 0 ? -1 : mode > 2 ? 2 : mode; }
extern "C" void j40hip_frame_restoration(const j40hip_frame *h, j40hip_restoration *out) {
	if (!h || !out) return;
	const FrameHeader::Restoration &r = h->frame.fh.restoration;
	out->gab_enabled = r.gab ? 1 : 0;
	for (int c = 0; c < 3; ++c) for (int j = 0; j < 2; ++j) out->gab_weights[c][j] = r.gab_weights[c][j];
	out->epf_iters = r.epf_iters;
	for (int i = 0; i < 8; ++i) out->epf_sharp_lut[i] = r.sharp_lut[i];
	for (int c = 0; c < 3; ++c) out->epf_channel_scale[c] = r.channel_scale[c];
	out->epf_quant_mul = r.quant_mul; out->epf_pass0_sigma_scale = r.pass0_sigma_scale; out->epf_pass2_sigma_scale = r.pass2_sigma_scale;
	out->epf_border_sad_mul = r.border_sad_mul; out->epf_sigma_for_modular = r.sigma_for_modular;
}
// the sharpness map of LfGroup gg as decoded (i16 w8*h8), like j40hip_frame_lf_group_plane's planes
extern "C" int j40hip_frame_sharpness(const j40hip_frame *h, int64_t gg, int16_t *out) {
	if (!h || gg < 0 || (size_t) gg >= h->frame.lf_groups.size()) return -1;
	const LfGroup &g = h->frame.lf_groups[(size_t) gg];
	if (g.sharpness.size() != (size_t) g.width8 * (size_t) g.height8) return -1;
	memcpy(out, g.sharpness.data(), g.sharpness.size() * 2);
	return 0;
}
// known-answer / measuring hook: k_ycbcr_tail alone (include/j40hip.h)
extern "C" uint32_t j40hip_kat_device_ycbcr_tail(const float *const planes_dev[3], const int32_t plane_dims[9], const int32_t shifts[6], int32_t width, int32_t height, int32_t bpp, int32_t format, void *out_dev, size_t stride_bytes, void *stream) {
	if (format != J40HIP_U8X4 && format != J40HIP_U16X4) return ERR4('U', 'f', 'm', '?');
	const size_t pb = format == J40HIP_U16X4 ? 8 : 4;
	if (!planes_dev || !plane_dims || !shifts || !out_dev || bpp < 8 || bpp > 15 || width < 1 || height < 1) return ERR_RNGE;
	if (stride_bytes < pb * (size_t) width || stride_bytes % pb || (uintptr_t) out_dev % pb) return ERR_RNGE;
	YcbcrTail t;
	for (int c = 0; c < 3; ++c) {
		t.plane[c] = planes_dev[c]; t.pitch[c] = plane_dims[3 * c]; t.pw[c] = plane_dims[3 * c + 1]; t.ph[c] = plane_dims[3 * c + 2];
		t.hshift[c] = shifts[2 * c]; t.vshift[c] = shifts[2 * c + 1];
		if ((uintptr_t) planes_dev[c] % 4) return ERR_RNGE;
	}
	t.width = width; t.height = height;
	if (!ycbcr_tail_valid(t)) return ERR_RNGE;
	ycbcr_tail_scale(&t, bpp, format == J40HIP_U16X4);
	launch_ycbcr_tail(t, (uint8_t *) out_dev, stride_bytes, (hipStream_t) stream, format == J40HIP_U16X4);
	return hipGetLastError() == hipSuccess ? 0 : ERR_GPU;
}
// staged hook: plane c of the last decode through the YCbCr path as the tail read it, tightly packed (include/j40hip.h)
extern "C" uint32_t j40hip_frame_read_ycbcr(j40hip_frame *h, int c, float *out) {
	if (!h || !h->dev || !h->last.ycbcr_used || c < 0 || c > 2 || !out || !h->dev->ycc_read.plane[c]) return ERR_RNGE;
	const j40hip_device_state::YccRead &r = h->dev->ycc_read;
	if (hipSetDevice(h->dev->device) != hipSuccess) return ERR_GPU;
	return hipMemcpy2D(out, (size_t) r.pw[c] * 4, r.plane[c], (size_t) r.pitch[c] * 4, (size_t) r.pw[c] * 4, (size_t) r.ph[c], hipMemcpyDeviceToHost) == hipSuccess ? 0 : ERR_GPU;
}

// after a decode that ran the filters (synchronised): stage 0 the samples as the inverse transforms left them, 1 the filtered ones --
// three planes of width * height floats (X, Y, B); stage 2: the reciprocal-sigma plane (w8 * h8 floats)
// (a Modular frame of an XYB image with the switch in force, stage 0: k_modular_to_xyb over the integer planes the last decode left --
// "rnge" where that decode covered part of the frame, a region's groups or a group range: the planes outside it are stale)
static uint32_t read_modular_xyb(j40hip_frame *h, float *out) {
	j40hip_device_state *st = h->dev;
	if (!h->last.modular_xyb_whole) return ERR_RNGE;
	const FrameHeader &fh = h->frame.fh;
	const size_t plane = (size_t) fh.width * (size_t) fh.height;
	if (!out || st->final_planes.size() < 3) return ERR_RNGE;
	if (hipSetDevice(st->device) != hipSuccess) return ERR_GPU;
	ScopedBlock block;
	if (!block.ensure(st->device, sizeof(float) * 3 * plane, true)) return ERR_MEM;
	float *d = (float *) block.ptr;
	launch_modular_to_xyb(st->final_planes[0], st->final_planes[1], st->final_planes[2], fh.width, 0, 0, fh.width, fh.height, modular_xyb_consts(h->frame), d, d + plane, d + 2 * plane, (size_t) fh.width, nullptr);
	if (hipGetLastError() != hipSuccess || hipStreamSynchronize(nullptr) != hipSuccess) return ERR_GPU;
	return hipMemcpy(out, d, sizeof(float) * 3 * plane, hipMemcpyDeviceToHost) == hipSuccess ? 0 : ERR_GPU;
}
extern "C" uint32_t j40hip_frame_read_xyb(j40hip_frame *h, int stage, float *out) {
	// (stage 3, a frame with patches: the planes the last decode's tail read, after k_patch_blend)
	// (tail_planes names a buffer of this upload or nothing: a release of the device state forgets it)
	// (stage 4, a frame with noise: likewise, after k_noise_add. With both, what stood between the two kernels is gone: stage 3 is "rnge")
	// (stage 5, an upsampled frame: the shown-size planes k_upsample wrote and the tail read; stages 0 and 1 stay the coded planes)
	if (stage == 5) return guarded([&]() -> uint32_t {
		if (!h || !h->dev || !h->last.tail_planes || !h->last.coded_planes || h->frame.fh.upsampling <= 1 || !out) return ERR_RNGE;
		if (hipSetDevice(h->dev->device) != hipSuccess || hipDeviceSynchronize() != hipSuccess) return ERR_GPU;
		return hipMemcpy(out, h->last.tail_planes, sizeof(float) * 3 * (size_t) h->frame.fh.shown_width() * (size_t) h->frame.fh.shown_height(), hipMemcpyDeviceToHost) == hipSuccess ? 0 : ERR_GPU;
	});
	// (stage 6, a frame with splines: likewise, after k_spline_draw -- "rnge" where noise follows, stage 4 then has the planes after both.
	// Stage 3 of a frame with patches and splines: the copy render_planes kept of the planes between k_patch_blend and k_spline_draw,
	// with or without noise behind them)
	if (stage == 3 || stage == 4 || stage == 6) return guarded([&]() -> uint32_t {
		if (!h || !h->dev || !h->last.tail_planes || !out) return ERR_RNGE;
		const FrameHeader &fh = h->frame.fh;
		const bool kept = stage == 3 && fh.has_patches && fh.has_splines;
		if (kept && !h->last.patched_planes) return ERR_RNGE;
		if (kept ? false : stage == 3 ? !fh.has_patches || fh.has_noise : stage == 6 ? !fh.has_splines || fh.has_noise : !fh.has_noise) return ERR_RNGE;
		if (hipSetDevice(h->dev->device) != hipSuccess || hipDeviceSynchronize() != hipSuccess) return ERR_GPU;
		return hipMemcpy(out, kept ? h->last.patched_planes : h->last.tail_planes, sizeof(float) * 3 * (size_t) h->frame.fh.width * (size_t) h->frame.fh.height, hipMemcpyDeviceToHost) == hipSuccess ? 0 : ERR_GPU;
	});
	if (h && h->dev && h->dev->is_modular && stage == 0 && h->last.modular_xyb_used && j40hip_modular_xyb_on(h)) return guarded([&] { return read_modular_xyb(h, out); });
	// (the colour mode without the filters: the planes the last decode's k_colour_tail read, stages 0 and 1 alike)
	if (h && h->dev && !h->last.restore_ran && h->last.colour_used && h->last.tail_planes && (stage == 0 || stage == 1) && out) {
		if (hipSetDevice(h->dev->device) != hipSuccess) return ERR_GPU;
		const float *coded = h->frame.fh.upsampling > 1 ? h->last.coded_planes : h->last.tail_planes;   // (an upsampled frame's tail read the stretched planes)
		return coded && hipMemcpy(out, coded, sizeof(float) * 3 * (size_t) h->frame.fh.width * (size_t) h->frame.fh.height, hipMemcpyDeviceToHost) == hipSuccess ? 0 : ERR_GPU;
	}
	if (!h || !h->dev || !h->last.restore_ran || !h->dev->d_xyb) return ERR_RNGE;
	j40hip_device_state *st = h->dev;
	const FrameHeader &fh = h->frame.fh;
	const size_t plane = (size_t) fh.width * (size_t) fh.height, cells = (size_t) ((fh.width + 7) / 8) * (size_t) ((fh.height + 7) / 8);
	if (hipSetDevice(st->device) != hipSuccess) return ERR_GPU;
	if (stage == 2) return hipMemcpy(out, st->d_sigma, cells * 4, hipMemcpyDeviceToHost) == hipSuccess ? 0 : ERR_GPU;
	if (stage == 1) return hipMemcpy(out, st->d_restored, 3 * plane * 4, hipMemcpyDeviceToHost) == hipSuccess ? 0 : ERR_GPU;
	// stage 0: the planes the pixel kernels wrote are the filters' first input; they survive only when the result lies in the other buffer
	// pair at every step's end -- re-run the pixel kernels into the spare buffer instead
	const float *src = st->d_xyb;
	const FrameHeader::Restoration &r = fh.restoration;
	const int steps = (r.gab ? 1 : 0) + (r.epf_iters >= 3 ? 3 : r.epf_iters);
	if (steps >= 2) {   // d_xyb has been written over by the second step: once more, into whichever buffer the result does not occupy
		float *spare = st->d_restored == st->d_xyb ? st->d_xyb_tmp : st->d_xyb;
		launch_vardct_frame(st->plan, st->class_start, st->d_vb_sorted, st->d_large_scratch, K2Target{spare, (size_t) fh.width * 4, OutMode::XYB, 0}, nullptr);
		if (hipStreamSynchronize(nullptr) != hipSuccess) return ERR_GPU;
		src = spare;
	}
	return hipMemcpy(out, src, 3 * plane * 4, hipMemcpyDeviceToHost) == hipSuccess ? 0 : ERR_GPU;
}
// m[3] and the 15 colour constants of j40hip_frame_colour_consts as the kernels take them: by value (ModXybConsts) and as a DevFrame's fields
static void kat_colour_consts(const float *m, const float *cc15, int32_t bpp, ModXybConsts *k, DevFrame *df) {
	memset(df, 0, sizeof *df);
	for (int c = 0; c < 3; ++c) { k->m[c] = m ? m[c] : 0.0f; k->cc.opsin_bias[c] = df->opsin_bias[c] = cc15[9 + c]; k->cc.cbrt_opsin_bias[c] = df->cbrt_opsin_bias[c] = cbrtf(cc15[9 + c]); }
	for (int i = 0; i < 9; ++i) k->cc.m[i] = df->opsin_inv_mat[i] = cc15[i];
	k->cc.itscale = df->itscale = 255.0f / cc15[12]; k->cc.bpp = df->bpp = bpp;
}
// known-answer / measuring hook: the Modular XYB kernels on caller-supplied planes (include/j40hip.h)
extern "C" uint32_t j40hip_kat_device_modular_xyb(const void *const planes_dev[3], const void *alpha_dev, int32_t sample_bytes, int32_t width, int32_t height, const float m[3], const float colour_consts[15],
		int32_t bpp, int32_t format, void *fused_dev, void *two_kernel_dev, size_t stride_bytes, float *xyb_dev, void *stream) {
	return guarded([&]() -> uint32_t {
		if (format != J40HIP_U8X4 && format != J40HIP_U16X4) return ERR4('U', 'f', 'm', '?');
		const size_t pb = format == J40HIP_U16X4 ? 8 : 4;
		if (!planes_dev || !planes_dev[0] || !planes_dev[1] || !planes_dev[2] || !m || !colour_consts || !fused_dev || !two_kernel_dev || !xyb_dev) return ERR_RNGE;
		if ((sample_bytes != 2 && sample_bytes != 4) || width <= 0 || height <= 0 || width > (1 << 28) || height > (1 << 28) || bpp < 8 || bpp > 16 || (bpp == 16 && sample_bytes == 2)) return ERR_RNGE;
		if (stride_bytes < pb * (size_t) width || stride_bytes % pb || (uintptr_t) fused_dev % pb || (uintptr_t) two_kernel_dev % pb) return ERR_RNGE;
		for (int c = 0; c < 3; ++c) if ((uintptr_t) planes_dev[c] % (size_t) sample_bytes) return ERR_RNGE;
		if ((uintptr_t) alpha_dev % (size_t) sample_bytes || (uintptr_t) xyb_dev % 4) return ERR_RNGE;
		int device = 0;
		if (hipGetDevice(&device) != hipSuccess || !ensure_constant_tables(device)) return ERR_GPU;
		hipStream_t s = (hipStream_t) stream;
		ModXybConsts k;
		DevFrame df;
		kat_colour_consts(m, colour_consts, bpp, &k, &df);
		df.width = width; df.height = height;
		auto pp = [&](const void *p) { return PlanePtr{(uint8_t *) const_cast<void *>(p), sample_bytes}; };
		launch_modular_xyb_pack(pp(planes_dev[0]), pp(planes_dev[1]), pp(planes_dev[2]), pp(alpha_dev), width, height, k, (uint8_t *) fused_dev, stride_bytes, s, pb == 8);
		// the two-kernel route: the planes, the VarDCT colour tail's kernel over them (A opaque), A from the alpha plane as the pack kernels render it
		const size_t plane = (size_t) width * (size_t) height;
		launch_modular_to_xyb(pp(planes_dev[0]), pp(planes_dev[1]), pp(planes_dev[2]), width, 0, 0, width, height, k, xyb_dev, xyb_dev + plane, xyb_dev + 2 * plane, (size_t) width, s);
		j40hip_device_state tmp; tmp.device = device;
		bool ok = true;
		DevFrame *d_frame = tmp.upload(&df, 1, s, ok);
		if (ok) {
			launch_xyb_to_rgba(xyb_dev, (size_t) width, d_frame, width, height, (uint8_t *) two_kernel_dev, stride_bytes, s, pb == 8);
			if (alpha_dev) launch_alpha_from_plane(pp(alpha_dev), width, height, bpp, (uint8_t *) two_kernel_dev, stride_bytes, s, pb == 8);
			ok = hipGetLastError() == hipSuccess;
		}
		if (hipStreamSynchronize(s) != hipSuccess) ok = false;   // (df and the uploaded copy live until here)
		for (auto &b : tmp.buffers) b.release();
		tmp.buffers.clear();
		return ok ? 0 : ERR_GPU;
	});
}
// known-answer / measuring hook: k_colour_tail on caller-supplied planes, enqueued and not waited for (include/j40hip.h)
extern "C" uint32_t j40hip_kat_device_colour_tail(const float *xyb_dev, int32_t width, int32_t height, const float colour_consts[15], const int32_t enc[16], const float lum[3],
		int32_t bpp, const float *table_dev, const int32_t table_range[2], int32_t format, void *out_dev, size_t stride_bytes, void *stream) {
	return guarded([&]() -> uint32_t {
		if (format != J40HIP_U8X4 && format != J40HIP_U16X4) return ERR4('U', 'f', 'm', '?');
		const size_t pb = format == J40HIP_U16X4 ? 8 : 4;
		if (!xyb_dev || !colour_consts || !enc || !lum || !out_dev || width <= 0 || height <= 0 || width > (1 << 18) || height > (1 << 18) || bpp < 8 || bpp > 16) return ERR_RNGE;
		if (stride_bytes < pb * (size_t) width || stride_bytes % pb || (uintptr_t) out_dev % pb || (uintptr_t) xyb_dev % 4 || !(colour_consts[12] > 0.0f)) return ERR_RNGE;
		if (table_dev && (bpp != 8 || !table_range || table_range[0] < 0 || table_range[1] < table_range[0] || table_range[1] - table_range[0] + 1 > COLOUR_BUCKETS_MAX || (uintptr_t) table_dev % 4)) return ERR_RNGE;
		const ColourEncoding ce = colour::encoding_from_words(enc);
		if (!ce.have_gamma && ce.transfer != 1 && ce.transfer != 8 && ce.transfer != 13 && ce.transfer != 16 && ce.transfer != 17 && ce.transfer != 18) return ERR_UCS;
		if (ce.have_gamma && (ce.gamma <= 0 || ce.gamma > 10000000)) return ERR_UCS;
		ModXybConsts k; DevFrame df;
		kat_colour_consts(nullptr, colour_consts, bpp, &k, &df);
		ColourTailParams p;
		memset(&p, 0, sizeof p);
		p.cc = k.cc;
		const double lumd[3] = {lum[0], lum[1], lum[2]};
		p.curve = colour::curve_of(ce, colour_consts[12], lumd);
		if (table_dev) { p.table = table_dev; p.blo = table_range[0]; p.bhi = table_range[1]; p.table_floats = COLOUR_THRESHOLDS + (p.bhi - p.blo + 1 + 3) / 4; }
		launch_colour_tail(xyb_dev, (size_t) width, p, width, height, (uint8_t *) out_dev, stride_bytes, (hipStream_t) stream, pb == 8);
		return hipGetLastError() == hipSuccess ? 0 : ERR_GPU;
	});
}
// measuring hooks (tools/modxyb_probe.py; include/j40hip.h)
extern "C" size_t j40hip_kat_device_colour_frame(const float colour_consts[15], int32_t bpp, void *frame_dev, size_t bytes) {
	if (!colour_consts || !frame_dev || bytes < sizeof(DevFrame)) return sizeof(DevFrame);
	ModXybConsts k; DevFrame df;
	kat_colour_consts(nullptr, colour_consts, bpp, &k, &df);
	return hipMemcpy(frame_dev, &df, sizeof df, hipMemcpyHostToDevice) == hipSuccess ? sizeof(DevFrame) : 0;   // (0: the copy failed)
}
extern "C" uint32_t j40hip_kat_device_modular_xyb_launch(int32_t kernel, const void *const in_dev[3], int32_t sample_bytes, int32_t width, int32_t height, const float m[3], const float colour_consts[15],
		int32_t bpp, int32_t format, void *out_dev, size_t stride_bytes, const void *frame_dev, void *stream) {
	return guarded([&]() -> uint32_t {
	if (format != J40HIP_U8X4 && format != J40HIP_U16X4) return ERR4('U', 'f', 'm', '?');
	const size_t pb = format == J40HIP_U16X4 ? 8 : 4;
	if (kernel < 0 || kernel > 2 || !in_dev || !in_dev[0] || !in_dev[1] || !in_dev[2] || !m || !colour_consts || !out_dev || width <= 0 || height <= 0 || bpp < 8 || bpp > 16) return ERR_RNGE;
	if ((kernel != 2 && sample_bytes != 2 && sample_bytes != 4) || (kernel == 2 && !frame_dev) || stride_bytes < pb * (size_t) width || stride_bytes % pb || (uintptr_t) out_dev % pb) return ERR_RNGE;
	for (int c = 0; c < 3; ++c) if ((uintptr_t) in_dev[c] % (size_t) (kernel == 2 ? 4 : sample_bytes)) return ERR_RNGE;
	int device = 0;
	if (hipGetDevice(&device) != hipSuccess || !ensure_constant_tables(device)) return ERR_GPU;
	ModXybConsts k; DevFrame df;
	kat_colour_consts(m, colour_consts, bpp, &k, &df);
	auto pp = [&](const void *p) { return PlanePtr{(uint8_t *) const_cast<void *>(p), sample_bytes}; };
	const PlanePtr none = {nullptr, sample_bytes};
	if (kernel == 0) launch_modular_xyb_pack(pp(in_dev[0]), pp(in_dev[1]), pp(in_dev[2]), none, width, height, k, (uint8_t *) out_dev, stride_bytes, (hipStream_t) stream, pb == 8);
	else if (kernel == 1) launch_pack_planes(pp(in_dev[0]), pp(in_dev[1]), pp(in_dev[2]), none, width, height, bpp, (uint8_t *) out_dev, stride_bytes, (hipStream_t) stream, pb == 8);
	else {
		if ((const float *) in_dev[1] != (const float *) in_dev[0] + (size_t) width * (size_t) height || (const float *) in_dev[2] != (const float *) in_dev[1] + (size_t) width * (size_t) height) return ERR_RNGE;   // (one behind the other)
		launch_xyb_to_rgba((const float *) in_dev[0], (size_t) width, (const DevFrame *) frame_dev, width, height, (uint8_t *) out_dev, stride_bytes, (hipStream_t) stream, pb == 8);
	}
	return hipGetLastError() == hipSuccess ? 0 : ERR_GPU;
	});
}
extern "C" float j40hip_frame_restoration_ms(const j40hip_frame *h) { return h && h->dev ? h->dev->restore_ms : 0.0f; }
// known-answer hook: the filter kernels on caller-supplied planes ([3][h][w] floats, in place), a w8*h8 sharpness map and the HfMul
// reciprocal of the varblock covering each cell; mode 1 / 2 as j40hip_frame_set_restoration; sigma_out (optional): w8*h8 floats
extern "C" uint32_t j40hip_kat_device_restoration(float *xyb, int32_t w, int32_t h, const int16_t *sharpness, const float *hfmul_inv, const j40hip_restoration *r, int mode, int device, float *sigma_out) {
	return guarded([&]() -> uint32_t {
		if (!xyb || !r || w < 1 || h < 1 || j40hip_device_count() <= device || hipSetDevice(device) != hipSuccess) return ERR_GPU;
		if (!ensure_constant_tables(device)) return ERR_GPU;
		FrameHeader fh;
		fh.width = w; fh.height = h;
		fh.restoration.gab = r->gab_enabled != 0;
		for (int c = 0; c < 3; ++c) for (int j = 0; j < 2; ++j) fh.restoration.gab_weights[c][j] = r->gab_weights[c][j];
		fh.restoration.epf_iters = r->epf_iters;
		for (int i = 0; i < 8; ++i) fh.restoration.sharp_lut[i] = r->epf_sharp_lut[i];
		for (int c = 0; c < 3; ++c) fh.restoration.channel_scale[c] = r->epf_channel_scale[c];
		fh.restoration.quant_mul = r->epf_quant_mul; fh.restoration.pass0_sigma_scale = r->epf_pass0_sigma_scale; fh.restoration.pass2_sigma_scale = r->epf_pass2_sigma_scale;
		fh.restoration.border_sad_mul = r->epf_border_sad_mul;
		RestoreParams p;
		if (uint32_t e = restore_params(fh, mode, &p)) return e;
		if (fh.restoration.gab && w < 2) return ERR_TODO;
		const size_t plane = (size_t) w * (size_t) h, cells = (size_t) p.w8 * (size_t) p.h8;
		if (r->epf_iters > 0) { uint16_t ub = 0; for (size_t i = 0; i < cells; ++i) ub |= (uint16_t) sharpness[i]; if (!(ub < 8)) return ERR4('s', 'h', 'r', 'p'); }
		j40hip_device_state tmp; tmp.device = device;
		bool ok = true;
		float *d_a = tmp.upload(xyb, 3 * plane, nullptr, ok), *d_b = tmp.scratch<float>(3 * plane, ok), *d_sigma = tmp.scratch<float>(cells + 64, ok);
		if (ok && r->epf_iters > 0) {
			int16_t *d_sh = tmp.upload(sharpness, cells, nullptr, ok);
			float *d_hf = tmp.upload(hfmul_inv, cells, nullptr, ok);
			if (ok) { (void) hipMemsetAsync(d_sigma + cells, 0, 4, nullptr); launch_epf_sigma_cells(d_sh, d_hf, p, d_sigma, (uint32_t *) (d_sigma + cells), nullptr); }
		}
		if (ok) {
			const float *res = launch_restoration(d_a, d_b, (size_t) w, p, fh.restoration.gab, r->epf_iters, d_sigma, nullptr);
			ok = hipMemcpy(xyb, res, 3 * plane * 4, hipMemcpyDeviceToHost) == hipSuccess;
			if (ok && sigma_out && r->epf_iters > 0) ok = hipMemcpy(sigma_out, d_sigma, cells * 4, hipMemcpyDeviceToHost) == hipSuccess;
		}
		(void) hipDeviceSynchronize();
		for (auto &b : tmp.buffers) b.release();
		tmp.buffers.clear();
		return ok ? 0 : ERR_GPU;
	});
}

extern "C" uint32_t j40hip_frame_read_coeffs(j40hip_frame *h, int64_t gg, int c, float *out) {
	if (!h || !h->dev || h->dev->is_modular) return ERR_GPU;
	j40hip_device_state *st = h->dev;
	const LfGroup &g = h->frame.lf_groups[(size_t) gg];
	size_t base = 0;
	for (int64_t i = 0; i < gg; ++i) base += h->frame.lf_groups[(size_t) i].blocks.size();
	if (!st->plan.events) {   // dense planes, canonical order
		return hipMemcpy(out, st->plan.coeffs[c] + base * 64, sizeof(float) * g.blocks.size() * 64, hipMemcpyDeviceToHost) == hipSuccess ? 0 : ERR_GPU;
	}
	// sparse: expand the events of this LF group's blocks into the canonical layout the reference keeps
	std::vector<uint32_t> table(4 * st->num_blocks);
	if (hipMemcpy(table.data(), st->plan.block_events, sizeof(uint32_t) * table.size(), hipMemcpyDeviceToHost) != hipSuccess) return ERR_GPU;
	memset(out, 0, sizeof(float) * g.blocks.size() * 64);
	std::vector<CoeffEvent> ev;
	if (!host_vb_sorted(st)) return ERR_GPU;
	for (const DevVarblock &vb : st->vb_sorted) {
		if ((size_t) vb.llf_base < base || (size_t) vb.llf_base >= base + g.blocks.size()) continue;   // another LF group's block
		const uint32_t *be = table.data() + 4 * (size_t) vb.blk;
		const uint32_t skip = c == 1 ? 0 : c == 0 ? be[1] : be[1] + be[2], n = be[c == 1 ? 1 : c == 0 ? 2 : 3];   // emission order Y, X, B
		if (!n) continue;
		ev.resize(n);
		if (hipMemcpy(ev.data(), st->plan.events + be[0] + skip, sizeof(CoeffEvent) * n, hipMemcpyDeviceToHost) != hipSuccess) return ERR_GPU;
		const std::vector<int32_t> &order = h->frame.orders[0][DCT_SELECT[vb.dctsel].order_idx][(size_t) c];
		float *blk = out + ((size_t) vb.llf_base - base) * 64;
		for (const CoeffEvent &e : ev) blk[order[coeff_event_pos(e)]] = (float) coeff_event_value(e);
	}
	return 0;
}

extern "C" uint32_t j40hip_frame_read_plane_i16(j40hip_frame *h, int c, int16_t *out) {
	if (!h || !h->dev || !h->dev->is_modular) return ERR_GPU;
	j40hip_device_state *st = h->dev;
	if (c < 0 || (size_t) c >= st->final_planes.size()) return ERR_RNGE;
	const size_t n = (size_t) st->final_w[(size_t) c] * (size_t) st->final_h[(size_t) c];
	if (st->mod_wide) return ERR_TODO;   // (int32 planes: j40hip_frame_read_plane_i32)
	if (hipMemcpy(out, st->final_planes[(size_t) c].p, n * 2, hipMemcpyDeviceToHost) != hipSuccess) return ERR_GPU;
	return 0;
}
extern "C" uint32_t j40hip_frame_read_plane_i32(j40hip_frame *h, int c, int32_t *out) {
	if (!h || !h->dev || !h->dev->is_modular) return ERR_GPU;
	j40hip_device_state *st = h->dev;
	if (c < 0 || (size_t) c >= st->final_planes.size()) return ERR_RNGE;
	if (!st->mod_wide) return ERR_TODO;
	const size_t n = (size_t) st->final_w[(size_t) c] * (size_t) st->final_h[(size_t) c];
	if (hipMemcpy(out, st->final_planes[(size_t) c].p, n * 4, hipMemcpyDeviceToHost) != hipSuccess) return ERR_GPU;
	return 0;
}
// wide Modular frames (include/j40hip.h)
extern "C" void j40hip_frame_wide(const j40hip_frame *h, int32_t out[4]) {
	if (!out) return;
	memset(out, 0, sizeof(int32_t) * 4);
	if (!h) return;
	out[0] = h->frame.wide() ? 1 : 0; out[1] = h->frame.im.bpp; out[2] = h->last.wide_used ? 1 : 0;
	out[3] = h->dev && h->dev->is_modular ? (h->dev->mod_wide ? 4 : 2) : 0;
}

// known-answer hooks: n floats through the pixel kernels' sRGB tail on the device (launch(dv, dout)), one sample of T each
template <typename T, typename L> static uint32_t kat_srgb(const float *v_host, size_t n, T *out_host, L launch) {
	if (j40hip_device_count() <= 0) return ERR_GPU;
	float *dv = nullptr; T *dout = nullptr;
	bool ok = hipMalloc((void **) &dv, n * 4 + 16) == hipSuccess && hipMalloc((void **) &dout, n * sizeof(T) + 16) == hipSuccess;
	ok = ok && hipMemcpy(dv, v_host, n * 4, hipMemcpyHostToDevice) == hipSuccess;
	if (ok) { int dev = 0; ok = hipGetDevice(&dev) == hipSuccess && ensure_constant_tables(dev); if (ok) launch(dv, dout); }
	ok = ok && hipMemcpy(out_host, dout, n * sizeof(T), hipMemcpyDeviceToHost) == hipSuccess;
	if (dv) (void) hipFree(dv);
	if (dout) (void) hipFree(dout);
	return ok ? 0 : ERR_GPU;
}
extern "C" uint32_t j40hip_kat_device_srgb_u8(const float *v_host, size_t n, uint8_t *out_host) {
	return kat_srgb(v_host, n, out_host, [&](const float *dv, uint8_t *dout) { launch_kat_srgb_u8(dv, n, dout, nullptr); });
}
extern "C" uint32_t j40hip_kat_device_srgb_u16(const float *v_host, size_t n, int32_t bpp, uint16_t *out_host) {
	if (bpp < 8 || bpp > 15) return ERR_RNGE;
	return kat_srgb(v_host, n, out_host, [&](const float *dv, uint16_t *dout) { launch_kat_srgb_u16(dv, n, bpp, dout, nullptr); });
}
