// j40_amd/csrc/device/runtime_lfp.hip -- the LF preview (lf_preview.hip; include/j40hip.h, j40hip_frame_decode_lf): a frame's 1:8
// picture from its LF sections alone
#include "runtime_state.hpp"
#include "orient_dev.h"

// does the frame hold LF integers: parsed from a bitstream (frames built from a plan view carry LLF coefficients only)
static bool lfp_has_integers(const j40hip_frame *h) {
	for (const LfGroup &gg : h->frame.lf_groups) if (gg.lfraw[0].size() != (size_t) gg.width8 * (size_t) gg.height8) return false;
	return !h->frame.lf_groups.empty();
}

// the frame's preview state on its device: the LfGroups as the kernel reads them and, unless the plan holds them, the LF integers in an
// allocation of their own (copied on `s` from st->lfp_host, which stays with the frame)
static uint32_t lfp_prepare(j40hip_frame *h, hipStream_t s) {
	j40hip_device_state *st = h->dev;
	if (st->lfp_ready) return 0;
	const Frame &fr = h->frame;
	const size_t nlf = fr.lf_groups.size();
	std::vector<DevLfpGroup> groups(nlf);
	size_t cells = 0;
	for (size_t g = 0; g < nlf; ++g) {
		const LfGroup &gg = fr.lf_groups[g];
		DevLfpGroup &d = groups[g];
		d.x8 = gg.left / 8; d.y8 = gg.top / 8; d.width8 = gg.width8; d.height8 = gg.height8; d.cell_base = (int32_t) cells;   // (plan_build's layout)
		for (int c = 0; c < 3; ++c) d.mult_lf[c] = gg.mult_lf[c];
		cells += (size_t) gg.width8 * (size_t) gg.height8;
	}
	if (cells >= ((size_t) 1 << 31)) return ERR_TODO;
	const bool own = st->plan.lfraw[0] == nullptr;
	const size_t o_raw = (sizeof(DevLfpGroup) * nlf + 255) & ~(size_t) 255, bytes = o_raw + (own ? 3 * ((sizeof(int16_t) * cells + 255) & ~(size_t) 255) : 0);
	st->lfp_host.assign(bytes, 0);
	memcpy(st->lfp_host.data(), groups.data(), sizeof(DevLfpGroup) * nlf);
	if (own) for (int c = 0; c < 3; ++c) {
		int16_t *dst = (int16_t *) (st->lfp_host.data() + o_raw + (size_t) c * ((sizeof(int16_t) * cells + 255) & ~(size_t) 255));
		for (size_t g = 0; g < nlf; ++g) std::copy(fr.lf_groups[g].lfraw[c].begin(), fr.lf_groups[g].lfraw[c].end(), dst + groups[g].cell_base);
	}
	bool ok = true;
	uint8_t *d = st->upload(st->lfp_host.data(), bytes, s, ok);   // (a buffer of the frame's own: freed with it)
	if (!ok) return ERR_GPU;
	DevLfpFrame &p = st->lfp;
	p.groups = (const DevLfpGroup *) d;
	for (int c = 0; c < 3; ++c) p.lfraw[c] = own ? (const int16_t *) (d + o_raw + (size_t) c * ((sizeof(int16_t) * cells + 255) & ~(size_t) 255)) : st->plan.lfraw[c];
	DevFrame df;
	fill_frame_constants(fr, &df);   // (the colour constants exactly as the pixel kernels get them)
	for (int k = 0; k < 9; ++k) p.opsin_inv_mat[k] = df.opsin_inv_mat[k];
	for (int k = 0; k < 3; ++k) { p.opsin_bias[k] = df.opsin_bias[k]; p.cbrt_opsin_bias[k] = df.cbrt_opsin_bias[k]; p.inv_m_lf[k] = (float) (fr.global_scale * fr.quant_lf) / fr.m_lf_scaled[k] / 65536.0f; }   // j40.h:6497
	p.itscale = df.itscale; p.kx_lf = df.kx_lf; p.kb_lf = df.kb_lf; p.bpp = df.bpp; p.smooth = fr.fh.skip_adapt_lf_smooth ? 0 : 1;
	st->lfp_ready = true;
	return 0;
}

// j40hip_frame_upload of an LF-only frame: the preview's state and nothing else
uint32_t j40hip_rt::upload_lf_only(j40hip_frame *h, int device, hipStream_t s) {
	if (h->frame.fh.is_modular) return ERR_TODO;
	if (h->frame.im.bpp < 8 || h->frame.im.exp_bits || h->frame.im.grey || h->frame.fh.do_ycbcr) return ERR_TODO;   // (what build_vardct_plan refuses)
	j40hip_device_state *st = new j40hip_device_state();
	h->dev = st; st->device = device;
	uint32_t err = ensure_constant_tables(device) ? lfp_prepare(h, s) : ERR_GPU;
	if (!err && hipStreamSynchronize(s) != hipSuccess) err = ERR_GPU;
	if (err) j40hip_release_device(h);
	return err;
}

// The per-call arrays of a preview launch (frames with their outputs, the work list) go up through a pinned buffer and a device buffer
// borrowed from this pool; an event recorded behind the launch tells the next borrower when both may be written again.
struct LfpArgs { int device; uint8_t *dev, *host; size_t cap; hipEvent_t done; };
static IdlePool<LfpArgs> g_lfp_idle;
static void lfp_args_destroy(LfpArgs &a) {
	if (a.dev) (void) hipFree(a.dev);
	if (a.host) (void) hipHostFree(a.host);
	if (a.done) (void) hipEventDestroy(a.done);
	a.dev = a.host = nullptr; a.done = nullptr; a.cap = 0;
}
static bool lfp_args_borrow(int device, size_t bytes, LfpArgs *out) {
	if (!g_lfp_idle.take(device, out)) {
		*out = LfpArgs{device, nullptr, nullptr, 0, nullptr};
		if (hipEventCreateWithFlags(&out->done, hipEventDisableTiming) != hipSuccess) { out->done = nullptr; return false; }
	}
	if (hipEventSynchronize(out->done) != hipSuccess) { lfp_args_destroy(*out); return false; }   // (the launch that read them last is through)
	if (out->cap < bytes) {
		if (out->dev) (void) hipFree(out->dev);
		if (out->host) (void) hipHostFree(out->host);
		out->dev = out->host = nullptr; out->cap = 0;
		const size_t cap = std::max(bytes + bytes / 2, (size_t) 64 << 10);
		if (hipMalloc((void **) &out->dev, cap) != hipSuccess || hipHostMalloc((void **) &out->host, cap, hipHostMallocDefault) != hipSuccess) { (void) hipGetLastError(); lfp_args_destroy(*out); return false; }
		out->cap = cap;
	}
	return true;
}
void j40hip_rt::lfp_args_shutdown() { g_lfp_idle.drain([](LfpArgs &a) { (void) hipSetDevice(a.device); lfp_args_destroy(a); }); }

// n frames in one launch. mode LFP_U8 / LFP_U16 (the frames' own format; members that disagree "Uof?") or LFP_PLANE (channel `channel`
// as floats, 4 bytes a cell). Everything is checked before anything is copied or launched.
static uint32_t lfp_launch(j40hip_frame *const *frames, int64_t n, void *const *out, const size_t *stride, hipStream_t s, bool plane, int32_t channel) {
	if (n <= 0 || !frames || !out || !stride) return ERR_RNGE;
	if (!frames[0] || !frames[0]->dev) return ERR_GPU;
	const int device = frames[0]->dev->device;
	for (int64_t i = 0; i < n; ++i) {
		j40hip_frame *h = frames[i];
		if (!h || !h->dev || h->dev->device != device) return ERR_GPU;
		if (h->frame.fh.is_modular || h->dev->is_modular || !lfp_has_integers(h)) return ERR_TODO;
		if (!plane && h->output_format != frames[0]->output_format) return ERR4('U', 'o', 'f', '?');
		const size_t w8 = (size_t) (h->frame.fh.width + 7) / 8;
		if (stride[i] < (plane ? 4 : pixel_bytes(h)) * w8) return ERR_RNGE;
	}
	if (hipSetDevice(device) != hipSuccess) return ERR_GPU;
	std::vector<DevLfpFrame> fl((size_t) n);
	std::vector<DevLfpWork> work;
	uint32_t blocks = 0;
	for (int64_t i = 0; i < n; ++i) {
		j40hip_frame *h = frames[i];
		if (uint32_t e = lfp_prepare(h, s)) return e;
		fl[(size_t) i] = h->dev->lfp;
		fl[(size_t) i].out = (uint8_t *) out[i]; fl[(size_t) i].stride = stride[i];
		for (size_t g = 0; g < h->frame.lf_groups.size(); ++g) {
			const LfGroup &gg = h->frame.lf_groups[g];
			const uint64_t nb = ((uint64_t) gg.width8 * (uint64_t) gg.height8 + LFP_LANES - 1) / LFP_LANES;
			if ((uint64_t) blocks + nb >= ((uint64_t) 1 << 31)) return ERR_TODO;
			work.push_back(DevLfpWork{(int32_t) i, (int32_t) g, blocks, 0});
			blocks += (uint32_t) nb;
		}
	}
	if (work.size() >= ((size_t) 1 << 31)) return ERR_TODO;
	const size_t o_work = (sizeof(DevLfpFrame) * fl.size() + 255) & ~(size_t) 255, bytes = o_work + sizeof(DevLfpWork) * work.size();
	LfpArgs a;
	if (!lfp_args_borrow(device, bytes, &a)) return ERR_GPU;
	memcpy(a.host, fl.data(), sizeof(DevLfpFrame) * fl.size());
	memcpy(a.host + o_work, work.data(), sizeof(DevLfpWork) * work.size());
	bool ok = hipMemcpyAsync(a.dev, a.host, bytes, hipMemcpyHostToDevice, s) == hipSuccess;
	if (ok) launch_lf_preview((const DevLfpFrame *) a.dev, (const DevLfpWork *) (a.dev + o_work), (int32_t) work.size(), blocks, plane ? LFP_PLANE : out16(frames[0]) ? LFP_U16 : LFP_U8, channel, s);
	ok = ok && hipGetLastError() == hipSuccess && hipEventRecord(a.done, s) == hipSuccess;
	if (!ok) { (void) hipGetLastError(); (void) hipStreamSynchronize(s); }
	g_lfp_idle.give(a);
	return ok ? 0 : ERR_GPU;
}

extern "C" uint32_t j40hip_frames_decode_lf(j40hip_frame *const *frames, int64_t n, void *const *rgba_dev, const size_t *stride_bytes, void *stream) {
	// many previews in one launch are written in stored order and as sRGB: a member whose orientation or colour mode is in force is refused before anything is launched
	for (int64_t i = 0; frames && i < n; ++i) if (frames[i]) if (uint32_t e = mode_refusal(frames[i], Mode::LfPreviewBatch)) return e;
	return guarded([&] { return lfp_launch(frames, n, rgba_dev, stride_bytes, (hipStream_t) stream, false, 0); });
}

// the preview of one frame, in the image's orientation where that is in force (j40hip_frame_set_orientation): the stored-order preview
// goes to the frame's staging block and k_orient writes `rgba_dev` behind it on `s`, as decode_oriented does for the full decode
static uint32_t lfp_one(j40hip_frame *h, void *rgba_dev, size_t stride_bytes, hipStream_t s) {
	if (!h || !h->dev) return ERR_GPU;
	if (h->frame.fh.use_lf_frame) return ERR_TODO;   // (it holds no LF integers: the LF frame's own handle decodes that picture)
	if (j40hip_colour_on(h)) return ERR_UCS;   // the preview's tail renders sRGB: refused while the colour mode is in force (the float planes, j40hip_frame_read_lf, are not its business)
	h->orient_applied = 0; h->orient_staging_bytes = 0;
	const int32_t o = j40hip_orientation_in_force(h);
	if (o == 1) return lfp_launch(&h, 1, &rgba_dev, &stride_bytes, s, false, 0);
	if (h->frame.fh.is_modular || h->dev->is_modular) return ERR_TODO;   // (lfp_launch's own refusal, before anything is staged)
	j40hip_device_state *st = h->dev;
	const int32_t W = (h->frame.fh.width + 7) / 8, H = (h->frame.fh.height + 7) / 8;
	int32_t ow, oh;
	orient_out_size(W, H, o, &ow, &oh);
	const size_t pb = pixel_bytes(h);
	if (!rgba_dev || stride_bytes < pb * (size_t) ow) return ERR_RNGE;
	if (hipSetDevice(st->device) != hipSuccess) return ERR_GPU;
	size_t img_stride = pb * (size_t) W;
	const size_t bytes = img_stride * (size_t) H;
	if (!st->orient_staging.ensure(st->device, bytes, false)) return ERR_MEM;
	void *img = st->orient_staging.ptr;
	h->orient_staging_bytes = (int64_t) bytes;
	if (uint32_t e = lfp_launch(&h, 1, &img, &img_stride, s, false, 0)) return e;
	launch_orient((const uint8_t *) img, img_stride, (uint8_t *) rgba_dev, stride_bytes, W, H, o, (int32_t) pb, s);
	h->orient_applied = 1;
	return hipGetLastError() == hipSuccess ? 0 : ERR_GPU;
}

extern "C" uint32_t j40hip_frame_decode_lf(j40hip_frame *h, void *rgba_dev, size_t stride_bytes, void *stream) {
	return guarded([&] { return lfp_one(h, rgba_dev, stride_bytes, (hipStream_t) stream); });
}

// the preview (or a plane) in a device buffer of the cache, then to the host; synchronous
static uint32_t lfp_to_host(j40hip_frame *h, void *host, size_t stride_bytes, bool plane, int32_t channel) {
	if (!h || !h->dev) return ERR_GPU;
	if (!host) return ERR_RNGE;
	// (the preview proper comes back in the image's orientation where that is in force: lfp_one; a plane never does)
	const bool turned = !plane && orient_transposes(j40hip_orientation_in_force(h));
	const size_t bytes = stride_bytes * (size_t) (((turned ? h->frame.fh.width : h->frame.fh.height) + 7) / 8);
	if (hipSetDevice(h->dev->device) != hipSuccess) return ERR_GPU;
	ScopedBlock block;
	if (!block.ensure(h->dev->device, bytes, true)) return ERR_GPU;
	void *d = block.ptr;
	uint32_t err = plane ? lfp_launch(&h, 1, &d, &stride_bytes, nullptr, true, channel) : lfp_one(h, d, stride_bytes, nullptr);
	if (!err && hipStreamSynchronize(nullptr) != hipSuccess) err = ERR_GPU;
	if (!err && hipMemcpy(host, d, bytes, hipMemcpyDeviceToHost) != hipSuccess) err = ERR_GPU;
	return err;
}

extern "C" uint32_t j40hip_frame_decode_lf_to_host(j40hip_frame *h, void *rgba_host, size_t stride_bytes) {
	return guarded([&] { return lfp_to_host(h, rgba_host, stride_bytes, false, 0); });
}

extern "C" uint32_t j40hip_frame_read_lf(j40hip_frame *h, int c, float *out) {
	if (c < 0 || c > 2) return ERR_RNGE;
	return guarded([&] { return h ? lfp_to_host(h, out, sizeof(float) * (size_t) ((h->frame.fh.width + 7) / 8), true, c) : ERR_GPU; });
}
