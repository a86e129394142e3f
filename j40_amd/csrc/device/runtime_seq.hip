// j40_amd/csrc/device/runtime_seq.hip -- the device half of a frame sequence (j40hip_sequence, include/j40hip.h): the canvas, its four
// reference slots, the staging image a cropped frame decodes into, and the playback that walks the coded frames.
//
// A coded frame is an ordinary frame handle (capi_host.cpp: j40hip_sequence_frame) and decodes through j40hip_frame_decode. Where it goes:
// a frame that covers the canvas exactly decodes straight into its destination; every other one into the staging image, from where
// k_frame_compose (compose_kernels.hip) puts it onto the canvas. A frame with a blend mode other than Replace (Row::blended) decodes into
// the staging image whatever it covers and goes through k_frame_blend. The destination of a frame that is saved is its slot -- a frame that
// draws over the slot it is saved into touches only its rectangle -- and a shown one is then copied out; a frame that is only shown is
// composed into the caller's image. All on the caller's stream, in order: one staging image serves every frame.
#include "runtime_state.hpp"
#include "compose_dev.h"

struct j40hip_sequence_device {
	int device = -1;
	CacheBlock slot[4], staging;
	size_t slot_stride = 0;
	bool slot_saved[4] = {false, false, false, false};
	// LF frames (J40HIP_SEQ_LFFRAME): LF slot k holds the picture of the last decoded frame of lf_level k + 1 -- three planes of float32
	// (X, Y, B), lf_w x lf_h each, one behind the other; taken at the upload for the largest LF frame the index sends there
	CacheBlock lf_slot[4];
	int32_t lf_w[4] = {0, 0, 0, 0}, lf_h[4] = {0, 0, 0, 0};
	bool lf_filled[4] = {false, false, false, false};
	// patches (J40HIP_SEQ_PATCHES): reference slot k as a reference-only frame fills it -- three planes of float32 (X, Y, B), ref_w x ref_h
	// each, one behind the other; taken at the upload for the largest such frame the index stores there. A slot holds these planes or
	// pixels (`slot`), whichever the playback put there last
	CacheBlock ref_xyb[4];
	int32_t ref_w[4] = {0, 0, 0, 0}, ref_h[4] = {0, 0, 0, 0};
	bool ref_filled[4] = {false, false, false, false};
	int64_t cursor = 0;          // the next coded frame
	int64_t decoded = 0;         // coded frames [0, decoded) have been enqueued since the last rewind
};

namespace {

size_t seq_pixel_bytes(const j40hip_sequence *s) { return s->output_format == J40HIP_U16X4 ? 8 : 4; }

// whether the decode of `h` that has just been enqueued writes an alpha channel of its own (else A is full scale)
bool renders_alpha(const j40hip_frame *h) { return h->dev->is_modular ? h->dev->alpha_channel >= 0 : h->last.alpha_written; }

size_t slot_bytes(const j40hip_sequence *s) { return s->dev->slot_stride * (size_t) s->im.height; }

// what the staging image of a w x h frame takes at the most: rows padded to 16 bytes and up to 15 more each, so that they sit like the
// destination's, up to 15 bytes in front of the first one and 16 behind the last
size_t staging_bound(const j40hip_sequence *s, int32_t w, int32_t h) { return 32 + ((((size_t) w * seq_pixel_bytes(s) + 15) & ~(size_t) 15) + 16) * (size_t) h; }

// Every slot the index saves into and one staging image large enough for each frame that does not cover the canvas exactly or is blended, taken
// where the host may wait for the device (the upload, a change of the output format): taking or growing a block waits for it
// (CacheBlock::ensure), and the playback must not.
bool reserve_blocks(j40hip_sequence *s) {
	j40hip_sequence_device *d = s->dev;
	d->slot_stride = ((size_t) s->im.width * seq_pixel_bytes(s) + 15) & ~(size_t) 15;
	size_t staging = 0, lf_bytes[4] = {0, 0, 0, 0}, ref_bytes[4] = {0, 0, 0, 0};
	for (const j40hip_sequence::Row &row : s->rows) {
		if (row.code) break;
		if (row.stored_xyb) { size_t &b = ref_bytes[row.xyb_slot]; b = std::max(b, sizeof(float) * 3 * (size_t) row.fh.width * (size_t) row.fh.height); continue; }
		if (row.fh.type == 1) { size_t &b = lf_bytes[row.fh.lf_level - 1]; b = std::max(b, sizeof(float) * 3 * (size_t) row.fh.width * (size_t) row.fh.height); continue; }
		if (row.saved && !d->slot[row.fh.save_as_ref].ensure(d->device, slot_bytes(s), false)) return false;
		if (row.blended || !(row.fh.x0 == 0 && row.fh.y0 == 0 && row.fh.width == s->im.width && row.fh.height == s->im.height)) staging = std::max(staging, staging_bound(s, row.fh.width, row.fh.height));
	}
	for (int k = 0; k < 4; ++k) if (lf_bytes[k] && !d->lf_slot[k].ensure(d->device, lf_bytes[k], false)) return false;
	for (int k = 0; k < 4; ++k) if (ref_bytes[k] && !d->ref_xyb[k].ensure(d->device, ref_bytes[k], false)) return false;
	return !staging || d->staging.ensure(d->device, staging, false);
}

// the LF source of a frame with use_lf_frame: the picture in LF slot `slot` as the playback last filled it ("lfno": it never did)
uint32_t bind_lf_source(j40hip_sequence *s, j40hip_frame *h, int32_t slot) {
	j40hip_sequence_device *d = s->dev;
	if (slot < 0 || slot > 3 || !d->lf_filled[slot] || !d->lf_slot[slot].ptr) return ERR4('l', 'f', 'n', 'o');
	const size_t plane = (size_t) d->lf_w[slot] * (size_t) d->lf_h[slot];
	const float *base = (const float *) d->lf_slot[slot].ptr, *planes[3] = {base, base + plane, base + 2 * plane};
	j40hip_frame_bind_lf_source(h, planes, d->lf_w[slot], d->lf_h[slot]);
	return 0;
}

// A frame the playback keeps as planes -- an LF frame (type 1) in its LF slot, a reference-only frame (type 2) in its reference slot: the
// whole frame's XYB planes into `block`, nothing composed, nothing shown; *w, *h, *filled: the slot's bookkeeping
uint32_t play_plane_frame(j40hip_sequence *s, int64_t k, j40hip_frame *h, hipStream_t stream, bool sync, const CacheBlock &block, int32_t *w, int32_t *hh, bool *filled) {
	j40hip_sequence_device *d = s->dev;
	const FrameHeader &fh = s->rows[(size_t) k].fh;
	if (!block.ptr || block.bytes < sizeof(float) * 3 * (size_t) fh.width * (size_t) fh.height) return ERR_GPU;   // (reserve_blocks sized it)
	float *planes = (float *) block.ptr;
	if (uint32_t e = decode_frame_xyb(h, planes, stream)) return e;
	d->decoded = std::max(d->decoded, k + 1);
	if (sync) if (uint32_t e = wait_with_dense_retry(h, d->device, stream, [&] { return decode_frame_xyb(h, planes, stream); })) return e;
	*w = fh.width; *hh = fh.height; *filled = true;
	return hipGetLastError() == hipSuccess ? 0 : ERR_GPU;
}

// the reference slots a frame with patches reads, as the playback last filled them ("ptno": it never did)
uint32_t bind_patch_sources(j40hip_sequence *s, const j40hip_sequence::Row &row, j40hip_frame *h) {
	j40hip_sequence_device *d = s->dev;
	for (int k = 0; k < 4; ++k) {
		const bool read = (row.patches.slots >> k & 1) != 0;
		if (read && (!d->ref_filled[k] || !d->ref_xyb[k].ptr)) return ERR4('p', 't', 'n', 'o');
		j40hip_frame_bind_patch_source(h, k, read ? (const float *) d->ref_xyb[k].ptr : nullptr, read ? d->ref_w[k] : 0, read ? d->ref_h[k] : 0);
	}
	return 0;
}

uint8_t *slot_image(j40hip_sequence *s, int k) {
	const CacheBlock &b = s->dev->slot[k];
	return b.ptr && b.bytes >= slot_bytes(s) ? (uint8_t *) b.ptr : nullptr;
}

// the staging image of a w x h frame whose pixel `fx` of every row sits within 16 bytes like pixel `cx` of the destination's rows
uint8_t *staging_image(j40hip_sequence *s, const uint8_t *dst, size_t dst_stride, int32_t w, int32_t h, int32_t fx, int32_t cx, size_t *stride) {
	const size_t pb = seq_pixel_bytes(s), row = ((size_t) w * pb + 15) & ~(size_t) 15;
	*stride = row + (dst_stride & 15 & ~(pb - 1));
	const size_t lead = ((uintptr_t) dst + (size_t) cx * pb - (size_t) fx * pb) & 15 & ~(pb - 1);
	const CacheBlock &b = s->dev->staging;
	return b.ptr && b.bytes >= lead + *stride * (size_t) h + 16 ? (uint8_t *) b.ptr + lead : nullptr;   // (reserve_blocks sized it for every frame)
}

// Coded frame k onto `out` (null: the frame is not shown). sync: wait for the frame and read its status before it is composed (the
// synchronous entry point), with the "evof" retry.
uint32_t play_frame(j40hip_sequence *s, int64_t k, uint8_t *out, size_t out_stride, hipStream_t stream, bool sync) {
	j40hip_sequence_device *d = s->dev;
	const j40hip_sequence::Row &row = s->rows[(size_t) k];
	if (row.code) return row.code;
	j40hip_frame *h = s->frames[(size_t) k];
	if (!h || !h->dev || h->dev->device != d->device) return ERR_GPU;
	const FrameHeader &fh = row.fh;
	if (fh.type == 1) {   // an LF frame: it may take its own LF image from the next coarser level
		const int slot = fh.lf_level - 1;
		if (slot < 0 || slot > 3) return ERR_GPU;
		if (fh.use_lf_frame) { if (uint32_t e = bind_lf_source(s, h, fh.lf_level)) return e; }
		return play_plane_frame(s, k, h, stream, sync, d->lf_slot[slot], &d->lf_w[slot], &d->lf_h[slot], &d->lf_filled[slot]);
	}
	if (row.stored_xyb) {   // a reference-only frame
		const int slot = row.xyb_slot;
		if (slot < 0 || slot > 3) return ERR_GPU;
		const uint32_t e = play_plane_frame(s, k, h, stream, sync, d->ref_xyb[slot], &d->ref_w[slot], &d->ref_h[slot], &d->ref_filled[slot]);
		if (!e) d->slot_saved[slot] = false;   // (the slot holds planes now: no pixels for a later frame to draw over)
		return e;
	}
	// (the main frame of an LF-frame still takes a scale and the orientation for decodes of its own, capi.hpp: the canvas is full size, stored order)
	if (uint32_t e = mode_refusal(h, Mode::Playback)) return e;
	const int32_t W = s->im.width, H = s->im.height;
	const size_t pb = seq_pixel_bytes(s);
	// where the canvas of this frame is made
	uint8_t *dst = out; size_t dst_stride = out_stride;
	if (row.saved) { dst = slot_image(s, fh.save_as_ref); dst_stride = d->slot_stride; if (!dst) return ERR_GPU; }
	if (!dst) return 0;   // neither shown nor saved: nothing of it is ever seen
	const bool exact = !row.blended && fh.x0 == 0 && fh.y0 == 0 && fh.width == W && fh.height == H;   // decoded where it is wanted
	const ComposeRect r = compose_clip(W, H, fh.x0, fh.y0, fh.width, fh.height);
	uint8_t *img = dst; size_t img_stride = dst_stride;
	if (!exact) { img = staging_image(s, dst, dst_stride, fh.width, fh.height, r.fx, r.cx0, &img_stride); if (!img) return ERR_GPU; }
	if (fh.use_lf_frame) { if (uint32_t e = bind_lf_source(s, h, fh.lf_level)) return e; }   // (its LfGroup tail reads the LF frame's picture)
	if (fh.has_patches) { if (uint32_t e = bind_patch_sources(s, row, h)) return e; }        // (its patches read the reference-only frames' planes)
	uint32_t e = j40hip_frame_decode(h, img, img_stride, stream);
	if (e) return e;
	d->decoded = std::max(d->decoded, k + 1);   // (enqueued: j40hip_sequence_status looks at it, whatever becomes of it)
	if (sync) if ((e = wait_with_dense_retry(h, d->device, stream, [&] { return j40hip_frame_decode(h, img, img_stride, stream); })) != 0) return e;
	if (!exact) {
		const uint8_t *src = d->slot_saved[row.src] ? (const uint8_t *) d->slot[row.src].ptr : nullptr;
		const bool a0 = renders_alpha(h);
		const uint32_t lo = pb == 4 && !a0 ? 0xff000000u : 0u, hi = pb == 8 && !a0 ? 0xffff0000u : 0u;
		if (row.blended) launch_frame_blend(dst, dst_stride, src, d->slot_stride, img, img_stride, W, H, fh.x0, fh.y0, fh.width, fh.height, lo, hi, (int32_t) pb, fh.blend.mode, row.alpha_mode, stream);
		else launch_frame_compose(dst, dst_stride, src, d->slot_stride, img, img_stride, W, H, fh.x0, fh.y0, fh.width, fh.height, lo, hi, (int32_t) pb, stream);
		if (hipGetLastError() != hipSuccess) return ERR_GPU;
	}
	if (row.saved) {
		d->slot_saved[fh.save_as_ref] = true; d->ref_filled[fh.save_as_ref] = false;   // (pixels take the place of a reference-only frame's planes)
		if (out && hipMemcpy2DAsync(out, out_stride, dst, dst_stride, (size_t) W * pb, (size_t) H, hipMemcpyDeviceToDevice, stream) != hipSuccess) return ERR_GPU;
	}
	return 0;
}

uint32_t next_impl(j40hip_sequence *s, void *rgba_dev, size_t stride_bytes, hipStream_t stream, bool sync) {
	if (!s || !rgba_dev) return ERR_RNGE;
	if (!s->dev) return ERR_GPU;
	j40hip_sequence_device *d = s->dev;
	const size_t pb = seq_pixel_bytes(s);
	if (stride_bytes < pb * (size_t) s->im.width || stride_bytes % pb || (uintptr_t) rgba_dev % pb) return ERR_RNGE;
	if (hipSetDevice(d->device) != hipSuccess) return ERR_GPU;
	const int64_t n = (int64_t) s->rows.size();
	for (;;) {
		if (d->cursor >= n) return ERR4('U', 's', 'e', 'q');
		const int64_t k = d->cursor;
		const j40hip_sequence::Row &row = s->rows[(size_t) k];
		if (uint32_t e = play_frame(s, k, row.shown ? (uint8_t *) rgba_dev : nullptr, stride_bytes, stream, sync)) return e;
		d->cursor = k + 1;
		if (row.shown) return 0;
	}
}

} // namespace

extern "C" void j40hip_sequence_release_device(j40hip_sequence *s) {
	if (!s || !s->dev) return;
	(void) hipSetDevice(s->dev->device);
	bool waited = false;
	auto give = [&](CacheBlock &b) { if (b.ptr) { b.release(waited); waited = true; } };   // (one device-wide wait covers them all)
	for (CacheBlock &b : s->dev->slot) give(b);
	for (CacheBlock &b : s->dev->lf_slot) give(b);
	for (CacheBlock &b : s->dev->ref_xyb) give(b);
	give(s->dev->staging);
	delete s->dev;
	s->dev = nullptr;
}

extern "C" uint32_t j40hip_sequence_upload(j40hip_sequence *s, int device) {
	return guarded([&]() -> uint32_t {
		if (!s) return ERR_RNGE;
		if (s->dev && s->dev->device != device) j40hip_sequence_release_device(s);
		for (size_t k = 0; k < s->rows.size(); ++k) {
			if (s->rows[k].code) break;   // (reported when the playback gets there)
			uint32_t e = 0;
			j40hip_frame *h = j40hip_sequence_frame(s, (int64_t) k, &e);
			if (!h) {
				// a frame that does not parse ends the index like one that j40hip_sequence_open refuses: the playback fails there, the
				// frames before it play, and nothing behind it counts
				for (size_t j = k + 1; j < s->frames.size(); ++j) j40hip_frame_free(s->frames[j]);
				s->rows.resize(k + 1); s->frames.resize(k + 1);
				s->rows[k].code = e; s->rows[k].shown = s->rows[k].saved = false;
				break;
			}
			if ((e = j40hip_frame_set_output_format(h, s->output_format)) != 0 || (e = j40hip_frame_upload(h, device)) != 0) return e;
		}
		if (!s->dev) { s->dev = new j40hip_sequence_device(); s->dev->device = device; }
		if (hipSetDevice(device) != hipSuccess || !reserve_blocks(s)) return ERR_GPU;
		return 0;
	});
}

extern "C" uint32_t j40hip_sequence_set_output_format(j40hip_sequence *s, int32_t format) {
	if (!s) return ERR_RNGE;
	if (format != J40HIP_U8X4 && format != J40HIP_U16X4) return ERR4('U', 'f', 'm', '?');
	if (s->dev && s->dev->cursor > 0 && format != s->output_format) return ERR4('U', 'o', 'f', '?');   // (the slots hold pixels of the other format)
	const bool changed = format != s->output_format;
	s->output_format = format;
	for (j40hip_frame *h : s->frames) if (h) h->output_format = format;
	// (the slots and the staging image of pixels twice or half as wide: taken here, where waiting for the device is allowed)
	if (changed && s->dev) return guarded([&]() -> uint32_t { return hipSetDevice(s->dev->device) == hipSuccess && reserve_blocks(s) ? 0 : ERR_GPU; });
	return 0;
}

extern "C" uint32_t j40hip_sequence_next(j40hip_sequence *s, void *rgba_dev, size_t stride_bytes, void *stream) {
	return guarded([&] { return next_impl(s, rgba_dev, stride_bytes, (hipStream_t) stream, false); });
}

extern "C" uint32_t j40hip_sequence_next_to_host(j40hip_sequence *s, void *rgba_host, size_t stride_bytes) {
	return guarded([&]() -> uint32_t {
		if (!s || !rgba_host) return ERR_RNGE;
		if (!s->dev) return ERR_GPU;
		if (hipSetDevice(s->dev->device) != hipSuccess) return ERR_GPU;
		// the device image uses the caller's row stride, so one contiguous copy brings it back
		const size_t bytes = stride_bytes * (size_t) s->im.height;
		ScopedBlock block;
		if (!block.ensure(s->dev->device, bytes, true)) return ERR_GPU;
		uint32_t e = next_impl(s, block.ptr, stride_bytes, nullptr, true);
		if (!e && hipStreamSynchronize(nullptr) != hipSuccess) e = ERR_GPU;
		if (!e && hipMemcpy(rgba_host, block.ptr, bytes, hipMemcpyDeviceToHost) != hipSuccess) e = ERR_GPU;
		return e;
	});
}

extern "C" void j40hip_sequence_rewind(j40hip_sequence *s) {
	if (!s || !s->dev) return;
	s->dev->cursor = s->dev->decoded = 0;
	for (bool &b : s->dev->slot_saved) b = false;
	for (bool &b : s->dev->lf_filled) b = false;
	for (bool &b : s->dev->ref_filled) b = false;
	for (j40hip_frame *h : s->frames) if (h) for (int k = 0; k < 4; ++k) j40hip_frame_bind_patch_source(h, k, nullptr, 0, 0);
	// (no handle keeps reading a slot that the next playback fills again: a decode of its own is "lfno" until the playback has passed it)
	static const float *const none[3] = {nullptr, nullptr, nullptr};
	for (j40hip_frame *h : s->frames) if (h) j40hip_frame_bind_lf_source(h, none, 0, 0);
}

extern "C" uint32_t j40hip_sequence_read_lf_slot(j40hip_sequence *s, int32_t level, int32_t c, float *out) {
	return guarded([&]() -> uint32_t {
		if (!s || !s->dev || level < 1 || level > 4 || c < 0 || c > 2 || !out || !s->dev->lf_filled[level - 1]) return ERR_RNGE;
		const j40hip_sequence_device *d = s->dev;
		const size_t plane = (size_t) d->lf_w[level - 1] * (size_t) d->lf_h[level - 1];
		if (hipSetDevice(d->device) != hipSuccess || hipDeviceSynchronize() != hipSuccess) return ERR_GPU;
		return hipMemcpy(out, (const float *) d->lf_slot[level - 1].ptr + (size_t) c * plane, sizeof(float) * plane, hipMemcpyDeviceToHost) == hipSuccess ? 0 : ERR_GPU;
	});
}

extern "C" uint32_t j40hip_sequence_ref_slot_size(j40hip_sequence *s, int32_t slot, int32_t *width, int32_t *height) {
	if (!s || !s->dev || slot < 0 || slot > 3 || !width || !height || !s->dev->ref_filled[slot]) return ERR_RNGE;
	*width = s->dev->ref_w[slot]; *height = s->dev->ref_h[slot];
	return 0;
}

extern "C" uint32_t j40hip_sequence_read_ref_slot(j40hip_sequence *s, int32_t slot, int32_t c, float *out) {
	return guarded([&]() -> uint32_t {
		if (!s || !s->dev || slot < 0 || slot > 3 || c < 0 || c > 2 || !out || !s->dev->ref_filled[slot]) return ERR_RNGE;
		const j40hip_sequence_device *d = s->dev;
		const size_t plane = (size_t) d->ref_w[slot] * (size_t) d->ref_h[slot];
		if (hipSetDevice(d->device) != hipSuccess || hipDeviceSynchronize() != hipSuccess) return ERR_GPU;
		return hipMemcpy(out, (const float *) d->ref_xyb[slot].ptr + (size_t) c * plane, sizeof(float) * plane, hipMemcpyDeviceToHost) == hipSuccess ? 0 : ERR_GPU;
	});
}

// known-answer / measuring hook: k_patch_blend on caller-supplied planes, slot planes and placement list (include/j40hip.h). The list is
// checked and binned on the host and copied; the launch is enqueued on `stream` and waited for (the copies live until then)
extern "C" uint32_t j40hip_kat_device_patches(float *planes_dev, int32_t width, int32_t height, const float *const slot_dev[4], const int32_t slot_w[4], const int32_t slot_h[4],
		const int32_t *placements, int32_t count, int32_t *tiles_out, void *stream) {
	return guarded([&]() -> uint32_t {
		if (!planes_dev || width <= 0 || height <= 0 || (int64_t) width * height > (1 << 28) || !slot_dev || !slot_w || !slot_h || count < 0 || (count && !placements)) return ERR_RNGE;
		PatchSlots slots;
		for (int k = 0; k < 4; ++k) { slots.base[k] = slot_dev[k]; slots.w[k] = slot_w[k]; slots.h[k] = slot_h[k]; if (slot_dev[k] && (slot_w[k] <= 0 || slot_h[k] <= 0)) return ERR_RNGE; }
		std::vector<PatchRec> recs((size_t) count);
		for (int32_t i = 0; i < count; ++i) {
			const int32_t *v = placements + (size_t) i * 9;   // x, y, w, h, sx, sy, slot, mode, clamp
			if (v[8] != 0 && v[8] != 1) return ERR4('p', 't', 'c', 'h');
			recs[(size_t) i] = PatchRec{v[0], v[1], v[2], v[3], v[4], v[5], v[6], v[7] | v[8] << 8};
			if (uint32_t e = patch_check(recs[(size_t) i], slots, width, height)) return e;
		}
		PatchBins bins;
		if (!patch_bin(recs.data(), recs.size(), width, height, &bins)) return ERR4('p', 't', 'c', 'h');   // (more tile entries than patch_bin_limit)
		if (tiles_out) *tiles_out = (int32_t) bins.tile_ids.size();
		if (bins.tile_ids.empty()) return 0;
		int device = 0;
		if (hipGetDevice(&device) != hipSuccess) return ERR_GPU;
		hipStream_t st = (hipStream_t) stream;
		j40hip_device_state tmp; tmp.device = device;
		bool ok = true;
		DevPatches p;
		p.recs = tmp.upload(recs.data(), recs.size(), st, ok); p.tile_ids = tmp.upload(bins.tile_ids.data(), bins.tile_ids.size(), st, ok);
		p.offsets = tmp.upload(bins.offsets.data(), bins.offsets.size(), st, ok); p.index = tmp.upload(bins.index.data(), bins.index.size(), st, ok);
		p.num_tiles = (int32_t) bins.tile_ids.size(); p.tiles_x = bins.tiles_x;
		if (ok) { launch_patch_blend(planes_dev, width, height, p, slots, st); ok = hipGetLastError() == hipSuccess; }
		if (hipStreamSynchronize(st) != hipSuccess) ok = false;
		for (auto &b : tmp.buffers) b.release();
		tmp.buffers.clear();
		return ok ? 0 : ERR_GPU;
	});
}

extern "C" uint32_t j40hip_sequence_status(j40hip_sequence *s, int64_t *out_frame) {
	return guarded([&]() -> uint32_t {
		if (out_frame) *out_frame = -1;
		if (!s || !s->dev) return 0;
		for (int64_t k = 0; k < s->dev->decoded; ++k) if (j40hip_frame *h = s->frames[(size_t) k]) if (uint32_t e = j40hip_frame_status(h)) { if (out_frame) *out_frame = k; return e; }
		return 0;
	});
}

namespace {
// what both hooks refuse before anything is launched
uint32_t kat_compose_check(const void *out_dev, size_t out_stride, const void *src_dev, size_t src_stride, const void *frame_dev, size_t frame_stride,
		int32_t W, int32_t H, int32_t w, int32_t h, int32_t format) {
	if (format != J40HIP_U8X4 && format != J40HIP_U16X4) return ERR4('U', 'f', 'm', '?');
	const size_t pb = format == J40HIP_U16X4 ? 8 : 4;
	if (!out_dev || !frame_dev || W <= 0 || H <= 0 || w <= 0 || h <= 0) return ERR_RNGE;
	if (out_stride < (size_t) W * pb || frame_stride < (size_t) w * pb || (src_dev && src_stride < (size_t) W * pb)) return ERR_RNGE;
	if (((uintptr_t) out_dev | (uintptr_t) frame_dev | (uintptr_t) src_dev | out_stride | frame_stride | (src_dev ? src_stride : 0)) % pb) return ERR_RNGE;
	if (src_dev == out_dev && src_stride != out_stride) return ERR_RNGE;
	return 0;
}
}

extern "C" uint32_t j40hip_kat_device_blend(void *out_dev, size_t out_stride, const void *src_dev, size_t src_stride, const void *frame_dev, size_t frame_stride,
		int32_t W, int32_t H, int32_t x0, int32_t y0, int32_t w, int32_t h, uint32_t empty_lo, uint32_t empty_hi, int32_t format, int32_t colour_mode, int32_t alpha_mode, void *stream) {
	if (uint32_t e = kat_compose_check(out_dev, out_stride, src_dev, src_stride, frame_dev, frame_stride, W, H, w, h, format)) return e;
	if (colour_mode < 0 || colour_mode > 4 || alpha_mode < 0 || alpha_mode > 4) return ERR_RNGE;
	launch_frame_blend((uint8_t *) out_dev, out_stride, (const uint8_t *) src_dev, src_stride, (const uint8_t *) frame_dev, frame_stride, W, H, x0, y0, w, h, empty_lo, empty_hi,
		format == J40HIP_U16X4 ? 8 : 4, colour_mode, alpha_mode, (hipStream_t) stream);
	return hipGetLastError() == hipSuccess ? 0 : ERR_GPU;
}

extern "C" uint32_t j40hip_kat_device_compose(void *out_dev, size_t out_stride, const void *src_dev, size_t src_stride, const void *frame_dev, size_t frame_stride,
		int32_t W, int32_t H, int32_t x0, int32_t y0, int32_t w, int32_t h, uint32_t empty_lo, uint32_t empty_hi, int32_t format, void *stream) {
	if (uint32_t e = kat_compose_check(out_dev, out_stride, src_dev, src_stride, frame_dev, frame_stride, W, H, w, h, format)) return e;
	const size_t pb = format == J40HIP_U16X4 ? 8 : 4;
	launch_frame_compose((uint8_t *) out_dev, out_stride, (const uint8_t *) src_dev, src_stride, (const uint8_t *) frame_dev, frame_stride, W, H, x0, y0, w, h, empty_lo, empty_hi, (int32_t) pb, (hipStream_t) stream);
	return hipGetLastError() == hipSuccess ? 0 : ERR_GPU;
}
