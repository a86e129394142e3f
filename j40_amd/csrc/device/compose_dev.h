// j40_amd/csrc/device/compose_dev.h -- putting a frame of a sequence onto the canvas (j40hip_sequence_next; blend mode Replace): the
// clipping of the frame's rectangle and the composition of one canvas row. Compiled for the device by compose_kernels.hip and for the
// CPU by tests/hostsim/compose_sim.cpp: the same functions.
//
// A canvas pixel inside the frame's rectangle (x0, y0, w, h), clipped to the canvas, is the frame's pixel; every other one is the
// source's pixel -- the reference slot the frame names -- or, without a source, the empty pixel. Each canvas pixel is written once.
// When the output IS the source (out == src: an animation that keeps drawing into one slot) only the rectangle is touched, the
// rest of the canvas already holds what it has to hold.
//
// A row is up to three spans: source / frame / source. Each span moves like region_crop_row's row: where its two rows sit alike
// within 16 bytes, a head of pixels up to the destination's first 16-byte boundary, whole 16-byte pieces (a lane takes every
// lanes-th piece: neighbouring lanes, neighbouring 16 bytes) and a tail; pixel by pixel otherwise. The empty pixel is stored the
// same way.
#pragma once
#include "region_dev.h"

namespace j40hip {

// the frame's rectangle clipped to the W x H canvas: canvas columns [cx0, cx1) of rows [cy0, cy1) (cx1 <= cx0: nothing of the frame
// is on the canvas), and the frame's pixel (fx, fy) that lands on canvas pixel (cx0, cy0)
struct ComposeRect { int32_t cx0, cy0, cx1, cy1, fx, fy; };

J40_HD ComposeRect compose_clip(int32_t W, int32_t H, int32_t x0, int32_t y0, int32_t w, int32_t h) {
	ComposeRect r;
	const int64_t x1 = (int64_t) x0 + w, y1 = (int64_t) y0 + h;
	r.cx0 = x0 > 0 ? x0 : 0; r.cy0 = y0 > 0 ? y0 : 0;
	r.cx1 = (int32_t) (x1 < W ? x1 : W); r.cy1 = (int32_t) (y1 < H ? y1 : H);
	if (r.cx1 <= r.cx0 || r.cy1 <= r.cy0) { r.cx0 = r.cy0 = r.cx1 = r.cy1 = 0; }
	r.fx = r.cx0 - x0; r.fy = r.cy0 - y0;
	if (r.cx1 == r.cx0) r.fx = r.fy = 0;
	return r;
}

#if defined(__HIP_DEVICE_COMPILE__)
J40_HD void compose_fill16(uint8_t *d, uint32_t a, uint32_t b, uint32_t c, uint32_t e) { region_u32x4 v = {a, b, c, e}; __builtin_nontemporal_store(v, (region_u32x4 *) d); }
template <int PB> J40_HD void compose_fill_pixel(uint8_t *d, uint32_t lo, uint32_t hi) {
	if (PB == 8) __builtin_nontemporal_store((uint64_t) lo | (uint64_t) hi << 32, (uint64_t *) d);
	else __builtin_nontemporal_store(lo, (uint32_t *) d);
}
#else
J40_HD void compose_fill16(uint8_t *d, uint32_t a, uint32_t b, uint32_t c, uint32_t e) { const uint32_t v[4] = {a, b, c, e}; memcpy(d, v, 16); }
template <int PB> J40_HD void compose_fill_pixel(uint8_t *d, uint32_t lo, uint32_t hi) {
	const uint32_t v[2] = {lo, hi};
	memcpy(d, v, PB);
}
#endif

// `w` pixels of PB bytes at dst (pixel-aligned) become the empty pixel, by lane `lane` of `lanes`. lo, hi: the pixel's first and
// second four bytes as little-endian words (u8x4: lo alone)
template <int PB> J40_HD void compose_fill_row(uint8_t *dst, int32_t w, uint32_t lo, uint32_t hi, int32_t lane, int32_t lanes) {
	const uintptr_t da = (uintptr_t) dst & 15u;
	int32_t head = (int32_t) (((16u - da) & 15u) / PB);
	if (head > w) head = w;
	const int32_t pieces = (w - head) / (16 / PB), wide = pieces * (16 / PB), narrow = w - wide;
	for (int32_t k = lane; k < pieces; k += lanes) {
		uint8_t *d = dst + (size_t) head * PB + (size_t) k * 16;
		if (PB == 8) compose_fill16(d, lo, hi, lo, hi); else compose_fill16(d, lo, lo, lo, lo);
	}
	for (int32_t k = lane; k < narrow; k += lanes) {
		const size_t x = (size_t) (k < head ? k : k + wide);
		compose_fill_pixel<PB>(dst + x * PB, lo, hi);
	}
}

// `w` pixels from src (or, src null, the empty pixel) to dst
template <int PB> J40_HD void compose_span(const uint8_t *src, uint8_t *dst, int32_t w, uint32_t lo, uint32_t hi, int32_t lane, int32_t lanes) {
	if (w <= 0) return;
	if (src) region_crop_row<PB>(src, dst, w, lane, lanes);
	else compose_fill_row<PB>(dst, w, lo, hi, lane, lanes);
}

// Canvas row y by lane `lane` of `lanes`. out_row, src_row: the row's first pixel in the output and in the source (null: no source);
// frm: the frame's image, frm_stride bytes a row. only_rect: the output is the source -- rows and columns outside the rectangle
// are left alone.
template <int PB> J40_HD void compose_row(uint8_t *out_row, const uint8_t *src_row, const uint8_t *frm, size_t frm_stride, int32_t W, int32_t y, const ComposeRect &r,
		uint32_t lo, uint32_t hi, bool only_rect, int32_t lane, int32_t lanes) {
	const bool inside = y >= r.cy0 && y < r.cy1;
	if (!inside) {
		if (!only_rect) compose_span<PB>(src_row, out_row, W, lo, hi, lane, lanes);
		return;
	}
	const uint8_t *frm_row = frm + (size_t) (r.fy + (y - r.cy0)) * frm_stride + (size_t) r.fx * PB;
	region_crop_row<PB>(frm_row, out_row + (size_t) r.cx0 * PB, r.cx1 - r.cx0, lane, lanes);
	if (only_rect) return;
	compose_span<PB>(src_row, out_row, r.cx0, lo, hi, lane, lanes);
	compose_span<PB>(src_row ? src_row + (size_t) r.cx1 * PB : nullptr, out_row + (size_t) r.cx1 * PB, W - r.cx1, lo, hi, lane, lanes);
}

} // namespace j40hip
