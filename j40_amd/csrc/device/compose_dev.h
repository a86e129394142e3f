// j40_amd/csrc/device/compose_dev.h -- putting a frame of a sequence onto the canvas (j40hip_sequence_next): the clipping of the
// frame's rectangle and the composition of one canvas row, for blend mode Replace (compose_row) and for the other four (blend_row,
// below). Compiled for the device by compose_kernels.hip and for the CPU by tests/hostsim/compose_sim.cpp and blend_sim.cpp: the same
// functions.
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

// ---- blend modes other than Replace (J40HIP_SEQ_BLEND): blend_row is compose_row with the frame's span blended over the source's ----
// The arithmetic works on rendered pixels, RGBA of PB bytes, M = 255 or 65535 (INTEGRATION.md "Several frames" states it; the tests
// restate it in numpy): every step below is one float32 operation in the order written, every division a division. n: the frame's
// pixel, o: the source's (or the empty pixel). The colour channels' mode and the alpha's are independent; the colour formulas use
// the incoming alphas.
enum { BLEND_REPLACE = 0, BLEND_ADD = 1, BLEND_BLEND = 2, BLEND_MULADD = 3, BLEND_MUL = 4 };

J40_HD uint32_t blend_quantise(float v, float M) {
	const float q = v * M + 0.5f;
	return q <= 0.0f ? 0u : q >= M ? (uint32_t) M : (uint32_t) q;   // (q > 0: the conversion truncates, which is floor)
}

// one pixel as one (u8x4) or two (u16x4) little-endian words. CM: the colour channels' mode, chosen outside the per-pixel work;
// amode: the alpha's
template <int PB, int CM> J40_HD void blend_pixel(uint32_t nlo, uint32_t nhi, uint32_t olo, uint32_t ohi, int32_t amode, uint32_t *rlo, uint32_t *rhi) {
	const float M = PB == 8 ? 65535.0f : 255.0f;
	uint32_t n[4], o[4], r[4];
	if (PB == 8) {
		n[0] = nlo & 0xffffu; n[1] = nlo >> 16; n[2] = nhi & 0xffffu; n[3] = nhi >> 16;
		o[0] = olo & 0xffffu; o[1] = olo >> 16; o[2] = ohi & 0xffffu; o[3] = ohi >> 16;
	} else for (int c = 0; c < 4; ++c) { n[c] = nlo >> (8 * c) & 0xffu; o[c] = olo >> (8 * c) & 0xffu; }
	const float fa = (float) n[3] / M, ba = (float) o[3] / M;
	switch (amode) {
	case BLEND_ADD: r[3] = blend_quantise(ba + fa, M); break;
	case BLEND_BLEND: r[3] = blend_quantise(fa + (ba * (1.0f - fa)), M); break;
	case BLEND_MULADD: r[3] = blend_quantise(ba, M); break;
	case BLEND_MUL: r[3] = blend_quantise(ba * fa, M); break;
	default: r[3] = n[3];
	}
	if (CM == BLEND_REPLACE) { r[0] = n[0]; r[1] = n[1]; r[2] = n[2]; }
	else {
		const float t = 1.0f - fa, w = ba * t, A = fa + w;   // (Blend alone reads them)
		for (int c = 0; c < 3; ++c) {
			const float f = (float) n[c] / M, b = (float) o[c] / M;
			float v;
			if (CM == BLEND_ADD) v = b + f;
			else if (CM == BLEND_BLEND) { const float num = (f * fa) + (b * w); v = A > 0.0f ? num / A : 0.0f; }
			else if (CM == BLEND_MULADD) v = b + (f * fa);
			else v = b * f;
			r[c] = blend_quantise(v, M);
		}
	}
	if (PB == 8) { *rlo = r[0] | r[1] << 16; *rhi = r[2] | r[3] << 16; }
	else { *rlo = r[0] | r[1] << 8 | r[2] << 16 | r[3] << 24; *rhi = 0; }
}

struct BlendPiece { uint32_t v[4]; };   // 16 bytes: four u8x4 pixels or two u16x4 pixels
#if defined(__HIP_DEVICE_COMPILE__)
J40_HD BlendPiece blend_load16(const uint8_t *s) { const region_u32x4 q = *(const region_u32x4 *) s; return BlendPiece{{q.x, q.y, q.z, q.w}}; }
J40_HD void blend_load_pixel(const uint8_t *s, int pb, uint32_t *lo, uint32_t *hi) {
	if (pb == 8) { const uint64_t q = *(const uint64_t *) s; *lo = (uint32_t) q; *hi = (uint32_t) (q >> 32); }
	else { *lo = *(const uint32_t *) s; *hi = 0; }
}
#else
J40_HD BlendPiece blend_load16(const uint8_t *s) { BlendPiece p; memcpy(p.v, s, 16); return p; }
J40_HD void blend_load_pixel(const uint8_t *s, int pb, uint32_t *lo, uint32_t *hi) { uint32_t v[2] = {0, 0}; memcpy(v, s, (size_t) pb); *lo = v[0]; *hi = v[1]; }
#endif

// `w` pixels: frm blended over src (src null: over the empty pixel lo, hi) into dst, by lane `lane` of `lanes`. Where the rows of all
// three sit alike within 16 bytes a lane takes whole 16-byte pieces, as region_crop_row does; pixel by pixel at the span's edges and
// otherwise. dst may be src: a lane reads the piece (or pixel) it writes before it writes it, and nobody else touches it.
template <int PB, int CM> J40_HD void blend_span_mode(const uint8_t *src, const uint8_t *frm, uint8_t *dst, int32_t w, uint32_t lo, uint32_t hi, int32_t amode, int32_t lane, int32_t lanes) {
	const uintptr_t da = (uintptr_t) dst & 15u;
	int32_t head = w, pieces = 0;
	if (((uintptr_t) frm & 15u) == da && (!src || ((uintptr_t) src & 15u) == da)) {
		head = (int32_t) (((16u - da) & 15u) / PB);
		if (head > w) head = w;
		pieces = (w - head) / (16 / PB);
	}
	const int32_t wide = pieces * (16 / PB), narrow = w - wide;
	for (int32_t k = lane; k < pieces; k += lanes) {
		const size_t at = (size_t) head * PB + (size_t) k * 16;
		const BlendPiece n = blend_load16(frm + at);
		const BlendPiece o = src ? blend_load16(src + at) : (PB == 8 ? BlendPiece{{lo, hi, lo, hi}} : BlendPiece{{lo, lo, lo, lo}});
		uint32_t r[4], unused;
		if (PB == 8) { blend_pixel<8, CM>(n.v[0], n.v[1], o.v[0], o.v[1], amode, r + 0, r + 1); blend_pixel<8, CM>(n.v[2], n.v[3], o.v[2], o.v[3], amode, r + 2, r + 3); }
		else for (int i = 0; i < 4; ++i) blend_pixel<4, CM>(n.v[i], 0, o.v[i], 0, amode, r + i, &unused);
		compose_fill16(dst + at, r[0], r[1], r[2], r[3]);
	}
	for (int32_t k = lane; k < narrow; k += lanes) {
		const size_t at = (size_t) (k < head ? k : k + wide) * PB;
		uint32_t nlo, nhi, olo = lo, ohi = hi, rlo, rhi;
		blend_load_pixel(frm + at, PB, &nlo, &nhi);
		if (src) blend_load_pixel(src + at, PB, &olo, &ohi);
		blend_pixel<PB, CM>(nlo, nhi, olo, ohi, amode, &rlo, &rhi);
		compose_fill_pixel<PB>(dst + at, rlo, rhi);
	}
}

// (cmode is the same for every lane: one branch a span, outside the per-pixel work)
template <int PB> J40_HD void blend_span(const uint8_t *src, const uint8_t *frm, uint8_t *dst, int32_t w, uint32_t lo, uint32_t hi, int32_t cmode, int32_t amode, int32_t lane, int32_t lanes) {
	switch (cmode) {
	case BLEND_ADD: blend_span_mode<PB, BLEND_ADD>(src, frm, dst, w, lo, hi, amode, lane, lanes); break;
	case BLEND_BLEND: blend_span_mode<PB, BLEND_BLEND>(src, frm, dst, w, lo, hi, amode, lane, lanes); break;
	case BLEND_MULADD: blend_span_mode<PB, BLEND_MULADD>(src, frm, dst, w, lo, hi, amode, lane, lanes); break;
	case BLEND_MUL: blend_span_mode<PB, BLEND_MUL>(src, frm, dst, w, lo, hi, amode, lane, lanes); break;
	default: blend_span_mode<PB, BLEND_REPLACE>(src, frm, dst, w, lo, hi, amode, lane, lanes);
	}
}

// compose_row with the modes: canvas row y is up to three spans, source / blended / source
template <int PB> J40_HD void blend_row(uint8_t *out_row, const uint8_t *src_row, const uint8_t *frm, size_t frm_stride, int32_t W, int32_t y, const ComposeRect &r,
		uint32_t lo, uint32_t hi, bool only_rect, int32_t cmode, int32_t amode, int32_t lane, int32_t lanes) {
	const bool inside = y >= r.cy0 && y < r.cy1;
	if (!inside) {
		if (!only_rect) compose_span<PB>(src_row, out_row, W, lo, hi, lane, lanes);
		return;
	}
	const uint8_t *frm_row = frm + (size_t) (r.fy + (y - r.cy0)) * frm_stride + (size_t) r.fx * PB;
	blend_span<PB>(src_row ? src_row + (size_t) r.cx0 * PB : nullptr, frm_row, out_row + (size_t) r.cx0 * PB, r.cx1 - r.cx0, lo, hi, cmode, amode, lane, lanes);
	if (only_rect) return;
	compose_span<PB>(src_row, out_row, r.cx0, lo, hi, lane, lanes);
	compose_span<PB>(src_row ? src_row + (size_t) r.cx1 * PB : nullptr, out_row + (size_t) r.cx1 * PB, W - r.cx1, lo, hi, lane, lanes);
}

} // namespace j40hip
