// j40_amd/csrc/device/alpha_dev.h -- the kept alpha channel of a VarDCT frame (j40hip_frame_set_alpha): what turns a sample of the
// alpha extra channel into the A of an output pixel, and the merge of a run of such samples into pixels that are already written.
// Compiled for the device by alpha_kernels.hip and for the CPU by tests/hostsim/alpha_sim.cpp: the same functions.
//
// The rule is the reference's render of a Modular frame's alpha (j40.h:7950-7951) and, for 16-bit output, the J40_U16X4 rule of
// include/j40hip.h: p clamped to [0, maxpixel = 2^bpp - 1], then (p * M + 2^(bpp - 1)) / maxpixel with M = 255 or 65535, bpp 8..15.
// The numerator stays below 2^31 (32767 * 65535 + 16384), so the division is one multiply-high by floor(2^32 / maxpixel) and one
// correction: n / d - n * floor(2^32 / d) / 2^32 < n / 2^32 < 1, the estimate is the quotient or one below it.
#pragma once
#include <stdint.h>
#include <string.h>
#ifndef J40_HD
#ifdef __HIPCC__
#define J40_HD __host__ __device__ __forceinline__
#else
#define J40_HD static inline
#endif
#endif
#ifndef J40_GLOBAL
#ifdef __HIPCC__
#define J40_GLOBAL __attribute__((address_space(1)))
#else
#define J40_GLOBAL
#endif
#endif

namespace j40hip {

// per frame: the alpha channel's depth as the kernel needs it
struct AlphaScale { uint32_t maxpixel, half, recip, identity; };

J40_HD AlphaScale alpha_scale_make(int32_t bpp, bool out16) {
	AlphaScale s;
	s.maxpixel = (1u << bpp) - 1u; s.half = 1u << (bpp - 1);
	s.recip = (uint32_t) (((uint64_t) 1 << 32) / s.maxpixel);
	s.identity = bpp == 8 && !out16;   // (p * 255 + 128) / 255 = p
	return s;
}

template <bool OUT16> J40_HD uint32_t alpha_value(int32_t p, const AlphaScale &s) {
	const uint32_t c = p < 0 ? 0u : (uint32_t) p > s.maxpixel ? s.maxpixel : (uint32_t) p;
	if (!OUT16 && s.identity) return c;
	const uint32_t n = c * (OUT16 ? 65535u : 255u) + s.half;
	uint32_t q = (uint32_t) (((uint64_t) n * s.recip) >> 32);
	if (n - q * s.maxpixel >= s.maxpixel) ++q;
	return q;
}

// four neighbouring pixels at once. u8: `px` is four RGBA words, A the top byte of each; u16: eight words, A the top half of every second
template <bool OUT16> J40_HD void alpha_insert4(uint32_t *px, const int16_t a[4], const AlphaScale &s) {
	for (int i = 0; i < 4; ++i) {
		const uint32_t v = alpha_value<OUT16>(a[i], s);
		if (OUT16) px[2 * i + 1] = (px[2 * i + 1] & 0x0000ffffu) | v << 16;
		else px[i] = (px[i] & 0x00ffffffu) | v << 24;
	}
}

// one pixel, the narrow path of row heads and tails: only the A sample is written
template <bool OUT16> J40_HD void alpha_store1(J40_GLOBAL uint8_t *pixel, int32_t a, const AlphaScale &s) {
	const uint32_t v = alpha_value<OUT16>(a, s);
	if (OUT16) *(J40_GLOBAL uint16_t *) (pixel + 6) = (uint16_t) v;
	else pixel[3] = (uint8_t) v;
}

// How a row of `w` pixels starting at `row` splits: `head` pixels up to the first 16-byte boundary (rows are only pixel-aligned:
// 4 bytes for u8, 8 for u16), then whole chunks of four pixels, 16-byte aligned, then the rest.
template <bool OUT16> J40_HD int32_t alpha_row_head(uintptr_t row, int32_t w) {
	const int32_t head = (int32_t) ((16u - (uint32_t) (row & 15u)) & 15u) / (OUT16 ? 8 : 4);
	return head < w ? head : w;
}

// chunk `k` of a row (k < (w - head) / 4): the wide path. `alpha` points at the row's first sample
template <bool OUT16> J40_HD void alpha_merge_chunk(J40_GLOBAL uint8_t *row, const J40_GLOBAL int16_t *alpha, int32_t head, int32_t k, const AlphaScale &s) {
	const int32_t x = head + 4 * k;
	int16_t a[4];
#ifdef __HIP_DEVICE_COMPILE__
	{   // one 8-byte load; the samples are 2-byte aligned only (tightly packed rows of any width), which global memory takes
		typedef uint32_t u32x2 __attribute__((ext_vector_type(2), aligned(2)));
		const u32x2 v = *(const J40_GLOBAL u32x2 *) (alpha + x);
		a[0] = (int16_t) (v.x & 0xffffu); a[1] = (int16_t) (v.x >> 16); a[2] = (int16_t) (v.y & 0xffffu); a[3] = (int16_t) (v.y >> 16);
	}
	typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
	J40_GLOBAL u32x4 *q = (J40_GLOBAL u32x4 *) (row + (size_t) x * (OUT16 ? 8 : 4));
	if (OUT16) {
		u32x4 lo = q[0], hi = q[1];
		uint32_t px[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
		alpha_insert4<true>(px, a, s);
		lo.y = px[1]; lo.w = px[3]; hi.y = px[5]; hi.w = px[7];
		q[0] = lo; q[1] = hi;
	} else {
		u32x4 v = q[0];
		uint32_t px[4] = {v.x, v.y, v.z, v.w};
		alpha_insert4<false>(px, a, s);
		v.x = px[0]; v.y = px[1]; v.z = px[2]; v.w = px[3];
		q[0] = v;
	}
#else
	uint32_t px[8];
	memcpy(a, (const int16_t *) alpha + x, sizeof a);
	uint8_t *q = (uint8_t *) row + (size_t) x * (OUT16 ? 8 : 4);
	memcpy(px, q, OUT16 ? 32 : 16);
	alpha_insert4<OUT16>(px, a, s);
	memcpy(q, px, OUT16 ? 32 : 16);
#endif
}

// the row's head and tail pixels, one by one
template <bool OUT16> J40_HD void alpha_merge_edges(J40_GLOBAL uint8_t *row, const J40_GLOBAL int16_t *alpha, int32_t head, int32_t w, const AlphaScale &s) {
	const int32_t body_end = head + ((w - head) & ~3);
	for (int32_t x = 0; x < head; ++x) alpha_store1<OUT16>(row + (size_t) x * (OUT16 ? 8 : 4), alpha[x], s);
	for (int32_t x = body_end; x < w; ++x) alpha_store1<OUT16>(row + (size_t) x * (OUT16 ? 8 : 4), alpha[x], s);
}

// a whole row on one thread (the CPU build; the kernel deals chunks and edges out to lanes)
template <bool OUT16> J40_HD void alpha_merge_row(J40_GLOBAL uint8_t *row, const J40_GLOBAL int16_t *alpha, int32_t w, const AlphaScale &s) {
	const int32_t head = alpha_row_head<OUT16>((uintptr_t) row, w);
	for (int32_t k = 0; k < (w - head) / 4; ++k) alpha_merge_chunk<OUT16>(row, alpha, head, k, s);
	alpha_merge_edges<OUT16>(row, alpha, head, w, s);
}

} // namespace j40hip
