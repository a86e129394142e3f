// j40_amd/csrc/device/scale_dev.h -- reduced-size decode (j40hip_frame_set_scale): the arithmetic of the 1:2 and 1:4 output, written
// once. Compiled for the device by the pixel kernels (kernels.hip, modular_kernels.hip) and k_downscale (scale_kernels.hip), and for
// the CPU by tests/hostsim/scale_sim.cpp: the same functions.
//
// Scale shift k in {0, 1, 2}, s = 1 << k. A frame of W x H gives ow = (W + s - 1) >> k by oh = (H + s - 1) >> k pixels. Sample c of output
// pixel (i, j) is (S + (n >> 1)) / n in integers: S the sum of sample c of the FULL decode in the same output format over the cell
// x in [i * s, min(W, (i + 1) * s)), y in [j * s, min(H, (j + 1) * s)), n the cell's pixels (1, 2, 3, 4, 6, 8, 9, 12 or 16; only cells on
// the right and bottom edges have n != s * s). The mean is taken on coded levels, the bytes the full decode writes -- not in linear
// light: the small image is then an exact function of pixels the reference pins.
//
// u8x4: two 32-bit accumulators with 16-bit fields take a pixel in two adds (16 * 255 fits a field). u16x4: the same with two 64-bit
// accumulators and 32-bit fields. Interior cells divide by a shift, the fields side by side; edge cells divide field by field
// (S < 2^20).
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
#ifdef __HIPCC__
#define J40_HD_MEMBER __host__ __device__ __forceinline__
#else
#define J40_HD_MEMBER inline
#endif

namespace j40hip {

enum { SCALE_MAX_SHIFT = 2 };

J40_HD int32_t scale_out_size(int32_t full, int32_t k) { return (full + (1 << k) - 1) >> k; }
// samples of output position o along a dimension of `lim` samples: s, fewer in the last cell (0 or less: the cell lies outside)
J40_HD int32_t scale_span(int32_t o, int32_t lim, int32_t k) { const int32_t s = 1 << k, left = lim - (o << k); return left < s ? left : s; }
// (S + (n >> 1)) / n; n == s * s by a shift
J40_HD uint32_t scale_div(uint32_t S, int32_t n, int32_t k) { return n == 1 << (2 * k) ? (S + ((uint32_t) n >> 1)) >> (2 * k) : (S + ((uint32_t) n >> 1)) / (uint32_t) n; }

template <int PB> struct ScaleAcc;
// u8x4: lo = samples 0 and 2 (R, B), hi = samples 1 and 3 (G, A) in 16-bit fields
template <> struct ScaleAcc<4> {
	typedef uint32_t pixel;
	uint32_t lo, hi;
	J40_HD_MEMBER void clear() { lo = hi = 0; }
	J40_HD_MEMBER void add(uint32_t v) { lo += v & 0x00ff00ffu; hi += (v >> 8) & 0x00ff00ffu; }
	J40_HD_MEMBER uint32_t mean(int32_t n, int32_t k) const {
		if (n == 1 << (2 * k)) {   // interior: both fields of an accumulator at once (a mean is at most 255: what the upper field shifts in is masked off)
			const uint32_t half = ((uint32_t) n >> 1) * 0x00010001u;
			return (((lo + half) >> (2 * k)) & 0x00ff00ffu) | ((((hi + half) >> (2 * k)) & 0x00ff00ffu) << 8);
		}
		return scale_div(lo & 0xffffu, n, k) | (scale_div(lo >> 16, n, k) << 16) | (scale_div(hi & 0xffffu, n, k) << 8) | (scale_div(hi >> 16, n, k) << 24);
	}
};
// u16x4: lo = samples 0 and 2, hi = samples 1 and 3 in 32-bit fields
template <> struct ScaleAcc<8> {
	typedef uint64_t pixel;
	uint64_t lo, hi;
	J40_HD_MEMBER void clear() { lo = hi = 0; }
	J40_HD_MEMBER void add(uint64_t v) { lo += v & 0x0000ffff0000ffffull; hi += (v >> 16) & 0x0000ffff0000ffffull; }
	J40_HD_MEMBER uint64_t mean(int32_t n, int32_t k) const {
		if (n == 1 << (2 * k)) {
			const uint64_t half = (uint64_t) ((uint32_t) n >> 1) * 0x0000000100000001ull;
			return (((lo + half) >> (2 * k)) & 0x0000ffff0000ffffull) | ((((hi + half) >> (2 * k)) & 0x0000ffff0000ffffull) << 16);
		}
		return (uint64_t) scale_div((uint32_t) lo, n, k) | ((uint64_t) scale_div((uint32_t) (lo >> 32), n, k) << 32)
			| ((uint64_t) scale_div((uint32_t) hi, n, k) << 16) | ((uint64_t) scale_div((uint32_t) (hi >> 32), n, k) << 48);
	}
};

// ---- a full-size image made small (k_downscale): `cw` pixels of PB bytes at p into the accumulator. Rows are pixel-aligned; where a
// cell's row of pixels is 8 or 16 bytes and sits on such a boundary the device takes it in one load ----
#if defined(__HIP_DEVICE_COMPILE__)
typedef uint32_t scale_u32x2 __attribute__((ext_vector_type(2)));
typedef uint32_t scale_u32x4 __attribute__((ext_vector_type(4)));
template <int PB> J40_HD void scale_add_span(ScaleAcc<PB> &acc, const uint8_t *p, int32_t cw);
template <> J40_HD void scale_add_span<4>(ScaleAcc<4> &acc, const uint8_t *p, int32_t cw) {
	if (cw == 4 && ((uintptr_t) p & 15u) == 0) { const scale_u32x4 v = *(const scale_u32x4 *) p; acc.add(v.x); acc.add(v.y); acc.add(v.z); acc.add(v.w); return; }
	if (cw == 2 && ((uintptr_t) p & 7u) == 0) { const scale_u32x2 v = *(const scale_u32x2 *) p; acc.add(v.x); acc.add(v.y); return; }
	for (int32_t x = 0; x < cw; ++x) acc.add(*(const uint32_t *) (p + 4 * x));
}
template <> J40_HD void scale_add_span<8>(ScaleAcc<8> &acc, const uint8_t *p, int32_t cw) {
	if ((cw & 1) == 0 && ((uintptr_t) p & 15u) == 0) {
		for (int32_t x = 0; x < cw; x += 2) { const scale_u32x4 v = *(const scale_u32x4 *) (p + 8 * x); acc.add((uint64_t) v.x | ((uint64_t) v.y << 32)); acc.add((uint64_t) v.z | ((uint64_t) v.w << 32)); }
		return;
	}
	for (int32_t x = 0; x < cw; ++x) acc.add(*(const uint64_t *) (p + 8 * x));
}
template <int PB> J40_HD void scale_store_pixel(uint8_t *d, typename ScaleAcc<PB>::pixel v) { __builtin_nontemporal_store(v, (typename ScaleAcc<PB>::pixel *) d); }
#else
template <int PB> J40_HD void scale_add_span(ScaleAcc<PB> &acc, const uint8_t *p, int32_t cw) {
	for (int32_t x = 0; x < cw; ++x) { typename ScaleAcc<PB>::pixel v; memcpy(&v, p + (size_t) PB * (size_t) x, PB); acc.add(v); }
}
template <int PB> J40_HD void scale_store_pixel(uint8_t *d, typename ScaleAcc<PB>::pixel v) { memcpy(d, &v, PB); }
#endif

// output row j of the small image by lane `lane` of `lanes`: src the full W x H image, dst_row the row's first pixel
template <int PB> J40_HD void scale_row(const uint8_t *src, size_t src_stride, uint8_t *dst_row, int32_t W, int32_t H, int32_t k, int32_t j, int32_t lane, int32_t lanes) {
	const int32_t ow = scale_out_size(W, k), ch = scale_span(j, H, k);
	if (ch <= 0) return;
	const uint8_t *rows = src + (size_t) (j << k) * src_stride;
	for (int32_t i = lane; i < ow; i += lanes) {
		const int32_t cw = scale_span(i, W, k);
		ScaleAcc<PB> acc;
		acc.clear();
		for (int32_t y = 0; y < ch; ++y) scale_add_span<PB>(acc, rows + (size_t) y * src_stride + (size_t) (i << k) * PB, cw);
		scale_store_pixel<PB>(dst_row + (size_t) i * PB, acc.mean(cw * ch, k));
	}
}

} // namespace j40hip
