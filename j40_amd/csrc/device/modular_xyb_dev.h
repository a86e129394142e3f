// j40_amd/csrc/device/modular_xyb_dev.h -- a Modular frame of an XYB image rendered through the XYB colour tail (j40hip_frame_set_modular_xyb;
// DESIGN.md section 4 "Modular frames of XYB images", PARITY UNPINNED): the per-sample rule and the work of one lane of
// k_modular_xyb_pack / k_modular_to_xyb. Compiles for the device and for the host (tests/hostsim/modular_xyb_sim.cpp).
//
// The rule. c0, c1, c2: the three colour planes after every inverse transform (quantised Y, X, B - Y); m = the frame's m_lf_scaled:
//   Y = (float) c0 * m[1]      X = (float) c1 * m[0]      B = (float) (c2 + c0) * m[2]
// The sum is an integer sum (int32 for int16 planes, int64 for int32 planes), then ONE conversion to float32 (round to nearest even) and
// ONE float32 multiply; there is no float add, so nothing can fuse. From X, Y, B on the pixel is xyb_to_rgba8 / xyb_to_rgba16's
// (idct_dev.h), A the alpha plane's level rendered as pack_rgba8 / pack_rgba16 render it (modular_dev.h), or full scale.
#pragma once
#include <cstdint>
#include <cstring>
#include "entropy_dev.h"
#include "idct_dev.h"
#include "modular_dev.h"

namespace j40hip {

// what the kernels take by value: the dequantisation factors and the colour tail's constants
struct ModXybConsts {
	float m[3];
	ColourConsts cc;
};

J40_DEV float modxyb_sum_to_float(int16_t a, int16_t b) { return (float) ((int32_t) a + (int32_t) b); }
J40_DEV float modxyb_sum_to_float(int32_t a, int32_t b) { return (float) ((int64_t) a + (int64_t) b); }

// xyb[0..2] = X, Y, B
template <typename S> J40_DEV void modular_sample_to_xyb(S c0, S c1, S c2, const float m[3], float xyb[3]) {
	xyb[0] = (float) c1 * m[0];
	xyb[1] = (float) c0 * m[1];
	xyb[2] = modxyb_sum_to_float(c2, c0) * m[2];
}

// the alpha sample at level `a` of a bpp-bit image: pack_rgba8's own (modular_dev.h), as scale_to_u16 is pack_rgba16's
J40_DEV uint32_t modxyb_alpha8(int32_t a, int32_t bpp) { return pack_rgba8(0, 0, 0, a, bpp) >> 24; }

template <typename S> J40_DEV uint32_t modular_xyb_rgba8(S c0, S c1, S c2, int32_t a, const ModXybConsts &k, const J40_LDS float *thr) {
	float v[3];
	modular_sample_to_xyb(c0, c1, c2, k.m, v);
	return (xyb_to_rgba8(v[0], v[1], v[2], k.cc, thr) & 0x00ffffffu) | modxyb_alpha8(a, k.cc.bpp) << 24;
}
template <typename S> J40_DEV uint64_t modular_xyb_rgba16(S c0, S c1, S c2, int32_t a, const ModXybConsts &k, const J40_LDS float *thr) {
	float v[3];
	modular_sample_to_xyb(c0, c1, c2, k.m, v);
	return (xyb_to_rgba16(v[0], v[1], v[2], k.cc, thr) & 0x0000ffffffffffffull) | (uint64_t) scale_to_u16(a, k.cc.bpp) << 48;
}

// ---- one lane's work ----
// A lane takes MODXYB_PX consecutive samples of one row of the rectangle: 8 bytes of an int16 plane, 16 of an int32 plane, as one load
// where the address allows it (the reason is the programming guide's figure for scalar 2-byte loads, about twice the time of wide ones; not
// measured here against a one-sample-per-lane form of this kernel) and sample by sample otherwise --
// which a whole row of lanes decides alike, since every lane of a row is a multiple of the load's size away from the first. Only samples
// of the rectangle are read, only its pixels written.
enum { MODXYB_PX = 4, MODXYB_LANES_X = 64, MODXYB_ROWS = 4 };   // a workgroup of 256: 256 pixels of 4 rows

template <typename T, int N> struct ModXybVec { T v[N]; };

template <typename S> J40_DEV void modxyb_load(const S *p, int32_t n, S out[MODXYB_PX]) {
	if (n == MODXYB_PX && ((uintptr_t) p & (sizeof(S) * MODXYB_PX - 1)) == 0) {
		ModXybVec<S, MODXYB_PX> w;
		__builtin_memcpy(&w, __builtin_assume_aligned(p, sizeof(S) * MODXYB_PX), sizeof w);
#pragma unroll
		for (int i = 0; i < MODXYB_PX; ++i) out[i] = w.v[i];
		return;
	}
#pragma unroll
	for (int i = 0; i < MODXYB_PX; ++i) out[i] = i < n ? p[i] : (S) 0;
}

#if defined(__HIP_DEVICE_COMPILE__)
typedef uint32_t modxyb_u32x4 __attribute__((ext_vector_type(4)));
#endif
// n pixels of P bytes at `to` (pixel-aligned): 16-byte pieces where all MODXYB_PX are there and the address allows it
J40_DEV void modxyb_store(const uint32_t px[MODXYB_PX], int32_t n, uint8_t *to) {
	if (n == MODXYB_PX && ((uintptr_t) to & 15) == 0) {
#if defined(__HIP_DEVICE_COMPILE__)
		const modxyb_u32x4 w = {px[0], px[1], px[2], px[3]};
		__builtin_nontemporal_store(w, (modxyb_u32x4 *) to);
#else
		memcpy(to, px, 16);
#endif
		return;
	}
	for (int i = 0; i < n; ++i) {
#if defined(__HIP_DEVICE_COMPILE__)
		__builtin_nontemporal_store(px[i], (uint32_t *) to + i);
#else
		memcpy(to + 4 * i, &px[i], 4);
#endif
	}
}
J40_DEV void modxyb_store(const uint64_t px[MODXYB_PX], int32_t n, uint8_t *to) {
	if (n == MODXYB_PX && ((uintptr_t) to & 15) == 0) {
#if defined(__HIP_DEVICE_COMPILE__)
		const modxyb_u32x4 w0 = {(uint32_t) px[0], (uint32_t) (px[0] >> 32), (uint32_t) px[1], (uint32_t) (px[1] >> 32)};
		const modxyb_u32x4 w1 = {(uint32_t) px[2], (uint32_t) (px[2] >> 32), (uint32_t) px[3], (uint32_t) (px[3] >> 32)};
		__builtin_nontemporal_store(w0, (modxyb_u32x4 *) to);
		__builtin_nontemporal_store(w1, (modxyb_u32x4 *) to + 1);
#else
		memcpy(to, px, 32);
#endif
		return;
	}
	for (int i = 0; i < n; ++i) {
#if defined(__HIP_DEVICE_COMPILE__)
		__builtin_nontemporal_store(px[i], (uint64_t *) to + i);
#else
		memcpy(to + 8 * i, &px[i], 8);
#endif
	}
}

// the rectangle (x0, y0, rw, rh) of planes `plane_width` samples wide; pixel (x, y) of the picture goes to rgba + y * stride + x * P
struct ModXybRect { int32_t plane_width, x0, y0, rw, rh; };

// lane (lx, ly) of the rectangle's lane grid: samples x0 + MODXYB_PX * lx .. of row y0 + ly. a: null where there is no alpha plane.
template <typename S, bool RGBA16>
J40_DEV void modular_xyb_pack_lane(const S *c0, const S *c1, const S *c2, const S *a, const ModXybRect &r, int32_t lx, int32_t ly, const ModXybConsts &k,
		const J40_LDS float *thr, uint8_t *rgba, size_t stride_bytes) {
	const int32_t rx = lx * MODXYB_PX;
	if (ly >= r.rh || rx >= r.rw) return;
	const int32_t n = r.rw - rx < MODXYB_PX ? r.rw - rx : MODXYB_PX;
	const size_t x = (size_t) r.x0 + (size_t) rx, y = (size_t) r.y0 + (size_t) ly, i = y * (size_t) r.plane_width + x;
	S s0[MODXYB_PX], s1[MODXYB_PX], s2[MODXYB_PX], sa[MODXYB_PX];
	modxyb_load(c0 + i, n, s0); modxyb_load(c1 + i, n, s1); modxyb_load(c2 + i, n, s2);
	const int32_t opaque = (1 << k.cc.bpp) - 1;
	if (a) modxyb_load(a + i, n, sa);
	if constexpr (RGBA16) {
		uint64_t px[MODXYB_PX];
#pragma unroll
		for (int j = 0; j < MODXYB_PX; ++j) px[j] = modular_xyb_rgba16(s0[j], s1[j], s2[j], a ? (int32_t) sa[j] : opaque, k, thr);
		modxyb_store(px, n, rgba + y * stride_bytes + x * 8);
	} else {
		uint32_t px[MODXYB_PX];
#pragma unroll
		for (int j = 0; j < MODXYB_PX; ++j) px[j] = modular_xyb_rgba8(s0[j], s1[j], s2[j], a ? (int32_t) sa[j] : opaque, k, thr);
		modxyb_store(px, n, rgba + y * stride_bytes + x * 4);
	}
}

// the same lane for the planes alone: X, Y, B at out[0..2], `pitch` floats a row, the rectangle's sample (0, 0) first
template <typename S>
J40_DEV void modular_to_xyb_lane(const S *c0, const S *c1, const S *c2, const ModXybRect &r, int32_t lx, int32_t ly, const float m[3], float *const out[3], size_t pitch) {
	const int32_t rx = lx * MODXYB_PX;
	if (ly >= r.rh || rx >= r.rw) return;
	const int32_t n = r.rw - rx < MODXYB_PX ? r.rw - rx : MODXYB_PX;
	const size_t i = ((size_t) r.y0 + (size_t) ly) * (size_t) r.plane_width + (size_t) r.x0 + (size_t) rx, o = (size_t) ly * pitch + (size_t) rx;
	S s0[MODXYB_PX], s1[MODXYB_PX], s2[MODXYB_PX];
	modxyb_load(c0 + i, n, s0); modxyb_load(c1 + i, n, s1); modxyb_load(c2 + i, n, s2);
	for (int j = 0; j < n; ++j) {
		float v[3];
		modular_sample_to_xyb(s0[j], s1[j], s2[j], m, v);
		out[0][o + (size_t) j] = v[0]; out[1][o + (size_t) j] = v[1]; out[2][o + (size_t) j] = v[2];
	}
}

} // namespace j40hip
