// j40_amd/csrc/device/ycbcr_dev.h -- the tail of a YCbCr VarDCT frame (a recompressed JPEG; j40hip_frame_set_ycbcr): from the three
// float planes the pixel kernels leave -- slot 0 Cb, 1 Y, 2 Cr, each at its own resolution -- to finished RGBA. Chroma upsampling
// where a channel is shifted, the colour conversion, the pack. Compiled for the device by ycbcr_kernels.hip and for the CPU by
// tests/hostsim/ycbcr_sim.cpp: the same functions.
//
// The reference refuses such frames (j40.h:7867), so none of this arithmetic is its own; it is pinned to JPEG's definition on the
// integers of real JPEG files (tests/test_jpeg_transcode.py; DESIGN.md, "YCbCr frames", also for what stays PARITY UNPINNED).
//   upsampling  by 2 per shifted axis, horizontal first, then vertical on the horizontally upsampled values:
//               out[2i] = 0.75 in[i] + 0.25 in[i-1], out[2i+1] = 0.75 in[i] + 0.25 in[i+1]; in[-1] = in[0] and in[n] = in[n-1] at the
//               PLANE's border only (the plane reaches the padded block grid, beyond the picture)
//   colour      k = 128/255; R = Y + 1.402 Cr + k, G = Y - 0.344136286 Cb - 0.714136286 Cr + k, B = Y + 1.772 Cb + k, left to right
//   pack        u8: clamp(floor(v * 255 + 0.5)); u16: the level p = clamp(floor(v * (2^bpp - 1) + 0.5)) through the J40_U16X4 rule
//               (alpha_dev.h's alpha_value<true>: (p * 65535 + 2^(bpp-1)) / (2^bpp - 1)); A opaque
// Everything in float32, no contraction (the build passes -ffp-contract=off on both sides).
#pragma once
#include "alpha_dev.h"

namespace j40hip {

// one launch: the planes (`pitch` floats a row, pw x ph samples), each channel's shifts (0 or 1), the picture's size
struct YcbcrTail {
	const float *plane[3];
	int32_t pitch[3], pw[3], ph[3], hshift[3], vshift[3];
	int32_t width, height;
	float maxv;        // the level scale: 255 (u8), 2^bpp - 1 (u16)
	AlphaScale s16;    // u16: the level's way to 16 bits
};

// 0, or what is wrong with a launch's arguments: every plane must cover the picture at its own resolution
J40_HD bool ycbcr_tail_valid(const YcbcrTail &t) {
	if (t.width < 1 || t.height < 1) return false;
	for (int c = 0; c < 3; ++c) {
		if (!t.plane[c] || t.hshift[c] < 0 || t.hshift[c] > 1 || t.vshift[c] < 0 || t.vshift[c] > 1) return false;
		if (t.pw[c] < 1 || t.ph[c] < 1 || t.pitch[c] < t.pw[c]) return false;
		if (((int64_t) t.pw[c] << t.hshift[c]) < t.width || ((int64_t) t.ph[c] << t.vshift[c]) < t.height) return false;
	}
	return true;
}

// the planes of a subsampled frame (DevFrame::ycc_shifts: hshift | vshift << 1 of channel c at bits 2c): the block grid padded to whole
// MCUs, in samples, at each channel's resolution
J40_HD void ycc_plane_dims(int32_t width, int32_t height, uint32_t shifts, int32_t pw[3], int32_t ph[3]) {
	int32_t mh = 0, mv = 0;
	for (int c = 0; c < 3; ++c) { mh |= (int32_t) ((shifts >> (2 * c)) & 1u); mv |= (int32_t) ((shifts >> (2 * c + 1)) & 1u); }
	const int32_t fw = ((width + (8 << mh) - 1) / (8 << mh)) << (mh + 3), fh = ((height + (8 << mv) - 1) / (8 << mv)) << (mv + 3);
	for (int c = 0; c < 3; ++c) { pw[c] = fw >> ((shifts >> (2 * c)) & 1u); ph[c] = fh >> ((shifts >> (2 * c + 1)) & 1u); }
}

J40_HD int32_t ycbcr_clampi(int32_t v, int32_t hi) { return v < 0 ? 0 : v > hi ? hi : v; }

// samples x0 .. x0 + 3 (x0 a multiple of 4) of one plane row after the horizontal step; columns beyond the plane repeat its last
J40_HD void ycbcr_row4(const J40_GLOBAL float *row, int32_t pw, int32_t x0, int32_t hshift, bool aligned, float o[4]) {
	if (!hshift) {
		if (aligned && x0 + 3 < pw) {   // one 16-byte load
#ifdef __HIP_DEVICE_COMPILE__
			typedef float f32x4 __attribute__((ext_vector_type(4)));
			const f32x4 v = *(const J40_GLOBAL f32x4 *) (row + x0);
			o[0] = v.x; o[1] = v.y; o[2] = v.z; o[3] = v.w;
#else
			for (int i = 0; i < 4; ++i) o[i] = row[x0 + i];
#endif
		} else for (int i = 0; i < 4; ++i) o[i] = row[ycbcr_clampi(x0 + i, pw - 1)];
		return;
	}
	const int32_t i = x0 >> 1;
	const float a = row[ycbcr_clampi(i - 1, pw - 1)], b = row[ycbcr_clampi(i, pw - 1)], c = row[ycbcr_clampi(i + 1, pw - 1)], d = row[ycbcr_clampi(i + 2, pw - 1)];
	o[0] = 0.75f * b + 0.25f * a; o[1] = 0.75f * b + 0.25f * c;
	o[2] = 0.75f * c + 0.25f * b; o[3] = 0.75f * c + 0.25f * d;
}

// channel c at pixels (x0 .. x0 + 3, y) of the picture
J40_HD void ycbcr_channel4(const YcbcrTail &t, int c, int32_t x0, int32_t y, float o[4]) {
	const J40_GLOBAL float *base = (const J40_GLOBAL float *) t.plane[c];
	const bool aligned = (t.pitch[c] & 3) == 0 && ((uintptr_t) t.plane[c] & 15u) == 0;
	if (!t.vshift[c]) { ycbcr_row4(base + (size_t) ycbcr_clampi(y, t.ph[c] - 1) * (size_t) t.pitch[c], t.pw[c], x0, t.hshift[c], aligned, o); return; }
	const int32_t j = ycbcr_clampi(y >> 1, t.ph[c] - 1), other = ycbcr_clampi((y & 1) ? j + 1 : j - 1, t.ph[c] - 1);
	float near[4], far[4];
	ycbcr_row4(base + (size_t) j * (size_t) t.pitch[c], t.pw[c], x0, t.hshift[c], aligned, near);
	ycbcr_row4(base + (size_t) other * (size_t) t.pitch[c], t.pw[c], x0, t.hshift[c], aligned, far);
	for (int i = 0; i < 4; ++i) o[i] = 0.75f * near[i] + 0.25f * far[i];
}

// a colour sample to its level: clamp(floor(v * maxv + 0.5)); a NaN gives 0
J40_HD uint32_t ycbcr_level(float v, float maxv) {
	const float s = floorf(v * maxv + 0.5f);
	return !(s > 0.0f) ? 0u : s > maxv ? (uint32_t) maxv : (uint32_t) s;
}

// one pixel: u8 -- a word R | G << 8 | B << 16 | 255 << 24 in px[0]; u16 -- R | G << 16 in px[0], B | 65535 << 16 in px[1]
template <bool OUT16> J40_HD void ycbcr_pixel(float cb, float yy, float cr, const YcbcrTail &t, uint32_t px[2]) {
	const float k = 128.0f / 255.0f;
	const float r = yy + 1.402f * cr + k;
	const float g = yy - 0.344136286f * cb - 0.714136286f * cr + k;
	const float b = yy + 1.772f * cb + k;
	const uint32_t lr = ycbcr_level(r, t.maxv), lg = ycbcr_level(g, t.maxv), lb = ycbcr_level(b, t.maxv);
	if (OUT16) {
		px[0] = alpha_value<true>((int32_t) lr, t.s16) | alpha_value<true>((int32_t) lg, t.s16) << 16;
		px[1] = alpha_value<true>((int32_t) lb, t.s16) | 0xffff0000u;
	} else { px[0] = lr | lg << 8 | lb << 16 | 0xff000000u; px[1] = 0; }
}

// chunk k of row y: pixels 4k .. 4k + 3, those inside the picture only. `out_row`: the row's first pixel (pixel-aligned)
template <bool OUT16> J40_HD void ycbcr_tail_chunk(const YcbcrTail &t, J40_GLOBAL uint8_t *out_row, int32_t y, int32_t k) {
	const int32_t x0 = 4 * k, n = t.width - x0 < 4 ? t.width - x0 : 4;
	if (n <= 0) return;
	float cb[4], yy[4], cr[4];
	ycbcr_channel4(t, 1, x0, y, yy);
	ycbcr_channel4(t, 0, x0, y, cb);
	ycbcr_channel4(t, 2, x0, y, cr);
	uint32_t px[4][2];
	for (int i = 0; i < 4; ++i) ycbcr_pixel<OUT16>(cb[i], yy[i], cr[i], t, px[i]);
	J40_GLOBAL uint8_t *q = out_row + (size_t) x0 * (OUT16 ? 8 : 4);
#ifdef __HIP_DEVICE_COMPILE__
	if (n == 4 && ((uintptr_t) q & 15u) == 0) {   // the wide path: written once, never read here
		typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
		if (OUT16) {
			const u32x4 lo = {px[0][0], px[0][1], px[1][0], px[1][1]}, hi = {px[2][0], px[2][1], px[3][0], px[3][1]};
			__builtin_nontemporal_store(lo, (J40_GLOBAL u32x4 *) q); __builtin_nontemporal_store(hi, (J40_GLOBAL u32x4 *) q + 1);
		} else {
			const u32x4 v = {px[0][0], px[1][0], px[2][0], px[3][0]};
			__builtin_nontemporal_store(v, (J40_GLOBAL u32x4 *) q);
		}
		return;
	}
#endif
	for (int i = 0; i < n; ++i) {   // rows that are only pixel-aligned, and the row's last pixels
		J40_GLOBAL uint32_t *p = (J40_GLOBAL uint32_t *) (q + (size_t) i * (OUT16 ? 8 : 4));
		p[0] = px[i][0];
		if (OUT16) p[1] = px[i][1];
	}
}

// the parameters of a launch for planes one behind the other; format: out16
J40_HD void ycbcr_tail_scale(YcbcrTail *t, int32_t bpp, bool out16) {
	t->maxv = out16 ? (float) ((1u << bpp) - 1u) : 255.0f;
	t->s16 = alpha_scale_make(out16 ? bpp : 8, out16);
}

} // namespace j40hip
