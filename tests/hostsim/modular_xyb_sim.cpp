// tests/hostsim/modular_xyb_sim.cpp -- TEST INFRASTRUCTURE ONLY. A Modular frame of an XYB image through the XYB colour tail on the CPU
// (tests/test_modular_xyb.py): device/modular_xyb_dev.h's lane functions, the ones k_modular_xyb_pack and k_modular_to_xyb run, walked lane
// by lane over the grid their launchers make, on planes in host memory; and decode_modular's choice between them and the pack functions.
// Never linked into the product library.
#include <cstdint>
#include <cstring>
#include <cmath>
#include "../../j40_amd/csrc/device/modular_xyb_dev.h"
#include "../../j40_amd/csrc/device/modular_dev.h"
#include "../../j40_amd/csrc/tables.hpp"

using namespace j40hip;

#define MODXYB_SIM_API extern "C" __attribute__((visibility("default")))

namespace {

// m[3] and the 15 floats of j40hip_frame_colour_consts, as runtime_state.hpp's modular_xyb_consts makes them of a frame
ModXybConsts consts_of(const float *m, const float *cc15, int32_t bpp) {
	ModXybConsts k;
	for (int c = 0; c < 3; ++c) { k.m[c] = m[c]; k.cc.opsin_bias[c] = cc15[9 + c]; k.cc.cbrt_opsin_bias[c] = cbrtf(cc15[9 + c]); }
	for (int i = 0; i < 9; ++i) k.cc.m[i] = cc15[i];
	k.cc.itscale = 255.0f / cc15[12]; k.cc.bpp = bpp;
	return k;
}

// the lane grid of modxyb_grid (modular_xyb_kernels.hip): whole workgroups of MODXYB_LANES_X x MODXYB_ROWS lanes
template <typename F> void for_lanes(int32_t rw, int32_t rh, F f) {
	const int32_t per_wg = MODXYB_LANES_X * MODXYB_PX, gx = (rw + per_wg - 1) / per_wg, gy = (rh + MODXYB_ROWS - 1) / MODXYB_ROWS;
	for (int32_t ly = 0; ly < gy * MODXYB_ROWS; ++ly) for (int32_t lx = 0; lx < gx * MODXYB_LANES_X; ++lx) f(lx, ly);
}

template <typename S>
void pack_of(const void *const planes[3], const void *alpha, const ModXybRect &r, const ModXybConsts &k, bool rgba16, uint8_t *rgba, size_t stride) {
	const S *c0 = (const S *) planes[0], *c1 = (const S *) planes[1], *c2 = (const S *) planes[2], *a = (const S *) alpha;
	const float *thr = srgb_u8_thresholds();
	for_lanes(r.rw, r.rh, [&](int32_t lx, int32_t ly) {
		if (rgba16) modular_xyb_pack_lane<S, true>(c0, c1, c2, a, r, lx, ly, k, thr, rgba, stride);
		else modular_xyb_pack_lane<S, false>(c0, c1, c2, a, r, lx, ly, k, thr, rgba, stride);
	});
}

// the pack kernels' pixels over the same rectangle (k_pack_planes_rect / k_pack_planes16_rect): what decode_modular launches with the switch off
template <typename S>
void plain_of(const void *const planes[3], const void *alpha, const ModXybRect &r, int32_t bpp, bool rgba16, uint8_t *rgba, size_t stride) {
	const S *c0 = (const S *) planes[0], *c1 = (const S *) planes[1], *c2 = (const S *) planes[2], *a = (const S *) alpha;
	const int32_t opaque = (1 << bpp) - 1;
	for (int32_t y = r.y0; y < r.y0 + r.rh; ++y) for (int32_t x = r.x0; x < r.x0 + r.rw; ++x) {
		const size_t i = (size_t) y * (size_t) r.plane_width + (size_t) x;
		if (rgba16) { const uint64_t px = pack_rgba16(c0[i], c1[i], c2[i], a ? (int32_t) a[i] : opaque, bpp); memcpy(rgba + (size_t) y * stride + (size_t) x * 8, &px, 8); }
		else { const uint32_t px = pack_rgba8(c0[i], c1[i], c2[i], a ? (int32_t) a[i] : opaque, bpp); memcpy(rgba + (size_t) y * stride + (size_t) x * 4, &px, 4); }
	}
}

} // namespace

// k_modular_to_xyb over rectangle (x0, y0, rw, rh) of planes `plane_width` samples wide (sample_bytes 2 or 4): X, Y, B at out[0..2],
// `pitch` floats a row, the rectangle's sample (0, 0) first
MODXYB_SIM_API int32_t modxyb_sim_planes(const void *const planes[3], int32_t sample_bytes, int32_t plane_width, int32_t x0, int32_t y0, int32_t rw, int32_t rh, const float *m, float *const out[3], size_t pitch) {
	if (sample_bytes != 2 && sample_bytes != 4) return -1;
	const ModXybRect r = {plane_width, x0, y0, rw, rh};
	for_lanes(rw, rh, [&](int32_t lx, int32_t ly) {
		if (sample_bytes == 4) modular_to_xyb_lane<int32_t>((const int32_t *) planes[0], (const int32_t *) planes[1], (const int32_t *) planes[2], r, lx, ly, m, out, pitch);
		else modular_to_xyb_lane<int16_t>((const int16_t *) planes[0], (const int16_t *) planes[1], (const int16_t *) planes[2], r, lx, ly, m, out, pitch);
	});
	return 0;
}

// decode_modular's last step over the rectangle: on = 1 k_modular_xyb_pack, on = 0 the pack kernels (m and cc15 unused). Pixel (x, y) of the
// picture goes to rgba + y * stride + x * (4 or 8); alpha: a plane like the others, or null
MODXYB_SIM_API int32_t modxyb_sim_pack(int32_t on, const void *const planes[3], const void *alpha, int32_t sample_bytes, int32_t plane_width, int32_t x0, int32_t y0, int32_t rw, int32_t rh,
		const float *m, const float *cc15, int32_t bpp, int32_t rgba16, uint8_t *rgba, size_t stride) {
	if ((sample_bytes != 2 && sample_bytes != 4) || bpp < 8 || bpp > 16) return -1;
	const ModXybRect r = {plane_width, x0, y0, rw, rh};
	if (!on) {
		if (sample_bytes == 4) plain_of<int32_t>(planes, alpha, r, bpp, rgba16 != 0, rgba, stride); else plain_of<int16_t>(planes, alpha, r, bpp, rgba16 != 0, rgba, stride);
		return 0;
	}
	const ModXybConsts k = consts_of(m, cc15, bpp);
	if (sample_bytes == 4) pack_of<int32_t>(planes, alpha, r, k, rgba16 != 0, rgba, stride); else pack_of<int16_t>(planes, alpha, r, k, rgba16 != 0, rgba, stride);
	return 0;
}
