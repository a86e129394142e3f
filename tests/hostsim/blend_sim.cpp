// tests/hostsim/blend_sim.cpp -- the blend modes of a frame sequence on the CPU (tests/test_blend.py): device/compose_dev.h's blend_row,
// the function k_frame_blend runs, lane by lane over a canvas in host memory: without a device.
#include <cstdint>
#include <cstring>
#include "../../j40_amd/csrc/device/compose_dev.h"

using namespace j40hip;

#define BLEND_SIM_API extern "C" __attribute__((visibility("default")))

// what launch_frame_blend launches: rows [0, H) of the canvas -- with out == src the rectangle's rows alone --, `lanes` lanes a row.
// pixel_bytes: 4 or 8; cmode, amode: the colour channels' and the alpha's blend mode, 0..4
BLEND_SIM_API void blend_sim(uint8_t *out, size_t out_stride, const uint8_t *src, size_t src_stride, const uint8_t *frm, size_t frm_stride, int32_t W, int32_t H,
		int32_t x0, int32_t y0, int32_t w, int32_t h, uint32_t empty_lo, uint32_t empty_hi, int32_t pixel_bytes, int32_t cmode, int32_t amode, int32_t lanes) {
	const ComposeRect r = compose_clip(W, H, x0, y0, w, h);
	const bool only_rect = src == out;
	const int32_t first = only_rect ? r.cy0 : 0, last = only_rect ? r.cy1 : H;
	for (int32_t y = first; y < last; ++y) for (int32_t lane = 0; lane < lanes; ++lane) {
		uint8_t *o = out + (size_t) y * out_stride; const uint8_t *s = src ? src + (size_t) y * src_stride : nullptr;
		if (pixel_bytes == 8) blend_row<8>(o, s, frm, frm_stride, W, y, r, empty_lo, empty_hi, only_rect, cmode, amode, lane, lanes);
		else blend_row<4>(o, s, frm, frm_stride, W, y, r, empty_lo, empty_hi, only_rect, cmode, amode, lane, lanes);
	}
}
