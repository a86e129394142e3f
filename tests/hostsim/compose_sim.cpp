// tests/hostsim/compose_sim.cpp -- frame composition on the CPU (tests/test_frames.py): device/compose_dev.h's clipping and row
// functions, the ones k_frame_compose runs, lane by lane over a canvas in host memory: without a device.
#include <cstdint>
#include <cstring>
#include "../../j40_amd/csrc/device/compose_dev.h"

using namespace j40hip;

#define COMPOSE_SIM_API extern "C" __attribute__((visibility("default")))

// what launch_frame_compose launches: rows [0, H) of the canvas -- with out == src the rectangle's rows alone --, `lanes` lanes a row.
// format: 4 or 8 bytes a pixel
COMPOSE_SIM_API void compose_sim(uint8_t *out, size_t out_stride, const uint8_t *src, size_t src_stride, const uint8_t *frm, size_t frm_stride, int32_t W, int32_t H,
		int32_t x0, int32_t y0, int32_t w, int32_t h, uint32_t empty_lo, uint32_t empty_hi, int32_t pixel_bytes, int32_t lanes) {
	const ComposeRect r = compose_clip(W, H, x0, y0, w, h);
	const bool only_rect = src == out;
	const int32_t first = only_rect ? r.cy0 : 0, last = only_rect ? r.cy1 : H;
	for (int32_t y = first; y < last; ++y) for (int32_t lane = 0; lane < lanes; ++lane) {
		uint8_t *o = out + (size_t) y * out_stride; const uint8_t *s = src ? src + (size_t) y * src_stride : nullptr;
		if (pixel_bytes == 8) compose_row<8>(o, s, frm, frm_stride, W, y, r, empty_lo, empty_hi, only_rect, lane, lanes);
		else compose_row<4>(o, s, frm, frm_stride, W, y, r, empty_lo, empty_hi, only_rect, lane, lanes);
	}
}

// out6: compose_clip's cx0, cy0, cx1, cy1, fx, fy
COMPOSE_SIM_API void compose_sim_clip(int32_t W, int32_t H, int32_t x0, int32_t y0, int32_t w, int32_t h, int32_t *out6) {
	const ComposeRect r = compose_clip(W, H, x0, y0, w, h);
	out6[0] = r.cx0; out6[1] = r.cy0; out6[2] = r.cx1; out6[3] = r.cy1; out6[4] = r.fx; out6[5] = r.fy;
}
