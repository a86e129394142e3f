// tests/hostsim/orient_sim.cpp -- oriented output on the CPU (tests/test_orient.py): device/orient_dev.h's functions, the ones k_orient
// runs, lane by lane over an image in host memory: without a device. Orientations 2 to 4 as launch_orient launches k_orient_rows;
// 5 to 8 tile by tile as k_orient_tiles: every lane's load, then (where the kernel has its one barrier) every lane's store.
#include <cstdint>
#include <cstring>
#include <vector>
#include "../../j40_amd/csrc/device/orient_dev.h"

using namespace j40hip;

#define ORIENT_SIM_API extern "C" __attribute__((visibility("default")))

template <int PB> static void orient_sim_image(uint8_t *out, size_t out_stride, const uint8_t *src, size_t src_stride, int32_t W, int32_t H, int32_t o, int32_t lanes) {
	if (o == 1) { for (int32_t y = 0; y < H; ++y) memcpy(out + (size_t) y * out_stride, src + (size_t) y * src_stride, (size_t) W * PB); return; }
	if (!orient_transposes(o)) {
		for (int32_t j = 0; j < H; ++j) for (int32_t lane = 0; lane < lanes; ++lane) orient_row<PB>(src, src_stride, out + (size_t) j * out_stride, W, H, o, j, lane, lanes);
		return;
	}
	std::vector<typename OrientPixel<PB>::type> tile(ORIENT_TILE_PIXELS);
	for (int32_t sy0 = 0; sy0 < H; sy0 += ORIENT_TILE) for (int32_t sx0 = 0; sx0 < W; sx0 += ORIENT_TILE) {
		// (what a tile held before is no pixel of this one: a lane that reads where none was loaded shows)
		memset(tile.data(), 0x5A, tile.size() * sizeof tile[0]);
		for (int32_t lane = 0; lane < ORIENT_LANES; ++lane) orient_tile_load<PB>(tile.data(), src, src_stride, W, H, sx0, sy0, lane);
		for (int32_t lane = 0; lane < ORIENT_LANES; ++lane) orient_tile_store<PB>(tile.data(), out, out_stride, W, H, o, sx0, sy0, lane);
	}
}

// what launch_orient launches. pixel_bytes: 4 (u8x4) or 8 (u16x4); lanes: the lanes along a row of orientations 2 to 4
ORIENT_SIM_API void orient_sim(uint8_t *out, size_t out_stride, const uint8_t *src, size_t src_stride, int32_t W, int32_t H, int32_t o, int32_t pixel_bytes, int32_t lanes) {
	if (pixel_bytes == 8) orient_sim_image<8>(out, out_stride, src, src_stride, W, H, o, lanes);
	else orient_sim_image<4>(out, out_stride, src, src_stride, W, H, o, lanes);
}

// out2: the oriented size of a W x H image
ORIENT_SIM_API void orient_sim_size(int32_t W, int32_t H, int32_t o, int32_t *out2) { orient_out_size(W, H, o, &out2[0], &out2[1]); }
// out2: the stored pixel that output pixel (i, j) shows
ORIENT_SIM_API void orient_sim_source(int32_t W, int32_t H, int32_t o, int32_t i, int32_t j, int32_t *out2) { orient_source(W, H, o, i, j, &out2[0], &out2[1]); }
// a rectangle between the oriented and the stored image
ORIENT_SIM_API void orient_sim_rect(int32_t W, int32_t H, int32_t o, int32_t to_stored, const int32_t *in4, int32_t *out4) {
	if (to_stored) orient_rect_to_stored(W, H, o, in4, out4); else orient_rect_to_displayed(W, H, o, in4, out4);
}
ORIENT_SIM_API int32_t orient_sim_tile() { return ORIENT_TILE; }
