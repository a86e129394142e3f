// tests/hostsim/upsample_main.cpp -- device/upsample_dev.h as a program of its own (tests/test_upsampling.py runs it plain and built with
// the host sanitizers; an executable, never loaded into Python): coded planes narrower than the halo, one past a tile, a tile's multiple,
// shown sizes cut on both axes, the coded plane, the output and the tile each in an allocation of exactly its size, so that a thread
// that steps outside one is caught. The kernel's tile functions, thread by thread, are compared with the rule sample by sample, bit for bit.
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <vector>
#include "../../j40_amd/csrc/device/upsample_dev.h"

using namespace j40hip;

static uint64_t g_state = 0x9e3779b97f4a7c15ull;
static uint32_t rnd(uint32_t n) { g_state = g_state * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t) (g_state >> 33) % n; }
static float rndf() { return (float) ((int32_t) rnd(4001) - 2000) / 1000.0f; }

template <int K> static int run(int32_t w, int32_t h, int32_t up_w, int32_t up_h) {
	std::vector<float> weights((size_t) upsample_weight_count(K)), e((size_t) K * K * 25), src((size_t) w * h), tiled((size_t) up_w * up_h, -7.0f), plain((size_t) up_w * up_h);
	for (size_t i = 0; i < weights.size(); ++i) weights[i] = (i % 7 == 3 ? 0.6f : 0.03f * rndf());
	for (float &v : src) v = rndf();
	upsample_expand(K, weights.data(), e.data());
	for (int32_t Y = 0; Y < up_h; ++Y) for (int32_t X = 0; X < up_w; ++X) plain[(size_t) Y * up_w + X] = upsample_sample<K>(src.data(), w, h, e.data(), X, Y);
	std::vector<float> tile((size_t) UP_LDS_FLOATS);
	for (int32_t ty = 0; ty < (h + UP_TILE_H - 1) / UP_TILE_H; ++ty) for (int32_t tx = 0; tx < (w + UP_TILE_W - 1) / UP_TILE_W; ++tx) {
		for (int32_t t = 0; t < UP_THREADS; ++t) upsample_tile_stage(tile.data(), src.data(), w, h, tx, ty, t);
		for (int32_t t = 0; t < UP_THREADS; ++t) upsample_tile_lane<K>(tiled.data(), (size_t) up_w, up_w, up_h, w, h, tile.data(), e.data(), tx, ty, t);
	}
	if (memcmp(tiled.data(), plain.data(), plain.size() * sizeof(float)) != 0) { fprintf(stderr, "upsample_main: K = %d, %d x %d -> %d x %d: the tiles differ from the rule\n", K, w, h, up_w, up_h); return 1; }
	return 0;
}

int main() {
	static const int32_t SIZES[][2] = {{1, 1}, {2, 1}, {1, 3}, {5, 5}, {33, 9}, {64, 32}, {67, 35}, {300, 20}, {3, 70}};
	int failures = 0;
	for (const auto &s : SIZES) {
		const int32_t w = s[0], h = s[1];
		failures += run<2>(w, h, 2 * w, 2 * h) + run<4>(w, h, 4 * w, 4 * h) + run<8>(w, h, 8 * w, 8 * h);
		failures += run<2>(w, h, 2 * w - 1, 2 * h - 1) + run<4>(w, h, 4 * w - 1, 4 * h - 3) + run<8>(w, h, 8 * w - 5, 8 * h - 7);
	}
	// the table: symmetric kernels mirror into each other
	std::vector<float> wts(210), e(8 * 8 * 25);
	for (size_t i = 0; i < wts.size(); ++i) wts[i] = (float) (i + 1);
	upsample_expand(8, wts.data(), e.data());
	for (int oy = 0; oy < 8; ++oy) for (int ox = 0; ox < 8; ++ox) for (int sy = 0; sy < 5; ++sy) for (int sx = 0; sx < 5; ++sx)
		if (e[(size_t) ((oy * 8 + ox) * 25 + sy * 5 + sx)] != e[(size_t) (((7 - oy) * 8 + (7 - ox)) * 25 + (4 - sy) * 5 + (4 - sx))]) { ++failures; }
	if (upsample_mirror(-1, 1) != 0 || upsample_mirror(2, 1) != 0 || upsample_mirror(-3, 2) != 1 || upsample_mirror(5, 3) != 0 || upsample_coded_size(599, 2) != 300 || upsample_coded_size(1, 8) != 1) { fprintf(stderr, "upsample_main: mirror or size\n"); ++failures; }
	printf("upsample_main: %d failure(s)\n", failures);
	return failures ? 1 : 0;
}
