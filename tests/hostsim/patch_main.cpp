// tests/hostsim/patch_main.cpp -- patch_sim.cpp as a program of its own (tests/test_patches.py runs it plain and built with the host
// sanitizers; an executable, never loaded into Python): random placement lists over frames whose sizes are no multiples of the tile, the
// planes and the slots each in an allocation of exactly its size, so that a lane that steps outside a plane, a slot or the record lists is
// caught. The result is compared with the placements applied one after the other, sample by sample.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <vector>
#include "../../j40_amd/csrc/device/patch_dev.h"

extern "C" uint32_t patch_sim_apply(float *planes, int32_t W, int32_t H, const float *const slot[4], const int32_t slot_w[4], const int32_t slot_h[4], const int32_t *placements, int32_t count);

static uint64_t g_state = 0x9e3779b97f4a7c15ull;
static uint32_t rnd(uint32_t n) { g_state = g_state * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t) (g_state >> 33) % n; }
static float rndf() { return (float) ((int32_t) rnd(4001) - 2000) / 1000.0f; }

int main() {
	static const int32_t SIZES[][2] = {{200, 136}, {64, 32}, {65, 33}, {1, 1}, {300, 270}, {63, 200}};
	int failures = 0;
	for (const auto &size : SIZES) for (int round = 0; round < 4; ++round) {
		const int32_t W = size[0], H = size[1];
		const int32_t sw[4] = {(int32_t) (1 + rnd(2 * W)), W, 0, (int32_t) (1 + rnd(40))}, sh[4] = {(int32_t) (1 + rnd(2 * H)), H, 0, (int32_t) (1 + rnd(40))};
		std::vector<std::vector<float>> slot(4);
		const float *sp[4];
		for (int k = 0; k < 4; ++k) { slot[k].resize((size_t) 3 * sw[k] * sh[k]); for (float &v : slot[k]) v = rndf(); sp[k] = slot[k].empty() ? nullptr : slot[k].data(); }
		std::vector<float> planes((size_t) 3 * W * H), want;
		for (float &v : planes) v = rndf();
		want = planes;
		const int32_t count = round == 0 ? 1 : (int32_t) (1 + rnd(200));   // (200: several chunks of records in the tiles they crowd into)
		std::vector<int32_t> pl;
		for (int32_t i = 0; i < count; ++i) {
			const int32_t k = rnd(3) == 0 ? 3 : (int32_t) rnd(2);
			const int32_t w = 1 + (int32_t) rnd((uint32_t) (sw[k] < W ? sw[k] : W)), h = 1 + (int32_t) rnd((uint32_t) (sh[k] < H ? sh[k] : H));
			const int32_t v[9] = {(int32_t) rnd((uint32_t) (W - w + 1)), (int32_t) rnd((uint32_t) (H - h + 1)), w, h, (int32_t) rnd((uint32_t) (sw[k] - w + 1)), (int32_t) rnd((uint32_t) (sh[k] - h + 1)), k, (int32_t) rnd(4), (int32_t) rnd(2)};
			pl.insert(pl.end(), v, v + 9);
			for (int c = 0; c < 3; ++c) for (int32_t y = 0; y < h; ++y) for (int32_t x = 0; x < w; ++x) {
				float &d = want[((size_t) c * H + (size_t) (v[1] + y)) * W + (size_t) (v[0] + x)];
				const float s = slot[k][((size_t) c * sh[k] + (size_t) (v[5] + y)) * sw[k] + (size_t) (v[4] + x)];
				d = j40hip::patch_blend(v[7], v[8], d, s);
			}
		}
		const uint32_t e = patch_sim_apply(planes.data(), W, H, sp, sw, sh, pl.data(), count);
		if (e || memcmp(planes.data(), want.data(), planes.size() * 4) != 0) { fprintf(stderr, "patch_main: %dx%d round %d: code %08x, planes %s\n", W, H, round, e, e ? "untouched" : "differ"); ++failures; }
	}
	{   // what the check refuses: an empty slot, a rectangle past its slot, a placement past the frame
		const float one[3] = {0, 0, 0}; const float *sp[4] = {one, nullptr, nullptr, nullptr}; const int32_t sw[4] = {1, 0, 0, 0}, sh[4] = {1, 0, 0, 0};
		float px[3] = {0, 0, 0};
		const int32_t empty[9] = {0, 0, 1, 1, 0, 0, 1, 1, 0}, past_slot[9] = {0, 0, 1, 1, 1, 0, 0, 1, 0}, past_frame[9] = {1, 0, 1, 1, 0, 0, 0, 1, 0};
		if (patch_sim_apply(px, 1, 1, sp, sw, sh, empty, 1) != 0x70746e6fu || patch_sim_apply(px, 1, 1, sp, sw, sh, past_slot, 1) != 0x70746368u || patch_sim_apply(px, 1, 1, sp, sw, sh, past_frame, 1) != 0x70746368u) { fprintf(stderr, "patch_main: the check let a bad list through\n"); ++failures; }
	}
	{   // a legal list whose binned total is over patch_bin_limit: refused before anything is counted or allocated, however long it is
		const int32_t W = 2048, H = 2048, sw[4] = {W, 0, 0, 0}, sh[4] = {H, 0, 0, 0};
		std::vector<float> planes((size_t) 3 * W * H, 0.0f), slot((size_t) 3 * W * H, 1.0f);
		const float *sp[4] = {slot.data(), nullptr, nullptr, nullptr};
		const int64_t limit = j40hip::patch_bin_limit(W, H);
		const int32_t tiles = (W / 64) * (H / 32), fits = (int32_t) (limit / tiles);   // whole-frame placements that fit
		for (int32_t count : {fits, fits + 1, 2097252}) {   // (the last: what wrapped a 32-bit total to a small positive number)
			std::vector<int32_t> pl;
			for (int32_t i = 0; i < count; ++i) { const int32_t v[9] = {0, 0, W, H, 0, 0, 0, 2, 0}; pl.insert(pl.end(), v, v + 9); }
			if (count > fits) { std::fill(planes.begin(), planes.end(), 0.0f); }
			const uint32_t e = patch_sim_apply(planes.data(), W, H, sp, sw, sh, pl.data(), count);
			const bool ok = count <= fits ? e == 0 && planes[0] == (float) fits && planes.back() == (float) fits : e == 0x70746368u && planes[0] == 0.0f;
			if (!ok) { fprintf(stderr, "patch_main: %d whole-frame placements on %dx%d: code %08x\n", count, W, H, e); ++failures; }
		}
	}
	printf("patch_main: %d failure(s)\n", failures);
	return failures ? 1 : 0;
}
