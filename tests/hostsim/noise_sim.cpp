// tests/hostsim/noise_sim.cpp -- photon noise on the CPU (tests/test_noise.py): device/noise_dev.h's generator in its sequential and its
// jumped form and the tile functions k_noise_add is made of, over planes in host memory. A workgroup's threads run one after the other
// here; each owns its rows (the fill) or its pixels (the addition, which reads only the staged tile and its own samples), so the order
// between them cannot matter -- which is the kernels' claim too.
#include <stdint.h>
#include <string.h>
#include <vector>
#include "../../j40_amd/csrc/device/noise_dev.h"

using namespace j40hip;

namespace {
NoiseFillArgs fill_args(int32_t W, int32_t H, int32_t gdim, uint32_t visible, uint32_t nonvisible) {
	NoiseFillArgs a = {W, H, gdim, (W + gdim - 1) / gdim, (H + gdim - 1) / gdim, visible, nonvisible};
	return a;
}
bool fill_args_valid(int32_t W, int32_t H, int32_t gdim) { return W > 0 && H > 0 && gdim >= 16 && gdim <= 1024 && gdim % 16 == 0; }
}

extern "C" {

// `steps` steps of the eight lanes seeded for a group at (x0, y0): out[16 * s + 2 * i], [.. + 1] = the low and the high half of lane i's output
__attribute__((visibility("default"))) void noise_sim_steps(uint32_t visible, uint32_t nonvisible, uint32_t x0, uint32_t y0, int32_t steps, uint32_t *out) {
	NoiseState st[NOISE_LANES];
	for (int32_t i = 0; i < NOISE_LANES; ++i) st[i] = noise_seed_lane(visible, nonvisible, x0, y0, i);
	for (int32_t s = 0; s < steps; ++s) for (int32_t i = 0; i < NOISE_LANES; ++i) {
		const uint64_t v = noise_step(st[i]);
		out[16 * s + 2 * i] = (uint32_t) v; out[16 * s + 2 * i + 1] = (uint32_t) (v >> 32);
	}
}

__attribute__((visibility("default"))) int64_t noise_sim_pitch(int32_t W) { return (int64_t) noise_pitch(W); }

// the three raw planes of a W x H frame with groups of gdim samples a side, [3][H][noise_sim_pitch(W)] floats: jumped = 0 the sequential
// form, 1 the jumped one (every thread of every group's workgroup, one after the other). What lies behind column W of a row is
// whatever the form leaves there. Returns 0, or -1 for sizes the fill does not take.
__attribute__((visibility("default"))) int32_t noise_sim_fill(float *raw, int32_t W, int32_t H, int32_t gdim, uint32_t visible, uint32_t nonvisible, int32_t jumped) {
	if (!fill_args_valid(W, H, gdim)) return -1;
	const NoiseFillArgs a = fill_args(W, H, gdim, visible, nonvisible);
	const size_t pitch = noise_pitch(W), plane = pitch * (size_t) H;
	if (!jumped) { for (int32_t g = 0; g < a.gcols * a.grows; ++g) noise_fill_group_sequential(raw, pitch, plane, a, g); return 0; }
	std::vector<uint64_t> sets((size_t) 4 * NOISE_SET_WORDS);
	noise_frame_jumps(a, sets.data());
	for (int32_t g = 0; g < a.gcols * a.grows; ++g) for (int32_t t = 0; t < NOISE_FILL_THREADS; ++t) noise_fill_lane(raw, pitch, plane, a, sets.data(), g, t);
	return 0;
}

// k_noise_add over planes [3][H][W] (X, Y, B), in place, from raw planes [3][H][noise_sim_pitch(W)]: every tile staged, then its 256 lanes
__attribute__((visibility("default"))) void noise_sim_add(float *planes, const float *raw, int32_t W, int32_t H, const float *lut8, float ytox, float ytob) {
	NoiseParams p;
	memcpy(p.lut, lut8, sizeof p.lut);
	p.ytox = ytox; p.ytob = ytob;
	const size_t pitch = noise_pitch(W), plane = pitch * (size_t) H;
	std::vector<float> tile((size_t) NOISE_LDS_FLOATS);
	for (int32_t ty = 0; ty < (H + NOISE_TILE_H - 1) / NOISE_TILE_H; ++ty) for (int32_t tx = 0; tx < (W + NOISE_TILE_W - 1) / NOISE_TILE_W; ++tx) {
		for (int32_t t = 0; t < NOISE_TILE_W * NOISE_WAVES; ++t) noise_tile_stage(tile.data(), raw, pitch, plane, W, H, tx, ty, t);
		for (int32_t wave = 0; wave < NOISE_WAVES; ++wave) for (int32_t lane = 0; lane < NOISE_TILE_W; ++lane) noise_tile_lane(planes, (size_t) W, (size_t) W * (size_t) H, W, H, tile.data(), p, tx, ty, lane, wave);
	}
}

__attribute__((visibility("default"))) float noise_sim_strength(const float *lut8, float v) { return noise_strength(lut8, v); }

} // extern "C"
