// tests/hostsim/spline_sim.cpp -- splines on the CPU (tests/test_splines.py): device/spline_dev.h's erf_r, binning and lane function over
// planes in host memory, as k_spline_draw's workgroups run them. A workgroup's threads run one after the other here; each owns its
// samples and reads only the staged chunk, so the order between them cannot matter -- which is the kernel's claim too.
#include <stdint.h>
#include <string.h>
#include <vector>
#include "../../j40_amd/csrc/device/spline_dev.h"

using namespace j40hip;

extern "C" {

__attribute__((visibility("default"))) void spline_sim_erf(const float *x, int64_t n, float *out) {
	for (int64_t i = 0; i < n; ++i) out[i] = spline_erf(x[i]);
}

__attribute__((visibility("default"))) int32_t spline_sim_chunk() { return SPLINE_CHUNK; }

// k_spline_draw over planes [3][H][W] (X, Y, B), in place, from `n` segments of 12 words in drawing order: binned as the parse bins a
// frame's, then every touched tile -- its segments staged chunk by chunk, each chunk walked by the tile's 256 lanes. Returns the tiles
// run, -1 for a box outside the frame or too many (tile, segment) pairs; most_out (optional): the longest list of a tile
__attribute__((visibility("default"))) int64_t spline_sim_draw(float *planes, int32_t W, int32_t H, const void *segments, int64_t n, int64_t *most_out) {
	if (W <= 0 || H <= 0 || n < 0 || n > SPLINE_MAX_SEGMENTS) return -1;
	SplinePlan plan;
	plan.segs.resize((size_t) n);
	if (n) memcpy(plan.segs.data(), segments, sizeof(SplineSeg) * (size_t) n);
	for (const SplineSeg &g : plan.segs) if (g.x0 < 0 || g.x0 > g.x1 || g.x1 >= W || g.y0 < 0 || g.y0 > g.y1 || g.y1 >= H) return -1;
	if (!spline_bin(W, &plan)) return -1;
	const size_t pitch = (size_t) W, plane = pitch * (size_t) H;
	std::vector<SplineSeg> chunk((size_t) SPLINE_CHUNK);
	int64_t most = 0;
	for (size_t b = 0; b < plan.tile_ids.size(); ++b) {
		const int32_t tile = plan.tile_ids[b], tx = tile % plan.tiles_x, ty = tile / plan.tiles_x, first = plan.tile_start[b], last = plan.tile_start[b + 1];
		if (last - first > most) most = last - first;
		// (the lanes' registers: every lane of the tile keeps its samples across the chunks)
		std::vector<float> regs((size_t) SPLINE_TILE_W * SPLINE_WAVES * 3 * SPLINE_ROWS, 0.0f);
		auto P = [&](int32_t wave, int32_t lane) { return reinterpret_cast<float (*)[SPLINE_ROWS]>(&regs[((size_t) wave * SPLINE_TILE_W + (size_t) lane) * 3 * SPLINE_ROWS]); };
		for (int32_t wave = 0; wave < SPLINE_WAVES; ++wave) for (int32_t lane = 0; lane < SPLINE_TILE_W; ++lane) for (int32_t r = 0; r < SPLINE_ROWS; ++r) {
			const int32_t x = tx * SPLINE_TILE_W + lane, y = ty * SPLINE_TILE_H + wave * SPLINE_ROWS + r;
			for (int c = 0; c < 3; ++c) P(wave, lane)[c][r] = x < W && y < H ? planes[(size_t) c * plane + (size_t) y * pitch + (size_t) x] : 0.0f;
		}
		for (int32_t base = first; base < last; base += SPLINE_CHUNK) {
			const int32_t m = last - base < SPLINE_CHUNK ? last - base : (int32_t) SPLINE_CHUNK;
			for (int32_t i = 0; i < m; ++i) chunk[(size_t) i] = plan.segs[(size_t) plan.seg_idx[(size_t) (base + i)]];
			for (int32_t wave = 0; wave < SPLINE_WAVES; ++wave) for (int32_t lane = 0; lane < SPLINE_TILE_W; ++lane)
				spline_lane_walk(chunk.data(), m, tx * SPLINE_TILE_W + lane, ty * SPLINE_TILE_H + wave * SPLINE_ROWS, P(wave, lane));
		}
		for (int32_t wave = 0; wave < SPLINE_WAVES; ++wave) for (int32_t lane = 0; lane < SPLINE_TILE_W; ++lane) for (int32_t r = 0; r < SPLINE_ROWS; ++r) {
			const int32_t x = tx * SPLINE_TILE_W + lane, y = ty * SPLINE_TILE_H + wave * SPLINE_ROWS + r;
			if (x >= W || y >= H) continue;
			for (int c = 0; c < 3; ++c) planes[(size_t) c * plane + (size_t) y * pitch + (size_t) x] = P(wave, lane)[c][r];
		}
	}
	if (most_out) *most_out = most;
	return (int64_t) plan.tile_ids.size();
}

// the segments of one spline given as the stream holds it (start, `npts` double-delta pairs, coefficients [4][32]) on a W x H frame:
// returns their number (up to `cap` copied to `out`, and their multipliers, float64, to `mult_out` where given), -1 for what the parse
// refuses with "spln"
__attribute__((visibility("default"))) int64_t spline_sim_segments(int64_t x, int64_t y, const int64_t *dd, int32_t npts, const int32_t *coef128, int32_t quant_adjust, float ytox, float ytob,
		int32_t W, int32_t H, void *out, int64_t cap, double *mult_out) {
	SplineData sd;
	sd.quant_adjust = quant_adjust;
	QuantSpline q;
	q.x = x; q.y = y;
	if (npts > 0) q.dd.assign(dd, dd + 2 * (size_t) npts);
	memcpy(q.coef, coef128, sizeof q.coef);
	sd.splines.push_back(q);
	SplinePlan plan;
	std::vector<double> mults;
	if (!spline_segments(sd, ytox, ytob, W, H, &plan.segs, &mults) || !spline_bin(W, &plan)) return -1;
	if (mult_out) for (size_t i = 0; i < mults.size() && (int64_t) i < cap; ++i) mult_out[i] = mults[i];
	if (out && cap > 0 && !plan.segs.empty()) memcpy(out, plan.segs.data(), sizeof(SplineSeg) * (plan.segs.size() < (size_t) cap ? plan.segs.size() : (size_t) cap));
	return (int64_t) plan.segs.size();
}

} // extern "C"
