// j40_amd/csrc/device/upsample_dev.h -- upsampling (a frame parsed with J40HIP_PARSE_UPSAMPLING whose header has upsampling = K > 1): the
// frame is coded at ceil(shown / K) samples an axis, and its XYB planes, behind the restoration filters, are stretched K times by a
// 5 x 5 stencil with K x K outputs per coded sample before anything else sees them. The rule, the expansion of a stream's weight table, the
// per-sample form and the tile functions k_upsample<K> is made of. Compiled for the device by upsample_kernels.hip and for the CPU by
// capi_host.cpp (j40hip_kat_host_upsample) and tests/hostsim/upsample_main.cpp: the same functions.
//
// THE RULE. PARITY UNPINNED: it is the standard's and libjxl's as far as recalled without the text, and no decoder on hand pins it (the
// reference refuses upsampling != 1, j40.h:3297-3306, 5244-5249, and custom weights, j40.h:3638).
//   Sizes. The width and height the frame header yields (the image's, or the crop's) are the SHOWN size; with K = upsampling > 1 the CODED
//   size is ceil(shown / K) per axis, and everything up to and including the restoration filters works on it. The upsampled picture is
//   K * coded on each axis, cut at the top-left to the shown size.
//   Weights. Let N = K / 2. A table of 15 (K = 2), 55 (K = 4) or 210 (K = 8) numbers w is the upper triangle of a symmetric 5N x 5N
//   matrix M, packed row by row: M[i][j] = w[5N * y - y * (y - 1) / 2 + x - y] with y = min(i, j), x = max(i, j).
//   kernel[j / 5][i / 5][j % 5][i % 5] = M[i][j]: N x N kernels of 5 x 5 taps, indexed [iy][ix][ky][kx].
//   Output (K * x + ox, K * y + oy) uses kernel[oy < N ? oy : K - 1 - oy][ox < N ? ox : K - 1 - ox]; its tap (ky, kx) is applied to the
//   coded sample (x + kx' - 2, y + ky' - 2) with ky' = oy < N ? ky : 4 - ky and kx' = ox < N ? kx : 4 - kx.
//   Coordinates outside the coded plane mirror: x < 0 -> -x - 1, x >= w -> 2w - 1 - x, repeated until in range (planes narrower than 3
//   exist).
//   Arithmetic. float32, one rounding per operation, nothing contracted (-ffp-contract=off): acc = 0; for ky' = 0..4, for kx' = 0..4, in
//   that order, acc = acc + weight * sample; the result is min(max(acc, lo), hi) with lo and hi the smallest and the largest of the same
//   25 samples. Each of the three planes on its own.
//   Place. Behind the restoration filters, ahead of patches, noise and the colour tail.
//
// THE EXPANDED TABLE. upsample_expand turns w into E[K][K][25], E[oy][ox][5 * ky' + kx'] = the weight the output phase (ox, oy) gives the
// coded sample at (kx' - 2, ky' - 2): the mirrored kernels written out, the taps in source order, so that the sum's order is the table's.
// Built on the host once per upload (j40hip_kat_upsampling_kernel shows it).
//
// THE TILE. The kernel writes 3 * up_w * up_h floats and reads a K * K-th of that: its stores are what it waits for, and after them the
// 25 weights every output reads. One workgroup of 256 threads takes a tile of 32 x 8 coded samples of ONE plane: its 36 x 12 halo,
// mirrored while it is staged, sits in LDS (432 floats) beside the expanded table (at most 1600 floats). A work item is one output
// column X of one coded row: 32 * K columns x 8 rows a tile, item i = t + 256 * j at column i % (32 * K) of row i / (32 * K), so a
// wavefront's 64 lanes are 64 neighbouring output columns of one coded row. The item reads its 5 x 5 window once -- lanes of one
// coded sample read one address (a broadcast), neighbouring samples neighbouring banks: no conflict at a row pitch of 36 --, finds lo
// and hi once, and makes the K outputs of its column, oy = 0..K - 1, each from the 25 weights of phase (ox, oy): the lanes' K phases ox
// lie 25 floats apart, an odd stride, so K <= 8 of them never share a bank. Every store of a wavefront is 64 consecutive floats of one
// output row (256 B). Reading the window once per K outputs halves the LDS reads against a thread per output. 32 coded columns make
// K = 2's output row exactly one wavefront wide; 8 rows keep the halo's overhead at (36 * 12) / (32 * 8) = 1.7 reads a sample, a
// K * K-th of the stores.
#pragma once
#include <stdint.h>
#include <stddef.h>
#ifndef J40_HD
#ifdef __HIPCC__
#define J40_HD __host__ __device__ __forceinline__
#else
#define J40_HD static inline
#endif
#endif

namespace j40hip {

enum { UP_TILE_W = 32, UP_TILE_H = 8, UP_THREADS = 256, UP_LDS_W = UP_TILE_W + 4, UP_LDS_H = UP_TILE_H + 4, UP_LDS_FLOATS = UP_LDS_W * UP_LDS_H, UP_MAX_TABLE = 8 * 8 * 25 };

J40_HD bool upsample_factor_valid(int32_t k) { return k == 2 || k == 4 || k == 8; }
J40_HD int32_t upsample_weight_count(int32_t k) { return k == 2 ? 15 : k == 4 ? 55 : k == 8 ? 210 : 0; }   // the upper triangle of a 5N x 5N matrix
J40_HD int32_t upsample_coded_size(int32_t shown, int32_t k) { return (int32_t) (((int64_t) shown + k - 1) / k); }

J40_HD int32_t upsample_mirror(int32_t x, int32_t w) {
	while (x < 0 || x >= w) x = x < 0 ? -x - 1 : 2 * w - 1 - x;
	return x;
}

// M[i][j] of the rule from the packed table
J40_HD float upsample_matrix(const float *w, int32_t n5, int32_t i, int32_t j) {
	const int32_t y = i < j ? i : j, x = i < j ? j : i;
	return w[n5 * y - y * (y - 1) / 2 + x - y];
}

// E[K][K][25] from the 15 / 55 / 210 weights (the header comment)
J40_HD void upsample_expand(int32_t k, const float *w, float *e) {
	const int32_t n = k / 2, n5 = 5 * n;
	for (int32_t oy = 0; oy < k; ++oy) for (int32_t ox = 0; ox < k; ++ox) {
		const int32_t iy = oy < n ? oy : k - 1 - oy, ix = ox < n ? ox : k - 1 - ox;
		for (int32_t sy = 0; sy < 5; ++sy) for (int32_t sx = 0; sx < 5; ++sx) {
			const int32_t ky = oy < n ? sy : 4 - sy, kx = ox < n ? sx : 4 - sx;
			// kernel[iy][ix][ky][kx] = M[5 * ix + kx][5 * iy + ky]
			e[(oy * k + ox) * 25 + sy * 5 + sx] = upsample_matrix(w, n5, 5 * ix + kx, 5 * iy + ky);
		}
	}
}

// the sum and the clamp over a 5 x 5 window (`win`: `pitch` floats a row) with the 25 weights of one phase; lo, hi: the window's range
J40_HD float upsample_dot(const float *win, int32_t pitch, const float *wt, float lo, float hi) {
	float acc = 0.0f;
#pragma unroll
	for (int32_t sy = 0; sy < 5; ++sy)
#pragma unroll
		for (int32_t sx = 0; sx < 5; ++sx) acc = acc + wt[sy * 5 + sx] * win[sy * pitch + sx];
	acc = acc < lo ? lo : acc;
	return acc > hi ? hi : acc;
}

// The rule for one output sample (X, Y) of one plane, straight from the coded plane `src` (w x h floats, w a row) and the expanded table
template <int K> J40_HD float upsample_sample(const float *src, int32_t w, int32_t h, const float *e, int32_t X, int32_t Y) {
	const int32_t x = X / K, ox = X % K, y = Y / K, oy = Y % K;
	float win[25];
	float lo = 0.0f, hi = 0.0f;
	for (int32_t sy = 0; sy < 5; ++sy) for (int32_t sx = 0; sx < 5; ++sx) {
		const float v = src[(size_t) upsample_mirror(y + sy - 2, h) * (size_t) w + (size_t) upsample_mirror(x + sx - 2, w)];
		win[sy * 5 + sx] = v;
		if (sy == 0 && sx == 0) lo = hi = v;
		lo = v < lo ? v : lo; hi = v > hi ? v : hi;
	}
	return upsample_dot(win, 5, e + (oy * K + ox) * 25, lo, hi);
}

// ---- the tile (the header comment): what thread t of the workgroup of tile (tx, ty) does ----
// the halo of the tile, mirrored, into `tile` (UP_LDS_FLOATS floats)
J40_HD void upsample_tile_stage(float *tile, const float *src, int32_t w, int32_t h, int32_t tx, int32_t ty, int32_t t) {
	for (int32_t i = t; i < UP_LDS_FLOATS; i += UP_THREADS) {
		const int32_t ly = i / UP_LDS_W, lx = i % UP_LDS_W;
		const int32_t sx = upsample_mirror(tx * UP_TILE_W + lx - 2, w), sy = upsample_mirror(ty * UP_TILE_H + ly - 2, h);
		tile[i] = src[(size_t) sy * (size_t) w + (size_t) sx];
	}
}

// the thread's output columns of the tile into the plane `out` (up_w x up_h floats, `opitch` a row), cut to that size; e: the expanded table
template <int K> J40_HD void upsample_tile_lane(float *out, size_t opitch, int32_t up_w, int32_t up_h, int32_t w, int32_t h, const float *tile, const float *e, int32_t tx, int32_t ty, int32_t t) {
	constexpr int32_t COLS = UP_TILE_W * K, ITEMS = COLS * UP_TILE_H;
#pragma unroll 1
	for (int32_t i = t; i < ITEMS; i += UP_THREADS) {
		const int32_t col = i % COLS, ly = i / COLS, lx = col / K, ox = col % K;
		const int32_t x = tx * UP_TILE_W + lx, y = ty * UP_TILE_H + ly, X = x * K + ox;
		if (x >= w || y >= h || X >= up_w) continue;
		const float *win = tile + ly * UP_LDS_W + lx;   // (the window's corner: coded (x - 2, y - 2))
		float v[25];
		float lo = win[0], hi = win[0];
#pragma unroll
		for (int32_t sy = 0; sy < 5; ++sy)
#pragma unroll
			for (int32_t sx = 0; sx < 5; ++sx) {
				const float s = win[sy * UP_LDS_W + sx];
				v[sy * 5 + sx] = s;
				lo = s < lo ? s : lo; hi = s > hi ? s : hi;
			}
#pragma unroll
		for (int32_t oy = 0; oy < K; ++oy) {
			const int32_t Y = y * K + oy;
			if (Y >= up_h) break;
			out[(size_t) Y * opitch + (size_t) X] = upsample_dot(v, 5, e + (oy * K + ox) * 25, lo, hi);
		}
	}
}

} // namespace j40hip
