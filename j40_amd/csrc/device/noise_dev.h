// j40_amd/csrc/device/noise_dev.h -- photon noise (a frame parsed with J40HIP_PARSE_NOISE whose header has has_noise): a pseudo-random
// field, shaped by the frame's eight NoiseParameters, added to the frame's XYB planes behind the patches and ahead of the colour tail.
// The rule, the generator in its sequential form, the jumped form the kernel runs, the convolution and the per-pixel addition.
// Compiled for the device by noise_kernels.hip and for the CPU by tests/hostsim/noise_sim.cpp: the same functions.
//
// THE RULE. PARITY UNPINNED: it is the standard's and libjxl's as far as recalled without the text, and no decoder on hand pins it
// (the reference stops at has_noise, j40.h:6264) -- the tile, the seed counters, the mirror and the order of the additions below are
// this project's statement.
//   Random planes. Three raw planes R, G, C of the frame's size are filled group by group; a group is the frame's own group
//   rectangle (1 << group_size_shift samples a side) clipped to the frame, w x h samples at (x0, y0). Within a group the order is R
//   whole, then G, then C, row by row, from ONE generator that keeps running: eight lanes of xorshift128+,
//       s0[0] = SplitMix64(((u64) visible << 32) + nonvisible + 0x9E3779B97F4A7C15)
//       s1[0] = SplitMix64(((u64) x0 << 32) + y0 + 0x9E3779B97F4A7C15),  s0[i] = SplitMix64(s0[i - 1]), s1 likewise
//       SplitMix64(z): z = (z ^ z >> 30) * 0xBF58476D1CE4E5B9; z = (z ^ z >> 27) * 0x94D049BB133111EB; z ^ z >> 31
//       a step of lane i: a = s0[i]; b = s1[i]; out = a + b; s0[i] = b; a ^= a << 23; s1[i] = a ^ b ^ (a >> 18) ^ (b >> 5)
//   A step of all eight lanes yields 16 uint32 -- lane 0's low half, its high half, lane 1's, ... --, each made a float in [1, 2) by
//   bits >> 9 | 0x3F800000. A row takes ceil(w / 16) steps; the unused tail of its last step is dropped.
//   Seeds. visible, nonvisible: the frame's counters, both 0 for a stand-alone handle; a sequence's index counts them -- after a
//   shown frame visible + 1 and nonvisible = 0, after any other frame nonvisible + 1.
//   Convolution. Each raw plane 5 x 5: the centre times -3.84f plus 0.16f times the sum of the other 24. Coordinates outside the
//   frame mirror over the whole frame (-1 -> 0, W -> W - 1, repeated for a frame narrower than the reach). THE ORDER OF THE float32
//   ADDITIONS: the 24 neighbours row-major (dy = -2..2, dx = -2..2, the centre left out), the first one the sum's start, each
//   next one added to the sum so far; then (centre * -3.84f) + (0.16f * sum). Nothing is contracted (-ffp-contract=off).
//   Strength. strength(v): s = max(0, v * 6); i = floor(s), f = s - i; s >= 7: i = 6, f = 1; clamp(lut[i] + (lut[i + 1] - lut[i]) * f, 0, 1).
//   Adding. Per pixel, X and Y read before anything is written:
//       sr = strength((Y + X) * 0.5f), sg = strength((Y - X) * 0.5f); nr = 0.22f * convR, ng = 0.22f * convG, nc = 0.22f * convC
//       red = sr * (0.0078125f * nr + 0.9921875f * nc), green = sg * (0.0078125f * ng + 0.9921875f * nc), rg = red + green
//       X += base_corr_x * rg + (red - green);  Y += rg;  B += base_corr_b * rg          (a Modular frame: base_corr_x 0, base_corr_b 1)
//   A LUT of eight zeros changes nothing: nothing is launched, nothing allocated.
//
// THE JUMPED FORM. The generator is sequential by construction -- 3 * h * ceil(w / 16) dependent steps a group --, but its state
// update is linear over GF(2) (shifts and xors; only the OUTPUT, a + b, is not): a step is a 128 x 128 bit matrix M on the 128 state
// bits of a lane, and the state at the start of row r of the group's 3 * h rows (R's, then G's, then C's) is M^(r * steps_per_row)
// applied to the seed state. The 3 * h rows are cut into NOISE_BLOCKS = 32 blocks of RB = ceil(3 * h / 32) rows; thread t of the
// group's 256 owns generator lane t & 7 of block t >> 3, jumps to the block's first row by the matrices M^(RB * steps_per_row * 2^k) of
// the set bits k of its block number (NoiseJumpSet: five matrices, 10 KB; they commute, being powers of one matrix), then steps
// through its rows as the sequential form does. Eight neighbouring threads are the eight lanes of one step: their 8-byte stores make
// the step's 64 bytes, a whole 16-float run of one row. The raw planes' rows are padded to 16 floats (noise_pitch), so the last
// step's tail lands in the padding instead of being tested for. A frame has at most two steps-per-row values (its last column of
// groups may be narrower) and two group heights (its last row): four sets, built by repeated squaring on the host once per upload.
//
// THE ADDITION, k_noise_add: one workgroup per NOISE_TILE_W x NOISE_TILE_H = 64 x 32 tile, k_patch_blend's shape. It stages the 68 x 36
// halo tile of the three raw planes in LDS (29 376 bytes), the mirror resolved while loading; rows are 68 floats, the 64 lanes of a
// wavefront read 64 consecutive floats at every tap: no bank conflict. Wavefront w takes rows 8w .. 8w + 7 of the tile: a lane reads its
// 12 x 5 window of a plane once and makes eight sums of it, then reads and writes 64 consecutive floats of each plane per row.
#pragma once
#include <stdint.h>
#include <string.h>
#ifndef J40_HD
#ifdef __HIPCC__
#define J40_HD __host__ __device__ __forceinline__
#else
#define J40_HD static inline
#endif
#endif

namespace j40hip {

enum { NOISE_TILE_W = 64, NOISE_TILE_H = 32, NOISE_WAVES = 4, NOISE_ROWS = NOISE_TILE_H / NOISE_WAVES, NOISE_LDS_W = NOISE_TILE_W + 4, NOISE_LDS_H = NOISE_TILE_H + 4,
       NOISE_LDS_FLOATS = 3 * NOISE_LDS_W * NOISE_LDS_H, NOISE_LANES = 8, NOISE_BLOCKS = 32, NOISE_JUMP_BITS = 5, NOISE_FILL_THREADS = NOISE_LANES * NOISE_BLOCKS,
       NOISE_MAT_WORDS = 256, NOISE_SET_WORDS = NOISE_JUMP_BITS * NOISE_MAT_WORDS };

// what the addition takes, by value: the LUT and LfGlobal's base correlations
struct NoiseParams { float lut[8]; float ytox, ytob; };
// what the fill takes: the frame, its groups and the frame's seed counters
struct NoiseFillArgs { int32_t W, H, gdim, gcols, grows; uint32_t visible, nonvisible; };

J40_HD size_t noise_pitch(int32_t W) { return ((size_t) W + 15) & ~(size_t) 15; }   // floats a row of a raw plane
J40_HD bool noise_lut_is_zero(const float *lut) { for (int i = 0; i < 8; ++i) if (lut[i] != 0.0f) return false; return true; }

// ---- the generator ----
J40_HD uint64_t noise_splitmix64(uint64_t z) {
	z = (z ^ z >> 30) * 0xBF58476D1CE4E5B9ull;
	z = (z ^ z >> 27) * 0x94D049BB133111EBull;
	return z ^ z >> 31;
}
struct NoiseState { uint64_t s0, s1; };   // one generator lane
J40_HD uint64_t noise_step(NoiseState &s) {
	uint64_t a = s.s0;
	const uint64_t b = s.s1, out = a + b;
	s.s0 = b;
	a ^= a << 23;
	s.s1 = a ^ b ^ (a >> 18) ^ (b >> 5);
	return out;
}
J40_HD NoiseState noise_seed_lane(uint32_t visible, uint32_t nonvisible, uint32_t x0, uint32_t y0, int32_t lane) {
	NoiseState s;
	s.s0 = noise_splitmix64(((uint64_t) visible << 32) + nonvisible + 0x9E3779B97F4A7C15ull);
	s.s1 = noise_splitmix64(((uint64_t) x0 << 32) + y0 + 0x9E3779B97F4A7C15ull);
	for (int32_t i = 0; i < lane; ++i) { s.s0 = noise_splitmix64(s.s0); s.s1 = noise_splitmix64(s.s1); }
	return s;
}
J40_HD float noise_float(uint32_t bits) {
	const uint32_t u = bits >> 9 | 0x3F800000u;
	float f;
	memcpy(&f, &u, 4);
	return f;
}

// group `g` (row-major over the frame's groups) clipped to the frame
J40_HD void noise_group_rect(const NoiseFillArgs &a, int32_t g, int32_t *x0, int32_t *y0, int32_t *w, int32_t *h) {
	*x0 = g % a.gcols * a.gdim; *y0 = g / a.gcols * a.gdim;
	*w = a.W - *x0 < a.gdim ? a.W - *x0 : a.gdim; *h = a.H - *y0 < a.gdim ? a.H - *y0 : a.gdim;
}
J40_HD int32_t noise_steps_per_row(int32_t w) { return (w + 15) / 16; }
J40_HD int32_t noise_rows_per_block(int32_t h) { return (3 * h + NOISE_BLOCKS - 1) / NOISE_BLOCKS; }
// which of the frame's four jump sets the group takes: bit 0 its last column of groups, bit 1 its last row
J40_HD int32_t noise_set_of(const NoiseFillArgs &a, int32_t g) { return (g % a.gcols == a.gcols - 1 ? 1 : 0) | (g / a.gcols == a.grows - 1 ? 2 : 0); }

// The sequential form, the reference the jumped form is held against bit for bit (the CPU tests): group g's share of the raw planes
// (`pitch` floats a row, `plane` floats a plane), one chain of dependent steps
inline void noise_fill_group_sequential(float *raw, size_t pitch, size_t plane, const NoiseFillArgs &a, int32_t g) {
	int32_t x0, y0, w, h;
	noise_group_rect(a, g, &x0, &y0, &w, &h);
	NoiseState st[NOISE_LANES];
	for (int32_t i = 0; i < NOISE_LANES; ++i) st[i] = noise_seed_lane(a.visible, a.nonvisible, (uint32_t) x0, (uint32_t) y0, i);
	const int32_t steps = noise_steps_per_row(w);
	for (int32_t c = 0; c < 3; ++c) for (int32_t y = 0; y < h; ++y) {
		float *row = raw + (size_t) c * plane + (size_t) (y0 + y) * pitch + (size_t) x0;
		for (int32_t s = 0; s < steps; ++s) for (int32_t i = 0; i < NOISE_LANES; ++i) {
			const uint64_t out = noise_step(st[i]);
			const int32_t x = 16 * s + 2 * i;
			if (x < w) row[x] = noise_float((uint32_t) out);
			if (x + 1 < w) row[x + 1] = noise_float((uint32_t) (out >> 32));
		}
	}
}

// ---- the jump ----
// A 128 x 128 bit matrix as its columns: words 2j, 2j + 1 are the image (s0, s1) of the state whose only set bit is j (bits 0..63: s0,
// 64..127: s1). M * v is the xor of the columns of v's set bits.
J40_HD NoiseState noise_mat_apply(const uint64_t *m, NoiseState v) {
	uint64_t r0 = 0, r1 = 0;
	for (int32_t j = 0; j < 64; ++j) {
		const uint64_t ma = 0 - (v.s0 >> j & 1), mb = 0 - (v.s1 >> j & 1);
		r0 ^= (m[2 * j] & ma) ^ (m[2 * (64 + j)] & mb);
		r1 ^= (m[2 * j + 1] & ma) ^ (m[2 * (64 + j) + 1] & mb);
	}
	NoiseState r = {r0, r1};
	return r;
}
// (host) one step as a matrix; the product a * b; m^n by repeated squaring
inline void noise_mat_step(uint64_t *m) {
	for (int32_t j = 0; j < 128; ++j) {
		NoiseState e = {j < 64 ? (uint64_t) 1 << j : 0, j < 64 ? 0 : (uint64_t) 1 << (j - 64)};
		(void) noise_step(e);
		m[2 * j] = e.s0; m[2 * j + 1] = e.s1;
	}
}
inline void noise_mat_mul(const uint64_t *a, const uint64_t *b, uint64_t *out) {   // (out is neither a nor b)
	for (int32_t j = 0; j < 128; ++j) {
		const NoiseState col = {b[2 * j], b[2 * j + 1]}, r = noise_mat_apply(a, col);
		out[2 * j] = r.s0; out[2 * j + 1] = r.s1;
	}
}
inline void noise_mat_pow(const uint64_t *m, uint64_t n, uint64_t *out) {
	uint64_t sq[NOISE_MAT_WORDS], tmp[NOISE_MAT_WORDS];
	memcpy(sq, m, sizeof sq);
	for (int32_t j = 0; j < 128; ++j) { out[2 * j] = j < 64 ? (uint64_t) 1 << j : 0; out[2 * j + 1] = j < 64 ? 0 : (uint64_t) 1 << (j - 64); }   // the identity
	for (; n; n >>= 1) {
		if (n & 1) { noise_mat_mul(sq, out, tmp); memcpy(out, tmp, sizeof tmp); }
		if (n > 1) { noise_mat_mul(sq, sq, tmp); memcpy(sq, tmp, sizeof tmp); }
	}
}
// the five matrices of a group w samples wide and h high: set[k] = M^(rows_per_block * steps_per_row * 2^k)
inline void noise_jump_set(int32_t w, int32_t h, uint64_t *set) {
	uint64_t step[NOISE_MAT_WORDS];
	noise_mat_step(step);
	noise_mat_pow(step, (uint64_t) noise_rows_per_block(h) * (uint64_t) noise_steps_per_row(w), set);
	for (int32_t k = 1; k < NOISE_JUMP_BITS; ++k) noise_mat_mul(set + (size_t) (k - 1) * NOISE_MAT_WORDS, set + (size_t) (k - 1) * NOISE_MAT_WORDS, set + (size_t) k * NOISE_MAT_WORDS);
}
// the frame's four sets (noise_set_of): full or last-column width by full or last-row height; 4 * NOISE_SET_WORDS words
inline void noise_frame_jumps(const NoiseFillArgs &a, uint64_t *sets) {
	const int32_t wl = a.W - (a.gcols - 1) * a.gdim, hl = a.H - (a.grows - 1) * a.gdim;
	const int32_t wf = a.gcols > 1 ? a.gdim : wl, hf = a.grows > 1 ? a.gdim : hl;
	for (int32_t k = 0; k < 4; ++k) noise_jump_set(k & 1 ? wl : wf, k & 2 ? hl : hf, sets + (size_t) k * NOISE_SET_WORDS);
}

// Thread t (0 .. NOISE_FILL_THREADS - 1) of group g: generator lane t & 7 of row block t >> 3. The raw planes' rows are padded
// (noise_pitch) and x0 is a multiple of 16, so every step's run lies inside its row and every store is 8-byte aligned.
J40_HD void noise_fill_lane(float *raw, size_t pitch, size_t plane, const NoiseFillArgs &a, const uint64_t *sets, int32_t g, int32_t t) {
	int32_t x0, y0, w, h;
	noise_group_rect(a, g, &x0, &y0, &w, &h);
	const int32_t steps = noise_steps_per_row(w), rows = 3 * h, rb = noise_rows_per_block(h);
	const int32_t lane = t & (NOISE_LANES - 1), blk = t / NOISE_LANES;
	const int32_t r0 = blk * rb, r1 = r0 + rb < rows ? r0 + rb : rows;
	if (r0 >= rows) return;
	NoiseState st = noise_seed_lane(a.visible, a.nonvisible, (uint32_t) x0, (uint32_t) y0, lane);
	const uint64_t *set = sets + (size_t) noise_set_of(a, g) * NOISE_SET_WORDS;
	for (int32_t k = 0; k < NOISE_JUMP_BITS; ++k) if (blk >> k & 1) st = noise_mat_apply(set + (size_t) k * NOISE_MAT_WORDS, st);
	for (int32_t r = r0; r < r1; ++r) {
		const int32_t c = r / h, y = r - c * h;
		float *row = raw + (size_t) c * plane + (size_t) (y0 + y) * pitch + (size_t) (x0 + 2 * lane);
		for (int32_t s = 0; s < steps; ++s) {
			const uint64_t out = noise_step(st);
#ifdef __HIP_DEVICE_COMPILE__
			*(float2 *) (row + 16 * s) = make_float2(noise_float((uint32_t) out), noise_float((uint32_t) (out >> 32)));
#else
			row[16 * s] = noise_float((uint32_t) out); row[16 * s + 1] = noise_float((uint32_t) (out >> 32));
#endif
		}
	}
}

// ---- the convolution and the addition ----
J40_HD int32_t noise_mirror(int32_t x, int32_t n) {
	while (x < 0 || x >= n) x = x < 0 ? -x - 1 : 2 * n - 1 - x;
	return x;
}
J40_HD float noise_strength(const float *lut, float v) {
	float s = v * 6.0f;
	if (!(s > 0.0f)) s = 0.0f;
	int32_t i = 6;
	float f = 1.0f;
	if (s < 7.0f) { i = (int32_t) s; f = s - (float) i; }
	const float r = lut[i] + (lut[i + 1] - lut[i]) * f;
	return r < 0.0f ? 0.0f : r > 1.0f ? 1.0f : r;
}
// d: the pixel's X, Y, B, changed in place; conv: the three convolved planes' values there (R, G, C)
J40_HD void noise_add_pixel(const NoiseParams &p, float d[3], const float conv[3]) {
	const float X = d[0], Y = d[1];
	const float sr = noise_strength(p.lut, (Y + X) * 0.5f), sg = noise_strength(p.lut, (Y - X) * 0.5f);
	const float nr = 0.22f * conv[0], ng = 0.22f * conv[1], nc = 0.22f * conv[2];
	const float red = sr * (0.0078125f * nr + 0.9921875f * nc), green = sg * (0.0078125f * ng + 0.9921875f * nc);
	const float rg = red + green;
	d[0] = X + (p.ytox * rg + (red - green));
	d[1] = Y + rg;
	d[2] = d[2] + p.ytob * rg;
}

// thread t of the tile's 256 stages its share of the three planes' halo tile (tile[c][ly][lx], NOISE_LDS_W floats a row): sample
// (tx * 64 - 2 + lx, ty * 32 - 2 + ly) of raw plane c, mirrored into the frame
J40_HD void noise_tile_stage(float *tile, const float *raw, size_t pitch, size_t plane, int32_t W, int32_t H, int32_t tx, int32_t ty, int32_t t) {
	for (int32_t i = t; i < NOISE_LDS_FLOATS; i += NOISE_TILE_W * NOISE_WAVES) {
		const int32_t c = i / (NOISE_LDS_W * NOISE_LDS_H), rem = i - c * (NOISE_LDS_W * NOISE_LDS_H), ly = rem / NOISE_LDS_W, lx = rem - ly * NOISE_LDS_W;
		const int32_t gx = noise_mirror(tx * NOISE_TILE_W - 2 + lx, W), gy = noise_mirror(ty * NOISE_TILE_H - 2 + ly, H);
		tile[i] = raw[(size_t) c * plane + (size_t) gy * pitch + (size_t) gx];
	}
}
// column `lane` of the tile, rows 8 * wave .. 8 * wave + 7, from the staged tile onto the frame's planes (`ppitch` floats a row,
// `pplane` floats a plane)
J40_HD void noise_tile_lane(float *planes, size_t ppitch, size_t pplane, int32_t W, int32_t H, const float *tile, const NoiseParams &p, int32_t tx, int32_t ty, int32_t lane, int32_t wave) {
	float conv[NOISE_ROWS][3];
#pragma unroll
	for (int32_t c = 0; c < 3; ++c) {
		float v[NOISE_ROWS + 4][5];
#pragma unroll
		for (int32_t i = 0; i < NOISE_ROWS + 4; ++i)
#pragma unroll
			for (int32_t j = 0; j < 5; ++j) v[i][j] = tile[(c * NOISE_LDS_H + NOISE_ROWS * wave + i) * NOISE_LDS_W + lane + j];
#pragma unroll
		for (int32_t r = 0; r < NOISE_ROWS; ++r) {
			float sum = v[r][0];
#pragma unroll
			for (int32_t k = 1; k < 25; ++k) if (k != 12) sum = sum + v[r + k / 5][k % 5];
			conv[r][c] = v[r + 2][2] * -3.84f + 0.16f * sum;
		}
	}
	const int32_t x = tx * NOISE_TILE_W + lane;
	if (x >= W) return;
#pragma unroll
	for (int32_t r = 0; r < NOISE_ROWS; ++r) {
		const int32_t y = ty * NOISE_TILE_H + NOISE_ROWS * wave + r;
		if (y >= H) break;
		float *q = planes + (size_t) y * ppitch + (size_t) x;
		float d[3] = {q[0], q[pplane], q[2 * pplane]};
		noise_add_pixel(p, d, conv[r]);
		q[0] = d[0]; q[pplane] = d[1]; q[2 * pplane] = d[2];
	}
}

} // namespace j40hip
