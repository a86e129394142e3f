// j40_amd/csrc/device/patch_dev.h -- patches (a sequence opened with J40HIP_SEQ_PATCHES): rectangles of a reference-only frame's XYB
// planes blended onto a frame's own XYB planes, ahead of its colour tail. The placement record, the per-sample blend, the walk of one
// lane over its pixels of a tile and the host's binning of the placement list into tiles. Compiled for the device by patch_kernels.hip
// and for the CPU by tests/hostsim/patch_sim.cpp: the same functions.
//
// Placements apply in dictionary order and may overlap (Replace then Add is not Add then Replace), so the order has to survive the
// parallelism: the frame is cut into tiles of PATCH_TILE_W x PATCH_TILE_H samples, the host lists for every tile the placements that
// touch it, in dictionary order (patch_bin: CSR -- tile_ids, offsets, index), and one workgroup per NON-EMPTY tile walks its list. A
// sample belongs to exactly one lane of exactly one workgroup, which applies every record to it in order: no atomics, nothing depends
// on which workgroup runs first, the planes are a pure function of the inputs.
//
// The tile is 64 x 32: a wavefront is 64 lanes, so a wavefront reads and writes one row of the tile as 64 consecutive floats -- 256
// coalesced bytes whatever the plane's pitch (a pitch is the frame's width, rarely a multiple of 4: no float4). The workgroup's four
// wavefronts take the rows 4 apart, eight rows a lane, whose 24 samples (three channels) stay in registers from the tile's first
// record to its last. The records come through LDS 64 at a time (2 KB); every lane reads the same record at once (a broadcast).
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
#include <vector>

namespace j40hip {

enum { PATCH_NONE = 0, PATCH_REPLACE = 1, PATCH_ADD = 2, PATCH_MUL = 3 };   // the colour channels' modes that are served (4..7 use alpha)
enum { PATCH_TILE_W = 64, PATCH_TILE_H = 32, PATCH_WAVES = 4, PATCH_ROWS = PATCH_TILE_H / PATCH_WAVES, PATCH_CHUNK = 64 };

// one placement, 32 bytes: the w x h samples at (sx, sy) of reference slot `slot` go onto the frame's samples at (x, y)
struct PatchRec { int32_t x, y, w, h, sx, sy, slot, mode_clamp; };   // mode_clamp: mode | clamp << 8
J40_HD int32_t patch_mode(const PatchRec &r) { return r.mode_clamp & 0xff; }
J40_HD int32_t patch_clamp(const PatchRec &r) { return r.mode_clamp >> 8 & 1; }

// the four reference slots, by value: three planes (X, Y, B) of w x h floats each, tightly packed, one behind the other; null: empty
struct PatchSlots { const float *base[4]; int32_t w[4], h[4]; };

// one float32 operation per sample and channel (-ffp-contract=off: nothing to contract, and nothing may be)
J40_HD float patch_blend(int32_t mode, int32_t clamp, float d, float s) {
	if (mode == PATCH_REPLACE) return s;
	if (mode == PATCH_ADD) return d + s;
	if (mode == PATCH_MUL) return d * (clamp ? (s < 0.0f ? 0.0f : s > 1.0f ? 1.0f : s) : s);
	return d;
}

// record `r` onto the frame's sample (x, y), three channels in d[]; false: the sample lies outside the placement
J40_HD bool patch_apply(const PatchRec &r, const PatchSlots &slots, int32_t x, int32_t y, float d[3]) {
	if (x < r.x || x >= r.x + r.w || y < r.y || y >= r.y + r.h) return false;
	const int32_t mode = patch_mode(r), clamp = patch_clamp(r);
	if (mode == PATCH_NONE) return false;
	const float *base = slots.base[r.slot & 3];
	const size_t pitch = (size_t) slots.w[r.slot & 3], plane = pitch * (size_t) slots.h[r.slot & 3];
	const float *s = base + (size_t) (r.sy + (y - r.y)) * pitch + (size_t) (r.sx + (x - r.x));
	d[0] = patch_blend(mode, clamp, d[0], s[0]);
	d[1] = patch_blend(mode, clamp, d[1], s[plane]);
	d[2] = patch_blend(mode, clamp, d[2], s[2 * plane]);
	return true;
}

// what the kernel and the host agree on beforehand (the index over a sequence's frames, the known-answer hook): 0, or why the
// placement list may not reach the kernel -- a slot that is empty ('ptno'), a rectangle outside its slot's planes or outside the frame,
// a mode that is not served ('ptch'). Nothing is checked again on the device.
J40_HD uint32_t patch_check(const PatchRec &r, const PatchSlots &slots, int32_t W, int32_t H) {
	const uint32_t ptch = 0x70746368u, ptno = 0x70746e6fu;
	if (r.slot < 0 || r.slot > 3 || patch_mode(r) > PATCH_MUL || r.mode_clamp < 0 || r.mode_clamp >> 9) return ptch;
	if (r.w < 1 || r.h < 1 || r.x < 0 || r.y < 0 || r.sx < 0 || r.sy < 0) return ptch;
	if ((int64_t) r.x + r.w > W || (int64_t) r.y + r.h > H) return ptch;
	if (!slots.base[r.slot]) return ptno;
	if ((int64_t) r.sx + r.w > slots.w[r.slot] || (int64_t) r.sy + r.h > slots.h[r.slot]) return ptch;
	return 0;
}

// the binned list as the kernel reads it: tile `tile_ids[b]` (row-major over the frame's tiles_x x tiles_y tiles) takes the records
// recs[index[offsets[b] .. offsets[b + 1])], in that order
struct DevPatches { const PatchRec *recs; const int32_t *tile_ids, *offsets, *index; int32_t num_tiles, tiles_x; };

// One lane's share of tile `b`: column `lane` (0..63) of the tile, rows `wave`, wave + 4, ... -- its samples loaded once, every record
// of the tile applied in order, the samples a record touched stored. `recs`: the tile's records one chunk at a time (the kernel stages
// them in LDS, the CPU build reads them in place); stage(at, n) makes recs[0..n) the records at..at + n of the tile's list.
template <typename Stage>
J40_HD void patch_tile_lane(float *planes, int32_t W, int32_t H, const DevPatches &p, const PatchSlots &slots, int32_t b, int32_t lane, int32_t wave, const PatchRec *recs, Stage stage) {
	const int32_t tile = p.tile_ids[b], tx = tile % p.tiles_x, ty = tile / p.tiles_x;
	const int32_t x = tx * PATCH_TILE_W + lane, y0 = ty * PATCH_TILE_H + wave;
	const size_t plane = (size_t) W * (size_t) H;
	const bool live = x < W;
	float d[PATCH_ROWS][3];
	uint32_t touched = 0;
#pragma unroll
	for (int i = 0; i < PATCH_ROWS; ++i) {
		const int32_t y = y0 + PATCH_WAVES * i;
		const bool in = live && y < H;
		const float *q = planes + (size_t) (in ? y : 0) * (size_t) W + (size_t) (in ? x : 0);
		d[i][0] = in ? q[0] : 0.0f; d[i][1] = in ? q[plane] : 0.0f; d[i][2] = in ? q[2 * plane] : 0.0f;
	}
	const int32_t end = p.offsets[b + 1];
	for (int32_t at = p.offsets[b]; at < end; at += PATCH_CHUNK) {
		const int32_t n = end - at < PATCH_CHUNK ? end - at : PATCH_CHUNK;
		stage(at, n);
		for (int32_t k = 0; k < n; ++k) {
			const PatchRec r = recs[k];
			if (!live || x < r.x || x >= r.x + r.w) continue;
#pragma unroll
			for (int i = 0; i < PATCH_ROWS; ++i) {
				const int32_t y = y0 + PATCH_WAVES * i;
				if (y < H && patch_apply(r, slots, x, y, d[i])) touched |= 1u << i;
			}
		}
	}
#pragma unroll
	for (int i = 0; i < PATCH_ROWS; ++i) if (touched >> i & 1) {
		float *q = planes + (size_t) (y0 + PATCH_WAVES * i) * (size_t) W + (size_t) x;
		q[0] = d[i][0]; q[plane] = d[i][1]; q[2 * plane] = d[i][2];
	}
}

// The host's binning of a flat placement list (dictionary order) over a W x H frame. Placements of mode None touch nothing and are
// left out; every other one is listed with each tile its rectangle meets. The records must have passed patch_check.
//
// What the binned list may hold: the dictionary bounds the placements, not the tiles they touch -- a few kilobytes of stream can
// name millions of whole-frame placements --, so the sum over the placements of the tiles each touches is bounded here:
// patch_bin_limit = 4096 + 64 entries per tile of the frame. That lets 64 layers cover the whole frame, or patches of 8 x 8 samples
// tile it without a gap (32 a tile, and those that straddle an edge), and keeps the index under 37 MB for the largest frame (2^28
// samples) and the work of a tile's workgroup at a few thousand records. The sum is taken in 64 bits, a product per placement,
// before anything is counted or allocated; a list beyond the limit is not binned (false: the caller answers 'ptch').
struct PatchBins {
	int32_t tiles_x = 0, tiles_y = 0;
	std::vector<int32_t> tile_ids, offsets, index;   // offsets: tile_ids.size() + 1 entries
};
inline int64_t patch_bin_limit(int32_t W, int32_t H) {
	return 4096 + 64 * (int64_t) ((W + PATCH_TILE_W - 1) / PATCH_TILE_W) * (int64_t) ((H + PATCH_TILE_H - 1) / PATCH_TILE_H);
}
inline bool patch_bin(const PatchRec *recs, size_t n, int32_t W, int32_t H, PatchBins *out) {
	out->tiles_x = (W + PATCH_TILE_W - 1) / PATCH_TILE_W; out->tiles_y = (H + PATCH_TILE_H - 1) / PATCH_TILE_H;
	out->tile_ids.clear(); out->offsets.clear(); out->index.clear();
	const int64_t limit = patch_bin_limit(W, H);
	int64_t entries = 0;
	for (size_t i = 0; i < n; ++i) {
		const PatchRec &r = recs[i];
		if (patch_mode(r) == PATCH_NONE) continue;
		entries += (int64_t) ((r.x + r.w - 1) / PATCH_TILE_W - r.x / PATCH_TILE_W + 1) * (int64_t) ((r.y + r.h - 1) / PATCH_TILE_H - r.y / PATCH_TILE_H + 1);
		if (entries > limit) return false;
	}
	const size_t tiles = (size_t) out->tiles_x * (size_t) out->tiles_y;
	std::vector<int32_t> count(tiles + 1, 0);   // (entries <= limit < 2^31: every count and offset fits)
	auto each_tile = [&](const PatchRec &r, auto fn) {
		if (patch_mode(r) == PATCH_NONE) return;
		for (int32_t ty = r.y / PATCH_TILE_H; ty <= (r.y + r.h - 1) / PATCH_TILE_H; ++ty)
			for (int32_t tx = r.x / PATCH_TILE_W; tx <= (r.x + r.w - 1) / PATCH_TILE_W; ++tx) fn((size_t) ty * (size_t) out->tiles_x + (size_t) tx);
	};
	for (size_t i = 0; i < n; ++i) each_tile(recs[i], [&](size_t t) { ++count[t]; });
	std::vector<int32_t> slot_of(tiles, -1), cursor;
	int32_t total = 0;
	for (size_t t = 0; t < tiles; ++t) if (count[t]) {
		slot_of[t] = (int32_t) out->tile_ids.size();
		out->tile_ids.push_back((int32_t) t); out->offsets.push_back(total); cursor.push_back(total);
		total += count[t];
	}
	out->offsets.push_back(total);
	out->index.assign((size_t) total, 0);
	for (size_t i = 0; i < n; ++i) each_tile(recs[i], [&](size_t t) { out->index[(size_t) cursor[(size_t) slot_of[t]]++] = (int32_t) i; });   // (i ascending: dictionary order inside each tile)
	return true;
}

// a frame's placements as records and their binning, made once when a sequence's index is built and shared with the frame's handle
struct PatchPlan { std::vector<PatchRec> recs; PatchBins bins; };

} // namespace j40hip
