// tests/hostsim/patch_sim.cpp -- patches on the CPU (tests/test_patches.py): device/patch_dev.h's lane function and tile binning, the same
// functions k_patch_blend is made of, over planes in host memory. A workgroup's lanes run one after the other here; each owns its samples,
// so the order between them cannot matter -- which is the kernel's claim too.
#include <stdint.h>
#include <string.h>
#include <vector>
#include "../../j40_amd/csrc/device/patch_dev.h"

using namespace j40hip;

namespace {
std::vector<PatchRec> records(const int32_t *placements, int32_t count) {
	std::vector<PatchRec> recs((size_t) count);
	for (int32_t i = 0; i < count; ++i) {
		const int32_t *v = placements + (size_t) i * 9;   // x, y, w, h, x0, y0, slot, mode, clamp
		recs[(size_t) i] = PatchRec{v[0], v[1], v[2], v[3], v[4], v[5], v[6], v[7] | (v[8] ? 1 : 0) << 8};
	}
	return recs;
}
}

extern "C" {

// the placement list binned over a W x H frame: returns the number of non-empty tiles (-1: the list is over patch_bin_limit); tile_ids
// (that many), offsets (one more) and index (offsets' last entry) are filled as far as their capacities go; tiles_xy: the frame's tiles per row and per column
__attribute__((visibility("default"))) int32_t patch_sim_bin(const int32_t *placements, int32_t count, int32_t W, int32_t H, int32_t *tiles_xy, int32_t *tile_ids, int32_t tile_cap, int32_t *offsets, int32_t *index, int32_t index_cap) {
	const std::vector<PatchRec> recs = records(placements, count);
	PatchBins bins;
	if (!patch_bin(recs.data(), recs.size(), W, H, &bins)) return -1;   // (more tile entries than patch_bin_limit)
	tiles_xy[0] = bins.tiles_x; tiles_xy[1] = bins.tiles_y;
	const int32_t n = (int32_t) bins.tile_ids.size();
	for (int32_t i = 0; i < n && i < tile_cap; ++i) { tile_ids[i] = bins.tile_ids[(size_t) i]; offsets[i] = bins.offsets[(size_t) i]; }
	if (n <= tile_cap) offsets[n] = bins.offsets[(size_t) n];
	for (size_t i = 0; i < bins.index.size() && (int32_t) i < index_cap; ++i) index[i] = bins.index[i];
	return n;
}

// the whole of k_patch_blend: check, bin, then every lane of every non-empty tile's workgroup. planes: [3][H][W] floats, in place;
// slot[k]: [3][slot_h[k]][slot_w[k]] floats or null. Returns 0 or the code the list is refused with
__attribute__((visibility("default"))) uint32_t patch_sim_apply(float *planes, int32_t W, int32_t H, const float *const slot[4], const int32_t slot_w[4], const int32_t slot_h[4], const int32_t *placements, int32_t count) {
	const std::vector<PatchRec> recs = records(placements, count);
	PatchSlots slots;
	for (int k = 0; k < 4; ++k) { slots.base[k] = slot[k]; slots.w[k] = slot_w[k]; slots.h[k] = slot_h[k]; }
	for (const PatchRec &r : recs) if (uint32_t e = patch_check(r, slots, W, H)) return e;
	PatchBins bins;
	if (!patch_bin(recs.data(), recs.size(), W, H, &bins)) return 0x70746368u;
	const DevPatches p = {recs.data(), bins.tile_ids.data(), bins.offsets.data(), bins.index.data(), (int32_t) bins.tile_ids.size(), bins.tiles_x};
	PatchRec chunk[PATCH_CHUNK];
	for (int32_t b = 0; b < p.num_tiles; ++b) for (int32_t wave = 0; wave < PATCH_WAVES; ++wave) for (int32_t lane = 0; lane < 64; ++lane)
		patch_tile_lane(planes, W, H, p, slots, b, lane, wave, chunk, [&](int32_t at, int32_t n) { for (int32_t t = 0; t < n; ++t) chunk[t] = p.recs[p.index[at + t]]; });
	return 0;
}

}
