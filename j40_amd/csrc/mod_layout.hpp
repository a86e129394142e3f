// j40_amd/csrc/mod_layout.hpp -- where everything a DevModPlan points at lies in ONE block of memory: the tables uploaded from a
// HostModPlan, the sample planes and the per-section scratch. Pure host arithmetic, the single source of the layout: runtime.hip lays
// out a Modular frame (upload_modular) and the extra channels' sub-images of a VarDCT frame (validate_trailers, keep_alpha) with it,
// tests/hostsim lays out the same blocks in host memory with guard bytes behind every region, so that a region sized too small shows
// on the CPU. The codestream stays outside the block.
#pragma once
#include <algorithm>
#include <cstring>
#include "plan_build.hpp"
#include "device/plan.h"

namespace j40hip {
// what the kernels' launchers need to know about the plan's trees and code tables (device/plan.h)
inline ModLaunchInfo mod_launch_info(const HostModPlan &hp) {
	return ModLaunchInfo{hp.max_tree_nodes, hp.max_num_dist, hp.max_clusters, hp.max_table_bytes, hp.frame.max_width, hp.any_wp ? 1 : 0, hp.coop_width, hp.coop_sections + hp.split_sections == (int32_t) hp.sections.size(),
		hp.quad_sections, hp.quad_spec, hp.quad_width, hp.coop_sections, hp.quad_sections ? hp.specs[(size_t) hp.quad_spec].table_span : 0u, hp.split_sections, hp.split_width, hp.split_channels, hp.frame.sample_bytes == 4 ? 1 : 0};
}

struct ModPlanLayout {
	// a region starts on a 256-byte boundary and is followed by `guard` bytes nobody may write (the product passes 0); one of 0 bytes
	// takes no room. The uploaded regions come first, in this order, then the planes, the sub-planes and the scratch
	struct Region { const char *name; size_t offset, bytes; };
	enum { FRAME, POOL_U8, POOL_I32, POOL_U64, CLUSTERS, SPECS, TREE, SECTIONS, COOP_TREES, LOCAL_RCT, CHAN_RECTS, PLANE_REFS, SUB_REFS, UPLOADS };
	std::vector<Region> regions;   // [UPLOADS] uploaded, [num_planes] "plane", [num_subs] "sub_plane", then the five below
	enum { WP_SCRATCH, LZ_WINDOW, STATUS, RESIDUALS, SPLIT_STATE };   // after the sub-planes
	size_t num_planes = 0, num_subs = 0, guard = 0, upload_bytes = 0, total_bytes = 0; uint32_t lz_window_size = 0;
	size_t sample_bytes = 2;   // 4: a wide frame's plan (DevModFrame::sample_bytes): int32 planes, 64-bit weighted-predictor cells
	ModPlanLayout(const HostModPlan &hp, size_t guard_bytes) : num_planes(hp.plane_w.size()), num_subs(hp.sub_w.size()), guard(guard_bytes), lz_window_size(hp.lz_window_size), sample_bytes(hp.frame.sample_bytes == 4 ? 4 : 2) {
		const size_t nsec = hp.sections.size();
		auto place = [&](const char *name, size_t bytes) { regions.push_back({name, total_bytes, bytes}); if (bytes) total_bytes = (total_bytes + bytes + guard + 255) & ~(size_t) 255; };
		place("frame", sizeof(DevModFrame)); place("pool_u8", hp.pool_u8.size()); place("pool_i32", 4 * hp.pool_i32.size()); place("pool_u64", 8 * hp.pool_u64.size());
		place("clusters", sizeof(DevCluster) * hp.clusters.size()); place("specs", sizeof(DevCodeSpec) * hp.specs.size()); place("tree", sizeof(DevTreeNode) * hp.tree.size());
		place("sections", sizeof(DevModSection) * nsec); place("coop_trees", sizeof(DevCoopTree) * hp.coop_trees.size()); place("local_rct", 4 * hp.local_rct.size());
		place("chan_rects", sizeof(DevChanRect) * hp.chan_rects.size()); place("plane_refs", sizeof(DevPlaneRef) * num_planes); place("sub_refs", sizeof(DevSubPlane) * num_subs);
		upload_bytes = total_bytes;
		for (size_t c = 0; c < num_planes; ++c) place("plane", sample_bytes * ((size_t) std::max(hp.plane_w[c], 0) * (size_t) std::max(hp.plane_h[c], 0) + 1));
		for (size_t k = 0; k < num_subs; ++k) place("sub_plane", sample_bytes * ((size_t) hp.sub_w[k] * (size_t) hp.sub_h[k] + 1));
		place("wp_scratch", hp.frame.tree_uses_wp ? 2 * sample_bytes * (nsec * (size_t) (2 * hp.frame.max_width * 5) + 16) : 0); place("lz_window", 4 * nsec * (size_t) hp.lz_window_size);
		place("status", 4 * (nsec + 1));
		place("residuals", hp.split_sections ? 4 * (hp.split_samples + 64) : 0); place("split_state", hp.split_sections ? 4 * (3 * nsec + 4) : 0);
	}
	const Region &scratch(int which) const { return regions[UPLOADS + num_planes + num_subs + (size_t) which]; }
	int16_t *plane(uint8_t *base, size_t c) const { return (int16_t *) (base + regions[UPLOADS + c].offset); }
	int16_t *sub_plane(uint8_t *base, size_t k) const { return (int16_t *) (base + regions[UPLOADS + num_planes + k].offset); }
	// the same for either sample size (a wide plan's planes are int32_t)
	void *plane_any(uint8_t *base, size_t c) const { return base + regions[UPLOADS + c].offset; }
	void *sub_plane_any(uint8_t *base, size_t k) const { return base + regions[UPLOADS + num_planes + k].offset; }
	PlanePtr plane_ptr(uint8_t *base, size_t c) const { return PlanePtr{base + regions[UPLOADS + c].offset, (int32_t) sample_bytes}; }
	PlanePtr sub_plane_ptr(uint8_t *base, size_t k) const { return PlanePtr{base + regions[UPLOADS + num_planes + k].offset, (int32_t) sample_bytes}; }
	// the uploaded regions into `staging` (upload_bytes of it), the two plane tables with the addresses the planes have in a block at `base`
	void stage(const HostModPlan &hp, uint8_t *staging, uint8_t *base) const {
		const void *src[UPLOADS] = {&hp.frame, hp.pool_u8.data(), hp.pool_i32.data(), hp.pool_u64.data(), hp.clusters.data(), hp.specs.data(), hp.tree.data(),
			hp.sections.data(), hp.coop_trees.data(), hp.local_rct.data(), hp.chan_rects.data(), nullptr, nullptr};
		for (int r = 0; r < UPLOADS; ++r) if (src[r] && regions[(size_t) r].bytes) memcpy(staging + regions[(size_t) r].offset, src[r], regions[(size_t) r].bytes);
		for (size_t c = 0; c < num_planes; ++c) { const DevPlaneRef ref = {plane_any(base, c), hp.plane_w[c], hp.plane_h[c], hp.plane_meta[c], 0}; memcpy(staging + regions[PLANE_REFS].offset + sizeof ref * c, &ref, sizeof ref); }
		for (size_t k = 0; k < num_subs; ++k) { const DevSubPlane ref = {sub_plane_any(base, k), hp.sub_w[k], hp.sub_h[k], hp.sub_meta[k], 0}; memcpy(staging + regions[SUB_REFS].offset + sizeof ref * k, &ref, sizeof ref); }
	}
	// every pointer of the plan. The tables every plan has point into the block even when they are empty; what only some plans have
	// (coop_trees, local_rct, chan_rects, sub_planes and all scratch but `status`) is null where the plan has none
	DevModPlan bind(uint8_t *base, const uint8_t *codestream) const {
		DevModPlan plan; memset(&plan, 0, sizeof plan);
		auto at = [&](const Region &r, bool always) { return r.bytes || always ? base + r.offset : nullptr; };
		plan.frame = (const DevModFrame *) at(regions[FRAME], true); plan.codestream = codestream;
		plan.pool_u8 = at(regions[POOL_U8], true); plan.pool_i32 = (const int32_t *) at(regions[POOL_I32], true); plan.pool_u64 = (const uint64_t *) at(regions[POOL_U64], true);
		plan.clusters = (const DevCluster *) at(regions[CLUSTERS], true); plan.spec = (const DevCodeSpec *) at(regions[SPECS], true); plan.tree = (const DevTreeNode *) at(regions[TREE], true);
		plan.sections = (const DevModSection *) at(regions[SECTIONS], true); plan.planes = (const DevPlaneRef *) at(regions[PLANE_REFS], true); plan.status = (uint32_t *) at(scratch(STATUS), true);
		plan.coop_trees = (const DevCoopTree *) at(regions[COOP_TREES], false); plan.local_rct = (const int32_t *) at(regions[LOCAL_RCT], false); plan.chan_rects = (const DevChanRect *) at(regions[CHAN_RECTS], false);
		plan.sub_planes = (const DevSubPlane *) at(regions[SUB_REFS], false); plan.wp_scratch = (int32_t *) at(scratch(WP_SCRATCH), false);
		plan.lz_window = (int32_t *) at(scratch(LZ_WINDOW), false); plan.lz_window_size = lz_window_size;
		plan.residuals = (int32_t *) at(scratch(RESIDUALS), false); plan.split_state = (uint32_t *) at(scratch(SPLIT_STATE), false);
		return plan;
	}
};
} // namespace j40hip
