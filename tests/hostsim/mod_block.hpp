// tests/hostsim/mod_block.hpp -- TEST INFRASTRUCTURE: a Modular plan in host memory, laid out by the product's ModPlanLayout
// (j40_amd/csrc/mod_layout.hpp) as runtime.hip lays it out on the device, in a block of exactly total_bytes from malloc with 64 guard
// bytes behind every region. Planes, sub-planes and status start at zero; the scratch regions and the guards hold 0x5a (device memory
// is not zeroed: what a decoder reads before it wrote must come from its own rule, not from here).
#pragma once
#include <cstdlib>
#include "../../j40_amd/csrc/mod_layout.hpp"

namespace j40hip {
// what the blocks of the last decode looked like (hostsim_guard_damage / hostsim_region_bytes and their alpha_sim twins)
inline size_t g_guard_damage = 0; inline std::vector<ModPlanLayout::Region> g_block_regions;
inline void mod_block_reset() { g_guard_damage = 0; g_block_regions.clear(); }
inline int64_t mod_block_region_bytes(const char *name) {
	int64_t n = 0;
	for (const ModPlanLayout::Region &r : g_block_regions) if (!strcmp(r.name, name)) n += (int64_t) r.bytes;
	return n;
}
struct ModBlock {
	enum { GUARD = 64, FILL = 0x5a };
	ModPlanLayout lay; uint8_t *base; DevModPlan plan;
	ModBlock(const HostModPlan &hp, const uint8_t *codestream) : lay(hp, GUARD), base((uint8_t *) malloc(lay.total_bytes)) {
		memset(base, FILL, lay.total_bytes);
		for (size_t r = ModPlanLayout::UPLOADS; r < ModPlanLayout::UPLOADS + lay.num_planes + lay.num_subs; ++r) memset(base + lay.regions[r].offset, 0, lay.regions[r].bytes);
		memset(base + lay.scratch(ModPlanLayout::STATUS).offset, 0, lay.scratch(ModPlanLayout::STATUS).bytes);
		lay.stage(hp, base, base); plan = lay.bind(base, codestream);
	}
	~ModBlock() {   // guard bytes that no longer read FILL
		for (const ModPlanLayout::Region &r : lay.regions) for (size_t i = 0; r.bytes && i < GUARD; ++i) g_guard_damage += base[r.offset + r.bytes + i] != FILL;
		g_block_regions.insert(g_block_regions.end(), lay.regions.begin(), lay.regions.end());
		free(base);
	}
};
} // namespace j40hip
