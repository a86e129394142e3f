// tests/hostsim/alpha_sim.cpp -- TEST INFRASTRUCTURE: the kept alpha channel of a VarDCT frame on the CPU (build/libhostsim_alpha.so).
// The product's host parser and plan builders, the entropy decoder for the bits where each section's coefficients end, the keep-mode
// trailer plan (build_trailer_plan, plan_build.cpp) decoded by the Modular device functions into frame-wide planes, and the merge
// functions of device/alpha_dev.h row by row: the code k_alpha_merge runs, without a device.
#include <cstdint>
#include <cstring>
#include <cmath>
#include <vector>
#include <algorithm>
#include "../../j40_amd/csrc/plan_build.hpp"
#include "../../j40_amd/csrc/tables.hpp"
#include "../../j40_amd/csrc/device/hf_dev.h"
#include "../../j40_amd/csrc/device/modular_dev.h"
#include "../../j40_amd/csrc/device/alpha_dev.h"
#include "../../include/j40hip.h"
#include "mod_block.hpp"

using namespace j40hip;

#define ALPHA_SIM_API extern "C" __attribute__((visibility("default")))

// the rule alone: sample p of an alpha channel of `bpp` bits as the A of format `fmt` (J40HIP_U8X4 / J40HIP_U16X4)
ALPHA_SIM_API uint32_t alpha_sim_scale(int32_t p, int32_t bpp, int32_t fmt) {
	const bool out16 = fmt == J40HIP_U16X4;
	const AlphaScale s = alpha_scale_make(bpp, out16);
	return out16 ? alpha_value<true>(p, s) : alpha_value<false>(p, s);
}

// the Modular block of the last alpha_sim_decode (mod_block.hpp): guard bytes that no longer read 0x5a; the bytes of the regions called `name`
ALPHA_SIM_API int64_t alpha_sim_guard_damage(void) { return (int64_t) g_guard_damage; }
ALPHA_SIM_API int64_t alpha_sim_region_bytes(const char *name) { return mod_block_region_bytes(name); }

// Merges the stream's alpha channel over the caller's pixels (width x height of format `fmt`, `stride` bytes a row; R, G, B are
// left as they are). Returns 0, the stream's error code, "Ual?" / "TODO" as j40hip_frame_set_alpha(f, 1) would.
ALPHA_SIM_API uint32_t alpha_sim_decode(const uint8_t *buf, size_t size, uint8_t *rgba, size_t stride, int32_t fmt) {
	Frame fr;
	const uint8_t *cs; size_t cs_size; std::vector<uint8_t> storage;
	HostPlan hp;
	mod_block_reset();
	try {
		extract_codestream(buf, size, &cs, &cs_size, &storage);
		parse_frame(cs, cs_size, &fr, 1);
	} catch (const DecodeError &e) { return e.code; }
	int32_t index = -1;
	if (uint32_t e = alpha_keep_scope(fr, &index)) return e;
	if (uint32_t e = build_vardct_plan(fr, cs, cs_size, &hp)) return e;
	// the entropy decode, for every section's status and the bit where its coefficients end
	std::vector<float> coeff_store(3 * hp.coeff_floats, 0.0f);
	std::vector<int8_t> nonzeros((size_t) hp.frame.num_groups * 32 * 32 * 3);
	std::vector<uint32_t> status(hp.sections.size(), 0), end_bits(hp.sections.size(), 0);
	std::vector<int32_t> window(hp.lz_window_size ? (size_t) hp.frame.num_groups * hp.lz_window_size : 0);
	DevPlan plan;
	memset(&plan, 0, sizeof plan);
	plan.frame = &hp.frame; plan.codestream = hp.codestream.data();
	plan.pool_u8 = hp.pool_u8.data(); plan.pool_u16 = hp.pool_u16.data(); plan.pool_i32 = hp.pool_i32.data(); plan.pool_u64 = hp.pool_u64.data(); plan.pool_f32 = hp.pool_f32.data();
	plan.clusters = hp.clusters.data(); plan.coeff_specs = hp.coeff_specs.data(); plan.lf_groups = hp.lf_groups.data(); plan.sections = hp.sections.data();
	plan.block_ctx_map_off = hp.block_ctx_map_off;
	plan.group_blocks = hp.group_blocks.data(); plan.group_block_start = hp.group_block_start.data();
	plan.blocks = hp.blocks.data(); plan.lfindices = hp.lfindices.data();
	for (int c = 0; c < 3; ++c) { plan.llf[c] = hp.llf[c].data(); plan.coeffs[c] = coeff_store.data() + (size_t) c * hp.coeff_floats; }
	plan.coeff_stride = (uint32_t) hp.coeff_floats;
	std::vector<CoeffEvent> events(hp.ev_capacity + 1);
	std::vector<uint32_t> block_events(4 * hp.group_blocks.size() + 4, 0);
	if (hp.frame.sparse_coeffs) { plan.events = events.data(); plan.ev_range = hp.ev_range.data(); plan.block_events = block_events.data(); }
	plan.vb_coeffoff_qfidx = hp.vb_coeffoff_qfidx.data(); plan.vb_hfmul_inv = hp.vb_hfmul_inv.data();
	plan.xfromy = hp.xfromy.data(); plan.bfromy = hp.bfromy.data();
	plan.nonzeros = nonzeros.data(); plan.status = status.data();
	plan.lz_window = window.empty() ? nullptr : window.data(); plan.lz_window_size = hp.lz_window_size;
	plan.section_end_bit = end_bits.data();
	for (int32_t g = 0; g < hp.frame.num_groups; ++g) decode_hf_group(plan, g, false);

	// the extra channels' sub-images into frame-wide planes
	HostModPlan tp;
	std::vector<std::pair<int32_t, uint32_t>> header_errors;
	std::vector<int32_t> section_of;
	if (uint32_t e = build_trailer_plan(fr, hp.codestream.data(), hp.codestream.size() - 16, end_bits.data(), status.data(), &tp, &header_errors, &section_of, true)) return e;
	const int32_t W = fr.fh.width, H = fr.fh.height;
	ModBlock blk(tp, hp.codestream.data());   // the block runtime.hip's keep_alpha lays out
	const DevModPlan &mp = blk.plan;
	for (int32_t i = 0; i < tp.frame.num_sections; ++i) {
		const ModTables mt = mod_tables_in_hbm(mp, i);
		if (const uint32_t e = decode_modular_section<false, false>(mp, mt, i)) status[(size_t) section_of[(size_t) i]] = e;
		else section_inverse_rcts(mp, i, 0, 1);
	}
	for (const auto &e : header_errors) status[(size_t) e.first] = e.second;
	{
		uint32_t first = 0, first_off = 0xffffffffu;
		for (size_t i = 0; i < status.size(); ++i) if (status[i] && hp.sections[i].byte_off < first_off) { first = status[i]; first_off = hp.sections[i].byte_off; }
		if (first) return first;
	}
	const bool out16 = fmt == J40HIP_U16X4;
	const AlphaScale s = alpha_scale_make(fr.im.bpp, out16);
	const int16_t *alpha = blk.lay.plane(blk.base, (size_t) index);
	for (int32_t y = 0; y < H; ++y) {
		if (out16) alpha_merge_row<true>(rgba + (size_t) y * stride, alpha + (size_t) y * (size_t) W, W, s);
		else alpha_merge_row<false>(rgba + (size_t) y * stride, alpha + (size_t) y * (size_t) W, W, s);
	}
	return 0;
}
