// tests/hostsim/wide_sim.cpp -- TEST INFRASTRUCTURE ONLY. Wide Modular frames (images with 32-bit Modular buffers, J40HIP_PARSE_WIDE) on
// the CPU: the device functions of the Modular path (j40_amd/csrc/device/modular_dev.h, squeeze_dev.h) instantiated with int32_t
// samples and run with the runtime's orchestration (device/runtime_upload.hip, runtime.hip), over planes laid out by the product's
// ModPlanLayout in a block with guard bytes (mod_block.hpp). The same template instantiated with int16_t serves narrow frames, so
// that the two paths can be compared through one orchestration (tests/test_wide_modular.py). Never linked into the product library.
#include <cstdint>
#include <cstring>
#include <vector>
#include <algorithm>
#include "../../j40_amd/csrc/plan_build.hpp"
#include "../../j40_amd/csrc/device/modular_dev.h"
#include "../../j40_amd/csrc/device/squeeze_dev.h"
#include "../../include/j40hip.h"
#include "mod_block.hpp"

using namespace j40hip;

namespace {

// what the last widesim_decode left: the coded planes' extremes before any inverse transform, the final planes
int64_t g_coded_min = 0, g_coded_max = 0;
std::vector<std::vector<int32_t>> g_final;
std::vector<int32_t> g_final_w, g_final_h;
int32_t g_sample_bytes = 0, g_neighbour_flip = 0;

// out_format: 0 RGBA u8 x 4, 1 RGBA u16 x 4 (little endian, R first)
template <typename S>
uint32_t decode_modular(const Frame &fr, const HostModPlan &hp, int out_format, uint8_t *out) {
	typedef typename ModWideOf<S>::type E;
	ModBlock blk(hp, hp.codestream.data());   // the block runtime_upload.hip's upload_modular lays out
	const DevModPlan &plan = blk.plan;
	uint32_t *status = plan.status;   // [num_sections + 1]
	struct Ref { S *p; int32_t w, h; };
	std::vector<Ref> planes;
	for (size_t c = 0; c < blk.lay.num_planes; ++c) planes.push_back({(S *) blk.lay.plane_any(blk.base, c), hp.plane_w[c], hp.plane_h[c]});
	// the rows and the weighted predictor's cells as the kernel lays them out in LDS: the cells are E (64-bit in a wide frame)
	std::vector<int32_t> ring(3 * ((size_t) hp.frame.max_width + 4) + 8, 0x7fff0000);
	std::vector<E> wperr(10 * (size_t) hp.frame.max_width + 8);
	for (int32_t sct = 0; sct < hp.frame.num_sections; ++sct) {
		const DevModSection &sec = hp.sections[(size_t) sct];
		if (sec.preset_status) { status[(size_t) sct] = sec.preset_status; continue; }
		if (sizeof(S) == 4 && (sec.quad || sec.split)) return ERR_RNGE;   // (the plan must never hand a wide section to the int16-only kernels)
		ModTables mt = mod_tables_in_hbm(plan, sct);
		mt.rows = ring.data(); mt.rows_width = hp.frame.max_width + 4; mt.wp_errors = (int32_t *) wperr.data(); mt.wp_errors_width = hp.frame.max_width;
		status[(size_t) sct] = ((sct ^ g_neighbour_flip) & 1) ? decode_modular_section<false, true, S>(plan, mt, sct) : decode_modular_section<false, false, S>(plan, mt, sct);   // both neighbour sources
	}
	{   // like j40hip_frame_status: the first failing section in file order
		uint32_t first = 0, first_off = 0xffffffffu;
		for (size_t i = 0; i < hp.sections.size(); ++i) if (status[i] && hp.sections[i].byte_off < first_off) { first = status[i]; first_off = hp.sections[i].byte_off; }
		if (first) return first;
	}
	g_coded_min = INT64_MAX; g_coded_max = INT64_MIN;
	for (const Ref &r : planes) for (size_t i = 0; i < (size_t) std::max(r.w, 0) * (size_t) std::max(r.h, 0); ++i) { g_coded_min = std::min<int64_t>(g_coded_min, r.p[i]); g_coded_max = std::max<int64_t>(g_coded_max, r.p[i]); }
	for (int32_t sct = 0; sct < hp.frame.num_sections; ++sct) for (int32_t lane = 0; lane < 3; ++lane) section_inverse_rcts<S>(plan, sct, lane, 3);
	static const uint8_t PERM[6][3] = {{0, 1, 2}, {1, 2, 0}, {2, 0, 1}, {0, 2, 1}, {1, 0, 2}, {2, 1, 0}};
	std::vector<std::vector<S>> extra;
	extra.reserve(1024);
	// undoes `trs` last to first on the image `planes` (the frame, or the sub-image of a section with a palette of its own)
	auto undo = [&](std::vector<Ref> &planes, const std::vector<Transform> &trs, const int8_t *wpb) -> uint32_t {
		for (size_t ti = trs.size(); ti-- > 0; ) {
			const Transform &t = trs[ti];
			if (t.kind == Transform::RCT) {
				Ref c[3] = {planes[(size_t) t.begin_c], planes[(size_t) t.begin_c + 1], planes[(size_t) t.begin_c + 2]};
				const size_t n = (size_t) c[0].w * (size_t) c[0].h;
				for (size_t i = 0; i < n; ++i) inverse_rct_pixel(t.rct_type % 7, c[0].p[i], c[1].p[i], c[2].p[i]);
				for (int i = 0; i < 3; ++i) planes[(size_t) (t.begin_c + PERM[t.rct_type / 7][i])] = c[i];
			} else if (t.kind == Transform::SQUEEZE) {
				const int32_t nc = (int32_t) planes.size(), end_c = t.begin_c + t.num_c, offset = t.in_place ? end_c : nc - t.num_c;
				for (int32_t c = t.begin_c; c < end_c; ++c) {
					const Ref avg = planes[(size_t) c], res = planes[(size_t) (offset + c - t.begin_c)];
					Ref o = {nullptr, t.horizontal ? avg.w + res.w : avg.w, t.horizontal ? avg.h : avg.h + res.h};
					extra.emplace_back((size_t) std::max(o.w, 0) * (size_t) std::max(o.h, 0) + 1, 0); o.p = extra.back().data();
					if (t.horizontal) for (int32_t y = 0; y < o.h; ++y)
						unsqueeze_line(avg.p + (size_t) y * (size_t) avg.w, 1, res.w > 0 ? res.p + (size_t) y * (size_t) res.w : avg.p, 1, avg.w, res.w, o.p + (size_t) y * (size_t) o.w, 1);
					else for (int32_t x = 0; x < o.w; ++x)
						unsqueeze_line(avg.p + x, avg.w, res.h > 0 ? res.p + x : avg.p, res.w, avg.h, res.h, o.p + x, o.w);
					planes[(size_t) c] = o;
				}
				planes.erase(planes.begin() + offset, planes.begin() + offset + t.num_c);
			} else {
				const int32_t first = t.begin_c + 1;
				const Ref idx = planes[(size_t) first], pal = planes[0];
				const size_t n = (size_t) idx.w * (size_t) idx.h;
				std::vector<Ref> outs;
				for (int32_t i = 0; i < t.num_c - 1; ++i) { extra.emplace_back(n + 1, 0); outs.push_back({extra.back().data(), idx.w, idx.h}); }
				outs.push_back(idx);
				ModWPT<E> wp;
				wp.on = t.nb_deltas > 0 && t.d_pred == 6; wp.width = idx.w; std::vector<E> errs((size_t) 2 * (size_t) idx.w * 5 + 16, 0); wp.errors = errs.data();
				wp.p1 = wpb[0]; wp.p2 = wpb[1]; for (int i = 0; i < 5; ++i) wp.p3[i] = wpb[2 + i]; for (int i = 0; i < 4; ++i) wp.w[i] = wpb[7 + i];
				uint32_t err = 0;
				for (int32_t i = 0; i < t.num_c; ++i) {
					const S *palrow = t.nb_colours > 0 ? pal.p + (size_t) i * (size_t) pal.w : nullptr;
					std::fill(errs.begin(), errs.end(), 0);
					for (int k = 0; k < 5; ++k) wp.pred[k] = 0;
					wp.blend_err_w = wp.blend_err_n = wp.blend_err_nw = wp.blend_err_ne = 0;
					for (int32_t y = 0; y < idx.h; ++y) for (int32_t x = 0; x < idx.w; ++x) {
						const S index = idx.p[(size_t) y * (size_t) idx.w + (size_t) x];
						S val = palette_value(index, i, palrow, t.nb_colours, fr.im.bpp);
						if (t.nb_deltas > 0) {
							S *line = outs[(size_t) i].p + (size_t) y * (size_t) idx.w;
							const ModNeigh p = mod_neighbours<false>(line, idx.w, idx.w, x, y);
							wp_before<false>(wp, x, y, p);
							if (index < t.nb_deltas) val = (S) (uint32_t) (uint64_t) (val + mod_predict(t.d_pred, wp, p, &err));
							wp_after(wp, x, y, val);
						}
						outs[(size_t) i].p[(size_t) y * (size_t) idx.w + (size_t) x] = val;
					}
				}
				if (err) return err;
				std::vector<Ref> next(planes.begin() + 1, planes.begin() + first);
				next.insert(next.end(), outs.begin(), outs.end());
				next.insert(next.end(), planes.begin() + first + 1, planes.end());
				planes.swap(next);
			}
		}
		return 0;
	};
	for (const HostModPlan::SubImage &si : hp.sub_images) if (si.paste) {
		std::vector<Ref> sp;
		for (int32_t k = 0; k < si.num_planes; ++k) sp.push_back({(S *) blk.lay.sub_plane_any(blk.base, (size_t) (si.first_plane + k)), hp.sub_w[(size_t) (si.first_plane + k)], hp.sub_h[(size_t) (si.first_plane + k)]});
		if (uint32_t e = undo(sp, si.transforms, si.wp)) return e;
		const DevModSection &sec = hp.sections[(size_t) si.section];
		for (size_t c = 0; c < sp.size(); ++c) {
			const Ref &dst = planes[(size_t) sec.first_channel + c];
			for (int32_t y = 0; y < sp[c].h; ++y) memcpy(dst.p + (size_t) (sec.gy + y) * (size_t) dst.w + (size_t) sec.gx, sp[c].p + (size_t) y * (size_t) sp[c].w, sizeof(S) * (size_t) sp[c].w);
		}
	}
	{ int8_t gwp[12]; const WPParams &gp = fr.gmodular.wp; gwp[0] = gp.p1; gwp[1] = gp.p2; for (int i = 0; i < 5; ++i) gwp[2 + i] = gp.p3[i]; for (int i = 0; i < 4; ++i) gwp[7 + i] = gp.w[i]; gwp[11] = 0;
	  if (uint32_t e = undo(planes, hp.transforms, gwp)) return e; }
	const int32_t W = hp.frame.width, H = hp.frame.height;
	if (planes.size() < 3) return ERR_TODO;
	for (const Ref &r : planes) { g_final.emplace_back(r.p, r.p + (size_t) std::max(r.w, 0) * (size_t) std::max(r.h, 0)); g_final_w.push_back(r.w); g_final_h.push_back(r.h); }
	const int32_t opaque = (1 << fr.im.bpp) - 1;
	for (size_t i = 0; i < (size_t) W * (size_t) H; ++i) {
		const int32_t a = hp.alpha_channel >= 0 ? (int32_t) planes[(size_t) hp.alpha_channel].p[i] : opaque;
		if (out_format == 1) { const uint64_t px = pack_rgba16(planes[0].p[i], planes[1].p[i], planes[2].p[i], a, fr.im.bpp); memcpy(out + i * 8, &px, 8); }
		else { const uint32_t px = pack_rgba8(planes[0].p[i], planes[1].p[i], planes[2].p[i], a, fr.im.bpp); memcpy(out + i * 4, &px, 4); }
	}
	return 0;
}

} // namespace

#define WIDESIM_API extern "C" __attribute__((visibility("default")))

// parses `buf` with `flags` (j40hip_frame_parse_ex's: J40HIP_PARSE_WIDE asks for wide frames) as the C-ABI does; 0 or the 4-char code
WIDESIM_API uint32_t widesim_parse(const uint8_t *buf, size_t size, uint32_t flags, int32_t *out4 /* wide, bpp, is_modular, sample_bytes of its plan; or null */) {
	try {
		Frame fr;
		fr.allow_wide = (flags & J40HIP_PARSE_WIDE) != 0;
		const uint8_t *cs; size_t cs_size; std::vector<uint8_t> storage;
		extract_codestream(buf, size, &cs, &cs_size, &storage);
		parse_frame(cs, cs_size, &fr, 1);
		if (out4) { out4[0] = fr.wide(); out4[1] = fr.im.bpp; out4[2] = fr.fh.is_modular; out4[3] = 0; }
		return 0;
	} catch (const DecodeError &e) { return e.code; }
}

// decodes a Modular stream with the device functions on the CPU. out: width * height * 4 bytes (out_format 0, u8) or * 8 (1, u16);
// flags: j40hip_frame_parse_ex's. Returns 0 or the first error code
WIDESIM_API uint32_t widesim_decode(const uint8_t *buf, size_t size, uint8_t *out, int out_format, uint32_t flags) {
	mod_block_reset();
	g_final.clear(); g_final_w.clear(); g_final_h.clear(); g_sample_bytes = 0; g_coded_min = g_coded_max = 0;
	try {
		Frame fr;
		fr.allow_wide = (flags & J40HIP_PARSE_WIDE) != 0;
		const uint8_t *cs; size_t cs_size; std::vector<uint8_t> storage;
		extract_codestream(buf, size, &cs, &cs_size, &storage);
		parse_frame(cs, cs_size, &fr, 1);
		HostModPlan hp;
		if (uint32_t e = build_modular_plan(fr, cs, cs_size, &hp)) return e;
		g_sample_bytes = hp.frame.sample_bytes;
		return hp.frame.sample_bytes == 4 ? decode_modular<int32_t>(fr, hp, out_format, out) : decode_modular<int16_t>(fr, hp, out_format, out);
	} catch (const DecodeError &e) { return e.code; }
}

WIDESIM_API void widesim_set_neighbour_flip(int32_t flip) { g_neighbour_flip = flip & 1; }
// of the last widesim_decode: bytes per sample of its planes; the smallest and largest coded sample before any inverse transform; its
// plan's sections in all and those the cooperative / quad / split kernels would take
WIDESIM_API int32_t widesim_sample_bytes(void) { return g_sample_bytes; }
WIDESIM_API void widesim_coded_range(int64_t *out2) { out2[0] = g_coded_min; out2[1] = g_coded_max; }
// channel c of the last decode after the inverse transforms, as int32 (whatever the sample size); returns its sample count, or -1
WIDESIM_API int64_t widesim_final_plane(int32_t c, int32_t *out, int32_t *w, int32_t *h) {
	if (c < 0 || (size_t) c >= g_final.size()) return -1;
	if (w) *w = g_final_w[(size_t) c];
	if (h) *h = g_final_h[(size_t) c];
	if (out) memcpy(out, g_final[(size_t) c].data(), sizeof(int32_t) * g_final[(size_t) c].size());
	return (int64_t) g_final[(size_t) c].size();
}
// the Modular blocks of the last widesim_decode (mod_block.hpp): guard bytes that no longer read 0x5a; the bytes of the regions called `name`
WIDESIM_API int64_t widesim_guard_damage(void) { return (int64_t) g_guard_damage; }
WIDESIM_API int64_t widesim_region_bytes(const char *name) { return mod_block_region_bytes(name); }
// the plan of a stream: out[0] sections, [1] cooperative, [2] quad, [3] split, [4] sample_bytes; 0 or the code
WIDESIM_API uint32_t widesim_plan_counts(const uint8_t *buf, size_t size, uint32_t flags, int32_t *out5) {
	try {
		Frame fr;
		fr.allow_wide = (flags & J40HIP_PARSE_WIDE) != 0;
		const uint8_t *cs; size_t cs_size; std::vector<uint8_t> storage;
		extract_codestream(buf, size, &cs, &cs_size, &storage);
		parse_frame(cs, cs_size, &fr, 1);
		HostModPlan hp;
		if (uint32_t e = build_modular_plan(fr, cs, cs_size, &hp)) return e;
		out5[0] = (int32_t) hp.sections.size(); out5[1] = hp.coop_sections; out5[2] = hp.quad_sections; out5[3] = hp.split_sections; out5[4] = hp.frame.sample_bytes;
		return 0;
	} catch (const DecodeError &e) { return e.code; }
}
