// tests/hostsim/region_sim.cpp -- TEST INFRASTRUCTURE: region decode on the CPU (build/libhostsim_region.so). The product's host parser
// and plan builder give the pixel kernels' varblock list; the functions of device/region_dev.h -- the ones k_region_count / _scan /
// _scatter / _gather / _crop run, lane by lane -- build the group-major index over it, gather a rectangle's cover into a list of its
// own and cut a rectangle out of an image: without a device.
#include <cstdint>
#include <cstring>
#include <vector>
#include <algorithm>
#include "../../j40_amd/csrc/plan_build.hpp"
#include "../../j40_amd/csrc/device/region_dev.h"
#include "../../include/j40hip.h"

using namespace j40hip;

#define REGION_SIM_API extern "C" __attribute__((visibility("default")))

struct RegionSim {
	int32_t width, height, shift, gcolumns, num_groups;
	std::vector<DevVarblock> sorted;
	int32_t class_start[28];
	std::vector<uint32_t> cursor, seg_start, index;
};

// parses the stream, builds the plan and the index (count, scan over REGION_SCAN_LANES lanes, scatter). Null + *err on failure.
REGION_SIM_API RegionSim *region_sim_open(const uint8_t *buf, size_t size, uint32_t *err) {
	Frame fr;
	const uint8_t *cs; size_t cs_size; std::vector<uint8_t> storage;
	HostPlan hp;
	try {
		extract_codestream(buf, size, &cs, &cs_size, &storage);
		parse_frame(cs, cs_size, &fr, 1);
	} catch (const DecodeError &e) { *err = e.code; return nullptr; }
	if (fr.fh.is_modular) { *err = ERR_TODO; return nullptr; }
	if (uint32_t e = build_vardct_plan(fr, cs, cs_size, &hp)) { *err = e; return nullptr; }
	RegionSim *r = new RegionSim();
	r->width = fr.fh.width; r->height = fr.fh.height; r->shift = fr.fh.group_size_shift; r->gcolumns = fr.fh.gcolumns; r->num_groups = (int32_t) fr.fh.num_groups;
	r->sorted = hp.vb_sorted;
	memcpy(r->class_start, hp.class_start, sizeof r->class_start);
	const uint32_t nkeys = (uint32_t) r->num_groups * REGION_KEYS, count = (uint32_t) r->sorted.size();
	r->cursor.assign(nkeys, 0); r->seg_start.assign((size_t) nkeys + 1, 0); r->index.assign(std::max<size_t>(count, 1), 0xffffffffu);
	for (uint32_t i = 0; i < count; ++i) region_count_one(r->sorted[i], r->shift, r->gcolumns, r->cursor.data());
	uint32_t sums[REGION_SCAN_LANES], at = 0;
	for (int lane = 0; lane < REGION_SCAN_LANES; ++lane) { uint32_t lo, hi; region_scan_span(nkeys, lane, &lo, &hi); sums[lane] = region_scan_sum(r->cursor.data(), lo, hi); }
	for (int lane = 0; lane < REGION_SCAN_LANES; ++lane) { uint32_t lo, hi; region_scan_span(nkeys, lane, &lo, &hi); region_scan_write(r->cursor.data(), r->seg_start.data(), lo, hi, at); at += sums[lane]; }
	r->seg_start[nkeys] = at;
	for (uint32_t i = count; i-- > 0; ) region_scatter_one(i, r->sorted[i], r->shift, r->gcolumns, r->cursor.data(), r->index.data());   // (backwards: the order inside a segment is not the list's)
	*err = 0;
	return r;
}
REGION_SIM_API void region_sim_close(RegionSim *r) { delete r; }
// out6: width, height, group shift, group columns, groups, varblocks
REGION_SIM_API void region_sim_info(const RegionSim *r, int32_t *out6) {
	out6[0] = r->width; out6[1] = r->height; out6[2] = r->shift; out6[3] = r->gcolumns; out6[4] = r->num_groups; out6[5] = (int32_t) r->sorted.size();
}
static void put(const DevVarblock &v, int32_t *o) { o[0] = v.px; o[1] = v.py; o[2] = v.effw; o[3] = v.effh; o[4] = v.dctsel; o[5] = v.blk; o[6] = v.llf_base; o[7] = v.coeff_base; }
// the whole list as the pixel kernels take it: out8 = px, py, effw, effh, dctsel, blk, llf_base, coeff_base per varblock
REGION_SIM_API void region_sim_sorted(const RegionSim *r, int32_t *out8, int32_t *class_start28) {
	for (size_t i = 0; i < r->sorted.size(); ++i) put(r->sorted[i], out8 + 8 * i);
	memcpy(class_start28, r->class_start, sizeof r->class_start);
}
// the region's list: class_start from the segments' sizes as the host computes it (runtime.hip: region_gather), the gather as
// k_region_gather's workgroups do it (`lanes` lanes each); cover4: first column, first row, columns, rows; returns the count, or -1
// when an entry would land outside [0, count) or is written twice
REGION_SIM_API int64_t region_sim_gather(const RegionSim *r, int32_t x0, int32_t y0, int32_t w, int32_t h, int32_t lanes, int32_t *out8, int64_t capacity, int32_t *class_start28, int32_t *cover4, uint32_t *order) {
	const RegionCover cover = region_cover(x0, y0, w, h, r->shift, r->gcolumns);
	cover4[0] = cover.gx0; cover4[1] = cover.gy0; cover4[2] = cover.cols; cover4[3] = cover.rows;
	const int32_t n = region_cover_groups(cover);
	int32_t at = 0;
	for (int d = 0; d < REGION_KEYS; ++d) {
		class_start28[d] = at;
		for (int32_t i = 0; i < n; ++i) { const size_t k = (size_t) region_cover_group(cover, i) * REGION_KEYS + (size_t) d; at += (int32_t) (r->seg_start[k + 1] - r->seg_start[k]); }
	}
	const int64_t total = class_start28[REGION_KEYS - 1];
	if (total > capacity) return -1;
	DevVarblock blank; memset(&blank, 0xff, sizeof blank);
	std::vector<DevVarblock> list((size_t) total, blank);
	std::vector<uint8_t> written((size_t) total, 0);
	for (int32_t i = 0; i < n; ++i) {
		order[i] = (uint32_t) region_cover_group(cover, i);
		for (int d = 0; d < REGION_KEYS - 1; ++d) {
			const size_t k = (size_t) order[i] * REGION_KEYS + (size_t) d;
			const uint32_t src0 = r->seg_start[k], cnt = r->seg_start[k + 1] - src0;
			uint32_t before = 0;
			for (int32_t lane = 0; lane < lanes; ++lane) before += region_prefix_share(cover, r->seg_start.data(), i, d, lane, lanes);
			const uint32_t dst0 = (uint32_t) class_start28[d] + before;
			for (uint32_t j = 0; j < cnt; ++j) {
				if ((int64_t) dst0 + j >= total || written[dst0 + j]) return -1;
				written[dst0 + j] = 1;
				region_gather_one(r->sorted.data(), r->index.data(), src0, list.data(), dst0, j, cover.gx0 << cover.shift, cover.gy0 << cover.shift);
			}
		}
	}
	for (int64_t i = 0; i < total; ++i) { if (!written[(size_t) i]) return -1; put(list[(size_t) i], out8 + 8 * i); }
	return total;
}

// region_crop_row over the h rows of a rectangle of w pixels of pixel_bytes (4 or 8), `lanes` lanes a row; src and dst point at the
// rectangle's first pixel
REGION_SIM_API void region_sim_crop(const uint8_t *src, size_t src_stride, uint8_t *dst, size_t dst_stride, int32_t w, int32_t h, int32_t pixel_bytes, int32_t lanes) {
	for (int32_t y = 0; y < h; ++y) for (int32_t lane = 0; lane < lanes; ++lane) {
		if (pixel_bytes == 8) region_crop_row<8>(src + (size_t) y * src_stride, dst + (size_t) y * dst_stride, w, lane, lanes);
		else region_crop_row<4>(src + (size_t) y * src_stride, dst + (size_t) y * dst_stride, w, lane, lanes);
	}
}
