// j40_amd/csrc/device/region_dev.h -- region decode (j40hip_frame_set_region): the arithmetic of a rectangle's cover, the group-major
// index of the pixel kernels' varblock list, the gather of a cover's varblocks into a list of its own, and the copy of a rectangle out
// of the cover-sized staging image. Compiled for the device by region_kernels.hip and for the CPU by tests/hostsim/region_sim.cpp:
// the same functions.
//
// A pass group is entropy-coded in a section of its own and no varblock straddles a group (the largest transform is one group wide), so
// the groups a rectangle intersects -- its cover -- hold everything its pixels depend on: their sections, and the varblocks whose
// top-left pixel lies in them.
//
// The index. The pixel kernels' list (d_vb_sorted) is sorted by DctSelect class; a region needs, per class, the varblocks of a few
// groups. Key k = group * REGION_KEYS + class: the varblocks are counted per key, the counts scanned (seg_start, REGION_KEYS per
// group, one more at the end) and the varblocks' positions in the sorted list scattered into `index`, segment after segment. The order
// inside a segment is whatever the scatter's atomics made it; the pixel kernels do not care, every varblock writes pixels of its own.
#pragma once
#include <stdint.h>
#include <string.h>
#include "plan.h"
#ifndef J40_HD
#ifdef __HIPCC__
#define J40_HD __host__ __device__ __forceinline__
#else
#define J40_HD static inline
#endif
#endif

namespace j40hip {

enum { REGION_KEYS = 28 };   // keys per group: the 27 DctSelect classes, padded to the 28 entries of a class_start table
enum { REGION_SCAN_LANES = 256 };   // lanes of the scan (one workgroup): each takes a run of keys

// the groups a rectangle intersects: columns gx0 .. gx0 + cols - 1 of rows gy0 .. gy0 + rows - 1 of the frame's `gcolumns` x ... groups
struct RegionCover { int32_t gx0, gy0, cols, rows, gcolumns, shift; };

J40_HD RegionCover region_cover(int32_t x0, int32_t y0, int32_t w, int32_t h, int32_t shift, int32_t gcolumns) {
	RegionCover c;
	c.gx0 = x0 >> shift; c.gy0 = y0 >> shift;
	c.cols = ((x0 + w - 1) >> shift) - c.gx0 + 1; c.rows = ((y0 + h - 1) >> shift) - c.gy0 + 1;
	c.gcolumns = gcolumns; c.shift = shift;
	return c;
}
J40_HD int32_t region_cover_groups(const RegionCover &c) { return c.cols * c.rows; }
// the frame's index of the cover's i-th group (row by row)
J40_HD int32_t region_cover_group(const RegionCover &c, int32_t i) { return (c.gy0 + i / c.cols) * c.gcolumns + c.gx0 + i % c.cols; }

J40_HD uint32_t region_fetch_add(uint32_t *p) {
#if defined(__HIP_DEVICE_COMPILE__)
	return atomicAdd(p, 1u);
#else
	return (*p)++;
#endif
}

J40_HD uint32_t region_key(const DevVarblock &vb, int32_t shift, int32_t gcolumns) {
	return (uint32_t) ((vb.py >> shift) * gcolumns + (vb.px >> shift)) * REGION_KEYS + vb.dctsel;
}

// ---- the index: count, scan, scatter ----
// `cursor` holds the counts after the count step (cleared before), every segment's start after the scan, its end after the scatter
J40_HD void region_count_one(const DevVarblock &vb, int32_t shift, int32_t gcolumns, uint32_t *cursor) {
	(void) region_fetch_add(cursor + region_key(vb, shift, gcolumns));
}
// the scan in two steps: lane `lane` of REGION_SCAN_LANES sums keys [lo, hi) -- region_scan_span --, then, given the sum of the lanes
// before it, writes the starts of its keys
J40_HD void region_scan_span(uint32_t nkeys, int32_t lane, uint32_t *lo, uint32_t *hi) {
	const uint32_t per = (nkeys + REGION_SCAN_LANES - 1) / REGION_SCAN_LANES;
	*lo = per * (uint32_t) lane < nkeys ? per * (uint32_t) lane : nkeys;
	*hi = *lo + per < nkeys ? *lo + per : nkeys;
}
J40_HD uint32_t region_scan_sum(const uint32_t *cursor, uint32_t lo, uint32_t hi) {
	uint32_t s = 0;
	for (uint32_t k = lo; k < hi; ++k) s += cursor[k];
	return s;
}
J40_HD void region_scan_write(uint32_t *cursor, uint32_t *seg_start, uint32_t lo, uint32_t hi, uint32_t at) {
	for (uint32_t k = lo; k < hi; ++k) { const uint32_t n = cursor[k]; seg_start[k] = at; cursor[k] = at; at += n; }
}
// varblock i of the sorted list into its segment
J40_HD void region_scatter_one(uint32_t i, const DevVarblock &vb, int32_t shift, int32_t gcolumns, uint32_t *cursor, uint32_t *index) {
	index[region_fetch_add(cursor + region_key(vb, shift, gcolumns))] = i;
}

// ---- the gather: per class, the segments of the cover's groups one behind the other ----
// where the segment of (the cover's i-th group, class d) starts in the region's list = class_start[d] + the class-d varblocks of the
// cover's groups before i. Lane `lane` of `lanes` sums its share of those groups; the caller adds the lanes up.
J40_HD uint32_t region_prefix_share(const RegionCover &c, const uint32_t *seg_start, int32_t i, int32_t d, int32_t lane, int32_t lanes) {
	uint32_t s = 0;
	for (int32_t j = lane; j < i; j += lanes) {
		const uint32_t k = (uint32_t) region_cover_group(c, j) * REGION_KEYS + (uint32_t) d;
		s += seg_start[k + 1] - seg_start[k];
	}
	return s;
}
// the j-th varblock of the segment starting at index[src0] becomes entry dst0 + j of the region's list, its pixel position counted
// from the cover's origin (ox, oy)
J40_HD void region_gather_one(const DevVarblock *sorted, const uint32_t *index, uint32_t src0, DevVarblock *list, uint32_t dst0, uint32_t j, int32_t ox, int32_t oy) {
	DevVarblock v = sorted[index[src0 + j]];
	v.px -= ox; v.py -= oy;
	list[dst0 + j] = v;
}

// ---- the crop: one row of `w` pixels of PB bytes from src to dst, by lane `lane` of `lanes` ----
// Both rows are pixel-aligned. Where they sit alike within 16 bytes the row is a head of pixels up to dst's first 16-byte boundary,
// whole 16-byte pieces (a lane takes every lanes-th piece: neighbouring lanes, neighbouring 16 bytes) and a tail; otherwise pixel by
// pixel. Written once and not read again here: non-temporal stores on the device.
#if defined(__HIP_DEVICE_COMPILE__)
typedef uint32_t region_u32x4 __attribute__((ext_vector_type(4)));
J40_HD void region_copy16(uint8_t *d, const uint8_t *s) { __builtin_nontemporal_store(*(const region_u32x4 *) s, (region_u32x4 *) d); }
template <int PB> J40_HD void region_copy_pixel(uint8_t *d, const uint8_t *s) {
	if (PB == 8) __builtin_nontemporal_store(*(const uint64_t *) s, (uint64_t *) d);
	else __builtin_nontemporal_store(*(const uint32_t *) s, (uint32_t *) d);
}
#else
J40_HD void region_copy16(uint8_t *d, const uint8_t *s) { memcpy(d, s, 16); }
template <int PB> J40_HD void region_copy_pixel(uint8_t *d, const uint8_t *s) { memcpy(d, s, PB); }
#endif

template <int PB> J40_HD void region_crop_row(const uint8_t *src, uint8_t *dst, int32_t w, int32_t lane, int32_t lanes) {
	const uintptr_t sa = (uintptr_t) src & 15u, da = (uintptr_t) dst & 15u;
	int32_t head = w, pieces = 0;
	if (sa == da) {
		head = (int32_t) (((16u - da) & 15u) / PB);
		if (head > w) head = w;
		pieces = (w - head) / (16 / PB);
	}
	const int32_t wide = pieces * (16 / PB), narrow = w - wide;   // pixels in whole pieces; pixels of head and tail
	for (int32_t k = lane; k < pieces; k += lanes) region_copy16(dst + (size_t) head * PB + (size_t) k * 16, src + (size_t) head * PB + (size_t) k * 16);
	for (int32_t k = lane; k < narrow; k += lanes) {
		const size_t x = (size_t) (k < head ? k : k + wide);
		region_copy_pixel<PB>(dst + x * PB, src + x * PB);
	}
}

} // namespace j40hip
