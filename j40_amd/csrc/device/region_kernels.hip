// j40_amd/csrc/device/region_kernels.hip -- the kernels of a region decode (j40hip_frame_set_region; region_dev.h has the functions,
// runtime.hip: decode_region decides what runs).
//
// k_region_count / k_region_scan / k_region_scatter: the group-major index of the pixel kernels' varblock list, once per upload.
// k_region_gather: per region, the cover's varblocks of every class into the region's list, and the cover's groups into the `order`
// list of the fast entropy kernel. One workgroup per (cover group, class): it adds up where its segment starts -- the host passes
// only the region's class_start --, then its lanes copy the segment's varblocks, 40 bytes each, a lane a varblock.
// k_region_crop: the rectangle out of the cover-sized staging image. A lane takes 16 bytes where source and destination rows sit
// alike within 16 bytes, neighbouring lanes neighbouring pieces: a wavefront reads and writes 1 KiB of one row at a time, every byte
// of the rectangle crosses HBM once in each direction.
#include <hip/hip_runtime.h>
#include <algorithm>
#include "region_dev.h"
#include "kernels.h"

namespace j40hip {

__global__ __launch_bounds__(256) void k_region_count(const DevVarblock *sorted, uint32_t count, int32_t shift, int32_t gcolumns, uint32_t *cursor) {
	const uint32_t i = blockIdx.x * 256u + threadIdx.x;
	if (i < count) region_count_one(sorted[i], shift, gcolumns, cursor);
}

__global__ __launch_bounds__(REGION_SCAN_LANES) void k_region_scan(uint32_t *cursor, uint32_t *seg_start, uint32_t nkeys) {
	__shared__ uint32_t sums[REGION_SCAN_LANES];
	const int32_t lane = (int32_t) threadIdx.x;
	uint32_t lo, hi;
	region_scan_span(nkeys, lane, &lo, &hi);
	sums[lane] = region_scan_sum(cursor, lo, hi);
	__syncthreads();
	uint32_t at = 0;
	for (int32_t k = 0; k < lane; ++k) at += sums[k];
	region_scan_write(cursor, seg_start, lo, hi, at);
	if (lane == REGION_SCAN_LANES - 1) seg_start[nkeys] = at + sums[lane];
}

__global__ __launch_bounds__(256) void k_region_scatter(const DevVarblock *sorted, uint32_t count, int32_t shift, int32_t gcolumns, uint32_t *cursor, uint32_t *index) {
	const uint32_t i = blockIdx.x * 256u + threadIdx.x;
	if (i < count) region_scatter_one(i, sorted[i], shift, gcolumns, cursor, index);
}

struct RegionClassStart { int32_t v[REGION_KEYS]; };

// grid: (the cover's groups, REGION_KEYS - 1 classes)
__global__ __launch_bounds__(64) void k_region_gather(const DevVarblock *sorted, const uint32_t *index, const uint32_t *seg_start, RegionCover cover, RegionClassStart class_start,
		DevVarblock *list, uint32_t *order) {
	const int32_t i = (int32_t) blockIdx.x, d = (int32_t) blockIdx.y, lane = (int32_t) threadIdx.x;
	const uint32_t g = (uint32_t) region_cover_group(cover, i);
	if (d == 0 && lane == 0) order[i] = g;
	const uint32_t k = g * REGION_KEYS + (uint32_t) d, src0 = seg_start[k], n = seg_start[k + 1] - src0;
	if (n == 0) return;   // (uniform over the workgroup)
	uint32_t before = region_prefix_share(cover, seg_start, i, d, lane, 64);
	for (int off = 32; off > 0; off >>= 1) before += __shfl_xor(before, off, 64);
	const uint32_t dst0 = (uint32_t) class_start.v[d] + before;
	for (uint32_t j = (uint32_t) lane; j < n; j += 64) region_gather_one(sorted, index, src0, list, dst0, j, cover.gx0 << cover.shift, cover.gy0 << cover.shift);
}

// src, dst: the rectangle's first pixel in either image; block (64, 4): 64 lanes along a row, 4 rows
template <int PB>
__global__ __launch_bounds__(256) void k_region_crop(const uint8_t *src, size_t src_stride, uint8_t *dst, size_t dst_stride, int32_t w, int32_t h) {
	const int32_t y = (int32_t) (blockIdx.y * blockDim.y + threadIdx.y);
	if (y >= h) return;
	region_crop_row<PB>(src + (size_t) y * src_stride, dst + (size_t) y * dst_stride, w, (int32_t) (blockIdx.x * 64 + threadIdx.x), (int32_t) (gridDim.x * 64));
}

void launch_region_index(const DevVarblock *sorted, uint32_t count, int32_t shift, int32_t gcolumns, uint32_t nkeys, uint32_t *cursor, uint32_t *seg_start, uint32_t *index, hipStream_t stream) {
	(void) hipMemsetAsync(cursor, 0, sizeof(uint32_t) * nkeys, stream);
	const unsigned blocks = (count + 255u) / 256u;
	if (count) hipLaunchKernelGGL(k_region_count, dim3(blocks), dim3(256), 0, stream, sorted, count, shift, gcolumns, cursor);
	hipLaunchKernelGGL(k_region_scan, dim3(1), dim3(REGION_SCAN_LANES), 0, stream, cursor, seg_start, nkeys);
	if (count) hipLaunchKernelGGL(k_region_scatter, dim3(blocks), dim3(256), 0, stream, sorted, count, shift, gcolumns, cursor, index);
}

void launch_region_gather(const DevVarblock *sorted, const uint32_t *index, const uint32_t *seg_start, const RegionCover &cover, const int32_t *class_start, DevVarblock *list, uint32_t *order, hipStream_t stream) {
	RegionClassStart cs;
	for (int d = 0; d < REGION_KEYS; ++d) cs.v[d] = class_start[d];
	hipLaunchKernelGGL(k_region_gather, dim3((unsigned) region_cover_groups(cover), REGION_KEYS - 1), dim3(64), 0, stream, sorted, index, seg_start, cover, cs, list, order);
}

void launch_region_crop(const uint8_t *src, size_t src_stride, uint8_t *dst, size_t dst_stride, int32_t w, int32_t h, int32_t pixel_bytes, hipStream_t stream) {
	if (w <= 0 || h <= 0) return;
	const int32_t slab = 4 * 65535;   // rows one launch covers (gridDim.y)
	const int64_t pieces = (int64_t) w * pixel_bytes / 16 + 2;
	const unsigned gx = (unsigned) std::min<int64_t>((pieces + 63) / 64, 64);
	for (int32_t y = 0; y < h; y += slab) {
		const int32_t rows = h - y < slab ? h - y : slab;
		const dim3 block(64, 4), grid(gx, (unsigned) ((rows + 3) / 4));
		if (pixel_bytes == 8) hipLaunchKernelGGL(k_region_crop<8>, grid, block, 0, stream, src + (size_t) y * src_stride, src_stride, dst + (size_t) y * dst_stride, dst_stride, w, rows);
		else hipLaunchKernelGGL(k_region_crop<4>, grid, block, 0, stream, src + (size_t) y * src_stride, src_stride, dst + (size_t) y * dst_stride, dst_stride, w, rows);
	}
}

} // namespace j40hip
