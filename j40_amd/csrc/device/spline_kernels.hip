// j40_amd/csrc/device/spline_kernels.hip -- splines: k_spline_draw, the frame's segments splatted onto its XYB planes in place, one
// workgroup of 256 threads per touched 64 x 32 tile, the tile's segments staged in LDS in chunks and walked in list order by every lane
// (spline_dev.h has the rule, the lane function and the reasons for the shape; runtime.hip: apply_splines decides when it runs).
// The chunk: SPLINE_CHUNK = 128 segments, 6 KiB of LDS a workgroup. What limits residency is registers, not LDS: the kernel takes 128
// VGPRs (24 plane values a lane, the splat's temporaries, no scratch), which allows 4 wavefronts a SIMD, four of these 256-thread
// workgroups a compute unit -- 24 KiB of its 160 KiB of LDS. A chunk up to 40 KiB would change nothing there, so the size is set by the
// other side: 128 segments make a chunk's two barriers vanish beside its arithmetic, and six words a thread stage it. Every lane reads
// the same segment words at a time, a broadcast, so the layout needs no padding against bank conflicts.
// No fast-math here: division and sqrtf stay correctly rounded (-fhip-fp32-correctly-rounded-divide-sqrt), nothing is contracted
// (-ffp-contract=off), so that numpy's float32 reproduces every bit.
#include <hip/hip_runtime.h>
#include "spline_dev.h"
#include "kernels.h"

namespace j40hip {

__global__ __launch_bounds__(SPLINE_TILE_W * SPLINE_WAVES) void k_spline_draw(float *planes, size_t pitch, size_t plane, int32_t W, int32_t H, DevSplines d) {
	__shared__ uint32_t chunk[SPLINE_CHUNK * SPLINE_SEG_WORDS];
	const int32_t tile = d.tile_ids[blockIdx.x], tx = tile % d.tiles_x, ty = tile / d.tiles_x;
	const int32_t first = d.tile_start[blockIdx.x], last = d.tile_start[blockIdx.x + 1];
	const int32_t lane = (int32_t) threadIdx.x, wave = (int32_t) threadIdx.y, t = wave * SPLINE_TILE_W + lane;
	const int32_t x = tx * SPLINE_TILE_W + lane, y_first = ty * SPLINE_TILE_H + wave * SPLINE_ROWS;
	float P[3][SPLINE_ROWS];
#pragma unroll
	for (int32_t r = 0; r < SPLINE_ROWS; ++r) {
		const bool in = x < W && y_first + r < H;
		const size_t at = (size_t) (y_first + r) * pitch + (size_t) x;
#pragma unroll
		for (int32_t c = 0; c < 3; ++c) P[c][r] = in ? planes[(size_t) c * plane + at] : 0.0f;
	}
	for (int32_t base = first; base < last; base += SPLINE_CHUNK) {
		const int32_t n = min((int32_t) SPLINE_CHUNK, last - base);
		__syncthreads();   // (the chunk before this one has been walked by everybody)
		for (int32_t i = t; i < n * SPLINE_SEG_WORDS; i += SPLINE_TILE_W * SPLINE_WAVES) {
			const int32_t s = i / SPLINE_SEG_WORDS, w = i - s * SPLINE_SEG_WORDS;
			chunk[i] = reinterpret_cast<const uint32_t *>(d.segs + d.seg_idx[base + s])[w];
		}
		__syncthreads();
		spline_lane_walk(reinterpret_cast<const SplineSeg *>(chunk), n, x, y_first, P);
	}
#pragma unroll
	for (int32_t r = 0; r < SPLINE_ROWS; ++r) {
		if (x >= W || y_first + r >= H) continue;
		const size_t at = (size_t) (y_first + r) * pitch + (size_t) x;
#pragma unroll
		for (int32_t c = 0; c < 3; ++c) planes[(size_t) c * plane + at] = P[c][r];
	}
}

void launch_spline_draw(float *planes, size_t pitch, int32_t W, int32_t H, const DevSplines &d, hipStream_t stream) {
	if (W <= 0 || H <= 0 || d.num_tiles <= 0) return;
	hipLaunchKernelGGL(k_spline_draw, dim3((unsigned) d.num_tiles), dim3(SPLINE_TILE_W, SPLINE_WAVES), 0, stream, planes, pitch, pitch * (size_t) H, W, H, d);
}

} // namespace j40hip
