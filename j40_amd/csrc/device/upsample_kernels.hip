// j40_amd/csrc/device/upsample_kernels.hip -- upsampling: k_upsample<K>, K = 2, 4, 8, the three coded XYB planes of a frame stretched K
// times into its shown-size planes; one workgroup of 256 threads per 32 x 8 tile of coded samples of one plane, the tile's mirrored
// 36 x 12 halo and the expanded weight table in LDS, the lanes laid along the output row (upsample_dev.h has the rule, the tile functions
// and the reasons for the shape; runtime.hip: apply_upsampling decides when it runs).
#include <hip/hip_runtime.h>
#include "upsample_dev.h"
#include "kernels.h"

namespace j40hip {

// src: three planes of w x h floats, one behind the other; out: three of up_w x up_h; e: the expanded table, K * K * 25 floats (device memory)
template <int K> __global__ __launch_bounds__(UP_THREADS) void k_upsample(const float *__restrict__ src, int32_t w, int32_t h, float *__restrict__ out, int32_t up_w, int32_t up_h, const float *__restrict__ e, int32_t tiles_x) {
	__shared__ float tile[UP_LDS_FLOATS];
	__shared__ float table[K * K * 25];
	const int32_t t = (int32_t) threadIdx.x, tx = (int32_t) blockIdx.x % tiles_x, ty = (int32_t) blockIdx.x / tiles_x, c = (int32_t) blockIdx.y;
	for (int32_t i = t; i < K * K * 25; i += UP_THREADS) table[i] = e[i];
	upsample_tile_stage(tile, src + (size_t) c * (size_t) w * (size_t) h, w, h, tx, ty, t);
	__syncthreads();
	upsample_tile_lane<K>(out + (size_t) c * (size_t) up_w * (size_t) up_h, (size_t) up_w, up_w, up_h, w, h, tile, table, tx, ty, t);
}

// false: a factor or a size the kernel does not take (nothing is launched)
bool launch_upsample(const float *src, int32_t w, int32_t h, int32_t k, const float *table_dev, float *out, int32_t up_w, int32_t up_h, hipStream_t stream) {
	if (!upsample_factor_valid(k) || w <= 0 || h <= 0 || up_w <= 0 || up_h <= 0 || (int64_t) up_w > (int64_t) k * w || (int64_t) up_h > (int64_t) k * h) return false;
	const int32_t tiles_x = (w + UP_TILE_W - 1) / UP_TILE_W, tiles_y = (h + UP_TILE_H - 1) / UP_TILE_H;
	const dim3 grid((unsigned) tiles_x * (unsigned) tiles_y, 3), block(UP_THREADS);
	if (k == 2) hipLaunchKernelGGL(k_upsample<2>, grid, block, 0, stream, src, w, h, out, up_w, up_h, table_dev, tiles_x);
	else if (k == 4) hipLaunchKernelGGL(k_upsample<4>, grid, block, 0, stream, src, w, h, out, up_w, up_h, table_dev, tiles_x);
	else hipLaunchKernelGGL(k_upsample<8>, grid, block, 0, stream, src, w, h, out, up_w, up_h, table_dev, tiles_x);
	return true;
}

} // namespace j40hip
