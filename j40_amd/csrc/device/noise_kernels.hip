// j40_amd/csrc/device/noise_kernels.hip -- photon noise: k_noise_fill, the three raw random planes of a frame, one workgroup of 256
// threads per group, every thread one generator lane of one block of rows behind a jump; k_noise_add, their 5 x 5 convolution and the
// per-pixel addition onto the frame's XYB planes in place, one workgroup per 64 x 32 tile with the raw planes' 68 x 36 halo tile in
// LDS (noise_dev.h has the rule, the lane functions and the reasons for both shapes; runtime.hip: apply_noise decides when they run).
#include <hip/hip_runtime.h>
#include "noise_dev.h"
#include "kernels.h"

namespace j40hip {

__global__ __launch_bounds__(NOISE_FILL_THREADS) void k_noise_fill(float *raw, size_t pitch, size_t plane, NoiseFillArgs a, const uint64_t *__restrict__ sets) {
	noise_fill_lane(raw, pitch, plane, a, sets, (int32_t) blockIdx.x, (int32_t) threadIdx.x);
}

__global__ __launch_bounds__(NOISE_TILE_W * NOISE_WAVES) void k_noise_add(float *planes, size_t ppitch, size_t pplane, const float *__restrict__ raw, size_t pitch, size_t plane, int32_t W, int32_t H, NoiseParams p) {
	__shared__ float tile[NOISE_LDS_FLOATS];
	const int32_t tiles_x = (W + NOISE_TILE_W - 1) / NOISE_TILE_W, tx = (int32_t) blockIdx.x % tiles_x, ty = (int32_t) blockIdx.x / tiles_x;
	noise_tile_stage(tile, raw, pitch, plane, W, H, tx, ty, (int32_t) (threadIdx.y * NOISE_TILE_W + threadIdx.x));
	__syncthreads();
	noise_tile_lane(planes, ppitch, pplane, W, H, tile, p, tx, ty, (int32_t) threadIdx.x, (int32_t) threadIdx.y);
}

void launch_noise_fill(float *raw, const NoiseFillArgs &a, const uint64_t *sets_dev, hipStream_t stream) {
	if (a.W <= 0 || a.H <= 0 || a.gcols <= 0 || a.grows <= 0) return;
	const size_t pitch = noise_pitch(a.W);
	hipLaunchKernelGGL(k_noise_fill, dim3((unsigned) (a.gcols * a.grows)), dim3(NOISE_FILL_THREADS), 0, stream, raw, pitch, pitch * (size_t) a.H, a, sets_dev);
}

void launch_noise_add(float *planes, size_t ppitch, const float *raw, int32_t W, int32_t H, const NoiseParams &p, hipStream_t stream) {
	if (W <= 0 || H <= 0) return;
	const size_t pitch = noise_pitch(W);
	hipLaunchKernelGGL(k_noise_add, dim3((unsigned) ((W + NOISE_TILE_W - 1) / NOISE_TILE_W) * (unsigned) ((H + NOISE_TILE_H - 1) / NOISE_TILE_H)), dim3(NOISE_TILE_W, NOISE_WAVES), 0, stream,
		planes, ppitch, ppitch * (size_t) H, raw, pitch, pitch * (size_t) H, W, H, p);
}

} // namespace j40hip
