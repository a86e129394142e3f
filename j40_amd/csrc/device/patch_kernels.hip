// j40_amd/csrc/device/patch_kernels.hip -- k_patch_blend: the placements of a frame's patch dictionary onto its XYB planes, one
// workgroup per non-empty tile (patch_dev.h has the lane's walk and the reasons for the shape; runtime.hip: apply_patches decides when
// it runs). Block (64, 4): 64 lanes along a row of the tile, four wavefronts four rows apart. LDS: one chunk of records, 2 KB.
#include <hip/hip_runtime.h>
#include "patch_dev.h"
#include "kernels.h"

namespace j40hip {

__global__ __launch_bounds__(256) void k_patch_blend(float *planes, int32_t W, int32_t H, DevPatches p, PatchSlots slots) {
	__shared__ PatchRec recs[PATCH_CHUNK];
	const int32_t b = (int32_t) blockIdx.x, t = (int32_t) (threadIdx.y * 64 + threadIdx.x);
	const int32_t first = p.offsets[b];
	patch_tile_lane(planes, W, H, p, slots, b, (int32_t) threadIdx.x, (int32_t) threadIdx.y, recs, [&](int32_t at, int32_t n) {
		if (at != first) __syncthreads();   // (every lane has done with the chunk before)
		if (t < n) recs[t] = p.recs[p.index[at + t]];
		__syncthreads();
	});
}

void launch_patch_blend(float *planes, int32_t W, int32_t H, const DevPatches &p, const PatchSlots &slots, hipStream_t stream) {
	if (p.num_tiles <= 0 || W <= 0 || H <= 0) return;
	hipLaunchKernelGGL(k_patch_blend, dim3((unsigned) p.num_tiles), dim3(64, PATCH_WAVES), 0, stream, planes, W, H, p, slots);
}

} // namespace j40hip
