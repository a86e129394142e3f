// j40_amd/csrc/device/scale_kernels.hip -- k_downscale: a full-size RGBA image in device memory made 1:2 or 1:4 (scale_dev.h has the
// arithmetic; runtime.hip: decode_scaled decides what runs). It serves the reduced-size decodes whose pixels come out of other kernels
// than the fused pixel kernels: restoration filters in force (k_xyb_to_rgba) and keep-alpha mode on a single frame (k_alpha_merge).
// Shaped like k_region_crop: block (64, 4), 64 lanes along an output row and 4 rows, a lane an output pixel; a lane reads its cell's
// rows in 8- or 16-byte pieces where they sit on such boundaries, so a wavefront reads whole runs of s source rows and every byte of the
// full image crosses HBM once.
#include <hip/hip_runtime.h>
#include <algorithm>
#include "scale_dev.h"
#include "kernels.h"

namespace j40hip {

// src: the full image's first pixel; dst: output row `j0`'s first pixel; rows: output rows this launch covers
template <int PB>
__global__ __launch_bounds__(256) void k_downscale(const uint8_t *src, size_t src_stride, uint8_t *dst, size_t dst_stride, int32_t W, int32_t H, int32_t k, int32_t j0, int32_t rows) {
	const int32_t r = (int32_t) (blockIdx.y * blockDim.y + threadIdx.y);
	if (r >= rows) return;
	scale_row<PB>(src, src_stride, dst + (size_t) r * dst_stride, W, H, k, j0 + r, (int32_t) (blockIdx.x * 64 + threadIdx.x), (int32_t) (gridDim.x * 64));
}

void launch_downscale(const uint8_t *src, size_t src_stride, uint8_t *dst, size_t dst_stride, int32_t W, int32_t H, int32_t shift, int32_t pixel_bytes, hipStream_t stream) {
	if (W <= 0 || H <= 0) return;
	const int32_t ow = scale_out_size(W, shift), oh = scale_out_size(H, shift);
	const int32_t slab = 4 * 65535;   // rows one launch covers (gridDim.y)
	const unsigned gx = (unsigned) std::min<int32_t>((ow + 63) / 64, 64);
	for (int32_t j = 0; j < oh; j += slab) {
		const int32_t rows = oh - j < slab ? oh - j : slab;
		const dim3 block(64, 4), grid(gx, (unsigned) ((rows + 3) / 4));
		if (pixel_bytes == 8) hipLaunchKernelGGL(k_downscale<8>, grid, block, 0, stream, src, src_stride, dst + (size_t) j * dst_stride, dst_stride, W, H, shift, j, rows);
		else hipLaunchKernelGGL(k_downscale<4>, grid, block, 0, stream, src, src_stride, dst + (size_t) j * dst_stride, dst_stride, W, H, shift, j, rows);
	}
}

} // namespace j40hip
