// j40_amd/csrc/device/alpha_kernels.hip -- k_alpha_merge: the kept alpha channel of a VarDCT frame into pixels the pixel kernels have
// written opaque (alpha_dev.h has the rule and the per-chunk code; runtime.hip: merge_alpha decides when).
//
// It runs behind the pixel kernels and the extra channels' Modular decode on the same stream. A lane takes four neighbouring pixels:
// one 16-byte load of RGBA (two for 16-bit output), one 8-byte load of four int16 samples, one 16-byte store (two). That is
// 4 + 2 + 4 = 10 bytes of HBM traffic a pixel (u8), 18 (u16); a wavefront covers 1 KiB (2 KiB) of one row. The caller's rows are only
// pixel-aligned, so the pixels in front of a row's first 16-byte boundary and behind its last whole chunk are written by one more
// lane of the row, A sample by A sample.
#include <hip/hip_runtime.h>
#include "alpha_dev.h"
#include "kernels.h"

namespace j40hip {

// rectangle (x0, y0, w, h) of the frame; plane: the frame-wide alpha samples, `pitch` of them a row
template <bool OUT16>
__global__ __launch_bounds__(256) void k_alpha_merge(uint8_t *rgba, size_t stride, const int16_t *plane, int32_t pitch,
		int32_t x0, int32_t y0, int32_t w, int32_t h, AlphaScale s) {
	const int32_t y = (int32_t) (blockIdx.y * blockDim.y + threadIdx.y), k = (int32_t) (blockIdx.x * blockDim.x + threadIdx.x);
	if (y >= h) return;
	J40_GLOBAL uint8_t *row = (J40_GLOBAL uint8_t *) rgba + (size_t) (y0 + y) * stride + (size_t) x0 * (OUT16 ? 8 : 4);
	const J40_GLOBAL int16_t *alpha = (const J40_GLOBAL int16_t *) plane + (size_t) (y0 + y) * (size_t) pitch + (size_t) x0;
	const int32_t head = alpha_row_head<OUT16>((uintptr_t) row, w), chunks = (w - head) / 4;
	if (k < chunks) alpha_merge_chunk<OUT16>(row, alpha, head, k, s);
	else if (k == chunks) alpha_merge_edges<OUT16>(row, alpha, head, w, s);
}

void launch_alpha_merge(const int16_t *plane, int32_t pitch, int32_t x0, int32_t y0, int32_t w, int32_t h, int32_t bpp, uint8_t *rgba, size_t stride, hipStream_t stream, bool rgba16) {
	if (w <= 0 || h <= 0) return;
	const AlphaScale s = alpha_scale_make(bpp, rgba16);
	const int32_t slab = 4 * 65535;   // rows one launch covers (gridDim.y)
	for (int32_t y = 0; y < h; y += slab) {
		const int32_t rows = h - y < slab ? h - y : slab;
		const dim3 block(64, 4), grid((unsigned) ((w / 4 + 1 + 63) / 64), (unsigned) ((rows + 3) / 4));
		if (rgba16) hipLaunchKernelGGL(k_alpha_merge<true>, grid, block, 0, stream, rgba, stride, plane, pitch, x0, y0 + y, w, rows, s);
		else hipLaunchKernelGGL(k_alpha_merge<false>, grid, block, 0, stream, rgba, stride, plane, pitch, x0, y0 + y, w, rows, s);
	}
}

} // namespace j40hip
