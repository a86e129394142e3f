// j40_amd/csrc/device/ycbcr_kernels.hip -- k_ycbcr_tail: the three float planes of a YCbCr VarDCT frame to RGBA (ycbcr_dev.h has the
// rules and the per-chunk code; runtime.hip: ycbcr_pixels decides when).
//
// Designed to be memory-bound (DESIGN.md section 5 has what was measured), no LDS: a lane makes four neighbouring pixels of a row.
// Y comes in as one 16-byte load; a chroma channel as one 16-byte load too where it is not shifted, else as four source samples of
// each of the one or two plane rows the four pixels lie between (neighbouring lanes ask for overlapping samples: the same cache
// lines). The pixels leave as one 16-byte non-temporal store (two for 16-bit output). Per pixel the algorithm needs 3 x 4 bytes
// read + 4 written = 16 bytes for 4:4:4 and 4 + 2 x 1 + 4 = 10 bytes for 4:2:0 (u8). A wavefront runs along a row: 256 pixels,
// 1 KiB of Y, 1 KiB of output. The shifts are launch arguments, uniform over the grid. Only pixels inside width x height are written.
#include <hip/hip_runtime.h>
#include "ycbcr_dev.h"
#include "kernels.h"

namespace j40hip {

template <bool OUT16>
__global__ __launch_bounds__(256) void k_ycbcr_tail(YcbcrTail t, uint8_t *rgba, size_t stride, int32_t y0) {
	const int32_t y = y0 + (int32_t) (blockIdx.y * blockDim.y + threadIdx.y), k = (int32_t) (blockIdx.x * blockDim.x + threadIdx.x);
	if (y >= t.height || 4 * k >= t.width) return;
	ycbcr_tail_chunk<OUT16>(t, (J40_GLOBAL uint8_t *) rgba + (size_t) y * stride, y, k);
}

void launch_ycbcr_tail(const YcbcrTail &t, uint8_t *rgba, size_t stride, hipStream_t stream, bool rgba16) {
	const int32_t slab = 4 * 65535;   // rows one launch covers (gridDim.y)
	for (int32_t y = 0; y < t.height; y += slab) {
		const int32_t rows = t.height - y < slab ? t.height - y : slab;
		const dim3 block(64, 4), grid((unsigned) (((t.width + 3) / 4 + 63) / 64), (unsigned) ((rows + 3) / 4));
		if (rgba16) hipLaunchKernelGGL(k_ycbcr_tail<true>, grid, block, 0, stream, t, rgba, stride, y);
		else hipLaunchKernelGGL(k_ycbcr_tail<false>, grid, block, 0, stream, t, rgba, stride, y);
	}
}

} // namespace j40hip
