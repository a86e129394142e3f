// j40_amd/csrc/device/orient_kernels.hip -- k_orient: a pixel-aligned RGBA image in device memory written out in the image's orientation
// (orient_dev.h has the arithmetic; runtime.hip: decode_oriented decides what runs). Orientations 2 to 4 keep rows rows: k_orient_rows,
// shaped like k_downscale -- block (64, 4), 64 lanes along an output row and 4 rows; a wavefront loads one contiguous run of a source row
// and stores one contiguous run of an output row. Orientations 5 to 8 turn rows into columns: k_orient_tiles moves one 32 x 32 tile per
// block of 256 lanes through LDS, so that the global loads run along source rows and the global stores along output rows; the tile's
// rows are padded by a pixel, which makes the column-wise LDS reads conflict-free for 4- and for 8-byte pixels.
#include <hip/hip_runtime.h>
#include <algorithm>
#include "orient_dev.h"
#include "kernels.h"

namespace j40hip {

// dst: output row `j0`'s first pixel; rows: output rows this launch covers
template <int PB, bool ALIGNED>
__global__ __launch_bounds__(256) void k_orient_rows(const uint8_t *src, size_t src_stride, uint8_t *dst, size_t dst_stride, int32_t W, int32_t H, int32_t o, int32_t j0, int32_t rows) {
	const int32_t r = (int32_t) (blockIdx.y * blockDim.y + threadIdx.y);
	if (r >= rows) return;
	orient_row<PB, ALIGNED>(src, src_stride, dst + (size_t) r * dst_stride, W, H, o, j0 + r, (int32_t) (blockIdx.x * 64 + threadIdx.x), (int32_t) (gridDim.x * 64));
}

// the tile (tx0 + blockIdx.x, ty0 + blockIdx.y) of the source image; dst: the output's first pixel
template <int PB, bool ALIGNED>
__global__ __launch_bounds__(ORIENT_LANES) void k_orient_tiles(const uint8_t *src, size_t src_stride, uint8_t *dst, size_t dst_stride, int32_t W, int32_t H, int32_t o, int32_t tx0, int32_t ty0) {
	__shared__ typename OrientPixel<PB>::type tile[ORIENT_TILE_PIXELS];
	const int32_t sx0 = (tx0 + (int32_t) blockIdx.x) * ORIENT_TILE, sy0 = (ty0 + (int32_t) blockIdx.y) * ORIENT_TILE, lane = (int32_t) threadIdx.x;
	orient_tile_load<PB>(tile, src, src_stride, W, H, sx0, sy0, lane);
	__syncthreads();
	orient_tile_store<PB, ALIGNED>(tile, dst, dst_stride, W, H, o, sx0, sy0, lane);
}

void launch_orient(const uint8_t *src, size_t src_stride, uint8_t *dst, size_t dst_stride, int32_t W, int32_t H, int32_t orientation, int32_t pixel_bytes, hipStream_t stream) {
	if (W <= 0 || H <= 0 || !orient_valid(orientation)) return;
	// the output's pixels all sit on multiples of their size, or (a caller's odd pointer or stride) are stored byte by byte
	const bool aligned = (uintptr_t) dst % (size_t) pixel_bytes == 0 && dst_stride % (size_t) pixel_bytes == 0;
	if (!orient_transposes(orientation)) {
		const int32_t slab = 4 * 65535;   // rows one launch covers (gridDim.y)
		const unsigned gx = (unsigned) std::min<int32_t>((W + 63) / 64, 64);
		for (int32_t j = 0; j < H; j += slab) {
			const int32_t rows = H - j < slab ? H - j : slab;
			const dim3 block(64, 4), grid(gx, (unsigned) ((rows + 3) / 4));
			uint8_t *d = dst + (size_t) j * dst_stride;
			if (pixel_bytes == 8) { if (aligned) hipLaunchKernelGGL((k_orient_rows<8, true>), grid, block, 0, stream, src, src_stride, d, dst_stride, W, H, orientation, j, rows); else hipLaunchKernelGGL((k_orient_rows<8, false>), grid, block, 0, stream, src, src_stride, d, dst_stride, W, H, orientation, j, rows); }
			else { if (aligned) hipLaunchKernelGGL((k_orient_rows<4, true>), grid, block, 0, stream, src, src_stride, d, dst_stride, W, H, orientation, j, rows); else hipLaunchKernelGGL((k_orient_rows<4, false>), grid, block, 0, stream, src, src_stride, d, dst_stride, W, H, orientation, j, rows); }
		}
		return;
	}
	// tiles: a launch takes at most 2^20 columns of them (gridDim.x * blockDim.x stays below 2^32) and 65535 rows (gridDim.y)
	const int32_t tiles_x = (int32_t) (((int64_t) W + ORIENT_TILE - 1) / ORIENT_TILE), tiles_y = (int32_t) (((int64_t) H + ORIENT_TILE - 1) / ORIENT_TILE);
	for (int32_t ty = 0; ty < tiles_y; ty += 65535) for (int32_t tx = 0; tx < tiles_x; tx += 1 << 20) {
		const dim3 block(ORIENT_LANES), grid((unsigned) std::min<int32_t>(tiles_x - tx, 1 << 20), (unsigned) std::min<int32_t>(tiles_y - ty, 65535));
		if (pixel_bytes == 8) { if (aligned) hipLaunchKernelGGL((k_orient_tiles<8, true>), grid, block, 0, stream, src, src_stride, dst, dst_stride, W, H, orientation, tx, ty); else hipLaunchKernelGGL((k_orient_tiles<8, false>), grid, block, 0, stream, src, src_stride, dst, dst_stride, W, H, orientation, tx, ty); }
		else { if (aligned) hipLaunchKernelGGL((k_orient_tiles<4, true>), grid, block, 0, stream, src, src_stride, dst, dst_stride, W, H, orientation, tx, ty); else hipLaunchKernelGGL((k_orient_tiles<4, false>), grid, block, 0, stream, src, src_stride, dst, dst_stride, W, H, orientation, tx, ty); }
	}
}

} // namespace j40hip
