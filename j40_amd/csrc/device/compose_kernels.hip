// j40_amd/csrc/device/compose_kernels.hip -- k_frame_compose and k_frame_blend: a frame of a sequence onto the canvas, in blend mode
// Replace and in the other four (compose_dev.h has the per-lane functions, runtime_seq.hip decides what runs). k_frame_blend reads the
// source inside the rectangle as well and does a few float32 operations a channel; everything else is alike. Shaped like k_region_crop: block (64, 4), 64 lanes along a row and 4 rows, a lane a
// 16-byte piece where the rows sit alike within 16 bytes, neighbouring lanes neighbouring pieces; every canvas pixel is written once and
// not read again here (non-temporal stores), every byte crosses HBM once in each direction. No LDS, no scratch.
#include <hip/hip_runtime.h>
#include <algorithm>
#include "compose_dev.h"
#include "kernels.h"

namespace j40hip {

// rows [y_first, y_first + rows) of the canvas. out, src: the canvas' first pixel in either image (src null: the empty pixel);
// frm: the frame's first pixel. only_rect: out is src, nothing outside the rectangle is touched
template <int PB>
__global__ __launch_bounds__(256) void k_frame_compose(uint8_t *out, size_t out_stride, const uint8_t *src, size_t src_stride, const uint8_t *frm, size_t frm_stride,
		int32_t W, int32_t y_first, int32_t rows, ComposeRect r, uint32_t lo, uint32_t hi, int32_t only_rect) {
	const int32_t i = (int32_t) (blockIdx.y * blockDim.y + threadIdx.y);
	if (i >= rows) return;
	const int32_t y = y_first + i;
	compose_row<PB>(out + (size_t) y * out_stride, src ? src + (size_t) y * src_stride : nullptr, frm, frm_stride, W, y, r, lo, hi, only_rect != 0,
		(int32_t) (blockIdx.x * 64 + threadIdx.x), (int32_t) (gridDim.x * 64));
}

// ... with the frame's span blended over the source's: cmode, amode are the colour channels' and the alpha's blend mode
template <int PB>
__global__ __launch_bounds__(256) void k_frame_blend(uint8_t *out, size_t out_stride, const uint8_t *src, size_t src_stride, const uint8_t *frm, size_t frm_stride,
		int32_t W, int32_t y_first, int32_t rows, ComposeRect r, uint32_t lo, uint32_t hi, int32_t only_rect, int32_t cmode, int32_t amode) {
	const int32_t i = (int32_t) (blockIdx.y * blockDim.y + threadIdx.y);
	if (i >= rows) return;
	const int32_t y = y_first + i;
	blend_row<PB>(out + (size_t) y * out_stride, src ? src + (size_t) y * src_stride : nullptr, frm, frm_stride, W, y, r, lo, hi, only_rect != 0, cmode, amode,
		(int32_t) (blockIdx.x * 64 + threadIdx.x), (int32_t) (gridDim.x * 64));
}

namespace {
// the launches that cover the canvas: all rows or, the output being the source, the rectangle's alone. fn(grid, block, first row, rows)
template <class Fn> void for_each_slab(bool only_rect, int32_t W, int32_t H, const ComposeRect &r, int32_t pixel_bytes, Fn fn) {
	const int32_t first = only_rect ? r.cy0 : 0, total = only_rect ? r.cy1 - r.cy0 : H;
	const int32_t span = only_rect ? r.cx1 - r.cx0 : W;   // the widest run of pixels a row moves
	if (total <= 0) return;
	const int32_t slab = 4 * 65535;   // rows one launch covers (gridDim.y)
	const int64_t pieces = (int64_t) span * pixel_bytes / 16 + 2;
	const unsigned gx = (unsigned) std::min<int64_t>((pieces + 63) / 64, 64);
	for (int32_t y = 0; y < total; y += slab) {
		const int32_t rows = total - y < slab ? total - y : slab;
		fn(dim3(gx, (unsigned) ((rows + 3) / 4)), dim3(64, 4), first + y, rows);
	}
}
}

void launch_frame_blend(uint8_t *out, size_t out_stride, const uint8_t *src, size_t src_stride, const uint8_t *frm, size_t frm_stride, int32_t W, int32_t H,
		int32_t x0, int32_t y0, int32_t w, int32_t h, uint32_t empty_lo, uint32_t empty_hi, int32_t pixel_bytes, int32_t cmode, int32_t amode, hipStream_t stream) {
	if (W <= 0 || H <= 0) return;
	const ComposeRect r = compose_clip(W, H, x0, y0, w, h);
	const int32_t only_rect = src == out;
	for_each_slab(only_rect, W, H, r, pixel_bytes, [&](dim3 grid, dim3 block, int32_t first, int32_t rows) {
		if (pixel_bytes == 8) hipLaunchKernelGGL(k_frame_blend<8>, grid, block, 0, stream, out, out_stride, src, src_stride, frm, frm_stride, W, first, rows, r, empty_lo, empty_hi, only_rect, cmode, amode);
		else hipLaunchKernelGGL(k_frame_blend<4>, grid, block, 0, stream, out, out_stride, src, src_stride, frm, frm_stride, W, first, rows, r, empty_lo, empty_hi, only_rect, cmode, amode);
	});
}

void launch_frame_compose(uint8_t *out, size_t out_stride, const uint8_t *src, size_t src_stride, const uint8_t *frm, size_t frm_stride, int32_t W, int32_t H,
		int32_t x0, int32_t y0, int32_t w, int32_t h, uint32_t empty_lo, uint32_t empty_hi, int32_t pixel_bytes, hipStream_t stream) {
	if (W <= 0 || H <= 0) return;
	const ComposeRect r = compose_clip(W, H, x0, y0, w, h);
	const int32_t only_rect = src == out;
	for_each_slab(only_rect, W, H, r, pixel_bytes, [&](dim3 grid, dim3 block, int32_t first, int32_t rows) {
		if (pixel_bytes == 8) hipLaunchKernelGGL(k_frame_compose<8>, grid, block, 0, stream, out, out_stride, src, src_stride, frm, frm_stride, W, first, rows, r, empty_lo, empty_hi, only_rect);
		else hipLaunchKernelGGL(k_frame_compose<4>, grid, block, 0, stream, out, out_stride, src, src_stride, frm, frm_stride, W, first, rows, r, empty_lo, empty_hi, only_rect);
	});
}

} // namespace j40hip
