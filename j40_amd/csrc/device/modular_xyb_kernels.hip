// j40_amd/csrc/device/modular_xyb_kernels.hip -- a Modular frame of an XYB image through the XYB colour tail (j40hip_frame_set_modular_xyb;
// modular_xyb_dev.h has the rule and the lane's work, DESIGN.md section 4 the reasoning).
//
//   k_modular_xyb_pack<S, RGBA16>   integer planes (S = int16_t / int32_t) -> XYB floats in registers -> linear -> sRGB -> u8x4 / u16x4, alpha
//                                   from its plane or opaque, over the whole frame or a rectangle of it; one pass, nothing in between
//                                   is written. Streaming: 6 / 8 bytes in (12 / 16 wide), 4 / 8 out per pixel. A workgroup of 256 takes
//                                   256 x 4 pixels, a lane 4 consecutive pixels of a row (8- or 16-byte loads, 16-byte nontemporal
//                                   stores); LDS: the sRGB threshold table, as in the VarDCT pixel kernels.
//   k_modular_to_xyb<S>             the three float planes alone (X, Y, B): LF slots of a sequence, j40hip_frame_read_xyb.
//
// Compiled with -ffp-contract=off like every kernel.
#include <hip/hip_runtime.h>
#include "modular_xyb_dev.h"
#include "modular_dev.h"
#include "kernels.h"

namespace j40hip {

__device__ float c_mxyb_srgb_thr[SRGB_TABLE_FLOATS];

void upload_modular_xyb_tables(const float *srgb_thr, hipStream_t stream) {
	(void) hipMemcpyToSymbolAsync(HIP_SYMBOL(c_mxyb_srgb_thr), srgb_thr, sizeof(float) * SRGB_TABLE_FLOATS, 0, hipMemcpyHostToDevice, stream);
}

template <typename S, bool RGBA16>
__global__ void __launch_bounds__(256) k_modular_xyb_pack(const S *c0, const S *c1, const S *c2, const S *a, ModXybRect r, ModXybConsts k, uint8_t *rgba, size_t stride_bytes) {
	__shared__ float s_thr[SRGB_TABLE_FLOATS];
	for (int32_t i = threadIdx.x; i < SRGB_TABLE_FLOATS; i += blockDim.x) s_thr[i] = c_mxyb_srgb_thr[i];
	__syncthreads();
	const int32_t lx = (int32_t) (blockIdx.x * MODXYB_LANES_X + (threadIdx.x & (MODXYB_LANES_X - 1))), ly = (int32_t) (blockIdx.y * MODXYB_ROWS + threadIdx.x / MODXYB_LANES_X);
	modular_xyb_pack_lane<S, RGBA16>(c0, c1, c2, a, r, lx, ly, k, (const J40_LDS float *) s_thr, rgba, stride_bytes);
}

struct ModXybOut { float *p[3]; };
struct ModXybFactors { float m[3]; };   // (the planes need nothing of the colour tail's)
template <typename S>
__global__ void __launch_bounds__(256) k_modular_to_xyb(const S *c0, const S *c1, const S *c2, ModXybRect r, ModXybFactors k, ModXybOut out, size_t pitch) {
	const int32_t lx = (int32_t) (blockIdx.x * MODXYB_LANES_X + (threadIdx.x & (MODXYB_LANES_X - 1))), ly = (int32_t) (blockIdx.y * MODXYB_ROWS + threadIdx.x / MODXYB_LANES_X);
	modular_to_xyb_lane<S>(c0, c1, c2, r, lx, ly, k.m, out.p, pitch);
}

// A alone, by the pack kernels' own functions (modular_dev.h), into pixels another kernel has written opaque: behind k_colour_tail on a
// Modular XYB frame under the colour mode (runtime.hip), and the known-answer hook's two-kernel route
template <typename S, bool RGBA16>
__global__ void __launch_bounds__(256) k_kat_alpha_from_plane(const S *a, int32_t width, int32_t height, int32_t bpp, uint8_t *rgba, size_t stride_bytes) {
	const int32_t x = (int32_t) (blockIdx.x * 64 + (threadIdx.x & 63)), y = (int32_t) (blockIdx.y * 4 + (threadIdx.x >> 6));
	if (x >= width || y >= height) return;
	const int32_t v = a[(size_t) y * (size_t) width + (size_t) x];
	if constexpr (RGBA16) ((uint16_t *) (rgba + (size_t) y * stride_bytes))[(size_t) x * 4 + 3] = (uint16_t) (pack_rgba16(0, 0, 0, v, bpp) >> 48);
	else (rgba + (size_t) y * stride_bytes)[(size_t) x * 4 + 3] = (uint8_t) (pack_rgba8(0, 0, 0, v, bpp) >> 24);
}
void launch_alpha_from_plane(PlanePtr a, int32_t width, int32_t height, int32_t bpp, uint8_t *rgba, size_t stride, hipStream_t stream, bool rgba16) {
	const dim3 grid((unsigned) ((width + 63) / 64), (unsigned) ((height + 3) / 4));
	if (a.wide()) {
		if (rgba16) hipLaunchKernelGGL((k_kat_alpha_from_plane<int32_t, true>), grid, dim3(256), 0, stream, (const int32_t *) a.p, width, height, bpp, rgba, stride);
		else hipLaunchKernelGGL((k_kat_alpha_from_plane<int32_t, false>), grid, dim3(256), 0, stream, (const int32_t *) a.p, width, height, bpp, rgba, stride);
	} else {
		if (rgba16) hipLaunchKernelGGL((k_kat_alpha_from_plane<int16_t, true>), grid, dim3(256), 0, stream, (const int16_t *) a.p, width, height, bpp, rgba, stride);
		else hipLaunchKernelGGL((k_kat_alpha_from_plane<int16_t, false>), grid, dim3(256), 0, stream, (const int16_t *) a.p, width, height, bpp, rgba, stride);
	}
}

static dim3 modxyb_grid(int32_t rw, int32_t rh) {
	const int32_t per_wg = MODXYB_LANES_X * MODXYB_PX;
	return dim3((unsigned) ((rw + per_wg - 1) / per_wg), (unsigned) ((rh + MODXYB_ROWS - 1) / MODXYB_ROWS));
}

enum { MODXYB_SLAB = MODXYB_ROWS * 65535 };   // rows one launch covers (gridDim.y)

template <typename S>
static void launch_modxyb_pack_of(const S *c0, const S *c1, const S *c2, const S *a, const ModXybRect &whole, const ModXybConsts &k, uint8_t *rgba, size_t stride, hipStream_t stream, bool rgba16) {
	for (int32_t y = 0; y < whole.rh; y += MODXYB_SLAB) {
		const ModXybRect r = {whole.plane_width, whole.x0, whole.y0 + y, whole.rw, whole.rh - y < MODXYB_SLAB ? whole.rh - y : MODXYB_SLAB};
		if (rgba16) hipLaunchKernelGGL((k_modular_xyb_pack<S, true>), modxyb_grid(r.rw, r.rh), dim3(256), 0, stream, c0, c1, c2, a, r, k, rgba, stride);
		else hipLaunchKernelGGL((k_modular_xyb_pack<S, false>), modxyb_grid(r.rw, r.rh), dim3(256), 0, stream, c0, c1, c2, a, r, k, rgba, stride);
	}
}
void launch_modular_xyb_pack_rect(PlanePtr c0, PlanePtr c1, PlanePtr c2, PlanePtr a, int32_t plane_width, int32_t x0, int32_t y0, int32_t rw, int32_t rh, const ModXybConsts &k, uint8_t *rgba, size_t stride, hipStream_t stream, bool rgba16) {
	if (rw <= 0 || rh <= 0) return;
	const ModXybRect r = {plane_width, x0, y0, rw, rh};
	if (c0.wide()) launch_modxyb_pack_of((const int32_t *) c0.p, (const int32_t *) c1.p, (const int32_t *) c2.p, (const int32_t *) a.p, r, k, rgba, stride, stream, rgba16);
	else launch_modxyb_pack_of((const int16_t *) c0.p, (const int16_t *) c1.p, (const int16_t *) c2.p, (const int16_t *) a.p, r, k, rgba, stride, stream, rgba16);
}
void launch_modular_xyb_pack(PlanePtr c0, PlanePtr c1, PlanePtr c2, PlanePtr a, int32_t width, int32_t height, const ModXybConsts &k, uint8_t *rgba, size_t stride, hipStream_t stream, bool rgba16) {
	launch_modular_xyb_pack_rect(c0, c1, c2, a, width, 0, 0, width, height, k, rgba, stride, stream, rgba16);
}
void launch_modular_to_xyb(PlanePtr c0, PlanePtr c1, PlanePtr c2, int32_t plane_width, int32_t x0, int32_t y0, int32_t rw, int32_t rh, const ModXybConsts &k, float *x, float *y, float *b, size_t pitch, hipStream_t stream) {
	if (rw <= 0 || rh <= 0) return;
	for (int32_t s = 0; s < rh; s += MODXYB_SLAB) {
		const ModXybRect r = {plane_width, x0, y0 + s, rw, rh - s < MODXYB_SLAB ? rh - s : MODXYB_SLAB};
		const size_t off = (size_t) s * pitch;
		const ModXybOut out = {{x + off, y + off, b + off}};
		const ModXybFactors f = {{k.m[0], k.m[1], k.m[2]}};
		if (c0.wide()) hipLaunchKernelGGL(k_modular_to_xyb<int32_t>, modxyb_grid(rw, r.rh), dim3(256), 0, stream, (const int32_t *) c0.p, (const int32_t *) c1.p, (const int32_t *) c2.p, r, f, out, pitch);
		else hipLaunchKernelGGL(k_modular_to_xyb<int16_t>, modxyb_grid(rw, r.rh), dim3(256), 0, stream, (const int16_t *) c0.p, (const int16_t *) c1.p, (const int16_t *) c2.p, r, f, out, pitch);
	}
}

} // namespace j40hip
