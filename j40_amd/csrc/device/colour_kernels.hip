// j40_amd/csrc/device/colour_kernels.hip -- the colour tail of the colour mode (j40hip_frame_set_colour; colour_dev.h has the lane's work,
// colour_space.hpp the host's half, DESIGN.md section 4 the reasoning).
//
//   k_colour_tail<TF, OUT16>   three float planes (X, Y, B: what an OutMode::XYB launch, the restoration filters or k_modular_to_xyb leave)
//                              -> linear values in the signalled primaries -> the signalled transfer curve -> u8x4 / u16x4, A opaque.
//                              Streaming: 12 bytes in, 4 / 8 out per pixel, nontemporal stores. A workgroup of 256 takes 64 x 4 pixels, a
//                              lane one pixel, as k_xyb_to_rgba does on the same planes (their rows are `width` floats apart: no wider
//                              aligned access exists for odd widths). 8-bit frames: the frame's threshold table staged in LDS (up to
//                              7 KB), no curve evaluated. Other depths: the curve in float64 (colour_dev.h) -- PQ, the dearest, is
//                              ~250 double-rate instructions a pixel, of the order of the time its 20 bytes take from and to HBM.
//
// Compiled with -ffp-contract=off like every kernel.
#include <hip/hip_runtime.h>
#include "colour_dev.h"
#include "kernels.h"

namespace j40hip {

template <int TF, bool OUT16>
__global__ void __launch_bounds__(256) k_colour_tail(ColourPlanes in, ColourTailParams p, int32_t width, int32_t height, uint8_t *out, size_t stride_bytes) {
	__shared__ float s_thr[COLOUR_TABLE_FLOATS];
	const bool use_table = p.cc.bpp == 8 && p.table_floats > 0;
	if (use_table) for (int32_t i = (int32_t) threadIdx.x; i < p.table_floats && i < COLOUR_TABLE_FLOATS; i += 256) s_thr[i] = p.table[i];
	__syncthreads();
	const int32_t x = (int32_t) (blockIdx.x * 64 + (threadIdx.x & 63));
	if (x >= width) return;
	for (int32_t y = (int32_t) (blockIdx.y * 4 + (threadIdx.x >> 6)); y < height; y += (int32_t) gridDim.y * 4) {
		const size_t i = (size_t) y * in.pitch + (size_t) x;
		const uint64_t px = colour_tail_pixel<TF, OUT16>(in.p[0][i], in.p[1][i], in.p[2][i], p.cc, p.curve, use_table, (const J40_LDS float *) s_thr, p.blo, p.bhi);
		if constexpr (OUT16) __builtin_nontemporal_store(px, (uint64_t *) (out + (size_t) y * stride_bytes + (size_t) x * 8));
		else __builtin_nontemporal_store((uint32_t) px, (uint32_t *) (out + (size_t) y * stride_bytes + (size_t) x * 4));
	}
}

template <int TF>
static void launch_colour_tail_of(const ColourPlanes &in, const ColourTailParams &p, int32_t width, int32_t height, uint8_t *out, size_t stride, hipStream_t stream, bool rgba16) {
	const int32_t rows = (height + 3) / 4;
	const dim3 grid((unsigned) ((width + 63) / 64), (unsigned) (rows < 65535 ? rows : 65535));
	if (rgba16) hipLaunchKernelGGL((k_colour_tail<TF, true>), grid, dim3(256), 0, stream, in, p, width, height, out, stride);
	else hipLaunchKernelGGL((k_colour_tail<TF, false>), grid, dim3(256), 0, stream, in, p, width, height, out, stride);
}

// `xyb`: three planes of width x height floats, `pitch` floats per row, one behind the other (launch_xyb_to_rgba's layout)
void launch_colour_tail(const float *xyb, size_t pitch, const ColourTailParams &p, int32_t width, int32_t height, uint8_t *out, size_t stride_bytes, hipStream_t stream, bool rgba16) {
	if (width <= 0 || height <= 0) return;
	ColourPlanes q; for (int c = 0; c < 3; ++c) q.p[c] = xyb + (size_t) c * pitch * (size_t) height; q.pitch = pitch;
	switch (p.curve.tf) {
	case CTF_LINEAR: launch_colour_tail_of<CTF_LINEAR>(q, p, width, height, out, stride_bytes, stream, rgba16); break;
	case CTF_SRGB: launch_colour_tail_of<CTF_SRGB>(q, p, width, height, out, stride_bytes, stream, rgba16); break;
	case CTF_BT709: launch_colour_tail_of<CTF_BT709>(q, p, width, height, out, stride_bytes, stream, rgba16); break;
	case CTF_GAMMA: launch_colour_tail_of<CTF_GAMMA>(q, p, width, height, out, stride_bytes, stream, rgba16); break;
	case CTF_PQ: launch_colour_tail_of<CTF_PQ>(q, p, width, height, out, stride_bytes, stream, rgba16); break;
	default: launch_colour_tail_of<CTF_HLG>(q, p, width, height, out, stride_bytes, stream, rgba16); break;
	}
}

} // namespace j40hip
