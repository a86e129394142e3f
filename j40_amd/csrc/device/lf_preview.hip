// j40_amd/csrc/device/lf_preview.hip -- the LF preview: the 1:8 image every VarDCT frame carries in its LfGroup sections, one XYB
// sample per 8x8 cell, through the full decode's colour tail into RGBA (include/j40hip.h: j40hip_frame_decode_lf).
//
//   k_lf_preview<MODE>   one lane per cell, the whole tail fused: the cell's LF integers (its 3x3 neighbourhood where it is smoothed)
//                        -> dequantisation (j40.h:6562) -> adaptive smoothing inside the LfGroup (lf_smooth_dev.h, the stencil
//                        k_lf_dequant_smooth uses) -> LF chroma from luma (j40.h:7158, 7170) -> XYB -> linear -> sRGB -> level -> u8x4 or u16x4 (idct_dev.h, the pixel kernels'
//                        xyb_to_rgba8 / xyb_to_rgba16, sRGB thresholds in LDS). Consecutive lanes take consecutive cells of an LfGroup's
//                        rows, so the 4- or 8-byte stores of a wavefront are contiguous. The grid is a flat list of (frame, LfGroup, 256
//                        cells) workgroups: one launch serves any number of frames. MODE LFP_PLANE writes one channel's dequantised,
//                        smoothed sample as a float instead (j40hip_frame_read_lf).
//
// Each cell reads 6 bytes (plus the neighbours its workgroup mostly has in cache) and writes 4 or 8: an 8K frame is 518 400 cells.
// Compiled with -ffp-contract=off like every kernel: the float path keeps the reference's operation order.
#include <hip/hip_runtime.h>
#include "entropy_dev.h"
#include "idct_dev.h"
#include "lf_smooth_dev.h"
#include "kernels.h"

namespace j40hip {

__device__ float c_lfp_srgb_thr[SRGB_TABLE_FLOATS];

void upload_lf_preview_tables(const float *srgb_thr, hipStream_t stream) {
	(void) hipMemcpyToSymbolAsync(HIP_SYMBOL(c_lfp_srgb_thr), srgb_thr, sizeof(float) * SRGB_TABLE_FLOATS, 0, hipMemcpyHostToDevice, stream);
}

template <int MODE> __global__ void __launch_bounds__(LFP_LANES) k_lf_preview(const DevLfpFrame *frames, const DevLfpWork *work, int32_t nwork, int32_t channel) {
	__shared__ float s_thr[MODE == LFP_PLANE ? 1 : SRGB_TABLE_FLOATS];
	if (MODE != LFP_PLANE) {
		for (int32_t i = threadIdx.x; i < SRGB_TABLE_FLOATS; i += blockDim.x) s_thr[i] = c_lfp_srgb_thr[i];
		__syncthreads();
	}
	// this workgroup's item: the last one that starts at or before it (every item has at least one workgroup)
	int32_t lo = 0, hi = nwork - 1;
	while (lo < hi) {
		const int32_t mid = (lo + hi + 1) >> 1;
		if (work[mid].first_block <= blockIdx.x) lo = mid; else hi = mid - 1;
	}
	const DevLfpWork wk = work[lo];
	const DevLfpFrame &f = frames[wk.frame];
	const DevLfpGroup g = f.groups[wk.group];
	const int32_t i = (int32_t) (blockIdx.x - wk.first_block) * LFP_LANES + (int32_t) threadIdx.x;
	if (i >= g.width8 * g.height8) return;
	const int32_t y = i / g.width8, x = i - y * g.width8;
	const size_t at = (size_t) g.cell_base + (size_t) i;
	float v[3];
	const bool edge = !f.smooth || g.width8 < 3 || g.height8 < 3 || y == 0 || x == 0 || y == g.height8 - 1 || x == g.width8 - 1;
	if (edge) {
		for (int c = 0; c < 3; ++c) v[c] = (float) f.lfraw[c][at] * g.mult_lf[c];
	} else {
		lf_smooth_interior(f.lfraw, at, g.width8, g.mult_lf, f.inv_m_lf, v);
	}
	if (MODE != LFP_PLANE) {   // chroma from luma on the LF sample, as the reference does to the LLF coefficients (j40.h:7158, 7170)
		v[0] = v[0] + v[1] * f.kx_lf;
		v[2] = v[2] + v[1] * f.kb_lf;
	}
	uint8_t *row = f.out + (size_t) (g.y8 + y) * (size_t) f.stride;
	const int32_t col = g.x8 + x;
	if (MODE == LFP_PLANE) {
		((float *) row)[col] = channel == 0 ? v[0] : channel == 1 ? v[1] : v[2];
		return;
	}
	ColourConsts cc;
	for (int k = 0; k < 3; ++k) { cc.cbrt_opsin_bias[k] = f.cbrt_opsin_bias[k]; cc.opsin_bias[k] = f.opsin_bias[k]; }
	for (int k = 0; k < 9; ++k) cc.m[k] = f.opsin_inv_mat[k];
	cc.itscale = f.itscale; cc.bpp = f.bpp;
	const J40_LDS float *thr = (const J40_LDS float *) s_thr;
	if (MODE == LFP_U16) ((uint64_t *) row)[col] = xyb_to_rgba16(v[0], v[1], v[2], cc, thr);
	else ((uint32_t *) row)[col] = xyb_to_rgba8(v[0], v[1], v[2], cc, thr);
}

void launch_lf_preview(const DevLfpFrame *frames, const DevLfpWork *work, int32_t nwork, uint32_t nblocks, int32_t mode, int32_t channel, hipStream_t stream) {
	if (nwork <= 0 || nblocks == 0) return;
	if (mode == LFP_U16) hipLaunchKernelGGL(k_lf_preview<LFP_U16>, dim3(nblocks), dim3(LFP_LANES), 0, stream, frames, work, nwork, channel);
	else if (mode == LFP_PLANE) hipLaunchKernelGGL(k_lf_preview<LFP_PLANE>, dim3(nblocks), dim3(LFP_LANES), 0, stream, frames, work, nwork, channel);
	else hipLaunchKernelGGL(k_lf_preview<LFP_U8>, dim3(nblocks), dim3(LFP_LANES), 0, stream, frames, work, nwork, channel);
}

} // namespace j40hip
