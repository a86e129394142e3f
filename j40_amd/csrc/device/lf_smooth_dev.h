// j40_amd/csrc/device/lf_smooth_dev.h -- adaptive LF smoothing of one interior 8x8 cell (j40__smooth_lf, j40.h:6492-6540): a 3x3
// stencil over the UNSMOOTHED dequantised samples of the cell's LfGroup, three channels at once because the blend factor is shared
// (j40.h:6517-6529). One statement for the LfGroup tail (lf_tail_kernels.hip: k_lf_dequant_smooth) and the LF preview (lf_preview.hip).
// Float arithmetic in the reference's order (-ffp-contract=off).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace j40hip {

// lfraw[c][at]: the cell's integer in channel c (X, Y, B) of planes w8 cells wide, m[c]: the LfGroup's dequantisation factor; out[c]:
// the smoothed sample. Interior cells only: edge cells (and frames that skip the smoothing) pass through as lfraw[c][at] * m[c].
__device__ __forceinline__ void lf_smooth_interior(const int16_t *const lfraw[3], size_t at, int32_t w8, const float m[3], const float inv_m_lf[3], float out[3]) {
	const float W0 = 0.05226273532324128f, W1 = 0.20345139757231578f, W2 = 0.0334829185968739f;
	float wa[3], centre[3], gap = 0.5f;
	for (int c = 0; c < 3; ++c) {
		const int16_t *q = lfraw[c] + at;
		const float mc = m[c];
		const float n0 = (float) q[-w8 - 1] * mc, n1 = (float) q[-w8] * mc, n2 = (float) q[-w8 + 1] * mc;
		const float l0 = (float) q[-1] * mc, l1 = (float) q[0] * mc, l2 = (float) q[1] * mc;
		const float s0 = (float) q[w8 - 1] * mc, s1 = (float) q[w8] * mc, s2 = (float) q[w8 + 1] * mc;
		wa[c] = (n0 * W2 + n1 * W1 + n2 * W2) + (l0 * W1 + l1 * W0 + l2 * W1) + (s0 * W2 + s1 * W1 + s2 * W2);
		centre[c] = l1;
		const float diff = fabsf(wa[c] - l1) * inv_m_lf[c];
		if (gap < diff) gap = diff;
	}
	gap = 3.0f - 4.0f * gap;
	gap = 0.0f > gap ? 0.0f : gap;
	for (int c = 0; c < 3; ++c) out[c] = (wa[c] - centre[c]) * gap + centre[c];
}

} // namespace j40hip
