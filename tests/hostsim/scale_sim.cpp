// tests/hostsim/scale_sim.cpp -- reduced-size decode on the CPU (tests/test_scale.py): device/scale_dev.h's row function, the one
// k_downscale runs, lane by lane over an image in host memory: without a device. The fused pixel kernels use the same accumulator and
// division (ScaleAcc), so what holds here holds for their arithmetic.
#include <cstdint>
#include <cstring>
#include "../../j40_amd/csrc/device/scale_dev.h"

using namespace j40hip;

#define SCALE_SIM_API extern "C" __attribute__((visibility("default")))

// what launch_downscale launches: every output row, `lanes` lanes a row. pixel_bytes: 4 (u8x4) or 8 (u16x4)
SCALE_SIM_API void scale_sim(uint8_t *out, size_t out_stride, const uint8_t *src, size_t src_stride, int32_t W, int32_t H, int32_t k, int32_t pixel_bytes, int32_t lanes) {
	const int32_t oh = scale_out_size(H, k);
	for (int32_t j = 0; j < oh; ++j) for (int32_t lane = 0; lane < lanes; ++lane) {
		if (pixel_bytes == 8) scale_row<8>(src, src_stride, out + (size_t) j * out_stride, W, H, k, j, lane, lanes);
		else scale_row<4>(src, src_stride, out + (size_t) j * out_stride, W, H, k, j, lane, lanes);
	}
}

// out3: the output size of a W x H frame at shift k and the pixels of cell (i, j)
SCALE_SIM_API void scale_sim_cell(int32_t W, int32_t H, int32_t k, int32_t i, int32_t j, int32_t *out3) {
	out3[0] = scale_out_size(W, k); out3[1] = scale_out_size(H, k); out3[2] = scale_span(i, W, k) * scale_span(j, H, k);
}
