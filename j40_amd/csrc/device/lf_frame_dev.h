// j40_amd/csrc/device/lf_frame_dev.h -- the LF image of a frame with use_lf_frame (include/j40hip.h, J40HIP_SEQ_LFFRAME): its LF samples
// are the picture of an LF frame decoded before it instead of quantised integers of its own. Compiled for the device by
// lf_tail_kernels.hip (k_lf_from_frame, k_lf_frame_bctx) and for the CPU by tests/hostsim/lf_frame_sim.cpp: the same functions.
//
//   lf_from_frame_cell    one cell of an LfGroup: the three samples of the LF frame's planes at the cell's frame-wide position go to
//                         the LfGroup tail's LF planes (what k_lf_dequant_smooth writes for every other frame: no factor, no smoothing),
//                         and the cell's LF index is counted on them. PARITY UNPINNED (the reference refuses such frames, j40.h:6763):
//                         channel c counts the thresholds t with sample > (float) t * mult_lf[c], mult_lf at extra_precision 0 -- for a
//                         sample that is an integer q times mult_lf exactly the q > t of j40.h:6566-6570 --, combined as frame.cpp
//                         (lf_group_finish) combines them
//   block_ctx3            the three block contexts of a varblock (j40.h:6951-6953) from its order, quantisation-field index and the LF
//                         index of its top-left cell: one statement for the device plan builder (plan_dev.h) and lf_frame_bctx_block
//   lf_frame_bctx_block   the plan was built before any LF sample existed, with LF index 0 everywhere: one block's contexts again
#pragma once
#include "hf_dev.h"

namespace j40hip {

J40_DEV uint8_t lf_frame_index(const LfFrameArgs &a, float x, float y, float b) {
	uint8_t idx = 0;   // 8-bit arithmetic like frame.cpp
	for (int32_t t = 0; t < a.nb_thr[0]; ++t) idx = (uint8_t) (idx + (x > a.thr[0][t]));
	idx = (uint8_t) (idx * (a.nb_thr[0] + 1));
	for (int32_t t = 0; t < a.nb_thr[2]; ++t) idx = (uint8_t) (idx + (b > a.thr[2][t]));
	idx = (uint8_t) (idx * (a.nb_thr[2] + 1));
	for (int32_t t = 0; t < a.nb_thr[1]; ++t) idx = (uint8_t) (idx + (y > a.thr[1][t]));
	return idx;
}

// cell i of LfGroup gg (row by row, gg.width8 a row)
J40_DEV void lf_from_frame_cell(const DevLfGroup &gg, int32_t i, const LfFrameArgs &a) {
	const int32_t w8 = gg.width8, h8 = gg.height8;
	if (i < 0 || i >= w8 * h8) return;
	const int32_t y = i / w8, x = i - y * w8;
	const int32_t sx = gg.left / 8 + x, sy = gg.top / 8 + y;
	if (sx >= a.src_w || sy >= a.src_h) return;   // (cannot happen once the sizes agree)
	const size_t from = (size_t) sy * (size_t) a.src_w + (size_t) sx, at = (size_t) gg.cell_base + (size_t) i;
	const float vx = a.src[0][from], vy = a.src[1][from], vb = a.src[2][from];
	a.out[0][at] = vx; a.out[1][at] = vy; a.out[2][at] = vb;
	a.lfindices[at] = lf_frame_index(a, vx, vy, vb);
}

// block_ctx_map[((c_yxb * 13 + order) * nb_qf1 + qfidx) * lfidx_size + lfidx] of channels Y, X, B at bits 0, 4, 8
J40_DEV uint32_t block_ctx3(const uint8_t *map, int32_t order_idx, int32_t qfidx, int32_t lfidx, int32_t nb_qf1, int32_t lfidx_size) {
	const int32_t bctx0 = (order_idx * nb_qf1 + qfidx) * lfidx_size + lfidx;
	uint32_t b3 = 0;
	for (int32_t c_yxb = 0; c_yxb < 3; ++c_yxb) b3 |= (uint32_t) (map[bctx0 + 13 * nb_qf1 * lfidx_size * c_yxb] & 15) << (4 * c_yxb);
	return b3;
}

// block k of group g's list (DevPlan::group_blocks); bits 12-14 of bctx3 stay
J40_DEV void lf_frame_bctx_block(const DevPlan &plan, DevGroupBlock *blocks, const uint8_t *lfindices, int32_t g, uint32_t k) {
	const uint32_t first = plan.group_block_start[g], end = plan.group_block_start[g + 1];
	if (k >= end - first) return;
	const DevSection &sec = plan.sections[g];   // (pass 0's: the geometry is every pass')
	const DevLfGroup &gg = plan.lf_groups[sec.ggidx];
	DevGroupBlock &gb = blocks[first + k];
	const int32_t x8 = gb.pos_dct & 31, y8 = (gb.pos_dct >> 5) & 31, dctsel = gb.pos_dct >> 10;
	const size_t cell = (size_t) gg.cell_base + (size_t) (sec.gy8 + y8) * (size_t) gg.width8 + (size_t) (sec.gx8 + x8);
	const DevFrame &fr = *plan.frame;
	const uint32_t b3 = block_ctx3(plan.pool_u8 + plan.block_ctx_map_off, DEV_DCT_SELECT[dctsel][2], (int32_t) (gb.coeffoff_qfidx & 15u), lfindices[cell], fr.nb_qf_thr + 1, fr.lfidx_size);
	gb.bctx3 = (uint16_t) ((gb.bctx3 & 0x7000u) | b3);
}

} // namespace j40hip
