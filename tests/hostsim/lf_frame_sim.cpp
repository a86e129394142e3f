// tests/hostsim/lf_frame_sim.cpp -- device/lf_frame_dev.h on the CPU (tests/test_lf_frames.py): the functions k_lf_from_frame and
// k_lf_frame_bctx run, over LfGroups laid out as frame.cpp lays them out and over the host plan of a parsed stream. Test infrastructure only.
#include <cstdint>
#include <cstring>
#include <vector>
#include <algorithm>
#include "../../j40_amd/csrc/plan_build.hpp"
#include "../../j40_amd/csrc/tables.hpp"
#include "../../j40_amd/csrc/device/lf_frame_dev.h"

using namespace j40hip;

#define LF_SIM_API extern "C" __attribute__((visibility("default")))

// the LfGroups of a W x H frame as the plan holds them: 2048 x 2048 pixels each, row by row, their cells one group behind the other
static std::vector<DevLfGroup> lay_out(int32_t W, int32_t H, size_t *cells) {
	std::vector<DevLfGroup> ggs;
	int32_t base = 0;
	for (int32_t y = 0; y < H; y += 2048) for (int32_t x = 0; x < W; x += 2048) {
		DevLfGroup g;
		memset(&g, 0, sizeof g);
		g.left = x; g.top = y; g.width = std::min(2048, W - x); g.height = std::min(2048, H - y);
		g.width8 = (g.width + 7) / 8; g.height8 = (g.height + 7) / 8; g.width64 = (g.width + 63) / 64; g.height64 = (g.height + 63) / 64;
		g.cell_base = base; base += g.width8 * g.height8;
		ggs.push_back(g);
	}
	*cells = (size_t) base;
	return ggs;
}

static void fill_args(LfFrameArgs *a, const float *src, int32_t w8, int32_t h8, const int32_t *nb_thr, const float *thr, float *out, size_t cells, uint8_t *lfidx) {
	memset(a, 0, sizeof *a);
	for (int c = 0; c < 3; ++c) {
		a->src[c] = src + (size_t) c * (size_t) w8 * (size_t) h8; a->out[c] = out + (size_t) c * cells;
		a->nb_thr[c] = nb_thr[c];
		for (int t = 0; t < 15; ++t) a->thr[c][t] = thr[c * 15 + t];
	}
	a->src_w = w8; a->src_h = h8; a->lfindices = lfidx;
}

// lf_from_frame_cell over every cell (and a few lanes past each LfGroup's end, as the grid has them) of a W x H frame. src: three
// planes of ceil(W / 8) x ceil(H / 8) floats; thr: [3][15]; out: three planes of `cells` floats in the cell layout; lfidx: `cells`
// bytes. Returns the number of cells, or -1 when out_cells is too small.
LF_SIM_API int64_t lfsim_gather(int32_t W, int32_t H, const float *src, const int32_t *nb_thr, const float *thr, float *out, uint8_t *lfidx, int64_t out_cells) {
	size_t cells = 0;
	const std::vector<DevLfGroup> ggs = lay_out(W, H, &cells);
	if ((int64_t) cells > out_cells) return -1;
	LfFrameArgs a;
	fill_args(&a, src, (W + 7) / 8, (H + 7) / 8, nb_thr, thr, out, cells, lfidx);
	for (const DevLfGroup &g : ggs) for (int32_t i = -3; i < g.width8 * g.height8 + 300; ++i) lf_from_frame_cell(g, i, a);
	return (int64_t) cells;
}

// a frame of a sequence parsed alone: the image header, then the headers of the coded frames up to row `k`
static uint32_t parse_row(const uint8_t *cs, size_t n, int k, ImageMeta *im, Frame *f, size_t *offset) {
	try {
		size_t at = 0;
		parse_image_header(cs, n, im, &at);
		for (int i = 0; i < k; ++i) { FrameHeader fh; Toc toc; parse_sequence_frame_header(cs, n, at, *im, false, true, &fh, &toc); at += toc.end_offset; }
		f->seq_im = im; f->allow_lf_frame = true; f->defer_lf_tail = true;
		parse_frame(cs + at, n - at, f, 1);
		*offset = at;
	} catch (const DecodeError &e) { return e.code; }
	return 0;
}

// The main frame (row `k`) of an LF-frame stream against its twin, the ordinary stream whose LF integers q are the flat LF frame's.
// out: [0] cells or varblocks whose layout, quantisation-field index, HfMul or sharpness differ between the two parses, [1] cells whose
// LF index, counted by lf_from_frame_cell on the samples (float) q * mult_lf, differs from the twin's (counted on q), [2] how many
// values the twin's LF index takes, [3] group blocks whose contexts, looked up again by lf_frame_bctx_block with those indices,
// differ from the twin's plan, [4] group blocks the second look-up changed, [5] cells whose gathered sample is not (float) q * mult_lf.
// Returns 0 or a 4-char code.
LF_SIM_API uint32_t lfsim_twin_check(const uint8_t *seq, size_t seq_size, int32_t k, const uint8_t *twin, size_t twin_size, int64_t *out) {
	for (int i = 0; i < 6; ++i) out[i] = 0;
	ImageMeta im;
	Frame fm, ft;
	size_t off = 0;
	if (uint32_t e = parse_row(seq, seq_size, k, &im, &fm, &off)) return e;
	try { ft.defer_lf_tail = true; parse_frame(twin, twin_size, &ft, 1); } catch (const DecodeError &e) { return e.code; }
	if (fm.lf_groups.size() != ft.lf_groups.size() || fm.fh.width != ft.fh.width || fm.fh.height != ft.fh.height) return 0x726e6765u;   // "rnge"
	HostPlan hm, ht;
	if (uint32_t e = build_vardct_plan(fm, seq + off, seq_size - off, &hm, 1, false)) return e;
	if (uint32_t e = build_vardct_plan(ft, twin, twin_size, &ht, 1, false)) return e;
	for (size_t g = 0; g < fm.lf_groups.size(); ++g) {
		const LfGroup &a = fm.lf_groups[g], &b = ft.lf_groups[g];
		if (a.blocks != b.blocks || a.sharpness != b.sharpness || a.xfromy != b.xfromy || a.bfromy != b.bfromy || a.varblocks.size() != b.varblocks.size()) { ++out[0]; continue; }
		for (size_t v = 0; v < a.varblocks.size(); ++v) {
			const VarblockInfo &x = a.varblocks[v], &y = b.varblocks[v];
			out[0] += x.coeffoff_qfidx != y.coeffoff_qfidx || x.hfmul_inv != y.hfmul_inv || x.x8 != y.x8 || x.y8 != y.y8 || x.dctsel != y.dctsel;
		}
		for (uint8_t v : a.lfindices) out[0] += v != 0;   // (the parse leaves them zero)
	}
	// the flat LF frame's picture: the twin's integers times its factors, frame-wide
	const int32_t w8 = (ft.fh.width + 7) / 8, h8 = (ft.fh.height + 7) / 8;
	const size_t cells = ht.blocks.size();
	std::vector<float> src((size_t) 3 * (size_t) w8 * (size_t) h8, 0.0f), lfs(3 * cells, 0.0f);
	for (const LfGroup &gg : ft.lf_groups) for (int c = 0; c < 3; ++c) for (int32_t y = 0; y < gg.height8; ++y) for (int32_t x = 0; x < gg.width8; ++x)
		src[((size_t) c * (size_t) h8 + (size_t) (gg.top / 8 + y)) * (size_t) w8 + (size_t) (gg.left / 8 + x)] = (float) gg.lfraw[c][(size_t) y * (size_t) gg.width8 + (size_t) x] * gg.mult_lf[c];
	int32_t nb_thr[3]; float thr[45] = {0};
	for (int c = 0; c < 3; ++c) {
		nb_thr[c] = fm.nb_lf_thr[c];
		const float mult_lf = fm.m_lf_scaled[c] / (float) (fm.global_scale * fm.quant_lf) * (float) 65536;   // (runtime.hip: lf_frame_tail)
		for (int t = 0; t < nb_thr[c]; ++t) thr[c * 15 + t] = (float) fm.lf_thr[c][t] * mult_lf;
	}
	std::vector<uint8_t> lfidx(cells, 0);
	LfFrameArgs a;
	fill_args(&a, src.data(), w8, h8, nb_thr, thr, lfs.data(), cells, lfidx.data());
	for (const DevLfGroup &g : hm.lf_groups) for (int32_t i = 0; i < g.width8 * g.height8; ++i) lf_from_frame_cell(g, i, a);
	bool seen[256] = {false};
	for (size_t i = 0; i < cells; ++i) { out[1] += lfidx[i] != ht.lfindices[i]; seen[ht.lfindices[i]] = true; }
	for (bool s : seen) out[2] += s;
	for (size_t g = 0; g < ft.lf_groups.size(); ++g) {
		const LfGroup &gg = ft.lf_groups[g];
		const DevLfGroup &d = ht.lf_groups[g];
		for (int c = 0; c < 3; ++c) for (size_t i = 0; i < gg.lfraw[c].size(); ++i) out[5] += lfs[(size_t) c * cells + (size_t) d.cell_base + i] != (float) gg.lfraw[c][i] * gg.mult_lf[c];
	}
	// the block contexts of the main frame's plan (built with LF index 0) looked up again
	DevPlan plan;
	memset(&plan, 0, sizeof plan);
	plan.frame = &hm.frame; plan.pool_u8 = hm.pool_u8.data(); plan.block_ctx_map_off = hm.block_ctx_map_off;
	plan.lf_groups = hm.lf_groups.data(); plan.sections = hm.sections.data(); plan.group_block_start = hm.group_block_start.data();
	std::vector<DevGroupBlock> blocks = hm.group_blocks;
	if (blocks.size() != ht.group_blocks.size()) return 0x726e6765u;
	for (int32_t g = 0; g < hm.frame.num_groups; ++g) for (uint32_t i = 0; i < 1024 + 7; ++i) lf_frame_bctx_block(plan, blocks.data(), lfidx.data(), g, i);
	for (size_t i = 0; i < blocks.size(); ++i) {
		out[3] += blocks[i].bctx3 != ht.group_blocks[i].bctx3 || blocks[i].coeffoff_qfidx != ht.group_blocks[i].coeffoff_qfidx || blocks[i].pos_dct != ht.group_blocks[i].pos_dct;
		out[4] += blocks[i].bctx3 != hm.group_blocks[i].bctx3;
	}
	return 0;
}
