// tests/hostsim/ycbcr_sim.cpp -- TEST INFRASTRUCTURE ONLY. YCbCr VarDCT frames on the CPU (tests/test_ycbcr.py): the host parser with
// YCbCr frames asked for, the plan, the device functions of the entropy decode (hf_dev.h, with its subsampled form), of the pixel
// stage and of the tail (ycbcr_dev.h: what k_ycbcr_tail runs), with the runtime's orchestration -- without a device. Transforms up
// to 64 x 64 (what the streams of the tests hold).
#include <cstdint>
#include <cstring>
#include <cmath>
#include <vector>
#include <algorithm>
#include "../../j40_amd/csrc/plan_build.hpp"
#include "../../j40_amd/csrc/tables.hpp"
#include "../../j40_amd/csrc/device/hf_dev.h"
#include "../../j40_amd/csrc/device/vardct_dev.h"
#include "../../j40_amd/csrc/device/special8_dev.h"
#include "../../j40_amd/csrc/device/ycbcr_dev.h"

using namespace j40hip;

#define YCBCR_SIM_API extern "C" __attribute__((visibility("default")))

namespace {

template <int N> void idct_rows(float *tile, int rows, int pitch, const float *hs) {
	for (int r = 0; r < rows; ++r) { float x[N]; for (int k = 0; k < N; ++k) x[k] = tile[r * pitch + k]; Idct1D<N>::run(x, hs); for (int k = 0; k < N; ++k) tile[r * pitch + k] = x[k]; }
}
template <int N> void idct_cols(float *tile, int cols, int pitch, const float *hs) {
	for (int c = 0; c < cols; ++c) { float x[N]; for (int k = 0; k < N; ++k) x[k] = tile[k * pitch + c]; Idct1D<N>::run(x, hs); for (int k = 0; k < N; ++k) tile[k * pitch + c] = x[k]; }
}
void idct_rows_dyn(float *t, int n, int rows, int pitch, const float *hs) {
	switch (n) { case 8: idct_rows<8>(t, rows, pitch, hs); break; case 16: idct_rows<16>(t, rows, pitch, hs); break; case 32: idct_rows<32>(t, rows, pitch, hs); break; default: idct_rows<64>(t, rows, pitch, hs); }
}
void idct_cols_dyn(float *t, int n, int cols, int pitch, const float *hs) {
	switch (n) { case 8: idct_cols<8>(t, cols, pitch, hs); break; case 16: idct_cols<16>(t, cols, pitch, hs); break; case 32: idct_cols<32>(t, cols, pitch, hs); break; default: idct_cols<64>(t, cols, pitch, hs); }
}

struct Parsed {
	Frame fr;
	const uint8_t *cs = nullptr; size_t cs_size = 0; std::vector<uint8_t> storage;
};
uint32_t parse(const uint8_t *buf, size_t size, bool allow, Parsed *p) {
	try {
		p->fr.allow_ycbcr = allow;
		extract_codestream(buf, size, &p->cs, &p->cs_size, &p->storage);
		parse_frame(p->cs, p->cs_size, &p->fr, 1);
	} catch (const DecodeError &e) { return e.code; }
	return 0;
}
uint32_t shifts_of(const FrameHeader &fh) {
	uint32_t s = 0;
	for (int c = 0; c < 3; ++c) s |= (uint32_t) (fh.hshift[c] | fh.vshift[c] << 1) << (2 * c);
	return s;
}
void plane_dims(const FrameHeader &fh, int32_t pw[3], int32_t ph[3]) {
	if (fh.subsampled()) ycc_plane_dims(fh.width, fh.height, shifts_of(fh), pw, ph);
	else for (int c = 0; c < 3; ++c) { pw[c] = fh.width; ph[c] = fh.height; }
}

} // namespace

// the tail alone over caller planes: what launch_ycbcr_tail launches, row by row and chunk by chunk. dims: {pitch, width, height} of
// planes 0..2, shifts: {hshift, vshift} of each. 0, or 1 when the arguments are out of range
YCBCR_SIM_API int32_t ycbcr_sim_tail(const float *p0, const float *p1, const float *p2, const int32_t *dims, const int32_t *shifts, int32_t W, int32_t H, int32_t bpp, int32_t out16, uint8_t *out, size_t stride) {
	YcbcrTail t;
	const float *p[3] = {p0, p1, p2};
	for (int c = 0; c < 3; ++c) { t.plane[c] = p[c]; t.pitch[c] = dims[3 * c]; t.pw[c] = dims[3 * c + 1]; t.ph[c] = dims[3 * c + 2]; t.hshift[c] = shifts[2 * c]; t.vshift[c] = shifts[2 * c + 1]; }
	t.width = W; t.height = H;
	if (!ycbcr_tail_valid(t) || bpp < 8 || bpp > 15) return 1;
	ycbcr_tail_scale(&t, bpp, out16 != 0);
	for (int32_t y = 0; y < H; ++y) for (int32_t k = 0; 4 * k < W; ++k) {
		if (out16) ycbcr_tail_chunk<true>(t, out + (size_t) y * stride, y, k);
		else ycbcr_tail_chunk<false>(t, out + (size_t) y * stride, y, k);
	}
	return 0;
}

// what the parser makes of a stream: out[0] the parse's code (allow: YCbCr frames asked for), [1] do_ycbcr, [2..7] (hshift, vshift) of
// Cb, Y, Cr, [8..13] (width, height) of the three planes, [14] width, [15] height, [16] what ycbcr_scope says, [17..20] width8,
// height8, width64, height64 of LfGroup 0, [21] what build_vardct_plan says with the switch on, [22] ... and off
YCBCR_SIM_API void ycbcr_sim_info(const uint8_t *buf, size_t size, int32_t allow, int32_t *out) {
	for (int i = 0; i < 24; ++i) out[i] = 0;
	Parsed p;
	out[0] = (int32_t) parse(buf, size, allow != 0, &p);
	if (out[0]) return;
	const FrameHeader &fh = p.fr.fh;
	out[1] = fh.do_ycbcr;
	for (int c = 0; c < 3; ++c) { out[2 + 2 * c] = fh.hshift[c]; out[3 + 2 * c] = fh.vshift[c]; }
	int32_t pw[3], ph[3];
	plane_dims(fh, pw, ph);
	for (int c = 0; c < 3; ++c) { out[8 + 2 * c] = pw[c]; out[9 + 2 * c] = ph[c]; }
	out[14] = fh.width; out[15] = fh.height;
	out[16] = (int32_t) ycbcr_scope(p.fr);
	if (!fh.is_modular && !p.fr.lf_groups.empty()) { const LfGroup &gg = p.fr.lf_groups[0]; out[17] = gg.width8; out[18] = gg.height8; out[19] = gg.width64; out[20] = gg.height64; }
	if (!fh.is_modular) {
		HostPlan hp, hq;
		out[21] = (int32_t) build_vardct_plan(p.fr, p.cs, p.cs_size, &hp, 1, true);
		out[22] = (int32_t) build_vardct_plan(p.fr, p.cs, p.cs_size, &hq, 1, false);
	}
}

// The whole decode with the switch on: planes[c] (tightly packed, the size ycbcr_sim_info reports) as the tail reads them, and the
// pixels (width x height, `stride` bytes a row; out16: u16x4). Returns the frame's code. A frame that is not YCbCr (a twin coded
// without do_ycbcr) leaves the same planes and no pixels: what the pixel kernels' OutMode::XYB stores.
// (`dense`: the plan without coefficient events, the form the runtime uploads again after "evof" -- a section whose events do not fit
// their region or a coefficient beyond int16, as every coefficient of a jpegdata= stream is)
static uint32_t decode_with(const Parsed &p, bool dense, float *plane0, float *plane1, float *plane2, uint8_t *rgba, size_t stride, int32_t out16) {
	const Frame &fr = p.fr;
	if (fr.fh.is_modular) return ERR_TODO;
	HostPlan hp;
	hp.force_dense = dense;
	if (uint32_t e = build_vardct_plan(fr, p.cs, p.cs_size, &hp, 1, true)) return e;
	std::vector<float> coeff_store(3 * hp.coeff_floats, 0.0f);
	std::vector<int8_t> nonzeros((size_t) hp.frame.num_groups * 32 * 32 * 3);
	std::vector<uint32_t> status(hp.sections.size(), 0);
	std::vector<int32_t> window(hp.lz_window_size ? (size_t) hp.frame.num_groups * hp.lz_window_size : 0);
	DevPlan plan;
	memset(&plan, 0, sizeof plan);
	plan.frame = &hp.frame; plan.codestream = hp.codestream.data();
	plan.pool_u8 = hp.pool_u8.data(); plan.pool_u16 = hp.pool_u16.data(); plan.pool_i32 = hp.pool_i32.data(); plan.pool_u64 = hp.pool_u64.data(); plan.pool_f32 = hp.pool_f32.data();
	plan.clusters = hp.clusters.data(); plan.coeff_specs = hp.coeff_specs.data(); plan.lf_groups = hp.lf_groups.data(); plan.sections = hp.sections.data();
	plan.block_ctx_map_off = hp.block_ctx_map_off;
	plan.group_blocks = hp.group_blocks.data(); plan.group_block_start = hp.group_block_start.data();
	plan.blocks = hp.blocks.data(); plan.lfindices = hp.lfindices.data();
	for (int c = 0; c < 3; ++c) { plan.llf[c] = hp.llf[c].data(); plan.coeffs[c] = coeff_store.data() + (size_t) c * hp.coeff_floats; }
	plan.coeff_stride = (uint32_t) hp.coeff_floats;
	std::vector<CoeffEvent> events(hp.ev_capacity + 1);
	std::vector<uint32_t> block_events(4 * hp.group_blocks.size() + 4, 0);
	if (hp.frame.sparse_coeffs) { plan.events = events.data(); plan.ev_range = hp.ev_range.data(); plan.block_events = block_events.data(); }
	plan.vb_coeffoff_qfidx = hp.vb_coeffoff_qfidx.data(); plan.vb_hfmul_inv = hp.vb_hfmul_inv.data();
	plan.xfromy = hp.xfromy.data(); plan.bfromy = hp.bfromy.data();
	plan.nonzeros = nonzeros.data(); plan.status = status.data();
	plan.lz_window = window.empty() ? nullptr : window.data(); plan.lz_window_size = hp.lz_window_size;
	std::vector<uint32_t> end_bits(status.size(), 0);
	plan.section_end_bit = hp.frame.sections_have_trailer ? end_bits.data() : nullptr;
	for (int32_t g = 0; g < hp.frame.num_groups; ++g) decode_hf_group(plan, g, false);
	{
		uint32_t first = 0, first_off = 0xffffffffu;
		for (size_t i = 0; i < status.size(); ++i) if (status[i] && hp.sections[i].byte_off < first_off) { first = status[i]; first_off = hp.sections[i].byte_off; }
		if (first) return first;
	}
	int32_t pw[3], ph[3];
	plane_dims(fr.fh, pw, ph);
	float *planes[3] = {plane0, plane1, plane2};
	const bool sub = fr.fh.subsampled();
	const float *hs = half_secants(), *afv = afv_basis();
	const DevFrame &f = hp.frame;
	std::vector<float> A(3 * 65536), scratch(SP8_TILE), scratch2(SP8_TILE);
	for (const DevVarblock &vb : hp.vb_sorted) {
		const int log_rows = DEV_DCT_SELECT[vb.dctsel][0], log_columns = DEV_DCT_SELECT[vb.dctsel][1];
		if (log_rows > 6 || log_columns > 6) return ERR_TODO;
		const int R = 1 << log_rows, C = 1 << log_columns, sz = R * C;
		const int long_side = R > C ? R : C, vh8 = (R < C ? R : C) / 8, vw8 = long_side / 8;
		static const int8_t PARAM[27] = {0, 1, 2, 3, 4, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 10, 10, 11, 12, 12, 13, 14, 14, 15, 16, 16};
		const float *dq = plan.pool_f32 + f.dq_off[PARAM[vb.dctsel]];
		const VbGeom g = varblock_geometry(plan, vb);
		const bool special = (vb.dctsel >= 1 && vb.dctsel <= 3) || (vb.dctsel >= 12 && vb.dctsel <= 17);
		const int P = special ? SP8_PITCH : C + 1;
		if (f.sparse_coeffs) {
			for (int ch = 0; ch < 3; ++ch) std::fill(A.begin() + (size_t) ch * 65536, A.begin() + (size_t) ch * 65536 + std::min<size_t>(65536, (size_t) R * (size_t) P), 0.0f);
			const TileMap map = {R, C, P, special ? 1 : 0};
			const uint16_t *order = plan.pool_u16 + f.order_off[DEV_DCT_SELECT[vb.dctsel][2] * 3];
			const uint32_t *be = plan.block_events + 4 * (size_t) vb.blk;
			tile_scatter_events(plan, g, be, order, plan.pool_f32 + f.dq_scan_off[PARAM[vb.dctsel]], sz, map, A.data(), 65536, f.quant_bias, f.quant_bias_num, 0, 1);
			tile_fill_llf(plan, g, long_side, vh8, vw8, map, A.data(), 65536, f.kx_lf, f.kb_lf, 0, 1);
		} else for (int i = 0; i < sz; ++i) {
			float v[3];
			load_coeff3(plan, g, dq, sz, i, long_side, vh8, vw8, v);
			int r, c;
			if (special) { r = i / 8; c = i % 8; }
			else { r = C > R ? i / C : i % R; c = C > R ? i % C : i / R; }
			for (int ch = 0; ch < 3; ++ch) A[(size_t) ch * 65536 + r * P + c] = v[ch];
		}
		for (int ch = 0; ch < 3; ++ch) {
			float *t = A.data() + (size_t) ch * 65536;
			if (special) {
				for (int l = 0; l < 8; ++l) special8_phase0(vb.dctsel, l, (const float *) t, scratch.data(), hs, afv, false);
				for (int l = 0; l < 8; ++l) special8_phase1(vb.dctsel, l, (const float *) scratch.data(), scratch2.data(), hs, false);
				memcpy(t, scratch2.data(), sizeof(float) * SP8_TILE);
			} else { idct_rows_dyn(t, C, R, P, hs); idct_cols_dyn(t, R, C, P, hs); }
		}
		if (!sub) {   // OutMode::XYB: the visible samples to the frame's planes
			for (int y = 0; y < g.effh; ++y) for (int x = 0; x < g.effw; ++x) for (int ch = 0; ch < 3; ++ch)
				planes[ch][(size_t) (g.py + y) * (size_t) pw[ch] + (size_t) (g.px + x)] = A[(size_t) ch * 65536 + y * P + x];
		} else {      // OutMode::YCC (kernels.hip: store_ycc): the whole block, where the channel has one, at its plane's own position
			const int32_t bx = g.px >> 3, by = g.py >> 3;
			for (int ch = 0; ch < 3; ++ch) {
				const int32_t hsft = fr.fh.hshift[ch], vsft = fr.fh.vshift[ch];
				if ((bx & hsft) || (by & vsft)) continue;
				for (int y = 0; y < 8; ++y) for (int x = 0; x < 8; ++x)
					planes[ch][(size_t) (((by >> vsft) << 3) + y) * (size_t) pw[ch] + (size_t) (((bx >> hsft) << 3) + x)] = A[(size_t) ch * 65536 + y * P + x];
			}
		}
	}
	if (!fr.fh.do_ycbcr || !rgba) return 0;
	int32_t dims[9], shifts[6];
	for (int c = 0; c < 3; ++c) { dims[3 * c] = pw[c]; dims[3 * c + 1] = pw[c]; dims[3 * c + 2] = ph[c]; shifts[2 * c] = fr.fh.hshift[c]; shifts[2 * c + 1] = fr.fh.vshift[c]; }
	return ycbcr_sim_tail(plane0, plane1, plane2, dims, shifts, fr.fh.width, fr.fh.height, fr.im.bpp, out16, rgba, stride) ? (uint32_t) ERR_RNGE : 0;
}

YCBCR_SIM_API uint32_t ycbcr_sim_decode(const uint8_t *buf, size_t size, float *plane0, float *plane1, float *plane2, uint8_t *rgba, size_t stride, int32_t out16) {
	Parsed p;
	if (uint32_t e = parse(buf, size, true, &p)) return e;
	const uint32_t e = decode_with(p, false, plane0, plane1, plane2, rgba, stride, out16);
	return e == (uint32_t) ERR_EVOF ? decode_with(p, true, plane0, plane1, plane2, rgba, stride, out16) : e;
}
