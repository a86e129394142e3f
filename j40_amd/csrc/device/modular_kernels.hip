// j40_amd/csrc/device/modular_kernels.hip -- HIP kernels of the Modular path for gfx950.
//
//   k_modular_sections   K3: per-pixel MA-tree walk + prediction + entropy decode, one section
//                        (LfGlobal's channel data or one group rectangle) per wavefront
//                        (replaces j40__modular_channel, j40.h:4127, as driven by j40__lf_global,
//                        j40.h:6334, and j40__pass_group, j40.h:7024-7033)
//   k_inverse_rct        K4: inverse reversible colour transform, one lane per pixel (j40.h:4318)
//   k_inverse_palette*   K4: palette look-up (one lane per pixel) or, with delta prediction, the
//                        serial form (j40.h:4402)
//   k_unsqueeze_h/_v     K4: one inverse Squeeze step (ISO 18181-1; squeeze_dev.h): an average and a residual channel
//                        joined along rows / columns. The recurrence runs along the squeezed axis, lines across it are
//                        independent: one lane per line, rows staged through LDS so that HBM sees whole 128-byte pieces
//   k_pack_planes        K5: int16 planes -> clamped RGBA u8x4 (j40.h:7910)
//
// Integer work throughout: results are bit-exact with the reference.
#include <hip/hip_runtime.h>
#include "modular_dev.h"
#include "squeeze_dev.h"
#include "scale_dev.h"
#include "kernels.h"

namespace j40hip {

// One section per wavefront, one wavefront per workgroup. Every lane runs the same (wave-uniform) decoder, so the serial
// per-pixel loop lives on the scalar unit like k_hf_entropy's. IN_LDS: the MA tree, the code spec's tables, the three most
// recent rows of the channel being decoded and the weighted predictor's error rows all live in LDS (the usual case; the
// template keeps their address space static, a run-time choice would turn every access into a flat one), so the tree
// walk, the symbol decode and the neighbour fetch wait on LDS instead of L2 -- a sample that was just stored to the plane is
// not in the vector L1, and the previous pixel is the next one's W neighbour.
// S: the planes' sample type (modular_dev.h); the wide form's weighted-predictor rows are 64-bit cells (wp_width counts samples)
template <bool IN_LDS, typename S = int16_t>
__global__ void __launch_bounds__(64) k_modular_sections(DevModPlan plan, int32_t first_section, int32_t rows_width, int32_t wp_width) {
	extern __shared__ __attribute__((aligned(16))) uint8_t mod_lds[];
	const int32_t lane = threadIdx.x;
	const int32_t s = first_section + (int32_t) blockIdx.x;
	const DevModSection &msec = plan.sections[s];
	if (msec.coop_idx >= 0 || msec.split) return;   // k_modular_coop's, modular_split.hip's
	if (msec.preset_status) { if (lane == 0) plan.status[s] = msec.preset_status; return; }
	const DevCodeSpec &spec = plan.spec[msec.spec_idx];
	ModTables t = mod_tables_in_hbm(plan, s);
	if (IN_LDS) {
		auto align16 = [](uint32_t v) { return (v + 15u) & ~15u; };
		const int32_t tree_nodes = msec.tree_nodes;
		uint32_t off = 0;
		DevTreeNode *l_tree = (DevTreeNode *) mod_lds; off = align16((uint32_t) tree_nodes * (uint32_t) sizeof(DevTreeNode));
		uint32_t *l_map = (uint32_t *) (mod_lds + off); off = align16(off + (uint32_t) spec.num_dist + 4);
		DevCluster *l_clusters = (DevCluster *) (mod_lds + off); off = align16(off + (uint32_t) spec.num_clusters * (uint32_t) sizeof(DevCluster));
		uint8_t *l_tab = mod_lds + off; off = align16(off + (spec.use_prefix_code ? 4u : 8u) * spec.table_span);
		int32_t *l_rows = (int32_t *) (mod_lds + off); off = align16(off + 12u * (uint32_t) rows_width);   // rows_width = widest rectangle + 4 spare entries
		int32_t *l_wp = (int32_t *) (mod_lds + off);
		{ const uint4 *src = (const uint4 *) (plan.tree + msec.tree_off); uint4 *dst = (uint4 *) l_tree; for (int32_t i = lane; i < tree_nodes; i += 64) dst[i] = src[i]; }
		{ const uint32_t *src = (const uint32_t *) (plan.pool_u8 + spec.cluster_map_off); for (int32_t i = lane; i < (spec.num_dist + 3) / 4; i += 64) l_map[i] = src[i]; }   // 4-byte aligned table (plan_build.cpp)
		const DevCluster *csrc = plan.clusters + spec.cluster_off;
		const uint32_t base_off = csrc[0].table_off;
		for (int32_t i = lane; i < spec.num_clusters; i += 64) { DevCluster c = csrc[i]; c.table_off -= base_off; l_clusters[i] = c; }
		if (spec.use_prefix_code) { const int32_t *src = plan.pool_i32 + base_off; int32_t *dst = (int32_t *) l_tab; for (uint32_t i = lane; i < spec.table_span; i += 64) dst[i] = src[i]; }
		else { const uint64_t *src = plan.pool_u64 + base_off; uint64_t *dst = (uint64_t *) l_tab; for (uint32_t i = lane; i < spec.table_span; i += 64) dst[i] = src[i]; }
		t.tree = l_tree; t.cluster_map = (const uint8_t *) l_map; t.clusters = l_clusters; t.alias = (const uint64_t *) l_tab; t.prefix = (const int32_t *) l_tab;
		t.rows = l_rows; t.rows_width = rows_width;
		if (wp_width) { t.wp_errors = l_wp; t.wp_errors_width = wp_width; }
		__syncthreads();
	}
	const uint32_t err = decode_modular_section<true, IN_LDS, S>(plan, t, s);
	if (lane == 0) plan.status[s] = err;
}

// one workgroup per section that lists transforms of its own; runs after K3 (kernel boundary = the planes are visible)
template <typename S>
__global__ void __launch_bounds__(256) k_section_inverse_rcts(DevModPlan plan, int32_t first_section) {
	section_inverse_rcts<S>(plan, first_section + (int32_t) blockIdx.x, (int32_t) threadIdx.x, 256);
}

// rows of a tightly packed sub-image plane over a rectangle of a frame plane (j40__combine_modular_from_pass_group, j40.h:3688)
template <typename S>
__global__ void __launch_bounds__(256) k_paste_plane(const S *src, int32_t w, size_t n, S *dst, int32_t dst_stride) {
	for (size_t i = (size_t) blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t) gridDim.x * blockDim.x) {
		const size_t y = i / (size_t) w, x = i - y * (size_t) w;
		dst[y * (size_t) dst_stride + x] = src[i];
	}
}

template <typename S>
__global__ void __launch_bounds__(256) k_inverse_rct(S *a, S *b, S *c, size_t n, int32_t type7) {
	for (size_t i = (size_t) blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t) gridDim.x * blockDim.x) {
		S p0 = a[i], p1 = b[i], p2 = c[i];
		inverse_rct_pixel(type7, p0, p1, p2);
		a[i] = p0; b[i] = p1; c[i] = p2;
	}
}

// output channel i of a palette without delta prediction; dst may alias idx (last channel, in place)
template <typename S>
__global__ void __launch_bounds__(256) k_inverse_palette_plain(const S *idx, const S *palrow, S *dst, size_t n, int32_t i, int32_t nb_colours, int32_t bpp) {
	for (size_t k = (size_t) blockIdx.x * blockDim.x + threadIdx.x; k < n; k += (size_t) gridDim.x * blockDim.x)
		dst[k] = palette_value(idx[k], i, palrow, nb_colours, bpp);
}

// palette with delta prediction: a delta entry is added to a prediction from already reconstructed
// neighbours of the same output channel, which makes the channel strictly sequential (j40.h:4469-4476)
template <typename S>
__global__ void __launch_bounds__(64) k_inverse_palette_predicted(const S *idx, const S *pal, int32_t pal_stride, S *const *dst, int32_t num_c,
		int32_t width, int32_t height, int32_t nb_colours, int32_t nb_deltas, int32_t d_pred, int32_t bpp, const int8_t *wpp, int32_t *wp_scratch, uint32_t *status) {
	if (threadIdx.x != 0 || blockIdx.x != 0) return;
	typedef typename ModWideOf<S>::type E;
	ModWPT<E> wp;
	wp.on = d_pred == 6; wp.width = width; wp.errors = (E *) wp_scratch;
	wp.p1 = wpp[0]; wp.p2 = wpp[1];
	for (int i = 0; i < 5; ++i) wp.p3[i] = wpp[2 + i];
	for (int i = 0; i < 4; ++i) wp.w[i] = wpp[7 + i];
	uint32_t err = 0;
	for (int32_t i = 0; i < num_c; ++i) {
		const S *palrow = nb_colours > 0 ? pal + (size_t) i * (size_t) pal_stride : nullptr;
		S *out = dst[i];
		if (wp.on) for (int32_t k = 0; k < 2 * width * 5; ++k) wp.errors[k] = 0;
		for (int k = 0; k < 5; ++k) wp.pred[k] = 0;
		wp.blend_err_w = wp.blend_err_n = wp.blend_err_nw = wp.blend_err_ne = 0;
		for (int32_t y = 0; y < height; ++y) {
			const S *idxline = idx + (size_t) y * (size_t) width;
			S *line = out + (size_t) y * (size_t) width;
			for (int32_t x = 0; x < width; ++x) {
				const S index = idxline[x];
				const bool is_delta = index < nb_deltas;
				S val = palette_value(index, i, palrow, nb_colours, bpp);
				const ModNeigh p = mod_neighbours<false>(line, width, width, x, y);
				wp_before<false>(wp, x, y, p);
				if (is_delta) val = (S) (uint32_t) (uint64_t) (val + mod_predict(d_pred, wp, p, &err));   // (wraps to the sample type)
				wp_after(wp, x, y, val);
				line[x] = val;
			}
		}
	}
	if (err) *status = err;
}

// horizontal step: out[y][2k], out[y][2k + 1] from avg[y][k], res[y][k]. One wavefront takes 64 rows; it walks along them in
// pieces of SQZ_CHUNK pairs: the pieces of all 64 rows are loaded with one coalesced 128-byte read per row into LDS (odd pitch
// in dwords: a lane walking its own row hits its own bank), each lane runs the recurrence over its row's piece, and the
// 2 * SQZ_CHUNK results per row go out as two coalesced 128-byte writes. `left` (the sample before the pair) stays in a register.
enum { SQZ_CHUNK = 64 };
template <typename S> constexpr int SQZ_ROWS = sizeof(S) == 2 ? 64 : 32;   // rows a wavefront takes
template <typename S>
__global__ void __launch_bounds__(64) k_unsqueeze_h(const S *__restrict__ avg, const S *__restrict__ res, S *__restrict__ out, int32_t aw, int32_t ah, int32_t rw) {
	// (the staging is sized from the sample: 64 rows of int16, 32 rows of int32 -- 33 KB either way; the pitch stays odd in dwords)
	constexpr int PAD = sizeof(S) == 2 ? 2 : 1, ROWS = SQZ_ROWS<S>;
	__shared__ S s_avg[ROWS][SQZ_CHUNK + PAD], s_res[ROWS][SQZ_CHUNK + PAD], s_out[ROWS][2 * SQZ_CHUNK + PAD];
	const int32_t lane = threadIdx.x, y0 = (int32_t) blockIdx.x * ROWS, rows = min(ROWS, ah - y0), ow = aw + rw;
	int32_t left = 0;
	for (int32_t x0 = 0; x0 < aw; x0 += SQZ_CHUNK) {
		for (int32_t r0 = 0; r0 < rows; r0 += 8) {   // eight rows' requests in flight before the first one is waited for
			S va[8], vr[8], ve[8];
#pragma unroll
			for (int j = 0; j < 8; ++j) {
				const int32_t r = min(r0 + j, rows - 1);
				const size_t ra = (size_t) (y0 + r) * (size_t) aw, rr = (size_t) (y0 + r) * (size_t) rw;
				va[j] = x0 + lane < aw ? avg[ra + (size_t) (x0 + lane)] : (S) 0;
				ve[j] = lane == 0 && x0 + SQZ_CHUNK < aw ? avg[ra + (size_t) (x0 + SQZ_CHUNK)] : (S) 0;
				vr[j] = x0 + lane < rw ? res[rr + (size_t) (x0 + lane)] : (S) 0;
			}
#pragma unroll
			for (int j = 0; j < 8; ++j) if (r0 + j < rows) {
				s_avg[r0 + j][lane] = va[j];
				if (lane == 0) s_avg[r0 + j][SQZ_CHUNK] = ve[j];
				s_res[r0 + j][lane] = vr[j];
			}
		}
		__syncthreads();
		if (lane < rows) {
			const int32_t n = min(SQZ_CHUNK, rw - x0);   // pairs in this piece (<= 0 behind the last residual)
			for (int32_t k = 0; k < n; ++k) {
				const int32_t a = s_avg[lane][k], next = x0 + k + 1 < aw ? (int32_t) s_avg[lane][k + 1] : a;
				int32_t p, q;
				unsqueeze_pair(a, s_res[lane][k], x0 + k > 0 ? left : a, next, &p, &q);
				s_out[lane][2 * k] = (S) p; s_out[lane][2 * k + 1] = (S) q;
				left = (S) q;
			}
			if (aw > rw && aw - 1 >= x0 && aw - 1 < x0 + SQZ_CHUNK) s_out[lane][2 * (aw - 1 - x0)] = s_avg[lane][aw - 1 - x0];   // odd width: the last average passes through
		}
		__syncthreads();
		for (int32_t r = 0; r < rows; ++r) {   // (stores do not wait for one another)
			const size_t ro = (size_t) (y0 + r) * (size_t) ow + (size_t) (2 * x0);
			if (2 * x0 + lane < ow) out[ro + (size_t) lane] = s_out[r][lane];
			if (2 * x0 + 64 + lane < ow) out[ro + 64 + (size_t) lane] = s_out[r][64 + lane];
		}
		__syncthreads();
	}
}

// vertical step: one lane per column; consecutive lanes touch consecutive samples of a row, so every access is coalesced. The
// recurrence runs down the column; its inputs do not depend on it, so they are requested SQZ_AHEAD rows ahead of their use (a
// column of 8192 pairs would otherwise wait for memory 8192 times)
enum { SQZ_AHEAD = 8 };
template <typename S>
__global__ void __launch_bounds__(256) k_unsqueeze_v(const S *__restrict__ avg, const S *__restrict__ res, S *__restrict__ out, int32_t aw, int32_t ah, int32_t rh) {
	const int32_t x = (int32_t) (blockIdx.x * blockDim.x + threadIdx.x);
	if (x >= aw) return;
	const size_t pitch = (size_t) aw;
	int32_t a_q[SQZ_AHEAD + 1], r_q[SQZ_AHEAD];   // a_q[j] = avg[k + j], r_q[j] = res[k + j] for the block of rows being processed
	int32_t left = 0;
	for (int32_t k0 = 0; k0 < rh; k0 += SQZ_AHEAD) {
#pragma unroll
		for (int j = 0; j <= SQZ_AHEAD; ++j) a_q[j] = k0 + j < ah ? (int32_t) avg[(size_t) (k0 + j) * pitch + (size_t) x] : 0;
#pragma unroll
		for (int j = 0; j < SQZ_AHEAD; ++j) r_q[j] = k0 + j < rh ? (int32_t) res[(size_t) (k0 + j) * pitch + (size_t) x] : 0;
#pragma unroll
		for (int j = 0; j < SQZ_AHEAD; ++j) {
			const int32_t k = k0 + j;
			if (k < rh) {
				const int32_t a = a_q[j], next = k + 1 < ah ? a_q[j + 1] : a;
				int32_t p, q;
				unsqueeze_pair(a, r_q[j], k > 0 ? left : a, next, &p, &q);
				out[(size_t) (2 * k) * pitch + (size_t) x] = (S) p; out[(size_t) (2 * k + 1) * pitch + (size_t) x] = (S) q;
				left = (S) q;
			}
		}
	}
	if (ah > rh) out[(size_t) (2 * rh) * pitch + (size_t) x] = avg[(size_t) rh * pitch + (size_t) x];
}

// K: the scale shift (scale_dev.h). K > 0: a lane per OUTPUT pixel renders each sample of its cell (clamp, then the 8-bit rule) and stores
// the mean of the rendered pixels -- no full-size RGBA is written. K = 0 is the kernel it always was.
template <int K, typename S>
__global__ void __launch_bounds__(256) k_pack_planes(const S *r, const S *g, const S *b, const S *a, int32_t width, int32_t height, int32_t bpp, uint8_t *rgba, size_t stride_bytes) {
	const size_t n = (size_t) width * (size_t) height;
	const int32_t opaque = (1 << bpp) - 1;
	if constexpr (K > 0) {
		const int32_t ow = scale_out_size(width, K), oh = scale_out_size(height, K);
		for (size_t o = (size_t) blockIdx.x * blockDim.x + threadIdx.x; o < (size_t) ow * (size_t) oh; o += (size_t) gridDim.x * blockDim.x) {
			const int32_t oy = (int32_t) (o / (size_t) ow), ox = (int32_t) (o - (size_t) oy * (size_t) ow), cw = scale_span(ox, width, K), ch = scale_span(oy, height, K);
			ScaleAcc<4> acc;
			acc.clear();
			for (int32_t dy = 0; dy < ch; ++dy) for (int32_t dx = 0; dx < cw; ++dx) {
				const size_t i = (size_t) ((oy << K) + dy) * (size_t) width + (size_t) ((ox << K) + dx);
				acc.add(pack_rgba8(r[i], g[i], b[i], a ? a[i] : opaque, bpp));
			}
			__builtin_nontemporal_store(acc.mean(cw * ch, K), (uint32_t *) (rgba + (size_t) oy * stride_bytes + (size_t) ox * 4));
		}
		return;
	}
	for (size_t i = (size_t) blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t) gridDim.x * blockDim.x) {
		const size_t y = i / (size_t) width, x = i - y * (size_t) width;
		*(uint32_t *) (rgba + y * stride_bytes + x * 4) = pack_rgba8(r[i], g[i], b[i], a ? a[i] : opaque, bpp);
	}
}

// the same over one rectangle of the picture (a group range's, sharded decodes): planes are `plane_width` samples wide
template <typename S>
__global__ void __launch_bounds__(256) k_pack_planes_rect(const S *r, const S *g, const S *b, const S *a, int32_t plane_width, int32_t x0, int32_t y0, int32_t rw, int32_t rh, int32_t bpp, uint8_t *rgba, size_t stride_bytes) {
	const size_t n = (size_t) rw * (size_t) rh;
	const int32_t opaque = (1 << bpp) - 1;
	for (size_t k = (size_t) blockIdx.x * blockDim.x + threadIdx.x; k < n; k += (size_t) gridDim.x * blockDim.x) {
		const size_t y = k / (size_t) rw + (size_t) y0, x = k % (size_t) rw + (size_t) x0, i = y * (size_t) plane_width + x;
		*(uint32_t *) (rgba + y * stride_bytes + x * 4) = pack_rgba8(r[i], g[i], b[i], a ? a[i] : opaque, bpp);
	}
}

// the 16-bit forms (J40_U16X4): pack_rgba16, 8 bytes a pixel as one store; alpha without a plane: 65535
template <int K, typename S>
__global__ void __launch_bounds__(256) k_pack_planes16(const S *r, const S *g, const S *b, const S *a, int32_t width, int32_t height, int32_t bpp, uint8_t *rgba, size_t stride_bytes) {
	const size_t n = (size_t) width * (size_t) height;
	const int32_t opaque = (1 << bpp) - 1;
	if constexpr (K > 0) {   // (k_pack_planes)
		const int32_t ow = scale_out_size(width, K), oh = scale_out_size(height, K);
		for (size_t o = (size_t) blockIdx.x * blockDim.x + threadIdx.x; o < (size_t) ow * (size_t) oh; o += (size_t) gridDim.x * blockDim.x) {
			const int32_t oy = (int32_t) (o / (size_t) ow), ox = (int32_t) (o - (size_t) oy * (size_t) ow), cw = scale_span(ox, width, K), ch = scale_span(oy, height, K);
			ScaleAcc<8> acc;
			acc.clear();
			for (int32_t dy = 0; dy < ch; ++dy) for (int32_t dx = 0; dx < cw; ++dx) {
				const size_t i = (size_t) ((oy << K) + dy) * (size_t) width + (size_t) ((ox << K) + dx);
				acc.add(pack_rgba16(r[i], g[i], b[i], a ? a[i] : opaque, bpp));
			}
			__builtin_nontemporal_store(acc.mean(cw * ch, K), (uint64_t *) (rgba + (size_t) oy * stride_bytes + (size_t) ox * 8));
		}
		return;
	}
	for (size_t i = (size_t) blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t) gridDim.x * blockDim.x) {
		const size_t y = i / (size_t) width, x = i - y * (size_t) width;
		__builtin_nontemporal_store(pack_rgba16(r[i], g[i], b[i], a ? a[i] : opaque, bpp), (uint64_t *) (rgba + y * stride_bytes + x * 8));
	}
}
template <typename S>
__global__ void __launch_bounds__(256) k_pack_planes16_rect(const S *r, const S *g, const S *b, const S *a, int32_t plane_width, int32_t x0, int32_t y0, int32_t rw, int32_t rh, int32_t bpp, uint8_t *rgba, size_t stride_bytes) {
	const size_t n = (size_t) rw * (size_t) rh;
	const int32_t opaque = (1 << bpp) - 1;
	for (size_t k = (size_t) blockIdx.x * blockDim.x + threadIdx.x; k < n; k += (size_t) gridDim.x * blockDim.x) {
		const size_t y = k / (size_t) rw + (size_t) y0, x = k % (size_t) rw + (size_t) x0, i = y * (size_t) plane_width + x;
		__builtin_nontemporal_store(pack_rgba16(r[i], g[i], b[i], a ? a[i] : opaque, bpp), (uint64_t *) (rgba + y * stride_bytes + x * 8));
	}
}

static unsigned grid_for(size_t n) { size_t b = (n + 255) / 256; return (unsigned) (b < 1 ? 1 : b > 8192 ? 8192 : b); }

// sections [first_section, first_section + num_sections): the passes of a multi-pass frame are launched one after the other
template <typename S>
static void launch_sections_of(const DevModPlan &plan, int32_t first_section, int32_t num_sections, const ModLaunchInfo &info, hipStream_t stream) {
	auto align16 = [](uint32_t v) { return (v + 15u) & ~15u; };
	const uint32_t wp_bytes = info.uses_wp ? align16((sizeof(S) == 4 ? 80u : 40u) * (uint32_t) info.max_width) : 0;
	const uint32_t lds = align16((uint32_t) info.num_tree_nodes * (uint32_t) sizeof(DevTreeNode)) + align16((uint32_t) info.num_dist + 4)
		+ align16((uint32_t) info.num_clusters * (uint32_t) sizeof(DevCluster)) + align16(info.table_bytes) + align16(12u * (uint32_t) (info.max_width + 4)) + wp_bytes + 64;
	if (lds <= 156u * 1024u) {
		static bool configured = false;
		if (!configured) { (void) hipFuncSetAttribute((const void *) k_modular_sections<true, S>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024); configured = true; }
		hipLaunchKernelGGL((k_modular_sections<true, S>), dim3((unsigned) num_sections), dim3(64), lds, stream, plan, first_section, info.max_width + 4, info.uses_wp ? info.max_width : 0);
	} else {
		hipLaunchKernelGGL((k_modular_sections<false, S>), dim3((unsigned) num_sections), dim3(64), 0, stream, plan, first_section, 0, 0);
	}
}
void launch_modular_sections(const DevModPlan &plan, int32_t first_section, int32_t num_sections, const ModLaunchInfo &info, hipStream_t stream) {
	if (num_sections <= 0) return;
	// the sections the wave-cooperative kernel takes (modular_coop.hip), then the others
	if (info.quad_sections > 0) launch_modular_quad(plan, first_section, num_sections, info.quad_spec, info.quad_table_span, info.quad_width, stream);
	if (info.coop_width > 0 && info.quad_sections < info.coop_sections) launch_modular_coop(plan, first_section, num_sections, info.coop_width, stream, info.wide != 0);
	if (info.split_sections > 0) launch_modular_split(plan, first_section, num_sections, info, stream);   // (sections with a position-only tree: modular_split.hip)
	if (info.all_coop) return;
	if (info.wide) launch_sections_of<int32_t>(plan, first_section, num_sections, info, stream);
	else launch_sections_of<int16_t>(plan, first_section, num_sections, info, stream);
}
void launch_section_inverse_rcts(const DevModPlan &plan, int32_t first_section, int32_t num_sections, hipStream_t stream, bool wide) {
	if (num_sections <= 0) return;
	if (wide) hipLaunchKernelGGL(k_section_inverse_rcts<int32_t>, dim3((unsigned) num_sections), dim3(256), 0, stream, plan, first_section);
	else hipLaunchKernelGGL(k_section_inverse_rcts<int16_t>, dim3((unsigned) num_sections), dim3(256), 0, stream, plan, first_section);
}
void launch_paste_plane(PlanePtr src, int32_t w, int32_t h, PlanePtr dst, int32_t dst_stride, hipStream_t stream) {
	const size_t n = (size_t) w * (size_t) h;
	if (!n) return;
	if (dst.wide()) hipLaunchKernelGGL(k_paste_plane<int32_t>, dim3(grid_for(n)), dim3(256), 0, stream, (const int32_t *) src.p, w, n, (int32_t *) dst.p, dst_stride);
	else hipLaunchKernelGGL(k_paste_plane<int16_t>, dim3(grid_for(n)), dim3(256), 0, stream, (const int16_t *) src.p, w, n, (int16_t *) dst.p, dst_stride);
}
void launch_inverse_rct(PlanePtr a, PlanePtr b, PlanePtr c, size_t n, int32_t type7, hipStream_t stream) {
	if (!n) return;
	if (a.wide()) hipLaunchKernelGGL(k_inverse_rct<int32_t>, dim3(grid_for(n)), dim3(256), 0, stream, (int32_t *) a.p, (int32_t *) b.p, (int32_t *) c.p, n, type7);
	else hipLaunchKernelGGL(k_inverse_rct<int16_t>, dim3(grid_for(n)), dim3(256), 0, stream, (int16_t *) a.p, (int16_t *) b.p, (int16_t *) c.p, n, type7);
}
void launch_inverse_palette_plain(PlanePtr idx, PlanePtr palrow, PlanePtr dst, size_t n, int32_t i, int32_t nb_colours, int32_t bpp, hipStream_t stream) {
	if (!n) return;
	if (dst.wide()) hipLaunchKernelGGL(k_inverse_palette_plain<int32_t>, dim3(grid_for(n)), dim3(256), 0, stream, (const int32_t *) idx.p, (const int32_t *) palrow.p, (int32_t *) dst.p, n, i, nb_colours, bpp);
	else hipLaunchKernelGGL(k_inverse_palette_plain<int16_t>, dim3(grid_for(n)), dim3(256), 0, stream, (const int16_t *) idx.p, (const int16_t *) palrow.p, (int16_t *) dst.p, n, i, nb_colours, bpp);
}
void launch_inverse_palette_predicted(PlanePtr idx, PlanePtr pal, int32_t pal_stride, void *const *dst_dev, int32_t num_c, int32_t width, int32_t height,
		int32_t nb_colours, int32_t nb_deltas, int32_t d_pred, int32_t bpp, const int8_t *wpp_dev, int32_t *wp_scratch, uint32_t *status, hipStream_t stream) {
	if (idx.wide()) hipLaunchKernelGGL(k_inverse_palette_predicted<int32_t>, dim3(1), dim3(64), 0, stream, (const int32_t *) idx.p, (const int32_t *) pal.p, pal_stride, (int32_t *const *) dst_dev, num_c, width, height, nb_colours, nb_deltas, d_pred, bpp, wpp_dev, wp_scratch, status);
	else hipLaunchKernelGGL(k_inverse_palette_predicted<int16_t>, dim3(1), dim3(64), 0, stream, (const int16_t *) idx.p, (const int16_t *) pal.p, pal_stride, (int16_t *const *) dst_dev, num_c, width, height, nb_colours, nb_deltas, d_pred, bpp, wpp_dev, wp_scratch, status);
}
// avg: aw x ah, res: rw x rh; horizontal: rh == ah, out is (aw + rw) x ah; vertical: rw == aw, out is aw x (ah + rh)
void launch_inverse_squeeze(PlanePtr avg, PlanePtr res, PlanePtr out, int32_t aw, int32_t ah, int32_t rw, int32_t rh, bool horizontal, hipStream_t stream) {
	if (aw <= 0 || ah <= 0) return;
	if (out.wide()) {
		if (horizontal) hipLaunchKernelGGL(k_unsqueeze_h<int32_t>, dim3((unsigned) ((ah + SQZ_ROWS<int32_t> - 1) / SQZ_ROWS<int32_t>)), dim3(64), 0, stream, (const int32_t *) avg.p, (const int32_t *) res.p, (int32_t *) out.p, aw, ah, rw);
		else hipLaunchKernelGGL(k_unsqueeze_v<int32_t>, dim3((unsigned) ((aw + 255) / 256)), dim3(256), 0, stream, (const int32_t *) avg.p, (const int32_t *) res.p, (int32_t *) out.p, aw, ah, rh);
		return;
	}
	if (horizontal) hipLaunchKernelGGL(k_unsqueeze_h<int16_t>, dim3((unsigned) ((ah + 63) / 64)), dim3(64), 0, stream, (const int16_t *) avg.p, (const int16_t *) res.p, (int16_t *) out.p, aw, ah, rw);
	else hipLaunchKernelGGL(k_unsqueeze_v<int16_t>, dim3((unsigned) ((aw + 255) / 256)), dim3(256), 0, stream, (const int16_t *) avg.p, (const int16_t *) res.p, (int16_t *) out.p, aw, ah, rh);
}
template <typename S>
static void launch_pack_of(const S *r, const S *g, const S *b, const S *a, int32_t width, int32_t height, int32_t bpp, uint8_t *rgba, size_t stride, hipStream_t stream, bool rgba16, int32_t shift) {
	if (shift > 0) {
		const unsigned grid = grid_for((size_t) scale_out_size(width, shift) * (size_t) scale_out_size(height, shift));
		if (rgba16 && shift == 1) hipLaunchKernelGGL((k_pack_planes16<1, S>), dim3(grid), dim3(256), 0, stream, r, g, b, a, width, height, bpp, rgba, stride);
		else if (rgba16) hipLaunchKernelGGL((k_pack_planes16<2, S>), dim3(grid), dim3(256), 0, stream, r, g, b, a, width, height, bpp, rgba, stride);
		else if (shift == 1) hipLaunchKernelGGL((k_pack_planes<1, S>), dim3(grid), dim3(256), 0, stream, r, g, b, a, width, height, bpp, rgba, stride);
		else hipLaunchKernelGGL((k_pack_planes<2, S>), dim3(grid), dim3(256), 0, stream, r, g, b, a, width, height, bpp, rgba, stride);
		return;
	}
	if (rgba16) hipLaunchKernelGGL((k_pack_planes16<0, S>), dim3(grid_for((size_t) width * (size_t) height)), dim3(256), 0, stream, r, g, b, a, width, height, bpp, rgba, stride);
	else hipLaunchKernelGGL((k_pack_planes<0, S>), dim3(grid_for((size_t) width * (size_t) height)), dim3(256), 0, stream, r, g, b, a, width, height, bpp, rgba, stride);
}
void launch_pack_planes(PlanePtr r, PlanePtr g, PlanePtr b, PlanePtr a, int32_t width, int32_t height, int32_t bpp, uint8_t *rgba, size_t stride, hipStream_t stream, bool rgba16, int32_t shift) {
	if (r.wide()) launch_pack_of((const int32_t *) r.p, (const int32_t *) g.p, (const int32_t *) b.p, (const int32_t *) a.p, width, height, bpp, rgba, stride, stream, rgba16, shift);
	else launch_pack_of((const int16_t *) r.p, (const int16_t *) g.p, (const int16_t *) b.p, (const int16_t *) a.p, width, height, bpp, rgba, stride, stream, rgba16, shift);
}

template <typename S>
static void launch_pack_rect_of(const S *r, const S *g, const S *b, const S *a, int32_t plane_width, int32_t x0, int32_t y0, int32_t rw, int32_t rh, int32_t bpp, uint8_t *rgba, size_t stride, hipStream_t stream, bool rgba16) {
	if (rgba16) hipLaunchKernelGGL(k_pack_planes16_rect<S>, dim3(grid_for((size_t) rw * (size_t) rh)), dim3(256), 0, stream, r, g, b, a, plane_width, x0, y0, rw, rh, bpp, rgba, stride);
	else hipLaunchKernelGGL(k_pack_planes_rect<S>, dim3(grid_for((size_t) rw * (size_t) rh)), dim3(256), 0, stream, r, g, b, a, plane_width, x0, y0, rw, rh, bpp, rgba, stride);
}
void launch_pack_planes_rect(PlanePtr r, PlanePtr g, PlanePtr b, PlanePtr a, int32_t plane_width, int32_t x0, int32_t y0, int32_t rw, int32_t rh, int32_t bpp, uint8_t *rgba, size_t stride, hipStream_t stream, bool rgba16) {
	if (rw <= 0 || rh <= 0) return;
	if (r.wide()) launch_pack_rect_of((const int32_t *) r.p, (const int32_t *) g.p, (const int32_t *) b.p, (const int32_t *) a.p, plane_width, x0, y0, rw, rh, bpp, rgba, stride, stream, rgba16);
	else launch_pack_rect_of((const int16_t *) r.p, (const int16_t *) g.p, (const int16_t *) b.p, (const int16_t *) a.p, plane_width, x0, y0, rw, rh, bpp, rgba, stride, stream, rgba16);
}

} // namespace j40hip
