// tools/jxlsynth_modular.hpp -- Modular sub-bitstream *encoder* for the synthetic stream generator
// (test/bench infrastructure). Inverse of the reference's MA-tree reader (j40__tree, j40.h:3461),
// Modular header (j40__modular_header, j40.h:3717) and per-pixel decode loop
// (j40__modular_channel, j40.h:4127).
#pragma once
#include "jxlsynth_common.hpp"

namespace synth {

struct TreeNode {
	// branch: prop >= 0 (property index), go to `left` if property value > threshold else `right`
	// leaf:   prop < 0
	int prop = -1;
	int threshold = 0;
	int left = -1, right = -1;      // node indices (builder order, any)
	int predictor = 5, offset = 0, mul_shift = 0, mul_bits = 0;  // multiplier = (mul_bits + 1) << mul_shift
	int ctx = -1;                   // assigned in BFS order when serialised
};

struct MATree {
	std::vector<TreeNode> nodes;    // nodes[0] = root
	std::vector<int> bfs;           // serialisation order
	int num_ctx = 0;
	int leaf(int predictor, int offset = 0, int mul_shift = 0, int mul_bits = 0) {
		TreeNode n; n.predictor = predictor; n.offset = offset; n.mul_shift = mul_shift; n.mul_bits = mul_bits;
		nodes.push_back(n); return (int) nodes.size() - 1;
	}
	int branch(int prop, int threshold, int left, int right) {
		TreeNode n; n.prop = prop; n.threshold = threshold; n.left = left; n.right = right;
		nodes.push_back(n); return (int) nodes.size() - 1;
	}
	// the reader numbers leaves in the order it meets them, which is breadth-first (j40.h:3475-3494)
	void finalise(int root) {
		bfs.clear(); num_ctx = 0;
		std::vector<int> queue{root};
		for (size_t h = 0; h < queue.size(); ++h) {
			int id = queue[h]; bfs.push_back(id);
			if (nodes[(size_t) id].prop >= 0) { queue.push_back(nodes[(size_t) id].left); queue.push_back(nodes[(size_t) id].right); }
			else nodes[(size_t) id].ctx = num_ctx++;
		}
		rootidx = root;
	}
	int rootidx = 0;
	bool uses_wp() const {
		for (const auto &n : nodes) if ((n.prop < 0 && n.predictor == 6) || n.prop == 15) return true;
		return false;
	}
};

// the six tree contexts: 1 = property + 1 (0 = leaf), 0 = threshold, 2 = predictor, 3 = offset,
// 4 = multiplier shift, 5 = multiplier bits (j40.h:3485-3501)
inline void tree_tokens(const MATree &t, StreamEncoder &enc) {
	for (int id : t.bfs) {
		const TreeNode &n = t.nodes[(size_t) id];
		if (n.prop >= 0) {
			enc.add(1, (uint32_t) (n.prop + 1));
			enc.add(0, pack_signed(n.threshold));
		} else {
			enc.add(1, 0);
			enc.add(2, (uint32_t) n.predictor);
			enc.add(3, pack_signed(n.offset));
			enc.add(4, (uint32_t) n.mul_shift);
			enc.add(5, (uint32_t) n.mul_bits);
		}
	}
}

// a channel being encoded: values are what the decoder must reconstruct
struct Channel {
	int w = 0, h = 0;
	int hshift = 0, vshift = 0;     // how often the channel was halved by Squeeze steps (decides which section codes it)
	std::vector<int32_t> px;
	Channel() {}
	Channel(int w_, int h_) : w(w_), h(h_), px((size_t) w_ * (size_t) h_, 0) {}
	int32_t &at(int x, int y) { return px[(size_t) y * (size_t) w + (size_t) x]; }
	int32_t at(int x, int y) const { return px[(size_t) y * (size_t) w + (size_t) x]; }
};

struct WPParams { int p1 = 16, p2 = 10, p3[5] = {7, 7, 7, 0, 0}, w[4] = {13, 12, 12, 12}; };

// weighted ("self-correcting") predictor state, restating what the decoder keeps (j40.h:3997-4111)
// (stats=1) how often the writer's walk used the weighted predictor: leaves with predictor 6 / tests of property 15
inline uint64_t &wp_predicted_samples() { static uint64_t n = 0; return n; }
inline uint64_t &wp_property_tests() { static uint64_t n = 0; return n; }
inline bool wp_is_default(const WPParams &p) { const WPParams d; return p.p1 == d.p1 && p.p2 == d.p2 && !memcmp(p.p3, d.p3, sizeof d.p3) && !memcmp(p.w, d.w, sizeof d.w); }
// the k-th header's own parameters where every header is to differ from the base and from its neighbours
inline WPParams wp_derived(const WPParams &base, int k) {
	WPParams p = base;
	p.p1 = (p.p1 + 3 * k + 1) & 31; p.p2 = (p.p2 + 5 * k + 2) & 31;
	for (int i = 0; i < 5; ++i) p.p3[i] = (p.p3[i] + (i + 2) * (k + 1)) & 31;
	for (int i = 0; i < 4; ++i) p.w[i] = (p.w[i] + (i + 1) * (k + 1)) & 15;
	return p;
}

struct WPState {
	int width = 0; WPParams params; bool on = false;
	std::vector<std::array<int64_t, 5>> err;   // two rows
	int64_t pred[5] = {0, 0, 0, 0, 0};
	int64_t te_w = 0, te_n = 0, te_nw = 0, te_ne = 0;
	void init(int w, const WPParams &p) { width = w; params = p; on = true; err.assign((size_t) w * 2, std::array<int64_t, 5>{0, 0, 0, 0, 0}); }
	static int64_t div24(int64_t i) { return ((int64_t) 1 << 24) / (i + 1); }
	void before(int x, int y, int64_t pw, int64_t pn, int64_t pnw, int64_t pne, int64_t pnn) {
		if (!on) return;
		static const std::array<int64_t, 5> ZERO{0, 0, 0, 0, 0};
		const std::array<int64_t, 5> *cur = &err[(size_t) ((y & 1) ? width : 0)], *prv = &err[(size_t) ((y & 1) ? 0 : width)];
		const auto &ew = x > 0 ? cur[x - 1] : ZERO;
		const auto &en = y > 0 ? prv[x] : ZERO;
		const auto &enw = x > 0 && y > 0 ? prv[x - 1] : en;
		const auto &ene = x + 1 < width && y > 0 ? prv[x + 1] : en;
		const auto &eww = x > 1 ? cur[x - 2] : ZERO;
		const auto &ew2 = x + 1 < width ? ZERO : ew;
		te_w = x > 0 ? cur[x - 1][4] : 0;
		te_n = y > 0 ? prv[x][4] : 0;
		te_nw = x > 0 && y > 0 ? prv[x - 1][4] : te_n;
		te_ne = x + 1 < width && y > 0 ? prv[x + 1][4] : te_n;
		pred[0] = (pw + pne - pn) * 8;
		pred[1] = pn * 8 - (((te_w + te_n + te_ne) * params.p1) >> 5);
		pred[2] = pw * 8 - (((te_w + te_n + te_nw) * params.p2) >> 5);
		pred[3] = pn * 8 - ((te_nw * params.p3[0] + te_n * params.p3[1] + te_ne * params.p3[2] + (pnn - pn) * 8 * params.p3[3] + (pnw - pw) * 8 * params.p3[4]) >> 5);
		int64_t w[4], wsum = 0, sum = 0;
		for (int i = 0; i < 4; ++i) {
			int64_t errsum = en[(size_t) i] + ew[(size_t) i] + enw[(size_t) i] + eww[(size_t) i] + ene[(size_t) i] + ew2[(size_t) i];
			int shift = std::max(floor_lg64((uint64_t) errsum + 1) - 5, 0);
			w[i] = 4 + ((int64_t) params.w[i] * div24(errsum >> shift) >> shift);
		}
		int logw = floor_lg64((uint64_t) (w[0] + w[1] + w[2] + w[3])) - 4;
		for (int i = 0; i < 4; ++i) { w[i] >>= logw; wsum += w[i]; sum += pred[i] * w[i]; }
		pred[4] = (sum + (wsum >> 1) - 1) * div24(wsum - 1) >> 24;
		if (((te_n ^ te_w) | (te_n ^ te_nw)) <= 0) {
			int64_t lo = std::min(pw, std::min(pn, pne)) * 8, hi = std::max(pw, std::max(pn, pne)) * 8;
			pred[4] = std::min(std::max(lo, pred[4]), hi);
		}
	}
	void after(int x, int y, int64_t val) {
		if (!on) return;
		auto &e = err[(size_t) ((y & 1) ? width : 0) + (size_t) x];
		for (int i = 0; i < 4; ++i) { int64_t d = pred[i] - val * 8; e[(size_t) i] = ((d < 0 ? -d : d) + 3) >> 3; }
		e[4] = pred[4] - val * 8;
	}
	static int floor_lg64(uint64_t x) { return 63 - __builtin_clzll(x); }
};

struct Neigh { int64_t w, n, nw, ne, nn, nee, ww, nww; };

inline Neigh neighbours(const Channel &c, int x, int y) {  // edge rules of j40.h:3981-3988
	Neigh p;
	p.w = x > 0 ? c.at(x - 1, y) : y > 0 ? c.at(x, y - 1) : 0;
	p.n = y > 0 ? c.at(x, y - 1) : p.w;
	p.nw = x > 0 && y > 0 ? c.at(x - 1, y - 1) : p.w;
	p.ne = x + 1 < c.w && y > 0 ? c.at(x + 1, y - 1) : p.n;
	p.nn = y > 1 ? c.at(x, y - 2) : p.n;
	p.nee = x + 2 < c.w && y > 0 ? c.at(x + 2, y - 1) : p.ne;
	p.ww = x > 1 ? c.at(x - 2, y) : p.w;
	p.nww = x > 1 && y > 0 ? c.at(x - 2, y - 1) : p.ww;
	return p;
}

inline int64_t clamp_grad(int64_t w, int64_t n, int64_t nw) { int64_t lo = std::min(w, n), hi = std::max(w, n); return std::min(std::max(lo, w + n - nw), hi); }

inline int64_t predict(int pred, const Neigh &p, const WPState &wp) {  // j40.h:4080-4100
	switch (pred) {
	case 0: return 0;
	case 1: return p.w;
	case 2: return p.n;
	case 3: return (p.w + p.n) / 2;
	case 4: return std::llabs(p.n - p.nw) < std::llabs(p.w - p.nw) ? p.w : p.n;
	case 5: return clamp_grad(p.w, p.n, p.nw);
	case 6: return (wp.pred[4] + 3) >> 3;
	case 7: return p.ne;
	case 8: return p.nw;
	case 9: return p.ww;
	case 10: return (p.w + p.nw) / 2;
	case 11: return (p.n + p.nw) / 2;
	case 12: return (p.n + p.ne) / 2;
	case 13: return (6 * p.n - 2 * p.nn + 7 * p.w + p.ww + p.nee + 3 * p.ne + 8) / 16;
	}
	die("bad predictor");
}

// The range of a coded sample: int16 (the image says modular_16bit_buffers = 1), or int32 with wide=1 (it says 0)
inline int64_t &sample_lo() { static int64_t v = -32768; return v; }
inline int64_t &sample_hi() { static int64_t v = 32767; return v; }
inline int32_t wrap_sample(int64_t v) { return sample_hi() == 32767 ? (int32_t) (int16_t) (uint16_t) (uint64_t) v : (int32_t) (uint32_t) (uint64_t) v; }

// ---- the picture a stream codes (dumpsrc=): where the writer did not run a forward transform -- a palette, whose picture IS the
//      look-up, and the RCT types it takes the picture as already transformed for -- the samples a reader must arrive at are worked
//      out here, in 64 bits wrapped to the sample type, from ISO 18181-1's statement of the inverse transforms ----
inline void expect_inverse_rct(std::vector<Channel> &ch, int first, int type) {
	static const int PERM[6][3] = {{0, 1, 2}, {1, 2, 0}, {2, 0, 1}, {0, 2, 1}, {1, 0, 2}, {2, 1, 0}};
	Channel *in[3] = {&ch[(size_t) first], &ch[(size_t) first + 1], &ch[(size_t) first + 2]};
	const size_t n = in[0]->px.size();
	for (size_t i = 0; i < n; ++i) {
		const int64_t p0 = in[0]->px[i], p1 = in[1]->px[i], p2 = in[2]->px[i];
		int64_t a = p0, b = p1, c = p2;
		switch (type % 7) {
		case 0: break;
		case 1: c = p2 + p0; break;
		case 2: c = p1 + p0; break;                    // (as the decoders here and j40.h:4353 have it)
		case 3: b = p1 + p0; c = p2 + p0; break;
		case 4: b = p1 + (p0 / 2 + p2 / 2 + (p0 & p2 & 1)); break;
		case 5: b = p1 + p0 + (p2 >> 1); c = p2 + p0; break;
		default: { const int64_t tmp = p0 - (p2 >> 1), q1 = p2 + tmp, q2 = tmp - (p1 >> 1); a = q2 + p1; b = q1; c = q2; }
		}
		in[0]->px[i] = wrap_sample(a); in[1]->px[i] = wrap_sample(b); in[2]->px[i] = wrap_sample(c);
	}
	Channel out[3] = {*in[0], *in[1], *in[2]};
	for (int j = 0; j < 3; ++j) ch[(size_t) (first + PERM[type / 7][j])] = out[j];
}
// the spec's 72 palette delta triples; index 2k is triple k, 2k + 1 its negation
static const int EXPECT_PALETTE_DELTAS[72][3] = {
	{0, 0, 0}, {4, 4, 4}, {11, 0, 0}, {0, 0, -13}, {0, -12, 0}, {-10, -10, -10}, {-18, -18, -18}, {-27, -27, -27},
	{-18, -18, 0}, {0, 0, -32}, {-32, 0, 0}, {-37, -37, -37}, {0, -32, -32}, {24, 24, 45}, {50, 50, 50}, {-45, -24, -24},
	{-24, -45, -45}, {0, -24, -24}, {-34, -34, 0}, {-24, 0, -24}, {-45, -45, -24}, {64, 64, 64}, {-32, 0, -32}, {0, -32, 0},
	{-32, 0, 32}, {-24, -45, -24}, {45, 24, 45}, {24, -24, -45}, {-45, -24, 24}, {80, 80, 80}, {64, 0, 0}, {0, 0, -64},
	{0, -64, -64}, {-24, -24, 45}, {96, 96, 96}, {64, 64, 0}, {45, -24, -24}, {34, -34, 0}, {112, 112, 112}, {24, -45, -45},
	{45, 45, -24}, {0, -32, 32}, {24, -24, 45}, {0, 96, 96}, {45, -24, 24}, {24, -45, -24}, {-24, -45, 24}, {0, -64, 0},
	{96, 0, 0}, {128, 128, 128}, {64, 0, 64}, {144, 144, 144}, {96, 96, 0}, {-36, -36, 36}, {45, -24, -45}, {45, -45, -24},
	{0, 0, -96}, {0, 128, 128}, {0, 96, 0}, {45, 24, -45}, {-128, 0, 0}, {24, -45, 24}, {-45, 24, -45}, {64, 0, -64},
	{64, -64, -64}, {96, 0, 96}, {45, -45, 24}, {24, 45, -45}, {64, 64, -64}, {128, 128, 0}, {0, 0, -128}, {-24, 45, -45},
};
// `ch` = {palette (meta channel), index channel, the rest}: the index channel becomes num_c colour channels in its place
inline void expect_inverse_palette(std::vector<Channel> &ch, int num_c, int nb_colours, int nb_deltas, int d_pred, int bpp, const WPParams &wpp) {
	const Channel pal = ch[0], idx = ch[1];
	std::vector<Channel> out;
	for (int i = 0; i < num_c; ++i) {
		Channel c(idx.w, idx.h);
		WPState wp;
		if (nb_deltas > 0 && d_pred == 6) wp.init(idx.w, wpp);
		for (int y = 0; y < idx.h; ++y) for (int x = 0; x < idx.w; ++x) {
			int64_t k = wrap_sample(idx.at(x, y)), val;
			const bool is_delta = k < nb_deltas;
			if (k < 0) {
				if (i < 3) {
					k = wrap_sample(~k % 143);
					const int64_t entry = k + 1;
					val = EXPECT_PALETTE_DELTAS[entry >> 1][i];
					if (entry & 1) val = -val;
					if (bpp > 8) val = val * ((int64_t) 1 << (std::min(bpp, 24) - 8));
				} else val = 0;
			} else if (k < nb_colours) val = pal.at((int) k, i);
			else {
				k = wrap_sample(k - nb_colours);
				if (k < 64) val = (i < 3 ? k >> (2 * i) : 0) * (((int64_t) 1 << bpp) - 1) / 4 + ((int64_t) 1 << std::max(0, bpp - 3));
				else { k = wrap_sample(k - 64); for (int j = 0; j < i; ++j) k = k / 5; val = (k % 5) * (((int64_t) 1 << bpp) - 1) / 4; }
			}
			val = wrap_sample(val);
			if (nb_deltas > 0) {
				const Neigh p = neighbours(c, x, y);
				wp.before(x, y, p.w, p.n, p.nw, p.ne, p.nn);
				if (is_delta) val = wrap_sample(val + predict(d_pred, p, wp));
				wp.after(x, y, val);
			}
			c.at(x, y) = (int32_t) val;
		}
		out.push_back(c);
	}
	std::vector<Channel> next(out);
	for (size_t c = 2; c < ch.size(); ++c) next.push_back(ch[c]);
	ch.swap(next);
}

// Encodes one channel of a Modular image into `enc` (decode order), mirroring the decoder's tree
// walk. `chans`/`cidx` give access to previous channels for properties >= 16; `sidx` is the stream
// index property. `lossy_quant` > 1 quantises residuals (the channel is updated with what the
// decoder will reconstruct, so later predictions stay in sync).
// `povf_in` (optional): that many samples from now the coded residual takes the sample beyond int16, where the
// reader stops with "povf" (j40.h:4225); what is coded behind it no reader looks at. `povf_to`: the value it is meant to take.
inline void encode_channel(const MATree &tree, std::vector<Channel> &chans, int cidx, int64_t sidx, const WPParams &wpp, StreamEncoder &enc, int64_t *povf_in = nullptr, int64_t povf_to = 40000) {
	Channel &c = chans[(size_t) cidx];
	if (c.w == 0 || c.h == 0) return;
	WPState wp;
	if (tree.uses_wp()) wp.init(c.w, wpp);
	std::vector<int> refc;
	for (int i = cidx - 1; i >= 0; --i) if (chans[(size_t) i].w == c.w && chans[(size_t) i].h == c.h && chans[(size_t) i].hshift == c.hshift && chans[(size_t) i].vshift == c.vshift) refc.push_back(i);
	for (int y = 0; y < c.h; ++y) for (int x = 0; x < c.w; ++x) {
		Neigh p = neighbours(c, x, y);
		wp.before(x, y, p.w, p.n, p.nw, p.ne, p.nn);
		int id = tree.rootidx;
		while (tree.nodes[(size_t) id].prop >= 0) {
			const TreeNode &n = tree.nodes[(size_t) id];
			int64_t val;
			switch (n.prop) {
			case 0: val = cidx; break;
			case 1: val = sidx; break;
			case 2: val = y; break;
			case 3: val = x; break;
			case 4: val = std::llabs(p.n); break;
			case 5: val = std::llabs(p.w); break;
			case 6: val = p.n; break;
			case 7: val = p.w; break;
			case 8: val = x > 0 ? p.w - (p.ww + p.nw - p.nww) : p.w; break;
			case 9: val = p.w + p.n - p.nw; break;
			case 10: val = p.w - p.nw; break;
			case 11: val = p.nw - p.n; break;
			case 12: val = p.n - p.ne; break;
			case 13: val = p.n - p.nn; break;
			case 14: val = p.w - p.ww; break;
			case 15:
				++wp_property_tests();
				val = wp.te_w;
				if (std::llabs(val) < std::llabs(wp.te_n)) val = wp.te_n;
				if (std::llabs(val) < std::llabs(wp.te_nw)) val = wp.te_nw;
				if (std::llabs(val) < std::llabs(wp.te_ne)) val = wp.te_ne;
				break;
			default: {
				int r = (n.prop - 16) / 4;
				if (r >= (int) refc.size()) die("tree references a missing previous channel");
				const Channel &rc = chans[(size_t) refc[(size_t) r]];
				val = rc.at(x, y);
				if ((n.prop - 16) & 2) {
					int64_t rw = x > 0 ? rc.at(x - 1, y) : 0, rn = y > 0 ? rc.at(x, y - 1) : rw, rnw = x > 0 && y > 0 ? rc.at(x - 1, y - 1) : rw;
					val -= clamp_grad(rw, rn, rnw);
				}
				if ((n.prop - 16) & 1) val = std::llabs(val);
				// NOTE the reader tests bits of ~prop = prop index; (prop index & 2) / (& 1)
			} }
			id = val > n.threshold ? n.left : n.right;
		}
		const TreeNode &lf = tree.nodes[(size_t) id];
		int64_t mult = (int64_t) (lf.mul_bits + 1) << lf.mul_shift;
		int64_t pr = predict(lf.predictor, p, wp);
		if (lf.predictor == 6) ++wp_predicted_samples();
		int64_t target = c.at(x, y);
		const bool overflow_here = povf_in && (*povf_in)-- == 0;
		if (overflow_here) target = povf_to;
		int64_t diff = target - pr - lf.offset;
		int64_t q = mult == 1 ? diff : (diff >= 0 ? (diff + mult / 2) / mult : -((-diff + mult / 2) / mult));
		int64_t recon = q * mult + lf.offset + pr;
		const int64_t lo = sample_lo(), hi = sample_hi();   // (int16, or int32 with wide=1)
		if (overflow_here) { while (recon >= lo && recon <= hi) recon = (povf_to < 0 ? --q : ++q) * mult + lf.offset + pr; }
		else if (mult > 1) {   // a coarse leaf may round past the end of the range: one step back
			while (recon > hi) recon = --q * mult + lf.offset + pr;
			while (recon < lo) recon = ++q * mult + lf.offset + pr;
		}
		if (!overflow_here && (recon < lo || recon > hi)) die(hi == 32767 ? "modular sample out of int16 range" : "modular sample out of int32 range");
		if (q < -((int64_t) 1 << 31) || q >= ((int64_t) 1 << 31)) die("modular: a residual leaves the 32 bits a packed hybrid integer has (readers refuse more than 30: iovf)");
		if (overflow_here) recon = hi;
		c.at(x, y) = (int32_t) recon;
		enc.add((uint32_t) lf.ctx, pack_signed((int32_t) q));
		wp.after(x, y, recon);
	}
}

// ---- Squeeze, forward direction (ISO 18181-1; the decoder's half is j40_amd/csrc/device/squeeze_dev.h). Written from the
// standard's formulas independently of the decoder: avg = (A + B + (A > B)) >> 1, residual = A - B - tendency ----
struct SqueezeStep { bool horizontal = true, in_place = true; int begin_c = 0, num_c = 1; };

inline int64_t smooth_tendency(int64_t B, int64_t a, int64_t n) {
	int64_t diff = 0;
	if (B >= a && a >= n) {
		diff = (4 * B - 3 * n - a + 6) / 12;
		if (diff - (diff & 1) > 2 * (B - a)) diff = 2 * (B - a) + 1;
		if (diff + (diff & 1) > 2 * (a - n)) diff = 2 * (a - n);
	} else if (B <= a && a <= n) {
		diff = (4 * B - 3 * n - a - 6) / 12;
		if (diff + (diff & 1) < 2 * (B - a)) diff = 2 * (B - a) - 1;
		if (diff - (diff & 1) < 2 * (a - n)) diff = 2 * (a - n);
	}
	return diff;
}

// one line of n samples (element stride `st`) -> ceil(n / 2) averages and floor(n / 2) residuals
inline void squeeze_line(const int32_t *in, size_t st, int n, int32_t *avg, size_t ast, int32_t *res, size_t rst) {
	const int na = (n + 1) / 2, nr = n / 2;
	for (int k = 0; k < nr; ++k) { const int64_t A = in[(size_t) (2 * k) * st], B = in[(size_t) (2 * k + 1) * st]; avg[(size_t) k * ast] = (int32_t) ((A + B + (A > B)) >> 1); }
	if (na > nr) avg[(size_t) nr * ast] = in[(size_t) (n - 1) * st];
	for (int k = 0; k < nr; ++k) {
		const int64_t A = in[(size_t) (2 * k) * st], B = in[(size_t) (2 * k + 1) * st], a = avg[(size_t) k * ast];
		const int64_t next = k + 1 < na ? avg[(size_t) (k + 1) * ast] : a, left = k > 0 ? in[(size_t) (2 * k - 1) * st] : a;
		res[(size_t) k * rst] = (int32_t) (A - B - smooth_tendency(left, a, next));
	}
}

// the channel list after one step: squeezed channels halved in place, residual channels behind them or at the end
inline void forward_squeeze_step(std::vector<Channel> &chs, const SqueezeStep &st) {
	const int end_c = st.begin_c + st.num_c;
	if (st.begin_c < 0 || st.num_c < 1 || end_c > (int) chs.size()) die("squeeze step out of range");
	std::vector<Channel> residuals;
	for (int c = st.begin_c; c < end_c; ++c) {
		Channel &in = chs[(size_t) c];
		Channel avg, res;
		if (st.horizontal) {
			avg = Channel((in.w + 1) / 2, in.h); res = Channel(in.w / 2, in.h);
			for (int y = 0; y < in.h; ++y) squeeze_line(in.px.data() + (size_t) y * (size_t) in.w, 1, in.w, avg.px.data() + (size_t) y * (size_t) avg.w, 1, res.px.data() + (size_t) y * (size_t) res.w, 1);
			avg.hshift = res.hshift = in.hshift + 1; avg.vshift = res.vshift = in.vshift;
		} else {
			avg = Channel(in.w, (in.h + 1) / 2); res = Channel(in.w, in.h / 2);
			for (int x = 0; x < in.w; ++x) squeeze_line(in.px.data() + x, (size_t) in.w, in.h, avg.px.data() + x, (size_t) in.w, res.px.data() + x, (size_t) in.w);
			avg.hshift = res.hshift = in.hshift; avg.vshift = res.vshift = in.vshift + 1;
		}
		in = std::move(avg);
		residuals.push_back(std::move(res));
	}
	const size_t offset = st.in_place ? (size_t) end_c : chs.size();
	chs.insert(chs.begin() + (long) offset, std::make_move_iterator(residuals.begin()), std::make_move_iterator(residuals.end()));
}

// the parameter list a decoder assumes when the bitstream gives none (num_sq = 0)
inline std::vector<SqueezeStep> default_squeeze_steps(const std::vector<Channel> &chs, int nb_meta) {
	std::vector<SqueezeStep> out;
	const int first = nb_meta, count = (int) chs.size() - first;
	if (count <= 0) return out;
	int w = chs[(size_t) first].w, h = chs[(size_t) first].h;
	SqueezeStep st;
	if (count > 2 && chs[(size_t) first + 1].w == w && chs[(size_t) first + 1].h == h) {
		st.begin_c = first + 1; st.num_c = 2; st.in_place = false;
		st.horizontal = true; out.push_back(st);
		st.horizontal = false; out.push_back(st);
	}
	st.begin_c = first; st.num_c = count; st.in_place = true;
	if (h >= w && h > 8) { st.horizontal = false; out.push_back(st); h = (h + 1) / 2; }
	while (w > 8 || h > 8) {
		if (w > 8) { st.horizontal = true; out.push_back(st); w = (w + 1) / 2; }
		if (h > 8) { st.horizontal = false; out.push_back(st); h = (h + 1) / 2; }
	}
	return out;
}

struct TransformW {
	int kind = 0; int begin_c = 0, rct_type = 0; int num_c = 0, nb_colours = 0, nb_deltas = 0, d_pred = 0;
	std::vector<SqueezeStep> sq;    // kind 2: the explicit parameter list; empty = the default list
};

// Modular header (j40.h:3730-3819)
// (stats=1) the parameter sets written into headers, one entry per header that carries its own
inline std::vector<std::array<int, 11>> &wp_headers_written() { static std::vector<std::array<int, 11>> v; return v; }
inline void write_modular_header(BitWriter &bw, bool use_global_tree, const WPParams *custom_wp, const std::vector<TransformW> &tr) {
	if (custom_wp) wp_headers_written().push_back({custom_wp->p1, custom_wp->p2, custom_wp->p3[0], custom_wp->p3[1], custom_wp->p3[2], custom_wp->p3[3], custom_wp->p3[4], custom_wp->w[0], custom_wp->w[1], custom_wp->w[2], custom_wp->w[3]});
	bw.put(use_global_tree ? 1 : 0, 1);
	if (!custom_wp) bw.put(1, 1);
	else {
		bw.put(0, 1);
		bw.put((uint64_t) custom_wp->p1, 5); bw.put((uint64_t) custom_wp->p2, 5);
		for (int i = 0; i < 5; ++i) bw.put((uint64_t) custom_wp->p3[i], 5);
		for (int i = 0; i < 4; ++i) bw.put((uint64_t) custom_wp->w[i], 4);
	}
	bw.u32((int64_t) tr.size(), 0, 0, 1, 0, 2, 4, 18, 8);
	for (const TransformW &t : tr) {
		bw.put((uint64_t) t.kind, 2);
		if (t.kind == 0) {
			bw.u32(t.begin_c, 0, 3, 8, 6, 72, 10, 1096, 13);
			bw.u32(t.rct_type, 6, 0, 0, 2, 2, 4, 10, 6);
		} else if (t.kind == 1) {
			bw.u32(t.begin_c, 0, 3, 8, 6, 72, 10, 1096, 13);
			bw.u32(t.num_c, 1, 0, 3, 0, 4, 0, 1, 13);
			bw.u32(t.nb_colours, 0, 8, 256, 10, 1280, 12, 5376, 16);
			bw.u32(t.nb_deltas, 0, 0, 1, 8, 257, 10, 1281, 16);
			bw.put((uint64_t) t.d_pred, 4);
		} else if (t.kind == 2) {
			bw.u32((int64_t) t.sq.size(), 0, 0, 1, 4, 9, 6, 41, 8);
			for (const SqueezeStep &q : t.sq) {
				bw.put(q.horizontal ? 1 : 0, 1); bw.put(q.in_place ? 1 : 0, 1);
				bw.u32(q.begin_c, 0, 3, 8, 6, 72, 10, 1096, 13);
				bw.u32(q.num_c, 1, 0, 2, 0, 3, 0, 4, 4);
			}
		} else die("unsupported transform in writer");
	}
}

} // namespace synth
