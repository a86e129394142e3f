// tools/jxlsynth_lz77.hpp -- LZ77 on the writer's side (test infrastructure): a matcher over the sequence of integers a stream
// decodes to, forced copies that DEFINE the values they cover, and the account of what a stream really contains (`stats=1`).
// The reader's half is j40__code (j40.h:2804-2876): a copy's distance symbol is a special code (< 120: dx + dist_mult * dy out of a
// table, at least 1) or a plain distance + 119; the distance is clamped to the number of integers decoded so far and to 2^20; a copy
// from before the first integer reads zeros.
#pragma once
#include "jxlsynth_common.hpp"
#include <unordered_map>

namespace synth {

// (dx + 7) * 16 + dy, the standard's table of special distances (ISO 18181-1, "LZ77 special distances")
static const uint8_t SPECIAL_DISTANCE_CODES[120] = {
	0x71, 0x80, 0x81, 0x61, 0x72, 0x90, 0x82, 0x62, 0x91, 0x51, 0x92, 0x52, 0x73, 0xa0, 0x83, 0x63, 0xa1, 0x41, 0x93, 0x53,
	0xa2, 0x42, 0x74, 0xb0, 0x84, 0x64, 0xb1, 0x31, 0xa3, 0x43, 0x94, 0x54, 0xb2, 0x32, 0x75, 0xa4, 0x44, 0xb3, 0x33, 0xc0,
	0x85, 0x65, 0xc1, 0x21, 0x95, 0x55, 0xc2, 0x22, 0xb4, 0x34, 0xa5, 0x45, 0xc3, 0x23, 0x76, 0xd0, 0x86, 0x66, 0xd1, 0x11,
	0x96, 0x56, 0xd2, 0x12, 0xb5, 0x35, 0xc4, 0x24, 0xa6, 0x46, 0xd3, 0x13, 0x77, 0xe0, 0x87, 0x67, 0xc5, 0x25, 0xe1, 0x01,
	0xb6, 0x36, 0xd4, 0x14, 0x97, 0x57, 0xe2, 0x02, 0xa7, 0x47, 0xe3, 0x03, 0xc6, 0x26, 0xd5, 0x15, 0xf0, 0xb7, 0x37, 0xe4,
	0x04, 0xf1, 0xf2, 0xd6, 0x16, 0xf3, 0xc7, 0x27, 0xe5, 0x05, 0xf4, 0xd7, 0x17, 0xe6, 0x06, 0xf5, 0xe7, 0x07, 0xf6, 0xf7,
};

// the distance special code `k` stands for under the multiplier `mult` (> 0), before the clamp to what has been decoded
inline int64_t special_distance(int k, int64_t mult) {
	const int s = SPECIAL_DISTANCE_CODES[k];
	return std::max<int64_t>(1, (int64_t) ((s >> 4) - 7) + mult * (int64_t) (s & 7));
}

enum { LZ_RUNS = 0, LZ_SPECIAL = 1, LZ_PLAIN = 2, LZ_OVERLAP = 3 };
enum { FORCE_NONE = 0, FORCE_SPECIALS = 1, FORCE_EARLY = 2, FORCE_OVER = 3, FORCE_FAR = 4 };

// what the streams of one file contain; printed as one JSON line by `stats=1`
struct LzStats {
	uint64_t copies = 0, special_copies = 0, plain_copies = 0, overlapping = 0, cross_row = 0, cross_channel = 0, clamped = 0;
	uint64_t first_symbol_copies = 0, beyond_need = 0, distance_one = 0, max_distance = 0, max_length = 0, max_section_integers = 0, far_copies = 0;
	bool code_seen[120] = {false};
	int distinct_codes() const { int n = 0; for (bool b : code_seen) n += b; return n; }
};

// one copy, accounted for. `pos`: integers decoded before it, `nominal`: the distance its symbol stands for, `len`: its length,
// `need`: integers the stream's reader asks for in all, row_of / chan_of: where each of them lies
inline void account_copy(LzStats &st, uint64_t pos, int64_t nominal, uint64_t len, uint32_t dist_code, uint64_t need, const std::vector<uint32_t> &row_of, const std::vector<uint32_t> &chan_of) {
	++st.copies;
	if (dist_code < 120) { ++st.special_copies; st.code_seen[dist_code] = true; } else ++st.plain_copies;
	const uint64_t eff = (uint64_t) std::min<int64_t>(std::min<int64_t>(nominal, (int64_t) pos), 1 << 20);
	if ((uint64_t) nominal > pos) ++st.clamped;
	if (pos == 0) ++st.first_symbol_copies;
	if (eff == 1) ++st.distance_one;
	if (eff > 1 && eff < len) ++st.overlapping;
	if (eff >= (1u << 20) - 4096) ++st.far_copies;
	st.max_distance = std::max(st.max_distance, eff); st.max_length = std::max(st.max_length, len);
	if (pos + len > need) ++st.beyond_need;
	const uint64_t last = std::min(pos + len, need) - 1;
	if (pos < need && row_of[(size_t) pos] != row_of[(size_t) last]) ++st.cross_row;
	if (pos < need && chan_of[(size_t) pos] != chan_of[(size_t) last]) ++st.cross_channel;
}

struct LzParams {
	int mode = LZ_RUNS, force = FORCE_NONE;
	int64_t dist_mult = 0;       // the reader's multiplier for this stream (Modular: the widest non-meta channel, j40.h:3840-3844)
	uint32_t literal_range = 256;  // forced copies: literals are even integers below 2 * literal_range (samples 0 .. literal_range - 1)
};

inline void push_copy(StreamEncoder &enc, const CodeSpecW &sp, uint32_t ctx, uint32_t len, uint32_t dist_code) {
	const uint32_t cl = sp.cluster_map[ctx];
	const HToken t = hybrid_encode(len - (uint32_t) sp.lz_min_length, sp.lz_len_cfg);
	if ((int) t.token + sp.lz_min_symbol >= sp.alphabet_limit()) dief("lz77: a copy of %u integers needs the symbol %d, beyond the alphabet of %d (a smaller min_symbol or length configuration, or prefix codes)", len, (int) t.token + sp.lz_min_symbol, sp.alphabet_limit());
	enc.items.push_back({cl, t.token + (uint32_t) sp.lz_min_symbol, t.extra, (uint8_t) t.nextra});
	const uint32_t lzcl = sp.cluster_map[(size_t) sp.total_dist() - 1];
	const HToken d = hybrid_encode(dist_code, sp.cfg[lzcl]);
	if ((int) d.token >= sp.alphabet_limit()) dief("lz77: the distance code %u needs a token beyond the alphabet of %d", dist_code, sp.alphabet_limit());
	enc.items.push_back({lzcl, d.token, d.extra, (uint8_t) d.nextra});
}

inline void push_literal(StreamEncoder &enc, const CodeSpecW &sp, uint32_t ctx, uint32_t value) {
	const uint32_t cl = sp.cluster_map[ctx];
	const HToken t = hybrid_encode(value, sp.cfg[cl]);
	if ((int) t.token >= sp.lz_min_symbol) dief("lz77: the literal %u needs token %u, which min_symbol = %d takes for a copy", value, t.token, sp.lz_min_symbol);
	enc.items.push_back({cl, t.token, t.extra, (uint8_t) t.nextra});
}

// The matcher: `ctx[i]`, `val[i]` are the context and the integer of the i-th symbol in decode order. Candidates for a copy at i
// are the distances the special codes stand for, 1 .. 8, and the last places the next three integers were seen at. Of the matches
// that reach min_length the mode prefers its own kind (special-coded / any, coded plain / overlapping) and takes the longest.
inline void lz77_match(StreamEncoder &enc, const CodeSpecW &sp, const LzParams &lp, const std::vector<uint32_t> &ctx, const std::vector<uint32_t> &val,
                       const std::vector<uint32_t> &row_of, const std::vector<uint32_t> &chan_of, LzStats &st) {
	const size_t n = val.size();
	const size_t min_len = (size_t) sp.lz_min_length;
	std::vector<std::pair<int64_t, int>> specials;   // (distance, first code that stands for it)
	if (lp.mode != LZ_PLAIN && lp.dist_mult > 0) {
		for (int k = 0; k < 120; ++k) {
			const int64_t d = special_distance(k, lp.dist_mult);
			bool seen = false;
			for (auto &s : specials) if (s.first == d) seen = true;
			if (!seen) specials.push_back({d, k});
		}
	}
	auto code_of = [&](int64_t d) -> uint32_t {
		for (auto &s : specials) if (s.first == d) return (uint32_t) s.second;
		return (uint32_t) d + 119;
	};
	std::unordered_map<uint64_t, std::array<size_t, 4>> last;   // three integers -> the four latest positions they started at (+ 1; 0 = none)
	auto key = [&](size_t i) { return ((uint64_t) val[i] * 0x9e3779b97f4a7c15ull) ^ ((uint64_t) val[i + 1] * 0xc2b2ae3d27d4eb4full) ^ ((uint64_t) val[i + 2] << 40); };
	auto remember = [&](size_t i) {
		if (i + 3 > n) return;
		auto &slot = last[key(i)];
		for (int k = 3; k > 0; --k) slot[(size_t) k] = slot[(size_t) k - 1];
		slot[0] = i + 1;
	};
	auto match_len = [&](size_t i, size_t d) { size_t l = 0; while (i + l < n && val[i + l] == val[i + l - d]) ++l; return l; };
	size_t i = 0;
	while (i < n) {
		size_t best_len = 0, best_d = 0; int best_rank = -1;
		auto consider = [&](size_t d) {
			if (d == 0 || d > i || d > ((size_t) 1 << 20)) return;
			const size_t l = match_len(i, d);
			if (l < min_len) return;
			int rank = 0;
			if (lp.mode == LZ_SPECIAL) rank = code_of((int64_t) d) < 120 ? 1 : 0;
			else if (lp.mode == LZ_OVERLAP) rank = d > 1 && d < l ? 1 : 0;
			if (rank > best_rank || (rank == best_rank && l > best_len)) { best_rank = rank; best_len = l; best_d = d; }
		};
		for (auto &s : specials) consider((size_t) s.first);
		for (size_t d = 1; d <= 8; ++d) consider(d);
		if (i + 3 <= n) { auto it = last.find(key(i)); if (it != last.end()) for (size_t p : it->second) if (p) consider(i - (p - 1)); }
		if (best_len >= min_len) {
			// (a stream without a multiplier codes distance - 1, j40.h:2829)
			const uint32_t code = lp.dist_mult == 0 ? (uint32_t) best_d - 1 : lp.mode == LZ_PLAIN ? (uint32_t) best_d + 119 : code_of((int64_t) best_d);
			push_copy(enc, sp, ctx[i], (uint32_t) best_len, code);
			account_copy(st, i, (int64_t) best_d, best_len, lp.dist_mult ? code : 120, n, row_of, chan_of);
			for (size_t k = 0; k < best_len; ++k) remember(i + k);
			i += best_len;
		} else {
			push_literal(enc, sp, ctx[i], val[i]);
			remember(i);
			++i;
		}
	}
	st.max_section_integers = std::max<uint64_t>(st.max_section_integers, n);
}

// Forced copies: the stream is a script of literals and copies, and the integers are whatever a reader makes of it (returned, `need`
// of them). Every symbol is read with context `ctx` (the caller's tree has one leaf).
inline std::vector<uint32_t> lz77_forced(StreamEncoder &enc, const CodeSpecW &sp, const LzParams &lp, uint32_t ctx, size_t need, SplitMix64 &rng,
                                         const std::vector<uint32_t> &row_of, const std::vector<uint32_t> &chan_of, LzStats &st) {
	std::vector<uint32_t> win;
	win.reserve(need + 1024);
	const uint32_t min_len = (uint32_t) sp.lz_min_length;
	const int64_t M = lp.dist_mult;
	if (M <= 0) die("lzforce: the stream has no distance multiplier");
	auto literal = [&]() { const uint32_t v = 2 * rng.below(lp.literal_range); push_literal(enc, sp, ctx, v); win.push_back(v); };
	auto copy = [&](uint32_t len, uint32_t code) {
		const int64_t nominal = code < 120 ? special_distance((int) code, M) : (int64_t) code - 119;
		const size_t pos = win.size();
		const size_t eff = (size_t) std::min<int64_t>(std::min<int64_t>(nominal, (int64_t) pos), 1 << 20);
		push_copy(enc, sp, ctx, len, code);
		account_copy(st, pos, nominal, len, code, need, row_of, chan_of);
		for (uint32_t k = 0; k < len; ++k) win.push_back(eff ? win[win.size() - eff] : 0);
	};
	auto copy_that_fits = [&](uint32_t len, uint32_t code) {   // (false: fewer than min_length integers are left)
		const size_t left = need - win.size();
		if (left < min_len) return false;
		copy((uint32_t) std::min<size_t>(len, left), code);
		return true;
	};
	const uint32_t len_span = (uint32_t) std::min<int64_t>(3 * M, 300) + 6;
	int next_code = 0;
	if (lp.force == FORCE_EARLY) {
		// a copy as the very first symbol (zeros), then copies whose distances lie beyond what has been decoded: special codes from the
		// far end of the table and plain distances, one literal between them
		copy_that_fits(min_len + 2 + rng.below(5), 0);
		for (int k = 0; k < 60 && win.size() + 2 * min_len + 8 < need; ++k) {
			literal();
			const uint32_t code = k % 3 == 2 ? 119 + 1000 + 37 * (uint32_t) k : k % 3 == 1 ? 119 + (uint32_t) win.size() + 1 + (uint32_t) k : 119 - (uint32_t) (k % 40);
			copy_that_fits(min_len + rng.below(4), code);
		}
	} else if (lp.force == FORCE_FAR) {
		// a section of more than 2^20 integers (the reference's window has wrapped): blocks of literals, long copies at any distance,
		// and beyond 2^20 integers copies whose plain distance lies just below, at and above 2^20 (the last is clamped to it)
		while (win.size() < need) {
			for (int k = 0; k < 40 && win.size() < need; ++k) literal();
			const size_t pos = win.size();
			if (pos >= need) break;
			uint32_t d;
			const uint32_t pick = rng.below(4);
			if (pos > ((size_t) 1 << 20) + 8192 && pick < 3) d = (1u << 20) - 3000 + (pick == 0 ? 3000 + rng.below(6) : rng.below(3000));
			else d = 1 + rng.below((uint32_t) std::min<size_t>(pos, (1u << 20) - 1));
			if (!copy_that_fits(min_len + 300 + rng.below(3000), d + 119)) literal();
		}
	} else {
		const int64_t warm = std::min<int64_t>(special_distance(119, M) + 1, (int64_t) need / 3);
		while ((int64_t) win.size() < warm) literal();
	}
	while (win.size() < need) {
		const uint32_t len = min_len + rng.below(len_span);
		const size_t left = need - win.size();
		if (lp.force == FORCE_OVER && left < min_len + len_span) { copy((uint32_t) left + 50, (uint32_t) next_code); break; }
		if (!copy_that_fits(len, (uint32_t) next_code)) { literal(); continue; }
		next_code = (next_code + 1) % 120;
		for (uint32_t k = 1 + rng.below(3); k > 0 && win.size() < need; --k) literal();
	}
	st.max_section_integers = std::max<uint64_t>(st.max_section_integers, win.size());
	win.resize(need);
	return win;
}

} // namespace synth
