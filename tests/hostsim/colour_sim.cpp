// tests/hostsim/colour_sim.cpp -- the colour mode's tail on the CPU (tests/test_colour.py, tests/test_colour_gpu.py): device/colour_dev.h
// compiled for the host over planes in host memory, with colour_space.hpp's curve and threshold table -- the functions k_colour_tail
// runs, so the device's bytes are held against these. TEST INFRASTRUCTURE.
#include <cstdint>
#include <cstring>
#include <thread>
#include <vector>
#include "../../j40_amd/csrc/colour_space.hpp"

using namespace j40hip;

static ColourCurve curve_from(const int32_t *enc, float it, const float *lum) {
	const ColourEncoding ce = colour::encoding_from_words(enc);
	const double l[3] = {lum ? lum[0] : 0.2126, lum ? lum[1] : 0.7152, lum ? lum[2] : 0.0722};
	return colour::curve_of(ce, it, l);
}

template <int TF>
static void tail_of(const float *xyb, int32_t w, int32_t h, const ColourTailParams &p, bool use_table, bool rgba16, uint8_t *out, size_t stride) {
	const size_t plane = (size_t) w * (size_t) h;
	for (int32_t y = 0; y < h; ++y) for (int32_t x = 0; x < w; ++x) {
		const size_t i = (size_t) y * (size_t) w + (size_t) x;
		if (rgba16) {
			const uint64_t px = colour_tail_pixel<TF, true>(xyb[i], xyb[plane + i], xyb[2 * plane + i], p.cc, p.curve, use_table, p.table, p.blo, p.bhi);
			memcpy(out + (size_t) y * stride + (size_t) x * 8, &px, 8);
		} else {
			const uint32_t px = (uint32_t) colour_tail_pixel<TF, false>(xyb[i], xyb[plane + i], xyb[2 * plane + i], p.cc, p.curve, use_table, p.table, p.blo, p.bhi);
			memcpy(out + (size_t) y * stride + (size_t) x * 4, &px, 4);
		}
	}
}

// j40hip_kat_device_colour_tail's arguments, host memory; returns 1 where an 8-bit frame took the table, 0 where the curve, -1: bad arguments
extern "C" int32_t colour_sim_tail(const float *xyb, int32_t w, int32_t h, const float *cc15, const int32_t *enc, const float *lum, int32_t bpp, int32_t use_table, int32_t rgba16, uint8_t *out, size_t stride) {
	if (!xyb || !cc15 || !enc || !lum || !out || w <= 0 || h <= 0 || bpp < 8 || bpp > 16 || stride < (size_t) w * (rgba16 ? 8 : 4)) return -1;
	ColourTailParams p;
	memset(&p, 0, sizeof p);
	for (int c = 0; c < 3; ++c) { p.cc.opsin_bias[c] = cc15[9 + c]; p.cc.cbrt_opsin_bias[c] = cbrtf(cc15[9 + c]); }
	for (int i = 0; i < 9; ++i) p.cc.m[i] = cc15[i];
	p.cc.itscale = 255.0f / cc15[12]; p.cc.bpp = bpp;
	p.curve = curve_from(enc, cc15[12], lum);
	std::vector<float> table;
	const bool tabled = bpp == 8 && use_table && colour::build_table(p.curve, &table, &p.blo, &p.bhi);
	p.table = tabled ? table.data() : nullptr;
	switch (p.curve.tf) {
	case CTF_LINEAR: tail_of<CTF_LINEAR>(xyb, w, h, p, tabled, rgba16 != 0, out, stride); break;
	case CTF_SRGB: tail_of<CTF_SRGB>(xyb, w, h, p, tabled, rgba16 != 0, out, stride); break;
	case CTF_BT709: tail_of<CTF_BT709>(xyb, w, h, p, tabled, rgba16 != 0, out, stride); break;
	case CTF_GAMMA: tail_of<CTF_GAMMA>(xyb, w, h, p, tabled, rgba16 != 0, out, stride); break;
	case CTF_PQ: tail_of<CTF_PQ>(xyb, w, h, p, tabled, rgba16 != 0, out, stride); break;
	default: tail_of<CTF_HLG>(xyb, w, h, p, tabled, rgba16 != 0, out, stride); break;
	}
	return tabled ? 1 : 0;
}

// the long way: the level at bpp of every v[i]
extern "C" void colour_sim_levels(const int32_t *enc, float it, const float *v, int64_t n, int32_t bpp, int32_t *out) {
	const ColourCurve k = curve_from(enc, it, nullptr);
	for (int64_t i = 0; i < n; ++i) out[i] = colour::level_of(k, v[i], bpp);
}

// BT.2100's inverse OOTF on n triples, in place
extern "C" void colour_sim_hlg_ootf(const int32_t *enc, float it, const float *lum, float *v, int64_t n) {
	const ColourCurve k = curve_from(enc, it, lum);
	for (int64_t i = 0; i < n; ++i) colour_hlg_inverse_ootf(v + 3 * i, k);
}

// x^p and ln x as the curves compute them
extern "C" void colour_sim_pow(const double *x, const double *p, int64_t n, double *out) { for (int64_t i = 0; i < n; ++i) out[i] = colour_pow(x[i], p[i]); }

// The threshold table against the long way. out[0]: 1 a table exists, [1] blo, [2] bhi, [3] floats compared, [4] floats whose lookup
// differs from the long way, [5] the first such float's bits. Every float of the table's range -- bucket blo's first to bucket bhi's last
// -- where step = 1 (else every step-th), and outside it: zeros, negatives, subnormals, the floats below and above the range in
// strides, infinities and NaNs. thr (optional): the table's 258 thresholds.
extern "C" void colour_sim_table_check(const int32_t *enc, float it, int32_t step, int32_t threads, int64_t *out, float *thr) {
	memset(out, 0, sizeof(int64_t) * 6);
	const ColourCurve k = curve_from(enc, it, nullptr);
	std::vector<float> table; int32_t blo = 0, bhi = 0;
	if (!colour::build_table(k, &table, &blo, &bhi)) return;
	out[0] = 1; out[1] = blo; out[2] = bhi;
	if (thr) memcpy(thr, table.data(), sizeof(float) * COLOUR_THRESHOLDS);
	auto from_bits = [](uint32_t u) { float f; memcpy(&f, &u, 4); return f; };
	const uint32_t first = (uint32_t) blo << 16, last = ((uint32_t) bhi << 16) | 0xffffu;
	if (step < 1) step = 1;
	if (threads < 1) threads = 1;
	std::vector<int64_t> bad((size_t) threads, 0), seen((size_t) threads, 0);
	std::vector<uint32_t> first_bad((size_t) threads, 0);
	auto check = [&](int t, uint32_t u) {
		const float v = from_bits(u);
		++seen[(size_t) t];
		if (colour_u8_from_thresholds(v, table.data(), blo, bhi) != colour::level_of(k, v, 8)) { if (!bad[(size_t) t]) first_bad[(size_t) t] = u; ++bad[(size_t) t]; }
	};
	auto work = [&](int t) {
		const uint64_t span = (uint64_t) last - first + 1, lo = span * (uint64_t) t / (uint64_t) threads, hi = span * (uint64_t) (t + 1) / (uint64_t) threads;
		for (uint64_t o = lo; o < hi; o += (uint64_t) step) check(t, first + (uint32_t) o);
		if (hi > lo) check(t, first + (uint32_t) (hi - 1));
	};
	std::vector<std::thread> pool;
	for (int t = 1; t < threads; ++t) pool.emplace_back(work, t);
	work(0);
	for (auto &th : pool) th.join();
	// outside the range
	for (uint32_t u = 0; u < first; u += 9973) check(0, u);
	for (uint32_t u = last; u < 0x7f800000u; u += 9973) check(0, u);
	for (uint32_t u : {0u, 1u, 0x007fffffu, 0x00800000u, first - 1, last + 1, 0x7f7fffffu, 0x7f800000u, 0x7fc00000u, 0x7f800001u, 0x80000000u, 0x80000001u, 0xbf800000u, 0xff800000u, 0xffc00000u}) check(0, u);
	for (uint32_t u = 0x80000000u; u < 0xff800000u; u += 1000003) check(0, u);
	for (int t = 0; t < threads; ++t) { out[3] += seen[(size_t) t]; if (bad[(size_t) t] && !out[4]) out[5] = first_bad[(size_t) t]; out[4] += bad[(size_t) t]; }
}
