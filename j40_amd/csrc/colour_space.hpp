// j40_amd/csrc/colour_space.hpp -- the host's half of the colour mode (j40hip_frame_set_colour): what a parsed ColourEncoding means.
// The gamut matrix from linear sRGB / D65 to the signalled primaries and white point, the transfer curve the tail evaluates
// (device/colour_dev.h), the per-frame threshold table of 8-bit frames, and which images the mode refuses. Plain C++, float64; no HIP.
// The chromaticities and curves are those of BT.709, BT.2100, SMPTE 428 / 431, sRGB and ST 2084. PARITY UNPINNED: no decoder at hand
// pins libjxl's conventions -- above all the HLG inverse OOTF.
#pragma once
#include "frame.hpp"
#include "device/colour_dev.h"
#include <cmath>
#include <vector>

namespace j40hip {
namespace colour {

constexpr uint32_t ERR_UCS = (uint32_t) 'U' << 24 | (uint32_t) 'c' << 16 | (uint32_t) 's' << 8 | (uint32_t) '?';   // the colour mode does not serve this image

inline void mul3(const double a[3][3], const double b[3][3], double r[3][3]) {
	double t[3][3];
	for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) t[i][j] = a[i][0] * b[0][j] + a[i][1] * b[1][j] + a[i][2] * b[2][j];
	for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) r[i][j] = t[i][j];
}
inline bool invert3(const double a[3][3], double r[3][3]) {
	double c[3][3];
	for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j)
		c[i][j] = a[(j + 1) % 3][(i + 1) % 3] * a[(j + 2) % 3][(i + 2) % 3] - a[(j + 1) % 3][(i + 2) % 3] * a[(j + 2) % 3][(i + 1) % 3];
	const double det = a[0][0] * c[0][0] + a[0][1] * c[1][0] + a[0][2] * c[2][0];
	if (!(std::fabs(det) > 1e-12) || !std::isfinite(det)) return false;
	for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) r[i][j] = c[i][j] / det;
	return true;
}
inline bool xy_to_xyz(const double xy[2], double xyz[3]) {
	if (!(std::fabs(xy[1]) > 1e-9)) return false;
	xyz[0] = xy[0] / xy[1]; xyz[1] = 1.0; xyz[2] = (1.0 - xy[0] - xy[1]) / xy[1];
	return true;
}

// the chromaticities in the unit: the stream's integers / 1e6; the white point E is (1/3, 1/3) exactly
inline void chromaticities(const ColourEncoding &ce, double white[2], double prim[3][2]) {
	for (int i = 0; i < 2; ++i) white[i] = ce.white_point == 10 ? 1.0 / 3.0 : (double) ce.white_xy[i] / 1e6;
	for (int c = 0; c < 3; ++c) for (int i = 0; i < 2; ++i) prim[c][i] = (double) ce.prim_xy[c][i] / 1e6;
}

// RGB -> XYZ of a set of primaries with a white point: the primaries' XYZ columns scaled so that (1, 1, 1) is the white (Y = 1)
inline bool rgb_to_xyz(const double prim[3][2], const double white[2], double m[3][3]) {
	double p[3][3], pinv[3][3], w[3];
	for (int c = 0; c < 3; ++c) { double v[3]; if (!xy_to_xyz(prim[c], v)) return false; for (int i = 0; i < 3; ++i) p[i][c] = v[i]; }
	if (!xy_to_xyz(white, w) || !invert3(p, pinv)) return false;
	for (int c = 0; c < 3; ++c) {
		const double s = pinv[c][0] * w[0] + pinv[c][1] * w[1] + pinv[c][2] * w[2];
		for (int i = 0; i < 3; ++i) m[i][c] = p[i][c] * s;
	}
	return true;
}

// Bradford chromatic adaptation, XYZ under `from` to XYZ under `to`
inline bool bradford(const double from[2], const double to[2], double a[3][3]) {
	static const double B[3][3] = {{0.8951, 0.2664, -0.1614}, {-0.7502, 1.7135, 0.0367}, {0.0389, -0.0685, 1.0296}};
	double binv[3][3], wf[3], wt[3], d[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}};
	if (!invert3(B, binv) || !xy_to_xyz(from, wf) || !xy_to_xyz(to, wt)) return false;
	for (int i = 0; i < 3; ++i) {
		const double cf = B[i][0] * wf[0] + B[i][1] * wf[1] + B[i][2] * wf[2], ct = B[i][0] * wt[0] + B[i][1] * wt[1] + B[i][2] * wt[2];
		if (!(std::fabs(cf) > 1e-12)) return false;
		d[i][i] = ct / cf;
	}
	mul3(d, B, a); mul3(binv, a, a);
	return true;
}

// P: linear sRGB / D65 -> the encoding's primaries and white point; lum: the luminance of the three target-space values. false: the
// chromaticities span no colour space (custom values on one line, y = 0)
inline bool gamut_matrix(const ColourEncoding &ce, double p[3][3], double lum[3]) {
	static const double SRGB[3][2] = {{0.64, 0.33}, {0.30, 0.60}, {0.15, 0.06}}, D65[2] = {0.3127, 0.3290};
	double white[2], prim[3][2], src[3][3], dst[3][3], dinv[3][3], adapt[3][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}};
	chromaticities(ce, white, prim);
	if (!rgb_to_xyz(SRGB, D65, src) || !rgb_to_xyz(prim, white, dst) || !invert3(dst, dinv)) return false;
	if (white[0] != D65[0] || white[1] != D65[1]) { if (!bradford(D65, white, adapt)) return false; }
	mul3(adapt, src, p); mul3(dinv, p, p);
	for (int c = 0; c < 3; ++c) { lum[c] = dst[1][c]; if (!std::isfinite(lum[c])) return false; }
	for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) if (!std::isfinite(p[i][j])) return false;
	return true;
}

// an encoding from the 16 words j40hip_frame_colour_encoding states it in (include/j40hip.h)
inline ColourEncoding encoding_from_words(const int32_t w[16]) {
	ColourEncoding ce;
	ce.colour_space = w[0]; ce.white_point = w[1]; ce.white_xy[0] = w[2]; ce.white_xy[1] = w[3]; ce.primaries = w[4];
	for (int c = 0; c < 3; ++c) { ce.prim_xy[c][0] = w[5 + 2 * c]; ce.prim_xy[c][1] = w[6 + 2 * c]; }
	ce.have_gamma = w[11] != 0; ce.gamma = w[12]; ce.transfer = w[13]; ce.intent = w[14];
	return ce;
}

// the curve the tail evaluates for an encoding (transfer function 2, "unknown", has none: colour_refusal)
inline ColourCurve curve_of(const ColourEncoding &ce, float intensity_target, const double lum[3]) {
	ColourCurve k;
	memset(&k, 0, sizeof k);
	const int32_t tf = ce.transfer;
	k.tf = ce.have_gamma ? CTF_GAMMA : tf == 8 ? CTF_LINEAR : tf == 1 ? CTF_BT709 : tf == 17 ? CTF_GAMMA : tf == 16 ? CTF_PQ : tf == 18 ? CTF_HLG : CTF_SRGB;
	k.g = ce.have_gamma ? (double) ce.gamma / 1e7 : 1.0 / 2.6;
	k.pq_scale = (double) intensity_target / 10000.0;
	const double gamma = 1.2 * std::pow(1.111, std::log2((double) intensity_target / 1000.0));
	k.hlg_exp = 1.0 / gamma - 1.0;
	for (int c = 0; c < 3; ++c) k.lum[c] = (float) lum[c];
	return k;
}

// 0, or "Ucs?": the profile is not interpreted (want_icc), no curve is known (transfer function 2), a grey image, an image whose
// colour space is not RGB, chromaticities that span nothing. An image with xyb_encoded = 0 holds samples in its signalled space
// already: never refused, the mode changes nothing for it
inline uint32_t image_refusal(const ImageMeta &im) {
	if (!im.xyb_encoded) return 0;
	const ColourEncoding &ce = im.cenc;
	if (im.want_icc || im.grey || ce.colour_space != 0 || (!ce.have_gamma && ce.transfer == 2)) return ERR_UCS;
	double p[3][3], lum[3];
	return gamut_matrix(ce, p, lum) ? 0 : ERR_UCS;
}

inline int32_t level_of(const ColourCurve &k, float v, int32_t bpp) {
	switch (k.tf) {
	case CTF_LINEAR: return colour_level_of<CTF_LINEAR>(v, bpp, k);
	case CTF_SRGB: return colour_level_of<CTF_SRGB>(v, bpp, k);
	case CTF_BT709: return colour_level_of<CTF_BT709>(v, bpp, k);
	case CTF_GAMMA: return colour_level_of<CTF_GAMMA>(v, bpp, k);
	case CTF_PQ: return colour_level_of<CTF_PQ>(v, bpp, k);
	default: return colour_level_of<CTF_HLG>(v, bpp, k);
	}
}

// The threshold table of 8-bit frames (colour_u8_from_thresholds): thr[k] = the smallest positive float whose level is >= k, by
// bisection over the floats from the curve itself, as tables.cpp builds the sRGB one; NaN where no float reaches k. The buckets run
// from the one that holds thr[1] to the one behind the last finite threshold. false -- and no table: the tail evaluates the curve --
// where a bucket would span more than one step or the range more than COLOUR_BUCKETS_MAX buckets (a gamma of next to nothing).
inline bool build_table(const ColourCurve &k, std::vector<float> *table, int32_t *blo, int32_t *bhi) {
	auto from_bits = [](uint32_t u) { float f; memcpy(&f, &u, 4); return f; };
	auto to_bits = [](float f) { uint32_t u; memcpy(&u, &f, 4); return u; };
	std::vector<float> t((size_t) COLOUR_TABLE_FLOATS, 0.0f);
	const uint32_t top = 0x7f7fffffu;   // the largest finite float
	t[0] = -INFINITY; t[256] = t[257] = NAN;
	int last = 0;
	for (int lv = 1; lv <= 255; ++lv) {
		if (level_of(k, from_bits(top), 8) < lv) { t[(size_t) lv] = NAN; continue; }
		uint32_t lo = 0, hi = top;   // level(lo) < lv <= level(hi)
		while (hi - lo > 1) { const uint32_t mid = lo + (hi - lo) / 2; if (level_of(k, from_bits(mid), 8) >= lv) hi = mid; else lo = mid; }
		t[(size_t) lv] = from_bits(hi);
		last = lv;
	}
	if (last == 0) return false;
	const int32_t lo_b = (int32_t) (to_bits(t[1]) >> 16), hi_b = (int32_t) (to_bits(t[(size_t) last]) >> 16) + 1;
	if (hi_b - lo_b + 1 > COLOUR_BUCKETS_MAX || hi_b > 0x7f7f) return false;
	uint8_t *bucket = (uint8_t *) (t.data() + COLOUR_THRESHOLDS);
	int prev = 0;
	for (int32_t b = 0; b <= hi_b - lo_b; ++b) {
		const float low = from_bits((uint32_t) (b + lo_b) << 16);
		int lv = 0; while (lv < 255 && t[(size_t) lv + 1] <= low) ++lv;
		if (b == 0) lv = 0;   // (it also takes everything below: thr[1] lies inside it)
		if (lv - prev > 1) return false;   // the bucket before spans more than one step: one comparison would not settle it
		bucket[b] = (uint8_t) lv; prev = lv;
	}
	if (last - prev > 0) return false;   // (the last bucket lies behind the last finite threshold)
	table->swap(t);
	*blo = lo_b; *bhi = hi_b;
	return true;
}

// the tail's frame constants: DevFrame's colour constants with the gamut matrix folded into the inverse opsin matrix, m' = (float) (P m)
inline bool tail_consts(const ImageMeta &im, ColourConsts *cc, ColourCurve *curve) {
	double p[3][3], lum[3];
	if (!gamut_matrix(im.cenc, p, lum)) return false;
	for (int c = 0; c < 3; ++c) { cc->opsin_bias[c] = im.opsin_bias[c]; cc->cbrt_opsin_bias[c] = cbrtf(im.opsin_bias[c]); }
	for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j)
		cc->m[i * 3 + j] = (float) (p[i][0] * (double) im.opsin_inv_mat[0][j] + p[i][1] * (double) im.opsin_inv_mat[1][j] + p[i][2] * (double) im.opsin_inv_mat[2][j]);
	cc->itscale = 255.0f / im.intensity_target; cc->bpp = im.bpp;
	*curve = curve_of(im.cenc, im.intensity_target, lum);
	return true;
}

} // namespace colour
} // namespace j40hip
