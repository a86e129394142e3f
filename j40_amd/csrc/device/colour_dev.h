// j40_amd/csrc/device/colour_dev.h -- the colour tail that renders an XYB image in the colour space its header signals
// (j40hip_frame_set_colour; colour_space.hpp has the host's half: the gamut matrix, the curve of a ColourEncoding, the threshold table).
// Per-lane functions, compiled for the device (colour_kernels.hip) and for the host (tests/hostsim/colour_sim.cpp): both give the same bytes.
//
// The tail keeps the shape of xyb_to_rgba8 (idct_dev.h): per channel a cube plus bias, then one 3x3 in float32 -- the matrix is the
// frame's inverse opsin matrix with the gamut matrix folded in on the host. The linear value v (1.0: intensity_target nits) then goes
// through the signalled transfer curve to f in [0, 1], and level = floor(maxpixel * f + 0.5) at the frame's bit depth; u8 and u16 are
// the existing reductions of a level. The reference's int16 wrap-around does not exist here: v <= 0 and NaN give 0, large v gives maxpixel.
//
// The curves are evaluated in float64 with a logarithm and an exponential of this file's own (a reduction and a polynomial each, every
// operation an IEEE one with explicit fma): the relative error of x^p is ~1e-14, against the 1.5e-8 that half of 2^-10 of a 16-bit
// level asks for -- PQ raises a ratio to the power 78.84, a float32 exp2(p * log2 x) is several 16-bit levels off. No hardware
// transcendental enters (v_log_f32 / v_exp_f32 differ from a host libm in their last bits; a seed from them would leave the host build
// and the device build one level apart once in ~10^7 samples, as pow_1_over_2p4 is): the host build is the device build, bit for bit.
// 8-bit frames do not evaluate a curve at all: a per-frame threshold table (colour_u8_from_thresholds) as srgb_u8_from_thresholds has it.
#pragma once
#include "entropy_dev.h"
#include "idct_dev.h"

namespace j40hip {

// DCI (x^(1/2.6)) and have_gamma (x^(gamma / 1e7)) are one curve with two exponents
enum ColourTF : int32_t { CTF_LINEAR = 0, CTF_SRGB = 1, CTF_BT709 = 2, CTF_GAMMA = 3, CTF_PQ = 4, CTF_HLG = 5, CTF_COUNT = 6 };

struct ColourCurve {
	int32_t tf;
	float lum[3];       // CTF_HLG: the luminance of the three target-space values (the Y row of the target primaries)
	double g;           // CTF_GAMMA: the exponent
	double pq_scale;    // CTF_PQ: intensity_target / 10000
	double hlg_exp;     // CTF_HLG: 1 / gamma - 1 of the inverse OOTF, gamma = 1.2 * 1.111^log2(intensity_target / 1000)
};

// three float planes, `pitch` floats per row: restore_kernels.h's XybPlanes, member for member (that header belongs to kernels.hip's translation unit)
struct ColourPlanes { const float *p[3]; size_t pitch; };

// the threshold table of one (curve, intensity_target): 258 thresholds as srgb_u8_from_thresholds', then one byte per bucket (the floats that
// share their top 16 bits) from bucket `blo` to bucket `bhi` -- the range is the curve's: PQ has 8-bit levels down to 2^-27
enum { COLOUR_THRESHOLDS = 258, COLOUR_BUCKETS_MAX = 48 * 128, COLOUR_TABLE_FLOATS = COLOUR_THRESHOLDS + COLOUR_BUCKETS_MAX / 4 };

struct ColourTailParams {
	ColourConsts cc;        // m: the gamut matrix times the inverse opsin matrix
	ColourCurve curve;
	const float *table;     // device memory (the host build: host memory), null: no table, every depth evaluates the curve
	int32_t blo, bhi, table_floats;
};

// the curve and the level serve the host as well in a HIP translation unit: the threshold table is built from them (colour_space.hpp)
#ifdef __HIPCC__
#define J40_HD __host__ __device__ __forceinline__
#else
#define J40_HD static inline
#endif

J40_HD double colour_f64_from_bits(uint64_t u) { double d; __builtin_memcpy(&d, &u, 8); return d; }
J40_HD uint64_t colour_bits_from_f64(double d) { uint64_t u; __builtin_memcpy(&u, &d, 8); return u; }

// ln x for a positive, finite, normal x (a float's value always is, as a double): x = 2^e * m with m in [sqrt(1/2), sqrt 2),
// ln m = 2 atanh s, s = (m - 1) / (m + 1), |s| <= 0.1716: the series to s^23 leaves 6e-19
J40_HD double colour_ln(double x) {
	const uint64_t bits = colour_bits_from_f64(x);
	int32_t e = (int32_t) (bits >> 52 & 0x7ff) - 1023;
	double m = colour_f64_from_bits((bits & 0x000fffffffffffffull) | 0x3ff0000000000000ull);
	if (m > 1.4142135623730951) { m *= 0.5; e += 1; }
	const double s = (m - 1.0) / (m + 1.0), z = s * s;
	double p = 1.0 / 23.0;
	p = fma(p, z, 1.0 / 21.0); p = fma(p, z, 1.0 / 19.0); p = fma(p, z, 1.0 / 17.0); p = fma(p, z, 1.0 / 15.0); p = fma(p, z, 1.0 / 13.0);
	p = fma(p, z, 1.0 / 11.0); p = fma(p, z, 1.0 / 9.0); p = fma(p, z, 1.0 / 7.0); p = fma(p, z, 1.0 / 5.0); p = fma(p, z, 1.0 / 3.0);
	const double lnm = fma(2.0 * s * z, p, 2.0 * s);
	return fma((double) e, 0.6931471805599453, lnm);
}

// e^t: t = n ln 2 + r, |r| <= 0.3466, the Taylor polynomial to r^13 (1.7e-16 left), times 2^n. Outside [-700, 700]: as at the ends
J40_HD double colour_exp(double t) {
	if (!(t == t)) return 0.0;
	t = t < -700.0 ? -700.0 : t > 700.0 ? 700.0 : t;
	const double n = rint(t * 1.4426950408889634);
	double r = fma(-n, 6.93147180369123816490e-01, t);
	r = fma(-n, 1.90821492927058770002e-10, r);
	double p = 1.0 / 6227020800.0;
	p = fma(p, r, 1.0 / 479001600.0); p = fma(p, r, 1.0 / 39916800.0); p = fma(p, r, 1.0 / 3628800.0); p = fma(p, r, 1.0 / 362880.0);
	p = fma(p, r, 1.0 / 40320.0); p = fma(p, r, 1.0 / 5040.0); p = fma(p, r, 1.0 / 720.0); p = fma(p, r, 1.0 / 120.0);
	p = fma(p, r, 1.0 / 24.0); p = fma(p, r, 1.0 / 6.0); p = fma(p, r, 0.5); p = fma(p, r, 1.0); p = fma(p, r, 1.0);
	return p * colour_f64_from_bits((uint64_t) ((int64_t) n + 1023) << 52);   // (n in [-1010, 1010]: a normal power of two)
}
// x^p, x > 0
J40_HD double colour_pow(double x, double p) { return colour_exp(p * colour_ln(x)); }

// the transfer curve: the linear value (a float32, as the 3x3 leaves it) to f in [0, 1], float64
template <int TF> J40_HD double colour_transfer(float vf, const ColourCurve &k) {
	if (!(vf > 0.0f)) return 0.0;   // (negative values and NaN)
	const double v = vf > 3.4028234e38f ? 3.4028234663852886e38 : (double) vf;   // (+inf: as the largest float)
	double f;
	if (TF == CTF_LINEAR) f = v;
	else if (TF == CTF_SRGB) f = v <= 0.0031308 ? 12.92 * v : 1.055 * colour_pow(v, 1.0 / 2.4) - 0.055;
	else if (TF == CTF_BT709) f = v < 0.018 ? 4.5 * v : 1.099 * colour_pow(v, 0.45) - 0.099;
	else if (TF == CTF_GAMMA) f = colour_pow(v, k.g);
	else if (TF == CTF_PQ) {   // SMPTE ST 2084
		const double ym = colour_pow(v * k.pq_scale, 2610.0 / 16384.0);
		f = colour_pow((3424.0 / 4096.0 + 2413.0 / 128.0 * ym) / (1.0 + 2392.0 / 128.0 * ym), 2523.0 / 32.0);
	} else {   // BT.2100 HLG OETF (the inverse OOTF has run: colour_hlg_inverse_ootf)
		const double a = 0.17883277, b = 1.0 - 4.0 * a, c = 0.5 - a * -0.3350097945111627;   // (ln 4a)
		f = v <= 1.0 / 12.0 ? colour_exp(0.5 * colour_ln(3.0 * v)) : a * colour_ln(12.0 * v - b) + c;
	}
	return f > 1.0 ? 1.0 : f > 0.0 ? f : 0.0;   // (NaN: 0)
}

// the level at bit depth bpp of f in [0, 1]
J40_HD int32_t colour_level(double f, int32_t bpp) {
	const int32_t maxpixel = (1 << bpp) - 1;
	const int32_t l = (int32_t) ((double) maxpixel * f + 0.5);
	return l < 0 ? 0 : l > maxpixel ? maxpixel : l;
}
template <int TF> J40_HD int32_t colour_level_of(float v, int32_t bpp, const ColourCurve &k) { return colour_level(colour_transfer<TF>(v, k), bpp); }

// BT.2100's inverse OOTF on the three target-space values: each times Yd^(1 / gamma - 1), Yd their luminance; nothing where Yd <= 0
J40_DEV void colour_hlg_inverse_ootf(float v[3], const ColourCurve &k) {
	const float yd = v[0] * k.lum[0] + v[1] * k.lum[1] + v[2] * k.lum[2];
	if (!(yd > 0.0f) || !(yd < 3.0e38f)) return;
	const float s = (float) colour_pow((double) yd, k.hlg_exp);
	for (int c = 0; c < 3; ++c) v[c] *= s;
}

// the 8-bit level by table: srgb_u8_from_thresholds with the table's own bucket range; v <= 0 and NaN are 0 as on the long way. The
// thresholds no float reaches (thr[256], thr[257] among them) are NaN: the comparison is false for every v, +inf too
J40_DEV int32_t colour_u8_from_thresholds(float v, const J40_LDS float *thr, int32_t blo, int32_t bhi) {
	if (!(v > 0.0f)) return 0;
	int32_t bits;
#ifdef __HIPCC__
	bits = __float_as_int(v);
#else
	memcpy(&bits, &v, 4);
#endif
	int32_t b = bits >> 16;
	b = (b < blo ? blo : b > bhi ? bhi : b) - blo;
	const int32_t k = ((const J40_LDS uint8_t *) (thr + COLOUR_THRESHOLDS))[b];
	return k + (int32_t) (v >= thr[k + 1]);
}

// One pixel: XYB samples to RGBA. OUT16: four u16 (R in the low 16 bits, A = 65535), else four u8 in the low 32 bits (A = 255).
// use_table: 8-bit frames take `thr` (never tested for null: idct_dev.h says why)
template <int TF, bool OUT16>
J40_DEV uint64_t colour_tail_pixel(float sx, float sy, float sb, const ColourConsts &f, const ColourCurve &k, bool use_table, const J40_LDS float *thr, int32_t blo, int32_t bhi) {
	const float p[3] = {sy + sx, sy - sx, sb};
	float s[3], v[3];
#pragma unroll
	for (int c = 0; c < 3; ++c) {
		const float pp = p[c] - f.cbrt_opsin_bias[c];
		s[c] = (pp * pp * pp + f.opsin_bias[c]) * f.itscale;
	}
#pragma unroll
	for (int c = 0; c < 3; ++c) v[c] = s[0] * f.m[c * 3] + s[1] * f.m[c * 3 + 1] + s[2] * f.m[c * 3 + 2];
	if (TF == CTF_HLG) colour_hlg_inverse_ootf(v, k);
	int32_t l[3];
	if (use_table) {
#pragma unroll
		for (int c = 0; c < 3; ++c) l[c] = colour_u8_from_thresholds(v[c], thr, blo, bhi);
	} else {
#pragma unroll
		for (int c = 0; c < 3; ++c) l[c] = colour_level_of<TF>(v[c], f.bpp, k);
	}
	if (OUT16) {
		uint32_t o[3];
#pragma unroll
		for (int c = 0; c < 3; ++c) o[c] = scale_to_u16(l[c], f.bpp);
		return (uint64_t) (o[0] | (o[1] << 16)) | (uint64_t) (o[2] | 0xffff0000u) << 32;
	}
	const int32_t maxpixel = (1 << f.bpp) - 1, half = 1 << (f.bpp - 1);
	uint32_t out = 0xff000000u;
#pragma unroll
	for (int c = 0; c < 3; ++c) out |= (uint32_t) ((l[c] * 255 + half) / maxpixel) << (8 * c);
	return out;
}

} // namespace j40hip

#undef J40_HD
