// j40_amd/csrc/device/spline_dev.h -- splines (a frame parsed with J40HIP_PARSE_SPLINES whose header has has_splines): curves drawn as
// Gaussian splats onto the frame's XYB planes behind the patches and ahead of the noise. The rule, the host's dequantisation into
// segments and their tiles, and the per-sample addition the kernel runs. Compiled for the device by spline_kernels.hip, for the host by
// frame.cpp (the parse builds the segments) and for the CPU tests by tests/hostsim/spline_sim.cpp: the same functions.
//
// THE RULE. PARITY UNPINNED: it is libjxl's as far as recalled without the text, and no decoder on hand pins it (the reference stops at
// has_splines, j40.h:6263) -- the constants, the order of the operations and the tile below are this project's statement.
// Everything up to the segments is float64 with the operations in the order written, nothing contracted (-ffp-contract=off); the
// segments are stored as float32.
//   Control points. The first is the starting point; then, in int64, delta += d, cur += delta for every double delta d, and cur is pushed.
//   Scale. inv_q = quant_adjust >= 0 ? 1 / (1 + quant_adjust / 8) : 1 - quant_adjust / 8;
//   coef[c][i] = ((q[c][i] * (i == 0 ? sqrt(0.5) : 1)) * w[c]) * inv_q, w = 0.0042, 0.075, 0.07 for X, Y, B and 0.3333 for sigma; then
//   X[i] += base_corr_x * Y[i], B[i] += base_corr_b * Y[i] (a Modular frame: 0 and 1).
//   Centripetal Catmull-Rom. The control points are extended by p0 + (p0 - p1) in front and pn + (pn - pn-1) behind. For every window
//   p[0..3] of four: emit p[1]; t[0] = 0, t[k] = t[k-1] + sqrt(sqrt(dx * dx + dy * dy)) of p[k] - p[k-1]; for j = 1..15:
//   tt = t[1] + (j / 16) * (t[2] - t[1]); A[k] = p[k] + ((tt - t[k]) / (t[k+1] - t[k])) * (p[k+1] - p[k]) for k = 0..2;
//   B[k] = A[k] + ((tt - t[k]) / (t[k+2] - t[k])) * (A[k+1] - A[k]) for k = 0, 1; emit B[0] + ((tt - t[1]) / (t[2] - t[1])) * (B[1] - B[0]).
//   Finally the last control point is emitted. A single control point gives that one point.
//   Equal spacing at distance 1. Emit (first point, 1). Walk the polyline from `cur` = its first point with `acc` = 0, the arc length
//   since the last emitted point: towards the next polyline point q, len = sqrt(dx * dx + dy * dy) of q - cur; while acc + len >= 1:
//   cur += ((1 - acc) / len) * (q - cur), emit (cur, 1), acc = 0, len anew; then acc += len, cur = q. At the end emit (last polyline
//   point, acc).
//   Arc length and progress. arc = (count - 2) + the last multiplier; a spline with arc <= 0 draws nothing (a one-point spline is one).
//   Point k: progress = min(1, k / arc), t = 31 * progress, value[c] = sum over i ascending of
//   (coef[c][i] * sqrt(2)) * cos((((pi / 32) * i) * (t + 0.5))) for X, Y, B and sigma, from 0.0 (a zero coefficient adds nothing and is
//   skipped).
//   Segment. Skipped when sigma is 0 or not finite, 1 / sigma is not finite or the multiplier is not finite.
//   m = max(0.01, max over c of |colour[c] * multiplier|); d = sqrt(((2 * sigma) * sigma) * (5 * ln 10 + ln m)); the box is
//   x0 = floor((cx - d) + 0.5), x1 = floor((cx + d) + 0.5), y0 and y1 likewise, clipped to the frame; an empty box drops the segment.
//   12 words: x0, x1, y0, y1 (int32), cx, cy, inv_sigma = 1 / sigma, s4 = (0.25 * sigma) * multiplier, colX, colY, colB (float32), a pad.
//   Sample (x, y) of a segment's box, in float32, nothing contracted, division and sqrtf correctly rounded:
//       dx = x - cx; dy = y - cy; dist = sqrtf(dx * dx + dy * dy)
//       f = erf_r((0.5f * dist + 0.35355339f) * inv_sigma) - erf_r((0.5f * dist - 0.35355339f) * inv_sigma)
//       v = s4 * f * f;  P[c] = P[c] + col[c] * v     (c = X, Y, B in that order)
//   erf_r(x), a = |x|: p = (((0.078108f * a + 0.000972f) * a + 0.230389f) * a + 0.278393f) * a + 1; r = 1 - 1 / ((p * p) * (p * p)),
//   with the sign of x (Abramowitz-Stegun 7.1.27, |error| <= 5e-4; libjxl's own constants differ in late digits).
//   THE ORDER OF THE ADDITIONS onto a sample: the segments in ascending index -- the splines in stream order, a spline's points in
//   order along it.
//
// THE KERNEL, k_spline_draw. Splines are a sparse, ordered scatter: a segment touches a few hundred samples anywhere in the frame, and
// float32 additions do not commute. So the host bins the segments: for every SPLINE_TILE_W x SPLINE_TILE_H = 64 x 32 tile a box
// touches, the tile's list keeps the segment's index, ascending (CSR: tile_ids, tile_start, seg_idx); only touched tiles are launched,
// one workgroup of 256 threads each, k_patch_blend's and k_noise_add's shape. Wavefront w owns rows 8w .. 8w + 7 of the tile, a lane one
// column of them: 3 x 8 plane values in registers, read once, written once. The tile's segments are staged in LDS in chunks of
// SPLINE_CHUNK = 128 (6 KiB) and walked in list order by every lane, so every sample's additions happen in ascending segment index:
// no atomics, nothing depends on scheduling. The segment is uniform across the workgroup -- every lane reads the same LDS words, a
// broadcast without bank conflicts --, a wavefront whose eight rows miss the box skips it with a uniform branch, a lane whose column is
// outside [x0, x1] with a predicate.
// THE CHUNK SIZE. Registers limit residency: k_spline_draw takes 128 VGPRs and no scratch, so a SIMD holds 4 of its wavefronts and a
// compute unit four of these workgroups. With 160 KiB of LDS a workgroup could take 40 KiB before LDS became the limit instead; 128
// segments are 6 KiB, well inside that, and six 4-byte words per thread to stage; a chunk costs two barriers against 128 segments'
// work, so a larger chunk would buy nothing measurable and a smaller one only adds barriers to the tiles of a curve that doubles back
// on itself.
#pragma once
#include <stdint.h>
#include <string.h>
#include <math.h>
#ifndef J40_HD
#ifdef __HIPCC__
#define J40_HD __host__ __device__ __forceinline__
#else
#define J40_HD static inline
#endif
#endif
#include <cmath>
#include <vector>

namespace j40hip {

enum { SPLINE_TILE_W = 64, SPLINE_TILE_H = 32, SPLINE_WAVES = 4, SPLINE_ROWS = SPLINE_TILE_H / SPLINE_WAVES, SPLINE_CHUNK = 128, SPLINE_SEG_WORDS = 12,
       SPLINE_MAX_SEGMENTS = 1 << 22, SPLINE_MAX_PAIRS = 1 << 24 };

struct SplineSeg { int32_t x0, x1, y0, y1; float cx, cy, inv_sigma, s4, col[3]; uint32_t pad; };
static_assert(sizeof(SplineSeg) == 4 * SPLINE_SEG_WORDS, "a segment is 12 words");

// the touched tiles of a frame in device memory, as k_spline_draw takes them
struct DevSplines { const SplineSeg *segs; const int32_t *tile_ids, *tile_start, *seg_idx; int32_t num_tiles, tiles_x; };

J40_HD float spline_erf(float x) {
	const float a = fabsf(x);
	const float p = (((0.078108f * a + 0.000972f) * a + 0.230389f) * a + 0.278393f) * a + 1.0f;
	const float r = 1.0f - 1.0f / ((p * p) * (p * p));
	return copysignf(r, x);
}

// the segment's contribution to sample (x, y), which its box holds, onto the sample's three values
J40_HD void spline_splat(const SplineSeg &g, int32_t x, int32_t y, float &X, float &Y, float &B) {
	const float dx = (float) x - g.cx, dy = (float) y - g.cy, dist = sqrtf(dx * dx + dy * dy);
	const float f = spline_erf((0.5f * dist + 0.35355339f) * g.inv_sigma) - spline_erf((0.5f * dist - 0.35355339f) * g.inv_sigma);
	const float v = g.s4 * f * f;
	X = X + g.col[0] * v; Y = Y + g.col[1] * v; B = B + g.col[2] * v;
}

// column x, rows y_first .. y_first + SPLINE_ROWS - 1 (one lane's samples, P[c][r]) under the `n` segments at `segs`, in their order.
// The boxes lie inside the frame, so a sample outside it is never touched.
J40_HD void spline_lane_walk(const SplineSeg *segs, int32_t n, int32_t x, int32_t y_first, float P[3][SPLINE_ROWS]) {
	for (int32_t i = 0; i < n; ++i) {
		const SplineSeg &g = segs[i];
		if (g.y1 < y_first || g.y0 >= y_first + SPLINE_ROWS) continue;   // (uniform across a wavefront)
		if (x < g.x0 || x > g.x1) continue;
#pragma unroll
		for (int32_t r = 0; r < SPLINE_ROWS; ++r) {
			const int32_t y = y_first + r;
			if (y >= g.y0 && y <= g.y1) spline_splat(g, x, y, P[0][r], P[1][r], P[2][r]);
		}
	}
}

// ---- the host's half: from the quantised splines of the stream to segments and their tiles ----
struct QuantSpline {
	int64_t x = 0, y = 0;                 // the starting point
	std::vector<int64_t> dd;              // the double deltas of its further control points, x and y in turn
	int32_t coef[4][32];                  // X, Y, B, sigma
	QuantSpline() { memset(coef, 0, sizeof coef); }
};
struct SplineData { std::vector<QuantSpline> splines; int32_t quant_adjust = 0; };
// the segments the decode draws, and the tiles their boxes touch in CSR form: tile_ids ascending, tile t's segment indices
// seg_idx[tile_start[t] .. tile_start[t + 1]), ascending
struct SplinePlan { std::vector<SplineSeg> segs; std::vector<int32_t> tile_ids, tile_start, seg_idx; int32_t tiles_x = 0; };

struct SplinePoint { double x, y; };

// the control points of a spline; false: a coordinate of magnitude above 1 << 23, or two successive points that are equal
inline bool spline_control_points(const QuantSpline &q, std::vector<SplinePoint> *out) {
	const int64_t lim = (int64_t) 1 << 23;
	int64_t cx = q.x, cy = q.y, dx = 0, dy = 0;
	if (cx > lim || cx < -lim || cy > lim || cy < -lim) return false;
	out->clear();
	out->push_back(SplinePoint{(double) cx, (double) cy});
	for (size_t i = 0; i + 1 < q.dd.size(); i += 2) {
		if (q.dd[i] > 4 * lim || q.dd[i] < -4 * lim || q.dd[i + 1] > 4 * lim || q.dd[i + 1] < -4 * lim) return false;   // (no such step between two points inside the bound; keeps the sums from overflowing)
		dx += q.dd[i]; dy += q.dd[i + 1];
		const int64_t nx = cx + dx, ny = cy + dy;
		if (nx > lim || nx < -lim || ny > lim || ny < -lim || (nx == cx && ny == cy)) return false;
		cx = nx; cy = ny;
		out->push_back(SplinePoint{(double) cx, (double) cy});
	}
	return true;
}

inline void spline_catmull_rom(const std::vector<SplinePoint> &pts, std::vector<SplinePoint> *out) {
	out->clear();
	if (pts.size() == 1) { out->push_back(pts[0]); return; }
	std::vector<SplinePoint> e;
	e.reserve(pts.size() + 2);
	e.push_back(SplinePoint{pts[0].x + (pts[0].x - pts[1].x), pts[0].y + (pts[0].y - pts[1].y)});
	e.insert(e.end(), pts.begin(), pts.end());
	const SplinePoint &l = pts[pts.size() - 1], &k = pts[pts.size() - 2];
	e.push_back(SplinePoint{l.x + (l.x - k.x), l.y + (l.y - k.y)});
	for (size_t w = 0; w + 3 < e.size(); ++w) {
		const SplinePoint *p = &e[w];
		out->push_back(p[1]);
		double t[4];
		t[0] = 0.0;
		for (int i = 1; i < 4; ++i) { const double dx = p[i].x - p[i - 1].x, dy = p[i].y - p[i - 1].y; t[i] = t[i - 1] + sqrt(sqrt(dx * dx + dy * dy)); }
		for (int j = 1; j < 16; ++j) {
			const double tt = t[1] + ((double) j / 16.0) * (t[2] - t[1]);
			SplinePoint A[3], B[2];
			for (int i = 0; i < 3; ++i) {
				const double f = (tt - t[i]) / (t[i + 1] - t[i]);
				A[i].x = p[i].x + f * (p[i + 1].x - p[i].x); A[i].y = p[i].y + f * (p[i + 1].y - p[i].y);
			}
			for (int i = 0; i < 2; ++i) {
				const double f = (tt - t[i]) / (t[i + 2] - t[i]);
				B[i].x = A[i].x + f * (A[i + 1].x - A[i].x); B[i].y = A[i].y + f * (A[i + 1].y - A[i].y);
			}
			const double f = (tt - t[1]) / (t[2] - t[1]);
			out->push_back(SplinePoint{B[0].x + f * (B[1].x - B[0].x), B[0].y + f * (B[1].y - B[0].y)});
		}
	}
	out->push_back(pts[pts.size() - 1]);
}

// the points at arc distance 1 and their multipliers; false: more than `max_points` of them (every one is a segment before the drops: the
// bound on the work a damaged stream can ask for)
inline bool spline_equal_spacing(const std::vector<SplinePoint> &poly, size_t max_points, std::vector<SplinePoint> *pts, std::vector<double> *mult) {
	pts->clear(); mult->clear();
	pts->push_back(poly[0]); mult->push_back(1.0);
	SplinePoint cur = poly[0];
	double acc = 0.0;
	for (size_t i = 1; i < poly.size(); ++i) {
		const SplinePoint q = poly[i];
		double dx = q.x - cur.x, dy = q.y - cur.y, len = sqrt(dx * dx + dy * dy);
		while (acc + len >= 1.0) {
			const double f = (1.0 - acc) / len;
			cur.x = cur.x + f * dx; cur.y = cur.y + f * dy;
			if (pts->size() >= max_points) return false;
			pts->push_back(cur); mult->push_back(1.0);
			acc = 0.0;
			dx = q.x - cur.x; dy = q.y - cur.y; len = sqrt(dx * dx + dy * dy);
		}
		acc += len; cur = q;
	}
	if (pts->size() >= max_points) return false;
	pts->push_back(poly[poly.size() - 1]); mult->push_back(acc);
	return true;
}

// one box edge pair, clipped to [0, n - 1]; false: empty
inline bool spline_box(double c, double d, int32_t n, int32_t *lo, int32_t *hi) {
	double a = floor((c - d) + 0.5), b = floor((c + d) + 0.5);
	if (!(a <= b)) return false;   // (a NaN among them)
	if (a < 0.0) a = 0.0;
	if (b > (double) (n - 1)) b = (double) (n - 1);
	if (!(a <= b)) return false;
	*lo = (int32_t) a; *hi = (int32_t) b;
	return true;
}

// The segments of the frame's splines, in drawing order, into plan->segs. false ("spln"): a control point out of bounds or repeated, more
// than SPLINE_MAX_SEGMENTS points along the splines. mults (optional, the CPU tests'): every kept segment's multiplier, which the record
// holds only inside s4.
inline bool spline_segments(const SplineData &sd, float base_corr_x, float base_corr_b, int32_t W, int32_t H, std::vector<SplineSeg> *segs, std::vector<double> *mults = nullptr) {
	static const double WEIGHT[4] = {0.0042, 0.075, 0.07, 0.3333};
	const double PI = 3.14159265358979323846, SQRT2 = sqrt(2.0), LN = 5.0 * log(10.0);
	const double qa = (double) sd.quant_adjust, inv_q = sd.quant_adjust >= 0 ? 1.0 / (1.0 + qa / 8.0) : 1.0 - qa / 8.0;
	segs->clear();
	if (mults) mults->clear();
	size_t points = 0;
	std::vector<SplinePoint> ctrl, poly, pts;
	std::vector<double> mult;
	for (const QuantSpline &q : sd.splines) {
		if (!spline_control_points(q, &ctrl)) return false;
		double coef[4][32];
		for (int c = 0; c < 4; ++c) for (int i = 0; i < 32; ++i) coef[c][i] = (((double) q.coef[c][i] * (i == 0 ? sqrt(0.5) : 1.0)) * WEIGHT[c]) * inv_q;
		for (int i = 0; i < 32; ++i) { coef[0][i] += (double) base_corr_x * coef[1][i]; coef[2][i] += (double) base_corr_b * coef[1][i]; }
		spline_catmull_rom(ctrl, &poly);
		if (!spline_equal_spacing(poly, (size_t) SPLINE_MAX_SEGMENTS - points, &pts, &mult)) return false;
		points += pts.size();
		const double arc = (double) ((int64_t) pts.size() - 2) + mult[mult.size() - 1];
		if (!(arc > 0.0)) continue;
		for (size_t k = 0; k < pts.size(); ++k) {
			double progress = (double) k / arc;
			if (progress > 1.0) progress = 1.0;
			const double t = 31.0 * progress;
			double val[4];
			for (int c = 0; c < 4; ++c) {
				double s = 0.0;
				for (int i = 0; i < 32; ++i) if (coef[c][i] != 0.0) s += (coef[c][i] * SQRT2) * cos(((PI / 32.0) * (double) i) * (t + 0.5));
				val[c] = s;
			}
			const double sigma = val[3], m1 = mult[k];
			if (sigma == 0.0 || !std::isfinite(sigma) || !std::isfinite(1.0 / sigma) || !std::isfinite(m1)) continue;
			double m = 0.01;
			for (int c = 0; c < 3; ++c) { const double a = fabs(val[c] * m1); if (a > m) m = a; }
			const double d = sqrt(((2.0 * sigma) * sigma) * (LN + log(m)));
			SplineSeg g;
			memset(&g, 0, sizeof g);
			if (!spline_box(pts[k].x, d, W, &g.x0, &g.x1) || !spline_box(pts[k].y, d, H, &g.y0, &g.y1)) continue;
			g.cx = (float) pts[k].x; g.cy = (float) pts[k].y; g.inv_sigma = (float) (1.0 / sigma); g.s4 = (float) ((0.25 * sigma) * m1);
			for (int c = 0; c < 3; ++c) g.col[c] = (float) val[c];
			segs->push_back(g);
			if (mults) mults->push_back(m1);
		}
	}
	return true;
}

// the tiles of the segments' boxes; false ("spln"): more than SPLINE_MAX_PAIRS (tile, segment) pairs. Nothing is made for no segments.
inline bool spline_bin(int32_t W, SplinePlan *plan) {
	const int32_t tiles_x = (W + SPLINE_TILE_W - 1) / SPLINE_TILE_W;
	plan->tiles_x = tiles_x;
	plan->tile_ids.clear(); plan->tile_start.clear(); plan->seg_idx.clear();
	if (plan->segs.empty()) return true;
	int64_t pairs = 0;
	int32_t max_tile = 0;
	for (const SplineSeg &g : plan->segs) {
		pairs += (int64_t) (g.x1 / SPLINE_TILE_W - g.x0 / SPLINE_TILE_W + 1) * (g.y1 / SPLINE_TILE_H - g.y0 / SPLINE_TILE_H + 1);
		if (pairs > SPLINE_MAX_PAIRS) return false;
		const int32_t last = (g.y1 / SPLINE_TILE_H) * tiles_x + g.x1 / SPLINE_TILE_W;
		if (last > max_tile) max_tile = last;
	}
	std::vector<int32_t> count((size_t) max_tile + 2, 0);   // (per tile of the frame up to the last touched one)
	auto each = [&](auto fn) {
		for (size_t i = 0; i < plan->segs.size(); ++i) {
			const SplineSeg &g = plan->segs[i];
			for (int32_t ty = g.y0 / SPLINE_TILE_H; ty <= g.y1 / SPLINE_TILE_H; ++ty) for (int32_t tx = g.x0 / SPLINE_TILE_W; tx <= g.x1 / SPLINE_TILE_W; ++tx) fn(ty * tiles_x + tx, (int32_t) i);
		}
	};
	each([&](int32_t tile, int32_t) { ++count[(size_t) tile + 1]; });
	std::vector<int32_t> slot((size_t) max_tile + 1, -1);
	plan->tile_start.push_back(0);
	for (int32_t t = 0; t <= max_tile; ++t) if (count[(size_t) t + 1]) {
		slot[(size_t) t] = (int32_t) plan->tile_ids.size();
		plan->tile_ids.push_back(t);
		plan->tile_start.push_back(plan->tile_start.back() + count[(size_t) t + 1]);
	}
	plan->seg_idx.assign((size_t) pairs, 0);
	std::vector<int32_t> fill(plan->tile_start.begin(), plan->tile_start.end() - 1);
	each([&](int32_t tile, int32_t i) { plan->seg_idx[(size_t) fill[(size_t) slot[(size_t) tile]]++] = i; });
	return true;
}

} // namespace j40hip
