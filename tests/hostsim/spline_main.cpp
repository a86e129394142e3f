// tests/hostsim/spline_main.cpp -- spline_sim.cpp as a program of its own (tests/test_splines.py runs it plain and built with the host
// sanitizers; an executable, never loaded into Python): frames whose sizes are no multiples of the tile, the planes in an allocation of
// exactly their size, so that a lane that steps outside them or a list that runs past its tile is caught. The tiled, chunked draw is
// compared with the rule written out sample by sample, segment by segment; the dequantisation runs over splines that leave the frame,
// that are refused, and that draw nothing.
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <vector>
#include "../../j40_amd/csrc/device/spline_dev.h"

extern "C" int64_t spline_sim_draw(float *planes, int32_t W, int32_t H, const void *segments, int64_t n, int64_t *most_out);
extern "C" int64_t spline_sim_segments(int64_t x, int64_t y, const int64_t *dd, int32_t npts, const int32_t *coef128, int32_t quant_adjust, float ytox, float ytob, int32_t W, int32_t H, void *out, int64_t cap, double *mult_out);

static uint64_t g_state = 0x9e3779b97f4a7c15ull;
static uint32_t rnd(uint32_t n) { g_state = g_state * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t) (g_state >> 33) % n; }
static float rndf() { return (float) ((int32_t) rnd(4001) - 2000) / 1000.0f; }

int main() {
	using namespace j40hip;
	static const int32_t SIZES[][3] = {{96, 80, 40}, {65, 33, 300}, {64, 32, 10}, {1, 1, 3}, {200, 7, 500}, {3, 150, 60}};
	int failures = 0;
	for (const auto &size : SIZES) {
		const int32_t W = size[0], H = size[1], n = size[2];
		std::vector<SplineSeg> segs((size_t) n);
		for (SplineSeg &g : segs) {
			memset(&g, 0, sizeof g);
			const int32_t xa = (int32_t) rnd((uint32_t) W), xb = (int32_t) rnd((uint32_t) W), ya = (int32_t) rnd((uint32_t) H), yb = (int32_t) rnd((uint32_t) H);
			g.x0 = xa < xb ? xa : xb; g.x1 = xa < xb ? xb : xa; g.y0 = ya < yb ? ya : yb; g.y1 = ya < yb ? yb : ya;
			g.cx = 0.5f * (float) (g.x0 + g.x1) + rndf(); g.cy = 0.5f * (float) (g.y0 + g.y1) + rndf();
			g.inv_sigma = 1.0f / (0.3f + (float) rnd(300) / 100.0f); g.s4 = 0.25f * (1.0f + rndf() * 0.4f);
			for (float &c : g.col) c = rndf() * 0.1f;
		}
		std::vector<float> planes((size_t) 3 * W * H), want;
		for (float &v : planes) v = rndf() * 0.7f;
		want = planes;
		for (const SplineSeg &g : segs) for (int32_t y = g.y0; y <= g.y1; ++y) for (int32_t x = g.x0; x <= g.x1; ++x) {
			const size_t at = (size_t) y * W + (size_t) x, plane = (size_t) W * H;
			spline_splat(g, x, y, want[at], want[plane + at], want[2 * plane + at]);
		}
		int64_t most = 0;
		const int64_t tiles = spline_sim_draw(planes.data(), W, H, segs.data(), n, &most);
		if (tiles <= 0 || memcmp(planes.data(), want.data(), planes.size() * 4) != 0) { fprintf(stderr, "spline_main: %dx%d, %d segments: the tiled draw %s\n", W, H, n, tiles <= 0 ? "refused" : "differs from the rule"); ++failures; }
	}
	{   // a box outside the frame is refused, no segments draw nothing
		SplineSeg g;
		memset(&g, 0, sizeof g);
		g.x1 = 10; g.y1 = 10;
		std::vector<float> planes(3 * 10 * 10, 1.0f);
		if (spline_sim_draw(planes.data(), 10, 10, &g, 1, nullptr) != -1 || spline_sim_draw(planes.data(), 10, 10, nullptr, 0, nullptr) != 0) { fprintf(stderr, "spline_main: a bad box was taken\n"); ++failures; }
	}
	{   // the dequantisation: a curve through and beyond a 96 x 80 frame, a one-point spline, repeated points, a coordinate out of bounds
		int32_t coef[4][32];
		memset(coef, 0, sizeof coef);
		coef[1][0] = 40; coef[0][1] = -7; coef[3][0] = 12; coef[3][2] = 3;
		const int64_t far[] = {150, 60, -260, -20, 150, -90}, same[] = {5, 5, -5, -5}, big[] = {(int64_t) 1 << 24, 0};
		std::vector<SplineSeg> out(4096);
		const int64_t a = spline_sim_segments(-40, 20, far, 3, &coef[0][0], -3, 0.25f, 0.9f, 96, 80, out.data(), (int64_t) out.size(), nullptr);
		const int64_t b = spline_sim_segments(10, 10, nullptr, 0, &coef[0][0], 0, 0.0f, 1.0f, 96, 80, out.data(), (int64_t) out.size(), nullptr);
		const int64_t c = spline_sim_segments(10, 10, same, 2, &coef[0][0], 0, 0.0f, 1.0f, 96, 80, nullptr, 0, nullptr);
		const int64_t d = spline_sim_segments(10, 10, big, 1, &coef[0][0], 0, 0.0f, 1.0f, 96, 80, nullptr, 0, nullptr);
		if (a <= 0 || a > (int64_t) out.size() || b != 0 || c != -1 || d != -1) { fprintf(stderr, "spline_main: segments %lld %lld %lld %lld\n", (long long) a, (long long) b, (long long) c, (long long) d); ++failures; }
		for (int64_t i = 0; i < a && i < (int64_t) out.size(); ++i) if (out[(size_t) i].x0 < 0 || out[(size_t) i].x1 >= 96 || out[(size_t) i].y0 < 0 || out[(size_t) i].y1 >= 80) { fprintf(stderr, "spline_main: a box leaves the frame\n"); ++failures; break; }
	}
	printf("spline_main: %d failure(s)\n", failures);
	return failures ? 1 : 0;
}
