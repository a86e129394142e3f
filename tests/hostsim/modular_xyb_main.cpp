// tests/hostsim/modular_xyb_main.cpp -- modular_xyb_sim.cpp's lane walks as a program of its own (tests/test_modular_xyb.py runs it plain and
// built with -fsanitize=address,undefined): odd sizes and rectangles that touch every edge of planes wider than they are, int16 and int32
// samples, both formats, with and without alpha. Every plane is a block of exactly its size from malloc, so a lane that reads past a
// plane's end is the sanitizer's; the output's rows have guard bytes round them. Checked:
//   - nothing outside the rectangle is written: the guards and every pixel outside the rectangle keep their fill;
//   - nothing outside the rectangle is read: the samples outside it refilled with other values, the output stays byte for byte;
//   - the rectangle's pixels equal those of the same samples in a tight plane of their own decoded whole -- rows that start at other
//     alignments, so wide loads and stores against the sample-by-sample ones;
//   - k_modular_to_xyb's floats equal (float) c * m with the integer sum first, written out here.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

extern "C" int32_t modxyb_sim_planes(const void *const planes[3], int32_t sample_bytes, int32_t plane_width, int32_t x0, int32_t y0, int32_t rw, int32_t rh, const float *m, float *const out[3], size_t pitch);
extern "C" int32_t modxyb_sim_pack(int32_t on, const void *const planes[3], const void *alpha, int32_t sample_bytes, int32_t plane_width, int32_t x0, int32_t y0, int32_t rw, int32_t rh,
		const float *m, const float *cc15, int32_t bpp, int32_t rgba16, uint8_t *rgba, size_t stride);

static uint32_t rng_state = 2463534242u;
static uint32_t rng() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 17; rng_state ^= rng_state << 5; return rng_state; }

static const float M[3] = {1.0f / 4096.0f, 1.0f / 512.0f, 1.0f / 256.0f};
static const float CC[15] = {11.031566901960783f, -9.866943921568629f, -0.16462299647058826f, -3.254147380392157f, 4.418770392156863f, -0.16462299647058826f,
	-3.6588512862745097f, 2.7129230470588235f, 1.9459282392156863f, -0.0037930732552754493f, -0.0037930732552754493f, -0.0037930732552754493f, 255.0f, 0.0f, 0.0f};

struct Tally { long cases = 0, mismatches = 0, outside_written = 0, outside_read = 0, plane_mismatches = 0; };

// a sample of the kind the planes hold: mostly what a picture has, now and then an extreme of the type
template <typename S> static S sample(int c) {
	const uint32_t r = rng();
	if ((r & 63) == 0) return (r & 64) ? std::numeric_limits<S>::min() : std::numeric_limits<S>::max();
	return c == 0 ? (S) (r >> 8 & 511) : c == 1 ? (S) ((int32_t) (r >> 8 & 255) - 128) : c == 2 ? (S) ((int32_t) (r >> 8 & 511) - 300) : (S) (r >> 8 & 255);
}

template <typename S> static void run_case(int PW, int PH, int x0, int y0, int rw, int rh, bool alpha, bool rgba16, Tally *t) {
	const size_t n = (size_t) PW * (size_t) PH, pb = rgba16 ? 8 : 4, guard = 32, stride = (size_t) PW * pb + guard;
	S *pl[4];
	for (int c = 0; c < 4; ++c) { pl[c] = (S *) malloc(n * sizeof(S)); if (!pl[c]) { fprintf(stderr, "out of memory\n"); exit(2); } for (size_t i = 0; i < n; ++i) pl[c][i] = sample<S>(c); }
	const void *planes[3] = {pl[0], pl[1], pl[2]};
	const size_t out_bytes = guard + stride * (size_t) PH;
	std::vector<uint8_t> out(out_bytes, 0xA5), again(out_bytes, 0xA5);
	modxyb_sim_pack(1, planes, alpha ? pl[3] : nullptr, (int32_t) sizeof(S), PW, x0, y0, rw, rh, M, CC, 8, rgba16, out.data() + guard, stride);
	// nothing outside the rectangle is written
	for (size_t b = 0; b < out_bytes; ++b) {
		bool inside = false;
		if (b >= guard) { const size_t y = (b - guard) / stride, xb = (b - guard) % stride; inside = (int) y >= y0 && (int) y < y0 + rh && xb >= (size_t) x0 * pb && xb < (size_t) (x0 + rw) * pb; }
		if (!inside && out[b] != 0xA5) ++t->outside_written;
	}
	// the planes' floats against the statement, and the same samples in tight planes of their own
	std::vector<float> f[3];
	for (auto &v : f) v.assign((size_t) rw * (size_t) rh, -1.0f);
	float *fo[3] = {f[0].data(), f[1].data(), f[2].data()};
	modxyb_sim_planes(planes, (int32_t) sizeof(S), PW, x0, y0, rw, rh, M, fo, (size_t) rw);
	S *tight[4];
	for (int c = 0; c < 4; ++c) { tight[c] = (S *) malloc((size_t) rw * (size_t) rh * sizeof(S)); for (int y = 0; y < rh; ++y) memcpy(tight[c] + (size_t) y * rw, pl[c] + (size_t) (y0 + y) * PW + x0, (size_t) rw * sizeof(S)); }
	for (int y = 0; y < rh; ++y) for (int x = 0; x < rw; ++x) {
		const size_t i = (size_t) y * rw + x;
		const float X = (float) tight[1][i] * M[0], Y = (float) tight[0][i] * M[1];
		const float B = (sizeof(S) == 4 ? (float) ((int64_t) tight[2][i] + (int64_t) tight[0][i]) : (float) ((int32_t) tight[2][i] + (int32_t) tight[0][i])) * M[2];
		if (memcmp(&f[0][i], &X, 4) || memcmp(&f[1][i], &Y, 4) || memcmp(&f[2][i], &B, 4)) ++t->plane_mismatches;
	}
	const void *tp[3] = {tight[0], tight[1], tight[2]};
	std::vector<uint8_t> whole((size_t) rw * pb * (size_t) rh + 1, 0);
	modxyb_sim_pack(1, tp, alpha ? tight[3] : nullptr, (int32_t) sizeof(S), rw, 0, 0, rw, rh, M, CC, 8, rgba16, whole.data() + 1, (size_t) rw * pb);   // (the rows start at odd addresses)
	for (int y = 0; y < rh; ++y) if (memcmp(whole.data() + 1 + (size_t) y * rw * pb, out.data() + guard + (size_t) (y0 + y) * stride + (size_t) x0 * pb, (size_t) rw * pb)) ++t->mismatches;
	// nothing outside the rectangle is read
	for (int c = 0; c < 4; ++c) for (int y = 0; y < PH; ++y) for (int x = 0; x < PW; ++x) if (y < y0 || y >= y0 + rh || x < x0 || x >= x0 + rw) pl[c][(size_t) y * PW + x] = (S) ~pl[c][(size_t) y * PW + x];
	modxyb_sim_pack(1, planes, alpha ? pl[3] : nullptr, (int32_t) sizeof(S), PW, x0, y0, rw, rh, M, CC, 8, rgba16, again.data() + guard, stride);
	if (out != again) ++t->outside_read;
	for (int c = 0; c < 4; ++c) { free(pl[c]); free(tight[c]); }
	++t->cases;
}

int main() {
	Tally t;
	std::vector<std::pair<int, int>> sizes;
	for (int w = 1; w <= 9; ++w) for (int h = 1; h <= 5; ++h) sizes.push_back({w, h});
	for (auto wh : {std::pair<int, int>{61, 7}, {64, 4}, {255, 3}, {257, 5}, {259, 2}, {515, 3}}) sizes.push_back(wh);
	for (auto wh : sizes) {
		const int W = wh.first, H = wh.second;
		// the whole plane, and rectangles that touch the left / top, the right / bottom, neither, one full row, one full column
		const int rects[6][4] = {{0, 0, W, H}, {0, 0, (W + 1) / 2, (H + 1) / 2}, {W / 2, H / 2, W - W / 2, H - H / 2}, {W > 2 ? 1 : 0, H > 2 ? 1 : 0, W > 2 ? W - 2 : W, H > 2 ? H - 2 : H},
			{0, H - 1, W, 1}, {W - 1, 0, 1, H}};
		for (const auto &r : rects) for (int alpha = 0; alpha < 2; ++alpha) for (int fmt = 0; fmt < 2; ++fmt) {
			run_case<int16_t>(W, H, r[0], r[1], r[2], r[3], alpha != 0, fmt != 0, &t);
			run_case<int32_t>(W, H, r[0], r[1], r[2], r[3], alpha != 0, fmt != 0, &t);
		}
	}
	printf("modular_xyb_main: %ld cases, %ld rows differing from the tight planes' decode, %ld plane floats off the statement, %ld bytes written outside the rectangle, %ld cases that read outside it\n",
		t.cases, t.mismatches, t.plane_mismatches, t.outside_written, t.outside_read);
	return t.mismatches || t.plane_mismatches || t.outside_written || t.outside_read ? 1 : 0;
}
