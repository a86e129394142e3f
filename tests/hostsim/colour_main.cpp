// tests/hostsim/colour_main.cpp -- colour_sim.cpp's tail as a program of its own (tests/test_colour.py runs it plain and built with
// -fsanitize=address,undefined): every curve, both formats, bit depths 8, 10 and 16, with and without the table, over planes that are blocks of
// exactly their size from malloc and an output with guard bytes round its rows -- a lane that reads past a plane or writes past a row
// is the sanitizer's, a float -> integer conversion out of range (NaN, infinities, 1e38 among the samples) UBSan's. Checked:
//   - nothing outside the rows' pixels is written;
//   - an 8-bit frame's pixels by table equal those by the curve;
//   - alpha is opaque; u16 of an 8-bit frame is u8 * 257;
//   - the table of every curve agrees with the long way on every 257th float of its range and on the samples outside it.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

extern "C" int32_t colour_sim_tail(const float *xyb, int32_t w, int32_t h, const float *cc15, const int32_t *enc, const float *lum, int32_t bpp, int32_t use_table, int32_t rgba16, uint8_t *out, size_t stride);
extern "C" void colour_sim_table_check(const int32_t *enc, float it, int32_t step, int32_t threads, int64_t *out, float *thr);

static uint32_t rng_state = 2463534242u;
static uint32_t rng() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 17; rng_state ^= rng_state << 5; return rng_state; }

static const float CC[15] = {11.031566901960783f, -9.866943921568629f, -0.16462299647058826f, -3.254147380392157f, 4.418770392156863f, -0.16462299647058826f,
	-3.6588512862745097f, 2.7129230470588235f, 1.9459282392156863f, -0.0037930732552754493f, -0.0037930732552754493f, -0.0037930732552754493f, 255.0f, 0.0f, 0.0f};
static const float LUM[3] = {0.2627f, 0.6780f, 0.0593f};

// the 16 words of an encoding: RGB, D65, sRGB primaries, the given transfer function or gamma
static void encoding(int32_t tf, int32_t gamma, int32_t enc[16]) {
	const int32_t base[16] = {0, 1, 312700, 329000, 1, 640000, 330000, 300000, 600000, 150000, 60000, gamma ? 1 : 0, gamma, tf, 1, 0};
	memcpy(enc, base, sizeof base);
}

int main() {
	const struct { const char *name; int32_t tf, gamma; float it; } CURVES[] = {{"linear", 8, 0, 255.0f}, {"srgb", 13, 0, 255.0f}, {"bt709", 1, 0, 255.0f}, {"dci", 17, 0, 255.0f},
		{"gamma_0.45", 0, 4500000, 255.0f}, {"gamma_1", 0, 10000000, 255.0f}, {"pq_255", 16, 0, 255.0f}, {"pq_4000", 16, 0, 4000.0f}, {"hlg_1000", 18, 0, 1000.0f}, {"hlg_255", 18, 0, 255.0f}};
	long cases = 0, outside = 0, table_vs_curve = 0, alpha_bad = 0, u16_bad = 0, table_bad = 0, no_table = 0;
	for (const auto &cv : CURVES) {
		int32_t enc[16];
		encoding(cv.tf, cv.gamma, enc);
		float cc[15];
		memcpy(cc, CC, sizeof cc); cc[12] = cv.it;
		for (auto wh : {std::pair<int, int>{1, 1}, {7, 3}, {37, 21}, {65, 5}}) {
			const int W = wh.first, H = wh.second;
			const size_t n = (size_t) W * (size_t) H;
			float *xyb = (float *) malloc(3 * n * sizeof(float));
			if (!xyb) return 2;
			for (size_t i = 0; i < 3 * n; ++i) {
				const uint32_t r = rng();
				float v = (float) ((int32_t) (r >> 8 & 0xffff) - 20000) / 60000.0f;   // what a picture holds, and beyond
				if ((r & 31) == 0) { const float odd[8] = {NAN, INFINITY, -INFINITY, 1e38f, -1e38f, 0.0f, -0.0f, 1e-30f}; v = odd[r >> 5 & 7]; }
				xyb[i] = v;
			}
			for (int bpp : {8, 10, 16}) for (int fmt = 0; fmt < 2; ++fmt) {
				const size_t pb = fmt ? 8 : 4, guard = 24, stride = (size_t) W * pb + guard, bytes = guard + stride * (size_t) H;
				std::vector<uint8_t> a(bytes, 0xA5), b(bytes, 0xA5);
				const int32_t ta = colour_sim_tail(xyb, W, H, cc, enc, LUM, bpp, 1, fmt, a.data() + guard, stride);
				const int32_t tb = colour_sim_tail(xyb, W, H, cc, enc, LUM, bpp, 0, fmt, b.data() + guard, stride);
				if (ta < 0 || tb != 0) return 3;
				if (bpp == 8 && ta != 1) ++no_table;
				for (size_t o = 0; o < bytes; ++o) {
					const bool inside = o >= guard && (o - guard) % stride < (size_t) W * pb;
					if (!inside && (a[o] != 0xA5 || b[o] != 0xA5)) ++outside;
				}
				if (a != b) ++table_vs_curve;
				for (int y = 0; y < H; ++y) for (int x = 0; x < W; ++x) {
					const uint8_t *px = a.data() + guard + (size_t) y * stride + (size_t) x * pb;
					if (fmt ? px[6] != 0xff || px[7] != 0xff : px[3] != 0xff) ++alpha_bad;
				}
				if (bpp == 8 && fmt) {   // u16 of an 8-bit frame: u8 * 257
					std::vector<uint8_t> c(guard + ((size_t) W * 4 + guard) * (size_t) H, 0);
					colour_sim_tail(xyb, W, H, cc, enc, LUM, 8, 1, 0, c.data() + guard, (size_t) W * 4 + guard);
					for (int y = 0; y < H; ++y) for (int x = 0; x < W; ++x) for (int ch = 0; ch < 3; ++ch) {
						uint16_t v16; memcpy(&v16, a.data() + guard + (size_t) y * stride + (size_t) x * 8 + 2 * ch, 2);
						if (v16 != 257u * c[guard + (size_t) y * ((size_t) W * 4 + guard) + (size_t) x * 4 + ch]) ++u16_bad;
					}
				}
				++cases;
			}
			free(xyb);
		}
		int64_t out[6];
		colour_sim_table_check(enc, cv.it, 257, 2, out, nullptr);
		if (!out[0]) ++no_table;
		table_bad += (long) out[4];
		printf("  %-10s table: buckets %lld..%lld, %lld floats compared, %lld differ\n", cv.name, (long long) out[1], (long long) out[2], (long long) out[3], (long long) out[4]);
	}
	printf("colour_main: %ld cases, %ld bytes written outside the rows, %ld cases where table and curve differ, %ld pixels not opaque, %ld u16 samples off u8 * 257, %ld table lookups off the long way, %ld curves without a table\n",
		cases, outside, table_vs_curve, alpha_bad, u16_bad, table_bad, no_table);
	return outside || table_vs_curve || alpha_bad || u16_bad || table_bad || no_table ? 1 : 0;
}
