// tests/hostsim/orient_main.cpp -- orient_sim.cpp's oriented output as a program of its own (tests/test_orient.py runs it plain and built
// with -fsanitize=address,undefined): every size 1..9 x 1..9 and every pair of sizes round the tile, all eight orientations, both
// formats, source and output in blocks of exactly their size from malloc with guard bytes round the output's rows, against a
// pixel-by-pixel restatement of the definition (the table of include/j40hip.h, not orient_dev.h's functions).
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <utility>
#include <vector>

extern "C" void orient_sim(uint8_t *out, size_t out_stride, const uint8_t *src, size_t src_stride, int32_t W, int32_t H, int32_t o, int32_t pixel_bytes, int32_t lanes);
extern "C" int32_t orient_sim_tile();

static uint32_t rng_state = 12345;
static uint32_t rng() { rng_state = rng_state * 1664525u + 1013904223u; return rng_state >> 8; }

static int run_case(int W, int H, int o, int pb, long *guard_damage) {
	const int ow = o >= 5 ? H : W, oh = o >= 5 ? W : H;
	const size_t src_stride = (size_t) W * pb, guard = 24, out_stride = (size_t) ow * pb + guard;
	uint8_t *src = (uint8_t *) malloc(src_stride * (size_t) H);
	uint8_t *out = (uint8_t *) malloc(guard + out_stride * (size_t) oh);
	if (!src || !out) { fprintf(stderr, "out of memory\n"); exit(2); }
	for (size_t b = 0; b < src_stride * (size_t) H; ++b) src[b] = (uint8_t) rng();
	memset(out, 0xA5, guard + out_stride * (size_t) oh);
	orient_sim(out + guard, out_stride, src, src_stride, W, H, o, pb, 7);
	int bad = 0;
	for (int j = 0; j < oh; ++j) for (int i = 0; i < ow; ++i) {
		int x = 0, y = 0;
		switch (o) {
		case 1: x = i; y = j; break;
		case 2: x = W - 1 - i; y = j; break;
		case 3: x = W - 1 - i; y = H - 1 - j; break;
		case 4: x = i; y = H - 1 - j; break;
		case 5: x = j; y = i; break;
		case 6: x = j; y = H - 1 - i; break;
		case 7: x = W - 1 - j; y = H - 1 - i; break;
		default: x = W - 1 - j; y = i; break;
		}
		if (memcmp(out + guard + (size_t) j * out_stride + (size_t) i * pb, src + (size_t) y * src_stride + (size_t) x * pb, (size_t) pb)) ++bad;
	}
	for (size_t b = 0; b < guard; ++b) if (out[b] != 0xA5) ++*guard_damage;
	for (int j = 0; j < oh; ++j) for (size_t b = (size_t) ow * pb; b < out_stride; ++b) if (out[guard + (size_t) j * out_stride + b] != 0xA5) ++*guard_damage;
	free(src); free(out);
	return bad;
}

int main() {
	long cases = 0, mismatches = 0, guard_damage = 0;
	const int T = orient_sim_tile();
	std::vector<std::pair<int, int>> sizes;
	for (int w = 1; w <= 9; ++w) for (int h = 1; h <= 9; ++h) sizes.push_back({w, h});
	const int edge[4] = {T - 1, T, T + 1, 2 * T + 3};
	for (int w : edge) for (int h : edge) sizes.push_back({w, h});
	for (auto wh : sizes) for (int o = 1; o <= 8; ++o) for (int pb = 4; pb <= 8; pb += 4) {
		mismatches += run_case(wh.first, wh.second, o, pb, &guard_damage);
		++cases;
	}
	printf("orient_main: %ld cases, %ld mismatches, %ld guard bytes damaged\n", cases, mismatches, guard_damage);
	return mismatches || guard_damage ? 1 : 0;
}
