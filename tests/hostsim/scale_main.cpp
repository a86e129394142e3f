// tests/hostsim/scale_main.cpp -- scale_sim.cpp's downscale as a program of its own (tests/test_scale.py runs it plain and built with
// -fsanitize=address,undefined): odd image sizes, both shifts, both formats, source and output in blocks of exactly their size from
// malloc with guard bytes round the output's rows, against a sample-by-sample restatement of the definition.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

extern "C" void scale_sim(uint8_t *out, size_t out_stride, const uint8_t *src, size_t src_stride, int32_t W, int32_t H, int32_t k, int32_t pixel_bytes, int32_t lanes);

static uint32_t rng_state = 12345;
static uint32_t rng() { rng_state = rng_state * 1664525u + 1013904223u; return rng_state >> 8; }

template <typename T> static int run_case(int W, int H, int k, int fill, long *guard_damage) {
	const int s = 1 << k, ow = (W + s - 1) >> k, oh = (H + s - 1) >> k, pb = 4 * (int) sizeof(T);
	const T top = (T) ~(T) 0;
	const size_t src_stride = (size_t) W * pb, guard = 32, out_stride = (size_t) ow * pb + guard;
	T *src = (T *) malloc(src_stride * (size_t) H);
	uint8_t *out = (uint8_t *) malloc(guard + out_stride * (size_t) oh);
	if (!src || !out) { fprintf(stderr, "out of memory\n"); exit(2); }
	for (int y = 0; y < H; ++y) for (int x = 0; x < W; ++x) for (int c = 0; c < 4; ++c)
		src[((size_t) y * W + x) * 4 + c] = fill == 0 ? 0 : fill == 1 ? top : fill == 2 ? (((x + y + c) & 1) ? top : 0) : (T) rng();
	memset(out, 0xA5, guard + out_stride * (size_t) oh);
	scale_sim(out + guard, out_stride, (const uint8_t *) src, src_stride, W, H, k, pb, 7);
	int bad = 0;
	for (int j = 0; j < oh; ++j) for (int i = 0; i < ow; ++i) for (int c = 0; c < 4; ++c) {
		uint32_t S = 0, n = 0;
		for (int y = j * s; y < (j + 1) * s && y < H; ++y) for (int x = i * s; x < (i + 1) * s && x < W; ++x) { S += src[((size_t) y * W + x) * 4 + c]; ++n; }
		T got;
		memcpy(&got, out + guard + (size_t) j * out_stride + ((size_t) i * 4 + c) * sizeof(T), sizeof(T));
		if (got != (T) ((S + n / 2) / n)) ++bad;
	}
	for (size_t b = 0; b < guard; ++b) if (out[b] != 0xA5) ++*guard_damage;
	for (int j = 0; j < oh; ++j) for (size_t b = (size_t) ow * pb; b < out_stride; ++b) if (out[guard + (size_t) j * out_stride + b] != 0xA5) ++*guard_damage;
	free(src); free(out);
	return bad;
}

int main() {
	long cases = 0, mismatches = 0, guard_damage = 0;
	std::vector<std::pair<int, int>> sizes;
	for (int w = 1; w <= 9; ++w) for (int h = 1; h <= 9; ++h) sizes.push_back({w, h});
	sizes.push_back({61, 43}); sizes.push_back({64, 64});
	for (auto wh : sizes) for (int k = 1; k <= 2; ++k) for (int fill = 0; fill < 4; ++fill) {
		mismatches += run_case<uint8_t>(wh.first, wh.second, k, fill, &guard_damage);
		mismatches += run_case<uint16_t>(wh.first, wh.second, k, fill, &guard_damage);
		cases += 2;
	}
	printf("scale_main: %ld cases, %ld mismatches, %ld guard bytes damaged\n", cases, mismatches, guard_damage);
	return mismatches || guard_damage ? 1 : 0;
}
