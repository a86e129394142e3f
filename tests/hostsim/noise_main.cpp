// tests/hostsim/noise_main.cpp -- noise_sim.cpp as a program of its own (tests/test_noise.py runs it plain and built with the host
// sanitizers; an executable, never loaded into Python): frames whose sizes are no multiples of the group, the tile or the 16-float run,
// the raw planes and the frame's planes each in an allocation of exactly its size, so that a thread that steps outside a plane or the
// jump sets is caught. The jumped fill is compared with the sequential one bit for bit, the tiled addition with the rule written out
// pixel by pixel.
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <vector>
#include "../../j40_amd/csrc/device/noise_dev.h"

extern "C" int64_t noise_sim_pitch(int32_t W);
extern "C" int32_t noise_sim_fill(float *raw, int32_t W, int32_t H, int32_t gdim, uint32_t visible, uint32_t nonvisible, int32_t jumped);
extern "C" void noise_sim_add(float *planes, const float *raw, int32_t W, int32_t H, const float *lut8, float ytox, float ytob);

static uint64_t g_state = 0x9e3779b97f4a7c15ull;
static uint32_t rnd(uint32_t n) { g_state = g_state * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t) (g_state >> 33) % n; }
static float rndf() { return (float) ((int32_t) rnd(4001) - 2000) / 1000.0f; }

int main() {
	using namespace j40hip;
	static const int32_t SIZES[][3] = {{300, 270, 128}, {128, 128, 128}, {44, 14, 128}, {16, 1, 128}, {17, 3, 128}, {1, 1, 128}, {128, 64, 128}, {70, 40, 16}, {260, 5, 256}, {3, 200, 64}};
	int failures = 0;
	for (const auto &size : SIZES) {
		const int32_t W = size[0], H = size[1], gdim = size[2];
		const size_t pitch = (size_t) noise_sim_pitch(W), plane = pitch * (size_t) H;
		const uint32_t visible = rnd(5), nonvisible = rnd(3);
		std::vector<float> seq(3 * plane, -1.0f), jumped(3 * plane, -1.0f);
		if (noise_sim_fill(seq.data(), W, H, gdim, visible, nonvisible, 0) || noise_sim_fill(jumped.data(), W, H, gdim, visible, nonvisible, 1)) { fprintf(stderr, "noise_main: %dx%d: the fill refused the size\n", W, H); ++failures; continue; }
		bool same = true, ranged = true;
		for (int c = 0; c < 3; ++c) for (int32_t y = 0; y < H; ++y) for (int32_t x = 0; x < W; ++x) {
			const size_t at = (size_t) c * plane + (size_t) y * pitch + (size_t) x;
			same = same && memcmp(&seq[at], &jumped[at], 4) == 0;
			ranged = ranged && seq[at] >= 1.0f && seq[at] < 2.0f;
		}
		if (!same || !ranged) { fprintf(stderr, "noise_main: %dx%d groups of %d: the jumped fill %s, the values %s\n", W, H, gdim, same ? "agrees" : "differs", ranged ? "in [1, 2)" : "out of range"); ++failures; }
		// the addition, against the rule pixel by pixel
		NoiseParams p;
		for (int i = 0; i < 8; ++i) p.lut[i] = (float) rnd(1400) / 1024.0f;   // (values past 1: the clamp)
		p.ytox = rndf(); p.ytob = rndf();
		std::vector<float> planes((size_t) 3 * W * H), want;
		for (float &v : planes) v = rndf() * 0.7f;
		want = planes;
		for (int32_t y = 0; y < H; ++y) for (int32_t x = 0; x < W; ++x) {
			float conv[3];
			for (int c = 0; c < 3; ++c) {
				float sum = 0.0f; bool first = true;
				for (int dy = -2; dy <= 2; ++dy) for (int dx = -2; dx <= 2; ++dx) {
					if (!dy && !dx) continue;
					const float v = jumped[(size_t) c * plane + (size_t) noise_mirror(y + dy, H) * pitch + (size_t) noise_mirror(x + dx, W)];
					sum = first ? v : sum + v; first = false;
				}
				conv[c] = jumped[(size_t) c * plane + (size_t) y * pitch + (size_t) x] * -3.84f + 0.16f * sum;
			}
			float d[3];
			for (int c = 0; c < 3; ++c) d[c] = want[((size_t) c * H + (size_t) y) * W + (size_t) x];
			noise_add_pixel(p, d, conv);
			for (int c = 0; c < 3; ++c) want[((size_t) c * H + (size_t) y) * W + (size_t) x] = d[c];
		}
		noise_sim_add(planes.data(), jumped.data(), W, H, p.lut, p.ytox, p.ytob);
		if (memcmp(planes.data(), want.data(), planes.size() * 4) != 0) { fprintf(stderr, "noise_main: %dx%d: the tiled addition differs from the rule\n", W, H); ++failures; }
	}
	if (noise_sim_fill(nullptr, 10, 10, 24, 0, 0, 0) != -1 || noise_sim_fill(nullptr, 0, 10, 128, 0, 0, 1) != -1) { fprintf(stderr, "noise_main: a bad size was taken\n"); ++failures; }
	printf("noise_main: %d failure(s)\n", failures);
	return failures ? 1 : 0;
}
