// tests/hostsim/ycbcr_main.cpp -- TEST INFRASTRUCTURE ONLY. The frame geometry of YCbCr VarDCT frames as a program of its own, so that it
// can run under the host sanitizers (an executable: never loaded into Python). Every argument is a stream: it is parsed with YCbCr
// frames asked for, its plan is built and it is decoded on the CPU (ycbcr_sim.cpp). Prints one line per stream; exit status 0 when
// every stream decoded.
#include <cstdint>
#include <cstdio>
#include <vector>

extern "C" void ycbcr_sim_info(const uint8_t *buf, size_t size, int32_t allow, int32_t *out);
extern "C" uint32_t ycbcr_sim_decode(const uint8_t *buf, size_t size, float *plane0, float *plane1, float *plane2, uint8_t *rgba, size_t stride, int32_t out16);

int main(int argc, char **argv) {
	int bad = 0;
	for (int a = 1; a < argc; ++a) {
		FILE *fp = fopen(argv[a], "rb");
		if (!fp) { fprintf(stderr, "cannot open %s\n", argv[a]); return 2; }
		std::vector<uint8_t> data;
		uint8_t chunk[4096];
		for (size_t n; (n = fread(chunk, 1, sizeof chunk, fp)) > 0; ) data.insert(data.end(), chunk, chunk + n);
		fclose(fp);
		int32_t info[24];
		ycbcr_sim_info(data.data(), data.size(), 1, info);
		if (info[0] || info[21]) { printf("%s: parse %08x plan %08x\n", argv[a], (unsigned) info[0], (unsigned) info[21]); ++bad; continue; }
		std::vector<float> planes[3];
		for (int c = 0; c < 3; ++c) planes[c].assign((size_t) info[8 + 2 * c] * (size_t) info[9 + 2 * c], 0.0f);
		for (int out16 = 0; out16 < 2; ++out16) {
			const size_t stride = (size_t) info[14] * (out16 ? 8 : 4);
			std::vector<uint8_t> rgba(stride * (size_t) info[15]);
			const uint32_t e = ycbcr_sim_decode(data.data(), data.size(), planes[0].data(), planes[1].data(), planes[2].data(), rgba.data(), stride, out16);
			unsigned long long sum = 0;
			for (uint8_t v : rgba) sum += v;
			printf("%s: %d x %d, planes %d x %d, %d x %d, %d x %d, %s: code %08x, sum %llu\n", argv[a], info[14], info[15], info[8], info[9], info[10], info[11], info[12], info[13], out16 ? "u16" : "u8", (unsigned) e, sum);
			if (e) ++bad;
		}
	}
	return bad ? 1 : 0;
}
