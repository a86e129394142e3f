// tests/hostsim/wide_main.cpp -- TEST INFRASTRUCTURE ONLY. The wide Modular path on the CPU (wide_sim.cpp) as a program of its own, so
// that it can run under the host sanitizers (an executable: never loaded into Python). Every argument is a stream: it is parsed with
// wide frames asked for and decoded to u8 and to u16. Prints one line per stream and output format -- the code, a sum over the output's
// bytes, the coded samples' extremes, the guard bytes damaged; exit status 0 when every stream decoded and no guard byte was damaged.
#include <cstdint>
#include <cstdio>
#include <vector>

extern "C" uint32_t widesim_decode(const uint8_t *buf, size_t size, uint8_t *out, int out_format, uint32_t flags);
extern "C" int64_t widesim_final_plane(int32_t c, int32_t *out, int32_t *w, int32_t *h);
extern "C" void widesim_coded_range(int64_t *out2);
extern "C" int64_t widesim_guard_damage(void);
extern "C" int32_t widesim_sample_bytes(void);

int main(int argc, char **argv) {
	int bad = 0;
	for (int a = 1; a < argc; ++a) {
		FILE *fp = fopen(argv[a], "rb");
		if (!fp) { fprintf(stderr, "cannot open %s\n", argv[a]); return 2; }
		std::vector<uint8_t> data;
		uint8_t chunk[4096];
		for (size_t n; (n = fread(chunk, 1, sizeof chunk, fp)) > 0; ) data.insert(data.end(), chunk, chunk + n);
		fclose(fp);
		// the size: a first decode into no pixels would be a decode of its own; the planes of a probe decode say it
		std::vector<uint8_t> probe((size_t) 1 << 26);   // (any picture of the tests fits: 2600 x 2100 x 8 bytes)
		for (int out16 = 0; out16 < 2; ++out16) {
			const uint32_t e = widesim_decode(data.data(), data.size(), probe.data(), out16, 8u /* J40HIP_PARSE_WIDE */);
			int32_t w = 0, h = 0;
			widesim_final_plane(0, nullptr, &w, &h);
			unsigned long long sum = 0;
			for (size_t i = 0; i < (size_t) w * (size_t) h * (out16 ? 8 : 4); ++i) sum += probe[i];
			int64_t range[2]; widesim_coded_range(range);
			printf("%s: %d x %d, %d bytes a sample, %s: code %08x, sum %llu, coded samples %lld .. %lld, %lld guard bytes damaged\n", argv[a], w, h, widesim_sample_bytes(), out16 ? "u16" : "u8",
				(unsigned) e, sum, (long long) range[0], (long long) range[1], (long long) widesim_guard_damage());
			if (e || widesim_guard_damage()) ++bad;
		}
	}
	return bad ? 1 : 0;
}
