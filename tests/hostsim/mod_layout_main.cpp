// tests/hostsim/mod_layout_main.cpp -- TEST INFRASTRUCTURE: the three CPU decodes that lay a Modular plan out with the product's
// ModPlanLayout (a Modular frame; a VarDCT frame's extra-channel sub-images in drop mode and in keep mode), as a stand-alone program
// over the codestream files named on the command line. Every plan lives in a block of exactly ModPlanLayout::total_bytes from malloc
// (mod_block.hpp), so the build with -fsanitize=address,undefined (build/mod_layout_main_san) sees a read or write one byte past the
// block, and the guard bytes behind every region show a write past a region inside it. Exit code 0: every decode returned 0 and
// left every guard as it was.
#include <cstdint>
#include <cstdio>
#include <vector>
#include "../../j40_amd/csrc/frame.hpp"

extern "C" uint32_t hostsim_decode(const uint8_t *buf, size_t size, uint8_t *rgba, float *coeffs_out, int only_entropy);
extern "C" int64_t hostsim_guard_damage(void);
extern "C" uint32_t alpha_sim_decode(const uint8_t *buf, size_t size, uint8_t *rgba, size_t stride, int32_t fmt);
extern "C" int64_t alpha_sim_guard_damage(void);

int main(int argc, char **argv) {
	int bad = 0;
	for (int a = 1; a < argc; ++a) {
		std::vector<uint8_t> data;
		if (FILE *fp = fopen(argv[a], "rb")) { for (int c; (c = fgetc(fp)) != EOF; ) data.push_back((uint8_t) c); fclose(fp); }
		j40hip::Frame fr;
		try {
			const uint8_t *cs; size_t cs_size; std::vector<uint8_t> storage;
			j40hip::extract_codestream(data.data(), data.size(), &cs, &cs_size, &storage);
			j40hip::parse_frame(cs, cs_size, &fr, 1);
		} catch (const j40hip::DecodeError &e) { printf("%s: does not parse (%08x)\n", argv[a], e.code); ++bad; continue; }
		const size_t w = (size_t) fr.fh.width, h = (size_t) fr.fh.height;
		std::vector<uint8_t> rgba(w * h * 4, 255);
		uint32_t e = hostsim_decode(data.data(), data.size(), rgba.data(), nullptr, 0);
		int64_t damage = hostsim_guard_damage();
		printf("%s: %s decode %08x, %lld guard bytes damaged\n", argv[a], fr.fh.is_modular ? "Modular" : "drop-mode", e, (long long) damage);
		bad += e != 0 || damage != 0;
		if (fr.fh.is_modular) continue;
		e = alpha_sim_decode(data.data(), data.size(), rgba.data(), w * 4, 0x0F33 /* J40HIP_U8X4 */);
		damage = alpha_sim_guard_damage();
		printf("%s: keep-mode decode %08x, %lld guard bytes damaged\n", argv[a], e, (long long) damage);
		bad += e != 0 || damage != 0;
	}
	return argc < 2 || bad ? 1 : 0;
}
