// tools/jxlsynth.cpp -- synthetic JPEG XL stream generator (test/bench infrastructure).
//
// No encoder or sample file exists offline, so this tool writes the streams
// the tests and bench.py decode: VarDCT frames (all 27 transform types, rANS with clustered
// contexts, optional custom block-context map / coefficient orders / HF presets / multiple passes)
// and Modular frames (single- and multi-group, RCT / Palette, prefix codes with LZ77, weighted
// predictor). Two ways to make a VarDCT frame:
//   forward=1  an ENCODE of a procedural picture: XYB forward, LF = 8x8 means, forward transform per varblock
//              (jxlsynth_forward.hpp), quantisation at about distance 1 with the library matrices, transform sizes and
//              HfMul chosen from local activity. Size, symbols per pixel and the spread of the sections' lengths follow
//              from the picture (1/f detail whose strength varies over the frame: `detail=`). What bench.py decodes.
//   forward=0  synthesis in the *coefficient domain* (the feature-matrix streams of the tests and the golden fixtures): the
//              LF image comes from a smooth procedural picture, HF coefficients are sparse with frequency-decaying
//              magnitudes; every transform type and bitstream feature can be forced into a small frame.
// lflevels=1|2 writes the LF image as LF frame(s) of its own in front of a main frame with use_lf_frame (run_lf_sequence, below).
// The reference decoder (oracle/_ref) is the judge of validity; what a stream decodes to is defined by it.
//
// usage: jxlsynth vardct  W H SEED OUT [key=value ...]
//        jxlsynth modular W H SEED OUT [key=value ...]
#include "jxlsynth_common.hpp"
#include "jxlsynth_modular.hpp"
#include "jxlsynth_forward.hpp"
#include "jxlsynth_lz77.hpp"
#include <cmath>
#include <map>
#include <functional>

using namespace synth;

// ------------------------------------------------------------------------------------------------
// options

struct Options {
	std::map<std::string, std::string> kv;
	int geti(const char *k, int def) const { auto it = kv.find(k); return it == kv.end() ? def : atoi(it->second.c_str()); }
	double getd(const char *k, double def) const { auto it = kv.find(k); return it == kv.end() ? def : atof(it->second.c_str()); }
	std::string gets(const char *k, const char *def) const { auto it = kv.find(k); return it == kv.end() ? def : it->second; }
};

// ------------------------------------------------------------------------------------------------
// several frames in one codestream (frames=N; main() runs the mode's writer once per coded frame). While `g_seq` is set a writer
// produces one coded frame of the sequence instead of a file: the image header carries the canvas' size (and the animation header),
// the frame header the frame's crop, source slot, duration, is_last and save_as_reference, and the bytes are appended to `cs`
// (signature and image header with the first frame only). With none of the sequence options the writers never see it.
struct SeqFrame {
	int canvas_w = 0, canvas_h = 0;
	bool anim = false;                // ImageMetadata with the animation header: 10/1 ticks per second, 0 loops
	bool first = true;                // this frame opens the codestream: signature and image header are written
	bool have_crop = false; int x0 = 0, y0 = 0;   // (its width and height are the writer's W and H)
	int blend = 0, src = 0, save = 0;
	int ec_blend = 0, ec_src = 0;     // the extra channels' blend mode and source slot (the colour channels' unless ecblends= / ecsrcs= say otherwise)
	long long duration = 0;
	bool is_last = true;
	int type = 0;                     // types=: 0 a regular frame, 2 a reference-only frame (its own size, no origin, no blend info, never last)
	int save_before_ct = 1;           // ... whose save_before_color_transform bit is this (sbct=0: a stream a decoder has to refuse)
	std::vector<uint8_t> *cs = nullptr;   // the codestream so far
	size_t first_section = 0;         // out: where this frame's first section starts in `cs`
};
static SeqFrame *g_seq = nullptr;

// patches=: the patch dictionary of the frame being written. A reference patch is the w x h rectangle at (x0, y0) of the reference-only
// frame in slot `ref`; every placement puts it at (x, y) of the frame in blend mode `mode` (0 None, 1 Replace, 2 Add, 3 Mul, 4..7 the
// alpha-using ones) with `clamp`. Nothing is checked: a dictionary a decoder has to refuse -- a mode above 7, a slot above 3, a rectangle
// or a placement outside its frame, a later placement left of or above the frame -- is written as it stands.
//   twin (patchtwin=1): the frame without the flag and without the dictionary, every other byte alike
//   ec_mode (patchec=M): the mode of every extra channel's blend entry (default 0, None)
//   cut (patchcut=1): LfGlobal ends in the middle of the dictionary (frames with several sections)
struct PatchPlace { long long x, y; int mode, clamp; };
struct PatchRef { int ref, x0, y0, w, h; std::vector<PatchPlace> at; };
struct PatchRole { std::vector<PatchRef> refs; bool twin = false; int ec_mode = 0; bool cut = false; };
static PatchRole *g_patch = nullptr;
static bool patch_flag() { return g_patch && !g_patch->twin; }
// One entropy-coded stream over 10 contexts (three clusters, ANS): num_ref (context 0); per reference patch ref (1), x0, y0 (3), w - 1,
// h - 1 (2), count - 1 (7); per placement x, y (4; from the second on the sign-folded differences to the one before, 6) and for each of
// num_ec + 1 blend entries the mode (5), the alpha channel (8; mode >= 4 and more than one extra channel) and clamp (9; mode >= 3)
static void write_patch_dictionary(BitWriter &bw, int num_ec) {
	if (!patch_flag()) return;
	CodeSpecW spec;
	std::vector<uint8_t> map(10);
	for (int i = 0; i < 10; ++i) map[(size_t) i] = (uint8_t) (i % 3);
	spec.init(10, map, 3);
	spec.log_alpha = 8;
	for (auto &c : spec.cfg) c = HybridCfg{4, 2, 0};
	StreamEncoder enc(spec);
	auto fold = [](long long v) { return (uint32_t) (v >= 0 ? 2 * v : -2 * v - 1); };
	enc.add(0, (uint32_t) g_patch->refs.size());
	for (const PatchRef &r : g_patch->refs) {
		enc.add(1, (uint32_t) r.ref); enc.add(3, (uint32_t) r.x0); enc.add(3, (uint32_t) r.y0); enc.add(2, (uint32_t) (r.w - 1)); enc.add(2, (uint32_t) (r.h - 1));
		enc.add(7, (uint32_t) (r.at.size() - 1));
		for (size_t j = 0; j < r.at.size(); ++j) {
			const PatchPlace &q = r.at[j];
			if (j == 0) { enc.add(4, (uint32_t) q.x); enc.add(4, (uint32_t) q.y); }
			else { enc.add(6, fold(q.x - r.at[j - 1].x)); enc.add(6, fold(q.y - r.at[j - 1].y)); }
			for (int e = 0; e <= num_ec; ++e) {
				const int mode = e == 0 ? q.mode : g_patch->ec_mode;
				enc.add(5, (uint32_t) mode);
				if (mode >= 4 && num_ec > 1) enc.add(8, 0);
				if (mode >= 3) enc.add(9, (uint32_t) (e == 0 ? q.clamp : 0));
			}
		}
	}
	count_stream(spec, enc);
	write_code_spec(bw, spec);
	enc.flush(bw);
}
// patchcut=1: true when LfGlobal is to end here, in the middle of the dictionary that has just been written into the empty `bw`
static bool cut_patch_dictionary(BitWriter &bw) {
	if (!patch_flag() || !g_patch->cut) return false;
	bw.pad();
	bw.bytes.resize(bw.bytes.size() / 2);
	return true;
}

// noise=v0,...,v7: the frame being written has the noise flag (FrameHeader.flags bit 0) and its eight NoiseParameters, u(10) each, in
// LfGlobal behind the patch dictionary and the splines (splines=, below). Both LfGlobal writers.
//   twin (noisetwin=1): the frame without the flag and without the parameters, every other byte alike
struct NoiseRole { int v[8] = {0, 0, 0, 0, 0, 0, 0, 0}; bool twin = false; };
static NoiseRole *g_noise = nullptr;
static bool noise_flag() { return g_noise && !g_noise->twin; }
static void write_noise_parameters(BitWriter &bw) {
	if (!noise_flag()) return;
	for (int i = 0; i < 8; ++i) bw.put((uint64_t) g_noise->v[i], 10);
}
// (the Modular writer has a noise=N of its own, the amplitude of its samples' noise: one integer. Eight of them are these parameters.)
static bool photon_noise_given(const Options &opt) { return opt.kv.count("noise") && opt.gets("noise", "").find(',') != std::string::npos; }
static void parse_noise_role(const std::string &s, NoiseRole *r) {
	int *v = r->v;
	if (sscanf(s.c_str(), "%d,%d,%d,%d,%d,%d,%d,%d", v, v + 1, v + 2, v + 3, v + 4, v + 5, v + 6, v + 7) != 8) die("noise=v0,...,v7 (eight integers 0..1023)");
	for (int i = 0; i < 8; ++i) if (v[i] < 0 || v[i] > 1023) die("noise=: a value outside 0..1023");
}

// splines=: the splines of the frame being written: the frame has the splines flag (FrameHeader.flags bit 4) and the spline data in
// LfGlobal between the patch dictionary and the noise parameters. Both LfGlobal writers. A description is a list of splines separated
// by '/'; a spline is  x,y[:dx,dy...][|c:i=v,...]  -- its starting point, the double deltas of its further control points as the stream
// holds them (delta += d, point += delta), and a sparse list of quantised coefficients, c = 0 X, 1 Y, 2 B, 3 sigma, i = 0..31. qadj=: the
// quantisation adjustment. Nothing is checked: what a decoder has to refuse is written as it stands. splinecount=N: the stream says N
// splines whatever follows; splinen=N: the first spline says N further control points whatever follows.
//   twin (splinetwin=1): the frame without the flag and without the data, every other byte alike
//   cut (splinecut=1): LfGlobal ends in the middle of the spline data (frames with several sections)
// One entropy-coded stream over 6 contexts (three clusters, ANS): count - 1 (context 2); per spline x, y (1; from the second spline on the
// sign-folded differences to the one before); the adjustment, sign-folded (0); per spline its number of control points (3), their double
// deltas, sign-folded (4), and 4 x 32 coefficients, sign-folded (5)
struct SplineW { long long x = 0, y = 0; std::vector<long long> dd; int coef[4][32]; SplineW() { memset(coef, 0, sizeof coef); } };
struct SplineRole { std::vector<SplineW> splines; int qadj = 0; long long count = -1, first_n = -1; bool twin = false, cut = false; };
static SplineRole *g_spline = nullptr;
static bool spline_flag() { return g_spline && !g_spline->twin; }
static void write_splines(BitWriter &bw) {
	if (!spline_flag()) return;
	CodeSpecW spec;
	std::vector<uint8_t> map(6);
	for (int i = 0; i < 6; ++i) map[(size_t) i] = (uint8_t) (i % 3);
	spec.init(6, map, 3);
	spec.log_alpha = 8;
	for (auto &c : spec.cfg) c = HybridCfg{4, 2, 0};
	StreamEncoder enc(spec);
	auto fold = [](long long v) { return (uint32_t) (v >= 0 ? 2 * v : -2 * v - 1); };
	const std::vector<SplineW> &sp = g_spline->splines;
	enc.add(2, (uint32_t) ((g_spline->count >= 0 ? g_spline->count : (long long) sp.size()) - 1));
	for (size_t i = 0; i < sp.size(); ++i) {
		if (i == 0) { enc.add(1, (uint32_t) sp[i].x); enc.add(1, (uint32_t) sp[i].y); }
		else { enc.add(1, fold(sp[i].x - sp[i - 1].x)); enc.add(1, fold(sp[i].y - sp[i - 1].y)); }
	}
	enc.add(0, fold(g_spline->qadj));
	for (size_t i = 0; i < sp.size(); ++i) {
		enc.add(3, (uint32_t) (i == 0 && g_spline->first_n >= 0 ? g_spline->first_n : (long long) sp[i].dd.size() / 2));
		for (long long d : sp[i].dd) enc.add(4, fold(d));
		for (int c = 0; c < 4; ++c) for (int k = 0; k < 32; ++k) enc.add(5, fold(sp[i].coef[c][k]));
	}
	count_stream(spec, enc);
	write_code_spec(bw, spec);
	enc.flush(bw);
}
// splinecut=1: true when LfGlobal is to end here, in the middle of the spline data that has just been written behind `before` bytes of `bw`
static bool cut_splines(BitWriter &bw, size_t before) {
	if (!spline_flag() || !g_spline->cut) return false;
	bw.pad();
	bw.bytes.resize(before + (bw.bytes.size() - before) / 2);
	return true;
}
static void parse_spline_role(const std::string &text, SplineRole *r) {
	size_t at = 0;
	while (at <= text.size()) {
		size_t end = text.find('/', at);
		if (end == std::string::npos) end = text.size();
		const std::string one = text.substr(at, end - at);
		at = end + 1;
		if (one.empty()) continue;
		SplineW w;
		const size_t bar = one.find('|');
		const std::string pts = one.substr(0, bar), coefs = bar == std::string::npos ? std::string() : one.substr(bar + 1);
		size_t p = 0; bool first = true;
		while (p <= pts.size()) {
			size_t q = pts.find(':', p);
			if (q == std::string::npos) q = pts.size();
			long long a = 0, b = 0;
			if (sscanf(pts.substr(p, q - p).c_str(), "%lld,%lld", &a, &b) != 2) die("splines=: a point is x,y");
			if (first) { w.x = a; w.y = b; first = false; } else { w.dd.push_back(a); w.dd.push_back(b); }
			p = q + 1;
		}
		p = 0;
		while (p < coefs.size()) {
			size_t q = coefs.find(',', p);
			if (q == std::string::npos) q = coefs.size();
			int c = 0, i = 0, v = 0;
			if (sscanf(coefs.substr(p, q - p).c_str(), "%d:%d=%d", &c, &i, &v) != 3 || c < 0 || c > 3 || i < 0 || i > 31) die("splines=: a coefficient is c:i=v, c = 0..3, i = 0..31");
			w.coef[c][i] = v;
			p = q + 1;
		}
		r->splines.push_back(w);
	}
	if (r->splines.empty()) die("splines=: no spline");
}
static void spline_role_options(const Options &opt, SplineRole *r) {
	r->qadj = opt.geti("qadj", 0); r->twin = opt.geti("splinetwin", 0) != 0; r->cut = opt.geti("splinecut", 0) != 0;
	r->count = opt.kv.count("splinecount") ? atoll(opt.gets("splinecount", "").c_str()) : -1;
	r->first_n = opt.kv.count("splinen") ? atoll(opt.gets("splinen", "").c_str()) : -1;
}
static const char *const SPLINE_KEYS[] = {"splines", "qadj", "splinetwin", "splinecut", "splinecount", "splinen"};

// LF frames (lflevels=1|2; run_lf_sequence): what the VarDCT writer is told about the frame it writes, and what it hands back for the
// next one. The planes of integers are frame-wide, ceil(W / 8) cells a row, in streamed order Y, X, B.
struct LfRole {
	int level = 0;              // > 0: the frame is an LF frame of this level (type 1, lf_level, no placement fields)
	bool use = false;           // use_lf_frame: no upsampling fields, and its LfGroups hold neither extra_precision nor the LF stream
	bool replicate = false;     // its LF integers are `src`'s, each over 8 x 8 cells (a flat LF frame's picture under it, or that frame's twin)
	std::vector<int32_t> src[3]; int src_w = 0;
	std::vector<int32_t> out[3]; int out_w = 0;   // out: the integers it ended up with
	std::vector<float> pic[3];  // an LF frame of a picture: its W x H samples (X, Y, B)
	bool capture = false;       // out: the 8 x 8 cell means of its samples (forward=1), what its decoder's LF chroma-from-luma adds taken off
	std::vector<float> means[3]; int means_w = 0, means_h = 0;
	int lfidx_distinct = 0;     // out: how many values its cells' LF index takes
};
static LfRole *g_lf = nullptr;
// lfmodular=1 (lflevels=; run_lf_sequence): the Modular writer codes these three planes (c0, c1, c2: quantised Y, X, B - Y on a grid of
// cells `src_w` wide, each cell over 8 x 8 samples) as an LF frame of `level` (type 1, lf_level, no placement fields) of an XYB image
struct ModularLfRole { int level = 0; std::vector<int32_t> src[3]; int src_w = 0; };
static ModularLfRole *g_mod_lf = nullptr;

// forward opsin (numerical inverse of the decoder's default inverse matrix, j40.h:3109): sRGB samples in [0, 1] to X, Y, B. The VarDCT
// writer's to_xyb, and what xybpic=1 quantises in Modular mode.
struct ForwardOpsin {
	double fwd[3][3], bias, cbias;
	ForwardOpsin() {
		const double inv[3][3] = {
			{11.031566901960783, -9.866943921568629, -0.16462299647058826},
			{-3.254147380392157, 4.418770392156863, -0.16462299647058826},
			{-3.6588512862745097, 2.7129230470588235, 1.9459282392156863}};
		double a = inv[0][0], b = inv[0][1], c = inv[0][2], d = inv[1][0], e = inv[1][1], f = inv[1][2], g = inv[2][0], h = inv[2][1], i = inv[2][2];
		double det = a * (e * i - f * h) - b * (d * i - f * g) + c * (d * h - e * g);
		fwd[0][0] = (e * i - f * h) / det; fwd[0][1] = (c * h - b * i) / det; fwd[0][2] = (b * f - c * e) / det;
		fwd[1][0] = (f * g - d * i) / det; fwd[1][1] = (a * i - c * g) / det; fwd[1][2] = (c * d - a * f) / det;
		fwd[2][0] = (d * h - e * g) / det; fwd[2][1] = (b * g - a * h) / det; fwd[2][2] = (a * e - b * d) / det;
		bias = -0.0037930732552754493; cbias = cbrt(bias);
	}
	void operator()(const float rgb[3], double xyb[3]) const {
		double lin[3];
		for (int c = 0; c < 3; ++c) { double v = rgb[c]; lin[c] = v <= 0.04045 ? v / 12.92 : pow((v + 0.055) / 1.055, 2.4); }
		double mix[3];
		for (int c = 0; c < 3; ++c) mix[c] = cbrt(fwd[c][0] * lin[0] + fwd[c][1] * lin[1] + fwd[c][2] * lin[2] - bias) + cbias;
		xyb[0] = (mix[0] - mix[1]) * 0.5; xyb[1] = (mix[0] + mix[1]) * 0.5; xyb[2] = mix[2];
	}
};

// orientation=N (1..8, every mode): ImageMetadata.extra_fields carries orientation - 1; 0: the option was not given
static int g_orientation = 0;
// tone=IT,MIN[,LINEAR_BELOW[,RELATIVE]] (vardct, and modular with xyb=1): extra fields (orientation 1 and nothing else unless other options say otherwise) and
// ToneMapping written out: intensity_target, min_nits, linear_below as f16 bits, relative_to_max_display. Empty: the option was not given
static std::vector<uint32_t> g_tone;
// opsin=M00,..,M22,B0,B1,B2,Q0,Q1,Q2,QNUM (vardct, and modular with xyb=1): default_m = 0 and the custom-transform block: opsin_inv_mat row-major, opsin_bias,
// quant_bias, quant_bias_num as f16, then cw_mask = 0 (cwmask=1..7: a stream decoders refuse). A value is a decimal number that an
// f16 holds exactly, or `h` and four hex digits: the f16's bits as they are (h7c00: an infinity, which decoders refuse as well)
static std::vector<uint32_t> g_opsin;
static int g_cw_mask = 0;
// upsampling=2|4|8 (vardct, and modular with xyb=1; a single frame): the frame header says upsampling = K and every extra channel's
// ec_upsampling = K. The positional size stays the CODED one; the image header states the SHOWN size, upshown=W,H (default K * coded),
// which must satisfy coded = ceil(shown / K).
//   upweights=nearest|default|V,V,...: the K's custom weight table in the image header (default_m = 0, the mask bit of that K, 15 / 55 /
//     210 F16). nearest: M[i][j] = 1 where i % 5 == 2 && j % 5 == 2, else 0 -- every output is its coded sample; a list: the packed upper
//     triangle, each value rounded to F16; default: no table (a decoder takes the standard's). A stream with a table writes the transform
//     block out: opsin='s values, else the format's defaults rounded to F16.
//   uptwin=1: the same coded frame with upsampling = 1, the coded size in the image header and no table (its transform block as above,
//     so that both streams render alike).
//     uptwin=2: the twin keeps the table (custom weights in an image whose frame has upsampling = 1).
//   ecup=1|2|4|8: the extra channels' ec_upsampling says this instead of K (streams a decoder refuses: "usmp" below K, "TODO" above)
struct UpRole { int k = 1, shown_w = 0, shown_h = 0, twin = 0, ecup = 0; bool block = false; std::vector<uint32_t> table; };
static UpRole g_up;
static bool up_flag() { return g_up.k > 1 && !g_up.twin; }
static int up_log_of(int k) { return k == 2 ? 1 : k == 4 ? 2 : k == 8 ? 3 : 0; }
static int up_log() { return up_flag() ? up_log_of(g_up.k) : 0; }
static int up_ec_log() { return g_up.ecup ? up_log_of(g_up.ecup) : up_log(); }   // (ecup= holds for a twin too: ec_upsampling beside upsampling = 1)
// cenc=1 and its family (every mode): ColourEncoding written out instead of all_default -- RGB, no ICC profile, then white=N (1 D65, 2 custom
// with whitexy=X,Y, 10 E, 11 DCI), primaries=N (1 sRGB, 2 custom with primxy=RX,RY,GX,GY,BX,BY, 9 BT.2100, 11 P3), gamma=G (have_gamma, G in
// units of 1e-7) or tf=N (1 BT.709, 2 unknown, 8 linear, 13 sRGB, 16 PQ, 17 DCI, 18 HLG), intent=N. The xy values are integers of 1e-6. Any
// of the family implies cenc=1. Nothing else of the stream changes: the coefficients are those of the stream without it.
static struct { bool set = false; int white = 1, primaries = 1, tf = 13, gamma = 0, intent = 1; int whitexy[2] = {312700, 329000}; int primxy[6] = {640000, 330000, 300000, 600000, 150000, 60000}; } g_cenc;
static void put_enum(BitWriter &cs, int v) {   // Enum: U32(0, 1, 2 + u(4), 18 + u(6))
	if (v < 2) cs.put((uint64_t) v, 2);
	else if (v < 18) { cs.put(2, 2); cs.put((uint64_t) (v - 2), 4); }
	else { cs.put(3, 2); cs.put((uint64_t) (v - 18), 6); }
}
static void put_customxy_value(BitWriter &cs, int v) {   // U32(u(19), 0x80000 + u(19), 0x100000 + u(20), 0x200000 + u(21)) of the sign-folded value
	const uint32_t u = v >= 0 ? (uint32_t) v << 1 : ((uint32_t) (-(int64_t) v) << 1) - 1;
	if (u < 0x80000u) { cs.put(0, 2); cs.put(u, 19); }
	else if (u < 0x100000u) { cs.put(1, 2); cs.put(u - 0x80000u, 19); }
	else if (u < 0x200000u) { cs.put(2, 2); cs.put(u - 0x100000u, 20); }
	else { if (u - 0x200000u >= (1u << 21)) die("cenc: xy value out of range"); cs.put(3, 2); cs.put(u - 0x200000u, 21); }
}
// ColourEncoding as cenc= states it; false (and nothing written): the option was not given, the caller writes its own
static bool write_colour_encoding(BitWriter &cs) {
	if (!g_cenc.set) return false;
	cs.put(0, 1); cs.put(0, 1);         // not all_default, no ICC profile
	put_enum(cs, 0);                    // colour_space = RGB
	put_enum(cs, g_cenc.white);
	if (g_cenc.white == 2) for (int v : g_cenc.whitexy) put_customxy_value(cs, v);
	put_enum(cs, g_cenc.primaries);
	if (g_cenc.primaries == 2) for (int v : g_cenc.primxy) put_customxy_value(cs, v);
	if (g_cenc.gamma) { cs.put(1, 1); cs.put((uint64_t) g_cenc.gamma, 24); }
	else { cs.put(0, 1); put_enum(cs, g_cenc.tf); }
	put_enum(cs, g_cenc.intent);
	return true;
}

// ImageMetadata.extra_fields (j40.h:3147-3163): 0, or for an animation: orientation 1, no intrinsic size, no preview, the animation
// header (tps 10 / 1, loops 0, no timecodes); with orientation=N: extra fields with that orientation (and, outside an animation,
// nothing else)
static void write_extra_fields(BitWriter &cs) {
	const bool anim = g_seq && g_seq->anim;
	if (!anim && !g_orientation && g_tone.empty()) { cs.put(0, 1); return; }
	cs.put(1, 1);
	cs.put((uint64_t) (g_orientation ? g_orientation - 1 : 0), 3); cs.put(0, 1); cs.put(0, 1);   // orientation - 1, have_intrinsic_size, have_preview
	if (!anim) { cs.put(0, 1); return; }            // have_animation
	cs.put(1, 1);                                   // have_animation
	cs.put(2, 2); cs.put(9, 10);                    // tps_numerator U32(100, 1000, 1 + u(10), 1 + u(30)) = 10
	cs.put(0, 2);                                   // tps_denominator U32(1, 1001, 1 + u(8), 1 + u(10)) = 1
	cs.put(0, 2);                                   // num_loops U32(0, u(3), u(16), u(32)) = 0
	cs.put(0, 1);                                   // have_timecodes
}

// the frame header from have_crop to save_before_color_transform (j40.h:5285-5336). Outside a sequence: no crop, Replace, is_last.
static void write_frame_placement(BitWriter &cs, int num_ec, int frame_w, int frame_h) {
	auto crop_u32 = [&](long long v) { cs.u32(v, 0, 8, 256, 11, 2304, 14, 18688, 30); };
	auto pack_signed = [](int v) { return v >= 0 ? 2ll * v : -2ll * v - 1; };
	if (!g_seq) {
		cs.put(0, 1);                       // have_crop
		for (int i = -1; i < num_ec; ++i) cs.u32(0, 0, 0, 1, 0, 2, 0, 3, 2);  // blend mode: replace (the frame's, then each extra channel's, j40.h:5299)
		cs.put(1, 1);                       // is_last
		return;
	}
	const SeqFrame &q = *g_seq;
	bool full_frame = true;
	if (q.type == 2) {   // a reference-only frame: its size alone, no blend info, no duration, never last (j40.h:5285-5336)
		cs.put(q.have_crop ? 1 : 0, 1);
		if (q.have_crop) { crop_u32(frame_w); crop_u32(frame_h); }
		cs.put((uint64_t) q.save, 2);
		cs.put((uint64_t) q.save_before_ct, 1);
		return;
	}
	cs.put(q.have_crop ? 1 : 0, 1);
	if (q.have_crop) {
		crop_u32(pack_signed(q.x0)); crop_u32(pack_signed(q.y0)); crop_u32(frame_w); crop_u32(frame_h);
		full_frame = q.x0 <= 0 && q.y0 <= 0 && frame_w + q.x0 >= q.canvas_w && frame_h + q.y0 >= q.canvas_h;
	}
	for (int i = -1; i < num_ec; ++i) {
		const int blend = i < 0 ? q.blend : q.ec_blend, src = i < 0 ? q.src : q.ec_src;
		cs.u32(blend, 0, 0, 1, 0, 2, 0, 3, 2);
		if (num_ec > 0) {
			if (blend == 2 || blend == 3) { cs.u32(0, 0, 0, 1, 0, 2, 0, 3, 3); cs.put(0, 1); }   // alpha channel 0, no clamp
			else if (blend == 4) cs.put(0, 1);
		}
		if (!full_frame || blend != 0) cs.put((uint64_t) src, 2);
	}
	if (q.anim) {   // duration U32(0, 1, u(8), u(32))
		if (q.duration == 0) cs.put(0, 2); else if (q.duration == 1) cs.put(1, 2); else if (q.duration < 256) { cs.put(2, 2); cs.put((uint64_t) q.duration, 8); } else { cs.put(3, 2); cs.put((uint64_t) q.duration, 32); }
	}
	cs.put(q.is_last ? 1 : 0, 1);
	if (!q.is_last) cs.put((uint64_t) q.save, 2);
	if (full_frame && q.blend == 0 && (q.duration == 0 || q.save != 0) && !q.is_last) cs.put(0, 1);   // save_before_color_transform
}

// the frame a writer has finished goes behind the codestream so far (every frame ends on a byte: its sections are whole bytes)
static void seq_append(const BitWriter &frame, const std::vector<std::vector<uint8_t>> &sections) {
	size_t stored = 0;
	for (const auto &sec : sections) stored += sec.size();
	g_seq->cs->insert(g_seq->cs->end(), frame.bytes.begin(), frame.bytes.end());
	g_seq->first_section = g_seq->cs->size() - stored;
}

// wp=random|max|zero|<eleven numbers>: weighted-predictor parameters other than the defaults (false: the option is absent)
static bool parse_wp(const Options &opt, uint64_t seed, WPParams &wp_base, const char *mode) {
	if (!opt.kv.count("wp")) return false;
	const std::string v = opt.gets("wp", "");
	int *f[11] = {&wp_base.p1, &wp_base.p2, &wp_base.p3[0], &wp_base.p3[1], &wp_base.p3[2], &wp_base.p3[3], &wp_base.p3[4], &wp_base.w[0], &wp_base.w[1], &wp_base.w[2], &wp_base.w[3]};
	if (v == "random") { SplitMix64 r(seed ^ 0x57505750ull); for (int i = 0; i < 11; ++i) *f[i] = (int) r.below(i < 7 ? 32 : 16); }
	else if (v == "max") for (int i = 0; i < 11; ++i) *f[i] = i < 7 ? 31 : 15;
	else if (v == "zero") for (int i = 0; i < 11; ++i) *f[i] = 0;
	else if (sscanf(v.c_str(), "%d,%d,%d,%d,%d,%d,%d,%d,%d,%d,%d", f[0], f[1], f[2], f[3], f[4], f[5], f[6], f[7], f[8], f[9], f[10]) != 11) dief("%s: wp=random|max|zero|p1,p2,p3a,p3b,p3c,p3d,p3e,w0,w1,w2,w3", mode);
	for (int i = 0; i < 11; ++i) if (*f[i] < 0 || *f[i] > (i < 7 ? 31 : 15)) dief("%s: wp: p1, p2, p3* are 5-bit and w* 4-bit fields", mode);
	return true;
}

// (stats=1) the headers that carry weighted-predictor parameters of their own, and the use the writer's trees made of the predictor
static std::string wp_stats_json() {
	std::vector<std::array<int, 11>> sets = wp_headers_written();
	const size_t headers = sets.size();
	size_t non_default = 0;
	for (const auto &a : sets) { WPParams p; p.p1 = a[0]; p.p2 = a[1]; for (int i = 0; i < 5; ++i) p.p3[i] = a[2 + i]; for (int i = 0; i < 4; ++i) p.w[i] = a[7 + i]; non_default += !wp_is_default(p); }
	std::sort(sets.begin(), sets.end());
	sets.erase(std::unique(sets.begin(), sets.end()), sets.end());
	char tmp[256];
	snprintf(tmp, sizeof tmp, "\"wp_headers\": %zu, \"wp_non_default_headers\": %zu, \"wp_distinct_sets\": %zu, \"wp_predicted_samples\": %llu, \"wp_property_tests\": %llu",
	         headers, non_default, sets.size(), (unsigned long long) wp_predicted_samples(), (unsigned long long) wp_property_tests());
	return tmp;
}

// ------------------------------------------------------------------------------------------------
// procedural source picture (deterministic, cheap): low-frequency sinusoids + value noise +
// hard-edged rectangles, sRGB in [0,1]

struct Picture {
	uint64_t seed;
	struct Rect { int x0, y0, x1, y1; float r, g, b; };
	std::vector<Rect> rects;
	float fx[6], fy[6], ph[6], amp[6][3];
	int W, H;
	Picture(int w, int h, uint64_t s) : seed(s), W(w), H(h) {
		SplitMix64 rng(s ^ 0x4A34304Aull);
		for (int i = 0; i < 6; ++i) {
			fx[i] = (float) (rng.unit() * 6.0 / w); fy[i] = (float) (rng.unit() * 6.0 / h); ph[i] = (float) (rng.unit() * 6.28318);
			for (int c = 0; c < 3; ++c) amp[i][c] = (float) (rng.unit() * 0.09);
		}
		int nrect = 24;
		for (int i = 0; i < nrect; ++i) {
			Rect r; r.x0 = (int) rng.below((uint32_t) w); r.y0 = (int) rng.below((uint32_t) h);
			r.x1 = r.x0 + 8 + (int) rng.below((uint32_t) std::max(9, w / 4)); r.y1 = r.y0 + 8 + (int) rng.below((uint32_t) std::max(9, h / 4));
			r.r = (float) (rng.unit() * 0.3 - 0.15); r.g = (float) (rng.unit() * 0.3 - 0.15); r.b = (float) (rng.unit() * 0.3 - 0.15);
			rects.push_back(r);
		}
	}
	static float hash01(uint64_t a) { a *= 0x9e3779b97f4a7c15ull; a ^= a >> 29; a *= 0xbf58476d1ce4e5b9ull; a ^= a >> 32; return (float) (a & 0xffffff) * (1.0f / 16777216.0f); }
	float vnoise(float x, float y, int oct, int ch) const {
		float sc = (float) (1 << oct) * 4.0f / (float) std::max(W, H);
		float u = x * sc, v = y * sc; int iu = (int) u, iv = (int) v; float fu = u - (float) iu, fv = v - (float) iv;
		auto hv = [&](int a, int b) { return hash01(seed * 31 + (uint64_t) a * 73856093ull + (uint64_t) b * 19349663ull + (uint64_t) oct * 83492791ull + (uint64_t) ch * 2654435761ull); };
		float su = fu * fu * (3 - 2 * fu), sv = fv * fv * (3 - 2 * fv);
		return (hv(iu, iv) * (1 - su) + hv(iu + 1, iv) * su) * (1 - sv) + (hv(iu, iv + 1) * (1 - su) + hv(iu + 1, iv + 1) * su) * sv;
	}
	// the smooth part of the picture (no rectangles, not clamped) / the rectangles' contribution: forward=1 evaluates the former
	// on a coarse grid
	void smooth(float x, float y, float out[3]) const {
		for (int c = 0; c < 3; ++c) {
			float v = 0.5f;
			for (int i = 0; i < 6; ++i) v += amp[i][c] * sinf(fx[i] * x * 6.28318f + fy[i] * y * 6.28318f + ph[i] + (float) c);
			for (int o = 0; o < 3; ++o) v += (vnoise(x, y, o, c) - 0.5f) * (0.16f / (float) (1 << o));
			out[c] = v;
		}
	}
	void add_rects(float x, float y, float out[3]) const {
		for (const Rect &r : rects) if (x >= (float) r.x0 && x < (float) r.x1 && y >= (float) r.y0 && y < (float) r.y1) { out[0] += r.r; out[1] += r.g; out[2] += r.b; }
	}
	void rgb(float x, float y, float out[3]) const {
		for (int c = 0; c < 3; ++c) {
			float v = 0.5f;
			for (int i = 0; i < 6; ++i) v += amp[i][c] * sinf(fx[i] * x * 6.28318f + fy[i] * y * 6.28318f + ph[i] + (float) c);
			for (int o = 0; o < 3; ++o) v += (vnoise(x, y, o, c) - 0.5f) * (0.16f / (float) (1 << o));
			out[c] = v;
		}
		for (const Rect &r : rects) if (x >= (float) r.x0 && x < (float) r.x1 && y >= (float) r.y0 && y < (float) r.y1) { out[0] += r.r; out[1] += r.g; out[2] += r.b; }
		for (int c = 0; c < 3; ++c) out[c] = std::min(0.92f, std::max(0.08f, out[c]));
	}
};

// ------------------------------------------------------------------------------------------------
// headers

static void write_size_header(BitWriter &bw, int w, int h) {  // inverse of j40.h:3008
	if (w % 8 == 0 && h % 8 == 0 && w <= 256 && h <= 256) {
		bw.put(1, 1); bw.put((uint64_t) (h / 8 - 1), 5);
		if (w == h) bw.put(1, 3); else { bw.put(0, 3); bw.put((uint64_t) (w / 8 - 1), 5); }
	} else {
		bw.put(0, 1); bw.u32(h, 1, 9, 1, 13, 1, 18, 1, 30);
		if (w == h) bw.put(1, 3); else { bw.put(0, 3); bw.u32(w, 1, 9, 1, 13, 1, 18, 1, 30); }
	}
}

static void write_toc_entry(BitWriter &bw, size_t size) { bw.u32((int64_t) size, 0, 10, 1024, 14, 17408, 22, 4211712, 30); }  // j40.h:5529

// IEEE half for values that are exactly representable (all the parameters below are)
static uint32_t f16_bits(float v) {
	if (v == 0.0f) return 0;
	uint32_t u; memcpy(&u, &v, 4);
	const uint32_t sign = u >> 31, mant = u & 0x7fffff; const int e = (int) ((u >> 23) & 0xff) - 127 + 15;
	if (e <= 0 || e >= 31 || (mant & 0x1fff)) die("f16: value not exactly representable");
	return sign << 15 | (uint32_t) e << 10 | mant >> 13;
}
// the nearest f16 (ties to even) of a value within the normal range, or of zero (upweights=, and the default transform beside it)
static uint32_t f16_round_bits(float v) {
	if (v == 0.0f) return 0;
	uint32_t u; memcpy(&u, &v, 4);
	const uint32_t sign = u >> 31;
	uint32_t mag = u & 0x7fffffffu;
	if (mag < 0x38800000u) {   // below 2^-14: the subnormals' step, 2^-24
		const float a = v < 0 ? -v : v;
		const uint32_t q = (uint32_t) lrintf(a * 16777216.0f);   // (ties to even in the default rounding mode)
		return sign << 15 | q;   // (q = 1024 is the smallest normal: the bit pattern carries over)
	}
	mag += 0xfffu + (mag >> 13 & 1);   // round the 13 dropped bits, ties to even
	const int e = (int) (mag >> 23) - 127 + 15;
	if (e >= 31) die("f16: value out of range");
	return sign << 15 | (uint32_t) e << 10 | (mag >> 13 & 0x3ff);
}

// ... and what they add behind ColourEncoding: ToneMapping (j40.h:3270-3286), all_default unless tone= is given
static void write_tone_mapping(BitWriter &cs) {
	if (!(g_seq && g_seq->anim) && !g_orientation && g_tone.empty()) return;
	if (g_tone.empty()) { cs.put(1, 1); return; }
	cs.put(0, 1);
	cs.put(g_tone[0], 16); cs.put(g_tone[1], 16);   // intensity_target, min_nits
	cs.put(g_tone[3] ? 1 : 0, 1);                   // relative_to_max_display
	cs.put(g_tone[2], 16);                          // linear_below
}
// the end of the image header (j40.h:3270-3307). Behind a written-out ImageMetadata (`metadata`): ToneMapping, no extensions; then in
// either case default_m, and with opsin=: the 16 values (in an XYB image only, as the format says) and cw_mask
static void write_header_tail(BitWriter &cs, bool metadata, bool xyb) {
	if (metadata) { write_tone_mapping(cs); cs.put(0, 2); }   // extensions
	if (g_opsin.empty() && !g_up.block) { cs.put(1, 1); return; }            // default_m
	cs.put(0, 1);
	if (xyb && !g_opsin.empty()) for (size_t i = 0; i < 16; ++i) cs.put(g_opsin[i], 16);
	else if (xyb) {   // (upweights=: the format's default transform, as F16 holds it)
		static const float DEFAULTS[16] = {11.031566901960783f, -9.866943921568629f, -0.16462299647058826f, -3.254147380392157f, 4.418770392156863f, -0.16462299647058826f,
			-3.6588512862745097f, 2.7129230470588235f, 1.9459282392156863f, -0.0037930732552754493f, -0.0037930732552754493f, -0.0037930732552754493f,
			1.0f - 0.05465007330715401f, 1.0f - 0.07005449891748593f, 1.0f - 0.049935103337343655f, 0.145f};
		for (float v : DEFAULTS) cs.put(f16_round_bits(v), 16);
	}
	const int up_bit = (up_flag() || g_up.twin == 2) && !g_up.table.empty() ? g_up.k >> 1 : 0;   // (K = 2: bit 0, 4: bit 1, 8: bit 2)
	cs.put((uint64_t) (g_cw_mask | up_bit), 3);
	if (up_bit) for (uint32_t v : g_up.table) cs.put(v, 16);
}

// dq=1: the dequantisation matrices of HfGlobal in their coded forms (j40.h:4696-4760) instead of "all default": band
// parameters for DCT8, the Hornuss, DCT2x2, DCT4x4, DCT4x8 and AFV forms (the reference accepts the coded forms only for the
// 8x8 matrices, band parameters included: HOW[6].requires8x8, j40.h:4751); values near the library's, rounded to halves. Scaled parameters are stored divided by 64.
static void write_dq_matrices(BitWriter &bw, std::vector<std::pair<int, StreamEncoder>> &raw, const std::function<const WPParams *(int)> &wp_of) {
	auto params = [&](const std::vector<std::array<float, 3>> &p, size_t first, size_t count, size_t scaled) {   // channel-major, as read (j40.h:4738)
		for (int c = 0; c < 3; ++c) for (size_t j = 0; j < count; ++j) bw.put(f16_bits(p[first + j][(size_t) c] / (j < scaled ? 64.0f : 1.0f)), 16);
	};
	auto bands = [&](const std::vector<std::array<float, 3>> &p) { bw.put((uint64_t) (p.size() - 1), 4); params(p, 0, p.size(), 1); };
	const std::vector<std::array<float, 3>> dct8 = {{3136, 576, 512}, {0, 0, -2}, {-0.5f, -0.25f, -1}, {-0.5f, -0.25f, 0}, {-0.5f, -0.25f, -1}, {-2, -0.25f, -2}};
	const std::vector<std::array<float, 3>> b4x4 = {{2176, 384, 112}, {0, 0, -0.25f}, {0, 0, -0.25f}, {0, 0, -0.5f}};
	const std::vector<std::array<float, 3>> b4x8 = {{2176, 768, 512}, {-1, -1, -1.5f}, {-0.75f, -1, -1.5f}, {-0.625f, -0.25f, -1.5f}};
	for (int idx = 0; idx < 17; ++idx) {
		switch (idx) {
		case 0: bw.put(6, 3); bands(dct8); break;
		case 1: { bw.put(1, 3); const std::vector<std::array<float, 3>> p = {{256, 64, 16}, {3200, 896, 192}, {3072, 832, 208}}; params(p, 0, 3, 3); break; }
		case 2: { bw.put(2, 3); const std::vector<std::array<float, 3>> p = {{3840, 960, 640}, {2560, 640, 320}, {1280, 320, 128}, {640, 180, 64}, {480, 140, 32}, {300, 120, 16}}; params(p, 0, 6, 6); break; }
		case 3: { bw.put(3, 3); const std::vector<std::array<float, 3>> p = {{1, 1, 1}, {2, 1, 0.5f}}; params(p, 0, 2, 2); bands(b4x4); break; }
		case 9: { bw.put(4, 3); const std::vector<std::array<float, 3>> p = {{1, 0.75f, 1.5f}}; params(p, 0, 1, 0); bands(b4x8); break; }
		case 10: {
			bw.put(5, 3);
			const std::vector<std::array<float, 3>> p = {{3072, 1024, 384}, {3072, 1024, 384}, {256, 48, 12}, {256, 48, 12}, {256, 48, 12}, {416, 56, 22}, {0, 0, -0.25f}, {0, 0, -0.25f}, {0, 0, -0.25f}};
			params(p, 0, 9, 6); bands(b4x8); bands(b4x4);
			break;
		}
		default: {
			StreamEncoder *enc = nullptr;
			for (auto &r : raw) if (r.first == idx) enc = &r.second;
			if (!enc) { bw.put(0, 3); break; }   // library
			// raw (j40.h:4712-4745): a denominator, then the weights times it as a three-channel Modular image
			bw.put(7, 3); bw.put(f16_bits(2.0f), 16);
			write_modular_header(bw, true, wp_of(100 + idx), {});
			enc->flush(bw);
		} }
	}
}

// BitDepth of ImageMetadata (j40.h:3175-3190): integer samples, U32(8, 10, 12, 1 + u(6)) bits
static void write_bit_depth(BitWriter &cs, int bpp) {
	cs.put(0, 1);   // not float
	if (bpp == 8) cs.put(0, 2); else if (bpp == 10) cs.put(1, 2); else if (bpp == 12) cs.put(2, 2); else { cs.put(3, 2); cs.put((uint64_t) (bpp - 1), 6); }
}

// TOC + sections (j40.h:5505-5543). permute != 0: the sections are stored in a shuffled order and the TOC carries the
// Lehmer-coded permutation that puts them back (the decoder applies it to the list of stored sections, j40.h:5540).
static void write_toc_and_sections(BitWriter &cs, const std::vector<std::vector<uint8_t>> &sections_in, int permute, SplitMix64 &rng, int slack = 0) {
	// slack=K: K junk bytes behind the data of every non-empty section. The reference does not notice them in frames with more
	// than one section (j40__finish_section_state drops the error of its own j40__no_more_bytes, j40.h:7778-7795)
	std::vector<std::vector<uint8_t>> sections = sections_in;
	if (slack) for (auto &s : sections) if (!s.empty()) for (int k = 0; k < slack; ++k) s.push_back((uint8_t) (0xa5 + 17 * k));
	const size_t n = sections.size();
	std::vector<size_t> stored_at(n);   // logical section i is the stored_at[i]-th stored one
	for (size_t i = 0; i < n; ++i) stored_at[i] = i;
	if (!permute || n < 3) cs.put(0, 1);
	else {
		const size_t end = n - 1 - (size_t) rng.below((uint32_t) std::min<size_t>(n - 2, 5));
		std::vector<uint32_t> lehmer(end);
		for (size_t i = 0; i < end; ++i) lehmer[i] = rng.below((uint32_t) std::min<size_t>(n - i, 40));
		{   // what the decoder's j40__apply_permutation makes of the stored list
			size_t *target = stored_at.data();
			for (uint32_t x : lehmer) { size_t tmp = target[x]; memmove(target + 1, target, sizeof(size_t) * x); target[0] = tmp; ++target; }
		}
		cs.put(1, 1);
		CodeSpecW pspec; pspec.init(8, std::vector<uint8_t>(8, 0), 1); pspec.log_alpha = 6; pspec.cfg[0] = HybridCfg{4, 1, 0};
		StreamEncoder penc(pspec);
		penc.add((uint32_t) std::min(7, ceil_lg((uint32_t) n + 1)), (uint32_t) end);   // j40.h:5437
		uint32_t prev = 0;
		for (uint32_t x : lehmer) { penc.add((uint32_t) std::min(7, ceil_lg(prev + 1)), x); prev = x; }
		count_stream(pspec, penc);
		write_code_spec(cs, pspec); penc.flush(cs);
	}
	cs.pad();
	std::vector<const std::vector<uint8_t> *> stored(n, nullptr);
	for (size_t i = 0; i < n; ++i) stored[stored_at[i]] = &sections[i];
	for (const auto *s : stored) write_toc_entry(cs, s->size());
	cs.pad();
	for (const auto *s : stored) cs.append_bytes(*s);
}

// transform table: the decoder's view (J40__DCT_SELECT, j40.h:4591): log rows, log columns, order
static const int8_t DCTSEL[27][3] = {
	{3,3,0},{3,3,1},{3,3,1},{3,3,1},{4,4,2},{5,5,3},{4,3,4},{3,4,4},{5,3,5},{3,5,5},{5,4,6},{4,5,6},{3,3,1},{3,3,1},
	{3,3,1},{3,3,1},{3,3,1},{3,3,1},{6,6,7},{6,5,8},{5,6,8},{7,7,9},{7,6,10},{6,7,10},{8,8,11},{8,7,12},{7,8,12},
};

// coefficient-context tables (spec constants as used at j40.h:6935-6947), pre-doubled
static const int8_t FREQ_CTX2[64] = {
	-1, 0, 2, 4, 6, 8, 10, 12, 14, 16, 18, 20, 22, 24, 26, 28, 30, 30, 32, 32, 34, 34, 36, 36, 38, 38, 40, 40, 42, 42, 44, 44,
	46, 46, 46, 46, 48, 48, 48, 48, 50, 50, 50, 50, 52, 52, 52, 52, 54, 54, 54, 54, 56, 56, 56, 56, 58, 58, 58, 58, 60, 60, 60, 60,
};
static int nnz_ctx2(int q) {
	static const int16_t LIMIT[8] = {2, 3, 5, 9, 13, 21, 33, 64}, VALUE[8] = {0, 62, 124, 186, 246, 304, 360, 412};
	for (int i = 0; i < 8; ++i) if (q < LIMIT[i]) return VALUE[i];
	return 412;
}

struct LfGroupW {
	int left, top, w, h, w8, h8, w64, h64;
	std::vector<int32_t> blocks;               // per cell: (dctsel + 2) << 20 | voff, 1 << 20 | voff, or 0
	struct VB { int x8, y8, dctsel, hfmul_m1; };
	std::vector<VB> vbs;
	Channel lfq[3];                            // Y, X, B order as streamed
	Channel xfromy, bfromy, blockinfo, sharp;
	std::vector<uint8_t> lfidx;
};

// jpegdata=PATH (vardct): the quantised integers of a baseline JPEG file, as tests/jpeg_ref.py's write_dump lays them out. Little-endian:
// int32 magic "JPGD", width, height; per component Y, Cb, Cr: int32 h factor, v factor, blocks_x, blocks_y (the whole-MCU block grid);
// per component 64 x uint16 quantisation table [v][u] (v: vertical frequency); per component blocks_y x blocks_x x 64 x int16
// coefficients [by][bx][v][u], DC differences undone.
struct JpegDump {
	bool present = false;
	std::string subsampling;
	struct Comp { int h, v, bx, by; uint16_t table[64]; std::vector<int16_t> coef; } comp[3];
	// slot c (0 = Cb, 1 = Y, 2 = Cr: the frame's channels X, Y, B) -> component
	const Comp &slot(int c) const { return comp[c == 1 ? 0 : c == 0 ? 1 : 2]; }
};
// What the stream has to be for the decoder's own rule to give q * Q / (8 * 255) for the JPEG integer q under table entry Q (the
// derivation: DESIGN.md, "YCbCr frames"). The decoder computes adj(n) * mult_c / (px / denom) with mult_1 = 65536 / (global_scale *
// HfMul), mult_0 = 0.8 mult_1 (x_qm_scale keeps its default 3 in a frame that is not XYB), adj(n) = n - 0.145 / n: the weight DIVIDES, its
// integer px cannot be proportional to 1 / Q for every Q, and the bias cannot be switched off. So Q is split, Q = g * f with
// g = gcd(Q, 32640): px = 32640 / g goes into the raw matrix, f into the integer, n = K_c * q * f with K = 2560, 2048, 2048 -- large
// enough that 0.145 / n^2 < 2^-24.
static const int JPEG_L = 32640, JPEG_GLOBAL_SCALE = 2048, JPEG_QUANT_LF = 255, JPEG_K[3] = {2560, 2048, 2048}, JPEG_LF_K[3] = {16, 2, 1};
static const float JPEG_DENOM = 1.0f / 4096.0f;
static int jpeg_gcd(int a, int b) { while (b) { const int t = a % b; a = b; b = t; } return a; }

static JpegDump load_jpeg_dump(const Options &opt, int W, int H) {
	JpegDump jd;
	if (!opt.kv.count("jpegdata")) return jd;
	const char *why = "it implies ycbcr=1, the file's subsampling, DCT8 blocks, one HfMul, one pass, zero chroma-from-luma, skip_adapt_lf_smooth, no filters, 8 bits and its own global_scale and quant_lf";
	if (opt.geti("forward", 0)) dief("vardct: jpegdata= carries a JPEG's integers, forward=1 takes them from the picture (%s)", why);
	if (opt.geti("passes", 1) > 1) dief("vardct: jpegdata= writes one pass (%s)", why);
	if (opt.geti("cfl", 0)) dief("vardct: jpegdata= and cfl=1 exclude each other (%s)", why);
	for (const char *k : {"maxlog", "ycbcr", "subsampling", "global_scale", "quant_lf", "hfmul", "dct8only", "nocfl", "nosmooth", "dq", "gab", "epf", "bpp", "extraprec", "bigshare", "flat", "noxyb", "grey", "flatchroma", "jpegup"})
		if (opt.kv.count(k)) dief("vardct: jpegdata= fixes what %s= would say (%s)", k, why);
	const std::string path = opt.gets("jpegdata", "");
	FILE *fp = fopen(path.c_str(), "rb");
	if (!fp) dief("vardct: jpegdata=%s cannot be read", path.c_str());
	int32_t head[3 + 12];
	if (fread(head, 4, 15, fp) != 15 || head[0] != 0x4447504A) die("vardct: jpegdata= is not a dump of tests/jpeg_ref.py (magic JPGD)");
	if (head[1] != W || head[2] != H) dief("vardct: the dump of jpegdata= holds a picture of %d x %d, the command line says %d x %d", head[1], head[2], W, H);
	for (int i = 0; i < 3; ++i) { JpegDump::Comp &c = jd.comp[i]; c.h = head[3 + 4 * i]; c.v = head[4 + 4 * i]; c.bx = head[5 + 4 * i]; c.by = head[6 + 4 * i]; }
	const int yh = jd.comp[0].h, yv = jd.comp[0].v;
	if (jd.comp[1].h != 1 || jd.comp[1].v != 1 || jd.comp[2].h != 1 || jd.comp[2].v != 1 || yh < 1 || yh > 2 || yv < 1 || yv > 2) die("vardct: jpegdata=: sampling factors other than 4:4:4, 4:2:0, 4:2:2, 4:4:0");
	jd.subsampling = yh == 2 ? (yv == 2 ? "420" : "422") : (yv == 2 ? "440" : "444");
	const int mx = (W + 8 * yh - 1) / (8 * yh), my = (H + 8 * yv - 1) / (8 * yv);
	for (int i = 0; i < 3; ++i) if (jd.comp[i].bx != mx * jd.comp[i].h || jd.comp[i].by != my * jd.comp[i].v) die("vardct: jpegdata=: a component's block grid is not the whole-MCU grid of the picture's size");
	for (int i = 0; i < 3; ++i) {
		if (fread(jd.comp[i].table, 2, 64, fp) != 64) die("vardct: jpegdata=: the file ends inside the tables");
		for (int k = 0; k < 64; ++k) if (jd.comp[i].table[k] < 1 || jd.comp[i].table[k] > 255) die("vardct: jpegdata=: a table entry outside 1..255");
	}
	for (int i = 0; i < 3; ++i) {
		JpegDump::Comp &c = jd.comp[i];
		c.coef.resize((size_t) c.bx * (size_t) c.by * 64);
		if (fread(c.coef.data(), 2, c.coef.size(), fp) != c.coef.size()) die("vardct: jpegdata=: the file ends inside the coefficients");
	}
	if (fgetc(fp) != EOF) die("vardct: jpegdata=: bytes behind the coefficients");
	fclose(fp);
	jd.present = true;
	return jd;
}

static int run_vardct(int W, int H, uint64_t seed, const char *out, const Options &opt) {
	SplitMix64 rng(seed * 0x100000001b3ull + 12345);
	const JpegDump jd = load_jpeg_dump(opt, W, H);
	const bool jpeg = jd.present;
	const int global_scale = jpeg ? JPEG_GLOBAL_SCALE : opt.geti("global_scale", 8192), quant_lf = jpeg ? JPEG_QUANT_LF : opt.geti("quant_lf", 4);
	const double density = opt.getd("density", 0.80), decay = opt.getd("decay", 0.84);
	const int max_log = opt.geti("maxlog", 6);              // largest transform side (log2) used in the mix
	const int coverage = opt.geti("coverage", opt.geti("forward", 0) ? 0 : 1);           // 1: force every transform type <= maxlog at least once per frame
	const int custom_bctx = opt.geti("bctx", 0);            // custom block context map with LF/QF thresholds
	const int num_presets = opt.geti("presets", 1);
	const int custom_orders = opt.geti("orders", 0);
	const int num_passes = opt.geti("passes", 1);
	// ycbcr=1: a YCbCr frame as a recompressed JPEG is one -- implies noxyb=1 and the full frame header, sets do_ycbcr; unlike noxyb
	// alone it does not need alpha=1, and a frame of one group is written as the single section it is. subsampling=444|420|422|440
	// writes jpeg_upsampling (channel c's mode at bits 2c, coded order Cb, Y, Cr; modes 0..3 = sampling factors (1,1), (2,2), (2,1),
	// (1,2)): the block grid padded to whole MCUs, every LF channel at its own size, DCT8 only, skip_adapt_lf_smooth, no filters, zero
	// chroma-from-luma maps, per block only the channels present. flatchroma=1: Cb and Cr constant. dct8only=1, hfmul=N, nocfl=1: what
	// a subsampled stream has anyway, for its 4:4:4 twins (every varblock DCT8; one HfMul; chroma-from-luma coded as all zero).
	// jpegdata=PATH: the frame a JPEG file's quantised integers make (the dump of tests/jpeg_ref.py, laid out above load_jpeg_dump). It
	// implies ycbcr=1, the file's subsampling, dct8only=1, hfmul=1, nocfl=1, nosmooth=1, no filters, 8 bits, global_scale 2048 and
	// quant_lf 255, and writes: DCT8's dequantisation matrix in raw form (denominator 2^-12, 32640 / gcd(Q, 32640) per entry, the
	// table transposed -- the stream's canonical index is 8 * horizontal + vertical frequency --, channels Cb, Y, Cr), the AC integers
	// times K_c * Q / gcd(Q, 32640) in the HF streams, the DC integers times Q_00 * (16, 2, 1 for Cb, Y, Cr) in the LF image.
	const int ycbcr = jpeg ? 1 : opt.geti("ycbcr", 0);
	const std::string subsampling = jpeg ? jd.subsampling : opt.gets("subsampling", "444");
	if (subsampling != "444" && subsampling != "420" && subsampling != "422" && subsampling != "440") die("vardct: subsampling=444|420|422|440");
	const bool subsampled = subsampling != "444";
	if (subsampled && !ycbcr) die("vardct: subsampling wants ycbcr=1");
	// slot order X (Cb), Y, B (Cr)
	const int sub_h = subsampling == "420" || subsampling == "422" ? 1 : 0, sub_v = subsampling == "420" || subsampling == "440" ? 1 : 0;
	const int hs[3] = {sub_h, 0, sub_h}, vs[3] = {sub_v, 0, sub_v};
	const int jpeg_upsampling = subsampling == "420" ? 4 : subsampling == "422" ? 8 : subsampling == "440" ? 12 : 0;
	const int dct8only = jpeg ? 1 : opt.geti("dct8only", subsampled ? 1 : 0), fixed_hfmul = jpeg ? 1 : opt.geti("hfmul", 0), nocfl = jpeg ? 1 : opt.geti("nocfl", 0), flatchroma = opt.geti("flatchroma", 0);
	if (fixed_hfmul < 0 || fixed_hfmul > 256) die("vardct: hfmul=1..256");
	const int nonzero_header = opt.geti("fullheader", (num_passes > 1 || ycbcr || g_noise || g_spline || g_up.k > 1) ? 1 : 0);   // (upsampling=: the twin's header too)
	const int x_qm = opt.geti("xqm", 3), b_qm = opt.geti("bqm", 2);
	const int skip_smooth = jpeg ? 1 : opt.geti("nosmooth", subsampled ? 1 : 0);
	const int small_clusters = opt.geti("simpleclusters", 0); // <= 8 clusters: simple cluster-map form
	const int log_alpha = opt.geti("logalpha", 7);
	const int container = opt.geti("container", 0);
	// coefficient statistics outside what an encoder writes at d1 (all default to that):
	//   bigshare=p bigbits=k  with probability p a non-zero's magnitude is drawn from [2^(k-1), 2^k): uniform, except that one draw in
	//                         eight takes one of the two ends so that the boundary values themselves always occur. Packed, such a
	//                         value has k + 1 bits; the reference's hybrid integers hold 30 (j40.h:2308-2319), so k = 30 is the
	//                         first it refuses ("iovf")
	//   flat=v                every non-zero coefficient is v: next to no entropy per non-zero
	//   hybrid=s,m,l          split_exp, msb_in_token, lsb_in_token of every HF cluster (default: {4,2,0} and {4,1,1} alternating)
	//   extraprec=0..3        the LfGroups' extra_precision; the LF integers grow by 2^extraprec so that the picture stays what it is
	const double bigshare = opt.getd("bigshare", 0.0);
	const int bigbits = opt.geti("bigbits", 0), flat = opt.geti("flat", 0), extra_prec = opt.geti("extraprec", 0);
	if (bigshare < 0 || bigshare > 1) die("vardct: bigshare is a probability");
	if (bigshare > 0 && (bigbits < 7 || bigbits > 30)) die("vardct: bigshare wants bigbits=7..30 (a magnitude below 2^bigbits packs into bigbits + 1 bits; the writer's tokens hold 32)");
	if (bigbits && bigshare <= 0) die("vardct: bigbits without bigshare changes nothing");
	if (flat && bigshare > 0) die("vardct: flat fixes every non-zero's value; it does not combine with bigshare");
	if (extra_prec < 0 || extra_prec > 3) die("vardct: extraprec is a 2-bit field (0..3)");
	if (opt.geti("forward", 0) && (bigshare > 0 || flat || opt.kv.count("hybrid"))) die("vardct: forward=1 takes its coefficients from the picture; bigshare / flat / hybrid belong to the synthetic statistics");
	if (global_scale < 1 || global_scale > 8193 + 65535) dief("vardct: global_scale=%d is outside its code U32(1+u(11), 2049+u(11), 4097+u(12), 8193+u(16)): 1..73728", global_scale);
	if (quant_lf < 1 || quant_lf > 65536) dief("vardct: quant_lf=%d is outside its code U32(16, 1+u(5), 1+u(8), 1+u(16)): 1..65536", quant_lf);
	HybridCfg forced_cfg; bool have_forced_cfg = false;
	if (opt.kv.count("hybrid")) {
		const std::string h = opt.gets("hybrid", "");
		if (sscanf(h.c_str(), "%d,%d,%d", &forced_cfg.split_exp, &forced_cfg.msb, &forced_cfg.lsb) != 3) die("vardct: hybrid=<split_exp>,<msb>,<lsb>");
		have_forced_cfg = true;
	}

	const int gcols = (W + 255) / 256, grows = (H + 255) / 256, num_groups = gcols * grows;
	const int ggcols = (W + 2047) / 2048, ggrows = (H + 2047) / 2048, num_lf_groups = ggcols * ggrows;
	const bool single_section = num_groups < 2 && num_passes == 1;
	if (single_section && !(ycbcr || opt.geti("noxyb", 0))) die("vardct: need at least 2 groups (single-section VarDCT order quirk, SURVEY section 0 fact 8)");
	if (single_section && opt.geti("alpha", 0)) die("vardct: a single-section frame carries its extra channels in LfGlobal, which is not generated: alpha=0");

	Picture pic(W, H, seed);

	// ---- forward opsin (ForwardOpsin, above) ----
	const ForwardOpsin opsin_fwd;
	const double (&fwd)[3][3] = opsin_fwd.fwd;
	const double bias = opsin_fwd.bias, cbias = opsin_fwd.cbias;
	auto to_xyb = [&](const float rgb[3], double xyb[3]) { opsin_fwd(rgb, xyb); };
	// LF dequant steps (j40.h:6562): m_lf_scaled / (global_scale * quant_lf) * 65536
	const double m_lf[3] = {1.0 / 4096, 1.0 / 512, 1.0 / 256};
	double lfstep[3]; for (int c = 0; c < 3; ++c) lfstep[c] = m_lf[c] / ((double) global_scale * quant_lf) * (double) (65536 >> extra_prec);

	// ---- forward=1: the picture's XYB samples (planes padded to whole cells, edges replicated) ----
	const int forward = opt.geti("forward", 0);
	if (forward && (num_passes > 1 || max_log > 6 || opt.geti("cfl", 0))) die("vardct: forward=1 takes one pass, transforms up to 64x64, default chroma-from-luma");
	if (nocfl && opt.geti("cfl", 0)) die("vardct: nocfl=1 and cfl=1 exclude each other");
	if (subsampled && (opt.geti("cfl", 0) || (opt.kv.count("dct8only") && !dct8only))) die("vardct: a subsampled stream has DCT8 blocks only and no chroma-from-luma");
	// the block grid in samples: padded to whole MCUs where channels are subsampled; plane c is pwc[c] x phc[c]
	const int PW = (W + (8 << sub_h) - 1) / (8 << sub_h) * (8 << sub_h), PH = (H + (8 << sub_v) - 1) / (8 << sub_v) * (8 << sub_v);
	const int pwc[3] = {PW >> hs[0], PW >> hs[1], PW >> hs[2]}, phc[3] = {PH >> vs[0], PH >> vs[1], PH >> vs[2]};
	std::vector<float> plane[3];
	std::unique_ptr<synthfwd::Forward> fwdx;
	// forward=1: the procedural picture of WC x HC pixels into three planes of OW x OH samples (edges replicated). A subsampled
	// stream evaluates it PER PLANE at the plane's own coordinates: sample (i, j) of plane c is pic(c, i, j) whatever the shift, so
	// the chroma planes of a 4:2:0 stream of 2W x 2H are those of a 4:4:4 stream of W x H.
	auto make_planes = [&](const int WC, const int HC, const int OW, const int OH, std::vector<float> out[3], const bool primary) {
		const int LW = (WC + 7) / 8 * 8, LH = (HC + 7) / 8 * 8;   // what the lattices are sized from: the picture's own size
		Picture fpic(WC, HC, seed);
		// 1/f detail: octaves of lattice noise from 256-pixel cells down to 2-pixel cells, amplitude falling with the cell size,
		// its strength modulated by a slowly varying mask (calm and busy regions, like sky and foliage)
		const double detail = opt.getd("detail", 2.4), beta = opt.getd("beta", 0.35);
		struct Lattice { int cell, w, h; float amp; std::vector<float> v; };
		std::vector<Lattice> lat;
		SplitMix64 lr(seed ^ 0xD37A11ull);
		for (int cell = 256; cell >= 2; cell /= 2) {
			Lattice l; l.cell = cell; l.w = LW / cell + 2; l.h = LH / cell + 2; l.amp = (float) (0.2 * detail * pow((double) cell / 256.0, beta));
			l.v.resize((size_t) l.w * (size_t) l.h);
			for (auto &v : l.v) v = (float) lr.unit() - 0.5f;
			lat.push_back(std::move(l));
		}
		Lattice mask; mask.cell = 512; mask.w = LW / 512 + 2; mask.h = LH / 512 + 2; mask.amp = 1.0f; mask.v.resize((size_t) mask.w * (size_t) mask.h);
		for (auto &v : mask.v) { const double u = lr.unit(); v = (float) (0.12 + 1.5 * u * u); }
		auto sample = [](const Lattice &l, int x, int y) {
			const float u = (float) x / (float) l.cell, v = (float) y / (float) l.cell;
			const int iu = (int) u, iv = (int) v; const float fu = u - (float) iu, fv = v - (float) iv;
			const float *p = l.v.data() + (size_t) iv * (size_t) l.w + (size_t) iu;
			return (p[0] * (1 - fu) + p[1] * fu) * (1 - fv) + (p[l.w] * (1 - fu) + p[l.w + 1] * fu) * fv;
		};
		for (int c = 0; c < 3; ++c) out[c].resize((size_t) OW * (size_t) OH);
		const std::string dumpsrc = primary ? opt.gets("dumpsrc", "") : std::string();   // the source picture as sRGB u8 x 3, for the fidelity test
		std::vector<uint8_t> srcdump(dumpsrc.empty() ? 0 : (size_t) WC * (size_t) HC * 3);
		static const float CHROMA[3] = {1.0f, 0.92f, 0.8f};
		// the smooth part of the picture on a grid of 4-pixel cells (it has no feature below ~100 pixels), sRGB -> linear by table
		const int GW = LW / 4 + 2, GH = LH / 4 + 2;
		std::vector<float> coarse((size_t) GW * (size_t) GH * 3);
		for (int gy = 0; gy < GH; ++gy) for (int gx = 0; gx < GW; ++gx) fpic.smooth((float) (gx * 4), (float) (gy * 4), &coarse[((size_t) gy * (size_t) GW + (size_t) gx) * 3]);
		std::vector<float> to_linear(4097);
		for (int i = 0; i <= 4096; ++i) { const double v = i / 4096.0; to_linear[(size_t) i] = (float) (v <= 0.04045 ? v / 12.92 : pow((v + 0.055) / 1.055, 2.4)); }
		for (int y = 0; y < OH; ++y) for (int x = 0; x < OW; ++x) {
			const int sx = std::min(x, WC - 1), sy = std::min(y, HC - 1);
			float rgb[3]; double xyb[3];
			{
				const int gx = sx >> 2, gy = sy >> 2; const float fu = (float) (sx & 3) * 0.25f, fv = (float) (sy & 3) * 0.25f;
				const float *p = &coarse[((size_t) gy * (size_t) GW + (size_t) gx) * 3];
				for (int c = 0; c < 3; ++c) rgb[c] = (p[c] * (1 - fu) + p[3 + c] * fu) * (1 - fv) + (p[(size_t) GW * 3 + c] * (1 - fu) + p[(size_t) GW * 3 + 3 + c] * fu) * fv;
				fpic.add_rects((float) sx, (float) sy, rgb);
			}
			float n = 0;
			for (const Lattice &l : lat) n += l.amp * sample(l, sx, sy);
			n *= sample(mask, sx, sy);
			for (int c = 0; c < 3; ++c) rgb[c] = std::min(0.97f, std::max(0.03f, rgb[c] + n * CHROMA[c]));
			if (!dumpsrc.empty() && x < WC && y < HC) for (int c = 0; c < 3; ++c) srcdump[((size_t) y * (size_t) WC + (size_t) x) * 3 + (size_t) c] = (uint8_t) lrintf(rgb[c] * 255.0f);
			{   // to_xyb with the table for the transfer function (quantise the sample to the table's grid first: what is
				// dumped as the source is an 8-bit picture anyway)
				double lin[3], mix[3];
				for (int c = 0; c < 3; ++c) { const float t = rgb[c] * 4096.0f; const int i = (int) t; const float f = t - (float) i; lin[c] = to_linear[(size_t) i] * (1 - f) + to_linear[(size_t) std::min(i + 1, 4096)] * f; }
				for (int c = 0; c < 3; ++c) mix[c] = cbrt(fwd[c][0] * lin[0] + fwd[c][1] * lin[1] + fwd[c][2] * lin[2] - bias) + cbias;
				xyb[0] = (mix[0] - mix[1]) * 0.5; xyb[1] = (mix[0] + mix[1]) * 0.5; xyb[2] = mix[2];
			}
			for (int c = 0; c < 3; ++c) out[c][(size_t) y * (size_t) OW + (size_t) x] = (float) xyb[c];
		}
		if (!dumpsrc.empty()) { FILE *fp = fopen(dumpsrc.c_str(), "wb"); if (!fp || fwrite(srcdump.data(), 1, srcdump.size(), fp) != srcdump.size()) die("cannot write dumpsrc"); fclose(fp); }
	};
	if (forward) {
		fwdx.reset(new synthfwd::Forward());
		if (g_lf && !g_lf->pic[0].empty()) {   // an LF frame of a picture: its samples are the next finer frame's cell means (edges replicated)
			for (int c = 0; c < 3; ++c) {
				plane[c].resize((size_t) PW * (size_t) PH);
				for (int y = 0; y < PH; ++y) for (int x = 0; x < PW; ++x) plane[c][(size_t) y * (size_t) PW + (size_t) x] = g_lf->pic[c][(size_t) std::min(y, H - 1) * (size_t) W + (size_t) std::min(x, W - 1)];
			}
		} else
		if (!subsampled) make_planes(W, H, PW, PH, plane, true);
		else {
			std::vector<float> tmp[3];
			make_planes(W, H, PW, PH, tmp, true); plane[1].swap(tmp[1]);
			make_planes((W + (1 << sub_h) - 1) >> sub_h, (H + (1 << sub_v) - 1) >> sub_v, pwc[0], phc[0], tmp, false); plane[0].swap(tmp[0]); plane[2].swap(tmp[2]);
		}
		if (flatchroma) { for (auto &v : plane[0]) v = 0.0625f; for (auto &v : plane[2]) v = -0.046875f; }
	}
	// activity of a cell: variance of its Y samples
	std::vector<float> activity(forward ? (size_t) (PW / 8) * (size_t) (PH / 8) : 0);
	for (int cy = 0; forward && cy < PH / 8; ++cy) for (int cx = 0; cx < PW / 8; ++cx) {
		double s = 0, s2 = 0;
		for (int y = 0; y < 8; ++y) for (int x = 0; x < 8; ++x) { const double v = plane[1][(size_t) (cy * 8 + y) * (size_t) PW + (size_t) (cx * 8 + x)]; s += v; s2 += v * v; }
		activity[(size_t) cy * (size_t) (PW / 8) + (size_t) cx] = (float) std::max(0.0, s2 / 64 - (s / 64) * (s / 64));
	}
	auto cell_activity = [&](int cx, int cy) { return (double) activity[(size_t) cy * (size_t) (PW / 8) + (size_t) cx]; };

	const int custom_cfl = opt.geti("cfl", 0);
	// (nocfl=1 codes an all-zero correlation; a subsampled frame's decoder applies none whatever the header says)
	const double kx_lf = custom_cfl ? 0.125 + 3.0 / 128.0 : 0.0, kb_lf = custom_cfl ? 0.75 - 2.0 / 128.0 : (nocfl || subsampled) ? 0.0 : 1.0;

	if (g_lf && g_lf->capture) {
		if (!forward || subsampled) die("vardct: an LF frame of a picture wants forward=1 and no subsampling");
		g_lf->means_w = PW / 8; g_lf->means_h = PH / 8;
		for (int c = 0; c < 3; ++c) g_lf->means[c].assign((size_t) (PW / 8) * (size_t) (PH / 8), 0.0f);
		for (int cy = 0; cy < PH / 8; ++cy) for (int cx = 0; cx < PW / 8; ++cx) {
			double m[3] = {0, 0, 0};
			for (int c = 0; c < 3; ++c) { for (int y = 0; y < 8; ++y) for (int x = 0; x < 8; ++x) m[c] += plane[c][(size_t) (cy * 8 + y) * (size_t) PW + (size_t) (cx * 8 + x)]; m[c] /= 64; }
			m[0] -= kx_lf * m[1]; m[2] -= kb_lf * m[1];   // (the frame's decoder adds these to the LF it is given, j40.h:7115-7116)
			for (int c = 0; c < 3; ++c) g_lf->means[c][(size_t) cy * (size_t) (PW / 8) + (size_t) cx] = (float) m[c];
		}
	}

	// ---- block context configuration ----
	int nb_lf_thr[3] = {0, 0, 0}, lf_thr[3][4] = {{0}}, nb_qf_thr = 0, qf_thr[4] = {0};
	std::vector<uint8_t> bctx_map;
	int nb_block_ctx = 15;
	static const uint8_t DEFAULT_BLKCTX[39] = {0, 1, 2, 2, 3, 3, 4, 5, 6, 6, 6, 6, 6, 7, 8, 9, 9, 10, 11, 12, 13, 14, 14, 14, 14, 14, 7, 8, 9, 9, 10, 11, 12, 13, 14, 14, 14, 14, 14};
	if (!custom_bctx) bctx_map.assign(DEFAULT_BLKCTX, DEFAULT_BLKCTX + 39);
	else {
		nb_lf_thr[0] = 1; lf_thr[0][0] = 3;                // X
		nb_lf_thr[1] = 2; lf_thr[1][0] = 60; lf_thr[1][1] = 140;  // Y
		nb_lf_thr[2] = 1; lf_thr[2][0] = 50;               // B
		nb_qf_thr = 2; qf_thr[0] = 4; qf_thr[1] = 9;
		int size = 39 * 2 * 3 * 2 * 3;
		nb_block_ctx = 11;
		bctx_map.resize((size_t) size);
		for (int i = 0; i < size; ++i) bctx_map[(size_t) i] = (uint8_t) ((i * 7 + i / 13) % nb_block_ctx);
		for (int i = 0; i < nb_block_ctx; ++i) bctx_map[(size_t) i] = (uint8_t) i;  // every cluster id present
	}
	const int lfidx_size = (nb_lf_thr[0] + 1) * (nb_lf_thr[1] + 1) * (nb_lf_thr[2] + 1);

	// ---- per LF group: LF image, varblock layout, HF metadata ----
	std::vector<LfGroupW> ggs((size_t) num_lf_groups);
	std::vector<int> forced;  // transform types still to be placed once (coverage)
	if (coverage && !dct8only) for (int t = 0; t < 27; ++t) if (std::max(DCTSEL[t][0], DCTSEL[t][1]) <= max_log) forced.push_back(t);
	// weights of the random mix (8x8-class transforms dominate, like a d1 encode)
	const int mixw[27] = {40, 3, 2, 3, 14, 6, 6, 6, 2, 2, 3, 3, 3, 3, 1, 1, 1, 1, 2, 1, 1, 1, 1, 1, 1, 1, 1};
	for (int ggy = 0, ggi = 0; ggy < ggrows; ++ggy) for (int ggx = 0; ggx < ggcols; ++ggx, ++ggi) {
		LfGroupW &gg = ggs[(size_t) ggi];
		gg.left = ggx * 2048; gg.top = ggy * 2048; gg.w = std::min(2048, W - gg.left); gg.h = std::min(2048, H - gg.top);
		gg.w8 = (gg.w + 7) / 8; gg.h8 = (gg.h + 7) / 8; gg.w64 = (gg.w + 63) / 64; gg.h64 = (gg.h + 63) / 64;
		if (subsampled) { gg.w8 = std::min(256, PW / 8 - gg.left / 8); gg.h8 = std::min(256, PH / 8 - gg.top / 8); gg.w64 = (gg.w8 + 7) / 8; gg.h64 = (gg.h8 + 7) / 8; }
		static const int SLOT_OF_STREAM[3] = {1, 0, 2};
		for (int c = 0; c < 3; ++c) gg.lfq[c] = Channel(gg.w8 >> hs[SLOT_OF_STREAM[c]], gg.h8 >> vs[SLOT_OF_STREAM[c]]);
		if (jpeg) {
			// the DC integers, scaled so that the LF rule gives d * Q_00 / (8 * 255): mult_lf = (1/4096, 1/512, 1/256) * 65536 / (2048 * 255)
			for (int k = 0; k < 3; ++k) {
				const int c = SLOT_OF_STREAM[k];
				const JpegDump::Comp &jc = jd.slot(c);
				for (int y = 0; y < gg.lfq[k].h; ++y) for (int x = 0; x < gg.lfq[k].w; ++x) {
					const int bx = (gg.left >> 3 >> hs[c]) + x, by = (gg.top >> 3 >> vs[c]) + y;
					if (bx >= jc.bx || by >= jc.by) die("vardct: jpegdata=: the LF image reaches beyond the component's block grid");
					const int64_t v = (int64_t) jc.coef[((size_t) by * (size_t) jc.bx + (size_t) bx) * 64] * jc.table[0] * JPEG_LF_K[c];
					if (v < -32767 || v > 32767) die("vardct: jpegdata=: a DC value leaves the LfGroup's 16-bit channels");
					gg.lfq[k].at(x, y) = (int32_t) v;
				}
			}
		} else if (subsampled) {
			// every channel's LF image at its own size: the cell's mean (forward=1) or the picture at the cell's centre, in the plane's own coordinates
			for (int k = 0; k < 3; ++k) {
				const int c = SLOT_OF_STREAM[k], cw = gg.w8 >> hs[c], chh = gg.h8 >> vs[c], left = gg.left >> hs[c], top = gg.top >> vs[c];
				for (int y = 0; y < chh; ++y) for (int x = 0; x < cw; ++x) {
					double v;
					if (forward) { double m = 0; for (int j = 0; j < 8; ++j) for (int i = 0; i < 8; ++i) m += plane[c][(size_t) (top + y * 8 + j) * (size_t) pwc[c] + (size_t) (left + x * 8 + i)]; v = m / 64; }
					else { float rgb[3]; double xyb[3]; pic.rgb((float) (left + x * 8) + 3.5f, (float) (top + y * 8) + 3.5f, rgb); to_xyb(rgb, xyb); v = flatchroma && c != 1 ? (c == 0 ? 0.0625 : -0.046875) : xyb[c]; }
					gg.lfq[k].at(x, y) = (int32_t) lrint(v / lfstep[c]);
					if (abs(gg.lfq[k].at(x, y)) > 32767) die("vardct: an LF integer leaves the LfGroup's 16-bit channels");
				}
			}
		} else
		for (int y = 0; y < gg.h8; ++y) for (int x = 0; x < gg.w8; ++x) {
			float rgb[3]; double xyb[3];
			if (g_lf && g_lf->replicate) {   // the LF frame's integers, each over 8 x 8 cells
				const int sx = (gg.left / 8 + x) / 8, sy = (gg.top / 8 + y) / 8;
				for (int k = 0; k < 3; ++k) gg.lfq[k].at(x, y) = g_lf->src[k][(size_t) sy * (size_t) g_lf->src_w + (size_t) sx];
				continue;
			}
			if (forward) {   // the cell's mean
				for (int c = 0; c < 3; ++c) { double m = 0; for (int j = 0; j < 8; ++j) for (int i = 0; i < 8; ++i) m += plane[c][(size_t) (gg.top + y * 8 + j) * (size_t) PW + (size_t) (gg.left + x * 8 + i)]; xyb[c] = m / 64; }
			} else {
				pic.rgb((float) (gg.left + x * 8) + 3.5f, (float) (gg.top + y * 8) + 3.5f, rgb);
				to_xyb(rgb, xyb);
				if (flatchroma) { xyb[0] = 0.0625; xyb[2] = -0.046875; }
			}
			gg.lfq[0].at(x, y) = (int32_t) lrint(xyb[1] / lfstep[1]);  // streamed order: Y, X, B
			gg.lfq[1].at(x, y) = (int32_t) lrint(xyb[0] / lfstep[0]);
			// the decoder adds kb_lf * Y to the LF of B and kx_lf * Y to X (j40.h:7115-7116, 7159-7171)
			double yq = (double) gg.lfq[0].at(x, y) * lfstep[1];
			gg.lfq[1].at(x, y) = (int32_t) lrint((xyb[0] - kx_lf * yq) / lfstep[0]);
			gg.lfq[2].at(x, y) = (int32_t) lrint((xyb[2] - kb_lf * yq) / lfstep[2]);
			for (int c = 0; c < 3; ++c) if (abs(gg.lfq[c].at(x, y)) > 32767)
				dief("vardct: global_scale=%d quant_lf=%d extraprec=%d make the LF step so fine (%.3g) that an LF integer reaches %d; the LfGroup's channels are "
				     "16-bit here, keep global_scale * quant_lf << extraprec below about 3.5 million (times the picture's brightest Y)", global_scale, quant_lf, extra_prec, lfstep[c == 0 ? 1 : c == 1 ? 0 : 2], gg.lfq[c].at(x, y));
		}
		gg.lfidx.assign((size_t) gg.w8 * (size_t) gg.h8, 0);
		for (int y = 0; y < gg.h8; ++y) for (int x = 0; x < gg.w8; ++x) {  // j40.h:6566-6570
			auto cnt = [&](int v, const int *thr, int n) { int k = 0; for (int t = 0; t < n; ++t) k += v > thr[t]; return k; };
			// (a subsampled channel: the cell looks at the channel's sample that covers it)
			int xi = cnt(gg.lfq[1].at(x >> hs[0], y >> vs[0]), lf_thr[0], nb_lf_thr[0]), yi = cnt(gg.lfq[0].at(x, y), lf_thr[1], nb_lf_thr[1]), bi = cnt(gg.lfq[2].at(x >> hs[2], y >> vs[2]), lf_thr[2], nb_lf_thr[2]);
			gg.lfidx[(size_t) y * (size_t) gg.w8 + (size_t) x] = (uint8_t) ((xi * (nb_lf_thr[0] + 1) + bi) * (nb_lf_thr[2] + 1) + yi);
		}
		gg.blocks.assign((size_t) gg.w8 * (size_t) gg.h8, 0);
		for (int y0 = 0; y0 < gg.h8; ++y0) for (int x0 = 0; x0 < gg.w8; ++x0) {
			if (gg.blocks[(size_t) y0 * (size_t) gg.w8 + (size_t) x0]) continue;
			auto fits = [&](int t) {
				int vw8 = 1 << (DCTSEL[t][1] - 3), vh8 = 1 << (DCTSEL[t][0] - 3);
				int x1 = x0 + vw8 - 1, y1 = y0 + vh8 - 1;
				if (x1 >= gg.w8 || y1 >= gg.h8 || (x0 >> 5) != (x1 >> 5) || (y0 >> 5) != (y1 >> 5)) return false;  // j40.h:6659-6660
				for (int y = y0; y <= y1; ++y) for (int x = x0; x <= x1; ++x) if (gg.blocks[(size_t) y * (size_t) gg.w8 + (size_t) x]) return false;
				return true;
			};
			int t = -1;
			for (size_t k = 0; k < forced.size(); ++k) if (fits(forced[k])) { t = forced[k]; forced.erase(forced.begin() + (long) k); break; }
			if (t < 0) {
				int total = 0; for (int k = 0; k < 27; ++k) if (std::max(DCTSEL[k][0], DCTSEL[k][1]) <= max_log) total += mixw[k];
				int pick = (int) rng.below((uint32_t) total);
				for (int k = 0; k < 27; ++k) if (std::max(DCTSEL[k][0], DCTSEL[k][1]) <= max_log) { if (pick < mixw[k]) { t = k; break; } pick -= mixw[k]; }
				if (!fits(t)) t = 0;
			}
			if (dct8only) t = 0;
			if (opt.geti("subdct16", 0) && x0 == 0 && y0 == 0 && ggi == 0 && fits(4)) t = 4;   // (a stream the decoder has to refuse: a DCT16 block in a subsampled frame)
			int hfmul_m1 = 3 + (int) rng.below(10);
			if (forward) {
				// what an encoder's heuristics amount to: large transforms only over calm content, the 8x8 specials only where there
				// is something to localise, finer quantisation (larger HfMul) where errors show (calm areas)
				auto worst = [&](int tt) { double a = 0; for (int y = y0; y < y0 + (1 << (DCTSEL[tt][0] - 3)); ++y) for (int x = x0; x < x0 + (1 << (DCTSEL[tt][1] - 3)); ++x) a = std::max(a, cell_activity(gg.left / 8 + x, gg.top / 8 + y)); return a; };
				if (std::max(DCTSEL[t][0], DCTSEL[t][1]) > 3 && worst(t) > 4e-5 * (double) (1 << (12 - DCTSEL[t][0] - DCTSEL[t][1])) ) t = 0;
				if (DCTSEL[t][0] == 3 && DCTSEL[t][1] == 3) {
					const double a = worst(t);
					if (a < 2e-5) t = 0;
					else if (!dct8only && t == 0 && a > 4e-4 && rng.below(3) == 0) { static const int SP[9] = {1, 2, 3, 12, 13, 14, 15, 16, 17}; t = SP[rng.below(9)]; }
				}
				const double a = worst(t);
				hfmul_m1 = (a < 1e-5 ? 8 : a < 1e-4 ? 7 : a < 1e-3 ? 6 : 5) - 1;
			}
			if (fixed_hfmul) hfmul_m1 = fixed_hfmul - 1;
			int vw8 = 1 << (DCTSEL[t][1] - 3), vh8 = 1 << (DCTSEL[t][0] - 3), voff = (int) gg.vbs.size();
			for (int y = y0; y < y0 + vh8; ++y) for (int x = x0; x < x0 + vw8; ++x) gg.blocks[(size_t) y * (size_t) gg.w8 + (size_t) x] = 1 << 20 | voff;
			gg.blocks[(size_t) y0 * (size_t) gg.w8 + (size_t) x0] = (t + 2) << 20 | voff;
			gg.vbs.push_back({x0, y0, t, hfmul_m1});
		}
		gg.xfromy = Channel(gg.w64, gg.h64); gg.bfromy = Channel(gg.w64, gg.h64);
		for (auto &v : gg.xfromy.px) v = forward || subsampled || nocfl ? 0 : (int32_t) rng.below(9) - 4;
		for (auto &v : gg.bfromy.px) v = forward || subsampled || nocfl ? 0 : (int32_t) rng.below(13) - 6;
		gg.blockinfo = Channel((int) gg.vbs.size(), 2);
		for (size_t i = 0; i < gg.vbs.size(); ++i) { gg.blockinfo.at((int) i, 0) = gg.vbs[i].dctsel; gg.blockinfo.at((int) i, 1) = gg.vbs[i].hfmul_m1; }
		gg.sharp = Channel(gg.w8, gg.h8);
		for (auto &v : gg.sharp.px) v = (int32_t) rng.below(8);
	}

	if (g_lf) {
		if (subsampled || jpeg) die("vardct: LF frames are not written for YCbCr streams");
		const int fw8 = (W + 7) / 8, fh8 = (H + 7) / 8;
		bool seen[256] = {false};
		g_lf->out_w = fw8;
		for (int k = 0; k < 3; ++k) g_lf->out[k].assign((size_t) fw8 * (size_t) fh8, 0);
		for (const LfGroupW &gg : ggs) for (int y = 0; y < gg.h8; ++y) for (int x = 0; x < gg.w8; ++x) {
			for (int k = 0; k < 3; ++k) g_lf->out[k][(size_t) (gg.top / 8 + y) * (size_t) fw8 + (size_t) (gg.left / 8 + x)] = gg.lfq[k].px[(size_t) y * (size_t) gg.w8 + (size_t) x];
			seen[gg.lfidx[(size_t) y * (size_t) gg.w8 + (size_t) x]] = true;
		}
		g_lf->lfidx_distinct = 0;
		for (bool s : seen) g_lf->lfidx_distinct += s;
	}

	// ---- global MA tree: splits on stream index (property 1) and channel (property 0) ----
	MATree tree;
	// wp= (with lftree=4, the tree that uses the weighted predictor): parameters other than the defaults in the Modular headers this
	// writer emits -- wpat=global: the global header alone (it exists with alpha=1 and decodes nothing: whoever takes ITS values for a
	// sub-image is wrong), group (default): every sub-image header (LfGroup's two, the raw dequantisation matrices, the alpha
	// sub-images) the same values, both: the global header and values of its own in every sub-image header
	WPParams wp_base;
	const bool custom_wp = parse_wp(opt, seed, wp_base, "vardct");
	const std::string wpat = opt.gets("wpat", "group");
	if (custom_wp && opt.geti("lftree", 0) != 4) die("vardct: wp= changes nothing unless the tree uses the weighted predictor: lftree=4");
	if (!custom_wp && opt.kv.count("wpat")) die("vardct: wpat places the parameters wp= gives");
	if (custom_wp && wpat != "global" && wpat != "group" && wpat != "both") die("vardct: wpat=global|group|both");
	if (custom_wp && wpat != "group" && !opt.geti("alpha", 0)) die("vardct: the global Modular header exists with extra channels only: wpat=global|both want alpha=1");
	std::map<int, WPParams> wp_store;   // header id -> its parameters: LfGroup gg 2 gg (LF image) and 2 gg + 1 (metadata), raw matrix idx 100 + idx, alpha of group g 200 + g
	const std::function<const WPParams *(int)> wp_of = [&](int k) -> const WPParams * {
		if (!custom_wp || wpat == "global") return nullptr;
		if (!wp_store.count(k)) wp_store[k] = wpat == "both" ? wp_derived(wp_base, k) : wp_base;
		return &wp_store[k];
	};
	const WPParams wp_default;
	auto wp_in = [&](int k) -> const WPParams & { const WPParams *p = wp_of(k); return p ? *p : wp_default; };
	if (opt.geti("lftree", 0) == 4) {
		// lftree=4: the weighted predictor and its error property on every channel of every sub-image
		int a = tree.branch(15, 4, tree.leaf(6), tree.leaf(6, 1)), b = tree.branch(15, -4, tree.leaf(5), tree.leaf(6));
		tree.finalise(tree.branch(0, 0, a, b));
	} else if (opt.geti("lftree", 0) == 2) {
		// lftree=2: every LfGroup channel under ONE test of a sample property over two leaves that predict alike (what libjxl's fixed LF
		// trees look like, with other properties and predictors), offsets and multipliers on some
		auto pair = [&](int prop, int thr, int pred, int off = 0, int mshift = 0, int mbits = 0) { int a = tree.leaf(pred, off, mshift, mbits), b = tree.leaf(pred, off, mshift, mbits); return tree.branch(prop, thr, a, b); };
		int lf_y = pair(9, 100, 5), lf_x = pair(8, 0, 4), lf_b = pair(5, 2, 3, 1);
		int lf_xb = tree.branch(0, 1, lf_b, lf_x);
		int lf = tree.branch(0, 0, lf_xb, lf_y);
		int cfl = pair(2, 3, 1), binfo = pair(3, 300, 9, 0, 0, 0), sharp = pair(12, 0, 12, -1);
		int meta_hi = tree.branch(0, 2, sharp, binfo);
		int meta = tree.branch(0, 1, meta_hi, cfl);
		int root = tree.branch(1, 2 * num_lf_groups, meta, lf);
		tree.finalise(root);
	} else if (opt.geti("lftree", 0) == 3) {
		// lftree=3: as 2 with the other testable properties and predictors
		auto pair = [&](int prop, int thr, int pred, int off = 0, int mshift = 0, int mbits = 0) { int a = tree.leaf(pred, off, mshift, mbits), b = tree.leaf(pred, off, mshift, mbits); return tree.branch(prop, thr, a, b); };
		int lf_y = pair(10, 0, 10), lf_x = pair(11, 1, 11), lf_b = pair(14, -1, 8);
		int lf_xb = tree.branch(0, 1, lf_b, lf_x);
		int lf = tree.branch(0, 0, lf_xb, lf_y);
		int cfl = pair(7, 0, 2), binfo = pair(14, 2, 1, 0, 0, 0), sharp = pair(4, 3, 7, 0, 1, 1);
		int meta_hi = tree.branch(0, 2, sharp, binfo);
		int meta = tree.branch(0, 1, meta_hi, cfl);
		int root = tree.branch(1, 2 * num_lf_groups, meta, lf);
		tree.finalise(root);
	} else if (opt.geti("lftree", 0)) {
		// lftree=1: below the stream / channel splits every LfGroup channel gets a subtree of its own over the sample properties, with
		// predictors that look at NE, NEE, NN, NWW -- also the varblock-info channel, whose second row is thousands of samples wide
		int y0 = tree.leaf(13), y1 = tree.leaf(5), y2 = tree.leaf(7), y3 = tree.leaf(12, 1);
		int ya = tree.branch(12, 2, y0, y1), yb = tree.branch(13, 0, y2, y3);   // N - NE, N - NN
		int lf_ysplit = tree.branch(9, 120, ya, yb);                             // W + N - NW
		int lf_x = tree.branch(8, 0, tree.leaf(9), tree.leaf(10));               // W - (WW + NW - NWW)
		int lf_b = tree.branch(14, 1, tree.leaf(11, -1), tree.branch(4, 3, tree.leaf(3), tree.leaf(4)));   // W - WW, |N|
		int lf_xb = tree.branch(0, 1, lf_b, lf_x);
		int lf = tree.branch(0, 0, lf_xb, lf_ysplit);
		int cfl = tree.branch(5, 2, tree.leaf(1), tree.leaf(8));                 // |W|
		int binfo = tree.branch(6, 3, tree.leaf(5), tree.branch(3, 300, tree.leaf(2), tree.branch(2, 0, tree.leaf(13), tree.leaf(0))));   // N, x, y
		int sharp = tree.branch(2, 5, tree.branch(11, 0, tree.leaf(4), tree.leaf(12)), tree.branch(7, 3, tree.leaf(2), tree.leaf(10)));   // y, NW - N, W
		int meta_hi = tree.branch(0, 2, sharp, binfo);
		int meta = tree.branch(0, 1, meta_hi, cfl);
		int root = tree.branch(1, 2 * num_lf_groups, meta, lf);
		tree.finalise(root);
	} else {
		int lf_y = tree.leaf(5), lf_x = tree.leaf(5), lf_b = tree.leaf(4);
		int lf_yhi = tree.leaf(5);
		int lf_ysplit = tree.branch(9, 120, lf_yhi, lf_y);          // W+N-NW > 120
		int lf_xb = tree.branch(0, 1, lf_b, lf_x);
		int lf = tree.branch(0, 0, lf_xb, lf_ysplit);               // channel > 0 ?
		int cfl = tree.leaf(1), binfo = tree.leaf(0), sharp = tree.leaf(2);
		int meta_hi = tree.branch(0, 2, sharp, binfo);
		int meta = tree.branch(0, 1, meta_hi, cfl);
		int root = tree.branch(1, 2 * num_lf_groups, meta, lf);     // sidx > 2*num_lf_groups  <=> HF metadata stream
		tree.finalise(root);
	}
	CodeSpecW treespec; treespec.init(6, std::vector<uint8_t>(6, 0), 1); treespec.log_alpha = 6; treespec.cfg[0] = HybridCfg{4, 1, 0};
	StreamEncoder tree_enc(treespec); tree_tokens(tree, tree_enc); count_stream(treespec, tree_enc);

	CodeSpecW gspec;  // global code spec shared by every LF-group Modular stream
	{
		// gprefix=1: the global code is a prefix code; glz77=1: it has LZ77 enabled (the distance context in a cluster of its own), and
		// the extra channels' sub-images (alpha=1) use it: runs of equal small tokens become copies of the previous symbol
		const int glz77 = opt.geti("glz77", 0);
		std::vector<uint8_t> map((size_t) (tree.num_ctx + (glz77 ? 1 : 0)));
		for (size_t i = 0; i < map.size(); ++i) map[i] = (uint8_t) i;
		gspec.lz77 = glz77 != 0;
		gspec.init(tree.num_ctx, map, (int) map.size());
		gspec.log_alpha = 8;
		gspec.use_prefix = opt.geti("gprefix", 0) != 0;
		for (auto &c : gspec.cfg) c = HybridCfg{4, 2, 0};
	}
	std::vector<StreamEncoder> lfq_enc, meta_enc;
	for (int ggi = 0; ggi < num_lf_groups; ++ggi) {
		LfGroupW &gg = ggs[(size_t) ggi];
		lfq_enc.emplace_back(gspec); meta_enc.emplace_back(gspec);
		std::vector<Channel> ch{gg.lfq[0], gg.lfq[1], gg.lfq[2]};
		for (int c = 0; c < 3; ++c) encode_channel(tree, ch, c, 1 + ggi, wp_in(2 * ggi), lfq_enc.back());
		std::vector<Channel> mc{gg.xfromy, gg.bfromy, gg.blockinfo, gg.sharp};
		for (int c = 0; c < 4; ++c) encode_channel(tree, mc, c, 1 + 2 * num_lf_groups + ggi, wp_in(2 * ggi + 1), meta_enc.back());
		count_stream(gspec, lfq_enc.back()); count_stream(gspec, meta_enc.back());
	}

	// dq=2: two of the larger matrices in raw form (DCT32x32 and DCT8x16), coded with the global tree and code spec
	std::vector<std::pair<int, StreamEncoder>> dq_raw;
	if (opt.geti("dq", 0) >= 2) for (int idx : {5, 6}) {
		const int ncols = idx == 5 ? 32 : 16, nrows = idx == 5 ? 32 : 8;
		std::vector<Channel> mc;
		for (int c = 0; c < 3; ++c) { Channel m(ncols, nrows); for (int y = 0; y < nrows; ++y) for (int x = 0; x < ncols; ++x) m.at(x, y) = 300 + 90 * (x + y) * (c + 1) + 17 * ((x * 5 + y * 3 + c) & 7); mc.push_back(m); }
		dq_raw.emplace_back(idx, StreamEncoder(gspec));
		for (int c = 0; c < 3; ++c) encode_channel(tree, mc, c, 1 + 3 * num_lf_groups + idx, wp_in(100 + idx), dq_raw.back().second);
		count_stream(gspec, dq_raw.back().second);
	}

	if (jpeg) {   // DCT8's matrix from the file's tables: entry (x, y) of channel c weighs canonical index 8 y + x = 8 * horizontal + vertical frequency
		std::vector<Channel> mc;
		for (int c = 0; c < 3; ++c) { Channel m(8, 8); for (int u = 0; u < 8; ++u) for (int v = 0; v < 8; ++v) { const int q = jd.slot(c).table[v * 8 + u]; m.at(v, u) = JPEG_L / jpeg_gcd(q, JPEG_L); } mc.push_back(m); }
		dq_raw.emplace_back(0, StreamEncoder(gspec));
		for (int c = 0; c < 3; ++c) encode_channel(tree, mc, c, 1 + 3 * num_lf_groups + 0, wp_in(100), dq_raw.back().second);
		count_stream(gspec, dq_raw.back().second);
	}

	// ---- optional alpha extra channel: a Modular sub-image per pass group, coded after the group's HF coefficients
	//      (j40.h:7024-7034) with the global tree and code spec ----
	const int with_alpha = opt.geti("alpha", 0);
	// With alpha=1: extra=N puts N depth channels ahead of the alpha channel (coded in the same sub-images, so that alpha is not
	// extra channel 0); bpp=9..15 codes alpha at the image's depth, its samples over the whole range; alphabpp= gives alpha a depth
	// of its own and alphaassoc=1 flags it associated (two things the reference's render answers with "TODO" in a Modular frame).
	const int ec_extra = with_alpha ? opt.geti("extra", 0) : 0;
	const int ec_bpp = opt.geti("bpp", 8), alpha_bpp = opt.geti("alphabpp", ec_bpp), alpha_assoc = opt.geti("alphaassoc", 0);
	const int num_ec = with_alpha ? ec_extra + 1 : 0;
	if (with_alpha && num_passes > 1) die("vardct: alpha with several passes is not generated");
	if (ec_extra < 0 || ec_extra > 3) die("vardct: extra=0..3 (four extra channels with alpha, j40.h:3171)");
	if (with_alpha && (alpha_bpp < 8 || alpha_bpp > 15)) die("vardct: alphabpp=8..15 (16-bit buffers)");
	if (!with_alpha && (opt.kv.count("alphabpp") || alpha_assoc)) die("vardct: alphabpp= and alphaassoc= want alpha=1");
	std::vector<StreamEncoder> alpha_enc;
	if (with_alpha) {
		Channel alpha(W, H);
		const int amax = (1 << alpha_bpp) - 1, emax = (1 << ec_bpp) - 1;
		for (int y = 0; y < H; ++y) for (int x = 0; x < W; ++x) {
			int v = (x * 3 + y * 2) / 4 + (int) rng.below(5) - 2 + (((x / 40) + (y / 24)) % 3 == 0 ? 90 : 0);
			v = std::max(0, std::min(255, v));
			if (alpha_bpp != 8) v = std::min(amax, v * amax / 255 + ((x * 7 + y * 13) & ((1 << (alpha_bpp - 8)) - 1)));
			// alpharange=1: 0, full scale and everything between (transparent and opaque cells in a diagonal ramp), for the blend modes
			if (opt.geti("alpharange", 0)) { const int cell = (x / 23 + y / 19) % 5; v = cell == 0 ? 0 : cell == 1 ? amax : ((x * 5 + y * 3) & 255) * amax / 255; }
			alpha.at(x, y) = v;
		}
		for (int g = 0; g < num_groups; ++g) {
			const int gx = (g % gcols) * 256, gy = (g / gcols) * 256, gw = std::min(256, W - gx), gh = std::min(256, H - gy);
			// (ecup= above the frame's upsampling: the extra channels are coded 1 << es times coarser than the frame, ceil(shown / ecup)
			// samples an axis, and a group holds the rectangle of its own shifted down by es)
			const int eff_k = up_flag() ? g_up.k : 1, eff_w = up_flag() ? g_up.shown_w : W, eff_h = up_flag() ? g_up.shown_h : H;
			// (eight times coarser: such samples would belong to the LfGroup sections; the header says so and the channels stay as they are -- a stream decoders refuse at the header)
			const int es = g_up.ecup > eff_k && g_up.ecup < 8 * eff_k ? up_log_of(g_up.ecup) - up_log_of(eff_k) : 0;
			const int ecw = es ? (eff_w + g_up.ecup - 1) / g_up.ecup : W, ech = es ? (eff_h + g_up.ecup - 1) / g_up.ecup : H;
			if (es && ecw <= 256 && ech <= 256) die("vardct: ecup=: the coarser extra channels would fit one group and belong to LfGlobal, which this writer leaves empty; take a larger frame");
			const int sx0 = gx >> es, sy0 = gy >> es, sw = std::min(256 >> es, ecw - sx0), sh = std::min(256 >> es, ech - sy0);
			std::vector<Channel> sub((size_t) num_ec, Channel(sw, sh));
			for (int y = 0; y < sh; ++y) for (int x = 0; x < sw; ++x) {
				const int fx = std::min(W - 1, (sx0 + x) << es), fy = std::min(H - 1, (sy0 + y) << es);
				for (int k = 0; k < ec_extra; ++k) sub[(size_t) k].at(x, y) = ((((fx >> 3) * (k + 2) + (fy >> 2)) & 31) * emax) / 31;
				sub[(size_t) ec_extra].at(x, y) = alpha.at(fx, fy);
			}
			(void) gw; (void) gh;
			alpha_enc.emplace_back(gspec);
			if (!gspec.lz77) for (int c = 0; c < num_ec; ++c) encode_channel(tree, sub, c, 1 + 3 * num_lf_groups + 17 + g, wp_in(200 + g), alpha_enc.back());
			else {
				// glz77=1: a run of >= 3 further items equal to one item becomes a copy at special distance code 1, the previous symbol
				// (the sub-image's distance multiplier, its width, is not zero; j40.h:2834) -- the Modular mode's run-length pass
				StreamEncoder raw(gspec);
				for (int c = 0; c < num_ec; ++c) encode_channel(tree, sub, c, 1 + 3 * num_lf_groups + 17 + g, wp_in(200 + g), raw);
				StreamEncoder &enc = alpha_enc.back();
				const auto &it = raw.items;
				for (size_t i = 0; i < it.size(); ) {
					size_t j = i + 1;
					while (j < it.size() && it[j].token == it[i].token && it[i].nextra == 0 && it[j].nextra == 0 && it[i].token < 16) ++j;
					enc.items.push_back(it[i]);
					const size_t run = j - i - 1;
					if (run >= 3 && it[i].token < 16) {   // (split_exp 4: a token below 16 is its own value)
						HToken t = hybrid_encode((uint32_t) run - (uint32_t) gspec.lz_min_length, gspec.lz_len_cfg);
						enc.items.push_back({it[i + 1].cluster, t.token + (uint32_t) gspec.lz_min_symbol, t.extra, (uint8_t) t.nextra});
						const uint32_t lzcl = gspec.cluster_map[(size_t) gspec.total_dist() - 1];
						HToken d = hybrid_encode(1, gspec.cfg[lzcl]);
						enc.items.push_back({lzcl, d.token, d.extra, (uint8_t) d.nextra});
						i = j;
					} else i = i + 1;
				}
			}
			count_stream(gspec, alpha_enc.back());
		}
	}

	// ---- HF coefficients: tokens per (pass, group) with the decoder's context model ----
	const int ctx_per_preset = 495 * nb_block_ctx;
	const int hf_prefix = opt.geti("hfprefix", 0);          // HF coefficient streams with prefix codes instead of rANS
	const int hf_lz77 = opt.geti("hflz77", 0);              // ... with LZ77 copies for runs of equal small values
	// hflzmode=plain|overlap (with hflz77=1): the matcher instead of the run-length pass -- the longest match at any distance / matches
	// that overlap themselves (1 < distance < length) first; hflzminlen=, hflzdistcfg=a,b,c: the header's min_length, the distance
	// cluster's hybrid integers. (Special distance codes exist under a distance multiplier only: Modular streams, lzmode=special.)
	int hf_lzmode = LZ_RUNS;
	{
		const std::string m = opt.gets("hflzmode", "runs");
		hf_lzmode = m == "runs" ? LZ_RUNS : m == "plain" ? LZ_PLAIN : m == "overlap" ? LZ_OVERLAP : -1;
		if (m == "special") die("vardct: coefficient streams have no distance multiplier and so no special distance codes: hflzmode=runs|plain|overlap");
		if (hf_lzmode < 0) die("vardct: hflzmode=runs|plain|overlap");
		if ((hf_lzmode != LZ_RUNS || opt.kv.count("hflzminlen") || opt.kv.count("hflzdistcfg")) && !hf_lz77) die("vardct: hflzmode / hflzminlen / hflzdistcfg describe LZ77 copies: they want hflz77=1");
	}
	const int hf_lzminlen = opt.geti("hflzminlen", 3);
	if (hf_lzminlen < 3 || hf_lzminlen > 264) die("vardct: hflzminlen 3..264");
	LzStats hf_lzstats;
	std::vector<CodeSpecW> cspec((size_t) num_passes);
	std::vector<std::vector<StreamEncoder>> hf_enc((size_t) num_passes);
	std::vector<int> group_preset((size_t) num_groups);
	for (int g = 0; g < num_groups; ++g) group_preset[(size_t) g] = num_presets > 1 ? (int) rng.below((uint32_t) num_presets) : 0;
	for (int pass = 0; pass < num_passes; ++pass) {
		CodeSpecW &cs = cspec[(size_t) pass];
		const int nctx = ctx_per_preset * num_presets;
		std::vector<uint8_t> map((size_t) nctx);
		int nclusters = 0;
		for (int ctx = 0; ctx < nctx; ++ctx) {
			int preset = ctx / ctx_per_preset, r = ctx % ctx_per_preset, cl;
			if (r < 37 * nb_block_ctx) {            // number-of-nonzeros contexts
				int k = r / nb_block_ctx, b = r % nb_block_ctx;
				cl = small_clusters ? (k < 8 ? 0 : 1) : (k < 4 ? 0 : k < 12 ? 1 : k < 24 ? 2 : 3) * 3 + b % 3;
			} else {                                // coefficient contexts
				int q = r - 37 * nb_block_ctx, b = q / 458, s = q % 458;
				cl = small_clusters ? 2 + std::min(5, s / 80) : 12 + (s / 46) * 3 + b % 3;
			}
			if (!small_clusters && num_presets > 1 && preset == 1) cl = (cl * 5 + 3) % 42;  // presets share clusters differently
			map[(size_t) ctx] = (uint8_t) cl; nclusters = std::max(nclusters, cl + 1);
		}
		{   // cluster ids must be dense (j40.h:2584-2588): compact them
			std::vector<int> remap((size_t) nclusters, -1); int next = 0;
			for (auto &m : map) { if (remap[m] < 0) remap[m] = next++; m = (uint8_t) remap[m]; }
			nclusters = next;
		}
		if (hf_lz77) { map.push_back((uint8_t) nclusters); ++nclusters; cs.lz77 = true; }   // the distance context gets its own cluster
		cs.init(nctx, map, nclusters);
		cs.lz_min_symbol = 224; cs.lz_min_length = hf_lzminlen; cs.lz_len_cfg = HybridCfg{0, 0, 0};
		cs.use_prefix = hf_prefix != 0;
		cs.log_alpha = (hf_lz77 || hf_prefix) ? 8 : log_alpha;
		if (!hf_prefix && (cs.log_alpha < 5 || cs.log_alpha > 8)) dief("vardct: logalpha=%d; an rANS alphabet has 2^5..2^8 symbols", cs.log_alpha);
		for (int c = 0; c < nclusters; ++c) cs.cfg[(size_t) c] = (c & 1) && !hf_lz77 ? HybridCfg{4, 1, 1} : HybridCfg{4, 2, 0};
		if (opt.kv.count("hflzdistcfg")) {
			HybridCfg d;
			const int las = hf_prefix ? 15 : 8;
			if (sscanf(opt.gets("hflzdistcfg", "").c_str(), "%d,%d,%d", &d.split_exp, &d.msb, &d.lsb) != 3 || d.split_exp < 0 || d.split_exp >= las || d.msb < 0 || d.msb > d.split_exp || d.lsb < 0 || d.lsb > d.split_exp - d.msb)
				dief("vardct: hflzdistcfg=<split_exp>,<msb>,<lsb> with split_exp < %d, msb <= split_exp, lsb <= split_exp - msb", las);
			cs.cfg[(size_t) nclusters - 1] = d;
		}
		if (have_forced_cfg) {
			// j40.h:2297-2311: split_exp is read with at_most(log_alpha_size) (15 for prefix codes), msb with at_most(split_exp), lsb with
			// at_most(split_exp - msb), and the last two are not coded at all when split_exp == log_alpha_size
			const int las = hf_prefix ? 15 : cs.log_alpha;
			const HybridCfg &h = forced_cfg;
			if (h.split_exp < 0 || h.split_exp > las) dief("vardct: hybrid: split_exp=%d, but it is coded in 0..%d (the code's log_alpha_size; logalpha=5..8 for rANS)", h.split_exp, las);
			if (h.msb < 0 || h.msb > h.split_exp) dief("vardct: hybrid: msb=%d, but msb_in_token <= split_exp=%d", h.msb, h.split_exp);
			if (h.lsb < 0 || h.lsb > h.split_exp - h.msb) dief("vardct: hybrid: lsb=%d, but lsb_in_token <= split_exp - msb=%d", h.lsb, h.split_exp - h.msb);
			if (h.split_exp == las && (h.msb || h.lsb)) dief("vardct: hybrid: with split_exp == log_alpha_size (%d) msb and lsb are not coded and read as 0; no token beyond the split exists then", las);
			for (int c = 0; c < nclusters; ++c) cs.cfg[(size_t) c] = h;
		}
		hf_enc[(size_t) pass].reserve((size_t) num_groups);
	}
	// custom coefficient orders: Lehmer codes per (pass, order, channel); the writer only needs them
	// in the header because coefficients are synthesised in scan-index space
	const int LOG_ORDER_SIZE[13][2] = {{3,3},{3,3},{4,4},{5,5},{3,4},{3,5},{4,5},{6,6},{5,6},{7,7},{6,7},{8,8},{7,8}};
	std::vector<std::vector<std::vector<uint32_t>>> lehmer((size_t) num_passes);  // [pass][order*3+c] -> values
	int used_orders_mask = 0;
	if (custom_orders) {
		used_orders_mask = (1 << 0) | (1 << 2) | (1 << 4);
		for (int pass = 0; pass < num_passes; ++pass) {
			lehmer[(size_t) pass].assign(13 * 3, {});
			for (int o = 0; o < 13; ++o) if (used_orders_mask >> o & 1) for (int c = 0; c < 3; ++c) {
				int size = 1 << (LOG_ORDER_SIZE[o][0] + LOG_ORDER_SIZE[o][1]), skip = size / 64;
				int end = 6 + (int) rng.below(10);
				std::vector<uint32_t> v;
				for (int i = 0; i < end; ++i) v.push_back(rng.below((uint32_t) std::min(24, size - skip - i)));
				lehmer[(size_t) pass][(size_t) (o * 3 + c)] = v;
			}
		}
	}

	std::vector<float> fpix, fcoef, fydeq;   // forward=1: one block's samples, coefficients, dequantised Y coefficients
	std::vector<int32_t> jpeg_order;         // jpegdata=: scan position -> canonical index of DCT8
	if (jpeg) j40hip::natural_order(3, 3, &jpeg_order);
	for (int pass = 0; pass < num_passes; ++pass) {
		for (int g = 0; g < num_groups; ++g) {
			hf_enc[(size_t) pass].emplace_back(cspec[(size_t) pass]);
			StreamEncoder &enc = hf_enc[(size_t) pass].back();
			std::vector<Tok> hf_src;
			if (hf_lz77 && hf_lzmode != LZ_RUNS) enc.src = &hf_src;
			const int grow = g / gcols, gcol = g % gcols, ggi = (grow / 8) * ggcols + gcol / 8;
			const LfGroupW &gg = ggs[(size_t) ggi];
			const int gx8 = (gcol % 8) * 32, gy8 = (grow % 8) * 32;
			const int gw = std::min(W, (gcol + 1) * 256) - gcol * 256, gh = std::min(H, (grow + 1) * 256) - grow * 256;
			// (a subsampled frame: the group's cells come from the padded grid)
			const int gw8 = subsampled ? std::min(32, gg.w8 - gx8) : (gw + 7) / 8, gh8 = subsampled ? std::min(32, gg.h8 - gy8) : (gh + 7) / 8;
			const int ctxoff = ctx_per_preset * group_preset[(size_t) g];
			std::vector<std::array<int8_t, 3>> nonzeros((size_t) gw8 * (size_t) gh8, std::array<int8_t, 3>{0, 0, 0});
			for (int y8 = 0; y8 < gh8; ++y8) for (int x8 = 0; x8 < gw8; ++x8) {
				int cell = gg.blocks[(size_t) (gy8 + y8) * (size_t) gg.w8 + (size_t) (gx8 + x8)];
				int dctsel = cell >> 20;
				if (dctsel < 2) continue;
				dctsel -= 2;
				const LfGroupW::VB &vb = gg.vbs[(size_t) (cell & 0xfffff)];
				const int log_rows = DCTSEL[dctsel][0], log_cols = DCTSEL[dctsel][1], log_size = log_rows + log_cols, order_idx = DCTSEL[dctsel][2];
				int qfidx = 0; for (int j = 0; j < nb_qf_thr; ++j) qfidx += vb.hfmul_m1 >= qf_thr[j];
				int lfidx = gg.lfidx[(size_t) (gy8 + y8) * (size_t) gg.w8 + (size_t) (gx8 + x8)];
				int bctx0 = (order_idx * (nb_qf_thr + 1) + qfidx) * lfidx_size + lfidx, bctxc = 13 * (nb_qf_thr + 1) * lfidx_size;
				for (int cyxb = 0; cyxb < 3; ++cyxb) {
					const int c = cyxb == 0 ? 1 : cyxb == 1 ? 0 : 2;
					// a subsampled channel has a block only where the block's column and row are multiples of its 1 << shift; its non-zero
					// counts are predicted in its own coordinates (a map of its own: the channel's entries at (x8 >> hs, y8 >> vs))
					if (((gx8 + x8) & ((1 << hs[c]) - 1)) || ((gy8 + y8) & ((1 << vs[c]) - 1))) continue;
					const int cx8 = x8 >> hs[c], cy8 = y8 >> vs[c], cpos = cy8 * gw8 + cx8;
					const int bctx = bctx_map[(size_t) (bctx0 + bctxc * cyxb)];
					// choose the non-zero positions: Bernoulli with frequency decay; X/B sparser than Y
					const int size = 1 << log_size, first = size >> 6;
					double p = density * (c == 1 ? 1.0 : c == 0 ? 0.35 : 0.55) / (double) num_passes;
					std::vector<std::pair<int, int>> coefs;  // (scan index, value)
					double pk = p; const double dk = pow(decay, 64.0 / (double) size);
					if (jpeg) {
						// the block's AC integers in the stream's scan order: scan position i holds canonical index 8 u + v (u: horizontal,
						// v: vertical frequency), the file's coefficient [v][u]
						const JpegDump::Comp &jc = jd.slot(c);
						const int bx = ((gg.left >> 3) + gx8 + x8) >> hs[c], by = ((gg.top >> 3) + gy8 + y8) >> vs[c];
						if (bx >= jc.bx || by >= jc.by) die("vardct: jpegdata=: a block beyond the component's block grid");
						const int16_t *q = &jc.coef[((size_t) by * (size_t) jc.bx + (size_t) bx) * 64];
						for (int i = first; i < size; ++i) {
							const int pos = jpeg_order[(size_t) i], at = (pos & 7) * 8 + (pos >> 3);
							if (!q[at]) continue;
							const int64_t n = (int64_t) q[at] * (jc.table[at] / jpeg_gcd(jc.table[at], JPEG_L)) * JPEG_K[c];
							if (n < -(1 << 28) || n > (1 << 28)) die("vardct: jpegdata=: a scaled coefficient leaves the 29 bits a hybrid integer holds here");
							coefs.push_back({i, (int) n});
						}
					} else if (forward) {
						// the block's samples -> coefficients -> quantised with the weights the decoder divides by (j40.h:7086-7094);
						// X and B code what is left after the decoder's chroma-from-luma term (default factors: 0 and 1 times the
						// dequantised Y coefficient, j40.h:7138-7143, 7159-7171)
						const int R = 1 << log_rows, C = 1 << log_cols;
						const int px0 = ((gg.left >> 3) + gx8 + x8) >> hs[c] << 3, py0 = ((gg.top >> 3) + gy8 + y8) >> vs[c] << 3;   // (in the plane's own coordinates)
						fpix.resize((size_t) size); fcoef.resize((size_t) size);
						for (int y = 0; y < R; ++y) for (int x = 0; x < C; ++x) fpix[(size_t) (y * C + x)] = plane[c][(size_t) (py0 + y) * (size_t) pwc[c] + (size_t) (px0 + x)];
						fwdx->analyse(dctsel, fpix.data(), fcoef.data());
						const float mult1 = 65536.0f / (float) global_scale / (float) (vb.hfmul_m1 + 1);
						const float mult_c = c == 1 ? mult1 : c == 0 ? mult1 * powf(0.8f, (float) (x_qm - 2)) : mult1 * powf(0.8f, (float) (b_qm - 2));
						const std::vector<float> &wt = fwdx->weight[dctsel][c];
						const std::vector<int32_t> &ord = fwdx->order[dctsel];
						if (c == 1) fydeq.assign((size_t) size, 0.0f);
						const float dead = (float) opt.getd("deadzone", 0.56);
						for (int i = first; i < size; ++i) {
							const int pos = ord[(size_t) i];
							float target = fcoef[(size_t) pos];
							if (c == 2 && !nocfl && !subsampled) target -= fydeq[(size_t) pos];
							const float scaled = target * wt[(size_t) pos] / mult_c;
							const int q = fabsf(scaled) < dead ? 0 : (int) lrintf(scaled);
							if (c == 1 && q) fydeq[(size_t) pos] = synthfwd::dequant((float) q, 1, mult_c, wt[(size_t) pos]);
							if (q) coefs.push_back({i, q});
						}
					} else {
					// d1-like statistics: non-zeros concentrate at low frequencies (so the scan ends early, as an
					// encoder's would) and low frequencies carry the larger magnitudes
					double cont = opt.getd("cont", 0.86);
					for (int i = first; i < size && pk > 2e-3; ++i) {
						if (rng.unit() < pk) {
							int mag = 1; while (mag < 40 && rng.unit() < cont) ++mag;
							int v = rng.below(2) ? mag : -mag;
							if (bigshare > 0 && rng.unit() < bigshare) {
								const uint32_t lo = 1u << (bigbits - 1), pick = rng.below(8);
								const uint32_t m = pick == 0 ? lo : pick == 1 ? 2 * lo - 1 : lo + (uint32_t) (rng.next() >> 20) % lo;
								v = v < 0 ? -(int) m : (int) m;
							}
							if (flat) v = flat;
							coefs.push_back({i, v});
						}
						pk *= dk; cont = 0.3 + (cont - 0.3) * pow(dk, 0.6);
					}
					}
					int nz = (int) coefs.size();
					if (nz > (63 << (log_size - 6))) { coefs.resize((size_t) (63 << (log_size - 6))); nz = (int) coefs.size(); }
					int pred;
					if (cx8 > 0) pred = cy8 > 0 ? (nonzeros[(size_t) cpos - 1][(size_t) c] + nonzeros[(size_t) (cpos - gw8)][(size_t) c] + 1) >> 1 : nonzeros[(size_t) cpos - 1][(size_t) c];
					else pred = cy8 > 0 ? nonzeros[(size_t) (cpos - gw8)][(size_t) c] : 32;
					int nzctx = ctxoff + bctx + (pred < 8 ? pred : 4 + pred / 2) * nb_block_ctx;
					enc.add((uint32_t) nzctx, (uint32_t) nz);
					int qnz = (nz + (1 << (log_size - 6)) - 1) >> (log_size - 6);
					for (int i = 0; i < (1 << (log_rows - 3)); ++i) for (int j = 0; j < (1 << (log_cols - 3)); ++j)
						if (cy8 + i < gh8 && cx8 + j < gw8) nonzeros[(size_t) (cpos + i * gw8 + j)][(size_t) c] = (int8_t) qnz;
					const int cctx = ctxoff + 458 * bctx + 37 * nb_block_ctx;
					int prev = nz <= (1 << (log_size - 4)), remaining = nz;
					size_t next = 0;
					for (int i = first; remaining > 0 && i < size; ++i) {
						int ctx = cctx + nnz_ctx2((remaining + (1 << (log_size - 6)) - 1) >> (log_size - 6)) + FREQ_CTX2[i >> (log_size - 6)] + prev;
						int v = 0;
						if (next < coefs.size() && coefs[next].first == i) v = coefs[next++].second;
						enc.add((uint32_t) ctx, pack_signed(v));
						prev = v != 0; remaining -= prev;
					}
				}
			}
			if (hf_lz77 && hf_lzmode != LZ_RUNS) {
				// the matcher of jxlsynth_lz77.hpp over this stream's integers (coefficient streams have no distance multiplier: the
				// symbol codes distance - 1, j40.h:2829); nothing here lies in rows or channels
				std::vector<uint32_t> ctxs, vals;
				for (const Tok &t : hf_src) { ctxs.push_back(t.ctx); vals.push_back(t.value); }
				const std::vector<uint32_t> nowhere(vals.size(), 0);
				LzParams lp; lp.mode = hf_lzmode; lp.dist_mult = 0;
				enc.items.clear(); enc.src = nullptr;
				lz77_match(enc, cspec[(size_t) pass], lp, ctxs, vals, nowhere, nowhere, hf_lzstats);
			} else if (hf_lz77) {
				// run-length pass: a run of >= 3 identical small values after its first occurrence becomes one copy with
				// distance 1 (dist_mult is 0 for coefficient streams, so the coded distance value is distance - 1, j40.h:2851)
				const CodeSpecW &cs = cspec[(size_t) pass];
				std::vector<StreamEncoder::Item> out;
				const auto &it = enc.items;
				for (const auto &item : it) if ((int) item.token >= cs.lz_min_symbol)
					dief("vardct: hflz77=1 reads tokens from %d on as copy lengths, but a literal needs token %u under hybrid integers {%d,%d,%d}",
					     cs.lz_min_symbol, item.token, cs.cfg[item.cluster].split_exp, cs.cfg[item.cluster].msb, cs.cfg[item.cluster].lsb);
				for (size_t i = 0; i < it.size(); ) {
					size_t j = i + 1;
					while (j < it.size() && it[j].token == it[i].token && it[i].nextra == 0 && it[j].nextra == 0 && it[i].token < 16) ++j;
					out.push_back(it[i]);
					const size_t run = j - i - 1;
					if (run >= 3 && it[i].token < 16) {
						HToken t = hybrid_encode((uint32_t) run - (uint32_t) cs.lz_min_length, cs.lz_len_cfg);
						out.push_back({it[i + 1].cluster, t.token + (uint32_t) cs.lz_min_symbol, t.extra, (uint8_t) t.nextra});
						const uint32_t lzcl = cs.cluster_map[(size_t) cs.total_dist() - 1];
						HToken d = hybrid_encode(0, cs.cfg[lzcl]);
						out.push_back({lzcl, d.token, d.extra, (uint8_t) d.nextra});
						++hf_lzstats.copies; ++hf_lzstats.plain_copies; ++hf_lzstats.distance_one; hf_lzstats.max_distance = std::max<uint64_t>(hf_lzstats.max_distance, 1);
						i = j;
					} else i = i + 1;
				}
				enc.items.swap(out);
			}
			count_stream(cspec[(size_t) pass], enc);
		}
	}

	for (int pass = 0; pass < num_passes; ++pass) {   // say why a combination cannot be written before the writer trips over it
		const CodeSpecW &cs = cspec[(size_t) pass];
		for (int c = 0; c < cs.num_clusters; ++c) {
			const int ntok = (int) cs.freq[(size_t) c].size();
			if (ntok > cs.alphabet_limit())
				dief("vardct: an HF cluster with hybrid integers {%d,%d,%d} needs token %d, but the alphabet has %d symbols (logalpha=%d): raise logalpha, "
				     "or lower what is coded (density, maxlog: a block's non-zero count; cont, bigbits: the magnitudes) or the hybrid split",
				     cs.cfg[(size_t) c].split_exp, cs.cfg[(size_t) c].msb, cs.cfg[(size_t) c].lsb, ntok - 1, cs.alphabet_limit(), cs.log_alpha);
		}
	}

	// ---- assemble sections ----
	std::vector<std::vector<uint8_t>> sections;
	auto write_lf_global = [&](BitWriter &section) {   // LfGlobal (j40.h:6257)
		write_patch_dictionary(section, num_ec);                 // (patches=: the dictionary comes first)
		BitWriter dropped;                                       // (patchcut=1: the rest is written all the same, the code specs' tables are made here)
		BitWriter &bw0 = cut_patch_dictionary(section) ? dropped : section;
		const size_t before_splines = bw0.bytes.size();
		write_splines(bw0);                                      // (splines=: behind the dictionary)
		BitWriter &bw = &bw0 == &section && cut_splines(section, before_splines) ? dropped : bw0;   // (splinecut=1: as patchcut=1)
		write_noise_parameters(bw);                              // (noise=: behind the splines)
		bw.put(1, 1);                                            // LF channel dequantisation: default
		bw.u32(global_scale, 1, 11, 2049, 11, 4097, 12, 8193, 16);
		bw.u32(quant_lf, 16, 0, 1, 5, 1, 8, 1, 16);
		if (!custom_bctx) bw.put(1, 1);
		else {
			bw.put(0, 1);
			for (int i = 0; i < 3; ++i) {
				bw.put((uint64_t) nb_lf_thr[i], 4);
				for (int j = 0; j < nb_lf_thr[i]; ++j) bw.u32(pack_signed(lf_thr[i][j]), 0, 4, 16, 8, 272, 16, 65808, 32);
			}
			bw.put((uint64_t) nb_qf_thr, 4);
			for (int j = 0; j < nb_qf_thr; ++j) bw.u32(qf_thr[j] - 1, 0, 2, 4, 3, 12, 5, 44, 8);
			write_cluster_map(bw, bctx_map, nb_block_ctx);
		}
		if (nocfl) { bw.put(0, 1); bw.u32(84, 84, 0, 256, 0, 2, 8, 258, 16); bw.f16(0.0f); bw.f16(0.0f); bw.put(127, 8); bw.put(127, 8); }   // all zero
		else if (!custom_cfl) bw.put(1, 1);                   // LF channel correlation: default
		else { bw.put(0, 1); bw.u32(128, 84, 0, 256, 0, 2, 8, 258, 16); bw.f16(0.125f); bw.f16(0.75f); bw.put(127 + 3, 8); bw.put(127 - 2, 8); }
		bw.put(1, 1);                                            // global tree present
		write_code_spec(bw, treespec); tree_enc.flush(bw);
		write_code_spec(bw, gspec);
		if (with_alpha) {   // the global Modular image (extra channels only): header, no channel decoded here (j40.h:6329-6338)
			write_modular_header(bw, true, custom_wp && wpat != "group" ? &wp_base : nullptr, {});
			StreamEncoder none(gspec); none.flush(bw);
		}
	};
	auto write_lf_group = [&](BitWriter &bw, int ggi) {  // LfGroup (j40.h:6722)
		LfGroupW &gg = ggs[(size_t) ggi];
		if (!(g_lf && g_lf->use)) {   // (a frame with use_lf_frame: the section starts at nb_varblocks, j40.h:6747)
			bw.put((uint64_t) extra_prec, 2);                        // extra_precision
			write_modular_header(bw, true, wp_of(2 * ggi), {});
			lfq_enc[(size_t) ggi].flush(bw);
		}
		bw.put((uint64_t) (gg.vbs.size() - 1), ceil_lg((uint32_t) (gg.w8 * gg.h8)));
		write_modular_header(bw, true, wp_of(2 * ggi + 1), {});
		meta_enc[(size_t) ggi].flush(bw);
	};
	auto write_hf_global = [&](BitWriter &bw) {   // HfGlobal + HfPass (j40.h:6819)
		if (jpeg) {   // DCT8 raw, the sixteen others from the library
			bw.put(0, 1);
			bw.put(7, 3); bw.put(f16_bits(JPEG_DENOM), 16);
			write_modular_header(bw, true, wp_of(100), {});
			dq_raw[0].second.flush(bw);
			for (int idx = 1; idx < 17; ++idx) bw.put(0, 3);
		} else if (opt.geti("dq", 0)) { bw.put(0, 1); write_dq_matrices(bw, dq_raw, wp_of); }
		else bw.put(1, 1);                                       // all dequantisation matrices default
		bw.put((uint64_t) (num_presets - 1), ceil_lg((uint32_t) num_groups));
		for (int pass = 0; pass < num_passes; ++pass) {
			if (!used_orders_mask) bw.put(2, 2);                 // used_orders = 0
			else {
				bw.put(3, 2); bw.put((uint64_t) used_orders_mask, 13);
				CodeSpecW ospec; ospec.init(8, std::vector<uint8_t>(8, 0), 1); ospec.log_alpha = 6; ospec.cfg[0] = HybridCfg{4, 1, 0};
				StreamEncoder oenc(ospec);
				for (int o = 0; o < 13; ++o) if (used_orders_mask >> o & 1) for (int c = 0; c < 3; ++c) {
					const auto &v = lehmer[(size_t) pass][(size_t) (o * 3 + c)];
					int size = 1 << (LOG_ORDER_SIZE[o][0] + LOG_ORDER_SIZE[o][1]);
					oenc.add((uint32_t) std::min(7, ceil_lg((uint32_t) size + 1)), (uint32_t) v.size());  // j40.h:5437
					uint32_t prev = 0;
					for (uint32_t x : v) { oenc.add((uint32_t) std::min(7, ceil_lg(prev + 1)), x); prev = x; }
				}
				count_stream(ospec, oenc);
				write_code_spec(bw, ospec); oenc.flush(bw);
			}
			write_code_spec(bw, cspec[(size_t) pass]);
		}
	};
	auto write_pass_group = [&](BitWriter &bw, int pass, int g) {  // PassGroup (j40.h:7007)
		bw.put((uint64_t) group_preset[(size_t) g], ceil_lg((uint32_t) num_presets));
		hf_enc[(size_t) pass][(size_t) g].flush(bw);
		if (with_alpha) { write_modular_header(bw, true, wp_of(200 + g), {}); alpha_enc[(size_t) g].flush(bw); }
	};
	if (single_section) {
		// one group, one pass: a single section, read in the order LfGlobal, HfGlobal, LfGroup, PassGroup (j40.h:8189-8199) with no
		// padding between them
		BitWriter bw;
		write_lf_global(bw); write_hf_global(bw); write_lf_group(bw, 0); write_pass_group(bw, 0, 0);
		bw.pad();
		sections.push_back(bw.bytes);
	} else {
		{ BitWriter bw; write_lf_global(bw); bw.pad(); sections.push_back(bw.bytes); }
		for (int ggi = 0; ggi < num_lf_groups; ++ggi) { BitWriter bw; write_lf_group(bw, ggi); bw.pad(); sections.push_back(bw.bytes); }
		{ BitWriter bw; write_hf_global(bw); bw.pad(); sections.push_back(bw.bytes); }
		for (int pass = 0; pass < num_passes; ++pass) for (int g = 0; g < num_groups; ++g) { BitWriter bw; write_pass_group(bw, pass, g); bw.pad(); sections.push_back(bw.bytes); }
	}

	// ---- codestream ----
	BitWriter cs;
	const bool seq_anim = g_seq && g_seq->anim;
	if (g_seq && (opt.geti("icc", 0) || !nonzero_header)) die("vardct: frames= wants fullheader=1 and no icc");
	const int icc_bytes = opt.geti("icc", 0);                // > 0: ColourEncoding with want_icc and an ICC stream of that many coded bytes
	const int img_bpp = opt.geti("bpp", 8);   // 9..15: the renderer's scaling to 8 bits and the long way through the transfer curve get work
	if (img_bpp != 8 && icc_bytes) die("vardct: bpp does not combine with icc here");
	const int noxyb = opt.geti("noxyb", 0) || ycbcr;
	if (noxyb && (icc_bytes || !nonzero_header || x_qm != 3 || b_qm != 2)) die("vardct: noxyb wants fullheader=1, no icc and the default qm scales");
	if (noxyb && g_seq && !with_alpha) die("vardct: noxyb in frames= wants alpha=1");
	// wide=1: the metadata says modular_16bit_buffers = 0 and nothing else changes (a stream readers refuse: "fm32", or "TODO" where wide
	// Modular frames are asked for). The metadata must be written out: bpp != 8 or alpha=1
	const int vd_wide = opt.geti("wide", 0);
	if (vd_wide && img_bpp == 8 && !with_alpha) die("vardct: wide=1 wants metadata that is written out: bpp=9..15 or alpha=1");
	if (!g_seq || g_seq->first) {
	cs.put(0xff, 8); cs.put(0x0a, 8);
	write_size_header(cs, g_seq ? g_seq->canvas_w : up_flag() ? g_up.shown_w : W, g_seq ? g_seq->canvas_h : up_flag() ? g_up.shown_h : H);   // (upsampling=: the shown size)
	if (with_alpha && (img_bpp != 8 || ec_extra || alpha_bpp != 8 || alpha_assoc)) {
		cs.put(0, 1);                       // ImageMetadata: not all_default
		write_extra_fields(cs);             // no extra fields (an animation: its header)
		write_bit_depth(cs, img_bpp);
		cs.put(vd_wide ? 0 : 1, 1);         // modular_16bit_buffers (wide=1: 0)
		if (num_ec == 1) cs.put(1, 2); else { cs.put(2, 2); cs.put((uint64_t) (num_ec - 2), 4); }   // num_extra_channels (j40.h:3170)
		for (int k = 0; k < ec_extra; ++k) {
			cs.put(0, 1);                   // not the default alpha
			cs.put(1, 2);                   // type: enum selector 1 = depth
			write_bit_depth(cs, img_bpp);
			cs.put(0, 2);                   // dim_shift 0
			cs.put(0, 2);                   // no name
		}
		if (alpha_bpp == 8 && !alpha_assoc) cs.put(1, 1);   // d_alpha
		else {
			cs.put(0, 1);
			cs.put(0, 2);                   // type: enum selector 0 = alpha
			write_bit_depth(cs, alpha_bpp);
			cs.put(0, 2);                   // dim_shift 0
			cs.put(0, 2);                   // no name
			cs.put((uint64_t) (alpha_assoc ? 1 : 0), 1);   // alpha_associated (j40.h:3188)
		}
		cs.put(noxyb ? 0 : 1, 1);           // xyb_encoded
		if (!write_colour_encoding(cs)) cs.put(1, 1);   // ColourEncoding.all_default (cenc=: written out)
		write_header_tail(cs, true, !noxyb);
	} else if ((g_cenc.set && !with_alpha && !icc_bytes) || img_bpp != 8 || (seq_anim && !with_alpha) || (noxyb && !with_alpha) || ((g_orientation || !g_tone.empty()) && !with_alpha && !icc_bytes)) {   // (orientation=N, tone=: the metadata written out where it would be all_default)
		cs.put(0, 1);                       // ImageMetadata: not all_default
		write_extra_fields(cs);             // no extra fields (an animation: its header)
		write_bit_depth(cs, img_bpp);
		cs.put(vd_wide ? 0 : 1, 1);         // modular_16bit_buffers (wide=1: 0)
		cs.put(0, 2);                       // no extra channels
		cs.put(noxyb ? 0 : 1, 1);           // xyb_encoded
		if (noxyb && opt.geti("grey", 0)) {
			// grey=1 (with noxyb / ycbcr, no alpha): the colour encoding says grey, D65, sRGB transfer, relative intent -- a stream the
			// decoder refuses (the frame still codes three channels)
			cs.put(0, 1); cs.put(0, 1);     // ColourEncoding: not all_default, no ICC profile
			cs.put(1, 2);                   // colour_space = grey (enum value 1)
			cs.put(1, 2);                   // white_point = D65
			cs.put(0, 1);                   // no gamma
			cs.put(2, 2); cs.put(11, 4);    // transfer function 13 (sRGB): enum selector 2, 2 + 11
			cs.put(1, 2);                   // rendering intent 1
		} else
		if (!write_colour_encoding(cs)) cs.put(1, 1);   // ColourEncoding.all_default (cenc=: written out)
		write_header_tail(cs, true, !noxyb);
	} else if (!icc_bytes && !with_alpha) {
		cs.put(1, 1);   // ImageMetadata.all_default: 8-bit, XYB, no extra channels
		write_header_tail(cs, false, true);
	} else if (!icc_bytes) {
		cs.put(0, 1);                       // ImageMetadata: not all_default
		write_extra_fields(cs);             // no extra fields (an animation: its header)
		cs.put(0, 1); cs.put(0, 2);         // integer samples, 8 bits
		cs.put(vd_wide ? 0 : 1, 1);         // modular_16bit_buffers (wide=1: 0)
		cs.put(1, 2); cs.put(1, 1);         // one extra channel, d_alpha
		cs.put(noxyb ? 0 : 1, 1);           // xyb_encoded (noxyb=1: the reference runs the XYB inverse on VarDCT frames regardless, j40.h:7206)
		if (!write_colour_encoding(cs)) cs.put(1, 1);   // ColourEncoding.all_default (cenc=: written out)
		write_header_tail(cs, true, !noxyb);
	} else {
		cs.put(0, 1);                       // ImageMetadata: not all_default
		write_extra_fields(cs);             // no extra fields (an animation: its header)
		cs.put(0, 1); cs.put(0, 2);         // integer samples, 8 bits
		cs.put(vd_wide ? 0 : 1, 1);         // modular_16bit_buffers (wide=1: 0)
		cs.put(0, 2);                       // no extra channels
		cs.put(1, 1);                       // xyb_encoded
		cs.put(0, 1);                       // ColourEncoding: not all_default
		cs.put(1, 1);                       // want_icc
		cs.put(0, 2);                       // colour_space = RGB (enum selector 0)
		write_header_tail(cs, true, true);
		write_icc_stream(cs, rng, icc_bytes);
	}
	}
	cs.pad();       // frame header starts byte aligned (j40.h:5228)
	if (!nonzero_header) cs.put(1, 1);  // FrameHeader.all_default
	else {
		cs.put(0, 1);
		const bool lf_frame = g_lf && g_lf->level > 0, use_lf_frame = g_lf && g_lf->use;
		if ((lf_frame || use_lf_frame) && !g_seq) die("vardct: an LF frame, and a frame with use_lf_frame, is written by lflevels= only");
		const int seq_type = g_seq ? g_seq->type : 0;
		cs.put(lf_frame ? 1 : (uint64_t) seq_type, 2);   // regular frame (an LF frame: type 1; types=: a reference-only frame, type 2)
		cs.put(0, 1);                       // VarDCT
		cs.u64((skip_smooth ? 128 : 0) | (use_lf_frame ? 32 : 0) | (patch_flag() ? 2 : 0) | (noise_flag() ? 1 : 0) | (spline_flag() ? 16 : 0));      // flags
		if (noxyb) cs.put(ycbcr ? 1 : 0, 1);   // do_ycbcr (read only without xyb_encoded)
		// (jpegup=N: the header says N whatever the stream holds -- a layout the decoder has to refuse before it reads anything of it)
		if (ycbcr) cs.put((uint64_t) opt.geti("jpegup", jpeg_upsampling), 6);   // jpeg_upsampling (read with do_ycbcr)
		if (!use_lf_frame) {                // (not coded with use_lf_frame, j40.h:5262)
		cs.put((uint64_t) up_log(), 2);     // log_upsampling (upsampling=)
		for (int i = 0; i < num_ec; ++i) cs.put((uint64_t) up_ec_log(), 2);   // ec_log_upsampling
		}
		if (!noxyb) { cs.put((uint64_t) x_qm, 3); cs.put((uint64_t) b_qm, 3); }
		if (seq_type == 2 && num_passes != 1) die("vardct: a reference-only frame codes no passes: passes=1");
		if (seq_type != 2) cs.u32(num_passes, 1, 0, 2, 0, 3, 0, 4, 3);   // (not coded for a reference-only frame, j40.h:5276)
		if (num_passes > 1) {
			cs.u32(0, 0, 0, 1, 0, 2, 0, 3, 1);                  // num_ds = 0
			for (int i = 0; i < num_passes - 1; ++i) cs.put(0, 2);  // shift[i]
		}
		if (lf_frame) cs.put((uint64_t) (g_lf->level - 1), 2);   // lf_level - 1; no crop, no blend info, never last, saved nowhere (j40.h:5285-5336)
		else
		write_frame_placement(cs, num_ec, W, H);   // have_crop, blend modes, is_last
		cs.u32(0, 0, 0, 0, 4, 16, 5, 48, 10);  // name length 0
		// RestorationFilter (j40.h:5339-5366). gab=1: Gaborish with the default weights, gab=2: custom weights; epf=1..3: iterations of the
		// edge-preserving filter, always with a custom sharpness table (the default table's first entry is 0, which the reference's
		// j40__epf_recip_sigmas rejects with "epf0", j40.h:7384; epflut=0 writes the default all the same), epfw=1: custom channel
		// scales, epfs=1: custom sigma parameters; rfdefault=1: all_default = 1 (the reference then still reads the conditional bits)
		const int gab = opt.geti("gab", 0), epf = opt.geti("epf", 0);
		if (opt.geti("rfdefault", 0)) { cs.put(1, 1); cs.put(0, 1); cs.put(0, 1); cs.put(0, 1); cs.put(0, 1); }   // all_default; then gab_custom 0, sharp_custom 0, weight_custom 0, sigma_custom 0
		else {
			cs.put(0, 1);                       // restoration: !all_default
			cs.put(gab ? 1 : 0, 1);
			if (gab) {
				cs.put(gab == 2 ? 1 : 0, 1);
				if (gab == 2) { const float w[6] = {0.125f, 0.0625f, 0.1875f, 0.03125f, 0.09375f, 0.078125f}; for (float v : w) cs.f16(v); }
			}
			cs.put((uint64_t) epf, 2);
			if (epf) {
				const int lut = opt.geti("epflut", 1);
				cs.put(lut ? 1 : 0, 1);
				if (lut) { const float t[8] = {0.25f, 0.375f, 0.5f, 0.625f, 0.75f, 1.0f, 1.25f, 1.5f}; for (float v : t) cs.f16(v); }
				const int ew = opt.geti("epfw", 0);
				cs.put(ew ? 1 : 0, 1);
				if (ew) { cs.f16(32.0f); cs.f16(6.0f); cs.f16(3.0f); cs.put(0, 32); }
				const int es = opt.geti("epfs", 0);
				cs.put(es ? 1 : 0, 1);
				if (es) { cs.f16(0.5f); cs.f16(0.75f); cs.f16(5.0f); cs.f16(0.625f); }
			}
			cs.u64(0);                          // restoration extensions
		}
		cs.u64(0);                          // frame extensions
	}
	// TOC (j40.h:5505-5531)
	write_toc_and_sections(cs, sections, opt.geti("permute", 0), rng, opt.geti("slack", 0));
	if (g_seq) { seq_append(cs, sections); return 0; }

	std::vector<uint8_t> file;
	if (!container) file = cs.bytes;
	else {
		// ISOBMFF wrapping (j40.h:1479): signature box, ftyp, then the codestream split over two jxlp boxes
		static const uint8_t HEAD[32] = {0, 0, 0, 0x0c, 'J', 'X', 'L', ' ', 0x0d, 0x0a, 0x87, 0x0a, 0, 0, 0, 0x14, 'f', 't', 'y', 'p', 'j', 'x', 'l', ' ', 0, 0, 0, 0, 'j', 'x', 'l', ' '};
		file.assign(HEAD, HEAD + 32);
		auto box = [&](const char *type, const uint8_t *p, size_t n, int jxlp_index) {
			size_t total = 8 + n + (jxlp_index != -1 ? 4 : 0);
			uint8_t hd[8] = {(uint8_t) (total >> 24), (uint8_t) (total >> 16), (uint8_t) (total >> 8), (uint8_t) total, (uint8_t) type[0], (uint8_t) type[1], (uint8_t) type[2], (uint8_t) type[3]};
			file.insert(file.end(), hd, hd + 8);
			if (jxlp_index != -1) { uint32_t idx = (uint32_t) jxlp_index; uint8_t ix[4] = {(uint8_t) (idx >> 24), (uint8_t) (idx >> 16), (uint8_t) (idx >> 8), (uint8_t) idx}; file.insert(file.end(), ix, ix + 4); }
			file.insert(file.end(), p, p + n);
		};
		if (container == 1) box("jxlc", cs.bytes.data(), cs.bytes.size(), -1);
		else {
			size_t half = cs.bytes.size() / 3;
			// NOTE the reference treats a jxlp index *without* the top bit as "last" (j40.h:1557, inverted
			// w.r.t. ISO 18181-2); order the flags the way it accepts
			box("jxlp", cs.bytes.data(), half, (int) 0x80000000u);
			static const uint8_t junk[5] = {1, 2, 3, 4, 5};
			box("xml ", junk, 5, -1);
			box("jxlp", cs.bytes.data() + half, cs.bytes.size() - half, 1);
		}
	}
	if (!write_file(out, file)) die("cannot write output");
	double bpp = 8.0 * (double) file.size() / ((double) W * H);
	if (opt.geti("stats", 0))
		printf("{\"copies\": %llu, \"plain_copies\": %llu, \"overlapping_copies\": %llu, \"distance_one_copies\": %llu, \"max_distance\": %llu, \"max_length\": %llu, %s}\n",
		       (unsigned long long) hf_lzstats.copies, (unsigned long long) hf_lzstats.plain_copies, (unsigned long long) hf_lzstats.overlapping, (unsigned long long) hf_lzstats.distance_one,
		       (unsigned long long) hf_lzstats.max_distance, (unsigned long long) hf_lzstats.max_length, wp_stats_json().c_str());
	fprintf(stderr, "vardct %dx%d: %zu bytes (%.3f bpp), %d groups, %d LF groups, %d passes\n", W, H, file.size(), bpp, num_groups, num_lf_groups, num_passes);
	return 0;
}

// ------------------------------------------------------------------------------------------------
// Modular frames (lossless-style): RGB or RGBA, global RCT and/or Palette, MA tree with a choice of
// predictors (incl. the weighted predictor), ANS or prefix codes, optional LZ77 run-lengths.
// Single-group frames put everything into LfGlobal (one section, j40.h:6329-6336); larger frames
// code every group's rectangle in its own PassGroup section (j40.h:7024-7033).

static void forward_rct(std::vector<Channel> &ch, int first, int type) {
	// exact inverse of the decoder's RCT for the un-permuted types (j40.h:4341-4393)
	const size_t n = ch[(size_t) first].px.size();
	int32_t *a = ch[(size_t) first].px.data(), *b = ch[(size_t) first + 1].px.data(), *c = ch[(size_t) first + 2].px.data();
	for (size_t i = 0; i < n; ++i) {
		int32_t p0 = a[i], p1 = b[i], p2 = c[i];
		switch (type % 7) {
		case 0: break;
		case 1: c[i] = p2 - p0; break;
		case 2: c[i] = p2 - p0; b[i] = p1; break;   // decoder: out2 = in1 + in0 (needs in1 == in2 - in0; see below)
		case 3: b[i] = p1 - p0; c[i] = p2 - p0; break;
		case 4: b[i] = p1 - ((p0 >> 1) + (p2 >> 1) + (p0 & p2 & 1)); break;
		case 5: c[i] = p2 - p0; b[i] = p1 - p0 - ((p2 - p0) >> 1); break;
		case 6: { int32_t co = p0 - p2, tmp = p2 + (co >> 1), cg = p1 - tmp, y = tmp + (cg >> 1); a[i] = y; b[i] = co; c[i] = cg; break; }
		}
	}
}

int run_modular(int W, int H, uint64_t seed, const char *out, const Options &opt) {
	SplitMix64 rng(seed * 0x9e3779b97f4a7c15ull + 777);
	const int alpha = opt.geti("alpha", 0);
	const int group_shift = opt.geti("groupshift", 8);
	const int rct = opt.geti("rct", 6);                   // -1: none
	const int use_prefix = opt.geti("prefix", 0);
	const int lz77 = opt.geti("lz77", 0);
	const int tree_kind = opt.geti("tree", 0);            // 0 gradient, 1 per-channel leaves + property splits, 2 weighted predictor, 3 previous-channel properties, 8 a first-sample leaf
	const int palette = opt.geti("palette", 0);           // 0 none, 1 plain palette, 2 with deltas / synthetic colours, 3 with delta prediction
	const int container = opt.geti("container", 0);
	// wide=1: the image metadata says modular_16bit_buffers = 0 -- samples are int32 to a reader -- and NOTHING else changes: at bpp <= 15
	// the same seed and options give the same picture and the same sections. It admits bpp=16 (a 16-bit sample does not fit int16),
	// an alpha channel at a depth other than 8 (written at the image's depth), range= and povfto= beyond int16, and bias=K (added to
	// every colour sample before the clamp to range=: pictures near the ends of int32)
	const int wide = opt.geti("wide", 0);
	const int bpp = opt.geti("bpp", 8);   // 8..15 (16-bit buffers); 16 with wide=1
	if (bpp < 8 || bpp > (wide ? 16 : 15)) die("modular: bpp 8..15 (8..16 with wide=1)");
	if (bpp != 8 && alpha && !wide) die("modular: the default alpha channel has 8 bits; the reference refuses a different colour depth");
	const bool deep_alpha = wide && alpha && bpp != 8;   // the alpha channel has the image's depth
	sample_lo() = wide ? INT32_MIN : -32768; sample_hi() = wide ? INT32_MAX : 32767;
	const int64_t bias = wide ? strtoll(opt.gets("bias", "0").c_str(), nullptr, 10) : 0;
	if (!wide && opt.kv.count("bias")) die("modular: bias= wants wide=1");
	const int gdim = 1 << group_shift;
	// ---- streams outside an encoder's habits (tests/test_modular_stress.py); every option defaults to what was written before ----
	// lzmode=special|plain|overlap (with lz77=1): a matcher over the decoded integers instead of the run-length pass; it prefers
	// distances a special code stands for / codes every distance plain / prefers copies that overlap themselves (1 < distance < length).
	// lzforce=specials|early|over|far: copies that define the samples they cover (jxlsynth_lz77.hpp; tree=4, no palette).
	// lzminlen=, lzminsym=, lzlencfg=a,b,c, lzdistcfg=a,b,c: the header's other selectors and hybrid-integer configurations;
	// hybrid=a,b,c: the configuration of the residual clusters.
	LzParams lzp;
	{
		const std::string m = opt.gets("lzmode", "runs"), f = opt.gets("lzforce", "none");
		lzp.mode = m == "runs" ? LZ_RUNS : m == "special" ? LZ_SPECIAL : m == "plain" ? LZ_PLAIN : m == "overlap" ? LZ_OVERLAP : -1;
		lzp.force = f == "none" ? FORCE_NONE : f == "specials" ? FORCE_SPECIALS : f == "early" ? FORCE_EARLY : f == "over" ? FORCE_OVER : f == "far" ? FORCE_FAR : -1;
		if (lzp.mode < 0) die("modular: lzmode=runs|special|plain|overlap");
		if (lzp.force < 0) die("modular: lzforce=none|specials|early|over|far");
		if ((lzp.mode != LZ_RUNS || lzp.force != FORCE_NONE || opt.kv.count("lzminlen") || opt.kv.count("lzminsym") || opt.kv.count("lzlencfg") || opt.kv.count("lzdistcfg")) && !lz77)
			die("modular: lzmode / lzforce / lzminlen / lzminsym / lzlencfg / lzdistcfg describe LZ77 copies: they want lz77=1");
		if (lzp.force != FORCE_NONE && (tree_kind != 4 || palette || opt.geti("squeeze", 0) || opt.geti("localpalette", 0) || opt.geti("localtree", 0)))
			die("modular: lzforce defines samples by the copies that cover them: that needs the zero predictor in one leaf (tree=4) and neither palette, squeeze nor local trees");
		if (lzp.force != FORCE_NONE && lzp.mode != LZ_RUNS) die("modular: lzforce writes its own copies; lzmode chooses among matches of a picture");
		lzp.literal_range = 1u << bpp;
	}
	auto parse_cfg = [&](const char *key, HybridCfg def, int log_alpha_size) {
		if (!opt.kv.count(key)) return def;
		HybridCfg c;
		if (sscanf(opt.gets(key, "").c_str(), "%d,%d,%d", &c.split_exp, &c.msb, &c.lsb) != 3) dief("modular: %s=<split_exp>,<msb>,<lsb>", key);
		if (c.split_exp < 0 || c.split_exp > log_alpha_size || c.msb < 0 || c.msb > c.split_exp || c.lsb < 0 || c.lsb > c.split_exp - c.msb) dief("modular: %s: split_exp <= %d, msb <= split_exp, lsb <= split_exp - msb", key, log_alpha_size);
		if (c.split_exp == log_alpha_size && (c.msb || c.lsb)) dief("modular: %s: split_exp == %d leaves msb and lsb uncoded (0)", key, log_alpha_size);
		return c;
	};
	const int lz_min_length = opt.geti("lzminlen", 3), lz_min_symbol = opt.geti("lzminsym", 224);
	if (lz_min_length < 3 || lz_min_length > 264) die("modular: lzminlen 3..264 (U32(3, 4, 5 + u(2), 9 + u(8)))");
	if (lz_min_symbol != 224 && lz_min_symbol != 512 && lz_min_symbol != 4096 && (lz_min_symbol < 8 || lz_min_symbol >= 8 + 32768)) die("modular: lzminsym 224, 512, 4096 or 8 + u(15)");
	if (!use_prefix && lz77 && lz_min_symbol >= 256) die("modular: rANS alphabets end at 256 here: lzminsym >= 256 wants prefix=1");
	// wp=random|max|zero|<eleven numbers>: weighted-predictor parameters other than the defaults; wpat=global (the global Modular header:
	// what LfGlobal codes, and a global palette's prediction), group (every pass-group header, the same values) or both (the global
	// header, and in every pass-group header values of its own derived from the group's index)
	WPParams wp_base;
	const bool custom_wp = parse_wp(opt, seed, wp_base, "modular");
	const std::string wpat = opt.gets("wpat", "global");
	if (custom_wp) {
		if (wpat != "global" && wpat != "group" && wpat != "both") die("modular: wpat=global|group|both");
		if (opt.geti("squeeze", 0)) die("modular: wp does not combine with squeeze (the sections' headers are shared there)");
	} else if (opt.kv.count("wpat")) die("modular: wpat places the parameters wp= gives");
	// repeat=K: the frame is the (W/K) x (H/K) picture tiled K x K times. Only the base picture is synthesised and encoded; its
	// group sections are reused (no tree here looks at the stream index), which makes 16384 x 16384 streams cheap to write
	const int num_passes = opt.geti("passes", 1);
	const int repeat = opt.geti("repeat", 1);
	if (repeat > 1 && num_passes > 1) die("repeat and passes do not combine");
	if (repeat > 1 && (lzp.mode != LZ_RUNS || lzp.force != FORCE_NONE)) die("modular: lzmode / lzforce do not combine with repeat (the base picture's sections would be written for a narrower frame's distance multiplier)");
	// squeeze=1: a Squeeze transform with the default parameter list behind the RCT (the "progressive" lossless form); 2: the same list
	// written out explicitly; 3: a short explicit list with residual channels appended (not in place) and partial channel ranges.
	// Squeeze couples neighbouring groups, so with repeat=K the base picture is tiled first and the whole frame is transformed;
	// group sections with identical content (most of them, the picture being periodic) are encoded once and shared.
	const int squeeze = opt.geti("squeeze", 0);
	if (squeeze && (num_passes > 1 || opt.geti("palette", 0) || opt.geti("localrct", -1) >= 0 || opt.geti("localpalette", 0) || opt.geti("localtree", 0))) die("squeeze combines with rct / tree / prefix / lz77 / alpha / extra / bpp / repeat only");
	const int Wfull = W, Hfull = H;
	const int tile_w = W / repeat, tile_h = H / repeat;   // the picture that is synthesised
	if (repeat > 1 && squeeze) {
		if (W % repeat || H % repeat) die("repeat: the frame must be whole tiles");
	} else if (repeat > 1) {
		if (W % (repeat * gdim) || H % (repeat * gdim)) die("repeat: the base picture must be whole groups");
		W /= repeat; H /= repeat;
		if (W == gdim && H == gdim) die("repeat: the base picture must have more than one group");
	}
	const int gcols = (W + gdim - 1) / gdim, grows = (H + gdim - 1) / gdim, num_groups = gcols * grows;
	const int num_lf_groups = ((W + 8 * gdim - 1) / (8 * gdim)) * ((H + 8 * gdim - 1) / (8 * gdim));
	const bool single = num_groups == 1;
	if (custom_wp && single && wpat != "global") die("modular: a frame of one group has no pass-group headers: wpat=global");
	if (single && opt.geti("passes", 1) > 1) die("modular: one group with several passes is not generated (the frame would not be a single section)");
	// extra=K: K more extra channels (type depth, same bit depth) ahead of the alpha channel, so that alpha is not the first one
	const int extra = opt.geti("extra", 0);
	if (extra < 0 || extra + (alpha ? 1 : 0) > 4) die("modular: at most four extra channels (j40.h:3247)");
	const int ncolour = 3, nch = ncolour + extra + (alpha ? 1 : 0);

	// ---- source picture -> channels: colour first, then extra channels (the renderer takes channels
	//      0..2 as RGB and 3.. as extra channels, j40.h:7923-7936) ----
	const int pic_w = squeeze ? tile_w : W, pic_h = squeeze ? tile_h : H;
	Picture pic(pic_w, pic_h, seed);
	std::vector<Channel> ch;
	for (int c = 0; c < nch; ++c) ch.emplace_back(pic_w, pic_h);
	const int colour0 = 0;               // index of the first colour channel
	// tile=px,py: the picture repeats with that period (matches in the same row, in rows above and diagonal ones), tilenoise=K per
	// mille of the samples differ from their tile's; noise=A adds uniform noise of that amplitude; range=lo,hi clamps the samples
	// there instead of to [0, 2^bpp) (samples the RCT has not been applied to may be anything in int16)
	int tile_px = 0, tile_py = 0;
	if (opt.kv.count("tile") && (sscanf(opt.gets("tile", "").c_str(), "%d,%d", &tile_px, &tile_py) != 2 || tile_px < 1 || tile_py < 1)) die("modular: tile=<px>,<py>");
	const int tile_noise = opt.geti("tilenoise", 20), noise = opt.geti("noise", 0);
	int range_lo = 0, range_hi = (1 << bpp) - 1;
	if (opt.kv.count("range") && (sscanf(opt.gets("range", "").c_str(), "%d,%d", &range_lo, &range_hi) != 2 || range_lo > range_hi || (!wide && (range_lo < -32768 || range_hi > 32767)))) die("modular: range=<lo>,<hi> within int16 (int32 with wide=1)");
	if (noise < 0 || noise > 65535) die("modular: noise 0..65535");
	for (int y = 0; y < pic_h; ++y) for (int x = 0; x < pic_w; ++x) {
		const int xs = tile_px ? x % tile_px : x, ys = tile_py ? y % tile_py : y;
		float rgb[3]; pic.rgb((float) xs, (float) ys, rgb);
		// flat regions + a bit of texture so that run-lengths and the predictors both get work
		for (int c = 0; c < 3; ++c) {
			int64_t v = (int) (rgb[c] * 255.0f);
			v = (v / 6) * 6 + (int) (Picture::hash01((uint64_t) xs * 7919 + (uint64_t) ys * 104729 + (uint64_t) c + seed) < 0.08f);
			v = std::min<int64_t>(255, std::max<int64_t>(0, v)) * ((1 << bpp) - 1) / 255;
			if (tile_px && Picture::hash01((uint64_t) x * 611953 + (uint64_t) y * 15485863 + (uint64_t) c * 31 + seed) * 1000.0f < (float) tile_noise) v ^= 1 + (int) (Picture::hash01((uint64_t) x * 31 + (uint64_t) y * 17 + seed) * 6.0f);
			if (noise) v += (int) (Picture::hash01((uint64_t) x * 2654435761ull + (uint64_t) y * 40503 + (uint64_t) c * 977 + seed * 13) * (float) (2 * noise + 1)) - noise;
			v += bias;
			if (tile_px || noise || opt.kv.count("range")) v = std::min<int64_t>(range_hi, std::max<int64_t>(range_lo, v));
			ch[(size_t) (colour0 + c)].at(x, y) = (int32_t) v;
		}
		for (int k = 0; k < extra; ++k) ch[(size_t) (3 + k)].at(x, y) = (((x >> 3) * (k + 2) + (y >> 2)) & 31) * ((1 << bpp) - 1) / 31;
		if (alpha) ch[(size_t) (3 + extra)].at(x, y) = ((x / 37 + y / 29) & 3) == 0 ? 128 + ((x * 3 + y) & 63) : 255;
		// alpharange=1: 0, full scale and everything between (a diagonal ramp with transparent and opaque cells), for the blend modes
		if (alpha && opt.geti("alpharange", 0)) { const int cell = (x / 23 + y / 19) % 5; ch[(size_t) (3 + extra)].at(x, y) = cell == 0 ? 0 : cell == 1 ? 255 : (x * 5 + y * 3) & 255; }
		// (wide=1, bpp != 8: the same alpha at the image's depth, its low bits filled so that the whole range occurs)
		if (deep_alpha) { int32_t &a = ch[(size_t) (3 + extra)].at(x, y); const int amax = (1 << bpp) - 1; a = a == 255 ? amax : a == 0 ? 0 : std::min(amax, a * amax / 255 + ((x * 7 + y * 13) & ((1 << (bpp - 8)) - 1))); }
	}

	// xyb=1: the image says xyb_encoded, and the three colour channels are read as quantised XYB -- c0 = Y / m[1], c1 = X / m[0],
	// c2 = B / m[2] - c0 with m = LfGlobal's LF dequantisation (the reference renders them as R, G, B all the same). By default the picture
	// above stands as it is, whatever colours that makes. xybpic=1: the procedural picture itself, through the VarDCT writer's forward
	// opsin (ForwardOpsin) and rounded to those integers: a lossy-Modular encode in miniature. dumprgb=PATH then writes the source picture,
	// float32 [height][width][3], sRGB samples in [0, 1]. lfdequant=a,b,c: m, other than the default 1/4096, 1/512, 1/256 (each times 128
	// must be a value an f16 holds).
	const int flag_xyb_image = opt.geti("xyb", 0), xybpic = opt.geti("xybpic", 0);
	double m_lf[3] = {1.0 / 4096, 1.0 / 512, 1.0 / 256};
	const bool custom_m_lf = opt.kv.count("lfdequant") != 0;
	if (custom_m_lf && (sscanf(opt.gets("lfdequant", "").c_str(), "%lf,%lf,%lf", &m_lf[0], &m_lf[1], &m_lf[2]) != 3 || !(m_lf[0] > 0 && m_lf[1] > 0 && m_lf[2] > 0))) die("modular: lfdequant=a,b,c, all positive");
	if ((xybpic || custom_m_lf) && !flag_xyb_image) die("modular: xybpic=1 and lfdequant= describe an XYB image: they want xyb=1");
	if (xybpic && (palette || squeeze || repeat > 1 || tile_px || noise || opt.kv.count("range") || opt.geti("fourvalues", 0) || bias)) die("modular: xybpic=1 codes the procedural picture itself: no palette, squeeze, repeat, tile, noise, range, fourvalues or bias");
	if (opt.kv.count("dumprgb") && !xybpic) die("modular: dumprgb= writes the picture xybpic=1 codes");
	if (xybpic) {
		const ForwardOpsin to_xyb;
		std::vector<float> source;
		for (int y = 0; y < pic_h; ++y) for (int x = 0; x < pic_w; ++x) {
			float rgb[3]; double xyb[3];
			pic.rgb((float) x, (float) y, rgb);
			for (int c = 0; c < 3; ++c) { rgb[c] = std::min(1.0f, std::max(0.0f, rgb[c])); source.push_back(rgb[c]); }
			to_xyb(rgb, xyb);
			const int32_t c0 = (int32_t) lrint(xyb[1] / m_lf[1]);
			ch[(size_t) colour0].at(x, y) = c0;
			ch[(size_t) colour0 + 1].at(x, y) = (int32_t) lrint(xyb[0] / m_lf[0]);
			ch[(size_t) colour0 + 2].at(x, y) = (int32_t) lrint(xyb[2] / m_lf[2]) - c0;
			if (!wide) for (int c = 0; c < 3; ++c) if (ch[(size_t) colour0 + (size_t) c].at(x, y) < -32768 || ch[(size_t) colour0 + (size_t) c].at(x, y) > 32767) die("modular: xybpic=1: a quantised sample leaves int16 (a coarser lfdequant=, or wide=1)");
		}
		if (opt.kv.count("dumprgb")) {
			FILE *fp = fopen(opt.gets("dumprgb", "").c_str(), "wb");
			if (!fp || fwrite(source.data(), 4, source.size(), fp) != source.size()) die("cannot write dumprgb");
			fclose(fp);
		}
	}
	// (lfmodular=1 of lflevels=: the planes run_lf_sequence hands over, each cell over 8 x 8 samples)
	if (g_mod_lf) {
		if (!flag_xyb_image || palette || squeeze || repeat > 1 || alpha || extra || wide || !g_seq) die("modular: an LF frame is written by lflevels= lfmodular=1 only");
		for (int c = 0; c < 3; ++c) for (int y = 0; y < pic_h; ++y) for (int x = 0; x < pic_w; ++x) ch[(size_t) colour0 + (size_t) c].at(x, y) = g_mod_lf->src[c][(size_t) (y / 8) * (size_t) g_mod_lf->src_w + (size_t) (x / 8)];
	}

	if (squeeze && repeat > 1) {   // lay the tile out over the whole frame
		for (Channel &c : ch) {
			Channel full(W, H);
			for (int y = 0; y < H; ++y) for (int x0 = 0; x0 < W; x0 += tile_w) memcpy(&full.at(x0, y), &c.at(0, y % tile_h), sizeof(int32_t) * (size_t) tile_w);
			c = std::move(full);
		}
	}

	// fourvalues=1: samples take four values only; with the zero predictor (tree=4) and no RCT every residual token is one of four
	// symbols, which makes prefix-coded streams use the NSYM = 4 simple code (simple4=1|2 chooses its tree-select-0 form)
	if (opt.geti("fourvalues", 0)) for (Channel &c : ch) for (int y = 0; y < c.h; ++y) for (int x = 0; x < c.w; ++x) {
		const float r = Picture::hash01((uint64_t) x * 7919 + (uint64_t) y * 104729 + seed);
		c.at(x, y) = r < 0.55f ? 0 : r < 0.8f ? 1 : r < 0.93f ? 2 : 3;
	}
	simple4_mode() = opt.geti("simple4", 0);

	// ---- global transforms (coded order = forward order; the decoder undoes them last to first) ----
	// dpred=0..13: the predictor of a palette's delta entries (palette=3 / localpalette=3; 6 is the weighted one, with the parameters
	// of the header that lists the palette)
	const int dpred = opt.geti("dpred", 5);
	if (dpred < 0 || dpred > 13) die("modular: dpred 0..13");
	if (opt.kv.count("dpred") && palette != 3 && opt.geti("localpalette", 0) != 3) die("modular: dpred belongs to a palette with delta entries (palette=3 or localpalette=3)");
	// dumpsrc=PATH: the picture the stream codes, raw little-endian int32 [channels][height][width], colour first, then the extra
	// channels. Where the writer runs a forward transform for everything it lists and no leaf quantises (`src_exact`), that is the source
	// picture as synthesised above, and the tool dies unless its own inverses (jxlsynth_modular.hpp, 64-bit) take what it coded back
	// to it -- a forward transform that is wrong at 18 bits cannot go unnoticed. Elsewhere -- a palette, whose picture IS the look-up;
	// the RCT types the picture is taken as already transformed for; trees whose leaves have multipliers -- there is no source to
	// return to, and the dump is what a reader must arrive at: the same inverses on what was coded (Squeeze is exact either way)
	const std::string dumpsrc = opt.gets("dumpsrc", "");
	const bool want_src = !dumpsrc.empty();
	if (want_src && (opt.geti("povf", -1) >= 0 || lzp.force != FORCE_NONE || g_seq)) die("modular: dumpsrc wants a stream that codes a picture: no povf, lzforce or frames=");
	std::vector<Channel> orig;
	if (want_src) orig = ch;
	bool src_exact = !palette && !(rct >= 0 && !(rct / 7 == 0 && rct % 7 != 2)) && !opt.geti("localpalette", 0) && tree_kind != 6 && tree_kind != 7 && tree_kind != 8 && !opt.geti("fourvalues", 0);
	std::vector<TransformW> transforms;
	if (palette) {
		// replace the colour channels by a palette (meta channel 0) + an index channel
		const int nb_colours = palette == 2 ? 24 : 40;
		const int nb_deltas = palette == 3 ? 6 : 0;
		Channel pal(nb_colours, 3), idx(W, H);
		for (int i = 0; i < nb_colours; ++i) for (int c = 0; c < 3; ++c) pal.at(i, c) = i < nb_deltas ? (int32_t) rng.below(9) - 4 : (int32_t) rng.below(256);
		for (int y = 0; y < H; ++y) for (int x = 0; x < W; ++x) {
			int v = (ch[(size_t) colour0].at(x, y) * 3 + ch[(size_t) colour0 + 1].at(x, y) * 5 + ch[(size_t) colour0 + 2].at(x, y)) / 9;
			int i = (v * nb_colours) >> 8;
			if (palette == 2) { if (((x ^ y) & 31) == 5) i = -1 - (int) rng.below(140); else if (((x + 2 * y) & 63) == 9) i = nb_colours + (int) rng.below(64 + 125); }
			idx.at(x, y) = i;
		}
		std::vector<Channel> next;
		next.push_back(pal);
		next.push_back(idx);
		for (int c = 3; c < nch; ++c) next.push_back(ch[(size_t) c]);
		ch.swap(next);
		TransformW t; t.kind = 1; t.begin_c = colour0; t.num_c = 3; t.nb_colours = nb_colours; t.nb_deltas = nb_deltas; t.d_pred = palette == 3 ? dpred : 0;
		transforms.push_back(t);
	} else if (rct >= 0) {
		if (rct / 7 == 0 && rct % 7 != 2) forward_rct(ch, colour0, rct);   // other types: the picture is taken as already transformed
		TransformW t; t.kind = 0; t.begin_c = colour0; t.rct_type = rct;
		transforms.push_back(t);
	}
	const int nb_meta = palette ? 1 : 0;
	std::vector<Channel> dec;   // what a reader holds once every section is decoded and pasted, before it undoes the global RCT / palette
	if (want_src) dec = ch;
	if (squeeze) {
		TransformW t; t.kind = 2;
		std::vector<SqueezeStep> steps = default_squeeze_steps(ch, nb_meta);
		if (squeeze == 3) {
			steps.clear();
			SqueezeStep a; a.horizontal = true; a.in_place = true; a.begin_c = 0; a.num_c = 3; steps.push_back(a);
			a.horizontal = false; steps.push_back(a);
			a.horizontal = true; a.in_place = false; a.begin_c = 1; a.num_c = 2; steps.push_back(a);
			a.horizontal = false; a.in_place = true; a.begin_c = 0; a.num_c = 1; steps.push_back(a);
			a.horizontal = false; a.in_place = false; a.begin_c = 0; a.num_c = (int) ch.size() >= 4 ? 4 : 3; steps.push_back(a);   // (with alpha: reaches into the residuals / the alpha channel)
		}
		if (squeeze >= 2) t.sq = steps;
		for (const SqueezeStep &st : steps) forward_squeeze_step(ch, st);
		transforms.push_back(t);
	}
	const int total_ch = (int) ch.size();

	// ---- MA tree ----
	MATree tree;
	{
		int root;
		if (tree_kind == 0) root = tree.leaf(5);
		else if (tree_kind == 4) root = tree.leaf(0);   // the zero predictor: residual = sample
		else if (tree_kind == 1) {
			int l0 = tree.leaf(5), l1 = tree.leaf(4), l2 = tree.leaf(13), l3 = tree.leaf(1), l4 = tree.leaf(2, 0, 0, 0), l5 = tree.leaf(12), l6 = tree.leaf(7), l7 = tree.leaf(3);
			int a = tree.branch(9, 100, l0, l1);      // W + N - NW
			int b = tree.branch(4, 40, l2, l3);       // |N|
			int c = tree.branch(12, -3, l4, l5);      // N - NE
			int d = tree.branch(3, 7, l6, l7);        // x
			int e = tree.branch(0, 1, a, b);          // channel index
			int f = tree.branch(2, 5, c, d);          // y
			root = tree.branch(10, 0, e, f);          // W - NW
		} else if (tree_kind == 2) {
			int l0 = tree.leaf(6), l1 = tree.leaf(6), l2 = tree.leaf(5), l3 = tree.leaf(6);
			int a = tree.branch(15, 8, l0, l1);       // max weighted-predictor error
			int b = tree.branch(15, -8, l2, l3);
			root = tree.branch(0, 1, a, b);
		} else if (tree_kind == 8) {
			// the first sample of every channel of a section takes a leaf of its own -- zero predictor, multiplier 65536 --, the others the
			// gradient: a picture far from zero (wide=1 with bias=) is coded with small residuals, where one leaf would need a first
			// residual beyond the 30 bits a hybrid integer holds. That first sample is quantised to a multiple of 65536
			int first = tree.leaf(0, 0, 16, 0), l0 = tree.leaf(5), l1 = tree.leaf(5);
			int a = tree.branch(2, 0, l0, first);     // y
			root = tree.branch(3, 0, l1, a);          // x
		} else if (tree_kind == 6 || tree_kind == 7) {
			// lossy-Modular style leaves: multipliers 37 and 1000, offsets +-500. 6 walks a sample's position only (the two-pass decoder's
			// kind of tree, the leaf changing along a row), 7 looks at neighbours as well
			int l0 = tree.leaf(5, 500, 0, 36), l1 = tree.leaf(1, -500, 3, 124), l2 = tree.leaf(2, 0, 0, 36), l3 = tree.leaf(13, -3, 1, 0), l4 = tree.leaf(4, 250, 0, 36);
			int a = tree.branch(3, 40, l0, l1);                                        // x
			int b = tree.branch(tree_kind == 6 ? 2 : 5, 33, l2, l3);                   // y / |W|
			int c = tree.branch(tree_kind == 6 ? 3 : 9, tree_kind == 6 ? 9 : 120, b, l4);   // x / W + N - NW
			root = tree.branch(0, 0, a, c);                                            // channel index
		} else if (tree_kind == 5) {
			// a wide tree: every property 0..14, every predictor but the weighted one, offsets and multipliers; 48 leaves
			static const int PREDS[13] = {5, 1, 2, 3, 4, 0, 7, 8, 9, 10, 11, 12, 13};
			static const int THR[15] = {1, 2, 60, 90, 30, 25, 110, 130, 2, 120, -1, 3, -4, 5, -2};
			uint32_t r = 12345u; int leaves = 0, splits = 0;
			std::function<int(int)> grow = [&](int depth) -> int {
				r = r * 1664525u + 1013904223u;
				if (depth == 0 || (depth < 4 && ((r >> 9) & 3) == 0)) {
					const int k = leaves++;
					return tree.leaf(PREDS[k % 13], (k % 5) - 2, k % 7 == 3 ? 1 : 0, k % 11 == 5 ? 2 : 0);
				}
				const int prop = splits++ % 15;
				const int thr = THR[prop] + (int) ((r >> 12) % 7) - 3;
				const int left = grow(depth - 1), right = grow(depth - 1);
				return tree.branch(prop, thr, left, right);
			};
			root = grow(6);
			while (leaves > 64) die("tree=5 grew past 64 leaves");
		} else {
			int l0 = tree.leaf(5), l1 = tree.leaf(5), l2 = tree.leaf(1), l3 = tree.leaf(2), l4 = tree.leaf(5);
			int a = tree.branch(16, 10, l0, l1);      // previous channel sample
			int b = tree.branch(19, 4, l2, l3);       // |previous channel sample - its gradient|
			int c = tree.branch(17, 60, a, b);        // |previous channel sample|
			root = tree.branch(0, 0, c, l4);          // channel 0 has no previous channel
		}
		tree.finalise(root);
	}
	CodeSpecW treespec; treespec.init(6, std::vector<uint8_t>(6, 0), 1); treespec.log_alpha = 6; treespec.cfg[0] = HybridCfg{4, 1, 0};
	StreamEncoder tree_enc(treespec); tree_tokens(tree, tree_enc); count_stream(treespec, tree_enc);

	auto make_spec = [&](const MATree &t) {
		CodeSpecW sp;
		const int nctx = t.num_ctx;
		std::vector<uint8_t> map((size_t) (nctx + (lz77 ? 1 : 0)));
		const int ncl = std::min(nctx, 3);
		for (int i = 0; i < nctx; ++i) map[(size_t) i] = (uint8_t) (i % ncl);
		int nclusters = ncl;
		if (lz77) { map[(size_t) nctx] = (uint8_t) ncl; nclusters = ncl + 1; }   // the distance context gets its own cluster
		sp.lz77 = lz77 != 0;
		sp.init(nctx, map, nclusters);
		sp.lz_min_symbol = lz_min_symbol; sp.lz_min_length = lz_min_length; sp.lz_len_cfg = parse_cfg("lzlencfg", HybridCfg{0, 0, 0}, 8);
		sp.use_prefix = use_prefix != 0; sp.log_alpha = 8;
		for (auto &c : sp.cfg) c = parse_cfg("hybrid", use_prefix ? HybridCfg{4, 2, 0} : HybridCfg{4, 1, 1}, use_prefix ? 15 : 8);
		if (lz77) sp.cfg[(size_t) ncl] = parse_cfg("lzdistcfg", sp.cfg[(size_t) ncl], use_prefix ? 15 : 8);
		return sp;
	};
	CodeSpecW gspec = make_spec(tree);
	// localtree=1: every other group section repeats the global MA tree with its own code spec
	// (use_global_tree = 0, j40.h:3740); localtree=2: those sections use a different tree, one that
	// needs the weighted predictor whatever the global tree does
	const int local_tree = opt.geti("localtree", 0);
	MATree ltree = tree;
	if (local_tree == 2) {
		ltree = MATree();
		int l0 = ltree.leaf(6), l1 = ltree.leaf(5), l2 = ltree.leaf(4), l3 = ltree.leaf(1, 2, 0, 0);
		int a = ltree.branch(15, 8, l0, l1);      // max weighted-predictor error
		int b = ltree.branch(3, 100, l2, l3);     // x
		ltree.finalise(ltree.branch(2, 17, a, b)); // y
	}
	StreamEncoder ltree_enc(treespec);
	if (local_tree) { tree_tokens(ltree, ltree_enc); count_stream(treespec, ltree_enc); }
	const StreamEncoder ltree_saved = ltree_enc;   // flush() consumes the items
	const CodeSpecW lspec_proto = make_spec(ltree);
	// the parameters of the header a section reads: LfGlobal's is the global one, a pass group's its own
	const WPParams wp_default;
	auto group_wp = [&](int g) {
		return wpat == "both" ? wp_derived(wp_base, g) : wp_base;
	};
	const WPParams *global_wp = custom_wp && wpat != "group" ? &wp_base : nullptr;
	const bool groups_have_wp = custom_wp && wpat != "global";
	const CodeSpecW &gspec_ref = gspec;
	LzStats lzstats;
	// povf=K: sample K of every section (decode order) is coded beyond int16, as povfto= (default 40000; up to +-2^30: a residual of
	// thirty bits); povfsection=N: only in the N-th stream the writer codes (from 0; default: every stream)
	const int povf_all = opt.geti("povf", -1);
	const bool povf_everywhere = !opt.kv.count("povfsection");
	int povf_section = opt.geti("povfsection", 0), coded_streams = 0;
	const int64_t povf_to = strtoll(opt.gets("povfto", wide ? "2147483648" : "40000").c_str(), nullptr, 10);
	if (povf_to >= sample_lo() && povf_to <= sample_hi()) die("modular: povfto lies outside int16 (outside int32 with wide=1)");
	if (!wide && (povf_to < -(1 << 30) || povf_to > (1 << 30))) die("modular: povfto within +-2^30 (the residual is a 32-bit hybrid integer)");
	if (wide && (povf_to < -((int64_t) 1 << 32) || povf_to > ((int64_t) 1 << 32))) die("modular: povfto within +-2^32");
	if (povf_all >= 0 && lzp.force != FORCE_NONE) die("modular: povf works on a coded picture, lzforce has none");

	// encodes the listed channels (sub-rectangles already cut out) into one stream; LZ77 replaces runs
	// of equal tokens ("previous symbol" = distance code 1 with a non-zero dist_mult, j40.h:2834)
	auto encode_image = [&](std::vector<Channel> &chs, int first, int64_t sidx, StreamEncoder &enc, bool local = false, const WPParams *wpp_in = nullptr, int64_t dist_mult = 0) {
		const WPParams &wpp = wpp_in ? *wpp_in : wp_default;
		const int povf = povf_everywhere || coded_streams++ == povf_section ? povf_all : -1;
		const MATree &use_tree = local ? ltree : tree;
		const CodeSpecW &gspec = local ? lspec_proto : gspec_ref;   // same cluster layout rules, the section's own contexts
		StreamEncoder raw(gspec);
		std::vector<Tok> src;
		if (lz77 && lzp.mode != LZ_RUNS) raw.src = &src;
		if (lz77 && (lzp.mode != LZ_RUNS || lzp.force != FORCE_NONE)) {
			// where each integer lies; `dist_mult`: the reader's multiplier, the widest channel behind the meta channels of the image the
			// header describes -- the WHOLE frame's where this is LfGlobal's stream, the section's own otherwise (j40.h:3840-3844)
			std::vector<uint32_t> row_of, chan_of;
			uint32_t row = 0;
			LzParams lp = lzp;
			for (int c = first; c < (int) chs.size(); ++c) {
				for (int y = 0; y < chs[(size_t) c].h; ++y, ++row) for (int x = 0; x < chs[(size_t) c].w; ++x) { row_of.push_back(row); chan_of.push_back((uint32_t) c); }
			}
			lp.dist_mult = dist_mult;
			if (row_of.empty()) return;
			if (dist_mult <= 0) die("modular: lzmode / lzforce: this stream's distance multiplier is not known to the writer");
			if (lzp.force != FORCE_NONE) {
				const std::vector<uint32_t> win = lz77_forced(enc, gspec, lp, 0, row_of.size(), rng, row_of, chan_of, lzstats);
				size_t k = 0;
				for (int c = first; c < (int) chs.size(); ++c) for (int32_t &v : chs[(size_t) c].px) { const uint32_t u = win[k++]; v = (u & 1) ? -(int32_t) ((u + 1) >> 1) : (int32_t) (u >> 1); }
				return;
			}
			int64_t povf_in = povf;
			for (int c = first; c < (int) chs.size(); ++c) encode_channel(use_tree, chs, c, sidx, wpp, raw, povf >= 0 ? &povf_in : nullptr, povf_to);
			std::vector<uint32_t> ctxs, vals;
			for (const Tok &t : src) { ctxs.push_back(t.ctx); vals.push_back(t.value); }
			lz77_match(enc, gspec, lp, ctxs, vals, row_of, chan_of, lzstats);
			return;
		}
		{ int64_t povf_in = povf; for (int c = first; c < (int) chs.size(); ++c) encode_channel(use_tree, chs, c, sidx, wpp, raw, povf >= 0 ? &povf_in : nullptr, povf_to); }
		if (!lz77) { enc.items = raw.items; if (povf >= 0 && (size_t) povf < enc.items.size()) enc.mark_item = (size_t) povf; return; }
		// run-length pass over the residual tokens: a run of >= 3 identical (cluster, token, extra) items
		// after its first occurrence becomes one copy with distance 1
		const auto &it = raw.items;
		for (size_t i = 0; i < it.size(); ) {
			size_t j = i + 1;
			while (j < it.size() && it[j].token == it[i].token && it[j].extra == it[i].extra && it[i].nextra == 0 && it[j].nextra == 0 && it[i].token < 16) ++j;
			enc.items.push_back(it[i]);
			size_t run = j - i - 1;
			if (run >= 3 && it[i].token < 16) {
				// the copied *values* are hybrid-decoded integers; with split_exp 4 a token < 16 is its own value
				uint32_t cl = it[i + 1].cluster;
				HToken t = hybrid_encode((uint32_t) run - (uint32_t) gspec.lz_min_length, gspec.lz_len_cfg);
				enc.items.push_back({cl, t.token + (uint32_t) gspec.lz_min_symbol, t.extra, (uint8_t) t.nextra});
				uint32_t lzcl = gspec.cluster_map[(size_t) gspec.total_dist() - 1];
				HToken d = hybrid_encode(1, gspec.cfg[lzcl]);   // special distance code 1 = previous symbol
				enc.items.push_back({lzcl, d.token, d.extra, (uint8_t) d.nextra});
				++lzstats.copies; ++lzstats.special_copies; ++lzstats.distance_one; lzstats.code_seen[1] = true; lzstats.max_length = std::max<uint64_t>(lzstats.max_length, run);
				i = j;
			} else i = i + 1;
		}
	};

	std::vector<StreamEncoder> encs;
	bool samples_known = !palette && !squeeze && povf_all < 0;   // (stats: `ch` ends up holding what a reader decodes, before the global RCT is undone)
	std::vector<std::vector<TransformW>> group_tr;
	const int local_rct = opt.geti("localrct", -1);
	const int local_palette = opt.geti("localpalette", 0);
	std::vector<uint8_t> section_is_group;
	// squeeze, frames larger than a group: which encoder (index into encs) holds each LfGroup / pass-group section; -1 = nothing coded there
	std::vector<int> sq_lf_enc, sq_group_enc;
	int64_t frame_dist_mult = 0;
	for (int c = nb_meta; c < total_ch; ++c) frame_dist_mult = std::max<int64_t>(frame_dist_mult, ch[(size_t) c].w);
	if (single) {
		encs.emplace_back(gspec);
		encode_image(ch, 0, 0, encs.back(), false, global_wp, frame_dist_mult);
		if (want_src && !squeeze) dec = ch;   // (what was coded: a leaf with a multiplier quantises)
	} else if (squeeze) {
		// The decoder deals the channels out by size and shift (ISO 18181-1): LfGlobal takes the meta channels and the channels behind
		// them that fit one group; an LfGroup section the channels shifted by >= 3 both ways, over its 8-groups-wide area; a pass-group
		// section the others over its own area. A channel's rectangle is the area shifted down, clipped to the channel.
		int num_gm = nb_meta;
		while (num_gm < total_ch && ch[(size_t) num_gm].w <= gdim && ch[(size_t) num_gm].h <= gdim) ++num_gm;
		encs.emplace_back(gspec);
		{ std::vector<Channel> head(ch.begin(), ch.begin() + num_gm); if (num_gm) encode_image(head, 0, 0, encs.back(), false, nullptr, frame_dist_mult); }
		std::map<uint64_t, int> seen;   // content hash of a section's channels -> its encoder
		auto cut = [&](bool lf, int left, int top, int dim, int64_t sidx) -> int {
			std::vector<Channel> sub;
			uint64_t hsh = 1469598103934665603ull;
			auto mix = [&](uint64_t v) { hsh = (hsh ^ v) * 1099511628211ull; };
			for (int c = num_gm; c < total_ch; ++c) {
				const Channel &full = ch[(size_t) c];
				if ((full.hshift >= 3 && full.vshift >= 3) != lf) continue;
				const int x0 = left >> full.hshift, y0 = top >> full.vshift, w = std::min(dim >> full.hshift, full.w - x0), h = std::min(dim >> full.vshift, full.h - y0);
				if (w <= 0 || h <= 0) continue;
				Channel s2(w, h); s2.hshift = full.hshift; s2.vshift = full.vshift;
				for (int y = 0; y < h; ++y) memcpy(&s2.at(0, y), full.px.data() + (size_t) (y0 + y) * (size_t) full.w + (size_t) x0, sizeof(int32_t) * (size_t) w);
				mix((uint64_t) w << 32 | (uint32_t) h); mix((uint64_t) full.hshift << 8 | (uint64_t) full.vshift);
				for (int32_t v : s2.px) mix((uint32_t) v);
				sub.push_back(std::move(s2));
			}
			if (sub.empty()) return -1;
			auto it = seen.find(hsh);
			if (it != seen.end()) return it->second;
			encs.emplace_back(gspec);
			{ int64_t widest = 0; for (const Channel &s2 : sub) widest = std::max<int64_t>(widest, s2.w); encode_image(sub, 0, sidx, encs.back(), false, nullptr, widest); }
			seen[hsh] = (int) encs.size() - 1;
			return (int) encs.size() - 1;
		};
		const int lfdim = gdim * 8, lfcols = (W + lfdim - 1) / lfdim;
		for (int gg = 0; gg < num_lf_groups; ++gg) sq_lf_enc.push_back(cut(true, (gg % lfcols) * lfdim, (gg / lfcols) * lfdim, lfdim, 1 + num_lf_groups + gg));
		for (int g = 0; g < num_groups; ++g) sq_group_enc.push_back(cut(false, (g % gcols) * gdim, (g / gcols) * gdim, gdim, 1 + 3 * num_lf_groups + 17 + g));
	} else {
		// meta channels (palette) are decoded inside LfGlobal (num_gm_channels = nb_meta_channels, j40.h:6332)
		encs.emplace_back(gspec);
		if (nb_meta) { std::vector<Channel> meta(ch.begin(), ch.begin() + nb_meta); encode_image(meta, 0, 0, encs.back(), false, global_wp, frame_dist_mult); if (want_src) for (int c = 0; c < nb_meta; ++c) dec[(size_t) c] = meta[(size_t) c]; }
		// passes=P: every pass codes the whole group again (the reference decodes and pastes all channels in each pass,
		// j40.h:7025-7033, so the last pass is what stays); earlier passes carry a perturbed picture
		for (int pass = 0; pass < num_passes; ++pass) for (int g = 0; g < num_groups; ++g) {
			const int gx = (g % gcols) * gdim, gy = (g / gcols) * gdim, gw = std::min(gdim, W - gx), gh = std::min(gdim, H - gy);
			std::vector<Channel> sub;
			for (int c = nb_meta; c < total_ch; ++c) {
				Channel s2(gw, gh);
				for (int y = 0; y < gh; ++y) for (int x = 0; x < gw; ++x) s2.at(x, y) = ch[(size_t) c].at(gx + x, gy + y) ^ (pass + 1 < num_passes ? ((x + 2 * y + pass) & 3) : 0);
				sub.push_back(s2);
			}
			const bool local = local_tree && (((size_t) (pass * num_groups + g) + 1) & 1);
			// localrct=K: the group's header lists one or two RCTs of its own (j40.h:3757-3773), type varying by group
			group_tr.emplace_back();
			// localpalette=K (1 plain, 2 with deltas and synthetic colours, 3 with delta prediction): every other group replaces its
			// three colour channels by a palette of its own + an index channel (j40.h:3774-3799); those groups list no RCT
			const bool own_palette = local_palette && sub.size() >= 3 && ((g + pass) & 1) == 0;
			if (own_palette) {
				const int nb_colours = local_palette == 2 ? 20 : 33, nb_deltas = local_palette == 3 ? 5 : 0;
				Channel pal(nb_colours, 3), idx(gw, gh);
				for (int i = 0; i < nb_colours; ++i) for (int c = 0; c < 3; ++c) pal.at(i, c) = i < nb_deltas ? (int32_t) rng.below(9) - 4 : (int32_t) rng.below(256);
				for (int y = 0; y < gh; ++y) for (int x = 0; x < gw; ++x) {
					int v = (sub[0].at(x, y) * 3 + sub[1].at(x, y) * 5 + sub[2].at(x, y)) / 9;
					int i = ((v & 255) * nb_colours) >> 8;
					if (local_palette == 2) { if (((x ^ y) & 31) == 5) i = -1 - (int) rng.below(140); else if (((x + 2 * y) & 63) == 9) i = nb_colours + (int) rng.below(64 + 125); }
					idx.at(x, y) = i;
				}
				std::vector<Channel> next{pal, idx};
				for (size_t c = 3; c < sub.size(); ++c) next.push_back(sub[c]);
				sub.swap(next);
				TransformW t; t.kind = 1; t.begin_c = 0; t.num_c = 3; t.nb_colours = nb_colours; t.nb_deltas = nb_deltas; t.d_pred = local_palette == 3 ? dpred : 0;
				group_tr.back().push_back(t);
			}
			if (local_rct >= 0 && sub.size() >= 3 && !own_palette) {
				const int t1 = (local_rct + 5 * (g + pass)) % 42, t2 = (3 * t1 + 1) % 42;
				TransformW a; a.kind = 0; a.begin_c = 0; a.rct_type = t1; group_tr.back().push_back(a);
				if (t1 / 7 == 0 && t1 % 7 != 2) forward_rct(sub, 0, t1); else src_exact = false;
				if (g % 3 == 2) {
					TransformW b; b.kind = 0; b.begin_c = (int) sub.size() - 3; b.rct_type = t2; group_tr.back().push_back(b);
					if (t2 / 7 == 0 && t2 % 7 != 2) forward_rct(sub, b.begin_c, t2); else src_exact = false;
				}
			}
			if (group_tr.back().size()) samples_known = false;
			encs.emplace_back(gspec);
			// stream index of a pass group (j40.h:7013): 1 + 3 * num_lf_groups + 17 + pass * num_groups + gidx
			const WPParams gwp = group_wp(pass * num_groups + g);
			encode_image(sub, 0, 1 + 3 * num_lf_groups + 17 + pass * num_groups + g, encs.back(), local, groups_have_wp ? &gwp : nullptr, gw);
			if (want_src && pass + 1 == num_passes) {   // the group as a reader has it once its own transforms are undone, last to first
				std::vector<Channel> got = sub;
				for (size_t k = group_tr.back().size(); k-- > 0; ) {
					const TransformW &t = group_tr.back()[k];
					if (t.kind == 1) expect_inverse_palette(got, t.num_c, t.nb_colours, t.nb_deltas, t.d_pred, bpp, groups_have_wp ? gwp : wp_default);
					else expect_inverse_rct(got, t.begin_c, t.rct_type);
				}
				for (int c = nb_meta; c < total_ch; ++c) for (int y = 0; y < gh; ++y) memcpy(&dec[(size_t) c].at(gx, gy + y), &got[(size_t) (c - nb_meta)].at(0, y), sizeof(int32_t) * (size_t) gw);
			}
			if (samples_known && pass + 1 == num_passes) for (int c = nb_meta; c < total_ch; ++c) for (int y = 0; y < gh; ++y) for (int x = 0; x < gw; ++x) ch[(size_t) c].at(gx + x, gy + y) = sub[(size_t) (c - nb_meta)].at(x, y);
		}
	}
	if (want_src) {
		for (size_t k = transforms.size(); k-- > 0; ) {
			const TransformW &t = transforms[k];
			if (t.kind == 1) expect_inverse_palette(dec, t.num_c, t.nb_colours, t.nb_deltas, t.d_pred, bpp, global_wp ? *global_wp : wp_default);
			else if (t.kind == 0) expect_inverse_rct(dec, t.begin_c, t.rct_type);
		}
		if (src_exact) {
			if (orig.size() != dec.size()) die("modular: dumpsrc: the inverse transforms do not return the source picture's channels");
			for (size_t c = 0; c < orig.size(); ++c) if (orig[c].w != dec[c].w || orig[c].h != dec[c].h || orig[c].px != dec[c].px) die("modular: dumpsrc: the forward transforms do not invert to the source picture");
		}
		const std::vector<Channel> &dump = src_exact ? orig : dec;
		FILE *fp = fopen(dumpsrc.c_str(), "wb");
		if (!fp) die("cannot write dumpsrc");
		for (const Channel &c : dump) for (int y = 0; y < Hfull; ++y) for (int x0 = 0; x0 < Wfull; x0 += c.w)   // (repeat=K without squeeze: the base picture tiled)
			if (fwrite(&c.px[(size_t) (y % c.h) * (size_t) c.w], 4, (size_t) std::min(c.w, Wfull - x0), fp) != (size_t) std::min(c.w, Wfull - x0)) die("cannot write dumpsrc");
		fclose(fp);
	}
	std::vector<CodeSpecW> lspec(encs.size(), lspec_proto);
	for (size_t i = 0; i < encs.size(); ++i) {
		if (local_tree && !single && i >= 1 && (i & 1)) { encs[i].spec = &lspec[i]; count_stream(lspec[i], encs[i]); }
		else count_stream(gspec, encs[i]);
	}

	// ---- sections ----
	// (stats) the overflowing residual of povf= in streams without LZ77: section, first of its extra bits within it, their number, their value
	struct PovfMark { size_t section, bit, nbits; uint32_t extra; };
	std::vector<PovfMark> povf_marks;
	int longest_symbol_bits = 0;   // (stats) prefix codes: code length + extra bits of one token; rANS: the extra bits alone
	auto note_bits = [&](const StreamEncoder &e) {
		for (const auto &it : e.items) {
			int bits = it.nextra;
			if (e.spec->use_prefix && e.spec->pfx[it.cluster].alphabet > 1) bits += e.spec->pfx[it.cluster].len[it.token];
			longest_symbol_bits = std::max(longest_symbol_bits, bits);
		}
	};
	std::vector<std::vector<uint8_t>> sections;
	{
		BitWriter bw;
		write_patch_dictionary(bw, extra + (alpha ? 1 : 0));   // (patches=: the dictionary comes first)
		write_splines(bw);                                     // (splines=: behind it)
		write_noise_parameters(bw);                            // (noise=: behind them)
		if (!custom_m_lf) bw.put(1, 1);   // LF channel dequantisation: default
		else { bw.put(0, 1); for (int c = 0; c < 3; ++c) bw.f16((float) (m_lf[c] * 128.0)); }   // (read back divided by 128, j40.h:6268)
		bw.put(1, 1);                 // global tree present
		write_code_spec(bw, treespec); tree_enc.flush(bw);
		write_code_spec(bw, gspec);
		write_modular_header(bw, true, global_wp, transforms);
		note_bits(encs[0]);
		encs[0].flush(bw);
		if (encs[0].mark_nbits >= 0) povf_marks.push_back({0, encs[0].mark_bit, (size_t) encs[0].mark_nbits, encs[0].mark_extra});
		bw.pad();
		sections.push_back(bw.bytes);
	}
	const int gcols_full = (Wfull + gdim - 1) / gdim, grows_full = (Hfull + gdim - 1) / gdim;
	const int num_lf_groups_full = ((Wfull + 8 * gdim - 1) / (8 * gdim)) * ((Hfull + 8 * gdim - 1) / (8 * gdim));
	if (!single && squeeze) {
		std::vector<std::vector<uint8_t>> done(encs.size());   // a shared encoder is serialised once
		auto section_of = [&](int e) -> std::vector<uint8_t> {
			if (e < 0) return {};
			if (done[(size_t) e].empty()) {
				BitWriter bw;
				write_modular_header(bw, true, nullptr, {});
				note_bits(encs[(size_t) e]);
				encs[(size_t) e].flush(bw);
				bw.pad();
				done[(size_t) e] = bw.bytes;
			}
			return done[(size_t) e];
		};
		for (int e : sq_lf_enc) sections.push_back(section_of(e));
		sections.push_back({});       // HfGlobal: empty in Modular frames
		for (int e : sq_group_enc) sections.push_back(section_of(e));
	} else if (!single) {
		for (int i = 0; i < num_lf_groups_full; ++i) sections.push_back({});
		sections.push_back({});       // HfGlobal must be empty for Modular frames (j40.h:7825)
		for (int g = 0; g < num_passes * num_groups; ++g) {
			BitWriter bw;
			const WPParams gwp = group_wp(g);
			const WPParams *own_wp = groups_have_wp ? &gwp : nullptr;
			if (local_tree && (((size_t) g + 1) & 1)) {
				write_modular_header(bw, false, own_wp, group_tr[(size_t) g]);
				StreamEncoder te = ltree_saved;
				write_code_spec(bw, treespec); te.flush(bw);
				write_code_spec(bw, lspec[(size_t) g + 1]);
			} else write_modular_header(bw, true, own_wp, group_tr[(size_t) g]);
			note_bits(encs[(size_t) g + 1]);
			encs[(size_t) g + 1].flush(bw);
			if (encs[(size_t) g + 1].mark_nbits >= 0) povf_marks.push_back({sections.size(), encs[(size_t) g + 1].mark_bit, (size_t) encs[(size_t) g + 1].mark_nbits, encs[(size_t) g + 1].mark_extra});
			bw.pad();
			sections.push_back(bw.bytes);
		}
		if (repeat > 1) {   // lay the base picture's group sections out over the full frame
			const size_t first = sections.size() - (size_t) num_groups;
			std::vector<std::vector<uint8_t>> base(sections.begin() + (long) first, sections.end());
			sections.resize(first);
			for (int gy = 0; gy < grows_full; ++gy) for (int gx = 0; gx < gcols_full; ++gx) sections.push_back(base[(size_t) (gy % grows) * (size_t) gcols + (size_t) (gx % gcols)]);
		}
	}

	// ---- codestream ----
	BitWriter cs;
	if (g_seq && (opt.geti("icc", 0) || repeat > 1)) die("modular: frames= does not combine with icc or repeat");
	if (!g_seq || g_seq->first) {
	cs.put(0xff, 8); cs.put(0x0a, 8);
	write_size_header(cs, g_seq ? g_seq->canvas_w : up_flag() ? g_up.shown_w : Wfull, g_seq ? g_seq->canvas_h : up_flag() ? g_up.shown_h : Hfull);   // (upsampling=: the shown size)
	cs.put(0, 1);                       // ImageMetadata: not all_default
	write_extra_fields(cs);             // no extra fields (an animation: its header)
	write_bit_depth(cs, bpp);
	cs.put(wide ? 0 : 1, 1);            // modular_16bit_buffers (wide=1: 0, and nothing else differs)
	{   // num_extra_channels U32(0, 1, 2 + u(4), 1 + u(12)), then one ExtraChannelInfo each (j40.h:3247-3290)
		const int nec = extra + (alpha ? 1 : 0);
		if (nec == 0) cs.put(0, 2); else if (nec == 1) cs.put(1, 2); else { cs.put(2, 2); cs.put((uint64_t) (nec - 2), 4); }
		for (int k = 0; k < extra; ++k) {
			cs.put(0, 1);                   // not the default alpha
			cs.put(1, 2);                   // type: enum selector 1 = depth
			write_bit_depth(cs, bpp);
			cs.put(0, 2);                   // dim_shift 0
			cs.put(0, 2);                   // no name
		}
		if (alpha && !deep_alpha) cs.put(1, 1);   // d_alpha
		else if (alpha) {                   // (wide=1, bpp != 8: an alpha channel of the image's depth)
			cs.put(0, 1);
			cs.put(0, 2);                   // type: enum selector 0 = alpha
			write_bit_depth(cs, bpp);
			cs.put(0, 2);                   // dim_shift 0
			cs.put(0, 2);                   // no name
			cs.put(0, 1);                   // not associated
		}
	}
	// xyb=1 / ycbcr=1: the frame is flagged XYB / YCbCr; the reference applies no colour transform to Modular
	// frames (j40.h:8209-8210, 7910) and renders the three channels as they are
	cs.put(opt.geti("xyb", 0) ? 1 : 0, 1);   // xyb_encoded
	const int icc_bytes = opt.geti("icc", 0);
	if (opt.geti("grey", 0)) {
		// grey=1 (with xyb=1, no icc): the colour encoding says grey, D65, sRGB transfer, relative intent. An XYB image codes three
		// channels whatever its colour space (j40.h:3619), so the stream is a valid one -- of a grey image
		if (!opt.geti("xyb", 0) || icc_bytes) die("modular: grey=1 wants xyb=1 (three coded channels all the same) and no icc");
		cs.put(0, 1); cs.put(0, 1);     // ColourEncoding: not all_default, no ICC profile
		cs.put(1, 2);                   // colour_space = grey (enum value 1)
		cs.put(1, 2);                   // white_point = D65
		cs.put(0, 1);                   // no gamma
		cs.put(2, 2); cs.put(11, 4);    // transfer function 13 (sRGB): enum selector 2, 2 + 11
		cs.put(1, 2);                   // rendering intent 1
	} else
	if (!icc_bytes) { if (!write_colour_encoding(cs)) cs.put(1, 1); }   // ColourEncoding.all_default (sRGB; cenc=: written out)
	else { cs.put(0, 1); cs.put(1, 1); cs.put(0, 2); }   // want_icc, colour_space = RGB
	write_header_tail(cs, true, opt.geti("xyb", 0) != 0);   // (tone= / opsin=: with xyb=1 only, main() sees to it)
	if (icc_bytes) write_icc_stream(cs, rng, icc_bytes);
	}
	const int flag_xyb = opt.geti("xyb", 0), flag_ycbcr = opt.geti("ycbcr", 0);
	cs.pad();
	cs.put(0, 1);                       // FrameHeader: not all_default
	const int seq_type = g_seq ? g_seq->type : 0;
	cs.put(g_mod_lf ? 1 : (uint64_t) seq_type, 2);   // regular frame (an LF frame: type 1; types=: a reference-only frame, type 2)
	cs.put(1, 1);                       // modular
	cs.u64((patch_flag() ? 2 : 0) | (noise_flag() ? 1 : 0) | (spline_flag() ? 16 : 0));       // flags
	if (!flag_xyb) cs.put(flag_ycbcr ? 1 : 0, 1);   // do_ycbcr
	if (!flag_xyb && flag_ycbcr) cs.put(0, 6);      // jpeg_upsampling: none
	cs.put((uint64_t) up_log(), 2);     // log_upsampling (upsampling=)
	for (int k = 0; k < extra + (alpha ? 1 : 0); ++k) cs.put((uint64_t) up_ec_log(), 2);   // extra channel upsampling
	cs.put((uint64_t) (group_shift - 7), 2);
	if (seq_type == 2 && num_passes != 1) die("modular: a reference-only frame codes no passes: passes=1");
	if (seq_type != 2) cs.u32(num_passes, 1, 0, 2, 0, 3, 0, 4, 3);   // (not coded for a reference-only frame, j40.h:5276)
	if (num_passes > 1) {
		cs.u32(0, 0, 0, 1, 0, 2, 0, 3, 1);                  // num_ds = 0
		for (int i = 0; i < num_passes - 1; ++i) cs.put(0, 2);  // shift[i]
	}
	if (g_mod_lf) cs.put((uint64_t) (g_mod_lf->level - 1), 2);   // lf_level - 1; no crop, no blend info, never last, saved nowhere (j40.h:5285-5336)
	else
	write_frame_placement(cs, extra + (alpha ? 1 : 0), Wfull, Hfull);   // have_crop, blend modes (colour, extra channels), is_last
	cs.u32(0, 0, 0, 0, 4, 16, 5, 48, 10);
	cs.put(0, 1); cs.put(0, 1); cs.put(0, 2); cs.u64(0);   // restoration: explicit, gab off, epf 0, no extensions
	cs.u64(0);                          // frame extensions
	write_toc_and_sections(cs, sections, opt.geti("permute", 0), rng, opt.geti("slack", 0));
	if (g_seq) { seq_append(cs, sections); return 0; }
	std::vector<uint8_t> file = cs.bytes;
	if (container) {
		static const uint8_t HEAD[32] = {0, 0, 0, 0x0c, 'J', 'X', 'L', ' ', 0x0d, 0x0a, 0x87, 0x0a, 0, 0, 0, 0x14, 'f', 't', 'y', 'p', 'j', 'x', 'l', ' ', 0, 0, 0, 0, 'j', 'x', 'l', ' '};
		file.assign(HEAD, HEAD + 32);
		size_t total = 8 + cs.bytes.size();
		uint8_t hd[8] = {(uint8_t) (total >> 24), (uint8_t) (total >> 16), (uint8_t) (total >> 8), (uint8_t) total, 'j', 'x', 'l', 'c'};
		file.insert(file.end(), hd, hd + 8);
		file.insert(file.end(), cs.bytes.begin(), cs.bytes.end());
	}
	if (!write_file(out, file)) die("cannot write output");
	if (opt.geti("stats", 0)) {
		// what a reader makes of the colour channels once the global RCT is undone, in the reference's 16-bit arithmetic: how many samples
		// leave int16 on the way (they wrap) and how many end outside [0, 2^bpp) (the output clamps them); -1: not worked out for this stream
		long long wraps = -1, outside = -1;
		if (samples_known && !single && num_groups * num_passes + 1 != (int) encs.size()) samples_known = false;
		if (samples_known && total_ch >= 3) {
			wraps = outside = 0;
			const int type = rct >= 0 ? rct % 7 : 0;
			const size_t n = ch[0].px.size();
			for (size_t i = 0; i < n; ++i) {
				const int64_t A = ch[0].px[i], B = ch[1].px[i], C = ch[2].px[i];
				int64_t v[4] = {A, B, C, 0};   // (the three outputs, and the one intermediate of type 6)
				if (type == 6) { v[3] = A - (C >> 1); v[1] = C + v[3]; v[2] = v[3] - (B >> 1); v[0] = v[2] + B; }
				else { if (type & 1) v[2] = C + A; if ((type >> 1) == 1) v[1] = B + A; if ((type >> 1) == 2) v[1] = B + ((A + v[2]) >> 1); }
				bool wrapped = false;
				for (int k = 0; k < 4; ++k) wrapped |= v[k] < -32768 || v[k] > 32767;
				wraps += wrapped;
				for (int k = 0; k < 3; ++k) { const int16_t w16 = (int16_t) (uint16_t) (uint64_t) v[k]; outside += w16 < 0 || w16 > (1 << bpp) - 1; }
			}
		}
		// povf_extra_bits: [bit of the file, number of bits, value] per marked residual (sections stored in order, no container)
		std::string povf_list;
		if (!container && !opt.geti("permute", 0)) for (const PovfMark &m : povf_marks) {
			size_t behind = 0;
			for (size_t k = m.section; k < sections.size(); ++k) behind += sections[k].size();
			char tmp[96]; snprintf(tmp, sizeof tmp, "%s[%zu, %zu, %u]", povf_list.empty() ? "" : ", ", 8 * (file.size() - behind) + m.bit, m.nbits, m.extra);
			povf_list += tmp;
		}
		std::string dpred_list;   // the predictor of every palette with delta entries, global first
		for (const TransformW &t : transforms) if (t.kind == 1 && t.nb_deltas) dpred_list += (dpred_list.empty() ? "" : ", ") + std::to_string(t.d_pred);
		for (const auto &trs : group_tr) for (const TransformW &t : trs) if (t.kind == 1 && t.nb_deltas) dpred_list += (dpred_list.empty() ? "" : ", ") + std::to_string(t.d_pred);
		printf("{\"copies\": %llu, \"special_copies\": %llu, \"distinct_special_codes\": %d, \"plain_copies\": %llu, \"overlapping_copies\": %llu, "
		       "\"copies_crossing_rows\": %llu, \"copies_crossing_channels\": %llu, \"clamped_distances\": %llu, \"first_symbol_copies\": %llu, "
		       "\"copies_beyond_need\": %llu, \"distance_one_copies\": %llu, \"copies_near_2_20\": %llu, \"max_distance\": %llu, \"max_length\": %llu, \"max_section_integers\": %llu, "
		       "\"longest_symbol_bits\": %d, \"rct_wraps\": %lld, \"samples_outside_range\": %lld, \"sections\": %zu, \"povf_extra_bits\": [%s], \"palette_d_pred\": [%s], %s}\n",
		       (unsigned long long) lzstats.copies, (unsigned long long) lzstats.special_copies, lzstats.distinct_codes(), (unsigned long long) lzstats.plain_copies, (unsigned long long) lzstats.overlapping,
		       (unsigned long long) lzstats.cross_row, (unsigned long long) lzstats.cross_channel, (unsigned long long) lzstats.clamped, (unsigned long long) lzstats.first_symbol_copies,
		       (unsigned long long) lzstats.beyond_need, (unsigned long long) lzstats.distance_one, (unsigned long long) lzstats.far_copies, (unsigned long long) lzstats.max_distance, (unsigned long long) lzstats.max_length,
		       (unsigned long long) lzstats.max_section_integers, longest_symbol_bits, wraps, outside, sections.size(), povf_list.c_str(), dpred_list.c_str(), wp_stats_json().c_str());
	}
	fprintf(stderr, "modular %dx%d: %zu bytes (%.3f bpp), %d groups%s\n", Wfull, Hfull, file.size(), 8.0 * (double) file.size() / ((double) Wfull * Hfull), gcols_full * grows_full, single ? " (single section)" : "");
	return 0;
}


// ------------------------------------------------------------------------------------------------
// frames=N: N coded frames under one image header of W x H (the canvas). Frame k's picture and statistics come from seed SEED + k and
// its crop's size; every other option of the mode holds for each frame alike.
//   anim=1             the image header carries the animation header (10/1 ticks per second, 0 loops) and every frame a duration
//   durations=d0,d1,.. per-frame durations in ticks (default 1 with anim=1; without anim there is no such field: 0)
//   crops=x,y,w,h;...  per-frame crops; an empty entry is the full frame
//   srcs= saves=       per-frame source slots and save_as_reference values (default 0)
//   blends=            per-frame blend mode, all channels alike (default 0, Replace; 1 Add, 2 Blend, 3 MulAdd, 4 Mul)
//   ecblends= ecsrcs=  per-frame blend mode and source slot of the extra channels alone (default: the colour channels')
//   only=k             coded frame k alone, as a last frame, under the same image header, with the same crop and the same section bytes
//                      (a reference-only frame: as a regular frame)
//   types=             per-frame type: 0 a regular frame (default), 2 a reference-only frame with save_before_color_transform = 1 (sbct=0: 0),
//                      of the size its crops= entry gives, without an origin; saved into its saves= slot, never shown
//   patches=           per frame (entries separated by ';') the patch dictionary: reference patches separated by '/', each
//                      ref,x0,y0,w,h:x,y,mode,clamp[:x,y,mode,clamp...] -- the rectangle of the reference frame in slot ref and where it goes in
//                      which blend mode. Sets the frame's has_patches flag; nothing is checked (PatchRole). patchec=M: the extra channels'
//                      entries have mode M; patchcut=1: LfGlobal ends inside the dictionary; patchtwin=1: the flag and the dictionary left
//                      out, every other byte alike. stats=1 lists the placements written
//   noise=             per frame (entries separated by ';') the eight NoiseParameters v0,...,v7 (0..1023): sets the frame's noise flag; an
//                      empty entry: a frame without noise. noisetwin=1: the flag and the parameters left out, every other byte alike
//   splines=           per frame (entries separated by ';') the frame's splines (SplineRole above: x,y[:dx,dy...][|c:i=v,...], '/' between
//                      splines): sets the frame's splines flag; an empty entry: a frame without splines. qadj=, splinecount=, splinen=,
//                      splinecut=1 and splinetwin=1 apply to every frame that has an entry
// The last frame is is_last. stats=1 prints frames, shown, saved_slots and every frame's offsets instead of the mode's own statistics.
static std::vector<std::string> split_list(const std::string &v, char sep) {
	std::vector<std::string> out;
	size_t at = 0;
	if (v.empty()) return out;
	for (;;) { const size_t e = v.find(sep, at); out.push_back(v.substr(at, e == std::string::npos ? e : e - at)); if (e == std::string::npos) break; at = e + 1; }
	return out;
}
static int run_sequence(bool vardct, int W, int H, uint64_t seed, const char *out, const Options &opt_in) {
	const int N = opt_in.geti("frames", 1), only = opt_in.geti("only", -1), container = opt_in.geti("container", 0);
	if (N < 1 || N > 64) die("frames=1..64");
	if (only >= N) die("only= names a frame the sequence does not have");
	const bool anim = opt_in.geti("anim", 0) != 0;
	const std::vector<std::string> durs = split_list(opt_in.gets("durations", ""), ','), crops = split_list(opt_in.gets("crops", ""), ';'),
		srcs = split_list(opt_in.gets("srcs", ""), ','), saves = split_list(opt_in.gets("saves", ""), ','), blends = split_list(opt_in.gets("blends", ""), ','),
		ecblends = split_list(opt_in.gets("ecblends", ""), ','), ecsrcs = split_list(opt_in.gets("ecsrcs", ""), ','),
		types = split_list(opt_in.gets("types", ""), ','), patches = split_list(opt_in.gets("patches", ""), ';'),
		noises = split_list(photon_noise_given(opt_in) ? opt_in.gets("noise", "") : std::string(), ';'),
		splines = split_list(opt_in.gets("splines", ""), ';');
	if (!durs.empty() && !anim) die("durations= wants anim=1 (frames of a still have no duration)");
	// modes=v,m,...: per-frame writers, v the VarDCT one and m the Modular one (an empty entry: the command's mode). Every frame gets every
	// option; the first frame writes the image header, so the options must describe one image to both writers (a Modular frame under a
	// VarDCT frame's header: xyb=1, and alpha=1 for both or neither)
	const std::vector<std::string> modes = split_list(opt_in.gets("modes", ""), ',');
	bool any_vardct = vardct;
	for (const std::string &m : modes) { if (!m.empty() && m != "v" && m != "m") die("modes=v|m,..."); any_vardct = any_vardct || m == "v"; }
	if (!modes.empty() && any_vardct && !opt_in.geti("xyb", 0)) die("modes=: a Modular frame beside VarDCT frames is a frame of an XYB image: xyb=1");
	Options opt = opt_in;
	for (const char *k : {"frames", "anim", "durations", "crops", "srcs", "saves", "blends", "ecblends", "ecsrcs", "only", "container", "stats", "modes", "types", "patches", "patchtwin", "patchec", "patchcut", "sbct", "noisetwin"}) opt.kv.erase(k);
	for (const char *k : SPLINE_KEYS) opt.kv.erase(k);
	if (photon_noise_given(opt_in)) opt.kv.erase("noise");
	if (any_vardct && !opt.kv.count("fullheader")) opt.kv["fullheader"] = "1";
	auto at = [](const std::vector<std::string> &v, int k, int def) { return k < (int) v.size() && !v[(size_t) k].empty() ? atoi(v[(size_t) k].c_str()) : def; };
	std::vector<uint8_t> cs;
	std::string rows, patch_rows;
	int shown = 0; unsigned saved_slots = 0;
	for (int k = 0; k < N; ++k) {
		PatchRole role;
		role.twin = opt_in.geti("patchtwin", 0) != 0; role.ec_mode = opt_in.geti("patchec", 0); role.cut = opt_in.geti("patchcut", 0) != 0;
		if (k < (int) patches.size() && !patches[(size_t) k].empty()) {
			std::string placed;
			for (const std::string &one : split_list(patches[(size_t) k], '/')) {
				const std::vector<std::string> parts = split_list(one, ':');
				PatchRef r;
				if (parts.size() < 2 || sscanf(parts[0].c_str(), "%d,%d,%d,%d,%d", &r.ref, &r.x0, &r.y0, &r.w, &r.h) != 5 || r.ref < 0 || r.x0 < 0 || r.y0 < 0 || r.w < 1 || r.h < 1) die("patches=ref,x0,y0,w,h:x,y,mode,clamp[:x,y,mode,clamp...][/...];...");
				for (size_t j = 1; j < parts.size(); ++j) {
					PatchPlace q;
					if (sscanf(parts[j].c_str(), "%lld,%lld,%d,%d", &q.x, &q.y, &q.mode, &q.clamp) != 4 || q.mode < 0 || q.clamp < 0 || q.clamp > 1 || (j == 1 && (q.x < 0 || q.y < 0))) die("patches=: a placement is x,y,mode,clamp (the first one of a reference patch not negative)");
					r.at.push_back(q);
					char tmp[200]; snprintf(tmp, sizeof tmp, "%s[%lld, %lld, %d, %d, %d, %d, %d, %d, %d, %zu]", placed.empty() ? "" : ", ", q.x, q.y, r.w, r.h, r.x0, r.y0, r.ref, q.mode, q.clamp, role.refs.size());
					placed += tmp;
				}
				role.refs.push_back(r);
			}
			if (only < 0 || k == only) { char tmp[64]; snprintf(tmp, sizeof tmp, "%s{\"frame\": %d, \"placements\": [", patch_rows.empty() ? "" : ", ", k); patch_rows += tmp + placed + "]}"; }
		}
		NoiseRole noise;
		noise.twin = opt_in.geti("noisetwin", 0) != 0;
		const bool noisy = k < (int) noises.size() && !noises[(size_t) k].empty();
		if (noisy) parse_noise_role(noises[(size_t) k], &noise);
		SplineRole spl;   // (splines=: per frame, entries separated by ';', an empty entry: a frame without splines)
		spline_role_options(opt_in, &spl);
		const bool splined = k < (int) splines.size() && !splines[(size_t) k].empty();
		if (splined) parse_spline_role(splines[(size_t) k], &spl);
		SeqFrame q;
		q.canvas_w = W; q.canvas_h = H; q.anim = anim; q.cs = &cs;
		int fw = W, fh = H;
		if (k < (int) crops.size() && !crops[(size_t) k].empty()) {
			if (sscanf(crops[(size_t) k].c_str(), "%d,%d,%d,%d", &q.x0, &q.y0, &fw, &fh) != 4 || fw < 1 || fh < 1) die("crops=x,y,w,h;... (an empty entry: the full frame)");
			q.have_crop = true;
		}
		q.blend = at(blends, k, 0); q.src = at(srcs, k, 0); q.save = at(saves, k, 0); q.duration = anim ? at(durs, k, 1) : 0;
		q.ec_blend = at(ecblends, k, q.blend); q.ec_src = at(ecsrcs, k, q.src);
		if (q.blend < 0 || q.blend > 4 || q.src < 0 || q.src > 3 || q.ec_blend < 0 || q.ec_blend > 4 || q.ec_src < 0 || q.ec_src > 3 || q.save < 0 || q.save > 3 || q.duration < 0) die("blends 0..4, srcs and saves 0..3, durations >= 0");
		q.is_last = only >= 0 || k == N - 1;
		q.type = only >= 0 ? 0 : at(types, k, 0); q.save_before_ct = opt_in.geti("sbct", 1) ? 1 : 0;
		if (q.type != 0 && q.type != 2) die("types=0|2,...");
		if (q.type == 2 && q.is_last) die("types=: a reference-only frame is never the last one");
		if (q.type == 2) { q.x0 = q.y0 = 0; q.blend = q.ec_blend = 0; }
		if (only >= 0 && at(types, k, 0) == 2) { q.have_crop = false; q.canvas_w = fw; q.canvas_h = fh; }   // (alone: a regular frame of an image of its own size)
		if (q.type != 2 && (q.duration > 0 || q.is_last)) ++shown;
		if (q.type != 2 && !q.is_last && (q.duration == 0 || q.save != 0)) saved_slots |= 1u << q.save;
		if (only >= 0 && k != only) continue;
		q.first = cs.empty();
		g_seq = &q; g_patch = role.refs.empty() ? nullptr : &role; g_noise = noisy ? &noise : nullptr; g_spline = splined ? &spl : nullptr;
		const bool frame_vardct = k < (int) modes.size() && !modes[(size_t) k].empty() ? modes[(size_t) k] == "v" : vardct;
		const int e = frame_vardct ? run_vardct(fw, fh, seed + (uint64_t) k, out, opt) : run_modular(fw, fh, seed + (uint64_t) k, out, opt);
		g_seq = nullptr; g_patch = nullptr; g_noise = nullptr; g_spline = nullptr;
		if (e) return e;
		// (the first frame's bytes start with the signature and the image header: its frame header is found by a reader, not here)
		char tmp[160]; snprintf(tmp, sizeof tmp, "%s{\"frame\": %d, \"first_section\": %zu, \"end\": %zu}", rows.empty() ? "" : ", ", k, q.first_section, cs.size());
		rows += tmp;
	}
	std::vector<uint8_t> file;
	if (!container) file = cs;
	else {   // ISOBMFF wrapping (j40.h:1479): one jxlc box, or (container=2) the codestream split over two jxlp boxes around another box
		static const uint8_t HEAD[32] = {0, 0, 0, 0x0c, 'J', 'X', 'L', ' ', 0x0d, 0x0a, 0x87, 0x0a, 0, 0, 0, 0x14, 'f', 't', 'y', 'p', 'j', 'x', 'l', ' ', 0, 0, 0, 0, 'j', 'x', 'l', ' '};
		file.assign(HEAD, HEAD + 32);
		auto box = [&](const char *type, const uint8_t *p, size_t n, bool indexed, uint32_t idx) {
			const size_t total = 8 + n + (indexed ? 4 : 0);
			const uint8_t hd[8] = {(uint8_t) (total >> 24), (uint8_t) (total >> 16), (uint8_t) (total >> 8), (uint8_t) total, (uint8_t) type[0], (uint8_t) type[1], (uint8_t) type[2], (uint8_t) type[3]};
			file.insert(file.end(), hd, hd + 8);
			if (indexed) { const uint8_t ix[4] = {(uint8_t) (idx >> 24), (uint8_t) (idx >> 16), (uint8_t) (idx >> 8), (uint8_t) idx}; file.insert(file.end(), ix, ix + 4); }
			file.insert(file.end(), p, p + n);
		};
		if (container == 1) box("jxlc", cs.data(), cs.size(), false, 0);
		else {   // (the reference takes a jxlp index WITHOUT the top bit as the last one, j40.h:1557)
			const size_t cut = cs.size() / 3;
			static const uint8_t junk[5] = {1, 2, 3, 4, 5};
			box("jxlp", cs.data(), cut, true, 0x80000000u);
			box("xml ", junk, 5, false, 0);
			box("jxlp", cs.data() + cut, cs.size() - cut, true, 1);
		}
	}
	if (!write_file(out, file)) die("cannot write output");
	if (opt_in.geti("stats", 0)) printf("{\"frames\": %d, \"shown\": %d, \"saved_slots\": %d, \"written\": [%s], \"patches\": [%s]}\n", only >= 0 ? 1 : N, only >= 0 ? 1 : shown, only >= 0 ? 0 : __builtin_popcount(saved_slots), rows.c_str(), patch_rows.c_str());
	fprintf(stderr, "%s %dx%d: %zu bytes, %d coded frame(s)%s\n", vardct ? "vardct" : "modular", W, H, file.size(), only >= 0 ? 1 : N, anim ? ", animation" : "");
	return 0;
}

// ------------------------------------------------------------------------------------------------
// lflevels=1|2 (vardct): the LF image of the main frame as a frame of its own. Written under one image header of W x H: the level-2
// frame (if any, 1/64 of the size), the level-1 frame (1/8; with two levels it has use_lf_frame itself) and the main frame with
// use_lf_frame, whose LfGroups hold no LF stream. Every other option is the main frame's.
//   lfkind=flat      (default) every LF frame is DCT8 only with all HF zero, no chroma-from-luma, no smoothing, no filters: its picture
//                    is its LF integers times the LF step, each over an 8 x 8 square. The coarsest frame's integers come from the
//                    procedural picture of its own size (seed SEED + level)
//   lfkind=picture   (with forward=1) the LF frames forward-code the 8 x 8 cell means of the next finer frame's XYB samples; lfgab= and
//                    lfepf= are the LF frames' gab= and epf=, lfhfmul= their HfMul (default 64, about ten times finer than the main
//                    frame's: an error in an LF sample is an error in all 64 pixels of its cell, so an encoder spends bits here).
//                    Not with bctx=1: the LF index of a cell is counted on the samples the LF frame DECODES to, which this writer does
//                    not know, so it cannot choose the block contexts a decoder will use (with lfkind=flat it knows them exactly)
//   lftwin=1         (flat) instead, the ordinary one-frame stream whose LfCoefficients are the flat LF frame's integers over 8 x 8
//                    (two levels: 64 x 64) cells, with nosmooth=1 and extraprec=0: same seed, so the same varblocks and HF sections
//   only=k           coded frame k (0: the coarsest LF frame) alone, as the regular last frame of an image of its own size. Not the main
//                    frame (alone it has no LF image; lftwin=1 is its stand-alone form where the LF frames are flat), and not a frame
//                    with use_lf_frame unless it is flat (then its LF integers are written out, as in a twin)
//   bctx=1           the custom block-context map with LF thresholds combines with all of it but lfkind=picture (above)
//   lfcrop=w,h       the main frame is a crop of w x h at (0, 0): a stream a decoder has to refuse, its LF frame is not of its cells' size
//   lfmodular=1      (flat) the coarsest LF frame is written as a Modular frame of the XYB image -- the only kind of LF frame libjxl writes --
//                    whose planes c0 = qY, c1 = qX, c2 = qB - qY are the flat VarDCT LF frame's integers, each over an 8 x 8 square. A decoder
//                    that renders such a frame to XYB floats as (float) c0 * m[1], (float) c1 * m[0], (float) (c2 + c0) * m[2] arrives at the
//                    flat VarDCT LF frame's samples float for float where that frame's LF step is m itself: global_scale * quant_lf = 65536;
//                    and nocfl=1, so that no B sample carries a Y term. Refused elsewhere. (lftwin=1: the twin is the same stream either way.)
// noise=v0,...,v7: the main frame's noise parameters (noisetwin=1: left out again); noiself=1: the LF frames carry them too.
// splines=: the main frame's splines (splinetwin=1: left out again); splinelf=1: the LF frames carry them too.
// stats=1 prints the number of coded frames and how many values the main frame's LF index takes.
static int run_lf_sequence(int W, int H, uint64_t seed, const char *out, const Options &opt_in) {
	const int levels = opt_in.geti("lflevels", 1), twin = opt_in.geti("lftwin", 0), only = opt_in.geti("only", -1);
	const std::string kind = opt_in.gets("lfkind", "flat");
	if (levels < 1 || levels > 2) die("lflevels=1|2");
	if (kind != "flat" && kind != "picture") die("lfkind=flat|picture");
	const bool picture = kind == "picture";
	if (picture && !opt_in.geti("forward", 0)) die("lfkind=picture wants forward=1");
	if (picture && (twin || opt_in.geti("bctx", 0))) die("lfkind=picture: what its LF frame decodes to is not known here, so neither a twin nor LF thresholds (bctx=1) can be written");
	if (opt_in.geti("extraprec", 0) || opt_in.geti("container", 0)) die("lflevels: extraprec=0 and no container");
	if (only >= levels) die("only= names an LF frame here (0: the coarsest); the main frame is nothing without its LF frame");
	if (only >= 0 && twin) die("only= and lftwin=1 exclude each other");
	const int lfmodular = opt_in.geti("lfmodular", 0);
	if (lfmodular) {
		if (picture || only >= 0) die("lfmodular=1 writes the flat LF frame's integers as a Modular frame: lfkind=flat, no only=");
		if ((long long) opt_in.geti("global_scale", 0) * opt_in.geti("quant_lf", 0) != 65536) die("lfmodular=1: the Modular LF frame's samples are integers times LfGlobal's LF dequantisation; they equal the flat VarDCT LF frame's only where its LF step is that factor: global_scale * quant_lf = 65536 (for instance global_scale=4096 quant_lf=16)");
		if (!opt_in.geti("nocfl", 0)) die("lfmodular=1 wants nocfl=1: with chroma-from-luma the B samples carry a Y term that B - Y integers do not state");
		if (opt_in.geti("alpha", 0)) die("lfmodular=1: no extra channels (an LF frame of such an image is refused)");
	}
	Options main_opt = opt_in;
	for (const char *k : {"lflevels", "lfkind", "lftwin", "only", "stats", "lfgab", "lfepf", "lfcrop", "lfhfmul", "lfmodular", "noisetwin", "noiself", "splinelf"}) main_opt.kv.erase(k);
	for (const char *k : SPLINE_KEYS) main_opt.kv.erase(k);
	// splines= (one entry): the main frame's; splinelf=1: the LF frames get the flag and the data too (a stream a decoder has to refuse)
	SplineRole spl;
	spline_role_options(opt_in, &spl);
	const bool splined = opt_in.kv.count("splines") != 0, spline_lf = opt_in.geti("splinelf", 0) != 0;
	if (splined) parse_spline_role(opt_in.gets("splines", ""), &spl);
	if (photon_noise_given(opt_in)) main_opt.kv.erase("noise");
	// noise= (one entry): the main frame's; noiself=1: the LF frames get the flag and the parameters too (a stream a decoder has to refuse)
	NoiseRole noise;
	noise.twin = opt_in.geti("noisetwin", 0) != 0;
	const bool noisy = photon_noise_given(opt_in), noise_lf = opt_in.geti("noiself", 0) != 0;
	if (noisy) parse_noise_role(opt_in.gets("noise", ""), &noise);
	int crop_w = 0, crop_h = 0;
	if (opt_in.kv.count("lfcrop") && (sscanf(opt_in.gets("lfcrop", "").c_str(), "%d,%d", &crop_w, &crop_h) != 2 || crop_w < 1 || crop_h < 1 || crop_w > W || crop_h > H || picture || twin || only >= 0)) die("lfcrop=w,h within the image, with lfkind=flat and neither lftwin nor only");
	main_opt.kv["fullheader"] = "1";
	// (a picture: every frame with use_lf_frame codes no chroma-from-luma, so that the LF frame under it holds the B samples themselves,
	// coded against its own dequantised Y like any frame's; B - Y in a plane of its own would take Y's coding error on top of its own)
	if (picture) main_opt.kv["nocfl"] = "1";
	Options lf_opt = main_opt;
	for (const char *k : {"gab", "epf", "dumpsrc", "passes", "rfdefault"}) lf_opt.kv.erase(k);
	lf_opt.kv["nocfl"] = "1"; lf_opt.kv["nosmooth"] = "1"; lf_opt.kv["coverage"] = "0";
	Options lf_top_opt;   // the coarsest LF frame's: it has no use_lf_frame
	if (!picture) { lf_opt.kv["dct8only"] = "1"; lf_opt.kv["density"] = "0"; lf_opt.kv["forward"] = "0"; }
	else {
		if (opt_in.kv.count("lfgab")) lf_opt.kv["gab"] = opt_in.gets("lfgab", "0");
		if (opt_in.kv.count("lfepf")) lf_opt.kv["epf"] = opt_in.gets("lfepf", "0");
		lf_opt.kv["hfmul"] = opt_in.gets("lfhfmul", "64");
	}
	lf_top_opt = lf_opt;
	if (picture) lf_top_opt.kv.erase("nocfl");
	auto lf_opt_of = [&](int l) -> const Options & { return l == levels ? lf_top_opt : lf_opt; };
	int fw[3], fh[3];
	fw[0] = W; fh[0] = H;
	for (int l = 1; l <= levels; ++l) { fw[l] = (fw[l - 1] + 7) / 8; fh[l] = (fh[l - 1] + 7) / 8; }
	std::vector<uint8_t> cs, nowhere;
	// one coded frame: level l (0: the main frame) with `role`, behind `into` (null: a file of its own, a regular last frame)
	auto write = [&](int l, LfRole &role, std::vector<uint8_t> *into, const Options &o) {
		SeqFrame q;
		q.canvas_w = W; q.canvas_h = H; q.cs = into; q.first = into && into->empty(); q.is_last = l == 0;
		q.have_crop = l == 0 && crop_w > 0;
		g_seq = into ? &q : nullptr; g_lf = &role; g_noise = noisy && (l == 0 || noise_lf) ? &noise : nullptr; g_spline = splined && (l == 0 || spline_lf) ? &spl : nullptr;
		const int e = run_vardct(q.have_crop ? crop_w : fw[l], q.have_crop ? crop_h : fh[l], seed + (uint64_t) l, out, o);
		g_seq = nullptr; g_lf = nullptr; g_noise = nullptr; g_spline = nullptr;
		if (e) die("lflevels: a frame could not be written");
	};
	LfRole roles[3];
	if (picture) {
		// the samples each LF frame codes: the next finer frame's cell means, found by writing that frame to nowhere first
		Options dry = main_opt; dry.kv.erase("dumpsrc");
		roles[0].capture = true;
		write(0, roles[0], &nowhere, dry);
		for (int c = 0; c < 3; ++c) roles[1].pic[c] = roles[0].means[c];
		if (roles[0].means_w != fw[1] || roles[0].means_h != fh[1]) die("lflevels: the cell means are not the LF frame's size");
		if (levels == 2) {
			nowhere.clear(); roles[1].capture = true;
			write(1, roles[1], &nowhere, lf_opt_of(1));
			for (int c = 0; c < 3; ++c) roles[2].pic[c] = roles[1].means[c];
			roles[1].capture = false;
		}
		roles[0].capture = false;
	}
	const bool alone = twin || only >= 0;
	int written = 0;
	for (int l = levels; l >= 0; --l) {
		LfRole &r = roles[l];
		const int k = levels - l;   // its place in coded order
		if (only >= 0 && k > only) break;
		const bool last_of_call = only >= 0 ? k == only : l == 0;
		if (l < levels && !picture) { r.replicate = true; for (int c = 0; c < 3; ++c) r.src[c] = roles[l + 1].out[c]; r.src_w = roles[l + 1].out_w; }
		if (alone && last_of_call) {
			if (l < levels && picture) die("only=: a frame with use_lf_frame decodes alone only where it is flat");
			Options o = l == 0 ? main_opt : lf_opt_of(l);
			if (l == 0) { o.kv["nosmooth"] = "1"; o.kv["extraprec"] = "0"; }
			write(l, r, nullptr, o);
			++written;
			break;
		}
		r.level = l; r.use = l < levels;
		nowhere.clear();
		if (lfmodular && l == levels) {
			// the flat VarDCT LF frame to nowhere, for its integers (streamed order Y, X, B); then the Modular frame that states them
			write(l, r, &nowhere, lf_opt_of(l));
			ModularLfRole mr;
			mr.level = l; mr.src_w = r.out_w;
			mr.src[0] = r.out[0]; mr.src[1] = r.out[1]; mr.src[2] = r.out[2];
			for (size_t i = 0; i < mr.src[2].size(); ++i) mr.src[2][i] -= mr.src[0][i];
			Options mo;
			mo.kv["xyb"] = "1"; mo.kv["rct"] = "-1";
			SeqFrame q;
			q.canvas_w = W; q.canvas_h = H; q.cs = alone ? &nowhere : &cs; q.first = q.cs->empty() || alone; q.is_last = false;
			if (alone) nowhere.clear();
			g_seq = &q; g_mod_lf = &mr;
			const int e = run_modular(fw[l], fh[l], seed + (uint64_t) l, out, mo);
			g_seq = nullptr; g_mod_lf = nullptr;
			if (e) die("lflevels: the Modular LF frame could not be written");
			++written;
			continue;
		}
		write(l, r, alone ? &nowhere : &cs, l == 0 ? main_opt : lf_opt_of(l));
		++written;
	}
	if (!alone && !write_file(out, cs)) die("cannot write output");
	if (opt_in.geti("stats", 0)) printf("{\"frames\": %d, \"lfidx_distinct\": %d}\n", alone ? 1 : written, roles[only >= 0 ? levels - only : 0].lfidx_distinct);
	return 0;
}

int main(int argc, char **argv) {
	if (argc < 6) { fprintf(stderr, "usage: %s vardct|modular W H SEED OUT [key=value ...]\n", argv[0]); return 1; }
	Options opt;
	for (int i = 6; i < argc; ++i) { std::string a = argv[i]; size_t eq = a.find('='); if (eq == std::string::npos) die("options are key=value"); opt.kv[a.substr(0, eq)] = a.substr(eq + 1); }
	int W = atoi(argv[2]), H = atoi(argv[3]); uint64_t seed = strtoull(argv[4], nullptr, 0);
	if (W <= 0 || H <= 0) die("bad dimensions");
	const bool vardct = !strcmp(argv[1], "vardct");
	if (!vardct && strcmp(argv[1], "modular")) die("unknown mode");
	if (opt.kv.count("orientation")) {
		g_orientation = opt.geti("orientation", 0);
		if (g_orientation < 1 || g_orientation > 8) die("orientation=1..8");
		opt.kv.erase("orientation");
	}
	{   // the cenc= family
		static const char *const CENC_KEYS[] = {"cenc", "white", "primaries", "tf", "gamma", "intent", "whitexy", "primxy"};
		for (const char *k : CENC_KEYS) g_cenc.set = g_cenc.set || opt.kv.count(k);
		if (opt.kv.count("cenc") && !opt.geti("cenc", 0)) g_cenc.set = false;
		auto ints = [&](const char *k, int *out, size_t n) {
			const std::string v = opt.gets(k, "");
			size_t at = 0, got = 0;
			while (at < v.size() && got < n) { size_t e = v.find(',', at); if (e == std::string::npos) e = v.size(); out[got++] = atoi(v.substr(at, e - at).c_str()); at = e + 1; }
			if (got != n) die("cenc: whitexy= wants 2 values, primxy= 6");
		};
		g_cenc.white = opt.geti("white", 1); g_cenc.primaries = opt.geti("primaries", 1); g_cenc.tf = opt.geti("tf", 13);
		g_cenc.gamma = opt.geti("gamma", 0); g_cenc.intent = opt.geti("intent", 1);
		if (opt.kv.count("whitexy")) ints("whitexy", g_cenc.whitexy, 2);
		if (opt.kv.count("primxy")) ints("primxy", g_cenc.primxy, 6);
		if (g_cenc.set && (g_cenc.white < 0 || g_cenc.white > 81 || g_cenc.primaries < 0 || g_cenc.primaries > 81 || g_cenc.tf < 0 || g_cenc.tf > 81 || g_cenc.intent < 0 || g_cenc.intent > 81 || g_cenc.gamma < 0 || g_cenc.gamma >= (1 << 24)))
			die("cenc: a value out of its field's range");
		if (g_cenc.set && (opt.geti("grey", 0) || opt.geti("icc", 0))) die("cenc= does not combine with grey=1 or icc=");
		for (const char *k : CENC_KEYS) opt.kv.erase(k);
	}
	if (opt.kv.count("tone") || opt.kv.count("opsin") || opt.kv.count("cwmask")) {
		if (!vardct && !opt.geti("xyb", 0)) die("tone=, opsin= and cwmask= belong to the vardct mode and to Modular frames of an XYB image (xyb=1)");
		auto halves = [&](const char *k) {   // f16 bits of every value of the list
			std::vector<uint32_t> v; const std::string s = opt.gets(k, "");
			for (size_t at = 0; at < s.size(); ) {
				size_t e = s.find(',', at); if (e == std::string::npos) e = s.size();
				const std::string t = s.substr(at, e - at);
				if (t.size() == 5 && t[0] == 'h') v.push_back((uint32_t) strtoul(t.c_str() + 1, nullptr, 16) & 0xffff);
				else v.push_back(f16_bits(strtof(t.c_str(), nullptr)));
				at = e + 1;
			}
			return v;
		};
		if (opt.kv.count("tone")) {
			g_tone = halves("tone");
			if (g_tone.size() < 2 || g_tone.size() > 4) die("tone=IT,MIN[,LINEAR_BELOW[,RELATIVE]]");
			g_tone.resize(4, 0);
		}
		if (opt.kv.count("opsin")) { g_opsin = halves("opsin"); if (g_opsin.size() != 16) die("opsin= wants 16 values"); }
		if (opt.kv.count("cwmask") && g_opsin.empty()) die("cwmask= wants opsin=");
		g_cw_mask = opt.geti("cwmask", 0);
		if (g_cw_mask < 0 || g_cw_mask > 7) die("cwmask=0..7");
		for (const char *k : {"tone", "opsin", "cwmask"}) opt.kv.erase(k);
	}
	if (opt.kv.count("upsampling")) {
		g_up.k = opt.geti("upsampling", 1);
		if (g_up.k != 2 && g_up.k != 4 && g_up.k != 8) die("upsampling=2|4|8");
		if (!vardct && !opt.geti("xyb", 0)) die("upsampling= belongs to the vardct mode and to Modular frames of an XYB image (xyb=1)");
		for (const char *k : {"lflevels", "frames", "anim", "modes", "types", "patches"}) if (opt.kv.count(k)) die("upsampling= belongs to a single frame");
		g_up.twin = opt.geti("uptwin", 0);
		g_up.ecup = opt.geti("ecup", 0);
		if (g_up.twin < 0 || g_up.twin > 2 || (g_up.ecup != 0 && g_up.ecup != 1 && g_up.ecup != 2 && g_up.ecup != 4 && g_up.ecup != 8)) die("uptwin=0|1|2, ecup=1|2|4|8");
		g_up.shown_w = g_up.k * W; g_up.shown_h = g_up.k * H;
		if (opt.kv.count("upshown") && sscanf(opt.gets("upshown", "").c_str(), "%d,%d", &g_up.shown_w, &g_up.shown_h) != 2) die("upshown=W,H");
		if ((g_up.shown_w + g_up.k - 1) / g_up.k != W || (g_up.shown_h + g_up.k - 1) / g_up.k != H) die("upshown=: the positional size must be ceil(shown / K)");
		const std::string uw = opt.gets("upweights", "default");
		const int n5 = 5 * g_up.k / 2, count = n5 * (n5 + 1) / 2;
		if (uw == "nearest") {
			for (int y = 0; y < n5; ++y) for (int x = y; x < n5; ++x) g_up.table.push_back(f16_bits(y % 5 == 2 && x % 5 == 2 ? 1.0f : 0.0f));
		} else if (uw != "default") {
			for (size_t at = 0; at < uw.size(); ) {
				size_t e = uw.find(',', at); if (e == std::string::npos) e = uw.size();
				g_up.table.push_back(f16_round_bits(strtof(uw.substr(at, e - at).c_str(), nullptr)));
				at = e + 1;
			}
			if ((int) g_up.table.size() != count) die("upweights=: 15 values for upsampling=2, 55 for 4, 210 for 8");
		}
		g_up.block = !g_up.table.empty();
		for (const char *k : {"upsampling", "uptwin", "upshown", "upweights", "ecup"}) opt.kv.erase(k);
	} else if (opt.kv.count("uptwin") || opt.kv.count("upshown") || opt.kv.count("upweights")) die("uptwin=, upshown= and upweights= want upsampling=");
	if (opt.kv.count("lflevels")) {
		if (!vardct) die("lflevels= belongs to the vardct mode");
		return run_lf_sequence(W, H, seed, argv[5], opt);
	}
	static const char *const SEQ_KEYS[] ={"frames", "anim", "durations", "crops", "srcs", "saves", "blends", "ecblends", "ecsrcs", "only", "modes", "types", "patches"};
	bool sequence = false;
	for (const char *k : SEQ_KEYS) sequence = sequence || opt.kv.count(k);
	if (!sequence) {   // (noise= on a single frame: the one entry)
		NoiseRole noise;
		noise.twin = opt.geti("noisetwin", 0) != 0;
		if (photon_noise_given(opt)) { parse_noise_role(opt.gets("noise", ""), &noise); g_noise = &noise; opt.kv.erase("noise"); }
		opt.kv.erase("noisetwin");
		SplineRole spl;   // (splines= on a single frame: the one entry)
		spline_role_options(opt, &spl);
		if (opt.kv.count("splines")) { parse_spline_role(opt.gets("splines", ""), &spl); g_spline = &spl; }
		for (const char *k : SPLINE_KEYS) opt.kv.erase(k);
		return vardct ? run_vardct(W, H, seed, argv[5], opt) : run_modular(W, H, seed, argv[5], opt);
	}
	return run_sequence(vardct, W, H, seed, argv[5], opt);
}
