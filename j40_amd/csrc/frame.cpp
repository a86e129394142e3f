// j40_amd/csrc/frame.cpp -- see frame.hpp
#include "frame.hpp"
#include "tables.hpp"
#include <algorithm>
#include <cmath>
#include <thread>
#include <atomic>
#include <chrono>
#include <mutex>

namespace j40hip {

// ------------------------------------------------------------------------------------------------
// container (ISO 18181-2 boxes; reference: j40__container, j40.h:1479)

static uint32_t be32(const uint8_t *p) { return ((uint32_t) p[0] << 24) | ((uint32_t) p[1] << 16) | ((uint32_t) p[2] << 8) | p[3]; }

void extract_codestream(const uint8_t *data, size_t size, const uint8_t **cs, size_t *cs_size, std::vector<uint8_t> *storage, int *stray_tail) {
	if (stray_tail) *stray_tail = 0;
	static const uint8_t SIGNATURE[32] = {0, 0, 0, 0x0c, 'J', 'X', 'L', ' ', 0x0d, 0x0a, 0x87, 0x0a, 0, 0, 0, 0x14, 'f', 't', 'y', 'p', 'j', 'x', 'l', ' ', 0, 0, 0, 0, 'j', 'x', 'l', ' '};
	J40HIP_SHOULD(size >= 2, "shrt");
	if (data[0] == 0xff && data[1] == 0x0a) { *cs = data; *cs_size = size; return; }
	J40HIP_SHOULD(data[0] == SIGNATURE[0] && data[1] == SIGNATURE[1], "!jxl");
	J40HIP_SHOULD(size >= 32, "shrt");
	J40HIP_SHOULD(memcmp(data, SIGNATURE, 12) == 0, "!jxl");
	J40HIP_SHOULD(memcmp(data + 12, SIGNATURE + 12, 20) == 0, "ftyp");
	size_t pos = 32;
	bool seen_jxlc = false, seen_jxlp = false, seen_jxll = false, seen_jxli = false;
	struct Piece { size_t off, len; };
	std::vector<Piece> pieces;
	// The reference maps boxes on demand (j40__container, j40.h:1479): once the codestream is complete it never looks at what
	// follows, and a codestream box that is cut off yields the bytes that are there (the decoder then runs out of data in whatever
	// section that hits). Same here: stop behind `jxlc` / the last `jxlp`, and take a truncated codestream box as far as it goes.
	bool complete = false, no_more_codestream = false;
	while (pos < size) {
		if (size - pos < 8) { J40HIP_SHOULD(!pieces.empty(), "shrt"); if (stray_tail) *stray_tail = (int) (size - pos); break; }
		if (complete) break;
		uint64_t box = be32(data + pos);
		uint32_t type = be32(data + pos + 4);
		size_t header = 8, payload;
		if (box == 1) {
			J40HIP_SHOULD(size - pos >= 16, "shrt");
			box = ((uint64_t) be32(data + pos + 8) << 32) | be32(data + pos + 12);
			J40HIP_SHOULD(box >= 16, "boxx");
			header = 16;
		} else if (box != 0) J40HIP_SHOULD(box >= 8, "boxx");
		bool to_eof = box == 0;
		payload = to_eof ? size - pos - header : (size_t) box - header;
		const bool cut_off = !to_eof && payload > size - pos - header;
		if (cut_off) {
			if (type != 0x6a786c63 && type != 0x6a786c70) { J40HIP_SHOULD(!pieces.empty(), "shrt"); break; }   // junk behind the codestream
			payload = size - pos - header; to_eof = true;
		}
		size_t body = pos + header;
		switch (type) {
		case 0x6a786c6c: J40HIP_SHOULD(!seen_jxll, "box?"); seen_jxll = true; break;          // jxll
		case 0x6a786c69: J40HIP_SHOULD(!seen_jxli, "box?"); seen_jxli = true; break;          // jxli
		case 0x6a786c63:                                                                       // jxlc
			J40HIP_SHOULD(!seen_jxlc && !seen_jxlp, "box?");
			seen_jxlc = true; pieces.push_back({body, payload}); complete = true;
			break;
		case 0x6a786c70:                                                                       // jxlp
			J40HIP_SHOULD(!seen_jxlc && !no_more_codestream, "box?");
			J40HIP_SHOULD(payload >= 4, "jxlp");
			seen_jxlp = true; pieces.push_back({body + 4, payload - 4});                       // the sequence index is not interpreted ...
			if (!(data[body] >> 7)) no_more_codestream = true;                                 // ... except for this (j40.h:1557, as the reference has it)
			break;
		case 0x62726f62:                                                                       // brob
			J40HIP_SHOULD(payload > 4, "brot");
			{ uint32_t inner = be32(data + body); J40HIP_SHOULD(inner != 0x62726f62 && (inner >> 8) != 0x6a786c, "brot"); }
			break;
		default: break;
		}
		if (to_eof) break;
		pos = body + payload;
	}
	J40HIP_SHOULD(!pieces.empty(), "shrt");
	if (pieces.size() == 1) { *cs = data + pieces[0].off; *cs_size = pieces[0].len; return; }
	storage->clear();
	for (const Piece &p : pieces) storage->insert(storage->end(), data + p.off, data + p.off + p.len);
	*cs = storage->data(); *cs_size = storage->size();
}

// ------------------------------------------------------------------------------------------------
// image metadata (j40.h:3001-3313)

static void read_size_header(BitReader &br, int32_t *w, int32_t *h) {  // j40.h:3008
	bool div8 = br.u(1);
	*h = div8 ? ((int32_t) br.u(5) + 1) * 8 : br.u32(1, 9, 1, 13, 1, 18, 1, 30);
	switch (br.u(3)) {
	case 0: *w = div8 ? ((int32_t) br.u(5) + 1) * 8 : br.u32(1, 9, 1, 13, 1, 18, 1, 30); break;
	case 1: *w = *h; break;
	case 2: *w = (int32_t) ((uint64_t) *h * 6 / 5); break;
	case 3: *w = (int32_t) ((uint64_t) *h * 4 / 3); break;
	case 4: *w = (int32_t) ((uint64_t) *h * 3 / 2); break;
	case 5: *w = (int32_t) ((uint64_t) *h * 16 / 9); break;
	case 6: *w = (int32_t) ((uint64_t) *h * 5 / 4); break;
	default: J40HIP_SHOULD(*h < 0x40000000, "bigg"); *w = *h * 2; break;
	}
}

static void read_bit_depth(BitReader &br, int32_t *bpp, int32_t *exp_bits) {  // j40.h:3033
	if (br.u(1)) {
		*bpp = br.u32(32, 0, 16, 0, 24, 0, 1, 6);
		*exp_bits = (int32_t) br.u(4) + 1;
		int32_t mantissa = *bpp - *exp_bits - 1;
		J40HIP_SHOULD(2 <= mantissa && mantissa <= 23, "bpp?");
		J40HIP_SHOULD(2 <= *exp_bits && *exp_bits <= 8, "exp?");
	} else {
		*bpp = br.u32(8, 0, 10, 0, 12, 0, 1, 6);
		*exp_bits = 0;
		J40HIP_SHOULD(1 <= *bpp && *bpp <= 31, "bpp?");
	}
}

// j40__name (j40.h:3050): the name is validated as UTF-8 the way the reference does it -- including `i + c < len` where `<=` was
// meant, which makes the last character of every name fail: any non-empty name is a `name` error there, and so it is here
static void skip_name(BitReader &br) {
	int32_t len = br.u32(0, 0, 0, 4, 16, 5, 48, 10);
	std::vector<uint8_t> buf((size_t) len + 1, 0);
	for (int32_t i = 0; i < len; ++i) buf[(size_t) i] = (uint8_t) br.u(8);
	for (int32_t i = 0; i < len; ) {
		int32_t c = buf[(size_t) i++];
		const int32_t cc = buf[(size_t) i];   // the terminating zero keeps this in range
		c = c < 0x80 ? 0 : c < 0xc2 ? -1 : c < 0xe0 ? 1 :
			c < 0xf0 ? ((c == 0xe0 ? cc >= 0xa0 : c == 0xed ? cc < 0xa0 : true) ? 2 : -1) :
			c < 0xf5 ? ((c == 0xf0 ? cc >= 0x90 : c == 0xf4 ? cc < 0x90 : true) ? 3 : -1) : -1;
		J40HIP_SHOULD(c >= 0 && i + c < len, "name");
		while (c-- > 0) J40HIP_SHOULD((buf[(size_t) i++] & 0xc0) == 0x80, "name");
	}
}

static void read_extensions(BitReader &br) {  // j40.h:3088
	uint64_t extensions = br.u64();
	int64_t nbits = 0;
	for (int i = 0; i < 64; ++i) if (extensions >> i & 1) {
		uint64_t n = br.u64();
		J40HIP_SHOULD(n <= (uint64_t) INT64_MAX - (uint64_t) nbits, "flen");
		nbits += (int64_t) n;
	}
	br.skip_bits_like_reference(nbits);
}

// a CustomXY: two values of 1e-6 each, stored sign-folded (the sign in bit 0)
static void read_customxy(BitReader &br, int32_t xy[2]) {
	for (int i = 0; i < 2; ++i) {
		const uint32_t u = (uint32_t) br.u32(0, 19, 0x80000, 19, 0x100000, 20, 0x200000, 21);
		xy[i] = (int32_t) (u >> 1) ^ -(int32_t) (u & 1);
	}
}
// the chromaticities the white point and primaries enums stand for (BT.709 / sRGB, BT.2100, SMPTE 431 / 428; 1e-6 each)
static void enum_white_xy(int32_t wp, int32_t xy[2]) {
	static const int32_t D65[2] = {312700, 329000}, E[2] = {333333, 333333}, DCI[2] = {314000, 351000};
	const int32_t *s = wp == 10 ? E : wp == 11 ? DCI : D65;
	xy[0] = s[0]; xy[1] = s[1];
}
static void enum_primaries_xy(int32_t pr, int32_t xy[3][2]) {
	static const int32_t SRGB[3][2] = {{640000, 330000}, {300000, 600000}, {150000, 60000}};
	static const int32_t BT2100[3][2] = {{708000, 292000}, {170000, 797000}, {131000, 46000}};
	static const int32_t P3[3][2] = {{680000, 320000}, {265000, 690000}, {150000, 60000}};
	const int32_t (*s)[2] = pr == 9 ? BT2100 : pr == 11 ? P3 : SRGB;
	for (int i = 0; i < 3; ++i) { xy[i][0] = s[i][0]; xy[i][1] = s[i][1]; }
}

static void read_image_metadata(BitReader &br, ImageMeta *im, bool allow_wide, bool allow_upsampling) {  // j40.h:3104
	static const float OPSIN_INV[3][3] = {
		{11.031566901960783f, -9.866943921568629f, -0.16462299647058826f},
		{-3.254147380392157f, 4.418770392156863f, -0.16462299647058826f},
		{-3.6588512862745097f, 2.7129230470588235f, 1.9459282392156863f}};
	memcpy(im->opsin_inv_mat, OPSIN_INV, sizeof OPSIN_INV);
	im->opsin_bias[0] = im->opsin_bias[1] = im->opsin_bias[2] = -0.0037930732552754493f;
	im->quant_bias[0] = 1.0f - 0.05465007330715401f;
	im->quant_bias[1] = 1.0f - 0.07005449891748593f;
	im->quant_bias[2] = 1.0f - 0.049935103337343655f;
	im->quant_bias_num = 0.145f;

	read_size_header(br, &im->width, &im->height);
	// Main profile, level 5 limits (j40.h:1170)
	J40HIP_SHOULD(im->width <= (1 << 18) && im->height <= (1 << 18), "slim");
	J40HIP_SHOULD((int64_t) im->width * im->height <= (1 << 28), "slim");

	if (!br.u(1)) {  // !all_default
		bool extra_fields = br.u(1);
		if (extra_fields) {
			im->orientation = 1 + (int32_t) br.u(3);
			if (br.u(1)) { int32_t w, h; read_size_header(br, &w, &h); }
			if (br.u(1)) J40HIP_RAISE("TODO");  // preview
			if (br.u(1)) {  // animation
				im->anim_tps_num = br.u32(100, 0, 1000, 0, 1, 10, 1, 30);
				im->anim_tps_den = br.u32(1, 0, 1001, 0, 1, 8, 1, 10);
				im->anim_loops = (int64_t) br.u32_64(0, 0, 0, 3, 0, 16, 0, 32);
				im->have_animation = true;
				im->anim_have_timecodes = br.u(1);
			}
		}
		read_bit_depth(br, &im->bpp, &im->exp_bits);
		J40HIP_SHOULD(im->bpp <= 16, "fbpp");
		im->modular_16bit_buffers = br.u(1);
		J40HIP_SHOULD(im->modular_16bit_buffers || allow_wide, "fm32");   // (Frame::allow_wide; the reference refuses every such image, j40.h:3169)
		int32_t num_ec = br.u32(0, 0, 1, 0, 2, 4, 1, 12);
		J40HIP_SHOULD(num_ec <= 4, "elim");
		im->ec.assign((size_t) num_ec, ExtraChannel());
		for (ExtraChannel &ec : im->ec) {
			if (br.u(1)) { ec.type = EC_ALPHA; ec.bpp = 8; }
			else {
				ec.type = br.enum_();
				read_bit_depth(br, &ec.bpp, &ec.exp_bits);
				ec.dim_shift = br.u32(0, 0, 3, 0, 4, 0, 1, 3);
				skip_name(br);
				switch (ec.type) {
				case EC_ALPHA: ec.alpha_associated = br.u(1); break;
				case EC_SPOT: for (int i = 0; i < 4; ++i) (void) br.f16(); break;
				case EC_CFA: (void) br.u32(1, 0, 0, 2, 3, 4, 19, 8); break;
				case EC_BLACK: J40HIP_RAISE("fblk");
				case 1: case 3: case 6: case 15: case 16: break;
				default: J40HIP_RAISE("ect?");
				}
			}
			J40HIP_SHOULD(ec.bpp <= 16, "fbpp");
		}
		im->xyb_encoded = br.u(1);
		if (!br.u(1)) {  // ColourEncoding
			im->want_icc = br.u(1);
			int32_t cspace = br.enum_();
			J40HIP_SHOULD(cspace <= 3, "csp?");
			im->grey = cspace == 1;
			ColourEncoding &ce = im->cenc;
			ce.colour_space = cspace;
			if (!im->want_icc) {
				if (cspace != 2) {
					int32_t wp = br.enum_();
					J40HIP_SHOULD(wp == 1 || wp == 2 || wp == 10 || wp == 11, "wpt?");
					ce.white_point = wp;
					if (wp == 2) read_customxy(br, ce.white_xy); else enum_white_xy(wp, ce.white_xy);
					if (cspace != 1) {
						int32_t pr = br.enum_();
						J40HIP_SHOULD(pr == 1 || pr == 2 || pr == 9 || pr == 11, "prm?");
						ce.primaries = pr;
						if (pr == 2) { for (int i = 0; i < 3; ++i) read_customxy(br, ce.prim_xy[i]); } else enum_primaries_xy(pr, ce.prim_xy);
					}
				}
				if (br.u(1)) {
					int32_t gamma = (int32_t) br.u(24);
					J40HIP_SHOULD(gamma > 0 && gamma <= 10000000, "gama");
					if (cspace == 2) J40HIP_SHOULD(gamma == 3333333, "gama");
					ce.have_gamma = true; ce.gamma = gamma;
				} else {
					int32_t tf = br.enum_();
					J40HIP_SHOULD(tf == 1 || tf == 2 || tf == 8 || tf == 13 || tf == 16 || tf == 17 || tf == 18, "tfn?");
					ce.transfer = tf;
				}
				int32_t intent = br.enum_();
				J40HIP_SHOULD(intent <= 3, "itt?");
				ce.intent = intent;
			}
		}
		if (extra_fields) {
			if (!br.u(1)) {  // ToneMapping
				im->intensity_target = br.f16();
				J40HIP_SHOULD(im->intensity_target > 0, "tone");
				float min_nits = br.f16();
				J40HIP_SHOULD(0 < min_nits && min_nits <= im->intensity_target, "tone");
				bool relative = br.u(1);
				float linear_below = br.f16();
				if (relative) J40HIP_SHOULD(0 <= linear_below && linear_below <= 1, "tone");
				else J40HIP_SHOULD(0 <= linear_below, "tone");
			}
		}
		read_extensions(br);
	}
	if (!br.u(1)) {  // !default_m
		if (im->xyb_encoded) {
			for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) im->opsin_inv_mat[i][j] = br.f16();
			for (int i = 0; i < 3; ++i) im->opsin_bias[i] = br.f16();
			for (int i = 0; i < 3; ++i) im->quant_bias[i] = br.f16();
			im->quant_bias_num = br.f16();
		}
		// custom upsampling weights: up2_weight, up4_weight, up8_weight, each behind its bit of the mask (read with the switch alone)
		im->cw_mask = (int32_t) br.u(3);
		J40HIP_SHOULD(im->cw_mask == 0 || allow_upsampling, "TODO");
		static const int32_t COUNT[3] = {15, 55, 210};
		for (int t = 0; t < 3; ++t) if (im->cw_mask >> t & 1) {
			im->up_weights[t].resize((size_t) COUNT[t]);
			for (float &w : im->up_weights[t]) w = br.f16();
		}
	}
}

// ---- the default upsampling weights (frame.hpp) ----
static std::mutex g_up_defaults_mutex;
static std::vector<float> g_up_defaults[3];
static int up_table_index(int32_t k) { return k == 2 ? 0 : k == 4 ? 1 : k == 8 ? 2 : -1; }
bool set_upsampling_defaults(int32_t k, const float *w, int32_t n) {
	static const int32_t COUNT[3] = {15, 55, 210};
	const int t = up_table_index(k);
	if (t < 0 || (n != 0 && (!w || n != COUNT[t]))) return false;
	std::lock_guard<std::mutex> lock(g_up_defaults_mutex);
	if (n == 0) { g_up_defaults[t].clear(); return true; }   // (n = 0 takes the table back: frames parsed afterwards answer "updf" again)
	g_up_defaults[t].assign(w, w + n);
	return true;
}
bool get_upsampling_defaults(int32_t k, std::vector<float> *out) {
	const int t = up_table_index(k);
	if (t < 0) return false;
	std::lock_guard<std::mutex> lock(g_up_defaults_mutex);
	if (g_up_defaults[t].empty()) return false;
	*out = g_up_defaults[t];
	return true;
}

// ------------------------------------------------------------------------------------------------
// frame header (j40.h:5163)

// `sequence`: the frame belongs to a frame sequence, which refuses the types it does not serve as soon as it has read them
// `lf_frames`: ... and the sequence serves LF frames (type 1), `patches`: and reference-only frames (type 2)
// `upsampling`: upsampling is asked for (Frame::allow_upsampling; never for a sequence's frame, which stays "TODO")
static void read_frame_header(BitReader &br, const ImageMeta &im, FrameHeader *f, bool sequence = false, bool lf_frames = false, bool patches = false, bool upsampling = false) {
	f->width = im.width; f->height = im.height;
	f->ec_blend.assign(im.ec.size(), FrameHeader::Blend());
	br.zero_pad_to_byte();
	if (!br.u(1)) {
		bool full_frame = true;
		f->type = (int32_t) br.u(2);
		if (sequence) J40HIP_SHOULD(f->type == 0 || f->type == 3 || (lf_frames && f->type == 1) || (patches && f->type == 2), "TODO");
		f->is_modular = br.u(1);
		uint64_t flags = br.u64();
		f->has_noise = flags & 1; f->has_patches = flags >> 1 & 1; f->has_splines = flags >> 4 & 1;
		f->use_lf_frame = flags >> 5 & 1; f->skip_adapt_lf_smooth = flags >> 7 & 1;
		if (!im.xyb_encoded) f->do_ycbcr = br.u(1);
		if (!f->use_lf_frame) {
			if (f->do_ycbcr) {
				f->jpeg_upsampling = (int32_t) br.u(6);
				// (FrameHeader::hshift: the sampling factors of the three modes, coarser channels shifted against the finest)
				static const int8_t FACTOR[4][2] = {{1, 1}, {2, 2}, {2, 1}, {1, 2}};
				int maxh = 1, maxv = 1;
				for (int c = 0; c < 3; ++c) { const int8_t *m = FACTOR[(f->jpeg_upsampling >> (2 * c)) & 3]; maxh = std::max<int>(maxh, m[0]); maxv = std::max<int>(maxv, m[1]); }
				for (int c = 0; c < 3; ++c) { const int8_t *m = FACTOR[(f->jpeg_upsampling >> (2 * c)) & 3]; f->hshift[c] = (int8_t) (maxh / m[0] - 1); f->vshift[c] = (int8_t) (maxv / m[1] - 1); }
			}
			// upsampling and every extra channel's ec_upsampling (with the switch alone: the reference refuses both, j40.h:5244-5249)
			f->upsampling = 1 << (int32_t) br.u(2);
			J40HIP_SHOULD(f->upsampling == 1 || upsampling, "TODO");
			f->ec_upsampling.assign(im.ec.size(), 1);
			for (size_t i = 0; i < im.ec.size(); ++i) {
				f->ec_upsampling[i] = 1 << (int32_t) br.u(2);
				J40HIP_SHOULD(f->ec_upsampling[i] == 1 || upsampling, "TODO");
				J40HIP_SHOULD((f->ec_upsampling[i] << im.ec[i].dim_shift) >= f->upsampling, "usmp");   // (j40.h:3637)
			}
		}
		if (f->is_modular) f->group_size_shift = 7 + (int32_t) br.u(2);
		else if (im.xyb_encoded) { f->x_qm_scale = (int32_t) br.u(3); f->b_qm_scale = (int32_t) br.u(3); }
		if (f->type != 2) {
			f->num_passes = br.u32(1, 0, 2, 0, 3, 0, 4, 3);
			if (f->num_passes > 1) {
				int32_t num_ds = br.u32(0, 0, 1, 0, 2, 0, 3, 1), prev_ds = 4, ppass = 0;
				J40HIP_SHOULD(num_ds < f->num_passes, "pass");
				for (int32_t i = 0; i < f->num_passes - 1; ++i) (void) br.u(2);  // shift
				for (int32_t i = 0; i < num_ds; ++i) { int32_t ds = (int32_t) br.u(2); J40HIP_SHOULD(prev_ds >= ds, "pass"); prev_ds = ds; }
				for (int32_t i = 0; i < num_ds; ++i) {
					int32_t pass = br.u32(0, 0, 1, 0, 2, 0, 0, 3);
					J40HIP_SHOULD(i > 0 ? ppass < pass && pass < f->num_passes : pass == 0, "pass");
					ppass = pass;
				}
			}
		}
		if (f->type == 1) {
			// an LF frame: the image's size divided by 8, rounding up, once per level (no crop, no blend info, never last, saved nowhere)
			f->lf_level = (int32_t) br.u(2) + 1;
			for (int32_t l = 0; l < f->lf_level; ++l) { f->width = ceil_div(f->width, 8); f->height = ceil_div(f->height, 8); }
		} else if (br.u(1)) {  // have_crop
			if (f->type != 2) {
				f->x0 = unpack_signed(br.u32(0, 8, 256, 11, 2304, 14, 18688, 30));
				f->y0 = unpack_signed(br.u32(0, 8, 256, 11, 2304, 14, 18688, 30));
			}
			f->width = br.u32(0, 8, 256, 11, 2304, 14, 18688, 30);
			f->height = br.u32(0, 8, 256, 11, 2304, 14, 18688, 30);
			J40HIP_SHOULD(f->width <= (1 << 18) && f->height <= (1 << 18), "slim");
			J40HIP_SHOULD((int64_t) f->width * f->height <= (1 << 28), "slim");
			full_frame = f->x0 <= 0 && f->y0 <= 0 && f->width + f->x0 >= im.width && f->height + f->y0 >= im.height;
		}
		int32_t blend_mode0 = 0, save_as_ref = 0;
		int64_t duration = 0;
		if (f->type == 0 || f->type == 3) {
			for (int32_t i = -1; i < (int32_t) im.ec.size(); ++i) {
				FrameHeader::Blend &b = i < 0 ? f->blend : f->ec_blend[(size_t) i];
				int32_t mode = br.u32(0, 0, 1, 0, 2, 0, 3, 2);
				if (i < 0) blend_mode0 = mode;
				b.mode = (int8_t) mode;
				if (!im.ec.empty()) {
					if (mode == 2 || mode == 3) { b.alpha_chan = (int8_t) br.u32(0, 0, 1, 0, 2, 0, 3, 3); b.clamp = (int8_t) br.u(1); }
					else if (mode == 4) b.clamp = (int8_t) br.u(1);
				}
				if (!full_frame || mode != 0) b.src_ref = (int8_t) br.u(2);
			}
			if (im.have_animation) {
				duration = br.u32_64(0, 0, 1, 0, 0, 8, 0, 32);
				if (im.anim_have_timecodes) (void) br.u64bits(32);
			}
			f->is_last = br.u(1);
		} else {
			f->is_last = false;
		}
		if (f->type != 1 && !f->is_last) save_as_ref = (int32_t) br.u(2);
		if (f->type == 2 || (full_frame && (f->type == 0 || f->type == 3) && blend_mode0 == 0 && (duration == 0 || save_as_ref != 0) && !f->is_last)) f->save_before_ct = br.u(1);
		f->full_frame = full_frame; f->duration = duration; f->save_as_ref = save_as_ref;
		skip_name(br);
		{   // RestorationFilter. The reference reads the conditional fields even when all_default is
			// set (j40.h:5339-5366); a drop-in has to consume the same bits.
			FrameHeader::Restoration &rf = f->restoration;
			bool all_default = br.u(1);
			rf.gab = all_default ? true : br.u(1);
			if (rf.gab && br.u(1)) for (int i = 0; i < 3; ++i) for (int j = 0; j < 2; ++j) rf.gab_weights[i][j] = br.f16();
			rf.epf_iters = all_default ? 2 : (int32_t) br.u(2);
			if (rf.epf_iters) {
				if (!f->is_modular && br.u(1)) for (int i = 0; i < 8; ++i) rf.sharp_lut[i] = br.f16();
				if (br.u(1)) { for (int i = 0; i < 3; ++i) rf.channel_scale[i] = br.f16(); br.skip_bits_like_reference(32); }
				if (br.u(1)) { if (!f->is_modular) rf.quant_mul = br.f16(); rf.pass0_sigma_scale = br.f16(); rf.pass2_sigma_scale = br.f16(); rf.border_sad_mul = br.f16(); }
				if (f->is_modular) rf.sigma_for_modular = br.f16();
			}
			if (!all_default) read_extensions(br);
		}
		read_extensions(br);
	}
	// the header's size is the shown one; an upsampled frame is coded at ceil(shown / K), and from here on width and height mean that
	f->up_width = f->width; f->up_height = f->height;
	if (f->upsampling > 1) {
		J40HIP_SHOULD(!sequence, "TODO");   // (no frame of a sequence; a stand-alone frame of type 1 or 2 is refused by its caller whatever its upsampling)
		f->width = ceil_div(f->up_width, f->upsampling); f->height = ceil_div(f->up_height, f->upsampling);
	}
	// An extra channel coarser than the frame (ec_upsampling above upsampling; "usmp" has seen to the other way): a VarDCT frame's, which
	// is decoded at its own size and dropped (init_global_modular), up to four times coarser -- from eight times on its samples would
	// belong to the LfGroup sections. A Modular frame renders its alpha plane, which nothing stretches on its own: "TODO"
	for (int32_t e : f->ec_upsampling) J40HIP_SHOULD(e == f->upsampling || (!f->is_modular && e <= 4 * f->upsampling), "TODO");
	f->grows = ceil_div(f->height, 1 << f->group_size_shift);
	f->gcolumns = ceil_div(f->width, 1 << f->group_size_shift);
	f->num_groups = (int64_t) f->grows * f->gcolumns;
	f->ggrows = ceil_div(f->height, 8 << f->group_size_shift);
	f->ggcolumns = ceil_div(f->width, 8 << f->group_size_shift);
	f->num_lf_groups = (int64_t) f->ggrows * f->ggcolumns;
}

GroupInfo group_info(const FrameHeader &fh, int64_t gidx) {  // j40.h:7734
	GroupInfo g;
	const int32_t shift = fh.group_size_shift;
	int64_t row = gidx / fh.gcolumns, column = gidx % fh.gcolumns;
	g.ggidx = (int32_t) ((row / 8) * fh.ggcolumns + column / 8);
	g.gx_in_gg = (int32_t) (column % 8) << shift;
	g.gy_in_gg = (int32_t) (row % 8) << shift;
	g.gw = (int32_t) (std::min<int64_t>(fh.width, (column + 1) << shift) - (column << shift));
	g.gh = (int32_t) (std::min<int64_t>(fh.height, (row + 1) << shift) - (row << shift));
	return g;
}

// ------------------------------------------------------------------------------------------------
// TOC (j40.h:5479). The whole codestream is in memory, so sections are addressed directly; the
// reference's dependency reordering is a streaming concern and not needed.

static void read_toc(BitReader &br, const FrameHeader &fh, Toc *toc) {
	int64_t nsections = fh.num_passes == 1 && fh.num_groups == 1 ? 1 : 1 + fh.num_lf_groups + 1 + fh.num_passes * fh.num_groups;
	J40HIP_SHOULD(nsections <= INT32_MAX, "flen");
	std::vector<int32_t> lehmer;
	if (br.u(1)) {  // permuted
		CodeSpec spec;
		read_code_spec(br, 8, &spec);
		CodeState code(&spec);
		lehmer = read_permutation(br, code, (int32_t) nsections, 0);
		finish_code(br, code);
	}
	br.zero_pad_to_byte();
	std::vector<Section> sections((size_t) nsections);
	for (Section &s : sections) s.size = (size_t) br.u32(0, 10, 1024, 14, 17408, 22, 4211712, 30);
	br.zero_pad_to_byte();
	size_t off = br.byte_position();
	for (Section &s : sections) { s.offset = off; off += s.size; }
	toc->first_offset = sections.empty() ? off : sections[0].offset;
	toc->end_offset = off;
	if (nsections == 1) { toc->single = true; toc->single_section = sections[0]; return; }
	if (!lehmer.empty()) apply_permutation(sections.data(), lehmer);
	toc->lf_global = sections[0];
	toc->lf_groups.assign(sections.begin() + 1, sections.begin() + 1 + fh.num_lf_groups);
	toc->hf_global = sections[(size_t) (1 + fh.num_lf_groups)];
	toc->pass_groups.assign(sections.begin() + 2 + fh.num_lf_groups, sections.end());
	// (the largest end, not the last listed: a permuted TOC may store an LfGroup section behind pass groups)
	toc->lf_end = toc->lf_global.offset + toc->lf_global.size;
	for (const Section &s : toc->lf_groups) toc->lf_end = std::max(toc->lf_end, s.offset + s.size);
}

// ------------------------------------------------------------------------------------------------
// LfGlobal (j40.h:6257)

static void init_global_modular(Frame *f) {  // j40.h:3619
	const ImageMeta &im = f->im; const FrameHeader &fh = f->fh;
	int32_t n = (int32_t) im.ec.size();
	if (fh.is_modular) n += (!fh.do_ycbcr && !im.xyb_encoded && im.grey) ? 1 : 3;
	f->gmodular.channel.assign((size_t) n, Plane());
	for (size_t i = 0; i < im.ec.size(); ++i) J40HIP_SHOULD(im.ec[i].dim_shift == 0, "TODO");
	for (Plane &p : f->gmodular.channel) { p.width = fh.width; p.height = fh.height; }
	// (PARITY UNPINNED, device/upsample_dev.h) extra channel i is coded at ceil(shown / ec_upsampling[i]); where that is coarser than the
	// frame its groups hold the frame's group rectangles shifted down by log2(ec_upsampling[i] / upsampling), like a squeezed channel's
	for (size_t i = 0; i < im.ec.size() && i < fh.ec_upsampling.size(); ++i) if (fh.ec_upsampling[i] > fh.upsampling) {
		Plane &p = f->gmodular.channel[f->gmodular.channel.size() - im.ec.size() + i];
		int32_t s = 0;
		while ((fh.upsampling << s) < fh.ec_upsampling[i]) ++s;
		p.width = ceil_div(fh.shown_width(), fh.ec_upsampling[i]); p.height = ceil_div(fh.shown_height(), fh.ec_upsampling[i]);
		p.hshift = p.vshift = (int8_t) s;
	}
	f->gmodular.bpp = im.bpp;
}

// LfGlobal's front: the patch dictionary, the splines, the noise parameters, the LF dequantisation and, for a VarDCT frame, the quantiser,
// the block contexts and the LF channel correlation -- as far as the spline segments need it. A sequence's index reads this much of a
// frame with splines (parse_sequence_splines); read_lf_global goes on with the global Modular image.
static void read_lf_global_front(BitReader &br, Frame *f) {
	const FrameHeader &fh = f->fh;
	J40HIP_SHOULD((!fh.has_patches || f->allow_patches) && (!fh.has_splines || f->allow_splines) && (!fh.has_noise || f->allow_noise), "TODO");
	// (splines likewise go onto the XYB samples of a frame that is shown as it is, and an LF image holds none of them)
	if (fh.has_splines) J40HIP_SHOULD(f->im.xyb_encoded && fh.type != 1 && fh.type != 2 && !f->lf_only, "TODO");
	// (noise goes onto the XYB samples of a frame that is shown as it is: not an LF frame's, not a reference-only frame's)
	// (... and not an LF-only parse: the LF image of such a frame is not its preview)
	if (fh.has_noise) J40HIP_SHOULD(f->im.xyb_encoded && fh.type != 1 && fh.type != 2 && !f->lf_only, "TODO");
	if (fh.has_patches) {   // the dictionary, ahead of everything else (the splines follow it, then the noise parameters)
		J40HIP_SHOULD(f->im.xyb_encoded && fh.type != 2 && fh.type != 1, "TODO");
		read_patch_dictionary(br, f->im, fh, &f->patches);
		J40HIP_SHOULD(!f->patches.unserved, "TODO");
	}
	if (fh.has_splines) read_splines(br, fh, &f->splines);
	if (fh.has_noise) for (int i = 0; i < 8; ++i) f->noise_lut[i] = (float) br.u(10) / 1024.0f;   // NoiseParameters
	if (!br.u(1)) for (int i = 0; i < 3; ++i) f->m_lf_scaled[i] = br.f16() / 128.0f;
	if (!fh.is_modular) {
		f->global_scale = br.u32(1, 11, 2049, 11, 4097, 12, 8193, 16);
		f->quant_lf = br.u32(16, 0, 1, 5, 1, 8, 1, 16);
		if (br.u(1)) {
			static const uint8_t DEFAULT_MAP[39] = {0, 1, 2, 2, 3, 3, 4, 5, 6, 6, 6, 6, 6, 7, 8, 9, 9, 10, 11, 12, 13, 14, 14, 14, 14, 14, 7, 8, 9, 9, 10, 11, 12, 13, 14, 14, 14, 14, 14};
			f->block_ctx_map.assign(DEFAULT_MAP, DEFAULT_MAP + 39);
			f->nb_block_ctx = 15;
		} else {
			int32_t size = 39;
			for (int i = 0; i < 3; ++i) {
				f->nb_lf_thr[i] = (int32_t) br.u(4);
				for (int32_t j = 0; j < f->nb_lf_thr[i]; ++j) f->lf_thr[i][j] = (int32_t) unpack_signed64(br.u32_64(0, 4, 16, 8, 272, 16, 65808, 32));
				size *= f->nb_lf_thr[i] + 1;
			}
			f->nb_qf_thr = (int32_t) br.u(4);
			for (int32_t i = 0; i < f->nb_qf_thr; ++i) f->qf_thr[i] = br.u32(0, 2, 4, 3, 12, 5, 44, 8) + 1;
			size *= f->nb_qf_thr + 1;
			J40HIP_SHOULD(size <= 39 * 64, "hfbc");
			read_cluster_map(br, size, 16, &f->nb_block_ctx, &f->block_ctx_map);
		}
		if (!br.u(1)) {
			f->inv_colour_factor = 1.0f / (float) br.u32(84, 0, 256, 0, 2, 8, 258, 16);
			f->base_corr_x = br.f16();
			f->base_corr_b = br.f16();
			f->x_factor_lf = (int32_t) br.u(8) - 127;
			f->b_factor_lf = (int32_t) br.u(8) - 127;
		}
	}
	if (fh.has_splines) {   // the segments every decode draws and their tiles, now that the base correlations are known (device/spline_dev.h)
		J40HIP_SHOULD(spline_segments(f->splines, f->base_corr_x, f->base_corr_b, fh.width, fh.height, &f->spline_plan.segs), "spln");
		J40HIP_SHOULD(spline_bin(fh.width, &f->spline_plan), "spln");
	}
}

static void read_lf_global(BitReader &br, Frame *f) {
	const FrameHeader &fh = f->fh;
	read_lf_global_front(br, f);
	init_global_modular(f);
	if (br.u(1)) {  // global tree
		// tree size limit with the reference's saturating 32-bit products (j40.h:6321-6322)
		int64_t area = std::min<int64_t>((int64_t) fh.width * fh.height, INT32_MAX);
		int64_t prod = std::min<int64_t>(area * (int64_t) f->gmodular.channel.size(), INT32_MAX);
		int64_t limit = std::min<int64_t>(1 << 22, 1024 + prod / 16);
		read_tree(br, (int32_t) limit, 64, &f->global_tree, &f->global_codespec);
	}
	if (!f->gmodular.channel.empty()) {
		read_modular_header(br, &f->global_tree, &f->global_codespec, &f->gmodular);
		// LfGlobal codes the meta channels and the channels behind them that fit into one group; the rest is left to the
		// LfGroup / pass-group sections. Without Squeeze that is the reference's rule (every channel of a frame no larger
		// than a group, else the meta channels only, j40.h:6329-6333); after a Squeeze the small channels qualify too
		{
			const int32_t gdim = 1 << fh.group_size_shift, nch = (int32_t) f->gmodular.channel.size();
			int32_t n = f->gmodular.nb_meta_channels;
			while (n < nch && f->gmodular.channel[(size_t) n].width <= gdim && f->gmodular.channel[(size_t) n].height <= gdim) ++n;
			f->num_gm_channels = n;
		}
		if (!fh.is_modular) {
			// A squeezed extra-channel image of a VarDCT frame that is not finished inside LfGlobal would need the ModularLfGroup data
			// between the LF coefficients and the HF metadata of every LfGroup section and shift-aware sub-images behind the
			// coefficients of every pass group; neither exists here, and the reference stops at the Squeeze parameters (j40.h:3812)
			bool squeezed = false;
			for (const Transform &t : f->gmodular.transforms) squeezed = squeezed || t.kind == Transform::SQUEEZE;
			J40HIP_SHOULD(!squeezed || f->num_gm_channels == (int32_t) f->gmodular.channel.size(), "TODO");
			allocate_modular(&f->gmodular);   // (Modular frames are decoded on the device: no host planes)
		}
		if (fh.is_modular) {
			// the channel data that follows (j40.h:6334-6337) is decoded by the HIP Modular kernel, which
			// continues from this bit position inside the section
			f->gm_data_bitpos = br.bit_position();
			f->gm_data_pending = true;
			return;
		}
		CodeState code(f->gmodular.codespec);
		for (int32_t i = 0; i < f->num_gm_channels; ++i) decode_modular_channel(br, f->gmodular, code, i, 0);
		finish_code(br, code);
	}
}

// ------------------------------------------------------------------------------------------------
// HfGlobal + HfPass (j40.h:6819)

static void read_dq_matrix(BitReader &br, int32_t idx, int64_t raw_sidx, Frame *f) {  // j40.h:4696
	DqMatrix &dq = f->dq_matrix[idx];
	static const int8_t LOGDIM[17][2] = {{3, 3}, {3, 3}, {3, 3}, {3, 3}, {4, 4}, {5, 5}, {3, 4}, {3, 5}, {4, 5}, {3, 3}, {3, 3}, {6, 6}, {5, 6}, {7, 7}, {6, 7}, {8, 8}, {7, 8}};
	const int32_t nrows = 1 << LOGDIM[idx][0], ncols = 1 << LOGDIM[idx][1];
	dq.mode = (int32_t) br.u(3);
	dq.params.clear();
	if (dq.mode == 7) {  // raw: coded as a 3-channel Modular image
		float denom = br.f16();
		J40HIP_SHOULD(std::isfinite(denom) && std::fabs(denom) >= 1e-8f, "dqm0");
		float inv_denom = 1.0f / denom;
		Modular m;
		m.bpp = f->im.bpp;
		m.channel.assign(3, Plane());
		for (Plane &p : m.channel) { p.width = ncols; p.height = nrows; }
		decode_modular_image(br, &f->global_tree, &f->global_codespec, raw_sidx, &m);
		dq.params.assign((size_t) (nrows * ncols), std::array<float, 3>{0, 0, 0});
		for (int c = 0; c < 3; ++c) for (int32_t i = 0; i < nrows * ncols; ++i) dq.params[(size_t) i][(size_t) c] = (float) m.channel[(size_t) c].px[(size_t) i] * inv_denom;
		dq.n = nrows; dq.m = ncols;
	} else {
		static const struct { int8_t needs8x8, nparams, nscaled, ndct; } HOW[7] = {{0, 0, 0, 0}, {1, 3, 3, 0}, {1, 6, 6, 0}, {1, 2, 2, 1}, {1, 1, 0, 1}, {1, 9, 6, 2}, {1, 0, 0, 1}};
		const auto how = HOW[dq.mode];
		if (how.needs8x8) J40HIP_SHOULD(nrows == 8 && ncols == 8, "dqm?");
		int32_t paramsize = how.nparams + how.ndct * 16, at = how.nparams;
		if (paramsize) {
			dq.params.assign((size_t) paramsize, std::array<float, 3>{0, 0, 0});
			for (int c = 0; c < 3; ++c) for (int32_t j = 0; j < how.nparams; ++j) dq.params[(size_t) j][(size_t) c] = br.f16() * (j < how.nscaled ? 64.0f : 1.0f);
			for (int32_t i = 0; i < how.ndct; ++i) {
				int32_t n = (int32_t) br.u(4) + 1;
				(i == 0 ? dq.n : dq.m) = n;
				for (int c = 0; c < 3; ++c) for (int32_t j = 0; j < n; ++j) dq.params[(size_t) (at + j)][(size_t) c] = br.f16() * (j == 0 ? 64.0f : 1.0f);
				at += n;
			}
		}
	}
}

static void read_hf_global(BitReader &br, Frame *f) {
	const FrameHeader &fh = f->fh;
	const int64_t sidx_base = 1 + 3 * fh.num_lf_groups;
	if (!br.u(1)) for (int32_t i = 0; i < 17; ++i) read_dq_matrix(br, i, sidx_base + i, f);
	f->num_hf_presets = (int32_t) br.u(ceil_lg32((uint32_t) fh.num_groups)) + 1;
	for (int32_t pass = 0; pass < fh.num_passes; ++pass) {
		int32_t used_orders = br.u32(0x5f, 0, 0x13, 0, 0, 0, 0, 13);
		if (used_orders > 0) {
			CodeSpec spec;
			read_code_spec(br, 8, &spec);
			CodeState code(&spec);
			for (int32_t j = 0; j < 13; ++j) if (used_orders >> j & 1) {
				int32_t size = 1 << (LOG_ORDER_SIZE[j][0] + LOG_ORDER_SIZE[j][1]);
				for (int c = 0; c < 3; ++c) { f->order_lehmer[pass][j][c] = read_permutation(br, code, size, size / 64); f->order_has_lehmer[pass][j][c] = true; }
			}
			finish_code(br, code);
		}
		read_code_spec(br, 495 * f->nb_block_ctx * f->num_hf_presets, &f->coeff_codespec[pass]);
	}
}

// ------------------------------------------------------------------------------------------------
// LfGroup (j40.h:6492-6790)

static void smooth_lf(const Frame &f, int32_t w8, int32_t h8, std::vector<float> lfq[3]) {  // j40.h:6492
	static const float W0 = 0.05226273532324128f, W1 = 0.20345139757231578f, W2 = 0.0334829185968739f;
	float inv_m_lf[3];
	for (int c = 0; c < 3; ++c) inv_m_lf[c] = (float) (f.global_scale * f.quant_lf) / f.m_lf_scaled[c] / 65536.0f;
	if (h8 < 3 || w8 < 3) return;
	std::vector<float> prev[3], cur[3];
	for (int c = 0; c < 3; ++c) { cur[c].assign(lfq[c].begin(), lfq[c].begin() + w8); prev[c].resize((size_t) w8); }
	for (int32_t y = 1; y < h8 - 1; ++y) {
		float *out[3]; const float *south[3];
		for (int c = 0; c < 3; ++c) {
			prev[c].swap(cur[c]);
			out[c] = lfq[c].data() + (size_t) y * (size_t) w8;
			south[c] = out[c] + w8;
			cur[c].assign(out[c], out[c] + w8);  // unsmoothed copy of this row
		}
		for (int32_t x = 1; x < w8 - 1; ++x) {
			float wa[3], gap = 0.5f;
			for (int c = 0; c < 3; ++c) {
				const float *n = prev[c].data(), *l = cur[c].data(), *s = south[c];
				wa[c] = (n[x - 1] * W2 + n[x] * W1 + n[x + 1] * W2) + (l[x - 1] * W1 + l[x] * W0 + l[x + 1] * W1) + (s[x - 1] * W2 + s[x] * W1 + s[x + 1] * W2);
				float diff = fabsf(wa[c] - l[x]) * inv_m_lf[c];
				if (gap < diff) gap = diff;
			}
			gap = 3.0f - 4.0f * gap;
			gap = 0.0f > gap ? 0.0f : gap;
			for (int c = 0; c < 3; ++c) out[c][x] = (wa[c] - cur[c][(size_t) x]) * gap + cur[c][(size_t) x];
		}
	}
}

// the LF image of an LfGroup: dequantisation (j40.h:6562) and adaptive smoothing (j40.h:6492) of the decoded integers
static void lf_samples(const Frame &f, const LfGroup &gg, std::vector<float> lfq[3]) {
	const int32_t w8 = gg.width8, h8 = gg.height8;
	for (int c = 0; c < 3; ++c) {
		lfq[c].resize((size_t) w8 * (size_t) h8);
		for (size_t i = 0; i < lfq[c].size(); ++i) lfq[c][i] = (float) gg.lfraw[c][i] * gg.mult_lf[c];
	}
	if (!f.fh.skip_adapt_lf_smooth) smooth_lf(f, w8, h8, lfq);
}

bool lf_plane(const Frame &f, int c, float *out) {
	const size_t w8 = (size_t) ceil_div(f.fh.width, 8);
	std::vector<float> lfq[3];
	for (const LfGroup &gg : f.lf_groups) if (gg.lfraw[0].size() != (size_t) gg.width8 * (size_t) gg.height8) return false;
	for (const LfGroup &gg : f.lf_groups) {
		lf_samples(f, gg, lfq);
		for (int32_t y = 0; y < gg.height8; ++y)
			std::copy(lfq[c].begin() + (long) y * gg.width8, lfq[c].begin() + (long) (y + 1) * gg.width8, out + (size_t) (gg.top / 8 + y) * w8 + (size_t) (gg.left / 8));
	}
	return true;
}

// the tail of an LfGroup: its LF image (lf_samples), LLF coefficients of every varblock (j40.h:6668-6683, 5944) from that and the
// varblock layout. The device does the same at upload (device/lf_tail_kernels: k_lf_dequant_smooth, k_llf) when Frame::defer_lf_tail is set.
static void lf_tail_on_host(const Frame &f, LfGroup *gg) {
	if (!gg->tail_pending) return;
	const int32_t w8 = gg->width8, h8 = gg->height8;
	std::vector<float> lfq[3];
	lf_samples(f, *gg, lfq);
	for (int c = 0; c < 3; ++c) gg->llfcoeffs[c].assign((size_t) w8 * (size_t) h8, 0.0f);
	std::vector<float> scratch(1024);
	for (const VarblockInfo &vb : gg->varblocks) {
		const DctSelect &dct = DCT_SELECT[vb.dctsel];
		const int32_t vw8 = 1 << (dct.log_columns - 3), vh8 = 1 << (dct.log_rows - 3), coeffoff = vb.coeffoff_qfidx & ~15;
		for (int c = 0; c < 3; ++c) {
			float *llf = gg->llfcoeffs[c].data() + (coeffoff >> 6);
			for (int32_t i = 0; i < vh8; ++i) for (int32_t j = 0; j < vw8; ++j) llf[i * vw8 + j] = lfq[c][(size_t) (vb.y8 + i) * (size_t) w8 + (size_t) (vb.x8 + j)];
			if (vw8 > 1 || vh8 > 1) forward_dct2d_scaled_for_llf(llf, scratch.data(), dct.log_rows - 3, dct.log_columns - 3);
		}
	}
	gg->tail_pending = false;
}
void finish_lf_tail(Frame *f) { for (LfGroup &gg : f->lf_groups) if (gg.loaded) lf_tail_on_host(*f, &gg); }

// what follows the two Modular sub-images of an LfGroup section (j40.h:6562-6570, 6634-6688): dequantisation factors, LF index,
// varblock placement. lf: the LF integers in streamed order Y, X, B (moved into gg->lfraw when `take` is given, else copied)
static void lf_group_finish(Frame *f, LfGroup *gg, int32_t extra_prec, const int16_t *const lf[3], std::vector<int16_t> *take[3],
		const int16_t *xfromy, const int16_t *bfromy, const int16_t *info0, const int16_t *info1, int32_t nb_varblocks) {
	const FrameHeader &fh = f->fh;
	const int32_t w8 = gg->width8, h8 = gg->height8, w64 = gg->width64, h64 = gg->height64;
	const size_t cells = (size_t) w8 * (size_t) h8;
	static const int XYB_FROM_STREAM[3] = {1, 0, 2};
	const int16_t *ch[3];
	for (int c = 0; c < 3; ++c) {
		gg->mult_lf[c] = f->m_lf_scaled[c] / (float) (f->global_scale * f->quant_lf) * (float) (65536 >> extra_prec);  // j40.h:6562
		ch[c] = lf[XYB_FROM_STREAM[c]];
	}
	// A YCbCr frame with subsampled channels (PARITY UNPINNED, FrameHeader::hshift): channel c's LF image is (w8 >> hshift) x (h8 >> vshift).
	// Everything behind this point works on the full grid, so each channel is spread over it: the sample of (x, y) goes to cell
	// (x << hshift, y << vshift), the one cell of its MCU where the channel has a block, and for the LF index -- which stays on the
	// full grid -- to every cell it covers. With DCT8 alone and no smoothing (ycbcr_scope) a block's LLF coefficient is its cell's sample.
	std::vector<int16_t> spread[3], covered[3];
	const bool subsampled = fh.subsampled();
	if (subsampled) {
		for (int c = 0; c < 3; ++c) {
			const int32_t hs = fh.hshift[c], vs = fh.vshift[c], cw = w8 >> hs;
			spread[c].assign(cells, 0); covered[c].resize(cells);
			for (int32_t y = 0; y < h8; ++y) for (int32_t x = 0; x < w8; ++x) covered[c][(size_t) y * (size_t) w8 + (size_t) x] = ch[c][(size_t) (y >> vs) * (size_t) cw + (size_t) (x >> hs)];
			for (int32_t y = 0; y < (h8 >> vs); ++y) for (int32_t x = 0; x < cw; ++x) spread[c][(size_t) (y << vs) * (size_t) w8 + (size_t) (x << hs)] = ch[c][(size_t) y * (size_t) cw + (size_t) x];
			ch[c] = covered[c].data();
		}
		take = nullptr;
	}
	// LF index: thresholds counted on the raw integers; note each factor is a channel's own threshold count (j40.h:6566-6570)
	gg->lfindices.assign(cells, 0);
	auto add = [&](const int16_t *p, const int32_t *thr, int32_t n) { for (int32_t t = 0; t < n; ++t) for (size_t i = 0; i < cells; ++i) gg->lfindices[i] = (uint8_t) (gg->lfindices[i] + (p[i] > thr[t])); };
	auto mul = [&](int32_t k) { if (k != 1) for (uint8_t &v : gg->lfindices) v = (uint8_t) (v * k); };
	add(ch[0], f->lf_thr[0], f->nb_lf_thr[0]); mul(f->nb_lf_thr[0] + 1);
	add(ch[2], f->lf_thr[2], f->nb_lf_thr[2]); mul(f->nb_lf_thr[2] + 1);
	add(ch[1], f->lf_thr[1], f->nb_lf_thr[1]);
	for (int c = 0; c < 3; ++c) {
		if (take) gg->lfraw[c].swap(*take[XYB_FROM_STREAM[c]]);
		else if (subsampled) gg->lfraw[c].swap(spread[c]);
		else gg->lfraw[c].assign(ch[c], ch[c] + cells);
	}
	gg->tail_pending = true;
	gg->xfromy.assign(xfromy, xfromy + (size_t) w64 * (size_t) h64); gg->bfromy.assign(bfromy, bfromy + (size_t) w64 * (size_t) h64);

	// place varblocks in raster order at the first free cell (j40.h:6634-6688)
	const int32_t log_gsize8 = fh.group_size_shift - 3;
	gg->blocks.assign(cells, 0);
	gg->varblocks.clear(); gg->varblocks.reserve((size_t) nb_varblocks);   // (filled in placement order below: no need to zero 20 bytes per block first)
	int32_t voff = 0, coeffoff = 0;
	uint32_t dct_used = 0, order_used = 0;
	for (int32_t y0 = 0; y0 < h8; ++y0) for (int32_t x0 = 0; x0 < w8; ++x0) {
		if (gg->blocks[(size_t) y0 * (size_t) w8 + (size_t) x0]) continue;
		J40HIP_SHOULD(voff < nb_varblocks, "vblk");
		const int32_t dctsel = info0[voff];
		J40HIP_SHOULD(0 <= dctsel && dctsel < 27, "dct?");
		const DctSelect &dct = DCT_SELECT[dctsel];
		dct_used |= 1u << dctsel; order_used |= 1u << dct.order_idx;
		const int32_t vw8 = 1 << (dct.log_columns - 3), vh8 = 1 << (dct.log_rows - 3);
		const int32_t x1 = x0 + vw8 - 1, y1 = y0 + vh8 - 1;
		J40HIP_SHOULD(x1 < w8 && (x0 >> log_gsize8) == (x1 >> log_gsize8), "vblk");
		J40HIP_SHOULD(y1 < h8 && (y0 >> log_gsize8) == (y1 >> log_gsize8), "vblk");
		// (the reference does not check this, see its note at j40.h:6691: blocks overlapping earlier ones can add up to more cells
		// than the LfGroup has, and it then writes past its coefficient arrays; same check as device/plan_dev.h)
		J40HIP_SHOULD((size_t) coeffoff + ((size_t) 1 << (dct.log_columns + dct.log_rows)) <= cells * 64, "vblk");
		for (int32_t i = 0; i < vh8; ++i) for (int32_t j = 0; j < vw8; ++j) gg->blocks[(size_t) (y0 + i) * (size_t) w8 + (size_t) (x0 + j)] = 1 << 20 | voff;
		gg->blocks[(size_t) y0 * (size_t) w8 + (size_t) x0] = (dctsel + 2) << 20 | voff;
		gg->varblocks.push_back(VarblockInfo());
		VarblockInfo &vb = gg->varblocks.back();
		vb.coeffoff_qfidx = coeffoff; vb.x8 = x0; vb.y8 = y0; vb.dctsel = dctsel;
		const int32_t hfmul_m1 = info1[voff];
		for (int32_t j = 0; j < f->nb_qf_thr; ++j) vb.coeffoff_qfidx += hfmul_m1 >= f->qf_thr[j];
		vb.hfmul_inv = 1.0f / ((float) hfmul_m1 + 1.0f);
		coeffoff += 1 << (dct.log_columns + dct.log_rows);
		++voff;
	}
	J40HIP_SHOULD(voff == nb_varblocks, "vblk");
	gg->loaded = true;
	if (!f->defer_lf_tail) lf_tail_on_host(*f, gg);
	static std::mutex mu;
	std::lock_guard<std::mutex> lock(mu);
	f->dct_select_used |= dct_used; f->order_used |= order_used;
}

// the streams of an LfGroup section (j40.h:6722-6790) as decoded, nothing derived yet
void read_lf_group_raw(BitReader &br, const Frame &f, const LfGroup &gg, LfRaw *out) {
	const FrameHeader &fh = f.fh;
	const int64_t sidx0 = 1 + gg.idx, sidx2 = 1 + 2 * fh.num_lf_groups + gg.idx;
	const int32_t w8 = gg.width8, h8 = gg.height8, w64 = gg.width64, h64 = gg.height64;
	// (use_lf_frame: refused as the reference refuses it, j40.h:6763, unless LF frames are asked for -- Frame::allow_lf_frame)
	J40HIP_SHOULD(!fh.use_lf_frame || (f.allow_lf_frame && !fh.do_ycbcr), "TODO");
	// (jpeg_upsampling: refused as the reference refuses it, j40.h:6749, unless YCbCr frames are asked for -- Frame::allow_ycbcr)
	J40HIP_SHOULD(fh.jpeg_upsampling == 0 || f.allow_ycbcr, "TODO");
	J40HIP_SHOULD(fh.layout_served(), "TODO");   // (a layout other than 4:4:4, 4:2:0, 4:2:2, 4:4:0: FrameHeader::layout_served)

	// LF image: three channels in Y, X, B order, each at its own size where the frame subsamples (FrameHeader::hshift)
	// With use_lf_frame neither extra_precision nor the stream is there: the section starts at nb_varblocks (j40.h:6747, 6766), out->lf stays empty
	static const int SLOT_OF_STREAM[3] = {1, 0, 2};
	Modular lfm; lfm.bpp = f.im.bpp;
	out->extra_prec = 0;
	if (!fh.use_lf_frame) {
		out->extra_prec = (int32_t) br.u(2);
		lfm.channel.assign(3, Plane());
		for (int c = 0; c < 3; ++c) { Plane &p = lfm.channel[(size_t) c]; p.width = w8 >> fh.hshift[SLOT_OF_STREAM[c]]; p.height = h8 >> fh.vshift[SLOT_OF_STREAM[c]]; }
		decode_modular_image(br, &f.global_tree, &f.global_codespec, sidx0, &lfm);
		for (int c = 0; c < 3; ++c) J40HIP_SHOULD(lfm.channel[(size_t) c].width == w8 >> fh.hshift[SLOT_OF_STREAM[c]] && lfm.channel[(size_t) c].height == h8 >> fh.vshift[SLOT_OF_STREAM[c]], "TODO");
	}

	// HF metadata
	const int32_t nb_varblocks = (int32_t) br.u(ceil_lg32((uint32_t) (w8 * h8))) + 1;
	Modular m; m.bpp = f.im.bpp;
	m.channel.assign(4, Plane());
	m.channel[0].width = m.channel[1].width = w64; m.channel[0].height = m.channel[1].height = h64;
	m.channel[2].width = nb_varblocks; m.channel[2].height = 2;
	m.channel[3].width = w8; m.channel[3].height = h8;
	decode_modular_image(br, &f.global_tree, &f.global_codespec, sidx2, &m);
	J40HIP_SHOULD(m.channel.size() == 4 && m.channel[2].width == nb_varblocks && m.channel[2].height == 2, "TODO");
	J40HIP_SHOULD((int32_t) m.channel[0].px.size() == w64 * h64 && (int32_t) m.channel[1].px.size() == w64 * h64, "TODO");
	out->nb_varblocks = nb_varblocks;
	for (int c = 0; c < 3; ++c) { out->lf[c].clear(); if (!fh.use_lf_frame) out->lf[c].swap(lfm.channel[(size_t) c].px); }
	out->xfromy.swap(m.channel[0].px); out->bfromy.swap(m.channel[1].px); out->info.swap(m.channel[2].px); out->sharp.swap(m.channel[3].px);
}

static void read_lf_group(BitReader &br, Frame *f, LfGroup *gg) {  // j40.h:6722
	if (f->fh.is_modular) { gg->loaded = true; return; }  // nothing is read: no channel has shift >= 3 (j40.h:6731)
	LfRaw raw;
	read_lf_group_raw(br, *f, *gg, &raw);
	if (f->fh.use_lf_frame) {
		// the LF image comes from an LF frame's picture, on the device: the integers are zeros here (so are the LLF coefficients a host
		// tail makes of them), and every LF index is 0 until k_lf_from_frame has counted the thresholds on the samples
		for (int c = 0; c < 3; ++c) raw.lf[c].assign((size_t) gg->width8 * (size_t) gg->height8, 0);
	}
	const int16_t *lf[3] = {raw.lf[0].data(), raw.lf[1].data(), raw.lf[2].data()};
	std::vector<int16_t> *take[3] = {&raw.lf[0], &raw.lf[1], &raw.lf[2]};
	lf_group_finish(f, gg, raw.extra_prec, lf, take, raw.xfromy.data(), raw.bfromy.data(), raw.info.data(), raw.info.data() + raw.nb_varblocks, raw.nb_varblocks);
	gg->sharpness.swap(raw.sharp);
	if (f->fh.use_lf_frame) std::fill(gg->lfindices.begin(), gg->lfindices.end(), (uint8_t) 0);   // (a negative threshold counted the zeros)
}

static void allocate_lf_groups(Frame *f) {  // j40.h:7659
	const FrameHeader &fh = f->fh;
	const int32_t ggsize = 8 << fh.group_size_shift;
	f->lf_groups.assign((size_t) fh.num_lf_groups, LfGroup());
	int32_t idx = 0;
	for (int32_t ggy = 0; ggy < fh.height; ggy += ggsize) for (int32_t ggx = 0; ggx < fh.width; ggx += ggsize, ++idx) {
		LfGroup &gg = f->lf_groups[(size_t) idx];
		gg.idx = idx; gg.left = ggx; gg.top = ggy;
		gg.width = std::min(ggsize, fh.width - ggx); gg.height = std::min(ggsize, fh.height - ggy);
		gg.width8 = ceil_div(gg.width, 8); gg.height8 = ceil_div(gg.height, 8);
		gg.width64 = ceil_div(gg.width, 64); gg.height64 = ceil_div(gg.height, 64);
		if (fh.subsampled()) {
			// PARITY UNPINNED: the block grid of a subsampled frame is padded to whole MCUs; group and LfGroup counts stay the picture's
			const int32_t mh = fh.max_hshift(), mv = fh.max_vshift();
			const int32_t fw8 = ceil_div(fh.width, 8 << mh) << mh, fh8 = ceil_div(fh.height, 8 << mv) << mv;
			gg.width8 = std::min(ggsize / 8, fw8 - ggx / 8); gg.height8 = std::min(ggsize / 8, fh8 - ggy / 8);
			gg.width64 = ceil_div(gg.width8, 8); gg.height64 = ceil_div(gg.height8, 8);
		}
	}
}

uint32_t ycbcr_scope(const Frame &f) {
	const FrameHeader &fh = f.fh;
	if (fh.is_modular || !fh.do_ycbcr) return (uint32_t) E4("TODO");   // (nothing of this kind to serve)
	if (f.im.grey) return (uint32_t) E4("TODO");                       // a grey JPEG has one channel; how its frame is laid out is not known here
	if (f.im.exp_bits || f.im.bpp < 8) return (uint32_t) E4("TODO");    // float samples and depths below 8: what the pixel kernels refuse for any frame
	if (fh.use_lf_frame) return (uint32_t) E4("TODO");                 // LF frames are not served at all
	if (!fh.layout_served()) return (uint32_t) E4("TODO");             // (the parse has refused it already)
	if (fh.subsampled()) {
		if (!f.allow_ycbcr) return (uint32_t) E4("TODO");              // (parsed without the switch: cannot happen, the parse refuses)
		if (f.dct_select_used & ~1u) return (uint32_t) E4("TODO");     // a varblock other than DCT8: how a larger block meets a coarser channel's grid is not known here
		if (!fh.skip_adapt_lf_smooth) return (uint32_t) E4("TODO");    // the smoothing reads the three channels of a cell together: they are of different sizes
		if (fh.restoration.gab || fh.restoration.epf_iters > 0) return (uint32_t) E4("TODO");   // the filters run over full-size planes of all three channels
	}
	return 0;
}

static void prepare_tables(Frame *f) {  // j40.h:7694-7732
	for (int32_t i = 0; i < 27; ++i) if (f->dct_select_used >> i & 1) load_dq_matrix(DCT_SELECT[i].param_idx, &f->dq_matrix[DCT_SELECT[i].param_idx]);
	for (int32_t i = 0; i < 13; ++i) if (f->order_used >> i & 1) {
		const int32_t skip = 1 << (LOG_ORDER_SIZE[i][0] + LOG_ORDER_SIZE[i][1] - 6);
		for (int32_t pass = 0; pass < f->fh.num_passes; ++pass) for (int c = 0; c < 3; ++c) {
			std::vector<int32_t> &order = f->orders[pass][i][c];
			if (!order.empty()) continue;
			natural_order(LOG_ORDER_SIZE[i][0], LOG_ORDER_SIZE[i][1], &order);
			if (f->order_has_lehmer[pass][i][c]) apply_permutation(order.data() + skip, f->order_lehmer[pass][i][c]);
		}
	}
}

// ------------------------------------------------------------------------------------------------

// ICC stream (j40.h:3351-3393): like the reference, decoded and discarded -- the renderer always produces sRGB
static void skip_icc(BitReader &br) {
	const uint64_t enc_size = br.u64();
	CodeSpec spec;
	read_code_spec(br, 41, &spec);
	CodeState code(&spec);
	uint64_t index = 0, output_size = 0;
	{   // output size: a varint of bytes coded with context 0
		int32_t shift = 0;
		for (;;) {
			J40HIP_SHOULD(index++ < enc_size, "icc?");
			const int32_t b = decode_symbol(br, code, 0, 0);
			output_size |= (uint64_t) (b & 0x7f) << shift;
			if (b < 128) break;
			shift += 7;
			J40HIP_SHOULD(shift < 63, "vint");
		}
	}
	J40HIP_SHOULD(output_size <= ((uint64_t) 1 << 22), "plim");   // main profile, level 5 (j40.h:1172)
	J40HIP_SHOULD(output_size >= enc_size / 21, "icc?");
	int32_t byte = 0, prev = 0, pprev = 0;
	auto kind = [](int32_t v) { return (97 <= (v | 32) && (v | 32) <= 122) ? 0 : (v == 44 || v == 46 || (48 <= v && v < 58)) ? 1 : 4; };
	for (; index < enc_size; ++index) {
		pprev = prev; prev = byte;
		int32_t ctx = 0;
		if (index > 128) {
			if (prev < 16) ctx = prev < 2 ? prev + 3 : 5;
			else if (prev > 240) ctx = 6 + (prev == 255);
			else ctx = kind(prev) == 0 ? 1 : kind(prev) == 1 ? 2 : 8;
			ctx += 8 * (pprev < 16 ? 2 : pprev > 240 ? 3 : kind(pprev));
		}
		byte = decode_symbol(br, code, ctx, 0);
	}
	finish_code(br, code);
}

// signature, image and frame headers, TOC (sections clipped to the bytes that exist), the LfGroups' geometry
// `limit`: how much of the codestream's cs_size bytes may be read (streaming input: what has arrived; else cs_size)
static void read_image_header(BitReader &br, ImageMeta *im, bool allow_wide, bool allow_upsampling = false) {
	J40HIP_SHOULD(br.u(16) == 0x0aff, "!jxl");
	read_image_metadata(br, im, allow_wide, allow_upsampling);
	if (im->want_icc) skip_icc(br);
}
void parse_image_header(const uint8_t *cs, size_t cs_size, ImageMeta *im, size_t *first_frame, bool allow_wide, bool allow_upsampling) {
	BitReader br(cs, cs_size);
	read_image_header(br, im, allow_wide, allow_upsampling);
	br.zero_pad_to_byte();
	*first_frame = br.byte_position();
}
int32_t rendered_alpha_channel(const ImageMeta &im) {
	for (size_t i = 0; i < im.ec.size(); ++i) if (im.ec[i].type == EC_ALPHA) return (int32_t) i;
	return -1;
}
uint32_t sequence_refusal(const FrameHeader &fh, bool blend, int32_t alpha_ec, bool lf_frames, bool xyb, bool modular_lf, bool patches, bool modular_ref) {
	bool ok = (fh.type == 0 || fh.type == 3) && !fh.use_lf_frame;
	// (a reference-only frame: the XYB planes of a frame that decode_frame_xyb serves, saved before the colour transform)
	if (patches && fh.type == 2) ok = fh.save_before_ct && xyb && !fh.has_patches && !fh.use_lf_frame && !fh.do_ycbcr && (!fh.is_modular || modular_ref);
	if (lf_frames && (fh.type == 1 || fh.use_lf_frame)) ok = (fh.type == 0 || fh.type == 3 || (fh.type == 1 && (!fh.is_modular || (modular_lf && !fh.do_ycbcr)))) && xyb && !(fh.use_lf_frame && (fh.do_ycbcr || fh.is_modular))
		&& !(fh.type == 1 && !fh.ec_blend.empty());   // (an LF frame with extra channels behind its coefficients: nothing here keeps or checks them)
	if (!blend) {
		ok = ok && fh.blend.mode == 0;
		for (const FrameHeader::Blend &b : fh.ec_blend) ok = ok && b.mode == 0;
	} else if (!fh.ec_blend.empty()) {
		// (an image without extra channels codes no alpha_chan: every alpha is full scale)
		auto names_it = [&](const FrameHeader::Blend &b) { return (b.mode != 2 && b.mode != 3) || b.alpha_chan == alpha_ec; };
		ok = ok && names_it(fh.blend) && (alpha_ec < 0 || names_it(fh.ec_blend[(size_t) alpha_ec]));
	}
	return ok ? 0 : (uint32_t) E4("TODO");
}
void parse_sequence_frame_header(const uint8_t *cs, size_t cs_size, size_t offset, const ImageMeta &im, bool blend, bool lf_frames, FrameHeader *fh, Toc *toc, bool modular_lf, bool patches, bool modular_ref) {
	J40HIP_SHOULD(offset < cs_size, "shrt");
	BitReader br(cs + offset, cs_size - offset);
	read_frame_header(br, im, fh, true, lf_frames, patches);
	if (uint32_t e = sequence_refusal(*fh, blend, rendered_alpha_channel(im), lf_frames, im.xyb_encoded, modular_lf, patches, modular_ref)) raise(e);
	read_toc(br, *fh, toc);
}

// ------------------------------------------------------------------------------------------------
// the patch dictionary. PARITY UNPINNED: the reference stops at has_patches (j40.h:6262); this is the standard's layout as far as it
// can be recalled without the text. One entropy-coded stream over 10 contexts of hybrid integers: the number of
// reference patches (context 0); per reference patch its slot (1), x0 and y0 in the reference frame (3), width - 1 and height - 1 (2),
// count - 1 (7); per placement x and y -- the first one's as they are (4), a later one's as the sign-folded difference to the placement
// before (6) -- and once for each of num_extra_channels + 1 blend entries, the colour channels' first, the mode (5), an alpha channel
// (8; with mode >= 4 and more than one extra channel) and clamp (9; with mode >= 3).
void read_patch_dictionary(BitReader &br, const ImageMeta &im, const FrameHeader &fh, PatchDictionary *out) {
	*out = PatchDictionary();
	CodeSpec spec;
	read_code_spec(br, 10, &spec);
	CodeState code(&spec);
	auto get = [&](int32_t ctx) { return decode_symbol(br, code, ctx, 0); };
	// what a damaged stream can make the host allocate: as many reference patches as a frame of this size could hold, four placements each
	const int64_t max_ref = 1024 + (int64_t) fh.width * fh.height / 4, max_placements = 4 * max_ref;
	const int32_t num_ref = get(0);
	J40HIP_SHOULD(num_ref >= 0 && num_ref <= max_ref, "ptch");
	out->num_ref = num_ref;
	const size_t entries = im.ec.size() + 1;
	for (int32_t i = 0; i < num_ref; ++i) {
		PatchPlacement p;
		memset(&p, 0, sizeof p);
		p.source = i;
		p.ref = get(1);
		J40HIP_SHOULD(p.ref >= 0 && p.ref <= 3, "ptch");
		p.sx = get(3); p.sy = get(3);
		const int32_t w1 = get(2), h1 = get(2);
		J40HIP_SHOULD(p.sx >= 0 && p.sy >= 0 && w1 >= 0 && h1 >= 0 && w1 < (1 << 18) && h1 < (1 << 18) && p.sx < (1 << 18) && p.sy < (1 << 18), "ptch");   // (no reference frame is larger)
		p.w = w1 + 1; p.h = h1 + 1;
		const int32_t count1 = get(7);
		J40HIP_SHOULD(count1 >= 0 && (int64_t) out->placements.size() + count1 + 1 <= max_placements, "ptch");
		for (int32_t j = 0; j <= count1; ++j) {
			if (j == 0) { p.x = get(4); p.y = get(4); J40HIP_SHOULD(p.x >= 0 && p.y >= 0, "ptch"); }
			else {
				const int64_t x = (int64_t) p.x + unpack_signed(get(6)), y = (int64_t) p.y + unpack_signed(get(6));
				J40HIP_SHOULD(x >= 0 && y >= 0 && x <= INT32_MAX && y <= INT32_MAX, "ptch");   // a negative coordinate
				p.x = (int32_t) x; p.y = (int32_t) y;
			}
			J40HIP_SHOULD((int64_t) p.x + p.w <= fh.width && (int64_t) p.y + p.h <= fh.height, "ptch");   // the placement leaves the frame
			p.mode = 0; p.clamp = 0;
			for (size_t e = 0; e < entries; ++e) {
				const int32_t mode = get(5);
				J40HIP_SHOULD(mode >= 0 && mode <= 7, "ptch");
				int32_t clamp = 0;
				if (mode >= 4 && im.ec.size() > 1) { const int32_t a = get(8); J40HIP_SHOULD(a >= 0 && (size_t) a < im.ec.size(), "ptch"); }
				if (mode >= 3) { clamp = get(9); J40HIP_SHOULD(clamp == 0 || clamp == 1, "ptch"); }
				if (e == 0) { p.mode = mode; p.clamp = clamp; if (mode >= 4) out->unserved = true; }
				else if (mode != 0) out->unserved = true;
			}
			out->placements.push_back(p);
			out->slots |= 1u << p.ref;
		}
	}
	finish_code(br, code);
}

// ------------------------------------------------------------------------------------------------
// the splines. PARITY UNPINNED: the reference stops at has_splines (j40.h:6263); this is the standard's layout as far as it can be
// recalled without the text. One entropy-coded stream over 6 contexts of hybrid integers: the quantisation
// adjustment (context 0), starting positions (1), the number of splines - 1 (2), a spline's number of further control points (3), their
// double deltas (4), the DCT coefficients (5). Order: the count; every spline's starting point, the first as it is, a later one's as the
// sign-folded difference to the spline before; the adjustment, sign-folded; then per spline its number of control points, that many
// sign-folded pairs, and 3 x 32 colour coefficients (X, Y, B) and 32 sigma coefficients, sign-folded. "spln": more splines than
// min(1 << 24, W * H / 4), more control points than min(1 << 20, W * H / 2) in all, a starting coordinate of magnitude above 1 << 23 (the
// accumulated control points and the segments are bounded where they are made: spline_dev.h).
void read_splines(BitReader &br, const FrameHeader &fh, SplineData *out) {
	*out = SplineData();
	CodeSpec spec;
	read_code_spec(br, 6, &spec);
	CodeState code(&spec);
	auto get = [&](int32_t ctx) { return decode_symbol(br, code, ctx, 0); };
	const int64_t area = (int64_t) fh.width * fh.height, max_splines = std::min<int64_t>((int64_t) 1 << 24, area / 4), max_points = std::min<int64_t>((int64_t) 1 << 20, area / 2);
	const int64_t lim = (int64_t) 1 << 23;
	const int64_t num = (int64_t) (uint32_t) get(2) + 1;
	J40HIP_SHOULD(num <= max_splines, "spln");
	out->splines.resize((size_t) num);
	for (int64_t i = 0; i < num; ++i) {
		QuantSpline &q = out->splines[(size_t) i];
		const int32_t vx = get(1), vy = get(1);
		J40HIP_SHOULD(vx >= 0 && vy >= 0, "spln");
		if (i == 0) { q.x = vx; q.y = vy; }
		else { q.x = out->splines[(size_t) i - 1].x + unpack_signed(vx); q.y = out->splines[(size_t) i - 1].y + unpack_signed(vy); }
		J40HIP_SHOULD(q.x <= lim && q.x >= -lim && q.y <= lim && q.y >= -lim, "spln");
	}
	const int32_t qa = get(0);
	J40HIP_SHOULD(qa >= 0, "spln");
	out->quant_adjust = unpack_signed(qa);
	int64_t points = 0;
	for (int64_t i = 0; i < num; ++i) {
		QuantSpline &q = out->splines[(size_t) i];
		const int32_t n = get(3);
		J40HIP_SHOULD(n >= 0 && (points += n) <= max_points, "spln");
		q.dd.resize((size_t) n * 2);
		for (int64_t &d : q.dd) { const int32_t v = get(4); J40HIP_SHOULD(v >= 0, "spln"); d = unpack_signed(v); }
		for (int c = 0; c < 4; ++c) for (int k = 0; k < 32; ++k) { const int32_t v = get(5); J40HIP_SHOULD(v >= 0, "spln"); q.coef[c][k] = unpack_signed(v); }
	}
	finish_code(br, code);
}

void parse_sequence_patches(const uint8_t *cs, size_t cs_size, size_t offset, const ImageMeta &im, const FrameHeader &fh, const Toc &toc, PatchDictionary *out) {
	// LfGlobal: the frame's one section (read to the end of the codestream, as parse_frame reads it), or the section the TOC names
	const Section sec = toc.single ? toc.single_section : toc.lf_global;
	const size_t at = std::min(cs_size, offset + sec.offset);
	const size_t size = toc.single ? cs_size - at : std::min(sec.size, cs_size - at);
	BitReader br(cs + at, size);
	read_patch_dictionary(br, im, fh, out);
}

// A frame with splines of a sequence, when the index is built: LfGlobal's front alone, which raises what parse_frame would raise for it
// ("spln" for a damaged spline stream: only here, behind the base correlations, are the segments and their tiles known)
void parse_sequence_splines(const uint8_t *cs, size_t cs_size, size_t offset, const ImageMeta &im, const FrameHeader &fh, const Toc &toc, bool allow_patches, bool allow_noise) {
	const Section sec = toc.single ? toc.single_section : toc.lf_global;
	const size_t at = std::min(cs_size, offset + sec.offset);
	const size_t size = toc.single ? cs_size - at : std::min(sec.size, cs_size - at);
	BitReader br(cs + at, size);
	Frame f;
	f.im = im; f.fh = fh;
	f.allow_patches = allow_patches; f.allow_noise = allow_noise; f.allow_splines = true;
	read_lf_global_front(br, &f);
}

static void parse_headers_within(const uint8_t *cs, size_t limit, size_t cs_size, Frame *f) {
	memset(f->order_has_lehmer, 0, sizeof f->order_has_lehmer);
	BitReader br(cs, limit);
	if (f->seq_im) {   // a sequence's member: its bytes start at the frame header
		f->im = *f->seq_im;
		read_frame_header(br, f->im, &f->fh, true, f->allow_lf_frame, f->allow_patches);
		if (uint32_t e = sequence_refusal(f->fh, f->seq_blend, rendered_alpha_channel(f->im), f->allow_lf_frame, f->im.xyb_encoded, f->allow_modular_lf, f->allow_patches, f->allow_modular_ref)) raise(e);
	} else {
		read_image_header(br, &f->im, f->allow_wide, f->allow_upsampling);
		read_frame_header(br, f->im, &f->fh, false, false, false, f->allow_upsampling);
		J40HIP_SHOULD(f->fh.is_last, "TODO");
		J40HIP_SHOULD(f->fh.type == 0, "TODO");
	}
	if (f->fh.upsampling > 1) {   // the frame's table: the stream's own for its K first, else what the application supplied
		const int t = up_table_index(f->fh.upsampling);
		if (f->im.cw_mask >> t & 1) f->up_table = f->im.up_weights[t];
		else J40HIP_SHOULD(get_upsampling_defaults(f->fh.upsampling, &f->up_table), "updf");
		// (an LF-only parse: the LF image of such a frame is not its 1:8 preview)
		J40HIP_SHOULD(!f->lf_only, "TODO");
		// (the stretch is of XYB planes, like noise; a YCbCr frame parses and its plan is refused by the route)
		J40HIP_SHOULD(f->im.xyb_encoded || f->fh.do_ycbcr, "TODO");
	}
	// an image with 32-bit Modular buffers: its Modular frames only, and only where they were asked for (its VarDCT frames would need wide LF,
	// HF-metadata and extra-channel streams; the reference's word for the combination is TODO as well, j40.h:7868)
	J40HIP_SHOULD(f->im.modular_16bit_buffers || (f->allow_wide && f->fh.is_modular), "TODO");
	read_toc(br, f->fh, &f->toc);
	{   // a truncated codestream fails where the reference fails: in the first section (in reading order) that
		// needs the missing bytes, not up front. Sections are clipped to the bytes that exist; readers raise "shrt".
		auto clip = [cs_size](Section &s) { if (s.offset >= cs_size) { s.offset = cs_size; s.size = 0; } else s.size = std::min(s.size, cs_size - s.offset); };
		if (f->toc.single) {
			f->toc.single_declared_end = f->toc.single_section.offset + f->toc.single_section.size;
			f->toc.single_section.size = cs_size > f->toc.single_section.offset ? cs_size - f->toc.single_section.offset : 0;
			f->toc.lf_end = cs_size;   // (one section holds the LF image and the pass group alike: the whole codestream)
		}
		clip(f->toc.single_section); clip(f->toc.lf_global); clip(f->toc.hf_global);
		for (Section &s : f->toc.lf_groups) clip(s);
		for (Section &s : f->toc.pass_groups) clip(s);
	}
	allocate_lf_groups(f);
}
// Headers and TOC. With a streaming source (Frame::need_bytes) their extent is not known ahead: they are parsed on the prefix that
// has arrived and, when that runs out ("shrt": every bit read until then was real, so any other error is the stream's own), again
// on a longer one -- a few hundred bytes for most streams, an embedded ICC profile's worth for some.
// An LF-only parse (Frame::lf_only) grows the prefix in small steps instead -- 256 bytes, a sixteenth of it past 4 KB -- so that it asks
// for little past the TOC: the LF sections behind it are what the caller may be waiting for, and nothing more may be asked for.
static void parse_headers(const uint8_t *cs, size_t cs_size, Frame *f) {
	if (!f->need_bytes || !f->have_bytes) { parse_headers_within(cs, cs_size, cs_size, f); return; }
	const bool small_steps = f->lf_only;
	size_t want = std::min<size_t>(cs_size, small_steps ? 256 : 4096);
	for (;;) {
		f->need(want);
		const size_t have = std::min(cs_size, std::max(want, f->have_bytes(f->need_ctx)));
		try { parse_headers_within(cs, have, cs_size, f); return; }
		catch (const DecodeError &e) {
			if (e.code != (uint32_t) E4("shrt") || have >= cs_size) throw;
			*f = f->with_same_inputs();
			want = std::min(cs_size, small_steps ? have + std::max<size_t>(256, have / 16) : std::max(have * 2, have + 4096));
		}
	}
}

// LfGlobal and HfGlobal of a frame with several sections (an LF-only parse: LfGlobal alone, HfGlobal's bytes are not asked for)
static void parse_globals(const uint8_t *cs, Frame *f) {
	const size_t lf_global_end = f->toc.lf_global.offset + f->toc.lf_global.size;
	f->need(f->lf_only ? lf_global_end : std::max(lf_global_end, f->toc.hf_global.offset + f->toc.hf_global.size));
	{
		BitReader sr(cs + f->toc.lf_global.offset, f->toc.lf_global.size);
		read_lf_global(sr, f);
		// (no check that the section ends here, in none of the sections of a frame that has several: the reference's
		// j40__finish_section_state runs j40__no_more_bytes on the section's own state and returns the parent's, j40.h:7778-7795)
	}
	if (f->lf_only) return;
	if (f->fh.is_modular) {
		J40HIP_SHOULD(f->toc.hf_global.size == 0, "excs");
	} else {
		BitReader sr(cs + f->toc.hf_global.offset, f->toc.hf_global.size);
		read_hf_global(sr, f);
	}
}

// What the pipeline's host stage reads of a VarDCT frame with several sections (device/async.hip): everything in front of the
// LfGroup sections, and of each of those what precedes its first stream. Returns false -- nothing is lost, parse_frame does it
// all again -- for frames that are not of that kind. `tasks` (one per LfGroup section): where the streams start; `plain`: whether
// every section's first Modular header is the plain one k_lf_groups handles (global tree, no transforms).
bool parse_frame_front(const uint8_t *cs, size_t cs_size, Frame *f, std::vector<LfDeviceTask> *tasks, std::vector<int32_t> *extra_prec, bool *plain) {
	parse_headers(cs, cs_size, f);
	if (f->toc.single || f->fh.is_modular) return false;
	parse_globals(cs, f);
	if (f->fh.use_lf_frame || f->fh.jpeg_upsampling != 0) return false;
	const int64_t n = f->fh.num_lf_groups;
	tasks->assign((size_t) n, LfDeviceTask()); extra_prec->assign((size_t) n, 0);
	*plain = true;
	for (int64_t i = 0; i < n; ++i) {
		const LfGroup &gg = f->lf_groups[(size_t) i];
		LfDeviceTask &t = (*tasks)[(size_t) i];
		t.byte_off = f->toc.lf_groups[(size_t) i].offset; t.size = f->toc.lf_groups[(size_t) i].size; t.bit_off = 0;
		t.w8 = gg.width8; t.h8 = gg.height8; t.w64 = gg.width64; t.h64 = gg.height64;
		t.sidx0 = (int32_t) (1 + gg.idx); t.sidx2 = (int32_t) (1 + 2 * f->fh.num_lf_groups + gg.idx);
		t.nbvb_bits = ceil_lg32((uint32_t) (gg.width8 * gg.height8));
		try {
			BitReader sr(cs + t.byte_off, t.size);
			(*extra_prec)[(size_t) i] = (int32_t) sr.u(2);
			Modular m; m.bpp = f->im.bpp;
			m.channel.assign(3, Plane());
			for (Plane &p : m.channel) { p.width = gg.width8; p.height = gg.height8; }
			read_modular_header(sr, &f->global_tree, &f->global_codespec, &m);
			if (!(m.use_global_tree && m.transforms.empty() && m.channel.size() == 3)) *plain = false;
			t.bit_off = (uint32_t) sr.bit_position();
		} catch (const DecodeError &) { *plain = false; }   // (the section's own decode reports it in its place)
	}
	return true;
}

void parse_frame(const uint8_t *cs, size_t cs_size, Frame *f, int threads) {
	const bool timing = api_timing();   // (where a parse's time goes)
	auto now = [] { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
	const double tp0 = timing ? now() : 0;
	parse_headers(cs, cs_size, f);
	const double tp1 = timing ? now() : 0;
	J40HIP_SHOULD(!f->lf_only || !f->fh.is_modular, "TODO");   // (no LF image without Squeeze)

	if (f->toc.single) {
		// one section holds LfGlobal, HfGlobal, LfGroup and PassGroup back to back, read in the order
		// the reference reads them (j40.h:8189-8199)
		f->need(cs_size);
		BitReader sr(cs + f->toc.single_section.offset, f->toc.single_section.size);
		read_lf_global(sr, f);
		if (f->fh.is_modular) return;   // LfGroup / PassGroup read nothing for single-group Modular frames (j40.h:6731, 7024)
		read_hf_global(sr, f);
		read_lf_group(sr, f, &f->lf_groups[0]);
		if (!f->fh.is_modular) {
			// the pass group continues in the middle of this section: the device reader starts at a bit offset
			prepare_tables(f);
			f->single_pass_group_bitpos = sr.bit_position();
			return;
		}
		// Modular: every channel was already decoded in LfGlobal (num_gm_channels = all), so the pass
		// group reads nothing (j40.h:7024-7025) and the section has to end here
		J40HIP_SHOULD(f->num_gm_channels == (int32_t) f->gmodular.channel.size(), "TODO");
		sr.zero_pad_to_byte();
		{   // j40__end_of_frame, j40.h:7796-7803: short of the TOC entry's end is `shrt`, beyond it `excs`
			const size_t at = f->toc.single_section.offset + sr.byte_position();
			J40HIP_SHOULD(at >= f->toc.single_declared_end, "shrt");
			J40HIP_SHOULD(at == f->toc.single_declared_end, "excs");
		}
		return;
	}

	parse_globals(cs, f);
	const double tp2 = timing ? now() : 0;
	// LfGroup sections are independent of each other
	const int64_t n = f->fh.num_lf_groups;
	std::atomic<int64_t> next(0);
	std::atomic<uint32_t> first_err(0);
	std::vector<uint32_t> errs((size_t) n, 0);
	std::vector<char> done((size_t) n, 0);
	if (f->lf_decoder) f->need(f->lf_only ? std::min(f->toc.lf_end, cs_size) : cs_size);   // (the device reads the sections out of the whole codestream)
	if (f->lf_decoder && !f->fh.is_modular && !f->fh.use_lf_frame && f->fh.jpeg_upsampling == 0 && f->defer_lf_tail) {
		// the streams of every LfGroup section on the device (device/lf_decode.hip): the host reads what precedes the LF coefficient
		// stream -- extra precision and the first Modular header, which has to be the plain one --, the device decodes both
		// sub-images, the host finishes (LF index, varblock placement). Anything irregular: the host path below, unchanged.
		std::vector<LfDeviceTask> tasks((size_t) n);
		std::vector<int32_t> extra_prec((size_t) n, 0);
		bool plain = true;
		try {
			for (int64_t i = 0; i < n && plain; ++i) {
				const LfGroup &gg = f->lf_groups[(size_t) i];
				BitReader sr(cs + f->toc.lf_groups[(size_t) i].offset, f->toc.lf_groups[(size_t) i].size);
				extra_prec[(size_t) i] = (int32_t) sr.u(2);
				Modular m; m.bpp = f->im.bpp;
				m.channel.assign(3, Plane());
				for (Plane &p : m.channel) { p.width = gg.width8; p.height = gg.height8; }
				read_modular_header(sr, &f->global_tree, &f->global_codespec, &m);
				plain = m.use_global_tree && m.transforms.empty() && m.channel.size() == 3;
				LfDeviceTask &t = tasks[(size_t) i];
				t.byte_off = f->toc.lf_groups[(size_t) i].offset; t.size = f->toc.lf_groups[(size_t) i].size; t.bit_off = (uint32_t) sr.bit_position();
				t.w8 = gg.width8; t.h8 = gg.height8; t.w64 = gg.width64; t.h64 = gg.height64;
				t.sidx0 = (int32_t) (1 + gg.idx); t.sidx2 = (int32_t) (1 + 2 * f->fh.num_lf_groups + gg.idx);
				t.nbvb_bits = ceil_lg32((uint32_t) (gg.width8 * gg.height8));
			}
		} catch (const DecodeError &) { plain = false; }
		if (plain && f->lf_decoder(f->lf_decoder_ctx, *f, cs, cs_size, tasks)) {
			f->lf_decoded_on_device = true;
			for (int64_t i = 0; i < n; ++i) {
				const LfDeviceTask &t = tasks[(size_t) i];
				if (t.status == (uint32_t) E4("lffb")) continue;   // the host decodes this one
				done[(size_t) i] = 1;
				if (t.status) { errs[(size_t) i] = t.status; continue; }
				try {
					lf_group_finish(f, &f->lf_groups[(size_t) i], extra_prec[(size_t) i], t.lf, nullptr, t.xfromy, t.bfromy, t.info0, t.info1, t.nb_varblocks);
					if (t.sharp) f->lf_groups[(size_t) i].sharpness.assign(t.sharp, t.sharp + (size_t) t.w8 * (size_t) t.h8);
				}
				catch (const DecodeError &e) { errs[(size_t) i] = e.code; }
				catch (const std::exception &) { errs[(size_t) i] = E4("!mem"); }
			}
		}
	}
	auto worker = [&]() {
		for (;;) {
			int64_t i = next.fetch_add(1);
			if (i >= n) break;
			if (done[(size_t) i]) continue;
			try {
				f->need(f->toc.lf_groups[(size_t) i].offset + f->toc.lf_groups[(size_t) i].size);   // (streaming input: this section's bytes)
				BitReader sr(cs + f->toc.lf_groups[(size_t) i].offset, f->toc.lf_groups[(size_t) i].size);
				read_lf_group(sr, f, &f->lf_groups[(size_t) i]);
			} catch (const DecodeError &e) { errs[(size_t) i] = e.code; }
			catch (const std::exception &) { errs[(size_t) i] = E4("!mem"); }   // (an exception leaving a thread would end the process)
		}
	};
	int nthreads = (int) std::min<int64_t>(threads < 1 ? 1 : threads, n);
	if (nthreads <= 1) worker();
	else {
		std::vector<std::thread> pool;
		for (int t = 1; t < nthreads; ++t) pool.emplace_back(worker);   // (the calling thread is one of the team)
		worker();
		for (auto &t : pool) t.join();
	}
	{   // the first failing section in the order the reference reads them: by offset (a permuted TOC stores them out of index order, j40.h:5608)
		size_t best = SIZE_MAX; uint32_t code = 0;
		for (size_t i = 0; i < errs.size(); ++i) if (errs[i] && f->toc.lf_groups[i].offset < best) { best = f->toc.lf_groups[i].offset; code = errs[i]; }
		if (code) raise(code);
	}
	(void) first_err;
	const double tp3 = timing ? now() : 0;
	if (!f->fh.is_modular && !f->lf_only) prepare_tables(f);   // (the coefficient orders come from HfGlobal)
	if (timing) fprintf(stderr, "[j40hip parse] headers + TOC %.2f ms, LfGlobal + HfGlobal %.2f ms, %lld LfGroups on %d threads %.2f ms, tables %.2f ms\n", tp1 - tp0, tp2 - tp1, (long long) n, nthreads, tp3 - tp2, now() - tp3);
}

} // namespace j40hip
