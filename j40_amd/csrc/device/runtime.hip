// j40_amd/csrc/device/runtime.hip -- device half of the thin C-ABI (include/j40hip.h): launches the hot-path kernels of one frame on
// the caller's stream -- Modular, VarDCT, a region, the single-image path in two phases -- and reads the status back.
//
// No CPU fallback lives here: without a HIP device every entry point returns "!gpu".
#include "runtime_state.hpp"
#include "hostcopy.hpp"
#include "ycbcr_dev.h"
#include "orient_dev.h"
#include <map>

// a Modular frame's groups can be decoded apart from each other when every group has a section of its own and no frame-wide inverse
// transform reads across groups (j40hip_frame_set_group_range's rule; a region is otherwise widened to every group)
bool j40hip_rt::modular_groups_independent(const j40hip_frame *h) {
	const j40hip_device_state *st = h->dev;
	if (st->mod_sections_per_pass != (int32_t) h->frame.fh.num_groups) return false;
	for (const auto &op : st->mod_ops) if (op.kind == 2 || op.kind == 4) return false;
	return true;
}

// ---- the colour mode (j40hip_frame_set_colour; colour_space.hpp, device/colour_dev.h, colour_kernels.hip) ----
// The threshold tables of 8-bit frames, one per distinct (curve, exponent, intensity_target): built once per process by bisection over
// the floats (a few milliseconds), never dropped -- the copies to the devices read them
struct ColourTableKey { int32_t tf; double g; float it; bool operator<(const ColourTableKey &o) const { return tf != o.tf ? tf < o.tf : g != o.g ? g < o.g : it < o.it; } };
struct ColourTableEntry { bool usable = false; std::vector<float> table; int32_t blo = 0, bhi = 0; };
static const ColourTableEntry &colour_table_of(const ColourCurve &k, float intensity_target) {
	static std::mutex m;
	static std::map<ColourTableKey, ColourTableEntry> cache;
	const bool keyed_it = k.tf == CTF_PQ;   // (the only curve whose levels depend on intensity_target; HLG's OOTF runs in front of its table)
	const ColourTableKey key = {k.tf, k.tf == CTF_GAMMA ? k.g : 0.0, keyed_it ? intensity_target : 0.0f};
	std::lock_guard<std::mutex> lock(m);
	auto it = cache.find(key);
	if (it != cache.end()) return it->second;
	ColourTableEntry e;
	e.usable = colour::build_table(k, &e.table, &e.blo, &e.bhi);
	return cache.emplace(key, std::move(e)).first->second;
}
// the tail's parameters of this frame, made at the first decode that takes it
static uint32_t colour_params(j40hip_frame *h, hipStream_t s, const ColourTailParams **out) {
	j40hip_device_state *st = h->dev;
	if (!st->colour.ready) {
		ColourTailParams p;
		memset(&p, 0, sizeof p);
		if (!colour::tail_consts(h->frame.im, &p.cc, &p.curve)) return ERR_UCS;   // (cannot happen: the route is in force only where the setter would pass)
		// (the linear curve needs no power: evaluating it is faster than staging its table)
		if (h->frame.im.bpp == 8 && p.curve.tf != CTF_LINEAR) {
			const ColourTableEntry &e = colour_table_of(p.curve, h->frame.im.intensity_target);
			if (e.usable) {
				bool ok = true;
				p.table = st->upload(e.table.data(), e.table.size(), s, ok);
				if (!ok) return ERR_MEM;
				p.blo = e.blo; p.bhi = e.bhi; p.table_floats = COLOUR_THRESHOLDS + (e.bhi - e.blo + 1 + 3) / 4;
			}
		}
		st->colour.p = p; st->colour.ready = true;
	}
	*out = &st->colour.p;
	return 0;
}
static bool fh_bpp8_without_table(const j40hip_frame *h, const ColourTailParams &p) { return h->frame.im.bpp == 8 && !p.table; }

// ---- patches (a sequence opened with J40HIP_SEQ_PATCHES; device/patch_dev.h, patch_kernels.hip) ----
// The frame's patch dictionary onto `planes` (width x height floats each, X, Y, B one behind the other), on `s`: called by every route
// that hands planes to a tail, after the restoration filters and before the tail. Nothing for a frame without patches; nothing is
// launched for a dictionary whose placements are all of mode None. The slots are those the playback has bound ("ptno": it has not),
// checked against every record once more on the host -- the kernel checks nothing.
uint32_t j40hip_rt::apply_patches(j40hip_frame *h, float *planes, hipStream_t s) {
	if (!h->frame.fh.has_patches) return 0;
	j40hip_device_state *st = h->dev;
	PatchSlots slots;
	for (int k = 0; k < 4; ++k) { slots.base[k] = h->patch_src[k].base; slots.w[k] = h->patch_src[k].w; slots.h[k] = h->patch_src[k].h; }
	if (!h->patch_plan) return ERR_TODO;   // (cannot happen: only a sequence's handle parses a dictionary, and its index made the plan)
	for (const PatchRec &r : h->patch_plan->recs) if (uint32_t e = patch_check(r, slots, h->frame.fh.width, h->frame.fh.height)) return e;
	if (st->patch.dev.num_tiles <= 0) return 0;
	launch_patch_blend(planes, h->frame.fh.width, h->frame.fh.height, st->patch.dev, slots, s);
	++h->patch_launches;
	return 0;
}

// ---- photon noise (a frame parsed with J40HIP_PARSE_NOISE; device/noise_dev.h, noise_kernels.hip) ----
// The two kernels on `s`: the raw planes into `raw` (3 * noise_pitch(W) * H floats) from the jump sets at `sets` (device memory), their
// convolution added onto `planes` (W floats a row). ms2 not null (J40HIP_NOISE_TIMING, the known-answer hook): the call waits for them
// and reports each kernel's device time, between events of its own, destroyed on every way out.
static uint32_t run_noise_kernels(float *planes, float *raw, const uint64_t *sets, const NoiseFillArgs &a, const NoiseParams &p, hipStream_t s, float *ms2) {
	struct Trio { hipEvent_t ev[3] = {nullptr, nullptr, nullptr}; ~Trio() { for (hipEvent_t e : ev) if (e) (void) hipEventDestroy(e); } } trio;
	bool timed = ms2 != nullptr;
	for (int i = 0; timed && i < 3; ++i) timed = hipEventCreate(&trio.ev[i]) == hipSuccess;
	if (timed) (void) hipEventRecord(trio.ev[0], s);
	launch_noise_fill(raw, a, sets, s);
	if (timed) (void) hipEventRecord(trio.ev[1], s);
	launch_noise_add(planes, (size_t) a.W, raw, a.W, a.H, p, s);
	if (timed) (void) hipEventRecord(trio.ev[2], s);
	if (hipGetLastError() != hipSuccess) return ERR_GPU;
	if (ms2) { ms2[0] = ms2[1] = 0.0f; }
	if (timed) {
		if (hipEventSynchronize(trio.ev[2]) != hipSuccess) return ERR_GPU;
		(void) hipEventElapsedTime(&ms2[0], trio.ev[0], trio.ev[1]); (void) hipEventElapsedTime(&ms2[1], trio.ev[1], trio.ev[2]);
	}
	return 0;
}

// The frame's noise onto `planes` (width x height floats each, X, Y, B one behind the other), on `s`: called by render_planes behind the
// patches and ahead of the tail. Nothing for a frame without noise; nothing is launched or allocated for a LUT of eight zeros. The raw
// planes and the frame's four jump sets (built on the host by repeated squaring, once per upload) are kept with the frame like d_xyb.
uint32_t j40hip_rt::apply_noise(j40hip_frame *h, float *planes, hipStream_t s) {
	const Frame &fr = h->frame;
	if (!fr.fh.has_noise || noise_lut_is_zero(fr.noise_lut)) return 0;
	j40hip_device_state *st = h->dev;
	const int32_t W = fr.fh.width, H = fr.fh.height, gdim = 1 << fr.fh.group_size_shift;
	const NoiseFillArgs a = {W, H, gdim, (W + gdim - 1) / gdim, (H + gdim - 1) / gdim, h->noise_seeds[0], h->noise_seeds[1]};
	NoiseParams p;
	memcpy(p.lut, fr.noise_lut, sizeof p.lut);
	p.ytox = fr.base_corr_x; p.ytob = fr.base_corr_b;   // (a Modular frame's LfGlobal has neither: the defaults 0 and 1)
	if (!st->keep(st->noise.d_raw, 3 * noise_pitch(W) * (size_t) H)) return ERR_MEM;
	if (!st->noise.d_sets) {
		st->noise.host_sets.assign((size_t) 4 * NOISE_SET_WORDS, 0);   // (kept: the copy is asynchronous)
		noise_frame_jumps(a, st->noise.host_sets.data());
		bool ok = true;
		st->noise.d_sets = st->upload(st->noise.host_sets.data(), st->noise.host_sets.size(), s, ok);
		if (!ok) { st->noise.d_sets = nullptr; return ERR_MEM; }
	}
	static const bool timed = env_str("J40HIP_NOISE_TIMING") != nullptr;
	if (uint32_t e = run_noise_kernels(planes, st->noise.d_raw, st->noise.d_sets, a, p, s, timed ? st->noise.ms : nullptr)) return e;
	++h->noise_launches;
	return 0;
}

extern "C" void j40hip_frame_noise_ms(const j40hip_frame *h, float *ms2) {
	if (!ms2) return;
	ms2[0] = h && h->dev ? h->dev->noise.ms[0] : 0.0f; ms2[1] = h && h->dev ? h->dev->noise.ms[1] : 0.0f;
}

extern "C" uint32_t j40hip_kat_device_noise(float *planes_dev, int32_t width, int32_t height, int32_t group_dim, const float *lut8, float ytox, float ytob,
		uint32_t visible, uint32_t nonvisible, float *raw_out_dev, void *stream, float *ms2) {
	return guarded([&]() -> uint32_t {
		if (ms2) ms2[0] = ms2[1] = 0.0f;
		if (!planes_dev || !lut8 || width <= 0 || height <= 0 || (int64_t) width * height > (1 << 28) || group_dim < 16 || group_dim > 1024 || group_dim % 16) return ERR_RNGE;
		if (noise_lut_is_zero(lut8)) return 0;
		const NoiseFillArgs a = {width, height, group_dim, (width + group_dim - 1) / group_dim, (height + group_dim - 1) / group_dim, visible, nonvisible};
		NoiseParams p;
		memcpy(p.lut, lut8, sizeof p.lut);
		p.ytox = ytox; p.ytob = ytob;
		int device = 0;
		if (hipGetDevice(&device) != hipSuccess) return ERR_GPU;
		hipStream_t s = (hipStream_t) stream;
		j40hip_device_state tmp; tmp.device = device;
		bool ok = true;
		std::vector<uint64_t> sets((size_t) 4 * NOISE_SET_WORDS);
		noise_frame_jumps(a, sets.data());
		const size_t pitch = noise_pitch(width);
		float *raw = tmp.scratch<float>(3 * pitch * (size_t) height, ok);
		const uint64_t *d_sets = tmp.upload(sets.data(), sets.size(), s, ok);
		uint32_t e = ok ? run_noise_kernels(planes_dev, raw, d_sets, a, p, s, ms2) : ERR_MEM;
		// (the raw planes without their rows' padding)
		if (!e && raw_out_dev && hipMemcpy2DAsync(raw_out_dev, sizeof(float) * (size_t) width, raw, sizeof(float) * pitch, sizeof(float) * (size_t) width, 3 * (size_t) height, hipMemcpyDeviceToDevice, s) != hipSuccess) e = ERR_GPU;
		if (hipStreamSynchronize(s) != hipSuccess && !e) e = ERR_GPU;
		for (auto &b : tmp.buffers) b.release();
		tmp.buffers.clear();
		return e;
	});
}

// ---- splines (a frame parsed with J40HIP_PARSE_SPLINES; device/spline_dev.h, spline_kernels.hip) ----
// k_spline_draw on `s` between two events of its own when ms is not null (J40HIP_SPLINE_TIMING, the known-answer hook): the call then
// waits for the kernel and reports its device time. The events are destroyed on every way out.
static uint32_t run_spline_kernel(float *planes, int32_t W, int32_t H, const DevSplines &d, hipStream_t s, float *ms) {
	struct Pair { hipEvent_t ev[2] = {nullptr, nullptr}; ~Pair() { for (hipEvent_t e : ev) if (e) (void) hipEventDestroy(e); } } pair;
	bool timed = ms != nullptr;
	for (int i = 0; timed && i < 2; ++i) timed = hipEventCreate(&pair.ev[i]) == hipSuccess;
	if (ms) *ms = 0.0f;
	if (timed) (void) hipEventRecord(pair.ev[0], s);
	launch_spline_draw(planes, (size_t) W, W, H, d, s);
	if (timed) (void) hipEventRecord(pair.ev[1], s);
	if (hipGetLastError() != hipSuccess) return ERR_GPU;
	if (timed) {
		if (hipEventSynchronize(pair.ev[1]) != hipSuccess) return ERR_GPU;
		(void) hipEventElapsedTime(ms, pair.ev[0], pair.ev[1]);
	}
	return 0;
}

// the segments and the tiles' lists of `plan` into `st`'s memory (the host vectors must outlive the copies)
static bool upload_spline_plan(j40hip_device_state *st, const SplinePlan &plan, hipStream_t s, DevSplines *d) {
	bool ok = true;
	d->segs = st->upload(plan.segs.data(), plan.segs.size(), s, ok);
	d->tile_ids = st->upload(plan.tile_ids.data(), plan.tile_ids.size(), s, ok);
	d->tile_start = st->upload(plan.tile_start.data(), plan.tile_start.size(), s, ok);
	d->seg_idx = st->upload(plan.seg_idx.data(), plan.seg_idx.size(), s, ok);
	d->num_tiles = (int32_t) plan.tile_ids.size(); d->tiles_x = plan.tiles_x;
	return ok;
}

// The frame's splines onto `planes` (width x height floats each, X, Y, B one behind the other), on `s`: called by render_planes behind the
// patches and ahead of the noise. Nothing for a frame without splines; nothing is launched or allocated for a frame whose segments all
// dropped. The segments and their tiles (made by the parse) are uploaded once per upload and kept with the frame.
uint32_t j40hip_rt::apply_splines(j40hip_frame *h, float *planes, hipStream_t s) {
	const Frame &fr = h->frame;
	if (!fr.fh.has_splines || fr.spline_plan.tile_ids.empty()) return 0;
	j40hip_device_state *st = h->dev;
	if (!st->spline.dev.segs) {
		DevSplines d;
		if (!upload_spline_plan(st, fr.spline_plan, s, &d)) return ERR_MEM;
		st->spline.dev = d;
	}
	static const bool timed = env_str("J40HIP_SPLINE_TIMING") != nullptr;
	if (uint32_t e = run_spline_kernel(planes, fr.fh.width, fr.fh.height, st->spline.dev, s, timed ? &st->spline.ms : nullptr)) return e;
	++h->spline_launches;
	return 0;
}

extern "C" float j40hip_frame_spline_ms(const j40hip_frame *h) { return h && h->dev ? h->dev->spline.ms : 0.0f; }

extern "C" uint32_t j40hip_kat_device_splines(float *planes_dev, int32_t width, int32_t height, const void *segments, int64_t n, int64_t *tiles_out, void *stream, float *ms) {
	return guarded([&]() -> uint32_t {
		if (ms) *ms = 0.0f;
		if (tiles_out) *tiles_out = 0;
		if (!planes_dev || width <= 0 || height <= 0 || (int64_t) width * height > (1 << 28) || n < 0 || n > SPLINE_MAX_SEGMENTS || (n > 0 && !segments)) return ERR_RNGE;
		SplinePlan plan;
		plan.segs.resize((size_t) n);
		if (n) memcpy(plan.segs.data(), segments, sizeof(SplineSeg) * (size_t) n);
		// (the kernel checks nothing: every box lies inside the frame)
		for (const SplineSeg &g : plan.segs) if (g.x0 < 0 || g.x0 > g.x1 || g.x1 >= width || g.y0 < 0 || g.y0 > g.y1 || g.y1 >= height) return ERR_RNGE;
		if (!spline_bin(width, &plan)) return ERR_RNGE;
		if (tiles_out) *tiles_out = (int64_t) plan.tile_ids.size();
		if (plan.tile_ids.empty()) return 0;
		int device = 0;
		if (hipGetDevice(&device) != hipSuccess) return ERR_GPU;
		hipStream_t s = (hipStream_t) stream;
		j40hip_device_state tmp; tmp.device = device;
		DevSplines d;
		uint32_t e = upload_spline_plan(&tmp, plan, s, &d) ? run_spline_kernel(planes_dev, width, height, d, s, ms) : ERR_MEM;
		if (hipStreamSynchronize(s) != hipSuccess && !e) e = ERR_GPU;
		for (auto &b : tmp.buffers) b.release();
		tmp.buffers.clear();
		return e;
	});
}

// ---- upsampling (a frame parsed with J40HIP_PARSE_UPSAMPLING whose header has upsampling > 1; device/upsample_dev.h, upsample_kernels.hip) ----
// k_upsample on `s` between two events of its own when ms is not null (J40HIP_UPSAMPLE_TIMING, the known-answer hook): the call then
// waits for the kernel and reports its device time. The events are destroyed on every way out.
static uint32_t run_upsample_kernel(const float *src, int32_t w, int32_t h, int32_t k, const float *table_dev, float *out, int32_t up_w, int32_t up_h, hipStream_t s, float *ms) {
	struct Pair { hipEvent_t ev[2] = {nullptr, nullptr}; ~Pair() { for (hipEvent_t e : ev) if (e) (void) hipEventDestroy(e); } } pair;
	bool timed = ms != nullptr;
	for (int i = 0; timed && i < 2; ++i) timed = hipEventCreate(&pair.ev[i]) == hipSuccess;
	if (ms) *ms = 0.0f;
	if (timed) (void) hipEventRecord(pair.ev[0], s);
	if (!launch_upsample(src, w, h, k, table_dev, out, up_w, up_h, s)) return ERR_RNGE;
	if (timed) (void) hipEventRecord(pair.ev[1], s);
	if (hipGetLastError() != hipSuccess) return ERR_GPU;
	if (timed) {
		if (hipEventSynchronize(pair.ev[1]) != hipSuccess) return ERR_GPU;
		(void) hipEventElapsedTime(ms, pair.ev[0], pair.ev[1]);
	}
	return 0;
}

// The frame's coded planes at `planes` (width x height floats each, X, Y, B one behind the other) stretched into its shown-size planes, on
// `s`: called by render_planes ahead of everything else it does. *out: where the planes the tail reads lie -- `planes` themselves for a
// frame with upsampling = 1, for which nothing is launched or allocated. The shown-size planes and the expanded table (built on the host
// once per upload) are kept with the frame like d_xyb.
uint32_t j40hip_rt::apply_upsampling(j40hip_frame *h, const float *planes, float **out, hipStream_t s) {
	const Frame &fr = h->frame;
	const int32_t k = fr.fh.upsampling;
	if (k <= 1) { *out = const_cast<float *>(planes); return 0; }
	j40hip_device_state *st = h->dev;
	const int32_t up_w = fr.fh.shown_width(), up_h = fr.fh.shown_height();
	if (!upsample_factor_valid(k) || (int32_t) fr.up_table.size() != upsample_weight_count(k)) return ERR_TODO;   // (cannot happen: the parse made both)
	if (!st->keep(st->up.d_up, 3 * (size_t) up_w * (size_t) up_h)) return ERR_MEM;
	if (!st->up.d_table) {
		st->up.host_table.assign((size_t) k * k * 25, 0.0f);
		upsample_expand(k, fr.up_table.data(), st->up.host_table.data());
		bool ok = true;
		st->up.d_table = st->upload(st->up.host_table.data(), st->up.host_table.size(), s, ok);
		if (!ok) { st->up.d_table = nullptr; return ERR_MEM; }
	}
	static const bool timed = env_str("J40HIP_UPSAMPLE_TIMING") != nullptr;
	if (uint32_t e = run_upsample_kernel(planes, fr.fh.width, fr.fh.height, k, st->up.d_table, st->up.d_up, up_w, up_h, s, timed ? &st->up.ms : nullptr)) return e;
	*out = st->up.d_up;
	return 0;
}

extern "C" float j40hip_frame_upsample_ms(const j40hip_frame *h) { return h && h->dev ? h->dev->up.ms : 0.0f; }

extern "C" uint32_t j40hip_kat_device_upsample(const float *planes_dev, int32_t width, int32_t height, int32_t k, const float *weights, int32_t out_w, int32_t out_h, float *out_dev, void *stream, float *ms) {
	return guarded([&]() -> uint32_t {
		if (ms) *ms = 0.0f;
		if (!planes_dev || !weights || !out_dev || !upsample_factor_valid(k) || width <= 0 || height <= 0 || out_w <= 0 || out_h <= 0 || (int64_t) out_w > (int64_t) k * width || (int64_t) out_h > (int64_t) k * height
			|| (int64_t) out_w * out_h > (1 << 28)) return ERR_RNGE;
		int device = 0;
		if (hipGetDevice(&device) != hipSuccess) return ERR_GPU;
		hipStream_t s = (hipStream_t) stream;
		j40hip_device_state tmp; tmp.device = device;
		bool ok = true;
		std::vector<float> table((size_t) k * k * 25);
		upsample_expand(k, weights, table.data());
		const float *d_table = tmp.upload(table.data(), table.size(), s, ok);
		uint32_t e = ok ? run_upsample_kernel(planes_dev, width, height, k, d_table, out_dev, out_w, out_h, s, ms) : ERR_MEM;
		if (hipStreamSynchronize(s) != hipSuccess && !e) e = ERR_GPU;
		for (auto &b : tmp.buffers) b.release();
		tmp.buffers.clear();
		return e;
	});
}

// ---- the plane stage: from the frame's three full-size float planes (X, Y, B; a YCbCr frame's Cb, Y, Cr) to the caller's pixels ----
// Who enters it is decided once per decode, before anything is launched (run_vardct, decode_modular): a decode whose restoration filters
// run, the colour mode, a frame with patches, a 4:4:4 YCbCr plan, a caller that wants the planes themselves. Two steps: the planes are
// made (vardct_planes: the pixel kernels with OutMode::XYB, then the filters; decode_modular: k_modular_to_xyb), then rendered
// (render_planes). A further operation on XYB planes is one call in render_planes.

// the frame's own planes, width floats a row: the filters' first buffer and everybody else's only one, made at the first decode that needs them
static uint32_t plane_buffer(j40hip_device_state *st, const FrameHeader &fh, float **out) {
	if (!st->keep(st->d_xyb, 3 * (size_t) fh.width * (size_t) fh.height)) return ERR_MEM;
	*out = st->d_xyb;
	return 0;
}

// k_ycbcr_tail over the planes `t` names (plane, pitch, size and shifts of every channel) into the caller's image; j40hip_frame_read_ycbcr reads them
static uint32_t ycbcr_tail(j40hip_frame *h, YcbcrTail &t, uint8_t *img, size_t stride, hipStream_t s) {
	t.width = h->frame.fh.width; t.height = h->frame.fh.height;
	ycbcr_tail_scale(&t, h->frame.im.bpp, out16(h));
	if (!ycbcr_tail_valid(t)) return ERR_RNGE;   // (cannot happen: full-size planes, or planes that reach the padded grid)
	launch_ycbcr_tail(t, img, stride, s, out16(h));
	j40hip_device_state::YccRead &r = h->dev->ycc_read;
	for (int c = 0; c < 3; ++c) { r.plane[c] = t.plane[c]; r.pitch[c] = t.pitch[c]; r.pw[c] = t.pw[c]; r.ph[c] = t.ph[c]; }
	h->last.ycbcr_used = true;
	return 0;
}

// Render the planes (`pitch` floats a row, one plane behind the other) into the caller's image: the frame's patches onto them, its splines, its noise, then exactly
// one tail -- k_ycbcr_tail for a YCbCr plan, k_colour_tail for the colour mode (`colour`), else the sRGB tail -- and a Modular plan's A from
// its plane, as the pack kernels render it (the tails write A opaque). What the tail read stays for j40hip_frame_read_xyb.
static uint32_t render_planes(j40hip_frame *h, float *planes, size_t pitch, bool colour, uint8_t *img, size_t stride_bytes, hipStream_t s) {
	j40hip_device_state *st = h->dev;
	const Frame &fr = h->frame;
	// the coded planes first: an upsampled frame's are stretched into a buffer of their own, and everything below runs over that one, with
	// the shown size and its pitch (the route refuses such a frame with patches, with noise or as a YCbCr plan)
	if (fr.fh.upsampling > 1) {
		if (pitch != (size_t) fr.fh.width) return ERR_TODO;   // (cannot happen: only a YCbCr plan pads its rows)
		h->last.coded_planes = planes;
		if (uint32_t e = apply_upsampling(h, planes, &planes, s)) return e;
		pitch = (size_t) fr.fh.shown_width();
	}
	const int32_t W = fr.fh.shown_width(), H = fr.fh.shown_height();
	if (uint32_t e = apply_patches(h, planes, s)) return e;
	if ((fr.fh.has_noise || fr.fh.has_splines) && pitch != (size_t) W) return ERR_TODO;   // (cannot happen: only a YCbCr plan pads its rows, and the route refuses it)
	// (a frame with patches and splines: what k_patch_blend left stays readable as stage 3, in a copy -- the splines are drawn in place)
	if (fr.fh.has_patches && fr.fh.has_splines) {
		const size_t n = 3 * (size_t) W * (size_t) H;
		if (!st->keep(st->spline.d_patched, n)) return ERR_MEM;
		if (hipMemcpyAsync(st->spline.d_patched, planes, sizeof(float) * n, hipMemcpyDeviceToDevice, s) != hipSuccess) return ERR_GPU;
		h->last.patched_planes = st->spline.d_patched;
	}
	if (uint32_t e = apply_splines(h, planes, s)) return e;
	if (uint32_t e = apply_noise(h, planes, s)) return e;
	h->last.tail_planes = planes;
	if (st->ycbcr) {
		YcbcrTail t;
		for (int c = 0; c < 3; ++c) { t.plane[c] = planes + (size_t) c * pitch * (size_t) H; t.pitch[c] = (int32_t) pitch; t.pw[c] = W; t.ph[c] = H; t.hshift[c] = t.vshift[c] = 0; }
		return ycbcr_tail(h, t, img, stride_bytes, s);
	}
	if (colour) {
		const ColourTailParams *p = nullptr;
		if (uint32_t e = colour_params(h, s, &p)) return e;
		launch_colour_tail(planes, pitch, *p, W, H, img, stride_bytes, s, out16(h));
		h->last.colour_used = true;
		h->last.colour_curve_8bit = fh_bpp8_without_table(h, *p);   // (an 8-bit frame whose curve has no table: j40hip_frame_colour says so)
	} else launch_xyb_to_rgba(planes, pitch, st->is_modular ? st->patch.d_frame : st->plan.frame, W, H, img, stride_bytes, s, out16(h));
	if (st->is_modular && st->alpha_channel >= 0) launch_alpha_from_plane(st->final_planes[(size_t) st->alpha_channel], W, H, fr.im.bpp, img, stride_bytes, s, out16(h));
	return 0;
}

// region (j40hip_frame_set_region): null, or the rectangle {x0, y0, w, h} that becomes the w x h pixels at rgba_dev -- the sections of
// its cover only (LfGlobal's too), one launch per row of the cover's groups and pass, the frame-wide per-pixel transforms over the
// cover's rows, and the rectangle packed with the destination moved back by its origin; every section where the groups depend on
// each other
// shift: the scale shift of a whole-frame decode (decode_scaled): the pack kernel writes the small image
// A Modular frame of an XYB image with the switch in force (j40hip_frame_set_modular_xyb): k_modular_xyb_pack stands in for k_pack_planes
// for whole frames and rectangles alike (never at a shift: decode_scaled stages such a frame). xyb_out (decode_frame_xyb, a Modular LF
// frame; the whole frame only): no pixels -- k_modular_to_xyb leaves the three float planes there, width * height floats each.
static uint32_t decode_modular(j40hip_frame *h, const DecodeRoute &route, void *rgba_dev, size_t stride_bytes, hipStream_t s, float *ms3, const int32_t *region = nullptr, int32_t shift = 0, float *xyb_out = nullptr) {
	j40hip_device_state *st = h->dev;
	const DevModPlan &plan = st->mod;
	const Frame &fr = h->frame;
	const bool wide = st->mod_wide;   // int32 planes (the plane pointers carry the sample size themselves)
	h->last = LastDecode();   // (what the last decode left behind for j40hip_frame_status and the getters: every decode starts from none of it)
	h->last.wide_used = wide;
	const bool xyb = route.modular_xyb && st->final_planes.size() >= 3;
	h->last.modular_xyb_used = xyb;
	if ((xyb_out && !xyb) || (xyb && shift > 0)) return ERR_TODO;
	const bool colour = route.colour && xyb && !xyb_out;   // (whole frames: the route stages a region or a scale)
	const bool patches = (route.patches || route.splines || route.noise || route.upsampling) && !xyb_out;        // (likewise; splines, noise and upsampling go the patches' way)
	if (patches && (!xyb || !st->patch.d_frame)) return ERR_TODO;
	if ((colour || patches) && (region || shift > 0 || !route.every_group)) return ERR_TODO;
	const bool planes = colour || patches || xyb_out;   // the decode goes through the plane stage
	RegionCover cover = {0, 0, 0, 0, 0, 0};
	bool covered = false;   // only the cover's groups are decoded
	if (region) {
		cover = region_cover(region[0], region[1], region[2], region[3], fr.fh.group_size_shift, fr.fh.gcolumns);
		const bool independent = modular_groups_independent(h);
		covered = independent && region_cover_groups(cover) != (int32_t) fr.fh.num_groups;
		h->region_widened = independent ? 0 : 1; h->region_varblocks = 0;
		h->region_sections = covered ? st->mod_sections - st->mod_sections_per_pass * st->mod_passes + st->mod_passes * region_cover_groups(cover) : st->mod_sections;
	}
	const StageMarks marks{ms3 ? st->ev : nullptr, s};
	marks.mark(0);
	if (hipMemsetAsync(plan.status, 0, sizeof(uint32_t) * ((size_t) st->total_sections + 1), s) != hipSuccess) return ERR_GPU;
	marks.mark(1);
	// LfGlobal's section and the first pass together, then every further pass on its own: a pass rewrites what the one before
	// it wrote (j40.h:7025-7033), so they must not overlap; the sections' own RCTs only matter for the last pass
	const int32_t per_pass = st->mod_sections_per_pass, lead = st->mod_sections - per_pass * st->mod_passes;
	// (sharded decodes, j40hip_frame_set_group_range: LfGlobal's section and this process' groups of every pass; only frames with a section per group take one)
	const bool ranged = !route.every_group;
	const int32_t g0 = ranged ? (int32_t) st->first_group : 0, gn = ranged ? (int32_t) st->num_groups : per_pass;
	h->last.modular_xyb_whole = xyb && !covered && !ranged;
	if (covered) {
		launch_modular_sections(plan, 0, lead, st->mod_info, s);
		for (int32_t p = 0; p < st->mod_passes; ++p) for (int32_t r = 0; r < cover.rows; ++r) launch_modular_sections(plan, lead + p * per_pass + (cover.gy0 + r) * cover.gcolumns + cover.gx0, cover.cols, st->mod_info, s);
		if (st->mod_local_rcts) for (int32_t r = 0; r < cover.rows; ++r) launch_section_inverse_rcts(plan, lead + (st->mod_passes - 1) * per_pass + (cover.gy0 + r) * cover.gcolumns + cover.gx0, cover.cols, s, wide);
	} else {
	if (ranged) { launch_modular_sections(plan, 0, lead, st->mod_info, s); launch_modular_sections(plan, lead + g0, gn, st->mod_info, s); }
	else launch_modular_sections(plan, 0, lead + per_pass, st->mod_info, s);
	for (int32_t p = 1; p < st->mod_passes; ++p) launch_modular_sections(plan, lead + p * per_pass + g0, gn, st->mod_info, s);
	if (st->mod_local_rcts) launch_section_inverse_rcts(plan, lead + (st->mod_passes - 1) * per_pass + g0, gn, s, wide);
	}
	marks.mark(2);
	// (a covered region: the frame-wide per-pixel transforms over the rows of the cover's groups only)
	const size_t frame_samples = (size_t) fr.fh.width * (size_t) fr.fh.height;
	const size_t band_off = covered ? ((size_t) cover.gy0 << cover.shift) * (size_t) fr.fh.width : 0;   // in samples
	const size_t band_n = covered ? (size_t) (std::min<int64_t>(fr.fh.height, (int64_t) (cover.gy0 + cover.rows) << cover.shift) - ((int64_t) cover.gy0 << cover.shift)) * (size_t) fr.fh.width : 0;
	for (const std::vector<j40hip_device_state::ModOp> *ops : {&st->mod_sub_ops, &st->mod_ops}) for (const auto &op : *ops) {
		if (ranged && op.group >= 0 && (op.group < g0 || op.group >= g0 + gn)) continue;   // the sub-image of a group this process did not decode
		if (covered && op.group >= 0 && (op.group % cover.gcolumns < cover.gx0 || op.group % cover.gcolumns >= cover.gx0 + cover.cols || op.group / cover.gcolumns < cover.gy0 || op.group / cover.gcolumns >= cover.gy0 + cover.rows)) continue;
		if (covered && op.group < 0 && op.n == frame_samples && op.kind == 0) launch_inverse_rct(op.a.at(band_off), op.b.at(band_off), op.c.at(band_off), band_n, op.p0, s);
		else if (covered && op.group < 0 && op.n == frame_samples && op.kind == 1) launch_inverse_palette_plain(op.src.at(band_off), op.aux, op.a.at(band_off), band_n, op.p0, op.p1, fr.im.bpp, s);
		else if (op.kind == 0) launch_inverse_rct(op.a, op.b, op.c, op.n, op.p0, s);
		else if (op.kind == 1) launch_inverse_palette_plain(op.src, op.aux, op.a, op.n, op.p0, op.p1, fr.im.bpp, s);
		else if (op.kind == 2) launch_inverse_palette_predicted(op.src, op.aux, op.p0, op.dst_list, op.p1, op.p2, op.p3, op.p4, op.p5 & 0xffffff, op.p5 >> 24, fr.im.bpp, op.wpp, st->pal_wp_scratch, st->mod_extra_status, s);
		else if (op.kind == 4) launch_inverse_squeeze(op.src, op.aux, op.a, op.p0, op.p1, op.p2, op.p3, op.p4 != 0, s);
		else launch_paste_plane(op.src, op.p0, op.p1, op.a, op.p2, s);
	}
	const PlanePtr alpha = st->alpha_channel >= 0 ? st->final_planes[(size_t) st->alpha_channel] : PlanePtr{nullptr, st->final_planes[0].sample_bytes};
	const ModXybConsts xk = xyb ? modular_xyb_consts(fr) : ModXybConsts();
	// rectangle (x0, y0, w, hh) of the frame into the image whose pixel (0, 0) is at `img`
	auto pack_rect = [&](int32_t x0, int32_t y0, int32_t w, int32_t hh, uint8_t *img) {
		if (xyb) launch_modular_xyb_pack_rect(st->final_planes[0], st->final_planes[1], st->final_planes[2], alpha, fr.fh.width, x0, y0, w, hh, xk, img, stride_bytes, s, out16(h));
		else launch_pack_planes_rect(st->final_planes[0], st->final_planes[1], st->final_planes[2], alpha, fr.fh.width, x0, y0, w, hh, fr.im.bpp, img, stride_bytes, s, out16(h));
	};
	if (planes) {
		// the plane stage: the float planes by k_modular_to_xyb -- into the caller's slot, which is all it wants, or the frame's own, which are rendered
		const size_t plane = (size_t) fr.fh.width * (size_t) fr.fh.height;
		float *d = xyb_out;
		if (!d) if (uint32_t e = plane_buffer(st, fr.fh, &d)) return e;
		launch_modular_to_xyb(st->final_planes[0], st->final_planes[1], st->final_planes[2], fr.fh.width, 0, 0, fr.fh.width, fr.fh.height, xk, d, d + plane, d + 2 * plane, (size_t) fr.fh.width, s);
		if (!xyb_out) if (uint32_t e = render_planes(h, d, (size_t) fr.fh.width, colour, (uint8_t *) rgba_dev, stride_bytes, s)) return e;
	} else if (region) {   // the rectangle alone; pixel (x0, y0) of the frame is the first one at rgba_dev
		pack_rect(region[0], region[1], region[2], region[3], (uint8_t *) rgba_dev - ((size_t) region[1] * stride_bytes + (size_t) region[0] * pixel_bytes(h)));
	} else if (ranged) {   // only this process' pixels are written
		int32_t rects[3][4];
		const int nr = group_range_rects(g0, gn, fr.fh.width, fr.fh.height, fr.fh.group_size_shift, rects);
		for (int k = 0; k < nr; ++k) pack_rect(rects[k][0], rects[k][1], rects[k][2] - rects[k][0], rects[k][3] - rects[k][1], (uint8_t *) rgba_dev);
	} else if (xyb) launch_modular_xyb_pack(st->final_planes[0], st->final_planes[1], st->final_planes[2], alpha, fr.fh.width, fr.fh.height, xk, (uint8_t *) rgba_dev, stride_bytes, s, out16(h));
	else launch_pack_planes(st->final_planes[0], st->final_planes[1], st->final_planes[2], alpha, fr.fh.width, fr.fh.height, fr.im.bpp, (uint8_t *) rgba_dev, stride_bytes, s, out16(h), shift);
	marks.mark(3);
	if (uint32_t e = marks.finish(ms3)) return e;
	return hipGetLastError() == hipSuccess ? 0 : ERR_GPU;
}

// dense planes are cleared before every decode (the passes accumulate into them). Sparse coefficients need nothing: the per-block
// table is cleared once per upload, and an entry the entropy kernel does not rewrite (a section failed before reaching the
// block) still describes events of this frame's previous decode -- in range, and the frame is reported as failed anyway.
uint32_t j40hip_rt::clear_before_decode(j40hip_device_state *st, hipStream_t s) {
	const DevPlan &plan = st->plan;
	if (plan.events) return 0;
	return hipMemsetAsync(plan.coeffs[0], 0, sizeof(float) * 3 * (size_t) plan.coeff_stride, s) == hipSuccess ? 0 : ERR_GPU;
}

// The sections' status words and (end_bits not null) where each section's coefficients ended, copied back on `s`; the caller waits
static bool read_section_words(const j40hip_device_state *st, std::vector<uint32_t> *end_bits, std::vector<uint32_t> *status, hipStream_t s) {
	const size_t n = (size_t) st->total_sections;
	status->resize(n);
	if (end_bits) end_bits->resize(n);
	if (end_bits && hipMemcpyAsync(end_bits->data(), st->plan.section_end_bit, sizeof(uint32_t) * n, hipMemcpyDeviceToHost, s) != hipSuccess) return false;
	return hipMemcpyAsync(status->data(), st->plan.status, sizeof(uint32_t) * n, hipMemcpyDeviceToHost, s) == hipSuccess;
}
// What the sub-images' decode found (found[i]: plan section i, the frame's section section_of[i]) and the headers that did not parse,
// into the frame's status words; *any: something changed, and `status` was written back and waited for
static bool merge_trailer_status(j40hip_device_state *st, std::vector<uint32_t> &status, const std::vector<uint32_t> &found, const std::vector<int32_t> &section_of, const std::vector<std::pair<int32_t, uint32_t>> &header_errors, hipStream_t s, bool *any) {
	*any = false;
	for (size_t i = 0; i < found.size(); ++i) if (found[i]) { status[(size_t) section_of[i]] = found[i]; *any = true; }
	for (const auto &e : header_errors) { status[(size_t) e.first] = e.second; *any = true; }
	return !*any || (hipMemcpyAsync(st->plan.status, status.data(), sizeof(uint32_t) * status.size(), hipMemcpyHostToDevice, s) == hipSuccess && hipStreamSynchronize(s) == hipSuccess);
}

// VarDCT frames with extra channels (latency path): decodes the Modular sub-image that follows the HF coefficients in every
// section -- into planes nobody reads, the reference drops them too (j40.h:7868) -- so that damage there is reported like the
// reference reports it. Needs the entropy kernel's results on the host (where each section's coefficients ended), i.e. it
// synchronises the stream; the statuses it finds are written back into the frame's status array.
static uint32_t validate_trailers(j40hip_frame *h, hipStream_t s) {
	j40hip_device_state *st = h->dev;
	const Frame &fr = h->frame;
	std::vector<uint32_t> end_bits, status;
	if (!read_section_words(st, &end_bits, &status, s) || hipStreamSynchronize(s) != hipSuccess) return ERR_GPU;
	HostModPlan hp;
	std::vector<std::pair<int32_t, uint32_t>> header_errors;
	std::vector<int32_t> section_of;
	if (uint32_t e = build_trailer_plan(fr, h->cs, h->cs_size, end_bits.data(), status.data(), &hp, &header_errors, &section_of)) return e;
	bool ok = true;
	std::vector<uint32_t> found(hp.sections.size(), 0);
	if (!hp.sections.empty()) {
		// one block of the device memory cache, given back once the stream has been synchronised
		const ModPlanLayout lay(hp, 0);
		CacheBlock block;
		if (!block.ensure(st->device, lay.total_bytes, true)) return ERR_GPU;
		uint8_t *base = (uint8_t *) block.ptr;
		std::vector<uint8_t> staging(lay.upload_bytes);
		lay.stage(hp, staging.data(), base);
		const DevModPlan plan = lay.bind(base, st->plan.codestream);
		ok = hipMemcpyAsync(base, staging.data(), lay.upload_bytes, hipMemcpyHostToDevice, s) == hipSuccess
			&& hipMemsetAsync(plan.status, 0, sizeof(uint32_t) * (found.size() + 1), s) == hipSuccess;   // (recycled memory, as in decode_modular and keep_alpha)
		if (ok) {
			launch_modular_sections(plan, 0, (int32_t) hp.sections.size(), mod_launch_info(hp), s);
			ok = hipMemcpyAsync(found.data(), plan.status, sizeof(uint32_t) * found.size(), hipMemcpyDeviceToHost, s) == hipSuccess;
		}
		if (hipStreamSynchronize(s) != hipSuccess) ok = false;
		block.release(true);   // (the stream has been waited for)
	}
	bool any = false;
	ok = ok && merge_trailer_status(st, status, found, section_of, header_errors, s, &any);
	if (ok && !any) ok = hipStreamSynchronize(s) == hipSuccess;
	return ok ? 0 : ERR_GPU;
}

// keep_alpha: validate_trailers for such a frame. The same Modular decode of every section's sub-image, but into frame-wide planes
// (build_trailer_plan's keep mode), then k_alpha_merge of the alpha channel's plane into the pixels at `rgba_dev`, which the pixel
// kernels have written opaque on the same stream. A ranged decode takes only its groups' sections and rectangles. The plan, the
// planes and the scratch live with the frame (AlphaKeep): the first decode waits for the entropy kernel's end bits and lays them
// out, later ones only launch. *fallback: nothing was done because a section lists transforms of its own that keep mode does not
// undo, and the mode came from the environment -- the caller validates the sub-images as in drop mode.
static uint32_t keep_alpha(j40hip_frame *h, void *rgba_dev, size_t stride_bytes, hipStream_t s, bool *fallback) {
	*fallback = false;
	j40hip_device_state *st = h->dev;
	j40hip_device_state::AlphaKeep &ak = st->alpha;
	const Frame &fr = h->frame;
	int32_t alpha_index = -1;
	if (uint32_t e = alpha_keep_scope(fr, &alpha_index)) return e;
	const bool whole = !h->partial_range;
	std::vector<uint32_t> status;
	if (!ak.ready || ak.first_group != st->first_group || ak.num_groups != st->num_groups) {
		ak.ready = false;
		std::vector<uint32_t> end_bits;
		if (!read_section_words(st, &end_bits, &status, s) || hipStreamSynchronize(s) != hipSuccess) return ERR_GPU;
		HostModPlan hp;
		ak.header_errors.clear(); ak.section_of.clear();
		if (uint32_t e = build_trailer_plan(fr, h->cs, h->cs_size, end_bits.data(), status.data(), &hp, &ak.header_errors, &ak.section_of, true, (int32_t) st->first_group, whole ? -1 : (int32_t) st->num_groups)) {
			if (e == (uint32_t) ERR_TODO && h->alpha < 0) { *fallback = true; return 0; }
			return e;
		}
		// one block (ModPlanLayout): what is uploaded first, the frame-wide planes and the scratch behind it
		const ModPlanLayout lay(hp, 0);
		if (!ak.block.ensure(st->device, lay.total_bytes, false)) return ERR_MEM;
		uint8_t *base = (uint8_t *) ak.block.ptr;
		ak.staging.assign(lay.upload_bytes, 0);
		lay.stage(hp, ak.staging.data(), base);
		if (hipMemcpyAsync(base, ak.staging.data(), lay.upload_bytes, hipMemcpyHostToDevice, s) != hipSuccess) return ERR_GPU;
		ak.plan = lay.bind(base, st->plan.codestream);
		ak.info = mod_launch_info(hp);
		ak.num_sections = (int32_t) hp.sections.size(); ak.local_rcts = !hp.local_rct.empty();
		ak.alpha_plane = lay.plane(base, (size_t) alpha_index);
		ak.first_group = st->first_group; ak.num_groups = st->num_groups;
		ak.ready = true;
	} else if (!read_section_words(st, nullptr, &status, s)) return ERR_GPU;
	std::vector<uint32_t> found((size_t) ak.num_sections, 0);
	if (ak.num_sections) {
		if (hipMemsetAsync(ak.plan.status, 0, sizeof(uint32_t) * ((size_t) ak.num_sections + 1), s) != hipSuccess) return ERR_GPU;
		launch_modular_sections(ak.plan, 0, ak.num_sections, ak.info, s);
		if (ak.local_rcts) launch_section_inverse_rcts(ak.plan, 0, ak.num_sections, s);
	}
	if (whole) launch_alpha_merge(ak.alpha_plane, fr.fh.width, 0, 0, fr.fh.width, fr.fh.height, fr.im.bpp, (uint8_t *) rgba_dev, stride_bytes, s, out16(h));
	else {
		int32_t rects[3][4];
		const int nr = group_range_rects((int32_t) st->first_group, (int32_t) st->num_groups, fr.fh.width, fr.fh.height, fr.fh.group_size_shift, rects);
		for (int k = 0; k < nr; ++k) launch_alpha_merge(ak.alpha_plane, fr.fh.width, rects[k][0], rects[k][1], rects[k][2] - rects[k][0], rects[k][3] - rects[k][1], fr.im.bpp, (uint8_t *) rgba_dev, stride_bytes, s, out16(h));
	}
	h->last.alpha_written = true;
	bool ok = hipGetLastError() == hipSuccess;
	if (ok && ak.num_sections) ok = hipMemcpyAsync(found.data(), ak.plan.status, sizeof(uint32_t) * found.size(), hipMemcpyDeviceToHost, s) == hipSuccess;
	if (ok) ok = hipStreamSynchronize(s) == hipSuccess;
	if (!ok) { ak.ready = false; return ERR_GPU; }
	bool any = false;
	return merge_trailer_status(st, status, found, ak.section_of, ak.header_errors, s, &any) ? 0 : ERR_GPU;
}

// the extra channels' sub-images behind a decode's coefficients: kept (the alpha channel merged into `rgba_dev`) or only validated
static uint32_t finish_trailers(j40hip_frame *h, void *rgba_dev, size_t stride_bytes, hipStream_t s, bool whole, bool alpha_merged) {
	if (alpha_merged && rgba_dev) {
		bool fallback = false;
		const uint32_t e = keep_alpha(h, rgba_dev, stride_bytes, s, &fallback);
		if (!fallback) return e;
	}
	return whole ? validate_trailers(h, s) : 0;
}

// ---- restoration filters (device/restore_dev.h, restore_kernels.h) ----
// Off unless asked for: j40 parses the frame header's RestorationFilter bundle and ignores it (j40.h:5339-5366; its j40__gaborish /
// j40__epf are never called), and the default decode matches j40. J40HIP_RESTORATION=1 (or j40hip_frame_set_restoration(f, 1)) runs the
// filters a VarDCT frame signals; =j40 (2) runs them exactly as j40's routines stand, aliased line buffers and all (restore_dev.h).
static bool surely_nonzero(float x) { return std::isfinite(x) && std::fabs(x) >= 1e-8f; }   // j40.h:625
// the kernels' parameters from the frame header's; 0 or the reference routines' own complaints: "gab0" (j40.h:7289), "epf0" (j40.h:7384)
uint32_t j40hip_rt::restore_params(const FrameHeader &fh, int mode, RestoreParams *p) {
	const FrameHeader::Restoration &r = fh.restoration;
	memset(p, 0, sizeof *p);
	p->width = fh.width; p->height = fh.height; p->w8 = (fh.width + 7) / 8; p->h8 = (fh.height + 7) / 8;
	p->quirk = mode == 2 ? 1 : 0;
	if (r.gab) for (int c = 0; c < 3; ++c) {
		float w0 = 1.0f, w1 = r.gab_weights[c][0], w2 = r.gab_weights[c][1];
		const float wsum = w0 + w1 * 4 + w2 * 4;
		if (!surely_nonzero(wsum)) return ERR4('g', 'a', 'b', '0');
		p->gab_w[c][0] = w0 / wsum; p->gab_w[c][1] = w1 / wsum; p->gab_w[c][2] = w2 / wsum;
	}
	if (r.epf_iters > 0) {
		for (int i = 0; i < 8; ++i) {
			const float q = r.quant_mul * r.sharp_lut[i];
			if (!surely_nonzero(q)) return ERR4('e', 'p', 'f', '0');
			p->inv_quant_sharp_lut[i] = 1.0f / q;
		}
		const float scale[3] = {r.pass0_sigma_scale, 1.0f, r.pass2_sigma_scale};
		for (int k = 0; k < 3; ++k) { p->sigma_scale[k] = scale[k] * 1.9330952441687859f; p->border_scale[k] = p->sigma_scale[k] * r.border_sad_mul; }   // j40.h:7466-7467
		for (int c = 0; c < 3; ++c) p->channel_scale[c] = r.channel_scale[c];
	}
	return 0;
}
// The filters' preparation, once per upload: the kernels' parameters, the frame-wide sharpness map and what keeps the filters from running
// -- in the order the reference's routines complain: "gab0" / "epf0", a picture one sample wide, "shrp". Known from the header and the map
// alone, so a decode looks here before it decides its route.
static const j40hip_device_state::Restore &restore_prepared(j40hip_frame *h) {
	j40hip_device_state::Restore &rs = h->dev->restore;
	if (rs.ready) return rs;
	const Frame &fr = h->frame;
	const FrameHeader::Restoration &r = fr.fh.restoration;
	rs.err = restore_params(fr.fh, 1, &rs.p);   // (mode 2 differs in `quirk` alone: run_filters sets it)
	if (!rs.err && r.gab && fr.fh.width < 2) rs.err = ERR_TODO;   // (j40__gaborish reads sample 1 of every row, j40.h:7304)
	// the sharpness map: frame-wide, in the cell order of `blocks` (LfGroup after LfGroup); "shrp" as j40__epf_recip_sigmas finds it (j40.h:7399)
	if (!rs.err && r.epf_iters > 0) {
		uint16_t ub = 0;
		for (const LfGroup &gg : fr.lf_groups) {
			if (gg.sharpness.size() != (size_t) gg.width8 * (size_t) gg.height8) { rs.err = ERR_TODO; break; }   // (a frame handle built without it: from a view or an LF bundle)
			for (int16_t v : gg.sharpness) ub |= (uint16_t) v;
			rs.sharp.insert(rs.sharp.end(), gg.sharpness.begin(), gg.sharpness.end());
		}
		if (!rs.err && !(ub < 8)) rs.err = ERR4('s', 'h', 'r', 'p');
	}
	rs.ready = true;
	return rs;
}

// Gaborish and the edge-preserving filter over the frame's planes (d_xyb, where the pixel kernels have left the samples on `s`) in `mode`;
// d_restored says where the result lies. Their second set of planes, the sigmas and the map's copy are made at the first run.
static uint32_t run_filters(j40hip_frame *h, int mode, hipStream_t s) {
	j40hip_device_state *st = h->dev;
	const Frame &fr = h->frame;
	const FrameHeader::Restoration &r = fr.fh.restoration;
	const int32_t W = fr.fh.width, H = fr.fh.height;
	const size_t cells = (size_t) ((W + 7) / 8) * (size_t) ((H + 7) / 8);
	if (!st->keep(st->d_xyb_tmp, 3 * (size_t) W * (size_t) H) || !st->keep(st->d_sigma, cells + 64)) return ERR_MEM;
	if (r.epf_iters > 0 && !st->d_sharp) {
		bool ok = true;
		st->d_sharp = st->upload(st->restore.sharp.data(), st->restore.sharp.size(), s, ok);
		if (!ok) { st->d_sharp = nullptr; return ERR_MEM; }
	}
	RestoreParams p = st->restore.p;
	p.quirk = mode == 2 ? 1 : 0;
	// J40HIP_RESTORATION_TIMING: the filters' time between two events of this call's own, destroyed on every way out
	struct Pair { hipEvent_t ev[2] = {nullptr, nullptr}; ~Pair() { for (hipEvent_t e : ev) if (e) (void) hipEventDestroy(e); } } pair;
	static const bool timed = env_str("J40HIP_RESTORATION_TIMING") != nullptr;
	const StageMarks marks{timed && hipEventCreate(&pair.ev[0]) == hipSuccess && hipEventCreate(&pair.ev[1]) == hipSuccess ? pair.ev : nullptr, s};
	marks.mark(0);
	uint32_t *sharp_or = (uint32_t *) (st->d_sigma + cells);   // (the device's own OR of the sharpness values: unused, the host checked)
	if (r.epf_iters > 0) {
		if (hipMemsetAsync(sharp_or, 0, 4, s) != hipSuccess) return ERR_GPU;
		launch_epf_sigma(st->plan, (int32_t) fr.lf_groups.size(), st->d_sharp, p, st->d_sigma, sharp_or, s);
	}
	st->d_restored = launch_restoration(st->d_xyb, st->d_xyb_tmp, (size_t) W, p, r.gab, r.epf_iters, st->d_sigma, s);
	marks.mark(1);
	h->last.restore_ran = mode;
	if (marks.ev && hipEventSynchronize(pair.ev[1]) == hipSuccess) (void) hipEventElapsedTime(&st->restore_ms, pair.ev[0], pair.ev[1]);
	return 0;
}

// ---- YCbCr frames (j40hip_frame_set_ycbcr; device/ycbcr_dev.h, ycbcr_kernels.hip) ----
// The pixel stage of a subsampled YCbCr frame, which has no full-size planes and so a route of its own: the pixel kernels leave a plane
// per channel at the channel's resolution over the padded grid (OutMode::YCC), and k_ycbcr_tail makes the pixels of them. (A 4:4:4
// frame goes through the plane stage.) The planes are made at the first decode and kept with the frame.
static uint32_t ycbcr_pixels(j40hip_frame *h, const int32_t *class_start, const DevVarblock *list, uint8_t *img, size_t stride, hipStream_t s) {
	j40hip_device_state *st = h->dev;
	const Frame &fr = h->frame;
	uint32_t shifts = 0;
	for (int c = 0; c < 3; ++c) shifts |= (uint32_t) (fr.fh.hshift[c] | fr.fh.vshift[c] << 1) << (2 * c);
	YcbcrTail t;
	ycc_plane_dims(fr.fh.width, fr.fh.height, shifts, t.pw, t.ph);
	size_t total = 0;
	for (int c = 0; c < 3; ++c) total += (size_t) t.pw[c] * (size_t) t.ph[c];
	if (!st->keep(st->d_ycc, total)) return ERR_MEM;
	launch_vardct_frame(st->plan, class_start, list, st->d_large_scratch, K2Target{st->d_ycc, 0, OutMode::YCC, 0}, s);
	size_t off = 0;
	for (int c = 0; c < 3; ++c) {
		t.plane[c] = st->d_ycc + off; t.pitch[c] = t.pw[c]; t.hshift[c] = fr.fh.hshift[c]; t.vshift[c] = fr.fh.vshift[c];
		off += (size_t) t.pw[c] * (size_t) t.ph[c];
	}
	return ycbcr_tail(h, t, img, stride, s);
}

// One VarDCT decode as decode_impl (whole frames, group ranges), decode_region (covers), decode_scaled and decode_frame_xyb describe it to
// run_vardct; as it stands, the whole frame from the frame's own lists, with nothing to write to yet
struct VardctRun {
	VardctRun(const j40hip_frame *h, const DecodeRoute &r) : num_groups((int32_t) h->frame.fh.num_groups), list(h->dev->d_vb_sorted), class_start(h->dev->class_start), restoration(r.restoration), alpha_merged(r.alpha_merged), colour(r.colour), patches(r.patches || r.splines || r.noise || r.upsampling) {}
	int32_t first_group = 0, num_groups; // the groups of the entropy launch ...
	const RegionCover *cover = nullptr;  // ... or (not null) a region's cover: through the fast kernel's order list (region.d_order), else a launch per row of its groups
	const DevVarblock *list; const int32_t *class_start;   // what the pixel kernels take
	uint8_t *img = nullptr; size_t img_stride = 0;   // where they write
	bool whole = true;                   // every group is decoded: the extra channels' sub-images can be validated
	int restoration;                     // the route's: the mode the restoration filters run in (0: they do not; never where `whole` is false)
	bool alpha_merged;                   // the route's
	bool colour;                         // the route's: the pixels come from k_colour_tail (whole frames at full size: the route stages everything else)
	bool patches;                        // the route's patches, noise or upsampling: the frame's patches, its noise, go onto its XYB planes ahead of the tail, an upsampled frame's planes are stretched there (whole frames at full size, likewise)
	const uint8_t *crop_from = nullptr; uint8_t *crop_to = nullptr; size_t crop_stride = 0; int32_t crop_w = 0, crop_h = 0;   // crop_to not null: these pixels of img are then moved there
	int32_t shift = 0;                   // the scale shift the pixel kernels write at (decode_scaled's fused route: img is the small image)
	float *xyb_out = nullptr;            // not null (an LF frame of a sequence, decode_frame_xyb): no pixels, img is null -- the three XYB planes, width * height
	                                     // floats each, as the inverse transforms or (where they run) the restoration filters leave them, go here
};

// A frame with use_lf_frame: its LfGroup tail on `s`, ahead of the entropy kernels -- the LF samples and LF indices from the picture the
// playback has bound (j40hip_frame_bind_lf_source), the block contexts where the frame has LF thresholds, the LLF coefficients
// (lf_tail_kernels.hip). The thresholds as samples: (float) t * mult_lf[c] with mult_lf at extra_precision 0, frame.cpp's expression.
static uint32_t lf_frame_tail(j40hip_frame *h, hipStream_t s) {
	j40hip_device_state *st = h->dev;
	const Frame &fr = h->frame;
	if (!h->lf_src[0] || !h->lf_src[1] || !h->lf_src[2] || !st->d_lf_frame) return ERR4('l', 'f', 'n', 'o');
	if (h->lf_src_w != (fr.fh.width + 7) / 8 || h->lf_src_h != (fr.fh.height + 7) / 8) return ERR4('l', 'f', 's', 'z');
	LfFrameArgs a;
	memset(&a, 0, sizeof a);
	for (int c = 0; c < 3; ++c) {
		a.src[c] = h->lf_src[c];
		const float mult_lf = fr.m_lf_scaled[c] / (float) (fr.global_scale * fr.quant_lf) * (float) 65536;
		a.nb_thr[c] = std::min(fr.nb_lf_thr[c], 15);
		for (int32_t t = 0; t < a.nb_thr[c]; ++t) a.thr[c][t] = (float) fr.lf_thr[c][t] * mult_lf;
	}
	a.src_w = h->lf_src_w; a.src_h = h->lf_src_h;
	const bool bctx = fr.nb_lf_thr[0] + fr.nb_lf_thr[1] + fr.nb_lf_thr[2] > 0;   // (lfidx_size > 1)
	launch_lf_frame_tail(st->plan, (int32_t) fr.lf_groups.size(), st->lf_max_cells, st->lf_cells, st->d_lf_frame, st->d_vb_sorted, (int32_t) st->vb_count, st->class_start[18], a, bctx, (int32_t) fr.fh.num_groups, s);
	return 0;
}

// Make the planes of a VarDCT plan: the pixel kernels with OutMode::XYB, then the restoration filters (`filters`: their mode, 0: they do
// not run). Where: the caller's slot (run.xyb_out) when nothing runs over the planes afterwards; the padded planes of a 4:4:4 YCbCr frame
// the filters do not run on; else the frame's own, from where what the filters leave is copied into the slot. *out: where they lie.
static uint32_t vardct_planes(j40hip_frame *h, const VardctRun &run, int filters, hipStream_t s, float **out, size_t *out_pitch) {
	j40hip_device_state *st = h->dev;
	const FrameHeader &fh = h->frame.fh;
	float *d = run.xyb_out;
	size_t pitch = (size_t) fh.width;
	if (st->ycbcr && !filters) {   // (rows padded to 16 bytes)
		pitch = ((size_t) fh.width + 3) & ~(size_t) 3;
		if (!st->keep(st->d_ycc, 3 * pitch * (size_t) fh.height)) return ERR_MEM;
		d = st->d_ycc;
	} else if (filters || !d) if (uint32_t e = plane_buffer(st, fh, &d)) return e;
	launch_vardct_frame(st->plan, run.class_start, run.list, st->d_large_scratch, K2Target{d, pitch * 4, OutMode::XYB, 0}, s);
	if (filters) {
		if (uint32_t e = run_filters(h, filters, s)) return e;
		d = const_cast<float *>(st->d_restored);   // (the filters' own buffer: nothing else reads it before the next decode)
		if (run.xyb_out && hipMemcpyAsync(run.xyb_out, d, sizeof(float) * 3 * pitch * (size_t) fh.height, hipMemcpyDeviceToDevice, s) != hipSuccess) return ERR_GPU;
	}
	*out = d; *out_pitch = pitch;
	return 0;
}

static uint32_t run_vardct(j40hip_frame *h, const VardctRun &run, hipStream_t s, float *ms3) {
	j40hip_device_state *st = h->dev;
	const DevPlan &plan = st->plan;
	const StageMarks marks{ms3 ? st->ev : nullptr, s};
	h->last = LastDecode();   // (what the last decode left behind for j40hip_frame_status and the getters: every decode starts from none of it)
	// What follows the entropy kernels, decided before anything is launched. The restoration filters asked for and signalled run where
	// their parameters are valid; else the picture comes without them and their complaint behind the sections' own (j40hip_frame_status).
	// The decode goes through the plane stage for them, for the colour mode, for patches, for a 4:4:4 YCbCr plan (a subsampled one whose
	// filters run is treated as one) and for a caller that wants the planes; anything else takes the fused pixel kernels.
	int filters = 0;
	if (run.restoration) {
		const uint32_t complaint = restore_prepared(h).err;
		if (complaint) h->last.restore_err = complaint; else filters = run.restoration;
	}
	const bool planes = filters || run.colour || run.patches || (st->ycbcr && !h->frame.fh.subsampled()) || run.xyb_out;
	if (planes && (!run.whole || run.shift || run.cover)) return ERR_TODO;   // (cannot happen: the route decodes such a frame whole and at full size)
	marks.mark(0);
	if (uint32_t e = clear_before_decode(st, s)) return e;
	if (hipMemsetAsync(plan.status, 0, sizeof(uint32_t) * (size_t) st->total_sections, s) != hipSuccess) return ERR_GPU;
	if (h->frame.fh.use_lf_frame) { if (uint32_t e = lf_frame_tail(h, s)) return e; }
	marks.mark(1);
	// (k_hf_entropy takes a run of groups and every pass of them)
	if (!run.cover) launch_hf_entropy(plan, st->hf, run.first_group, run.num_groups, s);
	else if (hf_entropy_fast_path(plan, st->hf)) launch_hf_entropy_fast_ordered(plan, st->hf, st->region.d_order, 0, region_cover_groups(*run.cover), s);
	else for (int32_t row = 0; row < run.cover->rows; ++row) launch_hf_entropy(plan, st->hf, (run.cover->gy0 + row) * run.cover->gcolumns + run.cover->gx0, run.cover->cols, s);
	marks.mark(2);
	if (planes) {
		float *d = nullptr; size_t pitch = 0;
		if (uint32_t e = vardct_planes(h, run, filters, s, &d, &pitch)) return e;
		if (!run.xyb_out) if (uint32_t e = render_planes(h, d, pitch, run.colour, run.img, run.img_stride, s)) return e;
	} else if (st->ycbcr) {
		if (uint32_t e = ycbcr_pixels(h, run.class_start, run.list, run.img, run.img_stride, s)) return e;
	} else launch_vardct_frame(plan, run.class_start, run.list, st->d_large_scratch, K2Target{run.img, run.img_stride, out_mode(h), run.shift}, s);
	if (run.crop_to) launch_region_crop(run.crop_from, run.img_stride, run.crop_to, run.crop_stride, run.crop_w, run.crop_h, (int32_t) pixel_bytes(h), s);
	marks.mark(3);
	if (uint32_t e = marks.finish(ms3)) return e;
	if (hipGetLastError() != hipSuccess) return ERR_GPU;
	if (st->has_trailers) return finish_trailers(h, run.img, run.img_stride, s, run.whole, run.alpha_merged);   // (synchronises `s`)
	return 0;
}

static uint32_t decode_region(j40hip_frame *h, const DecodeRoute &route, void *rgba_dev, size_t stride_bytes, hipStream_t s, float *ms3);
static uint32_t decode_scaled(j40hip_frame *h, const DecodeRoute &route, void *rgba_dev, size_t stride_bytes, hipStream_t s, float *ms3);

// The stored-order decode of a route that refuses nothing (decode_oriented has looked). full_size: decode_region's and decode_scaled's
// own call for a route with full_size_first -- the whole frame at full size, whatever shape the route has
static uint32_t decode_impl(j40hip_frame *h, const DecodeRoute &route, void *rgba_dev, size_t stride_bytes, hipStream_t s, float *ms3, bool full_size = false) {
	if (route.shape == DecodeRoute::Region && !full_size) return decode_region(h, route, rgba_dev, stride_bytes, s, ms3);
	if (route.shape == DecodeRoute::Scaled && !full_size) return decode_scaled(h, route, rgba_dev, stride_bytes, s, ms3);
	j40hip_device_state *st = h->dev;
	if (hipSetDevice(st->device) != hipSuccess) return ERR_GPU;
	if (st->is_modular) return decode_modular(h, route, rgba_dev, stride_bytes, s, ms3);
	VardctRun run(h, route);
	run.img = (uint8_t *) rgba_dev; run.img_stride = stride_bytes;
	if (!route.every_group) {   // a sharded decode: only this process' groups and their varblocks
		run.first_group = (int32_t) st->first_group; run.num_groups = (int32_t) st->num_groups; run.whole = false;
		run.list = st->d_vb_range; run.class_start = st->range_class_start;
	}
	return run_vardct(h, run, s, ms3);
}

// An LF frame of a sequence (runtime_seq.hip: play_frame): the whole frame decoded to its three XYB planes at `planes` (width * height
// floats each, one behind the other), no colour conversion, no pixels -- a VarDCT frame's as the inverse transforms or the restoration
// filters leave them, a Modular XYB frame's integer planes through k_modular_to_xyb. Enqueued on `s` like j40hip_frame_decode.
uint32_t j40hip_rt::decode_frame_xyb(j40hip_frame *h, float *planes, hipStream_t s) {
	if (!h || !h->dev || !planes) return ERR_GPU;
	j40hip_device_state *st = h->dev;
	const DecodeRoute route = route_of(h);
	if (route.xyb_refusal) return route.xyb_refusal;
	if (hipSetDevice(st->device) != hipSuccess) return ERR_GPU;
	if (st->is_modular) return decode_modular(h, route, nullptr, 0, s, nullptr, nullptr, 0, planes);
	VardctRun run(h, route);
	run.xyb_out = planes;
	return run_vardct(h, run, s, nullptr);
}

// ---- region decode (j40hip_frame_set_region, include/j40hip.h; device/region_dev.h, region_kernels.hip) ----
// An image of img_w x img_h pixels in the staging block -- kept with the frame and grown on demand, so that nothing is allocated on the path of
// a later decode and the asynchronous entry point stays asynchronous -- whose pixel (off_x, *) sits within 16 bytes like the destination's rows
// do, so that k_region_crop moves every row in 16-byte pieces; *stride: its row stride. Null: no memory.
static uint8_t *region_image(j40hip_frame *h, const void *dst, size_t dst_stride, int32_t img_w, int32_t img_h, int32_t off_x, size_t *stride) {
	const size_t pb = pixel_bytes(h), row = ((size_t) img_w * pb + 15) & ~(size_t) 15;
	const bool alike = (uintptr_t) dst % pb == 0 && dst_stride % pb == 0;   // (else the rows stay pixel by pixel)
	*stride = row + (alike ? dst_stride & 15 : 0);
	const size_t lead = alike ? ((uintptr_t) dst - (size_t) off_x * pb) & 15 : 0;
	CacheBlock &block = h->dev->region.staging;
	return block.ensure(h->dev->device, lead + *stride * (size_t) img_h + 16, false) ? (uint8_t *) block.ptr + lead : nullptr;
}

// the group-major index of the varblock list, once per upload: three kernels and one copy back of the segments' starts
static uint32_t region_index(j40hip_frame *h, hipStream_t s) {
	j40hip_device_state *st = h->dev;
	j40hip_device_state::Region &rg = st->region;
	if (rg.index_ready) return 0;
	const FrameHeader &fh = h->frame.fh;
	const size_t nkeys = (size_t) fh.num_groups * REGION_KEYS;
	bool ok = true;
	if (!rg.d_order) {
		rg.d_cursor = st->scratch<uint32_t>(nkeys, ok); rg.d_seg_start = st->scratch<uint32_t>(nkeys + 1, ok);
		rg.d_index = st->scratch<uint32_t>(std::max<size_t>(st->vb_count, 1), ok); rg.d_order = st->scratch<uint32_t>((size_t) fh.num_groups, ok);
		if (!ok) { rg.d_order = nullptr; return ERR_MEM; }
	}
	launch_region_index(st->d_vb_sorted, (uint32_t) st->vb_count, fh.group_size_shift, fh.gcolumns, (uint32_t) nkeys, rg.d_cursor, rg.d_seg_start, rg.d_index, s);
	std::vector<uint32_t> starts(nkeys + 1);
	if (hipMemcpyAsync(starts.data(), rg.d_seg_start, sizeof(uint32_t) * starts.size(), hipMemcpyDeviceToHost, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess) return ERR_GPU;
	if (starts[nkeys] != (uint32_t) st->vb_count) return ERR_GPU;
	rg.counts.resize(nkeys);
	for (size_t k = 0; k < nkeys; ++k) rg.counts[k] = starts[k + 1] - starts[k];
	rg.index_ready = true;
	return 0;
}

// the cover's varblocks and groups into the region's lists; nothing to do when the last region had the same cover
static uint32_t region_gather(j40hip_frame *h, const RegionCover &cover, hipStream_t s) {
	j40hip_device_state *st = h->dev;
	j40hip_device_state::Region &rg = st->region;
	if (uint32_t e = region_index(h, s)) return e;
	const RegionCover &g = rg.gathered;
	if (g.cols == cover.cols && g.rows == cover.rows && g.gx0 == cover.gx0 && g.gy0 == cover.gy0) return 0;
	// class_start from the host's count table: per class, the cover's groups summed
	int32_t at = 0;
	for (int d = 0; d < REGION_KEYS; ++d) {
		rg.class_start[d] = at;
		for (int32_t i = 0; i < region_cover_groups(cover); ++i) at += (int32_t) rg.counts[(size_t) region_cover_group(cover, i) * REGION_KEYS + (size_t) d];
	}
	const size_t total = (size_t) rg.class_start[REGION_KEYS - 1];   // (class 27 does not exist: the last entry is the end)
	if (total > rg.list_capacity) {
		bool ok = true;
		const size_t want = std::min(st->vb_count, total + total / 2);
		rg.gathered.cols = 0;
		rg.d_list = st->scratch<DevVarblock>(want, ok);
		if (!ok) { rg.d_list = nullptr; rg.list_capacity = 0; return ERR_MEM; }
		rg.list_capacity = want;
	}
	launch_region_gather(st->d_vb_sorted, rg.d_index, rg.d_seg_start, cover, rg.class_start, rg.d_list, rg.d_order, s);
	rg.gathered = cover;
	return 0;
}

static uint32_t decode_region(j40hip_frame *h, const DecodeRoute &route, void *rgba_dev, size_t stride_bytes, hipStream_t s, float *ms3) {
	j40hip_device_state *st = h->dev;
	const Frame &fr = h->frame;
	const int32_t x0 = h->region[0], y0 = h->region[1], w = h->region[2], hh = h->region[3];
	const size_t pb = route.pixel_bytes;
	if (hipSetDevice(st->device) != hipSuccess) return ERR_GPU;
	if (st->is_modular && !route.full_size_first) return decode_modular(h, route, rgba_dev, stride_bytes, s, ms3, h->region);   // (staged: a Modular XYB frame under the colour mode)
	const int32_t W = fr.fh.width, H = fr.fh.height, shift = fr.fh.group_size_shift;
	if (route.full_size_first) {
		// the filters read across groups, the kept alpha is merged into full-size pixels: the whole frame as ever, into a staging image
		// (of the shown size: an upsampled frame's picture is what the rectangle lies in)
		const int32_t SW = fr.fh.shown_width(), SH = fr.fh.shown_height();
		size_t img_stride = 0;
		uint8_t *img = region_image(h, rgba_dev, stride_bytes, SW, SH, x0, &img_stride);
		if (!img) return ERR_MEM;
		h->region_widened = 1; h->region_sections = st->total_sections; h->region_varblocks = (int32_t) st->vb_count;
		if (uint32_t e = decode_impl(h, route, img, img_stride, s, ms3, true)) return e;
		launch_region_crop(img + (size_t) y0 * img_stride + (size_t) x0 * pb, img_stride, (uint8_t *) rgba_dev, stride_bytes, w, hh, (int32_t) pb, s);
		return hipGetLastError() == hipSuccess ? 0 : ERR_GPU;
	}
	const RegionCover cover = region_cover(x0, y0, w, hh, shift, fr.fh.gcolumns);
	const int32_t ncover = region_cover_groups(cover);
	const bool all = ncover == (int32_t) fr.fh.num_groups;   // (the whole frame's lists and launches serve; also every single-section frame)
	if (!all) if (uint32_t e = region_gather(h, cover, s)) return e;
	const DevVarblock *list = all ? st->d_vb_sorted : st->region.d_list;
	const int32_t *class_start = all ? st->class_start : st->region.class_start;
	// the cover in pixels, and where its image goes: straight into the caller's when the rectangle is its cover
	const int32_t cx0 = cover.gx0 << shift, cy0 = cover.gy0 << shift;
	const int32_t cw = (int32_t) std::min<int64_t>(W, (int64_t) (cover.gx0 + cover.cols) << shift) - cx0, ch = (int32_t) std::min<int64_t>(H, (int64_t) (cover.gy0 + cover.rows) << shift) - cy0;
	const bool direct = x0 == cx0 && y0 == cy0 && w == cw && hh == ch;
	size_t img_stride = stride_bytes;
	uint8_t *img = direct ? (uint8_t *) rgba_dev : region_image(h, rgba_dev, stride_bytes, cw, ch, x0 - cx0, &img_stride);
	if (!img) return ERR_MEM;
	h->region_widened = 0; h->region_sections = all ? st->total_sections : fr.fh.num_passes * ncover; h->region_varblocks = class_start[REGION_KEYS - 1];
	// (drop mode, no filters, or the frame would have been widened; a partial cover does not validate the sub-images, like a group range)
	VardctRun run(h, route);
	run.cover = all ? nullptr : &cover; run.list = list; run.class_start = class_start; run.img = img; run.img_stride = img_stride; run.whole = all;
	if (!direct) { run.crop_from = img + (size_t) (y0 - cy0) * img_stride + (size_t) (x0 - cx0) * pb; run.crop_to = (uint8_t *) rgba_dev; run.crop_stride = stride_bytes; run.crop_w = w; run.crop_h = hh; }
	return run_vardct(h, run, s, ms3);
}

// ---- reduced-size decode (j40hip_frame_set_scale, include/j40hip.h; device/scale_dev.h, scale_kernels.hip) ----
// The whole frame at scale shift k: ceil(width / s) x ceil(height / s) pixels at rgba_dev. Fused: the pixel kernels (VarDCT) or the pack
// kernel (Modular) write the small image and nothing else. Staged (the route's full_size_first): the frame decodes as ever into a full-size
// image kept with the frame, and k_downscale makes the small one of it. Every section is entropy-decoded either way: status and codes
// are the full decode's.
static uint32_t decode_scaled(j40hip_frame *h, const DecodeRoute &route, void *rgba_dev, size_t stride_bytes, hipStream_t s, float *ms3) {
	j40hip_device_state *st = h->dev;
	const Frame &fr = h->frame;
	const int32_t W = fr.fh.shown_width(), H = fr.fh.shown_height(), k = h->scale;   // (the shown size: only a staged decode sees an upsampled frame)
	const size_t pb = route.pixel_bytes;
	if (hipSetDevice(st->device) != hipSuccess) return ERR_GPU;
	if (route.full_size_first) {
		const size_t img_stride = ((size_t) W * pb + 15) & ~(size_t) 15, bytes = img_stride * (size_t) H;
		if (!st->scale_staging.ensure(st->device, bytes, false)) return ERR_MEM;
		uint8_t *img = (uint8_t *) st->scale_staging.ptr;
		h->scale_staged = 1; h->scale_staging_bytes = (int64_t) bytes;
		if (uint32_t e = decode_impl(h, route, img, img_stride, s, ms3, true)) return e;
		launch_downscale(img, img_stride, (uint8_t *) rgba_dev, stride_bytes, W, H, k, (int32_t) pb, s);
		return hipGetLastError() == hipSuccess ? 0 : ERR_GPU;
	}
	h->scale_staged = 0; h->scale_staging_bytes = 0;
	if (st->is_modular) return decode_modular(h, route, rgba_dev, stride_bytes, s, ms3, nullptr, k);
	VardctRun run(h, route);
	run.img = (uint8_t *) rgba_dev; run.img_stride = stride_bytes; run.shift = k;
	return run_vardct(h, run, s, ms3);
}

// known-answer / measuring hook: k_downscale alone
extern "C" uint32_t j40hip_kat_device_downscale(void *out_dev, size_t out_stride, const void *src_dev, size_t src_stride, int32_t w, int32_t h, int32_t shift, int32_t format, void *stream) {
	if (format != J40HIP_U8X4 && format != J40HIP_U16X4) return ERR4('U', 'f', 'm', '?');
	const size_t pb = format == J40HIP_U16X4 ? 8 : 4;
	if (!out_dev || !src_dev || w <= 0 || h <= 0 || shift < 1 || shift > 2) return ERR_RNGE;
	const size_t ow = (size_t) ((w + (1 << shift) - 1) >> shift);
	if (src_stride < pb * (size_t) w || out_stride < pb * ow || src_stride % pb || out_stride % pb || (uintptr_t) out_dev % pb || (uintptr_t) src_dev % pb) return ERR_RNGE;
	launch_downscale((const uint8_t *) src_dev, src_stride, (uint8_t *) out_dev, out_stride, w, h, shift, (int32_t) pb, (hipStream_t) stream);
	return hipGetLastError() == hipSuccess ? 0 : ERR_GPU;
}

// ---- oriented output (j40hip_frame_set_orientation, include/j40hip.h; device/orient_dev.h, orient_kernels.hip) ----
// The head of the single-frame decode entries: the route's refusal, then the decode. With an orientation other than 1 in force the decode
// -- whatever it is -- is pointed at a stored-order staging image of exactly its W x H pixels, one block of the device memory cache kept
// with the frame, and k_orient then writes the caller's buffer on the same stream: the orientation is applied last.
static uint32_t decode_oriented(j40hip_frame *h, const DecodeRoute &route, void *rgba_dev, size_t stride_bytes, hipStream_t s, float *ms3) {
	if (h->dev && !h->frame.lf_only) { h->orient_applied = 0; h->orient_staging_bytes = 0; }
	if (route.refusal) return route.refusal;   // before anything is launched or allocated
	if (route.orientation == 1) return decode_impl(h, route, rgba_dev, stride_bytes, s, ms3);
	j40hip_device_state *st = h->dev;
	const int32_t W = route.stored_w, H = route.stored_h;
	const size_t img_stride = route.pixel_bytes * (size_t) W, bytes = img_stride * (size_t) H;
	if (hipSetDevice(st->device) != hipSuccess) return ERR_GPU;
	if (!st->orient_staging.ensure(st->device, bytes, false)) return ERR_MEM;
	h->orient_staging_bytes = (int64_t) bytes;
	uint8_t *img = (uint8_t *) st->orient_staging.ptr;
	if (uint32_t e = decode_impl(h, route, img, img_stride, s, ms3)) return e;
	launch_orient(img, img_stride, (uint8_t *) rgba_dev, stride_bytes, W, H, route.orientation, (int32_t) route.pixel_bytes, s);   // (any alignment of pointer and stride serves, as in stored order)
	h->orient_applied = 1;
	return hipGetLastError() == hipSuccess ? 0 : ERR_GPU;
}
// the decode entry points' head: the route of this call, then the decode
static uint32_t decode_entry(j40hip_frame *h, void *rgba_dev, size_t stride_bytes, hipStream_t s, float *ms3) {
	if (!h) return ERR_GPU;
	return decode_oriented(h, route_of(h, rgba_dev != nullptr, stride_bytes), rgba_dev, stride_bytes, s, ms3);
}

// known-answer / measuring hook: k_orient alone
extern "C" uint32_t j40hip_kat_device_orient(void *out_dev, size_t out_stride, const void *src_dev, size_t src_stride, int32_t w, int32_t h, int32_t orientation, int32_t format, void *stream) {
	if (format != J40HIP_U8X4 && format != J40HIP_U16X4) return ERR4('U', 'f', 'm', '?');
	const size_t pb = format == J40HIP_U16X4 ? 8 : 4;
	if (!out_dev || !src_dev || w <= 0 || h <= 0 || w > (1 << 28) || h > (1 << 28) || !orient_valid(orientation)) return ERR_RNGE;
	int32_t ow, oh;
	orient_out_size(w, h, orientation, &ow, &oh);
	if (src_stride < pb * (size_t) w || out_stride < pb * (size_t) ow || src_stride % pb || (uintptr_t) src_dev % pb) return ERR_RNGE;   // (the source pixel-aligned; the output anywhere)
	if (orientation == 1) {
		if (hipMemcpy2DAsync(out_dev, out_stride, src_dev, src_stride, pb * (size_t) w, (size_t) h, hipMemcpyDeviceToDevice, (hipStream_t) stream) != hipSuccess) return ERR_GPU;
		return 0;
	}
	launch_orient((const uint8_t *) src_dev, src_stride, (uint8_t *) out_dev, out_stride, w, h, orientation, (int32_t) pb, (hipStream_t) stream);
	return hipGetLastError() == hipSuccess ? 0 : ERR_GPU;
}

extern "C" uint32_t j40hip_frame_decode(j40hip_frame *h, void *rgba_dev, size_t stride_bytes, void *stream) {
	return guarded([&] { return decode_entry(h, rgba_dev, stride_bytes, (hipStream_t) stream, nullptr); });
}

extern "C" uint32_t j40hip_frame_decode_timed(j40hip_frame *h, void *rgba_dev, size_t stride_bytes, void *stream, float *ms3) {
	return guarded([&] { return decode_entry(h, rgba_dev, stride_bytes, (hipStream_t) stream, ms3); });
}

// Status words reduced to a frame's verdict: the code of the first failing section in the order the reference reads them, which is the
// order of their offsets in the stream (offset_of(i); two failing sections at one offset: the smaller code); 0: none failed
template <typename F> static uint32_t first_failure(const std::vector<uint32_t> &status, size_t n, F offset_of) {
	size_t best = SIZE_MAX; uint32_t code = 0;
	for (size_t i = 0; i < n; ++i) if (status[i] && (offset_of(i) < best || (offset_of(i) == best && status[i] < code))) { best = offset_of(i); code = status[i]; }
	return code;
}
static uint32_t vardct_verdict(const j40hip_frame *h, const std::vector<uint32_t> &status) {
	const Frame &fr = h->frame;
	if (fr.toc.single) return status.empty() ? 0 : status[0];
	return first_failure(status, status.size(), [&](size_t i) { return fr.toc.pass_groups[i].offset; });
}

static uint32_t j40hip_frame_status_body(j40hip_frame *h) {
	if (!h || !h->dev) return ERR_GPU;
	j40hip_device_state *st = h->dev;
	if (st->is_modular) {
		st->status_host.assign((size_t) st->total_sections + 1, 0);
		if (hipMemcpy(st->status_host.data(), st->mod.status, sizeof(uint32_t) * st->status_host.size(), hipMemcpyDeviceToHost) != hipSuccess) return ERR_GPU;
		const uint32_t code = first_failure(st->status_host, (size_t) st->total_sections, [&](size_t i) { return (size_t) st->mod_section_offsets[i]; });
		return code ? code : st->status_host[(size_t) st->total_sections];
	}
	if (h->last.trailers_pending) {
		// the frame was last decoded by a batch (asynchronous: it cannot stop for the host in the middle): the extra channels'
		// sub-images behind the coefficients are checked now, so that both modes report damage in them like the reference
		h->last.trailers_pending = false;
		if (hipSetDevice(st->device) != hipSuccess) return ERR_GPU;
		if (uint32_t e = finish_trailers(h, st->pending_rgba, st->pending_stride, nullptr, true, route_of(h).alpha_merged)) return e;
	}
	st->status_host.assign((size_t) st->total_sections, 0);
	if (hipMemcpy(st->status_host.data(), st->plan.status, sizeof(uint32_t) * st->status_host.size(), hipMemcpyDeviceToHost) != hipSuccess) return ERR_GPU;
	const uint32_t code = vardct_verdict(h, st->status_host);
	return code ? code : h->last.restore_err;   // (the filters run behind the last section: their complaint comes after every section's)
}

// ---- the single-image path in two phases ----
// One image alone is its longest section: every section has a wavefront and a SIMD of its own, the entropy launch lasts as long as the
// longest of them (1.9 x the mean in the bench's 8K frame), and 133 MB of pixels then take 2.3 ms over the link while the device has
// nothing left to do. Here the few longest sections -- those within the copy's time of the longest -- are decoded by a launch of their
// own on a second stream, beside the launch of all the others; when THAT one is through the pixel kernels run over the whole frame
// (the long sections' blocks, whose block_events entries are still zero, come out as their LF only) and the whole image starts over
// the link; when the long sections are through their block_events entries -- written to a table of their own meanwhile, so that the
// first pass never sees one half written -- are merged in, the pixel kernels run again (0.3 ms; same pixels everywhere else), and
// only the long sections' groups, a 256 x 256 rectangle each, follow the image over the link. Same pixels and codes as the one-phase
// decode (tests/test_gpu_parity.py runs both); J40HIP_TWO_PHASE=0: never.
struct TwoPhaseStream {   // a second stream and three events on a device, borrowed for one decode (hipStreamCreate is not for the path of one image)
	int device = -1; hipStream_t s = nullptr; hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
};
static IdlePool<TwoPhaseStream> g_two_phase_idle;   // (handed back after every decode)
static bool two_phase_borrow(int dev, TwoPhaseStream *out) {
	if (g_two_phase_idle.take(dev, out)) return true;
	TwoPhaseStream t;
	t.device = dev;
	if (hipStreamCreateWithFlags(&t.s, hipStreamNonBlocking) != hipSuccess) { (void) hipGetLastError(); return false; }
	for (auto &e : t.ev) if (hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) {
		(void) hipGetLastError();
		for (auto &d : t.ev) if (d) (void) hipEventDestroy(d);
		(void) hipStreamDestroy(t.s);
		return false;
	}
	*out = t;
	return true;
}
void j40hip_rt::two_phase_shutdown() {
	g_two_phase_idle.drain([](TwoPhaseStream &t) { if (hipSetDevice(t.device) != hipSuccess) return; (void) hipStreamDestroy(t.s); for (auto &e : t.ev) if (e) (void) hipEventDestroy(e); });
}

// decides once per upload whether the frame is decoded in two phases and with which groups on the second stream (st->two_k of st->two_order)
static void two_phase_plan(j40hip_frame *h, size_t image_bytes, bool every_group) {
	j40hip_device_state *st = h->dev;
	st->two_k = 0;
	const bool allowed = env_on("J40HIP_TWO_PHASE", true);   // (looked at per upload: tests switch it between frames)
	const Frame &fr = h->frame;
	const int64_t ng = fr.fh.num_groups;
	if (!allowed || st->is_modular || st->ycbcr || !st->plan.events || !st->plan.block_events || st->has_trailers || fr.toc.single || fr.fh.num_passes != 1 || ng < 64 || image_bytes < ((size_t) 16 << 20)) return;
	if (!every_group || fr.toc.pass_groups.size() != (size_t) ng) return;
	if (!hf_entropy_fast_path(st->plan, st->hf)) return;
	std::vector<uint32_t> order((size_t) ng);
	for (int64_t g = 0; g < ng; ++g) order[(size_t) g] = (uint32_t) g;
	std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return fr.toc.pass_groups[a].size > fr.toc.pass_groups[b].size; });
	// a section takes about a microsecond a byte on its wavefront, the link 57 GB/s: the sections within the copy's time of the longest
	const double copy_us = (double) image_bytes / 57e3, longest = (double) fr.toc.pass_groups[order[0]].size;
	int32_t k = 0;
	while (k < (int32_t) ng && k < 64 && (double) fr.toc.pass_groups[order[(size_t) k]].size > longest - 1.25 * copy_us) ++k;
	if (k < 1 || k > ng / 4) return;
	// the order and the long sections' table: one recycled block (a hipMalloc of 16 MB is a millisecond, on the path of one image)
	const size_t order_bytes = ((size_t) ng * 4 + 255) & ~(size_t) 255, shadow_bytes = 16 * st->num_blocks;
	if (!st->two_block.ensure(st->device, order_bytes + shadow_bytes, true)) return;
	st->d_two_order = (uint32_t *) st->two_block.ptr; st->d_two_shadow = (uint32_t *) ((uint8_t *) st->two_block.ptr + order_bytes);
	if (hipMemcpy(st->d_two_order, order.data(), (size_t) ng * 4, hipMemcpyHostToDevice) != hipSuccess || hipMemsetAsync(st->d_two_shadow, 0, shadow_bytes, nullptr) != hipSuccess) { (void) hipGetLastError(); return; }   // (the fill: ahead of the decode's launches on its stream)
	st->two_order = std::move(order);
	st->two_k = k;
}

// pixels of a whole VarDCT frame into rgba_host; d: the device image (stride_bytes per row). Returns the frame's code like decode_impl +
// j40hip_frame_status would; *done = false: nothing was enqueued, the caller decodes the usual way.
static uint32_t decode_two_phase(j40hip_frame *h, const DecodeRoute &route, uint8_t *d, uint8_t *rgba_host, size_t stride_bytes, bool *done) {
	*done = false;
	j40hip_device_state *st = h->dev;
	const Frame &fr = h->frame;
	const size_t bytes = stride_bytes * (size_t) fr.fh.height;
	if (st->two_k < 0) two_phase_plan(h, bytes, route.every_group);
	if (st->two_k <= 0 || route.restoration_asked || !route.every_group) return 0;   // (a restoration mode, or a group range set since the plan: the usual way)
	TwoPhaseStream tp;
	if (!two_phase_borrow(st->device, &tp)) return 0;
	struct GiveBack { const TwoPhaseStream &t; ~GiveBack() { (void) hipStreamSynchronize(t.s); g_two_phase_idle.give(t); } } give_back{tp};   // (whatever way the decode ends: nothing of it is left on the stream)
	*done = true;
	const bool timing = api_timing();
	auto now = [] { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
	const double t0 = timing ? now() : 0;
	const DevPlan &plan = st->plan;
	const int32_t ng = (int32_t) fr.fh.num_groups, k = st->two_k;
	hipStream_t s0 = nullptr, s1 = tp.s;
	h->last = LastDecode();   // (what the last decode left behind for j40hip_frame_status and the getters: every decode starts from none of it)
	if (hipMemsetAsync(plan.status, 0, sizeof(uint32_t) * (size_t) st->total_sections, s0) != hipSuccess) return ERR_GPU;
	if (hipEventRecord(tp.ev[0], s0) != hipSuccess || hipStreamWaitEvent(s1, tp.ev[0], 0) != hipSuccess) return ERR_GPU;
	DevPlan plan_long = plan;
	plan_long.block_events = st->d_two_shadow;
	launch_hf_entropy_fast_ordered(plan_long, st->hf, st->d_two_order, 0, k, s1);          // the long sections, on their own
	launch_hf_entropy_fast_ordered(plan, st->hf, st->d_two_order, k, ng - k, s0);           // all the others
	launch_vardct_frame(plan, st->class_start, st->d_vb_sorted, st->d_large_scratch, K2Target{d, stride_bytes, out_mode(h), 0}, s0);
	if (hipEventRecord(tp.ev[1], s0) != hipSuccess || hipStreamWaitEvent(s1, tp.ev[1], 0) != hipSuccess) return ERR_GPU;
	launch_merge_block_events(plan, st->d_two_order, k, st->d_two_shadow, s1);
	launch_vardct_frame(plan, st->class_start, st->d_vb_sorted, st->d_large_scratch, K2Target{d, stride_bytes, out_mode(h), 0}, s1);
	if (hipEventRecord(tp.ev[2], s1) != hipSuccess) return ERR_GPU;
	if (hipGetLastError() != hipSuccess) return ERR_GPU;
	// the image of the first pass over the link while the long sections are still being decoded: the copy the one-phase decode issues,
	// behind the first pass on its stream (the host waits in it)
	const double t1 = timing ? now() : 0;
	if (hipEventSynchronize(tp.ev[1]) != hipSuccess) return ERR_GPU;
	const double t2 = timing ? now() : 0;
	if (!hostcopy_d2h_sync(st->device, rgba_host, d, bytes) && hipMemcpy(rgba_host, d, bytes, hipMemcpyDeviceToHost) != hipSuccess) return ERR_GPU;
	const double t3 = timing ? now() : 0;
	// the long sections' groups, one rectangle each, on top: written by a kernel where the device can reach the host's image (pinned
	// memory: the public API's planes) -- a 2-D copy per rectangle is 0.1 ms each --, else copied one by one
	uint8_t *mapped = nullptr;
	{
		hipPointerAttribute_t at;
		if (hipPointerGetAttributes(&at, rgba_host) == hipSuccess && at.type == hipMemoryTypeHost && at.devicePointer) mapped = (uint8_t *) at.devicePointer;
		else (void) hipGetLastError();
	}
	const int32_t shift = fr.fh.group_size_shift, gdim = 1 << shift;
	const size_t pb = route.pixel_bytes;
	if (mapped) launch_store_group_rects(st->d_two_order, k, fr.fh.gcolumns, shift, fr.fh.width, fr.fh.height, d, mapped, stride_bytes, s1, (int32_t) pb);
	else {
		if (hipEventSynchronize(tp.ev[2]) != hipSuccess) return ERR_GPU;
		for (int32_t i = 0; i < k; ++i) {
			const int64_t g = st->two_order[(size_t) i], gx = g % fr.fh.gcolumns, gy = g / fr.fh.gcolumns;
			const size_t x0 = (size_t) gx << shift, y0 = (size_t) gy << shift;
			const size_t w = std::min<size_t>((size_t) gdim, (size_t) fr.fh.width - x0), rows = std::min<size_t>((size_t) gdim, (size_t) fr.fh.height - y0);
			const size_t off = y0 * stride_bytes + x0 * pb;
			if (hipMemcpy2DAsync(rgba_host + off, stride_bytes, d + off, stride_bytes, w * pb, rows, hipMemcpyDeviceToHost, s1) != hipSuccess) return ERR_GPU;
		}
	}
	const double t4 = timing ? now() : 0;
	if (hipStreamSynchronize(s1) != hipSuccess) return ERR_GPU;
	if (timing) fprintf(stderr, "[j40hip two phases] %d long sections of %d: enqueued %.2f ms, the others + first pass through after %.2f, image over the link %.2f, long sections + second pass + %d rectangles (%s) another %.2f ms\n",
		k, ng, t1 - t0, t2 - t1, t3 - t2, k, mapped ? "a kernel's stores" : "2-D copies", now() - t3);
	(void) t4;
	return j40hip_frame_status(h);
}

static uint32_t decode_to_host(j40hip_frame *h, void *rgba_host, size_t stride_bytes) {
	if (!h) return ERR_GPU;
	DecodeRoute route = route_of(h, true, stride_bytes);
	if (h->dev && !h->frame.lf_only) { h->orient_applied = 0; h->orient_staging_bytes = 0; }
	if (route.refusal) return route.refusal;   // before the block is taken
	const int device = h->dev->device;
	if (hipSetDevice(device) != hipSuccess) return ERR_GPU;
	// the device image uses the caller's row stride, so one contiguous copy brings it back
	const size_t bytes = stride_bytes * (size_t) route.out_h;
	ScopedBlock block;   // (whatever way the call ends, the image goes back behind a device-wide wait)
	if (!block.ensure(device, bytes, true)) return ERR_GPU;
	void *d = block.ptr;
	// (two phases: whole frames in stored order only -- just the rectangle's rows, the small image's or the oriented one's exist on either side)
	bool two_phase = false;
	uint32_t err = route.two_phase ? decode_two_phase(h, route, (uint8_t *) d, (uint8_t *) rgba_host, stride_bytes, &two_phase) : 0;
	if (two_phase && err != ERR_EVOF) return err;   // (the pixels are in rgba_host, or the frame has failed; "evof": the dense form below)
	if (two_phase) (void) hipDeviceSynchronize();
	// the device-side path, waited for (wait_with_dense_retry: the route is resolved anew for the frame uploaded again)
	err = decode_oriented(h, route, d, stride_bytes, nullptr, nullptr);
	if (!err) err = wait_with_dense_retry(h, device, nullptr, [&] { route = route_of(h, true, stride_bytes); return decode_oriented(h, route, d, stride_bytes, nullptr, nullptr); });
	// (the decode has been waited for: the copy may go to the SDMA engine a pipeline of this process measured, hostcopy.hpp)
	if (!err && !hostcopy_d2h_sync(device, rgba_host, d, bytes) && hipMemcpy(rgba_host, d, bytes, hipMemcpyDeviceToHost) != hipSuccess) err = ERR_GPU;
	return err;
}
extern "C" uint32_t j40hip_frame_status(j40hip_frame *h) { return guarded([&] { return j40hip_frame_status_body(h); }); }
extern "C" int32_t j40hip_frame_two_phase_sections(const j40hip_frame *h) { return h && h->dev ? h->dev->two_k : -1; }
extern "C" uint32_t j40hip_frame_decode_to_host(j40hip_frame *h, void *rgba_host, size_t stride_bytes) { return guarded([&] { return decode_to_host(h, rgba_host, stride_bytes); }); }
// j40hip_frame_status in two halves for pipelines: `begin` enqueues the copy of the status words on `stream` (no host wait),
// `end` -- after the caller has waited for that stream -- reduces them to the frame's verdict. VarDCT frames without extra
// channels only (others: ERR_TODO; use j40hip_frame_status).
extern "C" uint32_t j40hip_frame_status_begin(j40hip_frame *h, void *stream) {
	if (!h || !h->dev) return ERR_GPU;
	j40hip_device_state *st = h->dev;
	if (st->is_modular || st->has_trailers) return ERR_TODO;
	st->status_host.assign((size_t) st->total_sections, 0);
	return hipMemcpyAsync(st->status_host.data(), st->plan.status, sizeof(uint32_t) * st->status_host.size(), hipMemcpyDeviceToHost, (hipStream_t) stream) == hipSuccess ? 0 : ERR_GPU;
}
extern "C" uint32_t j40hip_frame_status_end(j40hip_frame *h) {
	if (!h || !h->dev || h->dev->status_host.size() != (size_t) h->dev->total_sections) return ERR_GPU;
	return vardct_verdict(h, h->dev->status_host);
}
extern "C" void j40hip_frame_mark_idle(j40hip_frame *h) { if (h && h->dev) h->dev->idle = true; }
