// j40_amd/csrc/device/runtime_state.hpp -- internal to device_memory.hip and the runtime*.hip units: a frame's device state
// (j40hip_device_state), the error codes, the small helpers every unit uses and the declarations of what crosses units
#pragma once
#include <hip/hip_runtime.h>
#include <deque>
#include <condition_variable>
#include <chrono>
#include <thread>
#include <algorithm>
#include <mutex>
#include <atomic>
#include <cmath>
#include <unistd.h>
#include "../decode_route.hpp"
#include "../tables.hpp"
#include "../plan_build.hpp"
#include "../mod_layout.hpp"
#include "kernels.h"
#include "modular_xyb_dev.h"
#include "colour_dev.h"
#include "runtime_shared.hpp"

using namespace j40hip;      // (an internal header: every unit that includes it is written in these two namespaces)
using namespace j40hip_rt;

namespace j40hip_rt {

constexpr uint32_t ERR4(char a, char b, char c, char d) { return ((uint32_t) (uint8_t) a << 24) | ((uint32_t) (uint8_t) b << 16) | ((uint32_t) (uint8_t) c << 8) | (uint32_t) (uint8_t) d; }
constexpr uint32_t ERR_GPU = ERR4('!', 'g', 'p', 'u'), ERR_MEM = ERR4('!', 'm', 'e', 'm');

// no exception crosses the C ABI: a parse error keeps its code, anything else (std::bad_alloc from a vector, ...) is "!mem"
template <typename F> uint32_t guarded(F f) {
	try { return f(); }
	catch (const DecodeError &e) { return e.code; }
	catch (const std::exception &) { return ERR_MEM; }
}

struct DeviceBuffer {
	void *ptr = nullptr; size_t bytes = 0;
	bool alloc(size_t n);   // (device_memory.hip)
	void release() { if (ptr) (void) hipFree(ptr); ptr = nullptr; }
};

// a temporary block of a synchronous call: back to the cache behind a device-wide wait on every return path (such calls return long
// before process exit, so this one may have a destructor)
struct ScopedBlock : CacheBlock { ~ScopedBlock() { release(false); } };

// this thread's pinned buffers and event (device_memory.hip; j40hip_thread_release frees them). No destructors: at process exit the
// runtime may be gone before the thread's storage.
extern thread_local PinnedStage t_stage;    // an upload's staged plan
extern thread_local PinnedStage t_lf_out;   // lf_device_decode's results land here; LfDeviceTask's pointers point into it until the thread's next call
extern thread_local hipEvent_t t_lf_done;
extern thread_local HostPlan t_host_plan;   // upload_impl's, storage kept from frame to frame

struct Stager {
	size_t size = 0; bool ok = true;
	// deferred: put() notes the copy, flush() makes them all, shared out by bytes over a few threads (an 8K frame's plan is 30 MB: a
	// millisecond of one core's memcpy on the single-image path); the sources have to live until then
	bool deferred = false;
	struct Copy { size_t off; const uint8_t *src; size_t bytes; };
	std::vector<Copy> copies;
	template <typename T> size_t put(const T *src, size_t n) {
		const size_t off = (size + 255) & ~(size_t) 255, end = off + sizeof(T) * n + 16;
		if (!ok || !t_stage.reserve(end, size)) { ok = false; return 0; }
		if (n) { if (deferred) copies.push_back({off, (const uint8_t *) src, sizeof(T) * n}); else memcpy(t_stage.ptr + off, src, sizeof(T) * n); }
		size = end;   // (deferred: a grown buffer keeps the bytes below `size` -- nothing of the noted copies is there yet, and nothing needs to be)
		return off;
	}
	void flush(int threads) {
		if (!deferred || !ok) { copies.clear(); return; }
		size_t total = 0;
		for (const Copy &c : copies) total += c.bytes;
		const int n = total < ((size_t) 4 << 20) ? 1 : std::max(1, std::min(threads, 8));
		uint8_t *base = t_stage.ptr;
		auto work = [&](int t) {
			const size_t lo = total / (size_t) n * (size_t) t, hi = t + 1 == n ? total : total / (size_t) n * (size_t) (t + 1);
			size_t at = 0;
			for (const Copy &c : copies) {
				const size_t a = std::max(lo, at), b = std::min(hi, at + c.bytes);
				if (a < b) memcpy(base + c.off + (a - at), c.src + (a - at), b - a);
				at += c.bytes;
			}
		};
		std::vector<std::thread> pool;
		try { for (int t = 1; t < n; ++t) pool.emplace_back(work, t); } catch (const std::exception &) {}
		const int started = (int) pool.size() + 1;
		work(0);
		for (int t = started; t < n; ++t) work(t);   // (threads that could not be had: their share here)
		for (auto &th : pool) th.join();
		copies.clear();
	}
	size_t reserve(size_t bytes) {   // room in the device block that nothing is copied into (the bytes staged for it are whatever is there)
		const size_t off = (size + 255) & ~(size_t) 255, end = off + bytes + 16;
		if (!ok || !t_stage.reserve(end, size)) { ok = false; return 0; }
		size = end;
		return off;
	}
	const uint8_t *data() const { return t_stage.ptr; }
};

// Four events around the three stages of a decode (clear | entropy | pixels), recorded on `s`; ev null: nothing is recorded or timed
struct StageMarks {
	hipEvent_t *ev; hipStream_t s;
	void mark(int i) const { if (ev) (void) hipEventRecord(ev[i], s); }
	// waits for the last mark; ms3[0]: entropy, [1]: pixels, [2]: clear
	uint32_t finish(float *ms3) const {
		if (!ev) return 0;
		if (hipEventSynchronize(ev[3]) != hipSuccess) return ERR_GPU;
		float t[3] = {0, 0, 0};
		for (int i = 0; i < 3; ++i) (void) hipEventElapsedTime(&t[i], ev[i], ev[i + 1]);
		ms3[0] = t[1]; ms3[1] = t[2]; ms3[2] = t[0];
		return 0;
	}
};

// Things borrowed for one call and handed back afterwards (T has a member `device`): the idle ones of every device, until
// j40hip_shutdown drains them
template <typename T> struct IdlePool {
	std::mutex m; std::vector<T> idle;
	bool take(int device, T *out) {
		std::lock_guard<std::mutex> lock(m);
		for (size_t i = 0; i < idle.size(); ++i) if (idle[i].device == device) { *out = idle[i]; idle.erase(idle.begin() + (long) i); return true; }
		return false;
	}
	void give(const T &t) { std::lock_guard<std::mutex> lock(m); idle.push_back(t); }
	template <typename F> void drain(F destroy) {
		std::vector<T> all;
		{ std::lock_guard<std::mutex> lock(m); all.swap(idle); }
		for (T &t : all) destroy(t);
	}
};

} // namespace j40hip_rt

struct j40hip_device_state {
	int device = 0;
	std::vector<DeviceBuffer> buffers;
	CacheBlock plan_block, work_block;                    // VarDCT frames: the uploaded plan and the working set (recycled, see cache_acquire)
	bool force_dense = false;                             // dense coefficient planes although the frame has one pass (after ERR_EVOF)
	size_t num_blocks = 0;                                // entries of plan.block_events / 4
	DevPlan plan;
	bool is_modular = false;
	int64_t first_group = 0, num_groups = 0;       // range decoded by this process
	std::vector<DevVarblock> vb_sorted;             // by DctSelect; host copy, fetched from the device on demand (host_vb_sorted)
	size_t vb_count = 0;
	int32_t class_start[28];
	DevVarblock *d_vb_sorted = nullptr;
	// sharded decode (j40hip_frame_set_group_range): the varblocks of the selected groups, same layout as vb_sorted
	DevVarblock *d_vb_range = nullptr; int32_t range_class_start[28]; size_t vb_range_capacity = 0;
	float *d_large_scratch = nullptr;
	// a frame with use_lf_frame (lf_frame_tail in runtime.hip): three planes of `lf_cells` floats its LfGroup tail runs through at every
	// decode, taken at upload; lf_max_cells: the cells of its largest LfGroup
	float *d_lf_frame = nullptr; size_t lf_cells = 0; int32_t lf_max_cells = 0;
	size_t coeff_floats = 0;
	int32_t total_sections = 0;
	HfLaunchInfo hf;
	// Modular frames
	DevModPlan mod;
	int32_t mod_sections = 0, mod_passes = 1, mod_sections_per_pass = 0;   // sections = LfGlobal's (0 or 1) + passes * per_pass
	bool mod_local_rcts = false;
	bool has_trailers = false;           // VarDCT frame whose sections go on with the extra channels' Modular sub-image
	bool idle = false;                   // j40hip_frame_mark_idle: nothing is pending on this frame's memory, freeing it needs no device-wide wait
	ModLaunchInfo mod_info = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
	std::vector<uint32_t> mod_section_offsets;
	// group: the group whose section's sub-image the op belongs to (mod_sub_ops; a ranged decode skips the ops of groups it did not decode), -1: the frame's
	struct ModOp { int kind; PlanePtr a, b, c, src, aux; size_t n; int32_t p0, p1, p2, p3, p4, p5; void *const *dst_list; const int8_t *wpp; int32_t group; };
	std::vector<ModOp> mod_ops;          // inverse transforms of the frame, in execution order
	std::vector<ModOp> mod_sub_ops;      // before them: inverse transforms of the sections' own sub-images and their paste (kind 3)
	std::vector<PlanePtr> final_planes;  // channel list after the inverse transforms (address + bytes per sample)
	bool mod_wide = false;               // a wide frame: every plane above holds int32 samples
	std::vector<int32_t> final_w, final_h;
	int32_t alpha_channel = -1;
	int32_t *pal_wp_scratch = nullptr;
	uint32_t *mod_extra_status = nullptr;
	std::vector<uint32_t> status_host;
	hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
	// the single-image path's two phases (decode_two_phase): the groups by decreasing section size, the `two_k` first of them decoded
	// beside the rest with their block_events entries in a table of their own; -1: not looked at yet, 0: not for this frame
	int32_t two_k = -1;
	uint32_t *d_two_order = nullptr, *d_two_shadow = nullptr;   // (one block of the device memory cache: two_block)
	CacheBlock two_block;
	std::vector<uint32_t> two_order;
	hipStream_t two_stream = nullptr; hipEvent_t two_ev[3] = {nullptr, nullptr, nullptr};
	// the plane stage (runtime.hip). d_xyb: the frame's three full-size float planes (X, Y, B; width floats a row), made at the first
	// decode that goes through planes (plane_buffer), kept with the frame
	float *d_xyb = nullptr;
	// the restoration filters (runtime.hip: restore_prepared, run_filters). restore: their parameters, the frame-wide sharpness map and
	// what keeps them from running, made at the first decode that asks for them, kept with the upload. The second set of planes, the
	// reciprocal sigmas and the map's copy are made at the first decode that runs them
	struct Restore { bool ready = false; RestoreParams p; uint32_t err = 0; std::vector<int16_t> sharp; } restore;
	float *d_xyb_tmp = nullptr, *d_sigma = nullptr; int16_t *d_sharp = nullptr;
	const float *d_restored = nullptr;   // where the last filtered planes lie (d_xyb or d_xyb_tmp)
	float restore_ms = 0;
	// the colour mode (j40hip_frame_set_colour; runtime.hip: colour_params). colour: the tail's parameters and, for an 8-bit frame, its
	// threshold table in device memory, made at the first decode that takes the tail, kept with the frame
	struct ColourTail { bool ready = false; ColourTailParams p; } colour;
	// a frame with patches (runtime.hip: apply_patches): the handle's records and tiles (j40hip_frame::patch_plan, made when the sequence's
	// index was built) copied into the frame's scratch at the upload; d_frame: a Modular frame's colour
	// constants as the sRGB tail takes them (a VarDCT frame's are its plan's)
	struct Patches { DevPatches dev = {nullptr, nullptr, nullptr, nullptr, 0, 0}; std::vector<DevFrame> host_frame; const DevFrame *d_frame = nullptr; } patch;
	// a frame with noise (runtime.hip: apply_noise): the three raw random planes (noise_pitch(width) floats a row) and the frame's four
	// jump sets, made at the first decode that adds noise, kept with the frame; ms: the two kernels' device time (J40HIP_NOISE_TIMING)
	struct Noise { float *d_raw = nullptr; const uint64_t *d_sets = nullptr; std::vector<uint64_t> host_sets; float ms[2] = {0, 0}; } noise;
	// an upsampled frame (runtime.hip: apply_upsampling): the three shown-size planes k_upsample writes and the tail reads
	// (3 * up_width * up_height floats) and the frame's expanded weight table (host_table: built once per upload, kept: the copy is
	// asynchronous), made at the first decode, kept with the frame; nothing for upsampling = 1. ms: the kernel's device time (J40HIP_UPSAMPLE_TIMING)
	// a frame with splines (runtime.hip: apply_splines): its segments and the CSR lists of the tiles they touch (Frame::spline_plan, which
	// outlives the copies), uploaded at the first decode that draws them, kept with the frame; ms: k_spline_draw's device time (J40HIP_SPLINE_TIMING)
	// d_patched: a frame with patches as well -- the planes as k_patch_blend left them, copied before the splines are drawn in place, for
	// j40hip_frame_read_xyb's stage 3 (made at the first such decode, kept with the frame)
	struct Splines { DevSplines dev = {nullptr, nullptr, nullptr, nullptr, 0, 0}; float *d_patched = nullptr; float ms = 0; } spline;
	struct Upsample { float *d_up = nullptr; const float *d_table = nullptr; std::vector<float> host_table; float ms = 0; } up;
	// a YCbCr frame (j40hip_frame_set_ycbcr; runtime.hip: ycbcr_pixels). ycbcr: the plan was built for one (the switch was on at upload).
	// d_ycc: the planes the pixel kernels leave for k_ycbcr_tail where the filters do not run, made at the first such decode, kept with
	// the frame. ycc_read: what the last decode's tail read (j40hip_frame_read_ycbcr) -- those planes, or the restoration filters' result
	bool ycbcr = false;
	float *d_ycc = nullptr;
	struct YccRead { const float *plane[3] = {nullptr, nullptr, nullptr}; int32_t pitch[3] = {0, 0, 0}, pw[3] = {0, 0, 0}, ph[3] = {0, 0, 0}; } ycc_read;
	// the LF preview (lf_preview.hip): the frame's LfGroups and LF integers as the preview kernel reads them -- the integers are the
	// plan's when it holds them (parsed with flags & 1), else in an allocation of their own (LF-only frames at upload, other frames at
	// their first preview); lfp_host is what was copied, kept with the frame because the copy is asynchronous
	DevLfpFrame lfp = {};
	bool lfp_ready = false;
	std::vector<uint8_t> lfp_host;

	// the kept alpha channel (j40hip_frame_set_alpha; keep_alpha below): the keep-mode trailer plan, the frame-wide planes of the extra
	// channels and the Modular decode's scratch in ONE block of the device memory cache, laid out at the first decode that keeps alpha
	// and used again by every later decode of the same group range (a stream's sections end where they ended before)
	struct AlphaKeep {
		CacheBlock block;
		bool ready = false; int64_t first_group = -1, num_groups = -1;
		DevModPlan plan; ModLaunchInfo info; int32_t num_sections = 0; bool local_rcts = false;
		const int16_t *alpha_plane = nullptr;
		std::vector<int32_t> section_of;                          // plan section -> the frame's section
		std::vector<std::pair<int32_t, uint32_t>> header_errors;  // sections whose sub-image header did not parse
		std::vector<uint8_t> staging;                             // what was copied into the block (the copy is asynchronous)
	} alpha;
	// region decode (j40hip_frame_set_region; decode_region below). The group-major index of d_vb_sorted, built on the device at the
	// first region decode of this upload (region_dev.h): seg_start, where every (group, class) segment of `index` starts, and on the
	// host only the segments' sizes. Per region: the cover's varblocks (list, class_start) and its groups (order), gathered on the
	// device when the cover changes. staging: the cover-sized image the pixel kernels write before the rectangle is cut out, one block
	// of the device memory cache, grown on demand, given back with the frame.
	struct Region {
		bool index_ready = false;
		uint32_t *d_cursor = nullptr, *d_seg_start = nullptr, *d_index = nullptr, *d_order = nullptr;
		std::vector<uint32_t> counts;                 // [num_groups * REGION_KEYS]
		DevVarblock *d_list = nullptr; size_t list_capacity = 0;
		int32_t class_start[REGION_KEYS]; RegionCover gathered = {0, 0, 0, 0, 0, 0};   // (what d_list and d_order hold: cols = 0, nothing)
		CacheBlock staging;
	} region;
	// reduced-size decode (j40hip_frame_set_scale; decode_scaled): the full-size image of the staged combinations (restoration filters,
	// keep-alpha), one block of the device memory cache, grown on demand, given back with the frame
	CacheBlock scale_staging;
	// oriented output (j40hip_frame_set_orientation; decode_oriented): the stored-order image k_orient reads, one block of the device
	// memory cache, grown on demand, given back with the frame
	CacheBlock orient_staging;
	// a batch decoded the frame (trailers_pending): where, for the merge at j40hip_frame_status
	void *pending_rgba = nullptr; size_t pending_stride = 0;

	template <typename T> T *upload(const T *src, size_t n, hipStream_t s, bool &ok) {
		DeviceBuffer b;
		if (!b.alloc(sizeof(T) * n)) { ok = false; return nullptr; }
		buffers.push_back(b);
		if (n && hipMemcpyAsync(b.ptr, src, sizeof(T) * n, hipMemcpyHostToDevice, s) != hipSuccess) ok = false;
		return (T *) b.ptr;
	}
	template <typename T> T *scratch(size_t n, bool &ok) {
		DeviceBuffer b;
		if (!b.alloc(sizeof(T) * n)) { ok = false; return nullptr; }
		buffers.push_back(b);
		return (T *) b.ptr;
	}
	// a buffer kept with the frame, made when first needed; false ("!mem"): there is none, and the pointer stays null
	template <typename T> bool keep(T *&p, size_t n) { bool ok = true; if (!p) p = scratch<T>(n, ok); return p != nullptr; }
};

namespace j40hip_rt {

// the frame's output format (j40hip_frame_set_output_format): 16-bit RGBA, 8 bytes a pixel, or the default u8x4
inline bool out16(const j40hip_frame *h) { return h->output_format == J40HIP_U16X4; }
inline OutMode out_mode(const j40hip_frame *h) { return out16(h) ? OutMode::RGBA16 : OutMode::RGBA8; }   // (the pixel kernels' form of it: K2Target)
inline size_t pixel_bytes(const j40hip_frame *h) { return out16(h) ? 8 : 4; }
// what the handle's next decode does (decode_route.hpp), with the upload's facts; `have_out`, `stride_bytes`: the caller's image
inline DecodeRoute route_of(const j40hip_frame *h, bool have_out = true, size_t stride_bytes = SIZE_MAX) {
	const j40hip_device_state *st = h->dev;
	const UploadFacts up = {st && st->is_modular, st && st->ycbcr, st && st->has_trailers, st ? st->first_group : 0, st ? st->num_groups : 0, st && st->is_modular && st->alpha_channel >= 0};
	return resolve_route(h, st ? &up : nullptr, have_out, stride_bytes);
}

// a Modular frame of an XYB image through the XYB colour tail (j40hip_frame_set_modular_xyb): what its kernels take -- LfGlobal's LF
// dequantisation and the colour constants as fill_frame_constants (plan_build.cpp) states them for DevFrame
inline ModXybConsts modular_xyb_consts(const Frame &fr) {
	ModXybConsts k;
	for (int c = 0; c < 3; ++c) { k.m[c] = fr.m_lf_scaled[c]; k.cc.opsin_bias[c] = fr.im.opsin_bias[c]; k.cc.cbrt_opsin_bias[c] = cbrtf(fr.im.opsin_bias[c]); }
	for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) k.cc.m[i * 3 + j] = fr.im.opsin_inv_mat[i][j];
	k.cc.itscale = 255.0f / fr.im.intensity_target; k.cc.bpp = fr.im.bpp;
	return k;
}

// what crosses units
bool host_vb_sorted(j40hip_device_state *st);                                  // runtime_upload.hip
uint32_t upload_lf_only(j40hip_frame *h, int device, hipStream_t s);           // runtime_lfp.hip
bool modular_groups_independent(const j40hip_frame *h);                        // runtime.hip
uint32_t clear_before_decode(j40hip_device_state *st, hipStream_t s);          // runtime.hip
uint32_t decode_frame_xyb(j40hip_frame *h, float *planes, hipStream_t s);      // runtime.hip
uint32_t apply_patches(j40hip_frame *h, float *planes, hipStream_t s);         // runtime.hip
uint32_t apply_splines(j40hip_frame *h, float *planes, hipStream_t s);         // runtime.hip
uint32_t apply_noise(j40hip_frame *h, float *planes, hipStream_t s);           // runtime.hip
uint32_t apply_upsampling(j40hip_frame *h, const float *planes, float **out, hipStream_t s);   // runtime.hip
uint32_t restore_params(const FrameHeader &fh, int mode, RestoreParams *p);    // runtime.hip
// A synchronous entry's wait behind a decode it has enqueued on `s`: the stream, then the frame's status. A section with more non-zero
// coefficients than its event region holds ("evof") has the frame uploaded again with dense planes, `decode` enqueues it once more, and
// that one's status is the answer.
template <typename F> uint32_t wait_with_dense_retry(j40hip_frame *h, int device, hipStream_t s, F decode) {
	for (int dense = 0;; ++dense) {
		if (hipStreamSynchronize(s) != hipSuccess) return ERR_GPU;
		uint32_t e = j40hip_frame_status(h);
		if (e != ERR_EVOF || dense) return e;
		h->force_dense = true;
		if ((e = j40hip_frame_upload(h, device)) != 0 || (e = decode()) != 0) return e;
	}
}
void lf_services_shutdown();   // runtime_lf.hip, runtime.hip, runtime_lfp.hip: j40hip_shutdown's steps
void two_phase_shutdown();
void lfp_args_shutdown();

} // namespace j40hip_rt
