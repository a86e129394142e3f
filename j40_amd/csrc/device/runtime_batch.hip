// j40_amd/csrc/device/runtime_batch.hip -- batches (throughput mode): many VarDCT frames behind one entropy launch
#include "runtime_state.hpp"

struct j40hip_batch {
	int device = 0;
	std::vector<j40hip_frame *> frames;
	DevPlan *d_plans = nullptr;
	std::vector<DevPlan> plans_host;   // what d_plans holds (batch_enqueue re-uploads it when a member was uploaded again)
	std::vector<HfLaneWork> work_host;
	size_t plans_cap = 0, work_cap = 0;
	bool arrays_dirty = true;          // plans_host / work_host have not been copied to the device yet
	int side_in_use = 0;               // side streams the current membership spreads its pixel kernels over
	HfLaneWork *d_work = nullptr;
	int32_t num_work = 0;
	bool tables_in_lds = true;
	uint32_t lds_bytes = 0;
	int32_t waves_per_wg = 1;
	bool lanes_fast = true;          // every frame qualifies for k_hf_lanes
	uint32_t lanes_lds_bytes = 0;
	hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
	std::vector<hipEvent_t> slots;   // 4 events per recorded decode (j40hip_batch_decode_recorded)
	// the pixel kernels of different frames are independent and individually too small to fill the GPU: they are spread
	// over a few side streams that fork after the entropy launch and join before anything else runs on the caller's stream
	std::vector<hipStream_t> side;
	std::vector<hipEvent_t> side_done;
	hipEvent_t fork = nullptr;
};

extern "C" void j40hip_batch_free(j40hip_batch *b) {
	if (!b) return;
	(void) hipSetDevice(b->device);
	if (b->d_plans) (void) hipFree(b->d_plans);
	if (b->d_work) (void) hipFree(b->d_work);
	for (auto &e : b->ev) if (e) (void) hipEventDestroy(e);
	for (auto &e : b->slots) if (e) (void) hipEventDestroy(e);
	for (auto &e : b->side_done) if (e) (void) hipEventDestroy(e);
	for (auto &st : b->side) if (st) (void) hipStreamDestroy(st);
	if (b->fork) (void) hipEventDestroy(b->fork);
	delete b;
}

// (Re)assigns the members of a batch: plans, the entropy kernel's work list and launch geometry. Device arrays are kept and only
// grown; their contents go up with the next decode (batch_enqueue), stream-ordered. The previous members' decodes must be complete.
static uint32_t batch_assign(j40hip_batch *b, j40hip_frame *const *frames, int64_t n) {
	if (n <= 0 || !frames) return ERR_RNGE;
	b->frames.clear(); b->plans_host.clear(); b->work_host.clear();
	b->tables_in_lds = true; b->lanes_fast = true; b->lanes_lds_bytes = 0; b->lds_bytes = 0;
	for (int64_t i = 0; i < n; ++i) {
		j40hip_frame *h = frames[i];
		if (h && h->frame.lf_only) return ERR_ULF;
		if (!h || !h->dev) return ERR_GPU;
		if (uint32_t e = mode_refusal(h, Mode::Batch)) return e;   // a batch writes whole frames in stored order
		if (h->dev->is_modular) return ERR_TODO;   // Modular frames: decode them one by one
		if (h->dev->ycbcr) return ERR_TODO;        // YCbCr frames (j40hip_frame_set_ycbcr): the single-frame decode alone serves them
		if (h->frame.fh.use_lf_frame) return ERR_TODO;   // a frame that takes its LF image from an LF frame: a sequence's playback alone serves it
		if (i == 0) b->device = h->dev->device;
		else if (h->dev->device != b->device) return ERR_RNGE;
		b->frames.push_back(h);
		b->plans_host.push_back(h->dev->plan);
		b->tables_in_lds = b->tables_in_lds && h->dev->hf.tables_fit_lds;
		b->lanes_fast = b->lanes_fast && h->dev->hf.lanes_fast;
		b->lanes_lds_bytes = std::max(b->lanes_lds_bytes, h->dev->hf.lanes_lds_bytes);
	}
	// Launch geometry of the entropy kernel. Sections per wavefront: 64 fills the lanes. Wavefronts per workgroup
	// share one copy of their frame's tables in LDS: with few wavefronts in the batch, one per workgroup spreads them
	// over the CUs; with many, sharing keeps the tables from capping the wavefronts a CU can hold.
	int32_t lanes = 64, total_waves = 0;
	lanes = env_int("J40HIP_LANES_PER_WAVE", lanes, 1, 64);
	for (j40hip_frame *h : b->frames) total_waves += (h->frame.fh.num_groups + lanes - 1) / lanes;
	static int cus_of[16];   // (hipGetDeviceProperties takes milliseconds)
	if (b->device >= 0 && b->device < 16 && !cus_of[b->device]) { hipDeviceProp_t prop; cus_of[b->device] = hipGetDeviceProperties(&prop, b->device) == hipSuccess && prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256; }
	const int cus = b->device >= 0 && b->device < 16 ? cus_of[b->device] : 256;
	b->waves_per_wg = total_waves <= 2 * cus ? 1 : total_waves <= 4 * cus ? 2 : 4;
	b->waves_per_wg = j40hip_rt::waves_per_wg(b->waves_per_wg, 4);
	std::vector<HfLaneWork> &work = b->work_host;
	for (size_t i = 0; i < b->frames.size(); ++i) {
		const int32_t groups = b->frames[i]->frame.fh.num_groups;
		for (int32_t g = 0; g < groups; g += lanes) work.push_back({(int32_t) i, g, std::min(lanes, groups - g), 0});
		while (work.size() % (size_t) b->waves_per_wg) work.push_back({(int32_t) i, 0, 0, 0});   // a workgroup stays on one frame
	}
	for (j40hip_frame *h : b->frames) {
		HfLaunchInfo info = h->dev->hf; info.tables_fit_lds = b->tables_in_lds;
		b->lds_bytes = std::max(b->lds_bytes, hf_lanes_lds_bytes(info));
	}
	b->num_work = (int32_t) work.size();
	if (hipSetDevice(b->device) != hipSuccess) return ERR_GPU;
	if (b->plans_host.size() > b->plans_cap) {
		if (b->d_plans) (void) hipFree(b->d_plans);
		b->plans_cap = b->plans_host.size() + b->plans_host.size() / 2;
		if (hipMalloc((void **) &b->d_plans, sizeof(DevPlan) * b->plans_cap) != hipSuccess) { b->d_plans = nullptr; b->plans_cap = 0; return ERR_GPU; }
	}
	if (work.size() > b->work_cap) {
		if (b->d_work) (void) hipFree(b->d_work);
		b->work_cap = work.size() + work.size() / 2;
		if (hipMalloc((void **) &b->d_work, sizeof(HfLaneWork) * b->work_cap) != hipSuccess) { b->d_work = nullptr; b->work_cap = 0; return ERR_GPU; }
	}
	b->arrays_dirty = true;
	// side streams for the pixel kernels: made once, as many as the largest membership so far asks for
	{
		int nside = (int) std::min<size_t>(16, b->frames.size());
		nside = env_int("J40HIP_SIDE_STREAMS", nside, 0, 32);
		if (nside < 2) nside = 0;
		while ((int) b->side.size() < nside) {
			hipStream_t st = nullptr; hipEvent_t ev = nullptr;
			if (hipStreamCreateWithFlags(&st, hipStreamNonBlocking) != hipSuccess || hipEventCreateWithFlags(&ev, hipEventDisableTiming) != hipSuccess) return ERR_GPU;
			b->side.push_back(st); b->side_done.push_back(ev);
		}
		b->side_in_use = nside;
		if (!b->fork && hipEventCreateWithFlags(&b->fork, hipEventDisableTiming) != hipSuccess) return ERR_GPU;
	}
	for (auto &e : b->ev) if (!e && hipEventCreate(&e) != hipSuccess) return ERR_GPU;
	return 0;
}

static j40hip_batch *batch_create_body(j40hip_frame *const *frames, int64_t n, uint32_t *err) {
	uint32_t dummy; if (!err) err = &dummy;
	j40hip_batch *b = new j40hip_batch();
	*err = batch_assign(b, frames, n);
	if (*err) { j40hip_batch_free(b); return nullptr; }
	return b;
}
extern "C" uint32_t j40hip_batch_reset(j40hip_batch *b, j40hip_frame *const *frames, int64_t n) {
	if (!b) return ERR_GPU;
	return guarded([&] { return batch_assign(b, frames, n); });
}

// ev: four events to record around the three stages (clear | entropy | pixels), or nullptr
static uint32_t batch_enqueue(j40hip_batch *b, void *const *rgba_dev, const size_t *stride_bytes, hipStream_t s, hipEvent_t *ev) {
	if (!b) return ERR_GPU;
	// every member in one output format (mixed batches: "Uof?"), each 16-bit member's rows wide enough: checked before anything is launched
	for (size_t i = 0; i < b->frames.size(); ++i) {
		const DecodeRoute route = route_of(b->frames[i]);
		if (b->frames[i]->output_format != b->frames[0]->output_format) return ERR4('U', 'o', 'f', '?');
		// ... and at one scale shift ("Usc?"); a keep-alpha member's alpha is merged into full-size pixels when its status is read: not at a scale
		if (b->frames[i]->scale != b->frames[0]->scale) return ERR_USC;
		if (route.shape == DecodeRoute::Scaled && route.alpha_merged) return ERR_USC;
		if (stride_bytes[i] < route.min_stride) return ERR_RNGE;
	}
	if (hipSetDevice(b->device) != hipSuccess) return ERR_GPU;
	// a member that was uploaded again since the batch was made (j40hip_frame_force_dense + j40hip_frame_upload after "evof")
	// has a new plan in new blocks: the array the entropy kernel reads is brought up to date, stream-ordered behind the
	// launches of an earlier decode that may still be reading it. A member without device state fails the batch.
	{
		bool changed = false;
		for (size_t i = 0; i < b->frames.size(); ++i) {
			j40hip_device_state *st = b->frames[i]->dev;
			if (!st || st->is_modular || st->device != b->device) return ERR_GPU;
			if (memcmp(&b->plans_host[i], &st->plan, sizeof(DevPlan)) != 0) { b->plans_host[i] = st->plan; changed = true; }
		}
		if (changed || b->arrays_dirty) {
			// (pageable sources: the runtime copies them out before the calls return; the vectors live until the next reset anyway)
			if (hipMemcpyAsync(b->d_plans, b->plans_host.data(), sizeof(DevPlan) * b->plans_host.size(), hipMemcpyHostToDevice, s) != hipSuccess) return ERR_GPU;
			if (b->arrays_dirty && hipMemcpyAsync(b->d_work, b->work_host.data(), sizeof(HfLaneWork) * b->work_host.size(), hipMemcpyHostToDevice, s) != hipSuccess) return ERR_GPU;
			b->arrays_dirty = false;
		}
	}
	const StageMarks marks{ev, s};
	marks.mark(0);
	for (size_t i = 0; i < b->frames.size(); ++i) {
		j40hip_frame *h = b->frames[i];
		j40hip_device_state *st = h->dev;
		h->last.trailers_pending = st->has_trailers;
		st->pending_rgba = h->scale > 0 ? nullptr : rgba_dev[i]; st->pending_stride = stride_bytes[i]; h->last.alpha_written = false;   // (a kept alpha is merged when the status is read -- never into a small image: the sub-images are validated all the same)
		if (uint32_t e = clear_before_decode(st, s)) return e;
		// (no need to clear the status words: a batch decodes every section of every frame and the entropy kernels store
		// each section's status unconditionally -- 256 tiny fills were 4 % of a step)
	}
	marks.mark(1);
	if (b->lanes_fast && !j40hip_rt::generic_lanes()) launch_hf_lanes(b->d_plans, b->d_work, b->num_work, b->waves_per_wg, b->lanes_lds_bytes, s);
	else launch_hf_entropy_lanes(b->d_plans, b->d_work, b->num_work, b->tables_in_lds, b->lds_bytes, s);
	marks.mark(2);
	if (b->side_in_use == 0) {
		for (size_t i = 0; i < b->frames.size(); ++i) {
			j40hip_device_state *st = b->frames[i]->dev;
			launch_vardct_frame(st->plan, st->class_start, st->d_vb_sorted, st->d_large_scratch, K2Target{rgba_dev[i], stride_bytes[i], out_mode(b->frames[i]), b->frames[i]->scale}, s);
		}
	} else {
		if (hipEventRecord(b->fork, s) != hipSuccess) return ERR_GPU;
		for (int k = 0; k < b->side_in_use; ++k) if (hipStreamWaitEvent(b->side[(size_t) k], b->fork, 0) != hipSuccess) return ERR_GPU;
		for (size_t i = 0; i < b->frames.size(); ++i) {
			j40hip_device_state *st = b->frames[i]->dev;
			launch_vardct_frame(st->plan, st->class_start, st->d_vb_sorted, st->d_large_scratch, K2Target{rgba_dev[i], stride_bytes[i], out_mode(b->frames[i]), b->frames[i]->scale}, b->side[i % (size_t) b->side_in_use]);
		}
		for (size_t k = 0; k < (size_t) b->side_in_use; ++k) {
			if (hipEventRecord(b->side_done[k], b->side[k]) != hipSuccess || hipStreamWaitEvent(s, b->side_done[k], 0) != hipSuccess) return ERR_GPU;
		}
	}
	marks.mark(3);
	return hipGetLastError() == hipSuccess ? 0 : ERR_GPU;
}

static uint32_t batch_decode_impl(j40hip_batch *b, void *const *rgba_dev, const size_t *stride_bytes, hipStream_t s, float *ms3) {
	if (!b) return ERR_GPU;
	if (uint32_t e = batch_enqueue(b, rgba_dev, stride_bytes, s, ms3 ? b->ev : nullptr)) return e;
	return StageMarks{ms3 ? b->ev : nullptr, s}.finish(ms3);
}

// asynchronous variant of the timed decode: records the stage events in `slot` and returns; the caller reads them
// with j40hip_batch_elapsed once the stream has been synchronised (keeps several batches in flight on different
// streams while still measuring every launch)
extern "C" uint32_t j40hip_batch_decode_recorded(j40hip_batch *b, void *const *rgba_dev, const size_t *stride_bytes, void *stream, int32_t slot) {
	if (!b || slot < 0 || slot >= 4096) return ERR_RNGE;
	if (hipSetDevice(b->device) != hipSuccess) return ERR_GPU;
	while (b->slots.size() < 4 * ((size_t) slot + 1)) { hipEvent_t e = nullptr; if (hipEventCreate(&e) != hipSuccess) return ERR_GPU; b->slots.push_back(e); }
	return guarded([&] { return batch_enqueue(b, rgba_dev, stride_bytes, (hipStream_t) stream, b->slots.data() + 4 * (size_t) slot); });
}
// makes `stream` wait until stage `stage` (1: cleared, 2: entropy decoded, 3: pixels written) of the decode recorded in
// `slot` has completed; used to stagger batches on different streams
extern "C" uint32_t j40hip_batch_wait_stage(j40hip_batch *b, int32_t slot, int32_t stage, void *stream) {
	if (!b || slot < 0 || stage < 0 || stage > 3 || b->slots.size() < 4 * ((size_t) slot + 1)) return ERR_RNGE;
	return hipStreamWaitEvent((hipStream_t) stream, b->slots[4 * (size_t) slot + (size_t) stage], 0) == hipSuccess ? 0 : ERR_GPU;
}
extern "C" uint32_t j40hip_batch_elapsed(j40hip_batch *b, int32_t slot, float *ms3) {
	if (!b || slot < 0 || b->slots.size() < 4 * ((size_t) slot + 1)) return ERR_RNGE;
	return StageMarks{b->slots.data() + 4 * (size_t) slot, nullptr}.finish(ms3);
}

extern "C" uint32_t j40hip_batch_decode(j40hip_batch *b, void *const *rgba_dev, const size_t *stride_bytes, void *stream) {
	return guarded([&] { return batch_decode_impl(b, rgba_dev, stride_bytes, (hipStream_t) stream, nullptr); });
}
extern "C" uint32_t j40hip_batch_decode_timed(j40hip_batch *b, void *const *rgba_dev, const size_t *stride_bytes, void *stream, float *ms3) {
	return guarded([&] { return batch_decode_impl(b, rgba_dev, stride_bytes, (hipStream_t) stream, ms3); });
}
extern "C" j40hip_batch *j40hip_batch_create(j40hip_frame *const *frames, int64_t n, uint32_t *err) {
	try { return batch_create_body(frames, n, err); } catch (const std::exception &) { if (err) *err = ERR_MEM; return nullptr; }
}
