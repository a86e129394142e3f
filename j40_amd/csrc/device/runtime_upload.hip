// j40_amd/csrc/device/runtime_upload.hip -- a frame's plan into HBM: j40hip_frame_upload for Modular and VarDCT frames, the group
// range of a sharded decode, j40hip_release_device
#include "runtime_state.hpp"

extern "C" void j40hip_release_device(j40hip_frame *f) {
	if (!f || !f->dev) return;
	(void) hipSetDevice(f->dev->device);
	bool idle = f->dev->idle;   // else one device-wide wait, ahead of the first block that goes back: nothing may still be running on memory that is handed to another frame
	for (CacheBlock *b : {&f->dev->plan_block, &f->dev->work_block, &f->dev->two_block, &f->dev->alpha.block, &f->dev->region.staging, &f->dev->scale_staging, &f->dev->orient_staging}) if (b->ptr) { b->release(idle); idle = true; }
	for (auto &b : f->dev->buffers) b.release();
	for (auto &e : f->dev->ev) if (e) (void) hipEventDestroy(e);
	delete f->dev;
	f->dev = nullptr;
	f->last.device_released();
}

extern "C" int j40hip_device_count(void) {
	int n = 0;
	if (hipGetDeviceCount(&n) != hipSuccess) return 0;
	return n;
}

static uint32_t upload_modular(j40hip_frame *h, int device) {
	HostModPlan hp;
	if (uint32_t e = build_modular_plan(h->frame, h->cs, h->cs_size, &hp)) return e;
	j40hip_device_state *st = new j40hip_device_state();
	h->dev = st; st->device = device; st->is_modular = true;
	st->first_group = 0; st->num_groups = h->frame.fh.num_groups;   // (j40hip_frame_set_group_range narrows it)
	hipStream_t s = nullptr;
	bool ok = true;
	// the plan's tables, the coded channels' planes, the sub-images' planes and the scratch: one allocation, laid out by ModPlanLayout
	// (a squeezed 16384 x 16384 frame has 70+ planes); the codestream beside it
	const ModPlanLayout lay(hp, 0);
	uint8_t *base = st->scratch<uint8_t>(lay.total_bytes, ok);
	if (!ok) { j40hip_release_device(h); return ERR_GPU; }
	std::vector<uint8_t> staging(lay.upload_bytes);   // (lives until the stream is synchronised below)
	lay.stage(hp, staging.data(), base);
	if (hipMemcpyAsync(base, staging.data(), lay.upload_bytes, hipMemcpyHostToDevice, s) != hipSuccess) ok = false;
	const DevModPlan &plan = st->mod = lay.bind(base, st->upload(hp.codestream.data(), hp.codestream.size(), s, ok));
	st->mod_local_rcts = !hp.local_rct.empty();
	st->mod_sections = (int32_t) hp.sections.size(); st->mod_passes = hp.num_passes; st->mod_sections_per_pass = hp.sections_per_pass;
	st->mod_info = mod_launch_info(hp);
	st->mod_wide = hp.frame.sample_bytes == 4;
	const int32_t sb = (int32_t) lay.sample_bytes;   // bytes a sample takes; every offset below is counted in samples (PlanePtr::at)
	auto new_plane = [&](size_t samples) { return PlanePtr{st->scratch<uint8_t>((size_t) sb * samples, ok), sb}; };
	for (const DevModSection &sec : hp.sections) st->mod_section_offsets.push_back(sec.byte_off);
	struct Ref { PlanePtr p; int32_t w, h; };
	std::vector<Ref> planes;
	for (size_t c = 0; c < lay.num_planes; ++c) planes.push_back({lay.plane_ptr(base, c), hp.plane_w[c], hp.plane_h[c]});
	bool palette_wp = false;
	for (const Transform &t : hp.transforms) palette_wp |= t.kind == Transform::PALETTE && t.nb_deltas > 0 && t.d_pred == 6;
	if (palette_wp) st->pal_wp_scratch = st->scratch<int32_t>((size_t) (sb / 2) * ((size_t) 2 * (size_t) hp.frame.width * 5 + 16), ok);   // (64-bit cells in a wide frame)
	st->mod_extra_status = const_cast<uint32_t *>(plan.status) + hp.sections.size();
	st->total_sections = (int32_t) hp.sections.size();

	// inverse transforms, last to first (j40.h:4513-4521), resolved to plane pointers now: of the frame, and before that of the
	// sub-images of the sections that list a palette of their own (undone there, then pasted over the section's rectangle)
	static const uint8_t PERM[6][3] = {{0, 1, 2}, {1, 2, 0}, {2, 0, 1}, {0, 2, 1}, {1, 0, 2}, {2, 1, 0}};
	auto schedule = [&](std::vector<Ref> &planes, const std::vector<Transform> &trs, const int8_t *wpb, std::vector<j40hip_device_state::ModOp> &ops, int32_t group) {
		const size_t ops_before = ops.size();
		for (size_t ti = trs.size(); ti-- > 0; ) {
			const Transform &t = trs[ti];
			if (t.kind == Transform::RCT) {
				j40hip_device_state::ModOp op; memset(&op, 0, sizeof op);
				Ref c[3] = {planes[(size_t) t.begin_c], planes[(size_t) t.begin_c + 1], planes[(size_t) t.begin_c + 2]};
				op.kind = 0; op.a = c[0].p; op.b = c[1].p; op.c = c[2].p; op.n = (size_t) c[0].w * (size_t) c[0].h; op.p0 = t.rct_type % 7;
				ops.push_back(op);
				for (int i = 0; i < 3; ++i) planes[(size_t) (t.begin_c + PERM[t.rct_type / 7][i])] = c[i];
			} else if (t.kind == Transform::PALETTE) {
				const int32_t first = t.begin_c + 1;
				const Ref idx = planes[(size_t) first], pal = planes[0];
				const size_t n = (size_t) idx.w * (size_t) idx.h;
				std::vector<Ref> outs;
				for (int32_t i = 0; i < t.num_c - 1; ++i) outs.push_back({new_plane(n ? n : 1), idx.w, idx.h});
				outs.push_back(idx);   // the index channel becomes the last colour channel, in place
				if (t.nb_deltas > 0) {
					std::vector<void *> ptrs; for (const Ref &o : outs) ptrs.push_back(o.p.p);
					j40hip_device_state::ModOp op; memset(&op, 0, sizeof op);
					op.kind = 2; op.src = idx.p; op.aux = pal.p; op.p0 = pal.w; op.p1 = t.num_c; op.p2 = idx.w; op.p3 = idx.h; op.p4 = t.nb_colours; op.p5 = t.nb_deltas | (t.d_pred << 24);
					op.dst_list = st->upload(ptrs.data(), ptrs.size(), s, ok);
					op.wpp = st->upload(wpb, 12, s, ok);
					ops.push_back(op);
				} else {
					for (int32_t i = 0; i < t.num_c; ++i) {
						j40hip_device_state::ModOp op; memset(&op, 0, sizeof op);
						op.kind = 1; op.src = idx.p; op.aux = t.nb_colours > 0 ? pal.p.at((size_t) i * (size_t) pal.w) : PlanePtr{nullptr, sb}; op.a = outs[(size_t) i].p; op.n = n; op.p0 = i; op.p1 = t.nb_colours;
						ops.push_back(op);
					}
				}
				std::vector<Ref> next(planes.begin() + 1, planes.begin() + first);
				next.insert(next.end(), outs.begin(), outs.end());
				next.insert(next.end(), planes.begin() + first + 1, planes.end());
				planes.swap(next);
			} else if (t.kind == Transform::SQUEEZE) {
				// one step: every squeezed channel and its residual channel are joined into a new plane (the recurrence runs along
				// the squeezed axis, so it is not done in place); the residual channels then leave the list
				const int32_t nc = (int32_t) planes.size(), end_c = t.begin_c + t.num_c, offset = t.in_place ? end_c : nc - t.num_c;
				if (t.begin_c < 0 || t.num_c < 1 || end_c > nc || offset + t.num_c > nc || offset < end_c) { ok = false; break; }
				for (int32_t c = t.begin_c; c < end_c; ++c) {
					const Ref avg = planes[(size_t) c], res = planes[(size_t) (offset + c - t.begin_c)];
					Ref out = {PlanePtr{nullptr, sb}, t.horizontal ? avg.w + res.w : avg.w, t.horizontal ? avg.h : avg.h + res.h};
					if ((t.horizontal ? res.h != avg.h || (res.w != avg.w && res.w != avg.w - 1) : res.w != avg.w || (res.h != avg.h && res.h != avg.h - 1))) { ok = false; break; }
					const size_t n = (size_t) std::max(out.w, 0) * (size_t) std::max(out.h, 0);
					out.p = new_plane(n ? n : 1);
					j40hip_device_state::ModOp op; memset(&op, 0, sizeof op);
					op.kind = 4; op.src = avg.p; op.aux = res.p; op.a = out.p; op.p0 = avg.w; op.p1 = avg.h; op.p2 = res.w; op.p3 = res.h; op.p4 = t.horizontal ? 1 : 0;
					ops.push_back(op);
					planes[(size_t) c] = out;
				}
				if (ok) planes.erase(planes.begin() + offset, planes.begin() + offset + t.num_c);
			} else { ok = false; }
		}
		for (size_t k = ops_before; k < ops.size(); ++k) ops[k].group = group;
	};
	if (!hp.sub_images.empty()) {
		int32_t widest = hp.frame.width;
		for (size_t k = 0; k < lay.num_subs; ++k) widest = std::max(widest, hp.sub_w[k]);
		for (const HostModPlan::SubImage &si : hp.sub_images) {
			if (!si.paste) continue;
			for (const Transform &t : si.transforms) palette_wp |= t.kind == Transform::PALETTE && t.nb_deltas > 0 && t.d_pred == 6;
			std::vector<Ref> sp;
			for (size_t k = (size_t) si.first_plane; k < (size_t) (si.first_plane + si.num_planes); ++k) sp.push_back({lay.sub_plane_ptr(base, k), hp.sub_w[k], hp.sub_h[k]});
			// (sections: LfGlobal's first, then passes x groups)
			const int32_t lead_sections = (int32_t) hp.sections.size() - hp.sections_per_pass * hp.num_passes;
			const int32_t sub_group = si.section >= lead_sections && hp.sections_per_pass > 0 ? (si.section - lead_sections) % hp.sections_per_pass : -1;
			schedule(sp, si.transforms, si.wp, st->mod_sub_ops, sub_group);
			const DevModSection &sec = hp.sections[(size_t) si.section];
			for (size_t c = 0; c < sp.size() && ok; ++c) {   // paste: rows of the sub-image over the section's rectangle
				const Ref &dst = planes[(size_t) sec.first_channel + c];
				if (sp[c].w != sec.gw || sp[c].h != sec.gh || (size_t) sec.first_channel + c >= planes.size()) { ok = false; break; }
				j40hip_device_state::ModOp op; memset(&op, 0, sizeof op);
				op.kind = 3; op.src = sp[c].p; op.a = dst.p.at((size_t) sec.gy * (size_t) dst.w + (size_t) sec.gx); op.p0 = sp[c].w; op.p1 = sp[c].h; op.p2 = dst.w; op.group = sub_group;
				st->mod_sub_ops.push_back(op);
			}
		}
		if (palette_wp && !st->pal_wp_scratch) st->pal_wp_scratch = st->scratch<int32_t>((size_t) (sb / 2) * ((size_t) 2 * (size_t) widest * 5 + 16), ok);
	}
	{
		int8_t gwp[12]; const WPParams &wp = h->frame.gmodular.wp;
		gwp[0] = wp.p1; gwp[1] = wp.p2; for (int i = 0; i < 5; ++i) gwp[2 + i] = wp.p3[i]; for (int i = 0; i < 4; ++i) gwp[7 + i] = wp.w[i]; gwp[11] = 0;
		schedule(planes, hp.transforms, gwp, st->mod_ops, -1);
	}
	for (const Ref &p : planes) { st->final_planes.push_back(p.p); st->final_w.push_back(p.w); st->final_h.push_back(p.h); }
	st->alpha_channel = hp.alpha_channel;
	// the renderer needs three full-size colour planes (j40.h:7923)
	bool renderable = planes.size() >= 3;
	for (size_t c = 0; renderable && c < 3; ++c) renderable = planes[c].w == hp.frame.width && planes[c].h == hp.frame.height;
	if (st->alpha_channel >= 0) renderable = renderable && (size_t) st->alpha_channel < planes.size() && planes[(size_t) st->alpha_channel].w == hp.frame.width && planes[(size_t) st->alpha_channel].h == hp.frame.height;
	for (auto &e : st->ev) if (hipEventCreate(&e) != hipSuccess) ok = false;
	if (hipStreamSynchronize(s) != hipSuccess) ok = false;
	if (!ok) { j40hip_release_device(h); return ERR_GPU; }
	if (!renderable) { j40hip_release_device(h); return ERR_TODO; }
	return 0;
}
// the frame's varblock list on the host (sharded decodes, stage dumps): copied back from the device when first asked for
bool j40hip_rt::host_vb_sorted(j40hip_device_state *st) {
	if (st->vb_sorted.size() == st->vb_count) return true;
	st->vb_sorted.resize(st->vb_count);
	if (hipSetDevice(st->device) != hipSuccess || hipMemcpy(st->vb_sorted.data(), st->d_vb_sorted, sizeof(DevVarblock) * st->vb_count, hipMemcpyDeviceToHost) != hipSuccess) { st->vb_sorted.clear(); return false; }
	return true;
}

// A frame with patches: its records and their tiles, as the sequence's index made them (j40hip_frame::patch_plan, which outlives the
// copies), into the frame's scratch; a Modular frame's colour constants for the sRGB tail beside them (a Modular frame with noise takes
// that tail too, and an upsampled one). Waits for the copies.
static uint32_t upload_patches(j40hip_frame *h, hipStream_t s) {
	if (!h->frame.fh.has_patches && !((h->frame.fh.has_splines || h->frame.fh.has_noise || h->frame.fh.upsampling > 1) && h->dev->is_modular)) return 0;
	j40hip_device_state *st = h->dev;
	j40hip_device_state::Patches &pt = st->patch;
	if (h->frame.fh.has_patches && !h->patch_plan) { j40hip_release_device(h); return ERR_TODO; }   // (cannot happen: only a sequence's handle parses a dictionary)
	static const PatchPlan no_plan;
	const PatchPlan &plan = h->frame.fh.has_patches ? *h->patch_plan : no_plan;
	bool ok = true;
	if (!plan.bins.tile_ids.empty()) {
		pt.dev.recs = st->upload(plan.recs.data(), plan.recs.size(), s, ok);
		pt.dev.tile_ids = st->upload(plan.bins.tile_ids.data(), plan.bins.tile_ids.size(), s, ok);
		pt.dev.offsets = st->upload(plan.bins.offsets.data(), plan.bins.offsets.size(), s, ok);
		pt.dev.index = st->upload(plan.bins.index.data(), plan.bins.index.size(), s, ok);
		pt.dev.num_tiles = (int32_t) plan.bins.tile_ids.size(); pt.dev.tiles_x = plan.bins.tiles_x;
	}
	if (st->is_modular) { pt.host_frame.assign(1, DevFrame()); fill_frame_constants(h->frame, pt.host_frame.data()); pt.d_frame = st->upload(pt.host_frame.data(), 1, s, ok); }
	if (hipStreamSynchronize(s) != hipSuccess) ok = false;
	if (!ok) { j40hip_release_device(h); return ERR_GPU; }
	return 0;
}

// `s`: the stream the copies and fills are enqueued on; the call returns once they have completed (the plan is staged in the
// calling thread's pinned buffer, which the next upload of this thread reuses)
static uint32_t upload_impl(j40hip_frame *h, int device, hipStream_t s) {
	if (!h) return ERR_GPU;
	if (h->dev) j40hip_release_device(h);
	h->partial_range = false;   // (an upload decodes every group again)
	if (j40hip_device_count() <= device || hipSetDevice(device) != hipSuccess) return ERR_GPU;
	if (h->frame.lf_only) return upload_lf_only(h, device, s);
	// (a frame the Modular XYB switch may be put in force for: its colour tail reads the sRGB thresholds, which a Modular upload never needed --
	// taken here, once per device, so that the decode entry points stay asynchronous)
	if (h->frame.fh.is_modular && j40hip_modular_xyb_applies(h) && !ensure_constant_tables(device)) return ERR_GPU;
	if (h->frame.fh.is_modular) { const uint32_t e = upload_modular(h, device); return e ? e : upload_patches(h, s); }
	HostPlan &hp = t_host_plan;   // (this thread's, storage kept from frame to frame)
	hp.reset();
	hp.force_dense = h->force_dense;
	const bool timing = api_timing();   // (where an upload's time goes: plan build, staging, copy + LfGroup tail)
	auto now = [] { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
	const double tu0 = timing ? now() : 0;
	if (uint32_t e = build_vardct_plan(h->frame, h->cs, h->cs_size, &hp, h->threads, j40hip_ycbcr_on(h))) return e;
	const double tu1 = timing ? now() : 0;

	j40hip_device_state *st = new j40hip_device_state();
	h->dev = st; st->device = device; st->force_dense = h->force_dense;
	st->ycbcr = h->frame.fh.do_ycbcr;   // (a plan exists: the switch was on)
	bool ok = ensure_constant_tables(device);
	DevPlan &plan = st->plan;
	memset(&plan, 0, sizeof plan);
	st->hf = hp.hf;
	st->vb_count = hp.vb_sorted.size();   // (the list itself stays on the device: host_vb_sorted fetches it for the rare callers)
	memcpy(st->class_start, hp.class_start, sizeof st->class_start);
	Stager sg;
	sg.deferred = h->threads > 1;
	const size_t o_cs = sg.put(hp.codestream.data(), hp.codestream.size()), o_u8 = sg.put(hp.pool_u8.data(), hp.pool_u8.size());
	const size_t o_u16 = sg.put(hp.pool_u16.data(), hp.pool_u16.size()), o_i32 = sg.put(hp.pool_i32.data(), hp.pool_i32.size());
	const size_t o_u64 = sg.put(hp.pool_u64.data(), hp.pool_u64.size()), o_f32 = sg.put(hp.pool_f32.data(), hp.pool_f32.size());
	const size_t o_cl = sg.put(hp.clusters.data(), hp.clusters.size()), o_spec = sg.put(hp.coeff_specs.data(), hp.coeff_specs.size());
	const size_t o_lfg = sg.put(hp.lf_groups.data(), hp.lf_groups.size()), o_sec = sg.put(hp.sections.data(), hp.sections.size());
	const size_t o_gb = sg.put(hp.group_blocks.data(), hp.group_blocks.size()), o_gbs = sg.put(hp.group_block_start.data(), hp.group_block_start.size());
	const size_t o_frame = sg.put(&hp.frame, 1), o_blocks = sg.put(hp.blocks.data(), hp.blocks.size()), o_lfi = sg.put(hp.lfindices.data(), hp.lfindices.size());
	const size_t cells = hp.blocks.size();
	size_t o_llf[3], o_raw[3] = {0, 0, 0};
	if (hp.lf_tail_pending) {   // the LLF arrays are an output of the device's LfGroup tail: only their place is reserved
		for (int c = 0; c < 3; ++c) { o_raw[c] = sg.put(hp.lfraw[c].data(), hp.lfraw[c].size()); o_llf[c] = 0; }   // (reserved behind everything that is copied, below)
	} else for (int c = 0; c < 3; ++c) o_llf[c] = sg.put(hp.llf[c].data(), hp.llf[c].size());
	const size_t o_vbc = sg.put(hp.vb_coeffoff_qfidx.data(), hp.vb_coeffoff_qfidx.size()), o_vbh = sg.put(hp.vb_hfmul_inv.data(), hp.vb_hfmul_inv.size());
	const size_t o_xfy = sg.put(hp.xfromy.data(), hp.xfromy.size()), o_bfy = sg.put(hp.bfromy.data(), hp.bfromy.size());
	const size_t o_vbs = sg.put(hp.vb_sorted.data(), hp.vb_sorted.size());
	const size_t o_evr = sg.put(hp.ev_range.data(), hp.ev_range.size());
	const size_t copy_bytes = sg.size;
	if (hp.lf_tail_pending) for (int c = 0; c < 3; ++c) o_llf[c] = sg.reserve(sizeof(float) * cells);
	if (!sg.ok) ok = false;
	sg.flush(h->threads);
	const double tu2 = timing ? now() : 0;
	uint8_t *pb = ok && st->plan_block.ensure(device, sg.size, true) ? (uint8_t *) st->plan_block.ptr : nullptr;
	if (!pb || hipMemcpyAsync(pb, sg.data(), copy_bytes, hipMemcpyHostToDevice, s) != hipSuccess) ok = false;
	plan.codestream = pb + o_cs; plan.pool_u8 = pb + o_u8; plan.pool_u16 = (const uint16_t *) (pb + o_u16); plan.pool_i32 = (const int32_t *) (pb + o_i32);
	plan.pool_u64 = (const uint64_t *) (pb + o_u64); plan.pool_f32 = (const float *) (pb + o_f32); plan.clusters = (const DevCluster *) (pb + o_cl);
	plan.coeff_specs = (const DevCodeSpec *) (pb + o_spec); plan.lf_groups = (const DevLfGroup *) (pb + o_lfg); plan.sections = (const DevSection *) (pb + o_sec);
	plan.group_blocks = (const DevGroupBlock *) (pb + o_gb); plan.group_block_start = (const uint32_t *) (pb + o_gbs); plan.frame = (const DevFrame *) (pb + o_frame);
	plan.block_ctx_map_off = hp.block_ctx_map_off;
	plan.blocks = (const int32_t *) (pb + o_blocks); plan.lfindices = pb + o_lfi;
	for (int c = 0; c < 3; ++c) { plan.llf[c] = (const float *) (pb + o_llf[c]); plan.lfraw[c] = hp.lf_tail_pending ? (const int16_t *) (pb + o_raw[c]) : nullptr; }
	plan.vb_coeffoff_qfidx = (const int32_t *) (pb + o_vbc); plan.vb_hfmul_inv = (const float *) (pb + o_vbh);
	plan.xfromy = (const int16_t *) (pb + o_xfy); plan.bfromy = (const int16_t *) (pb + o_bfy);
	st->d_vb_sorted = (DevVarblock *) (pb + o_vbs);
	plan.ev_range = (const uint32_t *) (pb + o_evr);
	// working set: the coefficients -- event lists plus the per-block table (single-pass frames) or three dense planes in one
	// allocation (multi-pass frames; hf_lanes_dev.h addresses a lane's channel by offset) --, the non-zero scratch, status
	// words, LZ77 windows, the scratch of the 128/256-sized transforms
	st->coeff_floats = hp.coeff_floats;
	st->num_blocks = hp.group_blocks.size();
	const int32_t num_groups = hp.frame.num_groups;
	{
		auto align = [](size_t v) { return (v + 255) & ~(size_t) 255; };
		const bool sparse = hp.frame.sparse_coeffs != 0;
		const size_t stride = (st->coeff_floats + 63) & ~(size_t) 63;
		const size_t coeff_bytes = sparse ? sizeof(CoeffEvent) * hp.ev_capacity : sizeof(float) * 3 * stride;
		const size_t w_coeffs = 0, w_blk = align(w_coeffs + coeff_bytes), blk_bytes = sparse ? sizeof(uint32_t) * 4 * st->num_blocks : 0;
		const size_t w_nz = align(w_blk + blk_bytes), w_status = align(w_nz + (size_t) num_groups * 32 * 32 * 3);
		const size_t w_endbit = align(w_status + sizeof(uint32_t) * hp.sections.size());
		const size_t w_lz = align(w_endbit + (hp.frame.sections_have_trailer ? sizeof(uint32_t) * hp.sections.size() : 0)), lz_bytes = sizeof(int32_t) * (size_t) num_groups * hp.lz_window_size;
		// (the 128/256-sized transforms' scratch doubles as the LfGroup tail's: three planes of dequantised, smoothed LF samples, used
		// once at upload, long before any decode)
		const size_t w_large = align(w_lz + lz_bytes), large_bytes = std::max(sizeof(float) * (size_t) hp.max_large * 6 * 65536, hp.lf_tail_pending ? sizeof(float) * 3 * cells : (size_t) 0);
		uint8_t *wb = st->work_block.ensure(device, w_large + large_bytes + 256, true) ? (uint8_t *) st->work_block.ptr : nullptr;
		if (!wb) ok = false;
		else {
			if (sparse) {
				plan.events = (CoeffEvent *) (wb + w_coeffs); plan.block_events = (uint32_t *) (wb + w_blk);
				if (hipMemsetAsync(plan.block_events, 0, blk_bytes, s) != hipSuccess) ok = false;   // recycled memory: no entry may point outside the event list
			}
			else for (int c = 0; c < 3; ++c) plan.coeffs[c] = (float *) (wb + w_coeffs) + (size_t) c * stride;
			plan.coeff_stride = (uint32_t) stride;
			plan.nonzeros = (int8_t *) (wb + w_nz); plan.status = (uint32_t *) (wb + w_status);
			plan.section_end_bit = hp.frame.sections_have_trailer ? (uint32_t *) (wb + w_endbit) : nullptr;
			plan.lz_window_size = hp.lz_window_size;
			plan.lz_window = hp.lz_window_size ? (int32_t *) (wb + w_lz) : nullptr;
			st->d_large_scratch = hp.max_large ? (float *) (wb + w_large) : nullptr;
			if (hp.lf_tail_pending && ok) {   // the LfGroup tail: LF integers -> LLF coefficients, on the upload stream behind the copy
				int32_t max_cells = 0;
				for (const DevLfGroup &g : hp.lf_groups) max_cells = std::max(max_cells, g.width8 * g.height8);
				launch_lf_tail(plan, (int32_t) hp.lf_groups.size(), max_cells, cells, (float *) (wb + w_large), st->d_vb_sorted, (int32_t) st->vb_count, st->class_start[18], hp.lf_smooth ? 1 : 0, hp.inv_m_lf, s);
			}
		}
	}
	if (h->frame.fh.use_lf_frame) {   // its LfGroup tail runs at every decode, on the LF frame's picture: the planes it goes through
		st->lf_cells = cells;
		for (const DevLfGroup &g : hp.lf_groups) st->lf_max_cells = std::max(st->lf_max_cells, g.width8 * g.height8);
		st->d_lf_frame = st->scratch<float>(3 * std::max<size_t>(cells, 1), ok);
	}
	st->total_sections = (int32_t) hp.sections.size();
	st->has_trailers = hp.frame.sections_have_trailer != 0 && !h->from_view;
	st->first_group = 0; st->num_groups = num_groups;
	for (auto &e : st->ev) if (hipEventCreate(&e) != hipSuccess) ok = false;
	// (asleep while the copy runs, like lf_device_decode: a pipeline may have many more uploading threads than CPUs)
	if (!t_lf_done && hipEventCreateWithFlags(&t_lf_done, hipEventBlockingSync | hipEventDisableTiming) != hipSuccess) { t_lf_done = nullptr; (void) hipGetLastError(); }
	if (t_lf_done ? (hipEventRecord(t_lf_done, s) != hipSuccess || hipEventSynchronize(t_lf_done) != hipSuccess) : hipStreamSynchronize(s) != hipSuccess) ok = false;
	if (timing) fprintf(stderr, "[j40hip upload] plan build %.2f ms (%d threads), staging %.2f ms (%.1f MB), copy + LfGroup tail + wait %.2f ms\n", tu1 - tu0, h->threads, tu2 - tu1, (double) copy_bytes / 1e6, now() - tu2);
	if (!ok) { j40hip_release_device(h); return ERR_GPU; }
	return upload_patches(h, s);
}

extern "C" void j40hip_frame_force_dense(j40hip_frame *h, int dense) { if (h) h->force_dense = dense != 0; }

static uint32_t j40hip_frame_set_group_range_body(j40hip_frame *h, int64_t first_group, int64_t num_groups) {
	if (!h || !h->dev) return ERR_GPU;
	if (first_group < 0 || num_groups < 0 || first_group + num_groups > h->frame.fh.num_groups) return ERR_RNGE;
	const bool whole = first_group == 0 && num_groups == h->frame.fh.num_groups;
	if (!whole) if (uint32_t e = mode_refusal(h, Mode::GroupRange)) return e;   // (a region, a scale, an orientation in force: decode_route.hpp)
	j40hip_device_state *st = h->dev;
	if (st->is_modular) {
		// Modular frames: the groups' sections are independent of each other (no predictor looks across a group's edge), and so are
		// the per-pixel inverse transforms (RCT, plain palette); a palette with predicted deltas or a Squeeze step reads across
		// groups, and frames coded with Squeeze have no one-section-per-group layout at all: those are decoded whole
		if (!whole && !modular_groups_independent(h)) return ERR_TODO;
	}
	st->first_group = first_group; st->num_groups = num_groups; h->partial_range = !whole;
	if (whole || st->is_modular) return 0;
	// varblocks never straddle a group (the largest transform is one group wide), so the pixel kernels' work lists are
	// the full lists filtered by the group of each block's top-left pixel
	const FrameHeader &fh = h->frame.fh;
	const int32_t shift = fh.group_size_shift;
	std::vector<DevVarblock> sel;
	if (!host_vb_sorted(st)) return ERR_GPU;
	for (const DevVarblock &vb : st->vb_sorted) {
		const int64_t gid = ((int64_t) vb.py >> shift) * fh.gcolumns + ((int64_t) vb.px >> shift);
		if (gid >= first_group && gid < first_group + num_groups) sel.push_back(vb);
	}
	size_t k = 0;   // sel keeps the DctSelect order of vb_sorted
	for (int d = 0; d <= 27; ++d) { while (k < sel.size() && sel[k].dctsel < d) ++k; st->range_class_start[d] = (int32_t) k; }
	if (hipSetDevice(st->device) != hipSuccess) return ERR_GPU;
	if (sel.size() > st->vb_range_capacity) {
		bool ok = true;
		st->d_vb_range = st->scratch<DevVarblock>(sel.size(), ok);
		if (!ok) return ERR_GPU;
		st->vb_range_capacity = sel.size();
	}
	if (!sel.empty() && hipMemcpy(st->d_vb_range, sel.data(), sizeof(DevVarblock) * sel.size(), hipMemcpyHostToDevice) != hipSuccess) return ERR_GPU;
	return 0;
}
extern "C" uint32_t j40hip_frame_upload(j40hip_frame *h, int device) { return guarded([&] { return upload_impl(h, device, nullptr); }); }
extern "C" uint32_t j40hip_frame_set_group_range(j40hip_frame *h, int64_t first_group, int64_t num_groups) { return guarded([&] { return j40hip_frame_set_group_range_body(h, first_group, num_groups); }); }
extern "C" uint32_t j40hip_frame_upload_on(j40hip_frame *h, int device, void *stream) { return guarded([&] { return upload_impl(h, device, (hipStream_t) stream); }); }
