// j40_amd/csrc/device/device_memory.hip -- the memory the runtime recycles: the per-device cache of device blocks, the pool of pinned
// image planes, the one-time upload of the constant tables, the calling thread's staging buffers; j40hip_shutdown
#include "runtime_state.hpp"
#include "hostcopy.hpp"
#include "block_cache.hpp"
#include "async.hpp"

namespace {

// The device memory cache: one BlockCacheCore (block_cache.hpp: free list, size classes, slabs) per device behind one mutex; the
// slow part -- hipMalloc / hipFree -- happens outside the lock.
std::mutex g_cache_mutex;
std::condition_variable g_cache_cv;      // a slab of some class has been adopted (or its allocation failed)
BlockCacheCore g_cache[16];
std::vector<size_t> g_slab_pending[16];  // size classes whose slab some thread is allocating right now
// Upper bound on what the cache of ONE device keeps idle, per process (J40HIP_CACHE_GB overrides; 0 disables recycling and slabs).
// When an allocation fails the cache is emptied and the allocation tried again (cache_trim), so idle blocks never turn into a
// spurious "!gpu". Default: 60 % of the device's memory -- a pipeline returns the working sets of a whole batch at once (256 8K
// frames: 54 GB), and hipFree / hipMalloc of such blocks cost tens of milliseconds each and synchronise the device. Processes that
// share a device (several ranks on one GPU, multi-tenant serving) each keep up to this much: set J40HIP_CACHE_GB to the device's
// memory divided by their number, less what the frames in flight need.
// what the cache did, for J40HIP_ASYNC_TIMING (j40hip_cache_counters): calls, and the milliseconds spent waiting for the lock, searching
// the free list, inside hipMalloc and inside hipFree
struct CacheCounters { std::atomic<uint64_t> acquires{0}, hits{0}, slab_mallocs{0}, plain_mallocs{0}, frees{0}, lock_us{0}, take_us{0}, malloc_us{0}, free_us{0}, idle_blocks{0}; };
CacheCounters g_cache_counters;
inline uint64_t cache_us() { return (uint64_t) std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
std::mutex g_limit_mutex;
size_t g_limit[16]; bool g_limit_known[16];
size_t cache_limit_bytes(int device) {   // (never called with g_cache_mutex held: hipMemGetInfo takes its time)
	if (device < 0 || device >= 16) return 0;
	{ std::lock_guard<std::mutex> lock(g_limit_mutex); if (g_limit_known[device]) return g_limit[device]; }
	size_t limit = (size_t) 48 << 30;
	if (const int gb = env_int("J40HIP_CACHE_GB", -1, 0, INT_MAX); gb >= 0) limit = (size_t) gb << 30;
	else {
		int cur = -1; size_t free_b = 0, total_b = 0;
		const bool switched = hipGetDevice(&cur) == hipSuccess && cur != device && hipSetDevice(device) == hipSuccess;
		if (hipMemGetInfo(&free_b, &total_b) == hipSuccess) limit = total_b / 10 * 6; else (void) hipGetLastError();
		if (switched) (void) hipSetDevice(cur);
	}
	std::lock_guard<std::mutex> lock(g_limit_mutex);
	g_limit[device] = limit; g_limit_known[device] = true;
	return limit;
}

} // namespace

// frees every cached block of `device` that can be freed (they are idle by construction: blocks enter the cache after a device
// synchronisation); the idle blocks of a slab that still has blocks in use stay
void j40hip_rt::cache_trim(int device) {
	if (device < 0 || device >= 16) return;
	std::vector<void *> gone;
	{ std::lock_guard<std::mutex> lock(g_cache_mutex); g_cache[device].trim(&gone); }
	for (void *q : gone) (void) hipFree(q);
}

void *j40hip_rt::cache_acquire(int device, size_t bytes, size_t *got, bool *clean) {
	bytes = BlockCacheCore::size_class(bytes);
	const bool cached = device >= 0 && device < 16;
	const size_t limit = cached ? cache_limit_bytes(device) : 0;
	bool slab = cached && limit > 0 && BlockCacheCore::slab_class(bytes);
	if (cached) {
		// One thread per size class allocates a slab; whoever else misses the class meanwhile waits for it and looks again (when a
		// pipeline starts, every worker misses the empty cache at the same moment: each of them used to allocate a slab of its own)
		const uint64_t tl0 = cache_us();
		std::unique_lock<std::mutex> lock(g_cache_mutex);
		const uint64_t tl1 = cache_us();
		g_cache_counters.lock_us += tl1 - tl0; ++g_cache_counters.acquires;
		for (;;) {
			const uint64_t tt0 = cache_us();
			void *q = g_cache[device].take(bytes, got, clean);
			g_cache_counters.take_us += cache_us() - tt0; g_cache_counters.idle_blocks = g_cache[device].idle.size();
			if (q) { ++g_cache_counters.hits; return q; }
			std::vector<size_t> &pend = g_slab_pending[device];
			if (!slab || std::find(pend.begin(), pend.end(), bytes) == pend.end()) { if (slab) pend.push_back(bytes); break; }
			g_cache_cv.wait(lock);
		}
	}
	void *p = nullptr;
	if (slab) {
		// a slab is up to 64 blocks / 1 GB; smaller when the device is short of memory or the cache near its limit (its idle blocks count)
		int n = BlockCacheCore::slab_blocks(bytes);
		size_t free_b = 0, total_b = 0, idle_b = 0;
		{ std::lock_guard<std::mutex> lock(g_cache_mutex); idle_b = g_cache[device].idle_bytes; }
		if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) { (void) hipGetLastError(); free_b = 0; }
		while (n > 1 && (bytes * (size_t) n > free_b / 4 || idle_b + bytes * (size_t) (n - 1) > limit)) n /= 2;
		const uint64_t tm0 = cache_us();
		if (n > 1 && hipMalloc(&p, bytes * (size_t) n) != hipSuccess) { (void) hipGetLastError(); p = nullptr; }
		g_cache_counters.malloc_us += cache_us() - tm0; ++g_cache_counters.slab_mallocs;
		{
			std::lock_guard<std::mutex> lock(g_cache_mutex);
			if (p) g_cache[device].adopt_slab(p, bytes, n);
			std::vector<size_t> &pend = g_slab_pending[device];
			pend.erase(std::find(pend.begin(), pend.end(), bytes));
		}
		g_cache_cv.notify_all();
		if (p) { *got = bytes; *clean = false; return p; }
	}
	const uint64_t tm0 = cache_us();
	const hipError_t first_try = hipMalloc(&p, bytes);
	g_cache_counters.malloc_us += cache_us() - tm0; ++g_cache_counters.plain_mallocs;
	if (first_try != hipSuccess) {
		// out of device memory while blocks sit idle in the cache: give them back and try once more
		(void) hipGetLastError();
		cache_trim(device);
		if (hipMalloc(&p, bytes) != hipSuccess) { (void) hipGetLastError(); return nullptr; }
	}
	*got = bytes; *clean = false;
	return p;
}

void j40hip_rt::cache_release(int device, void *ptr, size_t bytes, bool clean) {
	if (!ptr) return;
	void *gone = ptr;
	if (device >= 0 && device < 16) {
		const size_t limit = cache_limit_bytes(device);
		std::lock_guard<std::mutex> lock(g_cache_mutex);
		g_cache[device].give(ptr, bytes, clean, limit, &gone);
	}
	if (gone) { const uint64_t tf0 = cache_us(); (void) hipFree(gone); g_cache_counters.free_us += cache_us() - tf0; ++g_cache_counters.frees; }
}

// out[10]: acquires, hits, slab allocations, plain allocations, frees, then microseconds: lock, free-list search, hipMalloc, hipFree; idle blocks now
extern "C" __attribute__((visibility("default"))) void j40hip_cache_counters(uint64_t *out) {
	const CacheCounters &c = g_cache_counters;
	out[0] = c.acquires; out[1] = c.hits; out[2] = c.slab_mallocs; out[3] = c.plain_mallocs; out[4] = c.frees;
	out[5] = c.lock_us; out[6] = c.take_us; out[7] = c.malloc_us; out[8] = c.free_us; out[9] = c.idle_blocks;
}

// ---- pinned host memory for pixels that go back to the caller (the public API's image planes): pinning 133 MB takes tens of
// milliseconds (0.2 s for 133 MB measured, as long again to unpin), so planes are recycled by size across images.
// What sits idle is bounded three ways (a drop-in caller never calls j40hip_shutdown, and pinned memory cannot be swapped):
//   * J40HIP_PINNED_POOL_GB (default: the smaller of 32 GB -- 240 planes of an 8K image; with 128 callers and a 16 GB bound every
//     j40_free beyond the 123rd plane unpinned it and the next image pinned a new one -- and a quarter of the machine's memory;
//     0: nothing kept);
//   * a plane that does not fit is made room for by unpinning the planes that have been idle longest (a process that moves on to
//     another image size does not keep the old size's planes and pin / unpin every image of the new one);
//   * planes idle for more than J40HIP_PINNED_IDLE_S seconds (default 30) are unpinned at the library's next acquire or release.
namespace {
struct PinnedIdle { void *ptr; size_t bytes; double since; };
std::mutex g_pinned_mutex;
std::vector<PinnedIdle> g_pinned_idle;   // oldest first
size_t g_pinned_idle_bytes = 0;
size_t pinned_limit() {
	static const size_t v = [] {
		if (const int gb = env_int("J40HIP_PINNED_POOL_GB", -1, 0, INT_MAX); gb >= 0) return (size_t) gb << 30;
		const long pages = sysconf(_SC_PHYS_PAGES), page = sysconf(_SC_PAGESIZE);
		const size_t ram = pages > 0 && page > 0 ? (size_t) pages * (size_t) page : (size_t) 128 << 30;
		return std::min((size_t) 32 << 30, ram / 4);
	}();
	return v;
}
double pinned_idle_seconds() { static const double v = [] { const char *e = env_str("J40HIP_PINNED_IDLE_S"); return e && atof(e) > 0 ? atof(e) : 30.0; }(); return v; }
double pinned_now() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
// (under g_pinned_mutex) moves to `gone`: planes idle for too long, then the oldest ones until `incoming` more bytes fit the bound
void pinned_make_room(size_t incoming, std::vector<void *> *gone) {
	const double now = pinned_now(), keep = pinned_idle_seconds();
	size_t n = 0;
	while (n < g_pinned_idle.size() && (now - g_pinned_idle[n].since > keep || g_pinned_idle_bytes + incoming > pinned_limit())) {
		gone->push_back(g_pinned_idle[n].ptr); g_pinned_idle_bytes -= g_pinned_idle[n].bytes; ++n;
	}
	g_pinned_idle.erase(g_pinned_idle.begin(), g_pinned_idle.begin() + (long) n);
}
}
extern "C" __attribute__((visibility("default"))) void *j40hip_pinned_acquire(size_t bytes) {
	bytes = (bytes + 4095) & ~(size_t) 4095;
	std::vector<void *> gone;
	void *q = nullptr;
	{
		std::lock_guard<std::mutex> lock(g_pinned_mutex);
		for (size_t i = g_pinned_idle.size(); i-- > 0; ) if (g_pinned_idle[i].bytes == bytes) {   // the most recently used plane of this size
			q = g_pinned_idle[i].ptr;
			g_pinned_idle.erase(g_pinned_idle.begin() + (long) i); g_pinned_idle_bytes -= bytes;
			break;
		}
		pinned_make_room(q ? 0 : bytes, &gone);   // (a miss: the plane pinned now will come back to the pool)
	}
	for (void *g : gone) (void) hipHostFree(g);
	if (q) return q;
	if (hipHostMalloc(&q, bytes ? bytes : 4096, hipHostMallocDefault) != hipSuccess) { (void) hipGetLastError(); return nullptr; }
	return q;
}
extern "C" __attribute__((visibility("default"))) void j40hip_pinned_release(void *ptr, size_t bytes) {
	if (!ptr) return;
	bytes = (bytes + 4095) & ~(size_t) 4095;
	std::vector<void *> gone;
	{
		std::lock_guard<std::mutex> lock(g_pinned_mutex);
		pinned_make_room(bytes, &gone);
		if (g_pinned_idle_bytes + bytes <= pinned_limit()) { g_pinned_idle.push_back({ptr, bytes, pinned_now()}); g_pinned_idle_bytes += bytes; ptr = nullptr; }
	}
	for (void *g : gone) (void) hipHostFree(g);
	if (ptr) (void) hipHostFree(ptr);
}
// (what the pool holds: tests/test_api_threads.py)
extern "C" __attribute__((visibility("default"))) void j40hip_pinned_pool_stats(uint64_t *idle_bytes, uint64_t *idle_planes, uint64_t *limit_bytes) {
	std::lock_guard<std::mutex> lock(g_pinned_mutex);
	if (idle_bytes) *idle_bytes = g_pinned_idle_bytes;
	if (idle_planes) *idle_planes = g_pinned_idle.size();
	if (limit_bytes) *limit_bytes = pinned_limit();
}
static void pinned_trim() {
	std::vector<PinnedIdle> gone;
	{ std::lock_guard<std::mutex> lock(g_pinned_mutex); gone.swap(g_pinned_idle); g_pinned_idle_bytes = 0; }
	for (auto &b : gone) (void) hipHostFree(b.ptr);
}

bool DeviceBuffer::alloc(size_t n) {
	bytes = n;
	if (hipMalloc(&ptr, n ? n : 16) == hipSuccess) return true;
	(void) hipGetLastError();
	int device = 0;
	if (hipGetDevice(&device) == hipSuccess) cache_trim(device);
	return hipMalloc(&ptr, n ? n : 16) == hipSuccess;
}

// the constant tables of the pixel kernels go up once per device (they never change)
static std::mutex g_const_mutex;
static bool g_const_done[16];
bool j40hip_rt::ensure_constant_tables(int device) {
	if (device < 0 || device >= 16) return false;
	std::lock_guard<std::mutex> lock(g_const_mutex);
	if (g_const_done[device]) return true;
	upload_constant_tables(half_secants(), afv_basis(), srgb_u8_thresholds(), nullptr);
	upload_lf_tail_tables(half_secants(), lf2llf_scales(), nullptr);
	upload_lf_preview_tables(srgb_u8_thresholds(), nullptr);
	upload_modular_xyb_tables(srgb_u8_thresholds(), nullptr);
	if (hipStreamSynchronize(nullptr) != hipSuccess) return false;
	return g_const_done[device] = true;
}

thread_local PinnedStage j40hip_rt::t_stage, j40hip_rt::t_lf_out;
thread_local hipEvent_t j40hip_rt::t_lf_done = nullptr;
thread_local HostPlan j40hip_rt::t_host_plan;
extern "C" void j40hip_thread_release(void) { t_stage.release(); t_lf_out.release(); if (t_lf_done) { (void) hipEventDestroy(t_lf_done); t_lf_done = nullptr; } t_host_plan = HostPlan(); }

// Takes the library's process-wide state down: stops and joins the LfGroup service threads, gives the cached device memory back.
// No other call into the library may be running or follow on objects created before. Optional: a process may also just end.
extern "C" void j40hip_shutdown(void) {
	lf_services_shutdown();
	j40hip_serve_shutdown();
	j40hip_async_shutdown();
	two_phase_shutdown();
	lfp_args_shutdown();
	hostcopy_shutdown();
	pinned_trim();
	int n = 0;
	if (hipGetDeviceCount(&n) != hipSuccess) { (void) hipGetLastError(); n = 0; }
	for (int d = 0; d < n && d < 16; ++d) if (hipSetDevice(d) == hipSuccess) { (void) hipDeviceSynchronize(); cache_trim(d); }
	j40hip_thread_release();
}
