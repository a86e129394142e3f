// j40_amd/csrc/device/runtime_shared.hpp -- what device_memory.hip shares with the runtime units, async.hip, pipeline.hip and
// hostcopy.hip: the per-device cache of device memory blocks and the one-time upload of the kernels' constant tables
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <algorithm>
#include <hip/hip_runtime.h>
#include "../env.hpp"

extern "C" void j40hip_cache_counters(uint64_t *out);   // device_memory.hip: what the device memory cache did (J40HIP_ASYNC_TIMING)

namespace j40hip_rt {

// switches that more than one unit reads, each with one meaning
inline bool async_timing() { return j40hip::env_str("J40HIP_ASYNC_TIMING") != nullptr; }   // (looked at per call)
inline bool generic_lanes() { return j40hip::env_on("J40HIP_GENERIC_LANES", false); }        // =1: the batches' entropy launch through the general kernel (per call)
inline int waves_per_wg(int dflt, int hi) { return j40hip::env_int("J40HIP_WAVES_PER_WG", dflt, 1, hi); }

// a block of at least `bytes` (rounded up to 4 KB) from the device's cache or from hipMalloc; null when the device is out of memory
void *cache_acquire(int device, size_t bytes, size_t *got, bool *clean);
// gives a block back; nothing may still be running on it
void cache_release(int device, void *ptr, size_t bytes, bool clean);
void cache_trim(int device);
bool ensure_constant_tables(int device);

// A block of the cache in its owner's hands. No destructor: at process exit the runtime may be gone before the owner, so owners
// release explicitly. idle: nothing is pending on the device, handing the memory to another frame needs no device-wide wait.
struct CacheBlock {
	int device = 0; void *ptr = nullptr; size_t bytes = 0;
	void release(bool idle) {
		if (ptr && !idle) (void) hipDeviceSynchronize();   // nothing may still be running on memory that is about to be handed on
		cache_release(device, ptr, bytes, false);
		ptr = nullptr; bytes = 0;
	}
	// keeps a block that is large enough, else gives it back and takes one that is; false: the device is out of memory
	bool ensure(int dev, size_t want, bool idle) {
		if (ptr && bytes >= want) return true;
		release(idle);
		bool clean = false;
		device = dev; ptr = cache_acquire(dev, want, &bytes, &clean);
		return ptr != nullptr;
	}
};

// host-side staging of the plan: every array lands in one blob at a 256-byte aligned offset, one copy moves it. The blob lives
// in PINNED host memory owned by the calling thread (grown on demand, reused by that thread's next upload), so the copy is a
// true asynchronous DMA that overlaps the kernels of other frames; j40hip_thread_release gives it back.
struct PinnedStage {
	uint8_t *ptr = nullptr; size_t cap = 0;
	bool reserve(size_t n, size_t keep) {
		if (n <= cap) return true;
		size_t want = std::max(n + n / 4, (size_t) 1 << 20);
		void *q = nullptr;
		if (hipHostMalloc(&q, want, hipHostMallocDefault) != hipSuccess) { (void) hipGetLastError(); return false; }
		if (keep) memcpy(q, ptr, keep);
		if (ptr) (void) hipHostFree(ptr);
		ptr = (uint8_t *) q; cap = want;
		return true;
	}
	void release() { if (ptr) (void) hipHostFree(ptr); ptr = nullptr; cap = 0; }
};

} // namespace j40hip_rt
