// j40_amd/csrc/device/orient_dev.h -- oriented output (j40hip_frame_set_orientation): the arithmetic of the image orientation, written
// once. Compiled for the device by k_orient (orient_kernels.hip), for the host by the runtime and the C interface (output sizes, the
// rectangle maps), and for the CPU by tests/hostsim/orient_sim.cpp: the same functions.
//
// Orientation o in 1..8 is the EXIF numbering (the codestream's image metadata holds o - 1). The stored image is W x H, P(x, y) its
// pixels; the oriented image is ow x oh and its pixel (i, j) is P(x, y) with
//   o  ow x oh  (x, y)                      o  ow x oh  (x, y)
//   1  W x H    (i, j)                      5  H x W    (j, i)
//   2  W x H    (W - 1 - i, j)              6  H x W    (j, H - 1 - i)
//   3  W x H    (W - 1 - i, H - 1 - j)      7  H x W    (W - 1 - j, H - 1 - i)
//   4  W x H    (i, H - 1 - j)              8  H x W    (W - 1 - j, i)
// Orientations 2 to 4 keep rows rows (orient_row); 5 to 8 turn rows into columns and go through a tile (orient_tile_load,
// orient_tile_store).
#pragma once
#include <stdint.h>
#include <stddef.h>
#include <string.h>
#ifndef J40_HD
#ifdef __HIPCC__
#define J40_HD __host__ __device__ __forceinline__
#else
#define J40_HD static inline
#endif
#endif

namespace j40hip {

// The tile of orientations 5 to 8: ORIENT_TILE x ORIENT_TILE source pixels, ORIENT_LANES lanes, lane l at column l % ORIENT_TILE of
// rows l / ORIENT_TILE + k * ORIENT_ROWS. A row of the tile is ORIENT_PITCH pixels apart from the next: one pixel of padding, so that
// the column-wise reads of the store step fall on different banks (DESIGN.md section 4 has the calculation for 4- and 8-byte pixels).
enum { ORIENT_TILE = 32, ORIENT_LANES = 256, ORIENT_ROWS = ORIENT_LANES / ORIENT_TILE, ORIENT_PITCH = ORIENT_TILE + 1, ORIENT_TILE_PIXELS = ORIENT_TILE * ORIENT_PITCH };

template <int PB> struct OrientPixel;
template <> struct OrientPixel<4> { typedef uint32_t type; };
template <> struct OrientPixel<8> { typedef uint64_t type; };

J40_HD bool orient_valid(int32_t o) { return o >= 1 && o <= 8; }
J40_HD bool orient_transposes(int32_t o) { return o >= 5; }
// x runs against i (or j), y runs against j (or i)
J40_HD bool orient_mirrors_x(int32_t o) { return o == 2 || o == 3 || o == 7 || o == 8; }
J40_HD bool orient_mirrors_y(int32_t o) { return o == 3 || o == 4 || o == 6 || o == 7; }
// the orientation that undoes o: 6 and 8 undo each other, every other one undoes itself
J40_HD int32_t orient_inverse(int32_t o) { return o == 6 ? 8 : o == 8 ? 6 : o; }

J40_HD void orient_out_size(int32_t W, int32_t H, int32_t o, int32_t *ow, int32_t *oh) {
	*ow = orient_transposes(o) ? H : W; *oh = orient_transposes(o) ? W : H;
}
// the stored pixel (x, y) that output pixel (i, j) shows
J40_HD void orient_source(int32_t W, int32_t H, int32_t o, int32_t i, int32_t j, int32_t *x, int32_t *y) {
	const int32_t u = orient_transposes(o) ? j : i, v = orient_transposes(o) ? i : j;
	*x = orient_mirrors_x(o) ? W - 1 - u : u;
	*y = orient_mirrors_y(o) ? H - 1 - v : v;
}
// ... and the output pixel (i, j) that shows stored pixel (x, y): orient_source of the inverse orientation over the oriented image
J40_HD void orient_dest(int32_t W, int32_t H, int32_t o, int32_t x, int32_t y, int32_t *i, int32_t *j) {
	int32_t ow, oh;
	orient_out_size(W, H, o, &ow, &oh);
	orient_source(ow, oh, orient_inverse(o), x, y, i, j);
}
// Rectangle {x0, y0, w, h} of the oriented image (inside ow x oh) as the rectangle of the stored W x H image that holds the same pixels
J40_HD void orient_rect_to_stored(int32_t W, int32_t H, int32_t o, const int32_t in[4], int32_t out[4]) {
	int32_t xa, ya, xb, yb;
	orient_source(W, H, o, in[0], in[1], &xa, &ya);
	orient_source(W, H, o, in[0] + in[2] - 1, in[1] + in[3] - 1, &xb, &yb);
	out[0] = xa < xb ? xa : xb; out[1] = ya < yb ? ya : yb;
	out[2] = orient_transposes(o) ? in[3] : in[2]; out[3] = orient_transposes(o) ? in[2] : in[3];
}
// ... and back: rectangle {x0, y0, w, h} of the stored image as the rectangle of the oriented one
J40_HD void orient_rect_to_displayed(int32_t W, int32_t H, int32_t o, const int32_t in[4], int32_t out[4]) {
	int32_t ia, ja, ib, jb;
	orient_dest(W, H, o, in[0], in[1], &ia, &ja);
	orient_dest(W, H, o, in[0] + in[2] - 1, in[1] + in[3] - 1, &ib, &jb);
	out[0] = ia < ib ? ia : ib; out[1] = ja < jb ? ja : jb;
	out[2] = orient_transposes(o) ? in[3] : in[2]; out[3] = orient_transposes(o) ? in[2] : in[3];
}

// one pixel of PB bytes. The source image's rows are pixel-aligned; the output may sit anywhere (the caller's pointer and stride, as
// in stored order): ALIGNED says whether the output's pointer and stride are multiples of PB -- one decision per launch, a template
// parameter, so the aligned form carries no test --, and where they are not a pixel leaves byte by byte
#if defined(__HIP_DEVICE_COMPILE__)
template <int PB> J40_HD typename OrientPixel<PB>::type orient_load_pixel(const uint8_t *p) { return *(const typename OrientPixel<PB>::type *) p; }
template <int PB, bool ALIGNED> J40_HD void orient_store_pixel(uint8_t *d, typename OrientPixel<PB>::type v) {
	if (ALIGNED) { __builtin_nontemporal_store(v, (typename OrientPixel<PB>::type *) d); return; }
	for (int b = 0; b < PB; ++b) d[b] = (uint8_t) (v >> (8 * b));
}
#else
template <int PB> J40_HD typename OrientPixel<PB>::type orient_load_pixel(const uint8_t *p) { typename OrientPixel<PB>::type v; memcpy(&v, p, PB); return v; }
template <int PB, bool ALIGNED> J40_HD void orient_store_pixel(uint8_t *d, typename OrientPixel<PB>::type v) { memcpy(d, &v, PB); }
#endif

// ---- orientations 2 to 4: output row j by lane `lane` of `lanes`. Consecutive lanes take consecutive output pixels, whose sources are
// consecutive pixels of one source row, forwards or backwards: a wavefront's load and its store are each one contiguous run ----
template <int PB, bool ALIGNED = true> J40_HD void orient_row(const uint8_t *src, size_t src_stride, uint8_t *dst_row, int32_t W, int32_t H, int32_t o, int32_t j, int32_t lane, int32_t lanes) {
	for (int32_t i = lane; i < W; i += lanes) {
		int32_t x, y;
		orient_source(W, H, o, i, j, &x, &y);
		orient_store_pixel<PB, ALIGNED>(dst_row + (size_t) i * PB, orient_load_pixel<PB>(src + (size_t) y * src_stride + (size_t) x * PB));
	}
}

// ---- orientations 5 to 8: the tile whose first source pixel is (sx0, sy0), tw x th source pixels of it inside the image. Load: lane
// `lane` of ORIENT_LANES reads its pixels of ORIENT_TILE / ORIENT_ROWS source rows into `tile` -- lanes run along source rows. Store
// (after every lane of the tile has loaded): the tile's pixels are th x tw pixels of the output; lanes run along output rows, each reads
// `tile` down a column. Nothing outside the image is read and nothing outside the output's ow x oh pixels is written. ----
template <int PB> J40_HD void orient_tile_load(typename OrientPixel<PB>::type *tile, const uint8_t *src, size_t src_stride, int32_t W, int32_t H, int32_t sx0, int32_t sy0, int32_t lane) {
	const int32_t lx = lane % ORIENT_TILE, x = sx0 + lx;
	if (x >= W) return;
	for (int32_t ly = lane / ORIENT_TILE; ly < ORIENT_TILE && sy0 + ly < H; ly += ORIENT_ROWS)
		tile[ly * ORIENT_PITCH + lx] = orient_load_pixel<PB>(src + (size_t) (sy0 + ly) * src_stride + (size_t) x * PB);
}
template <int PB, bool ALIGNED = true> J40_HD void orient_tile_store(const typename OrientPixel<PB>::type *tile, uint8_t *dst, size_t dst_stride, int32_t W, int32_t H, int32_t o, int32_t sx0, int32_t sy0, int32_t lane) {
	const int32_t tw = W - sx0 < ORIENT_TILE ? W - sx0 : ORIENT_TILE, th = H - sy0 < ORIENT_TILE ? H - sy0 : ORIENT_TILE;
	// the output pixels of the tile: th of them along i from i0, tw rows from j0 (the tile's corner that comes first in the output)
	const int32_t i0 = orient_mirrors_y(o) ? H - sy0 - th : sy0, j0 = orient_mirrors_x(o) ? W - sx0 - tw : sx0;
	const int32_t a = lane % ORIENT_TILE;
	if (a >= th) return;
	for (int32_t b = lane / ORIENT_TILE; b < tw; b += ORIENT_ROWS) {
		int32_t x, y;
		orient_source(W, H, o, i0 + a, j0 + b, &x, &y);
		orient_store_pixel<PB, ALIGNED>(dst + (size_t) (j0 + b) * dst_stride + (size_t) (i0 + a) * PB, tile[(y - sy0) * ORIENT_PITCH + (x - sx0)]);
	}
}

} // namespace j40hip
