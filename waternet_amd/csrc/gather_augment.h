// Tile index math of k_gather_augment_u8 (elementwise.hip): gather one
// cached uint8 HWC image into a batch slot under a joint flip/rot90 code.
//
// Augmentation code (PairedAugment order: hflip, vflip, then np.rot90 k):
//   bit 0 hflip, bit 1 vflip, bits 2-3 k (counter-clockwise quarter turns).
// Output pixel (oy,ox) of an HxW source reads source pixel
//   k=0 (oy,ox)  k=1 (ox,W-1-oy)  k=2 (H-1-oy,W-1-ox)  k=3 (H-1-ox,oy)
// then y=H-1-y if vflip, x=W-1-x if hflip. Every case is the affine map
//   y = ay*oy + by*ox + cy,  x = ax*oy + bx*ox + cx   (coefficients -1/0/1)
// so the code costs a handful of block-uniform scalars and no per-lane
// branch.
//
// One block moves one GA_TILE x GA_TILE output tile through an LDS pixel
// tile kept in SOURCE orientation: phase 1 copies the source rectangle that
// the output tile maps to, row-contiguous dwords in, phase 2 assembles each
// output dword from four LDS bytes and stores row-contiguous dwords out.
// Both global sides are therefore row-contiguous for every code, the two
// transposes included. W % 8 == 0 makes every row, every tile origin
// (multiples of 8 pixels = 24 B, in both directions) and every tile width
// in bytes a multiple of 4.
//
// The two phases are plain functions of (tid, tile) so a host program can
// run them over every thread with bounds-checked buffers.
#pragma once

#include <cstdint>

#if defined(__HIPCC__)
#define GA_HD __host__ __device__ __forceinline__
#else
#define GA_HD inline
#endif

constexpr int GA_TILE = 32;                  // pixels per tile side
constexpr int GA_ROW_DW = GA_TILE * 3 / 4;   // 24 dwords per full tile row
// LDS row stride 25 dwords: the transposed codes read down a column, and an
// odd dword stride spreads the 32 rows over 32 distinct banks
constexpr int GA_LDS_STRIDE = GA_ROW_DW * 4 + 4;        // bytes
constexpr int GA_LDS_BYTES = GA_TILE * GA_LDS_STRIDE;   // 3200
constexpr int GA_THREADS = 256;
constexpr int GA_ITEMS = GA_TILE * GA_ROW_DW;           // 768 dwords / tile
static_assert(GA_ITEMS % GA_THREADS == 0, "whole passes over the tile");

struct GaTile {
  int ay, by, cy, ax, bx, cx;  // source (y,x) from output (oy,ox)
  int oy0, ox0, th, tw;        // output tile origin / extent (pixels)
  int sy0, sx0, srows, scols;  // source rectangle feeding it
};

GA_HD GaTile ga_make_tile(int code, bool allow_transpose, int H, int W,
                          int tile_y, int tile_x) {
  int k = (code >> 2) & 3;
  if (!allow_transpose) k &= 2;
  GaTile t;
  t.ay = (k == 0) - (k == 2);
  t.by = (k == 1) - (k == 3);
  t.cy = (k >= 2) ? H - 1 : 0;
  t.ax = (k == 3) - (k == 1);
  t.bx = (k == 0) - (k == 2);
  t.cx = (k == 1 || k == 2) ? W - 1 : 0;
  if (code & 2) { t.ay = -t.ay; t.by = -t.by; t.cy = H - 1 - t.cy; }
  if (code & 1) { t.ax = -t.ax; t.bx = -t.bx; t.cx = W - 1 - t.cx; }
  t.oy0 = tile_y * GA_TILE;
  t.ox0 = tile_x * GA_TILE;
  t.th = H - t.oy0 < GA_TILE ? H - t.oy0 : GA_TILE;
  t.tw = W - t.ox0 < GA_TILE ? W - t.ox0 : GA_TILE;
  // the map is monotone in each output axis: the source rectangle is
  // spanned by the images of the two opposite tile corners
  const int oy1 = t.oy0 + t.th - 1, ox1 = t.ox0 + t.tw - 1;
  const int ya = t.ay * t.oy0 + t.by * t.ox0 + t.cy;
  const int yb = t.ay * oy1 + t.by * ox1 + t.cy;
  const int xa = t.ax * t.oy0 + t.bx * t.ox0 + t.cx;
  const int xb = t.ax * oy1 + t.bx * ox1 + t.cx;
  t.sy0 = ya < yb ? ya : yb;
  t.sx0 = xa < xb ? xa : xb;
  const bool tr = k & 1;
  t.srows = tr ? t.tw : t.th;
  t.scols = tr ? t.th : t.tw;
  return t;
}

// Phase 1: source rectangle -> LDS (source orientation), 4 B per lane.
// `src` is the selected cache image (H*W*3 bytes, 4-byte aligned).
GA_HD void ga_load_tile(const GaTile& t, int tid, int W,
                        const uint8_t* src, uint8_t* lds) {
  const int dw = t.scols * 3 / 4;
#if defined(__HIPCC__)
#pragma unroll
#endif
  for (int it = 0; it < GA_ITEMS / GA_THREADS; ++it) {
    const int i = it * GA_THREADS + tid;
    const int r = i / GA_ROW_DW, d = i - r * GA_ROW_DW;
    if (r < t.srows && d < dw) {
      const long off = ((long)(t.sy0 + r) * W + t.sx0) * 3 + 4 * d;
      *reinterpret_cast<uint32_t*>(lds + r * GA_LDS_STRIDE + 4 * d) =
          *reinterpret_cast<const uint32_t*>(src + off);
    }
  }
}

// Phase 2: LDS -> output tile, each lane packs one row-contiguous dword.
// `dst` is the batch slot (H*W*3 bytes, 4-byte aligned).
GA_HD void ga_store_tile(const GaTile& t, int tid, int W,
                         const uint8_t* lds, uint8_t* dst) {
  const int dw = t.tw * 3 / 4;
#if defined(__HIPCC__)
#pragma unroll
#endif
  for (int it = 0; it < GA_ITEMS / GA_THREADS; ++it) {
    const int i = it * GA_THREADS + tid;
    const int r = i / GA_ROW_DW, d = i - r * GA_ROW_DW;
    if (r < t.th && d < dw) {
      const int oy = t.oy0 + r;
      uint32_t v = 0;
#if defined(__HIPCC__)
#pragma unroll
#endif
      for (int j = 0; j < 4; ++j) {
        const int b = 4 * d + j;
        const int px = b / 3, c = b - 3 * px;
        const int ox = t.ox0 + px;
        const int ly = t.ay * oy + t.by * ox + t.cy - t.sy0;
        const int lx = t.ax * oy + t.bx * ox + t.cx - t.sx0;
        v |= (uint32_t)lds[ly * GA_LDS_STRIDE + lx * 3 + c] << (8 * j);
      }
      const long off = ((long)oy * W + t.ox0) * 3 + 4 * d;
      *reinterpret_cast<uint32_t*>(dst + off) = v;
    }
  }
}
