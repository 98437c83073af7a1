// Host run of k_gather_augment_u8's two tile phases (csrc/gather_augment.h)
// over every thread of every tile, for all 16 codes on a list of shapes.
// The same functions the kernel calls, on canary-fenced buffers: a read or
// write outside the source image, the batch slot or the LDS tile shows as a
// broken canary or a wrong byte. Exit status 0 = all good.
//
//   c++ -std=c++17 -I waternet_amd/csrc gather_tile_check.cpp && ./a.out
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "gather_augment.h"

namespace {
constexpr int FENCE = 256;
constexpr uint8_t CANARY = 0x5A, POISON = 0xCD, FILL = 0xAB;

struct Fenced {
  std::vector<uint8_t> buf;
  size_t n;
  Fenced(size_t n_, uint8_t fill) : buf(n_ + 2 * FENCE, CANARY), n(n_) {
    memset(data(), fill, n);
  }
  uint8_t* data() { return buf.data() + FENCE; }
  bool intact() const {
    for (int i = 0; i < FENCE; ++i)
      if (buf[i] != CANARY || buf[FENCE + n + i] != CANARY) return false;
    return true;
  }
};

void ref_map(int code, bool allow, int H, int W, int oy, int ox, int& y,
             int& x) {
  int k = (code >> 2) & 3;
  if (!allow) k &= 2;
  switch (k) {
    case 0: y = oy; x = ox; break;
    case 1: y = ox; x = W - 1 - oy; break;
    case 2: y = H - 1 - oy; x = W - 1 - ox; break;
    default: y = H - 1 - ox; x = oy;
  }
  if (code & 2) y = H - 1 - y;
  if (code & 1) x = W - 1 - x;
}

int check(int H, int W, int code, bool allow) {
  const size_t n = (size_t)H * W * 3;
  Fenced src(n, 0), dst(n, FILL);
  for (size_t i = 0; i < n; ++i) {
    uint8_t v = (uint8_t)((i * 7 + 3) % 251);
    src.data()[i] = (v == FILL || v == POISON || v == CANARY) ? 1 : v;
  }
  const int ty = (H + GA_TILE - 1) / GA_TILE, tx = (W + GA_TILE - 1) / GA_TILE;
  for (int a = 0; a < ty; ++a)
    for (int b = 0; b < tx; ++b) {
      Fenced lds(GA_LDS_BYTES, POISON);
      const GaTile t = ga_make_tile(code, allow, H, W, a, b);
      if (t.sy0 < 0 || t.sx0 < 0 || t.sy0 + t.srows > H ||
          t.sx0 + t.scols > W || t.sx0 % 8 || t.scols % 8 || t.tw % 8 ||
          t.srows > GA_TILE || t.scols > GA_TILE) {
        printf("bad source rectangle H%d W%d code%d tile %d,%d\n", H, W,
               code, a, b);
        return 1;
      }
      for (int tid = 0; tid < GA_THREADS; ++tid)
        ga_load_tile(t, tid, W, src.data(), lds.data());
      for (int tid = 0; tid < GA_THREADS; ++tid)
        ga_store_tile(t, tid, W, lds.data(), dst.data());
      if (!lds.intact()) {
        printf("LDS overrun H%d W%d code%d\n", H, W, code);
        return 1;
      }
    }
  if (!src.intact() || !dst.intact()) {
    printf("image overrun H%d W%d code%d\n", H, W, code);
    return 1;
  }
  for (int oy = 0; oy < H; ++oy)
    for (int ox = 0; ox < W; ++ox) {
      int y, x;
      ref_map(code, allow, H, W, oy, ox, y, x);
      for (int c = 0; c < 3; ++c)
        if (dst.data()[((size_t)oy * W + ox) * 3 + c] !=
            src.data()[((size_t)y * W + x) * 3 + c]) {
          printf("mismatch H%d W%d code%d allow%d at (%d,%d,%d)\n", H, W,
                 code, (int)allow, oy, ox, c);
          return 1;
        }
    }
  return 0;
}
}  // namespace

int main() {
  const int shapes[][2] = {{8, 8},   {40, 40},   {24, 56}, {64, 64},
                           {112, 112}, {16, 72}, {96, 32}, {8, 40},
                           {256, 256}, {104, 104}};
  long cases = 0;
  for (auto& s : shapes)
    for (int allow = 0; allow < 2; ++allow) {
      if (allow && s[0] != s[1]) continue;
      for (int code = 0; code < 16; ++code, ++cases)
        if (check(s[0], s[1], code, allow)) return 1;
    }
  printf("OK %ld cases\n", cases);
  return 0;
}
