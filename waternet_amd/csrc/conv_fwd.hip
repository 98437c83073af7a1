// MFMA implicit-GEMM convolution engine for gfx950 (CDNA4).
//
// Replaces the reference's implicit cuDNN conv launches (SURVEY §2.2
// K2-K9, K12-K14, K17) with hand-written NHWC bf16 kernels:
//   - k_conv_igemm<BN,KS,SPLITK>: stride-1 same-pad conv fwd as implicit
//     GEMM (M = N*H*W rows, N = output channels, K = R*S*Cp) on
//     v_mfma_f32_16x16x32_bf16 with fused bias + ReLU/Sigmoid epilogue and
//     global_load_lds staging; SPLITK slices the K loop over gridDim.z into
//     fp32 slabs (3-deep LDS ring, counted vmcnt) for small-M shapes.
//     Also runs dgrad (conv of dY with rotated/transposed packed weights).
//   - k_conv_igemm8<BN,KS>: 8-wave 256-row phase-split variant for big-M
//     shapes (setprio-wrapped MFMA phases, counted vmcnt).
//   - k_conv_patch<KS,BN,CC>: big-M k3/k5/k7 layers with 64/128 channels and
//     H, W multiples of 16: a 16x16 output-pixel tile per block, the input
//     patch staged into LDS once and the taps taken by shifted reads.
//   - k_conv_tile<CC,IMG7,SLAB>: the deep k3 layers (Cp 128..512 on 56^2 ..
//     7^2 images): a 14x14 output-pixel tile (or four 7x7 images) and one
//     CC-channel chunk of the input patch resident per block, chunks summed
//     through the split-K slabs.
//   - k_splitk_finalize<GZ>: sums the split-K slabs, bias + activation.
// The weight-gradient kernels are in conv_wgrad.hip, weight packing in
// conv_pack.hip; conv_common.h has the notes and host helpers they share.
//
// Design notes (MI355X):
//   - igemm LDS tiles are FRAGMENT-MAJOR: slot (mf, kb, i) holds the 8
//     bf16 the MFMA lane (kb,i) consumes, so the lane-linear glds image and
//     ds_read_b128 fragment loads are bank-conflict-free without swizzles.

#include "conv_common.h"

// ---------------------------------------------------------------------------
// Pieces shared by the igemm tiers: tile geometry, staging sources, counted
// waits and the epilogue. A new tier takes its constants from a Geo struct
// (the launch takes LDS_BYTES from the same struct) and stores through
// store_tile.
// ---------------------------------------------------------------------------

// k_conv_igemm: 4 waves, 128 x BN tile.
template <int BN, bool SPLITK>
struct IgemmGeo {
  static constexpr int THREADS = 256;
  static constexpr int BM = 128;
  static constexpr int WM = (BN >= 64) ? 2 : 4, WN = 4 / WM;  // wave grid
  static constexpr int FM = BM / WM / 16;  // fragments per wave in M
  static constexpr int FN = BN / WN / 16;  // fragments per wave in N
  static constexpr int ASLOT = BM * 32 / 8 / THREADS;  // A slots per thread
  static constexpr int SLOTS_B = BN * 4;
  static constexpr int NBS = (SLOTS_B + 255) / 256;  // B slots per thread
  static constexpr int LA = BM * 32;        // A buffer elems
  static constexpr int LB = NBS * 256 * 8;  // B buffer elems (>= SLOTS_B*8, so
                                            // the glds of invalid slots lands
                                            // in-pad)
  // SPLITK uses a 5-deep buffer ring; the 2-phase path uses 2 stage buffers
  // of DK 32-K steps each (DK=2 for the narrow tiles).
  static constexpr int DK = (BN <= 32) ? 2 : 1;
  static constexpr int NBUF = SPLITK ? 5 : 2 * DK;
  static constexpr int GPS = ASLOT + NBS;  // glds per stage per thread
  static constexpr int LDS_BYTES = NBUF * (LA + LB) * (int)sizeof(bf16_t);
};

// k_conv_igemm8: 8 waves as 4(M) x 2(N), 256 x BN tile.
template <int BN, int VAR>
struct Igemm8Geo {
  static constexpr int THREADS = 512;
  static constexpr int BM = 256;
  static constexpr int WMW = 4, WNW = 2;  // wave grid
  static constexpr int FM = BM / WMW / 16, FN = BN / WNW / 16;
  static constexpr int FM32 = BM / WMW / 32, FN32 = BN / WNW / 32;
  static constexpr int ASLOT = BM * 32 / 8 / THREADS;  // = 2
  static constexpr int SLOTS_B = BN * 4;
  static constexpr int BSLOT = (SLOTS_B + 511) / 512;  // = 1
  static constexpr int LA = BM * 32;   // A buffer elems
  static constexpr int LB = 512 * 8;   // B buffer elems (>= SLOTS_B*8)
  static constexpr int RING = (VAR == 3) ? 4 : 3;
  static constexpr int AHEAD = RING - 2;  // tiles left in flight at the wait
  static constexpr int GPS = ASLOT + BSLOT;  // glds per stage per thread
  static constexpr bool PRIO = (VAR != 1);
  static constexpr int NPH = (VAR == 2) ? 4 : 2;  // M phases per K-step
  static constexpr int LDS_BYTES = RING * (LA + LB) * (int)sizeof(bf16_t);
};

// The lane-linear LDS image IS the fragment layout, so the slot -> (tile
// row, k offset) decode differs per MFMA shape (A and B alike):
//   16x16x32: slot = (f16, kb, i16) -> row = f16*16+i16, kOff = kb*8
//   32x32x16: slot = (f32, t, g, i32) -> row = f32*32+i32,
//             kOff = t*16 + g*8  (lane l reads k = (l>>5)*8+e)
struct FragSlot { int row, koff; };
template <bool M32>
WN_DEVFN FragSlot frag_slot(int slot) {
  if constexpr (M32)
    return {(slot >> 7) * 32 + (slot & 31),
            ((slot >> 6) & 1) * 16 + ((slot >> 5) & 1) * 8};
  else
    return {(slot >> 6) * 16 + (slot & 15), ((slot >> 4) & 3) * 8};
}

// Output pixel of GEMM row m: (n*H, oy, ox); rows past M are not valid.
struct ConvPixel {
  long rowBase;
  int oy, ox;
  bool valid;
};
WN_DEVFN ConvPixel conv_pixel(long m, long M, int H, int W, int HW) {
  ConvPixel p;
  p.valid = m < M;
  long mm = p.valid ? m : 0;
  int n = (int)(mm / HW);
  int rem = (int)(mm - (long)n * HW);
  p.oy = rem / W;
  p.ox = rem - p.oy * W;
  p.rowBase = (long)n * H;
  return p;
}

// glds source of the 8 A elements at reduction index rsc = (tap, c) of pixel
// p: inside X, or Zero16 for the conv halo, the K tail and the M tail.
template <int KS>
WN_DEVFN const bf16_t* conv_a_src(const bf16_t* X, const bf16_t* Zero16,
                                  ConvPixel p, int rsc, int KG, int H, int W,
                                  int Cp, int log2Cp) {
  constexpr int PAD = KS / 2;
  const bf16_t* src = Zero16;
  if (p.valid && rsc < KG) {
    int tap = rsc >> log2Cp;
    int c = rsc & (Cp - 1);
    int dy = tap / KS, dx = tap - (tap / KS) * KS;
    int iy = p.oy + dy - PAD, ix = p.ox + dx - PAD;
    if (iy >= 0 && iy < H && ix >= 0 && ix < W)
      src = X + (((p.rowBase + iy) * W + ix) << log2Cp) + c;
  }
  return src;
}

// B-side counterpart: 8 packed weights of output channel k at rsc, or Zero16
// for slots past the tile, pad rows of Wp and the K tail.
WN_DEVFN const bf16_t* conv_b_src(const bf16_t* Wp, const bf16_t* Zero16,
                                  bool slotValid, int k, int rsc, int Kp,
                                  int KG) {
  const bf16_t* src = Zero16;
  if (slotValid && k < Kp && rsc < KG) src = Wp + (long)k * KG + rsc;
  return src;
}

// One lane's 16 B global -> LDS DMA.
WN_DEVFN void glds16(const bf16_t* src, bf16_t* dst) {
  __builtin_amdgcn_global_load_lds(src, dst, 16, 0, 0);
}

// Wait until at most `tiles` (<= MAXT) staged tiles of GPS glds per thread
// each remain outstanding.
template <int GPS, int MAXT>
WN_DEVFN void wait_tiles(int tiles) {
  if constexpr (MAXT > 0) {
    if (tiles >= MAXT)
      wait_vmcnt<MAXT * GPS>();
    else
      wait_tiles<GPS, MAXT - 1>(tiles);
  } else {
    wait_vmcnt<0>();
  }
}

// Epilogue value: bias + activation, pad channels forced to zero.
WN_DEVFN float bias_act(float v, float bv, bool kpad, int act) {
  v += bv;
  if (act == ACT_RELU) v = fmaxf(v, 0.f);
  else if (act == ACT_SIGMOID) v = 1.f / (1.f + __expf(-v));
  if (kpad) v = 0.f;
  return v;
}

// Where a tile goes. SLAB (split-K slice): plain fp32 stores into this
// slice's slab of Y32 (no atomics — the finalize pass reduces over gridDim.z
// slabs). Y32 is NOT pre-zeroed (at::empty): every slice block fully stores
// its m<M rows, and finalize only reads i < M*Kp — an epilogue edit that
// skips stores must zero-fill first. Otherwise bf16 bias_act() into Y.
struct ConvOut {
  const float* Bias;  // [>=Klog] or nullptr
  bf16_t* Y;          // (M, Kp)
  float* Y32;         // [gridDim.z][M][Kp]
  long M;
  int Kp, Klog, act;
};
template <bool SLAB>
WN_DEVFN void store_out(const ConvOut& o, long m, int k, float v, float bv,
                        bool kpad) {
  if constexpr (SLAB)
    o.Y32[((long)blockIdx.z * o.M + m) * o.Kp + k] = v;
  else
    o.Y[m * o.Kp + k] = f2bf(bias_act(v, bv, kpad, o.act));
}

// A wave's FM x FN accumulators of FR x FR outputs (16: f32x4, 32: f32x16)
// whose first row / column are m0 + rW / kW (m0 stays apart so the row
// offset is summed in 32 bits). D map of both MFMA shapes: col = lane % FR,
// row = (r&3) + 8*(r>>2) + 4*(lane/FR) — for 16x16 that is lg*4 + r, li.
// The row map turns a tile row into the GEMM row m it is stored at: GemmRows
// for tiles of consecutive GEMM rows, PixelTileRows (k_conv_patch) for a
// TW-wide tile of output pixels.
struct GemmRows {
  long m0;
  WN_DEVFN long operator()(int r) const { return m0 + r; }
};
template <bool SLAB, int FR, class Acc, int FM, int FN, class RowMap>
WN_DEVFN void store_tile(const Acc (&acc)[FM][FN], const RowMap& rows, int rW,
                         int kW, int lane, const ConvOut& o) {
#pragma unroll
  for (int fn = 0; fn < FN; ++fn) {
    const int k = kW + fn * FR + (lane & (FR - 1));
    if (k >= o.Kp) continue;
    const float bv = (o.Bias != nullptr && k < o.Klog) ? o.Bias[k] : 0.f;
    const bool kpad = k >= o.Klog;
#pragma unroll
    for (int fm = 0; fm < FM; ++fm) {
#pragma unroll
      for (int r = 0; r < FR * FR / 64; ++r) {
        const int row = (r & 3) + 8 * (r >> 2) + 4 * (lane / FR);
        long m = rows(rW + fm * FR + row);
        if (m >= o.M) continue;
        store_out<SLAB>(o, m, k, acc[fm][fn][r], bv, kpad);
      }
    }
  }
}
template <bool SLAB, int FR, class Acc, int FM, int FN>
WN_DEVFN void store_tile(const Acc (&acc)[FM][FN], long m0, int rW, int kW,
                         int lane, const ConvOut& o) {
  store_tile<SLAB, FR>(acc, GemmRows{m0}, rW, kW, lane, o);
}

// ---------------------------------------------------------------------------
// Forward / dgrad implicit GEMM
// ---------------------------------------------------------------------------

template <int BN, int KS, bool SPLITK = false>
__global__ __launch_bounds__(256, 2) void k_conv_igemm(
    const bf16_t* __restrict__ X,   // (N, H, W, Cp)
    const bf16_t* __restrict__ Wp,  // [Kp][RS*Cp] k-major packed
    const float* __restrict__ Bias, // [>=Klog] or nullptr
    bf16_t* __restrict__ Y,         // (N, H, W, Kp)
    int N, int H, int W, int Cp, int log2Cp, int Kp, int Klog, int act,
    const bf16_t* __restrict__ Zero16,    // 16 B of zeros (halo/pad source)
    float* __restrict__ Y32 = nullptr) {  // SPLITK: fp32 partial slabs
                                          // (contract: see ConvOut)
  using G = IgemmGeo<BN, SPLITK>;
  constexpr int BM = G::BM, WN = G::WN, FM = G::FM, FN = G::FN;
  constexpr int ASLOT = G::ASLOT, NBS = G::NBS, LA = G::LA, LB = G::LB;
  constexpr int THREADS = G::THREADS;  // local: see k_conv_igemm8
  const int KG = KS * KS * Cp;
  const long M = (long)N * H * W;

  extern __shared__ __attribute__((aligned(16))) char smem[];
  bf16_t* lA = reinterpret_cast<bf16_t*>(smem);  // NBUF x LA
  bf16_t* lB = lA + G::NBUF * LA;                // NBUF x LB

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wid = tid >> 6;
  const int wr = wid / WN;
  const int wc = wid % WN;
  const long m0 = (long)blockIdx.x * BM;
  const int n0 = blockIdx.y * BN;

  // ---- per-thread A / B slot geometry ----
  ConvPixel aPx[ASLOT];
  int aKo[ASLOT], bK[NBS], bKo[NBS];
  bool bV[NBS];
  const int HW = H * W;
#pragma unroll
  for (int s = 0; s < ASLOT; ++s) {
    const FragSlot f = frag_slot<false>(tid + s * THREADS);
    aPx[s] = conv_pixel(m0 + f.row, M, H, W, HW);
    aKo[s] = f.koff;
  }
#pragma unroll
  for (int s = 0; s < NBS; ++s) {
    const FragSlot f = frag_slot<false>(tid + s * THREADS);
    bV[s] = tid + s * THREADS < G::SLOTS_B;
    bK[s] = n0 + f.row;
    bKo[s] = f.koff;
  }

  static_assert(WN_MFMA_KMAP == 0, "glds staging assumes KMAP 0");

  // Stage one K-step's A and B tiles straight into LDS buffer `buf` with
  // global_load_lds (16 B per lane, lane-linear LDS image — guide §5
  // "common mistake 1": width-16 glds is the staging lever). Out-of-range
  // lanes (conv halo, channel pad, M tail) read from Zero16 instead —
  // every lane always issues its DMA so the image is fully defined.
  auto stage = [&](int buf, int k0) {
#pragma unroll
    for (int s = 0; s < ASLOT; ++s)
      glds16(conv_a_src<KS>(X, Zero16, aPx[s], k0 + aKo[s], KG, H, W, Cp,
                            log2Cp),
             lA + buf * LA + (tid + s * THREADS) * 8);
#pragma unroll
    for (int s = 0; s < NBS; ++s)
      glds16(conv_b_src(Wp, Zero16, bV[s], bK[s], k0 + bKo[s], Kp, KG),
             lB + buf * LB + (tid + s * THREADS) * 8);
  };

  f32x4 acc[FM][FN];
#pragma unroll
  for (int a = 0; a < FM; ++a)
#pragma unroll
    for (int b = 0; b < FN; ++b) acc[a][b] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int nkAll = (KG + 31) / 32;
  // SPLITK: z-slice [ks0, nk) of the K loop; else the whole range. Floor
  // slicing keeps every slice non-empty for gz <= nkAll, so every fp32
  // slab is fully written (the finalize pass sums all of them).
  int ks0 = 0, nk = nkAll;
  if (SPLITK) {
    ks0 = (int)((long)blockIdx.z * nkAll / gridDim.z);
    nk = (int)((long)(blockIdx.z + 1) * nkAll / gridDim.z);
  }
  const int lg = lane >> 4;   // fragment k-group
  const int li = lane & 15;   // fragment row/col

  if constexpr (SPLITK) {
    // Split-K shapes run at ~1 block/CU (small M, chip filled by K
    // slices): the per-step vmcnt(0) drain is fully exposed there, so use
    // a 3-buffer glds pipeline with COUNTED vmcnt + raw barriers (guide
    // §5 "Pipelining across barriers": +40-83% in the 1-block/CU regime;
    // measured NEGATIVE at the big-M shapes' 5-blocks/CU occupancy, which
    // keep the simpler 2-phase below).
    // every stage() issues exactly GPS glds per thread (3 or 4), which the
    // counted waits below multiply out
    static_assert(G::GPS == 2 + NBS && (G::GPS == 3 || G::GPS == 4));
    // prologue: up to 4 tiles in flight, wait for tile ks0 only
    for (int t = 0; t < 4 && ks0 + t < nk; ++t) stage(t, (ks0 + t) * 32);
    wait_tiles<G::GPS, 3>(min(nk - ks0 - 1, 3));
    __builtin_amdgcn_s_barrier();
    for (int ks = ks0; ks < nk; ++ks) {
      const int b = (ks - ks0) % 5;
      if (ks + 4 < nk) stage((b + 4) % 5, (ks + 4) * 32);
      bf16x8 aF[FM], bF[FN];
#pragma unroll
      for (int fm = 0; fm < FM; ++fm)
        aF[fm] = *reinterpret_cast<const bf16x8*>(
            lA + b * LA + (((wr * FM + fm) * 4 + lg) * 16 + li) * 8);
#pragma unroll
      for (int fn = 0; fn < FN; ++fn)
        bF[fn] = *reinterpret_cast<const bf16x8*>(
            lB + b * LB + (((wc * FN + fn) * 4 + lg) * 16 + li) * 8);
#pragma unroll
      for (int fm = 0; fm < FM; ++fm)
#pragma unroll
        for (int fn = 0; fn < FN; ++fn)
          acc[fm][fn] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              aF[fm], bF[fn], acc[fm][fn], 0, 0, 0);
      if (ks + 1 < nk) {
        wait_tiles<G::GPS, 3>(min(nk - ks - 2, 3));  // tile ks+1 landed
        __builtin_amdgcn_s_barrier();
      }
    }
  } else {
    // 2-phase glds pipeline (guide §5 "minimum 2-phase"): issue next
    // tile's DMA first, ds_read + MFMA the current buffer, one
    // vmcnt(0)+barrier per staged tile (the __syncthreads drains the DMA).
    // Narrow tiles (BN<=32) do only FM*FN<=4 MFMAs per 32-K step, so they
    // stage DK=2 steps per barrier to amortize it (K tails are zero-filled
    // by the staging, so no edge code).
    constexpr int DK = G::DK;
#pragma unroll
    for (int h = 0; h < DK; ++h) stage(h, (ks0 + h) * 32);
    __syncthreads();
    int cur = 0;
    const int nk2 = (nk - ks0 + DK - 1) / DK;
    for (int ks2 = 0; ks2 < nk2; ++ks2) {
      if (ks2 + 1 < nk2) {
#pragma unroll
        for (int h = 0; h < DK; ++h)
          stage((cur ^ 1) * DK + h, (ks0 + (ks2 + 1) * DK + h) * 32);
      }
#pragma unroll
      for (int h = 0; h < DK; ++h) {
        bf16x8 aF[FM], bF[FN];
#pragma unroll
        for (int fm = 0; fm < FM; ++fm) {
          int mfG = wr * FM + fm;
          aF[fm] = *reinterpret_cast<const bf16x8*>(
              lA + (cur * DK + h) * LA +
              ((mfG * 4 + lg) * 16 + li) * 8);
        }
#pragma unroll
        for (int fn = 0; fn < FN; ++fn) {
          int nfG = wc * FN + fn;
          bF[fn] = *reinterpret_cast<const bf16x8*>(
              lB + (cur * DK + h) * LB + ((nfG * 4 + lg) * 16 + li) * 8);
        }
#pragma unroll
        for (int fm = 0; fm < FM; ++fm)
#pragma unroll
          for (int fn = 0; fn < FN; ++fn)
            acc[fm][fn] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                aF[fm], bF[fn], acc[fm][fn], 0, 0, 0);
      }
      if (ks2 + 1 < nk2) __syncthreads();
      cur ^= 1;
    }
  }

  // ---- epilogue: bias + activation (+ pad-channel zeroing), or this
  //      slice's fp32 slab when the launch is a split-K slice ----
  store_tile<SPLITK, 16>(acc, m0, wr * FM * 16, n0 + wc * FN * 16, lane,
                         ConvOut{Bias, Y, Y32, M, Kp, Klog, act});
}

// ---------------------------------------------------------------------------
// 8-wave 256xBN phase-split conv igemm for BIG-M shapes (guide §5 T3+T5:
// wave role diversity + setprio + counted vmcnt; the 4-wave 2-phase kernel
// above is schedule-bound at ~480 TF on these shapes — PMC r06/r18: ~58%
// WAIT_ANY with MFMA, TA and HBM all unsaturated).
//   - 512 threads = 8 waves as 4(M)x2(N); per-wave output 64 x BN/2.
//   - 3-deep LDS ring, glds staging (GPS=3 per thread per tile), counted
//     s_waitcnt vmcnt leaves the next tile's DMA in flight across barriers.
//   - two MFMA phases per K-step with s_setprio(1) around the matrix math.
// ---------------------------------------------------------------------------

// VAR: 0 = 2 setprio phases / 3-ring (default); 1 = no setprio;
// 2 = 4 phases; 3 = 4-deep ring (2 tiles in flight). Runtime-selectable
// via WN_IGEMM8_VAR for within-box A/B (guide §5.4 rule 24).
// M32: v_mfma_f32_32x32x16_bf16 fragments (half the MFMA instruction
// count at the higher 32x32 pipe rate; +5.5% proven on the wgrad).
template <int BN, int KS, int VAR = 0, bool M32 = false>
__global__ __launch_bounds__(512, 1) void k_conv_igemm8(
    const bf16_t* __restrict__ X,   // (N, H, W, Cp)
    const bf16_t* __restrict__ Wp,  // [Kp][RS*Cp]
    const float* __restrict__ Bias,
    bf16_t* __restrict__ Y,         // (N, H, W, Kp)
    int N, int H, int W, int Cp, int log2Cp, int Kp, int Klog, int act,
    const bf16_t* __restrict__ Zero16) {
  static_assert(WN_MFMA_KMAP == 0, "glds staging assumes KMAP 0");
  using G = Igemm8Geo<BN, VAR>;
  constexpr int BM = G::BM;
  constexpr int FM = G::FM;  // 4 fragments in M per wave
  constexpr int FN = G::FN;  // 4 (BN=128) / 2 (BN=64)
  constexpr int ASLOT = G::ASLOT, BSLOT = G::BSLOT;
  constexpr int LA = G::LA, LB8 = G::LB, RING = G::RING;
  // a local copy: the staging lambda must not name G (hipcc then drops the
  // kernel's host stub without a diagnostic)
  constexpr int THREADS = G::THREADS;
  const int KG = KS * KS * Cp;
  const long M = (long)N * H * W;

  extern __shared__ __attribute__((aligned(16))) char smem[];
  // the B buffers start after RING A buffers
  bf16_t* lA = reinterpret_cast<bf16_t*>(smem);   // RING x LA
  bf16_t* lB = lA + RING * LA;                    // RING x LB8

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wid = tid >> 6;
  const int wr = wid >> 1;
  const int wc = wid & 1;
  const long m0 = (long)blockIdx.x * BM;
  const int n0 = blockIdx.y * BN;
  const int HW = H * W;

  // per-thread A / B slot geometry (decode: frag_slot)
  ConvPixel aPx[ASLOT];
  int aKo[ASLOT], bK[BSLOT], bKo[BSLOT];
  bool bV[BSLOT];
#pragma unroll
  for (int s = 0; s < ASLOT; ++s) {
    const FragSlot f = frag_slot<M32>(tid + s * THREADS);
    aPx[s] = conv_pixel(m0 + f.row, M, H, W, HW);
    aKo[s] = f.koff;
  }
#pragma unroll
  for (int s = 0; s < BSLOT; ++s) {
    const FragSlot f = frag_slot<M32>(tid + s * THREADS);
    bV[s] = tid + s * THREADS < G::SLOTS_B;
    bK[s] = n0 + f.row;
    bKo[s] = f.koff;
  }

  // as k_conv_igemm's: every lane issues every DMA
  auto stage = [&](int buf, int ks) {
    const int k0 = ks * 32;
#pragma unroll
    for (int s = 0; s < ASLOT; ++s)
      glds16(conv_a_src<KS>(X, Zero16, aPx[s], k0 + aKo[s], KG, H, W, Cp,
                            log2Cp),
             lA + buf * LA + (tid + s * THREADS) * 8);
#pragma unroll
    for (int s = 0; s < BSLOT; ++s)
      glds16(conv_b_src(Wp, Zero16, bV[s], bK[s], k0 + bKo[s], Kp, KG),
             lB + buf * LB8 + (tid + s * THREADS) * 8);
  };

  constexpr int FM32 = G::FM32;  // 2
  constexpr int FN32 = G::FN32;  // 2 (BN=128) / 1 (BN=64)
  f32x4 acc[M32 ? 1 : FM][M32 ? 1 : FN];
  f32x16 acc32[M32 ? FM32 : 1][M32 ? FN32 : 1];
#pragma unroll
  for (int a = 0; a < (M32 ? FM32 : FM); ++a)
#pragma unroll
    for (int b = 0; b < (M32 ? FN32 : FN); ++b) {
      if constexpr (M32) {
#pragma unroll
        for (int e = 0; e < 16; ++e) acc32[a][b][e] = 0.f;
      } else {
        acc[a][b] = f32x4{0.f, 0.f, 0.f, 0.f};
      }
    }

  const int nk = (KG + 31) / 32;
  const int lg = lane >> 4, li = lane & 15;
  constexpr int AHEAD = G::AHEAD;  // tiles left in flight at the wait
  constexpr bool PRIO = G::PRIO;
  constexpr int NPH = G::NPH;  // M-fragment phases per K-step
  static_assert(G::GPS == 3, "stage() issues 3 glds per thread");

  for (int t = 0; t < RING - 1 && t < nk; ++t) stage(t, t);
  wait_tiles<G::GPS, AHEAD>(min(nk - 1, RING - 2));
  __builtin_amdgcn_s_barrier();

  for (int ks = 0; ks < nk; ++ks) {
    const int b = ks % RING;
    if (ks + RING - 1 < nk) stage((b + RING - 1) % RING, ks + RING - 1);
    if constexpr (M32) {
      // lane-linear fragment reads: block (mf32*2+t)*2+g at lane*16B
      bf16x8 aF[FM32][2], bF[FN32][2];
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int fn = 0; fn < FN32; ++fn)
          bF[fn][t] = *reinterpret_cast<const bf16x8*>(
              lB + b * LB8 + ((wc * FN32 + fn) * 2 + t) * 512 + lane * 8);
#pragma unroll
      for (int ph = 0; ph < 2; ++ph) {  // one M fragment per phase
#pragma unroll
        for (int t = 0; t < 2; ++t)
          aF[ph][t] = *reinterpret_cast<const bf16x8*>(
              lA + b * LA + ((wr * FM32 + ph) * 2 + t) * 512 + lane * 8);
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_sched_barrier(0);
        if constexpr (PRIO) __builtin_amdgcn_s_setprio(1);
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
          for (int fn = 0; fn < FN32; ++fn)
            acc32[ph][fn] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
                aF[ph][t], bF[fn][t], acc32[ph][fn], 0, 0, 0);
        if constexpr (PRIO) __builtin_amdgcn_s_setprio(0);
      }
    } else {
      bf16x8 aF[FM], bF[FN];
#pragma unroll
      for (int fn = 0; fn < FN; ++fn)
        bF[fn] = *reinterpret_cast<const bf16x8*>(
            lB + b * LB8 + (((wc * FN + fn) * 4 + lg) * 16 + li) * 8);
#pragma unroll
      for (int ph = 0; ph < NPH; ++ph) {
        constexpr int FPP = M32 ? 1 : FM / NPH;  // fragments per phase
#pragma unroll
        for (int fm = ph * FPP; fm < (ph + 1) * FPP; ++fm)
          aF[fm] = *reinterpret_cast<const bf16x8*>(
              lA + b * LA + (((wr * FM + fm) * 4 + lg) * 16 + li) * 8);
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_sched_barrier(0);
        if constexpr (PRIO) __builtin_amdgcn_s_setprio(1);
#pragma unroll
        for (int fm = ph * FPP; fm < (ph + 1) * FPP; ++fm)
#pragma unroll
          for (int fn = 0; fn < FN; ++fn)
            acc[fm][fn] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                aF[fm], bF[fn], acc[fm][fn], 0, 0, 0);
        if constexpr (PRIO) __builtin_amdgcn_s_setprio(0);
      }
    }
    if (ks + 1 < nk) {
      wait_tiles<G::GPS, AHEAD>(min(nk - ks - 2, AHEAD));
      __builtin_amdgcn_s_barrier();
    }
  }

  // epilogue: bias + activation + pad zeroing; the wave tile is 64 x BN/2
  const ConvOut out{Bias, Y, nullptr, M, Kp, Klog, act};
  const int rW = wr * (BM / G::WMW);
  const int kW = n0 + wc * (BN / G::WNW);
  if constexpr (M32)
    store_tile<false, 32>(acc32, m0, rW, kW, lane, out);
  else
    store_tile<false, 16>(acc, m0, rW, kW, lane, out);
}

// ---------------------------------------------------------------------------
// Patch-staged conv for big-M k3/k5/k7 layers with 64 / 128 channels.
// k_conv_igemm8 streams a fresh 256x32 A tile through the LDS DMA for every
// tap: an input pixel lands in LDS KS^2 times. Here a block owns a 16x16
// tile of output pixels of one image and stages the (16+KS-1)^2 input patch
// ONCE, all CC = Cp channels of it, as plain [pixel][CC] rows; the A fragment
// of tap (dy, dx) is the tap-0 read with every lane moved by dy*PW + dx
// pixel rows (A is K-contiguous, so plain ds_read_b128, no transpose read).
//   - 512 threads = 8 waves as 4(M)x2(N): a wave owns 4 output rows of the
//     tile (4 fragments of 16 pixels) x BN/2 channels, 16x16x32 MFMA.
//   - K order: the igemm's own rsc = tap*Cp + c in 32-wide steps, so the
//     sums are those of k_conv_igemm8 bit for bit. (Staging Cp = 128 as two
//     64-channel chunks would halve the patch and keep two blocks per CU,
//     but makes the order chunk-major: different fp32 rounding.)
//   - B (packed weights) goes through a 3-deep fragment-major ring exactly
//     as in k_conv_igemm8 (counted vmcnt, one tile in flight at a barrier);
//     only the waves whose slots are inside the BN x 32 tile issue.
//   - patch image: 128- or 256-byte pixel rows. A fragment read takes 16
//     consecutive pixels x one 16 B chunk per 16-lane MFMA k-group;
//     ds_read_b128 serves lanes in the groups {0-3,12-15,20-27},
//     {4-11,16-19,28-31} (+32), i.e. two neighbouring chunks c, c^1 of
//     interleaved pixel runs. The chunk index is XORed above its bit 0 with
//     pixel bits (CC=64: pixel bits 1-2, CC=128: bits 0-2), which puts the 16
//     lanes of a group on the 16 distinct 16 B columns of the 256 B bank row
//     at every pixel shift (cp_frag_conflict_free). The XOR moves whole
//     chunks, so the glds image stays lane-linear with the swizzle on the
//     SOURCE chunk.
// ---------------------------------------------------------------------------

// chunk-index XOR of a patch pixel row (slot map: PatchImage, conv_common.h)
struct CpSwz {
  static constexpr int chunk_xor(int pix, int CC) {
    return CC == 64 ? ((pix >> 1) & 3) << 1 : (pix & 7) << 1;
  }
};
using CpImage = PatchImage<CpSwz>;
// the 16x16x32 A fragment read (lane = kgroup*16 + pixel, chunk = kb*4 +
// kgroup) is conflict-free in each ds_read_b128 lane group at every shift
constexpr bool cp_frag_conflict_free(int CC) {
  for (int sh = 0; sh < 16; ++sh)
    for (int kb = 0; kb < CC / 32; ++kb)
      for (int g = 0; g < 4; ++g) {
        unsigned used = 0;
        for (int l = 0; l < 64; ++l) {
          const int m = l & 31;
          const bool first =
              m < 4 || (m >= 12 && m < 16) || (m >= 20 && m < 28);
          if ((l >> 5) * 2 + (first ? 0 : 1) != g) continue;
          const int a = CpImage::off(sh + (l & 15), kb * 4 + (l >> 4), CC);
          const unsigned bit = 1u << ((a / 16) % 16);
          if (used & bit) return false;
          used |= bit;
        }
        if (used != 0xffffu) return false;
      }
  return true;
}

template <int KS, int BN, int CC>
struct ConvPatchGeo {
  static constexpr int THREADS = 512;
  static constexpr int TH = 16, TW = 16, BM = TH * TW;  // output pixel tile
  static constexpr int PAD = KS / 2;
  static constexpr int PH = TH + KS - 1, PW = TW + KS - 1, NPX = PH * PW;
  static constexpr int PSLOTS = NPX * (CC / 8);
  // wave-wide glds instructions (1 KiB each) that cover the patch; the
  // surplus lanes of the last one land inside PBYTES
  static constexpr int PINSTR = (PSLOTS + 63) / 64;
  static constexpr int PBYTES = PINSTR * 1024;
  static constexpr int SP = (PINSTR * 64 + THREADS - 1) / THREADS;
  static constexpr int WMW = 4, WNW = 2;  // wave grid
  static constexpr int FM = BM / WMW / 16, FN = BN / WNW / 16;
  static constexpr int SLOTS_B = BN * 4;
  static constexpr int LB = BN * 32;  // B tile elems (32 K)
  static constexpr int RING = 3;
  static constexpr int AHEAD = RING - 2;  // B tiles in flight at the wait
  static constexpr int KB = CC / 32;      // K-steps per tap
  static constexpr int LDS_BYTES = PBYTES + RING * LB * (int)sizeof(bf16_t);
  static_assert(LDS_BYTES <= 160 * 1024);
  // resident blocks per CU by the 160 KiB of LDS (2 for CC = 64, 1 for
  // CC = 128); the launch bounds ask for 2 waves per SIMD per block
  static constexpr int BLOCKS_PER_CU = LDS_BYTES <= 80 * 1024 ? 2 : 1;
};

// tile row r = py*TW + px of the block's output tile -> GEMM row
struct PixelTileRows {
  long m00;  // GEMM row of the tile's first pixel
  int W;
  WN_DEVFN long operator()(int r) const {
    return m00 + (long)(r >> 4) * W + (r & 15);
  }
};

template <int KS, int BN, int CC>
__global__ __launch_bounds__(
    512, (2 * ConvPatchGeo<KS, BN, CC>::BLOCKS_PER_CU)) void k_conv_patch(
    const bf16_t* __restrict__ X,   // (N, H, W, Cp), Cp == CC
    const bf16_t* __restrict__ Wp,  // [Kp][RS*Cp]
    const float* __restrict__ Bias,
    bf16_t* __restrict__ Y,         // (N, H, W, Kp); H % 16 == W % 16 == 0
    int N, int H, int W, int Cp, int log2Cp, int Kp, int Klog, int act,
    const bf16_t* __restrict__ Zero16) {
  static_assert(WN_MFMA_KMAP == 0, "glds staging assumes KMAP 0");
  using G = ConvPatchGeo<KS, BN, CC>;
  constexpr int PAD = G::PAD, PW = G::PW, NPX = G::NPX, SP = G::SP;
  constexpr int FM = G::FM, FN = G::FN, LB = G::LB, RING = G::RING;
  constexpr int AHEAD = G::AHEAD, KB = G::KB;
  constexpr int THREADS = G::THREADS;  // local: see k_conv_igemm8
  static_assert(G::TW == 16 && (CC == 64 || CC == 128) && FM == 4,
                "a fragment is one 16-pixel output row");
  static_assert(CpImage::linear(NPX, CC),
                "glds slot order != image chunk order");
  static_assert(cp_frag_conflict_free(CC), "fragment read bank conflict");
  // the last pixel a fragment read touches is the patch's last; the swizzle
  // stays inside a pixel row
  static_assert((G::TH - 1 + KS - 1) * PW + (G::TW - 1 + KS - 1) == NPX - 1 &&
                NPX * CC * 2 <= G::PBYTES);
  static_assert(G::SLOTS_B % 64 == 0 && G::SLOTS_B <= THREADS,
                "whole waves stage the B tile, one slot per lane");
  constexpr int KG = KS * KS * CC;
  constexpr int nk = KG / 32;
  const long M = (long)N * H * W;

  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* lP = smem;                                           // patch
  bf16_t* lB = reinterpret_cast<bf16_t*>(smem + G::PBYTES);  // RING x LB

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wid = tid >> 6;
  const int wr = wid >> 1;
  const int wc = wid & 1;
  // block-uniform tile decode
  const int tilesX = W / G::TW, tilesY = H / G::TH;
  const int tx = blockIdx.x % tilesX;
  const int ty = (blockIdx.x / tilesX) % tilesY;
  const int n = blockIdx.x / (tilesX * tilesY);
  const int oy0 = ty * G::TH, ox0 = tx * G::TW;
  const int n0 = blockIdx.y * BN;

  // The patch: every lane of every issued wave-wide glds sources either its
  // pixel's (swizzled) 16 B chunk or Zero16 (halo outside the image, surplus
  // slots); whole instructions past the patch are not issued.
#pragma unroll
  for (int s = 0; s < SP; ++s) {
    const int sg = tid + s * THREADS;
    if ((sg >> 6) < G::PINSTR) {  // wave-uniform
      const int pix = CpImage::slot_pix(sg, CC);
      const int py = pix / PW, px = pix - py * PW;
      const int iy = oy0 + py - PAD, ix = ox0 + px - PAD;
      const bf16_t* src = Zero16;
      if (pix < NPX && iy >= 0 && iy < H && ix >= 0 && ix < W)
        src = X + (((long)n * H + iy) * W + ix) * CC +
              CpImage::slot_chunk(sg, CC) * 8;
      glds16(src, reinterpret_cast<bf16_t*>(lP + sg * 16));
    }
  }

  // B tile of K-step g, fragment-major
  const FragSlot bf = frag_slot<false>(tid);
  const bool bIssue = tid < G::SLOTS_B;  // wave-uniform
  auto stage_b = [&](int buf, int g) {
    if (bIssue)
      glds16(conv_b_src(Wp, Zero16, true, n0 + bf.row, g * 32 + bf.koff, Kp,
                        KG),
             lB + buf * LB + tid * 8);
  };

  f32x4 acc[FM][FN];
#pragma unroll
  for (int a = 0; a < FM; ++a)
#pragma unroll
    for (int b = 0; b < FN; ++b) acc[a][b] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int lg = lane >> 4, li = lane & 15;
  // patch pixel of this lane's row of fragment 0 at tap (0, 0)
  const int pix0 = wr * FM * PW + li;

  for (int t = 0; t < RING - 1 && t < nk; ++t) stage_b(t, t);
  wait_vmcnt<0>();
  __builtin_amdgcn_s_barrier();

  int g = 0, tapoff = 0, dx = 0;
  for (int tap = 0; tap < KS * KS; ++tap) {
    // kb = 0 addresses; kb flips chunk bits 2-3 (the swizzle touches the
    // chunk above bit 0 and kgroup < 4), i.e. address bits 6-7
    unsigned aAd[FM];
#pragma unroll
    for (int fm = 0; fm < FM; ++fm) {
      const int pix = pix0 + fm * PW + tapoff;
      aAd[fm] = (unsigned)CpImage::off(pix, lg, CC);
    }
#pragma unroll
    for (int kb = 0; kb < KB; ++kb, ++g) {
      const int b = g % RING;
      if (g + RING - 1 < nk) stage_b((b + RING - 1) % RING, g + RING - 1);
      bf16x8 aF[FM], bF[FN];
#pragma unroll
      for (int fn = 0; fn < FN; ++fn)
        bF[fn] = *reinterpret_cast<const bf16x8*>(
            lB + b * LB + (((wc * FN + fn) * 4 + lg) * 16 + li) * 8);
#pragma unroll
      for (int ph = 0; ph < 2; ++ph) {
#pragma unroll
        for (int fm = ph * 2; fm < ph * 2 + 2; ++fm)
          aF[fm] = *reinterpret_cast<const bf16x8*>(
              lP + (aAd[fm] ^ (unsigned)(kb * 64)));
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_sched_barrier(0);
        __builtin_amdgcn_s_setprio(1);
#pragma unroll
        for (int fm = ph * 2; fm < ph * 2 + 2; ++fm)
#pragma unroll
          for (int fn = 0; fn < FN; ++fn)
            acc[fm][fn] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                aF[fm], bF[fn], acc[fm][fn], 0, 0, 0);
        __builtin_amdgcn_s_setprio(0);
      }
      if (g + 1 < nk) {
        wait_tiles<1, AHEAD>(min(nk - g - 2, AHEAD));
        __builtin_amdgcn_s_barrier();
      }
    }
    if (++dx == KS) {
      dx = 0;
      tapoff += PW - (KS - 1);
    } else {
      ++tapoff;
    }
  }

  // epilogue: the shared bias/activation/pad path over a pixel-tile row map
  const ConvOut out{Bias, Y, nullptr, M, Kp, Klog, act};
  const PixelTileRows rows{((long)n * H + oy0) * W + ox0, W};
  store_tile<false, 16>(acc, rows, wr * (G::BM / G::WMW),
                        n0 + wc * (BN / G::WNW), lane, out);
}

// ---------------------------------------------------------------------------
// Tile-resident conv for the deep k3 layers (Cp 128..512 on 28^2, 14^2, 7^2
// images). The split-K igemm re-stages a 128x32 A tile for each of the 9 taps
// and streams every weight through every block; here a block owns 196 output
// pixels x 128 output channels x one CC-channel chunk of the reduction:
//   - rows: a 14x14 output-pixel tile of one image (14 divides 28, 14, 56),
//     or, for 7x7 images, four whole images of 49 pixels each (their GEMM rows
//     are consecutive). 196 rows = 13 fragments of 16, the last masked past
//     row 195.
//   - A: the 16x16-pixel input patch (or four 9x9 patches) of the chunk is
//     staged ONCE as [pixel][CC] rows; the fragment of tap (dy, dx) is the
//     tap-0 read moved by dy*PW + dx pixel rows, as in k_conv_patch.
//   - B: the fragment-major 3-deep ring of k_conv_patch with 64-K tiles (two
//     32-K sub-tiles per barrier). K order: tap-major, channel inner within
//     the chunk.
//   - reduction over the gz = Cp / CC chunks: gz == 1 writes bf16 through
//     bias_act; gz > 1 writes fp32 slabs that k_splitk_finalize<gz> sums in
//     slab order (no atomics: the bits repeat from call to call). The sums
//     are grouped by chunk, not by contiguous rsc range as in the split-K
//     igemm, so outputs differ from that tier at fp32-rounding level.
//   - 512 threads = 8 waves as 2(M) x 4(N): a wave owns 7 (6 for the second
//     M half) row fragments x 2 channel fragments.
//   - swizzle: 16 consecutive GEMM rows are not 16 consecutive patch pixels
//     (a tile row ends after 14 pixels, an image row after 7), so CpSwz does
//     not apply. Every patch pixel has a PHASE that grows by one per GEMM row
//     of the tile: (px + 6*py) & 7 with a 16-pixel pitch (14 + 2*16 = 6 mod
//     8 steps back to px = 0 of the next row), (px + 7*py + img) & 7 for the
//     9x9 patches; a tap shift adds a constant to all 16 rows of a fragment.
//     The chunk index is XORed with the phase as CpSwz does with the pixel
//     index, so the 8 rows ds_read_b128 serves together in one k-group land
//     on 8 distinct columns. tile_frag_conflict_free enumerates it for every
//     fragment, tap and k-step of each instantiation.
//   - block -> work: slice-major on a 1-D grid (block = slice * tiles +
//     tile, a slice being an (N block, chunk) pair). A map that gave the
//     blocks of equal blockIdx % 8 the same slices, to fetch a weight slice
//     once per XCD, measured equal or slower on every class and was dropped
//     (docs/HEADROOM.md).
// ---------------------------------------------------------------------------

template <bool IMG7>
struct TileMap {
  static constexpr int ROWS = 196;   // GEMM rows of a tile
  static constexpr int NFRAG = 13;   // 16-row fragments that hold them
  static constexpr int PW = IMG7 ? 9 : 16;          // patch row pitch
  static constexpr int NPX = IMG7 ? 4 * 81 : 256;   // staged patch pixels
  static constexpr int KDY = IMG7 ? 7 : 6;  // phase step of a patch row
  // tile row -> patch pixel its tap (0, 0) reads; rows 196..207 of the last
  // fragment continue the pattern past the staged pixels (masked outputs)
  static constexpr int pix(int r) {
    return IMG7 ? (r / 49) * 81 + (r % 49) / 7 * 9 + r % 7
                : (r / 14) * 16 + r % 14;
  }
  static constexpr int phase(int pix) {
    return IMG7 ? (pix / 81 + (pix % 81) / 9 * 7 + pix % 9) & 7
                : ((pix >> 4) * 6 + (pix & 15)) & 7;
  }
  // image pixels past the staged ones that the masked rows may read
  static constexpr int ALLOCPX = (pix(NFRAG * 16 - 1) + 2 * PW + 2 + 8) / 8 * 8;
};
// chunk XOR of a phase: above chunk bit 0 as CpSwz (CC = 64: two pixels share
// a 256 B bank row and the phase's bit 0 is the pixel's)
constexpr int tile_phase_xor(int ph, int CC) {
  return CC == 64 ? ((ph >> 1) & 3) << 1 : (ph & 7) << 1;
}
template <bool IMG7>
struct TileSwz {
  static constexpr int chunk_xor(int pix, int CC) {
    return tile_phase_xor(TileMap<IMG7>::phase(pix), CC);
  }
};
template <bool IMG7>
using TileImage = PatchImage<TileSwz<IMG7>>;

// Fragment `fr`'s A reads: at every tap and k-step the address the kernel
// forms (phase of lane row li at tap (dy, dx) = li + dx + KDY*dy, k-step by
// XOR) is the image's, stays inside the allocation, and is conflict-free in
// each ds_read_b128 lane group.
template <bool IMG7>
constexpr bool tile_frag_conflict_free(int CC, int fr) {
  using Map = TileMap<IMG7>;
  for (int tap = 0; tap < 9; ++tap)
    for (int kb = 0; kb < CC / 32; ++kb)
      for (int g = 0; g < 4; ++g) {
        const int dy = tap / 3, dx = tap % 3;
        unsigned used = 0;
        for (int l = 0; l < 64; ++l) {
          const int m = l & 31;
          const bool first =
              m < 4 || (m >= 12 && m < 16) || (m >= 20 && m < 28);
          if ((l >> 5) * 2 + (first ? 0 : 1) != g) continue;
          const int pixel = Map::pix(fr * 16 + (l & 15)) + dy * Map::PW + dx;
          const int a = TileImage<IMG7>::off(pixel, kb * 4 + (l >> 4), CC);
          const int ph = ((l & 15) + dx + Map::KDY * dy) & 7;
          const int mine =
              (pixel * CC * 2 + (((l >> 4) ^ tile_phase_xor(ph, CC)) << 4)) ^
              (kb * 64);
          if (a != mine || a + 16 > Map::ALLOCPX * CC * 2) return false;
          const unsigned bit = 1u << ((a / 16) % 16);
          if (used & bit) return false;
          used |= bit;
        }
        if (used != 0xffffu) return false;
      }
  return true;
}
// one constant evaluation per fragment
template <bool IMG7, int CC, int FR = TileMap<IMG7>::NFRAG - 1>
struct TileFragProof {
  static constexpr bool value = tile_frag_conflict_free<IMG7>(CC, FR) &&
                                TileFragProof<IMG7, CC, FR - 1>::value;
};
template <bool IMG7, int CC>
struct TileFragProof<IMG7, CC, -1> {
  static constexpr bool value = true;
};

template <int CC, bool IMG7>
struct ConvTileGeo {
  using Map = TileMap<IMG7>;
  static constexpr int THREADS = 512;
  static constexpr int BN = 128;
  static constexpr int WMW = 2, WNW = 4;  // wave grid
  static constexpr int FM = 7, FN = BN / WNW / 16;
  static constexpr int PSLOTS = Map::NPX * (CC / 8);
  static constexpr int PINSTR = (PSLOTS + 63) / 64;  // wave-wide glds
  static constexpr int SP = (PINSTR * 64 + THREADS - 1) / THREADS;
  static constexpr int PBYTES = Map::ALLOCPX * CC * 2;
  static constexpr int KSTEP = 64;        // K of a staged B tile
  static constexpr int LB = BN * KSTEP;   // B tile elems: two 32-K sub-tiles
  static constexpr int RING = 3;
  static constexpr int AHEAD = RING - 2;
  static constexpr int GPS = 2;           // glds per thread per B tile
  static constexpr int SPT = CC / KSTEP;  // B tiles per tap
  static constexpr int NK = 9 * SPT;
  static constexpr int LDS_BYTES = PBYTES + RING * LB * (int)sizeof(bf16_t);
  static_assert(PINSTR * 1024 <= PBYTES && PBYTES % 1024 == 0);
  static_assert(LDS_BYTES <= 160 * 1024);
  static_assert(BN * 4 == THREADS, "one B slot per thread and sub-tile");
};

// tile row -> GEMM row; rows past the tile's 196 map to M (not stored)
template <bool IMG7>
struct TileRows {
  long m00, M;
  int W;
  WN_DEVFN long operator()(int r) const {
    if (r >= TileMap<IMG7>::ROWS) return M;
    if constexpr (IMG7)
      return m00 + r;
    else
      return m00 + (long)(r / 14) * W + (r % 14);
  }
};

template <int CC, bool IMG7, bool SLAB>
__global__ __launch_bounds__(512, 2) void k_conv_tile(
    const bf16_t* __restrict__ X,   // (N, H, W, Cp), Cp = gz * CC
    const bf16_t* __restrict__ Wp,  // [Kp][9*Cp]
    const float* __restrict__ Bias,
    bf16_t* __restrict__ Y,         // (N, H, W, Kp), Kp % 128 == 0
    int N, int H, int W, int Cp, int log2Cp, int Kp, int Klog, int act,
    const bf16_t* __restrict__ Zero16,
    float* __restrict__ Y32,  // SLAB: [Cp / CC][M][Kp] (contract: ConvOut)
    int tiles) {
  static_assert(WN_MFMA_KMAP == 0, "glds staging assumes KMAP 0");
  using G = ConvTileGeo<CC, IMG7>;
  using Map = TileMap<IMG7>;
  using Img = TileImage<IMG7>;
  constexpr int PW = Map::PW, NPX = Map::NPX, SP = G::SP;
  constexpr int FM = G::FM, FN = G::FN, LB = G::LB, RING = G::RING;
  constexpr int AHEAD = G::AHEAD, SPT = G::SPT, NK = G::NK;
  constexpr int THREADS = G::THREADS;  // local: see k_conv_igemm8
  static_assert(CC == 64 || CC == 128);
  static_assert(Img::linear(NPX, CC), "glds slot order != image chunk order");
  static_assert(TileFragProof<IMG7, CC>::value,
                "fragment read: bank conflict or address mismatch");
  const int KG = 9 * Cp;
  const long M = (long)N * H * W;

  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* lP = smem;                                           // patch
  bf16_t* lB = reinterpret_cast<bf16_t*>(smem + G::PBYTES);  // RING x LB

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wid = tid >> 6;
  const int wr = __builtin_amdgcn_readfirstlane(wid >> 2);
  const int wc = wid & 3;

  // block -> (weight slice, tile), block-uniform; a slice is an (N block,
  // chunk) pair
  const int gy = Kp / G::BN;
  const int slice = blockIdx.x / tiles;
  const int tile = blockIdx.x - slice * tiles;
  const int n0 = (slice % gy) * G::BN;
  const int z = slice / gy;
  const int c0 = z * CC;

  // tile -> first image / first output pixel
  int nImg, oy0 = 0, ox0 = 0;
  if constexpr (IMG7) {
    nImg = tile * 4;
  } else {
    const int tilesX = W / 14, tilesY = H / 14;
    nImg = tile / (tilesX * tilesY);
    const int t = tile - nImg * (tilesX * tilesY);
    oy0 = (t / tilesX) * 14;
    ox0 = (t - (t / tilesX) * tilesX) * 14;
  }

  // The patch: as in k_conv_patch, every lane of every issued wave-wide glds
  // sources its pixel's (swizzled) chunk or Zero16 (halo outside the image,
  // images past N, surplus slots).
#pragma unroll
  for (int s = 0; s < SP; ++s) {
    const int sg = tid + s * THREADS;
    if ((sg >> 6) < G::PINSTR) {  // wave-uniform
      const int pix = Img::slot_pix(sg, CC);
      int n, iy, ix;
      if constexpr (IMG7) {
        const int img = pix / 81, q = pix - img * 81;
        n = nImg + img;
        iy = q / 9 - 1;
        ix = q - (q / 9) * 9 - 1;
      } else {
        n = nImg;
        iy = oy0 + (pix >> 4) - 1;
        ix = ox0 + (pix & 15) - 1;
      }
      const bf16_t* src = Zero16;
      if (pix < NPX && n < N && iy >= 0 && iy < H && ix >= 0 && ix < W)
        src = X + (((long)n * H + iy) * W + ix) * Cp + c0 +
              Img::slot_chunk(sg, CC) * 8;
      glds16(src, reinterpret_cast<bf16_t*>(lP + sg * 16));
    }
  }

  // B tile g: taps' CC-channel chunk in 64-K pieces, two fragment-major
  // 32-K sub-tiles; every thread issues GPS = 2 glds (k < Kp: Kp % 128 == 0)
  const FragSlot bf = frag_slot<false>(tid);
  const bf16_t* bSrc = Wp + (long)(n0 + bf.row) * KG + c0 + bf.koff;
  auto stage_b = [&](int buf, int g) {
    const int tap = g / SPT, h = g - tap * SPT;
    const bf16_t* src = bSrc + tap * Cp + h * G::KSTEP;
    glds16(src, lB + buf * LB + tid * 8);
    glds16(src + 32, lB + buf * LB + G::BN * 32 + tid * 8);
  };

  f32x4 acc[FM][FN];
#pragma unroll
  for (int a = 0; a < FM; ++a)
#pragma unroll
    for (int b = 0; b < FN; ++b) acc[a][b] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int lg = lane >> 4, li = lane & 15;
  // the second M half has 6 fragments: 13 in all
  const int nfm = wr == 0 ? FM : Map::NFRAG - FM;
  // byte offset of this lane's row of each fragment at tap (0, 0), chunk 0
  int aPix[FM];
#pragma unroll
  for (int fm = 0; fm < FM; ++fm) {
    const int r = min((wr * FM + fm) * 16 + li, Map::NFRAG * 16 - 1);
    aPix[fm] = Map::pix(r) * CC * 2;
  }

  for (int t = 0; t < RING - 1 && t < NK; ++t) stage_b(t, t);
  wait_vmcnt<0>();
  __builtin_amdgcn_s_barrier();

  int g = 0;
  for (int tap = 0; tap < 9; ++tap) {
    const int dy = tap / 3, dx = tap - dy * 3;
    // k-step 0 addresses; k-step kb flips chunk bits 2-3 = address bits 6-7
    const int ph = (li + dx + Map::KDY * dy) & 7;
    const int tapOff =
        (dy * PW + dx) * CC * 2 + ((lg ^ tile_phase_xor(ph, CC)) << 4);
    unsigned aAd[FM];
#pragma unroll
    for (int fm = 0; fm < FM; ++fm) aAd[fm] = (unsigned)(aPix[fm] + tapOff);
#pragma unroll
    for (int h = 0; h < SPT; ++h, ++g) {
      const int b = g % RING;
      if (g + RING - 1 < NK) stage_b((b + RING - 1) % RING, g + RING - 1);
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        const int kb = h * 2 + s;
        bf16x8 aF[FM], bF[FN];
#pragma unroll
        for (int fn = 0; fn < FN; ++fn)
          bF[fn] = *reinterpret_cast<const bf16x8*>(
              lB + b * LB + s * (G::BN * 32) +
              (((wc * FN + fn) * 4 + lg) * 16 + li) * 8);
#pragma unroll
        for (int ph2 = 0; ph2 < 2; ++ph2) {
          const int f0 = ph2 * 4, f1 = ph2 ? FM : 4;
#pragma unroll
          for (int fm = f0; fm < f1; ++fm)
            if (fm < nfm)
              aF[fm] = *reinterpret_cast<const bf16x8*>(
                  lP + (aAd[fm] ^ (unsigned)(kb * 64)));
          asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
          __builtin_amdgcn_sched_barrier(0);
          __builtin_amdgcn_s_setprio(1);
#pragma unroll
          for (int fm = f0; fm < f1; ++fm)
            if (fm < nfm) {
#pragma unroll
              for (int fn = 0; fn < FN; ++fn)
                acc[fm][fn] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                    aF[fm], bF[fn], acc[fm][fn], 0, 0, 0);
            }
          __builtin_amdgcn_s_setprio(0);
        }
      }
      if (g + 1 < NK) {
        wait_tiles<G::GPS, AHEAD>(min(NK - g - 2, AHEAD));
        __builtin_amdgcn_s_barrier();
      }
    }
  }

  // epilogue: the shared path over the tile's row map. store_out adds
  // blockIdx.z slabs, which is 0 on this 1-D grid: the chunk's slab is put
  // into the pointer instead.
  const ConvOut out{Bias, Y, SLAB ? Y32 + (long)z * M * Kp : nullptr, M, Kp,
                    Klog, act};
  TileRows<IMG7> rows;
  rows.M = M;
  rows.W = W;
  if constexpr (IMG7)
    rows.m00 = (long)tile * Map::ROWS;
  else
    rows.m00 = ((long)nImg * H + oy0) * W + ox0;
  store_tile<SLAB, 16>(acc, rows, wr * FM * 16, n0 + wc * (FN * 16), lane,
                       out);
}

// Split-K finalize: Y = act(sum over gz slabs of Y32 + bias), pad zeroed.
// GZ is a template constant so all slab loads issue in parallel (the
// runtime-bounded loop serialized up to 8 dependent ~500-cycle loads per
// element — measured 9.5 us per call, ~1.5 us unrolled).
template <int GZ>
__global__ void k_splitk_finalize(const float* __restrict__ Y32,
                                  const float* __restrict__ Bias,
                                  bf16_t* __restrict__ Y, long M, int Kp,
                                  int Klog, int act) {
  const long total = M * Kp;
  for (long i0 = ((long)blockIdx.x * blockDim.x + threadIdx.x) * 4;
       i0 < total; i0 += (long)gridDim.x * blockDim.x * 4) {
    f32x4 vz[GZ];
#pragma unroll
    for (int z = 0; z < GZ; ++z)
      vz[z] = *reinterpret_cast<const f32x4*>(Y32 + z * total + i0);
    f32x4 v = vz[0];
#pragma unroll
    for (int z = 1; z < GZ; ++z)
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] += vz[z][e];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const long i = i0 + e;
      const int k = (int)(i % Kp);
      const float bv = (Bias != nullptr && k < Klog) ? Bias[k] : 0.f;
      Y[i] = f2bf(bias_act(v[e], bv, k >= Klog, act));
    }
  }
}

// ---------------------------------------------------------------------------
// Host-side dispatch
// ---------------------------------------------------------------------------

namespace {

// Which forward kernel a conv shape runs on, and on what grid. The single
// source of the dispatch rule: launch_conv_bn launches what this returns and
// conv2d_fwd_plan reports it to the tests.
enum ConvTier {
  TIER_IGEMM = 0,
  TIER_SPLITK = 1,
  TIER_IGEMM8 = 2,
  TIER_PATCH = 3,
  TIER_TILE = 4
};

struct ConvPlan {
  ConvTier tier;
  int BN;      // N tile: 16 / 32 / 64 / 128
  int gx, gy;  // 128-row M blocks, BN-wide N blocks
  int nk;      // 32-wide K tiles
  int gz;      // split-K slices (TIER_SPLITK) or channel chunks (TIER_TILE)
  int cc;      // TIER_TILE: channels per chunk; gx = its tiles
};

// k_conv_patch is instantiated for KS 3/5/7 with Cp and Kp each 64 or 128.
inline bool conv_patch_instantiated(int ks, int Cp, int Kp) {
  return (ks == 3 || ks == 5 || ks == 7) && (Cp == 64 || Cp == 128) &&
         (Kp == 64 || Kp == 128);
}

// Classes where k_conv_patch measured faster than k_conv_igemm8 in the
// per-shape A/B (docs/KERNELS.md, k_conv_patch table): a class is listed only
// if every patch repeat beat the fastest igemm8 repeat at 112^2 and 256^2.
// Today that is every instantiated class (1.01-2.1x; the narrowest is
// k3 128->128 at 112^2, 136.8 us against 138.4).
inline bool conv_patch_wins(int ks, int Cp, int Kp) {
  return conv_patch_instantiated(ks, Cp, Kp);
}

// WN_CONV_PATCH, read once per process: 0 disables the patch tier, 1 forces
// it wherever it is instantiated and eligible, unset (-1) follows
// conv_patch_wins.
inline int conv_patch_knob() {
  static const int knob = [] {
    const char* e = getenv("WN_CONV_PATCH");
    return e ? (atoi(e) != 0 ? 1 : 0) : -1;
  }();
  return knob;
}

// k_conv_tile: k3, Cp 128 / 256 / 512 in 64- or 128-channel chunks, Kp a
// multiple of its 128-wide N tile, whole 14x14 tiles or 7x7 images.
inline bool conv_tile_eligible(int H, int W, int Cp, int Kp, int ks) {
  return ks == 3 && (Cp == 128 || Cp == 256 || Cp == 512) && Kp % 128 == 0 &&
         ((H % 14 == 0 && W % 14 == 0) || (H == 7 && W == 7));
}
inline int conv_tile_tiles(int N, int H, int W) {
  return H == 7 ? (N + 3) / 4 : N * (H / 14) * (W / 14);
}

// WN_CONV_TILE as WN_CONV_PATCH, read once per process: 0 disables the tile
// tier, 1 forces it wherever it is eligible, unset (-1) follows
// conv_tile_wins. WN_CONV_TILE_CC (64 / 128) is a bench-only knob: it
// overrides the chunk width of a shape that runs the tier, for the per-shape
// A/B (tools/conv_tile_ab.py) and the tests of both widths.
inline int conv_tile_on() {
  static const int knob = [] {
    const char* e = getenv("WN_CONV_TILE");
    return e ? (atoi(e) != 0 ? 1 : 0) : -1;
  }();
  return knob;
}
inline int conv_tile_cc_knob() {
  static const int cc = [] {
    const char* e = getenv("WN_CONV_TILE_CC");
    const int k = e ? atoi(e) : 0;
    return k == 64 || k == 128 ? k : 0;
  }();
  return cc;
}

// Chunk width the tile tier runs a shape at by default, 0 where the shape
// stays on its present tier. One row per class measured in the per-shape A/B
// (docs/KERNELS.md, k_conv_tile table; profiles/r12_conv_tile_ab.jsonl): a
// class is listed, at its faster width, only if every tile repeat beat the
// fastest repeat of its present tier. Measured at N = 16 (the flagship
// batch); smaller batches and every other size were not measured and stay
// where they are. Not listed because it lost: 7^2 512->512 (both widths).
struct ConvTileWin { int hw, Cp, Kp, cc; };
constexpr ConvTileWin CONV_TILE_WINS[] = {
    {56, 128, 128, 128},  // igemm8
    {28, 128, 256, 128}, {28, 256, 128, 64}, {28, 256, 256, 128},
    {14, 256, 512, 64},  {14, 512, 256, 64}, {14, 512, 512, 128},
};
constexpr int CONV_TILE_MIN_N = 16;
inline int conv_tile_wins(int N, int H, int W, int Cp, int Kp) {
  if (N < CONV_TILE_MIN_N || H != W) return 0;
  for (const ConvTileWin& w : CONV_TILE_WINS)
    if (w.hw == H && w.Cp == Cp && w.Kp == Kp) return w.cc;
  return 0;
}

inline ConvPlan conv_plan(int N, int H, int W, int Cp, int Kp, int ks) {
  const long M = (long)N * H * W;
  ConvPlan p;
  p.cc = 0;
  p.BN = Kp >= 128 ? 128 : Kp == 64 ? 64 : Kp == 32 ? 32 : 16;
  p.gx = (int)((M + 127) / 128);
  p.gy = (Kp + p.BN - 1) / p.BN;
  p.nk = (ks * ks * Cp + 31) / 32;
  // Small-M shapes (e.g. VGG 14^2/7^2 layers at bs=16) leave most of the
  // 256 CUs idle; split the K loop across gz slices into fp32 partials,
  // then finalize bias+act+bf16 in a second tiny pass.
  const int base = p.gx * p.gy;
  int gz = 1;
  if (base < 320 && p.nk >= 16)
    gz = std::min(std::max(1, 512 / base), p.nk / 4);
  // finalize's unrolled reads tolerate more slabs for the tiniest
  // (grid-limited) shapes; snap >8 to the instantiated 12/16 variants
  gz = std::min(gz, base < 64 ? 16 : 8);
  if (gz > 8) gz = (gz >= 16) ? 16 : 12;
  p.gz = gz;
  p.tier = TIER_IGEMM;
  if (gz > 1) {
    p.tier = TIER_SPLITK;
  } else if (p.BN >= 64) {
    static const long m8_thresh = [] {
      // A/B override: the M threshold above which the 8-wave 256-row
      // igemm8 is used instead of the 4-wave 128-row igemm
      const char* e = getenv("WN_IGEMM8_MTHRESH");
      return e ? atol(e) : 16384L;
    }();
    if (M >= m8_thresh) p.tier = TIER_IGEMM8;
  }
  // The patch tier takes over from igemm8 only: whole 16x16 pixel tiles and
  // an instantiated class, by the knob or the measured table.
  if (p.tier == TIER_IGEMM8 && conv_patch_instantiated(ks, Cp, Kp) &&
      H % 16 == 0 && W % 16 == 0) {
    const int knob = conv_patch_knob();
    if (knob == 1 || (knob == -1 && conv_patch_wins(ks, Cp, Kp)))
      p.tier = TIER_PATCH;
  }
  // The tile tier takes over from the split-K igemm and from igemm8 (never
  // from the patch tier), by the knob or the measured table.
  if ((p.tier == TIER_SPLITK || p.tier == TIER_IGEMM8) &&
      conv_tile_eligible(H, W, Cp, Kp, ks)) {
    const int knob = conv_tile_on();
    int cc = knob == 0 ? 0 : conv_tile_wins(N, H, W, Cp, Kp);
    if (knob == 1 && cc == 0) cc = 128;
    if (cc != 0 && conv_tile_cc_knob() != 0) cc = conv_tile_cc_knob();
    if (cc != 0) {
      p.tier = TIER_TILE;
      p.BN = 128;
      p.cc = cc;
      p.gx = conv_tile_tiles(N, H, W);
      p.gy = Kp / 128;
      p.gz = Cp / cc;
    }
  }
  return p;
}

// A/B knobs of the igemm8 tier, read once per process.
inline int igemm8_var() {
  static const int var = [] {
    const char* e = getenv("WN_IGEMM8_VAR");
    return e ? atoi(e) : 0;
  }();
  return var;
}
inline bool igemm8_m32() {
  static const bool m32 = [] {
    const char* e = getenv("WN_IGEMM8_M32");
    // default OFF: A/B measured a tie on training and -10% at
    // bs=1 1080p inference (the wgrad M32, by contrast, is +5.5%)
    return e != nullptr && atoi(e) != 0;
  }();
  return m32;
}

template <int KS>
void launch_conv_bn(const at::Tensor& x, const at::Tensor& wp,
                    const c10::optional<at::Tensor>& bias, at::Tensor& y,
                    int Klog, int act, hipStream_t stream) {
  const int N = x.size(0), H = x.size(1), W = x.size(2), Cp = x.size(3);
  const int Kp = y.size(3);
  const long M = (long)N * H * W;
  const float* bptr =
      bias.has_value() ? bias->data_ptr<float>() : nullptr;
  const ConvPlan plan = conv_plan(N, H, W, Cp, Kp, KS);
  const int gy = plan.gy, gz = plan.gz;
  const bf16_t* zptr = zero16_for(x);

  // The igemm tiers' argument list, written once: each tier's launch is
  // handed it as a pack and names its own kernel (k_conv_igemm appends Y32).
  auto with_args = [&](auto&& launch) {
    launch((const bf16_t*)x.data_ptr(), (const bf16_t*)wp.data_ptr(), bptr,
           (bf16_t*)y.data_ptr(), N, H, W, Cp, log2i(Cp), Kp, Klog, act,
           zptr);
  };
  dispatch_int_or<16, 128, 64, 32, 16>(plan.BN, [&](auto bn_const) {
    constexpr int BN = decltype(bn_const)::value;
    if constexpr (BN == 128 && KS == 3) {
      if (plan.tier == TIER_TILE) {  // deep k3 layers: tile-resident
        const bool slab = gz > 1;
        at::Tensor y32;
        if (slab)
          y32 = at::empty({gz, M, (long)Kp}, x.options().dtype(at::kFloat));
        float* y32p = slab ? y32.data_ptr<float>() : nullptr;
        const dim3 grid(plan.gx * gy * gz);
        dispatch_int<64, 128>(plan.cc, "k_conv_tile CC", [&](auto cc_const) {
          constexpr int CC = decltype(cc_const)::value;
          dispatch_int<0, 1>(H == 7, "IMG7", [&](auto i7_const) {
            constexpr bool I7 = decltype(i7_const)::value != 0;
            using G = ConvTileGeo<CC, I7>;
            dispatch_int<0, 1>(slab, "SLAB", [&](auto sl_const) {
              constexpr bool SL = decltype(sl_const)::value != 0;
              with_args([&](auto... a) {
                hipLaunchKernelGGL((k_conv_tile<CC, I7, SL>), grid,
                                   dim3(G::THREADS), (size_t)G::LDS_BYTES,
                                   stream, a..., y32p, plan.gx);
              });
            });
          });
        });
        if (slab) {
          const long total = M * Kp;
          const int fb = (int)std::min<long>(512, (total / 4 + 255) / 256);
          dispatch_int<2, 4, 8>(gz, "k_conv_tile gz", [&](auto gz_const) {
            constexpr int GZ = decltype(gz_const)::value;
            hipLaunchKernelGGL((k_splitk_finalize<GZ>), dim3(fb), dim3(256),
                               0, stream, y32p, bptr, (bf16_t*)y.data_ptr(),
                               M, Kp, Klog, act);
          });
        }
        return;
      }
    }
    TORCH_CHECK(plan.tier != TIER_TILE, "k_conv_tile<", KS, ", ", BN,
                "> is not instantiated");
    if (plan.tier == TIER_SPLITK) {
      using G = IgemmGeo<BN, true>;
      auto y32 = at::empty({gz, M, (long)Kp}, x.options().dtype(at::kFloat));
      with_args([&](auto... a) {
        hipLaunchKernelGGL((k_conv_igemm<BN, KS, true>),
                           dim3(plan.gx, gy, gz), dim3(G::THREADS),
                           (size_t)G::LDS_BYTES, stream, a...,
                           y32.data_ptr<float>());
      });
      const long total = M * Kp;
      const int fb = (int)std::min<long>(512, (total / 4 + 255) / 256);
      dispatch_int_or<8, 2, 3, 4, 5, 6, 7, 8, 12, 16>(gz, [&](auto gz_const) {
        constexpr int GZ = decltype(gz_const)::value;
        hipLaunchKernelGGL((k_splitk_finalize<GZ>), dim3(fb), dim3(256), 0,
                           stream, y32.data_ptr<float>(), bptr,
                           (bf16_t*)y.data_ptr(), M, Kp, Klog, act);
      });
      return;
    }
    if constexpr (BN >= 64 && KS >= 3) {
      if (plan.tier == TIER_PATCH) {  // big-M, whole 16x16 tiles
        dispatch_int<64, 128>(Cp, "k_conv_patch Cp", [&](auto cc_const) {
          constexpr int CC = decltype(cc_const)::value;
          using G = ConvPatchGeo<KS, BN, CC>;
          const dim3 grid(N * (H / G::TH) * (W / G::TW), gy);
          with_args([&](auto... a) {
            hipLaunchKernelGGL((k_conv_patch<KS, BN, CC>), grid,
                               dim3(G::THREADS), (size_t)G::LDS_BYTES, stream,
                               a...);
          });
        });
        return;
      }
    }
    TORCH_CHECK(plan.tier != TIER_PATCH, "k_conv_patch<", KS, ", ", BN,
                "> is not instantiated");
    if constexpr (BN >= 64) {
      if (plan.tier == TIER_IGEMM8) {  // big-M: 8-wave 256-row phase-split
        // M32 exists for VAR 0 only and wins over WN_IGEMM8_VAR
        const bool m32 = igemm8_m32();
        dispatch_int_or<0, 0, 1, 2, 3>(
            m32 ? 0 : igemm8_var(), [&](auto var_const) {
              constexpr int V = decltype(var_const)::value;
              using G = Igemm8Geo<BN, V>;
              const dim3 grid((int)((M + G::BM - 1) / G::BM), gy);
              dispatch_int<0, 1>(m32, "M32", [&](auto m32_const) {
                constexpr bool M32 = V == 0 && decltype(m32_const)::value;
                with_args([&](auto... a) {
                  hipLaunchKernelGGL((k_conv_igemm8<BN, KS, V, M32>), grid,
                                     dim3(G::THREADS), (size_t)G::LDS_BYTES,
                                     stream, a...);
                });
              });
            });
        return;
      }
    }
    using G = IgemmGeo<BN, false>;
    with_args([&](auto... a) {
      hipLaunchKernelGGL((k_conv_igemm<BN, KS, false>), dim3(plan.gx, gy),
                         dim3(G::THREADS), (size_t)G::LDS_BYTES, stream, a...,
                         (float*)nullptr);
    });
  });
  HIP_CHECK_LAST();
}
}  // namespace

// The dispatch decision conv2d_fwd would take for an (N,H,W,Cp) input and Kp
// output channels: (kernel, BN, gz). Host only: launches nothing and touches
// no device memory.
std::tuple<std::string, int64_t, int64_t> conv2d_fwd_plan(
    int64_t N, int64_t H, int64_t W, int64_t Cp, int64_t Kp, int64_t ks) {
  TORCH_CHECK(ks == 1 || ks == 3 || ks == 5 || ks == 7,
              "unsupported kernel size ", ks);
  const ConvPlan p =
      conv_plan((int)N, (int)H, (int)W, (int)Cp, (int)Kp, (int)ks);
  const char* name = p.tier == TIER_SPLITK   ? "splitk"
                     : p.tier == TIER_IGEMM8 ? "igemm8"
                     : p.tier == TIER_PATCH  ? "patch"
                     : p.tier == TIER_TILE   ? "tile"
                                             : "igemm";
  return {name, p.BN, p.gz};
}

at::Tensor conv2d_fwd(const at::Tensor& x, const at::Tensor& wp,
                      const c10::optional<at::Tensor>& bias, int64_t ks,
                      int64_t Kp, int64_t Klog, int64_t act) {
  TORCH_CHECK(x.is_cuda() && x.dtype() == at::kBFloat16 && x.dim() == 4,
              "x must be CUDA bf16 NHWC");
  TORCH_CHECK(wp.is_cuda() && wp.dtype() == at::kBFloat16);
  TORCH_CHECK(x.is_contiguous() && wp.is_contiguous());
  auto y = at::empty({x.size(0), x.size(1), x.size(2), Kp},
                     x.options());
  hipStream_t stream = at::cuda::getCurrentHIPStream();
  dispatch_int<1, 3, 5, 7>((int)ks, "kernel size", [&](auto ks_const) {
    launch_conv_bn<decltype(ks_const)::value>(x, wp, bias, y, (int)Klog,
                                              (int)act, stream);
  });
  return y;
}
