// Weight- and bias-gradient kernels of the MFMA conv engine for gfx950
// (CDNA4); forward / dgrad are in conv_fwd.hip. Replaces the reference's
// implicit cuDNN backward-filter launches with hand-written NHWC bf16
// kernels:
//   - k_conv_wgrad<KS,BK,CH>: weight gradient as reduction GEMM over M,
//     m-major LDS images + ds_read_b64_tr_b16 hardware transpose reads,
//     fp32 atomic accumulation into the NCHW fp32 grad tensor.
//   - k_conv_wgrad_patch<KS,BK,CT,CH>: weight gradient for KS >= 3 and
//     32/64-multiple channel classes: one X row segment staged once, the
//     KS dx taps taken by row-shifted tr reads, LDS-transposed epilogue so
//     the atomics are contiguous.
//   - k_conv_wgrad_patch16<KS,BK,CH>: the same for Cp = 16, two taps per
//     MFMA. Both patch kernels are wgrad_patch_body (ownership, staging, A
//     base, k-step ring, slab epilogue) with their own B-fragment policy, and
//     share launch_wgrad_patch_t.
//   - k_wgrad_smallk: VALU outer-product path for K <= 4 output convs.
//   - k_bias_grad(+_reduce): slab-partial column sums of dY.
//   - k_probe_tr(+_raw): ds_read_b64_tr_b16 semantics probes for the tests.
// Every kernel with dynamic LDS takes its tile constants from a Geo struct,
// and its launch takes LDS_BYTES from the same struct. The counted waits and
// the glds patch-image slot map (PatchImage) are in conv_common.h.

#include "conv_common.h"

// ---------------------------------------------------------------------------
// Weight gradient: dW[k][rsc] = sum_m dY[m][k] * X[m][rsc]
//
// v3: both GEMM operands are [reduction=m]-major in global memory (dY is
// (m,k), X gathers are (m,c)), i.e. TRANSPOSED relative to the MFMA
// fragment layout (lane needs 8 m for a fixed column). v2 transposed via
// 8x ds_write_b16 scatter, which lands 16-32 lanes on the same mod-32
// write bank (ds_write banks are (a/4)%32) — LDS-write-bound. v3 stores
// the tiles m-major with vector ds_write_b128 (conflict-free by kblk
// stride choice) and uses gfx950's ds_read_b64_tr_b16 hardware transpose
// read to deliver MFMA fragments (guide T10, the attention-V recipe).
//
// LDS image per operand: [col/16 kblk][m/4 mblk][4m][16col] subtiles,
// row-major inside a subtile; mblk stride 96 elems (2*96 dwords = 32 mod
// 64 so tr-read lane groups land on disjoint read banks), kblk stride
// 1552 elems (776 dwords = 8 mod 32 so the staging b128 writes of one
// 8-lane service group hit 8 distinct bank quads).
//
//   - BK x 128 output tile per block (BK = min(Kp,128)), 2x2 / 1x4 waves
//   - m-chunks of 64; DOUBLE-BUFFERED global_load_lds staging: the linear
//     chunk index of the tr image maps identically to tr_addr, so the DMA
//     writes the image lane-linearly while per-lane sources gather the
//     right 16 B of dY / halo-masked X (pad lanes read a zero buffer).
//     The next chunk's DMA issues before this chunk's MFMAs and drains at
//     the single trailing barrier.
//   - default MFMA is v_mfma_f32_32x32x16_bf16 (M32) with a per-kstep
//     counted-lgkmcnt tr-read interleave; WN_WGRAD_M32=0 selects the
//     16x16x32 path.
//   - split-m z dimension sized to fill the CUs; gy (rsc tiles) varies
//     fastest so co-resident blocks share dY/X chunks through L2.
//   - fp32 atomicAdd epilogue into the NCHW fp32 grad tensor (pre-zeroed).
// Requires the KMAP-0 fragment layout (lane group g consumes k = g*8+e).
// ---------------------------------------------------------------------------

constexpr int TR_MBS = 72;    // mblk stride (36 dwords; 2 mblks = 8 mod 64
                              // banks -> at most 2-way tr-read overlap, and
                              // the image fits 4 blocks/CU at CH=64)
constexpr int TR_KBS = 16 * TR_MBS + 16;  // kblk stride (584 dw = 8 mod 32:
                                          // conflict-free staging writes)

// Magic-multiply unsigned division by a launch-constant divisor d:
// q = (n * mul) >> 42 with mul = floor(2^42/d)+1 — exact for n*d < 2^42
// (holds for any image geometry we launch). Replaces the 64-bit v_div
// chains the m->(n,oy,ox) decode otherwise costs per chunk (PMC r06:
// wgrad SQ_WAIT_INST_ANY 47-75% with zero bank conflicts = serial VALU
// division RAW stalls).
struct MagicDiv {
  unsigned long long mul;
  static MagicDiv make(unsigned d) {
    return {(0x40000000000ULL / d) + 1};
  }
};
WN_DEVFN unsigned magic_div(unsigned n, unsigned long long mul) {
  return (unsigned)(((unsigned long long)n * mul) >> 42);
}

// elem offset of (m, col) inside a tr image
template <int KBS = TR_KBS>
WN_DEVFN int tr_addr(int m, int col) {
  return (col >> 4) * KBS + (m >> 2) * TR_MBS + (m & 3) * 16 + (col & 15);
}

typedef __attribute__((ext_vector_type(4))) __bf16 bf16x4;

// ds_read_b64_tr_b16: lane (l&15) of each 16-lane group receives column
// (l&15), rows 0..3, of the [4][16] row-major bf16 subtile whose 16
// 8-byte pieces the group's lanes address in canonical order (lane i ->
// subtile_base + i*8B). addr is an LDS byte address.
WN_DEVFN bf16x4 ds_tr16(unsigned addr) {
  bf16x4 v;
  // "memory" keeps the read below the staging stores / barrier (without it
  // hipcc hoists the first tr read above the LDS fill — measured garbage).
  asm volatile("ds_read_b64_tr_b16 %0, %1" : "=v"(v) : "v"(addr) : "memory");
  return v;
}

// dW[k][c][dy][dx] += v for GEMM element (k, rsc = tap*Cp + c); rows past K,
// columns past KG and pad channels are dropped.
template <int KS>
WN_DEVFN void wgrad_scatter_add(float* dW, int k, int rsc, float v, int K,
                                int KG, int C, int Cp, int log2Cp) {
  if (k >= K || rsc >= KG) return;
  const int tap = rsc >> log2Cp;
  const int c = rsc & (Cp - 1);
  if (c >= C) return;
  const int dy = tap / KS, dx = tap - (tap / KS) * KS;
  atomicAdd(&dW[(((long)k * C + c) * KS + dy) * KS + dx], v);
}

// k_conv_wgrad tile geometry: BK x 128 output tile, m-chunks of CH.
template <int BK, int CH>
struct WgradGeo {
  static constexpr int BR = 128;  // rsc tile
  // per-chunk tr image kblk stride: CH/4 mblks x 96 elems + 16 pad, which
  // keeps the stride 8 mod 32 dwords (conflict-free staging writes)
  static constexpr int KBS = CH / 4 * TR_MBS + 16;  // = TR_KBS at CH=64
  static constexpr int WR = (BK >= 64) ? 2 : 1;     // wave rows (k dim)
  static constexpr int WC = 4 / WR;                 // wave cols (rsc dim)
  static constexpr int FK = BK / WR / 16;  // k fragments per wave
  static constexpr int FR = BR / WC / 16;  // rsc fragments per wave
  // M32: the wave tile stays 64x64 (BK>=64), FK32 x FR32 accumulators
  static constexpr int FK32 = (BK >= 64) ? BK / WR / 32 : 1;
  static constexpr int FR32 = BR / WC / 32;
  static constexpr int CPK = KBS / 8;         // 16 B chunks per kblk
  static constexpr int AC = (BK / 16) * CPK;  // A image chunks
  static constexpr int BC = (BR / 16) * CPK;  // B image chunks
  static constexpr int SA = (AC + 255) / 256, SB = (BC + 255) / 256;
  static constexpr int ABUF = SA * 256 * 8;  // elems per buffer (padded so
  static constexpr int BBUF = SB * 256 * 8;  //  out-of-image slots land in-pad)
  static constexpr int LDS_BYTES =
      2 * (ABUF + BBUF) * (int)sizeof(bf16_t);  // double-buffered
};

template <int KS, int BK, int CH = 64, bool M32 = false>
__global__ __launch_bounds__(256, 2) void k_conv_wgrad(
    const bf16_t* __restrict__ dY,  // (N,H,W,Kp)
    const bf16_t* __restrict__ X,   // (N,H,W,Cp)
    float* __restrict__ dW,         // (K, C, KS, KS) fp32, pre-zeroed
    int N, int H, int W, int Cp, int log2Cp, int Kp, int K, int C,
    int splitm, unsigned long long mulHW, unsigned long long mulW,
    const bf16_t* __restrict__ Zero16w) {
  static_assert(WN_MFMA_KMAP == 0, "wgrad staging assumes KMAP 0");
  using G = WgradGeo<BK, CH>;
  constexpr int PAD = KS / 2;
  constexpr int RS = KS * KS;
  constexpr int BR = G::BR, KBS = G::KBS, WR = G::WR, WC = G::WC;
  constexpr int FK = G::FK, FR = G::FR, CPK = G::CPK, AC = G::AC, BC = G::BC;
  constexpr int SA = G::SA, SB = G::SB, ABUF = G::ABUF, BBUF = G::BBUF;
  const int KG = RS * Cp;
  const long M = (long)N * H * W;
  const int HW = H * W;

  // glds staging: the tr image's linear 8-element chunk index sigma maps
  // IDENTICALLY to tr_addr (sigma*8 == tr_addr(m, col) for m = mblk*4 +
  // (r>>1), col = kblk*16 + (r&1)*8, sigma = kblk*CPK + mblk*9 + r), so
  // global_load_lds writes the image lane-linearly while each lane's
  // SOURCE gathers the right 16 B of dY/X (pad/halo lanes read Zero16).
  // Double-buffered: the next chunk's DMA issues before this chunk's
  // MFMAs and drains at the single trailing barrier.
  extern __shared__ __attribute__((aligned(16))) char smem[];
  bf16_t* lA = reinterpret_cast<bf16_t*>(smem);   // 2 x ABUF
  bf16_t* lB = lA + 2 * ABUF;                     // 2 x BBUF

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wid = tid >> 6;
  const int wr = wid / WC;
  const int wc = wid % WC;
  const int kt0 = blockIdx.x * BK;
  const int rt0 = blockIdx.y * BR;

  // ---- static slot geometry (sigma -> image position -> source) ----
  int aM_[SA], aCol[SA];
  bool aPad[SA];
#pragma unroll
  for (int s = 0; s < SA; ++s) {
    const int sg = tid + s * 256;
    const int kblk = sg / CPK, c = sg % CPK;
    const int mblk = c / 9, r = c % 9;
    aPad[s] = (sg >= AC) || (r == 8) || (c >= (CH / 4) * 9);
    aM_[s] = mblk * 4 + (r >> 1);
    aCol[s] = kt0 + kblk * 16 + (r & 1) * 8;
  }
  int bM_[SB], bC_[SB], bDy[SB], bDx[SB];
  bool bPad[SB];
#pragma unroll
  for (int s = 0; s < SB; ++s) {
    const int sg = tid + s * 256;
    const int kblk = sg / CPK, c = sg % CPK;
    const int mblk = c / 9, r = c % 9;
    const int rsc = rt0 + kblk * 16 + (r & 1) * 8;
    bPad[s] = (sg >= BC) || (r == 8) || (c >= (CH / 4) * 9) || (rsc >= KG);
    bM_[s] = mblk * 4 + (r >> 1);
    const int tap = rsc >> log2Cp;
    bC_[s] = rsc & (Cp - 1);
    bDy[s] = tap / KS;
    bDx[s] = tap - bDy[s] * KS;
  }

  auto stage = [&](int buf, long mbase) {
#pragma unroll
    for (int s = 0; s < SA; ++s) {
      const bf16_t* src = Zero16w;
      const long m = mbase + aM_[s];
      if (!aPad[s] && m < M) src = dY + m * Kp + aCol[s];
      __builtin_amdgcn_global_load_lds(
          src, lA + buf * ABUF + (tid + s * 256) * 8, 16, 0, 0);
    }
#pragma unroll
    for (int s = 0; s < SB; ++s) {
      const bf16_t* src = Zero16w;
      const long m = mbase + bM_[s];
      if (!bPad[s] && m < M) {
        unsigned n = magic_div((unsigned)m, mulHW);
        unsigned rem = (unsigned)m - n * (unsigned)HW;
        unsigned oy = magic_div(rem, mulW);
        int ox = (int)(rem - oy * (unsigned)W);
        int iy = (int)oy + bDy[s] - PAD, ix = ox + bDx[s] - PAD;
        if (iy >= 0 && iy < H && ix >= 0 && ix < W)
          src = X + (((long)((int)n * H + iy) * W + ix) << log2Cp) + bC_[s];
      }
      __builtin_amdgcn_global_load_lds(
          src, lB + buf * BBUF + (tid + s * 256) * 8, 16, 0, 0);
    }
  };

  // M32 variant: v_mfma_f32_32x32x16_bf16 — half the MFMA instruction
  // count for the same MACs at the 2382-vs-2075 TF pipe rate (PMC shows
  // the 16x16 wgrad is MFMA-pipe-saturated). Wave tile stays 64x64
  // (BK>=64): FK32 x FR32 accumulators of 16 f32.
  constexpr int FK32 = G::FK32, FR32 = G::FR32;
  f32x4 acc[M32 ? 1 : FK][M32 ? 1 : FR];
  f32x16 acc32[M32 ? FK32 : 1][M32 ? FR32 : 1];
#pragma unroll
  for (int a = 0; a < (M32 ? FK32 : FK); ++a)
#pragma unroll
    for (int b = 0; b < (M32 ? FR32 : FR); ++b) {
      if constexpr (M32) {
#pragma unroll
        for (int e = 0; e < 16; ++e) acc32[a][b][e] = 0.f;
      } else {
        acc[a][b] = f32x4{0.f, 0.f, 0.f, 0.f};
      }
    }

  const long nChunks = (M + CH - 1) / CH;
  const int lg = lane >> 4, li = lane & 15;
  // per-lane tr-read byte addresses for kstep 0 / mblk (2*lg); the second
  // 4-m half (e=4..7) is the next mblk at +2*TR_MBS bytes.
  const unsigned aTr0 = (unsigned)(unsigned long long)lA +
                        (unsigned)(2 * lg * TR_MBS + li * 4) * 2;
  const unsigned bTr0 = (unsigned)(unsigned long long)lB +
                        (unsigned)(2 * lg * TR_MBS + li * 4) * 2;
  // M32 per-lane bases: lane l reads column (l&31) => col-block (l>>4)&1,
  // reduction m = (l>>5)*8 + e => mblk offset (l>>5)*2 (+h)
  const unsigned trM32 =
      (unsigned)(((lane >> 4) & 1) * KBS + (lane >> 5) * 2 * TR_MBS +
                 (lane & 15) * 4) * 2;
  const unsigned aTrM = (unsigned)(unsigned long long)lA + trM32;
  const unsigned bTrM = (unsigned)(unsigned long long)lB + trM32;

  long chunk = blockIdx.z;
  int buf = 0;
  if (chunk < nChunks) {
    stage(0, chunk * CH);
    __syncthreads();  // drains the DMA (vmcnt 0) + barrier
  }
  for (; chunk < nChunks; chunk += splitm) {
    const long next = chunk + splitm;
    if (next < nChunks) stage(buf ^ 1, next * CH);  // DMA under the math
    const unsigned aOff = (unsigned)(buf * ABUF) * 2;
    const unsigned bOff = (unsigned)(buf * BBUF) * 2;
    if constexpr (M32) {
      // fine-grained per-kstep interleave: tr-read kstep k+1 while the
      // MFMAs of kstep k issue, with COUNTED lgkmcnt so waves drift apart
      // instead of entering barrier-aligned MFMA bursts together (PMC:
      // 61% SQ_WAIT_INST_ANY at only ~24% MFMA-pipe duty).
      constexpr int KST = CH / 16;  // 32x32x16 ksteps per chunk
      constexpr int RPK = 2 * (FK32 + FR32);  // tr reads per kstep
      bf16x4 aT[2][FK32][2], bT[2][FR32][2];  // 2-deep kstep ring
      auto rdk = [&](int kst, int ring) {
#pragma unroll
        for (int f = 0; f < FK32; ++f) {
          const unsigned base =
              aTrM + aOff + (unsigned)((wr * (BK / WR / 16) + f * 2) * KBS +
                                       kst * 4 * TR_MBS) * 2;
          aT[ring][f][0] = ds_tr16(base);
          aT[ring][f][1] = ds_tr16(base + TR_MBS * 2);
        }
#pragma unroll
        for (int f = 0; f < FR32; ++f) {
          const unsigned base =
              bTrM + bOff + (unsigned)((wc * (BR / WC / 16) + f * 2) * KBS +
                                       kst * 4 * TR_MBS) * 2;
          bT[ring][f][0] = ds_tr16(base);
          bT[ring][f][1] = ds_tr16(base + TR_MBS * 2);
        }
      };
      rdk(0, 0);
#pragma unroll
      for (int kst = 0; kst < KST; ++kst) {
        const int ring = kst & 1;
        if (kst + 1 < KST) rdk(kst + 1, ring ^ 1);
        // wait for THIS kstep's reads only; the next kstep's RPK stay
        // in flight under the MFMAs
        if (kst + 1 < KST)
          wait_lgkmcnt<RPK>();
        else
          wait_lgkmcnt<0>();
        __builtin_amdgcn_sched_barrier(0);

#pragma unroll
        for (int fa = 0; fa < FK32; ++fa)
#pragma unroll
          for (int fb = 0; fb < FR32; ++fb) {
            const bf16x8 av = __builtin_shufflevector(
                aT[ring][fa][0], aT[ring][fa][1], 0, 1, 2, 3, 4, 5, 6, 7);
            const bf16x8 bv = __builtin_shufflevector(
                bT[ring][fb][0], bT[ring][fb][1], 0, 1, 2, 3, 4, 5, 6, 7);
            acc32[fa][fb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
                av, bv, acc32[fa][fb], 0, 0, 0);
          }
      }
    } else {
      // tr-read ALL fragments for this chunk into registers (guide T10)
      bf16x4 aT[CH / 32][FK][2], bT[CH / 32][FR][2];
#pragma unroll
      for (int s2 = 0; s2 < CH / 32; ++s2) {
#pragma unroll
        for (int f = 0; f < FK; ++f) {
          const unsigned base = aTr0 + aOff +
                                (unsigned)((wr * FK + f) * KBS +
                                           s2 * 8 * TR_MBS) * 2;
          aT[s2][f][0] = ds_tr16(base);
          aT[s2][f][1] = ds_tr16(base + TR_MBS * 2);
        }
#pragma unroll
        for (int f = 0; f < FR; ++f) {
          const unsigned base = bTr0 + bOff +
                                (unsigned)((wc * FR + f) * KBS +
                                           s2 * 8 * TR_MBS) * 2;
          bT[s2][f][0] = ds_tr16(base);
          bT[s2][f][1] = ds_tr16(base + TR_MBS * 2);
        }
      }
      wait_lgkmcnt<0>();
      __builtin_amdgcn_sched_barrier(0);  // keep MFMAs below the wait
#pragma unroll
      for (int s2 = 0; s2 < CH / 32; ++s2)
#pragma unroll
        for (int fa = 0; fa < FK; ++fa)
#pragma unroll
          for (int fb = 0; fb < FR; ++fb) {
            const bf16x8 av = __builtin_shufflevector(
                aT[s2][fa][0], aT[s2][fa][1], 0, 1, 2, 3, 4, 5, 6, 7);
            const bf16x8 bv = __builtin_shufflevector(
                bT[s2][fb][0], bT[s2][fb][1], 0, 1, 2, 3, 4, 5, 6, 7);
            acc[fa][fb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                av, bv, acc[fa][fb], 0, 0, 0);
          }
    }
    if (next < nChunks) __syncthreads();  // drains DMA + joins waves
    buf ^= 1;
  }

  if constexpr (M32) {
    // ---- 32x32 epilogue: D col = lane&31 (rsc), row = (r&3) + 8*(r>>2)
    //      + 4*(lane>>5) (k) ----
#pragma unroll
    for (int fa = 0; fa < FK32; ++fa) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
        const int k = kt0 + wr * (BK / WR) + fa * 32 + row;
#pragma unroll
        for (int fb = 0; fb < FR32; ++fb)
          wgrad_scatter_add<KS>(
              dW, k, rt0 + wc * (BR / WC) + fb * 32 + (lane & 31),
              acc32[fa][fb][r], K, KG, C, Cp, log2Cp);
      }
    }
    return;
  }

  // ---- epilogue: scatter-add into NCHW fp32 dW ----
#pragma unroll
  for (int fa = 0; fa < FK; ++fa) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int k = kt0 + (wr * FK + fa) * 16 + lg * 4 + r;
#pragma unroll
      for (int fb = 0; fb < FR; ++fb)
        wgrad_scatter_add<KS>(dW, k, rt0 + (wc * FR + fb) * 16 + li,
                              acc[fa][fb][r], K, KG, C, Cp, log2Cp);
    }
  }
}

// ---------------------------------------------------------------------------
// Patch weight gradient: stage each X row segment ONCE and take the KS dx
// taps by shifted tr reads.
//
// k_conv_wgrad stages X once per tap (RS x the unique bytes) because its
// [col/16][m/4][4m][16col] image only admits 4m-aligned shifts. Here both
// operands are plain [pixel][channel] rows: ds_read_b64_tr_b16 takes a
// per-lane address of 4 contiguous elements of one row, so the fragment of
// tap dx is the dx=0 read with every lane moved by dx whole pixel rows —
// always 8-byte aligned.
//
//   - a block owns one BK k-tile, one CT channel tile, ONE dy tap row and a
//     contiguous slice of m-chunks; it accumulates all KS dx taps (KS
//     32x32 accumulator tiles per wave).
//   - an m-chunk is CH consecutive output pixels of one image row, so
//     (n, oy, ox0) is block-uniform: no per-lane division. Rows whose input
//     row oy+dy-PAD falls outside the image contribute nothing and are not
//     enumerated at all.
//   - per chunk: dY [CH][BK] once, the X patch [CH+KS-1][CT] of input row
//     oy+dy-PAD once (halo from global memory; lanes outside the image or
//     past the row end source the 16 B zero buffer).
//   - images: 64 B rows (32 channels) need no swizzle: 4 consecutive pixels
//     cover the 64 banks exactly. 128 B rows (64 channels) XOR byte-bit 6
//     with pixel-bit 1, so ANY 4 consecutive pixels (every dx shift) hit 4
//     distinct 64 B bank quarters. The XOR moves whole 16 B chunks, so the
//     glds image stays lane-linear with the swizzle on the SOURCE chunk.
//   - 4 waves = WR x WC 32x32 output quadrants x WK k-step interleave
//     (BK=CT=64: 2x2x1; BK=CT=32: 1x1x4, each wave every 4th k-step).
//   - per k-step: 2 A tr reads shared by all KS taps + 2*KS B tr reads,
//     KS v_mfma_f32_32x32x16_bf16, 2-deep ring with counted lgkmcnt.
//
// k_conv_wgrad_patch16 (below) is the same scheme for 16-channel images.
// Ownership, staging, the A tr base, the k-step ring and the slab epilogue
// are written once (PatchOwner, PatchStager, patch_a_base, patch_chunk_mma,
// patch_slab_drain, driven by wgrad_patch_body); a kernel supplies its Geo
// struct, its B-fragment policy (PatchTapFrags / PatchPairFrags) and the
// static_asserts about its own images.
// ---------------------------------------------------------------------------

// chunk-index XOR of a pixel row of the wgrad images (slot map: PatchImage,
// conv_common.h): byte bit 6 = chunk bit 2 with pixel bit 1 at 128 B rows
struct PtSwz {
  static constexpr int chunk_xor(int pix, int COLS) {
    return COLS == 64 ? ((pix >> 1) & 1) << 2 : 0;
  }
};
using PtImage = PatchImage<PtSwz>;
// the XOR as a byte offset inside a row, for the per-lane read bases
constexpr int pt_swz(int pix, int COLS) {
  return PtSwz::chunk_xor(pix, COLS) << 4;
}
// byte offset of (pixel row, column) inside a [pixel][COLS] bf16 image
constexpr int pt_off(int pix, int col, int COLS) {
  return PtImage::off(pix, col >> 3, COLS) + (col & 7) * 2;
}
// the 32x32x16 transposed read (per 32-lane half: 2 column blocks x 4
// pixel rows x 4 8-byte pieces) is bank-conflict-free at every pixel shift
constexpr bool pt_tr_conflict_free(int COLS, int maxShift) {
  for (int sh = 0; sh <= maxShift; ++sh)
    for (int c32 = 0; c32 < COLS / 32; ++c32) {
      unsigned long long used = 0;
      for (int l = 0; l < 32; ++l) {
        const int pix = sh + ((l & 15) >> 2);
        const int col = c32 * 32 + ((l >> 4) & 1) * 16 + (l & 3) * 4;
        const int a = pt_off(pix, col, COLS);
        if (a % 8 != 0) return false;
        const unsigned long long bits = 3ull << ((a / 4) % 64);
        if (used & bits) return false;
        used |= bits;
      }
    }
  return true;
}

// Tile constants of a patch kernel: BK x CT tile, chunks of CH pixels, NPX
// staged patch pixels per chunk. 4 waves = WR x WC 32x32 quadrants x WK
// k-step interleave. The waves walk PXA >= CH pixel rows (whole k-steps for
// each of the WK; PXA == CH where WK divides CH/16) and the images are staged
// that long, the rows past the chunk sourced from the zero buffer, so a
// padded k-step adds 0.
template <int KS_, int BK_, int CT_, int CH_, int NPX_>
struct PatchGeoBase {
  static constexpr int KS = KS_, BK = BK_, CT = CT_, CH = CH_, NPX = NPX_;
  static constexpr int WR = BK / 32, WC = CT >= 32 ? CT / 32 : 1;
  static constexpr int WK = 4 / (WR * WC);  // waves interleaving k-steps
  static constexpr int KST = CH / 16;       // k-steps per chunk
  static constexpr int KSTW = (KST + WK - 1) / WK;  // k-steps per wave
  static constexpr int PXA = KSTW * WK * 16;  // pixel rows the waves walk
  static constexpr int ACPR = BK / 8, BCPR = CT / 8;  // 16 B chunks per row
  static constexpr int ASLOTS = CH * ACPR, BSLOTS = NPX * BCPR;
  static constexpr int SA = (PXA * ACPR + 255) / 256;
  static constexpr int SB = ((PXA - CH + NPX) * BCPR + 255) / 256;
  static constexpr int ABYTES = SA * 256 * 16;  // padded: surplus slots stay
  static constexpr int BBYTES = SB * 256 * 16;  // inside
  static constexpr int SLABN = WR * 8 * CT * KS;  // floats per slab copy
  // staging double buffer, reused by the epilogue's WK slab copies
  static constexpr int LDS_BYTES =
      2 * (ABYTES + BBYTES) > WK * SLABN * 4 ? 2 * (ABYTES + BBYTES)
                                             : WK * SLABN * 4;
};

// 32/64-channel tiles: the patch is the chunk plus the 2*PAD halo
template <int KS, int BK, int CT, int CH>
struct PatchGeo : PatchGeoBase<KS, BK, CT, CH, CH + KS - 1> {};

// What a block owns: one dy tap row and the chunks [c0, c1) of the N * Hv *
// nSeg whose input row oy + dy - PAD lies inside the image, as the
// gridDim.z-way slice blockIdx.z. (n, oyv, seg) is the current chunk.
struct PatchOwner {
  int oyLo, Hv, c0, c1, n, oyv, seg;
  // false: nothing owned (block-uniform; nothing staged or read yet)
  WN_DEVFN bool init(int N, int H, int PAD, int dy_, int nSeg) {
    oyLo = max(0, PAD - dy_);
    Hv = min(H, H + PAD - dy_) - oyLo;
    if (Hv <= 0) return false;
    const int total = N * Hv * nSeg;
    const int per = (total + (int)gridDim.z - 1) / (int)gridDim.z;
    c0 = blockIdx.z * per;
    c1 = min(total, c0 + per);
    if (c0 >= c1) return false;
    n = c0 / (Hv * nSeg);
    oyv = (c0 - n * Hv * nSeg) / nSeg;
    seg = c0 - (n * Hv + oyv) * nSeg;
    return true;
  }
  WN_DEVFN void advance(int nSeg) {
    if (++seg == nSeg) {
      seg = 0;
      if (++oyv == Hv) { oyv = 0; ++n; }
    }
  }
  WN_DEVFN int oy() const { return oyLo + oyv; }
};

// glds staging of one chunk: dY [CH][BK] and the X patch [NPX][CT] of input
// row oy + dy - PAD. Slot -> (pixel row, source chunk) is fixed per thread;
// slots past the image, past the row end or outside the picture source the
// 16 B zero buffer.
template <class G>
struct PatchStager {
  static constexpr int PAD = G::KS / 2;
  const bf16_t *dY, *X, *zero;
  char *lA, *lB;  // 2 x ABYTES, 2 x BBYTES
  int H, W, Kp, Cp, kt0, ct0, dy_, tid;
  int aPix[G::SA], aCh[G::SA], bPix[G::SB], bCh[G::SB];

  WN_DEVFN void init_slots() {
#pragma unroll
    for (int s = 0; s < G::SA; ++s) {
      const int sg = tid + s * 256;
      aPix[s] = (sg < G::ASLOTS) ? PtImage::slot_pix(sg, G::BK)
                                 : (1 << 28);  // -> zero
      aCh[s] = PtImage::slot_chunk(sg, G::BK) * 8;
    }
#pragma unroll
    for (int s = 0; s < G::SB; ++s) {
      const int sg = tid + s * 256;
      bPix[s] = (sg < G::BSLOTS) ? PtImage::slot_pix(sg, G::CT) - PAD
                                 : (1 << 28);
      bCh[s] = PtImage::slot_chunk(sg, G::CT) * 8;
    }
  }
  WN_DEVFN void operator()(int buf, int n_, int oy, int sg_) const {
    const int ox0 = sg_ * G::CH;
    const long rowm = ((long)n_ * H + oy) * W;
    const long rowx = ((long)n_ * H + oy + dy_ - PAD) * W;
#pragma unroll
    for (int s = 0; s < G::SA; ++s) {
      const bf16_t* src = zero;
      const int ox = ox0 + aPix[s];
      if (ox < W) src = dY + (rowm + ox) * Kp + kt0 + aCh[s];
      __builtin_amdgcn_global_load_lds(
          src, lA + buf * G::ABYTES + (tid + s * 256) * 16, 16, 0, 0);
    }
#pragma unroll
    for (int s = 0; s < G::SB; ++s) {
      const bf16_t* src = zero;
      const int ix = ox0 + bPix[s];
      if (ix >= 0 && ix < W) src = X + (rowx + ix) * Cp + ct0 + bCh[s];
      __builtin_amdgcn_global_load_lds(
          src, lB + buf * G::BBYTES + (tid + s * 256) * 16, 16, 0, 0);
    }
  }
};

// Per-lane tr-read geometry. Lane l reads column (l&31) of its 32-wide
// block: 16-column half hb = (l>>4)&1, reduction pixels (l>>5)*8 + 4h + e;
// inside the 16-lane group, lane 4q+p addresses row q, columns 4p..4p+3.
// rowl is the lane's pixel row in its wave's first k-step.
struct PatchLane {
  int q, hb, rowl;
  WN_DEVFN PatchLane(int lane, int wk)
      : q((lane & 15) >> 2), hb((lane >> 4) & 1),
        rowl(wk * 16 + (lane >> 5) * 8 + q) {}
};
// A (dY) base: the pixel of a read is rowl + 16*kst + 4h, so q alone feeds
// the swizzle
template <int BK>
WN_DEVFN unsigned patch_a_base(const char* lA, PatchLane L, int lane, int wr) {
  const int acol2 = (wr * 32 + L.hb * 16 + (lane & 3) * 4) * 2;
  return (unsigned)(unsigned long long)lA +
         (unsigned)(L.rowl * BK * 2 + (acol2 ^ pt_swz(L.q, BK)));
}

// B fragments of a 32/64-channel patch: fragment t is tap dx = t, the dx = 0
// read moved t pixel rows. The pixel of a read is rowl + (16*kst + 4h + dx):
// only (q + dx) & 2 feeds the swizzle, so 4 bases (dx & 3) cover every shift.
template <int KS, int CT>
struct PatchTapFrags {
  static constexpr int NB = KS;
  unsigned b[4];
  int col;  // D column of the lane inside the CT tile
  WN_DEVFN PatchTapFrags(const char* lB, PatchLane L, int lane, int wc)
      : col(wc * 32 + (lane & 31)) {
    const int bcol2 = (wc * 32 + L.hb * 16 + (lane & 3) * 4) * 2;
#pragma unroll
    for (int c = 0; c < 4; ++c)
      b[c] = (unsigned)(unsigned long long)lB +
             (unsigned)(L.rowl * CT * 2 + (bcol2 ^ pt_swz(L.q + c, CT)));
  }
  WN_DEVFN PatchTapFrags at(unsigned bufOff) const {
    PatchTapFrags f = *this;
#pragma unroll
    for (int i = 0; i < 4; ++i) f.b[i] += bufOff;
    return f;
  }
  // LDS address of fragment t for the 4-pixel read at pixel p
  WN_DEVFN unsigned addr(int t, int p) const {
    return b[t & 3] + (unsigned)((p + t) * CT * 2);
  }
  // element r of every accumulator -> slab row [c][dx] of one k
  WN_DEVFN void scatter(float* row, const f32x16 (&acc)[NB], int r) const {
    float* dst = row + col * KS;
#pragma unroll
    for (int dx = 0; dx < KS; ++dx) dst[dx] = acc[dx][r];
  }
};

// One chunk's MFMAs: KSTW k-steps through a 2-deep ring of tr reads. Issue
// order inside a k-step is part of the algorithm: the two A reads, then the
// B fragments in ascending t, each as a (row, row+4) pair. LDS reads return
// in issue order, so waiting until RPK are outstanding retires exactly this
// k-step's reads and leaves the next one's in flight under the MFMAs.
template <class G, class BF>
WN_DEVFN void patch_chunk_mma(f32x16 (&acc)[BF::NB], unsigned aB,
                              const BF& bf) {
  constexpr int NB = BF::NB, BK = G::BK, WK = G::WK, KSTW = G::KSTW;
  constexpr int RPK = 2 + 2 * NB;  // tr reads per k-step
  bf16x4 aT[2][2], bT[2][NB][2];   // 2-deep k-step ring
  auto rdk = [&](int i, int ring) {
    const int p0 = i * WK * 16;  // first pixel of this wave's i-th k-step
    aT[ring][0] = ds_tr16(aB + (unsigned)(p0 * BK * 2));
    aT[ring][1] = ds_tr16(aB + (unsigned)((p0 + 4) * BK * 2));
#pragma unroll
    for (int t = 0; t < NB; ++t) {
      bT[ring][t][0] = ds_tr16(bf.addr(t, p0));
      bT[ring][t][1] = ds_tr16(bf.addr(t, p0 + 4));
    }
  };
  rdk(0, 0);
#pragma unroll
  for (int i = 0; i < KSTW; ++i) {
    const int ring = i & 1;
    if (i + 1 < KSTW) {
      rdk(i + 1, ring ^ 1);
      // lgkmcnt saturates at 15: KS = 7's 16 reads in flight wait for one
      // more than needed
      wait_lgkmcnt<(RPK < 15 ? RPK : 15)>();
    } else {
      wait_lgkmcnt<0>();
    }
    __builtin_amdgcn_sched_barrier(0);
    const bf16x8 av = __builtin_shufflevector(aT[ring][0], aT[ring][1], 0, 1,
                                              2, 3, 4, 5, 6, 7);
#pragma unroll
    for (int t = 0; t < NB; ++t) {
      const bf16x8 bv = __builtin_shufflevector(
          bT[ring][t][0], bT[ring][t][1], 0, 1, 2, 3, 4, 5, 6, 7);
      acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(av, bv, acc[t], 0, 0,
                                                       0);
    }
  }
}

// Slab j ([WR*8 k][CT c][KS dx] floats, WK copies) -> dW: sum the copies in
// order w = 0..WK-1 and add; consecutive threads add to consecutive addresses.
template <class G>
WN_DEVFN void patch_slab_drain(const float* slab, float* dW, int j, int kt0,
                               int ct0, int dy_, int K, int C, int tid) {
  constexpr int KS = G::KS, CT = G::CT, WK = G::WK, SLABN = G::SLABN;
  for (int e = tid; e < SLABN; e += 256) {
    float v = slab[e];
#pragma unroll
    for (int w = 1; w < WK; ++w) v += slab[w * SLABN + e];
    const int kk = e / (CT * KS);
    const int rem = e - kk * (CT * KS);
    const int cc = rem / KS;
    const int dx = rem - cc * KS;
    const int k = kt0 + (kk >> 3) * 32 + j * 8 + (kk & 7);
    const int cch = ct0 + cc;
    if (k < K && cch < C)
      atomicAdd(&dW[(((long)k * C + cch) * KS + dy_) * KS + dx], v);
  }
}

// The patch kernels' body. ct0 / dy_: the block's channel tile and tap row.
template <class G, class BF>
WN_DEVFN void wgrad_patch_body(const bf16_t* __restrict__ dY,
                               const bf16_t* __restrict__ X,
                               float* __restrict__ dW, int N, int H, int W,
                               int Cp, int Kp, int K, int C, int nSeg,
                               const bf16_t* __restrict__ Zero16w, int ct0,
                               int dy_) {
  static_assert(WN_MFMA_KMAP == 0, "wgrad staging assumes KMAP 0");
  static_assert(G::BK == 32 || G::BK == 64);
  static_assert(G::CH % 16 == 0);
  constexpr int KS = G::KS, BK = G::BK, CT = G::CT;
  constexpr int WR = G::WR, WC = G::WC, SLABN = G::SLABN;

  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* lA = smem;                  // 2 x ABYTES
  char* lB = smem + 2 * G::ABYTES;  // 2 x BBYTES

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wid = tid >> 6;
  const int wk = wid / (WR * WC);
  const int wr = (wid % (WR * WC)) / WC;
  const int wc = wid % WC;
  const int kt0 = blockIdx.x * BK;

  PatchOwner own;
  if (!own.init(N, H, KS / 2, dy_, nSeg)) return;
  PatchStager<G> stage{dY, X, Zero16w, lA, lB, H, W, Kp, Cp, kt0, ct0, dy_,
                       tid};
  stage.init_slots();

  f32x16 acc[BF::NB];
#pragma unroll
  for (int t = 0; t < BF::NB; ++t)
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[t][e] = 0.f;

  const PatchLane L(lane, wk);
  const unsigned aB0 = patch_a_base<BK>(lA, L, lane, wr);
  const BF bf0(lB, L, lane, wc);

  int buf = 0;
  stage(0, own.n, own.oy(), own.seg);
  __syncthreads();  // drains the DMA (vmcnt 0) + barrier
  for (int c = own.c0; c < own.c1; ++c) {
    own.advance(nSeg);
    if (c + 1 < own.c1)
      stage(buf ^ 1, own.n, own.oy(), own.seg);  // DMA under the math
    patch_chunk_mma<G>(acc, aB0 + (unsigned)(buf * G::ABYTES),
                       bf0.at((unsigned)(buf * G::BBYTES)));
    if (c + 1 < own.c1) __syncthreads();  // drains DMA + joins waves
    buf ^= 1;
  }

  // ---- epilogue: D col = lane&31 (c), row = (r&3) + 8*(r>>2) +
  //      4*(lane>>5) (k). The kernel is bound by the fp32 atomics, not the
  //      math: straight from the D layout every lane of an atomic hits its
  //      own cache line (c stride = KS*KS floats). So the tile goes through
  //      LDS in 4 slabs of WR*8 k rows laid out [k][c][dx] — dW's own order
  //      for one dy — the WK k-step waves' partial sums are added on the
  //      way out, and consecutive lanes add to consecutive addresses. The
  //      WK slab copies reuse the staging buffers (LDS_BYTES covers both). ----
  float* slab = reinterpret_cast<float*>(smem);
  __syncthreads();  // every wave is past its last tr read; no DMA in flight
#pragma unroll
  for (int j = 0; j < 4; ++j) {
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) {
      const int kk = wr * 8 + rr + 4 * (lane >> 5);
      bf0.scatter(slab + wk * SLABN + kk * CT * KS, acc, 4 * j + rr);
    }
    __syncthreads();
    patch_slab_drain<G>(slab, dW, j, kt0, ct0, dy_, K, C, tid);
    __syncthreads();
  }
}

template <int KS, int BK, int CT, int CH>
__global__ __launch_bounds__(256, 2) void k_conv_wgrad_patch(
    const bf16_t* __restrict__ dY,  // (N,H,W,Kp)
    const bf16_t* __restrict__ X,   // (N,H,W,Cp)
    float* __restrict__ dW,         // (K, C, KS, KS) fp32, accumulated into
    int N, int H, int W, int Cp, int Kp, int K, int C, int nSeg,
    const bf16_t* __restrict__ Zero16w) {
  using G = PatchGeo<KS, BK, CT, CH>;
  static_assert(CT == 32 || CT == 64);
  static_assert(G::KST % G::WK == 0 && G::PXA == CH);
  static_assert(PtImage::linear(CH, BK) && PtImage::linear(G::NPX, CT),
                "glds slot order != image chunk order");
  static_assert(pt_tr_conflict_free(BK, 12) &&
                    pt_tr_conflict_free(CT, KS - 1 + 12),
                "tr read bank conflict");
  // last pixel row a tr read touches: last k-step, upper lane half, second
  // 4-pixel read, row 3 (+ the last dx for the patch); the swizzle stays
  // inside a row, so the row end bounds every lane address
  static_assert((CH - 16 + 8 + 4 + 3 + 1) * BK * 2 <= G::ASLOTS * 16);
  static_assert((CH - 16 + 8 + 4 + 3 + (KS - 1) + 1) * CT * 2 <=
                G::BSLOTS * 16);
  // all WK slab copies: 4096*KS bytes
  static_assert(G::WK * G::SLABN * 4 == 4096 * KS);
  wgrad_patch_body<G, PatchTapFrags<KS, CT>>(
      dY, X, dW, N, H, W, Cp, Kp, K, C, nSeg, Zero16w,
      (int)(blockIdx.y / KS) * CT, (int)(blockIdx.y % KS));
}


// ---------------------------------------------------------------------------
// Patch weight gradient for Cp = 16 (the 12->128 / 6->32 input convs): two
// taps per MFMA.
//
// A 32-column fragment of a 16-channel image would be half padding. But a
// pixel row of the [pixel][16] patch is 32 bytes, so two neighbouring pixels
// are 32 contiguous channels: the transposed read at pixel shift dx with row
// stride 16 elements delivers pixel p+dx in its low 16 columns and pixel
// p+dx+1 in its high 16 — tap dx and tap dx+1 of the same 16 channels. One
// 32x32x16 MFMA therefore accumulates D column c' = tap dx + (c' >> 4),
// channel c' & 15, and shifts 0, 2, .. cover KS taps in (KS+1)/2
// accumulators. For odd KS the high half of the last one is a phantom tap
// dx = KS: the patch is one pixel longer (NPX = CH + KS) so its reads stay
// inside the staged image, and the epilogue drops it.
//
// Ownership, chunking, staging and the slab epilogue are those of
// k_conv_wgrad_patch with a single channel tile. 4 waves = WR 32-row k
// quadrants x WK k-step interleave (BK=64: 2x2, BK=32: 1x4). CH/16 need not
// divide by WK: the images are staged PXA >= CH pixel rows long, the surplus
// rows of dY sourced from the zero buffer, so a padded k-step adds 0.
// ---------------------------------------------------------------------------

// the pair read: inside a 32-lane half the upper 16 lanes read one pixel row
// further than the lower 16, so lanes share addresses (pixels q+1..q+3).
// Identical addresses are one access; distinct ones must not share a bank.
constexpr bool pt_tr_pair_conflict_free(int maxShift) {
  for (int sh = 0; sh <= maxShift; ++sh) {
    int addr[32] = {};
    for (int l = 0; l < 32; ++l) {
      const int pix = sh + ((l & 15) >> 2) + ((l >> 4) & 1);
      const int a = pt_off(pix, (l & 3) * 4, 16);
      if (a % 8 != 0) return false;
      for (int m = 0; m < l; ++m)
        if (addr[m] != a && (addr[m] / 8) % 32 == (a / 8) % 32) return false;
      addr[l] = a;
    }
  }
  return true;
}

// 16-channel tile: the patch is the chunk plus the 2*PAD halo and the
// phantom pixel
template <int KS, int BK, int CH>
struct Patch16Geo : PatchGeoBase<KS, BK, 16, CH, CH + KS> {};

// B fragments of the 16-channel patch: fragment t is the tap pair (2t, 2t+1),
// the read moved 2t pixel rows. 32 B rows carry no swizzle, so one base
// serves every shift; the 16-column half hb is one whole pixel row further on.
template <int KS>
struct PatchPairFrags {
  static constexpr int NB = (KS + 1) / 2, CT = 16;  // tap-pair accumulators
  unsigned b;
  int col, hb;  // D column c' of the lane: channel c' & 15, pair half c' >> 4
  WN_DEVFN PatchPairFrags(const char* lB, PatchLane L, int lane, int)
      : b((unsigned)(unsigned long long)lB +
          (unsigned)((L.rowl + L.hb) * CT * 2 + (lane & 3) * 8)),
        col(lane & 15), hb(L.hb) {}
  WN_DEVFN PatchPairFrags at(unsigned bufOff) const {
    PatchPairFrags f = *this;
    f.b += bufOff;
    return f;
  }
  WN_DEVFN unsigned addr(int t, int p) const {
    return b + (unsigned)((p + 2 * t) * CT * 2);
  }
  // accumulator t holds taps 2t + hb; the phantom tap dx = KS is not written
  WN_DEVFN void scatter(float* row, const f32x16 (&acc)[NB], int r) const {
    float* dst = row + col * KS + hb;
#pragma unroll
    for (int t = 0; t < NB; ++t)
      if (2 * t + 1 < KS || hb == 0) dst[2 * t] = acc[t][r];
  }
};

template <int KS, int BK, int CH>
__global__ __launch_bounds__(256, 2) void k_conv_wgrad_patch16(
    const bf16_t* __restrict__ dY,  // (N,H,W,Kp)
    const bf16_t* __restrict__ X,   // (N,H,W,16)
    float* __restrict__ dW,         // (K, C, KS, KS) fp32, accumulated into
    int N, int H, int W, int Kp, int K, int C, int nSeg,
    const bf16_t* __restrict__ Zero16w) {
  using G = Patch16Geo<KS, BK, CH>;
  constexpr int CT = G::CT;
  static_assert(PtImage::linear(CH, BK) && PtImage::linear(G::NPX, CT),
                "glds slot order != image chunk order");
  static_assert(pt_tr_conflict_free(BK, 12) &&
                    pt_tr_pair_conflict_free(KS - 1 + 12),
                "tr read bank conflict");
  // last pixel row a tr read of a real k-step touches: last k-step, upper
  // lane half, second 4-pixel read, row 3 (+ the last shift and the pair's
  // second pixel for the patch) — inside the staged, defined image
  static_assert((CH - 16 + 8 + 4 + 3 + 1) * BK * 2 <= G::ASLOTS * 16);
  static_assert((CH - 16 + 8 + 4 + 3 + (KS - 1) + 1 + 1) * CT * 2 <=
                G::BSLOTS * 16);
  // the same for the padded k-steps: inside the zero-sourced surplus slots
  static_assert(G::PXA * BK * 2 <= G::ABYTES &&
                (G::PXA + KS) * CT * 2 <= G::BBYTES);
  wgrad_patch_body<G, PatchPairFrags<KS>>(dY, X, dW, N, H, W, CT, Kp, K, C,
                                          nSeg, Zero16w, 0, (int)blockIdx.y);
}

// ---------------------------------------------------------------------------
// Small-K weight gradient (K <= 4: the 64->3 / 32->3 output convs).
// The MFMA path wastes 13/16 rows of every fragment on Kp padding there;
// a VALU outer-product reduction is ~10x cheaper. Each block owns one
// (tap, m-slice); thread t owns channel octet t % (Cp/8) and accumulates
// acc[K][8] in registers over its m rows, LDS-reduces across the m-rows
// sharing the octet, then atomically adds into the fp32 dW.
// ---------------------------------------------------------------------------

// reduction scratch: one row of 256 threads per (k, e) partial sum
template <int KMAX>
struct SmallKGeo {
  static constexpr int RED_ROWS = KMAX * 8;
  static constexpr int LDS_BYTES = RED_ROWS * 256 * (int)sizeof(float);
};

template <int KMAX, int U>
__global__ __launch_bounds__(256, 4) void k_wgrad_smallk(
    const bf16_t* __restrict__ dY,  // (M, Kp)
    const bf16_t* __restrict__ X,   // (N,H,W,Cp)
    float* __restrict__ dW,         // (K, C, KS, KS) fp32
    int N, int H, int W, int Cp, int log2Cp, int Kp, int K, int C, int KS,
    int msplit, unsigned long long mulHW, unsigned long long mulW) {
  static_assert(KMAX == 4, "the dY row is read as one 8-byte vector");
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* red = reinterpret_cast<float*>(smem);  // [RED_ROWS][256]
  constexpr int RED_ROWS = SmallKGeo<KMAX>::RED_ROWS;
  const int PAD = KS / 2;
  const long M = (long)N * H * W;
  const int HW = H * W;
  const int cg = threadIdx.x & (Cp / 8 - 1);   // channel octet
  const int mr = threadIdx.x / (Cp / 8);       // m-row lane
  const int MR = 256 / (Cp / 8);
  const int tap = blockIdx.x;
  const int dy_ = tap / KS, dx_ = tap - dy_ * KS;

  float acc[KMAX][8] = {};
  const long rows = (M + msplit - 1) / msplit;
  const long mstart = (long)blockIdx.y * rows;
  const long mend = min(mstart + rows, M);
  // The loop is bound by load latency, not by bytes or FMAs: every
  // iteration issues the X and dY loads of U rows before the first FMA that
  // needs one, so U loads per thread are in flight instead of one.
  for (long m0 = mstart + mr; m0 < mend; m0 += (long)U * MR) {
    bf16x8 xv[U];
    bf16x4 dv[U];
    float mask[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      // branch-free tail: rows past the slice re-read its last row, masked
      const long mu = m0 + (long)u * MR;
      const long m = min(mu, mend - 1);
      unsigned n = magic_div((unsigned)m, mulHW);
      unsigned rem = (unsigned)m - n * (unsigned)HW;
      unsigned oy = magic_div(rem, mulW);
      int ox = (int)(rem - oy * (unsigned)W);
      int iy = (int)oy + dy_ - PAD, ix = ox + dx_ - PAD;
      // branch-free halo: clamped load + zero mask — a `continue` here makes
      // hipcc branch around the loads and drain vmcnt per element (guide §5
      // trap 4c), serializing the whole m loop on load latency
      const bool valid =
          mu < mend && iy >= 0 && iy < H && ix >= 0 && ix < W;
      const int iyc = min(max(iy, 0), H - 1), ixc = min(max(ix, 0), W - 1);
      xv[u] = *reinterpret_cast<const bf16x8*>(
          X + (((long)((int)n * H + iyc) * W + ixc) << log2Cp) + cg * 8);
      dv[u] = *reinterpret_cast<const bf16x4*>(dY + m * Kp);  // Kp >= 16
      mask[u] = valid ? 1.f : 0.f;
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
#pragma unroll
      for (int k = 0; k < KMAX; ++k) {
        const float d = mask[u] * bf2f(dv[u][k]);
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[k][e] += d * bf2f(xv[u][e]);
      }
    }
  }
  // red is [k*8+e][thread]: consecutive lanes touch consecutive words, so
  // neither the stores nor the tree conflict (thread-major rows of 32
  // floats put every lane of a wave on two banks and made this epilogue,
  // not the m loop, the larger part of a block's time)
  const int tid = threadIdx.x;  // == mr * CG + cg
#pragma unroll
  for (int k = 0; k < KMAX; ++k)
#pragma unroll
    for (int e = 0; e < 8; ++e) red[(k * 8 + e) * 256 + tid] = acc[k][e];
  __syncthreads();
  // parallel tree reduce over the MR m-rows sharing each channel octet
  const int CG = Cp / 8;
  for (int s = MR / 2; s > 0; s >>= 1) {
    if (mr < s) {
#pragma unroll
      for (int j = 0; j < RED_ROWS; ++j)
        red[j * 256 + tid] += red[j * 256 + tid + s * CG];
    }
    __syncthreads();
  }
  // row j of red now holds its CG octet sums in columns 0..CG-1
  for (int t = tid; t < RED_ROWS * CG; t += 256) {
    const int j = t / CG, g = t - j * CG;
    const int k = j >> 3, c = g * 8 + (j & 7);
    if (k < K && c < C)
      atomicAdd(&dW[(((long)k * C + c) * KS + dy_) * KS + dx_],
                red[j * 256 + g]);
  }
}

// ---------------------------------------------------------------------------
// tr-read semantics probe: one wave fills a tr image with addr-coded values
// via the SAME writeTiles addressing (tr_addr), tr-reads fragments the same
// way wgrad does, and writes what each (lane, frag, elem) received. The
// host test checks element (lane g*16+i, reg j) == value coded (m=..,col=..).
// ---------------------------------------------------------------------------

__global__ void k_probe_tr(float* __restrict__ out /* [64][2][4] */) {
  __shared__ __attribute__((aligned(16))) bf16_t img[2 * TR_KBS];
  const int lane = threadIdx.x & 63;
  // fill 64 m x 32 col with value m*100 + col (bf16-exact for m<..,col<32)
  for (int m = lane; m < 64; m += 64)
    for (int col = 0; col < 32; ++col)
      img[tr_addr(m, col)] = f2bf((float)(m * 100 + col));
  __syncthreads();
  const int lg = lane >> 4, li = lane & 15;
  const unsigned base0 = (unsigned)(unsigned long long)img +
                         (unsigned)(2 * lg * TR_MBS + li * 4) * 2;
#pragma unroll
  for (int f = 0; f < 2; ++f) {  // two col-blocks (kblk 0, 1)
    const unsigned b = base0 + (unsigned)(f * TR_KBS) * 2;
    bf16x4 lo = ds_tr16(b);
    bf16x4 hi = ds_tr16(b + TR_MBS * 2);
    wait_lgkmcnt<0>();
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      out[(lane * 2 + f) * 8 + j] = bf2f(lo[j]);
      out[(lane * 2 + f) * 8 + 4 + j] = bf2f(hi[j]);
    }
  }
}

// Raw semantics probe: linear image img[e] = e; lane l reads 8 B at
// byte offset l*8 (elements 4l..4l+3). out[l][j] = delivered element
// index — exposes the hardware's lane/element permutation directly.
__global__ void k_probe_tr_raw(float* __restrict__ out /* [64][4] */) {
  __shared__ __attribute__((aligned(16))) bf16_t img[256];
  const int lane = threadIdx.x & 63;
  for (int e = lane; e < 256; e += 64) img[e] = f2bf((float)e);
  __syncthreads();
  const unsigned addr =
      (unsigned)(unsigned long long)img + (unsigned)lane * 8;
  bf16x4 v = ds_tr16(addr);
  wait_lgkmcnt<0>();
#pragma unroll
  for (int j = 0; j < 4; ++j) out[lane * 4 + j] = bf2f(v[j]);
}

at::Tensor probe_tr() {
  auto out = at::zeros({64, 2, 8}, at::TensorOptions()
                                       .dtype(at::kFloat)
                                       .device(at::kCUDA));
  hipStream_t stream = at::cuda::getCurrentHIPStream();
  hipLaunchKernelGGL(k_probe_tr, dim3(1), dim3(64), 0, stream,
                     out.data_ptr<float>());
  HIP_CHECK_LAST();
  return out;
}

at::Tensor probe_tr_raw() {
  auto out = at::zeros({64, 4}, at::TensorOptions()
                                    .dtype(at::kFloat)
                                    .device(at::kCUDA));
  hipStream_t stream = at::cuda::getCurrentHIPStream();
  hipLaunchKernelGGL(k_probe_tr_raw, dim3(1), dim3(64), 0, stream,
                     out.data_ptr<float>());
  HIP_CHECK_LAST();
  return out;
}

// ---------------------------------------------------------------------------
// Bias gradient: db[k] = sum_m dY[m][k]
// ---------------------------------------------------------------------------

// Each thread owns one 8-wide k-group and vector-loads bf16x8 rows of dY,
// accumulating 8 fp32 partials in registers; threads covering the same
// k-group at different m-phases reduce through LDS, then each block writes
// a plain fp32 partial slab Part[blockIdx.y][Kp] (no atomics — dB is a few
// cache lines and msplit*K atomics serialize on them; measured 2.2 ms ->
// slabs + the tiny reduce below). Grid: (ceil(ngrp/KGR), msplit).
struct BiasGradGeo {
  static constexpr int RED_COLS = 8;  // fp32 partials per thread
  static constexpr int LDS_BYTES = 256 * RED_COLS * (int)sizeof(float);
};

__global__ void k_bias_grad(const bf16_t* __restrict__ dY,
                            float* __restrict__ Part, long M, int Kp,
                            int msplit) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* red = reinterpret_cast<float*>(smem);  // [256][RED_COLS] fp32
  constexpr int RED_COLS = BiasGradGeo::RED_COLS;
  const int ngrp = Kp >> 3;                  // 8-wide k-groups in Kp
  const int KGR = min(ngrp, 32);             // k-groups per block
  const int MR = 256 / KGR;                  // m-rows strided per block
  const int kg = threadIdx.x % KGR;          // group id (fastest: coalesced)
  const int mr = threadIdx.x / KGR;
  const int k0 = (blockIdx.x * KGR + kg) * 8;

  float acc[8] = {};
  const long rows = (M + msplit - 1) / msplit;
  const long mstart = (long)blockIdx.y * rows;
  const long mend = min(mstart + rows, M);
  if (k0 < Kp) {
    for (long m = mstart + mr; m < mend; m += MR) {
      const bf16x8 v = *reinterpret_cast<const bf16x8*>(dY + m * Kp + k0);
#pragma unroll
      for (int e = 0; e < 8; ++e) acc[e] += bf2f(v[e]);
    }
  }
#pragma unroll
  for (int e = 0; e < 8; ++e) red[threadIdx.x * RED_COLS + e] = acc[e];
  __syncthreads();
  // tree-reduce over the MR rows that share this thread's k-group
  if (mr == 0 && k0 < Kp) {
#pragma unroll 1
    for (int r = 1; r < MR; ++r)
#pragma unroll
      for (int e = 0; e < 8; ++e) acc[e] += red[(r * KGR + kg) * RED_COLS + e];
    *reinterpret_cast<f32x4*>(&Part[(long)blockIdx.y * Kp + k0]) =
        f32x4{acc[0], acc[1], acc[2], acc[3]};
    *reinterpret_cast<f32x4*>(&Part[(long)blockIdx.y * Kp + k0 + 4]) =
        f32x4{acc[4], acc[5], acc[6], acc[7]};
  }
}

// Reduce the [msplit][Kp] partials into dB (accumulating, like the old
// atomic path: dB may hold a pre-existing gradient). One block per output
// column, 256 threads strided over the msplit rows + LDS tree reduce.
__global__ void k_bias_grad_reduce(const float* __restrict__ Part,
                                   float* __restrict__ dB, int Kp, int K,
                                   int msplit) {
  __shared__ float red[256];
  const int k = blockIdx.x;
  float s = 0.f;
  for (int r = threadIdx.x; r < msplit; r += 256)
    s += Part[(long)r * Kp + k];
  red[threadIdx.x] = s;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if (threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x == 0) dB[k] += red[0];
}
// ---------------------------------------------------------------------------
// Host-side dispatch
// ---------------------------------------------------------------------------

namespace {

// k_wgrad_smallk launch shape: blocks over (tap, m-slice) and rows in flight
// per thread (sweep: docs/KERNELS.md, small-K section).
constexpr int WGRAD_SMALLK_BLOCKS = 768;
constexpr double WGRAD_SMALLK_BLOCKS_K = 0.17;
constexpr int WGRAD_SMALLK_U = 4;

// Patch kernels' split-m rule: blocks = K * sqrt(work/tile), capped. The
// patch16 tile (BK*16*KS atomics) is 4x smaller than 64x64, so more blocks
// pay.
constexpr double WGRAD_PATCH_BLOCKS_K = 110.0;
constexpr int WGRAD_PATCH_BLOCKS_MAX = 768;
constexpr double WGRAD_PATCH16_BLOCKS_K = 80.0;
constexpr int WGRAD_PATCH16_BLOCKS_MAX = 1024;

constexpr int WG_CH = 64;  // k_conv_wgrad m rows per chunk (glds double-buffer
                           // budget)

// Which weight-gradient kernel a conv shape runs on, and on what grid. The
// single source of the dispatch rule: conv2d_wgrad launches what wgrad_plan
// returns and conv2d_wgrad_plan reports it to the tests.
enum WgradKernel {
  WG_SMALLK = 0,
  WG_PATCH = 1,
  WG_PATCH16 = 2,
  WG_GENERIC = 3,    // k_conv_wgrad, 32x32x16 MFMA
  WG_GENERIC16 = 4   // k_conv_wgrad, 16x16x32 MFMA (BK = 16 or WN_WGRAD_M32=0)
};

struct WgradPlan {
  WgradKernel kernel;
  int BK;          // k tile (small-K: its KMAX = 4 rows)
  int gx, gy, gz;  // the grid launched; gz is the split-m count (small-K:
                   // gx taps x gy m-slices, gz = 1)
  int cls;         // patch kernels: channel class 64 / 32 / 16
  int ch;          // patch kernels: chunk length 64 / 112
  int unroll;      // small-K: rows in flight per thread
};

// Split-m block count of the patch kernels. Their time is main loop +
// epilogue atomics: T(blocks) ~ a*work/blocks + b*blocks*tile, with work =
// gx*gy*chunks*k-steps and tile = atomics per block, so the optimum is
// blocks ~ k * sqrt(work/tile), up to `cap` (beyond ~3 resident blocks per CU
// more blocks only add atomics). k and cap are fitted per kernel to block
// sweeps at 112^2 and 256^2 (docs/KERNELS.md). WN_WGRAD_PATCH_BLOCKS
// overrides the count for A/B sweeps. Returns gridDim.z.
inline int patch_split(double work, int tile, int gxgy, double k, int cap,
                       long maxChunks) {
  int blocks = std::min((int)(k * std::sqrt(work / tile)), cap);
  if (const char* be = getenv("WN_WGRAD_PATCH_BLOCKS")) blocks = atoi(be);
  const int split = std::max(1, (blocks + gxgy / 2) / gxgy);
  return (int)std::min<long>(split, maxChunks);
}

// WN_WGRAD_PATCH=0, read once per process, forces k_conv_wgrad wherever a
// patch kernel would run.
inline bool wgrad_patch_off() {
  static const bool off = [] {
    const char* e = getenv("WN_WGRAD_PATCH");
    return e != nullptr && atoi(e) == 0;
  }();
  return off;
}
// WN_WGRAD_M32, read once per process: default ON; 0 = the 16x16x32 path.
inline bool wgrad_m32() {
  static const bool m32 = [] {
    const char* e = getenv("WN_WGRAD_M32");
    return e == nullptr || atoi(e) != 0;
  }();
  return m32;
}

inline WgradPlan wgrad_plan(int N, int H, int W, int Cp, int Kp, int K,
                            int ks) {
  WgradPlan p{};
  const long M = (long)N * H * W;
  if (K <= 4) {  // output convs (K=3): VALU outer-product path
    const int RS = ks * ks;
    // m-slices per tap. A block pays a fixed LDS tree reduce + atomics, so
    // T(blocks) ~ a*work/blocks + b*blocks as for the patch kernel: blocks ~
    // sqrt(work) with work = taps * rows * channel octets, up to one resident
    // wave of blocks (more only queue behind it). WN_WGRAD_SMALLK_MSPLIT /
    // WN_WGRAD_SMALLK_U override the slice count and the rows in flight per
    // thread for A/B sweeps (docs/KERNELS.md has the sweep); read per call.
    const double work = (double)RS * N * H * W * (Cp / 8);
    const int blocks = std::min(
        WGRAD_SMALLK_BLOCKS, (int)(WGRAD_SMALLK_BLOCKS_K * std::sqrt(work)));
    int msplit = std::max(1, blocks / RS);
    if (const char* me = getenv("WN_WGRAD_SMALLK_MSPLIT"))
      msplit = std::max(1, atoi(me));
    p.unroll = WGRAD_SMALLK_U;
    if (const char* ue = getenv("WN_WGRAD_SMALLK_U")) p.unroll = atoi(ue);
    const int MR = 256 / (Cp / 8);
    msplit = (int)std::min<long>(msplit, (M + MR - 1) / MR);
    p.kernel = WG_SMALLK;
    p.BK = 4;
    p.gx = RS;
    p.gy = msplit;
    p.gz = 1;
    return p;
  }
  // Patch kernel (one X row segment staged once for all KS dx taps) for
  // every channel class it is instantiated for: each measured faster than
  // k_conv_wgrad on MI355X, the Cp = 16 tap-pair classes included (table:
  // docs/KERNELS.md, wgrad section). cls: 64 (Cp and Kp multiples of 64),
  // 32 (32 -> 32) or 16 (Cp = 16).
  const int cls = (Cp % 64 == 0 && Kp % 64 == 0)             ? 64
                  : (Cp == 32 && Kp == 32)                   ? 32
                  : (Cp == 16 && (Kp == 32 || Kp % 64 == 0)) ? 16
                                                             : 0;
  if (!wgrad_patch_off() && ks >= 3 && cls != 0) {
    // chunk length: the instantiated CH that pads a row the least (112 = 7
    // k-steps covers the flagship's 112-pixel rows exactly; 64 divides the
    // 256/512 widths). WN_WGRAD_PATCH_CH overrides it for tests and A/B
    // runs; it is read per call so one process can exercise both.
    const char* fe = getenv("WN_WGRAD_PATCH_CH");
    const int force_ch = fe ? atoi(fe) : 0;
    int ch = 64;
    if (cls == 64 || cls == 16) {
      const int pad64 = (W + 63) / 64 * 64, pad112 = (W + 111) / 112 * 112;
      ch = (pad112 < pad64) ? 112 : 64;
      if (force_ch == 64 || force_ch == 112) ch = force_ch;
    }
    // tile: BK x CT of one dy row; cls 16: Kp = 32 or n*64
    const int BK = cls == 64 ? 64 : cls == 32 ? 32 : (Kp == 32 ? 32 : 64);
    const int CT = cls;
    const int nSeg = (W + ch - 1) / ch;
    p.kernel = cls == 16 ? WG_PATCH16 : WG_PATCH;
    p.BK = BK;
    p.cls = cls;
    p.ch = ch;
    p.gx = Kp / BK;
    p.gy = (Cp / CT) * ks;
    const double work = (double)p.gx * p.gy * N * H * nSeg * (ch / 16);
    // a block's atomics: its BK x CT tile of one dy row
    p.gz = cls == 16
               ? patch_split(work, BK * CT * ks, p.gx * p.gy,
                             WGRAD_PATCH16_BLOCKS_K, WGRAD_PATCH16_BLOCKS_MAX,
                             (long)N * H * nSeg)
               : patch_split(work, BK * CT * ks, p.gx * p.gy,
                             WGRAD_PATCH_BLOCKS_K, WGRAD_PATCH_BLOCKS_MAX,
                             (long)N * H * nSeg);
    return p;
  }
  const int KG = ks * ks * Cp;
  p.BK = std::min(Kp, 128);
  p.gx = (Kp + p.BK - 1) / p.BK;
  p.gy = (KG + 127) / 128;
  // split so gx*gy*split fills 256 CUs x ~3 resident blocks
  const int split = std::max(1, 640 / std::max(1, p.gx * p.gy));
  const long nChunks = (M + WG_CH - 1) / WG_CH;
  p.gz = (int)std::min<long>(split, nChunks);
  // the 32x32 MFMA path exists for BK >= 32
  p.kernel = (p.BK >= 32 && wgrad_m32()) ? WG_GENERIC : WG_GENERIC16;
  return p;
}

// Launch of a patch kernel with tile constants G on the plan's grid. cp is
// the kernel's Cp argument: k_conv_wgrad_patch takes one,
// k_conv_wgrad_patch16 (Cp = 16) has none.
template <class G, class Kern, class... CpArg>
void launch_wgrad_patch_t(Kern kern, const WgradPlan& plan,
                          const at::Tensor& dy, const at::Tensor& x,
                          at::Tensor& dw, const bf16_t* zero16,
                          hipStream_t stream, CpArg... cp) {
  const int N = x.size(0), H = x.size(1), W = x.size(2);
  const int Kp = dy.size(3);
  const int K = dw.size(0), C = dw.size(1);
  TORCH_INTERNAL_ASSERT(G::BK == plan.BK && G::CT == plan.cls &&
                        (G::CH == plan.ch || plan.cls == 32));
  const int nSeg = (W + G::CH - 1) / G::CH;
  hipLaunchKernelGGL(kern, dim3(plan.gx, plan.gy, plan.gz), dim3(256),
                     (size_t)G::LDS_BYTES, stream,
                     (const bf16_t*)dy.data_ptr(),
                     (const bf16_t*)x.data_ptr(), dw.data_ptr<float>(), N, H,
                     W, cp..., Kp, K, C, nSeg, zero16);
}

void launch_wgrad_patch(const at::Tensor& dy, const at::Tensor& x,
                        at::Tensor& dw, int ks, const WgradPlan& plan,
                        const bf16_t* zero16, hipStream_t stream) {
  const int Cp = x.size(3);
  dispatch_int<3, 5, 7>(ks, "kernel size", [&](auto ks_const) {
    constexpr int KSV = decltype(ks_const)::value;
    dispatch_int<64, 112>(plan.ch, "patch chunk length", [&](auto ch_const) {
      constexpr int CHV = decltype(ch_const)::value;
      if (plan.cls == 16)
        dispatch_int<32, 64>(plan.BK, "patch16 k tile", [&](auto bk_const) {
          constexpr int BKV = decltype(bk_const)::value;
          launch_wgrad_patch_t<Patch16Geo<KSV, BKV, CHV>>(
              k_conv_wgrad_patch16<KSV, BKV, CHV>, plan, dy, x, dw, zero16,
              stream);
        });
      else if (plan.cls == 32)
        launch_wgrad_patch_t<PatchGeo<KSV, 32, 32, 64>>(
            k_conv_wgrad_patch<KSV, 32, 32, 64>, plan, dy, x, dw, zero16,
            stream, Cp);
      else
        launch_wgrad_patch_t<PatchGeo<KSV, 64, 64, CHV>>(
            k_conv_wgrad_patch<KSV, 64, 64, CHV>, plan, dy, x, dw, zero16,
            stream, Cp);
    });
  });
}

}  // namespace

// The launch decision conv2d_wgrad would take for an (N,H,W,Cp) input, a
// (N,H,W,Kp) output gradient and K logical output channels: (kernel, BK, gx,
// gy, gz). Host only: launches nothing and touches no device memory. Reads
// the same environment variables as conv2d_wgrad, at the same times.
std::tuple<std::string, int64_t, int64_t, int64_t, int64_t> conv2d_wgrad_plan(
    int64_t N, int64_t H, int64_t W, int64_t Cp, int64_t Kp, int64_t K,
    int64_t ks) {
  TORCH_CHECK(ks == 1 || ks == 3 || ks == 5 || ks == 7,
              "unsupported kernel size ", ks);
  TORCH_CHECK(N >= 1 && H >= 1 && W >= 1 && K >= 1 && Cp >= 16 && Kp >= 16 &&
                  (Cp & (Cp - 1)) == 0 && (Kp & (Kp - 1)) == 0 && K <= Kp,
              "conv2d_wgrad_plan: Cp and Kp powers of two >= 16, K <= Kp");
  const WgradPlan p = wgrad_plan((int)N, (int)H, (int)W, (int)Cp, (int)Kp,
                                 (int)K, (int)ks);
  const char* name = p.kernel == WG_SMALLK      ? "smallk"
                     : p.kernel == WG_PATCH     ? "patch"
                     : p.kernel == WG_PATCH16   ? "patch16"
                     : p.kernel == WG_GENERIC   ? "generic"
                                                : "generic16";
  return {name, p.BK, p.gx, p.gy, p.gz};
}

void conv2d_wgrad(const at::Tensor& dy, const at::Tensor& x, at::Tensor& dw,
                  int64_t ks) {
  TORCH_CHECK(dy.is_cuda() && dy.dtype() == at::kBFloat16);
  TORCH_CHECK(x.is_cuda() && x.dtype() == at::kBFloat16);
  TORCH_CHECK(dw.is_cuda() && dw.dtype() == at::kFloat && dw.dim() == 4);
  TORCH_CHECK(dy.is_contiguous() && x.is_contiguous() && dw.is_contiguous());
  const int N = x.size(0), H = x.size(1), W = x.size(2), Cp = x.size(3);
  const int Kp = dy.size(3);
  const int K = dw.size(0), C = dw.size(1);
  TORCH_CHECK(dw.size(2) == ks && dw.size(3) == ks);
  hipStream_t stream = at::cuda::getCurrentHIPStream();
  const WgradPlan plan = wgrad_plan(N, H, W, Cp, Kp, K, (int)ks);
  if (plan.kernel == WG_SMALLK) {
    dispatch_int<1, 2, 4, 6>(plan.unroll, "WN_WGRAD_SMALLK_U",
                             [&](auto u_const) {
      constexpr int UV = decltype(u_const)::value;
      hipLaunchKernelGGL((k_wgrad_smallk<4, UV>), dim3(plan.gx, plan.gy),
                         dim3(256), (size_t)SmallKGeo<4>::LDS_BYTES, stream,
                         (const bf16_t*)dy.data_ptr(),
                         (const bf16_t*)x.data_ptr(), dw.data_ptr<float>(),
                         N, H, W, Cp, log2i(Cp), Kp, K, C, (int)ks, plan.gy,
                         MagicDiv::make((unsigned)(H * W)).mul,
                         MagicDiv::make((unsigned)W).mul);
    });
    HIP_CHECK_LAST();
    return;
  }
  if (plan.kernel == WG_PATCH || plan.kernel == WG_PATCH16) {
    launch_wgrad_patch(dy, x, dw, (int)ks, plan, zero16_for(x), stream);
    HIP_CHECK_LAST();
    return;
  }
  const bf16_t* zptr = zero16_for(x);
  dispatch_int<1, 3, 5, 7>((int)ks, "kernel size", [&](auto ks_const) {
    // BK = min(Kp, 128) with Kp a power of two >= 16
    dispatch_int_or<16, 128, 64, 32, 16>(plan.BK, [&](auto bk_const) {
      constexpr int KSV = decltype(ks_const)::value;
      constexpr int BKV = decltype(bk_const)::value;
      dispatch_int<0, 1>(plan.kernel == WG_GENERIC, "M32",
                         [&](auto m32_const) {
        constexpr bool M32V = BKV >= 32 && decltype(m32_const)::value != 0;
        using G = WgradGeo<BKV, WG_CH>;
        hipLaunchKernelGGL((k_conv_wgrad<KSV, BKV, WG_CH, M32V>),
                           dim3(plan.gx, plan.gy, plan.gz), dim3(256),
                           (size_t)G::LDS_BYTES, stream,
                           (const bf16_t*)dy.data_ptr(),
                           (const bf16_t*)x.data_ptr(), dw.data_ptr<float>(),
                           N, H, W, Cp, log2i(Cp), Kp, K, C, plan.gz,
                           MagicDiv::make((unsigned)(H * W)).mul,
                           MagicDiv::make((unsigned)W).mul, zptr);
      });
    });
  });
  HIP_CHECK_LAST();
}

void bias_grad(const at::Tensor& dy, at::Tensor& db) {
  TORCH_CHECK(dy.is_cuda() && dy.dtype() == at::kBFloat16 && dy.dim() == 4 &&
                  dy.is_contiguous(),
              "bias_grad: dy must be contiguous (N,H,W,Kp) bf16 on the GPU");
  TORCH_CHECK(db.is_cuda() && db.dtype() == at::kFloat && db.dim() == 1 &&
                  db.is_contiguous() && db.device() == dy.device(),
              "bias_grad: db must be a contiguous 1-D fp32 tensor on dy's "
              "device");
  const int Kp = dy.size(3);
  TORCH_CHECK(Kp >= 8 && Kp % 8 == 0, "bias_grad: Kp must be a multiple of 8");
  const long M = dy.numel() / Kp;
  const int K = db.size(0);
  TORCH_CHECK(K <= Kp, "bias_grad: db longer than Kp");
  if (M == 0 || K == 0) return;
  const int ngrp = Kp / 8;
  const int KGR = std::min(ngrp, 32);
  const int gx = (ngrp + KGR - 1) / KGR;
  int msplit = std::max(1, 448 / gx);  // fill the chip; partial slabs
  const int MR = 256 / KGR;
  msplit = (int)std::min<long>(msplit, (M + MR - 1) / MR);
  hipStream_t stream = at::cuda::getCurrentHIPStream();
  auto part = at::empty({msplit, (long)Kp},
                        dy.options().dtype(at::kFloat));
  hipLaunchKernelGGL(k_bias_grad, dim3(gx, msplit), dim3(256),
                     (size_t)BiasGradGeo::LDS_BYTES, stream,
                     (const bf16_t*)dy.data_ptr(), part.data_ptr<float>(),
                     M, Kp, msplit);
  HIP_CHECK_LAST();
  hipLaunchKernelGGL(k_bias_grad_reduce, dim3(K), dim3(256), 0, stream,
                     part.data_ptr<float>(), db.data_ptr<float>(), Kp, K,
                     msplit);
  HIP_CHECK_LAST();
}
