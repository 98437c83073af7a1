// Fused elementwise / layout / reduction kernels for the WaterNet engine
// (gfx950). Covers SURVEY §2.2 K1/K10/K11 (cat/split folding via the input
// builders), K15 (gated fusion fwd/bwd), K16 (ImageNet normalize), K18/K19
// (fused squared-diff reductions), K23/K25 (fused flat Adam), K27 (uint8
// postprocess), plus the NCHW fp32 <-> NHWC bf16 bridges and activation
// backward.

#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>

#include "common.h"
#include "gather_augment.h"
#include "host_check.h"

// ---------------------------------------------------------------------------
// RGB pixel family. A pixel p of N*H*W holds three logical values in one of
// three layouts; an accessor loads or stores them as fp32:
//   U8     (N,H,W,3) uint8
//   Planar (N,3,H,W) fp32
//   Nhwc   (N,H,W,Cp) bf16, Cp >= 3; a store zero-fills channels 3..Cp-1
// A per-channel op sits between load and store. pixel_map_body serves the
// seven layout / normalize / postprocess kernels, build_inputs_body the two
// input builders; the __global__s below only name an instantiation.
// ---------------------------------------------------------------------------

struct SrcU8 {
  const uint8_t* __restrict__ x;
  WN_DEVFN void load(long p, float v[3]) const {
    const uint8_t* s = x + p * 3;
    v[0] = s[0]; v[1] = s[1]; v[2] = s[2];
  }
};
struct SrcPlanar {
  const float* __restrict__ x;
  long HW;
  WN_DEVFN void load(long p, float v[3]) const {
    const long n = p / HW, rem = p - n * HW;
    const float* s = x + (n * 3) * HW + rem;
    v[0] = s[0]; v[1] = s[HW]; v[2] = s[2 * HW];
  }
};
struct SrcNhwc {
  const bf16_t* __restrict__ x;
  int Cp;
  WN_DEVFN void load(long p, float v[3]) const {
    const bf16_t* s = x + p * Cp;
    v[0] = bf2f(s[0]); v[1] = bf2f(s[1]); v[2] = bf2f(s[2]);
  }
};

struct DstU8 {  // truncating cast: ten2arr semantics
  uint8_t* __restrict__ y;
  WN_DEVFN void store(long p, const float v[3]) const {
    uint8_t* d = y + p * 3;
    d[0] = (uint8_t)v[0]; d[1] = (uint8_t)v[1]; d[2] = (uint8_t)v[2];
  }
};
struct DstPlanar {
  float* __restrict__ y;
  long HW;
  WN_DEVFN void store(long p, const float v[3]) const {
    const long n = p / HW, rem = p - n * HW;
    float* d = y + (n * 3) * HW + rem;
    d[0] = v[0]; d[HW] = v[1]; d[2 * HW] = v[2];
  }
};
struct DstNhwc {
  bf16_t* __restrict__ y;
  int Cp;
  WN_DEVFN void store(long p, const float v[3]) const {
    bf16_t* d = y + p * Cp;
    d[0] = f2bf(v[0]); d[1] = f2bf(v[1]); d[2] = f2bf(v[2]);
    for (int c = 3; c < Cp; ++c) d[c] = f2bf(0.f);
  }
};

__constant__ float IMNET_MEAN[3] = {0.485f, 0.456f, 0.406f};
__constant__ float IMNET_STD[3] = {0.229f, 0.224f, 0.225f};

struct OpIdentity {
  WN_DEVFN float operator()(float v, int) const { return v; }
};
struct OpScale255 {  // uint8 -> [0,1]: a multiply by the fp32 constant
  WN_DEVFN float operator()(float v, int) const { return v * (1.f / 255.f); }
};
struct OpNormFwd {  // ImageNet normalize (train.py:111-116)
  WN_DEVFN float operator()(float v, int c) const {
    return (v - IMNET_MEAN[c]) / IMNET_STD[c];
  }
};
struct OpNormBwd {
  WN_DEVFN float operator()(float g, int c) const { return g / IMNET_STD[c]; }
};
struct OpClip255 {  // clip to [0,1], *255 (training_utils.py:27-43)
  WN_DEVFN float operator()(float v, int) const {
    return fminf(fmaxf(v, 0.f), 1.f) * 255.f;
  }
};

template <class Src, class Op>
WN_DEVFN void load_rgb(const Src& src, Op op, long p, float v[3]) {
  src.load(p, v);
#pragma unroll
  for (int c = 0; c < 3; ++c) v[c] = op(v[c], c);
}

// A thread's walk of a grid-stride loop. The __global__ passes its own
// blockDim.x: the compiler folds that read to the launch's uniform block
// size only in the kernel function itself; inside a device function, even a
// forceinline one, it becomes a dependent global load in the prologue.
struct GridStride {
  long first, step;
};
WN_DEVFN GridStride grid_stride(unsigned block_dim) {
  return {(long)blockIdx.x * block_dim + threadIdx.x,
          (long)gridDim.x * block_dim};
}

template <class Src, class Dst, class Op>
WN_DEVFN void pixel_map_body(GridStride t, Src src, Dst dst, Op op,
                             long NHW) {
  for (long p = t.first; p < NHW; p += t.step) {
    float v[3];
    load_rgb(src, op, p, v);
    dst.store(p, v);
  }
}

// Input builders: four RGB sources -> cmg input [raw wb ce gc 0000] and the
// three refiner inputs [raw src 0...], all (N,H,W,16) bf16. Folds the
// reference's torch.cat calls (net.py:46, net.py:76) into one pass.
template <class Src, class Op>
WN_DEVFN void build_inputs_body(GridStride t, Src raw, Src wb, Src ce,
                                Src gc, Op op, bf16_t* __restrict__ cmg_in,
                                bf16_t* __restrict__ rwb_in,
                                bf16_t* __restrict__ rce_in,
                                bf16_t* __restrict__ rgc_in, long NHW) {
  for (long p = t.first; p < NHW; p += t.step) {
    float r[3], w[3], c[3], g[3];
    load_rgb(raw, op, p, r);
    load_rgb(wb, op, p, w);
    load_rgb(ce, op, p, c);
    load_rgb(gc, op, p, g);
    auto put3 = [](bf16_t* q, const float a[3]) {
      q[0] = f2bf(a[0]); q[1] = f2bf(a[1]); q[2] = f2bf(a[2]);
    };
    bf16_t* o = cmg_in + p * 16;
    put3(o, r); put3(o + 3, w); put3(o + 6, c); put3(o + 9, g);
    o[12] = o[13] = o[14] = o[15] = f2bf(0.f);
    auto emit = [&](bf16_t* dst, const float a[3]) {
      bf16_t* q = dst + p * 16;
      put3(q, r); put3(q + 3, a);
#pragma unroll
      for (int i = 6; i < 16; ++i) q[i] = f2bf(0.f);
    };
    emit(rwb_in, w);
    emit(rce_in, c);
    emit(rgc_in, g);
  }
}

// 4x NCHW fp32 (3ch, already in [0,1])
__global__ void k_build_inputs(const float* __restrict__ raw,
                               const float* __restrict__ wb,
                               const float* __restrict__ ce,
                               const float* __restrict__ gc,
                               bf16_t* __restrict__ cmg_in,
                               bf16_t* __restrict__ rwb_in,
                               bf16_t* __restrict__ rce_in,
                               bf16_t* __restrict__ rgc_in, long NHW,
                               long HW) {
  build_inputs_body(grid_stride(blockDim.x), SrcPlanar{raw, HW},
                    SrcPlanar{wb, HW}, SrcPlanar{ce, HW}, SrcPlanar{gc, HW},
                    OpIdentity{}, cmg_in, rwb_in, rce_in, rgc_in, NHW);
}

// straight from the uint8 HWC batch tensors (raw + the GPU-preprocess
// outputs), /255: no u8->NCHW-fp32 bridges and no NCHW intermediates on the
// full-NHWC training path (reference arr2ten training_utils.py:11-27)
__global__ void k_build_inputs_u8(const uint8_t* __restrict__ raw,
                                  const uint8_t* __restrict__ wb,
                                  const uint8_t* __restrict__ ce,
                                  const uint8_t* __restrict__ gc,
                                  bf16_t* __restrict__ cmg_in,
                                  bf16_t* __restrict__ rwb_in,
                                  bf16_t* __restrict__ rce_in,
                                  bf16_t* __restrict__ rgc_in, long NHW) {
  build_inputs_body(grid_stride(blockDim.x), SrcU8{raw}, SrcU8{wb},
                    SrcU8{ce}, SrcU8{gc}, OpScale255{}, cmg_in, rwb_in, rce_in,
                    rgc_in, NHW);
}

// uint8 HWC -> (N,H,W,Cp) bf16 [0,1] (the ref tensor of the NHWC loss path)
__global__ void k_u8_to_nhwc(const uint8_t* __restrict__ x,
                             bf16_t* __restrict__ y, long NHW, int Cp) {
  pixel_map_body(grid_stride(blockDim.x), SrcU8{x}, DstNhwc{y, Cp},
                 OpScale255{}, NHW);
}

// uint8 HWC -> NCHW fp32 [0,1] input bridge
__global__ void k_u8_to_nchw(const uint8_t* __restrict__ x,
                             float* __restrict__ y, long NHW, long HW) {
  pixel_map_body(grid_stride(blockDim.x), SrcU8{x}, DstPlanar{y, HW},
                 OpScale255{}, NHW);
}

// Fused postprocess (K27): NHWC bf16 model output -> uint8 RGB
__global__ void k_out_to_u8(const bf16_t* __restrict__ x,
                            uint8_t* __restrict__ y, long NHW, int Cp) {
  pixel_map_body(grid_stride(blockDim.x), SrcNhwc{x, Cp}, DstU8{y},
                 OpClip255{}, NHW);
}

// ImageNet normalize fused with NCHW fp32 -> NHWC bf16, and its backward
__global__ void k_normalize_vgg_fwd(const float* __restrict__ x,
                                    bf16_t* __restrict__ y, long NHW,
                                    long HW, int Cp) {
  pixel_map_body(grid_stride(blockDim.x), SrcPlanar{x, HW}, DstNhwc{y, Cp},
                 OpNormFwd{}, NHW);
}

__global__ void k_normalize_vgg_bwd(const bf16_t* __restrict__ dy,
                                    float* __restrict__ dx, long NHW,
                                    long HW, int Cp) {
  pixel_map_body(grid_stride(blockDim.x), SrcNhwc{dy, Cp}, DstPlanar{dx, HW},
                 OpNormBwd{}, NHW);
}

// In-layout normalize (full-NHWC loss path: the WaterNet output and ref stay
// NHWC from the fusion kernel through the VGG towers, no NCHW round trip)
__global__ void k_normalize_nhwc_fwd(const bf16_t* __restrict__ x,
                                     bf16_t* __restrict__ y, long NHW,
                                     int Cp) {
  pixel_map_body(grid_stride(blockDim.x), SrcNhwc{x, Cp}, DstNhwc{y, Cp},
                 OpNormFwd{}, NHW);
}

__global__ void k_normalize_nhwc_bwd(const bf16_t* __restrict__ dy,
                                     bf16_t* __restrict__ dx, long NHW,
                                     int Cp) {
  pixel_map_body(grid_stride(blockDim.x), SrcNhwc{dy, Cp}, DstNhwc{dx, Cp},
                 OpNormBwd{}, NHW);
}

// ---------------------------------------------------------------------------
// NCHW fp32 <-> NHWC bf16 bridges
// ---------------------------------------------------------------------------

// LDS-tiled layout bridges: 256 pixels x 16 channels per block so BOTH
// sides are coalesced (the naive per-pixel loop read NCHW at stride HW and
// wrote 2 B scattered — measured 125 GB/s; these run at HBM rate).
__global__ void k_nchw2nhwc(const float* __restrict__ x,
                            bf16_t* __restrict__ y, long NHW, long HW, int C,
                            int Cp) {
  __shared__ float tile[16][257];
  const int tid = threadIdx.x;
  const long p = (long)blockIdx.x * 256 + tid;
  const int cc0 = blockIdx.z * 16;
  const bool pv = p < NHW;
  const long n = pv ? p / HW : 0;
  const long rem = p - n * HW;
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const int c = cc0 + i;
    tile[i][tid] =
        (pv && c < C) ? x[(n * C + c) * HW + rem] : 0.f;
  }
  __syncthreads();
  if (pv) {
#pragma unroll
    for (int v8 = 0; v8 < 2; ++v8) {
      bf16x8 v;
#pragma unroll
      for (int e = 0; e < 8; ++e) v[e] = f2bf(tile[v8 * 8 + e][tid]);
      *reinterpret_cast<bf16x8*>(y + p * Cp + cc0 + v8 * 8) = v;
    }
  }
}

__global__ void k_nhwc2nchw(const bf16_t* __restrict__ x,
                            float* __restrict__ y, long NHW, long HW, int C,
                            int Cp) {
  __shared__ float tile[16][257];
  const int tid = threadIdx.x;
  const long p = (long)blockIdx.x * 256 + tid;
  const int cc0 = blockIdx.z * 16;
  const bool pv = p < NHW;
  if (pv) {
#pragma unroll
    for (int v8 = 0; v8 < 2; ++v8) {
      const bf16x8 v =
          *reinterpret_cast<const bf16x8*>(x + p * Cp + cc0 + v8 * 8);
#pragma unroll
      for (int e = 0; e < 8; ++e) tile[v8 * 8 + e][tid] = bf2f(v[e]);
    }
  }
  __syncthreads();
  const long n = pv ? p / HW : 0;
  const long rem = p - n * HW;
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const int c = cc0 + i;
    if (pv && c < C) y[(n * C + c) * HW + rem] = tile[i][tid];
  }
}

// ---------------------------------------------------------------------------
// Gated fusion (net.py:104-108): out_c = sum_i refined_i_c * map_i
// maps = (N,H,W,16) logical 3 (cmg conv8 sigmoid output)
// refined_i = (N,H,W,16) logical 3
// ---------------------------------------------------------------------------

__global__ void k_fusion_fwd(const bf16_t* __restrict__ maps,
                             const bf16_t* __restrict__ rwb,
                             const bf16_t* __restrict__ rce,
                             const bf16_t* __restrict__ rgc,
                             bf16_t* __restrict__ out, long NHW) {
  for (long p = (long)blockIdx.x * blockDim.x + threadIdx.x; p < NHW;
       p += (long)gridDim.x * blockDim.x) {
    const long o = p * 16;
    float m0 = bf2f(maps[o]), m1 = bf2f(maps[o + 1]), m2 = bf2f(maps[o + 2]);
    bf16_t* dst = out + o;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      float v = bf2f(rwb[o + c]) * m0 + bf2f(rce[o + c]) * m1 +
                bf2f(rgc[o + c]) * m2;
      dst[c] = f2bf(v);
    }
#pragma unroll
    for (int c = 3; c < 16; ++c) dst[c] = f2bf(0.f);
  }
}

__global__ void k_fusion_bwd(const bf16_t* __restrict__ dout,
                             const bf16_t* __restrict__ maps,
                             const bf16_t* __restrict__ rwb,
                             const bf16_t* __restrict__ rce,
                             const bf16_t* __restrict__ rgc,
                             bf16_t* __restrict__ dmaps,
                             bf16_t* __restrict__ drwb,
                             bf16_t* __restrict__ drce,
                             bf16_t* __restrict__ drgc, long NHW) {
  for (long p = (long)blockIdx.x * blockDim.x + threadIdx.x; p < NHW;
       p += (long)gridDim.x * blockDim.x) {
    const long o = p * 16;
    float m0 = bf2f(maps[o]), m1 = bf2f(maps[o + 1]), m2 = bf2f(maps[o + 2]);
    float dm0 = 0.f, dm1 = 0.f, dm2 = 0.f;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      float g = bf2f(dout[o + c]);
      dm0 += g * bf2f(rwb[o + c]);
      dm1 += g * bf2f(rce[o + c]);
      dm2 += g * bf2f(rgc[o + c]);
      drwb[o + c] = f2bf(g * m0);
      drce[o + c] = f2bf(g * m1);
      drgc[o + c] = f2bf(g * m2);
    }
    dmaps[o] = f2bf(dm0);
    dmaps[o + 1] = f2bf(dm1);
    dmaps[o + 2] = f2bf(dm2);
#pragma unroll
    for (int c = 3; c < 16; ++c) {
      dmaps[o + c] = f2bf(0.f);
      drwb[o + c] = f2bf(0.f);
      drce[o + c] = f2bf(0.f);
      drgc[o + c] = f2bf(0.f);
    }
  }
}

// ---------------------------------------------------------------------------
// Activation backward: dpre = dY * act'(Y)  (Y = post-activation output)
// ---------------------------------------------------------------------------

WN_DEVFN float act_grad(float g, float v, int act) {
  return (act == ACT_RELU) ? (v > 0.f ? g : 0.f) : g * v * (1.f - v);
}

__global__ void k_act_bwd(const bf16_t* __restrict__ dy,
                          const bf16_t* __restrict__ y,
                          bf16_t* __restrict__ dpre, long n, int act) {
  // bf16x8 vector path (n is always a multiple of 8 here: NHWC with Cp a
  // multiple of 16); scalar tail kept for generality
  const long n8 = n / 8;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n8;
       i += (long)gridDim.x * blockDim.x) {
    const bf16x8 gv = *reinterpret_cast<const bf16x8*>(dy + i * 8);
    const bf16x8 vv = *reinterpret_cast<const bf16x8*>(y + i * 8);
    bf16x8 r;
#pragma unroll
    for (int e = 0; e < 8; ++e)
      r[e] = f2bf(act_grad(bf2f(gv[e]), bf2f(vv[e]), act));
    *reinterpret_cast<bf16x8*>(dpre + i * 8) = r;
  }
  for (long i = n8 * 8 + (long)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (long)gridDim.x * blockDim.x)
    dpre[i] = f2bf(act_grad(bf2f(dy[i]), bf2f(y[i]), act));
}

// act_bwd fused with the bias-gradient column sums (K25 epilogue fusion):
// dpre = dY * act'(Y) while accumulating sum_m dpre[m][k] per block into a
// partial slab — saves the separate bias_grad kernel's full re-read of
// dpre (the WaterNet layers' bias grads; the frozen VGG keeps plain
// act_bwd). Thread->channel-octet mapping is STABLE across grid-stride
// iterations because (gridDim*blockDim*8) % Kp == 0 (host guarantees
// blocks*2048 divisible by Kp; Kp is a power of two <= 128).
__global__ void k_act_bwd_bias(const bf16_t* __restrict__ dy,
                               const bf16_t* __restrict__ y,
                               bf16_t* __restrict__ dpre,
                               float* __restrict__ part,  // [grid][Kp]
                               long n8, int Kp, int act) {
  __shared__ float red[128];  // Kp <= 128
  if (threadIdx.x < Kp) red[threadIdx.x] = 0.f;
  __syncthreads();
  float s[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) s[e] = 0.f;
  const long i0 = (long)blockIdx.x * blockDim.x + threadIdx.x;
  for (long i = i0; i < n8; i += (long)gridDim.x * blockDim.x) {
    const bf16x8 gv = *reinterpret_cast<const bf16x8*>(dy + i * 8);
    const bf16x8 vv = *reinterpret_cast<const bf16x8*>(y + i * 8);
    bf16x8 r;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const float d = act_grad(bf2f(gv[e]), bf2f(vv[e]), act);
      r[e] = f2bf(d);
      s[e] += d;
    }
    *reinterpret_cast<bf16x8*>(dpre + i * 8) = r;
  }
  const int c0 = (int)((i0 * 8) % Kp);
#pragma unroll
  for (int e = 0; e < 8; ++e) atomicAdd(&red[c0 + e], s[e]);
  __syncthreads();
  if (threadIdx.x < Kp) part[(long)blockIdx.x * Kp + threadIdx.x] =
      red[threadIdx.x];
}

// slab reduce into db (ACCUMULATES — the arena view may already hold
// autograd-accumulated values)
__global__ void k_abb_reduce(const float* __restrict__ part,
                             float* __restrict__ db, int Kp, int K,
                             int nblk) {
  const int k = blockIdx.x;
  if (k >= K) return;
  __shared__ float red[256];
  float s = 0.f;
  for (int r = threadIdx.x; r < nblk; r += 256)
    s += part[(long)r * Kp + k];
  red[threadIdx.x] = s;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if (threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x == 0) db[k] += red[0];
}

// ---------------------------------------------------------------------------
// Scaled squared-difference reduction (K18/K19):
//   sum over logical elements of (255*(a-b))^2, fp64 accumulator.
// flat variant (Clog == Cp) and channel-masked variant.
// ---------------------------------------------------------------------------

// Every atomic of a launch lands on the one output address and they
// serialise, so the grid is capped (grid-stride loop) and a block issues
// exactly one: fp32 per thread, f64 across the wave and, through LDS, across
// the block.
constexpr int SQD_MAX_BLOCKS = 512;

__device__ __forceinline__ void sqdiff_block_atomic(float s,
                                                    double* __restrict__ out) {
  __shared__ double wsum[TPB / 64];
  double d = (double)s;
  for (int off = 32; off > 0; off >>= 1) d += __shfl_down(d, off, 64);
  if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = d;
  __syncthreads();
  if (threadIdx.x == 0) {
    double t = 0.0;
    for (int w = 0; w < (int)(blockDim.x >> 6); ++w) t += wsum[w];
    atomicAdd(out, t);
  }
}

__global__ void k_sqdiff255_flat(const bf16_t* __restrict__ a,
                                 const bf16_t* __restrict__ b,
                                 double* __restrict__ out, long n) {
  float s = 0.f;
  const long t0 = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long nt = (long)gridDim.x * blockDim.x;
  // 16 B body where both pointers allow it, scalar tail (or everything)
  const bool vec =
      (((unsigned long long)a | (unsigned long long)b) & 15ull) == 0;
  const long nv = vec ? n / 8 : 0;
  for (long i = t0; i < nv; i += nt) {
    const bf16x8 av = *reinterpret_cast<const bf16x8*>(a + i * 8);
    const bf16x8 bv = *reinterpret_cast<const bf16x8*>(b + i * 8);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      float d = 255.f * (bf2f(av[e]) - bf2f(bv[e]));
      s += d * d;
    }
  }
  for (long i = nv * 8 + t0; i < n; i += nt) {
    float d = 255.f * (bf2f(a[i]) - bf2f(b[i]));
    s += d * d;
  }
  sqdiff_block_atomic(s, out);
}

__global__ void k_sqdiff255_pix(const bf16_t* __restrict__ a,
                                const bf16_t* __restrict__ b,
                                double* __restrict__ out, long NHW, int Clog,
                                int Cp) {
  float s = 0.f;
  for (long p = (long)blockIdx.x * blockDim.x + threadIdx.x; p < NHW;
       p += (long)gridDim.x * blockDim.x) {
    const long o = p * Cp;
    for (int c = 0; c < Clog; ++c) {
      float d = 255.f * (bf2f(a[o + c]) - bf2f(b[o + c]));
      s += d * d;
    }
  }
  sqdiff_block_atomic(s, out);
}

// backward: da = gscale * (a - b), with gscale = grad * 2*255^2/numel
__global__ void k_sqdiff255_bwd(const bf16_t* __restrict__ a,
                                const bf16_t* __restrict__ b,
                                const float* __restrict__ gscale,
                                bf16_t* __restrict__ da, long n, float sign) {
  const float gs = gscale[0] * sign;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (long)gridDim.x * blockDim.x) {
    da[i] = f2bf(gs * (bf2f(a[i]) - bf2f(b[i])));
  }
}

// ---------------------------------------------------------------------------
// Fused flat Adam (K23): torch.optim.Adam semantics, fp32 master params.
// ---------------------------------------------------------------------------

// Graph-safe: the step counter and lr live in DEVICE buffers so a
// hipGraph-captured step keeps correct bias correction and per-minibatch
// StepLR semantics under replay (k_adam_tick runs first on the stream).
__global__ void k_adam_tick(int* __restrict__ step) {
  if (threadIdx.x == 0 && blockIdx.x == 0) step[0] += 1;
}

__global__ void k_adam(float* __restrict__ p, const float* __restrict__ g,
                       float* __restrict__ m, float* __restrict__ v, long n,
                       const float* __restrict__ lr_buf, float b1, float b2,
                       float eps, const int* __restrict__ step) {
  const float lr = lr_buf[0];
  const float t = (float)step[0];
  const float bc1 = 1.f - powf(b1, t);
  const float bc2 = 1.f - powf(b2, t);
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (long)gridDim.x * blockDim.x) {
    float gi = g[i];
    float mi = b1 * m[i] + (1.f - b1) * gi;
    float vi = b2 * v[i] + (1.f - b2) * gi * gi;
    m[i] = mi;
    v[i] = vi;
    float mhat = mi / bc1;
    float vhat = vi / bc2;
    p[i] -= lr * mhat / (sqrtf(vhat) + eps);
  }
}

// ===========================================================================
// Host wrappers. Every argument a kernel indexes is checked first (the
// vocabulary is host_check.h); an empty input returns its empty result
// without a launch; a contiguous copy lives in a named local.
// ===========================================================================

namespace {
inline const bf16_t* cbf(const at::Tensor& t) {
  return (const bf16_t*)t.data_ptr();
}
inline bf16_t* bf(at::Tensor& t) { return (bf16_t*)t.data_ptr(); }
}  // namespace

// the builders' four (N,H,W,16) bf16 outputs
static std::vector<at::Tensor> empty_inputs(const at::Tensor& raw, long N,
                                            long H, long W) {
  const auto opts = raw.options().dtype(at::kBFloat16);
  return {at::empty({N, H, W, 16}, opts), at::empty({N, H, W, 16}, opts),
          at::empty({N, H, W, 16}, opts), at::empty({N, H, W, 16}, opts)};
}

std::vector<at::Tensor> build_inputs(const at::Tensor& raw,
                                     const at::Tensor& wb,
                                     const at::Tensor& ce,
                                     const at::Tensor& gc) {
  TORCH_CHECK(on_gpu(raw, at::kFloat, 4) && raw.size(1) == 3,
              "build_inputs: raw must be (N,3,H,W) fp32 on the GPU");
  TORCH_CHECK(like(wb, raw) && like(ce, raw) && like(gc, raw),
              "build_inputs: wb, ce and gc must have raw's dtype, shape and "
              "device");
  const auto r = raw.contiguous(), w = wb.contiguous(), c = ce.contiguous(),
             g = gc.contiguous();
  const long N = raw.size(0), H = raw.size(2), W = raw.size(3);
  auto out = empty_inputs(raw, N, H, W);
  launch1d(k_build_inputs, N * H * W, r.data_ptr<float>(),
           w.data_ptr<float>(), c.data_ptr<float>(), g.data_ptr<float>(),
           bf(out[0]), bf(out[1]), bf(out[2]), bf(out[3]), N * H * W, H * W);
  return out;
}

std::vector<at::Tensor> build_inputs_u8(const at::Tensor& raw,
                                        const at::Tensor& wb,
                                        const at::Tensor& ce,
                                        const at::Tensor& gc) {
  TORCH_CHECK(on_gpu(raw, at::kByte, 4) && raw.size(3) == 3,
              "build_inputs_u8: raw must be (N,H,W,3) uint8 on the GPU");
  TORCH_CHECK(like(wb, raw) && like(ce, raw) && like(gc, raw),
              "build_inputs_u8: wb, ce and gc must have raw's dtype, shape "
              "and device");
  const auto r = raw.contiguous(), w = wb.contiguous(), c = ce.contiguous(),
             g = gc.contiguous();
  const long N = raw.size(0), H = raw.size(1), W = raw.size(2);
  auto out = empty_inputs(raw, N, H, W);
  launch1d(k_build_inputs_u8, N * H * W, r.data_ptr<uint8_t>(),
           w.data_ptr<uint8_t>(), c.data_ptr<uint8_t>(),
           g.data_ptr<uint8_t>(), bf(out[0]), bf(out[1]), bf(out[2]),
           bf(out[3]), N * H * W);
  return out;
}

at::Tensor u8_to_nhwc(const at::Tensor& x, int64_t Cp) {
  TORCH_CHECK(on_gpu(x, at::kByte, 4) && x.size(3) == 3,
              "u8_to_nhwc: x must be (N,H,W,3) uint8 on the GPU");
  TORCH_CHECK(has_rgb(Cp), "u8_to_nhwc: Cp must be at least 3");
  const auto xc = x.contiguous();
  const long N = x.size(0), H = x.size(1), W = x.size(2);
  auto y = at::empty({N, H, W, Cp}, x.options().dtype(at::kBFloat16));
  launch1d(k_u8_to_nhwc, N * H * W, xc.data_ptr<uint8_t>(), bf(y), N * H * W,
           (int)Cp);
  return y;
}

at::Tensor u8_to_nchw(const at::Tensor& x) {
  TORCH_CHECK(on_gpu(x, at::kByte, 4) && x.size(3) == 3,
              "u8_to_nchw: x must be (N,H,W,3) uint8 on the GPU");
  const auto xc = x.contiguous();
  const long N = x.size(0), H = x.size(1), W = x.size(2);
  auto y = at::empty({N, 3, H, W}, x.options().dtype(at::kFloat));
  launch1d(k_u8_to_nchw, N * H * W, xc.data_ptr<uint8_t>(),
           y.data_ptr<float>(), N * H * W, H * W);
  return y;
}

// checks x: (N,H,W,Cp >= 3) bf16 on the GPU, any strides (the caller takes
// the contiguous copy); returns its pixel count
static long rgb_nhwc_pixels(const char* name, const at::Tensor& x) {
  TORCH_CHECK(on_gpu(x, at::kBFloat16, 4) && has_rgb(x.size(3)), name,
              ": the tensor must be (N,H,W,Cp >= 3) bf16 on the GPU");
  return x.size(0) * x.size(1) * x.size(2);
}

at::Tensor out_to_u8(const at::Tensor& x) {
  const long NHW = rgb_nhwc_pixels("out_to_u8", x);
  const auto xc = x.contiguous();
  auto y = at::empty({x.size(0), x.size(1), x.size(2), 3},
                     x.options().dtype(at::kByte));
  launch1d(k_out_to_u8, NHW, cbf(xc), y.data_ptr<uint8_t>(), NHW,
           (int)x.size(3));
  return y;
}

at::Tensor normalize_nhwc_fwd(const at::Tensor& x) {
  const long NHW = rgb_nhwc_pixels("normalize_nhwc_fwd", x);
  const auto xc = x.contiguous();
  auto y = at::empty_like(xc);
  launch1d(k_normalize_nhwc_fwd, NHW, cbf(xc), bf(y), NHW, (int)x.size(3));
  return y;
}

at::Tensor normalize_nhwc_bwd(const at::Tensor& dy) {
  const long NHW = rgb_nhwc_pixels("normalize_nhwc_bwd", dy);
  const auto dyc = dy.contiguous();
  auto dx = at::empty_like(dyc);
  launch1d(k_normalize_nhwc_bwd, NHW, cbf(dyc), bf(dx), NHW,
           (int)dy.size(3));
  return dx;
}

at::Tensor normalize_vgg_fwd(const at::Tensor& x, int64_t Cp) {
  TORCH_CHECK(on_gpu(x, at::kFloat, 4) && x.size(1) == 3,
              "normalize_vgg_fwd: x must be (N,3,H,W) fp32 on the GPU");
  TORCH_CHECK(has_rgb(Cp), "normalize_vgg_fwd: Cp must be at least 3");
  const auto xc = x.contiguous();
  const long N = x.size(0), H = x.size(2), W = x.size(3);
  auto y = at::empty({N, H, W, Cp}, x.options().dtype(at::kBFloat16));
  launch1d(k_normalize_vgg_fwd, N * H * W, xc.data_ptr<float>(), bf(y),
           N * H * W, H * W, (int)Cp);
  return y;
}

at::Tensor normalize_vgg_bwd(const at::Tensor& dy, int64_t C) {
  TORCH_CHECK(C == 3, "normalize_vgg_bwd: C must be 3");
  const long NHW = rgb_nhwc_pixels("normalize_vgg_bwd", dy);
  const auto dyc = dy.contiguous();
  const long H = dy.size(1), W = dy.size(2);
  auto dx = at::empty({dy.size(0), C, H, W}, dy.options().dtype(at::kFloat));
  launch1d(k_normalize_vgg_bwd, NHW, cbf(dyc), dx.data_ptr<float>(), NHW,
           H * W, (int)dy.size(3));
  return dx;
}

// grid of the LDS-tiled bridges: 256 pixels x 16 channels per block
static dim3 bridge_grid(long NHW, long Cp) {
  return dim3((unsigned)((NHW + 255) / 256), 1, (unsigned)(Cp / 16));
}

at::Tensor nchw_to_nhwc(const at::Tensor& x, int64_t Cp) {
  TORCH_CHECK(on_gpu(x, at::kFloat, 4),
              "nchw_to_nhwc: x must be (N,C,H,W) fp32 on the GPU");
  const long N = x.size(0), C = x.size(1), H = x.size(2), W = x.size(3);
  TORCH_CHECK(bridge_channels(C, Cp),
              "nchw_to_nhwc: Cp must be a positive multiple of 16 and at "
              "least C");
  const auto xc = x.contiguous();
  auto y = at::empty({N, H, W, Cp}, x.options().dtype(at::kBFloat16));
  const long NHW = N * H * W;
  if (NHW == 0) return y;
  hipLaunchKernelGGL(k_nchw2nhwc, bridge_grid(NHW, Cp), dim3(256), 0,
                     cur_stream(), xc.data_ptr<float>(), bf(y), NHW, H * W,
                     (int)C, (int)Cp);
  HIP_CHECK_LAST();
  return y;
}

at::Tensor nhwc_to_nchw(const at::Tensor& x, int64_t C) {
  TORCH_CHECK(on_gpu(x, at::kBFloat16, 4),
              "nhwc_to_nchw: x must be (N,H,W,Cp) bf16 on the GPU");
  const long N = x.size(0), H = x.size(1), W = x.size(2), Cp = x.size(3);
  TORCH_CHECK(bridge_channels(C, Cp),
              "nhwc_to_nchw: Cp must be a positive multiple of 16 and at "
              "least C >= 0");
  const auto xc = x.contiguous();
  auto y = at::empty({N, C, H, W}, x.options().dtype(at::kFloat));
  const long NHW = N * H * W;
  if (y.numel() == 0) return y;
  hipLaunchKernelGGL(k_nhwc2nchw, bridge_grid(NHW, Cp), dim3(256), 0,
                     cur_stream(), cbf(xc), y.data_ptr<float>(), NHW, H * W,
                     (int)C, (int)Cp);
  HIP_CHECK_LAST();
  return y;
}

at::Tensor fusion_fwd(const at::Tensor& maps, const at::Tensor& rwb,
                      const at::Tensor& rce, const at::Tensor& rgc) {
  TORCH_CHECK(dense(maps, at::kBFloat16, 4) && maps.size(3) == 16,
              "fusion_fwd: maps must be contiguous (N,H,W,16) bf16 on the "
              "GPU");
  TORCH_CHECK(dense_like(rwb, maps) && dense_like(rce, maps) &&
                  dense_like(rgc, maps),
              "fusion_fwd: rwb, rce and rgc must be contiguous, of maps' "
              "dtype, shape and device");
  const long NHW = maps.size(0) * maps.size(1) * maps.size(2);
  auto out = at::empty_like(maps);
  launch1d(k_fusion_fwd, NHW, cbf(maps), cbf(rwb), cbf(rce), cbf(rgc),
           bf(out), NHW);
  return out;
}

std::vector<at::Tensor> fusion_bwd(const at::Tensor& dout,
                                   const at::Tensor& maps,
                                   const at::Tensor& rwb,
                                   const at::Tensor& rce,
                                   const at::Tensor& rgc) {
  TORCH_CHECK(dense(maps, at::kBFloat16, 4) && maps.size(3) == 16,
              "fusion_bwd: maps must be contiguous (N,H,W,16) bf16 on the "
              "GPU");
  TORCH_CHECK(dense_like(dout, maps) && dense_like(rwb, maps) &&
                  dense_like(rce, maps) && dense_like(rgc, maps),
              "fusion_bwd: dout, rwb, rce and rgc must be contiguous, of "
              "maps' dtype, shape and device");
  const long NHW = maps.size(0) * maps.size(1) * maps.size(2);
  auto dmaps = at::empty_like(maps);
  auto drwb = at::empty_like(maps);
  auto drce = at::empty_like(maps);
  auto drgc = at::empty_like(maps);
  launch1d(k_fusion_bwd, NHW, cbf(dout), cbf(maps), cbf(rwb), cbf(rce),
           cbf(rgc), bf(dmaps), bf(drwb), bf(drce), bf(drgc), NHW);
  return {dmaps, drwb, drce, drgc};
}

at::Tensor act_bwd(const at::Tensor& dy, const at::Tensor& y, int64_t act) {
  TORCH_CHECK(dense(dy, at::kBFloat16) && dense_like(y, dy),
              "act_bwd: dy and y must be contiguous bf16 on the GPU, of one "
              "shape and device");
  TORCH_CHECK(act == ACT_RELU || act == ACT_SIGMOID,
              "act_bwd: act must be relu (1) or sigmoid (2)");
  auto dpre = at::empty_like(dy);
  const long n = dy.numel();
  launch1d(k_act_bwd, (n + 7) / 8, cbf(dy), cbf(y), bf(dpre), n, (int)act);
  return dpre;
}

at::Tensor act_bwd_bias(const at::Tensor& dy, const at::Tensor& y,
                        int64_t act, at::Tensor& db) {
  TORCH_CHECK(dense(dy, at::kBFloat16, 4) && dense_like(y, dy),
              "act_bwd_bias: dy and y must be contiguous (N,H,W,Kp) bf16 on "
              "the GPU, of one shape and device");
  TORCH_CHECK(dense(db, at::kFloat, 1) && db.device() == dy.device(),
              "act_bwd_bias: db must be a contiguous 1-D fp32 tensor on dy's "
              "device");
  TORCH_CHECK(act == ACT_RELU || act == ACT_SIGMOID,
              "act_bwd_bias: act must be relu (1) or sigmoid (2)");
  const int Kp = (int)dy.size(3);
  TORCH_CHECK(Kp >= 8 && Kp <= 128 && (Kp & (Kp - 1)) == 0,
              "act_bwd_bias: Kp power of two in [8, 128]");
  const int K = (int)db.size(0);
  TORCH_CHECK(K <= Kp, "act_bwd_bias: db longer than Kp");
  auto dpre = at::empty_like(dy);
  const long n = dy.numel();
  if (n == 0 || K == 0) return dpre;
  const long n8 = n / 8;
  // blocks*blockDim*8 must be divisible by Kp: 256*8 = 2048 is divisible
  // by every Kp <= 128, so any block count works
  const int blocks = grid1d(n8, TPB, 512);
  auto part = at::empty({blocks, (long)Kp},
                        dy.options().dtype(at::kFloat));
  hipLaunchKernelGGL(k_act_bwd_bias, dim3(blocks), dim3(TPB), 0,
                     cur_stream(), cbf(dy), cbf(y), bf(dpre),
                     part.data_ptr<float>(), n8, Kp, (int)act);
  HIP_CHECK_LAST();
  hipLaunchKernelGGL(k_abb_reduce, dim3(K), dim3(256), 0, cur_stream(),
                     part.data_ptr<float>(), db.data_ptr<float>(), Kp, K,
                     blocks);
  HIP_CHECK_LAST();
  return dpre;
}

at::Tensor sqdiff255_sum(const at::Tensor& a, const at::Tensor& b,
                         int64_t Clog) {
  TORCH_CHECK(dense(a, at::kBFloat16, 4) && dense_like(b, a),
              "sqdiff255_sum: a and b must be contiguous (N,H,W,Cp) bf16 on "
              "the GPU, of one shape and device");
  const long Cp = a.size(3), n = a.numel();
  TORCH_CHECK(logical_channels(Clog, Cp),
              "sqdiff255_sum: Clog must be in [1, Cp]");
  auto out = at::zeros({}, a.options().dtype(at::kDouble));
  if (Clog == Cp)
    launch1d_capped(k_sqdiff255_flat, (n + 7) / 8, SQD_MAX_BLOCKS, cbf(a),
                    cbf(b), out.data_ptr<double>(), n);
  else
    launch1d_capped(k_sqdiff255_pix, n / Cp, SQD_MAX_BLOCKS, cbf(a), cbf(b),
                    out.data_ptr<double>(), n / Cp, (int)Clog, (int)Cp);
  return out;
}

at::Tensor sqdiff255_bwd(const at::Tensor& a, const at::Tensor& b,
                         const at::Tensor& gscale, double sign) {
  TORCH_CHECK(dense(a, at::kBFloat16) && dense_like(b, a),
              "sqdiff255_bwd: a and b must be contiguous bf16 on the GPU, of "
              "one shape and device");
  TORCH_CHECK(device_scalar(gscale, at::kFloat, a) && gscale.numel() == 1,
              "sqdiff255_bwd: gscale must be one fp32 value on a's device");
  auto da = at::empty_like(a);
  const long n = a.numel();
  launch1d(k_sqdiff255_bwd, n, cbf(a), cbf(b), gscale.data_ptr<float>(),
           bf(da), n, (float)sign);
  return da;
}

void adam_step(at::Tensor& p, const at::Tensor& g, at::Tensor& m,
               at::Tensor& v, const at::Tensor& lr_buf, double b1, double b2,
               double eps, at::Tensor& step_buf) {
  TORCH_CHECK(dense(p, at::kFloat),
              "adam_step: p must be contiguous fp32 on the GPU");
  TORCH_CHECK(dense_like(g, p) && dense_like(m, p) && dense_like(v, p),
              "adam_step: g, m and v must be contiguous, of p's dtype, shape "
              "and device");
  TORCH_CHECK(device_scalar(lr_buf, at::kFloat, p) &&
                  device_scalar(step_buf, at::kInt, p),
              "adam_step: lr_buf (fp32) and step_buf (int32) must hold a "
              "value on p's device");
  const long n = p.numel();
  if (n == 0) return;
  hipLaunchKernelGGL(k_adam_tick, dim3(1), dim3(64), 0, cur_stream(),
                     step_buf.data_ptr<int>());
  launch1d(k_adam, n, p.data_ptr<float>(), g.data_ptr<float>(),
           m.data_ptr<float>(), v.data_ptr<float>(), n,
           lr_buf.data_ptr<float>(), (float)b1, (float)b2, (float)eps,
           step_buf.data_ptr<int>());
}

// ---------------------------------------------------------------------------
// Device-resident dataset cache: gather a minibatch of cached uint8 HWC
// pairs into the engine's input buffers under the joint flip/rot90
// augmentation (data/augment.py PairedAugment), one launch for raw + ref.
// grid = (tiles, B, 2): blockIdx.y is the batch slot (its index and code
// are block-uniform), blockIdx.z picks raw / ref. Index math and the LDS
// tile scheme: gather_augment.h.
// ---------------------------------------------------------------------------

__global__ __launch_bounds__(GA_THREADS) void k_gather_augment_u8(
    const uint8_t* __restrict__ cache_raw,
    const uint8_t* __restrict__ cache_ref, const int* __restrict__ idx,
    const int* __restrict__ codes, uint8_t* __restrict__ out_raw,
    uint8_t* __restrict__ out_ref, int Nc, int H, int W, int tiles_x,
    int allow_transpose) {
  __shared__ __attribute__((aligned(16))) uint8_t lds[GA_LDS_BYTES];
  const int slot = blockIdx.y;
  // unsigned min: a negative or too-large index can never read outside
  // the cache (the Python layer validates on the host before upload)
  const unsigned n = min((unsigned)idx[slot], (unsigned)(Nc - 1));
  const int tile_y = blockIdx.x / tiles_x;
  const int tile_x = blockIdx.x - tile_y * tiles_x;
  const GaTile t = ga_make_tile(codes[slot], allow_transpose != 0, H, W,
                                tile_y, tile_x);
  const size_t img = (size_t)H * W * 3;
  const uint8_t* src = (blockIdx.z ? cache_ref : cache_raw) + n * img;
  uint8_t* dst = (blockIdx.z ? out_ref : out_raw) + (size_t)slot * img;
  ga_load_tile(t, threadIdx.x, W, src, lds);
  __syncthreads();
  ga_store_tile(t, threadIdx.x, W, lds, dst);
}

void gather_augment_u8(const at::Tensor& cache_raw,
                       const at::Tensor& cache_ref, const at::Tensor& idx,
                       const at::Tensor& codes, at::Tensor& out_raw,
                       at::Tensor& out_ref, bool allow_transpose) {
  TORCH_CHECK(dense(cache_raw, at::kByte, 4) && cache_raw.size(3) == 3 &&
                  cache_raw.size(0) >= 1 && dense_like(cache_ref, cache_raw),
              "gather_augment_u8: the caches must be contiguous (Nc>=1,H,W,3) "
              "uint8 on the GPU, of one shape and device");
  TORCH_CHECK(dense(idx, at::kInt, 1) && dense_like(codes, idx) &&
                  idx.device() == cache_raw.device(),
              "gather_augment_u8: idx and codes must both be contiguous (B,) "
              "int32 on the caches' device");
  const long Nc = cache_raw.size(0), H = cache_raw.size(1),
             W = cache_raw.size(2), B = idx.size(0);
  TORCH_CHECK(dense(out_raw, at::kByte, 4) &&
                  out_raw.sizes() == at::IntArrayRef({B, H, W, 3}) &&
                  out_raw.device() == cache_raw.device() &&
                  dense_like(out_ref, out_raw),
              "gather_augment_u8: the outputs must be contiguous (B,H,W,3) "
              "uint8 matching the caches and idx, on their device");
  TORCH_CHECK(H % 8 == 0 && W % 8 == 0,
              "gather_augment_u8: H and W must be divisible by 8");
  TORCH_CHECK(!allow_transpose || H == W,
              "gather_augment_u8: allow_transpose (odd rot90 k) needs H == W");
  TORCH_CHECK(Nc < (1L << 31) && B <= 65535,
              "gather_augment_u8: Nc < 2^31 and B <= 65535");
  // dword accesses: image bases are multiples of 192 B off these pointers
  TORCH_CHECK(((uintptr_t)cache_raw.data_ptr() | (uintptr_t)cache_ref.data_ptr() |
               (uintptr_t)out_raw.data_ptr() | (uintptr_t)out_ref.data_ptr()) %
                      4 == 0,
              "gather_augment_u8: tensors must be 4-byte aligned");
  if (B == 0) return;
  const int tiles_x = (int)((W + GA_TILE - 1) / GA_TILE);
  const int tiles_y = (int)((H + GA_TILE - 1) / GA_TILE);
  hipLaunchKernelGGL(k_gather_augment_u8,
                     dim3((unsigned)(tiles_x * tiles_y), (unsigned)B, 2),
                     dim3(GA_THREADS), 0, cur_stream(),
                     cache_raw.data_ptr<uint8_t>(),
                     cache_ref.data_ptr<uint8_t>(), idx.data_ptr<int>(),
                     codes.data_ptr<int>(), out_raw.data_ptr<uint8_t>(),
                     out_ref.data_ptr<uint8_t>(), (int)Nc, (int)H, (int)W,
                     tiles_x, (int)allow_transpose);
  HIP_CHECK_LAST();
}
