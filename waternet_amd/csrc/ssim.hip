// SSIM on gfx950: 11x11 gaussian-weighted window
// statistics + reduction, matching waternet_amd.utils.metrics._ssim_torch
// (valid convolution, sigma 1.5, k1/k2 configurable).
//
// Each 16x16-thread block computes a 16x16 tile of valid window positions
// for one (n,c) plane from an LDS-staged 26x26 patch and writes one fp32
// partial; the host sums the partials in f64. ssim_body is the one kernel
// body: k_ssim (NCHW fp32) and k_ssim_nhwc (padded NHWC bf16) hand it their
// plane's first element and the distance between neighbouring pixels.
//
// Loss path (ssim_fwd_save_nhwc / ssim_bwd_nhwc): k_ssim_nhwc_save is the
// same body with SAVE set; besides the partial it stores, per valid window
// q, the three derivatives of S(q) that the backward needs
//   D1 = dS/dsx, D2 = dS/dsxx, D3 = dS/dsxy
// as fp32 maps (N, Clog, 3, OH, OW). k_ssim_nhwc_bwd is the transposed
// (full) correlation of those maps with the same window:
//   dx(p) = gscale * sum_{q in window(p)} w(p-q) * [D1 + 2 x(p) D2 + y(p) D3](q)
// so no window statistic is recomputed and no 36x36 input halo is read.

#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>

#include "common.h"
#include "host_check.h"

#define SSIM_K 11
#define SSIM_TILE 16
#define SSIM_PATCH (SSIM_TILE + SSIM_K - 1)  // 26
// Row stride (floats) of the backward's LDS patches: 48 = 16 mod 32, so the
// two 16-lane rows that share a 32-lane ds_read_b32 group land on disjoint
// banks (the stride 26 of the forward overlaps 10 of them).
#define SSIM_BSTRIDE 48

__constant__ float SSIM_W[SSIM_K * SSIM_K];

WN_DEVFN float ssim_elem(float v) { return v; }
WN_DEVFN float ssim_elem(bf16_t v) { return bf2f(v); }

// a, b: element (0,0) of this block's plane; pixel (iy,ix) lies
// (iy*W + ix) * stride elements further on
// SAVE: also store D1, D2, D3 of every valid window at
// dmaps[k * OH * OW + oy * OW + ox] (dmaps = this block's plane triple).
template <bool SAVE, class T>
WN_DEVFN void ssim_body(const T* __restrict__ a, const T* __restrict__ b,
                        long stride, float* __restrict__ partials,
                        float* __restrict__ dmaps, int H, int W, int OH,
                        int OW, float c1, float c2) {
  __shared__ __attribute__((aligned(16))) float sA[SSIM_PATCH][SSIM_PATCH];
  __shared__ __attribute__((aligned(16))) float sB[SSIM_PATCH][SSIM_PATCH];
  __shared__ float red[4];

  const int oy0 = blockIdx.y * SSIM_TILE;
  const int ox0 = blockIdx.x * SSIM_TILE;
  const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;

  // stage patch (26x26 <= 2 passes of 16x16 + edges)
  for (int yy = ty; yy < SSIM_PATCH; yy += 16)
    for (int xx = tx; xx < SSIM_PATCH; xx += 16) {
      int iy = oy0 + yy, ix = ox0 + xx;
      bool v = iy < H && ix < W;
      const long off = ((long)iy * W + ix) * stride;
      sA[yy][xx] = v ? ssim_elem(a[off]) : 0.f;
      sB[yy][xx] = v ? ssim_elem(b[off]) : 0.f;
    }
  __syncthreads();

  float ssim = 0.f;
  const int oy = oy0 + ty, ox = ox0 + tx;
  if (oy < OH && ox < OW) {
    float sx = 0.f, sy = 0.f, sxx = 0.f, syy = 0.f, sxy = 0.f;
#pragma unroll 1
    for (int ky = 0; ky < SSIM_K; ++ky) {
#pragma unroll
      for (int kx = 0; kx < SSIM_K; ++kx) {
        float w = SSIM_W[ky * SSIM_K + kx];
        float xa = sA[ty + ky][tx + kx];
        float xb = sB[ty + ky][tx + kx];
        sx += w * xa;
        sy += w * xb;
        sxx += w * xa * xa;
        syy += w * xb * xb;
        sxy += w * xa * xb;
      }
    }
    float vx = sxx - sx * sx;
    float vy = syy - sy * sy;
    float cxy = sxy - sx * sy;
    float num = (2.f * sx * sy + c1) * (2.f * cxy + c2);
    float den = (sx * sx + sy * sy + c1) * (vx + vy + c2);
    ssim = num / den;
    if constexpr (SAVE) {
      // S = a1 a2 / (b1 b2); the metric value above is left as it is, so
      // both instantiations return the same bits
      const float a1 = 2.f * sx * sy + c1, a2 = 2.f * cxy + c2;
      const float b1 = sx * sx + sy * sy + c1, b2 = vx + vy + c2;
      const float rb1 = 1.f / b1, rb2 = 1.f / b2;
      const long plane = (long)OH * OW, o = (long)oy * OW + ox;
      dmaps[o] = 2.f * sy * (a2 - a1) * rb1 * rb2 -
                 2.f * sx * ssim * (rb1 - rb2);
      dmaps[plane + o] = -ssim * rb2;
      dmaps[2 * plane + o] = 2.f * a1 * rb1 * rb2;
    }
  }
  // wave reduce -> LDS -> ONE fp32 partial per block (a single f64
  // accumulator serialized ~9.4K atomics and dominated the kernel)
  for (int off = 32; off > 0; off >>= 1) ssim += __shfl_down(ssim, off, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = ssim;
  __syncthreads();
  if (threadIdx.x == 0) {
    const int bid =
        (blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
    partials[bid] = red[0] + red[1] + red[2] + red[3];
  }
}

__global__ void k_ssim(const float* __restrict__ A,
                       const float* __restrict__ B,
                       float* __restrict__ partials, int H, int W, int OH,
                       int OW, float c1, float c2) {
  const long plane = (long)blockIdx.z * H * W;  // blockIdx.z = n*C + c
  ssim_body<false>(A + plane, B + plane, 1, partials, nullptr, H, W, OH, OW,
                   c1, c2);
}

// full-NHWC metric path: blockIdx.z decodes (n, logical channel)
__global__ void k_ssim_nhwc(const bf16_t* __restrict__ A,
                            const bf16_t* __restrict__ B,
                            float* __restrict__ partials, int H, int W,
                            int OH, int OW, int Cp, int Clog, float c1,
                            float c2) {
  const int n = blockIdx.z / Clog, c = blockIdx.z - n * Clog;
  const long plane = (long)n * H * W * Cp + c;
  ssim_body<false>(A + plane, B + plane, Cp, partials, nullptr, H, W, OH, OW,
                   c1, c2);
}

// k_ssim_nhwc that also saves the derivative maps (N, Clog, 3, OH, OW)
__global__ void k_ssim_nhwc_save(const bf16_t* __restrict__ A,
                                 const bf16_t* __restrict__ B,
                                 float* __restrict__ partials,
                                 float* __restrict__ dmaps, int H, int W,
                                 int OH, int OW, int Cp, int Clog, float c1,
                                 float c2) {
  const int n = blockIdx.z / Clog, c = blockIdx.z - n * Clog;
  const long plane = (long)n * H * W * Cp + c;
  ssim_body<true>(A + plane, B + plane, Cp, partials,
                  dmaps + (long)blockIdx.z * 3 * OH * OW, H, W, OH, OW, c1,
                  c2);
}

// Backward of mean-SSIM w.r.t. A. One 16x16-thread block owns a 16x16 tile
// of input pixels of image blockIdx.z and walks its logical channels; per
// channel it stages the 26x26 windows q = p - k (k in [0,11)^2) that contain
// a pixel of the tile, zero outside [0,OH)x[0,OW), from the three maps.
// Results are packed 8 channels at a time and stored as 16 B vectors, so a
// Cp = 16 pixel row leaves as two full stores (pad channels are zeros).
__global__ void k_ssim_nhwc_bwd(const bf16_t* __restrict__ A,
                                const bf16_t* __restrict__ B,
                                const float* __restrict__ dmaps,
                                const float* __restrict__ gscale,
                                bf16_t* __restrict__ dA, int H, int W, int OH,
                                int OW, int Cp, int Clog) {
  __shared__ float sD[3][SSIM_PATCH][SSIM_BSTRIDE];

  const int n = blockIdx.z;
  const int py0 = blockIdx.y * SSIM_TILE, px0 = blockIdx.x * SSIM_TILE;
  const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
  const int py = py0 + ty, px = px0 + tx;
  const bool live = py < H && px < W;
  const long pix = (((long)n * H + py) * W + px) * Cp;
  const long plane = (long)OH * OW;
  const float gs = gscale[0];
  const bool vec = (Cp & 7) == 0;  // 16 B stores stay aligned

  for (int c0 = 0; c0 < Cp; c0 += 8) {
    u32x4 pk = {0u, 0u, 0u, 0u};
    const int cend = min(c0 + 8, Clog);
#pragma unroll 1
    for (int c = c0; c < cend; ++c) {
      const float* __restrict__ d = dmaps + ((long)n * Clog + c) * 3 * plane;
      __syncthreads();  // the previous channel's reads are done
      for (int yy = ty; yy < SSIM_PATCH; yy += 16)
        for (int xx = tx; xx < SSIM_PATCH; xx += 16) {
          const int qy = py0 - (SSIM_K - 1) + yy;
          const int qx = px0 - (SSIM_K - 1) + xx;
          const bool v = qy >= 0 && qy < OH && qx >= 0 && qx < OW;
          const long o = (long)qy * OW + qx;
#pragma unroll
          for (int k = 0; k < 3; ++k)
            sD[k][yy][xx] = v ? d[k * plane + o] : 0.f;
        }
      __syncthreads();

      float g1 = 0.f, g2 = 0.f, g3 = 0.f;
#pragma unroll 1
      for (int ky = 0; ky < SSIM_K; ++ky) {
#pragma unroll
        for (int kx = 0; kx < SSIM_K; ++kx) {
          // window q = p - k holds p at offset k: patch (p - k) - (p0 - 10)
          const float w = SSIM_W[ky * SSIM_K + kx];
          const int yy = ty + SSIM_K - 1 - ky, xx = tx + SSIM_K - 1 - kx;
          g1 += w * sD[0][yy][xx];
          g2 += w * sD[1][yy][xx];
          g3 += w * sD[2][yy][xx];
        }
      }
      if (live) {
        const float x = bf2f(A[pix + c]), y = bf2f(B[pix + c]);
        const bf16_t r = f2bf(gs * (g1 + 2.f * x * g2 + y * g3));
        const std::uint32_t bits =
            (std::uint32_t)__builtin_bit_cast(unsigned short, r)
            << (16 * (c & 1));
        const int j = (c - c0) >> 1;
#pragma unroll
        for (int i = 0; i < 4; ++i) pk[i] |= i == j ? bits : 0u;
      }
    }
    if (live) {
      if (vec) {
        *reinterpret_cast<u32x4*>(dA + pix + c0) = pk;
      } else {
#pragma unroll
        for (int e = 0; e < 8; ++e)
          if (c0 + e < Cp)
            dA[pix + c0 + e] = __builtin_bit_cast(
                bf16_t, (unsigned short)(pk[e >> 1] >> (16 * (e & 1))));
      }
    }
  }
}

static void ssim_init_weights() {
  static bool weights_ready = false;
  if (!weights_ready) {
    float g[SSIM_K], w[SSIM_K * SSIM_K];
    float sum = 0.f;
    for (int i = 0; i < SSIM_K; ++i) {
      float d = i - (SSIM_K - 1) / 2.0f;
      g[i] = expf(-(d * d) / (2.f * 1.5f * 1.5f));
      sum += g[i];
    }
    for (int i = 0; i < SSIM_K; ++i) g[i] /= sum;
    for (int i = 0; i < SSIM_K; ++i)
      for (int j = 0; j < SSIM_K; ++j) w[i * SSIM_K + j] = g[i] * g[j];
    hipMemcpyToSymbol(HIP_SYMBOL(SSIM_W), w, sizeof(w));
    weights_ready = true;
  }
}

// The part both entries share: N * planes blocks in z over (H,W) images,
// one partial per block, summed in f64 (the caller divides by the count).
// `launch(grid, partials, OH, OW, c1, c2)` starts the entry's kernel.
template <class Launch>
static at::Tensor ssim_run(const char* name, const at::Tensor& a, long N,
                           long planes, long H, long W, double data_range,
                           double k1, double k2, Launch launch) {
  const long OH = H - SSIM_K + 1, OW = W - SSIM_K + 1;
  TORCH_CHECK(OH > 0 && OW > 0, name, ": image smaller than SSIM window");
  const auto opts = a.options().dtype(at::kFloat);
  if (N * planes == 0) return at::zeros({}, opts.dtype(at::kDouble));
  ssim_init_weights();
  const float c1 = (float)((k1 * data_range) * (k1 * data_range));
  const float c2 = (float)((k2 * data_range) * (k2 * data_range));
  const dim3 grid((OW + 15) / 16, (OH + 15) / 16, N * planes);
  auto partials = at::empty({(long)grid.x * grid.y * grid.z}, opts);
  launch(grid, partials.data_ptr<float>(), (int)OH, (int)OW, c1, c2);
  HIP_CHECK_LAST();
  return partials.sum(at::kDouble);
}

at::Tensor ssim_sum_nhwc(const at::Tensor& a, const at::Tensor& b,
                         int64_t Clog, double data_range, double k1,
                         double k2) {
  TORCH_CHECK(on_gpu(a, at::kBFloat16, 4) && like(b, a),
              "ssim_sum_nhwc: a and b must be (N,H,W,Cp) bf16 on the GPU, of "
              "one shape and device");
  TORCH_CHECK(logical_channels(Clog, a.size(3)),
              "ssim_sum_nhwc: Clog must be in [1, Cp]");
  const auto ac = a.contiguous(), bc = b.contiguous();
  const int H = a.size(1), W = a.size(2), Cp = a.size(3);
  return ssim_run(
      "ssim_sum_nhwc", a, a.size(0), Clog, H, W, data_range, k1, k2,
      [&](dim3 grid, float* partials, int OH, int OW, float c1, float c2) {
        hipLaunchKernelGGL(k_ssim_nhwc, grid, dim3(256), 0, cur_stream(),
                           (const bf16_t*)ac.data_ptr(),
                           (const bf16_t*)bc.data_ptr(), partials, H, W, OH,
                           OW, Cp, (int)Clog, c1, c2);
      });
}

// ssim_sum_nhwc that also returns the derivative maps (N,Clog,3,OH,OW) fp32
// for ssim_bwd_nhwc: {sum (f64 scalar), dmaps}
std::vector<at::Tensor> ssim_fwd_save_nhwc(const at::Tensor& a,
                                           const at::Tensor& b, int64_t Clog,
                                           double data_range, double k1,
                                           double k2) {
  TORCH_CHECK(on_gpu(a, at::kBFloat16, 4) && like(b, a),
              "ssim_fwd_save_nhwc: a and b must be (N,H,W,Cp) bf16 on the "
              "GPU, of one shape and device");
  TORCH_CHECK(logical_channels(Clog, a.size(3)),
              "ssim_fwd_save_nhwc: Clog must be in [1, Cp]");
  const auto ac = a.contiguous(), bc = b.contiguous();
  const int H = a.size(1), W = a.size(2), Cp = a.size(3);
  const auto fopts = a.options().dtype(at::kFloat);
  at::Tensor dmaps;
  auto sum = ssim_run(
      "ssim_fwd_save_nhwc", a, a.size(0), Clog, H, W, data_range, k1, k2,
      [&](dim3 grid, float* partials, int OH, int OW, float c1, float c2) {
        dmaps = at::empty({a.size(0), Clog, 3, OH, OW}, fopts);
        hipLaunchKernelGGL(k_ssim_nhwc_save, grid, dim3(256), 0, cur_stream(),
                           (const bf16_t*)ac.data_ptr(),
                           (const bf16_t*)bc.data_ptr(), partials,
                           dmaps.data_ptr<float>(), H, W, OH, OW, Cp,
                           (int)Clog, c1, c2);
      });
  if (!dmaps.defined())  // empty batch: nothing was launched
    dmaps = at::empty({0, Clog, 3, H - SSIM_K + 1, W - SSIM_K + 1}, fopts);
  return {sum, dmaps};
}

// d(mean SSIM)/da from the saved maps; gscale = upstream grad / count, one
// fp32 value on the device, so the launch can sit in a captured graph.
// Returns (N,H,W,Cp) bf16 with channels >= Clog zero.
at::Tensor ssim_bwd_nhwc(const at::Tensor& a, const at::Tensor& b,
                         const at::Tensor& dmaps, const at::Tensor& gscale,
                         int64_t Clog) {
  TORCH_CHECK(on_gpu(a, at::kBFloat16, 4) && like(b, a),
              "ssim_bwd_nhwc: a and b must be (N,H,W,Cp) bf16 on the GPU, of "
              "one shape and device");
  TORCH_CHECK(logical_channels(Clog, a.size(3)),
              "ssim_bwd_nhwc: Clog must be in [1, Cp]");
  const long N = a.size(0), H = a.size(1), W = a.size(2), Cp = a.size(3);
  const long OH = H - SSIM_K + 1, OW = W - SSIM_K + 1;
  TORCH_CHECK(OH > 0 && OW > 0,
              "ssim_bwd_nhwc: image smaller than SSIM window");
  TORCH_CHECK(dense(dmaps, at::kFloat, 5) && dmaps.device() == a.device() &&
                  dmaps.sizes() == at::IntArrayRef({N, Clog, 3, OH, OW}),
              "ssim_bwd_nhwc: dmaps must be the contiguous (N,Clog,3,OH,OW) "
              "fp32 maps of ssim_fwd_save_nhwc on a's device");
  TORCH_CHECK(device_scalar(gscale, at::kFloat, a),
              "ssim_bwd_nhwc: gscale must be one fp32 value on a's device");
  TORCH_CHECK(N <= 65535, "ssim_bwd_nhwc: at most 65535 images per call");
  if (N == 0) return at::zeros_like(a, at::MemoryFormat::Contiguous);
  ssim_init_weights();
  const auto ac = a.contiguous(), bc = b.contiguous();
  auto da = at::empty(a.sizes(), a.options());
  const dim3 grid((W + 15) / 16, (H + 15) / 16, N);
  hipLaunchKernelGGL(k_ssim_nhwc_bwd, grid, dim3(256), 0, cur_stream(),
                     (const bf16_t*)ac.data_ptr(),
                     (const bf16_t*)bc.data_ptr(), dmaps.data_ptr<float>(),
                     gscale.data_ptr<float>(), (bf16_t*)da.data_ptr(), (int)H,
                     (int)W, (int)OH, (int)OW, (int)Cp, (int)Clog);
  HIP_CHECK_LAST();
  return da;
}

at::Tensor ssim_sum(const at::Tensor& a, const at::Tensor& b,
                    double data_range, double k1, double k2) {
  TORCH_CHECK(on_gpu(a, at::kFloat, 4) && like(b, a),
              "ssim_sum: a and b must be (N,C,H,W) fp32 on the GPU, of one "
              "shape and device");
  const auto ac = a.contiguous(), bc = b.contiguous();
  const int H = a.size(2), W = a.size(3);
  return ssim_run(
      "ssim_sum", a, a.size(0), a.size(1), H, W, data_range, k1, k2,
      [&](dim3 grid, float* partials, int OH, int OW, float c1, float c2) {
        hipLaunchKernelGGL(k_ssim, grid, dim3(256), 0, cur_stream(),
                           ac.data_ptr<float>(), bc.data_ptr<float>(),
                           partials, H, W, OH, OW, c1, c2);
      });
}
