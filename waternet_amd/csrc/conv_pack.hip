// Weight packing for the MFMA conv engine (gfx950):
//   - k_pack_fwd / k_pack_dgrad / k_pack_all: NCHW fp32 masters -> bf16
//     packed k-major [Kp][R*S*Cp] (fwd, read by conv_fwd.hip's B staging)
//     and c-major rotated [Cp][R*S*Kp] (dgrad) layouts. Pad rows / channels
//     are written as zeros, which the GEMMs rely on.

#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>

#include "common.h"

// Fill of the fwd layout out[Kp][RS*Cp] from Wm (K,C,R,S) by `stride`
// threads, this one starting at element `first`.
WN_DEVFN void pack_fwd(const float* Wm, bf16_t* out, int K, int C, int R,
                       int S, int Kp, int Cp, long first, long stride) {
  const int KG = R * S * Cp;
  const long total = (long)Kp * KG;
  for (long idx = first; idx < total; idx += stride) {
    int k = (int)(idx / KG);
    int rsc = (int)(idx - (long)k * KG);
    int tap = rsc / Cp, c = rsc - (rsc / Cp) * Cp;
    int r = tap / S, s = tap - (tap / S) * S;
    float v = (k < K && c < C) ? Wm[(((long)k * C + c) * R + r) * S + s] : 0.f;
    out[idx] = f2bf(v);
  }
}

// The same for the dgrad layout out[Cp][RS*Kp], taps rotated 180.
WN_DEVFN void pack_dgrad(const float* Wm, bf16_t* out, int K, int C, int R,
                         int S, int Kp, int Cp, long first, long stride) {
  const int KG = R * S * Kp;
  const long total = (long)Cp * KG;
  for (long idx = first; idx < total; idx += stride) {
    int c = (int)(idx / KG);
    int rsk = (int)(idx - (long)c * KG);
    int tap = rsk / Kp, k = rsk - (rsk / Kp) * Kp;
    int rr = tap / S, ss = tap - (tap / S) * S;
    int r = R - 1 - rr, s = S - 1 - ss;  // rotate 180
    float v = (c < C && k < K) ? Wm[(((long)k * C + c) * R + r) * S + s] : 0.f;
    out[idx] = f2bf(v);
  }
}

__global__ void k_pack_fwd(const float* __restrict__ Wm,  // (K,C,R,S)
                           bf16_t* __restrict__ out,      // [Kp][RS*Cp]
                           int K, int C, int R, int S, int Kp, int Cp) {
  pack_fwd(Wm, out, K, C, R, S, Kp, Cp,
           (long)blockIdx.x * blockDim.x + threadIdx.x,
           (long)gridDim.x * blockDim.x);
}

__global__ void k_pack_dgrad(const float* __restrict__ Wm,  // (K,C,R,S)
                             bf16_t* __restrict__ out,      // [Cp][RS*Kp]
                             int K, int C, int R, int S, int Kp, int Cp) {
  pack_dgrad(Wm, out, K, C, R, S, Kp, Cp,
             (long)blockIdx.x * blockDim.x + threadIdx.x,
             (long)gridDim.x * blockDim.x);
}

// Batched repack: one launch packs EVERY layer's fwd + dgrad layouts from
// the fp32 masters (the per-layer k_pack_* launches cost ~5 us each x 36
// per training step under the lazy per-ConvSpec refresh). desc: int64
// [njobs][9] = (Wm, wp, wd, K, C, R, S, Kp, Cp).
__global__ void k_pack_all(const long* __restrict__ desc, int njobs) {
  const long tid0 = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long nthreads = (long)gridDim.x * blockDim.x;
  for (int j = 0; j < njobs; ++j) {
    const long* d = desc + (long)j * 9;
    const float* Wm = reinterpret_cast<const float*>(d[0]);
    const int K = (int)d[3], C = (int)d[4], R = (int)d[5], S = (int)d[6];
    const int Kp = (int)d[7], Cp = (int)d[8];
    pack_fwd(Wm, reinterpret_cast<bf16_t*>(d[1]), K, C, R, S, Kp, Cp, tid0,
             nthreads);
    pack_dgrad(Wm, reinterpret_cast<bf16_t*>(d[2]), K, C, R, S, Kp, Cp, tid0,
               nthreads);
  }
}

void pack_all(const at::Tensor& desc, int64_t njobs) {
  TORCH_CHECK(desc.is_cuda() && desc.dtype() == at::kLong &&
              desc.is_contiguous());
  hipStream_t stream = at::cuda::getCurrentHIPStream();
  hipLaunchKernelGGL(k_pack_all, dim3(512), dim3(256), 0, stream,
                     desc.data_ptr<long>(), (int)njobs);
  HIP_CHECK_LAST();
}

namespace {
// out = (rows, R*S*cols) bf16 packed from the (K,C,R,S) fp32 master w
template <class Kernel>
at::Tensor pack_weight(const at::Tensor& w, int64_t rows, int64_t cols,
                       Kernel kernel, int64_t Kp, int64_t Cp) {
  TORCH_CHECK(w.is_cuda() && w.dtype() == at::kFloat && w.dim() == 4);
  TORCH_CHECK(w.is_contiguous());
  const int K = w.size(0), C = w.size(1), R = w.size(2), S = w.size(3);
  auto out = at::empty({rows, (long)R * S * cols},
                       w.options().dtype(at::kBFloat16));
  const long total = out.numel();
  const int blocks = (int)std::min<long>(2048, (total + 255) / 256);
  hipStream_t stream = at::cuda::getCurrentHIPStream();
  hipLaunchKernelGGL(kernel, dim3(blocks), dim3(256), 0, stream,
                     w.data_ptr<float>(), (bf16_t*)out.data_ptr(), K, C, R, S,
                     (int)Kp, (int)Cp);
  HIP_CHECK_LAST();
  return out;
}
}  // namespace

at::Tensor pack_weight_fwd(const at::Tensor& w, int64_t Kp, int64_t Cp) {
  return pack_weight(w, Kp, Cp, k_pack_fwd, Kp, Cp);
}

// output [Cp][RS*Kp]: dgrad conv consumes dY (channels Kp) and produces
// dX (channels Cp); weights rotated 180 and transposed.
at::Tensor pack_weight_dgrad(const at::Tensor& w, int64_t Kp, int64_t Cp) {
  return pack_weight(w, Cp, Kp, k_pack_dgrad, Kp, Cp);
}
