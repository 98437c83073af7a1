// Host-side vocabulary of the elementwise / pool / ssim / preprocess
// wrappers: the stream, the capped 1-D grid and the argument checks. The
// kernels index raw data_ptr()s as dense arrays, so a wrapper proves every
// extent they rely on, with a message that starts with its own name, before
// it launches anything:
//   TORCH_CHECK(dense(x, at::kBFloat16, 4) && has_rgb(x.size(3)),
//               "out_to_u8: x must be ...");
#pragma once

#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>

#include <algorithm>

#include "common.h"

namespace {

inline hipStream_t cur_stream() { return at::cuda::getCurrentHIPStream(); }

constexpr int TPB = 256;

// Blocks of a grid-stride loop over n > 0 items. 0 items give 0 blocks,
// which is no valid launch: a wrapper returns its empty result before.
inline int grid1d(long n, int tpb = TPB, int cap = 4096) {
  return (int)std::min<long>(cap, (n + tpb - 1) / tpb);
}

// One grid-stride launch of `kernel` over n items on the current stream;
// nothing for n == 0, so an empty input costs no launch.
template <class K, class... A>
inline void launch1d_capped(K kernel, long n, int cap, A... args) {
  if (n == 0) return;
  hipLaunchKernelGGL(kernel, dim3(grid1d(n, TPB, cap)), dim3(TPB), 0,
                     cur_stream(), args...);
  HIP_CHECK_LAST();
}
template <class K, class... A>
inline void launch1d(K kernel, long n, A... args) {
  launch1d_capped(kernel, n, 4096, args...);
}

// A `rank`-D tensor of `dt` on the GPU, any strides: for the wrappers that
// take a contiguous copy (held in a named local, so it outlives the launch).
inline bool on_gpu(const at::Tensor& t, at::ScalarType dt, int rank) {
  return t.is_cuda() && t.scalar_type() == dt && t.dim() == rank;
}

// The same, usable through data_ptr() as it stands.
inline bool dense(const at::Tensor& t, at::ScalarType dt, int rank) {
  return on_gpu(t, dt, rank) && t.is_contiguous();
}

// Any rank.
inline bool dense(const at::Tensor& t, at::ScalarType dt) {
  return t.is_cuda() && t.scalar_type() == dt && t.is_contiguous();
}

// t may stand where ref does: same dtype, shape and device.
inline bool like(const at::Tensor& t, const at::Tensor& ref) {
  return t.scalar_type() == ref.scalar_type() && t.sizes() == ref.sizes() &&
         t.device() == ref.device();
}

// ... and is contiguous, as the dense ref is.
inline bool dense_like(const at::Tensor& t, const at::Tensor& ref) {
  return like(t, ref) && t.is_contiguous();
}

// One value of `dt` (or more) on ref's device, read by a kernel.
inline bool device_scalar(const at::Tensor& t, at::ScalarType dt,
                          const at::Tensor& ref) {
  return t.is_cuda() && t.scalar_type() == dt && t.is_contiguous() &&
         t.numel() >= 1 && t.device() == ref.device();
}

// Channel rules. The RGB kernels touch channels 0..2 of a padded pixel; the
// layout bridges move 16 channels per block in 16-byte vectors; a reduction
// over the logical channels reads 1..Cp of them.
inline bool has_rgb(long Cp) { return Cp >= 3; }
inline bool bridge_channels(long C, long Cp) {
  return Cp > 0 && Cp % 16 == 0 && C >= 0 && C <= Cp;
}
inline bool logical_channels(long Clog, long Cp) {
  return Clog >= 1 && Clog <= Cp;
}

}  // namespace
