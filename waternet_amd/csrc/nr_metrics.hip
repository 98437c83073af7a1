// No-reference quality metrics UIQM (Panetta, Gao, Agaian 2016) and UCIQE
// (Yang, Sowmya 2015) for uint8 NHWC RGB batches, as CDNA4 kernels.
//
// Semantics match waternet_amd/utils/nr_metrics.py (the NumPy float64
// oracle the unit tests compare against). Everything that can be an integer
// is one: the RG / YB2 / L8 histograms, the trimmed sums, the Sobel energy
// (64-bit) and the block extrema are exact, so the only rounding left is in
// double sums of non-negative terms and in log/sqrt of exact arguments.
//
// Three kernels per call, after k_rgb2lab (preprocess.hip) produced the
// 8-bit LAB image UCIQE is defined on:
//   k_nr_hist     grid (N, nsplit): LDS histograms of RG, YB2 and L8 merged
//                 into global ones with integer atomics, plus per-block
//                 double partials of the chroma / saturation sums.
//   k_nr_blocks   one wave64 per 8x8 block, lane = pixel: Sobel energy per
//                 channel, wave max/min, the block's three EME terms and
//                 its UIConM term.
//   k_nr_finalize one block per image: fixed-order sums of the block terms
//                 and partials, one wave per histogram for the trimmed
//                 sums, variances and order statistics, then the five
//                 doubles [uicm, uism, uiconm, uiqm, uciqe].
// No floating-point atomics: two calls on one input return identical bits.

#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>

#include "common.h"

// preprocess.hip
at::Tensor rgb2lab_u8(const at::Tensor& rgb_u8);

namespace {

constexpr int RG_BINS = 511;    // R-G     in [-255, 255]
constexpr int YB_BINS = 1021;   // R+G-2B  in [-510, 510]
constexpr int L_BINS = 256;
constexpr int RG_OFF = 0;
constexpr int YB_OFF = RG_BINS;
constexpr int L_OFF = RG_BINS + YB_BINS;
constexpr int NR_BINS = RG_BINS + YB_BINS + L_BINS;  // 1788
constexpr int NR_THREADS = 256;
constexpr int FIN_THREADS = 1024;  // k_nr_finalize: one block per image
constexpr int NR_PARTS = 3;   // sum d, sum d*d, sum c/l
constexpr int NR_TERMS = 4;   // EME_R, EME_G, EME_B, UIConM

// chroma c = sqrt(a^2+b^2) of one LAB pixel, a = (A8-128)/255
WN_DEVFN double lab_chroma(int A8, int B8) {
  const int ia = A8 - 128, ib = B8 - 128;
  return sqrt((double)(ia * ia + ib * ib)) / 255.0;
}

// fixed-order block sum of one double per thread; result valid on thread 0
template <int THREADS>
WN_DEVFN double block_sum(double v, double* red) {
  __syncthreads();  // red may still be read from a previous call
  red[threadIdx.x] = v;
  __syncthreads();
  for (int s = THREADS / 2; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
    __syncthreads();
  }
  return red[0];
}

}  // namespace

// ---------------------------------------------------------------------------
// Histogram pass
// ---------------------------------------------------------------------------

__global__ __launch_bounds__(NR_THREADS) void k_nr_hist(
    const uint8_t* __restrict__ rgb, const uint8_t* __restrict__ lab,
    unsigned int* __restrict__ hist,  // (N, NR_BINS), zeroed
    double* __restrict__ partials,    // (N, nsplit, NR_PARTS)
    long HW, int nsplit) {
  __shared__ unsigned int h[NR_BINS];
  __shared__ double red[NR_THREADS];
  for (int i = threadIdx.x; i < NR_BINS; i += NR_THREADS) h[i] = 0;
  __syncthreads();
  const long n = blockIdx.x;
  const long chunk = (HW + nsplit - 1) / nsplit;
  const long p0 = blockIdx.y * chunk;
  const long p1 = min(p0 + chunk, HW);
  const uint8_t* rbase = rgb + n * HW * 3;
  const uint8_t* lbase = lab + n * HW * 3;
  // the chroma variance is accumulated about the first pixel's chroma
  // (shifted-data form): exact zero for constant chroma, no cancellation
  const double pivot = lab_chroma(lbase[1], lbase[2]);
  double sd = 0.0, sdd = 0.0, ssat = 0.0;
  // four pixels per trip, all their loads issued before the first use; the
  // pixels of one thread are still visited in ascending order
  constexpr int UNR = 4;
  for (long pb = p0 + threadIdx.x; pb < p1; pb += NR_THREADS * UNR) {
    int px[UNR][6];
#pragma unroll
    for (int u = 0; u < UNR; ++u) {
      const long p = pb + u * NR_THREADS;
      const long q = (p < p1 ? p : pb) * 3;  // in range either way
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        px[u][k] = rbase[q + k];
        px[u][3 + k] = lbase[q + k];
      }
    }
#pragma unroll
    for (int u = 0; u < UNR; ++u) {
      if (pb + u * NR_THREADS >= p1) break;
      const int r = px[u][0], g = px[u][1], b = px[u][2], L8 = px[u][3];
      atomicAdd(&h[RG_OFF + (r - g) + 255], 1u);
      atomicAdd(&h[YB_OFF + (r + g - 2 * b) + 510], 1u);
      atomicAdd(&h[L_OFF + L8], 1u);
      const double c = lab_chroma(px[u][4], px[u][5]);
      const double d = c - pivot;
      sd += d;
      sdd += d * d;
      if (L8 > 0) ssat += c / ((double)L8 / 255.0);
    }
  }
  __syncthreads();
  unsigned int* out = hist + n * NR_BINS;
  for (int i = threadIdx.x; i < NR_BINS; i += NR_THREADS)
    if (h[i]) atomicAdd(&out[i], h[i]);
  double* part = partials + (n * nsplit + blockIdx.y) * NR_PARTS;
  const double t0 = block_sum<NR_THREADS>(sd, red);
  if (threadIdx.x == 0) part[0] = t0;
  const double t1 = block_sum<NR_THREADS>(sdd, red);
  if (threadIdx.x == 0) part[1] = t1;
  const double t2 = block_sum<NR_THREADS>(ssat, red);
  if (threadIdx.x == 0) part[2] = t2;
}

// ---------------------------------------------------------------------------
// Block pass: one wave per 8x8 block
// ---------------------------------------------------------------------------

WN_DEVFN unsigned long long wave_max_u64(unsigned long long v) {
  for (int off = 32; off > 0; off >>= 1) {
    const unsigned long long o = __shfl_xor(v, off, 64);
    v = o > v ? o : v;
  }
  return v;
}
WN_DEVFN unsigned long long wave_min_u64(unsigned long long v) {
  for (int off = 32; off > 0; off >>= 1) {
    const unsigned long long o = __shfl_xor(v, off, 64);
    v = o < v ? o : v;
  }
  return v;
}

__global__ __launch_bounds__(NR_THREADS) void k_nr_blocks(
    const uint8_t* __restrict__ rgb,
    double* __restrict__ terms,  // (N, k2*k1, NR_TERMS)
    int H, int W, int k1, int k2, long nblocks /* N*k2*k1 */) {
  const long wave = (long)blockIdx.x * (NR_THREADS / WAVE) + (threadIdx.x >> 6);
  if (wave >= nblocks) return;  // wave-uniform; no barrier below
  const int lane = threadIdx.x & 63;
  const long per_img = (long)k1 * k2;
  const long n = wave / per_img;
  const int blk = (int)(wave - n * per_img);
  const int by = blk / k1, bx = blk - by * k1;
  const int y = by * 8 + (lane >> 3), x = bx * 8 + (lane & 7);
  const uint8_t* base = rgb + n * (long)H * W * 3;
  // replicate border on the full image, not on the block grid
  const long ro[3] = {(long)max(y - 1, 0) * W, (long)y * W,
                      (long)min(y + 1, H - 1) * W};
  const int xo[3] = {max(x - 1, 0), x, min(x + 1, W - 1)};
  int vmax = 0, vmin = 255;
  double term[NR_TERMS];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    int p[3][3];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int j = 0; j < 3; ++j) p[i][j] = base[(ro[i] + xo[j]) * 3 + c];
    const int gx = (p[0][2] + 2 * p[1][2] + p[2][2]) -
                   (p[0][0] + 2 * p[1][0] + p[2][0]);
    const int gy = (p[2][0] + 2 * p[2][1] + p[2][2]) -
                   (p[0][0] + 2 * p[0][1] + p[0][2]);
    const int v = p[1][1];
    // (gx^2+gy^2) <= 2*1020^2 fits 32 bits; times v^2 it needs 64
    const unsigned long long e2 =
        (unsigned long long)(gx * gx + gy * gy) * (unsigned long long)(v * v);
    const unsigned long long mx = wave_max_u64(e2);
    const unsigned long long mn = wave_min_u64(e2);
    term[c] = mn == 0 ? 0.0 : 0.5 * log((double)mx / (double)mn);
    vmax = max(vmax, v);
    vmin = min(vmin, v);
  }
  for (int off = 32; off > 0; off >>= 1) {
    vmax = max(vmax, __shfl_xor(vmax, off, 64));
    vmin = min(vmin, __shfl_xor(vmin, off, 64));
  }
  const int t = vmax - vmin, s = vmax + vmin;
  if (t == 0) {
    term[3] = 0.0;
  } else {
    const double q = (double)t / (double)s;
    term[3] = q * log(q);
  }
  if (lane == 0) {
    double* o = terms + wave * NR_TERMS;
#pragma unroll
    for (int i = 0; i < NR_TERMS; ++i) o[i] = term[i];
  }
}

// ---------------------------------------------------------------------------
// Finalize: one block per image
// ---------------------------------------------------------------------------

namespace {

// exclusive prefix sum over the wave
WN_DEVFN long long wave_excl_scan(long long v, int lane) {
  long long inc = v;
  for (int off = 1; off < WAVE; off <<= 1) {
    const long long o = __shfl_up(inc, off, WAVE);
    if (lane >= off) inc += o;
  }
  return inc - v;
}

// One wave walks one histogram, lane l owning the bins [l*per, (l+1)*per):
// mean of sorted[lo:hi) and the sum over all of cnt*(x-mu)^2, where bin v
// holds the value (v - off) * scale. The trimmed sum is an exact integer;
// the squares are summed per lane, then by a butterfly (a fixed order).
__device__ void wave_trimmed_moments(const unsigned int* h, int bins, int off,
                                     double scale, long long lo, long long hi,
                                     int lane, double* mu_out,
                                     double* ss_out) {
  const int per = (bins + WAVE - 1) / WAVE;
  const int v0 = lane * per, v1 = min(v0 + per, bins);
  long long seg = 0;
  for (int v = v0; v < v1; ++v) seg += h[v];
  long long cum = wave_excl_scan(seg, lane);
  long long tsum = 0;
  for (int v = v0; v < v1; ++v) {
    const long long cnt = h[v];
    const long long take = min(cum + cnt, hi) - max(cum, lo);
    if (take > 0) tsum += take * (long long)(v - off);
    cum += cnt;
  }
  for (int o = WAVE / 2; o > 0; o >>= 1) tsum += __shfl_xor(tsum, o, WAVE);
  const double mu = ((double)tsum * scale) / (double)(hi - lo);
  double ss = 0.0;
  for (int v = v0; v < v1; ++v) {
    const double d = (double)(v - off) * scale - mu;
    ss += (double)h[v] * (d * d);
  }
  for (int o = WAVE / 2; o > 0; o >>= 1) ss += __shfl_xor(ss, o, WAVE);
  if (lane == 0) {
    *mu_out = mu;
    *ss_out = ss;
  }
}

// value of rank r (0-based) in the sorted multiset the histogram describes;
// every lane returns it
__device__ int wave_order_stat(const unsigned int* h, int bins, long long r,
                               int lane) {
  const int per = (bins + WAVE - 1) / WAVE;
  const int v0 = lane * per, v1 = min(v0 + per, bins);
  long long seg = 0;
  for (int v = v0; v < v1; ++v) seg += h[v];
  long long cum = wave_excl_scan(seg, lane);
  int found = bins - 1;
  for (int v = v1 - 1; v >= v0; --v) {  // smallest v of the segment wins
    if (cum + seg > r) found = v;
    seg -= h[v];
  }
  for (int o = WAVE / 2; o > 0; o >>= 1)
    found = min(found, __shfl_xor(found, o, WAVE));
  return found;
}

}  // namespace

__global__ __launch_bounds__(FIN_THREADS) void k_nr_finalize(
    const unsigned int* __restrict__ hist, const double* __restrict__ partials,
    const double* __restrict__ terms, double* __restrict__ out,  // (N,5)
    long HW, int nsplit, long per_img) {
  __shared__ unsigned int h[NR_BINS];
  __shared__ double red[FIN_THREADS];
  __shared__ double sums[NR_TERMS + NR_PARTS];
  __shared__ double walk[5];  // mu_rg, ss_rg, mu_yb, ss_yb, con
  const long n = blockIdx.x;
  for (int i = threadIdx.x; i < NR_BINS; i += FIN_THREADS)
    h[i] = hist[n * NR_BINS + i];

  // fixed-order sums: thread t takes every FIN_THREADS-th entry, then a tree
  const double* tb = terms + n * per_img * NR_TERMS;
  double ts[NR_TERMS] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll 4
  for (long i = threadIdx.x; i < per_img; i += FIN_THREADS) {
#pragma unroll
    for (int k = 0; k < NR_TERMS; ++k) ts[k] += tb[i * NR_TERMS + k];
  }
#pragma unroll
  for (int k = 0; k < NR_TERMS; ++k) {
    const double s = block_sum<FIN_THREADS>(ts[k], red);
    if (threadIdx.x == 0) sums[k] = s;
  }
  const double* pb = partials + n * nsplit * NR_PARTS;
  for (int k = 0; k < NR_PARTS; ++k) {
    double s = 0.0;
    for (int i = threadIdx.x; i < nsplit; i += FIN_THREADS)
      s += pb[i * NR_PARTS + k];
    s = block_sum<FIN_THREADS>(s, red);
    if (threadIdx.x == 0) sums[NR_TERMS + k] = s;
  }
  __syncthreads();  // h and sums complete

  // the three histogram walks, one wave each
  const long long T_L = (HW + 9) / 10, T_R = HW / 10;
  const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
  if (wv == 0) {
    wave_trimmed_moments(h + RG_OFF, RG_BINS, 255, 1.0, T_L, HW - T_R, lane,
                         &walk[0], &walk[1]);
  } else if (wv == 1) {
    wave_trimmed_moments(h + YB_OFF, YB_BINS, 510, 0.5, T_L, HW - T_R, lane,
                         &walk[2], &walk[3]);
  } else if (wv == 2) {
    const long long r_hi = min((long long)HW - 1, (99LL * HW) / 100);
    const int hi = wave_order_stat(h + L_OFF, L_BINS, r_hi, lane);
    const int lo = wave_order_stat(h + L_OFF, L_BINS, HW / 100, lane);
    if (lane == 0) walk[4] = (double)(hi - lo) / 255.0;
  }
  __syncthreads();

  if (threadIdx.x == 0) {
    const double Nd = (double)HW;
    const double mu_rg = walk[0], mu_yb = walk[2];
    const double var_rg = walk[1] / Nd, var_yb = walk[3] / Nd;
    const double uicm = -0.0268 * sqrt(mu_rg * mu_rg + mu_yb * mu_yb) +
                        0.1586 * sqrt(var_rg + var_yb);
    const double kk = 2.0 / (double)per_img;
    const double uism = 0.299 * (kk * sums[0]) + 0.587 * (kk * sums[1]) +
                        0.114 * (kk * sums[2]);
    const double uiconm = -(1.0 / (double)per_img) * sums[3];
    const double uiqm = 0.0282 * uicm + 0.2953 * uism + 3.5753 * uiconm;
    const double md = sums[4] / Nd;
    const double var_c = fmax(0.0, sums[5] / Nd - md * md);
    const double mu_s = sums[6] / Nd;
    const double uciqe =
        0.4680 * sqrt(var_c) + 0.2745 * walk[4] + 0.2576 * mu_s;
    double* o = out + n * 5;
    o[0] = uicm;
    o[1] = uism;
    o[2] = uiconm;
    o[3] = uiqm;
    o[4] = uciqe;
  }
}

// ---------------------------------------------------------------------------
// Host orchestration
// ---------------------------------------------------------------------------

at::Tensor nr_metrics(const at::Tensor& rgb_u8) {
  TORCH_CHECK(rgb_u8.is_cuda() && rgb_u8.dtype() == at::kByte &&
              rgb_u8.dim() == 4 && rgb_u8.size(3) == 3,
              "nr_metrics: input must be (N,H,W,3) uint8 CUDA");
  const long N = rgb_u8.size(0), H = rgb_u8.size(1), W = rgb_u8.size(2);
  TORCH_CHECK(H >= 8 && W >= 8, "nr_metrics: image must be at least 8x8 "
              "(got ", H, "x", W, ")");
  // H, W and the block counts are ints in the kernels
  TORCH_CHECK(H * W < (1L << 31), "nr_metrics: image too large");
  auto out = at::empty({N, 5}, rgb_u8.options().dtype(at::kDouble));
  if (N == 0) return out;
  auto rgb = rgb_u8.contiguous();
  auto lab = rgb2lab_u8(rgb);
  const long HW = H * W;
  const int k1 = (int)(W / 8), k2 = (int)(H / 8);
  const long per_img = (long)k1 * k2, nblocks = N * per_img;
  const int nsplit = (int)std::max(1L, std::min(256L, HW / 16384));
  auto opts = rgb.options();
  auto hist = at::zeros({N, NR_BINS}, opts.dtype(at::kInt));
  auto partials = at::empty({N, nsplit, NR_PARTS}, opts.dtype(at::kDouble));
  auto terms = at::empty({nblocks, NR_TERMS}, opts.dtype(at::kDouble));
  hipStream_t stream = at::cuda::getCurrentHIPStream();
  hipLaunchKernelGGL(k_nr_hist, dim3(N, nsplit), dim3(NR_THREADS), 0, stream,
                     rgb.data_ptr<uint8_t>(), lab.data_ptr<uint8_t>(),
                     (unsigned int*)hist.data_ptr<int>(),
                     partials.data_ptr<double>(), HW, nsplit);
  const long waves_per_wg = NR_THREADS / WAVE;
  hipLaunchKernelGGL(k_nr_blocks,
                     dim3((nblocks + waves_per_wg - 1) / waves_per_wg),
                     dim3(NR_THREADS), 0, stream, rgb.data_ptr<uint8_t>(),
                     terms.data_ptr<double>(), (int)H, (int)W, k1, k2,
                     nblocks);
  hipLaunchKernelGGL(k_nr_finalize, dim3(N), dim3(FIN_THREADS), 0, stream,
                     (const unsigned int*)hist.data_ptr<int>(),
                     partials.data_ptr<double>(), terms.data_ptr<double>(),
                     out.data_ptr<double>(), HW, nsplit, per_img);
  HIP_CHECK_LAST();
  return out;
}
