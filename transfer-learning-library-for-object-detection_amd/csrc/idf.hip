// IDF (lib/IDF, methods/IDF) device ops: the domain attention map (DAM), the cross-branch
// modulation with the separation distance, and the per-image domain losses.
//
// The reference composes dam() from sigmoid / mean / mean / where (net_utils.py:300-306), the
// distance from two masked products, pairwise_distance and a mean, and the modulation from two
// more products (faster_rcnn.py:77-101): about ten passes over a 512-channel map forward and
// more backward, per level, branch pair and image.  Here a level is one DAM entry per branch
// (the map is read once), one separation forward (a and b are read once; d, dist and both
// modulated maps come out of it) and one separation backward.
//
// Launch shape: the conv4 / conv5 maps of a 600x1200 image have 11,250 / 2,775 pixels, fewer
// than the chip has lanes, so a thread per pixel with a serial channel loop would leave most
// SIMDs empty.  A workgroup is 16 waves over 64 consecutive pixels: lane = pixel (W-contiguous,
// one 256-B segment per wave load), wave = channel slice c = wave, wave + 16, ...; the 16
// partials of a pixel meet in LDS and are added in wave order, then the 64 pixels of the
// workgroup in a fixed shuffle tree, then the workgroups' partials (workspace) in index order
// by a second small launch.  No atomics: results are bit-identical from run to run.
//
// Arithmetic: the sigmoid is evaluated in double from the fp32 value, as us_daf.hip does; the
// channel mean stays in double and is rounded to fp32 once (avg), the threshold is the fp32
// rounding of the double mean of those fp32 avg, and the compare is fp32 against fp32 as in
// the reference.  The distance and its backward are evaluated in double from the fp32 inputs
// and rounded once; the modulation a (1 + att) is fp32 (one add, one multiply, no contraction),
// bit for bit the torch composition.
#include <algorithm>

#include "common.h"
#include "tlod_idf.h"

namespace tlod {
namespace {

constexpr int kWaves = 16;              // channel slices of a workgroup
constexpr int kThreads = 64 * kWaves;   // 64 pixels x 16 slices
constexpr int kRed = 256;               // the small reduction / threshold launches
constexpr double kEps = 1e-6;           // pairwise_distance's eps

// Lane 0 gets the sum of the wave's 64 values, added in a fixed tree.
__device__ __forceinline__ double wave_sum(double v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o);
  return v;
}

// The kWaves channel-slice partials of each pixel, added in wave order; valid in wave 0.
__device__ __forceinline__ double combine_slices(double v, double (*sh)[64]) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  sh[wave][lane] = v;
  __syncthreads();
  double s = 0.0;
  if (wave == 0)
    for (int w = 0; w < kWaves; ++w) s += sh[w][lane];
  return s;
}

// Sum of n doubles by a kRed-thread workgroup in a fixed order (every thread gets it).
__device__ __forceinline__ double block_sum_of(const double* __restrict__ p, int n, double* sh) {
  double v = 0.0;
  for (int i = threadIdx.x; i < n; i += kRed) v += p[i];
  v = wave_sum(v);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  double s = 0.0;
  for (int w = 0; w < kRed / 64; ++w) s += sh[w];
  return s;
}

// grid (ceil(P / 64), N).  att <- avg (fp32); part[n, block] = sum of the block's avg.
__global__ void __launch_bounds__(kThreads)
dam_avg_kernel(const float* __restrict__ x, int C, int P, float* __restrict__ att,
               double* __restrict__ part) {
  __shared__ double sh[kWaves][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, n = blockIdx.y;
  const int p = blockIdx.x * 64 + lane;
  const bool ok = p < P;
  double s = 0.0;
  if (ok) {
    const float* xp = x + (size_t)n * C * P + p;
#pragma unroll 4
    for (int c = wave; c < C; c += kWaves) s += 1.0 / (1.0 + exp(-(double)xp[(size_t)c * P]));
  }
  s = combine_slices(s, sh);
  if (wave == 0) {
    const float avg = ok ? (float)(s / (double)C) : 0.f;
    if (ok) att[(size_t)n * P + p] = avg;
    const double t = wave_sum((double)avg);
    if (lane == 0) part[(size_t)n * gridDim.x + blockIdx.x] = t;
  }
}

// grid (ceil(P / kRed), N).  att <- avg < thr ? 0 : avg with thr = mean of the image's avg.
__global__ void __launch_bounds__(kRed)
dam_threshold_kernel(const double* __restrict__ part, int nblk, int P, float* __restrict__ att) {
  __shared__ double sh[kRed / 64];
  const int n = blockIdx.y;
  const float thr = (float)(block_sum_of(part + (size_t)n * nblk, nblk, sh) / (double)P);
  const int p = blockIdx.x * kRed + threadIdx.x;
  if (p < P) {
    const float avg = att[(size_t)n * P + p];
    att[(size_t)n * P + p] = avg < thr ? 0.f : avg;
  }
}

// grid (ceil(P / 64), N).  MOD: also a_out = a (1 + att_b), b_out = b (1 + att_a).
template <bool MOD>
__global__ void __launch_bounds__(kThreads)
sep_fwd_kernel(const float* __restrict__ a, const float* __restrict__ b,
               const float* __restrict__ att_a, const float* __restrict__ att_b, int C, int P,
               float* __restrict__ a_out, float* __restrict__ b_out, float* __restrict__ d,
               double* __restrict__ part) {
  __shared__ double sh[kWaves][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, n = blockIdx.y;
  const int p = blockIdx.x * 64 + lane;
  const bool ok = p < P;
  double ss = 0.0;
  if (ok) {
    const size_t np = (size_t)n * P + p, base = (size_t)n * C * P + p;
    const double w = att_b ? (double)att_b[np] : 1.0;
    float ma = 0.f, mb = 0.f;
    if (MOD) {
      ma = 1.f + att_b[np];
      mb = 1.f + att_a[np];
    }
#pragma unroll 4
    for (int c = wave; c < C; c += kWaves) {
      const size_t i = base + (size_t)c * P;
      const float av = a[i], bv = b[i];
      const double e = ((double)av - (double)bv) * w + kEps;
      ss += e * e;
      if (MOD) {
        a_out[i] = av * ma;
        b_out[i] = bv * mb;
      }
    }
  }
  ss = combine_slices(ss, sh);
  if (wave == 0) {
    const double dd = ok ? sqrt(ss) : 0.0;
    if (ok) d[(size_t)n * P + p] = (float)dd;
    const double t = wave_sum(dd);
    if (lane == 0) part[(size_t)n * gridDim.x + blockIdx.x] = t;
  }
}

// grid N.  dist[n] = (sum of the image's block partials) / P.
__global__ void __launch_bounds__(kRed)
sep_mean_kernel(const double* __restrict__ part, int nblk, int P, float* __restrict__ dist) {
  __shared__ double sh[kRed / 64];
  const int n = blockIdx.x;
  const double s = block_sum_of(part + (size_t)n * nblk, nblk, sh);
  if (threadIdx.x == 0) dist[n] = (float)(s / (double)P);
}

// grid (ceil(P / 64), N), the forward's thread layout (no LDS: element-wise given d).
template <bool MOD>
__global__ void __launch_bounds__(kThreads)
sep_bwd_kernel(const float* __restrict__ a, const float* __restrict__ b,
               const float* __restrict__ att_a, const float* __restrict__ att_b,
               const float* __restrict__ d, const float* __restrict__ g_a_out,
               const float* __restrict__ g_b_out, const float* __restrict__ g_dist, int C, int P,
               float* __restrict__ g_a, float* __restrict__ g_b) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, n = blockIdx.y;
  const int p = blockIdx.x * 64 + lane;
  if (p >= P) return;
  const size_t np = (size_t)n * P + p, base = (size_t)n * C * P + p;
  const double w = att_b ? (double)att_b[np] : 1.0;
  const double dd = (double)d[np];
  // d ||e|| / d a = w e / ||e||; a zero weight gives exactly 0
  const double k = dd > 0.0 ? (double)g_dist[n] / (double)P * w / dd : 0.0;
  double ma = 0.0, mb = 0.0;
  if (MOD) {
    ma = 1.0 + (double)att_b[np];
    mb = 1.0 + (double)att_a[np];
  }
#pragma unroll 4
  for (int c = wave; c < C; c += kWaves) {
    const size_t i = base + (size_t)c * P;
    const double t = k * (((double)a[i] - (double)b[i]) * w + kEps);
    if (MOD) {
      g_a[i] = (float)((double)g_a_out[i] * ma + t);
      g_b[i] = (float)((double)g_b_out[i] * mb - t);
    } else {
      g_a[i] = (float)t;
      g_b[i] = (float)(-t);
    }
  }
}

// softmax[label] of a two-logit row, in double.
__device__ __forceinline__ double p_label(const float* __restrict__ z, int label) {
  const double zl = (double)z[label], zo = (double)z[1 - label];
  return 1.0 / (1.0 + exp(zo - zl));
}

// One workgroup.  loss[i < n_img] = CE(z_img[i], label_img); loss[n_img] = focal mean.
__global__ void __launch_bounds__(kRed)
domain_loss_fwd_kernel(const float* __restrict__ z_img, int n_img, int label_img,
                       const float* __restrict__ z_ins, int R, int label_ins, double gamma,
                       float* __restrict__ loss) {
  __shared__ double sh[kRed / 64];
  for (int i = threadIdx.x; i < n_img; i += kRed) {
    const double zl = (double)z_img[2 * i + label_img], zo = (double)z_img[2 * i + 1 - label_img];
    // logsumexp(z) - z[label] = log(1 + exp(zo - zl)), stable on both sides
    const double x = zo - zl;
    loss[i] = (float)(x > 0.0 ? x + log1p(exp(-x)) : log1p(exp(x)));
  }
  double v = 0.0;
  for (int r = threadIdx.x; r < R; r += kRed) {
    const double p = p_label(z_ins + 2 * (size_t)r, label_ins);
    const double P = (float)p < 1e-6f ? (double)1e-6f : p;  // clamp(1e-6, 1) of the fp32 softmax
    v += -pow(1.0 - P, gamma) * log(P);
  }
  v = wave_sum(v);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  if (threadIdx.x == 0) {
    double s = 0.0;
    for (int w = 0; w < kRed / 64; ++w) s += sh[w];
    loss[n_img] = (float)(s / (double)R);
  }
}

// One thread per row of z_img, then of z_ins.
__global__ void __launch_bounds__(kRed)
domain_loss_bwd_kernel(const float* __restrict__ z_img, int n_img, int label_img,
                       const float* __restrict__ z_ins, int R, int label_ins, double gamma,
                       const float* __restrict__ g_loss, float* __restrict__ dz_img,
                       float* __restrict__ dz_ins) {
  const int i = blockIdx.x * kRed + threadIdx.x;
  if (i < n_img) {
    const double p = p_label(z_img + 2 * (size_t)i, label_img);
    const double g = (double)g_loss[i] * (p - 1.0);  // softmax - onehot at the label
    dz_img[2 * i + label_img] = (float)g;
    dz_img[2 * i + 1 - label_img] = (float)(-g);
    return;
  }
  const int r = i - n_img;
  if (r >= R) return;
  const double p = p_label(z_ins + 2 * (size_t)r, label_ins);
  double g = 0.0;
  const double q = 1.0 - p;
  // q == 0 (the label leads by 37 or more): the gradient is below 1e-16 of g_loss / R and the
  // formula gives 0 for gamma >= 1; for gamma < 1 pow(0, gamma - 1) * log(1) would be inf * 0
  if (!((float)p < 1e-6f) && (q > 0.0 || gamma >= 1.0)) {
    // L = -(1 - P)^gamma log P; dL/dP = gamma (1 - P)^(gamma - 1) log P - (1 - P)^gamma / P
    const double dLdP = gamma * pow(q, gamma - 1.0) * log(p) - pow(q, gamma) / p;
    g = (double)g_loss[n_img] / (double)R * dLdP * p * q;  // dP / dz[label] = P (1 - P)
  }
  dz_ins[2 * (size_t)r + label_ins] = (float)g;
  dz_ins[2 * (size_t)r + 1 - label_ins] = (float)(-g);
}

int check_map(const char* fn, int N, int C, int H, int W) {
  if (!(N > 0 && C > 0 && H > 0 && W > 0 && N <= 65535 && (long long)H * W <= 0x7fffffffLL)) {
    set_error(std::string(fn) + ": bad shape");
    return kInvalidArg;
  }
  return kOk;
}

size_t partial_bytes(int N, int H, int W) {
  if (N <= 0 || H <= 0 || W <= 0) return 0;
  const long long P = (long long)H * W;
  return align_up((size_t)N * (size_t)((P + 63) / 64) * sizeof(double), 256);
}

}  // namespace
}  // namespace tlod

using namespace tlod;

extern "C" {

size_t tlod_idf_dam_workspace_bytes(int N, int H, int W) { return partial_bytes(N, H, W); }

int tlod_idf_dam_f32(const float* x, int N, int C, int H, int W, float* att, void* ws,
                     size_t ws_bytes, tlod_stream_t stream) {
  TLOD_CHECK_ARG(x && att, "null pointer");
  const int st = check_map(__func__, N, C, H, W);
  if (st != kOk) return st;
  if (!ws || ws_bytes < partial_bytes(N, H, W)) {
    set_error(std::string(__func__) + ": workspace too small");
    return kWorkspace;
  }
  const int P = H * W, nblk = div_up(P, 64);
  double* part = static_cast<double*>(ws);
  dam_avg_kernel<<<dim3(nblk, N), kThreads, 0, (hipStream_t)stream>>>(x, C, P, att, part);
  TLOD_LAUNCH_CHECK();
  dam_threshold_kernel<<<dim3(div_up(P, kRed), N), kRed, 0, (hipStream_t)stream>>>(part, nblk, P,
                                                                                  att);
  TLOD_LAUNCH_CHECK();
  return kOk;
}

size_t tlod_idf_sep_fwd_workspace_bytes(int N, int H, int W) { return partial_bytes(N, H, W); }

int tlod_idf_sep_fwd_f32(const float* a, const float* b, const float* att_a, const float* att_b,
                         int N, int C, int H, int W, float* a_out, float* b_out, float* d,
                         float* dist, void* ws, size_t ws_bytes, tlod_stream_t stream) {
  TLOD_CHECK_ARG(a && b && d && dist, "null pointer");
  TLOD_CHECK_ARG(!a_out == !b_out, "a_out and b_out: both or neither");
  TLOD_CHECK_ARG(!a_out || (att_a && att_b), "the modulation needs att_a and att_b");
  TLOD_CHECK_ARG(!a_out || (a_out != a && a_out != b && b_out != a && b_out != b &&
                            a_out != b_out), "a_out / b_out alias an input");
  const int st = check_map(__func__, N, C, H, W);
  if (st != kOk) return st;
  if (!ws || ws_bytes < partial_bytes(N, H, W)) {
    set_error(std::string(__func__) + ": workspace too small");
    return kWorkspace;
  }
  const int P = H * W, nblk = div_up(P, 64);
  double* part = static_cast<double*>(ws);
  const dim3 grid(nblk, N);
  if (a_out)
    sep_fwd_kernel<true><<<grid, kThreads, 0, (hipStream_t)stream>>>(a, b, att_a, att_b, C, P,
                                                                     a_out, b_out, d, part);
  else
    sep_fwd_kernel<false><<<grid, kThreads, 0, (hipStream_t)stream>>>(a, b, att_a, att_b, C, P,
                                                                      nullptr, nullptr, d, part);
  TLOD_LAUNCH_CHECK();
  sep_mean_kernel<<<N, kRed, 0, (hipStream_t)stream>>>(part, nblk, P, dist);
  TLOD_LAUNCH_CHECK();
  return kOk;
}

int tlod_idf_sep_bwd_f32(const float* a, const float* b, const float* att_a, const float* att_b,
                         const float* d, const float* g_a_out, const float* g_b_out,
                         const float* g_dist, int N, int C, int H, int W, float* g_a, float* g_b,
                         tlod_stream_t stream) {
  TLOD_CHECK_ARG(a && b && d && g_dist && g_a && g_b, "null pointer");
  TLOD_CHECK_ARG(!g_a_out == !g_b_out, "g_a_out and g_b_out: both or neither");
  TLOD_CHECK_ARG(!g_a_out || (att_a && att_b), "the modulation needs att_a and att_b");
  const int st = check_map(__func__, N, C, H, W);
  if (st != kOk) return st;
  const int P = H * W;
  const dim3 grid(div_up(P, 64), N);
  if (g_a_out)
    sep_bwd_kernel<true><<<grid, kThreads, 0, (hipStream_t)stream>>>(
        a, b, att_a, att_b, d, g_a_out, g_b_out, g_dist, C, P, g_a, g_b);
  else
    sep_bwd_kernel<false><<<grid, kThreads, 0, (hipStream_t)stream>>>(
        a, b, att_a, att_b, d, nullptr, nullptr, g_dist, C, P, g_a, g_b);
  TLOD_LAUNCH_CHECK();
  return kOk;
}

int tlod_idf_domain_loss_f32(const float* z_img, int n_img, int label_img, const float* z_ins,
                             int R, int label_ins, float gamma, float* loss,
                             tlod_stream_t stream) {
  TLOD_CHECK_ARG(z_ins && loss && (z_img || n_img == 0), "null pointer");
  TLOD_CHECK_ARG(n_img >= 0 && R > 0, "bad shape");
  TLOD_CHECK_ARG((label_img == 0 || label_img == 1) && (label_ins == 0 || label_ins == 1),
                 "labels are 0 or 1");
  TLOD_CHECK_ARG(gamma > 0.f, "gamma must be positive");
  domain_loss_fwd_kernel<<<1, kRed, 0, (hipStream_t)stream>>>(z_img, n_img, label_img, z_ins, R,
                                                              label_ins, (double)gamma, loss);
  TLOD_LAUNCH_CHECK();
  return kOk;
}

int tlod_idf_domain_loss_bwd_f32(const float* z_img, int n_img, int label_img,
                                 const float* z_ins, int R, int label_ins, float gamma,
                                 const float* g_loss, float* dz_img, float* dz_ins,
                                 tlod_stream_t stream) {
  TLOD_CHECK_ARG(z_ins && g_loss && dz_ins && ((z_img && dz_img) || n_img == 0), "null pointer");
  TLOD_CHECK_ARG(n_img >= 0 && R > 0, "bad shape");
  TLOD_CHECK_ARG((label_img == 0 || label_img == 1) && (label_ins == 0 || label_ins == 1),
                 "labels are 0 or 1");
  TLOD_CHECK_ARG(gamma > 0.f, "gamma must be positive");
  domain_loss_bwd_kernel<<<div_up(n_img + R, kRed), kRed, 0, (hipStream_t)stream>>>(
      z_img, n_img, label_img, z_ins, R, label_ins, (double)gamma, g_loss, dz_img, dz_ins);
  TLOD_LAUNCH_CHECK();
  return kOk;
}

}  // extern "C"
