// PA-ATF (lib/PA_ATF, methods/PA_ATF) device ops: the strided convolution's im2col / col2im
// around the split-bf16 GEMM, the gated image discriminator's channel gate, and the prototype
// pooling that feeds CLUB.
//
// Strided convolution.  The mask net of _ImageDA starts with a 5x5 stride-3 conv and a 3x3
// stride-2 conv at full channel width (faster_rcnn.py:68-103), CLUB with a 3x3 stride-2 conv
// (:105-147).  col[(n, ho, wo)][(c, kh, kw)] is the nn.Conv2d weight's own column order, so
// the (Cout, Cin KS^2) weight is a GEMM operand as it is (tlod_gemm_bs_ex_f32: bias and ReLU
// in the epilogue).  im2col: a workgroup is 256 consecutive columns of one output pixel, so
// the stores are one contiguous 1-KiB run and the pixel's (n, ho, wo) is workgroup-uniform;
// the loads are KS-long runs of x that the caches serve (each x cell is read about
// (KS / stride)^2 times).  col2im is the adjoint as a gather: a thread per input cell adds its
// <= ceil(KS / stride)^2 taps in (kh, kw) order, so there are no atomics, every cell is written
// (0 where no window covers it) and the sum has one order.
//
// Channel gate: mask = sigmoid(adaptive_max_pool2d(z, 1)).  A plane of the mask net's output is
// at most a few hundred cells and there are N C <= 1024 of them: one wave per plane, lanes
// strided over the cells, (value, index) pairs meeting in a fixed shuffle tree under torch's
// rule (first maximum in row-major order; a NaN wins, the last one).  The sigmoid is evaluated
// in double from the fp32 maximum and rounded once, as us_daf.hip and idf.hip do.
//
// Prototype pooling: RoI max pooling (roi.hip's roi_pool_fwd_kernel, bit for bit) of the G
// source gt boxes on one level's map, times the level's channel mask and its complement, with
// CLUB's shuffled pairing: one launch writes both 2C-channel inputs of CLUB.  The backward is a
// gather over feature cells (gt boxes overlap, a scatter would need atomics): a cell visits
// the RoIs in index order, and of a RoI only the <= 2 x 2 bins whose window holds the cell, in
// bin order; double accumulation, one rounding, CLUB's gradient reversal folded in.
//
// Losses: the 14 scalar terms of a step (six image BCEs from the logits, two instance L1 terms
// in the reference's (R, R)-broadcast form, six two-logit cross entropies) are one launch of 14
// workgroups forward (a term is a thread-strided double sum, a fixed shuffle tree and the four
// waves in order) and one element-wise launch backward, through pointer tables passed by
// value.  (The target's subsampled proposal layer of the same header lives in proposal.hip,
// beside the decode / sort / NMS it reuses.)
#include <algorithm>
#include <cfloat>
#include <climits>

#include "common.h"
#include "tlod_pa_atf.h"

namespace tlod {
namespace {

constexpr int kThreads = 256;
constexpr int kBins = 7;  // _RoIPooling(7, 7, scale)

// ------------------------------------------------------------------ im2col / col2im
struct ConvGeo {
  int N, C, H, W, KS, stride, pad, Ho, Wo, K;
};

// grid (N Ho Wo, ceil(K / 256)).
__global__ void __launch_bounds__(kThreads)
im2col_kernel(const float* __restrict__ x, ConvGeo g, float* __restrict__ col) {
  const int row = blockIdx.x;
  const int k = blockIdx.y * kThreads + threadIdx.x;
  if (k >= g.K) return;
  const int wo = row % g.Wo, ho = (row / g.Wo) % g.Ho, n = row / (g.Wo * g.Ho);
  const int kw = k % g.KS, kh = (k / g.KS) % g.KS, c = k / (g.KS * g.KS);
  const int h = ho * g.stride + kh - g.pad, w = wo * g.stride + kw - g.pad;
  float v = 0.f;
  if (h >= 0 && h < g.H && w >= 0 && w < g.W)
    v = x[(((size_t)n * g.C + c) * g.H + h) * g.W + w];
  col[(size_t)row * g.K + k] = v;
}

// One thread per input cell, W-contiguous.
__global__ void __launch_bounds__(kThreads)
col2im_kernel(const float* __restrict__ dcol, ConvGeo g, size_t total, float* __restrict__ dx) {
  const size_t idx = (size_t)blockIdx.x * kThreads + threadIdx.x;
  if (idx >= total) return;
  const int w = (int)(idx % g.W), h = (int)((idx / g.W) % g.H);
  const int c = (int)((idx / ((size_t)g.W * g.H)) % g.C);
  const int n = (int)(idx / ((size_t)g.W * g.H * g.C));
  float acc = 0.f;
  for (int kh = 0; kh < g.KS; ++kh) {
    const int th = h + g.pad - kh;
    if (th < 0) break;
    if (th % g.stride) continue;
    const int ho = th / g.stride;
    if (ho >= g.Ho) continue;
    for (int kw = 0; kw < g.KS; ++kw) {
      const int tw = w + g.pad - kw;
      if (tw < 0) break;
      if (tw % g.stride) continue;
      const int wo = tw / g.stride;
      if (wo >= g.Wo) continue;
      acc += dcol[(((size_t)n * g.Ho + ho) * g.Wo + wo) * g.K + (c * g.KS + kh) * g.KS + kw];
    }
  }
  dx[idx] = acc;
}

int conv_geo(const char* fn, int N, int C, int H, int W, int KS, int stride, int pad,
             ConvGeo* g) {
  const bool ok = N > 0 && C > 0 && H > 0 && W > 0 && KS >= 1 && stride >= 1 && pad >= 0 &&
                  H + 2 * pad >= KS && W + 2 * pad >= KS;
  if (!ok) {
    set_error(std::string(fn) + ": bad shape (KS >= 1, stride >= 1, pad >= 0, an output of "
                                "at least 1 x 1)");
    return kInvalidArg;
  }
  const int Ho = (H + 2 * pad - KS) / stride + 1, Wo = (W + 2 * pad - KS) / stride + 1;
  const long long rows = (long long)N * Ho * Wo, K = (long long)C * KS * KS;
  const long long cells = (long long)N * C * H * W;
  if (rows > 0x7fffffffLL || K > 65535LL * kThreads || cells / kThreads >= 0x7fffffffLL) {
    set_error(std::string(fn) + ": shape too large");
    return kInvalidArg;
  }
  *g = ConvGeo{N, C, H, W, KS, stride, pad, Ho, Wo, (int)K};
  return kOk;
}

// ------------------------------------------------------------------ channel gate
// (v1, i1) before (v2, i2) under adaptive_max_pool2d's scan (val > max || isnan(val) takes
// over): the larger value and of equal values the smaller index; a NaN wins, and of several
// NaNs the last one.
__device__ __forceinline__ bool before(float v1, int i1, float v2, int i2) {
  const bool n1 = v1 != v1, n2 = v2 != v2;
  if (n1 || n2) return (n1 && n2) ? i1 > i2 : n1;
  if (v1 > v2) return true;
  if (v1 < v2) return false;
  return i1 < i2;
}

// A wave per (n, c) plane of P cells; 4 planes per workgroup.
__global__ void __launch_bounds__(kThreads)
gate_fwd_kernel(const float* __restrict__ z, int planes, int P, float* __restrict__ mask,
                int32_t* __restrict__ arg) {
  const int lane = threadIdx.x & 63;
  const int plane = blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6);
  if (plane >= planes) return;  // wave-uniform
  const float* zp = z + (size_t)plane * P;
  float v = -INFINITY;
  int i = INT_MAX;
  for (int p = lane; p < P; p += 64) {
    const float t = zp[p];
    if (before(t, p, v, i)) { v = t; i = p; }
  }
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_down(v, o);
    const int oi = __shfl_down(i, o);
    if (before(ov, oi, v, i)) { v = ov; i = oi; }
  }
  if (lane == 0) {
    mask[plane] = (float)(1.0 / (1.0 + exp(-(double)v)));
    arg[plane] = i;
  }
}

// One thread per cell of dz.  sigmoid's backward as torch states it: (g (1 - m)) m in fp32.
__global__ void __launch_bounds__(kThreads)
gate_bwd_kernel(const float* __restrict__ dmask, const float* __restrict__ mask,
                const int32_t* __restrict__ arg, int P, size_t total, float* __restrict__ dz) {
  const size_t idx = (size_t)blockIdx.x * kThreads + threadIdx.x;
  if (idx >= total) return;
  const size_t plane = idx / P;
  const int p = (int)(idx - plane * P);
  float g = 0.f;
  if (p == arg[plane]) {
    const float m = mask[plane];
    g = dmask[plane] * (1.f - m) * m;
  }
  dz[idx] = g;
}

// ------------------------------------------------------------------ prototype pooling
struct Box {
  int sw, sh, rw, rh;
};

// roi_pool_fwd_kernel's box arithmetic (roi.hip).
__device__ __forceinline__ Box scaled_box(const float* __restrict__ r, float scale) {
  const int sw = (int)round(r[1] * scale), sh = (int)round(r[2] * scale);
  const int ew = (int)round(r[3] * scale), eh = (int)round(r[4] * scale);
  return Box{sw, sh, max(ew - sw + 1, 1), max(eh - sh + 1, 1)};
}

__device__ __forceinline__ void bin_range(int b, int size, int start, int limit, int* lo,
                                          int* hi) {
  const float bs = (float)size / (float)kBins;
  const int s = (int)floorf((float)b * bs), e = (int)ceilf((float)(b + 1) * bs);
  *lo = min(max(s + start, 0), limit);
  *hi = min(max(e + start, 0), limit);
}

// Max of channel c over bin (ph, pw) of a box; 0 and index -1 when the bin is empty.
__device__ __forceinline__ float pool_bin(const float* __restrict__ feat, int c, int H, int W,
                                          const Box& b, int ph, int pw, int* idx) {
  int hs, he, ws, we;
  bin_range(ph, b.rh, b.sh, H, &hs, &he);
  bin_range(pw, b.rw, b.sw, W, &ws, &we);
  const bool empty = (he <= hs) || (we <= ws);
  float maxval = empty ? 0.f : -FLT_MAX;
  int maxidx = -1;
  const size_t off = (size_t)c * H * W;
  for (int h = hs; h < he; ++h)
    for (int w = ws; w < we; ++w) {
      const float v = feat[off + h * W + w];
      if (v > maxval) { maxval = v; maxidx = (int)(off + h * W + w); }
    }
  *idx = maxidx;
  return maxval;
}

// One thread per (g, c, ph, pw).
__global__ void __launch_bounds__(kThreads)
proto_fwd_kernel(const float* __restrict__ feat, int C, int H, int W,
                 const float* __restrict__ rois, int G, float scale,
                 const float* __restrict__ mask, const int32_t* __restrict__ perm,
                 float* __restrict__ same, float* __restrict__ diff,
                 int32_t* __restrict__ argmax) {
  const int index = blockIdx.x * kThreads + threadIdx.x;
  if (index >= G * C * kBins * kBins) return;
  const int pw = index % kBins, ph = (index / kBins) % kBins;
  const int c = (index / (kBins * kBins)) % C, g = index / (kBins * kBins * C);
  int idx, other;
  const float p = pool_bin(feat, c, H, W, scaled_box(rois + 5 * g, scale), ph, pw, &idx);
  const int pg = perm[g];
  float q = 0.f;  // a perm entry outside [0, G) pairs the RoI with zeros
  if (pg >= 0 && pg < G)
    q = pool_bin(feat, c, H, W, scaled_box(rois + 5 * pg, scale), ph, pw, &other);
  const float m = mask[c], cm = 1.f - m;
  const size_t bin = (size_t)ph * kBins + pw, plane = kBins * kBins;
  const size_t lo = ((size_t)g * 2 * C + c) * plane + bin, hi = lo + (size_t)C * plane;
  const float a = p * m;
  same[lo] = a;
  same[hi] = p * cm;
  diff[lo] = a;
  diff[hi] = q * cm;
  argmax[index] = idx;
}

// One thread per (c, h, w) cell of dfeat.
__global__ void __launch_bounds__(kThreads)
proto_bwd_kernel(const float* __restrict__ d_same, const float* __restrict__ d_diff,
                 const float* __restrict__ mask, const int32_t* __restrict__ perm,
                 const int32_t* __restrict__ argmax, const float* __restrict__ rois, int G,
                 float scale, int C, int H, int W, float alpha, float* __restrict__ dfeat) {
  const int cell = blockIdx.x * kThreads + threadIdx.x;
  if (cell >= C * H * W) return;
  const int w = cell % W, h = (cell / W) % H, c = cell / (W * H);
  const double m = (double)mask[c], cm = (double)(1.f - mask[c]);
  const size_t plane = kBins * kBins;
  double acc = 0.0;
  for (int g = 0; g < G; ++g) {
    const Box b = scaled_box(rois + 5 * g, scale);
    if (h < b.sh || h >= b.sh + b.rh + 1 || w < b.sw || w >= b.sw + b.rw + 1) continue;
    for (int ph = 0; ph < kBins; ++ph) {
      int hs, he;
      bin_range(ph, b.rh, b.sh, H, &hs, &he);
      if (h < hs || h >= he) continue;
      for (int pw = 0; pw < kBins; ++pw) {
        int ws, we;
        bin_range(pw, b.rw, b.sw, W, &ws, &we);
        if (w < ws || w >= we) continue;
        const size_t bin = (size_t)ph * kBins + pw;
        if (argmax[((size_t)g * C + c) * plane + bin] != cell) continue;
        const size_t lo = ((size_t)g * 2 * C + c) * plane + bin, hi = lo + (size_t)C * plane;
        double t = m * ((double)d_same[lo] + (double)d_diff[lo]) + cm * (double)d_same[hi];
        for (int g2 = 0; g2 < G; ++g2)  // the RoIs this one was paired to as the partner
          if (perm[g2] == g)
            t += cm * (double)d_diff[((size_t)g2 * 2 * C + C + c) * plane + bin];
        acc += t;
      }
    }
  }
  dfeat[cell] = (float)(-(double)alpha * acc);
}

int check_proto(const char* fn, int C, int H, int W, int G) {
  if (!(C > 0 && H > 0 && W > 0 && G > 0) || (long long)C * H * W > 0x7fffffffLL ||
      (long long)G * 2 * C * kBins * kBins > 0x7fffffffLL) {
    set_error(std::string(fn) + ": bad shape");
    return kInvalidArg;
  }
  return kOk;
}

// ------------------------------------------------------------------ the 14 loss terms
// Terms 0..5: image BCEs; 6, 7: instance L1 terms; 8..13: CLUB's two-logit cross entropies.
constexpr int kTerms = TLOD_PA_ATF_TERMS;
constexpr int kImg = 6, kIns = 2;

struct LossArgs {
  const float* z[kTerms];
  float* dz[kTerms];
  int n[kTerms];      // image: cells; instance: R rows; CLUB: G rows of two logits
  int label[kTerms];  // image / CLUB: 0 or 1; instance: the number of ones among the R labels
};

__device__ __forceinline__ double softplus(double x) {
  return x > 0.0 ? x + log1p(exp(-x)) : log1p(exp(x));
}

// One workgroup per term; the sum runs thread-strided, then a fixed shuffle tree, then the four
// waves in order.
__global__ void __launch_bounds__(kThreads)
loss_fwd_kernel(LossArgs a, float* __restrict__ loss) {
  __shared__ double sh[kThreads / 64];
  const int t = blockIdx.x, n = a.n[t], label = a.label[t];
  const float* __restrict__ z = a.z[t];
  double v = 0.0;
  if (t < kImg) {
    // BCELoss(sigmoid(z), label) with its log clamp at -100: -log p = softplus(-z)
    for (int i = threadIdx.x; i < n; i += kThreads) {
      const double x = (double)z[i];
      v += fmin(softplus(label ? -x : x), 100.0);
    }
  } else if (t < kImg + kIns) {
    // mean_j |x_i - l_j| over `label` ones and n - label zeros, x = sigmoid(z) in [0, 1]
    const double ones = (double)label, zeros = (double)(n - label);
    for (int i = threadIdx.x; i < n; i += kThreads) {
      const double x = 1.0 / (1.0 + exp(-(double)z[i]));
      v += (ones * (1.0 - x) + zeros * x) / (double)n;
    }
  } else {
    for (int i = threadIdx.x; i < n; i += kThreads)
      v += softplus((double)z[2 * i + 1 - label] - (double)z[2 * i + label]);
  }
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  if (threadIdx.x == 0) {
    double s = 0.0;
    for (int w = 0; w < kThreads / 64; ++w) s += sh[w];
    loss[t] = (float)(s / (double)n);
  }
}

// grid (ceil(max n / 256), 14): one thread per logit (per row of two for CLUB).
__global__ void __launch_bounds__(kThreads)
loss_bwd_kernel(LossArgs a, const float* __restrict__ g_loss) {
  const int t = blockIdx.y, n = a.n[t], label = a.label[t];
  const int i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= n) return;
  const float* __restrict__ z = a.z[t];
  float* __restrict__ dz = a.dz[t];
  const double g = (double)g_loss[t] / (double)n;
  if (t < kImg) {
    const double x = (double)z[i], u = label ? -x : x;  // d softplus(u) / du = sigmoid(u)
    const double d = softplus(u) < 100.0 ? 1.0 / (1.0 + exp(-u)) : 0.0;
    dz[i] = (float)(g * (label ? -d : d));
  } else if (t < kImg + kIns) {
    const double x = 1.0 / (1.0 + exp(-(double)z[i]));
    dz[i] = (float)(g * (double)(n - 2 * label) / (double)n * x * (1.0 - x));
  } else {
    const double zl = (double)z[2 * i + label], zo = (double)z[2 * i + 1 - label];
    const double d = g * (1.0 / (1.0 + exp(zo - zl)) - 1.0);  // softmax - onehot at the label
    dz[2 * i + label] = (float)d;
    dz[2 * i + 1 - label] = (float)(-d);
  }
}

int loss_args(const char* fn, const float* const* z, const int* n, const int* label,
              float* const* dz, LossArgs* a) {
  if (!z || !n || !label) {
    set_error(std::string(fn) + ": null table");
    return kInvalidArg;
  }
  for (int t = 0; t < kTerms; ++t) {
    const bool ins = t >= kImg && t < kImg + kIns;
    if (!z[t] || (dz && !dz[t]) || n[t] < 1 || n[t] > (1 << 30) || label[t] < 0 ||
        label[t] > (ins ? n[t] : 1)) {
      set_error(std::string(fn) + ": term " + std::to_string(t) +
                ": null pointer, n < 1 or a label outside its range");
      return kInvalidArg;
    }
    a->z[t] = z[t];
    a->dz[t] = dz ? dz[t] : nullptr;
    a->n[t] = n[t];
    a->label[t] = label[t];
  }
  return kOk;
}

}  // namespace
}  // namespace tlod

using namespace tlod;

extern "C" {

int tlod_im2col_f32(const float* x, int N, int C, int H, int W, int KS, int stride, int pad,
                    float* col, tlod_stream_t stream) {
  TLOD_CHECK_ARG(x && col, "null pointer");
  ConvGeo g;
  const int st = conv_geo(__func__, N, C, H, W, KS, stride, pad, &g);
  if (st != kOk) return st;
  im2col_kernel<<<dim3(N * g.Ho * g.Wo, div_up(g.K, kThreads)), kThreads, 0,
                  (hipStream_t)stream>>>(x, g, col);
  TLOD_LAUNCH_CHECK();
  return kOk;
}

int tlod_col2im_f32(const float* dcol, int N, int C, int H, int W, int KS, int stride, int pad,
                    float* dx, tlod_stream_t stream) {
  TLOD_CHECK_ARG(dcol && dx, "null pointer");
  ConvGeo g;
  const int st = conv_geo(__func__, N, C, H, W, KS, stride, pad, &g);
  if (st != kOk) return st;
  const size_t total = (size_t)N * C * H * W;
  col2im_kernel<<<(unsigned)((total + kThreads - 1) / kThreads), kThreads, 0,
                  (hipStream_t)stream>>>(dcol, g, total, dx);
  TLOD_LAUNCH_CHECK();
  return kOk;
}

int tlod_pa_gate_f32(const float* z, int N, int C, int h, int w, float* mask, int32_t* arg,
                     tlod_stream_t stream) {
  TLOD_CHECK_ARG(z && mask && arg, "null pointer");
  TLOD_CHECK_ARG(N > 0 && C > 0 && h > 0 && w > 0 && (long long)N * C <= 0x7fffffffLL &&
                 (long long)h * w < 0x7fffffffLL, "bad shape");
  const int planes = N * C;
  gate_fwd_kernel<<<div_up(planes, kThreads / 64), kThreads, 0, (hipStream_t)stream>>>(
      z, planes, h * w, mask, arg);
  TLOD_LAUNCH_CHECK();
  return kOk;
}

int tlod_pa_gate_bwd_f32(const float* dmask, const float* mask, const int32_t* arg, int N, int C,
                         int h, int w, float* dz, tlod_stream_t stream) {
  TLOD_CHECK_ARG(dmask && mask && arg && dz, "null pointer");
  TLOD_CHECK_ARG(N > 0 && C > 0 && h > 0 && w > 0 && (long long)N * C <= 0x7fffffffLL &&
                 (long long)h * w < 0x7fffffffLL, "bad shape");
  const size_t total = (size_t)N * C * h * w;
  TLOD_CHECK_ARG(total / kThreads < 0x7fffffffULL, "shape too large");
  gate_bwd_kernel<<<(unsigned)((total + kThreads - 1) / kThreads), kThreads, 0,
                    (hipStream_t)stream>>>(dmask, mask, arg, h * w, total, dz);
  TLOD_LAUNCH_CHECK();
  return kOk;
}

int tlod_pa_proto_pool_fwd_f32(const float* feat, int C, int H, int W, const float* rois, int G,
                               float scale, const float* mask, const int32_t* perm, float* same,
                               float* diff, int32_t* argmax, tlod_stream_t stream) {
  TLOD_CHECK_ARG(feat && rois && mask && perm && same && diff && argmax, "null pointer");
  const int st = check_proto(__func__, C, H, W, G);
  if (st != kOk) return st;
  proto_fwd_kernel<<<div_up(G * C * kBins * kBins, kThreads), kThreads, 0,
                     (hipStream_t)stream>>>(feat, C, H, W, rois, G, scale, mask, perm, same,
                                            diff, argmax);
  TLOD_LAUNCH_CHECK();
  return kOk;
}

int tlod_pa_proto_pool_bwd_f32(const float* d_same, const float* d_diff, const float* mask,
                               const int32_t* perm, const int32_t* argmax, const float* rois,
                               int G, float scale, int C, int H, int W, float alpha,
                               float* dfeat, tlod_stream_t stream) {
  TLOD_CHECK_ARG(d_same && d_diff && mask && perm && argmax && rois && dfeat, "null pointer");
  const int st = check_proto(__func__, C, H, W, G);
  if (st != kOk) return st;
  proto_bwd_kernel<<<div_up(C * H * W, kThreads), kThreads, 0, (hipStream_t)stream>>>(
      d_same, d_diff, mask, perm, argmax, rois, G, scale, C, H, W, alpha, dfeat);
  TLOD_LAUNCH_CHECK();
  return kOk;
}

int tlod_pa_atf_loss_f32(const float* const* z, const int* n, const int* label, float* loss,
                         tlod_stream_t stream) {
  TLOD_CHECK_ARG(loss, "null pointer");
  LossArgs a;
  const int st = loss_args(__func__, z, n, label, nullptr, &a);
  if (st != kOk) return st;
  loss_fwd_kernel<<<kTerms, kThreads, 0, (hipStream_t)stream>>>(a, loss);
  TLOD_LAUNCH_CHECK();
  return kOk;
}

int tlod_pa_atf_loss_bwd_f32(const float* const* z, const int* n, const int* label,
                             const float* g_loss, float* const* dz, tlod_stream_t stream) {
  TLOD_CHECK_ARG(g_loss && dz, "null pointer");
  LossArgs a;
  const int st = loss_args(__func__, z, n, label, dz, &a);
  if (st != kOk) return st;
  for (int t = 0; t < kTerms; ++t)
    for (int u = 0; u < t; ++u) TLOD_CHECK_ARG(dz[t] != dz[u], "the gradient buffers repeat");
  int most = 0;
  for (int t = 0; t < kTerms; ++t) most = std::max(most, a.n[t]);
  loss_bwd_kernel<<<dim3(div_up(most, kThreads), kTerms), kThreads, 0, (hipStream_t)stream>>>(
      a, g_loss);
  TLOD_LAUNCH_CHECK();
  return kOk;
}

}  // extern "C"
