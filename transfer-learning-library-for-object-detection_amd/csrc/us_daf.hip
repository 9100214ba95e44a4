// US-DAF (lib/US_DAF, methods/US_DAF) device ops: the RoI scale labels and the four domain
// losses of the scale-aware multi-label instance head and the one-channel image head.
//
// The reference builds the scale labels with two Python loops over the RoIs that read four
// device scalars per row (faster_rcnn.py:104-126, 207-231: ~2,200 host syncs per step for 256
// + 300 RoIs), then BCELoss / BCEloss_margin from a dozen torch temporaries (:25-33, 265-282).
// The tensors are a few thousand elements, so the cost is launches and host round trips: here
// the labels are one launch, and both domains' losses are one forward and one backward launch
// that compute the labels in place, read the upstream gradients from device memory and never
// synchronise with the host.
//
// Arithmetic: the sigmoid is evaluated in double from the fp32 logit and rounded once, so the
// saved s is the correctly rounded fp32 sigmoid (within 0.5 ulp of the exact value, whatever
// exp a reference uses); everything after it — the area, the logs, the element losses, the
// gate compare and the gradients — is fp32 from that s, as torch computes them from its own
// fp32 sigmoid.  Sums are accumulated in double in a fixed order by one workgroup per domain,
// so results are bit-identical from run to run.
#include <algorithm>

#include "common.h"
#include "tlod.h"

namespace tlod {
namespace {

constexpr int kRedThreads = 1024;
constexpr float kNear0 = 1e-10f;  // BCEloss_margin's NEAR_0

// Block-wide sum of NV doubles in a fixed order (every thread gets the totals).
template <int NV>
__device__ __forceinline__ void block_sum(double (&v)[NV], double* sh) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
#pragma unroll
  for (int k = 0; k < NV; ++k)
    for (int o = 32; o > 0; o >>= 1) v[k] += __shfl_down(v[k], o);
  if (lane == 0)
#pragma unroll
    for (int k = 0; k < NV; ++k) sh[wave * NV + k] = v[k];
  __syncthreads();
#pragma unroll
  for (int k = 0; k < NV; ++k) {
    double s = 0.0;
    for (int w = 0; w < nw; ++w) s += sh[w * NV + k];
    v[k] = s;
  }
  __syncthreads();
}

__device__ __forceinline__ float sigmoid_rn(float z) {
  return (float)(1.0 / (1.0 + exp(-(double)z)));
}

// faster_rcnn.py:108-119: area = (x2 - x1) * (y2 - y1) on the fp32 coordinates (no +1; two
// subtractions and one multiply, nothing to contract), area <= 400 small, 400 < area < 10000
// middle, area >= 10000 large.  A NaN area gets no label, as in the reference's if / elif.
struct ScaleLabel {
  float c[3];
  __device__ __forceinline__ explicit ScaleLabel(const float* __restrict__ roi) {
    const float area = (roi[3] - roi[1]) * (roi[4] - roi[2]);
    c[0] = area <= 400.f ? 1.f : 0.f;
    c[1] = (area > 400.f && area < 10000.f) ? 1.f : 0.f;
    c[2] = area >= 10000.f ? 1.f : 0.f;
  }
};

__global__ void __launch_bounds__(256)
roi_scale_labels_kernel(const float* __restrict__ rois, int R, float* __restrict__ labels) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= R) return;
  const ScaleLabel l(rois + 5 * (size_t)r);
  labels[3 * (size_t)r + 0] = l.c[0];
  labels[3 * (size_t)r + 1] = l.c[1];
  labels[3 * (size_t)r + 2] = l.c[2];
}

struct UsDomain {
  const float* z_img;    // forward: (npix) image logits
  const float* z_ins;    // forward: (n, 4) instance logits
  const float* rois;     // (n, 5)
  const float* gate_in;  // forward: (n) gates to use instead of the loss's own, or null
  float* s_img;          // (npix) sigmoid: written by the forward, read by the backward
  float* s_ins;          // (n, 4) likewise
  float* gate;           // (n) 0 / 1: written by the forward, read by the backward
  float* dz_img;         // backward
  float* dz_ins;
  long long npix;
  int n;
  float y;               // the domain label: 1 source, 0 target
};

struct UsArgs {
  UsDomain d[2];
};

// BCEloss_margin's element loss (faster_rcnn.py:28) from the saved sigmoid.
__device__ __forceinline__ float margin_elem(float s, float y) {
  return -(y * logf(s + kNear0) + (1.f - y) * logf(1.f - s + kNear0));
}

// One workgroup per domain: loss[2 * dom] = BCELoss of the image map against the domain
// label (mean over npix, logs clamped at -100), loss[2 * dom + 1] = BCEloss_margin of the
// (n, 4) instance outputs against [domain, small, middle, large] (mean over 4 n).
__global__ void __launch_bounds__(kRedThreads)
us_daf_loss_fwd_kernel(UsArgs a, float* __restrict__ loss) {
  __shared__ double sh[16];
  const UsDomain d = a.d[blockIdx.x];
  double v[1] = {0.0};
  for (long long p = threadIdx.x; p < d.npix; p += blockDim.x) {
    const float s = sigmoid_rn(d.z_img[p]);
    d.s_img[p] = s;
    const float ls = fmaxf(logf(s), -100.f), l1s = fmaxf(logf(1.f - s), -100.f);
    v[0] += (double)((d.y - 1.f) * l1s - d.y * ls);  // torch binary_cross_entropy
  }
  block_sum<1>(v, sh);
  double w[1] = {0.0};
  for (int r = threadIdx.x; r < d.n; r += blockDim.x) {
    const ScaleLabel l(d.rois + 5 * (size_t)r);
    const float* z = d.z_ins + 4 * (size_t)r;
    float* s = d.s_ins + 4 * (size_t)r;
    float e[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      s[c] = sigmoid_rn(z[c]);
      e[c] = margin_elem(s[c], c == 0 ? d.y : l.c[c - 1]);
    }
    const float g = d.gate_in ? d.gate_in[r] : (e[0] > 0.5f ? 1.f : 0.f);
    d.gate[r] = g;
    w[0] += (double)(e[0] * g) + (double)e[1] + (double)e[2] + (double)e[3];
  }
  block_sum<1>(w, sh);
  if (threadIdx.x == 0) {
    loss[2 * blockIdx.x + 0] = (float)(v[0] / (double)d.npix);
    loss[2 * blockIdx.x + 1] = (float)(w[0] / (4.0 * (double)(d.n > 0 ? d.n : 1)));
  }
}

// grid.y = domain; gloss in the forward's loss layout.  Image: BCELoss's backward
// (p - y) / max(p (1 - p), 1e-12) times the sigmoid's p (1 - p): 0 at saturation.  Instance:
// the element loss's derivative in s times s (1 - s), times the gate in column 0.
__global__ void __launch_bounds__(256)
us_daf_loss_bwd_kernel(UsArgs a, const float* __restrict__ gloss) {
  const int dom = blockIdx.y;
  const UsDomain d = a.d[dom];
  const float gi = gloss[2 * dom + 0] / (float)d.npix;
  const float gn = gloss[2 * dom + 1] / (4.f * (float)(d.n > 0 ? d.n : 1));
  const long long total = d.npix + 4LL * d.n;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total;
       i += (long long)gridDim.x * blockDim.x) {
    if (i < d.npix) {
      const float p = d.s_img[i];
      const float q = p * (1.f - p);
      d.dz_img[i] = gi * (p - d.y) * (q / fmaxf(q, 1e-12f));
    } else {
      const long long k = i - d.npix;
      const int r = (int)(k >> 2), c = (int)(k & 3);
      const float s = d.s_ins[k];
      float y = d.y, w = d.gate[r];
      if (c > 0) {
        const ScaleLabel l(d.rois + 5 * (size_t)r);
        y = c == 1 ? l.c[0] : (c == 2 ? l.c[1] : l.c[2]);  // selects: no indexed private array
        w = 1.f;
      }
      const float de = -(y / (s + kNear0) - (1.f - y) / (1.f - s + kNear0));
      d.dz_ins[k] = gn * w * de * (s * (1.f - s));
    }
  }
}

int us_args(const float* rois_s, const float* rois_t, int Bs, int Bt, int Hs, int Ws, int Ht,
            int Wt, int n_s, int n_t, float* s_img_s, float* s_img_t, float* s_ins_s,
            float* s_ins_t, float* gate_s, float* gate_t, UsArgs* a) {
  TLOD_CHECK_ARG(s_img_s && s_img_t, "null pointer");
  TLOD_CHECK_ARG((rois_s && s_ins_s && gate_s) || n_s == 0, "null source instance pointer");
  TLOD_CHECK_ARG((rois_t && s_ins_t && gate_t) || n_t == 0, "null target instance pointer");
  TLOD_CHECK_ARG(Bs > 0 && Bt > 0 && Hs > 0 && Ws > 0 && Ht > 0 && Wt > 0 && n_s >= 0 &&
                 n_t >= 0, "bad shape");
  a->d[0] = UsDomain{nullptr, nullptr, rois_s, nullptr, s_img_s, s_ins_s, gate_s, nullptr,
                     nullptr, (long long)Bs * Hs * Ws, n_s, 1.f};
  a->d[1] = UsDomain{nullptr, nullptr, rois_t, nullptr, s_img_t, s_ins_t, gate_t, nullptr,
                     nullptr, (long long)Bt * Ht * Wt, n_t, 0.f};
  return kOk;
}

}  // namespace
}  // namespace tlod

using namespace tlod;

extern "C" {

int tlod_roi_scale_labels_f32(const float* rois, int R, float* labels, tlod_stream_t stream) {
  TLOD_CHECK_ARG(rois && labels, "null pointer");
  TLOD_CHECK_ARG(R > 0, "bad shape");
  roi_scale_labels_kernel<<<div_up(R, 256), 256, 0, (hipStream_t)stream>>>(rois, R, labels);
  TLOD_LAUNCH_CHECK();
  return kOk;
}

int tlod_us_daf_loss_f32(const float* z_img_s, const float* z_img_t, const float* z_ins_s,
                         const float* z_ins_t, const float* rois_s, const float* rois_t,
                         const float* gate_in_s, const float* gate_in_t, int Bs, int Bt, int Hs,
                         int Ws, int Ht, int Wt, int n_s, int n_t, float* s_img_s,
                         float* s_img_t, float* s_ins_s, float* s_ins_t, float* gate_s,
                         float* gate_t, float* loss, tlod_stream_t stream) {
  TLOD_CHECK_ARG(z_img_s && z_img_t && loss, "null pointer");
  TLOD_CHECK_ARG((z_ins_s || n_s == 0) && (z_ins_t || n_t == 0), "null instance logits");
  TLOD_CHECK_ARG(!gate_in_s == !gate_in_t, "gate override: both domains or neither");
  UsArgs a;
  const int st = us_args(rois_s, rois_t, Bs, Bt, Hs, Ws, Ht, Wt, n_s, n_t, s_img_s, s_img_t,
                         s_ins_s, s_ins_t, gate_s, gate_t, &a);
  if (st != kOk) return st;
  a.d[0].z_img = z_img_s;
  a.d[0].z_ins = z_ins_s;
  a.d[0].gate_in = gate_in_s;
  a.d[1].z_img = z_img_t;
  a.d[1].z_ins = z_ins_t;
  a.d[1].gate_in = gate_in_t;
  us_daf_loss_fwd_kernel<<<2, kRedThreads, 0, (hipStream_t)stream>>>(a, loss);
  TLOD_LAUNCH_CHECK();
  return kOk;
}

int tlod_us_daf_loss_bwd_f32(const float* s_img_s, const float* s_img_t, const float* s_ins_s,
                             const float* s_ins_t, const float* rois_s, const float* rois_t,
                             const float* gate_s, const float* gate_t, int Bs, int Bt, int Hs,
                             int Ws, int Ht, int Wt, int n_s, int n_t, const float* grad_loss,
                             float* dz_img_s, float* dz_img_t, float* dz_ins_s, float* dz_ins_t,
                             tlod_stream_t stream) {
  TLOD_CHECK_ARG(grad_loss && dz_img_s && dz_img_t && (dz_ins_s || n_s == 0) &&
                 (dz_ins_t || n_t == 0), "null pointer");
  UsArgs a;
  const int st = us_args(rois_s, rois_t, Bs, Bt, Hs, Ws, Ht, Wt, n_s, n_t,
                         const_cast<float*>(s_img_s), const_cast<float*>(s_img_t),
                         const_cast<float*>(s_ins_s), const_cast<float*>(s_ins_t),
                         const_cast<float*>(gate_s), const_cast<float*>(gate_t), &a);
  if (st != kOk) return st;
  a.d[0].dz_img = dz_img_s;
  a.d[0].dz_ins = dz_ins_s;
  a.d[1].dz_img = dz_img_t;
  a.d[1].dz_ins = dz_ins_t;
  const long long n = std::max(a.d[0].npix + 4LL * n_s, a.d[1].npix + 4LL * n_t);
  const long long g = (n + 255) / 256;
  dim3 grid((unsigned)(g > 1024 ? 1024 : g), 2);
  us_daf_loss_bwd_kernel<<<grid, 256, 0, (hipStream_t)stream>>>(a, grad_loss);
  TLOD_LAUNCH_CHECK();
  return kOk;
}

}  // extern "C"
