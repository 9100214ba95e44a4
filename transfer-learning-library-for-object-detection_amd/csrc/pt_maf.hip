// PT-MAF (lib/PT_MAF, methods/PT_MAF) device ops: the RPN foreground / background maps,
// the masked two-way NLL of the six image discriminators, the temperature KL of the
// distillation loss and the ground-truth cell mask.
//
// The reference builds these from a dozen torch.where / full_like maps, softmax / log / "/"
// temporaries and a host double loop over feature cells behind a .item() per step
// (faster_rcnn.py:132-148, 290-398; PT_MAF_train.py:444-456; faster_rcnn_kd.py:58-65).  The
// maps are a few thousand cells, so the cost is launches and the host round trip, not
// bandwidth: every op here is one launch, reads its scalars (counts, upstream gradients,
// num_boxes) from device memory and never synchronises with the host.  Element arithmetic is
// fp32 (the KD row terms, a cancellation, are double: see kl_row); sums are accumulated in
// double in a fixed order by one workgroup per reduction (as in losses.hip) and cell counts in
// integers, so results are bit-identical from run to run.
#include "common.h"
#include "tlod.h"

namespace tlod {
namespace {

constexpr int kRedThreads = 1024;
constexpr int kMaxPairs = 8;

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

// 2-way log_softmax in torch's form (losses.hip).
struct LogSoftmax2 {
  float l0, l1;
  __device__ __forceinline__ LogSoftmax2(float a, float b) {
    const float m = fmaxf(a, b);
    const float lz = logf(expf(a - m) + expf(b - m));
    l0 = (a - m) - lz;
    l1 = (b - m) - lz;
  }
};

// ------------------------------------------------------------------ fg / bg maps
// One workgroup per image: t = max over the A object channels, m = max t, then the two
// strict compares against m * high and m * low (one fp32 multiply each), integer counts and
// the two ratios.  t is recomputed in the second pass (A loads per cell, L2 hits) instead of
// staged, so any H * W fits.
__device__ __forceinline__ float cell_max(const float* __restrict__ p, int A, int HW, int q) {
  float t = p[q];
  for (int a = 1; a < A; ++a) t = fmaxf(t, p[(size_t)a * HW + q]);
  return t;
}

__global__ void __launch_bounds__(kRedThreads)
fgbg_maps_kernel(const float* __restrict__ prob, int A, int HW, float high, float low,
                 float* __restrict__ f, float* __restrict__ b, float* __restrict__ stats) {
  __shared__ float shm[16];
  __shared__ int shc[16 * 2];
  const int img = blockIdx.x;
  const float* obj = prob + ((size_t)img * 2 * A + A) * HW;  // channels A .. 2A-1
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
  float m = -INFINITY;
  for (int q = threadIdx.x; q < HW; q += blockDim.x) m = fmaxf(m, cell_max(obj, A, HW, q));
  for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_down(m, o));
  if (lane == 0) shm[wave] = m;
  __syncthreads();
  m = shm[0];
  for (int w = 1; w < nw; ++w) m = fmaxf(m, shm[w]);
  const float th = m * high, tl = m * low;
  int nf = 0, nb = 0;
  for (int q = threadIdx.x; q < HW; q += blockDim.x) {
    const float t = cell_max(obj, A, HW, q);
    const bool isf = t > th, isb = t < tl;
    f[(size_t)img * HW + q] = isf ? 1.f : 0.f;
    b[(size_t)img * HW + q] = isb ? 1.f : 0.f;
    nf += isf;
    nb += isb;
  }
  for (int o = 32; o > 0; o >>= 1) {
    nf += __shfl_down(nf, o);
    nb += __shfl_down(nb, o);
  }
  if (lane == 0) {
    shc[2 * wave] = nf;
    shc[2 * wave + 1] = nb;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    nf = nb = 0;
    for (int w = 0; w < nw; ++w) {
      nf += shc[2 * w];
      nb += shc[2 * w + 1];
    }
    // the 0/1 sums are exact in fp32 (H * W < 2^24): the reference's sum() / (sum() + sum())
    const float sf = (float)nf, sb = (float)nb, den = sf + sb;
    float* s = stats + 5 * img;
    s[0] = m;
    s[1] = sf;
    s[2] = sb;
    s[3] = den > 0.f ? sf / den : 0.f;  // den = 0 only for high >= 1 (the max cell is in f)
    s[4] = den > 0.f ? sb / den : 0.f;
  }
}

// ------------------------------------------------------------------ masked 2-way NLL
struct NllArgs {
  const float* score[kMaxPairs];  // (B, 2, H, W)
  const float* map[kMaxPairs];    // (B, H, W), 0 / 1
  float* dscore[kMaxPairs];
};

// grid (B, K): loss[k * B + b] = mean over map == 1 of -log_softmax(score)[label_b], 0 for
// an empty map; count[k * B + b] = the number of map cells (saved for the backward).
__global__ void __launch_bounds__(kRedThreads)
masked_nll2_fwd_kernel(NllArgs a, const float* __restrict__ need, int B, int HW,
                       float* __restrict__ loss, float* __restrict__ count) {
  __shared__ double sh[16 * 2];
  const int img = blockIdx.x, k = blockIdx.y;
  const float* s = a.score[k] + (size_t)img * 2 * HW;
  const float* mp = a.map[k] + (size_t)img * HW;
  const bool one = (long long)need[img] == 1;
  double v[2] = {0.0, 0.0};
  for (int q = threadIdx.x; q < HW; q += blockDim.x) {
    if (mp[q] != 1.f) continue;
    const LogSoftmax2 ls(s[q], s[HW + q]);
    v[0] -= (double)(one ? ls.l1 : ls.l0);
    v[1] += 1.0;
  }
  block_sum<2>(v, sh);
  if (threadIdx.x == 0) {
    loss[k * B + img] = v[1] > 0.0 ? (float)(v[0] / v[1]) : 0.f;
    count[k * B + img] = (float)v[1];
  }
}

// grid (blocks, B, K): dscore = map * (softmax - onehot) * gout / count, 0 for count = 0;
// every element of every dscore is written.
__global__ void __launch_bounds__(256)
masked_nll2_bwd_kernel(NllArgs a, const float* __restrict__ need, int B, int HW,
                       const float* __restrict__ gout, const float* __restrict__ count) {
  const int img = blockIdx.y, k = blockIdx.z;
  const float* s = a.score[k] + (size_t)img * 2 * HW;
  const float* mp = a.map[k] + (size_t)img * HW;
  float* d = a.dscore[k] + (size_t)img * 2 * HW;
  const float n = count[k * B + img];
  const float g = n > 0.f ? gout[k * B + img] / n : 0.f;
  const bool one = (long long)need[img] == 1;
  for (int q = blockIdx.x * blockDim.x + threadIdx.x; q < HW; q += gridDim.x * blockDim.x) {
    float d0 = 0.f, d1 = 0.f;
    if (n > 0.f && mp[q] == 1.f) {
      const LogSoftmax2 ls(s[q], s[HW + q]);
      d0 = g * (expf(ls.l0) - (one ? 0.f : 1.f));
      d1 = g * (expf(ls.l1) - (one ? 1.f : 0.f));
    }
    d[q] = d0;
    d[HW + q] = d1;
  }
}

// ------------------------------------------------------------------ KD KL
// Row r, class c of the student / teacher scores is x[r * row_stride + c * class_stride];
// the row's weight is weight[r % wmod] (wmod = H * W expands the RPN's g[h, w] over the
// anchors by index).  With z = x / T: log p_c = (z_c - max z) - log sum exp(z - max z), and
// KL_r = sum_c p1_c (log p1_c - log p2_c): log-sum-exp form, no quotient of probabilities.
// The row terms are evaluated in double from the fp32 scores: KL_r and the gradient's
// (log p1 - log p2 - KL_r) are differences of O(1) terms, and fp32's ~1e-8 absolute error
// in them is more than 2e-5 of a small KL (a student close to its teacher).  The rows are
// short (C classes) and few, so the double exp / log cost nothing next to the launch.
struct KlRow {
  double m1, lz1, m2, lz2, kl;
};

__device__ __forceinline__ KlRow kl_row(const float* __restrict__ s, const float* __restrict__ t,
                                        int C, long long cs, double T) {
  KlRow r;
  r.m1 = (double)s[0] / T;
  r.m2 = (double)t[0] / T;
  for (int c = 1; c < C; ++c) {
    r.m1 = fmax(r.m1, (double)s[c * cs] / T);
    r.m2 = fmax(r.m2, (double)t[c * cs] / T);
  }
  double z1 = 0.0, z2 = 0.0;
  for (int c = 0; c < C; ++c) {
    z1 += exp((double)s[c * cs] / T - r.m1);
    z2 += exp((double)t[c * cs] / T - r.m2);
  }
  r.lz1 = log(z1);
  r.lz2 = log(z2);
  double kl = 0.0;
  for (int c = 0; c < C; ++c) {
    const double l1 = ((double)s[c * cs] / T - r.m1) - r.lz1;
    const double l2 = ((double)t[c * cs] / T - r.m2) - r.lz2;
    kl += exp(l1) * (l1 - l2);
  }
  r.kl = kl;
  return r;
}

// One workgroup: out[0] = sum_r w_r KL_r / (sum w + 1), out[1] = sum w + 1 (for the backward);
// sum w runs over the wmod weights, not over the rows that share them.
__global__ void __launch_bounds__(kRedThreads)
kd_kl_fwd_kernel(const float* __restrict__ student, const float* __restrict__ teacher,
                 const float* __restrict__ weight, int R, int C, long long rs, long long cs,
                 int wmod, float T, float* __restrict__ out) {
  __shared__ double sh[16 * 2];
  double v[2] = {0.0, 0.0};
  for (int r = threadIdx.x; r < R; r += blockDim.x) {
    const float w = weight[r % wmod];
    if (r < wmod) v[1] += (double)w;  // the normaliser counts each weight once (sum g + 1)
    if (w == 0.f) continue;
    const KlRow k = kl_row(student + r * rs, teacher + r * rs, C, cs, (double)T);
    v[0] += (double)w * k.kl;
  }
  block_sum<2>(v, sh);
  if (threadIdx.x == 0) {
    out[0] = (float)(v[0] / (v[1] + 1.0));
    out[1] = (float)(v[1] + 1.0);
  }
}

// dstudent[r, j] = gout * w_r / (sum w + 1) * (1 / T) * p1_j (log p1_j - log p2_j - KL_r);
// every element is written (0 where w_r = 0).
__global__ void __launch_bounds__(256)
kd_kl_bwd_kernel(const float* __restrict__ student, const float* __restrict__ teacher,
                 const float* __restrict__ weight, int R, int C, long long rs, long long cs,
                 int wmod, float T, const float* __restrict__ gout,
                 const float* __restrict__ aux, float* __restrict__ dstudent) {
  const double Td = (double)T;
  const double g = (double)gout[0] / (double)aux[1] / Td;
  for (int r = blockIdx.x * blockDim.x + threadIdx.x; r < R; r += gridDim.x * blockDim.x) {
    const float w = weight[r % wmod];
    const float* s = student + r * rs;
    const float* t = teacher + r * rs;
    float* d = dstudent + r * rs;
    if (w == 0.f) {
      for (int c = 0; c < C; ++c) d[c * cs] = 0.f;
      continue;
    }
    const KlRow k = kl_row(s, t, C, cs, Td);
    const double gw = g * (double)w;
    for (int c = 0; c < C; ++c) {
      const double l1 = ((double)s[c * cs] / Td - k.m1) - k.lz1;
      const double l2 = ((double)t[c * cs] / Td - k.m2) - k.lz2;
      d[c * cs] = (float)(gw * (exp(l1) * ((l1 - l2) - k.kl)));
    }
  }
}

// ------------------------------------------------------------------ gt cell mask
// One thread per cell over the first min(num_boxes, G) boxes: faster_rcnn_kd.py:58-65's
// range(int(x1 / 16), int(x2 / 16)) x range(int(y1 / 16), int(y2 / 16)); x * 0.0625f is the
// exact fp32 quotient and (int) truncates as Python's int().
__global__ void __launch_bounds__(256)
gt_cell_mask_kernel(const float* __restrict__ gt, const long long* __restrict__ num_boxes,
                    int G, int H, int W, float* __restrict__ g) {
  const int q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= H * W) return;
  const int j = q / W, i = q - j * W;
  long long n = num_boxes[0];
  n = n < 0 ? 0 : (n > G ? G : n);
  float hit = 0.f;
  for (int k = 0; k < (int)n; ++k) {
    const float* bb = gt + 5 * k;
    const int x1 = (int)(bb[0] * 0.0625f), y1 = (int)(bb[1] * 0.0625f);
    const int x2 = (int)(bb[2] * 0.0625f), y2 = (int)(bb[3] * 0.0625f);
    if (i >= x1 && i < x2 && j >= y1 && j < y2) hit = 1.f;
  }
  g[q] = hit;
}

int nll_args(const float* const* scores, const float* const* maps, float* const* dscores, int K,
             NllArgs* a) {
  TLOD_CHECK_ARG(scores && maps, "null pointer");
  TLOD_CHECK_ARG(K > 0 && K <= kMaxPairs, "1..8 (score, map) pairs per call");
  for (int k = 0; k < kMaxPairs; ++k) {
    const int j = k < K ? k : 0;
    TLOD_CHECK_ARG(scores[j] && maps[j] && (!dscores || dscores[j]), "null pointer in a pair");
    a->score[k] = scores[j];
    a->map[k] = maps[j];
    a->dscore[k] = dscores ? dscores[j] : nullptr;
  }
  return kOk;
}

}  // namespace
}  // namespace tlod

using namespace tlod;

extern "C" {

int tlod_fgbg_maps_f32(const float* prob, int B, int A, int H, int W, float high, float low,
                       float* f, float* b, float* stats, tlod_stream_t stream) {
  TLOD_CHECK_ARG(prob && f && b && stats, "null pointer");
  TLOD_CHECK_ARG(B > 0 && A > 0 && H > 0 && W > 0 && (long long)H * W < (1 << 24),
                 "bad shape");
  fgbg_maps_kernel<<<B, kRedThreads, 0, (hipStream_t)stream>>>(prob, A, H * W, high, low, f, b,
                                                               stats);
  TLOD_LAUNCH_CHECK();
  return kOk;
}

int tlod_masked_nll2_f32(const float* const* scores, const float* const* maps, int K,
                         const float* need, int B, int H, int W, float* loss, float* count,
                         tlod_stream_t stream) {
  TLOD_CHECK_ARG(need && loss && count, "null pointer");
  TLOD_CHECK_ARG(B > 0 && B <= 65535 && H > 0 && W > 0 && (long long)H * W < (1 << 24),
                 "bad shape");
  NllArgs a;
  const int st = nll_args(scores, maps, nullptr, K, &a);
  if (st != kOk) return st;
  masked_nll2_fwd_kernel<<<dim3(B, K), kRedThreads, 0, (hipStream_t)stream>>>(a, need, B, H * W,
                                                                              loss, count);
  TLOD_LAUNCH_CHECK();
  return kOk;
}

int tlod_masked_nll2_bwd_f32(const float* const* scores, const float* const* maps, int K,
                             const float* need, int B, int H, int W, const float* grad_loss,
                             const float* count, float* const* dscores, tlod_stream_t stream) {
  TLOD_CHECK_ARG(need && grad_loss && count && dscores, "null pointer");
  TLOD_CHECK_ARG(B > 0 && B <= 65535 && H > 0 && W > 0 && (long long)H * W < (1 << 24),
                 "bad shape");
  NllArgs a;
  const int st = nll_args(scores, maps, dscores, K, &a);
  if (st != kOk) return st;
  const int HW = H * W;
  const int gx = div_up(HW, 256) > 64 ? 64 : div_up(HW, 256);
  masked_nll2_bwd_kernel<<<dim3(gx, B, K), 256, 0, (hipStream_t)stream>>>(a, need, B, HW,
                                                                         grad_loss, count);
  TLOD_LAUNCH_CHECK();
  return kOk;
}

static int kd_check(const float* student, const float* teacher, const float* weight, int R, int C,
                    long long row_stride, long long class_stride, int wmod, float T) {
  TLOD_CHECK_ARG(student && teacher && weight, "null pointer");
  TLOD_CHECK_ARG(R > 0 && C > 0 && wmod > 0 && wmod <= R && row_stride > 0 && class_stride > 0,
                 "bad shape / strides");
  TLOD_CHECK_ARG(T > 0.f, "temperature must be positive");
  return kOk;
}

int tlod_kd_kl_f32(const float* student, const float* teacher, const float* weight, int R, int C,
                   long long row_stride, long long class_stride, int wmod, float T, float* out,
                   tlod_stream_t stream) {
  TLOD_CHECK_ARG(out, "null pointer");
  const int st = kd_check(student, teacher, weight, R, C, row_stride, class_stride, wmod, T);
  if (st != kOk) return st;
  kd_kl_fwd_kernel<<<1, kRedThreads, 0, (hipStream_t)stream>>>(
      student, teacher, weight, R, C, row_stride, class_stride, wmod, T, out);
  TLOD_LAUNCH_CHECK();
  return kOk;
}

int tlod_kd_kl_bwd_f32(const float* student, const float* teacher, const float* weight, int R,
                       int C, long long row_stride, long long class_stride, int wmod, float T,
                       const float* grad_loss, const float* aux, float* dstudent,
                       tlod_stream_t stream) {
  TLOD_CHECK_ARG(grad_loss && aux && dstudent, "null pointer");
  const int st = kd_check(student, teacher, weight, R, C, row_stride, class_stride, wmod, T);
  if (st != kOk) return st;
  const int grid = div_up(R, 256) > 1024 ? 1024 : div_up(R, 256);
  kd_kl_bwd_kernel<<<grid, 256, 0, (hipStream_t)stream>>>(student, teacher, weight, R, C,
                                                          row_stride, class_stride, wmod, T,
                                                          grad_loss, aux, dstudent);
  TLOD_LAUNCH_CHECK();
  return kOk;
}

int tlod_gt_cell_mask_f32(const float* gt_boxes, const long long* num_boxes, int G, int H, int W,
                          float* g, tlod_stream_t stream) {
  TLOD_CHECK_ARG(gt_boxes && num_boxes && g, "null pointer");
  TLOD_CHECK_ARG(G >= 0 && H > 0 && W > 0 && (long long)H * W < (1 << 24), "bad shape");
  gt_cell_mask_kernel<<<div_up(H * W, 256), 256, 0, (hipStream_t)stream>>>(gt_boxes, num_boxes, G,
                                                                           H, W, g);
  TLOD_LAUNCH_CHECK();
  return kOk;
}

}  // extern "C"
