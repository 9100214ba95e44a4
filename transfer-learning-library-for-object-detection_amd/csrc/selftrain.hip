// IDF self-training device ops (include/tlod_selftrain.h): the pseudo ground truth of one target
// image packed from tlod_detect_f32's outputs, and the domain losses with EFocalLoss.
//
// The packer stands in for the reference's offline label route — faster_rcnn_test.py --savelabel
// (:316-369) writes str(int(x)) into VOC XML, foggy_cityscape.py:239-242 reads max(x - 1, 0) into
// an integer roidb, minibatch.py:39-49 multiplies by the Python-float image scale into float32,
// roibatchLoader drops the degenerate rows, shuffles and keeps MAX_NUM_GT_BOXES — so a frozen
// detector can label the target image inside the training step without a host round trip.
//
// Launch shape: a latency-bound tail over at most (C - 1) R <= a few thousand rows of one image,
// so one workgroup of 16 waves and no workspace.  The (class, row) slots are walked class-major
// 1024 at a time; a slot's survivor rank is its wave's ballot prefix plus the waves' counts
// scanned through LDS, which keeps the reference's order without a sort.  The common case
// (n <= max_gt) is that one walk.  Otherwise the max_gt-th smallest key is found by an 8-bit
// radix select over the keys — they depend on the rank alone, rng_u64(seed, stream, r), so they
// are recomputed, never stored — with a 256-bin LDS histogram per digit, and a second walk
// writes the selected rows in ascending rank.  Equal keys are broken by rank, as the rule says.
//
// Arithmetic: trunc, - 1 and the clamp in double (exact for every float), one double product,
// one rounding to float.  Nothing here can contract.
#include "common.h"
#include "tlod_selftrain.h"

namespace tlod {
namespace {

constexpr int kMaxR = 2048;             // detect.hip's bound on R
constexpr int kThreads = 1024;
constexpr int kWaves = kThreads / 64;
constexpr uint64_t kPseudoStream = 0x70736575ull;  // clear of the sampling layers' streams
constexpr int kRed = 256;               // the loss launches, as idf.hip

struct PackShared {
  uint32_t surv[2][kWaves], lt[kWaves], eq[kWaves];  // surv: one per walk-iteration parity
  uint32_t hist[256];
  uint32_t digit, rest;
};

// Exclusive prefix of this thread's wave over per-wave counts, and their total.
__device__ __forceinline__ uint32_t wave_offset(const uint32_t* cnt, uint32_t* total) {
  const int wave = threadIdx.x >> 6;
  uint32_t off = 0, sum = 0;
#pragma unroll
  for (int w = 0; w < kWaves; ++w) {
    const uint32_t c = cnt[w];
    if (w < wave) off += c;
    sum += c;
  }
  *total = sum;
  return off;
}

// One ordered walk over the (class, row) slots.  A survivor of rank r is written when
//   all:  at row r (if r < max_gt);
//   else: when key(r) < kstar, or key(r) == kstar and fewer than `ties` equal keys precede it —
//         at the row given by the count of selected survivors before it.
// Returns the number of survivors (the same in every thread).
__device__ uint32_t pack_walk(const float* __restrict__ dets, const int32_t* __restrict__ counts,
                              int C, int R, double im_scale, int max_gt, uint64_t seed, bool all,
                              uint64_t kstar, uint32_t ties, float* __restrict__ out,
                              PackShared& sh) {
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const uint64_t below = (1ull << lane) - 1ull;
  const int total = (C - 1) * R;
  uint32_t n = 0, n_lt = 0, n_eq = 0;
  for (int base = 0, it = 0; base < total; base += kThreads, ++it) {  // uniform trip count
    uint32_t* surv = sh.surv[it & 1];
    const int slot = base + t;
    bool ok = false;
    float g[4] = {0.f, 0.f, 0.f, 0.f};
    int j = 0;
    if (slot < total) {
      j = 1 + slot / R;
      const int i = slot - (j - 1) * R;
      if (i < counts[j]) {  // rows at or past counts[j] are never read
        const float* d = dets + ((size_t)j * R + i) * 5;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const double v = fmax(trunc((double)d[k]) - 1.0, 0.0);
          g[k] = (float)(v * im_scale);
        }
        ok = !(g[0] == g[2] || g[1] == g[3]);
      }
    }
    const uint64_t b = __ballot(ok);
    if (lane == 0) surv[wave] = (uint32_t)__popcll(b);
    __syncthreads();
    uint32_t chunk;
    const uint32_t r = n + wave_offset(surv, &chunk) + (uint32_t)__popcll(b & below);
    n += chunk;
    uint32_t pos = r;
    bool sel = ok;
    if (!all) {  // uniform
      const uint64_t key = ok ? rng_u64(seed, kPseudoStream, r) : 0;
      const bool is_lt = ok && key < kstar, is_eq = ok && key == kstar;
      const uint64_t bl = __ballot(is_lt), be = __ballot(is_eq);
      if (lane == 0) {
        sh.lt[wave] = (uint32_t)__popcll(bl);
        sh.eq[wave] = (uint32_t)__popcll(be);
      }
      __syncthreads();
      uint32_t c_lt, c_eq;
      const uint32_t p_lt = n_lt + wave_offset(sh.lt, &c_lt) + (uint32_t)__popcll(bl & below);
      const uint32_t p_eq = n_eq + wave_offset(sh.eq, &c_eq) + (uint32_t)__popcll(be & below);
      n_lt += c_lt;
      n_eq += c_eq;
      sel = is_lt || (is_eq && p_eq < ties);
      pos = p_lt + min(p_eq, ties);
    }
    if (sel && pos < (uint32_t)max_gt) {
      float* o = out + (size_t)pos * 5;
      o[0] = g[0]; o[1] = g[1]; o[2] = g[2]; o[3] = g[3];
      o[4] = (float)j;
    }
    // an `all` walk has one barrier an iteration, so surv alternates between two buffers: this
    // one is next written behind the next iteration's barrier, as are sh.lt / sh.eq, when every
    // reader of this iteration is past its reads
  }
  return n;
}

// The k-th smallest (1-based) of rng_u64(seed, stream, r), r < n (k <= n), one 8-bit digit a
// round from the top; *ties = how many keys equal to it the k smallest include.
__device__ uint64_t kth_key(uint64_t seed, uint32_t n, uint32_t k, uint32_t* ties,
                            PackShared& sh) {
  const int t = threadIdx.x;
  uint64_t prefix = 0;
  for (int shift = 56; shift >= 0; shift -= 8) {
    if (t < 256) sh.hist[t] = 0;
    __syncthreads();
    for (uint32_t r = t; r < n; r += kThreads) {
      const uint64_t key = rng_u64(seed, kPseudoStream, r);
      // the digits above this one match the prefix chosen so far
      if (shift == 56 || (key >> (shift + 8)) == (prefix >> (shift + 8)))
        atomicAdd(&sh.hist[(key >> shift) & 255], 1u);
    }
    __syncthreads();
    if (t < 64) {  // wave 0: four bins a lane, scanned across the wave
      uint32_t h[4], s = 0;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        h[q] = sh.hist[4 * t + q];
        s += h[q];
      }
      uint32_t incl = s;
      for (int o = 1; o < 64; o <<= 1) {
        const uint32_t up = __shfl_up(incl, o);
        if (t >= o) incl += up;
      }
      const uint64_t reach = __ballot(incl >= k);  // never empty: k <= the keys still in play
      if (reach != 0 && t == __ffsll((long long)reach) - 1) {
        uint32_t rest = k - (incl - s);  // 1-based rank inside this lane's four bins
        int q = 0;
        while (q < 3 && rest > h[q]) rest -= h[q++];
        sh.digit = 4 * t + q;
        sh.rest = rest;
      }
    }
    __syncthreads();
    prefix |= (uint64_t)sh.digit << shift;
    k = sh.rest;
    // sh.digit / sh.rest are next written two barriers on
  }
  *ties = k;
  return prefix;
}

__global__ void __launch_bounds__(kThreads)
pseudo_gt_kernel(const float* __restrict__ dets, const int32_t* __restrict__ counts, int C, int R,
                 double im_scale, int max_gt, uint64_t seed, float* __restrict__ gt_boxes,
                 long long* __restrict__ num_boxes) {
  __shared__ PackShared sh;
  uint32_t n = pack_walk(dets, counts, C, R, im_scale, max_gt, seed, true, 0, 0, gt_boxes, sh);
  if (n > (uint32_t)max_gt) {  // uniform
    __syncthreads();  // the first walk's rows are overwritten: order the stores
    uint32_t ties;
    const uint64_t kstar = kth_key(seed, n, (uint32_t)max_gt, &ties, sh);
    pack_walk(dets, counts, C, R, im_scale, max_gt, seed, false, kstar, ties, gt_boxes, sh);
    n = (uint32_t)max_gt;
  }
  for (size_t e = (size_t)n * 5 + threadIdx.x; e < (size_t)max_gt * 5; e += kThreads)
    gt_boxes[e] = 0.f;
  if (threadIdx.x == 0) *num_boxes = (long long)n;
}

// ---------------------------------------------------------------------------- EFocalLoss
// (idf.hip's helpers restated, so that file and its results stay what they are)
__device__ __forceinline__ double wave_sum(double v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o);
  return v;
}

// softmax[label] of a two-logit row, in double.
__device__ __forceinline__ double p_label(const float* __restrict__ z, int label) {
  const double zl = (double)z[label], zo = (double)z[1 - label];
  return 1.0 / (1.0 + exp(zo - zl));
}

// One workgroup.  loss[i < n_img] = CE(z_img[i], label_img); loss[n_img] = EFocal mean.
__global__ void __launch_bounds__(kRed)
domain_loss_ef_fwd_kernel(const float* __restrict__ z_img, int n_img, int label_img,
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
    const double p = p_label(z_ins + 2 * (size_t)r, label_ins);  // no clamp
    v += -exp(-gamma * p) * log(p);
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
domain_loss_ef_bwd_kernel(const float* __restrict__ z_img, int n_img, int label_img,
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
  // L = -exp(-gamma p) log p; dL/dp = exp(-gamma p) (gamma log p - 1 / p)
  const double dLdp = exp(-gamma * p) * (gamma * log(p) - 1.0 / p);
  const double g = (double)g_loss[n_img] / (double)R * dLdp * p * (1.0 - p);  // dp / dz[label]
  dz_ins[2 * (size_t)r + label_ins] = (float)g;
  dz_ins[2 * (size_t)r + 1 - label_ins] = (float)(-g);
}

}  // namespace
}  // namespace tlod

using namespace tlod;

extern "C" {

int tlod_pseudo_gt_f32(const float* dets, const int32_t* counts, int C, int R, double im_scale,
                       int max_gt, uint64_t seed, float* gt_boxes, int64_t* num_boxes,
                       tlod_stream_t stream) {
  TLOD_CHECK_ARG(dets && counts && gt_boxes && num_boxes, "null pointer");
  TLOD_CHECK_ARG(C >= 2 && R > 0 && R <= kMaxR && (long long)(C - 1) * R <= 0x7fffffffLL,
                 "bad sizes");
  TLOD_CHECK_ARG(max_gt >= 1, "max_gt < 1");
  TLOD_CHECK_ARG(im_scale > 0.0, "im_scale <= 0");
  pseudo_gt_kernel<<<1, kThreads, 0, (hipStream_t)stream>>>(
      dets, counts, C, R, im_scale, max_gt, seed, gt_boxes,
      reinterpret_cast<long long*>(num_boxes));
  TLOD_LAUNCH_CHECK();
  return kOk;
}

int tlod_idf_domain_loss_ef_f32(const float* z_img, int n_img, int label_img, const float* z_ins,
                                int R, int label_ins, float gamma, float* loss,
                                tlod_stream_t stream) {
  TLOD_CHECK_ARG(z_ins && loss && (z_img || n_img == 0), "null pointer");
  TLOD_CHECK_ARG(n_img >= 0 && R > 0, "bad shape");
  TLOD_CHECK_ARG((label_img == 0 || label_img == 1) && (label_ins == 0 || label_ins == 1),
                 "labels are 0 or 1");
  domain_loss_ef_fwd_kernel<<<1, kRed, 0, (hipStream_t)stream>>>(
      z_img, n_img, label_img, z_ins, R, label_ins, (double)gamma, loss);
  TLOD_LAUNCH_CHECK();
  return kOk;
}

int tlod_idf_domain_loss_ef_bwd_f32(const float* z_img, int n_img, int label_img,
                                    const float* z_ins, int R, int label_ins, float gamma,
                                    const float* g_loss, float* dz_img, float* dz_ins,
                                    tlod_stream_t stream) {
  TLOD_CHECK_ARG(z_ins && g_loss && dz_ins && ((z_img && dz_img) || n_img == 0), "null pointer");
  TLOD_CHECK_ARG(n_img >= 0 && R > 0, "bad shape");
  TLOD_CHECK_ARG((label_img == 0 || label_img == 1) && (label_ins == 0 || label_ins == 1),
                 "labels are 0 or 1");
  domain_loss_ef_bwd_kernel<<<div_up(n_img + R, kRed), kRed, 0, (hipStream_t)stream>>>(
      z_img, n_img, label_img, z_ins, R, label_ins, (double)gamma, g_loss, dz_img, dz_ins);
  TLOD_LAUNCH_CHECK();
  return kOk;
}

}  // extern "C"
