// RoI crop (POOLING_MODE 'crop') for gfx950: the bilinear grid sampler of
// lib/model/roi_crop/src/roi_crop_cuda_kernel.cu:11-194 and the fused affine grid + sampler +
// 2x2 max-pool the detectors use (lib/model/faster_rcnn/faster_rcnn.py:73-81,
// lib/model/utils/net_utils.py:142-164).
//
// Numerics follow the CUDA kernel's operation order (compiled with -ffp-contract=off):
// getTopLeft's coordinate and weight, the four in-bounds tests, the weighted sum left to right.
// A sample whose four taps are all outside the map is written as 0 (the reference leaves its
// zero-initialised output untouched there).
//
// Layout choices (MI355X-first, not a translation of the reference launch shape):
//   * fused forward: one workgroup per (roi, 64 channels).  theta and the 2P coordinates /
//     weights per axis are computed once into LDS; a thread owns one pooled output, so a wave
//     covers 64 consecutive outputs of one or two channels: its stores (value and argmax
//     byte) are contiguous and each of its loads touches at most P short W-runs of the map.
//     No grid and no (R, C, 2P, 2P) map is written.
//   * both backwards are owner-computes gathers, no atomics: a workgroup owns one map row
//     (x up to 96 columns) of 64 channels in LDS, one thread per channel.  It walks the RoIs
//     of its image in index order and their outputs / samples in row-major order, skipping
//     what misses its row, so every cell's sum has a fixed order: two runs are bit-identical.
//     The owner then writes its row of grad_in, zeros included (no pre-zeroing needed).
#include <algorithm>

#include "common.h"
#include "tlod.h"

namespace tlod {

constexpr int kCropCh = 64;        // channels per forward workgroup
constexpr int kCropThreads = 256;
constexpr int kCropMaxG = 32;      // samples per axis (P, or 2P with the max-pool)
constexpr int kCbCh = 64;          // backward: channels (= threads) per workgroup
constexpr int kCbTw = 96;          // backward: map columns per workgroup
constexpr int kCbLd = kCbCh + 1;   // LDS row pitch (the write-out reads across cells)

// roi_crop_cuda_kernel.cu:11-22 (getTopLeft).  The clamp only moves coordinates whose two
// taps are both outside [0, size-1] either way (and NaN): it keeps the int conversion and
// point + 1 defined, the weight finite, and changes no in-range value.
__device__ __forceinline__ void crop_top_left(float x, int size, int* point, float* weight) {
  float xcoord = (x + 1.f) * (float)(size - 1) / 2.f;
  xcoord = fminf(fmaxf(xcoord, -2.f), (float)size);
  const float f = floorf(xcoord);
  *point = (int)f;
  *weight = 1.f - (xcoord - f);
}

__device__ __forceinline__ bool crop_between(int v, int lo, int hi) { return v >= lo && v <= hi; }

// roi_crop_cuda_kernel.cu:82-104: the 4-tap value, taps outside the map contribute 0
__device__ __forceinline__ float crop_sample(const float* __restrict__ plane, int H, int W, int y0,
                                             int x0, float wy, float wx) {
  const bool xl = crop_between(x0, 0, W - 1), xr = crop_between(x0 + 1, 0, W - 1);
  const bool yt = crop_between(y0, 0, H - 1), yb = crop_between(y0 + 1, 0, H - 1);
  float tl = 0.f, tr = 0.f, bl = 0.f, br = 0.f;
  if (xl && yt) tl = plane[y0 * W + x0];
  if (xr && yt) tr = plane[y0 * W + x0 + 1];
  if (xl && yb) bl = plane[(y0 + 1) * W + x0];
  if (xr && yb) br = plane[(y0 + 1) * W + x0 + 1];
  return wx * wy * tl + (1.f - wx) * wy * tr + wx * (1.f - wy) * bl +
         (1.f - wx) * (1.f - wy) * br;
}

// net_utils.py:154-160: one row of theta for the axis [lo, hi] of a map of `size` cells
__device__ __forceinline__ void crop_theta(float lo, float hi, int size, float* a, float* t) {
  const float d = (float)(size - 1);
  *a = (hi - lo) / d;
  *t = (lo + hi - (float)size + 1.f) / d;
}

// base grid of F.affine_grid(align_corners=True): G points spanning [-1, 1] inclusive
__device__ __forceinline__ float crop_base(int i, int G) {
  return G > 1 ? (float)(2 * i - (G - 1)) / (float)(G - 1) : -1.f;
}

// rois[:, 0] names the image; a value outside [0, B) (or NaN) selects none
__device__ __forceinline__ bool crop_image(float v, int B, int* b) {
  const bool ok = v >= 0.f && v < (float)B;
  *b = ok ? (int)v : 0;
  return ok;
}

// ------------------------------------------------------------ general sampler, forward
__global__ void __launch_bounds__(256) roi_crop_fwd_kernel(
    long total, const float* __restrict__ x, int C, int H, int W, const float* __restrict__ grid,
    int per_image, int gh, int gw, float* __restrict__ out) {
  for (long index = (long)blockIdx.x * blockDim.x + threadIdx.x; index < total;
       index += (long)blockDim.x * gridDim.x) {
    const int xo = (int)(index % gw);
    const int yo = (int)((index / gw) % gh);
    const int c = (int)((index / gw / gh) % C);
    const int r = (int)(index / gw / gh / C);
    const int b = r / per_image;
    const float* g = grid + (((size_t)r * gh + yo) * gw + xo) * 2;
    int y0, x0;
    float wy, wx;
    crop_top_left(g[1], W, &x0, &wx);
    crop_top_left(g[0], H, &y0, &wy);
    out[index] = crop_sample(x + ((size_t)b * C + c) * H * W, H, W, y0, x0, wy, wx);
  }
}

// ------------------------------------------------------------ fused forward
// grid (R, ceil(C / 64)); out (R, C, P, P); argmax: which of the 2x2 samples won (row-major,
// first on ties, as F.max_pool2d)
__global__ void __launch_bounds__(kCropThreads) roi_crop_pool_fwd_kernel(
    const float* __restrict__ x, int B, int C, int H, int W, const float* __restrict__ rois, int P,
    float scale, int max_pool, float* __restrict__ out, uint8_t* __restrict__ argmax) {
  const int G = max_pool ? 2 * P : P;
  const int r = blockIdx.x, c0 = blockIdx.y * kCropCh, t = threadIdx.x;
  const int nc = min(kCropCh, C - c0);
  __shared__ int sy0[kCropMaxG], sx0[kCropMaxG];
  __shared__ float swy[kCropMaxG], swx[kCropMaxG];
  const float* ro = rois + (size_t)r * 5;
  if (t < G) {
    float a, s;
    crop_theta(ro[2] * scale, ro[4] * scale, H, &a, &s);
    crop_top_left(a * crop_base(t, G) + s, H, &sy0[t], &swy[t]);
  } else if (t >= 64 && t < 64 + G) {
    const int i = t - 64;
    float a, s;
    crop_theta(ro[1] * scale, ro[3] * scale, W, &a, &s);
    crop_top_left(a * crop_base(i, G) + s, W, &sx0[i], &swx[i]);
  }
  __syncthreads();
  int b;
  const bool bok = crop_image(ro[0], B, &b);
  const int PP = P * P;
  const size_t o0 = ((size_t)r * C + c0) * PP;
  const float* base = x + ((size_t)b * C + c0) * H * W;
  for (int e = t; e < nc * PP; e += kCropThreads) {
    const int c = e / PP, q = e % PP;
    const int py = q / P, px = q % P;
    const float* plane = base + (size_t)c * H * W;
    float best = 0.f;
    int bi = 0;
    if (bok) {
      if (max_pool) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const int sy = 2 * py + (k >> 1), sx = 2 * px + (k & 1);
          const float v = crop_sample(plane, H, W, sy0[sy], sx0[sx], swy[sy], swx[sx]);
          if (k == 0 || v > best || v != v) {
            best = v;
            bi = k;
          }
        }
      } else {
        best = crop_sample(plane, H, W, sy0[py], sx0[px], swy[py], swx[px]);
      }
    }
    out[o0 + e] = best;
    if (max_pool) argmax[o0 + e] = (uint8_t)bi;
  }
}

// ------------------------------------------------------------ backward: the row owner
// One map row y, columns [x_lo, x_lo + tw), channel c0 + threadIdx.x: acc[j * kCbLd + t].
struct CropRow {
  int y, x_lo, tw;
  float* my;  // this thread's column of the LDS accumulator
  // one sample's taps on this row (roi_crop_cuda_kernel.cu:166-191: (wx * wy) * g etc.)
  __device__ __forceinline__ void add(int y0, float wy, int x0, float wx, float g) const {
    float wrow;
    if (y == y0) wrow = wy;
    else if (y == y0 + 1) wrow = 1.f - wy;
    else return;
    const int j0 = x0 - x_lo, j1 = j0 + 1;
    if (j0 >= 0 && j0 < tw) my[j0 * kCbLd] += wx * wrow * g;
    if (j1 >= 0 && j1 < tw) my[j1 * kCbLd] += (1.f - wx) * wrow * g;
  }
};

__device__ __forceinline__ void crop_row_store(const float* acc, int tw, int nc, size_t HW,
                                               float* __restrict__ dst) {
  // dst = grad_in + ((b * C + c0) * H + y) * W + x_lo; lanes along x
  for (int e = threadIdx.x; e < nc * tw; e += kCbCh) {
    const int c = e / tw, j = e % tw;
    dst[(size_t)c * HW + j] = acc[j * kCbLd + c];
  }
}

// grid (H * ceil(W / 96), ceil(C / 64), B)
__global__ void __launch_bounds__(kCbCh) roi_crop_pool_bwd_kernel(
    const float* __restrict__ grad_out, const uint8_t* __restrict__ argmax,
    const float* __restrict__ rois, int R, int B, int C, int H, int W, int P, float scale,
    int max_pool, float* __restrict__ grad_in) {
  __shared__ float acc[kCbTw * kCbLd];
  __shared__ float sbase[kCropMaxG];
  const int G = max_pool ? 2 * P : P, PP = P * P;
  const int t = threadIdx.x;
  const int y = blockIdx.x % H, x_lo = (blockIdx.x / H) * kCbTw;
  const int tw = min(kCbTw, W - x_lo);
  const int c0 = blockIdx.y * kCbCh, b = blockIdx.z;
  const int nc = min(kCbCh, C - c0);
  for (int i = t; i < tw * kCbLd; i += kCbCh) acc[i] = 0.f;
  if (t < G) sbase[t] = crop_base(t, G);
  __syncthreads();
  const CropRow row{y, x_lo, tw, acc + t};
  if (t < nc) {
    for (int r = 0; r < R; ++r) {
      const float* ro = rois + (size_t)r * 5;
      int rb;
      if (!crop_image(ro[0], B, &rb) || rb != b) continue;
      float ay, ty, ax, tx;
      crop_theta(ro[2] * scale, ro[4] * scale, H, &ay, &ty);
      crop_theta(ro[1] * scale, ro[3] * scale, W, &ax, &tx);
      // the grid is monotone along each axis: the RoI's row range is spanned by its ends
      int ya, yb;
      float wa, wb;
      crop_top_left(ay * sbase[0] + ty, H, &ya, &wa);
      crop_top_left(ay * sbase[G - 1] + ty, H, &yb, &wb);
      if (y < min(ya, yb) || y > max(ya, yb) + 1) continue;
      const size_t o0 = ((size_t)r * C + c0 + t) * PP;
      for (int py = 0; py < P; ++py) {
        int y0[2];
        float wy[2];
        if (max_pool) {
          crop_top_left(ay * sbase[2 * py] + ty, H, &y0[0], &wy[0]);
          crop_top_left(ay * sbase[2 * py + 1] + ty, H, &y0[1], &wy[1]);
        } else {
          crop_top_left(ay * sbase[py] + ty, H, &y0[0], &wy[0]);
          y0[1] = y0[0];
          wy[1] = wy[0];
        }
        if (y != y0[0] && y != y0[0] + 1 && y != y0[1] && y != y0[1] + 1) continue;
        for (int px = 0; px < P; ++px) {
          const float g = grad_out[o0 + py * P + px];
          const int k = max_pool ? (int)argmax[o0 + py * P + px] & 3 : 0;
          const int dy = k >> 1;
          int x0;
          float wx;
          crop_top_left(ax * sbase[max_pool ? 2 * px + (k & 1) : px] + tx, W, &x0, &wx);
          row.add(dy ? y0[1] : y0[0], dy ? wy[1] : wy[0], x0, wx, g);
        }
      }
    }
  }
  __syncthreads();
  crop_row_store(acc, tw, nc, (size_t)H * W,
                 grad_in + (((size_t)b * C + c0) * H + y) * W + x_lo);
}

// General grid: nothing is known about the samples, so each wave tests 64 of them at a time
// (lane = sample), and the channels (lane = channel) then visit the hits in ascending order.
__global__ void __launch_bounds__(kCbCh) roi_crop_bwd_kernel(
    const float* __restrict__ grad_out, const float* __restrict__ grid, int per_image, int C,
    int gh, int gw, int H, int W, float* __restrict__ grad_in) {
  __shared__ float acc[kCbTw * kCbLd];
  const int t = threadIdx.x, S = gh * gw;
  const int y = blockIdx.x % H, x_lo = (blockIdx.x / H) * kCbTw;
  const int tw = min(kCbTw, W - x_lo);
  const int c0 = blockIdx.y * kCbCh, b = blockIdx.z;
  const int nc = min(kCbCh, C - c0);
  for (int i = t; i < tw * kCbLd; i += kCbCh) acc[i] = 0.f;
  __syncthreads();
  const CropRow row{y, x_lo, tw, acc + t};
  const bool cok = t < nc;
  for (int r = b * per_image; r < (b + 1) * per_image; ++r) {
    const float* gr = grid + (size_t)r * S * 2;
    const float* go = grad_out + ((size_t)r * C + c0 + (cok ? t : 0)) * S;
    for (int s0 = 0; s0 < S; s0 += 64) {
      int y0 = 0, x0 = 0;
      float wy = 0.f, wx = 0.f;
      bool hit = false;
      if (s0 + t < S) {
        crop_top_left(gr[(size_t)(s0 + t) * 2], H, &y0, &wy);
        crop_top_left(gr[(size_t)(s0 + t) * 2 + 1], W, &x0, &wx);
        hit = (y == y0 || y == y0 + 1) && x0 + 1 >= x_lo && x0 < x_lo + tw;
      }
      unsigned long long m = __ballot(hit);
      while (m) {
        const int l = __builtin_ctzll(m);
        m &= m - 1;
        const int y0l = __builtin_amdgcn_readlane(y0, l);
        const int x0l = __builtin_amdgcn_readlane(x0, l);
        const float wyl = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(wy), l));
        const float wxl = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(wx), l));
        if (cok) row.add(y0l, wyl, x0l, wxl, go[s0 + l]);
      }
    }
  }
  __syncthreads();
  crop_row_store(acc, tw, nc, (size_t)H * W,
                 grad_in + (((size_t)b * C + c0) * H + y) * W + x_lo);
}

}  // namespace tlod

using namespace tlod;

extern "C" int tlod_roi_crop_fwd_f32(const float* x, int B, int C, int H, int W,
                                     const float* grid, int R, int gh, int gw, float* out,
                                     tlod_stream_t stream) {
  TLOD_CHECK_ARG(B > 0 && C > 0 && R > 0 && gh > 0 && gw > 0, "bad shape (sizes must be positive)");
  TLOD_CHECK_ARG(H >= 2 && W >= 2, "bad shape (the map needs H >= 2 and W >= 2)");
  TLOD_CHECK_ARG(R % B == 0, "R % B != 0 (the sampler maps grid r to image r / (R / B))");
  TLOD_CHECK_ARG(x != nullptr && grid != nullptr && out != nullptr, "null pointer");
  TLOD_CHECK_ARG((size_t)H * W < (1u << 30), "feature map too large");
  const long total = (long)R * C * gh * gw;
  const int blocks = (int)std::min<long>((total + 255) / 256, 256 * 64);
  hipLaunchKernelGGL(roi_crop_fwd_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, total,
                     x, C, H, W, grid, R / B, gh, gw, out);
  TLOD_LAUNCH_CHECK();
  return kOk;
}

extern "C" int tlod_roi_crop_bwd_f32(const float* grad_out, const float* grid, int R, int C,
                                     int gh, int gw, int B, int H, int W, float* grad_in,
                                     tlod_stream_t stream) {
  TLOD_CHECK_ARG(B > 0 && C > 0 && R > 0 && gh > 0 && gw > 0, "bad shape (sizes must be positive)");
  TLOD_CHECK_ARG(H >= 2 && W >= 2, "bad shape (the map needs H >= 2 and W >= 2)");
  TLOD_CHECK_ARG(R % B == 0, "R % B != 0 (the sampler maps grid r to image r / (R / B))");
  TLOD_CHECK_ARG(grad_out != nullptr && grid != nullptr && grad_in != nullptr, "null pointer");
  TLOD_CHECK_ARG((size_t)H * W < (1u << 30) && B <= 65535 && div_up(C, kCbCh) <= 65535,
                 "feature map too large");
  hipLaunchKernelGGL(roi_crop_bwd_kernel, dim3(H * div_up(W, kCbTw), div_up(C, kCbCh), B),
                     dim3(kCbCh), 0, (hipStream_t)stream, grad_out, grid, R / B, C, gh, gw, H, W,
                     grad_in);
  TLOD_LAUNCH_CHECK();
  return kOk;
}

extern "C" int tlod_roi_crop_pool_fwd_f32(const float* x, int B, int C, int H, int W,
                                          const float* rois, int R, int P, float spatial_scale,
                                          int max_pool, float* out, uint8_t* argmax,
                                          tlod_stream_t stream) {
  TLOD_CHECK_ARG(B > 0 && C > 0 && R >= 0 && P > 0, "bad shape (sizes must be positive)");
  TLOD_CHECK_ARG(H >= 2 && W >= 2, "bad shape (the map needs H >= 2 and W >= 2)");
  TLOD_CHECK_ARG((max_pool ? 2 * P : P) <= kCropMaxG, "at most 32 samples per axis");
  TLOD_CHECK_ARG((size_t)H * W < (1u << 30) && div_up(C, kCropCh) <= 65535,
                 "feature map too large");
  if (R == 0) return kOk;
  TLOD_CHECK_ARG(x != nullptr && rois != nullptr && out != nullptr, "null pointer");
  TLOD_CHECK_ARG(!max_pool || argmax != nullptr, "null pointer (argmax, needed with max_pool)");
  hipLaunchKernelGGL(roi_crop_pool_fwd_kernel, dim3(R, div_up(C, kCropCh)), dim3(kCropThreads), 0,
                     (hipStream_t)stream, x, B, C, H, W, rois, P, spatial_scale, max_pool ? 1 : 0,
                     out, argmax);
  TLOD_LAUNCH_CHECK();
  return kOk;
}

extern "C" int tlod_roi_crop_pool_bwd_f32(const float* grad_out, const uint8_t* argmax, int B,
                                          int C, int H, int W, const float* rois, int R, int P,
                                          float spatial_scale, int max_pool, float* grad_in,
                                          tlod_stream_t stream) {
  TLOD_CHECK_ARG(B > 0 && C > 0 && R >= 0 && P > 0, "bad shape (sizes must be positive)");
  TLOD_CHECK_ARG(H >= 2 && W >= 2, "bad shape (the map needs H >= 2 and W >= 2)");
  TLOD_CHECK_ARG((max_pool ? 2 * P : P) <= kCropMaxG, "at most 32 samples per axis");
  TLOD_CHECK_ARG((size_t)H * W < (1u << 30) && B <= 65535 && div_up(C, kCbCh) <= 65535,
                 "feature map too large");
  TLOD_CHECK_ARG(grad_in != nullptr, "null pointer");
  TLOD_CHECK_ARG(R == 0 || (grad_out != nullptr && rois != nullptr), "null pointer");
  TLOD_CHECK_ARG(R == 0 || !max_pool || argmax != nullptr,
                 "null pointer (argmax, needed with max_pool)");
  hipLaunchKernelGGL(roi_crop_pool_bwd_kernel, dim3(H * div_up(W, kCbTw), div_up(C, kCbCh), B),
                     dim3(kCbCh), 0, (hipStream_t)stream, grad_out, argmax, rois, R, B, C, H, W, P,
                     spatial_scale, max_pool ? 1 : 0, grad_in);
  TLOD_LAUNCH_CHECK();
  return kOk;
}
