// Fused clip_gradient + SGD(momentum) over all trainable parameters.
//
// Replaces clip_gradient (lib/model/utils/net_utils.py:38-49: a Python loop of per-param
// .norm() and a .item() host sync, then a second loop of p.grad.mul_) followed by
// torch.optim.SGD (methods/DAF/DAF_train.py:406-408).  Three stream-ordered launches, no
// host sync, deterministic (fixed-order reductions):
//   0. (data parallel) g = grad_scale * G, G the all-reduced gradient sum (applied as read);
//   1. per-chunk sum of squares of the gradients;
//   2. one workgroup: total = sqrt(sum), scale = clip / max(total, clip);
//   3. per chunk: g' = scale*g; d = g' + wd*p; buf = m*buf + d; p -= lr*buf.
// HBM traffic: read g twice, read+write p and buf once: 6 x 4 B per parameter.
//
// tlod_sgd_clip_pack_f32: the 3x3 conv weights are updated by 32 x 32-channel tiles that also
// store the new weights' split-bf16 packs (the forward and input-gradient operand layouts of
// the conv kernels), so no pack launch runs between the step and the next forward: +6.7 B
// written per weight element and pack instead of a separate pass that re-reads the weight.
//
// tlod_adam_clip_pack_f32: the same step with torch.optim.Adam's update (defaults: L2 weight
// decay, no amsgrad) in place of SGD's.  Launches 1 and 2 are shared; launch 2 also advances
// each live parameter's device-side step count and writes its two bias corrections, which
// the chunk / tile rows read through a pointer (nothing step-dependent is baked into the
// cached tables).  HBM traffic: read g twice, read+write p, m and v once: 8 x 4 B per
// parameter.
#include <cmath>

#include "common.h"
#include "bs_common.h"
#include "tlod.h"

#ifndef TLOD_SGD_NT
#define TLOD_SGD_NT 1
#endif

namespace tlod {

static_assert(sizeof(tlod_sgd_chunk) == 48, "descriptor layout (tlod/optim.py _DESC)");
static_assert(sizeof(tlod_sgd_pack_tile) == 96, "descriptor layout (tlod/optim.py _TILE)");
static_assert(sizeof(tlod_adam_chunk) == 64, "descriptor layout (tlod/optim.py _ADAM_DESC)");
static_assert(sizeof(tlod_adam_pack_tile) == 104, "descriptor layout (tlod/optim.py _ADAM_TILE)");
static_assert(sizeof(tlod_adam_state) == 24, "descriptor layout (tlod/optim.py _ADAM_STATE)");

// 16-B vector path when the chunk's pointers are 16-B aligned and its count a multiple of
// 4 (the grads can be views into the DP reducer's flat buckets at any float offset).
__device__ __forceinline__ bool vec4_ok(const void* a, const void* b, const void* c,
                                        long long n, const void* d = nullptr) {
  return ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b) |
           reinterpret_cast<uintptr_t>(c) | reinterpret_cast<uintptr_t>(d)) & 15) == 0 &&
         (n & 3) == 0;
}

// One workgroup's fixed-order sum of squares of (gs * grad[0, count)) -> *partial.
__device__ __forceinline__ void chunk_sumsq(const float* __restrict__ grad, long long count,
                                            float gs, float* __restrict__ partial) {
  float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
  if (vec4_ok(grad, grad, grad, count)) {
    typedef float v4 __attribute__((ext_vector_type(4)));
    const v4* g4 = reinterpret_cast<const v4*>(grad);
    const long long n4 = count / 4;
#pragma unroll 4
    for (long long i = threadIdx.x; i < n4; i += 256) {
      v4 g = g4[i];  // (a plain load: the update pass re-reads g, partly from the MALL)
      g *= gs;
      s0 += g.x * g.x; s1 += g.y * g.y; s2 += g.z * g.z; s3 += g.w * g.w;
    }
  } else {
    for (long long i = threadIdx.x; i < count; i += 256) {
      const float g = grad[i] * gs;
      s0 += g * g;
    }
  }
  float s = (s0 + s1) + (s2 + s3);
  for (int o = 32; o > 0; o >>= 1) s += __shfl_down(s, o);
  __shared__ float ws[4];
  if ((threadIdx.x & 63) == 0) ws[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) *partial = (ws[0] + ws[1]) + (ws[2] + ws[3]);
}

__global__ void __launch_bounds__(256) sgd_sumsq_kernel(const tlod_sgd_chunk* __restrict__ chunks,
                                                        float gs, float* __restrict__ partials) {
  const tlod_sgd_chunk c = chunks[blockIdx.x];
  // (a negative count: a norm-only row, see tlod_sgd_chunk)
  chunk_sumsq(c.grad, c.count < 0 ? -c.count : c.count, gs, partials + blockIdx.x);
}

__global__ void __launch_bounds__(256) adam_sumsq_kernel(const tlod_adam_chunk* __restrict__ chunks,
                                                         float gs, float* __restrict__ partials) {
  const tlod_adam_chunk c = chunks[blockIdx.x];
  chunk_sumsq(c.grad, c.count < 0 ? -c.count : c.count, gs, partials + blockIdx.x);
}

// One workgroup: out[0] = sqrt(sum of the partials), out[1] = the clip scale.
__device__ __forceinline__ void grad_norm(const float* __restrict__ partials, int n, float clip,
                                          float* __restrict__ out) {
  __shared__ double ws[256];
  double s = 0.0;
  for (int i = threadIdx.x; i < n; i += 256) s += (double)partials[i];
  ws[threadIdx.x] = s;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (threadIdx.x < o) ws[threadIdx.x] += ws[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const float total = (float)sqrt(ws[0]);
    out[0] = total;
    out[1] = clip > 0.f ? clip / fmaxf(total, clip) : 1.f;  // net_utils.py:46
  }
}

__global__ void __launch_bounds__(256) sgd_norm_kernel(const float* __restrict__ partials, int n,
                                                       float clip, float* __restrict__ out) {
  grad_norm(partials, n, clip, out);
}

// The norm launch of the Adam step also advances the step count of every live parameter
// (one table row per parameter, so no two threads touch one count) and writes the bias
// corrections of its new count: corr = {1 / (1 - b1^t), 1 / sqrt(1 - b2^t)}, in double.
__global__ void __launch_bounds__(256) adam_norm_step_kernel(
    const float* __restrict__ partials, int n, float clip, float* __restrict__ out,
    const tlod_adam_state* __restrict__ states, int n_states, double b1, double b2) {
  grad_norm(partials, n, clip, out);
  for (int i = threadIdx.x; i < n_states; i += 256) {
    const tlod_adam_state st = states[i];
    if (st.active != nullptr && *st.active == 0.f) continue;  // no rank produced its gradient
    const int t = *st.step + 1;
    *st.step = t;
    st.corr[0] = (float)(1.0 / (1.0 - pow(b1, (double)t)));
    st.corr[1] = (float)(1.0 / sqrt(1.0 - pow(b2, (double)t)));
  }
}

__device__ __forceinline__ void sgd1(float g, float& p, float& b, float gs, float scale,
                                     float wd, float lr, float momentum) {
  const float d = (g * gs) * scale + wd * p;
  b = momentum * b + d;
  p = p - lr * b;
}

__global__ void __launch_bounds__(256) sgd_update_kernel(const tlod_sgd_chunk* __restrict__ chunks,
                                                         const float* __restrict__ norm_scale,
                                                         float gs, float momentum) {
  const tlod_sgd_chunk c = chunks[blockIdx.x];
  if (c.count < 0) return;  // norm-only row: a pack tile updates these elements
  if (c.active != nullptr && *c.active == 0.f) return;  // no rank produced this gradient
  const float scale = norm_scale[1];
  if (vec4_ok(c.grad, c.param, c.momentum_buf, c.count)) {
    const long long n4 = c.count / 4;
#if TLOD_SGD_NT
    // streaming: every element is touched once per step, ~15 ms and >10 GB of other traffic
    // apart, so the loads and stores bypass the caches' retention (nontemporal)
    typedef float v4 __attribute__((ext_vector_type(4)));
    const v4* gv = reinterpret_cast<const v4*>(c.grad);
    v4* pv = reinterpret_cast<v4*>(c.param);
    v4* bv = reinterpret_cast<v4*>(c.momentum_buf);
#pragma unroll 4
    for (long long i = threadIdx.x; i < n4; i += 256) {
      const v4 g = __builtin_nontemporal_load(gv + i);
      v4 p = __builtin_nontemporal_load(pv + i), b = __builtin_nontemporal_load(bv + i);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        float pe = p[e], be = b[e];
        sgd1(g[e], pe, be, gs, scale, c.weight_decay, c.lr, momentum);
        p[e] = pe;
        b[e] = be;
      }
      __builtin_nontemporal_store(b, bv + i);
      __builtin_nontemporal_store(p, pv + i);
    }
#else
    const float4* __restrict__ g4 = reinterpret_cast<const float4*>(c.grad);
    float4* __restrict__ p4 = reinterpret_cast<float4*>(c.param);
    float4* __restrict__ b4 = reinterpret_cast<float4*>(c.momentum_buf);
#pragma unroll 2
    for (long long i = threadIdx.x; i < n4; i += 256) {
      const float4 g = g4[i];
      float4 p = p4[i], b = b4[i];
      sgd1(g.x, p.x, b.x, gs, scale, c.weight_decay, c.lr, momentum);
      sgd1(g.y, p.y, b.y, gs, scale, c.weight_decay, c.lr, momentum);
      sgd1(g.z, p.z, b.z, gs, scale, c.weight_decay, c.lr, momentum);
      sgd1(g.w, p.w, b.w, gs, scale, c.weight_decay, c.lr, momentum);
      b4[i] = b;
      p4[i] = p;
    }
#endif
    return;
  }
  for (long long i = threadIdx.x; i < c.count; i += 256) {
    float p = c.param[i], b = c.momentum_buf[i];
    sgd1(c.grad[i], p, b, gs, scale, c.weight_decay, c.lr, momentum);
    c.momentum_buf[i] = b;
    c.param[i] = p;
  }
}

// torch.optim.Adam's update of one element (L2 weight decay, no amsgrad), in product form:
// step = lr / (1 - b1^t) and c2 = 1 / sqrt(1 - b2^t) come from the parameter's corr pair.
struct AdamK {
  float b1, omb1, b2, omb2, eps;  // omb = 1 - beta, rounded once from double
};

__device__ __forceinline__ void adam1(float g, float& p, float& m, float& v, float gs,
                                      float scale, float wd, float step, float c2,
                                      const AdamK& k) {
  const float d = (g * gs) * scale + wd * p;
  m = k.b1 * m + k.omb1 * d;
  v = k.b2 * v + k.omb2 * d * d;
  p = p - step * (m / (sqrtf(v) * c2 + k.eps));
}

__global__ void __launch_bounds__(256) adam_update_kernel(const tlod_adam_chunk* __restrict__ chunks,
                                                          const float* __restrict__ norm_scale,
                                                          float gs, AdamK k) {
  const tlod_adam_chunk c = chunks[blockIdx.x];
  if (c.count < 0) return;  // norm-only row: a pack tile updates these elements
  if (c.active != nullptr && *c.active == 0.f) return;  // no rank produced this gradient
  const float scale = norm_scale[1];
  const float step = c.lr * c.corr[0], c2 = c.corr[1];
  if (vec4_ok(c.grad, c.param, c.exp_avg, c.count, c.exp_avg_sq)) {
    // streaming, as sgd_update_kernel: every element is touched once per step
    typedef float v4 __attribute__((ext_vector_type(4)));
    const long long n4 = c.count / 4;
    const v4* gv = reinterpret_cast<const v4*>(c.grad);
    v4* pv = reinterpret_cast<v4*>(c.param);
    v4* mv = reinterpret_cast<v4*>(c.exp_avg);
    v4* vv = reinterpret_cast<v4*>(c.exp_avg_sq);
#pragma unroll 2
    for (long long i = threadIdx.x; i < n4; i += 256) {
      const v4 g = __builtin_nontemporal_load(gv + i);
      v4 p = __builtin_nontemporal_load(pv + i), m = __builtin_nontemporal_load(mv + i),
         v = __builtin_nontemporal_load(vv + i);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        float pe = p[e], me = m[e], ve = v[e];
        adam1(g[e], pe, me, ve, gs, scale, c.weight_decay, step, c2, k);
        p[e] = pe;
        m[e] = me;
        v[e] = ve;
      }
      __builtin_nontemporal_store(m, mv + i);
      __builtin_nontemporal_store(v, vv + i);
      __builtin_nontemporal_store(p, pv + i);
    }
    return;
  }
  for (long long i = threadIdx.x; i < c.count; i += 256) {
    float p = c.param[i], m = c.exp_avg[i], v = c.exp_avg_sq[i];
    adam1(c.grad[i], p, m, v, gs, scale, c.weight_decay, step, c2, k);
    c.exp_avg[i] = m;
    c.exp_avg_sq[i] = v;
    c.param[i] = p;
  }
}


// One tile of a (cout, cin, 3, 3) weight: 32 output x 32 input channels x 9 taps.  The update
// is the one sgd_update_kernel applies; the updated tile is kept in LDS ([o][ci * 9 + tap],
// 289-float rows) and written out as the packed units of pack_bs_kernel (conv.hip): forward
// unit (o, chunk, tap) = 8 input channels, input-gradient unit (ci, chunk, 8 - tap) = 8
// output channels, 3 bf16 planes of 16 B each.  Zero padding of the packs (tap slot 9,
// channels past the last) is never rewritten; lanes past the last channel store zeros.
constexpr int kPT = 32;
constexpr int kPTRow = kPT * 9 + 1;

__device__ __forceinline__ void store_units(unsigned short* P, size_t plane, size_t off,
                                            const float (&v)[8]) {
  u32x4 sp[3];
  split8<3>(v, sp);
#pragma unroll
  for (int pl = 0; pl < 3; ++pl) *reinterpret_cast<u32x4*>(P + pl * plane + off) = sp[pl];
}

// The pack-writing half of a tile kernel (Tile: tlod_sgd_pack_tile or tlod_adam_pack_tile):
// w holds the updated tile, no x ni its live output x input channels.
template <class Tile>
__device__ __forceinline__ void store_tile_packs(const Tile& t, const float* w, int no, int ni) {
  if (t.pack_fwd != nullptr) {
    const int rowlen = ((t.cin + 7) / 8) * kBsKP, ncl = ((ni + 7) / 8);
    const size_t plane = (size_t)t.cout * rowlen;
    for (int u = threadIdx.x; u < kPT * 4 * 9; u += 256) {
      const int s = u % 9, r = u / 9, cl = r & 3, ol = r >> 2;
      if (ol >= no || cl >= ncl) continue;
      float v[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) v[e] = w[ol * kPTRow + (cl * 8 + e) * 9 + s];
      store_units(t.pack_fwd, plane,
                  (size_t)(t.o0 + ol) * rowlen + (size_t)(t.i0 / 8 + cl) * kBsKP + s * 8, v);
    }
  }
  if (t.pack_dgrad != nullptr || t.pack_dgrad_scaled != nullptr) {
    const int rowlen = ((t.cout + 7) / 8) * kBsKP, nocl = ((no + 7) / 8);
    const size_t plane = (size_t)t.cin * rowlen;
    for (int u = threadIdx.x; u < kPT * 4 * 9; u += 256) {
      const int s = u % 9, r = u / 9, ocl = r & 3, il = r >> 2;
      if (il >= ni || ocl >= nocl) continue;
      float v[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) v[e] = w[(ocl * 8 + e) * kPTRow + il * 9 + (8 - s)];
      const size_t off = (size_t)(t.i0 + il) * rowlen + (size_t)(t.o0 / 8 + ocl) * kBsKP + s * 8;
      if (t.pack_dgrad != nullptr) store_units(t.pack_dgrad, plane, off, v);
      if (t.pack_dgrad_scaled != nullptr) {
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const int o = t.o0 + ocl * 8 + e;
          if (o < t.cout) v[e] *= t.scale[o];
        }
        store_units(t.pack_dgrad_scaled, plane, off, v);
      }
    }
  }
}

__global__ void __launch_bounds__(256) sgd_pack_kernel(const tlod_sgd_pack_tile* __restrict__ tiles,
                                                       const float* __restrict__ norm_scale,
                                                       float gs, float momentum) {
  const tlod_sgd_pack_tile t = tiles[blockIdx.x];
  if (t.active != nullptr && *t.active == 0.f) return;
  __shared__ float w[kPT * kPTRow];
  const float scale = norm_scale[1];
  const int no = min(kPT, t.cout - t.o0), ni = min(kPT, t.cin - t.i0);
  const int seg = ni * 9;  // contiguous elements of one output channel inside the tile
#pragma unroll 4
  for (int idx = threadIdx.x; idx < kPT * kPT * 9; idx += 256) {
    const int ol = idx / (kPT * 9), j = idx - ol * (kPT * 9);
    float pv = 0.f;
    if (ol < no && j < seg) {
      const size_t e = ((size_t)(t.o0 + ol) * t.cin + t.i0) * 9 + j;
      const float g = __builtin_nontemporal_load(t.grad + e);
      float p = __builtin_nontemporal_load(t.param + e);
      float b = __builtin_nontemporal_load(t.momentum_buf + e);
      sgd1(g, p, b, gs, scale, t.weight_decay, t.lr, momentum);
      __builtin_nontemporal_store(b, t.momentum_buf + e);
      __builtin_nontemporal_store(p, t.param + e);
      pv = p;
    }
    w[ol * kPTRow + j] = pv;
  }
  __syncthreads();
  store_tile_packs(t, w, no, ni);
}

// sgd_pack_kernel with the Adam update (adam1, so a tile-updated weight is bit-identical to a
// chunk-updated one).
__global__ void __launch_bounds__(256) adam_pack_kernel(const tlod_adam_pack_tile* __restrict__ tiles,
                                                        const float* __restrict__ norm_scale,
                                                        float gs, AdamK k) {
  const tlod_adam_pack_tile t = tiles[blockIdx.x];
  if (t.active != nullptr && *t.active == 0.f) return;
  __shared__ float w[kPT * kPTRow];
  const float scale = norm_scale[1];
  const float step = t.lr * t.corr[0], c2 = t.corr[1];
  const int no = min(kPT, t.cout - t.o0), ni = min(kPT, t.cin - t.i0);
  const int seg = ni * 9;  // contiguous elements of one output channel inside the tile
#pragma unroll 4
  for (int idx = threadIdx.x; idx < kPT * kPT * 9; idx += 256) {
    const int ol = idx / (kPT * 9), j = idx - ol * (kPT * 9);
    float pv = 0.f;
    if (ol < no && j < seg) {
      const size_t e = ((size_t)(t.o0 + ol) * t.cin + t.i0) * 9 + j;
      const float g = __builtin_nontemporal_load(t.grad + e);
      float p = __builtin_nontemporal_load(t.param + e);
      float m = __builtin_nontemporal_load(t.exp_avg + e);
      float v = __builtin_nontemporal_load(t.exp_avg_sq + e);
      adam1(g, p, m, v, gs, scale, t.weight_decay, step, c2, k);
      __builtin_nontemporal_store(m, t.exp_avg + e);
      __builtin_nontemporal_store(v, t.exp_avg_sq + e);
      __builtin_nontemporal_store(p, t.param + e);
      pv = p;
    }
    w[ol * kPTRow + j] = pv;
  }
  __syncthreads();
  store_tile_packs(t, w, no, ni);
}

}  // namespace tlod

using namespace tlod;

extern "C" int tlod_sgd_clip_pack_f32(const tlod_sgd_chunk* chunks, int n_chunks, int n_update,
                                      const tlod_sgd_pack_tile* tiles, int n_tiles,
                                      float grad_scale, float momentum, float clip_norm,
                                      float* partials, float* norm_scale, tlod_stream_t stream) {
  TLOD_CHECK_ARG(n_chunks > 0 && chunks && partials && norm_scale, "bad arguments");
  TLOD_CHECK_ARG(n_update >= 0 && n_update <= n_chunks && n_tiles >= 0 && (n_tiles == 0 || tiles),
                 "bad update / tile counts");
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(sgd_sumsq_kernel, dim3(n_chunks), dim3(256), 0, s, chunks, grad_scale, partials);
  TLOD_LAUNCH_CHECK();
  hipLaunchKernelGGL(sgd_norm_kernel, dim3(1), dim3(256), 0, s, partials, n_chunks, clip_norm,
                     norm_scale);
  TLOD_LAUNCH_CHECK();
  if (n_update > 0) {
    hipLaunchKernelGGL(sgd_update_kernel, dim3(n_update), dim3(256), 0, s, chunks, norm_scale,
                       grad_scale, momentum);
    TLOD_LAUNCH_CHECK();
  }
  if (n_tiles > 0) {
    hipLaunchKernelGGL(sgd_pack_kernel, dim3(n_tiles), dim3(256), 0, s, tiles, norm_scale,
                       grad_scale, momentum);
    TLOD_LAUNCH_CHECK();
  }
  return kOk;
}

extern "C" int tlod_sgd_clip_f32(const tlod_sgd_chunk* chunks, int n_chunks, float grad_scale,
                                 float momentum, float clip_norm, float* partials,
                                 float* norm_scale, tlod_stream_t stream) {
  return tlod_sgd_clip_pack_f32(chunks, n_chunks, n_chunks, nullptr, 0, grad_scale, momentum,
                                clip_norm, partials, norm_scale, stream);
}

extern "C" int tlod_adam_clip_pack_f32(const tlod_adam_chunk* chunks, int n_chunks, int n_update,
                                       const tlod_adam_pack_tile* tiles, int n_tiles,
                                       const tlod_adam_state* states, int n_states,
                                       float grad_scale, double beta1, double beta2, double eps,
                                       float clip_norm, float* partials, float* norm_scale,
                                       tlod_stream_t stream) {
  TLOD_CHECK_ARG(chunks && states && partials && norm_scale, "null table or buffer");
  TLOD_CHECK_ARG(n_chunks > 0 && n_update >= 0 && n_update <= n_chunks && n_tiles >= 0 &&
                     (n_tiles == 0 || tiles) && n_states > 0,
                 "bad update / tile / state counts");
  TLOD_CHECK_ARG(beta1 >= 0.0 && beta1 < 1.0 && beta2 >= 0.0 && beta2 < 1.0,
                 "beta outside [0, 1)");
  TLOD_CHECK_ARG(eps > 0.0, "eps must be > 0");
  const AdamK k = {(float)beta1, (float)(1.0 - beta1), (float)beta2, (float)(1.0 - beta2),
                   (float)eps};
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(adam_sumsq_kernel, dim3(n_chunks), dim3(256), 0, s, chunks, grad_scale,
                     partials);
  TLOD_LAUNCH_CHECK();
  hipLaunchKernelGGL(adam_norm_step_kernel, dim3(1), dim3(256), 0, s, partials, n_chunks,
                     clip_norm, norm_scale, states, n_states, beta1, beta2);
  TLOD_LAUNCH_CHECK();
  if (n_update > 0) {
    hipLaunchKernelGGL(adam_update_kernel, dim3(n_update), dim3(256), 0, s, chunks, norm_scale,
                       grad_scale, k);
    TLOD_LAUNCH_CHECK();
  }
  if (n_tiles > 0) {
    hipLaunchKernelGGL(adam_pack_kernel, dim3(n_tiles), dim3(256), 0, s, tiles, norm_scale,
                       grad_scale, k);
    TLOD_LAUNCH_CHECK();
  }
  return kOk;
}

extern "C" int tlod_adam_clip_f32(const tlod_adam_chunk* chunks, int n_chunks,
                                  const tlod_adam_state* states, int n_states, float grad_scale,
                                  double beta1, double beta2, double eps, float clip_norm,
                                  float* partials, float* norm_scale, tlod_stream_t stream) {
  return tlod_adam_clip_pack_f32(chunks, n_chunks, n_chunks, nullptr, 0, states, n_states,
                                 grad_scale, beta1, beta2, eps, clip_norm, partials, norm_scale,
                                 stream);
}
