// RPN proposal layer on device: decode + clip -> stable descending sort -> top pre_nms
// -> NMS -> top post_nms -> zero-padded rois.  Replaces _ProposalLayer.forward
// (lib/model/rpn/proposal_layer.py:49-161), which builds anchors with numpy on the host,
// sorts with torch, loops over images in Python and round-trips NMS through the host.
//
// Float semantics: bbox_transform_inv (lib/model/rpn/bbox_transform.py:77-103) and
// clip_boxes (:125-133), one rounding per op (-ffp-contract=off), expf from ocml.
#include <hipcub/hipcub.hpp>

#include "common.h"
#include "nms_impl.h"
#include "tlod.h"
#include "tlod_pa_atf.h"

namespace tlod {

// One thread per anchor of image `img`: idx = (h*W + w)*A + a (proposal_layer.py:90-103).
__global__ void proposal_decode_kernel(const float* __restrict__ cls_prob,
                                       const float* __restrict__ deltas,
                                       const float* __restrict__ im_info,
                                       const float* __restrict__ base_anchors, int img, int A,
                                       int H, int W, int stride, float* __restrict__ scores,
                                       int32_t* __restrict__ ids, float4* __restrict__ props,
                                       float* __restrict__ props_out) {
  const int N = H * W * A;
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= N) return;
  const int a = idx % A;
  const int hw = idx / A;
  const int w = hw % W, h = hw / W;
  const size_t HW = (size_t)H * W;
  const float sx = (float)(w * stride), sy = (float)(h * stride);
  const float x1 = base_anchors[a * 4 + 0] + sx, y1 = base_anchors[a * 4 + 1] + sy;
  const float x2 = base_anchors[a * 4 + 2] + sx, y2 = base_anchors[a * 4 + 3] + sy;
  const float* d = deltas + ((size_t)img * 4 * A + 4 * a) * HW + hw;
  const float dx = d[0], dy = d[HW], dw = d[2 * HW], dh = d[3 * HW];
  const float widths = x2 - x1 + 1.0f, heights = y2 - y1 + 1.0f;
  const float cx = x1 + 0.5f * widths, cy = y1 + 0.5f * heights;
  const float pcx = dx * widths + cx, pcy = dy * heights + cy;
  const float pw = expf(dw) * widths, ph = expf(dh) * heights;
  const float imh = im_info[img * 3 + 0], imw = im_info[img * 3 + 1];
  const float xm = imw - 1.f, ym = imh - 1.f;
  float4 p;
  p.x = fminf(fmaxf(pcx - 0.5f * pw, 0.f), xm);
  p.y = fminf(fmaxf(pcy - 0.5f * ph, 0.f), ym);
  p.z = fminf(fmaxf(pcx + 0.5f * pw, 0.f), xm);
  p.w = fminf(fmaxf(pcy + 0.5f * ph, 0.f), ym);
  props[idx] = p;
  if (props_out) reinterpret_cast<float4*>(props_out)[(size_t)img * N + idx] = p;
  scores[idx] = cls_prob[((size_t)img * 2 * A + A + a) * HW + hw];
  ids[idx] = idx;
}

__global__ void gather_sorted_kernel(const float4* __restrict__ props,
                                     const int32_t* __restrict__ order, int n,
                                     float4* __restrict__ dets) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) dets[i] = props[order[i]];
}

// rois_out[img] = (img, box) for kept, zero padding after (proposal_layer.py:154-159).
__global__ void write_rois_kernel(const float4* __restrict__ dets, const int32_t* __restrict__ keep,
                                  const int32_t* __restrict__ num_keep, int img, int post,
                                  float* __restrict__ rois) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= post) return;
  float* o = rois + ((size_t)img * post + j) * 5;
  o[0] = (float)img;
  if (j < *num_keep) {
    const float4 b = dets[keep[j]];
    o[1] = b.x; o[2] = b.y; o[3] = b.z; o[4] = b.w;
  } else {
    o[1] = 0.f; o[2] = 0.f; o[3] = 0.f; o[4] = 0.f;
  }
}

struct ProposalWs {
  float* scores; float* scores_sorted; int32_t* ids; int32_t* ids_sorted;
  float4* props; float4* dets; int32_t* keep; int32_t* num_keep;
  void* cub_tmp; size_t cub_bytes; void* nms_ws; size_t nms_bytes;
};

static size_t cub_sort_bytes(int N) {
  size_t bytes = 0;
  (void)hipcub::DeviceRadixSort::SortPairsDescending(nullptr, bytes, (const float*)nullptr,
                                               (float*)nullptr, (const int32_t*)nullptr,
                                               (int32_t*)nullptr, N);
  return bytes;
}

static size_t carve_proposal(Carve& c, ProposalWs& w, int A, int H, int W, int pre_nms) {
  const int N = H * W * A;
  const int n_top = (pre_nms > 0 && pre_nms < N) ? pre_nms : N;
  w.scores = c.take<float>(N);
  w.scores_sorted = c.take<float>(N);
  w.ids = c.take<int32_t>(N);
  w.ids_sorted = c.take<int32_t>(N);
  w.props = c.take<float4>(N);
  w.dets = c.take<float4>(n_top);
  w.keep = c.take<int32_t>(n_top);
  w.num_keep = c.take<int32_t>(1);
  w.cub_bytes = cub_sort_bytes(N);
  w.cub_tmp = c.take<char>(w.cub_bytes);
  w.nms_bytes = nms_ws_bytes(n_top);
  w.nms_ws = c.take<char>(w.nms_bytes);
  return align_up(c.off, 256);
}

}  // namespace tlod

using namespace tlod;

extern "C" size_t tlod_proposal_workspace_bytes(int B, int A, int H, int W, int pre_nms) {
  (void)B;
  Carve c(nullptr, 0);
  ProposalWs w;
  return carve_proposal(c, w, A, H, W, pre_nms);
}

extern "C" int tlod_proposal_f32(const float* cls_prob, const float* bbox_deltas,
                                 const float* im_info, const float* base_anchors, int B, int A,
                                 int H, int W, int feat_stride, int pre_nms, int post_nms,
                                 float nms_thresh, float* rois_out, float* props_out, void* ws,
                                 size_t ws_bytes, tlod_stream_t stream) {
  TLOD_CHECK_ARG(B > 0 && A > 0 && H > 0 && W > 0 && post_nms > 0, "bad shape");
  hipStream_t s = (hipStream_t)stream;
  Carve c(ws, ws_bytes);
  ProposalWs w;
  carve_proposal(c, w, A, H, W, pre_nms);
  if (!c.ok()) {
    set_error("tlod_proposal_f32: workspace too small");
    return kWorkspace;
  }
  const int N = H * W * A;
  // proposal_layer.py:134: pre_nms_topN compared against numel over the whole batch.
  const int n_top = (pre_nms > 0 && pre_nms < B * N) ? std::min(pre_nms, N) : N;
  for (int img = 0; img < B; ++img) {
    hipLaunchKernelGGL(proposal_decode_kernel, dim3(div_up(N, 256)), dim3(256), 0, s, cls_prob,
                       bbox_deltas, im_info, base_anchors, img, A, H, W, feat_stride, w.scores,
                       w.ids, w.props, props_out);
    TLOD_LAUNCH_CHECK();
    size_t cb = w.cub_bytes;
    TLOD_HIP(hipcub::DeviceRadixSort::SortPairsDescending(w.cub_tmp, cb, w.scores,
                                                          w.scores_sorted, w.ids, w.ids_sorted,
                                                          N, 0, 32, s));
    hipLaunchKernelGGL(gather_sorted_kernel, dim3(div_up(n_top, 256)), dim3(256), 0, s, w.props,
                       w.ids_sorted, n_top, w.dets);
    TLOD_LAUNCH_CHECK();
    int st = nms_launch(reinterpret_cast<const float*>(w.dets), n_top, 4, nms_thresh, post_nms,
                        w.keep, w.num_keep, w.nms_ws, w.nms_bytes, s);
    if (st != kOk) return st;
    hipLaunchKernelGGL(write_rois_kernel, dim3(div_up(post_nms, 256)), dim3(256), 0, s, w.dets,
                       w.keep, w.num_keep, img, post_nms, rois_out);
    TLOD_LAUNCH_CHECK();
  }
  return kOk;
}

// ------------------------------------------------------------------ PA-ATF's subsampled form
// lib/PA_ATF/proposal_layer1.py:152-160: for cfg_key != 'TRAIN' the NMS survivors are not
// truncated — the first int(post * 0.25) stay and min(len(rest), int(post * 0.75)) of the rest
// are drawn without replacement.  Two phases, like the anchor and proposal targets, so a test
// can replay the draws: keep (every survivor, in score order, with its count), then pick.
namespace tlod {
namespace {

constexpr int kPickThreads = 256;
constexpr int kPickTile = 2048;     // random keys staged in LDS per pass
constexpr int kPickMaxRows = 16384; // survivors per image the selection bitmask covers

// kept[img] = the survivors' boxes in score order, zeros after; counts[img] = how many.
__global__ void write_kept_kernel(const float4* __restrict__ dets,
                                  const int32_t* __restrict__ keep,
                                  const int32_t* __restrict__ num_keep, int img, int cap,
                                  float* __restrict__ kept, int32_t* __restrict__ counts) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= cap) return;
  const int n = min(*num_keep, cap);
  reinterpret_cast<float4*>(kept)[(size_t)img * cap + j] =
      j < n ? dets[keep[j]] : make_float4(0.f, 0.f, 0.f, 0.f);
  if (j == 0) counts[img] = n;
}

// One workgroup per image.  Rows [0, nh): the head; then the picked survivors; zeros after.
__global__ void __launch_bounds__(kPickThreads)
proposal_pick_kernel(const float* __restrict__ kept, const int32_t* __restrict__ counts, int cap,
                     int post, int head, const int32_t* __restrict__ pick,
                     const int32_t* __restrict__ pick_off, uint64_t seed,
                     float* __restrict__ rois) {
  __shared__ uint64_t keys[kPickTile];
  __shared__ uint64_t bits[kPickMaxRows / 64];  // bit r: survivor head + r is picked
  const int b = blockIdx.x, tid = threadIdx.x;
  const float4* __restrict__ src = reinterpret_cast<const float4*>(kept) + (size_t)b * cap;
  float* __restrict__ out = rois + (size_t)b * post * 5;
  const int count = min(max(counts[b], 0), cap);
  const int nh = min(count, head), n = count - nh;  // n: the survivors past the head
  int k = min(n, post - head);                      // rows appended after the head
  if (pick) k = min(k, max(pick_off[b + 1] - pick_off[b], 0));
  const int total = nh + k;
  for (int j = tid; j < post; j += kPickThreads) {
    float* o = out + (size_t)j * 5;
    o[0] = (float)b;
    if (j < nh) {
      const float4 v = src[j];
      o[1] = v.x; o[2] = v.y; o[3] = v.z; o[4] = v.w;
    } else if (j >= total) {
      o[1] = 0.f; o[2] = 0.f; o[3] = 0.f; o[4] = 0.f;
    }
  }
  if (k <= 0) return;  // workgroup-uniform
  if (pick) {  // explicit: survivor head + pick[...], in the given order (0 if out of range)
    const int32_t* __restrict__ p = pick + pick_off[b];
    for (int j = tid; j < k; j += kPickThreads) {
      const int r = p[j];
      const float4 v = (r >= 0 && r < n) ? src[head + r] : make_float4(0.f, 0.f, 0.f, 0.f);
      float* o = out + (size_t)(head + j) * 5;
      o[1] = v.x; o[2] = v.y; o[3] = v.z; o[4] = v.w;
    }
    return;
  }
  // device RNG: survivor r of the rest gets the key rng(seed, image, r); the k smallest keys
  // (ties by index) are a uniform k-subset, appended in ascending r
  for (int i = tid; i < kPickMaxRows / 64; i += kPickThreads) bits[i] = 0ull;
  __syncthreads();
  for (int r0 = 0; r0 < n; r0 += kPickThreads) {  // every thread takes part in the barriers
    const int r = r0 + tid;
    const uint64_t mine = r < n ? rng_u64(seed, (uint64_t)b, (uint64_t)r) : 0;
    int rank = 0;
    for (int t0 = 0; t0 < n; t0 += kPickTile) {
      const int tn = min(kPickTile, n - t0);
      for (int i = tid; i < tn; i += kPickThreads)
        keys[i] = rng_u64(seed, (uint64_t)b, (uint64_t)(t0 + i));
      __syncthreads();
      if (r < n)
        for (int i = 0; i < tn; ++i) {
          const uint64_t o = keys[i];
          rank += (o < mine || (o == mine && t0 + i < r)) ? 1 : 0;
        }
      __syncthreads();
    }
    const uint64_t picked = __ballot(r < n && rank < k);  // a wave is 64 consecutive r
    if ((tid & 63) == 0) bits[(r0 + tid) >> 6] = picked;
  }
  __syncthreads();
  for (int r = tid; r < n; r += kPickThreads) {
    if (!((bits[r >> 6] >> (r & 63)) & 1ull)) continue;
    int pos = __popcll(bits[r >> 6] & ((1ull << (r & 63)) - 1ull));
    for (int wd = 0; wd < (r >> 6); ++wd) pos += __popcll(bits[wd]);
    const float4 v = src[head + r];
    float* o = out + (size_t)(head + pos) * 5;
    o[1] = v.x; o[2] = v.y; o[3] = v.z; o[4] = v.w;
  }
}

int keep_cap(int A, int H, int W, int pre_nms) {
  const int N = H * W * A;
  return (pre_nms > 0 && pre_nms < N) ? pre_nms : N;
}

int launch_keep(const float* cls_prob, const float* bbox_deltas, const float* im_info,
                const float* base_anchors, int B, int A, int H, int W, int feat_stride,
                int pre_nms, float nms_thresh, float* kept, int32_t* counts, ProposalWs& w,
                hipStream_t s) {
  const int N = H * W * A, cap = keep_cap(A, H, W, pre_nms);
  const int n_top = (pre_nms > 0 && pre_nms < B * N) ? std::min(pre_nms, N) : N;  // == cap
  for (int img = 0; img < B; ++img) {
    hipLaunchKernelGGL(proposal_decode_kernel, dim3(div_up(N, 256)), dim3(256), 0, s, cls_prob,
                       bbox_deltas, im_info, base_anchors, img, A, H, W, feat_stride, w.scores,
                       w.ids, w.props, (float*)nullptr);
    TLOD_LAUNCH_CHECK();
    size_t cb = w.cub_bytes;
    TLOD_HIP(hipcub::DeviceRadixSort::SortPairsDescending(w.cub_tmp, cb, w.scores,
                                                          w.scores_sorted, w.ids, w.ids_sorted,
                                                          N, 0, 32, s));
    hipLaunchKernelGGL(gather_sorted_kernel, dim3(div_up(n_top, 256)), dim3(256), 0, s, w.props,
                       w.ids_sorted, n_top, w.dets);
    TLOD_LAUNCH_CHECK();
    int st = nms_launch(reinterpret_cast<const float*>(w.dets), n_top, 4, nms_thresh, n_top,
                        w.keep, w.num_keep, w.nms_ws, w.nms_bytes, s);
    if (st != kOk) return st;
    hipLaunchKernelGGL(write_kept_kernel, dim3(div_up(cap, 256)), dim3(256), 0, s, w.dets, w.keep,
                       w.num_keep, img, cap, kept, counts);
    TLOD_LAUNCH_CHECK();
  }
  return kOk;
}

int check_pick(const char* fn, int B, int cap, int post, int head) {
  if (!(B > 0 && cap > 0 && post > 0 && head >= 0 && head <= post)) {
    set_error(std::string(fn) + ": bad shape (0 <= head <= post)");
    return kInvalidArg;
  }
  if (cap > kPickMaxRows) {
    set_error(std::string(fn) + ": more than 16384 survivor rows per image");
    return kUnsupported;
  }
  return kOk;
}

size_t carve_subsample(Carve& c, ProposalWs& w, float** kept, int32_t** counts, int B, int A,
                       int H, int W, int pre_nms) {
  carve_proposal(c, w, A, H, W, pre_nms);
  *kept = c.take<float>((size_t)B * keep_cap(A, H, W, pre_nms) * 4);
  *counts = c.take<int32_t>(B);
  return align_up(c.off, 256);
}

}  // namespace
}  // namespace tlod

extern "C" int tlod_proposal_keep_f32(const float* cls_prob, const float* bbox_deltas,
                                      const float* im_info, const float* base_anchors, int B,
                                      int A, int H, int W, int feat_stride, int pre_nms,
                                      float nms_thresh, float* kept, int32_t* counts, void* ws,
                                      size_t ws_bytes, tlod_stream_t stream) {
  TLOD_CHECK_ARG(cls_prob && bbox_deltas && im_info && base_anchors && kept && counts,
                 "null pointer");
  TLOD_CHECK_ARG(B > 0 && A > 0 && H > 0 && W > 0, "bad shape");
  Carve c(ws, ws_bytes);
  ProposalWs w;
  carve_proposal(c, w, A, H, W, pre_nms);
  if (!ws || !c.ok()) {
    set_error("tlod_proposal_keep_f32: workspace too small");
    return kWorkspace;
  }
  return launch_keep(cls_prob, bbox_deltas, im_info, base_anchors, B, A, H, W, feat_stride,
                     pre_nms, nms_thresh, kept, counts, w, (hipStream_t)stream);
}

extern "C" int tlod_proposal_pick_f32(const float* kept, const int32_t* counts, int B, int cap,
                                      int post, int head, const int32_t* pick,
                                      const int32_t* pick_off, uint64_t seed, float* rois_out,
                                      tlod_stream_t stream) {
  TLOD_CHECK_ARG(kept && counts && rois_out, "null pointer");
  TLOD_CHECK_ARG(!pick == !pick_off, "pick and pick_off: both or neither");
  const int st = check_pick(__func__, B, cap, post, head);
  if (st != kOk) return st;
  hipLaunchKernelGGL(proposal_pick_kernel, dim3(B), dim3(kPickThreads), 0, (hipStream_t)stream,
                     kept, counts, cap, post, head, pick, pick_off, seed, rois_out);
  TLOD_LAUNCH_CHECK();
  return kOk;
}

extern "C" size_t tlod_proposal_subsample_workspace_bytes(int B, int A, int H, int W,
                                                          int pre_nms) {
  if (B <= 0 || A <= 0 || H <= 0 || W <= 0) return 0;
  Carve c(nullptr, 0);
  ProposalWs w;
  float* kept;
  int32_t* counts;
  return carve_subsample(c, w, &kept, &counts, B, A, H, W, pre_nms);
}

extern "C" int tlod_proposal_subsample_f32(const float* cls_prob, const float* bbox_deltas,
                                           const float* im_info, const float* base_anchors,
                                           int B, int A, int H, int W, int feat_stride,
                                           int pre_nms, int post, int head, float nms_thresh,
                                           uint64_t seed, float* rois_out, void* ws,
                                           size_t ws_bytes, tlod_stream_t stream) {
  TLOD_CHECK_ARG(cls_prob && bbox_deltas && im_info && base_anchors && rois_out, "null pointer");
  TLOD_CHECK_ARG(B > 0 && A > 0 && H > 0 && W > 0, "bad shape");
  const int cap = keep_cap(A, H, W, pre_nms);
  int st = check_pick(__func__, B, cap, post, head);
  if (st != kOk) return st;
  Carve c(ws, ws_bytes);
  ProposalWs w;
  float* kept;
  int32_t* counts;
  carve_subsample(c, w, &kept, &counts, B, A, H, W, pre_nms);
  if (!ws || !c.ok()) {
    set_error("tlod_proposal_subsample_f32: workspace too small");
    return kWorkspace;
  }
  hipStream_t s = (hipStream_t)stream;
  st = launch_keep(cls_prob, bbox_deltas, im_info, base_anchors, B, A, H, W, feat_stride,
                   pre_nms, nms_thresh, kept, counts, w, s);
  if (st != kOk) return st;
  hipLaunchKernelGGL(proposal_pick_kernel, dim3(B), dim3(kPickThreads), 0, s, kept, counts, cap,
                     post, head, (const int32_t*)nullptr, (const int32_t*)nullptr, seed,
                     rois_out);
  TLOD_LAUNCH_CHECK();
  return kOk;
}
