/*
 * tlod_pa_atf.h — extension of the tlod C ABI (include/tlod.h, whose conventions all hold here:
 * status return + tlod_last_error(), explicit stream, every output element written, const
 * inputs never written, no allocation, no atomics and no host synchronisation) with the
 * device ops of PA-ATF (lib/PA_ATF/faster_rcnn.py, methods/PA_ATF/PA_ATF_train.py of the
 * reference): the im2col / col2im pair that puts a strided convolution on the split-bf16 GEMM,
 * the gated image discriminator's channel gate, the prototype pooling in front of CLUB, the 14
 * scalar loss terms of a step, and the target's subsampled proposal layer.
 *
 * Maps are contiguous NCHW float32.  Every sum runs in one fixed order, so results are
 * bit-identical from run to run.
 */
#ifndef TLOD_PA_ATF_H_
#define TLOD_PA_ATF_H_

#include "tlod.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Strided convolution as a GEMM.  Replaces nn.Conv2d / cuDNN for _ImageDA's Convm1 (5x5,
 * stride 3) and Convm2 (3x3, stride 2) (faster_rcnn.py:74-77) and CLUB's out_score.0 (3x3,
 * stride 2, :110).  Square kernels, KS >= 1, stride >= 1, pad >= 0, and an output of at least
 * 1 x 1: Ho = (H + 2 pad - KS) / stride + 1, Wo likewise.
 *   col[(n, ho, wo)][(c, kh, kw)] = x[n][c][ho stride + kh - pad][wo stride + kw - pad],
 *   0 outside the map; col is (N Ho Wo, C KS KS) row-major.  The column order is the
 *   nn.Conv2d weight's own, so y (N Ho Wo, Cout) = tlod_gemm_bs_ex_f32(col, weight (Cout,
 *   C KS KS), bias, relu) with both operands K-contiguous. */
int tlod_im2col_f32(const float* x, int N, int C, int H, int W, int KS, int stride, int pad,
                    float* col, tlod_stream_t stream);
/* The adjoint, as a gather: dx[n][c][h][w] = the sum, in (kh, kw) order, of the
 *   dcol[(n, ho, wo)][(c, kh, kw)] with ho stride + kh - pad == h and wo stride + kw - pad == w
 *   (at most ceil(KS / stride)^2 of them).  dx (N, C, H, W) is fully written: cells that no
 *   window covers (the trailing rows / columns when (H + 2 pad - KS) % stride != 0) get 0. */
int tlod_col2im_f32(const float* dcol, int N, int C, int H, int W, int KS, int stride, int pad,
                    float* dx, tlod_stream_t stream);

/* Channel gate of _ImageDA (faster_rcnn.py:90-92): mask = sigmoid(adaptive_max_pool2d(z, 1)).
 *   z (N, C, h, w) -> mask (N, C) float32, arg (N, C) int32: the plane's maximum under torch's
 *   rule (the first maximum in row-major order; a NaN wins, of several the last one:
 *   adaptive_max_pool2d's scan takes over on val > max || isnan(val)) as the index
 *   y w + x inside the plane; the sigmoid is evaluated in double and rounded once. */
int tlod_pa_gate_f32(const float* z, int N, int C, int h, int w, float* mask, int32_t* arg,
                     tlod_stream_t stream);
/* Its backward: dz (N, C, h, w) = (dmask (1 - mask)) mask (fp32, torch's sigmoid backward) at
 *   arg, 0 elsewhere; fully written. */
int tlod_pa_gate_bwd_f32(const float* dmask, const float* mask, const int32_t* arg, int N, int C,
                         int h, int w, float* dz, tlod_stream_t stream);

/* Prototype pooling of one feature level (faster_rcnn.py:387-406 with CLUB.forward :131-138).
 *   feat (1, C, H, W); rois (G, 5) = (index, x1, y1, x2, y2) — the index column is not read,
 *   the map holds one image; mask (C): the level's channel gate; perm (G) int32: CLUB's
 *   shuffle.  With p = _RoIPooling(7, 7, scale)(feat, rois), exactly tlod_roi_pool_fwd_f32's
 *   arithmetic (an empty bin gives 0 and argmax -1):
 *     same[g, c] = p[g, c] m[c]           same[g, C + c] = p[g, c] (1.f - m[c])
 *     diff[g, c] = same[g, c]             diff[g, C + c] = p[perm[g], c] (1.f - m[c])
 *   fp32 products.  same, diff: (G, 2C, 7, 7); argmax (G, C, 7, 7) int32: p's flat index into
 *   feat.  A perm entry outside [0, G) pairs its RoI with zeros (nothing is read through it). */
int tlod_pa_proto_pool_fwd_f32(const float* feat, int C, int H, int W, const float* rois, int G,
                               float scale, const float* mask, const int32_t* perm, float* same,
                               float* diff, int32_t* argmax, tlod_stream_t stream);
/* Its backward with CLUB's gradient reversal folded in: dfeat (1, C, H, W) = -alpha times the
 *   gradient of both outputs routed through argmax (mask carries no gradient: the reference
 *   detaches it); fully written.  A gather: each cell adds, over the RoIs in index order and
 *   the bins of a RoI in (ph, pw) order that took their maximum there,
 *     m (d_same[g, c] + d_diff[g, c]) + (1 - m) (d_same[g, C + c] + sum over g2 with
 *     perm[g2] == g of d_diff[g2, C + c])
 *   in double, rounded once.  rois / scale: the forward's (they bound the bins a cell can be
 *   in). */
int tlod_pa_proto_pool_bwd_f32(const float* d_same, const float* d_diff, const float* mask,
                               const int32_t* perm, const int32_t* argmax, const float* rois,
                               int G, float scale, int C, int H, int W, float alpha,
                               float* dfeat, tlod_stream_t stream);

/* The 14 scalar loss terms of a PA-ATF step, unweighted, in one launch each way (the reference
 *   builds 14 small graphs: faster_rcnn.py:57-66, 84-103, 141-147).  z, n, label (and dz) are
 *   host arrays of TLOD_PA_ATF_TERMS entries; z[t] / dz[t] are device pointers, every one
 *   required, n[t] >= 1.
 *   t = 0..5, image terms (source and target at conv3, conv4, conv5 in the caller's order):
 *     z[t] holds n[t] logits, label[t] in {0, 1} the constant domain label;
 *     loss[t] = BCELoss(sigmoid(z), label) = mean min(softplus(label ? -z : z), 100): the
 *     elementwise BCE over equal element counts with BCELoss's log clamp at -100, evaluated
 *     from the logit (so the clamp acts at |z| >= 100, not where an fp32 sigmoid saturates).
 *   t = 6, 7, instance terms: z[t] holds n[t] = R logits, label[t] in [0, R] the number of ones
 *     among the R labels; with x = sigmoid(z), loss[t] = mean_i mean_j |x_i - l_j| =
 *     mean_i (ones (1 - x_i) + (R - ones) x_i) / R — torch.abs(x (R, 1) - label (R)).mean() of
 *     the reference, which broadcasts to (R, R).
 *   t = 8..13, CLUB terms: z[t] holds (n[t] = G, 2) logits, label[t] in {0, 1};
 *     loss[t] = mean_g cross_entropy(z[g], label).
 *   Everything is evaluated in double from the fp32 logits and rounded once; each term is one
 *   workgroup's fixed-order sum.
 * Backward: dz[t] = g_loss[t] (device, 14 floats) times the term's derivative, every element
 *   written (0 where the BCE clamp is active); the 14 dz buffers must be distinct. */
#define TLOD_PA_ATF_TERMS 14
int tlod_pa_atf_loss_f32(const float* const* z, const int* n, const int* label, float* loss,
                         tlod_stream_t stream);
int tlod_pa_atf_loss_bwd_f32(const float* const* z, const int* n, const int* label,
                             const float* g_loss, float* const* dz, tlod_stream_t stream);

/* The target's subsampled proposal layer (proposal_layer1.py:152-160: for cfg_key != 'TRAIN'
 *   the NMS survivors are not truncated; the first head = int(post * 0.25) stay, then
 *   min(len(rest), post - head) of the rest are drawn without replacement; zero padded), in two
 *   phases so that the draw can be replayed (csrc/proposal.hip).
 * keep: tlod_proposal_f32's inputs, decode, sort, pre-NMS top-N and NMS, but every survivor is
 *   written: kept (B, cap, 4) in score order, zeros after the survivors, cap = pre_nms if
 *   0 < pre_nms < A H W else A H W; counts (B) int32.  ws: tlod_proposal_workspace_bytes.
 * pick: rois_out (B, post, 5), fully written, column 0 the image index:
 *   rows [0, min(count, head)): the first survivors;
 *   then, pick != NULL: the survivors head + pick[pick_off[b] + j], j < min(pick_off[b + 1] -
 *     pick_off[b], count - head, post - head), in the given order (pick, pick_off (B + 1):
 *     device int32; an index outside [0, count - head) gives a zero row);
 *   pick == NULL (pick_off NULL too): min(count - head, post - head) distinct survivors of the
 *     rest, a uniform subset drawn with the counter-based generator of the anchor / proposal
 *     targets keyed by (seed, image, survivor), appended in ascending rank;
 *   zeros after.  0 <= head <= post; cap <= 16384 (TLOD_EUNSUPPORTED beyond).
 *   Cost of the device draw: one workgroup per image ranks the n = count - head keys against
 *   each other, n^2 compares and n^2 / 256 key evaluations per thread pass — about 4e6
 *   compares at the 2000 survivors of a 600 x 1200 image, 2.7e8 on one CU at the cap; sized
 *   for the former.
 * subsample: both phases chained with the device RNG, no host synchronisation;
 *   ws: tlod_proposal_subsample_workspace_bytes. */
int tlod_proposal_keep_f32(const float* cls_prob, const float* bbox_deltas, const float* im_info,
                           const float* base_anchors, int B, int A, int H, int W,
                           int feat_stride, int pre_nms, float nms_thresh, float* kept,
                           int32_t* counts, void* ws, size_t ws_bytes, tlod_stream_t stream);
int tlod_proposal_pick_f32(const float* kept, const int32_t* counts, int B, int cap, int post,
                           int head, const int32_t* pick, const int32_t* pick_off, uint64_t seed,
                           float* rois_out, tlod_stream_t stream);
size_t tlod_proposal_subsample_workspace_bytes(int B, int A, int H, int W, int pre_nms);
int tlod_proposal_subsample_f32(const float* cls_prob, const float* bbox_deltas,
                                const float* im_info, const float* base_anchors, int B, int A,
                                int H, int W, int feat_stride, int pre_nms, int post, int head,
                                float nms_thresh, uint64_t seed, float* rois_out, void* ws,
                                size_t ws_bytes, tlod_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* TLOD_PA_ATF_H_ */
