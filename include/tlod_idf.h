/*
 * tlod_idf.h — extension of the tlod C ABI (include/tlod.h, whose conventions all hold here:
 * status return + tlod_last_error(), explicit stream, caller-provided workspace checked
 * against its *_workspace_bytes query, every output element written, const inputs never
 * written, no allocation and no host synchronisation) with the device ops of IDF
 * (lib/IDF/{faster_rcnn,net_utils}.py, methods/IDF/IDF_train.py of the reference).
 *
 * Replaces, per feature level and image: torch.sigmoid + mean + mean + where of dam()
 *   (net_utils.py:300-306), the two masked products, F.pairwise_distance and its mean, and the
 *   two (1 + att) modulations (faster_rcnn.py:77-85, 95-101) — about ten passes over a
 *   512-channel map forward and more backward — and the seven small loss graphs per image of
 *   IDF_train.py:242-327 (six two-logit cross entropies, one FocalLoss over the RoI rows).
 *
 * Maps are contiguous NCHW float32; att / d maps are (N, H, W).  Every sum runs in a fixed
 * order with double accumulators, so results are bit-identical from run to run.  All scalars
 * (thresholds, distances, losses, upstream gradients) live in device memory.
 */
#ifndef TLOD_IDF_H_
#define TLOD_IDF_H_

#include "tlod.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Domain attention map, per image n: s = sigmoid(x) (evaluated in double from the fp32 value
 *   and rounded once at the end of the channel mean), avg[n, p] = mean_c s[n, c, p] (fp32),
 *   thr[n] = mean_p avg[n, p] (fp32), att[n, p] = avg[n, p] < thr[n] ? 0 : avg[n, p].
 *   Each image of a batch gets its own threshold (the reference's mean(avg) is over a batch
 *   of one).  ws: tlod_idf_dam_workspace_bytes(N, H, W). */
size_t tlod_idf_dam_workspace_bytes(int N, int H, int W);
int tlod_idf_dam_f32(const float* x, int N, int C, int H, int W, float* att, void* ws,
                     size_t ws_bytes, tlod_stream_t stream);

/* Separation forward.  With w = att_b[n, p] (1 where att_b is NULL):
 *   d[n, p]  = || (a[n, :, p] - b[n, :, p]) w + 1e-6 ||_2 over the C channels (the channel-axis
 *              pairwise_distance of PyTorch 0.4, eps added to the difference),
 *   dist[n]  = mean_p d[n, p],
 *   a_out    = a (1 + att_b),  b_out = b (1 + att_a)   (fp32: one add, one multiply).
 *   a_out and b_out are both given or both NULL (no modulation; att_a is then unused and may
 *   be NULL); when they are given, att_a and att_b are required.  a and b are read once.
 *   a_out / b_out may not alias a / b.  ws: tlod_idf_sep_fwd_workspace_bytes(N, H, W). */
size_t tlod_idf_sep_fwd_workspace_bytes(int N, int H, int W);
int tlod_idf_sep_fwd_f32(const float* a, const float* b, const float* att_a, const float* att_b,
                         int N, int C, int H, int W, float* a_out, float* b_out, float* d,
                         float* dist, void* ws, size_t ws_bytes, tlod_stream_t stream);

/* Separation backward (att carries no gradient: the reference detaches it).  With w as above
 *   and t = g_dist[n] / (H W) * w * ((a - b) w + 1e-6) / d[n, p] (0 where d is 0):
 *   g_a = g_a_out (1 + att_b) + t,   g_b = g_b_out (1 + att_a) - t.
 *   g_a_out / g_b_out: both given (att_a and att_b then required) or both NULL (their terms
 *   are 0).  g_dist (N) is required; the caller folds the loss weight (0.001) into it. */
int tlod_idf_sep_bwd_f32(const float* a, const float* b, const float* att_a, const float* att_b,
                         const float* d, const float* g_a_out, const float* g_b_out,
                         const float* g_dist, int N, int C, int H, int W, float* g_a, float* g_b,
                         tlod_stream_t stream);

/* Domain losses of one image (weights not folded in):
 *   z_img (n_img, 2): the two-logit outputs of the image discriminators, one row each;
 *     loss[i] = cross_entropy(z_img[i], label_img), i < n_img (n_img >= 0);
 *   z_ins (R, 2): the instance discriminator's logits; loss[n_img] = FocalLoss(class_num = 2,
 *     gamma)(z_ins, label_ins) = mean_r -(1 - P_r)^gamma log P_r, P_r =
 *     clamp(softmax(z_ins[r])[label_ins], 1e-6, 1) (net_utils.py:151-177).  R >= 1.
 *   Labels are 0 or 1; gamma > 0 (anything else is refused: pow(1 - P, gamma) at P = 1 has no
 *   finite meaning there).  loss holds n_img + 1 floats.
 * Backward from g_loss (n_img + 1), one upstream scalar per term: dz_img = g_loss[i] (softmax -
 *   onehot); dz_ins = g_loss[n_img] / R * dL/dP * dP/dz, 0 in rows where the fp32 softmax[label]
 *   is below 1e-6 (the clamp's gradient, as in the reference) and in rows where 1 - P is 0 in
 *   double (the label's logit leads by about 37 or more), for every gamma > 0, gamma < 1
 *   included.  One launch each. */
int tlod_idf_domain_loss_f32(const float* z_img, int n_img, int label_img, const float* z_ins,
                             int R, int label_ins, float gamma, float* loss,
                             tlod_stream_t stream);
int tlod_idf_domain_loss_bwd_f32(const float* z_img, int n_img, int label_img,
                                 const float* z_ins, int R, int label_ins, float gamma,
                                 const float* g_loss, float* dz_img, float* dz_ins,
                                 tlod_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* TLOD_IDF_H_ */
