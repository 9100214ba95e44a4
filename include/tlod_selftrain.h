/*
 * tlod_selftrain.h — extension of the tlod C ABI (include/tlod.h, whose conventions all hold
 * here: status return + tlod_last_error(), explicit stream, every output element written, const
 * inputs never written, no allocation, no host synchronisation, argument errors refused before
 * anything is launched) with the device ops that close the IDF self-training loop: the pseudo
 * ground truth of one target image straight from tlod_detect_f32's outputs, and the domain
 * losses with EFocalLoss (methods/IDF/IDF_train.py --ef) on the instance rows.
 *
 * Replaces, per target image: the --savelabel pass of methods/IDF/faster_rcnn_test.py:316-369
 *   (detections to the host, str(int(x)) into VOC XML by lib/IDF/xml_create.py), the XML reader
 *   of lib/IDF/foggy_cityscape.py:239-242 and the gt bookkeeping of the training loader
 *   (minibatch.py:39-49, roibatchLoader.py) — for an image that needs no crop — by one launch;
 *   and the EFocalLoss graph of lib/IDF/net_utils.py:73-102 by one launch each way.
 */
#ifndef TLOD_SELFTRAIN_H_
#define TLOD_SELFTRAIN_H_

#include "tlod.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Pseudo ground truth of one image.
 *   dets (C, R, 5), counts (C): as tlod_detect_f32 leaves them — (x1, y1, x2, y2, score) rows in
 *     original-image coordinates, class-major; rows at or past counts[j] are never read; class 0
 *     is skipped whatever its count.  2 <= C, 1 <= R <= 2048, (C - 1) R < 2^31.
 *   Rows are taken for j = 1 .. C-1, each class in the order of dets.  Per coordinate x:
 *     v = max(trunc(x) - 1, 0)  (the XML's str(int(x)), then the reader's 0-based clamp),
 *     g = (float)((double)v * im_scale)  (one rounding).
 *   A row with g.x1 == g.x2 or g.y1 == g.y2 is dropped.  With n survivors of rank r = 0 .. n-1:
 *     n <= max_gt: all of them, in rank order;
 *     n >  max_gt: the max_gt with the smallest (rng_u64(seed, 0x70736575, r), r), in ascending
 *       r (rng_u64: the counter generator of the sampling layers) — a uniform random subset in
 *       place of the loader's shuffle + [:max_gt].
 *   gt_boxes (max_gt, 5): (g.x1, g.y1, g.x2, g.y2, (float)j) rows, zero past num_boxes;
 *   num_boxes: one int64 = min(n, max_gt).  im_scale > 0, max_gt >= 1.  One launch, no
 *   workspace. */
int tlod_pseudo_gt_f32(const float* dets, const int32_t* counts, int C, int R, double im_scale,
                       int max_gt, uint64_t seed, float* gt_boxes, int64_t* num_boxes,
                       tlod_stream_t stream);

/* tlod_idf_domain_loss_f32 / _bwd_f32 (include/tlod_idf.h: same arguments, same n_img cross
 *   entropies, bit for bit) with the last term EFocalLoss(class_num = 2, gamma):
 *     loss[n_img] = mean_r -exp(-gamma p_r) log p_r,  p_r = softmax(z_ins[r])[label_ins],
 *   alpha = 1 and no clamp (net_utils.py:73-102 has none), evaluated in double from the fp32
 *   logits.  Backward: dz_ins = g_loss[n_img] / R * exp(-gamma p) (gamma log p - 1 / p) *
 *   p (onehot - softmax).  Labels are 0 or 1; R >= 1; n_img >= 0.  One launch each. */
int tlod_idf_domain_loss_ef_f32(const float* z_img, int n_img, int label_img, const float* z_ins,
                                int R, int label_ins, float gamma, float* loss,
                                tlod_stream_t stream);
int tlod_idf_domain_loss_ef_bwd_f32(const float* z_img, int n_img, int label_img,
                                    const float* z_ins, int R, int label_ins, float gamma,
                                    const float* g_loss, float* dz_img, float* dz_ins,
                                    tlod_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* TLOD_SELFTRAIN_H_ */
