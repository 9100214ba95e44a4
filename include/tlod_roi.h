/*
 * tlod_roi.h — extension of the tlod C ABI (include/tlod.h, whose conventions all hold here:
 * status return + tlod_last_error(), explicit stream, const inputs never written, no
 * allocation and no host synchronisation) with the RoIPool backward that follows the
 * reference's gather (lib/model/roi_pooling/src/roi_pooling_kernel.cu:128-203) test for test.
 *
 * tlod_roi_pool_bwd_f32 (tlod.h) scatters top_grad through argmax and nothing else.  The
 * reference adds top_grad(roi, c, ph, pw) to input element a only if a is that bin's argmax
 * AND a lies in the RoI's image (:150-154) and in channel c, (h, w) of a lies inside the
 * RoI's rounded, unclipped, inclusive extent (:162-166), and (ph, pw) lies in the feasible bin
 * range of (h, w) (:182-190).  The two differ for a RoI whose rounded extent is inverted
 * (round(x2 * scale) < round(x1 * scale), or the same in y): the forward forces it to 1 x 1
 * and pools the cell at its start, which lies outside [start, end], so the reference passes no
 * gradient through it.  This entry point applies those tests per bin; tlod.roi_pool uses it.
 *
 * top_grad, argmax (R,C,ph,pw); rois (R,5) and scale as given to tlod_roi_pool_fwd_f32.
 * ACCUMULATES into bottom_grad (B,C,H,W) (zero it first).  An argmax outside [0, B*C*H*W) is
 * skipped.
 */
#ifndef TLOD_ROI_H_
#define TLOD_ROI_H_

#include "tlod.h"

#ifdef __cplusplus
extern "C" {
#endif

int tlod_roi_pool_bwd_gather_f32(const float* top_grad, const int32_t* argmax, int B, int C,
                                 int H, int W, const float* rois, int R, int ph, int pw,
                                 float scale, float* bottom_grad, tlod_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* TLOD_ROI_H_ */
