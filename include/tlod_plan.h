/*
 * tlod_plan.h — extension of the tlod C ABI (include/tlod.h, whose conventions hold here:
 * status return + tlod_last_error()) with host-only queries of what a kernel's plan does.
 * They run without a GPU, like the *_workspace_bytes queries.
 *
 * tlod_conv_ws_store_map: the store plan of the warp-specialized 3x3 kernel's epilogue on whole
 * tiles (tlod_conv_fwd_bs_f32 / tlod_conv_dgrad_bs_mask_f32 / tlod_conv_fwd_bs_pool_f32 at
 * Cin >= 64) for one channel plane of an H x W map.  It replays the kernel's own
 * classification functions with the kernel's address arithmetic.
 *   pool == 0  the direct epilogue on the H x W output, in the tiles the planner picks: a
 *              lane's four consecutive pixels leave in one 16-B store when they are a run
 *              inside one tile row and the map, per element when the group straddles a
 *              tile-row end, the tile's end or the map's right edge.
 *              wide[h * W + w], single[h * W + w] (H * W ints each): how many 16-B / 4-B
 *              stores write the element.
 *   pool != 0  the pooling epilogue (16 x 32 tiles; H, W >= 2), which writes the (H / 2) x
 *              (W / 2) pooled map and nothing else: a lane's two pooled outputs leave in one
 *              8-B store, or the first alone in an odd pooled width's last column.
 *              wide[hp * (W / 2) + wp], single[...] ((H / 2) * (W / 2) ints each): how many
 *              8-B / 4-B stores write the pooled element.
 *   *stray   how many floats a store would put outside the written map or, for a 16-B / 8-B
 *            store, into another row of it than its first element's
 *   tile     (optional) {tile rows, tile columns}
 * A correct plan has wide + single == 1 everywhere and *stray == 0.  Split-K pieces store to
 * their slab, not to the map; the query does not cover them.
 */
#ifndef TLOD_PLAN_H_
#define TLOD_PLAN_H_

#include "tlod.h"

#ifdef __cplusplus
extern "C" {
#endif

int tlod_conv_ws_store_map(int H, int W, int pool, int32_t* wide, int32_t* single,
                           int32_t* tile, int32_t* stray);

#ifdef __cplusplus
}
#endif

#endif /* TLOD_PLAN_H_ */
