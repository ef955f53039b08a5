/* The C ABI of the frame-side map queries of libeod_hip.so: entry points beside include/eod_hip.h, with the same conventions
 * (plain pointers and sizes, EOD_ERR_* status codes, all work queued on the stream passed in, nothing allocates or
 * synchronises).  The typed binding is `PLACE_SIGNATURES` of embodied_object_detection_amd/_lib.py. */
#ifndef EOD_PLACE_H
#define EOD_PLACE_H
#include "eod_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Place detections on the map: the grid cells under each instance mask.  A read-only query beside the frame; integers only.
 *   masks  [K_cap, H, W] bytes (uint8 or bool; any alignment), nonzero = set
 *   proj   [H, W] int32, one grid cell per pixel
 *   count  device int32 or NULL (= K_cap): rows k >= count are not read (clamped into [0, K_cap])
 *   rects  int32 [K_cap, 4] (x0, y0, x1, y1), half-open, clipped to the image by the kernel, or NULL (= the whole image)
 *   topk   T in 1..EOD_PLACE_TOPK_MAX;  exclude_cell: a cell whose pixels are dropped (typically the robot's own cell, where
 *          zero-depth pixels land), -1 for none
 * For row k < count let S_k be the pixels inside the rect whose mask byte is nonzero (pixels outside the rect are ignored by
 * definition).  A pixel of S_k with cell c = proj[y, x] is INVALID if c < 0 or c >= n_cells (counted in invalid[k] and nowhere else;
 * c is never used as an index), is dropped if c == exclude_cell, and otherwise adds 1 to the histogram h_k[c].
 * out (int32, (4 + 2 T) * K_cap words):
 *   [0, K_cap) mask_pixels = |S_k|;  [K_cap, 2 K_cap) pixels = sum of h_k;  [2 K_cap, 3 K_cap) invalid;
 *   [3 K_cap, 4 K_cap) distinct = number of cells with h_k > 0 (the footprint);
 *   then cells [K_cap][T]: the T cells with the largest h_k by (count descending, cell ascending), padded with -1;
 *   then cell_pixels [K_cap][T]: their counts, padded with 0.
 * Rows k >= count hold the padding values (0, 0, 0, 0, -1, 0).  Integer atomics only: the result is a pure function of the inputs.
 *
 * table_log2: size of the per-detection LDS hash table, EOD_PLACE_TABLE_LOG2_MIN..EOD_PLACE_TABLE_LOG2_MAX, 0 = the default
 * EOD_PLACE_TABLE_LOG2 (4096 entries: a detection that fills it spans 4096 map cells).  A detection whose cells do not fit is
 * counted again, exactly, by a second kernel in one of EOD_PLACE_SLOTS dense int32[n_cells] tables of the workspace, so the result
 * does not depend on table_log2.  workspace: eod_place_masks_workspace_bytes(K_cap, n_cells) bytes, 4-byte aligned, any contents
 * (an overflow list of K_cap + 64 words and the slots' tables; the call initialises what it reads).  K_cap == 0 launches nothing.
 * EOD_ERR_BAD_DIMS: K_cap < 0, H or W < 1, H * W beyond int32, n_cells < 1, topk or table_log2 out of range;
 * EOD_ERR_CAPACITY: workspace_bytes too small. */
#define EOD_PLACE_TOPK_MAX 8
#define EOD_PLACE_TABLE_LOG2_MIN 4
#define EOD_PLACE_TABLE_LOG2_MAX 12
#define EOD_PLACE_TABLE_LOG2 12
#define EOD_PLACE_SLOTS 4
size_t eod_place_masks_workspace_bytes(int K_cap, int n_cells);
int eod_place_masks(const uint8_t* masks, const int32_t* proj, const int32_t* count, const int32_t* rects, int K_cap, int H, int W,
                    int n_cells, int topk, int exclude_cell, int table_log2, int32_t* out, void* workspace, size_t workspace_bytes,
                    eod_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* EOD_PLACE_H */
