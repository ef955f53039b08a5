/* The C ABI of the map-region query of libeod_hip.so: entry points beside include/eod_hip.h and include/eod_place.h, with the same
 * conventions (plain pointers and sizes, EOD_ERR_* status codes, all work queued on the stream passed in, nothing allocates or
 * synchronises).  The typed binding is `REGIONS_SIGNATURES` of embodied_object_detection_amd/_lib.py. */
#ifndef EOD_REGIONS_H
#define EOD_REGIONS_H
#include "eod_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Map regions: the connected areas of each queried class, ranked by size.  A read-only query on a [Q, N] map (what
 * EOD_SEMMAP_LOCATE leaves as `prob`, or any other map); integers and comparisons only.
 *   prob   [Q, N] float32, N = rows * cols, cell i = r * cols + c
 *   level  finite, in (0, 1];  connectivity 4 or 8;  min_cells >= 1;  topk K in 1..EOD_REGIONS_TOPK_MAX
 * FOREGROUND of class q: the cells with prob[q, i] >= level (a NaN compares false: background).
 * ADJACENT: two foreground cells (r, c), (r', c') of one class with |r - r'| + |c - c'| == 1 (connectivity 4), or with
 * max(|r - r'|, |c - c'|) == 1 (connectivity 8).  Rows and columns are the grid's: (r, cols - 1) and (r + 1, 0) are not adjacent.
 * COMPONENT: a maximal set of foreground cells joined by adjacency; its LABEL is its smallest cell index, its AREA its cell count.
 *
 * labels (int32 [Q, N]): the label of the cell's component, -1 for background.
 * out (int32 words, 8-byte aligned, EOD_REGIONS_OUT_WORDS(Q, K) of them):
 *   [0] status: 0, or nonzero when a bounded loop of a kernel reached its bound (the results are then void);  [1] reserved (0)
 *   count      int32 [Q]        at 2            components with area >= min_cells
 *   foreground int32 [Q]        at 2 + Q        foreground cells
 *   then, with B = 2 + 2 Q, per class the K components with area >= min_cells that come first by (area descending, label
 *   ascending); the slots behind them hold region -1 and zeros everywhere else:
 *   region     int32 [Q, K]     at B            the label
 *   area       int32 [Q, K]     at B + Q K
 *   peak       int32 [Q, K]     at B + 2 Q K    the cell of the component with the largest prob, the lowest cell on ties
 *   peak_prob  float32 [Q, K]   at B + 3 Q K    the bits of prob at that cell
 *   bbox       int32 [Q, K, 4]  at B + 4 Q K    r0, c0, r1, c1, inclusive
 *   sum_rc     int64 [Q, K, 2]  at B + 8 Q K    sum of the rows, sum of the columns of its cells
 *   mass_q24   int64 [Q, K]     at B + 12 Q K   sum over its cells of (int)(min(prob, 1.0f) * 16777216.0f): the product is exact and
 *                                               the conversion truncates, so the sum does not depend on its order
 * Integer atomics only: every output is a pure function of the inputs.
 *
 * workspace: eod_map_regions_workspace_bytes(Q, N, topk) bytes, 8-byte aligned, any contents: three int32 [Q, N] arrays (parent,
 * area, slot), rounded up to 256 bytes, and Q K 64-bit peak keys.  0 for arguments the call refuses.
 * EOD_ERR_BAD_DIMS, before any launch: Q outside 1..EOD_REGIONS_Q_MAX, topk outside 1..EOD_REGIONS_TOPK_MAX, connectivity not 4 or 8,
 * min_cells < 1, cols < 1, N < 1, N > EOD_REGIONS_N_MAX, N % cols != 0, level NaN, infinite, <= 0 or > 1;
 * EOD_ERR_NULL / EOD_ERR_ALIGN: a pointer; EOD_ERR_CAPACITY: workspace_bytes too small.
 * EOD_REGIONS_TILE_ROWS x EOD_REGIONS_TILE_COLS is the tile one workgroup labels in LDS (csrc/regions.hip); the result does not
 * depend on it. */
#define EOD_REGIONS_Q_MAX 32
#define EOD_REGIONS_TOPK_MAX 64
#define EOD_REGIONS_N_MAX 4194304
#define EOD_REGIONS_TILE_ROWS 32
#define EOD_REGIONS_TILE_COLS 32
#define EOD_REGIONS_OUT_WORDS(Q, K) (2 + 2 * (Q) + 14 * (Q) * (K))
size_t eod_map_regions_workspace_bytes(int Q, int N, int topk);
int eod_map_regions(const float* prob, int Q, int N, int cols, float level, int connectivity, int min_cells, int topk, int32_t* labels,
                    int32_t* out, void* workspace, size_t workspace_bytes, eod_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* EOD_REGIONS_H */
