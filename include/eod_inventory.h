/* The C ABI of the map inventory of libeod_hip.so: entry points beside include/eod_hip.h, include/eod_place.h and
 * include/eod_regions.h, with the same conventions (plain pointers and sizes, EOD_ERR_* status codes, all work queued on the stream
 * passed in, nothing allocates or synchronises).  The typed binding is `INVENTORY_SIGNATURES` of
 * embodied_object_detection_amd/_lib.py. */
#ifndef EOD_INVENTORY_H
#define EOD_INVENTORY_H
#include "eod_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Map inventory: every object of B label maps, all classes in one call.  A read-only query on what eod_semmap_labels leaves with
 * EOD_SEMMAP_SCORES (or on any other label map); integers and comparisons only.
 *   labels [B, N] int32, scores [B, N] float32, N = rows * cols, cell i = r * cols + c
 *   keep   uint8 [C], shared by all maps, or null;  C classes
 *   level  finite, in (0, 1];  connectivity 4 or 8;  min_cells >= 1;  topk K in 1..EOD_INVENTORY_TOPK_MAX
 * FOREGROUND: the cells with 0 <= labels[i] < C, with keep null or keep[labels[i]] != 0, and with scores[i] >= level (a NaN compares
 * false).  Every other label value is background: -1, C, any negative number, INT_MAX.
 * ADJACENT: two foreground cells (r, c), (r', c') that carry THE SAME LABEL, with |r - r'| + |c - c'| == 1 (connectivity 4), or with
 * max(|r - r'|, |c - c'|) == 1 (connectivity 8).  Rows and columns are the grid's: (r, cols - 1) and (r + 1, 0) are not adjacent.
 * COMPONENT: a maximal set of foreground cells joined by adjacency; its label is its smallest cell index, its AREA its cell count,
 * its CLASS the label its cells carry.  THE ORDER of components: area descending, then label ascending.
 *
 * object_labels (int32 [B, N]): the label of the cell's component, -1 for background.
 * out (int32 words, 8-byte aligned, EOD_INVENTORY_OUT_WORDS(B, K, C) of them):
 *   [0] status: 0, or nonzero when a bounded loop of a kernel reached its bound (the results are then void);  [1] reserved (0)
 *   count      int32 [B]        at 2            components with area >= min_cells, of all classes
 *   foreground int32 [B]        at 2 + B        foreground cells
 *   then, with S = 2 + 2 B, per map the K components with area >= min_cells that come first in the order, over all classes
 *   together; the slots behind them hold object -1, cls -1 and zeros everywhere else:
 *   object     int32 [B, K]     at S            the label
 *   area       int32 [B, K]     at S + B K
 *   peak       int32 [B, K]     at S + 2 B K    the cell of the component with the largest score, the lowest cell on ties
 *   peak_score float32 [B, K]   at S + 3 B K    the bits of scores at that cell
 *   bbox       int32 [B, K, 4]  at S + 4 B K    r0, c0, r1, c1, inclusive
 *   sum_rc     int64 [B, K, 2]  at S + 8 B K    sum of the rows, sum of the columns of its cells
 *   mass_q24   int64 [B, K]     at S + 12 B K   sum over its cells of (int)(min(score, 1.0f) * 16777216.0f): the product is exact and
 *                                               the conversion truncates, so the sum does not depend on its order
 *   cls        int32 [B, K]     at S + 14 B K   the class
 *   then, with T = S + 15 B K, the table of the classes:
 *   class_objects      int32 [B, C]  at T          components of the class with area >= min_cells
 *   class_cells        int32 [B, C]  at T + B C    foreground cells of the class, whatever the area of their components
 *   class_largest      int32 [B, C]  at T + 2 B C  the label of the first component of the class in the order, among those with
 *                                                  area >= min_cells; -1 if there is none
 *   class_largest_area int32 [B, C]  at T + 3 B C  its area; 0 if there is none
 * Integer atomics only: every output is a pure function of the inputs.
 *
 * workspace: eod_map_inventory_workspace_bytes(B, N, C, topk) bytes, 8-byte aligned, any contents: three int32 [B, N] arrays (parent,
 * area, slot), rounded up to 256 bytes, B K 64-bit peak keys and B C 64-bit class keys.  0 for arguments the call refuses.
 * EOD_ERR_BAD_DIMS, before any launch: B outside 1..EOD_INVENTORY_B_MAX, C outside 1..EOD_INVENTORY_C_MAX, topk outside
 * 1..EOD_INVENTORY_TOPK_MAX, connectivity not 4 or 8, min_cells < 1, cols < 1, N < 1, N > EOD_INVENTORY_N_MAX, N % cols != 0, level
 * NaN, infinite, <= 0 or > 1;  EOD_ERR_NULL / EOD_ERR_ALIGN: a pointer (keep may be null);  EOD_ERR_CAPACITY: workspace_bytes too
 * small.  The tile one workgroup labels in LDS is that of include/eod_regions.h; the result does not depend on it. */
#define EOD_INVENTORY_B_MAX 32
#define EOD_INVENTORY_C_MAX 2047
#define EOD_INVENTORY_TOPK_MAX 64
#define EOD_INVENTORY_N_MAX 4194304
#define EOD_INVENTORY_OUT_WORDS(B, K, C) (2 + 2 * (B) + 15 * (B) * (K) + 4 * (B) * (C))
size_t eod_map_inventory_workspace_bytes(int B, int N, int C, int topk);
int eod_map_inventory(const int32_t* labels, const float* scores, const uint8_t* keep, int B, int N, int cols, int C, float level,
                      int connectivity, int min_cells, int topk, int32_t* object_labels, int32_t* out, void* workspace,
                      size_t workspace_bytes, eod_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* EOD_INVENTORY_H */
