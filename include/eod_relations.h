/* The C ABI of the object relations of libeod_hip.so: one entry point beside include/eod_hip.h, include/eod_place.h,
 * include/eod_regions.h, include/eod_inventory.h and include/eod_describe.h, with the same conventions (plain pointers and sizes,
 * EOD_ERR_* status codes, all work queued on the stream passed in, nothing allocates or synchronises).  The typed binding is
 * `RELATIONS_SIGNATURES` of embodied_object_detection_amd/_lib.py. */
#ifndef EOD_RELATIONS_H
#define EOD_RELATIONS_H
#include "eod_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define EOD_RELATIONS_K_MAX 64        /* objects of one call: one wave looks a label up, one 64-bit mask holds the slots a cell saw */
#define EOD_RELATIONS_N_MAX 4194304   /* cells */
#define EOD_RELATIONS_DIM_MAX 32767   /* rows and columns: 2 * 32766^2 < 2^31, so a squared distance is a positive int32 below INT_MAX */
#define EOD_RELATIONS_RADIUS_MAX 16
#define EOD_RELATIONS_TOPN_MAX 8

/* How the objects of a label map stand to each other and to one given cell: a scene graph over up to 64 objects.
 *   object_labels  int32 [N], N = rows * cols, cell i = r * cols + c: object_labels of eod_map_inventory, a row of region_labels of
 *                  eod_map_regions, or any other label map
 *   objects        int32 [K], 1 <= K <= EOD_RELATIONS_K_MAX: the labels asked for, -1 (any negative value) in unused slots
 *   1 <= N <= EOD_RELATIONS_N_MAX, cols >= 1, N % cols == 0, rows = N / cols and cols <= EOD_RELATIONS_DIM_MAX
 *   radius R       1..EOD_RELATIONS_RADIUS_MAX;  from_cell -1..N-1;  topn 1..EOD_RELATIONS_TOPN_MAX
 * SLOT, as in eod_describe_pool: cell i belongs to the lowest slot k with objects[k] == object_labels[i] and objects[k] >= 0.  A
 * later duplicate slot gets no cells.  A cell whose label is in no slot (-1, any negative value, a label not asked for) takes no part.
 * DISTANCE: d2(i, j) = (r_i - r_j)^2 + (c_i - c_j)^2 on the rows and columns of the grid: the cells (r, cols - 1) and (r + 1, 0) are
 * cols - 1 columns apart, not neighbours.  Outside the grid there is no cell.
 * WITHIN REACH: d2 <= R * R: a disc, not a square.
 * For every ordered pair of slots a != b, over the cell pairs (i in a, j in b) within reach:
 *   pair_key    uint64 [K, K], 8-byte aligned: the minimum of (d2 << 32) | i; all ones where no pair is within reach and on the diagonal
 *   min_d2      int32 [K, K]: the upper half of pair_key; INT_MAX where none and on the diagonal.  Symmetric.
 *   closest     int32 [K, K]: the lower half of pair_key: the cell of a nearest to b, the lowest such cell on ties; -1 where none
 *   near_cells  int32 [K, K]: the cells of a with at least one cell of b within reach; 0 on the diagonal.  Not symmetric:
 *               near_cells[a, b] == cells[a] says "a lies on / inside the reach of b".
 *   edges       int32 [K, K]: the cell pairs (i, j) with d2 == 1, each counted once: the length of the shared border; 0 on the
 *               diagonal.  Symmetric.
 *   cells       int32 [K]: the slot's cells
 *   nearest     int32 [K, topn]: per slot a the slots b with min_d2[a, b] < INT_MAX by (min_d2 ascending, slot ascending); then -1
 *   nearest_d2  int32 [K, topn]: the min_d2 of those slots; then INT_MAX
 *   from_key    uint64 [K], 8-byte aligned: over ALL cells i of the slot, whatever the radius, the minimum of
 *               (d2(i, from_cell) << 32) | i; all ones for a slot without cells and with from_cell == -1
 *   from_d2     int32 [K]: the upper half of from_key; INT_MAX where from_key is all ones
 *   from_closest int32 [K]: the lower half of from_key: the slot's cell nearest to from_cell, the lowest on ties; -1 where all ones
 * Every output may hold anything on entry.  Integer atomics (min, add) and comparisons only: every output is a pure function of the
 * inputs, independent of order, grid and scheduling.
 * EOD_ERR_BAD_DIMS, before any launch: K, N, radius, topn or from_cell out of range, cols < 1, N % cols != 0, rows or cols above
 * EOD_RELATIONS_DIM_MAX; then EOD_ERR_NULL; then EOD_ERR_ALIGN (pair_key and from_key 8 bytes, the others 4).  No workspace. */
int eod_map_relations(const int32_t* object_labels, const int32_t* objects, int N, int K, int cols, int radius, int from_cell, int topn,
                      uint64_t* pair_key, int32_t* min_d2, int32_t* closest, int32_t* near_cells, int32_t* edges, int32_t* cells,
                      int32_t* nearest, int32_t* nearest_d2, uint64_t* from_key, int32_t* from_d2, int32_t* from_closest,
                      eod_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* EOD_RELATIONS_H */
