/* The C ABI of the line of sight on the map of libeod_hip.so: two entry points beside include/eod_hip.h, include/eod_place.h,
 * include/eod_regions.h, include/eod_inventory.h, include/eod_describe.h, include/eod_relations.h, include/eod_route.h and
 * include/eod_clearance.h, with the same conventions (plain pointers and sizes, EOD_ERR_* status codes, all work queued on the
 * stream passed in, nothing allocates or synchronises).  The typed binding is `SIGHT_SIGNATURES` of
 * embodied_object_detection_amd/_lib.py. */
#ifndef EOD_SIGHT_H
#define EOD_SIGHT_H
#include "eod_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define EOD_SIGHT_K_MAX 64            /* objects of one call: one wave looks a label up */
#define EOD_SIGHT_P_MAX 64            /* passable labels of one call: the same wave looks them up */
#define EOD_SIGHT_S_MAX 64            /* sources of one call: one bit of seen_mask each */
#define EOD_SIGHT_N_MAX 4194304       /* cells: the limits of eod_map_route and eod_map_clearance */
#define EOD_SIGHT_DIM_MAX 32767       /* rows and columns: a squared distance is at most 2 * 32766^2 = 2147221512 < 2^31 - 1 */
#define EOD_SIGHT_LDS_CELLS 131072    /* up to this many cells the walk stages the opacity bit plane (one bit a cell, 16 KB here)
                                         in LDS; above it the walk reads the bit plane from the workspace */
#define EOD_SIGHT_SOURCE_GROUP 16     /* the sources one workgroup of the walk looks from: their per-slot sums are in its LDS */

/* Which cells of a label map each of up to 64 cells can see, and how much of every object.
 *   object_labels  int32 [N], N = rows * cols, cell i = r * cols + c: object_labels of eod_map_inventory or any other label map
 *   objects        int32 [K], 1 <= K <= EOD_SIGHT_K_MAX: the labels asked for, -1 (any negative value) in unused slots
 *   passable       int32 [P], 0 <= P <= EOD_SIGHT_P_MAX: labels that do not block the view; NULL only when P == 0
 *   from_cells     int32 [S], 1 <= S <= EOD_SIGHT_S_MAX, IN HOST MEMORY (the only such argument: it is read during the call, so
 *                  that a cell outside the map is refused before any launch, and handed to the kernels by value): the cells to
 *                  look from, 0..N-1 each; any negative value marks an unused source; duplicates are allowed
 *   1 <= N <= EOD_SIGHT_N_MAX, cols >= 1, N % cols == 0, rows = N / cols and cols <= EOD_SIGHT_DIM_MAX
 *   range2  0 <= range2 <= INT_MAX: the sensor's range in cells, squared; INT_MAX is unbounded (a real squared distance is at most
 *           2 * (EOD_SIGHT_DIM_MAX - 1)^2 < INT_MAX, as in eod_map_clearance)
 * SLOT, as in eod_map_route: cell i belongs to the lowest slot k with objects[k] == object_labels[i] and objects[k] >= 0.  A later
 * duplicate slot gets no cells.
 * OPAQUE: a cell is opaque when its label is >= 0 and is not one of passable.  Every other cell is transparent.  On the lines of
 * source s the cell from_cells[s] is transparent whatever its label (the robot stands there, as on from_cell of eod_map_route); on
 * another source's lines it is what its label says.
 * THE LINE from s = (r0, c0) to t = (r1, c1): with dr = r1 - r0, dc = c1 - c0 and n = max(|dr|, |dc|), line cell i, i = 0..n, is
 *   (r0 + rnd(i * dr, n), c0 + rnd(i * dc, n)),   rnd(a, n) = sign(a) * floor((2 * |a| + n) / (2 * n)):
 * a / n rounded to the nearest integer, a half away from zero.  Cell 0 is s, cell n is t, consecutive cells differ by at most one
 * row and one column, and the line never leaves the box its two ends span.  Mirroring or transposing the grid mirrors or transposes
 * the line.  The line is NOT symmetric in s and t: a half is rounded away from the end the line starts from (the 3 x 5 map below).
 * SEES: source s sees cell t when all three hold:
 *   1. dr^2 + dc^2 <= range2;
 *   2. every line cell i with 1 <= i <= n - 1 is transparent;
 *   3. for every step i - 1 -> i, 1 <= i <= n, that changes both row and column, from (ra, ca) to (rb, cb), the side cells
 *      (ra, cb) and (rb, ca) are not both opaque: no sight through the point where two objects touch at a corner (the rule of
 *      eod_map_route for a diagonal step, applied to light).
 * So t itself may be opaque (one sees the face of an object), and a source sees its own cell.
 *   seen_mask      uint64 [N], 8-byte aligned: bit s is set exactly when from_cells[s] >= 0 and source s sees cell i
 *   cells          int32 [K]: the slot's cells
 *   seen_cells     int32 [S, K]: the cells of slot k that source s sees
 *   near_key       uint64 [S, K], 8-byte aligned: the minimum over those cells of ((uint64)d2 << 32) | cell, d2 the squared distance
 *                  from the source; all ones where there are none
 *   near_d2, near_cell  int32 [S, K]: the two halves of near_key; INT_MAX and -1 where there are none.  near_cell is the nearest
 *                  visible cell of the object, the lowest on a tie
 *   best_key       uint64 [K], 8-byte aligned: the maximum over the used sources with seen_cells[s, k] > 0 of
 *                  ((uint64)seen_cells[s, k] << 32) | (uint32)~s; 0 where there are none
 *   best_seen, best_source  int32 [K]: the two halves of best_key; 0 and -1 where there are none.  best_source is the source that
 *                  sees most of the object, the lowest s on a tie
 *   source_counts  int32 [S, 2]: the transparent and the opaque cells source s sees, both by the map's labels (the source's own
 *                  cell counts by its label); 0, 0 for an unused source
 *   counts         int32 [3]: opaque cells, transparent cells, cells with a nonzero seen_mask
 *   status         int32 [2]: status[0] bit 1: a bounded in-kernel loop reached its bound, the outputs are void (the loops of this
 *                  build are bounded by 64, rows and cols and cannot, so it holds 0); status[1] is reserved (0).
 * Every output may hold anything on entry.  Every output is a pure function of the inputs: integer comparisons, additions,
 * multiplications and atomics (add, min, max, or) only, the same bits on every call, staged or not.
 * Hand-worked maps, all with range2 = INT_MAX, `seen` by rows (1: the source sees the cell):
 *   A. 5 x 7, all -1 but label 9 at (1, 2) and label 4 at (2, 3), the source cell 14 = (2, 0):
 *        1110000  1110000  1111000  1111111  1111111
 *   B. 3 x 3, label 1 at (0, 1), label 2 at (1, 0), the source cell 0:   110  100  000
 *      (the step from cell 0 to cell 4 goes between two opaque cells that touch at a corner)
 *   C. 3 x 3, only label 1 at (0, 1), the source cell 0:   110  111  111   (one corner hides nothing)
 *   D. 3 x 5, only label 1 at (1, 2).  From cell 0:   11111  11100  11100;   from cell 14:   00111  00111  11111.
 *      Cell 0 does not see cell 9 = (1, 4): line cell 2 is row rnd(2, 4) = 1, the opaque (1, 2).  Cell 9 sees cell 0: its line
 *      cells are (1, 3), (0, 2), (0, 1).  This is the asymmetry.
 * workspace: eod_map_sight_workspace_bytes(N, cols) bytes, 8-byte aligned, any contents: one byte per cell (transparent or opaque,
 * and the slot) and one bit per cell (the opacity bit plane, one 64-bit word per 64 consecutive cells).
 * EOD_ERR_BAD_DIMS, before any launch: N, K, P, S or range2 out of range, cols < 1, N % cols != 0, rows or cols above
 * EOD_SIGHT_DIM_MAX, or (from_cells not null) an entry of from_cells >= N; then EOD_ERR_NULL (passable may be null only when
 * P == 0); then EOD_ERR_ALIGN (seen_mask, near_key, best_key and workspace 8 bytes, the others 4); then EOD_ERR_CAPACITY:
 * workspace_bytes too small.  eod_map_sight_workspace_bytes gives 0 for dimensions the call refuses. */
size_t eod_map_sight_workspace_bytes(int N, int cols);
int eod_map_sight(const int32_t* object_labels, const int32_t* objects, const int32_t* passable, const int32_t* from_cells, int N,
                  int K, int P, int S, int cols, int range2, uint64_t* seen_mask, int32_t* cells, int32_t* seen_cells,
                  uint64_t* near_key, int32_t* near_d2, int32_t* near_cell, uint64_t* best_key, int32_t* best_seen,
                  int32_t* best_source, int32_t* source_counts, int32_t* counts, int32_t* status, void* workspace,
                  size_t workspace_bytes, eod_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* EOD_SIGHT_H */
