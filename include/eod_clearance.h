/* The C ABI of the clearance map of libeod_hip.so: two entry points beside include/eod_hip.h, include/eod_place.h,
 * include/eod_regions.h, include/eod_inventory.h, include/eod_describe.h, include/eod_relations.h and include/eod_route.h, with the
 * same conventions (plain pointers and sizes, EOD_ERR_* status codes, all work queued on the stream passed in, nothing allocates or
 * synchronises).  The typed binding is `CLEARANCE_SIGNATURES` of embodied_object_detection_amd/_lib.py. */
#ifndef EOD_CLEARANCE_H
#define EOD_CLEARANCE_H
#include "eod_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define EOD_CLEARANCE_K_MAX 64        /* objects of one call: one wave looks a label up */
#define EOD_CLEARANCE_P_MAX 64        /* passable labels of one call: the same wave looks them up */
#define EOD_CLEARANCE_N_MAX 4194304   /* cells: the limits of eod_map_route */
#define EOD_CLEARANCE_DIM_MAX 32767   /* rows and columns: a squared distance is at most 2 * 32766^2 = 2147221512 < 2^31 - 1 */
#define EOD_CLEARANCE_TILE_ROWS 4     /* the rows one workgroup of the row pass owns: one wave each */
#define EOD_CLEARANCE_CHUNK_COLS 64   /* the columns of a row one wave of the row pass owns: one lane each */
#define EOD_CLEARANCE_HALO_COLS 64    /* the columns either side of a chunk it stages beside the chunk; further out it reads memory */

/* The exact squared distance from every cell of a label map to the nearest blocked cell, that cell, and the map inflated by a body.
 *   object_labels  int32 [N], N = rows * cols, cell i = r * cols + c: object_labels of eod_map_inventory or any other label map
 *   objects        int32 [K], 1 <= K <= EOD_CLEARANCE_K_MAX: the labels asked for, -1 (any negative value) in unused slots
 *   passable       int32 [P], 0 <= P <= EOD_CLEARANCE_P_MAX: labels that do not block; NULL only when P == 0
 *   1 <= N <= EOD_CLEARANCE_N_MAX, cols >= 1, N % cols == 0, rows = N / cols and cols <= EOD_CLEARANCE_DIM_MAX
 *   radius2  0 <= radius2 < INT_MAX: the radius of the robot's body, squared, in cells
 *   keep_cell  -1, or 0..N-1: the cell the robot stands on
 * SLOT, as in eod_map_route: cell i belongs to the lowest slot k with objects[k] == object_labels[i] and objects[k] >= 0.  A later
 * duplicate slot gets no cells.
 * BLOCKED: a cell is blocked when its label is >= 0 and is not one of passable.  Every other cell is free.  keep_cell does not
 * change this.
 *   d2          int32 [N]: the minimum over the blocked cells j of (ri - rj)^2 + (ci - cj)^2 on the rows and columns of the grid
 *               ((r, cols - 1) and (r + 1, 0) are cols - 1 columns apart, not one); 0 for a blocked cell; INT_MAX when the map has
 *               no blocked cell.  A real distance is at most 2 * (EOD_CLEARANCE_DIM_MAX - 1)^2 < INT_MAX, so never INT_MAX.
 *   nearest     int32 [N]: the lowest blocked cell j that attains d2[i]; i itself for a blocked cell; -1 when there is none
 *   owner       int32 [N]: object_labels[nearest[i]], or -1
 *   inflated    int32 [N]: object_labels[i] for a blocked cell; for a free cell owner[i] when d2[i] <= radius2, unless keep_cell >= 0
 *               and the squared distance from i to keep_cell is <= radius2 (the robot's own footprint already fits where it
 *               stands); otherwise object_labels[i].  With radius2 == 0 inflated equals object_labels bit for bit.
 *   cells       int32 [K]: the slot's cells
 *   territory   int32 [K]: the free cells whose nearest cell belongs to slot k
 *   widest_key  uint64 [K], 8-byte aligned: the maximum over those cells of ((uint64)d2 << 32) | (uint32)~i, so the lowest cell
 *               wins a tie; 0 where there are none
 *   widest_d2, widest_cell  int32 [K]: the upper half of widest_key, and the cell of its lower half; 0 and -1 where there are none
 *   open_key    uint64 [1], 8-byte aligned: the same maximum over all free cells, the most open place of the map; 0 when no cell
 *               is free
 *   counts      int32 [3]: blocked cells, free cells, free cells with inflated[i] != object_labels[i]
 *   status      int32 [2]: status[0] bit 1: a bounded in-kernel loop reached its bound, the outputs are void (the loops of this
 *               build are bounded by rows and cols and cannot, so it holds 0); status[1] is reserved (0).
 * Every output may hold anything on entry.  Every output is a pure function of the inputs: integer comparisons, multiplications,
 * additions and atomics (max, add) only, the same bits on every call and for every tile, chunk and halo size.
 * Two hand-worked maps.  The 3 x 4 map [[-1,-1,-1,-1],[-1,5,-1,-1],[-1,-1,-1,6]] with objects = [6, 5], radius2 = 1, keep_cell = -1:
 *   d2        = [2,1,2,4, 1,0,1,1, 2,1,1,0]
 *   nearest   = [5,5,5,11, 5,5,5,11, 5,5,11,11]     (cell 3 is 5 from cell 5 and 4 from cell 11, cell 7 is 4 and 1)
 *   inflated  = [-1,5,-1,-1, 5,5,5,6, -1,5,6,6]
 *   cells = [1,1], territory = [3,7], widest_d2 = [4,2], widest_cell = [3,0], counts = [2,10,6], open_key = (4 << 32) | ~3
 * The 1 x 3 map [[3,-1,4]]: d2[1] = 1, nearest[1] = 0, owner[1] = 3: the lowest cell wins the tie.
 * workspace: eod_map_clearance_workspace_bytes(N, cols) bytes, 8-byte aligned, any contents: one byte per cell (free or blocked,
 * and the slot) and one int32 per cell (the row of the nearest blocked cell of its column).
 * EOD_ERR_BAD_DIMS, before any launch: N, K, P, radius2 or keep_cell out of range, cols < 1, N % cols != 0, rows or cols above
 * EOD_CLEARANCE_DIM_MAX; then EOD_ERR_NULL (passable may be null only when P == 0); then EOD_ERR_ALIGN (widest_key, open_key and
 * workspace 8 bytes, the others 4); then EOD_ERR_CAPACITY: workspace_bytes too small.  eod_map_clearance_workspace_bytes gives 0 for
 * dimensions the call refuses. */
size_t eod_map_clearance_workspace_bytes(int N, int cols);
int eod_map_clearance(const int32_t* object_labels, const int32_t* objects, const int32_t* passable, int N, int K, int P, int cols,
                      int radius2, int keep_cell, int32_t* d2, int32_t* nearest, int32_t* owner, int32_t* inflated, int32_t* cells,
                      int32_t* territory, uint64_t* widest_key, int32_t* widest_d2, int32_t* widest_cell, uint64_t* open_key,
                      int32_t* counts, int32_t* status, void* workspace, size_t workspace_bytes, eod_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* EOD_CLEARANCE_H */
