/* The C ABI of the routes on the map of libeod_hip.so: two entry points beside include/eod_hip.h, include/eod_place.h,
 * include/eod_regions.h, include/eod_inventory.h, include/eod_describe.h and include/eod_relations.h, with the same conventions (plain
 * pointers and sizes, EOD_ERR_* status codes, all work queued on the stream passed in, nothing allocates or synchronises).  The typed
 * binding is `ROUTE_SIGNATURES` of embodied_object_detection_amd/_lib.py. */
#ifndef EOD_ROUTE_H
#define EOD_ROUTE_H
#include "eod_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define EOD_ROUTE_K_MAX 64            /* objects of one call: one wave looks a label up, one 64-bit mask holds the slots a cell touches */
#define EOD_ROUTE_P_MAX 64            /* passable labels of one call: the same wave looks them up */
#define EOD_ROUTE_N_MAX 4194304       /* cells: a path has fewer than N moves, so a cost is below 7 * 2^22 < 2^31 and never INT_MAX */
#define EOD_ROUTE_DIM_MAX 32767       /* rows and columns */
#define EOD_ROUTE_PATH_MAX 1024       /* cells of one path written */
#define EOD_ROUTE_SWEEPS_MAX 1024     /* sweep launches one call queues */
#define EOD_ROUTE_COST_ORTH 5         /* a move along a row or a column */
#define EOD_ROUTE_COST_DIAG 7         /* a diagonal move: the octile distance with sqrt(2) taken as 7 / 5 */
#ifndef EOD_ROUTE_TILE_ROWS           /* the cells one workgroup of a sweep owns: a build-time choice (their product a multiple of 256, */
#define EOD_ROUTE_TILE_ROWS 32        /* the columns a power of two).  No output depends on them, only the number of sweeps a map needs: */
#define EOD_ROUTE_TILE_COLS 32        /* about one per tile border a shortest path crosses, plus two */
#endif

/* Shortest paths round the objects of a label map, from one cell to every cell and to each of up to 64 objects.
 *   object_labels  int32 [N], N = rows * cols, cell i = r * cols + c: object_labels of eod_map_inventory or any other label map
 *   objects        int32 [K], 1 <= K <= EOD_ROUTE_K_MAX: the labels asked for, -1 (any negative value) in unused slots
 *   passable       int32 [P], 0 <= P <= EOD_ROUTE_P_MAX: labels that do not block (a rug, a floor class); NULL when P == 0
 *   1 <= N <= EOD_ROUTE_N_MAX, cols >= 1, N % cols == 0, rows = N / cols and cols <= EOD_ROUTE_DIM_MAX
 *   from_cell 0..N-1: the start;  path_max 1..EOD_ROUTE_PATH_MAX;  sweeps 1..EOD_ROUTE_SWEEPS_MAX;  resume 0 or 1
 * SLOT, as in eod_describe_pool and eod_map_relations: cell i belongs to the lowest slot k with objects[k] == object_labels[i] and
 * objects[k] >= 0.  A later duplicate slot gets no cells.
 * FREE: a cell is free when its label is negative, or its label is one of passable, or it is from_cell (the robot stands there,
 * whatever the label says).  Every other cell is blocked.
 * MOVE: from a free cell to one of its 8 neighbours on the rows and columns of the grid: (r, cols - 1) and (r + 1, 0) are not
 * neighbours, and outside the grid there is no cell.  The target must be free.  A diagonal move from (r, c) to (r + dr, c + dc) also
 * needs (r + dr, c) and (r, c + dc) free: no squeezing between two objects that touch at a corner.  A move along a row or a column
 * costs EOD_ROUTE_COST_ORTH, a diagonal move EOD_ROUTE_COST_DIAG.
 *   dist        int32 [N]: the smallest cost of a path of moves from from_cell; 0 at from_cell; INT_MAX for blocked cells and for
 *               free cells no path reaches
 *   parent      int32 [N]: for a reached free cell i other than from_cell the lowest cell j from which a legal move of cost w into
 *               i has dist[j] + w == dist[i]; -1 for from_cell, blocked cells and unreached cells
 *   goal_key    uint64 [K], 8-byte aligned: over the reached free cells g that touch the slot (some cell of the slot, g itself
 *               included, is at most one row and one column from g: d2 <= 2) the minimum of (dist[g] << 32) | g; all ones where none
 *   goal_cost   int32 [K]: the upper half of goal_key; INT_MAX where goal_key is all ones
 *   goal_cell   int32 [K]: the lower half of goal_key: the free cell beside the object to stop on, the lowest such cell on ties; -1
 *   cells       int32 [K]: the slot's cells
 *   path        int32 [K, path_max]: path[k, 0] = goal_cell[k], path[k, t + 1] = parent[path[k, t]], until from_cell has been
 *               written or path_max cells have been; -1 behind that
 *   path_cells  int32 [K]: the cells written; the path is complete exactly when its last cell is from_cell
 *   counts      int32 [2]: free cells, reached free cells
 *   status      int32 [2]: status[0] is 0 or a bit set: bit 0: the sweeps ran out while a tile had still lowered a value in the last
 *               one; bit 1: a bounded in-kernel loop reached its bound.  With a nonzero status[0] every output but dist is void.
 *               status[1] is reserved (0).
 * Every output may hold anything on entry, except dist when resume == 1: it then holds the dist an earlier call on the same
 * object_labels, passable and from_cell left (whatever that call's status[0] bit 0 says), and the sweeps continue from it instead of
 * starting over.  Every value ever stored in dist is INT_MAX or the cost of a real path, and values only fall; at status[0] == 0
 * dist is the one fixed point, so every output is a pure function of the inputs: the same bits on every call, whatever the number of
 * sweeps and resumed calls that led there.  Integer comparisons, additions and atomics (min, add, or) only.
 * workspace: eod_map_route_workspace_bytes(N, cols) bytes, 8-byte aligned, any contents: one byte per cell (free or blocked, and
 * the slot) and three activity flags per tile.  The same workspace need not be passed to a resumed call.
 * EOD_ERR_BAD_DIMS, before any launch: N, K, P, from_cell, path_max, sweeps or resume out of range, cols < 1, N % cols != 0, rows or
 * cols above EOD_ROUTE_DIM_MAX; then EOD_ERR_NULL (passable may be null only when P == 0); then EOD_ERR_ALIGN (goal_key and workspace 8
 * bytes, the others 4); then EOD_ERR_CAPACITY: workspace_bytes too small.  eod_map_route_workspace_bytes gives 0 for dimensions the
 * call refuses. */
size_t eod_map_route_workspace_bytes(int N, int cols);
int eod_map_route(const int32_t* object_labels, const int32_t* objects, const int32_t* passable, int N, int K, int P, int cols,
                  int from_cell, int path_max, int sweeps, int resume, int32_t* dist, int32_t* parent, uint64_t* goal_key,
                  int32_t* goal_cost, int32_t* goal_cell, int32_t* cells, int32_t* path, int32_t* path_cells, int32_t* counts,
                  int32_t* status, void* workspace, size_t workspace_bytes, eod_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* EOD_ROUTE_H */
