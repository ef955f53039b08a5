/* The C ABI of the rooms on the map of libeod_hip.so: two entry points beside include/eod_hip.h, include/eod_place.h,
 * include/eod_regions.h, include/eod_inventory.h, include/eod_describe.h, include/eod_relations.h, include/eod_route.h,
 * include/eod_clearance.h, include/eod_sight.h, include/eod_frontier.h and include/eod_obstacles.h, with the same conventions (plain
 * pointers and sizes, EOD_ERR_* status codes, all work queued on the stream passed in, nothing allocates or synchronises).  The typed
 * binding is `ROOMS_SIGNATURES` of embodied_object_detection_amd/_lib.py. */
#ifndef EOD_ROOMS_H
#define EOD_ROOMS_H
#include "eod_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define EOD_ROOMS_K_MAX 64            /* object slots of one call: one wave looks a label up, one 64-bit mask holds the slots a cell touches */
#define EOD_ROOMS_P_MAX 64            /* passable labels of one call */
#define EOD_ROOMS_TOPK_MAX 64         /* ranked rooms of one call */
#define EOD_ROOMS_N_MAX 4194304       /* cells: the limit of eod_map_route */
#define EOD_ROOMS_DIM_MAX 32767       /* rows and columns, as in eod_map_route */
#define EOD_ROOMS_SWEEPS_MAX 1024     /* sweep launches one call queues */
#define EOD_ROOMS_TILE_ROWS 32        /* the cells one workgroup of a sweep owns; no output depends on them, only the number of */
#define EOD_ROOMS_TILE_COLS 32        /* sweeps a map needs */

/* THE ROOMS: the free space of a label map split at its doorways, and the objects by room.
 *   labels    int32 [N], N = rows * cols, cell i = r * cols + c: a label map, typically merged_labels of eod_map_obstacles
 *   passable  int32 [P], 0 <= P <= EOD_ROOMS_P_MAX: labels that do not block; NULL only when P == 0
 *   d2        int32 [N]: d2 of eod_map_clearance on the same labels and passable (0 on a blocked cell, INT_MAX on a map without
 *             one).  It is the caller's input: the op does not recompute it
 *   known     uint8 [N] or NULL: a cell with known == 0 is VOID unless it is blocked.  kind of eod_map_obstacles fits as it stands
 *             (EOD_OBSTACLES_UNSEEN is 0)
 *   objects   int32 [K_obj], 0 <= K_obj <= EOD_ROOMS_K_MAX: labels to sort by room, -1 (any negative value) in unused slots; NULL
 *             only when K_obj == 0
 *   1 <= N <= EOD_ROOMS_N_MAX, cols >= 1, N % cols == 0, rows = N / cols and cols <= EOD_ROOMS_DIM_MAX
 *   door_r2 >= 0;  min_cells >= 1;  topk K in 1..EOD_ROOMS_TOPK_MAX;  sweeps in 1..EOD_ROOMS_SWEEPS_MAX
 * BLOCKED, as in eod_map_clearance: the label is >= 0 and not one of passable.  VOID: not blocked, known is given and known[i] == 0.
 * FREE: every other cell.  A void cell is in no room and no move enters it or passes it at a corner.
 * SLOT, as in eod_map_route: cell i belongs to the lowest slot k with objects[k] == labels[i] and objects[k] >= 0, whatever else
 * the cell is.  A later duplicate slot gets no cells.
 * CORE: a free cell with d2 > door_r2: a body that does not fit a doorway fits here.
 * CORE REGION: a 4-connected component of core cells on the rows and columns of the grid; a row's end is not next to the following
 * row's start.  Its LABEL is its lowest cell.  A region of fewer than min_cells cells is no room: its cells count as ordinary free
 * cells from here on.  The others are the ROOMS.
 * GROW: every free cell gets the key (g << 32) | room: g is the smallest cost of a path of MOVEs of eod_map_route (5 along a row or
 * column, 7 diagonally and then both cells passed between free too; free cells only) from any cell of any room's core, room the
 * lowest label among the rooms that attain g.  It is the one fixed point of key[i] = min(key[i], key[j] + (w << 32)) over the
 * legal moves j -> i of cost w, the cores of the rooms starting at (0 << 32) | label.  A free cell no path reaches is UNASSIGNED.
 * Per cell, int32 [N]:
 *   room_labels  the room's label, on the cells of unranked rooms too; -1 on blocked, void and unassigned cells
 *   grow_dist    0 on a room's core, g on grown cells, INT_MAX elsewhere
 * Per room: count[0] is the number of rooms.  The K rooms with the largest (area << 32) | ~label fill slots 0..K-1 in descending
 * order (the lowest label wins a tie).  int32 unless said otherwise:
 *   room [K] (the label), area [K] (core and grown cells), core_area [K], bbox [K, 4] (min row, min col, max row, max col), sum_rc
 *   uint64 [K, 2] (the sums of its cells' rows and columns), widest_key uint64 [K] (the maximum over its cells of (d2 << 32) | ~cell),
 *   widest_d2 [K], widest_cell [K] (its halves: where to stand in the room), room_objects [K] (below).  A padding slot holds -1, 0,
 *   0, zeros, zeros, 0, 0, -1, 0.
 * Doorways between ranked rooms, for slots a != b:
 *   door_edges  int32 [K, K]: the ordered pairs (i in a, j in b) of 4-neighbours; symmetric
 *   door_key    uint64 [K, K]: the maximum of (d2[i] << 32) | ~i over the cells i of a that have a 4-neighbour in b; 0 where none
 *   door_d2, door_cell  int32 [K, K]: its halves; 0 and -1 where there are none and on the diagonal.  door_cell[a, b] is a cell of
 *               a: the middle of the door, on a's side.  The diagonal of door_edges and door_key holds 0.
 * Objects by room: a free cell TOUCHES slot k when some cell of the slot is at most one row and one column from it (the goal rule
 * of eod_map_route).
 *   obj_room_cells  int32 [K_obj, K]: the cells of ranked room s that touch slot k; a cell that touches several slots counts for each
 *   obj_room        int32 [K_obj]: the slot s with the most such cells, the lowest s on a tie; -1 if none
 *   obj_room_label  int32 [K_obj]: that room's label, or -1
 *   room_objects    int32 [K]: the number of k with obj_room[k] == s
 * The three obj_ outputs may be null only when K_obj == 0.  A wall passed as an object shows up in both rooms it separates.
 *   counts  int32 [6]: blocked, void, free, core cells of rooms, grown cells, unassigned free cells
 *   status  int32 [2]: status[0] bit 0: the sweeps ran out while a tile had still lowered a key in the last one: every output but
 *           the keys (room_labels, grow_dist) is void; bit 1: a bounded in-kernel loop reached its bound.  status[1] is reserved (0).
 * Every output may hold anything on entry.  At status[0] == 0 every output is a pure function of the inputs: integer comparisons,
 * additions and atomics (add, min, max) only, the same bits on every call and for every tile size.
 * Hand-worked map: 7 x 11 cells, label 0 on the whole border and on column 5 except cell 38 = (3, 5), the door; -1 elsewhere.
 * door_r2 = 1, min_cells = 1, known NULL, objects = [0].  d2 by rows of the interior (rows 1..5, columns 1..9):
 *     1 1 1 1 0 1 1 1 1
 *     1 4 4 1 0 1 4 4 1
 *     1 4 5 2 1 2 5 4 1
 *     1 4 4 1 0 1 4 4 1
 *     1 1 1 1 0 1 1 1 1
 *   Cores: {24, 25, 35, 36, 37, 46, 47} and {29, 30, 39, 40, 41, 51, 52}; cells 37 and 39 have d2 2; the door has d2 1 and is no core.
 *   Rooms 24 and 29, count 2.  grow_dist is 5 or 7 on the rim cells and 5 on the door from both sides, so the door goes to room 24
 *   (the lowest label).
 *   Slot 0 = room 24: area 21, core_area 7, bbox 1 1 5 5, sum_rc 63 55, widest_d2 5 at cell 36.
 *   Slot 1 = room 29: area 20, core_area 7, bbox 1 6 5 9, sum_rc 60 150, widest_d2 5 at cell 40.
 *   door_edges[0,1] = door_edges[1,0] = 1.  door_cell[0,1] = 38 with door_d2 1.  door_cell[1,0] = 39 with door_d2 2.
 *   obj_room_cells[0] = [15, 14], obj_room[0] = 0, room_objects = [1, 0].  counts = [36, 0, 41, 14, 27, 0].
 *   door_r2 = 2: 37 and 39 leave the cores (6 cells each, same labels) and the door's grow_dist is 10; the areas are unchanged.
 *   door_r2 = 0: one room, label 12, area 41, no doorways.
 *   min_cells = 8: no room, every room_labels -1, counts = [36, 0, 41, 0, 0, 41].
 * workspace: eod_map_rooms_workspace_bytes(N, cols) bytes, 8-byte aligned, any contents: five int32, one uint64 and two bytes per
 * cell, three activity flags per tile and the raw status.
 * EOD_ERR_BAD_DIMS, before any launch: N, P, K_obj, door_r2, min_cells, topk or sweeps out of range, cols < 1, N % cols != 0, rows or
 * cols above EOD_ROOMS_DIM_MAX; then EOD_ERR_NULL (known may always be null; passable only when P == 0; objects and the three obj_
 * outputs only when K_obj == 0); then EOD_ERR_ALIGN (sum_rc, widest_key, door_key and workspace 8 bytes, known 1, the others 4);
 * then EOD_ERR_CAPACITY: workspace_bytes too small.  eod_map_rooms_workspace_bytes gives 0 for dimensions the call refuses. */
size_t eod_map_rooms_workspace_bytes(int N, int cols);
int eod_map_rooms(const int32_t* labels, const int32_t* passable, const int32_t* d2, const uint8_t* known, const int32_t* objects, int N,
                  int P, int cols, int K_obj, int door_r2, int min_cells, int topk, int sweeps, int32_t* room_labels, int32_t* grow_dist,
                  int32_t* count, int32_t* room, int32_t* area, int32_t* core_area, int32_t* bbox, uint64_t* sum_rc, uint64_t* widest_key,
                  int32_t* widest_d2, int32_t* widest_cell, int32_t* room_objects, int32_t* door_edges, uint64_t* door_key,
                  int32_t* door_d2, int32_t* door_cell, int32_t* obj_room_cells, int32_t* obj_room, int32_t* obj_room_label,
                  int32_t* counts, int32_t* status, void* workspace, size_t workspace_bytes, eod_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* EOD_ROOMS_H */
