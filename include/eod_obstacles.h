/* The C ABI of the obstacles on the map of libeod_hip.so: three entry points beside include/eod_hip.h, include/eod_place.h,
 * include/eod_regions.h, include/eod_inventory.h, include/eod_describe.h, include/eod_relations.h, include/eod_route.h,
 * include/eod_clearance.h, include/eod_sight.h and include/eod_frontier.h, with the same conventions (plain pointers and sizes,
 * EOD_ERR_* status codes, all work queued on the stream passed in, nothing allocates or synchronises).  The typed binding is
 * `OBSTACLES_SIGNATURES` of embodied_object_detection_amd/_lib.py. */
#ifndef EOD_OBSTACLES_H
#define EOD_OBSTACLES_H
#include "eod_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define EOD_OBSTACLES_K_MAX 64             /* object slots of one call: one wave looks a label up */
#define EOD_OBSTACLES_TOPK_MAX 64          /* ranked structures of one call */
#define EOD_OBSTACLES_N_MAX 4194304        /* cells: the limit of eod_map_frontier */
#define EOD_OBSTACLES_DIM_MAX 32767        /* rows and columns, as in eod_map_frontier */
#define EOD_OBSTACLES_PIXELS_MAX 16777216  /* pixels of one call of eod_map_heights */
#define EOD_OBSTACLES_BAND_MAX 1000000     /* |band_lo_mm|, |band_hi_mm| and the |millimetres| of a valid pixel are at most this */
#define EOD_OBSTACLES_UNSEEN 0             /* the kinds of a cell */
#define EOD_OBSTACLES_CLEAR 1
#define EOD_OBSTACLES_OBSTACLE 2
#define EOD_OBSTACLES_OBJECT 3

/* THE HEIGHT RECORD.  Pixel p has the cell c = proj_indices[p] and the height y = height[p * height_stride] (the world y of
 * eod_unproject_grid_index: `xyz + 1` with stride 3 reads the height column of its xyz output in place).  The pixel is VALID when
 * 0 <= c < N, c != exclude_cell, y is finite and |y| <= 1000.0f; every other pixel is dropped and never used as an index (the rule
 * of eod_map_cover; zero-depth pixels land in the robot's own cell, which is what exclude_cell is for).  A valid pixel has
 *   q = (int)rintf(__fmul_rn(y, 1000.0f))     millimetres: one fp32 product, ties to even (numpy: np.rint(np.float32(y) *
 *                                             np.float32(1000))); |q| <= EOD_OBSTACLES_BAND_MAX
 * and does
 *   hits[c] += 1;  band_hits[c] += (band_lo_mm <= q && q <= band_hi_mm);  h_min_mm[c] = min(h_min_mm[c], q);
 *   h_max_mm[c] = max(h_max_mm[c], q).
 * The band is tested on the rounded millimetres, both edges inside.
 *   proj_indices  int32 [P], 0 <= P <= EOD_OBSTACLES_PIXELS_MAX;  height  float [(P - 1) * height_stride + 1], height_stride >= 1
 *   hits, band_hits, h_min_mm, h_max_mm  int32 [N], 1 <= N <= EOD_OBSTACLES_N_MAX: READ AND WRITTEN, the only such arguments of
 *                 this header.  The caller makes them once with 0, 0, INT_MAX, INT_MIN
 *   band_lo_mm <= band_hi_mm, both within +-EOD_OBSTACLES_BAND_MAX;  exclude_cell: any int (-1: none)
 * One launch, integer atomics (add, min, max) only: the record depends neither on the order of the pixels, nor on that of the
 * frames, nor on how a frame's pixels are split over calls.  The counters are plain 32-bit adds: a cell overflows after 2^31 valid
 * pixels.
 * Hand-worked record: one row of 6 cells, band 100..1500, exclude_cell 5, the pixels as (cell, y)
 *     (0, 0.0) (0, -0.25) (1, 0.5) (1, 1.25) (1, 2.0) (2, 0.0625) (2, 0.099609375) (2, 1.5009765625) (3, NaN) (3, inf) (-1, 0.5)
 *     (6, 0.5) (5, 0.5) (4, 1000.5) (4, 1.5)
 *   millimetres 0, -250, 500, 1250, 2000, 62, 100, 1501 and 1500 for the last one: 62.5 rounds to 62 (ties to even); 99.609375 rounds
 *   to 100 and is in the band (rounding comes before the band test); 1500.9765625 rounds to 1501 and is not.  Six pixels are dropped.
 *   (hits, band_hits, min, max):  cell 0 (2, 0, -250, 0);  cell 1 (3, 2, 500, 2000);  cell 2 (3, 1, 62, 1501);
 *   cell 3 (0, 0, INT_MAX, INT_MIN);  cell 4 (1, 1, 1500, 1500);  cell 5 untouched.
 * EOD_ERR_BAD_DIMS, before any launch: P, N, height_stride or the band out of range; then EOD_ERR_NULL (proj_indices and height may
 * be null only when P == 0); then EOD_ERR_ALIGN (4 bytes).  P == 0 queues nothing. */
int eod_map_heights(const int32_t* proj_indices, const float* height, int height_stride, int P, int N, int band_lo_mm, int band_hi_mm,
                    int exclude_cell, int32_t* hits, int32_t* band_hits, int32_t* h_min_mm, int32_t* h_max_mm, eod_stream_t stream);

/* THE OBSTACLES: which cells something stands in, joined into structures, merged with the detected objects into one label map.
 *   hits, band_hits, h_min_mm, h_max_mm  int32 [N]: the record of eod_map_heights, read only
 *   object_labels  int32 [N] or NULL: object_labels of eod_map_inventory or any other label map
 *   objects        int32 [K_obj], 0 <= K_obj <= EOD_OBSTACLES_K_MAX: labels to report on; NULL only when K_obj == 0
 *   1 <= N <= EOD_OBSTACLES_N_MAX, cols >= 1, N % cols == 0, rows = N / cols and cols <= EOD_OBSTACLES_DIM_MAX, cell i = r * cols + c
 *   min_hits >= 1;  min_cells >= 1;  topk K in 1..EOD_OBSTACLES_TOPK_MAX
 * KIND: every cell is exactly one of, tested in this order,
 *   OBJECT   3  object_labels is given and the cell's label is >= 0, whatever the record says
 *   OBSTACLE 2  band_hits >= min_hits
 *   CLEAR    1  hits > 0
 *   UNSEEN   0  otherwise
 * STRUCTURE: an 8-connected component of OBSTACLE cells on the rows and columns of the grid; a row's end is not next to the
 * following row's start, and outside the grid there is no cell.  Its LABEL is its lowest cell, as everywhere in this library.  A
 * structure of fewer than min_cells cells is a SPECK (depth noise, a flying pixel at an object's edge).
 * Per cell:
 *   kind              uint8 [N]
 *   structure_labels  int32 [N]: the structure's label on every OBSTACLE cell, specks included, -1 elsewhere
 *   merged_labels     int32 [N]: the object's label on an OBJECT cell, the structure's label on an OBSTACLE cell whose structure is no
 *                     speck, -1 elsewhere.  This is the label map that eod_map_route, eod_map_clearance, eod_map_sight and
 *                     eod_map_frontier take as it stands.  With lowest-cell object labels, as eod_map_inventory makes them, an
 *                     object's label and a structure's label are never equal: each is a cell of its own component, and kind[label]
 *                     tells which of the two it is.  Other label maps are the caller's concern.
 * Per structure: the structures with area >= min_cells are counted in count[0]; the K of them with the largest
 * (area << 32) | ~label fill slots 0..K-1 in descending order (the lowest label wins a tie).  int32 unless said otherwise:
 *   structure [K] (the label), area [K], bbox [K, 4] (min row, min col, max row, max col), sum_rc uint64 [K, 2] (the sums of its
 *   cells' rows and columns), top_mm [K] (the maximum of h_max_mm over its cells).  A padding slot holds -1, 0, zeros, zeros,
 *   INT_MIN.
 * Per object slot: a cell with the label l >= 0 belongs to the lowest slot k with objects[k] == l (a negative objects[k] is an
 * unused slot): the rule of eod_map_route.  A later duplicate and an unused slot hold the values of an object without cells.
 *   obj_cells [K_obj], obj_seen_cells [K_obj] (its cells with hits > 0), obj_top_mm [K_obj] (the maximum of h_max_mm over those,
 *   INT_MIN if none), obj_base_mm [K_obj] (the minimum of h_min_mm over those, INT_MAX if none): how high the table is.  The four may
 *   be null only when K_obj == 0.  Without object_labels no cell belongs to any slot.
 *   counts  int32 [6]: UNSEEN, CLEAR, OBSTACLE and OBJECT cells, structures (specks included), speck cells
 *   status  int32 [2]: status[0] bit 1 (value 2): a bounded in-kernel loop reached its bound, the outputs are void (the loops are
 *           bounded by the number of cells they descend through and cannot, so it holds 0); status[1] is reserved (0).
 * Every output may hold anything on entry.  Every output is a pure function of the inputs: integer comparisons, additions and
 * atomics (add, min, max) only, the same bits on every call.
 * Hand-worked map: 4 x 6 cells, min_hits 2, min_cells 2.  Cells 13 and 14 carry the object label 13; band_hits is 2 or more on the
 * cells 0, 1, 8, 16 and on 13 (5; the object wins), 1 on cell 9 (below min_hits); hits is 0 on the cells 4, 5, 10, 11, 17, 23 and
 * on cell 14 (an object never seen), positive elsewhere.
 *     kinds by rows (# OBSTACLE, . CLEAR, ? UNSEEN, O OBJECT, s an OBSTACLE cell that ends as a speck)
 *         ##..??   ..#.??   .OO.s?   .....?
 *   counts = 6, 12, 4, 2, 2, 1 and count = 1.  Structure 0 = {0, 1, 8}, joined across the corner (0, 1)-(1, 2): area 3, bbox 0 0 1 2,
 *   sum_rc 1 3, top_mm the largest of the three h_max_mm.  Cell 16: structure_labels 16, merged_labels -1.  merged_labels is 0 on
 *   {0, 1, 8}, 13 on {13, 14} and -1 elsewhere.  With objects = [13]: obj_cells 2, obj_seen_cells 1, top and base from cell 13 alone.
 *   With min_cells 1: count 2, counts = 6, 12, 4, 2, 2, 0, no speck, merged_labels[16] = 16.
 *   With object_labels NULL: cell 13 is OBSTACLE and cell 14 UNSEEN; (1, 2) and (2, 1) touch at a corner, so 13 joins {0, 1, 8}:
 *   counts = 7, 12, 5, 0, 2, 1, count = 1, structure 0 = {0, 1, 8, 13}: area 4, bbox 0 0 2 2, sum_rc 3 4; obj_cells 0.
 * workspace: eod_map_obstacles_workspace_bytes(N, cols) bytes, 8-byte aligned, any contents: three int32 per cell (the parents, the
 * slots and the areas of the structures) and the raw status.
 * EOD_ERR_BAD_DIMS, before any launch: N, K_obj, min_hits, min_cells or topk out of range, cols < 1, N % cols != 0, rows or cols
 * above EOD_OBSTACLES_DIM_MAX; then EOD_ERR_NULL (object_labels may always be null; objects and the four obj_ outputs only when
 * K_obj == 0); then EOD_ERR_ALIGN (sum_rc and workspace 8 bytes, kind 1, the others 4); then EOD_ERR_CAPACITY: workspace_bytes too
 * small.  eod_map_obstacles_workspace_bytes gives 0 for dimensions the call refuses. */
size_t eod_map_obstacles_workspace_bytes(int N, int cols);
int eod_map_obstacles(const int32_t* hits, const int32_t* band_hits, const int32_t* h_min_mm, const int32_t* h_max_mm,
                      const int32_t* object_labels, const int32_t* objects, int N, int cols, int K_obj, int min_hits, int min_cells,
                      int topk, uint8_t* kind, int32_t* structure_labels, int32_t* merged_labels, int32_t* count, int32_t* structure,
                      int32_t* area, int32_t* bbox, uint64_t* sum_rc, int32_t* top_mm, int32_t* obj_cells, int32_t* obj_seen_cells,
                      int32_t* obj_top_mm, int32_t* obj_base_mm, int32_t* counts, int32_t* status, void* workspace,
                      size_t workspace_bytes, eod_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* EOD_OBSTACLES_H */
