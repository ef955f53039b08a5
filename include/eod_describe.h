/* The C ABI of the object descriptions of libeod_hip.so: entry points beside include/eod_hip.h, include/eod_place.h,
 * include/eod_regions.h and include/eod_inventory.h, with the same conventions (plain pointers and sizes, EOD_ERR_* status codes, all
 * work queued on the stream passed in, nothing allocates or synchronises).  The typed binding is `DESCRIBE_SIGNATURES` of
 * embodied_object_detection_amd/_lib.py. */
#ifndef EOD_DESCRIBE_H
#define EOD_DESCRIBE_H
#include "eod_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define EOD_DESCRIBE_D 512           /* the width of a memory row and of an embedding (CLIP space) */
#define EOD_DESCRIBE_K_MAX 64        /* objects of one call: one wave looks a label up */
#define EOD_DESCRIBE_N_MAX 4194304   /* cells: 2^22 cells of at most 2^30 each stay below 2^53 */
#define EOD_DESCRIBE_C_MAX 2047      /* classes of a vocabulary, the background column not counted */
#define EOD_DESCRIBE_TOPN_MAX 8

/* Pool the memory rows of the cells of each object: one direction per object, whatever the order of its cells.
 *   mem            float32 [N, 512], 16-byte aligned: the memory's sum rows (a direction does not depend on the scale, so the
 *                  observation counts are not needed)
 *   object_labels  int32 [N]: object_labels of eod_map_inventory, a row of region_labels of eod_map_regions, or any other label map
 *   objects        int32 [K], 1 <= K <= EOD_DESCRIBE_K_MAX: the labels to describe, -1 (any negative value) in unused slots
 *   1 <= N <= EOD_DESCRIBE_N_MAX
 * SLOT: cell i belongs to the lowest slot k with objects[k] == object_labels[i] and objects[k] >= 0.  A later duplicate slot gets no
 * cells.  A cell whose label is in no slot (-1, any negative value, a label that was not asked for) is skipped; its row is not read.
 * NORMALISATION, per cell of a slot, in fp32: s = sum_c mem[i, c]^2 (the order of this sum is the kernel's own, with or without
 * fused multiply-adds; it is one fixed order, and it is not that of the semantic map's row prologue), n = sqrt(s), n = 1e-12f where
 * n < 1e-12f (a NaN stays a NaN, as in torch.clamp_min), x[c] = mem[i, c] / n.
 * NON-FINITE: where x[c] is not finite it counts as 0, BEFORE anything else is done with it: a row that holds an Inf or a NaN, or
 * whose sum of squares overflows, has n = Inf or NaN and so contributes zeros in every channel (finite / Inf = 0, Inf / Inf = NaN);
 * its cell is counted all the same.  Then x[c] is clamped to [-1, 1].  No Inf and no NaN reaches the float-to-int conversion.
 * FIXED POINT: q[c] = (int32)(x[c] * 1073741824.0f).  The product is exact (a power of two, |x| <= 1) and the conversion truncates
 * (towards zero).
 *   sum_q      int64 [K, 512], 8-byte aligned: the sum of q[c] over the slot's cells
 *   cells      int32 [K]: their count
 * Integer atomics only: given the x values every output is a pure function of the inputs, independent of order, grid and scheduling
 * (the argument of mass_q24 of include/eod_regions.h).  sum_q and cells may hold anything on entry.
 * EMBEDDING, in fp64: mean[k, c] = (double)sum_q[k, c] / ((double)cells[k] * 2^30), norm = sqrt(sum_c mean[k, c]^2) in a fixed order.
 *   coherence  float32 [K]: (float)norm.  1 when all cells point the same way, near 0 for an object that mixes unrelated things
 *   embedding  float32 [K, 512], 16-byte aligned: (float)(mean / norm)
 * Slots with cells == 0 or norm == 0 get zeros in both.
 * EOD_ERR_BAD_DIMS, before any launch: K outside 1..EOD_DESCRIBE_K_MAX, N outside 1..EOD_DESCRIBE_N_MAX; then EOD_ERR_NULL, then
 * EOD_ERR_ALIGN (mem and embedding 16 bytes, sum_q 8, the others 4). */
int eod_describe_pool(const float* mem, const int32_t* object_labels, const int32_t* objects, int N, int K, int64_t* sum_q,
                      int32_t* cells, float* embedding, float* coherence, eod_stream_t stream);

/* Classify embeddings in any vocabulary: K x C work, no pass over the cells.
 *   embedding  float32 [K, 512], 16-byte aligned: what eod_describe_pool wrote, now or earlier, here or in a snapshot
 *   zs         float32 [512, C1] as the heads and eod_semmap_labels take it; the last column is the background and never enters.
 *              C = C1 - 1, 1 <= C <= EOD_DESCRIBE_C_MAX;  1 <= topn <= min(EOD_DESCRIBE_TOPN_MAX, C)
 *   prob       float32 [K, C]: the softmax over the C classes of 50 * sum_ch embedding[k, ch] * zs[ch, c], in fp32: the sum over ch
 *              ascending, the maximum subtracted, expf, the sum of the C terms in a fixed order, one division per class
 *   top_cls    int32 [K, topn], top_prob float32 [K, topn]: the row's topn entries by (prob descending, class ascending): an exact
 *              function of the bits of prob
 * An all-zero embedding row (+0 or -0 in every channel) is an empty slot: a prob row of zeros, top_cls -1, top_prob 0.
 * Comparisons and fixed summation orders only: two calls give the same bits.
 * EOD_ERR_BAD_DIMS, before any launch: K outside 1..EOD_DESCRIBE_K_MAX, C1 - 1 outside 1..EOD_DESCRIBE_C_MAX, topn outside
 * 1..min(EOD_DESCRIBE_TOPN_MAX, C1 - 1); then EOD_ERR_NULL, then EOD_ERR_ALIGN (embedding 16 bytes, the others 4). */
int eod_describe_classify(const float* embedding, const float* zs, int K, int C1, int topn, float* prob, int32_t* top_cls,
                          float* top_prob, eod_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* EOD_DESCRIBE_H */
