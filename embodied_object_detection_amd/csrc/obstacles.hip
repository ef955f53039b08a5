// Obstacles on the map (eod_map_heights, eod_map_obstacles; semantics in include/eod_obstacles.h): the per-cell record of the heights
// the frames' pixels brought, and from it the cells something stands in, joined into structures and merged with the detected objects
// into one label map for the other map queries.  Read-only queries beside the frame: one fp32 product per pixel, otherwise integers
// and comparisons only, integer atomics only, the result a pure function of the inputs.  One launch of eod_map_heights and nine of
// eod_map_obstacles; what one needs of another is complete at the launch boundary between them, and no workgroup ever waits for
// another one (no spin, no flag, no grid barrier).  The connected components are the union-find of regions.hip on one plane, the
// OBSTACLE cells, 8-connected: the plane takes the place of a class q of regions.hip in the workspace's parent and slot.
//
//   heights_kernel             a workgroup per 1024 pixels, gathered per cell in an LDS table first (below, at the kernel)
//   obstacles_classify_kernel  one thread per cell: its kind.  count, counts, status, the raw status and the object slots to their
//                              neutral values.
//   obstacles_tile_kernel      regions_tile_kernel per 32 x 32 tile: the OBSTACLE cells of the tile joined in LDS
//   obstacles_border_kernel    regions_border_kernel: left, up and the two upper diagonals (at a tile corner the only link).  A
//                              neighbour is foreground where its parent is >= 0.
//   regions_compress_kernel    (regions_common.h)
//   regions_flatten_kernel     (regions_common.h) structure_labels, the structures' areas, counts[2]
//   regions_list_kernel        (regions_common.h) the structures with area >= min_cells: count[0] and the list, in parent
//   obstacles_select_kernel    one workgroup: K rounds of a workgroup-wide maximum of (area << 32) | ~label over the list, below the
//                              previous pick, each leaving slot[root] = k and the slot's outputs at their neutral values
//   obstacles_stats_kernel     every cell: merged_labels; the kinds, the structures and the speck cells counted; bbox, sum_rc and top_mm
//                              of the structures that have a slot and the four values of the object slots, per workgroup in LDS
//                              first, then one global atomic per slot the workgroup touched.  Lane l holds objects[l], the wave
//                              compares a label with all of them at once (frontier_classify_kernel's ballot).  status[0].
//
// THE INVARIANT of regions.hip carries over word for word: every value ever stored in parent[x] is a member of x's component and is
// <= x.  Whether two cells are adjacent depends on the kinds alone, which do not change after the first launch.  The bounds of the
// loops are those of regions.hip (RG_TILE hops in LDS, RG_FIND_CAP and RG_HOOK_CAP globally); a thread that reaches one stops and
// sets the raw status, which the last launch turns into status[0] bit 1.
// BOUNDS: every per-cell array is indexed by i < N or by an 8-neighbour of i that the row and column tests keep inside the grid; a
// label of a structure is a cell; a slot is < K, an object slot < K_obj <= 64; proj_indices' cells are tested against [0, N)
// before they index the record; height is read at p * height_stride for p < P only; a table entry is h < HT_TABLE and its key a
// cell that passed that test.
#include "regions_common.h"
#include "../../include/eod_obstacles.h"

namespace {

static_assert(EOD_OBSTACLES_N_MAX == EOD_REGIONS_N_MAX && EOD_OBSTACLES_TOPK_MAX == EOD_REGIONS_TOPK_MAX, "the shared launches' limits");
static_assert(EOD_OBSTACLES_K_MAX == 64, "one wave looks a label up");

constexpr unsigned char OB_UNSEEN = EOD_OBSTACLES_UNSEEN, OB_CLEAR = EOD_OBSTACLES_CLEAR, OB_OBSTACLE = EOD_OBSTACLES_OBSTACLE,
                        OB_OBJECT = EOD_OBSTACLES_OBJECT;
constexpr int HT_THREADS = 256, HT_PIXELS = 1024;                   // a workgroup's pixels share its LDS table
constexpr int HT_TABLE_LOG2 = 9, HT_TABLE = 1 << HT_TABLE_LOG2, HT_PROBES = 8;

// Whether pixel p counts, and its millimetres.
__device__ __forceinline__ bool heights_pixel(const int* __restrict__ proj, const float* __restrict__ height, int stride, int p, int P,
                                              int N, int exclude_cell, int& c, int& q) {
  c = -1;
  q = 0;
  if (p >= P) return false;
  c = proj[p];
  if (c < 0 || c >= N || c == exclude_cell) return false;
  const float y = height[(size_t)p * stride];
  if (!(fabsf(y) <= 1000.0f)) return false;                           // NaN and the infinities fail the comparison too
  q = (int)rintf(__fmul_rn(y, 1000.0f));
  return true;
}

// n pixels of cell c, b of them in the band, the lowest lo and the highest hi: minima and maxima only shrink and grow, so a stale
// relaxed read costs an atomic at most (frontier_cover_kernel).
__device__ __forceinline__ void heights_commit(int c, int n, int b, int lo, int hi, int* __restrict__ hits, int* __restrict__ band_hits,
                                               int* __restrict__ h_min, int* __restrict__ h_max) {
  atomicAdd(&hits[c], n);
  if (b) atomicAdd(&band_hits[c], b);
  if (agent_ld(&h_min[c]) > lo) atomicMin(&h_min[c], lo);
  if (agent_ld(&h_max[c]) < hi) atomicMax(&h_max[c], hi);
}

// THE RECORD, a workgroup per HT_PIXELS pixels.  Neighbouring pixels share a cell (a 640 x 640 frame lands on a few hundred cells), so
// four global atomics a pixel queue on a few hundred addresses in L2.  The workgroup gathers its pixels per cell in an LDS table
// first (open addressing as in regions_flatten_kernel: the cell is the key, claimed with a compare-and-swap; count, band count,
// minimum and maximum beside it by LDS atomics) and then commits each entry it used once.  A pixel that finds no entry within its
// probes (a workgroup across more than HT_TABLE cells) commits itself: the same sums, minima and maxima in another order, and
// integers do not care.  Measured against one thread per pixel with plain atomics and against a wave that groups its lanes by
// cell (profiles/obstacles_variants.txt).
__global__ __launch_bounds__(HT_THREADS) void heights_kernel(const int* __restrict__ proj, const float* __restrict__ height, int stride,
                                                             int P, int N, int band_lo, int band_hi, int exclude_cell,
                                                             int* __restrict__ hits, int* __restrict__ band_hits,
                                                             int* __restrict__ h_min, int* __restrict__ h_max) {
  __shared__ int key_s[HT_TABLE], n_s[HT_TABLE], b_s[HT_TABLE], lo_s[HT_TABLE], hi_s[HT_TABLE];
  const int tid = threadIdx.x;
  for (int e = tid; e < HT_TABLE; e += HT_THREADS) {
    key_s[e] = -1;
    n_s[e] = 0;
    b_s[e] = 0;
    lo_s[e] = INT_MAX;
    hi_s[e] = INT_MIN;
  }
  __syncthreads();
  for (int j = 0; j < HT_PIXELS / HT_THREADS; ++j) {
    const int p = blockIdx.x * HT_PIXELS + j * HT_THREADS + tid;       // P <= 2^24: no overflow
    int c, q;
    if (!heights_pixel(proj, height, stride, p, P, N, exclude_cell, c, q)) continue;
    const bool in_band = band_lo <= q && q <= band_hi;
    unsigned h = ((unsigned)c * 2654435761u) >> (32 - HT_TABLE_LOG2);
    bool done = false;
    for (int probe = 0; probe < HT_PROBES && !done; ++probe) {
      int old = lds_ld(&key_s[h]);
      if (old == -1) old = atomicCAS(&key_s[h], -1, c);
      if (old == -1 || old == c) {
        atomicAdd(&n_s[h], 1);
        if (in_band) atomicAdd(&b_s[h], 1);
        atomicMin(&lo_s[h], q);
        atomicMax(&hi_s[h], q);
        done = true;
      }
      h = (h + 1) & (HT_TABLE - 1);
    }
    if (!done) heights_commit(c, 1, in_band ? 1 : 0, q, q, hits, band_hits, h_min, h_max);
  }
  __syncthreads();
  for (int e = tid; e < HT_TABLE; e += HT_THREADS)
    if (key_s[e] >= 0) heights_commit(key_s[e], n_s[e], b_s[e], lo_s[e], hi_s[e], hits, band_hits, h_min, h_max);
}

__global__ __launch_bounds__(256) void obstacles_classify_kernel(const int* __restrict__ hits, const int* __restrict__ band_hits,
                                                                 const int* __restrict__ labels, int N, int K_obj, int min_hits,
                                                                 unsigned char* __restrict__ kind, int* __restrict__ count,
                                                                 int* __restrict__ counts, int* __restrict__ status,
                                                                 int* __restrict__ raw, int* __restrict__ obj_cells,
                                                                 int* __restrict__ obj_seen, int* __restrict__ obj_top,
                                                                 int* __restrict__ obj_base) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < N)
    kind[i] = labels && labels[i] >= 0 ? OB_OBJECT : band_hits[i] >= min_hits ? OB_OBSTACLE : hits[i] > 0 ? OB_CLEAR : OB_UNSEEN;
  if (i < 6) counts[i] = 0;
  if (i < 2) status[i] = 0;
  if (i == 0) {
    count[0] = 0;
    raw[0] = 0;
  }
  if (i < K_obj) {
    obj_cells[i] = 0;
    obj_seen[i] = 0;
    obj_top[i] = INT_MIN;
    obj_base[i] = INT_MAX;
  }
}

__global__ __launch_bounds__(RG_THREADS) void obstacles_tile_kernel(const unsigned char* __restrict__ kind, int rows, int cols, int tiles_c,
                                                                     int* __restrict__ parent, int* __restrict__ slot,
                                                                     int* __restrict__ area, int* __restrict__ status) {
  __shared__ int p_s[RG_TILE];
  const int tid = threadIdx.x;
  const int ty = blockIdx.x / tiles_c, tx = blockIdx.x - ty * tiles_c;
  const int r0 = ty * RG_TR, c0 = tx * RG_TC;
  for (int l = tid; l < RG_TILE; l += RG_THREADS) {
    const int r = r0 + l / RG_TC, c = c0 + (l & (RG_TC - 1));
    p_s[l] = r < rows && c < cols && kind[r * cols + c] == OB_OBSTACLE ? l : -1;
  }
  __syncthreads();
  for (int l = tid; l < RG_TILE; l += RG_THREADS) {
    if (lds_ld(&p_s[l]) < 0) continue;
    const int lr = l / RG_TC, lc = l & (RG_TC - 1);
    if (lc > 0 && lds_ld(&p_s[l - 1]) >= 0) tile_union(p_s, l, l - 1, status);
    if (lr > 0) {
      if (lds_ld(&p_s[l - RG_TC]) >= 0) tile_union(p_s, l, l - RG_TC, status);
      if (lc > 0 && lds_ld(&p_s[l - RG_TC - 1]) >= 0) tile_union(p_s, l, l - RG_TC - 1, status);
      if (lc < RG_TC - 1 && lds_ld(&p_s[l - RG_TC + 1]) >= 0) tile_union(p_s, l, l - RG_TC + 1, status);
    }
  }
  __syncthreads();
  for (int l = tid; l < RG_TILE; l += RG_THREADS) {
    const int r = r0 + l / RG_TC, c = c0 + (l & (RG_TC - 1));
    if (r >= rows || c >= cols) continue;
    int v = p_s[l];
    bool local_root = false;
    if (v >= 0) {
      v = tile_find(p_s, v, status);
      local_root = v == l;
      v = (r0 + v / RG_TC) * cols + c0 + (v & (RG_TC - 1));          // the tile's smallest cell of the component: <= this cell
    }
    const int g = r * cols + c;
    parent[g] = v;
    slot[g] = local_root ? -2 : -1;
    area[g] = 0;
  }
}

__global__ __launch_bounds__(RG_THREADS) void obstacles_border_kernel(int* __restrict__ p, int N, int cols, int* __restrict__ status) {
  const int i = blockIdx.x * RG_THREADS + threadIdx.x;
  if (i >= N) return;
  const int r = i / cols, c = i - r * cols;
  const int lr = r & (RG_TR - 1), lc = c & (RG_TC - 1);
  if (lr != 0 && lc != 0 && lc != RG_TC - 1) return;                 // all four neighbours before it are in its own tile
  if (agent_ld(&p[i]) < 0) return;
  // the row and the column are the grid's: c > 0 and c < cols - 1 keep (r, 0) away from (r - 1, cols - 1) and from (r, cols - 1)
  if (lc == 0 && c > 0 && agent_ld(&p[i - 1]) >= 0) grid_union(p, i, i - 1, status);
  if (r > 0) {
    if (lr == 0 && agent_ld(&p[i - cols]) >= 0) grid_union(p, i, i - cols, status);
    if (c > 0 && (lr == 0 || lc == 0) && agent_ld(&p[i - cols - 1]) >= 0) grid_union(p, i, i - cols - 1, status);
    if (c < cols - 1 && (lr == 0 || lc == RG_TC - 1) && agent_ld(&p[i - cols + 1]) >= 0) grid_union(p, i, i - cols + 1, status);
  }
}

struct ObstaclesOut {    // the per-slot arrays of the entry point
  int *structure, *area, *bbox;
  u64* sum_rc;
  int *top_mm, *obj_cells, *obj_seen, *obj_top, *obj_base;
};

__global__ __launch_bounds__(RG_SEL_THREADS) void obstacles_select_kernel(const int* __restrict__ area, int* __restrict__ slot,
                                                                           const int* __restrict__ list, const int* __restrict__ count,
                                                                           int N, int K, const ObstaclesOut o) {
  __shared__ u64 red_s[RG_SEL_THREADS / 64];
  const int tid = threadIdx.x;
  const int n = count[0] < N ? count[0] : N;
  u64 prev = ~0ull;                                                   // above every key
  for (int k = 0; k < K; ++k) {
    u64 best = 0ull;                                                  // below every key: a listed area is at least 1
    if (prev) {                                                       // block-uniform
      for (int j = tid; j < n; j += RG_SEL_THREADS) {
        const int root = list[j];
        const u64 key = ((u64)(unsigned)area[root] << 32) | (unsigned)~root;
        if (key < prev && key > best) best = key;
      }
    }
    prev = block_max_u64(best, red_s);                                // 0 once the structures are used up: the rest is padding
    if (tid == 0) {
      const int root = (int)~(unsigned)prev;
      o.structure[k] = prev ? root : -1;
      o.area[k] = (int)(prev >> 32);
      o.bbox[4 * k + 0] = prev ? INT_MAX : 0;
      o.bbox[4 * k + 1] = prev ? INT_MAX : 0;
      o.bbox[4 * k + 2] = prev ? -1 : 0;
      o.bbox[4 * k + 3] = prev ? -1 : 0;
      o.sum_rc[2 * k] = 0ull;
      o.sum_rc[2 * k + 1] = 0ull;
      o.top_mm[k] = INT_MIN;
      if (prev) slot[root] = k;
    }
  }
}

__global__ __launch_bounds__(RG_THREADS) void obstacles_stats_kernel(const unsigned char* __restrict__ kind, const int* __restrict__ labels,
                                                                      const int* __restrict__ objects, const int* __restrict__ hits,
                                                                      const int* __restrict__ h_min, const int* __restrict__ h_max,
                                                                      const int* __restrict__ structure_labels,
                                                                      const int* __restrict__ area, const int* __restrict__ slot, int N,
                                                                      int cols, int K, int K_obj, int min_cells,
                                                                      int* __restrict__ merged, const ObstaclesOut o,
                                                                      int* __restrict__ counts, const int* __restrict__ raw,
                                                                      int* __restrict__ status) {
  __shared__ int bb_s[EOD_OBSTACLES_TOPK_MAX][4], top_s[EOD_OBSTACLES_TOPK_MAX];
  __shared__ u64 acc_s[EOD_OBSTACLES_TOPK_MAX][2];                    // sum of rows, sum of columns
  __shared__ int obj_s[EOD_OBSTACLES_K_MAX][4];                       // cells, seen cells, top, base
  __shared__ int cnt_s[6];
  const int tid = threadIdx.x, lane = tid & 63;
  if (tid < K) {
    bb_s[tid][0] = INT_MAX; bb_s[tid][1] = INT_MAX; bb_s[tid][2] = -1; bb_s[tid][3] = -1;
    top_s[tid] = INT_MIN;
    acc_s[tid][0] = 0ull; acc_s[tid][1] = 0ull;
  }
  if (tid < EOD_OBSTACLES_K_MAX) {
    obj_s[tid][0] = 0; obj_s[tid][1] = 0; obj_s[tid][2] = INT_MIN; obj_s[tid][3] = INT_MAX;
  }
  if (tid < 6) cnt_s[tid] = 0;
  __syncthreads();
  const bool has_obj = lane < K_obj && objects[lane] >= 0;
  const int obj = has_obj ? objects[lane] : -1;
  const int base = blockIdx.x * RG_STAT_CELLS;
  for (int j = 0; j < RG_STAT_CELLS / RG_THREADS; ++j) {             // every thread stays to the end (ballots)
    const int i = base + j * RG_THREADS + tid;
    const bool in = i < N;
    const int kd = in ? kind[i] : -1;
    const int lab = kd == OB_OBJECT ? labels[i] : -1;
    const int sl = kd == OB_OBSTACLE ? structure_labels[i] : -1;
    const bool kept = sl >= 0 && area[sl] >= min_cells;
    if (in) merged[i] = kd == OB_OBJECT ? lab : kept ? sl : -1;
    // the kinds (OBSTACLE cells are counted by the flatten launch), the structures by their label cells, the speck cells
    const u64 b0 = __ballot(kd == OB_UNSEEN), b1 = __ballot(kd == OB_CLEAR), b3 = __ballot(kd == OB_OBJECT);
    const u64 b4 = __ballot(sl >= 0 && sl == i), b5 = __ballot(sl >= 0 && !kept);
    if (lane == 0) {
      if (b0) atomicAdd(&cnt_s[0], __popcll(b0));
      if (b1) atomicAdd(&cnt_s[1], __popcll(b1));
      if (b3) atomicAdd(&cnt_s[3], __popcll(b3));
      if (b4) atomicAdd(&cnt_s[4], __popcll(b4));
      if (b5) atomicAdd(&cnt_s[5], __popcll(b5));
    }
    if (kept) {
      const int k = slot[sl];
      if (k >= 0) {
        const int r = i / cols, c = i - r * cols;
        atomicMin(&bb_s[k][0], r);
        atomicMin(&bb_s[k][1], c);
        atomicMax(&bb_s[k][2], r);
        atomicMax(&bb_s[k][3], c);
        atomicAdd(&acc_s[k][0], (u64)r);
        atomicAdd(&acc_s[k][1], (u64)c);
        atomicMax(&top_s[k], h_max[i]);
      }
    }
    // the object slot of every distinct label of the wave: the lowest lane that holds it
    int k_obj = -1;
    u64 todo = K_obj > 0 ? __ballot(lab >= 0) : 0ull;
    for (int n = 0; n < 64 && todo; ++n) {                           // wave-uniform
      const int l = __shfl(lab, __ffsll((long long)todo) - 1, 64);
      const u64 hit = __ballot(has_obj && obj == l);
      if (lab == l) k_obj = hit ? __ffsll((long long)hit) - 1 : -1;
      todo &= ~__ballot(lab == l);
    }
    if (k_obj >= 0) {
      atomicAdd(&obj_s[k_obj][0], 1);
      if (hits[i] > 0) {
        atomicAdd(&obj_s[k_obj][1], 1);
        atomicMax(&obj_s[k_obj][2], h_max[i]);
        atomicMin(&obj_s[k_obj][3], h_min[i]);
      }
    }
  }
  __syncthreads();
  if (tid < K && bb_s[tid][2] >= 0) {                                 // a slot this workgroup met
    atomicMin(&o.bbox[4 * tid + 0], bb_s[tid][0]);
    atomicMin(&o.bbox[4 * tid + 1], bb_s[tid][1]);
    atomicMax(&o.bbox[4 * tid + 2], bb_s[tid][2]);
    atomicMax(&o.bbox[4 * tid + 3], bb_s[tid][3]);
    atomicAdd(&o.sum_rc[2 * tid], acc_s[tid][0]);
    atomicAdd(&o.sum_rc[2 * tid + 1], acc_s[tid][1]);
    atomicMax(&o.top_mm[tid], top_s[tid]);
  }
  if (tid < K_obj && obj_s[tid][0] > 0) {
    atomicAdd(&o.obj_cells[tid], obj_s[tid][0]);
    if (obj_s[tid][1] > 0) {
      atomicAdd(&o.obj_seen[tid], obj_s[tid][1]);
      atomicMax(&o.obj_top[tid], obj_s[tid][2]);
      atomicMin(&o.obj_base[tid], obj_s[tid][3]);
    }
  }
  if (tid < 6 && cnt_s[tid] > 0) atomicAdd(&counts[tid], cnt_s[tid]);
  if (blockIdx.x == 0 && tid == 0 && raw[0] != 0) status[0] = 2;      // the raw status is final since the flatten launch
}

inline bool obstacles_dims_ok(int N, int cols) {
  return N >= 1 && N <= EOD_OBSTACLES_N_MAX && cols >= 1 && N % cols == 0 && cols <= EOD_OBSTACLES_DIM_MAX &&
         N / cols <= EOD_OBSTACLES_DIM_MAX;
}

inline bool obstacles_aligned(const void* p, unsigned a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1u)) == 0; }

}  // namespace

extern "C" int eod_map_heights(const int32_t* proj_indices, const float* height, int height_stride, int P, int N, int band_lo_mm,
                               int band_hi_mm, int exclude_cell, int32_t* hits, int32_t* band_hits, int32_t* h_min_mm,
                               int32_t* h_max_mm, eod_stream_t stream) {
  if (P < 0 || P > EOD_OBSTACLES_PIXELS_MAX || N < 1 || N > EOD_OBSTACLES_N_MAX || height_stride < 1 || band_lo_mm > band_hi_mm ||
      band_lo_mm < -EOD_OBSTACLES_BAND_MAX || band_hi_mm > EOD_OBSTACLES_BAND_MAX)
    return EOD_ERR_BAD_DIMS;
  if ((P > 0 && (!proj_indices || !height)) || !hits || !band_hits || !h_min_mm || !h_max_mm) return EOD_ERR_NULL;
  if (!obstacles_aligned(proj_indices, 4) || !obstacles_aligned(height, 4) || !obstacles_aligned(hits, 4) ||
      !obstacles_aligned(band_hits, 4) || !obstacles_aligned(h_min_mm, 4) || !obstacles_aligned(h_max_mm, 4))
    return EOD_ERR_ALIGN;
  if (P == 0) return EOD_OK;
  hipLaunchKernelGGL(heights_kernel, dim3((P + HT_PIXELS - 1) / HT_PIXELS), dim3(HT_THREADS), 0, (hipStream_t)stream, (const int*)proj_indices, height,
                     height_stride, P, N, band_lo_mm, band_hi_mm, exclude_cell, (int*)hits, (int*)band_hits, (int*)h_min_mm,
                     (int*)h_max_mm);
  return eod_launch_status();
}

// the workspace: parent [N], slot [N], area [N] int32 | raw status
extern "C" size_t eod_map_obstacles_workspace_bytes(int N, int cols) {
  if (!obstacles_dims_ok(N, cols)) return 0;
  return up256((size_t)3 * N * 4) + 256;
}

extern "C" int eod_map_obstacles(const int32_t* hits, const int32_t* band_hits, const int32_t* h_min_mm, const int32_t* h_max_mm,
                                 const int32_t* object_labels, const int32_t* objects, int N, int cols, int K_obj, int min_hits,
                                 int min_cells, int topk, uint8_t* kind, int32_t* structure_labels, int32_t* merged_labels,
                                 int32_t* count, int32_t* structure, int32_t* area, int32_t* bbox, uint64_t* sum_rc, int32_t* top_mm,
                                 int32_t* obj_cells, int32_t* obj_seen_cells, int32_t* obj_top_mm, int32_t* obj_base_mm,
                                 int32_t* counts, int32_t* status, void* workspace, size_t workspace_bytes, eod_stream_t stream) {
  if (!obstacles_dims_ok(N, cols) || K_obj < 0 || K_obj > EOD_OBSTACLES_K_MAX || min_hits < 1 || min_cells < 1 || topk < 1 ||
      topk > EOD_OBSTACLES_TOPK_MAX)
    return EOD_ERR_BAD_DIMS;
  if (!hits || !band_hits || !h_min_mm || !h_max_mm || !kind || !structure_labels || !merged_labels || !count || !structure || !area ||
      !bbox || !sum_rc || !top_mm || !counts || !status || !workspace ||
      (K_obj > 0 && (!objects || !obj_cells || !obj_seen_cells || !obj_top_mm || !obj_base_mm)))
    return EOD_ERR_NULL;
  if (!obstacles_aligned(hits, 4) || !obstacles_aligned(band_hits, 4) || !obstacles_aligned(h_min_mm, 4) ||
      !obstacles_aligned(h_max_mm, 4) || !obstacles_aligned(object_labels, 4) || !obstacles_aligned(objects, 4) ||
      !obstacles_aligned(structure_labels, 4) || !obstacles_aligned(merged_labels, 4) || !obstacles_aligned(count, 4) ||
      !obstacles_aligned(structure, 4) || !obstacles_aligned(area, 4) || !obstacles_aligned(bbox, 4) || !obstacles_aligned(sum_rc, 8) ||
      !obstacles_aligned(top_mm, 4) || !obstacles_aligned(obj_cells, 4) || !obstacles_aligned(obj_seen_cells, 4) ||
      !obstacles_aligned(obj_top_mm, 4) || !obstacles_aligned(obj_base_mm, 4) || !obstacles_aligned(counts, 4) ||
      !obstacles_aligned(status, 4) || !obstacles_aligned(workspace, 8))
    return EOD_ERR_ALIGN;
  if (workspace_bytes < eod_map_obstacles_workspace_bytes(N, cols)) return EOD_ERR_CAPACITY;
  hipStream_t s = (hipStream_t)stream;
  char* ws = static_cast<char*>(workspace);
  int* parent = reinterpret_cast<int*>(ws);
  int* slot = parent + (size_t)N;
  int* area_ws = slot + (size_t)N;
  int* raw = reinterpret_cast<int*>(ws + up256((size_t)3 * N * 4));
  ObstaclesOut o;
  o.structure = (int*)structure; o.area = (int*)area; o.bbox = (int*)bbox; o.sum_rc = reinterpret_cast<u64*>(sum_rc);
  o.top_mm = (int*)top_mm; o.obj_cells = (int*)obj_cells; o.obj_seen = (int*)obj_seen_cells; o.obj_top = (int*)obj_top_mm;
  o.obj_base = (int*)obj_base_mm;
  const int rows = N / cols;
  const int tiles_r = (rows + RG_TR - 1) / RG_TR, tiles_c = (cols + RG_TC - 1) / RG_TC;      // N <= 2^22: fewer than 2^18 tiles
  const int per_cell = (N + RG_THREADS - 1) / RG_THREADS, chunks = (N + RG_FLAT_CELLS - 1) / RG_FLAT_CELLS;
  hipLaunchKernelGGL(obstacles_classify_kernel, dim3((N + 255) / 256), dim3(256), 0, s, (const int*)hits, (const int*)band_hits,
                     (const int*)object_labels, N, K_obj, min_hits, (unsigned char*)kind, (int*)count, (int*)counts, (int*)status, raw,
                     o.obj_cells, o.obj_seen, o.obj_top, o.obj_base);
  hipLaunchKernelGGL(obstacles_tile_kernel, dim3(tiles_r * tiles_c), dim3(RG_THREADS), 0, s, (const unsigned char*)kind, rows, cols,
                     tiles_c, parent, slot, area_ws, raw);
  hipLaunchKernelGGL(obstacles_border_kernel, dim3(per_cell), dim3(RG_THREADS), 0, s, parent, N, cols, raw);
  hipLaunchKernelGGL(regions_compress_kernel, dim3(per_cell), dim3(RG_THREADS), 0, s, parent, (const int*)slot, N, raw);
  hipLaunchKernelGGL(regions_flatten_kernel, dim3(chunks), dim3(RG_FLAT_THREADS), 0, s, (const int*)parent, N, (int*)structure_labels,
                     area_ws, (int*)counts + 2, raw);
  hipLaunchKernelGGL(regions_list_kernel, dim3(chunks), dim3(RG_FLAT_THREADS), 0, s, (const int*)structure_labels, (const int*)area_ws,
                     parent, N, min_cells, (int*)count);
  hipLaunchKernelGGL(obstacles_select_kernel, dim3(1), dim3(RG_SEL_THREADS), 0, s, (const int*)area_ws, slot, (const int*)parent,
                     (const int*)count, N, topk, o);
  hipLaunchKernelGGL(obstacles_stats_kernel, dim3((N + RG_STAT_CELLS - 1) / RG_STAT_CELLS), dim3(RG_THREADS), 0, s,
                     (const unsigned char*)kind, (const int*)object_labels, (const int*)objects, (const int*)hits, (const int*)h_min_mm,
                     (const int*)h_max_mm, (const int*)structure_labels, (const int*)area_ws, (const int*)slot, N, cols, topk, K_obj,
                     min_cells, (int*)merged_labels, o, (int*)counts, (const int*)raw, (int*)status);
  return eod_launch_status();
}
