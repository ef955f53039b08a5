// Frontiers on the map (eod_map_cover, eod_map_frontier; semantics in include/eod_frontier.h): the record of the cells a frame
// covered, and from it the known free cells next to unknown ones, joined into frontiers, with the unknown region behind each and
// the cell of each that is cheapest to reach.  A read-only query beside the frame: integers and comparisons only, integer atomics
// only, the result a pure function of the inputs.  Eleven launches of eod_map_frontier and one of eod_map_cover; what one needs
// of another is complete at the launch boundary between them, and no workgroup ever waits for another one (no spin, no flag, no grid barrier).  The connected components are the
// union-find of regions.hip on two planes: plane 0 the frontier cells, 8-connected, plane 1 the UNKNOWN cells, 4-connected.  A
// plane takes the place of a class q of regions.hip in the workspace's parent and slot, so the launches of regions_common.h that see
// only those run on both planes at once (blockIdx.y); flatten runs once per plane, because the labels and the areas of the two
// planes are separate arguments of the entry point.
//
//   frontier_classify_kernel  one thread per cell: the cell's kind, one byte to the workspace.  Lane l holds passable[l], the wave
//                             compares a cell's label with all of them at once (sight_init_kernel's ballot).  count, counts, status and
//                             the raw status to 0.
//   frontier_tile_kernel      regions_tile_kernel per 32 x 32 tile and plane.  The kinds of the tile and of a halo of one cell round
//                             it come to LDS first (34 x 34 bytes; outside the grid: BLOCKED, which is neither UNKNOWN nor OPEN, so the
//                             grid's edges need no other test); plane 0 tells a frontier cell from them, plane 1 an UNKNOWN cell.
//                             Plane 0 also counts the BLOCKED and the OPEN cells of its tile and clears its cells' behind keys.
//   frontier_border_kernel    regions_border_kernel per plane: left, up and, on plane 0, the two upper diagonals (at a tile corner the
//                             only link).  A neighbour is foreground where its parent is >= 0.
//   regions_compress_kernel   (regions_common.h) both planes
//   regions_flatten_kernel    (regions_common.h) plane 0: frontier_labels, the frontiers' areas, counts[3]; plane 1: unknown_labels,
//                             unknown_area, counts[2]
//   frontier_behind_kernel    both planes' labels and areas are final.  Every frontier cell brings the key of each UNKNOWN 4-neighbour's
//                             region to its frontier's label cell with a 64-bit atomicMax (skipped where the key there is as large
//                             already: a maximum only grows, so a stale read skips nothing that would have counted).  The unknown
//                             regions' label cells are counted: counts[4].
//   regions_list_kernel       (regions_common.h) the frontiers with area >= min_cells: count[0] and the list, in plane 0's parent
//   frontier_select_kernel    one workgroup: K rounds of a workgroup-wide maximum of the rank key over the list, below the previous pick,
//                             each leaving slot[root] = k and the slot's outputs at their neutral values
//   frontier_stats_kernel     every frontier cell whose frontier has a slot: bbox, sum_rc, open_edges, reach_key, per workgroup in LDS
//                             first, then one global atomic per slot the workgroup touched
//   frontier_finish_kernel    the halves of reach_key; status[0]
//
// THE INVARIANT of regions.hip carries over word for word: every value ever stored in parent[x] is a member of x's component and is
// <= x.  Whether two cells are adjacent depends on the kinds alone, which do not change after the first launch.  The bounds of the
// loops are those of regions.hip (RG_TILE hops in LDS, RG_FIND_CAP and RG_HOOK_CAP globally); a thread that reaches one stops and
// sets the raw status, which the last launch turns into status[0] bit 1.
// BOUNDS: every per-cell array is indexed by i < N or by a 4- or 8-neighbour of i that the row and column tests keep inside the
// grid; a label is a cell; a slot is < K; the halo is indexed by (lr + 1 + dr) * 34 + lc + 1 + dc with 0 <= lr, lc < 32 and
// |dr|, |dc| <= 1; proj_indices' cells are tested against [0, N) before they index last_seen.
#include "regions_common.h"
#include "../../include/eod_frontier.h"

namespace {

static_assert(EOD_FRONTIER_N_MAX == EOD_REGIONS_N_MAX && EOD_FRONTIER_TOPK_MAX == EOD_REGIONS_TOPK_MAX, "the shared launches' limits");
static_assert(EOD_FRONTIER_P_MAX == 64, "one wave looks a label up");
static_assert(2ll * (EOD_FRONTIER_DIM_MAX - 1) * (EOD_FRONTIER_DIM_MAX - 1) < (long long)INT_MAX, "a squared distance is never INT_MAX");

constexpr unsigned char FR_BLOCKED = 0, FR_OPEN = 1, FR_UNKNOWN = 2;
constexpr int FR_HALO_C = RG_TC + 2, FR_HALO = (RG_TR + 2) * FR_HALO_C;
constexpr u64 FR_NONE = ~0ull;

__global__ __launch_bounds__(256) void frontier_cover_kernel(const int* __restrict__ proj, int P, int N, int stamp, int exclude_cell,
                                                             int* __restrict__ last_seen) {
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= P) return;
  const int c = proj[p];
  if (c < 0 || c >= N || c == exclude_cell) return;
  if (agent_ld(&last_seen[c]) < stamp) atomicMax(&last_seen[c], stamp);         // it only grows: a stale read costs an atomic at most
}

__global__ __launch_bounds__(256) void frontier_classify_kernel(const int* __restrict__ labels, const int* __restrict__ passable,
                                                                const int* __restrict__ last_seen, int N, int P, int since,
                                                                unsigned char* __restrict__ kind, int* __restrict__ count,
                                                                int* __restrict__ counts, int* __restrict__ status, int* __restrict__ raw) {
  const int i = blockIdx.x * 256 + threadIdx.x, lane = threadIdx.x & 63;
  const bool has_pas = lane < P;
  const int pas = has_pas ? passable[lane] : 0;
  const int lab = i < N ? labels[i] : -1;
  bool pass = false;
  u64 todo = __ballot(lab >= 0);
  for (int n = 0; n < 64 && todo; ++n) {                             // wave-uniform
    const int j = __ffsll((long long)todo) - 1;
    todo &= todo - 1;
    const int l = __shfl(lab, j, 64);
    const u64 hit = __ballot(has_pas && pas == l);
    if (lane == j) pass = hit != 0;
  }
  if (i < N) kind[i] = lab >= 0 && !pass ? FR_BLOCKED : last_seen[i] >= since ? FR_OPEN : FR_UNKNOWN;
  if (i < 5) counts[i] = 0;
  if (i < 2) status[i] = 0;
  if (i == 0) {
    count[0] = 0;
    raw[0] = 0;
  }
}

__global__ __launch_bounds__(RG_THREADS) void frontier_tile_kernel(const unsigned char* __restrict__ kind, int N, int rows, int cols,
                                                                    int tiles_c, int* __restrict__ parent, int* __restrict__ slot,
                                                                    int* __restrict__ area0, int* __restrict__ area1,
                                                                    u64* __restrict__ behind, int* __restrict__ counts,
                                                                    int* __restrict__ status) {
  __shared__ int p_s[RG_TILE];
  __shared__ unsigned char k_s[FR_HALO];
  __shared__ int cnt_s[2];
  const int tid = threadIdx.x, plane = blockIdx.y;
  const int ty = blockIdx.x / tiles_c, tx = blockIdx.x - ty * tiles_c;
  const int r0 = ty * RG_TR, c0 = tx * RG_TC;
  const size_t qoff = (size_t)plane * N;
  if (tid < 2) cnt_s[tid] = 0;
  for (int h = tid; h < FR_HALO; h += RG_THREADS) {
    const int hr = h / FR_HALO_C, hc = h - hr * FR_HALO_C;
    const int r = r0 - 1 + hr, c = c0 - 1 + hc;
    k_s[h] = r >= 0 && r < rows && c >= 0 && c < cols ? kind[r * cols + c] : FR_BLOCKED;
  }
  __syncthreads();
  for (int l = tid; l < RG_TILE; l += RG_THREADS) {                  // uniform: RG_TILE is a multiple of RG_THREADS
    const int lr = l / RG_TC, lc = l & (RG_TC - 1);
    const int h = (lr + 1) * FR_HALO_C + lc + 1;
    const bool in = r0 + lr < rows && c0 + lc < cols;
    const unsigned char k = k_s[h];                                  // BLOCKED outside the grid
    bool fg;
    if (plane == 0)
      fg = k == FR_OPEN && (k_s[h - FR_HALO_C] == FR_UNKNOWN || k_s[h + FR_HALO_C] == FR_UNKNOWN || k_s[h - 1] == FR_UNKNOWN ||
                            k_s[h + 1] == FR_UNKNOWN);
    else
      fg = k == FR_UNKNOWN;
    p_s[l] = fg ? l : -1;
    if (plane == 0) {
      const u64 b = __ballot(in && k == FR_BLOCKED), o = __ballot(k == FR_OPEN);
      if ((tid & 63) == 0) {
        if (b) atomicAdd(&cnt_s[0], __popcll(b));
        if (o) atomicAdd(&cnt_s[1], __popcll(o));
      }
    }
  }
  __syncthreads();
  const bool conn8 = plane == 0;
  for (int l = tid; l < RG_TILE; l += RG_THREADS) {
    if (lds_ld(&p_s[l]) < 0) continue;
    const int lr = l / RG_TC, lc = l & (RG_TC - 1);
    if (lc > 0 && lds_ld(&p_s[l - 1]) >= 0) tile_union(p_s, l, l - 1, status);
    if (lr > 0) {
      if (lds_ld(&p_s[l - RG_TC]) >= 0) tile_union(p_s, l, l - RG_TC, status);
      if (conn8) {
        if (lc > 0 && lds_ld(&p_s[l - RG_TC - 1]) >= 0) tile_union(p_s, l, l - RG_TC - 1, status);
        if (lc < RG_TC - 1 && lds_ld(&p_s[l - RG_TC + 1]) >= 0) tile_union(p_s, l, l - RG_TC + 1, status);
      }
    }
  }
  __syncthreads();
  int* area = plane == 0 ? area0 : area1;
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
    parent[qoff + g] = v;
    slot[qoff + g] = local_root ? -2 : -1;
    area[g] = 0;
    if (plane == 0) behind[g] = 0ull;
  }
  if (plane == 0 && tid < 2 && cnt_s[tid] > 0) atomicAdd(&counts[tid], cnt_s[tid]);
}

__global__ __launch_bounds__(RG_THREADS) void frontier_border_kernel(int* __restrict__ parent, int N, int cols, int* __restrict__ status) {
  const int i = blockIdx.x * RG_THREADS + threadIdx.x;
  if (i >= N) return;
  const int r = i / cols, c = i - r * cols;
  const int lr = r & (RG_TR - 1), lc = c & (RG_TC - 1);
  if (lr != 0 && lc != 0 && lc != RG_TC - 1) return;                 // all four neighbours before it are in its own tile
  int* p = parent + (size_t)blockIdx.y * N;
  if (agent_ld(&p[i]) < 0) return;
  const bool conn8 = blockIdx.y == 0;
  // the row and the column are the grid's: c > 0 and c < cols - 1 keep (r, 0) away from (r - 1, cols - 1) and from (r, cols - 1)
  if (lc == 0 && c > 0 && agent_ld(&p[i - 1]) >= 0) grid_union(p, i, i - 1, status);
  if (r > 0) {
    if (lr == 0 && agent_ld(&p[i - cols]) >= 0) grid_union(p, i, i - cols, status);
    if (conn8) {
      if (c > 0 && (lr == 0 || lc == 0) && agent_ld(&p[i - cols - 1]) >= 0) grid_union(p, i, i - cols - 1, status);
      if (c < cols - 1 && (lr == 0 || lc == RG_TC - 1) && agent_ld(&p[i - cols + 1]) >= 0) grid_union(p, i, i - cols + 1, status);
    }
  }
}

// The UNKNOWN 4-neighbours of cell i = (r, c) by their labels: f(j) for each.
template <typename F>
__device__ __forceinline__ void frontier_unknown_neighbours(const int* __restrict__ unknown_labels, int i, int r, int c, int rows, int cols,
                                                            F f) {
  if (r > 0 && unknown_labels[i - cols] >= 0) f(unknown_labels[i - cols]);
  if (c > 0 && unknown_labels[i - 1] >= 0) f(unknown_labels[i - 1]);
  if (c < cols - 1 && unknown_labels[i + 1] >= 0) f(unknown_labels[i + 1]);
  if (r < rows - 1 && unknown_labels[i + cols] >= 0) f(unknown_labels[i + cols]);
}

__global__ __launch_bounds__(RG_THREADS) void frontier_behind_kernel(const int* __restrict__ frontier_labels,
                                                                      const int* __restrict__ unknown_labels,
                                                                      const int* __restrict__ unknown_area, int N, int rows, int cols,
                                                                      u64* __restrict__ behind, int* __restrict__ counts) {
  __shared__ int roots_s;
  const int i = blockIdx.x * RG_THREADS + threadIdx.x;
  if (threadIdx.x == 0) roots_s = 0;
  __syncthreads();
  const int lab = i < N ? frontier_labels[i] : -1;
  if (lab >= 0) {
    const int r = i / cols, c = i - r * cols;
    u64 best = 0ull;
    frontier_unknown_neighbours(unknown_labels, i, r, c, rows, cols, [&](int ul) {
      const u64 key = ((u64)(unsigned)unknown_area[ul] << 32) | (unsigned)~ul;
      if (key > best) best = key;
    });
    u64* at = &behind[lab];
    if (best > __hip_atomic_load(at, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(at, best);
  }
  const u64 roots = __ballot(i < N && unknown_labels[i] == i);
  if ((threadIdx.x & 63) == 0 && roots) atomicAdd(&roots_s, __popcll(roots));
  __syncthreads();
  if (threadIdx.x == 0 && roots_s > 0) atomicAdd(&counts[4], roots_s);
}

struct FrontierOut {     // the per-slot arrays of the entry point
  int *frontier, *area, *bbox;
  u64* sum_rc;
  int* open_edges;
  u64* behind_key;
  int *behind_area, *behind_label;
  u64* reach_key;
  int *reach_cost, *reach_cell;
};

__global__ __launch_bounds__(RG_SEL_THREADS) void frontier_select_kernel(const int* __restrict__ area, const u64* __restrict__ behind,
                                                                          int* __restrict__ slot, const int* __restrict__ list,
                                                                          const int* __restrict__ count, int N, int K, int rank_by,
                                                                          const FrontierOut o) {
  __shared__ u64 red_s[RG_SEL_THREADS / 64];
  const int tid = threadIdx.x;
  const int n = count[0] < N ? count[0] : N;
  u64 prev = ~0ull;                                                   // above every key
  for (int k = 0; k < K; ++k) {
    u64 best = 0ull;                                                  // below every key: an area, listed or behind, is at least 1
    if (prev) {                                                       // block-uniform
      for (int j = tid; j < n; j += RG_SEL_THREADS) {
        const int root = list[j];
        const unsigned a = rank_by ? (unsigned)(behind[root] >> 32) : (unsigned)area[root];
        const u64 key = ((u64)a << 32) | (unsigned)~root;
        if (key < prev && key > best) best = key;
      }
    }
    prev = block_max_u64(best, red_s);                                // 0 once the frontiers are used up: the rest is padding
    if (tid == 0) {
      const int root = (int)~(unsigned)prev;
      const u64 bk = prev ? behind[root] : 0ull;
      o.frontier[k] = prev ? root : -1;
      o.area[k] = prev ? area[root] : 0;
      o.bbox[4 * k + 0] = prev ? INT_MAX : 0;
      o.bbox[4 * k + 1] = prev ? INT_MAX : 0;
      o.bbox[4 * k + 2] = prev ? -1 : 0;
      o.bbox[4 * k + 3] = prev ? -1 : 0;
      o.sum_rc[2 * k] = 0ull;
      o.sum_rc[2 * k + 1] = 0ull;
      o.open_edges[k] = 0;
      o.behind_key[k] = bk;
      o.behind_area[k] = (int)(unsigned)(bk >> 32);
      o.behind_label[k] = prev ? (int)~(unsigned)bk : -1;
      o.reach_key[k] = FR_NONE;
      if (prev) slot[root] = k;
    }
  }
}

__global__ __launch_bounds__(RG_THREADS) void frontier_stats_kernel(const int* __restrict__ frontier_labels,
                                                                     const int* __restrict__ unknown_labels, const int* __restrict__ slot,
                                                                     const int* __restrict__ dist, int N, int rows, int cols, int K,
                                                                     int from_cell, const FrontierOut o) {
  __shared__ int bb_s[EOD_FRONTIER_TOPK_MAX][4], edges_s[EOD_FRONTIER_TOPK_MAX];
  __shared__ u64 acc_s[EOD_FRONTIER_TOPK_MAX][3];                     // sum of rows, sum of columns, reach key
  const int tid = threadIdx.x;
  if (tid < K) {
    bb_s[tid][0] = INT_MAX; bb_s[tid][1] = INT_MAX; bb_s[tid][2] = -1; bb_s[tid][3] = -1;
    edges_s[tid] = 0;
    acc_s[tid][0] = 0ull; acc_s[tid][1] = 0ull; acc_s[tid][2] = FR_NONE;
  }
  __syncthreads();
  const int fr = from_cell >= 0 ? from_cell / cols : 0, fc = from_cell >= 0 ? from_cell - fr * cols : 0;
  const int base = blockIdx.x * RG_STAT_CELLS;
  for (int j = tid; j < RG_STAT_CELLS; j += RG_THREADS) {
    const int i = base + j;
    if (i >= N) break;
    const int lab = frontier_labels[i];
    if (lab < 0) continue;
    const int k = slot[lab];
    if (k < 0) continue;
    const int r = i / cols, c = i - r * cols;
    int edges = 0;
    frontier_unknown_neighbours(unknown_labels, i, r, c, rows, cols, [&](int) { ++edges; });
    const int v = dist ? dist[i] : from_cell >= 0 ? (r - fr) * (r - fr) + (c - fc) * (c - fc) : 0;
    atomicMin(&bb_s[k][0], r);
    atomicMin(&bb_s[k][1], c);
    atomicMax(&bb_s[k][2], r);
    atomicMax(&bb_s[k][3], c);
    atomicAdd(&edges_s[k], edges);
    atomicAdd(&acc_s[k][0], (u64)r);
    atomicAdd(&acc_s[k][1], (u64)c);
    if (v >= 0 && v < INT_MAX) atomicMin(&acc_s[k][2], ((u64)(unsigned)v << 32) | (unsigned)i);
  }
  __syncthreads();
  if (tid < K && bb_s[tid][2] >= 0) {                                  // a slot this workgroup met
    atomicMin(&o.bbox[4 * tid + 0], bb_s[tid][0]);
    atomicMin(&o.bbox[4 * tid + 1], bb_s[tid][1]);
    atomicMax(&o.bbox[4 * tid + 2], bb_s[tid][2]);
    atomicMax(&o.bbox[4 * tid + 3], bb_s[tid][3]);
    atomicAdd(&o.open_edges[tid], edges_s[tid]);
    atomicAdd(&o.sum_rc[2 * tid], acc_s[tid][0]);
    atomicAdd(&o.sum_rc[2 * tid + 1], acc_s[tid][1]);
    if (acc_s[tid][2] != FR_NONE) atomicMin(&o.reach_key[tid], acc_s[tid][2]);
  }
}

__global__ __launch_bounds__(64) void frontier_finish_kernel(int K, const FrontierOut o, const int* __restrict__ raw, int* __restrict__ status) {
  const int k = threadIdx.x;
  if (k < K) {
    const u64 key = o.reach_key[k];
    o.reach_cost[k] = key == FR_NONE ? INT_MAX : (int)(unsigned)(key >> 32);
    o.reach_cell[k] = key == FR_NONE ? -1 : (int)(unsigned)key;
  }
  if (k == 0 && raw[0] != 0) status[0] = 2;
}

inline bool frontier_dims_ok(int N, int cols) {
  return N >= 1 && N <= EOD_FRONTIER_N_MAX && cols >= 1 && N % cols == 0 && cols <= EOD_FRONTIER_DIM_MAX &&
         N / cols <= EOD_FRONTIER_DIM_MAX;
}

inline bool frontier_aligned(const void* p, unsigned a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1u)) == 0; }

}  // namespace

extern "C" int eod_map_cover(const int32_t* proj_indices, int P, int N, int stamp, int exclude_cell, int32_t* last_seen,
                             eod_stream_t stream) {
  if (P < 0 || P > EOD_FRONTIER_PIXELS_MAX || N < 1 || N > EOD_FRONTIER_N_MAX || stamp < 0) return EOD_ERR_BAD_DIMS;
  if ((P > 0 && !proj_indices) || !last_seen) return EOD_ERR_NULL;
  if (!frontier_aligned(proj_indices, 4) || !frontier_aligned(last_seen, 4)) return EOD_ERR_ALIGN;
  if (P == 0) return EOD_OK;
  hipLaunchKernelGGL(frontier_cover_kernel, dim3((P + 255) / 256), dim3(256), 0, (hipStream_t)stream, (const int*)proj_indices, P, N,
                     stamp, exclude_cell, (int*)last_seen);
  return eod_launch_status();
}

// the workspace: parent [2, N], slot [2, N], area0 [N] int32 | raw status | behind uint64 [N] | kind [N] bytes
extern "C" size_t eod_map_frontier_workspace_bytes(int N, int cols) {
  if (!frontier_dims_ok(N, cols)) return 0;
  return up256((size_t)5 * N * 4) + 256 + up256((size_t)N * 8) + up256((size_t)N);
}

extern "C" int eod_map_frontier(const int32_t* object_labels, const int32_t* passable, const int32_t* last_seen, const int32_t* dist,
                                int N, int P, int cols, int since, int from_cell, int min_cells, int topk, int rank_by,
                                int32_t* frontier_labels, int32_t* unknown_labels, int32_t* unknown_area, int32_t* count,
                                int32_t* frontier, int32_t* area, int32_t* bbox, uint64_t* sum_rc, int32_t* open_edges,
                                uint64_t* behind_key, int32_t* behind_area, int32_t* behind_label, uint64_t* reach_key,
                                int32_t* reach_cost, int32_t* reach_cell, int32_t* counts, int32_t* status, void* workspace,
                                size_t workspace_bytes, eod_stream_t stream) {
  if (!frontier_dims_ok(N, cols) || P < 0 || P > EOD_FRONTIER_P_MAX || from_cell < -1 || from_cell >= N || min_cells < 1 || topk < 1 ||
      topk > EOD_FRONTIER_TOPK_MAX || (rank_by != 0 && rank_by != 1))
    return EOD_ERR_BAD_DIMS;
  if (!object_labels || (P > 0 && !passable) || !last_seen || !frontier_labels || !unknown_labels || !unknown_area || !count ||
      !frontier || !area || !bbox || !sum_rc || !open_edges || !behind_key || !behind_area || !behind_label || !reach_key ||
      !reach_cost || !reach_cell || !counts || !status || !workspace)
    return EOD_ERR_NULL;
  if (!frontier_aligned(object_labels, 4) || !frontier_aligned(passable, 4) || !frontier_aligned(last_seen, 4) ||
      !frontier_aligned(dist, 4) || !frontier_aligned(frontier_labels, 4) || !frontier_aligned(unknown_labels, 4) ||
      !frontier_aligned(unknown_area, 4) || !frontier_aligned(count, 4) || !frontier_aligned(frontier, 4) || !frontier_aligned(area, 4) ||
      !frontier_aligned(bbox, 4) || !frontier_aligned(sum_rc, 8) || !frontier_aligned(open_edges, 4) || !frontier_aligned(behind_key, 8) ||
      !frontier_aligned(behind_area, 4) || !frontier_aligned(behind_label, 4) || !frontier_aligned(reach_key, 8) ||
      !frontier_aligned(reach_cost, 4) || !frontier_aligned(reach_cell, 4) || !frontier_aligned(counts, 4) ||
      !frontier_aligned(status, 4) || !frontier_aligned(workspace, 8))
    return EOD_ERR_ALIGN;
  if (workspace_bytes < eod_map_frontier_workspace_bytes(N, cols)) return EOD_ERR_CAPACITY;
  hipStream_t s = (hipStream_t)stream;
  char* ws = static_cast<char*>(workspace);
  int* parent = reinterpret_cast<int*>(ws);
  int* slot = parent + (size_t)2 * N;
  int* area0 = slot + (size_t)2 * N;
  int* raw = reinterpret_cast<int*>(ws + up256((size_t)5 * N * 4));
  u64* behind = reinterpret_cast<u64*>(ws + up256((size_t)5 * N * 4) + 256);
  unsigned char* kind = reinterpret_cast<unsigned char*>(ws + up256((size_t)5 * N * 4) + 256 + up256((size_t)N * 8));
  FrontierOut o;
  o.frontier = (int*)frontier; o.area = (int*)area; o.bbox = (int*)bbox; o.sum_rc = reinterpret_cast<u64*>(sum_rc);
  o.open_edges = (int*)open_edges; o.behind_key = reinterpret_cast<u64*>(behind_key); o.behind_area = (int*)behind_area;
  o.behind_label = (int*)behind_label; o.reach_key = reinterpret_cast<u64*>(reach_key); o.reach_cost = (int*)reach_cost;
  o.reach_cell = (int*)reach_cell;
  const int rows = N / cols;
  const int tiles_r = (rows + RG_TR - 1) / RG_TR, tiles_c = (cols + RG_TC - 1) / RG_TC;      // N <= 2^22: fewer than 2^18 tiles
  const int per_cell = (N + RG_THREADS - 1) / RG_THREADS, chunks = (N + RG_FLAT_CELLS - 1) / RG_FLAT_CELLS;
  hipLaunchKernelGGL(frontier_classify_kernel, dim3((N + 255) / 256), dim3(256), 0, s, (const int*)object_labels, (const int*)passable,
                     (const int*)last_seen, N, P, since, kind, (int*)count, (int*)counts, (int*)status, raw);
  hipLaunchKernelGGL(frontier_tile_kernel, dim3(tiles_r * tiles_c, 2), dim3(RG_THREADS), 0, s, (const unsigned char*)kind, N, rows, cols,
                     tiles_c, parent, slot, area0, (int*)unknown_area, behind, (int*)counts, raw);
  hipLaunchKernelGGL(frontier_border_kernel, dim3(per_cell, 2), dim3(RG_THREADS), 0, s, parent, N, cols, raw);
  hipLaunchKernelGGL(regions_compress_kernel, dim3(per_cell, 2), dim3(RG_THREADS), 0, s, parent, (const int*)slot, N, raw);
  hipLaunchKernelGGL(regions_flatten_kernel, dim3(chunks), dim3(RG_FLAT_THREADS), 0, s, (const int*)parent, N, (int*)frontier_labels,
                     area0, (int*)counts + 3, raw);
  hipLaunchKernelGGL(regions_flatten_kernel, dim3(chunks), dim3(RG_FLAT_THREADS), 0, s, (const int*)(parent + N), N,
                     (int*)unknown_labels, (int*)unknown_area, (int*)counts + 2, raw);
  hipLaunchKernelGGL(frontier_behind_kernel, dim3(per_cell), dim3(RG_THREADS), 0, s, (const int*)frontier_labels,
                     (const int*)unknown_labels, (const int*)unknown_area, N, rows, cols, behind, (int*)counts);
  hipLaunchKernelGGL(regions_list_kernel, dim3(chunks), dim3(RG_FLAT_THREADS), 0, s, (const int*)frontier_labels, (const int*)area0,
                     parent, N, min_cells, (int*)count);
  hipLaunchKernelGGL(frontier_select_kernel, dim3(1), dim3(RG_SEL_THREADS), 0, s, (const int*)area0, (const u64*)behind, slot,
                     (const int*)parent, (const int*)count, N, topk, rank_by, o);
  hipLaunchKernelGGL(frontier_stats_kernel, dim3((N + RG_STAT_CELLS - 1) / RG_STAT_CELLS), dim3(RG_THREADS), 0, s,
                     (const int*)frontier_labels, (const int*)unknown_labels, (const int*)slot, (const int*)dist, N, rows, cols, topk,
                     from_cell, o);
  hipLaunchKernelGGL(frontier_finish_kernel, dim3(1), dim3(64), 0, s, topk, o, (const int*)raw, (int*)status);
  return eod_launch_status();
}
