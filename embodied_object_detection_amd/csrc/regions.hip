// Map regions: the connected areas of each queried class of a [Q, N] map, ranked by size (eod_map_regions; semantics in
// include/eod_regions.h).  A read-only query: integers and comparisons only, integer atomics only, the result a pure function of
// the inputs.  Eight launches; what one needs of another is complete at the launch boundary between them, and no workgroup ever
// waits for another one (no spin, no flag, no grid barrier).  The launches that see only parent, area, slot and the list are in
// regions_common.h, which eod_map_inventory (inventory.hip) shares.
//
//   regions_tile_kernel     one workgroup per 32 x 32 tile and class: union-find in LDS on tile-local row-major indices (the larger
//                           root is hooked under the smaller with an LDS atomicMin), then parent[q][i] = the global cell of the
//                           tile-local root (-1: background), area[q][i] = 0, slot[q][i] = -1 for the tile's own cells (-2 marks a
//                           tile-local root: the only cells whose parent a later launch changes).
//   regions_border_kernel   every foreground cell on a tile border unites itself with its foreground neighbours in the tiles before it
//                           (left, up and, under 8-connectivity, the two upper diagonals: at a tile corner these are the only link),
//                           on the global parent with atomicMin.
//   regions_compress_kernel every tile-local root follows parent to its root and stores it as its parent, so that the chains, which
//                           are as long as the merges made them, are walked once per tile-local root and not once per cell.
//   regions_flatten_kernel  every foreground cell follows parent to its root (its tile-local root, then the root): labels,
//                           area[root] += 1 (counted per workgroup in an LDS table first: one add per root and workgroup),
//                           foreground[q].
//   regions_list_kernel     the roots with area >= min_cells are counted (count[q]) and listed, into parent's storage, which nobody
//                           reads any more.  The order of the list is the scheduler's; nothing below depends on it.
//   regions_select_kernel   one workgroup per class: K rounds of a workgroup-wide maximum of (area << 32) | ~label over the list, below
//                           the previous pick, each leaving slot[root] = k and the slot's accumulators at their neutral values.
//   regions_stats_kernel    every cell whose root has a slot: bbox (min / max), sum_rc, the peak key (prob bits << 32) | ~cell (max)
//                           and mass_q24, per workgroup in LDS first, then one integer global atomic per slot the workgroup touched.
//   regions_finish_kernel   the peak keys become peak and peak_prob.
//
// Launch 2 is the only place where workgroups meet, and they meet only through atomicMin on parent and through loads that may be
// stale.  THE INVARIANT: every value ever stored in parent[x] is a member of x's component and is <= x (launch 1 stores the smallest
// cell of x's part of the tile; an atomicMin stores the root of a cell adjacent to x's tree, which is smaller).  So a stale read of
// parent[x] is still an ancestor-or-self that was valid once and is in the component for good; `find` strictly descends and ends
// at a cell that was a root when read; and a hook is decided by the atomic alone: atomicMin(&parent[a], b) returns the value it
// replaced, which is a if and only if a was still a root (the hook holds), and otherwise an older, smaller parent `old` of a.  Then
// parent[a] = min(old, b), both in the component, and the union goes on with (old, b), so no link is ever lost.  Loads of parent in
// launch 2 are relaxed agent-scope atomics: they see what the other seven L2s' atomics did, which keeps retries few; correctness
// does not need it.  Launch 3 keeps the invariant too: it stores a cell's root, read while other tile-local roots store theirs; a
// reader finds the old parent or the root, both ancestors, and the roots themselves no longer change.
//
// Bounds of the loops: `find` descends, so it makes fewer hops than its array has cells (RG_TILE in LDS, N <= 2^22 globally); a hook
// retry lowers the larger of its two cells, so it is bounded likewise.  The caps below are those numbers; a thread that reaches
// one stops and sets status.  A probe of the flatten kernel's LDS table ends after RG_FLAT_PROBES entries; what finds no entry is
// added to global memory directly, which is exact too, so that bound sets no status.
#include "regions_common.h"

namespace {

__global__ __launch_bounds__(RG_THREADS) void regions_tile_kernel(const float* __restrict__ prob, int N, int rows, int cols, int tiles_c,
                                                                   float level, int conn8, int* __restrict__ parent,
                                                                   int* __restrict__ area, int* __restrict__ slot,
                                                                   int* __restrict__ status) {
  __shared__ int p_s[RG_TILE];
  const int tid = threadIdx.x;
  const int ty = blockIdx.x / tiles_c, tx = blockIdx.x - ty * tiles_c;
  const int r0 = ty * RG_TR, c0 = tx * RG_TC;
  const size_t qoff = (size_t)blockIdx.y * N;
  for (int l = tid; l < RG_TILE; l += RG_THREADS) {
    const int r = r0 + l / RG_TC, c = c0 + (l & (RG_TC - 1));
    int v = -1;
    if (r < rows && c < cols && prob[qoff + r * cols + c] >= level) v = l;       // a NaN compares false
    p_s[l] = v;
  }
  __syncthreads();
  // a cell unites itself with the foreground neighbours before it in row-major order; p_s[x] >= 0 says foreground at any time
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
    const size_t g = qoff + r * cols + c;
    parent[g] = v;
    area[g] = 0;
    slot[g] = local_root ? -2 : -1;
  }
}

__global__ __launch_bounds__(RG_THREADS) void regions_border_kernel(int* __restrict__ parent, int N, int cols, int conn8,
                                                                     int* __restrict__ status) {
  const int i = blockIdx.x * RG_THREADS + threadIdx.x;
  if (i >= N) return;
  const int r = i / cols, c = i - r * cols;
  const int lr = r & (RG_TR - 1), lc = c & (RG_TC - 1);
  if (lr != 0 && lc != 0 && lc != RG_TC - 1) return;                 // all four neighbours before it are in its own tile
  int* p = parent + (size_t)blockIdx.y * N;
  if (agent_ld(&p[i]) < 0) return;
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

__global__ __launch_bounds__(RG_THREADS) void regions_stats_kernel(const float* __restrict__ prob, const int* __restrict__ labels,
                                                                    const int* __restrict__ slot, int N, int cols, int Q, int K,
                                                                    int* __restrict__ out, u64* __restrict__ peak_key) {
  __shared__ int bb_s[EOD_REGIONS_TOPK_MAX][4];
  __shared__ u64 acc_s[EOD_REGIONS_TOPK_MAX][4];                      // sum of rows, sum of columns, mass, peak key
  const int tid = threadIdx.x, q = blockIdx.y;
  const size_t qoff = (size_t)q * N;
  if (tid < K) {
    bb_s[tid][0] = INT_MAX; bb_s[tid][1] = INT_MAX; bb_s[tid][2] = -1; bb_s[tid][3] = -1;
    acc_s[tid][0] = 0ull; acc_s[tid][1] = 0ull; acc_s[tid][2] = 0ull; acc_s[tid][3] = 0ull;
  }
  __syncthreads();
  const int base = blockIdx.x * RG_STAT_CELLS;
  for (int j = tid; j < RG_STAT_CELLS; j += RG_THREADS) {
    const int i = base + j;
    if (i >= N) break;
    const int lab = labels[qoff + i];
    if (lab < 0) continue;
    const int k = slot[qoff + lab];
    if (k < 0) continue;
    const int r = i / cols, c = i - r * cols;
    const float p = prob[qoff + i];                                   // >= level > 0: the bits order as the values do
    atomicMin(&bb_s[k][0], r);
    atomicMin(&bb_s[k][1], c);
    atomicMax(&bb_s[k][2], r);
    atomicMax(&bb_s[k][3], c);
    atomicAdd(&acc_s[k][0], (u64)r);
    atomicAdd(&acc_s[k][1], (u64)c);
    atomicAdd(&acc_s[k][2], (u64)(int)(fminf(p, 1.0f) * 16777216.0f));
    atomicMax(&acc_s[k][3], ((u64)__float_as_uint(p) << 32) | (unsigned)~i);
  }
  __syncthreads();
  if (tid < K && bb_s[tid][2] >= 0) {                                  // a slot this workgroup met
    const RegionsOut o = regions_out(out, Q, K);
    const size_t s = (size_t)q * K + tid;
    atomicMin(&o.bbox[4 * s + 0], bb_s[tid][0]);
    atomicMin(&o.bbox[4 * s + 1], bb_s[tid][1]);
    atomicMax(&o.bbox[4 * s + 2], bb_s[tid][2]);
    atomicMax(&o.bbox[4 * s + 3], bb_s[tid][3]);
    atomicAdd(&o.sum_rc[2 * s], acc_s[tid][0]);
    atomicAdd(&o.sum_rc[2 * s + 1], acc_s[tid][1]);
    atomicAdd(&o.mass[s], acc_s[tid][2]);
    atomicMax(&peak_key[s], acc_s[tid][3]);
  }
}

inline bool regions_dims_ok(int Q, int N, int topk) {
  return Q >= 1 && Q <= EOD_REGIONS_Q_MAX && N >= 1 && N <= EOD_REGIONS_N_MAX && topk >= 1 && topk <= EOD_REGIONS_TOPK_MAX;
}

}  // namespace

extern "C" size_t eod_map_regions_workspace_bytes(int Q, int N, int topk) {
  if (!regions_dims_ok(Q, N, topk)) return 0;
  return up256((size_t)3 * Q * N * 4) + (size_t)Q * topk * 8;
}

extern "C" int eod_map_regions(const float* prob, int Q, int N, int cols, float level, int connectivity, int min_cells, int topk,
                               int32_t* labels, int32_t* out, void* workspace, size_t workspace_bytes, eod_stream_t stream) {
  if (!regions_dims_ok(Q, N, topk) || (connectivity != 4 && connectivity != 8) || min_cells < 1 || cols < 1 || N % cols != 0)
    return EOD_ERR_BAD_DIMS;
  if (!(level > 0.0f && level <= 1.0f)) return EOD_ERR_BAD_DIMS;      // a NaN fails both
  if (!prob || !labels || !out || !workspace) return EOD_ERR_NULL;
  auto aligned = [](const void* p, unsigned a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1u)) == 0; };
  if (!aligned(prob, 4) || !aligned(labels, 4) || !aligned(out, 8) || !aligned(workspace, 8)) return EOD_ERR_ALIGN;
  if (workspace_bytes < eod_map_regions_workspace_bytes(Q, N, topk)) return EOD_ERR_CAPACITY;
  hipStream_t s = (hipStream_t)stream;
  const size_t QN = (size_t)Q * N;
  int* parent = static_cast<int*>(workspace);
  int* area = parent + QN;
  int* slot = area + QN;
  u64* peak_key = reinterpret_cast<u64*>(static_cast<char*>(workspace) + up256(3 * QN * 4));
  int* status = out;
  int* foreground = out + 2 + Q;
  if (hipMemsetAsync(out, 0, (size_t)(2 + 2 * Q) * 4, s) != hipSuccess) return EOD_ERR_LAUNCH;
  const int rows = N / cols, conn8 = connectivity == 8;
  const int tiles_r = (rows + RG_TR - 1) / RG_TR, tiles_c = (cols + RG_TC - 1) / RG_TC;      // N <= 2^22: fewer than 2^18 tiles
  const dim3 cells((N + RG_THREADS - 1) / RG_THREADS, Q);
  hipLaunchKernelGGL(regions_tile_kernel, dim3(tiles_r * tiles_c, Q), dim3(RG_THREADS), 0, s, prob, N, rows, cols, tiles_c, level,
                     conn8, parent, area, slot, status);
  hipLaunchKernelGGL(regions_border_kernel, cells, dim3(RG_THREADS), 0, s, parent, N, cols, conn8, status);
  hipLaunchKernelGGL(regions_compress_kernel, cells, dim3(RG_THREADS), 0, s, parent, (const int*)slot, N, status);
  const dim3 chunks((N + RG_FLAT_CELLS - 1) / RG_FLAT_CELLS, Q);
  hipLaunchKernelGGL(regions_flatten_kernel, chunks, dim3(RG_FLAT_THREADS), 0, s, (const int*)parent, N, labels, area, foreground,
                     status);
  hipLaunchKernelGGL(regions_list_kernel, chunks, dim3(RG_FLAT_THREADS), 0, s, (const int*)labels, (const int*)area, parent, N,
                     min_cells, out + 2);
  hipLaunchKernelGGL(regions_select_kernel, dim3(Q), dim3(RG_SEL_THREADS), 0, s, (const int*)area, slot, (const int*)parent, N, Q, topk,
                     out, peak_key);
  hipLaunchKernelGGL(regions_stats_kernel, dim3((N + RG_STAT_CELLS - 1) / RG_STAT_CELLS, Q), dim3(RG_THREADS), 0, s, prob,
                     (const int*)labels, (const int*)slot, N, cols, Q, topk, out, peak_key);
  hipLaunchKernelGGL(regions_finish_kernel, dim3((Q * topk + RG_THREADS - 1) / RG_THREADS), dim3(RG_THREADS), 0, s, Q, topk, out,
                     (const u64*)peak_key);
  return eod_launch_status();
}
