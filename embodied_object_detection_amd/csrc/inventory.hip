// Map inventory: every object of B label maps, all classes in one call (eod_map_inventory; semantics in include/eod_inventory.h).
// The connected components of eod_map_regions with one more condition on adjacency: the two cells carry the same class.  A
// read-only query: integers and comparisons only, integer atomics only, the result a pure function of the inputs.  Eleven launches;
// what one needs of another is complete at the launch boundary between them, and no workgroup ever waits for another one (no spin,
// no flag, no grid barrier).  A map b takes the place of a class q of regions.hip, and the ranked slots of `out` begin with the
// arrays of eod_map_regions, so the launches of regions_common.h run here as they are.
//
//   inventory_init_kernel     status, count, foreground, class_objects, class_cells and the class keys to 0, cls to -1.
//   inventory_tile_kernel     regions_tile_kernel with each cell's class beside its parent in LDS (-1: background): a cell unites
//                             itself with a neighbour before it only where the classes are equal.
//   inventory_border_kernel   regions_border_kernel; a neighbour in another tile is united only where it is foreground (parent >= 0)
//                             and its label equals this cell's.  At a four-tile corner the diagonal pair of equal classes is the only
//                             link, whatever the other diagonal holds.
//   regions_compress_kernel, regions_flatten_kernel, regions_list_kernel, regions_select_kernel      (regions_common.h)
//   inventory_classes_kernel  the table of the classes.  class_cells: every foreground cell, counted per workgroup in an LDS histogram
//                             first (and per wave before that, as in the flatten kernel), one global add per class and workgroup.
//                             From the list of roots (area >= min_cells): class_objects += 1 and the 64-bit maximum of
//                             (area << 32) | ~label per class, through LDS likewise.
//   inventory_stats_kernel    regions_stats_kernel on `scores`; the thread that holds a ranked root also stores its class.
//   regions_finish_kernel     (regions_common.h) the peak keys become peak and peak_score.
//   inventory_finish_kernel   the class keys become class_largest and class_largest_area.
//
// THE INVARIANT of regions.hip carries over word for word: every value ever stored in parent[x] is a member of x's component and is
// <= x.  The tile kernel stores the smallest cell of x's part of the tile, united under the new adjacency only; the border kernel
// hooks with atomicMin the root of a cell adjacent to x's tree, under the new adjacency only.  Neither the classes nor the scores
// change during the call, so whether two cells are adjacent never depends on when it is asked.  The bounds of the loops are those of
// regions.hip (RG_TILE hops in LDS, RG_FIND_CAP and RG_HOOK_CAP globally); a thread that reaches one stops and sets status.
#include "regions_common.h"
#include "../../include/eod_inventory.h"

namespace {

static_assert(EOD_INVENTORY_B_MAX == EOD_REGIONS_Q_MAX && EOD_INVENTORY_TOPK_MAX == EOD_REGIONS_TOPK_MAX &&
              EOD_INVENTORY_N_MAX == EOD_REGIONS_N_MAX, "the shared launches take a map for a class of eod_map_regions");
constexpr int IV_CLASSES = 2048;                 // LDS entries of the class tables: C <= EOD_INVENTORY_C_MAX
static_assert(EOD_INVENTORY_C_MAX < IV_CLASSES, "class tables");

struct InventoryOut {    // the arrays of `out` behind those of RegionsOut (include/eod_inventory.h)
  int *cls, *class_objects, *class_cells, *class_largest, *class_largest_area;
};
__device__ __host__ __forceinline__ InventoryOut inventory_out(int* out, int B, int K, int C) {
  InventoryOut o;
  const size_t BK = (size_t)B * K, BC = (size_t)B * C;
  o.cls = out + 2 + 2 * B + 14 * BK;
  o.class_objects = o.cls + BK;
  o.class_cells = o.class_objects + BC;
  o.class_largest = o.class_cells + BC;
  o.class_largest_area = o.class_largest + BC;
  return o;
}

__global__ __launch_bounds__(RG_THREADS) void inventory_init_kernel(int B, int K, int C, int* __restrict__ out,
                                                                     u64* __restrict__ class_key) {
  const int i = blockIdx.x * RG_THREADS + threadIdx.x;
  const InventoryOut o = inventory_out(out, B, K, C);
  if (i < 2 + 2 * B) out[i] = 0;
  if (i < B * K) o.cls[i] = -1;
  if (i < B * C) {
    o.class_objects[i] = 0;
    o.class_cells[i] = 0;
    class_key[i] = 0ull;
  }
}

__global__ __launch_bounds__(RG_THREADS) void inventory_tile_kernel(const int* __restrict__ cls, const float* __restrict__ scores,
                                                                     const unsigned char* __restrict__ keep, int N, int rows, int cols,
                                                                     int tiles_c, int C, float level, int conn8, int* __restrict__ parent,
                                                                     int* __restrict__ area, int* __restrict__ slot,
                                                                     int* __restrict__ status) {
  __shared__ int p_s[RG_TILE], c_s[RG_TILE];
  const int tid = threadIdx.x;
  const int ty = blockIdx.x / tiles_c, tx = blockIdx.x - ty * tiles_c;
  const int r0 = ty * RG_TR, c0 = tx * RG_TC;
  const size_t boff = (size_t)blockIdx.y * N;
  for (int l = tid; l < RG_TILE; l += RG_THREADS) {
    const int r = r0 + l / RG_TC, c = c0 + (l & (RG_TC - 1));
    int v = -1, cl = -1;
    if (r < rows && c < cols) {
      const size_t g = boff + r * cols + c;
      const int lab = cls[g];
      if ((unsigned)lab < (unsigned)C && (!keep || keep[lab]) && scores[g] >= level) {       // a NaN compares false
        v = l;
        cl = lab;
      }
    }
    p_s[l] = v;
    c_s[l] = cl;
  }
  __syncthreads();
  // a cell unites itself with the neighbours of its class before it in row-major order; c_s is -1 on the background and does not
  // change, so an equal class says foreground too
  for (int l = tid; l < RG_TILE; l += RG_THREADS) {
    const int cl = c_s[l];
    if (cl < 0) continue;
    const int lr = l / RG_TC, lc = l & (RG_TC - 1);
    if (lc > 0 && c_s[l - 1] == cl) tile_union(p_s, l, l - 1, status);
    if (lr > 0) {
      if (c_s[l - RG_TC] == cl) tile_union(p_s, l, l - RG_TC, status);
      if (conn8) {
        if (lc > 0 && c_s[l - RG_TC - 1] == cl) tile_union(p_s, l, l - RG_TC - 1, status);
        if (lc < RG_TC - 1 && c_s[l - RG_TC + 1] == cl) tile_union(p_s, l, l - RG_TC + 1, status);
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
    const size_t g = boff + r * cols + c;
    parent[g] = v;
    area[g] = 0;
    slot[g] = local_root ? -2 : -1;
  }
}

__global__ __launch_bounds__(RG_THREADS) void inventory_border_kernel(int* __restrict__ parent, const int* __restrict__ cls, int N, int cols,
                                                                       int conn8, int* __restrict__ status) {
  const int i = blockIdx.x * RG_THREADS + threadIdx.x;
  if (i >= N) return;
  const int r = i / cols, c = i - r * cols;
  const int lr = r & (RG_TR - 1), lc = c & (RG_TC - 1);
  if (lr != 0 && lc != 0 && lc != RG_TC - 1) return;                 // all four neighbours before it are in its own tile
  int* p = parent + (size_t)blockIdx.y * N;
  if (agent_ld(&p[i]) < 0) return;
  const int* k = cls + (size_t)blockIdx.y * N;
  const int mine = k[i];
  // a neighbour is united where it is foreground and of this cell's class (a background cell may carry any label, this one too)
  auto joins = [&](int j) { return agent_ld(&p[j]) >= 0 && k[j] == mine; };
  // the row and the column are the grid's: c > 0 and c < cols - 1 keep (r, 0) away from (r - 1, cols - 1) and from (r, cols - 1)
  if (lc == 0 && c > 0 && joins(i - 1)) grid_union(p, i, i - 1, status);
  if (r > 0) {
    if (lr == 0 && joins(i - cols)) grid_union(p, i, i - cols, status);
    if (conn8) {
      if (c > 0 && (lr == 0 || lc == 0) && joins(i - cols - 1)) grid_union(p, i, i - cols - 1, status);
      if (c < cols - 1 && (lr == 0 || lc == RG_TC - 1) && joins(i - cols + 1)) grid_union(p, i, i - cols + 1, status);
    }
  }
}

// after the list kernel: object_labels, area and the list (in parent's storage) are final.  Workgroup x of map b takes the cells and
// the list entries [x RG_FLAT_CELLS, (x + 1) RG_FLAT_CELLS).  Every thread stays to the end (ballots, barriers).
__global__ __launch_bounds__(RG_FLAT_THREADS) void inventory_classes_kernel(const int* __restrict__ cls, const int* __restrict__ object_labels,
                                                                             const int* __restrict__ area, const int* __restrict__ lists,
                                                                             int N, int B, int K, int C, int* __restrict__ out,
                                                                             u64* __restrict__ class_key) {
  __shared__ int cells_s[IV_CLASSES], objs_s[IV_CLASSES];
  __shared__ u64 key_s[IV_CLASSES];
  const int tid = threadIdx.x, lane = tid & 63, b = blockIdx.y;
  const size_t boff = (size_t)b * N;
  for (int e = tid; e < C; e += RG_FLAT_THREADS) {
    cells_s[e] = 0;
    objs_s[e] = 0;
    key_s[e] = 0ull;
  }
  __syncthreads();
  const int n = out[2 + b] < N ? out[2 + b] : N;                       // count[b]: the entries of the list
  for (int j = 0; j < RG_FLAT_CELLS / RG_FLAT_THREADS; ++j) {
    const int i = blockIdx.x * RG_FLAT_CELLS + j * RG_FLAT_THREADS + tid;
    if (i < n) {
      const int root = lists[boff + i];
      const int cl = cls[boff + root];                                 // a root is foreground: 0 <= cl < C
      atomicAdd(&objs_s[cl], 1);
      atomicMax(&key_s[cl], ((u64)(unsigned)area[boff + root] << 32) | (unsigned)~root);
    }
    // the cells of the wave that carry the class of its first foreground cell count as one add
    const bool fg = i < N && object_labels[boff + i] >= 0;
    const int cl = fg ? cls[boff + i] : -1;
    const u64 m = __ballot(fg);
    if (!m) continue;                                                  // wave-uniform
    const int lead = __ffsll((long long)m) - 1;
    const int first = __shfl(cl, lead, 64);
    const u64 same = __ballot(fg && cl == first);
    if (!fg || (cl == first && lane != lead)) continue;
    atomicAdd(&cells_s[cl], cl == first ? __popcll(same) : 1);
  }
  __syncthreads();
  const InventoryOut o = inventory_out(out, B, K, C);
  for (int e = tid; e < C; e += RG_FLAT_THREADS) {
    const size_t t = (size_t)b * C + e;
    if (cells_s[e]) atomicAdd(&o.class_cells[t], cells_s[e]);
    if (objs_s[e]) {
      atomicAdd(&o.class_objects[t], objs_s[e]);
      atomicMax(&class_key[t], key_s[e]);
    }
  }
}

__global__ __launch_bounds__(RG_THREADS) void inventory_stats_kernel(const int* __restrict__ cls, const float* __restrict__ scores,
                                                                      const int* __restrict__ labels, const int* __restrict__ slot, int N,
                                                                      int cols, int B, int K, int C, int* __restrict__ out,
                                                                      u64* __restrict__ peak_key) {
  __shared__ int bb_s[EOD_INVENTORY_TOPK_MAX][4];
  __shared__ u64 acc_s[EOD_INVENTORY_TOPK_MAX][4];                    // sum of rows, sum of columns, mass, peak key
  const int tid = threadIdx.x, b = blockIdx.y;
  const size_t boff = (size_t)b * N;
  if (tid < K) {
    bb_s[tid][0] = INT_MAX; bb_s[tid][1] = INT_MAX; bb_s[tid][2] = -1; bb_s[tid][3] = -1;
    acc_s[tid][0] = 0ull; acc_s[tid][1] = 0ull; acc_s[tid][2] = 0ull; acc_s[tid][3] = 0ull;
  }
  __syncthreads();
  const int base = blockIdx.x * RG_STAT_CELLS;
  for (int j = tid; j < RG_STAT_CELLS; j += RG_THREADS) {
    const int i = base + j;
    if (i >= N) break;
    const int lab = labels[boff + i];
    if (lab < 0) continue;
    const int k = slot[boff + lab];
    if (k < 0) continue;
    const int r = i / cols, c = i - r * cols;
    const float p = scores[boff + i];                                 // >= level > 0: the bits order as the values do
    if (lab == i) inventory_out(out, B, K, C).cls[(size_t)b * K + k] = cls[boff + i];      // the root: one thread per slot
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
    const RegionsOut o = regions_out(out, B, K);
    const size_t s = (size_t)b * K + tid;
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

__global__ __launch_bounds__(RG_THREADS) void inventory_finish_kernel(int B, int K, int C, int* __restrict__ out,
                                                                       const u64* __restrict__ class_key) {
  const int t = blockIdx.x * RG_THREADS + threadIdx.x;
  if (t >= B * C) return;
  const InventoryOut o = inventory_out(out, B, K, C);
  const u64 key = class_key[t];                                       // 0: no component of the class (a listed area is at least 1)
  o.class_largest[t] = key ? (int)~(unsigned)key : -1;
  o.class_largest_area[t] = (int)(key >> 32);
}

inline bool inventory_dims_ok(int B, int N, int C, int topk) {
  return B >= 1 && B <= EOD_INVENTORY_B_MAX && N >= 1 && N <= EOD_INVENTORY_N_MAX && C >= 1 && C <= EOD_INVENTORY_C_MAX && topk >= 1 &&
         topk <= EOD_INVENTORY_TOPK_MAX;
}

}  // namespace

extern "C" size_t eod_map_inventory_workspace_bytes(int B, int N, int C, int topk) {
  if (!inventory_dims_ok(B, N, C, topk)) return 0;
  return up256((size_t)3 * B * N * 4) + (size_t)B * topk * 8 + (size_t)B * C * 8;
}

extern "C" int eod_map_inventory(const int32_t* labels, const float* scores, const uint8_t* keep, int B, int N, int cols, int C,
                                 float level, int connectivity, int min_cells, int topk, int32_t* object_labels, int32_t* out,
                                 void* workspace, size_t workspace_bytes, eod_stream_t stream) {
  if (!inventory_dims_ok(B, N, C, topk) || (connectivity != 4 && connectivity != 8) || min_cells < 1 || cols < 1 || N % cols != 0)
    return EOD_ERR_BAD_DIMS;
  if (!(level > 0.0f && level <= 1.0f)) return EOD_ERR_BAD_DIMS;      // a NaN fails both
  if (!labels || !scores || !object_labels || !out || !workspace) return EOD_ERR_NULL;          // keep may be null
  auto aligned = [](const void* p, unsigned a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1u)) == 0; };
  if (!aligned(labels, 4) || !aligned(scores, 4) || !aligned(object_labels, 4) || !aligned(out, 8) || !aligned(workspace, 8))
    return EOD_ERR_ALIGN;
  if (workspace_bytes < eod_map_inventory_workspace_bytes(B, N, C, topk)) return EOD_ERR_CAPACITY;
  hipStream_t s = (hipStream_t)stream;
  const size_t BN = (size_t)B * N;
  int* parent = static_cast<int*>(workspace);
  int* area = parent + BN;
  int* slot = area + BN;
  u64* peak_key = reinterpret_cast<u64*>(static_cast<char*>(workspace) + up256(3 * BN * 4));
  u64* class_key = peak_key + (size_t)B * topk;
  int* status = out;
  int* foreground = out + 2 + B;
  const int rows = N / cols, conn8 = connectivity == 8;
  const int tiles_r = (rows + RG_TR - 1) / RG_TR, tiles_c = (cols + RG_TC - 1) / RG_TC;      // N <= 2^22: fewer than 2^18 tiles
  int init = 2 + 2 * B;
  if (B * topk > init) init = B * topk;
  if (B * C > init) init = B * C;
  hipLaunchKernelGGL(inventory_init_kernel, dim3((init + RG_THREADS - 1) / RG_THREADS), dim3(RG_THREADS), 0, s, B, topk, C, out, class_key);
  const dim3 cells((N + RG_THREADS - 1) / RG_THREADS, B);
  hipLaunchKernelGGL(inventory_tile_kernel, dim3(tiles_r * tiles_c, B), dim3(RG_THREADS), 0, s, (const int*)labels, scores, keep, N, rows,
                     cols, tiles_c, C, level, conn8, parent, area, slot, status);
  hipLaunchKernelGGL(inventory_border_kernel, cells, dim3(RG_THREADS), 0, s, parent, (const int*)labels, N, cols, conn8, status);
  hipLaunchKernelGGL(regions_compress_kernel, cells, dim3(RG_THREADS), 0, s, parent, (const int*)slot, N, status);
  const dim3 chunks((N + RG_FLAT_CELLS - 1) / RG_FLAT_CELLS, B);
  hipLaunchKernelGGL(regions_flatten_kernel, chunks, dim3(RG_FLAT_THREADS), 0, s, (const int*)parent, N, object_labels, area, foreground,
                     status);
  hipLaunchKernelGGL(regions_list_kernel, chunks, dim3(RG_FLAT_THREADS), 0, s, (const int*)object_labels, (const int*)area, parent, N,
                     min_cells, out + 2);
  hipLaunchKernelGGL(regions_select_kernel, dim3(B), dim3(RG_SEL_THREADS), 0, s, (const int*)area, slot, (const int*)parent, N, B, topk,
                     out, peak_key);
  hipLaunchKernelGGL(inventory_classes_kernel, chunks, dim3(RG_FLAT_THREADS), 0, s, (const int*)labels, (const int*)object_labels,
                     (const int*)area, (const int*)parent, N, B, topk, C, out, class_key);
  hipLaunchKernelGGL(inventory_stats_kernel, dim3((N + RG_STAT_CELLS - 1) / RG_STAT_CELLS, B), dim3(RG_THREADS), 0, s, (const int*)labels,
                     scores, (const int*)object_labels, (const int*)slot, N, cols, B, topk, C, out, peak_key);
  hipLaunchKernelGGL(regions_finish_kernel, dim3((B * topk + RG_THREADS - 1) / RG_THREADS), dim3(RG_THREADS), 0, s, B, topk, out,
                     (const u64*)peak_key);
  hipLaunchKernelGGL(inventory_finish_kernel, dim3((B * C + RG_THREADS - 1) / RG_THREADS), dim3(RG_THREADS), 0, s, B, topk, C, out,
                     (const u64*)class_key);
  return eod_launch_status();
}
