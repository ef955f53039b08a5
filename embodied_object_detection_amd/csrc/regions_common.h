// The union-find machinery that the map queries on connected components share (regions.hip: eod_map_regions; inventory.hip:
// eod_map_inventory): the constants, find and union in LDS and on the global parent array, and the launches that see only
// `parent`, `area`, `slot`, the list of roots and the ranked slots of `out` (compress, flatten, list, select, finish).  What decides
// which cells are adjacent (the tile and the border kernels) and what is summed per slot (the stats kernels) stays with each query.
// THE INVARIANT and the bounds of the loops are stated once, at the top of regions.hip; every function here keeps them.
#pragma once
#include "eod_common.h"
#include "../../include/eod_regions.h"
#include <climits>

namespace {

typedef unsigned long long u64;

constexpr int RG_TR = EOD_REGIONS_TILE_ROWS, RG_TC = EOD_REGIONS_TILE_COLS;
constexpr int RG_TILE = RG_TR * RG_TC;           // 1024 cells: 4 KB of LDS, four cells per thread
constexpr int RG_THREADS = 256;
constexpr int RG_FLAT_THREADS = 1024, RG_FLAT_CELLS = 4096;      // flatten, list: a workgroup's cells share its adds
constexpr int RG_FLAT_TABLE_LOG2 = 11, RG_FLAT_TABLE = 1 << RG_FLAT_TABLE_LOG2, RG_FLAT_PROBES = 16;
constexpr int RG_FIND_CAP = EOD_REGIONS_N_MAX;   // hops of one find on the global parent
constexpr int RG_HOOK_CAP = EOD_REGIONS_N_MAX;   // retries of one union
constexpr int RG_SEL_THREADS = 1024;
constexpr int RG_STAT_CELLS = 2048;              // cells per workgroup of the stats kernel
constexpr int RG_ST_FIND = 1, RG_ST_HOOK = 2, RG_ST_TILE = 4;
static_assert((RG_TC & (RG_TC - 1)) == 0 && (RG_TR & (RG_TR - 1)) == 0 && RG_TILE % RG_THREADS == 0, "tile");

__device__ __forceinline__ int lds_ld(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
__device__ __forceinline__ int agent_ld(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// LDS: the root of x; at most RG_TILE hops (it descends)
__device__ __forceinline__ int tile_find(const int* p_s, int x, int* __restrict__ status) {
  for (int n = 0; n < RG_TILE; ++n) {
    const int y = lds_ld(&p_s[x]);
    if (y == x) return x;
    x = y;
  }
  atomicOr(status, RG_ST_TILE);
  return x;
}

__device__ __forceinline__ void tile_union(int* p_s, int a, int b, int* __restrict__ status) {
  for (int n = 0; n < RG_TILE; ++n) {
    a = tile_find(p_s, a, status);
    b = tile_find(p_s, b, status);
    if (a == b) return;
    if (a < b) { const int t = a; a = b; b = t; }
    const int old = atomicMin(&p_s[a], b);        // a > b
    if (old == a) return;                         // a was a root: hooked
    a = old;                                      // it had the parent old < a; p_s[a] is min(old, b) now: go on with (old, b)
  }
  atomicOr(status, RG_ST_TILE);
}

// global parent, launch 2: stale reads allowed (see the invariant at the top of regions.hip)
__device__ __forceinline__ int grid_find(const int* p, int x, int* __restrict__ status) {
  for (int n = 0; n < RG_FIND_CAP; ++n) {
    const int y = agent_ld(&p[x]);
    if (y == x) return x;
    x = y;
  }
  atomicOr(status, RG_ST_FIND);
  return x;
}

__device__ __forceinline__ void grid_union(int* p, int a, int b, int* __restrict__ status) {
  for (int n = 0; n < RG_HOOK_CAP; ++n) {
    a = grid_find(p, a, status);
    b = grid_find(p, b, status);
    if (a == b) return;
    if (a < b) { const int t = a; a = b; b = t; }
    const int old = atomicMin(&p[a], b);          // a > b, both of one component
    if (old == a) return;                         // a was a root: hooked
    a = old;                                      // retry from what the atomic returned: (old, b), old < a
  }
  atomicOr(status, RG_ST_HOOK);
}

// launch 3: the roots are final; a tile-local root's parent goes from some ancestor to its root (agent-scope loads and stores: other
// threads read the entry meanwhile and may find either)
__global__ __launch_bounds__(RG_THREADS) void regions_compress_kernel(int* __restrict__ parent, const int* __restrict__ slot, int N,
                                                                       int* __restrict__ status) {
  const int i = blockIdx.x * RG_THREADS + threadIdx.x;
  if (i >= N) return;
  const size_t qoff = (size_t)blockIdx.y * N;
  if (slot[qoff + i] != -2) return;
  int* p = parent + qoff;
  const int up = agent_ld(&p[i]);
  if (up == i) return;
  __hip_atomic_store(&p[i], grid_find(p, up, status), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// launch 4: parent is final; every thread stays to the end (ballots, barriers).  One add to the same address from every wave is
// what this launch would spend its time on (thousands of waves share the root of a large component), so a workgroup counts its
// RG_FLAT_CELLS cells per root in an LDS table first (open addressing as in place_masks_kernel; an insert that finds no entry
// within its probes adds to area directly, which is the same sum) and adds each entry once.
__global__ __launch_bounds__(RG_FLAT_THREADS) void regions_flatten_kernel(const int* __restrict__ parent, int N, int* __restrict__ labels,
                                                                           int* __restrict__ area, int* __restrict__ foreground,
                                                                           int* __restrict__ status) {
  __shared__ int key_s[RG_FLAT_TABLE], cnt_s[RG_FLAT_TABLE];
  __shared__ int fg_s;
  const int tid = threadIdx.x, lane = tid & 63;
  const size_t qoff = (size_t)blockIdx.y * N;
  for (int e = tid; e < RG_FLAT_TABLE; e += RG_FLAT_THREADS) {
    key_s[e] = -1;
    cnt_s[e] = 0;
  }
  if (tid == 0) fg_s = 0;
  __syncthreads();
  for (int j = 0; j < RG_FLAT_CELLS / RG_FLAT_THREADS; ++j) {
    const int i = blockIdx.x * RG_FLAT_CELLS + j * RG_FLAT_THREADS + tid;
    int root = -1;
    if (i < N) {
      root = parent[qoff + i];
      if (root >= 0) {
        int n = 0;
        for (; n < RG_FIND_CAP; ++n) {                               // two hops after launch 3: the tile-local root, the root
          const int y = parent[qoff + root];
          if (y == root) break;
          root = y;
        }
        if (n == RG_FIND_CAP) atomicOr(status, RG_ST_FIND);
      }
      labels[qoff + i] = root;
    }
    // the cells of the wave that share the root of its first foreground cell count as one insert
    const bool fg = root >= 0;
    const u64 m = __ballot(fg);
    if (!m) continue;                                                // wave-uniform
    const int lead = __ffsll((long long)m) - 1;
    const int first = __shfl(root, lead, 64);
    const u64 same = __ballot(fg && root == first);
    if (lane == lead) atomicAdd(&fg_s, __popcll(m));
    if (!fg || (root == first && lane != lead)) continue;
    const int n = root == first ? __popcll(same) : 1;
    unsigned h = ((unsigned)root * 2654435761u) >> (32 - RG_FLAT_TABLE_LOG2);
    bool done = false;
    for (int probe = 0; probe < RG_FLAT_PROBES && !done; ++probe) {
      int old = lds_ld(&key_s[h]);
      if (old == -1) old = atomicCAS(&key_s[h], -1, root);
      if (old == -1 || old == root) {
        atomicAdd(&cnt_s[h], n);
        done = true;
      }
      h = (h + 1) & (RG_FLAT_TABLE - 1);
    }
    if (!done) atomicAdd(&area[qoff + root], n);
  }
  __syncthreads();
  for (int e = tid; e < RG_FLAT_TABLE; e += RG_FLAT_THREADS)
    if (key_s[e] >= 0) atomicAdd(&area[qoff + key_s[e]], cnt_s[e]);
  if (tid == 0 && fg_s) atomicAdd(&foreground[blockIdx.y], fg_s);
}

// launch 5: area is final.  A workgroup gathers the roots among its RG_FLAT_CELLS cells in LDS and takes its place in the list with
// one add to count[q].
__global__ __launch_bounds__(RG_FLAT_THREADS) void regions_list_kernel(const int* __restrict__ labels, const int* __restrict__ area,
                                                                        int* __restrict__ lists, int N, int min_cells,
                                                                        int* __restrict__ count) {
  __shared__ int buf_s[RG_FLAT_CELLS];
  __shared__ int n_s, base_s;
  const int tid = threadIdx.x, lane = tid & 63;
  const size_t qoff = (size_t)blockIdx.y * N;
  if (tid == 0) n_s = 0;
  __syncthreads();
  for (int j = 0; j < RG_FLAT_CELLS / RG_FLAT_THREADS; ++j) {
    const int i = blockIdx.x * RG_FLAT_CELLS + j * RG_FLAT_THREADS + tid;
    const bool take = i < N && labels[qoff + i] == i && area[qoff + i] >= min_cells;
    const u64 m = __ballot(take);
    if (!m) continue;                                                // wave-uniform
    const int lead = __ffsll((long long)m) - 1;
    int base = 0;
    if (lane == lead) base = atomicAdd(&n_s, __popcll(m));
    base = __shfl(base, lead, 64);
    if (take) buf_s[base + __popcll(m & ((1ull << lane) - 1ull))] = i;            // at most one entry per cell of the workgroup
  }
  __syncthreads();
  if (tid == 0 && n_s) base_s = atomicAdd(&count[blockIdx.y], n_s);
  __syncthreads();
  for (int e = tid; e < n_s; e += RG_FLAT_THREADS) lists[qoff + base_s + e] = buf_s[e];   // at most N roots: inside the class's [N]
}

struct RegionsOut {      // the arrays of `out` (include/eod_regions.h); include/eod_inventory.h begins with the same ones
  int *count, *region, *area, *peak, *peak_prob, *bbox;
  u64 *sum_rc, *mass;
};
__device__ __host__ __forceinline__ RegionsOut regions_out(int* out, int Q, int K) {
  RegionsOut o;
  int* b = out + 2 + 2 * Q;
  const size_t QK = (size_t)Q * K;
  o.count = out + 2;
  o.region = b; o.area = b + QK; o.peak = b + 2 * QK; o.peak_prob = b + 3 * QK; o.bbox = b + 4 * QK;
  o.sum_rc = reinterpret_cast<u64*>(b + 8 * QK);
  o.mass = reinterpret_cast<u64*>(b + 12 * QK);
  return o;
}

__global__ __launch_bounds__(RG_SEL_THREADS) void regions_select_kernel(const int* __restrict__ area, int* __restrict__ slot,
                                                                         const int* __restrict__ lists, int N, int Q, int K,
                                                                         int* __restrict__ out, u64* __restrict__ peak_key) {
  __shared__ u64 red_s[RG_SEL_THREADS / 64];
  const int tid = threadIdx.x, q = blockIdx.x;
  const size_t qoff = (size_t)q * N;
  const int* list = lists + qoff;                                     // regions_list_kernel's, in the class's [N] of parent
  const RegionsOut o = regions_out(out, Q, K);
  const int n = o.count[q] < N ? o.count[q] : N;
  u64 prev = ~0ull;                                                   // above every key
  for (int k = 0; k < K; ++k) {
    u64 best = 0ull;                                                  // below every key: a listed area is at least 1
    if (prev) {                                                       // block-uniform
      for (int j = tid; j < n; j += RG_SEL_THREADS) {
        const int root = list[j];
        const u64 key = ((u64)(unsigned)area[qoff + root] << 32) | (unsigned)~root;
        if (key < prev && key > best) best = key;
      }
    }
    prev = block_max_u64(best, red_s);                                // 0 once the components are used up: the rest is padding
    if (tid == 0) {
      const size_t s = (size_t)q * K + k;
      const int root = (int)~(unsigned)prev;
      o.region[s] = prev ? root : -1;
      o.area[s] = (int)(prev >> 32);
      o.peak[s] = 0;
      o.peak_prob[s] = 0;
      o.bbox[4 * s + 0] = prev ? INT_MAX : 0;
      o.bbox[4 * s + 1] = prev ? INT_MAX : 0;
      o.bbox[4 * s + 2] = prev ? -1 : 0;
      o.bbox[4 * s + 3] = prev ? -1 : 0;
      o.sum_rc[2 * s] = 0ull;
      o.sum_rc[2 * s + 1] = 0ull;
      o.mass[s] = 0ull;
      peak_key[s] = 0ull;
      if (prev) slot[qoff + root] = k;
    }
  }
}

__global__ __launch_bounds__(RG_THREADS) void regions_finish_kernel(int Q, int K, int* __restrict__ out, const u64* __restrict__ peak_key) {
  const int s = blockIdx.x * RG_THREADS + threadIdx.x;
  if (s >= Q * K) return;
  const RegionsOut o = regions_out(out, Q, K);
  if (o.region[s] < 0) return;                                        // padding: zeros from the select kernel
  const u64 key = peak_key[s];
  o.peak[s] = (int)~(unsigned)key;
  o.peak_prob[s] = (int)(unsigned)(key >> 32);
}

inline size_t up256(size_t v) { return (v + 255) / 256 * 256; }

}  // namespace
