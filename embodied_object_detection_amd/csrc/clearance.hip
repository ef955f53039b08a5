// The clearance map (eod_map_clearance; semantics in include/eod_clearance.h): for every cell of a label map the exact squared
// distance to the nearest blocked cell and that cell, the map inflated by a body's radius, and per object its territory and the
// most open cell of it.  A read-only query beside the frame.  Five kernels; what one needs of another is complete at the launch
// boundary between them, and no workgroup ever waits for another one.
//
//   clearance_init_kernel    one thread per cell.  One byte per cell to the workspace: bit 7 free, bits 0..6 the slot (CL_NOSLOT:
//                            none), found as route_init_kernel finds it: lane l holds objects[l] and passable[l], the wave compares
//                            a cell's label with all of them at once, and a ballot and a find-first give the lowest slot.  cells,
//                            territory, widest_key, open_key, counts and status to 0.
//   clearance_column_kernel  one thread per column, adjacent threads adjacent columns.  One scan down leaves in near_row the row of
//                            the last blocked cell at or above each cell (-1: none), one scan up replaces it by the row of the
//                            nearest blocked cell of the column, the upper one on a tie (it is the lower cell).  Of one column only
//                            that cell can attain a cell's minimum: any other cell of the column is further away in rows and as far
//                            in columns, or as far in rows and a higher cell.
//   clearance_row_kernel     the hot path.  A workgroup of four waves owns CL_TR = 4 rows x CL_CC = 64 columns, a wave one row, a
//                            lane one cell.  A wave stages near_row of its chunk and of CL_HALO = 64 columns either side in LDS
//                            (-1 outside the grid, so a row's end never meets the next row's start) and every lane scans outward,
//                            dx = 0, 1, 2, ..., keeping the minimum of (d2 << 32) | cell over the two candidates of each dx, from LDS
//                            up to the halo and from memory beyond it.  It stops once dx^2 > best d2: a candidate at dx^2 == best
//                            can still be a lower cell (dy = 0, to the left), none beyond it can tie or win.
//   clearance_finish_kernel  one thread per cell: owner, inflated, and the sums and keys per slot: LDS atomics, then one global
//                            atomic per slot and sum the workgroup met, as route_finish_kernel flushes.
//   clearance_widest_kernel  one thread per slot: the two halves of widest_key.
//
// EXACT: d2 is a minimum of sums of two squares of integers below 2^15, each sum below 2^31; the key orders by d2, then by cell, and
// unsigned 64-bit min and max are associative and commutative, so neither the order of the scan nor that of the atomics changes a bit.
// BOUNDS: labels, info, near_row, d2, nearest, owner and inflated are indexed by r * cols + c with 0 <= r < rows, 0 <= c < cols only,
// and by nearest[i], which is -1 (not followed) or such a cell; the LDS stage by w * CL_SW + CL_HALO + lane + dx with 0 <= w < CL_TR,
// 0 <= lane < CL_CC, |dx| <= CL_HALO, inside CL_TR * CL_SW; a slot is < 64 by construction (a bit of a ballot) and < K because
// objects[l] is -1 from lane K on.  Every loop is bounded by 64, rows or cols.
#include "eod_common.h"
#include "../../include/eod_clearance.h"
#include <climits>

namespace {

typedef unsigned long long u64;

constexpr int CL_TR = EOD_CLEARANCE_TILE_ROWS, CL_CC = EOD_CLEARANCE_CHUNK_COLS, CL_HALO = EOD_CLEARANCE_HALO_COLS;
constexpr int CL_SW = CL_CC + 2 * CL_HALO;                           // a wave's stage: the chunk and its halo
constexpr int CL_K = EOD_CLEARANCE_K_MAX;
constexpr unsigned CL_FREE = 0x80u, CL_NOSLOT = 0x7Fu;               // a cell's byte: free | slot
constexpr u64 CL_NONE = ~0ull;
static_assert(CL_K == 64 && EOD_CLEARANCE_P_MAX == 64, "one wave looks a label up");
static_assert(CL_CC == 64 && CL_TR >= 1 && CL_TR <= 16 && CL_HALO >= 0, "a wave owns one row of a chunk, a lane one cell");
static_assert(2ll * (EOD_CLEARANCE_DIM_MAX - 1) * (EOD_CLEARANCE_DIM_MAX - 1) < (long long)INT_MAX, "a distance is never INT_MAX");

inline size_t clearance_up256(size_t v) { return (v + 255) & ~(size_t)255; }

__global__ __launch_bounds__(256) void clearance_init_kernel(const int* __restrict__ labels, const int* __restrict__ objects,
                                                             const int* __restrict__ passable, int N, int K, int P,
                                                             unsigned char* __restrict__ info, int* __restrict__ cells,
                                                             int* __restrict__ territory, u64* __restrict__ widest_key,
                                                             u64* __restrict__ open_key, int* __restrict__ counts,
                                                             int* __restrict__ status) {
  const int i = blockIdx.x * 256 + threadIdx.x, lane = threadIdx.x & 63;
  const int obj = lane < K ? objects[lane] : -1;
  const bool has_pas = lane < P;
  const int pas = has_pas ? passable[lane] : 0;
  const int lab = i < N ? labels[i] : -1;
  unsigned slot = CL_NOSLOT;
  bool pass = false;
  u64 todo = __ballot(lab >= 0);
  for (int n = 0; n < 64 && todo; ++n) {                             // wave-uniform
    const int j = __ffsll((long long)todo) - 1;
    todo &= todo - 1;
    const int l = __shfl(lab, j, 64);
    const u64 hit = __ballot(obj >= 0 && obj == l), hit_pas = __ballot(has_pas && pas == l);
    if (lane == j) {
      if (hit) slot = (unsigned)(__ffsll((long long)hit) - 1);       // the lowest slot wins a duplicate
      pass = hit_pas != 0;
    }
  }
  if (i < N) info[i] = (unsigned char)(((lab < 0 || pass) ? CL_FREE : 0u) | slot);
  if (i < K) {
    cells[i] = 0;
    territory[i] = 0;
    widest_key[i] = 0ull;
  }
  if (i == 0) {
    open_key[0] = 0ull;
    counts[0] = 0;
    counts[1] = 0;
    counts[2] = 0;
    status[0] = 0;
    status[1] = 0;
  }
}

__global__ __launch_bounds__(64) void clearance_column_kernel(const unsigned char* __restrict__ info, int rows, int cols,
                                                              int* __restrict__ near_row) {
  const int c = blockIdx.x * 64 + threadIdx.x;
  if (c >= cols) return;
  int last = -1;
#pragma unroll 8
  for (int r = 0; r < rows; ++r) {
    if (!(info[r * cols + c] & CL_FREE)) last = r;
    near_row[r * cols + c] = last;
  }
  int next = -1;
#pragma unroll 8
  for (int r = rows - 1; r >= 0; --r) {
    const int above = near_row[r * cols + c];                        // this thread's own store of the scan down
    if (above == r) next = r;
    // the upper cell on a tie: it is the lower cell
    const int pick = above < 0 ? next : (next < 0 || r - above <= next - r) ? above : next;
    near_row[r * cols + c] = pick;
  }
}

// the candidate of one column: the blocked cell of row nr (-1: the column has none) in column cc, seen from (r, c +- dx)
__device__ __forceinline__ u64 clearance_candidate(int nr, int r, unsigned dx2, int cc, int cols) {
  if (nr < 0) return CL_NONE;
  const int dy = r - nr;
  return ((u64)(dx2 + (unsigned)(dy * dy)) << 32) | (unsigned)(nr * cols + cc);
}

__global__ __launch_bounds__(CL_TR * 64) void clearance_row_kernel(const int* __restrict__ near_row, int rows, int cols,
                                                                   int* __restrict__ d2, int* __restrict__ nearest) {
  __shared__ int near_s[CL_TR * CL_SW];                              // 3 KB
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int r = blockIdx.y * CL_TR + w, c0 = blockIdx.x * CL_CC, c = c0 + lane;
  int* s = near_s + w * CL_SW;
  for (int t = lane; t < CL_SW; t += 64) {
    const int cc = c0 - CL_HALO + t;
    s[t] = (r < rows && cc >= 0 && cc < cols) ? near_row[r * cols + cc] : -1;
  }
  __syncthreads();
  if (r >= rows || c >= cols) return;
  const int* row = near_row + r * cols;
  const int pos = CL_HALO + lane;
  u64 best = clearance_candidate(s[pos], r, 0u, c, cols);
  const int reach = max(c, cols - 1 - c);                            // further out both candidates lie outside the grid
  const int near_end = min(reach, CL_HALO);
  int dx = 1;
  for (; dx <= near_end; ++dx) {                                     // at most CL_HALO: from the stage
    const unsigned dx2 = (unsigned)(dx * dx);
    if (dx2 > (unsigned)(best >> 32)) break;                         // CL_NONE: 0xFFFFFFFF, above every square
    best = min(best, clearance_candidate(s[pos - dx], r, dx2, c - dx, cols));      // -1 in the stage outside the grid
    best = min(best, clearance_candidate(s[pos + dx], r, dx2, c + dx, cols));
  }
  if (dx > near_end) {                                               // not stopped yet
    for (; dx <= reach; ++dx) {                                      // fewer than cols: from memory
      const unsigned dx2 = (unsigned)(dx * dx);
      if (dx2 > (unsigned)(best >> 32)) break;
      const int cl = c - dx, cr = c + dx;
      best = min(best, clearance_candidate(cl >= 0 ? row[cl] : -1, r, dx2, cl, cols));
      best = min(best, clearance_candidate(cr < cols ? row[cr] : -1, r, dx2, cr, cols));
    }
  }
  const int i = r * cols + c;
  d2[i] = best == CL_NONE ? INT_MAX : (int)(unsigned)(best >> 32);
  nearest[i] = best == CL_NONE ? -1 : (int)(unsigned)best;
}

__global__ __launch_bounds__(256) void clearance_finish_kernel(const int* __restrict__ labels, const unsigned char* __restrict__ info,
                                                               const int* __restrict__ d2, const int* __restrict__ nearest, int N,
                                                               int cols, int radius2, int keep_cell, int* __restrict__ owner,
                                                               int* __restrict__ inflated, int* __restrict__ cells,
                                                               int* __restrict__ territory, u64* __restrict__ widest_key,
                                                               u64* __restrict__ open_key, int* __restrict__ counts) {
  __shared__ u64 key_s[CL_K + 1];                                    // the slots, then the map
  __shared__ int cells_s[CL_K], terr_s[CL_K];
  __shared__ int count_s[3];
  const int tid = threadIdx.x, lane = tid & 63;
  const int i = blockIdx.x * 256 + tid;
  if (tid < CL_K) {
    cells_s[tid] = 0;
    terr_s[tid] = 0;
  }
  if (tid <= CL_K) key_s[tid] = 0ull;
  if (tid < 3) count_s[tid] = 0;
  __syncthreads();
  bool blocked = false, free_cell = false, grown = false;
  if (i < N) {
    const unsigned v = info[i];
    const int lab = labels[i], d = d2[i], j = nearest[i];
    free_cell = (v & CL_FREE) != 0;
    blocked = !free_cell;
    const int own = j >= 0 ? labels[j] : -1;
    int inf = lab;
    if (free_cell && d <= radius2) {                                 // INT_MAX (no blocked cell) is above every radius2
      bool keep = false;
      if (keep_cell >= 0) {
        const int r = i / cols, kr = keep_cell / cols;
        const int dr = r - kr, dc = (i - r * cols) - (keep_cell - kr * cols);
        keep = (unsigned)(dr * dr) + (unsigned)(dc * dc) <= (unsigned)radius2;
      }
      if (!keep) inf = own;
    }
    grown = free_cell && inf != lab;
    owner[i] = own;
    inflated[i] = inf;
    const unsigned mine = v & CL_NOSLOT;
    if (mine != CL_NOSLOT) atomicAdd(&cells_s[mine], 1);
    if (free_cell) {
      const u64 key = ((u64)(unsigned)d << 32) | (unsigned)~(unsigned)i;
      atomicMax(&key_s[CL_K], key);
      const unsigned k = j >= 0 ? (info[j] & CL_NOSLOT) : CL_NOSLOT;
      if (k != CL_NOSLOT) {
        atomicAdd(&terr_s[k], 1);
        atomicMax(&key_s[k], key);
      }
    }
  }
  const u64 nb = __ballot(blocked), nf = __ballot(free_cell), ng = __ballot(grown);
  if (lane == 0) {
    if (nb) atomicAdd(&count_s[0], __popcll(nb));
    if (nf) atomicAdd(&count_s[1], __popcll(nf));
    if (ng) atomicAdd(&count_s[2], __popcll(ng));
  }
  __syncthreads();
  if (tid < CL_K) {                                                  // only what this workgroup met
    if (key_s[tid] != 0ull) atomicMax(&widest_key[tid], key_s[tid]);
    if (cells_s[tid] > 0) atomicAdd(&cells[tid], cells_s[tid]);
    if (terr_s[tid] > 0) atomicAdd(&territory[tid], terr_s[tid]);
  }
  if (tid == CL_K && key_s[CL_K] != 0ull) atomicMax(&open_key[0], key_s[CL_K]);
  if (tid < 3 && count_s[tid] > 0) atomicAdd(&counts[tid], count_s[tid]);
}

__global__ __launch_bounds__(64) void clearance_widest_kernel(const u64* __restrict__ widest_key, int K, int* __restrict__ widest_d2,
                                                              int* __restrict__ widest_cell) {
  const int k = threadIdx.x;
  if (k >= K) return;
  const u64 key = widest_key[k];
  widest_d2[k] = (int)(unsigned)(key >> 32);
  widest_cell[k] = key == 0ull ? -1 : (int)~(unsigned)key;          // a key of 0 would be cell 2^32 - 1: there is none
}

inline bool clearance_dims_ok(int N, int cols) {
  return N >= 1 && N <= EOD_CLEARANCE_N_MAX && cols >= 1 && N % cols == 0 && cols <= EOD_CLEARANCE_DIM_MAX &&
         N / cols <= EOD_CLEARANCE_DIM_MAX;
}

inline bool clearance_aligned(const void* p, unsigned a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1u)) == 0; }

}  // namespace

extern "C" size_t eod_map_clearance_workspace_bytes(int N, int cols) {
  if (!clearance_dims_ok(N, cols)) return 0;
  return clearance_up256((size_t)N) + clearance_up256((size_t)N * 4);
}

extern "C" int eod_map_clearance(const int32_t* object_labels, const int32_t* objects, const int32_t* passable, int N, int K, int P,
                                 int cols, int radius2, int keep_cell, int32_t* d2, int32_t* nearest, int32_t* owner, int32_t* inflated,
                                 int32_t* cells, int32_t* territory, uint64_t* widest_key, int32_t* widest_d2, int32_t* widest_cell,
                                 uint64_t* open_key, int32_t* counts, int32_t* status, void* workspace, size_t workspace_bytes,
                                 eod_stream_t stream) {
  if (!clearance_dims_ok(N, cols) || K < 1 || K > EOD_CLEARANCE_K_MAX || P < 0 || P > EOD_CLEARANCE_P_MAX || radius2 < 0 ||
      radius2 == INT_MAX || keep_cell < -1 || keep_cell >= N)
    return EOD_ERR_BAD_DIMS;
  if (!object_labels || !objects || (P > 0 && !passable) || !d2 || !nearest || !owner || !inflated || !cells || !territory ||
      !widest_key || !widest_d2 || !widest_cell || !open_key || !counts || !status || !workspace)
    return EOD_ERR_NULL;
  if (!clearance_aligned(object_labels, 4) || !clearance_aligned(objects, 4) || !clearance_aligned(passable, 4) ||
      !clearance_aligned(d2, 4) || !clearance_aligned(nearest, 4) || !clearance_aligned(owner, 4) || !clearance_aligned(inflated, 4) ||
      !clearance_aligned(cells, 4) || !clearance_aligned(territory, 4) || !clearance_aligned(widest_key, 8) ||
      !clearance_aligned(widest_d2, 4) || !clearance_aligned(widest_cell, 4) || !clearance_aligned(open_key, 8) ||
      !clearance_aligned(counts, 4) || !clearance_aligned(status, 4) || !clearance_aligned(workspace, 8))
    return EOD_ERR_ALIGN;
  if (workspace_bytes < eod_map_clearance_workspace_bytes(N, cols)) return EOD_ERR_CAPACITY;
  hipStream_t s = (hipStream_t)stream;
  const int rows = N / cols;
  unsigned char* info = static_cast<unsigned char*>(workspace);
  int* near_row = reinterpret_cast<int*>(info + clearance_up256((size_t)N));
  u64* wk = reinterpret_cast<u64*>(widest_key);
  u64* ok = reinterpret_cast<u64*>(open_key);
  const int per_cell = ((N > CL_K ? N : CL_K) + 255) / 256;
  hipLaunchKernelGGL(clearance_init_kernel, dim3(per_cell), dim3(256), 0, s, (const int*)object_labels, (const int*)objects,
                     (const int*)passable, N, K, P, info, (int*)cells, (int*)territory, wk, ok, (int*)counts, (int*)status);
  hipLaunchKernelGGL(clearance_column_kernel, dim3((cols + 63) / 64), dim3(64), 0, s, (const unsigned char*)info, rows, cols, near_row);
  hipLaunchKernelGGL(clearance_row_kernel, dim3((cols + CL_CC - 1) / CL_CC, (rows + CL_TR - 1) / CL_TR), dim3(CL_TR * 64), 0, s,
                     (const int*)near_row, rows, cols, (int*)d2, (int*)nearest);
  hipLaunchKernelGGL(clearance_finish_kernel, dim3((N + 255) / 256), dim3(256), 0, s, (const int*)object_labels,
                     (const unsigned char*)info, (const int*)d2, (const int*)nearest, N, cols, radius2, keep_cell, (int*)owner,
                     (int*)inflated, (int*)cells, (int*)territory, wk, ok, (int*)counts);
  hipLaunchKernelGGL(clearance_widest_kernel, dim3(1), dim3(64), 0, s, (const u64*)wk, K, (int*)widest_d2, (int*)widest_cell);
  return eod_launch_status();
}
