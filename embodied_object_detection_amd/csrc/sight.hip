// Line of sight on the map (eod_map_sight; semantics in include/eod_sight.h): which cells each of up to 64 source cells sees along
// the rounded straight line to them, and how much of every object.  A read-only query beside the frame.  Three kernels; what one
// needs of another is complete at the launch boundary between them, and no workgroup ever waits for another one.
//
//   sight_init_kernel    one thread per cell.  One byte per cell to the workspace: bit 7 transparent, bits 0..6 the slot (SI_NOSLOT:
//                        none), found as clearance_init_kernel finds it: lane l holds objects[l] and passable[l], the wave compares a
//                        cell's label with all of them at once, and a ballot and a find-first give the lowest slot.  The ballot of
//                        "opaque" over a wave is one word of the bit plane: bit b of word w is cell 64 * w + b, and the lanes beyond
//                        N vote 0.  cells, seen_cells, source_counts, counts and status to 0, near_key to all ones, and seen_mask to
//                        0 when there is more than one group of sources.
//   sight_walk_kernel    the hot path.  A workgroup of four waves owns 256 consecutive cells (blockIdx.x) and one group of
//                        EOD_SIGHT_SOURCE_GROUP sources (blockIdx.y), a thread one target cell, so the lines of a wave from one
//                        source run nearly parallel and its lanes leave the loop at about the same step.  A thread walks the line
//                        from each used source of the group (the loop over the sources is uniform) until the first opaque line
//                        cell or blocked corner, not at all when d2 > range2, and collects the answers as the bits of one register:
//                        with one group seen_mask is stored once, with more each group ORs its bits in (a 64-bit atomic; measured
//                        against one workgroup walking all 64 sources: 3.0 times faster at 200 x 200, 1.4 at 512 x 512, equal up
//                        to 16 sources, profiles/sight_variants.txt).  The coordinates of a step come from two error terms (below), no division.  The
//                        bit plane is read from LDS when the map has at most EOD_SIGHT_LDS_CELLS cells (STAGED: every workgroup
//                        copies it first, 8 coalesced 8-byte loads a thread at the most), from the workspace otherwise.  The sums
//                        and keys per (source, slot) go through LDS atomics, then one global atomic per pair the workgroup met, as
//                        clearance_finish_kernel flushes.  The first group's workgroups also count the slots' cells and the map's.
//   sight_finish_kernel  one thread per (source, slot): the halves of near_key; one thread per slot: best_key over the complete
//                        seen_cells, and its halves; with more than one group one thread per cell: counts[2] over the complete
//                        seen_mask, summed in LDS and added once per workgroup.
//
// THE ERROR TERM.  For a = |dr| (or |dc|) <= n the walk keeps q and e with 2 * i * a + n == q * 2n + e and 0 <= e < 2n, so that
// q == floor((2 * i * a + n) / (2n)) == |rnd(i * d, n)|: at i = 0, q = 0 and e = n < 2n; a step adds 2a <= 2n to e, and if that
// reaches 2n it takes 2n off and adds one to q, once, as e + 2a < 4n.  The sign goes on the step.  All of it stays below
// 4 * EOD_SIGHT_DIM_MAX; the closed form's 2 * i * a + n stays below 2^31 (asserted), which is what a reference in int32 would need.
// EXACT: the walk is integer comparisons and additions; d2 is a sum of two squares of integers below 2^15; unsigned 64-bit min, max,
// or and 32-bit add are associative and commutative, so neither the order of the walk nor that of the atomics changes a bit.
// BOUNDS: labels, info and seen_mask are indexed by i < N; the bit plane by cell >> 6 of a line or side cell, which has
// min(r0, r1) <= r <= max(r0, r1) and the same for c (0 <= q <= i <= n and the step's sign), inside the grid, so cell < N and the
// word is below ceil(N / 64), in LDS below the staged size; a slot is < 64 by construction (a bit of a ballot) and < K because
// objects[l] is -1 from lane K on; a source is < S <= 64 and the pair (s - g, slot) inside the group's arrays; seen_mask is ORed at i < N.  Every loop is
// bounded by 64, rows or cols.
#include "eod_common.h"
#include "../../include/eod_sight.h"
#include <climits>
#include <cstring>

namespace {

typedef unsigned long long u64;

constexpr int SI_K = EOD_SIGHT_K_MAX, SI_S = EOD_SIGHT_S_MAX, SI_G = EOD_SIGHT_SOURCE_GROUP;
constexpr int SI_WG = 256;                                           // threads of a workgroup of the walk: four waves
constexpr unsigned SI_CLEAR = 0x80u, SI_NOSLOT = 0x7Fu;              // a cell's byte: transparent | slot
constexpr u64 SI_NONE = ~0ull;
static_assert(SI_K == 64 && EOD_SIGHT_P_MAX == 64 && SI_S == 64, "one wave looks a label up, one bit of a word per source");
static_assert(SI_S % SI_G == 0 && SI_G * SI_K % SI_WG == 0, "a workgroup flushes a group's pairs in whole rounds");
static_assert(EOD_SIGHT_LDS_CELLS % 64 == 0 && EOD_SIGHT_LDS_CELLS / 8 <= 64 * 1024, "the staged bit plane is whole words in 64 KB");
static_assert(2ll * (EOD_SIGHT_DIM_MAX - 1) * (EOD_SIGHT_DIM_MAX - 1) < (long long)INT_MAX, "a distance is never INT_MAX");
static_assert(2ll * (EOD_SIGHT_DIM_MAX - 1) * (EOD_SIGHT_DIM_MAX - 1) + (EOD_SIGHT_DIM_MAX - 1) < (1ll << 31),
              "2 * i * |d| + n of the closed form fits 31 bits");

struct SightSources {                                                // from_cells, by value: read-only, so it stays in the kernel arguments
  int cell[SI_S];
};

inline size_t sight_up256(size_t v) { return (v + 255) & ~(size_t)255; }
inline int sight_words(int N) { return (N + 63) / 64; }

__global__ __launch_bounds__(256) void sight_init_kernel(const int* __restrict__ labels, const int* __restrict__ objects,
                                                         const int* __restrict__ passable, int N, int K, int P, int S,
                                                         unsigned char* __restrict__ info, u64* __restrict__ plane,
                                                         u64* __restrict__ seen_mask, int* __restrict__ cells, int* __restrict__ seen_cells,
                                                         u64* __restrict__ near_key, int* __restrict__ source_counts,
                                                         int* __restrict__ counts, int* __restrict__ status) {
  const int i = blockIdx.x * 256 + threadIdx.x, lane = threadIdx.x & 63;
  const int obj = lane < K ? objects[lane] : -1;
  const bool has_pas = lane < P;
  const int pas = has_pas ? passable[lane] : 0;
  const int lab = i < N ? labels[i] : -1;
  unsigned slot = SI_NOSLOT;
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
  const bool opaque = i < N && lab >= 0 && !pass;                    // a lane beyond N votes 0: the tail of the last word is clear
  const u64 word = __ballot(opaque);
  if (i < N) info[i] = (unsigned char)((opaque ? 0u : SI_CLEAR) | slot);
  if (lane == 0 && i < N) plane[i >> 6] = word;
  if (i < N && S > SI_G) seen_mask[i] = 0ull;                      // the source groups OR their bits in
  if (i < S * K) {
    seen_cells[i] = 0;
    near_key[i] = SI_NONE;
  }
  if (i < K) cells[i] = 0;
  if (i < 2 * S) source_counts[i] = 0;
  if (i < 3) counts[i] = 0;
  if (i < 2) status[i] = 0;
}

// One bit of the plane.  The source's own cell, transparent on its own lines whatever its label, is never asked for: it is line
// cell 0, the walk tests the line cells from 1 on, and the side cells of step k lie k - 1 or k cells from the source along the
// line's longer axis, which is 1 at least when both coordinates change at step 1 and k - 1 >= 1 after it.
__device__ __forceinline__ bool sight_opaque(const u64* plane, int cell) {
  return ((plane[cell >> 6] >> (cell & 63)) & 1ull) != 0;
}

template <bool STAGED>
__global__ __launch_bounds__(SI_WG) void sight_walk_kernel(const unsigned char* __restrict__ info, const u64* __restrict__ plane_g,
                                                           const SightSources src, int N, int K, int S, int cols, int range2,
                                                           u64* __restrict__ seen_mask, int* __restrict__ cells,
                                                           int* __restrict__ seen_cells, u64* __restrict__ near_key,
                                                           int* __restrict__ source_counts, int* __restrict__ counts) {
  extern __shared__ u64 plane_s[];                                   // STAGED: ceil(N / 64) words, at most 16 KB
  __shared__ u64 near_s[SI_G * SI_K];                                // 8 KB
  __shared__ int seen_s[SI_G * SI_K];                                // 4 KB
  __shared__ int cells_s[SI_K], source_s[2 * SI_S], count_s[3];
  const int tid = threadIdx.x, lane = tid & 63;
  const int i = blockIdx.x * SI_WG + tid;
  if (STAGED) {
    const int words = (N + 63) >> 6;
    for (int t = tid; t < words; t += SI_WG) plane_s[t] = plane_g[t];            // at most EOD_SIGHT_LDS_CELLS / 64 / 256 = 8 rounds
  }
  for (int t = tid; t < SI_G * SI_K; t += SI_WG) {
    near_s[t] = SI_NONE;
    seen_s[t] = 0;
  }
  if (tid < SI_K) cells_s[tid] = 0;
  if (tid < 2 * SI_S) source_s[tid] = 0;
  if (tid < 3) count_s[tid] = 0;
  __syncthreads();
  const u64* plane = STAGED ? plane_s : plane_g;
  const bool live = i < N;
  const int r1 = live ? i / cols : 0, c1 = live ? i - r1 * cols : 0;
  const unsigned mine = live ? info[i] : (SI_CLEAR | SI_NOSLOT);
  const unsigned slot = mine & SI_NOSLOT;
  const int base = i - lane;                                         // this wave's 64 cells are one word: a workgroup starts on one
  const u64 opaque_w = base < N ? plane[base >> 6] : 0ull;
  u64 mask = 0ull;
  {
    const int g = blockIdx.y * SI_G;                                 // this workgroup's sources
    const int g_end = min(S, g + SI_G);
    for (int s = g; s < g_end; ++s) {                                // uniform
      const int f = src.cell[s];
      if (f < 0) continue;                                           // an unused source
      const int r0 = f / cols, c0 = f - r0 * cols;
      const int dr = r1 - r0, dc = c1 - c0;
      const int ar = abs(dr), ac = abs(dc), n = max(ar, ac);
      const int d2 = dr * dr + dc * dc;                              // below INT_MAX
      bool seen = live && d2 <= range2;
      if (seen) {
        const int sr = dr < 0 ? -cols : cols, sc = dc < 0 ? -1 : 1;
        const int two_n = 2 * n, two_ar = 2 * ar, two_ac = 2 * ac;
        int er = n, ec = n, cell = f;
        for (int k = 1; k <= n; ++k) {                               // at most max(rows, cols) - 1 steps
          er += two_ar;
          ec += two_ac;
          const bool row_step = er >= two_n, col_step = ec >= two_n;
          int next = cell;
          if (row_step) {
            er -= two_n;
            next += sr;
          }
          if (col_step) {
            ec -= two_n;
            next += sc;
          }
          if (row_step && col_step && sight_opaque(plane, cell + sr) && sight_opaque(plane, cell + sc)) {
            seen = false;                                            // between two opaque cells that touch at a corner
            break;
          }
          if (k < n && sight_opaque(plane, next)) {               // the target itself may be opaque
            seen = false;
            break;
          }
          cell = next;
        }
      }
      if (seen) {
        mask |= 1ull << s;
        if (slot != SI_NOSLOT) {
          const int p = (s - g) * SI_K + (int)slot;
          atomicAdd(&seen_s[p], 1);
          atomicMin(&near_s[p], ((u64)(unsigned)d2 << 32) | (unsigned)i);
        }
      }
      const u64 b = __ballot(seen);
      if (lane == 0 && b) {
        const int clear = __popcll(b & ~opaque_w), solid = __popcll(b & opaque_w);
        if (clear) atomicAdd(&source_s[2 * s], clear);
        if (solid) atomicAdd(&source_s[2 * s + 1], solid);
      }
    }
    __syncthreads();
    for (int t = tid; t < SI_G * SI_K; t += SI_WG) {                 // only what this workgroup met
      const int s = g + t / SI_K, k = t % SI_K;
      if (seen_s[t] > 0) {
        atomicAdd(&seen_cells[s * K + k], seen_s[t]);
        atomicMin(&near_key[s * K + k], near_s[t]);
      }
    }
    __syncthreads();
  }
  const bool alone = gridDim.y == 1, first = blockIdx.y == 0;
  if (live) {
    if (alone) seen_mask[i] = mask;
    else if (mask != 0ull) atomicOr(&seen_mask[i], mask);
    if (first && slot != SI_NOSLOT) atomicAdd(&cells_s[slot], 1);
  }
  const u64 any = __ballot(alone && live && mask != 0ull), in = __ballot(live);
  if (lane == 0 && in && first) {
    const int solid = __popcll(opaque_w);                            // the bit plane's own count: its tail bits are 0
    if (solid) atomicAdd(&count_s[0], solid);
    if (__popcll(in) - __popcll(opaque_w & in)) atomicAdd(&count_s[1], __popcll(in) - __popcll(opaque_w & in));
    if (any) atomicAdd(&count_s[2], __popcll(any));
  }
  __syncthreads();
  if (tid < SI_K && cells_s[tid] > 0) atomicAdd(&cells[tid], cells_s[tid]);
  if (tid < 2 * S && source_s[tid] > 0) atomicAdd(&source_counts[tid], source_s[tid]);
  if (tid < 3 && count_s[tid] > 0) atomicAdd(&counts[tid], count_s[tid]);
}

__global__ __launch_bounds__(256) void sight_finish_kernel(const SightSources src, const int* __restrict__ seen_cells,
                                                           const u64* __restrict__ near_key, const u64* __restrict__ seen_mask, int N, int K, int S,
                                                           int* __restrict__ counts, int* __restrict__ near_d2,
                                                           int* __restrict__ near_cell, u64* __restrict__ best_key,
                                                           int* __restrict__ best_seen, int* __restrict__ best_source) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (S > SI_G) {                                                    // the walk's source groups could not count the cells anyone sees
    __shared__ int any_s;                                            // S is uniform over the grid: every thread comes here or none
    if (threadIdx.x == 0) any_s = 0;
    __syncthreads();
    const u64 any = __ballot(t < N && seen_mask[t] != 0ull);
    if ((threadIdx.x & 63) == 0 && any) atomicAdd(&any_s, __popcll(any));
    __syncthreads();
    if (threadIdx.x == 0 && any_s > 0) atomicAdd(&counts[2], any_s);  // one global atomic per workgroup that met a seen cell
  }
  if (t < S * K) {
    const u64 key = near_key[t];
    near_d2[t] = key == SI_NONE ? INT_MAX : (int)(unsigned)(key >> 32);
    near_cell[t] = key == SI_NONE ? -1 : (int)(unsigned)key;
  }
  if (t < K) {
    u64 best = 0ull;
    for (int s = 0; s < S; ++s) {                                    // at most 64
      const int seen = seen_cells[s * K + t];
      if (src.cell[s] >= 0 && seen > 0) best = max(best, ((u64)(unsigned)seen << 32) | (unsigned)~(unsigned)s);
    }
    best_key[t] = best;
    best_seen[t] = (int)(unsigned)(best >> 32);
    best_source[t] = best == 0ull ? -1 : (int)~(unsigned)best;
  }
}

inline bool sight_dims_ok(int N, int cols) {
  return N >= 1 && N <= EOD_SIGHT_N_MAX && cols >= 1 && N % cols == 0 && cols <= EOD_SIGHT_DIM_MAX && N / cols <= EOD_SIGHT_DIM_MAX;
}

inline bool sight_aligned(const void* p, unsigned a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1u)) == 0; }

}  // namespace

extern "C" size_t eod_map_sight_workspace_bytes(int N, int cols) {
  if (!sight_dims_ok(N, cols)) return 0;
  return sight_up256((size_t)N) + sight_up256((size_t)sight_words(N) * 8);
}

extern "C" int eod_map_sight(const int32_t* object_labels, const int32_t* objects, const int32_t* passable, const int32_t* from_cells,
                             int N, int K, int P, int S, int cols, int range2, uint64_t* seen_mask, int32_t* cells,
                             int32_t* seen_cells, uint64_t* near_key, int32_t* near_d2, int32_t* near_cell, uint64_t* best_key,
                             int32_t* best_seen, int32_t* best_source, int32_t* source_counts, int32_t* counts, int32_t* status,
                             void* workspace, size_t workspace_bytes, eod_stream_t stream) {
  if (!sight_dims_ok(N, cols) || K < 1 || K > EOD_SIGHT_K_MAX || P < 0 || P > EOD_SIGHT_P_MAX || S < 1 || S > EOD_SIGHT_S_MAX ||
      range2 < 0)
    return EOD_ERR_BAD_DIMS;
  SightSources src;
  for (int s = 0; s < SI_S; ++s) src.cell[s] = -1;
  if (from_cells) {
    std::memcpy(src.cell, from_cells, sizeof(int32_t) * (size_t)S);  // host memory, of any alignment: that is judged below
    for (int s = 0; s < S; ++s)
      if (src.cell[s] >= N) return EOD_ERR_BAD_DIMS;
  }
  if (!object_labels || !objects || (P > 0 && !passable) || !from_cells || !seen_mask || !cells || !seen_cells || !near_key ||
      !near_d2 || !near_cell || !best_key || !best_seen || !best_source || !source_counts || !counts || !status || !workspace)
    return EOD_ERR_NULL;
  if (!sight_aligned(object_labels, 4) || !sight_aligned(objects, 4) || !sight_aligned(passable, 4) || !sight_aligned(from_cells, 4) ||
      !sight_aligned(seen_mask, 8) || !sight_aligned(cells, 4) || !sight_aligned(seen_cells, 4) || !sight_aligned(near_key, 8) ||
      !sight_aligned(near_d2, 4) || !sight_aligned(near_cell, 4) || !sight_aligned(best_key, 8) || !sight_aligned(best_seen, 4) ||
      !sight_aligned(best_source, 4) || !sight_aligned(source_counts, 4) || !sight_aligned(counts, 4) || !sight_aligned(status, 4) ||
      !sight_aligned(workspace, 8))
    return EOD_ERR_ALIGN;
  if (workspace_bytes < eod_map_sight_workspace_bytes(N, cols)) return EOD_ERR_CAPACITY;
  hipStream_t st = (hipStream_t)stream;
  unsigned char* info = static_cast<unsigned char*>(workspace);
  u64* plane = reinterpret_cast<u64*>(info + sight_up256((size_t)N));
  u64* sm = reinterpret_cast<u64*>(seen_mask);
  u64* nk = reinterpret_cast<u64*>(near_key);
  u64* bk = reinterpret_cast<u64*>(best_key);
  const int most = N > S * K ? N : S * K;                            // the first workgroup's 256 threads cover K, 2 * S and the counts
  hipLaunchKernelGGL(sight_init_kernel, dim3((most + 255) / 256), dim3(256), 0, st, (const int*)object_labels, (const int*)objects,
                     (const int*)passable, N, K, P, S, info, plane, sm, (int*)cells, (int*)seen_cells, nk, (int*)source_counts,
                     (int*)counts, (int*)status);
  const dim3 grid((N + SI_WG - 1) / SI_WG, (S + SI_G - 1) / SI_G);
  if (N <= EOD_SIGHT_LDS_CELLS)
    hipLaunchKernelGGL(sight_walk_kernel<true>, grid, dim3(SI_WG), (size_t)sight_words(N) * 8, st, (const unsigned char*)info,
                       (const u64*)plane, src, N, K, S, cols, range2, sm, (int*)cells, (int*)seen_cells, nk, (int*)source_counts,
                       (int*)counts);
  else
    hipLaunchKernelGGL(sight_walk_kernel<false>, grid, dim3(SI_WG), 0, st, (const unsigned char*)info, (const u64*)plane, src, N, K,
                       S, cols, range2, sm, (int*)cells, (int*)seen_cells, nk, (int*)source_counts, (int*)counts);
  hipLaunchKernelGGL(sight_finish_kernel, dim3(((S > SI_G && N > S * K ? N : S * K) + 255) / 256), dim3(256), 0, st, src, (const int*)seen_cells,
                     (const u64*)nk, (const u64*)sm, N, K, S, (int*)counts,
                     (int*)near_d2, (int*)near_cell, bk, (int*)best_seen, (int*)best_source);
  return eod_launch_status();
}
