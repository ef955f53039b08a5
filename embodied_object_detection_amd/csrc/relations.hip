// Object relations (eod_map_relations; semantics in include/eod_relations.h): for up to 64 objects of a label map all pairwise
// relations within a radius (closest approach, the cell of it, cells within reach, shared border) and each object's distance from
// one given cell.  A read-only query beside the frame.  Three kernels; what one needs of another is complete at the launch boundary
// between them, and no workgroup ever waits for another one.
//
//   relations_init_kernel    pair_key and from_key to all ones, near_cells, edges and cells to 0: the buffers may hold anything.
//   relations_pair_kernel    the hot path.  A workgroup of four waves owns a tile of RL_TR x RL_TC = 32 x 32 cells, a thread four of
//                            them.  SLOTS: the slot of every cell of the tile goes to LDS as one byte (255: no slot, or no cell
//                            there), found as describe_pool_kernel finds it: lane l holds objects[l], the wave compares a cell's
//                            label with all 64 at once, and a ballot and a find-first give the lowest slot.  A tile without a slot
//                            cell of its own returns here: on a real map that is nearly every tile, and it has read 4 KiB of
//                            labels and touched no table.  The others stage the halo of R cells around the tile the same way (cells
//                            outside the grid: 255, so a row's end never meets the next row's start) and gather the 64-bit set of
//                            the slots present in tile and halo.  A tile with fewer than two slots there (the inside of a large
//                            object) has no pair: it clears no table and walks nothing.  The others clear the tables.
//                            PAIRS: every slot cell walks the offsets of the disc in ascending d2 (relations_disc: 796 offsets for
//                            R = 16, built at compile time, a prefix of it for a smaller R, copied to LDS first; the 32 LDS bytes
//                            of a step of eight offsets are in flight together) and keeps a 64-bit mask of the slots it has seen.
//                            The first hit of a slot b is this cell's minimum for b: one LDS atomicMin of (d2 << 10) | the cell's
//                            index in the tile into key_s[a][b] (32 bits: d2 <= 256, 1024 cells, and the index orders the tile's
//                            cells as their cell numbers do) and one add to the cell count: at most 63 of each per cell, whatever
//                            R.  The four d2 == 1 offsets come first and add the shared border.  A cell that has seen every slot
//                            present is done; a wave stops when all its cells are, and a wave without a slot cell walks nothing.
//                            The cell counts share a word, near_cells in the lower half (at most 1024 in a tile), edges in the
//                            upper (at most 4096): 32 KiB of tables instead of 64, four workgroups per CU.  FLUSH: only the
//                            entries the tile set go out, the key widened to (d2 << 32) | cell, with one global 64-bit atomicMin
//                            and one or two 32-bit atomicAdd each; then the slots' cell counts and from keys.
//   relations_finish_kernel  one wave per slot a: lane b unpacks pair_key[a][b]; topn rounds of a wave minimum over
//                            (min_d2 << 32) | b rank the neighbours; lane 0 unpacks from_key[a].
//
// THE INVARIANT: a cell pair (i in a, j in b) within reach is seen by the tile that owns i, whatever tile owns j (the halo is R
// cells wide and d2 <= R^2 implies |dr|, |dc| <= R), and by no other tile.  Per cell and slot b the walk reports the smallest d2 once
// (ascending order, the seen mask); minimum and sum over the cells of a are integer atomics, so no output depends on which tile,
// wave or lane holds a cell or on the order of the flushes.
// BOUNDS: labels are read at r * cols + c with 0 <= r < rows, 0 <= c < cols only; slot_s is indexed by (tr + R + dr) * SW + tc + R + dc
// with |dr|, |dc| <= R <= 16, inside (32 + 2R)^2 <= 4096 bytes; a slot is < 64 by construction (a bit of a ballot) and < K because
// objects[l] is -1 from lane K on, so a * K + b stays inside the [K, K] tables.  Every loop has a compile-time bound.
#include "eod_common.h"
#include "../../include/eod_relations.h"
#include <climits>

namespace {

typedef unsigned long long u64;

constexpr int RL_TR = 32, RL_TC = 32, RL_THREADS = 256, RL_PER = RL_TR * RL_TC / RL_THREADS;
constexpr int RL_RMAX = EOD_RELATIONS_RADIUS_MAX, RL_STAGE = (RL_TR + 2 * RL_RMAX) * (RL_TC + 2 * RL_RMAX);
constexpr int RL_K = EOD_RELATIONS_K_MAX, RL_DISC_N = 796;           // the lattice points with 0 < dr^2 + dc^2 <= 16^2
constexpr int RL_STEP = 8, RL_DISC_PAD = (RL_DISC_N + RL_STEP - 1) / RL_STEP * RL_STEP;      // offsets per step of the walk; zeros behind the table
constexpr unsigned RL_NOSLOT = 255u;
constexpr u64 RL_NONE = ~0ull;
constexpr unsigned RL_NOKEY = ~0u;
static_assert(RL_K == 64, "one wave looks a label up; the seen mask is one 64-bit word");
static_assert(RL_TC == 32 && RL_PER == 4 && RL_STAGE % RL_THREADS == 0, "the cell <-> thread mapping of the pair kernel");
static_assert(RL_TR * RL_TC == 1024 && RL_RMAX * RL_RMAX < (1 << 22), "a tile's key: d2 above the ten bits of the cell's index in the tile");
static_assert(RL_TR * RL_TC < 65536 && 4 * RL_TR * RL_TC < 65536, "near_cells and edges of one tile share a 32-bit word");

// the offsets of the disc in ascending d2: (d2 << 12) | (dr + 16) << 6 | (dc + 16); upto[R]: how many have d2 <= R * R
struct RelationsDisc {
  int upto[RL_RMAX + 1];
  int e[RL_DISC_PAD];
};

constexpr RelationsDisc relations_make_disc() {
  RelationsDisc d{};
  int root[RL_RMAX * RL_RMAX + 1] = {};
  for (int v = 0; v <= RL_RMAX * RL_RMAX; ++v) root[v] = -1;
  for (int c = 0; c <= RL_RMAX; ++c) root[c * c] = c;
  int n = 0;
  for (int d2 = 1; d2 <= RL_RMAX * RL_RMAX; ++d2) {
    for (int dr = -RL_RMAX; dr <= RL_RMAX; ++dr) {
      const int rem = d2 - dr * dr;
      if (rem < 0 || root[rem] < 0) continue;
      const int c = root[rem];
      d.e[n++] = (d2 << 12) | ((dr + 16) << 6) | (16 - c);
      if (c > 0) d.e[n++] = (d2 << 12) | ((dr + 16) << 6) | (16 + c);
    }
    if (root[d2] >= 0) d.upto[root[d2]] = n;
  }
  return d;
}

constexpr RelationsDisc RL_DISC = relations_make_disc();
static_assert(RL_DISC.upto[1] == 4 && RL_DISC.upto[RL_RMAX] == RL_DISC_N, "the four d2 == 1 offsets come first; the table is full");
__constant__ RelationsDisc relations_disc = RL_DISC;

__global__ __launch_bounds__(256) void relations_init_kernel(int K, u64* __restrict__ pair_key, int* __restrict__ near_cells,
                                                             int* __restrict__ edges, int* __restrict__ cells, u64* __restrict__ from_key) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < K * K) {
    pair_key[i] = RL_NONE;
    near_cells[i] = 0;
    edges[i] = 0;
  }
  if (i < K) {
    cells[i] = 0;
    from_key[i] = RL_NONE;
  }
}

// the slot of each lane's label (RL_NOSLOT: none), for all 64 lanes of the wave; every lane of the wave calls it
__device__ __forceinline__ unsigned relations_slot(int lab, int obj, int lane) {
  unsigned slot = RL_NOSLOT;
  u64 todo = __ballot(lab >= 0);
  for (int n = 0; n < 64 && todo; ++n) {                             // wave-uniform
    const int j = __ffsll((long long)todo) - 1;
    todo &= todo - 1;
    const int l = __shfl(lab, j, 64);
    const u64 hit = __ballot(obj >= 0 && obj == l);
    if (lane == j && hit) slot = (unsigned)(__ffsll((long long)hit) - 1);      // the lowest slot wins a duplicate
  }
  return slot;
}

__device__ __forceinline__ u64 relations_wave_or_u64(u64 v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const unsigned lo = __shfl_xor((unsigned)v, off, 64), hi = __shfl_xor((unsigned)(v >> 32), off, 64);
    v |= ((u64)hi << 32) | lo;
  }
  return v;
}

__global__ __launch_bounds__(RL_THREADS) void relations_pair_kernel(const int* __restrict__ labels, const int* __restrict__ objects,
                                                                    int rows, int cols, int K, int R, int n_off, int tiles_x,
                                                                    int from_cell, u64* __restrict__ pair_key,
                                                                    int* __restrict__ near_cells, int* __restrict__ edges,
                                                                    int* __restrict__ cells, u64* __restrict__ from_key) {
  __shared__ unsigned key_s[RL_K * RL_K];                            // 16 KiB: (d2 << 10) | the cell's index in the tile
  __shared__ unsigned cnt_s[RL_K * RL_K];                            // 16 KiB: near_cells | edges << 16
  __shared__ int disc_s[RL_DISC_PAD];                                // 3 KiB: the offsets of this radius
  __shared__ u64 from_s[RL_K];
  __shared__ int cells_s[RL_K];
  __shared__ unsigned char slot_s[RL_STAGE];                         // 4 KiB
  __shared__ u64 present_s;                                          // the slots of the tile and its halo
  __shared__ int any_s;
  const int tid = threadIdx.x, lane = tid & 63;
  const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
  const int r0 = ty * RL_TR, c0 = tx * RL_TC;
  const int SW = RL_TC + 2 * R, total = (RL_TR + 2 * R) * SW;
  const int obj = lane < K ? objects[lane] : -1;
  if (tid == 0) {
    any_s = 0;
    present_s = 0ull;
  }
  __syncthreads();
  // the tile's own cells
  unsigned a[RL_PER];
  bool mine = false;
  u64 present = 0ull;
#pragma unroll
  for (int j = 0; j < RL_PER; ++j) {
    const int t = j * RL_THREADS + tid, tr = t >> 5, tc = t & 31;
    const int r = r0 + tr, c = c0 + tc;
    const int lab = (r < rows && c < cols) ? labels[r * cols + c] : -1;
    a[j] = relations_slot(lab, obj, lane);
    slot_s[(tr + R) * SW + tc + R] = (unsigned char)a[j];
    mine |= a[j] != RL_NOSLOT;
    if (a[j] != RL_NOSLOT) present |= 1ull << a[j];
  }
  const bool wave_mine = __ballot(mine) != 0;
  if (wave_mine && lane == 0) any_s = 1;
  __syncthreads();
  if (!any_s) return;                                                // no slot cell in this tile: no table is touched
  // the halo
  for (int base = 0; base < RL_STAGE; base += RL_THREADS) {
    if (base >= total) break;                                        // uniform over the workgroup
    const int s = base + tid, sr = s / SW, sc = s - sr * SW;
    const bool halo = s < total && !(sr >= R && sr < R + RL_TR && sc >= R && sc < R + RL_TC);
    const int r = r0 - R + sr, c = c0 - R + sc;
    const int lab = (halo && r >= 0 && r < rows && c >= 0 && c < cols) ? labels[r * cols + c] : -1;
    const unsigned slot = relations_slot(lab, obj, lane);
    if (halo) slot_s[s] = (unsigned char)slot;
    if (slot != RL_NOSLOT) present |= 1ull << slot;
  }
  present = relations_wave_or_u64(present);
  if (lane == 0 && present) atomicOr(&present_s, present);
  if (tid < RL_K) {
    from_s[tid] = RL_NONE;
    cells_s[tid] = 0;
  }
  __syncthreads();
  present = present_s;
  const bool pairs = (present & (present - 1)) != 0;                 // two slots or more within the tile and its halo; uniform
  if (pairs) {                                                       // a tile deep inside one object has no pair: no table, no walk
    for (int i = tid; i < RL_K * RL_K; i += RL_THREADS) {
      key_s[i] = RL_NOKEY;
      cnt_s[i] = 0u;
    }
    for (int i = tid; i < RL_DISC_PAD; i += RL_THREADS)              // every load in flight at once; zeros behind the table
      if (i < ((n_off + RL_STEP - 1) & -RL_STEP)) disc_s[i] = relations_disc.e[i];
    __syncthreads();
  }
  if (wave_mine) {
    u64 seen[RL_PER];
    int cell[RL_PER], pos[RL_PER];
    const int fr = from_cell >= 0 ? from_cell / cols : 0, fc = from_cell >= 0 ? from_cell - fr * cols : 0;
#pragma unroll
    for (int j = 0; j < RL_PER; ++j) {
      const int t = j * RL_THREADS + tid, tr = t >> 5, tc = t & 31;
      seen[j] = 0ull;
      cell[j] = (r0 + tr) * cols + c0 + tc;
      pos[j] = (tr + R) * SW + tc + R;
      if (a[j] != RL_NOSLOT) {
        seen[j] = 1ull << a[j];                                      // its own slot is no neighbour
        atomicAdd(&cells_s[a[j]], 1);
        if (from_cell >= 0) {
          const int dr = r0 + tr - fr, dc = c0 + tc - fc;
          const unsigned d2 = (unsigned)(dr * dr) + (unsigned)(dc * dc);        // < 2^31: rows, cols <= 32767
          atomicMin(&from_s[a[j]], ((u64)d2 << 32) | (unsigned)cell[j]);
        }
      }
    }
    // RL_STEP offsets at a time: every LDS byte of the step is in flight before the first is used.  An offset past n_off counts as
    // (0, 0), the cell itself, which is no neighbour.
    for (int k0 = 0; k0 < RL_DISC_N; k0 += RL_STEP) {
      if (k0 >= n_off || !pairs) break;                              // uniform
      bool open = false;                                             // a cell is done when it has seen every slot there is
#pragma unroll
      for (int j = 0; j < RL_PER; ++j) open |= a[j] != RL_NOSLOT && (present & ~seen[j]) != 0;
      if (!__ballot(open)) break;                                    // wave-uniform
      int off[RL_STEP];
      unsigned b[RL_PER][RL_STEP];
#pragma unroll
      for (int i = 0; i < RL_STEP; ++i) {
        const int e = disc_s[k0 + i];
        off[i] = k0 + i < n_off ? (((e >> 6) & 63) - 16) * SW + (e & 63) - 16 : 0;
      }
#pragma unroll
      for (int j = 0; j < RL_PER; ++j)
#pragma unroll
        for (int i = 0; i < RL_STEP; ++i) b[j][i] = slot_s[pos[j] + off[i]];
#pragma unroll
      for (int i = 0; i < RL_STEP; ++i) {
        const unsigned d2 = (unsigned)disc_s[k0 + i] >> 12;
        const unsigned border = k0 + i < 4 ? 0x10000u : 0u;          // d2 == 1: one cell pair of the shared border
#pragma unroll
        for (int j = 0; j < RL_PER; ++j) {
          const unsigned bb = b[j][i];
          if (bb == a[j] || bb == RL_NOSLOT || a[j] == RL_NOSLOT) continue;      // its own slot is no neighbour
          const u64 bit = 1ull << bb;
          unsigned add = border;
          if (!(seen[j] & bit)) {                                    // the first hit of b in ascending d2: this cell's minimum for b
            seen[j] |= bit;
            add += 1u;
            atomicMin(&key_s[a[j] * RL_K + bb], (d2 << 10) | (unsigned)(j * RL_THREADS + tid));
          }
          if (add) atomicAdd(&cnt_s[a[j] * RL_K + bb], add);
        }
      }
    }
  }
  __syncthreads();
  // only what this tile set; the cell of a key from its index in the tile (their orders agree)
  for (int i = tid; i < RL_K * RL_K; i += RL_THREADS) {
    if (!pairs) break;                                               // uniform
    const unsigned key = key_s[i];
    if (key == RL_NOKEY) continue;                                   // an edge is a first hit too: no count without a key
    const int g = (i >> 6) * K + (i & 63);
    const unsigned cnt = cnt_s[i], t = key & 1023u;
    const unsigned cell = (unsigned)((r0 + (int)(t >> 5)) * cols + c0 + (int)(t & 31u));
    atomicMin(&pair_key[g], ((u64)(key >> 10) << 32) | cell);
    atomicAdd(&near_cells[g], (int)(cnt & 0xffffu));
    if (cnt >> 16) atomicAdd(&edges[g], (int)(cnt >> 16));
  }
  if (tid < RL_K && cells_s[tid] > 0) {
    atomicAdd(&cells[tid], cells_s[tid]);
    if (from_s[tid] != RL_NONE) atomicMin(&from_key[tid], from_s[tid]);
  }
}

__device__ __forceinline__ u64 relations_wave_min_u64(u64 v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const unsigned lo = __shfl_xor((unsigned)v, off, 64), hi = __shfl_xor((unsigned)(v >> 32), off, 64);
    const u64 o = ((u64)hi << 32) | lo;
    v = o < v ? o : v;
  }
  return v;
}

__global__ __launch_bounds__(64) void relations_finish_kernel(const u64* __restrict__ pair_key, const u64* __restrict__ from_key, int K,
                                                              int topn, int* __restrict__ min_d2, int* __restrict__ closest,
                                                              int* __restrict__ nearest, int* __restrict__ nearest_d2,
                                                              int* __restrict__ from_d2, int* __restrict__ from_closest) {
  const int a = blockIdx.x, b = threadIdx.x;
  const u64 key = b < K ? pair_key[a * K + b] : RL_NONE;
  if (b < K) {
    min_d2[a * K + b] = key == RL_NONE ? INT_MAX : (int)(key >> 32);
    closest[a * K + b] = key == RL_NONE ? -1 : (int)(unsigned)key;
  }
  u64 cand = key == RL_NONE ? RL_NONE : ((key >> 32) << 32) | (unsigned)b;       // min_d2 ascending, then the slot ascending
  for (int r = 0; r < EOD_RELATIONS_TOPN_MAX; ++r) {
    if (r >= topn) break;
    const u64 best = relations_wave_min_u64(cand);
    if (cand == best) cand = RL_NONE;
    if (b == 0) {
      nearest[a * topn + r] = best == RL_NONE ? -1 : (int)(unsigned)best;
      nearest_d2[a * topn + r] = best == RL_NONE ? INT_MAX : (int)(best >> 32);
    }
  }
  if (b == 0) {
    const u64 fk = from_key[a];
    from_d2[a] = fk == RL_NONE ? INT_MAX : (int)(fk >> 32);
    from_closest[a] = fk == RL_NONE ? -1 : (int)(unsigned)fk;
  }
}

inline bool relations_aligned(const void* p, unsigned a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1u)) == 0; }

}  // namespace

extern "C" int eod_map_relations(const int32_t* object_labels, const int32_t* objects, int N, int K, int cols, int radius, int from_cell,
                                 int topn, uint64_t* pair_key, int32_t* min_d2, int32_t* closest, int32_t* near_cells, int32_t* edges,
                                 int32_t* cells, int32_t* nearest, int32_t* nearest_d2, uint64_t* from_key, int32_t* from_d2,
                                 int32_t* from_closest, eod_stream_t stream) {
  if (K < 1 || K > EOD_RELATIONS_K_MAX || N < 1 || N > EOD_RELATIONS_N_MAX || cols < 1 || N % cols != 0 ||
      cols > EOD_RELATIONS_DIM_MAX || N / cols > EOD_RELATIONS_DIM_MAX || radius < 1 || radius > EOD_RELATIONS_RADIUS_MAX || topn < 1 ||
      topn > EOD_RELATIONS_TOPN_MAX || from_cell < -1 || from_cell >= N)
    return EOD_ERR_BAD_DIMS;
  if (!object_labels || !objects || !pair_key || !min_d2 || !closest || !near_cells || !edges || !cells || !nearest || !nearest_d2 ||
      !from_key || !from_d2 || !from_closest)
    return EOD_ERR_NULL;
  if (!relations_aligned(object_labels, 4) || !relations_aligned(objects, 4) || !relations_aligned(pair_key, 8) ||
      !relations_aligned(min_d2, 4) || !relations_aligned(closest, 4) || !relations_aligned(near_cells, 4) ||
      !relations_aligned(edges, 4) || !relations_aligned(cells, 4) || !relations_aligned(nearest, 4) ||
      !relations_aligned(nearest_d2, 4) || !relations_aligned(from_key, 8) || !relations_aligned(from_d2, 4) ||
      !relations_aligned(from_closest, 4))
    return EOD_ERR_ALIGN;
  hipStream_t s = (hipStream_t)stream;
  const int rows = N / cols, tiles_x = (cols + RL_TC - 1) / RL_TC, tiles_y = (rows + RL_TR - 1) / RL_TR;
  u64* pk = reinterpret_cast<u64*>(pair_key);
  u64* fk = reinterpret_cast<u64*>(from_key);
  hipLaunchKernelGGL(relations_init_kernel, dim3((K * K + 255) / 256), dim3(256), 0, s, K, pk, (int*)near_cells, (int*)edges, (int*)cells,
                     fk);
  hipLaunchKernelGGL(relations_pair_kernel, dim3(tiles_x * tiles_y), dim3(RL_THREADS), 0, s, (const int*)object_labels,
                     (const int*)objects, rows, cols, K, radius, RL_DISC.upto[radius], tiles_x, from_cell, pk, (int*)near_cells,
                     (int*)edges, (int*)cells, fk);
  hipLaunchKernelGGL(relations_finish_kernel, dim3(K), dim3(64), 0, s, (const u64*)pk, (const u64*)fk, K, topn, (int*)min_d2,
                     (int*)closest, (int*)nearest, (int*)nearest_d2, (int*)from_d2, (int*)from_closest);
  return eod_launch_status();
}
