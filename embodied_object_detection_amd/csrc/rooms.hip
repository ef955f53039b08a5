// Rooms on the map (eod_map_rooms; semantics in include/eod_rooms.h): the free space of a label map split at its doorways, and the
// objects sorted by room.  A read-only query beside the frame: integers and comparisons only, integer atomics only, the result a
// pure function of the inputs.  Twelve launches and `sweeps` of the sweep kernel; what one needs of another is complete at the launch
// boundary between them, and no workgroup ever waits for another one (no spin, no flag, no grid barrier).  The core regions are the
// union-find of regions.hip on one plane, the CORE cells, 4-connected (the unknown plane of frontier.hip); the grow is the tile
// relaxation of route.hip on 64-bit keys.
//
//   rooms_classify_kernel   one thread per cell: its kind (BLOCKED, VOID, FREE, CORE) and its object slot, one byte each to the
//                           workspace.  Lane l holds objects[l] and passable[l], the wave compares a cell's label with all of them at
//                           once (route_init_kernel's ballot).  count, counts, status, the raw words to 0; every tile's flag set.
//   rooms_tile_kernel       regions_tile_kernel per 32 x 32 tile: the CORE cells of the tile joined in LDS, left and up only
//   rooms_border_kernel     regions_border_kernel: left and up across the tile borders
//   regions_compress_kernel (regions_common.h)
//   regions_flatten_kernel  (regions_common.h) the core regions' labels (kept in room_labels until the second flatten) and areas
//   regions_list_kernel     (regions_common.h) the regions with area >= min_cells, the ROOMS: count[0] and the list, in parent
//   rooms_seed_kernel       one thread per cell: the key (0 << 32) | label on a room's core, all ones elsewhere; counts[3]
//   rooms_sweep_kernel      the hot path, queued `sweeps` times: route_sweep_kernel on the keys.  A key is one 64-bit word, read and
//                           written whole (relaxed atomic loads and stores, in LDS and in memory), so a neighbour tile's cell read
//                           while that tile stores is either its old or its new key, never the g of one and the room of the other.
//                           Two int32 planes need an order on the two stores and the two loads there instead.
//   rooms_assign_kernel     one thread per cell: grow_dist, the room of the cell as a parent entry for the second flatten, the
//                           kinds, the grown and the unassigned cells counted; status[0] bit 0 from the last sweep's flags
//   regions_flatten_kernel  (regions_common.h) room_labels and the rooms' areas, core and grown: a room's label cell is a cell of
//                           its own core, whose key never changes, so a cell's entry is its root at one hop
//   rooms_select_kernel     one workgroup: K rounds of a workgroup-wide maximum of (area << 32) | ~label over the list, below the
//                           previous pick, each leaving slot[root] = k and the slot's outputs at their neutral values; the K x K and
//                           K_obj x K tables to 0
//   rooms_stats_kernel      every cell of a ranked room: bbox, sum_rc and widest_key per slot in LDS first, then one global atomic per
//                           slot the workgroup touched; the doorway pairs (a, b) and the object pairs (k, s) it meets in an LDS
//                           table keyed by the pair (regions_flatten_kernel's open addressing), committed once per entry
//   rooms_finish_kernel     one workgroup: the halves of widest_key and door_key, obj_room, obj_room_label, room_objects; status[0]
//                           bit 1
//
// THE INVARIANT of regions.hip carries over to the core regions word for word.  That of route.hip carries over to the keys: every
// value ever stored in key[i] is all ones or (g << 32) | room for a real path of cost g from a cell of room's core to i, and values
// only fall; the fixed point is the componentwise-lexicographic minimum, which is what the header defines.
// BOUNDS: every per-cell array is indexed by i < N or by a neighbour of i that the row and column tests keep inside the grid; the
// LDS stage by (tr + 1 + dr) * RM_SW + tc + 1 + dc with 0 <= tr < RM_TR, 0 <= tc < RM_TC, |dr|, |dc| <= 1; a tile's flags by
// y * tiles_x + x inside the tile grid; a label is a cell whose key is (0 << 32) | itself; a room slot is < K, an object slot is a
// bit of a 64-bit mask and < K_obj because objects[l] counts as -1 from lane K_obj on; a table entry is h < RM_PAIRS and its key
// (a << 6) | b or RM_OBJ + ((k << 6) | s) with all four below 64.  Every loop has a compile-time bound.
// THE ROUNDS of the in-tile relaxation: a cell is final after as many rounds as its cheapest path from the halo or from a seed
// has moves inside the tile, and one more round sees that nothing falls.  A cheapest path never visits all four cells of a
// 2 x 2 block: any two of them are one legal move apart (all four are free, so the diagonal passes the corner rule) at a cost of
// 7 at the most, and the way between the first and the last of them through the other two costs 10 at the least.  The tile is
// 256 such blocks, so the path has at most 768 cells in it and the relaxation settles within 769 rounds, below RM_ROUNDS = 1024.
// Should it ever reach the bound, the raw status says so, status[0] bit 1 is set and every output is void.
#include "regions_common.h"
#include "../../include/eod_rooms.h"

namespace {

static_assert(EOD_ROOMS_N_MAX == EOD_REGIONS_N_MAX && EOD_ROOMS_TOPK_MAX == EOD_REGIONS_TOPK_MAX, "the shared launches' limits");
static_assert(EOD_ROOMS_K_MAX == 64 && EOD_ROOMS_P_MAX == 64 && EOD_ROOMS_TOPK_MAX == 64, "one wave looks a label up; a pair is 12 bits");
static_assert(EOD_ROOMS_TILE_ROWS == EOD_REGIONS_TILE_ROWS && EOD_ROOMS_TILE_COLS == EOD_REGIONS_TILE_COLS, "one tile grid");

constexpr unsigned char RM_BLOCKED = 0, RM_VOID = 1, RM_FREE = 2, RM_CORE = 3;       // free: >= RM_FREE
constexpr unsigned RM_NOSLOT = 0xFFu;
constexpr int RM_TR = EOD_ROOMS_TILE_ROWS, RM_TC = EOD_ROOMS_TILE_COLS, RM_THREADS = 256, RM_PER = RM_TR * RM_TC / RM_THREADS;
constexpr int RM_SW = RM_TC + 2, RM_STAGE = (RM_TR + 2) * RM_SW;     // the tile and a halo of one cell
constexpr int RM_ROUNDS = RM_TR * RM_TC;                             // the bound of the in-tile relaxation
constexpr u64 RM_ORTH = 5ull << 32, RM_DIAG = 7ull << 32;            // EOD_ROUTE_COST_ORTH, EOD_ROUTE_COST_DIAG in a key's upper half
constexpr u64 RM_NONE = ~0ull;
constexpr int RM_PAIRS_LOG2 = 9, RM_PAIRS = 1 << RM_PAIRS_LOG2, RM_PROBES = 8, RM_OBJ = 4096;
static_assert(RM_PER >= 1 && RM_PER * RM_THREADS == RM_TR * RM_TC && (RM_TC & (RM_TC - 1)) == 0, "the cell <-> thread mapping of the sweep");
static_assert(7ull * EOD_ROOMS_N_MAX < (u64)INT_MAX, "a cost is never INT_MAX");

__device__ __forceinline__ u64 key_ld(const u64* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void key_st(u64* p, u64 v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ u64 lds_ld64(const u64* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
__device__ __forceinline__ void lds_st64(u64* p, u64 v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }

__global__ __launch_bounds__(256) void rooms_classify_kernel(const int* __restrict__ labels, const int* __restrict__ passable,
                                                             const int* __restrict__ d2, const unsigned char* __restrict__ known,
                                                             const int* __restrict__ objects, int N, int P, int K_obj, int door_r2,
                                                             int tiles, unsigned char* __restrict__ kind,
                                                             unsigned char* __restrict__ slotb, int* __restrict__ flags,
                                                             int* __restrict__ count, int* __restrict__ counts, int* __restrict__ status,
                                                             int* __restrict__ raw) {
  const int i = blockIdx.x * 256 + threadIdx.x, lane = threadIdx.x & 63;
  const int obj = lane < K_obj ? objects[lane] : -1;
  const bool has_pas = lane < P;
  const int pas = has_pas ? passable[lane] : 0;
  const int lab = i < N ? labels[i] : -1;
  unsigned slot = RM_NOSLOT;
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
  if (i < N) {
    const bool blocked = lab >= 0 && !pass;
    const bool is_void = !blocked && known && known[i] == 0;
    kind[i] = blocked ? RM_BLOCKED : is_void ? RM_VOID : d2[i] > door_r2 ? RM_CORE : RM_FREE;
    slotb[i] = (unsigned char)slot;
  }
  if (i < tiles) {
    flags[i] = 1;                                                    // what sweep 0 reads: a room may lie in any tile
    flags[tiles + i] = 0;                                            // what sweep 0 sets in
    flags[2 * tiles + i] = 0;
  }
  if (i < 6) counts[i] = 0;
  if (i < 4) raw[i] = 0;
  if (i < 2) status[i] = 0;
  if (i == 0) count[0] = 0;
}

__global__ __launch_bounds__(RG_THREADS) void rooms_tile_kernel(const unsigned char* __restrict__ kind, int rows, int cols, int tiles_c,
                                                                 int* __restrict__ parent, int* __restrict__ slot, int* __restrict__ area,
                                                                 int* __restrict__ status) {
  __shared__ int p_s[RG_TILE];
  const int tid = threadIdx.x;
  const int ty = blockIdx.x / tiles_c, tx = blockIdx.x - ty * tiles_c;
  const int r0 = ty * RG_TR, c0 = tx * RG_TC;
  for (int l = tid; l < RG_TILE; l += RG_THREADS) {
    const int r = r0 + l / RG_TC, c = c0 + (l & (RG_TC - 1));
    p_s[l] = r < rows && c < cols && kind[r * cols + c] == RM_CORE ? l : -1;
  }
  __syncthreads();
  for (int l = tid; l < RG_TILE; l += RG_THREADS) {
    if (lds_ld(&p_s[l]) < 0) continue;
    const int lr = l / RG_TC, lc = l & (RG_TC - 1);
    if (lc > 0 && lds_ld(&p_s[l - 1]) >= 0) tile_union(p_s, l, l - 1, status);
    if (lr > 0 && lds_ld(&p_s[l - RG_TC]) >= 0) tile_union(p_s, l, l - RG_TC, status);
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

__global__ __launch_bounds__(RG_THREADS) void rooms_border_kernel(int* __restrict__ p, int N, int cols, int* __restrict__ status) {
  const int i = blockIdx.x * RG_THREADS + threadIdx.x;
  if (i >= N) return;
  const int r = i / cols, c = i - r * cols;
  const int lr = r & (RG_TR - 1), lc = c & (RG_TC - 1);
  if (lr != 0 && lc != 0) return;                                    // both neighbours before it are in its own tile
  if (agent_ld(&p[i]) < 0) return;
  // the row and the column are the grid's: c > 0 keeps (r, 0) away from (r - 1, cols - 1)
  if (lc == 0 && c > 0 && agent_ld(&p[i - 1]) >= 0) grid_union(p, i, i - 1, status);
  if (lr == 0 && r > 0 && agent_ld(&p[i - cols]) >= 0) grid_union(p, i, i - cols, status);
}

__global__ __launch_bounds__(256) void rooms_seed_kernel(const unsigned char* __restrict__ kind, const int* __restrict__ core_labels,
                                                         const int* __restrict__ core_area, int N, int min_cells, u64* __restrict__ key,
                                                         int* __restrict__ counts) {
  __shared__ int n_s;
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (threadIdx.x == 0) n_s = 0;
  __syncthreads();
  bool seed = false;
  if (i < N) {
    const int lab = kind[i] == RM_CORE ? core_labels[i] : -1;
    seed = lab >= 0 && core_area[lab] >= min_cells;
    key[i] = seed ? (u64)(unsigned)lab : RM_NONE;
  }
  const u64 m = __ballot(seed);
  if ((threadIdx.x & 63) == 0 && m) atomicAdd(&n_s, __popcll(m));
  __syncthreads();
  if (threadIdx.x == 0 && n_s > 0) atomicAdd(&counts[3], n_s);
}

// the moves that may enter a free cell, from the free bits f[dr + 1][dc + 1] of its 3 x 3 neighbourhood (route_moves of route.hip)
__device__ __forceinline__ unsigned rooms_moves(const bool f[3][3]) {
  unsigned m = 0;
  if (f[0][1]) m |= 1u << 1;
  if (f[1][0]) m |= 1u << 3;
  if (f[1][2]) m |= 1u << 4;
  if (f[2][1]) m |= 1u << 6;
  if (f[0][0] && f[0][1] && f[1][0]) m |= 1u << 0;
  if (f[0][2] && f[0][1] && f[1][2]) m |= 1u << 2;
  if (f[2][0] && f[2][1] && f[1][0]) m |= 1u << 5;
  if (f[2][2] && f[2][1] && f[1][2]) m |= 1u << 7;
  return m;
}

// a neighbour's key after a move of cost w (in a key's upper half); all ones gives all ones
__device__ __forceinline__ u64 rooms_via(bool may, u64 d, u64 w) { return may && d != RM_NONE ? d + w : RM_NONE; }

__global__ __launch_bounds__(RM_THREADS) void rooms_sweep_kernel(const unsigned char* __restrict__ kind, int rows, int cols, int tiles_y,
                                                                 int tiles_x, const int* __restrict__ flags_read,
                                                                 int* __restrict__ flags_set, int* __restrict__ flags_clear, u64* key,
                                                                 int* __restrict__ raw) {
  __shared__ u64 d_s[RM_STAGE];                                      // 9248 B: the keys of the tile and its halo; all ones where not free
  __shared__ unsigned char f_s[RM_STAGE];                            // 1156 B: 1 where free
  __shared__ int low_s[3];                                           // a round lowered something: round n sets low_s[n % 3]
  __shared__ int act_s;
  const int tid = threadIdx.x, lane = tid & 63;
  const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
  if (tid == 0) {
    act_s = 0;
    low_s[0] = 0;
    low_s[1] = 0;
    flags_clear[blockIdx.x] = 0;
  }
  __syncthreads();
  if (tid < 9) {
    const int y = ty + tid / 3 - 1, x = tx + tid % 3 - 1;
    if (y >= 0 && y < tiles_y && x >= 0 && x < tiles_x && flags_read[y * tiles_x + x] != 0) act_s = 1;
  }
  __syncthreads();
  if (!act_s) return;                                                // nothing changed around this tile in the last sweep
  const int r0 = ty * RM_TR, c0 = tx * RM_TC;
  for (int base = 0; base < RM_STAGE; base += RM_THREADS) {
    const int s = base + tid;
    if (s < RM_STAGE) {
      const int sr = s / RM_SW, sc = s - sr * RM_SW;
      const int r = r0 - 1 + sr, c = c0 - 1 + sc;
      const bool in = r >= 0 && r < rows && c >= 0 && c < cols;
      const bool free_cell = in && kind[r * cols + c] >= RM_FREE;
      d_s[s] = free_cell ? key_ld(&key[r * cols + c]) : RM_NONE;     // a blocked or void cell passes nothing on
      f_s[s] = free_cell ? 1 : 0;
    }
  }
  __syncthreads();
  unsigned moves[RM_PER];
  u64 cur[RM_PER], first[RM_PER];
  int pos[RM_PER];
#pragma unroll
  for (int j = 0; j < RM_PER; ++j) {
    const int t = j * RM_THREADS + tid, tr = t / RM_TC, tc = t % RM_TC;
    pos[j] = (tr + 1) * RM_SW + tc + 1;
    bool f[3][3];
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
      for (int b = 0; b < 3; ++b) f[a][b] = f_s[pos[j] + (a - 1) * RM_SW + b - 1] != 0;
    moves[j] = f[1][1] ? rooms_moves(f) : 0u;                        // a cell that is not free, or outside the grid, is never entered
    cur[j] = first[j] = d_s[pos[j]];
  }
  bool settled = false;
  for (int n = 0; n < RM_ROUNDS; ++n) {
    bool low = false;
#pragma unroll
    for (int j = 0; j < RM_PER; ++j) {
      if (!moves[j]) continue;
      const int p = pos[j];
      const unsigned m = moves[j];
      // a neighbour's key of this round or of the one before: either stands for a real path
      u64 best = cur[j];
      best = min(best, rooms_via(m & 1u, lds_ld64(&d_s[p - RM_SW - 1]), RM_DIAG));
      best = min(best, rooms_via(m & 2u, lds_ld64(&d_s[p - RM_SW]), RM_ORTH));
      best = min(best, rooms_via(m & 4u, lds_ld64(&d_s[p - RM_SW + 1]), RM_DIAG));
      best = min(best, rooms_via(m & 8u, lds_ld64(&d_s[p - 1]), RM_ORTH));
      best = min(best, rooms_via(m & 16u, lds_ld64(&d_s[p + 1]), RM_ORTH));
      best = min(best, rooms_via(m & 32u, lds_ld64(&d_s[p + RM_SW - 1]), RM_DIAG));
      best = min(best, rooms_via(m & 64u, lds_ld64(&d_s[p + RM_SW]), RM_ORTH));
      best = min(best, rooms_via(m & 128u, lds_ld64(&d_s[p + RM_SW + 1]), RM_DIAG));
      if (best < cur[j]) {
        cur[j] = best;
        lds_st64(&d_s[p], best);
        low = true;
      }
    }
    const int slot = n % 3;
    if (__ballot(low) && lane == 0) low_s[slot] = 1;
    __syncthreads();
    const bool any = low_s[slot] != 0;
    if (tid == 0) low_s[(n + 2) % 3] = 0;                            // round n + 2 sets it, behind the barrier of round n + 1
    if (!any) {                                                      // uniform over the workgroup
      settled = true;
      break;
    }
  }
  if (!settled && tid == 0) atomicOr(&raw[0], RG_ST_TILE);
  bool lowered = false;
#pragma unroll
  for (int j = 0; j < RM_PER; ++j) {
    if (cur[j] < first[j]) {                                         // its own cells only: free cells inside the grid
      const int t = j * RM_THREADS + tid;
      key_st(&key[(r0 + t / RM_TC) * cols + c0 + t % RM_TC], cur[j]);
      lowered = true;
    }
  }
  if (__ballot(lowered) && lane == 0) flags_set[blockIdx.x] = 1;
}

__global__ __launch_bounds__(256) void rooms_assign_kernel(const unsigned char* __restrict__ kind, const u64* __restrict__ key, int N,
                                                           int tiles, const int* __restrict__ flags_last, int* __restrict__ grow_dist,
                                                           int* __restrict__ room_of, int* __restrict__ slot, int* __restrict__ area,
                                                           int* __restrict__ counts, int* __restrict__ status) {
  __shared__ int cnt_s[6];
  const int tid = threadIdx.x, lane = tid & 63;
  const int i = blockIdx.x * 256 + tid;
  if (tid < 6) cnt_s[tid] = 0;
  __syncthreads();
  if (i < tiles && flags_last[i] != 0) atomicOr(&status[0], 1);      // a tile lowered a key in the last sweep
  int kd = -1;
  bool assigned = false, grown = false;
  if (i < N) {
    kd = kind[i];
    const u64 k = key[i];
    assigned = kd >= RM_FREE && k != RM_NONE;
    grown = assigned && (k >> 32) != 0ull;
    grow_dist[i] = assigned ? (int)(unsigned)(k >> 32) : INT_MAX;
    room_of[i] = assigned ? (int)(unsigned)k : -1;                   // the second flatten's parent: the room's label cell holds itself
    slot[i] = -1;
    area[i] = 0;
  }
  const u64 b0 = __ballot(kd == RM_BLOCKED), b1 = __ballot(kd == RM_VOID), b2 = __ballot(kd >= RM_FREE), b4 = __ballot(grown);
  const u64 b5 = __ballot(kd >= RM_FREE && !assigned);
  if (lane == 0) {
    if (b0) atomicAdd(&cnt_s[0], __popcll(b0));
    if (b1) atomicAdd(&cnt_s[1], __popcll(b1));
    if (b2) atomicAdd(&cnt_s[2], __popcll(b2));
    if (b4) atomicAdd(&cnt_s[4], __popcll(b4));
    if (b5) atomicAdd(&cnt_s[5], __popcll(b5));
  }
  __syncthreads();
  if (tid < 6 && cnt_s[tid] > 0) atomicAdd(&counts[tid], cnt_s[tid]);
}

struct RoomsOut {        // the per-slot, per-pair and per-object arrays of the entry point
  int *room, *area, *core_area, *bbox;
  u64 *sum_rc, *widest_key;
  int *widest_d2, *widest_cell, *room_objects, *door_edges;
  u64* door_key;
  int *door_d2, *door_cell, *obj_room_cells, *obj_room, *obj_room_label;
};

__global__ __launch_bounds__(RG_SEL_THREADS) void rooms_select_kernel(const int* __restrict__ area, const int* __restrict__ core_area,
                                                                       int* __restrict__ slot, const int* __restrict__ list,
                                                                       const int* __restrict__ count, int N, int K, int K_obj,
                                                                       const RoomsOut o) {
  __shared__ u64 red_s[RG_SEL_THREADS / 64];
  const int tid = threadIdx.x;
  const int n = count[0] < N ? count[0] : N;
  for (int e = tid; e < K * K; e += RG_SEL_THREADS) {
    o.door_edges[e] = 0;
    o.door_key[e] = 0ull;
  }
  for (int e = tid; e < K_obj * K; e += RG_SEL_THREADS) o.obj_room_cells[e] = 0;
  u64 prev = ~0ull;                                                   // above every key
  for (int k = 0; k < K; ++k) {
    u64 best = 0ull;                                                  // below every key: a room's area is at least 1
    if (prev) {                                                       // block-uniform
      for (int j = tid; j < n; j += RG_SEL_THREADS) {
        const int root = list[j];
        const u64 key = ((u64)(unsigned)area[root] << 32) | (unsigned)~root;
        if (key < prev && key > best) best = key;
      }
    }
    prev = block_max_u64(best, red_s);                                // 0 once the rooms are used up: the rest is padding
    if (tid == 0) {
      const int root = (int)~(unsigned)prev;
      o.room[k] = prev ? root : -1;
      o.area[k] = (int)(prev >> 32);
      o.core_area[k] = prev ? core_area[root] : 0;
      o.bbox[4 * k + 0] = prev ? INT_MAX : 0;
      o.bbox[4 * k + 1] = prev ? INT_MAX : 0;
      o.bbox[4 * k + 2] = prev ? -1 : 0;
      o.bbox[4 * k + 3] = prev ? -1 : 0;
      o.sum_rc[2 * k] = 0ull;
      o.sum_rc[2 * k + 1] = 0ull;
      o.widest_key[k] = 0ull;
      if (prev) slot[root] = k;
    }
  }
}

__global__ __launch_bounds__(RG_THREADS) void rooms_stats_kernel(const int* __restrict__ room_labels, const int* __restrict__ slot,
                                                                  const int* __restrict__ d2, const unsigned char* __restrict__ slotb,
                                                                  int N, int rows, int cols, int K, int K_obj, const RoomsOut o) {
  __shared__ int bb_s[EOD_ROOMS_TOPK_MAX][4];
  __shared__ u64 acc_s[EOD_ROOMS_TOPK_MAX][3];                        // sum of rows, sum of columns, widest key
  __shared__ int pk_s[RM_PAIRS], pc_s[RM_PAIRS];                      // a pair's key and count
  __shared__ u64 pm_s[RM_PAIRS];                                      // a doorway pair's door key
  const int tid = threadIdx.x;
  if (tid < K) {
    bb_s[tid][0] = INT_MAX; bb_s[tid][1] = INT_MAX; bb_s[tid][2] = -1; bb_s[tid][3] = -1;
    acc_s[tid][0] = 0ull; acc_s[tid][1] = 0ull; acc_s[tid][2] = 0ull;
  }
  for (int e = tid; e < RM_PAIRS; e += RG_THREADS) {
    pk_s[e] = -1;
    pc_s[e] = 0;
    pm_s[e] = 0ull;
  }
  __syncthreads();
  // pair < RM_OBJ: the doorway (a << 6) | b; from RM_OBJ on: object slot k and room slot s as RM_OBJ + ((k << 6) | s)
  auto commit = [&](int pair, int n, u64 mx) {
    if (pair < RM_OBJ) {
      const int e = (pair >> 6) * K + (pair & 63);
      atomicAdd(&o.door_edges[e], n);
      atomicMax(&o.door_key[e], mx);
    } else {
      atomicAdd(&o.obj_room_cells[((pair - RM_OBJ) >> 6) * K + (pair & 63)], n);
    }
  };
  auto add = [&](int pair, u64 mx) {
    unsigned h = ((unsigned)pair * 2654435761u) >> (32 - RM_PAIRS_LOG2);
    for (int probe = 0; probe < RM_PROBES; ++probe) {
      int old = lds_ld(&pk_s[h]);
      if (old == -1) old = atomicCAS(&pk_s[h], -1, pair);
      if (old == -1 || old == pair) {
        atomicAdd(&pc_s[h], 1);
        if (mx) atomicMax(&pm_s[h], mx);
        return;
      }
      h = (h + 1) & (RM_PAIRS - 1);
    }
    commit(pair, 1, mx);                                              // no entry within the probes: the same sums in another order
  };
  const int base = blockIdx.x * RG_STAT_CELLS;
  for (int j = tid; j < RG_STAT_CELLS; j += RG_THREADS) {
    const int i = base + j;
    if (i >= N) break;
    const int lab = room_labels[i];
    if (lab < 0) continue;
    const int s = slot[lab];
    if (s < 0) continue;
    const int r = i / cols, c = i - r * cols;
    const u64 wkey = ((u64)(unsigned)d2[i] << 32) | (unsigned)~i;
    atomicMin(&bb_s[s][0], r);
    atomicMin(&bb_s[s][1], c);
    atomicMax(&bb_s[s][2], r);
    atomicMax(&bb_s[s][3], c);
    atomicAdd(&acc_s[s][0], (u64)r);
    atomicAdd(&acc_s[s][1], (u64)c);
    atomicMax(&acc_s[s][2], wkey);
    auto door = [&](int nb) {
      const int lb = room_labels[nb];
      if (lb < 0 || lb == lab) return;
      const int sb = slot[lb];
      if (sb >= 0) add((s << 6) | sb, wkey);
    };
    if (r > 0) door(i - cols);
    if (c > 0) door(i - 1);
    if (c < cols - 1) door(i + 1);
    if (r < rows - 1) door(i + cols);
    if (K_obj > 0) {
      u64 touch = 0ull;
#pragma unroll
      for (int a = -1; a <= 1; ++a) {
#pragma unroll
        for (int b = -1; b <= 1; ++b) {
          const int rr = r + a, cc = c + b;
          if (rr < 0 || rr >= rows || cc < 0 || cc >= cols) continue;
          const unsigned v = slotb[rr * cols + cc];
          if (v != RM_NOSLOT) touch |= 1ull << (v & 63u);
        }
      }
      for (int n = 0; n < 9 && touch; ++n) {                         // at most the nine cells' slots
        const int k = __ffsll((long long)touch) - 1;
        touch &= touch - 1;
        add(RM_OBJ + ((k << 6) | s), 0ull);
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
    atomicMax(&o.widest_key[tid], acc_s[tid][2]);
  }
  for (int e = tid; e < RM_PAIRS; e += RG_THREADS)
    if (pk_s[e] >= 0) commit(pk_s[e], pc_s[e], pm_s[e]);
}

__global__ __launch_bounds__(RG_SEL_THREADS) void rooms_finish_kernel(int K, int K_obj, const RoomsOut o, const int* __restrict__ raw,
                                                                       int* __restrict__ status) {
  __shared__ int ro_s[EOD_ROOMS_TOPK_MAX];
  const int tid = threadIdx.x;
  if (tid < EOD_ROOMS_TOPK_MAX) ro_s[tid] = 0;
  __syncthreads();
  for (int e = tid; e < K * K; e += RG_SEL_THREADS) {
    const u64 key = o.door_key[e];
    o.door_d2[e] = (int)(unsigned)(key >> 32);
    o.door_cell[e] = key ? (int)~(unsigned)key : -1;
  }
  if (tid < K) {
    const u64 key = o.widest_key[tid];
    o.widest_d2[tid] = (int)(unsigned)(key >> 32);
    o.widest_cell[tid] = key ? (int)~(unsigned)key : -1;
  }
  if (tid < K_obj) {
    int best = -1, most = 0;
    for (int s = 0; s < EOD_ROOMS_TOPK_MAX; ++s) {
      if (s >= K) break;
      const int n = o.obj_room_cells[tid * K + s];
      if (n > most) {                                                 // the lowest slot wins a tie
        most = n;
        best = s;
      }
    }
    o.obj_room[tid] = best;
    o.obj_room_label[tid] = best >= 0 ? o.room[best] : -1;
    if (best >= 0) atomicAdd(&ro_s[best], 1);
  }
  __syncthreads();
  if (tid < K) o.room_objects[tid] = ro_s[tid];
  if (tid == 0 && raw[0] != 0) atomicOr(&status[0], 2);
}

inline bool rooms_dims_ok(int N, int cols) {
  return N >= 1 && N <= EOD_ROOMS_N_MAX && cols >= 1 && N % cols == 0 && cols <= EOD_ROOMS_DIM_MAX && N / cols <= EOD_ROOMS_DIM_MAX;
}

inline int rooms_tiles(int N, int cols) { return ((N / cols + RM_TR - 1) / RM_TR) * ((cols + RM_TC - 1) / RM_TC); }

inline bool rooms_aligned(const void* p, unsigned a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1u)) == 0; }

}  // namespace

// the workspace: parent, slot, core_area, room_of, area [N] int32 | raw status | key uint64 [N] | kind [N] bytes | slots [N] bytes |
// three flags per tile
extern "C" size_t eod_map_rooms_workspace_bytes(int N, int cols) {
  if (!rooms_dims_ok(N, cols)) return 0;
  return up256((size_t)5 * N * 4) + 256 + up256((size_t)N * 8) + 2 * up256((size_t)N) + up256((size_t)3 * rooms_tiles(N, cols) * 4);
}

extern "C" int eod_map_rooms(const int32_t* labels, const int32_t* passable, const int32_t* d2, const uint8_t* known,
                             const int32_t* objects, int N, int P, int cols, int K_obj, int door_r2, int min_cells, int topk, int sweeps,
                             int32_t* room_labels, int32_t* grow_dist, int32_t* count, int32_t* room, int32_t* area, int32_t* core_area,
                             int32_t* bbox, uint64_t* sum_rc, uint64_t* widest_key, int32_t* widest_d2, int32_t* widest_cell,
                             int32_t* room_objects, int32_t* door_edges, uint64_t* door_key, int32_t* door_d2, int32_t* door_cell,
                             int32_t* obj_room_cells, int32_t* obj_room, int32_t* obj_room_label, int32_t* counts, int32_t* status,
                             void* workspace, size_t workspace_bytes, eod_stream_t stream) {
  if (!rooms_dims_ok(N, cols) || P < 0 || P > EOD_ROOMS_P_MAX || K_obj < 0 || K_obj > EOD_ROOMS_K_MAX || door_r2 < 0 || min_cells < 1 ||
      topk < 1 || topk > EOD_ROOMS_TOPK_MAX || sweeps < 1 || sweeps > EOD_ROOMS_SWEEPS_MAX)
    return EOD_ERR_BAD_DIMS;
  if (!labels || (P > 0 && !passable) || !d2 || !room_labels || !grow_dist || !count || !room || !area || !core_area || !bbox || !sum_rc ||
      !widest_key || !widest_d2 || !widest_cell || !room_objects || !door_edges || !door_key || !door_d2 || !door_cell || !counts ||
      !status || !workspace || (K_obj > 0 && (!objects || !obj_room_cells || !obj_room || !obj_room_label)))
    return EOD_ERR_NULL;
  if (!rooms_aligned(labels, 4) || !rooms_aligned(passable, 4) || !rooms_aligned(d2, 4) || !rooms_aligned(objects, 4) ||
      !rooms_aligned(room_labels, 4) || !rooms_aligned(grow_dist, 4) || !rooms_aligned(count, 4) || !rooms_aligned(room, 4) ||
      !rooms_aligned(area, 4) || !rooms_aligned(core_area, 4) || !rooms_aligned(bbox, 4) || !rooms_aligned(sum_rc, 8) ||
      !rooms_aligned(widest_key, 8) || !rooms_aligned(widest_d2, 4) || !rooms_aligned(widest_cell, 4) ||
      !rooms_aligned(room_objects, 4) || !rooms_aligned(door_edges, 4) || !rooms_aligned(door_key, 8) || !rooms_aligned(door_d2, 4) ||
      !rooms_aligned(door_cell, 4) || !rooms_aligned(obj_room_cells, 4) || !rooms_aligned(obj_room, 4) ||
      !rooms_aligned(obj_room_label, 4) || !rooms_aligned(counts, 4) || !rooms_aligned(status, 4) || !rooms_aligned(workspace, 8))
    return EOD_ERR_ALIGN;
  if (workspace_bytes < eod_map_rooms_workspace_bytes(N, cols)) return EOD_ERR_CAPACITY;
  hipStream_t s = (hipStream_t)stream;
  const int rows = N / cols;
  const int tiles_r = (rows + RG_TR - 1) / RG_TR, tiles_c = (cols + RG_TC - 1) / RG_TC, tiles = tiles_r * tiles_c;   // fewer than 2^18
  char* ws = static_cast<char*>(workspace);
  int* parent = reinterpret_cast<int*>(ws);
  int* slot = parent + (size_t)N;
  int* core_area_ws = slot + (size_t)N;
  int* room_of = core_area_ws + (size_t)N;
  int* area_ws = room_of + (size_t)N;
  size_t at = up256((size_t)5 * N * 4);
  int* raw = reinterpret_cast<int*>(ws + at);                        // [0] the loops' bounds, [1], [2] the flatten launches' foreground
  at += 256;
  u64* key = reinterpret_cast<u64*>(ws + at);
  at += up256((size_t)N * 8);
  unsigned char* kind = reinterpret_cast<unsigned char*>(ws + at);
  at += up256((size_t)N);
  unsigned char* slotb = reinterpret_cast<unsigned char*>(ws + at);
  at += up256((size_t)N);
  int* flags = reinterpret_cast<int*>(ws + at);
  RoomsOut o;
  o.room = (int*)room; o.area = (int*)area; o.core_area = (int*)core_area; o.bbox = (int*)bbox;
  o.sum_rc = reinterpret_cast<u64*>(sum_rc); o.widest_key = reinterpret_cast<u64*>(widest_key);
  o.widest_d2 = (int*)widest_d2; o.widest_cell = (int*)widest_cell; o.room_objects = (int*)room_objects;
  o.door_edges = (int*)door_edges; o.door_key = reinterpret_cast<u64*>(door_key); o.door_d2 = (int*)door_d2;
  o.door_cell = (int*)door_cell; o.obj_room_cells = (int*)obj_room_cells; o.obj_room = (int*)obj_room;
  o.obj_room_label = (int*)obj_room_label;
  const int per_cell = (N + RG_THREADS - 1) / RG_THREADS, chunks = (N + RG_FLAT_CELLS - 1) / RG_FLAT_CELLS;
  hipLaunchKernelGGL(rooms_classify_kernel, dim3((N + 255) / 256), dim3(256), 0, s, (const int*)labels, (const int*)passable,
                     (const int*)d2, (const unsigned char*)known, (const int*)objects, N, P, K_obj, door_r2, tiles, kind, slotb, flags,
                     (int*)count, (int*)counts, (int*)status, raw);      // tiles <= N, and a launch has at least 256 threads
  hipLaunchKernelGGL(rooms_tile_kernel, dim3(tiles), dim3(RG_THREADS), 0, s, (const unsigned char*)kind, rows, cols, tiles_c, parent, slot,
                     core_area_ws, raw);
  hipLaunchKernelGGL(rooms_border_kernel, dim3(per_cell), dim3(RG_THREADS), 0, s, parent, N, cols, raw);
  hipLaunchKernelGGL(regions_compress_kernel, dim3(per_cell), dim3(RG_THREADS), 0, s, parent, (const int*)slot, N, raw);
  hipLaunchKernelGGL(regions_flatten_kernel, dim3(chunks), dim3(RG_FLAT_THREADS), 0, s, (const int*)parent, N, (int*)room_labels,
                     core_area_ws, raw + 1, raw);
  hipLaunchKernelGGL(regions_list_kernel, dim3(chunks), dim3(RG_FLAT_THREADS), 0, s, (const int*)room_labels, (const int*)core_area_ws,
                     parent, N, min_cells, (int*)count);
  hipLaunchKernelGGL(rooms_seed_kernel, dim3((N + 255) / 256), dim3(256), 0, s, (const unsigned char*)kind, (const int*)room_labels,
                     (const int*)core_area_ws, N, min_cells, key, (int*)counts);
  for (int n = 0; n < sweeps; ++n)
    hipLaunchKernelGGL(rooms_sweep_kernel, dim3(tiles), dim3(RM_THREADS), 0, s, (const unsigned char*)kind, rows, cols, tiles_r, tiles_c,
                       (const int*)(flags + (n % 3) * tiles), flags + ((n + 1) % 3) * tiles, flags + ((n + 2) % 3) * tiles, key, raw);
  hipLaunchKernelGGL(rooms_assign_kernel, dim3((N + 255) / 256), dim3(256), 0, s, (const unsigned char*)kind, (const u64*)key, N, tiles,
                     (const int*)(flags + (sweeps % 3) * tiles), (int*)grow_dist, room_of, slot, area_ws, (int*)counts, (int*)status);
  hipLaunchKernelGGL(regions_flatten_kernel, dim3(chunks), dim3(RG_FLAT_THREADS), 0, s, (const int*)room_of, N, (int*)room_labels, area_ws,
                     raw + 2, raw);
  hipLaunchKernelGGL(rooms_select_kernel, dim3(1), dim3(RG_SEL_THREADS), 0, s, (const int*)area_ws, (const int*)core_area_ws, slot,
                     (const int*)parent, (const int*)count, N, topk, K_obj, o);
  hipLaunchKernelGGL(rooms_stats_kernel, dim3((N + RG_STAT_CELLS - 1) / RG_STAT_CELLS), dim3(RG_THREADS), 0, s, (const int*)room_labels,
                     (const int*)slot, (const int*)d2, (const unsigned char*)slotb, N, rows, cols, topk, K_obj, o);
  hipLaunchKernelGGL(rooms_finish_kernel, dim3(1), dim3(RG_SEL_THREADS), 0, s, topk, K_obj, o, (const int*)raw, (int*)status);
  return eod_launch_status();
}
