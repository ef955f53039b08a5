// Routes on the map (eod_map_route; semantics in include/eod_route.h): from one cell the cheapest path of 8-neighbour moves round
// the blocked cells of a label map to every cell, and for up to 64 objects the free cell beside each to stop on and the path
// there.  A read-only query beside the frame.  Four kernels; what one needs of another is complete at the launch boundary between
// them, and no workgroup ever waits for another one.
//
//   route_init_kernel    one thread per cell.  One byte per cell to the workspace: bit 7 free, bits 0..6 the slot (RT_NOSLOT: none),
//                        found as describe_pool_kernel finds it: lane l holds objects[l] and passable[l], the wave compares a cell's
//                        label with all of them at once, and a ballot and a find-first give the lowest slot.  Once per cell, not
//                        once per sweep.  Unless resume is set, dist to INT_MAX with 0 at the start.  The tile activity flags: only
//                        the start's tile is active, or every tile on resume.  status, counts, cells to 0, goal_key to all ones.
//   route_sweep_kernel   the hot path, queued `sweeps` times.  A workgroup of four waves owns a tile of RT_TR x RT_TC = 32 x 32 cells,
//                        a thread four of them (the header's tile constants; 64 x 64 builds too: DESIGN 3.13).  It reads the
//                        flags of its own tile and its 8 neighbour tiles as the previous sweep left them and returns when none is set.  Otherwise it stages dist and the free bit of its cells and of a
//                        halo of one cell in LDS (cells outside the grid: blocked, so a row's end never meets the next row's
//                        start; the corner rule needs nothing further out), works out once per cell the set of the 8 moves that
//                        may enter it, and relaxes in LDS, every cell taking the minimum over those moves, until one round lowers
//                        nothing: at most RT_TR * RT_TC rounds (a cell is final after as many rounds as its cheapest path has moves
//                        inside the tile, and that path visits no cell twice).  It stores the cells it lowered, its own cells
//                        only, with plain stores, and sets its flag for this sweep if there was one.
//                        The flags rotate over three buffers: sweep s reads buffer s % 3 (written by sweep s - 1), sets in buffer
//                        (s + 1) % 3 and clears its tile's flag in buffer (s + 2) % 3, which sweep s + 1 sets in: no sweep reads a
//                        flag of its own launch.
//   route_finish_kernel  one thread per cell: parent (the eight neighbours in ascending cell order, the first that fits), the free
//                        and the reached cells, the slots' cells, and per reached free cell the 64-bit set of the slots among its
//                        3 x 3 neighbours: per slot one LDS atomicMin of (dist << 32) | cell, then one global 64-bit atomicMin per
//                        slot the workgroup met, as relations_pair_kernel flushes.  Sets status bit 0 if a flag of the last sweep
//                        is set.
//   route_path_kernel    one wave per slot: lane 0 unpacks goal_key and chases parent, at most path_max dependent loads; the wave
//                        fills the rest of the row with -1.
//
// THE INVARIANT: every value ever stored in dist[i] is INT_MAX or the cost of a real path from the start to i (the start's 0, or a
// free neighbour's stored value plus the cost of a legal move), and values only fall.  So a read of a neighbour tile's cell that is
// stale (another XCD's L2, a store of the same launch not yet seen) is still a valid upper bound, and the shortest distances are
// the only fixed point.  What a tile missed in sweep s it sees in sweep s + 1: the launch boundary makes the neighbour's stores and
// its flag visible, and the flag makes the tile run.  At status == 0 no tile lowered anything in the last sweep although every tile
// beside a change of the sweep before ran: dist is the fixed point, a pure function of the inputs, and parent, goals, paths and
// counts are computed from it with integer min and add alone: the same bits on every call, for every tile size and schedule.
// BOUNDS: labels, dist, parent and the cell bytes are indexed by r * cols + c with 0 <= r < rows, 0 <= c < cols only; the LDS stage
// by (tr + 1 + dr) * RT_SW + tc + 1 + dc with 0 <= tr < RT_TR, 0 <= tc < RT_TC, |dr|, |dc| <= 1, inside (RT_TR + 2) * (RT_TC + 2); a
// tile's flags by y * tiles_x + x with 0 <= y < tiles_y, 0 <= x < tiles_x; a slot is < 64 by construction (a bit of a ballot) and < K because
// objects[l] is -1 from lane K on; the path chase follows parent, which holds -1 or a neighbour inside the grid whatever dist holds.
// Every loop has a compile-time bound.
#include "eod_common.h"
#include "../../include/eod_route.h"
#include <climits>

namespace {

typedef unsigned long long u64;

constexpr int RT_TR = EOD_ROUTE_TILE_ROWS, RT_TC = EOD_ROUTE_TILE_COLS, RT_THREADS = 256, RT_PER = RT_TR * RT_TC / RT_THREADS;
constexpr int RT_SW = RT_TC + 2, RT_STAGE = (RT_TR + 2) * RT_SW;     // the tile and a halo of one cell
constexpr int RT_ROUNDS = RT_TR * RT_TC;                             // the bound of the in-tile relaxation
constexpr int RT_K = EOD_ROUTE_K_MAX;
constexpr unsigned RT_FREE = 0x80u, RT_NOSLOT = 0x7Fu;               // a cell's byte: free | slot
constexpr unsigned RT_ORTH = EOD_ROUTE_COST_ORTH, RT_DIAG = EOD_ROUTE_COST_DIAG;
constexpr unsigned RT_INF = (unsigned)INT_MAX;
constexpr u64 RT_NONE = ~0ull;
static_assert(RT_K == 64 && EOD_ROUTE_P_MAX == 64, "one wave looks a label up; the touch mask is one 64-bit word");
static_assert(RT_PER >= 1 && RT_PER * RT_THREADS == RT_TR * RT_TC && (RT_TC & (RT_TC - 1)) == 0,
              "the cell <-> thread mapping of the sweep kernel");
static_assert((u64)EOD_ROUTE_COST_DIAG * EOD_ROUTE_N_MAX < (u64)INT_MAX, "a cost is never INT_MAX, and INT_MAX + a move does not wrap");

// the eight moves in ascending order of the cell they come from: bit b of a move set is move b
__device__ __constant__ const int route_dr[8] = {-1, -1, -1, 0, 0, 1, 1, 1};
__device__ __constant__ const int route_dc[8] = {-1, 0, 1, -1, 1, -1, 0, 1};

inline size_t route_up256(size_t v) { return (v + 255) & ~(size_t)255; }

// the moves that may enter a free cell, from the free bits f[dr + 1][dc + 1] of its 3 x 3 neighbourhood: the source is free, and a
// diagonal move has both cells it passes between free
__device__ __forceinline__ unsigned route_moves(const bool f[3][3]) {
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

__global__ __launch_bounds__(256) void route_init_kernel(const int* __restrict__ labels, const int* __restrict__ objects,
                                                         const int* __restrict__ passable, int N, int K, int P, int from_cell, int resume,
                                                         int tiles, int start_tile, int* __restrict__ dist,
                                                         unsigned char* __restrict__ info, int* __restrict__ flags,
                                                         u64* __restrict__ goal_key, int* __restrict__ cells, int* __restrict__ counts,
                                                         int* __restrict__ status) {
  const int i = blockIdx.x * 256 + threadIdx.x, lane = threadIdx.x & 63;
  const int obj = lane < K ? objects[lane] : -1;
  const bool has_pas = lane < P;
  const int pas = has_pas ? passable[lane] : 0;
  const int lab = i < N ? labels[i] : -1;
  unsigned slot = RT_NOSLOT;
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
    const bool free_cell = lab < 0 || pass || i == from_cell;        // the robot stands on the start, whatever the label says
    info[i] = (unsigned char)((free_cell ? RT_FREE : 0u) | slot);
    if (!resume) dist[i] = i == from_cell ? 0 : INT_MAX;
  }
  if (i < tiles) {
    flags[i] = (resume || i == start_tile) ? 1 : 0;                  // what sweep 0 reads
    flags[tiles + i] = 0;                                            // what sweep 0 sets in
    flags[2 * tiles + i] = 0;
  }
  if (i < K) {
    goal_key[i] = RT_NONE;
    cells[i] = 0;
  }
  if (i == 0) {
    counts[0] = 0;
    counts[1] = 0;
    status[0] = 0;
    status[1] = 0;
  }
}

__global__ __launch_bounds__(RT_THREADS) void route_sweep_kernel(const unsigned char* __restrict__ info, int rows, int cols, int tiles_y,
                                                                 int tiles_x, const int* __restrict__ flags_read,
                                                                 int* __restrict__ flags_set, int* __restrict__ flags_clear, int* dist,
                                                                 int* __restrict__ status) {
  __shared__ unsigned d_s[RT_STAGE];                                 // 4624 B at 32 x 32: dist of the tile and its halo; RT_INF where not free
  __shared__ unsigned char f_s[RT_STAGE];                            // 1156 B: 1 where free
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
  const int r0 = ty * RT_TR, c0 = tx * RT_TC;
  for (int base = 0; base < RT_STAGE; base += RT_THREADS) {
    const int s = base + tid;
    if (s < RT_STAGE) {
      const int sr = s / RT_SW, sc = s - sr * RT_SW;
      const int r = r0 - 1 + sr, c = c0 - 1 + sc;
      const bool in = r >= 0 && r < rows && c >= 0 && c < cols;
      const bool free_cell = in && (info[r * cols + c] & RT_FREE) != 0;
      d_s[s] = free_cell ? (unsigned)dist[r * cols + c] : RT_INF;    // a blocked cell passes nothing on, whatever dist holds
      f_s[s] = free_cell ? 1 : 0;
    }
  }
  __syncthreads();
  unsigned moves[RT_PER], cur[RT_PER], first[RT_PER];
  int pos[RT_PER];
#pragma unroll
  for (int j = 0; j < RT_PER; ++j) {
    const int t = j * RT_THREADS + tid, tr = t / RT_TC, tc = t % RT_TC;
    pos[j] = (tr + 1) * RT_SW + tc + 1;
    bool f[3][3];
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
      for (int b = 0; b < 3; ++b) f[a][b] = f_s[pos[j] + (a - 1) * RT_SW + b - 1] != 0;
    moves[j] = f[1][1] ? route_moves(f) : 0u;                        // a blocked cell, and a cell outside the grid, is never entered
    cur[j] = first[j] = d_s[pos[j]];
  }
  bool settled = false;
  for (int n = 0; n < RT_ROUNDS; ++n) {
    bool low = false;
#pragma unroll
    for (int j = 0; j < RT_PER; ++j) {
      if (!moves[j]) continue;
      const int p = pos[j];
      const unsigned m = moves[j];
      // a neighbour's value of this round or of the one before: either is the cost of a real path
      const unsigned d0 = d_s[p - RT_SW - 1], d1 = d_s[p - RT_SW], d2 = d_s[p - RT_SW + 1], d3 = d_s[p - 1];
      const unsigned d4 = d_s[p + 1], d5 = d_s[p + RT_SW - 1], d6 = d_s[p + RT_SW], d7 = d_s[p + RT_SW + 1];
      unsigned best = cur[j];
      best = min(best, (m & 1u) ? d0 + RT_DIAG : RT_INF);
      best = min(best, (m & 2u) ? d1 + RT_ORTH : RT_INF);
      best = min(best, (m & 4u) ? d2 + RT_DIAG : RT_INF);
      best = min(best, (m & 8u) ? d3 + RT_ORTH : RT_INF);
      best = min(best, (m & 16u) ? d4 + RT_ORTH : RT_INF);
      best = min(best, (m & 32u) ? d5 + RT_DIAG : RT_INF);
      best = min(best, (m & 64u) ? d6 + RT_ORTH : RT_INF);
      best = min(best, (m & 128u) ? d7 + RT_DIAG : RT_INF);
      if (best < cur[j]) {                                           // RT_INF + a move is above RT_INF: an unreached neighbour gives nothing
        cur[j] = best;
        d_s[p] = best;
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
  if (!settled && tid == 0) atomicOr(&status[0], 2);
  bool lowered = false;
#pragma unroll
  for (int j = 0; j < RT_PER; ++j) {
    if (cur[j] < first[j]) {                                         // its own cells only: free cells inside the grid
      const int t = j * RT_THREADS + tid;
      dist[(r0 + t / RT_TC) * cols + c0 + t % RT_TC] = (int)cur[j];
      lowered = true;
    }
  }
  if (__ballot(lowered) && lane == 0) flags_set[blockIdx.x] = 1;
}

__global__ __launch_bounds__(256) void route_finish_kernel(const unsigned char* __restrict__ info, const int* __restrict__ dist, int N,
                                                           int rows, int cols, int from_cell, int tiles,
                                                           const int* __restrict__ flags_last, int* __restrict__ parent,
                                                           u64* __restrict__ goal_key, int* __restrict__ cells, int* __restrict__ counts,
                                                           int* __restrict__ status) {
  __shared__ u64 key_s[RT_K];
  __shared__ int cells_s[RT_K];
  __shared__ int count_s[2];
  const int tid = threadIdx.x, lane = tid & 63;
  const int i = blockIdx.x * 256 + tid;
  if (tid < RT_K) {
    key_s[tid] = RT_NONE;
    cells_s[tid] = 0;
  }
  if (tid < 2) count_s[tid] = 0;
  __syncthreads();
  if (i < tiles && flags_last[i] != 0) atomicOr(&status[0], 1);      // a tile lowered a value in the last sweep
  bool free_cell = false, reached = false;
  if (i < N) {
    const int r = i / cols, c = i - r * cols;
    bool f[3][3];
    unsigned nd[3][3];
    u64 touch = 0ull;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
#pragma unroll
      for (int b = 0; b < 3; ++b) {
        const int rr = r + a - 1, cc = c + b - 1;
        const bool in = rr >= 0 && rr < rows && cc >= 0 && cc < cols;
        const unsigned v = in ? info[rr * cols + cc] : RT_NOSLOT;
        f[a][b] = (v & RT_FREE) != 0;
        nd[a][b] = f[a][b] ? (unsigned)dist[rr * cols + cc] : RT_INF;
        if ((v & RT_NOSLOT) != RT_NOSLOT) touch |= 1ull << (v & RT_NOSLOT);
      }
    }
    const unsigned mine = info[i] & RT_NOSLOT;
    if (mine != RT_NOSLOT) atomicAdd(&cells_s[mine], 1);
    free_cell = f[1][1];
    const unsigned d = nd[1][1];
    reached = free_cell && d != RT_INF;
    int par = -1;
    if (reached && i != from_cell) {
      const unsigned m = route_moves(f);
#pragma unroll
      for (int b = 7; b >= 0; --b) {                                 // descending, so the lowest cell is written last
        const int a0 = route_dr[b] + 1, b0 = route_dc[b] + 1;
        const unsigned w = (route_dr[b] != 0 && route_dc[b] != 0) ? RT_DIAG : RT_ORTH;
        if (((m >> b) & 1u) && nd[a0][b0] != RT_INF && nd[a0][b0] + w == d) par = (r + route_dr[b]) * cols + c + route_dc[b];
      }
    }
    parent[i] = par;
    if (reached) {
      const u64 key = ((u64)d << 32) | (unsigned)i;
      for (int n = 0; n < 9 && touch; ++n) {                         // at most the nine cells' slots
        const int k = __ffsll((long long)touch) - 1;
        touch &= touch - 1;
        atomicMin(&key_s[k], key);
      }
    }
  }
  const u64 nf = __ballot(free_cell), nr = __ballot(reached);
  if (lane == 0) {
    if (nf) atomicAdd(&count_s[0], __popcll(nf));
    if (nr) atomicAdd(&count_s[1], __popcll(nr));
  }
  __syncthreads();
  if (tid < RT_K) {                                                  // only what this workgroup met
    if (key_s[tid] != RT_NONE) atomicMin(&goal_key[tid], key_s[tid]);
    if (cells_s[tid] > 0) atomicAdd(&cells[tid], cells_s[tid]);
  }
  if (tid < 2 && count_s[tid] > 0) atomicAdd(&counts[tid], count_s[tid]);
}

__global__ __launch_bounds__(64) void route_path_kernel(const u64* __restrict__ goal_key, const int* __restrict__ parent, int from_cell,
                                                        int path_max, int* __restrict__ goal_cost, int* __restrict__ goal_cell,
                                                        int* __restrict__ path, int* __restrict__ path_cells) {
  const int k = blockIdx.x, lane = threadIdx.x;
  int n = 0;
  if (lane == 0) {
    const u64 key = goal_key[k];
    int cur = key == RT_NONE ? -1 : (int)(unsigned)key;
    goal_cost[k] = key == RT_NONE ? INT_MAX : (int)(key >> 32);
    goal_cell[k] = cur;
    for (int t = 0; t < EOD_ROUTE_PATH_MAX; ++t) {
      if (t >= path_max || cur < 0) break;
      path[k * path_max + t] = cur;
      n = t + 1;
      if (cur == from_cell) break;                                   // the start has been written
      cur = parent[cur];
    }
    path_cells[k] = n;
  }
  n = __shfl(n, 0, 64);
  for (int t0 = 0; t0 < EOD_ROUTE_PATH_MAX; t0 += 64) {
    const int t = t0 + lane;
    if (t >= n && t < path_max) path[k * path_max + t] = -1;
  }
}

inline bool route_dims_ok(int N, int cols) {
  return N >= 1 && N <= EOD_ROUTE_N_MAX && cols >= 1 && N % cols == 0 && cols <= EOD_ROUTE_DIM_MAX && N / cols <= EOD_ROUTE_DIM_MAX;
}

inline int route_tiles(int N, int cols) { return ((N / cols + RT_TR - 1) / RT_TR) * ((cols + RT_TC - 1) / RT_TC); }

inline bool route_aligned(const void* p, unsigned a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1u)) == 0; }

}  // namespace

extern "C" size_t eod_map_route_workspace_bytes(int N, int cols) {
  if (!route_dims_ok(N, cols)) return 0;
  return route_up256((size_t)3 * route_tiles(N, cols) * 4) + route_up256((size_t)N);
}

extern "C" int eod_map_route(const int32_t* object_labels, const int32_t* objects, const int32_t* passable, int N, int K, int P, int cols,
                             int from_cell, int path_max, int sweeps, int resume, int32_t* dist, int32_t* parent, uint64_t* goal_key,
                             int32_t* goal_cost, int32_t* goal_cell, int32_t* cells, int32_t* path, int32_t* path_cells, int32_t* counts,
                             int32_t* status, void* workspace, size_t workspace_bytes, eod_stream_t stream) {
  if (!route_dims_ok(N, cols) || K < 1 || K > EOD_ROUTE_K_MAX || P < 0 || P > EOD_ROUTE_P_MAX || from_cell < 0 || from_cell >= N ||
      path_max < 1 || path_max > EOD_ROUTE_PATH_MAX || sweeps < 1 || sweeps > EOD_ROUTE_SWEEPS_MAX || (resume != 0 && resume != 1))
    return EOD_ERR_BAD_DIMS;
  if (!object_labels || !objects || (P > 0 && !passable) || !dist || !parent || !goal_key || !goal_cost || !goal_cell || !cells || !path ||
      !path_cells || !counts || !status || !workspace)
    return EOD_ERR_NULL;
  if (!route_aligned(object_labels, 4) || !route_aligned(objects, 4) || !route_aligned(passable, 4) || !route_aligned(dist, 4) ||
      !route_aligned(parent, 4) || !route_aligned(goal_key, 8) || !route_aligned(goal_cost, 4) || !route_aligned(goal_cell, 4) ||
      !route_aligned(cells, 4) || !route_aligned(path, 4) || !route_aligned(path_cells, 4) || !route_aligned(counts, 4) ||
      !route_aligned(status, 4) || !route_aligned(workspace, 8))
    return EOD_ERR_ALIGN;
  if (workspace_bytes < eod_map_route_workspace_bytes(N, cols)) return EOD_ERR_CAPACITY;
  hipStream_t s = (hipStream_t)stream;
  const int rows = N / cols, tiles_x = (cols + RT_TC - 1) / RT_TC, tiles_y = (rows + RT_TR - 1) / RT_TR, tiles = tiles_x * tiles_y;
  int* flags = static_cast<int*>(workspace);
  unsigned char* info = static_cast<unsigned char*>(workspace) + route_up256((size_t)3 * tiles * 4);
  u64* gk = reinterpret_cast<u64*>(goal_key);
  const int start_tile = (from_cell / cols / RT_TR) * tiles_x + from_cell % cols / RT_TC;
  const int per_cell = ((N > RT_K ? N : RT_K) + 255) / 256;          // tiles <= N
  hipLaunchKernelGGL(route_init_kernel, dim3(per_cell), dim3(256), 0, s, (const int*)object_labels, (const int*)objects,
                     (const int*)passable, N, K, P, from_cell, resume, tiles, start_tile, (int*)dist, info, flags, gk, (int*)cells,
                     (int*)counts, (int*)status);
  for (int n = 0; n < sweeps; ++n)
    hipLaunchKernelGGL(route_sweep_kernel, dim3(tiles), dim3(RT_THREADS), 0, s, (const unsigned char*)info, rows, cols, tiles_y, tiles_x,
                       (const int*)(flags + (n % 3) * tiles), flags + ((n + 1) % 3) * tiles, flags + ((n + 2) % 3) * tiles, (int*)dist,
                       (int*)status);
  hipLaunchKernelGGL(route_finish_kernel, dim3((N + 255) / 256), dim3(256), 0, s, (const unsigned char*)info, (const int*)dist, N, rows,
                     cols, from_cell, tiles, (const int*)(flags + (sweeps % 3) * tiles), (int*)parent, gk, (int*)cells, (int*)counts,
                     (int*)status);
  hipLaunchKernelGGL(route_path_kernel, dim3(K), dim3(64), 0, s, (const u64*)gk, (const int*)parent, from_cell, path_max, (int*)goal_cost,
                     (int*)goal_cell, (int*)path, (int*)path_cells);
  return eod_launch_status();
}
