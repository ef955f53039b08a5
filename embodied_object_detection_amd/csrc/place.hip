// Place detections on the map: for every instance mask, the grid cells under its set pixels (eod_place_masks; semantics in
// include/eod_place.h).  A read-only query beside the frame: integers only, integer atomics only, the result a pure function of the
// inputs.
//
//   place_masks_kernel     one workgroup per detection.  It walks the detection's rect with aligned dword loads of the mask bytes
//                          (the address k*H*W + y*W + x0 has any alignment: the first and the last dword of a row are masked down to
//                          the row's own bytes), skips all-zero words, loads proj for set pixels only and counts cells in an LDS
//                          open-addressing table (atomicCAS on the key, atomicAdd on the count; 2^table_log2 entries).  The top T
//                          are T rounds of a workgroup-wide maximum of (count << 32) | ~cell over the table.
//   place_overflow_kernel  a detection whose cells do not fit the table (an insert found no slot within its probe limit) is queued
//                          and counted again from scratch here: EOD_PLACE_SLOTS workgroups each own a dense int32[n_cells] table in
//                          the workspace.  Distinct cells are the adds that found a zero, the top T are T further walks over the
//                          detection's pixels, and a last walk leaves the table zero for the slot's next detection.  The result of
//                          a detection is the same integers whichever kernel counts it, and the queue's order decides only which
//                          slot does the work.
//
// What it moves: the rect's mask bytes once, 4 bytes of proj per set pixel, a few dozen bytes out per detection; the LDS atomics of
// neighbouring pixels, which mostly share a cell, are merged per dword before they are issued.  What bounds it is not those bytes
// (30-40 MB for 300 detections) but the longest workgroup: a frame's detections are about one workgroup per CU, and each thread's
// walk is a chain of dependent steps (mask word, proj, LDS atomic).  Hence 1024 threads per detection: 256 took 2.6 times as long
// (0.36 against 0.14 ms for 300 detections at 640 x 640; profiles/place_bench.txt).
#include "eod_common.h"
#include "../../include/eod_place.h"
#include <climits>

namespace {

typedef unsigned long long u64;

constexpr int PM_THREADS = 1024;
constexpr int PM_TABLE_MAX = 1 << EOD_PLACE_TABLE_LOG2_MAX;
constexpr int PM_PROBES = 64;            // probe limit of an insert; a full neighbourhood counts as overflow (exact either way)
constexpr int PO_THREADS = 1024;
constexpr int PM_QUEUE_OFF = 64;         // int32 index of the overflow list in the workspace; word 0 is its length

struct PlaceRect {
  int x0, y0, x1, y1;
};

// rect of row k clipped to the image (rects == nullptr: the image); false: empty
__device__ __forceinline__ bool place_rect(const int* __restrict__ rects, int k, int H, int W, PlaceRect& r) {
  r.x0 = 0; r.y0 = 0; r.x1 = W; r.y1 = H;
  if (rects) {
    const int a = rects[k * 4 + 0], b = rects[k * 4 + 1], c = rects[k * 4 + 2], d = rects[k * 4 + 3];
    r.x0 = a < 0 ? 0 : a;
    r.y0 = b < 0 ? 0 : b;
    r.x1 = c > W ? W : c;
    r.y1 = d > H ? H : d;
  }
  return r.x1 > r.x0 && r.y1 > r.y0;
}

// Every non-zero dword of the rect's mask bytes: f(word, p) with the bytes of other pixels zeroed; byte b of `word` is pixel p + b
// of the image (p may lie up to 3 before the row's first pixel: those bytes are zero).  f returns false to stop this thread's walk.
// A dword load is aligned and holds at least one byte of the row, so it stays inside that byte's page.
template <class F>
__device__ __forceinline__ void place_walk(const unsigned char* __restrict__ m, int W, const PlaceRect& r, F&& f) {
  const int w = r.x1 - r.x0;
  const int nd = (w + 6) >> 2;                    // dwords a row of w bytes touches at the worst alignment
  const int items = (r.y1 - r.y0) * nd;           // < H * (W / 4 + 2)
  for (int i = threadIdx.x; i < items; i += blockDim.x) {
    const int row = i / nd, j = i - row * nd;
    const int y = r.y0 + row;
    const uintptr_t a = reinterpret_cast<uintptr_t>(m + (size_t)y * W + r.x0);
    const uintptr_t e = a + (uintptr_t)w;
    const uintptr_t d = (a & ~(uintptr_t)3) + 4u * (uintptr_t)j;
    if (d >= e) continue;
    unsigned word = *reinterpret_cast<const unsigned*>(d);
    if (d < a) word &= 0xFFFFFFFFu << (8u * (unsigned)(a - d));             // little endian: the low byte is the low address
    if (d + 4 > e) word &= 0xFFFFFFFFu >> (8u * (unsigned)(d + 4 - e));
    if (!word) continue;
    const int x = r.x0 + (int)((long long)d - (long long)a);
    if (!f(word, y * W + x)) break;
  }
}

// The set pixels of one word, classified; neighbouring pixels of one cell become one add(cell, n).  cnt[0..2] += set, counted, invalid.
template <class A>
__device__ __forceinline__ void place_word(unsigned word, int p, const int* __restrict__ proj, int n_cells, int exclude, int (&cnt)[3],
                                           A&& add) {
  int cur = -1, n = 0;
#pragma unroll
  for (int b = 0; b < 4; ++b) {
    if (!((word >> (8 * b)) & 0xFFu)) continue;
    ++cnt[0];
    const int c = proj[p + b];
    if ((unsigned)c >= (unsigned)n_cells) {        // never an index
      ++cnt[2];
      continue;
    }
    if (c == exclude) continue;
    ++cnt[1];
    if (c == cur) {
      ++n;
    } else {
      if (n) add(cur, n);
      cur = c;
      n = 1;
    }
  }
  if (n) add(cur, n);
}

__device__ __forceinline__ u64 place_key(int count, int cell) { return ((u64)(unsigned)count << 32) | (unsigned)~cell; }

// sums over the workgroup, in every thread; sum_s: N words
template <int N>
__device__ __forceinline__ void block_sum(int (&v)[N], int* sum_s) {
  if (threadIdx.x < N) sum_s[threadIdx.x] = 0;
  __syncthreads();
#pragma unroll
  for (int j = 0; j < N; ++j) {
    int s = v[j];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
    if ((threadIdx.x & 63) == 0 && s) atomicAdd(&sum_s[j], s);
  }
  __syncthreads();
#pragma unroll
  for (int j = 0; j < N; ++j) v[j] = sum_s[j];
  __syncthreads();
}

// out: mask_pixels, pixels, invalid, distinct [K_cap] each, then cells [K_cap][T], cell_pixels [K_cap][T]
__device__ __forceinline__ void place_write_stats(int* __restrict__ out, int K_cap, int k, int set, int counted, int invalid, int distinct) {
  out[k] = set;
  out[K_cap + k] = counted;
  out[2 * K_cap + k] = invalid;
  out[3 * K_cap + k] = distinct;
}
__device__ __forceinline__ void place_write_top(int* __restrict__ out, int K_cap, int T, int k, int t, u64 key) {
  out[4 * K_cap + k * T + t] = key ? (int)~(unsigned)key : -1;
  out[(4 + T) * K_cap + k * T + t] = (int)(key >> 32);
}

__global__ __launch_bounds__(PM_THREADS) void place_masks_kernel(const unsigned char* __restrict__ masks, const int* __restrict__ proj,
                                                                  const int* __restrict__ count, const int* __restrict__ rects, int K_cap,
                                                                  int H, int W, int n_cells, int T, int exclude, int table_log2,
                                                                  int* __restrict__ out, int* __restrict__ queue) {
  __shared__ int key_s[PM_TABLE_MAX], cnt_s[PM_TABLE_MAX];
  __shared__ u64 red_s[PM_THREADS / 64];
  __shared__ int sum_s[3];
  __shared__ int ovf_s;
  const int k = blockIdx.x, tid = threadIdx.x;
  int n_det = count ? *count : K_cap;
  n_det = n_det > K_cap ? K_cap : n_det;
  PlaceRect r;
  const bool any = k < n_det && place_rect(rects, k, H, W, r);       // block-uniform
  if (!any) {                                                         // padding row, or nothing inside the rect
    if (tid == 0) place_write_stats(out, K_cap, k, 0, 0, 0, 0);
    if (tid < T) place_write_top(out, K_cap, T, k, tid, 0ull);
    return;
  }
  const int size = 1 << table_log2;
  for (int i = tid; i < size; i += PM_THREADS) {
    key_s[i] = -1;
    cnt_s[i] = 0;
  }
  if (tid == 0) ovf_s = 0;
  __syncthreads();
  const unsigned hmask = (unsigned)size - 1u;
  const int probes = size < PM_PROBES ? size : PM_PROBES;
  int cnt[3] = {0, 0, 0};
  auto add = [&](int c, int n) {
    unsigned h = ((unsigned)c * 2654435761u) >> (32 - table_log2);
    for (int probe = 0; probe < probes; ++probe) {
      int old = __hip_atomic_load(&key_s[h], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
      if (old == -1) old = atomicCAS(&key_s[h], -1, c);
      if (old == -1 || old == c) {
        atomicAdd(&cnt_s[h], n);
        return;
      }
      h = (h + 1) & hmask;
    }
    __hip_atomic_store(&ovf_s, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  };
  place_walk(masks + (size_t)k * H * W, W, r, [&](unsigned word, int p) {
    place_word(word, p, proj, n_cells, exclude, cnt, add);
    return __hip_atomic_load(&ovf_s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) == 0;   // overflowed: the walk is void
  });
  __syncthreads();
  if (ovf_s) {                                                        // block-uniform; place_overflow_kernel writes this row
    if (tid == 0) queue[PM_QUEUE_OFF + atomicAdd(&queue[0], 1)] = k;
    return;
  }
  block_sum(cnt, sum_s);
  int distinct[1] = {0};
  for (int i = tid; i < size; i += PM_THREADS) distinct[0] += key_s[i] != -1;
  block_sum(distinct, sum_s);
  if (tid == 0) place_write_stats(out, K_cap, k, cnt[0], cnt[1], cnt[2], distinct[0]);
  u64 prev = ~0ull;                                                   // above every key
  for (int t = 0; t < T; ++t) {
    u64 best = 0ull;                                                  // below every key: a table entry's count is at least 1
    for (int i = tid; i < size; i += PM_THREADS) {
      const int c = key_s[i];
      if (c != -1) {
        const u64 key = place_key(cnt_s[i], c);
        if (key < prev && key > best) best = key;
      }
    }
    prev = block_max_u64(best, red_s);                                // 0 once the cells are used up: the rest is padding
    if (tid == 0) place_write_top(out, K_cap, T, k, t, prev);
  }
}

__global__ __launch_bounds__(PO_THREADS) void place_overflow_kernel(const unsigned char* __restrict__ masks, const int* __restrict__ proj,
                                                                     const int* __restrict__ rects, int K_cap, int H, int W, int n_cells,
                                                                     int T, int exclude, int* __restrict__ out,
                                                                     const int* __restrict__ queue, int* __restrict__ tables,
                                                                     size_t table_stride) {
  __shared__ u64 red_s[PO_THREADS / 64];
  __shared__ int sum_s[4];
  const int tid = threadIdx.x;
  int n = queue[0];
  n = n > K_cap ? K_cap : n;
  if ((int)blockIdx.x >= n) return;                                   // nothing overflowed, or fewer detections than slots
  int* tab = tables + (size_t)blockIdx.x * table_stride;
  // The table is only ever touched by device-scope atomics and by these stores, which the fence completes before the first add.
  for (int i = tid; i < n_cells; i += PO_THREADS) __hip_atomic_store(&tab[i], 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  __threadfence();
  __syncthreads();
  for (int q = blockIdx.x; q < n; q += gridDim.x) {
    const int k = queue[PM_QUEUE_OFF + q];                            // written by place_masks_kernel: 0 <= k < K_cap, rect not empty
    PlaceRect r;
    place_rect(rects, k, H, W, r);
    const unsigned char* m = masks + (size_t)k * H * W;
    int cnt[4] = {0, 0, 0, 0};                                        // set, counted, invalid, distinct
    {
      int c3[3] = {0, 0, 0};
      place_walk(m, W, r, [&](unsigned word, int p) {
        place_word(word, p, proj, n_cells, exclude, c3, [&](int c, int nn) { cnt[3] += atomicAdd(&tab[c], nn) == 0; });
        return true;
      });
      cnt[0] = c3[0]; cnt[1] = c3[1]; cnt[2] = c3[2];
    }
    __threadfence();
    block_sum(cnt, sum_s);                                            // its barriers order the adds before the reads below
    if (tid == 0) place_write_stats(out, K_cap, k, cnt[0], cnt[1], cnt[2], cnt[3]);
    u64 prev = ~0ull;
    for (int t = 0; t < T; ++t) {
      u64 best = 0ull;
      if (prev) {                                                     // block-uniform
        int unused[3] = {0, 0, 0};
        place_walk(m, W, r, [&](unsigned word, int p) {
          place_word(word, p, proj, n_cells, exclude, unused, [&](int c, int) {
            const u64 key = place_key(__hip_atomic_load(&tab[c], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT), c);
            if (key < prev && key > best) best = key;
          });
          return true;
        });
      }
      prev = block_max_u64(best, red_s);
      if (tid == 0) place_write_top(out, K_cap, T, k, t, prev);
    }
    {                                                                 // the table is zero again for the slot's next detection
      int unused[3] = {0, 0, 0};
      place_walk(m, W, r, [&](unsigned word, int p) {
        place_word(word, p, proj, n_cells, exclude, unused,
                   [&](int c, int) { __hip_atomic_store(&tab[c], 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); });
        return true;
      });
    }
    __threadfence();
    __syncthreads();
  }
}

inline size_t up256(size_t v) { return (v + 255) / 256 * 256; }
inline size_t place_table_stride(int n_cells) { return up256((size_t)n_cells * 4) / 4; }     // in int32
inline size_t place_queue_bytes(int K_cap) { return up256(((size_t)PM_QUEUE_OFF + (size_t)K_cap) * 4); }

}  // namespace

extern "C" size_t eod_place_masks_workspace_bytes(int K_cap, int n_cells) {
  if (K_cap < 0 || n_cells < 1) return 0;
  return place_queue_bytes(K_cap) + (size_t)EOD_PLACE_SLOTS * place_table_stride(n_cells) * 4;
}

extern "C" int eod_place_masks(const uint8_t* masks, const int32_t* proj, const int32_t* count, const int32_t* rects, int K_cap, int H,
                               int W, int n_cells, int topk, int exclude_cell, int table_log2, int32_t* out, void* workspace,
                               size_t workspace_bytes, eod_stream_t stream) {
  if (K_cap < 0 || H < 1 || W < 1 || n_cells < 1 || (long long)H * W > INT_MAX - 4 || topk < 1 || topk > EOD_PLACE_TOPK_MAX)
    return EOD_ERR_BAD_DIMS;
  if (table_log2 == 0) table_log2 = EOD_PLACE_TABLE_LOG2;
  if (table_log2 < EOD_PLACE_TABLE_LOG2_MIN || table_log2 > EOD_PLACE_TABLE_LOG2_MAX) return EOD_ERR_BAD_DIMS;
  if ((long long)K_cap * (4 + 2 * topk) > INT_MAX) return EOD_ERR_BAD_DIMS;
  if (K_cap == 0) return EOD_OK;
  if (!masks || !proj || !out || !workspace) return EOD_ERR_NULL;
  auto aligned4 = [](const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3u) == 0; };
  if (!aligned4(proj) || !aligned4(out) || !aligned4(workspace) || (count && !aligned4(count)) || (rects && !aligned4(rects)))
    return EOD_ERR_ALIGN;
  if (workspace_bytes < eod_place_masks_workspace_bytes(K_cap, n_cells)) return EOD_ERR_CAPACITY;
  hipStream_t s = (hipStream_t)stream;
  int* queue = static_cast<int*>(workspace);
  int* tables = reinterpret_cast<int*>(static_cast<char*>(workspace) + place_queue_bytes(K_cap));
  if (hipMemsetAsync(queue, 0, 4, s) != hipSuccess) return EOD_ERR_LAUNCH;
  hipLaunchKernelGGL(place_masks_kernel, dim3(K_cap), dim3(PM_THREADS), 0, s, masks, proj, count, rects, K_cap, H, W, n_cells, topk,
                     exclude_cell, table_log2, out, queue);
  const int slots = K_cap < EOD_PLACE_SLOTS ? K_cap : EOD_PLACE_SLOTS;
  hipLaunchKernelGGL(place_overflow_kernel, dim3(slots), dim3(PO_THREADS), 0, s, masks, proj, rects, K_cap, H, W, n_cells, topk,
                     exclude_cell, out, (const int*)queue, tables, place_table_stride(n_cells));
  return eod_launch_status();
}
