// Object descriptions (eod_describe_pool, eod_describe_classify; semantics in include/eod_describe.h): the memory rows of an
// object's cells pooled into one CLIP-space direction per object, and that direction classified in any vocabulary.  Read-only
// queries beside the frame.  Four kernels; what one needs of another is complete at the launch boundary between them, and no
// workgroup ever waits for another one.
//
//   describe_init_kernel      sum_q and cells to 0: the buffers may hold anything on entry.
//   describe_pool_kernel      the hot path.  A wave owns DS_WAVE_CELLS = 64 consecutive cells, a workgroup of four waves 256.  Lane l
//                             loads the label of cell l of the wave's range and objects[l] (-1 from slot K on).  SLOT LOOKUP: for every
//                             cell with a label >= 0 the wave compares the cell's label with all 64 slots at once; a ballot and a
//                             find-first give the lowest slot, kept in the cell's lane.  No table over the 2^22 labels.  ROWS: only
//                             the rows of cells that have a slot are read, each lane two 16-byte loads (channels 4l..4l+3 and
//                             256+4l..256+4l+3: every load instruction covers 1 KiB without a gap), the next row's loads issued before
//                             this row's arithmetic.  The sum of squares: eight terms per lane in a fixed order, then a butterfly over
//                             the wave, so every lane holds the same bits.  SUMS: each lane keeps its eight int64 sums in registers
//                             while consecutive cells stay in one slot and adds them with 64-bit integer global atomics when the slot
//                             changes and at the end of the wave's range; lane 0 adds the cell count.  An object on a grid is made of
//                             runs along rows, so flushes are rare.  No LDS, no scratch, no float atomics.
//   describe_finish_kernel    one workgroup per slot: mean, norm, embedding and coherence in fp64, the 512 squares summed two per
//                             thread and then over a fixed tree.
//   describe_classify_kernel  one workgroup per object, threads over classes (coalesced reads of zs, channel after channel, the sum in
//                             ascending channel order), the logits in LDS, maximum, expf, a fixed-order sum, one division per class;
//                             then topn rounds of a 64-bit key maximum ((bits of prob << 32) | ~class: prob >= 0, so its bits order
//                             as its values do).
//
// THE INVARIANT of the pooling: every cell with a slot adds its q[c] to exactly one slot exactly once (a run is added when it ends,
// and the running sums return to 0), and q[c] depends on the cell's row alone.  Integer addition is associative and commutative, so
// sum_q and cells do not depend on which wave holds a cell, on the order of the flushes or on the grid.
// BOUNDS: a wave reads labels and rows of cells < N only (its range is clipped to N); a slot is < 64 by construction (a bit of a
// 64-bit ballot) and < K because objects[l] is -1 from lane K on; sum_q has K * 512 words.
#include "eod_common.h"
#include "../../include/eod_describe.h"
#include <cmath>

namespace {

typedef unsigned long long u64;
typedef long long i64;

constexpr int DS_D = EOD_DESCRIBE_D;
constexpr int DS_WAVE_CELLS = 64, DS_POOL_THREADS = 256, DS_WG_CELLS = DS_WAVE_CELLS * (DS_POOL_THREADS / 64);
constexpr int DS_FIN_THREADS = 256;
constexpr int DS_CLS_THREADS = 1024, DS_CLS_PER_THREAD = 2;
static_assert(DS_D == 8 * 64 && DS_D == 2 * DS_FIN_THREADS, "a lane holds eight channels of a row, a finish thread two");
static_assert(EOD_DESCRIBE_C_MAX < DS_CLS_THREADS * DS_CLS_PER_THREAD, "classes per classify thread");
static_assert(EOD_DESCRIBE_K_MAX == 64, "one wave looks a label up");

__global__ __launch_bounds__(256) void describe_init_kernel(int K, u64* __restrict__ sum_q, int* __restrict__ cells) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < K * DS_D) sum_q[i] = 0ull;
  if (i < K) cells[i] = 0;
}

// x = v / n as the header defines it, in fixed point
__device__ __forceinline__ i64 describe_q(float v, float n) {
  float x = v / n;
  x = fabsf(x) <= 3.402823466e+38f ? x : 0.0f;                       // an Inf or a NaN compares false
  x = fminf(fmaxf(x, -1.0f), 1.0f);
  return (i64)(int)(x * 1073741824.0f);                             // exact product; the conversion truncates
}

__device__ __forceinline__ void describe_flush(u64* __restrict__ sum_q, int* __restrict__ cells, int slot, int lane, i64 (&acc)[8], int& run) {
  u64* row = sum_q + (size_t)slot * DS_D;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    if (acc[j] != 0) atomicAdd(&row[(j >> 2) * 256 + 4 * lane + (j & 3)], (u64)acc[j]);     // two's complement: the sum of the int64
    acc[j] = 0;
  }
  if (lane == 0) atomicAdd(&cells[slot], run);
  run = 0;
}

__global__ __launch_bounds__(DS_POOL_THREADS) void describe_pool_kernel(const float* __restrict__ mem, const int* __restrict__ labels,
                                                                        const int* __restrict__ objects, int N, int K,
                                                                        u64* __restrict__ sum_q, int* __restrict__ cells) {
  const int lane = threadIdx.x & 63;
  const int base = blockIdx.x * DS_WG_CELLS + (threadIdx.x >> 6) * DS_WAVE_CELLS;      // wave-uniform; N <= 2^22: no overflow
  if (base >= N) return;
  const int cell = base + lane;
  const int lab = cell < N ? labels[cell] : -1;
  const int obj = lane < K ? objects[lane] : -1;
  // the slot of every cell of the range, in the cell's lane
  int slot = -1;
  u64 todo = __ballot(lab >= 0);
  while (todo) {                                                     // wave-uniform
    const int j = __ffsll((i64)todo) - 1;
    todo &= todo - 1;
    const int l = __shfl(lab, j, 64);
    const u64 hit = __ballot(obj >= 0 && obj == l);
    if (lane == j && hit) slot = __ffsll((i64)hit) - 1;               // the lowest slot wins a duplicate
  }
  u64 rows = __ballot(slot >= 0);
  if (!rows) return;
  i64 acc[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) acc[j] = 0;
  int run = 0;
  int j = __ffsll((i64)rows) - 1;
  rows &= rows - 1;
  int cur = __shfl(slot, j, 64);
  const f32x4* p = reinterpret_cast<const f32x4*>(mem + (size_t)(base + j) * DS_D);
  f32x4 a0 = p[lane], a1 = p[64 + lane];
  for (;;) {
    const bool more = rows != 0;                                     // wave-uniform
    int jn = 0;
    f32x4 b0 = a0, b1 = a1;
    if (more) {                                                      // the next row's loads before this row's arithmetic
      jn = __ffsll((i64)rows) - 1;
      rows &= rows - 1;
      const f32x4* pn = reinterpret_cast<const f32x4*>(mem + (size_t)(base + jn) * DS_D);
      b0 = pn[lane];
      b1 = pn[64 + lane];
    }
    float s = a0.x * a0.x;
    s += a0.y * a0.y; s += a0.z * a0.z; s += a0.w * a0.w;
    s += a1.x * a1.x; s += a1.y * a1.y; s += a1.z * a1.z; s += a1.w * a1.w;
    s = wave_reduce_sum(s);                                          // a butterfly: the same bits in every lane
    float n = sqrtf(s);
    n = n < 1e-12f ? 1e-12f : n;                                     // a NaN stays a NaN
    acc[0] += describe_q(a0.x, n); acc[1] += describe_q(a0.y, n); acc[2] += describe_q(a0.z, n); acc[3] += describe_q(a0.w, n);
    acc[4] += describe_q(a1.x, n); acc[5] += describe_q(a1.y, n); acc[6] += describe_q(a1.z, n); acc[7] += describe_q(a1.w, n);
    ++run;
    if (!more) break;
    const int next = __shfl(slot, jn, 64);
    if (next != cur) {                                               // wave-uniform: the run ends here
      describe_flush(sum_q, cells, cur, lane, acc, run);
      cur = next;
    }
    a0 = b0; a1 = b1;
  }
  describe_flush(sum_q, cells, cur, lane, acc, run);
}

// sum over the workgroup in a fixed order (the waves' butterflies, then the waves in ascending order), in every thread
__device__ __forceinline__ double describe_block_sum(double v, double* red_s) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  if ((threadIdx.x & 63) == 0) red_s[threadIdx.x >> 6] = v;
  __syncthreads();
  double t = red_s[0];
  for (int w = 1; w < (int)(blockDim.x >> 6); ++w) t += red_s[w];
  __syncthreads();
  return t;
}

__global__ __launch_bounds__(DS_FIN_THREADS) void describe_finish_kernel(const i64* __restrict__ sum_q, const int* __restrict__ cells,
                                                                         float* __restrict__ embedding, float* __restrict__ coherence) {
  __shared__ double red_s[DS_FIN_THREADS / 64];
  const int k = blockIdx.x, tid = threadIdx.x;
  const int n = cells[k];
  double m0 = 0.0, m1 = 0.0;
  if (n > 0) {                                                       // uniform over the workgroup; n * 2^30 is exact
    m0 = (double)sum_q[(size_t)k * DS_D + tid] / ((double)n * 1073741824.0);
    m1 = (double)sum_q[(size_t)k * DS_D + DS_FIN_THREADS + tid] / ((double)n * 1073741824.0);
  }
  const double norm = sqrt(describe_block_sum(m0 * m0 + m1 * m1, red_s));
  const bool empty = !(norm > 0.0);
  embedding[(size_t)k * DS_D + tid] = empty ? 0.0f : (float)(m0 / norm);
  embedding[(size_t)k * DS_D + DS_FIN_THREADS + tid] = empty ? 0.0f : (float)(m1 / norm);
  if (tid == 0) coherence[k] = empty ? 0.0f : (float)norm;
}

__device__ __forceinline__ float describe_block_sum_f32(float v, float* red_s) {
  v = wave_reduce_sum(v);
  if ((threadIdx.x & 63) == 0) red_s[threadIdx.x >> 6] = v;
  __syncthreads();
  float t = red_s[0];
  for (int w = 1; w < (int)(blockDim.x >> 6); ++w) t += red_s[w];
  __syncthreads();
  return t;
}

__global__ __launch_bounds__(DS_CLS_THREADS) void describe_classify_kernel(const float* __restrict__ embedding, const float* __restrict__ zs,
                                                                            int C1, int topn, float* __restrict__ prob,
                                                                            int* __restrict__ top_cls, float* __restrict__ top_prob) {
  __shared__ float emb_s[DS_D];
  __shared__ float red_s[DS_CLS_THREADS / 64];
  __shared__ u64 key_s[DS_CLS_THREADS / 64];
  __shared__ int any_s;
  const int k = blockIdx.x, tid = threadIdx.x, C = C1 - 1;
  if (tid == 0) any_s = 0;
  __syncthreads();
  if (tid < DS_D) {
    const float e = embedding[(size_t)k * DS_D + tid];
    emb_s[tid] = e;
    if (e != 0.0f) atomicOr(&any_s, 1);                              // +0 and -0 are zero; a NaN is not
  }
  __syncthreads();
  const int c0 = tid, c1 = tid + DS_CLS_THREADS;
  const bool in0 = c0 < C, in1 = c1 < C;                             // the background column C never enters
  if (!any_s) {                                                      // an empty slot; uniform over the workgroup
    if (in0) prob[(size_t)k * C + c0] = 0.0f;
    if (in1) prob[(size_t)k * C + c1] = 0.0f;
    if (tid < topn) {
      top_cls[k * topn + tid] = -1;
      top_prob[k * topn + tid] = 0.0f;
    }
    return;
  }
  float l0 = 0.0f, l1 = 0.0f;
  const float* z0 = zs + (in0 ? c0 : 0);                             // a thread without a class reads column 0 and drops it
  const float* z1 = zs + (in1 ? c1 : 0);
#pragma unroll 8
  for (int ch = 0; ch < DS_D; ++ch) {
    const float e = emb_s[ch];
    l0 = fmaf(e, z0[(size_t)ch * C1], l0);
    l1 = fmaf(e, z1[(size_t)ch * C1], l1);
  }
  l0 *= 50.0f;
  l1 *= 50.0f;
  const float ninf = -INFINITY;
  float mx = fmaxf(in0 ? l0 : ninf, in1 ? l1 : ninf);
  mx = wave_reduce_max(mx);
  if ((tid & 63) == 0) red_s[tid >> 6] = mx;
  __syncthreads();
  mx = red_s[0];
  for (int w = 1; w < DS_CLS_THREADS / 64; ++w) mx = fmaxf(mx, red_s[w]);
  __syncthreads();
  const float e0 = in0 ? expf(l0 - mx) : 0.0f, e1 = in1 ? expf(l1 - mx) : 0.0f;
  const float sum = describe_block_sum_f32(e0 + e1, red_s);
  const float p0 = e0 / sum, p1 = e1 / sum;
  if (in0) prob[(size_t)k * C + c0] = p0;
  if (in1) prob[(size_t)k * C + c1] = p1;
  // topn rounds: the largest key among the classes not taken yet; a class's key is nonzero (~class != 0)
  u64 k0 = in0 ? ((u64)__float_as_uint(p0) << 32) | (unsigned)~c0 : 0ull;
  u64 k1 = in1 ? ((u64)__float_as_uint(p1) << 32) | (unsigned)~c1 : 0ull;
  for (int r = 0; r < topn; ++r) {
    const u64 best = block_max_u64(k0 > k1 ? k0 : k1, key_s);       // topn <= C: there is one
    if (k0 == best) k0 = 0ull;
    if (k1 == best) k1 = 0ull;
    if (tid == 0) {
      top_cls[k * topn + r] = (int)~(unsigned)best;
      top_prob[k * topn + r] = __uint_as_float((unsigned)(best >> 32));
    }
  }
}

inline bool describe_aligned(const void* p, unsigned a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1u)) == 0; }

}  // namespace

extern "C" int eod_describe_pool(const float* mem, const int32_t* object_labels, const int32_t* objects, int N, int K, int64_t* sum_q,
                                 int32_t* cells, float* embedding, float* coherence, eod_stream_t stream) {
  if (K < 1 || K > EOD_DESCRIBE_K_MAX || N < 1 || N > EOD_DESCRIBE_N_MAX) return EOD_ERR_BAD_DIMS;
  if (!mem || !object_labels || !objects || !sum_q || !cells || !embedding || !coherence) return EOD_ERR_NULL;
  if (!describe_aligned(mem, 16) || !describe_aligned(object_labels, 4) || !describe_aligned(objects, 4) || !describe_aligned(sum_q, 8) ||
      !describe_aligned(cells, 4) || !describe_aligned(embedding, 16) || !describe_aligned(coherence, 4))
    return EOD_ERR_ALIGN;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(describe_init_kernel, dim3((K * DS_D + 255) / 256), dim3(256), 0, s, K, reinterpret_cast<u64*>(sum_q), (int*)cells);
  hipLaunchKernelGGL(describe_pool_kernel, dim3((N + DS_WG_CELLS - 1) / DS_WG_CELLS), dim3(DS_POOL_THREADS), 0, s, mem,
                     (const int*)object_labels, (const int*)objects, N, K, reinterpret_cast<u64*>(sum_q), (int*)cells);
  hipLaunchKernelGGL(describe_finish_kernel, dim3(K), dim3(DS_FIN_THREADS), 0, s, reinterpret_cast<const i64*>(sum_q), (const int*)cells,
                     embedding, coherence);
  return eod_launch_status();
}

extern "C" int eod_describe_classify(const float* embedding, const float* zs, int K, int C1, int topn, float* prob, int32_t* top_cls,
                                     float* top_prob, eod_stream_t stream) {
  const long long C = (long long)C1 - 1;
  if (K < 1 || K > EOD_DESCRIBE_K_MAX || C < 1 || C > EOD_DESCRIBE_C_MAX || topn < 1 || topn > EOD_DESCRIBE_TOPN_MAX || topn > C)
    return EOD_ERR_BAD_DIMS;
  if (!embedding || !zs || !prob || !top_cls || !top_prob) return EOD_ERR_NULL;
  if (!describe_aligned(embedding, 16) || !describe_aligned(zs, 4) || !describe_aligned(prob, 4) || !describe_aligned(top_cls, 4) ||
      !describe_aligned(top_prob, 4))
    return EOD_ERR_ALIGN;
  hipLaunchKernelGGL(describe_classify_kernel, dim3(K), dim3(DS_CLS_THREADS), 0, (hipStream_t)stream, embedding, zs, C1, topn, prob,
                     (int*)top_cls, top_prob);
  return eod_launch_status();
}
