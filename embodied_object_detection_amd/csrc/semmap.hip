// a20: explicit semantic map from the implicit memory (custom_rcnn.py:745-756, 938-1017); evaluated lazily.
//
// Four forms of one entry point (eod_semmap_labels):
//   plain               semmap_cell_kernel: one wave per cell walks the classes one by one.  The reference's 20-class map.
//   EOD_SEMMAP_SCORES   semmap_query_kernel: the same product as a [n_cells, 512] x [512, C1-1] GEMM on the fp32 matrix cores
//                       (v_mfma_f32_32x32x2_f32, exact fp32) with the row normalisation fused in front and an online
//                       softmax / argmax behind; any vocabulary the heads accept (C1 <= 2048), label and confidence per cell.
//   EOD_SEMMAP_LOCATE   the SCORES form with one gathered panel more (semmap_query_kernel<true>): the probability maps of up to 32
//                       queried classes, prob[Q][n_cells], zeroed below the threshold by semmap_threshold_locate_kernel.
//   EOD_SEMMAP_PEAKS    a second call on the same workspace: the K best local maxima of each map (semmap_peak_flag_kernel,
//                       semmap_peak_select_kernel).  How Q, K, radius and the grid's columns travel: include/eod_hip.h.
// All share the row prologue (semmap_row_prologue) and the threshold rule, so a cell's intensity, and with it the set of cells
// labelled -1, is the same bits in each.
#include "eod_common.h"
#include "../../include/eod_hip.h"

namespace {

// One wave, one cell: the lane's 8 channels q*64 + lane into x, the row's L2 denominator returned in every lane; lane 0 writes the
// cell's observation intensity mean|mem| (/obs if obs > 1) and gets its bit pattern in `inten_bits` for the map's min/max
// (non-negative floats order like their bit patterns; the caller enters it, per cell or per workgroup: a minimum and a maximum do
// not depend on how they are grouped).
__device__ __forceinline__ float semmap_row_prologue(const float* __restrict__ mem, const float* __restrict__ obs, int cell, int D, int lane,
                                                     float (&x)[8], float* __restrict__ intensity, unsigned& inten_bits) {
  float ss = 0.f, sa = 0.f;
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    x[q] = mem[(size_t)cell * D + q * 64 + lane];
    ss += x[q] * x[q];
    sa += fabsf(x[q]);
  }
  ss = wave_reduce_sum(ss);
  sa = wave_reduce_sum(sa);
  const float denom = fmaxf(sqrtf(ss), 1e-12f);
  if (lane == 0) {
    float inten = sa / (float)D;
    const float o = obs[cell];
    if (o > 1.0f) inten = inten / o;
    intensity[cell] = inten;
    inten_bits = __float_as_uint(inten);
  }
  return denom;
}

// one wave per cell: label = argmax_c<C of (temp * mem/|mem|) . zs[:,c] (softmax is monotonic), intensity = mean|mem| (/obs if obs>1)
__global__ __launch_bounds__(256) void semmap_cell_kernel(const float* __restrict__ mem, const float* __restrict__ obs,
                                                           const float* __restrict__ zs, int n_cells, int D, int C1,
                                                           float* __restrict__ intensity, int* __restrict__ labels,
                                                           unsigned* __restrict__ minmax) {
  const int lane = threadIdx.x & 63;
  const int wpb = blockDim.x >> 6;
  for (int cell = blockIdx.x * wpb + (threadIdx.x >> 6); cell < n_cells; cell += gridDim.x * wpb) {
    float x[8];
    unsigned bits = 0u;
    const float denom = semmap_row_prologue(mem, obs, cell, D, lane, x, intensity, bits);
    if (lane == 0) {
      atomicMin(minmax + 0, bits);
      atomicMax(minmax + 1, bits);
    }
    float best = -INFINITY;
    int besti = 0;
    for (int c = 0; c < C1 - 1; ++c) {
      float s = 0.f;
#pragma unroll
      for (int q = 0; q < 8; ++q) s += (50.0f * (x[q] / denom)) * zs[(size_t)(q * 64 + lane) * C1 + c];
      s = wave_reduce_sum(s);
      if (s > best) {
        best = s;
        besti = c;
      }
    }
    if (lane == 0) labels[cell] = besti;
  }
}

__global__ __launch_bounds__(256) void semmap_threshold_kernel(const float* __restrict__ intensity, const unsigned* __restrict__ minmax,
                                                                int n_cells, float thresh, int* __restrict__ labels) {
  const float lo = __uint_as_float(minmax[0]), hi = __uint_as_float(minmax[1]);
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n_cells; i += gridDim.x * blockDim.x) {
    const float v = (intensity[i] - lo) / (hi - lo);   // NaN when hi == lo: nothing is thresholded (reference quirk, :751)
    if (v < thresh) labels[i] = -1;
  }
}

// ------------------------------------------------------------------------------------------------------
// EOD_SEMMAP_SCORES: label and softmax confidence per cell, any vocabulary, on the fp32 matrix cores
// ------------------------------------------------------------------------------------------------------
// A workgroup of eight waves owns 64 rows (cells) for the whole of K = 512: the prologue normalises them (one wave per row, the plain
// kernel's arithmetic) and leaves 50 * x / |x| in LDS, 128 KB, in the order the matrix cores read it.  The class panels of 32 columns
// then stream past the resident rows: wave w takes panels w, w + 8, ...; for a panel it runs both 32-row tiles against one B operand
// (two accumulators, 2 x 256 MFMAs), the B element of lane l at step k being zs[k][panel * 32 + (l & 31)] as the matrix lies (32
// consecutive floats of a channel row, from L2: the whole matrix is at most 4 MB).  The B loads of the next 16 channels are in flight
// while the current 16 multiply.
//
// A in LDS: the value of row r = 32 rt + i at channel k = 8 g + 2 j + h sits at float4 slot (2 g + rt) * 64 + 32 h + i, component j.
// Lane l = 32 h + i of a wave reads slot (2 g + rt) * 64 + l: one conflict-free ds_read_b128 feeds four MFMA steps.
//
// The score matrix never exists.  A lane keeps, for each of its 32 accumulator slots (a row of the tile), the running
// (max, sum of exp(l - max), argmax) over the columns it has seen, one column per panel in ascending order; a column that raises the
// maximum rescales the sum.  Columns >= C1 - 1 (the background column, the tail of the last panel) never enter.  At the end the 32
// lanes that share a row are combined by a butterfly and the eight waves in wave order, always as (state with the larger maximum,
// ties: the lower class index) + rescaled other: the result does not depend on which side a state arrives from, and the tie rule is
// the lowest class index at every level.
constexpr int SQ_ROWS = 64;          // rows per workgroup
constexpr int SQ_WAVES = 8;
constexpr int SQ_CHUNK = 2;          // channel groups (of 8 channels) per B register buffer
constexpr int SQ_EMPTY = 0x7fffffff;

struct SoftArg {
  float m, s;
  int a;
};

// (m, s, a) of the union of two column sets
__device__ __forceinline__ SoftArg softarg_combine(const SoftArg& p, const SoftArg& q) {
  const bool p_hi = p.m > q.m || (p.m == q.m && p.a <= q.a);
  const SoftArg hi = p_hi ? p : q, lo = p_hi ? q : p;
  const float e = (lo.m == -INFINITY) ? 0.f : __expf(lo.m - hi.m);
  return SoftArg{hi.m, hi.s + lo.s * e, hi.a};
}

//
// LOCATE (EOD_SEMMAP_LOCATE): one more panel joins the stream as panel number `panels`, on the wave whose turn it is.  Its B operand
// is gathered: lane l multiplies column qidx[l & 31] (clamped into [0, C1 - 2]; lanes >= Q repeat query 0 and are not written out).
// It runs the loop body of every other panel, so a queried logit is the bits the main pass saw for that column; it stays out of the
// online softmax and leaves its 64 x 32 logits in LDS.  Once the rows' (m, s) are final, all eight waves turn them into
// prob[q][cell] = exp(l - m) * (1 / s), 64 consecutive cells per queried class: where the class is the row's argmax, l == m and the
// value is the row's score, bit for bit.
constexpr int SQ_QMAX = 32;          // queried classes per call: one panel
constexpr int SQ_QLD = SQ_ROWS + 1;  // row stride of the queried logits in LDS: the 32 lanes of a store hit 32 banks

template <bool LOCATE>
__global__ __launch_bounds__(SQ_WAVES * 64) void semmap_query_kernel(const float* __restrict__ mem, const float* __restrict__ obs,
                                                                      const float* __restrict__ zs, int n_cells, int C1,
                                                                      float* __restrict__ intensity, int* __restrict__ labels,
                                                                      float* __restrict__ scores, unsigned* __restrict__ minmax,
                                                                      const int* __restrict__ qidx, int Q, float* __restrict__ prob) {
  __shared__ f32x4 As[64 * 2 * 64];                   // [g][rt][lane] float4: 128 KB
  __shared__ float qlog[LOCATE ? SQ_QMAX * SQ_QLD : 1];   // [query][row] logits of the gathered panel
  __shared__ float red_m[SQ_WAVES][SQ_ROWS];
  __shared__ float red_s[SQ_WAVES][SQ_ROWS];
  __shared__ int red_a[SQ_WAVES][SQ_ROWS];
  __shared__ unsigned wave_lo[SQ_WAVES], wave_hi[SQ_WAVES];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int row0 = blockIdx.x * SQ_ROWS;             // < n_cells by the launch
  // ---- prologue: rows wave * 8 .. wave * 8 + 7 of the tile; rows beyond n_cells are not read, hold zeros and stay out of the
  // min/max, which the workgroup enters once (40 000 cells entering one by one serialise on the two words: 1 ms)
  {
    float* Af = reinterpret_cast<float*>(As);
    unsigned lo = 0xFFFFFFFFu, hi = 0u;               // lane 0's
    for (int r8 = 0; r8 < SQ_ROWS / SQ_WAVES; ++r8) {
      const int r = wave * (SQ_ROWS / SQ_WAVES) + r8;
      const int cell = row0 + r;                      // wave-uniform
      float x[8];
      float denom = 1.0f;
      if (cell < n_cells) {
        unsigned bits = 0u;
        denom = semmap_row_prologue(mem, obs, cell, 512, lane, x, intensity, bits);
        lo = bits < lo ? bits : lo;
        hi = bits > hi ? bits : hi;
      } else {
#pragma unroll
        for (int q = 0; q < 8; ++q) x[q] = 0.f;
      }
      const int rt = r >> 5, i = r & 31;
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        const int g = q * 8 + (lane >> 3), j = (lane >> 1) & 3, h = lane & 1;      // channel k = q * 64 + lane
        Af[(((g * 2 + rt) * 64) + h * 32 + i) * 4 + j] = 50.0f * (x[q] / denom);
      }
    }
    if (lane == 0) {
      wave_lo[wave] = lo;
      wave_hi[wave] = hi;
    }
  }
  __syncthreads();
  if (tid == 0) {                                     // row0 < n_cells: wave 0 has seen at least one cell
    unsigned lo = wave_lo[0], hi = wave_hi[0];
#pragma unroll
    for (int w = 1; w < SQ_WAVES; ++w) {
      lo = wave_lo[w] < lo ? wave_lo[w] : lo;
      hi = wave_hi[w] > hi ? wave_hi[w] : hi;
    }
    atomicMin(minmax + 0, lo);
    atomicMax(minmax + 1, hi);
  }
  // ---- class panels
  const int C = C1 - 1;                               // columns that count
  const int panels = (C + 31) >> 5;
  const int h = lane >> 5;
  int qcol = 0;                                       // the lane's column of the gathered panel
  if constexpr (LOCATE) {
    qcol = qidx[(lane & 31) < Q ? (lane & 31) : 0];
    qcol = qcol < 0 ? 0 : (qcol > C1 - 2 ? C1 - 2 : qcol);
  }
  float sm[2][16], ssum[2][16];
  int sarg[2][16];
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      sm[t][q] = -INFINITY;
      ssum[t][q] = 0.f;
      sarg[t][q] = SQ_EMPTY;
    }
  // B registers of one chunk: channel 8 (g0 + gg) + 2 j + h at [gg * 4 + j]
  auto load_b = [&](float (&b)[SQ_CHUNK * 4], int panel, int g0) {
    int col = panel * 32 + (lane & 31);
    col = col < C1 ? col : C1 - 1;                    // stays inside the matrix; masked below
    if constexpr (LOCATE) col = panel == panels ? qcol : col;
    const float* zb = zs + (size_t)(8 * g0 + h) * C1 + col;
#pragma unroll
    for (int e = 0; e < SQ_CHUNK * 4; ++e) b[e] = zb[(size_t)(2 * e) * C1];
  };
  auto mma_chunk = [&](const float (&b)[SQ_CHUNK * 4], int g0, f32x16& acc0, f32x16& acc1) {
#pragma unroll
    for (int gg = 0; gg < SQ_CHUNK; ++gg) {
      const f32x4 a0 = As[((g0 + gg) * 2 + 0) * 64 + lane];
      const f32x4 a1 = As[((g0 + gg) * 2 + 1) * 64 + lane];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a0[j], b[gg * 4 + j], acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a1[j], b[gg * 4 + j], acc1, 0, 0, 0);
      }
    }
  };
  float b0[SQ_CHUNK * 4], b1[SQ_CHUNK * 4];
  const int streamed = panels + (LOCATE ? 1 : 0);
  if (wave < streamed) load_b(b0, wave, 0);
  for (int panel = wave; panel < streamed; panel += SQ_WAVES) {
    f32x16 acc[2];
#pragma unroll
    for (int q = 0; q < 16; ++q) acc[0][q] = acc[1][q] = 0.f;
    for (int g0 = 0; g0 < 64; g0 += 2 * SQ_CHUNK) {
      load_b(b1, panel, g0 + SQ_CHUNK);
      mma_chunk(b0, g0, acc[0], acc[1]);
      if (g0 + 2 * SQ_CHUNK < 64)
        load_b(b0, panel, g0 + 2 * SQ_CHUNK);
      else if (panel + SQ_WAVES < streamed)
        load_b(b0, panel + SQ_WAVES, 0);
      mma_chunk(b1, g0 + SQ_CHUNK, acc[0], acc[1]);
    }
    const int c = panel * 32 + (lane & 31);
    if (LOCATE && panel == panels) {                  // wave-uniform; C/D layout as below
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int q = 0; q < 16; ++q) qlog[(lane & 31) * SQ_QLD + t * 32 + (q & 3) + 8 * (q >> 2) + 4 * h] = acc[t][q];
    } else if (c < C) {
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int q = 0; q < 16; ++q) {
          const float l = acc[t][q];
          if (l > sm[t][q]) {                         // strictly: an equal later column keeps the earlier index
            ssum[t][q] = ssum[t][q] * __expf(sm[t][q] - l) + 1.0f;       // first column: 0 * exp(-inf) + 1
            sm[t][q] = l;
            sarg[t][q] = c;
          } else {
            ssum[t][q] += __expf(l - sm[t][q]);
          }
        }
    }
  }
  // ---- the 32 lanes of a row (C/D layout: column = lane & 31, row = (q & 3) + 8 (q >> 2) + 4 (lane >> 5)), then the waves
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      SoftArg v{sm[t][q], ssum[t][q], sarg[t][q]};
#pragma unroll
      for (int off = 1; off < 32; off <<= 1) {
        const SoftArg o{__shfl_xor(v.m, off, 64), __shfl_xor(v.s, off, 64), __shfl_xor(v.a, off, 64)};
        v = softarg_combine(v, o);
      }
      if ((lane & 31) == 0) {
        const int r = t * 32 + (q & 3) + 8 * (q >> 2) + 4 * h;
        red_m[wave][r] = v.m;
        red_s[wave][r] = v.s;
        red_a[wave][r] = v.a;
      }
    }
  __syncthreads();
  if (tid < SQ_ROWS && row0 + tid < n_cells) {
    SoftArg v{red_m[0][tid], red_s[0][tid], red_a[0][tid]};
#pragma unroll
    for (int w = 1; w < SQ_WAVES; ++w) v = softarg_combine(v, SoftArg{red_m[w][tid], red_s[w][tid], red_a[w][tid]});
    labels[row0 + tid] = v.a == SQ_EMPTY ? 0 : v.a;   // no finite logit (a NaN row): the plain kernel's answer
    const float score = 1.0f / v.s;
    scores[row0 + tid] = score;
    if constexpr (LOCATE) {                           // this thread alone reads column tid of red_*: wave 0's slots are free
      red_m[0][tid] = v.m;
      red_s[0][tid] = score;
    }
  }
  if constexpr (LOCATE) {
    __syncthreads();
    for (int e = tid; e < Q * SQ_ROWS; e += SQ_WAVES * 64) {
      const int q = e >> 6, r = e & (SQ_ROWS - 1);
      if (row0 + r < n_cells) prob[(size_t)q * n_cells + row0 + r] = __expf(qlog[q * SQ_QLD + r] - red_m[0][r]) * red_s[0][r];
    }
  }
}

// The threshold launch of the LOCATE call: a cell labelled -1 is 0 in the map of every queried class.
__global__ __launch_bounds__(256) void semmap_threshold_locate_kernel(const float* __restrict__ intensity, const unsigned* __restrict__ minmax,
                                                                       int n_cells, float thresh, int* __restrict__ labels, int Q,
                                                                       float* __restrict__ prob) {
  const float lo = __uint_as_float(minmax[0]), hi = __uint_as_float(minmax[1]);
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n_cells; i += gridDim.x * blockDim.x) {
    const float v = (intensity[i] - lo) / (hi - lo);   // as semmap_threshold_kernel
    if (v < thresh) {
      labels[i] = -1;
      for (int q = 0; q < Q; ++q) prob[(size_t)q * n_cells + i] = 0.f;
    }
  }
}

// ------------------------------------------------------------------------------------------------------
// EOD_SEMMAP_PEAKS: the K best local maxima of each queried class's map
// ------------------------------------------------------------------------------------------------------
// Cells are ordered by (prob descending, cell ascending); a peak is a positive cell that no other cell of its window precedes.
// semmap_peak_flag_kernel leaves cand[q][i] = prob[q][i] at peaks and 0 elsewhere; semmap_peak_select_kernel, one workgroup per
// class, takes the maximum of the order K times, each round among the candidates behind the previous pick.  The order as one
// 64-bit key: the positive float's bits above ~cell.  Comparisons only: no atomics, nothing depends on scheduling.
constexpr int SP_THREADS = 1024;

__global__ __launch_bounds__(256) void semmap_peak_flag_kernel(const float* __restrict__ prob, int n_cells, int cols, int radius,
                                                                float* __restrict__ cand) {
  const int rows = n_cells / cols;
  const float* p = prob + (size_t)blockIdx.y * n_cells;
  float* out = cand + (size_t)blockIdx.y * n_cells;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n_cells; i += gridDim.x * blockDim.x) {
    const float v = p[i];
    bool peak = v > 0.f;
    if (peak) {
      const int r = i / cols, c = i - r * cols;
      const int r0 = r - radius < 0 ? 0 : r - radius, r1 = r + radius > rows - 1 ? rows - 1 : r + radius;
      const int c0 = c - radius < 0 ? 0 : c - radius, c1 = c + radius > cols - 1 ? cols - 1 : c + radius;
      for (int rr = r0; rr <= r1; ++rr)
        for (int cc = c0; cc <= c1; ++cc) {
          const int j = rr * cols + cc;
          const float o = p[j];
          peak = peak && !(o > v || (o == v && j < i));
        }
    }
    out[i] = peak ? v : 0.f;
  }
}

__device__ __forceinline__ unsigned long long peak_key_max(unsigned long long a, unsigned long long b) { return a > b ? a : b; }

__global__ __launch_bounds__(SP_THREADS) void semmap_peak_select_kernel(const float* __restrict__ cand, int n_cells, int K,
                                                                         int* __restrict__ peaks, float* __restrict__ peak_scores) {
  __shared__ unsigned long long wave_best[SP_THREADS / 64];
  __shared__ unsigned long long picked;
  const float* p = cand + (size_t)blockIdx.x * n_cells;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  unsigned long long prev = ~0ull;                    // above every key
  for (int k = 0; k < K; ++k) {
    unsigned long long best = 0ull;                   // below every key: a candidate's float bits are non-zero
    for (int i = tid; i < n_cells; i += SP_THREADS) {
      const float v = p[i];
      if (v > 0.f) {
        const unsigned long long key = ((unsigned long long)__float_as_uint(v) << 32) | (unsigned)~i;
        if (key < prev) best = peak_key_max(best, key);
      }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const unsigned lo = __shfl_xor((unsigned)best, off, 64), hi = __shfl_xor((unsigned)(best >> 32), off, 64);
      best = peak_key_max(best, ((unsigned long long)hi << 32) | lo);
    }
    if (lane == 0) wave_best[wave] = best;
    __syncthreads();
    if (tid == 0) {
      unsigned long long b = wave_best[0];
      for (int w = 1; w < SP_THREADS / 64; ++w) b = peak_key_max(b, wave_best[w]);
      picked = b;
      peaks[blockIdx.x * K + k] = b ? (int)~(unsigned)b : -1;
      peak_scores[blockIdx.x * K + k] = b ? __uint_as_float((unsigned)(b >> 32)) : 0.f;
    }
    __syncthreads();
    prev = picked;                                    // 0 once the candidates are used up: no key is below it, the rest is padding
  }
}

inline bool aligned4(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3u) == 0; }

}  // namespace

extern "C" int eod_semmap_labels(const float* mem, const float* obs, const float* zs, int n_cells, int D, int C1, float thresh,
                                 int32_t* labels, float* workspace, eod_stream_t stream) {
  if (!mem || !obs || !zs || !labels || !workspace) return EOD_ERR_NULL;
  const bool locate = (D & EOD_SEMMAP_LOCATE) != 0, peaks = (D & EOD_SEMMAP_PEAKS) != 0;
  const bool query = (D & EOD_SEMMAP_SCORES) != 0 || locate;
  hipStream_t s = (hipStream_t)stream;
  int Q = 0;
  if (locate || peaks) {                               // the fields the two modes read; every other bit is checked with D below
    Q = (D >> EOD_SEMMAP_Q_SHIFT) & 0x3F;
    if (Q < 1 || Q > SQ_QMAX || (locate && peaks)) return EOD_ERR_BAD_DIMS;
    D &= ~(0x3F << EOD_SEMMAP_Q_SHIFT);
  }
  if (peaks) {                                         // the second call of a locate: C1 carries the grid's columns
    const int K = ((D >> EOD_SEMMAP_K_SHIFT) & 0xF) + 1, radius = (D >> EOD_SEMMAP_RADIUS_SHIFT) & 0x3, cols = C1;
    D &= ~(EOD_SEMMAP_PEAKS | (0xF << EOD_SEMMAP_K_SHIFT) | (0x3 << EOD_SEMMAP_RADIUS_SHIFT));
    if (n_cells <= 0 || D != 512 || cols < 1 || n_cells % cols != 0) return EOD_ERR_BAD_DIMS;
    if (!aligned4(workspace)) return EOD_ERR_ALIGN;
    float* prob = workspace + EOD_SEMMAP_LOCATE_PROB(n_cells);
    float* cand = prob + (size_t)Q * n_cells;
    int32_t* out = reinterpret_cast<int32_t*>(cand + (size_t)Q * n_cells);
    const int blocks = (n_cells + 255) / 256 > 1024 ? 1024 : (n_cells + 255) / 256;
    hipLaunchKernelGGL(semmap_peak_flag_kernel, dim3(blocks, Q), dim3(256), 0, s, prob, n_cells, cols, radius, cand);
    hipLaunchKernelGGL(semmap_peak_select_kernel, dim3(Q), dim3(SP_THREADS), 0, s, cand, n_cells, K, out,
                       reinterpret_cast<float*>(out + Q * K));
    return eod_launch_status();
  }
  D &= ~(EOD_SEMMAP_SCORES | EOD_SEMMAP_LOCATE);
  if (n_cells <= 0 || D != 512 || C1 < 2) return EOD_ERR_BAD_DIMS;
  if (query) {
    if (C1 > 2048) return EOD_ERR_CAPACITY;
    if (!aligned4(mem) || !aligned4(obs) || !aligned4(zs) || !aligned4(labels) || !aligned4(workspace)) return EOD_ERR_ALIGN;
  }
  unsigned* minmax = reinterpret_cast<unsigned*>(workspace);
  float* intensity = workspace + 4;
  static const unsigned init[2] = {0x7F800000u, 0u};   // +inf, 0 (static: outlives the async copy)
  if (hipMemcpyAsync(minmax, init, sizeof(init), hipMemcpyHostToDevice, s) != hipSuccess) return EOD_ERR_LAUNCH;
  const dim3 thr_grid((n_cells + 255) / 256 > 1024 ? 1024 : (n_cells + 255) / 256);
  if (locate) {
    const int* qidx = reinterpret_cast<const int*>(workspace + EOD_SEMMAP_LOCATE_QUERY(n_cells));
    float* prob = workspace + EOD_SEMMAP_LOCATE_PROB(n_cells);
    hipLaunchKernelGGL(semmap_query_kernel<true>, dim3((n_cells - 1) / SQ_ROWS + 1), dim3(SQ_WAVES * 64), 0, s, mem, obs, zs, n_cells, C1,
                       intensity, labels, intensity + n_cells, minmax, qidx, Q, prob);
    hipLaunchKernelGGL(semmap_threshold_locate_kernel, thr_grid, dim3(256), 0, s, intensity, minmax, n_cells, thresh, labels, Q, prob);
    return eod_launch_status();
  }
  if (query) {
    // one workgroup per 64 cells, every one resident work for the whole class matrix: no grid cap, no tile loop
    hipLaunchKernelGGL(semmap_query_kernel<false>, dim3((n_cells - 1) / SQ_ROWS + 1), dim3(SQ_WAVES * 64), 0, s, mem, obs, zs, n_cells, C1,
                       intensity, labels, intensity + n_cells, minmax, (const int*)nullptr, 0, (float*)nullptr);
  } else {
    int blocks = (n_cells + 3) / 4;
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(semmap_cell_kernel, dim3(blocks), dim3(256), 0, s, mem, obs, zs, n_cells, D, C1, intensity, labels, minmax);
  }
  hipLaunchKernelGGL(semmap_threshold_kernel, thr_grid, dim3(256), 0, s, intensity, minmax, n_cells, thresh, labels);
  return eod_launch_status();
}
