// a20: explicit semantic map from the implicit memory (custom_rcnn.py:745-756, 938-1017); evaluated lazily.
//
// Two forms of one entry point (eod_semmap_labels):
//   plain               semmap_cell_kernel: one wave per cell walks the classes one by one.  The reference's 20-class map.
//   EOD_SEMMAP_SCORES   semmap_query_kernel: the same product as a [n_cells, 512] x [512, C1-1] GEMM on the fp32 matrix cores
//                       (v_mfma_f32_32x32x2_f32, exact fp32) with the row normalisation fused in front and an online
//                       softmax / argmax behind; any vocabulary the heads accept (C1 <= 2048), label and confidence per cell.
// Both share the row prologue (semmap_row_prologue) and semmap_threshold_kernel, so a cell's intensity, and with it the set of
// cells labelled -1, is the same bits in both.
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

__global__ __launch_bounds__(SQ_WAVES * 64) void semmap_query_kernel(const float* __restrict__ mem, const float* __restrict__ obs,
                                                                      const float* __restrict__ zs, int n_cells, int C1,
                                                                      float* __restrict__ intensity, int* __restrict__ labels,
                                                                      float* __restrict__ scores, unsigned* __restrict__ minmax) {
  __shared__ f32x4 As[64 * 2 * 64];                   // [g][rt][lane] float4: 128 KB
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
  if (wave < panels) load_b(b0, wave, 0);
  for (int panel = wave; panel < panels; panel += SQ_WAVES) {
    f32x16 acc[2];
#pragma unroll
    for (int q = 0; q < 16; ++q) acc[0][q] = acc[1][q] = 0.f;
    for (int g0 = 0; g0 < 64; g0 += 2 * SQ_CHUNK) {
      load_b(b1, panel, g0 + SQ_CHUNK);
      mma_chunk(b0, g0, acc[0], acc[1]);
      if (g0 + 2 * SQ_CHUNK < 64)
        load_b(b0, panel, g0 + 2 * SQ_CHUNK);
      else if (panel + SQ_WAVES < panels)
        load_b(b0, panel + SQ_WAVES, 0);
      mma_chunk(b1, g0 + SQ_CHUNK, acc[0], acc[1]);
    }
    const int c = panel * 32 + (lane & 31);
    if (c < C) {
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
    scores[row0 + tid] = 1.0f / v.s;
  }
}

inline bool aligned4(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3u) == 0; }

}  // namespace

extern "C" int eod_semmap_labels(const float* mem, const float* obs, const float* zs, int n_cells, int D, int C1, float thresh,
                                 int32_t* labels, float* workspace, eod_stream_t stream) {
  if (!mem || !obs || !zs || !labels || !workspace) return EOD_ERR_NULL;
  const bool query = (D & EOD_SEMMAP_SCORES) != 0;
  if (query) D &= ~EOD_SEMMAP_SCORES;
  if (n_cells <= 0 || D != 512 || C1 < 2) return EOD_ERR_BAD_DIMS;
  if (query) {
    if (C1 > 2048) return EOD_ERR_CAPACITY;
    if (!aligned4(mem) || !aligned4(obs) || !aligned4(zs) || !aligned4(labels) || !aligned4(workspace)) return EOD_ERR_ALIGN;
  }
  hipStream_t s = (hipStream_t)stream;
  unsigned* minmax = reinterpret_cast<unsigned*>(workspace);
  float* intensity = workspace + 4;
  static const unsigned init[2] = {0x7F800000u, 0u};   // +inf, 0 (static: outlives the async copy)
  if (hipMemcpyAsync(minmax, init, sizeof(init), hipMemcpyHostToDevice, s) != hipSuccess) return EOD_ERR_LAUNCH;
  if (query) {
    // one workgroup per 64 cells, every one resident work for the whole class matrix: no grid cap, no tile loop
    hipLaunchKernelGGL(semmap_query_kernel, dim3((n_cells - 1) / SQ_ROWS + 1), dim3(SQ_WAVES * 64), 0, s, mem, obs, zs, n_cells, C1,
                       intensity, labels, intensity + n_cells, minmax);
  } else {
    int blocks = (n_cells + 3) / 4;
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(semmap_cell_kernel, dim3(blocks), dim3(256), 0, s, mem, obs, zs, n_cells, D, C1, intensity, labels, minmax);
  }
  hipLaunchKernelGGL(semmap_threshold_kernel, dim3((n_cells + 255) / 256 > 1024 ? 1024 : (n_cells + 255) / 256), dim3(256), 0, s, intensity,
                     minmax, n_cells, thresh, labels);
  return eod_launch_status();
}
