// The steps the weight-gradient kernels share (conv_wgrad.hip, and proj_backward_weights_kernel of memory_backward.hip).  Every one of
// them computes dW[co][k] = sum over positions of G[pos][co] * X[pos -> input pixel][k] and db[co] = sum over positions of G[pos][co]
// with the position as the contraction index, in one of two schemes:
//   direct  -- no LDS staging: v_mfma_f32_32x32x2_f32's operand layout (lane l supplies row l % 32, k = l / 32) reads 32 consecutive
//              channels of one position per half wave.  A workgroup's four waves take a quarter of its positions each, in k-steps of 8
//              positions, and are added in wave order through LDS.
//   staged  -- a workgroup of 2 x 2 waves walks its positions in chunks that 16 loader rows of 16 threads stage in LDS.
// Either way a launch may cut the positions into `splits` contiguous ranges (blockIdx.z); range z then writes partial results
// part [output][z][n] / bpart [output][z][Cout], and wgrad_reduce_ranges adds them in range order.  Everything is added in a fixed
// order: the results are deterministic.
// A is the kernel's argument struct.  Every helper reads splits / part / bpart of it, the address helpers its geometry as well.  All are
// force-inlined and only READ the struct (a helper that wrote a field would make the compiler keep a private copy of it in scratch,
// which the build refuses); results come back in out-parameters, not in structs.
#pragma once
#include "eod_common.h"

// ---- 1. the positions of a workgroup and of a wave -----------------------------------------------------------
// Direct scheme: k-steps [s_begin, s_end) of wave `wave`: the range's steps, a contiguous quarter each.
template <class A>
__device__ __forceinline__ void wgrad_wave_steps(const A& a, int P, int wave, int& s_begin, int& s_end) {
  const int steps = (P + 7) / 8;
  const int sps = (steps + a.splits - 1) / a.splits;           // steps of a range
  const int z_begin = (int)blockIdx.z * sps;
  const int z_end = min(z_begin + sps, steps);
  const int spw = (sps + 3) / 4;
  s_begin = z_begin + wave * spw;
  s_end = min(s_begin + spw, z_end);
}

// Staged scheme: chunks [c_begin, c_end) of PK positions of the workgroup's range (empty for the last ranges of a short layer).
template <int PK, class A>
__device__ __forceinline__ void wgrad_chunk_range(const A& a, int P, int& c_begin, int& c_end) {
  const int chunks = (P + PK - 1) / PK;
  const int cps = (chunks + a.splits - 1) / a.splits;
  c_begin = (int)blockIdx.z * cps;
  c_end = min(c_begin + cps, chunks);
}

// ---- 2. position -> input pixel ------------------------------------------------------------------------------
// Image mode: output position pos = (n, oy, ox) under tap (ky, kx); false when the tap falls on the padding (`pixel` is then
// meaningless).  `pixel` counts NHWC rows of x: the operand is x[pixel * Cin + channel].
template <class A>
__device__ __forceinline__ bool wgrad_input_pixel(const A& a, int pos, int ky, int kx, size_t& pixel) {
  const int row = (int)fdiv((unsigned)pos, a.div_w);           // n * OH + oy
  const int ox = pos - row * a.OW;
  const int n = (int)fdiv((unsigned)row, a.div_h);
  const int oy = row - n * a.OH;
  const int iy = oy * a.stride + ky - a.pad, ix = ox * a.stride + kx - a.pad;
  pixel = (size_t)(n * a.H + iy) * a.W + ix;
  return (unsigned)iy < (unsigned)a.H && (unsigned)ix < (unsigned)a.W;
}

// Pyramid mode (stride 1, 'same' padding): rows [lv_off[l], lv_off[l + 1]) of the row list are an lv_h[l] x lv_w[l] image.
template <int MAX_LEVELS, class A>
__device__ __forceinline__ bool wgrad_level_pixel(const A& a, int pos, int ky, int kx, size_t& pixel) {
  int l = 0;
#pragma unroll
  for (int q = 1; q < MAX_LEVELS; ++q) l += (q < a.nlv && pos >= a.lv_off[q]) ? 1 : 0;
  const int base = a.lv_off[l], lw = a.lv_w[l], lh = a.lv_h[l];
  const int local = pos - base;
  const int oy = local / lw, ox = local - oy * lw;
  const int iy = oy + ky - a.pad, ix = ox + kx - a.pad;
  pixel = (size_t)base + (size_t)iy * lw + ix;
  return (unsigned)iy < (unsigned)lh && (unsigned)ix < (unsigned)lw;
}

// ---- 3. where a workgroup writes -----------------------------------------------------------------------------
// The real outputs, or with ranges the partial buffers of slot (output * splits + blockIdx.z); n = elements of one dW.
template <class A>
__device__ __forceinline__ void wgrad_outputs(const A& a, size_t slot, size_t n, int Cout, float* dw_final, float* db_final, float*& dw,
                                              float*& db) {
  dw = a.splits > 1 ? a.part + slot * n : dw_final;
  db = a.splits > 1 ? a.bpart + slot * Cout : db_final;
}

// ---- 4. direct scheme: four waves' results become one -----------------------------------------------------------
// Waves 1..3 hand their 32 x 32 accumulators to wave 0 through red [3 * 16 * 64]; wave 0 adds them to its own in wave order and gets
// true.  Contains one barrier; the caller separates two uses of `red` by another.
__device__ __forceinline__ bool wgrad_reduce_waves(float* red, f32x16& acc, int wave, int lane) {
  if (wave > 0) {
#pragma unroll
    for (int r = 0; r < 16; ++r) red[((wave - 1) * 16 + r) * 64 + lane] = acc[r];
  }
  __syncthreads();
  if (wave != 0) return false;
#pragma unroll
  for (int w = 1; w < 4; ++w)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] += red[((w - 1) * 16 + r) * 64 + lane];
  return true;
}

// C/D layout of the 32 x 32 MFMA: the lane holds column lane & 31 of rows (r & 3) + 8 (r >> 2) + 4 (lane >> 5).  dst = the element
// (row 0, this lane's column) of the destination, rows `pitch` apart.
__device__ __forceinline__ void wgrad_store_tile(const f32x16& v, int lane, float* dst, size_t pitch, float scale) {
#pragma unroll
  for (int r = 0; r < 16; ++r) dst[(size_t)((r & 3) + 8 * (r >> 2) + 4 * (lane >> 5)) * pitch] = v[r] * scale;
}

// db of the direct scheme: every lane leaves the sum of its G values in bred [4 * 64] BEFORE the barrier of wgrad_reduce_waves; after
// it, lane < 32 reads channel `lane`: even + odd positions, wave order.
__device__ __forceinline__ void wgrad_bias_put(float* bred, int wave, int lane, float bsum) { bred[wave * 64 + lane] = bsum; }
__device__ __forceinline__ float wgrad_bias_sum(const float* bred, int lane) {
  float v = 0.f;
#pragma unroll
  for (int w = 0; w < 4; ++w) v += bred[w * 64 + lane] + bred[w * 64 + 32 + lane];
  return v;
}

// The whole 32 x 32 tile of the direct scheme.  fetch(pos, gv, xv) supplies this lane's G and X value of a position < P (preset
// to 0: the X value stays 0 on the padding).  where(dst, db_tile) is asked on wave 0 once the sum is there: dst as in
// wgrad_store_tile (null: the lane's column is dropped), db_tile non-null: the tile also writes the G sums of its 32 rows there.
// Both results are multiplied by scale.
template <class A, class Fetch, class Where>
__device__ __forceinline__ void wgrad_direct_tile(const A& a, int P, Fetch fetch, Where where, size_t pitch, float scale) {
  __shared__ float red[3 * 16 * 64];
  __shared__ float bred[4 * 64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int kh = lane >> 5;
  int s_begin, s_end;
  wgrad_wave_steps(a, P, wave, s_begin, s_end);
  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;
  float bsum = 0.f;
  for (int s = s_begin; s < s_end; ++s) {
    float av[4], bv[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const int pos = s * 8 + 2 * t + kh;            // instruction t contracts positions 8 s + 2 t and 8 s + 2 t + 1
      float gv = 0.f, xv = 0.f;
      if (pos < P) fetch(pos, gv, xv);
      av[t] = gv;
      bv[t] = xv;
    }
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av[t], bv[t], acc, 0, 0, 0);
      bsum += av[t];
    }
  }
  wgrad_bias_put(bred, wave, lane, bsum);
  if (!wgrad_reduce_waves(red, acc, wave, lane)) return;
  float *dst, *db_tile;
  where(dst, db_tile);
  if (dst) wgrad_store_tile(acc, lane, dst, pitch, scale);
  if (db_tile && lane < 32) db_tile[lane] = wgrad_bias_sum(bred, lane) * scale;
}

// ---- 5. staged scheme: db --------------------------------------------------------------------------------------
// Loader row lp holds in bsum the sums of its positions for channels c4 .. c4 + 3 of the tile; the 16 rows are added in row order.
// Called by the whole workgroup (one barrier).
__device__ __forceinline__ void wgrad_bias_rows(float (*bred)[64], int lp, int c4, const f32x4& bsum, int co0, int Cout, float* db) {
  bred[lp][c4 + 0] = bsum.x; bred[lp][c4 + 1] = bsum.y; bred[lp][c4 + 2] = bsum.z; bred[lp][c4 + 3] = bsum.w;
  __syncthreads();
  const int tid = threadIdx.x;
  if (tid < 64 && co0 + tid < Cout) {
    float v = 0.f;
#pragma unroll
    for (int q = 0; q < 16; ++q) v += bred[q][tid];
    db[co0 + tid] = v;
  }
}

// ---- 6. host side ----------------------------------------------------------------------------------------------
// Workspace of a launch with `splits` ranges and `outputs` results of n + Cout floats each (0: no ranges, no workspace).
static inline size_t wgrad_workspace_bytes(int splits, int outputs, size_t n, int Cout) {
  return splits > 1 ? (size_t)outputs * splits * (n + Cout) * sizeof(float) : 0;
}

// dw[o] / db[o] (db[o] may be null) = the partial results of the ranges, added in range order (conv_wgrad.hip)
__attribute__((visibility("hidden"))) void wgrad_reduce_ranges(const float* part, const float* bpart, int splits, int outputs, size_t n,
                                                               int Cout, float* const* dw, float* const* db, hipStream_t stream);

// One weight-gradient launch: with a workspace the positions are cut into `splits` ranges (a.splits / part / bpart are set here,
// a.splits = 1 otherwise), launch() starts the kernel over (.., .., a.splits), then the ranges are reduced into dw / db.
template <class A, class Launch>
static inline int wgrad_launch_ranges(A& a, int splits, void* workspace, size_t workspace_bytes, int outputs, size_t n, int Cout,
                                      float* const* dw, float* const* db, hipStream_t stream, Launch launch) {
  a.splits = 1;
  if (workspace && splits > 1) {
    if (wgrad_workspace_bytes(splits, outputs, n, Cout) > workspace_bytes) return EOD_ERR_CAPACITY;
    a.splits = splits;
    a.part = static_cast<float*>(workspace);
    a.bpart = a.part + (size_t)outputs * splits * n;
  }
  launch();
  if (a.splits > 1) wgrad_reduce_ranges(a.part, a.bpart, a.splits, outputs, n, Cout, dw, db, stream);
  return eod_launch_status();
}
