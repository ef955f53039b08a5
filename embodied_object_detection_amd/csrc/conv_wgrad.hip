// Backward of a convolution layer (FPN output convs timm.py:118-136, CenterNet tower centernet_head.py:141-161, mask head convs, the
// trunk: KH x KW taps, NHWC).  Weight gradient in the layout of the packed forward weights:
//   dW[co][(ky, kx, ci)] = sum over positions (n, oy, ox) of G[pos][co] * X[n][oy s + ky - pad][ox s + kx - pad][ci]      (0 outside the image)
//   db[co] = sum over positions of G[pos][co]
// The gradient with respect to the input of a stride-1 layer is a convolution of G with the 180-degree rotated, in/out-transposed
// weights: eod_conv2d (ops.ConvBackward); strided layers take conv_backward_input_kernel below.
//
// Which kernel runs (conv2d_backward_weights_impl):
//   staged<WgradStageF32>   LDS-tiled, fp32: every layer with 32-multiple channel counts; <.., true>: pyramid mode
//   staged<WgradStageF16>   the same frame in f16 arithmetic (EOD_WGRAD_F16, the AMP training step)
//   tap4_mfma               the 4-channel stem (KW <= 8)
//   tap4                    scalar fallback: 4 channels, kernel rows wider than 8 taps
//   rb / 32 x 32            direct scheme, 64 x 64 register block / one 32 x 32 tile: the EOD_WGRAD_LDS=0 / EOD_WGRAD_RB=0 fallbacks
// The position ranges, the position -> input pixel step, the partial buffers, the wave-order reduction and the db epilogues are in
// wgrad_common.h.
#include "wgrad_common.h"
#include "../../include/eod_hip.h"
#include <cstdlib>

namespace {

#define WGRAD_MAX_LEVELS 8
struct ConvBwdArgs {
  const float* x;   // [N,H,W,Cin]
  const float* g;   // [N,H,W,Cout]
  float* dw;        // [Cout][KH*KW*Cin]
  float* db;        // [Cout] or null
  int N, H, W, Cin, Cout, KH, KW, pad, stride, OH, OW;
  FastDiv div_w, div_h;     // by OW, OH
  // splits > 1 (blockIdx.z): the positions are cut into `splits` contiguous ranges, each writing its own partial dW / db into
  // part [splits][Cout * Ktot] / bpart [splits][Cout]; wgrad_reduce_kernel adds them in range order.  Layers with few channel tiles
  // and many positions (the trunk's first stages: 4 .. 64 workgroups otherwise) fill the chip this way.
  int splits;
  float* part;
  float* bpart;
  // pyramid mode of the LDS-tiled kernel (nlv > 0; stride 1, 'same' padding): x / g are row lists, rows [lv_off[l], lv_off[l+1])
  // are an lv_h[l] x lv_w[l] image, the weights are shared by the levels and dW / db are summed over all of them
  int nlv;
  int lv_off[WGRAD_MAX_LEVELS + 1], lv_h[WGRAD_MAX_LEVELS], lv_w[WGRAD_MAX_LEVELS];
};

// this range's dW / db (one output: slot = the range)
__device__ __forceinline__ void conv_wgrad_outputs(const ConvBwdArgs& a, int Ktot, float*& dw, float*& db) {
  wgrad_outputs(a, blockIdx.z, (size_t)a.Cout * Ktot, a.Cout, a.dw, a.db, dw, db);
}

// Direct scheme, one 32 (co) x 32 (ci) tile of one tap per workgroup (EOD_WGRAD_RB=0 and EOD_WGRAD_LDS=0).
__global__ __launch_bounds__(256) void conv_backward_weights_kernel(ConvBwdArgs a) {
  const int ci_tiles = a.Cin >> 5;
  const int tile = blockIdx.x;                       // (co tile, ci tile)
  const int co0 = (tile / ci_tiles) * 32, ci0 = (tile % ci_tiles) * 32;
  const int tap = blockIdx.y;
  const int ky = tap / a.KW, kx = tap - ky * a.KW;
  const int col = threadIdx.x & 31;
  const int Ktot = a.KH * a.KW * a.Cin;
  wgrad_direct_tile(
      a, a.N * a.OH * a.OW,            // positions of the OUTPUT grid
      [&](int pos, float& gv, float& xv) {
        gv = a.g[(size_t)pos * a.Cout + co0 + col];
        size_t pixel;
        if (wgrad_input_pixel(a, pos, ky, kx, pixel)) xv = a.x[pixel * a.Cin + ci0 + col];
      },
      [&](float*& dst, float*& db_tile) {
        float *dw, *db;
        conv_wgrad_outputs(a, Ktot, dw, db);
        dst = dw + (size_t)co0 * Ktot + (size_t)tap * a.Cin + ci0 + col;
        db_tile = a.db && tap == 0 && (tile % ci_tiles) == 0 ? db + co0 : nullptr;
      },
      Ktot, 1.f);
}

// The stem's weight gradient on the matrix cores (Cin = 4, KW * 4 <= 32): for one kernel row ky the packed columns (kx, ci) of an
// output position are KW * 4 CONSECUTIVE floats of the 4-channel image row, so a workgroup owns a 32 (co) x 32 (kx, ci) tile of one ky
// and contracts over the positions exactly like conv_backward_weights_kernel (columns >= KW * 4 are computed and dropped).
__global__ __launch_bounds__(256) void conv_backward_weights_tap4_mfma_kernel(ConvBwdArgs a) {
  const int tile = blockIdx.x;                       // (co tile, ky)
  const int co0 = (tile / a.KH) * 32, ky = tile % a.KH;
  const int col = threadIdx.x & 31;
  const int kx = col >> 2;
  const bool col_live = kx < a.KW;
  const int Ktot = a.KH * a.KW * 4;
  wgrad_direct_tile(
      a, a.N * a.OH * a.OW,
      [&](int pos, float& gv, float& xv) {
        gv = a.g[(size_t)pos * a.Cout + co0 + col];
        size_t pixel;
        const bool inside = wgrad_input_pixel(a, pos, ky, kx, pixel);
        if (col_live && inside) xv = a.x[pixel * 4 + (col & 3)];
      },
      [&](float*& dst, float*& db_tile) {
        float *dw, *db;
        conv_wgrad_outputs(a, Ktot, dw, db);
        dst = col_live ? dw + (size_t)co0 * Ktot + ky * a.KW * 4 + col : nullptr;
        db_tile = a.db && ky == 0 ? db + co0 : nullptr;
      },
      Ktot, 1.f);
}

// The direct contraction with a 64 (co) x 64 (ci) register block per wave (EOD_WGRAD_LDS=0).  The 32 x 32 form issues one MFMA per
// pair of operand loads and redoes the position arithmetic for every load: bound by instruction issue and by the L1 operand path, not
// by the matrix cores.  Here a k-step loads G for two 32-channel blocks and X for two, with ONE position computation, and feeds four
// MFMAs: half the loads and a quarter of the address arithmetic per FLOP.  A layer with 32 channels on one side (the 5-channel head
// padded to 32, bbox_pred.2) runs with the second block switched off.
__global__ __launch_bounds__(256) void conv_backward_weights_rb_kernel(ConvBwdArgs a) {
  const int ci_tiles = (a.Cin + 63) >> 6;
  const int tile = blockIdx.x;                       // (co tile, ci tile) of 64 x 64
  const int co0 = (tile / ci_tiles) * 64, ci0 = (tile % ci_tiles) * 64;
  const bool co2 = co0 + 32 < a.Cout, ci2 = ci0 + 32 < a.Cin;     // workgroup-uniform
  const int tap = blockIdx.y;
  const int ky = tap / a.KW, kx = tap - ky * a.KW;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int col = lane & 31, kh = lane >> 5;
  const int P = a.N * a.OH * a.OW;
  int s_begin, s_end;
  wgrad_wave_steps(a, P, wave, s_begin, s_end);
  f32x16 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
  float bsum0 = 0.f, bsum1 = 0.f;
  for (int s = s_begin; s < s_end; ++s) {
    float g0[4], g1[4], x0[4], x1[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const int pos = s * 8 + 2 * t + kh;            // instruction t contracts positions 8 s + 2 t and 8 s + 2 t + 1
      float ga = 0.f, gb = 0.f, xa = 0.f, xb = 0.f;
      if (pos < P) {
        const float* gp = a.g + (size_t)pos * a.Cout + co0 + col;
        ga = gp[0];
        if (co2) gb = gp[32];
        size_t pixel;
        if (wgrad_input_pixel(a, pos, ky, kx, pixel)) {
          const float* xp = a.x + pixel * a.Cin + ci0 + col;
          xa = xp[0];
          if (ci2) xb = xp[32];
        }
      }
      g0[t] = ga; g1[t] = gb; x0[t] = xa; x1[t] = xb;
    }
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(g0[t], x0[t], acc[0][0], 0, 0, 0);
      if (ci2) acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(g0[t], x1[t], acc[0][1], 0, 0, 0);
      if (co2) acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(g1[t], x0[t], acc[1][0], 0, 0, 0);
      if (co2 && ci2) acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(g1[t], x1[t], acc[1][1], 0, 0, 0);
      bsum0 += g0[t];
      bsum1 += g1[t];
    }
  }
  // waves 1..3 hand their 64 x 64 block to wave 0 through LDS, one 32 x 32 quarter at a time (12 KB)
  __shared__ float red[3 * 16 * 64];
  __shared__ float bred[2][4 * 64];
  wgrad_bias_put(bred[0], wave, lane, bsum0);
  wgrad_bias_put(bred[1], wave, lane, bsum1);
  const int Ktot = a.KH * a.KW * a.Cin;
  float *dw, *db;
  conv_wgrad_outputs(a, Ktot, dw, db);
#pragma unroll
  for (int i = 0; i < 2; ++i) {
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      if ((i && !co2) || (j && !ci2)) continue;      // workgroup-uniform
      __syncthreads();                               // the previous quarter has been consumed
      f32x16 v = acc[i][j];
      if (wgrad_reduce_waves(red, v, wave, lane))
        wgrad_store_tile(v, lane, dw + (size_t)(co0 + 32 * i) * Ktot + (size_t)tap * a.Cin + ci0 + 32 * j + col, Ktot, 1.f);
    }
  }
  if (a.db && tap == 0 && (tile % ci_tiles) == 0 && wave == 0 && lane < 32) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      if (i && !co2) continue;
      db[co0 + 32 * i + lane] = wgrad_bias_sum(bred[i], lane);
    }
  }
}

// Staged scheme (LDS-tiled).  The contraction index of dW = G^T . X is the POSITION, the slow index of both operands, so the direct
// kernels fetch one dword per lane and MFMA and compute an address per operand pair.  Here a workgroup (2 x 2 waves, 64 co x 64 ci of
// one tap) walks its position range in chunks of Stage::PK: the chunk's G rows and the tap-shifted, border-masked X rows are fetched
// with Stage::NL 16-byte loads per thread each (ONE position computation per load) into registers, staged in LDS in the Stage's
// format, and contracted from there.  The next chunk's global loads are in flight under the MFMAs of the current one.
//
// fp32 staging: chunks of 32 positions, a loader thread takes positions lp and lp + 16; the rows are staged as they lie ([position]
// [channel]: conflict-free stores), and every MFMA operand is one ds_read_b32 (lane = channel, half wave = position parity).
struct WgradStageF32 {
  static constexpr int PK = 32, NL = 2;
  __attribute__((aligned(16))) float As[PK][64];
  __attribute__((aligned(16))) float Bs[PK][64];
  static __device__ __forceinline__ int chunk_pos(int lp, int i) { return lp + 16 * i; }
  __device__ __forceinline__ void put(int lp, int c4, const f32x4* gr, const f32x4* xr) {
#pragma unroll
    for (int i = 0; i < NL; ++i) {
      *reinterpret_cast<f32x4*>(&As[lp + 16 * i][c4]) = gr[i];
      *reinterpret_cast<f32x4*>(&Bs[lp + 16 * i][c4]) = xr[i];
    }
  }
  __device__ __forceinline__ void mma(int row_a, int row_b, int kh, f32x16& acc) const {
    const float* ap = &As[kh][row_a];
    const float* bp = &Bs[kh][row_b];
#pragma unroll
    for (int kk = 0; kk < PK / 2; ++kk) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(ap[kk * 2 * 64], bp[kk * 2 * 64], acc, 0, 0, 0);
  }
};

// f16 staging (the AMP training step): dW = half(G)^T . half(X) on v_mfma_f32_32x32x16_f16, fp32 accumulate; db stays the
// fp32 sum of the unrounded G.  The f16 MFMA wants 8 consecutive k per lane, so the operands are transposed on their way into LDS: a
// loader thread fetches four channels of FOUR consecutive positions 4 lp .. 4 lp + 3 of a chunk of 64, rounds them (v_cvt_pk_f16_f32:
// RNE, overflow to inf, nothing clamped) and writes, per channel, its four positions as one 8-byte store into the [channel][position]
// image.  Rows are 64 halves + 16 bytes (144: an odd number of 16-byte slots, as in conv_f16.hip), so that the one ds_read_b128
// per operand and MFMA (lane = channel, half wave = positions 8h .. 8h + 7 of the K = 16 step) is conflict free.
typedef _Float16 wg_f16x2 __attribute__((ext_vector_type(2)));
typedef _Float16 wg_f16x8 __attribute__((ext_vector_type(8)));
typedef float wg_f32x2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ unsigned wg_pk_f16(float a, float b) {
  wg_f32x2 v = {a, b};
  return __builtin_bit_cast(unsigned, __builtin_convertvector(v, wg_f16x2));   // v_cvt_pk_f16_f32 (RNE)
}

struct WgradStageF16 {
  static constexpr int PK = 64, NL = 4, ROWB = 2 * PK + 16;
  __attribute__((aligned(16))) char As[64 * ROWB];     // half(G)^T: [co][position]
  __attribute__((aligned(16))) char Bs[64 * ROWB];     // half(X)^T: [ci][position]
  static __device__ __forceinline__ int chunk_pos(int lp, int i) { return 4 * lp + i; }
  __device__ __forceinline__ void put(int lp, int c4, const f32x4* gr, const f32x4* xr) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {                                      // channel c4 + j: its four positions, rounded, 8 bytes
      *reinterpret_cast<uint2*>(As + (c4 + j) * ROWB + lp * 8) = make_uint2(wg_pk_f16(gr[0][j], gr[1][j]), wg_pk_f16(gr[2][j], gr[3][j]));
      *reinterpret_cast<uint2*>(Bs + (c4 + j) * ROWB + lp * 8) = make_uint2(wg_pk_f16(xr[0][j], xr[1][j]), wg_pk_f16(xr[2][j], xr[3][j]));
    }
  }
  __device__ __forceinline__ void mma(int row_a, int row_b, int kh, f32x16& acc) const {
    const char* ap = As + row_a * ROWB + kh * 16;
    const char* bp = Bs + row_b * ROWB + kh * 16;
#pragma unroll
    for (int s = 0; s < PK / 16; ++s) {
      const wg_f16x8 af = __builtin_bit_cast(wg_f16x8, *reinterpret_cast<const uint4*>(ap + s * 32));
      const wg_f16x8 bf = __builtin_bit_cast(wg_f16x8, *reinterpret_cast<const uint4*>(bp + s * 32));
      acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(af, bf, acc, 0, 0, 0);
    }
  }
};

template <class Stage, bool LEVELS>
__global__ __launch_bounds__(256) void conv_backward_weights_staged_kernel(ConvBwdArgs a) {
  constexpr int PK = Stage::PK, NL = Stage::NL, TC = 64;
  __shared__ Stage st;
  __shared__ float bred[16][TC];
  const int ci_tiles = (a.Cin + 63) >> 6;
  const int tile = blockIdx.x;
  const int co0 = (tile / ci_tiles) * 64, ci0 = (tile % ci_tiles) * 64;
  const int tap = blockIdx.y;
  const int ky = tap / a.KW, kx = tap - ky * a.KW;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int r = lane & 31, kh = lane >> 5;
  const int P = LEVELS ? a.lv_off[a.nlv] : a.N * a.OH * a.OW;
  int c_begin, c_end;
  wgrad_chunk_range<PK>(a, P, c_begin, c_end);
  // loader role: thread -> (positions Stage::chunk_pos(lp, i) of the chunk, four channels c4 .. c4 + 3)
  const int lp = tid >> 4, c4 = (tid & 15) * 4;
  const bool g_ok = co0 + c4 < a.Cout, x_ok = ci0 + c4 < a.Cin;          // Cout, Cin are multiples of 32 (and of 4)
  f32x4 gr[NL], xr[NL];
  auto load_chunk = [&](int c) {
#pragma unroll
    for (int i = 0; i < NL; ++i) {
      const int pos = c * PK + Stage::chunk_pos(lp, i);
      f32x4 gv = {0.f, 0.f, 0.f, 0.f}, xv = {0.f, 0.f, 0.f, 0.f};
      if (pos < P) {
        if (g_ok) gv = *reinterpret_cast<const f32x4*>(a.g + (size_t)pos * a.Cout + co0 + c4);
        size_t pixel;
        const bool inside = LEVELS ? wgrad_level_pixel<WGRAD_MAX_LEVELS>(a, pos, ky, kx, pixel) : wgrad_input_pixel(a, pos, ky, kx, pixel);
        if (x_ok && inside) xv = *reinterpret_cast<const f32x4*>(a.x + pixel * a.Cin + ci0 + c4);
      }
      gr[i] = gv;
      xr[i] = xv;
    }
  };
  f32x16 acc;
#pragma unroll
  for (int q = 0; q < 16; ++q) acc[q] = 0.f;
  f32x4 bsum = {0.f, 0.f, 0.f, 0.f};
  if (c_begin < c_end) load_chunk(c_begin);
  for (int c = c_begin; c < c_end; ++c) {
    st.put(lp, c4, gr, xr);
#pragma unroll
    for (int i = 0; i < NL; ++i) bsum += gr[i];                        // positions in ascending order, unrounded
    __syncthreads();
    if (c + 1 < c_end) load_chunk(c + 1);
    st.mma(wm * 32 + r, wn * 32 + r, kh, acc);
    __syncthreads();
  }
  // C/D layout: column (ci) = lane & 31, row (co) = (q & 3) + 8 (q >> 2) + 4 (lane >> 5)
  const int Ktot = a.KH * a.KW * a.Cin;
  float *dw, *db;
  conv_wgrad_outputs(a, Ktot, dw, db);
  const int ci = ci0 + wn * 32 + r;
  if (ci < a.Cin) {
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      const int co = co0 + wm * 32 + (q & 3) + 8 * (q >> 2) + 4 * kh;
      if (co < a.Cout) dw[(size_t)co * Ktot + (size_t)tap * a.Cin + ci] = acc[q];
    }
  }
  if (a.db && tap == 0 && (tile % ci_tiles) == 0) wgrad_bias_rows(bred, lp, c4, bsum, co0, a.Cout, db);
}

// dW / db = the partial results of the position ranges added in range order (deterministic)
__global__ __launch_bounds__(256) void wgrad_reduce_kernel(const float* __restrict__ part, const float* __restrict__ bpart, float* __restrict__ dw,
                                                           float* __restrict__ db, size_t n, int Cout, int splits) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n + (db ? Cout : 0); i += (size_t)gridDim.x * blockDim.x) {
    float v = 0.f;
    if (i < n) {
      for (int z = 0; z < splits; ++z) v += part[(size_t)z * n + i];
      dw[i] = v;
    } else {
      const size_t c = i - n;
      for (int z = 0; z < splits; ++z) v += bpart[(size_t)z * Cout + c];
      db[c] = v;
    }
  }
}

// Weight gradient of a 4-channel layer whose kernel rows are wider than 8 taps (fallback; the stem, timm.py:279, takes the MFMA
// kernel above): tap layout, packed k = (ky, kx, ci), ci < 4.  Workgroup = one tap x 16 output channels; its 16 waves take every 16th
// output position, lane = (co, ci); the 16 partial sums are added in wave order through LDS (deterministic).  Tap 0's workgroups also
// write db.
__global__ __launch_bounds__(1024) void conv_backward_weights_tap4_kernel(ConvBwdArgs a) {
  __shared__ float part[16][64];
  __shared__ float partb[16][16];
  const int tap = blockIdx.x, co0 = blockIdx.y * 16;
  const int ky = tap / a.KW, kx = tap - ky * a.KW;
  const int t = threadIdx.x, ci = t & 3, col = (t >> 2) & 15, lane_p = t >> 6;
  const int P = a.N * a.OH * a.OW;
  const int pps = (P + a.splits - 1) / a.splits;
  const int p_begin = blockIdx.z * pps, p_end = min(p_begin + pps, P);
  float acc = 0.f, accb = 0.f;
#pragma unroll 4
  for (int p = p_begin + lane_p; p < p_end; p += 16) {
    const int ox = p % a.OW, r = p / a.OW;
    const int oy = r % a.OH, n = r / a.OH;
    const float gv = a.g[(size_t)p * a.Cout + co0 + col];
    accb += gv;
    const int iy = oy * a.stride - a.pad + ky, ix = ox * a.stride - a.pad + kx;
    if (iy >= 0 && iy < a.H && ix >= 0 && ix < a.W) acc += gv * a.x[((size_t)(n * a.H + iy) * a.W + ix) * 4 + ci];
  }
  part[lane_p][t & 63] = acc;
  if (ci == 0) partb[lane_p][col] = accb;
  __syncthreads();
  if (t < 64) {
    float s = 0.f;
    for (int i = 0; i < 16; ++i) s += part[i][t];
    const int Ktot = a.KH * a.KW * 4;
    float *dw, *db;
    conv_wgrad_outputs(a, Ktot, dw, db);
    dw[(size_t)(co0 + col) * Ktot + tap * 4 + ci] = s;
    if (tap == 0 && ci == 0 && a.db) {
      float sb = 0.f;
      for (int i = 0; i < 16; ++i) sb += partb[i][col];
      db[co0 + col] = sb;
    }
  }
}

// Input gradient of a STRIDED convolution (P6 / P7, timm.py:359-364; the trunk's stride-2 layers), gather form: one workgroup per
// input position, thread = input channel; dX[n][iy][ix][ci] = sum over the taps (ky, kx) with (iy + pad - ky) and (ix + pad - kx)
// multiples of the stride of sum_co G[n][(iy + pad - ky) / s][(ix + pad - kx) / s][co] * W[co][(ky, kx, ci)].  Weight reads are
// coalesced over ci, G values are broadcasts.  (Stride-1 layers use eod_conv2d with the rotated weights: matrix cores.)
__global__ __launch_bounds__(256) void conv_backward_input_kernel(ConvBwdArgs a, const float* __restrict__ w, int Kpad, float* __restrict__ dx) {
  const int pos = blockIdx.x;                         // (n, iy, ix)
  const int ix = pos % a.W, t = pos / a.W;
  const int iy = t % a.H, n = t / a.H;
  for (int ci = threadIdx.x; ci < a.Cin; ci += blockDim.x) {
    float acc = 0.f;
    for (int ky = 0; ky < a.KH; ++ky) {
      const int ny = iy + a.pad - ky;
      if (ny < 0 || ny % a.stride != 0) continue;
      const int oy = ny / a.stride;
      if (oy >= a.OH) continue;
      for (int kx = 0; kx < a.KW; ++kx) {
        const int nx = ix + a.pad - kx;
        if (nx < 0 || nx % a.stride != 0) continue;
        const int ox = nx / a.stride;
        if (ox >= a.OW) continue;
        const float* gp = a.g + ((size_t)(n * a.OH + oy) * a.OW + ox) * a.Cout;
        const float* wp = w + (size_t)(ky * a.KW + kx) * a.Cin + ci;
        for (int co = 0; co < a.Cout; ++co) acc += gp[co] * wp[(size_t)co * Kpad];
      }
    }
    dx[(size_t)pos * a.Cin + ci] = acc;
  }
}

}  // namespace

void wgrad_reduce_ranges(const float* part, const float* bpart, int splits, int outputs, size_t n, int Cout, float* const* dw,
                         float* const* db, hipStream_t stream) {
  size_t blocks = (n + Cout + 255) / 256;
  if (blocks > 4096) blocks = 4096;
  for (int o = 0; o < outputs; ++o)
    hipLaunchKernelGGL(wgrad_reduce_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, part + (size_t)o * splits * n,
                       bpart + (size_t)o * splits * Cout, dw[o], db[o], n, Cout, splits);
}

static int conv_bwd_args(ConvBwdArgs& a, int N, int H, int W, int Cin, int Cout, int KH, int KW, int pad, int stride) {
  if (N <= 0 || H <= 0 || W <= 0 || Cin <= 0 || Cout <= 0 || (Cin & 31) || (Cout & 31) || KH <= 0 || KW <= 0 || KH * KW > 64 ||
      pad < 0 || stride < 1 || H + 2 * pad < KH || W + 2 * pad < KW)
    return EOD_ERR_BAD_DIMS;
  if ((long)N * H * W >= (1L << 28)) return EOD_ERR_BAD_DIMS;
  a.N = N; a.H = H; a.W = W; a.Cin = Cin; a.Cout = Cout; a.KH = KH; a.KW = KW; a.pad = pad; a.stride = stride;
  a.OH = (H + 2 * pad - KH) / stride + 1;
  a.OW = (W + 2 * pad - KW) / stride + 1;
  a.div_w = eod_make_fastdiv((unsigned)a.OW);
  a.div_h = eod_make_fastdiv((unsigned)a.OH);
  return EOD_OK;
}

// EOD_WGRAD_RB=0 selects the 32 x 32 kernel instead of the register-blocked one, EOD_WGRAD_LDS=0 the register-blocked kernel instead
// of the LDS-tiled one (same-box A/B; read once)
static bool wgrad_switch(const char* name) {
  const char* e = getenv(name);
  return !(e && e[0] == '0');
}
static bool wgrad_register_blocked() {
  static const bool on = wgrad_switch("EOD_WGRAD_RB");
  return on;
}
static bool wgrad_lds() {
  static const bool on = wgrad_switch("EOD_WGRAD_LDS");
  return on;
}

// Position ranges of a weight-gradient launch: enough of them that ranges of `wgs` workgroups fill the chip (`want` when the kernel
// fixes the number), at most `cap` so that a range keeps a minimum of positions, at most 64.
static int wgrad_split_rule(long wgs, long cap, long want = 0) {
  long s = want ? want : (768 + wgs - 1) / wgs;
  if (s > cap) s = cap;
  if (s > 64) s = 64;
  return s < 1 ? 1 : (int)s;
}

// workgroups of the staged kernels per range
static long wgrad_staged_wgs(int Cin, int Cout, int KH, int KW) { return (long)((Cout + 63) >> 6) * ((Cin + 63) >> 6) * KH * KW; }

// image mode: ranges of at least 4 chunks of 32 positions (staged kernels; the f16 kernel cuts the positions like the fp32 one), 16
// k-steps of 8 (direct kernels), 2048 positions (scalar kernel)
static int wgrad_splits(int N, int H, int W, int Cin, int Cout, int KH, int KW, int pad, int stride) {
  const int OH = (H + 2 * pad - KH) / stride + 1, OW = (W + 2 * pad - KW) / stride + 1;
  const long P = (long)N * OH * OW;
  if (Cin == 4 && KW > 8) return wgrad_split_rule((long)KH * KW * (Cout >> 4), P / 2048, 16);     // the scalar kernel
  if (Cin == 4) return wgrad_split_rule((long)(Cout >> 5) * KH, (P + 7) / 8 / 16);
  const long wgs = wgrad_register_blocked() ? wgrad_staged_wgs(Cin, Cout, KH, KW)        // 64 x 64 tiles
                                            : (long)(Cout >> 5) * (Cin >> 5) * KH * KW;
  return wgrad_split_rule(wgs, wgrad_lds() ? (P + 31) / 32 / 4 : (P + 7) / 8 / 16);
}

// pyramid mode: the staged fp32 kernel over all levels' rows
static int wgrad_levels_splits(long rows, int Cin, int Cout, int KH, int KW) {
  return wgrad_split_rule(wgrad_staged_wgs(Cin, Cout, KH, KW), (rows + 31) / 32 / 4);
}

extern "C" size_t eod_conv2d_backward_weights_workspace_bytes(int N, int H, int W, int Cin, int Cout, int KH, int KW, int pad, int stride) {
  if (N <= 0 || H <= 0 || W <= 0 || Cin <= 0 || Cout <= 0 || KH <= 0 || KW <= 0 || pad < 0 || stride < 1) return 0;
  stride &= ~EOD_WGRAD_F16;
  if (stride < 1) return 0;
  return wgrad_workspace_bytes(wgrad_splits(N, H, W, Cin, Cout, KH, KW, pad, stride), 1, (size_t)Cout * KH * KW * Cin, Cout);
}

static int conv2d_backward_weights_impl(const float* x, const float* g, int N, int H, int W, int Cin, int Cout, int KH, int KW, int pad,
                                        int stride, float* dw, float* db, void* workspace, size_t workspace_bytes, eod_stream_t stream) {
  if (!x || !g || !dw) return EOD_ERR_NULL;
  // EOD_WGRAD_F16 on the stride argument: the f16 kernel (32-multiple channel counts; the 4-channel stem has no f16 form)
  const bool f16 = stride > 0 && (stride & EOD_WGRAD_F16) != 0;
  if (stride > 0) stride &= ~EOD_WGRAD_F16;
  if (f16 && Cin == 4) return EOD_ERR_BAD_DIMS;
  if (f16 && (!eod_aligned16(x) || !eod_aligned16(g))) return EOD_ERR_ALIGN;
  ConvBwdArgs a{};
  const int st = conv_bwd_args(a, N, H, W, Cin == 4 ? 32 : Cin, Cout, KH, KW, pad, stride);     // Cin == 4: the stem's tap layout
  if (st != EOD_OK) return st;
  a.Cin = Cin;
  a.x = x; a.g = g; a.dw = dw; a.db = db;
  const hipStream_t s = (hipStream_t)stream;
  const int taps = KH * KW, tiles64 = ((Cout + 63) >> 6) * ((Cin + 63) >> 6);
  return wgrad_launch_ranges(a, wgrad_splits(N, H, W, Cin, Cout, KH, KW, pad, stride), workspace, workspace_bytes, 1,
                             (size_t)Cout * taps * Cin, Cout, &dw, &db, s, [&] {
    if (f16)
      hipLaunchKernelGGL((conv_backward_weights_staged_kernel<WgradStageF16, false>), dim3(tiles64, taps, a.splits), dim3(256), 0, s, a);
    else if (Cin == 4 && KW <= 8)
      hipLaunchKernelGGL(conv_backward_weights_tap4_mfma_kernel, dim3((Cout >> 5) * KH, 1, a.splits), dim3(256), 0, s, a);
    else if (Cin == 4)
      hipLaunchKernelGGL(conv_backward_weights_tap4_kernel, dim3(taps, Cout >> 4, a.splits), dim3(1024), 0, s, a);
    else if (wgrad_lds())
      hipLaunchKernelGGL((conv_backward_weights_staged_kernel<WgradStageF32, false>), dim3(tiles64, taps, a.splits), dim3(256), 0, s, a);
    else if (wgrad_register_blocked())
      hipLaunchKernelGGL(conv_backward_weights_rb_kernel, dim3(tiles64, taps, a.splits), dim3(256), 0, s, a);
    else
      hipLaunchKernelGGL(conv_backward_weights_kernel, dim3((Cout >> 5) * (Cin >> 5), taps, a.splits), dim3(256), 0, s, a);
  });
}

extern "C" int eod_conv2d_backward_weights(const float* x, const float* g, int N, int H, int W, int Cin, int Cout, int KH, int KW, int pad,
                                           int stride, float* dw, float* db, eod_stream_t stream) {
  return conv2d_backward_weights_impl(x, g, N, H, W, Cin, Cout, KH, KW, pad, stride, dw, db, nullptr, 0, stream);
}

extern "C" int eod_conv2d_backward_weights_ws(const float* x, const float* g, int N, int H, int W, int Cin, int Cout, int KH, int KW,
                                              int pad, int stride, float* dw, float* db, void* workspace, size_t workspace_bytes,
                                              eod_stream_t stream) {
  if (workspace_bytes && !workspace) return EOD_ERR_NULL;
  return conv2d_backward_weights_impl(x, g, N, H, W, Cin, Cout, KH, KW, pad, stride, dw, db, workspace, workspace_bytes, stream);
}

// Pyramid mode: one launch for a level-shared layer (CenterNet tower / head, centernet_head.py:141-161) over all levels' rows.
extern "C" size_t eod_conv2d_backward_weights_levels_workspace_bytes(int rows, int Cin, int Cout, int KH, int KW) {
  if (rows <= 0 || Cin <= 0 || Cout <= 0 || KH <= 0 || KW <= 0) return 0;
  return wgrad_workspace_bytes(wgrad_levels_splits(rows, Cin, Cout, KH, KW), 1, (size_t)Cout * KH * KW * Cin, Cout);
}

extern "C" int eod_conv2d_backward_weights_levels(const float* x, const float* g, int levels, const int32_t* level_off,
                                                  const int32_t* level_h, const int32_t* level_w, int Cin, int Cout, int KH, int KW, int pad,
                                                  float* dw, float* db, void* workspace, size_t workspace_bytes, eod_stream_t stream) {
  if (!x || !g || !dw || !level_off || !level_h || !level_w) return EOD_ERR_NULL;
  if (levels < 1 || levels > WGRAD_MAX_LEVELS || Cin <= 0 || Cout <= 0 || (Cin & 31) || (Cout & 31) || KH <= 0 || KW <= 0 || KH != KW ||
      pad * 2 != KH - 1 || level_off[0] != 0)
    return EOD_ERR_BAD_DIMS;
  for (int l = 0; l < levels; ++l)
    if (level_h[l] <= 0 || level_w[l] <= 0 || level_off[l + 1] - level_off[l] != level_h[l] * level_w[l]) return EOD_ERR_BAD_DIMS;
  if (workspace_bytes && !workspace) return EOD_ERR_NULL;
  if (!eod_aligned16(x) || !eod_aligned16(g) || !eod_aligned16(dw)) return EOD_ERR_ALIGN;
  ConvBwdArgs a{};
  a.x = x; a.g = g; a.dw = dw; a.db = db;
  a.N = 1; a.H = a.OH = level_h[0]; a.W = a.OW = level_w[0];
  a.Cin = Cin; a.Cout = Cout; a.KH = KH; a.KW = KW; a.pad = pad; a.stride = 1;
  a.nlv = levels;
  for (int l = 0; l < levels; ++l) {
    a.lv_off[l] = level_off[l]; a.lv_h[l] = level_h[l]; a.lv_w[l] = level_w[l];
  }
  a.lv_off[levels] = level_off[levels];
  const hipStream_t s = (hipStream_t)stream;
  return wgrad_launch_ranges(a, wgrad_levels_splits(level_off[levels], Cin, Cout, KH, KW), workspace, workspace_bytes, 1,
                             (size_t)Cout * KH * KW * Cin, Cout, &dw, &db, s, [&] {
    hipLaunchKernelGGL((conv_backward_weights_staged_kernel<WgradStageF32, true>),
                       dim3(((Cout + 63) >> 6) * ((Cin + 63) >> 6), KH * KW, a.splits), dim3(256), 0, s, a);
  });
}

extern "C" int eod_conv2d_backward_input(const float* g, const float* w, int Kpad, int N, int H, int W, int Cin, int Cout, int KH, int KW,
                                         int pad, int stride, float* dx, eod_stream_t stream) {
  if (!g || !w || !dx) return EOD_ERR_NULL;
  ConvBwdArgs a{};
  const int st = conv_bwd_args(a, N, H, W, Cin, Cout, KH, KW, pad, stride);
  if (st != EOD_OK) return st;
  if (Kpad < KH * KW * Cin) return EOD_ERR_BAD_DIMS;
  a.g = g;
  hipLaunchKernelGGL(conv_backward_input_kernel, dim3(N * H * W), dim3(256), 0, (hipStream_t)stream, a, w, Kpad, dx);
  return eod_launch_status();
}
