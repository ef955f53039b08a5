// Convolution with operands rounded to binary16 on the f16 matrix cores, fp32 accumulate: opt-in arithmetic mode, DESIGN.md §3.
#include "conv_operands.h"

namespace eodconv {
namespace {

// ------------------------------------------------------------------------------------------------------
// y = epilogue( sum_k half(x)_k * half(w)_k ) on v_mfma_f32_32x32x16_f16: what torch.autocast makes of conv2d / linear.
//   * half() is v_cvt_pk_f16_f32: IEEE round-to-nearest-even, |v| > 65504 -> inf, subnormals kept, NaN stays NaN.  Nothing is
//     clamped or scaled, so inf / NaN propagate as IEEE says (0 * inf = NaN included);
//   * the products of two halves are exact in fp32 and summed in the fp32 MFMA accumulator; split-K slabs and the epilogue are the
//     fp32 ones of conv_common.h, the output is stored as unrounded fp32;
//   * the activations are fetched as fp32 exactly like the other kernels (same buffer-load addressing and padding mask),
//     converted in registers at staging time and written to LDS as [row][BK halves] + 16 B pad: 144-byte rows for BK = 64, 80 for
//     BK = 32 (9 / 5 slots of 16 B: an odd pitch, so the 16-lane groups of ds_read_b128 are conflict free);
//   * one ds_read_b128 per (32-row tile, K = 16 step) feeds the MFMA fragment directly: lane (r, h) takes k = 8h .. 8h+7 of its row;
//   * WH: the weights come as a half copy ([Cout][Kpad] binary16, eod_conv_half_weights): their LDS image is a plain copy of
//     16-byte pieces.  Without it they are fetched as fp32 and rounded like the activations (same values, twice the bytes).
//   * two LDS stages: the halves of chunk c+1 are written into the other stage in the iteration that multiplies chunk c, the
//     fp32 registers are refilled with chunk c+2 at once: one barrier per chunk, a full iteration for every load to land.
// The planner uses BK = 32 (measured: two 256x128 workgroups per CU instead of one); BK = 64 is selectable and needs Cin % 64 == 0
// (a chunk never straddles two filter taps).
typedef _Float16 f16x2_t __attribute__((ext_vector_type(2)));
typedef _Float16 f16x8_t __attribute__((ext_vector_type(8)));
typedef float f32x2_t __attribute__((ext_vector_type(2)));
typedef unsigned u32x4_t __attribute__((ext_vector_type(4)));

__device__ __forceinline__ unsigned pk_f16(float a, float b) {
  f32x2_t v = {a, b};
  return __builtin_bit_cast(unsigned, __builtin_convertvector(v, f16x2_t));   // v_cvt_pk_f16_f32 (RNE)
}
__device__ __forceinline__ uint2 half4(f32x4 v) { return make_uint2(pk_f16(v.x, v.y), pk_f16(v.z, v.w)); }

// GATE: the kernel honours ConvArgs.gate (EodConvDesc.gate: a ReLU's backward, with res_mode 1 the shortcut's sum, on the way out of
// an input-gradient launch).  Compiled into the 64x64 image-mode instantiations only, the ones the planner gives a gated f16 call:
// in the wide tiles the extra load spilled (conv_common.h), and the build refuses a kernel that uses scratch.
template <int BM, int BN, int NT, int BK, bool MULTI, bool WH, bool GATE = false>
__global__ __launch_bounds__(NT) void conv_f16_kernel(ConvArgs p) {
#if defined(__HIP_DEVICE_COMPILE__)
  constexpr int ROWB = 2 * BK + 16;              // bytes per tile row
  constexpr int STAGE = (BM + BN) * ROWB;
  constexpr int WM = NT / 128;                   // waves as WM x 2
  constexpr int TM = BM / (32 * WM), TN = BN / 64;
  constexpr int TPR = BK / 4;                    // threads per row at one float4 each
  constexpr int RPP = NT / TPR;                  // rows per staging pass
  constexpr int AR = BM / RPP, BR = WH ? 0 : BN / RPP, UNITS = AR + BR;
  constexpr int PPR = BK / 8;                    // WH: 16-byte weight pieces per row and chunk
  constexpr int BP = WH ? BN * PPR / NT : 0;
  static_assert(TM >= 1 && TN >= 1 && AR >= 1 && BN % RPP == 0 && (BN * PPR) % NT == 0, "tile / thread shape");
  extern __shared__ __attribute__((aligned(16))) char lds_dyn[];
  char* lds = lds_dyn;

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;

  int M;
  const int t = conv_first_tile<BM>(p, M);
  if (t < 0) return;
  const int tile_m = t / p.tiles_n;
  const int tile_n = t - tile_m * p.tiles_n;
  const int m0 = tile_m * BM, n0 = tile_n * BN;
  if (!conv_tile_active(p, m0, BM)) return;
  const int z = blockIdx.y;
  int c_end;
  const int c_begin = conv_chunk_range(p, p.cps, z, c_end);

  const int lr = tid / TPR, lq = tid % TPR;
  unsigned a_voff[AR];
  unsigned long long a_mask[AR];
  unsigned a_pitch[MULTI ? AR : 1];
#pragma unroll
  for (int i = 0; i < AR; ++i) conv_row_address<MULTI>(p, m0 + lr + RPP * i, M, lq, a_voff[i], a_mask[i], a_pitch[MULTI ? i : 0]);
  unsigned w_voff[BR > 0 ? BR : 1];
#pragma unroll
  for (int j = 0; j < BR; ++j) w_voff[j] = conv_w_row_offset(p, n0 + lr + RPP * j, lq);
  // WH: piece q = tid + NT u of the [BN rows][PPR pieces] weight tile
  unsigned wh_voff[BP > 0 ? BP : 1];
  int wh_lds[BP > 0 ? BP : 1];
#pragma unroll
  for (int u = 0; u < BP; ++u) {
    const int q = tid + NT * u;
    const int row = q / PPR, pc = q - row * PPR;
    const int n = n0 + row;
    wh_voff[u] = n < p.Cout ? (unsigned)(n * p.Kpad * 2 + pc * 16) : 0xFFFFFFFFu;
    wh_lds[u] = (BM + row) * ROWB + pc * 16;
  }
  const __amdgpu_buffer_rsrc_t rsrc_x = conv_buffer(p.x, p.x_bytes);
  const __amdgpu_buffer_rsrc_t rsrc_w = conv_buffer(p.w, p.w_bytes);
  const __amdgpu_buffer_rsrc_t rsrc_wh = conv_buffer(p.wh, WH ? p.wh_bytes : 0u);

  f32x4 raw[UNITS];
  u32x4_t braw[BP > 0 ? BP : 1];
  ChunkWalker<BK, MULTI> walk(p, c_begin);
  auto load_chunk = [&](const TapInfo& ti) {
#pragma unroll
    for (int u = 0; u < UNITS; ++u) {
      if (u < AR) raw[u] = conv_load_a<MULTI>(rsrc_x, ti, a_voff[u], a_mask[u], a_pitch[MULTI ? u : 0]);
      else raw[u] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rsrc_w, w_voff[u - AR], ti.k0b, 0));
    }
#pragma unroll
    for (int u = 0; u < BP; ++u) braw[u] = __builtin_amdgcn_raw_buffer_load_b128(rsrc_wh, wh_voff[u], ti.k0b >> 1, 0);
  };
  // rounds the fp32 registers to half and writes the tile image of one chunk
  auto stage_chunk = [&](char* stage) {
#pragma unroll
    for (int u = 0; u < UNITS; ++u) {
      const int row = u < AR ? lr + RPP * u : BM + lr + RPP * (u - AR);
      *reinterpret_cast<uint2*>(stage + row * ROWB + lq * 8) = half4(raw[u]);
    }
#pragma unroll
    for (int u = 0; u < BP; ++u) *reinterpret_cast<u32x4_t*>(stage + wh_lds[u]) = braw[u];
  };

  f32x16 acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  const int frow = lane & 31, fh = lane >> 5;
  const int a_fo = (wm * TM * 32 + frow) * ROWB + fh * 16;
  const int b_fo = (BM + wn * TN * 32 + frow) * ROWB + fh * 16;

  load_chunk(walk.next(p));
  stage_chunk(lds);
  load_chunk(walk.next(p));
  for (int chunk = c_begin; chunk < c_end; ++chunk) {
    const int st = (chunk - c_begin) & 1;
    const char* cur = lds + st * STAGE;
    char* nxt = lds + (st ^ 1) * STAGE;
    __syncthreads();      // stage `cur` fully written (previous iteration), stage `nxt` no longer read
    stage_chunk(nxt);     // chunk + 1, fetched one iteration ago
    load_chunk(walk.next(p));   // chunk + 2
#pragma unroll
    for (int s = 0; s < BK / 16; ++s) {
      f16x8_t af[TM], bfr[TN];
#pragma unroll
      for (int i = 0; i < TM; ++i) af[i] = __builtin_bit_cast(f16x8_t, *reinterpret_cast<const uint4*>(cur + a_fo + i * 32 * ROWB + s * 32));
#pragma unroll
      for (int j = 0; j < TN; ++j) bfr[j] = __builtin_bit_cast(f16x8_t, *reinterpret_cast<const uint4*>(cur + b_fo + j * 32 * ROWB + s * 32));
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(af[i], bfr[j], acc[i][j], 0, 0, 0);
    }
  }

  store_wave_tiles<TM, TN, GATE>(p, acc, m0 + wm * TM * 32, n0 + wn * TN * 32, M, z, lane);
#endif
}

}  // namespace

// [Cout][Kpad] fp32 -> [Cout][Kpad] binary16 (round-to-nearest-even), eight values per thread and step
__global__ __launch_bounds__(256) void half_weights_kernel(const float* __restrict__ w, uint4* __restrict__ out, size_t octs) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < octs; i += (size_t)gridDim.x * blockDim.x) {
    const uint2 lo = half4(*reinterpret_cast<const f32x4*>(w + i * 8));
    const uint2 hi = half4(*reinterpret_cast<const f32x4*>(w + i * 8 + 4));
    out[i] = make_uint4(lo.x, lo.y, hi.x, hi.y);
  }
}

void launch_half_weights(const float* w, void* out, int Cout, int Kpad, hipStream_t s) {
  const size_t octs = (size_t)Cout * Kpad / 8;
  int blocks = (int)((octs + 255) / 256);
  if (blocks > 4096) blocks = 4096;
  hipLaunchKernelGGL(half_weights_kernel, dim3(blocks), dim3(256), 0, s, w, static_cast<uint4*>(out), octs);
}

template <int BM, int BN, int NT, int BK, bool MULTI, bool WH, bool GATE = false>
static void launch_f16_one(const ConvArgs& a, dim3 grid, hipStream_t s) {
  constexpr int kLds = 2 * (BM + BN) * (2 * BK + 16);
  // above the 64 KiB a kernel gets without asking; a refused attribute shows up as a launch error (EOD_ERR_LAUNCH)
  static const bool attr = kLds <= 65536 || hipFuncSetAttribute(reinterpret_cast<const void*>(&conv_f16_kernel<BM, BN, NT, BK, MULTI, WH, GATE>),
                                                                hipFuncAttributeMaxDynamicSharedMemorySize, kLds) == hipSuccess;
  (void)attr;
  hipLaunchKernelGGL((conv_f16_kernel<BM, BN, NT, BK, MULTI, WH, GATE>), grid, dim3(NT), kLds, s, a);
}

template <int BM, int BN, int NT>
static void launch_f16_tile(const ConvArgs& a, int bk, dim3 grid, hipStream_t s) {
  const bool multi = a.nlv > 0, wh = a.wh != nullptr;
  if (bk == 64) {
    if (multi) wh ? launch_f16_one<BM, BN, NT, 64, true, true>(a, grid, s) : launch_f16_one<BM, BN, NT, 64, true, false>(a, grid, s);
    else wh ? launch_f16_one<BM, BN, NT, 64, false, true>(a, grid, s) : launch_f16_one<BM, BN, NT, 64, false, false>(a, grid, s);
  } else {
    if (multi) wh ? launch_f16_one<BM, BN, NT, 32, true, true>(a, grid, s) : launch_f16_one<BM, BN, NT, 32, true, false>(a, grid, s);
    else wh ? launch_f16_one<BM, BN, NT, 32, false, true>(a, grid, s) : launch_f16_one<BM, BN, NT, 32, false, false>(a, grid, s);
  }
}

// the gated 64x64 tile (image mode: make_plan gives a gated pyramid launch the fp32 kernel)
static void launch_f16_gated(const ConvArgs& a, int bk, dim3 grid, hipStream_t s) {
  const bool wh = a.wh != nullptr;
  if (bk == 64) wh ? launch_f16_one<64, 64, 256, 64, false, true, true>(a, grid, s) : launch_f16_one<64, 64, 256, 64, false, false, true>(a, grid, s);
  else wh ? launch_f16_one<64, 64, 256, 32, false, true, true>(a, grid, s) : launch_f16_one<64, 64, 256, 32, false, false, true>(a, grid, s);
}

// tile 4 = 256x128 (8 waves), anything else 64x64 (4 waves); bk = 64 only by force_tile and with Cin % 64 == 0 (make_plan)
void launch_conv_f16(const ConvArgs& a, int tile, int bk, dim3 grid, hipStream_t s) {
  if (a.gate) launch_f16_gated(a, bk, grid, s);
  else if (tile == 4) launch_f16_tile<256, 128, 512>(a, bk, grid, s);
  else launch_f16_tile<64, 64, 256>(a, bk, grid, s);
}

}  // namespace eodconv
