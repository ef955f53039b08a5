// Pointwise (1x1, stride 1) fp32 convolution with a shallow K of 64, 128 or 256: the ResNet trunk's layer1 / layer2.0 conv1, every
// conv3 of layer1-3 and layer1.0's downsample.
//
// The generic conv_igemm_kernel<64,64,32> gives such a layer thousands of 64x64 tiles of only 2-8 K chunks: every tile pays the whole
// prologue (tile claim, row origins, tap masks), the activation tile is fetched again for each 64-column tile and the residual is
// loaded only after the last MFMA.  Here a workgroup (256 threads, 2 x 2 waves) owns 64 output rows and `np` consecutive 64-column
// panels:
//   * the activation tile -- 64 rows x the whole K, one contiguous run of memory because a 1x1 stride-1 row is the pixel itself --
//     is fetched once with wide loads and stays in LDS as [row][K + 4];
//   * the weight panels stream through a double-buffered LDS stage ([64][BKW + 4], BKW = 32; 16 at K = 256 so that two workgroups
//     fit on a CU), two stages ahead in registers, one barrier per stage, straight across the panel boundaries;
//   * the bias and residual of panel p + 1 are requested before the MFMAs of panel p.
// LDS per workgroup: K = 64 35 840 B, K = 128 52 224 B (3 per CU, K = 64 by its registers), K = 256 76 800 B (2 per CU).
//
// Arithmetic: bitwise that of conv_igemm_kernel<64,64,32>.  K is walked in ascending order in k-steps of 8; lane half h supplies
// k = 8 * step + 4h + t to instruction t; even t feeds one accumulator chain and odd t the other; the chains are added once as a + b;
// the epilogue's statements are those of epilogue_store (conv_common.h) on operands already in registers.
#include "conv_operands.h"

namespace eodconv {
namespace {

template <int K>
struct PointwiseCfg {
  static constexpr int BKW = K == 256 ? 16 : 32;     // K width of a weight stage
  static constexpr int LSA = K + 4;                  // LDS row strides in floats (+4: conflict-free ds_read_b128, as in conv_fp32.hip)
  static constexpr int LSW = BKW + 4;
  static constexpr int A_FLOATS = 64 * LSA;
  static constexpr int W_FLOATS = 64 * LSW;          // one stage buffer
  static constexpr int LDS_BYTES = (A_FLOATS + 2 * W_FLOATS) * 4;
  // workgroups per CU the register budget is set for: what LDS allows of 160 KB, but 3 at K = 64 (LDS would take 4: the two
  // residual sets and the accumulators spill at 128 registers)
  static constexpr int WG_PER_CU = K == 256 ? 2 : 3;
};

template <int K>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(PointwiseCfg<K>::WG_PER_CU))) void conv_pointwise_kernel(ConvArgs p, int np) {
  using Cfg = PointwiseCfg<K>;
  constexpr int BKW = Cfg::BKW, LSA = Cfg::LSA, LSW = Cfg::LSW;
  constexpr int NC = K / BKW;        // weight stages per panel (even: a stage's LDS buffer and register set follow from its parity)
  constexpr int KS = BKW / 8;        // k-steps of four MFMAs per stage
  constexpr int QPR = BKW / 4;       // float4 per staged weight row
  constexpr int RPP = 256 / QPR;     // weight rows staged per pass of the 256 threads
  constexpr int BR = 64 / RPP;
  constexpr int AQ = K / 4;          // float4 per activation row
  constexpr int AR = K / 16;         // float4 of the activation tile per thread
  static_assert(NC % 2 == 0, "stage parity");
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float* As = lds;
  float* Ws = lds + Cfg::A_FLOATS;

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;

  // p.tiles_n = panel groups per row tile; the XCD remap runs over the live tiles (conv_first_tile)
  int M;
  const int t = conv_first_tile<64>(p, M);
  if (t < 0) return;
  const int tile_m = t / p.tiles_n;
  const int grp = t - tile_m * p.tiles_n;
  const int m0 = tile_m * 64;
  const int panels = p.Cout >> 6;
  const int p0 = grp * np;
  const int p1 = p0 + np < panels ? p0 + np : panels;

  const __amdgpu_buffer_rsrc_t rsrc_x = conv_buffer(p.x, p.x_bytes);
  const __amdgpu_buffer_rsrc_t rsrc_w = conv_buffer(p.w, p.w_bytes);

  // weight stage c of a panel (c may run past the panel's last stage: the next panel's; past the last panel: nothing)
  const int lr = tid / QPR, lq = tid % QPR;
  auto load_w = [&](int panel, int c, f32x4 (&wr)[BR]) {
    if (c >= NC) {
      c -= NC;
      ++panel;
    }
    if (panel >= p1) return;
#pragma unroll
    for (int j = 0; j < BR; ++j)
      wr[j] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rsrc_w, conv_w_row_offset(p, panel * 64 + lr + RPP * j, lq),
                                                                              c * BKW * 4, 0));
  };
  auto store_w = [&](int buf, const f32x4 (&wr)[BR]) {
#pragma unroll
    for (int j = 0; j < BR; ++j) *reinterpret_cast<f32x4*>(Ws + buf * Cfg::W_FLOATS + (lr + RPP * j) * LSW + 4 * lq) = wr[j];
  };

  // this lane's share of a panel's bias and residual (MFMA C/D layout: col = lane & 31, row = (r&3) + 8*(r>>2) + 4*(lane>>5))
  const int half = lane >> 5;
  const int m_base = m0 + wm * 32 + 4 * half;
  const int n_lane = wn * 32 + (lane & 31);
  auto load_res = [&](int panel, float (&rr)[16], float& bb) {
    const int n = panel * 64 + n_lane;
    if (p.bias) bb = p.bias[n];
    if (p.res_mode == 1) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int m = m_base + (r & 3) + 8 * (r >> 2);
        if (m < M) rr[r] = p.res[(unsigned)(m * p.Cout + n)];      // rows x Cout < 2^31: check_desc
      }
    }
  };

  // ---- prologue: the activation tile (one contiguous run; rows past M read zeros through the range check), the first two weight
  // stages and the first panel's bias / residual
  f32x4 w0[BR], w1[BR];
  float rcur[16], rnext[16];
  float bcur = 0.f, bnext = 0.f;
#pragma unroll
  for (int r = 0; r < 16; ++r) rcur[r] = rnext[r] = 0.f;
  {
    f32x4 ar[AR];
    const unsigned a_off = (unsigned)(m0 * K + 4 * tid) * 4u;
#pragma unroll
    for (int i = 0; i < AR; ++i) ar[i] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rsrc_x, a_off + i * 4096u, 0, 0));
    load_w(p0, 0, w0);
    load_w(p0, 1, w1);
    load_res(p0, rcur, bcur);
#pragma unroll
    for (int i = 0; i < AR; ++i) {
      const int idx = i * 256 + tid;
      *reinterpret_cast<f32x4*>(As + (idx / AQ) * LSA + 4 * (idx % AQ)) = ar[i];
    }
    store_w(0, w0);
  }
  __syncthreads();

  const int frag_row = lane & 31;
  const int frag_k = 4 * half;
  const float* a_base = As + (wm * 32 + frag_row) * LSA + frag_k;
  const float* b_base = Ws + (wn * 32 + frag_row) * LSW + frag_k;

  f32x16 acc, acc_b;
  // stage c of `panel` from LDS buffer c & 1: `hold` has stage c + 1 in registers (stored to the other buffer after the MFMAs),
  // `fill` is free and receives stage c + 2
  auto stage = [&](int panel, int c, int buf, f32x4 (&hold)[BR], f32x4 (&fill)[BR]) {
    load_w(panel, c + 2, fill);
    const float* ab = a_base + c * BKW;
    const float* bb = b_base + buf * Cfg::W_FLOATS;
    f32x4 af[2], bf[2];
    af[0] = *reinterpret_cast<const f32x4*>(ab);
    bf[0] = *reinterpret_cast<const f32x4*>(bb);
#pragma unroll
    for (int kk = 0; kk < KS; ++kk) {
      const int cur = kk & 1, nxt = cur ^ 1;
      if (kk + 1 < KS) {
        af[nxt] = *reinterpret_cast<const f32x4*>(ab + (kk + 1) * 8);
        bf[nxt] = *reinterpret_cast<const f32x4*>(bb + (kk + 1) * 8);
      }
      __builtin_amdgcn_s_setprio(1);
#pragma unroll
      for (int tt = 0; tt < 4; ++tt)
        if (tt & 1)
          acc_b = __builtin_amdgcn_mfma_f32_32x32x2f32(af[cur][tt], bf[cur][tt], acc_b, 0, 0, 0);
        else
          acc = __builtin_amdgcn_mfma_f32_32x32x2f32(af[cur][tt], bf[cur][tt], acc, 0, 0, 0);
      __builtin_amdgcn_s_setprio(0);
    }
    if (c + 1 < NC || panel + 1 < p1) store_w(buf ^ 1, hold);
    __syncthreads();
  };

  for (int panel = p0; panel < p1; ++panel) {
    if (panel + 1 < p1) load_res(panel + 1, rnext, bnext);
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      acc[r] = 0.f;
      acc_b[r] = 0.f;
    }
    for (int c = 0; c < NC; c += 2) {
      stage(panel, c, 0, w1, w0);
      stage(panel, c + 1, 1, w0, w1);
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] += acc_b[r];
    // the fused epilogue: epilogue_store's statements (out_mode 0, res_mode 0 / 1), bias and residual from registers
    const int n = panel * 64 + n_lane;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int m = m_base + (r & 3) + 8 * (r >> 2);
      if (m < M) {
        float v = acc[r];
        if (p.bias) v += bcur;
        v *= p.out_scale;
        if (p.res_mode == 1) v += rcur[r];
        if (p.relu) v = fmaxf(v, 0.0f);
        p.y[(unsigned)(m * p.Cout + n)] = v;
      }
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) rcur[r] = rnext[r];
    bcur = bnext;
  }
}

template <int K>
void launch_pointwise(const ConvArgs& a, int np, dim3 grid, hipStream_t s) {
  constexpr int kLds = PointwiseCfg<K>::LDS_BYTES;
  // above the 64 KiB a kernel gets without asking; a refused attribute shows up as a launch error (EOD_ERR_LAUNCH)
  static const bool attr = kLds <= 65536 || hipFuncSetAttribute(reinterpret_cast<const void*>(&conv_pointwise_kernel<K>),
                                                                hipFuncAttributeMaxDynamicSharedMemorySize, kLds) == hipSuccess;
  (void)attr;
  hipLaunchKernelGGL((conv_pointwise_kernel<K>), grid, dim3(256), kLds, s, a, np);
}

}  // namespace

// K = a.Kpad in {64, 128, 256} (make_plan's pointwise_eligible); grid = row tiles x panel groups of `np` panels (a.tiles_n groups)
void launch_conv_pointwise(const ConvArgs& a, int np, dim3 grid, hipStream_t s) {
  switch (a.Kpad) {
    case 64: launch_pointwise<64>(a, np, grid, s); break;
    case 128: launch_pointwise<128>(a, np, grid, s); break;
    default: launch_pointwise<256>(a, np, grid, s); break;
  }
}

}  // namespace eodconv
