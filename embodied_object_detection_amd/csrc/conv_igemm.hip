// eod_conv2d: argument checks, tile / split-K planning, arithmetic-mode switch and the C ABI of the implicit-GEMM convolution.
//
//   y[m][n] = act( (sum_k A[m][k] * Wt[n][k] + bias[n]) * out_scale + res[m][n] )
//
// A[m][k] is the im2col view of the NHWC input (m = (img, oy, ox), k = (ky, kx, c), c fastest), Wt is [Cout][Kpad].  The kernels
// live in conv_fp32.hip (fp32 MFMA, default), conv_pointwise.hip (the trunk's shallow-K 1x1 layers, fp32), conv_bf16x3.hip (opt-in split-bf16 arithmetic) and conv_f16.hip (opt-in: operands rounded
// to half, fp32 accumulate); this file picks one, sizes the grid and, for small problems, splits K into fp32 slabs that
// conv_splitk_reduce_kernel sums in a fixed order before the fused epilogue (deterministic, no atomics).
#include "conv_common.h"
#include "../../include/eod_hip.h"
#include <atomic>
#include <cstdlib>
#include <cstring>

namespace {

using namespace eodconv;

// Sums the K slabs in slab order and applies the fused epilogue.  VEC = 4: one float4 of four consecutive output channels per
// thread and slab (Cout % 4 == 0); VEC = 1 for the odd-width heads.  32-bit indices (check_desc bounds rows x Cout below 2^31).
template <int VEC>
__global__ __launch_bounds__(256) void conv_splitk_reduce_kernel(ConvArgs p) {
  EOD_CHAIN_PRIO();
  const int M = conv_row_limit(p, p.M);
  const unsigned per_row = (unsigned)p.Cout / VEC;
  const unsigned total = (unsigned)M * per_row;
  const size_t slab = (size_t)p.M * p.Cout;
  for (unsigned idx = blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += gridDim.x * blockDim.x) {
    const unsigned m = fdiv(idx, p.div_row);
    if (!conv_row_active(p, (int)m)) continue;          // segmented counts: the tile that would have written this row's slabs left early
    const unsigned n = (idx - m * per_row) * VEC;
    const float* src = p.partial + (size_t)m * p.Cout + n;
    if (VEC == 4) {
      f32x4 v = {0.f, 0.f, 0.f, 0.f};
      // four slabs at a time: independent loads in flight together, added in slab order
      for (int zb = 0; zb < p.splitk; zb += 4) {
        f32x4 t[4];
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (zb + j < p.splitk) t[j] = *reinterpret_cast<const f32x4*>(src + (size_t)(zb + j) * slab);
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (zb + j < p.splitk) v += t[j];
      }
      epilogue_store<true>(p, v.x, (int)m, (int)n);
      epilogue_store<true>(p, v.y, (int)m, (int)n + 1);
      epilogue_store<true>(p, v.z, (int)m, (int)n + 2);
      epilogue_store<true>(p, v.w, (int)m, (int)n + 3);
    } else {
      float v = 0.f;
      for (int z = 0; z < p.splitk; ++z) v += src[z * slab];
      epilogue_store<true>(p, v, (int)m, (int)n);
    }
  }
}

// The slab reduce of a pyramid-mode layer that is followed by GroupNorm (CenterNet tower, centernet_head.py:76-79): the same sums
// in slab order + epilogue, one workgroup per 32-row chunk of one level (eod_groupnorm_relu's chunks), and the chunk's GroupNorm
// partial sums on the way -> partial[chunk][group][2] -- so that the statistics launch is not needed.  Memory access as in the
// plain reduce: a thread owns one float4 column (4 consecutive channels) and every (256 / (C/4))-th row of the chunk; sum and sum
// of squares are accumulated in double per thread (rows in ascending order, the four channels in order), combined over the
// threads of a channel group with shuffles and over the row subsets through LDS in subset order: deterministic.  (The first
// version walked one channel per thread over 32 rows x slabs: 44 us against 12 + 11 for the two separate launches.)
#define EOD_GN_ROWS 32
__global__ __launch_bounds__(256) void conv_splitk_reduce_gn_kernel(ConvArgs p) {
  EOD_CHAIN_PRIO();
  __shared__ double red[4][64][2];           // [row subset][group][sum, sum of squares]; groups <= 64, subsets <= 4
  int level = 0, first_chunk = 0;
  for (;;) {
    const int rows = p.lv_off[level + 1] - p.lv_off[level];
    const int nch = (rows + EOD_GN_ROWS - 1) / EOD_GN_ROWS;
    if ((int)blockIdx.x < first_chunk + nch || level + 1 >= p.nlv) break;
    first_chunk += nch;
    ++level;
  }
  const int r0 = p.lv_off[level] + ((int)blockIdx.x - first_chunk) * EOD_GN_ROWS;
  const int r1 = min(r0 + EOD_GN_ROWS, p.lv_off[level + 1]);
  const int C = p.Cout;
  const int c4 = C >> 2;                     // float4 columns per row: 64 for the tower (checked on the host: 256 % c4 == 0)
  const int nsub = 256 / c4;                 // row subsets: 4
  const int col = threadIdx.x % c4, sub = threadIdx.x / c4;
  const int cpg4 = (C / p.gn_groups) >> 2;   // float4 columns per channel group: 2
  const size_t slab = (size_t)p.M * C;
  double s = 0.0, q = 0.0;
  for (int r = r0 + sub; r < r1; r += nsub) {
    const float* src = p.partial + (size_t)r * C + col * 4;
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    for (int zb = 0; zb < p.splitk; zb += 4) {
      f32x4 t[4];
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (zb + j < p.splitk) t[j] = *reinterpret_cast<const f32x4*>(src + (size_t)(zb + j) * slab);
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (zb + j < p.splitk) v += t[j];
    }
    const double o0 = (double)epilogue_store<true>(p, v.x, r, col * 4 + 0);
    const double o1 = (double)epilogue_store<true>(p, v.y, r, col * 4 + 1);
    const double o2 = (double)epilogue_store<true>(p, v.z, r, col * 4 + 2);
    const double o3 = (double)epilogue_store<true>(p, v.w, r, col * 4 + 3);
    s += o0; q += o0 * o0;
    s += o1; q += o1 * o1;
    s += o2; q += o2 * o2;
    s += o3; q += o3 * o3;
  }
  for (int off = 1; off < cpg4; off <<= 1) {      // the columns of one group are adjacent lanes (c4 is a multiple of cpg4, 64 of c4)
    s += __shfl_xor(s, off, 64);
    q += __shfl_xor(q, off, 64);
  }
  if ((col % cpg4) == 0) {
    red[sub][col / cpg4][0] = s;
    red[sub][col / cpg4][1] = q;
  }
  __syncthreads();
  if ((int)threadIdx.x < p.gn_groups) {
    double ts = 0.0, tq = 0.0;
    for (int u = 0; u < nsub; ++u) {
      ts += red[u][threadIdx.x][0];
      tq += red[u][threadIdx.x][1];
    }
    p.gn_partial[((size_t)blockIdx.x * p.gn_groups + threadIdx.x) * 2 + 0] = ts;
    p.gn_partial[((size_t)blockIdx.x * p.gn_groups + threadIdx.x) * 2 + 1] = tq;
  }
}

// Process-wide arithmetic mode of eod_conv2d (eod_set_conv_math / EOD_CONV_MATH): 0 fp32 MFMA, 1 bf16x3 split, 2 f16 operands.
// The environment value is matched exactly; anything else (unset, empty, a misspelling) is the fp32 default.
std::atomic<int>& math_mode() {
  static std::atomic<int> v([] {
    const char* e = getenv("EOD_CONV_MATH");
    if (e && strcmp(e, "bf16x3") == 0) return EOD_MATH_BF16X3;
    if (e && strcmp(e, "f16") == 0) return EOD_MATH_F16;
    return EOD_MATH_FP32;
  }());
  return v;
}

struct Plan {
  int tile;  // 1=128x128 2=128x64 3=64x64
  int bk;    // K chunk staged per barrier pair: 32 or 64
  int glds;  // 2: bf16x3 split kernel (BK = 32); 3: f16 kernel (BK = 32; 64 by force_tile 8x); 0: fp32 MFMA kernel
  int bm, bn, tiles_m, tiles_n, splitk, cps, nchunks;
  int wavek;  // 0, or the number of waves (4 / 8) of the 32x32-tile kernel that splits K over the waves of a workgroup
  int pw_np;  // 0, or the 64-column panels per workgroup of the pointwise kernel (conv_pointwise.hip; tile 6, bn = 64 * pw_np)
  int border; // 1: the 64x64 fp32 kernel deals its rows in the border-major order and skips all-padding K chunks (conv_fp32.hip)
};

// force_tile code of the pointwise kernel: forces it on a call it can take (pointwise_eligible), EOD_ERR_BAD_DIMS for any other
constexpr int kForcePointwise = 30;

int effective_math(const EodConvDesc* d) { return d->math > 0 ? d->math - 1 : math_mode().load(std::memory_order_relaxed); }

// What conv_pointwise_kernel takes: fp32 arithmetic, a 1x1 stride-1 image-mode layer whose whole K is 64, 128 or 256, whole
// 64-column panels, the plain or same-shape-residual epilogue and a static row count.
bool pointwise_eligible(const EodConvDesc* d) {
  return effective_math(d) == EOD_MATH_FP32 && d->KH == 1 && d->KW == 1 && d->stride == 1 && d->pad == 0 && d->levels <= 0 && !d->tap4 &&
         d->Cin == d->Kpad && (d->Cin == 64 || d->Cin == 128 || d->Cin == 256) && d->Cout % 64 == 0 && d->out_mode == 0 &&
         (d->res_mode == 0 || d->res_mode == 1) && !d->in_relu && !d->gate && !d->m_count && d->split_n == 0 && !d->gn_partial &&
         d->lds_reserve == 0;
}

// force_tile code of the border-major row order: forces it on a call it can take (border_eligible), EOD_ERR_BAD_DIMS for any other.
// force_tile 13 stays the pixel-major order on every call (the A/B switch and the tests' reference).
constexpr int kForceBorder = 43;
// Whether the planner gives an eligible call the border-major order by itself (profiles/r16_border_order.md: the measurement the
// default rests on).
constexpr bool kBorderAuto = true;

// What the border-major order takes: fp32 arithmetic, a 3x3 / stride 1 / pad 1 image-mode layer over maps of at least 3x3 pixels
// whose row count is ONE device-side count of whole maps, the plain epilogue and the default pipeline.
bool border_eligible(const EodConvDesc* d) {
  return effective_math(d) == EOD_MATH_FP32 && d->KH == 3 && d->KW == 3 && d->stride == 1 && d->pad == 1 && d->levels <= 0 && !d->tap4 &&
         d->m_count && d->m_segments <= 1 && d->m_unit == d->OH * d->OW && d->OH >= 3 && d->OW >= 3 && d->Cin % 32 == 0 &&
         d->out_mode == 0 && d->res_mode == 0 && !d->in_relu && !d->gate && d->split_n == 0 && !d->gn_partial && d->prefetch2 == 0;
}

Plan make_plan(const EodConvDesc* d, int M) {
  // 256x128: bf16x3 / f16 8-wave kernels only; 64x256: fused mask-head tail (out_mode 2) only
  static const int cfg[5][2] = {{128, 128}, {128, 64}, {64, 64}, {256, 128}, {64, 256}};
  Plan pl{};
  // Measured on MI355X (tools/conv_bench.py, profiles/r01_conv_bench.log): the 64x64 tile (7 waves/SIMD, finest
  // tile quantisation over 256 CUs) is the fastest or ties on every shape of this path, including the
  // 50k x 256 x 2304 mask-head GEMM (107 vs 92 TFLOP/s for 128x128).  The larger tiles stay selectable.
  int pick = 2;
  // force_tile = tile + 10 (BK 32) / + 20 (BK 64); + 50: bf16x3 kernels; + 90 / + 80: f16 kernels (tile 3 or 4) with BK 32 (the planner's) / 64
  const int ft = d->force_tile % 10, fbk = d->force_tile / 10;
  const bool half_ok = !d->tap4 && !d->in_relu;                  // what the bf16x3 and f16 kernels take; the rest stays fp32
  const bool f16_forced = (fbk == 8 || fbk == 9) && half_ok;
  if (f16_forced) pick = ft == 4 ? 3 : 2;
  else if (ft >= 1 && ft <= 3) pick = ft - 1;
  else if (ft == 4 && fbk == 5 && half_ok) pick = 3;
  const bool bk64_ok = !d->tap4 && d->Cin % 64 == 0 && d->Kpad % 64 == 0;
  pl.glds = f16_forced ? 3 : ((fbk == 5 && half_ok) ? 2 : 0);
  // tile and split-K are decided on `plan_rows` when given (a batch planned like one image: identical K walk, bitwise equal results)
  const int Mp = (d->plan_rows > 0 && d->plan_rows < M) ? d->plan_rows : M;
  // EodConvDesc.math: this call's arithmetic (EOD_MATH_* + 1), 0 = the process-wide mode
  const int math = effective_math(d);
  if (d->force_tile == 0 && math == EOD_MATH_F16 && half_ok) {
    pl.glds = 3;
    // like bf16x3: the 8-wave 256x128 tile once it fills the chip, else the finest tile; decided on plan_rows like the slabs
    pick = (long)((Mp + 255) / 256) * ((d->Cout + 127) / 128) >= 256 ? 3 : 2;
  }
  if (d->force_tile == 0 && math == EOD_MATH_BF16X3 && half_ok) {
    pl.glds = 2;
    const long t128 = (long)((Mp + 127) / 128) * ((d->Cout + 127) / 128);
    const long t256 = (long)((Mp + 255) / 256) * ((d->Cout + 127) / 128);
    // measured (profiles/r01_bf16x3_accuracy_speed.log): 256x128 (8 waves, one workgroup per CU) once it fills the chip,
    // 128x128 once it fills two workgroups per CU, else the finest tile
    pick = t256 >= 256 ? 3 : (t128 >= 512 ? 0 : 2);
  }
  if (d->out_mode == 2) {   // one workgroup owns all 256 channels of a deconv quadrant; fp32 kernel in every arithmetic mode
    pick = 4;
    pl.glds = 0;
  }
  if (d->gate) {            // the gated epilogue lives in the 64x64 fp32 tile, the wave-K kernel and the slab reduces ...
    // ... and in the 64x64 f16 tile, which a call that asks for f16 itself (EodConvDesc.math: the AMP step's input-gradient
    // launches) gets; the process-wide f16 mode is for inference and keeps gated launches in fp32 as before
    const bool f16_gated = d->math == EOD_MATH_F16 + 1 && half_ok && d->levels <= 0 && (d->force_tile == 0 || f16_forced);
    pick = 2;
    pl.glds = f16_gated ? 3 : 0;
  }
  // f16: BK = 32 measured faster or equal on the frame's layers (two 256x128 workgroups per CU instead of one; tools/f16_check.py);
  // BK = 64 stays selectable (force_tile 8x) where Cin % 64 == 0, so that a chunk never straddles two filter taps
  if (pl.glds == 3) pl.bk = (fbk == 8 && d->Cin % 64 == 0) ? 64 : 32;
  // fp32: BK = 32 unless force_tile 2x asks for 64.  Measured end to end on the final schedule (profiles/r01_bench_640_default.log
  // era): BK=32 140.8 frames/s / 119.6 TFLOP/s on the mask GEMM vs BK=64 139.4 / 117.4 (smaller LDS tile -> one more workgroup per
  // CU; the halved barrier count of BK=64 stopped paying once the K-loop bookkeeping became incremental)
  else pl.bk = (pl.glds == 0 && d->out_mode != 2 && fbk == 2 && bk64_ok) ? 64 : 32;
  const int nchunks = d->Kpad / pl.bk;
  pl.nchunks = nchunks;
  pl.tile = pick + 1;
  pl.bm = cfg[pick][0];
  pl.bn = cfg[pick][1];
  pl.tiles_m = (M + pl.bm - 1) / pl.bm;
  pl.tiles_n = (d->Cout + pl.bn - 1) / pl.bn;
  const long tiles = (long)((Mp + pl.bm - 1) / pl.bm) * pl.tiles_n;
  int splitk = 1;
  if (d->out_mode == 2) {
    splitk = 1;
  } else if (d->force_splitk > 0) {
    splitk = d->force_splitk;
  } else if (pl.glds == 0 && !d->tap4 && nchunks >= 8 &&
             ((d->force_tile == 6 || d->force_tile == 7) ||
              (tiles < 256 && nchunks <= 192 && pl.bk == 32 && d->force_tile == 0 &&
               ((Mp <= 512 && nchunks / (nchunks >= 64 ? 8 : 4) >= 8) || nchunks >= 128)))) {
    // Few rows and a deep K (ResNet layer4 at batch 1, FPN lateral / output 5, P6/P7, the box heads' 1024-wide FC layers): K is
    // split over the waves of a workgroup that owns a 32x32 tile (conv_wavek_kernel) -- no slabs, no reduce launch.  Eight waves
    // once a wave's share would exceed 16 chunks.  Measured per layer against the slab form (rocprofv3, 640x640 trunk,
    // profiles/r03_*): it wins or ties where a wave gets >= 8 chunks and the row count is small (layer4 conv2 25 against 38 us,
    // the FC layers equal with one launch less); with many rows (layer2/3: 32x32 tiles re-read the weights per tile) or a
    // shallow K per wave (layer4 conv3) the slabs are faster (31 against 42 us, 21 against 34 us) and keep the layer.
    pl.wavek = d->force_tile == 6 ? 4 : (d->force_tile == 7 ? 8 : (nchunks >= 64 ? 8 : 4));     // force_tile 6 / 7: benchmarks, tests
    pl.bk = 32;
    pl.nchunks = d->Kpad / 32;
    pl.bm = pl.bn = 32;
    pl.tiles_m = (M + 31) / 32;
    pl.tiles_n = (d->Cout + 31) / 32;
  } else if (tiles < 256 && nchunks >= 8) {
    // Deep-K, few-row GEMMs (the box head's fc1: 320 x 12544 -> 1024, 80 tiles, 392 chunks) are a serial chain of ~1.5 us chunk
    // round trips per workgroup: 7 workgroups per CU instead of 2 shorten the chain 3.5x (105 -> ~35 us on the cascade's critical
    // path) for 4x the slab traffic of a 10 us reduce.
    const int target = (nchunks >= 128 && Mp <= 512) ? 1792 : 512;
    int want = (int)((target + tiles - 1) / tiles);
    int maxs = nchunks / 4;
    splitk = want < maxs ? want : maxs;
    if (splitk < 1) splitk = 1;
  } else if (tiles >= 256 && tiles <= 1024 && d->m_count == nullptr && nchunks >= 18) {
    // A few hundred tiles on 256 CUs: every workgroup is resident at once and a CU works through its workgroups' MFMAs one
    // after the other, so the launch takes ceil(tiles / 256) tile times -- the CenterNet tower's 536 tiles take 3 where 2.09
    // would do.  Split-K makes the units finer: time ~ ceil(tiles * s / 256) / s (+ ~0.12 of a tile for the slab reduce).
    // Measured (tools/conv_bench.py tower, reduce included): 8 556 rows x 256 x 2304: s = 1 122-135 us, 2 109-118, 3 106-113,
    // 4 110.  Static row counts only: a device-side count (the mask passes) is not known here, and their two variants
    // (lazy / all proposals) must walk K in the same order to stay bitwise equal.
    double best = 1e30;
    for (int sct = 1; sct <= 4; ++sct) {
      if (nchunks / sct < 9) break;
      const double est = (double)((tiles * sct + 255) / 256) / sct + (sct > 1 ? 0.12 : 0.0);
      if (est < best - 1e-9) {
        best = est;
        splitk = sct;
      }
    }
  }
  if (splitk > nchunks) splitk = nchunks;
  pl.cps = (nchunks + splitk - 1) / splitk;
  pl.splitk = (nchunks + pl.cps - 1) / pl.cps;
  // The shallow-K pointwise layers of the trunk (conv_pointwise.hip; bitwise the 64x64 kernel's results, so the choice may differ
  // between a batch and its single images).  The planner's own choice takes the launches the generic plan runs as plain 64x64
  // tiles that fill the chip (>= 256 tiles on plan_rows, no slabs): measured per class in profiles/r15_pointwise_layers.txt.
  // K = 256 with one or two 64-column panels (layer1.{1,2}.conv1, layer2.0.conv1) stays generic: a workgroup fetches its whole
  // 64 KB activation tile before its first MFMA and has 1-2 panels to use it for.  Faster at 25 600 rows (18.5 against 20.0 us,
  // 28.1 against 29.9) but not at 51 200 (31.4 against 29.9; 46.3 against 46.8, within the parent's spread).  Of K = 256 only the
  // measured winner goes over: 16 panels and more (layer3's conv3, 17 against 26 us).
  const bool pw_forced = d->force_tile == kForcePointwise && d->force_splitk <= 1;          // check_desc has refused the others
  const bool pw_auto = d->force_tile == 0 && d->force_splitk == 0 && pointwise_eligible(d) && pl.splitk == 1 && !pl.wavek && tiles >= 256 &&
                       !(d->Kpad == 256 && d->Cout < 1024);
  if (pw_forced || pw_auto) {
    // panels per workgroup: as many (up to 4: one fetch of the activation tile serves them all) as leave >= 512 workgroups
    const int panels = d->Cout / 64;
    const long row_tiles = (Mp + 63) / 64;
    // (forced below the 256 tiles of the planner's own choice -- tests: no grid target, so that small shapes walk the panel loop)
    const long want = tiles >= 256 ? 512 : 1;
    int np = 1;
    for (int cand = 4; cand > 1; cand >>= 1)
      if (panels >= cand && row_tiles * ((panels + cand - 1) / cand) >= want) {
        np = cand;
        break;
      }
    pl.pw_np = np;
    pl.tile = 6;
    pl.glds = 0;
    pl.bk = 32;
    pl.nchunks = d->Kpad / 32;
    pl.bm = 64;
    pl.bn = 64 * np;
    pl.tiles_m = (M + 63) / 64;
    pl.tiles_n = (panels + np - 1) / np;
    pl.splitk = 1;
    pl.cps = pl.nchunks;
    pl.wavek = 0;
  }
  // The mask head's 3x3 convs (a ROI list of 14x14 maps under a device-side count): same tile, same plan fields, another row order
  // inside the launch.  The planner's own choice needs the generic plan to be the plain 64x64 / BK 32 kernel without slabs; the
  // forced code takes the slabs away (tests: small shapes).
  const bool border_forced = d->force_tile == kForceBorder && d->force_splitk <= 1;         // check_desc has refused the others
  const bool border_auto = kBorderAuto && d->force_tile == 0 && border_eligible(d) && pl.glds == 0 && pl.tile == 3 && pl.bk == 32 &&
                           pl.splitk == 1 && !pl.wavek;
  if (border_forced) {
    pl.splitk = 1;
    pl.cps = pl.nchunks;
  }
  pl.border = (border_forced || border_auto) ? 1 : 0;
  return pl;
}

int total_rows(const EodConvDesc* d) { return d->levels > 0 ? d->level_off[d->levels] : d->N * d->OH * d->OW; }

int check_desc(const EodConvDesc* d) {
  if (!d || !d->x || !d->w || !d->y) return EOD_ERR_NULL;
  if (d->N <= 0 || d->Cin <= 0 || d->Cout <= 0) return EOD_ERR_BAD_DIMS;
  if (d->levels <= 0 && (d->H <= 0 || d->W <= 0 || d->OH <= 0 || d->OW <= 0)) return EOD_ERR_BAD_DIMS;
  if (d->KH <= 0 || d->KW <= 0 || d->stride <= 0 || d->pad < 0) return EOD_ERR_BAD_DIMS;
  if (d->Kpad % 32 != 0 || d->Kpad < d->KH * d->KW * d->Cin) return EOD_ERR_BAD_DIMS;
  if (d->tap4) {
    if (d->Cin != 4) return EOD_ERR_BAD_DIMS;
  } else {
    if (d->Cin % 32 != 0 || d->Kpad != d->KH * d->KW * d->Cin) return EOD_ERR_BAD_DIMS;
  }
  if (d->levels > 0) {
    // pyramid mode: stride-1 'same' conv over up to 5 level images stored back to back
    if (d->levels > EOD_MAX_LEVELS || d->N != 1 || d->stride != 1 || d->KH != d->KW || d->pad != d->KH / 2 || d->tap4 || d->out_mode != 0 ||
        d->res_mode == 2 || d->level_off[0] != 0)
      return EOD_ERR_BAD_DIMS;
    for (int l = 0; l < d->levels; ++l)
      if (d->level_h[l] <= 0 || d->level_w[l] <= 0 || d->level_off[l + 1] - d->level_off[l] != d->level_h[l] * d->level_w[l])
        return EOD_ERR_BAD_DIMS;
  } else {
    if (d->OH != (d->H + 2 * d->pad - d->KH) / d->stride + 1) return EOD_ERR_BAD_DIMS;
    if (d->OW != (d->W + 2 * d->pad - d->KW) / d->stride + 1) return EOD_ERR_BAD_DIMS;
  }
  // operand buffers are addressed with 32-bit byte offsets (buffer descriptors): < 2 GiB each
  if (d->levels <= 0 && (long)d->N * d->H * d->W * d->Cin >= (1L << 29)) return EOD_ERR_BAD_DIMS;
  if ((long)d->Cout * d->Kpad >= (1L << 29)) return EOD_ERR_BAD_DIMS;
  if (d->KH * d->KW > 64) return EOD_ERR_BAD_DIMS;
  if ((long)total_rows(d) * (d->Cout > d->Cin ? d->Cout : d->Cin) >= (1L << 31)) return EOD_ERR_BAD_DIMS;
  if (d->out_mode == 1 && (d->Cout % 4 != 0)) return EOD_ERR_BAD_DIMS;
  if (d->out_mode == 2) {
    if (d->Cout != 1024 || d->KH != 1 || d->KW != 1 || d->stride != 1 || d->tap4 || d->levels > 0 || d->res_mode != 0 || d->in_relu ||
        d->force_splitk > 1)
      return EOD_ERR_BAD_DIMS;
    if (!d->fuse_w) return EOD_ERR_NULL;
  }
  if (d->out_mode < 0 || d->out_mode > 2) return EOD_ERR_BAD_DIMS;
  if (d->res_mode != 0 && !d->res) return EOD_ERR_NULL;
  if (d->res_mode == 2 && ((d->OH & 1) || (d->OW & 1))) return EOD_ERR_BAD_DIMS;
  if (d->m_count && d->m_unit <= 0) return EOD_ERR_BAD_DIMS;
  if (d->m_segments > 1) {
    // B unit lists back to back: whole images per list, a count per list
    if (!d->m_count || d->levels > 0 || d->out_mode == 2 || d->m_segments > EOD_MAX_BATCH || d->N % d->m_segments != 0)
      return EOD_ERR_BAD_DIMS;
    if (((long)(d->N / d->m_segments) * d->OH * d->OW) % d->m_unit != 0) return EOD_ERR_BAD_DIMS;
  }
  if (d->gate && (d->out_mode != 0 || d->split_n != 0 || d->gn_partial)) return EOD_ERR_BAD_DIMS;
  if (d->gate && d->force_tile != 0 && d->force_tile % 10 != 3 && d->force_tile != 6 && d->force_tile != 7) return EOD_ERR_BAD_DIMS;
  if (d->gate && d->force_tile / 10 == 5) return EOD_ERR_BAD_DIMS;          // no gated epilogue in the bf16x3 kernels
  // ... and in the f16 family only in the 64x64 tile of a call that asks for f16 itself (image mode, no in_relu / tap4)
  if (d->gate && (d->force_tile / 10 == 8 || d->force_tile / 10 == 9) &&
      (d->math != EOD_MATH_F16 + 1 || d->force_tile % 10 != 3 || d->levels > 0 || d->tap4 || d->in_relu))
    return EOD_ERR_BAD_DIMS;
  if (d->math < 0 || d->math > EOD_MATH_F16 + 1) return EOD_ERR_BAD_DIMS;
  if ((d->force_tile / 10 == 8 || d->force_tile / 10 == 9) && d->force_tile % 10 != 3 && d->force_tile % 10 != 4) return EOD_ERR_BAD_DIMS;
  if (d->lds_reserve < 0 || d->lds_reserve > 48 * 1024) return EOD_ERR_BAD_DIMS;
  if (d->force_tile == kForcePointwise && (!pointwise_eligible(d) || d->force_splitk > 1)) return EOD_ERR_BAD_DIMS;
  if (d->force_tile == kForceBorder && (!border_eligible(d) || d->force_splitk > 1)) return EOD_ERR_BAD_DIMS;
  if (d->split_n != 0) {
    if (!d->y2) return EOD_ERR_NULL;
    if (d->split_n < 0 || d->split_n >= d->Cout || d->out_mode != 0 || d->res_mode != 0 || d->levels > 0 || d->gn_partial)
      return EOD_ERR_BAD_DIMS;
  }
  if (d->gn_partial) {
    // statistics for a following GroupNorm: pyramid mode, static row count, plain epilogue, channel groups of a power of two <= 64
    const int cpg = d->gn_groups > 0 ? d->Cout / d->gn_groups : 0;
    if (d->levels <= 0 || d->m_count || d->out_mode != 0 || d->gn_groups <= 0 || d->gn_groups > 64 || d->Cout % d->gn_groups != 0 ||
        cpg > 64 || (cpg & (cpg - 1)) != 0 || cpg < 4 || d->Cout % 4 != 0 || d->Cout > 1024 || 256 % (d->Cout / 4) != 0 ||
        64 % (cpg / 4) != 0)
      return EOD_ERR_BAD_DIMS;
  }
  if (!eod_aligned16(d->x) || !eod_aligned16(d->w) || !eod_aligned16(d->w_split) || !eod_aligned16(d->w_half)) return EOD_ERR_ALIGN;
  return EOD_OK;
}

}  // namespace

extern "C" int eod_set_conv_math(int mode) {
  if (mode != EOD_MATH_FP32 && mode != EOD_MATH_BF16X3 && mode != EOD_MATH_F16) return EOD_ERR_BAD_DIMS;
  return math_mode().exchange(mode);
}

extern "C" int eod_get_conv_math(void) { return math_mode().load(); }

extern "C" size_t eod_conv_split_weights_bytes(int Cout, int Kpad) {
  return (Cout > 0 && Kpad > 0 && Kpad % 32 == 0) ? (size_t)Cout * Kpad * 6 : 0;
}

extern "C" int eod_conv_split_weights_bf16x3(const float* w, int Cout, int Kpad, void* out, eod_stream_t stream) {
  if (!w || !out) return EOD_ERR_NULL;
  if (Cout <= 0 || Kpad <= 0 || Kpad % 32 != 0 || (long)Cout * Kpad * 6 >= (1L << 32)) return EOD_ERR_BAD_DIMS;
  if (!eod_aligned16(w) || !eod_aligned16(out)) return EOD_ERR_ALIGN;
  launch_split_weights(w, out, Cout, Kpad, static_cast<hipStream_t>(stream));
  return eod_launch_status();
}

extern "C" size_t eod_conv_half_weights_bytes(int Cout, int Kpad) {
  return (Cout > 0 && Kpad > 0 && Kpad % 32 == 0) ? (size_t)Cout * Kpad * 2 : 0;
}

extern "C" int eod_conv_half_weights(const float* w, int Cout, int Kpad, void* out, eod_stream_t stream) {
  if (!w || !out) return EOD_ERR_NULL;
  if (Cout <= 0 || Kpad <= 0 || Kpad % 32 != 0 || (long)Cout * Kpad >= (1L << 29)) return EOD_ERR_BAD_DIMS;
  if (!eod_aligned16(w) || !eod_aligned16(out)) return EOD_ERR_ALIGN;
  launch_half_weights(w, out, Cout, Kpad, static_cast<hipStream_t>(stream));
  return eod_launch_status();
}

extern "C" int eod_conv2d_gn_fused(const EodConvDesc* d) {
  EodConvDesc t = *d;
  t.gn_partial = nullptr;
  if (check_desc(&t) != EOD_OK) return 0;
  return make_plan(&t, total_rows(&t)).splitk > 1 ? 1 : 0;
}

extern "C" int eod_conv2d_plan(const EodConvDesc* d, EodConvPlan* out) {
  if (!out) return EOD_ERR_NULL;
  const int st = check_desc(d);
  if (st != EOD_OK) return st;
  const Plan pl = make_plan(d, total_rows(d));
  out->tile = pl.tile; out->bm = pl.bm; out->bn = pl.bn; out->bk = pl.bk;
  out->splitk = pl.splitk; out->cps = pl.cps; out->nchunks = pl.nchunks;
  out->wavek = pl.wavek; out->glds = pl.glds;
  out->tiles_m = pl.tiles_m; out->tiles_n = pl.tiles_n;
  out->gn_fused = (d->gn_partial && pl.splitk > 1) ? 1 : 0;
  return EOD_OK;
}

extern "C" size_t eod_conv2d_workspace_bytes(const EodConvDesc* d) {
  if (check_desc(d) != EOD_OK) return 0;
  const int M = total_rows(d);
  const Plan pl = make_plan(d, M);
  if (pl.splitk <= 1) return 0;
  return (size_t)pl.splitk * M * d->Cout * sizeof(float);
}

extern "C" int eod_conv2d(const EodConvDesc* d, eod_stream_t stream) {
  const int st = check_desc(d);
  if (st != EOD_OK) return st;
  hipStream_t s = static_cast<hipStream_t>(stream);
  ConvArgs a{};
  a.x = d->x; a.w = d->w; a.bias = d->bias; a.res = d->res; a.y = d->y;
  a.partial = d->workspace;
  a.m_count = d->m_count; a.m_unit = d->m_unit;
  a.m_segs = d->m_segments > 1 ? d->m_segments : 1;
  a.seg_rows = a.m_segs > 1 ? (d->N / d->m_segments) * d->OH * d->OW : 0;
  a.fuse_w = d->fuse_w; a.out_units = d->out_units; a.fuse_b = d->fuse_b;
  a.N = d->N; a.H = d->H; a.W = d->W; a.Cin = d->Cin; a.OH = d->OH; a.OW = d->OW; a.Cout = d->Cout;
  a.KH = d->KH; a.KW = d->KW; a.stride = d->stride; a.pad = d->pad; a.Kpad = d->Kpad;
  a.M = total_rows(d);
  a.div_ow = eod_make_fastdiv((unsigned)(d->OW > 0 ? d->OW : 1));
  a.div_oh = eod_make_fastdiv((unsigned)(d->OH > 0 ? d->OH : 1));
  a.div_row = eod_make_fastdiv((unsigned)(d->Cout % 4 == 0 ? d->Cout / 4 : d->Cout));   // split-K reduce: work items per output row
  a.div_cd = eod_make_fastdiv((unsigned)((d->Cout >> 2) > 0 ? (d->Cout >> 2) : 1));
  a.div_bh = eod_make_fastdiv((unsigned)(d->OH > 2 ? d->OH - 2 : 1));                        // border-major order: border_row()
  a.div_bw = eod_make_fastdiv((unsigned)(d->OW > 2 ? d->OW - 2 : 1));
  a.div_bi = eod_make_fastdiv((unsigned)(d->OH > 2 && d->OW > 2 ? (d->OH - 2) * (d->OW - 2) : 1));
  {
    const size_t xe = d->levels > 0 ? (size_t)d->level_off[d->levels] * d->Cin : (size_t)d->N * d->H * d->W * d->Cin;
    a.x_bytes = (unsigned)(xe * sizeof(float));
    a.w_bytes = (unsigned)((size_t)d->Cout * d->Kpad * sizeof(float));
    a.w3 = d->w_split;
    a.w3_bytes = (unsigned)((size_t)d->Cout * d->Kpad * 6);
    a.wh = d->w_half;
    a.wh_bytes = (unsigned)((size_t)d->Cout * d->Kpad * 2);
  }
  a.nlv = d->levels > 0 ? d->levels : 0;
  for (int l = 0; l < a.nlv; ++l) {
    a.lv_off[l] = d->level_off[l];
    a.lv_h[l] = d->level_h[l];
    a.lv_w[l] = d->level_w[l];
  }
  if (a.nlv) a.lv_off[a.nlv] = d->level_off[a.nlv];
  a.relu = d->relu; a.res_mode = d->res_mode; a.in_relu = d->in_relu; a.out_mode = d->out_mode;
  a.gate = d->gate;
  a.out_scale = d->out_scale;
  a.gn_partial = d->gn_partial;
  a.gn_groups = d->gn_groups;
  a.y2 = d->y2;
  a.split_n = d->split_n;
  const Plan pl = make_plan(d, a.M);
  if (d->gn_partial && pl.splitk <= 1) return EOD_ERR_BAD_DIMS;      // the statistics ride on the slab reduce (see eod_conv2d_gn_fused)
  a.nchunks = pl.nchunks;
  a.splitk = pl.splitk; a.cps = pl.cps; a.tiles_m = pl.tiles_m; a.tiles_n = pl.tiles_n;
  a.border = pl.border;
  if (pl.splitk > 1) {
    const size_t need = (size_t)pl.splitk * a.M * a.Cout * sizeof(float);
    if (!d->workspace || d->workspace_bytes < need) return EOD_ERR_CAPACITY;
  }
  dim3 grid(pl.tiles_m * pl.tiles_n, pl.splitk);
  if (pl.border) grid.x = (pl.tiles_m + 7) / 8 * 8 * pl.tiles_n;        // row tiles dealt over the XCDs in groups of 8 (conv_claim_tile_border)
  if (pl.pw_np) launch_conv_pointwise(a, pl.pw_np, grid, s);
  else if (pl.wavek) launch_conv_wavek(a, pl.wavek, grid, s);
  else if (pl.glds == 3) launch_conv_f16(a, pl.tile, pl.bk, grid, s);
  else if (pl.glds == 2) launch_conv_bf16x3(a, pl.tile, grid, s);
  else launch_conv_fp32(a, pl.tile, pl.bk, d->tap4 != 0, grid, s, d->lds_reserve, d->prefetch2);
  if (pl.splitk > 1) {
    const size_t total = (size_t)a.M * a.Cout;
    const bool vec = a.Cout % 4 == 0;
    int blocks = (int)((total / (vec ? 4 : 1) + 255) / 256);
    if (blocks > 2048) blocks = 2048;
    if (blocks < 1) blocks = 1;
    if (a.gn_partial) {
      int chunks = 0;
      for (int l = 0; l < a.nlv; ++l) chunks += (a.lv_off[l + 1] - a.lv_off[l] + EOD_GN_ROWS - 1) / EOD_GN_ROWS;
      hipLaunchKernelGGL(conv_splitk_reduce_gn_kernel, dim3(chunks), dim3(256), 0, s, a);
    } else if (vec) hipLaunchKernelGGL(conv_splitk_reduce_kernel<4>, dim3(blocks), dim3(256), 0, s, a);
    else hipLaunchKernelGGL(conv_splitk_reduce_kernel<1>, dim3(blocks), dim3(256), 0, s, a);
  }
  return eod_launch_status();
}
