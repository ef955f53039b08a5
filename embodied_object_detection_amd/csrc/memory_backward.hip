// The training step's backward kernels that are not a convolution's weight gradient (those: conv_wgrad.hip):
//   * backward of the memory READ: gradients of the three `map_merge_projection` 1x1 convolutions and of the cascaded average pools
//     of `CustomRecurrentFPN.forward` (Detic/detic/modeling/backbone/timm.py:142-192), below;
//   * AdamW with detectron2's clip by value, for one tensor and for many in one launch, and the loss scaler's non-finite pass;
//   * backward of the FPN top-down add (upsample), of the trunk's 3x3 s2 max pool and of ReLU;
//   * the rotation of a layer's weights for its input-gradient convolution.
//
// The memory read (the part of `forward_model`, custom_rcnn.py:584-679, that is specific to the spatial memory).  Forward, per level
// l = 3, 4, 5:
//
//   E_l = half(avg_pool2(float(E_{l-1})))          E_2 := avg_pool4(float(memory[proj]))  (fp32)
//   out_l = (conv1x1(float(E_l); W_l, b_l) * weight) + P_l
//
// Given G_l = dL/d out_l ([P_l, 256] rows, NHWC):
//   dW_l[co][ci] = weight * sum_pos G_l[pos][co] * E_l[pos][ci]      db_l[co] = weight * sum_pos G_l[pos][co]         (kernel 1)
//   dEc_l[pos][ci] = weight * sum_co G_l[pos][co] * W_l[co][ci]       a 1x1 convolution with the transposed weights: eod_conv2d
//   pools (autograd semantics of the fp16 casts: a gradient that flows into a half tensor is rounded to half, two contributions
//   to one half tensor are added in half):                                                                              (kernel 2)
//     gE_5 = half(dEc_5)
//     gE_4 = half(dEc_4) +h half(up2(float(gE_5)) / 4)
//     gE_3 = half(dEc_3) +h half(up2(float(gE_4)) / 4)
//     gE_2 = up2(float(gE_3)) / 4                                    (fp32, [H/4 * W/4, 512])
// The memory table itself is an input of the reference's training step (loaded from disk, loader.py:199-223), not a parameter: no
// gradient flows below E_2.
//
// Kernel 1 is the direct scheme of wgrad_common.h: a workgroup owns one 32x32 tile of dW_l, its four waves take a quarter of the
// positions each and are added in wave order (deterministic).
#include "wgrad_common.h"
#include <algorithm>
#include "../../include/eod_hip.h"
#include <hip/hip_fp16.h>
#include <cmath>
#include <cstdlib>

namespace {

// pooled rows in the operand-fragment order eod_memory_gather_pool writes (include/eod_hip.h):
// [32-row tile][k-step s<32][hi<2][r<32][8] halves = element (row 32*tile + r, channel 16 s + 8 hi + j)
__device__ __forceinline__ size_t frag_half_offset(int tile32, int r, int c8) {
  return ((((size_t)tile32 * 32 + (c8 >> 1)) * 2 + (c8 & 1)) * 32 + r) * 8;
}

struct BwdArgs {
  const float* g[3];        // G_l [P_l, 256]
  const __half* pooled;     // E_3..E_5, fragment order, each level on a tile boundary
  float* dw[3];             // [256, 512]
  float* db[3];             // [256]
  int rows[3];              // P_l
  int tile_base[3];         // first 32-row tile of level l in `pooled`
  float weight;
  // splits > 1 (blockIdx.z): the positions of a level are cut into `splits` ranges, each writing its own partial dW / db into
  // part [level][splits][256 * 512] / bpart [level][splits][256]; wgrad_reduce_kernel adds them in range order.  Without it the 128
  // workgroups of the finest level each walk all of its 6 400 positions (290 us at 640x640).
  int splits;
  float* part;
  float* bpart;
};

__global__ __launch_bounds__(256) void proj_backward_weights_kernel(BwdArgs a) {
  const int level = blockIdx.y;
  const int tile = blockIdx.x;              // 8 (co) x 16 (ci) tiles of 32x32
  const int co0 = (tile >> 4) * 32, ci0 = (tile & 15) * 32;
  const float* __restrict__ G = a.g[level];
  const int col = threadIdx.x & 31;
  const int ci = ci0 + col;
  wgrad_direct_tile(
      a, a.rows[level],
      [&](int pos, float& gv, float& xv) {
        gv = G[(size_t)pos * 256 + co0 + col];
        xv = __half2float(a.pooled[frag_half_offset(a.tile_base[level] + (pos >> 5), pos & 31, ci >> 3) + (ci & 7)]);
      },
      [&](float*& dst, float*& db_tile) {
        float *dw, *db;
        wgrad_outputs(a, (size_t)level * a.splits + blockIdx.z, 256 * 512, 256, a.dw[level], a.db[level], dw, db);
        dst = dw + (size_t)co0 * 512 + ci;
        db_tile = (tile & 15) == 0 ? db + co0 : nullptr;
      },
      512, a.weight);
}

struct PoolBwdArgs {
  const float* dec[3];      // dEc_3, dEc_4, dEc_5: [P_l, 512] fp32 rows
  __half* ge[3];            // gE_3, gE_4, gE_5: [P_l, 512] half rows
  float* ge2;               // [(H/4) * (W/4), 512] fp32
  int h2, w2;               // H / 4, W / 4
};

__device__ __forceinline__ float round_half(float v) { return __half2float(__float2half_rn(v)); }

// one thread per (position of the H/4 x W/4 grid, channel): it recomputes the chain of its P5 / P4 / P3 ancestors (pointwise) and
// stores the levels whose top-left corner it is
__global__ __launch_bounds__(256) void pool_backward_kernel(PoolBwdArgs a) {
  const size_t total = (size_t)a.h2 * a.w2 * 512;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int c = (int)(i & 511);
    const int p = (int)(i >> 9);
    const int y = p / a.w2, x = p - y * a.w2;
    const int w3 = a.w2 >> 1, w4 = a.w2 >> 2, w5 = a.w2 >> 3;
    const size_t p3 = (size_t)(y >> 1) * w3 + (x >> 1), p4 = (size_t)(y >> 2) * w4 + (x >> 2), p5 = (size_t)(y >> 3) * w5 + (x >> 3);
    const float g5 = round_half(a.dec[2][p5 * 512 + c]);
    const float g4 = round_half(round_half(a.dec[1][p4 * 512 + c]) + round_half(g5 * 0.25f));
    const float g3 = round_half(round_half(a.dec[0][p3 * 512 + c]) + round_half(g4 * 0.25f));
    a.ge2[i] = g3 * 0.25f;
    if (((y | x) & 1) == 0) a.ge[0][p3 * 512 + c] = __float2half_rn(g3);
    if (((y | x) & 3) == 0) a.ge[1][p4 * 512 + c] = __float2half_rn(g4);
    if (((y | x) & 7) == 0) a.ge[2][p5 * 512 + c] = __float2half_rn(g5);
  }
}

// torch.optim.AdamW, single-tensor form (the reference trains with SOLVER.OPTIMIZER ADAMW, Base-C2_L_R5021k_640b64_4x_recurrent.yaml:69),
// preceded by detectron2's per-parameter clip_grad_value_ (SOLVER.CLIP_GRADIENTS.ENABLED, CLIP_TYPE "value"):
//   g = clamp(g, -clip, clip);  p *= 1 - lr wd;  m += (g - m)(1 - b1);  v = v b2 + (1 - b2) g g;
//   p += -step_size * (m / (sqrt(v) / bc2_sqrt + eps)),   step_size = lr / (1 - b1^t), bc2_sqrt = sqrt(1 - b2^t) (host, double)
__global__ __launch_bounds__(256) void adamw_step_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                          float* __restrict__ v, size_t n, float decay, float one_minus_b1, float b2,
                                                          float one_minus_b2, float step_size, float bc2_sqrt, float eps, float clip) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    float gi = g[i];
    if (clip > 0.f) gi = fminf(fmaxf(gi, -clip), clip);
    float pi = p[i] * decay;
    float mi = m[i];
    mi = mi + (gi - mi) * one_minus_b1;
    const float vi = v[i] * b2 + one_minus_b2 * (gi * gi);
    const float denom = sqrtf(vi) / bc2_sqrt + eps;
    pi = pi + (-step_size) * (mi / denom);
    p[i] = pi;
    m[i] = mi;
    v[i] = vi;
  }
}

// The same update for up to ADAMW_MULTI tensors in ONE launch (the training step has 126 parameter tensors: 126 launches of a few
// microseconds each were 4 % of the iteration's kernel time and 126 launch boundaries).  The tensors' constants travel in the
// kernel arguments; a workgroup finds its tensor by the prefix of the tensors' workgroup counts.  Element for element the
// arithmetic of adamw_step_kernel.
#define ADAMW_MULTI 20
struct AdamWMulti {
  float* p[ADAMW_MULTI];
  const float* g[ADAMW_MULTI];
  float* m[ADAMW_MULTI];
  float* v[ADAMW_MULTI];
  unsigned long long n[ADAMW_MULTI];
  float decay[ADAMW_MULTI], step_size[ADAMW_MULTI], bc2_sqrt[ADAMW_MULTI];
  unsigned block_end[ADAMW_MULTI];     // exclusive end of tensor t's workgroups
  // optional: the stepped value times a per-row factor, written to a second matrix (a trunk conv's raw master -> the layer's weights
  // with its FrozenBatchNorm folded in: timm.py:277-299 keeps weight / bias of the norm as buffers, not parameters)
  float* folded[ADAMW_MULTI];
  const float* row_scale[ADAMW_MULTI];
  unsigned cols[ADAMW_MULTI], ld_out[ADAMW_MULTI];
  unsigned grad_of_folded;             // bit t: g is the gradient of the FOLDED weights (x row_scale = the master's, chain rule)
  int count;
  float one_minus_b1, b2, one_minus_b2, eps, clip;
  // loss scaler (EodAdamWTensor.inv_scale / found_inf): g is multiplied by inv_scale[t] first (0 = off); with `found_inf` the whole
  // launch leaves everything as it is when the flag is set (GradScaler.step skipping optimizer.step)
  float inv_scale[ADAMW_MULTI];
  const int* found_inf;
};

__global__ __launch_bounds__(256) void adamw_multi_kernel(AdamWMulti a) {
  int t = 0;
  while (t + 1 < a.count && blockIdx.x >= a.block_end[t]) ++t;
  const unsigned first = t ? a.block_end[t - 1] : 0u;
  const size_t nb = a.block_end[t] - first;
  float* __restrict__ p = a.p[t];
  const float* __restrict__ g = a.g[t];
  float* __restrict__ m = a.m[t];
  float* __restrict__ v = a.v[t];
  const size_t n = a.n[t];
  const float decay = a.decay[t], step_size = a.step_size[t], bc2_sqrt = a.bc2_sqrt[t];
  float* __restrict__ folded = a.folded[t];
  const float* __restrict__ rs = a.row_scale[t];
  const unsigned cols = a.cols[t], ldo = a.ld_out[t];
  const bool gscale = (a.grad_of_folded >> t) & 1u;
  const float inv = a.inv_scale[t];
  if (a.found_inf && *a.found_inf != 0) return;
  for (size_t i = (size_t)(blockIdx.x - first) * blockDim.x + threadIdx.x; i < n; i += nb * blockDim.x) {
    float gi = g[i];
    if (inv != 0.f) gi *= inv;
    if (gscale) gi *= rs[(unsigned)(i / cols)];
    if (a.clip > 0.f) gi = fminf(fmaxf(gi, -a.clip), a.clip);
    float pi = p[i] * decay;
    float mi = m[i];
    mi = mi + (gi - mi) * a.one_minus_b1;
    const float vi = v[i] * a.b2 + a.one_minus_b2 * (gi * gi);
    const float denom = sqrtf(vi) / bc2_sqrt + a.eps;
    pi = pi + (-step_size) * (mi / denom);
    p[i] = pi;
    m[i] = mi;
    v[i] = vi;
    if (folded) {
      const unsigned r = (unsigned)(i / cols), c = (unsigned)(i - (size_t)r * cols);
      folded[(size_t)r * ldo + c] = pi * rs[r];
    }
  }
}

// The loss scaler's found-inf pass over up to FINITE_MULTI gradient tensors in one launch (the check entries of eod_adamw_step_multi):
// *flag = 1 when any element is inf or NaN (exponent all ones).  Every writer stores the same value: no atomics, no order.
#define FINITE_MULTI 32
struct FiniteMulti {
  const float* g[FINITE_MULTI];
  unsigned long long n[FINITE_MULTI];
  unsigned block_end[FINITE_MULTI];
  int count;
  int* flag;
};

__global__ __launch_bounds__(256) void grads_nonfinite_kernel(FiniteMulti a) {
  int t = 0;
  while (t + 1 < a.count && blockIdx.x >= a.block_end[t]) ++t;
  const unsigned first = t ? a.block_end[t - 1] : 0u;
  const size_t nb = a.block_end[t] - first;
  const unsigned* __restrict__ g = reinterpret_cast<const unsigned*>(a.g[t]);
  const size_t n = a.n[t];
  bool bad = false;
  for (size_t i = (size_t)(blockIdx.x - first) * blockDim.x + threadIdx.x; i < n; i += nb * blockDim.x)
    bad |= (g[i] & 0x7F800000u) == 0x7F800000u;
  if (bad) *a.flag = 1;
}

// FPN top-down add (timm.py:128-133: lateral + nearest x2 of the coarser level): the coarser level's gradient is the sum over each
// 2x2 block of the finer level's gradient (the lateral branch gets the gradient itself).  g [N,2h,2w,C] -> out [N,h,w,C] (+= when
// accumulate: the coarser level also has its own output-conv branch).
__global__ __launch_bounds__(256) void upsample2_backward_kernel(const float* __restrict__ g, float* __restrict__ out, int N, int h, int w,
                                                                  int C4, int accumulate) {
  const size_t total = (size_t)N * h * w * C4;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int c = (int)(i % C4);
    size_t t = i / C4;
    const int x = (int)(t % w);
    t /= w;
    const int y = (int)(t % h), n = (int)(t / h);
    const f32x4* gp = reinterpret_cast<const f32x4*>(g);
    const size_t r0 = ((size_t)(n * 2 * h + 2 * y) * (2 * w) + 2 * x) * C4 + c, r1 = r0 + (size_t)2 * w * C4;
    f32x4 v = gp[r0];
    v += gp[r0 + C4];
    v += gp[r1];
    v += gp[r1 + C4];
    f32x4* op = reinterpret_cast<f32x4*>(out) + i;
    if (accumulate) v += *op;
    *op = v;
  }
}

// timm ResNet maxpool 3x3 s2 p1 (timm.py:281) backward: every input position collects the gradient of the output windows whose
// maximum it is -- the FIRST maximum of a window in row-major tap order, as torch's max_pool2d backward routes it.  Gather form
// (no atomics): x [N,H,W,C], y / g [N,OH,OW,C] -> dx [N,H,W,C].
__global__ __launch_bounds__(256) void maxpool3x3s2_backward_kernel(const float* __restrict__ x, const float* __restrict__ y,
                                                                     const float* __restrict__ g, float* __restrict__ dx, int N, int H, int W,
                                                                     int C, int OH, int OW) {
  const size_t total = (size_t)N * H * W * C;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int c = (int)(i % C);
    size_t t = i / C;
    const int ix = (int)(t % W);
    t /= W;
    const int iy = (int)(t % H), n = (int)(t / H);
    const float xv = x[i];
    float acc = 0.f;
    // output windows that contain (iy, ix): oy in {ceil((iy - 1) / 2) .. floor((iy + 1) / 2)}: one for an even row, two for an odd one
    for (int oy = (iy + 1) / 2 - (iy & 1); oy <= (iy + 1) / 2; ++oy) {
      if (oy < 0 || oy >= OH) continue;
      for (int ox = (ix + 1) / 2 - (ix & 1); ox <= (ix + 1) / 2; ++ox) {
        if (ox < 0 || ox >= OW) continue;
        const size_t o = ((size_t)(n * OH + oy) * OW + ox) * C + c;
        if (y[o] != xv) continue;
        // am I the first tap of this window (row-major) that holds the maximum?
        bool first = true;
        for (int ky = 0; ky < 3 && first; ++ky) {
          const int yy = oy * 2 - 1 + ky;
          if (yy < 0 || yy >= H) continue;
          for (int kx = 0; kx < 3; ++kx) {
            const int xx = ox * 2 - 1 + kx;
            if (xx < 0 || xx >= W) continue;
            if (yy == iy && xx == ix) {
              ky = 3;
              break;
            }
            if (x[((size_t)(n * H + yy) * W + xx) * C + c] == xv) {
              first = false;
              break;
            }
          }
        }
        if (first) acc += g[o];
      }
    }
    dx[i] = acc;
  }
}

// dL/d(pre-activation) of a ReLU layer from dL/d(output): g where the output was positive
__global__ __launch_bounds__(256) void relu_backward_kernel(const float* __restrict__ g, const float* __restrict__ y, float* __restrict__ out,
                                                             size_t n4) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (size_t)gridDim.x * blockDim.x) {
    const f32x4 gv = reinterpret_cast<const f32x4*>(g)[i];
    const f32x4 yv = reinterpret_cast<const f32x4*>(y)[i];
    f32x4 o;
    o.x = yv.x > 0.f ? gv.x : 0.f;
    o.y = yv.y > 0.f ? gv.y : 0.f;
    o.z = yv.z > 0.f ? gv.z : 0.f;
    o.w = yv.w > 0.f ? gv.w : 0.f;
    reinterpret_cast<f32x4*>(out)[i] = o;
  }
}

}  // namespace

extern "C" int eod_upsample2_sum_backward(const float* g, float* out, int N, int h, int w, int C, int accumulate, eod_stream_t stream) {
  if (!g || !out) return EOD_ERR_NULL;
  if (N <= 0 || h <= 0 || w <= 0 || C <= 0 || (C & 3)) return EOD_ERR_BAD_DIMS;
  if (!eod_aligned16(g) || !eod_aligned16(out)) return EOD_ERR_ALIGN;
  const size_t total = (size_t)N * h * w * (C >> 2);
  size_t blocks = (total + 255) / 256;
  if (blocks > 8192) blocks = 8192;
  hipLaunchKernelGGL(upsample2_backward_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, g, out, N, h, w, C >> 2, accumulate);
  return eod_launch_status();
}

extern "C" int eod_maxpool3x3s2_backward(const float* x, const float* y, const float* g, float* dx, int N, int H, int W, int C, int OH,
                                         int OW, eod_stream_t stream) {
  if (!x || !y || !g || !dx) return EOD_ERR_NULL;
  if (N <= 0 || H <= 0 || W <= 0 || C <= 0 || OH != (H + 2 - 3) / 2 + 1 || OW != (W + 2 - 3) / 2 + 1) return EOD_ERR_BAD_DIMS;
  const size_t total = (size_t)N * H * W * C;
  size_t blocks = (total + 255) / 256;
  if (blocks > 8192) blocks = 8192;
  hipLaunchKernelGGL(maxpool3x3s2_backward_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, x, y, g, dx, N, H, W, C, OH, OW);
  return eod_launch_status();
}

extern "C" int eod_relu_backward(const float* g, const float* y, float* out, size_t n, eod_stream_t stream) {
  if (!g || !y || !out) return EOD_ERR_NULL;
  if (n == 0 || (n & 3)) return EOD_ERR_BAD_DIMS;
  if (!eod_aligned16(g) || !eod_aligned16(y) || !eod_aligned16(out)) return EOD_ERR_ALIGN;
  size_t blocks = (n / 4 + 255) / 256;
  if (blocks > 8192) blocks = 8192;
  hipLaunchKernelGGL(relu_backward_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, g, y, out, n / 4);
  return eod_launch_status();
}

extern "C" int eod_adamw_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, size_t n, double lr, double beta1,
                              double beta2, double eps, double weight_decay, int step, double clip_value, eod_stream_t stream) {
  if (!param || !grad || !exp_avg || !exp_avg_sq) return EOD_ERR_NULL;
  if (n == 0 || step < 1 || !(lr >= 0.0) || !(beta1 >= 0.0 && beta1 < 1.0) || !(beta2 >= 0.0 && beta2 < 1.0)) return EOD_ERR_BAD_DIMS;
  const double bc1 = 1.0 - pow(beta1, (double)step), bc2 = 1.0 - pow(beta2, (double)step);
  size_t blocks = (n + 255) / 256;
  if (blocks > 4096) blocks = 4096;
  hipLaunchKernelGGL(adamw_step_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, param, grad, exp_avg, exp_avg_sq, n,
                     (float)(1.0 - lr * weight_decay), (float)(1.0 - beta1), (float)beta2, (float)(1.0 - beta2), (float)(lr / bc1),
                     (float)sqrt(bc2), (float)eps, (float)clip_value);
  return eod_launch_status();
}

// The weights of a layer's input-gradient convolution (dX = conv of dY with the 180-degree rotated, in/out-transposed kernel), from the
// layer's packed forward weights: out[ci][(ky', kx', co)] = w[co][(KH-1-ky', KW-1-kx', ci)].  One launch per layer after an optimizer
// step (torch's flip + permute + copy were three).
__global__ __launch_bounds__(256) void rotate_weights_kernel(const float* __restrict__ w, int Cout, int KH, int KW, int Cin, int ld_in,
                                                              float* __restrict__ out, int ld_out) {
  const size_t n = (size_t)Cin * KH * KW * Cout;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    const int co = (int)(i % Cout);
    size_t r = i / Cout;
    const int kx = (int)(r % KW);
    r /= KW;
    const int ky = (int)(r % KH);
    const int ci = (int)(r / KH);
    out[(size_t)ci * ld_out + ((size_t)ky * KW + kx) * Cout + co] =
        w[(size_t)co * ld_in + ((size_t)(KH - 1 - ky) * KW + (KW - 1 - kx)) * Cin + ci];
  }
}

extern "C" int eod_conv_rotate_weights(const float* w, int Cout, int KH, int KW, int Cin, int ld_in, float* out, int ld_out,
                                       eod_stream_t stream) {
  if (!w || !out) return EOD_ERR_NULL;
  if (Cout <= 0 || KH <= 0 || KW <= 0 || Cin <= 0 || ld_in < KH * KW * Cin || ld_out < KH * KW * Cout) return EOD_ERR_BAD_DIMS;
  size_t blocks = ((size_t)Cin * KH * KW * Cout + 255) / 256;
  if (blocks > 2048) blocks = 2048;
  hipLaunchKernelGGL(rotate_weights_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, w, Cout, KH, KW, Cin, ld_in, out, ld_out);
  return eod_launch_status();
}

// The rotation for up to ROTATE_MULTI layers in one launch: after an optimizer step every layer with an input-gradient convolution
// needs it (74 layers of the recurrent detector: 74 launches of ~9 us were 4 % of the iteration).
#define ROTATE_MULTI 24
struct RotateMulti {
  const float* w[ROTATE_MULTI];
  float* out[ROTATE_MULTI];
  int Cout[ROTATE_MULTI], KH[ROTATE_MULTI], KW[ROTATE_MULTI], Cin[ROTATE_MULTI], ld_in[ROTATE_MULTI], ld_out[ROTATE_MULTI];
  unsigned block_end[ROTATE_MULTI];
  int count;
};

// Per tap the rotation is a (co, ci) -> (ci, co) transpose: a workgroup moves one 32 x 32 tile of one tap through LDS, reading rows of
// w along ci and writing rows of out along co (both coalesced; the element-per-thread form reads with a stride of a weight row).
__global__ __launch_bounds__(256) void rotate_weights_multi_kernel(RotateMulti a) {
  __shared__ float tile[32][33];
  int t = 0;
  while (t + 1 < a.count && blockIdx.x >= a.block_end[t]) ++t;
  const unsigned b = blockIdx.x - (t ? a.block_end[t - 1] : 0u);
  const float* __restrict__ w = a.w[t];
  float* __restrict__ out = a.out[t];
  const int Cout = a.Cout[t], KH = a.KH[t], KW = a.KW[t], Cin = a.Cin[t], ld_in = a.ld_in[t], ld_out = a.ld_out[t];
  const unsigned tiles_ci = (unsigned)(Cin + 31) >> 5, tiles_co = (unsigned)(Cout + 31) >> 5;
  const unsigned tap = b / (tiles_co * tiles_ci), rem = b - tap * tiles_co * tiles_ci;
  const int co0 = (int)(rem / tiles_ci) * 32, ci0 = (int)(rem % tiles_ci) * 32;
  const int ky = (int)tap / KW, kx = (int)tap - ky * KW;
  const int src_tap = (KH - 1 - ky) * KW + (KW - 1 - kx);
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int co = co0 + ty + 8 * j, ci = ci0 + tx;
    tile[ty + 8 * j][tx] = (co < Cout && ci < Cin) ? w[(size_t)co * ld_in + (size_t)src_tap * Cin + ci] : 0.f;
  }
  __syncthreads();
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int ci = ci0 + ty + 8 * j, co = co0 + tx;
    if (ci < Cin && co < Cout) out[(size_t)ci * ld_out + (size_t)tap * Cout + co] = tile[tx][ty + 8 * j];
  }
}

extern "C" int eod_conv_rotate_weights_multi(const EodRotateTensor* tensors, int count, eod_stream_t stream) {
  if (!tensors) return EOD_ERR_NULL;
  if (count < 1) return EOD_ERR_BAD_DIMS;
  for (int i = 0; i < count; ++i) {
    const EodRotateTensor& t = tensors[i];
    if (!t.w || !t.out) return EOD_ERR_NULL;
    if (t.Cout <= 0 || t.KH <= 0 || t.KW <= 0 || t.Cin <= 0 || t.ld_in < t.KH * t.KW * t.Cin || t.ld_out < t.KH * t.KW * t.Cout)
      return EOD_ERR_BAD_DIMS;
  }
  for (int i0 = 0; i0 < count; i0 += ROTATE_MULTI) {
    RotateMulti a{};
    a.count = std::min(ROTATE_MULTI, count - i0);
    unsigned blocks = 0;
    for (int k = 0; k < a.count; ++k) {
      const EodRotateTensor& t = tensors[i0 + k];
      a.w[k] = t.w; a.out[k] = t.out;
      a.Cout[k] = t.Cout; a.KH[k] = t.KH; a.KW[k] = t.KW; a.Cin[k] = t.Cin; a.ld_in[k] = t.ld_in; a.ld_out[k] = t.ld_out;
      blocks += (unsigned)((size_t)t.KH * t.KW * ((t.Cout + 31) >> 5) * ((t.Cin + 31) >> 5));     // one 32 x 32 tile each
      a.block_end[k] = blocks;
    }
    hipLaunchKernelGGL(rotate_weights_multi_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, a);
  }
  return eod_launch_status();
}

extern "C" int eod_adamw_step_multi(const EodAdamWTensor* tensors, int count, double beta1, double beta2, double eps, double clip_value,
                                    eod_stream_t stream) {
  if (!tensors) return EOD_ERR_NULL;
  if (count < 1 || !(beta1 >= 0.0 && beta1 < 1.0) || !(beta2 >= 0.0 && beta2 < 1.0)) return EOD_ERR_BAD_DIMS;
  // check entries (param == NULL; all entries of a call or none): the loss scaler's found-inf pass, nothing is stepped
  int checks = 0;
  for (int i = 0; i < count; ++i) checks += tensors[i].param ? 0 : 1;
  if (checks) {
    int* flag = tensors[0].found_inf;
    if (checks != count) return EOD_ERR_BAD_DIMS;
    if (!flag) return EOD_ERR_NULL;
    for (int i = 0; i < count; ++i) {
      if (!tensors[i].grad) return EOD_ERR_NULL;
      if (tensors[i].n == 0 || tensors[i].found_inf != flag) return EOD_ERR_BAD_DIMS;
    }
    for (int i0 = 0; i0 < count; i0 += FINITE_MULTI) {
      FiniteMulti f{};
      f.count = std::min(FINITE_MULTI, count - i0);
      f.flag = flag;
      unsigned blocks = 0;
      for (int k = 0; k < f.count; ++k) {
        const EodAdamWTensor& t = tensors[i0 + k];
        f.g[k] = t.grad; f.n[k] = t.n;
        size_t nb = (t.n + 1023) / 1024;
        if (nb > 1024) nb = 1024;
        blocks += (unsigned)nb;
        f.block_end[k] = blocks;
      }
      hipLaunchKernelGGL(grads_nonfinite_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, f);
    }
    return eod_launch_status();
  }
  for (int i = 0; i < count; ++i) {
    const EodAdamWTensor& t = tensors[i];
    if (t.found_inf != tensors[0].found_inf || !(t.inv_scale >= 0.f)) return EOD_ERR_BAD_DIMS;
    if (!t.param || !t.grad || !t.exp_avg || !t.exp_avg_sq) return EOD_ERR_NULL;
    if (t.n == 0 || t.step < 1 || !(t.lr >= 0.0)) return EOD_ERR_BAD_DIMS;
    if (t.folded_out && (!t.row_scale || t.cols <= 0 || t.ld_out < t.cols || t.n % (size_t)t.cols != 0)) return EOD_ERR_BAD_DIMS;
    if (t.grad_of_folded && (!t.row_scale || t.cols <= 0 || t.n % (size_t)t.cols != 0)) return EOD_ERR_BAD_DIMS;
  }
  for (int i0 = 0; i0 < count; i0 += ADAMW_MULTI) {
    AdamWMulti a{};
    a.count = std::min(ADAMW_MULTI, count - i0);
    a.one_minus_b1 = (float)(1.0 - beta1); a.b2 = (float)beta2; a.one_minus_b2 = (float)(1.0 - beta2); a.eps = (float)eps;
    a.clip = (float)clip_value;
    unsigned blocks = 0;
    for (int k = 0; k < a.count; ++k) {
      const EodAdamWTensor& t = tensors[i0 + k];
      const double bc1 = 1.0 - pow(beta1, (double)t.step), bc2 = 1.0 - pow(beta2, (double)t.step);
      a.p[k] = t.param; a.g[k] = t.grad; a.m[k] = t.exp_avg; a.v[k] = t.exp_avg_sq; a.n[k] = t.n;
      a.folded[k] = t.folded_out; a.row_scale[k] = t.row_scale; a.cols[k] = (unsigned)t.cols; a.ld_out[k] = (unsigned)t.ld_out;
      if (t.grad_of_folded) a.grad_of_folded |= 1u << k;
      a.inv_scale[k] = t.inv_scale;
      a.found_inf = t.found_inf;
      a.decay[k] = (float)(1.0 - t.lr * t.weight_decay);
      a.step_size[k] = (float)(t.lr / bc1);
      a.bc2_sqrt[k] = (float)sqrt(bc2);
      size_t nb = (t.n + 1023) / 1024;                  // four elements per thread and pass
      if (nb > 1024) nb = 1024;
      blocks += (unsigned)nb;
      a.block_end[k] = blocks;
    }
    hipLaunchKernelGGL(adamw_multi_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, a);
  }
  return eod_launch_status();
}

#define PROJ_WGRAD_SPLITS 8
extern "C" size_t eod_memory_project_backward_weights_workspace_bytes(void) {
  return wgrad_workspace_bytes(PROJ_WGRAD_SPLITS, 3, 256 * 512, 256);
}

static int memory_project_backward_weights_impl(const float* g3, const float* g4, const float* g5, const uint16_t* pooled_f16, int H,
                                                int W, float weight, float* dw3, float* db3, float* dw4, float* db4, float* dw5,
                                                float* db5, void* workspace, size_t workspace_bytes, eod_stream_t stream);

extern "C" int eod_memory_project_backward_weights(const float* g3, const float* g4, const float* g5, const uint16_t* pooled_f16, int H,
                                                   int W, float weight, float* dw3, float* db3, float* dw4, float* db4, float* dw5,
                                                   float* db5, eod_stream_t stream) {
  return memory_project_backward_weights_impl(g3, g4, g5, pooled_f16, H, W, weight, dw3, db3, dw4, db4, dw5, db5, nullptr, 0, stream);
}

extern "C" int eod_memory_project_backward_weights_ws(const float* g3, const float* g4, const float* g5, const uint16_t* pooled_f16, int H,
                                                      int W, float weight, float* dw3, float* db3, float* dw4, float* db4, float* dw5,
                                                      float* db5, void* workspace, size_t workspace_bytes, eod_stream_t stream) {
  if (!workspace || workspace_bytes < eod_memory_project_backward_weights_workspace_bytes()) return EOD_ERR_CAPACITY;
  return memory_project_backward_weights_impl(g3, g4, g5, pooled_f16, H, W, weight, dw3, db3, dw4, db4, dw5, db5, workspace,
                                              workspace_bytes, stream);
}

static int memory_project_backward_weights_impl(const float* g3, const float* g4, const float* g5, const uint16_t* pooled_f16, int H,
                                                int W, float weight, float* dw3, float* db3, float* dw4, float* db4, float* dw5,
                                                float* db5, void* workspace, size_t workspace_bytes, eod_stream_t stream) {
  if (!g3 || !g4 || !g5 || !pooled_f16 || !dw3 || !db3 || !dw4 || !db4 || !dw5 || !db5) return EOD_ERR_NULL;
  if (H <= 0 || W <= 0 || (H & 31) || (W & 31)) return EOD_ERR_BAD_DIMS;
  BwdArgs a{};
  a.g[0] = g3; a.g[1] = g4; a.g[2] = g5;
  a.pooled = reinterpret_cast<const __half*>(pooled_f16);
  a.dw[0] = dw3; a.dw[1] = dw4; a.dw[2] = dw5;
  a.db[0] = db3; a.db[1] = db4; a.db[2] = db5;
  int base = 0;
  for (int l = 0; l < 3; ++l) {
    a.rows[l] = (H >> (3 + l)) * (W >> (3 + l));
    a.tile_base[l] = base;
    base += (a.rows[l] + 31) / 32;
  }
  a.weight = weight;
  return wgrad_launch_ranges(a, PROJ_WGRAD_SPLITS, workspace, workspace_bytes, 3, 256 * 512, 256, a.dw, a.db, (hipStream_t)stream, [&] {
    hipLaunchKernelGGL(proj_backward_weights_kernel, dim3(128, 3, a.splits), dim3(256), 0, (hipStream_t)stream, a);
  });
}

extern "C" int eod_memory_pool_backward(const float* dec3, const float* dec4, const float* dec5, int H, int W, uint16_t* ge3_f16,
                                        uint16_t* ge4_f16, uint16_t* ge5_f16, float* ge2, eod_stream_t stream) {
  if (!dec3 || !dec4 || !dec5 || !ge3_f16 || !ge4_f16 || !ge5_f16 || !ge2) return EOD_ERR_NULL;
  if (H <= 0 || W <= 0 || (H & 31) || (W & 31)) return EOD_ERR_BAD_DIMS;
  PoolBwdArgs a{};
  a.dec[0] = dec3; a.dec[1] = dec4; a.dec[2] = dec5;
  a.ge[0] = reinterpret_cast<__half*>(ge3_f16); a.ge[1] = reinterpret_cast<__half*>(ge4_f16); a.ge[2] = reinterpret_cast<__half*>(ge5_f16);
  a.ge2 = ge2;
  a.h2 = H >> 2; a.w2 = W >> 2;
  const size_t total = (size_t)a.h2 * a.w2 * 512;
  size_t blocks = (total + 255) / 256;
  if (blocks > 8192) blocks = 8192;
  hipLaunchKernelGGL(pool_backward_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, a);
  return eod_launch_status();
}
