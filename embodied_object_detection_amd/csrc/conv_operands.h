// Operand addressing of the forward convolution kernels (conv_fp32.hip, conv_bf16x3.hip, conv_f16.hip): everything that happens
// before the first MFMA and does not depend on the arithmetic mode -- which tile a workgroup owns, where a tile row of the
// activation operand starts and which of its filter taps are padding, the weight-row offsets, the walk over the K chunks and the
// masked activation load.  The kernels keep their thread-to-row mapping (lr / lq, rows per pass), staging format, pipeline shape
// and MFMA loop.  All helpers are force-inlined and only read ConvArgs (a helper that wrote to a field would make the compiler
// keep a private copy of the struct in scratch, which the build refuses).
#pragma once
#include "conv_common.h"

namespace eodconv {

// ---- 1. claiming a tile ------------------------------------------------------------------------------
// Row limit M under the device-side count, and the tile this workgroup owns (-1: none).  Only the tiles that hold valid rows do
// work; the XCD remap is taken over THAT count so that a short dynamic row count (e.g. 256 of 320 ROI slots) still spreads evenly
// over the 8 XCDs instead of idling the last ones.  The caller derives tile_m / tile_n / m0 / n0 from the tile id and leaves when
// conv_tile_active() says no: spelled in the kernel, not returned in a struct (the struct form cost the 256x128 f16 kernels 10-16
// VGPRs and a wave of occupancy).
template <int BM>
__device__ __forceinline__ int conv_first_tile(const ConvArgs& p, int& M) {
  M = conv_row_limit(p, p.M);
  const int ntiles = ((M + BM - 1) / BM) * p.tiles_n;
  if ((int)blockIdx.x >= ntiles) return -1;
  return xcd_remap(blockIdx.x, ntiles);
}

// The border-major order (conv_border_order.h) claims its tiles differently.  Its cheap tiles (the border regions: 6 of 9 taps) are
// the first row tiles of the launch; under the contiguous ranges of xcd_remap() the first two XCDs would get all of them and finish
// early while the others take as long as before (measured: 1.4 % slower than pixel-major).  Here row tile r goes to XCD r % 8, its column tiles
// with it (they read the same activation rows), and the LAST row tile is dispatched first: the full interior tiles start first and
// the cheap ones fill the tail.  The grid is rounded up to whole groups of 8 row tiles (eod_conv2d).
template <int BM>
__device__ __forceinline__ bool conv_claim_tile_border(const ConvArgs& p, int& M, int& tile_m, int& tile_n) {
  M = conv_row_limit(p, p.M);
  const int live = (M + BM - 1) / BM;
  const int xcd = blockIdx.x & 7, k = blockIdx.x >> 3;
  const int g = k / p.tiles_n;
  const int r = g * 8 + xcd;
  tile_n = k - g * p.tiles_n;
  tile_m = live - 1 - r;
  return r < live;
}

// Chunks [c_begin, c_end) of share `idx` when the K chunks are dealt out `per` at a time (split-K slab z: per = p.cps; wave-K: a
// wave's share).
__device__ __forceinline__ int conv_chunk_range(const ConvArgs& p, int per, int idx, int& c_end) {
  const int c_begin = idx * per;
  c_end = c_begin + per;
  if (c_end > p.nchunks) c_end = p.nchunks;
  return c_begin;
}

// ---- 2. addressing a tile row of the activation operand -------------------------------------------------
// Output row m as a window into its input image: the window's (ky, kx) = (0, 0) tap sits at pixel (iy0, ix0) of an hh x ww image
// whose first pixel is pixel `off` of the input buffer.  MULTI (pyramid mode): the image is the level that holds row m, stride 1.
// A row without work (rowok false) gets the 1 x 1 image at the origin.
struct RowOrigin {
  int iy0, ix0, off, hh, ww;
};
template <bool MULTI>
__device__ __forceinline__ RowOrigin conv_row_origin(const ConvArgs& p, int m, bool rowok) {
  RowOrigin o = {0, 0, 0, 1, 1};
  if (rowok) {
    if (MULTI) {
      int l = 0;
      while (l + 1 < p.nlv && m >= p.lv_off[l + 1]) ++l;
      const int local = m - p.lv_off[l];
      o.ww = p.lv_w[l];
      o.hh = p.lv_h[l];
      const int oy = local / o.ww;
      o.iy0 = oy - p.pad;
      o.ix0 = (local - oy * o.ww) - p.pad;
      o.off = p.lv_off[l];
    } else {
      const int t = (int)fdiv((unsigned)m, p.div_ow);      // invariant divisors: one mul_hi instead of a division sequence
      const int ox = m - t * p.OW;
      const int img = (int)fdiv((unsigned)t, p.div_oh);
      const int oy = t - img * p.OH;
      o.iy0 = oy * p.stride - p.pad;
      o.ix0 = ox * p.stride - p.pad;
      o.off = img * p.H * p.W;
      o.hh = p.H;
      o.ww = p.W;
    }
  }
  return o;
}

// Logical row m of the border-major order (conv_border_order.h: image mode, `rois` live maps) as a window into its map.
__device__ __forceinline__ RowOrigin conv_row_origin_border(const ConvArgs& p, int m, bool rowok, int rois) {
  RowOrigin o = {0, 0, 0, 1, 1};
  if (rowok) {
    const BorderRow b = border_row(m, rois, p.OH, p.OW, p.div_ow, p.div_bh, p.div_bw, p.div_bi);
    o.iy0 = b.oy * p.stride - p.pad;
    o.ix0 = b.ox * p.stride - p.pad;
    o.off = b.img * p.H * p.W;
    o.hh = p.H;
    o.ww = p.W;
  }
  return o;
}

// Both operand tiles are fetched with SRSRC buffer loads (32-bit byte offsets + hardware range check):
//  * every tile row gets ONE byte offset (its (ky,kx)=(0,0) tap position, plus this thread's float4 column lq) and a bit mask of
//    the taps that fall inside the image, both computed once per workgroup; per chunk a load costs an add, a bit test and a
//    select -- no 64-bit address arithmetic, no exec-mask branches; a masked-off / out-of-tile lane gets offset 0xFFFFFFFF, which
//    the range check turns into zeros (the conv's zero padding);
//  * a weight row's offset never changes: the K position goes into the scalar offset of the instruction.
// `pitch` (bytes per image row of the level) is written in pyramid mode only, where it differs from row to row.
template <bool MULTI>
__device__ __forceinline__ void conv_row_address(const ConvArgs& p, const RowOrigin& o, bool rowok, int lq, unsigned& voff,
                                                 unsigned long long& mask, unsigned& pitch) {
  mask = rowok ? tap_mask(o.iy0, o.ix0, o.hh, o.ww, p.KH, p.KW) : 0ull;
  voff = (unsigned)(((o.off + o.iy0 * o.ww + o.ix0) * p.Cin + 4 * lq) * 4);   // may wrap for padded taps: only used when the tap bit is set
  if (MULTI) pitch = (unsigned)(o.ww * p.Cin * 4);
}
template <bool MULTI>
__device__ __forceinline__ void conv_row_address(const ConvArgs& p, int m, int M, int lq, unsigned& voff, unsigned long long& mask,
                                                 unsigned& pitch) {
  const bool rowok = m < M;
  conv_row_address<MULTI>(p, conv_row_origin<MULTI>(p, m, rowok), rowok, lq, voff, mask, pitch);
}

// ---- 3. weight rows and buffer descriptors ---------------------------------------------------------------
// Byte offset of float4 column lq of weight row n ([Cout][Kpad] fp32); rows past Cout read zeros through the range check.
__device__ __forceinline__ unsigned conv_w_row_offset(const ConvArgs& p, int n, int lq) {
  return n < p.Cout ? (unsigned)((n * p.Kpad + 4 * lq) * 4) : 0xFFFFFFFFu;
}

// Raw buffer descriptor over `bytes` bytes at `ptr`: offsets at or past `bytes` load zeros.
__device__ __forceinline__ __amdgpu_buffer_rsrc_t conv_buffer(const void* ptr, unsigned bytes) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(ptr), 0, bytes, 0x00020000);
}

// ---- 4. walking the K chunks --------------------------------------------------------------------------
// What a chunk's loads need: its filter tap (bit index into the row masks), the tap's image row ky (pyramid mode adds ky * pitch),
// the byte offset of (tap, first channel) relative to a row's (0, 0) tap, and the byte offset of the chunk in a weight row.
struct TapInfo {
  int tap, ky;
  unsigned tap_off, k0b;
};

// next() is called for consecutive chunks (c_begin, c_begin + 1, ...): the (tap, channel) position is advanced instead of
// re-derived with two divisions per chunk (Cin is a multiple of BK, or the chunk never straddles two taps: make_plan).  The fp32
// kernels fetch chunk c + 1 only when it exists; the bf16x3 / f16 pipelines call next() once or twice past c_end: those chunks are
// fetched (range-checked buffer loads) and never used, and `tap` is clamped to 63 so that the shift of the 64-bit row mask stays
// defined for them.  seek() continues the walk at the first chunk of a given tap (image mode; Cin a multiple of BK): the
// border-major order leaves out the taps that are padding for a whole tile.
template <int BK, bool MULTI>
struct ChunkWalker {
  int tap, c0, ky, kx, k0;
  __device__ __forceinline__ ChunkWalker(const ConvArgs& p, int c_begin) {
    k0 = c_begin * BK;
    tap = k0 / p.Cin;
    c0 = k0 - tap * p.Cin;
    ky = tap / p.KW;
    kx = tap - ky * p.KW;
  }
  __device__ __forceinline__ void seek(const ConvArgs& p, int t) {
    tap = t;
    c0 = 0;
    k0 = t * p.Cin;
    ky = t / p.KW;
    kx = t - ky * p.KW;
  }
  __device__ __forceinline__ TapInfo next(const ConvArgs& p) {
    TapInfo ti;
    ti.tap = tap < 63 ? tap : 63;
    ti.ky = ky;
    ti.tap_off = MULTI ? (unsigned)((kx * p.Cin + c0) * 4) : (unsigned)(((ky * p.W + kx) * p.Cin + c0) * 4);
    ti.k0b = (unsigned)(k0 * 4);
    k0 += BK;
    c0 += BK;
    if (c0 >= p.Cin) {
      c0 = 0;
      ++tap;
      if (++kx == p.KW) {
        kx = 0;
        ++ky;
      }
    }
    return ti;
  }
};

// ---- 5. the masked activation load ----------------------------------------------------------------------
// One float4 of a tile row at chunk `ti`: zeros where the tap is padding or the row holds no work.
template <bool MULTI>
__device__ __forceinline__ f32x4 conv_load_a(__amdgpu_buffer_rsrc_t rsrc_x, const TapInfo& ti, unsigned voff, unsigned long long mask,
                                             unsigned pitch) {
  const bool ok = (mask >> ti.tap) & 1ull;
  unsigned vo = voff + ti.tap_off;
  if (MULTI) vo += (unsigned)ti.ky * pitch;
  vo = ok ? vo : 0xFFFFFFFFu;
  return __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rsrc_x, vo, 0, 0));
}

// ConvArgs.in_relu: the ReLU of the producing layer applied on the way in
__device__ __forceinline__ f32x4 conv_relu4(f32x4 v) {
  v.x = fmaxf(v.x, 0.f);
  v.y = fmaxf(v.y, 0.f);
  v.z = fmaxf(v.z, 0.f);
  v.w = fmaxf(v.w, 0.f);
  return v;
}

}  // namespace eodconv
