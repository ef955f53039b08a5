// The border-major row order of the 64x64 fp32 convolution kernel (conv_fp32.hip, PIPE 3) as a pure function.
//
// A 3x3 / stride 1 / pad 1 launch over R live maps of OH x OW pixels (a ROI list under a device-side count) may deal its logical
// rows by border class across ALL maps instead of pixel by pixel: first the top image rows of every map (R * OW logical rows), then
// the bottom rows, then what is left of the left columns (R * (OH - 2)), of the right columns, then the interior pixels.  Every row
// of the first four regions has the same three filter taps in the zero padding (ky = 0, ky = 2, kx = 0, kx = 2), so a 64-row tile
// that lies inside one region can leave those taps' K chunks out.  border_row() is the bijection logical row -> (map, oy, ox); the
// kernel uses it for the row origin and for the storage row of the epilogue, nothing outside one launch sees the order.  Host and
// device run the same arithmetic: this file needs no HIP header, and tests/test_conv_border_order_cpu.py compiles it as it is.
#pragma once
#include "fastdiv.h"

#if defined(__HIPCC__)
#define EOD_BORDER_FN __host__ __device__ __forceinline__
#else
#define EOD_BORDER_FN static inline
#endif

namespace eodconv {

struct BorderRow {
  int img, oy, ox;
};
EOD_BORDER_FN unsigned border_fdiv(unsigned n, const FastDiv& f) {      // fdiv(), also for the host
  const unsigned t = (unsigned)(((unsigned long long)f.mp * n) >> 32);
  return (t + ((n - t) >> f.sh1)) >> f.sh2;
}
// `d_ow`, `d_bh`, `d_bw`, `d_bi`: divisors OW, OH - 2, OW - 2, (OH - 2) * (OW - 2); OH, OW >= 3; 0 <= m < R * OH * OW
EOD_BORDER_FN BorderRow border_row(int m, int R, int OH, int OW, const FastDiv& d_ow, const FastDiv& d_bh, const FastDiv& d_bw,
                                   const FastDiv& d_bi) {
  const int rows = R * OW, cols = R * (OH - 2);
  BorderRow b;
  if (m < 2 * rows) {                          // top rows of all maps, then bottom rows
    const bool bottom = m >= rows;
    const int l = bottom ? m - rows : m;
    b.img = (int)border_fdiv((unsigned)l, d_ow);
    b.ox = l - b.img * OW;
    b.oy = bottom ? OH - 1 : 0;
  } else if (m < 2 * rows + 2 * cols) {        // left columns without their corners, then right columns
    const int l0 = m - 2 * rows;
    const bool right = l0 >= cols;
    const int l = right ? l0 - cols : l0;
    b.img = (int)border_fdiv((unsigned)l, d_bh);
    b.oy = 1 + l - b.img * (OH - 2);
    b.ox = right ? OW - 1 : 0;
  } else {                                     // interior pixels, map by map
    const int l = m - 2 * rows - 2 * cols;
    b.img = (int)border_fdiv((unsigned)l, d_bi);
    const int rem = l - b.img * (OH - 2) * (OW - 2);
    const int q = (int)border_fdiv((unsigned)rem, d_bw);
    b.oy = 1 + q;
    b.ox = 1 + rem - q * (OW - 2);
  }
  return b;
}

}  // namespace eodconv
