// The divisor record of fdiv() (eod_common.h) and its host-side constructor.  Plain C++ without HIP headers: the host-only check of
// the border-major row order (conv_border_order.h, tests/test_conv_border_order_cpu.py) compiles it with the system compiler.
#pragma once

struct FastDiv {
  unsigned mp, sh1, sh2, d;
};

static inline FastDiv eod_make_fastdiv(unsigned d) {
  FastDiv f{};
  if (d == 0) d = 1;
  unsigned l = 0;
  while ((1ull << l) < d) ++l;
  f.mp = (unsigned)((((1ull << 32) * ((1ull << l) - d)) / d) + 1);
  f.sh1 = l < 1 ? l : 1;
  f.sh2 = l > 0 ? l - 1 : 0;
  f.d = d;
  return f;
}
