"""Helpers the two production-plan modules share (test_conv_plans_gpu.py: the forward launches; test_conv_backward_plans_gpu.py:
the backward launches)."""
from typing import Tuple

SENTINEL = -777.0


def plan_in(conv, mode):
    """The plan of the layer's last descriptor in `mode`, with the process's mode put back."""
    from embodied_object_detection_amd import ops
    prev = ops.set_conv_math(mode)
    try:
        return conv.plan()
    finally:
        ops.set_conv_math(prev)


def exact_hw(M: int) -> Tuple[int, int]:
    """An image of exactly M positions, as square as M's divisors allow."""
    h = int(M ** 0.5)
    while M % h:
        h -= 1
    return h, M // h


# Ceiling on mean |y - ref64| / mean |ref64| of a convolution that does not depend on the CPU's own summation order
# (tests/test_kernels_gpu.py, test_conv_bf16x3_accuracy): 3e-6 up to K = 4608, 1e-5 up to the box head's fc1 (K = 12544).
def ceiling(K: int) -> float:
    assert K <= 12544, K
    return 3e-6 if K <= 4608 else 1e-5
