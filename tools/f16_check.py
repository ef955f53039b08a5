#!/usr/bin/env python
"""Accuracy (against fp64 convolutions of the unrounded and of the half-rounded operands) and speed of the f16 kernels next to the
fp32-MFMA and bf16x3 kernels (GPU box only).  force_tile: 0 / 23 fp32, 53 / 54 bf16x3 64x64 / 256x128, 93 / 94 f16 64x64 / 256x128 with BK = 32 (the
planner's), 83 / 84 the same with BK = 64."""
import sys, os
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn.functional as F
from embodied_object_detection_amd import ops

dev = torch.device("cuda:0")
g = torch.Generator().manual_seed(0)
F16_PEAK = 2516.0      # dense f16 MFMA TFLOP/s of the chip (16 x the 157 of the fp32 MFMA)


def accuracy(N, H, W, Cin, Cout, k, pad, tiles):
    x = torch.randn((N, Cin, H, W), generator=g)
    w = torch.randn((Cout, Cin, k, k), generator=g) * (1.0 / (Cin * k * k)) ** 0.5
    b = torch.randn((Cout,), generator=g)
    ref = F.conv2d(x.double(), w.double(), b.double(), padding=pad)
    refh = F.conv2d(x.half().double(), w.half().double(), b.double(), padding=pad)     # what the f16 kernels are to compute
    scale = ref.abs().mean().item()
    conv = ops.Conv(w, b, stride=1, pad=pad, device=dev)
    xd = x.permute(0, 2, 3, 1).contiguous().to(dev)
    out = {}
    for t in tiles:
        y = conv(xd, N, H, W, force_tile=t, force_splitk=1).cpu().permute(0, 3, 1, 2).double()
        e, eh = (y - ref).abs(), (y - refh).abs()
        out[t] = f"vs fp64 {e.max().item() / scale:.2e} / {e.mean().item() / scale:.2e}  vs fp64 of rounded {eh.max().item() / scale:.2e} / {eh.mean().item() / scale:.2e}"
    e = (F.conv2d(x.half().float(), w.half().float(), b, padding=pad).double() - refh).abs()
    out["cpu fp32 on rounded"] = f"{e.max().item() / scale:.2e} / {e.mean().item() / scale:.2e}"
    return out


def speed(name, N, H, W, Cin, Cout, k, stride, pad, tiles, iters=30):
    x = torch.randn((N, H, W, Cin), generator=g).to(dev)
    w = torch.randn((Cout, Cin, k, k), generator=g) * 0.05
    conv = ops.Conv(w, torch.zeros(Cout), stride=stride, pad=pad, device=dev)
    OH, OW = conv.out_hw(H, W)
    flops = 2.0 * N * OH * OW * Cout * Cin * k * k
    # what one pass moves at least: fp32 activations in and out, half weights
    bytes_min = 4.0 * N * H * W * Cin + 4.0 * N * OH * OW * Cout + 2.0 * Cout * Cin * k * k
    for t in tiles:
        out = conv(x, N, H, W, relu=True, force_tile=t)
        for _ in range(3):
            conv(x, N, H, W, relu=True, force_tile=t, out=out)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            conv(x, N, H, W, relu=True, force_tile=t, out=out)
        e1.record()
        torch.cuda.synchronize()
        ms = e0.elapsed_time(e1) / iters
        p = conv.plan()
        print(f"{name:28s} tile={t:3d} {p['bm']:3d}x{p['bn']:3d} BK{p['bk']} sk{p['splitk']}  {ms*1e3:8.1f} us  {flops/ms/1e9:7.1f} TFLOP/s "
              f"({flops/ms/1e9/F16_PEAK*100:4.1f} % of the f16 peak)  >= {bytes_min/ms/1e9:6.2f} TB/s", flush=True)


if __name__ == "__main__":
    print("relative error (max / mean; normalised by mean |y|)")
    for label, args in (("3x3 256->256 K=2304", (8, 14, 14, 256, 256, 3, 1)), ("1x1 2048->256", (1, 20, 20, 2048, 256, 1, 0)),
                        ("fc 12544->128", (64, 1, 1, 12544, 128, 1, 0)), ("3x3 32->64 (BK 32)", (2, 30, 30, 32, 64, 3, 1))):
        for k, v in accuracy(*args, tiles=(23, 53, 83, 84, 93, 94)).items():
            print(f"{label:22s} {str(k):20s} {v}", flush=True)
    T = (0, 53, 54, 83, 84, 93, 94)
    speed("mask_fcn 256 rois", 256, 14, 14, 256, 256, 3, 1, 1, tiles=T + T)
    speed("mask_fcn 300 rois", 300, 14, 14, 256, 256, 3, 1, 1, tiles=T)
    speed("tower 3x3 256 80x80", 1, 80, 80, 256, 256, 3, 1, 1, tiles=T)
    speed("l1 conv1 1x1 256->64", 1, 160, 160, 256, 64, 1, 1, 0, tiles=T)
    speed("l1 conv2 3x3 64 160x160", 1, 160, 160, 64, 64, 3, 1, 1, tiles=T)
    speed("l1 conv3 1x1 64->256", 1, 160, 160, 64, 256, 1, 1, 0, tiles=T)
    speed("l2 conv2 3x3 128 80x80", 1, 80, 80, 128, 128, 3, 1, 1, tiles=T)
    speed("l3 conv2 3x3 256 40x40", 1, 40, 40, 256, 256, 3, 1, 1, tiles=(0, 53, 83, 93))
    speed("l4 conv2 3x3 512 20x20", 1, 20, 20, 512, 512, 3, 1, 1, tiles=(0, 53, 83, 93))
    speed("l4 conv3 1x1 512->2048", 1, 20, 20, 512, 2048, 1, 1, 0, tiles=(0, 53, 83, 93))
    speed("fc1 256x12544->1024", 256, 1, 1, 12544, 1024, 1, 1, 0, tiles=(0, 53, 83, 93))
