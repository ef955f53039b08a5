#!/usr/bin/env python
"""Micro-benchmark of the implicit-GEMM conv kernel on the shapes of the hot path (GPU box only).  `modes`: the per-layer table of
the three arithmetic modes (fp32 / bf16x3 / f16) with the planner's own choice.  `border`: the mask head's 3x3 GEMM under a device-side
ROI count in the pixel-major (force_tile 13) and the border-major row order (force_tile 43), back to back."""
import sys, os, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from embodied_object_detection_amd import ops

dev = torch.device("cuda:0")
g = torch.Generator().manual_seed(0)

def bench(name, N, H, W, Cin, Cout, k, stride, pad, tiles=(0, 1, 2, 3), splitks=(0,), deconv=False, iters=20, prefetch2=0):
    x = torch.randn((N, H, W, Cin), generator=g).to(dev)
    if deconv:
        w = torch.randn((Cin, Cout, 2, 2), generator=g) * 0.05
        conv = ops.Conv(w, torch.zeros(Cout), device=dev, deconv=True)
        flops = 2.0 * N * H * W * Cin * Cout * 4
    else:
        w = torch.randn((Cout, Cin, k, k), generator=g) * 0.05
        conv = ops.Conv(w, torch.zeros(Cout), stride=stride, pad=pad, device=dev)
        OH, OW = conv.out_hw(H, W)
        flops = 2.0 * N * OH * OW * Cout * Cin * k * k
        conv.prefetch2 = prefetch2
    for t in tiles:
        for sk in splitks:
            try:
                out = conv(x, N, H, W, relu=True, force_tile=t, force_splitk=sk)
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(iters):
                    conv(x, N, H, W, relu=True, force_tile=t, force_splitk=sk, out=out)
                e1.record()
                torch.cuda.synchronize()
                ms = e0.elapsed_time(e1) / iters
                print(f"{name:28s} tile={t} splitk={sk}  {ms*1e3:9.1f} us  {flops/ms/1e9:7.1f} TFLOP/s", flush=True)
            except Exception as ex:
                print(name, t, sk, "ERR", ex)

F16_PEAK, HBM_TBS = 2516.0, 8.0      # dense f16 MFMA TFLOP/s (16 x the fp32 MFMA's 157) and HBM TB/s of the chip


def modes(name, N, H, W, Cin, Cout, k, stride, pad, iters=30):
    """One layer with the planner's own choice in the three arithmetic modes: time, plan, and for f16 the fraction of the f16 MFMA peak
    next to the fraction of the HBM rate its least traffic (fp32 activations in and out, half weights) would need in that time."""
    x = torch.randn((N, H, W, Cin), generator=g).to(dev)
    w = torch.randn((Cout, Cin, k, k), generator=g) * 0.05
    conv = ops.Conv(w, torch.zeros(Cout), stride=stride, pad=pad, device=dev)
    OH, OW = conv.out_hw(H, W)
    flops = 2.0 * N * OH * OW * Cout * Cin * k * k
    least = 4.0 * N * H * W * Cin + 4.0 * N * OH * OW * Cout + 2.0 * Cout * Cin * k * k
    cols = []
    for mode in ("fp32", "bf16x3", "f16"):
        prev = ops.set_conv_math(mode)
        try:
            out = conv(x, N, H, W, relu=True)
            for _ in range(3):
                conv(x, N, H, W, relu=True, out=out)
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(iters):
                conv(x, N, H, W, relu=True, out=out)
            e1.record()
            torch.cuda.synchronize()
            p = conv.plan()
        finally:
            ops.set_conv_math(prev)
        us = e0.elapsed_time(e1) / iters * 1e3
        kern = f"wave-K {p['wavek']}" if p["wavek"] else f"{p['bm']}x{p['bn']} BK{p['bk']}" + (f" sk{p['splitk']}" if p["splitk"] > 1 else "")
        cols.append((mode, us, kern))
    us16 = cols[2][1]
    tf, tb = flops / us16 / 1e6, least / us16 / 1e6
    bound = "HBM-bound" if tb / HBM_TBS > 4 * tf / F16_PEAK and tb / HBM_TBS > 0.25 else ("latency / launch" if us16 < 15 else "mixed")
    print(f"{name:26s} " + "  ".join(f"{m} {us:7.1f} us ({kern})" for m, us, kern in cols) +
          f"  | f16 {tf:6.1f} TFLOP/s = {tf / F16_PEAK * 100:4.1f} % of the f16 peak, >= {tb:4.2f} TB/s = {tb / HBM_TBS * 100:4.1f} % of HBM: {bound};"
          f" x{cols[0][1] / us16:.2f} of fp32, x{cols[1][1] / us16:.2f} of bf16x3", flush=True)


def backward(name, N, H, W, Cin, Cout, k, stride, pad, iters=20):
    """One backbone layer's backward in fp32 and in f16 arithmetic (`ops.ConvBackward(conv, math=)`): the weight-gradient launch alone
    (reduce of the position ranges included) and the gated + residual input-gradient launch alone."""
    conv = ops.Conv(torch.randn((Cout, Cin, k, k), generator=g) * 0.05, torch.zeros(Cout), stride=stride, pad=pad, device=dev)
    OH, OW = conv.out_hw(H, W)
    x = torch.relu(torch.randn((N, H, W, Cin), generator=g)).to(dev)
    gr = torch.randn((N, OH, OW, Cout), generator=g).to(dev)
    res = torch.randn((N, H, W, Cin), generator=g).to(dev)

    def timed(fn):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / iters * 1e3
    t = {}
    for math in (None, "f16"):
        bw = ops.ConvBackward(conv, math=math)
        both = timed(lambda: bw(x, None, gr, dx_res=res, dx_gate=x))
        wg = timed(lambda: bw(x, None, gr, need_dx=False))
        t[math] = (wg, both - wg, bw._flipped.plan())
    p32, p16 = t[None][2], t["f16"][2]
    kern = lambda p: ("f16 " if p["glds"] == 3 else "") + (f"wave-K {p['wavek']}" if p["wavek"] else f"{p['bm']}x{p['bn']}") + (f" sk{p['splitk']}" if p["splitk"] > 1 else "")
    print(f"{name:26s} wgrad fp32 {t[None][0]:7.1f} us  f16 {t['f16'][0]:7.1f} us  x{t[None][0] / t['f16'][0]:.2f} | gated dgrad fp32 {t[None][1]:7.1f} us "
          f"({kern(p32)})  f16 {t['f16'][1]:7.1f} us ({kern(p16)})  x{t[None][1] / t['f16'][1]:.2f}", flush=True)


def border_skipped_share(rois, oh=14, ow=14):
    """Share of a border-order launch's (tile, tap) pairs whose tap is zero padding for every row of the 64-row tile = the share of
    MFMA work it leaves out, counted from the order itself (csrc/conv_border_order.h)."""
    import numpy as np
    oy, ox = [], []
    for y in (0, oh - 1):                                   # top rows of all maps, then bottom rows
        oy.append(np.full(rois * ow, y)); ox.append(np.tile(np.arange(ow), rois))
    for x in (0, ow - 1):                                   # left columns without corners, then right columns
        oy.append(np.tile(np.arange(1, oh - 1), rois)); ox.append(np.full(rois * (oh - 2), x))
    iy, ix = np.divmod(np.arange((oh - 2) * (ow - 2)), ow - 2)
    oy.append(np.tile(iy + 1, rois)); ox.append(np.tile(ix + 1, rois))
    oy, ox = np.concatenate(oy), np.concatenate(ox)
    ky, kx = np.divmod(np.arange(9), 3)
    live = ((oy[:, None] - 1 + ky >= 0) & (oy[:, None] - 1 + ky < oh) & (ox[:, None] - 1 + kx >= 0) & (ox[:, None] - 1 + kx < ow))
    tiles = [live[m0:m0 + 64].any(axis=0) for m0 in range(0, len(oy), 64)]
    return 1.0 - float(np.mean(tiles))


def border(rois, cap, Cin=256, Cout=256, iters=50, rounds=5):
    """mask_fcn GEMM (14x14 maps, 3x3, Cin -> Cout) on `rois` of `cap` ROI slots: both row orders alternating, `rounds` times."""
    x = torch.randn((cap, 14, 14, Cin), generator=g).to(dev)
    conv = ops.Conv(torch.randn((Cout, Cin, 3, 3), generator=g) * 0.02, torch.zeros(Cout), stride=1, pad=1, device=dev)
    count = torch.tensor([rois], dtype=torch.int32, device=dev)
    out = torch.empty((cap, 14, 14, Cout), device=dev)
    t = {13: [], 43: []}
    for _ in range(rounds):
        for ft in (13, 43):
            for _w in range(5):
                conv(x, cap, 14, 14, relu=True, m_count=count, m_unit=196, out=out, force_tile=ft, force_splitk=1)
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _i in range(iters):
                conv(x, cap, 14, 14, relu=True, m_count=count, m_unit=196, out=out, force_tile=ft, force_splitk=1)
            e1.record()
            torch.cuda.synchronize()
            t[ft].append(e0.elapsed_time(e1) / iters * 1e3)
    a, b = sorted(t[13])[rounds // 2], sorted(t[43])[rounds // 2]
    flops = 2.0 * rois * 196 * Cout * Cin * 9
    print(f"mask_fcn {rois:3d} of {cap:3d} rois  pixel-major {a:7.1f} us ({min(t[13]):.1f}-{max(t[13]):.1f}, {flops / a / 1e6:5.1f} TFLOP/s)  "
          f"border-major {b:7.1f} us ({min(t[43]):.1f}-{max(t[43]):.1f})  measured -{(1 - b / a) * 100:4.1f} %  "
          f"skipped chunk share {border_skipped_share(rois) * 100:4.1f} %", flush=True)


which = sys.argv[1] if len(sys.argv) > 1 else "all"
if which == "border":
    for rois, cap in ((43, 128), (88, 300), (300, 300)):
        border(rois, cap)
    sys.exit(0)
if which == "backward":
    # the backbone's layers of one 640x640 training step: weight gradient and gated input gradient, fp32 against f16 arithmetic
    for sh in [("l1 conv1 1x1 256->64", 1, 160, 160, 256, 64, 1, 1, 0), ("l1 conv2 3x3 64->64", 1, 160, 160, 64, 64, 3, 1, 1),
               ("l1 conv3 1x1 64->256", 1, 160, 160, 64, 256, 1, 1, 0), ("l2 conv1 1x1 512->128", 1, 80, 80, 512, 128, 1, 1, 0),
               ("l2 conv2 3x3 128->128", 1, 80, 80, 128, 128, 3, 1, 1), ("l2 conv2 3x3 s2 (block 0)", 1, 160, 160, 128, 128, 3, 2, 1),
               ("l2 conv3 1x1 128->512", 1, 80, 80, 128, 512, 1, 1, 0), ("l2 downsample 1x1 s2", 1, 160, 160, 256, 512, 1, 2, 0),
               ("l3 conv1 1x1 1024->256", 1, 40, 40, 1024, 256, 1, 1, 0), ("l3 conv2 3x3 256->256", 1, 40, 40, 256, 256, 3, 1, 1),
               ("l3 conv3 1x1 256->1024", 1, 40, 40, 256, 1024, 1, 1, 0), ("l4 conv1 1x1 2048->512", 1, 20, 20, 2048, 512, 1, 1, 0),
               ("l4 conv2 3x3 512->512", 1, 20, 20, 512, 512, 3, 1, 1), ("l4 conv3 1x1 512->2048", 1, 20, 20, 512, 2048, 1, 1, 0),
               ("fpn lateral3 1x1 512->256", 1, 80, 80, 512, 256, 1, 1, 0), ("fpn out3 3x3 256 80x80", 1, 80, 80, 256, 256, 3, 1, 1),
               ("fpn out5 3x3 256 20x20", 1, 20, 20, 256, 256, 3, 1, 1), ("p6 3x3 s2 256 20x20", 1, 20, 20, 256, 256, 3, 2, 1)]:
        backward(*sh)
    sys.exit(0)
if which == "modes":
    # the layers of one 640x640 frame (ResNet-50 trunk, FPN, tower, box and mask heads) in fp32 / bf16x3 / f16 arithmetic
    for sh in [("l1 conv1 1x1 256->64", 1, 160, 160, 256, 64, 1, 1, 0), ("l1 conv2 3x3 64->64", 1, 160, 160, 64, 64, 3, 1, 1),
               ("l1 conv3 1x1 64->256", 1, 160, 160, 64, 256, 1, 1, 0), ("l2 conv1 1x1 512->128", 1, 80, 80, 512, 128, 1, 1, 0),
               ("l2 conv2 3x3 128->128", 1, 80, 80, 128, 128, 3, 1, 1), ("l2 conv3 1x1 128->512", 1, 80, 80, 128, 512, 1, 1, 0),
               ("l3 conv1 1x1 1024->256", 1, 40, 40, 1024, 256, 1, 1, 0), ("l3 conv2 3x3 256->256", 1, 40, 40, 256, 256, 3, 1, 1),
               ("l3 conv3 1x1 256->1024", 1, 40, 40, 256, 1024, 1, 1, 0), ("l4 conv1 1x1 2048->512", 1, 20, 20, 2048, 512, 1, 1, 0),
               ("l4 conv2 3x3 512->512", 1, 20, 20, 512, 512, 3, 1, 1), ("l4 conv3 1x1 512->2048", 1, 20, 20, 512, 2048, 1, 1, 0),
               ("fpn out3 3x3 256 80x80", 1, 80, 80, 256, 256, 3, 1, 1), ("tower-like 3x3 256 92x93", 1, 92, 93, 256, 256, 3, 1, 1),
               ("fc1 256x12544->1024", 256, 1, 1, 12544, 1024, 1, 1, 0), ("fc2 256x1024->1024", 256, 1, 1, 1024, 1024, 1, 1, 0),
               ("mask_fcn 43 rois", 43, 14, 14, 256, 256, 3, 1, 1), ("mask_fcn 92 rois", 92, 14, 14, 256, 256, 3, 1, 1),
               ("mask_fcn 300 rois", 300, 14, 14, 256, 256, 3, 1, 1)]:
        modes(*sh)
    sys.exit(0)
if which == "pipe":
    # pipeline variants of the 64x64 kernel (EodConvDesc.prefetch2: 0 default, 2 = double-buffered LDS) on shapes of the frame
    shapes = [("stem-like l1 conv1 256->64", 1, 160, 160, 256, 64, 1, 1, 0), ("l1 conv2 3x3 64->64", 1, 160, 160, 64, 64, 3, 1, 1),
              ("l1 conv3 64->256", 1, 160, 160, 64, 256, 1, 1, 0), ("l2 conv2 3x3 128->128", 1, 80, 80, 128, 128, 3, 1, 1),
              ("l2 conv3 128->512", 1, 80, 80, 128, 512, 1, 1, 0), ("l3 conv1 1024->256", 1, 40, 40, 1024, 256, 1, 1, 0),
              ("l3 conv2 3x3 256->256", 1, 40, 40, 256, 256, 3, 1, 1), ("l3 conv3 256->1024", 1, 40, 40, 256, 1024, 1, 1, 0),
              ("fpn out3 3x3 256", 1, 80, 80, 256, 256, 3, 1, 1), ("fc1 256 rois", 256, 1, 1, 12544, 1024, 1, 1, 0),
              ("mask_fcn 43 rois", 43, 14, 14, 256, 256, 3, 1, 1), ("mask_fcn 92 rois", 92, 14, 14, 256, 256, 3, 1, 1),
              ("mask_fcn 300 rois", 300, 14, 14, 256, 256, 3, 1, 1)]
    for sh in shapes:
        for pf in (0, 2):
            bench(f"{sh[0]} pipe={pf}", *sh[1:], tiles=(0,), iters=30, prefetch2=pf)
    sys.exit(0)
if which == "propmask":
    # the proposal-mask pass (~43 ROIs) and the de-duplicated detection pass (~100 ROIs): 64x64 tiles against the wave-split-K kernel
    for rois in (43, 100, 300):
        bench(f"mask_fcn {rois} rois", rois, 14, 14, 256, 256, 3, 1, 1, tiles=(13, 12, 6, 7), iters=30)
        bench(f"mask_fcn {rois} rois prefetch2", rois, 14, 14, 256, 256, 3, 1, 1, tiles=(13,), iters=30, prefetch2=1)
    sys.exit(0)
if which == "masktiles":
    bench("mask_fcn 300 rois", 300, 14, 14, 256, 256, 3, 1, 1, tiles=(13, 12, 11, 13, 12), iters=30)
    bench("mask_fcn 45 rois", 45, 14, 14, 256, 256, 3, 1, 1, tiles=(13, 12, 11), iters=30)
if which == "tower":
    bench("tower-like 3x3 256 92x93", 1, 92, 93, 256, 256, 3, 1, 1, tiles=(13,), splitks=(1, 2, 3, 4, 6, 1, 2, 3), iters=40)
    bench("prop-mask 45 rois", 45, 14, 14, 256, 256, 3, 1, 1, tiles=(13,), splitks=(1, 2, 3, 4, 1, 2), iters=40)
if which in ("all", "mask"):
    bench("mask_fcn 256 rois", 256, 14, 14, 256, 256, 3, 1, 1, tiles=(3, 23, 13, 22, 21))
    bench("mask_fcn 300 rois", 300, 14, 14, 256, 256, 3, 1, 1, tiles=(23, 13, 22, 21))
    bench("deconv 256 rois", 256, 14, 14, 256, 256, 2, 1, 0, deconv=True, tiles=(3, 2, 23, 22, 21))
if which in ("all", "resnet"):
    bench("l1 conv2 3x3 64 160x160", 1, 160, 160, 64, 64, 3, 1, 1)
    bench("l1 conv3 1x1 64->256", 1, 160, 160, 64, 256, 1, 1, 0)
    bench("l2 conv2 3x3 128 80x80", 1, 80, 80, 128, 128, 3, 1, 1)
    bench("l3 conv2 3x3 256 40x40", 1, 40, 40, 256, 256, 3, 1, 1, splitks=(0, 1, 2, 4))
    bench("l4 conv2 3x3 512 20x20", 1, 20, 20, 512, 512, 3, 1, 1, splitks=(0, 1, 4, 8))
    bench("l4 conv3 1x1 512->2048", 1, 20, 20, 512, 2048, 1, 1, 0, splitks=(0, 1, 2))
    bench("tower 3x3 256 80x80", 1, 80, 80, 256, 256, 3, 1, 1)
    bench("fc1 256x12544->1024", 256, 1, 1, 12544, 1024, 1, 1, 0, tiles=(0, 2, 3), splitks=(0, 4, 7, 14))
    bench("fc2 256x1024->1024", 256, 1, 1, 1024, 1024, 1, 1, 0, tiles=(0, 3), splitks=(0, 1, 2, 4))
