"""Vocabulary width against speed: frames/s through `model([episode])` at 640x640 (200x200 grid) for 20, 80, 365 and 1203 classes
(same weights, class matrix sliced from tests/golden/lvis_v1_clip.npy), and event-timed microseconds of one classifier stage, of
`memory_scores` and of both selections, launch alone, at each width.

    python tools/vocab_bench.py [--out profiles/vocab_bench.txt] [--frames 40]
"""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
LVIS = os.path.join(ROOT, "tests", "golden", "lvis_v1_clip.npy")


def class_matrix(C: int) -> torch.Tensor:
    w = torch.tensor(np.load(LVIS), dtype=torch.float32)[:C].t().contiguous()
    return F.normalize(torch.cat([w, w.new_zeros((512, 1))], dim=1), p=2, dim=0).contiguous()


def timed_us(fn, iters: int = 50, warm: int = 5) -> float:
    """Median over `iters` single launches, each between two events on an otherwise idle stream."""
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1e3)
    return float(np.median(ts))


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--frames", type=int, default=40)
    args = ap.parse_args()
    from embodied_object_detection_amd import build_model, ops, setup_cfg
    from embodied_object_detection_amd.checkpoint import synthetic_state_dict
    from embodied_object_detection_amd.data.synthetic import SyntheticSequence
    from embodied_object_detection_amd.modeling import reset_cls_test
    dev = torch.device("cuda:0")
    lines = ["classes  frames/s  classifier_stage_us  memory_scores_us  det_select_us(topk 100)  mem_select_us(thr 0.3)"]
    sd = synthetic_state_dict(0)
    cfg = setup_cfg(None, ["MODEL.MEMORY_TYPE", "implicit_memory", "MODEL.MAP_FEAT_FUSION", "sum", "MODEL.MAP_FEATURE_WEIGHT", 5])
    model = build_model(cfg, sd)
    seq = SyntheticSequence(0, H=640, W=640, n_frames=args.frames + 10, map_w=200, map_h=200, cell=0.5)
    frames = [seq.frame(i) for i in range(args.frames + 10)]
    R = 256
    g = torch.Generator().manual_seed(1)
    feat = torch.randn((R, 512), generator=g).to(dev)
    ps = torch.rand((R,), generator=g).to(dev)
    ctr = torch.rand((R, 2), generator=g) * 600
    boxes = torch.cat([ctr, ctr + 20 + torch.rand((R, 2), generator=g) * 200], dim=1).to(dev)
    cnt = torch.tensor([200], dtype=torch.int32, device=dev)
    for C in (20, 80, 365, 1203):
        zs = class_matrix(C)
        reset_cls_test(model, zs[:, :C], C)
        model([frames[:10]])
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        model([frames[10:]])
        b.record()
        b.synchronize()
        fps = args.frames / (a.elapsed_time(b) * 1e-3)
        C1 = C + 1
        zd = zs.to(dev)
        prob, featn = torch.zeros((R, C1), device=dev), torch.zeros((R, 512), device=dev)
        t_cls = timed_us(lambda: ops.zs_classify(feat, zd, prob, False, featn, cnt, R, C1, wide=True))
        scores = torch.zeros((R, C1), device=dev)
        t_mem = timed_us(lambda: ops.memory_scores(featn, zd, ps, scores, cnt, R, C1))
        ops.zs_classify(feat, zd, prob, False, None, cnt, R, C1, prop_scores=ps, final_inv_stages=1.0, wide=True)
        det = ops.DetectionSelector(R, C1, 100, dev, groups=True)
        t_det = timed_us(lambda: det(boxes, prob, cnt, 640.0, 640.0, 0.02, 0.5))
        mem = ops.DetectionSelector(R, C1, 100, dev, unique=True)
        t_msel = timed_us(lambda: mem(boxes, scores, cnt, 640.0, 640.0, 0.3, 0.5))
        lines.append(f"{C:7d}  {fps:8.1f}  {t_cls:19.1f}  {t_mem:16.1f}  {t_det:23.1f}  {t_msel:22.1f}")
        print(lines[-1], flush=True)
    text = "\n".join(lines) + "\n"
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text)
    print(text)


if __name__ == "__main__":
    main()
