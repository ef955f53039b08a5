"""Vocabulary width against speed: frames/s through `model([episode])` at 640x640 (200x200 grid) for 20, 80, 365 and 1203 classes
(same weights, class matrix sliced from tests/golden/lvis_v1_clip.npy), and event-timed microseconds of one classifier stage, of
`memory_scores` and of both selections, launch alone, at each width.

    python tools/vocab_bench.py [--out profiles/vocab_bench.txt] [--frames 40]

`train`: the two logits launches of the training step alone (`eod_zs_logits`, `eod_zs_logits_backward`, B = 512) at 25 to 2048
columns, the one-wave-per-row kernels against the matrix-core ones, and the federated loss's class choice + loss launches.  The
kernels are chosen by EOD_ZS_TRAIN_WIDE, read once when the library loads, so each side is timed in a child process of its own.

    python tools/vocab_bench.py train [--out profiles/vocab_train_bench.txt]
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


TRAIN_WIDTHS = (25, 41, 366, 1204, 2048)


def train_child() -> None:
    """One JSON line: microseconds per launch at every width, with the kernels this process's environment selects."""
    import json
    from embodied_object_detection_amd import ops
    dev = torch.device("cuda:0")
    B = 512
    g = torch.Generator().manual_seed(2)
    feat = torch.randn((B, 512), generator=g).to(dev)
    out = {}
    for C1 in TRAIN_WIDTHS:
        zs = F.normalize(torch.randn((512, C1), generator=g), p=2, dim=0).contiguous().to(dev)
        dl = (torch.randn((B, C1), generator=g) / C1).to(dev)
        featn = torch.empty((B, 512), device=dev)
        fw = timed_us(lambda: ops.zs_logits(feat, zs, 50.0, featn_out=featn))
        alloc = timed_us(lambda: torch.zeros((B, C1), device=dev))                 # the wrapper's own zero-filled output
        bw = timed_us(lambda: ops.zs_logits_backward(feat, zs, dl, 50.0))
        out[C1] = [round(fw - alloc, 1), round(bw, 1)]
    for C in (20, 365, 1203, 2047):
        gt = torch.cat([torch.randint(0, C, (128,), generator=g), torch.full((384,), C)]).int().to(dev)
        fed = ops.FedLossParams(C, 50, torch.rand((C,), generator=g) + 0.1, None, dev)
        fed.draw_q()
        scores, box = torch.randn((B, C + 1), generator=g).to(dev), torch.tensor([0.0, 0.0, 8.0, 8.0], device=dev).repeat(B, 1)
        deltas = torch.zeros((B, 4), device=dev)
        cw = torch.ones((C,), device=dev)
        plain = timed_us(lambda: ops.fast_rcnn_loss(scores, deltas, box, box, gt, C, (10.0, 10.0, 5.0, 5.0), cw))
        with_choice = timed_us(lambda: ops.fast_rcnn_loss(scores, deltas, box, box, gt, C, (10.0, 10.0, 5.0, 5.0), fed=fed))
        out[f"fed{C}"] = [round(plain, 1), round(with_choice, 1)]
    print("TRAIN_BENCH " + json.dumps(out), flush=True)


def train_parent(out_path) -> None:
    import json
    import subprocess
    res = {}
    for wide in ("0", "1"):
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "train", "--child"], env=dict(os.environ, EOD_ZS_TRAIN_WIDE=wide),
                           capture_output=True, text=True, timeout=600)
        if r.returncode != 0:
            raise SystemExit(f"child with EOD_ZS_TRAIN_WIDE={wide} failed ({r.returncode}):\n{r.stdout[-2000:]}{r.stderr[-2000:]}")
        res[wide] = json.loads([l for l in r.stdout.splitlines() if l.startswith("TRAIN_BENCH ")][-1][len("TRAIN_BENCH "):])
    lines = ["B = 512, event-timed median of 50 single launches, microseconds (forward without the wrapper's zero fill)",
             "columns  forward one-wave-per-row  forward matrix cores  backward one-wave-per-row  backward matrix cores (2 launches)"]
    for C1 in TRAIN_WIDTHS:
        o, n = res["0"][str(C1)], res["1"][str(C1)]
        lines.append(f"{C1:7d}  {o[0]:24.1f}  {n[0]:20.1f}  {o[1]:25.1f}  {n[1]:21.1f}")
    lines.append("classes  loss launches with a given weight  with the federated class choice in front (3 launches)")
    for C in (20, 365, 1203, 2047):
        v = res["1"][f"fed{C}"]
        lines.append(f"{C:7d}  {v[0]:35.1f}  {v[1]:40.1f}")
    text = "\n".join(lines) + "\n"
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as fh:
            fh.write(text)
    print(text)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", nargs="?", default="frames", choices=["frames", "train"])
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--out", default=None)
    ap.add_argument("--frames", type=int, default=40)
    args = ap.parse_args()
    if args.mode == "train":
        return train_child() if args.child else train_parent(args.out)
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
