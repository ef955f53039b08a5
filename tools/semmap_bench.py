#!/usr/bin/env python
"""Event-timed `eod_semmap_labels`, plain (one wave per cell, class by class) against EOD_SEMMAP_SCORES (the matrix-core GEMM with
the online softmax / argmax), in one process: per shape both calls are warmed up, then timed alternately, one pair of device events
per call, and the medians reported.  A call is everything the entry point enqueues: the 8-byte min/max reset, the cell or GEMM
kernel and the threshold kernel.  Shapes: 40 000 and 262 144 cells at 21 (the mp3d matrix), 81 and 1204 columns (slices of the
LVIS fixture).  The GEMM's rate is 2 x cells x 512 x (columns - 1) over the flagged call's median, against the fp32 matrix-core
peak of 157.3 TFLOP/s; the agreement of the two calls' labels on the timed inputs is printed beside it.

    python tools/semmap_bench.py [--launches 20] [--out profiles/semmap_query.txt]
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from embodied_object_detection_amd import _lib, ops, setup_cfg          # noqa: E402
from embodied_object_detection_amd.modeling.utils import load_classifier  # noqa: E402

PEAK_TFLOPS = 157.3
LVIS = os.path.join(ROOT, "tests", "golden", "lvis_v1_clip.npy")


def class_matrix(C1: int) -> torch.Tensor:
    if C1 == 21:
        return load_classifier(str(setup_cfg(None, []).MODEL.ROI_BOX_HEAD.ZEROSHOT_WEIGHT_PATH), 20)
    rows = torch.tensor(np.load(LVIS), dtype=torch.float32)
    return load_classifier(rows[:C1 - 1].t().contiguous(), C1 - 1)


def memory(n: int, zs: torch.Tensor, dev):
    """Cells as a run leaves them: two thirds sums of observations of a class (a text column + noise, x 50, x a count), a third never
    written."""
    g = torch.Generator(device=dev).manual_seed(n)
    cols = torch.randint(0, zs.shape[1] - 1, (n,), generator=g, device=dev)
    count = torch.randint(1, 41, (n, 1), generator=g, device=dev).float()
    mem = zs.t()[cols]
    mem = (mem + torch.randn((n, 512), generator=g, device=dev) / 512 ** 0.5) * 50.0 * count
    mem[torch.arange(n, device=dev) % 3 == 2] = 0.0
    obs = torch.where(mem[:, 0] != 0, count[:, 0], torch.zeros_like(count[:, 0]))
    return mem.contiguous(), obs.contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "semmap_query.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("semmap_bench: no GPU visible; nothing is measured without one")
    launches = max(20, args.launches)
    dev = torch.device("cuda:0")
    _lib.load()
    lines = [f"eod_semmap_labels, plain vs EOD_SEMMAP_SCORES: median of {launches} event-timed calls each, alternating, after warm-up",
             f"device: {torch.cuda.get_device_name(0)}",
             "GEMM rate = 2 x cells x 512 x (columns - 1) / flagged call time; share of the fp32 matrix-core peak of 157.3 TFLOP/s",
             "",
             f"{'cells':>8} {'columns':>8} {'plain ms':>10} {'flagged ms':>11} {'plain/flagged':>14} {'TFLOP/s':>9} {'of peak':>8} "
             f"{'labels equal':>13} {'-1 sets equal':>14}"]
    print("\n".join(lines), flush=True)
    for C1 in (21, 81, 1204):
        zs = class_matrix(C1).to(dev)
        for n in (40000, 262144):
            mem, obs = memory(n, zs, dev)
            calls = {"plain": lambda: ops.semmap_labels(mem, obs, zs, 0.4), "flagged": lambda: ops.semmap_query(mem, obs, zs, 0.4)[0]}
            out = {k: f() for k, f in calls.items()}                     # warm-up of this shape, and the outputs to compare
            for f in calls.values():
                f()
            torch.cuda.synchronize()
            times = {k: [] for k in calls}
            for _ in range(launches):
                for k, f in calls.items():
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record()
                    f()
                    b.record()
                    b.synchronize()
                    times[k].append(a.elapsed_time(b))
            tp, tq = float(np.median(times["plain"])), float(np.median(times["flagged"]))
            tf = 2.0 * n * 512 * (C1 - 1) / (tq * 1e-3) / 1e12
            seen = out["plain"] >= 0
            equal = (out["plain"][seen] == out["flagged"][seen]).float().mean().item() if bool(seen.any()) else float("nan")
            same_set = bool(torch.equal(out["plain"] < 0, out["flagged"] < 0))
            line = (f"{n:8d} {C1:8d} {tp:10.3f} {tq:11.3f} {tp / tq:14.2f} {tf:9.2f} {100 * tf / PEAK_TFLOPS:7.1f}% "
                    f"{100 * equal:12.4f}% {str(same_set):>14}")
            print(line, flush=True)
            lines.append(line)
            del mem, obs
    from embodied_object_detection_amd.build import resource_usage
    for name, u in sorted(resource_usage().items()):
        if "semmap_query_kernel" in name:
            lines += ["", f"semmap_query_kernel as built: {u.get('vgprs')} VGPRs, {u.get('lds')} bytes of LDS per workgroup of 512 threads, "
                          f"{u.get('occupancy')} waves per SIMD, {u.get('scratch')} bytes of scratch"]
            print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
