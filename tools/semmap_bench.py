#!/usr/bin/env python
"""Event-timed `eod_semmap_labels`, plain (one wave per cell, class by class) against EOD_SEMMAP_SCORES (the matrix-core GEMM with
the online softmax / argmax), in one process: per shape both calls are warmed up, then timed alternately, one pair of device events
per call, and the medians reported.  A call is everything the entry point enqueues: the 8-byte min/max reset, the cell or GEMM
kernel and the threshold kernel.  Shapes: 40 000 and 262 144 cells at 21 (the mp3d matrix), 81 and 1204 columns (slices of the
LVIS fixture).  The GEMM's rate is 2 x cells x 512 x (columns - 1) over the flagged call's median, against the fp32 matrix-core
peak of 157.3 TFLOP/s; the agreement of the two calls' labels on the timed inputs is printed beside it.

    python tools/semmap_bench.py [--launches 20] [--out profiles/semmap_query.txt]

`--locate` measures the locate query instead (EOD_SEMMAP_LOCATE, then EOD_SEMMAP_PEAKS; K = 8, radius 1) at 40 000 and 262 144 cells
x 1204 columns (38 panels: the wave that takes the gathered panel has one panel less than the fullest) and x 1025 columns (32 panels,
four per wave: the gathered panel is some wave's fifth), beside the SCORES call, all calls of a shape alternating: the maps call at Q = 1, 8 and 32 (the gathered panel is 32
wide whatever Q is, so Q = 1 over SCORES is the panel and the second threshold kernel, and the growth with Q is the Q x N floats
written), the peaks call at Q = 8, and `ops.semmap_locate` whole.  `--parent-lib` names a libeod_hip.so of another build, loaded
beside this one; its SCORES call joins the alternation.

    python tools/semmap_bench.py --locate [--parent-lib other/libeod_hip.so] [--locate-out profiles/semmap_locate.txt]
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


def timed(calls, launches):
    """{name: sorted event times in ms} of `calls` {name: callable}, warmed up, then alternating."""
    for _ in range(3):
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
    return {k: sorted(v) for k, v in times.items()}


def locate(args, launches, dev):
    import ctypes as C
    lib = _lib.load()
    other = None
    if args.parent_lib:
        other = C.CDLL(os.path.abspath(args.parent_lib))
        other.eod_semmap_labels.restype, other.eod_semmap_labels.argtypes = _lib.SIGNATURES["eod_semmap_labels"]
    K, radius = 8, 1
    lines = [f"eod_semmap_labels, the locate query beside the SCORES call: {launches} event-timed calls each, alternating, after warm-up",
             f"device: {torch.cuda.get_device_name(0)}; K = {K}, radius {radius}; ms as median [min, max]",
             "maps Q: the EOD_SEMMAP_LOCATE call (GEMM with the gathered panel, prob written, threshold); peaks: the EOD_SEMMAP_PEAKS call;",
             "locate: ops.semmap_locate whole (query indices copied in, both calls)", ""]
    print("\n".join(lines), flush=True)
    for C1, n in ((1204, 40000), (1204, 262144), (1025, 40000), (1025, 262144)):
        zs = class_matrix(C1).to(dev)
        panels = (C1 + 30) // 32
        mem, obs = memory(n, zs, dev)
        cols = 200 if n == 40000 else 512
        stream = torch.cuda.current_stream().cuda_stream
        labels = torch.empty((n,), dtype=torch.int32, device=dev)
        ws = torch.empty((ops.semmap_locate_workspace(n, 32, K),), dtype=torch.float32, device=dev)
        ws[4 + 2 * n:4 + 2 * n + 32].view(torch.int32).copy_(torch.arange(32, dtype=torch.int32) * 31)
        classes = [31 * i for i in range(8)]

        def raw(l, D, c1):
            st = l.eod_semmap_labels(mem.data_ptr(), obs.data_ptr(), zs.data_ptr(), n, D, c1, 0.4, labels.data_ptr(), ws.data_ptr(), stream)
            assert st == 0, st

        def maps(Q):
            return lambda: raw(lib, 512 | _lib.SEMMAP_LOCATE | Q << _lib.SEMMAP_Q_SHIFT, C1)

        pbits = 512 | _lib.SEMMAP_PEAKS | 8 << _lib.SEMMAP_Q_SHIFT | (K - 1) << _lib.SEMMAP_K_SHIFT | radius << _lib.SEMMAP_RADIUS_SHIFT
        calls = {"SCORES": lambda: raw(lib, 512 | _lib.SEMMAP_SCORES, C1)}
        if other is not None:
            calls["SCORES, parent build"] = lambda: raw(other, 512 | _lib.SEMMAP_SCORES, C1)
        calls.update({"maps Q=1": maps(1), "maps Q=32": maps(32), "maps Q=8": maps(8), "peaks Q=8": lambda: raw(lib, pbits, cols),
                      "locate Q=8": lambda: ops.semmap_locate(mem, obs, zs, classes, 0.4, cols=cols, radius=radius, topk=K, workspace=ws)})
        t = timed(calls, launches)
        med = {k: float(np.median(v)) for k, v in t.items()}
        lines.append(f"{n} cells ({n // cols} x {cols}), {C1} columns ({panels} panels)")
        for k, v in t.items():
            lines.append(f"  {k:22s} {med[k]:8.3f} [{v[0]:.3f}, {v[-1]:.3f}]   x SCORES {med[k] / med['SCORES']:.3f}")
        lines += [f"  panel + second threshold kernel (maps Q=1 - SCORES)   {med['maps Q=1'] - med['SCORES']:+.3f} ms; one panel's share of the "
                  f"GEMM, 1/{panels}: {med['SCORES'] / panels:.3f} ms",
                  f"  writing prob (maps Q=8 - maps Q=1)                    {med['maps Q=8'] - med['maps Q=1']:+.3f} ms for {8 * n * 4 / 1e6:.1f} MB; "
                  f"Q=32 - Q=1: {med['maps Q=32'] - med['maps Q=1']:+.3f} ms",
                  f"  peaks                                                 {med['peaks Q=8']:.3f} ms", ""]
        print("\n".join(lines[-(len(t) + 5):]), flush=True)
        del mem, obs, ws
    from embodied_object_detection_amd.build import resource_usage
    for name, u in sorted(resource_usage().items()):
        if "semmap_query_kernel" in name or "semmap_peak" in name or "threshold_locate" in name:
            lines.append(f"{name}: {u.get('vgprs')} VGPRs, {u.get('lds')} bytes of LDS, {u.get('occupancy')} waves per SIMD, "
                         f"{u.get('scratch')} bytes of scratch")
    os.makedirs(os.path.dirname(os.path.abspath(args.locate_out)), exist_ok=True)
    with open(args.locate_out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "semmap_query.txt"))
    ap.add_argument("--locate", action="store_true", help="measure the locate query instead of plain vs SCORES")
    ap.add_argument("--parent-lib", default="", help="with --locate: another build's library, its SCORES call timed alongside")
    ap.add_argument("--locate-out", default=os.path.join(ROOT, "profiles", "semmap_locate.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("semmap_bench: no GPU visible; nothing is measured without one")
    launches = max(20, args.launches)
    if args.locate:
        return locate(args, launches, torch.device("cuda:0"))
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
