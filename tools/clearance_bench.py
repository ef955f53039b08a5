#!/usr/bin/env python
"""Event-timed `map_clearance` against what a user composes in torch without it, in one process: maps of 200 x 200 (40 000 cells)
and 512 x 512 (262 144 cells); at each size the inventory's label map of the synthetic model after three 640 x 640 frames with its
16 largest objects (level 2 ** -11: every labelled cell is in an object), the same map with its largest object passable, and a map
whose only blocked cell is in a corner.  Everything is warmed up, then timed alternately, one pair of device events per call, 20
calls each; medians with [min, max].

  clearance   `ops.map_clearance(labels, objects, cols, radius2=4, keep_cell=K, passable=P)` with a workspace of the caller's:
              the init, column, row, finish and widest launches
  composed    on the device, exact: for chunks of cells the minimum over all blocked cells of (d2 << 32) | cell in int64, which
              gives `d2` and `nearest` alone, without owner, inflated, territories or keys.  Checked equal to the op's before the
              timing: the tool stops, and writes nothing, if it is not, or if two calls of the op differ in a bit.  Its 20 calls
              fit `COMPOSED_BUDGET_S` on every map here (about 1.5 s a call where every cell of 512 x 512 is blocked); on a
              machine where they do not, fewer are timed and the line says how many

Then the op alone on the worst cases of its two scans: a 1 x 32767 and a 32767 x 1 map whose only blocked cell is the last one.

    python tools/clearance_bench.py [--launches 20] [--out profiles/clearance_bench.txt]
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from embodied_object_detection_amd import _lib, build_model, ops, setup_cfg          # noqa: E402
from embodied_object_detection_amd.checkpoint import synthetic_state_dict            # noqa: E402
from embodied_object_detection_amd.data.synthetic import SyntheticSequence           # noqa: E402

GRIDS = ((200, 200, 0.2), (512, 512, 0.08))
TOPK = 16
INT_MAX = 2 ** 31 - 1
PAIRS = 1 << 25                                                      # (cell, blocked cell) pairs of one chunk: 256 MB of int64
COMPOSED_BUDGET_S = 90.0                                             # for the 20 timed calls and the 3 of the warm-up of one map


def timed(calls, launches):
    """{name: sorted event times in ms} of `calls` {name: (callable, calls to time)}, warmed up, then alternating."""
    for f, n in calls.values():
        for _ in range(3 if n >= launches else 1):
            f()
    torch.cuda.synchronize()
    times = {k: [] for k in calls}
    for i in range(launches):
        for k, (f, n) in calls.items():
            if i >= n:
                continue
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            f()
            b.record()
            b.synchronize()
            times[k].append(a.elapsed_time(b))
    return {k: sorted(v) for k, v in times.items()}


def composed(labels, rows, cols, passable=()):
    """What a user writes today: d2 and nearest int32 [N], exact."""
    N = rows * cols
    blocked = labels >= 0
    for p in passable:
        blocked &= labels != p
    bj = torch.nonzero(blocked).view(-1)
    if bj.numel() == 0:
        return (torch.full((N,), INT_MAX, dtype=torch.int32, device=labels.device),
                torch.full((N,), -1, dtype=torch.int32, device=labels.device))
    br, bc = bj // cols, bj % cols
    cell = torch.arange(N, device=labels.device)
    r, c = cell // cols, cell % cols
    best = torch.empty((N,), dtype=torch.int64, device=labels.device)
    step = max(1, PAIRS // int(bj.numel()))
    for a in range(0, N, step):
        dr, dc = r[a:a + step, None] - br[None, :], c[a:a + step, None] - bc[None, :]
        best[a:a + step] = (((dr * dr + dc * dc) << 32) | bj[None, :]).amin(dim=1)
    return (best >> 32).to(torch.int32), (best & 0xFFFFFFFF).to(torch.int32)


def corner(rows, cols, dev, last=False):
    g = torch.full((rows * cols,), -1, dtype=torch.int32, device=dev)
    g[rows * cols - 1 if last else 0] = 10
    return g


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "clearance_bench.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("clearance_bench: no GPU visible; nothing is measured without one")
    launches = max(20, args.launches)
    dev = torch.device("cuda:0")
    _lib.load()
    sd = synthetic_state_dict(0)
    lines = [f"map_clearance vs an exact chunked minimum over the blocked cells in torch: {launches} event-timed calls each, alternating, "
             "after warm-up",
             f"device: {torch.cuda.get_device_name(0)}; row pass: {ops.CLEARANCE_TILE_ROWS} rows x {ops.CLEARANCE_CHUNK_COLS} columns a "
             f"workgroup, halo {ops.CLEARANCE_HALO_COLS}; ms as median [min, max]", ""]
    print("\n".join(lines), flush=True)
    ten = torch.tensor([10], dtype=torch.int32, device=dev)
    for map_w, map_h, cell in GRIDS:
        N = map_w * map_h
        cfg = setup_cfg(None, ["MODEL.MEMORY_TYPE", "implicit_memory", "MODEL.MAP_FEAT_FUSION", "sum", "MODEL.MAP_FEATURE_WEIGHT", 5,
                               "MODEL.MEMORY_CLS_SCORE_THRESH", 0.3, "MODEL.DEVICE", "cuda:0"])
        model = build_model(cfg, sd)
        seq = SyntheticSequence(7, H=640, W=640, n_frames=3, map_w=map_w, map_h=map_h, cell=cell)
        for i in range(3):
            model([[seq.frame(i)]])
        inv = model.inventory(thresh=0.0, map_shape=(map_w, map_h), level=2.0 ** -11, topk=TOPK)
        inv_labels, inv_objects = inv["object_labels"].clone(), inv["object"].clone()
        big = inv_objects[:1].clone()                                 # the largest object: the synthetic scene's background class
        in_big = torch.nonzero(inv_labels == big[0]).view(-1)
        keep = int(in_big[in_big.numel() // 2]) if in_big.numel() else -1
        ws = torch.empty((ops.map_clearance_workspace(N, map_h),), dtype=torch.int32, device=dev)
        for name, labels, objects, keep_cell, passable in (("inventory", inv_labels, inv_objects, -1, None),
                                                           ("inventory, its largest object passable", inv_labels, inv_objects, keep, big),
                                                           ("one blocked cell, in the corner", corner(map_w, map_h, dev), ten, N - 1, None)):
            host_pass = [] if passable is None else passable.tolist()
            op = lambda: ops.map_clearance(labels, objects, map_h, radius2=4, keep_cell=keep_cell, passable=passable, workspace=ws)
            out = {k: v.clone() for k, v in op().items()}
            again = op()
            op_same = all(torch.equal(out[k], again[k]) for k in out)
            t0 = time.time()
            cd2, cnear = composed(labels, map_w, map_h, host_pass)
            torch.cuda.synchronize()
            first = time.time() - t0
            same = bool(torch.equal(cd2, out["d2"])) and bool(torch.equal(cnear, out["nearest"]))
            if not same or not op_same:
                raise SystemExit(f"clearance_bench: {map_w} x {map_h}, {name}: composed d2 and nearest are the op's: {same}; two calls "
                                 f"of the op agree bitwise: {op_same}; nothing is timed or written")
            n_composed = launches if first * (launches + 3) <= COMPOSED_BUDGET_S else max(2, int(COMPOSED_BUDGET_S / first))
            t = timed({"clearance": (op, launches), "composed": (lambda: composed(labels, map_w, map_h, host_pass), min(launches, n_composed))},
                      launches)
            med = {k: float(np.median(v)) for k, v in t.items()}
            counts = out["counts"].tolist()
            d2 = out["d2"]
            block = [f"{map_w} x {map_h} = {N} cells, {name}: {counts[0]} blocked cells, {counts[1]} free, {counts[2]} grown at radius2 4; "
                     f"{int((objects >= 0).sum())} objects asked, territory {out['territory'].tolist()}; largest d2 "
                     f"{int(d2[d2 < INT_MAX].max()) if bool((d2 < INT_MAX).any()) else 'none'}, status {out['status'].tolist()}"]
            for k, v in t.items():
                block.append(f"  {k:10s} {med[k]:9.3f} [{v[0]:.3f}, {v[-1]:.3f}] ms  ({len(v)} calls)")
            block.append(f"  composed / clearance = {med['composed'] / med['clearance']:.1f}")
            block.append(f"  composed d2 and nearest are the op's: {same}; two calls of the op agree bitwise: {op_same}")
            block.append("")
            print("\n".join(block), flush=True)
            lines += block
        del model
        torch.cuda.empty_cache()
    for rows, cols in ((1, 32767), (32767, 1)):
        labels = corner(rows, cols, dev, last=True)
        ws = torch.empty((ops.map_clearance_workspace(rows * cols, cols),), dtype=torch.int32, device=dev)
        op = lambda: ops.map_clearance(labels, ten, cols, radius2=4, workspace=ws)
        out = op()
        want = (torch.arange(rows * cols - 1, -1, -1, device=dev, dtype=torch.int64) ** 2).to(torch.int32)
        ok = bool(torch.equal(out["d2"], want)) and bool((out["nearest"] == rows * cols - 1).all())
        if not ok:
            raise SystemExit(f"clearance_bench: {rows} x {cols}: d2 is not the squared distance along the line; nothing is written")
        t = timed({"clearance": (op, launches)}, launches)["clearance"]
        block = [f"{rows} x {cols}, the only blocked cell is the last: clearance {float(np.median(t)):9.3f} [{t[0]:.3f}, {t[-1]:.3f}] ms  "
                 f"({len(t)} calls); d2 is the squared distance along the line: {ok}", ""]
        print("\n".join(block), flush=True)
        lines += block
    from embodied_object_detection_amd.build import resource_usage
    for name, u in sorted(resource_usage().items()):
        if "clearance_" in name:
            lines.append(f"{name}: {u.get('vgprs')} VGPRs, {u.get('lds')} bytes of LDS, {u.get('occupancy')} waves per SIMD, "
                         f"{u.get('scratch')} bytes of scratch")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
