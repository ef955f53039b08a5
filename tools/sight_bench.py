#!/usr/bin/env python
"""Event-timed `map_sight` against what a user composes in torch without it, in one process: maps of 200 x 200 (40 000 cells) and
512 x 512 (262 144 cells); at each size the inventory's label map of the synthetic model after three 640 x 640 frames with its
largest object (the background of the synthetic scene) passable, a sparse random map (3 % of the cells opaque) and an empty map,
the worst case: every line runs its full length.  S = 1, 8 and 64 sources spread over the map, with an unbounded range and with
`sight_range2(4.0)` of a front end of the map's cell size.  Everything is warmed up, then timed alternately, one pair of device
events per call, 20 calls each; medians with [min, max].

  sight       `ops.map_sight(labels, objects, cols, from_cells, range2=R, passable=P)` with a workspace of the caller's: the init,
              walk and finish launches
  composed    on the device, exact: per source the same walk as masked tensor steps over the targets within the range's window,
              one step of all lines per iteration, with the closed-form rounding in int64.  It gives `seen_mask` alone, without the
              per-object sums and keys.  Checked equal to the op's before the timing: the tool stops, and writes nothing, if it is
              not, or if two calls of the op differ in a bit.  Where its 20 calls do not fit `COMPOSED_BUDGET_S` fewer are timed and
              the line says how many

    python tools/sight_bench.py [--launches 20] [--out profiles/sight_bench.txt] [--op-only]

`--op-only` times the op alone (for a kernel trace: the composed form's launches would drown the op's).
"""
import argparse
import math
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from embodied_object_detection_amd import _lib, build_model, ops, setup_cfg          # noqa: E402
from embodied_object_detection_amd.checkpoint import synthetic_state_dict            # noqa: E402
from embodied_object_detection_amd.data.robot import RobotFrontEnd                   # noqa: E402
from embodied_object_detection_amd.data.synthetic import SyntheticSequence           # noqa: E402

GRIDS = ((200, 200, 0.2), (512, 512, 0.08))
SOURCES = (1, 8, 64)
TOPK = 16
INT_MAX = 2 ** 31 - 1
COMPOSED_BUDGET_S = 30.0                                             # for the timed calls and the warm-up of one line of the table


def timed(calls, launches):
    """{name: sorted event times in ms} of `calls` {name: (callable, calls to time)}, warmed up, then alternating."""
    for f, n in calls.values():
        for _ in range(3 if n >= launches else 0):              # a form timed fewer times has run once already, for the check
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


def composed(labels, rows, cols, sources, range2, passable=()):
    """What a user writes today: seen_mask int64 [N], exact.  One masked step of every line of a source per iteration."""
    dev = labels.device
    opaque = labels >= 0
    for p in passable:
        opaque &= labels != p
    mask = torch.zeros((rows * cols,), dtype=torch.int64, device=dev)
    reach = min(math.isqrt(range2), max(rows, cols))
    for s, f in enumerate(sources):
        if f < 0:
            continue
        r0, c0 = divmod(int(f), cols)
        O = opaque.clone()
        O[f] = False
        ra, rb, ca, cb = max(0, r0 - reach), min(rows, r0 + reach + 1), max(0, c0 - reach), min(cols, c0 + reach + 1)
        R, C = torch.meshgrid(torch.arange(ra, rb, device=dev), torch.arange(ca, cb, device=dev), indexing="ij")
        R, C = R.reshape(-1), C.reshape(-1)
        dr, dc = R - r0, C - c0
        n = torch.maximum(dr.abs(), dc.abs())
        alive = dr * dr + dc * dc <= range2
        nn = n.clamp(min=1)
        pr, pc = torch.full_like(R, r0), torch.full_like(C, c0)
        for i in range(1, max(rb - 1 - r0, r0 - ra, cb - 1 - c0, c0 - ca) + 1):
            r = r0 + torch.sign(dr) * ((2 * i * dr.abs() + nn) // (2 * nn))
            c = c0 + torch.sign(dc) * ((2 * i * dc.abs() + nn) // (2 * nn))
            on = i <= n                                              # lines that have not yet arrived
            r, c = torch.where(on, r, pr), torch.where(on, c, pc)
            corner = (r != pr) & (c != pc) & O[pr * cols + c] & O[r * cols + pc]
            alive &= ~(on & (corner | ((i < n) & O[r * cols + c])))
            pr, pc = r, c
        mask[(R * cols + C)[alive]] |= (1 << s) if s < 63 else -(1 << 63)
    return mask


def spread(S, rows, cols):
    """S cells spread over the map: the centre first."""
    cells = [(rows // 2) * cols + cols // 2]
    for k in range(1, S):
        cells.append(((k * 37) % rows) * cols + (k * 101) % cols)
    return cells


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sight_bench.txt"))
    ap.add_argument("--op-only", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("sight_bench: no GPU visible; nothing is measured without one")
    launches = max(20, args.launches)
    dev = torch.device("cuda:0")
    _lib.load()
    sd = synthetic_state_dict(0)
    lines = [f"map_sight vs the same walk as masked tensor steps in torch: {launches} event-timed calls each, alternating, after warm-up",
             f"device: {torch.cuda.get_device_name(0)}; the bit plane is staged in LDS up to {ops.SIGHT_LDS_CELLS} cells; a workgroup "
             f"owns {ops.SIGHT_WORKGROUP} cells; ms as median [min, max]", ""]
    print("\n".join(lines), flush=True)
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
        front = RobotFrontEnd.__new__(RobotFrontEnd)
        front.res = cell
        near = front.sight_range2(4.0)
        gen = torch.Generator().manual_seed(N)
        sparse = torch.where(torch.rand((N,), generator=gen) < 0.03, torch.randint(0, TOPK, (N,), generator=gen), -1).to(torch.int32).to(dev)
        empty = torch.full((N,), -1, dtype=torch.int32, device=dev)
        some = torch.arange(TOPK, dtype=torch.int32, device=dev)
        ws = torch.empty((ops.map_sight_workspace(N, map_h),), dtype=torch.int32, device=dev)
        for name, labels, objects, passable in (("inventory, its largest object passable", inv_labels, inv_objects, big),
                                                ("sparse, 3 % of the cells opaque", sparse, some, None),
                                                ("empty", empty, some, None)):
            host_pass = [] if passable is None else passable.tolist()
            for S in SOURCES:
                src = spread(S, map_w, map_h)
                for rname, range2 in (("unbounded", INT_MAX), (f"4 m = range2 {near}", near)):
                    op = lambda: ops.map_sight(labels, objects, map_h, src, range2=range2, passable=passable, workspace=ws)
                    out = {k: v.clone() for k, v in op().items()}
                    again = op()
                    op_same = all(torch.equal(out[k], again[k]) for k in out)
                    head = f"{map_w} x {map_h} = {N} cells, {name}, S = {S}, {rname}"
                    if args.op_only:
                        if not op_same:
                            raise SystemExit(f"sight_bench: {head}: two calls of the op differ; nothing is written")
                        t = timed({"sight": (op, launches)}, launches)["sight"]
                        block = [f"{head}: sight {float(np.median(t)):9.3f} [{t[0]:.3f}, {t[-1]:.3f}] ms"]
                        print("\n".join(block), flush=True)
                        lines += block
                        continue
                    t0 = time.time()
                    cm = composed(labels, map_w, map_h, src, range2, host_pass)
                    torch.cuda.synchronize()
                    first = time.time() - t0
                    same = bool(torch.equal(cm, out["seen_mask"]))
                    if not same or not op_same:
                        raise SystemExit(f"sight_bench: {head}: composed seen_mask is the op's: {same}; two calls of the op agree "
                                         f"bitwise: {op_same}; nothing is timed or written")
                    n_composed = launches if first * (launches + 3) <= COMPOSED_BUDGET_S else max(1, int(COMPOSED_BUDGET_S / first) - 1)
                    t = timed({"sight": (op, launches),
                               "composed": (lambda: composed(labels, map_w, map_h, src, range2, host_pass), min(launches, n_composed))}, launches)
                    med = {k: float(np.median(v)) for k, v in t.items()}
                    counts = out["counts"].tolist()
                    block = [f"{head}: {counts[0]} opaque cells, {counts[1]} transparent, {counts[2]} seen by some source; source 0 sees "
                             f"{out['source_counts'][0].tolist()}; best_seen {out['best_seen'].tolist()}, status {out['status'].tolist()}"]
                    for k, v in t.items():
                        block.append(f"  {k:10s} {med[k]:9.3f} [{v[0]:.3f}, {v[-1]:.3f}] ms  ({len(v)} calls)")
                    block.append(f"  composed / sight = {med['composed'] / med['sight']:.1f}; composed seen_mask is the op's: {same}; two calls "
                                 f"of the op agree bitwise: {op_same}")
                    block.append("")
                    print("\n".join(block), flush=True)
                    lines += block
        del model
        torch.cuda.empty_cache()
    from embodied_object_detection_amd.build import resource_usage
    for name, u in sorted(resource_usage().items()):
        if "sight_" in name:
            lines.append(f"{name}: {u.get('vgprs')} VGPRs, {u.get('lds')} bytes of static LDS, {u.get('occupancy')} waves per SIMD, "
                         f"{u.get('scratch')} bytes of scratch")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
