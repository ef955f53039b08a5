#!/usr/bin/env python
"""Event-timed `map_frontier` against what a user composes in torch without it, in one process: maps of 200 x 200 (40 000 cells) and
512 x 512 (262 144 cells) with rooms (walls of labelled cells with doors), in three states of exploration: a tenth, half and nearly
all (98 %) of the free cells covered, outward from the robot's cell with a ragged edge.  Everything is warmed up, then timed
alternately, one pair of device events per call, 20 calls each; medians with [min, max].

  frontier    `ops.map_frontier(labels, last_seen, cols, from_cell=robot, min_cells=2, topk=16, rank_by="behind")` with a workspace
              of the caller's: the eleven launches
  cover       `ops.map_cover` of one 640 x 640 frame of pixels into the record (one launch)
  composed    on the device, exact: the kinds by comparisons, the frontier cells by four shifted masks, and both label planes by the
              iterated minimum over the neighbours (8 for the frontier cells, 4 for the UNKNOWN ones) to a fixed point, which is
              looked for every 8 rounds.  It gives `frontier_labels` and `unknown_labels` alone, without the areas, the ranking and
              the per-frontier values.  Checked equal to the op's before the timing: the tool stops, and writes nothing, if it is
              not, or if two calls of the op differ in a bit.  Where its 20 calls do not fit `COMPOSED_BUDGET_S` fewer are timed and
              the line says how many

    python tools/frontier_bench.py [--launches 20] [--out profiles/frontier_bench.txt] [--op-only]

`--op-only` times the op alone (for a kernel trace: the composed form's launches would drown the op's).
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from embodied_object_detection_amd import _lib, ops          # noqa: E402

GRIDS = ((200, 200), (512, 512))
STATES = (("a tenth", 0.1), ("half", 0.5), ("nearly all", 0.98))
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


def rooms(rows, cols, seed):
    """Labels of a floor plan: walls every 40 or so cells, each with a door, and a few pieces of furniture."""
    rng = np.random.default_rng(seed)
    lab = np.full((rows, cols), -1, np.int32)
    for r in range(40, rows - 8, 40):
        lab[r, :] = 1
        for c0 in range(0, cols, 40):
            d = c0 + int(rng.integers(4, 34))
            lab[r, d:d + 3] = -1
    for c in range(40, cols - 8, 40):
        lab[:, c] = 1
        for r0 in range(0, rows, 40):
            d = r0 + int(rng.integers(4, 34))
            lab[d:d + 3, c] = -1
    for k in range(rows * cols // 2000):
        r, c = int(rng.integers(0, rows - 4)), int(rng.integers(0, cols - 4))
        lab[r:r + 3, c:c + 4] = 2 + k % 14
    return lab


def explored(lab, fraction, seed):
    """last_seen: the `fraction` of the free cells nearest to the robot's cell (with noise on the distance: a ragged edge) hold 0."""
    rows, cols = lab.shape
    rng = np.random.default_rng(seed)
    r, c = np.mgrid[0:rows, 0:cols]
    robot = (rows // 2 + 7, cols // 2 + 5)
    d = np.hypot(r - robot[0], c - robot[1]) * (1.0 + 0.15 * rng.random((rows, cols)))
    free = lab < 0
    cut = np.quantile(d[free], fraction)
    seen = np.where(d <= cut, 0, -1).astype(np.int32)
    return seen, robot[0] * cols + robot[1]


def components(mask, rows, cols, conn8):
    """Labels (the lowest cell) by the iterated minimum over the neighbours, to a fixed point."""
    big = rows * cols
    idx = torch.arange(big, dtype=torch.int32, device=mask.device).view(rows, cols)
    lab = torch.where(mask, idx, big)
    pad = torch.nn.functional.pad
    shifts = [(-1, 0), (1, 0), (0, -1), (0, 1)] + ([(-1, -1), (-1, 1), (1, -1), (1, 1)] if conn8 else [])
    while True:
        for _ in range(8):
            p = pad(lab, (1, 1, 1, 1), value=big)
            new = lab
            for dr, dc in shifts:
                new = torch.minimum(new, p[1 + dr:1 + dr + rows, 1 + dc:1 + dc + cols])
            prev, lab = lab, torch.where(mask, new, big)
        if torch.equal(prev, lab):
            break
    return torch.where(mask, lab, -1).view(-1)


def composed(labels, last_seen, rows, cols, since=0):
    lab, seen = labels.view(rows, cols), last_seen.view(rows, cols)
    blocked = lab >= 0
    unknown = ~blocked & (seen < since)
    p = torch.nn.functional.pad(unknown, (1, 1, 1, 1), value=False)
    near = p[:-2, 1:-1] | p[2:, 1:-1] | p[1:-1, :-2] | p[1:-1, 2:]
    fcell = ~blocked & (seen >= since) & near
    return components(fcell, rows, cols, True), components(unknown, rows, cols, False)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "frontier_bench.txt"))
    ap.add_argument("--op-only", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("frontier_bench: no GPU visible; nothing is measured without one")
    launches = max(20, args.launches)
    dev = torch.device("cuda:0")
    _lib.load()
    lines = [f"map_frontier vs the kinds, shifted masks and iterated neighbour minima in torch: {launches} event-timed calls each, "
             "alternating, after warm-up", f"device: {torch.cuda.get_device_name(0)}; ms as median [min, max]", ""]
    print("\n".join(lines), flush=True)
    for rows, cols in GRIDS:
        N = rows * cols
        lab = rooms(rows, cols, N)
        labels = torch.from_numpy(lab.reshape(-1)).to(dev)
        ws = torch.empty((ops.map_frontier_workspace(N, cols),), dtype=torch.int32, device=dev)
        proj = torch.randint(-1, N, (640, 640), dtype=torch.int32, device=dev)
        record = torch.full((N,), -1, dtype=torch.int32, device=dev)
        t = timed({"cover": (lambda: ops.map_cover(proj, record, 1), launches)}, launches)["cover"]
        block = [f"{rows} x {cols} = {N} cells: cover of 640 x 640 pixels {float(np.median(t)):9.3f} [{t[0]:.3f}, {t[-1]:.3f}] ms", ""]
        print("\n".join(block), flush=True)
        lines += block
        for sname, fraction in STATES:
            seen_np, robot = explored(lab, fraction, N + 1)
            seen = torch.from_numpy(seen_np.reshape(-1)).to(dev)
            op = lambda: ops.map_frontier(labels, seen, cols, from_cell=robot, min_cells=2, topk=16, rank_by="behind", workspace=ws)
            out = {k: v.clone() for k, v in op().items()}
            again = op()
            op_same = all(torch.equal(out[k], again[k]) for k in out)
            head = f"{rows} x {cols} = {N} cells, {sname} of the free cells known"
            if not op_same:
                raise SystemExit(f"frontier_bench: {head}: two calls of the op differ; nothing is written")
            if args.op_only:
                t = timed({"frontier": (op, launches)}, launches)["frontier"]
                block = [f"{head}: frontier {float(np.median(t)):9.3f} [{t[0]:.3f}, {t[-1]:.3f}] ms"]
                print("\n".join(block), flush=True)
                lines += block
                continue
            t0 = time.time()
            fl, ul = composed(labels, seen, rows, cols)
            torch.cuda.synchronize()
            first = time.time() - t0
            same = bool(torch.equal(fl, out["frontier_labels"])) and bool(torch.equal(ul, out["unknown_labels"]))
            if not same:
                raise SystemExit(f"frontier_bench: {head}: the composed labels are not the op's; nothing is timed or written")
            n_composed = launches if first * (launches + 3) <= COMPOSED_BUDGET_S else max(1, int(COMPOSED_BUDGET_S / first) - 1)
            t = timed({"frontier": (op, launches),
                       "composed": (lambda: composed(labels, seen, rows, cols), min(launches, n_composed))}, launches)
            med = {k: float(np.median(v)) for k, v in t.items()}
            block = [f"{head}: counts {out['counts'].tolist()} (BLOCKED, OPEN, UNKNOWN, frontier cells, unknown regions), "
                     f"{int(out['count'])} frontiers of 2 cells or more; area {out['area'][:4].tolist()}, behind_area "
                     f"{out['behind_area'][:4].tolist()}, reach_cost {out['reach_cost'][:4].tolist()}, status {out['status'].tolist()}"]
            for k, v in t.items():
                block.append(f"  {k:10s} {med[k]:9.3f} [{v[0]:.3f}, {v[-1]:.3f}] ms  ({len(v)} calls)")
            block.append(f"  composed / frontier = {med['composed'] / med['frontier']:.1f}; the composed labels are the op's: {same}; two "
                         f"calls of the op agree bitwise: {op_same}")
            block.append("")
            print("\n".join(block), flush=True)
            lines += block
    from embodied_object_detection_amd.build import resource_usage
    for name, u in sorted(resource_usage().items()):
        if "frontier_" in name or "regions_compress" in name or "regions_flatten" in name or "regions_list" in name:
            lines.append(f"{name}: {u.get('vgprs')} VGPRs, {u.get('lds')} bytes of static LDS, {u.get('occupancy')} waves per SIMD, "
                         f"{u.get('scratch')} bytes of scratch")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
