#!/usr/bin/env python
"""Event-timed `map_heights` and `map_obstacles` against what a user composes in torch without them, in one process.

  heights     `ops.map_heights(proj_indices, xyz, record)` of one frame, the height column of the projector's xyz read in place
              (one launch), on two inputs: `frame`, the `proj_indices` and `xyz` of `ops.unproject_grid_index` on the depth image of a
              room (a floor, a ceiling, a wall whose distance varies along the image, holes of depth 0), 640 x 640 pixels over
              200 x 200 cells of 0.2 m and 960 x 960 over 512 x 512 cells of 0.08 m; and `one cell`, every pixel of the frame in one
              cell, the worst case for the atomics
  composed    the same record in torch: the valid pixels by comparisons, the millimetres by one product and `round`, `bincount`
              for the two counters and `scatter_reduce_` with amin / amax for the two heights.  Checked equal to the op's before
              the timing
  obstacles   `ops.map_obstacles(record, cols, object_labels, objects, min_hits=4, min_cells=2, topk=16)` with a workspace of the
              caller's (nine launches), at 200 x 200 = 40 000 and 512 x 512 = 262 144 cells, on the record of rooms: walls with doors
              seen as heights, furniture as objects, a part of the map never seen
  kinds       the kinds alone composed in torch (three `where`), without the structures, the merged labels, the ranking and the
              per-object values.  Checked equal to the op's `kind`

Everything is warmed up, then timed alternately, one pair of device events per call, 20 calls each; medians with [min, max].  The
tool stops, and writes nothing, if a composed result is not the op's or if two calls of an op differ in a bit.

    python tools/obstacles_bench.py [--launches 20] [--out profiles/obstacles_bench.txt] [--op-only] [--heights-only]

`--op-only` times the ops alone (for a kernel trace: the composed forms' launches would drown the ops'); `--heights-only` leaves
`map_obstacles` out (for comparing builds of the heights kernel).
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from embodied_object_detection_amd import _lib, ops          # noqa: E402

FRAMES = ((640, 200, 0.2), (960, 512, 0.08))                        # pixels a side, cells a side, metres a cell
BAND = (100, 1500)
CAMERA_HEIGHT = 0.65


def timed(calls, launches):
    """{name: sorted event times in ms} of `calls` {name: callable}, warmed up, then alternating."""
    for f in calls.values():
        for _ in range(3):
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


def fmt(t):
    return f"{float(np.median(t)):9.3f} [{t[0]:.3f}, {t[-1]:.3f}] ms"


def room_depth(S, seed):
    """The depth image [S, S] of a camera 0.65 m above the floor of a room 2.5 m high, looking at a wall 3 to 4.5 m away."""
    rng = np.random.default_rng(seed)
    v, u = np.mgrid[0:S, 0:S]
    ys = (v + 0.5 - S / 2.0) / (S / 2.0)                             # image down: positive below the horizon
    wall = 3.0 + 1.5 * np.abs(np.sin(u / (S / 6.6)))
    with np.errstate(divide="ignore"):
        floor = np.where(ys > 0, CAMERA_HEIGHT / ys, np.inf)
        ceiling = np.where(ys < 0, (CAMERA_HEIGHT - 2.5) / ys, np.inf)
    depth = np.minimum(np.minimum(floor, ceiling), wall) * (1.0 + 0.004 * rng.standard_normal((S, S)))
    depth[rng.random((S, S)) < 0.02] = 0.0                           # holes: they land in the camera's own cell
    return depth.astype(np.float32)


def project(depth, cells, cell, dev):
    """(proj_indices [S, S], xyz [S, S, 3], the camera's own cell) of the room's depth image, the camera in the middle of the map."""
    S = depth.shape[0]
    T = np.eye(4, dtype=np.float32)
    T[1, 1], T[1, 3] = -1.0, CAMERA_HEIGHT                           # the image's down is the world's -y
    half = cells * cell / 2.0
    idx, xyz = ops.unproject_grid_index(torch.from_numpy(depth).to(dev), T, (S / 2.0, S / 2.0, S / 2.0, S / 2.0), (0.0, 0.0, 0.0),
                                        (-half, 0.0, -half), cell, cells, cells, 0, want_xyz=True)
    zero = torch.zeros((1, 1), dtype=torch.float32, device=dev)
    own = int(ops.unproject_grid_index(zero, T, (0.5, 0.5, 0.5, 0.5), (0.0, 0.0, 0.0), (-half, 0.0, -half), cell, cells, cells, 0))
    return idx, xyz, own


def composed_record(proj, xyz, N, own, band=BAND):
    c = proj.reshape(-1).long()
    y = xyz.reshape(-1, 3)[:, 1]
    ok = (c >= 0) & (c < N) & (c != own) & torch.isfinite(y) & (y.abs() <= 1000.0)
    c, q = c[ok], torch.round(y[ok] * 1000.0).to(torch.int32)
    rec = torch.empty((4, N), dtype=torch.int32, device=proj.device)
    rec[0] = torch.bincount(c, minlength=N)
    rec[1] = torch.bincount(c[(q >= band[0]) & (q <= band[1])], minlength=N)
    rec[2].fill_(2 ** 31 - 1).scatter_reduce_(0, c, q, "amin")
    rec[3].fill_(-2 ** 31).scatter_reduce_(0, c, q, "amax")
    return rec


def composed_kinds(rec, labels, min_hits=4):
    k = torch.where(rec[1] >= min_hits, 2, torch.where(rec[0] > 0, 1, 0))
    return torch.where(labels >= 0, 3, k).to(torch.uint8)


def rooms_record(cells, seed, dev):
    """(record [4, N], object_labels [N], objects [16]) of a floor plan: walls every 40 or so cells with doors, seen as heights;
    furniture as labelled objects; the outer tenth of the map never seen."""
    rng = np.random.default_rng(seed)
    rows = cols = cells
    wall = np.zeros((rows, cols), bool)
    for r in range(40, rows - 8, 40):
        wall[r, :] = True
        for c0 in range(0, cols, 40):
            d = c0 + int(rng.integers(4, 34))
            wall[r, d:d + 3] = False
    for c in range(40, cols - 8, 40):
        wall[:, c] = True
        for r0 in range(0, rows, 40):
            d = r0 + int(rng.integers(4, 34))
            wall[d:d + 3, c] = False
    wall |= rng.random((rows, cols)) < 0.002                         # flying pixels: specks
    labels = np.full((rows, cols), -1, np.int32)
    objects = []
    for _ in range(rows * cols // 2000):
        r, c = int(rng.integers(0, rows - 4)), int(rng.integers(0, cols - 4))
        if (labels[r:r + 3, c:c + 4] >= 0).any():
            continue
        labels[r:r + 3, c:c + 4] = r * cols + c
        objects.append(r * cols + c)
    rr, cc = np.mgrid[0:rows, 0:cols]
    seen = np.hypot(rr - rows / 2, cc - cols / 2) < 0.45 * rows * (1.0 + 0.1 * rng.random((rows, cols)))
    N = rows * cols
    rec = np.zeros((4, N), np.int32)
    hits = np.where(seen, rng.integers(3, 60, (rows, cols)), 0)
    band = np.where(wall & seen, np.minimum(hits, rng.integers(4, 40, (rows, cols))), np.where(seen, rng.integers(0, 3, (rows, cols)), 0))
    lo = rng.integers(-30, 40, (rows, cols))
    rec[0], rec[1] = np.maximum(hits, band).reshape(-1), band.reshape(-1)
    rec[2] = np.where(seen, lo, 2 ** 31 - 1).reshape(-1)
    rec[3] = np.where(seen, lo + np.where(wall, rng.integers(1500, 2400, (rows, cols)), rng.integers(0, 60, (rows, cols))), -2 ** 31).reshape(-1)
    objs = (objects + [-1] * 16)[:16]
    return (torch.from_numpy(rec).to(dev), torch.from_numpy(labels.reshape(-1)).to(dev), torch.tensor(objs, dtype=torch.int32, device=dev))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "obstacles_bench.txt"))
    ap.add_argument("--op-only", action="store_true")
    ap.add_argument("--heights-only", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("obstacles_bench: no GPU visible; nothing is measured without one")
    launches = max(20, args.launches)
    dev = torch.device("cuda:0")
    _lib.load()
    lines = [f"map_heights and map_obstacles vs the same composed in torch: {launches} event-timed calls each, alternating, after "
             "warm-up", f"device: {torch.cuda.get_device_name(0)}; ms as median [min, max]", ""]
    print("\n".join(lines), flush=True)
    for S, cells, cell in FRAMES:
        N = cells * cells
        proj, xyz, own = project(room_depth(S, S), cells, cell, dev)
        worst = torch.full_like(proj, N // 2 + 7)
        for name, pr in (("frame", proj), ("one cell", worst)):
            fresh = lambda: ops.new_height_record(N, dev)
            once = ops.map_heights(pr, xyz, fresh(), band_mm=BAND, exclude_cell=own)
            again = ops.map_heights(pr, xyz, fresh(), band_mm=BAND, exclude_cell=own)
            want = composed_record(pr, xyz, N, own)
            head = f"{S} x {S} pixels over {cells} x {cells} cells, {name}"
            if not torch.equal(once, again):
                raise SystemExit(f"obstacles_bench: {head}: two calls of map_heights differ; nothing is written")
            if not torch.equal(once, want):
                raise SystemExit(f"obstacles_bench: {head}: the composed record is not the op's; nothing is timed or written")
            record = fresh()
            calls = {"heights": lambda: ops.map_heights(pr, xyz, record, band_mm=BAND, exclude_cell=own)}
            if not args.op_only:
                calls["composed"] = lambda: composed_record(pr, xyz, N, own)
            t = timed(calls, launches)
            block = [f"{head}: {int((once[0] > 0).sum())} cells hit, {int(once[0].sum())} valid pixels, {int(once[1].sum())} in the band "
                     f"{BAND[0]}..{BAND[1]} mm"]
            block += [f"  {k:10s} {fmt(v)}  ({len(v)} calls)" for k, v in t.items()]
            if not args.op_only:
                block.append(f"  composed / heights = {np.median(t['composed']) / np.median(t['heights']):.1f}; the composed record is "
                             "the op's: True; two calls of the op agree bitwise: True")
            block.append("")
            print("\n".join(block), flush=True)
            lines += block
    for _, cells, _ in (() if args.heights_only else FRAMES):
        N = cells * cells
        rec, labels, objs = rooms_record(cells, cells, dev)
        ws = torch.empty((ops.map_obstacles_workspace(N, cells),), dtype=torch.int32, device=dev)
        op = lambda: ops.map_obstacles(rec, cells, object_labels=labels, objects=objs, min_hits=4, min_cells=2, topk=16, workspace=ws)
        out = {k: v.clone() for k, v in op().items()}
        again = op()
        head = f"{cells} x {cells} = {N} cells"
        if not all(torch.equal(out[k], again[k]) for k in out):
            raise SystemExit(f"obstacles_bench: {head}: two calls of map_obstacles differ; nothing is written")
        if not torch.equal(composed_kinds(rec, labels), out["kind"]):
            raise SystemExit(f"obstacles_bench: {head}: the composed kinds are not the op's; nothing is timed or written")
        calls = {"obstacles": op}
        if not args.op_only:
            calls["kinds"] = lambda: composed_kinds(rec, labels)
        t = timed(calls, launches)
        block = [f"{head}: counts {out['counts'].tolist()} (UNSEEN, CLEAR, OBSTACLE, OBJECT, structures, speck cells), "
                 f"{int(out['count'])} structures of 2 cells or more; area {out['area'][:4].tolist()}, top_mm {out['top_mm'][:4].tolist()}, "
                 f"obj_cells {out['obj_cells'][:4].tolist()}, status {out['status'].tolist()}"]
        block += [f"  {k:10s} {fmt(v)}  ({len(v)} calls)" for k, v in t.items()]
        if not args.op_only:
            block.append("  the composed kinds are the op's: True; two calls of the op agree bitwise: True")
        block.append("")
        print("\n".join(block), flush=True)
        lines += block
    from embodied_object_detection_amd.build import resource_usage
    for name, u in sorted(resource_usage().items()):
        if "obstacles_" in name or "heights_kernel" in name:
            lines.append(f"{name}: {u.get('vgprs')} VGPRs, {u.get('lds')} bytes of static LDS, {u.get('occupancy')} waves per SIMD, "
                         f"{u.get('scratch')} bytes of scratch")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
