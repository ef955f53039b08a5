#!/usr/bin/env python
"""Event-timed `map_relations` against what a user composes in torch without it, in one process: maps of 200 x 200 (40 000 cells)
and 512 x 512 (262 144 cells) on the synthetic model's memory after three 640 x 640 frames, the 16 largest objects of
`model.inventory` at level 2 ** -11 (every labelled cell is in an object), radius 1, 5 and 16.  Everything is warmed up, then timed
alternately, one pair of device events per call, at least 20 calls each; medians with [min, max].

  relations   `ops.map_relations(inv["object_labels"], inv["object"], cols, radius, from_cell, topn=4)`: init, pair and finish launches
  composed    per object one dilation of its mask by the disc (`F.conv2d` with the disc's 0/1 kernel, zero padding, `> 0`;
              `max_pool2d` dilates by the square and pads the same way), then all intersections at once, masks @ dilated.T: K + 2
              launches and 2 K temporaries of map size for `near_cells` alone, without min_d2, closest, edges, nearest or from_*
  floor       the same op on a 1 x 1 map: its three launches with nothing to do
  bound       the labels the pair launch has to read, 4 N bytes at 6.3 TB/s from HBM (both maps stay in the Infinity Cache between
              calls), plus the floor

Also printed: whether the composed near_cells are the op's, and whether two calls of the op agree in their bits.

    python tools/relations_bench.py [--launches 20] [--out profiles/relations_bench.txt]
"""
import argparse
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from embodied_object_detection_amd import _lib, build_model, ops, setup_cfg          # noqa: E402
from embodied_object_detection_amd.checkpoint import synthetic_state_dict            # noqa: E402
from embodied_object_detection_amd.data.synthetic import SyntheticSequence           # noqa: E402

GRIDS = ((200, 200, 0.2), (512, 512, 0.08))
RADII = (1, 5, 16)
TOPK = 16
HBM_BYTES_PER_MS = 6.3e9


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


def disc_kernel(R, dev):
    d = torch.arange(-R, R + 1, device=dev)
    return ((d[:, None] ** 2 + d[None, :] ** 2) <= R * R).to(torch.float32)[None, None]


def composed(labels, objects, rows, cols, kernel):
    """What a user writes today: near_cells int64 [K, K] (the diagonal holds the objects' cells)."""
    R = kernel.shape[-1] // 2
    grid = labels.view(1, 1, rows, cols)
    masks, dilated = [], []
    for obj in objects:
        m = (grid == obj).to(torch.float32) if obj >= 0 else torch.zeros_like(grid, dtype=torch.float32)
        masks.append(m.view(-1))
        dilated.append((F.conv2d(m, kernel, padding=R) > 0).to(torch.float32).view(-1))
    return (torch.stack(masks) @ torch.stack(dilated).t()).to(torch.int64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "relations_bench.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("relations_bench: no GPU visible; nothing is measured without one")
    launches = max(20, args.launches)
    dev = torch.device("cuda:0")
    _lib.load()
    sd = synthetic_state_dict(0)
    lines = [f"map_relations vs one disc dilation per object + intersections in torch: {launches} event-timed calls each, alternating, "
             f"after warm-up",
             f"device: {torch.cuda.get_device_name(0)}; the {TOPK} largest objects of model.inventory; ms as median [min, max]", ""]
    print("\n".join(lines), flush=True)
    one = torch.zeros((1,), dtype=torch.int32, device=dev)
    for map_w, map_h, cell in GRIDS:
        N = map_w * map_h
        cfg = setup_cfg(None, ["MODEL.MEMORY_TYPE", "implicit_memory", "MODEL.MAP_FEAT_FUSION", "sum", "MODEL.MAP_FEATURE_WEIGHT", 5,
                               "MODEL.MEMORY_CLS_SCORE_THRESH", 0.3, "MODEL.DEVICE", "cuda:0"])
        model = build_model(cfg, sd)
        seq = SyntheticSequence(7, H=640, W=640, n_frames=3, map_w=map_w, map_h=map_h, cell=cell)
        for i in range(3):
            model([[seq.frame(i)]])
        inv = model.inventory(thresh=0.0, map_shape=(map_w, map_h), level=2.0 ** -11, topk=TOPK)
        labels, objects = inv["object_labels"].clone(), inv["object"].clone()
        host_objects = objects.tolist()
        from_cell = (map_w // 2) * map_h + map_h // 2
        tr, tc = ops.RELATIONS_TILE_ROWS, ops.RELATIONS_TILE_COLS
        slot = torch.isin(labels, objects[objects >= 0]).view(map_w, map_h)
        pad = torch.zeros((-(-map_w // tr) * tr, -(-map_h // tc) * tc), dtype=torch.bool, device=dev)
        pad[:map_w, :map_h] = slot
        busy = int(pad.view(pad.shape[0] // tr, tr, pad.shape[1] // tc, tc).any(dim=3).any(dim=1).sum())
        tiles = (pad.shape[0] // tr) * (pad.shape[1] // tc)
        for R in RADII:
            kernel = disc_kernel(R, dev)
            rel = lambda: ops.map_relations(labels, objects, map_h, radius=R, from_cell=from_cell, topn=4)
            out = {k: v.clone() for k, v in rel().items()}
            again = rel()
            op_same = all(torch.equal(out[k], again[k]) for k in out)
            near = composed(labels, host_objects, map_w, map_h, kernel)
            K = len(host_objects)
            off = ~torch.eye(K, dtype=torch.bool, device=dev)
            near_same = bool(torch.equal(near[off], out["near_cells"].to(torch.int64)[off]))
            calls = {"relations": rel, "composed": lambda: composed(labels, host_objects, map_w, map_h, kernel),
                     "floor": lambda: ops.map_relations(one, one, 1, radius=R, from_cell=0, topn=4)}
            t = timed(calls, launches)
            med = {k: float(np.median(v)) for k, v in t.items()}
            bound = 4 * N / HBM_BYTES_PER_MS + med["floor"]
            block = [f"{map_w} x {map_h} = {N} cells, radius {R}: {int(inv['count'])} objects, the {int((objects >= 0).sum())} asked hold "
                     f"{int(out['cells'].sum())} cells (largest {out['cells'][:4].tolist()}) in {busy} of {tiles} tiles; "
                     f"{int((out['min_d2'] < 2 ** 31 - 1).sum()) // 2} pairs within reach, {int(out['edges'].sum()) // 2} border pairs"]
            for k, v in t.items():
                block.append(f"  {k:10s} {med[k]:9.3f} [{v[0]:.3f}, {v[-1]:.3f}] ms")
            block.append(f"  bound: {4 * N / 1e6:.2f} MB of labels at 6.3 TB/s = {4e3 * N / HBM_BYTES_PER_MS:.2f} us + floor = {bound:.4f} ms; "
                         f"relations / bound = {med['relations'] / bound:.1f}; composed / relations = {med['composed'] / med['relations']:.1f}")
            block.append(f"  composed near_cells are the op's: {near_same}; two calls of the op agree bitwise: {op_same}")
            block.append("")
            print("\n".join(block), flush=True)
            lines += block
        del model
        torch.cuda.empty_cache()
    from embodied_object_detection_amd.build import resource_usage
    for name, u in sorted(resource_usage().items()):
        if "relations_" in name:
            lines.append(f"{name}: {u.get('vgprs')} VGPRs, {u.get('lds')} bytes of LDS, {u.get('occupancy')} waves per SIMD, "
                         f"{u.get('scratch')} bytes of scratch")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
