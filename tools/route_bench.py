#!/usr/bin/env python
"""Event-timed `map_route` against what a user composes in torch without it, in one process: maps of 200 x 200 (40 000 cells) and
512 x 512 (262 144 cells); at each size the inventory's label map of the synthetic model after three 640 x 640 frames with its 16
largest objects (level 2 ** -11: every labelled cell is in an object), the same map with its largest object passable and the
start inside it, and a serpentine (a wall every 8 rows with a gap at
alternating ends).  Everything is warmed up, then timed alternately, one pair of device events per call, at least 20 calls each;
medians with [min, max].

  route       `ops.map_route(labels, objects, cols, from_cell, path_max=256, sweeps=S)`: init, S sweep launches, finish and path
              launches.  S is found before the timing: the smallest multiple of 4 after which one call leaves status 0 (a map that
              needs more than 1024 sweeps is timed as the chain of resumed calls that settles it)
  chase       the same call with path_max = 1024 (the serpentines: their paths are longer than that)
  floor       the same op with `sweeps` at its default on a map of the same size where only the start is free: the queued launches
              with no tile to run after the first
  composed    on the device: dist under the eight shifted minima with the corner rule (eight legality masks, built per call),
              iterated until unchanged, checked on the host every 16 rounds.  It gives `dist` alone, without parent, goals or
              paths.  Where one call takes long, fewer than 20 calls are timed (printed)

Also printed: whether the composed dist is the op's, and whether two calls of the op agree in their bits.

    python tools/route_bench.py [--launches 20] [--out profiles/route_bench.txt] [--lib OTHER.so --tile 64 64]

`--lib` times a library built with other tile constants (-DEOD_ROUTE_TILE_ROWS=64 -DEOD_ROUTE_TILE_COLS=64); `--tile` tells the
default sweep count what they are.
"""
import argparse
import os
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from embodied_object_detection_amd import _lib, build_model, ops, setup_cfg          # noqa: E402
from embodied_object_detection_amd.checkpoint import synthetic_state_dict            # noqa: E402
from embodied_object_detection_amd.data.synthetic import SyntheticSequence           # noqa: E402

GRIDS = ((200, 200, 0.2), (512, 512, 0.08))
TOPK = 16
INT_MAX = 2 ** 31 - 1
INF = 1 << 29                                                        # the composed form's "unreached": INF + INF stays an int32
MOVES = ((-1, -1), (-1, 0), (-1, 1), (0, -1), (0, 1), (1, -1), (1, 0), (1, 1))
COMPOSED_BUDGET_S = 20.0


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


def composed(labels, rows, cols, from_cell, passable=()):
    """What a user writes today: dist int32 [N] (INT_MAX: blocked or unreached), and the rounds it took."""
    free = (labels < 0).view(rows, cols).clone()
    for p in passable:
        free |= (labels == p).view(rows, cols)
    free.view(-1)[from_cell] = True
    fp = F.pad(free, (1, 1, 1, 1), value=False)

    def shifted(t, dr, dc):                                          # the value at (r + dr, c + dc)
        return t[1 + dr:1 + dr + rows, 1 + dc:1 + dc + cols]
    cost = []
    for dr, dc in MOVES:
        ok = free & shifted(fp, dr, dc)
        if dr and dc:
            ok = ok & shifted(fp, dr, 0) & shifted(fp, 0, dc)        # both cells the move passes between
        cost.append(torch.where(ok, 7 if dr and dc else 5, INF).to(torch.int32))
    d = torch.full((rows, cols), INF, dtype=torch.int32, device=labels.device)
    d.view(-1)[from_cell] = 0
    rounds = 0
    while True:
        before = d
        for _ in range(16):
            dp = F.pad(d, (1, 1, 1, 1), value=INF)
            for (dr, dc), w in zip(MOVES, cost):
                d = torch.minimum(d, shifted(dp, dr, dc) + w)
        rounds += 16
        if torch.equal(d, before):                                   # the host waits here
            break
    return torch.where(d >= INF, INT_MAX, d).view(-1), rounds


def serpentine(rows, cols, dev):
    g = torch.full((rows, cols), -1, dtype=torch.int32, device=dev)
    for n, w in enumerate(range(7, rows - 1, 8)):
        g[w, :] = 1
        g[w, cols - 1 if n % 2 == 0 else 0] = -1
    g[rows - 1, cols // 2] = 10                                      # an object in the last corridor
    return g.view(-1).contiguous()


def settle(labels, objects, cols, from_cell, path_max, passable):
    """The smallest multiple of 4 sweeps after which one call leaves status 0, or the chain of 1024-sweep calls that does."""
    for s in range(4, ops.ROUTE_SWEEPS_MAX + 1, 4):
        res = ops.map_route(labels, objects, cols, from_cell, passable=passable, path_max=path_max, sweeps=s)
        if int(res["status"][0]) == 0:
            return [s]
    chain = [ops.ROUTE_SWEEPS_MAX]
    while int(res["status"][0]) == 1 and len(chain) < 64:
        res = ops.map_route(labels, objects, cols, from_cell, passable=passable, path_max=path_max, sweeps=ops.ROUTE_SWEEPS_MAX, resume=res)
        chain.append(ops.ROUTE_SWEEPS_MAX)
    assert int(res["status"][0]) == 0, res["status"].tolist()
    return chain


def route_chain(labels, objects, cols, from_cell, path_max, chain, passable):
    res = ops.map_route(labels, objects, cols, from_cell, passable=passable, path_max=path_max, sweeps=chain[0])
    for s in chain[1:]:
        res = ops.map_route(labels, objects, cols, from_cell, passable=passable, path_max=path_max, sweeps=s, resume=res)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "route_bench.txt"))
    ap.add_argument("--lib", default=None)
    ap.add_argument("--tile", type=int, nargs=2, default=None, metavar=("ROWS", "COLS"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("route_bench: no GPU visible; nothing is measured without one")
    if args.lib:
        _lib.LIB_PATH = os.path.abspath(args.lib)
    if args.tile:
        ops.ROUTE_TILE_ROWS, ops.ROUTE_TILE_COLS = args.tile
    launches = max(20, args.launches)
    dev = torch.device("cuda:0")
    _lib.load()
    sd = synthetic_state_dict(0)
    lines = [f"map_route vs dist under eight shifted minima in torch: {launches} event-timed calls each, alternating, after warm-up",
             f"device: {torch.cuda.get_device_name(0)}; tiles of {ops.ROUTE_TILE_ROWS} x {ops.ROUTE_TILE_COLS} cells"
             + (f" ({os.path.basename(args.lib)})" if args.lib else "") + "; ms as median [min, max]", ""]
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
        free = torch.nonzero(inv_labels < 0).view(-1)
        inv_from = int(free[0]) if free.numel() else 0
        only_start = torch.ones((N,), dtype=torch.int32, device=dev)
        default = ops.map_route_sweeps(map_w, map_h)
        ten = torch.tensor([10], dtype=torch.int32, device=dev)
        big = inv_objects[:1].clone()                                 # the largest object: the synthetic scene's background class
        in_big = torch.nonzero(inv_labels == big[0]).view(-1)
        big_from = int(in_big[in_big.numel() // 2]) if in_big.numel() else inv_from
        for name, labels, objects, from_cell, passable in (("inventory", inv_labels, inv_objects, inv_from, None),
                                                           ("inventory, its largest object passable", inv_labels, inv_objects, big_from, big),
                                                           ("serpentine", serpentine(map_w, map_h, dev), ten, 0, None)):
            host_pass = [] if passable is None else passable.tolist()
            chain = settle(labels, objects, map_h, from_cell, 256, passable)
            route = lambda pm=256: route_chain(labels, objects, map_h, from_cell, pm, chain, passable)
            out = {k: v.clone() for k, v in route().items()}
            again = route()
            op_same = all(torch.equal(out[k], again[k]) for k in out)
            t0 = time.time()
            cd, rounds = composed(labels, map_w, map_h, from_cell, host_pass)
            torch.cuda.synchronize()
            first = time.time() - t0
            dist_same = bool(torch.equal(cd, out["dist"]))
            n_composed = launches if first * (launches + 3) <= COMPOSED_BUDGET_S else max(2, int(COMPOSED_BUDGET_S / first))
            calls = {"route": (route, launches), "chase": (lambda: route(1024), launches),
                     "floor": (lambda: ops.map_route(only_start, ten, map_h, from_cell, sweeps=default), launches),
                     "composed": (lambda: composed(labels, map_w, map_h, from_cell, host_pass), min(launches, n_composed))}
            t = timed(calls, launches)
            med = {k: float(np.median(v)) for k, v in t.items()}
            counts = out["counts"].tolist()
            block = [f"{map_w} x {map_h} = {N} cells, {name}: from cell {from_cell}, {counts[0]} free cells, {counts[1]} reached; "
                     f"{int((objects >= 0).sum())} objects asked, {int((out['goal_cost'] < INT_MAX).sum())} reached, path_cells "
                     f"{out['path_cells'].tolist()}; largest dist {int(out['dist'][out['dist'] < INT_MAX].max())}",
                     f"  sweeps to status 0: {chain[0] if len(chain) == 1 else chain} (default {default}); composed rounds {rounds}"]
            for k, v in t.items():
                block.append(f"  {k:10s} {med[k]:9.3f} [{v[0]:.3f}, {v[-1]:.3f}] ms  ({len(v)} calls)")
            block.append(f"  per sweep launch: route {med['route'] / sum(chain) * 1e3:.2f} us, floor {med['floor'] / default * 1e3:.2f} us; "
                         f"chase - route = {(med['chase'] - med['route']) * 1e3:.1f} us; composed / route = {med['composed'] / med['route']:.1f}")
            block.append(f"  composed dist is the op's: {dist_same}; two calls of the op agree bitwise: {op_same}")
            block.append("")
            print("\n".join(block), flush=True)
            lines += block
        del model
        torch.cuda.empty_cache()
    if not args.lib:
        from embodied_object_detection_amd.build import resource_usage
        for name, u in sorted(resource_usage().items()):
            if "route_" in name:
                lines.append(f"{name}: {u.get('vgprs')} VGPRs, {u.get('lds')} bytes of LDS, {u.get('occupancy')} waves per SIMD, "
                             f"{u.get('scratch')} bytes of scratch")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
