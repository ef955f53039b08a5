#!/usr/bin/env python
"""Event-timed `map_rooms` against the same per-cell result composed in torch, in one process.

  rooms       `ops.map_rooms(labels, d2, cols, door_r2, min_cells, topk=16, objects)` with a workspace of the caller's, at
              200 x 200 = 40 000 and 512 x 512 = 262 144 cells, on three maps: `open plan` (one hall with pillars), `flat` (walls
              every 40 cells with doors of three cells: many rooms) and `corridor` (a room and a corridor one cell wide wound across
              the whole map: the grow crosses a tile border per sweep).  `d2` is that of `ops.map_clearance`, computed once outside
              the timing, as a caller that already has it would.  `sweeps` is the smallest power of two at which status is 0
  composed    `room_labels` and `grow_dist` alone in torch: the threshold, the core regions by iterated minima over the four
              neighbours, the areas by `bincount`, the grow by iterated minima over the eight shifted key planes with the corner rule
              as masks; each loop stops when an iteration changes nothing, looked at every 16 iterations (one synchronisation each).
              Checked equal to the op's before the timing.  No ranking, no per-room, per-door or per-object values

Everything is warmed up, then timed alternately, one pair of device events per call; medians with [min, max].  The tool stops, and
writes nothing, if the composed result is not the op's or if two calls of the op differ in a bit.

    python tools/rooms_bench.py [--launches 20] [--out profiles/rooms_bench.txt] [--op-only] [--lib path/to/a/variant.so]

`--op-only` times the op alone (for a kernel trace); `--lib` binds `eod_map_rooms` from another library (a variant build of
csrc/rooms.hip alone) in place of the package's, for comparing builds.
"""
import argparse
import ctypes
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from embodied_object_detection_amd import _lib, ops          # noqa: E402

SIDES = (200, 512)
INF = 1 << 62


def timed(calls, launches):
    """{name: sorted event times in ms} of `calls` {name: (callable, launches, warm-up calls)}, warmed up, then alternating."""
    for f, _, warm in calls.values():
        for _ in range(warm):
            f()
    torch.cuda.synchronize()
    times = {k: [] for k in calls}
    for n in range(launches):
        for k, (f, own, _) in calls.items():
            if n >= own:
                continue
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            f()
            b.record()
            b.synchronize()
            times[k].append(a.elapsed_time(b))
    return {k: sorted(v) for k, v in times.items()}


def fmt(t):
    return f"{float(np.median(t)):10.3f} [{t[0]:.3f}, {t[-1]:.3f}] ms"


def open_plan(S, seed):
    rng = np.random.default_rng(seed)
    m = np.full((S, S), -1, np.int32)
    m[0], m[-1], m[:, 0], m[:, -1] = 0, 0, 0, 0
    for _ in range(S // 10):
        r, c = int(rng.integers(4, S - 6)), int(rng.integers(4, S - 6))
        m[r:r + 2, c:c + 2] = r * S + c                                    # a pillar, an object of its own
    return m


def flat(S, seed):
    rng = np.random.default_rng(seed)
    m = np.full((S, S), -1, np.int32)
    m[0], m[-1], m[:, 0], m[:, -1] = 0, 0, 0, 0
    for r in range(40, S - 8, 40):
        m[r, :] = 0
    for c in range(40, S - 8, 40):
        m[:, c] = 0
    for r in range(40, S - 8, 40):
        for c0 in range(0, S, 40):
            d = c0 + int(rng.integers(4, 34))
            m[r, d:d + 3] = -1
    for c in range(40, S - 8, 40):
        for r0 in range(0, S, 40):
            d = r0 + int(rng.integers(4, 34))
            m[d:d + 3, c] = -1
    m[0], m[-1], m[:, 0], m[:, -1] = 0, 0, 0, 0
    for _ in range(S * S // 2000):
        r, c = int(rng.integers(2, S - 6)), int(rng.integers(2, S - 6))
        if (m[r - 1:r + 4, c - 1:c + 5] >= 0).any():
            continue
        m[r:r + 3, c:c + 4] = r * S + c                                    # furniture
    return m


def corridor(S, pitch):
    """A room of 9 x 9 cells in the corner and a corridor one cell wide that leaves it and winds across the map, a lane every
    `pitch` rows."""
    m = np.zeros((S, S), np.int32)
    room = 9
    m[1:1 + room, 1:1 + room] = -1
    r, lo, hi = 1 + room // 2, room + 2, S - 2
    m[r, 1 + room:hi + 1] = -1
    right = True
    while r + pitch <= S - 2:
        m[r:r + pitch, hi if right else lo] = -1
        r += pitch
        m[r, lo:hi + 1] = -1
        right = not right
    return m


def shifted(t, dr, dc, fill):
    """t moved so that out[r, c] = t[r - dr, c - dc], `fill` where that is outside."""
    out = torch.full_like(t, fill)
    R, C = t.shape
    out[max(dr, 0):R + min(dr, 0), max(dc, 0):C + min(dc, 0)] = t[max(-dr, 0):R + min(-dr, 0), max(-dc, 0):C + min(-dc, 0)]
    return out


def composed(blocked, d2, door_r2, min_cells):
    """(room_labels, grow_dist) [R, C] in torch; blocked bool [R, C], d2 int32 [R, C]."""
    R, C = blocked.shape
    N = R * C
    free = ~blocked
    core = free & (d2 > door_r2)
    idx = torch.arange(N, device=blocked.device, dtype=torch.int64).view(R, C)
    lab = torch.where(core, idx, N)
    while True:
        for _ in range(16):
            m = lab
            for dr, dc in ((1, 0), (-1, 0), (0, 1), (0, -1)):
                m = torch.minimum(m, shifted(lab, dr, dc, N))
            new = torch.where(core, m, N)
            same = torch.equal(new, lab) if _ == 15 else False
            lab = new
        if same:
            break
    area = torch.bincount(lab[core], minlength=N + 1)
    room = core & (area[lab.clamp(max=N)] >= min_cells)
    key = torch.where(room, lab, INF)
    moves = []
    for dr in (-1, 0, 1):
        for dc in (-1, 0, 1):
            if dr == 0 and dc == 0:
                continue
            ok = free & shifted(free, dr, dc, False)                        # into a free cell from a free cell
            if dr and dc:
                ok = ok & shifted(free, dr, 0, False) & shifted(free, 0, dc, False)      # both cells passed between
            moves.append((dr, dc, (7 if dr and dc else 5) << 32, ok))
    while True:
        for n in range(16):
            m = key
            for dr, dc, w, ok in moves:
                m = torch.minimum(m, torch.where(ok, shifted(key, dr, dc, INF) + w, INF))
            new = torch.where(m >= INF, INF, m)
            same = torch.equal(new, key) if n == 15 else False
            key = new
        if same:
            break
    got = key < INF
    return (torch.where(got, key & 0xFFFFFFFF, -1).to(torch.int32), torch.where(got, key >> 32, 2 ** 31 - 1).to(torch.int32))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rooms_bench.txt"))
    ap.add_argument("--op-only", action="store_true")
    ap.add_argument("--lib", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("rooms_bench: no GPU visible; nothing is measured without one")
    launches = max(20, args.launches)
    dev = torch.device("cuda:0")
    lib = _lib.load()
    if args.lib:
        other = ctypes.CDLL(os.path.abspath(args.lib))
        res, argtypes = _lib.ROOMS_SIGNATURES["eod_map_rooms"]
        other.eod_map_rooms.restype, other.eod_map_rooms.argtypes = res, argtypes
        lib.eod_map_rooms = other.eod_map_rooms
    lines = [f"map_rooms vs room_labels and grow_dist composed in torch: {launches} event-timed calls of the op, 3 of the composed form, "
             "alternating, after warm-up", f"device: {torch.cuda.get_device_name(0)}; ms as median [min, max]"
             + (f"; eod_map_rooms from {os.path.basename(args.lib)}" if args.lib else ""), ""]
    print("\n".join(lines), flush=True)
    for S in SIDES:
        N = S * S
        for name, grid, door_r2, min_cells in (("open plan", open_plan(S, S), 4, 20), ("flat", flat(S, S + 1), 4, 20),
                                               ("corridor", corridor(S, 4 if S <= 200 else 16), 1, 4)):
            labels = torch.from_numpy(grid.reshape(-1)).to(dev)
            objs = sorted(set(grid[grid > 0].tolist()))[:15] + [0]
            objects = torch.tensor(objs, dtype=torch.int32, device=dev)
            d2 = ops.map_clearance(labels, objects, S)["d2"]
            ws = torch.empty((ops.map_rooms_workspace(N, S),), dtype=torch.int32, device=dev)
            sweeps = 8
            while True:
                op = lambda: ops.map_rooms(labels, d2, S, door_r2, min_cells=min_cells, topk=16, objects=objects, sweeps=sweeps, workspace=ws)
                out = {k: v.clone() for k, v in op().items()}
                if int(out["status"][0]) == 0 or sweeps == ops.ROOMS_SWEEPS_MAX:
                    break
                sweeps *= 2
            head = f"{S} x {S} = {N} cells, {name}, door_r2 {door_r2}, min_cells {min_cells}, {sweeps} sweeps"
            if int(out["status"][0]) != 0:
                raise SystemExit(f"rooms_bench: {head}: status {out['status'].tolist()}; nothing is written")
            again = op()
            if not all(torch.equal(out[k], again[k]) for k in out):
                raise SystemExit(f"rooms_bench: {head}: two calls of map_rooms differ; nothing is written")
            calls = {"rooms": (op, launches, 3)}
            if not args.op_only:
                blocked, d2g = (labels >= 0).view(S, S), d2.view(S, S)
                rl, gd = composed(blocked, d2g, door_r2, min_cells)
                if not (torch.equal(rl.view(-1), out["room_labels"]) and torch.equal(gd.view(-1), out["grow_dist"])):
                    raise SystemExit(f"rooms_bench: {head}: the composed rooms are not the op's; nothing is timed or written")
                calls["composed"] = (lambda: composed(blocked, d2g, door_r2, min_cells), 3, 0)      # the check above warmed it up
            t = timed(calls, launches)
            block = [f"{head}: {int(out['count'])} rooms, counts {out['counts'].tolist()} (blocked, void, free, core, grown, unassigned); "
                     f"area {out['area'][:4].tolist()}, doorways {int((out['door_edges'] > 0).sum()) // 2}, the farthest grown cell "
                     f"{int(out['grow_dist'][out['grow_dist'] < 2 ** 31 - 1].max())}"]
            block += [f"  {k:10s} {fmt(v)}  ({len(v)} calls)" for k, v in t.items()]
            if not args.op_only:
                block.append(f"  composed / rooms = {np.median(t['composed']) / np.median(t['rooms']):.0f}; the composed rooms are the "
                             "op's: True; two calls of the op agree bitwise: True")
            block.append("")
            print("\n".join(block), flush=True)
            lines += block
    from embodied_object_detection_amd.build import resource_usage
    for name, u in sorted(resource_usage().items()):
        if "rooms_" in name:
            short = name[name.index("rooms_"):].split("kernel")[0] + "kernel"
            lines.append(f"{short}: {u.get('vgprs')} VGPRs, {u.get('lds')} bytes of static LDS, {u.get('occupancy')} waves per SIMD, "
                         f"{u.get('scratch')} bytes of scratch")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
