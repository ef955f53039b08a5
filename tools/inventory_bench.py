#!/usr/bin/env python
"""Event-timed `map_inventory` against the `semantic_map(scores=True)` call it follows and against what a user composes without it,
in one process: maps of 200 x 200 (40 000 cells) and 512 x 512 (262 144 cells) on the synthetic model's memory after three
640 x 640 frames, read with the model's own 20 classes and with the 1203 classes of the LVIS fixture, B = 1 and B = 4 maps per call.
Everything is warmed up, then timed alternately, one pair of device events per call, at least 20 calls each; medians with [min, max].

  maps       `labels`, `scores` of `model.semantic_map(thresh=0, scores=True)`; for B = 4 the map and three copies of it rolled by
             different numbers of cells (different maps of the same statistics).  Two levels: 2 ** -11, which keeps every labelled
             cell, and the median of the distinct scores, which cuts the map.
  inventory  `ops.map_inventory(labels, scores, cols, C, level, topk=16)` with a caller-held workspace
  semmap     `model.semantic_map(thresh=0, scores=True)` in the same vocabulary: the call that produces one map
  composed   what a user writes today for the same answer: the classes present among the foreground, found on the host (a sync),
             then per map `ops.map_regions` on 32-class chunks of `where(labels == c, scores, 0)`; the rankings are left unmerged.
             Its label maps are checked against the op's.

    python tools/inventory_bench.py [--launches 20] [--out profiles/inventory_bench.txt]
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from embodied_object_detection_amd import _lib, build_model, ops, setup_cfg          # noqa: E402
from embodied_object_detection_amd.checkpoint import synthetic_state_dict            # noqa: E402
from embodied_object_detection_amd.data.synthetic import SyntheticSequence           # noqa: E402

GRIDS = ((200, 200, 0.2), (512, 512, 0.08))
LVIS = os.path.join(ROOT, "tests", "golden", "lvis_v1_clip.npy")
VOCABS = (("own 20 classes", 20, dict()), ("LVIS, 1203 classes", 1203, dict(classifier=LVIS, num_classes=1203)))
BS = (1, 4)
TOPK = 16


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


def composed(labels, scores, cols, level):
    """[(classes, regions dict)] per map and chunk: unique labels on the host, then `map_regions` on 32-class chunks."""
    res = []
    for b in range(labels.shape[0]):
        lab, sc = labels[b], scores[b]
        present = torch.unique(lab[(lab >= 0) & (sc >= level)]).tolist()              # the host learns the classes here
        for i in range(0, len(present), ops.REGIONS_Q_MAX):
            chunk = present[i:i + ops.REGIONS_Q_MAX]
            ids = torch.tensor(chunk, dtype=torch.int32, device=lab.device)
            prob = torch.where(lab[None, :] == ids[:, None], sc[None, :], torch.zeros((), device=lab.device))
            res.append((b, chunk, ops.map_regions(prob, cols, level, topk=TOPK)))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "inventory_bench.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("inventory_bench: no GPU visible; nothing is measured without one")
    launches = max(20, args.launches)
    dev = torch.device("cuda:0")
    _lib.load()
    sd = synthetic_state_dict(0)
    lines = [f"map_inventory vs the semantic_map(scores=True) call before it and vs unique labels on the host + map_regions on 32-class "
             f"chunks: {launches} event-timed calls each, alternating, after warm-up",
             f"device: {torch.cuda.get_device_name(0)}; topk {TOPK}, connectivity 8; ms as median [min, max]", ""]
    print("\n".join(lines), flush=True)
    for map_w, map_h, cell in GRIDS:
        N = map_w * map_h
        cfg = setup_cfg(None, ["MODEL.MEMORY_TYPE", "implicit_memory", "MODEL.MAP_FEAT_FUSION", "sum", "MODEL.MAP_FEATURE_WEIGHT", 5,
                               "MODEL.MEMORY_CLS_SCORE_THRESH", 0.3, "MODEL.DEVICE", "cuda:0"])
        model = build_model(cfg, sd)
        seq = SyntheticSequence(7, H=640, W=640, n_frames=3, map_w=map_w, map_h=map_h, cell=cell)
        for i in range(3):
            model([[seq.frame(i)]])
        for vname, C, vocab in VOCABS:
            semmap = lambda: model.semantic_map(thresh=0.0, scores=True, **vocab)
            lab1, sc1 = (t.clone() for t in semmap())
            distinct = torch.unique(sc1[lab1 >= 0])
            for B in BS:
                shifts = [0, 37, N // 3 + 11, N // 2 + 5][:B]
                labels = torch.stack([torch.roll(lab1, s) for s in shifts]).contiguous()
                scores = torch.stack([torch.roll(sc1, s) for s in shifts]).contiguous()
                ws = torch.empty((ops.map_inventory_workspace(B, N, C, TOPK),), dtype=torch.int32, device=dev)
                for level in (2.0 ** -11, float(distinct[distinct.numel() // 2])):
                    inventory = lambda: ops.map_inventory(labels, scores, map_h, C, level=level, topk=TOPK, workspace=ws)
                    out = inventory()
                    assert int(out["status"]) == 0
                    parts = composed(labels, scores, map_h, level)
                    for b, chunk, reg in parts:                                   # the composed answer labels the cells alike
                        for q, c in enumerate(chunk):
                            want = torch.where(labels[b] == c, out["object_labels"][b], torch.full_like(labels[b], -1))
                            assert torch.equal(reg["region_labels"][q], want), "the two formulations label differently"
                    calls = {"inventory": inventory, "semmap": semmap, "composed": lambda: composed(labels, scores, map_h, level)}
                    t = timed(calls, launches)
                    med = {k: float(np.median(v)) for k, v in t.items()}
                    block = [f"{map_w} x {map_h} = {N} cells, {vname}, B = {B}, level {level:.4g}: foreground {out['foreground'].tolist()}, "
                             f"objects {out['count'].tolist()}, classes present {(out['class_cells'] > 0).sum(dim=1).tolist()}, largest "
                             f"{out['area'][:, 0].tolist()}; composed: {len(parts)} map_regions calls"]
                    for k, v in t.items():
                        block.append(f"  {k:9s} {med[k]:9.3f} [{v[0]:.3f}, {v[-1]:.3f}] ms")
                    block.append(f"  composed / inventory = {med['composed'] / med['inventory']:.1f}; inventory / semmap = "
                                 f"{med['inventory'] / med['semmap']:.2f} (semmap produces one of the {B})")
                    block.append("")
                    print("\n".join(block), flush=True)
                    lines += block
                del ws
        del model
        torch.cuda.empty_cache()
    from embodied_object_detection_amd.build import resource_usage
    for name, u in sorted(resource_usage().items()):
        if "inventory_" in name or "regions_" in name:
            lines.append(f"{name}: {u.get('vgprs')} VGPRs, {u.get('lds')} bytes of LDS, {u.get('occupancy')} waves per SIMD, "
                         f"{u.get('scratch')} bytes of scratch")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
