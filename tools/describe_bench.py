#!/usr/bin/env python
"""Event-timed `describe_pool` and `describe_classify` against what a user composes in torch without them, in one process: maps of
200 x 200 (40 000 cells) and 512 x 512 (262 144 cells) on the synthetic model's memory after three 640 x 640 frames, the 16 largest
objects of `model.inventory` at two levels: 2 ** -11, which keeps every labelled cell, and the median of the distinct scores, which
cuts the map.  Everything is warmed up, then timed alternately, one pair of device events per call, at least 20 calls each; medians
with [min, max].

  pool        `ops.describe_pool(mem, inv["object_labels"], inv["object"])`: init, pool and finish launches
  classify    `ops.describe_classify(embedding, zs)` with the model's own 20 classes and with the 1203 classes of the LVIS fixture
  composed    `F.normalize(mem)` (a [N, 512] temporary), per object the cells by `nonzero` and an `index_add_` of their rows, then
              `F.normalize` of the sums and the softmax of 50 * (embedding @ zs) with the model's own classes
  bound       the rows the pooling has to read, pooled cells x 2 KB, at 6.3 TB/s from HBM (a 200 x 200 memory, 82 MB, stays in the
              Infinity Cache between calls; a 512 x 512 one, 537 MB, does not)

Also printed: how far the composed embeddings lie from the op's (largest element difference) and whether two composed calls, and two
calls of the op, agree in their bits.

    python tools/describe_bench.py [--launches 20] [--out profiles/describe_bench.txt]
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
from embodied_object_detection_amd.modeling.utils import query_classifier            # noqa: E402

GRIDS = ((200, 200, 0.2), (512, 512, 0.08))
LVIS = os.path.join(ROOT, "tests", "golden", "lvis_v1_clip.npy")
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


def composed(mem, labels, objects, zs):
    """What a user writes today: (embedding [K, 512], prob [K, C])."""
    x = F.normalize(mem, dim=1)
    sums = torch.zeros((len(objects), 512), dtype=torch.float32, device=mem.device)
    for k, obj in enumerate(objects):
        if obj < 0:
            continue
        idx = torch.nonzero(labels == obj).flatten()
        sums.index_add_(0, torch.full_like(idx, k), x[idx])
    emb = F.normalize(sums, dim=1)
    return emb, torch.softmax(50.0 * (emb @ zs[:, :-1]), dim=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "describe_bench.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("describe_bench: no GPU visible; nothing is measured without one")
    launches = max(20, args.launches)
    dev = torch.device("cuda:0")
    _lib.load()
    sd = synthetic_state_dict(0)
    lvis = query_classifier(LVIS, 1203, True, dev)
    lines = [f"describe_pool and describe_classify vs F.normalize + index_add_ per object + mm in torch: {launches} event-timed calls "
             f"each, alternating, after warm-up",
             f"device: {torch.cuda.get_device_name(0)}; the {TOPK} largest objects of model.inventory; ms as median [min, max]", ""]
    print("\n".join(lines), flush=True)
    for map_w, map_h, cell in GRIDS:
        N = map_w * map_h
        cfg = setup_cfg(None, ["MODEL.MEMORY_TYPE", "implicit_memory", "MODEL.MAP_FEAT_FUSION", "sum", "MODEL.MAP_FEATURE_WEIGHT", 5,
                               "MODEL.MEMORY_CLS_SCORE_THRESH", 0.3, "MODEL.DEVICE", "cuda:0"])
        model = build_model(cfg, sd)
        seq = SyntheticSequence(7, H=640, W=640, n_frames=3, map_w=map_w, map_h=map_h, cell=cell)
        for i in range(3):
            model([[seq.frame(i)]])
        mem, own = model.implicit_memory, model.zs_weight
        lab1, sc1 = model.semantic_map(thresh=0.0, scores=True)
        distinct = torch.unique(sc1[lab1 >= 0])
        for level in (2.0 ** -11, float(distinct[distinct.numel() // 2])):
            inv = model.inventory(thresh=0.0, map_shape=(map_w, map_h), level=level, topk=TOPK)
            labels, objects = inv["object_labels"].clone(), inv["object"].clone()
            host_objects = objects.tolist()
            pool = lambda: ops.describe_pool(mem, labels, objects)
            out = {k: v.clone() for k, v in pool().items()}
            again = pool()
            op_same = all(torch.equal(out[k].view(torch.int32) if out[k].dtype == torch.float32 else out[k],
                                      again[k].view(torch.int32) if again[k].dtype == torch.float32 else again[k]) for k in out)
            emb = out["embedding"]
            c_emb, c_prob = composed(mem, labels, host_objects, own)
            c_emb2, _ = composed(mem, labels, host_objects, own)
            prob = ops.describe_classify(emb, own)["prob"]
            pooled = int(out["cells"].sum())
            calls = {"pool": pool, "classify, 20 classes": lambda: ops.describe_classify(emb, own),
                     "classify, 1203 classes": lambda: ops.describe_classify(emb, lvis),
                     "composed": lambda: composed(mem, labels, host_objects, own)}
            t = timed(calls, launches)
            med = {k: float(np.median(v)) for k, v in t.items()}
            bound = pooled * 2048 / HBM_BYTES_PER_MS
            block = [f"{map_w} x {map_h} = {N} cells, level {level:.4g}: {int(inv['count'])} objects, foreground {int(inv['foreground'])}, "
                     f"the {int((objects >= 0).sum())} described hold {pooled} cells (largest {out['cells'][:4].tolist()}), coherence "
                     f"{[round(v, 3) for v in out['coherence'][:4].tolist()]}"]
            for k, v in t.items():
                block.append(f"  {k:23s} {med[k]:9.3f} [{v[0]:.3f}, {v[-1]:.3f}] ms")
            block.append(f"  bound of the pooling: {pooled} rows x 2 KB = {pooled * 2048 / 1e6:.1f} MB at 6.3 TB/s = {bound:.4f} ms; pool / bound = "
                         f"{med['pool'] / bound if bound else float('nan'):.1f}; composed / (pool + classify, 20 classes) = "
                         f"{med['composed'] / (med['pool'] + med['classify, 20 classes']):.1f}")
            block.append(f"  composed against the op: embedding off by at most {float((c_emb - emb).abs().max()):.3e}, prob by "
                         f"{float((c_prob - prob).abs().max()):.3e}; two composed calls agree bitwise: {bool(torch.equal(c_emb, c_emb2))}; "
                         f"two calls of the op agree bitwise: {op_same}")
            block.append("")
            print("\n".join(block), flush=True)
            lines += block
        del model
        torch.cuda.empty_cache()
    from embodied_object_detection_amd.build import resource_usage
    for name, u in sorted(resource_usage().items()):
        if "describe_" in name:
            lines.append(f"{name}: {u.get('vgprs')} VGPRs, {u.get('lds')} bytes of LDS, {u.get('occupancy')} waves per SIMD, "
                         f"{u.get('scratch')} bytes of scratch")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
