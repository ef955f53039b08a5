#!/usr/bin/env python
"""Event-timed `place` against the plain torch formulation, in one process, on the synthetic model's own detections: 640 x 640 frames
over a 200 x 200 map (40 000 cells) and 960 x 960 frames over a 512 x 512 map (262 144 cells).  Per shape the model runs three frames;
the third frame's instances are placed.  Both sides are warmed up, then timed alternately, one pair of device events per call, at least
20 calls each; medians with [min, max].

  place      `model.place(instances, proj)`: the rects from the boxes (a few torch launches) and `eod_place_masks`
  op         `ops.place_masks` alone with those rects and a caller-held workspace
  op, image  the same without rects: every mask read whole
  torch      per detection `bincount(proj[mask], minlength=n_cells)`, then `topk(4)`; no sync inside the loop

Bytes touched by the op = the rects' mask bytes + 4 bytes of proj per set pixel + the (4 + 2 T) int32 per detection it writes; the
GB/s is that over the op's median.  The torch side's top-k breaks ties its own way, so only the counts are compared.

    python tools/place_bench.py [--launches 20] [--out profiles/place_bench.txt]
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
from embodied_object_detection_amd.modeling.meta_arch import place_rects             # noqa: E402

SHAPES = ((640, 640, 200, 200, 0.2), (960, 960, 512, 512, 0.08))
TOPK = 4


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


def torch_place(masks, proj, n_cells, topk):
    """The formulation a user writes without the op: one bincount and one topk per detection."""
    counts, cells = [], []
    for k in range(masks.shape[0]):
        h = torch.bincount(proj[masks[k]], minlength=n_cells)
        v, i = torch.topk(h, topk)
        counts.append(v)
        cells.append(i)
    if not counts:
        return torch.zeros((0, topk), dtype=torch.int64, device=proj.device), torch.zeros((0, topk), dtype=torch.int64, device=proj.device)
    return torch.stack(counts), torch.stack(cells)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "place_bench.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("place_bench: no GPU visible; nothing is measured without one")
    launches = max(20, args.launches)
    dev = torch.device("cuda:0")
    _lib.load()
    sd = synthetic_state_dict(0)
    lines = [f"place vs the torch formulation (bincount + topk per detection): {launches} event-timed calls each, alternating, after warm-up",
             f"device: {torch.cuda.get_device_name(0)}; topk {TOPK}; table_log2 {ops.PLACE_TABLE_LOG2} (default); ms as median [min, max]", ""]
    print("\n".join(lines), flush=True)
    for H, W, map_w, map_h, cell in SHAPES:
        n_cells = map_w * map_h
        cfg = setup_cfg(None, ["MODEL.MEMORY_TYPE", "implicit_memory", "MODEL.MAP_FEAT_FUSION", "sum", "MODEL.MAP_FEATURE_WEIGHT", 5,
                               "MODEL.MEMORY_CLS_SCORE_THRESH", 0.3, "MODEL.DEVICE", "cuda:0"])
        model = build_model(cfg, sd)
        seq = SyntheticSequence(7, H=H, W=W, n_frames=3, map_w=map_w, map_h=map_h, cell=cell)
        frames = [seq.frame(i) for i in range(3)]
        for f in frames[:2]:
            model([[f]])
        inst = model([[frames[2]]])[0]["instances"]
        proj = model._device_proj(frames[2])
        masks = inst.pred_masks
        K = len(inst)
        ref = model.place(inst, proj, topk=TOPK)
        # the rects `place` derives, for the byte count and the bare op
        rects = place_rects(inst.pred_boxes.tensor, H, W)
        ws = torch.empty((ops.place_masks_workspace(K, n_cells),), dtype=torch.int32, device=dev)
        bare = ops.place_masks(masks, proj, n_cells, rects=rects, topk=TOPK, workspace=ws)
        assert all(torch.equal(bare[k], ref[k]) for k in ref)
        tc, _ = torch_place(masks, proj, n_cells, TOPK)
        assert torch.equal(tc.to(torch.int32), ref["cell_pixels"]), "the two formulations count differently"
        cw = rects[:, 2].clamp(max=W) - rects[:, 0].clamp(min=0)                     # the kernel's clip to the image
        ch = rects[:, 3].clamp(max=H) - rects[:, 1].clamp(min=0)
        rect_bytes = int((cw.clamp(min=0) * ch.clamp(min=0)).sum())
        set_pixels = int(ref["mask_pixels"].sum())
        out_bytes = K * (4 + 2 * TOPK) * 4
        touched = rect_bytes + 4 * set_pixels + out_bytes
        whole = K * H * W + 4 * set_pixels + out_bytes
        calls = {"place": lambda: model.place(inst, proj, topk=TOPK),
                 "op": lambda: ops.place_masks(masks, proj, n_cells, rects=rects, topk=TOPK, workspace=ws),
                 "op, image": lambda: ops.place_masks(masks, proj, n_cells, topk=TOPK, workspace=ws),
                 "torch": lambda: torch_place(masks, proj, n_cells, TOPK)}
        t = timed(calls, launches)
        med = {k: float(np.median(v)) for k, v in t.items()}
        block = [f"{H} x {W}, {n_cells} cells ({map_w} x {map_h}): {K} detections, {set_pixels} set pixels, "
                 f"distinct cells per detection max {int(ref['distinct'].max()) if K else 0}, mean {float(ref['distinct'].float().mean()) if K else 0:.1f}",
                 f"  bytes touched: rects {rect_bytes} + proj {4 * set_pixels} + out {out_bytes} = {touched / 1e6:.3f} MB "
                 f"(whole masks: {whole / 1e6:.3f} MB)"]
        for k, v in t.items():
            block.append(f"  {k:10s} {med[k]:9.3f} [{v[0]:.3f}, {v[-1]:.3f}] ms")
        block += [f"  op: {touched / (med['op'] * 1e-3) / 1e9:.1f} GB/s of its bytes; op, image: {whole / (med['op, image'] * 1e-3) / 1e9:.1f} GB/s",
                  f"  torch / place = {med['torch'] / med['place']:.1f}; torch / op = {med['torch'] / med['op']:.1f}", ""]
        print("\n".join(block), flush=True)
        lines += block
        del model, inst, masks, ws
        torch.cuda.empty_cache()
    from embodied_object_detection_amd.build import resource_usage
    for name, u in sorted(resource_usage().items()):
        if "place_" in name:
            lines.append(f"{name}: {u.get('vgprs')} VGPRs, {u.get('lds')} bytes of LDS, {u.get('occupancy')} waves per SIMD, "
                         f"{u.get('scratch')} bytes of scratch")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
