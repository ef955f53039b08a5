"""`CustomRCNNRecurrent` (eval branch) on the HIP kernels: the recurrent state machine, the memory read-prep and
the memory write.

Mirrors `Detic/detic/modeling/meta_arch/custom_rcnn.py`: `forward` eval branch (435-546), `inference` (548-582),
`create_implicit_memory` (762-774), `preprocess_spatial_memory` (1019-1042), `update_implicit_memory` (681-760),
`inference_with_proposals` (825-882), `box_to_image_features` (884-901), `project_image_features` (903-936) and
`CustomRCNN._postprocess` -> detectron2 `detector_postprocess` (579-580).

Call convention: `model(batched_inputs: List[List[dict]]) -> List[dict]`; the module is stateful
between calls.  A frame is enqueued with no host synchronisation on the current HIP stream plus three scheduling streams
(box cascade + detection selection + memory write; the coming frames' memory-independent trunk; the detection mask pass + paste,
which may trail under the next frame of a call) -- or, with `overlap_branches = False`, in order on the current stream alone.
The only sync per frame is the read-back of the final detection count when the result `Instances` are materialised.
"""
from __future__ import annotations

from typing import Dict, List, Optional, Tuple

import time as _time

import numpy as np
import torch

from .. import _lib, ops
from ..checkpoint import fill_missing, load_checkpoint, load_zs_weight, reset_cls_test, synthetic_state_dict
from ..registry import BACKBONE_REGISTRY, META_ARCH_REGISTRY, PROPOSAL_GENERATOR_REGISTRY, ROI_HEADS_REGISTRY
from ..structures import Boxes, Instances
from .utils import query_classifier


# The scheduling streams are created ONCE per device and shared by every model of the process: HIP multiplexes streams onto a
# few hardware queues, and two of a model's streams landing on the same queue would silently serialise them (measured: 127 vs
# 104 frames/s for otherwise identical runs when each model created its own).  Models of one process run from one host thread,
# so sharing the streams only adds the ordering that already exists.
_SCHED_STREAMS: Dict[int, Tuple[torch.cuda.Stream, ...]] = {}
# Result sets (post-processed detections + pasted masks, detection lists): `forward` hands frame t's Instances out after frame
# t+2 has been enqueued, so that the host never waits for a detection pass that still trails on the GPU (the host needs ~3.7 ms
# to enqueue a frame, about as long as the GPU needs to run one).
from .roi_heads import RESULT_SETS  # noqa: E402

MEMORY_NMS_THRESH = 0.5     # `inference_with_proposals`' per-class NMS (custom_rcnn.py:869)
PYRAMID_SETS = 6        # current frame, the frame before (its detection pass may trail), and up to four frames computed ahead


def _sched_streams(device: torch.device) -> Tuple[torch.cuda.Stream, ...]:
    """(side: box cascade + detection selection + memory write, look-ahead trunk, main chain): the high-priority streams.  The device
    offers two priority levels (0 and -1); the detection pass that trails under the next frame runs at 0, everything latency-bound
    at -1."""
    idx = device.index if device.index is not None else torch.cuda.current_device()
    if idx not in _SCHED_STREAMS:
        # four, not three: the fourth has no role, it stays because it decides which hardware queue every later stream lands on
        _SCHED_STREAMS[idx] = tuple(torch.cuda.Stream(device=device, priority=-1) for _ in range(4))
    return _SCHED_STREAMS[idx]


_DET_STREAMS: Dict[int, torch.cuda.Stream] = {}


def _det_stream(device: torch.device) -> torch.cuda.Stream:
    """The detection-pass stream (normal priority), also ONE per device and process.  A stream per model instance made the frame
    rate of otherwise identical models bimodal (270 or 200-220 frames/s at 640x640, tools/knob_ab.py): the runtime hands its
    hardware queues out round robin, and a later model's stream could land on the queue of one of the chain streams, which
    serialises the detection pass with that chain."""
    idx = device.index if device.index is not None else torch.cuda.current_device()
    if idx not in _DET_STREAMS:
        _DET_STREAMS[idx] = torch.cuda.Stream(device=device, priority=0)
    return _DET_STREAMS[idx]


def _query_matrix(model, mem, classifier, num_classes):
    """The class matrix a read of the memory uses (`model`: the single-scene model that holds the configuration): the
    meta-architecture's own, or `classifier` as `reset_cls_test` takes it.  Refuses a memory that no frame has filled."""
    if mem is None:
        raise _lib.EodError("semantic_map: no memory yet (no frame has run)")
    if classifier is None:
        return model.zs_weight
    return query_classifier(classifier, num_classes, bool(getattr(model.roi_heads, "norm_weight", True)), model.device)


def _semmap_query(model, mem, obs, classifier, num_classes, thresh):
    """`semantic_map` in query form on one scene's state."""
    zs = _query_matrix(model, mem, classifier, num_classes)
    return ops.semmap_query(mem, obs, zs, model.obs_score_thresh if thresh is None else float(thresh))


def _semmap_locate(model, mem, obs, classes, classifier, num_classes, thresh, map_shape, radius, topk):
    """`locate` on one scene's state.  `map_shape` (rows, cols) names the grid the cell index r * cols + c runs over; None: no grid,
    the peaks are the plain top-k."""
    zs = _query_matrix(model, mem, classifier, num_classes)
    cols = None
    if map_shape is not None:
        rows, cols = int(map_shape[0]), int(map_shape[1])
        if rows * cols != mem.shape[0]:
            raise _lib.EodError(f"locate: map_shape {tuple(map_shape)} does not hold the memory's {mem.shape[0]} cells")
    return ops.semmap_locate(mem, obs, zs, classes, model.obs_score_thresh if thresh is None else float(thresh), cols=cols,
                             radius=radius, topk=topk)


def _map_regions(model, mem, obs, classes, classifier, num_classes, thresh, map_shape, level, connectivity, min_cells, topk, radius,
                 peaks):
    """`regions` on one scene's state: `locate`, then `ops.map_regions` on its `prob`."""
    if map_shape is None:
        raise _lib.EodError("regions: map_shape (rows, cols) is required: the regions live on the grid")
    out = dict(_semmap_locate(model, mem, obs, classes, classifier, num_classes, thresh, map_shape, radius, peaks))
    reg = ops.map_regions(out["prob"], int(map_shape[1]), level, connectivity=connectivity, min_cells=min_cells, topk=topk)
    status = int(reg["status"])                                      # the results are handed over here
    if status != 0:
        raise _lib.EodError(f"regions: a bounded loop of eod_map_regions reached its bound (status {status}); the result is void")
    out.update(reg)
    return out


def _map_inventory(model, states, classifier, num_classes, thresh, map_shape, level, connectivity, min_cells, topk, exclude):
    """`inventory` on the states [(mem, obs), ...] of one scene or of several: `semantic_map(scores=True)` in query form on each,
    then one `ops.map_inventory` call on all of them ([N] maps for one state, [B, N] for a list of B)."""
    if map_shape is None:
        raise _lib.EodError("inventory: map_shape (rows, cols) is required: the objects live on the grid")
    single = not isinstance(states, list)
    states = [states] if single else states
    zs = _query_matrix(model, states[0][0], classifier, num_classes)
    rows, cols = int(map_shape[0]), int(map_shape[1])
    if rows * cols != states[0][0].shape[0]:
        raise _lib.EodError(f"inventory: map_shape {tuple(map_shape)} does not hold the memory's {states[0][0].shape[0]} cells")
    C = int(zs.shape[1]) - 1                                        # the last column is the background
    keep = None
    if exclude is not None:
        exclude = [int(c) for c in (exclude.tolist() if isinstance(exclude, torch.Tensor) else exclude)]
        bad = [c for c in exclude if not 0 <= c < C]
        if bad:
            raise _lib.EodError(f"inventory: exclude: class indices {bad} outside [0, {C - 1}]")
        table = torch.ones((C,), dtype=torch.uint8)
        table[exclude] = 0
        keep = table.to(model.device)
    th = model.obs_score_thresh if thresh is None else float(thresh)
    maps = [ops.semmap_query(mem, obs, zs, th) for mem, obs in states]
    if single:
        labels, scores = maps[0]
    else:
        labels, scores = torch.stack([m[0] for m in maps]), torch.stack([m[1] for m in maps])
    inv = ops.map_inventory(labels, scores, cols, C, level=level, connectivity=connectivity, min_cells=min_cells, topk=topk, keep=keep)
    status = int(inv["status"])                                      # the results are handed over here
    if status != 0:
        raise _lib.EodError(f"inventory: a bounded loop of eod_map_inventory reached its bound (status {status}); the result is void")
    out = {"labels": labels, "scores": scores}
    out.update(inv)
    return out


def _describe(model, mem, objects, object_labels, classifier, num_classes, topn, embedding):
    """`describe` on one scene's memory: `ops.describe_pool` (skipped with `embedding`), then `ops.describe_classify` with the
    class matrix of `_query_matrix`."""
    zs = _query_matrix(model, mem, classifier, num_classes)
    out = {}
    if embedding is None:
        if not isinstance(objects, torch.Tensor):
            objects = torch.as_tensor(objects, dtype=torch.int32, device=mem.device)
        out.update(ops.describe_pool(mem, object_labels, objects))
        embedding = out["embedding"]
    out.update(ops.describe_classify(embedding, zs, topn=topn))
    return out


def _relations(objects, object_labels, map_shape, radius, from_cell, topn):
    """`relations` on one label map: `ops.map_relations` on the grid `map_shape`.  Reads no model and no memory."""
    if map_shape is None:
        raise _lib.EodError("relations: map_shape (rows, cols) is required: the distances are those of the grid")
    rows, cols = int(map_shape[0]), int(map_shape[1])
    if not isinstance(object_labels, torch.Tensor) or object_labels.dim() != 1 or rows < 1 or cols < 1 or rows * cols != object_labels.shape[0]:
        raise _lib.EodError(f"relations: map_shape {tuple(map_shape)} does not hold the {tuple(getattr(object_labels, 'shape', ()))} "
                            "cells of object_labels")
    if not isinstance(objects, torch.Tensor):
        objects = torch.as_tensor(objects, dtype=torch.int32, device=object_labels.device)
    return ops.map_relations(object_labels, objects, cols, radius=radius, from_cell=-1 if from_cell is None else from_cell, topn=topn)


def _clearance(objects, object_labels, map_shape, radius2=0, keep_cell=None, passable=None):
    """`clearance` on one label map: `ops.map_clearance` on the grid `map_shape`.  Reads no model and no memory."""
    if map_shape is None:
        raise _lib.EodError("clearance: map_shape (rows, cols) is required: the distances are those of the grid")
    rows, cols = int(map_shape[0]), int(map_shape[1])
    if not isinstance(object_labels, torch.Tensor) or object_labels.dim() != 1 or rows < 1 or cols < 1 or rows * cols != object_labels.shape[0]:
        raise _lib.EodError(f"clearance: map_shape {tuple(map_shape)} does not hold the {tuple(getattr(object_labels, 'shape', ()))} "
                            "cells of object_labels")
    if not isinstance(objects, torch.Tensor):
        objects = torch.as_tensor(objects, dtype=torch.int32, device=object_labels.device)
    if passable is not None and not isinstance(passable, torch.Tensor):
        passable = torch.as_tensor(passable, dtype=torch.int32, device=object_labels.device).reshape(-1)
    res = ops.map_clearance(object_labels, objects, cols, radius2=radius2, keep_cell=-1 if keep_cell is None else keep_cell,
                            passable=passable)
    status = int(res["status"][0])                                   # the results are handed over here
    if status & 2:
        raise _lib.EodError(f"clearance: a bounded loop of eod_map_clearance reached its bound (status {status}); the result is void")
    return res


def _sight(objects, object_labels, map_shape, from_cells, range2=None, passable=None):
    """`sight` on one label map: `ops.map_sight` on the grid `map_shape`.  Reads no model and no memory."""
    if map_shape is None:
        raise _lib.EodError("sight: map_shape (rows, cols) is required: the lines are those of the grid")
    rows, cols = int(map_shape[0]), int(map_shape[1])
    if not isinstance(object_labels, torch.Tensor) or object_labels.dim() != 1 or rows < 1 or cols < 1 or rows * cols != object_labels.shape[0]:
        raise _lib.EodError(f"sight: map_shape {tuple(map_shape)} does not hold the {tuple(getattr(object_labels, 'shape', ()))} "
                            "cells of object_labels")
    if from_cells is None:
        raise _lib.EodError("sight: from_cells is required: the cells to look from (RobotFrontEnd.exclude_cell(pose), "
                            "clearance's widest_cell, route's goal_cell)")
    if not isinstance(objects, torch.Tensor):
        objects = torch.as_tensor(objects, dtype=torch.int32, device=object_labels.device)
    if passable is not None and not isinstance(passable, torch.Tensor):
        passable = torch.as_tensor(passable, dtype=torch.int32, device=object_labels.device).reshape(-1)
    res = ops.map_sight(object_labels, objects, cols, from_cells, range2=range2, passable=passable)
    status = int(res["status"][0])                                   # the results are handed over here
    if status & 2:
        raise _lib.EodError(f"sight: a bounded loop of eod_map_sight reached its bound (status {status}); the result is void")
    return res


def _cover(model, proj_indices, last_seen, n_cells, stamp, exclude_cell):
    """`cover` on one scene: `ops.map_cover` into `last_seen` (None: a new int32 [n_cells] of -1).  Returns the buffer."""
    proj = model._device_proj({"proj_indices": proj_indices})
    if last_seen is None:
        last_seen = torch.full((int(n_cells),), -1, dtype=torch.int32, device=proj.device)
    return ops.map_cover(proj, last_seen, stamp, exclude_cell)


def _frontiers(object_labels, map_shape, last_seen, since=0, from_cell=None, route=None, passable=None, min_cells=2, topk=16,
               rank_by="behind"):
    """`frontiers` on one label map: `ops.map_frontier` on the grid `map_shape`.  Reads no model and no memory."""
    if map_shape is None:
        raise _lib.EodError("frontiers: map_shape (rows, cols) is required: the neighbours are those of the grid")
    rows, cols = int(map_shape[0]), int(map_shape[1])
    if not isinstance(object_labels, torch.Tensor) or object_labels.dim() != 1 or rows < 1 or cols < 1 or rows * cols != object_labels.shape[0]:
        raise _lib.EodError(f"frontiers: map_shape {tuple(map_shape)} does not hold the {tuple(getattr(object_labels, 'shape', ()))} "
                            "cells of object_labels")
    if not object_labels.is_cuda:
        raise _lib.EodError("frontiers: object_labels on the host (no CPU fallback)")
    if last_seen is None:
        raise _lib.EodError("frontiers: no record of what was covered: call cover(proj_indices) on every frame, or pass last_seen")
    dist = None
    if route is not None:
        dist = route["dist"] if isinstance(route, dict) else route
    res = ops.map_frontier(object_labels, last_seen, cols, since=since, dist=dist, from_cell=-1 if from_cell is None else from_cell,
                           passable=passable, min_cells=min_cells, topk=topk, rank_by=rank_by)
    status = int(res["status"][0])                                   # the results are handed over here
    if status != 0:
        raise _lib.EodError(f"frontiers: a bounded loop of eod_map_frontier reached its bound (status {status}); the result is void")
    return res


def _device_heights(heights, device):
    """The heights of a frame's pixels (numpy or tensor; [H, W], [H, W, 1] or xyz [H, W, 3]) as contiguous float32 on the device."""
    h = heights
    if not torch.is_tensor(h):
        h = torch.from_numpy(np.ascontiguousarray(h))
    if h.dim() == 3 and h.shape[2] == 1:
        h = h.squeeze(2)
    if h.dtype != torch.float32:
        h = h.to(torch.float32)
    return h.to(device, non_blocking=True).contiguous()


def _heights(model, proj_indices, heights, record, n_cells, band_mm, exclude_cell):
    """`heights` on one scene: `ops.map_heights` into `record` (None: a new one of `ops.new_height_record`).  Returns the record."""
    if heights is None:
        raise _lib.EodError("heights: the frame carries no heights (RobotFrontEnd.frame(..., heights=True), or the xyz of "
                            "ops.unproject_grid_index(..., want_xyz=True))")
    proj = model._device_proj({"proj_indices": proj_indices})
    if record is None:
        record = ops.new_height_record(int(n_cells), proj.device)
    return ops.map_heights(proj, _device_heights(heights, proj.device), record, band_mm=band_mm, exclude_cell=exclude_cell)


def _obstacles(record, map_shape, object_labels=None, objects=None, min_hits=4, min_cells=2, topk=16):
    """`obstacles` on one record: `ops.map_obstacles` on the grid `map_shape`.  Reads no model and no memory."""
    if map_shape is None:
        raise _lib.EodError("obstacles: map_shape (rows, cols) is required: the neighbours are those of the grid")
    if record is None:
        raise _lib.EodError("obstacles: no height record: call heights(proj_indices, heights) on every frame, or pass record")
    rows, cols = int(map_shape[0]), int(map_shape[1])
    if not isinstance(record, torch.Tensor) or record.dim() != 2 or rows < 1 or cols < 1 or rows * cols != record.shape[1]:
        raise _lib.EodError(f"obstacles: map_shape {tuple(map_shape)} does not hold the cells of the record "
                            f"{tuple(getattr(record, 'shape', ()))}")
    if not record.is_cuda:
        raise _lib.EodError("obstacles: record on the host (no CPU fallback)")
    res = ops.map_obstacles(record, cols, object_labels=object_labels, objects=objects, min_hits=min_hits, min_cells=min_cells,
                            topk=topk)
    status = int(res["status"][0])                                   # the results are handed over here
    if status != 0:
        raise _lib.EodError(f"obstacles: a bounded loop of eod_map_obstacles reached its bound (status {status}); the result is void")
    return res


def _rooms(labels, objects, map_shape, door_r2, min_cells, topk=16, passable=None, known=None, clearance=None, sweeps=None):
    """`rooms` on one label map: `ops.map_rooms` on the grid `map_shape`, after `ops.map_clearance` unless `clearance` brings its
    `d2`; run again with twice the sweeps while they run out.  Reads no model and no memory."""
    if map_shape is None:
        raise _lib.EodError("rooms: map_shape (rows, cols) is required: the neighbours are those of the grid")
    rows, cols = int(map_shape[0]), int(map_shape[1])
    if not isinstance(labels, torch.Tensor) or labels.dim() != 1 or rows < 1 or cols < 1 or rows * cols != labels.shape[0]:
        raise _lib.EodError(f"rooms: map_shape {tuple(map_shape)} does not hold the {tuple(getattr(labels, 'shape', ()))} cells of labels")
    if door_r2 is None or min_cells is None:
        raise _lib.EodError("rooms: door_r2 and min_cells are required: the squared half-width in cells of the widest gap that still "
                            "counts as a doorway (RobotFrontEnd.door_r2) and the fewest core cells of a room")
    if not labels.is_cuda:
        raise _lib.EodError("rooms: labels on the host (no CPU fallback)")
    if objects is not None and not isinstance(objects, torch.Tensor):
        objects = torch.as_tensor(objects, dtype=torch.int32, device=labels.device).reshape(-1)
    if passable is not None and not isinstance(passable, torch.Tensor):
        passable = torch.as_tensor(passable, dtype=torch.int32, device=labels.device).reshape(-1)
    if clearance is None:
        slots = objects if objects is not None and objects.numel() > 0 else torch.full((1,), -1, dtype=torch.int32, device=labels.device)
        clearance = _clearance(slots, labels, map_shape, 0, None, passable)
    d2 = clearance["d2"] if isinstance(clearance, dict) else clearance
    n = ops.map_route_sweeps(rows, cols) if sweeps is None else int(sweeps)
    for _ in range(ops.ROUTE_RESUMES + 1):
        res = ops.map_rooms(labels, d2, cols, door_r2, min_cells=min_cells, topk=topk, objects=objects, passable=passable, known=known,
                            sweeps=n)
        status = int(res["status"][0])                               # the results are handed over here
        if status != 1 or n >= ops.ROOMS_SWEEPS_MAX:
            break
        n = min(2 * n, ops.ROOMS_SWEEPS_MAX)
    if status & 2:
        raise _lib.EodError(f"rooms: a bounded loop of eod_map_rooms reached its bound (status {status}); the result is void")
    if status != 0:
        raise _lib.EodError(f"rooms: the keys had not settled after {n} sweeps (status {status}); the result is void")
    res = dict(res)
    res["clearance_d2"] = d2
    return res


def _rooms_batched(what, labels, objects, map_shape, door_r2, min_cells, topk, passable, known, clearance, sweeps):
    """The `[B, N]` form of `rooms` of the lock-step batch: one call per scene, every entry gaining a leading [B]."""
    B = int(labels.shape[0])
    if objects is not None:
        objects = torch.as_tensor(objects, dtype=torch.int32, device=labels.device)
        if objects.dim() != 2 or objects.shape[0] != B:
            raise _lib.EodError(f"{what}: objects {tuple(objects.shape)}: expected [B, K] beside labels {tuple(labels.shape)}")
    if known is not None and (not isinstance(known, torch.Tensor) or known.dim() != 2 or known.shape[0] != B):
        raise _lib.EodError(f"{what}: known {tuple(getattr(known, 'shape', ()))}: expected [B, N] beside labels {tuple(labels.shape)}")
    d2 = clearance["d2"] if isinstance(clearance, dict) else clearance
    if d2 is not None and (not isinstance(d2, torch.Tensor) or d2.dim() != 2 or d2.shape[0] != B):
        raise _lib.EodError(f"{what}: clearance {tuple(getattr(d2, 'shape', ()))}: expected d2 [B, N] beside labels {tuple(labels.shape)}")
    per = [_rooms(labels[b].contiguous(), None if objects is None else objects[b].contiguous(), map_shape, door_r2, min_cells, topk,
                  passable, None if known is None else known[b].contiguous(), None if d2 is None else d2[b].contiguous(), sweeps)
           for b in range(B)]
    return {k: torch.stack([p[k] for p in per]) for k in per[0]}


def _observed(observations):
    """The weaker record where `cover` never ran: 0 where the memory was written, -1 elsewhere."""
    return torch.where(observations > 0, 0, -1).to(torch.int32)


def _route(objects, object_labels, map_shape, from_cell, passable=None, path_max=256, sweeps=None, body_radius2=None):
    """`route` on one label map: `ops.map_route` on the grid `map_shape`, resumed while the sweeps run out (each resumed call with
    twice the sweeps of the last, `ops.ROUTE_RESUMES` of them at the most).  With `body_radius2` the route runs on the `inflated`
    labels of `_clearance(radius2=body_radius2, keep_cell=from_cell)`.  Reads no model and no memory."""
    if body_radius2 is not None:
        if from_cell is None:
            raise _lib.EodError("route: from_cell is required: the cell the paths start from (RobotFrontEnd.exclude_cell(pose))")
        clr = _clearance(objects, object_labels, map_shape, body_radius2, from_cell, passable)
        res = dict(_route(objects, clr["inflated"], map_shape, from_cell, passable, path_max, sweeps))
        res["clearance_d2"] = clr["d2"]
        res["inflated_labels"] = clr["inflated"]
        return res
    if map_shape is None:
        raise _lib.EodError("route: map_shape (rows, cols) is required: the moves are those of the grid")
    rows, cols = int(map_shape[0]), int(map_shape[1])
    if not isinstance(object_labels, torch.Tensor) or object_labels.dim() != 1 or rows < 1 or cols < 1 or rows * cols != object_labels.shape[0]:
        raise _lib.EodError(f"route: map_shape {tuple(map_shape)} does not hold the {tuple(getattr(object_labels, 'shape', ()))} "
                            "cells of object_labels")
    if from_cell is None:
        raise _lib.EodError("route: from_cell is required: the cell the paths start from (RobotFrontEnd.exclude_cell(pose))")
    if not isinstance(objects, torch.Tensor):
        objects = torch.as_tensor(objects, dtype=torch.int32, device=object_labels.device)
    if passable is not None and not isinstance(passable, torch.Tensor):
        passable = torch.as_tensor(passable, dtype=torch.int32, device=object_labels.device).reshape(-1)
    res = ops.map_route(object_labels, objects, cols, from_cell, passable=passable, path_max=path_max, sweeps=sweeps)
    n = ops.map_route_sweeps(rows, cols) if sweeps is None else int(sweeps)
    total = n
    for _ in range(ops.ROUTE_RESUMES):
        status = int(res["status"][0])                               # the results are handed over here
        if status != 1:
            break
        n = min(2 * n, ops.ROUTE_SWEEPS_MAX)
        total += n
        res = ops.map_route(object_labels, objects, cols, from_cell, passable=passable, path_max=path_max, sweeps=n, resume=res)
    status = int(res["status"][0])
    if status & 2:
        raise _lib.EodError(f"route: a bounded loop of eod_map_route reached its bound (status {status}); the result is void")
    if status != 0:
        raise _lib.EodError(f"route: the distances had not settled after {total} sweeps in {ops.ROUTE_RESUMES + 1} calls (status "
                            f"{status}); the result is void")
    return res


def place_rects(boxes: torch.Tensor, H: int, W: int) -> torch.Tensor:
    """int32 [K, 4] half-open rects outside which the pasted masks of `boxes` (float [K, 4], x0 y0 x1 y1) are zero: the box grown
    by (w / 14 + 1, h / 14 + 1) pixels, floor and ceil.  A pasted mask is exactly zero more than one mask pixel (box side / 28)
    outside its box (`mw_cover_kernel`'s quick reject, csrc/memory.hip).  The values are only kept near the image here; the
    kernel clips each rect to it."""
    b = boxes.to(torch.float32)
    m = (b[:, 2:] - b[:, :2]) / 14.0 + 1.0
    r = torch.cat([torch.floor(b[:, :2] - m), torch.ceil(b[:, 2:] + m)], dim=1)
    return r.clamp_(-1.0, float(max(H, W) + 1)).to(torch.int32)


def _place(model, mem, instances, proj_indices, topk, exclude_cell, attach):
    """`place` against one scene's cell count (`mem`: that scene's memory)."""
    if mem is None:
        raise _lib.EodError("place: no memory yet (no frame has run)")
    proj = model._device_proj({"proj_indices": proj_indices})
    masks = instances.pred_masks
    if not masks.is_contiguous():
        masks = masks.contiguous()
    rects = place_rects(instances.pred_boxes.tensor, int(masks.shape[1]), int(masks.shape[2]))
    out = ops.place_masks(masks, proj, int(mem.shape[0]), rects=rects, topk=topk, exclude_cell=exclude_cell)
    if attach:
        instances.pred_cells = out["cells"][:, 0]
        instances.pred_cell_pixels = out["cell_pixels"][:, 0]
    return out


def _result_sets(B: int, D: int, hw: Tuple[int, int], dev) -> List[dict]:
    """RESULT_SETS result sets of B scenes with up to D detections each.  boxes / scores / classes / masks of a set are allocated anew
    for every frame (`roi_heads.postprocess_and_paste`) and handed to the caller as they are: no copy of the 0/1 byte masks
    ([300,H,W]: 123 MB at 640x640) when the Instances are built."""
    return [dict(hw=hw, boxes=None, scores=None, classes=None, masks=None,
                 src=torch.zeros((B * D,), dtype=torch.int32, device=dev), count=torch.zeros((B,), dtype=torch.int32, device=dev),
                 count_host=torch.zeros((B,), dtype=torch.int32).pin_memory(), err_host=torch.zeros((1,), dtype=torch.int32).pin_memory(),
                 ready=torch.cuda.Event(), err_ready=torch.cuda.Event()) for _ in range(RESULT_SETS)]


def _ticket(P: dict, err: torch.Tensor, cur: torch.cuda.Stream, det_stream: Optional[torch.cuda.Stream], after=None) -> dict:
    """Async read-back of result set P's detection counts (and the device error word) into pinned host memory + an event.
    `det_stream`: the detection pass of this frame may still be running there: the counts are copied on that stream (behind the
    event `after`, if given) and the ticket's event covers both streams.  None: everything ran on `cur`."""
    P["err_host"].copy_(err, non_blocking=True)
    if det_stream is not None:
        if after is not None:
            det_stream.wait_event(after)
        P["err_ready"].record(cur)
        det_stream.wait_event(P["err_ready"])
        with torch.cuda.stream(det_stream):
            P["count_host"].copy_(P["count"], non_blocking=True)
            P["ready"].record(det_stream)
    else:
        P["count_host"].copy_(P["count"], non_blocking=True)
        P["ready"].record(cur)
    return P


def _instances(P: dict, err: torch.Tensor, host_profile: dict, n_cells: int, device, active=None) -> List[Optional[Instances]]:
    """Slice a result set by its scenes' detection counts (the frame's only host wait: on the event recorded after the counts'
    async copy) -> one `Instances` per scene, None for a scene that is not `active`.  The paste kernel writes 0/1 bytes, so the
    masks are handed out as a bool view."""
    t0 = _time.perf_counter()
    P["ready"].synchronize()
    host_profile["wait_s"] += _time.perf_counter() - t0
    flags = int(P["err_host"][0])
    if flags:
        err.zero_()
        raise _lib.EodError(
            f"device error flags {flags:#x}: proj_indices holds cell indices outside [0, {n_cells}) "
            "(an index image written for another map size?); they were clamped, the frame's results are not trustworthy")
    cur = torch.cuda.current_stream(device)
    for k in ("boxes", "scores", "classes", "masks"):
        P[k].record_stream(cur)           # allocated on the stream that filled them; the caller reads them on this one
    B = P["count_host"].shape[0]
    D = P["src"].shape[0] // B
    out = []
    for b in range(B):
        if active is not None and not active[b]:
            out.append(None)
            continue
        n = int(P["count_host"][b])
        inst = Instances(P["hw"])
        inst.pred_boxes = Boxes(P["boxes"][b * D:b * D + n])
        inst.scores = P["scores"][b * D:b * D + n]
        inst.pred_classes = P["classes"][b * D:b * D + n].to(torch.int64)
        inst.pred_masks = P["masks"][b, :n].view(torch.bool)       # the paste kernel writes 0/1 bytes: a view, no copy
        out.append(inst)
    P["boxes"] = P["scores"] = P["classes"] = P["masks"] = None
    return out


@META_ARCH_REGISTRY.register()
class CustomRCNNRecurrent:
    def __init__(self, cfg, state_dict: Optional[Dict[str, torch.Tensor]] = None):
        dev = str(cfg.MODEL.DEVICE)
        if not dev.startswith("cuda"):
            raise _lib.EodError(
                f"MODEL.DEVICE={dev!r}: the product path is HIP-only (no CPU fallback). The CPU restatement lives in "
                "oracle/ and is test infrastructure.")
        if not torch.cuda.is_available():
            raise _lib.EodError("no GPU visible: the HIP product path cannot run")
        _lib.load()
        self.cfg = cfg
        self.device = torch.device(dev if ":" in dev else "cuda:0")
        torch.cuda.set_device(self.device)
        self.map_conditioned = cfg.MODEL.TIMM.BASE_NAME == "resnet50_in21k_map"
        self.memory_type = cfg.MODEL.MEMORY_TYPE
        self.save_semmap = bool(cfg.MODEL.TEST_SAVE_SEMMAP)
        self.output_dir = cfg.OUTPUT_DIR
        self.cls_score_thresh = float(cfg.MODEL.MEMORY_CLS_SCORE_THRESH)
        self.obs_score_thresh = float(cfg.MODEL.MEMORY_OBS_SCORE_THRESH)
        self.test_type = cfg.MODEL.TEST_TYPE
        if self.test_type not in ("default", "episodic", "longterm"):
            raise ValueError(f"MODEL.TEST_TYPE={self.test_type!r}")
        self.pixel_mean = [float(v) for v in cfg.MODEL.PIXEL_MEAN]
        self.pixel_std = [float(v) for v in cfg.MODEL.PIXEL_STD]
        self.mask_threshold = 0.5
        self.training = False
        # Default: compute the proposal masks only for the proposals the memory update reads (<= 100 unique rows kept by
        # `inference_with_proposals`, custom_rcnn.py:875-880).  The reference runs the mask head on all 256 proposals
        # (custom_rcnn.py:573) and never reads the others; they are not observable through the boundary and every output is
        # bitwise identical (tests/test_model_gpu.py::test_lazy_proposal_masks_give_identical_results).  `False` restores the
        # reference-faithful 256-proposal pass (bench.py reports it beside the headline).
        self.lazy_proposal_masks = True
        # Detections that come from one proposal carry the SAME class-agnostic box (fast_rcnn_inference keeps up to 20 classes of a
        # proposal as separate detections, detic_roi_heads.py:214-221) and the mask head is class agnostic (CLS_AGNOSTIC_MASK): their
        # masks are identical.  Default: the mask head runs once per distinct box (~100 of 300 detections on the benchmark scene)
        # and every detection of the group reads that mask; outputs are bitwise those of the 300-ROI pass
        # (tests/test_model_gpu.py::test_detection_mask_groups_give_identical_results).  `False` restores the reference-faithful
        # one-ROI-per-detection pass (bench.py reports it beside the headline).
        self.dedup_detection_masks = True
        # The frame has two schedules.  `overlap_branches = False`: every launch in order on the current stream (`_frame_in_order`).
        # True (`_frame_pipelined`): the proposal mask pass (custom_rcnn.py:573) needs the FPN features, the proposals and -- lazily --
        # the memory selection, which reads what cascade stage 0 leaves and nothing of stages 1-2: the cascade's small latency-bound
        # launches (15 FC GEMMs, 3 ROIAligns, the detection selection) and the memory write-back go to a second, high-priority
        # stream, and behind stage 0 the main stream runs the memory selection and the pass's large GEMMs beside stages 1-2; and
        # nothing of frame t+1 depends on frame t's DETECTION masks (the memory write needs the proposal masks only), so the
        # detection mask pass + post-processing + paste run on a normal-priority stream of their own, inside
        # `forward([episode])` underneath frame t+1's memory read, tower, proposal decoding and box cascade (short chains that
        # leave most of the chip idle).  PYRAMID_SETS pyramid sets and RESULT_SETS detection-list sets make the overlap hazard
        # free.  Same kernels, same inputs, bitwise the same results.
        self.overlap_branches = True
        self._side_stream = None
        self._ev_props = self._ev_pm = self._ev_box = self._ev_mem = self._ev_s0 = None
        # Look-ahead: the ResNet trunk does not read the memory, so the NEXT frames' bottom-up pass and FPN top-down convs (known from
        # the inner frame list of `forward`, or passed as `next_frame`) are enqueued on a third stream from the start of this frame
        # on; they write pyramid sets of their own.
        self.prefetch_trunk = True
        self._ev_start = None
        self._trunk_stream = None
        self._ev_trunk = None
        self._prefetched = None      # (image object of the frame, padded H, W)
        self._pyramid = 0            # which of the PYRAMID_SETS FPN buffer sets the current frame uses
        # how many coming frames of an episode the look-ahead computes at once (their images are all there when `forward` is
        # called): 2 = the memory-independent trunk + FPN top-down of frames t+1 and t+2 as ONE N = 2 pass every second frame
        # (planned like one image: bitwise the N = 1 results).  Measured at 640x640: the pass costs 1.23 ms per image instead of 1.61
        # (tools/trunk_batch_time.py).  With a window of the same size (round 3) the frames WITH the double trunk lost what the
        # others gained; inside a deeper window (`lookahead_depth`) the N = 2 pass has two frame periods to finish: default 2.
        self.lookahead_frames = 2
        # how many coming frames may be AHEAD at any time (>= lookahead_frames; PYRAMID_SETS - 2 at most).  With depth == batch size
        # a pass starts when the last frame computed ahead has been consumed and must be over one frame later -- the trunk's ~75
        # launches then span the whole frame (profiles/r03_frame_schedule.txt: 0.24 -> 3.60 ms of a 3.5 ms frame) and the next frame
        # waits for them: the look-ahead is a second critical chain.  A deeper window decouples it: a pass is started while frames
        # are still ahead and has several frame periods to finish (only its throughput matters, and N = 2 passes cost 24 % less per
        # image).  None = lookahead_frames (the round-3 schedule).  Measured at 640x640 (tools/knob_ab.py, one call): batch 1 /
        # window 1 287 frames/s, 1 / 2 287, 2 / 3 301, 2 / 4 300, 3 / 5 297, 4 / 6 295 (the last two with eight pyramid sets).
        self.lookahead_depth: Optional[int] = 3
        self._ahead: List[dict] = []        # frames computed (or being computed) ahead, in order: image, Hp, Wp, event
        self.front_event: Optional[torch.cuda.Event] = None      # one-stream schedule only: recorded after the box cascade
        # where the (deferred, low-priority) detection mask pass may start: "cascade" (as soon as the detections exist),
        # "proposal_masks" / "memory_write" (behind this frame's critical chain: it then runs beside the NEXT frame's
        # latency-bound front instead of beside this frame's proposal masks and memory write)
        self.detection_pass_after = "cascade"
        self._det_stream = None
        self._ev_call = None
        self._ev_det = [None] * RESULT_SETS   # per result set: detection pass + paste finished
        self._pyr_reader = {}                # pyramid set -> event of the last detection pass that read it
        self._frame_no = 0

        num_classes = int(cfg.MODEL.ROI_HEADS.NUM_CLASSES)
        if state_dict is None:
            if cfg.MODEL.WEIGHTS and str(cfg.MODEL.WEIGHTS).endswith((".pth", ".pkl")) and __import__("os").path.exists(cfg.MODEL.WEIGHTS):
                sd, _ = load_checkpoint(cfg.MODEL.WEIGHTS, num_classes)
                state_dict = fill_missing(sd, 0, num_classes, cfg.MODEL.ROI_BOX_HEAD.ZEROSHOT_WEIGHT_PATH)
            else:
                state_dict = synthetic_state_dict(0, num_classes, cfg.MODEL.ROI_BOX_HEAD.ZEROSHOT_WEIGHT_PATH)
        if cfg.MODEL.RESET_CLS_TESTS and cfg.MODEL.TEST_CLASSIFIERS:
            import os
            p = cfg.MODEL.TEST_CLASSIFIERS[0]
            if not os.path.exists(p):
                p = cfg.MODEL.ROI_BOX_HEAD.ZEROSHOT_WEIGHT_PATH
            state_dict = dict(state_dict)
            reset_cls_test(state_dict, p, int(cfg.MODEL.TEST_NUM_CLASSES[0]))          # utils.py:32-50
        self.state_dict_ref = state_dict
        # zs_weight of the meta-arch itself (custom_rcnn.py:375-382)
        self.zs_weight = load_zs_weight(cfg.MODEL.ROI_BOX_HEAD.ZEROSHOT_WEIGHT_PATH).contiguous().to(self.device)
        self.C1 = self.zs_weight.shape[1]

        self.backbone = BACKBONE_REGISTRY.get(cfg.MODEL.BACKBONE.NAME)(cfg, state_dict, self.device)
        self.proposal_generator = PROPOSAL_GENERATOR_REGISTRY.get(cfg.MODEL.PROPOSAL_GENERATOR.NAME)(cfg, state_dict, self.device)
        self.roi_heads = ROI_HEADS_REGISTRY.get(cfg.MODEL.ROI_HEADS.NAME)(cfg, state_dict, self.device, self.proposal_generator.cap)
        R = self.proposal_generator.cap
        self.mem_scores = torch.zeros((R, self.C1), dtype=torch.float32, device=self.device)
        # inference_with_proposals' selection (custom_rcnn.py:862-875) in one launch: threshold, per-class NMS, top 100, unique rows
        self.mem_selector = ops.DetectionSelector(R, self.C1, 100, self.device, unique=True)
        self._uniq_rows, self._uniq_count = self.mem_selector.uniq_rows, self.mem_selector.uniq_count
        self._mem_scores_frame = -1      # frame whose CLIP re-score `mem_scores` holds (written by stage 0 of the cascade)
        # recurrent state
        self.implicit_memory: Optional[torch.Tensor] = None   # [N,512] f32  (== semmap_features)
        self.observations: Optional[torch.Tensor] = None      # [N] f32      (== observation_count)
        self.semmap = None
        self._last_seen: Optional[torch.Tensor] = None        # [N] int32: the stamp of the last `cover` of each cell, -1: none
        self._cover_stamp = 0
        self._height_record: Optional[torch.Tensor] = None    # [4,N] int32: hits, band_hits, h_min_mm, h_max_mm of `heights`
        self._mem_f16: Optional[torch.Tensor] = None
        self._dirty: Optional[torch.Tensor] = None          # int32 [N]: rows of the fp16 snapshot that are out of date
        self._f16_valid = False
        self._dirty_pending = False          # some write marked rows in `_dirty` that the snapshot does not have yet
        # TEST_TYPE default / episodic read the memory as it stands at every frame (loader.py:289-293): the write refreshes the
        # snapshot rows it invalidates itself (ops.MemoryWriter `snapshot`), no normalise launch at the start of the next frame.
        # `longterm` freezes the snapshot after the first frame: there the write only marks the rows.
        self.snapshot_follows_write: Optional[bool] = None      # None: decided by TEST_TYPE at every write
        self._err = torch.zeros((1,), dtype=torch.int32, device=self.device)   # device error word (EOD_FLAG_*), read with the count
        self._writer = None
        self._writer_key = None
        self._post = None
        self._posts = None
        self._post_slot = 0
        self.last_stats: Dict[str, torch.Tensor] = {}
        self.stats_log = None
        self.trace = None
        self.host_profile = {"frames": 0, "enqueue_s": 0.0, "materialize_s": 0.0, "wait_s": 0.0}   # host seconds spent in forward()

    # detectron2 nn.Module surface used by the drivers
    def eval(self):
        self.training = False
        return self

    def train(self, mode: bool = True):
        """Training mode: `forward` runs `forward_model` on every frame through the attached `modeling.training.Trainer`."""
        self.training = bool(mode)
        return self

    def to(self, *_a, **_k):
        return self

    def __call__(self, batched_inputs):
        return self.forward(batched_inputs)

    # ---- state ----------------------------------------------------------------------------------------
    def reset_memory(self, n_cells: int):
        """`frame['memory_reset']` branch (custom_rcnn.py:470-479)."""
        if self.implicit_memory is None or self.implicit_memory.shape[0] != n_cells:
            self.implicit_memory = torch.empty((n_cells, 512), dtype=torch.float32, device=self.device)
            self.observations = torch.empty((n_cells,), dtype=torch.float32, device=self.device)
            self._mem_f16 = torch.empty((n_cells, 512), dtype=torch.float16, device=self.device)
            self._dirty = torch.empty((n_cells,), dtype=torch.int32, device=self.device)
        lib = _lib.load()
        s = torch.cuda.current_stream().cuda_stream
        _lib.check(lib.eod_fill_f32(self.implicit_memory.data_ptr(), 0.0, self.implicit_memory.numel(), s), "fill")
        _lib.check(lib.eod_fill_f32(self.observations.data_ptr(), 0.0, self.observations.numel(), s), "fill")
        # the resident fp16 snapshot of an all-zero memory is all zero; from here on it is kept incrementally (dirty rows only)
        _lib.check(lib.eod_fill_i32(self._mem_f16.data_ptr(), 0, self._mem_f16.numel() // 2, s), "fill")
        _lib.check(lib.eod_fill_i32(self._dirty.data_ptr(), 0, n_cells, s), "fill")
        self._f16_valid = True
        self._dirty_pending = False
        self.semmap = None
        self._last_seen = None
        self._height_record = None

    def invalidate_memory_snapshot(self):
        """Call after writing `implicit_memory` / `observations` from outside (e.g. a loaded snapshot): the next frame
        re-normalises the whole table instead of the dirty rows."""
        self._f16_valid = False

    def _refresh_memory_snapshot(self):
        """a4 + fp16 cast (create_implicit_memory + preprocess_spatial_memory): bring the resident fp16 table up to the state."""
        if self._f16_valid:
            if self._dirty_pending:
                ops.memory_normalize_dirty_f16(self.implicit_memory, self.observations, self._dirty, self._mem_f16)
        else:
            ops.memory_normalize_f16(self.implicit_memory, self.observations, out=self._mem_f16)
            _lib.check(_lib.load().eod_fill_i32(self._dirty.data_ptr(), 0, self._dirty.numel(), torch.cuda.current_stream().cuda_stream), "fill")
            self._f16_valid = True
        self._dirty_pending = False

    def _ensure_frame_buffers(self, H: int, W: int, n_cells: int):
        key = (H, W, n_cells)
        if self._writer_key != key:
            self._writer = ops.MemoryWriter(H, W, n_cells, 100, self.proposal_generator.cap, self.device, mask_thresh=0.5)
            self._writer_key = key
        if self._posts is None or self._posts[0]["hw"] != (H, W):
            # RESULT_SETS result sets: frame t's `Instances` are sliced out of set t % 3 only after frame t+2 has been enqueued
            # (`forward`), so the host's read-back of the detection count never leaves the GPU idle
            self._posts = _result_sets(1, self.roi_heads.topk, (H, W), self.device)
            self._post_slot = 0
        self._post = self._posts[self._post_slot]

    # ---- forward ----------------------------------------------------------------------------------------
    def forward(self, batched_inputs: List[List[dict]]):
        """Sequential pass over sequences and frames; the memory persists across calls (custom_rcnn.py:435-546)."""
        if self.training:
            # custom_rcnn.py:444-461: forward_model per frame, the loss terms summed.  There is no autograd graph on this path: the
            # attached `modeling.training.Trainer` runs forward AND backward and keeps the gradients for its `optimizer_step()`.
            if getattr(self, "trainer", None) is None:
                raise RuntimeError("training mode needs a trainer: `modeling.training.Trainer(model, state_dict)` attaches itself to the "
                                   "model; then `model.train(); losses = model(data); trainer.optimizer_step()`")
            return self.trainer.forward_backward_frames(batched_inputs)
        if self.overlap_branches:
            # The frame's own chain (memory read -> tower -> proposals -> proposal masks -> memory write) moves to a HIGH priority
            # stream for the duration of the call: the previous frame's detection pass trails at normal priority, and at equal
            # priority the short chain would queue behind the GEMMs' thousands of workgroups.  The caller's stream is joined on
            # both sides, so the call keeps its in-order meaning.
            caller = torch.cuda.current_stream(self.device)
            ms = _sched_streams(self.device)[2]
            if self._ev_call is None:
                self._ev_call = (torch.cuda.Event(), torch.cuda.Event())
            self._ev_call[0].record(caller)
            ms.wait_event(self._ev_call[0])
            with torch.cuda.stream(ms):
                out = self._forward_frames(batched_inputs)
                self._ev_call[1].record(ms)
            caller.wait_event(self._ev_call[1])
            return out
        return self._forward_frames(batched_inputs)

    def _forward_frames(self, batched_inputs: List[List[dict]]):
        batch_output = []
        pending = []              # tickets of the last frames: Instances are built RESULT_SETS - 1 frames behind the enqueue
        for input_seq in batched_inputs:
            for i, frame in enumerate(input_seq):
                n_cells = int(input_seq[0]["memory"].shape[0])
                if frame["memory_reset"]:
                    self.reset_memory(n_cells)
                if self.implicit_memory is None:
                    raise RuntimeError("first frame of a scene must carry memory_reset=True (custom_rcnn.py:485 reads unset state)")
                refresh = self.test_type in ("default", "episodic") or (self.test_type == "longterm" and i == 0)
                nxt = input_seq[i + 1:i + 1 + PYRAMID_SETS] or None                            # the frames that follow, in order
                last = nxt is None and input_seq is batched_inputs[-1]
                t0 = _time.perf_counter()
                self.inference_frame(frame, refresh_memory_snapshot=refresh, materialize=False, next_frame=nxt,
                                     trailing_detection_pass=not last)
                pending.append(self._post_ticket())
                t1 = _time.perf_counter()
                if len(pending) == RESULT_SETS:
                    batch_output.append({"instances": self._materialize(pending.pop(0))})
                hp = self.host_profile
                hp["frames"] += 1
                hp["enqueue_s"] += t1 - t0
                hp["materialize_s"] += _time.perf_counter() - t1
                if self.save_semmap and i == 0:
                    self.save_memory_snapshot(frame["sequence_name"])          # custom_rcnn.py:518-530
        for ticket in pending:
            batch_output.append({"instances": self._materialize(ticket)})
        return batch_output

    def _post_ticket(self):
        """Async read-back of the frame's detection count into pinned host memory + an event; flips the result set."""
        cur = torch.cuda.current_stream(self.device)
        if self.overlap_branches:
            P = _ticket(self._post, self._err, cur, self._det_stream, after=self._ev_det[self._post_slot])
        else:
            P = _ticket(self._post, self._err, cur, None)
        self._post_slot = (self._post_slot + 1) % RESULT_SETS
        return P

    def _device_image(self, frame) -> torch.Tensor:
        img = frame["image"]
        if not torch.is_tensor(img):
            img = torch.as_tensor(np.asarray(img))
        if img.dtype != torch.uint8:
            img = img.to(torch.uint8)
        return img.to(self.device, non_blocking=True).contiguous()

    def _device_proj(self, frame) -> torch.Tensor:
        p = frame["proj_indices"]
        if not torch.is_tensor(p):
            p = torch.from_numpy(np.ascontiguousarray(p))
        if p.dim() == 3:
            p = p.squeeze(2)
        if p.dtype != torch.int32:
            p = p.to(torch.int32)
        return p.to(self.device, non_blocking=True).contiguous()

    def _enqueue_trunk(self, frames: List[dict], after: torch.cuda.Event, first: int = 0):
        """Bottom-up pass + FPN top-down convs of the coming frame(s) on the look-ahead stream, ordered after `after` (an event of
        the main stream recorded once the previous frame has fully finished).  Frame b of the list is written into pyramid set
        (current + 1 + first + b) -- `first` frames are ahead already; more than one frame = one batched pass.  The frames join
        `self._ahead` with the pass's own event."""
        if self._trunk_stream is None:
            # high priority like the side stream: its ~75 launches are small and must not queue behind the mask GEMMs' thousands
            # of workgroups
            self._trunk_stream = _sched_streams(self.device)[1]
            self._ev_trunk = torch.cuda.Event()
        ts = self._trunk_stream
        ts.wait_event(after)
        done = torch.cuda.Event()
        sets = [(self._pyramid + 1 + first + b) % PYRAMID_SETS for b in range(len(frames))]
        for st in sets:
            if st in self._pyr_reader:
                ts.wait_event(self._pyr_reader[st])      # a trailing detection pass may still read that set
        with torch.cuda.stream(ts):
            self._mark("trunk_lookahead_begin", ts)
            xs = []
            for f in frames:
                x4, Hp, Wp = ops.preprocess_image(self._device_image(f), self.pixel_mean, self.pixel_std)
                xs.append(x4)
            if len(frames) == 1:
                self.backbone.top_down(self.backbone.bottom_up.forward(xs[0], Hp, Wp), 1, self.backbone._plan(Hp, Wp, sets[0])[3])
            else:
                n = len(frames)
                c = self.backbone.bottom_up.forward(torch.cat(xs, dim=0), Hp, Wp, N=n)
                p345 = self.backbone.top_down(c, n, planned=True)
                for b, st in enumerate(sets):
                    views = self.backbone._plan(Hp, Wp, st)[3]
                    for l in range(3):
                        views[l].copy_(p345[l][b:b + 1])
            done.record(ts)
            self._mark("trunk_lookahead", ts)
        self._ahead = self._ahead + [dict(image=f["image"], Hp=Hp, Wp=Wp, event=done) for f in frames]

    def inference_frame(self, frame: dict, refresh_memory_snapshot: bool = True, materialize: bool = True,
                        next_frame=None, trailing_detection_pass: bool = False):
        """One frame: `inference` (custom_rcnn.py:548-582) + `update_implicit_memory` (681-760).  `next_frame` (optional) is the
        frame the caller will pass next -- or the list of the frames it will pass next, in order: their memory-independent
        bottom-up passes are started early (`lookahead_frames` of them at a time as one batched pass).  `trailing_detection_pass`
        (set by `forward` for every frame but the last of a call): do not join the detection-pass stream at the end of the frame;
        the caller reads the results through `_post_ticket` / `_materialize` only."""
        H, W = int(frame["image"].shape[-2]), int(frame["image"].shape[-1])
        if H % 32 or W % 32:
            raise ValueError("H and W must be multiples of 32 (proj_indices is not padded: SURVEY §8 notation)")
        proj = self._device_proj(frame)
        if tuple(proj.shape) != (H, W):
            raise ValueError(f"proj_indices shape {tuple(proj.shape)} != image {(H, W)}")
        n_cells = self.implicit_memory.shape[0]
        self._ensure_frame_buffers(H, W, n_cells)
        self._frame_no += 1
        self._mark("start")

        # a4 + fp16 cast (create_implicit_memory + preprocess_spatial_memory)
        mem_f16 = None
        if self.memory_type == "implicit_memory":
            if refresh_memory_snapshot:
                self._refresh_memory_snapshot()
            mem_f16 = self._mem_f16

        coming = [] if next_frame is None else (list(next_frame) if isinstance(next_frame, (list, tuple)) else [next_frame])
        pre, start_batch, first_ahead = self._claim_lookahead(frame, coming)
        if start_batch:
            # the look-ahead may start NOW, beside this frame's memory fusion, tower and proposal decoding (a short latency-bound
            # chain that leaves most of the chip idle); the host enqueues that chain first so that the main stream never starves
            if self._ev_start is None:
                self._ev_start = torch.cuda.Event()
            self._ev_start.record(torch.cuda.current_stream(self.device))
        views, shapes, props = self._front(frame, pre, proj, mem_f16)
        if start_batch:
            self._enqueue_trunk(start_batch, self._ev_start, first_ahead)
        if self.roi_heads.fuses_mem_rescore(self.zs_weight):
            self._mem_scores_frame = self._frame_no      # `mem_scores`: written by stage 0 of this frame's cascade
        if self.overlap_branches:
            self._frame_pipelined(frame, (H, W), views, shapes, props, proj, trailing_detection_pass)
        else:
            self._frame_in_order(frame, (H, W), views, shapes, props, proj)

        P = self._post
        self.last_stats = {"prop_count": props[2], "det_count": P["count"], "mem_k": self._writer.k_out,
                           "det_mask_rois": self.roi_heads.last_selector.rep_count if self.dedup_detection_masks else P["count"]}
        if self.stats_log is not None:      # bench.py: device-side copies of the frame's counters, read after the timed region
            if self.overlap_branches and trailing_detection_pass:
                with torch.cuda.stream(self._det_stream):      # the count is written by the trailing detection pass: copy it there
                    cnt = P["count"].clone()
            else:
                cnt = P["count"].clone()
            self.stats_log.append((props[2].clone(), cnt, self._writer.k_out.clone(), self._uniq_count.clone(),
                                   self.last_stats["det_mask_rois"].clone()))
        if not materialize:
            return None
        return {"instances": self._materialize(self._post_ticket())}

    def _claim_lookahead(self, frame: dict, coming: List[dict]):
        """The frame's place in the look-ahead window; bookkeeping and `wait_event`s on the current stream, no launch.  Moves
        `self._pyramid` to the frame's pyramid set and returns (the entry of `self._ahead` that holds this frame's trunk, or None when
        it has to be computed now; the frames of `coming` whose trunk pass starts in this frame, one batch of one image size, [] for
        none; how many frames are ahead already)."""
        cur = torch.cuda.current_stream(self.device)
        ext, self._prefetched = self._prefetched, None
        if isinstance(ext, tuple):                 # (image, Hp, Wp) computed into the next set by BatchedSequences, its event in _ev_trunk
            self._ahead = [dict(image=ext[0], Hp=ext[1], Wp=ext[2], event=self._ev_trunk)]
        ahead = self._ahead
        hit = bool(ahead) and ahead[0]["image"] is frame["image"]
        if ahead and not hit:
            for e in ahead:                        # the hint was wrong: what runs ahead must be over before any set or the trunk's
                cur.wait_event(e["event"])         # own buffers are touched again
            ahead = []
        pre = None
        if hit:
            pre = ahead.pop(0)
            cur.wait_event(pre["event"])           # this frame's own pass only: later passes may still be running
        # every frame moves to the next of PYRAMID_SETS pyramid sets (the look-ahead wrote P3..P5 of a hit into exactly that one);
        # a trailing detection pass of the frame that last used the set must be over before a miss recomputes into it
        self._pyramid = (self._pyramid + 1) % PYRAMID_SETS
        if not hit and self._pyramid in self._pyr_reader:
            cur.wait_event(self._pyr_reader[self._pyramid])
        # frames further ahead stay valid only if the caller really passes them next (checked frame by frame)
        keep = 0
        while keep < len(ahead) and keep < len(coming) and ahead[keep]["image"] is coming[keep]["image"]:
            keep += 1
        for e in ahead[keep:]:
            cur.wait_event(e["event"])             # dropped: over before their sets are written again
        self._ahead = ahead = ahead[:keep]
        depth = max(1, int(self.lookahead_frames)) if self.lookahead_depth is None else max(1, int(self.lookahead_depth))
        batch = []
        if self.prefetch_trunk and self.overlap_branches and len(ahead) < min(depth, PYRAMID_SETS - 2):
            room = PYRAMID_SETS - 2 - len(ahead)
            batch = coming[len(ahead):len(ahead) + min(max(1, int(self.lookahead_frames)), room)]
            # one pass = one image size (the N = 2 pass stacks the images); a frame of another size starts its own pass later
            n_same = 0
            for f in batch:
                if tuple(f["image"].shape) != tuple(batch[0]["image"].shape):
                    break
                n_same += 1
            batch = batch[:n_same]
        return pre, batch, len(ahead)

    def _front(self, frame: dict, pre: Optional[dict], proj, mem_f16):
        """Memory read + fusion and the top of the pyramid (on the trunk computed ahead, `pre`, or behind the frame's own preprocess
        + trunk), then the proposal generator -> (views, shapes, (proposal boxes, scores, count))."""
        if pre is not None:
            feats, views, shapes, off = self.backbone.fuse_memory_and_top(pre["Hp"], pre["Wp"], mem_f16, proj, self._pyramid, self._err)
        else:
            x4, Hp, Wp = ops.preprocess_image(self._device_image(frame), self.pixel_mean, self.pixel_std)
            feats, views, shapes, off = self.backbone.forward(x4, Hp, Wp, mem_f16, proj, self._pyramid, self._err)
        return views, shapes, self.proposal_generator.forward(feats, shapes, off)

    def _frame_in_order(self, frame: dict, image_hw, views, shapes, props, proj):
        """`overlap_branches = False`: the rest of the frame on the current stream, one launch after the other."""
        H, W = image_hw
        prop_boxes, prop_scores, prop_count = props
        self.roi_heads.forward_box(views, shapes, prop_boxes, prop_scores, prop_count, (H, W), mem_rescore=(self.zs_weight, self.mem_scores))
        if self.front_event is not None:
            # the latency-bound front of the frame (memory fusion, tower, proposal decoding, cascade) ends here; what follows is
            # dense (mask passes): BatchedSequences staggers its scenes on this point
            self.front_event.record(torch.cuda.current_stream(self.device))
        rh, k = self.roi_heads, self._post_slot
        self._check_output_size(frame, (H, W))
        rh.detection_masks(rh.bufs, views, shapes, rh.last_selector, k, self.dedup_detection_masks, rh.det_pass_lds_reserve,
                           ("det", self._frame_no))
        mem_sel = None
        if self.lazy_proposal_masks:
            # select the memory instances first, then run the mask head only on those proposals (same results: the other
            # proposals' masks are never read, custom_rcnn.py:875-880)
            mem_sel = self.select_memory_instances(prop_boxes, prop_scores, prop_count, (H, W))
            prop_masks = self.roi_heads.forward_mask_memory(views, shapes, prop_boxes, prop_count, rows=self._uniq_rows,
                                                            rows_count=self._uniq_count, tag=("prop", self._frame_no))
        else:
            prop_masks = self.roi_heads.forward_mask_memory(views, shapes, prop_boxes, prop_count, tag=("prop_all", self._frame_no))
        # detector_postprocess (custom_rcnn.py:579-580)
        rh.postprocess_and_paste(rh.bufs, rh.last_selector, self._post, (H, W), self.mask_threshold, self.dedup_detection_masks)
        # memory update (custom_rcnn.py:515)
        self.update_implicit_memory(prop_boxes, prop_scores, prop_count, prop_masks, proj, (H, W), mem_sel)

    def _frame_pipelined(self, frame: dict, image_hw, views, shapes, props, proj, trailing_detection_pass: bool):
        """`overlap_branches`: the rest of the frame over three streams, in the order the host enqueues it.
        main (the current stream): the memory selection's suppression matrix; behind cascade stage 0 the memory selection and the
        proposal masks; joins the memory write -- and the detection pass unless it may trail.
        side: box cascade (stage 0 | stages 1-2) -> detection selection -> memory write.
        detection stream: detection masks + post-processing + paste, behind `detection_pass_after`."""
        H, W = image_hw
        prop_boxes, prop_scores, prop_count = props
        main = torch.cuda.current_stream(self.device)
        if self._side_stream is None:
            self._side_stream = _sched_streams(self.device)[0]     # high priority: the small launches go first
            self._ev_props, self._ev_pm, self._ev_box, self._ev_mem, self._ev_s0 = (torch.cuda.Event() for _ in range(5))
        side = self._side_stream
        self._ev_props.record(main)
        self._mark("proposals", main)
        lazy = self.lazy_proposal_masks
        # Host enqueue order matters (the GPU runs behind the host here): a stream's launches are enqueued in the order the GPU
        # gets to them -- stage 0, then the main stream's selection and large mask launches (`memory_chain`), then the side
        # stream's other ~35 small ones; they all execute beside the two mask passes.
        if not lazy:
            prop_masks = self.roi_heads.forward_mask_memory(views, shapes, prop_boxes, prop_count,
                                                            bufs=self.roi_heads.bufs.proposal_pass_buffers(), tag=("prop_all", self._frame_no))
            self._ev_pm.record(main)
        mem_sel = None
        # the memory selection's suppression matrix needs the proposal boxes only: built here, on the main stream, which has nothing
        # else to do until stage 0 is over, it is off the chain
        if lazy and self.mem_selector.takes_row_matrix:
            self.mem_selector.build_row_matrix(prop_boxes, prop_count, float(W), float(H), MEMORY_NMS_THRESH)

        def memory_chain():
            # Called by the cascade between stage 0 and stage 1 (side stream current).  The frame's critical chain (memory selection
            # -> proposal masks -> memory write -> next frame's memory read) starts here: all it reads -- `mem_scores` and `featn0`
            # (stage 0's classifier launch), the proposal boxes and count -- is final, and stages 1-2 write none of it (their
            # outputs: pool7, h1, h2, hb, feat, deltas, prob, boxes[2..3]).  The refined boxes feed the detections only, which have
            # slack.  The mask head runs only on the proposals the selection keeps (same results: the other proposals' masks are
            # never read, custom_rcnn.py:875-880); its large launches are enqueued here, ahead of the ~20 small ones of stages 1-2,
            # the detection selection and the detection pass, because the GPU gets to them first.
            nonlocal mem_sel, prop_masks
            self._ev_s0.record(side)
            main.wait_event(self._ev_s0)
            with torch.cuda.stream(main):
                mem_sel = self.select_memory_instances(prop_boxes, prop_scores, prop_count, (H, W))
                self._mark("mem_select", main)
                prop_masks = self.roi_heads.forward_mask_memory(views, shapes, prop_boxes, prop_count, rows=self._uniq_rows,
                                                                rows_count=self._uniq_count,
                                                                bufs=self.roi_heads.bufs.proposal_pass_buffers(), tag=("prop", self._frame_no))
                self._ev_pm.record(main)
                self._mark("prop_masks", main)

        side.wait_event(self._ev_props)
        with torch.cuda.stream(side):
            k = self._post_slot
            if self._ev_det[k] is not None:
                side.wait_event(self._ev_det[k])     # the detection list set k is still read by frame t-2's pass
            self.roi_heads.forward_box(views, shapes, prop_boxes, prop_scores, prop_count, (H, W), sel=k,
                                       mem_rescore=(self.zs_weight, self.mem_scores), after_stage0=memory_chain if lazy else None)
            self._ev_box.record(side)
            self._mark("cascade+det_select", side)
        det_after = self.detection_pass_after if lazy else "cascade"
        if det_after == "cascade":
            self._enqueue_detection_pass(views, shapes, (H, W), frame)
        if det_after == "proposal_masks":
            self._enqueue_detection_pass(views, shapes, (H, W), frame, after=self._ev_pm)
        # memory update (custom_rcnn.py:515): it needs the proposal masks and the selection (main stream, both before `_ev_pm`) and
        # runs on the side stream beside the detection mask pass -- behind this frame's stages 1-2 and ahead of the next frame's
        # stage 0, which overwrites `featn0` and `mem_scores`; the main stream joins below
        with torch.cuda.stream(side):
            if not lazy:
                mem_sel = self.select_memory_instances(prop_boxes, prop_scores, prop_count, (H, W))
            side.wait_event(self._ev_pm)
            self.update_implicit_memory(prop_boxes, prop_scores, prop_count, prop_masks, proj, (H, W), mem_sel)
            self._ev_mem.record(side)
            self._mark("mem_write", side)
        if det_after == "memory_write":
            self._enqueue_detection_pass(views, shapes, (H, W), frame, after=self._ev_mem)
        main.wait_event(self._ev_mem)
        if not trailing_detection_pass:
            main.wait_event(self._ev_det[self._post_slot])     # in-order callers see a finished frame

    def _mark(self, name: str, stream=None):
        """Diagnostics (`model.trace = []`): a timing event on `stream` (default: current) at a named point of the frame's schedule;
        tools/frame_schedule.py turns the list into a per-frame timeline without a profiler in the way."""
        if self.trace is None:
            return
        ev = torch.cuda.Event(enable_timing=True)
        ev.record(stream if stream is not None else torch.cuda.current_stream(self.device))
        self.trace.append((self._frame_no, name, ev))

    @staticmethod
    def _check_output_size(frame: dict, image_hw):
        H, W = image_hw
        if (int(frame.get("height", H)), int(frame.get("width", W))) != (H, W):
            raise NotImplementedError("output size != input size is not used on this path (train_mp3d.py:487-490)")

    def _enqueue_detection_pass(self, views, shapes, image_hw, frame, after=None):
        """`forward_with_given_boxes` (detic_roi_heads.py:257) + `detector_postprocess` + paste (custom_rcnn.py:579-580) of this
        frame on the detection stream (lowest priority: its GEMMs fill whatever the latency-bound chains of the frame -- and of
        the next frame -- leave idle)."""
        if self._det_stream is None:
            self._det_stream = _det_stream(self.device)
            self._ev_det = [torch.cuda.Event() for _ in range(RESULT_SETS)]
        ds = self._det_stream
        rh, k = self.roi_heads, self._post_slot
        self._check_output_size(frame, image_hw)
        ds.wait_event(self._ev_box)
        if after is not None:
            ds.wait_event(after)
        with torch.cuda.stream(ds):
            self._mark("det_pass_begin", ds)
            rh.detection_pass(rh.bufs, views, shapes, rh.last_selector, k, self._post, image_hw, self.mask_threshold,
                              self.dedup_detection_masks, rh.det_pass_lds_reserve, ("det", self._frame_no))
            self._ev_det[k].record(ds)
            self._mark("det_pass", ds)
        self._pyr_reader[self._pyramid] = self._ev_det[k]

    def select_memory_instances(self, prop_boxes, prop_scores, prop_count, image_hw):
        """`inference_with_proposals` up to the NMS (custom_rcnn.py:825-875): CLIP re-score of the proposals, threshold
        MEMORY_CLS_SCORE_THRESH, per-class NMS 0.5, top 100 -> (proposal row of every kept detection, count).
        The selector reads the suppression matrix of these boxes when `mem_selector.build_row_matrix` has built it ahead."""
        H, W = image_hw
        R = self.proposal_generator.cap
        if self._mem_scores_frame != self._frame_no:        # not written by this frame's cascade (forward_box without mem_rescore)
            ops.memory_scores(self.roi_heads.featn0, self.zs_weight, prop_scores, self.mem_scores, prop_count, R, self.C1)
        _, _, _, rows, cnt = self.mem_selector(prop_boxes, self.mem_scores, prop_count, float(W), float(H), self.cls_score_thresh,
                                               MEMORY_NMS_THRESH)
        return rows, cnt

    def update_implicit_memory(self, prop_boxes, prop_scores, prop_count, prop_masks, proj, image_hw, mem_sel=None):
        """The write-back; like the reference, the frame runs it for every MEMORY_TYPE (custom_rcnn.py:515,573)."""
        rows, cnt = mem_sel if mem_sel is not None else self.select_memory_instances(prop_boxes, prop_scores, prop_count, image_hw)
        self._last_write = (prop_boxes, prop_masks, rows, cnt, proj)          # bench.py's HBM-class probe replays it
        follow = self.snapshot_follows_write if self.snapshot_follows_write is not None else self.test_type in ("default", "episodic")
        if follow and self._f16_valid and not self._dirty_pending:
            self._writer(self.roi_heads.featn0, prop_boxes, prop_masks, rows, cnt, proj, self.implicit_memory, self.observations,
                         err=self._err, snapshot=self._mem_f16)
        else:
            self._writer(self.roi_heads.featn0, prop_boxes, prop_masks, rows, cnt, proj, self.implicit_memory, self.observations,
                         dirty=self._dirty, err=self._err)
            self._dirty_pending = True

    def save_memory_snapshot(self, sequence_name: str) -> str:
        """`MODEL.TEST_SAVE_SEMMAP` dump (custom_rcnn.py:518-530): semmap, impicit_memory [sic], observations -> OUTPUT_DIR/memory/."""
        from ..data.snapshot import write_snapshot
        semmap = self.semantic_map()
        return write_snapshot(self.output_dir, sequence_name, semmap.cpu().numpy(), self.implicit_memory.cpu().numpy(),
                              self.observations.cpu().numpy())

    def _materialize(self, P) -> Instances:
        """The `Instances` of a ticket (`_instances`: the frame's only host wait)."""
        return _instances(P, self._err, self.host_profile, self.implicit_memory.shape[0], self.device)[0]

    def semantic_map(self, classifier=None, num_classes: Optional[int] = None, thresh: Optional[float] = None, scores: bool = False):
        """a20, evaluated lazily: the explicit map `self.semmap` the reference recomputes (and syncs to the host) every
        frame (custom_rcnn.py:756) but only consumes when MODEL.TEST_SAVE_SEMMAP dumps it (518-530).

        With `classifier` (a `[C, 512]` .npy path or a `[512, C]` tensor of up to 2047 classes, as `reset_cls_test` takes it) or
        `scores=True` the memory is read as it stands in that vocabulary (default: the meta-architecture's own) and the call returns
        `(labels, scores)`: per cell the argmax class, -1 below `thresh` (None: MEMORY_OBS_SCORE_THRESH; 0.0 keeps every cell), and
        the softmax probability of that class (`max_scores`, custom_rcnn.py:955-958).  Such a query changes nothing in the model."""
        if classifier is None and not scores:
            self.semmap = ops.semmap_labels(self.implicit_memory, self.observations, self.zs_weight,
                                            self.obs_score_thresh if thresh is None else float(thresh))
            return self.semmap
        return _semmap_query(self, self.implicit_memory, self.observations, classifier, num_classes, thresh)

    def locate(self, classes, classifier=None, num_classes: Optional[int] = None, thresh: Optional[float] = None, map_shape=None,
               radius: int = 1, topk: int = 8):
        """Where on the map the classes `classes` (1 to 32 indices into the vocabulary; `classifier`, `num_classes`, `thresh` as in
        `semantic_map`) are most likely, as `ops.semmap_locate` returns it: `labels`, `scores`, `prob` [Q, N] (each class's softmax
        probability per cell, 0 below the threshold), `peaks` / `peak_scores` [Q, topk] (the best local maxima within `radius`
        cells on the grid `map_shape` = (rows, cols), cell = r * cols + c; without it the plain top-k).  Changes nothing in the
        model."""
        return _semmap_locate(self, self.implicit_memory, self.observations, classes, classifier, num_classes, thresh, map_shape,
                              radius, topk)

    def regions(self, classes, classifier=None, num_classes: Optional[int] = None, thresh: Optional[float] = None, map_shape=None,
                level: float = 0.5, connectivity: int = 8, min_cells: int = 1, topk: int = 16, radius: int = 1, peaks: int = 8) -> dict:
        """The map objects of the queried classes: `locate(classes, ..., map_shape, radius, topk=peaks)` and, on its `prob`, the
        connected regions of the cells with `prob >= level` as `ops.map_regions` returns them (`region_labels` [Q, N], `count`,
        `foreground` [Q], and for the `topk` largest regions of at least `min_cells` cells `region`, `area`, `bbox`, `sum_rc`, `peak`,
        `peak_prob`, `mass_q24`, `status`), in one dict with locate's keys.  `map_shape` = (rows, cols) is required.
        `region_labels[q, cell]` names the map object a cell belongs to (a `pred_cells` of `place`, for one).  Raises `EodError`
        if the op's status is nonzero.  Changes nothing in the model."""
        return _map_regions(self, self.implicit_memory, self.observations, classes, classifier, num_classes, thresh, map_shape, level,
                            connectivity, min_cells, topk, radius, peaks)

    def inventory(self, classifier=None, num_classes: Optional[int] = None, thresh: Optional[float] = None, map_shape=None,
                  level: float = 0.5, connectivity: int = 8, min_cells: int = 1, topk: int = 16, exclude=None) -> dict:
        """What the map holds, all classes at once: `semantic_map(classifier, num_classes, thresh, scores=True)` as `labels` and
        `scores` [N] and, on them, every object as `ops.map_inventory` returns it: a connected area of cells that carry one label
        with `scores >= level` (`object_labels` [N], `count`, `foreground`; for the `topk` largest objects of at least `min_cells`
        cells over all classes `object`, `cls`, `area`, `bbox`, `sum_rc`, `peak`, `peak_score`, `mass_q24`; per class
        `class_objects`, `class_cells`, `class_largest`, `class_largest_area` [C]; `status`).  `map_shape` = (rows, cols) is required.
        `exclude`: class indices to leave out (walls and floors would otherwise be the largest objects).  `level = 2 ** -11` keeps
        every labelled cell of any vocabulary.  Raises `EodError` if the op's status is nonzero.  Changes nothing in the model."""
        return _map_inventory(self, (self.implicit_memory, self.observations), classifier, num_classes, thresh, map_shape, level,
                              connectivity, min_cells, topk, exclude)

    def describe(self, objects, object_labels, classifier=None, num_classes: Optional[int] = None, topn: int = 5, embedding=None) -> dict:
        """What the map objects are, each as a whole: the memory rows of an object's cells pooled into one CLIP-space direction
        (`ops.describe_pool`: `sum_q`, `cells`, `embedding` [K, 512], `coherence` [K]) and that direction classified
        (`ops.describe_classify`: `prob` [K, C], `top_cls`, `top_prob` [K, topn]) in the model's own vocabulary or in `classifier`
        (as in `semantic_map`), in one dict.  `objects` int32 [K] (a sequence will do) and `object_labels` int32 [N]: `inv["object"]`
        and `inv["object_labels"]` of `inventory`, or a row of `region_labels` of `regions` with its `region` row.  With
        `embedding=` (an earlier call's, or a snapshot's) the pooling is skipped: the same objects asked in another vocabulary, no
        pass over the cells; `objects` and `object_labels` are then not read.  Embeddings of two maps compare as
        `a["embedding"] @ b["embedding"].T`.  Changes nothing in the model."""
        return _describe(self, self.implicit_memory, objects, object_labels, classifier, num_classes, topn, embedding)

    def relations(self, objects, object_labels, map_shape=None, radius: int = 2, from_cell: Optional[int] = None, topn: int = 4) -> dict:
        """How the map objects stand to each other and to one cell: the dict of `ops.map_relations` for `objects` int32 [K] (a
        sequence will do) and `object_labels` int32 [N] (`inv["object"]` and `inv["object_labels"]` of `inventory`, or a row of
        `region_labels` of `regions` with its `region` row) on the grid `map_shape` = (rows, cols), which is required.  For every
        ordered pair of objects with cells within `radius` of each other (a disc on the grid): `min_d2`, `closest` (the cell of a
        nearest to b), `near_cells` (`near_cells[a, b] == cells[a]`: a lies on / inside the reach of b), `edges` (the shared
        border), `pair_key`; per object `cells`, its `topn` `nearest` objects with `nearest_d2`, and from `from_cell` (the robot's
        cell, `RobotFrontEnd.exclude_cell(pose)`; None: not asked) `from_d2`, `from_closest` (the cell to drive to) and `from_key`,
        whatever the radius.  Distances in metres: `RobotFrontEnd.relation_metres`.  Reads neither the model nor the memory."""
        return _relations(objects, object_labels, map_shape, radius, from_cell, topn)

    def route(self, objects, object_labels, map_shape=None, from_cell: Optional[int] = None, passable=None, path_max: int = 256,
              sweeps: Optional[int] = None, body_radius2: Optional[int] = None) -> dict:
        """How to reach the map objects: the dict of `ops.map_route` for `objects` int32 [K] (a sequence will do) and
        `object_labels` int32 [N] (`inv["object"]` and `inv["object_labels"]` of `inventory`) on the grid `map_shape` =
        (rows, cols), from `from_cell` (the robot's cell, `RobotFrontEnd.exclude_cell(pose)`); both are required.  Every labelled
        cell blocks unless its label is one of `passable`; unlabelled cells are free, also where the memory knows nothing: the
        optimistic planner's assumption.  Moves go to the 8 neighbours and never between two blocked cells that touch at a corner;
        they cost 5 along a row or column and 7 diagonally.  `dist` and `parent` [N] are the cost from `from_cell` and the cell a
        cheapest path enters from; per object `goal_cell` is the free cell beside it to stop on, `goal_cost` the cost to it
        (INT_MAX: no way there), `path` [K, path_max] the cells from `goal_cell` back to `from_cell` (-1 behind them), `path_cells`
        their number, `cells` the object's cells; `counts` the free and the reached cells.  Metres: `RobotFrontEnd.route_metres`
        and `cell_centers(route["path"][k])`.  `sweeps` (None: `ops.map_route_sweeps`) is the number of sweep launches of one call;
        the status is read here, a call whose sweeps ran out is resumed up to `ops.ROUTE_RESUMES` times, and `EodError` is raised
        if the distances have not settled by then.  `body_radius2` (None: a point, nothing else runs): the squared radius of the
        robot's body in cells (`RobotFrontEnd.body_radius2`); the call then runs `clearance(radius2=body_radius2,
        keep_cell=from_cell, passable=passable)` first and routes on its `inflated` labels, and the dict gains `clearance_d2` and
        `inflated_labels` [N].  Every object is then grown by the radius: `goal_cell` lies on the rim of the inflated object, where
        the body's centre may stand, and `cells` counts the inflated cells.  Reads neither the model nor the memory.  See also
        `obstacles`: `model.route(inv["object"], obs["merged_labels"], ...)` goes round the walls the heights show as well."""
        return _route(objects, object_labels, map_shape, from_cell, passable, path_max, sweeps, body_radius2)

    def clearance(self, objects, object_labels, map_shape=None, radius2: int = 0, keep_cell: Optional[int] = None, passable=None) -> dict:
        """How much room there is round the map objects: the dict of `ops.map_clearance` for `objects` int32 [K] (a sequence will
        do) and `object_labels` int32 [N] (`inv["object"]` and `inv["object_labels"]` of `inventory`) on the grid `map_shape` =
        (rows, cols), which is required.  Every labelled cell blocks unless its label is one of `passable`.  Per cell `d2` is the
        exact squared distance in cells to the nearest blocked cell (0 on one; INT_MAX on a map without any), `nearest` that cell
        (the lowest on a tie) and `owner` its label: the partition of the free space by nearest object.  `inflated` is the label map
        for a body of squared radius `radius2` (`RobotFrontEnd.body_radius2`): free cells at most that far from an object take its
        label, except those at most that far from `keep_cell` (the robot's cell; None: no exception); hand it to `route`, or
        pass `body_radius2` there.  Per object `cells`, `territory` (the free cells nearest to it), and `widest_cell` / `widest_d2`:
        the most open cell of its territory (`sight` says whether the object is in view from it); `open_key`: the most open cell of the map;
        `counts`: blocked, free and inflated cells.  Metres: `RobotFrontEnd.clearance_metres`.  The status is read here.  Reads
        neither the model nor the memory.  See also `obstacles`: `model.clearance(inv["object"], obs["merged_labels"], ...)`
        measures the room between the walls the heights show as well."""
        return _clearance(objects, object_labels, map_shape, radius2, keep_cell, passable)

    def sight(self, objects, object_labels, map_shape=None, from_cells=None, range2: Optional[int] = None, passable=None) -> dict:
        """What can be seen from where: the dict of `ops.map_sight` for `objects` int32 [K] (a sequence will do) and
        `object_labels` int32 [N] (`inv["object"]` and `inv["object_labels"]` of `inventory`) on the grid `map_shape` =
        (rows, cols), from the cells `from_cells` (one int, or a sequence or tensor of up to 64; negative: unused); both are
        required.  Every labelled cell is opaque unless its label is one of `passable`; a source's own cell never blocks its own
        view.  `range2` is the sensor's range in cells, squared (`RobotFrontEnd.sight_range2`; None: unbounded).  Source s sees a
        cell when it is in range and the rounded straight line to it meets no opaque cell before it and passes between no two
        opaque cells that touch at a corner; the cell itself may be opaque: one sees the face of an object.  `seen_mask` int64 [N]
        holds bit s of cell i for source s; per (source, object) `seen_cells` is how many of the object's cells the source sees and
        `near_cell` / `near_d2` the nearest of them (-1 / INT_MAX: none; metres: `RobotFrontEnd.relation_metres(near_d2)`); per
        object `best_source` is the candidate that sees most of it (-1: none does) and `best_seen` how many cells that is;
        `source_counts` the transparent and opaque cells each source sees; `counts` the opaque, the transparent and the seen cells.

            clr = model.clearance(objs, labels, shape)
            rt = model.route(objs, labels, shape, from_cell=here)
            s = model.sight(objs, labels, shape, from_cells=torch.cat([torch.tensor([here], device=labels.device),
                            clr["widest_cell"], rt["goal_cell"]]), range2=front.sight_range2(4.0))
            s["best_source"][k]          # which of the candidates to drive to for a look at object k

        `from_cells` is the one argument the entry point reads on the host (a cell outside the map is refused before any launch):
        a device tensor, as in the lines above, is copied there first, one synchronisation; a sequence of ints costs none.  Never
        hand `eod_map_sight` itself a device pointer for it.  The status is read here.  Reads neither the model nor the memory.  See
        also `obstacles`: `model.sight(inv["object"], obs["merged_labels"], ...)` stops at the walls the heights show as well."""
        return _sight(objects, object_labels, map_shape, from_cells, range2, passable)

    def cover(self, proj_indices, stamp: Optional[int] = None, exclude_cell: int = -1) -> torch.Tensor:
        """Record what the camera covered: every cell under a pixel of the frame's `proj_indices` (numpy or tensor, [H, W] or
        [H, W, 1]; the cells outside the map and `exclude_cell` are dropped, as in `place`) takes the stamp of this call in
        `last_seen` int32 [N], which is returned (-1: never covered).  The buffer is made at the first call after a
        `reset_memory` and dropped by the next one.  `stamp` None: a counter that grows by one per call, from 0, and goes on across a
        `reset_memory` (a stamp never repeats; `since=` the first stamp after the reset asks for what was covered since); an int:
        that stamp, and the counter goes on behind it.  One launch of `ops.map_cover`; the frame itself never calls it, and nothing it
        computes changes."""
        if self.implicit_memory is None:
            raise _lib.EodError("cover: no memory yet (no frame has run)")
        if stamp is None:
            stamp = self._cover_stamp
        self._last_seen = _cover(self, proj_indices, self._last_seen, int(self.implicit_memory.shape[0]), stamp, exclude_cell)
        self._cover_stamp = max(self._cover_stamp, int(stamp) + 1)
        return self._last_seen

    def frontiers(self, object_labels, map_shape=None, since: int = 0, last_seen=None, from_cell: Optional[int] = None, route=None,
                  passable=None, min_cells: int = 2, topk: int = 16, rank_by="behind") -> dict:
        """Where the known space ends and what lies beyond: the dict of `ops.map_frontier` for `object_labels` int32 [N]
        (`inv["object_labels"]` of `inventory`) on the grid `map_shape` = (rows, cols), which is required.  A labelled cell is
        BLOCKED unless its label is one of `passable`; every other cell is OPEN when `last_seen >= since` and UNKNOWN when not.  A
        frontier is an 8-connected set of OPEN cells that each have an UNKNOWN 4-neighbour.  Per frontier, ranked by `rank_by`
        ("behind": the cells of the largest unknown region it opens onto; "area": its own cells), `frontier` (its label, the
        lowest cell; -1: padding), `area`, `bbox`, `sum_rc` (`RobotFrontEnd.region_centroids`), `open_edges`, `behind_area` /
        `behind_label`, and `reach_cell` / `reach_cost`: the known free cell of it to drive to (`RobotFrontEnd.cell_centers`) and
        what the way costs: with `route=` (the dict of `route`, or its `dist`) the cost of the route there
        (`RobotFrontEnd.route_metres`; a frontier no route reaches has INT_MAX / -1), otherwise with `from_cell` the squared
        distance in cells (`RobotFrontEnd.relation_metres`), otherwise 0 and the lowest cell.  Per cell `frontier_labels`,
        `unknown_labels`, `unknown_area`; `count`, `counts` (BLOCKED, OPEN, UNKNOWN, frontier cells, unknown regions).

            model.cover(data["proj_indices"], exclude_cell=front.exclude_cell(pose))        # after every frame
            rt = model.route(inv["object"], inv["object_labels"], shape, from_cell=here)
            fr = model.frontiers(inv["object_labels"], shape, route=rt)
            front.cell_centers(fr["reach_cell"][:1])     # where to drive to look into the largest unknown region

        `last_seen` None takes the record `cover` keeps.  Where `cover` was never called since the last `reset_memory` it takes
        `observations > 0` as 0 / -1, a weaker record: the memory counts a cell only where a proposal's mask covered a pixel that
        landed in it, so bare floor and walls the camera saw without proposing anything there stay UNKNOWN, and the frontiers lie
        round the detected objects rather than at the edge of the view.  Raises when `status` is not 0.  Changes nothing of the
        model.  See also `obstacles`: `model.frontiers(obs["merged_labels"], ...)` takes a cell a wall's pixels covered as BLOCKED."""
        if last_seen is None:
            last_seen = self._last_seen
            if last_seen is None and self.observations is not None:
                last_seen = _observed(self.observations)
        return _frontiers(object_labels, map_shape, last_seen, since, from_cell, route, passable, min_cells, topk, rank_by)

    def heights(self, proj_indices, heights, band_mm=(100, 1500), exclude_cell: int = -1) -> torch.Tensor:
        """Record how high the things under the camera stand: every pixel of the frame's `proj_indices` (numpy or tensor, [H, W]
        or [H, W, 1]) brings its world height `heights` (float32 metres, [H, W], or the xyz [H, W, 3] of the projector, whose y is
        read in place; `frame["heights"]` of `RobotFrontEnd.frame(..., heights=True)`) to its cell of the height record int32
        [4, N], which is returned: hits, band_hits (the pixels with `band_mm[0]` <= millimetres <= `band_mm[1]`: the band a body
        takes, `RobotFrontEnd.height_band_mm`), h_min_mm, h_max_mm.  The cells outside the map, `exclude_cell` (the robot's own,
        where zero-depth pixels land) and heights that are not finite or beyond 1000 m are dropped.  The record is made at the first
        call after a `reset_memory` and dropped by the next one.  One launch of `ops.map_heights`; the frame itself never calls it,
        and nothing it computes changes."""
        if self.implicit_memory is None:
            raise _lib.EodError("heights: no memory yet (no frame has run)")
        self._height_record = _heights(self, proj_indices, heights, self._height_record, int(self.implicit_memory.shape[0]), band_mm,
                                       exclude_cell)
        return self._height_record

    def obstacles(self, object_labels=None, objects=None, map_shape=None, record=None, min_hits: int = 4, min_cells: int = 2,
                  topk: int = 16) -> dict:
        """What stands in the way, whether the vocabulary has a word for it or not: the dict of `ops.map_obstacles` for the height
        record `heights` keeps (`record` None) or the one given, on the grid `map_shape` = (rows, cols), which is required.  A
        cell is an OBSTACLE where at least `min_hits` pixels of the band landed; obstacle cells that touch (8 neighbours) form a
        structure (a wall, a cupboard), one of fewer than `min_cells` cells is dropped as noise.  `merged_labels` int32 [N] holds
        the labels of `object_labels` (None, or `inv["object_labels"]` of `inventory`) and, beside them, the structures' labels:
        the label map the other queries take as it stands,

            model.heights(data["proj_indices"], data["heights"], exclude_cell=front.exclude_cell(pose))     # after every frame
            obs = model.obstacles(inv["object_labels"], inv["object"], shape)
            rt = model.route(inv["object"], obs["merged_labels"], shape, from_cell=here)                    # round the walls

        and `clearance`, `sight` and `frontiers` alike.  Per cell also `kind` (0 UNSEEN, 1 CLEAR, 2 OBSTACLE, 3 OBJECT) and
        `structure_labels`; per structure `structure`, `area`, `bbox`, `sum_rc` (`RobotFrontEnd.region_centroids`), `top_mm`; per
        slot of `objects` (`inv["object"]`) `obj_cells`, `obj_seen_cells`, `obj_top_mm`, `obj_base_mm`: how high the table is;
        `count`, `counts`.  Raises when `status` is not 0.  Changes nothing of the model."""
        return _obstacles(self._height_record if record is None else record, map_shape, object_labels, objects, min_hits, min_cells,
                          topk)

    def rooms(self, labels, objects=None, map_shape=None, door_r2: Optional[int] = None, min_cells: Optional[int] = None,
              topk: int = 16, passable=None, known=None, clearance=None, sweeps: Optional[int] = None) -> dict:
        """The rooms of the map: the dict of `ops.map_rooms` for the label map `labels` int32 [N] (`obs["merged_labels"]` of
        `obstacles`, so that the walls divide the space) on the grid `map_shape` = (rows, cols); `map_shape`, `door_r2` and
        `min_cells` are required.  A free cell farther than `door_r2` (squared, in cells; `RobotFrontEnd.door_r2`) from every
        blocked cell is core; core cells that touch along a row or column form a region, one of at least `min_cells` cells is a
        room (its label its lowest cell), and every other free cell goes to the room that reaches it first by `route`'s moves.
        `known` (None, or uint8 [N]: `obs["kind"]`) takes the cells it holds 0 for out of every room.  `clearance`: the dict of
        `clearance` on the same labels and `passable`, or its `d2`; None: `ops.map_clearance` runs first, as in
        `route(body_radius2=...)`, and the dict gains `clearance_d2` either way.

            obs = model.obstacles(inv["object_labels"], inv["object"], shape)
            rooms = model.rooms(obs["merged_labels"], inv["object"], shape, door_r2=front.door_r2(1.0), min_cells=20, known=obs["kind"])
            rooms["obj_room"][k]                                   # the slot of the room object k stands in: "the chair in the other room"
            rooms["door_cell"][a, b]                               # the cell of room a in the door to room b (-1: no door)
            names = model.describe(rooms["room"], rooms["room_labels"], classifier=room_vocabulary)      # "kitchen", "bedroom"

        Per cell `room_labels` and `grow_dist`; per room `room`, `area`, `core_area`, `bbox`, `sum_rc`
        (`RobotFrontEnd.region_centroids`), `widest_cell` / `widest_d2` (where to stand), `room_objects`; per pair `door_edges`,
        `door_d2`, `door_cell`; per object `obj_room_cells`, `obj_room`, `obj_room_label`; `count`, `counts`.  `sweeps` None takes
        `ops.map_route_sweeps`; the status is read here, a call whose sweeps ran out is run again with twice as many, and
        `EodError` is raised if the keys have not settled by then.  Reads neither the model nor the memory."""
        return _rooms(labels, objects, map_shape, door_r2, min_cells, topk, passable, known, clearance, sweeps)

    def place(self, instances: Instances, proj_indices, topk: int = 4, exclude_cell: int = -1, attach: bool = False) -> dict:
        """Where on the map the detections of a frame stand: for every instance the grid cells under its mask, as
        `ops.place_masks` returns them (`mask_pixels`, `pixels`, `invalid`, `distinct` [K]; `cells`, `cell_pixels` [K, topk], the
        cells with the most mask pixels first, padded with -1 / 0).  `instances`: what the model returned for the frame;
        `proj_indices`: the frame's, numpy or tensor, [H, W] or [H, W, 1].  `exclude_cell` drops one cell (the robot's own, where
        zero-depth pixels land).  `attach=True` also sets `instances.pred_cells` (the cell with the most pixels, -1 for none) and
        `instances.pred_cell_pixels`.  One op on the current stream; nothing of the model changes."""
        return _place(self, self.implicit_memory, instances, proj_indices, topk, exclude_cell, attach)

    # ---- introspection used by tests / bench -----------------------------------------------------------
    def proposals_snapshot(self):
        dec = self.proposal_generator._plans[next(iter(self.proposal_generator._plans))][3]
        n = int(dec.count.item())
        return dict(proposal_boxes=dec.boxes[:n].cpu(), scores=dec.scores[:n].cpu(),
                    feat=self.roi_heads.feat0.view(-1, 512)[:n].cpu(), featn=self.roi_heads.featn0[:n].cpu(),
                    pred_masks=self.roi_heads.prop_masks[:n].cpu())
