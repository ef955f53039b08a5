"""B independent sequences in lock-step on one GPU with N = B through EVERY stage of the frame (BASELINE.json configs[4]: 4 sequences
at 960x960, 512x512 memory grid): one launch per stage for all scenes, B independent memory states.

Only independent sequences may be batched: inside a sequence frame t+1 reads the memory frame t wrote
(`Detic/detic/modeling/meta_arch/custom_rcnn.py:485-515`, `Detic/SMNet/loader.py:289-293`).

The frame is the one `CustomRCNNRecurrent.inference_frame` runs (`custom_rcnn.py:548-582` + `update_implicit_memory` 681-760), stage
by stage, on buffers that hold the B scenes back to back (the batch convention of include/eod_hip.h):

  preprocess (B small launches: the images arrive as B tensors) -> ResNet-50 trunk + FPN top-down, N = B (`timm.py:277-299,118-136`)
  -> memory read: gather + cascaded pooling and projection + fusion, grid.y = scene, B fp16 tables (`timm.py:142-192`)
  -> P6 / P7, N = B -> CenterNet tower + GroupNorm on the 5 B level images of the batch as one row list (`centernet_head.py:141-161`)
  -> proposal decoding, one workgroup per (level, scene) and per scene (`centernet.py:603-745`)
  -> cascade: ROIAlign over B x R boxes, the FC layers as ONE GEMM over B x R rows (per-scene counts: EodConvDesc.m_segments),
     classifier / deltas over B x R rows, detection selection one workgroup per scene (`detic_roi_heads.py:88-222`); stages 1-2
     and the detection selection on the side stream, beside what follows
  -> memory selection behind stage 0, one workgroup per scene (`custom_rcnn.py:825-875`)
  -> mask head on the memory instances and on the detection groups of ALL scenes: the scenes' lists are concatenated
     (eod_concat_lists) and each pass is one ROIAlign + 4 convs + the fused tail over the concatenation (`detic_roi_heads.py:257-268`)
  -> memory write: three launches for the B states (`custom_rcnn.py:884-936`) -> post-processing + paste, grid = scene.

This module holds the step's SCHEDULE only (streams, events, the look-ahead trunk, the idle slots) and the B memory states.  Every
stage above is the function the single-scene model calls, handed the batch: `backbone.top_down / fuse_memory_and_top`,
`CenterNet.forward`, and the heads' `_cascade`, `forward_mask_memory`, `detection_pass` on a `RoiBuffers` for B scenes
(modeling/roi_heads.py); result sets, ticket and `Instances` come from meta_arch.  The heads' knobs therefore mean here what they
mean for one scene.

Every layer is planned like ONE scene (`plan_rows`), so it walks K exactly as the single-scene call: the results of every scene
are bitwise those of its own `CustomRCNNRecurrent` run (tests/test_fullsize_gpu.py).  Pyramids are LEVEL MAJOR over the scenes
([level][scene][h*w] rows: the [B,h,w,256] images the N = B convs write), which is the one layout change against the single-scene
model.  `modeling/batched.py` (B scene objects on B streams, only the trunk batched) stays as the alternative schedule.

A sequence whose episode has ended (ragged episodes) stays in the batch as an idle slot: it is fed its last frame again, its memory
selection is emptied before the write (a write without instances leaves the state untouched, custom_rcnn.py:689-690) and its
results are dropped."""
from __future__ import annotations

import time as _time
from typing import Dict, List, Optional

import torch

from .. import _lib, ops
from .meta_arch import (RESULT_SETS, CustomRCNNRecurrent, _clearance, _cover, _describe, _det_stream, _frontiers, _heights, _instances,
                        _map_inventory, _map_regions, _observed, _obstacles, _place, _relations, _result_sets, _rooms, _rooms_batched, _route,
                        _sched_streams, _semmap_locate, _semmap_query, _sight, _ticket)
from .roi_heads import RoiBuffers

PYRAMID_SETS = 3      # the step's own, the one computed ahead, the previous step's (its detection pass may trail)


class _SceneView:
    """What tests and drivers read of one scene of the batch: its recurrent state."""

    def __init__(self, owner: "LockstepScenes", b: int):
        self._o, self._b = owner, b

    @property
    def implicit_memory(self):
        return None if self._o.implicit_memory is None else self._o.implicit_memory[self._b]

    @property
    def observations(self):
        return None if self._o.observations is None else self._o.observations[self._b]


class LockstepScenes:
    """`LockstepScenes(cfg, B)(episodes)`: `episodes` = list of B frame lists, one per sequence (`None` or `[]`: that sequence sits
    this call out; lengths may differ); returns a list of B output lists, each what `CustomRCNNRecurrent.forward([episode_b])`
    returns."""

    def __init__(self, cfg, batch: int, state_dict: Optional[Dict[str, torch.Tensor]] = None):
        if batch < 1 or batch > _lib.MAX_BATCH:
            raise ValueError(f"batch must be in [1, {_lib.MAX_BATCH}]")
        self.B = int(batch)
        # the layers, their weights and the configuration exist once; its single-scene buffers are not used
        self.model = CustomRCNNRecurrent(cfg, state_dict)
        m = self.model
        self.device = m.device
        self.scenes = [_SceneView(self, b) for b in range(self.B)]
        self.trunk_lookahead = True          # step t + 1's memory-independent trunk on its own stream beside step t's chain
        self.trail_detection_pass = True     # step t's detection mask pass + paste under step t + 1's latency-bound front
        self.implicit_memory: Optional[torch.Tensor] = None     # [B,N,512]
        self.observations: Optional[torch.Tensor] = None        # [B,N]
        self._last_seen: Optional[torch.Tensor] = None          # [B,N] int32: the stamp of the last `cover` of each cell, -1: none
        self._cover_stamp = [0] * self.B
        self._height_record: Optional[torch.Tensor] = None      # [B,4,N] int32: the record of `heights`, one row per scene
        self._mem_f16 = self._dirty = None
        self._f16_valid = False
        self._dirty_pending = False
        self._err = torch.zeros((1,), dtype=torch.int32, device=self.device)
        self._bufs = None
        self._pyramid = 0
        self._prefetched = None              # tuple of the image objects whose trunk has been computed into the next pyramid set
        self._trunk_stream = self._det_stream = None
        self._ev_trunk = torch.cuda.Event()
        self._ev_start = torch.cuda.Event()
        self._ev_box = torch.cuda.Event()
        self._ev_s0 = torch.cuda.Event()     # stage 0 of the cascade is enqueued: the memory chain and stages 1-2 part here
        self._ev_det = [None] * RESULT_SETS
        self._pyr_reader = {}
        self._slot = 0
        self._step_no = 0
        self.stats_log = None
        self.trace = None                    # diagnostics: list of (step, name, timing event), see tools/frame_schedule.py
        self.host_profile = {"frames": 0, "enqueue_s": 0.0, "materialize_s": 0.0, "wait_s": 0.0}
        if bool(cfg.MODEL.TEST_SAVE_SEMMAP):
            raise NotImplementedError("MODEL.TEST_SAVE_SEMMAP is served by the single-scene model (custom_rcnn.py:518-530)")
        R, dev, B = m.proposal_generator.cap, self.device, self.B
        rh = m.roi_heads
        self.R, self.D = R, rh.topk
        # the ROI half's buffers, B x the single-scene ones, under the same names (`ls.feat0`, `ls.prob`, `ls.boxes`, ...)
        self.roi = RoiBuffers(rh, B, lockstep=True)
        self.roi.expose_on(self)
        self.roi.proposal_pass_buffers()
        # rh.C1: the heads' vocabulary; the memory's matrix (m.C1 columns) may differ
        self.mem_scores = torch.zeros((B * R, m.C1), dtype=torch.float32, device=dev)
        self.selectors = [ops.DetectionSelector(R, rh.C1, rh.topk, dev, groups=True, batch=B) for _ in range(RESULT_SETS)]
        self.mem_selector = ops.DetectionSelector(R, m.C1, 100, dev, unique=True, batch=B)

    @property
    def plan_like_single(self) -> bool:
        """`RoiBuffers.plan_like_single`: every layer of the frame planned like ONE scene (bitwise the single-scene results)."""
        return self.roi.plan_like_single

    @plan_like_single.setter
    def plan_like_single(self, value: bool):
        self.roi.plan_like_single = bool(value)

    # nn.Module surface of the drivers
    def eval(self):
        return self

    def to(self, *_a, **_k):
        return self

    def __call__(self, episodes):
        return self.forward(episodes)

    def _mark(self, name: str, stream=None):
        if self.trace is None:
            return
        ev = torch.cuda.Event(enable_timing=True)
        ev.record(stream if stream is not None else torch.cuda.current_stream(self.device))
        self.trace.append((self._step_no, name, ev))

    # ---- buffers that depend on the frame size -----------------------------------------------------------------------------
    def _frame_buffers(self, H: int, W: int, n_cells: int):
        key = (H, W, n_cells)
        if self._bufs is not None and self._bufs["key"] == key:
            return self._bufs
        m, B, dev = self.model, self.B, self.device
        bb, pg = m.backbone, m.proposal_generator
        # the pyramid sets (level major over the scenes), the tower's buffers and the decoder are the backbone's and the proposal
        # generator's own plans for a batch of B
        plans = [bb._plan(H, W, i, B) for i in range(PYRAMID_SETS)]
        shapes, off = plans[0][:2]
        d = dict(key=key, shapes=shapes, off=off, pyr=[p[2:4] for p in plans], dec=pg._plan(shapes, off, B)[3])
        d["x"] = torch.empty((B, H, W, 4), dtype=torch.float32, device=dev)
        d["proj"] = torch.zeros((B, H, W), dtype=torch.int32, device=dev)
        d["writer"] = ops.MemoryWriter(H, W, n_cells, 100, self.R, dev, mask_thresh=0.5, batch=B)
        d["posts"] = _result_sets(B, self.D, (H, W), dev)
        self._bufs = d
        self._prefetched = None
        return d

    # ---- state -------------------------------------------------------------------------------------------------------------
    def _ensure_state(self, n_cells: int):
        if self.implicit_memory is None or self.implicit_memory.shape[1] != n_cells:
            B, dev = self.B, self.device
            self.implicit_memory = torch.zeros((B, n_cells, 512), dtype=torch.float32, device=dev)
            self.observations = torch.zeros((B, n_cells), dtype=torch.float32, device=dev)
            self._mem_f16 = torch.zeros((B, n_cells, 512), dtype=torch.float16, device=dev)
            self._dirty = torch.zeros((B, n_cells), dtype=torch.int32, device=dev)
            self._f16_valid = True
            self._dirty_pending = False
            self._started = [False] * B

    def reset_memory(self, b: int):
        """`frame['memory_reset']` branch (custom_rcnn.py:470-479) for scene b."""
        lib, s = _lib.load(), torch.cuda.current_stream(self.device).cuda_stream
        mem, obs, m16, dirty = self.implicit_memory[b], self.observations[b], self._mem_f16[b], self._dirty[b]
        _lib.check(lib.eod_fill_f32(mem.data_ptr(), 0.0, mem.numel(), s), "fill")
        _lib.check(lib.eod_fill_f32(obs.data_ptr(), 0.0, obs.numel(), s), "fill")
        _lib.check(lib.eod_fill_i32(m16.data_ptr(), 0, m16.numel() // 2, s), "fill")
        _lib.check(lib.eod_fill_i32(dirty.data_ptr(), 0, dirty.numel(), s), "fill")
        if self._last_seen is not None:
            self._last_seen[b].fill_(-1)
        if self._height_record is not None:
            for plane, v in enumerate(ops.HEIGHT_RECORD_INIT):
                self._height_record[b, plane].fill_(v)
        self._started[b] = True

    def invalidate_memory_snapshot(self):
        self._f16_valid = False

    def semantic_map(self, scene: int, classifier=None, num_classes: Optional[int] = None, thresh: Optional[float] = None,
                     scores: bool = False):
        """`CustomRCNNRecurrent.semantic_map` on scene `scene`'s state: the labels, or with `classifier` / `scores=True` the
        `(labels, scores)` of a query in any vocabulary.  Nothing of the batch model changes."""
        if not 0 <= int(scene) < self.B:
            raise IndexError(f"scene {scene} of a lock-step batch of {self.B}")
        if self.implicit_memory is None:
            raise _lib.EodError("semantic_map: no memory yet (no frame has run)")
        mem, obs, m = self.implicit_memory[int(scene)], self.observations[int(scene)], self.model
        if classifier is None and not scores:
            return ops.semmap_labels(mem, obs, m.zs_weight, m.obs_score_thresh if thresh is None else float(thresh))
        return _semmap_query(m, mem, obs, classifier, num_classes, thresh)

    def locate(self, scene: int, classes, classifier=None, num_classes: Optional[int] = None, thresh: Optional[float] = None,
               map_shape=None, radius: int = 1, topk: int = 8):
        """`CustomRCNNRecurrent.locate` on scene `scene`'s state.  Nothing of the batch model changes."""
        if not 0 <= int(scene) < self.B:
            raise IndexError(f"scene {scene} of a lock-step batch of {self.B}")
        if self.implicit_memory is None:
            raise _lib.EodError("semantic_map: no memory yet (no frame has run)")
        return _semmap_locate(self.model, self.implicit_memory[int(scene)], self.observations[int(scene)], classes, classifier,
                              num_classes, thresh, map_shape, radius, topk)

    def regions(self, scene: int, classes, classifier=None, num_classes: Optional[int] = None, thresh: Optional[float] = None,
                map_shape=None, level: float = 0.5, connectivity: int = 8, min_cells: int = 1, topk: int = 16, radius: int = 1,
                peaks: int = 8):
        """`CustomRCNNRecurrent.regions` on scene `scene`'s state.  Nothing of the batch model changes."""
        if not 0 <= int(scene) < self.B:
            raise IndexError(f"scene {scene} of a lock-step batch of {self.B}")
        if self.implicit_memory is None:
            raise _lib.EodError("semantic_map: no memory yet (no frame has run)")
        return _map_regions(self.model, self.implicit_memory[int(scene)], self.observations[int(scene)], classes, classifier,
                            num_classes, thresh, map_shape, level, connectivity, min_cells, topk, radius, peaks)

    def inventory(self, scene: Optional[int] = None, classifier=None, num_classes: Optional[int] = None, thresh: Optional[float] = None,
                  map_shape=None, level: float = 0.5, connectivity: int = 8, min_cells: int = 1, topk: int = 16, exclude=None):
        """`CustomRCNNRecurrent.inventory` on scene `scene`'s state; `scene=None`: all B scenes, queried one after the other and
        handed to the op as one [B, N] call (every entry of the dict but `status` gains a leading [B]).  Nothing of the batch model changes."""
        if scene is not None and not 0 <= int(scene) < self.B:
            raise IndexError(f"scene {scene} of a lock-step batch of {self.B}")
        if self.implicit_memory is None:
            raise _lib.EodError("semantic_map: no memory yet (no frame has run)")
        scenes = range(self.B) if scene is None else [int(scene)]
        states = [(self.implicit_memory[b], self.observations[b]) for b in scenes]
        return _map_inventory(self.model, states if scene is None else states[0], classifier, num_classes, thresh, map_shape, level,
                              connectivity, min_cells, topk, exclude)

    def describe(self, scene: int, objects, object_labels, classifier=None, num_classes: Optional[int] = None, topn: int = 5,
                 embedding=None):
        """`CustomRCNNRecurrent.describe` on scene `scene`'s memory.  Nothing of the batch model changes."""
        if not 0 <= int(scene) < self.B:
            raise IndexError(f"scene {scene} of a lock-step batch of {self.B}")
        if self.implicit_memory is None:
            raise _lib.EodError("semantic_map: no memory yet (no frame has run)")
        return _describe(self.model, self.implicit_memory[int(scene)], objects, object_labels, classifier, num_classes, topn, embedding)

    def relations(self, objects, object_labels, map_shape=None, radius: int = 2, from_cell: Optional[int] = None, topn: int = 4):
        """`CustomRCNNRecurrent.relations`; with the `[B, K]` objects and `[B, N]` object_labels of `inventory(None, ...)` the op
        runs once per scene and every entry of the dict gains a leading [B].  Nothing of the batch model changes."""
        if isinstance(object_labels, torch.Tensor) and object_labels.dim() == 2:
            objects = torch.as_tensor(objects, dtype=torch.int32, device=object_labels.device)
            if objects.dim() != 2 or objects.shape[0] != object_labels.shape[0]:
                raise _lib.EodError(f"relations: objects {tuple(objects.shape)}: expected [B, K] beside object_labels "
                                    f"{tuple(object_labels.shape)}")
            per = [_relations(objects[b].contiguous(), object_labels[b].contiguous(), map_shape, radius, from_cell, topn)
                   for b in range(int(object_labels.shape[0]))]
            return {k: torch.stack([p[k] for p in per]) for k in per[0]}
        return _relations(objects, object_labels, map_shape, radius, from_cell, topn)

    def route(self, objects, object_labels, map_shape=None, from_cell=None, passable=None, path_max: int = 256,
              sweeps: Optional[int] = None, body_radius2: Optional[int] = None):
        """`CustomRCNNRecurrent.route`; with the `[B, K]` objects and `[B, N]` object_labels of `inventory(None, ...)` the op runs
        once per scene, `from_cell` is one int or a sequence of B, and every entry of the dict gains a leading [B].  Nothing of
        the batch model changes."""
        if isinstance(object_labels, torch.Tensor) and object_labels.dim() == 2:
            B = int(object_labels.shape[0])
            objects = torch.as_tensor(objects, dtype=torch.int32, device=object_labels.device)
            if objects.dim() != 2 or objects.shape[0] != B:
                raise _lib.EodError(f"route: objects {tuple(objects.shape)}: expected [B, K] beside object_labels "
                                    f"{tuple(object_labels.shape)}")
            if isinstance(from_cell, torch.Tensor):
                from_cell = from_cell.tolist()
            cells = list(from_cell) if hasattr(from_cell, "__len__") else [from_cell] * B
            if len(cells) != B:
                raise _lib.EodError(f"route: from_cell: {len(cells)} cells for {B} scenes")
            per = [_route(objects[b].contiguous(), object_labels[b].contiguous(), map_shape, None if cells[b] is None else int(cells[b]),
                          passable, path_max, sweeps, body_radius2) for b in range(B)]
            return {k: torch.stack([p[k] for p in per]) for k in per[0]}
        return _route(objects, object_labels, map_shape, from_cell, passable, path_max, sweeps, body_radius2)

    def clearance(self, objects, object_labels, map_shape=None, radius2: int = 0, keep_cell=None, passable=None):
        """`CustomRCNNRecurrent.clearance`; with the `[B, K]` objects and `[B, N]` object_labels of `inventory(None, ...)` the op
        runs once per scene, `keep_cell` is None, one int or a sequence of B, and every entry of the dict gains a leading [B].
        Nothing of the batch model changes."""
        if isinstance(object_labels, torch.Tensor) and object_labels.dim() == 2:
            B = int(object_labels.shape[0])
            objects = torch.as_tensor(objects, dtype=torch.int32, device=object_labels.device)
            if objects.dim() != 2 or objects.shape[0] != B:
                raise _lib.EodError(f"clearance: objects {tuple(objects.shape)}: expected [B, K] beside object_labels "
                                    f"{tuple(object_labels.shape)}")
            if isinstance(keep_cell, torch.Tensor):
                keep_cell = keep_cell.tolist()
            cells = list(keep_cell) if hasattr(keep_cell, "__len__") else [keep_cell] * B
            if len(cells) != B:
                raise _lib.EodError(f"clearance: keep_cell: {len(cells)} cells for {B} scenes")
            per = [_clearance(objects[b].contiguous(), object_labels[b].contiguous(), map_shape, radius2,
                              None if cells[b] is None else int(cells[b]), passable) for b in range(B)]
            return {k: torch.stack([p[k] for p in per]) for k in per[0]}
        return _clearance(objects, object_labels, map_shape, radius2, keep_cell, passable)

    def sight(self, objects, object_labels, map_shape=None, from_cells=None, range2: Optional[int] = None, passable=None):
        """`CustomRCNNRecurrent.sight`; with the `[B, K]` objects and `[B, N]` object_labels of `inventory(None, ...)` the op runs
        once per scene, `from_cells` is [B, S] (a tensor or a sequence of B sequences), and every entry of the dict gains a leading
        [B].  Nothing of the batch model changes."""
        if isinstance(object_labels, torch.Tensor) and object_labels.dim() == 2:
            B = int(object_labels.shape[0])
            objects = torch.as_tensor(objects, dtype=torch.int32, device=object_labels.device)
            if objects.dim() != 2 or objects.shape[0] != B:
                raise _lib.EodError(f"sight: objects {tuple(objects.shape)}: expected [B, K] beside object_labels "
                                    f"{tuple(object_labels.shape)}")
            if isinstance(from_cells, torch.Tensor):
                from_cells = from_cells.tolist()
            rows = list(from_cells) if hasattr(from_cells, "__len__") else None
            if rows is None or len(rows) != B or any(not hasattr(r, "__len__") or len(r) != len(rows[0]) for r in rows):
                raise _lib.EodError(f"sight: from_cells: expected [B, S] cells for the {B} scenes")
            per = [_sight(objects[b].contiguous(), object_labels[b].contiguous(), map_shape, [int(v) for v in rows[b]], range2, passable)
                   for b in range(B)]
            return {k: torch.stack([p[k] for p in per]) for k in per[0]}
        return _sight(objects, object_labels, map_shape, from_cells, range2, passable)

    def cover(self, scene: int, proj_indices, stamp: Optional[int] = None, exclude_cell: int = -1):
        """`CustomRCNNRecurrent.cover` for scene `scene`: the record is int32 [B, N], a row per scene with a stamp counter of its
        own, made at the first call and cleared to -1 for a scene by its `reset_memory`; the scene's counter goes on across a reset, so a
        stamp never repeats and `since=` the stamp of the first call after the reset asks for what was covered since.  Returns the
        scene's row."""
        if not 0 <= int(scene) < self.B:
            raise IndexError(f"scene {scene} of a lock-step batch of {self.B}")
        if self.implicit_memory is None:
            raise _lib.EodError("cover: no memory yet (no frame has run)")
        b, n_cells = int(scene), int(self.implicit_memory.shape[1])
        if self._last_seen is None or self._last_seen.shape[1] != n_cells:
            self._last_seen = torch.full((self.B, n_cells), -1, dtype=torch.int32, device=self.device)
        if stamp is None:
            stamp = self._cover_stamp[b]
        row = _cover(self.model, proj_indices, self._last_seen[b], n_cells, stamp, exclude_cell)
        self._cover_stamp[b] = max(self._cover_stamp[b], int(stamp) + 1)
        return row

    def frontiers(self, object_labels, map_shape=None, since: int = 0, last_seen=None, from_cell=None, route=None, passable=None,
                  min_cells: int = 2, topk: int = 16, rank_by="behind", scene: Optional[int] = None):
        """`CustomRCNNRecurrent.frontiers`; with the `[B, N]` object_labels of `inventory(None, ...)` the op runs once per scene
        and every entry of the dict gains a leading [B]: `last_seen` is [B, N] (None: the record `cover` keeps, or
        `observations > 0` where it was never called), `from_cell` None, one int or a sequence of B, `route` None or a sequence of
        the B dicts of `route` (or one dict whose `dist` is [B, N]).  With object_labels [N], `scene` picks the scene whose record
        to take.  Nothing of the batch model changes."""
        if last_seen is None:
            last_seen = self._last_seen
            if last_seen is None and self.observations is not None:
                last_seen = _observed(self.observations)
        if isinstance(object_labels, torch.Tensor) and object_labels.dim() == 2:
            B = int(object_labels.shape[0])
            if not isinstance(last_seen, torch.Tensor) or last_seen.dim() != 2 or last_seen.shape[0] != B:
                raise _lib.EodError(f"frontiers: last_seen {tuple(getattr(last_seen, 'shape', ()))}: expected [B, N] beside object_labels "
                                    f"{tuple(object_labels.shape)}")
            cells = list(from_cell) if hasattr(from_cell, "__len__") else [from_cell] * B
            if isinstance(route, dict):
                routes = [route["dist"][b].contiguous() for b in range(B)]
            else:
                routes = list(route) if route is not None else [None] * B
            if len(cells) != B or len(routes) != B:
                raise _lib.EodError(f"frontiers: from_cell and route: expected one entry for each of the {B} scenes")
            per = [_frontiers(object_labels[b].contiguous(), map_shape, last_seen[b].contiguous(), since,
                              None if cells[b] is None else int(cells[b]), routes[b], passable, min_cells, topk, rank_by) for b in range(B)]
            return {k: torch.stack([p[k] for p in per]) for k in per[0]}
        if isinstance(last_seen, torch.Tensor) and last_seen.dim() == 2:
            if scene is None or not 0 <= int(scene) < last_seen.shape[0]:
                raise _lib.EodError(f"frontiers: object_labels [N] beside a record of {last_seen.shape[0]} scenes: pass scene=")
            last_seen = last_seen[int(scene)].contiguous()
        return _frontiers(object_labels, map_shape, last_seen, since, from_cell, route, passable, min_cells, topk, rank_by)

    def heights(self, scene: int, proj_indices, heights, band_mm=(100, 1500), exclude_cell: int = -1):
        """`CustomRCNNRecurrent.heights` for scene `scene`: the record is int32 [B, 4, N], a row per scene, made at the first call
        and emptied for a scene by its `reset_memory`.  Returns the scene's row [4, N]."""
        if not 0 <= int(scene) < self.B:
            raise IndexError(f"scene {scene} of a lock-step batch of {self.B}")
        if self.implicit_memory is None:
            raise _lib.EodError("heights: no memory yet (no frame has run)")
        b, n_cells = int(scene), int(self.implicit_memory.shape[1])
        if self._height_record is None or self._height_record.shape[2] != n_cells:
            self._height_record = torch.stack([ops.new_height_record(n_cells, self.device) for _ in range(self.B)])
        return _heights(self.model, proj_indices, heights, self._height_record[b], n_cells, band_mm, exclude_cell)

    def obstacles(self, object_labels=None, objects=None, map_shape=None, record=None, min_hits: int = 4, min_cells: int = 2,
                  topk: int = 16, scene: Optional[int] = None):
        """`CustomRCNNRecurrent.obstacles` (`merged_labels`, `kind`, ...); `record` None takes the [B, 4, N] record `heights` keeps.  With the `[B, N]`
        object_labels (and `[B, K]` objects) of `inventory(None, ...)`, or with neither and no `scene`, the op runs once per scene
        and every entry of the dict gains a leading [B].  With object_labels [N] or None, `scene` picks the scene whose record to
        take.  Nothing of the batch model changes."""
        if record is None:
            record = self._height_record
        if record is None:
            raise _lib.EodError("obstacles: no height record: call heights(scene, proj_indices, heights) on every frame, or pass record")
        batched = isinstance(object_labels, torch.Tensor) and object_labels.dim() == 2
        if batched or (object_labels is None and scene is None and isinstance(record, torch.Tensor) and record.dim() == 3):
            if not isinstance(record, torch.Tensor) or record.dim() != 3 or (batched and record.shape[0] != object_labels.shape[0]):
                raise _lib.EodError(f"obstacles: record {tuple(getattr(record, 'shape', ()))}: expected [B, 4, N] beside object_labels "
                                    f"{tuple(getattr(object_labels, 'shape', ()))}")
            B = int(record.shape[0])
            if objects is not None:
                objects = torch.as_tensor(objects, dtype=torch.int32, device=record.device)
                if objects.dim() != 2 or objects.shape[0] != B:
                    raise _lib.EodError(f"obstacles: objects {tuple(objects.shape)}: expected [B, K] for the {B} scenes")
            per = [_obstacles(record[b], map_shape, object_labels[b].contiguous() if batched else None,
                              None if objects is None else objects[b].contiguous(), min_hits, min_cells, topk) for b in range(B)]
            return {k: torch.stack([p[k] for p in per]) for k in per[0]}
        if isinstance(record, torch.Tensor) and record.dim() == 3:
            if scene is None or not 0 <= int(scene) < record.shape[0]:
                raise _lib.EodError(f"obstacles: object_labels [N] beside a record of {record.shape[0]} scenes: pass scene=")
            record = record[int(scene)]
        return _obstacles(record, map_shape, object_labels, objects, min_hits, min_cells, topk)

    def rooms(self, labels, objects=None, map_shape=None, door_r2: Optional[int] = None, min_cells: Optional[int] = None,
              topk: int = 16, passable=None, known=None, clearance=None, sweeps: Optional[int] = None):
        """`CustomRCNNRecurrent.rooms` (`room_labels`, `room`, `door_cell`, `obj_room`, ...); with the `[B, N]` labels of
        `obstacles` (and `[B, K]` objects, `[B, N]` known, and a clearance whose `d2` is [B, N]) the op runs once per scene and
        every entry of the dict gains a leading [B].  Nothing of the batch model changes."""
        if isinstance(labels, torch.Tensor) and labels.dim() == 2:
            return _rooms_batched("rooms", labels, objects, map_shape, door_r2, min_cells, topk, passable, known, clearance, sweeps)
        return _rooms(labels, objects, map_shape, door_r2, min_cells, topk, passable, known, clearance, sweeps)

    def place(self, scene: int, instances, proj_indices, topk: int = 4, exclude_cell: int = -1, attach: bool = False):
        """`CustomRCNNRecurrent.place` with scene `scene`'s cell count.  Nothing of the batch model changes."""
        if not 0 <= int(scene) < self.B:
            raise IndexError(f"scene {scene} of a lock-step batch of {self.B}")
        mem = None if self.implicit_memory is None else self.implicit_memory[int(scene)]
        return _place(self.model, mem, instances, proj_indices, topk, exclude_cell, attach)

    def _refresh_snapshot(self):
        """a4 + fp16 cast for the B tables: they are one [B*N,512] table to the kernels."""
        mem, obs = self.implicit_memory.view(-1, 512), self.observations.view(-1)
        m16, dirty = self._mem_f16.view(-1, 512), self._dirty.view(-1)
        if self._f16_valid:
            if self._dirty_pending:
                ops.memory_normalize_dirty_f16(mem, obs, dirty, m16)
        else:
            ops.memory_normalize_f16(mem, obs, out=m16)
            _lib.check(_lib.load().eod_fill_i32(dirty.data_ptr(), 0, dirty.numel(), torch.cuda.current_stream().cuda_stream), "fill")
            self._f16_valid = True
        self._dirty_pending = False

    # ---- the memory-independent half -----------------------------------------------------------------------------------------
    def _trunk(self, frames: List[dict], H: int, W: int, which: int):
        """preprocess + ResNet-50 + FPN top-down for the B images, N = B, into pyramid set `which` (level-major views)."""
        m, B, d = self.model, self.B, self._bufs
        bb = m.backbone
        x = d["x"]
        for b, f in enumerate(frames):
            ops.preprocess_image(m._device_image(f), m.pixel_mean, m.pixel_std, out=x[b:b + 1])
        c = bb.bottom_up.forward(x, H, W, N=B, plan_like_single=self.plan_like_single)
        bb.top_down(c, B, d["pyr"][which][1], planned=self.plan_like_single)

    def _enqueue_trunk_ahead(self, frames: List[dict], H: int, W: int):
        if self._trunk_stream is None:
            self._trunk_stream = _sched_streams(self.device)[1]
        ts = self._trunk_stream
        nxt = (self._pyramid + 1) % PYRAMID_SETS
        ts.wait_event(self._ev_start)
        if nxt in self._pyr_reader:
            ts.wait_event(self._pyr_reader[nxt])            # a trailing detection pass may still read that set
        with torch.cuda.stream(ts):
            self._mark("trunk_lookahead_begin", ts)
            self._trunk(frames, H, W, nxt)
            self._ev_trunk.record(ts)
            self._mark("trunk_lookahead", ts)
        self._prefetched = tuple(id(f["image"]) for f in frames)

    # ---- one step: one frame of every scene ----------------------------------------------------------------------------------
    def set_classifier_width(self) -> None:
        """The heads' class matrix changed width (`reset_cls_test`): the batch's score buffer and detection selectors follow it.
        The memory side (`mem_scores`, `mem_selector`, the tables) is not touched."""
        rh, B = self.model.roi_heads, self.B
        torch.cuda.synchronize(self.device)           # results of earlier steps still read the old selectors' buffers
        self.roi.set_width(rh.C1)
        self.roi.expose_on(self)
        self.selectors = [ops.DetectionSelector(self.R, rh.C1, rh.topk, self.device, groups=True, batch=B) for _ in range(RESULT_SETS)]

    def _step(self, frames: List[dict], active: List[bool], refresh: bool, next_frames: Optional[List[dict]], trailing: bool):
        m, B, dev = self.model, self.B, self.device
        bb, pg, rh = m.backbone, m.proposal_generator, m.roi_heads
        H, W = int(frames[0]["image"].shape[-2]), int(frames[0]["image"].shape[-1])
        if H % 32 or W % 32:
            raise ValueError("H and W must be multiples of 32 (proj_indices is not padded: SURVEY §8 notation)")
        if any((int(f["image"].shape[-2]), int(f["image"].shape[-1])) != (H, W) for f in frames):
            raise ValueError("the frames of one lock-step must have one size")
        n_cells = self.implicit_memory.shape[1]
        d = self._frame_buffers(H, W, n_cells)
        cur = torch.cuda.current_stream(dev)
        R, g = self.R, self.roi
        if self.prob.shape[1] != rh.C1:               # `reset_cls_test` on the model since the last step: follow the heads' width
            self.set_classifier_width()
        self._step_no += 1
        self._mark("start")
        # The previous step's stages 1-2 and detection selection run on the side stream.  They read the proposal decoder's boxes,
        # scores and count (one buffer set, rewritten by this step's decode) and the cascade's buffers (rewritten by this step's
        # stage 0): the step's stream joins them before anything of this step is enqueued.  They are long over by then.
        cur.wait_event(self._ev_box)
        for b, f in enumerate(frames):
            p = m._device_proj(f)
            if tuple(p.shape) != (H, W):
                raise ValueError(f"proj_indices shape {tuple(p.shape)} != image {(H, W)}")
            d["proj"][b].copy_(p, non_blocking=True)
        use_mem = m.memory_type == "implicit_memory"
        if use_mem and refresh:
            self._refresh_snapshot()

        key = tuple(id(f["image"]) for f in frames)
        had_ahead = self._prefetched is not None
        hit = had_ahead and self._prefetched == key
        self._prefetched = None
        if had_ahead:
            cur.wait_event(self._ev_trunk)                      # used or not, it must be over before any set is touched
        self._pyramid = (self._pyramid + 1) % PYRAMID_SETS
        which = self._pyramid
        if not hit:
            if which in self._pyr_reader:
                cur.wait_event(self._pyr_reader[which])
            self._trunk(frames, H, W, which)
        look = next_frames is not None and self.trunk_lookahead
        if look:
            self._ev_start.record(cur)

        # memory read + fusion (timm.py:142-192), P6 / P7 (timm.py:359-364); CenterNet tower + proposals (centernet_head.py:141-161,
        # centernet.py:603-745)
        planned = self.plan_like_single
        feats, views, shapes, off = bb.fuse_memory_and_top(H, W, self._mem_f16, d["proj"], which, self._err, batch=B, planned=planned)
        prop_boxes, prop_scores, prop_count = pg.forward(feats, shapes, off, batch=B, planned=planned)
        self._mark("proposals")
        if look:
            self._enqueue_trunk_ahead(next_frames, H, W)

        # cascade (detic_roi_heads.py:88-222)
        k = self._slot
        if self._ev_det[k] is not None:
            cur.wait_event(self._ev_det[k])                     # detection list set k is still read by the pass of RESULT_SETS steps ago
        # Stage 0 on the step's stream; everything the memory side reads (`featn0`, `mem_scores`, the proposal boxes) is final behind
        # it and stages 1-2 write none of it, so the step's critical chain (memory selection -> proposal masks -> memory write) goes on
        # from here while stages 1-2 and the detection selection, which only the detections need, run beside it on the side stream.
        # The memory update's CLIP re-score: for every MEMORY_TYPE, as in the reference (custom_rcnn.py:515,573); in stage 0's launch
        # when both class matrices are narrow and equally wide, else a launch per scene behind it.
        cascade = (views, shapes, prop_boxes, prop_scores, prop_count, (H, W), (m.zs_weight, self.mem_scores))
        carry = rh._cascade(*cascade, part=range(0, 1), g=g)
        self._ev_s0.record(cur)
        if not rh.fuses_mem_rescore(m.zs_weight):
            for b in range(B):
                ops.memory_scores(self.featn0[b * R:(b + 1) * R], m.zs_weight, prop_scores[b * R:(b + 1) * R],
                                  self.mem_scores[b * R:(b + 1) * R], prop_count[b:b + 1], R, m.C1)
        # memory selection first: the step's critical chain waits for it (custom_rcnn.py:825-875)
        msel = self.mem_selector
        _, _, _, mem_rows, mem_cnt = msel(prop_boxes, self.mem_scores, prop_count, float(W), float(H), m.cls_score_thresh, 0.5)
        for b in range(B):
            if not active[b]:                               # idle slot: no instances -> its state stays as it is
                s_raw = torch.cuda.current_stream(dev).cuda_stream
                _lib.check(_lib.load().eod_fill_i32(mem_cnt[b:b + 1].data_ptr(), 0, 1, s_raw), "fill")
                _lib.check(_lib.load().eod_fill_i32(msel.uniq_count[b:b + 1].data_ptr(), 0, 1, s_raw), "fill")
        self._mark("cascade+mem_select")
        side = _sched_streams(dev)[0]
        side.wait_event(self._ev_s0)
        sel = self.selectors[k]
        with torch.cuda.stream(side):
            boxes, _ = rh._cascade(*cascade, part=range(1, rh.num_stages), carry=carry, g=g)
            sel(boxes, self.prob, prop_count, float(W), float(H), rh.score_thresh, rh.nms_thresh)
            self._ev_box.record(side)
            self._mark("cascade+det_select", side)

        # detection mask pass + post-processing + paste (detic_roi_heads.py:257, custom_rcnn.py:579-580)
        post = d["posts"][k]
        det_pass = (g, views, shapes, sel, k, post, (H, W), m.mask_threshold, m.dedup_detection_masks, 0, ("det", self._step_no))
        if self.trail_detection_pass:
            if self._det_stream is None:
                self._det_stream = _det_stream(dev)
                self._ev_det = [torch.cuda.Event() for _ in range(RESULT_SETS)]
            ds = self._det_stream
            ds.wait_event(self._ev_box)
            with torch.cuda.stream(ds):
                self._mark("det_pass_begin", ds)
                rh.detection_pass(*det_pass)
                self._ev_det[k].record(ds)
                self._mark("det_pass", ds)
            self._pyr_reader[which] = self._ev_det[k]
        else:
            cur.wait_event(self._ev_box)
            rh.detection_pass(*det_pass)

        # mask head on the memory instances of all scenes (custom_rcnn.py:573-574, only the proposals 875-880 read), memory write
        rh.forward_mask_memory(views, shapes, prop_boxes, prop_count, rows=msel.uniq_rows, rows_count=msel.uniq_count,
                               bufs=g.proposal_pass_buffers(), tag=("prop", self._step_no), g=g, lds_reserve=0)
        self._mark("prop_masks")
        follow = m.snapshot_follows_write if m.snapshot_follows_write is not None else m.test_type in ("default", "episodic")
        wr = d["writer"]
        if follow and self._f16_valid and not self._dirty_pending:
            wr(self.featn0, prop_boxes, self.prop_masks, mem_rows, mem_cnt, d["proj"], self.implicit_memory, self.observations,
               err=self._err, snapshot=self._mem_f16)
        else:
            wr(self.featn0, prop_boxes, self.prop_masks, mem_rows, mem_cnt, d["proj"], self.implicit_memory, self.observations,
               dirty=self._dirty, err=self._err)
            self._dirty_pending = True
        self._mark("mem_write")
        if self.trail_detection_pass and not trailing:
            cur.wait_event(self._ev_det[k])
        if self.stats_log is not None:
            if self.trail_detection_pass:
                with torch.cuda.stream(self._det_stream):
                    cnt = post["count"].clone()
            else:
                cnt = post["count"].clone()
            self.stats_log.append((prop_count.clone(), cnt, d["writer"].k_out.clone(), msel.uniq_count.clone(), sel.rep_count.clone()))
        # async read-back of the step's detection counts; flips the result set
        self._slot = (self._slot + 1) % RESULT_SETS
        return _ticket(post, self._err, cur, self._det_stream if self.trail_detection_pass else None)

    # ---- forward ---------------------------------------------------------------------------------------------------------------
    def forward(self, episodes: List[Optional[List[dict]]]):
        B, m = self.B, self.model
        if len(episodes) != B:
            raise ValueError(f"need {B} episodes (None for a sequence that sits this call out)")
        episodes = [e if e else [] for e in episodes]
        T = max(len(e) for e in episodes)
        outs: List[List[dict]] = [[] for _ in range(B)]
        if T == 0:
            return outs
        first = next(e[0] for e in episodes if e)
        self._ensure_state(int(first["memory"].shape[0]))
        # the step's chain runs on the process-wide high-priority chain stream; the caller's stream is joined on both sides
        caller = torch.cuda.current_stream(self.device)
        ms = _sched_streams(self.device)[2]
        ev_in, ev_out = torch.cuda.Event(), torch.cuda.Event()
        ev_in.record(caller)
        ms.wait_event(ev_in)
        idle = dict(image=first["image"], proj_indices=first["proj_indices"])

        def frames_at(t):
            fr, act = [], []
            for b in range(B):
                e = episodes[b]
                act.append(t < len(e))
                fr.append(e[t] if t < len(e) else (e[-1] if e else idle))
            return fr, act

        def hand_out(post, act):
            insts = _instances(post, self._err, self.host_profile, self.implicit_memory.shape[1], self.device, act)
            for b, inst in enumerate(insts):
                if inst is not None:
                    outs[b].append({"instances": inst})

        pending = []
        with torch.cuda.stream(ms):
            for t in range(T):
                frames, active = frames_at(t)
                t0 = _time.perf_counter()
                for b in range(B):
                    if active[b] and frames[b]["memory_reset"]:
                        if int(episodes[b][0]["memory"].shape[0]) != self.implicit_memory.shape[1]:
                            raise ValueError("the scenes of one lock-step must have one memory size")
                        self.reset_memory(b)
                    if active[b] and not self._started[b]:
                        raise RuntimeError("first frame of a scene must carry memory_reset=True (custom_rcnn.py:485 reads unset state)")
                refresh = m.test_type in ("default", "episodic") or (m.test_type == "longterm" and t == 0)
                nxt = frames_at(t + 1)[0] if t + 1 < T else None
                pending.append((self._step(frames, active, refresh, nxt, trailing=t + 1 < T), active))
                t1 = _time.perf_counter()
                if len(pending) == RESULT_SETS:
                    hand_out(*pending.pop(0))
                hp = self.host_profile
                hp["frames"] += sum(active)
                hp["enqueue_s"] += t1 - t0
                hp["materialize_s"] += _time.perf_counter() - t1
            for post, act in pending:
                hand_out(post, act)
            ev_out.record(ms)
        caller.wait_event(ev_out)
        return outs
