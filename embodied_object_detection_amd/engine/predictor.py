"""Single-frame predictor of the robot demo (`EmbodiedPredictor`, `Detic/detic/predictor.py:389-439`).

Same call shape: `pred(data)` with `data = {"image": HWC uint8, "memory", "proj_indices", "memory_reset", "sequence_name"}` ->
`{"instances": Instances}`; like the reference it reverses the channel order when `INPUT.FORMAT == "RGB"` (`:421-423`: the
detectron2 predictor convention of BGR inputs), keeps `height` / `width` of the original image and runs
`model([[inputs]])[0]`.  `ResizeShortestEdge([480, 480], INPUT.MAX_SIZE_TEST)` (`:402-404`) is the identity for the 480 x 640
frames of this path; any other size is refused, because the reference resizes the image but not `proj_indices` and then fails
inside the memory fusion (SURVEY §8 notation).
"""
from __future__ import annotations

from typing import Dict, Optional

import numpy as np
import torch


# `--vocabulary` of the reference's predictor (predictor.py:33-37): CLIP text matrices under datasets/metadata/
BUILDIN_CLASSIFIER = {
    "lvis": "datasets/metadata/lvis_v1_clip_a+cname.npy",
    "objects365": "datasets/metadata/o365_clip_a+cnamefix.npy",
    "openimages": "datasets/metadata/oid_clip_a+cname.npy",
    "coco": "datasets/metadata/coco_clip_a+cname.npy",
    "mp3d": "datasets/metadata/mp3d_clip.npy",
}


def resolve_vocabulary(vocabulary: str) -> str:
    """File of a built-in vocabulary: the reference's relative path if it exists from the working directory, else the copy under the
    package's `metadata/` (as `setup_cfg` resolves ZEROSHOT_WEIGHT_PATH).  Only `mp3d_clip.npy` ships with the package."""
    import os
    if vocabulary == "custom":
        raise ValueError("vocabulary='custom' needs classifier=<[C, 512] .npy path or [512, C] tensor>: computing CLIP text embeddings "
                         "from class names needs the downloaded CLIP weights and is out of scope here")
    if vocabulary not in BUILDIN_CLASSIFIER:
        raise ValueError(f"vocabulary {vocabulary!r}: expected one of {sorted(BUILDIN_CLASSIFIER)} or 'custom'")
    rel = BUILDIN_CLASSIFIER[vocabulary]
    if os.path.exists(rel):
        return rel
    cand = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "metadata", os.path.basename(rel))
    if os.path.exists(cand):
        return cand
    raise FileNotFoundError(f"vocabulary {vocabulary!r}: neither {rel} nor {cand} exists")


class EmbodiedPredictor:
    def __init__(self, cfg, state_dict: Optional[Dict[str, torch.Tensor]] = None, vocabulary: Optional[str] = None, classifier=None):
        """`vocabulary`: lvis / objects365 / openimages / coco / mp3d (predictor.py:183-231); `classifier`: a `[C, 512]` .npy path
        or a `[512, C]` tensor (what the reference calls `custom`).  Either one swaps the heads' classifier of the built model
        (`reset_cls_test`); neither keeps the configuration's."""
        from .. import build_model
        self.cfg = cfg
        if vocabulary is not None and classifier is None:
            classifier = resolve_vocabulary(vocabulary)
        self.model = build_model(cfg, state_dict)          # loads cfg.MODEL.WEIGHTS like DetectionCheckpointer (:399-400)
        if classifier is not None:
            from ..modeling.utils import reset_cls_test
            if isinstance(classifier, torch.Tensor):
                num_classes = int(classifier.shape[1])
            else:
                num_classes = int(np.load(classifier, mmap_mode="r").shape[0])
            reset_cls_test(self.model, classifier, num_classes)
        self.input_format = cfg.INPUT.FORMAT
        assert self.input_format in ("RGB", "BGR"), self.input_format
        self.max_size = int(cfg.INPUT.MAX_SIZE_TEST)

    def semantic_map(self, vocabulary: Optional[str] = None, classifier=None, thresh: Optional[float] = None) -> Dict:
        """The spatial memory as it stands, read as a map: `{"labels": int32 [N], "scores": float32 [N]}`, per cell the most likely
        class (-1 below `thresh`; None: MEMORY_OBS_SCORE_THRESH) and its softmax probability.  `vocabulary` / `classifier` as in the
        constructor; neither: the memory's own class matrix.  The model, its heads and the memory are left as they are."""
        if vocabulary is not None and classifier is None:
            classifier = resolve_vocabulary(vocabulary)
        labels, scores = self.model.semantic_map(classifier=classifier, thresh=thresh, scores=True)
        return {"labels": labels, "scores": scores}

    def locate(self, classes, vocabulary: Optional[str] = None, classifier=None, thresh: Optional[float] = None, map_shape=None,
               radius: int = 1, topk: int = 8) -> Dict:
        """Where on the map the queried classes are: the dict of `CustomRCNNRecurrent.locate` (`labels`, `scores`, `prob`, `peaks`,
        `peak_scores`).  `classes`: indices into the vocabulary that `vocabulary` / `classifier` name as in the constructor;
        neither: the memory's own class matrix.  The model, its heads and the memory are left as they are."""
        if vocabulary is not None and classifier is None:
            classifier = resolve_vocabulary(vocabulary)
        return self.model.locate(classes, classifier=classifier, thresh=thresh, map_shape=map_shape, radius=radius, topk=topk)

    def regions(self, classes, vocabulary: Optional[str] = None, classifier=None, thresh: Optional[float] = None, map_shape=None,
                level: float = 0.5, connectivity: int = 8, min_cells: int = 1, topk: int = 16, radius: int = 1, peaks: int = 8) -> Dict:
        """The map objects of the queried classes: the dict of `CustomRCNNRecurrent.regions`; `classes`, `vocabulary` and
        `classifier` as in `locate`.  The model, its heads and the memory are left as they are."""
        if vocabulary is not None and classifier is None:
            classifier = resolve_vocabulary(vocabulary)
        return self.model.regions(classes, classifier=classifier, thresh=thresh, map_shape=map_shape, level=level,
                                  connectivity=connectivity, min_cells=min_cells, topk=topk, radius=radius, peaks=peaks)

    def inventory(self, vocabulary: Optional[str] = None, classifier=None, thresh: Optional[float] = None, map_shape=None,
                  level: float = 0.5, connectivity: int = 8, min_cells: int = 1, topk: int = 16, exclude=None) -> Dict:
        """What the map holds, all classes at once: the dict of `CustomRCNNRecurrent.inventory`; `vocabulary` and `classifier` as in
        `semantic_map`.  The model, its heads and the memory are left as they are."""
        if vocabulary is not None and classifier is None:
            classifier = resolve_vocabulary(vocabulary)
        return self.model.inventory(classifier=classifier, thresh=thresh, map_shape=map_shape, level=level, connectivity=connectivity,
                                    min_cells=min_cells, topk=topk, exclude=exclude)

    def describe(self, objects, object_labels, vocabulary: Optional[str] = None, classifier=None, topn: int = 5, embedding=None) -> Dict:
        """What the map objects are, each as a whole: the dict of `CustomRCNNRecurrent.describe` (`embedding`, `coherence`, `prob`,
        `top_cls`, `top_prob`, ...) for the objects of an `inventory`; `vocabulary` and `classifier` as in `semantic_map`.  The model,
        its heads and the memory are left as they are."""
        if vocabulary is not None and classifier is None:
            classifier = resolve_vocabulary(vocabulary)
        return self.model.describe(objects, object_labels, classifier=classifier, topn=topn, embedding=embedding)

    def relations(self, objects, object_labels, map_shape=None, radius: int = 2, from_cell: Optional[int] = None, topn: int = 4) -> Dict:
        """How the map objects stand to each other and to one cell: the dict of `CustomRCNNRecurrent.relations` (`min_d2`, `closest`,
        `near_cells`, `edges`, `cells`, `nearest`, `from_d2`, `from_closest`, ...) for the objects of an `inventory` on the grid
        `map_shape` = (rows, cols).  The model, its heads and the memory are neither read nor changed."""
        return self.model.relations(objects, object_labels, map_shape=map_shape, radius=radius, from_cell=from_cell, topn=topn)

    def route(self, objects, object_labels, map_shape=None, from_cell: Optional[int] = None, passable=None, path_max: int = 256,
              sweeps: Optional[int] = None, body_radius2: Optional[int] = None) -> Dict:
        """How to reach the map objects: the dict of `CustomRCNNRecurrent.route` (`dist`, `parent`, `goal_cost`, `goal_cell`, `path`,
        `path_cells`, `cells`, `counts`, ...) for the objects of an `inventory` on the grid `map_shape` = (rows, cols), from
        `from_cell`; with `body_radius2` for a body of that squared radius in cells, on the inflated map (`clearance_d2` and
        `inflated_labels` are added).  The model, its heads and the memory are neither read nor changed."""
        return self.model.route(objects, object_labels, map_shape=map_shape, from_cell=from_cell, passable=passable, path_max=path_max,
                                sweeps=sweeps, body_radius2=body_radius2)

    def clearance(self, objects, object_labels, map_shape=None, radius2: int = 0, keep_cell: Optional[int] = None, passable=None) -> Dict:
        """How much room there is round the map objects: the dict of `CustomRCNNRecurrent.clearance` (`d2`, `nearest`, `owner`,
        `inflated`, `cells`, `territory`, `widest_d2`, `widest_cell`, `open_key`, `counts`, ...) for the objects of an `inventory` on
        the grid `map_shape` = (rows, cols).  The model, its heads and the memory are neither read nor changed."""
        return self.model.clearance(objects, object_labels, map_shape=map_shape, radius2=radius2, keep_cell=keep_cell, passable=passable)

    def sight(self, objects, object_labels, map_shape=None, from_cells=None, range2: Optional[int] = None, passable=None) -> Dict:
        """What can be seen from where: the dict of `CustomRCNNRecurrent.sight` (`seen_mask`, `seen_cells`, `near_d2`, `near_cell`,
        `best_seen`, `best_source`, `source_counts`, `counts`, ...) for the objects of an `inventory` on the grid `map_shape` =
        (rows, cols), from up to 64 candidate cells `from_cells` within the squared range `range2` (None: unbounded).  The model,
        its heads and the memory are neither read nor changed."""
        return self.model.sight(objects, object_labels, map_shape=map_shape, from_cells=from_cells, range2=range2, passable=passable)

    def cover(self, data: Dict, stamp: Optional[int] = None, exclude_cell: int = -1):
        """Record what the camera covered in the frame `data` (the dict the predictor was called with): `CustomRCNNRecurrent.cover`
        on `data["proj_indices"]`.  Returns `last_seen` int32 [N].  Nothing the frame computes changes."""
        return self.model.cover(data["proj_indices"], stamp=stamp, exclude_cell=exclude_cell)

    def frontiers(self, object_labels, map_shape=None, since: int = 0, last_seen=None, from_cell: Optional[int] = None, route=None,
                  passable=None, min_cells: int = 2, topk: int = 16, rank_by="behind") -> Dict:
        """Where the known space ends and what lies beyond: the dict of `CustomRCNNRecurrent.frontiers` (`frontier`, `area`,
        `behind_area`, `reach_cell`, `reach_cost`, `frontier_labels`, `unknown_labels`, `counts`, ...) for the label map of an
        `inventory` on the grid `map_shape` = (rows, cols), from the record `cover` keeps (`last_seen` None) or the `last_seen` given.  The model,
        its heads and the memory are not changed."""
        return self.model.frontiers(object_labels, map_shape=map_shape, since=since, last_seen=last_seen, from_cell=from_cell,
                                    route=route, passable=passable, min_cells=min_cells, topk=topk, rank_by=rank_by)

    def heights(self, data: Dict, band_mm=(100, 1500), exclude_cell: int = -1):
        """Record how high the things under the camera stand in the frame `data` (the dict the predictor was called with, made with
        `RobotFrontEnd.frame(..., heights=True)`): `CustomRCNNRecurrent.heights` on `data["proj_indices"]` and `data["heights"]`.
        Returns the height record int32 [4, N].  Nothing the frame computes changes."""
        if "heights" not in data:
            from .. import _lib
            raise _lib.EodError("heights: the frame carries no \"heights\" (RobotFrontEnd.frame(..., heights=True))")
        return self.model.heights(data["proj_indices"], data["heights"], band_mm=band_mm, exclude_cell=exclude_cell)

    def obstacles(self, object_labels=None, objects=None, map_shape=None, record=None, min_hits: int = 4, min_cells: int = 2,
                  topk: int = 16) -> Dict:
        """What stands in the way, from the heights alone, merged with the detected objects: the dict of
        `CustomRCNNRecurrent.obstacles` (`merged_labels`, `kind`, `structure_labels`, `structure`, `area`, `top_mm`, `obj_top_mm`,
        `counts`, ...) on the grid `map_shape` = (rows, cols), from the record `heights` keeps (`record` None) or the one given;
        `route`, `clearance`, `sight` and `frontiers` take `merged_labels` in place of `object_labels`.  The model, its heads and
        the memory are not changed."""
        return self.model.obstacles(object_labels, objects, map_shape=map_shape, record=record, min_hits=min_hits, min_cells=min_cells,
                                    topk=topk)

    def rooms(self, labels, objects=None, map_shape=None, door_r2: Optional[int] = None, min_cells: Optional[int] = None,
              topk: int = 16, passable=None, known=None, clearance=None, sweeps: Optional[int] = None) -> Dict:
        """The rooms of the map: the dict of `CustomRCNNRecurrent.rooms` (`room_labels`, `grow_dist`, `room`, `area`, `widest_cell`,
        `door_cell`, `door_d2`, `obj_room`, `obj_room_label`, `counts`, ...) for a label map (`obs["merged_labels"]` of `obstacles`)
        on the grid `map_shape` = (rows, cols); `describe(rooms["room"], rooms["room_labels"], classifier=<room vocabulary>)` names them.  The
        model, its heads and the memory are neither read nor changed."""
        return self.model.rooms(labels, objects, map_shape=map_shape, door_r2=door_r2, min_cells=min_cells, topk=topk,
                                passable=passable, known=known, clearance=clearance, sweeps=sweeps)

    def place(self, instances, data: Dict, topk: int = 4, exclude_cell: int = -1, attach: bool = False) -> Dict:
        """Where on the map the detections stand: the dict of `CustomRCNNRecurrent.place` for `instances` (what the call on `data`
        returned under "instances") and `data`, the dict the predictor was called with.  The model is left as it is."""
        return self.model.place(instances, data["proj_indices"], topk=topk, exclude_cell=exclude_cell, attach=attach)

    def _resized_hw(self, h: int, w: int):
        """`ResizeShortestEdge([480, 480], max_size).get_output_shape`."""
        scale = 480.0 / min(h, w)
        nh, nw = (480.0, scale * w) if h < w else (scale * h, 480.0)
        if max(nh, nw) > self.max_size:
            s = self.max_size / max(nh, nw)
            nh, nw = nh * s, nw * s
        return int(nh + 0.5), int(nw + 0.5)

    def __call__(self, data: Dict) -> Dict:
        original_image = np.asarray(data["image"])
        if self.input_format == "RGB":
            original_image = original_image[:, :, ::-1]
        height, width = original_image.shape[:2]
        if self._resized_hw(height, width) != (height, width):
            raise ValueError(f"image {height}x{width}: the predictor's resize would change the image but not proj_indices "
                             "(the reference path only works for frames whose shortest edge is 480)")
        image = torch.from_numpy(np.ascontiguousarray(original_image)).permute(2, 0, 1)
        inputs = {"image": image, "height": height, "width": width, "memory": data["memory"], "proj_indices": data["proj_indices"],
                  "memory_reset": data["memory_reset"], "sequence_name": data["sequence_name"]}
        return self.model([[inputs]])[0]
