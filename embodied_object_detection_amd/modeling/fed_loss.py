"""The class frequencies behind the federated loss and the zero-frequency mask (USE_FED_LOSS / IGNORE_ZERO_CATS of
`DeticFastRCNNOutputLayers`, detic_fast_rcnn.py:85-96,213-225).  The class choice itself runs on the device
(`ops.FedLossParams`, `fed_loss_weight_kernel`)."""
from __future__ import annotations

import json
import os
from typing import Optional

import torch

FREQ_KEY = "roi_heads.box_predictor.{}.freq_weight"      # the reference registers the frequencies as a buffer of every stage


def load_class_freq(path: str, freq_weight: float = 1.0, num_classes: Optional[int] = None) -> torch.Tensor:
    """`load_class_freq` (detic/modeling/utils.py:7-13): image_count ** freq_weight of the categories in `path` (a JSON list of
    {"id", "image_count", ...}), in the order of their ids.  With `num_classes`: a shorter list is extended with zeros
    (detic_fast_rcnn.py:89-96), a longer one is refused (the reference fails later, inside the class choice, with a shape error)."""
    if not os.path.exists(path):
        raise FileNotFoundError(f"MODEL.ROI_BOX_HEAD.CAT_FREQ_PATH: no such file: {path!r} (USE_FED_LOSS / IGNORE_ZERO_CATS need the "
                                "categories' image counts)")
    with open(path, "r") as fh:
        cat_info = json.load(fh)
    counts = torch.tensor([c["image_count"] for c in sorted(cat_info, key=lambda x: x["id"])])
    w = counts.float() ** freq_weight
    if num_classes is not None:
        if w.numel() > num_classes:
            raise ValueError(f"MODEL.ROI_BOX_HEAD.CAT_FREQ_PATH {path!r} lists {w.numel()} categories, MODEL.ROI_HEADS.NUM_CLASSES is "
                             f"{num_classes}")
        if w.numel() < num_classes:
            w = torch.cat([w, w.new_zeros(num_classes - w.numel())])
    return w


def class_freq_from_cfg(cfg, num_classes: int) -> Optional[torch.Tensor]:
    """The stage predictors' `freq_weight` [C] for a configuration, None when neither USE_FED_LOSS nor IGNORE_ZERO_CATS is set."""
    rb = cfg.MODEL.ROI_BOX_HEAD
    if not (bool(rb.USE_FED_LOSS) or bool(rb.IGNORE_ZERO_CATS)):
        return None
    return load_class_freq(str(rb.CAT_FREQ_PATH), float(rb.FED_LOSS_FREQ_WEIGHT), num_classes)
