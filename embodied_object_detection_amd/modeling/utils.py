"""`reset_cls_test` on a built model (`Detic/detic/modeling/utils.py:32-50`): swap the open-vocabulary classifier at test time.

The reference replaces `cls_score.zs_weight` of the three cascade predictors and sets `roi_heads.num_classes`; the
meta-architecture's own `zs_weight` (the memory's CLIP re-score, `custom_rcnn.py:374-382`), the memory and the pyramids stay.
"""
from __future__ import annotations

from typing import Union

import numpy as np
import torch
import torch.nn.functional as F


def load_classifier(cls_path_or_tensor: Union[str, torch.Tensor], num_classes: int, norm_weight: bool = True) -> torch.Tensor:
    """A `.npy` path (CLIP text rows `[C, 512]`, any float type) or a tensor `[512, C]` -> the matrix the classifier holds:
    `[512, C + 1]` fp32 with a zero background column appended, columns L2-normalised when `norm_weight`."""
    if isinstance(cls_path_or_tensor, (str, bytes)) or hasattr(cls_path_or_tensor, "__fspath__"):
        w = torch.tensor(np.load(cls_path_or_tensor), dtype=torch.float32).permute(1, 0).contiguous()      # D x C
    else:
        w = torch.as_tensor(cls_path_or_tensor).detach().to(dtype=torch.float32, device="cpu")
    if w.dim() != 2 or w.shape[0] != 512:
        raise ValueError(f"classifier {tuple(w.shape)}: expected a [C, 512] .npy file or a [512, C] tensor")
    if w.shape[1] != int(num_classes):
        raise ValueError(f"classifier with {w.shape[1]} classes, num_classes = {num_classes}")
    w = torch.cat([w, w.new_zeros((w.shape[0], 1))], dim=1)                                                  # D x (C + 1)
    if norm_weight:
        w = F.normalize(w, p=2, dim=0)
    return w.contiguous()


def query_classifier(classifier: Union[str, torch.Tensor], num_classes, norm_weight: bool, device) -> torch.Tensor:
    """The class matrix of a one-off memory query (`semantic_map(classifier=...)`): `load_classifier` with `num_classes` read off the
    matrix when not given, on `device`.  Nothing of a model is touched."""
    if num_classes is None:
        if isinstance(classifier, torch.Tensor):
            num_classes = int(classifier.shape[1])
        else:
            num_classes = int(np.load(classifier, mmap_mode="r").shape[0])
    return load_classifier(classifier, int(num_classes), norm_weight).to(device)


def reset_cls_test(model, cls_path_or_tensor: Union[str, torch.Tensor], num_classes: int) -> None:
    """Works on the single-scene model and on the lock-step batch model, between two frames of a running sequence: the memory is
    not reset.  Vocabularies of 1 to 2047 classes; up to 23 classes the heads run the narrow kernels they ran before."""
    inner = getattr(model, "model", model)               # LockstepScenes wraps the single-scene model whose heads it runs
    rh = inner.roi_heads
    zs = load_classifier(cls_path_or_tensor, num_classes, bool(getattr(rh, "norm_weight", True)))
    dev = getattr(rh, "device", None)
    if dev is not None and torch.device(dev).type == "cuda":
        torch.cuda.synchronize(dev)                      # frames in flight still read the old matrix and selectors
    rh.set_classifier(zs)
    if model is not inner and hasattr(model, "set_classifier_width"):
        model.set_classifier_width()
