"""Wide vocabularies without a GPU: the host-side checks of the C ABI (workspace sizes, refusals before any device call), the
model-level `reset_cls_test` argument handling on a stub, and the predictor's vocabulary table."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from embodied_object_detection_amd.modeling import load_classifier, reset_cls_test

LVIS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lvis_v1_clip.npy")
EOD_ZS_WIDE = 2
ERR_BAD_DIMS, ERR_NULL, ERR_CAPACITY = -1, -4, -5


def test_detection_workspace_sizes_and_refusals():
    from embodied_object_detection_amd import _lib
    from embodied_object_detection_amd.ops import EodDetDesc
    lib = _lib.load()
    narrow, wide = lib.eod_detections_workspace_bytes(320, 21), lib.eod_detections_workspace_bytes(320, 1204)
    assert wide > narrow > 0
    assert lib.eod_detections_workspace_bytes(320, 2048) > wide
    assert lib.eod_detections_workspace_bytes(320, 2049) == 0 and lib.eod_detections_workspace_bytes(513, 1204) == 0
    buf = (C.c_float * 64)()
    d = EodDetDesc()
    p = C.addressof(buf)
    d.boxes = d.scores = d.out_boxes = d.out_scores = d.out_classes = d.out_rows = d.out_count = d.workspace = p
    d.R_cap, d.C1, d.topk, d.batch = 320, 1204, 100, 1
    d.workspace_bytes = 256                                       # too small: refused by the host-side check, nothing is launched
    assert lib.eod_fast_rcnn_inference(C.byref(d), None) == ERR_CAPACITY
    d.C1 = 2049
    assert lib.eod_fast_rcnn_inference(C.byref(d), None) == ERR_BAD_DIMS
    d.C1, d.R_cap = 1204, 513
    assert lib.eod_fast_rcnn_inference(C.byref(d), None) == ERR_BAD_DIMS


def test_classifier_flag_checks_before_any_device_call():
    from embodied_object_detection_amd import _lib
    lib = _lib.load()
    buf = (C.c_float * 64)()
    p = C.addressof(buf)
    args = lambda acc, C1: (p, p, p, acc, None, None, 64, 512, C1, 50.0, None, None, None, 0.0, 1, None)
    assert lib.eod_zs_classify(*args(0, 30)) == ERR_CAPACITY                       # wide vocabulary without the flag
    assert lib.eod_zs_classify(*args(1, 30)) == ERR_CAPACITY
    assert lib.eod_zs_classify(*args(EOD_ZS_WIDE, 2049)) == ERR_CAPACITY           # beyond the wide kernel as well
    assert lib.eod_zs_classify(*args(EOD_ZS_WIDE, 1)) == ERR_BAD_DIMS
    d = _lib.EodStageTailDesc()
    d.feat = d.zs = d.prob_acc = d.hb = d.w2 = d.b2 = d.boxes_in = d.boxes_out = p
    d.R_cap, d.D, d.C1, d.hb_dim, d.w2_ld, d.batch = 64, 512, 30, 1024, 1024, 1
    assert lib.eod_cascade_stage_tail(C.byref(d), None) == ERR_CAPACITY
    d.accumulate, d.C1 = EOD_ZS_WIDE | 1, 2049
    assert lib.eod_cascade_stage_tail(C.byref(d), None) == ERR_CAPACITY
    assert lib.eod_memory_scores(p, p, p, p, None, 64, 512, 2049, None) == ERR_CAPACITY


def test_ops_refusal_messages_name_the_argument_and_the_limit():
    from embodied_object_detection_amd import ops
    assert "classes" in ops._zs_refusal("eod_zs_classify", 30, False) and "wide=True" in ops._zs_refusal("eod_zs_classify", 30, False)
    assert "2047 classes" in ops._zs_refusal("eod_zs_classify", 2049, True)


class _StubHeads:
    device = "cpu"

    def __init__(self, norm_weight=True):
        self.norm_weight = norm_weight
        self.zs = None

    def set_classifier(self, zs):
        self.zs = zs


class _StubModel:
    def __init__(self, norm_weight=True):
        self.roi_heads = _StubHeads(norm_weight)


def test_reset_cls_test_argument_handling(tmp_path):
    rows = np.load(LVIS)
    assert rows.shape == (1203, 512) and rows.dtype == np.int8 and os.path.getsize(LVIS) < 700_000     # tests/golden/gen_lvis_clip.py
    unit = rows[:200].astype(np.float32)
    unit /= np.linalg.norm(unit, axis=1, keepdims=True)
    assert float((unit @ unit.T)[~np.eye(200, dtype=bool)].mean()) > 0.6       # real text rows: strongly correlated classes
    m = _StubModel()
    reset_cls_test(m, LVIS, 1203)                                  # a .npy path: [C, 512]
    zs = m.roi_heads.zs
    assert zs.shape == (512, 1204) and zs.dtype == torch.float32 and zs.is_contiguous()
    assert bool((zs[:, -1] == 0).all())                            # zero background column
    assert torch.allclose(zs[:, :-1].norm(dim=0), torch.ones(1203), atol=1e-5)
    w = torch.tensor(rows[:80], dtype=torch.float32).t() * 3.0     # a tensor: [512, C]
    reset_cls_test(m, w, 80)
    assert m.roi_heads.zs.shape == (512, 81) and torch.allclose(m.roi_heads.zs[:, :80].norm(dim=0), torch.ones(80), atol=1e-5)
    assert torch.equal(m.roi_heads.zs, load_classifier(w, 80))
    raw = _StubModel(norm_weight=False)
    reset_cls_test(raw, w, 80)
    assert torch.equal(raw.roi_heads.zs[:, :80], w) and bool((raw.roi_heads.zs[:, 80] == 0).all())
    with pytest.raises(ValueError, match="80 classes"):
        reset_cls_test(m, w, 81)                                   # width and num_classes disagree
    with pytest.raises(ValueError, match="512"):
        reset_cls_test(m, w.t().contiguous(), 80)                  # a tensor is [512, C], not [C, 512]
    small = tmp_path / "coco80.npy"
    np.save(small, rows[:80])
    reset_cls_test(m, str(small), 80)
    assert m.roi_heads.zs.shape == (512, 81)


def test_predictor_vocabulary_table():
    from embodied_object_detection_amd.engine.predictor import BUILDIN_CLASSIFIER, resolve_vocabulary
    assert sorted(BUILDIN_CLASSIFIER) == ["coco", "lvis", "mp3d", "objects365", "openimages"]
    assert os.path.basename(BUILDIN_CLASSIFIER["lvis"]) == "lvis_v1_clip_a+cname.npy"
    p = resolve_vocabulary("mp3d")                                 # the one matrix that ships with the package
    assert os.path.exists(p) and np.load(p).shape == (20, 512)
    with pytest.raises(FileNotFoundError, match="lvis_v1_clip_a\\+cname.npy"):
        resolve_vocabulary("lvis")
    with pytest.raises(ValueError, match="classifier="):
        resolve_vocabulary("custom")
    with pytest.raises(ValueError, match="expected one of"):
        resolve_vocabulary("imagenet")
