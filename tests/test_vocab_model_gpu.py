"""Wide vocabularies through the models: frames with a 1203-class head matrix against the CPU oracle, `reset_cls_test` on a built
model in the middle of a sequence, the lock-step batch, the predictor and the CLI."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import memory as OM
from oracle import model as M
from oracle import ops as OO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LVIS = os.path.join(ROOT, "tests", "golden", "lvis_v1_clip.npy")


def _frames(H, W, n, map_w=24, map_h=24, seed=0):
    from embodied_object_detection_amd.data.synthetic import SyntheticSequence
    seq = SyntheticSequence(seed, H=H, W=W, n_frames=n, map_w=map_w, map_h=map_h, cell=0.5)
    return [seq.frame(i) for i in range(n)]


def _cfg(*extra):
    from embodied_object_detection_amd import setup_cfg
    return setup_cfg(None, ["MODEL.MEMORY_TYPE", "implicit_memory", "MODEL.MAP_FEAT_FUSION", "sum", "MODEL.MAP_FEATURE_WEIGHT", 5,
                            "MODEL.MEMORY_CLS_SCORE_THRESH", 0.3, *extra])


# the shipped yaml resets the heads' classifier at build time (RESET_CLS_TESTS: True, mp3d): point that reset at the LVIS matrix
LVIS_HEADS = ["MODEL.TEST_CLASSIFIERS", f"('{LVIS}',)", "MODEL.TEST_NUM_CLASSES", "[1203]"]


def _lvis_matrix():
    from embodied_object_detection_amd.modeling import load_classifier
    return load_classifier(LVIS, 1203)


def _sd_with_heads(sd, zs):
    sd = dict(sd)
    for k in range(3):
        sd[f"roi_heads.box_predictor.{k}.cls_score.zs_weight"] = zs.clone()
    return sd


def _out(model, f):
    o = model([[f]])[0]["instances"]
    return o.pred_boxes.tensor.clone(), o.scores.clone(), o.pred_classes.clone(), o.pred_masks.clone()


def _check_frame(out, ref, tol_box, tol_score, tag):
    """The assertions of tests/test_model_gpu.py::test_recurrent_frames_match_oracle on the detections of one frame."""
    r = ref["instances"]
    gb, gs, gc = out.pred_boxes.tensor.cpu(), out.scores.cpu(), out.pred_classes.cpu()
    n_ref, n_got = r["pred_boxes"].shape[0], len(out)
    assert abs(n_ref - n_got) <= max(3, int(0.02 * n_ref)), (tag, n_ref, n_got)
    ious = torch.stack([OO.iou_one_to_many(b, gb) for b in r["pred_boxes"]])
    same = r["pred_classes"].long()[:, None] == gc.long()[None, :]
    iou, idx = torch.where(same, ious, torch.full_like(ious, -1.0)).max(dim=1)
    ok = iou > 0.99
    assert ok.float().mean().item() >= 0.98, (tag, ok.float().mean().item())
    box_err = (gb[idx] - r["pred_boxes"]).abs().max(dim=1).values[ok].max().item()
    score_err = (gs[idx] - r["scores"]).abs()[ok].max().item()
    print(f"[{tag}] matched {int(ok.sum())}/{n_ref}, max dbox {box_err:.2e} px, max dscore {score_err:.2e}")
    assert box_err < tol_box and score_err < tol_score, (tag, box_err, score_err)
    mism = (out.pred_masks.cpu()[idx][ok] != r["pred_masks"][ok]).float().mean().item()
    assert mism < 5e-3, (tag, mism)


@pytest.mark.parametrize("memory_wide", [False, True])
def test_frames_with_lvis_heads_match_oracle(synthetic_sd, memory_wide, tmp_path):
    """Head matrix 1203 classes wide; the memory's matrix 20 wide (mixed case) or 1203 wide as well (the Base yaml's case)."""
    from embodied_object_detection_amd import build_model
    H, W = 128, 160
    frames = _frames(H, W, 3)
    zs = _lvis_matrix()
    sd = _sd_with_heads(synthetic_sd, zs)
    extra = list(LVIS_HEADS)
    if memory_wide:
        extra += ["MODEL.ROI_BOX_HEAD.ZEROSHOT_WEIGHT_PATH", LVIS]
    model = build_model(_cfg(*extra), sd)
    assert model.roi_heads.num_classes == 1203 and model.C1 == (1204 if memory_wide else 21)
    oracle = OM.RecurrentOracle(sd, M.OracleCfg(memory_cls_score_thresh=0.3, map_feature_weight=5.0, num_classes=1203))
    if not memory_wide:
        oracle.zs_weight = synthetic_sd["roi_heads.box_predictor.0.cls_score.zs_weight"]       # the meta-architecture's own matrix
    for i, f in enumerate(frames):
        out = model([[f]])[0]["instances"]
        ref = oracle.step(f, i, frames)
        assert int(out.pred_classes.max()) < 1203
        _check_frame(out, ref, 5e-3, 1e-3, f"lvis heads, memory {'lvis' if memory_wide else 'mp3d'}, frame {i}")
        assert torch.equal(model.observations.cpu(), oracle.observations), f"frame {i}: observation counters differ"
        # the next frame starts from the oracle's memory: this test is about the vocabulary, not about knife-edge mask pixels
        model.implicit_memory.copy_(oracle.implicit_memory.to(model.device))
        model.invalidate_memory_snapshot()


def test_fullsize_frame_with_lvis_heads_and_written_memory(synthetic_sd):
    from embodied_object_detection_amd import build_model
    H = W = 640
    frames = _frames(H, W, 2, map_w=200, map_h=200)
    sd = _sd_with_heads(synthetic_sd, _lvis_matrix())
    model = build_model(_cfg(*LVIS_HEADS), sd)
    assert model.roi_heads.num_classes == 1203
    oracle = OM.RecurrentOracle(sd, M.OracleCfg(memory_cls_score_thresh=0.3, map_feature_weight=5.0, num_classes=1203))
    oracle.zs_weight = synthetic_sd["roi_heads.box_predictor.0.cls_score.zs_weight"]
    model([[frames[0]]])
    oracle.step(frames[0], 0, frames)
    model.implicit_memory.copy_(oracle.implicit_memory.to(model.device))
    model.invalidate_memory_snapshot()
    out = model([[frames[1]]])[0]["instances"]
    _check_frame(out, oracle.step(frames[1], 1, frames), 5e-3, 1e-3, "640x640, lvis heads, written memory")


def test_reset_cls_test_mid_sequence(synthetic_sd):
    """20 -> 1203 -> 20 classes on one built model: the last segment is bitwise the unswitched run's, the memory is not reset."""
    from embodied_object_detection_amd import build_model
    from embodied_object_detection_amd.modeling import reset_cls_test
    frames = _frames(128, 160, 6)
    plain = build_model(_cfg(), synthetic_sd)
    ref = [_out(plain, f) for f in frames]
    ref_mem = plain.implicit_memory.clone()
    model = build_model(_cfg(), synthetic_sd)
    mp3d = str(_cfg().MODEL.ROI_BOX_HEAD.ZEROSHOT_WEIGHT_PATH)      # the file the model was built with: same arithmetic, same bits
    got = []
    for i, f in enumerate(frames):
        if i == 2:
            mem_before = model.implicit_memory.clone()
            reset_cls_test(model, LVIS, 1203)
            assert model.roi_heads.num_classes == 1203 and torch.equal(model.implicit_memory, mem_before) and model.C1 == 21
        if i == 4:
            reset_cls_test(model, mp3d, 20)
            assert model.roi_heads.num_classes == 20
        got.append(_out(model, f))
    for i in (0, 1, 4, 5):
        for a, b in zip(ref[i], got[i]):
            assert torch.equal(a, b), f"frame {i} differs from the unswitched run"
    assert int(got[2][2].max()) > 20 and int(got[3][2].max()) < 1203
    assert torch.equal(model.implicit_memory, ref_mem) and torch.equal(model.observations, plain.observations)


def test_lockstep_two_scenes_with_lvis_heads_equal_single_runs(synthetic_sd):
    from embodied_object_detection_amd import build_model
    from embodied_object_detection_amd.modeling.lockstep import LockstepScenes
    from embodied_object_detection_amd.modeling import reset_cls_test
    seqs = [_frames(128, 160, 3, seed=s) for s in (0, 1)]
    singles = []
    for fr in seqs:
        m = build_model(_cfg(), synthetic_sd)
        reset_cls_test(m, LVIS, 1203)
        singles.append([_out(m, f) for f in fr])
    ls = LockstepScenes(_cfg(), 2, synthetic_sd)
    reset_cls_test(ls, LVIS, 1203)
    assert ls.model.roi_heads.num_classes == 1203
    res = ls([list(seqs[0]), list(seqs[1])])
    for b in range(2):
        for t in range(3):
            o = res[b][t]["instances"]
            got = (o.pred_boxes.tensor, o.scores, o.pred_classes, o.pred_masks)
            for a, g in zip(singles[b][t], got):
                assert torch.equal(a, g), f"scene {b} frame {t}"


def test_predictor_with_a_custom_classifier(synthetic_sd):
    from embodied_object_detection_amd.engine.predictor import EmbodiedPredictor
    f = _frames(480, 640, 1, map_w=40, map_h=40)[0]
    pred = EmbodiedPredictor(_cfg("INPUT.FORMAT", "BGR"), synthetic_sd, classifier=LVIS)
    assert pred.model.roi_heads.num_classes == 1203
    img = f["image"].permute(1, 2, 0).numpy().astype(np.uint8)
    out = pred({"image": img, "memory": f.get("memory"), "proj_indices": f["proj_indices"], "memory_reset": f["memory_reset"],
                "sequence_name": f["sequence_name"]})["instances"]
    assert len(out) > 0 and 0 <= int(out.pred_classes.min()) and int(out.pred_classes.max()) < 1203
    with pytest.raises(FileNotFoundError):
        EmbodiedPredictor(_cfg(), synthetic_sd, vocabulary="lvis")


def test_cli_evaluates_with_test_num_classes_1203(tmp_path):
    cmd = [sys.executable, "-m", "embodied_object_detection_amd.train_mp3d", "--eval-only", "--synthetic-scenes", "1", "--synthetic-frames",
           "4", "--synthetic-size", "128", "160", "MODEL.MEMORY_TYPE", "implicit_memory", "MODEL.RESET_CLS_TESTS", "True",
           "MODEL.TEST_CLASSIFIERS", f"('{LVIS}',)", "MODEL.TEST_NUM_CLASSES", "[1203]", "OUTPUT_DIR", str(tmp_path)]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "[eval] all: AP" in r.stdout and "frames/s" in r.stdout, r.stdout[-2000:]
