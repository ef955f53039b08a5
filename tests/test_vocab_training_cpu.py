"""Training on wide vocabularies, the host side: the class-frequency file, the three configuration keys, the restated class choice
against torch.multinomial, `freq_weight` in checkpoints.  No GPU."""
import json
import os

import pytest
import torch

from _fed_loss_ref import fed_loss_weight_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FREQ = os.path.join(ROOT, "tests", "golden", "lvis_v1_cat_freq.json")


def test_load_class_freq_on_the_lvis_fixture(tmp_path):
    from embodied_object_detection_amd.modeling.fed_loss import load_class_freq
    cats = json.load(open(FREQ))
    assert len(cats) == 1203 and set(cats[0]) == {"id", "image_count"}
    w = load_class_freq(FREQ, 0.5)
    by_id = {c["id"]: c["image_count"] for c in cats}
    assert w.dtype == torch.float32 and tuple(w.shape) == (1203,)
    assert torch.equal(w, torch.tensor([by_id[i] for i in range(1, 1204)]).float() ** 0.5)
    assert torch.equal(load_class_freq(FREQ, 1.0), torch.tensor([by_id[i] for i in range(1, 1204)]).float())
    # id order, whatever the file's order
    shuffled = tmp_path / "shuffled.json"
    shuffled.write_text(json.dumps(cats[::-1]))
    assert torch.equal(load_class_freq(str(shuffled), 0.5), w)
    # shorter than NUM_CLASSES: zero-extended (detic_fast_rcnn.py:89-96); longer: refused at construction
    ext = load_class_freq(FREQ, 0.5, num_classes=1210)
    assert tuple(ext.shape) == (1210,) and torch.equal(ext[:1203], w) and float(ext[1203:].abs().max()) == 0.0
    assert torch.equal(load_class_freq(FREQ, 0.5, num_classes=1203), w)
    with pytest.raises(ValueError, match="1203 categories"):
        load_class_freq(FREQ, 0.5, num_classes=20)
    with pytest.raises(FileNotFoundError, match="CAT_FREQ_PATH"):
        load_class_freq(str(tmp_path / "nothing.json"), 0.5)


def test_the_three_keys_parse_from_yaml_and_overrides(tmp_path):
    from embodied_object_detection_amd import setup_cfg
    from embodied_object_detection_amd.modeling.fed_loss import class_freq_from_cfg
    rb = setup_cfg(None).MODEL.ROI_BOX_HEAD
    assert str(rb.CAT_FREQ_PATH) == "datasets/metadata/lvis_v1_train_cat_info.json" and int(rb.FED_LOSS_NUM_CAT) == 50
    assert float(rb.FED_LOSS_FREQ_WEIGHT) == 0.5 and not bool(rb.USE_FED_LOSS) and not bool(rb.IGNORE_ZERO_CATS)
    assert class_freq_from_cfg(setup_cfg(None), 20) is None
    cfg = setup_cfg(None, ["MODEL.ROI_BOX_HEAD.CAT_FREQ_PATH", FREQ, "MODEL.ROI_BOX_HEAD.FED_LOSS_NUM_CAT", 30,
                           "MODEL.ROI_BOX_HEAD.FED_LOSS_FREQ_WEIGHT", 0.25, "MODEL.ROI_BOX_HEAD.USE_FED_LOSS", True])
    rb = cfg.MODEL.ROI_BOX_HEAD
    assert (str(rb.CAT_FREQ_PATH), int(rb.FED_LOSS_NUM_CAT), float(rb.FED_LOSS_FREQ_WEIGHT), bool(rb.USE_FED_LOSS)) == (FREQ, 30, 0.25, True)
    w = class_freq_from_cfg(cfg, 1203)
    cats = sorted(json.load(open(FREQ)), key=lambda c: c["id"])
    assert torch.equal(w, torch.tensor([c["image_count"] for c in cats]).float() ** 0.25)
    y = tmp_path / "fed.yaml"
    y.write_text("MODEL:\n  ROI_BOX_HEAD:\n    USE_FED_LOSS: True\n    IGNORE_ZERO_CATS: True\n    FED_LOSS_NUM_CAT: 12\n"
                 f"    FED_LOSS_FREQ_WEIGHT: 1.0\n    CAT_FREQ_PATH: '{FREQ}'\n")
    rb = setup_cfg(str(y)).MODEL.ROI_BOX_HEAD
    assert (str(rb.CAT_FREQ_PATH), int(rb.FED_LOSS_NUM_CAT), float(rb.FED_LOSS_FREQ_WEIGHT)) == (FREQ, 12, 1.0)
    assert bool(rb.USE_FED_LOSS) and bool(rb.IGNORE_ZERO_CATS)


@pytest.mark.parametrize("C,n", [(20, 8), (365, 50), (1203, 50), (2047, 300)])
def test_the_restated_class_choice_is_torch_multinomial(C, n):
    """`get_fed_loss_inds` with torch.multinomial as the reference calls it, against the restatement fed the q of a generator with
    the same seed: the same set of classes.  (torch draws q = empty_like(prob).exponential_(1) and takes the top n of prob / q; a
    torch that changes this fails here, the GPU tests do not depend on it.)"""
    for seed in range(4):
        g = torch.Generator().manual_seed(100 * C + seed)
        prob = torch.rand((C,), generator=g) ** 2 * 30 if seed % 2 else None
        if prob is not None:
            prob[torch.randperm(C, generator=g)[:C // 5]] = 0.0            # zero-frequency classes are never drawn
        labels = torch.randint(0, C, (max(1, n // 3),), generator=g)
        gt = torch.cat([labels[torch.randint(0, labels.numel(), (60,), generator=g)], torch.full((40,), C)]).int()
        # the reference, literally (utils.py:16-28); its prob vector has C + 1 entries, the last one (background) zero
        appeared = torch.unique(gt.long())
        p = torch.ones(C + 1)
        p[-1] = 0
        if prob is not None:
            p[:C] = prob.clone()
        p[appeared] = 0
        g1, g2 = torch.Generator().manual_seed(seed), torch.Generator().manual_seed(seed)
        more = torch.multinomial(p, n - appeared.numel(), replacement=False, generator=g1)
        ref = torch.zeros(C + 1)
        ref[torch.cat([appeared, more])] = 1
        q = torch.empty((C + 1,)).exponential_(1, generator=g2)            # the draw torch.multinomial makes inside
        w = fed_loss_weight_ref(gt, C, q[:C], n, prob)
        assert torch.equal(w, ref[:C]), (C, seed)
        assert int(w.sum()) == n - 1                                       # n labels, one of them the background


def test_restatement_edge_cases():
    C = 30
    q = torch.ones(C)
    # ties (equal prob / q): the lower class index wins
    w = fed_loss_weight_ref(torch.tensor([5, 5, 7]), C, q, 6)
    assert w.nonzero().flatten().tolist() == [0, 1, 2, 3, 5, 7]
    # more labels than num_sample_cats: nothing is drawn; rows of -1 are no rows
    w = fed_loss_weight_ref(torch.tensor([1, 2, 3, 4, -1, C]), C, q, 3)
    assert w.nonzero().flatten().tolist() == [1, 2, 3, 4]
    # fewer eligible classes than asked for: all of them
    prob = torch.zeros(C)
    prob[[2, 9]] = 1.0
    w = fed_loss_weight_ref(torch.tensor([4]), C, q, 10, prob)
    assert w.nonzero().flatten().tolist() == [2, 4, 9]
    # the zero mask also clears a class that appeared
    w = fed_loss_weight_ref(torch.tensor([4]), C, q, 10, prob, zero_mask_src=prob)
    assert w.nonzero().flatten().tolist() == [2, 9]


def test_checkpoints_carry_freq_weight(tmp_path):
    """The reference's state dicts hold `roi_heads.box_predictor.{k}.freq_weight` when the federated loss / zero mask is on: a file
    with them loads without a complaint, and they survive the round trip."""
    from embodied_object_detection_amd.checkpoint import expected_shapes, load_checkpoint, save_checkpoint, synthetic_state_dict
    from embodied_object_detection_amd.modeling.fed_loss import FREQ_KEY, load_class_freq
    sd = synthetic_state_dict(0)
    fw = load_class_freq(FREQ, 0.5)
    for k in range(3):
        sd[FREQ_KEY.format(k)] = fw.clone()
    path = str(tmp_path / "model.pth")
    save_checkpoint(path, sd, iteration=3)
    back, report = load_checkpoint(path, 20, verbose=False)
    assert report == {"missing": [], "shape_mismatch": [], "unexpected": []}
    for k in range(3):
        assert torch.equal(back[FREQ_KEY.format(k)], fw)
    assert set(back) == set(expected_shapes(20)) | {FREQ_KEY.format(k) for k in range(3)}
    sd["roi_heads.box_predictor.0.something_else"] = torch.zeros(1)
    save_checkpoint(path, sd, iteration=3)
    assert load_checkpoint(path, 20, verbose=False)[1]["unexpected"] == ["roi_heads.box_predictor.0.something_else"]


def test_fed_loss_params_refuse_bad_sizes():
    from embodied_object_detection_amd import ops
    with pytest.raises(ValueError, match="2047"):
        ops.FedLossParams(2048, 50, None, None, "cpu")
    with pytest.raises(ValueError, match="one entry per class"):
        ops.FedLossParams(20, 5, torch.ones(21), None, "cpu")
    assert ops.fed_loss_param_bytes(1203) == (16 + 12 * 1203 + 15) // 16 * 16 and ops.EOD_LOSS_FED == 1 << 30
