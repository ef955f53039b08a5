"""Wide vocabularies (24 to 2047 classes) at kernel level: the matrix-core classifier, the wide memory re-score and the
three-launch fast_rcnn_inference, against the CPU oracle's arithmetic.  Class matrices are row slices of the LVIS CLIP fixture (int8
per row, tests/golden/gen_lvis_clip.py): real text rows are strongly correlated, which floods the selection with near-equal candidates."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from oracle import ops as OO

LVIS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lvis_v1_clip.npy")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    from embodied_object_detection_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def class_matrix(C: int) -> torch.Tensor:
    """[512, C + 1] as the classifier holds it (zero background column, unit columns); beyond LVIS' 1203 rows the rows repeat."""
    rows = torch.tensor(np.load(LVIS), dtype=torch.float32)
    if C > rows.shape[0]:
        rows = torch.cat([rows, rows.flip(0) * 0.5 + rows.roll(7, 0) * 0.5])
    w = rows[:C].t().contiguous()
    w = torch.cat([w, w.new_zeros((512, 1))], dim=1)
    return F.normalize(w, p=2, dim=0).contiguous()


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(shape, generator=g) * scale


def close(a, b, rtol, atol):
    a, b = a.detach().cpu().float(), b.detach().cpu().float()
    assert a.shape == b.shape, (a.shape, b.shape)
    err = (a - b).abs()
    assert bool((err <= atol + rtol * b.abs()).all()), f"max err {err.max().item():.3e}"


def run_cascade(ops, dev, feats, zs, ps, cnt, cap, C1, batch=1, wide=True):
    """Three stages accumulated + the final fusion -> (prob, featn of stage 0)."""
    prob = torch.full((cap * batch, C1), -7.0, device=dev)
    featn = torch.full((cap * batch, 512), -7.0, device=dev)
    for k in range(3):
        ops.zs_classify(feats[k], zs, prob, k > 0, featn if k == 0 else None, cnt, cap, C1, prop_scores=ps if k == 2 else None,
                        final_inv_stages=1.0 / 3 if k == 2 else 0.0, batch=batch, wide=wide)
    return prob, featn


@pytest.mark.parametrize("C1", [25, 81, 366, 1204, 2048])
def test_wide_classifier_matches_oracle(dev, C1):
    from embodied_object_detection_amd import ops
    cap, R = 96, 70
    zs = class_matrix(C1 - 1)
    feats = [rnd(cap, 512, seed=30 + k) for k in range(3)]
    ps = torch.rand(cap, generator=torch.Generator().manual_seed(5))
    cnt = torch.tensor([R], dtype=torch.int32, device=dev)
    prob, featn = run_cascade(ops, dev, [f.to(dev) for f in feats], zs.to(dev), ps.to(dev), cnt, cap, C1)
    # oracle/model.py:232-246 + detic_roi_heads.py:164-173
    ref = sum(torch.sigmoid((50.0 * F.normalize(f, p=2, dim=1)) @ zs) for f in feats) / 3
    ref = torch.sqrt(ref * ps[:, None])
    close(prob[:R], ref[:R], rtol=1e-5, atol=1e-5)
    assert bool((prob[R:] == -7.0).all()) and bool((featn[R:] == -7.0).all()), "rows beyond count were written"
    # feat_norm_out does not depend on the classes: bitwise the narrow kernel's
    zs21 = class_matrix(20).to(dev)
    prob21, featn21 = run_cascade(ops, dev, [f.to(dev) for f in feats], zs21, ps.to(dev), cnt, cap, 21, wide=False)
    assert torch.equal(featn[:R], featn21[:R])
    prob21w, featn21w = run_cascade(ops, dev, [f.to(dev) for f in feats], zs21, ps.to(dev), cnt, cap, 21, wide=True)
    assert torch.equal(prob21, prob21w) and torch.equal(featn21, featn21w)          # wide=True below 25 columns: the narrow kernel


def test_wide_classifier_batch_equals_single_calls(dev):
    from embodied_object_detection_amd import ops
    cap, C1 = 64, 366
    zs = class_matrix(C1 - 1).to(dev)
    feats = [rnd(2 * cap, 512, seed=40 + k).to(dev) for k in range(3)]
    ps = torch.rand(2 * cap, generator=torch.Generator().manual_seed(6)).to(dev)
    counts = [50, 9]
    cnt = torch.tensor(counts, dtype=torch.int32, device=dev)
    prob, featn = run_cascade(ops, dev, feats, zs, ps, cnt, cap, C1, batch=2)
    for b in range(2):
        sl = slice(b * cap, (b + 1) * cap)
        p1, f1 = run_cascade(ops, dev, [f[sl].contiguous() for f in feats], zs, ps[sl].contiguous(), cnt[b:b + 1], cap, C1)
        assert torch.equal(prob[sl], p1) and torch.equal(featn[sl], f1)


def test_wide_classifier_needs_the_flag(dev):
    from embodied_object_detection_amd import _lib, ops
    cap = 32
    feat, prob = rnd(cap, 512).to(dev), torch.zeros((cap, 2049), device=dev)
    with pytest.raises(_lib.EodError, match="classes.*wide=True"):
        ops.zs_classify(feat, class_matrix(29).to(dev), prob, False, None, None, cap, 30)
    with pytest.raises(_lib.EodError, match="2047 classes"):
        ops.zs_classify(feat, torch.zeros((512, 2049), device=dev), prob, False, None, None, cap, 2049, wide=True)


@pytest.mark.parametrize("C1", [81, 1204])
def test_wide_stage_tail_boxes_bitwise_equal_narrow(dev, C1):
    """`eod_cascade_stage_tail` with a wide matrix: the BoxTail rides in the wide launch; boxes and deltas are bitwise those of a
    narrow (21 column) call on the same rows, the probabilities those of `zs_classify`."""
    from embodied_object_detection_amd import ops
    cap, R = 64, 45
    g = torch.Generator().manual_seed(3)
    feat, hb = rnd(cap, 512, seed=50).to(dev), torch.relu(rnd(cap, 1024, seed=51)).to(dev)
    bb2 = ops.Conv((torch.randn((4, 1024), generator=g) * 0.01)[:, :, None, None], torch.randn((4,), generator=g) * 0.01, device=dev,
                   name="bb2")
    xy = torch.rand((cap, 2), generator=g) * 80
    boxes = torch.cat([xy, xy + 10 + torch.rand((cap, 2), generator=g) * 60], dim=1).to(dev)
    cnt = torch.tensor([R], dtype=torch.int32, device=dev)
    out = {}
    for c1, wide in ((21, False), (C1, True)):
        zs = class_matrix(c1 - 1).to(dev)
        prob, featn = torch.zeros((cap, c1), device=dev), torch.zeros((cap, 512), device=dev)
        bo, de = torch.full((cap, 4), -3.0, device=dev), torch.full((cap, 4), -3.0, device=dev)
        ops.cascade_stage_tail(feat, zs, prob, False, featn, cnt, cap, c1, 50.0, hb, bb2, boxes, bo, (10.0, 10.0, 5.0, 5.0), True, 200.0,
                               150.0, deltas_out=de, wide=wide)
        ref = torch.zeros((cap, c1), device=dev)
        ops.zs_classify(feat, zs, ref, False, None, cnt, cap, c1, wide=wide)
        assert torch.equal(prob, ref)
        out[c1] = (bo, de, featn)
    for a, b in zip(out[21], out[C1]):
        assert torch.equal(a, b)
    assert bool((out[C1][0][R:] == -3.0).all())


@pytest.mark.parametrize("C1", [81, 1204])
def test_wide_memory_scores(dev, C1):
    from embodied_object_detection_amd import ops
    cap, R = 64, 41
    zs = class_matrix(C1 - 1)
    featn = 50.0 * F.normalize(rnd(cap, 512, seed=60), p=2, dim=1)
    ps = torch.rand(cap, generator=torch.Generator().manual_seed(8)) * 1.2          # some >= 1: excluded rows
    out = torch.full((cap, C1), -7.0, device=dev)
    ops.memory_scores(featn.to(dev), zs.to(dev), ps.to(dev), out, torch.tensor([R], dtype=torch.int32, device=dev), cap, C1)
    ref = torch.where(ps[:, None] < 1.0, torch.sqrt(torch.sigmoid(featn @ zs) * ps[:, None]), torch.zeros(()))
    close(out[:R], ref[:R], rtol=1e-5, atol=1e-5)
    assert bool((out[R:] == -7.0).all())


# ---- selection -------------------------------------------------------------------------------------------------------------------
def selection_inputs(R, C, spread, kind, seed=11):
    g = torch.Generator().manual_seed(seed)
    ctr = torch.tensor([100.0, 75.0]) + (torch.rand((R, 2), generator=g) - 0.5) * torch.tensor([200.0, 150.0]) * spread
    size = torch.rand((R, 2), generator=g) * 80 * min(1.0, spread * 4) + (4 if spread == 1.0 else 60)
    boxes = torch.cat([ctr - size / 2, ctr + size / 2], dim=1)
    if kind == "uniform":
        scores = torch.rand((R, C + 1), generator=g)
    else:       # classifier-shaped: sqrt(sigmoid(x @ lvis) * proposal score), many near-equal columns
        x = 50.0 * F.normalize(torch.randn((R, 512), generator=g) + 3.0 * class_matrix(C)[:, torch.randint(0, C, (R,), generator=g)].t(),
                               p=2, dim=1)
        scores = torch.sqrt(torch.sigmoid(x @ class_matrix(C)) * torch.rand((R, 1), generator=g))
    scores[3, 5] = float("nan")                                     # non-finite rows are dropped
    boxes[7, 2] = float("inf")
    return boxes, scores


def check_selection(dev, sel, boxes, scores, R, cap, C, thresh, topk, ref=None):
    rb, rs, rc, rr = ref if ref is not None else OO.fast_rcnn_inference_single(boxes, scores, (150, 200), thresh, 0.5, topk)
    bp = torch.zeros((cap, 4)); bp[:R] = boxes
    sp = torch.zeros((cap, C + 1)); sp[:R] = scores
    cnt = torch.tensor([R], dtype=torch.int32, device=dev)
    b, s, c, r, n = sel(bp.to(dev), sp.to(dev), cnt, 200.0, 150.0, thresh, 0.5)
    n = int(n.item())
    assert n == rb.shape[0], (n, rb.shape[0])
    assert torch.equal(s[:n].cpu(), rs) and torch.equal(b[:n].cpu(), rb)
    assert torch.equal(c[:n].cpu().long(), rc.long()) and torch.equal(r[:n].cpu().long(), rr.long())
    return (b[:n].clone(), s[:n].clone(), c[:n].clone(), r[:n].clone()), (rb, rs, rc, rr)


@pytest.mark.parametrize("kind,C,thresh,topk,spread", [
    ("uniform", 80, 0.02, 300, 1.0), ("clip", 80, 0.0, 100, 0.05), ("clip", 365, 0.3, 100, 1.0), ("uniform", 365, 0.02, 300, 0.05),
    ("uniform", 1203, 0.0, 300, 1.0), ("clip", 1203, 0.02, 100, 1.0), ("uniform", 1203, 0.3, 300, 1.0), ("clip", 1203, 0.3, 300, 1.0),
    ("uniform", 1203, 0.0, 300, 0.05), ("clip", 1203, 0.02, 100, 0.05), ("uniform", 1203, 0.02, 300, 1.0)])
def test_wide_selection_matches_oracle(dev, kind, C, thresh, topk, spread):
    """`spread` 0.05 piles the boxes up: per-class NMS removes nearly everything and the tail workgroup has to fetch further batches
    below the first cut.  Threshold 0.0 makes every slot of the matrix a candidate."""
    from embodied_object_detection_amd import ops
    R, cap = 256, 320
    boxes, scores = selection_inputs(R, C, spread, kind)
    sel = ops.DetectionSelector(cap, C + 1, topk, dev, unique=True, groups=True)
    got, ref = check_selection(dev, sel, boxes, scores, R, cap, C, thresh, topk)
    rr = ref[3].long()
    n = rr.numel()
    u = torch.unique(rr)
    assert int(sel.uniq_count.item()) == u.numel() and torch.equal(sel.uniq_rows[:u.numel()].cpu().long(), u)
    first = {}
    for k, row in enumerate(rr.tolist()):
        first.setdefault(row, k)
    assert torch.equal(sel.rep_of[:n].cpu().long(), torch.tensor([first[row] for row in rr.tolist()], dtype=torch.long))
    reps = sorted(first.values())
    assert int(sel.rep_count.item()) == len(reps) and sel.rep_list[:len(reps)].cpu().tolist() == reps
    # a second call on the same object: same bits (the call leaves its workspace as it found it)
    again, _ = check_selection(dev, sel, boxes, scores, R, cap, C, thresh, topk, ref=ref)
    for a, b in zip(got, again):
        assert torch.equal(a, b)


def test_wide_selection_equal_scores(dev):
    """Every score equal: one histogram bin holds all 2 x 10^5 candidates, the order is the slot order alone."""
    from embodied_object_detection_amd import ops
    R, cap, C = 200, 256, 1203
    boxes, _ = selection_inputs(R, C, 1.0, "uniform")
    boxes[7, 2] = 150.0
    scores = torch.full((R, C + 1), 0.5)
    sel = ops.DetectionSelector(cap, C + 1, 100, dev)
    check_selection(dev, sel, boxes, scores, R, cap, C, 0.1, 100)


@pytest.mark.parametrize("B", [2, 4])
def test_wide_selection_batch_equals_single_runs(dev, B):
    from embodied_object_detection_amd import ops
    cap, C, topk = 256, 365, 100
    Rs = [256, 40, 0, 130][:B]
    single = ops.DetectionSelector(cap, C + 1, topk, dev, unique=True, groups=True)
    batch = ops.DetectionSelector(cap, C + 1, topk, dev, unique=True, groups=True, batch=B)
    bp, sp = torch.zeros((B * cap, 4)), torch.zeros((B * cap, C + 1))
    for b, R in enumerate(Rs):
        if R:
            boxes, scores = selection_inputs(R, C, 0.3, "clip" if b % 2 else "uniform", seed=20 + b)
            bp[b * cap:b * cap + R], sp[b * cap:b * cap + R] = boxes, scores
    bp, sp = bp.to(dev), sp.to(dev)
    cnt = torch.tensor(Rs, dtype=torch.int32, device=dev)
    batch(bp, sp, cnt, 200.0, 150.0, 0.02, 0.5)
    for b in range(B):
        sb, ss, sc, sr, sn = single(bp[b * cap:(b + 1) * cap], sp[b * cap:(b + 1) * cap], cnt[b:b + 1], 200.0, 150.0, 0.02, 0.5)
        n = int(sn.item())
        assert int(batch.count[b].item()) == n
        sl = slice(b * topk, b * topk + n)
        assert torch.equal(batch.boxes[sl], sb[:n]) and torch.equal(batch.scores[sl], ss[:n])
        assert torch.equal(batch.classes[sl], sc[:n]) and torch.equal(batch.rows[sl], sr[:n])
        nu = int(single.uniq_count.item())
        assert int(batch.uniq_count[b].item()) == nu and torch.equal(batch.uniq_rows[b * cap:b * cap + nu], single.uniq_rows[:nu])
        nr = int(single.rep_count.item())
        assert int(batch.rep_count[b].item()) == nr and torch.equal(batch.rep_list[sl.start:sl.start + nr], single.rep_list[:nr])
        assert torch.equal(batch.rep_of[sl], single.rep_of[:n])
