"""The spatial memory read as a semantic map in any vocabulary, with a confidence per cell (EOD_SEMMAP_SCORES on
`eod_semmap_labels`, `ops.semmap_query`, `semantic_map(classifier=..., scores=True)`): the matrix-core kernel against float64 on the
fp32 inputs, the decisions that must be exact, the flagged call against the plain one, and the Python surface on the models.

The kernel launches one workgroup per 64 cells without a grid cap or a loop over row tiles, so there is no cap to test beyond.

Bounds (u = 2^-24, xh the float64-normalised row, L = 50 xh . z_c):
  one fp32 logit       B(row, c) = 50 u [514 sum_k |xh_k||z_kc| + 260 |xh . z_c|]   (a 512-term fma chain in any order and the two
                       roundings of the operand; the sum of squares, sqrt, divide and scale), B_row = max_c B(row, c)
  label                L64[row, got] >= max_c L64[row, c] - 2 B_row, for every row
  score                |score - p64[got]| <= p64[got] (2 B_row + (max_c |L64 - L64max| + 4) 2^-23 + (C1 - 1) 2^-24): the logit
                       differences, the exponential's argument scaling and rounding, the sum.
"""
import ctypes as C
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LVIS = os.path.join(ROOT, "tests", "golden", "lvis_v1_clip.npy")
N = 421                  # no multiple of 32, 64, 128 or 256: every tile size has a row tail
U = 2.0 ** -24
WIDTHS = [2, 21, 25, 33, 65, 81, 1204, 2048]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    from embodied_object_detection_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def class_matrix(C1: int) -> torch.Tensor:
    """[512, C1] through load_classifier (zero background column, unit columns): the first C1 - 1 LVIS rows; beyond LVIS' 1203 rows,
    normalised sums of two of them."""
    from embodied_object_detection_amd.modeling.utils import load_classifier
    rows = torch.tensor(np.load(LVIS), dtype=torch.float32)
    n = C1 - 1
    if n > rows.shape[0]:
        extra = rows + rows.roll(7, 0)
        rows = torch.cat([rows, extra / extra.norm(dim=1, keepdim=True)])
    return load_classifier(rows[:n].t().contiguous(), n)


def mp3d_matrix() -> torch.Tensor:
    from embodied_object_detection_amd import setup_cfg
    from embodied_object_detection_amd.modeling.utils import load_classifier
    return load_classifier(str(setup_cfg(None, []).MODEL.ROI_BOX_HEAD.ZEROSHOT_WEIGHT_PATH), 20)


def memory_rows(zs: torch.Tensor, n: int = N, seed: int = 0, zero_rows: int = 2):
    """mem [n, 512] f32, obs [n] f32: class-like rows (a text column + Gaussian noise of relative size 0.5 to 2, x 50, x an
    observation count of 1 to 40), Gaussian rows (randn x U(0, 30)), never-written rows (all zero); some rows rescaled to cover
    1e-3 to 1e4.  No subnormal-scale rows: the 1e-12 clamp is fp32-specific."""
    g = torch.Generator().manual_seed(seed)
    C = zs.shape[1] - 1
    kind = torch.arange(n) % 3                         # 0, 1: class-like, 2: Gaussian
    cols = torch.randint(0, C, (n,), generator=g)
    rel = 0.5 + 1.5 * torch.rand((n,), generator=g)
    noise = torch.randn((n, 512), generator=g) / 512 ** 0.5
    count = torch.randint(1, 41, (n,), generator=g).float()
    like = (zs[:, cols].t() + noise * rel[:, None]) * 50.0 * count[:, None]
    gauss = torch.randn((n, 512), generator=g) * (30.0 * torch.rand((n, 1), generator=g))
    mem = torch.where((kind == 2)[:, None], gauss, like)
    rescale = torch.rand((n,), generator=g) < 0.3
    # the row's new largest magnitude; the top scale comes twice, so that a threshold on the map's normalised intensity keeps some
    target = 10.0 ** torch.tensor([-3.0, -1.0, 1.0, 4.0, 4.0])[torch.randint(0, 5, (n,), generator=g)]
    mem = torch.where(rescale[:, None], mem / mem.abs().amax(dim=1, keepdim=True) * target[:, None], mem)
    zero = torch.randperm(n, generator=g)[:zero_rows]
    mem[zero] = 0.0
    obs = torch.randint(0, 5, (n,), generator=g).float()
    norms = mem.norm(dim=1)
    assert bool(((norms == 0) | (norms > 1e-4)).all())
    return mem.float().contiguous(), obs, zero


def reference(mem: torch.Tensor, zs: torch.Tensor):
    """float64 on the fp32 inputs -> L64 [n, C], B_row [n], p64 [n, C]."""
    x, z = mem.double(), zs.double()[:, :-1]
    xh = x / x.norm(dim=1, keepdim=True).clamp_min(1e-12)
    L = 50.0 * (xh @ z)
    B = 50.0 * U * (514.0 * (xh.abs() @ z.abs()) + 260.0 * (xh @ z).abs())
    return L, B.max(dim=1).values, torch.softmax(L, dim=1)


def near_ties(L: torch.Tensor, B_row: torch.Tensor) -> torch.Tensor:
    """Rows whose float64 top-2 gap is within 2 B_row: the only rows where an fp32 argmax may differ from the float64 one."""
    if L.shape[1] < 2:
        return torch.zeros((L.shape[0],), dtype=torch.bool)
    top = L.topk(2, dim=1).values
    return (top[:, 0] - top[:, 1]) <= 2.0 * B_row


def check_against_float64(labels, scores, mem, zs, tag):
    L, B_row, p = reference(mem, zs)
    C = L.shape[1]
    labels, scores = labels.cpu().long(), scores.cpu().double()
    assert int(labels.min()) >= 0 and int(labels.max()) < C, tag
    got_L = L.gather(1, labels[:, None])[:, 0]
    slack = got_L - (L.max(dim=1).values - 2.0 * B_row)
    ties = near_ties(L, B_row)
    flips = int((labels != L.argmax(dim=1)).sum())
    got_p = p.gather(1, labels[:, None])[:, 0]
    spread = (L - L.max(dim=1, keepdim=True).values).abs().max(dim=1).values
    bound = got_p * (2.0 * B_row + (spread + 4.0) * 2.0 ** -23 + C * 2.0 ** -24)
    err = (scores - got_p).abs()
    # the largest error/bound ratio is taken over the rows with a non-zero bound; a zero bound admits no error at all
    ratio = (err[bound > 0] / bound[bound > 0]).max().item() if bool((bound > 0).any()) else 0.0
    print(f"[{tag}] near-tie rows {int(ties.sum())}/{L.shape[0]}, labels != argmax64 {flips}, min label slack {slack.min().item():.3e}, "
          f"max B_row {B_row.max().item():.3e}, max score err {err.max().item():.3e}, max err/bound {ratio:.3e}")
    assert bool((slack >= 0).all()), (tag, "label is no epsilon-argmax", int((slack < 0).sum()))
    assert bool((err <= bound).all()), (tag, "score", int((err > bound).sum()))
    return ties


@pytest.mark.parametrize("C1", WIDTHS)
def test_labels_and_scores_against_float64(dev, C1):
    from embodied_object_detection_amd import ops
    zs = class_matrix(C1)
    mem, obs, _ = memory_rows(zs, seed=C1)
    L, B_row, _ = reference(mem, zs)
    ties = near_ties(L, B_row)
    assert ties.float().mean().item() <= 0.01, ("the reference itself leaves too many rows undecided", int(ties.sum()))
    labels, scores = ops.semmap_query(mem.to(dev), obs.to(dev), zs.to(dev), 0.0)
    assert labels.dtype == torch.int32 and scores.dtype == torch.float32 and labels.shape == scores.shape == (N,)
    check_against_float64(labels, scores, mem, zs, f"C1 = {C1}")


def test_equal_columns_give_the_lower_index(dev):
    """Pairs of identical text columns, in one panel (10, 20), across a panel boundary (30, 33), in two panels that two waves hold
    (5, 45) and in two panels of one wave and one lane (7, 263); rows aimed at them."""
    from embodied_object_detection_amd import ops
    zs = class_matrix(1204)
    pairs = [(5, 45), (30, 33), (10, 20), (7, 263)]
    for lo, hi in pairs:
        zs[:, hi] = zs[:, lo]
    g = torch.Generator().manual_seed(5)
    per = 25
    aim = torch.tensor([p[i % 2] for p in pairs for i in range(per)])
    want = torch.tensor([p[0] for p in pairs for _ in range(per)])
    noise = torch.randn((len(aim), 512), generator=g) / 512 ** 0.5
    mem = ((zs[:, aim].t() + 0.1 * noise) * 50.0 * torch.randint(1, 41, (len(aim), 1), generator=g)).float().contiguous()
    obs = torch.ones((len(aim),))
    L, B_row, _ = reference(mem, zs)
    top3 = L.topk(3, dim=1)
    assert bool((top3.values[:, 0] == top3.values[:, 1]).all()) and bool((top3.values[:, 1] - top3.values[:, 2] > 2 * B_row).all())
    labels, scores = ops.semmap_query(mem.to(dev), obs.to(dev), zs.to(dev), 0.0)
    assert torch.equal(labels.cpu().long(), want), (labels.cpu().tolist(), want.tolist())
    # and at a narrow width, where one wave holds every panel
    zs = class_matrix(81)
    for lo, hi in pairs[:3]:
        zs[:, hi] = zs[:, lo]
    keep = torch.arange(len(aim)) < 3 * per                 # the rows of the three pairs below column 80
    labels, _ = ops.semmap_query(mem[keep].contiguous().to(dev), obs[keep].to(dev), zs.to(dev), 0.0)
    L, B_row, _ = reference(mem[keep], zs)
    top3 = L.topk(3, dim=1)
    assert bool((top3.values[:, 0] == top3.values[:, 1]).all()) and bool((top3.values[:, 1] - top3.values[:, 2] > 2 * B_row).all())
    assert torch.equal(labels.cpu().long(), want[keep])


@pytest.mark.parametrize("C1", [21, 1204, 2048])
def test_never_written_rows(dev, C1):
    from embodied_object_detection_amd import ops
    zs = class_matrix(C1)
    mem, obs, zero = memory_rows(zs, seed=3, zero_rows=9)
    labels, scores = ops.semmap_query(mem.to(dev), obs.to(dev), zs.to(dev), 0.0)
    labels, scores = labels.cpu(), scores.cpu().double()
    C = C1 - 1
    assert bool((labels[zero] == 0).all())
    assert bool(((scores[zero] - 1.0 / C).abs() <= (1.0 / C) * (4.0 * 2.0 ** -23 + C * 2.0 ** -24)).all()), scores[zero].tolist()


def test_one_class_is_certain(dev):
    from embodied_object_detection_amd import ops
    zs = class_matrix(2)
    mem, obs, _ = memory_rows(zs, seed=2, zero_rows=5)
    labels, scores = ops.semmap_query(mem.to(dev), obs.to(dev), zs.to(dev), 0.0)
    assert bool((labels == 0).all()) and bool((scores == 1.0).all())


def _raw_call(dev, mem, obs, zs, thresh, flag, labels=None, ws=None):
    """The C entry point with buffers of the test's own: (labels [n] i32, workspace [2 n + 4] f32)."""
    from embodied_object_detection_amd import _lib
    n = mem.shape[0]
    labels = torch.full((n,), -7, dtype=torch.int32, device=dev) if labels is None else labels
    ws = torch.full((2 * n + 4,), -7.0, dtype=torch.float32, device=dev) if ws is None else ws
    st = _lib.load().eod_semmap_labels(mem.data_ptr(), obs.data_ptr(), zs.data_ptr(), n, 512 | (_lib.SEMMAP_SCORES if flag else 0),
                                       zs.shape[1], C.c_float(thresh), labels.data_ptr(), ws.data_ptr(),
                                       torch.cuda.current_stream().cuda_stream)
    assert st == 0, st
    torch.cuda.synchronize()
    return labels, ws


@pytest.mark.parametrize("C1", [21, 1204])
def test_flagged_call_against_the_plain_call(dev, C1):
    zs = mp3d_matrix() if C1 == 21 else class_matrix(C1)
    assert zs.shape[1] == C1
    mem, obs, _ = memory_rows(zs, seed=7)
    ties = near_ties(*reference(mem, zs)[:2])
    d_mem, d_obs, d_zs = mem.to(dev), obs.to(dev), zs.to(dev)
    lab_p, ws_p = _raw_call(dev, d_mem, d_obs, d_zs, 0.4, False)
    lab_q, ws_q = _raw_call(dev, d_mem, d_obs, d_zs, 0.4, True)
    assert torch.equal(ws_p[:2].view(torch.int32), ws_q[:2].view(torch.int32))                    # the map's min / max
    assert torch.equal(ws_p[4:4 + N].view(torch.int32), ws_q[4:4 + N].view(torch.int32)), "intensities differ"
    assert bool((ws_p[4 + N:] == -7.0).all()), "the plain call wrote beyond n_cells + 4 floats"
    lab_p, lab_qc = lab_p.cpu(), lab_q.cpu()
    assert torch.equal(lab_p == -1, lab_qc == -1)
    assert bool((lab_p == -1).any()) and bool((lab_p >= 0).any())
    both = (lab_p >= 0) & ~ties
    assert torch.equal(lab_p[both], lab_qc[both])
    # the same with nothing thresholded: every row outside the near-tie set
    lab_p0, _ = _raw_call(dev, d_mem, d_obs, d_zs, 0.0, False)
    lab_q0, ws_q0 = _raw_call(dev, d_mem, d_obs, d_zs, 0.0, True)
    assert int(lab_p0.min()) >= 0 and torch.equal(lab_p0.cpu()[~ties], lab_q0.cpu()[~ties])
    assert torch.equal(ws_q0[4 + N:].view(torch.int32), ws_q[4 + N:].view(torch.int32)), "the threshold touched the scores"
    check_against_float64(lab_q0, ws_q0[4 + N:], mem, zs, f"flagged, C1 = {C1}")
    # a second flagged call into the same buffers
    first = (lab_q.clone(), ws_q.clone())
    _raw_call(dev, d_mem, d_obs, d_zs, 0.4, True, labels=lab_q, ws=ws_q)
    assert torch.equal(first[0], lab_q) and torch.equal(first[1].view(torch.int32), ws_q.view(torch.int32))


def test_query_refuses_what_the_kernel_cannot_hold(dev):
    from embodied_object_detection_amd import _lib, ops
    mem, obs = torch.zeros((8, 512), device=dev), torch.zeros((8,), device=dev)
    with pytest.raises(_lib.EodError):
        ops.semmap_query(mem, obs, torch.zeros((512, 2049), device=dev), 0.0)
    with pytest.raises(_lib.EodError):
        ops.semmap_query(mem, obs, torch.zeros((2049, 512), device=dev).t(), 0.0)


# ---- the models ---------------------------------------------------------------------------------------------------------------
def _frames(n, seed=0, H=128, W=160):
    from embodied_object_detection_amd.data.synthetic import SyntheticSequence
    seq = SyntheticSequence(seed, H=H, W=W, n_frames=n, map_w=24, map_h=24, cell=0.5)
    return [seq.frame(i) for i in range(n)]


def _cfg(*extra):
    from embodied_object_detection_amd import setup_cfg
    return setup_cfg(None, ["MODEL.MEMORY_TYPE", "implicit_memory", "MODEL.MAP_FEAT_FUSION", "sum", "MODEL.MAP_FEATURE_WEIGHT", 5,
                            "MODEL.MEMORY_CLS_SCORE_THRESH", 0.3, *extra])


def _out(model, f):
    o = model([[f]])[0]["instances"]
    return o.pred_boxes.tensor.clone(), o.scores.clone(), o.pred_classes.clone(), o.pred_masks.clone()


@pytest.fixture(scope="module")
def single_runs(dev, synthetic_sd):
    """Per seed: the single-scene model after two frames and its LVIS query (labels, scores)."""
    from embodied_object_detection_amd import build_model
    runs = {}
    for seed in (0, 1):
        model = build_model(_cfg(), synthetic_sd)
        frames = _frames(3, seed)
        for f in frames[:2]:
            model([[f]])
        lab, sc = model.semantic_map(classifier=LVIS, num_classes=1203, scores=True)
        runs[seed] = dict(model=model, frames=frames, labels=lab.clone(), scores=sc.clone())
    return runs


def test_model_query_equals_the_op_and_changes_nothing(dev, synthetic_sd, single_runs):
    from embodied_object_detection_amd import build_model, ops
    from embodied_object_detection_amd.modeling.utils import load_classifier
    run = single_runs[0]
    model, frames = run["model"], run["frames"]
    before = dict(semmap=model.semmap, zs=model.zs_weight, zs_val=model.zs_weight.clone(), heads=[st["zs"] for st in model.roi_heads.stages],
                  heads_val=model.roi_heads.stages[0]["zs"].clone(), mem=model.implicit_memory.clone(), obs=model.observations.clone())
    lab, sc = model.semantic_map(classifier=LVIS, num_classes=1203, scores=True)
    zs = load_classifier(LVIS, 1203).to(dev)
    ref_lab, ref_sc = ops.semmap_query(model.implicit_memory, model.observations, zs, model.obs_score_thresh)
    assert torch.equal(lab, ref_lab) and torch.equal(sc, ref_sc) and torch.equal(lab, run["labels"]) and torch.equal(sc, run["scores"])
    assert int(lab.max()) < 1203 and bool((lab >= 0).any()) and bool(((sc > 0) & (sc <= 1)).all())
    # a tensor, a width read off the matrix, another threshold, the model's own vocabulary
    lab_t, sc_t = model.semantic_map(classifier=torch.tensor(np.load(LVIS), dtype=torch.float32).t(), thresh=0.0)
    assert torch.equal(sc_t, sc) and int(lab_t.min()) >= 0 and torch.equal(lab_t[lab >= 0], lab[lab >= 0])
    own_lab, own_sc = model.semantic_map(scores=True)
    ref_own = ops.semmap_query(model.implicit_memory, model.observations, model.zs_weight, model.obs_score_thresh)
    assert torch.equal(own_lab, ref_own[0]) and torch.equal(own_sc, ref_own[1]) and int(own_lab.max()) < 20
    assert model.semmap is before["semmap"] and model.zs_weight is before["zs"] and torch.equal(model.zs_weight, before["zs_val"])
    assert all(st["zs"] is z for st, z in zip(model.roi_heads.stages, before["heads"]))
    assert torch.equal(model.roi_heads.stages[0]["zs"], before["heads_val"]) and model.roi_heads.num_classes == 20
    assert torch.equal(model.implicit_memory, before["mem"]) and torch.equal(model.observations, before["obs"])
    # the plain call is still the plain call
    plain = model.semantic_map()
    assert plain is model.semmap
    assert torch.equal(plain, ops.semmap_labels(model.implicit_memory, model.observations, model.zs_weight, model.obs_score_thresh))
    # frame 3 after the queries against a run that never asked
    other = build_model(_cfg(), synthetic_sd)
    for f in frames[:2]:
        other([[f]])
    for a, b in zip(_out(other, frames[2]), _out(model, frames[2])):
        assert torch.equal(a, b)
    assert torch.equal(other.implicit_memory, model.implicit_memory)


def test_lockstep_query_equals_the_single_scene_runs(dev, synthetic_sd, single_runs):
    from embodied_object_detection_amd.modeling.lockstep import LockstepScenes
    ls = LockstepScenes(_cfg(), 2, synthetic_sd)
    ls([list(single_runs[0]["frames"][:2]), list(single_runs[1]["frames"][:2])])
    for b in (0, 1):
        lab, sc = ls.semantic_map(b, classifier=LVIS, num_classes=1203, scores=True)
        assert torch.equal(lab, single_runs[b]["labels"]) and torch.equal(sc, single_runs[b]["scores"]), f"scene {b}"
    from embodied_object_detection_amd import ops
    m = ls.model
    assert torch.equal(ls.semantic_map(1), ops.semmap_labels(ls.implicit_memory[1], ls.observations[1], m.zs_weight, m.obs_score_thresh))
    with pytest.raises(IndexError):
        ls.semantic_map(2, scores=True)
    with pytest.raises(NotImplementedError):
        LockstepScenes(_cfg("MODEL.TEST_SAVE_SEMMAP", True), 2, synthetic_sd)


def test_predictor_query(dev, synthetic_sd):
    from embodied_object_detection_amd.engine.predictor import EmbodiedPredictor
    pred = EmbodiedPredictor(_cfg(), synthetic_sd)
    for f in _frames(2):
        pred.model([[f]])
    out = pred.semantic_map(classifier=LVIS)
    lab, sc = pred.model.semantic_map(classifier=LVIS, num_classes=1203, scores=True)
    assert sorted(out) == ["labels", "scores"] and torch.equal(out["labels"], lab) and torch.equal(out["scores"], sc)
    own = pred.semantic_map(vocabulary="mp3d", thresh=0.0)
    assert int(own["labels"].min()) >= 0 and int(own["labels"].max()) < 20
