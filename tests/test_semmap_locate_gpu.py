"""Where on the map a queried class is (EOD_SEMMAP_LOCATE / EOD_SEMMAP_PEAKS on `eod_semmap_labels`, `ops.semmap_locate`,
`locate` on the models): the probability maps against float64, their bitwise ties to the SCORES call, the peaks against the exact
reference of `_locate_cases.py` on the call's own maps, the workspace's bounds, and the Python surface.

N = 19 x 23 = 437 cells: six full 64-row tiles and a tail of 53, no multiple of 32.  Widths 21, 33, 1204, 2048: the gathered panel
then runs on wave 1, 2, 6 and 0, as the only, the second or a later panel of its wave.

Bound of a queried probability (u = 2^-24; L, B_row, p64 as in test_semmap_query_gpu.py): `_locate_cases.prob_bound`,
p64 (4 B_row + 2 (spread + 4) 2^-23 + C 2^-24) + 2^-126.  It is loose (about 0.85 % relative), so the layout of the extra panel is
carried by the bitwise test: prob[q, i] is scores[i], bit for bit, wherever labels[i] is the queried class.
"""
import numpy as np
import pytest
import torch

from _locate_cases import aimed_rows, peak_flags, peaks_reference, prob_bound, query_classes
from test_semmap_query_gpu import LVIS, class_matrix, memory_rows, mp3d_matrix, reference

pytestmark = pytest.mark.gpu

ROWS, COLS = 19, 23
N = ROWS * COLS
WIDTHS = [21, 33, 1204, 2048]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    from embodied_object_detection_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


_CASES = {}


def case(C1, dev):
    """Per width, computed once and left unchanged: the matrix, the memory, the float64 reference, the queried classes."""
    if C1 not in _CASES:
        zs = class_matrix(C1)
        mem, obs, zero = memory_rows(zs, n=N, seed=C1, zero_rows=4)
        L, B_row, p64 = reference(mem, zs)
        _CASES[C1] = dict(zs=zs, mem=mem, obs=obs, zero=zero, L=L, B_row=B_row, p64=p64, classes=query_classes(L, C1),
                          d=(mem.to(dev), obs.to(dev), zs.to(dev)))
    return _CASES[C1]


def bits(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize("C1", WIDTHS)
def test_prob_against_float64(dev, C1):
    from embodied_object_detection_amd import ops
    c = case(C1, dev)
    classes = c["classes"]
    assert 8 <= len(classes) <= 9 and 0 in classes and C1 - 2 in classes
    out = ops.semmap_locate(*c["d"], classes, 0.0, cols=COLS)
    prob = out["prob"]
    assert prob.dtype == torch.float32 and prob.shape == (len(classes), N)
    assert out["labels"].dtype == torch.int32 and out["labels"].shape == out["scores"].shape == (N,)
    want = c["p64"][:, classes].t()
    bound = prob_bound(c["L"], c["B_row"], c["p64"], classes)
    err = (prob.cpu().double() - want).abs()
    print(f"[C1 = {C1}] classes {classes}, max err/bound {(err / bound).max().item():.3e}, max err {err.max().item():.3e}, "
          f"max bound/p64 {((bound - 2.0 ** -126) / want).max().item():.3e}")
    assert bool(torch.isfinite(prob).all())
    assert bool((err <= bound).all()), (int((err > bound).sum()), (err / bound).max().item())        # every cell, every class


@pytest.mark.parametrize("C1", WIDTHS)
def test_bitwise_ties_to_the_scores_call(dev, C1):
    from embodied_object_detection_amd import ops
    c = case(C1, dev)
    classes = c["classes"]
    out0 = {k: v.clone() for k, v in ops.semmap_locate(*c["d"], classes, 0.0, cols=COLS).items()}
    out4 = {k: v.clone() for k, v in ops.semmap_locate(*c["d"], classes, 0.4, cols=COLS).items()}
    for out, thresh in ((out0, 0.0), (out4, 0.4)):
        lab, sc = ops.semmap_query(*c["d"], thresh)
        assert torch.equal(out["labels"], lab) and torch.equal(bits(out["scores"]), bits(sc)), thresh
    # where the queried class is the cell's label, its probability is the cell's score
    lab, sc, prob = out0["labels"].cpu().long(), out0["scores"].cpu(), out0["prob"].cpu()
    assert int(lab.min()) >= 0
    hits = 0
    for q, cls in enumerate(classes):
        own = lab == cls
        hits += int(own.sum())
        assert torch.equal(bits(prob[q, own]), bits(sc[own])), (cls, int(own.sum()))
        assert bool((prob[q] <= sc).all()), cls                                  # no class above the argmax's
    assert hits >= 8, hits                                                       # the frequent classes and column 0 (the zero rows)
    # never-written rows: one bit pattern across cells and classes, the score's
    zero = c["zero"]
    assert len(zero) == 4 and bool((lab[zero] == 0).all())
    assert len(set(bits(prob[:, zero]).flatten().tolist()) | set(bits(sc[zero]).tolist())) == 1
    # the threshold: exactly the cells labelled -1 are 0 in every row, every other bit is unchanged
    lab4, prob4 = out4["labels"].cpu(), out4["prob"].cpu()
    gone = lab4 == -1
    assert bool(gone.any()) and bool((~gone).any())
    assert torch.equal((prob4 == 0).all(dim=0), gone)
    assert bool((prob4[:, gone] == 0).all()) and torch.equal(bits(prob4[:, ~gone]), bits(prob[:, ~gone]))
    assert torch.equal(lab4[~gone].long(), lab[~gone])


def _check_peaks(out, cols, radius, K, tag):
    prob = out["prob"].cpu().numpy()
    want_p, want_s = peaks_reference(prob, cols, radius, K)
    got_p, got_s = out["peaks"].cpu().numpy(), out["peak_scores"].cpu().numpy()
    assert got_p.dtype == np.int32 and got_s.dtype == np.float32 and got_p.shape == got_s.shape == (prob.shape[0], K), tag
    assert np.array_equal(got_p, want_p), (tag, got_p.tolist(), want_p.tolist())
    assert np.array_equal(got_s.view(np.int32), want_s.view(np.int32)), tag
    return want_p


@pytest.mark.parametrize("cols", [COLS, ROWS])
@pytest.mark.parametrize("radius", [0, 1, 3])
def test_peaks_are_exact(dev, cols, radius):
    from embodied_object_detection_amd import ops
    c = case(1204, dev)
    for K in (1, 8, 16):
        for thresh in (0.0, 0.4):
            out = ops.semmap_locate(*c["d"], c["classes"], thresh, cols=cols, radius=radius, topk=K)
            want = _check_peaks(out, cols, radius, K, f"cols {cols} radius {radius} K {K} thresh {thresh}")
            if thresh == 0.0 and radius <= 1:
                assert int((want >= 0).sum()) == want.size                       # more than 16 peaks per class; radius 3: 8 to 14, padded
    if radius == 0:                                                              # no grid named: the plain top-K
        out = ops.semmap_locate(*c["d"], c["classes"], 0.0, topk=8)
        _check_peaks(out, None, 0, 8, "cols None")
        assert torch.equal(out["peaks"], ops.semmap_locate(*c["d"], c["classes"], 0.0, cols=cols, radius=0, topk=8)["peaks"])


def test_a_plateau_gives_its_lowest_cell(dev):
    """Nine never-written rows as a 3 x 3 block among rows aimed at classes 0..9; class 15, which no row is aimed at, is most likely
    (1 / C, equal bits) on the block, and its first cell is the peak."""
    from embodied_object_detection_amd import ops
    zs = mp3d_matrix()
    mem, obs = aimed_rows(zs, N, list(range(10)), seed=1)
    block = [(r, cc) for r in (7, 8, 9) for cc in (11, 12, 13)]
    for cols in (COLS, ROWS):
        cells = [r * cols + cc for r, cc in block]
        m = mem.clone()
        m[cells] = 0.0
        for radius in (1, 3):
            out = ops.semmap_locate(m.to(dev), obs.to(dev), zs.to(dev), [15, 3], 0.0, cols=cols, radius=radius, topk=8)
            want = _check_peaks(out, cols, radius, 8, f"plateau cols {cols} radius {radius}")
            prob = out["prob"].cpu()
            assert len(set(bits(prob[0, cells]).tolist())) == 1
            assert int(out["peaks"][0, 0]) == cells[0] == int(want[0, 0]), (out["peaks"][0].tolist(), cells)
            assert bits(out["peak_scores"][0, :1].cpu()).item() == bits(prob[0, cells[:1]]).item()
            assert not set(out["peaks"][0].tolist()) & set(cells[1:])
            flags = peak_flags(prob[0].numpy(), cols, radius)
            assert flags[cells[0]] and not flags[cells[1:]].any()


def test_padding_one_class_and_thirty_two(dev):
    from embodied_object_detection_amd import ops
    zs = class_matrix(33)
    mem, obs, _ = memory_rows(zs, n=35, seed=11, zero_rows=1)
    d = (mem.to(dev), obs.to(dev), zs.to(dev))
    # 5 x 7, radius 2: two peaks are at least 3 apart in a row or a column, so at most 2 x 3 = 6 of them
    for classes in ([4], [(5 * i) % 32 for i in range(16)] * 2):
        out = ops.semmap_locate(*d, classes, 0.0, cols=7, radius=2, topk=8)
        assert out["prob"].shape == (len(classes), 35)
        want = _check_peaks(out, 7, 2, 8, f"5 x 7, Q = {len(classes)}")
        assert bool((out["peaks"][:, 6:] == -1).all()) and bool((out["peak_scores"][:, 6:] == 0.0).all())
        assert bool((out["peaks"][:, 0] >= 0).all()) and int((want >= 0).sum(axis=1).max()) <= 6
    prob = out["prob"].cpu()                                                     # the duplicates: rows q and q + 16 are one query
    assert torch.equal(bits(prob[:16]), bits(prob[16:])) and torch.equal(out["peaks"][:16], out["peaks"][16:])
    one = ops.semmap_locate(*d, [classes[3]], 0.0, cols=7, radius=2, topk=8)
    assert torch.equal(bits(one["prob"].cpu()[0]), bits(prob[3])) and torch.equal(one["peaks"][0], out["peaks"][3])


def test_workspace_bounds_and_determinism(dev):
    from embodied_object_detection_amd import ops
    c = case(1204, dev)
    classes, K = c["classes"], 16
    need = ops.semmap_locate_workspace(N, len(classes), K)
    assert need == 4 + 2 * N + 32 + 2 * len(classes) * N + 2 * len(classes) * K
    ws = torch.full((need + 64,), -7.0, dtype=torch.float32, device=dev)
    out = ops.semmap_locate(*c["d"], classes, 0.4, cols=COLS, radius=1, topk=K, workspace=ws)
    assert bool((ws[need:] == -7.0).all()), "the call wrote behind its workspace"
    assert out["prob"].data_ptr() == ws.data_ptr() + 4 * (4 + 2 * N + 32)
    first_ws, first_lab = ws.clone(), out["labels"].clone()
    again = ops.semmap_locate(*c["d"], classes, 0.4, cols=COLS, radius=1, topk=K, workspace=ws)
    assert torch.equal(bits(first_ws), bits(ws)) and torch.equal(first_lab, again["labels"])
    fresh = ops.semmap_locate(*c["d"], classes, 0.4, cols=COLS, radius=1, topk=K)
    for k in ("labels", "scores", "prob", "peaks", "peak_scores"):
        assert torch.equal(bits(fresh[k]) if fresh[k].dtype == torch.float32 else fresh[k],
                           bits(again[k]) if again[k].dtype == torch.float32 else again[k]), k


def test_locate_refuses_on_the_host(dev):
    from embodied_object_detection_amd import _lib, ops
    c = case(21, dev)
    d = c["d"]
    ok = dict(thresh=0.0, cols=COLS, radius=1, topk=8)
    bad = [dict(classes=[]), dict(classes=list(range(20)) + list(range(13))), dict(classes=[20]), dict(classes=[-1]),
           dict(classes=[3], cols=20), dict(classes=[3], cols=0), dict(classes=[3], radius=4), dict(classes=[3], radius=-1),
           dict(classes=[3], topk=0), dict(classes=[3], topk=17),
           dict(classes=[3], workspace=torch.zeros((ops.semmap_locate_workspace(N, 1, 8) - 1,), device=dev))]
    for kw in bad:
        args = {**ok, **kw}
        with pytest.raises(_lib.EodError):
            ops.semmap_locate(*d, args.pop("classes"), args.pop("thresh"), **args)
    mem, obs = d[0], d[1]
    with pytest.raises(_lib.EodError):
        ops.semmap_locate(mem, obs, torch.zeros((512, 2049), device=dev), [3], 0.0)
    with pytest.raises(_lib.EodError):
        ops.semmap_locate(mem, obs, torch.zeros((2049, 512), device=dev).t(), [3], 0.0)
    out = ops.semmap_locate(*d, torch.tensor([19, 0, 19]), 0.0, cols=COLS)       # the ends of the range, a tensor, a duplicate
    assert out["prob"].shape == (3, N)


# ---- the models ---------------------------------------------------------------------------------------------------------------
MAP = (24, 24)
QUERY = [3, 77, 1202, 0, 77]


def _frames(n, seed=0, H=128, W=160):
    from embodied_object_detection_amd.data.synthetic import SyntheticSequence
    seq = SyntheticSequence(seed, H=H, W=W, n_frames=n, map_w=24, map_h=24, cell=0.5)
    return [seq.frame(i) for i in range(n)]


def _cfg():
    from embodied_object_detection_amd import setup_cfg
    return setup_cfg(None, ["MODEL.MEMORY_TYPE", "implicit_memory", "MODEL.MAP_FEAT_FUSION", "sum", "MODEL.MAP_FEATURE_WEIGHT", 5,
                            "MODEL.MEMORY_CLS_SCORE_THRESH", 0.3])


def _out(model, f):
    o = model([[f]])[0]["instances"]
    return o.pred_boxes.tensor.clone(), o.scores.clone(), o.pred_classes.clone(), o.pred_masks.clone()


def _same(a, b):
    assert sorted(a) == sorted(b) == ["labels", "peak_scores", "peaks", "prob", "scores"]
    for k in a:
        assert a[k].shape == b[k].shape and a[k].dtype == b[k].dtype, k
        assert torch.equal(bits(a[k]) if a[k].dtype == torch.float32 else a[k], bits(b[k]) if b[k].dtype == torch.float32 else b[k]), k


@pytest.fixture(scope="module")
def single_runs(dev, synthetic_sd):
    """Per seed: the single-scene model after two frames and its LVIS locate."""
    from embodied_object_detection_amd import build_model
    runs = {}
    for seed in (0, 1):
        model = build_model(_cfg(), synthetic_sd)
        frames = _frames(3, seed)
        for f in frames[:2]:
            model([[f]])
        out = model.locate(QUERY, classifier=LVIS, num_classes=1203, map_shape=MAP)
        runs[seed] = dict(model=model, frames=frames, out={k: v.clone() for k, v in out.items()})
    return runs


def test_model_locate_equals_the_op_and_changes_nothing(dev, synthetic_sd, single_runs):
    from embodied_object_detection_amd import _lib, build_model, ops
    from embodied_object_detection_amd.modeling.utils import load_classifier
    run = single_runs[0]
    model, frames = run["model"], run["frames"]
    before = dict(semmap=model.semmap, zs=model.zs_weight, zs_val=model.zs_weight.clone(), heads=[st["zs"] for st in model.roi_heads.stages],
                  mem=model.implicit_memory.clone(), obs=model.observations.clone())
    out = model.locate(QUERY, classifier=LVIS, num_classes=1203, map_shape=MAP)
    zs = load_classifier(LVIS, 1203).to(dev)
    _same(out, ops.semmap_locate(model.implicit_memory, model.observations, zs, QUERY, model.obs_score_thresh, cols=24, radius=1, topk=8))
    _same(out, run["out"])
    assert out["prob"].shape == (5, 576) and bool((out["peaks"][:, 0] >= 0).all()) and bool(((out["prob"] >= 0) & (out["prob"] <= 1)).all())
    lab, sc = model.semantic_map(classifier=LVIS, num_classes=1203, scores=True)
    assert torch.equal(out["labels"], lab) and torch.equal(out["scores"], sc)
    # the model's own vocabulary, another threshold, no grid
    own = model.locate([0, 19], thresh=0.0, topk=4, radius=0)
    _same(own, ops.semmap_locate(model.implicit_memory, model.observations, model.zs_weight, [0, 19], 0.0, topk=4))
    with pytest.raises(_lib.EodError):
        model.locate([3], map_shape=(24, 23))
    with pytest.raises(_lib.EodError):
        build_model(_cfg(), synthetic_sd).locate([3])                            # no memory yet
    assert model.semmap is before["semmap"] and model.zs_weight is before["zs"] and torch.equal(model.zs_weight, before["zs_val"])
    assert all(st["zs"] is z for st, z in zip(model.roi_heads.stages, before["heads"])) and model.roi_heads.num_classes == 20
    assert torch.equal(model.implicit_memory, before["mem"]) and torch.equal(model.observations, before["obs"])
    # frame 3 after the queries against a run that never asked
    other = build_model(_cfg(), synthetic_sd)
    for f in frames[:2]:
        other([[f]])
    for a, b in zip(_out(other, frames[2]), _out(model, frames[2])):
        assert torch.equal(a, b)
    assert torch.equal(other.implicit_memory, model.implicit_memory)


def test_lockstep_locate_equals_the_single_scene_runs(dev, synthetic_sd, single_runs):
    from embodied_object_detection_amd.modeling.lockstep import LockstepScenes
    ls = LockstepScenes(_cfg(), 2, synthetic_sd)
    ls([list(single_runs[0]["frames"][:2]), list(single_runs[1]["frames"][:2])])
    for b in (0, 1):
        _same(ls.locate(b, QUERY, classifier=LVIS, num_classes=1203, map_shape=MAP), single_runs[b]["out"])
    with pytest.raises(IndexError):
        ls.locate(2, QUERY)


def test_predictor_locate(dev, synthetic_sd):
    from embodied_object_detection_amd.engine.predictor import EmbodiedPredictor
    pred = EmbodiedPredictor(_cfg(), synthetic_sd)
    for f in _frames(2):
        pred.model([[f]])
    out = pred.locate(QUERY, classifier=LVIS, map_shape=MAP)
    _same(out, pred.model.locate(QUERY, classifier=LVIS, num_classes=1203, map_shape=MAP))
    own = pred.locate([0, 19], vocabulary="mp3d", thresh=0.0)
    assert own["prob"].shape == (2, 576) and own["peaks"].shape == (2, 8)
