"""The map inventory (`eod_map_inventory`, `ops.map_inventory`, `inventory` on the models) against the exact reference of
`_inventory_cases.py`: every output, every cell, every slot, every class, for equality.  There is no tolerance anywhere: the op is
integers and comparisons, and `peak_score` is compared by its bits.

The hostile maps of one grid are the maps of one [B, N] call (a different map per b, so a wrong map stride shows), under both
connectivities; the two that need a `keep` table are calls of their own.  Grids: 19 x 23 (one ragged tile) and 33 x 65 (two by three
tiles with ragged edges), one 96 x 96 and one 200 x 200 call."""
import os

import numpy as np
import pytest
import torch

import _inventory_cases as IC
import _regions_cases as RC

pytestmark = pytest.mark.gpu

LEVEL = IC.LEVEL
LVIS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lvis_v1_clip.npy")
GRIDS = {"19x23": (19, 23), "33x65": (33, 65)}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    from embodied_object_detection_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


_MAPS = {}


def maps_of(name):
    """The hostile maps of a grid, made once and left unchanged: {name: (labels, scores, keep)}."""
    if name not in _MAPS:
        from embodied_object_detection_amd import ops
        _MAPS[name] = IC.hostile_maps(*GRIDS[name], ops.REGIONS_TILE_ROWS, ops.REGIONS_TILE_COLS, level=LEVEL)
    return _MAPS[name]


def bits(a):
    return a.view(np.int32) if a.dtype == np.float32 else a


def check(out, labels, scores, cols, C, level, conn, min_cells, topk, tag, keep=None, names=None):
    """Every output of the op on [B, N] maps against the reference, for equality; status 0; the types and shapes of the interface."""
    ref = IC.reference(labels, scores, cols, C, level, conn, min_cells, topk, keep)
    got = {k: v.cpu().numpy() for k, v in out.items()}
    assert sorted(got) == sorted(IC.KEYS + ("status",)), sorted(got)
    assert got["status"].dtype == np.int32 and got["status"].tolist() == [0], (tag, got["status"])
    for k in IC.KEYS:
        assert got[k].dtype == ref[k].dtype and got[k].shape == ref[k].shape, (tag, k, got[k].dtype, got[k].shape, ref[k].shape)
        same = bits(got[k]) == bits(ref[k])
        if not same.all():
            b = int(np.argwhere(~same)[0][0])
            raise AssertionError(f"{tag}: {k} differs in {int((~same).sum())} places, first in map {b}"
                                 f"{' (' + names[b] + ')' if names else ''}: got {got[k][b].reshape(-1)[:16].tolist()}, "
                                 f"want {ref[k][b].reshape(-1)[:16].tolist()}")
    return ref


def run(dev, labels, scores, cols, C, level=LEVEL, conn=8, min_cells=1, topk=16, keep=None, tag="", names=None, **kw):
    from embodied_object_detection_amd import ops
    dl, ds = torch.from_numpy(labels).to(dev), torch.from_numpy(scores).to(dev)
    dk = None if keep is None else torch.from_numpy(keep).to(dev)
    out = ops.map_inventory(dl, ds, cols, C, level=level, connectivity=conn, min_cells=min_cells, topk=topk, keep=dk, **kw)
    ref = check(out, labels, scores, cols, C, level, conn, min_cells, topk, tag, keep, names)
    assert torch.equal(dl, torch.from_numpy(labels).to(dev)) and torch.equal(ds.view(torch.int32), torch.from_numpy(scores).to(dev).view(torch.int32))
    return out, ref


@pytest.mark.parametrize("conn", [4, 8])
@pytest.mark.parametrize("grid", list(GRIDS))
def test_hostile_maps_equal_the_reference(dev, grid, conn):
    rows, cols = GRIDS[grid]
    N = rows * cols
    maps = maps_of(grid)
    plain = [n for n, m in maps.items() if m[2] is None]
    assert 15 < len(plain) <= 32 and ("corner, both diagonals" in plain) == (grid != "19x23")
    labels, scores = np.stack([maps[n][0] for n in plain]), np.stack([maps[n][1] for n in plain])
    out, ref = run(dev, labels, scores, cols, IC.C5, conn=conn, tag=f"{grid} conn {conn}", names=plain)
    cnt = dict(zip(plain, ref["count"].tolist()))
    print(f"[{grid}, {conn}] objects: {cnt}")
    b = plain.index("checkerboard")
    assert cnt["checkerboard"] == (2 if conn == 8 else N) and ref["class_objects"][b].tolist() == ([0, 1, 0, 1, 0] if conn == 8 else
                                                                                                   [0, (N + 1) // 2, 0, N // 2, 0])
    stripes = -(-cols // 32)
    assert cnt["column stripes"] == stripes and cnt["row stripes"] == -(-rows // 32) and cnt["row-end pair"] == 2
    assert cnt["one class everywhere"] == 1 and cnt["all background"] == 0 and cnt["below the level"] == 0 and cnt["at the level"] > 0
    assert cnt["serpentine"] > 4 and cnt["spirals"] > 4 and cnt["equal areas"] > 16 and cnt["bernoulli 0.3"] > 64
    if grid != "19x23":
        for name in ("corner, both diagonals", "corner, class all around"):
            b = plain.index(name)
            assert cnt[name] == (2 if conn == 8 else 4) and ref["cls"][b, :2].tolist() == ([2, 4] if conn == 8 else [2, 4])
            assert ref["area"][b, :2].tolist() == ([2, 2] if conn == 8 else [1, 1])
    b = plain.index("all background")
    for k in IC.KEYS:
        assert (out[k][b].cpu().numpy() == (-1 if k in ("object", "cls", "object_labels", "class_largest") else 0)).all(), k
    # min_cells above some areas, and a ranking shorter than the count
    run(dev, labels, scores, cols, IC.C5, conn=conn, min_cells=3, topk=4, tag=f"{grid} conn {conn} min_cells 3", names=plain)
    # the keep tables: a call per table
    for name in ("keep cuts", "keep on random classes"):
        lab, sc, keep = maps[name]
        _, r = run(dev, lab[None], sc[None], cols, IC.C5, conn=conn, keep=keep, tag=f"{grid} conn {conn} {name}")
        _, r0 = run(dev, lab[None], sc[None], cols, IC.C5, conn=conn, tag=f"{grid} conn {conn} {name}, no table")
        assert r["foreground"][0] < r0["foreground"][0]
        if name == "keep cuts":
            assert r["count"][0] == 2 and r0["count"][0] == 3 and r["class_cells"][0].tolist() == [N - rows, 0, 0, 0, 0]


def _drawn(rows, cols, classes, p, seed):
    """A map whose cells draw their class from `classes`, with a Bernoulli(p) foreground."""
    pick = np.asarray(classes, np.int32)[np.random.default_rng(seed).integers(0, len(classes), rows * cols)]
    return pick, RC.paint(RC.bernoulli(rows, cols, p, seed=seed + 1), LEVEL, seed=seed)


@pytest.mark.parametrize("B", [1, 3])
def test_call_shapes(dev, B):
    """B = 1, 3 with a map of its own per b; C = 1, 5, 2047; topk 1, 16, 64; min_cells 1 and 3; both connectivities."""
    rows, cols = 33, 65
    for C, classes in ((1, [0, 1, -1]), (5, [0, 1, 2, 3, 4, 5]), (2047, [0, 1000, 2046, 2047]), (2047, list(range(2047)))):
        maps = [_drawn(rows, cols, classes, (0.5, 0.8, 0.95)[b], seed=1000 + 10 * b + C) for b in range(B)]
        labels, scores = np.stack([m[0] for m in maps]), np.stack([m[1] for m in maps])
        for conn, topk, min_cells in ((4, 1, 1), (8, 16, 1), (8, 64, 3), (4, 64, 1), (8, 1, 3), (4, 16, 3)):
            _, ref = run(dev, labels, scores, cols, C, conn=conn, topk=topk, min_cells=min_cells,
                         tag=f"B {B} C {C} ({len(classes)} labels) conn {conn} topk {topk} min_cells {min_cells}")
        assert (ref["class_cells"].sum(axis=1) == ref["foreground"]).all() and (ref["foreground"] > 0).all()
        if len(classes) < 10:
            assert (ref["count"] > 0).all()
    # a single map as [N]: the same without the leading [B]
    from embodied_object_detection_amd import ops
    lab, sc = maps[0]
    one = ops.map_inventory(torch.from_numpy(lab).to(dev), torch.from_numpy(sc).to(dev), cols, 2047, level=LEVEL, topk=8)
    two = ops.map_inventory(torch.from_numpy(lab[None]).to(dev), torch.from_numpy(sc[None]).to(dev), cols, 2047, level=LEVEL, topk=8)
    assert one["object_labels"].shape == (rows * cols,) and one["object"].shape == (8,) and one["class_cells"].shape == (2047,)
    assert one["count"].shape == () and one["status"].shape == (1,)
    for k in IC.KEYS:
        assert torch.equal(one[k], two[k][0]), k


def test_96_by_96_five_classes_drawn_per_cell(dev):
    rows = cols = 96
    for p in (0.6, 0.9):
        lab, sc = _drawn(rows, cols, [0, 1, 2, 3, 4], p, seed=int(p * 100))
        for conn in (4, 8):
            _, ref = run(dev, lab[None], sc[None], cols, 5, conn=conn, topk=64, tag=f"96 x 96 p {p} conn {conn}")
            assert ref["count"][0] > 64 and (ref["class_objects"][0] > 10).all()


def test_200_by_200_lvis_sized(dev):
    """The robot's production grid with B = 2 and the 1203 classes of LVIS: rooms of a few classes, noise of all of them."""
    rows = cols = 200
    r, c = np.mgrid[0:rows, 0:cols]
    rooms = np.asarray([0, 5, 77, 600, 1202], np.int32)
    maps = []
    for b in range(2):
        rng = np.random.default_rng(50 + b)
        lab = rooms[(r // (17 + 6 * b) + c // (29 - 4 * b)) % 5].reshape(-1).copy()
        noise = rng.random(rows * cols) < 0.05
        lab[noise] = rng.integers(-1, 1204, int(noise.sum())).astype(np.int32)              # -1 and 1203 are no class
        maps.append((lab, RC.paint(RC.bernoulli(rows, cols, 0.85 + 0.1 * b, seed=60 + b), LEVEL, seed=b)))
    labels, scores = np.stack([m[0] for m in maps]), np.stack([m[1] for m in maps])
    keep = np.ones(1203, np.uint8)
    keep[77] = 0
    _, ref = run(dev, labels, scores, cols, 1203, conn=8, topk=16, min_cells=2, tag="200 x 200")
    _, cut = run(dev, labels, scores, cols, 1203, conn=4, topk=16, keep=keep, tag="200 x 200, keep")
    assert (ref["area"][:, 0] > 300).all() and (ref["class_objects"] > 0).sum() >= 10 and (cut["class_cells"][:, 77] == 0).all()
    assert (ref["class_cells"][:, 77] > 1000).all()


def test_one_column_one_row_one_cell(dev):
    for rows, cols in ((1, 1), (1, 300), (300, 1), (2, 2)):
        maps = [_drawn(rows, cols, [0, 1, 2], p, seed=70 + i) for i, p in enumerate((0.0, 0.6, 1.0))]
        labels, scores = np.stack([m[0] for m in maps]), np.stack([m[1] for m in maps])
        for conn in (4, 8):
            run(dev, labels, scores, cols, 3, conn=conn, topk=3, tag=f"{rows} x {cols} conn {conn}")


def test_workspace_and_determinism(dev):
    from embodied_object_detection_amd import _lib, ops
    maps = maps_of("33x65")
    plain = [n for n, m in maps.items() if m[2] is None]
    labels, scores = np.stack([maps[n][0] for n in plain]), np.stack([maps[n][1] for n in plain])
    B, N = labels.shape
    cols, C = 65, IC.C5
    dl, ds = torch.from_numpy(labels).to(dev), torch.from_numpy(scores).to(dev)
    need = ops.map_inventory_workspace(B, N, C, 16)
    assert need == ((3 * B * N * 4 + 255) // 256 * 256 + B * 16 * 8 + B * C * 8) // 4
    call = lambda **kw: ops.map_inventory(dl, ds, cols, C, level=LEVEL, **kw)
    fresh = {k: v.clone() for k, v in call().items()}
    check(fresh, labels, scores, cols, C, LEVEL, 8, 1, 16, "fresh", names=plain)
    # 0xFF in every byte of a workspace larger than needed: the kernels initialise what they read and stay inside their part
    ws = torch.full((need + 64,), -1, dtype=torch.int32, device=dev)
    first = {k: v.clone() for k, v in call(workspace=ws).items()}
    assert bool((ws[need:] == -1).all()), "the call wrote behind its workspace"
    again = call(workspace=ws)                                                    # on what the first call left
    for k in fresh:
        for other in (first, again):
            a, b = fresh[k], other[k]
            assert torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a, b.view(torch.int32) if b.dtype == torch.float32 else b), k
    # a zeroed workspace, and the other connectivity after this one on the same workspace
    ws.zero_()
    check(call(connectivity=4, workspace=ws), labels, scores, cols, C, LEVEL, 4, 1, 16, "zeroed workspace", names=plain)
    with pytest.raises(_lib.EodError, match="workspace"):
        call(workspace=ws[:need - 1])
    with pytest.raises(_lib.EodError, match="workspace"):
        call(workspace=ws[1:])                                                    # 4 bytes off an 8-byte boundary
    with pytest.raises(_lib.EodError, match="keep"):
        call(keep=torch.ones(C + 1, dtype=torch.uint8, device=dev))
    with pytest.raises(_lib.EodError, match="keep"):
        call(keep=torch.ones(C, dtype=torch.uint8))                               # on the host
    with pytest.raises(_lib.EodError, match="scores"):
        ops.map_inventory(dl, ds.cpu(), cols, C)


# ---- the models ---------------------------------------------------------------------------------------------------------------
MAP = (24, 24)
KEYS = ("labels", "scores") + IC.KEYS + ("status",)


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


def _level(model, **vocab):
    """The median of the distinct scores of the labelled cells (the cells no frame has written all share one score): cells on either
    side of it, whatever the synthetic weights give."""
    lab, sc = model.semantic_map(thresh=0.0, scores=True, **vocab)
    sc = torch.unique(sc[lab >= 0])
    assert sc.numel() > 2
    return float(sc[sc.numel() // 2])


def _same(a, b):
    assert sorted(a) == sorted(b) == sorted(KEYS), sorted(a)
    for k in a:
        assert a[k].shape == b[k].shape and a[k].dtype == b[k].dtype, k
        assert torch.equal(a[k].contiguous().view(torch.int32) if a[k].dtype == torch.float32 else a[k],
                           b[k].contiguous().view(torch.int32) if b[k].dtype == torch.float32 else b[k]), k


VOCABS = {"own": dict(), "lvis": dict(classifier=LVIS, num_classes=1203)}


@pytest.fixture(scope="module")
def single_runs(dev, synthetic_sd):
    """Per seed: the single-scene model after two frames, its inventory in both vocabularies and the third frame still to run."""
    from embodied_object_detection_amd import build_model
    runs = {}
    for seed in (0, 1):
        model = build_model(_cfg(), synthetic_sd)
        frames = _frames(3, seed)
        model([[frames[0]]])
        inst = model([[frames[1]]])[0]["instances"]
        lvl = runs[0]["lvl"] if runs else {v: _level(model, **kw) for v, kw in VOCABS.items()}        # one level for every run
        out = {v: {k: t.clone() for k, t in model.inventory(thresh=0.0, map_shape=MAP, level=lvl[v], **kw).items()} for v, kw in VOCABS.items()}
        runs[seed] = dict(model=model, frames=frames, inst=inst, lvl=lvl, out=out)
    return runs


def test_model_inventory_equals_the_op_and_the_reference_and_changes_nothing(dev, synthetic_sd, single_runs):
    from embodied_object_detection_amd import _lib, build_model, ops
    run0 = single_runs[0]
    model, frames, inst = run0["model"], run0["frames"], run0["inst"]
    before = dict(semmap=model.semmap, zs=model.zs_weight, mem=model.implicit_memory.clone(), obs=model.observations.clone())
    cut = {}
    for v, kw in VOCABS.items():
        LVL, C = run0["lvl"][v], 20 if v == "own" else 1203
        out = model.inventory(thresh=0.0, map_shape=MAP, level=LVL, **kw)
        _same(out, run0["out"][v])
        lab, sc = model.semantic_map(thresh=0.0, scores=True, **kw)
        assert torch.equal(out["labels"], lab) and torch.equal(out["scores"].view(torch.int32), sc.view(torch.int32))
        op = ops.map_inventory(lab, sc, 24, C, level=LVL)
        for k in op:
            assert torch.equal(out[k], op[k]), (v, k)
        labels, scores = lab.cpu().numpy()[None], sc.cpu().numpy()[None]
        batched = {k: (t if k in ("status",) else t[None]) for k, t in out.items() if k not in ("labels", "scores")}
        ref = check(batched, labels, scores, 24, C, LVL, 8, 1, 16, f"model.inventory, {v}")
        present = np.flatnonzero(ref["class_cells"][0])
        labelled = int((labels[0] >= 0).sum())
        print(f"model.inventory, {v}: level {LVL:.6g}, labelled {labelled}, foreground {ref['foreground'].tolist()}, count "
              f"{ref['count'].tolist()}, classes present {present.tolist()[:12]}, areas {ref['area'][0, :6].tolist()}")
        cut[v] = 0 < ref["foreground"][0] < labelled and len(present) >= 2
        # the other arguments reach the op, `exclude` as its keep table
        drop = [int(ref["cls"][0, 0])] if ref["count"][0] else [0]
        keep = np.ones(C, np.uint8)
        keep[drop] = 0
        o2 = model.inventory(thresh=0.0, map_shape=MAP, level=LVL, connectivity=4, min_cells=2, topk=3, exclude=drop, **kw)
        b2 = {k: (t if k in ("status",) else t[None]) for k, t in o2.items() if k not in ("labels", "scores")}
        r2 = check(b2, labels, scores, 24, C, LVL, 4, 2, 3, f"model.inventory, {v}, excluded {drop}", keep=keep)
        assert o2["object"].shape == (3,) and r2["class_cells"][0, drop[0]] == 0
        o3 = model.inventory(thresh=0.0, map_shape=MAP, level=LVL, exclude=torch.tensor(drop), **kw)
        assert torch.equal(o3["object_labels"], model.inventory(thresh=0.0, map_shape=MAP, level=LVL, exclude=tuple(drop), **kw)["object_labels"])
    # some cells on each side of the level and two classes among the foreground, in one of the vocabularies at least
    assert cut["own"] or cut["lvis"], cut
    # a detection's cell names an object of the map, or none
    out = run0["out"]["own"]
    place = model.place(inst, frames[1]["proj_indices"], attach=True)
    cells = inst.pred_cells.long()
    assert len(cells) == len(inst) > 0 and place["cells"].shape[0] == len(inst)
    lab = torch.where(cells >= 0, out["object_labels"][cells.clamp(min=0)], torch.full_like(cells, -1, dtype=torch.int32))
    valid = (lab == -1) | ((lab >= 0) & (lab < 576) & (out["object_labels"][lab.clamp(min=0).long()] == lab))
    assert bool(valid.all())                                                      # a label is a cell that is its own label
    # host refusals
    for kw in (dict(level=0.0), dict(level=float("nan")), dict(level=1.5), dict(connectivity=6), dict(map_shape=(24, 23)), dict(topk=65),
               dict(map_shape=None), dict(min_cells=0), dict(exclude=[20]), dict(exclude=[-1])):
        with pytest.raises(_lib.EodError):
            model.inventory(**{**dict(thresh=0.0, map_shape=MAP, level=run0["lvl"]["own"]), **kw})
    with pytest.raises(_lib.EodError):
        build_model(_cfg(), synthetic_sd).inventory(map_shape=MAP)                 # no memory yet
    assert model.semmap is before["semmap"] and model.zs_weight is before["zs"]
    assert torch.equal(model.implicit_memory, before["mem"]) and torch.equal(model.observations, before["obs"])
    # frame 3 after the queries against a run that never asked
    other = build_model(_cfg(), synthetic_sd)
    for f in frames[:2]:
        other([[f]])
    for a, b in zip(_out(other, frames[2]), _out(model, frames[2])):
        assert torch.equal(a, b)
    assert torch.equal(other.implicit_memory, model.implicit_memory) and torch.equal(other.observations, model.observations)


def test_class_largest_is_a_region_of_model_regions(dev, synthetic_sd):
    """Where every cell of class c with `prob >= level` has c as its argmax, the objects of class c are the regions of
    `regions([c])`: `class_largest[c]` is one of its `region_labels`, and it is its first region."""
    from embodied_object_detection_amd import build_model
    model = build_model(_cfg(), synthetic_sd)
    for f in _frames(2):
        model([[f]])
    checked = []
    for LVL in (_level(model), 0.5):
        inv = model.inventory(thresh=0.0, map_shape=MAP, level=LVL)
        present = torch.nonzero(inv["class_largest"] >= 0).flatten().tolist()
        for c in present[:6]:
            reg = model.regions([c], thresh=0.0, map_shape=MAP, level=LVL)
            fg = reg["prob"][0] >= LVL
            if not bool((inv["labels"][fg] == c).all()):
                continue                                                          # a cell of the region belongs to another class
            mine = torch.where(inv["labels"] == c, inv["object_labels"], torch.full_like(inv["object_labels"], -1))
            assert torch.equal(mine, reg["region_labels"][0]), (LVL, c)
            assert int(inv["class_largest"][c]) in set(reg["region_labels"][0].tolist()) and inv["class_largest"][c] == reg["region"][0, 0]
            assert inv["class_largest_area"][c] == reg["area"][0, 0] and inv["class_objects"][c] == reg["count"][0]
            checked.append((round(LVL, 4), c))
    print(f"class_largest against regions: checked {checked}")
    assert checked, "no class whose region is wholly its own argmax: the cross-check compared nothing"


def test_lockstep_inventory_equals_the_single_scene_runs(dev, synthetic_sd, single_runs):
    from embodied_object_detection_amd.modeling.lockstep import LockstepScenes
    ls = LockstepScenes(_cfg(), 2, synthetic_sd)
    ls([list(single_runs[0]["frames"][:2]), list(single_runs[1]["frames"][:2])])
    for v, kw in VOCABS.items():
        lvl = single_runs[0]["lvl"][v]
        for b in (0, 1):
            _same(ls.inventory(b, thresh=0.0, map_shape=MAP, level=lvl, **kw), single_runs[b]["out"][v])
        both = ls.inventory(None, thresh=0.0, map_shape=MAP, level=lvl, **kw)
        assert sorted(both) == sorted(KEYS) and both["object_labels"].shape == (2, 576) and both["count"].shape == (2,)
        for k in KEYS:
            want = both[k] if k == "status" else torch.stack([single_runs[b]["out"][v][k] for b in (0, 1)])
            assert both[k].dtype == want.dtype and torch.equal(both[k].contiguous().view(torch.int32) if both[k].dtype == torch.float32 else both[k],
                                                               want.view(torch.int32) if want.dtype == torch.float32 else want), (v, k)
    with pytest.raises(IndexError):
        ls.inventory(2, map_shape=MAP)


def test_predictor_inventory(dev, synthetic_sd):
    from embodied_object_detection_amd.engine.predictor import EmbodiedPredictor
    pred = EmbodiedPredictor(_cfg(), synthetic_sd)
    for f in _frames(2):
        pred.model([[f]])
    LVL = _level(pred.model)
    out = pred.inventory(thresh=0.0, map_shape=MAP, level=LVL, topk=4, exclude=[1])
    _same(out, pred.model.inventory(thresh=0.0, map_shape=MAP, level=LVL, topk=4, exclude=[1]))
    own = pred.inventory(vocabulary="mp3d", thresh=0.0, map_shape=MAP, level=LVL)
    assert own["object_labels"].shape == (576,) and own["object"].shape == (16,) and own["class_cells"].shape == (20,)
    assert own["sum_rc"].dtype == torch.int64
    from embodied_object_detection_amd.engine.predictor import resolve_vocabulary
    _same(own, pred.model.inventory(classifier=resolve_vocabulary("mp3d"), thresh=0.0, map_shape=MAP, level=LVL))
