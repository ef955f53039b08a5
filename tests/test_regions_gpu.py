"""The connected regions of a map (`eod_map_regions`, `ops.map_regions`, `regions` on the models) against the exact reference of
`_regions_cases.py`: every output, every cell, every slot, for equality.  There is no tolerance anywhere: the op is integers and
comparisons, and `peak_prob` is compared by its bits.

The hostile maps of one grid are the classes of one call (a different map per class, so a wrong class stride shows), under both
connectivities.  Grids: 19 x 23 (less than a tile), 131 x 197, (2 T_r + 3) x (3 T_c + 1) from the tile the library was built with
(three tiles each way with ragged edges, whatever the tile), and one 512 x 512 call."""
import numpy as np
import pytest
import torch

import _regions_cases as RC

pytestmark = pytest.mark.gpu

LEVEL = RC.LEVEL


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    from embodied_object_detection_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def tile():
    from embodied_object_detection_amd import ops
    return ops.REGIONS_TILE_ROWS, ops.REGIONS_TILE_COLS


def grids():
    tr, tc = tile()
    return {"19x23": (19, 23), "131x197": (131, 197), "tiles": (2 * tr + 3, 3 * tc + 1)}


_MAPS = {}


def maps_of(name):
    """The hostile maps of a grid, made once and left unchanged: (names, float32 [Q, N], rows, cols)."""
    if name not in _MAPS:
        rows, cols = grids()[name]
        m = RC.hostile_maps(rows, cols, *tile(), level=LEVEL)
        _MAPS[name] = (list(m), np.stack(list(m.values())), rows, cols)
    return _MAPS[name]


def bits(a):
    return a.view(np.int32) if a.dtype == np.float32 else a


def check(out, prob, cols, level, conn, min_cells, topk, tag, names=None):
    """Every output of the op against the reference, for equality; status 0; the types and shapes of the interface."""
    Q, N = prob.shape
    ref = RC.reference(prob, cols, level, conn, min_cells, topk)
    got = {k: v.cpu().numpy() for k, v in out.items()}
    assert sorted(got) == sorted(RC.KEYS + ("status",)), sorted(got)
    assert got["status"].dtype == np.int32 and got["status"].tolist() == [0], (tag, got["status"])
    for k in RC.KEYS:
        assert got[k].dtype == ref[k].dtype and got[k].shape == ref[k].shape, (tag, k, got[k].dtype, got[k].shape)
        same = bits(got[k]) == bits(ref[k])
        if not same.all():
            q = int(np.argwhere(~same)[0][0]) if same.ndim else 0
            raise AssertionError(f"{tag}: {k} differs in {int((~same).sum())} places, first in class {q}"
                                 f"{' (' + names[q] + ')' if names else ''}: got {got[k][q].reshape(-1)[:16].tolist()}, "
                                 f"want {ref[k][q].reshape(-1)[:16].tolist()}")
    return ref


@pytest.mark.parametrize("conn", [4, 8])
@pytest.mark.parametrize("grid", ["19x23", "131x197", "tiles"])
def test_hostile_maps_equal_the_reference(dev, grid, conn):
    from embodied_object_detection_amd import ops
    names, prob, rows, cols = maps_of(grid)
    assert 5 < len(names) <= 32 and ("corner diagonal" in names) == (grid != "19x23")
    d = torch.from_numpy(prob).to(dev)
    before = d.clone()
    out = ops.map_regions(d, cols, LEVEL, connectivity=conn)
    ref = check(out, prob, cols, LEVEL, conn, 1, 16, f"{grid} conn {conn}", names)
    assert torch.equal(d.view(torch.int32), before.view(torch.int32)), "prob was written"
    cnt = dict(zip(names, ref["count"].tolist()))
    print(f"[{grid}, {conn}] components: {cnt}")
    assert cnt["serpentine"] == 1 and ref["region"][names.index("serpentine"), 0] == 0
    assert cnt["spirals"] == 2 and cnt["row-end pair"] == 2 and cnt["row ends"] == 2
    assert cnt["checkerboard"] == (1 if conn == 8 else (rows * cols + 1) // 2)
    assert cnt["all foreground"] == 1 and cnt["all background"] == 0 and cnt["below the level"] == 0 and cnt["at the level"] > 0
    if grid != "19x23":
        assert cnt["corner diagonal"] == cnt["corner anti-diagonal"] == (1 if conn == 8 else 2)
    q = names.index("all background")
    for k in RC.KEYS:
        assert (out[k][q].cpu().numpy() == (-1 if k in ("region", "region_labels") else 0)).all(), k


@pytest.mark.parametrize("Q", [1, 5, 32])
def test_call_shapes(dev, Q):
    """Q = 1, 5, 32 with a map of its own per class; topk 1, 16, 64; min_cells 1 and 5; both connectivities."""
    from embodied_object_detection_amd import ops
    rows, cols = 131, 197
    p = (0.3, 0.45, 0.5, 0.55, 0.593, 0.62, 0.66, 0.7)
    prob = np.stack([RC.paint(RC.bernoulli(rows, cols, p[q % 8], seed=1000 + q), LEVEL, seed=q) for q in range(Q)])
    d = torch.from_numpy(prob).to(dev)
    for conn in (4, 8):
        for topk in (1, 16, 64):
            for min_cells in (1, 5):
                out = ops.map_regions(d, cols, LEVEL, connectivity=conn, min_cells=min_cells, topk=topk)
                ref = check(out, prob, cols, LEVEL, conn, min_cells, topk, f"Q {Q} conn {conn} topk {topk} min_cells {min_cells}")
                assert (ref["count"] > 0).all()
    assert (ref["count"] > 64).any() or Q == 1                      # topk is a cut, not the count
    # another level on the same maps
    out = ops.map_regions(d, cols, 0.75, connectivity=8, topk=16)
    check(out, prob, cols, 0.75, 8, 1, 16, f"Q {Q} level 0.75")


def test_512_by_512(dev):
    """262 144 cells, Q = 2: site percolation at its threshold under 4-connectivity (the most tortuous clusters) and the serpentine."""
    from embodied_object_detection_amd import ops
    rows = cols = 512
    prob = np.stack([RC.paint(RC.bernoulli(rows, cols, 0.593, seed=7), LEVEL, seed=7), RC.paint(RC.serpentine(rows, cols), LEVEL, seed=8)])
    out = ops.map_regions(torch.from_numpy(prob).to(dev), cols, LEVEL, connectivity=4, topk=16)
    ref = check(out, prob, cols, LEVEL, 4, 1, 16, "512 x 512")
    assert ref["count"][1] == 1 and ref["area"][1, 0] == 256 * 512 + 255 and ref["area"][0, 0] > 10000


def test_workspace_and_determinism(dev):
    from embodied_object_detection_amd import _lib, ops
    names, prob, rows, cols = maps_of("tiles")
    Q, N = prob.shape
    d = torch.from_numpy(prob).to(dev)
    need = ops.map_regions_workspace(Q, N, 16)
    assert need == ((3 * Q * N * 4 + 255) // 256 * 256 + Q * 16 * 8) // 4
    fresh = {k: v.clone() for k, v in ops.map_regions(d, cols, LEVEL, connectivity=8).items()}
    ref = check(fresh, prob, cols, LEVEL, 8, 1, 16, "fresh")
    # 0xFF in every byte of a workspace larger than needed: the kernels initialise what they read and stay inside their part
    ws = torch.full((need + 64,), -1, dtype=torch.int32, device=dev)
    first = {k: v.clone() for k, v in ops.map_regions(d, cols, LEVEL, connectivity=8, workspace=ws).items()}
    assert bool((ws[need:] == -1).all()), "the call wrote behind its workspace"
    again = ops.map_regions(d, cols, LEVEL, connectivity=8, workspace=ws)                    # on what the first call left
    for k in fresh:
        for other in (first, again):
            a, b = fresh[k], other[k]
            assert torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a, b.view(torch.int32) if b.dtype == torch.float32 else b), k
    # a zeroed workspace, and the other connectivity after this one on the same workspace
    ws.zero_()
    check(ops.map_regions(d, cols, LEVEL, connectivity=4, workspace=ws), prob, cols, LEVEL, 4, 1, 16, "zeroed workspace")
    with pytest.raises(_lib.EodError, match="workspace"):
        ops.map_regions(d, cols, LEVEL, workspace=ws[:need - 1])
    with pytest.raises(_lib.EodError, match="workspace"):
        ops.map_regions(d, cols, LEVEL, workspace=ws[1:])                                    # 4 bytes off an 8-byte boundary
    assert ref["count"].sum() > 0


def test_one_column_one_row_one_cell(dev):
    from embodied_object_detection_amd import ops
    rng = np.random.default_rng(5)
    for rows, cols in ((1, 1), (1, 300), (300, 1), (2, 2)):
        prob = np.stack([RC.paint(rng.random(rows * cols) < p, LEVEL, seed=3) for p in (0.0, 0.6, 1.0)])
        for conn in (4, 8):
            out = ops.map_regions(torch.from_numpy(prob).to(dev), cols, LEVEL, connectivity=conn, topk=3)
            check(out, prob, cols, LEVEL, conn, 1, 3, f"{rows} x {cols} conn {conn}")


# ---- the models ---------------------------------------------------------------------------------------------------------------
MAP = (24, 24)
QUERY = [3, 0, 19, 7]


def _level(model):
    """Halfway between the smallest and the largest probability of the queried maps: some cells on either side, whatever the
    synthetic weights give."""
    prob = model.locate(QUERY, thresh=0.0, map_shape=MAP)["prob"]
    lo, hi = float(prob.min()), float(prob.max())
    assert 0.0 < lo < hi <= 1.0, (lo, hi)
    return (lo + hi) / 2


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


LOCATE_KEYS = ["labels", "peak_scores", "peaks", "prob", "scores"]


def _same(a, b):
    assert sorted(a) == sorted(b) == sorted(LOCATE_KEYS + list(RC.KEYS) + ["status"]), sorted(a)
    for k in a:
        assert a[k].shape == b[k].shape and a[k].dtype == b[k].dtype, k
        assert torch.equal(a[k].contiguous().view(torch.int32) if a[k].dtype == torch.float32 else a[k],
                           b[k].contiguous().view(torch.int32) if b[k].dtype == torch.float32 else b[k]), k


@pytest.fixture(scope="module")
def single_runs(dev, synthetic_sd):
    """Per seed: the single-scene model after two frames, its regions query and the third frame still to run."""
    from embodied_object_detection_amd import build_model
    runs = {}
    for seed in (0, 1):
        model = build_model(_cfg(), synthetic_sd)
        frames = _frames(3, seed)
        model([[frames[0]]])
        inst = model([[frames[1]]])[0]["instances"]
        lvl = runs[0]["lvl"] if runs else _level(model)                 # one level for every run
        out = model.regions(QUERY, thresh=0.0, map_shape=MAP, level=lvl)
        runs[seed] = dict(model=model, frames=frames, inst=inst, lvl=lvl, out={k: v.clone() for k, v in out.items()})
    return runs


def test_model_regions_equals_the_op_and_the_reference_and_changes_nothing(dev, synthetic_sd, single_runs):
    from embodied_object_detection_amd import _lib, build_model, ops
    run = single_runs[0]
    model, frames, inst, LVL = run["model"], run["frames"], run["inst"], run["lvl"]
    before = dict(semmap=model.semmap, zs=model.zs_weight, mem=model.implicit_memory.clone(), obs=model.observations.clone())
    out = model.regions(QUERY, thresh=0.0, map_shape=MAP, level=LVL)
    _same(out, run["out"])
    loc = model.locate(QUERY, thresh=0.0, map_shape=MAP)
    for k in LOCATE_KEYS:
        assert torch.equal(out[k], loc[k]), k
    op = ops.map_regions(loc["prob"], 24, LVL)
    for k in op:
        assert torch.equal(out[k], op[k]), k
    prob = loc["prob"].cpu().numpy()
    ref = check({k: out[k] for k in RC.KEYS + ("status",)}, prob, 24, LVL, 8, 1, 16, "model.regions")
    print(f"model.regions: foreground {ref['foreground'].tolist()}, count {ref['count'].tolist()}, areas {ref['area'][:, :4].tolist()}")
    assert (ref["foreground"] > 0).any() and (ref["foreground"] < 576).any(), "the level does not cut the synthetic maps"
    # the other arguments reach the op
    o2 = model.regions(QUERY, thresh=0.0, map_shape=MAP, level=LVL, connectivity=4, min_cells=2, topk=3, radius=0, peaks=4)
    check({k: o2[k] for k in RC.KEYS + ("status",)}, prob, 24, LVL, 4, 2, 3, "model.regions, 4-connectivity")
    assert o2["peaks"].shape == (len(QUERY), 4) and o2["region"].shape == (len(QUERY), 3)
    # a detection's cells name a region of the map, or none
    place = model.place(inst, frames[1]["proj_indices"], attach=True)
    cells = inst.pred_cells.long()
    assert len(cells) == len(inst) > 0
    lab = out["region_labels"][:, cells.clamp(min=0)]                # [Q, K]
    lab = torch.where(cells[None, :] >= 0, lab, torch.full_like(lab, -1))
    valid = (lab == -1) | ((lab >= 0) & (lab < 576) & (out["region_labels"].gather(1, lab.clamp(min=0).long()) == lab))
    assert bool(valid.all()) and place["cells"].shape[0] == len(inst)      # a label is a cell that is its own label
    # host refusals
    for kw in (dict(level=0.0), dict(level=float("nan")), dict(level=1.5), dict(connectivity=6), dict(map_shape=(24, 23)), dict(topk=65),
               dict(map_shape=None), dict(min_cells=0)):
        with pytest.raises(_lib.EodError):
            model.regions(QUERY, **{**dict(thresh=0.0, map_shape=MAP, level=LVL), **kw})
    with pytest.raises(_lib.EodError):
        build_model(_cfg(), synthetic_sd).regions(QUERY, map_shape=MAP)             # no memory yet
    assert model.semmap is before["semmap"] and model.zs_weight is before["zs"]
    assert torch.equal(model.implicit_memory, before["mem"]) and torch.equal(model.observations, before["obs"])
    # frame 3 after the queries against a run that never asked
    other = build_model(_cfg(), synthetic_sd)
    for f in frames[:2]:
        other([[f]])
    for a, b in zip(_out(other, frames[2]), _out(model, frames[2])):
        assert torch.equal(a, b)
    assert torch.equal(other.implicit_memory, model.implicit_memory) and torch.equal(other.observations, model.observations)


def test_lockstep_regions_equals_the_single_scene_runs(dev, synthetic_sd, single_runs):
    from embodied_object_detection_amd.modeling.lockstep import LockstepScenes
    ls = LockstepScenes(_cfg(), 2, synthetic_sd)
    ls([list(single_runs[0]["frames"][:2]), list(single_runs[1]["frames"][:2])])
    for b in (0, 1):
        _same(ls.regions(b, QUERY, thresh=0.0, map_shape=MAP, level=single_runs[0]["lvl"]), single_runs[b]["out"])
    with pytest.raises(IndexError):
        ls.regions(2, QUERY, map_shape=MAP)


def test_predictor_regions(dev, synthetic_sd):
    from embodied_object_detection_amd.engine.predictor import EmbodiedPredictor
    pred = EmbodiedPredictor(_cfg(), synthetic_sd)
    for f in _frames(2):
        pred.model([[f]])
    LVL = _level(pred.model)
    out = pred.regions(QUERY, thresh=0.0, map_shape=MAP, level=LVL, topk=4)
    _same(out, pred.model.regions(QUERY, thresh=0.0, map_shape=MAP, level=LVL, topk=4))
    own = pred.regions([0, 19], vocabulary="mp3d", thresh=0.0, map_shape=MAP, level=LVL)
    assert own["region_labels"].shape == (2, 576) and own["region"].shape == (2, 16) and own["sum_rc"].dtype == torch.int64
