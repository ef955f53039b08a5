"""`ops.map_sight` on the GPU against the reference of `_sight_cases.py`: exact integer equality of every output, on the smallest
grids at which the kernels can go wrong and on one grid either side of the staging limit, then beyond the reference (dirty buffers,
repeated calls, permuted slots and sources), and the three model surfaces.  No tolerance anywhere."""
import numpy as np
import pytest
import torch

import _inventory_cases as IC
import _sight_cases as SC

pytestmark = pytest.mark.gpu

INT_MAX = SC.INT_MAX


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    from embodied_object_detection_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def grids():
    """1 x 1, one row, one column, a partial bit-plane word and workgroup, N no multiple of 64 under many workgroups, long rows."""
    return {"1x1": (1, 1), "1x70": (1, 70), "70x1": (70, 1), "3x61": (3, 61), "70x67": (70, 67), "19x195": (19, 195)}


def wg():
    from embodied_object_detection_amd import ops
    return ops.SIGHT_WORKGROUP


def run(dev, labels, objects, cols, from_cells, range2=INT_MAX, passable=()):
    from embodied_object_detection_amd import ops
    dl, do = torch.from_numpy(np.ascontiguousarray(labels)).to(dev), torch.from_numpy(np.ascontiguousarray(objects)).to(dev)
    dp = torch.from_numpy(np.ascontiguousarray(passable, dtype=np.int32)).to(dev) if len(passable) else None
    src = np.array(from_cells, np.int32)
    out = ops.map_sight(dl, do, cols, src, range2=None if range2 == INT_MAX else range2, passable=dp)
    N, K, S = labels.size, len(objects), src.size
    assert sorted(out) == sorted(SC.KEYS)
    assert out["seen_mask"].shape == (N,) and out["seen_mask"].dtype == torch.int64 and out["seen_mask"].is_contiguous()
    for k in SC.PAIR_KEYS:
        assert out[k].shape == (S, K) and out[k].dtype == (torch.int64 if k == "near_key" else torch.int32), k
    for k in SC.SLOT_KEYS:
        assert out[k].shape == (K,) and out[k].dtype == (torch.int64 if k == "best_key" else torch.int32), k
    assert out["source_counts"].shape == (S, 2) and out["counts"].shape == (3,) and out["status"].shape == (2,)
    assert torch.equal(dl.cpu(), torch.from_numpy(labels)) and torch.equal(do.cpu(), torch.from_numpy(objects))     # read-only
    assert np.array_equal(src, np.array(from_cells, np.int32))
    if dp is not None:
        assert torch.equal(dp.cpu(), torch.from_numpy(np.ascontiguousarray(passable, dtype=np.int32)))
    return out


def check(dev, tag, m, cols, range2=None, from_cells=None):
    range2 = m["range2"] if range2 is None else range2
    from_cells = m["from_cells"] if from_cells is None else from_cells
    got = SC.host(run(dev, m["labels"], m["objects"], cols, from_cells, range2, m["passable"]))
    ref = SC.reference(m["labels"], m["objects"], cols, from_cells, range2, m["passable"])
    bad = SC.differences(got, ref)
    assert not bad, (tag, range2, bad, {k: (got[k], ref[k]) for k in bad[:2]})
    return ref


@pytest.mark.parametrize("grid", ["1x1", "1x70", "70x1", "3x61", "70x67", "19x195"])
def test_own_maps(dev, grid):
    rows, cols = grids()[grid]
    maps = SC.maps(rows, cols, wg())
    for name, m in maps.items():
        check(dev, f"{grid} {name}", m, cols)
    m = maps["no opaque cell"]
    ref = SC.reference(m["labels"], m["objects"], cols, m["from_cells"])
    used = sum(1 << s for s, f in enumerate(m["from_cells"]) if f >= 0)
    assert (ref["seen_mask"] == np.uint64(used)).all() and ref["counts"].tolist() == [0, rows * cols, rows * cols]
    m = maps["every cell opaque"]
    ref = SC.reference(m["labels"], m["objects"], cols, m["from_cells"])
    assert ref["source_counts"][0, 0] == 0 and 1 <= ref["source_counts"][0, 1] <= 9           # itself and its neighbours
    if grid in ("70x67", "19x195"):
        assert len(maps) == 49
    print(f"{grid}: {len(maps)} maps, all equal")


@pytest.mark.parametrize("grid", ["3x61", "70x67"])
def test_ranges(dev, grid):
    """range2 0, 1, 2, 25, one past the largest d2 of the grid and INT_MAX."""
    rows, cols = grids()[grid]
    maps = SC.maps(rows, cols, wg())
    for name in ("64 objects, 64 sources", "a slot made passable", "no opaque cell", "labels and slots that name nothing"):
        m = maps[name]
        full = SC.reference(m["labels"], m["objects"], cols, m["from_cells"], INT_MAX, m["passable"])
        for range2 in SC.ranges(rows, cols):
            ref = check(dev, f"{grid} {name}", m, cols, range2=range2)
            if range2 == 0:
                used = m["from_cells"][m["from_cells"] >= 0]
                assert ref["counts"][2] == len(set(used.tolist()))                 # every source sees its own cell and no other
            if range2 > (rows - 1) ** 2 + (cols - 1) ** 2:
                assert not SC.differences(ref, full)                               # beyond the grid: unbounded


@pytest.mark.parametrize("grid", ["3x61", "70x67"])
def test_inventory_maps(dev, grid):
    """The object_labels and objects that the inventory's reference gives on its hostile maps."""
    rows, cols = grids()[grid]
    N = rows * cols
    n = 0
    for name, (labels, scores, keep) in IC.hostile_maps(rows, cols, 4, 64).items():
        inv = IC.reference(labels[None], scores[None], cols, IC.C5, IC.LEVEL, topk=64, keep=keep)
        objects, lab = inv["object"][0], inv["object_labels"][0]
        K = (1, 2, 5, 64)[n % 4]
        passable = [int(v) for v in objects[1:3] if v >= 0] if n % 3 == 0 else []
        m = dict(labels=lab, objects=np.ascontiguousarray(objects[:K]), passable=np.asarray(passable, np.int32))
        sources = np.array([(n * 7) % N, N - 1, -1, N // 2, 0][:(1, 5, 3)[n % 3]], np.int32)
        check(dev, f"{grid} {name}", m, cols, range2=(INT_MAX, 1, 25, 400)[n % 4], from_cells=sources)
        n += 1
    print(f"{grid}: {n} maps, all equal")


def test_slot_counts_duplicates_and_unused_slots(dev):
    rows, cols = grids()["70x67"]
    base = SC.maps(rows, cols, wg())["64 objects, 64 sources"]
    for objects in ([4], [4, 9], [9, 4, 9, -1, 4], [-1], [-5, -1], [13, 13], [77, 78], list(range(13, -1, -1)) * 4 + [-1] * 8):
        m = dict(base, objects=np.array(objects, np.int32))
        ref = check(dev, f"slots {objects[:6]}", m, cols, from_cells=base["from_cells"][:9])
    assert len(objects) == 64 and ref["cells"][14:].sum() == 0 and ref["seen_cells"][:, 14:].sum() == 0
    assert (ref["best_source"][14:] == -1).all() and (ref["near_cell"][:, 14:] == -1).all() and (ref["cells"][:14] > 0).all()


@pytest.mark.parametrize("side", ["past the staging limit", "at the staging limit"])
def test_either_side_of_the_staging_limit(dev, side):
    """A square grid one row and column past EOD_SIGHT_LDS_CELLS (the bit plane is read from the workspace) and the one that just
    fits (it is staged), range2 = 400, sources at the centre, in a corner and on the last row, against the windowed reference."""
    from embodied_object_detection_amd import ops
    import math
    n = math.isqrt(ops.SIGHT_LDS_CELLS)
    rows = cols = n + 1 if side.startswith("past") else n
    N = rows * cols
    assert (N > ops.SIGHT_LDS_CELLS) == side.startswith("past") and (n + 1) ** 2 > ops.SIGHT_LDS_CELLS >= n * n
    rng = np.random.default_rng(rows)
    labels = np.where(rng.random(N) < 0.04, rng.integers(0, 6, N), -1).astype(np.int32)
    sources = [(rows // 2) * cols + cols // 2, 0, -1, (rows - 1) * cols + cols // 3, N - 1]
    m = dict(labels=labels, objects=np.array([3, 0, 5, 9], np.int32), passable=np.array([2], np.int32))
    ref = check(dev, side, m, cols, range2=400, from_cells=sources)
    assert ref["counts"][2] > 300 and ref["seen_cells"].sum() > 0 and (ref["seen_mask"][:cols * 20 + 21] & np.uint64(2)).any()
    empty = dict(m, labels=np.full(N, -1, np.int32))
    ref = check(dev, side, empty, cols, range2=400, from_cells=sources)
    assert ref["source_counts"][0].tolist() == [1257, 0]                           # the lattice points of a disc of radius 20
    # 17 and 64 sources: more than one source group, so the groups OR their bits into seen_mask and the finish launch counts the
    # seen cells, staged and not; an unused and a duplicate source among them, and sources in both groups that see the same cells
    for S in (ops.SIGHT_SOURCE_GROUP + 1, 64):
        many = [int(v) for v in rng.integers(0, N, S)]
        many[0], many[1], many[-1] = sources[0], -1, sources[0] + 3
        many[ops.SIGHT_SOURCE_GROUP - 1], many[ops.SIGHT_SOURCE_GROUP] = N - 1, N - 1
        ref = check(dev, f"{side}, S = {S}", m, cols, range2=400, from_cells=many)
        assert ref["counts"][2] > 1257 and (ref["seen_mask"] >> np.uint64(ops.SIGHT_SOURCE_GROUP)).any()


def raw(dev, m, cols, fill):
    """The entry point on buffers of this test's own, outputs and workspace filled with `fill` bytes before the call."""
    from embodied_object_detection_amd import _lib, ops
    from embodied_object_detection_amd.ops import _stream
    labels, objects, passable = m["labels"], m["objects"], m["passable"]
    src = np.ascontiguousarray(m["from_cells"], dtype=np.int32)
    N, K, P, S = labels.size, len(objects), len(passable), src.size
    dl, do = torch.from_numpy(labels).to(dev), torch.from_numpy(objects).to(dev)
    dp = torch.from_numpy(passable).to(dev) if P else None
    shapes = dict(seen_mask=(N,), cells=(K,), seen_cells=(S, K), near_key=(S, K), near_d2=(S, K), near_cell=(S, K), best_key=(K,),
                  best_seen=(K,), best_source=(K,), source_counts=(S, 2), counts=(3,), status=(2,))
    out = {}
    for k, shape in shapes.items():
        wide = k in SC.WIDE
        t = torch.full((int(np.prod(shape)) * (8 if wide else 4),), fill, dtype=torch.uint8, device=dev)
        out[k] = t.view(torch.int64 if wide else torch.int32).view(shape)
    words = ops.map_sight_workspace(N, cols)
    ws = torch.full((words * 4,), fill, dtype=torch.uint8, device=dev).view(torch.int32)
    _lib.check(_lib.load().eod_map_sight(dl.data_ptr(), do.data_ptr(), dp.data_ptr() if P else None, src.ctypes.data, N, K, P, S, cols,
                                         m["range2"], *[out[k].data_ptr() for k in shapes], ws.data_ptr(), words * 4, _stream()),
               "eod_map_sight")
    return out


def test_dirty_buffers_and_repeated_calls(dev):
    rows, cols = grids()["70x67"]
    maps = SC.maps(rows, cols, wg())
    for name in ("64 objects, 64 sources", "labels and slots that name nothing", "no opaque cell", "every cell opaque",
                 "a slot made passable"):
        m = maps[name]
        ref = SC.reference(m["labels"], m["objects"], cols, m["from_cells"], m["range2"], m["passable"])
        for fill in (0xFF, 0x00, 0x5A):
            assert not SC.differences(SC.host(raw(dev, m, cols, fill)), ref), (name, fill)
        a, b = (SC.host(run(dev, m["labels"], m["objects"], cols, m["from_cells"], m["range2"], m["passable"])) for _ in range(2))
        assert not SC.differences(a, b) and not SC.differences(a, ref), name


def test_permuted_slots_and_sources_permute_results(dev):
    rows, cols = grids()["70x67"]
    rng = np.random.default_rng(5)
    m = SC.maps(rows, cols, wg())["64 objects, 64 sources"]
    objects, sources = m["objects"], m["from_cells"]
    assert len(set(objects.tolist())) == objects.size                 # distinct slots
    base = SC.host(run(dev, m["labels"], objects, cols, sources, 900))
    p = rng.permutation(objects.size)
    got = SC.host(run(dev, m["labels"], np.ascontiguousarray(objects[p]), cols, sources, 900))
    for k in SC.SLOT_KEYS:
        assert np.array_equal(got[k], base[k][p]), k                  # slot k of `got` is slot p[k] of `base`
    for k in SC.PAIR_KEYS:
        assert np.array_equal(got[k], base[k][:, p]), k
    for k in ("seen_mask", "source_counts", "counts", "status"):
        assert np.array_equal(got[k], base[k]), k
    q = rng.permutation(sources.size)
    got = SC.host(run(dev, m["labels"], objects, cols, np.ascontiguousarray(sources[q]), 900))
    for k in SC.PAIR_KEYS + ("source_counts",):
        assert np.array_equal(got[k], base[k][q]), k                  # source s of `got` is source q[s] of `base`
    bits = (base["seen_mask"][:, None] >> q.astype(np.uint64)[None, :]) & np.uint64(1)
    assert np.array_equal(got["seen_mask"], (bits << np.arange(64, dtype=np.uint64)[None, :]).sum(axis=1, dtype=np.uint64))   # the bits move with them
    assert np.array_equal(got["cells"], base["cells"]) and np.array_equal(got["counts"], base["counts"])
    assert np.array_equal(got["best_seen"], base["best_seen"])        # the most any source sees of a slot; which source: by the new order
    seen = np.where((sources[q] >= 0)[:, None], got["seen_cells"], 0)
    assert np.array_equal(got["best_source"], np.where(seen.max(axis=0) > 0, seen.argmax(axis=0), -1))       # argmax: the lowest s on a tie


# ---- the models ------------------------------------------------------------------------------------------------------------------
MAP = (24, 24)
LEVEL = 2.0 ** -11                                                   # below any argmax probability: every labelled cell is in an object


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


def _against_reference(res, inv, from_cells, range2=INT_MAX, passable=()):
    ref = SC.reference(inv["object_labels"].cpu().numpy(), inv["object"].cpu().numpy(), MAP[1], from_cells, range2, passable)
    bad = SC.differences(SC.host(res), ref)
    assert not bad, bad
    return ref


def test_model_sight_changes_nothing(dev, synthetic_sd):
    from embodied_object_detection_amd import _lib, build_model
    model = build_model(_cfg(), synthetic_sd)
    frames = _frames(4)
    for f in frames[:3]:
        model([[f]])
    inv = model.inventory(thresh=0.0, map_shape=MAP, level=LEVEL)
    assert int(inv["count"]) >= 2, "the synthetic map holds too few objects for this test"
    before = dict(mem=model.implicit_memory.clone(), obs=model.observations.clone(), lab=inv["object_labels"].clone())
    first = int(inv["object"][0])
    here = 24 * 11 + 7
    ref = _against_reference(model.sight(inv["object"], inv["object_labels"], map_shape=MAP, from_cells=here), inv, [here])
    _against_reference(model.sight(inv["object"].tolist(), inv["object_labels"], map_shape=MAP, from_cells=[here, 0, -1, 575], range2=64,
                                   passable=[first]), inv, [here, 0, -1, 575], 64, [first])
    # the intended use: the robot's cell, the most open cell of every territory and the goal cell beside every object as candidates
    clr = model.clearance(inv["object"], inv["object_labels"], map_shape=MAP)
    rt = model.route(inv["object"], inv["object_labels"], map_shape=MAP, from_cell=here, path_max=64)
    cand = torch.cat([torch.tensor([here], dtype=torch.int32, device=dev), clr["widest_cell"], rt["goal_cell"]])
    assert cand.is_cuda and cand.numel() == 1 + 2 * inv["object"].numel() <= 64
    s = model.sight(inv["object"], inv["object_labels"], map_shape=MAP, from_cells=cand, range2=64)
    ref = _against_reference(s, inv, cand.cpu().numpy(), 64)
    assert np.array_equal(ref["cells"], inv["area"].cpu().numpy())                # an object's cells are its area
    print(f"model.sight: {int(inv['count'])} objects of {ref['cells'][ref['cells'] > 0].tolist()} cells, best_source "
          f"{ref['best_source'].tolist()}, best_seen {ref['best_seen'].tolist()}, counts {ref['counts'].tolist()}")
    with pytest.raises(_lib.EodError, match="map_shape"):
        model.sight(inv["object"], inv["object_labels"], from_cells=here)
    with pytest.raises(_lib.EodError, match="from_cells is required"):
        model.sight(inv["object"], inv["object_labels"], map_shape=MAP)
    with pytest.raises(_lib.EodError, match="from_cells"):
        model.sight(inv["object"], inv["object_labels"], map_shape=MAP, from_cells=torch.tensor([576], device=dev))
    with pytest.raises(_lib.EodError, match="range2"):
        model.sight(inv["object"], inv["object_labels"], map_shape=MAP, from_cells=here, range2=-1)
    assert torch.equal(model.implicit_memory, before["mem"]) and torch.equal(model.observations, before["obs"])
    assert torch.equal(inv["object_labels"], before["lab"])
    # the next frame after the queries against a run that never asked
    other = build_model(_cfg(), synthetic_sd)
    for f in frames[:3]:
        other([[f]])
    for a, b in zip(_out(other, frames[3]), _out(model, frames[3])):
        assert torch.equal(a, b)
    assert torch.equal(other.implicit_memory, model.implicit_memory) and torch.equal(other.observations, model.observations)


def test_predictor_sight(dev, synthetic_sd):
    from embodied_object_detection_amd.engine.predictor import EmbodiedPredictor
    pred = EmbodiedPredictor(_cfg(), synthetic_sd)
    frames = _frames(4)
    for f in frames[:3]:
        pred.model([[f]])
    inv = pred.inventory(thresh=0.0, map_shape=MAP, level=LEVEL)
    s = pred.sight(inv["object"], inv["object_labels"], map_shape=MAP, from_cells=[30, 500, 30], range2=100)
    _against_reference(s, inv, [30, 500, 30], 100)
    other = EmbodiedPredictor(_cfg(), synthetic_sd)
    for f in frames[:3]:
        other.model([[f]])
    for a, b in zip(_out(other.model, frames[3]), _out(pred.model, frames[3])):
        assert torch.equal(a, b)


def test_lockstep_sight(dev, synthetic_sd):
    from embodied_object_detection_amd import _lib
    from embodied_object_detection_amd.modeling.lockstep import LockstepScenes
    seqs = [_frames(4, 0), _frames(4, 1)]
    ls = LockstepScenes(_cfg(), 2, synthetic_sd)
    ls([s[:3] for s in seqs])
    inv = ls.inventory(None, thresh=0.0, map_shape=MAP, level=LEVEL)
    assert inv["object"].shape == (2, 16) and inv["object_labels"].shape == (2, 24 * 24)
    sources = [[30, -1, 24 * 20 + 3], [575, 0, 300]]
    s = ls.sight(inv["object"], inv["object_labels"], map_shape=MAP, from_cells=sources, range2=144)
    t = ls.sight(inv["object"], inv["object_labels"], map_shape=MAP, from_cells=torch.tensor(sources, device=dev), range2=144)
    assert s["seen_mask"].shape == (2, 24 * 24) and s["seen_cells"].shape == (2, 3, 16) and s["best_key"].shape == (2, 16)
    for b in (0, 1):
        one = {k: v[b] for k, v in inv.items() if k in ("object", "object_labels")}
        _against_reference({k: v[b] for k, v in s.items()}, one, sources[b], 144)
        _against_reference({k: v[b] for k, v in t.items()}, one, sources[b], 144)
        single = ls.sight(inv["object"][b], inv["object_labels"][b], map_shape=MAP, from_cells=sources[b], range2=144)
        assert not SC.differences(SC.host(single), SC.host({k: v[b] for k, v in s.items()}))
    with pytest.raises(_lib.EodError, match="from_cells"):
        ls.sight(inv["object"], inv["object_labels"], map_shape=MAP, from_cells=[1, 2, 3])
    with pytest.raises(_lib.EodError, match="from_cells"):
        ls.sight(inv["object"], inv["object_labels"], map_shape=MAP, from_cells=[[1, 2], [3]])
    other = LockstepScenes(_cfg(), 2, synthetic_sd)
    other([s_[:3] for s_ in seqs])
    got, want = ls([s_[3:] for s_ in seqs]), other([s_[3:] for s_ in seqs])
    for g, w in zip(got, want):
        for a, b in zip(g, w):
            ia, ib = a["instances"], b["instances"]
            assert torch.equal(ia.pred_boxes.tensor, ib.pred_boxes.tensor) and torch.equal(ia.scores, ib.scores)
            assert torch.equal(ia.pred_classes, ib.pred_classes) and torch.equal(ia.pred_masks, ib.pred_masks)
