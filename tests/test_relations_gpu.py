"""`ops.map_relations` on the GPU against the brute-force reference of `_relations_cases.py`: exact integer equality of every
output, on the smallest grids at which the kernel can go wrong, then beyond the reference (dirty buffers, repeated calls, permuted
slots) and through the three model surfaces.  No tolerance anywhere."""
import numpy as np
import pytest
import torch

import _inventory_cases as IC
import _relations_cases as LC

pytestmark = pytest.mark.gpu

INT_MAX = LC.INT_MAX


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    from embodied_object_detection_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def tiles():
    from embodied_object_detection_amd import ops
    return ops.RELATIONS_TILE_ROWS, ops.RELATIONS_TILE_COLS


def grids():
    tr, tc = tiles()
    return {"37x29": (37, 29), "1x1": (1, 1), "1x70": (1, 70), "70x1": (70, 1), "tiles": (tr + 6, 2 * tc + 3)}


def run(dev, labels, objects, cols, radius, from_cell=-1, topn=4):
    from embodied_object_detection_amd import ops
    dl, do = torch.from_numpy(np.ascontiguousarray(labels)).to(dev), torch.from_numpy(np.ascontiguousarray(objects)).to(dev)
    out = ops.map_relations(dl, do, cols, radius=radius, from_cell=from_cell, topn=topn)
    K = len(objects)
    assert sorted(out) == sorted(LC.KEYS)
    for k in LC.MATRIX_KEYS:
        assert out[k].shape == (K, K) and out[k].dtype == (torch.int64 if k == "pair_key" else torch.int32), k
    for k in ("cells", "from_key", "from_d2", "from_closest"):
        assert out[k].shape == (K,) and out[k].dtype == (torch.int64 if k == "from_key" else torch.int32), k
    assert out["nearest"].shape == (K, topn) and out["nearest_d2"].shape == (K, topn)
    assert torch.equal(dl.cpu(), torch.from_numpy(labels)) and torch.equal(do.cpu(), torch.from_numpy(objects))     # read-only
    return LC.host(out)


def check(dev, tag, labels, objects, cols, radius, from_cell=-1, topn=4):
    got = run(dev, labels, objects, cols, radius, from_cell, topn)
    ref = LC.reference(labels, objects, cols, radius, from_cell, topn)
    bad = LC.differences(got, ref)
    assert not bad, (tag, radius, from_cell, topn, bad, {k: (got[k], ref[k]) for k in bad[:2]})
    return ref


def from_cells(labels, objects, N):
    """A corner, the last cell, a cell inside an object (d2 = 0), a cell of no object, and none."""
    s = LC.slots(labels, objects)
    out = [0, N - 1, -1]
    if (s >= 0).any():
        out.append(int(np.flatnonzero(s >= 0)[len(np.flatnonzero(s >= 0)) // 2]))
    if (s < 0).any():
        out.append(int(np.flatnonzero(s < 0)[-1]))
    return out


@pytest.mark.parametrize("grid", ["37x29", "1x1", "1x70", "70x1", "tiles"])
def test_own_maps(dev, grid):
    rows, cols = grids()[grid]
    tr, tc = tiles()
    n = 0
    for R in (1, 3, 5, 16):
        maps = LC.own_maps(rows, cols, tr, tc, R)
        dense = ("64 alternating", "one everywhere", "labels and slots that name nothing")
        for name, (labels, objects) in maps.items():
            if R == 16 and name in dense and not (grid == "tiles" and name == "64 alternating") and rows * cols > 100:
                continue                                             # R = 16 on sparse maps, and on one dense one (the reference's time)
            fcs = from_cells(labels, objects, rows * cols)
            for m, topn in enumerate((1, 8, 4)):
                ref = check(dev, f"{grid} {name}", labels, objects, cols, R, fcs[(n + m) % len(fcs)], topn)
            n += 1
            if name == "four corners" and R == 16 and grid == "37x29":
                assert (ref["min_d2"] == INT_MAX).all()              # 28 columns apart
            if name == "four corners" and R == 16 and grid == "1x70":
                assert (ref["min_d2"] == INT_MAX).all() and ref["cells"].tolist() == [1, 1, 0, 0]
    print(f"{grid}: {n} maps x 3 calls, all equal")


def test_four_corners_with_a_radius_larger_than_the_grid(dev):
    for rows, cols in ((9, 12), (1, 5), (10, 11), (3, 2)):
        labels, objects = LC.own_maps(rows, cols, *tiles(), 16)["four corners"]
        for fc in (0, rows * cols - 1, -1):
            ref = check(dev, f"corners {rows}x{cols}", labels, objects, cols, 16, fc, 8)
        assert (ref["min_d2"][0, 1] == (cols - 1) ** 2) and (ref["nearest"][0] >= 0).sum() == (3 if rows > 1 else 1)


def test_at_and_beyond_the_radius(dev):
    """A pair at exactly d2 = R^2 is within reach, the first d2 beyond it is not: for every radius."""
    for R in range(1, 17):
        bdr, bdc = LC.first_beyond(R)
        g = np.full((40, 120), -1, np.int32)
        objs, lab, c0 = [], 0, 0
        for dr, dc in LC.exactly_at(R) + [(bdr, bdc)]:
            g[20, c0], g[20 + dr, c0 + dc] = lab, lab + 1
            objs += [lab, lab + 1]
            lab += 2
            c0 += dc + R + 2
        ref = check(dev, f"radius {R}", g.reshape(-1), np.array(objs, np.int32), 120, R, 20 * 120, 2)
        n = len(objs) // 2
        assert [int(ref["min_d2"][2 * k, 2 * k + 1]) for k in range(n)] == [R * R] * (n - 1) + [INT_MAX]


@pytest.mark.parametrize("grid", ["37x29", "tiles"])
def test_inventory_maps(dev, grid):
    """The object_labels and objects that the inventory's reference gives on its hostile maps."""
    rows, cols = grids()[grid]
    tr, tc = tiles()
    n = 0
    for name, (labels, scores, keep) in IC.hostile_maps(rows, cols, tr, tc).items():
        inv = IC.reference(labels[None], scores[None], cols, IC.C5, IC.LEVEL, topk=64, keep=keep)
        objects, lab = inv["object"][0], inv["object_labels"][0]
        K = (1, 2, 5, 64)[n % 4]
        R = (2, 1, 3, 5)[n % 4]
        fcs = from_cells(lab, objects[:K], rows * cols)
        check(dev, f"{grid} {name}", lab, np.ascontiguousarray(objects[:K]), cols, R, fcs[n % len(fcs)], (4, 1, 8)[n % 3])
        n += 1
    # one dense map at the largest radius
    labels, scores, keep = IC.hostile_maps(rows, cols, tr, tc)["bernoulli 0.593"]
    inv = IC.reference(labels[None], scores[None], cols, IC.C5, IC.LEVEL, topk=64, keep=keep)
    check(dev, f"{grid} bernoulli, R 16", inv["object_labels"][0], inv["object"][0], cols, 16, rows * cols // 2, 8)
    print(f"{grid}: {n + 1} maps, all equal")


def test_slot_counts_duplicates_and_unused_slots(dev):
    rows, cols = grids()["tiles"]
    labels, _ = LC.own_maps(rows, cols, *tiles(), 3)["blobs"]
    for objects in ([4], [4, 9], [9, 4, 9, -1, 4], [-1], [-5, -1], [13, 13], [77, 78], list(range(13, -1, -1)) * 4 + [-1] * 8):
        ref = check(dev, f"slots {objects[:6]}", labels, np.array(objects, np.int32), cols, 4, 7, 8)
    assert ref["cells"][14:].sum() == 0 and (ref["nearest"][14:] == -1).all()


def raw(dev, labels, objects, cols, radius, from_cell, topn, fill):
    """The entry point on buffers of this test's own, filled with `fill` bytes before the call."""
    from embodied_object_detection_amd import _lib
    from embodied_object_detection_amd.ops import _stream
    K, T = len(objects), topn
    dl, do = torch.from_numpy(labels).to(dev), torch.from_numpy(objects).to(dev)
    shapes = dict(pair_key=(K, K), min_d2=(K, K), closest=(K, K), near_cells=(K, K), edges=(K, K), cells=(K,), nearest=(K, T),
                  nearest_d2=(K, T), from_key=(K,), from_d2=(K,), from_closest=(K,))
    out = {}
    for k, shape in shapes.items():
        wide = k in ("pair_key", "from_key")
        t = torch.full((int(np.prod(shape)) * (8 if wide else 4),), fill, dtype=torch.uint8, device=dev)
        out[k] = t.view(torch.int64 if wide else torch.int32).view(shape)
    order = ("pair_key", "min_d2", "closest", "near_cells", "edges", "cells", "nearest", "nearest_d2", "from_key", "from_d2", "from_closest")
    _lib.check(_lib.load().eod_map_relations(dl.data_ptr(), do.data_ptr(), labels.size, K, cols, radius, from_cell, T,
                                             *[out[k].data_ptr() for k in order], _stream()), "eod_map_relations")
    return LC.host(out)


def test_dirty_buffers_and_repeated_calls(dev):
    rows, cols = grids()["tiles"]
    for name in ("blobs", "64 alternating", "long shared borders"):
        labels, objects = LC.own_maps(rows, cols, *tiles(), 5)[name]
        ref = LC.reference(labels, objects, cols, 5, 40, 8)
        for fill in (0xFF, 0x00, 0x5A):
            assert not LC.differences(raw(dev, labels, objects, cols, 5, 40, 8, fill), ref), (name, fill)
        a, b = run(dev, labels, objects, cols, 5, 40, 8), run(dev, labels, objects, cols, 5, 40, 8)
        assert not LC.differences(a, b) and not LC.differences(a, ref), name


def test_permuted_slots_permute_rows_and_columns(dev):
    rows, cols = grids()["tiles"]
    rng = np.random.default_rng(5)
    for name in ("blobs", "64 alternating", "astride the tile borders"):
        labels, objects = LC.own_maps(rows, cols, *tiles(), 4)[name]
        assert len(set(objects.tolist())) == objects.size             # distinct slots
        base = run(dev, labels, objects, cols, 4, 11, 8)
        assert not LC.differences(base, LC.reference(labels, objects, cols, 4, 11, 8))
        p = rng.permutation(objects.size)
        got = run(dev, labels, np.ascontiguousarray(objects[p]), cols, 4, 11, 8)      # slot k of `got` is slot p[k] of `base`
        for k in LC.MATRIX_KEYS:
            assert np.array_equal(got[k], base[k][np.ix_(p, p)]), (name, k)
        for k in ("cells", "from_key", "from_d2", "from_closest"):
            assert np.array_equal(got[k], base[k][p]), (name, k)
        assert np.array_equal(got["nearest_d2"], base["nearest_d2"][p]), name          # the distances stay; the ties are re-ranked
        inv = np.argsort(p)
        for k in range(objects.size):
            mine = sorted((int(base["min_d2"][p[k], b]), int(inv[b])) for b in range(objects.size) if base["min_d2"][p[k], b] < INT_MAX)[:8]
            assert got["nearest"][k].tolist() == [b for _, b in mine] + [-1] * (8 - len(mine)), (name, k)


# ---- the models ------------------------------------------------------------------------------------------------------------------
MAP = (24, 24)


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


LEVEL = 2.0 ** -11                                                   # below any argmax probability: every labelled cell is in an object


def _against_reference(rel, inv, radius, from_cell, topn):
    ref = LC.reference(inv["object_labels"].cpu().numpy(), inv["object"].cpu().numpy(), MAP[1], radius, from_cell, topn)
    bad = LC.differences(LC.host(rel), ref)
    assert not bad, bad
    return ref


def test_model_relations_equal_the_reference_and_change_nothing(dev, synthetic_sd):
    from embodied_object_detection_amd import _lib, build_model
    model = build_model(_cfg(), synthetic_sd)
    frames = _frames(4)
    for f in frames[:3]:
        model([[f]])
    inv = model.inventory(thresh=0.0, map_shape=MAP, level=LEVEL)
    assert int(inv["count"]) >= 2, "the synthetic map holds too few objects for this test"
    before = dict(mem=model.implicit_memory.clone(), obs=model.observations.clone(), lab=inv["object_labels"].clone())
    for radius, fc, topn in ((2, None, 4), (1, 0, 1), (16, 24 * 11 + 7, 8)):
        rel = model.relations(inv["object"], inv["object_labels"], map_shape=MAP, radius=radius, from_cell=fc, topn=topn)
        ref = _against_reference(rel, inv, radius, -1 if fc is None else fc, topn)
    assert np.array_equal(ref["cells"], inv["area"].cpu().numpy())                # an object's cells are its area
    print(f"model.relations: {int(inv['count'])} objects of {ref['cells'][ref['cells'] > 0].tolist()} cells, "
          f"{int((ref['min_d2'] < INT_MAX).sum()) // 2} pairs within 16 cells, from_d2 {ref['from_d2'].tolist()}")
    rel2 = model.relations(inv["object"].tolist(), inv["object_labels"], map_shape=MAP)          # a sequence will do; the defaults
    _against_reference(rel2, inv, 2, -1, 4)
    with pytest.raises(_lib.EodError, match="map_shape"):
        model.relations(inv["object"], inv["object_labels"])
    with pytest.raises(_lib.EodError, match="map_shape"):
        model.relations(inv["object"], inv["object_labels"], map_shape=(24, 23))
    with pytest.raises(_lib.EodError, match="radius"):
        model.relations(inv["object"], inv["object_labels"], map_shape=MAP, radius=17)
    assert torch.equal(model.implicit_memory, before["mem"]) and torch.equal(model.observations, before["obs"])
    assert torch.equal(inv["object_labels"], before["lab"])
    # the next frame after the queries against a run that never asked
    other = build_model(_cfg(), synthetic_sd)
    for f in frames[:3]:
        other([[f]])
    for a, b in zip(_out(other, frames[3]), _out(model, frames[3])):
        assert torch.equal(a, b)
    assert torch.equal(other.implicit_memory, model.implicit_memory) and torch.equal(other.observations, model.observations)


def test_predictor_relations(dev, synthetic_sd):
    from embodied_object_detection_amd.engine.predictor import EmbodiedPredictor
    pred = EmbodiedPredictor(_cfg(), synthetic_sd)
    frames = _frames(4)
    for f in frames[:3]:
        pred.model([[f]])
    inv = pred.inventory(thresh=0.0, map_shape=MAP, level=LEVEL)
    rel = pred.relations(inv["object"], inv["object_labels"], map_shape=MAP, radius=3, from_cell=5, topn=8)
    _against_reference(rel, inv, 3, 5, 8)
    other = EmbodiedPredictor(_cfg(), synthetic_sd)
    for f in frames[:3]:
        other.model([[f]])
    for a, b in zip(_out(other.model, frames[3]), _out(pred.model, frames[3])):
        assert torch.equal(a, b)


def test_lockstep_relations(dev, synthetic_sd):
    from embodied_object_detection_amd.modeling.lockstep import LockstepScenes
    seqs = [_frames(4, 0), _frames(4, 1)]
    ls = LockstepScenes(_cfg(), 2, synthetic_sd)
    ls([s[:3] for s in seqs])
    inv = ls.inventory(None, thresh=0.0, map_shape=MAP, level=LEVEL)
    assert inv["object"].shape == (2, 16) and inv["object_labels"].shape == (2, 24 * 24)
    rel = ls.relations(inv["object"], inv["object_labels"], map_shape=MAP, radius=3, from_cell=30, topn=8)
    for b in (0, 1):
        one = {k: t[b] for k, t in inv.items() if k in ("object", "object_labels")}
        _against_reference({k: t[b] for k, t in rel.items()}, one, 3, 30, 8)
        single = ls.relations(inv["object"][b], inv["object_labels"][b], map_shape=MAP, radius=3, from_cell=30, topn=8)
        assert not LC.differences(LC.host(single), LC.host({k: t[b] for k, t in rel.items()}))
    other = LockstepScenes(_cfg(), 2, synthetic_sd)
    other([s[:3] for s in seqs])
    got, want = ls([s[3:] for s in seqs]), other([s[3:] for s in seqs])
    for g, w in zip(got, want):
        for a, b in zip(g, w):
            ia, ib = a["instances"], b["instances"]
            assert torch.equal(ia.pred_boxes.tensor, ib.pred_boxes.tensor) and torch.equal(ia.scores, ib.scores)
            assert torch.equal(ia.pred_classes, ib.pred_classes) and torch.equal(ia.pred_masks, ib.pred_masks)
