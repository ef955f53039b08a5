"""`ops.map_clearance` on the GPU against the brute-force reference of `_clearance_cases.py`: exact integer equality of every
output, on the smallest grids at which the kernels can go wrong, then beyond the reference (dirty buffers, repeated calls, permuted
slots), the route on the inflated map against the Dijkstra reference of `_route_cases.py`, and the three model surfaces.  No
tolerance anywhere."""
import numpy as np
import pytest
import torch

import _clearance_cases as CC
import _inventory_cases as IC
import _route_cases as RC

pytestmark = pytest.mark.gpu

INT_MAX = CC.INT_MAX


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    from embodied_object_detection_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def tiles():
    from embodied_object_detection_amd import ops
    return ops.CLEARANCE_TILE_ROWS, ops.CLEARANCE_CHUNK_COLS, ops.CLEARANCE_HALO_COLS


def grids():
    """1 x 1, one row, one column, a partial tile and chunk, two chunks and a remainder under many tile rows, and a grid whose rows
    reach beyond the halo of the first chunk and of the last."""
    tr, cc, halo = tiles()
    return {"1x1": (1, 1), "1x70": (1, 70), "70x1": (70, 1), "partial": (tr - 1, cc - 3), "tiles": (70, cc + 3),
            "wide": (4 * tr + 3, 2 * cc + halo + 3)}


def run(dev, labels, objects, cols, radius2=0, keep_cell=-1, passable=()):
    from embodied_object_detection_amd import ops
    dl, do = torch.from_numpy(np.ascontiguousarray(labels)).to(dev), torch.from_numpy(np.ascontiguousarray(objects)).to(dev)
    dp = torch.from_numpy(np.ascontiguousarray(passable, dtype=np.int32)).to(dev) if len(passable) else None
    out = ops.map_clearance(dl, do, cols, radius2=radius2, keep_cell=keep_cell, passable=dp)
    N, K = labels.size, len(objects)
    assert sorted(out) == sorted(CC.KEYS)
    for k in CC.CELL_KEYS:
        assert out[k].shape == (N,) and out[k].dtype == torch.int32 and out[k].is_contiguous(), k
    for k in CC.SLOT_KEYS:
        assert out[k].shape == (K,) and out[k].dtype == (torch.int64 if k == "widest_key" else torch.int32), k
    assert out["open_key"].shape == (1,) and out["open_key"].dtype == torch.int64
    assert out["counts"].shape == (3,) and out["status"].shape == (2,)
    assert torch.equal(dl.cpu(), torch.from_numpy(labels)) and torch.equal(do.cpu(), torch.from_numpy(objects))     # read-only
    if dp is not None:
        assert torch.equal(dp.cpu(), torch.from_numpy(np.ascontiguousarray(passable, dtype=np.int32)))
    return out


def check(dev, tag, m, cols, radius2=None, keep_cell=None):
    radius2 = m["radius2"] if radius2 is None else radius2
    keep_cell = m["keep_cell"] if keep_cell is None else keep_cell
    got = CC.host(run(dev, m["labels"], m["objects"], cols, radius2, keep_cell, m["passable"]))
    ref = CC.reference(m["labels"], m["objects"], cols, radius2, keep_cell, m["passable"])
    bad = CC.differences(got, ref)
    assert not bad, (tag, radius2, keep_cell, bad, {k: (got[k], ref[k]) for k in bad[:2]})
    return ref


@pytest.mark.parametrize("grid", ["1x1", "1x70", "70x1", "partial", "tiles", "wide"])
def test_own_maps(dev, grid):
    rows, cols = grids()[grid]
    maps = CC.maps(rows, cols, *tiles())
    for name, m in maps.items():
        ref = check(dev, f"{grid} {name}", m, cols)
        if m["radius2"]:
            zero = check(dev, f"{grid} {name}", m, cols, radius2=0)
            assert np.array_equal(zero["inflated"], m["labels"]) and zero["counts"][2] == 0, name         # bit for bit the labels
            assert np.array_equal(zero["d2"], ref["d2"]) and np.array_equal(zero["nearest"], ref["nearest"]), name
    ref = CC.reference(maps["no blocked cell"]["labels"], maps["no blocked cell"]["objects"], cols, 4)
    assert (ref["d2"] == INT_MAX).all() and (ref["nearest"] == -1).all() and ref["open_key"][0] == (INT_MAX << 32) | 0xFFFFFFFF
    if grid == "wide":
        tr, cc, halo = tiles()
        assert len(maps) == 27
        m = maps["corner 00"]                                        # seen from the far corner: across every chunk, beyond every halo
        ref = CC.reference(m["labels"], m["objects"], cols, m["radius2"])
        assert ref["d2"][-1] == (rows - 1) ** 2 + (cols - 1) ** 2 and cols - 1 > cc + halo
        m = maps["row-end pair"]
        ref = CC.reference(m["labels"], m["objects"], cols, m["radius2"])
        assert ref["d2"][rows // 2 * cols] == 1 + (cols - 1) ** 2
    print(f"{grid}: {len(maps)} maps, all equal")


@pytest.mark.parametrize("grid", ["tiles", "wide"])
def test_radius_and_keep_cell(dev, grid):
    """radius2 0, 1, 2, 4, 25 and one larger than the map, each with no keep_cell, one on a free cell, one on a blocked cell and one
    beside an object."""
    rows, cols = grids()[grid]
    maps = CC.maps(rows, cols, *tiles())
    for name in ("64 objects", "a slot made passable", "borders +0"):
        m = maps[name]
        blocked = CC.blocked_cells(m["labels"], m["passable"])
        base = CC.reference(m["labels"], m["objects"], cols, 0, -1, m["passable"])
        on_free = int(np.flatnonzero(base["d2"] >= 9)[0])
        on_blocked = int(np.flatnonzero(blocked)[len(np.flatnonzero(blocked)) // 2])
        beside = int(np.flatnonzero(base["d2"] == 1)[-1])
        for radius2 in (0, 1, 2, 4, 25, rows * rows + cols * cols):
            for keep in (-1, on_free, on_blocked, beside):
                ref = check(dev, f"{grid} {name}", m, cols, radius2=radius2, keep_cell=keep)
                if keep >= 0 and not blocked[keep]:
                    assert ref["inflated"][keep] == m["labels"][keep]                      # the robot's own cell stays free
            if radius2 == 25:
                assert ref["counts"][2] > 0, (name, radius2)
            elif radius2 > 25:
                assert ref["counts"][2] == 0, (name, radius2)      # every cell is within a radius larger than the map of keep_cell
        whole = CC.reference(m["labels"], m["objects"], cols, rows * rows + cols * cols, -1, m["passable"])
        assert np.array_equal(whole["inflated"], whole["owner"]) and whole["counts"][2] == whole["counts"][1]


@pytest.mark.parametrize("grid", ["partial", "tiles"])
def test_inventory_maps(dev, grid):
    """The object_labels and objects that the inventory's reference gives on its hostile maps."""
    rows, cols = grids()[grid]
    tr, cc, _ = tiles()
    n = 0
    for name, (labels, scores, keep) in IC.hostile_maps(rows, cols, tr, cc).items():
        inv = IC.reference(labels[None], scores[None], cols, IC.C5, IC.LEVEL, topk=64, keep=keep)
        objects, lab = inv["object"][0], inv["object_labels"][0]
        K = (1, 2, 5, 64)[n % 4]
        passable = [int(v) for v in objects[1:3] if v >= 0] if n % 3 == 0 else []
        m = dict(labels=lab, objects=np.ascontiguousarray(objects[:K]), passable=np.asarray(passable, np.int32))
        check(dev, f"{grid} {name}", m, cols, radius2=(0, 1, 4, 25)[n % 4], keep_cell=(-1, (n * 7) % (rows * cols))[n % 2])
        n += 1
    print(f"{grid}: {n} maps, all equal")


def test_slot_counts_duplicates_and_unused_slots(dev):
    rows, cols = grids()["tiles"]
    base = CC.maps(rows, cols, *tiles())["64 objects"]
    for objects in ([4], [4, 9], [9, 4, 9, -1, 4], [-1], [-5, -1], [13, 13], [77, 78], list(range(13, -1, -1)) * 4 + [-1] * 8):
        m = dict(base, objects=np.array(objects, np.int32))
        ref = check(dev, f"slots {objects[:6]}", m, cols)
    assert len(objects) == 64 and ref["cells"][14:].sum() == 0 and ref["territory"][14:].sum() == 0 and (ref["widest_cell"][14:] == -1).all()
    assert (ref["cells"][:14] > 0).all() and ref["territory"][:14].sum() > 0


def raw(dev, m, cols, fill):
    """The entry point on buffers of this test's own, outputs and workspace filled with `fill` bytes before the call."""
    from embodied_object_detection_amd import _lib, ops
    from embodied_object_detection_amd.ops import _stream
    labels, objects, passable = m["labels"], m["objects"], m["passable"]
    N, K, P = labels.size, len(objects), len(passable)
    dl, do = torch.from_numpy(labels).to(dev), torch.from_numpy(objects).to(dev)
    dp = torch.from_numpy(passable).to(dev) if P else None
    shapes = dict(d2=(N,), nearest=(N,), owner=(N,), inflated=(N,), cells=(K,), territory=(K,), widest_key=(K,), widest_d2=(K,),
                  widest_cell=(K,), open_key=(1,), counts=(3,), status=(2,))
    out = {}
    for k, shape in shapes.items():
        wide = k in ("widest_key", "open_key")
        t = torch.full((int(np.prod(shape)) * (8 if wide else 4),), fill, dtype=torch.uint8, device=dev)
        out[k] = t.view(torch.int64 if wide else torch.int32).view(shape)
    words = ops.map_clearance_workspace(N, cols)
    ws = torch.full((words * 4,), fill, dtype=torch.uint8, device=dev).view(torch.int32)
    _lib.check(_lib.load().eod_map_clearance(dl.data_ptr(), do.data_ptr(), dp.data_ptr() if P else None, N, K, P, cols, m["radius2"],
                                             m["keep_cell"], *[out[k].data_ptr() for k in shapes], ws.data_ptr(), words * 4, _stream()),
               "eod_map_clearance")
    return out


def test_dirty_buffers_and_repeated_calls(dev):
    rows, cols = grids()["wide"]
    maps = CC.maps(rows, cols, *tiles())
    for name in ("64 objects", "labels and slots that name nothing", "no blocked cell", "every cell blocked", "a slot made passable"):
        m = maps[name]
        ref = CC.reference(m["labels"], m["objects"], cols, m["radius2"], m["keep_cell"], m["passable"])
        for fill in (0xFF, 0x00, 0x5A):
            assert not CC.differences(CC.host(raw(dev, m, cols, fill)), ref), (name, fill)
        a, b = (CC.host(run(dev, m["labels"], m["objects"], cols, m["radius2"], m["keep_cell"], m["passable"])) for _ in range(2))
        assert not CC.differences(a, b) and not CC.differences(a, ref), name


def test_permuted_slots_permute_results(dev):
    rows, cols = grids()["tiles"]
    rng = np.random.default_rng(5)
    m = CC.maps(rows, cols, *tiles())["64 objects"]
    objects = m["objects"]
    assert len(set(objects.tolist())) == objects.size                 # distinct slots
    base = CC.host(run(dev, m["labels"], objects, cols, 4, m["keep_cell"]))
    p = rng.permutation(objects.size)
    got = CC.host(run(dev, m["labels"], np.ascontiguousarray(objects[p]), cols, 4, m["keep_cell"]))
    for k in CC.SLOT_KEYS:
        assert np.array_equal(got[k], base[k][p]), k                  # slot k of `got` is slot p[k] of `base`
    for k in CC.CELL_KEYS + ("open_key", "counts", "status"):
        assert np.array_equal(got[k], base[k]), k
    assert base["territory"].sum() == base["counts"][1]               # every blocked cell has a slot here: the territories partition the free space


# ---- the route on the inflated map ----------------------------------------------------------------------------------------------
def test_route_for_a_body_closes_the_gap_a_point_passes(dev):
    """A wall with a gap one cell wide: open at radius2 = 0, closed at radius2 = 1.  `ops.map_route` on `inflated` equals the
    Dijkstra reference on the reference's `inflated`."""
    from embodied_object_detection_amd import ops
    rows, cols = 11, 14
    g, gap = CC.wall_with_gap(rows, cols)
    labels, objects = g.reshape(-1), np.array([10, CC.WALL], np.int32)
    costs = {}
    for radius2 in (0, 1, 2):
        ref = CC.reference(labels, objects, cols, radius2, 0)
        clr = run(dev, labels, objects, cols, radius2, 0)
        assert not CC.differences(CC.host(clr), ref)
        route = ops.map_route(clr["inflated"], torch.from_numpy(objects).to(dev), cols, 0, path_max=64, sweeps=64)
        want = RC.reference(ref["inflated"], objects, cols, 0, (), 64)
        assert not RC.differences(RC.host(route), want), radius2
        costs[radius2] = int(want["goal_cost"][0])
        assert (ref["inflated"][gap] == -1) == (radius2 == 0)
    assert costs[0] < INT_MAX and costs[1] == INT_MAX and costs[2] == INT_MAX, costs
    # a second gap three cells wide: the body of radius2 = 1 takes the detour through it
    g[rows // 2, cols - 4:cols - 1] = -1
    labels = g.reshape(-1)
    ref0, ref1 = (CC.reference(labels, objects, cols, r2, 0) for r2 in (0, 1))
    clr = run(dev, labels, objects, cols, 1, 0)
    route = ops.map_route(clr["inflated"], torch.from_numpy(objects).to(dev), cols, 0, path_max=64, sweeps=64)
    want = RC.reference(ref1["inflated"], objects, cols, 0, (), 64)
    assert not RC.differences(RC.host(route), want)
    point = RC.reference(ref0["inflated"], objects, cols, 0, (), 64)
    assert np.array_equal(ref0["inflated"], labels) and point["goal_cost"][0] < want["goal_cost"][0] < INT_MAX
    assert gap in point["path"][0] and gap not in want["path"][0]


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


def _against_reference(clr, inv, radius2=0, keep_cell=-1, passable=()):
    ref = CC.reference(inv["object_labels"].cpu().numpy(), inv["object"].cpu().numpy(), MAP[1], radius2, keep_cell, passable)
    bad = CC.differences(CC.host(clr), ref)
    assert not bad, bad
    return ref


def _route_with_body(route, inv, from_cell, body_radius2, passable=(), path_max=256):
    """The dict of `route(..., body_radius2=)`: the clearance's outputs, and the route's on the reference's inflated map."""
    ref = CC.reference(inv["object_labels"].cpu().numpy(), inv["object"].cpu().numpy(), MAP[1], body_radius2, from_cell, passable)
    assert sorted(route) == sorted(RC.KEYS + ("clearance_d2", "inflated_labels"))
    assert np.array_equal(route["clearance_d2"].cpu().numpy(), ref["d2"]) and np.array_equal(route["inflated_labels"].cpu().numpy(), ref["inflated"])
    want = RC.reference(ref["inflated"], inv["object"].cpu().numpy(), MAP[1], from_cell, passable, path_max)
    bad = RC.differences(RC.host(route), want)
    assert not bad, bad
    return want


def test_model_clearance_and_route_with_a_body_change_nothing(dev, synthetic_sd):
    from embodied_object_detection_amd import _lib, build_model
    model = build_model(_cfg(), synthetic_sd)
    frames = _frames(4)
    for f in frames[:3]:
        model([[f]])
    inv = model.inventory(thresh=0.0, map_shape=MAP, level=LEVEL)
    assert int(inv["count"]) >= 2, "the synthetic map holds too few objects for this test"
    before = dict(mem=model.implicit_memory.clone(), obs=model.observations.clone(), lab=inv["object_labels"].clone())
    first = int(inv["object"][0])
    for radius2, keep, passable in ((0, None, None), (4, 24 * 11 + 7, [first]), (1, 0, None), (2 * 24 * 24, None, None)):
        clr = model.clearance(inv["object"], inv["object_labels"], map_shape=MAP, radius2=radius2, keep_cell=keep, passable=passable)
        ref = _against_reference(clr, inv, radius2, -1 if keep is None else keep, passable or ())
    assert np.array_equal(ref["cells"], inv["area"].cpu().numpy())                # an object's cells are its area
    ref = _against_reference(model.clearance(inv["object"].tolist(), inv["object_labels"], map_shape=MAP, radius2=2), inv, 2)
    print(f"model.clearance: {int(inv['count'])} objects of {ref['cells'][ref['cells'] > 0].tolist()} cells, territory "
          f"{ref['territory'].tolist()}, widest_d2 {ref['widest_d2'].tolist()}, counts {ref['counts'].tolist()}")
    # body_radius2=None: the keys and the bits of the call without the keyword
    plain = model.route(inv["object"], inv["object_labels"], map_shape=MAP, from_cell=5, path_max=64)
    none = model.route(inv["object"], inv["object_labels"], map_shape=MAP, from_cell=5, path_max=64, body_radius2=None)
    assert sorted(plain) == sorted(none) == sorted(RC.KEYS) and not RC.differences(RC.host(none), RC.host(plain))
    zero = model.route(inv["object"], inv["object_labels"], map_shape=MAP, from_cell=5, path_max=64, body_radius2=0)
    assert not RC.differences(RC.host(zero), RC.host(plain)) and torch.equal(zero["inflated_labels"], inv["object_labels"])
    for fc, r2, passable in ((5, 1, None), (24 * 11 + 7, 4, [first]), (24 * 24 - 1, 2, None)):
        route = model.route(inv["object"], inv["object_labels"], map_shape=MAP, from_cell=fc, passable=passable, path_max=64, body_radius2=r2)
        want = _route_with_body(route, inv, fc, r2, passable or (), 64)
    assert (want["cells"] >= inv["area"].cpu().numpy()).all()                     # `cells` counts the inflated cells
    with pytest.raises(_lib.EodError, match="map_shape"):
        model.clearance(inv["object"], inv["object_labels"])
    with pytest.raises(_lib.EodError, match="radius2"):
        model.clearance(inv["object"], inv["object_labels"], map_shape=MAP, radius2=-1)
    with pytest.raises(_lib.EodError, match="from_cell"):
        model.route(inv["object"], inv["object_labels"], map_shape=MAP, body_radius2=1)
    assert torch.equal(model.implicit_memory, before["mem"]) and torch.equal(model.observations, before["obs"])
    assert torch.equal(inv["object_labels"], before["lab"])
    # the next frame after the queries against a run that never asked
    other = build_model(_cfg(), synthetic_sd)
    for f in frames[:3]:
        other([[f]])
    for a, b in zip(_out(other, frames[3]), _out(model, frames[3])):
        assert torch.equal(a, b)
    assert torch.equal(other.implicit_memory, model.implicit_memory) and torch.equal(other.observations, model.observations)


def test_predictor_clearance(dev, synthetic_sd):
    from embodied_object_detection_amd.engine.predictor import EmbodiedPredictor
    pred = EmbodiedPredictor(_cfg(), synthetic_sd)
    frames = _frames(4)
    for f in frames[:3]:
        pred.model([[f]])
    inv = pred.inventory(thresh=0.0, map_shape=MAP, level=LEVEL)
    clr = pred.clearance(inv["object"], inv["object_labels"], map_shape=MAP, radius2=4, keep_cell=30)
    _against_reference(clr, inv, 4, 30)
    route = pred.route(inv["object"], inv["object_labels"], map_shape=MAP, from_cell=30, path_max=64, body_radius2=1)
    _route_with_body(route, inv, 30, 1, (), 64)
    other = EmbodiedPredictor(_cfg(), synthetic_sd)
    for f in frames[:3]:
        other.model([[f]])
    for a, b in zip(_out(other.model, frames[3]), _out(pred.model, frames[3])):
        assert torch.equal(a, b)


def test_lockstep_clearance(dev, synthetic_sd):
    from embodied_object_detection_amd import _lib
    from embodied_object_detection_amd.modeling.lockstep import LockstepScenes
    seqs = [_frames(4, 0), _frames(4, 1)]
    ls = LockstepScenes(_cfg(), 2, synthetic_sd)
    ls([s[:3] for s in seqs])
    inv = ls.inventory(None, thresh=0.0, map_shape=MAP, level=LEVEL)
    assert inv["object"].shape == (2, 16) and inv["object_labels"].shape == (2, 24 * 24)
    keeps = (30, 24 * 20 + 3)
    clr = ls.clearance(inv["object"], inv["object_labels"], map_shape=MAP, radius2=4, keep_cell=keeps)
    same = ls.clearance(inv["object"], inv["object_labels"], map_shape=MAP, radius2=4, keep_cell=30)
    free = ls.clearance(inv["object"], inv["object_labels"], map_shape=MAP, radius2=4)
    route = ls.route(inv["object"], inv["object_labels"], map_shape=MAP, from_cell=keeps, path_max=64, body_radius2=1)
    assert clr["d2"].shape == (2, 24 * 24) and clr["open_key"].shape == (2, 1) and clr["widest_key"].shape == (2, 16)
    for b in (0, 1):
        one = {k: t[b] for k, t in inv.items() if k in ("object", "object_labels")}
        _against_reference({k: t[b] for k, t in clr.items()}, one, 4, keeps[b])
        _against_reference({k: t[b] for k, t in same.items()}, one, 4, 30)
        _against_reference({k: t[b] for k, t in free.items()}, one, 4, -1)
        _route_with_body({k: t[b] for k, t in route.items()}, one, keeps[b], 1, (), 64)
        single = ls.clearance(inv["object"][b], inv["object_labels"][b], map_shape=MAP, radius2=4, keep_cell=keeps[b])
        assert not CC.differences(CC.host(single), CC.host({k: t[b] for k, t in clr.items()}))
    with pytest.raises(_lib.EodError, match="keep_cell"):
        ls.clearance(inv["object"], inv["object_labels"], map_shape=MAP, keep_cell=(1, 2, 3))
    other = LockstepScenes(_cfg(), 2, synthetic_sd)
    other([s[:3] for s in seqs])
    got, want = ls([s[3:] for s in seqs]), other([s[3:] for s in seqs])
    for g, w in zip(got, want):
        for a, b in zip(g, w):
            ia, ib = a["instances"], b["instances"]
            assert torch.equal(ia.pred_boxes.tensor, ib.pred_boxes.tensor) and torch.equal(ia.scores, ib.scores)
            assert torch.equal(ia.pred_classes, ib.pred_classes) and torch.equal(ia.pred_masks, ib.pred_masks)
