"""`ops.map_route` on the GPU against the Dijkstra reference of `_route_cases.py`: exact integer equality of every output, on the
smallest grids at which the kernels can go wrong, then beyond the reference (dirty buffers, repeated calls, permuted slots, sweeps
that run out and resumed calls) and through the three model surfaces.  No tolerance anywhere."""
import numpy as np
import pytest
import torch

import _inventory_cases as IC
import _route_cases as RC

pytestmark = pytest.mark.gpu

INT_MAX = RC.INT_MAX
SWEEPS = 256                                                         # enough for every map here (the serpentine needs 74: below)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    from embodied_object_detection_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def tiles():
    from embodied_object_detection_amd import ops
    return ops.ROUTE_TILE_ROWS, ops.ROUTE_TILE_COLS


def grids():
    tr, tc = tiles()
    return {"1x1": (1, 1), "1x70": (1, 70), "70x1": (70, 1), "partial": (tr - 5, tc - 3), "tiles": (2 * tr + 6, 2 * tc + 3)}


def run(dev, labels, objects, cols, from_cell, passable=(), path_max=256, sweeps=SWEEPS, resume=None):
    from embodied_object_detection_amd import ops
    dl, do = torch.from_numpy(np.ascontiguousarray(labels)).to(dev), torch.from_numpy(np.ascontiguousarray(objects)).to(dev)
    dp = torch.from_numpy(np.ascontiguousarray(passable, dtype=np.int32)).to(dev) if len(passable) else None
    out = ops.map_route(dl, do, cols, from_cell, passable=dp, path_max=path_max, sweeps=sweeps, resume=resume)
    N, K = labels.size, len(objects)
    assert sorted(out) == sorted(RC.KEYS)
    for k in RC.CELL_KEYS:
        assert out[k].shape == (N,) and out[k].dtype == torch.int32, k
    for k in ("goal_key", "goal_cost", "goal_cell", "cells", "path_cells"):
        assert out[k].shape == (K,) and out[k].dtype == (torch.int64 if k == "goal_key" else torch.int32), k
    assert out["path"].shape == (K, path_max) and out["counts"].shape == (2,) and out["status"].shape == (2,)
    assert torch.equal(dl.cpu(), torch.from_numpy(labels)) and torch.equal(do.cpu(), torch.from_numpy(objects))     # read-only
    return out


def check(dev, tag, m, cols, path_max=256, sweeps=SWEEPS):
    got = RC.host(run(dev, m["labels"], m["objects"], cols, m["from_cell"], m["passable"], path_max, sweeps))
    ref = RC.reference(m["labels"], m["objects"], cols, m["from_cell"], m["passable"], path_max)
    bad = RC.differences(got, ref)
    assert not bad, (tag, path_max, bad, {k: (got[k], ref[k]) for k in bad[:2]})
    return ref


@pytest.mark.parametrize("grid", ["1x1", "1x70", "70x1", "partial", "tiles"])
def test_own_maps(dev, grid):
    rows, cols = grids()[grid]
    maps = RC.maps(rows, cols, *tiles())
    for name, m in maps.items():
        ref = check(dev, f"{grid} {name}", m, cols)
        if name.startswith("open"):
            assert np.array_equal(ref["dist"], RC.open_field(rows, cols, m["from_cell"])), name
        check(dev, f"{grid} {name}", m, cols, path_max=(1, 7, 1024)[len(name) % 3])
    if grid == "tiles":
        assert len(maps) == 18
        for name in ("corner opening at the four-tile corner", "row-end pair as the only link"):
            ref = RC.reference(maps[name]["labels"], maps[name]["objects"], cols, maps[name]["from_cell"], maps[name]["passable"])
            assert ref["goal_cost"][0] == INT_MAX and ref["counts"][1] < ref["counts"][0], name
    print(f"{grid}: {len(maps)} maps x 2 calls, all equal")


def test_path_max_one_short_exact_and_one(dev):
    rows, cols = grids()["tiles"]
    maps = RC.maps(rows, cols, *tiles())
    for name in ("wall, gap one off the tile border", "spiral inside one tile", "64 objects"):
        m = maps[name]
        full = RC.reference(m["labels"], m["objects"], cols, m["from_cell"], m["passable"], 1024)
        L = int(full["path_cells"].max())
        assert 2 < L < 1024, (name, L)
        for pm in (L - 1, L, 1):
            ref = check(dev, name, m, cols, path_max=pm)
            k = int(full["path_cells"].argmax())
            assert (ref["path"][k, -1] == m["from_cell"]) == (pm == L)                     # complete exactly when it ends at the start


@pytest.mark.parametrize("grid", ["partial", "tiles"])
def test_inventory_maps(dev, grid):
    """The object_labels and objects that the inventory's reference gives on its hostile maps."""
    rows, cols = grids()[grid]
    tr, tc = tiles()
    n = 0
    for name, (labels, scores, keep) in IC.hostile_maps(rows, cols, tr, tc).items():
        inv = IC.reference(labels[None], scores[None], cols, IC.C5, IC.LEVEL, topk=64, keep=keep)
        objects, lab = inv["object"][0], inv["object_labels"][0]
        K = (1, 2, 5, 64)[n % 4]
        free = np.flatnonzero(lab < 0)
        fc = int(free[len(free) // 3]) if len(free) else (n * 7) % (rows * cols)            # a free cell, or a labelled one
        passable = [int(v) for v in objects[1:3] if v >= 0] if n % 3 == 0 else []
        m = dict(labels=lab, objects=np.ascontiguousarray(objects[:K]), passable=np.asarray(passable, np.int32), from_cell=fc)
        check(dev, f"{grid} {name}", m, cols, path_max=(256, 16)[n % 2])
        n += 1
    print(f"{grid}: {n} maps, all equal")


def test_slot_counts_duplicates_and_unused_slots(dev):
    rows, cols = grids()["tiles"]
    base = RC.maps(rows, cols, *tiles())["64 objects"]
    for objects in ([4], [4, 9], [9, 4, 9, -1, 4], [-1], [-5, -1], [13, 13], [77, 78], list(range(13, -1, -1)) * 4 + [-1] * 8):
        m = dict(base, objects=np.array(objects, np.int32))
        ref = check(dev, f"slots {objects[:6]}", m, cols, path_max=64)
    assert ref["cells"][14:].sum() == 0 and (ref["goal_cell"][14:] == -1).all() and (ref["path"][14:] == -1).all()


def raw(dev, m, cols, path_max, sweeps, fill, resume=0, dist=None):
    """The entry point on buffers of this test's own, outputs and workspace filled with `fill` bytes before the call."""
    from embodied_object_detection_amd import _lib, ops
    from embodied_object_detection_amd.ops import _stream
    labels, objects, passable = m["labels"], m["objects"], m["passable"]
    N, K, P, T = labels.size, len(objects), len(passable), path_max
    dl, do = torch.from_numpy(labels).to(dev), torch.from_numpy(objects).to(dev)
    dp = torch.from_numpy(passable).to(dev) if P else None
    shapes = dict(dist=(N,), parent=(N,), goal_key=(K,), goal_cost=(K,), goal_cell=(K,), cells=(K,), path=(K, T), path_cells=(K,),
                  counts=(2,), status=(2,))
    out = {}
    for k, shape in shapes.items():
        wide = k == "goal_key"
        t = torch.full((int(np.prod(shape)) * (8 if wide else 4),), fill, dtype=torch.uint8, device=dev)
        out[k] = t.view(torch.int64 if wide else torch.int32).view(shape)
    if dist is not None:
        out["dist"] = dist
    words = ops.map_route_workspace(N, cols)
    ws = torch.full((words * 4,), fill, dtype=torch.uint8, device=dev).view(torch.int32)
    order = ("dist", "parent", "goal_key", "goal_cost", "goal_cell", "cells", "path", "path_cells", "counts", "status")
    _lib.check(_lib.load().eod_map_route(dl.data_ptr(), do.data_ptr(), dp.data_ptr() if P else None, N, K, P, cols, m["from_cell"], T,
                                         sweeps, resume, *[out[k].data_ptr() for k in order], ws.data_ptr(), words * 4, _stream()),
               "eod_map_route")
    return out


def test_dirty_buffers_and_repeated_calls(dev):
    rows, cols = grids()["tiles"]
    maps = RC.maps(rows, cols, *tiles())
    for name in ("64 objects", "labels and slots that name nothing", "wall, gap at the tile border", "a slot made passable"):
        m = maps[name]
        ref = RC.reference(m["labels"], m["objects"], cols, m["from_cell"], m["passable"], 96)
        for fill in (0xFF, 0x00, 0x5A):
            assert not RC.differences(RC.host(raw(dev, m, cols, 96, 64, fill)), ref), (name, fill)
        a, b = (RC.host(run(dev, m["labels"], m["objects"], cols, m["from_cell"], m["passable"], 96, s)) for s in (64, 200))
        assert not RC.differences(a, b) and not RC.differences(a, ref), name


def test_permuted_slots_permute_results(dev):
    rows, cols = grids()["tiles"]
    rng = np.random.default_rng(5)
    m = RC.maps(rows, cols, *tiles())["64 objects"]
    objects = m["objects"]
    assert len(set(objects.tolist())) == objects.size                 # distinct slots
    base = RC.host(run(dev, m["labels"], objects, cols, m["from_cell"], path_max=128))
    p = rng.permutation(objects.size)
    got = RC.host(run(dev, m["labels"], np.ascontiguousarray(objects[p]), cols, m["from_cell"], path_max=128))
    for k in RC.SLOT_KEYS:
        assert np.array_equal(got[k], base[k][p]), k                  # slot k of `got` is slot p[k] of `base`
    for k in RC.CELL_KEYS + ("counts", "status"):
        assert np.array_equal(got[k], base[k]), k


def test_diagonal_step_wakes_the_tile_across_the_corner(dev):
    """Tile (0, 0) settles in sweep 0; in sweep 1 tile (1, 1), which touches it at the corner alone, takes the diagonal step and
    settles (every way into it is that step); sweep 2 lowers nothing.  Three sweeps give status 0; two do not."""
    rows, cols = grids()["tiles"]
    m = RC.maps(rows, cols, *tiles())["diagonal step across the four-tile corner"]
    ref = check(dev, "diagonal, 3 sweeps", m, cols, sweeps=3)
    tr, tc = tiles()
    assert ref["parent"][tr * cols + tc] == (tr - 1) * cols + tc - 1 and ref["goal_cost"][0] < INT_MAX
    two = RC.host(run(dev, m["labels"], m["objects"], cols, m["from_cell"], sweeps=2))
    assert two["status"].tolist() == [1, 0] and np.array_equal(two["dist"], ref["dist"])


def serpentine_crossings(rows, cols):
    """The tile borders the serpentine's path to its last corridor crosses: every corridor runs across all tile columns, and the
    path comes down through every tile row."""
    tr, tc = tiles()
    return (rows + 1) // 2 * (-(-cols // tc) - 1) + (-(-rows // tr) - 1)


def test_sweeps_run_out_and_resumed_calls_finish(dev):
    """A tile runs once per sweep, and the front of the serpentine enters a tile anew at every border it crosses, so `small`
    sweeps below the number of crossings leave the distances unsettled: status bit 0.  A sweep in which every tile saw only the
    state before it carries the front over one border, so crossings + 1 sweeps settle the map and one more sees nothing change;
    a resumed call starts with every tile active, which is no worse: ceil((crossings + 2 - small) / step) resumed calls of `step`
    sweeps reach status 0, with the bits of one call with enough sweeps."""
    rows, cols = grids()["tiles"]
    m = RC.maps(rows, cols, *tiles())["serpentine"]
    crossings = serpentine_crossings(rows, cols)
    small, step = 4, 16
    assert small < crossings and crossings + 2 <= SWEEPS
    ref = check(dev, "serpentine", m, cols, path_max=1024)
    assert ref["goal_cost"][0] < INT_MAX and ref["path_cells"][0] == 1024                  # longer than the longest path written
    res = run(dev, m["labels"], m["objects"], cols, m["from_cell"], path_max=1024, sweeps=small)
    assert int(res["status"][0]) & 1 and int(res["status"][1]) == 0
    first = res["dist"].cpu().numpy()
    assert ((first == INT_MAX) | (first >= ref["dist"])).all() and (first != ref["dist"]).any()       # upper bounds, not yet the distances
    calls = -(-(crossings + 2 - small) // step)
    done = None
    for n in range(calls):
        res = run(dev, m["labels"], m["objects"], cols, m["from_cell"], path_max=1024, sweeps=step, resume=res if n % 2 else res["dist"])
        if int(res["status"][0]) == 0:
            done = n + 1
            break
        assert int(res["status"][0]) == 1
    print(f"serpentine {rows} x {cols}: {crossings} crossings, {small} sweeps + {done} resumed calls of {step} (at most {calls})")
    assert done is not None, (crossings, calls, res["status"].tolist())
    assert not RC.differences(RC.host(res), ref)
    # the raw entry point resumes alike on dirty buffers: only dist is kept
    part = raw(dev, m, cols, 1024, small, 0x5A)
    assert int(part["status"][0]) == 1
    again = raw(dev, m, cols, 1024, SWEEPS, 0xFF, resume=1, dist=part["dist"])
    assert not RC.differences(RC.host(again), ref)


def test_model_call_resumes_by_itself(dev):
    from embodied_object_detection_amd import _lib
    from embodied_object_detection_amd.modeling.meta_arch import _route
    rows, cols = grids()["tiles"]
    m = RC.maps(rows, cols, *tiles())["serpentine"]
    ref = RC.reference(m["labels"], m["objects"], cols, m["from_cell"], m["passable"], 1024)
    labels = torch.from_numpy(m["labels"]).to(dev)
    got = _route(m["objects"].tolist(), labels, (rows, cols), m["from_cell"], None, 1024, 2)          # 2, 4, 8, ... sweeps
    assert not RC.differences(RC.host(got), ref)
    assert serpentine_crossings(rows, cols) > 2
    with pytest.raises(_lib.EodError, match="map_shape"):
        _route(m["objects"].tolist(), labels, (rows, cols + 1), m["from_cell"])


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


def _against_reference(route, inv, from_cell, passable=(), path_max=256):
    ref = RC.reference(inv["object_labels"].cpu().numpy(), inv["object"].cpu().numpy(), MAP[1], from_cell, passable, path_max)
    bad = RC.differences(RC.host(route), ref)
    assert not bad, bad
    return ref


def test_model_route_equals_the_reference_and_changes_nothing(dev, synthetic_sd):
    from embodied_object_detection_amd import _lib, build_model
    model = build_model(_cfg(), synthetic_sd)
    frames = _frames(4)
    for f in frames[:3]:
        model([[f]])
    inv = model.inventory(thresh=0.0, map_shape=MAP, level=LEVEL)
    assert int(inv["count"]) >= 2, "the synthetic map holds too few objects for this test"
    before = dict(mem=model.implicit_memory.clone(), obs=model.observations.clone(), lab=inv["object_labels"].clone())
    first = int(inv["object"][0])
    for fc, passable, pm in ((0, None, 256), (24 * 11 + 7, [first], 16), (24 * 24 - 1, None, 1)):
        route = model.route(inv["object"], inv["object_labels"], map_shape=MAP, from_cell=fc, passable=passable, path_max=pm)
        ref = _against_reference(route, inv, fc, passable or (), pm)
    assert np.array_equal(ref["cells"], inv["area"].cpu().numpy())                # an object's cells are its area
    ref = _against_reference(model.route(inv["object"].tolist(), inv["object_labels"], map_shape=MAP, from_cell=5), inv, 5)
    print(f"model.route: {int(inv['count'])} objects of {ref['cells'][ref['cells'] > 0].tolist()} cells, goal_cost "
          f"{ref['goal_cost'].tolist()}, path_cells {ref['path_cells'].tolist()}, counts {ref['counts'].tolist()}")
    with pytest.raises(_lib.EodError, match="map_shape"):
        model.route(inv["object"], inv["object_labels"], from_cell=0)
    with pytest.raises(_lib.EodError, match="from_cell"):
        model.route(inv["object"], inv["object_labels"], map_shape=MAP)
    with pytest.raises(_lib.EodError, match="path_max"):
        model.route(inv["object"], inv["object_labels"], map_shape=MAP, from_cell=0, path_max=1025)
    assert torch.equal(model.implicit_memory, before["mem"]) and torch.equal(model.observations, before["obs"])
    assert torch.equal(inv["object_labels"], before["lab"])
    # the next frame after the queries against a run that never asked
    other = build_model(_cfg(), synthetic_sd)
    for f in frames[:3]:
        other([[f]])
    for a, b in zip(_out(other, frames[3]), _out(model, frames[3])):
        assert torch.equal(a, b)
    assert torch.equal(other.implicit_memory, model.implicit_memory) and torch.equal(other.observations, model.observations)


def test_predictor_route(dev, synthetic_sd):
    from embodied_object_detection_amd.engine.predictor import EmbodiedPredictor
    pred = EmbodiedPredictor(_cfg(), synthetic_sd)
    frames = _frames(4)
    for f in frames[:3]:
        pred.model([[f]])
    inv = pred.inventory(thresh=0.0, map_shape=MAP, level=LEVEL)
    route = pred.route(inv["object"], inv["object_labels"], map_shape=MAP, from_cell=30, path_max=64)
    _against_reference(route, inv, 30, (), 64)
    other = EmbodiedPredictor(_cfg(), synthetic_sd)
    for f in frames[:3]:
        other.model([[f]])
    for a, b in zip(_out(other.model, frames[3]), _out(pred.model, frames[3])):
        assert torch.equal(a, b)


def test_lockstep_route(dev, synthetic_sd):
    from embodied_object_detection_amd import _lib
    from embodied_object_detection_amd.modeling.lockstep import LockstepScenes
    seqs = [_frames(4, 0), _frames(4, 1)]
    ls = LockstepScenes(_cfg(), 2, synthetic_sd)
    ls([s[:3] for s in seqs])
    inv = ls.inventory(None, thresh=0.0, map_shape=MAP, level=LEVEL)
    assert inv["object"].shape == (2, 16) and inv["object_labels"].shape == (2, 24 * 24)
    starts = (30, 24 * 20 + 3)
    route = ls.route(inv["object"], inv["object_labels"], map_shape=MAP, from_cell=starts, path_max=64)
    same = ls.route(inv["object"], inv["object_labels"], map_shape=MAP, from_cell=30, path_max=64)
    for b in (0, 1):
        one = {k: t[b] for k, t in inv.items() if k in ("object", "object_labels")}
        _against_reference({k: t[b] for k, t in route.items()}, one, starts[b], (), 64)
        _against_reference({k: t[b] for k, t in same.items()}, one, 30, (), 64)
        single = ls.route(inv["object"][b], inv["object_labels"][b], map_shape=MAP, from_cell=starts[b], path_max=64)
        assert not RC.differences(RC.host(single), RC.host({k: t[b] for k, t in route.items()}))
    with pytest.raises(_lib.EodError, match="from_cell"):
        ls.route(inv["object"], inv["object_labels"], map_shape=MAP, from_cell=(1, 2, 3))
    other = LockstepScenes(_cfg(), 2, synthetic_sd)
    other([s[:3] for s in seqs])
    got, want = ls([s[3:] for s in seqs]), other([s[3:] for s in seqs])
    for g, w in zip(got, want):
        for a, b in zip(g, w):
            ia, ib = a["instances"], b["instances"]
            assert torch.equal(ia.pred_boxes.tensor, ib.pred_boxes.tensor) and torch.equal(ia.scores, ib.scores)
            assert torch.equal(ia.pred_classes, ib.pred_classes) and torch.equal(ia.pred_masks, ib.pred_masks)
