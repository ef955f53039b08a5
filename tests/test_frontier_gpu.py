"""`ops.map_cover` and `ops.map_frontier` on the GPU against the reference of `_frontier_cases.py`: exact integer equality of every
output on the smallest grids that reach each mechanism (a tile corner, several tiles, a ragged last tile, one row, long merge chains,
more frontiers than slots), then beyond the reference (dirty buffers, repeated calls), and the three model surfaces.  No tolerance
anywhere."""
import numpy as np
import pytest
import torch

import _frontier_cases as FC

pytestmark = pytest.mark.gpu

INT_MAX = FC.INT_MAX
PASSABLE = (2,)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    from embodied_object_detection_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def run(dev, labels, seen, cols, since=0, dist=None, from_cell=-1, passable=PASSABLE, min_cells=1, topk=16, rank_by=1):
    from embodied_object_detection_amd import ops
    dl, ds = torch.from_numpy(np.ascontiguousarray(labels)).to(dev), torch.from_numpy(np.ascontiguousarray(seen)).to(dev)
    dd = None if dist is None else torch.from_numpy(np.ascontiguousarray(dist)).to(dev)
    dp = torch.from_numpy(np.asarray(passable, np.int32)).to(dev) if len(passable) else None
    out = ops.map_frontier(dl, ds, cols, since=since, dist=dd, from_cell=from_cell, passable=dp, min_cells=min_cells, topk=topk,
                           rank_by=rank_by)
    N = labels.size
    assert sorted(out) == sorted(FC.KEYS)
    for k in FC.CELL_KEYS:
        assert out[k].shape == (N,) and out[k].dtype == torch.int32 and out[k].is_contiguous(), k
    for k in FC.SLOT_KEYS:
        assert out[k].shape[0] == topk and out[k].dtype == (torch.int64 if k in FC.WIDE else torch.int32), k
    assert out["bbox"].shape == (topk, 4) and out["sum_rc"].shape == (topk, 2) and out["count"].shape == (1,)
    assert out["counts"].shape == (5,) and out["status"].shape == (2,)
    assert torch.equal(dl.cpu(), torch.from_numpy(labels)) and torch.equal(ds.cpu(), torch.from_numpy(seen))         # read-only
    return out


def check(dev, tag, labels, seen, cols, **kw):
    got = FC.host(run(dev, labels, seen, cols, **kw))
    kw.setdefault("passable", PASSABLE)
    kw.setdefault("min_cells", 1)
    ref = FC.reference(labels, seen, cols, **kw)
    bad = FC.differences(got, ref)
    assert not bad, (tag, kw, bad, {k: (got[k], ref[k]) for k in bad[:2]})
    return ref


def test_hand_worked_map(dev):
    labels, seen, cols, since, here = FC.hand_map()
    for rank_by, first in ((0, 32), (1, 20)):
        ref = check(dev, "hand", labels, seen, cols, since=since, from_cell=here, passable=(), topk=3, rank_by=rank_by)
        assert ref["counts"].tolist() == [5, 24, 19, 3, 2] and ref["frontier"].tolist()[0] == first
    shut = labels.copy()
    shut[20] = 7
    assert check(dev, "shut", shut, seen, cols, from_cell=here, passable=())["counts"].tolist() == [6, 23, 19, 2, 2]
    assert check(dev, "passable", shut, seen, cols, from_cell=here, passable=(7,))["counts"].tolist() == [5, 24, 19, 3, 2]
    assert check(dev, "since 1", labels, seen, cols, since=1, from_cell=here, passable=())["counts"].tolist() == [5, 0, 43, 0, 1]


GRIDS = {"33x33": (33, 33), "64x65": (64, 65), "31x97": (31, 97), "1x130": (1, 130), "96x96": (96, 96), "40x40": (40, 40),
         "130x1": (130, 1), "1x1": (1, 1)}


@pytest.mark.parametrize("grid", list(GRIDS))
def test_own_maps(dev, grid):
    """Every map of `_frontier_cases.maps` on the grid, the options taken in turn: both rank keys, K 1, 16 and 64, min_cells 1 and
    3, with and without from_cell, since below and between the stamps."""
    rows, cols = GRIDS[grid]
    N = rows * cols
    n = 0
    for name, m in FC.maps(rows, cols).items():
        ref = check(dev, f"{grid} {name}", m["labels"], m["last_seen"], cols, since=0 if name.startswith("all") else (0, 2, 0, 1)[n % 4],
                    rank_by=n % 2,
                    topk=(16, 64, 1)[n % 3], min_cells=(1, 1, 3)[n % 3], from_cell=(-1, (n * 37) % N, N - 1)[n % 3])
        if name == "all open":
            assert ref["counts"].tolist() == [0, N, 0, 0, 0] and ref["count"][0] == 0
        if name == "all unknown":
            assert ref["counts"].tolist() == [0, 0, N, 0, 1] and ref["unknown_area"][0] == N
        if name == "all blocked":
            assert ref["counts"].tolist() == [N, 0, 0, 0, 0]
        n += 1
    print(f"{grid}: {n} maps, all equal")


@pytest.mark.parametrize("grid", ["33x33", "64x65"])
def test_frontier_across_a_tile_corner(dev, grid):
    """Two frontier cells whose only link is the diagonal across a four-tile corner, beside two unknown cells that touch only there."""
    rows, cols = GRIDS[grid]
    labels, seen, gadgets = FC.corner_map(rows, cols)
    for rank_by in (0, 1):
        ref = check(dev, grid, labels, seen, cols, topk=64, rank_by=rank_by)
    for a, b, u, w, anti in gadgets:
        ia, ib, iu, iw = (x[0] * cols + x[1] for x in (a, b, u, w))
        assert ref["frontier_labels"][ia] == ref["frontier_labels"][ib] == min(ia, ib)
        assert ref["unknown_labels"][iu] == iu and ref["unknown_labels"][iw] == iw
    assert {g[4] for g in gadgets} == ({False, True} if grid == "64x65" else {False})


def test_serpentine_through_every_tile(dev):
    labels, seen = FC.serpentine(96, 96)
    for rank_by in (0, 1):
        ref = check(dev, "serpentine", labels, seen, 96, from_cell=96 * 95, topk=4, rank_by=rank_by)
    assert ref["count"][0] == 1 and ref["bbox"][0].tolist() == [0, 0, 95, 95] and ref["area"][0] > 4500
    assert ref["counts"][4] == 48 and ref["reach_cell"][0] == 96 * 95 and ref["reach_cost"][0] == 0        # the robot stands on it
    # the same path with the map turned: the chains run down the columns, against the row-major order of the labels
    t_seen = np.ascontiguousarray(seen.reshape(96, 96).T).reshape(-1)
    ref = check(dev, "serpentine, transposed", labels, t_seen, 96, topk=4)
    assert ref["count"][0] == 1 and ref["counts"][4] == 48


def test_checkerboard_more_frontiers_than_slots(dev):
    labels, seen = FC.checkerboard(40, 40)
    for topk in (1, 16, 64):
        for rank_by in (0, 1):
            ref = check(dev, "checkerboard", labels, seen, 40, topk=topk, rank_by=rank_by, from_cell=40 * 20 + 20)
            assert ref["count"][0] == 400 and ref["frontier"].tolist() == [2 * (k % 20) + 80 * (k // 20) for k in range(topk)]
    ref = check(dev, "checkerboard, min_cells 3", labels, seen, 40, topk=16, min_cells=3)
    assert ref["count"][0] == 0 and (ref["frontier"] == -1).all() and ref["counts"][3] == 400
    # distinct sizes: two triples along a row and five cells joined across their corners, among the single cells
    seen = seen.reshape(40, 40).copy()
    seen[0, 0:3] = 0
    seen[4, 4:7] = 0
    seen[11, 11] = 0
    seen = seen.reshape(-1)
    for min_cells, want in ((1, 395), (2, 3), (3, 3), (4, 1), (5, 1), (6, 0)):       # a triple takes two single cells in, the five four
        for rank_by in (0, 1):
            ref = check(dev, "checkerboard, sizes", labels, seen, 40, topk=16, min_cells=min_cells, rank_by=rank_by)
            assert ref["count"][0] == want, min_cells


def test_dist_with_unreachable_cells(dev):
    rows, cols = 64, 65
    labels, seen = FC.explored(rows, cols, 1)
    base = FC.reference(labels, seen, cols, 0, None, -1, PASSABLE, 1, 16, 0)
    assert base["count"][0] >= 3 and base["area"][0] >= 4
    rng = np.random.default_rng(0)
    dist = rng.integers(0, 5000, rows * cols).astype(np.int32)
    first, second = (np.flatnonzero(base["frontier_labels"] == base["frontier"][k]) for k in (0, 1))
    dist[first[::2]] = INT_MAX                                                   # on part of one frontier
    dist[second] = INT_MAX                                                       # on all of another
    dist[np.flatnonzero(base["frontier_labels"] == base["frontier"][2])[:1]] = 0
    for rank_by in (0, 1):
        ref = check(dev, "dist", labels, seen, cols, dist=dist, from_cell=7, topk=16, rank_by=rank_by)
    ref = check(dev, "dist", labels, seen, cols, dist=dist, from_cell=-1, topk=16, rank_by=0)
    assert ref["reach_cost"][0] < INT_MAX and ref["reach_cell"][0] in first[1::2] and ref["reach_cost"][2] == 0
    assert ref["reach_cost"][1] == INT_MAX and ref["reach_cell"][1] == -1 and ref["reach_key"][1] == FC.ALL_ONES
    ref = check(dev, "dist, no way at all", labels, seen, cols, dist=np.full(rows * cols, INT_MAX, np.int32), topk=16, rank_by=0)
    assert (ref["reach_cell"] == -1).all() and (ref["area"][:3] > 0).all()


def test_from_cell_alone_and_neither(dev):
    rows, cols = 31, 97
    labels, seen = FC.explored(rows, cols, 2)
    a = check(dev, "from_cell", labels, seen, cols, from_cell=15 * 97 + 40, topk=8, rank_by=0)
    b = check(dev, "neither", labels, seen, cols, from_cell=-1, topk=8, rank_by=0)
    used = a["frontier"] >= 0
    assert used.sum() >= 2 and (b["reach_cost"][used] == 0).all() and np.array_equal(b["reach_cell"][used], b["frontier"][used])
    assert (a["reach_cost"][used] > 0).any() and np.array_equal(a["frontier"], b["frontier"])


def test_since_above_and_below_the_stamps(dev):
    rows, cols = 33, 33
    labels, seen = FC.explored(rows, cols, 1)
    assert seen.min() == -1 and seen.max() == 3
    opens = []
    for since in (-5, -1, 0, 1, 3, 4, INT_MAX, -2 ** 31):
        ref = check(dev, f"since {since}", labels, seen, cols, since=since, topk=8)
        opens.append(int(ref["counts"][1]))
    assert opens[0] == opens[1] == opens[7] > opens[2] > opens[3] > opens[4] > opens[5] == opens[6] == 0


def raw(dev, labels, seen, cols, fill, dist=None, from_cell=-1, since=0, min_cells=1, topk=16, rank_by=1):
    """The entry point on buffers of this test's own, outputs and workspace filled with `fill` bytes before the call."""
    from embodied_object_detection_amd import _lib, ops
    from embodied_object_detection_amd.ops import _stream
    N, K = labels.size, topk
    dl, ds = torch.from_numpy(labels).to(dev), torch.from_numpy(seen).to(dev)
    dd = None if dist is None else torch.from_numpy(dist).to(dev)
    dp = torch.tensor(PASSABLE, dtype=torch.int32, device=dev)
    shapes = dict(frontier_labels=(N,), unknown_labels=(N,), unknown_area=(N,), count=(1,), frontier=(K,), area=(K,), bbox=(K, 4),
                  sum_rc=(K, 2), open_edges=(K,), behind_key=(K,), behind_area=(K,), behind_label=(K,), reach_key=(K,), reach_cost=(K,),
                  reach_cell=(K,), counts=(5,), status=(2,))
    out = {}
    for k, shape in shapes.items():
        wide = k in FC.WIDE
        t = torch.full((int(np.prod(shape)) * (8 if wide else 4) + 8,), fill, dtype=torch.uint8, device=dev)[:-8]
        out[k] = t.view(torch.int64 if wide else torch.int32).view(shape)
    words = ops.map_frontier_workspace(N, cols)
    ws = torch.full((words * 4,), fill, dtype=torch.uint8, device=dev).view(torch.int32)
    _lib.check(_lib.load().eod_map_frontier(dl.data_ptr(), dp.data_ptr(), ds.data_ptr(), None if dd is None else dd.data_ptr(), N,
                                            len(PASSABLE), cols, since, from_cell, min_cells, K, rank_by,
                                            *[out[k].data_ptr() for k in shapes], ws.data_ptr(), words * 4, _stream()), "eod_map_frontier")
    return out


def test_dirty_buffers_and_repeated_calls(dev):
    rows, cols = 64, 65
    maps = FC.maps(rows, cols)
    for name in ("explored 1", "noise 0.5", "all blocked", "all unknown", "checkerboard"):
        m = maps[name]
        ref = FC.reference(m["labels"], m["last_seen"], cols, 0, None, 99, PASSABLE, 1, 16, 1)
        for fill in (0xFF, 0x00, 0x5A):
            got = FC.host(raw(dev, m["labels"], m["last_seen"], cols, fill, from_cell=99))
            assert not FC.differences(got, ref), (name, fill, FC.differences(got, ref))
        a, b = (FC.host(run(dev, m["labels"], m["last_seen"], cols, from_cell=99)) for _ in range(2))
        assert not FC.differences(a, b) and not FC.differences(a, ref), name


def test_map_cover(dev):
    from embodied_object_detection_amd import ops
    N = 5000
    rng = np.random.default_rng(4)
    want = np.full(N, -1, np.int32)
    seen = torch.full((N,), -1, dtype=torch.int32, device=dev)
    frames = []
    for stamp, shape in ((0, (37, 53)), (1, (64, 64)), (1, (5, 7, 1)), (0, (64, 64)), (5, (9,)), (3, (700,))):
        proj = rng.integers(-3, N + 3, shape).astype(np.int32)
        proj.reshape(-1)[:6] = (-1, N, 17, 17, -2 ** 31, 2 ** 31 - 1)[:proj.size]
        frames.append((stamp, proj))
        want = FC.cover_reference(proj, want, stamp, exclude_cell=17)
        got = ops.map_cover(torch.from_numpy(proj).to(dev), seen, stamp, exclude_cell=17)
        assert got is seen and np.array_equal(seen.cpu().numpy(), want), (stamp, shape)
    assert want[17] == -1 and want.max() == 5 and (want == -1).sum() > 0 and set(want.tolist()) >= {-1, 0, 1, 3}
    # the frames in another order, the pixels of each shuffled: the same record
    again = torch.full((N,), -1, dtype=torch.int32, device=dev)
    for stamp, proj in frames[::-1]:
        ops.map_cover(torch.from_numpy(rng.permutation(proj.reshape(-1))).to(dev), again, stamp, exclude_cell=17)
    assert torch.equal(again, seen)
    assert ops.map_cover(torch.zeros((0,), dtype=torch.int32, device=dev), again, 9) is again and torch.equal(again, seen)
    none = ops.map_cover(torch.from_numpy(frames[1][1]).to(dev), torch.full((N,), 7, dtype=torch.int32, device=dev), 7)
    assert (none == 7).all()                                                     # nothing to raise


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


def _against_reference(res, labels, seen, **kw):
    ref = FC.reference(labels.cpu().numpy(), seen.cpu().numpy() if torch.is_tensor(seen) else seen, MAP[1], **kw)
    bad = FC.differences(FC.host(res), ref)
    assert not bad, bad
    return ref


def _detour_map(dev):
    """24 x 24, everything covered but two patches.  The robot stands at (12, 2); the near patch lies behind a long wall (label 9 in
    column 4), the far one at the end of a free corridor: nearest by distance is not cheapest by route."""
    labels = np.full(MAP, -1, np.int32)
    labels[2:22, 4] = 9
    seen = np.zeros(MAP, np.int32)
    seen[10:15, 6:9] = -1
    seen[20:23, 2] = -1
    return torch.from_numpy(labels.reshape(-1)).to(dev), torch.from_numpy(seen.reshape(-1)).to(dev), 12 * 24 + 2


def test_model_cover_and_frontiers_change_nothing(dev, synthetic_sd):
    from embodied_object_detection_amd import _lib, build_model
    model = build_model(_cfg(), synthetic_sd)
    frames = _frames(4)
    want = np.full(24 * 24, -1, np.int32)
    with pytest.raises(_lib.EodError, match="no memory yet"):
        model.cover(frames[0]["proj_indices"])
    for t, f in enumerate(frames[:3]):
        model([[f]])
        seen = model.cover(f["proj_indices"], exclude_cell=300)
        want = FC.cover_reference(np.asarray(f["proj_indices"]), want, t, exclude_cell=300)
        assert np.array_equal(seen.cpu().numpy(), want), t
    assert want.max() == 2 and want[300] == -1 and (want >= 0).sum() >= 5      # the synthetic camera sees a few cells a frame
    inv = model.inventory(thresh=0.0, map_shape=MAP, level=LEVEL)
    before = dict(mem=model.implicit_memory.clone(), obs=model.observations.clone(), lab=inv["object_labels"].clone(), seen=seen.clone())
    here = 24 * 11 + 7
    # the synthetic inventory labels every cell (level below every probability): the largest object, the background, is the floor
    floor = [int(inv["object"][0])]
    ref = _against_reference(model.frontiers(inv["object_labels"], MAP, from_cell=here), inv["object_labels"], want, from_cell=here)
    assert ref["counts"].tolist() == [24 * 24, 0, 0, 0, 0]
    ref = _against_reference(model.frontiers(inv["object_labels"], MAP, from_cell=here, passable=floor, min_cells=1),
                             inv["object_labels"], want, from_cell=here, passable=floor, min_cells=1)
    assert ref["counts"][:3].sum() == 24 * 24 and ref["counts"][0] < 24 * 24
    print(f"model.frontiers: count {ref['count'].tolist()}, frontier {ref['frontier'][:4].tolist()}, behind_area "
          f"{ref['behind_area'][:4].tolist()}, reach_cell {ref['reach_cell'][:4].tolist()}, counts {ref['counts'].tolist()}")
    _against_reference(model.frontiers(inv["object_labels"], MAP, since=2, min_cells=1, topk=64, rank_by="area",
                                       passable=[int(inv["object"][0])]), inv["object_labels"], want, since=2, min_cells=1, topk=64,
                       rank_by=0, passable=[int(inv["object"][0])])
    # route's dist ranks the frontiers by the way there: on the detour map the nearest frontier is not the cheapest
    labels, known, robot = _detour_map(dev)
    rt = model.route([9], labels, map_shape=MAP, from_cell=robot, path_max=64)
    by_route = model.frontiers(labels, MAP, last_seen=known, route=rt, min_cells=1, topk=4)
    by_d2 = model.frontiers(labels, MAP, last_seen=known, from_cell=robot, min_cells=1, topk=4)
    r1 = _against_reference(by_route, labels, known, dist=rt["dist"].cpu().numpy(), min_cells=1, topk=4)
    r2 = _against_reference(by_d2, labels, known, from_cell=robot, min_cells=1, topk=4)
    assert r1["frontier"].tolist() == r2["frontier"].tolist() and r1["count"][0] == 2 and r1["behind_area"].tolist() == [15, 3, 0, 0]
    assert r2["reach_cost"][0] < r2["reach_cost"][1] and r1["reach_cost"][0] > r1["reach_cost"][1]      # near behind the wall, far free
    assert r2["reach_cell"][0] == 12 * 24 + 5 and r1["reach_cell"][1] == 19 * 24 + 2 and r1["reach_cost"][1] == 35
    _against_reference(model.frontiers(labels, MAP, last_seen=known, route=rt["dist"], from_cell=robot, min_cells=1, topk=4), labels,
                       known, dist=rt["dist"].cpu().numpy(), from_cell=robot, min_cells=1, topk=4)
    with pytest.raises(_lib.EodError, match="map_shape"):
        model.frontiers(inv["object_labels"])
    with pytest.raises(_lib.EodError, match="rank_by"):
        model.frontiers(inv["object_labels"], MAP, rank_by="size")
    assert torch.equal(model.implicit_memory, before["mem"]) and torch.equal(model.observations, before["obs"])
    assert torch.equal(inv["object_labels"], before["lab"]) and torch.equal(model._last_seen, before["seen"])
    # the next frame after the queries against a run that never asked; there the weaker record stands in
    other = build_model(_cfg(), synthetic_sd)
    for f in frames[:3]:
        other([[f]])
    weak = np.where(other.observations.cpu().numpy() > 0, 0, -1).astype(np.int32)
    _against_reference(other.frontiers(inv["object_labels"], MAP), inv["object_labels"], weak)
    for a, b in zip(_out(other, frames[3]), _out(model, frames[3])):
        assert torch.equal(a, b)
    assert torch.equal(other.implicit_memory, model.implicit_memory) and torch.equal(other.observations, model.observations)
    model.reset_memory(24 * 24)
    assert model._last_seen is None
    assert model.cover(frames[0]["proj_indices"], stamp=9).max() == 9 and model._cover_stamp == 10


def test_predictor_cover_and_frontiers(dev, synthetic_sd):
    from embodied_object_detection_amd.engine.predictor import EmbodiedPredictor
    pred = EmbodiedPredictor(_cfg(), synthetic_sd)
    frames = _frames(3)
    want = np.full(24 * 24, -1, np.int32)
    for t, f in enumerate(frames):
        pred.model([[f]])
        seen = pred.cover(f)
        want = FC.cover_reference(np.asarray(f["proj_indices"]), want, t)
    assert np.array_equal(seen.cpu().numpy(), want)
    inv = pred.inventory(thresh=0.0, map_shape=MAP, level=LEVEL)
    _against_reference(pred.frontiers(inv["object_labels"], map_shape=MAP, since=1, from_cell=30, min_cells=1, rank_by="area"),
                       inv["object_labels"], want, since=1, from_cell=30, min_cells=1, rank_by=0)


def test_lockstep_cover_and_frontiers(dev, synthetic_sd):
    from embodied_object_detection_amd import _lib
    from embodied_object_detection_amd.modeling.lockstep import LockstepScenes
    seqs = [_frames(3, 0), _frames(3, 1)]
    ls = LockstepScenes(_cfg(), 2, synthetic_sd)
    ls([s[:3] for s in seqs])
    want = np.full((2, 24 * 24), -1, np.int32)
    for b in (0, 1):
        for t, f in enumerate(seqs[b]):
            row = ls.cover(b, f["proj_indices"])
            want[b] = FC.cover_reference(np.asarray(f["proj_indices"]), want[b], t)
        assert np.array_equal(row.cpu().numpy(), want[b])
    assert ls._last_seen.shape == (2, 24 * 24)
    inv = ls.inventory(None, thresh=0.0, map_shape=MAP, level=LEVEL)
    labels = inv["object_labels"]
    fr = ls.frontiers(labels, MAP, from_cell=[30, 500], min_cells=1)
    assert fr["frontier_labels"].shape == (2, 24 * 24) and fr["sum_rc"].shape == (2, 16, 2) and fr["counts"].shape == (2, 5)
    for b in (0, 1):
        _against_reference({k: v[b] for k, v in fr.items()}, labels[b], want[b], from_cell=(30, 500)[b], min_cells=1)
        single = ls.frontiers(labels[b].contiguous(), MAP, from_cell=(30, 500)[b], min_cells=1, scene=b)
        assert not FC.differences(FC.host(single), FC.host({k: v[b] for k, v in fr.items()}))
    with pytest.raises(_lib.EodError, match="from_cell and route"):
        ls.frontiers(labels, MAP, from_cell=[1, 2, 3])
    with pytest.raises(_lib.EodError, match="scene="):
        ls.frontiers(labels[0].contiguous(), MAP)
