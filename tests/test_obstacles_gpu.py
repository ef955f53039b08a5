"""`ops.map_heights` and `ops.map_obstacles` on the GPU against the reference of `_obstacle_cases.py`: exact integer equality of every
output.  The record on the pixel counts and cell patterns that reach each path of the kernel (one wave, a wave and a lane, several
workgroups; one cell, a cell a lane, runs across the wave and workgroup boundaries, two cells lane by lane, dropped pixels in
between, more cells than a workgroup's table holds), the query on the smallest grids that reach each mechanism (a tile corner, several tiles, a ragged last tile, one row, long
merge chains, more structures than slots), then beyond the reference (dirty buffers, repeated calls), the composition with
`ops.map_route`, and the three model surfaces.  No tolerance anywhere."""
import numpy as np
import pytest
import torch

import _obstacle_cases as OC
import _route_cases as RC

pytestmark = pytest.mark.gpu

INT_MAX, INT_MIN = OC.INT_MAX, OC.INT_MIN
BAND = (100, 1500)
PIXELS = (1, 63, 64, 65, 255, 257, 4099)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    from embodied_object_detection_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


# ---- the record --------------------------------------------------------------------------------------------------------------------
def some_heights(P, seed):
    """Heights in and round the band, a quarter of them on a band edge or a .5 mm tie."""
    rng = np.random.default_rng(seed)
    y = rng.uniform(-0.5, 2.5, P).astype(np.float32)
    special = np.array([0.1, 0.0995, 0.1005, 1.5, 1.5005, 1.4995, 0.0625, 0.0635, 0.099609375, 1.5009765625, -0.0005, 0.0, 1000.0,
                        -1000.0, 0.09949999, 1.50050001], np.float32)
    at = rng.random(P) < 0.25
    y[at] = special[rng.integers(0, special.size, int(at.sum()))]
    return y


def cell_patterns(P, N):
    """name -> int32 [P] cells."""
    p = np.arange(P)
    runs = np.repeat(np.arange(1, 131), np.arange(1, 131))               # runs of lengths 1..130: they straddle 64 and 256 many times
    out = {"one cell": np.full(P, N // 2), "a cell a pixel": p % N, "runs": (runs[p % runs.size] * 7) % N,
           "two cells lane by lane": np.where(p % 2 == 0, 3, N - 1)}
    bad = np.array([-1, N, -2 ** 31, 2 ** 31 - 1, 5, N + 7])             # 5 is the excluded cell
    mixed = (p // 3) % N
    mixed[p % 4 == 1] = bad[(p[p % 4 == 1] // 4) % bad.size]
    out["dropped in between"] = mixed
    return {k: v.astype(np.int32) for k, v in out.items()}


def run_heights(dev, proj, y, record, band=BAND, exclude_cell=5, xyz=False):
    from embodied_object_detection_amd import ops
    dp = torch.from_numpy(np.ascontiguousarray(proj)).to(dev)
    if xyz:
        full = np.random.default_rng(1).uniform(-3, 3, y.shape + (3,)).astype(np.float32)
        full[..., 1] = y
        dh = torch.from_numpy(full).to(dev)
        keep = full
    else:
        dh = torch.from_numpy(np.ascontiguousarray(y)).to(dev)
        keep = y
    got = ops.map_heights(dp, dh, record, band_mm=band, exclude_cell=exclude_cell)
    assert got is record
    assert np.array_equal(dp.cpu().numpy(), proj) and np.array_equal(dh.cpu().numpy(), keep, equal_nan=True)      # read-only
    return record


def test_hand_worked_record(dev):
    from embodied_object_detection_amd import ops
    proj, y, N, band, ex, want = OC.hand_record()
    rec = run_heights(dev, proj, y, ops.new_height_record(N, dev), band, ex)
    assert rec.cpu().numpy().T.tolist() == [list(w) for w in want]
    assert np.array_equal(rec.cpu().numpy(), OC.heights_reference(proj, y, OC.new_record(N), band, ex))


@pytest.mark.parametrize("P", PIXELS)
def test_record_pixel_counts_and_cell_patterns(dev, P):
    from embodied_object_detection_amd import ops
    N = 300
    for n, (name, cells) in enumerate(cell_patterns(P, N).items()):
        y = some_heights(P, 10 * P + n)
        if name == "dropped in between":
            y[2::8] = (np.nan, np.inf, -np.inf, 1000.5, -1e30, 1000.0001)[n % 6]
            y[6::16] = np.nan
        for xyz in (False, True):
            rec = run_heights(dev, cells, y, ops.new_height_record(N, dev), xyz=xyz)
            ref = OC.heights_reference(cells, y, OC.new_record(N), BAND, 5)
            assert np.array_equal(rec.cpu().numpy(), ref), (P, name, xyz)
        assert ref[0].sum() > 0 or name == "dropped in between", (P, name)
        assert ref[0, 5] == 0


def test_record_more_cells_than_a_workgroup_gathers(dev):
    """A workgroup gathers its 1024 pixels per cell in a table of 512 entries before it commits them: a cell a pixel (1024 cells a
    workgroup: half of them find no entry and commit themselves), two pixels a cell (512: the table exactly full, probes run out),
    and a stride that makes the cells collide in the table, across one, two and three workgroups and a ragged last one."""
    from embodied_object_detection_amd import ops
    N = 6000
    for P in (1023, 1024, 1025, 2049, 4099):
        p = np.arange(P)
        for n, cells in enumerate((p % N, (p // 2) % N, (p * 512) % N, (p % 700) * 8)):
            y = some_heights(P, P + n)
            rec = run_heights(dev, cells.astype(np.int32), y, ops.new_height_record(N, dev), xyz=bool(n % 2))
            ref = OC.heights_reference(cells, y, OC.new_record(N), BAND, 5)
            assert np.array_equal(rec.cpu().numpy(), ref), (P, n)
        assert ref[0].sum() == P and (ref[0] > 0).sum() == min(P, 700)


def test_record_band_edges_and_ties(dev):
    """Every height within 3 mm of a band edge in steps of a quarter millimetre, as the nearest float32: rounding comes before the
    band test, ties go to even, both edges are inside."""
    from embodied_object_detection_amd import ops
    mm = np.concatenate([np.arange(e - 3, e + 3.25, 0.25) for e in (100, 1500, 0, -250)])
    y = (mm / 1000.0).astype(np.float32)
    for band in (BAND, (-250, 0), (100, 100), (0, 0), (-1000000, 1000000)):
        # every height a cell of its own, then all of them in one cell
        for cells, N in ((np.arange(y.size, dtype=np.int32), y.size), (np.zeros(y.size, np.int32), 2)):
            rec = run_heights(dev, cells, y, ops.new_height_record(N, dev), band, -1)
            ref = OC.heights_reference(cells, y, OC.new_record(N), band, -1)
            assert np.array_equal(rec.cpu().numpy(), ref), band
    q = OC.millimetres(y)
    assert (np.abs(mm * 2 - np.round(mm * 2)) < 1e-9).sum() > 40 and set(np.unique(q[np.abs(mm - 100) <= 0.5]).tolist()) == {100.0}
    ref = OC.heights_reference(np.arange(y.size), y, OC.new_record(y.size), BAND, -1)
    assert 0 < ref[1].sum() < y.size


def test_record_order_split_and_extension(dev):
    """The same pixels permuted, and split over two and three calls, give the same bits; a record that holds data is extended."""
    from embodied_object_detection_amd import ops
    N, P = 500, 4099
    rng = np.random.default_rng(8)
    cells = cell_patterns(P, N)["runs"]
    cells = np.where(rng.random(P) < 0.2, rng.integers(-2, N + 2, P), cells).astype(np.int32)
    y = some_heights(P, 9)
    whole = run_heights(dev, cells, y, ops.new_height_record(N, dev)).clone()
    assert np.array_equal(whole.cpu().numpy(), OC.heights_reference(cells, y, OC.new_record(N), BAND, 5))
    perm = rng.permutation(P)
    assert torch.equal(run_heights(dev, cells[perm], y[perm], ops.new_height_record(N, dev)), whole)
    for cuts in ((1000,), (64, 3001), (4098,)):
        rec = ops.new_height_record(N, dev)
        for a, b in zip((0,) + cuts, cuts + (P,)):
            run_heights(dev, cells[a:b], y[a:b], rec, xyz=bool(a))
        assert torch.equal(rec, whole), cuts
    # a second frame on top of the first
    cells2, y2 = cell_patterns(257, N)["a cell a pixel"], some_heights(257, 10) - np.float32(0.7)
    rec = run_heights(dev, cells2, y2, whole.clone(), (0, 900), 7)
    ref = OC.heights_reference(cells2, y2, OC.heights_reference(cells, y, OC.new_record(N), BAND, 5), (0, 900), 7)
    assert np.array_equal(rec.cpu().numpy(), ref) and not torch.equal(rec, whole)
    empty = ops.map_heights(torch.zeros((0,), dtype=torch.int32, device=dev), torch.zeros((0,), device=dev), rec)
    assert empty is rec and np.array_equal(rec.cpu().numpy(), ref)


def test_record_of_a_projected_frame(dev):
    """One 128 x 160 frame through the projector: the height column of its xyz read in place, against the same column copied out."""
    from embodied_object_detection_amd import ops
    H, W, map_w, map_h = 128, 160, 24, 24
    rng = np.random.default_rng(3)
    r, c = np.mgrid[0:H, 0:W]
    depth = (2.0 + 1.5 * np.sin(c / 23.0) + 0.3 * np.cos(r / 11.0) + 0.02 * rng.random((H, W))).astype(np.float32)
    depth[rng.random((H, W)) < 0.03] = 0.0                                   # holes: they land in the camera's own cell
    T = np.eye(4, dtype=np.float32)
    T[1, 3] = 0.65
    intr = (120.0, 120.0, W / 2.0, H / 2.0)
    idx, xyz = ops.unproject_grid_index(torch.from_numpy(depth).to(dev), T, intr, (0.0, 0.0, 0.0), (-6.0, 0.0, -6.0), 0.5, map_w, map_h,
                                        0, want_xyz=True)
    assert idx.shape == (H, W) and xyz.shape == (H, W, 3)
    proj, y = idx.cpu().numpy(), xyz.cpu().numpy()[:, :, 1].copy()
    own = int(np.bincount(proj[depth == 0.0].reshape(-1)).argmax())
    N = map_w * map_h
    band = (-200, 400)
    ref = OC.heights_reference(proj, y, OC.new_record(N), band, own)
    a = ops.map_heights(idx, xyz, ops.new_height_record(N, dev), band_mm=band, exclude_cell=own)
    b = ops.map_heights(idx, torch.from_numpy(y).to(dev), ops.new_height_record(N, dev), band_mm=band, exclude_cell=own)
    assert np.array_equal(a.cpu().numpy(), ref) and torch.equal(a, b)
    assert (ref[0] > 0).sum() >= 8 and 0 < ref[1].sum() < ref[0].sum() and ref[0, own] == 0
    print(f"frame: {int((ref[0] > 0).sum())} cells hit, {int(ref[0].sum())} pixels, {int(ref[1].sum())} in the band")


# ---- the query ---------------------------------------------------------------------------------------------------------------------
def run(dev, record, cols, labels=None, objects=(), min_hits=4, min_cells=2, topk=16):
    from embodied_object_detection_amd import ops
    dr = torch.from_numpy(np.ascontiguousarray(record)).to(dev)
    dl = None if labels is None else torch.from_numpy(np.ascontiguousarray(labels)).to(dev)
    do = torch.from_numpy(np.asarray(objects, np.int32)).to(dev) if len(objects) else None
    out = ops.map_obstacles(dr, cols, object_labels=dl, objects=do, min_hits=min_hits, min_cells=min_cells, topk=topk)
    N, Ko = record.shape[1], len(objects)
    assert sorted(out) == sorted(OC.KEYS)
    assert out["kind"].shape == (N,) and out["kind"].dtype == torch.uint8
    for k in OC.CELL_KEYS[1:]:
        assert out[k].shape == (N,) and out[k].dtype == torch.int32 and out[k].is_contiguous(), k
    for k in OC.SLOT_KEYS:
        assert out[k].shape[0] == topk and out[k].dtype == (torch.int64 if k in OC.WIDE else torch.int32), k
    for k in OC.OBJ_KEYS:
        assert out[k].shape == (Ko,) and out[k].dtype == torch.int32, k
    assert out["bbox"].shape == (topk, 4) and out["sum_rc"].shape == (topk, 2) and out["count"].shape == (1,)
    assert out["counts"].shape == (6,) and out["status"].shape == (2,)
    assert np.array_equal(dr.cpu().numpy(), record) and (dl is None or np.array_equal(dl.cpu().numpy(), labels))   # read-only
    return out


def check(dev, tag, record, cols, labels=None, objects=(), **kw):
    got = OC.host(run(dev, record, cols, labels, objects, **kw))
    ref = OC.reference(record, cols, labels, objects, **kw)
    bad = OC.differences(got, ref)
    assert not bad, (tag, kw, bad, {k: (got[k], ref[k]) for k in bad[:2]})
    return ref


def test_hand_worked_map(dev):
    rec, cols, labels, min_hits, min_cells = OC.hand_map()
    ref = check(dev, "hand", rec, cols, labels, (13,), min_hits=min_hits, min_cells=min_cells, topk=4)
    assert ref["counts"].tolist() == [6, 12, 4, 2, 2, 1] and ref["count"].tolist() == [1] and ref["top_mm"][0] == 780
    assert (ref["obj_cells"][0], ref["obj_seen_cells"][0], ref["obj_top_mm"][0], ref["obj_base_mm"][0]) == (2, 1, 830, 23)
    ref = check(dev, "hand, min_cells 1", rec, cols, labels, (13,), min_hits=min_hits, min_cells=1, topk=4)
    assert ref["count"].tolist() == [2] and ref["merged_labels"][16] == 16 and ref["counts"][5] == 0
    ref = check(dev, "hand, no labels", rec, cols, None, (13,), min_hits=min_hits, min_cells=min_cells, topk=4)
    assert ref["counts"].tolist() == [7, 12, 5, 0, 2, 1] and ref["area"][0] == 4 and ref["obj_cells"].tolist() == [0]
    ref = check(dev, "hand, min_hits 1", rec, cols, labels, (), min_hits=1, min_cells=min_cells, topk=4)
    assert ref["counts"][2] == 5 and ref["area"][0] == 5                         # cell 9 joins {0, 1, 8} and the speck


GRIDS = {"33x33": (33, 33), "64x65": (64, 65), "31x97": (31, 97), "1x130": (1, 130), "130x1": (130, 1), "96x96": (96, 96),
         "40x40": (40, 40), "1x1": (1, 1)}


def slots_64(labels, N):
    """64 object slots for a label map: its labels, a duplicate of the first, a negative slot, labels no cell carries."""
    have = sorted(set(labels[labels >= 0].tolist()))
    objs = have[:20] + have[:1] + [-1] + [N + k for k in range(64)]
    return objs[:64]


@pytest.mark.parametrize("grid", list(GRIDS))
def test_own_maps(dev, grid):
    """Every map of `_obstacle_cases.maps` on the grid, the options taken in turn: min_hits 1 and 4, min_cells 1 and 3, K 1, 16 and
    64, no object slot, one, and 64 with a duplicate and a negative one, with and without object_labels."""
    rows, cols = GRIDS[grid]
    N = rows * cols
    n = 0
    for name, m in OC.maps(rows, cols).items():
        labels = m["labels"]
        if labels is None and n % 4 == 3:                                        # lowest-cell labels of a block of the map's own
            labels = np.full(N, -1, np.int32)
            labels[N // 3: N // 3 + max(1, cols // 2)] = N // 3
        if labels is None:
            objects = ((), (5,), (5, 5))[n % 3]                                  # slots without a label map: no cell is theirs
        else:
            objects = (m["objects"] or (N // 3,), slots_64(labels, N))[n % 2]
        for with_labels in ((True, False) if labels is not None else (False,)):
            ref = check(dev, f"{grid} {name}", m["record"], cols, labels if with_labels else None, objects,
                        min_hits=(4, 1)[n % 2], min_cells=(1, 3, 2)[n % 3], topk=(16, 64, 1)[n % 3])
        if name == "all unseen":
            assert ref["counts"].tolist() == [N, 0, 0, 0, 0, 0]
        if name == "all obstacle":
            assert ref["counts"][2] == N and ref["counts"][4] == 1 and ref["structure_labels"].max() == 0
        n += 1
    print(f"{grid}: {n} maps, all equal")


@pytest.mark.parametrize("grid", ["33x33", "64x65", "96x96"])
def test_every_option_on_the_hard_maps(dev, grid):
    rows, cols = GRIDS[grid]
    N = rows * cols
    maps = OC.maps(rows, cols)
    for name in ("spirals", "checkerboard", "many structures", "random 0.4", "objects over obstacles"):
        m = maps[name]
        for min_hits in (1, 4):
            for min_cells in (1, 3):
                for topk in (1, 16, 64):
                    ref = check(dev, f"{grid} {name}", m["record"], cols, m["labels"], m["objects"], min_hits=min_hits,
                                min_cells=min_cells, topk=topk)
        if name == "spirals":
            assert ref["counts"][4] == 2 and ref["count"][0] == 2 and ref["area"][1] > 2 * min(rows, cols)
        if name == "checkerboard":
            assert ref["counts"][4] == 1 and ref["area"][0] == (N + 1) // 2
        if name == "many structures" and grid != "33x33":
            assert ref["count"][0] > 64 and (ref["structure"] >= 0).all() and ref["area"][0] == ref["area"][63] == 3
        if name == "objects over obstacles":
            m2 = slots_64(m["labels"], N)
            ref = check(dev, f"{grid} {name}, 64 slots", m["record"], cols, m["labels"], m2, min_hits=4, min_cells=2, topk=16)
            dup = m2.index(m2[0], 1)
            assert ref["obj_cells"][0] > 0 and ref["obj_cells"][dup] == 0 and ref["obj_cells"][21] == 0      # duplicate, negative
            assert (ref["obj_seen_cells"] < ref["obj_cells"]).any() and (ref["obj_top_mm"][ref["obj_seen_cells"] == 0] == INT_MIN).all()
            assert ((ref["kind"] == OC.OBJECT) & (m["record"][1] >= 4)).any()                                   # objects over obstacles


def raw(dev, record, cols, labels, objects, fill, min_hits=4, min_cells=2, topk=16):
    """The entry point on buffers of this test's own, outputs and workspace filled with `fill` bytes before the call."""
    from embodied_object_detection_amd import _lib, ops
    from embodied_object_detection_amd.ops import _stream
    N, K, Ko = record.shape[1], topk, len(objects)
    dr = torch.from_numpy(record).to(dev)
    dl = None if labels is None else torch.from_numpy(labels).to(dev)
    do = torch.tensor(list(objects), dtype=torch.int32, device=dev)
    shapes = dict(kind=(N,), structure_labels=(N,), merged_labels=(N,), count=(1,), structure=(K,), area=(K,), bbox=(K, 4), sum_rc=(K, 2),
                  top_mm=(K,), obj_cells=(Ko,), obj_seen_cells=(Ko,), obj_top_mm=(Ko,), obj_base_mm=(Ko,), counts=(6,), status=(2,))
    out = {}
    for k, shape in shapes.items():
        size = 1 if k == "kind" else 8 if k in OC.WIDE else 4
        t = torch.full((int(np.prod(shape)) * size + 8,), fill, dtype=torch.uint8, device=dev)[:-8]
        out[k] = t.view({1: torch.uint8, 4: torch.int32, 8: torch.int64}[size]).view(shape)
    words = ops.map_obstacles_workspace(N, cols)
    ws = torch.full((words * 4,), fill, dtype=torch.uint8, device=dev).view(torch.int32)
    _lib.check(_lib.load().eod_map_obstacles(dr[0].data_ptr(), dr[1].data_ptr(), dr[2].data_ptr(), dr[3].data_ptr(),
                                             None if dl is None else dl.data_ptr(), do.data_ptr(), N, cols, Ko, min_hits, min_cells, K,
                                             *[out[k].data_ptr() for k in shapes], ws.data_ptr(), words * 4, _stream()),
               "eod_map_obstacles")
    return out


def test_dirty_buffers_and_repeated_calls(dev):
    rows, cols = 64, 65
    maps = OC.maps(rows, cols)
    for name in ("objects over obstacles", "random 0.4", "all obstacle", "all unseen", "many structures"):
        m = maps[name]
        objects = m["objects"] or (7, 7, -1)
        ref = OC.reference(m["record"], cols, m["labels"], objects, 4, 2, 16)
        for fill in (0xFF, 0x00, 0x5A):
            got = OC.host(raw(dev, m["record"], cols, m["labels"], objects, fill))
            assert not OC.differences(got, ref), (name, fill, OC.differences(got, ref))
        a, b = (OC.host(run(dev, m["record"], cols, m["labels"], objects)) for _ in range(2))
        assert not OC.differences(a, b) and not OC.differences(a, ref), name


# ---- the composition ---------------------------------------------------------------------------------------------------------------
MAP = (24, 24)
WALL_COL, TABLE = 12, 4 * 24 + 18                                        # the wall's column; the object's label: its lowest cell


def _wall_pixels(door=True, seed=0):
    """The pixels of frames that look at a flat with a wall down column 12 (a door at rows 11 and 12) and a table behind it: (proj
    [P], heights [P]).  The floor brings heights round 0, the wall heights up to 2.4 m, the table top 0.75 m."""
    rng = np.random.default_rng(seed)
    proj, y = [], []
    for cell in range(MAP[0] * MAP[1]):
        r, c = divmod(cell, MAP[1])
        if r in (0, 23) and c > 20:
            continue                                                             # a corner the camera never saw
        n = int(rng.integers(6, 30))
        wall = c == WALL_COL and not (door and r in (11, 12))
        h = np.append(rng.uniform(0.2, 1.4, n - 1), 2.3) if wall else rng.uniform(-0.02, 0.03, n)      # five band hits or more
        if cell in (TABLE, TABLE + 1):
            h = rng.uniform(0.70, 0.75, n)
        proj += [cell] * n
        y += h.tolist()
    pad = -len(proj) % 16                                                        # dropped pixels: two frames of 8 columns
    proj, y = proj + [-1] * pad, y + [0.0] * pad
    perm = rng.permutation(len(proj))
    return np.asarray(proj, np.int32)[perm], np.asarray(y, np.float32)[perm]


def _table_labels():
    labels = np.full(MAP[0] * MAP[1], -1, np.int32)
    labels[[TABLE, TABLE + 1]] = TABLE
    return labels


HERE = 3 * 24 + 2                                                          # the robot: left of the wall, far from the door


def test_route_goes_through_the_door_of_a_wall_made_of_heights(dev):
    from embodied_object_detection_amd import ops
    N, cols = MAP[0] * MAP[1], MAP[1]
    labels = _table_labels()
    dl, objs = torch.from_numpy(labels).to(dev), torch.tensor([TABLE], dtype=torch.int32, device=dev)
    cost = {}
    for door in (True, False):
        proj, y = _wall_pixels(door)
        rec = ops.map_heights(torch.from_numpy(proj).to(dev), torch.from_numpy(y).to(dev), ops.new_height_record(N, dev))
        assert np.array_equal(rec.cpu().numpy(), OC.heights_reference(proj, y, OC.new_record(N)))
        obs = ops.map_obstacles(rec, cols, object_labels=dl, objects=objs)
        ref = OC.reference(rec.cpu().numpy(), cols, labels, (TABLE,))
        assert not OC.differences(OC.host(obs), ref)
        assert ref["count"][0] == (2 if door else 1) and ref["counts"][3] == 2 and ref["obj_top_mm"][0] in range(700, 751)
        assert ref["top_mm"][0] > 1500 and ref["counts"][0] == 6
        merged = obs["merged_labels"]
        rt = ops.map_route(merged, objs, cols, HERE, path_max=64)
        want = RC.reference(merged.cpu().numpy(), np.array([TABLE], np.int32), cols, HERE, path_max=64)
        assert not RC.differences(RC.host(rt), want), RC.differences(RC.host(rt), want)
        cost[door] = int(rt["goal_cost"][0])
        if door:
            path = rt["path"][0][: int(rt["path_cells"][0])].cpu().numpy()
            assert {int(p) for p in path if p % cols == WALL_COL} <= {11 * cols + WALL_COL, 12 * cols + WALL_COL}     # through the door
            assert any(p % cols == WALL_COL for p in path)
    plain = int(ops.map_route(dl, objs, cols, HERE, path_max=64)["goal_cost"][0])
    assert plain < cost[True] < INT_MAX and cost[False] == INT_MAX, (plain, cost)
    print(f"goal_cost: {plain} on object_labels alone, {cost[True]} round the wall, door shut {cost[False]}")


def _cfg():
    from embodied_object_detection_amd import setup_cfg
    return setup_cfg(None, ["MODEL.MEMORY_TYPE", "implicit_memory", "MODEL.MAP_FEAT_FUSION", "sum", "MODEL.MAP_FEATURE_WEIGHT", 5,
                            "MODEL.MEMORY_CLS_SCORE_THRESH", 0.3])


def _frames(n, seed=0, H=128, W=160):
    from embodied_object_detection_amd.data.synthetic import SyntheticSequence
    seq = SyntheticSequence(seed, H=H, W=W, n_frames=n, map_w=24, map_h=24, cell=0.5)
    return [seq.frame(i) for i in range(n)]


def _halves(proj, y):
    """The pixels as two frames of [h, 8] pixels each."""
    P = proj.size // 16 * 16
    return [(proj[a:b].reshape(-1, 8), y[a:b].reshape(-1, 8)) for a, b in ((0, P // 2), (P // 2, P))]


def test_model_heights_and_obstacles_change_nothing(dev, synthetic_sd):
    from embodied_object_detection_amd import _lib, build_model
    model = build_model(_cfg(), synthetic_sd)
    frames = _frames(2)
    N, cols = MAP[0] * MAP[1], MAP[1]
    proj, y = _wall_pixels()
    with pytest.raises(_lib.EodError, match="no memory yet"):
        model.heights(proj, y)
    model([[frames[0]]])
    with pytest.raises(_lib.EodError, match="no height record"):
        model.obstacles(map_shape=MAP)
    before = dict(mem=model.implicit_memory.clone(), obs=model.observations.clone())
    want = OC.new_record(N)
    for n, (p, h) in enumerate(_halves(proj, y)):
        xyz = np.zeros(h.shape + (3,), np.float32)
        xyz[..., 1] = h
        rec = model.heights(p[..., None] if n else p, xyz if n else h, exclude_cell=3)       # numpy, [H, W, 1] and xyz included
        want = OC.heights_reference(p, h, want, BAND, 3)
    assert rec is model._height_record and np.array_equal(rec.cpu().numpy(), want)
    labels = torch.from_numpy(_table_labels()).to(dev)
    obs = model.obstacles(labels, [TABLE], MAP)
    assert not OC.differences(OC.host(obs), OC.reference(want, cols, _table_labels(), (TABLE,)))
    rt = model.route([TABLE], obs["merged_labels"], MAP, from_cell=HERE, path_max=64)
    ref = RC.reference(obs["merged_labels"].cpu().numpy(), np.array([TABLE], np.int32), cols, HERE, path_max=64)
    assert not RC.differences(RC.host(rt), ref)
    assert int(rt["goal_cost"][0]) > int(model.route([TABLE], labels, MAP, from_cell=HERE, path_max=64)["goal_cost"][0])
    other = torch.from_numpy(OC.maps(*MAP)["random 0.4"]["record"]).to(dev)
    assert not OC.differences(OC.host(model.obstacles(map_shape=MAP, record=other, min_hits=1, min_cells=3, topk=64)),
                              OC.reference(other.cpu().numpy(), cols, None, (), 1, 3, 64))
    with pytest.raises(_lib.EodError, match="map_shape"):
        model.obstacles(labels)
    with pytest.raises(_lib.EodError, match="topk"):
        model.obstacles(labels, None, MAP, topk=65)
    assert torch.equal(model.implicit_memory, before["mem"]) and torch.equal(model.observations, before["obs"])
    assert np.array_equal(model._height_record.cpu().numpy(), want)
    # the next frame after the queries against a run that never asked
    fresh = build_model(_cfg(), synthetic_sd)
    fresh([[frames[0]]])
    a, b = (m([[frames[1]]])[0]["instances"] for m in (fresh, model))
    assert torch.equal(a.pred_boxes.tensor, b.pred_boxes.tensor) and torch.equal(a.scores, b.scores)
    assert torch.equal(fresh.implicit_memory, model.implicit_memory)
    model.reset_memory(N)
    assert model._height_record is None
    assert 0 < int(model.heights(proj[:64], y[:64])[0].sum()) <= 64


def test_predictor_heights_and_obstacles(dev, synthetic_sd):
    from embodied_object_detection_amd import _lib
    from embodied_object_detection_amd.engine.predictor import EmbodiedPredictor
    pred = EmbodiedPredictor(_cfg(), synthetic_sd)
    pred.model([[_frames(1)[0]]])
    proj, y = _wall_pixels()
    want = OC.new_record(MAP[0] * MAP[1])
    for p, h in _halves(proj, y):
        rec = pred.heights({"proj_indices": p, "heights": h}, band_mm=(50, 2000))
        want = OC.heights_reference(p, h, want, (50, 2000))
    assert np.array_equal(rec.cpu().numpy(), want)
    with pytest.raises(_lib.EodError, match="heights"):
        pred.heights({"proj_indices": proj})
    labels = torch.from_numpy(_table_labels()).to(dev)
    obs = pred.obstacles(labels, [TABLE], map_shape=MAP, min_cells=1)
    assert not OC.differences(OC.host(obs), OC.reference(want, MAP[1], _table_labels(), (TABLE,), min_cells=1))


def test_lockstep_heights_and_obstacles(dev, synthetic_sd):
    from embodied_object_detection_amd import _lib
    from embodied_object_detection_amd.modeling.lockstep import LockstepScenes
    ls = LockstepScenes(_cfg(), 2, synthetic_sd)
    ls([_frames(1, 0), _frames(1, 1)])
    N, cols = MAP[0] * MAP[1], MAP[1]
    want = np.stack([OC.new_record(N), OC.new_record(N)])
    for b, door in ((0, True), (1, False)):                                  # two scenes that hold different records
        for p, h in _halves(*_wall_pixels(door, seed=b)):
            row = ls.heights(b, p, h)
            want[b] = OC.heights_reference(p, h, want[b])
        assert np.array_equal(row.cpu().numpy(), want[b])
    assert ls._height_record.shape == (2, 4, N) and not np.array_equal(want[0], want[1])
    labels = torch.from_numpy(np.stack([_table_labels(), _table_labels()])).to(dev)
    objs = torch.tensor([[TABLE], [TABLE]], dtype=torch.int32, device=dev)
    obs = ls.obstacles(labels, objs, MAP)
    assert obs["merged_labels"].shape == (2, N) and obs["sum_rc"].shape == (2, 16, 2) and obs["counts"].shape == (2, 6)
    for b in (0, 1):
        ref = OC.reference(want[b], cols, _table_labels(), (TABLE,))
        assert not OC.differences(OC.host({k: v[b] for k, v in obs.items()}), ref)
        single = ls.obstacles(labels[b].contiguous(), [TABLE], MAP, scene=b)
        assert not OC.differences(OC.host(single), ref)
    rt = ls.route(objs, obs["merged_labels"], MAP, from_cell=HERE, path_max=64)
    assert int(rt["goal_cost"][0, 0]) < INT_MAX and int(rt["goal_cost"][1, 0]) == INT_MAX       # the door of scene 1 is shut
    bare = ls.obstacles(map_shape=MAP)
    assert bare["kind"].shape == (2, N) and (bare["kind"] != OC.OBJECT).all()
    with pytest.raises(_lib.EodError, match="scene="):
        ls.obstacles(labels[0].contiguous(), None, MAP)
    ls.reset_memory(1)
    assert np.array_equal(ls._height_record[1].cpu().numpy(), OC.new_record(N)) and np.array_equal(ls._height_record[0].cpu().numpy(), want[0])
