"""The rooms on the map on the GPU: every output of eod_map_rooms, bit for bit, against the numpy reference of `_rooms_cases.py`: the
hand-worked map of include/eod_rooms.h and its variants, maps that cross the 32-cell tile borders both ways, one row and one
column, maps without a blocked or without a free cell, more rooms than slots, a corridor that needs many sweeps, an unassigned
closet, known masks, the corner rule, passable labels, 64 object slots, dirty buffers, and the chain heights -> obstacles ->
clearance -> rooms -> describe through the model, the predictor and the lock-step batch."""
import numpy as np
import pytest
import torch

import _obstacle_cases as OC
import _rooms_cases as RC

pytestmark = pytest.mark.gpu

INT_MAX = RC.INT_MAX


@pytest.fixture(scope="module")
def dev():
    import __graft_entry__
    __graft_entry__.build()
    return torch.device("cuda")


def run(dev, labels, cols, door_r2, min_cells=1, topk=16, objects=(), passable=(), known=None, sweeps=None, d2=None):
    from embodied_object_detection_amd import ops
    d2 = RC.brute_d2(labels, cols, passable) if d2 is None else d2
    return ops.map_rooms(torch.from_numpy(np.asarray(labels, np.int32)).to(dev), torch.from_numpy(d2).to(dev), cols, door_r2,
                         min_cells=min_cells, topk=topk, objects=list(objects) if len(objects) else None,
                         passable=list(passable) if len(passable) else None,
                         known=None if known is None else torch.from_numpy(known).to(dev), sweeps=sweeps)


def check(dev, tag, labels, cols, door_r2, **kw):
    ref = RC.reference(labels, cols, door_r2, **{k: v for k, v in kw.items() if k != "sweeps"})
    got = RC.host(run(dev, labels, cols, door_r2, **kw))
    bad = RC.differences(got, ref)
    assert not bad, (tag, bad, {k: (got[k].reshape(-1)[:12].tolist(), ref[k].reshape(-1)[:12].tolist()) for k in bad[:3]})
    return ref


def test_hand_worked_map_and_its_variants(dev):
    labels, cols = RC.hand_map()
    r = check(dev, "hand", labels, cols, 1, min_cells=1, topk=2, objects=(0,))
    assert r["room"].tolist() == [24, 29] and r["area"].tolist() == [21, 20] and r["door_cell"].tolist() == [[-1, 38], [39, -1]]
    assert r["obj_room_cells"].tolist() == [[15, 14]] and r["counts"].tolist() == [36, 0, 41, 14, 27, 0] and r["room_labels"][38] == 24
    r = check(dev, "door_r2 2", labels, cols, 2, min_cells=1, topk=2, objects=(0,))
    assert r["core_area"].tolist() == [6, 6] and r["grow_dist"][38] == 10 and r["area"].tolist() == [21, 20]
    r = check(dev, "door_r2 0", labels, cols, 0, min_cells=1, topk=2, objects=(0,))
    assert r["room"].tolist() == [12, -1] and r["area"].tolist() == [41, 0] and not r["door_edges"].any()
    r = check(dev, "min_cells 8", labels, cols, 1, min_cells=8, topk=2, objects=(0,))
    assert (r["room_labels"] == -1).all() and r["counts"].tolist() == [36, 0, 41, 0, 0, 41]
    check(dev, "topk 1", labels, cols, 1, topk=1, objects=(0,))
    check(dev, "topk 64, no objects", labels, cols, 1, topk=64)
    # d2 is the caller's: that of map_clearance is the one the reference computes by brute force
    from embodied_object_detection_amd import ops
    dl = torch.from_numpy(labels).to(dev)
    clr = ops.map_clearance(dl, torch.tensor([0], dtype=torch.int32, device=dev), cols)
    assert np.array_equal(clr["d2"].cpu().numpy(), RC.brute_d2(labels, cols))


@pytest.mark.parametrize("rows,cols", [(33, 65), (70, 70)])
def test_maps_across_the_tile_borders(dev, rows, cols):
    for seed, (nr, nc, door) in enumerate(((2, 3, 2), (1, 1, 2), (3, 2, 1), (4, 5, 3))):
        labels = RC.flat(rows, cols, nr, nc, door=door, seed=seed, label_per_wall=bool(seed & 1))
        for door_r2, min_cells in ((1, 1), (2, 4), (4, 2), (0, 1)):
            r = check(dev, (rows, cols, nr, nc, door_r2), labels, cols, door_r2, min_cells=min_cells, topk=16, objects=(0, int(labels.max())))
        assert r["count"][0] >= 1
        check(dev, ("transposed", nr, nc), np.ascontiguousarray(labels.reshape(rows, cols).T).reshape(-1), rows, 1, min_cells=2,
              topk=7, objects=(0,))
    labels = RC.flat(rows, cols, 2, 2, door=2, seed=5)
    r = check(dev, "a room border on a tile border", labels, cols, 1, min_cells=2)
    assert r["count"][0] == 4 and (r["door_edges"] > 0).sum() >= 6


def test_one_row_and_one_column(dev):
    for n in (1, 31, 32, 33, 130):
        line = np.full(n, -1, np.int32)
        line[::17] = 3
        for labels in (line, np.full(n, -1, np.int32)):
            for door_r2 in (0, 4):
                check(dev, ("row", n, door_r2), labels, n, door_r2, topk=8, objects=(3,))
                check(dev, ("column", n, door_r2), labels, 1, door_r2, topk=8, objects=(3,))


def test_no_blocked_cell_and_no_free_cell(dev):
    for rows, cols in ((7, 11), (40, 70)):
        free = np.full(rows * cols, -1, np.int32)
        r = check(dev, "all free", free, cols, 1, topk=3, objects=(5,))
        assert r["count"][0] == 1 and r["area"][0] == rows * cols and r["widest_d2"][0] == INT_MAX and r["widest_cell"][0] == 0
        r = check(dev, "all blocked", np.full(rows * cols, 9, np.int32), cols, 1, topk=3, objects=(9,))
        assert r["count"][0] == 0 and r["counts"].tolist() == [rows * cols, 0, 0, 0, 0, 0] and r["obj_room"].tolist() == [-1]
        r = check(dev, "all void", free, cols, 1, topk=3, known=np.zeros(rows * cols, np.uint8))
        assert r["counts"].tolist() == [0, rows * cols, 0, 0, 0, 0]
        r = check(dev, "all passable", np.full(rows * cols, 9, np.int32), cols, 1, topk=3, passable=(9,), objects=(9,))
        assert r["count"][0] == 1 and r["obj_room_cells"][0, 0] == rows * cols


def test_more_rooms_than_slots(dev):
    labels = RC.flat(65, 65, 9, 9, door=1, seed=2)
    r = check(dev, "cubicles", labels, 65, 1, min_cells=1, topk=4, objects=(0,))
    assert r["count"][0] > 64 and (r["room"] >= 0).all()
    seen = set(r["room_labels"][r["room_labels"] >= 0].tolist())
    assert len(seen) == r["count"][0] and set(r["room"].tolist()) < seen          # the others keep their labels on the map
    check(dev, "cubicles, 64 slots", labels, 65, 1, min_cells=1, topk=64, objects=(0,))
    check(dev, "cubicles, min_cells", labels, 65, 1, min_cells=17, topk=64)


def test_wound_corridor_needs_sweeps(dev):
    labels = RC.corridor(70, 70)
    r = check(dev, "corridor", labels, 70, 1, min_cells=2, topk=4, sweeps=512)
    assert r["count"][0] == 1 and r["counts"][5] == 0 and r["grow_dist"][labels < 0].max() > 5 * 70 * 20
    out = run(dev, labels, 70, 1, min_cells=2, topk=4, sweeps=1)
    assert int(out["status"][0]) & 1 == 1                                     # the sweeps ran out: nothing else is promised
    assert int(run(dev, labels, 70, 1, min_cells=2, topk=4, sweeps=512)["status"][0]) == 0
    t = np.ascontiguousarray(RC.corridor(40, 97).reshape(40, 97).T).reshape(-1)
    check(dev, "corridor, transposed", t, 40, 1, min_cells=2, topk=4, sweeps=512)


def test_closet_below_min_cells_is_unassigned(dev):
    r = check(dev, "closet", RC.closet(), 24, 1, min_cells=2, topk=4, objects=(0,))
    assert r["count"][0] == 2 and r["counts"][5] == 9
    r = check(dev, "closet as a room", RC.closet(), 24, 1, min_cells=1, topk=4, objects=(0,))
    assert r["count"][0] == 3 and r["counts"][5] == 0
    big = np.zeros((70, 70), np.int32)
    big[2:68, 2:68] = -1
    big[30:37, 30:37] = 0
    big[31:36, 31:36] = -1                                                    # a closet across a tile corner
    r = check(dev, "closet on a tile corner", big.reshape(-1), 70, 1, min_cells=10, topk=4)
    assert r["counts"][5] == 25


def test_known_masks(dev):
    labels = RC.flat(33, 65, 1, 2, door=2, seed=4)
    grid = labels.reshape(33, 65)
    door = np.flatnonzero((grid[:, 32] < 0))
    assert door.size == 2
    known = np.ones((33, 65), np.uint8)
    known[door, 32] = 0                                                       # the doorway was never seen
    r = check(dev, "void doorway", labels, 65, 1, min_cells=2, known=known.reshape(-1))
    assert r["count"][0] == 2 and not r["door_edges"].any() and r["counts"][1] == 2
    known = np.full((33, 65), 7, np.uint8)
    known[16] = 0                                                             # a stripe across both rooms, walls included
    r = check(dev, "a stripe cuts the rooms", labels, 65, 1, min_cells=2, known=known.reshape(-1), objects=(0,))
    assert r["count"][0] == 4 and r["counts"][0] == (labels >= 0).sum()
    rng = np.random.default_rng(0)
    check(dev, "random known", labels, 65, 1, min_cells=1, known=(rng.random(33 * 65) > 0.1).astype(np.uint8), topk=64)


def test_corner_rule_refuses_the_diagonal_gap(dev):
    r = check(dev, "diagonal gap", RC.diagonal_gap(), 16, 1, min_cells=2, topk=4, objects=(0,))
    assert r["count"][0] == 2 and not r["door_edges"].any()
    m = RC.diagonal_gap(40, 70).reshape(40, 70)
    check(dev, "diagonal gap, larger", m.reshape(-1), 70, 1, min_cells=2, topk=4)
    # a pocket of 2 x 2 cells without a core whose only link to the room is the diagonal step (2, 2) -> (3, 3) between the wall
    # ends (2, 3) and (3, 2): the corner rule leaves it unassigned
    for rows, cols, at in ((12, 12, 0), (70, 70, 30)):                        # in a corner, and across the corner of four tiles
        p = np.full((rows, cols), -1, np.int32)
        p[0], p[-1], p[:, 0], p[:, -1] = 0, 0, 0, 0
        p[at:at + 4, at:at + 4] = 0
        p[at + 1:at + 3, at + 1:at + 3] = -1
        p[at + 3, at + 3] = -1
        r = check(dev, ("pocket", at), p.reshape(-1), cols, 1, min_cells=1, topk=4)
        assert r["counts"][5] == 4 and r["count"][0] == 1 and r["room_labels"][(at + 3) * cols + at + 3] >= 0


def test_passable_labels(dev):
    labels, cols = RC.hand_map()
    labels = labels.copy()
    labels[[36, 38]] = 5                                                      # a rug in the door and in the middle of a room
    r = check(dev, "rug", labels, cols, 1, topk=2, passable=(5,), objects=(5, 0))
    assert r["count"][0] == 2 and r["door_edges"][0, 1] == 1
    r = check(dev, "rug blocks", labels, cols, 1, topk=2, objects=(5, 0))
    assert not r["door_edges"].any()
    flat = RC.flat(33, 65, 2, 2, door=2, seed=1, label_per_wall=True)
    walls = sorted(set(flat[flat >= 0].tolist()))
    check(dev, "64 passable", flat, 65, 1, min_cells=2, passable=walls[:64], objects=walls[60:70])


def test_64_object_slots(dev):
    labels, objects = RC.objects_in_rooms(33, 65)
    r = check(dev, "64 slots", labels, 65, 2, min_cells=4, topk=8, objects=objects)
    assert r["obj_room"][3] == -1 and r["obj_room"][4] == -1 and (r["obj_room"] >= 0).sum() > 10
    assert (r["obj_room_cells"][objects.index(0)] > 0).sum() == 6 and r["room_objects"].sum() == (r["obj_room"] >= 0).sum()
    check(dev, "64 slots, 2 rooms ranked", labels, 65, 2, min_cells=4, topk=2, objects=objects)
    labels, objects = RC.objects_in_rooms(70, 70, seed=3)
    check(dev, "64 slots, 70 x 70", labels, 70, 2, min_cells=4, topk=64, objects=objects)


def raw(dev, labels, cols, d2, objects, passable, known, fill, door_r2=1, min_cells=2, topk=16, sweeps=16):
    """The entry point on buffers of this test's own, outputs and workspace filled with `fill` bytes before the call."""
    from embodied_object_detection_amd import _lib, ops
    from embodied_object_detection_amd.ops import _stream
    N, K, Ko = labels.size, topk, len(objects)
    dl, dd = torch.from_numpy(labels).to(dev), torch.from_numpy(d2).to(dev)
    do = torch.tensor(list(objects), dtype=torch.int32, device=dev)
    dp = torch.tensor(list(passable), dtype=torch.int32, device=dev)
    dk = None if known is None else torch.from_numpy(known).to(dev)
    shapes = dict(room_labels=(N,), grow_dist=(N,), count=(1,), room=(K,), area=(K,), core_area=(K,), bbox=(K, 4), sum_rc=(K, 2),
                  widest_key=(K,), widest_d2=(K,), widest_cell=(K,), room_objects=(K,), door_edges=(K, K), door_key=(K, K),
                  door_d2=(K, K), door_cell=(K, K), obj_room_cells=(Ko, K), obj_room=(Ko,), obj_room_label=(Ko,), counts=(6,), status=(2,))
    out = {}
    for k, shape in shapes.items():
        size = 8 if k in RC.WIDE else 4
        t = torch.full((int(np.prod(shape)) * size + 8,), fill, dtype=torch.uint8, device=dev)[:-8]
        out[k] = t.view({4: torch.int32, 8: torch.int64}[size]).view(shape)
    words = ops.map_rooms_workspace(N, cols)
    ws = torch.full((words * 4,), fill, dtype=torch.uint8, device=dev).view(torch.int32)
    _lib.check(_lib.load().eod_map_rooms(dl.data_ptr(), dp.data_ptr() if len(passable) else None, dd.data_ptr(),
                                         None if dk is None else dk.data_ptr(), do.data_ptr() if Ko else None, N, len(passable), cols, Ko,
                                         door_r2, min_cells, K, sweeps, *[out[k].data_ptr() if out[k].numel() else None for k in shapes],
                                         ws.data_ptr(), words * 4, _stream()), "eod_map_rooms")
    return out


def test_dirty_buffers_and_repeated_calls(dev):
    labels, objects = RC.objects_in_rooms(33, 65)
    rng = np.random.default_rng(1)
    cases = {"objects": (labels, 65, objects, (), None), "void": (labels, 65, objects[:5], (0,), (rng.random(labels.size) > 0.05).astype(np.uint8)),
             "cubicles": (RC.flat(65, 65, 9, 9, door=1, seed=2), 65, (), (), None), "closet": (RC.closet(), 24, (0,), (), None)}
    for name, (lab, cols, objs, pas, known) in cases.items():
        d2 = RC.brute_d2(lab, cols, pas)
        ref = RC.reference(lab, cols, 1, 2, topk=16, objects=objs, passable=pas, known=known)
        for fill in (0xFF, 0x00, 0x5A):
            got = RC.host(raw(dev, lab, cols, d2, objs, pas, known, fill))
            assert not RC.differences(got, ref), (name, fill, RC.differences(got, ref))
        a, b = (RC.host(run(dev, lab, cols, 1, min_cells=2, objects=objs, passable=pas, known=known)) for _ in range(2))
        assert not RC.differences(a, b) and not RC.differences(a, ref), name


# ---- the composition ---------------------------------------------------------------------------------------------------------------
MAP = (24, 24)
WALL_COL, TABLE = 12, 4 * 24 + 18                                        # the wall's column; the object's label: its lowest cell
DOOR_R2, MIN_CELLS = 1, 4


def _wall_pixels(door=True, seed=0):
    """The pixels of frames that look at a flat with a wall down column 12 (a door at rows 11 and 12) and a table behind it: (proj
    [P], heights [P]).  The floor brings heights round 0, the wall heights up to 2.4 m, the table top 0.75 m.  Two corners were never
    seen."""
    rng = np.random.default_rng(seed)
    proj, y = [], []
    for cell in range(MAP[0] * MAP[1]):
        r, c = divmod(cell, MAP[1])
        if r in (0, 23) and c > 20:
            continue
        n = int(rng.integers(6, 30))
        wall = c == WALL_COL and not (door and r in (11, 12))
        h = np.append(rng.uniform(0.2, 1.4, n - 1), 2.3) if wall else rng.uniform(-0.02, 0.03, n)
        if cell in (TABLE, TABLE + 1):
            h = rng.uniform(0.70, 0.75, n)
        proj += [cell] * n
        y += h.tolist()
    pad = -len(proj) % 8
    proj, y = proj + [-1] * pad, y + [0.0] * pad
    perm = rng.permutation(len(proj))
    return np.asarray(proj, np.int32)[perm].reshape(-1, 8), np.asarray(y, np.float32)[perm].reshape(-1, 8)


def _table_labels():
    labels = np.full(MAP[0] * MAP[1], -1, np.int32)
    labels[[TABLE, TABLE + 1]] = TABLE
    return labels


def _cfg():
    from embodied_object_detection_amd import setup_cfg
    return setup_cfg(None, ["MODEL.MEMORY_TYPE", "implicit_memory", "MODEL.MAP_FEAT_FUSION", "sum", "MODEL.MAP_FEATURE_WEIGHT", 5,
                            "MODEL.MEMORY_CLS_SCORE_THRESH", 0.3])


def _frames(n, seed=0, H=128, W=160):
    from embodied_object_detection_amd.data.synthetic import SyntheticSequence
    seq = SyntheticSequence(seed, H=H, W=W, n_frames=n, map_w=24, map_h=24, cell=0.5)
    return [seq.frame(i) for i in range(n)]


def _chain_reference(door, seed=0):
    """What the chain must give: the reference of the obstacles, then the reference of the rooms on its merged labels and kinds."""
    proj, y = _wall_pixels(door, seed)
    rec = OC.heights_reference(proj, y, OC.new_record(MAP[0] * MAP[1]))
    obs = OC.reference(rec, MAP[1], _table_labels(), (TABLE,))
    return obs, RC.reference(obs["merged_labels"], MAP[1], DOOR_R2, MIN_CELLS, topk=16, objects=(TABLE,), known=obs["kind"])


def _check_chain(rooms, door, seed=0):
    obs, ref = _chain_reference(door, seed)
    got = RC.host(rooms)
    assert not RC.differences(got, ref), RC.differences(got, ref)
    assert np.array_equal(rooms["clearance_d2"].cpu().numpy(), RC.brute_d2(obs["merged_labels"], MAP[1]))
    return ref


def test_model_chain_to_the_rooms_changes_nothing(dev, synthetic_sd):
    from embodied_object_detection_amd import _lib, build_model, ops
    model = build_model(_cfg(), synthetic_sd)
    frames = _frames(2)
    model([[frames[0]]])
    before = dict(mem=model.implicit_memory.clone(), obs=model.observations.clone())
    model.heights(*_wall_pixels())
    labels = torch.from_numpy(_table_labels()).to(dev)
    obs = model.obstacles(labels, [TABLE], MAP)
    rooms = model.rooms(obs["merged_labels"], [TABLE], MAP, door_r2=DOOR_R2, min_cells=MIN_CELLS, known=obs["kind"])
    ref = _check_chain(rooms, True)
    assert ref["count"][0] == 2 and ref["counts"][1] == 6 and ref["door_edges"][0, 1] == 2          # two rooms, a door of two cells
    assert ref["obj_room"][0] >= 0 and ref["obj_room_label"][0] == ref["room_labels"][TABLE + 24]   # the table's room: the right one
    assert ref["door_cell"][0, 1] % 24 in (WALL_COL - 1, WALL_COL, WALL_COL + 1)
    # the same with the clearance handed in, as a dict and as its d2; and without objects
    clr = model.clearance([TABLE], obs["merged_labels"], MAP)
    for c in (clr, clr["d2"]):
        again = model.rooms(obs["merged_labels"], [TABLE], MAP, door_r2=DOOR_R2, min_cells=MIN_CELLS, known=obs["kind"], clearance=c)
        assert not RC.differences(RC.host(again), ref) and again["clearance_d2"] is clr["d2"]
    bare = model.rooms(obs["merged_labels"], None, MAP, door_r2=DOOR_R2, min_cells=MIN_CELLS, known=obs["kind"])
    assert bare["obj_room"].shape == (0,) and torch.equal(bare["room_labels"], rooms["room_labels"])
    # what kind of room: the memory pooled over a room's cells, classified like an object
    desc = model.describe(rooms["room"], rooms["room_labels"])
    pool = ops.describe_pool(model.implicit_memory, rooms["room_labels"], rooms["room"])
    assert desc["cells"][:2].tolist() == rooms["area"][:2].tolist() and desc["cells"][2:].sum() == 0
    assert torch.equal(desc["embedding"], pool["embedding"]) and desc["prob"].shape[0] == 16
    with pytest.raises(_lib.EodError, match="door_r2 and min_cells are required"):
        model.rooms(obs["merged_labels"], None, MAP)
    wound = torch.from_numpy(RC.corridor(70, 70)).to(dev)                     # the sweeps are doubled until the keys settle
    for sweeps in (None, 1):
        assert not RC.differences(RC.host(model.rooms(wound, None, (70, 70), door_r2=1, min_cells=2, sweeps=sweeps)),
                                  RC.reference(RC.corridor(70, 70), 70, 1, 2)), sweeps
    assert torch.equal(model.implicit_memory, before["mem"]) and torch.equal(model.observations, before["obs"])
    # the next frame after the queries against a run that never asked
    fresh = build_model(_cfg(), synthetic_sd)
    fresh([[frames[0]]])
    a, b = (m([[frames[1]]])[0]["instances"] for m in (fresh, model))
    assert torch.equal(a.pred_boxes.tensor, b.pred_boxes.tensor) and torch.equal(a.scores, b.scores)
    assert torch.equal(fresh.implicit_memory, model.implicit_memory)


def test_predictor_chain_to_the_rooms(dev, synthetic_sd):
    from embodied_object_detection_amd.engine.predictor import EmbodiedPredictor
    pred = EmbodiedPredictor(_cfg(), synthetic_sd)
    pred.model([[_frames(1)[0]]])
    proj, y = _wall_pixels()
    pred.heights({"proj_indices": proj, "heights": y})
    labels = torch.from_numpy(_table_labels()).to(dev)
    obs = pred.obstacles(labels, [TABLE], map_shape=MAP)
    rooms = pred.rooms(obs["merged_labels"], [TABLE], map_shape=MAP, door_r2=DOOR_R2, min_cells=MIN_CELLS, known=obs["kind"])
    _check_chain(rooms, True)
    desc = pred.describe(rooms["room"], rooms["room_labels"])
    assert desc["cells"][:2].tolist() == rooms["area"][:2].tolist()


def test_lockstep_chain_to_the_rooms(dev, synthetic_sd):
    from embodied_object_detection_amd.modeling.lockstep import LockstepScenes
    ls = LockstepScenes(_cfg(), 2, synthetic_sd)
    ls([_frames(1, 0), _frames(1, 1)])
    N = MAP[0] * MAP[1]
    for b, door in ((0, True), (1, False)):                                  # the door of scene 1 is shut
        ls.heights(b, *_wall_pixels(door, seed=b))
    labels = torch.from_numpy(np.stack([_table_labels(), _table_labels()])).to(dev)
    objs = torch.tensor([[TABLE], [TABLE]], dtype=torch.int32, device=dev)
    obs = ls.obstacles(labels, objs, MAP)
    rooms = ls.rooms(obs["merged_labels"], objs, MAP, door_r2=DOOR_R2, min_cells=MIN_CELLS, known=obs["kind"])
    assert rooms["room_labels"].shape == (2, N) and rooms["door_cell"].shape == (2, 16, 16) and rooms["sum_rc"].shape == (2, 16, 2)
    refs = [_check_chain({k: v[b] for k, v in rooms.items()}, door, seed=b) for b, door in ((0, True), (1, False))]
    assert refs[0]["door_edges"][0, 1] == 2 and not refs[1]["door_edges"].any() and refs[1]["count"][0] == 2
    clr = ls.clearance(objs, obs["merged_labels"], MAP)
    again = ls.rooms(obs["merged_labels"], objs, MAP, door_r2=DOOR_R2, min_cells=MIN_CELLS, known=obs["kind"], clearance=clr)
    assert all(torch.equal(again[k], rooms[k]) for k in RC.KEYS)
    single = ls.rooms(obs["merged_labels"][1].contiguous(), [TABLE], MAP, door_r2=DOOR_R2, min_cells=MIN_CELLS,
                      known=obs["kind"][1].contiguous())
    assert not RC.differences(RC.host(single), refs[1])
    desc = ls.describe(0, rooms["room"][0].contiguous(), rooms["room_labels"][0].contiguous())
    assert desc["cells"][:2].tolist() == rooms["area"][0, :2].tolist()
