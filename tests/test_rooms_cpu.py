"""The rooms on the map without a GPU: the numpy reference of `_rooms_cases.py` on the hand-worked map of include/eod_rooms.h and
its three variants, every figure by hand; its symmetries; the header against the ctypes table and the cross-compiled library; every
argument the entry point, the op and the model surfaces refuse before any launch."""
import numpy as np
import pytest

import _rooms_cases as RC

INT_MAX = RC.INT_MAX


def test_reference_hand_worked_map():
    labels, cols = RC.hand_map()
    assert (labels.size, cols) == (77, 11) and (labels >= 0).sum() == 36 and labels[38] == -1
    d2 = RC.brute_d2(labels, cols)
    assert d2.reshape(7, 11)[1:6, 1:10].tolist() == [[1, 1, 1, 1, 0, 1, 1, 1, 1], [1, 4, 4, 1, 0, 1, 4, 4, 1], [1, 4, 5, 2, 1, 2, 5, 4, 1],
                                                     [1, 4, 4, 1, 0, 1, 4, 4, 1], [1, 1, 1, 1, 0, 1, 1, 1, 1]]
    r = RC.reference(labels, cols, 1, 1, topk=2, objects=(0,))
    left, right = [24, 25, 35, 36, 37, 46, 47], [29, 30, 39, 40, 41, 51, 52]
    assert np.flatnonzero(r["grow_dist"] == 0).tolist() == sorted(left + right) and d2[37] == d2[39] == 2 and d2[38] == 1
    assert r["count"].tolist() == [2] and r["room"].tolist() == [24, 29] and r["status"].tolist() == [0, 0]
    rim = (labels < 0) & (r["grow_dist"] != 0)
    assert set(r["grow_dist"][rim].tolist()) == {5, 7} and r["grow_dist"][38] == 5 and r["room_labels"][38] == 24
    assert (r["grow_dist"][labels >= 0] == INT_MAX).all() and (r["room_labels"][labels >= 0] == -1).all()
    want = np.full((7, 11), -1)
    want[1:6, 1:5], want[1:6, 6:10], want[3, 5] = 24, 29, 24
    assert r["room_labels"].tolist() == want.reshape(-1).tolist()
    assert r["area"].tolist() == [21, 20] and r["core_area"].tolist() == [7, 7]
    assert r["bbox"].tolist() == [[1, 1, 5, 5], [1, 6, 5, 9]] and r["sum_rc"].tolist() == [[63, 55], [60, 150]]
    assert r["widest_d2"].tolist() == [5, 5] and r["widest_cell"].tolist() == [36, 40]
    assert r["widest_key"].tolist() == [(5 << 32) | (~36 & 0xFFFFFFFF), (5 << 32) | (~40 & 0xFFFFFFFF)]
    assert r["door_edges"].tolist() == [[0, 1], [1, 0]] and r["door_cell"].tolist() == [[-1, 38], [39, -1]]
    assert r["door_d2"].tolist() == [[0, 1], [2, 0]] and r["door_key"][0, 1] == (1 << 32) | (~38 & 0xFFFFFFFF) and r["door_key"][0, 0] == 0
    assert r["obj_room_cells"].tolist() == [[15, 14]] and r["obj_room"].tolist() == [0] and r["obj_room_label"].tolist() == [24]
    assert r["room_objects"].tolist() == [1, 0] and r["counts"].tolist() == [36, 0, 41, 14, 27, 0]
    assert r["sum_rc"].dtype == r["widest_key"].dtype == r["door_key"].dtype == np.uint64 and r["room_labels"].dtype == np.int32
    # padding slots: the values eod_map_obstacles pads with
    r = RC.reference(labels, cols, 1, 1, topk=4, objects=())
    assert r["room"].tolist() == [24, 29, -1, -1] and r["area"][2:].tolist() == [0, 0] and r["bbox"][2:].tolist() == [[0] * 4] * 2
    assert r["widest_cell"][2:].tolist() == [-1, -1] and r["door_cell"][2:].min() == r["door_cell"][2:].max() == -1
    assert r["obj_room_cells"].shape == (0, 4) and r["obj_room"].shape == (0,)
    # topk 1: room 29 keeps its label on the map and is absent from the tables
    r = RC.reference(labels, cols, 1, 1, topk=1, objects=(0,))
    assert r["count"].tolist() == [2] and r["room"].tolist() == [24] and (r["room_labels"] == 29).sum() == 20
    assert r["door_edges"].tolist() == [[0]] and r["obj_room_cells"].tolist() == [[15]]


def test_reference_hand_worked_variants():
    labels, cols = RC.hand_map()
    r = RC.reference(labels, cols, 2, 1, topk=2, objects=(0,))
    assert r["core_area"].tolist() == [6, 6] and r["room"].tolist() == [24, 29] and r["area"].tolist() == [21, 20]
    assert r["grow_dist"][[37, 38, 39]].tolist() == [5, 10, 5] and r["room_labels"][38] == 24 and r["counts"].tolist() == [36, 0, 41, 12, 29, 0]
    r = RC.reference(labels, cols, 0, 1, topk=2, objects=(0,))
    assert r["count"].tolist() == [1] and r["room"].tolist() == [12, -1] and r["area"].tolist() == [41, 0]
    assert not r["door_edges"].any() and (r["door_cell"] == -1).all() and r["counts"].tolist() == [36, 0, 41, 41, 0, 0]
    r = RC.reference(labels, cols, 1, 8, topk=2, objects=(0,))
    assert r["count"].tolist() == [0] and (r["room_labels"] == -1).all() and r["counts"].tolist() == [36, 0, 41, 0, 0, 41]
    assert (r["grow_dist"] == INT_MAX).all() and r["room"].tolist() == [-1, -1] and r["obj_room"].tolist() == [-1]
    # a known mask that voids the door: two rooms without a doorway; one that cuts room 24 in two
    known = np.ones(77, np.uint8)
    known[38] = 0
    r = RC.reference(labels, cols, 1, 1, topk=2, known=known)
    assert r["counts"].tolist() == [36, 1, 40, 14, 26, 0] and not r["door_edges"].any() and r["room_labels"][38] == -1
    known = np.ones((7, 11), np.uint8)
    known[3, :5] = 0                                                       # blocked cells stay blocked whatever known says
    r = RC.reference(labels, cols, 1, 1, topk=3, known=known.reshape(-1))
    assert r["counts"][:3].tolist() == [36, 4, 37] and r["count"].tolist() == [3] and sorted(r["room"].tolist()) == [24, 29, 46]
    # passable: the wall's label blocks nothing, so d2 is INT_MAX everywhere and the whole map is one room
    r = RC.reference(labels, cols, 1, 1, topk=2, passable=(0,))
    assert r["counts"].tolist() == [0, 0, 77, 77, 0, 0] and r["room"].tolist() == [0, -1] and r["widest_d2"].tolist() == [INT_MAX, 0]
    assert r["widest_cell"].tolist() == [0, -1]


def _shape_of(r):
    """What moves neither with the labels nor with the tie rule: the counts and, sorted, the rooms' cores and widest places."""
    K = int((r["room"] >= 0).sum())
    return r["counts"].tolist(), r["count"].tolist(), sorted(r["core_area"][:K].tolist()), sorted(r["widest_d2"][:K].tolist())


def test_reference_transpose_and_mirror_identities():
    """Transposing or mirroring the map does the same to the rooms, up to their labels.  A cell that two rooms reach at the same cost
    goes to the lower label, which an image of the map changes: those cells (where the lowest and the highest label differ) are
    left out of the comparison of the partitions, and the areas with them."""
    maps = {"hand": RC.hand_map(), "flat": (RC.flat(21, 30, 2, 3, seed=1), 30), "closet": (RC.closet(), 24), "diagonal": (RC.diagonal_gap(), 16)}
    for name, (labels, cols) in maps.items():
        rows = labels.size // cols
        grid = labels.reshape(rows, cols)
        for door_r2 in (0, 1, 2):
            base = RC.reference(labels, cols, door_r2, 2, topk=16, objects=(0,))
            high = RC.reference(labels, cols, door_r2, 2, topk=16, objects=(0,), tie_high=True)
            assert (base["door_edges"] == base["door_edges"].T).all() and np.array_equal(base["grow_dist"], high["grow_dist"]), name
            sure = base["room_labels"] == high["room_labels"]
            assert sure[base["grow_dist"] == 0].all() and (name != "hand" or door_r2 == 0 or np.flatnonzero(~sure).tolist() == [38])
            for tag, fwd, back in (("transpose", lambda a: a.T, lambda a: a.T), ("mirror rows", lambda a: a[::-1], lambda a: a[::-1]),
                                   ("mirror cols", lambda a: a[:, ::-1], lambda a: a[:, ::-1])):
                g = np.ascontiguousarray(fwd(grid))
                r = RC.reference(g.reshape(-1), g.shape[1], door_r2, 2, topk=16, objects=(0,))
                assert _shape_of(r) == _shape_of(base), (name, door_r2, tag)
                assert np.array_equal(back(r["grow_dist"].reshape(g.shape)).reshape(-1), base["grow_dist"]), (name, door_r2, tag)
                there = back(r["room_labels"].reshape(g.shape)).reshape(-1)
                pairs = {(int(x), int(y)) for x, y in zip(there[sure], base["room_labels"][sure])}
                assert len({x for x, _ in pairs}) == len(pairs) == len({y for _, y in pairs}), (name, door_r2, tag)      # one to one


def test_maps_hold_the_cases_they_name():
    r = RC.reference(RC.closet(), 24, 1, 2, topk=4)
    assert r["count"][0] == 2 and r["counts"][5] == 9 and r["door_edges"][0, 1] > 0                 # the closet is unassigned
    r = RC.reference(RC.closet(), 24, 1, 1, topk=4)
    assert r["count"][0] == 3 and r["counts"][5] == 0 and r["area"][2] == 9 and r["core_area"][2] == 1
    r = RC.reference(RC.diagonal_gap(), 16, 1, 2, topk=4)
    assert r["count"][0] == 2 and not r["door_edges"].any() and r["counts"][5] == 0                 # the corner rule: no way through
    m = RC.corridor(70, 70)
    r = RC.reference(m, 70, 1, 2, topk=4)
    assert r["count"][0] == 1 and r["counts"][5] == 0 and r["grow_dist"][m < 0].max() > 5 * 70 * 20  # a long way through many tiles
    labels, objects = RC.objects_in_rooms(33, 65)
    assert len(objects) == 64 and objects[3] == objects[0] and objects[4] == -1 and 0 in objects and 5000 in objects
    r = RC.reference(labels, 65, 2, 4, topk=8, objects=objects)
    assert r["count"][0] == 6 and r["obj_room"][3] == -1 and r["obj_room"][4] == -1 and r["obj_room"][objects.index(5000)] == -1
    assert (r["obj_room_cells"][objects.index(0)] > 0).sum() == 6 and (r["obj_room"] >= 0).sum() > 10      # the wall is in every room
    r = RC.reference(RC.flat(65, 65, 9, 9, door=1, seed=2), 65, 1, 1, topk=4)
    assert r["count"][0] > 64 and (r["room"] >= 0).all() and (r["door_edges"] > 0).any() and len(set(r["room_labels"][r["room_labels"] >= 0].tolist())) == r["count"][0]


def test_rooms_header_and_ctypes_table_agree():
    import os
    import re
    import shutil
    import subprocess
    import tempfile
    import __graft_entry__
    __graft_entry__.build()
    from embodied_object_detection_amd import _lib, build, ops
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    path = os.path.join(root, "include", "eod_rooms.h")
    txt = open(path).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    declared = sorted(set(re.findall(r"^(?:int|size_t)\s+(eod_\w+)\s*\(", code, flags=re.M)))
    assert declared == sorted(_lib.ROOMS_SIGNATURES) == ["eod_map_rooms", "eod_map_rooms_workspace_bytes"]
    others = (set(_lib.SIGNATURES) | set(_lib.PLACE_SIGNATURES) | set(_lib.REGIONS_SIGNATURES) | set(_lib.INVENTORY_SIGNATURES)
              | set(_lib.DESCRIBE_SIGNATURES) | set(_lib.RELATIONS_SIGNATURES) | set(_lib.ROUTE_SIGNATURES) | set(_lib.CLEARANCE_SIGNATURES)
              | set(_lib.SIGHT_SIGNATURES) | set(_lib.FRONTIER_SIGNATURES) | set(_lib.OBSTACLES_SIGNATURES))
    assert not set(_lib.ROOMS_SIGNATURES) & others
    for name, n in (("eod_map_rooms", 37), ("eod_map_rooms_workspace_bytes", 2)):
        res, args = _lib.ROOMS_SIGNATURES[name]
        params = re.search(rf"\b{name}\s*\(([^)]*)\)", code, flags=re.S).group(1)
        assert len(params.split(",")) == len(args) == n, name
        for decl, arg in zip(params.split(","), args):                           # pointers, ints and the size in the header's order
            want = _lib.C.c_void_p if "*" in decl or "eod_stream_t" in decl else _lib.C.c_size_t if "size_t" in decl else _lib.C.c_int
            assert arg is want, (name, decl)
    lib = _lib.load()
    for name, (res, args) in _lib.ROOMS_SIGNATURES.items():
        fn = getattr(lib, name)                                                  # exported by the library built for gfx950
        assert fn.restype is res and list(fn.argtypes) == list(args), name
    val = lambda name: int(re.search(rf"#define {name} (\d+)", txt).group(1))
    assert (ops.ROOMS_K_MAX, ops.ROOMS_P_MAX, ops.ROOMS_TOPK_MAX, ops.ROOMS_N_MAX, ops.ROOMS_DIM_MAX, ops.ROOMS_SWEEPS_MAX) == (
        val("EOD_ROOMS_K_MAX"), val("EOD_ROOMS_P_MAX"), val("EOD_ROOMS_TOPK_MAX"), val("EOD_ROOMS_N_MAX"), val("EOD_ROOMS_DIM_MAX"),
        val("EOD_ROOMS_SWEEPS_MAX")) == (64, 64, 64, 2 ** 22, 32767, 1024)
    assert (ops.ROOMS_N_MAX, ops.ROOMS_DIM_MAX, ops.ROOMS_SWEEPS_MAX) == (ops.ROUTE_N_MAX, ops.ROUTE_DIM_MAX, ops.ROUTE_SWEEPS_MAX)
    assert (val("EOD_ROOMS_TILE_ROWS"), val("EOD_ROOMS_TILE_COLS")) == (ops.ROUTE_TILE_ROWS, ops.ROUTE_TILE_COLS) == (RC.TILE, RC.TILE)
    assert "rooms.hip" in build.SOURCES
    for said in ("{24, 25, 35, 36, 37, 46, 47} and {29, 30, 39, 40, 41, 51, 52}", "area 21, core_area 7, bbox 1 1 5 5, sum_rc 63 55",
                 "area 20, core_area 7, bbox 1 6 5 9, sum_rc 60 150", "door_cell[0,1] = 38 with door_d2 1", "door_cell[1,0] = 39 with door_d2 2",
                 "obj_room_cells[0] = [15, 14]", "counts = [36, 0, 41, 14, 27, 0]", "counts = [36, 0, 41, 0, 0, 41]",
                 "one room, label 12, area 41", "the door's grow_dist is 10", "1 4 5 2 1 2 5 4 1"):
        assert said in txt, said
    for rows, cols in ((1, 1), (200, 200), (70, 67), (32767, 128), (1, 32767)):
        N = rows * cols
        need = lib.eod_map_rooms_workspace_bytes(N, cols)
        tiles = -(-rows // 32) * -(-cols // 32)
        assert need >= 30 * N + 12 * tiles + 4 and need % 8 == 0 and need == 4 * ops.map_rooms_workspace(N, cols)
    for N, cols in ((0, 1), (10, 3), (2 ** 22 + 1, 1), (32768, 1), (32768, 32768), (-4, 2), (4, 0)):
        assert lib.eod_map_rooms_workspace_bytes(N, cols) == 0
    with pytest.raises(_lib.EodError, match="map_rooms_workspace"):
        ops.map_rooms_workspace(10, 3)
    cc = next((p for p in (shutil.which(n) for n in ("gcc", "cc", "clang")) if p), None)
    assert cc is not None, "no C compiler (gcc, cc, clang) on PATH: the header cannot be checked as C"
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "t.c")
        open(c, "w").write(f'#include "{path}"\nint main(void) {{ return EOD_ROOMS_TOPK_MAX == 64 && EOD_ROOMS_SWEEPS_MAX == 1024 ? 0 : 1; }}\n')
        subprocess.run([cc, "-std=c11", "-Wall", "-Werror", "-o", os.path.join(d, "t"), c], check=True)
        assert subprocess.run([os.path.join(d, "t")]).returncode == 0


def test_rooms_kernels_use_no_scratch():
    import __graft_entry__
    __graft_entry__.build()
    from embodied_object_detection_amd import build
    usage = build.resource_usage()
    if not any("rooms_" in k for k in usage):           # a library built elsewhere, without the remarks: build them here
        build.build(force=True, verbose=False)
        usage = build.resource_usage()
    mine = {k: v for k, v in usage.items() if "rooms_" in k}
    names = ("rooms_classify_kernel", "rooms_tile_kernel", "rooms_border_kernel", "rooms_seed_kernel", "rooms_sweep_kernel",
             "rooms_assign_kernel", "rooms_select_kernel", "rooms_stats_kernel", "rooms_finish_kernel")
    assert sorted(n for k in mine for n in names if n in k) == sorted(names), sorted(mine)
    assert not [k for k in build.scratch_offenders(usage) if k in mine]
    assert all(v.get("scratch", 0) == 0 for v in mine.values())


def test_entry_point_refuses_bad_arguments_before_any_launch():
    import ctypes as C
    import __graft_entry__
    __graft_entry__.build()
    from embodied_object_detection_amd import _lib
    lib = _lib.load()
    buf = (C.c_int64 * 4096)()
    p = C.addressof(buf)
    p += (-p) % 16
    BAD, ALIGN, NULL, CAPACITY = -1, -2, -4, -5
    ptrs = ("labels", "passable", "d2", "known", "objects", "room_labels", "grow_dist", "count", "room", "area", "core_area", "bbox",
            "sum_rc", "widest_key", "widest_d2", "widest_cell", "room_objects", "door_edges", "door_key", "door_d2", "door_cell",
            "obj_room_cells", "obj_room", "obj_room_label", "counts", "status", "workspace")
    wide = ("sum_rc", "widest_key", "door_key", "workspace")
    with_objects = ("objects", "obj_room_cells", "obj_room", "obj_room_label")

    def call(N=100, cols=10, P=2, K_obj=2, door_r2=1, min_cells=2, topk=4, sweeps=8, workspace_bytes=8192, **kw):
        a = {name: p for name in ptrs}
        a.update(kw)
        return lib.eod_map_rooms(*[a[n] for n in ptrs[:5]], N, P, cols, K_obj, door_r2, min_cells, topk, sweeps,
                                 *[a[n] for n in ptrs[5:]], workspace_bytes, None)

    for kw in (dict(N=0), dict(N=2 ** 22 + 1), dict(N=-5), dict(cols=0), dict(cols=-10), dict(cols=7), dict(cols=101),
               dict(N=32768, cols=32768), dict(N=32768, cols=1), dict(N=2 ** 22, cols=2 ** 22), dict(N=2 ** 22, cols=64), dict(P=-1),
               dict(P=65), dict(K_obj=-1), dict(K_obj=65), dict(door_r2=-1), dict(min_cells=0), dict(min_cells=-1), dict(topk=0),
               dict(topk=65), dict(topk=-1), dict(sweeps=0), dict(sweeps=1025), dict(sweeps=-1)):
        assert call(**kw) == BAD, kw
    none = {name: None for name in ptrs}
    assert call(topk=0, **none) == BAD                                           # a bad dimension wins over a null pointer
    assert call(door_r2=-1, sum_rc=p + 4) == BAD                                 # and over alignment
    assert call(sweeps=0, workspace_bytes=0) == BAD                              # and over the workspace
    for name in ptrs:
        if name == "known":
            continue
        assert call(**{name: None}) == NULL, name
        assert call(**{name: None, "sum_rc" if name != "sum_rc" else "workspace": p + 4}) == NULL, name       # null wins over alignment
        assert call(workspace_bytes=0, **{name: None}) == NULL, name                                          # and over the workspace
    assert call(known=None, workspace_bytes=0) == CAPACITY                       # known may be null
    assert call(P=0, passable=None, workspace_bytes=0) == CAPACITY               # passable too, without any
    assert call(K_obj=0, workspace_bytes=0, **{n: None for n in with_objects}) == CAPACITY      # and the object slots
    assert call(K_obj=0, P=0, workspace_bytes=0, known=None, passable=None, objects=None) == CAPACITY
    for name in ptrs:
        if name == "known":
            assert call(known=p + 1, workspace_bytes=0) == CAPACITY              # bytes: any address
            continue
        for off in ((4, 1) if name in wide else (2, 1)):
            assert call(**{name: p + off}) == ALIGN, (name, off)
            assert call(workspace_bytes=0, **{name: p + off}) == ALIGN, (name, off)     # alignment wins over the workspace
    need = lib.eod_map_rooms_workspace_bytes(100, 10)
    assert need == 2048 + 256 + 1024 + 2 * 256 + 256
    for short in (0, 8, need - 1):
        assert call(workspace_bytes=short) == CAPACITY, short
    assert call(P=64, K_obj=64, door_r2=2 ** 31 - 1, min_cells=2 ** 31 - 1, topk=64, sweeps=1024, workspace_bytes=need - 1) == CAPACITY
    assert call(P=0, K_obj=0, door_r2=0, min_cells=1, topk=1, sweeps=1, workspace_bytes=need - 1) == CAPACITY     # the edges pass


def test_op_refuses_on_the_host_naming_the_argument():
    import torch
    import __graft_entry__
    __graft_entry__.build()
    from embodied_object_detection_amd import _lib, ops
    i32 = lambda *shape, **kw: torch.zeros(shape, dtype=torch.int32, **kw)
    labels, d2 = i32(120), i32(120)
    for bad in (i32(12, 10), torch.zeros((120,), dtype=torch.int64), i32(240)[::2], None, np.zeros(120, np.int32), i32(0)):
        with pytest.raises(_lib.EodError, match="labels"):
            ops.map_rooms(bad, d2, 10, 1)
    with pytest.raises(_lib.EodError, match="labels: N 4194305"):
        ops.map_rooms(torch.empty((2 ** 22 + 1,), dtype=torch.int32, device="meta"), d2, 1, 1)
    for bad in (i32(119), torch.zeros((120,), dtype=torch.int64), i32(240)[::2], i32(120, device="meta"), None, [0] * 120):
        with pytest.raises(_lib.EodError, match="d2"):
            ops.map_rooms(labels, bad, 10, 1)
    for bad in (0, -10, 7, 121, 2.5, True, None):
        with pytest.raises(_lib.EodError, match="cols"):
            ops.map_rooms(labels, d2, bad, 1)
    with pytest.raises(_lib.EodError, match="cols"):
        ops.map_rooms(i32(32768), i32(32768), 1, 1)                              # 32768 rows
    for name, bads in (("door_r2", (-1, 1.5, None, 2 ** 31, True)), ("min_cells", (0, -1, 1.5, None, 2 ** 31)),
                       ("topk", (0, 65, -1, 2.0, None)), ("sweeps", (0, 1025, -1, 2.0, True))):
        for bad in bads:
            kw = dict(door_r2=1)
            kw[name] = bad
            with pytest.raises(_lib.EodError, match=name):
                ops.map_rooms(labels, d2, 10, **kw)
    for name in ("objects", "passable"):
        for bad in (i32(65), torch.zeros((3,), dtype=torch.int64), i32(2, 2), i32(4, device="meta"), 7, ["a"], list(range(65))):
            with pytest.raises(_lib.EodError, match=name):
                ops.map_rooms(labels, d2, 10, 1, **{name: bad})
    for bad in (torch.zeros((119,), dtype=torch.uint8), i32(120), torch.zeros((240,), dtype=torch.uint8)[::2],
                torch.zeros((120,), dtype=torch.uint8, device="meta"), np.zeros(120, np.uint8)):
        with pytest.raises(_lib.EodError, match="known"):
            ops.map_rooms(labels, d2, 10, 1, known=bad)
    for kw in (dict(), dict(objects=[3, 3, -1], passable=(5,), min_cells=9, topk=64, sweeps=1024, known=torch.ones((120,), dtype=torch.uint8)),
               dict(objects=torch.tensor([1], dtype=torch.int32), topk=1, sweeps=1)):
        with pytest.raises(_lib.EodError, match="map_rooms: labels on the host .no CPU fallback"):          # refused last
            ops.map_rooms(labels, d2, 10, 1, **kw)


def test_model_surfaces_refuse_before_any_launch_and_say_what_they_take():
    import inspect
    import torch
    import __graft_entry__
    __graft_entry__.build()
    from embodied_object_detection_amd import _lib
    from embodied_object_detection_amd.data.robot import RobotFrontEnd
    from embodied_object_detection_amd.engine.predictor import EmbodiedPredictor
    from embodied_object_detection_amd.modeling.lockstep import LockstepScenes
    from embodied_object_detection_amd.modeling.meta_arch import CustomRCNNRecurrent, _rooms
    labels = torch.zeros((120,), dtype=torch.int32)
    with pytest.raises(_lib.EodError, match="rooms: map_shape"):
        _rooms(labels, None, None, 1, 2)
    with pytest.raises(_lib.EodError, match="rooms: map_shape"):
        _rooms(labels, None, (11, 10), 1, 2)
    with pytest.raises(_lib.EodError, match="rooms: door_r2 and min_cells are required"):
        _rooms(labels, None, (12, 10), None, 2)
    with pytest.raises(_lib.EodError, match="rooms: door_r2 and min_cells are required"):
        _rooms(labels, None, (12, 10), 1, None)
    with pytest.raises(_lib.EodError, match="rooms: labels on the host .no CPU fallback"):
        _rooms(labels, [3], (12, 10), 1, 2)
    bare = CustomRCNNRecurrent.__new__(CustomRCNNRecurrent)
    with pytest.raises(_lib.EodError, match="rooms: labels on the host"):
        bare.rooms(labels, None, (12, 10), door_r2=1, min_cells=2)
    pred = EmbodiedPredictor.__new__(EmbodiedPredictor)
    pred.model = bare
    with pytest.raises(_lib.EodError, match="rooms: map_shape"):
        pred.rooms(labels, door_r2=1, min_cells=2)
    ls = LockstepScenes.__new__(LockstepScenes)
    both = torch.stack([labels, labels])
    with pytest.raises(_lib.EodError, match=r"objects .*expected \[B, K\]"):
        ls.rooms(both, [1, 2, 3], (12, 10), door_r2=1, min_cells=2)
    with pytest.raises(_lib.EodError, match=r"known .*expected \[B, N\]"):
        ls.rooms(both, None, (12, 10), door_r2=1, min_cells=2, known=torch.ones((120,), dtype=torch.uint8))
    with pytest.raises(_lib.EodError, match=r"clearance .*expected d2 \[B, N\]"):
        ls.rooms(both, None, (12, 10), door_r2=1, min_cells=2, clearance=labels)
    with pytest.raises(_lib.EodError, match="rooms: labels on the host"):
        ls.rooms(both, [[1], [2]], (12, 10), door_r2=1, min_cells=2)
    want = ["labels", "objects", "map_shape", "door_r2", "min_cells", "topk", "passable", "known", "clearance", "sweeps"]
    for cls in (CustomRCNNRecurrent, LockstepScenes, EmbodiedPredictor):
        sig = inspect.signature(cls.rooms)
        assert list(sig.parameters)[1:] == want and sig.parameters["topk"].default == 16 and sig.parameters["sweeps"].default is None
        assert "room_labels" in cls.rooms.__doc__ and "door_cell" in cls.rooms.__doc__
    doc = CustomRCNNRecurrent.rooms.__doc__
    assert 'model.describe(rooms["room"], rooms["room_labels"], classifier=' in doc and 'obs["merged_labels"]' in doc and "door_r2" in doc
    front = RobotFrontEnd.__new__(RobotFrontEnd)
    front.res = 0.05
    assert front.door_r2(1.0) == 100 and front.door_r2(0.9) == 81 and front.door_r2(0.0) == 0 and front.door_r2(0.25) == 6
    assert front.door_r2(1.0) == front.body_radius2(0.5)                          # half the width, as a body's radius
