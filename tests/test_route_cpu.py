"""The host side of `map_route` (no GPU): the reference of `_route_cases.py` on hand-worked maps, include/eod_route.h against its
ctypes table and the cross-compiled library, the build's records, and every refused argument (the entry point returns before a
launch, so it is callable here)."""
import numpy as np
import pytest

import _route_cases as RC

INT_MAX = RC.INT_MAX


def _ref(rows_of_labels, objects, from_cell, passable=(), path_max=8):
    g = np.array(rows_of_labels, np.int32)
    return RC.reference(g.reshape(-1), np.array(objects, np.int32), g.shape[1], from_cell, passable, path_max)


def test_reference_open_field_costs_parents_and_ties():
    ref = _ref([[-1] * 4] * 3, [9], 0)
    assert ref["dist"].tolist() == [0, 5, 10, 15, 5, 7, 12, 17, 10, 12, 14, 19]
    # (1, 2) costs 12 over (0, 1) + 7 and over (1, 1) + 5: the lowest cell is the parent; so for (2, 1) over (1, 0) and (1, 1)
    assert ref["parent"].tolist() == [-1, 0, 1, 2, 0, 0, 1, 2, 4, 4, 5, 6]
    assert ref["counts"].tolist() == [12, 12] and ref["cells"].tolist() == [0] and ref["goal_cell"].tolist() == [-1]
    assert ref["goal_key"][0] == RC.NONE and ref["goal_cost"].tolist() == [INT_MAX] and ref["path_cells"].tolist() == [0]
    assert (ref["path"] == -1).all() and ref["path"].shape == (1, 8) and ref["status"].tolist() == [0, 0]
    for rows, cols, fc in ((7, 9, 30), (1, 6, 2), (6, 1, 5), (1, 1, 0)):
        ref = RC.reference(np.full(rows * cols, -1, np.int32), np.array([3], np.int32), cols, fc)
        assert np.array_equal(ref["dist"], RC.open_field(rows, cols, fc))


def test_reference_no_squeezing_between_two_corners_and_no_row_wrap():
    ref = _ref([[-1, 1], [1, -1]], [1], 0)
    assert ref["dist"].tolist() == [0, INT_MAX, INT_MAX, INT_MAX] and ref["parent"].tolist() == [-1] * 4
    assert ref["counts"].tolist() == [2, 1] and ref["cells"].tolist() == [2]
    assert ref["goal_cell"].tolist() == [0] and ref["goal_cost"].tolist() == [0]          # the start touches the object
    assert ref["path"][0].tolist() == [0] + [-1] * 7 and ref["path_cells"].tolist() == [1]
    # cells 2 = (0, 2) and 3 = (1, 0) follow each other in memory and are two columns apart
    ref = _ref([[-1, 1, -1], [-1, 1, 1]], [4], 2)
    assert ref["dist"].tolist() == [INT_MAX, INT_MAX, 0, INT_MAX, INT_MAX, INT_MAX] and ref["counts"].tolist() == [3, 1]


def test_reference_detour_goal_and_paths():
    rows = [[-1, -1, -1], [1, 1, -1], [5, -1, -1]]
    ref = _ref(rows, [5, 1], 0)
    # (0, 1) -> (1, 2) would pass the blocked (1, 1), (1, 2) -> (2, 1) too: five moves along the rows and columns
    assert ref["dist"].tolist() == [0, 5, 10, INT_MAX, INT_MAX, 15, INT_MAX, 25, 20]
    assert ref["parent"].tolist() == [-1, 0, 1, -1, -1, 2, -1, 8, 5]
    assert ref["goal_cell"].tolist() == [7, 0] and ref["goal_cost"].tolist() == [25, 0] and ref["cells"].tolist() == [1, 2]
    assert ref["goal_key"].tolist() == [(25 << 32) | 7, 0]
    assert ref["path"][0].tolist() == [7, 8, 5, 2, 1, 0, -1, -1] and ref["path_cells"].tolist() == [6, 1]
    assert ref["counts"].tolist() == [6, 6]
    short = _ref(rows, [5, 1], 0, path_max=5)
    assert short["path"][0].tolist() == [7, 8, 5, 2, 1] and short["path_cells"].tolist() == [5, 1]          # not complete: no 0 at its end
    assert _ref(rows, [5, 1], 0, path_max=6)["path"][0].tolist() == [7, 8, 5, 2, 1, 0]
    one = _ref(rows, [5, 1], 0, path_max=1)
    assert one["path"].tolist() == [[7], [0]] and one["path_cells"].tolist() == [1, 1]
    # the wall made passable: the diagonal is open, the wall's own cells are goals, and the start may stand on a labelled cell
    ref = _ref(rows, [5, 1, 1, -1], 6, passable=[1])
    assert ref["dist"].tolist() == [10, 12, 14, 5, 7, 12, 0, 5, 10] and ref["counts"].tolist() == [9, 9]
    assert ref["goal_cell"].tolist() == [6, 6, -1, -1] and ref["goal_cost"].tolist() == [0, 0, INT_MAX, INT_MAX]      # the start touches both
    assert ref["cells"].tolist() == [1, 2, 0, 0] and ref["path"][1].tolist() == [6] + [-1] * 7
    ref = _ref([[1, 1, 2], [2, 2, 2]], [1], 1, passable=[1])         # nothing free but the passable object: its own cells are the goals
    assert ref["dist"].tolist() == [5, 0] + [INT_MAX] * 4 and ref["goal_cell"].tolist() == [1] and ref["path"][0].tolist() == [1] + [-1] * 7


def test_reference_goal_tie_takes_the_lowest_cell():
    m = RC.maps(8, 9, 32, 32)["two goal cells of equal cost"]
    ref = RC.reference(m["labels"], m["objects"], 9, m["from_cell"])
    r, c = divmod(m["from_cell"], 9)
    assert ref["goal_cost"].tolist() == [7] and ref["goal_cell"].tolist() == [(r + 1) * 9 + c - 1]
    assert ref["dist"][(r + 1) * 9 + c + 1] == 7


def test_reference_maps_are_what_their_names_say():
    tr, tc = 8, 8                                                    # small tiles: the same maps, quickly
    ms = RC.maps(2 * tr + 6, 2 * tc + 3, tr, tc)
    assert len(ms) == 18
    refs = {k: RC.reference(m["labels"], m["objects"], 2 * tc + 3, m["from_cell"], m["passable"]) for k, m in ms.items()}
    for name in ("corner opening", "corner opening at the four-tile corner", "row-end pair as the only link"):
        assert refs[name]["goal_cost"][0] == INT_MAX and refs[name]["path_cells"][0] == 0, name
        assert refs[name]["counts"][1] < refs[name]["counts"][0], name
    assert refs["object enclosed"]["goal_cost"].tolist()[1] == INT_MAX and refs["object enclosed"]["goal_cost"][0] < INT_MAX
    assert refs["start enclosed"]["counts"][1] == 1 and refs["start enclosed"]["goal_cost"].tolist() == [0, INT_MAX]
    assert refs["start on a labelled cell"]["goal_cost"][1] == 0
    m, ref = ms["a slot made passable"], refs["a slot made passable"]
    own = RC.slots(m["labels"], m["objects"]) == 1
    assert (ref["dist"][own] < INT_MAX).all() and ref["goal_cost"][1] < ref["dist"][own].min()      # crossed, and touched before that
    ref = refs["diagonal step across the four-tile corner"]
    assert ref["dist"][tr * (2 * tc + 3) + tc] == ref["dist"][(tr - 1) * (2 * tc + 3) + tc - 1] + 7
    assert ref["parent"][tr * (2 * tc + 3) + tc] == (tr - 1) * (2 * tc + 3) + tc - 1
    for name in ("wall, gap at the tile border", "wall, gap before the tile border", "wall, gap one off the tile border", "serpentine",
                 "spiral inside one tile"):
        assert refs[name]["goal_cost"][0] < INT_MAX and refs[name]["path_cells"][0] > tr, name
    assert refs["serpentine"]["goal_cost"][0] >= 5 * (2 * tc + 2) * (tr + 2)               # along every corridor
    assert (refs["64 objects"]["cells"] > 0).sum() > 32


def test_route_header_and_ctypes_table_agree():
    """include/eod_route.h against `_lib.ROUTE_SIGNATURES`: the same two entry points on both sides, exported by the cross-compiled
    library, in no other table or header; the header's constants are the binding's; the header compiles as C on its own."""
    import os
    import re
    import shutil
    import subprocess
    import tempfile
    import __graft_entry__
    __graft_entry__.build()
    from embodied_object_detection_amd import _lib, build, ops
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    path = os.path.join(root, "include", "eod_route.h")
    txt = open(path).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    declared = sorted(set(re.findall(r"^(?:int|size_t)\s+(eod_\w+)\s*\(", code, flags=re.M)))
    assert declared == sorted(_lib.ROUTE_SIGNATURES) == ["eod_map_route", "eod_map_route_workspace_bytes"]
    others = (set(_lib.SIGNATURES) | set(_lib.PLACE_SIGNATURES) | set(_lib.REGIONS_SIGNATURES) | set(_lib.INVENTORY_SIGNATURES)
              | set(_lib.DESCRIBE_SIGNATURES) | set(_lib.RELATIONS_SIGNATURES))
    assert not set(_lib.ROUTE_SIGNATURES) & others and len(_lib.SIGNATURES) == 75
    for other in ("eod_hip.h", "eod_place.h", "eod_regions.h", "eod_inventory.h", "eod_describe.h", "eod_relations.h"):
        assert "eod_map_route" not in open(os.path.join(root, "include", other)).read()
    for name, n in (("eod_map_route", 24), ("eod_map_route_workspace_bytes", 2)):
        res, args = _lib.ROUTE_SIGNATURES[name]
        params = re.search(rf"\b{name}\s*\(([^)]*)\)", code, flags=re.S).group(1)
        assert len(params.split(",")) == len(args) == n, name
    lib = _lib.load()
    for name, (res, args) in _lib.ROUTE_SIGNATURES.items():
        fn = getattr(lib, name)                                                  # exported by the library built for gfx950
        assert fn.restype is res and list(fn.argtypes) == list(args), name
    val = lambda name: int(re.search(rf"#define {name} (\d+)", txt).group(1))
    assert (ops.ROUTE_K_MAX, ops.ROUTE_P_MAX, ops.ROUTE_N_MAX, ops.ROUTE_DIM_MAX, ops.ROUTE_PATH_MAX, ops.ROUTE_SWEEPS_MAX) == (
        val("EOD_ROUTE_K_MAX"), val("EOD_ROUTE_P_MAX"), val("EOD_ROUTE_N_MAX"), val("EOD_ROUTE_DIM_MAX"), val("EOD_ROUTE_PATH_MAX"),
        val("EOD_ROUTE_SWEEPS_MAX")) == (64, 64, 2 ** 22, 32767, 1024, 1024)
    assert (ops.ROUTE_COST_ORTH, ops.ROUTE_COST_DIAG) == (val("EOD_ROUTE_COST_ORTH"), val("EOD_ROUTE_COST_DIAG")) == (RC.ORTH, RC.DIAG) == (5, 7)
    assert (ops.ROUTE_TILE_ROWS, ops.ROUTE_TILE_COLS) == (val("EOD_ROUTE_TILE_ROWS"), val("EOD_ROUTE_TILE_COLS"))
    assert ops.ROUTE_COST_DIAG * ops.ROUTE_N_MAX < INT_MAX                       # a cost is never the "none" value
    src = open(os.path.join(root, "embodied_object_detection_amd", "csrc", "route.hip")).read()
    assert "RT_TR = EOD_ROUTE_TILE_ROWS, RT_TC = EOD_ROUTE_TILE_COLS" in src   # the kernels' tile is the header's
    assert "route.hip" in build.SOURCES
    for rows, cols in ((1, 1), (200, 200), (70, 67), (32767, 128), (1, 32767)):
        tiles = -(-rows // ops.ROUTE_TILE_ROWS) * -(-cols // ops.ROUTE_TILE_COLS)
        need = lib.eod_map_route_workspace_bytes(rows * cols, cols)
        assert need >= 12 * tiles + rows * cols and need % 8 == 0 and need == 4 * ops.map_route_workspace(rows * cols, cols)
    for N, cols in ((0, 1), (10, 3), (2 ** 22 + 1, 1), (32768, 1), (32768, 32768), (-4, 2), (4, 0)):
        assert lib.eod_map_route_workspace_bytes(N, cols) == 0
    assert ops.map_route_sweeps(200, 200) == 4 * 7 + 4 and ops.map_route_sweeps(1, 32767) == 1024 and ops.map_route_sweeps(1, 1) == 8
    gcc = shutil.which("gcc")                                                    # the header compiles as C on its own
    if gcc is not None:
        with tempfile.TemporaryDirectory() as d:
            c = os.path.join(d, "t.c")
            open(c, "w").write(f'#include "{path}"\nint main(void) {{ return EOD_ROUTE_K_MAX == 64 ? 0 : 1; }}\n')
            subprocess.run([gcc, "-std=c11", "-Wall", "-Werror", "-o", os.path.join(d, "t"), c], check=True)
            assert subprocess.run([os.path.join(d, "t")]).returncode == 0


def test_route_kernels_use_no_scratch():
    import __graft_entry__
    __graft_entry__.build()
    from embodied_object_detection_amd import build
    usage = build.resource_usage()
    if not any("route_" in k for k in usage):       # a library built elsewhere, without the remarks: build them here
        build.build(force=True, verbose=False)
        usage = build.resource_usage()
    mine = {k: v for k, v in usage.items() if "route_" in k}
    names = ("init", "sweep", "finish", "path")
    assert sorted(n for k in mine for n in names if f"route_{n}_kernel" in k) == sorted(names), sorted(mine)
    for k in mine:
        assert not any(s in k for s in ("place_", "regions_", "inventory_", "describe_", "relations_")), k
    assert not [k for k in build.scratch_offenders(usage) if "route_" in k]
    assert all(v.get("scratch", 0) == 0 for v in mine.values())
    sweep = next(v for k, v in mine.items() if "route_sweep_kernel" in k)
    assert sweep["lds"] <= 160 * 1024 // 8 and sweep["vgprs"] <= 64, sweep       # eight workgroups of four waves per CU


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
    ptrs = ("labels", "objects", "passable", "dist", "parent", "goal_key", "goal_cost", "goal_cell", "cells", "path", "path_cells", "counts",
            "status", "workspace")

    def call(N=100, K=5, P=2, cols=10, from_cell=0, path_max=16, sweeps=4, resume=0, workspace_bytes=4096, **kw):
        a = {name: p for name in ptrs}
        a.update(kw)
        return lib.eod_map_route(a["labels"], a["objects"], a["passable"], N, K, P, cols, from_cell, path_max, sweeps, resume,
                                 *[a[n] for n in ptrs[3:]], workspace_bytes, None)

    for kw in (dict(K=0), dict(K=65), dict(K=-1), dict(P=-1), dict(P=65), dict(N=0), dict(N=2 ** 22 + 1), dict(N=-5), dict(cols=0),
               dict(cols=-10), dict(cols=7), dict(cols=101), dict(from_cell=-1), dict(from_cell=100), dict(from_cell=2 ** 31 - 1),
               dict(path_max=0), dict(path_max=1025), dict(path_max=-3), dict(sweeps=0), dict(sweeps=1025), dict(sweeps=-1),
               dict(resume=2), dict(resume=-1), dict(N=32768, cols=32768), dict(N=32768, cols=1), dict(N=2 ** 22, cols=2 ** 22),
               dict(N=2 ** 22, cols=64)):
        assert call(**kw) == BAD, kw
    none = {name: None for name in ptrs}
    assert call(K=0, **none) == BAD                                              # a bad dimension wins over a null pointer
    assert call(sweeps=0, goal_key=p + 4) == BAD                                 # and over alignment
    assert call(path_max=0, workspace_bytes=0) == BAD                            # and over the workspace
    for name in ptrs:
        assert call(**{name: None}) == NULL, name
        assert call(**{name: None, "goal_key" if name != "goal_key" else "workspace": p + 4}) == NULL, name     # null wins over alignment
    assert call(P=0, passable=None, workspace_bytes=0) == CAPACITY               # passable may be null without passable labels
    for kw in (dict(goal_key=p + 4), dict(workspace=p + 4), dict(goal_key=p + 1), dict(labels=p + 2), dict(objects=p + 1),
               dict(passable=p + 2), dict(dist=p + 2), dict(parent=p + 1), dict(goal_cost=p + 3), dict(goal_cell=p + 2), dict(cells=p + 1),
               dict(path=p + 2), dict(path_cells=p + 3), dict(counts=p + 1), dict(status=p + 2)):
        assert call(**kw) == ALIGN, kw
        assert call(workspace_bytes=0, **kw) == ALIGN, kw                        # alignment wins over the workspace
    need = lib.eod_map_route_workspace_bytes(100, 10)
    for short in (0, 8, need - 1):
        assert call(workspace_bytes=short) == CAPACITY, short


def test_ops_refuse_on_the_host_naming_the_argument():
    import torch
    import __graft_entry__
    __graft_entry__.build()
    from embodied_object_detection_amd import _lib, ops
    labels, objects = torch.zeros((120,), dtype=torch.int32), torch.zeros((5,), dtype=torch.int32)
    for bad in (torch.zeros((0,), dtype=torch.int32), torch.zeros((120,), dtype=torch.int64), torch.zeros((12, 10), dtype=torch.int32),
                torch.zeros((240,), dtype=torch.int32)[::2], torch.zeros((120,)), np.zeros(120, np.int32)):
        with pytest.raises(_lib.EodError, match="object_labels"):
            ops.map_route(bad, objects, 10, 0)
    with pytest.raises(_lib.EodError, match="object_labels: N 4194305"):          # no storage behind it: refused by its shape
        ops.map_route(torch.empty((2 ** 22 + 1,), dtype=torch.int32, device="meta"), objects, 1, 0)
    for bad in (torch.zeros((0,), dtype=torch.int32), torch.zeros((65,), dtype=torch.int32), torch.zeros((5,), dtype=torch.int64),
                torch.zeros((1, 5), dtype=torch.int32), torch.zeros((10,), dtype=torch.int32)[::2], [1, 2, 3],
                torch.zeros((5,), dtype=torch.int32, device="meta")):
        with pytest.raises(_lib.EodError, match="objects"):
            ops.map_route(labels, bad, 10, 0)
    for bad in (0, -10, 7, 121, 2.5, True, None):
        with pytest.raises(_lib.EodError, match="cols"):
            ops.map_route(labels, objects, bad, 0)
    with pytest.raises(_lib.EodError, match="cols"):
        ops.map_route(torch.zeros((32768,), dtype=torch.int32), objects, 1, 0)    # 32768 rows
    for bad in (-1, 120, 3.0, None, False):
        with pytest.raises(_lib.EodError, match="from_cell"):
            ops.map_route(labels, objects, 10, bad)
    for bad in (torch.zeros((65,), dtype=torch.int32), torch.zeros((3,), dtype=torch.int64), torch.zeros((2, 2), dtype=torch.int32),
                torch.zeros((4,), dtype=torch.int32, device="meta"), 7, ["a"], list(range(65))):
        with pytest.raises(_lib.EodError, match="passable"):
            ops.map_route(labels, objects, 10, 0, passable=bad)
    for bad in (0, 1025, -1, 2.5, True):
        with pytest.raises(_lib.EodError, match="path_max"):
            ops.map_route(labels, objects, 10, 0, path_max=bad)
    for bad in (0, 1025, -1, 2.5, True):
        with pytest.raises(_lib.EodError, match="sweeps"):
            ops.map_route(labels, objects, 10, 0, sweeps=bad)
    for bad in (torch.zeros((119,), dtype=torch.int32), torch.zeros((120,), dtype=torch.int64), {"dist": torch.zeros((60, 2), dtype=torch.int32)},
                3, torch.zeros((120,), dtype=torch.int32, device="meta")):
        with pytest.raises(_lib.EodError, match="resume"):
            ops.map_route(labels, objects, 10, 0, resume=bad)
    with pytest.raises(_lib.EodError, match="no CPU fallback"):                   # tensors on the host: refused last
        ops.map_route(labels, objects, 10, 119, passable=[3, 4], path_max=1024, sweeps=1024, resume=torch.zeros((120,), dtype=torch.int32))


def test_model_surfaces_require_the_grid_and_the_start():
    import torch
    import __graft_entry__
    __graft_entry__.build()
    from embodied_object_detection_amd import _lib
    from embodied_object_detection_amd.modeling.meta_arch import _route
    labels = torch.zeros((120,), dtype=torch.int32)
    with pytest.raises(_lib.EodError, match="map_shape"):
        _route([1, 2], labels, None, 0)
    with pytest.raises(_lib.EodError, match="map_shape"):
        _route([1, 2], labels, (11, 10), 0)
    with pytest.raises(_lib.EodError, match="from_cell"):
        _route([1, 2], labels, (12, 10), None)
    with pytest.raises(_lib.EodError, match="from_cell"):
        _route([1, 2], labels, (12, 10), 120)
    with pytest.raises(_lib.EodError, match="path_max"):
        _route([1, 2], labels, (12, 10), 0, path_max=0)
    with pytest.raises(_lib.EodError, match="no CPU fallback"):                   # sequences of objects and passable labels will do
        _route([1, 2], labels, (12, 10), 5, passable=[0])


def test_route_metres():
    from embodied_object_detection_amd.data.robot import RobotFrontEnd
    front = RobotFrontEnd.__new__(RobotFrontEnd)
    front.res = 0.05
    m = front.route_metres(np.array([[0, 25, INT_MAX], [5, 7, 12]], np.int32))
    assert m.dtype == np.float64 and m.shape == (2, 3)
    assert m[0].tolist() == [0.0, 5 * 0.05, np.inf] and m[1].tolist() == [0.05, 7 / 5.0 * 0.05, 12 / 5.0 * 0.05]
    import torch
    assert front.route_metres(torch.tensor([10, INT_MAX], dtype=torch.int32)).tolist() == [0.1, np.inf]
