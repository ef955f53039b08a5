"""The host side of `map_clearance` (no GPU): the reference of `_clearance_cases.py` on hand-worked maps, include/eod_clearance.h
against its ctypes table and the cross-compiled library, the build's records, and every refused argument (the entry point returns
before a launch, so it is callable here)."""
import time

import numpy as np
import pytest

import _clearance_cases as CC

INT_MAX = CC.INT_MAX


def _ref(rows_of_labels, objects, radius2=0, keep_cell=-1, passable=()):
    g = np.array(rows_of_labels, np.int32)
    return CC.reference(g.reshape(-1), np.array(objects, np.int32), g.shape[1], radius2, keep_cell, passable)


def test_reference_hand_worked_examples():
    """The two maps of the header's comment."""
    ref = _ref([[-1, -1, -1, -1], [-1, 5, -1, -1], [-1, -1, -1, 6]], [6, 5], radius2=1)
    assert ref["d2"].tolist() == [2, 1, 2, 4, 1, 0, 1, 1, 2, 1, 1, 0]
    assert ref["nearest"].tolist() == [5, 5, 5, 11, 5, 5, 5, 11, 5, 5, 11, 11]
    assert ref["owner"].tolist() == [5, 5, 5, 6, 5, 5, 5, 6, 5, 5, 6, 6]
    assert ref["inflated"].tolist() == [-1, 5, -1, -1, 5, 5, 5, 6, -1, 5, 6, 6]
    assert ref["cells"].tolist() == [1, 1] and ref["territory"].tolist() == [3, 7]
    assert ref["widest_d2"].tolist() == [4, 2] and ref["widest_cell"].tolist() == [3, 0]
    assert ref["widest_key"].tolist() == [(4 << 32) | (~3 & 0xFFFFFFFF), (2 << 32) | (~0 & 0xFFFFFFFF)]
    assert ref["counts"].tolist() == [2, 10, 6] and ref["open_key"].tolist() == [(4 << 32) | (~3 & 0xFFFFFFFF)]
    assert ref["status"].tolist() == [0, 0]
    for k in CC.KEYS:
        assert ref[k].dtype == (np.uint64 if k in ("widest_key", "open_key") else np.int32), k
    ref = _ref([[3, -1, 4]], [3, 4])
    assert ref["d2"][1] == 1 and ref["nearest"][1] == 0 and ref["owner"][1] == 3          # the lowest cell wins the tie
    assert ref["inflated"].tolist() == [3, -1, 4] and ref["territory"].tolist() == [1, 0] and ref["counts"].tolist() == [2, 1, 0]


def test_reference_radius_keep_cell_and_passable():
    rows = [[-1, -1, -1, -1], [-1, 5, -1, -1], [-1, -1, -1, 6]]
    zero = _ref(rows, [6, 5])
    assert zero["inflated"].tolist() == np.array(rows).reshape(-1).tolist() and zero["counts"].tolist() == [2, 10, 0]
    # keep_cell 6 = (1, 2): the cells at most 1 from it (2, 5, 6, 7, 10) are not grown; 5 is blocked anyway
    kept = _ref(rows, [6, 5], radius2=1, keep_cell=6)
    assert kept["inflated"].tolist() == [-1, 5, -1, -1, 5, 5, -1, -1, -1, 5, -1, 6] and kept["counts"].tolist() == [2, 10, 3]
    assert kept["d2"].tolist() == zero["d2"].tolist()                # keep_cell changes nothing but inflated and counts[2]
    on_blocked = _ref(rows, [6, 5], radius2=1, keep_cell=5)          # standing on the object: its four neighbours stay free
    assert on_blocked["inflated"].tolist() == [-1, -1, -1, -1, -1, 5, -1, 6, -1, -1, 6, 6]
    big = _ref(rows, [6, 5], radius2=INT_MAX - 1)
    assert big["inflated"].tolist() == big["owner"].tolist() and big["counts"].tolist() == [2, 10, 10]
    # 5 made passable: it is free, has cells, no territory, and is grown over like any free cell
    ref = _ref(rows, [6, 5], radius2=9, passable=[5, 8])
    assert ref["d2"].tolist() == [13, 8, 5, 4, 10, 5, 2, 1, 9, 4, 1, 0] and (ref["nearest"] == 11).all()
    assert ref["cells"].tolist() == [1, 1] and ref["territory"].tolist() == [11, 0] and ref["counts"].tolist() == [1, 11, 9]
    assert ref["inflated"].tolist() == [-1, 6, 6, 6, -1, 6, 6, 6, 6, 6, 6, 6]
    assert ref["widest_d2"].tolist() == [13, 0] and ref["widest_cell"].tolist() == [0, -1] and ref["widest_key"][1] == 0
    none = _ref(rows, [6, 5], radius2=3, passable=[5, 6])
    assert (none["d2"] == INT_MAX).all() and (none["nearest"] == -1).all() and (none["owner"] == -1).all()
    assert none["inflated"].tolist() == zero["inflated"].tolist() and none["counts"].tolist() == [0, 12, 0]
    assert none["open_key"].tolist() == [(INT_MAX << 32) | 0xFFFFFFFF] and none["territory"].tolist() == [0, 0]
    full = _ref([[1, 2], [2, 1]], [2])
    assert full["d2"].tolist() == [0] * 4 and full["nearest"].tolist() == [0, 1, 2, 3] and full["open_key"].tolist() == [0]
    assert full["cells"].tolist() == [2] and full["counts"].tolist() == [4, 0, 0] and full["widest_cell"].tolist() == [-1]


def test_reference_rows_do_not_wrap_and_ties_take_the_lowest_cell():
    ref = _ref([[-1, -1, 9], [-1, -1, -1]], [9])
    assert ref["d2"].tolist() == [4, 1, 0, 5, 2, 1]                  # cell 3 = (1, 0) follows cell 2 in memory: two columns and a row away
    ref = _ref([[3], [-1], [4]], [3, 4])
    assert ref["nearest"].tolist() == [0, 0, 2]                      # up/down
    g = np.full((5, 5), -1, np.int32)
    g[0, 2], g[2, 0], g[2, 4], g[4, 2] = 5, 6, 7, 8
    ref = CC.reference(g.reshape(-1), np.array([5, 6, 7, 8], np.int32), 5)
    assert ref["d2"][12] == 4 and ref["nearest"][12] == 2 and ref["owner"][12] == 5       # four-way
    tr, cc, halo = 4, 64, 64
    ms = CC.maps(4 * tr + 3, 2 * cc + halo + 3, tr, cc, halo)
    cols = 2 * cc + halo + 3
    n = 0
    for name, m in ms.items():
        if name.startswith("diagonal/straight"):
            r = CC.reference(m["labels"], m["objects"], cols)
            x = m["keep_cell"]
            assert r["d2"][x] == 25 and r["owner"][x] == (31 if "below" in name else 30), name
            n += 1
    assert n == 6
    for rows_, cols_ in ((70, cc + 3), (4 * tr + 3, cols)):           # both multi-chunk grids of the GPU tests: the border is crossed
        crossing = {k: m for k, m in CC.maps(rows_, cols_, tr, cc, halo).items() if "across the chunk border" in k}
        assert len(crossing) == 4, sorted(crossing)
        for name, m in crossing.items():
            seen = m["keep_cell"] % cols_
            cand = np.flatnonzero(m["labels"] >= 0) % cols_
            assert cand.size == 2 and ((cand >= cc).all() and seen < cc if "right" in name else (cand < cc).all() and seen >= cc), name
    assert not [k for k in CC.maps(tr - 1 + 4, cc - 3, tr, cc, halo) if "across" in k]      # one chunk: the names say "inside"
    r = CC.reference(ms["row-end pair"]["labels"], ms["row-end pair"]["objects"], cols)
    mid = (4 * tr + 3) // 2
    assert r["d2"][mid * cols] == 1 + (cols - 1) ** 2 and r["d2"][mid * cols - 1] == 0
    r = CC.reference(ms["corner 00"]["labels"], ms["corner 00"]["objects"], cols)
    assert r["d2"][-1] == (4 * tr + 2) ** 2 + (cols - 1) ** 2 and (r["nearest"] == 0).all()
    m = ms["a slot made passable"]
    r = CC.reference(m["labels"], m["objects"], cols, m["radius2"], m["keep_cell"], m["passable"])
    assert r["cells"][1] == 9 and r["territory"][1] == 0 and r["d2"][m["keep_cell"]] > 0
    assert len(ms) == 27


def test_reference_is_quick_enough():
    """The largest grid of the GPU tests with every cell blocked: N^2 = 22 M pairs."""
    labels = np.full(70 * 67, 4, np.int32)
    times = []
    for keep in (11, 12, 13):                                        # three maps the reference has not cached; the quickest counts
        t = time.perf_counter()
        ref = CC.reference(labels, np.array([4], np.int32), 67, 3, keep)
        times.append(time.perf_counter() - t)
        assert (ref["d2"] == 0).all()
    print(f"reference, 70 x 67, every cell blocked: {min(times):.2f} s (of {[round(v, 2) for v in times]})")
    assert min(times) < 2.0                                          # a second or two per map


def test_clearance_header_and_ctypes_table_agree():
    """include/eod_clearance.h against `_lib.CLEARANCE_SIGNATURES`: the same two entry points on both sides, exported by the
    cross-compiled library, in no other table or header; the header's constants are the binding's; the header compiles as C on its
    own; a real distance is never INT_MAX."""
    import os
    import re
    import shutil
    import subprocess
    import tempfile
    import __graft_entry__
    __graft_entry__.build()
    from embodied_object_detection_amd import _lib, build, ops
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    path = os.path.join(root, "include", "eod_clearance.h")
    txt = open(path).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    declared = sorted(set(re.findall(r"^(?:int|size_t)\s+(eod_\w+)\s*\(", code, flags=re.M)))
    assert declared == sorted(_lib.CLEARANCE_SIGNATURES) == ["eod_map_clearance", "eod_map_clearance_workspace_bytes"]
    others = (set(_lib.SIGNATURES) | set(_lib.PLACE_SIGNATURES) | set(_lib.REGIONS_SIGNATURES) | set(_lib.INVENTORY_SIGNATURES)
              | set(_lib.DESCRIBE_SIGNATURES) | set(_lib.RELATIONS_SIGNATURES) | set(_lib.ROUTE_SIGNATURES))
    assert not set(_lib.CLEARANCE_SIGNATURES) & others and len(_lib.SIGNATURES) == 75 and len(_lib.ROUTE_SIGNATURES) == 2
    for other in ("eod_hip.h", "eod_place.h", "eod_regions.h", "eod_inventory.h", "eod_describe.h", "eod_relations.h", "eod_route.h"):
        assert "eod_map_clearance" not in open(os.path.join(root, "include", other)).read()
    for name, n in (("eod_map_clearance", 24), ("eod_map_clearance_workspace_bytes", 2)):
        res, args = _lib.CLEARANCE_SIGNATURES[name]
        params = re.search(rf"\b{name}\s*\(([^)]*)\)", code, flags=re.S).group(1)
        assert len(params.split(",")) == len(args) == n, name
    lib = _lib.load()
    for name, (res, args) in _lib.CLEARANCE_SIGNATURES.items():
        fn = getattr(lib, name)                                                  # exported by the library built for gfx950
        assert fn.restype is res and list(fn.argtypes) == list(args), name
    val = lambda name: int(re.search(rf"#define {name} (\d+)", txt).group(1))
    assert (ops.CLEARANCE_K_MAX, ops.CLEARANCE_P_MAX, ops.CLEARANCE_N_MAX, ops.CLEARANCE_DIM_MAX) == (
        val("EOD_CLEARANCE_K_MAX"), val("EOD_CLEARANCE_P_MAX"), val("EOD_CLEARANCE_N_MAX"), val("EOD_CLEARANCE_DIM_MAX")) == (
        ops.ROUTE_K_MAX, ops.ROUTE_P_MAX, ops.ROUTE_N_MAX, ops.ROUTE_DIM_MAX) == (64, 64, 2 ** 22, 32767)      # the route's limits
    assert (ops.CLEARANCE_TILE_ROWS, ops.CLEARANCE_CHUNK_COLS, ops.CLEARANCE_HALO_COLS) == (
        val("EOD_CLEARANCE_TILE_ROWS"), val("EOD_CLEARANCE_CHUNK_COLS"), val("EOD_CLEARANCE_HALO_COLS"))
    # the largest real distance, between opposite corners of the largest grid one way, is below the "none" value
    assert 2 * (ops.CLEARANCE_DIM_MAX - 1) ** 2 == 2 * 32766 ** 2 < 2 ** 31 - 1 == INT_MAX == ops.CLEARANCE_NONE
    src = open(os.path.join(root, "embodied_object_detection_amd", "csrc", "clearance.hip")).read()
    assert "CL_TR = EOD_CLEARANCE_TILE_ROWS, CL_CC = EOD_CLEARANCE_CHUNK_COLS, CL_HALO = EOD_CLEARANCE_HALO_COLS" in src
    assert "clearance.hip" in build.SOURCES
    for rows, cols in ((1, 1), (200, 200), (70, 67), (32767, 128), (1, 32767)):
        need = lib.eod_map_clearance_workspace_bytes(rows * cols, cols)
        assert need >= 5 * rows * cols and need % 8 == 0 and need == 4 * ops.map_clearance_workspace(rows * cols, cols)
    for N, cols in ((0, 1), (10, 3), (2 ** 22 + 1, 1), (32768, 1), (32768, 32768), (-4, 2), (4, 0)):
        assert lib.eod_map_clearance_workspace_bytes(N, cols) == 0
    with pytest.raises(_lib.EodError, match="map_clearance_workspace"):
        ops.map_clearance_workspace(10, 3)
    # the header compiles as C on its own, with whichever C compiler there is (the one that builds the oracle's C restatement)
    cc = next((p for p in (shutil.which(n) for n in ("gcc", "cc", "clang")) if p), None)
    assert cc is not None, "no C compiler (gcc, cc, clang) on PATH: the header cannot be checked as C"
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "t.c")
        open(c, "w").write(f'#include "{path}"\nint main(void) {{ return EOD_CLEARANCE_K_MAX == 64 ? 0 : 1; }}\n')
        subprocess.run([cc, "-std=c11", "-Wall", "-Werror", "-o", os.path.join(d, "t"), c], check=True)
        assert subprocess.run([os.path.join(d, "t")]).returncode == 0


def test_clearance_kernels_use_no_scratch():
    import __graft_entry__
    __graft_entry__.build()
    from embodied_object_detection_amd import build
    usage = build.resource_usage()
    if not any("clearance_" in k for k in usage):       # a library built elsewhere, without the remarks: build them here
        build.build(force=True, verbose=False)
        usage = build.resource_usage()
    mine = {k: v for k, v in usage.items() if "clearance_" in k}
    names = ("init", "column", "row", "finish", "widest")
    assert sorted(n for k in mine for n in names if f"clearance_{n}_kernel" in k) == sorted(names), sorted(mine)
    for k in mine:
        assert not any(s in k for s in ("route_", "place_", "regions_", "inventory_", "describe_", "relations_")), k
    assert not [k for k in build.scratch_offenders(usage) if "clearance_" in k]
    assert all(v.get("scratch", 0) == 0 for v in mine.values())
    row = next(v for k, v in mine.items() if "clearance_row_kernel" in k)
    assert row["lds"] <= 160 * 1024 // 8 and row["vgprs"] <= 64, row             # eight workgroups of four waves per CU


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
    ptrs = ("labels", "objects", "passable", "d2", "nearest", "owner", "inflated", "cells", "territory", "widest_key", "widest_d2",
            "widest_cell", "open_key", "counts", "status", "workspace")

    def call(N=100, K=5, P=2, cols=10, radius2=4, keep_cell=-1, workspace_bytes=4096, **kw):
        a = {name: p for name in ptrs}
        a.update(kw)
        return lib.eod_map_clearance(a["labels"], a["objects"], a["passable"], N, K, P, cols, radius2, keep_cell,
                                     *[a[n] for n in ptrs[3:]], workspace_bytes, None)

    for kw in (dict(K=0), dict(K=65), dict(K=-1), dict(P=-1), dict(P=65), dict(N=0), dict(N=2 ** 22 + 1), dict(N=-5), dict(cols=0),
               dict(cols=-10), dict(cols=7), dict(cols=101), dict(radius2=-1), dict(radius2=2 ** 31 - 1), dict(radius2=-2 ** 31),
               dict(keep_cell=-2), dict(keep_cell=100), dict(keep_cell=2 ** 31 - 1), dict(N=32768, cols=32768), dict(N=32768, cols=1),
               dict(N=2 ** 22, cols=2 ** 22), dict(N=2 ** 22, cols=64)):
        assert call(**kw) == BAD, kw
    none = {name: None for name in ptrs}
    assert call(K=0, **none) == BAD                                              # a bad dimension wins over a null pointer
    assert call(radius2=-1, widest_key=p + 4) == BAD                             # and over alignment
    assert call(keep_cell=100, workspace_bytes=0) == BAD                         # and over the workspace
    for name in ptrs:
        assert call(**{name: None}) == NULL, name
        assert call(**{name: None, "widest_key" if name != "widest_key" else "workspace": p + 4}) == NULL, name     # null wins over alignment
        assert call(workspace_bytes=0, **{name: None}) == NULL, name                                                # and over the workspace
    assert call(P=0, passable=None, workspace_bytes=0) == CAPACITY               # passable may be null without passable labels
    for kw in (dict(widest_key=p + 4), dict(open_key=p + 4), dict(workspace=p + 4), dict(widest_key=p + 1), dict(labels=p + 2),
               dict(objects=p + 1), dict(passable=p + 2), dict(d2=p + 2), dict(nearest=p + 1), dict(owner=p + 3), dict(inflated=p + 2),
               dict(cells=p + 1), dict(territory=p + 2), dict(widest_d2=p + 3), dict(widest_cell=p + 1), dict(counts=p + 1),
               dict(status=p + 2)):
        assert call(**kw) == ALIGN, kw
        assert call(workspace_bytes=0, **kw) == ALIGN, kw                        # alignment wins over the workspace
    need = lib.eod_map_clearance_workspace_bytes(100, 10)
    assert need == 256 + 512
    for short in (0, 8, need - 1):
        assert call(workspace_bytes=short) == CAPACITY, short
    assert call(radius2=2 ** 31 - 2, keep_cell=99, workspace_bytes=need - 1) == CAPACITY      # the largest values pass the first check


def test_ops_refuse_on_the_host_naming_the_argument():
    import torch
    import __graft_entry__
    __graft_entry__.build()
    from embodied_object_detection_amd import _lib, ops
    labels, objects = torch.zeros((120,), dtype=torch.int32), torch.zeros((5,), dtype=torch.int32)
    for bad in (torch.zeros((0,), dtype=torch.int32), torch.zeros((120,), dtype=torch.int64), torch.zeros((12, 10), dtype=torch.int32),
                torch.zeros((240,), dtype=torch.int32)[::2], torch.zeros((120,)), np.zeros(120, np.int32)):
        with pytest.raises(_lib.EodError, match="object_labels"):
            ops.map_clearance(bad, objects, 10)
    with pytest.raises(_lib.EodError, match="object_labels: N 4194305"):          # no storage behind it: refused by its shape
        ops.map_clearance(torch.empty((2 ** 22 + 1,), dtype=torch.int32, device="meta"), objects, 1)
    for bad in (torch.zeros((0,), dtype=torch.int32), torch.zeros((65,), dtype=torch.int32), torch.zeros((5,), dtype=torch.int64),
                torch.zeros((1, 5), dtype=torch.int32), torch.zeros((10,), dtype=torch.int32)[::2], [1, 2, 3],
                torch.zeros((5,), dtype=torch.int32, device="meta")):
        with pytest.raises(_lib.EodError, match="objects"):
            ops.map_clearance(labels, bad, 10)
    for bad in (0, -10, 7, 121, 2.5, True, None):
        with pytest.raises(_lib.EodError, match="cols"):
            ops.map_clearance(labels, objects, bad)
    with pytest.raises(_lib.EodError, match="cols"):
        ops.map_clearance(torch.zeros((32768,), dtype=torch.int32), objects, 1)   # 32768 rows
    for bad in (-1, 2 ** 31 - 1, 2 ** 40, 2.0, None, True):
        with pytest.raises(_lib.EodError, match="radius2"):
            ops.map_clearance(labels, objects, 10, radius2=bad)
    for bad in (-2, 120, 3.0, None, False):
        with pytest.raises(_lib.EodError, match="keep_cell"):
            ops.map_clearance(labels, objects, 10, keep_cell=bad)
    for bad in (torch.zeros((65,), dtype=torch.int32), torch.zeros((3,), dtype=torch.int64), torch.zeros((2, 2), dtype=torch.int32),
                torch.zeros((4,), dtype=torch.int32, device="meta"), 7, ["a"], list(range(65))):
        with pytest.raises(_lib.EodError, match="passable"):
            ops.map_clearance(labels, objects, 10, passable=bad)
    with pytest.raises(_lib.EodError, match="no CPU fallback"):                   # tensors on the host: refused last
        ops.map_clearance(labels, objects, 10, radius2=2 ** 31 - 2, keep_cell=119, passable=[3, 4])


def test_model_surfaces_require_the_grid():
    import torch
    import __graft_entry__
    __graft_entry__.build()
    from embodied_object_detection_amd import _lib
    from embodied_object_detection_amd.modeling.meta_arch import _clearance, _route
    labels = torch.zeros((120,), dtype=torch.int32)
    with pytest.raises(_lib.EodError, match="clearance: map_shape"):
        _clearance([1, 2], labels, None)
    with pytest.raises(_lib.EodError, match="clearance: map_shape"):
        _clearance([1, 2], labels, (11, 10))
    with pytest.raises(_lib.EodError, match="radius2"):
        _clearance([1, 2], labels, (12, 10), radius2=-1)
    with pytest.raises(_lib.EodError, match="keep_cell"):
        _clearance([1, 2], labels, (12, 10), keep_cell=120)
    with pytest.raises(_lib.EodError, match="map_clearance: object_labels on the host .no CPU fallback"):      # sequences will do
        _clearance([1, 2], labels, (12, 10), 4, 7, passable=[0])
    # the route with a body: the clearance's refusals come first, and a point's route is refused as before
    with pytest.raises(_lib.EodError, match="from_cell"):
        _route([1, 2], labels, (12, 10), None, body_radius2=1)
    with pytest.raises(_lib.EodError, match="map_shape"):
        _route([1, 2], labels, None, 0, body_radius2=1)
    with pytest.raises(_lib.EodError, match="radius2"):
        _route([1, 2], labels, (12, 10), 0, body_radius2=-1)
    with pytest.raises(_lib.EodError, match="map_clearance: object_labels on the host"):
        _route([1, 2], labels, (12, 10), 5, passable=[0], body_radius2=2)
    with pytest.raises(_lib.EodError, match="map_route: object_labels on the host"):
        _route([1, 2], labels, (12, 10), 5, passable=[0], body_radius2=None)


def test_clearance_metres_and_body_radius2():
    from embodied_object_detection_amd.data.robot import RobotFrontEnd
    front = RobotFrontEnd.__new__(RobotFrontEnd)
    front.res = 0.05
    m = front.clearance_metres(np.array([[0, 25, INT_MAX], [1, 2, 16]], np.int32))
    assert m.dtype == np.float64 and m.shape == (2, 3)
    assert m[0].tolist() == [0.0, 5 * 0.05, np.inf] and m[1].tolist() == [0.05, np.sqrt(2.0) * 0.05, 4 * 0.05]
    import torch
    assert front.clearance_metres(torch.tensor([4, INT_MAX], dtype=torch.int32)).tolist() == [0.1, np.inf]
    # 0.25 m on a 0.05 m grid is five cells: 25, although 0.25 / 0.05 is 5.000000000000001 or 4.999999999999999 in binary
    assert [front.body_radius2(v) for v in (0.0, 0.05, 0.07, 0.1, 0.25, 0.3, 0.04)] == [0, 1, 1, 4, 25, 36, 0]
    assert isinstance(front.body_radius2(0.25), int)
    front.res = 0.5
    assert [front.body_radius2(v) for v in (0.25, 0.5, 0.75, 1.0)] == [0, 1, 2, 4]
