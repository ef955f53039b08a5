"""The frontiers on the map without a GPU: the numpy reference of `_frontier_cases.py` on the hand-worked map of
include/eod_frontier.h and its variants, every output by hand; its symmetries; the header against the ctypes table and the
cross-compiled library; and every argument the entry points, the ops and the model surfaces refuse before any launch."""
import time

import numpy as np
import pytest

import _frontier_cases as FC

INT_MAX = FC.INT_MAX


def _key(hi, lo):
    return np.uint64((hi << 32) | (lo & 0xFFFFFFFF))


def test_reference_hand_worked_map():
    labels, seen, cols, since, here = FC.hand_map()
    assert (cols, since, here) == (8, 0, 16) and labels.size == 48
    kind = FC.kinds(labels, seen, since).reshape(6, 8)
    rows = ["".join("#.?"[k] for k in row) for row in kind]
    assert rows == ["....#???", "....#???", ".....???", "....#???", "....#???", "?...#???"]
    ones = FC.ALL_ONES
    for rank_by, order in ((0, (32, 20)), (1, (20, 32))):
        r = FC.reference(labels, seen, cols, since, None, here, (), min_cells=1, topk=3, rank_by=rank_by)
        assert r["counts"].tolist() == [5, 24, 19, 3, 2] and r["count"].tolist() == [2] and r["status"].tolist() == [0, 0]
        fl = np.full(48, -1)
        fl[[32, 41]] = 32
        fl[20] = 20
        assert r["frontier_labels"].tolist() == fl.tolist()
        ul = np.full((6, 8), -1)
        ul[:, 5:] = 5
        ul[5, 0] = 40
        assert r["unknown_labels"].tolist() == ul.reshape(-1).tolist()
        ua = np.zeros(48, int)
        ua[5], ua[40] = 18, 1
        assert r["unknown_area"].tolist() == ua.tolist()
        by = {32: dict(area=2, bbox=[4, 0, 5, 1], sum_rc=[9, 1], open_edges=2, behind_key=_key(1, ~40), behind_area=1, behind_label=40,
                       reach_key=_key(4, 32), reach_cost=4, reach_cell=32),
              20: dict(area=1, bbox=[2, 4, 2, 4], sum_rc=[2, 4], open_edges=1, behind_key=_key(18, ~5), behind_area=18, behind_label=5,
                       reach_key=_key(16, 20), reach_cost=16, reach_cell=20)}
        assert r["frontier"].tolist() == list(order) + [-1]
        for k, t in enumerate(order):
            for name, want in by[t].items():
                assert np.asarray(r[name][k]).tolist() == np.asarray(want).tolist(), (rank_by, t, name)
        pad = dict(frontier=-1, area=0, bbox=[0, 0, 0, 0], sum_rc=[0, 0], open_edges=0, behind_key=0, behind_area=0, behind_label=-1,
                   reach_key=int(ones), reach_cost=INT_MAX, reach_cell=-1)
        for name, want in pad.items():
            assert np.asarray(r[name][2]).tolist() == want, name
        assert [r[k].dtype for k in FC.WIDE] == [np.uint64] * 3
    # min_cells 2: the door is too small to be listed
    r = FC.reference(labels, seen, cols, since, None, here, (), min_cells=2, topk=2, rank_by=1)
    assert r["count"].tolist() == [1] and r["frontier"].tolist() == [32, -1] and r["counts"].tolist() == [5, 24, 19, 3, 2]


def test_reference_hand_worked_variants():
    labels, seen, cols, since, here = FC.hand_map()
    shut = labels.copy()
    shut[20] = 7                                                                 # the door shut by an object
    r = FC.reference(shut, seen, cols, since, None, here, (), min_cells=1, topk=2, rank_by=1)
    assert r["counts"].tolist() == [6, 23, 19, 2, 2] and r["count"].tolist() == [1] and r["frontier"].tolist() == [32, -1]
    assert r["behind_label"].tolist() == [40, -1] and r["unknown_area"][5] == 18
    base = FC.reference(labels, seen, cols, since, None, here, (), min_cells=1, topk=2, rank_by=1)
    r = FC.reference(shut, seen, cols, since, None, here, (7,), min_cells=1, topk=2, rank_by=1)       # ... which one can pass
    assert not FC.differences(r, base)
    r = FC.reference(labels, seen, cols, 1, None, here, (), min_cells=1, topk=2, rank_by=1)           # nothing is recent enough
    assert r["counts"].tolist() == [5, 0, 43, 0, 1] and r["count"].tolist() == [0] and r["frontier"].tolist() == [-1, -1]
    assert r["unknown_area"][0] == 43 and r["unknown_area"].sum() == 43 and set(r["unknown_labels"].tolist()) == {-1, 0}
    assert (r["frontier_labels"] == -1).all() and (r["reach_key"] == FC.ALL_ONES).all()
    # the cost of the way: a dist that cannot reach the door, then one that reaches nothing; no from_cell: cost 0, the lowest cell
    dist = np.full(48, 7, np.int32)
    dist[20] = INT_MAX
    dist[41] = 3
    r = FC.reference(labels, seen, cols, 0, dist, here, (), min_cells=1, topk=2, rank_by=0)
    assert r["reach_cost"].tolist() == [3, INT_MAX] and r["reach_cell"].tolist() == [41, -1] and r["reach_key"][1] == FC.ALL_ONES
    r = FC.reference(labels, seen, cols, 0, np.full(48, INT_MAX, np.int32), here, (), min_cells=1, topk=2, rank_by=0)
    assert r["reach_cost"].tolist() == [INT_MAX] * 2 and r["reach_cell"].tolist() == [-1, -1] and r["area"].tolist() == [2, 1]
    r = FC.reference(labels, seen, cols, 0, None, -1, (), min_cells=1, topk=2, rank_by=0)
    assert r["reach_cost"].tolist() == [0, 0] and r["reach_cell"].tolist() == [32, 20]


def test_cover_reference():
    seen = np.full(10, -1, np.int32)
    got = FC.cover_reference([[3, 3, -1], [10, 9, 4]], seen, 2, exclude_cell=4)
    assert got.tolist() == [-1, -1, -1, 2, -1, -1, -1, -1, -1, 2] and seen.tolist() == [-1] * 10
    assert FC.cover_reference([3, 0], got, 1).tolist() == [1, -1, -1, 2, -1, -1, -1, -1, -1, 2]       # an older stamp lowers nothing


def test_reference_mirror_and_transpose_identities():
    """Labels move with the lowest cell, so the kinds, the sorted areas of both planes, the counts and the ranked areas are
    compared."""
    rows, cols = 13, 21
    for name, m in FC.maps(rows, cols).items():
        lab, seen = m["labels"].reshape(rows, cols), m["last_seen"].reshape(rows, cols)
        base = FC.reference(lab.reshape(-1), seen.reshape(-1), cols, 1, None, -1, (2,), min_cells=1, topk=64, rank_by=0)
        kind = FC.kinds(lab, seen, 1, (2,))

        def areas(r, key):
            if key == "unknown_area":
                return sorted(r[key][r[key] > 0].tolist())
            return sorted(np.bincount(r[key][r[key] >= 0]).tolist())
        for tag, f, c2 in (("mirror rows", lambda a: a[::-1], cols), ("mirror cols", lambda a: a[:, ::-1], cols),
                           ("transpose", lambda a: a.T, rows)):
            l2, s2 = np.ascontiguousarray(f(lab)), np.ascontiguousarray(f(seen))
            r = FC.reference(l2.reshape(-1), s2.reshape(-1), c2, 1, None, -1, (2,), min_cells=1, topk=64, rank_by=0)
            assert np.array_equal(FC.kinds(l2, s2, 1, (2,)), f(kind)), (name, tag)
            assert r["counts"].tolist() == base["counts"].tolist() and r["count"].tolist() == base["count"].tolist(), (name, tag)
            assert areas(r, "unknown_area") == areas(base, "unknown_area"), (name, tag)
            assert [a for a in areas(r, "frontier_labels") if a] == [a for a in areas(base, "frontier_labels") if a], (name, tag)
            assert r["area"].tolist() == base["area"].tolist(), (name, tag)      # ranked by area: the same areas in the same order
            assert np.array_equal((r["frontier_labels"] >= 0).reshape(l2.shape), f((base["frontier_labels"] >= 0).reshape(rows, cols)))
            assert np.array_equal((r["unknown_labels"] >= 0).reshape(l2.shape), f((base["unknown_labels"] >= 0).reshape(rows, cols)))


def test_reference_is_quick_enough():
    for rows, cols in ((96, 96), (64, 65)):
        for name, m in FC.maps(rows, cols).items():
            t = time.perf_counter()
            FC.reference(m["labels"], m["last_seen"], cols, 0, None, 5, (2,), 1, 64, 1)
            assert time.perf_counter() - t < 2.0, (rows, cols, name)


def test_maps_hold_the_cases_they_name():
    r = FC.reference(*FC.serpentine(96, 96), 96, min_cells=1, topk=4)
    assert r["count"].tolist() == [1] and r["area"][0] > 96 * 47 and r["bbox"][0].tolist() == [0, 0, 95, 95]      # one frontier, every tile
    assert r["counts"][4] == 48
    r = FC.reference(*FC.checkerboard(40, 40), 40, min_cells=1, topk=64, rank_by=0)
    assert r["count"].tolist() == [400] and (r["area"] == 1).all() and (r["behind_area"] == 1200).all()              # ties in both keys
    assert r["frontier"].tolist() == [2 * (k % 20) + 80 * (k // 20) for k in range(64)]                              # the lowest labels
    for rows, cols, n in ((33, 33, 1), (64, 65, 2)):
        lab, seen, gadgets = FC.corner_map(rows, cols)
        assert len(gadgets) == n
        r = FC.reference(lab, seen, cols, 0, None, -1, (2,), min_cells=1, topk=64, rank_by=0)
        for a, b, u, w, anti in gadgets:
            ia, ib, iu, iw = (x[0] * cols + x[1] for x in (a, b, u, w))
            assert a[0] // FC.TILE != b[0] // FC.TILE and a[1] // FC.TILE != b[1] // FC.TILE                       # across the corner
            assert r["frontier_labels"][ia] == r["frontier_labels"][ib] == min(ia, ib)
            assert (r["frontier_labels"] == min(ia, ib)).sum() == 2
            assert r["unknown_labels"][iu] == iu and r["unknown_labels"][iw] == iw and r["unknown_area"][iu] == r["unknown_area"][iw] == 1


def test_frontier_header_and_ctypes_table_agree():
    import os
    import re
    import shutil
    import subprocess
    import tempfile
    import __graft_entry__
    __graft_entry__.build()
    from embodied_object_detection_amd import _lib, build, ops
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    path = os.path.join(root, "include", "eod_frontier.h")
    txt = open(path).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    declared = sorted(set(re.findall(r"^(?:int|size_t)\s+(eod_\w+)\s*\(", code, flags=re.M)))
    assert declared == sorted(_lib.FRONTIER_SIGNATURES) == ["eod_map_cover", "eod_map_frontier", "eod_map_frontier_workspace_bytes"]
    others = (set(_lib.SIGNATURES) | set(_lib.PLACE_SIGNATURES) | set(_lib.REGIONS_SIGNATURES) | set(_lib.INVENTORY_SIGNATURES)
              | set(_lib.DESCRIBE_SIGNATURES) | set(_lib.RELATIONS_SIGNATURES) | set(_lib.ROUTE_SIGNATURES) | set(_lib.CLEARANCE_SIGNATURES)
              | set(_lib.SIGHT_SIGNATURES))
    assert not set(_lib.FRONTIER_SIGNATURES) & others
    for name, n in (("eod_map_cover", 7), ("eod_map_frontier", 32), ("eod_map_frontier_workspace_bytes", 2)):
        res, args = _lib.FRONTIER_SIGNATURES[name]
        params = re.search(rf"\b{name}\s*\(([^)]*)\)", code, flags=re.S).group(1)
        assert len(params.split(",")) == len(args) == n, name
    lib = _lib.load()
    for name, (res, args) in _lib.FRONTIER_SIGNATURES.items():
        fn = getattr(lib, name)                                                  # exported by the library built for gfx950
        assert fn.restype is res and list(fn.argtypes) == list(args), name
    val = lambda name: int(re.search(rf"#define {name} (\d+)", txt).group(1))
    assert (ops.FRONTIER_P_MAX, ops.FRONTIER_TOPK_MAX, ops.FRONTIER_N_MAX, ops.FRONTIER_DIM_MAX, ops.FRONTIER_PIXELS_MAX) == (
        val("EOD_FRONTIER_P_MAX"), val("EOD_FRONTIER_TOPK_MAX"), val("EOD_FRONTIER_N_MAX"), val("EOD_FRONTIER_DIM_MAX"),
        val("EOD_FRONTIER_PIXELS_MAX")) == (64, 64, 2 ** 22, 32767, 2 ** 24)
    assert (ops.FRONTIER_N_MAX, ops.FRONTIER_DIM_MAX) == (ops.SIGHT_N_MAX, ops.SIGHT_DIM_MAX)
    assert "frontier.hip" in build.SOURCES
    for said in ("counts = 5, 24, 19, 3, 2", "6, 23, 19, 2, 2", "43 cells with label 0", "....#???  ....#???  .....???", "behind 18 / 5"):
        assert said in txt, said
    for rows, cols in ((1, 1), (200, 200), (70, 67), (32767, 128), (1, 32767)):
        N = rows * cols
        need = lib.eod_map_frontier_workspace_bytes(N, cols)
        assert need >= 29 * N + 4 and need % 8 == 0 and need == 4 * ops.map_frontier_workspace(N, cols)
    for N, cols in ((0, 1), (10, 3), (2 ** 22 + 1, 1), (32768, 1), (32768, 32768), (-4, 2), (4, 0)):
        assert lib.eod_map_frontier_workspace_bytes(N, cols) == 0
    with pytest.raises(_lib.EodError, match="map_frontier_workspace"):
        ops.map_frontier_workspace(10, 3)
    cc = next((p for p in (shutil.which(n) for n in ("gcc", "cc", "clang")) if p), None)
    assert cc is not None, "no C compiler (gcc, cc, clang) on PATH: the header cannot be checked as C"
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "t.c")
        open(c, "w").write(f'#include "{path}"\nint main(void) {{ return EOD_FRONTIER_TOPK_MAX == 64 ? 0 : 1; }}\n')
        subprocess.run([cc, "-std=c11", "-Wall", "-Werror", "-o", os.path.join(d, "t"), c], check=True)
        assert subprocess.run([os.path.join(d, "t")]).returncode == 0


def test_frontier_kernels_use_no_scratch():
    import __graft_entry__
    __graft_entry__.build()
    from embodied_object_detection_amd import build
    usage = build.resource_usage()
    if not any("frontier_" in k for k in usage):        # a library built elsewhere, without the remarks: build them here
        build.build(force=True, verbose=False)
        usage = build.resource_usage()
    mine = {k: v for k, v in usage.items() if "frontier_" in k}
    names = ("cover", "classify", "tile", "border", "behind", "select", "stats", "finish")
    assert sorted(n for k in mine for n in names if f"frontier_{n}_kernel" in k) == sorted(names), sorted(mine)
    assert not [k for k in build.scratch_offenders(usage) if "frontier_" in k]
    assert all(v.get("scratch", 0) == 0 for v in mine.values())


def test_entry_points_refuse_bad_arguments_before_any_launch():
    import ctypes as C
    import __graft_entry__
    __graft_entry__.build()
    from embodied_object_detection_amd import _lib
    lib = _lib.load()
    buf = (C.c_int64 * 4096)()
    p = C.addressof(buf)
    p += (-p) % 16
    BAD, ALIGN, NULL, CAPACITY = -1, -2, -4, -5

    def cover(proj=p, P=10, N=100, stamp=0, exclude_cell=-1, last_seen=p):
        return lib.eod_map_cover(proj, P, N, stamp, exclude_cell, last_seen, None)
    for kw in (dict(P=-1), dict(P=2 ** 24 + 1), dict(N=0), dict(N=-3), dict(N=2 ** 22 + 1), dict(stamp=-1), dict(stamp=-2 ** 31)):
        assert cover(**kw) == BAD, kw
    assert cover(stamp=-1, proj=None) == BAD and cover(N=0, last_seen=p + 1) == BAD           # a bad dimension wins
    assert cover(proj=None) == NULL and cover(last_seen=None) == NULL and cover(proj=None, last_seen=p + 2) == NULL
    assert cover(proj=p + 2) == ALIGN and cover(last_seen=p + 1) == ALIGN
    assert cover(P=0, proj=None) == 0 and cover(P=0) == 0                                       # no pixel: nothing is queued
    assert cover(P=0, proj=None, last_seen=None) == NULL

    ptrs = ("labels", "passable", "last_seen", "dist", "frontier_labels", "unknown_labels", "unknown_area", "count", "frontier", "area",
            "bbox", "sum_rc", "open_edges", "behind_key", "behind_area", "behind_label", "reach_key", "reach_cost", "reach_cell",
            "counts", "status", "workspace")

    def call(N=100, P=2, cols=10, since=0, from_cell=5, min_cells=1, topk=4, rank_by=1, workspace_bytes=2048, **kw):
        a = {name: p for name in ptrs}
        a.update(kw)
        return lib.eod_map_frontier(a["labels"], a["passable"], a["last_seen"], a["dist"], N, P, cols, since, from_cell, min_cells, topk,
                                    rank_by, *[a[n] for n in ptrs[4:]], workspace_bytes, None)

    for kw in (dict(P=-1), dict(P=65), dict(N=0), dict(N=2 ** 22 + 1), dict(N=-5), dict(cols=0), dict(cols=-10), dict(cols=7),
               dict(cols=101), dict(N=32768, cols=32768), dict(N=32768, cols=1), dict(N=2 ** 22, cols=2 ** 22), dict(N=2 ** 22, cols=64),
               dict(from_cell=-2), dict(from_cell=100), dict(from_cell=2 ** 31 - 1), dict(min_cells=0), dict(min_cells=-1), dict(topk=0),
               dict(topk=65), dict(topk=-1), dict(rank_by=2), dict(rank_by=-1)):
        assert call(**kw) == BAD, kw
    none = {name: None for name in ptrs}
    assert call(topk=0, **none) == BAD                                           # a bad dimension wins over a null pointer
    assert call(rank_by=3, reach_key=p + 4) == BAD                               # and over alignment
    assert call(min_cells=0, workspace_bytes=0) == BAD                           # and over the workspace
    for name in ptrs:
        if name == "dist":
            continue
        assert call(**{name: None}) == NULL, name
        assert call(**{name: None, "reach_key" if name != "reach_key" else "workspace": p + 4}) == NULL, name     # null wins over alignment
        assert call(workspace_bytes=0, **{name: None}) == NULL, name                                              # and over the workspace
    assert call(dist=None, workspace_bytes=0) == CAPACITY                        # dist may be null
    assert call(P=0, passable=None, workspace_bytes=0) == CAPACITY               # passable too, without passable labels
    for name in ptrs:
        wide = name in ("sum_rc", "behind_key", "reach_key", "workspace")
        for off in ((4, 1) if wide else (2, 1)):
            assert call(**{name: p + off}) == ALIGN, (name, off)
            assert call(workspace_bytes=0, **{name: p + off}) == ALIGN, (name, off)     # alignment wins over the workspace
    need = lib.eod_map_frontier_workspace_bytes(100, 10)
    assert need == 2048 + 256 + 1024 + 256
    for short in (0, 8, need - 1):
        assert call(workspace_bytes=short) == CAPACITY, short
    assert call(since=-2 ** 31, from_cell=-1, min_cells=2 ** 31 - 1, topk=64, P=64, rank_by=0, workspace_bytes=need - 1) == CAPACITY
    assert call(since=2 ** 31 - 1, from_cell=99, workspace_bytes=need - 1) == CAPACITY          # the largest values pass the first check


def test_ops_refuse_on_the_host_naming_the_argument():
    import torch
    import __graft_entry__
    __graft_entry__.build()
    from embodied_object_detection_amd import _lib, ops
    labels, seen = torch.zeros((120,), dtype=torch.int32), torch.zeros((120,), dtype=torch.int32)
    for bad in (torch.zeros((0,), dtype=torch.int32), torch.zeros((120,), dtype=torch.int64), torch.zeros((12, 10), dtype=torch.int32),
                torch.zeros((240,), dtype=torch.int32)[::2], torch.zeros((120,)), np.zeros(120, np.int32)):
        with pytest.raises(_lib.EodError, match="object_labels"):
            ops.map_frontier(bad, seen, 10)
    with pytest.raises(_lib.EodError, match="object_labels: N 4194305"):
        ops.map_frontier(torch.empty((2 ** 22 + 1,), dtype=torch.int32, device="meta"), seen, 1)
    for bad in (torch.zeros((119,), dtype=torch.int32), torch.zeros((120,), dtype=torch.int64), torch.zeros((240,), dtype=torch.int32)[::2],
                torch.zeros((120,), dtype=torch.int32, device="meta"), None, [0] * 120):
        with pytest.raises(_lib.EodError, match="last_seen"):
            ops.map_frontier(labels, bad, 10)
    for bad in (torch.zeros((119,), dtype=torch.int32), torch.zeros((120,), dtype=torch.int64), torch.zeros((120,)), [0] * 120,
                torch.zeros((120,), dtype=torch.int32, device="meta")):
        with pytest.raises(_lib.EodError, match="dist"):
            ops.map_frontier(labels, seen, 10, dist=bad)
    for bad in (0, -10, 7, 121, 2.5, True, None):
        with pytest.raises(_lib.EodError, match="cols"):
            ops.map_frontier(labels, seen, bad)
    big = torch.zeros((32768,), dtype=torch.int32)
    with pytest.raises(_lib.EodError, match="cols"):
        ops.map_frontier(big, big, 1)                                            # 32768 rows
    for name, bads in (("since", (2 ** 31, -2 ** 31 - 1, 1.0, None, True)), ("from_cell", (-2, 120, 2 ** 40, 0.5, True)),
                       ("min_cells", (0, -1, 1.5, None, 2 ** 31)), ("topk", (0, 65, -1, 2.0, None)),
                       ("rank_by", (2, -1, "size", None, 1.0, True))):
        for bad in bads:
            with pytest.raises(_lib.EodError, match=name):
                ops.map_frontier(labels, seen, 10, **{name: bad})
    for bad in (torch.zeros((65,), dtype=torch.int32), torch.zeros((3,), dtype=torch.int64), torch.zeros((2, 2), dtype=torch.int32),
                torch.zeros((4,), dtype=torch.int32, device="meta"), 7, ["a"], list(range(65))):
        with pytest.raises(_lib.EodError, match="passable"):
            ops.map_frontier(labels, seen, 10, passable=bad)
    for kw in (dict(), dict(since=-5, dist=seen, from_cell=119, passable=[3, 4], min_cells=1, topk=64, rank_by="area"),
               dict(from_cell=None, rank_by=0, passable=torch.tensor([1], dtype=torch.int32))):
        with pytest.raises(_lib.EodError, match="map_frontier: object_labels on the host .no CPU fallback"):       # refused last
            ops.map_frontier(labels, seen, 10, **kw)
    proj = torch.zeros((4, 5), dtype=torch.int32)
    for bad in (torch.zeros((4, 5), dtype=torch.int64), torch.zeros((4, 10), dtype=torch.int32)[:, ::2], np.zeros(4, np.int32), None):
        with pytest.raises(_lib.EodError, match="proj_indices"):
            ops.map_cover(bad, seen, 0)
    for bad in (torch.zeros((120,), dtype=torch.int64), torch.zeros((12, 10), dtype=torch.int32), torch.zeros((0,), dtype=torch.int32),
                torch.zeros((120,), dtype=torch.int32, device="meta"), None):
        with pytest.raises(_lib.EodError, match="last_seen|cells"):
            ops.map_cover(proj, bad, 0)
    for bad in (-1, 2 ** 31, 1.0, None, True):
        with pytest.raises(_lib.EodError, match="stamp"):
            ops.map_cover(proj, seen, bad)
    for bad in (2 ** 31, 0.5, None):
        with pytest.raises(_lib.EodError, match="exclude_cell"):
            ops.map_cover(proj, seen, 0, exclude_cell=bad)
    with pytest.raises(_lib.EodError, match="map_cover: last_seen on the host .no CPU fallback"):
        ops.map_cover(proj, seen, 3, exclude_cell=7)
    assert (seen == 0).all()


def test_model_surfaces_refuse_host_tensors_and_say_what_they_take():
    import torch
    import __graft_entry__
    __graft_entry__.build()
    from embodied_object_detection_amd import _lib
    from embodied_object_detection_amd.data.robot import RobotFrontEnd
    from embodied_object_detection_amd.engine.predictor import EmbodiedPredictor
    from embodied_object_detection_amd.modeling.lockstep import LockstepScenes
    from embodied_object_detection_amd.modeling.meta_arch import CustomRCNNRecurrent, _frontiers
    labels, seen = torch.zeros((120,), dtype=torch.int32), torch.zeros((120,), dtype=torch.int32)
    with pytest.raises(_lib.EodError, match="frontiers: map_shape"):
        _frontiers(labels, None, seen)
    with pytest.raises(_lib.EodError, match="frontiers: map_shape"):
        _frontiers(labels, (11, 10), seen)
    with pytest.raises(_lib.EodError, match="frontiers: object_labels on the host .no CPU fallback"):
        _frontiers(labels, (12, 10), seen, from_cell=3, route=dict(dist=seen), passable=[1])
    bare = CustomRCNNRecurrent.__new__(CustomRCNNRecurrent)
    bare.implicit_memory = bare.observations = bare._last_seen = None
    with pytest.raises(_lib.EodError, match="cover: no memory yet"):
        bare.cover(np.zeros((4, 4), np.int32))
    with pytest.raises(_lib.EodError, match="frontiers: object_labels on the host"):
        bare.frontiers(labels, (12, 10), last_seen=seen)
    for cls in (CustomRCNNRecurrent, LockstepScenes, EmbodiedPredictor):
        assert "last_seen" in cls.frontiers.__doc__ and callable(cls.cover) and cls.cover.__doc__
    doc = CustomRCNNRecurrent.frontiers.__doc__
    assert "observations > 0" in doc and "weaker record" in doc and "reach_cell" in doc and "route_metres" in doc
    assert "reach_cell" in RobotFrontEnd.cell_centers.__doc__ and "reach_cost" in RobotFrontEnd.route_metres.__doc__
    assert "reach_cost" in RobotFrontEnd.relation_metres.__doc__
