"""The host side of `map_regions` (no GPU): include/eod_regions.h against its ctypes table, the workspace formula, every refused
argument (the entry point returns before a launch, so it is callable here), the reference of `_regions_cases.py` on hand-worked
maps, what the hostile maps hold, and the robot front-end's centroids."""
import numpy as np
import pytest

import _regions_cases as RC


def _ref(grid, cols, conn, level=0.5, **kw):
    prob = np.asarray(grid, dtype=np.float32).reshape(1, -1)
    return {k: v[0] for k, v in RC.reference(prob, cols, level, conn, **kw).items()}


def test_reference_on_a_hand_worked_3_by_4_map():
    #   cells 0..11:   X . X X      4-connectivity: {0}, {2, 3, 7}, {5, 8, 9}
    #                  . X . X      8-connectivity: {0, 5, 2, 3, 7, 8, 9} is one component
    #                  X X . .
    g = [.9, 0, .6, .7,
         0, .8, 0, .5,
         .5, .6, 0, 0]
    r4 = _ref(g, 4, 4, topk=5)
    assert r4["region_labels"].tolist() == [0, -1, 2, 2, -1, 5, -1, 2, 5, 5, -1, -1]
    assert r4["count"] == 3 and r4["foreground"] == 7
    assert r4["region"].tolist() == [2, 5, 0, -1, -1] and r4["area"].tolist() == [3, 3, 1, 0, 0]         # area, then label
    assert r4["bbox"].tolist() == [[0, 2, 1, 3], [1, 0, 2, 1], [0, 0, 0, 0], [0, 0, 0, 0], [0, 0, 0, 0]]
    assert r4["sum_rc"].tolist() == [[1, 8], [5, 2], [0, 0], [0, 0], [0, 0]]
    assert r4["peak"].tolist() == [3, 5, 0, 0, 0]
    assert r4["peak_prob"].tolist() == [np.float32(.7), np.float32(.8), np.float32(.9), 0.0, 0.0]
    q24 = lambda *v: sum(int(np.float32(x) * np.float32(2 ** 24)) for x in v)
    assert r4["mass_q24"].tolist() == [q24(.6, .7, .5), q24(.8, .5, .6), q24(.9), 0, 0]
    r8 = _ref(g, 4, 8, topk=2)
    assert r8["region_labels"].tolist() == [0, -1, 0, 0, -1, 0, -1, 0, 0, 0, -1, -1]
    assert r8["count"] == 1 and r8["region"].tolist() == [0, -1] and r8["area"].tolist() == [7, 0]
    assert r8["bbox"][0].tolist() == [0, 0, 2, 3] and r8["sum_rc"][0].tolist() == [6, 10] and r8["peak"][0] == 0
    # min_cells drops the singletons from the count and from the ranking, not from the label map
    m2 = _ref(g, 4, 4, topk=5, min_cells=2)
    assert m2["count"] == 2 and m2["region"].tolist() == [2, 5, -1, -1, -1] and m2["region_labels"].tolist() == r4["region_labels"].tolist()


def test_reference_row_wrap_tie_and_edges():
    # (0, 2) and (1, 0) are neighbours in memory, not on the grid; neither are (1, 0) and (1, 2)
    g = [0, 0, 1,
         1, 0, 1 * 0,
         0, 0, 0]
    for conn in (4, 8):
        r = _ref(g, 3, conn)
        assert r["count"] == 2 and r["region"][:2].tolist() == [2, 3], conn
    r = _ref([1, 0, 1], 3, 8)
    assert r["count"] == 2
    # equal areas: the lower label first; the plateau's peak is its lowest cell
    g = [.5, .5, 0, .7, .7,
         0, 0, 0, 0, 0,
         .6, .6, 0, 0, 0]
    r = _ref(g, 5, 4, topk=4)
    assert r["region"].tolist() == [0, 3, 10, -1] and r["area"].tolist() == [2, 2, 2, 0] and r["peak"].tolist() == [0, 3, 10, 0]
    # the level: equal is in, the float below is out, a NaN is out; values above 1 count as 1 in the mass
    lv = np.float32(0.3)
    r = _ref([lv, np.nextafter(lv, np.float32(0)), np.nan, 1.5], 4, 8, level=0.3)
    assert r["region_labels"].tolist() == [0, -1, -1, 3] and r["foreground"] == 2
    assert r["mass_q24"][:2].tolist() == [int(lv * np.float32(2 ** 24)), 2 ** 24] and r["peak_prob"][1] == np.float32(1.5)


def test_hostile_maps_hold_what_their_names_say():
    rows, cols, tr, tc = 21, 37, 8, 16
    maps = RC.hostile_maps(rows, cols, tr, tc)
    assert len(maps) <= 32
    one = lambda name, conn, **kw: _ref(maps[name], cols, conn, **kw)
    s = one("serpentine", 4)
    assert s["count"] == 1 and s["region"][0] == 0 and s["area"][0] == s["foreground"] == 11 * cols + 10
    for conn in (4, 8):
        sp = one("spirals", conn)
        assert sp["count"] == 2 and sp["area"][1] > 20, (conn, sp["count"])
    assert one("checkerboard", 8)["count"] == 1
    cb = one("checkerboard", 4)
    assert cb["count"] == (rows * cols + 1) // 2 and cb["region"].tolist() == list(range(0, 32, 2)) and (cb["area"] == 1).all()
    for name in ("row-end pair", "row ends"):
        assert [one(name, c)["count"] for c in (4, 8)] == [2, 2], name
    for name in ("corner diagonal", "corner anti-diagonal"):
        assert [one(name, c)["count"] for c in (4, 8)] == [2, 1], name
    assert one("all foreground", 4)["area"][0] == rows * cols
    bg = one("all background", 8)
    assert bg["count"] == 0 and (bg["region"] == -1).all() and (bg["region_labels"] == -1).all() and not bg["sum_rc"].any()
    assert one("at the level", 8)["foreground"] > 300 and one("below the level", 8)["foreground"] == 0
    assert np.isnan(maps["nan"]).sum() > 30 and (one("nan", 8)["region_labels"][np.isnan(maps["nan"])] == -1).all()
    pl = one("plateau", 4)
    assert pl["count"] == 2 and pl["peak"][:2].tolist() == [2 * cols + 2, (rows - 2) * cols + cols - 3]
    ms = maps["mass"]
    assert (ms == 1.0).sum() > 20 and (ms > 1.0).sum() > 20
    m = one("mass", 8)
    assert 0 < m["mass_q24"][0] <= int(m["area"][0]) << 24


def test_robot_front_end_region_centroids():
    import torch
    from embodied_object_detection_amd.data.robot import RobotFrontEnd
    fe = RobotFrontEnd(projector=lambda *a: None, map_w=30, map_h=20, res=0.25, map_shift=(-3.0, 0.0, -2.0))
    # one cell: its centre; two cells of one row: between them; padding: NaN
    cells = [7 * 20 + 3, 7 * 20 + 4]
    sum_rc = np.array([[[7, 3], [14, 7], [0, 0]]], dtype=np.int64)
    area = np.array([[1, 2, 0]], dtype=np.int32)
    got = fe.region_centroids(sum_rc, area)
    assert got.dtype == np.float64 and got.shape == (1, 3, 2)
    assert tuple(got[0, 0]) == fe.cell_center(cells[0])
    a, b = fe.cell_center(cells[0]), fe.cell_center(cells[1])
    assert np.allclose(got[0, 1], [(a[0] + b[0]) / 2, (a[1] + b[1]) / 2], rtol=0, atol=1e-12)
    assert np.isnan(got[0, 2]).all()
    assert np.array_equal(fe.region_centroids(torch.from_numpy(sum_rc), torch.from_numpy(area)), got, equal_nan=True)
    with pytest.raises(ValueError):
        fe.region_centroids(sum_rc[0], area)


def test_regions_header_and_ctypes_table_agree():
    """include/eod_regions.h against `_lib.REGIONS_SIGNATURES`: the same entry points on both sides, every one exported by the
    library, none of them in the other two tables; the header's constants are the binding's."""
    import os
    import re
    import shutil
    import subprocess
    import tempfile
    import __graft_entry__
    __graft_entry__.build()
    from embodied_object_detection_amd import _lib, build, ops
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    path = os.path.join(root, "include", "eod_regions.h")
    txt = open(path).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    declared = sorted(set(re.findall(r"^(?:int|size_t)\s+(eod_\w+)\s*\(", code, flags=re.M)))
    assert declared == sorted(_lib.REGIONS_SIGNATURES) == ["eod_map_regions", "eod_map_regions_workspace_bytes"]
    assert not set(_lib.REGIONS_SIGNATURES) & (set(_lib.SIGNATURES) | set(_lib.PLACE_SIGNATURES))
    assert len(_lib.SIGNATURES) == 75 and len(_lib.PLACE_SIGNATURES) == 2
    for other in ("eod_hip.h", "eod_place.h"):
        assert "eod_map_regions" not in open(os.path.join(root, "include", other)).read()
    lib = _lib.load()
    for name, (res, args) in _lib.REGIONS_SIGNATURES.items():
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == list(args), name
    val = lambda name: int(re.search(rf"#define {name} (\d+)", txt).group(1))
    assert (ops.REGIONS_Q_MAX, ops.REGIONS_TOPK_MAX, ops.REGIONS_N_MAX, ops.REGIONS_TILE_ROWS, ops.REGIONS_TILE_COLS) == (
        val("EOD_REGIONS_Q_MAX"), val("EOD_REGIONS_TOPK_MAX"), val("EOD_REGIONS_N_MAX"), val("EOD_REGIONS_TILE_ROWS"),
        val("EOD_REGIONS_TILE_COLS")) and ops.REGIONS_N_MAX == 2 ** 22
    assert "regions.hip" in build.SOURCES
    gcc = shutil.which("gcc")                                                    # the header compiles as C on its own
    if gcc is not None:
        with tempfile.TemporaryDirectory() as d:
            src = os.path.join(d, "t.c")
            open(src, "w").write(f'#include "{path}"\nint main(void) {{ return EOD_REGIONS_OUT_WORDS(8, 16) == 2 + 16 + 14 * 128 ? 0 : 1; }}\n')
            subprocess.run([gcc, "-std=c11", "-Wall", "-Werror", "-o", os.path.join(d, "t"), src], check=True)
            assert subprocess.run([os.path.join(d, "t")]).returncode == 0


def test_entry_point_refuses_bad_arguments_before_any_launch():
    import ctypes as C
    import __graft_entry__
    __graft_entry__.build()
    from embodied_object_detection_amd import _lib, ops
    lib = _lib.load()
    buf = (C.c_int64 * 4096)()
    p = C.addressof(buf)
    BAD, ALIGN, NULL, CAP = -1, -2, -4, -5
    up256 = lambda v: (v + 255) // 256 * 256
    wsb = lib.eod_map_regions_workspace_bytes
    assert wsb(5, 437, 16) == up256(3 * 5 * 437 * 4) + 5 * 16 * 8                 # parent, area, slot; the peak keys
    assert wsb(8, 262144, 16) == 3 * 8 * 262144 * 4 + 8 * 16 * 8
    assert wsb(32, 2 ** 22, 64) == 3 * 32 * 2 ** 22 * 4 + 32 * 64 * 8             # beyond 2^31: a size_t
    assert ops.map_regions_workspace(5, 437, 16) == wsb(5, 437, 16) // 4
    for bad in ((0, 437, 16), (33, 437, 16), (5, 0, 16), (5, 2 ** 22 + 1, 16), (5, 437, 0), (5, 437, 65), (-1, -1, -1)):
        assert wsb(*bad) == 0, bad
        with pytest.raises(_lib.EodError):
            ops.map_regions_workspace(*bad)
    need = wsb(5, 437, 16)
    call = lambda prob=p, Q=5, N=437, cols=23, level=0.5, conn=8, min_cells=1, K=16, labels=p, out=p, ws=p, ws_bytes=need: (
        lib.eod_map_regions(prob, Q, N, cols, level, conn, min_cells, K, labels, out, ws, ws_bytes, None))
    for kw in (dict(Q=0), dict(Q=33), dict(Q=-1), dict(K=0), dict(K=65), dict(conn=6), dict(conn=0), dict(min_cells=0), dict(min_cells=-3),
               dict(cols=0), dict(cols=-23), dict(cols=20), dict(N=0), dict(N=2 ** 22 + 1, cols=1), dict(level=0.0), dict(level=-0.5),
               dict(level=float("nan")), dict(level=float("inf")), dict(level=1.0000001), dict(level=1e-50)):
        assert call(**kw) == BAD, kw
    # a bad dimension wins over everything a launch would need
    assert call(Q=0, prob=None, labels=None, out=None, ws=None, ws_bytes=0) == BAD
    for kw in (dict(prob=None), dict(labels=None), dict(out=None), dict(ws=None)):
        assert call(**kw) == NULL, kw
    for kw in (dict(prob=p + 2), dict(labels=p + 1), dict(out=p + 4), dict(ws=p + 4)):
        assert call(**kw) == ALIGN, kw
    assert call(ws_bytes=need - 1) == CAP and call(ws_bytes=0) == CAP
    assert call(N=2 ** 22, cols=2048, ws_bytes=need) == CAP                        # the largest N is a dimension it takes


def test_op_refuses_on_the_host_naming_the_argument():
    import torch
    import __graft_entry__
    __graft_entry__.build()
    from embodied_object_detection_amd import _lib, ops
    prob = torch.zeros((2, 12))
    ok = dict(cols=4, level=0.5)
    for name, kw in (("level", dict(level=0.0)), ("level", dict(level=float("nan"))), ("level", dict(level=1.5)), ("level", dict(level=1e-50)),
                     ("connectivity", dict(connectivity=6)), ("min_cells", dict(min_cells=0)), ("topk", dict(topk=0)),
                     ("topk", dict(topk=65)), ("cols", dict(cols=5)), ("cols", dict(cols=0))):
        with pytest.raises(_lib.EodError, match=name):
            ops.map_regions(prob, **{**ok, **kw})
    for bad in (torch.zeros((33, 12)), torch.zeros((0, 12)), torch.zeros((12,)), torch.zeros((2, 12), dtype=torch.float64),
                torch.zeros((12, 2)).t(), np.zeros((2, 12), np.float32)):
        with pytest.raises(_lib.EodError, match="prob"):
            ops.map_regions(bad, **ok)
    with pytest.raises(_lib.EodError, match="no CPU fallback"):
        ops.map_regions(prob, **ok)
