"""The obstacles on the map without a GPU: the numpy reference of `_obstacle_cases.py` on the two hand-worked examples of
include/eod_obstacles.h, every output by hand; its symmetries; the header against the ctypes table and the cross-compiled library;
every argument the entry points, the ops and the model surfaces refuse before any launch; and the robot front end's frame, which
keeps today's keys unless heights are asked for."""
import time

import numpy as np
import pytest

import _obstacle_cases as OC

INT_MAX, INT_MIN = OC.INT_MAX, OC.INT_MIN


def test_reference_hand_worked_record():
    proj, y, N, band, ex, want = OC.hand_record()
    assert (N, band, ex) == (6, (100, 1500), 5) and proj.size == 15
    assert OC.millimetres(y[[0, 1, 2, 3, 4, 5, 6, 7, 14]]).tolist() == [0, -250, 500, 1250, 2000, 62, 100, 1501, 1500]
    rec = OC.heights_reference(proj, y, OC.new_record(N), band, ex)
    assert rec.dtype == np.int32 and rec.shape == (4, 6)
    assert rec[0].tolist() == [2, 3, 3, 0, 1, 0] and rec[1].tolist() == [0, 2, 1, 0, 1, 0]
    assert rec[2].tolist() == [-250, 500, 62, INT_MAX, 1500, INT_MAX] and rec[3].tolist() == [0, 2000, 1501, INT_MIN, 1500, INT_MIN]
    assert rec.T.tolist() == [list(w) for w in want] and rec[0].sum() == 15 - 6              # six pixels are dropped
    # the band is tested after the rounding, both edges inside; without the exclusion cell 5 takes its pixel
    assert OC.heights_reference(proj, y, OC.new_record(N), (101, 1499), ex)[1].tolist() == [0, 2, 0, 0, 0, 0]
    assert OC.heights_reference(proj, y, OC.new_record(N), (62, 100), ex)[1].tolist() == [0, 0, 2, 0, 0, 0]
    assert OC.heights_reference(proj, y, OC.new_record(N), band, -1).T.tolist()[5] == [1, 1, 500, 500]
    # the order of the pixels and the split over calls do not matter; a record that holds data is extended
    perm = np.random.default_rng(0).permutation(15)
    assert np.array_equal(OC.heights_reference(proj[perm], y[perm], OC.new_record(N), band, ex), rec)
    part = OC.heights_reference(proj[:7], y[:7], OC.new_record(N), band, ex)
    assert np.array_equal(OC.heights_reference(proj[7:], y[7:], part, band, ex), rec)
    twice = OC.heights_reference(proj, y, rec, band, ex)
    assert twice[0].tolist() == [4, 6, 6, 0, 2, 0] and np.array_equal(twice[2:], rec[2:])


def test_reference_hand_worked_map():
    rec, cols, labels, min_hits, min_cells = OC.hand_map()
    assert (cols, min_hits, min_cells) == (6, 2, 2) and rec.shape == (4, 24)
    r = OC.reference(rec, cols, labels, (13,), min_hits, min_cells, topk=3)
    rows = ["".join("?.#O"[k] for k in row) for row in r["kind"].reshape(4, 6)]
    assert rows == ["##..??", "..#.??", ".OO.#?", ".....?"]
    assert r["counts"].tolist() == [6, 12, 4, 2, 2, 1] and r["count"].tolist() == [1] and r["status"].tolist() == [0, 0]
    sl = np.full(24, -1)
    sl[[0, 1, 8]] = 0
    sl[16] = 16
    assert r["structure_labels"].tolist() == sl.tolist()
    ml = np.full(24, -1)
    ml[[0, 1, 8]] = 0
    ml[[13, 14]] = 13
    assert r["merged_labels"].tolist() == ml.tolist()
    assert r["structure"].tolist() == [0, -1, -1] and r["area"].tolist() == [3, 0, 0]
    assert r["bbox"].tolist() == [[0, 0, 1, 2], [0, 0, 0, 0], [0, 0, 0, 0]] and r["sum_rc"].tolist() == [[1, 3], [0, 0], [0, 0]]
    assert r["top_mm"].tolist() == [max(rec[3][[0, 1, 8]]), INT_MIN, INT_MIN] and r["top_mm"][0] == 780
    assert r["sum_rc"].dtype == np.uint64 and r["kind"].dtype == np.uint8
    assert (r["obj_cells"].tolist(), r["obj_seen_cells"].tolist()) == ([2], [1])
    assert (r["obj_top_mm"].tolist(), r["obj_base_mm"].tolist()) == ([int(rec[3][13])], [int(rec[2][13])])      # from cell 13 alone
    # the object-slot rule: the lowest slot that holds the label; a negative slot and a later duplicate hold nothing
    r = OC.reference(rec, cols, labels, (-1, 13, 13, 7), min_hits, min_cells, topk=1)
    assert r["obj_cells"].tolist() == [0, 2, 0, 0] and r["obj_top_mm"].tolist() == [INT_MIN, 830, INT_MIN, INT_MIN]
    assert r["obj_base_mm"].tolist() == [INT_MAX, 23, INT_MAX, INT_MAX]
    # min_cells 1: no speck
    r = OC.reference(rec, cols, labels, (), min_hits, 1, topk=3)
    assert r["count"].tolist() == [2] and r["counts"].tolist() == [6, 12, 4, 2, 2, 0] and r["merged_labels"][16] == 16
    assert r["structure"].tolist() == [0, 16, -1] and r["area"].tolist() == [3, 1, 0] and r["top_mm"][1] == rec[3][16]
    assert r["obj_cells"].shape == (0,)
    # without object_labels: 13 is an obstacle and joins {0, 1, 8} across the corner (1, 2)-(2, 1); 14 was never seen
    r = OC.reference(rec, cols, None, (13,), min_hits, min_cells, topk=2)
    assert r["counts"].tolist() == [7, 12, 5, 0, 2, 1] and r["count"].tolist() == [1] and r["kind"][13] == OC.OBSTACLE
    assert r["kind"][14] == OC.UNSEEN and r["area"].tolist() == [4, 0] and r["bbox"][0].tolist() == [0, 0, 2, 2]
    assert r["sum_rc"][0].tolist() == [3, 4] and r["merged_labels"][13] == 0 and r["obj_cells"].tolist() == [0]
    assert r["top_mm"][0] == 830
    # min_hits 1: the cell with one band hit counts, and joins {0, 1, 8} and, across a corner, the speck
    r = OC.reference(rec, cols, labels, (), 1, min_cells, topk=2)
    assert r["counts"].tolist() == [6, 11, 5, 2, 1, 0] and r["structure_labels"][[9, 16]].tolist() == [0, 0] and r["area"][0] == 5


def test_reference_mirror_and_transpose_identities():
    """Labels move with the lowest cell, so the kinds, the sorted areas, the counts and the ranked areas are compared."""
    rows, cols = 13, 21
    for name, m in OC.maps(rows, cols).items():
        rec = m["record"].reshape(4, rows, cols)
        lab = None if m["labels"] is None else (m["labels"] >= 0).astype(np.int32).reshape(rows, cols) - 1       # one label: 0
        base = OC.reference(m["record"], cols, None if lab is None else lab.reshape(-1), (), min_hits=4, min_cells=1, topk=64)
        for tag, f, c2 in (("mirror rows", lambda a: a[..., ::-1, :], cols), ("mirror cols", lambda a: a[..., ::-1], cols),
                           ("transpose", lambda a: np.swapaxes(a, -1, -2), rows)):
            r2 = np.ascontiguousarray(f(rec)).reshape(4, -1)
            l2 = None if lab is None else np.ascontiguousarray(f(lab)).reshape(-1)
            r = OC.reference(r2, c2, l2, (), min_hits=4, min_cells=1, topk=64)
            assert np.array_equal(r["kind"].reshape(f(rec[0]).shape), f(base["kind"].reshape(rows, cols))), (name, tag)
            assert r["counts"].tolist() == base["counts"].tolist() and r["count"].tolist() == base["count"].tolist(), (name, tag)
            areas = lambda o: sorted(np.bincount(o["structure_labels"][o["structure_labels"] >= 0]).tolist())
            assert [a for a in areas(r) if a] == [a for a in areas(base) if a], (name, tag)
            assert r["area"].tolist() == base["area"].tolist(), (name, tag)      # ranked by area: the same areas in the same order
            assert sorted(r["top_mm"].tolist()) == sorted(base["top_mm"].tolist()), (name, tag)


def test_reference_is_quick_enough_and_maps_hold_the_cases_they_name():
    for rows, cols in ((96, 96), (64, 65)):
        for name, m in OC.maps(rows, cols).items():
            t = time.perf_counter()
            OC.reference(m["record"], cols, m["labels"], m["objects"], 4, 1, 64)
            assert time.perf_counter() - t < 2.0, (rows, cols, name)
    for rows, cols in ((33, 33), (64, 65), (96, 96), (31, 97)):
        maps = OC.maps(rows, cols)
        N = rows * cols
        assert sorted(maps) == sorted(["all unseen", "all clear", "all obstacle", "wall with a door", "checkerboard", "spirals",
                                       "spirals, transposed", "random 0.1", "random 0.4", "random 0.7", "many structures", "specks only",
                                       "objects over obstacles"])
        ref = {k: OC.reference(m["record"], cols, m["labels"], m["objects"], 4, 2, 64) for k, m in maps.items()}
        assert ref["all unseen"]["counts"].tolist() == [N, 0, 0, 0, 0, 0] and ref["all clear"]["counts"].tolist() == [0, N, 0, 0, 0, 0]
        assert ref["all obstacle"]["counts"].tolist() == [0, 0, N, 0, 1, 0] and ref["all obstacle"]["area"][0] == N
        assert ref["wall with a door"]["count"][0] == 2 and ref["wall with a door"]["area"][:2].sum() == rows - 1
        assert ref["checkerboard"]["counts"][4] == 1 and ref["checkerboard"]["area"][0] == (N + 1) // 2      # one, through the corners
        for k in ("spirals", "spirals, transposed"):
            assert ref[k]["counts"][4] == 2 and ref[k]["area"][1] > 2 * min(rows, cols), k                   # two long arms
        assert ref["many structures"]["count"][0] > 64 and (ref["many structures"]["structure"] >= 0).all()
        assert ref["specks only"]["count"][0] == 0 and ref["specks only"]["counts"][5] == ref["specks only"]["counts"][2] > 0
        assert (ref["specks only"]["merged_labels"] == -1).all() and (ref["specks only"]["structure_labels"] >= 0).sum() > 0
        o, m = ref["objects over obstacles"], maps["objects over obstacles"]
        assert ((o["kind"] == OC.OBJECT) & (m["record"][1] >= 4)).any() and o["counts"][3] > 0                # objects over obstacles
        assert ((o["obj_cells"] > 0) & (o["obj_seen_cells"] == 0)).any()                                       # an object never seen
        assert (o["obj_cells"][3] == 0) and m["objects"][3] == m["objects"][0] and m["objects"][4] == -1      # a duplicate, a negative
        dens = [int(ref[f"random {d}"]["counts"][2]) for d in (0.1, 0.4, 0.7)]
        assert dens[0] < dens[1] < dens[2]
    # the label of an object and of a structure never meet: each is a cell of its own component
    o = OC.reference(maps["objects over obstacles"]["record"], cols, maps["objects over obstacles"]["labels"], (), 4, 1, 64)
    lab = o["merged_labels"]
    assert all(o["kind"][t] == (OC.OBJECT if t in set(maps["objects over obstacles"]["labels"].tolist()) else OC.OBSTACLE)
               for t in set(lab[lab >= 0].tolist()))


def test_obstacles_header_and_ctypes_table_agree():
    import os
    import re
    import shutil
    import subprocess
    import tempfile
    import __graft_entry__
    __graft_entry__.build()
    from embodied_object_detection_amd import _lib, build, ops
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    path = os.path.join(root, "include", "eod_obstacles.h")
    txt = open(path).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    declared = sorted(set(re.findall(r"^(?:int|size_t)\s+(eod_\w+)\s*\(", code, flags=re.M)))
    assert declared == sorted(_lib.OBSTACLES_SIGNATURES) == ["eod_map_heights", "eod_map_obstacles", "eod_map_obstacles_workspace_bytes"]
    others = (set(_lib.SIGNATURES) | set(_lib.PLACE_SIGNATURES) | set(_lib.REGIONS_SIGNATURES) | set(_lib.INVENTORY_SIGNATURES)
              | set(_lib.DESCRIBE_SIGNATURES) | set(_lib.RELATIONS_SIGNATURES) | set(_lib.ROUTE_SIGNATURES) | set(_lib.CLEARANCE_SIGNATURES)
              | set(_lib.SIGHT_SIGNATURES) | set(_lib.FRONTIER_SIGNATURES))
    assert not set(_lib.OBSTACLES_SIGNATURES) & others
    for name, n in (("eod_map_heights", 13), ("eod_map_obstacles", 30), ("eod_map_obstacles_workspace_bytes", 2)):
        res, args = _lib.OBSTACLES_SIGNATURES[name]
        params = re.search(rf"\b{name}\s*\(([^)]*)\)", code, flags=re.S).group(1)
        assert len(params.split(",")) == len(args) == n, name
        for decl, arg in zip(params.split(","), args):                           # pointers, ints and the size in the header's order
            want = _lib.C.c_void_p if "*" in decl or "eod_stream_t" in decl else _lib.C.c_size_t if "size_t" in decl else _lib.C.c_int
            assert arg is want, (name, decl)
    lib = _lib.load()
    for name, (res, args) in _lib.OBSTACLES_SIGNATURES.items():
        fn = getattr(lib, name)                                                  # exported by the library built for gfx950
        assert fn.restype is res and list(fn.argtypes) == list(args), name
    val = lambda name: int(re.search(rf"#define {name} (\d+)", txt).group(1))
    assert (ops.OBSTACLES_K_MAX, ops.OBSTACLES_TOPK_MAX, ops.OBSTACLES_N_MAX, ops.OBSTACLES_DIM_MAX, ops.OBSTACLES_PIXELS_MAX,
            ops.OBSTACLES_BAND_MAX) == (val("EOD_OBSTACLES_K_MAX"), val("EOD_OBSTACLES_TOPK_MAX"), val("EOD_OBSTACLES_N_MAX"),
                                        val("EOD_OBSTACLES_DIM_MAX"), val("EOD_OBSTACLES_PIXELS_MAX"), val("EOD_OBSTACLES_BAND_MAX")) == (
        64, 64, 2 ** 22, 32767, 2 ** 24, 10 ** 6)
    assert (ops.OBSTACLES_N_MAX, ops.OBSTACLES_DIM_MAX, ops.OBSTACLES_PIXELS_MAX) == (ops.FRONTIER_N_MAX, ops.FRONTIER_DIM_MAX,
                                                                                     ops.FRONTIER_PIXELS_MAX)
    assert ops.OBSTACLES_KINDS == {k: val(f"EOD_OBSTACLES_{k.upper()}") for k in ("unseen", "clear", "obstacle", "object")}
    assert ops.OBSTACLES_KINDS == dict(unseen=OC.UNSEEN, clear=OC.CLEAR, obstacle=OC.OBSTACLE, object=OC.OBJECT)
    assert ops.HEIGHT_RECORD_INIT == (0, 0, INT_MAX, INT_MIN)
    assert "obstacles.hip" in build.SOURCES
    for said in ("counts = 6, 12, 4, 2, 2, 1", "counts = 7, 12, 5, 0, 2, 1", "##..??   ..#.??   .OO.s?   .....?", "bbox 0 0 2 2, sum_rc 3 4",
                 "cell 2 (3, 1, 62, 1501)", "62.5 rounds to 62", "2^31 valid", "rintf(__fmul_rn(y, 1000.0f))"):
        assert said in txt, said
    for rows, cols in ((1, 1), (200, 200), (70, 67), (32767, 128), (1, 32767)):
        N = rows * cols
        need = lib.eod_map_obstacles_workspace_bytes(N, cols)
        assert need >= 12 * N + 4 and need % 8 == 0 and need == 4 * ops.map_obstacles_workspace(N, cols)
    for N, cols in ((0, 1), (10, 3), (2 ** 22 + 1, 1), (32768, 1), (32768, 32768), (-4, 2), (4, 0)):
        assert lib.eod_map_obstacles_workspace_bytes(N, cols) == 0
    with pytest.raises(_lib.EodError, match="map_obstacles_workspace"):
        ops.map_obstacles_workspace(10, 3)
    cc = next((p for p in (shutil.which(n) for n in ("gcc", "cc", "clang")) if p), None)
    assert cc is not None, "no C compiler (gcc, cc, clang) on PATH: the header cannot be checked as C"
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "t.c")
        open(c, "w").write(f'#include "{path}"\nint main(void) {{ return EOD_OBSTACLES_TOPK_MAX == 64 && EOD_OBSTACLES_OBJECT == 3 ? 0 : 1; }}\n')
        subprocess.run([cc, "-std=c11", "-Wall", "-Werror", "-o", os.path.join(d, "t"), c], check=True)
        assert subprocess.run([os.path.join(d, "t")]).returncode == 0


def test_obstacles_kernels_use_no_scratch():
    import __graft_entry__
    __graft_entry__.build()
    from embodied_object_detection_amd import build
    usage = build.resource_usage()
    if not any("obstacles_" in k for k in usage):       # a library built elsewhere, without the remarks: build them here
        build.build(force=True, verbose=False)
        usage = build.resource_usage()
    mine = {k: v for k, v in usage.items() if "obstacles_" in k or "heights_kernel" in k}
    names = ("heights_kernel", "obstacles_classify_kernel", "obstacles_tile_kernel", "obstacles_border_kernel", "obstacles_select_kernel",
             "obstacles_stats_kernel")
    assert sorted(n for k in mine for n in names if n in k) == sorted(names), sorted(mine)
    assert not [k for k in build.scratch_offenders(usage) if k in mine]
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

    hp = ("proj", "height", "hits", "band_hits", "h_min", "h_max")

    def heights(P=10, N=100, stride=1, lo=100, hi=1500, exclude_cell=-1, **kw):
        a = {name: p for name in hp}
        a.update(kw)
        return lib.eod_map_heights(a["proj"], a["height"], stride, P, N, lo, hi, exclude_cell, *[a[n] for n in hp[2:]], None)
    for kw in (dict(P=-1), dict(P=2 ** 24 + 1), dict(N=0), dict(N=-3), dict(N=2 ** 22 + 1), dict(stride=0), dict(stride=-3),
               dict(lo=1501), dict(lo=5, hi=4), dict(lo=-1000001), dict(hi=1000001), dict(lo=-2 ** 31, hi=2 ** 31 - 1)):
        assert heights(**kw) == BAD, kw
    assert heights(stride=0, proj=None) == BAD and heights(N=0, hits=p + 1) == BAD              # a bad dimension wins
    for name in hp:
        assert heights(**{name: None}) == NULL, name
        assert heights(**{name: None, "hits" if name != "hits" else "h_max": p + 2}) == NULL, name     # null wins over alignment
        for off in (2, 1):
            assert heights(**{name: p + off}) == ALIGN, (name, off)
    assert heights(P=0, proj=None, height=None) == 0 and heights(P=0) == 0                      # no pixel: nothing is queued
    assert heights(P=0, proj=None, height=None, h_min=None) == NULL
    assert heights(P=0, lo=-1000000, hi=1000000, stride=2 ** 31 - 1, exclude_cell=-2 ** 31) == 0 and heights(P=0, lo=7, hi=7) == 0

    ptrs = ("hits", "band_hits", "h_min", "h_max", "labels", "objects", "kind", "structure_labels", "merged_labels", "count", "structure",
            "area", "bbox", "sum_rc", "top_mm", "obj_cells", "obj_seen_cells", "obj_top_mm", "obj_base_mm", "counts", "status", "workspace")
    optional = ("labels",)
    with_objects = ("objects", "obj_cells", "obj_seen_cells", "obj_top_mm", "obj_base_mm")

    def call(N=100, cols=10, K_obj=2, min_hits=4, min_cells=2, topk=4, workspace_bytes=4096, **kw):
        a = {name: p for name in ptrs}
        a.update(kw)
        return lib.eod_map_obstacles(*[a[n] for n in ptrs[:6]], N, cols, K_obj, min_hits, min_cells, topk, *[a[n] for n in ptrs[6:]],
                                     workspace_bytes, None)

    for kw in (dict(N=0), dict(N=2 ** 22 + 1), dict(N=-5), dict(cols=0), dict(cols=-10), dict(cols=7), dict(cols=101),
               dict(N=32768, cols=32768), dict(N=32768, cols=1), dict(N=2 ** 22, cols=2 ** 22), dict(N=2 ** 22, cols=64), dict(K_obj=-1),
               dict(K_obj=65), dict(min_hits=0), dict(min_hits=-1), dict(min_cells=0), dict(min_cells=-1), dict(topk=0), dict(topk=65),
               dict(topk=-1)):
        assert call(**kw) == BAD, kw
    none = {name: None for name in ptrs}
    assert call(topk=0, **none) == BAD                                           # a bad dimension wins over a null pointer
    assert call(min_hits=0, sum_rc=p + 4) == BAD                                 # and over alignment
    assert call(min_cells=0, workspace_bytes=0) == BAD                           # and over the workspace
    for name in ptrs:
        if name in optional:
            continue
        assert call(**{name: None}) == NULL, name
        assert call(**{name: None, "sum_rc" if name != "sum_rc" else "workspace": p + 4}) == NULL, name       # null wins over alignment
        assert call(workspace_bytes=0, **{name: None}) == NULL, name                                          # and over the workspace
    assert call(labels=None, workspace_bytes=0) == CAPACITY                      # object_labels may be null
    assert call(K_obj=0, workspace_bytes=0, **{n: None for n in with_objects}) == CAPACITY      # the object slots too, without any
    assert call(K_obj=0, workspace_bytes=0, labels=None, objects=None) == CAPACITY
    for name in ptrs:
        if name == "kind":
            assert call(kind=p + 1, workspace_bytes=0) == CAPACITY               # bytes: any address
            continue
        wide = name in ("sum_rc", "workspace")
        for off in ((4, 1) if wide else (2, 1)):
            assert call(**{name: p + off}) == ALIGN, (name, off)
            assert call(workspace_bytes=0, **{name: p + off}) == ALIGN, (name, off)     # alignment wins over the workspace
    need = lib.eod_map_obstacles_workspace_bytes(100, 10)
    assert need == 1280 + 256
    for short in (0, 8, need - 1):
        assert call(workspace_bytes=short) == CAPACITY, short
    assert call(K_obj=64, min_hits=2 ** 31 - 1, min_cells=2 ** 31 - 1, topk=64, workspace_bytes=need - 1) == CAPACITY
    assert call(K_obj=0, min_hits=1, min_cells=1, topk=1, workspace_bytes=need - 1) == CAPACITY       # the edges pass the first check


def test_ops_refuse_on_the_host_naming_the_argument():
    import torch
    import __graft_entry__
    __graft_entry__.build()
    from embodied_object_detection_amd import _lib, ops
    i32 = lambda *shape, **kw: torch.zeros(shape, dtype=torch.int32, **kw)
    for bad in (0, -1, 2 ** 22 + 1, 2.0, None, True):
        with pytest.raises(_lib.EodError, match="n_cells"):
            ops.new_height_record(bad, "cpu")
    rec = ops.new_height_record(120, "cpu")
    assert rec.shape == (4, 120) and rec.dtype == torch.int32 and rec.is_contiguous()
    assert [rec[k].unique().tolist() for k in range(4)] == [[0], [0], [INT_MAX], [INT_MIN]]
    assert np.array_equal(rec.numpy(), OC.new_record(120))
    proj, y = i32(4, 5), torch.zeros((4, 5))
    for bad in (torch.zeros((4, 5), dtype=torch.int64), i32(4, 10)[:, ::2], np.zeros(4, np.int32), None):
        with pytest.raises(_lib.EodError, match="proj_indices"):
            ops.map_heights(bad, y, rec)
    for bad in (torch.zeros((4, 5), dtype=torch.float64), torch.zeros((4, 6)), torch.zeros((4, 5, 2)), torch.zeros((4, 5, 6))[:, :, ::2],
                torch.zeros((4, 10))[:, ::2], torch.zeros((4, 5), device="meta"), np.zeros((4, 5), np.float32), None, i32(4, 5)):
        with pytest.raises(_lib.EodError, match="heights"):
            ops.map_heights(proj, bad, rec)
    for bad in (i32(120), i32(3, 120), i32(4, 0), torch.zeros((4, 120), dtype=torch.int64), i32(4, 240)[:, ::2], i32(4, 120, device="meta"),
                None, np.zeros((4, 120), np.int32)):
        with pytest.raises(_lib.EodError, match="record"):
            ops.map_heights(proj, y, bad)
    with pytest.raises(_lib.EodError, match="record: N 4194305"):
        ops.map_heights(i32(2, device="meta"), torch.zeros((2,), device="meta"), torch.empty((4, 2 ** 22 + 1), dtype=torch.int32, device="meta"))
    with pytest.raises(_lib.EodError, match="pixels"):
        ops.map_heights(torch.empty((2 ** 24 + 1,), dtype=torch.int32, device="meta"), torch.empty((2 ** 24 + 1,), device="meta"),
                        i32(4, 8, device="meta"))
    for bad in ((1500, 100), (100,), (100, 1500, 3), (0.1, 1.5), (-1000001, 0), (0, 1000001), None, 100, (True, 5), ("a", "b")):
        with pytest.raises(_lib.EodError, match="band_mm"):
            ops.map_heights(proj, y, rec, band_mm=bad)
    for bad in (2 ** 31, 0.5, None, True):
        with pytest.raises(_lib.EodError, match="exclude_cell"):
            ops.map_heights(proj, y, rec, exclude_cell=bad)
    for kw in (dict(), dict(band_mm=(-5, 5), exclude_cell=7), dict(band_mm=[0, 0])):
        with pytest.raises(_lib.EodError, match="map_heights: record on the host .no CPU fallback"):       # refused last
            ops.map_heights(proj, y, rec, **kw)
    with pytest.raises(_lib.EodError, match="map_heights: record on the host"):
        ops.map_heights(proj, torch.zeros((4, 5, 3)), rec)                                                  # xyz passes the checks
    assert np.array_equal(rec.numpy(), OC.new_record(120))

    labels = i32(120)
    for bad in (i32(120), i32(3, 120), torch.zeros((4, 120), dtype=torch.int64), i32(4, 240)[:, ::2], None, np.zeros((4, 120), np.int32)):
        with pytest.raises(_lib.EodError, match="record"):
            ops.map_obstacles(bad, 10)
    for bad in (0, -10, 7, 121, 2.5, True, None):
        with pytest.raises(_lib.EodError, match="cols"):
            ops.map_obstacles(rec, bad)
    with pytest.raises(_lib.EodError, match="cols"):
        ops.map_obstacles(i32(4, 32768), 1)                                      # 32768 rows
    for bad in (i32(119), torch.zeros((120,), dtype=torch.int64), i32(240)[::2], i32(120, device="meta"), [0] * 120, i32(12, 10)):
        with pytest.raises(_lib.EodError, match="object_labels"):
            ops.map_obstacles(rec, 10, object_labels=bad)
    for bad in (i32(65), torch.zeros((3,), dtype=torch.int64), i32(2, 2), i32(4, device="meta"), 7, ["a"], list(range(65))):
        with pytest.raises(_lib.EodError, match="objects"):
            ops.map_obstacles(rec, 10, object_labels=labels, objects=bad)
    for name, bads in (("min_hits", (0, -1, 1.5, None, 2 ** 31, True)), ("min_cells", (0, -1, 1.5, None, 2 ** 31)),
                       ("topk", (0, 65, -1, 2.0, None))):
        for bad in bads:
            with pytest.raises(_lib.EodError, match=name):
                ops.map_obstacles(rec, 10, **{name: bad})
    for kw in (dict(), dict(object_labels=labels, objects=[3, 3, -1], min_hits=1, min_cells=1, topk=64),
               dict(objects=torch.tensor([1], dtype=torch.int32), topk=1)):
        with pytest.raises(_lib.EodError, match="map_obstacles: record on the host .no CPU fallback"):      # refused last
            ops.map_obstacles(rec, 10, **kw)


def test_model_surfaces_refuse_before_any_launch_and_say_what_they_take():
    import torch
    import __graft_entry__
    __graft_entry__.build()
    from embodied_object_detection_amd import _lib, ops
    from embodied_object_detection_amd.data.robot import RobotFrontEnd
    from embodied_object_detection_amd.engine.predictor import EmbodiedPredictor
    from embodied_object_detection_amd.modeling.lockstep import LockstepScenes
    from embodied_object_detection_amd.modeling.meta_arch import CustomRCNNRecurrent, _heights, _obstacles
    rec, labels = ops.new_height_record(120, "cpu"), torch.zeros((120,), dtype=torch.int32)
    with pytest.raises(_lib.EodError, match="obstacles: map_shape"):
        _obstacles(rec, None)
    with pytest.raises(_lib.EodError, match="obstacles: map_shape"):
        _obstacles(rec, (11, 10))
    with pytest.raises(_lib.EodError, match="obstacles: no height record"):
        _obstacles(None, (12, 10))
    with pytest.raises(_lib.EodError, match="obstacles: record on the host .no CPU fallback"):
        _obstacles(rec, (12, 10), labels, [3])
    with pytest.raises(_lib.EodError, match="heights: the frame carries no heights"):
        _heights(None, np.zeros((4, 4), np.int32), None, None, 16, (100, 1500), -1)
    bare = CustomRCNNRecurrent.__new__(CustomRCNNRecurrent)
    bare.implicit_memory = bare.observations = bare._height_record = None
    with pytest.raises(_lib.EodError, match="heights: no memory yet"):
        bare.heights(np.zeros((4, 4), np.int32), np.zeros((4, 4), np.float32))
    with pytest.raises(_lib.EodError, match="obstacles: no height record"):
        bare.obstacles(labels, None, (12, 10))
    with pytest.raises(_lib.EodError, match="obstacles: record on the host"):
        bare.obstacles(labels, None, (12, 10), record=rec)
    pred = EmbodiedPredictor.__new__(EmbodiedPredictor)
    pred.model = bare
    with pytest.raises(_lib.EodError, match='carries no "heights"'):
        pred.heights({"proj_indices": np.zeros((4, 4), np.int32)})
    with pytest.raises(_lib.EodError, match="heights: no memory yet"):
        pred.heights({"proj_indices": np.zeros((4, 4), np.int32), "heights": np.zeros((4, 4), np.float32)})
    ls = LockstepScenes.__new__(LockstepScenes)
    ls.B, ls.implicit_memory, ls._height_record = 2, None, None
    with pytest.raises(IndexError):
        ls.heights(2, None, None)
    with pytest.raises(_lib.EodError, match="heights: no memory yet"):
        ls.heights(1, np.zeros((4, 4), np.int32), np.zeros((4, 4), np.float32))
    with pytest.raises(_lib.EodError, match="obstacles: no height record"):
        ls.obstacles(map_shape=(12, 10))
    both = torch.stack([rec, rec])
    with pytest.raises(_lib.EodError, match="scene="):
        ls.obstacles(labels, None, (12, 10), record=both)
    with pytest.raises(_lib.EodError, match=r"expected \[B, 4, N\]"):
        ls.obstacles(torch.stack([labels] * 3), None, (12, 10), record=both)
    with pytest.raises(_lib.EodError, match=r"objects .*expected \[B, K\]"):
        ls.obstacles(torch.stack([labels] * 2), [1, 2, 3], (12, 10), record=both)
    with pytest.raises(_lib.EodError, match="obstacles: record on the host"):
        ls.obstacles(torch.stack([labels] * 2), [[1], [2]], (12, 10), record=both)
    for cls in (CustomRCNNRecurrent, LockstepScenes, EmbodiedPredictor):
        assert "merged_labels" in cls.obstacles.__doc__ and callable(cls.heights) and cls.heights.__doc__
    doc = CustomRCNNRecurrent.obstacles.__doc__
    assert 'model.route(inv["object"], obs["merged_labels"]' in doc and "obj_top_mm" in doc and "region_centroids" in doc
    for q in ("route", "clearance", "sight", "frontiers"):
        assert "`obstacles`" in getattr(CustomRCNNRecurrent, q).__doc__ and 'obs["merged_labels"]' in getattr(CustomRCNNRecurrent, q).__doc__
    assert "height_band_mm" in CustomRCNNRecurrent.heights.__doc__


def test_front_end_frame_keeps_its_keys_unless_heights_are_asked_for():
    from embodied_object_detection_amd.data.robot import RobotFrontEnd
    calls = []

    def plain(depth, T, intr, proj_shift, map_shift, cell, map_w, map_h, order=0):
        calls.append(order)
        return np.arange(depth.size, dtype=np.int32).reshape(depth.shape) % (map_w * map_h)

    def with_xyz(depth, T, intr, proj_shift, map_shift, cell, map_w, map_h, order=0, want_xyz=False):
        idx = plain(depth, T, intr, proj_shift, map_shift, cell, map_w, map_h, order)
        xyz = np.stack([depth * 2, depth + 0.25, depth * 3], axis=-1).astype(np.float32)
        return (idx, xyz) if want_xyz else idx
    with_xyz.returns_xyz = True
    rgb, depth = np.zeros((6, 8, 3), np.uint8), (np.arange(48, dtype=np.uint16).reshape(6, 8) * 100)
    today = ["file_name", "height", "image", "memory", "memory_reset", "observations", "proj_indices", "sequence_name", "width"]
    f = RobotFrontEnd(projector=plain).frame(rgb, depth, (0.0, 0.0, 0.0))
    assert sorted(f) == today and f["proj_indices"].shape == (6, 8, 1) and f["memory_reset"] is True
    assert sorted(RobotFrontEnd(projector=plain).frame(rgb, depth, (0.0, 0.0, 0.0), "a.png", heights=False)) == today
    with pytest.raises(ValueError, match="cannot return heights"):
        RobotFrontEnd(projector=plain).frame(rgb, depth, (0.0, 0.0, 0.0), heights=True)
    front = RobotFrontEnd(projector=with_xyz)
    g = front.frame(rgb, depth, (0.0, 0.0, 0.0), heights=True)
    assert sorted(g) == sorted(today + ["heights"]) and g["heights"].shape == (6, 8) and g["heights"].dtype == np.float32
    assert g["heights"].flags["C_CONTIGUOUS"] and np.array_equal(g["heights"], (depth.astype(np.float64) / 1000).astype(np.float32) + np.float32(0.25))
    assert np.array_equal(g["proj_indices"], f["proj_indices"]) and calls == [1, 1, 1]
    assert sorted(front.frame(rgb, depth, (0.0, 0.0, 0.0))) == today and front.frame(rgb, depth, (0.0, 0.0, 0.0))["memory_reset"] is False
    assert front.height_band_mm(0.1, 1.5) == (100, 1500) and front.height_band_mm(-0.25, 0.0005) == (-250, 0)
    assert front.height_band_mm(0.0994, 0.0996) == (99, 100)
    for bad in ((1.5, 0.1), (0.0, 1000.1), (-1000.1, 0.0)):
        with pytest.raises(ValueError, match="height_band_mm"):
            front.height_band_mm(*bad)
    from embodied_object_detection_amd.data import synthetic
    import inspect
    sig = inspect.signature(synthetic.hip_projector("cpu"))
    assert list(sig.parameters)[:9] == ["depth", "T", "intr", "proj_shift", "map_shift", "cell", "map_w", "map_h", "order"]
    assert sig.parameters["want_xyz"].default is False and synthetic.hip_projector("cpu").returns_xyz is True
