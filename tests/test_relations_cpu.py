"""The host side of `map_relations` (no GPU): the reference of `_relations_cases.py` on hand-worked maps, include/eod_relations.h
against its ctypes table and the cross-compiled library, the build's records, and every refused argument (the entry point returns
before a launch, so it is callable here)."""
import numpy as np
import pytest

import _relations_cases as LC

INT_MAX = LC.INT_MAX


def _grid(rows, cols, cells):
    g = np.full((rows, cols), -1, np.int32)
    for (r, c), v in cells.items():
        g[r, c] = v
    return g.reshape(-1)


def test_reference_lowest_slot_wins_a_duplicate():
    labels = np.array([5, 3, -1, 5, 9, INT_MAX, -7, 3], np.int32)
    assert LC.slots(labels, np.array([3, 5, 3, -1, 9], np.int32)).tolist() == [1, 0, -1, 1, 4, -1, -1, 0]
    assert LC.slots(labels, np.array([-1, -7, INT_MAX], np.int32)).tolist() == [-1, -1, -1, -1, -1, 2, -1, -1]       # -7 names nothing
    ref = LC.reference(labels, np.array([3, 5, 3, -1, 9], np.int32), cols=8, radius=1)
    assert ref["cells"].tolist() == [2, 2, 0, 0, 1]
    assert (ref["min_d2"][2] == INT_MAX).all() and (ref["min_d2"][:, 2] == INT_MAX).all() and not ref["near_cells"][2].any()
    assert ref["min_d2"][0, 1] == 1 and ref["closest"][0, 1] == 1 and ref["closest"][1, 0] == 0 and ref["edges"][0, 1] == 1
    assert ref["min_d2"][1, 4] == 1 and ref["closest"][1, 4] == 3 and ref["closest"][4, 1] == 4
    assert ref["pair_key"][0, 1] == np.uint64((1 << 32) | 1) and ref["pair_key"][0, 0] == LC.NONE and ref["pair_key"][0, 4] == LC.NONE


def test_reference_disc_and_not_square():
    labels = _grid(12, 12, {(2, 2): 1, (5, 6): 2, (6, 6): 3})          # offsets (3, 4) and (4, 4) from the cell of 1
    ref = LC.reference(labels, np.array([1, 2, 3], np.int32), cols=12, radius=5)
    assert ref["min_d2"][0].tolist() == [INT_MAX, 25, INT_MAX] and ref["near_cells"][0].tolist() == [0, 1, 0]
    assert ref["min_d2"][1, 2] == 1 and ref["edges"][1, 2] == 1 and ref["edges"][0, 1] == 0
    assert ref["nearest"][0].tolist() == [1, -1, -1, -1] and ref["nearest_d2"][0].tolist() == [25, INT_MAX, INT_MAX, INT_MAX]
    assert len(LC.disc(16)) == 796 and len(LC.disc(1)) == 4 and len(LC.disc(5)) == 80


def test_reference_ties_lowest_cell_and_lower_slot():
    # the cell of 2 is one step from two cells of 1: the lowest cell is the closest; 3 and 4 are equally far from 2
    labels = _grid(5, 7, {(1, 3): 1, (2, 2): 1, (2, 3): 2, (2, 5): 4, (4, 3): 3})
    ref = LC.reference(labels, np.array([1, 2, 4, 3], np.int32), cols=7, radius=2, topn=8)
    assert ref["closest"][0, 1] == 1 * 7 + 3 and ref["min_d2"][0, 1] == 1 and ref["edges"][0, 1] == 2 and ref["near_cells"][0, 1] == 2
    assert ref["near_cells"][1, 0] == 1 and ref["edges"][1, 0] == 2
    assert ref["min_d2"][1, 2] == 4 and ref["min_d2"][1, 3] == 4
    assert ref["nearest"][1].tolist() == [0, 2, 3, -1, -1, -1, -1, -1]                # slot 2 (label 4) before slot 3 (label 3)
    assert ref["nearest_d2"][1].tolist() == [1, 4, 4] + [INT_MAX] * 5
    ref = LC.reference(labels, np.array([1, 2, 4, 3], np.int32), cols=7, radius=2, topn=2)
    assert ref["nearest"][1].tolist() == [0, 2]


def test_reference_row_end_pair_is_cols_minus_one_apart():
    cols = 6
    labels = _grid(4, cols, {(1, cols - 1): 1, (2, 0): 2})
    ref = LC.reference(labels, np.array([1, 2], np.int32), cols=cols, radius=4)
    assert (ref["min_d2"] == INT_MAX).all() and not ref["edges"].any() and not ref["near_cells"].any()
    ref = LC.reference(labels, np.array([1, 2], np.int32), cols=cols, radius=6)
    assert ref["min_d2"][0, 1] == (cols - 1) ** 2 + 1 and ref["edges"][0, 1] == 0
    ref = LC.reference(labels, np.array([1, 2], np.int32), cols=cols, radius=1, from_cell=2 * cols)
    assert ref["from_d2"].tolist() == [(cols - 1) ** 2 + 1, 0] and ref["from_closest"].tolist() == [2 * cols - 1, 2 * cols]
    ref = LC.reference(labels, np.array([1, 2, 9], np.int32), cols=cols, radius=1, from_cell=-1)
    assert ref["from_d2"].tolist() == [INT_MAX] * 3 and ref["from_closest"].tolist() == [-1] * 3 and (ref["from_key"] == LC.NONE).all()
    ref = LC.reference(labels, np.array([1, 2, 9], np.int32), cols=cols, radius=1, from_cell=0)
    assert ref["from_d2"].tolist() == [1 + (cols - 1) ** 2, 4, INT_MAX] and ref["from_closest"][2] == -1


def test_reference_symmetry_and_near_cells_below_cells():
    for name, (labels, objects) in LC.own_maps(37, 29, 32, 32, 3).items():
        ref = LC.reference(labels, objects, 29, 3, from_cell=5, topn=8)
        assert np.array_equal(ref["min_d2"], ref["min_d2"].T), name
        assert np.array_equal(ref["edges"], ref["edges"].T), name
        assert (ref["near_cells"] <= ref["cells"][:, None]).all(), name
        assert (np.diag(ref["min_d2"]) == INT_MAX).all() and not np.diag(ref["edges"]).any() and not np.diag(ref["near_cells"]).any()
        assert ((ref["near_cells"] > 0) == (ref["min_d2"] < INT_MAX)).all(), name
        assert ref["cells"].sum() == (LC.slots(labels, objects) >= 0).sum()
    ref = LC.reference(*LC.own_maps(37, 29, 32, 32, 3)["one everywhere"], 29, 3)
    assert (ref["near_cells"][1:, 0] == ref["cells"][1:]).all()                 # every single cell lies inside the reach of the big one


def test_relations_header_and_ctypes_table_agree():
    """include/eod_relations.h against `_lib.RELATIONS_SIGNATURES`: the same entry point on both sides, exported by the
    cross-compiled library, in no other table or header; the header's constants are the binding's."""
    import os
    import re
    import shutil
    import subprocess
    import tempfile
    import __graft_entry__
    __graft_entry__.build()
    from embodied_object_detection_amd import _lib, build, ops
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    path = os.path.join(root, "include", "eod_relations.h")
    txt = open(path).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    declared = sorted(set(re.findall(r"^(?:int|size_t)\s+(eod_\w+)\s*\(", code, flags=re.M)))
    assert declared == sorted(_lib.RELATIONS_SIGNATURES) == ["eod_map_relations"]
    others = (set(_lib.SIGNATURES) | set(_lib.PLACE_SIGNATURES) | set(_lib.REGIONS_SIGNATURES) | set(_lib.INVENTORY_SIGNATURES)
              | set(_lib.DESCRIBE_SIGNATURES))
    assert not set(_lib.RELATIONS_SIGNATURES) & others
    for other in ("eod_hip.h", "eod_place.h", "eod_regions.h", "eod_inventory.h", "eod_describe.h"):
        assert "relations" not in open(os.path.join(root, "include", other)).read().lower()
    for name, (res, args) in _lib.RELATIONS_SIGNATURES.items():
        params = re.search(rf"\b{name}\s*\(([^)]*)\)", code, flags=re.S).group(1)
        assert len(params.split(",")) == len(args) == 20, name
    lib = _lib.load()
    for name, (res, args) in _lib.RELATIONS_SIGNATURES.items():
        fn = getattr(lib, name)                                                  # exported by the library built for gfx950
        assert fn.restype is res and list(fn.argtypes) == list(args), name
    val = lambda name: int(re.search(rf"#define {name} (\d+)", txt).group(1))
    assert (ops.RELATIONS_K_MAX, ops.RELATIONS_N_MAX, ops.RELATIONS_DIM_MAX, ops.RELATIONS_RADIUS_MAX, ops.RELATIONS_TOPN_MAX) == (
        val("EOD_RELATIONS_K_MAX"), val("EOD_RELATIONS_N_MAX"), val("EOD_RELATIONS_DIM_MAX"), val("EOD_RELATIONS_RADIUS_MAX"),
        val("EOD_RELATIONS_TOPN_MAX")) == (64, 2 ** 22, 32767, 16, 8)
    assert 2 * (ops.RELATIONS_DIM_MAX - 1) ** 2 < INT_MAX                        # a squared distance is never the "none" value
    src = open(os.path.join(root, "embodied_object_detection_amd", "csrc", "relations.hip")).read()
    assert (ops.RELATIONS_TILE_ROWS, ops.RELATIONS_TILE_COLS) == tuple(
        int(re.search(rf"\b{n} = (\d+)", src).group(1)) for n in ("RL_TR", "RL_TC"))
    assert "relations.hip" in build.SOURCES
    gcc = shutil.which("gcc")                                                    # the header compiles as C on its own
    if gcc is not None:
        with tempfile.TemporaryDirectory() as d:
            c = os.path.join(d, "t.c")
            open(c, "w").write(f'#include "{path}"\nint main(void) {{ return EOD_RELATIONS_K_MAX == 64 ? 0 : 1; }}\n')
            subprocess.run([gcc, "-std=c11", "-Wall", "-Werror", "-o", os.path.join(d, "t"), c], check=True)
            assert subprocess.run([os.path.join(d, "t")]).returncode == 0


def test_relations_kernels_use_no_scratch():
    import __graft_entry__
    __graft_entry__.build()
    from embodied_object_detection_amd import build
    usage = build.resource_usage()
    if not any("relations_" in k for k in usage):   # a library built elsewhere, without the remarks: build them here
        build.build(force=True, verbose=False)
        usage = build.resource_usage()
    mine = {k: v for k, v in usage.items() if "relations_" in k}
    assert sorted(n for k in mine for n in ("init", "pair", "finish") if f"relations_{n}_kernel" in k) == ["finish", "init", "pair"], sorted(mine)
    assert not [k for k in build.scratch_offenders(usage) if "relations_" in k]
    assert all(v.get("scratch", 0) == 0 for v in mine.values())
    pair = next(v for k, v in mine.items() if "relations_pair_kernel" in k)
    assert pair["lds"] <= 160 * 1024 // 4 and pair["vgprs"] <= 128, pair         # four workgroups per CU


def test_entry_point_refuses_bad_arguments_before_any_launch():
    import ctypes as C
    import __graft_entry__
    __graft_entry__.build()
    from embodied_object_detection_amd import _lib
    lib = _lib.load()
    buf = (C.c_int64 * 4096)()
    p = C.addressof(buf)
    p += (-p) % 16
    BAD, ALIGN, NULL = -1, -2, -4
    ptrs = ("labels", "objects", "pair_key", "min_d2", "closest", "near_cells", "edges", "cells", "nearest", "nearest_d2", "from_key",
            "from_d2", "from_closest")

    def call(N=100, K=5, cols=10, radius=2, from_cell=-1, topn=4, **kw):
        a = {name: p for name in ptrs}
        a.update(kw)
        return lib.eod_map_relations(a["labels"], a["objects"], N, K, cols, radius, from_cell, topn, *[a[n] for n in ptrs[2:]], None)

    for kw in (dict(K=0), dict(K=65), dict(K=-1), dict(N=0), dict(N=2 ** 22 + 1), dict(N=-5), dict(cols=0), dict(cols=-10), dict(cols=7),
               dict(cols=101), dict(radius=0), dict(radius=17), dict(radius=-1), dict(topn=0), dict(topn=9), dict(topn=-2),
               dict(from_cell=-2), dict(from_cell=100), dict(from_cell=2 ** 31 - 1), dict(N=32768, cols=32768), dict(N=32768, cols=1),
               dict(N=2 ** 22, cols=2 ** 22), dict(N=2 ** 22, cols=64)):
        assert call(**kw) == BAD, kw
    none = {name: None for name in ptrs}
    assert call(K=0, **none) == BAD                                              # a bad dimension wins over a null pointer
    assert call(radius=17, pair_key=p + 4) == BAD                                # and over alignment
    for name in ptrs:
        assert call(**{name: None}) == NULL, name
        assert call(**{name: None, "pair_key" if name != "pair_key" else "from_key": p + 4}) == NULL, name      # null wins over alignment
    for kw in (dict(pair_key=p + 4), dict(from_key=p + 4), dict(pair_key=p + 1), dict(labels=p + 2), dict(objects=p + 1), dict(min_d2=p + 2),
               dict(closest=p + 1), dict(near_cells=p + 3), dict(edges=p + 2), dict(cells=p + 1), dict(nearest=p + 2),
               dict(nearest_d2=p + 3), dict(from_d2=p + 1), dict(from_closest=p + 2)):
        assert call(**kw) == ALIGN, kw


def test_ops_refuse_on_the_host_naming_the_argument():
    import torch
    import __graft_entry__
    __graft_entry__.build()
    from embodied_object_detection_amd import _lib, ops
    labels, objects = torch.zeros((120,), dtype=torch.int32), torch.zeros((5,), dtype=torch.int32)
    for bad in (torch.zeros((0,), dtype=torch.int32), torch.zeros((120,), dtype=torch.int64), torch.zeros((12, 10), dtype=torch.int32),
                torch.zeros((240,), dtype=torch.int32)[::2], torch.zeros((120,)), np.zeros(120, np.int32)):
        with pytest.raises(_lib.EodError, match="object_labels"):
            ops.map_relations(bad, objects, 10)
    with pytest.raises(_lib.EodError, match="object_labels: N 4194305"):          # no storage behind it: refused by its shape
        ops.map_relations(torch.empty((2 ** 22 + 1,), dtype=torch.int32, device="meta"), objects, 1)
    for bad in (torch.zeros((0,), dtype=torch.int32), torch.zeros((65,), dtype=torch.int32), torch.zeros((5,), dtype=torch.int64),
                torch.zeros((1, 5), dtype=torch.int32), torch.zeros((10,), dtype=torch.int32)[::2], [1, 2, 3],
                torch.zeros((5,), dtype=torch.int32, device="meta")):
        with pytest.raises(_lib.EodError, match="objects"):
            ops.map_relations(labels, bad, 10)
    for bad in (0, -10, 7, 121, 2.5, True, None):
        with pytest.raises(_lib.EodError, match="cols"):
            ops.map_relations(labels, objects, bad)
    with pytest.raises(_lib.EodError, match="cols"):
        ops.map_relations(torch.zeros((32768,), dtype=torch.int32), objects, 1)   # 32768 rows
    for bad in (0, 17, -1, 1.5, True):
        with pytest.raises(_lib.EodError, match="radius"):
            ops.map_relations(labels, objects, 10, radius=bad)
    for bad in (-2, 120, 3.0, None, False):
        with pytest.raises(_lib.EodError, match="from_cell"):
            ops.map_relations(labels, objects, 10, from_cell=bad)
    for bad in (0, 9, -1, 2.5, True):
        with pytest.raises(_lib.EodError, match="topn"):
            ops.map_relations(labels, objects, 10, topn=bad)
    with pytest.raises(_lib.EodError, match="no CPU fallback"):                   # tensors on the host: refused last
        ops.map_relations(labels, objects, 10, radius=16, from_cell=119, topn=8)


def test_model_surfaces_require_the_grid():
    import torch
    import __graft_entry__
    __graft_entry__.build()
    from embodied_object_detection_amd import _lib
    from embodied_object_detection_amd.modeling.meta_arch import _relations
    labels = torch.zeros((120,), dtype=torch.int32)
    with pytest.raises(_lib.EodError, match="map_shape"):
        _relations([1, 2], labels, None, 2, None, 4)
    with pytest.raises(_lib.EodError, match="map_shape"):
        _relations([1, 2], labels, (11, 10), 2, None, 4)
    with pytest.raises(_lib.EodError, match="no CPU fallback"):                   # a sequence of objects will do; from_cell None is -1
        _relations([1, 2], labels, (12, 10), 2, None, 4)


def test_relation_metres():
    from embodied_object_detection_amd.data.robot import RobotFrontEnd
    front = RobotFrontEnd.__new__(RobotFrontEnd)
    front.res = 0.05
    m = front.relation_metres(np.array([[0, 25, INT_MAX], [1, 2, 4]], np.int32))
    assert m.dtype == np.float64 and m.shape == (2, 3)
    assert m[0].tolist() == [0.0, 5 * 0.05, np.inf] and m[1].tolist() == [0.05, np.sqrt(2.0) * 0.05, 0.1]
