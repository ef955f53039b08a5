"""The host side of `place` (no GPU): the numpy reference of `_place_cases.py` against a brute-force count on the edge cases of
`test_place_gpu.py`, what those cases hold, and the robot front-end's cell helpers."""
import numpy as np
import pytest

import _place_cases as PC


@pytest.mark.parametrize("topk", [1, 4, 8])
@pytest.mark.parametrize("count", [PC.COUNT, None])
def test_reference_equals_the_brute_force_count(topk, count):
    c = PC.edge_cases()
    for rects, excl in ((c["rects"], c["exclude_cell"]), (None, -1)):
        ref = PC.reference(c["masks"], c["proj"], PC.N_CELLS, count, rects, topk, excl)
        bf = PC.brute_force(c["masks"], c["proj"], PC.N_CELLS, count, rects, topk, excl)
        for k in PC.KEYS:
            assert ref[k].dtype == np.int32 and np.array_equal(ref[k], bf[k]), (k, ref[k].tolist(), bf[k].tolist())


def test_edge_cases_hold_what_their_names_say():
    c = PC.edge_cases()
    ref = PC.reference(c["masks"], c["proj"], PC.N_CELLS, PC.COUNT, c["rects"], 8, c["exclude_cell"])
    mp, px, inv, dis, cells, cp = (ref[k] for k in PC.KEYS)
    assert len(PC.ROW_NAMES) == PC.K_CAP
    assert (mp[0], px[0], dis[0]) == (0, 0, 0) and (cells[0] == -1).all()
    assert (mp[1], px[1], dis[1]) == (2, 2, 2) and cells[1, :2].tolist() == [0, PC.N_CELLS - 1]
    assert mp[2] == PC.H * PC.W and inv[2] == 4 and dis[2] >= 300 and px[2] < mp[2] - 4          # the excluded cell's pixels are dropped
    assert mp[3] == (25 - 10) * (31 - 12) and mp[3] < int(c["masks"][3].sum())
    assert 0 < mp[4] < 20 * 15 and set(np.unique(c["masks"][4]).tolist()) == {0, 2, 255}
    assert (mp[5], px[5], inv[5], dis[5]) == (0, 0, 0, 0) and int(c["masks"][5].sum()) > 0
    assert cells[6, :6].tolist() == c["tie_cells"] and cp[6, :6].tolist() == [2] * 6 and cells[6, 6] == -1 and dis[6] == 6
    assert dis[7] == 1 and cells[7].tolist() == [c["one_cell"]] + [-1] * 7 and cp[7, 0] == mp[7] == px[7] > 0 and cp[7, 1] == 0
    assert mp[8] > 0 and (px[8], inv[8], dis[8]) == (0, 0, 0) and (cells[8] == -1).all()
    assert inv[9] == 4 and mp[9] == 6 * 7 and set(np.unique(c["masks"][9]).tolist()) == {0, 2, 255}
    assert (mp[10:] == 0).all() and (cells[10:] == -1).all() and (cp[10:] == 0).all() and int(c["masks"][10:].astype(bool).sum()) > 1000
    every = PC.reference(c["masks"], c["proj"], PC.N_CELLS, None, c["rects"], 8, c["exclude_cell"])
    assert (every["mask_pixels"][10:] > 0).all()


def test_robot_front_end_cell_helpers():
    from embodied_object_detection_amd.data.robot import RobotFrontEnd
    fe = RobotFrontEnd(projector=lambda *a: None, map_w=30, map_h=20, res=0.25, map_shift=(-3.0, 0.0, -2.0))
    cells = np.array([0, 19, 20, 599, -1, 7 * 20 + 3], dtype=np.int32)
    got = fe.cell_centers(cells)
    assert got.dtype == np.float64 and got.shape == (6, 2)
    for i, cell in enumerate(cells.tolist()):
        if cell < 0:
            assert np.isnan(got[i]).all()
        else:
            assert tuple(got[i].tolist()) == fe.cell_center(cell), cell
    assert fe.cell_centers([]).shape == (0, 2)
    import torch
    assert np.array_equal(fe.cell_centers(torch.tensor([[20, 599], [-1, 0]])), fe.cell_centers([20, 599, -1, 0]), equal_nan=True)
    for pose in ((0.0, 0.0, 0.3), (1.13, -0.4, 0.0), (-2.9, 2.6, 1.0)):
        x, y = fe.robot_cell(pose)
        cell = fe.exclude_cell(pose)
        assert cell == x * fe.map_h + y and 0 <= cell < fe.n_cells
        assert fe.cell_center(cell) == fe.cell_center((x, y))
        cx, cy = fe.cell_center(cell)
        assert abs(cx - pose[0]) <= fe.res / 2 + 1e-6 and abs(cy - pose[1]) <= fe.res / 2 + 1e-6


def test_place_header_and_ctypes_table_agree():
    """include/eod_place.h against `_lib.PLACE_SIGNATURES`, as tests/test_host_cpu.py holds include/eod_hip.h to `_lib.SIGNATURES`:
    the same entry points on both sides, every one exported by the library, none of them twice; and the header's constants are
    the binding's (the header is the definition)."""
    import os
    import re
    import __graft_entry__
    __graft_entry__.build()
    from embodied_object_detection_amd import _lib, ops
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    txt = open(os.path.join(root, "include", "eod_place.h")).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    declared = sorted(set(re.findall(r"^(?:int|size_t)\s+(eod_\w+)\s*\(", code, flags=re.M)))
    assert declared == sorted(_lib.PLACE_SIGNATURES) == ["eod_place_masks", "eod_place_masks_workspace_bytes"]
    assert not set(_lib.PLACE_SIGNATURES) & set(_lib.SIGNATURES)
    lib = _lib.load()
    for name, (res, args) in _lib.PLACE_SIGNATURES.items():
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == list(args), name
    val = lambda name: int(re.search(rf"#define {name} (\d+)", txt).group(1))
    assert (ops.PLACE_TOPK_MAX, ops.PLACE_TABLE_LOG2_MIN, ops.PLACE_TABLE_LOG2_MAX, ops.PLACE_TABLE_LOG2) == (
        val("EOD_PLACE_TOPK_MAX"), val("EOD_PLACE_TABLE_LOG2_MIN"), val("EOD_PLACE_TABLE_LOG2_MAX"), val("EOD_PLACE_TABLE_LOG2"))
    assert ops.PLACE_TABLE_LOG2_MIN <= 4 and ops.PLACE_TABLE_LOG2_MAX >= 12
    # the header compiles as C on its own
    import shutil
    import subprocess
    import tempfile
    gcc = shutil.which("gcc")
    if gcc is not None:
        with tempfile.TemporaryDirectory() as d:
            src = os.path.join(d, "t.c")
            open(src, "w").write(f'#include "{os.path.join(root, "include", "eod_place.h")}"\nint main(void) {{ return EOD_PLACE_SLOTS == 4 ? 0 : 1; }}\n')
            subprocess.run([gcc, "-std=c11", "-Wall", "-Werror", "-o", os.path.join(d, "t"), src], check=True)
            assert subprocess.run([os.path.join(d, "t")]).returncode == 0


def test_entry_point_refuses_bad_arguments_before_any_launch():
    import ctypes as C
    import __graft_entry__
    __graft_entry__.build()
    from embodied_object_detection_amd import _lib
    lib = _lib.load()
    buf = (C.c_int32 * 4096)()
    p = C.addressof(buf)
    BAD, ALIGN, NULL, CAP = -1, -2, -4, -5
    need = lib.eod_place_masks_workspace_bytes(12, 437)
    assert need == (64 + 12 + 63) // 64 * 256 + 4 * ((437 * 4 + 255) // 256 * 256)          # the list, four dense tables; no K_cap * n_cells
    assert lib.eod_place_masks_workspace_bytes(300, 262144) == (64 + 300 + 63) // 64 * 256 + 4 * 262144 * 4
    assert lib.eod_place_masks_workspace_bytes(-1, 437) == 0 and lib.eod_place_masks_workspace_bytes(12, 0) == 0
    call = lambda masks=p, proj=p, K=12, H=45, W=37, n=437, T=4, log2=0, out=p, ws=p, ws_bytes=need: lib.eod_place_masks(
        masks, proj, None, None, K, H, W, n, T, -1, log2, out, ws, ws_bytes, None)
    assert call(K=0) == 0 and call(K=0, masks=None, proj=None, out=None, ws=None, ws_bytes=0) == 0      # nothing to do, nothing launched
    for kw in (dict(K=-1), dict(H=0), dict(W=0), dict(n=0), dict(T=0), dict(T=9), dict(log2=3), dict(log2=13), dict(log2=-1),
               dict(H=65536, W=65536)):
        assert call(**kw) == BAD, kw
    for kw in (dict(masks=None), dict(proj=None), dict(out=None), dict(ws=None)):
        assert call(**kw) == NULL, kw
    for kw in (dict(proj=p + 2), dict(out=p + 1), dict(ws=p + 2)):
        assert call(**kw) == ALIGN, kw
    assert call(ws_bytes=need - 1) == CAP
