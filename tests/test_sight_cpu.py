"""The host side of `map_sight` (no GPU): the reference of `_sight_cases.py` on the header's hand-worked maps and under mirroring
and transposing, include/eod_sight.h against its ctypes table and the cross-compiled library, the build's records, and every
refused argument (the entry point returns before a launch, so it is callable here)."""
import time

import numpy as np
import pytest

import _sight_cases as SC

INT_MAX = SC.INT_MAX


def test_reference_hand_worked_maps():
    """Maps A to D of the header's comment, and the asymmetric pair of map D."""
    for name in SC.HAND:
        g, want = SC.hand_map(name)
        sources = sorted(want)
        ref = SC.reference(g.reshape(-1), [1, 9], g.shape[1], sources)
        for s, f in enumerate(sources):
            assert SC.seen_rows(ref, s, *g.shape) == want[f], (name, f)
        assert ref["status"].tolist() == [0, 0]
        for k in SC.KEYS:
            assert ref[k].dtype == (np.uint64 if k in SC.WIDE else np.int32), k
    g, _ = SC.hand_map("D")
    ref = SC.reference(g.reshape(-1), [1], 5, [0, 9])
    assert not (int(ref["seen_mask"][9]) >> 0) & 1 and (int(ref["seen_mask"][0]) >> 1) & 1      # 0 does not see 9; 9 sees 0
    assert SC.rnd(np.array([2]), np.array([4]))[0] == 1 and SC.rnd(np.array([-2]), np.array([4]))[0] == -1     # a half: away from zero
    assert SC.rnd(np.array([1, -1, 3, -3, 5, 6]), np.array([4, 4, 4, 4, 4, 4])).tolist() == [0, 0, 1, -1, 1, 2]


def test_reference_other_outputs_on_a_hand_worked_map():
    """Map A from two sources and an unused one: slots 9 and 4, a label nobody asked for, every output by hand."""
    g, _ = SC.hand_map("A")
    ref = SC.reference(g.reshape(-1), [4, 9, 9, -1], 7, [14, -1, 6, 14])           # 6 = (0, 6), the far corner
    assert ref["cells"].tolist() == [1, 1, 0, 0]                                   # the later duplicate slot gets no cells
    assert SC.seen_rows(ref, 1, 5, 7) == ["0000000"] * 5 and ref["source_counts"][1].tolist() == [0, 0]
    assert SC.seen_rows(ref, 3, 5, 7) == SC.seen_rows(ref, 0, 5, 7)
    # source 0 = cell 14 sees both objects: (1, 2) at d2 = 1 + 4, (2, 3) at d2 = 9
    assert ref["seen_cells"][0].tolist() == [1, 1, 0, 0] and ref["near_d2"][0].tolist() == [9, 5, INT_MAX, INT_MAX]
    assert ref["near_cell"][0].tolist() == [17, 9, -1, -1] and ref["near_key"][0, 0] == (9 << 32) | 17
    assert ref["near_key"][0, 2] == 2 ** 64 - 1
    assert ref["source_counts"][0].tolist() == [22, 2] and ref["counts"][:2].tolist() == [2, 33]
    # both sources see one cell of each object: the lowest source wins the tie
    assert ref["seen_cells"][2].tolist() == [1, 1, 0, 0]
    assert ref["best_seen"].tolist() == [1, 1, 0, 0] and ref["best_source"].tolist() == [0, 0, -1, -1]
    assert ref["best_key"][0] == (1 << 32) | 0xFFFFFFFF and ref["best_key"][2] == 0
    # range2 = 5 from cell 14: (1, 2) is in range, (2, 3) is not; range2 = 0: the source's own cell alone
    near = SC.reference(g.reshape(-1), [4, 9], 7, [14], range2=5)
    assert near["seen_cells"][0].tolist() == [0, 1] and near["best_source"].tolist() == [-1, 0]
    assert SC.seen_rows(near, 0, 5, 7) == ["1100000", "1110000", "1110000", "1110000", "1100000"]
    own = SC.reference(g.reshape(-1), [4, 9], 7, [14, 9], range2=0)
    assert own["counts"].tolist() == [2, 33, 2] and own["seen_cells"].tolist() == [[0, 0], [0, 1]]        # a source on an object sees it
    assert own["source_counts"].tolist() == [[1, 0], [0, 1]]                       # its own cell counts by its label
    # 9 made passable: transparent, it keeps its cells, and the view through it is open
    thru = SC.reference(g.reshape(-1), [4, 9], 7, [14], passable=[9])
    assert SC.seen_rows(thru, 0, 5, 7)[0] == "1111111" and thru["counts"][:2].tolist() == [1, 34] and thru["cells"].tolist() == [1, 1]
    assert thru["source_counts"][0].tolist() == [int(sum(r.count("1") for r in SC.seen_rows(thru, 0, 5, 7))) - 1, 1]


def test_reference_mirror_and_transpose_identities():
    """seen(mirror(map), mirror(source)) == mirror(seen(map, source)), and the same for the transpose; not so for swapping the
    ends, which map D shows."""
    rng = np.random.default_rng(3)
    for rows, cols in ((9, 14), (14, 9), (1, 12), (11, 11)):
        opaque = rng.random((rows, cols)) < 0.15
        for f in rng.integers(0, rows * cols, 6).tolist():
            r0, c0 = divmod(f, cols)
            for range2 in (INT_MAX, 30):
                seen = SC.seen_from(opaque, f, range2)
                assert np.array_equal(SC.seen_from(opaque[::-1], (rows - 1 - r0) * cols + c0, range2), seen[::-1])
                assert np.array_equal(SC.seen_from(opaque[:, ::-1], r0 * cols + cols - 1 - c0, range2), seen[:, ::-1])
                assert np.array_equal(SC.seen_from(np.ascontiguousarray(opaque.T), c0 * rows + r0, range2), seen.T)
                assert seen[r0, c0]


def test_reference_is_quick_enough():
    """The largest ordinary grid of the GPU tests, 64 distinct sources, no opaque cell: every line runs its full length."""
    times = []
    for shift in (0, 1, 2):                                          # three calls the reference has not cached; each is held to the bound
        t = time.perf_counter()
        ref = SC.reference(np.full(70 * 67, -1, np.int32), [1], 67, np.arange(64) * 70 + shift)
        times.append(time.perf_counter() - t)
        assert (ref["seen_mask"] == np.uint64(2 ** 64 - 1)).all()
    print(f"reference, 70 x 67, 64 sources, no opaque cell: {[round(v, 2) for v in times]} s")
    assert max(times) < 2.0


def test_maps_hold_the_cases_they_name():
    ms = SC.maps(70, 67)
    assert SC.tie_cells(1, 2) == [(1, 1, 0)] and SC.tie_cells(1, 4) == [(2, 1, 0)] and SC.tie_cells(3, 6) == [(1, 1, 0), (3, 2, 1), (5, 3, 2)]
    ties = [k for k in ms if k.startswith("half tie")]
    assert len(ties) == 20 and len([k for k in ms if k.startswith("neighbour")]) == 8
    y, x = 35, 33
    for name in ties:
        m = ms[name]
        ref = SC.reference(m["labels"], m["objects"], 67, m["from_cells"])
        a, b = (int(v) for v in name.split()[2].split(":"))
        if name.endswith("columns"):
            hidden = [not (int(ref["seen_mask"][(y + sy * a) * 67 + x + sx * b]) & 1) for sy in (-1, 1) for sx in (-1, 1)]
        else:
            hidden = [not (int(ref["seen_mask"][(y + sy * b) * 67 + x + sx * a]) & 1) for sy in (-1, 1) for sx in (-1, 1)]
        assert all(hidden) if ", picked" in name else not any(hidden), name         # in the four octants of the map
    for name, hides in (("both", True), ("one side", False), ("the other side", False), ("both, opaque target", True),
                        ("one side, opaque target", False), ("neither, opaque target", False)):
        m = ms[f"corner pair: {name}"]
        ref = SC.reference(m["labels"], m["objects"], 67, m["from_cells"])
        for sy in (-1, 1):
            for sx in (-1, 1):
                assert bool(int(ref["seen_mask"][(y + 3 * sy) * 67 + x + 3 * sx]) & 1) != hides, name
    m = ms["row-end pair"]
    ref = SC.reference(m["labels"], m["objects"], 67, m["from_cells"])
    assert m["labels"][y * 67 - 1] == 10 and ref["seen_mask"][y * 67] == 7         # (y, 0) follows the opaque cell in memory: all three see it
    m = ms["a source on an opaque cell"]
    ref = SC.reference(m["labels"], m["objects"], 67, m["from_cells"])
    assert (ref["seen_mask"][y * 67 + x + 1:(y + 1) * 67] & np.uint64(1)).all()    # standing on it, it hides nothing
    assert not (ref["seen_mask"][y * 67 + x + 1:(y + 1) * 67] & np.uint64(2)).any()        # from (y, 0) the two cells hide the rest of the row
    assert len(ms) == 49
    assert len(SC.maps(3, 61)) < len(SC.maps(19, 195)) == 49


def test_sight_header_and_ctypes_table_agree():
    """include/eod_sight.h against `_lib.SIGHT_SIGNATURES`: the same two entry points on both sides, exported by the cross-compiled
    library, in no other table or header; the header's constants are the binding's and the kernel's; the header compiles as C on its
    own and says what it must about the line's asymmetry."""
    import os
    import re
    import shutil
    import subprocess
    import tempfile
    import __graft_entry__
    __graft_entry__.build()
    from embodied_object_detection_amd import _lib, build, ops
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    path = os.path.join(root, "include", "eod_sight.h")
    txt = open(path).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    declared = sorted(set(re.findall(r"^(?:int|size_t)\s+(eod_\w+)\s*\(", code, flags=re.M)))
    assert declared == sorted(_lib.SIGHT_SIGNATURES) == ["eod_map_sight", "eod_map_sight_workspace_bytes"]
    others = (set(_lib.SIGNATURES) | set(_lib.PLACE_SIGNATURES) | set(_lib.REGIONS_SIGNATURES) | set(_lib.INVENTORY_SIGNATURES)
              | set(_lib.DESCRIBE_SIGNATURES) | set(_lib.RELATIONS_SIGNATURES) | set(_lib.ROUTE_SIGNATURES) | set(_lib.CLEARANCE_SIGNATURES))
    assert not set(_lib.SIGHT_SIGNATURES) & others and len(_lib.SIGNATURES) == 75 and len(_lib.CLEARANCE_SIGNATURES) == 2
    for other in ("eod_hip.h", "eod_place.h", "eod_regions.h", "eod_inventory.h", "eod_describe.h", "eod_relations.h", "eod_route.h",
                  "eod_clearance.h"):
        assert "eod_map_sight" not in open(os.path.join(root, "include", other)).read()
    for name, n in (("eod_map_sight", 25), ("eod_map_sight_workspace_bytes", 2)):
        res, args = _lib.SIGHT_SIGNATURES[name]
        params = re.search(rf"\b{name}\s*\(([^)]*)\)", code, flags=re.S).group(1)
        assert len(params.split(",")) == len(args) == n, name
    lib = _lib.load()
    for name, (res, args) in _lib.SIGHT_SIGNATURES.items():
        fn = getattr(lib, name)                                                  # exported by the library built for gfx950
        assert fn.restype is res and list(fn.argtypes) == list(args), name
    val = lambda name: int(re.search(rf"#define {name} (\d+)", txt).group(1))
    assert (ops.SIGHT_K_MAX, ops.SIGHT_P_MAX, ops.SIGHT_N_MAX, ops.SIGHT_DIM_MAX) == (
        val("EOD_SIGHT_K_MAX"), val("EOD_SIGHT_P_MAX"), val("EOD_SIGHT_N_MAX"), val("EOD_SIGHT_DIM_MAX")) == (
        ops.CLEARANCE_K_MAX, ops.CLEARANCE_P_MAX, ops.CLEARANCE_N_MAX, ops.CLEARANCE_DIM_MAX) == (64, 64, 2 ** 22, 32767)
    assert (ops.SIGHT_S_MAX, ops.SIGHT_LDS_CELLS, ops.SIGHT_SOURCE_GROUP) == (
        val("EOD_SIGHT_S_MAX"), val("EOD_SIGHT_LDS_CELLS"), val("EOD_SIGHT_SOURCE_GROUP")) == (64, 131072, 16)
    assert 2 * (ops.SIGHT_DIM_MAX - 1) ** 2 < INT_MAX == ops.SIGHT_UNBOUNDED     # a real distance is below the unbounded range
    assert 2 * (ops.SIGHT_DIM_MAX - 1) ** 2 + ops.SIGHT_DIM_MAX - 1 < 2 ** 31    # 2 * i * |d| + n of the closed form
    src = open(os.path.join(root, "embodied_object_detection_amd", "csrc", "sight.hip")).read()
    assert f"SI_WG = {ops.SIGHT_WORKGROUP};" in src and "SI_G = EOD_SIGHT_SOURCE_GROUP" in src and "N <= EOD_SIGHT_LDS_CELLS" in src
    assert "sight.hip" in build.SOURCES
    assert "NOT symmetric" in txt and "Cell 0 does not see cell 9" in txt and "Cell 9 sees cell 0" in txt
    for rows, cols in ((1, 1), (200, 200), (70, 67), (32767, 128), (1, 32767)):
        N = rows * cols
        need = lib.eod_map_sight_workspace_bytes(N, cols)
        assert need >= N + (N + 63) // 64 * 8 and need % 8 == 0 and need == 4 * ops.map_sight_workspace(N, cols)
    for N, cols in ((0, 1), (10, 3), (2 ** 22 + 1, 1), (32768, 1), (32768, 32768), (-4, 2), (4, 0)):
        assert lib.eod_map_sight_workspace_bytes(N, cols) == 0
    with pytest.raises(_lib.EodError, match="map_sight_workspace"):
        ops.map_sight_workspace(10, 3)
    cc = next((p for p in (shutil.which(n) for n in ("gcc", "cc", "clang")) if p), None)
    assert cc is not None, "no C compiler (gcc, cc, clang) on PATH: the header cannot be checked as C"
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "t.c")
        open(c, "w").write(f'#include "{path}"\nint main(void) {{ return EOD_SIGHT_S_MAX == 64 ? 0 : 1; }}\n')
        subprocess.run([cc, "-std=c11", "-Wall", "-Werror", "-o", os.path.join(d, "t"), c], check=True)
        assert subprocess.run([os.path.join(d, "t")]).returncode == 0


def test_sight_kernels_use_no_scratch():
    import __graft_entry__
    __graft_entry__.build()
    from embodied_object_detection_amd import build, ops
    usage = build.resource_usage()
    if not any("sight_" in k for k in usage):           # a library built elsewhere, without the remarks: build them here
        build.build(force=True, verbose=False)
        usage = build.resource_usage()
    mine = {k: v for k, v in usage.items() if "sight_" in k}
    names = ("init", "walk", "walk", "finish")          # the walk twice: staged and not
    assert sorted(n for k in mine for n in set(names) if f"sight_{n}_kernel" in k) == sorted(names), sorted(mine)
    assert not [k for k in build.scratch_offenders(usage) if "sight_" in k]
    assert all(v.get("scratch", 0) == 0 for v in mine.values())
    for k, v in mine.items():
        if "sight_walk_kernel" in k:
            # static LDS (the sums of one source group) plus the staged bit plane at its limit: five workgroups of four waves a CU
            assert 5 * (v["lds"] + ops.SIGHT_LDS_CELLS // 8) <= 160 * 1024 and v["vgprs"] <= 64, (k, v)


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
    ptrs = ("labels", "objects", "passable", "from_cells", "seen_mask", "cells", "seen_cells", "near_key", "near_d2", "near_cell",
            "best_key", "best_seen", "best_source", "source_counts", "counts", "status", "workspace")
    src = (C.c_int32 * 64)(*([5, -1, 99, 0, -2 ** 31] + [7] * 59))
    sp = C.addressof(src)

    def call(N=100, K=5, P=2, S=5, cols=10, range2=4, workspace_bytes=4096, **kw):
        a = {name: p for name in ptrs}
        a["from_cells"] = sp
        a.update(kw)
        return lib.eod_map_sight(a["labels"], a["objects"], a["passable"], a["from_cells"], N, K, P, S, cols, range2,
                                 *[a[n] for n in ptrs[4:]], workspace_bytes, None)

    for kw in (dict(K=0), dict(K=65), dict(K=-1), dict(P=-1), dict(P=65), dict(S=0), dict(S=65), dict(S=-3), dict(N=0),
               dict(N=2 ** 22 + 1), dict(N=-5), dict(cols=0), dict(cols=-10), dict(cols=7), dict(cols=101), dict(range2=-1),
               dict(range2=-2 ** 31), dict(N=32768, cols=32768), dict(N=32768, cols=1), dict(N=2 ** 22, cols=2 ** 22),
               dict(N=2 ** 22, cols=64), dict(N=99, cols=9), dict(N=90, cols=10), dict(N=10, cols=10, S=3)):      # a source >= N
        assert call(**kw) == BAD, kw
    one = (C.c_int32 * 2)(100, 3)
    assert call(S=1, from_cells=C.addressof(one)) == BAD and call(S=2, from_cells=C.addressof(one)) == BAD
    assert call(S=1, from_cells=C.addressof(one) + 4, workspace_bytes=0) == CAPACITY          # only the first S entries are judged
    none = {name: None for name in ptrs}
    assert call(K=0, **none) == BAD                                              # a bad dimension wins over a null pointer
    assert call(range2=-1, near_key=p + 4) == BAD                                # and over alignment
    assert call(S=65, workspace_bytes=0) == BAD                                  # and over the workspace
    assert call(N=90, cols=10, seen_mask=None) == BAD                            # a source outside the map too
    for name in ptrs:
        assert call(**{name: None}) == NULL, name
        assert call(**{name: None, "near_key" if name != "near_key" else "workspace": p + 4}) == NULL, name     # null wins over alignment
        assert call(workspace_bytes=0, **{name: None}) == NULL, name                                            # and over the workspace
    assert call(P=0, passable=None, workspace_bytes=0) == CAPACITY               # passable may be null without passable labels
    for kw in (dict(seen_mask=p + 4), dict(near_key=p + 4), dict(best_key=p + 4), dict(workspace=p + 4), dict(near_key=p + 1),
               dict(labels=p + 2), dict(objects=p + 1), dict(passable=p + 2), dict(from_cells=p + 2), dict(cells=p + 1),
               dict(seen_cells=p + 2), dict(near_d2=p + 3), dict(near_cell=p + 1), dict(best_seen=p + 2), dict(best_source=p + 3),
               dict(source_counts=p + 1), dict(counts=p + 1), dict(status=p + 2)):
        assert call(**kw) == ALIGN, kw
        assert call(workspace_bytes=0, **kw) == ALIGN, kw                        # alignment wins over the workspace
    need = lib.eod_map_sight_workspace_bytes(100, 10)
    assert need == 256 + 256
    for short in (0, 8, need - 1):
        assert call(workspace_bytes=short) == CAPACITY, short
    assert call(range2=2 ** 31 - 1, S=64, K=64, P=64, workspace_bytes=need - 1) == CAPACITY     # the largest values pass the first check


def test_ops_refuse_on_the_host_naming_the_argument():
    import torch
    import __graft_entry__
    __graft_entry__.build()
    from embodied_object_detection_amd import _lib, ops
    labels, objects = torch.zeros((120,), dtype=torch.int32), torch.zeros((5,), dtype=torch.int32)
    for bad in (torch.zeros((0,), dtype=torch.int32), torch.zeros((120,), dtype=torch.int64), torch.zeros((12, 10), dtype=torch.int32),
                torch.zeros((240,), dtype=torch.int32)[::2], torch.zeros((120,)), np.zeros(120, np.int32)):
        with pytest.raises(_lib.EodError, match="object_labels"):
            ops.map_sight(bad, objects, 10, [0])
    with pytest.raises(_lib.EodError, match="object_labels: N 4194305"):          # no storage behind it: refused by its shape
        ops.map_sight(torch.empty((2 ** 22 + 1,), dtype=torch.int32, device="meta"), objects, 1, [0])
    for bad in (torch.zeros((0,), dtype=torch.int32), torch.zeros((65,), dtype=torch.int32), torch.zeros((5,), dtype=torch.int64),
                torch.zeros((1, 5), dtype=torch.int32), torch.zeros((10,), dtype=torch.int32)[::2], [1, 2, 3],
                torch.zeros((5,), dtype=torch.int32, device="meta")):
        with pytest.raises(_lib.EodError, match="objects"):
            ops.map_sight(labels, bad, 10, [0])
    for bad in (0, -10, 7, 121, 2.5, True, None):
        with pytest.raises(_lib.EodError, match="cols"):
            ops.map_sight(labels, objects, bad, [0])
    with pytest.raises(_lib.EodError, match="cols"):
        ops.map_sight(torch.zeros((32768,), dtype=torch.int32), objects, 1, [0])  # 32768 rows
    for bad in ([], list(range(65)), 120, [3, 120], [0.5], 2.0, None, True, "ab", torch.zeros((3,)), torch.zeros((2, 2), dtype=torch.int32),
                torch.zeros((65,), dtype=torch.int64), torch.tensor([120]), [-2 ** 31 - 1], torch.zeros((2,), dtype=torch.int32, device="meta")):
        with pytest.raises(_lib.EodError, match="from_cells"):
            ops.map_sight(labels, objects, 10, bad)
    for bad in (-1, 2 ** 31, 2 ** 40, 2.0, True):
        with pytest.raises(_lib.EodError, match="range2"):
            ops.map_sight(labels, objects, 10, [0], range2=bad)
    for bad in (torch.zeros((65,), dtype=torch.int32), torch.zeros((3,), dtype=torch.int64), torch.zeros((2, 2), dtype=torch.int32),
                torch.zeros((4,), dtype=torch.int32, device="meta"), 7, ["a"], list(range(65))):
        with pytest.raises(_lib.EodError, match="passable"):
            ops.map_sight(labels, objects, 10, [0], passable=bad)
    for good in (119, [0, -1, 119, 0], torch.tensor([5, -7], dtype=torch.int32), torch.tensor(7), np.array([1, 2])):
        with pytest.raises(_lib.EodError, match="no CPU fallback"):               # tensors on the host: refused last
            ops.map_sight(labels, objects, 10, good, range2=2 ** 31 - 1, passable=[3, 4])


def test_model_surfaces_require_the_grid_and_the_sources():
    import torch
    import __graft_entry__
    __graft_entry__.build()
    from embodied_object_detection_amd import _lib
    from embodied_object_detection_amd.engine.predictor import EmbodiedPredictor
    from embodied_object_detection_amd.modeling.lockstep import LockstepScenes
    from embodied_object_detection_amd.modeling.meta_arch import CustomRCNNRecurrent, _sight
    labels = torch.zeros((120,), dtype=torch.int32)
    with pytest.raises(_lib.EodError, match="sight: map_shape"):
        _sight([1, 2], labels, None, [0])
    with pytest.raises(_lib.EodError, match="sight: map_shape"):
        _sight([1, 2], labels, (11, 10), [0])
    with pytest.raises(_lib.EodError, match="sight: from_cells is required"):
        _sight([1, 2], labels, (12, 10), None)
    with pytest.raises(_lib.EodError, match="from_cells"):
        _sight([1, 2], labels, (12, 10), [120])
    with pytest.raises(_lib.EodError, match="range2"):
        _sight([1, 2], labels, (12, 10), 0, range2=-1)
    with pytest.raises(_lib.EodError, match="map_sight: object_labels on the host .no CPU fallback"):      # sequences will do
        _sight([1, 2], labels, (12, 10), 7, 16, passable=[0])
    for cls in (CustomRCNNRecurrent, LockstepScenes, EmbodiedPredictor):
        assert "from_cells" in cls.sight.__doc__ and callable(cls.sight)
    assert "best_source" in CustomRCNNRecurrent.sight.__doc__ and "sight_range2" in CustomRCNNRecurrent.sight.__doc__
    assert "stand and look" not in CustomRCNNRecurrent.clearance.__doc__ and "sight" in CustomRCNNRecurrent.clearance.__doc__


def test_sight_range2():
    from embodied_object_detection_amd.data.robot import RobotFrontEnd
    front = RobotFrontEnd.__new__(RobotFrontEnd)
    front.res = 0.05
    # 0.25 m on a 0.05 m grid is five cells: 25, although 0.25 / 0.05 is not 5 in binary; as body_radius2 rounds
    values = (0.0, 0.05, 0.07, 0.1, 0.25, 0.3, 0.04, 4.0)
    assert [front.sight_range2(v) for v in values] == [0, 1, 1, 4, 25, 36, 0, 6400] == [front.body_radius2(v) for v in values]
    assert isinstance(front.sight_range2(4.0), int)
    front.res = 0.5
    assert [front.sight_range2(v) for v in (0.25, 0.5, 0.75, 1.0, 4.0)] == [0, 1, 2, 4, 64]
    assert front.sight_range2(1e9) == INT_MAX                                     # beyond every map: unbounded
    assert front.relation_metres(np.array([25, INT_MAX], np.int32)).tolist() == [2.5, np.inf]       # near_d2 in metres
