"""The host side of `map_inventory` (no GPU): the reference of `_inventory_cases.py` on a hand-worked map and against the reference
of `map_regions` class by class, what the hostile maps hold, include/eod_inventory.h against its ctypes table, the workspace
formula, and every refused argument (the entry point returns before a launch, so it is callable here)."""
import numpy as np
import pytest

import _inventory_cases as IC
import _regions_cases as RC


def _ref(labels, scores, cols, C, conn, level=0.5, **kw):
    ref = IC.reference(np.asarray(labels, np.int32).reshape(1, -1), np.asarray(scores, np.float32).reshape(1, -1), cols, C, level, conn, **kw)
    return {k: v[0] for k, v in ref.items()}


def test_reference_on_a_hand_worked_3_by_5_map():
    #   cells 0..14, class (score):    0(.9) 0(.8) 1(.6) 1(.7) 2(.5)      cell 6 is below the level, cell 14 carries no class
    #                                  1(.6) 0(.4) 1(.9) 2(.5) 2(.8)      4-connectivity: class 0 {0, 1}, {12}; class 1 {2, 3, 7}, {5, 10, 11};
    #                                  1(.7) 1(.6) 0(.9) 2(1.) -1(.9)     class 2 {4, 8, 9, 13}.  8-connectivity: 7 and 11 join class 1
    lab = [0, 0, 1, 1, 2,
           1, 0, 1, 2, 2,
           1, 1, 0, 2, -1]
    sc = [.9, .8, .6, .7, .5,
          .6, .4, .9, .5, .8,
          .7, .6, .9, 1., .9]
    q24 = lambda *v: sum(int(np.float32(x) * np.float32(2 ** 24)) for x in v)
    f32 = lambda *v: [np.float32(x) for x in v]
    r4 = _ref(lab, sc, 5, 3, 4, topk=6)
    assert r4["object_labels"].tolist() == [0, 0, 2, 2, 4, 5, -1, 2, 4, 4, 5, 5, 12, 4, -1]
    assert r4["count"] == 5 and r4["foreground"] == 13
    assert r4["object"].tolist() == [4, 2, 5, 0, 12, -1] and r4["cls"].tolist() == [2, 1, 1, 0, 0, -1]        # area, then label
    assert r4["area"].tolist() == [4, 3, 3, 2, 1, 0]
    assert r4["bbox"].tolist() == [[0, 3, 2, 4], [0, 2, 1, 3], [1, 0, 2, 1], [0, 0, 0, 1], [2, 2, 2, 2], [0, 0, 0, 0]]
    assert r4["sum_rc"].tolist() == [[4, 14], [1, 7], [5, 1], [0, 1], [2, 2], [0, 0]]
    assert r4["peak"].tolist() == [13, 7, 10, 0, 12, 0]
    assert r4["peak_score"].tolist() == f32(1., .9, .7, .9, .9, 0.)
    assert r4["mass_q24"].tolist() == [q24(.5, .5, .8, 1.), q24(.6, .7, .9), q24(.6, .7, .6), q24(.9, .8), q24(.9), 0]
    assert r4["class_objects"].tolist() == [2, 2, 1] and r4["class_cells"].tolist() == [3, 6, 4]
    assert r4["class_largest"].tolist() == [0, 2, 4] and r4["class_largest_area"].tolist() == [2, 3, 4]
    # min_cells drops small objects from the count, the ranking and class_objects; the label map and class_cells keep their cells
    m2 = _ref(lab, sc, 5, 3, 4, topk=6, min_cells=2)
    assert m2["count"] == 4 and m2["object"].tolist() == [4, 2, 5, 0, -1, -1] and m2["cls"].tolist() == [2, 1, 1, 0, -1, -1]
    assert m2["class_objects"].tolist() == [1, 2, 1] and m2["class_cells"].tolist() == [3, 6, 4]
    assert m2["object_labels"].tolist() == r4["object_labels"].tolist() and m2["foreground"] == 13
    m4 = _ref(lab, sc, 5, 3, 4, topk=2, min_cells=4)
    assert m4["count"] == 1 and m4["object"].tolist() == [4, -1] and m4["class_objects"].tolist() == [0, 0, 1]
    assert m4["class_largest"].tolist() == [-1, -1, 4] and m4["class_largest_area"].tolist() == [0, 0, 4]
    r8 = _ref(lab, sc, 5, 3, 8, topk=2)
    assert r8["object_labels"].tolist() == [0, 0, 2, 2, 4, 2, -1, 2, 4, 4, 2, 2, 12, 4, -1]
    assert r8["count"] == 4 and r8["object"].tolist() == [2, 4] and r8["cls"].tolist() == [1, 2] and r8["area"].tolist() == [6, 4]
    assert r8["bbox"][0].tolist() == [0, 0, 2, 3] and r8["sum_rc"][0].tolist() == [6, 8] and r8["peak"][0] == 7
    assert r8["class_objects"].tolist() == [2, 1, 1] and r8["class_largest"].tolist() == [0, 2, 4]             # topk does not cut the table
    # a keep table that leaves class 1 out
    k = _ref(lab, sc, 5, 3, 8, topk=4, keep=np.array([1, 0, 1], np.uint8))
    assert k["foreground"] == 7 and k["object"].tolist() == [4, 0, 12, -1] and k["class_cells"].tolist() == [3, 0, 4]
    assert k["object_labels"].tolist() == [0, 0, -1, -1, 4, -1, -1, -1, 4, 4, -1, -1, 12, 4, -1]
    # with two classes only, the cells of class 2 are background
    c2 = _ref(lab, sc, 5, 2, 4, topk=4)
    assert c2["foreground"] == 9 and c2["object"].tolist() == [2, 5, 0, 12] and c2["class_cells"].tolist() == [3, 6]


def test_each_class_of_the_reference_is_the_regions_reference_on_that_class():
    rows, cols, C = 21, 37, 4
    for seed, p in enumerate((0.4, 0.7, 0.95)):
        labels = IC.random_classes(rows * cols, C, 300 + seed)
        labels[np.random.default_rng(seed).random(rows * cols) < 0.1] = -1
        scores = RC.paint(RC.bernoulli(rows, cols, p, seed=310 + seed), 0.5, seed=seed)
        for conn in (4, 8):
            for min_cells in (1, 3):
                K = 1024                                                      # the references themselves have no limit
                inv = {k: v[0] for k, v in IC.reference(labels[None], scores[None], cols, C, 0.5, conn, min_cells, K).items()}
                assert inv["count"] <= K, "the ranking must hold every object for this comparison"
                prob = np.stack([np.where(labels == c, scores, np.float32(0)) for c in range(C)]).astype(np.float32)
                reg = RC.reference(prob, cols, 0.5, conn, min_cells, K)
                assert inv["count"] == reg["count"].sum() and inv["foreground"] == reg["foreground"].sum()
                for c in range(C):
                    mine = inv["object_labels"].copy()
                    mine[labels != c] = -1
                    assert np.array_equal(mine, reg["region_labels"][c]), (seed, conn, c)
                    n = int(reg["count"][c])
                    assert inv["class_objects"][c] == n and inv["class_cells"][c] == reg["foreground"][c]
                    assert inv["class_largest"][c] == reg["region"][c, 0] and inv["class_largest_area"][c] == reg["area"][c, 0]
                    got = IC.restricted(inv, c)
                    for k, v in got.items():
                        assert len(v) == n and np.array_equal(v.view(np.int32) if v.dtype == np.float32 else v,
                                                              reg[k][c, :n].view(np.int32) if v.dtype == np.float32 else reg[k][c, :n]), (k, c)
                # the slots of all classes together are in the order (area descending, label ascending)
                n = int(inv["count"])
                keys = list(zip((-inv["area"][:n]).tolist(), inv["object"][:n].tolist()))
                assert keys == sorted(keys) and (inv["object"][n:] == -1).all() and (inv["cls"][n:] == -1).all()


def test_hostile_maps_hold_what_their_names_say():
    rows, cols, tr, tc = 21, 37, 8, 16
    maps = IC.hostile_maps(rows, cols, tr, tc)
    N = rows * cols

    def one(name, conn, **kw):
        lab, sc, keep = maps[name]
        return _ref(lab, sc, cols, IC.C5, conn, keep=keep, **kw)

    cb = one("checkerboard", 8)
    assert cb["count"] == 2 and cb["object"][:2].tolist() == [0, 1] and cb["cls"][:2].tolist() == [1, 3]
    assert cb["class_objects"].tolist() == [0, 1, 0, 1, 0]
    cb = one("checkerboard", 4)
    assert cb["count"] == N and (cb["area"] == 1).all() and cb["object"].tolist() == list(range(16))
    for conn in (4, 8):
        st = one("column stripes", conn)
        assert st["count"] == 3 and st["class_objects"].tolist() == [2, 1, 0, 0, 0] and st["foreground"] == N       # 16 + 16 + 5 columns
        assert st["area"][:3].tolist() == [16 * rows, 16 * rows, 5 * rows] and st["object"][:3].tolist() == [0, 16, 32]
        assert one("row stripes", conn)["count"] == 3
        assert one("row-end pair", conn)["count"] == 2
        assert one("one class everywhere", conn)["area"][0] == N
        cut = one("keep cuts", conn)
        assert cut["count"] == 2 and cut["class_cells"].tolist() == [N - rows, 0, 0, 0, 0] and cut["foreground"] == N - rows
        assert one("serpentine", conn)["count"] > 8 and one("spirals", conn)["count"] > 8
    # the anti-diagonal tiles of the blocks carry one class and meet at a corner only
    assert one("tile blocks", 8)["count"] < one("tile blocks", 4)["count"]
    for name in ("corner, both diagonals", "corner, class all around"):
        d8, d4 = one(name, 8), one(name, 4)
        assert d8["count"] == 2 and d8["area"][:2].tolist() == [2, 2] and d8["cls"][:2].tolist() == [2, 4] and d4["count"] == 4, name
        assert d8["object"][:2].tolist() == [(tr - 1) * cols + tc - 1, (tr - 1) * cols + tc]
    bg = one("all background", 8)
    assert bg["count"] == 0 and (bg["object"] == -1).all() and (bg["object_labels"] == -1).all() and not bg["class_cells"].any()
    assert (bg["class_largest"] == -1).all()
    assert one("at the level", 8)["foreground"] > 300 and one("below the level", 8)["foreground"] == 0
    lab, sc, _ = maps["nan"]
    assert np.isnan(sc).sum() > 30 and (one("nan", 8)["object_labels"][np.isnan(sc)] == -1).all()
    lab, sc, _ = maps["labels that are no class"]
    bad = one("labels that are no class", 8)
    for v in (-1, IC.C5, -7, IC.INT_MAX):
        assert (lab == v).sum() > 20 and (bad["object_labels"][lab == v] == -1).all(), v
    assert bad["foreground"] == ((lab >= 0) & (lab < IC.C5)).sum()
    kr = one("keep on random classes", 8)
    assert kr["class_cells"][0] == 0 and kr["class_cells"][3] == 0 and kr["class_cells"][1] > 0
    # equal areas: the lower label first, whatever its class; class_largest is the class's lowest label
    eq = one("equal areas", 4, topk=8)
    assert (eq["area"] == 4).all() and eq["object"].tolist() == [0, 3, 6, 9, 12, 15, 18, 21] and eq["cls"].tolist() == [3, 1, 4, 1, 0, 3, 2, 3]
    assert eq["class_largest"].tolist() == [12, 3, 18, 0, 6] and eq["count"] > 64
    # min_cells above some areas: their cells stay in class_cells, their objects leave class_objects
    lo, hi = one("bernoulli 0.3", 4, min_cells=1), one("bernoulli 0.3", 4, min_cells=3)
    assert hi["count"] < lo["count"] and np.array_equal(hi["class_cells"], lo["class_cells"]) and (hi["class_objects"] < lo["class_objects"]).all()
    assert lo["count"] > 64                                                       # more objects than any topk
    pl = one("plateau", 4)
    assert pl["count"] == 3 and pl["peak"][:3].tolist() == [cols + cols // 3 + 1, cols, cols + cols // 3]


def test_inventory_header_and_ctypes_table_agree():
    """include/eod_inventory.h against `_lib.INVENTORY_SIGNATURES`: the same entry points on both sides, every one exported by the
    library, none of them in the other three tables or headers; the header's constants are the binding's."""
    import os
    import re
    import shutil
    import subprocess
    import tempfile
    import __graft_entry__
    __graft_entry__.build()
    from embodied_object_detection_amd import _lib, build, ops
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    path = os.path.join(root, "include", "eod_inventory.h")
    txt = open(path).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    declared = sorted(set(re.findall(r"^(?:int|size_t)\s+(eod_\w+)\s*\(", code, flags=re.M)))
    assert declared == sorted(_lib.INVENTORY_SIGNATURES) == ["eod_map_inventory", "eod_map_inventory_workspace_bytes"]
    assert not set(_lib.INVENTORY_SIGNATURES) & (set(_lib.SIGNATURES) | set(_lib.PLACE_SIGNATURES) | set(_lib.REGIONS_SIGNATURES))
    assert len(_lib.SIGNATURES) == 75 and len(_lib.PLACE_SIGNATURES) == 2 and len(_lib.REGIONS_SIGNATURES) == 2
    for other in ("eod_hip.h", "eod_place.h", "eod_regions.h"):
        assert "eod_map_inventory" not in open(os.path.join(root, "include", other)).read()
    lib = _lib.load()
    for name, (res, args) in _lib.INVENTORY_SIGNATURES.items():
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == list(args), name
    val = lambda name: int(re.search(rf"#define {name} (\d+)", txt).group(1))
    assert (ops.INVENTORY_B_MAX, ops.INVENTORY_C_MAX, ops.INVENTORY_TOPK_MAX, ops.INVENTORY_N_MAX) == (
        val("EOD_INVENTORY_B_MAX"), val("EOD_INVENTORY_C_MAX"), val("EOD_INVENTORY_TOPK_MAX"), val("EOD_INVENTORY_N_MAX")) == (32, 2047, 64, 2 ** 22)
    assert "inventory.hip" in build.SOURCES and "regions.hip" in build.SOURCES
    gcc = shutil.which("gcc")                                                    # the header compiles as C on its own
    if gcc is not None:
        with tempfile.TemporaryDirectory() as d:
            src = os.path.join(d, "t.c")
            open(src, "w").write(f'#include "{path}"\n'
                                 "int main(void) { return EOD_INVENTORY_OUT_WORDS(3, 16, 20) == 2 + 6 + 15 * 48 + 4 * 60 ? 0 : 1; }\n")
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
    wsb = lib.eod_map_inventory_workspace_bytes
    assert wsb(3, 437, 20, 16) == up256(3 * 3 * 437 * 4) + 3 * 16 * 8 + 3 * 20 * 8          # parent, area, slot; peak keys; class keys
    assert wsb(2, 40000, 1203, 16) == 3 * 2 * 40000 * 4 + 2 * 16 * 8 + 2 * 1203 * 8
    # the largest call the limits allow: 3 * 2^29 bytes of arrays and the keys, beyond 2^30.  (With B <= 32 and N <= 2^22 no call
    # reaches 2^31 bytes; the function answers in size_t all the same.)
    big = wsb(32, 2 ** 22, 2047, 64)
    assert big == 3 * 32 * 2 ** 22 * 4 + 32 * 64 * 8 + 32 * 2047 * 8 and big > 2 ** 30 + 2 ** 29
    assert ops.map_inventory_workspace(3, 437, 20, 16) == wsb(3, 437, 20, 16) // 4
    for bad in ((0, 437, 20, 16), (33, 437, 20, 16), (3, 0, 20, 16), (3, 2 ** 22 + 1, 20, 16), (3, 437, 0, 16), (3, 437, 2048, 16),
                (3, 437, 20, 0), (3, 437, 20, 65), (-1, -1, -1, -1), (2 ** 16, 2 ** 16, 1, 1)):       # the last: dimensions whose product is beyond 2^31 bytes
        assert wsb(*bad) == 0, bad
        with pytest.raises(_lib.EodError):
            ops.map_inventory_workspace(*bad)
    need = wsb(3, 437, 20, 16)

    def call(labels=p, scores=p, keep=p, B=3, N=437, cols=23, Cn=20, level=0.5, conn=8, min_cells=1, K=16, obj=p, out=p, ws=p, ws_bytes=need):
        return lib.eod_map_inventory(labels, scores, keep, B, N, cols, Cn, level, conn, min_cells, K, obj, out, ws, ws_bytes, None)

    for kw in (dict(B=0), dict(B=33), dict(B=-1), dict(Cn=0), dict(Cn=2048), dict(Cn=-5), dict(K=0), dict(K=65), dict(conn=6), dict(conn=0),
               dict(min_cells=0), dict(min_cells=-3), dict(cols=0), dict(cols=-23), dict(cols=20), dict(N=0), dict(N=2 ** 22 + 1, cols=1),
               dict(level=0.0), dict(level=-0.5), dict(level=float("nan")), dict(level=float("inf")), dict(level=1.0000001), dict(level=1e-50)):
        assert call(**kw) == BAD, kw
    # a bad dimension wins over everything a launch would need
    assert call(B=0, labels=None, scores=None, obj=None, out=None, ws=None, ws_bytes=0) == BAD
    assert call(level=0.0, labels=p + 1, ws_bytes=0) == BAD
    for kw in (dict(labels=None), dict(scores=None), dict(obj=None), dict(out=None), dict(ws=None)):
        assert call(**kw) == NULL, kw
    for kw in (dict(labels=p + 2), dict(scores=p + 1), dict(obj=p + 3), dict(out=p + 4), dict(ws=p + 4)):
        assert call(**kw) == ALIGN, kw
    assert call(ws_bytes=need - 1) == CAP and call(ws_bytes=0) == CAP
    assert call(keep=None, ws_bytes=need - 1) == CAP                               # keep may be null
    assert call(keep=p + 1, ws_bytes=need - 1) == CAP                              # and has no alignment
    assert call(N=2 ** 22, cols=2048, ws_bytes=need) == CAP                        # the largest N is a dimension it takes
    assert call(Cn=2047, K=64, ws_bytes=need) == CAP


def test_op_refuses_on_the_host_naming_the_argument():
    import torch
    import __graft_entry__
    __graft_entry__.build()
    from embodied_object_detection_amd import _lib, ops
    labels, scores = torch.zeros((2, 12), dtype=torch.int32), torch.zeros((2, 12))
    ok = dict(cols=4, num_classes=5, level=0.5)
    for name, kw in (("level", dict(level=0.0)), ("level", dict(level=float("nan"))), ("level", dict(level=1.5)), ("level", dict(level=1e-50)),
                     ("connectivity", dict(connectivity=6)), ("min_cells", dict(min_cells=0)), ("topk", dict(topk=0)),
                     ("topk", dict(topk=65)), ("cols", dict(cols=5)), ("cols", dict(cols=0)), ("num_classes", dict(num_classes=0)),
                     ("num_classes", dict(num_classes=2048)), ("num_classes", dict(num_classes=2.5)),
                     ("keep", dict(keep=torch.ones(4, dtype=torch.uint8))), ("keep", dict(keep=torch.ones(5))),
                     ("keep", dict(keep=np.ones(5, np.uint8))), ("keep", dict(keep=torch.ones((1, 5), dtype=torch.uint8)))):
        with pytest.raises(_lib.EodError, match=name):
            ops.map_inventory(labels, scores, **{**ok, **kw})
    for bad in (torch.zeros((33, 12), dtype=torch.int32), torch.zeros((0, 12), dtype=torch.int32), torch.zeros((2, 2, 3), dtype=torch.int32),
                torch.zeros((2, 12), dtype=torch.int64), torch.zeros((12, 2), dtype=torch.int32).t(), np.zeros((2, 12), np.int32)):
        with pytest.raises(_lib.EodError, match="labels"):
            ops.map_inventory(bad, scores, **ok)
    for bad in (torch.zeros((2, 11)), torch.zeros((12,)), torch.zeros((2, 12), dtype=torch.float64), torch.zeros((12, 2)).t(),
                np.zeros((2, 12), np.float32)):
        with pytest.raises(_lib.EodError, match="scores"):
            ops.map_inventory(labels, bad, **ok)
    # a workspace that is too small, or 4 bytes off an 8-byte boundary
    need = ops.map_inventory_workspace(2, 12, 5, 16)
    assert need == ((3 * 2 * 12 * 4 + 255) // 256 * 256 + 2 * 16 * 8 + 2 * 5 * 8) // 4
    ws = torch.zeros((need + 2,), dtype=torch.int32)
    assert ws.data_ptr() % 8 == 0
    for bad in (ws[:need - 1], ws[1:], ws.to(torch.float32), ws.view(2, -1)):
        with pytest.raises(_lib.EodError, match="workspace"):
            ops.map_inventory(labels, scores, workspace=bad, **ok)
    with pytest.raises(_lib.EodError, match="no CPU fallback"):                   # tensors on the host
        ops.map_inventory(labels, scores, **ok)
    with pytest.raises(_lib.EodError, match="no CPU fallback"):
        ops.map_inventory(labels[0], scores[0], keep=torch.ones(5, dtype=torch.uint8), **ok)
