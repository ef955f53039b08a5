"""The host side of `describe_pool` and `describe_classify` (no GPU): the reference of `_describe_cases.py` on hand-worked inputs,
include/eod_describe.h against its ctypes table and the cross-compiled library, the build's records, and every refused argument (the
entry points return before a launch, so they are callable here)."""
import numpy as np
import pytest

import _describe_cases as DC


def test_reference_lowest_slot_wins_and_unasked_labels_are_skipped():
    labels = np.array([5, 3, -1, 5, 9, 2 ** 31 - 1, -7, 3], np.int32)
    assert DC.slots(labels, np.array([3, 5, 3, -1, 9], np.int32)).tolist() == [1, 0, -1, 1, 4, -1, -1, 0]
    assert DC.slots(labels, np.array([-1, -7, 2 ** 31 - 1], np.int32)).tolist() == [-1, -1, -1, -1, -1, 2, -1, -1]       # -7 names nothing
    mem, q = DC.exact_rows(8, seed=3)
    sum_q, cells = DC.exact_pool(q, labels, np.array([3, 5, 3, -1, 9], np.int32))
    assert cells.tolist() == [2, 2, 0, 0, 1] and not sum_q[2].any() and not sum_q[3].any()
    assert np.array_equal(sum_q[0], q[1] + q[7]) and np.array_equal(sum_q[1], q[0] + q[3]) and np.array_equal(sum_q[4], q[4])


def test_reference_exact_rows_are_what_float64_gives():
    mem, q = DC.exact_rows(400, seed=1)
    x = DC.unit_rows64(mem)
    # float64 holds every x of the four kinds but for the relative 2^-63 that the small element of kind 3 adds to the norm
    assert np.array_equal(np.trunc(np.round(x * DC.Q30, 6)).astype(np.int64), q)
    assert set(np.unique(np.abs(q))) == {0, DC.Q30 >> 2, DC.Q30 >> 1, DC.Q30}
    small = (mem != 0) & (q == 0)
    assert small.sum() > 50 and np.allclose(np.abs(x[small]) * DC.Q30, 0.75)              # the elements that tell truncation from rounding
    assert (x[small] < 0).sum() > 10 and (x[small] > 0).sum() > 10


def test_reference_coherence_and_embedding():
    rng = np.random.default_rng(0)
    row = rng.standard_normal(DC.D)
    unit = row / np.linalg.norm(row)
    q = np.trunc(unit * DC.Q30).astype(np.int64)
    emb, coh = DC.finish64(np.stack([q * 7, q - q, q * 3, q]), np.array([7, 4, 3, 0], np.int32))          # identical rows; zeros; no cells
    assert abs(coh[0] - 1.0) < 1e-8 and abs(coh[2] - 1.0) < 1e-8 and np.allclose(emb[0], unit, atol=1e-8)
    assert coh[1] == 0.0 and not emb[1].any() and coh[3] == 0.0 and not emb[3].any()
    # two opposite rows cancel; two orthogonal unit rows give 1 / sqrt(2)
    e0, e1 = np.zeros(DC.D, np.int64), np.zeros(DC.D, np.int64)
    e0[3], e1[400] = DC.Q30, DC.Q30
    emb, coh = DC.finish64(np.stack([e0 - e0, e0 + e1]), np.array([2, 2], np.int32))
    assert coh[0] == 0.0 and abs(coh[1] - 0.5 ** 0.5) < 1e-15 and abs(emb[1, 3] - 0.5 ** 0.5) < 1e-15
    # non-finite rows give zeros, rows below the clamp are divided by it
    mem = np.zeros((4, DC.D), np.float32)
    mem[0, 5], mem[1, 6], mem[2, 7], mem[3, 8] = np.inf, np.nan, 1e-20, 2.0
    mem[0, 9] = mem[1, 9] = 1.0
    x = DC.unit_rows64(mem)
    assert not x[0].any() and not x[1].any() and x[3, 8] == 1.0 and x[2, 7] == float(np.float32(1e-20)) / float(DC.TINY)
    tot, mag, cells = DC.pool64(mem, np.array([1, 1, 0, 1], np.int32), np.array([1], np.int32))
    assert cells.tolist() == [3] and tot[0, 8] == 1.0 and tot[0].sum() == 1.0


def test_reference_softmax_and_topn():
    rng = np.random.default_rng(1)
    e = rng.standard_normal((3, DC.D)).astype(np.float32)
    e /= np.linalg.norm(e, axis=1, keepdims=True)
    e[1] = 0
    zs = rng.standard_normal((DC.D, 8)).astype(np.float32) * 0.05
    zs[:, 7] = 100.0                                                              # the background column never enters
    zs[:, 5] = zs[:, 2]                                                           # two equal columns
    L, B, p = DC.classify64(e, zs)
    assert p.shape == (3, 7) and np.allclose(p[[0, 2]].sum(axis=1), 1.0) and not p[1].any() and (B[[0, 2]] > 0).all()
    assert np.array_equal(p[:, 5], p[:, 2])
    cls, val = DC.topn(p, 7)
    for k in (0, 2):
        assert sorted(cls[k].tolist()) == list(range(7)) and (np.diff(val[k]) <= 0).all()
        at = cls[k].tolist()
        assert at.index(2) + 1 == at.index(5)                                     # the lower class first
    assert DC.topn(np.array([[0.25, 0.5, 0.25, 0.0]], np.float32), 3)[0].tolist() == [[1, 0, 2]]


def test_describe_header_and_ctypes_table_agree():
    """include/eod_describe.h against `_lib.DESCRIBE_SIGNATURES`: the same entry points on both sides, both exported by the
    cross-compiled library, none of them in the other tables or headers; the header's constants are the binding's."""
    import os
    import re
    import shutil
    import subprocess
    import tempfile
    import __graft_entry__
    __graft_entry__.build()
    from embodied_object_detection_amd import _lib, build, ops
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    path = os.path.join(root, "include", "eod_describe.h")
    txt = open(path).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    declared = sorted(set(re.findall(r"^(?:int|size_t)\s+(eod_\w+)\s*\(", code, flags=re.M)))
    assert declared == sorted(_lib.DESCRIBE_SIGNATURES) == ["eod_describe_classify", "eod_describe_pool"]
    others = set(_lib.SIGNATURES) | set(_lib.PLACE_SIGNATURES) | set(_lib.REGIONS_SIGNATURES) | set(_lib.INVENTORY_SIGNATURES)
    assert not set(_lib.DESCRIBE_SIGNATURES) & others
    for other in ("eod_hip.h", "eod_place.h", "eod_regions.h", "eod_inventory.h"):
        assert "eod_describe" not in open(os.path.join(root, "include", other)).read()
    # the number of arguments of each declaration is the table's
    for name, (res, args) in _lib.DESCRIBE_SIGNATURES.items():
        params = re.search(rf"\b{name}\s*\(([^)]*)\)", code, flags=re.S).group(1)
        assert len(params.split(",")) == len(args), name
    lib = _lib.load()
    for name, (res, args) in _lib.DESCRIBE_SIGNATURES.items():
        fn = getattr(lib, name)                                                  # exported by the library built for gfx950
        assert fn.restype is res and list(fn.argtypes) == list(args), name
    val = lambda name: int(re.search(rf"#define {name} (\d+)", txt).group(1))
    assert (ops.DESCRIBE_D, ops.DESCRIBE_K_MAX, ops.DESCRIBE_N_MAX, ops.DESCRIBE_C_MAX, ops.DESCRIBE_TOPN_MAX) == (
        val("EOD_DESCRIBE_D"), val("EOD_DESCRIBE_K_MAX"), val("EOD_DESCRIBE_N_MAX"), val("EOD_DESCRIBE_C_MAX"),
        val("EOD_DESCRIBE_TOPN_MAX")) == (512, 64, 2 ** 22, 2047, 8)
    assert "describe.hip" in build.SOURCES
    gcc = shutil.which("gcc")                                                    # the header compiles as C on its own
    if gcc is not None:
        with tempfile.TemporaryDirectory() as d:
            src = os.path.join(d, "t.c")
            open(src, "w").write(f'#include "{path}"\nint main(void) {{ return EOD_DESCRIBE_K_MAX == 64 ? 0 : 1; }}\n')
            subprocess.run([gcc, "-std=c11", "-Wall", "-Werror", "-o", os.path.join(d, "t"), src], check=True)
            assert subprocess.run([os.path.join(d, "t")]).returncode == 0


def test_describe_kernels_use_no_scratch():
    import __graft_entry__
    __graft_entry__.build()
    from embodied_object_detection_amd import build
    usage = build.resource_usage()
    if not any("describe_" in k for k in usage):   # a library built elsewhere, without the remarks: build them here
        build.build(force=True, verbose=False)
        usage = build.resource_usage()
    mine = {k: v for k, v in usage.items() if "describe_" in k}
    assert sorted(n for k in mine for n in ("init", "pool", "finish", "classify") if f"describe_{n}_kernel" in k) == [
        "classify", "finish", "init", "pool"], sorted(mine)
    assert not [k for k in build.scratch_offenders(usage) if "describe_" in k]
    assert all(v.get("scratch", 0) == 0 for v in mine.values())
    pool = next(v for k, v in mine.items() if "describe_pool_kernel" in k)
    assert pool["lds"] == 0 and pool["vgprs"] <= 64, pool                          # eight waves per SIMD


def test_entry_points_refuse_bad_arguments_before_any_launch():
    import ctypes as C
    import __graft_entry__
    __graft_entry__.build()
    from embodied_object_detection_amd import _lib
    lib = _lib.load()
    buf = (C.c_int64 * 4096)()
    p = C.addressof(buf)
    p += (-p) % 16
    BAD, ALIGN, NULL = -1, -2, -4

    def pool(mem=p, labels=p, objects=p, N=100, K=5, sum_q=p, cells=p, emb=p, coh=p):
        return lib.eod_describe_pool(mem, labels, objects, N, K, sum_q, cells, emb, coh, None)

    for kw in (dict(K=0), dict(K=65), dict(K=-1), dict(N=0), dict(N=2 ** 22 + 1), dict(N=-5)):
        assert pool(**kw) == BAD, kw
    # a bad dimension wins over everything a launch would need
    assert pool(K=0, mem=None, labels=None, objects=None, sum_q=None, cells=None, emb=None, coh=None) == BAD
    assert pool(N=2 ** 22 + 1, mem=p + 4, sum_q=p + 4) == BAD
    for name in ("mem", "labels", "objects", "sum_q", "cells", "emb", "coh"):
        assert pool(**{name: None}) == NULL, name
        assert pool(**{name: None, "mem" if name != "mem" else "emb": p + 1}) == NULL, name          # null wins over alignment
    for kw in (dict(mem=p + 4), dict(mem=p + 8), dict(labels=p + 2), dict(objects=p + 1), dict(sum_q=p + 4), dict(cells=p + 3),
               dict(emb=p + 8), dict(coh=p + 2)):
        assert pool(**kw) == ALIGN, kw

    def classify(emb=p, zs=p, K=5, C1=21, topn=5, prob=p, top_cls=p, top_prob=p):
        return lib.eod_describe_classify(emb, zs, K, C1, topn, prob, top_cls, top_prob, None)

    for kw in (dict(K=0), dict(K=65), dict(C1=1), dict(C1=0), dict(C1=2049), dict(C1=-3), dict(topn=0), dict(topn=9), dict(topn=-1),
               dict(C1=4, topn=4), dict(C1=2, topn=2), dict(C1=-2 ** 31, topn=1)):
        assert classify(**kw) == BAD, kw
    assert classify(K=65, emb=None, zs=None, prob=None, top_cls=None, top_prob=None) == BAD
    assert classify(topn=9, emb=p + 4) == BAD
    for name in ("emb", "zs", "prob", "top_cls", "top_prob"):
        assert classify(**{name: None}) == NULL, name
    assert classify(zs=None, emb=p + 4) == NULL
    for kw in (dict(emb=p + 4), dict(emb=p + 8), dict(zs=p + 2), dict(prob=p + 1), dict(top_cls=p + 3), dict(top_prob=p + 2)):
        assert classify(**kw) == ALIGN, kw


def test_ops_refuse_on_the_host_naming_the_argument():
    import torch
    import __graft_entry__
    __graft_entry__.build()
    from embodied_object_detection_amd import _lib, ops
    mem, labels, objects = torch.zeros((12, 512)), torch.zeros((12,), dtype=torch.int32), torch.zeros((5,), dtype=torch.int32)
    for bad in (torch.zeros((12, 511)), torch.zeros((0, 512)), torch.zeros((12, 512), dtype=torch.float64), torch.zeros((512, 12)).t(),
                torch.zeros((12, 1024))[:, ::2], torch.zeros((2, 6, 512)), np.zeros((12, 512), np.float32),
                torch.zeros((12 * 512 + 1,))[1:].view(12, 512)):                  # 4 bytes off a 16-byte boundary
        with pytest.raises(_lib.EodError, match="mem"):
            ops.describe_pool(bad, labels, objects)
    with pytest.raises(_lib.EodError, match="mem: N 4194305"):                    # no storage behind it: refused by its shape
        ops.describe_pool(torch.empty((2 ** 22 + 1, 512), device="meta"), labels, objects)
    for bad in (torch.zeros((11,), dtype=torch.int32), torch.zeros((12,), dtype=torch.int64), torch.zeros((12, 1), dtype=torch.int32),
                torch.zeros((24,), dtype=torch.int32)[::2], np.zeros(12, np.int32)):
        with pytest.raises(_lib.EodError, match="object_labels"):
            ops.describe_pool(mem, bad, objects)
    for bad in (torch.zeros((0,), dtype=torch.int32), torch.zeros((65,), dtype=torch.int32), torch.zeros((5,), dtype=torch.int64),
                torch.zeros((1, 5), dtype=torch.int32), torch.zeros((10,), dtype=torch.int32)[::2], [1, 2, 3]):
        with pytest.raises(_lib.EodError, match="objects"):
            ops.describe_pool(mem, labels, bad)
    with pytest.raises(_lib.EodError, match="no CPU fallback"):                   # tensors on the host: refused last
        ops.describe_pool(mem, labels, objects)
    emb, zs = torch.zeros((5, 512)), torch.zeros((512, 21))
    for bad in (torch.zeros((0, 512)), torch.zeros((65, 512)), torch.zeros((5, 256)), torch.zeros((5, 512), dtype=torch.float16),
                torch.zeros((512, 5)).t(), torch.zeros((512,)), np.zeros((5, 512), np.float32)):
        with pytest.raises(_lib.EodError, match="embedding"):
            ops.describe_classify(bad, zs)
    for bad in (torch.zeros((512, 1)), torch.zeros((512, 2049)), torch.zeros((511, 21)), torch.zeros((512, 21), dtype=torch.float64),
                torch.zeros((21, 512)).t(), torch.zeros((512,)), np.zeros((512, 21), np.float32)):
        with pytest.raises(_lib.EodError, match="zs"):
            ops.describe_classify(emb, bad)
    for bad, z in ((0, zs), (9, zs), (-1, zs), (2.5, zs), (True, zs), (4, torch.zeros((512, 4))), (2, torch.zeros((512, 2)))):
        with pytest.raises(_lib.EodError, match="topn"):
            ops.describe_classify(emb, z, topn=bad)
    with pytest.raises(_lib.EodError, match="no CPU fallback"):
        ops.describe_classify(emb, zs)
    with pytest.raises(_lib.EodError, match="no CPU fallback"):
        ops.describe_classify(emb, torch.zeros((512, 2048)), topn=8)              # the largest vocabulary is one it takes
