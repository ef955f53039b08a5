"""EOD_SEMMAP_SCORES on `eod_semmap_labels` (the memory read as a map in any vocabulary, with a confidence): the flag's value in
the header and in the ctypes layer, and the host-side argument checks, which answer before any device work."""
import os
import re

from embodied_object_detection_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK_PTR = 0x1000          # never dereferenced: every call below is refused on the host
BAD_DIMS, ALIGN, NULL, CAPACITY = -1, -2, -4, -5


def _call(lib, D, C1, mem=OK_PTR, obs=OK_PTR, zs=OK_PTR, labels=OK_PTR, ws=OK_PTR, n_cells=100):
    return lib.eod_semmap_labels(mem, obs, zs, n_cells, D, C1, 0.4, labels, ws, None)


def test_flag_value_in_header_and_ctypes_layer():
    text = open(os.path.join(ROOT, "include", "eod_hip.h")).read()
    m = re.search(r"^#define\s+EOD_SEMMAP_SCORES\s+(\S+)", text, re.M)
    assert m, "include/eod_hip.h does not define EOD_SEMMAP_SCORES"
    assert int(m.group(1), 0) == 0x10000
    assert _lib.SEMMAP_SCORES == 0x10000
    assert _lib.load().eod_abi_version() == 1


def test_flagged_call_is_checked_on_the_host():
    lib = _lib.load()
    F = _lib.SEMMAP_SCORES
    assert _call(lib, 512 | F, 4096) == CAPACITY            # without the feature: BAD_DIMS (D != 512)
    assert _call(lib, 512 | F, 2049) == CAPACITY
    assert _call(lib, 256 | F, 21) == BAD_DIMS
    assert _call(lib, 512 | F | 0x20000, 21) == BAD_DIMS     # no other bit of D means anything
    assert _call(lib, 512 | F, 1) == BAD_DIMS
    assert _call(lib, 512 | F, 21, n_cells=0) == BAD_DIMS
    assert _call(lib, 512 | F, 21, ws=None) == NULL
    for name in ("mem", "obs", "zs", "labels"):
        assert _call(lib, 512 | F, 21, **{name: None}) == NULL, name
    assert _call(lib, 512 | F, 21, zs=OK_PTR + 2) == ALIGN
    assert _call(lib, 256 | F, 4096, ws=None) == NULL       # null pointers are reported first, as without the flag


def test_unflagged_call_answers_as_before():
    lib = _lib.load()
    assert _call(lib, 512, 1) == BAD_DIMS
    assert _call(lib, 512, 0) == BAD_DIMS
    assert _call(lib, 256, 21) == BAD_DIMS
    assert _call(lib, 512, 21, n_cells=0) == BAD_DIMS
    assert _call(lib, 512, 21, ws=None) == NULL
    assert _call(lib, 512 | 0x20000, 21) == BAD_DIMS
