"""The locate query off the GPU: the exact peak reference of `_locate_cases.py` on hand-written maps with known answers, the mode bits
of `eod_semmap_labels` in the header and in the ctypes layer, the host's answer to every bit combination that means nothing, and
`RobotFrontEnd.cell_center` as the inverse of `robot_cell`."""
import os
import re

import numpy as np

from _locate_cases import peak_flags, peaks_reference
from embodied_object_detection_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK_PTR = 0x1000          # never dereferenced: every call below is refused on the host
BAD_DIMS, NULL = -1, -4


def _map(rows):
    return np.asarray(rows, dtype=np.float32).reshape(1, -1)


def test_peaks_of_a_hand_written_map():
    # 4 x 5, cell = r * 5 + c
    prob = _map([[0.9, 0.1, 0.0, 0.2, 0.8],
                 [0.1, 0.1, 0.0, 0.1, 0.3],
                 [0.0, 0.0, 0.5, 0.0, 0.0],
                 [0.7, 0.0, 0.0, 0.0, 0.6]])
    # radius 1: the corners 0 (0.9), 4 (0.8), 15 (0.7), 19 (0.6) see only their clipped windows; 12 (0.5) beats its eight neighbours
    peaks, scores = peaks_reference(prob, 5, 1, 8)
    assert peaks.tolist() == [[0, 4, 15, 19, 12, -1, -1, -1]]
    assert scores.tolist() == [[np.float32(v) for v in (0.9, 0.8, 0.7, 0.6, 0.5)] + [0.0] * 3]
    # radius 2: 12's window now holds every larger corner; the corners do not see one another (3 or 4 cells apart)
    assert peaks_reference(prob, 5, 2, 4)[0].tolist() == [[0, 4, 15, 19]]
    # radius 3: 0 sees 15 and 19? rows 0..3, columns 0..3: 15 yes (3 rows down), 19 no (4 columns away)
    assert peaks_reference(prob, 5, 3, 4)[0].tolist() == [[0, 4, -1, -1]]
    # radius 0: the plain top-K of the positive cells, ties by the lower cell (the 0.1s: 1, 5, 6, 8)
    top, val = peaks_reference(prob, 5, 0, 12)
    assert top.tolist() == [[0, 4, 15, 19, 12, 9, 3, 1, 5, 6, 8, -1]]
    assert peaks_reference(prob, None, 1, 12)[0].tolist() == top.tolist()
    # the same values as a 5 x 4 grid, cell = r * 4 + c: 0.9 at (0, 0) hides 0.8 at (1, 0); 0.7 at (3, 3) hides 0.6 at (4, 3); 0.5 at
    # (3, 0) and 0.2 at (0, 3) now stand alone; 0.3 at (2, 1) touches the 0.8
    assert peaks_reference(prob, 4, 1, 6)[0].tolist() == [[0, 15, 12, 3, -1, -1]]
    flags = peak_flags(prob[0], 4, 1)
    assert flags.nonzero()[0].tolist() == [0, 3, 12, 15]


def test_equal_values_give_the_lowest_cell():
    prob = _map([[0.0, 0.0, 0.0, 0.0, 0.0],
                 [0.0, 0.4, 0.4, 0.4, 0.0],
                 [0.0, 0.4, 0.4, 0.4, 0.0],
                 [0.0, 0.0, 0.0, 0.0, 0.4]])
    # the 2 x 3 plateau: only its first cell (6) has no equal cell of lower index in reach; 19 touches 13 (equal, lower): no peak
    assert peaks_reference(prob, 5, 1, 3)[0].tolist() == [[6, -1, -1]]
    # radius 0: every positive cell, in cell order
    assert peaks_reference(prob, 5, 0, 8)[0].tolist() == [[6, 7, 8, 11, 12, 13, 19, -1]]
    # a whole map of one value: cell 0 with any window; with radius 1 also nothing else, every cell has a lower equal neighbour
    flat = np.full((1, 20), 0.05, dtype=np.float32)
    assert peaks_reference(flat, 5, 1, 2)[0].tolist() == [[0, -1]]
    assert peaks_reference(flat, 5, 0, 3)[0].tolist() == [[0, 1, 2]]


def test_all_zeros_and_more_than_the_peaks():
    zero = np.zeros((2, 20), dtype=np.float32)
    zero[1, 7] = 0.25
    for radius in (0, 1, 3):
        peaks, scores = peaks_reference(zero, 5, radius, 16)
        assert peaks[0].tolist() == [-1] * 16 and scores[0].tolist() == [0.0] * 16
        assert peaks[1].tolist() == [7] + [-1] * 15 and scores[1].tolist() == [0.25] + [0.0] * 15


def _define(text, name):
    m = re.search(r"^#define\s+%s\s+(\S+)" % name, text, re.M)
    assert m, f"include/eod_hip.h does not define {name}"
    return int(m.group(1), 0)


def test_mode_bits_in_header_and_ctypes_layer():
    text = open(os.path.join(ROOT, "include", "eod_hip.h")).read()
    assert _define(text, "EOD_SEMMAP_SCORES") == _lib.SEMMAP_SCORES == 0x10000
    assert _define(text, "EOD_SEMMAP_LOCATE") == _lib.SEMMAP_LOCATE
    assert _define(text, "EOD_SEMMAP_PEAKS") == _lib.SEMMAP_PEAKS
    assert _define(text, "EOD_SEMMAP_K_SHIFT") == _lib.SEMMAP_K_SHIFT
    assert _define(text, "EOD_SEMMAP_RADIUS_SHIFT") == _lib.SEMMAP_RADIUS_SHIFT
    assert _define(text, "EOD_SEMMAP_Q_SHIFT") == _lib.SEMMAP_Q_SHIFT
    # the fields and bits do not overlap one another or D = 512
    fields = [512, _lib.SEMMAP_SCORES, _lib.SEMMAP_LOCATE, _lib.SEMMAP_PEAKS, 0xF << _lib.SEMMAP_K_SHIFT, 0x3 << _lib.SEMMAP_RADIUS_SHIFT,
              0x3F << _lib.SEMMAP_Q_SHIFT]
    assert sum(fields) == np.bitwise_or.reduce(fields) and sum(fields) < 2 ** 31
    assert _lib.load().eod_abi_version() == 1


def _call(lib, D, C1=21, n_cells=100, ws=OK_PTR):
    return lib.eod_semmap_labels(OK_PTR, OK_PTR, OK_PTR, n_cells, D, C1, 0.4, OK_PTR, ws, None)


def test_undefined_bit_combinations_are_refused_on_the_host():
    lib = _lib.load()
    S, L, P = _lib.SEMMAP_SCORES, _lib.SEMMAP_LOCATE, _lib.SEMMAP_PEAKS
    q = lambda n: n << _lib.SEMMAP_Q_SHIFT                       # noqa: E731
    k = lambda n: (n - 1) << _lib.SEMMAP_K_SHIFT                 # noqa: E731
    r = lambda n: n << _lib.SEMMAP_RADIUS_SHIFT                  # noqa: E731
    bad = {"Q = 0": 512 | L, "Q = 33": 512 | L | q(33), "Q = 63": 512 | L | q(63), "both modes": 512 | L | P | q(4),
           "peaks with scores": 512 | P | S | q(4), "Q without a mode": 512 | S | q(4), "K without peaks": 512 | L | q(4) | k(8),
           "radius without peaks": 512 | L | q(4) | r(1), "K on the plain call": 512 | k(2), "radius on the SCORES call": 512 | S | r(1),
           "bit 17": 512 | L | q(4) | 0x20000, "bit 22": 512 | P | q(4) | 1 << 22, "bit 30": 512 | L | q(4) | 1 << 30,
           "D = 256": 256 | L | q(4), "peaks, D = 256": 256 | P | q(4), "peaks, Q = 0": 512 | P | k(8)}
    for name, D in bad.items():
        assert _call(lib, D) == BAD_DIMS, name
    assert _call(lib, 512 | P | q(4) | k(8) | r(1), C1=7) == BAD_DIMS            # 100 cells are no rows of 7
    assert _call(lib, 512 | P | q(4) | k(8) | r(1), C1=0) == BAD_DIMS
    assert _call(lib, 512 | L | q(4), C1=1) == BAD_DIMS
    assert _call(lib, 512 | L | q(4), n_cells=0) == BAD_DIMS
    assert _call(lib, 512 | L | q(4), ws=None) == NULL
    assert _call(lib, 512 | L | q(4), C1=4096) == -5                              # EOD_ERR_CAPACITY, as the SCORES call


def test_cell_center_inverts_robot_cell():
    from embodied_object_detection_amd.data.robot import RobotFrontEnd
    fe = RobotFrontEnd(projector=lambda *a: None)
    rng = np.random.default_rng(0)
    lo = np.asarray([fe.map_shift[0], fe.map_shift[2]], dtype=np.float64)
    for _ in range(200):
        p = lo + rng.uniform(0.0, 1.0, 2) * np.asarray([fe.map_w - 1, fe.map_h - 1]) * fe.res
        cell = fe.robot_cell((p[0], p[1], 0.0))
        x, y = fe.cell_center(cell)
        assert abs(x - p[0]) <= fe.res / 2 + 1e-4 and abs(y - p[1]) <= fe.res / 2 + 1e-4, (p, cell, (x, y))
        assert fe.cell_center(cell[0] * fe.map_h + cell[1]) == (x, y)              # the memory's index of the same cell
        assert fe.robot_cell((x, y, 0.0)) == cell
