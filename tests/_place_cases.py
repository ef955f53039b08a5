"""The exact reference of `eod_place_masks` in numpy (a boolean index, `np.unique(..., return_counts=True)`, a lexsort) and the
inputs of its edge-case tests.  No GPU here; `test_place_cpu.py` holds the reference to a brute-force count."""
import numpy as np

KEYS = ("mask_pixels", "pixels", "invalid", "distinct", "cells", "cell_pixels")
INT32_MIN, INT32_MAX = -2 ** 31, 2 ** 31 - 1


def clip_rect(rect, H, W):
    if rect is None:
        return 0, 0, W, H
    x0, y0, x1, y1 = (int(v) for v in rect)
    return max(x0, 0), max(y0, 0), min(x1, W), min(y1, H)


def reference(masks, proj, n_cells, count=None, rects=None, topk=4, exclude_cell=-1):
    """masks [K_cap, H, W] (any integer or bool dtype, nonzero = set), proj [H, W] -> the dict of int32 arrays the op returns."""
    masks, proj = np.asarray(masks), np.asarray(proj).astype(np.int64)
    K_cap, H, W = masks.shape
    n = K_cap if count is None else max(0, min(int(count), K_cap))
    out = {k: np.zeros((K_cap,), dtype=np.int32) for k in KEYS[:4]}
    out["cells"] = np.full((K_cap, topk), -1, dtype=np.int32)
    out["cell_pixels"] = np.zeros((K_cap, topk), dtype=np.int32)
    for k in range(n):
        x0, y0, x1, y1 = clip_rect(None if rects is None else rects[k], H, W)
        if x1 <= x0 or y1 <= y0:
            continue
        cells = proj[y0:y1, x0:x1][masks[k, y0:y1, x0:x1] != 0]
        out["mask_pixels"][k] = cells.size
        bad = (cells < 0) | (cells >= n_cells)
        out["invalid"][k] = int(bad.sum())
        cells = cells[~bad]
        cells = cells[cells != exclude_cell]
        out["pixels"][k] = cells.size
        u, c = np.unique(cells, return_counts=True)
        out["distinct"][k] = u.size
        order = np.lexsort((u, -c))[:topk]                  # count descending, then cell ascending
        out["cells"][k, :order.size] = u[order]
        out["cell_pixels"][k, :order.size] = c[order]
    return out


def brute_force(masks, proj, n_cells, count=None, rects=None, topk=4, exclude_cell=-1):
    """The same by one Python loop over the pixels and a Counter."""
    from collections import Counter
    masks, proj = np.asarray(masks), np.asarray(proj)
    K_cap, H, W = masks.shape
    n = K_cap if count is None else max(0, min(int(count), K_cap))
    out = {k: np.zeros((K_cap,), dtype=np.int32) for k in KEYS[:4]}
    out["cells"] = np.full((K_cap, topk), -1, dtype=np.int32)
    out["cell_pixels"] = np.zeros((K_cap, topk), dtype=np.int32)
    for k in range(n):
        x0, y0, x1, y1 = clip_rect(None if rects is None else rects[k], H, W)
        h = Counter()
        for y in range(y0, y1):
            for x in range(x0, x1):
                if not masks[k, y, x]:
                    continue
                out["mask_pixels"][k] += 1
                c = int(proj[y, x])
                if c < 0 or c >= n_cells:
                    out["invalid"][k] += 1
                elif c != exclude_cell:
                    h[c] += 1
        out["pixels"][k] = sum(h.values())
        out["distinct"][k] = len(h)
        for t, (c, v) in enumerate(sorted(h.items(), key=lambda cv: (-cv[1], cv[0]))[:topk]):
            out["cells"][k, t], out["cell_pixels"][k, t] = c, v
    return out


# ---- the edge cases: H, W odd (every row of a mask starts at another alignment), 19 x 23 cells, 12 rows of which 10 count ----
H, W = 45, 37
ROWS, COLS = 19, 23
N_CELLS = ROWS * COLS
K_CAP, COUNT = 12, 10
ROW_NAMES = ["empty mask", "pixels (0, 0) and (H-1, W-1)", "full image", "mask larger than its rect", "rect partly outside the image",
             "empty rect", "six cells with two pixels each", "all pixels in one cell", "every pixel in the excluded cell",
             "invalid cells under the mask, bytes 255 and 2", "garbage", "garbage"]


def edge_cases(seed=0):
    """dict(masks uint8 [12, H, W], proj int32 [H, W], rects int32 [12, 4], exclude_cell, one_cell, tie_cells)."""
    rng = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    proj = ((yy * ROWS) // H * COLS + (xx * COLS) // W).astype(np.int32)          # blocks of 2-3 x 1-2 pixels, every cell hit
    for (y, x), v in zip(((3, 5), (3, 6), (4, 5), (4, 6)), (-1, N_CELLS, INT32_MIN, INT32_MAX)):
        proj[y, x] = v
    full = (0, 0, W, H)
    masks = np.zeros((K_CAP, H, W), dtype=np.uint8)
    rects = np.zeros((K_CAP, 4), dtype=np.int32)
    rects[:] = full
    masks[1, 0, 0] = masks[1, H - 1, W - 1] = 1
    masks[2] = 1
    masks[3, 5:40, 3:30] = 1
    rects[3] = (10, 12, 25, 31)
    masks[4] = np.where(rng.rand(H, W) < 0.5, rng.choice([255, 2], size=(H, W)), 0)
    rects[4] = (-5, -7, 20, 15)
    masks[5] = 1
    rects[5] = (20, 10, 20, 30)
    # ties: the first two pixels of six cells, picked from the high indices down so that no scan order gives the answer by accident
    valid = proj[(proj >= 0) & (proj < N_CELLS)]
    u, c = np.unique(valid, return_counts=True)
    tie_cells = [int(v) for v in u[c >= 2][::-1][3:60:10]][:6]
    assert len(tie_cells) == 6
    for cell in tie_cells:
        ys, xs = np.nonzero(proj == cell)
        masks[6, ys[:2], xs[:2]] = 1
    one_cell = int(proj[30, 20])
    masks[7] = proj == one_cell
    exclude_cell = int(proj[22, 18])
    masks[8] = proj == exclude_cell
    masks[9, 2:8, 3:10] = np.where((yy[2:8, 3:10] + xx[2:8, 3:10]) % 2 == 0, 255, 2)
    rects[9] = (0, 0, W + 9, H + 9)
    masks[10:] = rng.randint(0, 256, size=(2, H, W))
    rects[10] = (3, 4, 30, 40)
    rects[11] = (-100, -100, 1000, 1000)
    assert exclude_cell not in tie_cells and exclude_cell != one_cell and one_cell not in tie_cells
    return dict(masks=masks, proj=proj, rects=rects, exclude_cell=exclude_cell, one_cell=one_cell, tie_cells=sorted(tie_cells))
