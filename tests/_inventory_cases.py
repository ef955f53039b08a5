"""The exact reference of `ops.map_inventory` and the hostile maps of its tests (numpy only).

The reference is written from the definition in include/eod_inventory.h, not from the kernels: a plain union-find over the grid, one
cell after the other, uniting grid neighbours that carry the same class, then every statistic from the finished label map."""
import numpy as np

import _regions_cases as RC

SLOT_KEYS = ("object", "cls", "area", "bbox", "sum_rc", "peak", "peak_score", "mass_q24")
CLASS_KEYS = ("class_objects", "class_cells", "class_largest", "class_largest_area")
KEYS = ("object_labels", "count", "foreground") + SLOT_KEYS + CLASS_KEYS
LEVEL = RC.LEVEL
C5 = 5                                                               # the classes of the hostile maps
INT_MAX = 2 ** 31 - 1
_LABELS = {}


def foreground_class(labels, scores, C, level, keep=None):
    """int64 [N]: the class of each foreground cell, -1 for the background."""
    labels = np.asarray(labels, dtype=np.int64)
    ok = (labels >= 0) & (labels < C)
    if keep is not None:
        keep = np.asarray(keep)
        assert keep.shape == (C,)
        ok &= keep[np.where(ok, labels, 0)] != 0
    with np.errstate(invalid="ignore"):
        ok &= np.asarray(scores, dtype=np.float32) >= np.float32(level)         # a NaN compares false
    return np.where(ok, labels, -1)


def label_map(cls, cols, connectivity):
    """int32 [N]: the smallest cell index of each foreground cell's component, -1 for background (`cls`: -1)."""
    cls = np.asarray(cls, dtype=np.int64)
    key = (cls.tobytes(), int(cols), int(connectivity))
    if key in _LABELS:
        return _LABELS[key]
    N = cls.size
    parent = list(range(N))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    def union(a, b):
        a, b = find(a), find(b)
        if a != b:
            parent[max(a, b)] = min(a, b)                            # the root is the smallest cell

    k = cls.tolist()
    cells = np.flatnonzero(cls >= 0).tolist()
    for i in cells:
        r, c = divmod(i, cols)
        if c > 0 and k[i - 1] == k[i]:
            union(i, i - 1)
        if r > 0:
            if k[i - cols] == k[i]:
                union(i, i - cols)
            if connectivity == 8:
                if c > 0 and k[i - cols - 1] == k[i]:
                    union(i, i - cols - 1)
                if c < cols - 1 and k[i - cols + 1] == k[i]:
                    union(i, i - cols + 1)
    out = np.full(N, -1, dtype=np.int32)
    for i in cells:
        out[i] = find(i)
    _LABELS[key] = out
    return out


def reference(labels, scores, cols, C, level, connectivity=8, min_cells=1, topk=16, keep=None):
    """Every output of `ops.map_inventory` for `labels` int32 and `scores` float32 [B, N], as numpy arrays of the op's types."""
    labels = np.ascontiguousarray(labels, dtype=np.int32)
    scores = np.ascontiguousarray(scores, dtype=np.float32)
    assert connectivity in (4, 8) and labels.shape == scores.shape and labels.ndim == 2
    B, N = labels.shape
    K = int(topk)
    out = dict(object_labels=np.full((B, N), -1, np.int32), count=np.zeros(B, np.int32), foreground=np.zeros(B, np.int32),
               object=np.full((B, K), -1, np.int32), cls=np.full((B, K), -1, np.int32), area=np.zeros((B, K), np.int32),
               bbox=np.zeros((B, K, 4), np.int32), sum_rc=np.zeros((B, K, 2), np.int64), peak=np.zeros((B, K), np.int32),
               peak_score=np.zeros((B, K), np.float32), mass_q24=np.zeros((B, K), np.int64),
               class_objects=np.zeros((B, C), np.int32), class_cells=np.zeros((B, C), np.int32),
               class_largest=np.full((B, C), -1, np.int32), class_largest_area=np.zeros((B, C), np.int32))
    for b in range(B):
        cls = foreground_class(labels[b], scores[b], C, level, keep)
        lab = label_map(cls, cols, connectivity)
        out["object_labels"][b] = lab
        cells = np.flatnonzero(cls >= 0)
        out["foreground"][b] = len(cells)
        out["class_cells"][b] = np.bincount(cls[cells], minlength=C)
        roots, inv = np.unique(lab[cells], return_inverse=True)
        area = np.bincount(inv, minlength=len(roots))
        big = np.flatnonzero(area >= min_cells)
        out["count"][b] = len(big)
        order = big[np.lexsort((roots[big], -area[big]))]            # area descending, label ascending
        for j in order.tolist()[::-1]:                               # the first of the order is written last
            c = int(cls[roots[j]])
            out["class_objects"][b, c] += 1
            out["class_largest"][b, c] = roots[j]
            out["class_largest_area"][b, c] = area[j]
        for k, j in enumerate(order[:K].tolist()):
            mine = cells[inv == j]                                   # ascending
            assert (cls[mine] == cls[roots[j]]).all()
            r, c = mine // cols, mine % cols
            p = scores[b, mine]
            best = int(np.argmax(p))                                 # the first of the maxima: the lowest cell
            out["object"][b, k] = roots[j]
            out["cls"][b, k] = cls[roots[j]]
            out["area"][b, k] = area[j]
            out["bbox"][b, k] = (r.min(), c.min(), r.max(), c.max())
            out["sum_rc"][b, k] = (int(r.sum()), int(c.sum()))
            out["peak"][b, k] = mine[best]
            out["peak_score"][b, k] = p[best]
            q24 = np.minimum(p, np.float32(1.0)) * np.float32(16777216.0)         # float32: exact
            assert q24.dtype == np.float32
            out["mass_q24"][b, k] = int(q24.astype(np.int64).sum())               # truncated
    return out


# ---- maps ---------------------------------------------------------------------------------------------------------------------
def random_classes(N, C, seed):
    return np.random.default_rng(seed).integers(0, C, N).astype(np.int32)


def alternating(rows, cols, a, b, dr=3, dc=5):
    """int32 [N]: blocks of dr x dc cells that carry the classes a and b in turn."""
    r, c = np.mgrid[0:rows, 0:cols]
    return np.where((r // dr + c // dc) % 2 == 0, a, b).astype(np.int32).reshape(-1)


def hostile_maps(rows, cols, tile_rows, tile_cols, level=LEVEL):
    """{name: (labels int32 [N], scores float32 [N], keep uint8 [C5] or None)}: the maps of tests/test_inventory_gpu.py for one grid,
    all in C5 classes.  Where nothing else is said every cell carries a valid label, the background too: the scores alone decide.
    The pairs at a four-tile corner exist where the grid has one (more than one tile in both directions)."""
    N = rows * cols
    lv = np.float32(level)
    r, c = np.mgrid[0:rows, 0:cols]
    r, c = r.reshape(-1), c.reshape(-1)
    ones = RC.paint(np.ones(N, bool), level, seed=40)
    maps = {}
    for i, p in enumerate((0.3, 0.593, 0.8)):                                     # five classes drawn per cell
        maps[f"bernoulli {p}"] = (random_classes(N, C5, 200 + i), RC.paint(RC.bernoulli(rows, cols, p, seed=100 + i), level, seed=i), None)
    maps["two classes"] = (random_classes(N, 2, 210) * 3 + 1, RC.paint(RC.bernoulli(rows, cols, 0.9, seed=110), level, seed=9), None)
    maps["checkerboard"] = (np.where((r + c) % 2 == 0, 1, 3).astype(np.int32), ones, None)
    maps["column stripes"] = ((c // tile_cols % 2).astype(np.int32), ones, None)               # touch along whole tile borders
    maps["row stripes"] = ((r // tile_rows % 2 * 2).astype(np.int32), ones, None)
    maps["tile blocks"] = (((r // tile_rows + c // tile_cols) % 3).astype(np.int32), ones, None)     # anti-diagonal tiles are equal
    rm = rows // 2
    maps["row-end pair"] = (np.full(N, 2, np.int32), RC.paint(RC.cells(rows, cols, [(rm, cols - 1), (rm + 1, 0)]), level, seed=13), None)
    if rows > tile_rows and cols > tile_cols:
        tr, tc = tile_rows, tile_cols
        lab = np.full((rows, cols), 0, np.int32)
        lab[tr - 1, tc - 1] = lab[tr, tc] = 2
        lab[tr - 1, tc] = lab[tr, tc - 1] = 4
        four = [(tr - 1, tc - 1), (tr, tc), (tr - 1, tc), (tr, tc - 1)]
        maps["corner, both diagonals"] = (lab.reshape(-1), RC.paint(RC.cells(rows, cols, four), level, seed=15), None)
        lab = lab.copy()
        lab[lab == 0] = 2                                                         # the diagonal's class all around, below the level
        maps["corner, class all around"] = (lab.reshape(-1), RC.paint(RC.cells(rows, cols, four), level, seed=16), None)
    maps["serpentine"] = (alternating(rows, cols, 1, 2), RC.paint(RC.serpentine(rows, cols), level, seed=10), None)
    maps["spirals"] = (alternating(rows, cols, 0, 4, dr=4, dc=7), RC.paint(RC.spirals(rows, cols), level, seed=11), None)
    maps["one class everywhere"] = (np.full(N, 3, np.int32), ones, None)
    maps["all background"] = (random_classes(N, C5, 220), RC.paint(np.zeros(N, bool), level, seed=18), None)
    # scores equal to the level are foreground, the float below it is not
    at = RC.bernoulli(rows, cols, 0.55, seed=19)
    maps["at the level"] = (random_classes(N, 3, 221), np.where(at, lv, np.float32(0.0)).astype(np.float32), None)
    maps["below the level"] = (random_classes(N, 3, 221), np.where(at, np.nextafter(lv, np.float32(0.0)), np.float32(0.0)).astype(np.float32), None)
    nan = RC.paint(RC.bernoulli(rows, cols, 0.8, seed=20), level, seed=20)
    nan[np.random.default_rng(21).random(N) < 0.1] = np.nan
    maps["nan"] = (random_classes(N, 2, 222), nan, None)
    # labels that are no class: background whatever the score
    lab = random_classes(N, 2, 223)
    kind = np.random.default_rng(24).integers(0, 10, N)
    for k, v in ((0, -1), (1, C5), (2, -7), (3, INT_MAX)):
        lab[kind == k] = v
    maps["labels that are no class"] = (lab, ones, None)
    # class 1 joins two areas of class 0 on the left and on the right; the keep table removes class 1, not the gap
    lab = np.where(c == cols // 2, 1, 0).astype(np.int32)
    maps["keep cuts"] = (lab, ones, np.array([1, 0, 1, 1, 1], np.uint8))
    maps["keep on random classes"] = (random_classes(N, C5, 224), RC.paint(RC.bernoulli(rows, cols, 0.7, seed=25), level, seed=25),
                                      np.array([0, 1, 1, 0, 1], np.uint8))
    # equal areas in different classes, the classes not in the order of the labels: 2 x 2 blocks, one free cell between them
    lab = np.full((rows, cols), -1, np.int32)
    order = (3, 1, 4, 1, 0, 3, 2)
    n = 0
    for r0 in range(0, rows - 1, 3):
        for c0 in range(0, cols - 1, 3):
            lab[r0:r0 + 2, c0:c0 + 2] = order[n % len(order)]
            n += 1
    maps["equal areas"] = (lab.reshape(-1), ones, None)
    # the peak on a plateau of one class that another class cuts in two
    sc = np.full((rows, cols), 0.625, np.float32)
    sc[1:4, :] = 0.875
    lab = np.full((rows, cols), 1, np.int32)
    lab[:, cols // 3] = 0
    maps["plateau"] = (lab.reshape(-1), sc.reshape(-1), None)
    for lab, sc, keep in maps.values():
        assert lab.dtype == np.int32 and lab.shape == (N,) and sc.dtype == np.float32 and sc.shape == (N,)
        assert keep is None or (keep.dtype == np.uint8 and keep.shape == (C5,))
    return maps


def restricted(ref, c):
    """Of a one-map reference (every array without its leading [B]) the objects of class c in their order, as `RC.reference` names
    them: region, area, bbox, sum_rc, peak, peak_prob, mass_q24 of the slots whose cls is c."""
    at = np.flatnonzero(ref["cls"] == c)
    names = dict(object="region", area="area", bbox="bbox", sum_rc="sum_rc", peak="peak", peak_score="peak_prob", mass_q24="mass_q24")
    return {v: ref[k][at] for k, v in names.items()}
