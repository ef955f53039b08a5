"""The exact reference of `ops.map_regions` and the hostile maps of its tests (numpy only).

The reference is written from the definition in include/eod_regions.h, not from the kernels: a plain union-find over the grid, one
cell after the other, then every statistic from the finished label map."""
import numpy as np

KEYS = ("region_labels", "count", "foreground", "region", "area", "bbox", "sum_rc", "peak", "peak_prob", "mass_q24")
LEVEL = 0.5
_LABELS = {}


def label_map(fg, cols, connectivity):
    """int32 [N]: the smallest cell index of each foreground cell's component, -1 for background."""
    fg = np.asarray(fg, dtype=bool)
    key = (fg.tobytes(), int(cols), int(connectivity))
    if key in _LABELS:
        return _LABELS[key]
    N = fg.size
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

    f = fg.tolist()
    cells = np.flatnonzero(fg).tolist()
    for i in cells:
        r, c = divmod(i, cols)
        if c > 0 and f[i - 1]:
            union(i, i - 1)
        if r > 0:
            if f[i - cols]:
                union(i, i - cols)
            if connectivity == 8:
                if c > 0 and f[i - cols - 1]:
                    union(i, i - cols - 1)
                if c < cols - 1 and f[i - cols + 1]:
                    union(i, i - cols + 1)
    labels = np.full(N, -1, dtype=np.int32)
    for i in cells:
        labels[i] = find(i)
    _LABELS[key] = labels
    return labels


def reference(prob, cols, level, connectivity=8, min_cells=1, topk=16):
    """Every output of `ops.map_regions` for `prob` float32 [Q, N], as numpy arrays of the op's types."""
    prob = np.ascontiguousarray(prob, dtype=np.float32)
    assert connectivity in (4, 8)
    Q, N = prob.shape
    K = int(topk)
    out = dict(region_labels=np.full((Q, N), -1, np.int32), count=np.zeros(Q, np.int32), foreground=np.zeros(Q, np.int32),
               region=np.full((Q, K), -1, np.int32), area=np.zeros((Q, K), np.int32), bbox=np.zeros((Q, K, 4), np.int32),
               sum_rc=np.zeros((Q, K, 2), np.int64), peak=np.zeros((Q, K), np.int32), peak_prob=np.zeros((Q, K), np.float32),
               mass_q24=np.zeros((Q, K), np.int64))
    for q in range(Q):
        with np.errstate(invalid="ignore"):
            fg = prob[q] >= np.float32(level)                        # a NaN compares false
        labels = label_map(fg, cols, connectivity)
        out["region_labels"][q] = labels
        out["foreground"][q] = int(fg.sum())
        cells = np.flatnonzero(fg)
        roots, inv = np.unique(labels[cells], return_inverse=True)
        area = np.bincount(inv, minlength=len(roots))
        keep = np.flatnonzero(area >= min_cells)
        out["count"][q] = len(keep)
        order = keep[np.lexsort((roots[keep], -area[keep]))][:K]      # area descending, label ascending
        for k, j in enumerate(order.tolist()):
            mine = cells[inv == j]                                   # ascending
            r, c = mine // cols, mine % cols
            p = prob[q, mine]
            best = int(np.argmax(p))                                 # the first of the maxima: the lowest cell
            out["region"][q, k] = roots[j]
            out["area"][q, k] = area[j]
            out["bbox"][q, k] = (r.min(), c.min(), r.max(), c.max())
            out["sum_rc"][q, k] = (int(r.sum()), int(c.sum()))
            out["peak"][q, k] = mine[best]
            out["peak_prob"][q, k] = p[best]
            q24 = np.minimum(p, np.float32(1.0)) * np.float32(16777216.0)         # float32: exact
            assert q24.dtype == np.float32
            out["mass_q24"][q, k] = int(q24.astype(np.int64).sum())               # truncated
    return out


# ---- maps ---------------------------------------------------------------------------------------------------------------------
def paint(fg, level=LEVEL, seed=0):
    """float32 [N]: values in [level, 1] on `fg`, in [0, level) elsewhere."""
    fg = np.asarray(fg, dtype=bool).reshape(-1)
    rng = np.random.default_rng(seed)
    lv = np.float32(level)
    hi = (lv + (np.float32(1.0) - lv) * rng.random(fg.size, dtype=np.float32)).astype(np.float32)
    lo = (np.nextafter(lv, np.float32(0.0)) * rng.random(fg.size, dtype=np.float32)).astype(np.float32)
    out = np.where(fg, np.clip(hi, lv, np.float32(1.0)), lo).astype(np.float32)
    assert np.array_equal(out >= lv, fg)
    return out


def bernoulli(rows, cols, p, seed):
    return np.random.default_rng(seed).random(rows * cols) < p


def serpentine(rows, cols):
    """Full even rows, joined alternately at the right and at the left end: one component under either connectivity, root 0."""
    fg = np.zeros((rows, cols), bool)
    fg[0::2] = True
    for r in range(1, rows - 1, 2):
        fg[r, cols - 1 if (r // 2) % 2 == 0 else 0] = True
    return fg.reshape(-1)


def spirals(rows, cols):
    """Two interleaved rectangular spirals, one cell thick and one cell apart: two walkers, from the first cell heading right and
    from the last cell heading left, step in turn, go straight while the three cells ahead of the next cell are free, turn
    clockwise otherwise and stop when they cannot move."""
    occ = np.zeros((rows, cols), bool)
    free = lambda r, c: not (0 <= r < rows and 0 <= c < cols) or not occ[r, c]
    walkers = [[0, 0, 0, 1], [rows - 1, cols - 1, 0, -1]]
    for w in walkers:
        occ[w[0], w[1]] = True
    active = [True, True]
    while any(active):
        for i, w in enumerate(walkers):
            if not active[i]:
                continue
            for _ in range(2):
                r, c, dr, dc = w
                nr, nc = r + dr, c + dc
                if (0 <= nr < rows and 0 <= nc < cols and not occ[nr, nc]
                        and all(free(nr + dr + k * dc, nc + dc + k * dr) for k in (-1, 0, 1))):
                    occ[nr, nc] = True
                    w[0], w[1] = nr, nc
                    break
                w[2], w[3] = dc, -dr
            else:
                active[i] = False
    return occ.reshape(-1)


def checkerboard(rows, cols):
    r, c = np.mgrid[0:rows, 0:cols]
    return ((r + c) % 2 == 0).reshape(-1)


def cells(rows, cols, rc):
    fg = np.zeros((rows, cols), bool)
    for r, c in rc:
        fg[r, c] = True
    return fg.reshape(-1)


def hostile_maps(rows, cols, tile_rows, tile_cols, level=LEVEL):
    """{name: float32 [N]}: the maps of tests/test_regions_gpu.py for one grid.  The pairs at a four-tile corner exist where the grid
    has one (more than one tile in both directions)."""
    N = rows * cols
    lv = np.float32(level)
    maps = {}
    for i, p in enumerate((0.3, 0.5, 0.593, 0.7)):
        maps[f"bernoulli {p}"] = paint(bernoulli(rows, cols, p, seed=100 + i), level, seed=i)
    maps["serpentine"] = paint(serpentine(rows, cols), level, seed=10)
    maps["spirals"] = paint(spirals(rows, cols), level, seed=11)
    maps["checkerboard"] = paint(checkerboard(rows, cols), level, seed=12)
    rm = rows // 2
    maps["row-end pair"] = paint(cells(rows, cols, [(rm, cols - 1), (rm + 1, 0)]), level, seed=13)
    maps["row ends"] = paint(cells(rows, cols, [(rm, 0), (rm, cols - 1)]), level, seed=14)
    if rows > tile_rows and cols > tile_cols:
        maps["corner diagonal"] = paint(cells(rows, cols, [(tile_rows - 1, tile_cols - 1), (tile_rows, tile_cols)]), level, seed=15)
        maps["corner anti-diagonal"] = paint(cells(rows, cols, [(tile_rows - 1, tile_cols), (tile_rows, tile_cols - 1)]), level, seed=16)
    maps["all foreground"] = paint(np.ones(N, bool), level, seed=17)
    maps["all background"] = paint(np.zeros(N, bool), level, seed=18)
    # values equal to the level are foreground, the float below it is not
    at = bernoulli(rows, cols, 0.55, seed=19)
    maps["at the level"] = np.where(at, lv, np.float32(0.0)).astype(np.float32)
    maps["below the level"] = np.where(at, np.nextafter(lv, np.float32(0.0)), np.float32(0.0)).astype(np.float32)
    # NaN: background, also where it cuts a component
    nan = paint(bernoulli(rows, cols, 0.65, seed=20), level, seed=20)
    nan[np.random.default_rng(21).random(N) < 0.1] = np.nan
    maps["nan"] = nan
    # a plateau of the maximum: the peak is its lowest cell (two blobs, the plateau not at a blob's first cell)
    pl = np.zeros((rows, cols), np.float32)
    pl[1:min(rows, 9), 0:min(cols, 7)] = 0.625
    pl[2:min(rows, 5), 2:min(cols, 6)] = 0.875
    pl[rows - 2:, cols - 3:] = 0.75
    maps["plateau"] = pl.reshape(-1)
    # mass_q24: 1.0, multiples of 2^-24, values above 1 (clamped) and generic floats
    rng = np.random.default_rng(22)
    ms = paint(bernoulli(rows, cols, 0.6, seed=23), level, seed=23)
    fg = np.flatnonzero(ms >= lv)
    kind = rng.integers(0, 4, fg.size)
    ms[fg[kind == 0]] = 1.0
    ms[fg[kind == 1]] = (rng.integers(2 ** 23, 2 ** 24, int((kind == 1).sum())).astype(np.float64) * 2.0 ** -24).astype(np.float32)
    ms[fg[kind == 2]] = np.float32(1.0) + rng.random(int((kind == 2).sum()), dtype=np.float32)
    maps["mass"] = ms
    for v in maps.values():
        assert v.dtype == np.float32 and v.shape == (N,)
    return maps


def centroid(sum_rc, area):
    return np.asarray(sum_rc, np.float64) / np.asarray(area, np.float64)[..., None]
