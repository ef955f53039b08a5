"""The exact reference of `ops.map_clearance` and the maps of its tests (numpy only).

The reference is written from the definitions in include/eod_clearance.h, not from the kernels: for every cell the minimum of
(d2 << 32) | j over all blocked cells j by brute force in int64, in chunks, then the other outputs by their definitions.  Every
comparison against it is integer equality."""
import numpy as np

INT_MAX = 2 ** 31 - 1
INT_MIN = -2 ** 31
CELL_KEYS = ("d2", "nearest", "owner", "inflated")
SLOT_KEYS = ("cells", "territory", "widest_key", "widest_d2", "widest_cell")
KEYS = CELL_KEYS + SLOT_KEYS + ("open_key", "counts", "status")
_PAIRS = 1 << 21                                                     # (cell, blocked cell) pairs of one chunk
_REFS = {}


def slots(labels, objects):
    """int64 [N]: the lowest slot k with objects[k] == labels[i] and objects[k] >= 0; -1 where there is none."""
    labels = np.asarray(labels, dtype=np.int64)
    out = np.full(labels.shape, -1, np.int64)
    for k in range(len(objects) - 1, -1, -1):                        # the lowest slot is written last
        if objects[k] >= 0:
            out[labels == int(objects[k])] = k
    return out


def blocked_cells(labels, passable):
    """bool [N]: a label >= 0 that is not passable."""
    labels = np.asarray(labels, dtype=np.int64)
    b = labels >= 0
    for p in passable:
        b &= labels != int(p)
    return b


def key_of(d2, cell):
    """((u64)d2 << 32) | (u32)~cell."""
    return (np.asarray(d2).astype(np.uint64) << np.uint64(32)) | (np.uint64(0xFFFFFFFF) - np.asarray(cell).astype(np.uint64))


def reference(labels, objects, cols, radius2=0, keep_cell=-1, passable=()):
    """Every output of `ops.map_clearance` as numpy arrays: widest_key and open_key uint64, the others int32."""
    labels = np.ascontiguousarray(labels, dtype=np.int32)
    objects = np.ascontiguousarray(objects, dtype=np.int32)
    passable = np.ascontiguousarray(passable, dtype=np.int32).reshape(-1)
    key = (labels.tobytes(), objects.tobytes(), passable.tobytes(), int(cols), int(radius2), int(keep_cell))
    if key in _REFS:
        return _REFS[key]
    N, K = labels.size, objects.size
    rows = N // cols
    assert rows * cols == N and 1 <= K <= 64 and passable.size <= 64 and 0 <= radius2 < INT_MAX and -1 <= keep_cell < N
    assert rows <= 32767 and cols <= 32767
    B = blocked_cells(labels, passable)
    S = slots(labels, objects)
    cell = np.arange(N, dtype=np.int64)
    r, c = cell // cols, cell % cols
    bj = np.flatnonzero(B).astype(np.int64)
    if bj.size == 0:
        d2, nearest = np.full(N, INT_MAX, np.int64), np.full(N, -1, np.int64)
    else:
        br, bc = bj // cols, bj % cols
        best = np.empty(N, np.int64)
        step = max(1, _PAIRS // bj.size)
        for a in range(0, N, step):
            dr, dc = r[a:a + step, None] - br[None, :], c[a:a + step, None] - bc[None, :]
            best[a:a + step] = (((dr * dr + dc * dc) << 32) | bj[None, :]).min(axis=1)
        d2, nearest = best >> 32, best & 0xFFFFFFFF
        assert d2.max() < INT_MAX and (d2[B] == 0).all() and (nearest[B] == cell[B]).all()
    owner = np.where(nearest >= 0, labels[np.maximum(nearest, 0)].astype(np.int64), -1)
    free = ~B
    grow = free & (d2 <= radius2)
    if keep_cell >= 0:
        kr, kc = divmod(int(keep_cell), cols)
        grow &= ~((r - kr) ** 2 + (c - kc) ** 2 <= radius2)
    inflated = np.where(grow, owner, labels.astype(np.int64))
    near_slot = np.where(nearest >= 0, S[np.maximum(nearest, 0)], -1)
    keys = key_of(d2, cell)
    widest_key = np.zeros(K, np.uint64)
    territory = np.zeros(K, np.int64)
    for k in range(K):
        mine = free & (near_slot == k)
        territory[k] = mine.sum()
        if territory[k]:
            widest_key[k] = keys[mine].max()
    none = widest_key == 0
    widest_d2 = (widest_key >> np.uint64(32)).astype(np.int64)
    widest_cell = np.where(none, -1, 0xFFFFFFFF - (widest_key & np.uint64(0xFFFFFFFF)).astype(np.int64))
    open_key = np.array([keys[free].max() if free.any() else 0], np.uint64)
    out = dict(d2=d2.astype(np.int32), nearest=nearest.astype(np.int32), owner=owner.astype(np.int32), inflated=inflated.astype(np.int32),
               cells=np.bincount(S[S >= 0], minlength=K).astype(np.int32), territory=territory.astype(np.int32), widest_key=widest_key,
               widest_d2=widest_d2.astype(np.int32), widest_cell=widest_cell.astype(np.int32), open_key=open_key,
               counts=np.array([B.sum(), free.sum(), (free & (inflated != labels)).sum()], np.int32), status=np.zeros(2, np.int32))
    _REFS[key] = out
    return out


def host(res):
    """The dict of `ops.map_clearance` as the reference's arrays (the keys as uint64)."""
    out = {k: res[k].cpu().numpy() for k in KEYS}
    out["widest_key"] = out["widest_key"].view(np.uint64)
    out["open_key"] = out["open_key"].view(np.uint64)
    return out


def differences(got, ref, keys=KEYS):
    """The names of the outputs that differ in type, shape or any bit."""
    return [k for k in keys if got[k].dtype != ref[k].dtype or got[k].shape != ref[k].shape or not np.array_equal(got[k], ref[k])]


# ---- maps ---------------------------------------------------------------------------------------------------------------------
WALL = 1                                                             # a label no map asks for: it blocks and belongs to no slot


def maps(rows, cols, tile_rows, chunk_cols, halo_cols):
    """{name: dict(labels int32 [N], objects int32 [K], passable int32 [P], radius2, keep_cell)}: the maps of this op's own for one
    grid.  Maps that need room are left out on grids without it."""
    N, tr, cc, halo = rows * cols, tile_rows, chunk_cols, halo_cols
    rng = np.random.default_rng(rows * 1000 + cols)
    out = {}

    def grid(fill=-1):
        return np.full((rows, cols), fill, np.int32)

    def put(name, g, objects, radius2=0, keep_rc=None, passable=()):
        out[name] = dict(labels=g.reshape(-1).copy(), objects=np.asarray(objects, np.int32), passable=np.asarray(passable, np.int32),
                         radius2=int(radius2), keep_cell=-1 if keep_rc is None else int(keep_rc[0]) * cols + int(keep_rc[1]))

    put("no blocked cell", grid(), [10, -1], radius2=4)
    put("negative labels only", grid(-7), [10], radius2=1, keep_rc=(rows - 1, cols - 1))
    g = grid(10)
    g[rows // 2:, :] = 11
    put("every cell blocked", g, [11, 10, 12], radius2=25, keep_rc=(0, 0))
    # one blocked cell far away: from the opposite corner its own row and column are empty, and the scan runs across the grid
    for name, rc in (("corner 00", (0, 0)), ("corner 01", (0, cols - 1)), ("corner 10", (rows - 1, 0)), ("corner 11", (rows - 1, cols - 1))):
        g = grid()
        g[rc] = 10
        put(name, g, [10], radius2=2)
    g = grid()
    g[0, 0], g[0, cols - 1], g[rows - 1, 0], g[rows - 1, cols - 1] = 10, 11, 12, 13
    put("four corners", g, [13, 12, 11, 10], radius2=4)
    if rows >= 2:
        g = grid()
        g[rows // 2 - 1, cols - 1] = 10                              # (rows // 2, 0) follows it in memory and is cols - 1 columns away
        put("row-end pair", g, [10], radius2=1)
        g = grid()
        g[rows // 2, 0] = 10
        put("row-start pair", g, [10], radius2=1)
    # blocked cells before, on and after every border of a tile, a chunk and a halo, both ways
    rb = sorted({0, rows - 1} | set(range(tr, rows, tr)))
    cb = sorted({0, cols - 1} | set(range(cc, cols, cc)) | {b + halo for b in range(0, cols, cc) if b + halo < cols})
    thin = 3 if len(rb) * len(cb) > 12 else 1                         # sparse where there are many borders: distances stay long
    for off in (-1, 0, 1):
        g = grid()
        yo, xo = (off if rows > 1 else 0), (off if cols > 1 else 0)   # a single row or column has borders one way only
        for a, y in enumerate(rb):
            for b, x in enumerate(cb):
                if (a + b) % thin == 0 and 0 <= y + yo < rows and 0 <= x + xo < cols:
                    g[y + yo, x + xo] = 20 + (a + 2 * b) % 5
        put(f"borders {off:+d}", g, [20, 21, 22, 23, 24], radius2=2, keep_rc=(rows // 2, cols // 2))
    if cols >= 3:
        g = grid()
        g[rows // 2, 0], g[rows // 2, 2] = 3, 4
        if cols > cc + 1:
            g[rows // 2, cc - 1], g[rows // 2, cc + 1] = 4, 3        # the tied cell is the first of the second chunk
        put("left/right tie", g, [3, 4], radius2=1)
    if rows >= 3:
        g = grid()
        g[0, cols // 2], g[2, cols // 2] = 3, 4
        if rows > tr + 1:
            g[tr - 1, 0], g[tr + 1, 0] = 4, 3
        put("up/down tie", g, [4, 3], radius2=1)
    if rows >= 5 and cols >= 5:
        for name, x in (("diamond", cols // 2), ("diamond on the chunk border", cc)):
            if 2 <= x < cols - 2:
                g = grid()
                y = rows // 2
                g[y - 2, x], g[y, x - 2], g[y, x + 2], g[y + 2, x] = 5, 6, 7, 8
                put(name, g, [8, 7, 6, 5], radius2=4)
    # a diagonal candidate (3, 4) and a straight one (5, 0) at the same d2 = 25: the scan meets the diagonal one first, at dx = 4,
    # and the straight one, at dx = 5 with dx^2 == best, is the lower cell when the diagonal one lies in a row below
    # Where the grid has a second chunk of at least three columns (cols >= cc + 3) the viewing cell lies on one side of the first
    # chunk border and both candidates on the other, to the right (from column cc - 3: candidates at cc + 1, cc + 2) and to the
    # left (from cc + 1: candidates at cc - 3, cc - 4); on narrower grids the same figures stand inside the one chunk, and the
    # names say which.
    if rows >= 7 and cols >= 11:
        across = cols >= cc + 3
        where = "across the chunk border" if across else "inside the chunk"
        for name, x, sx in ((f"diagonal/straight tie to the right {where}", (cc if across else cols - 6) - 3, 1),
                            (f"diagonal/straight tie to the left {where}", (cc if across else cols - 6) + 1, -1),
                            ("diagonal/straight tie mid-chunk", 5, 1)):
            for below in (True, False):
                if 0 <= x + 5 * sx < cols and 0 <= x < cols:
                    g = grid()
                    y = 3
                    g[y + (3 if below else -3), x + 4 * sx] = 30
                    g[y, x + 5 * sx] = 31
                    put(f"{name}, diagonal {'below' if below else 'above'}", g, [30, 31], radius2=25, keep_rc=(y, x))
    if rows >= 3 and cols >= 3:
        g = grid()
        y, x = rows // 2, cols // 2
        g[max(0, y - 1):y + 2, max(0, x - 1):x + 2] = 12             # passable: free, with distances of its own, and no territory
        g[0, :cols - 1] = 13
        g[rows - 1, 1:] = 14
        put("a slot made passable", g, [13, 12, 14], radius2=2, keep_rc=(y, x), passable=[12, 99])
    g = rng.integers(0, 9, N).astype(np.int32).reshape(rows, cols)
    kind = rng.integers(0, 24, N).reshape(rows, cols)
    g[kind < 18] = -1
    for k, v in ((18, INT_MAX), (19, -7), (20, INT_MIN)):
        g[kind == k] = v
    put("labels and slots that name nothing", g, [3, -1, 1, 3, INT_MAX, -7, 1, 6, 0, 77, -1], radius2=2, keep_rc=(rows // 2, cols // 2),
        passable=[2, 5, 77, -7, INT_MAX, 5])
    g = grid()
    pick = rng.random(N).reshape(rows, cols) < 0.05
    g[pick] = (rng.integers(0, 64, N).reshape(rows, cols))[pick]
    put("64 objects", g, np.arange(64)[::-1], radius2=4, keep_rc=(rows - 1, cols // 2))
    put("one object of 64", g, [7], radius2=1)
    for m in out.values():
        assert m["labels"].dtype == np.int32 and m["labels"].shape == (N,) and 1 <= m["objects"].size <= 64 and -1 <= m["keep_cell"] < N
    return out


def wall_with_gap(rows, cols):
    """int32 [rows, cols]: a wall across the middle row with a gap one cell wide, the object 10 in the last row, and the cell of the
    gap.  A body of radius2 >= 1 does not fit through the gap."""
    g = np.full((rows, cols), -1, np.int32)
    g[rows // 2, :] = WALL
    gap = (rows // 2, cols // 3)
    g[gap] = -1
    g[rows - 1, cols - 1] = 10
    return g, gap[0] * cols + gap[1]
