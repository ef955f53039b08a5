"""The exact reference of `ops.map_relations` and the maps of its tests (numpy only).

The reference is written from the definition in include/eod_relations.h, not from the kernel: every offset of the disc, in no
particular order, is laid over the whole grid; every cell pair (i in a, j in b) it finds goes into the minimum of the keys, into the
set of (cell, slot) pairs that counts near_cells and, at d2 == 1, into edges."""
import numpy as np

INT_MAX = 2 ** 31 - 1
NONE = np.uint64(2 ** 64 - 1)
MATRIX_KEYS = ("pair_key", "min_d2", "closest", "near_cells", "edges")
SLOT_KEYS = ("cells", "nearest", "nearest_d2", "from_key", "from_d2", "from_closest")
KEYS = MATRIX_KEYS + SLOT_KEYS
_REFS = {}


def slots(labels, objects):
    """int64 [N]: the lowest slot k with objects[k] == labels[i] and objects[k] >= 0; -1 where there is none."""
    labels = np.asarray(labels, dtype=np.int64)
    out = np.full(labels.shape, -1, np.int64)
    for k in range(len(objects) - 1, -1, -1):                        # the lowest slot is written last
        if objects[k] >= 0:
            out[labels == int(objects[k])] = k
    return out


def disc(R):
    """The offsets (dr, dc) with 0 < dr^2 + dc^2 <= R^2."""
    return [(dr, dc) for dr in range(-R, R + 1) for dc in range(-R, R + 1) if 0 < dr * dr + dc * dc <= R * R]


def reference(labels, objects, cols, radius, from_cell=-1, topn=4):
    """Every output of `ops.map_relations` as numpy arrays: pair_key and from_key uint64, the others int32."""
    labels = np.ascontiguousarray(labels, dtype=np.int32)
    objects = np.ascontiguousarray(objects, dtype=np.int32)
    key = (labels.tobytes(), objects.tobytes(), int(cols), int(radius), int(from_cell), int(topn))
    if key in _REFS:
        return _REFS[key]
    N, K = labels.size, objects.size
    rows = N // cols
    assert rows * cols == N and 1 <= K <= 64 and 1 <= radius <= 16 and -1 <= from_cell < N and 1 <= topn <= 8
    S = slots(labels, objects).reshape(rows, cols)
    cell = np.arange(N, dtype=np.int64).reshape(rows, cols)
    pair_key = np.full((K, K), NONE, np.uint64)
    edges = np.zeros((K, K), np.int64)
    near = np.zeros((N, K), bool)                                    # near[i, b]: cell i has a cell of slot b within reach
    for dr, dc in disc(radius):
        if abs(dr) >= rows or abs(dc) >= cols:
            continue
        # cell i = (r, c) and cell j = (r + dr, c + dc), both on the grid: a row's end and the next row's start never meet
        ri = slice(max(0, -dr), rows - max(0, dr))
        ci = slice(max(0, -dc), cols - max(0, dc))
        rj = slice(max(0, dr), rows - max(0, -dr))
        cj = slice(max(0, dc), cols - max(0, -dc))
        a, b, i = S[ri, ci], S[rj, cj], cell[ri, ci]
        m = (a >= 0) & (b >= 0) & (a != b)
        a, b, i = a[m], b[m], i[m]
        d2 = dr * dr + dc * dc
        np.minimum.at(pair_key, (a, b), (np.uint64(d2) << np.uint64(32)) | i.astype(np.uint64))
        near[i, b] = True
        if d2 == 1:
            np.add.at(edges, (a, b), 1)
    flat = S.reshape(-1)
    has = flat >= 0
    cells = np.bincount(flat[has], minlength=K).astype(np.int32)
    near_cells = np.zeros((K, K), np.int64)
    for k in range(K):
        near_cells[k] = near[flat == k].sum(axis=0)
    none = pair_key == NONE
    min_d2 = np.where(none, INT_MAX, (pair_key >> np.uint64(32)).astype(np.int64)).astype(np.int32)
    closest = np.where(none, -1, (pair_key & np.uint64(0xFFFFFFFF)).astype(np.int64)).astype(np.int32)
    nearest = np.full((K, topn), -1, np.int32)
    nearest_d2 = np.full((K, topn), INT_MAX, np.int32)
    for a in range(K):
        order = sorted((int(min_d2[a, b]), b) for b in range(K) if min_d2[a, b] < INT_MAX)[:topn]
        for n, (d, b) in enumerate(order):
            nearest[a, n], nearest_d2[a, n] = b, d
    from_key = np.full(K, NONE, np.uint64)
    if from_cell >= 0:
        fr, fc = divmod(int(from_cell), cols)
        r, c = np.divmod(np.arange(N, dtype=np.int64), cols)
        k64 = (((r - fr) ** 2 + (c - fc) ** 2).astype(np.uint64) << np.uint64(32)) | np.arange(N, dtype=np.uint64)
        np.minimum.at(from_key, flat[has], k64[has])
    fnone = from_key == NONE
    out = dict(pair_key=pair_key, min_d2=min_d2, closest=closest, near_cells=near_cells.astype(np.int32), edges=edges.astype(np.int32),
               cells=cells, nearest=nearest, nearest_d2=nearest_d2, from_key=from_key,
               from_d2=np.where(fnone, INT_MAX, (from_key >> np.uint64(32)).astype(np.int64)).astype(np.int32),
               from_closest=np.where(fnone, -1, (from_key & np.uint64(0xFFFFFFFF)).astype(np.int64)).astype(np.int32))
    _REFS[key] = out
    return out


def host(res):
    """The dict of `ops.map_relations` as the reference's arrays (the two key tables as uint64)."""
    out = {k: res[k].cpu().numpy() for k in KEYS}
    out["pair_key"], out["from_key"] = out["pair_key"].view(np.uint64), out["from_key"].view(np.uint64)
    return out


def differences(got, ref):
    """The names of the outputs that differ in type, shape or any bit."""
    return [k for k in KEYS if got[k].dtype != ref[k].dtype or got[k].shape != ref[k].shape or not np.array_equal(got[k], ref[k])]


# ---- maps ---------------------------------------------------------------------------------------------------------------------
def first_beyond(R):
    """The smallest d2 above R^2 that two cells can have, as (dr, dc)."""
    best = min((dr * dr + dc * dc, dr, dc) for dr in range(0, R + 2) for dc in range(0, R + 2) if dr * dr + dc * dc > R * R)
    return best[1], best[2]


def exactly_at(R):
    """Offsets with d2 == R^2: the axis one and, where R is a hypotenuse (5, 10, 13, 15), a slanted one."""
    out = [(0, R)]
    out += [(dr, dc) for dr in range(1, R) for dc in range(dr, R) if dr * dr + dc * dc == R * R][:1]
    return out


def own_maps(rows, cols, tile_rows, tile_cols, R):
    """{name: (labels int32 [N], objects int32 [K])}: the maps of this op's own for one grid and radius.  Maps that need room are
    left out on grids without it."""
    N = rows * cols
    maps = {}

    def grid():
        return np.full((rows, cols), -1, np.int32)

    def put(name, g, objects):
        maps[name] = (g.reshape(-1).copy(), np.asarray(objects, np.int32))

    # single cells at exactly d2 = R^2 and at the first d2 beyond it, in pairs of their own labels
    g, objs, lab = grid(), [], 10
    bdr, bdc = first_beyond(R)
    offs = exactly_at(R) + [(bdr, bdc)]
    offs += [(dc, dr) for dr, dc in offs]                            # along the columns too
    r0 = 0
    for dr, dc in offs:
        ends = [(r0, 0, r0 + dr, dc)]
        if cols >= 2 * dc + R + 3:                                   # a mirrored pair at the row's end, out of the first one's reach
            ends.append((r0, cols - 1, r0 + dr, cols - 1 - dc))
        for ar, ac, br, bc in ends:
            if br < rows and 0 <= bc < cols and g[ar, ac] < 0 and g[br, bc] < 0:
                g[ar, ac], g[br, bc] = lab, lab + 1
                objs += [lab, lab + 1]
                lab += 2
        r0 += max(dr, 0) + R + 2                                     # the next pair is out of every earlier cell's reach downwards
        if r0 >= rows:
            break
    if objs:
        put("at and beyond the radius", g, objs[:64])
    # pairs astride the tile borders and across the four-tile corner: within the halo (R apart) and one cell outside it
    if rows > tile_rows and cols > tile_cols + R + 2:
        tr, tc = tile_rows, tile_cols
        g, objs, lab = grid(), [], 100
        pairs = []
        for gap in (R, R + 1):
            pairs.append(((3 + 2 * (gap - R), tc - 1), (3 + 2 * (gap - R), tc - 1 + gap)))          # across a column border, along a row
            pairs.append(((tr - 1, 20 + 2 * (gap - R)), (tr - 1 + gap, 20 + 2 * (gap - R))))        # across a row border, along a column
        pairs.append(((tr - 1, tc - 1), (tr, tc)))                                                  # the corner's diagonals
        pairs.append(((tr - 1, tc + R + 1), (tr, tc + R)))
        for (ar, ac), (br, bc) in pairs:
            if br < rows and bc < cols and g[ar, ac] < 0 and g[br, bc] < 0:
                g[ar, ac], g[br, bc] = lab, lab + 1
                objs += [lab, lab + 1]
                lab += 2
        put("astride the tile borders", g, objs)
        # two touching blocks with a long shared border across a tile border
        g = grid()
        g[2:tr + 4, 5:tc + 20] = 7
        g[tr - 3:tr + 1, 0:5] = 8                                    # to the left: a border along a column, across the row border
        g[tr + 4:tr + 6, 3:tc + 25] = 9                              # below: a border along a row, across the column border
        put("long shared borders", g, [9, 7, 8, 3])
    # 64 objects alternating cell by cell
    g = (np.arange(N, dtype=np.int64) * 37 % 64).astype(np.int32).reshape(rows, cols)
    put("64 alternating", g, np.arange(64)[::-1])
    # one object everywhere with single cells of others inside it
    g = np.full((rows, cols), 5, np.int32)
    rng = np.random.default_rng(rows * 1000 + cols)
    inside = rng.choice(N, size=min(N, 12), replace=False)
    g.reshape(-1)[inside] = 20 + np.arange(len(inside)) % 6
    put("one everywhere", g, [5, 20, 21, 22, 23, 24, 25])
    # the row-end pair
    if rows >= 2 and cols >= 3:
        g = grid()
        rm = rows // 2
        g[rm - 1, cols - 1], g[rm, 0] = 1, 2
        put("row-end pair", g, [1, 2])
    # the grid's four corners
    g = grid()
    for n, (r, c) in enumerate(((0, 0), (0, cols - 1), (rows - 1, 0), (rows - 1, cols - 1))):
        if g[r, c] < 0:
            g[r, c] = 30 + n
    put("four corners", g, [30, 31, 32, 33])
    # labels not asked for, -1, INT_MAX and negatives; duplicate and -1 slots
    g = rng.integers(0, 9, N).astype(np.int32).reshape(rows, cols)
    kind = rng.integers(0, 12, N).reshape(rows, cols)
    for k, v in ((0, -1), (1, INT_MAX), (2, -7), (3, -INT_MAX - 1)):
        g[kind == k] = v
    put("labels and slots that name nothing", g, [3, -1, 1, 3, INT_MAX, -7, 1, 6, 0, 77, -1])
    # blobs: a few random rectangles, the kind of map an inventory gives
    g = grid()
    for n in range(40):
        r, c = int(rng.integers(0, rows)), int(rng.integers(0, cols))
        g[r:r + int(rng.integers(1, 9)), c:c + int(rng.integers(1, 12))] = n % 14
    put("blobs", g, rng.permutation(14))
    for lab, objs in maps.values():
        assert lab.dtype == np.int32 and lab.shape == (N,) and objs.dtype == np.int32 and 1 <= objs.size <= 64
    return maps
