"""A plain-numpy reference of `eod_map_heights` and `eod_map_obstacles`, written from include/eod_obstacles.h, and the records and maps
the tests run it on.  The record is made with `np.add.at`, `np.minimum.at` and `np.maximum.at` on the valid pixels; the structures by
a flood fill over the 8 neighbours from every OBSTACLE cell in ascending order (so a structure's first cell is its label); every other
output is counted cell by cell from the definition."""
import numpy as np

INT_MAX, INT_MIN = 2 ** 31 - 1, -2 ** 31
UNSEEN, CLEAR, OBSTACLE, OBJECT = 0, 1, 2, 3
TILE = 32                                                # the tile one workgroup labels in LDS (EOD_REGIONS_TILE_ROWS / _COLS)
CELL_KEYS = ("kind", "structure_labels", "merged_labels")
SLOT_KEYS = ("structure", "area", "bbox", "sum_rc", "top_mm")
OBJ_KEYS = ("obj_cells", "obj_seen_cells", "obj_top_mm", "obj_base_mm")
WIDE = ("sum_rc",)                                       # uint64 in the header, int64 tensors in Python
KEYS = CELL_KEYS + SLOT_KEYS + OBJ_KEYS + ("count", "counts", "status")
N8 = ((-1, -1), (-1, 0), (-1, 1), (0, -1), (0, 1), (1, -1), (1, 0), (1, 1))


def new_record(N):
    rec = np.zeros((4, N), np.int32)
    rec[2], rec[3] = INT_MAX, INT_MIN
    return rec


def millimetres(y):
    """q of the header for float32 heights: one fp32 product, ties to even."""
    return np.rint(np.asarray(y, np.float32) * np.float32(1000))


def heights_reference(proj, heights, record, band=(100, 1500), exclude_cell=-1):
    """The record after one eod_map_heights (a copy).  `heights`: one float32 per pixel."""
    out = np.array(record, np.int32)
    N = out.shape[1]
    c = np.asarray(proj, np.int64).reshape(-1)
    y = np.asarray(heights, np.float32).reshape(-1)
    assert c.size == y.size
    with np.errstate(invalid="ignore"):
        ok = (c >= 0) & (c < N) & (c != exclude_cell) & np.isfinite(y) & (np.abs(y) <= np.float32(1000.0))
    c = c[ok]
    q = millimetres(y[ok]).astype(np.int64)
    wide = out.astype(np.int64)
    np.add.at(wide[0], c, 1)
    np.add.at(wide[1], c, ((band[0] <= q) & (q <= band[1])).astype(np.int64))
    np.minimum.at(wide[2], c, q)
    np.maximum.at(wide[3], c, q)
    return wide.astype(np.int32)


def kinds(record, object_labels=None, min_hits=4):
    hits, band = np.asarray(record[0]), np.asarray(record[1])
    k = np.where(band >= min_hits, OBSTACLE, np.where(hits > 0, CLEAR, UNSEEN))
    if object_labels is not None:
        k = np.where(np.asarray(object_labels) >= 0, OBJECT, k)
    return k.astype(np.uint8)


def structures(mask):
    """The label (lowest cell) of every cell of `mask` [rows, cols] by flood fill over the 8 neighbours, -1 elsewhere."""
    rows, cols = mask.shape
    lab = np.full((rows, cols), -1, np.int32)
    m = mask.tolist()
    for start in np.flatnonzero(mask.reshape(-1)).tolist():
        r0, c0 = divmod(start, cols)
        if lab[r0, c0] >= 0:
            continue
        lab[r0, c0] = start
        stack = [(r0, c0)]
        while stack:
            r, c = stack.pop()
            for dr, dc in N8:
                rr, cc = r + dr, c + dc
                if 0 <= rr < rows and 0 <= cc < cols and m[rr][cc] and lab[rr, cc] < 0:
                    lab[rr, cc] = start
                    stack.append((rr, cc))
    return lab


def reference(record, cols, object_labels=None, objects=(), min_hits=4, min_cells=2, topk=16):
    record = np.asarray(record, np.int32)
    N = record.shape[1]
    rows = N // cols
    assert rows * cols == N
    hits, band, h_min, h_max = record
    kind = kinds(record, object_labels, min_hits)
    sl = structures((kind == OBSTACLE).reshape(rows, cols)).reshape(-1)
    r, c = np.divmod(np.arange(N, dtype=np.int64), cols)
    roots = np.flatnonzero(sl == np.arange(N)).tolist()
    area = np.bincount(sl[sl >= 0], minlength=N)
    keep = (sl >= 0) & (area[np.maximum(sl, 0)] >= min_cells)
    merged = np.where(kind == OBJECT, -1 if object_labels is None else np.asarray(object_labels), np.where(keep, sl, -1)).astype(np.int32)
    listed = [t for t in roots if area[t] >= min_cells]
    order = sorted(listed, key=lambda t: (int(area[t]) << 32) | ((~t) & 0xFFFFFFFF), reverse=True)[:topk]
    K, Ko = topk, len(objects)
    out = dict(kind=kind, structure_labels=sl, merged_labels=merged, count=np.array([len(listed)], np.int32),
               structure=np.full(K, -1, np.int32), area=np.zeros(K, np.int32), bbox=np.zeros((K, 4), np.int32),
               sum_rc=np.zeros((K, 2), np.uint64), top_mm=np.full(K, INT_MIN, np.int32),
               obj_cells=np.zeros(Ko, np.int32), obj_seen_cells=np.zeros(Ko, np.int32), obj_top_mm=np.full(Ko, INT_MIN, np.int32),
               obj_base_mm=np.full(Ko, INT_MAX, np.int32),
               counts=np.array([(kind == UNSEEN).sum(), (kind == CLEAR).sum(), (kind == OBSTACLE).sum(), (kind == OBJECT).sum(),
                                len(roots), ((sl >= 0) & ~keep).sum()], np.int32), status=np.zeros(2, np.int32))
    for k, t in enumerate(order):
        cells = np.flatnonzero(sl == t)
        out["structure"][k], out["area"][k] = t, cells.size
        out["bbox"][k] = [r[cells].min(), c[cells].min(), r[cells].max(), c[cells].max()]
        out["sum_rc"][k] = [r[cells].sum(), c[cells].sum()]
        out["top_mm"][k] = h_max[cells].max()
    if object_labels is not None:
        labels = np.asarray(object_labels)
        taken = set()
        for k, t in enumerate(objects):                  # the lowest slot that holds a label takes its cells
            t = int(t)
            if t < 0 or t in taken:
                continue
            taken.add(t)
            cells = np.flatnonzero(labels == t)
            seen = cells[hits[cells] > 0]
            out["obj_cells"][k], out["obj_seen_cells"][k] = cells.size, seen.size
            if seen.size:
                out["obj_top_mm"][k], out["obj_base_mm"][k] = h_max[seen].max(), h_min[seen].min()
    return out


def host(out):
    """A dict of tensors as the reference's arrays (the int64 tensors of the 64-bit sums as uint64)."""
    res = {}
    for k, v in out.items():
        a = v.detach().cpu().numpy() if hasattr(v, "detach") else np.asarray(v)
        res[k] = a.view(np.uint64) if k in WIDE and a.dtype == np.int64 else a
    return res


def differences(got, ref):
    return [k for k in KEYS if k not in got or got[k].shape != ref[k].shape or got[k].dtype != ref[k].dtype
            or not np.array_equal(got[k], ref[k])]


# ---- the hand-worked examples of the header ----------------------------------------------------------------------------------------
def hand_record():
    """(proj, heights, N, band, exclude_cell, the record to expect as rows of (hits, band_hits, min, max) per cell)."""
    px = [(0, 0.0), (0, -0.25), (1, 0.5), (1, 1.25), (1, 2.0), (2, 0.0625), (2, 0.099609375), (2, 1.5009765625), (3, np.nan),
          (3, np.inf), (-1, 0.5), (6, 0.5), (5, 0.5), (4, 1000.5), (4, 1.5)]
    proj = np.array([p[0] for p in px], np.int32)
    y = np.array([p[1] for p in px], np.float32)
    want = [(2, 0, -250, 0), (3, 2, 500, 2000), (3, 1, 62, 1501), (0, 0, INT_MAX, INT_MIN), (1, 1, 1500, 1500), (0, 0, INT_MAX, INT_MIN)]
    return proj, y, 6, (100, 1500), 5, want


def hand_map():
    """The 4 x 6 map of the header: (record, cols, object_labels, min_hits, min_cells)."""
    rows, cols = 4, 6
    rec = new_record(rows * cols)
    hits = np.full(rows * cols, 3, np.int32)
    hits[[4, 5, 10, 11, 17, 23, 14]] = 0
    rec[0] = hits
    seen = hits > 0
    rec[2][seen] = 10 + np.arange(rows * cols)[seen]
    rec[3][seen] = 700 + 10 * np.arange(rows * cols)[seen]
    for cell, b in ((0, 2), (1, 3), (8, 2), (16, 2), (13, 5), (9, 1)):
        rec[1][cell] = b
        rec[0][cell] = max(rec[0][cell], b)
    labels = np.full(rows * cols, -1, np.int32)
    labels[[13, 14]] = 13
    return rec, cols, labels, 2, 2


# ---- the maps ----------------------------------------------------------------------------------------------------------------------
def record_from_kinds(kind, seed=0):
    """A consistent record whose kinds (without objects, min_hits 4) are `kind` (UNSEEN / CLEAR / OBSTACLE), with heights that differ
    from cell to cell."""
    kind = np.asarray(kind).reshape(-1)
    N = kind.size
    rng = np.random.default_rng(seed)
    rec = new_record(N)
    seen = kind != UNSEEN
    rec[0] = np.where(seen, rng.integers(1, 40, N), 0)
    rec[1] = np.where(kind == OBSTACLE, rng.integers(4, 9, N), np.where(seen, rng.integers(0, 4, N), 0))
    rec[0] = np.maximum(rec[0], rec[1])
    lo = rng.integers(-300, 900, N)
    rec[2] = np.where(seen, lo, INT_MAX)
    rec[3] = np.where(seen, lo + rng.integers(0, 2500, N), INT_MIN)
    return rec


def wall_with_door(rows, cols, door=True):
    k = np.full((rows, cols), CLEAR, np.uint8)
    if cols >= 3:
        k[:, cols // 2] = OBSTACLE
        if door:
            k[rows // 2, cols // 2] = CLEAR
    return k


def checkerboard(rows, cols):
    """Obstacles on the cells with an even row + column: one structure through the corners."""
    r, c = np.mgrid[0:rows, 0:cols]
    return np.where((r + c) % 2 == 0, OBSTACLE, CLEAR).astype(np.uint8)


def spirals(rows, cols):
    """Two spirals of OBSTACLE cells wound into each other (every fourth ring line, cut open), which never touch: long merge
    chains through every tile."""
    def spiral(h, w, pitch=4):
        """One arm wound inward from (0, 0), its turns `pitch` cells apart: it goes on while the next cell is inside and no cell is
        drawn yet within `pitch` - 1 of it ahead or to either side."""
        a = np.zeros((h, w), bool)
        if h < 1 or w < 1:
            return a
        drawn = lambda rr, cc: 0 <= rr < h and 0 <= cc < w and a[rr, cc]
        r = c = d = 0
        a[0, 0] = True
        turned = 0
        while turned < 2:
            dr, dc = ((0, 1), (1, 0), (0, -1), (-1, 0))[d]
            nr, nc = r + dr, c + dc
            free = 0 <= nr < h and 0 <= nc < w and not any(
                drawn(nr + k * dr, nc + k * dc) or drawn(nr + k * dc, nc - k * dr) or drawn(nr - k * dc, nc + k * dr)
                for k in range(1, pitch))
            if free:
                r, c, turned = nr, nc, 0
                a[r, c] = True
            else:
                d, turned = (d + 1) % 4, turned + 1
        return a
    k = np.full((rows, cols), CLEAR, np.uint8)
    k[spiral(rows, cols)] = OBSTACLE
    if rows > 4 and cols > 4:                            # the second arm: the same, two cells further in
        k[2:rows - 2, 2:cols - 2][spiral(rows - 4, cols - 4)] = OBSTACLE
    return k


def random_kinds(rows, cols, density, seed):
    rng = np.random.default_rng(seed)
    u = rng.random((rows, cols))
    return np.where(u < density, OBSTACLE, np.where(u < density + 0.25, UNSEEN, CLEAR)).astype(np.uint8)


def many_structures(rows, cols):
    """Blocks of 1 to 3 cells every third column of every other row: more structures than 64 slots on all but the smallest grids,
    with ties in the area."""
    k = np.full((rows, cols), CLEAR, np.uint8)
    n = 0
    for r in range(0, rows, 2):
        for c in range(0, cols, 4):
            k[r, c:c + 1 + n % 3] = OBSTACLE
            n += 1
    return k


def specks(rows, cols):
    k = np.full((rows, cols), CLEAR, np.uint8)
    k[0::3, 0::3] = OBSTACLE
    return k


def objects_over(rows, cols, kind, seed):
    """Lowest-cell labels of a few rectangles laid over `kind` (obstacle cells included), and one object on UNSEEN ground."""
    rng = np.random.default_rng(seed)
    labels = np.full((rows, cols), -1, np.int32)
    kind = kind.copy()
    for _ in range(6):
        r0, c0 = int(rng.integers(0, rows)), int(rng.integers(0, cols))
        r1, c1 = min(rows, r0 + int(rng.integers(1, 5))), min(cols, c0 + int(rng.integers(1, 5)))
        if (labels[r0:r1, c0:c1] >= 0).any():
            continue
        labels[r0:r1, c0:c1] = r0 * cols + c0
    never = np.flatnonzero(labels.reshape(-1) >= 0)
    if never.size:
        t = labels.reshape(-1)[never[-1]]
        kind[labels == t] = UNSEEN                       # an object never seen
    return labels.reshape(-1), kind


def maps(rows, cols):
    """name -> dict(record [4, N], labels [N] or None, objects)."""
    N = rows * cols
    out = {}

    def add(name, kind, labels=None, objects=(), seed=0):
        out[name] = dict(record=record_from_kinds(kind, seed), labels=labels, objects=tuple(objects))
    add("all unseen", np.full(N, UNSEEN, np.uint8))
    add("all clear", np.full(N, CLEAR, np.uint8))
    add("all obstacle", np.full(N, OBSTACLE, np.uint8))
    add("wall with a door", wall_with_door(rows, cols))
    add("checkerboard", checkerboard(rows, cols))
    add("spirals", spirals(rows, cols))
    add("spirals, transposed", np.ascontiguousarray(spirals(cols, rows).T))
    for density in (0.1, 0.4, 0.7):
        add(f"random {density}", random_kinds(rows, cols, density, int(density * 10)), seed=int(density * 10))
    add("many structures", many_structures(rows, cols))
    add("specks only", specks(rows, cols))
    labels, kind = objects_over(rows, cols, random_kinds(rows, cols, 0.35, 11), 12)
    objs = sorted(set(labels[labels >= 0].tolist()))
    add("objects over obstacles", kind, labels, objs[:3] + objs[:1] + [-1, N + 5] + objs[3:], seed=5)
    return out
