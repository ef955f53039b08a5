"""A plain-numpy reference of `eod_map_cover` and `eod_map_frontier` (include/eod_frontier.h) and the maps the tests run it on.  The
components are labelled by the iterated minimum over the neighbours (with a jump to the label's own label after every round, which
stays inside the component and only shortens the chains), no scipy; every other output is counted cell by cell from the definition."""
import numpy as np

INT_MAX = 2 ** 31 - 1
BLOCKED, OPEN, UNKNOWN = 0, 1, 2
TILE = 32                                                # the tile one workgroup labels in LDS (EOD_REGIONS_TILE_ROWS / _COLS)
CELL_KEYS = ("frontier_labels", "unknown_labels", "unknown_area")
SLOT_KEYS = ("frontier", "area", "bbox", "sum_rc", "open_edges", "behind_key", "behind_area", "behind_label", "reach_key", "reach_cost",
             "reach_cell")
WIDE = ("sum_rc", "behind_key", "reach_key")             # uint64 in the header, int64 tensors in Python
KEYS = CELL_KEYS + SLOT_KEYS + ("count", "counts", "status")
ALL_ONES = np.uint64(2 ** 64 - 1)


def cover_reference(proj, last_seen, stamp, exclude_cell=-1):
    """last_seen after one eod_map_cover (a copy)."""
    out = np.array(last_seen, np.int32)
    c = np.asarray(proj, np.int64).reshape(-1)
    c = c[(c >= 0) & (c < out.size) & (c != exclude_cell)]
    np.maximum.at(out, c, np.int32(stamp))
    return out


def kinds(labels, last_seen, since, passable=()):
    labels, last_seen = np.asarray(labels), np.asarray(last_seen)
    blocked = (labels >= 0) & ~np.isin(labels, np.asarray(passable, np.int64))
    return np.where(blocked, BLOCKED, np.where(last_seen >= since, OPEN, UNKNOWN)).astype(np.int8)


def _shift(a, dr, dc, fill):
    """b[r, c] = a[r + dr, c + dc], `fill` outside the grid."""
    rows, cols = a.shape
    b = np.full_like(a, fill)
    rs, rd = (slice(dr, rows), slice(0, rows - dr)) if dr >= 0 else (slice(0, rows + dr), slice(-dr, rows))
    cs, cd = (slice(dc, cols), slice(0, cols - dc)) if dc >= 0 else (slice(0, cols + dc), slice(-dc, cols))
    b[rd, cd] = a[rs, cs]
    return b


N4 = ((-1, 0), (1, 0), (0, -1), (0, 1))
N8 = N4 + ((-1, -1), (-1, 1), (1, -1), (1, 1))


def components(mask, conn8):
    """The label (lowest cell) of every cell of `mask` [rows, cols], -1 elsewhere."""
    rows, cols = mask.shape
    big = rows * cols
    lab = np.where(mask, np.arange(big, dtype=np.int64).reshape(rows, cols), big)
    while True:
        new = lab
        for dr, dc in (N8 if conn8 else N4):
            new = np.minimum(new, _shift(lab, dr, dc, big))
        new = np.where(mask, new, big)
        flat = new.reshape(-1)
        m = mask.reshape(-1)
        flat[m] = flat[flat[m]]                          # the label of a cell's label: a cell of the same component, not above it
        if np.array_equal(new, lab):
            break
        lab = new
    return np.where(mask, lab, -1).astype(np.int32)


def reference(labels, last_seen, cols, since=0, dist=None, from_cell=-1, passable=(), min_cells=2, topk=16, rank_by=1):
    labels = np.asarray(labels, np.int32)
    N = labels.size
    rows = N // cols
    assert rows * cols == N and rank_by in (0, 1)
    kind = kinds(labels, last_seen, since, passable).reshape(rows, cols)
    unknown = kind == UNKNOWN
    near = np.zeros((rows, cols), np.int64)              # UNKNOWN 4-neighbours of each cell
    for dr, dc in N4:
        near += _shift(unknown, dr, dc, False)
    fcell = (kind == OPEN) & (near > 0)
    fl = components(fcell, True).reshape(-1)
    ul = components(unknown, False).reshape(-1)
    ua = np.zeros(N, np.int32)
    np.add.at(ua, ul[ul >= 0], 1)
    ukey = np.zeros(N, np.uint64)                        # the key of the unknown region a cell lies in
    u = ul >= 0
    ukey[u] = (ua[ul[u]].astype(np.uint64) << np.uint64(32)) | (~ul[u]).astype(np.uint32).astype(np.uint64)
    behind_cell = np.zeros((rows, cols), np.uint64)      # per cell: the largest key among its UNKNOWN 4-neighbours
    for dr, dc in N4:
        behind_cell = np.maximum(behind_cell, _shift(ukey.reshape(rows, cols), dr, dc, 0))
    behind_cell = behind_cell.reshape(-1)
    r, c = np.divmod(np.arange(N, dtype=np.int64), cols)
    if dist is not None:
        v = np.asarray(dist, np.int64)
    elif from_cell >= 0:
        v = (r - from_cell // cols) ** 2 + (c - from_cell % cols) ** 2
    else:
        v = np.zeros(N, np.int64)
    roots = np.flatnonzero(fl == np.arange(N))
    info = {}
    for root in roots.tolist():
        cells = np.flatnonzero(fl == root)
        ok = cells[(v[cells] >= 0) & (v[cells] < INT_MAX)]
        reach = ALL_ONES if ok.size == 0 else ((v[ok].astype(np.uint64) << np.uint64(32)) | ok.astype(np.uint64)).min()
        info[root] = dict(area=cells.size, bbox=[r[cells].min(), c[cells].min(), r[cells].max(), c[cells].max()],
                          sum_rc=[r[cells].sum(), c[cells].sum()], open_edges=int(near.reshape(-1)[cells].sum()),
                          behind=behind_cell[cells].max(), reach=reach)
    listed = [t for t in roots.tolist() if info[t]["area"] >= min_cells]

    def rank(t):
        a = info[t]["area"] if rank_by == 0 else int(info[t]["behind"] >> np.uint64(32))
        return (a << 32) | ((~t) & 0xFFFFFFFF)
    order = sorted(listed, key=rank, reverse=True)[:topk]
    K = topk
    out = dict(frontier_labels=fl, unknown_labels=ul, unknown_area=ua, count=np.array([len(listed)], np.int32),
               frontier=np.full(K, -1, np.int32), area=np.zeros(K, np.int32), bbox=np.zeros((K, 4), np.int32),
               sum_rc=np.zeros((K, 2), np.uint64), open_edges=np.zeros(K, np.int32), behind_key=np.zeros(K, np.uint64),
               behind_area=np.zeros(K, np.int32), behind_label=np.full(K, -1, np.int32), reach_key=np.full(K, ALL_ONES, np.uint64),
               reach_cost=np.full(K, INT_MAX, np.int32), reach_cell=np.full(K, -1, np.int32),
               counts=np.array([(kind == BLOCKED).sum(), (kind == OPEN).sum(), unknown.sum(), fcell.sum(),
                                (ul == np.arange(N)).sum()], np.int32), status=np.zeros(2, np.int32))
    for k, t in enumerate(order):
        f = info[t]
        out["frontier"][k], out["area"][k], out["bbox"][k], out["sum_rc"][k] = t, f["area"], f["bbox"], f["sum_rc"]
        out["open_edges"][k], out["behind_key"][k] = f["open_edges"], f["behind"]
        out["behind_area"][k] = int(f["behind"] >> np.uint64(32))
        out["behind_label"][k] = (~int(f["behind"])) & 0xFFFFFFFF
        out["reach_key"][k] = f["reach"]
        if f["reach"] != ALL_ONES:
            out["reach_cost"][k], out["reach_cell"][k] = int(f["reach"] >> np.uint64(32)), int(f["reach"]) & 0xFFFFFFFF
    return out


def host(out):
    """A dict of tensors as the reference's arrays (the int64 tensors of the 64-bit keys as uint64)."""
    res = {}
    for k, v in out.items():
        a = v.detach().cpu().numpy() if hasattr(v, "detach") else np.asarray(v)
        res[k] = a.view(np.uint64) if k in WIDE and a.dtype == np.int64 else a
    return res


def differences(got, ref):
    return [k for k in KEYS if k not in got or got[k].shape != ref[k].shape or got[k].dtype != ref[k].dtype
            or not np.array_equal(got[k], ref[k])]


# ---- the maps --------------------------------------------------------------------------------------------------------------------
def hand_map():
    """The 6 x 8 map of include/eod_frontier.h: (labels, last_seen, cols, since, from_cell)."""
    rows, cols = 6, 8
    labels = np.full((rows, cols), -1, np.int32)
    labels[:, 4] = 3
    labels[2, 4] = -1
    seen = np.full((rows, cols), -1, np.int32)
    seen[:, :4] = 0
    seen[2, 4] = 0
    seen[5, 0] = -1
    seen[0, 4] = 5
    return labels.reshape(-1), seen.reshape(-1), cols, 0, 16


def corner_gadget(labels, seen, R, C, anti=False):
    """Round the tile corner whose lower right tile starts at (R, C): two frontier cells that touch only across the corner, and two
    UNKNOWN cells on the other diagonal that touch only there; the other neighbours of the UNKNOWN cells are walled off, so that the
    diagonal across the corner is the frontier's only link.  `anti`: the two diagonals change places."""
    rows, cols = labels.shape
    a, b = ((R - 1, C), (R, C - 1)) if anti else ((R - 1, C - 1), (R, C))              # the frontier cells
    u, w = ((R - 1, C - 1), (R, C)) if anti else ((R - 1, C), (R, C - 1))              # the UNKNOWN cells
    for rr in range(max(R - 3, 0), min(R + 3, rows)):
        for cc in range(max(C - 3, 0), min(C + 3, cols)):
            labels[rr, cc], seen[rr, cc] = -1, 0
    for cell in (u, w):
        if cell[0] < rows and cell[1] < cols:
            seen[cell] = -1
            for dr, dc in N4:
                rr, cc = cell[0] + dr, cell[1] + dc
                if 0 <= rr < rows and 0 <= cc < cols and (rr, cc) not in (a, b):
                    labels[rr, cc] = 5
    return a, b, u, w


def serpentine(rows, cols):
    """A one-cell path of OPEN cells through an UNKNOWN map: every even row, joined at alternating ends.  The path is one frontier
    through every tile; the odd rows' remains are long unknown regions."""
    seen = np.full((rows, cols), -1, np.int32)
    seen[0::2, :] = 0
    seen[1::4, cols - 1] = 0
    seen[3::4, 0] = 0
    return np.full(rows * cols, -1, np.int32), seen.reshape(-1)


def checkerboard(rows, cols):
    """Known cells on the even rows and columns only: rows / 2 * cols / 2 one-cell frontiers round one unknown region."""
    seen = np.full((rows, cols), -1, np.int32)
    seen[0::2, 0::2] = 0
    return np.full(rows * cols, -1, np.int32), seen.reshape(-1)


def explored(rows, cols, seed, walls=0.06, holes=0.02):
    """A map as a robot leaves it: discs of covered cells with stamps 0..3 round a few view points, walls of labels 0..5 (label 2 is
    used as passable), and single uncovered cells inside the known space."""
    rng = np.random.default_rng(seed)
    r, c = np.mgrid[0:rows, 0:cols]
    seen = np.full((rows, cols), -1, np.int32)
    for stamp in range(4):
        pr, pc = rng.integers(0, rows), rng.integers(0, cols)
        rad = max(2, int(0.3 * max(rows, cols)))
        seen[(r - pr) ** 2 + (c - pc) ** 2 <= rad * rad] = stamp
    seen[rng.random((rows, cols)) < holes] = -1
    labels = np.where(rng.random((rows, cols)) < walls, rng.integers(0, 6, (rows, cols)), -1).astype(np.int32)
    if rows > 4 and cols > 4:
        labels[rows // 2, : cols - 2] = 4                                # a long wall with a gap at its end
    return labels.reshape(-1), seen.reshape(-1)


def noise(rows, cols, seed, known=0.5, walls=0.1):
    rng = np.random.default_rng(seed)
    N = rows * cols
    seen = np.where(rng.random(N) < known, rng.integers(0, 4, N), -1).astype(np.int32)
    labels = np.where(rng.random(N) < walls, rng.integers(0, 6, N), -1).astype(np.int32)
    return labels, seen


def maps(rows, cols):
    """name -> dict(labels, last_seen) on a rows x cols grid."""
    N = rows * cols
    out = {}
    for seed in (1, 2):
        lab, seen = explored(rows, cols, seed)
        out[f"explored {seed}"] = dict(labels=lab, last_seen=seen)
    for known in (0.1, 0.5, 0.9):
        lab, seen = noise(rows, cols, int(known * 10), known)
        out[f"noise {known}"] = dict(labels=lab, last_seen=seen)
    out["all open"] = dict(labels=np.full(N, -1, np.int32), last_seen=np.zeros(N, np.int32))
    out["all unknown"] = dict(labels=np.full(N, -1, np.int32), last_seen=np.full(N, -1, np.int32))
    out["all blocked"] = dict(labels=np.full(N, 1, np.int32), last_seen=np.zeros(N, np.int32))
    lab, seen = serpentine(rows, cols)
    out["serpentine"] = dict(labels=lab, last_seen=seen)
    lab, seen = checkerboard(rows, cols)
    out["checkerboard"] = dict(labels=lab, last_seen=seen)
    return out


def corner_map(rows, cols, seed=3):
    """An explored map with a gadget at every tile corner of the grid (alternately the two diagonals): (labels, last_seen, gadgets)."""
    lab, seen = noise(rows, cols, seed, known=0.7, walls=0.05)
    lab, seen = lab.reshape(rows, cols).copy(), seen.reshape(rows, cols).copy()
    gadgets = []
    n = 0
    for R in range(TILE, rows, TILE):
        for C in range(TILE, cols, TILE):
            gadgets.append(corner_gadget(lab, seen, R, C, anti=bool(n % 2)) + (bool(n % 2),))
            n += 1
    return lab.reshape(-1), seen.reshape(-1), gadgets
