"""The exact reference of `ops.map_route` and the maps of its tests (numpy and heapq only).

The reference is written from the definition in include/eod_route.h, not from the kernels: a plain Dijkstra over the move rule,
then `parent`, the goals and the paths by their definitions.  Every comparison against it is integer equality."""
import heapq

import numpy as np

INT_MAX = 2 ** 31 - 1
INT_MIN = -2 ** 31
NONE = np.uint64(2 ** 64 - 1)
ORTH, DIAG = 5, 7
CELL_KEYS = ("dist", "parent")
SLOT_KEYS = ("goal_key", "goal_cost", "goal_cell", "cells", "path", "path_cells")
KEYS = CELL_KEYS + SLOT_KEYS + ("counts", "status")
MOVES = ((-1, -1), (-1, 0), (-1, 1), (0, -1), (0, 1), (1, -1), (1, 0), (1, 1))        # by the cell they come from, ascending
_REFS = {}


def slots(labels, objects):
    """int64 [N]: the lowest slot k with objects[k] == labels[i] and objects[k] >= 0; -1 where there is none."""
    labels = np.asarray(labels, dtype=np.int64)
    out = np.full(labels.shape, -1, np.int64)
    for k in range(len(objects) - 1, -1, -1):                        # the lowest slot is written last
        if objects[k] >= 0:
            out[labels == int(objects[k])] = k
    return out


def free_cells(labels, passable, from_cell):
    """bool [N]: a negative label, a passable label, or the start."""
    labels = np.asarray(labels, dtype=np.int64)
    f = labels < 0
    for p in passable:
        f |= labels == int(p)
    f[from_cell] = True
    return f


def legal(F, r, c, dr, dc):
    """A move from (r, c) to (r + dr, c + dc) on the free map F [rows, cols]: both on the grid and free, and a diagonal move with
    both cells it passes between free."""
    rows, cols = F.shape
    rr, cc = r + dr, c + dc
    if not (0 <= r < rows and 0 <= c < cols and 0 <= rr < rows and 0 <= cc < cols):
        return False
    if not (F[r, c] and F[rr, cc]):
        return False
    return dr == 0 or dc == 0 or bool(F[rr, c] and F[r, cc])


def reference(labels, objects, cols, from_cell, passable=(), path_max=256):
    """Every output of `ops.map_route` at status 0 as numpy arrays: goal_key uint64, the others int32."""
    labels = np.ascontiguousarray(labels, dtype=np.int32)
    objects = np.ascontiguousarray(objects, dtype=np.int32)
    passable = np.ascontiguousarray(passable, dtype=np.int32).reshape(-1)
    key = (labels.tobytes(), objects.tobytes(), passable.tobytes(), int(cols), int(from_cell), int(path_max))
    if key in _REFS:
        return _REFS[key]
    N, K = labels.size, objects.size
    rows = N // cols
    assert rows * cols == N and 1 <= K <= 64 and passable.size <= 64 and 0 <= from_cell < N and 1 <= path_max <= 1024
    F = free_cells(labels, passable, from_cell).reshape(rows, cols)
    S = slots(labels, objects).reshape(rows, cols)
    dist = np.full(N, INT_MAX, np.int64)
    dist[from_cell] = 0
    heap = [(0, int(from_cell))]
    while heap:
        d, i = heapq.heappop(heap)
        if d > dist[i]:
            continue
        r, c = divmod(i, cols)
        for dr, dc in MOVES:
            if legal(F, r, c, dr, dc):
                j = (r + dr) * cols + c + dc
                nd = d + (DIAG if dr and dc else ORTH)
                if nd < dist[j]:
                    dist[j] = nd
                    heapq.heappush(heap, (nd, j))
    parent = np.full(N, -1, np.int64)
    for i in range(N):
        if dist[i] == INT_MAX or i == from_cell:
            continue
        r, c = divmod(i, cols)
        for dr, dc in MOVES:                                         # the source (r + dr, c + dc), ascending: the first that fits
            if legal(F, r + dr, c + dc, -dr, -dc):
                j = (r + dr) * cols + c + dc
                if dist[j] != INT_MAX and dist[j] + (DIAG if dr and dc else ORTH) == dist[i]:
                    parent[i] = j
                    break
        assert parent[i] >= 0
    goal_key = np.full(K, NONE, np.uint64)
    for g in range(N):
        if dist[g] == INT_MAX:
            continue
        r, c = divmod(g, cols)
        for k in {int(S[rr, cc]) for rr in range(max(0, r - 1), min(rows, r + 2)) for cc in range(max(0, c - 1), min(cols, c + 2))}:
            if k >= 0:
                goal_key[k] = min(goal_key[k], np.uint64((int(dist[g]) << 32) | g))
    none = goal_key == NONE
    goal_cost = np.where(none, INT_MAX, (goal_key >> np.uint64(32)).astype(np.int64)).astype(np.int32)
    goal_cell = np.where(none, -1, (goal_key & np.uint64(0xFFFFFFFF)).astype(np.int64)).astype(np.int32)
    path = np.full((K, path_max), -1, np.int32)
    path_cells = np.zeros(K, np.int32)
    for k in range(K):
        cur, t = int(goal_cell[k]), 0
        while cur >= 0 and t < path_max:
            path[k, t] = cur
            t += 1
            if cur == from_cell:
                break
            cur = int(parent[cur])
        path_cells[k] = t
    flat = S.reshape(-1)
    out = dict(dist=dist.astype(np.int32), parent=parent.astype(np.int32), goal_key=goal_key, goal_cost=goal_cost, goal_cell=goal_cell,
               cells=np.bincount(flat[flat >= 0], minlength=K).astype(np.int32), path=path, path_cells=path_cells,
               counts=np.array([F.sum(), (dist != INT_MAX).sum()], np.int32), status=np.zeros(2, np.int32))
    _REFS[key] = out
    return out


def host(res):
    """The dict of `ops.map_route` as the reference's arrays (goal_key as uint64)."""
    out = {k: res[k].cpu().numpy() for k in KEYS}
    out["goal_key"] = out["goal_key"].view(np.uint64)
    return out


def differences(got, ref, keys=KEYS):
    """The names of the outputs that differ in type, shape or any bit."""
    return [k for k in keys if got[k].dtype != ref[k].dtype or got[k].shape != ref[k].shape or not np.array_equal(got[k], ref[k])]


def open_field(rows, cols, from_cell):
    """dist of a grid without blocked cells: 7 * min(dr, dc) + 5 * |dr - dc|."""
    fr, fc = divmod(from_cell, cols)
    dr = np.abs(np.arange(rows)[:, None] - fr)
    dc = np.abs(np.arange(cols)[None, :] - fc)
    return (DIAG * np.minimum(dr, dc) + ORTH * np.abs(dr - dc)).astype(np.int32).reshape(-1)


# ---- maps ---------------------------------------------------------------------------------------------------------------------
WALL = 1                                                             # a label no map asks for: it blocks and belongs to no slot


def spiral(h, w):
    """bool [h, w]: a corridor one cell wide that winds inwards from (0, 0), and its cells in order."""
    a = np.zeros((h, w), bool)
    a[0, 0] = True
    order = [(0, 0)]
    r = c = d = 0
    dirs = ((0, 1), (1, 0), (0, -1), (-1, 0))
    while True:
        for _ in range(2):
            dr, dc = dirs[d]
            nr, nc, fr, fc = r + dr, c + dc, r + 2 * dr, c + 2 * dc
            if 0 <= nr < h and 0 <= nc < w and not a[nr, nc] and not (0 <= fr < h and 0 <= fc < w and a[fr, fc]):
                r, c = nr, nc
                a[r, c] = True
                order.append((r, c))
                break
            d = (d + 1) % 4
        else:
            return a, order


def serpentine(rows, cols):
    """int32 [rows, cols]: a wall in every second row with a gap at alternating ends; the corridors are the even rows."""
    g = np.full((rows, cols), -1, np.int32)
    for w in range(1, rows, 2):
        g[w, :] = WALL
        g[w, cols - 1 if (w // 2) % 2 == 0 else 0] = -1
    return g


def maps(rows, cols, tile_rows, tile_cols):
    """{name: dict(labels int32 [N], objects int32 [K], passable int32 [P], from_cell)}: the maps of this op's own for one grid.
    Maps that need room are left out on grids without it."""
    N, tr, tc = rows * cols, tile_rows, tile_cols
    rng = np.random.default_rng(rows * 1000 + cols)
    out = {}

    def grid(fill=-1):
        return np.full((rows, cols), fill, np.int32)

    def put(name, g, objects, from_rc, passable=()):
        out[name] = dict(labels=g.reshape(-1).copy(), objects=np.asarray(objects, np.int32), passable=np.asarray(passable, np.int32),
                         from_cell=int(from_rc[0]) * cols + int(from_rc[1]))

    put("open", grid(), [10], (rows // 3, cols // 4))
    put("open from the last cell", grid(), [10, -1], (rows - 1, cols - 1))
    if rows >= 3 and cols >= 2:
        for name, gap in (("wall, gap at the tile border", min(tc, cols - 1)), ("wall, gap before the tile border", min(tc, cols) - 1),
                          ("wall, gap one off the tile border", min(tc + 1, cols - 1))):
            g = grid()
            m = min(tr, rows - 2) if rows > tr else rows // 2           # the wall is the first row of the second tile row
            g[m, :] = WALL
            g[m, gap] = -1
            g[rows - 1, 0] = 10
            g[0, cols - 1] = 11
            put(name, g, [10, 11], (0, 0))
    for name, m, q in (("corner opening", 2, 3), ("corner opening at the four-tile corner", tr - 1, tc - 1)):
        if rows >= m + 3 and cols >= q + 3:
            g = grid()
            g[m, :q + 1] = WALL
            g[m + 1, q + 1:] = WALL
            g[rows - 1, 0] = 10                                      # below the walls: no way there
            g[0, cols - 1] = 11
            put(name, g, [10, 11], (0, 0))
    if rows > tr and cols > tc:
        # tiles (0, 1) and (1, 0) blocked but for the two cells a diagonal step across the corner passes between; the rest of the
        # grid beyond the first 2 x 2 tiles blocked: the only way into tile (1, 1) is that step
        g = grid(WALL)
        g[:tr, :tc] = -1
        g[tr:2 * tr, tc:2 * tc] = -1
        g[tr - 1, tc] = g[tr, tc - 1] = -1
        g[min(rows, 2 * tr) - 1, min(cols, 2 * tc) - 1] = 10
        put("diagonal step across the four-tile corner", g, [10], (0, 0))
    if rows >= 4 and cols >= 2:
        g = grid()
        m = rows // 2 - 1
        g[m, :cols - 1] = WALL                                       # only (m, cols - 1) and (m + 1, 0) are free in these rows
        g[m + 1, 1:] = WALL
        g[rows - 1, cols - 1] = 10
        put("row-end pair as the only link", g, [10], (0, 0))
    if rows >= 5 and cols >= 5:
        h, w = min(rows, tr), min(cols, tc)
        a, order = spiral(h, w)
        g = grid(WALL)
        g[:h, :w][a] = -1
        er, ec = order[-1]
        beside = [(er + dr, ec + dc) for dr, dc in MOVES if 0 <= er + dr < h and 0 <= ec + dc < w and not a[er + dr, ec + dc]]
        g[beside[0]] = 10
        put("spiral inside one tile", g, [10], (0, 0))
    if rows >= 3 and cols >= 2:
        g = serpentine(rows, cols)
        last = (rows - 1) // 2 * 2                                   # the last corridor: the way in is at cols - 1 when last // 2 is odd
        g[last, 0 if (last // 2) % 2 == 1 else cols - 1] = 10        # the end opposite the way in
        put("serpentine", g, [10], (0, 0))
    if rows >= 3 and cols >= 3:
        g = grid()
        r, c = rows // 2, cols // 2
        g[max(0, r - 1):r + 2, max(0, c - 1):c + 2] = WALL
        g[r, c] = 10                                                 # enclosed by blocked cells: no free cell touches it
        g[0, cols - 1] = 11
        put("object enclosed", g, [11, 10], (rows - 1, 0))
        g = grid()
        g[max(0, r - 1):r + 2, max(0, c - 1):c + 2] = WALL
        g[r, c] = -1
        g[0, 0] = 10
        put("start enclosed", g, [WALL, 10], (r, c))
        g = grid()
        g[max(0, r - 1):r + 2, max(0, c - 1):c + 2] = 10
        g[0, cols - 1] = 11
        put("start on a labelled cell", g, [11, 10], (r, c))
        g = grid()
        g[max(0, r - 1):r + 2, max(0, c - 1):c + 2] = 12             # passable: its own cells are goals at d2 = 0
        g[0, :cols - 1] = 13
        g[rows - 1, 1:] = 14
        put("a slot made passable", g, [13, 12, 14], (rows - 1, 0), passable=[12, 99])
    if rows >= 4 and cols >= 7:
        g = grid()
        r, c = rows // 2 - 1, cols // 2
        g[r + 2, c - 2] = g[r + 2, c + 2] = 10                       # (r + 1, c - 1) and (r + 1, c + 1) both cost 7
        put("two goal cells of equal cost", g, [10], (r, c))
    g = rng.integers(0, 9, N).astype(np.int32).reshape(rows, cols)
    kind = rng.integers(0, 12, N).reshape(rows, cols)
    g[kind < 6] = -1
    for k, v in ((6, INT_MAX), (7, -7), (8, INT_MIN)):
        g[kind == k] = v
    put("labels and slots that name nothing", g, [3, -1, 1, 3, INT_MAX, -7, 1, 6, 0, 77, -1], (rows // 2, cols // 2),
        passable=[2, 5, 77, -7, INT_MAX, 5])
    g = grid()
    pick = rng.random(N).reshape(rows, cols) < 0.3
    g[pick] = (rng.integers(0, 64, N).reshape(rows, cols))[pick]
    put("64 objects", g, np.arange(64)[::-1], (rows - 1, cols // 2))
    for m in out.values():
        assert m["labels"].dtype == np.int32 and m["labels"].shape == (N,) and 1 <= m["objects"].size <= 64 and 0 <= m["from_cell"] < N
    return out
