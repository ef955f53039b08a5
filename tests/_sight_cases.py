"""The exact reference of `ops.map_sight` and the maps of its tests (numpy only).

The reference is written from the definitions in include/eod_sight.h, not from the kernels: the closed form
rnd(a, n) = sign(a) * floor((2 |a| + n) / (2 n)) in int64 for line cell i of every target at once, one loop over i, then the other
outputs by their definitions.  Only the window of cells with d2 <= range2 round a source is walked (a line never leaves the box its
two ends span); everything outside it is unseen by rule 1.  Every comparison against it is integer equality."""
import math

import numpy as np

INT_MAX = 2 ** 31 - 1
INT_MIN = -2 ** 31
PAIR_KEYS = ("seen_cells", "near_key", "near_d2", "near_cell")
SLOT_KEYS = ("cells", "best_key", "best_seen", "best_source")
KEYS = ("seen_mask",) + PAIR_KEYS + SLOT_KEYS + ("source_counts", "counts", "status")
WIDE = ("seen_mask", "near_key", "best_key")                         # uint64 in the reference, int64 bits in torch
_REFS = {}


def slots(labels, objects):
    """int64 [N]: the lowest slot k with objects[k] == labels[i] and objects[k] >= 0; -1 where there is none."""
    labels = np.asarray(labels, dtype=np.int64)
    out = np.full(labels.shape, -1, np.int64)
    for k in range(len(objects) - 1, -1, -1):                        # the lowest slot is written last
        if objects[k] >= 0:
            out[labels == int(objects[k])] = k
    return out


def opaque_cells(labels, passable):
    """bool [N]: a label >= 0 that is not passable."""
    labels = np.asarray(labels, dtype=np.int64)
    b = labels >= 0
    for p in passable:
        b &= labels != int(p)
    return b


def rnd(a, n):
    """a / n to the nearest integer, a half away from zero (int64 arrays, n >= 1)."""
    return np.sign(a) * ((2 * np.abs(a) + n) // (2 * n))


def seen_from(opaque, source, range2=INT_MAX):
    """bool [rows, cols]: the cells the cell `source` of the bool [rows, cols] map `opaque` sees."""
    rows, cols = opaque.shape
    r0, c0 = divmod(int(source), cols)
    O = opaque.copy()
    O[r0, c0] = False                                                # the robot stands there
    reach = min(math.isqrt(int(range2)), max(rows, cols))
    ra, rb, ca, cb = max(0, r0 - reach), min(rows, r0 + reach + 1), max(0, c0 - reach), min(cols, c0 + reach + 1)
    R, C = np.meshgrid(np.arange(ra, rb, dtype=np.int64), np.arange(ca, cb, dtype=np.int64), indexing="ij")
    R, C = R.reshape(-1), C.reshape(-1)
    dr, dc = R - r0, C - c0
    inside = dr * dr + dc * dc <= int(range2)
    R, C, dr, dc = R[inside], C[inside], dr[inside], dc[inside]
    n = np.maximum(np.abs(dr), np.abs(dc))
    seen = np.zeros((rows, cols), bool)
    seen[r0, c0] = True                                              # n == 0: a source sees its own cell
    alive = np.flatnonzero(n >= 1)
    pr, pc = np.full(alive.size, r0, np.int64), np.full(alive.size, c0, np.int64)
    for i in range(1, int(n.max()) + 1 if n.size else 0):
        na = n[alive]
        r, c = r0 + rnd(i * dr[alive], na), c0 + rnd(i * dc[alive], na)
        assert (np.abs(r - pr) <= 1).all() and (np.abs(c - pc) <= 1).all()
        blocked = (r != pr) & (c != pc) & O[pr, c] & O[r, pc]        # between two opaque cells that touch at a corner
        blocked |= (i < na) & O[r, c]                                # the target itself may be opaque
        done = (i == na) & ~blocked
        assert (r[done] == R[alive[done]]).all() and (c[done] == C[alive[done]]).all()          # cell n is the target
        seen[r[done], c[done]] = True
        go = ~blocked & (i < na)
        alive, pr, pc = alive[go], r[go], c[go]
    return seen


def reference(labels, objects, cols, from_cells, range2=INT_MAX, passable=()):
    """Every output of `ops.map_sight` as numpy arrays: seen_mask, near_key and best_key uint64, the others int32."""
    labels = np.ascontiguousarray(labels, dtype=np.int32)
    objects = np.ascontiguousarray(objects, dtype=np.int32)
    passable = np.ascontiguousarray(passable, dtype=np.int32).reshape(-1)
    from_cells = np.ascontiguousarray(from_cells, dtype=np.int32).reshape(-1)
    key = (labels.tobytes(), objects.tobytes(), passable.tobytes(), from_cells.tobytes(), int(cols), int(range2))
    if key in _REFS:
        return _REFS[key]
    N, K, S = labels.size, objects.size, from_cells.size
    rows = N // cols
    assert rows * cols == N and 1 <= K <= 64 and passable.size <= 64 and 1 <= S <= 64 and 0 <= range2 <= INT_MAX
    assert rows <= 32767 and cols <= 32767 and (from_cells < N).all()
    B = opaque_cells(labels, passable)
    slot = slots(labels, objects)
    cell = np.arange(N, dtype=np.int64)
    r, c = cell // cols, cell % cols
    seen_mask = np.zeros(N, np.uint64)
    seen_cells = np.zeros((S, K), np.int64)
    near_key = np.full((S, K), 2 ** 64 - 1, np.uint64)
    source_counts = np.zeros((S, 2), np.int64)
    views = {}
    for s in range(S):
        f = int(from_cells[s])
        if f < 0:
            continue
        if f not in views:
            views[f] = seen_from(B.reshape(rows, cols), f, range2).reshape(-1)
        seen = views[f]
        assert seen[f]                                               # a source sees its own cell
        seen_mask |= seen.astype(np.uint64) << np.uint64(s)
        source_counts[s] = ((seen & ~B).sum(), (seen & B).sum())
        d2 = (r - f // cols) ** 2 + (c - f % cols) ** 2
        keys = (d2.astype(np.uint64) << np.uint64(32)) | cell.astype(np.uint64)
        for k in range(K):
            mine = seen & (slot == k)
            seen_cells[s, k] = mine.sum()
            if seen_cells[s, k]:
                near_key[s, k] = keys[mine].min()
    none = near_key == np.uint64(2 ** 64 - 1)
    near_d2 = np.where(none, INT_MAX, (near_key >> np.uint64(32)).astype(np.int64))
    near_cell = np.where(none, -1, (near_key & np.uint64(0xFFFFFFFF)).astype(np.int64))
    best_key = np.zeros(K, np.uint64)
    for k in range(K):
        for s in range(S):
            if from_cells[s] >= 0 and seen_cells[s, k] > 0:
                best_key[k] = max(int(best_key[k]), (int(seen_cells[s, k]) << 32) | (0xFFFFFFFF - s))
    best_seen = (best_key >> np.uint64(32)).astype(np.int64)
    best_source = np.where(best_key == 0, -1, 0xFFFFFFFF - (best_key & np.uint64(0xFFFFFFFF)).astype(np.int64))
    out = dict(seen_mask=seen_mask, cells=np.bincount(slot[slot >= 0], minlength=K).astype(np.int32),
               seen_cells=seen_cells.astype(np.int32), near_key=near_key, near_d2=near_d2.astype(np.int32),
               near_cell=near_cell.astype(np.int32), best_key=best_key, best_seen=best_seen.astype(np.int32),
               best_source=best_source.astype(np.int32), source_counts=source_counts.astype(np.int32),
               counts=np.array([B.sum(), (~B).sum(), (seen_mask != 0).sum()], np.int32), status=np.zeros(2, np.int32))
    _REFS[key] = out
    return out


def seen_rows(ref, s, rows, cols):
    """The `seen` of source s as the strings of the header's hand-worked maps."""
    bits = ((ref["seen_mask"] >> np.uint64(s)) & np.uint64(1)).astype(np.int64).reshape(rows, cols)
    return ["".join(str(v) for v in row) for row in bits]


def host(res):
    """The dict of `ops.map_sight` as the reference's arrays (seen_mask and the keys as uint64)."""
    out = {k: res[k].cpu().numpy() for k in KEYS}
    for k in WIDE:
        out[k] = out[k].view(np.uint64)
    return out


def differences(got, ref, keys=KEYS):
    """The names of the outputs that differ in type, shape or any bit."""
    return [k for k in keys if got[k].dtype != ref[k].dtype or got[k].shape != ref[k].shape or not np.array_equal(got[k], ref[k])]


# ---- maps ---------------------------------------------------------------------------------------------------------------------
WALL = 1                                                             # a label no map asks for: opaque, and in no slot
HAND = {                                                             # the header's hand-worked maps: (rows, cols, {cell: label}, {source: seen})
    "A": (5, 7, {(1, 2): 9, (2, 3): 4}, {14: ["1110000", "1110000", "1111000", "1111111", "1111111"]}),
    "B": (3, 3, {(0, 1): 1, (1, 0): 2}, {0: ["110", "100", "000"]}),
    "C": (3, 3, {(0, 1): 1}, {0: ["110", "111", "111"]}),
    "D": (3, 5, {(1, 2): 1}, {0: ["11111", "11100", "11100"], 14: ["00111", "00111", "11111"]}),
}
HALF_TIES = ((1, 2), (1, 4), (3, 6))                                 # minor : major steps of a line with a line cell on a half


def hand_map(name):
    rows, cols, put, want = HAND[name]
    g = np.full((rows, cols), -1, np.int32)
    for rc, v in put.items():
        g[rc] = v
    return g, want


def tie_cells(a, b):
    """[(i, picked minor coordinate, the one not picked)] of the line cells of a line of `a` minor and `b` major steps that lie on a half."""
    return [(i, (2 * i * a + b) // (2 * b), (2 * i * a + b) // (2 * b) - 1) for i in range(1, b) if (2 * i * a) % (2 * b) == b]


def maps(rows, cols, wg=256):
    """{name: dict(labels int32 [N], objects int32 [K], passable int32 [P], from_cells int32 [S], range2)}: the maps of this op's own
    for one grid.  Maps that need room are left out on grids without it."""
    N = rows * cols
    rng = np.random.default_rng(rows * 1000 + cols)
    out = {}
    y, x = rows // 2, cols // 2
    centre = y * cols + x
    usual = [centre, 0, -1, N - 1 - cols // 3, centre, (rows - 1) * cols]           # the centre, a corner, unused, the last row, a duplicate

    def grid(fill=-1):
        return np.full((rows, cols), fill, np.int32)

    def put(name, g, objects, from_cells=None, range2=INT_MAX, passable=()):
        out[name] = dict(labels=g.reshape(-1).copy(), objects=np.asarray(objects, np.int32), passable=np.asarray(passable, np.int32),
                         from_cells=np.asarray(usual if from_cells is None else from_cells, np.int32), range2=int(range2))

    put("no opaque cell", grid(), [10, -1])
    put("negative labels only", grid(-7), [10])
    g = grid(10)
    g[y:, :] = 11
    put("every cell opaque", g, [11, 10, 12])
    if rows >= 2:
        g = grid()
        g[y - 1, cols - 1] = 10                                      # (y, 0) follows it in memory: it hides nothing from a source in row y
        put("row-end pair", g, [10], [y * cols + cols - 1, y * cols + cols // 2, y * cols])
    if rows >= 3 and cols >= 3:
        # a source on an opaque cell, and a second source whose line crosses it
        g = grid()
        g[y, x] = 10
        g[y, max(0, x - 1)] = 11
        put("a source on an opaque cell", g, [10, 11], [centre, y * cols, centre - 1, 0])
        for n, (dy, dx) in enumerate(((-1, -1), (-1, 0), (-1, 1), (0, -1), (0, 1), (1, -1), (1, 0), (1, 1))):
            g = grid()
            g[y + dy, x + dx] = 10
            put(f"neighbour {dy:+d}{dx:+d}", g, [10], [centre, 0] if n % 2 else [centre])
    if rows >= 15 and cols >= 15:
        for a, b in HALF_TIES:
            for i, picked, other in tie_cells(a, b):
                for which, minor in (("picked", picked), ("not picked", other)):
                    # the four octants along the columns and the four along the rows, apart: at step 1 the cells not picked are
                    # the source's four neighbours, and all four at once would close every diagonal by the corner rule
                    for along in ("columns", "rows"):
                        g = grid()
                        for sy in (-1, 1):
                            for sx in (-1, 1):
                                if along == "columns":
                                    g[y + sy * minor, x + sx * i] = 10
                                else:
                                    g[y + sy * i, x + sx * minor] = 11
                        put(f"half tie {a}:{b} at step {i}, {which}, along the {along}", g, [10, 11], [centre])
        for name, sides, target in (("both", (1, 1), False), ("one side", (1, 0), False), ("the other side", (0, 1), False),
                                    ("both, opaque target", (1, 1), True), ("one side, opaque target", (1, 0), True),
                                    ("neither, opaque target", (0, 0), True)):
            g = grid()
            for sy in (-1, 1):
                for sx in (-1, 1):                                   # the step (2, 2) -> (3, 3) of each diagonal
                    if sides[0]:
                        g[y + 2 * sy, x + 3 * sx] = 10
                    if sides[1]:
                        g[y + 3 * sy, x + 2 * sx] = 11
                    if target:
                        g[y + 3 * sy, x + 3 * sx] = 12
            put(f"corner pair: {name}", g, [12, 11, 10], [centre, 0])
    # opaque cells on the last bit of a bit-plane word and the first of the next, and either side of a workgroup border
    for name, step in (("word", 64), ("workgroup", wg)):
        if N > step + 1:
            for off in (-1, 0):
                g = grid().reshape(-1)
                g[np.arange(step, N, step) + off] = 10
                put(f"{name} border {off:+d}", g.reshape(rows, cols), [10], [centre, 0, N - 1])
    if rows >= 3 and cols >= 3:
        g = grid()
        g[max(0, y - 1):y + 2, max(0, x - 1):x + 2] = 12             # passable: transparent, with cells of its own
        g[0, :cols - 1] = 13
        g[rows - 1, 1:] = 14
        put("a slot made passable", g, [13, 12, 14], [centre, cols - 1, (rows - 1) * cols], passable=[12, 99])
    g = rng.integers(0, 9, N).astype(np.int32).reshape(rows, cols)
    kind = rng.integers(0, 24, N).reshape(rows, cols)
    g[kind < 18] = -1
    for k, v in ((18, INT_MAX), (19, -7), (20, INT_MIN)):
        g[kind == k] = v
    put("labels and slots that name nothing", g, [3, -1, 1, 3, INT_MAX, -7, 1, 6, 0, 77, -1], passable=[2, 5, 77, -7, INT_MAX, 5])
    g = grid()
    pick = rng.random(N).reshape(rows, cols) < 0.05
    g[pick] = (rng.integers(0, 64, N).reshape(rows, cols))[pick]
    many = rng.integers(0, N, 64).astype(np.int32)
    many[5], many[17], many[40], many[63] = -1, INT_MIN, many[3], many[0]                  # unused and duplicate sources
    put("64 objects, 64 sources", g, np.arange(64)[::-1], many)
    put("one object, one source", g, [7], [centre])
    put("64 objects, one source", g, np.arange(64), [N - 1])
    put("one object, 64 sources", g, [7], many)
    for m in out.values():
        assert m["labels"].dtype == np.int32 and m["labels"].shape == (N,) and 1 <= m["objects"].size <= 64
        assert 1 <= m["from_cells"].size <= 64 and (m["from_cells"] < N).all()
    return out


def ranges(rows, cols):
    """The range2 of the tests: 0, 1, 2, 25, one past the largest d2 of the grid, and unbounded."""
    return (0, 1, 2, 25, (rows - 1) ** 2 + (cols - 1) ** 2 + 1, INT_MAX)
