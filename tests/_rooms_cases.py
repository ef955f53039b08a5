"""The rooms on the map in plain numpy, written from include/eod_rooms.h alone, and the maps the tests run on.  The reference
takes no short cut the kernels take: d2 by brute force over the blocked cells, the core regions by a flood fill in raster order,
the grow by Dijkstra on (g, room) pairs, every table by a loop over the cells."""
import heapq

import numpy as np

INT_MAX = 2 ** 31 - 1
TILE = 32                                                # the tile one workgroup owns (EOD_ROOMS_TILE_ROWS / _COLS)
ORTH, DIAG = 5, 7                                        # EOD_ROUTE_COST_ORTH, EOD_ROUTE_COST_DIAG
CELL_KEYS = ("room_labels", "grow_dist")
SLOT_KEYS = ("room", "area", "core_area", "bbox", "sum_rc", "widest_key", "widest_d2", "widest_cell", "room_objects")
PAIR_KEYS = ("door_edges", "door_key", "door_d2", "door_cell")
OBJ_KEYS = ("obj_room_cells", "obj_room", "obj_room_label")
WIDE = ("sum_rc", "widest_key", "door_key")              # uint64 in the header, int64 tensors in Python
KEYS = CELL_KEYS + SLOT_KEYS + PAIR_KEYS + OBJ_KEYS + ("count", "counts", "status")
MOVES = [(-1, -1), (-1, 0), (-1, 1), (0, -1), (0, 1), (1, -1), (1, 0), (1, 1)]


def blocked_cells(labels, passable=()):
    labels = np.asarray(labels)
    return (labels >= 0) & ~np.isin(labels, np.asarray(list(passable), dtype=np.int64))


def brute_d2(labels, cols, passable=()):
    """d2 of eod_map_clearance: the squared distance to the nearest blocked cell, by brute force; INT_MAX without one."""
    b = blocked_cells(labels, passable)
    N = b.size
    r, c = np.divmod(np.arange(N), cols)
    if not b.any():
        return np.full(N, INT_MAX, np.int32)
    br, bc = r[b].astype(np.int64), c[b].astype(np.int64)
    out = np.empty(N, np.int64)
    for a in range(0, N, 512):
        out[a:a + 512] = ((r[a:a + 512, None] - br[None]) ** 2 + (c[a:a + 512, None] - bc[None]) ** 2).min(axis=1)
    return out.astype(np.int32)


def slots_of(labels, objects):
    """SLOT: the lowest slot that holds the cell's label; -1."""
    slot = np.full(len(labels), -1, np.int64)
    for k in range(len(objects) - 1, -1, -1):
        if objects[k] >= 0:
            slot[np.asarray(labels) == objects[k]] = k
    return slot


def reference(labels, cols, door_r2, min_cells=1, topk=16, objects=(), passable=(), known=None, d2=None, tie_high=False):
    """Every output of eod_map_rooms.  `tie_high` (not in the header) hands a cell that several rooms reach at the same cost to the
    highest label: where both rules agree, one room alone attains the cost."""
    labels = np.asarray(labels, np.int32)
    N = labels.size
    rows = N // cols
    objects = [int(v) for v in objects]
    K, Ko = int(topk), len(objects)
    if d2 is None:
        d2 = brute_d2(labels, cols, passable)
    d2 = np.asarray(d2, np.int64)
    blocked = blocked_cells(labels, passable)
    void = ~blocked & (np.asarray(known) == 0) if known is not None else np.zeros(N, bool)
    free = ~blocked & ~void
    core = free & (d2 > door_r2)
    F, C = free.reshape(rows, cols), core.reshape(rows, cols)
    # the core regions: a flood fill from every core cell not yet labelled, in raster order, so the label is the lowest cell
    core_lab = np.full(N, -1, np.int64)
    core_size = {}
    for i in range(N):
        if not core[i] or core_lab[i] >= 0:
            continue
        core_lab[i] = i
        stack, n = [i], 0
        while stack:
            j = stack.pop()
            n += 1
            r, c = divmod(j, cols)
            for rr, cc in ((r - 1, c), (r, c - 1), (r, c + 1), (r + 1, c)):
                if 0 <= rr < rows and 0 <= cc < cols and C[rr, cc] and core_lab[rr * cols + cc] < 0:
                    core_lab[rr * cols + cc] = i
                    stack.append(rr * cols + cc)
        core_size[i] = n
    rooms = sorted(l for l, n in core_size.items() if n >= min_cells)
    # the grow: Dijkstra on (g, room); adding a cost keeps the order of two keys, so the first pop of a cell is its smallest key
    key = {}
    heap = []
    sgn = -1 if tie_high else 1
    for i in range(N):
        if core_lab[i] >= 0 and core_size[core_lab[i]] >= min_cells:
            key[i] = (0, sgn * int(core_lab[i]))
            heap.append((0, sgn * int(core_lab[i]), i))
    heapq.heapify(heap)
    done = np.zeros(N, bool)
    while heap:
        g, room, j = heapq.heappop(heap)
        if done[j]:
            continue
        done[j] = True
        r, c = divmod(j, cols)
        for dr, dc in MOVES:
            rr, cc = r + dr, c + dc
            if not (0 <= rr < rows and 0 <= cc < cols) or not F[rr, cc]:
                continue
            if dr and dc and not (F[r + dr, c] and F[r, c + dc]):
                continue                                                  # no squeezing between two cells that touch at a corner
            t = rr * cols + cc
            cand = (g + (DIAG if dr and dc else ORTH), room)
            if not done[t] and (t not in key or cand < key[t]):
                key[t] = cand
                heapq.heappush(heap, (cand[0], cand[1], t))
    room_labels = np.full(N, -1, np.int32)
    grow = np.full(N, INT_MAX, np.int32)
    for i, (g, room) in key.items():
        room_labels[i], grow[i] = sgn * room, g
    area = {l: int((room_labels == l).sum()) for l in rooms}
    ranked = sorted(rooms, key=lambda l: (-area[l], l))[:K]
    slot_of_room = {l: s for s, l in enumerate(ranked)}
    o = {"room_labels": room_labels, "grow_dist": grow, "count": np.array([len(rooms)], np.int32),
         "room": np.full(K, -1, np.int32), "area": np.zeros(K, np.int32), "core_area": np.zeros(K, np.int32),
         "bbox": np.zeros((K, 4), np.int32), "sum_rc": np.zeros((K, 2), np.uint64), "widest_key": np.zeros(K, np.uint64),
         "widest_d2": np.zeros(K, np.int32), "widest_cell": np.full(K, -1, np.int32), "room_objects": np.zeros(K, np.int32),
         "door_edges": np.zeros((K, K), np.int32), "door_key": np.zeros((K, K), np.uint64), "door_d2": np.zeros((K, K), np.int32),
         "door_cell": np.full((K, K), -1, np.int32), "obj_room_cells": np.zeros((Ko, K), np.int32),
         "obj_room": np.full(Ko, -1, np.int32), "obj_room_label": np.full(Ko, -1, np.int32), "status": np.zeros(2, np.int32)}
    wkey = lambda i: (int(d2[i]) << 32) | (~i & 0xFFFFFFFF)
    slot = slots_of(labels, objects)
    for s, l in enumerate(ranked):
        cells = np.flatnonzero(room_labels == l)
        r, c = np.divmod(cells, cols)
        o["room"][s], o["area"][s], o["core_area"][s] = l, cells.size, core_size[l]
        o["bbox"][s] = (r.min(), c.min(), r.max(), c.max())
        o["sum_rc"][s] = (r.sum(), c.sum())
        best = max(wkey(int(i)) for i in cells)
        o["widest_key"][s], o["widest_d2"][s], o["widest_cell"][s] = best, best >> 32, ~best & 0xFFFFFFFF
    door_key = {}
    for i in range(N):
        a = slot_of_room.get(int(room_labels[i]), -1)
        if a < 0:
            continue
        r, c = divmod(i, cols)
        for rr, cc in ((r - 1, c), (r, c - 1), (r, c + 1), (r + 1, c)):
            if not (0 <= rr < rows and 0 <= cc < cols):
                continue
            b = slot_of_room.get(int(room_labels[rr * cols + cc]), -1)
            if b >= 0 and b != a:
                o["door_edges"][a, b] += 1
                door_key[a, b] = max(door_key.get((a, b), 0), wkey(i))
        touch = set()
        for rr in range(max(r - 1, 0), min(r + 2, rows)):
            for cc in range(max(c - 1, 0), min(c + 2, cols)):
                if slot[rr * cols + cc] >= 0:
                    touch.add(int(slot[rr * cols + cc]))
        for k in touch:
            o["obj_room_cells"][k, a] += 1
    for (a, b), v in door_key.items():
        o["door_key"][a, b], o["door_d2"][a, b], o["door_cell"][a, b] = v, v >> 32, ~v & 0xFFFFFFFF
    for k in range(Ko):
        row = o["obj_room_cells"][k]
        if row.max(initial=0) > 0:
            s = int(np.argmax(row))                                       # the first of the largest: the lowest slot on a tie
            o["obj_room"][k], o["obj_room_label"][k] = s, ranked[s]
            o["room_objects"][s] += 1
    seeds = sum(core_size[l] for l in rooms)
    assigned = int((room_labels >= 0).sum())
    o["counts"] = np.array([blocked.sum(), void.sum(), free.sum(), seeds, assigned - seeds, free.sum() - assigned], np.int32)
    return o


def host(out):
    """The dict of `ops.map_rooms` as numpy arrays in the reference's types."""
    o = {}
    for k in KEYS:
        a = out[k].detach().cpu().numpy()
        o[k] = a.view(np.uint64) if k in WIDE else a
    return o


def differences(got, ref, keys=KEYS):
    return [k for k in keys if got[k].shape != ref[k].shape or got[k].dtype != ref[k].dtype or not np.array_equal(got[k], ref[k])]


# ---- the maps: label maps [rows * cols] int32, -1 free -----------------------------------------------------------------------------
def hand_map():
    """The 7 x 11 map of the header: (labels, cols)."""
    m = np.full((7, 11), -1, np.int32)
    m[0], m[-1], m[:, 0], m[:, -1], m[:, 5] = 0, 0, 0, 0, 0
    m[3, 5] = -1
    return m.reshape(-1), 11


def flat(rows, cols, nr, nc, door=2, seed=0, label_per_wall=False):
    """A flat of nr x nc rooms: walls one cell thick on the border and between the rooms, a door of `door` cells in every inner wall
    at a place drawn from `seed`.  One label (0) for all walls, or one per wall cell."""
    rng = np.random.default_rng(seed)
    m = np.full((rows, cols), -1, np.int32)
    m[0], m[-1], m[:, 0], m[:, -1] = 0, 0, 0, 0
    rs = [round(k * (rows - 1) / nr) for k in range(nr + 1)]
    cs = [round(k * (cols - 1) / nc) for k in range(nc + 1)]
    for r in rs[1:-1]:
        m[r] = 0
    for c in cs[1:-1]:
        m[:, c] = 0
    for a in range(nr):
        for b in range(nc):
            if b + 1 < nc and rs[a + 1] - rs[a] > door + 2:
                at = int(rng.integers(rs[a] + 1, rs[a + 1] - door))
                m[at:at + door, cs[b + 1]] = -1
            if a + 1 < nr and cs[b + 1] - cs[b] > door + 2:
                at = int(rng.integers(cs[b] + 1, cs[b + 1] - door))
                m[rs[a + 1], at:at + door] = -1
    if label_per_wall:
        m = np.where(m >= 0, np.arange(rows * cols, dtype=np.int32).reshape(rows, cols), -1).astype(np.int32)
    return m.reshape(-1)


def corridor(rows, cols, room=7):
    """A room in the top left corner and a corridor one cell wide that leaves it and winds across the whole map, row after row:
    every corridor cell has d2 1, so the grow walks its whole length, tile after tile and back."""
    m = np.zeros((rows, cols), np.int32)
    m[1:1 + room, 1:1 + room] = -1
    r, lo, hi = 1 + room // 2, room + 2, cols - 2
    m[r, 1 + room:hi + 1] = -1                                            # out of the room to the right edge
    right = True
    while r + 2 <= rows - 2:
        m[r + 1, hi if right else lo] = -1                                # one cell down at the lane's end
        r += 2
        m[r, lo:hi + 1] = -1                                              # and back along the next lane
        right = not right
    return m.reshape(-1)


def closet(rows=20, cols=24):
    """Two rooms with a door between them and, walled off inside the right one, a closet of 3 x 3 free cells whose core is one cell:
    with min_cells 2 the closet is no room and nothing reaches it."""
    m = flat(rows, cols, 1, 2, door=2, seed=3).reshape(rows, cols)
    m[3:8, cols - 7:cols - 2] = 0
    m[4:7, cols - 6:cols - 3] = -1
    return m.reshape(-1)


def diagonal_gap(rows=12, cols=16):
    """Two rooms whose only link is the diagonal step between two wall ends that touch at a corner: the corner rule refuses it."""
    m = np.full((rows, cols), -1, np.int32)
    m[0], m[-1], m[:, 0], m[:, -1] = 0, 0, 0, 0
    m[:6, 7] = 0
    m[6:, 8] = 0                                                          # (5, 7) and (6, 8) touch at a corner; (5, 8) -> (6, 7) passes between
    return m.reshape(-1)


def objects_in_rooms(rows, cols, seed=0):
    """A flat of 2 x 3 rooms with labelled blobs in them: (labels, objects) with 64 slots, a duplicate, an unused slot, a label no
    cell has and the wall's label among them."""
    rng = np.random.default_rng(seed)
    m = flat(rows, cols, 2, 3, door=2, seed=seed).reshape(rows, cols)
    labs = []
    for n in range(40):
        r, c = int(rng.integers(2, rows - 3)), int(rng.integers(2, cols - 3))
        if (m[r - 1:r + 3, c - 1:c + 3] >= 0).any():
            continue
        lab = 1000 + n
        m[r:r + 2, c:c + 1 + n % 2] = lab
        labs.append(lab)
    objects = (labs + [0, 5000])[:61]
    objects = objects[:3] + [objects[0], -1] + objects[3:]
    objects += [-1] * (64 - len(objects))
    return m.reshape(-1), objects[:64]
