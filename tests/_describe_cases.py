"""The reference of `ops.describe_pool` and `ops.describe_classify` and the inputs of their tests (numpy only).

Written from the definitions in include/eod_describe.h, not from the kernels: the slot of every cell by a plain search through
`objects`, the exact integer `sum_q` for rows whose normalisation is exact in fp32 (python integers), and float64 for everything
that carries a tolerance (pooling, embedding, softmax, top-n)."""
import numpy as np

D = 512
Q30 = 2 ** 30
U = 2.0 ** -24                                                       # the unit roundoff of fp32
INT_MAX = 2 ** 31 - 1
TINY = np.float32(1e-12)                                             # the clamp of the norm, as fp32 holds it


def slots(object_labels, objects):
    """int64 [N]: the lowest slot k with objects[k] == object_labels[i] and objects[k] >= 0, -1 for a cell in no slot."""
    labels = np.asarray(object_labels, dtype=np.int64)
    out = np.full(labels.shape, -1, np.int64)
    for k in range(len(objects) - 1, -1, -1):                        # the lowest slot is written last
        if int(objects[k]) >= 0:
            out[labels == int(objects[k])] = k
    return out


# ---- rows whose normalisation is exact in fp32 ------------------------------------------------------------------------------------
def exact_rows(N, seed):
    """(mem float32 [N, 512], q int64 [N, 512]): rows of four kinds and the q[c] the header defines for them, known without any
    floating-point arithmetic.  With a = 2^e, e in -20..20, and random signs and channels:
      kind 0: one nonzero +-a                      s = a^2, n = a, x = +-1              q = +-2^30
      kind 1: four equal +-a                       s = 4 a^2, n = 2 a, x = +-0.5         q = +-2^29
      kind 2: sixteen equal +-a                    s = 16 a^2, n = 4 a, x = +-0.25       q = +-2^28
      kind 3: one +-a and one +-1.5 * 2^-31 a      s = a^2 (1 + 2.25 * 2^-62) rounds to a^2 in any order, with or without fused
              multiply-adds; n = a; x = +-1 and +-0.75 * 2^-30: the product with 2^30 is +-0.75 and truncates to 0 (rounding to
              nearest would give +-1, rounding down -1 for the negative sign)
    Every partial sum of squares is a power of two times 1, 2, 3, ... 16 (kinds 0 to 2): exact in fp32 in any order."""
    rng = np.random.default_rng(seed)
    mem = np.zeros((N, D), np.float32)
    q = np.zeros((N, D), np.int64)
    kind = rng.integers(0, 4, N)
    for i in range(N):
        a = np.float32(2.0) ** np.float32(int(rng.integers(-20, 21)))
        n = (1, 4, 16, 2)[kind[i]]
        ch = rng.choice(D, n, replace=False)
        sign = rng.choice(np.array([-1.0, 1.0], np.float32), n)
        if kind[i] < 3:
            mem[i, ch] = sign * a
            q[i, ch] = sign.astype(np.int64) * (Q30 >> kind[i])
        else:
            mem[i, ch[0]] = sign[0] * a
            mem[i, ch[1]] = sign[1] * np.float32(1.5) * np.float32(2.0 ** -31) * a
            q[i, ch[0]] = int(sign[0]) * Q30
            q[i, ch[1]] = 0
    assert np.isfinite(mem).all() and (mem != 0).sum() == sum((1, 4, 16, 2)[k] for k in kind)
    return mem, q


def exact_pool(q, object_labels, objects):
    """(sum_q int64 [K, 512], cells int32 [K]) from the per-cell q of `exact_rows`: integer sums."""
    s = slots(object_labels, objects)
    K = len(objects)
    sum_q = np.zeros((K, D), np.int64)
    cells = np.zeros(K, np.int32)
    for k in range(K):
        mine = s == k
        cells[k] = int(mine.sum())
        sum_q[k] = q[mine].sum(axis=0)
    return sum_q, cells


# ---- float64 ---------------------------------------------------------------------------------------------------------------------
def unit_rows64(mem):
    """float64 [N, 512]: x as the header defines it, evaluated in float64 on the fp32 inputs; a row with an Inf or a NaN gives zeros."""
    m = np.asarray(mem, dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        n = np.sqrt((m * m).sum(axis=1, keepdims=True))
        n = np.where(n < float(TINY), float(TINY), n)                 # a NaN stays a NaN
        x = m / n
    x = np.where(np.isfinite(x), x, 0.0)
    return np.clip(x, -1.0, 1.0)


def pool64(mem, object_labels, objects):
    """(sum float64 [K, 512] of the unit rows, abs float64 [K, 512]: the sum of their magnitudes, cells int32 [K])."""
    s = slots(object_labels, objects)
    x = unit_rows64(mem)
    K = len(objects)
    tot, mag, cells = np.zeros((K, D)), np.zeros((K, D)), np.zeros(K, np.int32)
    for k in range(K):
        mine = s == k
        cells[k] = int(mine.sum())
        tot[k] = x[mine].sum(axis=0)
        mag[k] = np.abs(x[mine]).sum(axis=0)
    return tot, mag, cells


def finish64(sum_q, cells):
    """(embedding float64 [K, 512], coherence float64 [K]) from integer sums, as the header defines them."""
    sum_q = np.asarray(sum_q, dtype=np.int64)
    K = sum_q.shape[0]
    emb, coh = np.zeros((K, D)), np.zeros(K)
    for k in range(K):
        if int(cells[k]) <= 0:
            continue
        mean = sum_q[k].astype(np.float64) / (float(int(cells[k])) * float(Q30))
        norm = float(np.sqrt((mean * mean).sum()))
        if norm > 0.0:
            emb[k], coh[k] = mean / norm, norm
    return emb, coh


def classify64(embedding, zs):
    """(L float64 [K, C] the logits, B float64 [K, C] the bound of an fp32 logit's error, p float64 [K, C] the softmax; rows of an
    all-zero embedding hold zeros in p).  B: a 512-term fp32 dot product, in any order and with or without fused multiply-adds, is
    off by at most gamma_512 * sum |e| |z| <= 513 U sum |e| |z|; the product with 50 adds one rounding of the result."""
    e, z = np.asarray(embedding, np.float64), np.asarray(zs, np.float64)[:, :-1]
    dot = e @ z
    L = 50.0 * dot
    B = 50.0 * U * (514.0 * (np.abs(e) @ np.abs(z)) + 2.0 * np.abs(dot))
    m = L.max(axis=1, keepdims=True)
    ex = np.exp(L - m)
    p = ex / ex.sum(axis=1, keepdims=True)
    p[~np.asarray(embedding).any(axis=1)] = 0.0
    return L, B, p


def topn(prob, n):
    """(top_cls int32 [K, n], top_prob [K, n] in prob's type): by (prob descending, class ascending); an all-zero row of an empty
    slot is NOT treated here (the caller knows which rows are empty)."""
    prob = np.asarray(prob)
    K, C = prob.shape
    cls = np.zeros((K, n), np.int32)
    val = np.zeros((K, n), prob.dtype)
    for k in range(K):
        order = np.lexsort((np.arange(C), -prob[k].astype(np.float64)))
        cls[k] = order[:n]
        val[k] = prob[k, order[:n]]
    return cls, val


# ---- label maps -------------------------------------------------------------------------------------------------------------------
def label_cases(rows, cols, hostile):
    """{name: (object_labels int32 [N], objects int32 [K])}: the label maps of the exact test on one grid.  `hostile`: the maps of
    `_inventory_cases.hostile_maps` for this grid; their class labels serve as object labels (many short runs, labels that are in
    no slot, INT_MAX and negative values)."""
    N = rows * cols
    rng = np.random.default_rng(7)
    r, c = np.mgrid[0:rows, 0:cols]
    r, c = r.reshape(-1).astype(np.int32), c.reshape(-1).astype(np.int32)
    i32 = lambda v: np.asarray(v, dtype=np.int32)
    pad = lambda v, K: i32(list(v) + [-1] * (K - len(v)))
    cases = {}
    for name, (lab, _, _) in hostile.items():
        cases[f"hostile: {name}"] = (lab, i32([0, 1, 2, 3, 4]))
    cases["one object owns every cell"] = (np.full(N, 9, np.int32), i32([9]))
    cases["one object owns every cell, K 64"] = (np.full(N, 9, np.int32), pad([-1, -1, 9], 64))
    cases["single-cell objects"] = (np.arange(N, dtype=np.int32), i32(rng.permutation(N)[:min(64, N)]))
    cases["alternating along the row"] = (i32(10 + (r + c) % 2), i32([11, 10]))            # a flush on every cell
    cases["alternating three"] = (i32((r * cols + c) % 3), i32([2, 0, 1, 0, 2]))
    cases["labels not asked for"] = (i32(rng.integers(0, 12, N)), i32([3, 7, 11, 40, 5]))
    lab = i32(rng.integers(0, 6, N))
    kind = rng.integers(0, 8, N)
    lab[kind == 0], lab[kind == 1], lab[kind == 2] = -1, INT_MAX, -7
    cases["-1, INT_MAX and negative labels"] = (lab, i32([INT_MAX, 0, 5, -7, 2]))          # INT_MAX is a label like any other; -7 is none
    cases["a duplicate in objects"] = (i32(rng.integers(0, 4, N)), i32([2, 1, 2, 0, 1]))
    cases["-1 slots in the middle"] = (i32(rng.integers(0, 5, N)), i32([4, -1, -1, 0, -1, 3] + [-1] * 20 + [1]))
    cases["K 1"] = (i32(rng.integers(0, 3, N)), i32([1]))
    cases["K 64"] = (i32(rng.integers(0, 80, N)), i32(rng.permutation(80)[:64]))
    cases["K 64, blocks"] = (i32(r // 3 * 100 + c // 4), i32(np.unique(r // 3 * 100 + c // 4)[:64]))
    cases["nothing asked for is there"] = (i32(rng.integers(0, 5, N)), i32([7, 8, -1]))
    for lab, objects in cases.values():
        assert lab.dtype == np.int32 and lab.shape == (N,) and objects.dtype == np.int32 and 1 <= len(objects) <= 64
    return cases
