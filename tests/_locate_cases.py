"""References for the locate query (EOD_SEMMAP_LOCATE / EOD_SEMMAP_PEAKS, `ops.semmap_locate`): the peak definition, exact, on any
probability map; the float64 bound on a queried class's probability; memories whose rows are aimed at chosen classes.

Peak: cell i = r * cols + c of class q is a peak iff prob[q, i] > 0 and no other cell j of the (2 radius + 1)^2 window around it,
clipped at the grid's edge, has prob[q, j] > prob[q, i], or prob[q, j] == prob[q, i] and j < i.  The K best peaks by
(prob descending, cell ascending) are returned, padded with (-1, 0.0).  Comparisons only, so the reference is exact on the bits it
is given.
"""
import numpy as np
import torch


def peak_flags(p: np.ndarray, cols: int, radius: int) -> np.ndarray:
    """bool [N]: which cells of the map `p` [N] are peaks."""
    p = np.asarray(p)
    n = p.shape[0]
    assert n % cols == 0 and 0 <= radius
    rows = n // cols
    grid = p.reshape(rows, cols)
    pad = np.full((rows + 2 * radius, cols + 2 * radius), -1.0, dtype=grid.dtype)     # never above or equal to a positive value
    pad[radius:radius + rows, radius:radius + cols] = grid
    peak = grid > 0
    for dr in range(-radius, radius + 1):
        for dc in range(-radius, radius + 1):
            if dr == 0 and dc == 0:
                continue
            nb = pad[radius + dr:radius + dr + rows, radius + dc:radius + dc + cols]
            lower = dr < 0 or (dr == 0 and dc < 0)                                     # j < i
            peak &= ~((nb > grid) | ((nb == grid) & lower))
    return peak.reshape(n)


def peaks_reference(prob: np.ndarray, cols, radius: int, K: int):
    """prob [Q, N] -> (peaks int32 [Q, K], peak_scores [Q, K] of prob's dtype).  `cols=None`: the plain top-K of the positive cells."""
    prob = np.asarray(prob)
    Q, n = prob.shape
    if cols is None:
        cols, radius = n, 0
    peaks = np.full((Q, K), -1, dtype=np.int32)
    scores = np.zeros((Q, K), dtype=prob.dtype)
    for q in range(Q):
        cells = np.nonzero(peak_flags(prob[q], cols, radius))[0]
        order = cells[np.lexsort((cells, -prob[q, cells]))][:K]                        # last key first: prob descending, then cell
        peaks[q, :len(order)] = order
        scores[q, :len(order)] = prob[q, order]
    return peaks, scores


def prob_bound(L: torch.Tensor, B_row: torch.Tensor, p64: torch.Tensor, classes) -> torch.Tensor:
    """[Q, N] float64: the admitted |prob - p64| of the queried classes.  As the score bound of test_semmap_query_gpu.py, with the
    queried logit's own error (2 B_row more) and the second exponential (its argument scaling and rounding once more):
    p64 (4 B_row + 2 (spread + 4) 2^-23 + C 2^-24) + 2^-126, the floor because exp(-100) is subnormal in fp32."""
    C = L.shape[1]
    spread = (L - L.max(dim=1, keepdim=True).values).abs().max(dim=1).values
    rel = 4.0 * B_row + 2.0 * (spread + 4.0) * 2.0 ** -23 + C * 2.0 ** -24
    return p64[:, list(classes)].t() * rel[None, :] + 2.0 ** -126


def query_classes(L: torch.Tensor, seed: int):
    """The classes test 1 asks for: the three most frequent float64 argmax classes, column 0, the last column, three random ones."""
    C = L.shape[1]
    freq = torch.bincount(L.argmax(dim=1), minlength=C).topk(min(3, C)).indices.tolist()
    g = torch.Generator().manual_seed(seed)
    return freq + [0, C - 1] + torch.randint(0, C, (3,), generator=g).tolist()


def aimed_rows(zs: torch.Tensor, n: int, classes, seed: int = 0):
    """mem [n, 512], obs [n]: every row a text column of `classes` (in turn) + 10 % noise, x 50, x an observation count: rows whose
    probability of a class nobody aimed at is far below a never-written row's 1 / C."""
    g = torch.Generator().manual_seed(seed)
    aim = torch.tensor([classes[i % len(classes)] for i in range(n)])
    noise = torch.randn((n, 512), generator=g) / 512 ** 0.5
    count = torch.randint(1, 41, (n, 1), generator=g).float()
    mem = ((zs[:, aim].t() + 0.1 * noise) * 50.0 * count).float().contiguous()
    return mem, torch.ones((n,))
