"""CPU side of test_memory_write_edges_gpu.py: the scenes, a float64 restatement of the memory write (custom_rcnn.py:681-760,875-936
as the header of csrc/memory.hip states it) and the facts about a scene that decide which paths of the three write kernels it
runs.  Nothing here touches a GPU.

The scenes have NO THRESHOLD BAND.  The write samples every 8th observed pixel in row-major order, so one mask decision taken
differently re-phases every later sample: no pixel can be left out of the comparison.  Box widths and heights are powers of two
(8 .. 64), box corners multiples of 1/8, mask values multiples of 1/16 and the threshold 0.5: every intermediate of the kernel's
`row_sample` / `mask_hit_row` is then a dyadic number of few bits, exact in fp32 whether or not multiply-adds are fused, and the
decision `v >= 0.5` is the float64 one -- including the samples exactly at 0.5.  `paste_values` is that arithmetic at a chosen
precision; test_fp32_sampler_is_float64_on_every_scene asserts the equality for every scene built here."""
import functools
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from _launch_cases import SENTINEL, U    # noqa: F401  (re-exported)

HEAD = 2.0               # head-room of the value bound, as ROI_HEAD and the head modules' HEAD
SCAN_ELEMS = 1024        # pixels per workgroup of the cover and scatter passes
MW_AGG = 512             # slots of the scatter pass's LDS aggregation table
R_CAP = 512
THRESH = 0.5


# ------------------------------------------------------------------------------------------------
# the mask sampler at a chosen precision
# ------------------------------------------------------------------------------------------------
def paste_values(masks: np.ndarray, boxes: np.ndarray, H: int, W: int, dtype) -> Tuple[np.ndarray, np.ndarray]:
    """masks [K,28,28], boxes [K,4] -> (v [K,H,W], inside [K,H,W]): the bilinear sample of every instance's 28x28 mask at every pixel
    centre, step for step and in the order of `row_sample` / `mask_hit_row` (csrc/memory.hip), every step rounded to `dtype`;
    `inside`: the sample point lies in (-1, 28) on both axes (outside it the instance does not cover the pixel whatever `v`)."""
    t = dtype
    m, b = masks.astype(t), boxes.astype(t)
    K = m.shape[0]
    half, one, two, n28 = t(0.5), t(1.0), t(2.0), t(28.0)

    def axis(lo, hi, n):
        g = (np.arange(n, dtype=t)[None, :] + half - lo[:, None]) / (hi - lo)[:, None] * two - one
        i = ((g + one) * n28 - one) / two
        inside = (i > -one) & (i < n28)
        lo_i = np.floor(i).astype(np.int64)
        hi_i = lo_i + 1
        return inside, lo_i, hi_i, hi_i.astype(t) - i, i - lo_i.astype(t)

    iny, yn, ys, wyn, wys = axis(b[:, 1], b[:, 3], H)
    inx, xw, xe, wxw, wxe = axis(b[:, 0], b[:, 2], W)
    kk = np.arange(K)[:, None, None]

    def tap(yi, xi):
        yi, xi = np.broadcast_to(yi[:, :, None], (K, H, W)), np.broadcast_to(xi[:, None, :], (K, H, W))
        valid = (yi >= 0) & (yi < 28) & (xi >= 0) & (xi < 28)
        return np.where(valid, m[kk, np.clip(yi, 0, 27), np.clip(xi, 0, 27)], t(0.0))

    v = np.zeros((K, H, W), dtype=t)
    v = v + tap(yn, xw) * (wxw[:, None, :] * wyn[:, :, None])
    v = v + tap(yn, xe) * (wxe[:, None, :] * wyn[:, :, None])
    v = v + tap(ys, xw) * (wxw[:, None, :] * wys[:, :, None])
    v = v + tap(ys, xe) * (wxe[:, None, :] * wys[:, :, None])
    assert v.dtype == t
    return v, iny[:, :, None] & inx[:, None, :]


def mask_rows_of(box: np.ndarray, y_lo: int, y_hi: int) -> List[int]:
    """The mask rows the image rows y_lo .. y_hi - 1 sample in an instance with this box."""
    y = np.arange(y_lo, y_hi, dtype=np.float64)
    iy = (((y + 0.5 - box[1]) / (box[3] - box[1]) * 2 - 1) + 1) * 14 - 0.5
    lo = np.floor(iy).astype(np.int64)
    return sorted({int(r) for r in np.concatenate([lo, lo + 1]) if 0 <= r < 28})


# ------------------------------------------------------------------------------------------------
# scenes
# ------------------------------------------------------------------------------------------------
class Scene:
    """R_CAP proposal rows of which `inst` (128 of them, rows 0 and 511 among them) hold the scene's instances; every other row holds
    a whole-image box with a mask of ones and huge features: read by mistake, it covers every pixel and shows."""

    def __init__(self, name: str, H: int, W: int, seed: int, sizes: Sequence[int], y0_range: Tuple[int, int],
                 blank_rows: Optional[Tuple[int, int]] = None, special: Optional[Tuple[float, float]] = None, density: float = 1.0):
        rng = np.random.RandomState(seed)
        self.name, self.H, self.W, self.blank_rows = name, H, W, blank_rows
        n = 128
        rest = rng.permutation(np.arange(1, R_CAP - 1))[:n - 2]
        self.inst = rng.permutation(np.concatenate([[0, R_CAP - 1], rest]))          # instance i lives in proposal row inst[i]
        bw, bh = rng.choice(sizes, n).astype(np.float64), rng.choice(sizes, n).astype(np.float64)
        x0 = rng.randint((-bw / 2 * 8).astype(np.int64), ((W - bw / 2) * 8).astype(np.int64)) / 8.0
        y0 = rng.randint(y0_range[0] * 8, y0_range[1] * 8, n) / 8.0
        boxes = np.stack([x0, y0, x0 + bw, y0 + bh], axis=1)
        masks = rng.randint(0, 17, (n, 28, 28)) / 16.0
        if density < 1.0:                         # sparse masks: not every pixel under a box is observed
            masks = masks * (rng.rand(n, 28, 28) < density)
        if blank_rows is not None:                # no instance covers a pixel of these image rows ...
            for i in range(n):
                masks[i, mask_rows_of(boxes[i], *blank_rows)] = 0.0
        self.special = None
        if special is not None:                   # ... but the last one: an 8 x 8 box whose mask is one short bar (see `set_bar`)
            boxes[n - 1] = [special[0], special[1], special[0] + 8.0, special[1] + 8.0]
            masks[n - 1] = 0.0
            self.special = n - 1
        self.boxes = np.tile(np.array([0.0, 0.0, W, H]), (R_CAP, 1))
        self.masks = np.ones((R_CAP, 28, 28))
        self.boxes[self.inst], self.masks[self.inst] = boxes, masks
        g = torch.Generator().manual_seed(seed)
        self.featn = torch.full((R_CAP, 512), 1.0e4)
        f = torch.randn((n, 512), generator=g)
        self.featn[torch.from_numpy(self.inst)] = 50.0 * f / f.norm(dim=1, keepdim=True)

    def set_bar(self, pixels: int) -> None:
        """The special instance covers exactly `pixels` (1 .. 7) pixels of ONE image row: image column c of its 8 x 8 box samples the
        mask at 3.5 c + 1.25, image row 2 at 8.25 -- between mask rows 8 and 9, which hold ones under the first `pixels` columns'
        two taps each and zeros elsewhere."""
        assert self.special is not None and 1 <= pixels <= 7
        m = np.zeros((28, 28))
        for c in range(pixels):
            x = int(np.floor(3.5 * c + 1.25))
            m[8:10, x:x + 2] = 1.0
        self.masks[self.inst[self.special]] = m

    def det_list(self, unique: int, K_cap: int, style: str, seed: int = 0) -> Tuple[np.ndarray, int]:
        """-> (det_rows [K_cap], det_count) naming exactly the first `unique` instances (proposal rows 0 and 511 are instances 0 / 1
        of that order when unique >= 2; the special instance is the third).
          'plain'    the rows once each, shuffled; det_count = unique (entries behind it name other rows and must not be read)
          'hostile'  duplicates, -1 and 512 (both ignored) shuffled among them; det_count = all the list holds
          'over'     as hostile, filling the list; det_count = 1000, clamped to K_cap"""
        rows = [int(self.inst[i]) for i in self.order[:unique]]
        others = [r for r in range(R_CAP) if r not in set(rows)]
        rng = np.random.RandomState(1000 + seed + unique)
        if style == "plain":
            lst, count = [int(r) for r in rng.permutation(rows)], unique
        else:
            pool = [-1, R_CAP] + [rows[j % unique] for j in range(K_cap)]          # the two ignored entries, then duplicates
            n_extra = K_cap - unique if style == "over" else min(K_cap - unique, 2 + unique // 3)
            lst = [int(r) for r in rng.permutation(rows + pool[:n_extra])]
            count = 1000 if style == "over" else len(lst)
        assert len(lst) <= K_cap and (style != "over" or len(lst) == K_cap)
        lst = lst + [int(r) for r in rng.choice(others, K_cap - len(lst))]
        return np.asarray(lst, dtype=np.int64), int(count)

    @property
    def order(self) -> np.ndarray:
        """Instances in the order `det_list` takes them: those in proposal rows 0 and 511, the special one, then the rest."""
        first = [int(np.nonzero(self.inst == 0)[0][0]), int(np.nonzero(self.inst == R_CAP - 1)[0][0])]
        if self.special is not None:
            first.append(self.special)
        return np.asarray(first + [i for i in range(128) if i not in first])


def unique_rows(det_rows: np.ndarray, det_count: int, K_cap: int) -> List[int]:
    k = max(0, min(int(det_count), K_cap))
    return sorted({int(r) for r in det_rows[:k] if 0 <= int(r) < R_CAP})


@functools.lru_cache(maxsize=None)
def scene(name: str) -> Scene:
    """The module's scenes.  'dense' / 'dense2': 64 x 96 (six whole blocks of 1024 pixels, W does not divide 1024), boxes 32 or 64 tall
    starting at rows -24 .. 24, image rows 10 .. 31 blank: block 1 (pixels 1024 .. 2047: row 10 column 64 to row 21 column 31) has
    no observed pixel, block 2 (to the end of row 31) only the special instance's bar.  'tail': 40 x 72, 2880 pixels, a tail block
    of 832.  'partial': 28 x 36, 1008 pixels, one partial block."""
    if name in ("dense", "dense2"):
        s = Scene(name, 64, 96, 1 if name == "dense" else 6, (32, 64), (-24, 24), blank_rows=(10, 32), special=(40.0, 23.0))
        # the bar's length is chosen from the reference alone: the observed pixels before block 2 leave rank r (mod 8) for its first
        # one; r = 0 would sample it whatever the length, else 8 - r pixels stay unsampled
        s.set_bar(1)
        f = scene_facts(s, [int(s.inst[i]) for i in s.order])
        r = int(f["first_rank"][2]) % 8
        assert r != 0, "choose another seed: the bar's first pixel has a rank that is a multiple of 8"
        s.set_bar(min(7, 8 - r))
        return s
    if name == "tail":
        return Scene(name, 40, 72, 7, (16, 32), (-12, 28), density=0.5)
    if name == "partial":
        return Scene(name, 28, 36, 8, (8, 16, 32), (-8, 20), density=0.4)
    raise KeyError(name)


SCENES = ("dense", "dense2", "tail", "partial")


# ------------------------------------------------------------------------------------------------
# index images
# ------------------------------------------------------------------------------------------------
def proj_image(pattern: str, H: int, W: int, seed: int = 0) -> Tuple[np.ndarray, int]:
    """-> (proj int64 [H,W], n_cells).
      'pixel'   one cell per pixel, scattered over N = P + 37 cells (no multiple of 64)
      'one'     every pixel in cell 4 of 5
      'blocky'  8 x 8 pixel blocks, cells 0 and N - 1 among them, N = 301"""
    rng = np.random.RandomState(50 + seed)
    P = H * W
    if pattern == "pixel":
        return rng.permutation(P + 37)[:P].reshape(H, W).astype(np.int64), P + 37
    if pattern == "one":
        return np.full((H, W), 4, dtype=np.int64), 5
    if pattern == "blocky":
        N = 301
        hb, wb = (H + 7) // 8, (W + 7) // 8
        cells = rng.randint(0, N, (hb, wb))
        cells[0, 0], cells[-1, -1], cells[hb // 2, wb // 2] = N - 1, 0, 0
        return np.repeat(np.repeat(cells, 8, 0), 8, 1)[:H, :W].astype(np.int64).copy(), N
    raise KeyError(pattern)


# ------------------------------------------------------------------------------------------------
# the write in float64
# ------------------------------------------------------------------------------------------------
def hits_of(sc: Scene, rows: Sequence[int], thresh: float = THRESH) -> np.ndarray:
    """bool [K, P]: instance k (proposal row rows[k]) covers pixel p."""
    v, inside = paste_values(sc.masks[list(rows)], sc.boxes[list(rows)], sc.H, sc.W, np.float64)
    return (inside & (v >= thresh)).reshape(len(rows), -1)


def write_reference(sc: Scene, det_rows: np.ndarray, det_count: int, K_cap: int, proj: np.ndarray, n_cells: int, mem0: torch.Tensor,
                    obs0: torch.Tensor, thresh: float = THRESH) -> Dict:
    """unique(det_rows[:min(count, K_cap)]) ascending, rows outside [0, R_CAP) ignored; a pixel is observed when an instance's pasted
    mask is >= thresh at its centre; every 8th observed pixel (row-major) is sampled and contributes the mean of its covering
    instances' features; a cell takes the mean over its sampled pixels, mem[cell] += mean; obs[cell] += 1 for every cell `proj`
    names; no instance: nothing changes.  `proj` must be in range (the caller clamps by hand)."""
    N = n_cells
    rows = unique_rows(det_rows, det_count, K_cap)
    K = len(rows)
    out = dict(k=K, rows=rows, mem=mem0.double().clone(), obs=obs0.clone(), dirty=torch.zeros(N, dtype=torch.bool),
               written=torch.zeros(N, dtype=torch.bool), bound=torch.zeros((N, 512), dtype=torch.float64), cover_max=0)
    if K == 0:
        return out
    cell = proj.reshape(-1)
    assert cell.min() >= 0 and cell.max() < N
    hits = hits_of(sc, rows, thresh)
    cover = hits.sum(0)
    observed = np.nonzero(cover > 0)[0]
    samp = observed[::8]
    wt = np.zeros((N, K))
    kk, pp = np.nonzero(hits[:, samp])
    np.add.at(wt, (cell[samp][pp], kk), 1.0 / cover[samp][pp])
    cnt = np.bincount(cell[samp], minlength=N)
    written = cnt > 0
    f = sc.featn[rows].double().numpy()
    mean = np.zeros((N, 512))
    mean[written] = (wt[written] @ f) / cnt[written, None]
    flag = np.zeros(N, dtype=bool)
    flag[cell] = True
    mean_t = torch.from_numpy(mean)
    out["mem"] = mem0.double() + mean_t
    out["obs"] = obs0 + torch.from_numpy(flag).to(obs0.dtype)
    out["dirty"], out["written"] = torch.from_numpy(flag), torch.from_numpy(written)
    cover_max = int(cover[samp].max()) if samp.size else 0
    # the two fp32 roundings of the commit ((float)mean, then mem + that) and the 2^-32 fixed-point shares: a share is off by at most
    # 2^-33, a cell's n sampled pixels hold at most n * cover_max of them, and the sum is divided by n
    bound = HEAD * (U * (mean_t.abs() + out["mem"].abs()) + cover_max * 2.0 ** -33 * float(np.abs(f).max()))
    out["bound"] = torch.where(out["written"][:, None], bound, torch.zeros_like(bound))
    out.update(cover_max=cover_max, hits=hits, cover=cover, samp=samp, wt=wt, cnt=cnt)
    return out


# ------------------------------------------------------------------------------------------------
# which paths of the kernels a scene runs
# ------------------------------------------------------------------------------------------------
def scene_facts(sc: Scene, rows: Sequence[int]) -> Dict:
    """Per 1024-pixel block, from the reference alone: `n_cand` band candidates (instances whose box, grown by (y1 - y0) / 14,
    reaches the block's image rows), `observed` pixels, `first_rank` (observed pixels before the block), `sampled` pixels,
    `high_hit` (a sampled pixel is covered by a candidate at position >= 64 of the block's list), `keys` (with one cell per pixel:
    distinct (cell, instance) entries plus cell entries the block adds to the LDS table)."""
    rows = sorted(rows)
    H, W, P = sc.H, sc.W, sc.H * sc.W
    hits = hits_of(sc, rows)
    cover = hits.sum(0)
    obs = cover > 0
    rank = np.cumsum(obs) - obs                                   # observed pixels before p
    b = sc.boxes[rows]
    my = (b[:, 3] - b[:, 1]) / 14.0
    nb = (P + SCAN_ELEMS - 1) // SCAN_ELEMS
    f = dict(n_cand=[], observed=[], first_rank=[], sampled=[], high_hit=[], keys=[], blocks=nb, cover_max=0)
    for blk in range(nb):
        p0, p1 = blk * SCAN_ELEMS, min(P, (blk + 1) * SCAN_ELEMS) - 1
        ylo, yhi = p0 // W + 0.5, p1 // W + 0.5
        cand = np.nonzero(~((yhi < b[:, 1] - my) | (ylo > b[:, 3] + my)))[0]
        sl = slice(p0, p1 + 1)
        samp = p0 + np.nonzero(obs[sl] & (rank[sl] % 8 == 0))[0]
        f["n_cand"].append(int(cand.size))
        f["observed"].append(int(obs[sl].sum()))
        f["first_rank"].append(int(rank[p0]))
        f["sampled"].append(int(samp.size))
        f["high_hit"].append(bool(hits[cand[64:]][:, samp].any()) if cand.size > 64 else False)
        f["keys"].append(int(samp.size + hits[:, samp].sum()))
        assert not hits[np.setdiff1d(np.arange(len(rows)), cand)][:, sl].any(), "an instance outside the band covers a pixel"
        if samp.size:
            f["cover_max"] = max(f["cover_max"], int(cover[samp].max()))
    return f
