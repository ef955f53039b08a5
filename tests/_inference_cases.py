"""CPU side of test_inference_launches_gpu.py: the production configurations whose frames are recorded, the families a recording
must hold, the hostile inputs of the replays and the references written out in torch / numpy.  Nothing here touches a GPU."""
import math
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from _launch_cases import U

# configuration -> (H, W, memory grid, cell size, scenes, config overrides, LVIS heads)
CONFIGS = {
    "640x640": (640, 640, 200, 0.2, 1, [], False),
    "480x640": (480, 640, 200, 0.2, 1, [], False),
    "640x640 lock-step 2": (640, 640, 200, 0.2, 2, [], False),
    "640x640 lock-step 4": (640, 640, 200, 0.2, 4, [], False),
    "960x960 config 5": (960, 960, 512, 0.08, 1, [], False),
    "960x960 config 5 lock-step 4": (960, 960, 512, 0.08, 4, [], False),
    "640x640 mem_only": (640, 640, 200, 0.2, 1, ["MODEL.MAP_FEAT_FUSION", "mem_only"], False),
    "640x640 LVIS": (640, 640, 200, 0.2, 1, [], True),
}
# what every recorded episode (an empty-memory frame, then recurrent frames) must contain
FRAME_FAMILIES = ("preprocess_image", "maxpool3x3s2", "groupnorm_relu", "proposals", "roi_align", "detection_selector",
                  "detector_postprocess", "paste_masks", "unproject_grid_index", "memory_gather_pool",
                  "memory_projector", "memory_writer")
# the box head's classifier: fused with the stage's last layer (cascade_stage_tail) or alone (zs_classify), one of the two per stage
CLASSIFIER_FAMILIES = ("zs_classify", "cascade_stage_tail")
LOCKSTEP_FAMILIES = ("concat_lists",)
# (the frame's mask predictor rides on the deconvolution's epilogue: `mask_predictor_sigmoid` is wrapped but no frame calls it)
OPTIONAL_FAMILIES = ("mask_predictor_sigmoid", "apply_deltas", "memory_scores", "memory_normalize_f16", "memory_normalize_dirty_f16", "semmap_labels")
ALL_FAMILIES = FRAME_FAMILIES + CLASSIFIER_FAMILIES + LOCKSTEP_FAMILIES + OPTIONAL_FAMILIES

STRIDES = (8, 16, 32, 64, 128)


def pyramid_hw(H: int, W: int) -> List[Tuple[int, int]]:
    return [(-(-H // s), -(-W // s)) for s in STRIDES]


# ------------------------------------------------------------------------------------------------
# proposal decode: heat maps built to hurt the histogram cut, the sorts and the tie rules
# ------------------------------------------------------------------------------------------------
OFF = -12.0            # sigmoid(-12) = 6e-6 < INFERENCE_TH = 1e-4: not a candidate
SEP_LO, SEP_HI = -6.0, 6.0


def separated_logits(n: int, g: torch.Generator) -> torch.Tensor:
    """n DISTINCT logits whose sigmoids differ by >= 1e-6 (>= 16 ulp at 1.0, thousands of ulp further down): every order decision on
    them is the same whichever correctly-behaved expf took it, so the CPU's sigmoid can take the reference's decisions."""
    J = 12000                                                   # step 1e-3 in the logit: >= 2.5e-6 in the sigmoid at |x| = 6
    assert n <= J
    pick = torch.randperm(J, generator=g)[:n]
    return (SEP_HI - pick.double() * ((SEP_HI - SEP_LO) / (J - 1))).float()


def robust_sigmoids(lo: float = 3.0, hi: float = 9.0, step: float = 1e-4) -> Tuple[np.ndarray, np.ndarray]:
    """(logits, heats): fp32 logits whose fp32 sigmoid 1 / (1 + expf(-x)) is the same BIT PATTERN for every expf within 4 ulp of the
    true exponential: 1 + e rounds to the same fp32 number over that whole interval, and the IEEE division of 1 by it has one
    result.  Sorted by heat, heats distinct.  These let a test put two scores a chosen number of ulp apart.  (Read back from the
    level top-k kernel through a build that emits the heat instead of its root: all 42 384 agree with the device bit for bit.)"""
    x = np.arange(lo, hi, step).astype(np.float32)
    e = np.exp(-x.astype(np.float64))
    t_lo = (1.0 + e * (1 - 2.0 ** -21)).astype(np.float32)
    t_hi = (1.0 + e * (1 + 2.0 ** -21)).astype(np.float32)
    ok = t_lo == t_hi
    x, t = x[ok], t_lo[ok]
    heat = (np.float32(1.0) / t).astype(np.float32)
    heat, first = np.unique(heat, return_index=True)
    return x[first], heat


def bin_of(heat: np.ndarray) -> np.ndarray:
    """The 4096-bin histogram of the level top-k: 2^14-wide ranges of the fp32 bit pattern from 2^-7 up, everything below in bin 0."""
    return np.clip((heat.astype(np.float32).view(np.uint32) >> 14).astype(np.int64) - (0x3C000000 >> 14), 0, 4095)


HEAT_CASES = ("seeded", "equal", "two values", "bin 0", "one bin", "cut tie", "cut edge above", "cut edge below", "saturated", "empty level",
              "exactly topk", "topk + 1", "few fine many coarse", "post-nms ties")


def hostile_heat(case: str, sizes: Sequence[int], topk: int, post: int, seed: int) -> Tuple[List[torch.Tensor], Optional[List[torch.Tensor]], str]:
    """-> (logits per level, exact heats per level or None, box regime).  Box regimes: "tiny" (NMS removes nothing), "stacked" (NMS at
    0.9 removes nearly everything), "seeded"."""
    g = torch.Generator().manual_seed(seed)
    L = len(sizes)

    def sep(n):
        return separated_logits(n, g)

    def scatter(n, vals):
        """`vals` at seeded distinct positions of a level of n, OFF elsewhere."""
        out = torch.full((n,), OFF)
        out[torch.randperm(n, generator=g)[:vals.numel()]] = vals
        return out

    heats = None
    regime = "seeded"
    if case == "seeded":
        lv = [sep(n) if n <= 12000 else torch.cat([sep(12000), torch.full((n - 12000,), OFF)])[torch.randperm(n, generator=g)] for n in sizes]
    elif case == "equal":
        lv, regime = [torch.zeros(n) for n in sizes], "stacked"
    elif case == "two values":
        lv = [torch.where(torch.rand(n, generator=g) < 0.1, torch.tensor(2.0), torch.tensor(-2.0)) for n in sizes]
    elif case == "bin 0":
        # 1e-4 < sigmoid(-8 .. -5) = 3.4e-4 .. 6.7e-3 < 2^-7: the whole level is one bin, the compacted list is the whole level
        lv, regime = [torch.tensor([-5.0, -6.0, -7.0, -8.0])[torch.randint(0, 4, (n,), generator=g)] for n in sizes], "tiny"
    elif case == "one bin":
        # sigmoid(0 .. 0.003) = 0.5 .. 0.50075 < 0.5 + 2^-10: one bin above bin 0, four values a thousand ulp apart
        lv, regime = [torch.tensor([0.0, 0.001, 0.002, 0.003])[torch.randint(0, 4, (n,), generator=g)] for n in sizes], "tiny"
    elif case == "cut tie":
        lv = []
        for n in sizes:
            if n > topk + 8:
                v = sep(topk + 3).sort(descending=True).values
                v[topk - 2:topk + 3] = v[topk - 2]                 # ranks topk-1 .. topk+3 equal: the lower positions win
                lv.append(scatter(n, v))
            else:
                lv.append(sep(n))
    elif case in ("cut edge above", "cut edge below"):
        # the topk-th and the (topk+1)-th score are neighbours among the robust sigmoids on the two sides of a 2^14 boundary of the
        # bit pattern ("above": the cut bin starts at the topk-th; "below": the topk-th is the last value under the boundary)
        x, h = robust_sigmoids()
        b = bin_of(h)
        edges = np.nonzero(b[1:] != b[:-1])[0]                      # h[i] below a boundary, h[i + 1] above it
        edges = edges[(edges > 8) & (edges < len(h) - topk - 8)]
        i = int(edges[np.argmin((h[edges + 1].view(np.uint32) - h[edges].view(np.uint32)))])
        lv, heats = [], []
        for n in sizes:
            if n > topk + 8:
                top = i + 1 if case == "cut edge above" else i      # index of the topk-th score in the table
                must = np.array([top] if case == "cut edge above" else [top, top + 1])
                pool = np.arange(top + len(must), len(h))
                rest = pool[torch.randperm(len(pool), generator=g)[:topk - len(must)].numpy()]
                idx = np.concatenate([np.arange(top - 3, top), must, rest])       # three losers, the topk-th (and its neighbour), the rest
                pos = torch.randperm(n, generator=g)[:len(idx)]
                lg, ht = torch.full((n,), OFF), torch.zeros(n)
                lg[pos], ht[pos] = torch.from_numpy(x[idx]), torch.from_numpy(h[idx])
            else:
                k = torch.randperm(len(h), generator=g)[:n].numpy()
                lg, ht = torch.from_numpy(x[k]), torch.from_numpy(h[k])
            lv.append(lg)
            heats.append(ht)
    elif case == "saturated":
        # 1 + expf(-20) rounds to 1: the score is exactly 1.0 on more positions than topk where the level is large enough
        lv = [torch.where(torch.rand(n, generator=g) < 0.4, torch.tensor(20.0), sep(n) if n <= 12000 else torch.full((n,), -1.0)) for n in sizes]
    elif case == "empty level":
        lv = [sep(min(n, 12000)) if n <= 12000 else scatter(n, sep(12000)) for n in sizes]
        lv[1 % L] = torch.full((sizes[1 % L],), OFF)
    elif case in ("exactly topk", "topk + 1"):
        k = topk if case == "exactly topk" else topk + 1
        lv = [scatter(n, sep(min(k, n))) for n in sizes]
    elif case == "few fine many coarse":
        lv = [scatter(n, sep(min(n, 300 if l == 0 else 12000))) for l, n in enumerate(sizes)]
    elif case == "post-nms ties":
        # tiny boxes: NMS keeps everything; post - 10 distinct high scores, then 30 equal ones straddling the cut, lower ones behind
        lv, regime = [], "tiny"
        for l, n in enumerate(sizes):
            if l == 0:
                v = sep(post + 200).sort(descending=True).values
                v[post - 10:post + 20] = v[post - 10]
                lv.append(scatter(n, v))
            else:
                lv.append(torch.full((n,), OFF))
    else:
        raise KeyError(case)
    return [v.float().contiguous() for v in lv], heats, regime


def hostile_reg(regime: str, level_hw: Sequence[Tuple[int, int]], seed: int) -> List[torch.Tensor]:
    """Raw bbox_pred per level [n, 4] (the kernel takes relu(scale * reg) * stride)."""
    g = torch.Generator().manual_seed(seed)
    out = []
    for h, w in level_hw:
        n = h * w
        if regime == "tiny":
            out.append(torch.full((n, 4), 0.2) + torch.rand((n, 4), generator=g) * 0.05)
        elif regime == "stacked":
            out.append(torch.full((n, 4), 40.0) + torch.rand((n, 4), generator=g) * 0.01)
        else:
            r = torch.randn((n, 4), generator=g) * 2.0 + 3.0        # a fifth of them negative: the ReLU's zero side
            out.append(r)
    return out


def sqrt_rn(x: torch.Tensor) -> torch.Tensor:
    """The correctly rounded fp32 square root (what sqrtf is on the device, and what numpy gives): the root in float64, rounded once
    more -- float64 carries more than twice fp32's bits plus two, so the second rounding cannot move the result.  torch.sqrt on a
    float32 CPU tensor is NOT this on every host: its vectorised path was seen one ulp off on 108 of the 42 384 values of
    `robust_sigmoids` (short tensors, which take the scalar path, were right), enough to tie two scores the device keeps apart."""
    return torch.sqrt(x.double()).float()


def proposals_reference(heat: Sequence[torch.Tensor], reg: Sequence[torch.Tensor], level_hw, strides, scales, thresh: float, pre: int, post: int,
                        nms_thresh: float):
    """CenterNet.inference written out on given fp32 heat values (oracle/model.py `centernet_proposals` takes logits; this is the same
    sequence of decisions with the sigmoid taken out, so a test can hand in scores whose bits it knows)."""
    from oracle import ops as OO
    all_boxes, all_scores = [], []
    for l, ((h, w), ht, rg) in enumerate(zip(level_hw, heat, reg)):
        s = strides[l]
        regl = torch.relu(rg * scales[l]) * s
        gx = (torch.arange(w, dtype=torch.float32) * s + s // 2).repeat(h)
        gy = (torch.arange(h, dtype=torch.float32) * s + s // 2).repeat_interleave(w)
        cand = torch.nonzero(ht > thresh).squeeze(1)
        sc = ht[cand]
        if cand.numel() > pre:
            order = torch.sort(sc, descending=True, stable=True).indices[:pre]
            order = torch.sort(order).values
            cand, sc = cand[order], sc[order]
        r, x, y = regl[cand], gx[cand], gy[cand]
        det = torch.stack([x - r[:, 0], y - r[:, 1], x + r[:, 2], y + r[:, 3]], dim=1)
        det[:, 2] = torch.max(det[:, 2], det[:, 0] + 0.01)
        det[:, 3] = torch.max(det[:, 3], det[:, 1] + 0.01)
        all_boxes.append(det)
        all_scores.append(sqrt_rn(sc))
    boxes, scores = torch.cat(all_boxes), torch.cat(all_scores)
    keep = OO.nms(boxes, scores, nms_thresh)
    boxes, scores = boxes[keep], scores[keep]
    n_nms = boxes.shape[0]
    if n_nms > post:
        kth = torch.kthvalue(scores, n_nms - post + 1).values
        k = torch.nonzero(scores >= kth).squeeze(1)
        boxes, scores = boxes[k], scores[k]
    return boxes, scores, int(torch.cat([(h > thresh).sum().clamp(max=pre)[None] for h in heat]).sum()), n_nms


def head_rows(logits: Sequence[Sequence[torch.Tensor]], reg: Sequence[Sequence[torch.Tensor]], head_stride: int) -> torch.Tensor:
    """logits[b][l], reg[b][l] -> the head's output rows, LEVEL MAJOR over the scenes, `head_stride` columns (column 0 the logit, 1..4
    the regression, the rest a NaN pad nothing may read into a result)."""
    B, L = len(logits), len(logits[0])
    rows = []
    for l in range(L):
        for b in range(B):
            r = torch.full((logits[b][l].numel(), head_stride), float("nan"))
            r[:, 0], r[:, 1:5] = logits[b][l], reg[b][l]
            rows.append(r)
    return torch.cat(rows).contiguous()


# ------------------------------------------------------------------------------------------------
# paste: the sampled probability of every pixel in float64, and the band inside which fp32 may decide either way
# ------------------------------------------------------------------------------------------------
def _paste_axis(lo: float, hi: float, extent: int, dtype=torch.float64) -> torch.Tensor:
    """[extent, 28]: the bilinear weights of F.grid_sample(bilinear, zeros, align_corners=False) along one axis on the normalised grid
    detectron2's _do_paste_mask builds: g = (c + 0.5 - lo) / (hi - lo) * 2 - 1, i = ((g + 1) * 28 - 1) / 2; taps floor(i), floor(i) + 1
    with weights 1 - frac, frac; a tap outside [0, 28) contributes zero.  hi == lo: no finite sample, zeros."""
    A = torch.zeros((extent, 28), dtype=dtype)
    lo, hi = torch.tensor(lo, dtype=dtype), torch.tensor(hi, dtype=dtype)
    if not bool(torch.isfinite(lo) & torch.isfinite(hi)) or bool(hi == lo):
        return A
    c = torch.arange(extent, dtype=dtype) + 0.5
    i = (((c - lo) / (hi - lo) * 2 - 1 + 1) * 28 - 1) / 2
    ok = (i > -1) & (i < 28)
    f = torch.floor(i)
    frac = i - f
    f = f.long()
    for tap, wgt in ((f, 1 - frac), (f + 1, frac)):
        m = ok & (tap >= 0) & (tap < 28)
        A[torch.nonzero(m).squeeze(1), tap[m]] += wgt[m]
    return A


def paste_prob(mask: torch.Tensor, box: torch.Tensor, H: int, W: int, dtype=torch.float64) -> torch.Tensor:
    """One instance: mask [28, 28], box [4] (the fp32 values, taken to `dtype` unrounded) -> [H, W] sampled probabilities.  The
    bilinear sample is a product of a y and an x weight, so the image is Ay . m . Ax^T."""
    b = [float(v) for v in box]
    Ay, Ax = _paste_axis(b[1], b[3], H, dtype), _paste_axis(b[0], b[2], W, dtype)
    return Ay @ mask.to(dtype) @ Ax.t()


PASTE_HEAD = 2.0


def paste_band(mask: torch.Tensor) -> float:
    """How far from the threshold the float64 probability of a pixel must be for the fp32 kernel's decision to be determined.
    The coordinate chain of one axis in fp32: c + 0.5 exact; - lo one rounding (relative U of the difference); hi - lo one; the
    quotient one: 3 U relative on a ratio of magnitude <= 29/28 wherever the sample is in range, 3.2 U absolute.  * 2 - 1 adds U |g|
    <= 1.1 U: 7.5 U on g.  g + 1 (2.1 U), * 28 (U 58), - 1 (U 58), / 2: i is off by <= (9.6 U * 28 + 116 U) / 2 < 200 U mask pixels.
    A bilinear sample moves by at most the largest step between neighbouring mask pixels (the zero padding counted as a neighbour)
    per mask pixel and axis: 400 U G.  The four weights (2 roundings each) and the four-term sum add 12 U max|m|."""
    m = mask.double()
    p = torch.zeros((30, 30), dtype=torch.float64)
    p[1:29, 1:29] = m
    G = max(float((p[1:] - p[:-1]).abs().max()), float((p[:, 1:] - p[:, :-1]).abs().max()))
    return PASTE_HEAD * U * (400.0 * G + 12.0 * float(m.abs().max()))


def hostile_paste_boxes(H: int, W: int, K: int, seed: int) -> torch.Tensor:
    """K boxes built to hurt the 16-pixel run skip of the paste kernel: edges exactly on run boundaries and half a pixel to either side,
    boxes that start inside a run, narrower than a pixel, zero-width, inverted, wider than the image, crossing every border, wholly
    outside; seeded boxes for the rest."""
    fx = [[0.0, 0.0, W, H], [-0.4 * W, -0.3 * H, 1.5 * W, 1.2 * H],                                     # the image; wider than it
          [16.0, 32.0, 48.0, 64.0], [15.5, 31.5, 47.5, 63.5], [16.5, 32.5, 48.5, 64.5],                 # edges on run boundaries, +- 1/2
          [W - 32.0, H - 32.0, W, H], [W - 32.5, H - 31.5, W - 0.5, H + 0.5],
          [21.3, 40.7, 26.9, 90.1], [W - 9.1, 5.3, W - 2.2, 200.7],                                     # inside one run
          [100.2, 50.0, 100.9, 300.0], [300.4, 17.5, 300.6, 18.4], [77.0, 77.0, 77.0, 300.0],            # under a pixel; zero width
          [200.3, 90.1, 150.7, 140.9], [240.1, 220.3, 300.7, 190.1], [0.0, 0.0, 0.0, 0.0],               # inverted; empty
          [-23.3, 50.3, 40.9, 122.7], [W - 48.1, 77.7, W + 31.3, 160.3], [91.3, -19.1, 170.7, 44.3], [203.1, H - 39.3, 290.9, H + 27.7],
          [-60.3, -44.1, -10.7, -3.3], [W + 12.3, 40.1, W + 90.7, 133.3],                                # wholly outside
          [31.9, 10.0, 64.1, 24.0], [32.0 - 2.0 ** -18, 12.0, 64.0 + 2.0 ** -18, 30.0],                  # a hair around run boundaries
          [0.0, 0.0, 14.0, 14.0], [5.0, 5.0, 5.0 + 28.0, 5.0 + 28.0], [3.5, 3.5, 3.5 + 56.0, 3.5 + 56.0]]  # half / one / two image pixels per mask pixel
    fx = fx[:K]
    g = torch.Generator().manual_seed(seed)
    n = K - len(fx)
    ctr = torch.rand((n, 2), generator=g) * torch.tensor([float(W), float(H)])
    half = torch.exp(torch.rand((n, 2), generator=g) * 4.5 + 0.5)
    rnd = torch.cat([ctr - half, ctr + half], dim=1)
    return torch.cat([torch.tensor(fx, dtype=torch.float32).reshape(-1, 4), rnd.float()]).contiguous()


def hostile_masks(n: int, seed: int) -> torch.Tensor:
    """[n, 28, 28] probabilities: seeded noise (steps of up to 1 between neighbours), plateaus of 0 / 1 with one-pixel edges, smooth
    blobs whose 0.5 contour crosses the pixel grid at every phase, a full mask (the border against the zero padding is the edge).
    No plateau AT the threshold: the four fp32 bilinear weights need not sum to exactly 1, so every pixel of a 0.5 plateau lies
    inside the band, where either decision is right, and nothing could be asserted about it."""
    g = torch.Generator().manual_seed(seed)
    yy, xx = torch.meshgrid(torch.arange(28.0), torch.arange(28.0), indexing="ij")
    out = torch.empty((n, 28, 28))
    for k in range(n):
        kind = k % 4
        if kind == 0:
            out[k] = torch.rand((28, 28), generator=g)
        elif kind == 1:
            a, b = sorted(torch.randint(2, 26, (2,), generator=g).tolist())
            out[k] = ((xx >= a) & (xx <= b) & (yy >= 28 - b) & (yy <= 30 - a)).float()
        elif kind == 2:
            c = torch.rand(2, generator=g) * 12 + 8
            r = float(torch.rand(1, generator=g)) * 6 + 4
            out[k] = torch.sigmoid((r - torch.sqrt((xx - c[0]) ** 2 + (yy - c[1]) ** 2)) * 0.8)
        else:
            out[k] = 1.0
    return out.contiguous()


# ------------------------------------------------------------------------------------------------
# detection selection: boxes and scores built to hurt the sort batches, the per-class NMS and the row grouping
# ------------------------------------------------------------------------------------------------
def hostile_detections(case: str, R: int, C1: int, img_w: float, img_h: float, seed: int) -> Tuple[torch.Tensor, torch.Tensor]:
    g = torch.Generator().manual_seed(seed)
    ctr = torch.rand((R, 2), generator=g) * torch.tensor([img_w, img_h])
    size = torch.exp(torch.rand((R, 2), generator=g) * 4.0 + 2.0)
    boxes = torch.cat([ctr - size / 2, ctr + size / 2], dim=1)
    scores = torch.rand((R, C1), generator=g) ** 3
    if case == "seeded":
        scores[3 % R, 5] = float("nan")
        boxes[7 % R, 2] = float("inf")
    elif case == "equal scores":
        # 1/4 of the entries share one of four scores, across classes and rows: order = (row, class) among equals
        tie = torch.tensor([0.75, 0.5, 0.25, 0.125])[torch.randint(0, 4, (R, C1), generator=g)]
        scores = torch.where(torch.rand((R, C1), generator=g) < 0.25, tie, scores)
    elif case == "stacked":
        # everything on one spot: per-class NMS removes nearly all, the first 1024 candidates do not fill topk
        ctr = torch.tensor([img_w / 2, img_h / 2]) + (torch.rand((R, 2), generator=g) - 0.5) * 12
        size = 200 + torch.rand((R, 2), generator=g) * 40
        boxes = torch.cat([ctr - size / 2, ctr + size / 2], dim=1)
        scores = torch.rand((R, C1), generator=g) * 0.5 + 0.4
    elif case == "iou at threshold":
        # power-of-two coordinates: intersections, areas and the quotient are exact in fp32.  Pairs at IoU = 1/2 exactly (kept:
        # the test is '>'), at 1/3 (kept) and at 0.6 (suppressed).  One ulp either side of 1/2 needs areas of ~2^23 units with exact
        # sums, which boxes on 1/16-pixel coordinates could give; that case is not built here
        n = R // 4
        x0 = (torch.arange(n) * 192.0) % (img_w - 192)
        y0 = (torch.arange(n) * 192.0 // (img_w - 192)) * 80.0 % (img_h - 80)
        a = torch.stack([x0, y0, x0 + 128, y0 + 64], dim=1)
        b = torch.stack([x0 + 64, y0, x0 + 128 + 64 + 64, y0 + 64], dim=1)          # inter 64x64 = 4096 / union 8192 + 8192 - 4096: 1/3
        b2 = torch.stack([x0 + 32, y0, x0 + 32 + 128, y0 + 64], dim=1)              # inter 96 x 64 / union 160 x 64 = 0.6: clearly above
        c = torch.stack([x0, y0, x0 + 128, y0 + 32], dim=1)                         # inside a: 1/2 exactly
        boxes = torch.cat([a, b, c, b2])[:R]
        boxes = torch.cat([boxes, torch.zeros((R - boxes.shape[0], 4))])
        scores = torch.rand((R, C1), generator=g) * 0.5 + 0.3
    else:
        raise KeyError(case)
    scores[:, C1 - 1] = torch.where(torch.isfinite(scores[:, C1 - 1]), 1.0 - scores[:, :C1 - 1].nan_to_num().max(dim=1).values.clamp(0, 1),
                                    scores[:, C1 - 1])
    return boxes.float().contiguous(), scores.float().contiguous()


DET_CASES = ("seeded", "equal scores", "stacked", "iou at threshold")


def group_rows(rows: Sequence[int]) -> Tuple[List[int], List[int]]:
    """The detection-mask groups restated: detections of one proposal row share a box, the first of them stands for the group.
    -> (rep_of[k] = index of the first detection with k's row, rep_list = those first detections in order)."""
    first: Dict[int, int] = {}
    rep_of, rep_list = [], []
    for k, r in enumerate(rows):
        if r not in first:
            first[r] = k
            rep_list.append(k)
        rep_of.append(first[r])
    return rep_of, rep_list


# ------------------------------------------------------------------------------------------------
# memory read: the pooled rows of the three levels in fp16, summed in F.avg_pool2d's order
# ------------------------------------------------------------------------------------------------
def gather_patterns(name: str, H: int, W: int, N: int, seed: int) -> torch.Tensor:
    """Cell index images [H, W] of test_memory_read_matches_oracle at any size, plus `half`: the left half of every row its own cell
    per pixel (a tile's list overflows), the right half one cell (the uniform shortcut) -- both in one 32-pixel-wide tile row."""
    g = torch.Generator().manual_seed(seed)
    if name == "blocky":
        proj = torch.randint(0, N, (H, W), generator=g)
        blocky = ((torch.arange(H)[:, None] // 6) * 17 + (torch.arange(W)[None, :] // 9)) % N
        return torch.where(torch.rand((H, W), generator=g) < 0.7, blocky, proj)
    if name == "distinct":
        return (torch.randperm(H * W, generator=g) % N).reshape(H, W) if N < H * W else torch.randperm(N, generator=g)[:H * W].reshape(H, W)
    if name == "constant":
        return torch.full((H, W), N - 1, dtype=torch.int64)
    if name == "columns":
        return (torch.arange(W)[None, :] * 5 % N).expand(H, W).contiguous()
    if name == "half":
        proj = (torch.arange(H * W).reshape(H, W) * 7919) % N
        proj[:, (torch.arange(W) // 16) % 2 == 1] = 0
        return proj
    raise KeyError(name)


GATHER_PATTERNS = ("blocky", "distinct", "constant", "columns", "half")


def pooled_reference(m16: torch.Tensor, proj: torch.Tensor) -> List[torch.Tensor]:
    """oracle/model.py `memory_read_pooled` on the fp16 table -> the row-major [P_l, 512] rows of the three levels."""
    from oracle import model as M
    return [r[0].permute(1, 2, 0).reshape(-1, 512).contiguous() for r in M.memory_read_pooled(m16, proj)]


def rows_to_fragments(level_rows: Sequence[torch.Tensor]) -> torch.Tensor:
    """Row-major [P_l, 512] rows of the three levels -> the operand-fragment order the projection reads (the inverse of
    `_launch_cases.fragments_to_rows`); padding rows are NaN: they must never reach a stored result."""
    out = []
    for rws in level_rows:
        rows = rws.shape[0]
        tiles = (rows + 31) // 32
        pad = torch.full((tiles * 32, 512), float("nan"), dtype=rws.dtype)
        pad[:rows] = rws
        out.append(pad.view(tiles, 32, 32, 2, 8).permute(0, 2, 3, 1, 4).reshape(-1))
    return torch.cat(out).view(-1, 512)


def projector_bound(absdot: torch.Tensor, result: torch.Tensor, weight: float) -> torch.Tensor:
    """Element-wise bound on the fp32 error of (pooled . W^T + b) * weight (+ P): the weights enter as two fp16 pieces that reproduce
    the fp32 value to one rounding (U relative per product), the 512 products are exact and summed in fp32 in some order (at most
    512 U of the sum of magnitudes; the head-room below counts a quarter of that worst case, as pairwise / blocked orders give),
    then bias, scale and residual: three roundings of the result."""
    return (U * (1.0 + 128.0) * absdot * abs(weight) + 4.0 * U * result.abs()) * 2.0
