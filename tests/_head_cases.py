"""CPU side of test_head_launches_gpu.py: float64 references, derived bounds, CPU fp32 emulations of the kernels' summation orders
and the input builders of the box-head and post-processing launches.  Plain torch / numpy; nothing here touches a GPU.

Every operation below is written ONCE, over a dtype: at float64 with a plain matrix product it is the reference, at float32 with one
of the emulated summation orders it is the yardstick (the error a correct fp32 implementation in the kernel's order makes).  What the
references share with the kernels are the upstream definitions only: `normalize(p=2, eps=1e-12) * temp`, the sigmoid,
`sqrt(p * inv_stages * ps)`, `p < 1 ? sqrt(sigmoid * p) : 0`, and Box2BoxTransform with the `log(1000/16)` clamp followed by the clip.

BOUNDS.  U = 2^-24 is the fp32 unit round-off; a sum of n roundings of terms t_k errs by at most U * n * sum|t_k| to first order.
Every count below is multiplied by HEAD = 2, the project's usual head-room (ROI_HEAD, PASTE_HEAD), and by nothing else.

  logit       HEAD * U * (n_norm + n_sum) * A,  A = sum_k |xn_k * z_k| in float64.
              n_norm = 17: the relative error of a normalised channel -- eight squares-and-adds per lane, six butterfly steps, the
              square root, the division, the multiplication by temp (the sum of squares has positive terms only, the root halves its
              error: 17 is an upper count).  n_norm = 0 where the launch is handed normalised rows (`memory_scores`).
              n_sum = the longest chain of additions a product goes through, plus one for the product itself:
                narrow  8 per lane + 6 butterfly steps + 1 = 15
                wide    128 matrix-core steps of a K-quarter + 3 additions of the quarters + 1 = 132
  featn       HEAD * U * n_norm * |xn|
  probability |dp| <= sigmoid'(logit) * e^{dlogit} * dlogit + 4 U p + TINY.  4 U p: expf to one ulp (2 U), 1 + e, the division.  The
              second term is RELATIVE: a probability of 1e-20 is held to 1e-27.  sigmoid' = p (1 - p) is evaluated as e / (1 + e)^2
              (1 - p is 0 in float64 long before p (1 - p) is); e^{dlogit} bounds sigmoid' over the interval.  TINY is the smallest
              normal fp32, the absolute floor.
  accumulate  acc = old + p: d acc = dp + HEAD * U * acc (`old` is an input of the launch: exact).
  fusion      v = sqrt(acc * inv * ps): relative error (d acc / acc + 2 U) / 2 + U, hence dv = v * d acc / (2 acc) + HEAD * 2 U * v + TINY.
              ps = 0 gives v = 0 with a bound of TINY: the kernel's product is exactly 0 too.
  re-score    v = p < 1 ? sqrt(sigmoid * p) : 0: dv = v * dsig / (2 sig) + HEAD * 1.5 U * v + TINY; `p < 1` is a decision on an INPUT.
  deltas      d = sum_k h_k w_k + b with 16 inputs per lane and trip, six butterfly steps, the product, then the bias:
              HEAD * U * ((16 trips + 6 + 1) * S + (S + |b|)),  S = sum|h w|.  With b = 0 this is 2 U (16 trips + 6 + 2) S; the addition
              of the bias rounds at the size of the RESULT, which a bias of 20 beside S = 0.5 dominates -- a bound in S alone is below
              the error of a correctly rounded fp32 addition there.
  boxes       first-order propagation of dd through the transform (`box_bounds`); min(., clamp) and the clip are 1-Lipschitz, so no
              element is excluded.
  mask prob.  s = sum x w + bias with four products per lane and trip added as one expression (4 additions per trip), six butterfly
              steps, the bias: HEAD * U * ((4 trips + 6 + 1) * S + (S + |bias|)); then the probability as above.

The square roots are propagated to first order; their second-order term is (relative error)^2 / 8 < 1e-9 of the bound here.
test_head_launches_gpu.py::test_fp32_emulation_stays_inside_every_bound holds every one of these bounds against the emulation on every
case of the tables below; ::test_references_are_the_oracles ties every reference to oracle/ops.py, oracle/model.py and oracle/memory.py."""
import functools
import math
from typing import Dict, Optional, Sequence, Tuple

import numpy as np
import torch

from _launch_cases import SENTINEL, U          # noqa: F401  (re-exported)

HEAD = 2.0
TINY = 2.0 ** -126
TEMP = 50.0
INV3 = float(np.float32(1.0 / 3.0))                                 # the `final_inv_stages` the launch really receives
BELOW1 = float(np.nextafter(np.float32(1.0), np.float32(0.0)))      # the largest float below 1
SCALE_CLAMP = math.log(1000.0 / 16)
N_NORM = 8 + 6 + 3
N_SUM = {"narrow": 8 + 6 + 1, "wide": 128 + 3 + 1}
F32, F64 = torch.float32, torch.float64
I32_SENTINEL = -77777


# ------------------------------------------------------------------------------------------------
# summation orders (fp32 emulations) and the float64 product
# ------------------------------------------------------------------------------------------------
_LANES = torch.arange(64)


def _butterfly(s: torch.Tensor) -> torch.Tensor:
    """s [R, 64, ...] -> the wave's xor butterfly (offsets 32 .. 1); every lane ends with the same bits: lane 0's are returned."""
    for off in (32, 16, 8, 4, 2, 1):
        s = s + s[:, _LANES ^ off]
    return s[:, 0]


def lane_dot(x: torch.Tensor, z: torch.Tensor, per: int, grouped: bool = False) -> torch.Tensor:
    """fp32 x [R, K] @ z [K, C] in the order of a wave-per-row kernel: lane l owns inputs l * per .. l * per + per - 1 of every trip of
    64 * per, adds their products one after the other (`grouped`: the trip's products are added to each other first and then onto the
    lane's sum, as one expression), then the butterfly.  Lanes beyond K hold 0."""
    R, K = x.shape
    C = z.shape[1]
    T = -(-K // (64 * per))
    xp = torch.zeros((R, T * 64 * per), dtype=F32)
    xp[:, :K] = x
    zp = torch.zeros((T * 64 * per, C), dtype=F32)
    zp[:K] = z
    xp, zp = xp.view(R, T, 64, per), zp.view(T, 64, per, C)
    s = torch.zeros((R, 64, C), dtype=F32)
    for t in range(T):
        e = None
        for q in range(per):
            p = xp[:, t, :, q, None] * zp[None, t, :, q, :]
            if grouped:
                e = p if e is None else e + p
            else:
                s = s + p
        if grouped:
            s = s + e
    return _butterfly(s)


def lane_sumsq(x: torch.Tensor) -> torch.Tensor:
    """fp32 sum of squares of x [R, 512]: eight per lane in channel order, then the butterfly."""
    xv = x.view(x.shape[0], 64, 8)
    s = torch.zeros((x.shape[0], 64), dtype=F32)
    for q in range(8):
        s = s + xv[:, :, q] * xv[:, :, q]
    return _butterfly(s)


def quarter_dot(x: torch.Tensor, z: torch.Tensor) -> torch.Tensor:
    """fp32 x [R, 512] @ z [512, C] in the wide kernel's order: four K-quarters of 128 channels, each 64 matrix-core steps of two
    channels (s and 64 + s of the quarter), then ((q0 + q1) + q2) + q3."""
    qs = []
    for w in range(4):
        acc = torch.zeros((x.shape[0], z.shape[1]), dtype=F32)
        for s in range(64):
            for k in (128 * w + s, 128 * w + 64 + s):
                acc = acc + x[:, k, None] * z[None, k, :]
        qs.append(acc)
    return ((qs[0] + qs[1]) + qs[2]) + qs[3]


def dot(x: torch.Tensor, z: torch.Tensor, order: str, dt) -> torch.Tensor:
    if dt == F64:
        return x.double() @ z.double()
    return lane_dot(x, z, 8) if order == "narrow" else quarter_dot(x, z)


# ------------------------------------------------------------------------------------------------
# the definitions, over a dtype
# ------------------------------------------------------------------------------------------------
def sigmoid(x: torch.Tensor) -> torch.Tensor:
    return 1.0 / (1.0 + torch.exp(-x))


def sigmoid_slope(x64: torch.Tensor) -> torch.Tensor:
    """p (1 - p) without the cancellation of 1 - p."""
    e = torch.exp(-x64.abs())
    return e / (1.0 + e) ** 2


def normalise(feat: torch.Tensor, dt, temp: float = TEMP) -> torch.Tensor:
    x = feat.to(dt)
    ss = (x * x).sum(1) if dt == F64 else lane_sumsq(x)
    den = torch.sqrt(ss).clamp(min=1e-12)
    return torch.tensor(temp, dtype=dt) * (x / den[:, None])


def classifier(feat, zs, order: str, dt, *, old=None, inv: float = 0.0, ps=None, zs_mem=None, normalised: bool = False) -> Dict[str, torch.Tensor]:
    """One classifier launch.  -> featn, and as asked: logit / p / out (sigmoid, + old, fused with ps when inv > 0) and
    mem_logit / mem_sig / mem (the re-score with `zs_mem`).  `normalised`: `feat` are normalised rows already and only the re-score is
    computed (`memory_scores`)."""
    r = {"featn": feat.to(dt) if normalised else normalise(feat, dt)}
    if not normalised:
        r["logit"] = dot(r["featn"], zs.to(dt), order, dt)
        r["p"] = sigmoid(r["logit"])
        r["acc"] = r["p"] if old is None else old.to(dt) + r["p"]
        r["out"] = torch.sqrt(r["acc"] * torch.tensor(inv, dtype=dt) * ps.to(dt)[:, None]) if inv > 0 else r["acc"]
    if zs_mem is not None:
        p = ps.to(dt)[:, None]
        r["mem_logit"] = dot(r["featn"], zs_mem.to(dt), order, dt)
        r["mem_sig"] = sigmoid(r["mem_logit"])
        r["mem"] = torch.where(p < 1, torch.sqrt(r["mem_sig"] * p), torch.zeros((), dtype=dt))
    return r


def share(err: torch.Tensor, bound: torch.Tensor) -> torch.Tensor:
    """err / bound; where the bound is 0 (an exact result is expected): 0 for no error, inf for any."""
    return torch.where(bound > 0, err / bound.clamp(min=1e-300), torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))


def prob_bound(logit64, b_logit, p64):
    return sigmoid_slope(logit64) * torch.exp(b_logit) * b_logit + 4 * U * p64 + TINY


def classifier_bounds(r, zs, order: str, *, old=None, inv: float = 0.0, ps=None, zs_mem=None, normalised: bool = False) -> Dict[str, torch.Tensor]:
    """The bounds of `classifier`'s outputs from its float64 result `r` (module docstring)."""
    n = (0 if normalised else N_NORM) + N_SUM[order]
    ax = r["featn"].abs()
    b = {"featn": HEAD * U * N_NORM * ax + TINY}
    if not normalised:
        b["logit"] = HEAD * U * n * (ax @ zs.double().abs())
        b_acc = prob_bound(r["logit"], b["logit"], r["p"])
        if old is not None:
            b_acc = b_acc + HEAD * U * r["acc"]
        b["out"] = r["out"] * b_acc / (2 * r["acc"]) + HEAD * 2 * U * r["out"] + TINY if inv > 0 else b_acc
    if zs_mem is not None:
        b["mem_logit"] = HEAD * U * n * (ax @ zs_mem.double().abs())
        b_sig = prob_bound(r["mem_logit"], b["mem_logit"], r["mem_sig"])
        live = (ps.double() < 1)[:, None]
        b["mem"] = torch.where(live, r["mem"] * b_sig / (2 * r["mem_sig"]) + HEAD * 1.5 * U * r["mem"] + TINY, torch.zeros((), dtype=F64))
    return b


def box_transform(d, boxes, weights, clip: bool, img_w: float, img_h: float, dt) -> torch.Tensor:
    """Box2BoxTransform.apply_deltas (`log(1000/16)` clamp on dw, dh) and, with `clip`, Boxes.clip to the image."""
    d, b = d.to(dt), boxes.to(dt)
    wx, wy, ww, wh = (torch.tensor(v, dtype=dt) for v in weights)
    w, h = b[:, 2] - b[:, 0], b[:, 3] - b[:, 1]
    cx, cy = b[:, 0] + 0.5 * w, b[:, 1] + 0.5 * h
    dx, dy = d[:, 0] / wx, d[:, 1] / wy
    dw, dh = (d[:, 2] / ww).clamp(max=SCALE_CLAMP), (d[:, 3] / wh).clamp(max=SCALE_CLAMP)
    pcx, pcy = dx * w + cx, dy * h + cy
    pw, ph = torch.exp(dw) * w, torch.exp(dh) * h
    out = torch.stack([pcx - 0.5 * pw, pcy - 0.5 * ph, pcx + 0.5 * pw, pcy + 0.5 * ph], dim=1)
    if clip:
        out = torch.stack([out[:, 0].clamp(0, img_w), out[:, 1].clamp(0, img_h), out[:, 2].clamp(0, img_w), out[:, 3].clamp(0, img_h)], dim=1)
    return out


def box_bounds(d64, b_d, boxes, weights) -> torch.Tensor:
    """|error| of the transformed box [R, 4] given |error| b_d [R, 4] of the deltas (0 where they are inputs).  Per axis, with
    w = x2 - x1, cx = x1 + w / 2, dx = d0 / wx, dw = min(d2 / ww, clamp):
      centre  pcx = dx w + cx: (|w| / wx) dd0 + HEAD * 5 U (|dx w| + |x1| + |w| / 2)   -- w, the division, the product, cx, the sum
      extent  pw = exp(dw) w:  |pw| (dd2 / ww + HEAD * U (|dw| + 4))                   -- the division (and the fp32 clamp constant)
                                                                                          move the exponent by |dw| U; expf to an ulp
                                                                                          (2 U), w, the product
      corner  pcx -+ pw / 2:   the two above, the second halved, + HEAD * U (|pcx| + |pw| / 2)
    The clip moves no corner further than it already erred."""
    d, b = d64.double(), boxes.double()
    out = torch.zeros((d.shape[0], 4), dtype=F64)
    for a in (0, 1):
        wc, ws = float(weights[a]), float(weights[2 + a])
        w = b[:, 2 + a] - b[:, a]
        dc = d[:, a] / wc
        de = (d[:, 2 + a] / ws).clamp(max=SCALE_CLAMP)
        pc = dc * w + b[:, a] + 0.5 * w
        pe = torch.exp(de) * w
        e_c = w.abs() / wc * b_d[:, a] + HEAD * 5 * U * ((dc * w).abs() + b[:, a].abs() + 0.5 * w.abs())
        e_e = pe.abs() * (b_d[:, 2 + a] / ws + HEAD * U * (de.abs() + 4))
        e = e_c + 0.5 * e_e + HEAD * U * (pc.abs() + 0.5 * pe.abs()) + TINY
        out[:, a], out[:, 2 + a] = e, e
    return out


def linear_bound(S: torch.Tensor, bias: torch.Tensor, per: int, K: int) -> torch.Tensor:
    """sum + bias of a wave-per-row dot product of `per` inputs per lane and trip: HEAD U ((per trips + 6 + 1) S + (S + |bias|))."""
    trips = -(-K // (64 * per))
    return HEAD * U * ((per * trips + 6 + 1) * S + (S + bias.double().abs())) + TINY


# ------------------------------------------------------------------------------------------------
# inputs
# ------------------------------------------------------------------------------------------------
NARROW_C1 = (2, 21, 24)
WIDE_C1 = (25, 32, 33, 1204)
# (R_cap, counts or None, batch)
NARROW_ROWS = ((8, None, 1), (8, (5,), 1), (8, (0,), 1), (6, None, 1), (64, (50,), 1), (8, (8, 0, 3), 3))
WIDE_ROWS = ((32, None, 1), (33, None, 1), (40, (33,), 1), (40, (0,), 1), (64, (31,), 1), (36, (36, 0, 5), 3))
FORMS = ("stage0", "middle", "last")
SMALL_R = (1, 255, 257)
NORM15_C1 = (21, 33)                  # the class matrices whose column 0 has norm 1.5


def wide_rows(C1: int):
    return ((40, (33,), 1),) if C1 == 1204 else WIDE_ROWS


def classifier_table():
    """Every (order, C1, R_cap, counts, batch) of the two classifier kernels."""
    for C1 in NARROW_C1:
        for R_cap, counts, batch in NARROW_ROWS:
            yield "narrow", C1, R_cap, counts, batch
    for C1 in WIDE_C1:
        for R_cap, counts, batch in wide_rows(C1):
            yield "wide", C1, R_cap, counts, batch


def live_rows(R_cap: int, counts: Optional[Sequence[int]], batch: int) -> torch.Tensor:
    """bool [R_cap * batch]: row r of list r // R_cap holds work."""
    r = torch.arange(R_cap * batch)
    if counts is None:
        return torch.ones_like(r, dtype=torch.bool)
    c = torch.tensor(counts).clamp(max=R_cap)
    return (r % R_cap) < c[r // R_cap]


@functools.lru_cache(maxsize=None)
def class_matrix(C1: int, seed: int) -> torch.Tensor:
    """[512, C1] fp32, every column of norm 1 (to fp32 rounding); column 0 of norm 1.5 for C1 in NORM15_C1 and seed 0."""
    g = torch.Generator().manual_seed(1000 * seed + C1)
    z = torch.randn((512, C1), generator=g, dtype=F64)
    z = z / z.norm(dim=0, keepdim=True)
    if seed == 0 and C1 in NORM15_C1:
        z[:, 0] *= 1.5
    return z.float().contiguous()


def feature_rows(R_cap: int, batch: int, zs: torch.Tensor, seed: int) -> torch.Tensor:
    """[R_cap * batch, 512] fp32.  Row j of every list is of kind j mod 7: all zero (featn = 0, p = 0.5 exactly) / one non-zero
    channel / scaled by 1e-3 / scaled by 1e4 / + column 1 of the class matrix / - column 1 (logits +-50) / plain; the hostile kinds come
    first so that a list of five live rows still holds five of them.  Rows beyond a list's count hold features too (a kernel that
    computed them would write them)."""
    g = torch.Generator().manual_seed(seed)
    f = torch.randn((R_cap * batch, 512), generator=g)
    for r in range(R_cap * batch):
        kind = (r % R_cap) % 7
        if kind == 0:
            f[r] = 0
        elif kind == 1:
            f[r] = 0
            f[r, (37 * r + 5) % 512] = -3e-7
        elif kind == 2:
            f[r] *= 1e-3
        elif kind == 3:
            f[r] *= 1e4
        elif kind == 4:
            f[r] = zs[:, 1]
        elif kind == 5:
            f[r] = -zs[:, 1]
    return f.contiguous()


def proposal_scores(rows: int, seed: int) -> torch.Tensor:
    """[rows] fp32 cycling through 0, the largest float below 1, 1.0, 1.5 and a plain score in [0.05, 0.95]."""
    g = torch.Generator().manual_seed(seed)
    ps = torch.rand((rows,), generator=g) * 0.9 + 0.05
    for k, v in enumerate((0.0, BELOW1, 1.0, 1.5)):
        ps[k::5] = v
    return ps


@functools.lru_cache(maxsize=None)
def classifier_case(order: str, C1: int, R_cap: int, counts, batch: int, form: str) -> Dict[str, object]:
    """Inputs, float64 reference, bounds and fp32 emulation of one classifier launch in one of the cascade's three forms:
    stage0 = fresh + featn_out + zs_mem / mem_scores_out; middle = accumulate onto a non-zero prob; last = accumulate + fusion."""
    rows = R_cap * batch
    zs, zs_mem = class_matrix(C1, 0), class_matrix(C1, 1)
    feat = feature_rows(R_cap, batch, zs, 7 * C1 + R_cap)
    ps = proposal_scores(rows, C1 + 3 * R_cap)
    g = torch.Generator().manual_seed(R_cap + C1)
    kw = dict(old=None if form == "stage0" else (torch.rand((rows, C1), generator=g) * 2 + 1e-3),
              inv=INV3 if form == "last" else 0.0, ps=ps, zs_mem=zs_mem if form == "stage0" else None)
    ref = classifier(feat, zs, order, F64, **kw)
    return dict(order=order, C1=C1, R_cap=R_cap, counts=counts, batch=batch, form=form, rows=rows, feat=feat, zs=zs, live=live_rows(R_cap, counts, batch),
                ref=ref, bound=classifier_bounds(ref, zs, order, **kw), emu=classifier(feat, zs, order, F32, **kw), **kw)


@functools.lru_cache(maxsize=None)
def rescore_case(order: str, C1: int, R_cap: int, counts) -> Dict[str, object]:
    """`memory_scores`: normalised fp32 rows in, sqrt(sigmoid * p) out (one list; the entry point has no batch form)."""
    zs = class_matrix(C1, 1)
    featn = normalise(feature_rows(R_cap, 1, zs, 11 * C1 + R_cap), F64).float().contiguous()
    ps = proposal_scores(R_cap, C1 + 5 * R_cap)
    kw = dict(ps=ps, zs_mem=zs, normalised=True)
    ref = classifier(featn, None, order, F64, **kw)
    return dict(order=order, C1=C1, R_cap=R_cap, counts=counts, featn=featn, zs=zs, ps=ps, live=live_rows(R_cap, counts, 1), ref=ref,
                bound=classifier_bounds(ref, None, order, **kw), emu=classifier(featn, None, order, F32, **kw))


def rescore_table():
    for C1 in (21, 24):
        for R_cap in SMALL_R:
            for counts in (None, (0,), (R_cap - 1,)):
                yield "narrow", C1, R_cap, counts
    for C1 in WIDE_C1:
        for R_cap, counts, batch in wide_rows(C1):
            if batch == 1:
                yield "wide", C1, R_cap, counts


IMG_W, IMG_H = 160.0, 120.0
CASCADE_WEIGHTS = ((10.0, 10.0, 5.0, 5.0), (20.0, 20.0, 10.0, 10.0), (30.0, 30.0, 15.0, 15.0))


def hostile_boxes(rows: int, seed: int) -> torch.Tensor:
    """[rows, 4] on a 160 x 120 image, kind j mod 6: plain / zero width and height / wholly outside (left and above) / plain touching the
    origin / zero height only / wholly outside (right and below)."""
    g = torch.Generator().manual_seed(seed)
    c = torch.rand((rows, 2), generator=g) * torch.tensor([IMG_W, IMG_H])
    half = torch.rand((rows, 2), generator=g) * 30 + 2
    b = torch.cat([c - half, c + half], dim=1)
    for r in range(rows):
        kind = r % 6
        if kind == 1:
            b[r, 2:] = b[r, :2]
        elif kind == 2:
            b[r] = torch.tensor([-300.5, -200.25, -250.0, -150.75])
        elif kind == 3:
            b[r, :2] = 0
        elif kind == 4:
            b[r, 3] = b[r, 1]
        elif kind == 5:
            b[r] = torch.tensor([IMG_W + 400.0, IMG_H + 300.0, IMG_W + 460.5, IMG_H + 333.25])
    return b.contiguous()


TAIL_K = (16, 1024, 1040)        # one lane / the production width / a second trip of the lane loop
TAIL_BIAS = (0.5, -0.5, 0.2, 20.0)


def tail_layer(K: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """bbox_pred.2 at width K as the OIHW weight of a 1x1 layer over the next multiple of 32 channels (what `ops.Conv` packs) and its
    bias.  The columns beyond K are NOT zero: a kernel that read past `hb_dim` would show.  Row 3 is scaled so that, with the bias of
    20 and wh = 5, dh = 4 + N(0, 0.2): about a quarter of the rows pass the exponent clamp of 4.135, the rest stay just below it."""
    g = torch.Generator().manual_seed(K)
    Kp = (K + 31) // 32 * 32
    w = torch.randn((4, Kp), generator=g) * (1.0 / math.sqrt(K / 2))
    return w.reshape(4, Kp, 1, 1).contiguous(), torch.tensor(TAIL_BIAS)


@functools.lru_cache(maxsize=None)
def tail_case(K: int, rows: int, stage: int, clip: bool) -> Dict[str, object]:
    """The BoxTail on `rows` rows: hb (ReLU'd: non-negative with exact zeros, row 2 all zero), hostile boxes, float64 deltas and boxes,
    their bounds and the fp32 emulation (16 inputs per lane and trip, butterfly, bias)."""
    w4, bias = tail_layer(K)
    w = w4.reshape(4, -1)[:, :K]
    g = torch.Generator().manual_seed(K + rows)
    hb = torch.randn((rows, K), generator=g).clamp(min=0)
    if rows > 2:
        hb[2] = 0
    boxes = hostile_boxes(rows, K + 3 * rows)
    weights = CASCADE_WEIGHTS[stage]
    d64 = hb.double() @ w.double().t() + bias.double()
    b_d = linear_bound(hb.double().abs() @ w.double().abs().t(), bias[None, :], 16, K)
    d32 = lane_dot(hb, w.t().contiguous(), 16) + bias
    return dict(K=K, hb=hb.contiguous(), w4=w4, bias=bias, boxes=boxes, weights=weights, clip=clip, d64=d64, b_d=b_d, d32=d32,
                box64=box_transform(d64, boxes, weights, clip, IMG_W, IMG_H, F64), b_box=box_bounds(d64, b_d, boxes, weights),
                box32=box_transform(d32, boxes, weights, clip, IMG_W, IMG_H, F32))


def tail_table():
    """(order, C1, R_cap, counts, batch, K, with deltas_out, clip, form): the row tables at C1 = 21 and 33, the three widths, deltas_out
    given and None, clip on and off; the cascade's three forms (and stage weights) in turn."""
    i = 0
    for order, C1, table in (("narrow", 21, NARROW_ROWS), ("wide", 33, WIDE_ROWS)):
        for R_cap, counts, batch in table:
            for K in TAIL_K:
                for with_deltas in (True, False):
                    for clip in (True, False):
                        yield order, C1, R_cap, counts, batch, K, with_deltas, clip, FORMS[i % 3]
                        i += 1


@functools.lru_cache(maxsize=None)
def deltas_case(R_cap: int, batch: int, ld: int, clip: bool) -> Dict[str, object]:
    """`apply_deltas`: deltas [rows, ld] whose columns beyond 4 hold other numbers; some dw far past the clamp, some very negative."""
    rows = R_cap * batch
    g = torch.Generator().manual_seed(R_cap * 10 + ld)
    d = torch.randn((rows, ld), generator=g) * 3
    d[0::4, 2] = 100.0
    d[1::4, 3] = -40.0
    boxes = hostile_boxes(rows, R_cap + ld)
    weights = CASCADE_WEIGHTS[0]
    z = torch.zeros((rows, 4), dtype=F64)
    return dict(d=d.contiguous(), boxes=boxes, weights=weights, box64=box_transform(d[:, :4], boxes, weights, clip, IMG_W, IMG_H, F64),
                b_box=box_bounds(d[:, :4], z, boxes, weights), box32=box_transform(d[:, :4], boxes, weights, clip, IMG_W, IMG_H, F32))


def fusion(acc: torch.Tensor, inv: float, ps: torch.Tensor, dt) -> torch.Tensor:
    """`cascade_scores`: sqrt(acc * inv_stages * ps)."""
    return torch.sqrt(acc.to(dt) * torch.tensor(inv, dtype=dt) * ps.to(dt)[:, None])


@functools.lru_cache(maxsize=None)
def fusion_case(R_cap: int, C1: int = 21) -> Dict[str, object]:
    """`cascade_scores` on [R_cap, C1] accumulated probabilities in (0, 3), one of them 1e-30: two products and a root, 2 U relative."""
    g = torch.Generator().manual_seed(R_cap)
    acc = torch.rand((R_cap, C1), generator=g) * 3
    acc[0, 0] = 1e-30
    ps = proposal_scores(R_cap, R_cap + 1)
    ref = fusion(acc, INV3, ps, F64)
    return dict(acc=acc, ps=ps, ref=ref, emu=fusion(acc, INV3, ps, F32), bound=HEAD * 2 * U * ref + TINY)


# ------------------------------------------------------------------------------------------------
# detector_postprocess: fp32 on the CPU, compared exactly
# ------------------------------------------------------------------------------------------------
POST_SCALES = ((1.0, 1.0), (0.75, 1.3333334), (2.5, 0.4))
POST_CAPS = (1, 16, 512)
POST_IN = (80.0, 60.0)             # the frame the detections were made on (w, h)


def post_inputs(cap: int, batch: int, sx: float, sy: float, seed: int, all_dropped: bool = False):
    """boxes [batch * cap, 4], scores, classes, remap, (out_w, out_h).  Detection j is of kind j mod 5: plain / empty only after scaling
    and clipping (beyond the output's right border once scaled) / on the output's border / zero width / plain.  The output frame is a
    little SMALLER than the scaled input frame, so that the clip really cuts."""
    n = cap * batch
    g = torch.Generator().manual_seed(seed)
    W, H = POST_IN
    out_w, out_h = float(math.floor(W * sx * 0.9)), float(math.floor(H * sy * 0.9))
    c = torch.rand((n, 2), generator=g) * torch.tensor([W * 0.85, H * 0.85])
    half = torch.rand((n, 2), generator=g) * 8 + 0.5
    b = torch.cat([(c - half).clamp(min=0), c + half], dim=1)
    s32 = torch.tensor([sx, sy], dtype=F32)
    for r in range(n):
        kind = r % 5
        if all_dropped or kind == 1:
            b[r, 0], b[r, 2] = W * 0.93, W * 0.99            # inside the input frame, right of the output frame after the scale
        elif kind == 2:
            b[r, 0], b[r, 1] = 0.0, 0.0
            b[r, 2:] = torch.tensor([out_w, out_h]) / s32 * 1.5      # clipped onto the border
        elif kind == 3:
            b[r, 2] = b[r, 0]
    scores = torch.rand((n,), generator=g)
    classes = torch.randint(0, 1203, (n,), generator=g, dtype=torch.int32)
    remap = torch.randint(0, cap, (n,), generator=g, dtype=torch.int32)
    return b.contiguous(), scores, classes, remap, (out_w, out_h)


def postprocess(boxes, scores, classes, count: Optional[int], cap: int, sx: float, sy: float, out_w: float, out_h: float, remap=None):
    """One scene in fp32: scale (one multiplication per coordinate by the fp32 factor), clip, keep the boxes with positive width and height,
    in order.  -> boxes [n, 4], scores [n], classes [n], source indices [n] (through `remap` when given), n."""
    D = cap if count is None else min(count, cap)
    s = torch.tensor([sx, sy, sx, sy], dtype=F32)
    hi = torch.tensor([out_w, out_h, out_w, out_h], dtype=F32)
    b = torch.minimum(torch.maximum(boxes[:D].float() * s, torch.zeros(4)), hi)
    keep = ((b[:, 2] - b[:, 0]) > 0) & ((b[:, 3] - b[:, 1]) > 0)
    idx = keep.nonzero().flatten()
    src = idx.int() if remap is None else remap[:D][idx]
    return b[idx], scores[:D][idx], classes[:D][idx], src, int(idx.numel())


# ------------------------------------------------------------------------------------------------
# mask predictor
# ------------------------------------------------------------------------------------------------
MASK_C = (4, 256, 260)             # one lane / one full trip of the channel loop / a second trip
MASK_BIAS = -0.375
MASK_STRIDE_UNITS = 8193           # x 4 rows of 4 channels: 32772 rows > 8192 workgroups x 4 waves, a second grid-stride pass


@functools.lru_cache(maxsize=None)
def mask_case(C: int, unit_rows: int, units: int) -> Dict[str, object]:
    """x [units * unit_rows, C], w [C] and the float64 logit / probability, bounds and the fp32 emulation of the predictor."""
    rows = units * unit_rows
    g = torch.Generator().manual_seed(C * 7 + unit_rows + units)
    x = torch.randn((rows, C), generator=g).clamp(min=0) * 2            # the deconvolution's ReLU'd output
    x[0] = 0
    w = torch.randn((C,), generator=g) * (3.0 / math.sqrt(C))
    bias = torch.tensor([MASK_BIAS])
    s64 = x.double() @ w.double() + MASK_BIAS
    b_s = linear_bound(x.double().abs() @ w.double().abs(), bias, 4, C)
    p64 = sigmoid(s64)
    s32 = lane_dot(x, w[:, None].contiguous(), 4, grouped=True)[:, 0] + bias
    return dict(x=x.contiguous(), w=w.contiguous(), p64=p64, b_p=prob_bound(s64, b_s, p64), p32=sigmoid(s32), s64=s64)


def mask_table():
    """(C, unit_rows, units, count, with out_units)."""
    for C in MASK_C:
        for unit_rows in (4, 784):
            for units in (1, 3):
                for count in (None, 0, units - 1):
                    for scatter in (False, True):
                        yield C, unit_rows, units, count, scatter
    yield 4, 4, MASK_STRIDE_UNITS, None, False
    yield 4, 4, MASK_STRIDE_UNITS, MASK_STRIDE_UNITS - 1, True


def scatter_units(units: int) -> torch.Tensor:
    """A non-identity injection of `units` compact units into units + 2 output units: the list reversed, output units 0 and 1 unused."""
    return torch.arange(units + 1, 1, -1).int()
