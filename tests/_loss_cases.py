"""CPU side of test_loss_launches_gpu.py: float64 references, derived per-element bounds, CPU fp32 emulations and the input builders of
the training loss and target kernels (csrc/train_losses.hip).  Plain torch / numpy; nothing here touches a GPU.

Every kernel's arithmetic is written ONCE below, in the kernel's own operation order, over a number type:

  * fp32 tensors: the yardstick -- what a correct fp32 implementation in the kernel's order computes (`torch` fp32; the device may fuse
    a multiply-add, which only removes a rounding);
  * `E` values: the float64 reference WITH its bound.  An `E` carries a float64 value v and a first-order bound e on the error an fp32
    evaluation of the same expression makes.  Every operator propagates e through the float64 partial derivatives and adds
    U * |result| for its own fp32 rounding (U = 2^-24): a + b -> e_a + e_b + U |a + b| (so a cancellation is charged with the
    magnitude of its operands' errors: the differences inside `diou` and `dfrac`, `tx - sx` of the box targets);  a b -> |a| e_b +
    |b| e_a + U |a b|;  a / b -> e_a / |b| + |a / b| e_b / |b| + U |a / b|;  min / max are 1-Lipschitz.  Operations that happen to be
    exact (a product by 0.5, 1 - p for p >= 0.5) are charged all the same: the bound is an upper count.

Device `expf`, `logf`, `log1pf`, `powf` and `sqrtf` are allowed 4 ulp = 8 U relative per call: the ROCm installation carries no
statement of their accuracy, so the issue's default applies.  The references read the fp32 inputs and take the kernels' constants at
their fp32 values (`sigmoid_clamp`, `1.f - clampv`, the quotients c_pos / c_neg / c_reg, `1.f / B`): they are inputs, not results.

Each family's bound is HEAD * e + TINY with HEAD = 2, the project's usual head-room, fixed before any GPU run: the fp32 emulation
stays at or under half of it on every case (test_loss_launches_gpu.py::test_fp32_emulation_stays_inside_half_of_every_bound).  TINY,
the smallest normal fp32, is the absolute floor (a sigmoid of -88 is subnormal).  A loss scalar is a double sum of fp32 terms: the sum
of the terms' bounds plus one fp32 rounding of the result.

DECISIONS.  Where the float64 and the fp32 value of a comparand can fall on different sides of a threshold the element is excluded,
counted and printed (`band_*` masks): the sigmoid against clampv, 1 - clampv and ignore_high_fp, within HEAD times the sigmoid's own
bound; e against 0 when beta < 1e-5; the heat map's `< 1e-4 -> 0` cut.  Planted threshold inputs lie at least 64 ulp on a known side
and are never excluded.  At |e| = beta smooth-L1 and its gradient are continuous: no exclusion, the quadratic branch's bound is used
on both sides where |e| is within the bound of beta.  Ties of min / max are decisions on fp32 values too: planted ties are exact in
both precisions (a power-of-two scale), and the builders keep every other prediction at least 1e-3 (relative) away from its target."""
import functools
import math
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from _launch_cases import SENTINEL, U          # noqa: F401  (re-exported)

HEAD = 2.0
TINY = 2.0 ** -126
ULP4 = 8 * U                          # 4 ulp of a device math call, relative
F32, F64 = torch.float32, torch.float64
I32_SENTINEL = -77777
BAND_CAP_SHARE, BAND_CAP = 1e-4, 16   # at most this share of a tensor's elements / this many may fall into a decision band


def f32(x: float) -> float:
    """x rounded to fp32, as a Python float."""
    return float(np.float32(x))


# ------------------------------------------------------------------------------------------------
# values with an error bound
# ------------------------------------------------------------------------------------------------
class E:
    """float64 value `v` and first-order fp32 error bound `e` (module docstring)."""
    __slots__ = ("v", "e")

    def __init__(self, v, e=None):
        self.v = v if torch.is_tensor(v) else torch.tensor(float(v), dtype=F64)
        self.v = self.v.to(F64)
        self.e = torch.zeros_like(self.v) if e is None else e

    @staticmethod
    def of(x) -> "E":
        return x if isinstance(x, E) else E(x)

    def _r(self, v, e):
        return E(v, e + U * v.abs())

    def __add__(self, o):
        o = E.of(o)
        return self._r(self.v + o.v, self.e + o.e)

    __radd__ = __add__

    def __sub__(self, o):
        o = E.of(o)
        return self._r(self.v - o.v, self.e + o.e)

    def __rsub__(self, o):
        return E.of(o) - self

    def __mul__(self, o):
        o = E.of(o)
        return self._r(self.v * o.v, self.v.abs() * o.e + o.v.abs() * self.e)

    __rmul__ = __mul__

    def __truediv__(self, o):
        o = E.of(o)
        v = self.v / o.v
        return self._r(v, self.e / o.v.abs() + v.abs() * o.e / o.v.abs())

    def __rtruediv__(self, o):
        return E.of(o) / self

    def __neg__(self):
        return E(-self.v, self.e)

    def __getitem__(self, i):
        return E(self.v[i], self.e[i])

    def sum(self):
        """A double sum of fp32 terms: no rounding of its own."""
        return E(self.v.sum(), self.e.sum())


def val(x):
    return x.v if isinstance(x, E) else x


def fwhere(m, a, b):
    if isinstance(a, E) or isinstance(b, E):
        a, b = E.of(a), E.of(b)
        return E(torch.where(m, a.v, b.v), torch.where(m, a.e, b.e))
    return torch.where(m, a, b)


def fstack(xs, dim):
    if isinstance(xs[0], E):
        return E(torch.stack([x.v for x in xs], dim), torch.stack([x.e for x in xs], dim))
    return torch.stack(xs, dim)


def fmin(a, b):
    if isinstance(a, E) or isinstance(b, E):
        a, b = E.of(a), E.of(b)
        return E(torch.minimum(a.v, b.v), torch.maximum(a.e, b.e))
    return torch.minimum(a, b)


def fmax(a, b):
    if isinstance(a, E) or isinstance(b, E):
        a, b = E.of(a), E.of(b)
        return E(torch.maximum(a.v, b.v), torch.maximum(a.e, b.e))
    return torch.maximum(a, b)


def fabs(a):
    return E(a.v.abs(), a.e) if isinstance(a, E) else a.abs()


def flog(a):
    if isinstance(a, E):
        v = torch.log(a.v)
        return E(v, a.e / a.v.abs() + ULP4 * v.abs())
    return torch.log(a)


def flog1p(a):
    if isinstance(a, E):
        v = torch.log1p(a.v)
        return E(v, a.e / (1 + a.v) + ULP4 * v.abs())
    return torch.log1p(a)


def fexp(a):
    if isinstance(a, E):
        v = torch.exp(a.v)
        return E(v, v * a.e + ULP4 * v)
    return torch.exp(a)


def fpow(a, g: float):
    """a ** g for a >= 0 and a constant g > 0."""
    if isinstance(a, E):
        v = a.v ** g
        return E(v, torch.where(a.v > 0, abs(g) * v / a.v.clamp(min=1e-300) * a.e, torch.zeros_like(v)) + ULP4 * v)
    return torch.pow(a, g)


def fsigmoid(x):
    """`eod_sigmoid_precise`: 1 / (1 + expf(-x)).  The reference evaluates it without overflow; its bound is s ((1 - s) (e_x + 4 ulp
    of expf) + 2 U): expf's error reaches s through e / (1 + e) = 1 - s, then 1 + e and the division round."""
    if isinstance(x, E):
        v, c = torch.sigmoid(x.v), torch.sigmoid(-x.v)
        return E(v, v * (c * (x.e + ULP4) + 2 * U))
    return 1.0 / (1.0 + torch.exp(-x))


def num(t: torch.Tensor, mode: str):
    """An input tensor as the number type of `mode`: "f32" (the emulation) or "ref" (float64 with bounds)."""
    return t.to(F32) if mode == "f32" else E(t.to(F64))


def bound(x: E) -> torch.Tensor:
    return HEAD * x.e + TINY


def share(err: torch.Tensor, bnd: torch.Tensor) -> torch.Tensor:
    """err / bound; where the bound is 0 (an exact result is expected): 0 for no error, inf for any."""
    return torch.where(bnd > 0, err / bnd.clamp(min=1e-300), torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))


# ------------------------------------------------------------------------------------------------
# eod_centernet_loss
# ------------------------------------------------------------------------------------------------
PARAM_SETS = {
    "default": dict(alpha=0.25, beta=4.0, gamma=2.0, sigmoid_clamp=1e-4, ignore_high_fp=0.85, pos_weight=0.5, neg_weight=0.5, reg_weight=1.0),
    "noalpha": dict(alpha=-1.0, beta=4.0, gamma=2.0, sigmoid_clamp=1e-4, ignore_high_fp=0.0, pos_weight=0.5, neg_weight=0.5, reg_weight=1.0),
}
LEVEL_SCALES = (1.0, 0.8, 1.3, 2.0, 0.5, 1.7, 0.6, 2.5)          # distinct; 1, 2 and 0.5 take the exact ties


def cn_constants(prm: Dict[str, float], n_pos: int, n_reg: int, world: int = 1) -> Dict[str, float]:
    """The kernel's constants at their fp32 values: the normalisers max(float32(count / world), 1), the three quotients, clampv,
    1.f - clampv, ignore_high_fp, an = 1 - alpha (or 1), ap = alpha (or 1)."""
    one = np.float32(1.0)
    npa = max(np.float32(np.float64(n_pos) / np.float64(world)), one)
    rn = max(np.float32(np.float64(n_reg) / np.float64(world)), one)
    a = np.float32(prm["alpha"])
    cl = np.float32(prm["sigmoid_clamp"])
    return dict(num_pos_avg=float(npa), reg_norm=float(rn), c_pos=float(np.float32(prm["pos_weight"]) / npa),
                c_neg=float(np.float32(prm["neg_weight"]) / npa), c_reg=float(np.float32(prm["reg_weight"]) / rn),
                cl=float(cl), hi=float(one - cl), ign=f32(prm["ignore_high_fp"]), an=float(one - a) if a >= 0 else 1.0,
                ap=float(a) if a >= 0 else 1.0, beta=f32(prm["beta"]), gamma=f32(prm["gamma"]))


def level_of(lv_off: Sequence[int], P: int) -> torch.Tensor:
    """The level of every position: the l with lv_off[l] <= i < lv_off[l + 1] (an empty level holds none)."""
    return torch.bucketize(torch.arange(P), torch.tensor(list(lv_off[1:-1]), dtype=torch.long), right=True)


def _clamped(s, k):
    """(p, inside): p = min(max(s, clampv), 1 - clampv)."""
    sv = val(s)
    lo_c = torch.full_like(sv, k["cl"])
    hi_c = torch.full_like(sv, k["hi"])
    if isinstance(s, E):
        lo_c, hi_c = E(lo_c), E(hi_c)
    return fwhere(sv < k["cl"], lo_c, fwhere(sv > k["hi"], hi_c, s)), (sv >= k["cl"]) & (sv <= k["hi"])


TIE_VALUE = 0.5          # the self-check sets 1.0 for a moment to show that the bounds tell the two apart


def _tie(a, b, less: bool, like):
    """`half_on_tie` on values: a decision, hence an exact constant."""
    av, bv = val(a), val(b)
    w = torch.where(av == bv, TIE_VALUE, torch.where((av < bv) if less else (av > bv), 1.0, 0.0)).to(av.dtype)
    return E(w) if isinstance(like, E) else w


def cn_dense(head: torch.Tensor, heat: torch.Tensor, reg_t: torch.Tensor, sc_rows: torch.Tensor, k: Dict[str, float], mode: str):
    """`centernet_loss_dense_kernel` over every position -> d0 [P] (the negative term's gradient), g [P, 4], the per-position terms of
    the negative and the regression sum, and the sigmoid (for the bands)."""
    z = num(head[:, 0], mode)
    s = fsigmoid(z)
    p, inside = _clamped(s, k)
    nw = fpow(1.0 - num(heat, mode), k["beta"])
    keep = (val(p) < k["ign"]) if k["ign"] > 0 else torch.ones_like(inside)
    q = 1.0 - p
    l1p, pg = flog(q), fpow(p, k["gamma"])
    neg_raw = l1p * pg * nw
    neg_term = fwhere(keep, neg_raw, 0.0 * neg_raw)
    dp = ((-pg) / q + (k["gamma"] * fpow(p, k["gamma"] - 1.0)) * l1p) * nw
    kn = float(np.float32(-k["an"]) * np.float32(k["c_neg"]))
    gz = kn * dp * s * (1.0 - s)
    d0 = fwhere(keep & inside, gz, 0.0 * gz)
    # ---- GIoU
    has = reg_t.max(dim=1)[0] >= 0
    safe = torch.where(has[:, None], reg_t, torch.ones_like(reg_t))
    tl, tt, tr, tb = (num(safe[:, j], mode) for j in range(4))
    sc = num(sc_rows, mode)
    r = [num(head[:, 1 + j], mode) * sc for j in range(4)]
    pl, pt, pr, pb = (fwhere(val(x) > 0, x, 0.0 * x) for x in r)
    t_area, p_area = (tl + tr) * (tt + tb), (pl + pr) * (pt + pb)
    wi, hi_ = fmin(pl, tl) + fmin(pr, tr), fmin(pb, tb) + fmin(pt, tt)
    gw, gh = fmax(pl, tl) + fmax(pr, tr), fmax(pb, tb) + fmax(pt, tt)
    ac, ai = gw * gh, wi * hi_
    au = t_area + p_area - ai
    iou = (ai + 1.0) / (au + 1.0)
    giou = iou - (ac - au) / ac
    loc_term = fwhere(has, 1.0 - giou, 0.0 * giou)
    dpa = (pt + pb, pl + pr, pt + pb, pl + pr)
    dai = (_tie(pl, tl, True, z) * hi_, _tie(pt, tt, True, z) * wi, _tie(pr, tr, True, z) * hi_, _tie(pb, tb, True, z) * wi)
    dac = (_tie(pl, tl, False, z) * gh, _tie(pt, tt, False, z) * gw, _tie(pr, tr, False, z) * gh, _tie(pb, tb, False, z) * gw)
    g = []
    for j in range(4):
        dau = dpa[j] - dai[j]
        diou = (dai[j] * (au + 1.0) - (ai + 1.0) * dau) / ((au + 1.0) * (au + 1.0))
        dfrac = (dau * ac - au * dac[j]) / (ac * ac)
        dg = diou + dfrac
        gj = (-k["c_reg"]) * dg * sc
        g.append(fwhere(has & (val(r[j]) > 0), gj, 0.0 * gj))
    return dict(d0=d0, g=fstack(g, 1), neg_term=neg_term, neg_raw=neg_raw, loc_term=loc_term, s=s, has=has)


def cn_pos(head: torch.Tensor, idx: torch.Tensor, k: Dict[str, float], mode: str):
    """`centernet_loss_pos_kernel` on the listed (valid) positions `idx` -> the term of the positive sum and the gradient each adds."""
    s = fsigmoid(num(head[idx, 0], mode))
    p, inside = _clamped(s, k)
    lp, q = flog(p), fpow(1.0 - p, k["gamma"])
    term = lp * q
    dp = q / p - (k["gamma"] * lp) * fpow(1.0 - p, k["gamma"] - 1.0)
    kp = float(np.float32(-k["ap"]) * np.float32(k["c_pos"]))
    g = kp * dp * s * (1.0 - s)
    return dict(term=term, g=fwhere(inside, g, 0.0 * g), s=s)


def _scalar(c: float, total, mode: str):
    """(float)((double)c * sum): the sum of the terms' bounds plus one rounding of the result."""
    if mode == "f32":
        return (c * total.double().sum()).to(F32)
    t = total.sum()
    v = c * t.v
    return E(v, abs(c) * t.e + U * v.abs())


def cn_loss(head, heat, reg_t, sc_rows, pos_list: torch.Tensor, k: Dict[str, float], mode: str):
    """The whole entry point -> d_head[:, 0:5] (d0 with the positives added, in list order; g) and the three losses.  `pos_list`: the
    list as the kernel reads it (entries < 0 or >= P are skipped)."""
    P = head.shape[0]
    d = cn_dense(head, heat, reg_t, sc_rows, k, mode)
    valid = pos_list[(pos_list >= 0) & (pos_list < P)].long()
    uniq, mult = torch.unique(valid, return_counts=True)
    pu = cn_pos(head, uniq, k, mode)
    d0 = d["d0"]
    acc = d0[uniq]
    for t in range(int(mult.max()) if mult.numel() else 0):
        acc = fwhere(mult > t, acc + pu["g"], acc)
    if isinstance(d0, E):
        v, e = d0.v.clone(), d0.e.clone()
        v[uniq], e[uniq] = acc.v, acc.e
        full = E(v, e)
        pos_terms = E(pu["term"].v * mult, pu["term"].e * mult)
    else:
        full = d0.clone()
        full[uniq] = acc
        pos_terms = pu["term"].double() * mult
    losses = [_scalar(k["c_reg"], d["loc_term"], mode),
              _scalar(-float(np.float32(k["ap"]) * np.float32(k["c_pos"])), pos_terms, mode),
              _scalar(-float(np.float32(k["an"]) * np.float32(k["c_neg"])), d["neg_term"], mode)]
    return dict(d0_neg=d0, d0=full, g=d["g"], losses=fstack(losses, 0), s=d["s"], has=d["has"], neg_raw=d["neg_raw"], uniq=uniq, mult=mult, pos_g=pu["g"])


def sigmoid_band(s: E, k: Dict[str, float]) -> torch.Tensor:
    """Positions whose float64 sigmoid is within HEAD times its own fp32 bound of clampv, 1 - clampv or ignore_high_fp."""
    m = torch.zeros_like(s.v, dtype=torch.bool)
    for thr in (k["cl"], k["hi"]) + ((k["ign"],) if k["ign"] > 0 else ()):
        m |= (s.v - thr).abs() <= HEAD * s.e
    return m


def band_ok(n_excluded: int, n: int) -> bool:
    return n_excluded <= min(BAND_CAP, BAND_CAP_SHARE * n) or n_excluded == 0


def planted_logits(k: Dict[str, float]) -> List[float]:
    """fp32 logits whose float64 sigmoid lies at least 64 fp32 ulps below and above clampv, 1 - clampv and ignore_high_fp."""
    out = []
    for thr in (k["cl"], k["hi"]) + ((k["ign"],) if k["ign"] > 0 else ()):
        ulp = float(np.spacing(np.float32(thr)))
        z0 = math.log(thr / (1 - thr))
        dz = max(128 * ulp / (thr * (1 - thr)), 64 * float(np.spacing(np.float32(abs(z0)))))
        for sgn in (-1.0, 1.0):
            z = f32(z0 + sgn * dz)
            sv = 1.0 / (1.0 + math.exp(-z))
            assert (sv - thr) * sgn >= 64 * ulp, (thr, z, sv)
            out.append(z)
    return out


def level_offsets(P: int, L: int) -> List[int]:
    """Ascending offsets of L levels over P positions, level 2 empty when there are five or more."""
    off = [P * l // L for l in range(L + 1)]
    if L >= 5:
        off[2] = off[3]
    return off


#        P, head_stride, levels, n_pos
CN_SHAPES = ((1, 5, 1, 1), (255, 8, 5, 0), (256, 9, 8, 255), (257, 5, 5, 256), (131072, 8, 8, 257), (131073, 9, 5, 1000))
SPECIAL_LOGITS = (0.0, 1e-3, -1e-3, 20.0, -20.0, 100.0, -100.0)


@functools.lru_cache(maxsize=None)
def cn_inputs(P: int, stride: int, L: int, n_pos: int, pset: str) -> Dict[str, object]:
    """Inputs of one `eod_centernet_loss` call (module docstring of the test for what each row kind is)."""
    prm = PARAM_SETS[pset]
    g = torch.Generator().manual_seed(P * 31 + stride * 7 + L)
    off = level_offsets(P, L)
    scales = LEVEL_SCALES[:L]
    lev = level_of(off, P)
    sc_rows = torch.tensor(scales)[lev]
    i = torch.arange(P)
    k0 = cn_constants(prm, 1, 1)
    # ---- logits: the special values and the planted threshold neighbours on rows i mod 19, random elsewhere
    special = list(SPECIAL_LOGITS) + planted_logits(k0)
    logits = torch.randn((P,), generator=g) * 3
    kind = i % 19
    for j, v in enumerate(special):
        logits[kind == j] = v
    planted = (kind >= len(SPECIAL_LOGITS)) & (kind < len(special))
    # ---- heat: 0, 1, 1e-4 and rand ** 8 on rows i mod 7
    heat = torch.rand((P,), generator=g) ** 8
    heat[i % 7 == 0], heat[i % 7 == 1], heat[i % 7 == 2] = 0.0, 1.0, 1e-4
    # ---- regression rows
    rk = (i * 7 + 3) % 16
    first = torch.tensor([o for o in off[1:-1] if o < P], dtype=torch.long)
    edge = torch.zeros(P, dtype=torch.bool)
    edge[first] = True
    edge[(first - 1).clamp(min=0)] = True                 # the rows on both sides of every level boundary regress
    if P > 1:
        rk[edge] = 8
    pow2 = (sc_rows == 1.0) | (sc_rows == 2.0) | (sc_rows == 0.5)
    rk[((rk == 12) | (rk == 13)) & ~pow2] = 9
    tgt = torch.rand((P, 4), generator=g) * 70 + 0.5
    pred = torch.rand((P, 4), generator=g) * 60 + 0.25
    raw = pred / sc_rows[:, None]
    u = torch.rand((P, 4), generator=g)
    raw = torch.where(u < 0.05, torch.zeros_like(raw), torch.where(u < 0.15, -raw, raw))        # raw == 0 and raw < 0
    raw[edge] = raw[edge].abs() + 0.125                     # ... with four open predictions: a neighbouring level's scale shows
    tgt[rk == 11] = torch.tensor([-1.0, 5.0, 3.0, 2.0])
    raw[rk == 11] = raw[rk == 11].abs() + 0.125
    axis = (i // 16) % 4
    exact = tgt / sc_rows[:, None]                          # exact where the scale is a power of two
    for a in range(4):
        m = (rk == 12) & (axis == a)
        raw[m, a] = exact[m, a]
    raw[rk == 13] = exact[rk == 13]
    raw[rk == 14] = torch.where(u[rk == 14] < 0.5, torch.zeros(()), -raw[rk == 14].abs() - 0.5)
    tie = torch.zeros((P, 4), dtype=torch.bool)
    for a in range(4):
        tie[:, a] = ((rk == 12) & (axis == a)) | (rk == 13)
    # keep every other prediction away from its target (a tie is a decision on fp32 values)
    r64 = raw.double() * sc_rows.double()[:, None]
    near = ((r64 - tgt.double()).abs() < 1e-3 * tgt.double().abs()) & ~tie
    raw = torch.where(near, raw * 1.25, raw)
    reg_t = torch.where((rk >= 8)[:, None], tgt, torch.full_like(tgt, -1e8))
    head = torch.randn((P, stride), generator=g)
    head[:, 0], head[:, 1:5] = logits, raw
    # ---- the positives' list
    if n_pos == 0:
        pos = torch.zeros((0,), dtype=torch.int32)
    else:
        pos = torch.randint(0, P, (n_pos,), generator=g).int() if n_pos > P else torch.randperm(P, generator=g)[:n_pos].int()
        if n_pos >= 8:
            pos[1] = pos[0]                                  # listed twice
            pos[3], pos[4] = pos[2], pos[2]                  # listed three times
            pos[5], pos[6] = -1, P                           # skipped
    return dict(P=P, stride=stride, L=L, off=off, scales=scales, sc_rows=sc_rows, head=head.contiguous(), heat=heat, reg_t=reg_t.contiguous(),
                pos=pos, prm=prm, pset=pset, planted=planted, tie=tie, rk=rk, n_reg=int((rk >= 8).sum()))


def cn_reference(c, pos_list: torch.Tensor, k: Dict[str, float]):
    """(float64 reference with bounds, fp32 emulation) of the call on inputs `c` with list `pos_list` and constants `k`."""
    return (cn_loss(c["head"], c["heat"], c["reg_t"], c["sc_rows"], pos_list, k, "ref"),
            cn_loss(c["head"], c["heat"], c["reg_t"], c["sc_rows"], pos_list, k, "f32"))


@functools.lru_cache(maxsize=None)
def cn_case(P: int, stride: int, L: int, n_pos: int, pset: str):
    c = cn_inputs(P, stride, L, n_pos, pset)
    n_valid = int(((c["pos"] >= 0) & (c["pos"] < P)).sum())
    k = cn_constants(c["prm"], n_valid, c["n_reg"])
    ref, emu = cn_reference(c, c["pos"], k)
    ref0, emu0 = cn_reference(c, c["pos"][:0], k)           # no list: the negative term's store alone
    return dict(c, k=k, ref=ref, emu=emu, ref0=ref0, emu0=emu0)


def cn_table():
    for shape in CN_SHAPES:
        for pset in PARAM_SETS:
            yield shape + (pset,)


# ------------------------------------------------------------------------------------------------
# eod_fast_rcnn_loss
# ------------------------------------------------------------------------------------------------
RC_LOGITS = (0.0, 1e-3, -1e-3, 20.0, -20.0, 88.0, -88.0, 100.0, -100.0, 1e4, -1e4)
#          B, C, ld, class weight, gt kind, beta, box weights
RC_TABLE = ((1, 1, 2, "none", "mixed", 0.0, 0), (2, 20, 21, "mask", "mixed", 0.3, 1), (511, 20, 24, "frac", "mixed", 1.0, 0),
            (512, 255, 256, "zero", "mixed", 0.0, 1), (513, 256, 257, "none", "all_fg", 0.3, 0), (2, 257, 260, "frac", "all_bg", 1.0, 1),
            (513, 1203, 1216, "mask", "mixed", 0.0, 0), (511, 2047, 2048, "none", "mixed", 0.3, 1), (512, 20, 21, "frac", "mixed", 0.0, 1),
            (513, 20, 24, "mask", "all_fg", 1.0, 0))
BOX_WEIGHTS = ((10.0, 10.0, 5.0, 5.0), (30.0, 30.0, 15.0, 15.0))


def rc_loss(scores, deltas, prop, gtb, gt, cw: Optional[torch.Tensor], C: int, weights, beta: float, mode: str):
    """`fast_rcnn_loss_rows_kernel` + `fast_rcnn_loss_sum_kernel` -> d_scores [B, ld], d_deltas [B, 4], losses [2], e [B, 4]."""
    B, ld = scores.shape
    inv_b = float(np.float32(1.0) / np.float32(B))
    beta = f32(beta)
    v = num(scores[:, :C], mode)
    y = (torch.arange(C)[None, :] == gt[:, None].long())
    yv = num(y.to(F32), mode)
    w = num((torch.ones(C) if cw is None else cw)[None, :].expand(B, C).contiguous(), mode)
    zero = 0.0 * v
    soft = flog1p(fexp(-fabs(v)))
    term = w * ((1.0 - yv) * v + soft + fwhere(val(v) < 0, -v, zero))
    dz = w * (fsigmoid(v) - yv) * inv_b
    pad = torch.zeros((B, ld - C), dtype=F32 if mode == "f32" else F64)
    if mode == "f32":
        d_scores = torch.cat([dz, pad], 1)
        loss_cls = (term.double().sum() / B).to(F32)
    else:
        d_scores = E(torch.cat([dz.v, pad], 1), torch.cat([dz.e, pad], 1))
        t = term.sum()
        loss_cls = E(t.v / B, t.e / B + U * (t.v / B).abs())
    # ---- the box term of the foreground rows
    fg = (gt >= 0) & (gt < C)
    s = [num(prop[:, j], mode) for j in range(4)]
    t_ = [num(gtb[:, j], mode) for j in range(4)]
    sw, sh = s[2] - s[0], s[3] - s[1]
    sx, sy = s[0] + 0.5 * sw, s[1] + 0.5 * sh
    tw, th = t_[2] - t_[0], t_[3] - t_[1]
    tx, ty = t_[0] + 0.5 * tw, t_[1] + 0.5 * th
    wx, wy, ww, wh = weights
    tgt = (wx * (tx - sx) / sw, wy * (ty - sy) / sh, ww * flog(tw / sw), wh * flog(th / sh))
    gd, reg, es = [], [], []
    for j in range(4):
        e = num(deltas[:, j], mode) - tgt[j]
        ae, ev = fabs(e), val(e)
        sgn = torch.sign(ev)
        sgn_n = E(sgn) if mode == "ref" else sgn
        lin_g = sgn_n * inv_b
        if beta < 1e-5:
            r_, g_ = ae, lin_g
        else:
            quad = val(ae) < beta
            qg = e / beta * inv_b
            if mode == "ref":                      # continuity at |e| = beta: the quadratic branch's bound on both sides of it
                close = (ae.v - beta).abs() <= HEAD * ae.e
                lin_g = E(lin_g.v, torch.where(close, torch.maximum(lin_g.e, qg.e + (qg.v - lin_g.v).abs()), lin_g.e))
            r_, g_ = fwhere(quad, 0.5 * e * e / beta, ae - 0.5 * beta), fwhere(quad, qg, lin_g)
        gd.append(fwhere(fg, g_, 0.0 * g_))
        reg.append(fwhere(fg, r_, 0.0 * r_))
        es.append(e)
    reg = fstack(reg, 1)
    if mode == "f32":
        loss_box = (reg.double().sum() / B).to(F32)
    else:
        t = reg.sum()
        loss_box = E(t.v / B, t.e / B + U * (t.v / B).abs())
    return dict(d_scores=d_scores, d_deltas=fstack(gd, 1), losses=fstack([loss_cls, loss_box], 0), e=fstack(es, 1), fg=fg)


def planted_deltas(beta: float) -> List[float]:
    """|e| in {0, beta / 2, just below beta, beta, just above beta, 10 beta} (beta = 0: 0 and plain values), with both signs."""
    if beta < 1e-5:
        return [0.0, 0.0, 0.0, 0.0, 0.25, -0.25, 3.0, -3.0]
    b = np.float32(beta)
    lo, hi = float(np.nextafter(b, np.float32(0))), float(np.nextafter(b, np.float32(10)))
    return [0.0, float(b) / 2, -float(b) / 2, lo, -lo, float(b), -float(b), hi, -hi, 10 * float(b), -10 * float(b), 0.0]


@functools.lru_cache(maxsize=None)
def rc_case(B: int, C: int, ld: int, cw_kind: str, gt_kind: str, beta: float, wsel: int) -> Dict[str, object]:
    g = torch.Generator().manual_seed(B * 13 + C + ld)
    scores = torch.randn((B, ld), generator=g) * 4
    flat = (torch.arange(B)[:, None] * ld + torch.arange(ld)[None, :]) % 29
    for j, v in enumerate(RC_LOGITS):
        scores[flat == j] = v
    gt = torch.randint(0, C + 1, (B,), generator=g).int()
    gt[::4] = C
    if gt_kind == "all_bg":
        gt[:] = C
    elif gt_kind == "all_fg":
        gt = torch.randint(0, C, (B,), generator=g).int()
    cw = {"none": None, "mask": (torch.rand((C,), generator=g) < 0.3).float(), "zero": torch.zeros(C),
          "frac": torch.rand((C,), generator=g) * 1.5}[cw_kind]
    side = 4.0 * (250.0 ** torch.rand((B, 2), generator=g))                 # 4 .. 1000 px
    xy = torch.rand((B, 2), generator=g) * (1000.0 - side)
    prop = torch.cat([xy, xy + side], 1)
    gtb = prop + (torch.rand((B, 4), generator=g) - 0.5) * 0.2 * side.repeat(1, 2)
    gtb[:, 2:] = torch.maximum(gtb[:, 2:], gtb[:, :2] + 2)
    deltas = torch.randn((B, 4), generator=g) * 0.4
    plant = torch.arange(B) % 3 == 0                                        # proposal == gt: the target deltas are exactly 0, e = delta
    gtb[plant] = prop[plant]
    pd = planted_deltas(beta)
    rows = plant.nonzero().flatten()
    for n, r_ in enumerate(rows.tolist()):
        deltas[r_] = torch.tensor([pd[(4 * n + j) % len(pd)] for j in range(4)])
    weights = BOX_WEIGHTS[wsel]
    for _ in range(3):
        args = (scores.contiguous(), deltas.contiguous(), prop.contiguous(), gtb.contiguous(), gt, cw, C, weights, beta)
        ref = rc_loss(*args, "ref")
        fg = ref["fg"]
        planted = (plant & fg)[:, None].expand(B, 4)
        band = torch.zeros((B, 4), dtype=torch.bool)
        if beta < 1e-5:                                                     # e against 0 decides the sign: |e| stays above the band
            band = fg[:, None] & (ref["e"].v.abs() <= HEAD * ref["e"].e) & ~planted
            close = fg[:, None] & (ref["e"].v.abs() <= 1e-3) & ~planted
            if bool(close.any()):
                deltas = torch.where(close, deltas + 0.5, deltas)
                continue
        break
    emu = rc_loss(*args, "f32")
    return dict(B=B, C=C, ld=ld, cw=cw, gt=gt, beta=beta, weights=weights, scores=args[0], deltas=args[1], prop=args[2], gtb=args[3],
                ref=ref, emu=emu, band=band, planted=planted, cw_kind=cw_kind, gt_kind=gt_kind)


# ------------------------------------------------------------------------------------------------
# eod_centernet_targets
# ------------------------------------------------------------------------------------------------
STRIDES8 = (8, 16, 32, 64, 128, 256, 512, 1024)
SOI8 = ((0, 80), (64, 160), (128, 320), (256, 640), (512, 10000000), (600, 10000000), (24, 48), (0, 10000000))
#   name -> (level_hw, image (W, H))
TG_PYRAMIDS = {
    77: (((7, 11),), (88.0, 56.0)),
    256: (((10, 12), (6, 8), (4, 6), (4, 4), (3, 4), (3, 4), (3, 4), (3, 4)), (96.0, 80.0)),
    8525: (((80, 80), (40, 40), (20, 20), (10, 10), (5, 5)), (640.0, 640.0)),
}
#          P, N
TG_TABLE = ((77, 0), (77, 1), (77, 64), (256, 16), (256, 255), (8525, 13), (8525, 256), (8525, 257), (8525, 512), (8525, 513), (77, 4096))


def tg_boxes(P: int, N: int) -> torch.Tensor:
    """N boxes inside the pyramid's image.  Box 0's centre lies exactly on a cell edge.  On the full-size pyramid boxes 255 and 256
    share centre and area but not shape (equal weighted distance everywhere: the first must win, across the LDS chunk boundary), and
    box 512 is an isolated small box (the first of the third chunk); the random boxes keep out of their strip (y >= 560)."""
    (W, H) = TG_PYRAMIDS[P][1]
    g = torch.Generator().manual_seed(P + 3 * N)
    full = P == 8525
    xy = torch.rand((N, 2), generator=g) * torch.tensor([W * 0.85, (H - 100.0) if full else H * 0.85])
    n_small = N - N // 3
    wh = torch.cat([torch.rand((n_small, 2), generator=g) * W * 0.1 + 4, torch.rand((N - n_small, 2), generator=g) * W * 0.7 + W * 0.06])
    hi = torch.tensor([W - 1.0, (H - 90.0) if full else H - 1.0])
    b = torch.cat([xy, torch.minimum(xy + wh, hi)], 1)
    if N > 0:
        b[0] = torch.tensor([16.0, 12.0, 48.0, 36.0]) if not full else torch.tensor([52.0, 40.0, 76.0, 60.0])       # centre (32, 24) / (64, 50)
    if full and N > 255:
        b[255] = torch.tensor([288.0, 594.0, 312.0, 606.0])
    if full and N > 256:
        b[256] = torch.tensor([294.0, 588.0, 306.0, 612.0])
    if full and N > 512:
        b[512] = torch.tensor([500.0, 596.0, 516.0, 612.0])
    return b.contiguous()


def tg_heat_ref(boxes: torch.Tensor, level_hw, strides, hm_min_overlap: float = 0.8, min_radius: float = 4.0) -> E:
    """The class-agnostic heat map BEFORE the 1e-4 cut, in float64 with its bound: exp(-min_j dist2_j / radius2_j).  `is_peak` (the
    distance is 0 on the centre's own cell) is a comparison of exactly representable grid coordinates; it is taken in fp32 as the
    kernel and the oracle take it."""
    delta = (1 - hm_min_overlap) / (1 + hm_min_overlap)
    rs, mr2 = f32(delta * delta * 2.0), f32(min_radius * min_radius)
    N = boxes.shape[0]
    x1, y1, x2, y2 = (E(boxes[:, j].double())[None, :] for j in range(4))
    cx, cy = (x1 + x2) / 2.0, (y1 + y2) / 2.0
    area = (x2 - x1) * (y2 - y1)
    r2 = fmax(area * rs, E(torch.full((1, N), mr2, dtype=F64)))
    c32 = (boxes[:, :2] + boxes[:, 2:]) / 2
    out_v, out_e = [], []
    for (h, w), s in zip(level_hw, strides):
        ys, xs = torch.meshgrid(torch.arange(h, dtype=F32) * s + s // 2, torch.arange(w, dtype=F32) * s + s // 2, indexing="ij")
        gx, gy = xs.reshape(-1, 1), ys.reshape(-1, 1)
        if N == 0:
            out_v.append(torch.zeros(h * w, dtype=F64))
            out_e.append(torch.zeros(h * w, dtype=F64))
            continue
        cdx = (c32[:, 0].view(1, N) / s).int().float() * s + s / 2
        cdy = (c32[:, 1].view(1, N) / s).int().float() * s + s / 2
        is_peak = ((gx - cdx) ** 2 + (gy - cdy) ** 2) == 0
        dx, dy = E(gx.double()) - cx, E(gy.double()) - cy
        d2 = dx * dx + dy * dy
        d2 = fwhere(is_peak, 0.0 * d2, d2)
        wd = d2 / r2
        m_hi = (wd.v + wd.e).min(dim=1, keepdim=True)[0]                 # the minimum errs by at most the largest bound among the
        cand = (wd.v - wd.e) <= m_hi                                     # objects that can be the minimum in fp32
        hmin = E(wd.v.min(dim=1)[0], torch.where(cand, wd.e, torch.zeros_like(wd.e)).max(dim=1)[0])
        hm = fexp(-hmin)
        out_v.append(hm.v)
        out_e.append(hm.e)
    return E(torch.cat(out_v), torch.cat(out_e))


@functools.lru_cache(maxsize=None)
def tg_case(P: int, N: int) -> Dict[str, object]:
    from oracle import losses as OL
    level_hw = TG_PYRAMIDS[P][0]
    L = len(level_hw)
    strides, soi = STRIDES8[:L], (OL.CENTERNET_SOI if L == 5 else SOI8[:L])
    boxes = tg_boxes(P, N)
    pos, reg, heat = OL.centernet_targets(boxes, list(level_hw), strides, soi)
    hm = tg_heat_ref(boxes, level_hw, strides)
    cut = E(torch.where(hm.v < 1e-4, torch.zeros_like(hm.v), hm.v), hm.e)
    band = (hm.v - f32(1e-4)).abs() <= HEAD * hm.e
    off = [0]
    for (h, w) in level_hw:
        off.append(off[-1] + h * w)
    return dict(P=P, N=N, L=L, level_hw=level_hw, strides=strides, soi=soi, boxes=boxes, pos=pos, reg=reg, heat32=heat, heat=cut, band=band,
                off=off, n_reg=int((reg.max(dim=1)[0] >= 0).sum()))
