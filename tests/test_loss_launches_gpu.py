"""The training loss and target launches of csrc/train_losses.hip, each alone on small tensors at its own loop edges, against float64
references with per-element bounds derived from the arithmetic (tests/_loss_cases.py states every derivation).

No model is built: every test calls `ops.CenterNetLoss` or the entry points of the loaded library directly and owns every output
buffer.  Every output is pre-filled with the sentinel and carries GUARD rows behind it; what lies outside the live part must keep the
sentinel's bits.  Every launch runs twice and the second result must have the first one's bits (at a position listed more than once
two atomics land on one float: there only the bound is required, and whether it repeated is printed).  No element is left out of a
comparison except those inside a decision band (counted, printed, capped at 1e-4 of the tensor and 16).  Where the reference's value
and bound are both 0 the output must be exactly 0.  `pytest -s` prints one line per comparison: the worst error, the bound at that
element, the share of the bound it takes, and the largest share the CPU fp32 emulation takes in the same comparison.

  eod_centernet_loss      P in {1, 255, 256, 257, 131072, 131073} (the grid cap and one position beyond it), head_stride in {5, 8, 9},
                          1 / 5 / 8 levels with an empty one and regressing rows on both sides of every boundary, two parameter sets;
                          logits 0, +-1e-3, +-20, +-100 and the planted neighbours of clampv, 1 - clampv, ignore_high_fp; heat 0, 1,
                          1e-4; rows without a target, target (-1, 5, 3, 2), raw < 0 and == 0, exact ties on one axis and on all four,
                          all-zero predictions; lists of 0, 1, 255, 256, 257 and 1000 positives with a position listed twice and three
                          times and the indices -1 and P                                                  test_centernet_loss
  ... device-count form   counts_local below, above the capacity and negative, counts_total (0, 0), world_size 1, 2, 3
                                                                                                          test_centernet_loss_device_counts
  eod_fast_rcnn_loss      B in {1, 2, 511, 512, 513} x (C, ld) from (1, 2) to (2047, 2048); class weights none / mask / zero /
                          fractional; logits up to +-1e4; smooth-L1 at |e| in {0, beta / 2, beta-, beta, beta+, 10 beta}; beta = 0
                          with e == 0 exactly                                                             test_fast_rcnn_loss
  ... EOD_LOSS_FED        the chosen weight is tests/_fed_loss_ref.py's, the loss that of a call given it    test_fast_rcnn_loss_fed
  eod_centernet_targets   N in {0, 1, 13, 16, 64, 255, 256, 257, 512, 513, 4096}, P in {77, 256, 8525}, 1 / 5 / 8 levels; the
                          equal-distance twin across the LDS chunk boundary; 4097 boxes refused            test_centernet_targets

Measured on an MI355X (worst share of its bound per output family, the CPU fp32 emulation's worst in brackets; HEAD = 2 was fixed
before the run and the asserts know none of these figures):
  centernet_loss     d_logit 0.302 (0.302)   d_pos 0.464   d_reg 0.151 (0.158)   losses 0.226 (0.226)
  ... device counts  d_logit 0.297           d_reg 0.096                         losses 0.059; both forms bitwise equal at world_size 1
  fast_rcnn_loss     d_scores 0.355 (0.355)  d_deltas 0.486 (0.486)              losses 0.113 (0.113)
  centernet_targets  heat 0.239 (0.240); positions, counts and regression targets exact
Excluded by a decision band: one logit of 131072 (P = 131072, `noalpha`), no element anywhere else.  The positions listed twice and
three times repeated bitwise in every run.

Mutants of train_losses.hip, built apart and not kept, each through this module (the factor is the worst share of a bound):
  half_on_tie returning 1 on a tie          test_centernet_loss, ..._device_counts: d_reg 2.1e5 to 3.5e5 times the bound
  `inside` dropped from the dense gradient  the same tests: d_logit must be exactly 0 on 24 to 35 saturated rows and is not
  level chain comparing i > lv_off[q]       the same tests: d_reg 2.4e5 to 4.7e5 times the bound on the rows at the boundaries
  dense pass skipping position 131072       test_centernet_loss[131073-*]: the row keeps the sentinel (an exact check, no factor)
  positive term stored, not added           test_centernet_loss (every case with a list), ..._device_counts: d_logit 1.2e5 to 1.5e5
  c > C for c >= C in the rows kernel       test_fast_rcnn_loss: column C of d_scores is not exactly 0 (exact check)
  quadratic branch without the 0.5          test_fast_rcnn_loss, ..._fed with beta > 0: loss_box_reg 2.2e2 to 7.0e3 times the bound
                                            (the gradient does not change)
  targets' wd <= best for wd < best         test_centernet_targets: 43 to 292 regression targets differ from the oracle's bits

The unmarked tests are the references' own checks and pass without a GPU."""
import ctypes as C
import os
import sys
from typing import Dict, Optional

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if __name__ == "__main__":
    sys.path[:0] = [ROOT, os.path.dirname(os.path.abspath(__file__))]

import _loss_cases as LC                                                               # noqa: E402
from _loss_cases import E, F32, F64, SENTINEL                                          # noqa: E402

gpu = pytest.mark.gpu          # every test below that launches anything carries it; the references' CPU self-checks do not

GUARD = 32                     # sentinel rows behind every output buffer
WORST: Dict[str, float] = {}   # family -> the largest share of a bound any of its comparisons took



@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    from embodied_object_detection_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


# ------------------------------------------------------------------------------------------------
# comparison and reporting
# ------------------------------------------------------------------------------------------------
def _compare(family: str, tag: str, what: str, got: Optional[torch.Tensor], ref: E, emu: torch.Tensor, exclude: Optional[torch.Tensor] = None,
             extra_bound: Optional[torch.Tensor] = None, limit: float = 1.0) -> float:
    """Every element of `got` within HEAD * e + TINY of the float64 `ref` (exactly 0 where value and bound are 0), the elements of
    `exclude` apart; the fp32 emulation within `limit` of the same bound.  `got` None: the emulation alone.  -> the emulation's share."""
    bound = LC.bound(ref) + (0 if extra_bound is None else extra_bound)
    keep = torch.ones_like(ref.v, dtype=torch.bool) if exclude is None else ~exclude
    n_ex = int((~keep).sum())
    assert LC.band_ok(n_ex, ref.v.numel()), f"{tag} {what}: {n_ex} of {ref.v.numel()} elements inside a decision band"
    if int(keep.sum()) == 0:
        print(f"{tag:66s} {what:9s} nothing to compare ({n_ex} excluded)", flush=True)
        return 0.0
    yard = float(LC.share((emu.double() - ref.v).abs()[keep], bound[keep]).max())
    assert yard <= limit, f"{tag} {what}: the fp32 emulation itself is at {yard:.3f} of the bound"
    if got is None:
        return yard
    got = got.detach().cpu().double()
    assert torch.isfinite(got).all(), f"{tag} {what}: non-finite output"
    err = (got - ref.v).abs()
    sh = torch.where(keep, LC.share(err, bound), torch.zeros_like(err))
    i = int(sh.argmax())
    worst = float(sh.reshape(-1)[i])
    print(f"{tag:66s} {what:9s} err {float(err.reshape(-1)[i]):.3e}  bound {float(bound.reshape(-1)[i]):.3e}  ({worst:.3f} of it)  "
          f"cpu fp32 {yard:.3f}  excluded {n_ex}", flush=True)
    WORST[family + " " + what] = max(WORST.get(family + " " + what, 0.0), worst)
    exact = keep & (ref.v == 0) & (ref.e == 0)
    assert bool((got[exact] == 0).all()), f"{tag} {what}: {int((got[exact] != 0).sum())} elements that must be exactly 0 are not"
    bad = int((sh > 1).sum())
    assert bad == 0, f"{tag} {what}: {bad} of {err.numel()} elements beyond the bound, the worst at {worst:.3f} of it"
    return yard


def _bits(t: torch.Tensor) -> torch.Tensor:
    return t.view(torch.int32) if t.dtype == F32 else t


def _same_bits(a: torch.Tensor, b: torch.Tensor) -> bool:
    return torch.equal(_bits(a.cpu().contiguous()), _bits(b.cpu().contiguous()))


def _sent(shape, dev, dtype=F32) -> torch.Tensor:
    return torch.full(shape, SENTINEL if dtype == F32 else LC.I32_SENTINEL, dtype=dtype, device=dev)


def _guarded(tag: str, buf: torch.Tensor, live: int) -> None:
    """Everything behind the first `live` rows of `buf` holds the sentinel's bits."""
    tail = buf[live:].cpu()
    fill = torch.full_like(tail, SENTINEL if buf.dtype == F32 else LC.I32_SENTINEL)
    assert torch.equal(_bits(tail.contiguous()), _bits(fill)), f"{tag}: written behind its end"


def _summary(prefix: str) -> None:
    for f in sorted(WORST):
        if f.startswith(prefix):
            print(f"  [{f}] worst share of a bound so far: {WORST[f]:.3f}", flush=True)


# ------------------------------------------------------------------------------------------------
# eod_centernet_loss
# ------------------------------------------------------------------------------------------------
def _cn_launch(ops, dev, c, k, pos: torch.Tensor, counts_local=None, counts_total=None, world: int = 1):
    """One call into fresh sentinel-filled buffers -> (d_head [P + GUARD, stride], losses [3 + GUARD])."""
    P, stride = c["P"], c["stride"]
    fn = ops.CenterNetLoss(c["off"], c["scales"], dev, head_stride=stride, **c["prm"])
    losses = _sent((3 + GUARD,), dev)
    fn.losses, fn.desc.losses = losses, losses.data_ptr()
    out = _sent((P + GUARD, stride), dev)
    dc = lambda t: None if t is None else torch.tensor(t, dtype=torch.int32, device=dev)          # noqa: E731
    fn(c["head"].to(dev), c["heat"].to(dev), c["reg_t"].to(dev), pos.to(dev), k["num_pos_avg"], k["reg_norm"], out=out[:P],
       counts_local=dc(counts_local), counts_total=dc(counts_total), world_size=world)
    torch.cuda.synchronize()
    return out, losses


def _cn_check(family: str, tag: str, c, k, ref, emu, out, losses, limit: float = 1.0) -> None:
    P = c["P"]
    if out is not None:
        _guarded(f"{tag} d_head", out, P)
        _guarded(f"{tag} losses", losses, 3)
        assert bool((out[:P, 5:] == 0).all()), f"{tag}: a column beyond the fifth is not exactly 0"
    band = LC.sigmoid_band(ref["s"], k) & ~c["planted"]
    o = None if out is None else out[:P].cpu()
    _compare(family, tag, "d_logit", None if o is None else o[:, 0], ref["d0"], emu["d0"], exclude=band, limit=limit)
    _compare(family, tag, "d_reg", None if o is None else o[:, 1:5], ref["g"], emu["g"], limit=limit)
    # an element inside the ignore_high_fp band may or may not contribute its term to the negative sum
    extra = torch.zeros(3, dtype=F64)
    kn = abs(k["an"] * k["c_neg"])
    extra[2] = kn * float(ref["neg_raw"].v.abs()[band].sum()) * 1.001
    _compare(family, tag, "losses", None if losses is None else losses[:3], ref["losses"], emu["losses"], extra_bound=extra, limit=limit)


@gpu
@pytest.mark.parametrize("P,stride,L,n_pos,pset", list(LC.cn_table()))
def test_centernet_loss(dev, P, stride, L, n_pos, pset):
    """`eod_centernet_loss`, host-count form: the dense pass at its workgroup, grid-cap and level edges, the positives' workgroup at
    its loop edges; the negative term's store alone (no list) and with the positives added, and the added part by itself."""
    from embodied_object_detection_amd import ops
    c = LC.cn_case(P, stride, L, n_pos, pset)
    k, tag = c["k"], f"centernet_loss P {P} stride {stride} L {L} n_pos {n_pos} {pset}"
    none = c["pos"][:0]
    a0, b0 = _cn_launch(ops, dev, c, k, none), _cn_launch(ops, dev, c, k, none)
    assert _same_bits(a0[0], b0[0]) and _same_bits(a0[1], b0[1]), f"{tag}: a second launch without a list gave other bits"
    _cn_check("centernet_loss", tag + " no list", c, k, c["ref0"], c["emu0"], *a0)
    if n_pos == 0:
        return _summary("centernet_loss")
    a, b = _cn_launch(ops, dev, c, k, c["pos"]), _cn_launch(ops, dev, c, k, c["pos"])
    ref, emu = c["ref"], c["emu"]
    dup = torch.zeros(P, dtype=torch.bool)
    dup[ref["uniq"][ref["mult"] > 1]] = True
    x, y = a[0][:P].cpu(), b[0][:P].cpu()
    assert _same_bits(x[:, 1:], y[:, 1:]) and _same_bits(x[~dup, 0], y[~dup, 0]) and _same_bits(a[1], b[1]), f"{tag}: a second launch gave other bits"
    if bool(dup.any()):
        print(f"{tag:66s} positions listed more than once: {int(dup.sum())}, repeated bitwise: {_same_bits(x[dup, 0], y[dup, 0])}", flush=True)
    _cn_check("centernet_loss", tag, c, k, ref, emu, *a)
    # the part the positives added, by itself: m equal addends onto the negative term's store
    u, m = ref["uniq"], ref["mult"].double()
    added = (x[u, 0].double() - a0[0][:P].cpu()[u, 0].double())
    want = E(ref["pos_g"].v * m, ref["pos_g"].e * m + m * LC.U * ref["d0"].v[u].abs())
    band = (LC.sigmoid_band(ref["s"], k) & ~c["planted"])[u]
    _compare("centernet_loss", tag, "d_pos", added, want, (emu["d0"][u].double() - emu["d0_neg"][u].double()), exclude=band)
    # nothing was written for the indices -1 and P: the guard rows checked above lie right behind position P - 1
    _summary("centernet_loss")


@gpu
def test_centernet_loss_device_counts(dev):
    """The device-count form (`counts_local`, `counts_total`, `world_size`: what modeling/training.py calls) against the same float64
    reference: the list's length read on the device (below the capacity with live-looking indices behind it, above it, negative), the
    normalisers max(float32(count / world), 1)."""
    from embodied_object_detection_amd import ops
    P, stride, L = 257, 8, 5
    c = LC.cn_case(P, stride, L, 256, "default")
    cap = 300
    g = torch.Generator().manual_seed(3)
    lst = torch.randint(0, P, (cap,), generator=g).int()
    for n_local, totals, world in ((200, (200, 37), 1), (200, (200, 37), 2), (200, (401, 100), 3), (400, (300, 96), 1), (-5, (0, 0), 1), (0, (0, 0), 2),
                                   (1, (7, 5), 3)):
        n = min(max(n_local, 0), cap)
        k = LC.cn_constants(c["prm"], totals[0], totals[1], world)
        ref, emu = LC.cn_reference(c, lst[:n], k)
        tag = f"centernet_loss counts_local {n_local} total {totals} world {world}"
        a = _cn_launch(ops, dev, c, k, lst, (n_local, 0), totals, world)
        b = _cn_launch(ops, dev, c, k, lst, (n_local, 0), totals, world)
        dup = torch.zeros(P, dtype=torch.bool)
        dup[ref["uniq"][ref["mult"] > 1]] = True
        x, y = a[0][:P].cpu(), b[0][:P].cpu()
        assert _same_bits(x[:, 1:], y[:, 1:]) and _same_bits(x[~dup, 0], y[~dup, 0]) and _same_bits(a[1], b[1]), f"{tag}: a second launch gave other bits"
        _cn_check("centernet_loss counts", tag, c, k, ref, emu, *a)
        if world == 1:
            h = _cn_launch(ops, dev, c, k, lst[:n])
            print(f"{tag:66s} host-count form bitwise equal: d_head {_same_bits(h[0], a[0])}, losses {_same_bits(h[1], a[1])}", flush=True)
            _cn_check("centernet_loss counts", tag + " (host form)", c, k, ref, emu, *h)
    _summary("centernet_loss counts")


# ------------------------------------------------------------------------------------------------
# eod_fast_rcnn_loss
# ------------------------------------------------------------------------------------------------
def _rc_launch(ops, lib, dev, c, cw: Optional[torch.Tensor], fed=None):
    """One call of the library's entry point into fresh sentinel-filled buffers -> (d_scores, d_deltas, losses[, class weight])."""
    B, Cn, ld = c["B"], c["C"], c["ld"]
    ds, dd, losses = _sent((B + GUARD, ld), dev), _sent((B + GUARD, 4), dev), _sent((2 + GUARD,), dev)
    ins = [c[n].to(dev) for n in ("scores", "deltas", "prop", "gtb")] + [c["gt"].to(dev)]
    flag = 0
    if fed is not None:
        fed.reserve(B)
        cw = _sent((Cn + GUARD,), dev)
        ws, nbytes, flag = fed.ws, fed.ws.numel() * 4, ops.EOD_LOSS_FED
    else:
        nbytes = lib.eod_fast_rcnn_loss_workspace_bytes(B)
        ws = torch.empty((nbytes // 8,), dtype=F64, device=dev)
        cw = None if cw is None else cw.to(dev)
    wx, wy, ww, wh = c["weights"]
    st = lib.eod_fast_rcnn_loss(ins[0].data_ptr(), ld, ins[1].data_ptr(), ins[2].data_ptr(), ins[3].data_ptr(), ins[4].data_ptr(),
                                None if cw is None else cw.data_ptr(), B, Cn | flag, wx, wy, ww, wh, c["beta"], ds.data_ptr(), dd.data_ptr(),
                                losses.data_ptr(), ws.data_ptr(), nbytes, ops._stream())
    assert st == 0, f"eod_fast_rcnn_loss returned {st}"
    torch.cuda.synchronize()
    return (ds, dd, losses) + ((cw,) if fed is not None else ())


def _rc_tag(c) -> str:
    return f"fast_rcnn_loss B {c['B']} C {c['C']} ld {c['ld']} cw {c['cw_kind']} gt {c['gt_kind']} beta {c['beta']} w {c['weights'][0]:.0f}"


def _rc_check(tag: str, c, ds, dd, losses) -> None:
    B, ref, emu = c["B"], c["ref"], c["emu"]
    _guarded(f"{tag} d_scores", ds, B)
    _guarded(f"{tag} d_deltas", dd, B)
    _guarded(f"{tag} losses", losses, 2)
    assert bool((ds[:B, c["C"]:] == 0).all()), f"{tag}: the background or a padding column of d_scores is not exactly 0"
    _compare("fast_rcnn_loss", tag, "d_scores", ds[:B], ref["d_scores"], emu["d_scores"])
    _compare("fast_rcnn_loss", tag, "d_deltas", dd[:B], ref["d_deltas"], emu["d_deltas"], exclude=c["band"])
    _compare("fast_rcnn_loss", tag, "losses", losses[:2], ref["losses"], emu["losses"])
    if c["beta"] < 1e-5 and bool(c["planted"].any()):
        zero = c["planted"] & (c["deltas"] == 0)
        assert bool(zero.any()) and bool((dd[:B].cpu()[zero] == 0).all()), f"{tag}: e == 0 exactly must give a gradient of exactly 0"
    if c["cw_kind"] == "zero":
        assert float(losses[0]) == 0.0 and bool((ds[:B] == 0).all()), f"{tag}: all-zero class weights must give exactly 0"


@gpu
@pytest.mark.parametrize("row", LC.RC_TABLE, ids=lambda r: f"B{r[0]}-C{r[1]}-ld{r[2]}-{r[3]}-{r[4]}-beta{r[5]}")
def test_fast_rcnn_loss(dev, row):
    """`eod_fast_rcnn_loss` on the library's entry point: one workgroup per row at one and several passes of its column loop, the
    background and padding columns, the smooth-L1 branches at their joints, the row sums added in row order."""
    from embodied_object_detection_amd import _lib, ops
    lib = _lib.load()
    c = LC.rc_case(*row)
    tag = _rc_tag(c)
    a, b = _rc_launch(ops, lib, dev, c, c["cw"]), _rc_launch(ops, lib, dev, c, c["cw"])
    assert all(_same_bits(x, y) for x, y in zip(a, b)), f"{tag}: a second launch gave other bits"
    _rc_check(tag, c, *a)
    _summary("fast_rcnn_loss")


@gpu
@pytest.mark.parametrize("row,n_cat", [((2, 20, 21, "none", "mixed", 0.3, 1), 8), ((513, 256, 257, "none", "all_fg", 0.3, 0), 50),
                                       ((511, 2047, 2048, "none", "mixed", 0.3, 1), 300)], ids=("C20", "C256", "C2047"))
def test_fast_rcnn_loss_fed(dev, row, n_cat):
    """`EOD_LOSS_FED`: the class weight the launch in front chooses is exactly tests/_fed_loss_ref.py's, and loss and gradients are
    bitwise those of a call that is handed that weight."""
    from _fed_loss_ref import fed_loss_weight_ref
    from embodied_object_detection_amd import _lib, ops
    lib = _lib.load()
    c = LC.rc_case(*row)
    Cn, tag = c["C"], _rc_tag(c) + " fed"
    g = torch.Generator().manual_seed(Cn)
    q = torch.empty(Cn).exponential_(1.0, generator=g)
    prob = torch.rand((Cn,), generator=g) ** 0.5
    prob[::7] = 0.0
    src = torch.rand((Cn,), generator=g)
    src[::5] = 0.0
    fed = ops.FedLossParams(Cn, n_cat, prob, src, dev)
    fed.set_q(q)
    a, b = _rc_launch(ops, lib, dev, c, None, fed), _rc_launch(ops, lib, dev, c, None, fed)
    assert all(_same_bits(x, y) for x, y in zip(a, b)), f"{tag}: a second launch gave other bits"
    cw = a[3]
    _guarded(f"{tag} class weight", cw, Cn)
    want = fed_loss_weight_ref(c["gt"], Cn, q, n_cat, prob, src)
    assert torch.equal(cw[:Cn].cpu(), want), f"{tag}: {int((cw[:Cn].cpu() != want).sum())} class weights differ from the reference choice"
    assert 0 < int(want.sum()) < Cn
    given = _rc_launch(ops, lib, dev, c, cw[:Cn].clone())
    assert all(_same_bits(x, y) for x, y in zip(a[:3], given)), f"{tag}: not the bits of a call given the same weight"
    c2 = dict(c, cw=want, cw_kind="fed")
    r = LC.rc_loss(c["scores"], c["deltas"], c["prop"], c["gtb"], c["gt"], want, Cn, c["weights"], c["beta"], "ref")
    e = LC.rc_loss(c["scores"], c["deltas"], c["prop"], c["gtb"], c["gt"], want, Cn, c["weights"], c["beta"], "f32")
    _rc_check(tag, dict(c2, ref=r, emu=e), *a[:3])
    print(f"{tag:66s} class weight: {int(want.sum())} of {Cn} on, exact; bits of the call given it", flush=True)


# ------------------------------------------------------------------------------------------------
# eod_centernet_targets
# ------------------------------------------------------------------------------------------------
def _tg_launch(lib, ops, dev, c, n_boxes: Optional[int] = None):
    """One call on the library's entry point into fresh sentinel-filled buffers -> (status, heat, reg, pos, counts)."""
    from embodied_object_detection_amd import _lib
    N, L, P = c["N"], c["L"], c["P"]
    d = _lib.EodCenterNetTargetDesc()
    boxes = c["boxes"].to(dev)
    n_boxes = N if n_boxes is None else n_boxes
    d.gt_boxes, d.n_boxes, d.levels = (boxes.data_ptr() if N else None), n_boxes, L
    for i, v in enumerate(c["off"]):
        d.level_off[i] = v
    for l in range(L):
        d.level_w[l], d.level_stride[l] = c["level_hw"][l][1], c["strides"][l]
        d.soi_lo[l], d.soi_hi[l] = float(c["soi"][l][0]), float(c["soi"][l][1])
    d.hm_min_overlap, d.min_radius = 0.8, 4.0
    heat, reg = _sent((P + GUARD,), dev), _sent((P + GUARD, 4), dev)
    pos, counts = _sent((N * L + GUARD,), dev, torch.int32), _sent((2 + GUARD,), dev, torch.int32)
    d.agn_heatmap, d.reg_targets, d.pos_inds, d.counts = heat.data_ptr(), reg.data_ptr(), pos.data_ptr(), counts.data_ptr()
    st = lib.eod_centernet_targets(C.byref(d), ops._stream())
    torch.cuda.synchronize()
    return st, heat, reg, pos, counts


@gpu
@pytest.mark.parametrize("P,N", LC.TG_TABLE)
def test_centernet_targets(dev, P, N):
    """`eod_centernet_targets`: positions, counts and regression targets bit for bit the oracle's, the heat map against float64 with
    its bound (the 1e-4 cut is a decision band), `pos` behind counts[0] and every guard row untouched."""
    from embodied_object_detection_amd import _lib, ops
    lib = _lib.load()
    c = LC.tg_case(P, N)
    tag = f"centernet_targets P {P} N {N} L {c['L']}"
    a, b = _tg_launch(lib, ops, dev, c), _tg_launch(lib, ops, dev, c)
    assert a[0] == 0 and b[0] == 0, f"{tag}: status {a[0]}"
    assert all(_same_bits(x, y) for x, y in zip(a[1:], b[1:])), f"{tag}: a second launch gave other bits"
    _, heat, reg, pos, counts = a
    n_pos, n_reg = counts[:2].cpu().tolist()
    _guarded(f"{tag} counts", counts, 2)
    assert n_pos == c["pos"].numel() and pos[:n_pos].cpu().tolist() == c["pos"].tolist(), f"{tag}: the positive locations differ"
    _guarded(f"{tag} pos", pos, n_pos)
    _guarded(f"{tag} reg", reg, P)
    _guarded(f"{tag} heat", heat, P)
    assert _same_bits(reg[:P], c["reg"]), f"{tag}: {int((reg[:P].cpu() != c['reg']).sum())} regression targets differ from the oracle's bits"
    assert n_reg == c["n_reg"]
    h = heat[:P].cpu()
    assert torch.equal((h == 0)[~c["band"]], (c["heat32"] == 0)[~c["band"]])
    _compare("centernet_targets", tag, "heat", h, c["heat"], c["heat32"], exclude=c["band"])
    print(f"{tag:66s} positives {n_pos}, regression rows {n_reg}: exact", flush=True)
    _summary("centernet_targets")


@gpu
def test_centernet_targets_refuses_4097_boxes(dev):
    """4096 boxes are accepted (the table above), 4097 are refused before any launch: nothing is written."""
    from embodied_object_detection_amd import _lib, ops
    c = dict(LC.tg_case(77, 4096))
    c["boxes"] = torch.cat([c["boxes"], c["boxes"][:1]])
    st, heat, reg, pos, counts = _tg_launch(_lib.load(), ops, dev, c, n_boxes=4097)
    assert st == -1, f"status {st}, EOD_ERR_BAD_DIMS expected"
    for name, buf in (("heat", heat), ("reg", reg), ("pos", pos), ("counts", counts)):
        _guarded(f"4097 boxes {name}", buf, 0)


# ------------------------------------------------------------------------------------------------
# the references' own checks (no GPU)
# ------------------------------------------------------------------------------------------------
def test_fp32_emulation_stays_inside_half_of_every_bound():
    """HEAD was fixed from this side alone: a CPU fp32 computation in the kernel's operation order stays at or under HALF of every
    bound on every case of the tables, and the decision bands of the inputs hold no more elements than the cap allows.  The builders'
    own promises are checked too: planted ties are ties in float64, every other prediction is clear of its target."""
    worst: Dict[str, float] = {}

    def note(fam, v):
        worst[fam] = max(worst.get(fam, 0.0), v)
    for P, stride, L, n_pos, pset in LC.cn_table():
        c = LC.cn_case(P, stride, L, n_pos, pset)
        k = c["k"]
        tag = f"centernet_loss P {P} {pset}"
        for ref, emu in ((c["ref0"], c["emu0"]), (c["ref"], c["emu"])):
            band = LC.sigmoid_band(ref["s"], k) & ~c["planted"]
            note("centernet_loss d_logit", _compare("", tag, "d_logit", None, ref["d0"], emu["d0"], exclude=band, limit=0.5))
            note("centernet_loss d_reg", _compare("", tag, "d_reg", None, ref["g"], emu["g"], limit=0.5))
            note("centernet_loss losses", _compare("", tag, "losses", None, ref["losses"], emu["losses"], limit=0.5))
        r64 = c["head"][:, 1:5].double() * c["sc_rows"].double()[:, None]
        t64 = c["reg_t"].double()
        has = (c["rk"] >= 8)[:, None]
        assert bool((r64 == t64)[c["tie"]].all()), f"{tag}: a planted tie is no tie in float64"
        clear = ((r64 - t64).abs() >= 5e-4 * t64.abs()) | c["tie"] | ~has
        assert bool(clear.all()), f"{tag}: a prediction within fp32 rounding of its target"
        if P >= 255:
            assert bool(c["tie"].all(1).any()) and bool((c["tie"].sum(1) == 1).any()) and bool((c["rk"] == 11).any()) and bool((c["rk"] == 14).any())
    for row in LC.RC_TABLE:
        c = LC.rc_case(*row)
        tag = f"fast_rcnn_loss {row}"
        for what, ex in (("d_scores", None), ("d_deltas", c["band"]), ("losses", None)):
            note(f"fast_rcnn_loss {what}", _compare("", tag, what, None, c["ref"][what], c["emu"][what], exclude=ex, limit=0.5))
    for P, N in LC.TG_TABLE:
        c = LC.tg_case(P, N)
        note("centernet_targets heat", _compare("", f"centernet_targets P {P} N {N}", "heat", None, c["heat"], c["heat32"], exclude=c["band"], limit=0.5))
    for fam, v in sorted(worst.items()):
        print(f"fp32 emulation, {fam:28s} at most {v:.3f} of its bound")
    # the twin across the chunk boundary decides a position: the cell that holds both centres regresses to box 255, not 256
    c = LC.tg_case(8525, 513)
    cell = 75 * 80 + 37
    assert torch.equal(c["reg"][cell] * 8, torch.tensor([12.0, 10.0, 12.0, 2.0]))
    cell = (600 // 8) * 80 + 508 // 8                                        # ... and box 512 alone claims its own centre cell
    assert float(c["reg"][cell].max()) >= 0
    # the bounds bite: a tie derivative of 1 where 0.5 belongs is far beyond the bound of a tied row's gradient
    c = LC.cn_case(257, 5, 5, 256, "default")
    LC.TIE_VALUE = 1.0
    try:
        wrong = LC.cn_dense(c["head"], c["heat"], c["reg_t"], c["sc_rows"], c["k"], "f32")["g"]
    finally:
        LC.TIE_VALUE = 0.5
    g, rows = c["ref"]["g"], c["tie"].any(1)
    over = LC.share((wrong.double() - g.v).abs(), LC.bound(g))
    print(f"tie derivative 1 for 0.5: at least {float(over[rows].max(1)[0].min()):.1f} times the bound on every tied row")
    assert float(over[rows].max(1)[0].min()) > 10 and float(over[~rows].max()) <= 0.5


def test_band_counts_of_random_logits():
    """`randn * 3` logits at P = 131073: the three sigmoid thresholds' bands hold no more elements than the cap, on five seeds."""
    k = LC.cn_constants(LC.PARAM_SETS["default"], 1, 1)
    for seed in range(5):
        z = torch.randn((131073,), generator=torch.Generator().manual_seed(seed)) * 3
        n = int(LC.sigmoid_band(LC.fsigmoid(E(z.double())), k).sum())
        print(f"seed {seed}: {n} of 131073 logits inside a band")
        assert LC.band_ok(n, 131073)


def test_references_are_the_oracles():
    """The float64 references against oracle/losses.py (fp32, autograd) at one ordinary shape each, within fp32 rounding."""
    from oracle import losses as OL
    # ---- CenterNet losses
    c = LC.cn_case(257, 5, 5, 256, "default")
    ref, P = c["ref"], 257
    valid = c["pos"][(c["pos"] >= 0) & (c["pos"] < P)].long()
    hz = c["head"].clone().requires_grad_()
    regp = torch.relu(hz[:, 1:5] * c["sc_rows"][:, None])
    want = OL.centernet_proposal_losses(hz[:, 0], regp, c["heat"], c["reg_t"], valid, **c["prm"])
    sum(want.values()).backward()
    for i, name in enumerate(("loss_centernet_loc", "loss_centernet_agn_pos", "loss_centernet_agn_neg")):
        assert abs(float(ref["losses"].v[i]) - want[name].item()) <= 2e-5 * abs(want[name].item()), name
    band = LC.sigmoid_band(ref["s"], c["k"])
    d0 = ref["d0"].v.float()
    torch.testing.assert_close(d0[~band], hz.grad[:, 0][~band], rtol=1e-4, atol=1e-9)
    torch.testing.assert_close(ref["g"].v.float(), hz.grad[:, 1:5], rtol=2e-4, atol=1e-8)
    # ---- Fast R-CNN losses
    for row in ((511, 20, 24, "frac", "mixed", 1.0, 0), (512, 20, 21, "frac", "mixed", 0.0, 1)):
        c = LC.rc_case(*row)
        B, Cn = c["B"], c["C"]
        zl = c["scores"][:, :Cn + 1].clone().requires_grad_()
        dl = c["deltas"].clone().requires_grad_()
        lc = OL.sigmoid_cross_entropy_loss(zl, c["gt"].long(), c["cw"])
        lb = OL.box_reg_loss(c["prop"], c["gtb"], dl, c["gt"].long(), Cn, c["weights"], c["beta"])
        (lc + lb).backward()
        ref = c["ref"]
        assert abs(float(ref["losses"].v[0]) - lc.item()) <= 1e-5 * lc.item() and abs(float(ref["losses"].v[1]) - lb.item()) <= 1e-5 * lb.item()
        torch.testing.assert_close(ref["d_scores"].v.float()[:, :Cn], zl.grad[:, :Cn], rtol=1e-4, atol=1e-9)
        ok = ~c["band"]
        # tx - sx cancels at coordinates near 1000 on sides of 4 px: fp32 rounding there is what the derived bound says it is
        assert bool(((ref["d_deltas"].v - dl.grad.double()).abs() <= LC.bound(ref["d_deltas"]))[ok].all())
    # ---- CenterNet targets: positions and regression targets ARE the oracle's; the float64 heat map against its fp32 one
    c = LC.tg_case(8525, 257)
    ok = ~c["band"]
    torch.testing.assert_close(c["heat"].v.float()[ok], c["heat32"][ok], rtol=1e-4, atol=1e-9)
    assert 0 < int((c["heat32"] == 0).sum()) < 8525 and c["pos"].numel() > 257


if __name__ == "__main__":
    sys.exit(pytest.main([__file__, "-s", "-q"] + sys.argv[1:]))
