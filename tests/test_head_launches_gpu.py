"""The box-head and post-processing launches of the inference frame, each alone on small tensors at its own tile and loop edges, against
float64 references with bounds derived from the arithmetic (tests/_head_cases.py states every derivation).

No model is built and nothing is recorded: every test calls `ops.*` directly.  Every output buffer is pre-filled with the sentinel and
carries GUARD rows behind it; whatever lies outside the live rows must keep the sentinel's bits.  Every launch runs twice into fresh
buffers and the second result must have the first one's bits.  No element is left out of any comparison.  `pytest -s` prints one line
per comparison: the worst error, the bound at that element, the share of the bound it takes, and the largest share the CPU fp32
emulation of the kernel's summation order takes anywhere in the same comparison (the yardstick).

  narrow classifier   `zs_classify`, C1 in {2, 21, 24}: four rows per workgroup            test_narrow_classifier
  wide classifier     `zs_classify(wide=True)`, C1 in {25, 32, 33, 1204}: 32 x 32 tiles,
                      four K-quarters; `memory_scores` with C1 > 24 (the kernel's mode 2)    test_wide_classifier, test_wide_memory_scores
  BoxTail             `cascade_stage_tail`, widths {16, 1024, 1040}: 16 inputs per lane       test_cascade_stage_tail
  glue                `apply_deltas`, `cascade_scores`, narrow `memory_scores`               test_apply_deltas, test_cascade_scores,
                                                                                             test_narrow_memory_scores
  post-process        `detector_postprocess`: 512 slots, exact                               test_detector_postprocess
  mask predictor      `mask_predictor_sigmoid`, C in {4, 256, 260}: 256 channels per trip     test_mask_predictor

The unmarked tests are the references' own checks and pass without a GPU: the fp32 emulation of every summation order stays inside
every bound on every case of the tables, and every float64 reference agrees with the committed oracle at fp32 tolerance."""
import os
import sys
import types
from typing import Dict, Optional

import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if __name__ == "__main__":
    sys.path[:0] = [ROOT, os.path.dirname(os.path.abspath(__file__))]

import _head_cases as HC                                                               # noqa: E402
from _head_cases import F32, F64, SENTINEL                                             # noqa: E402

gpu = pytest.mark.gpu          # every test below that launches anything carries it; the references' CPU self-checks do not

GUARD = 32                     # sentinel rows behind every output buffer: one whole tile of the widest kernel
WORST: Dict[str, float] = {}   # family -> the largest share of a bound any of its comparisons took (printed after every test)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    from embodied_object_detection_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


# ------------------------------------------------------------------------------------------------
# comparison and reporting
# ------------------------------------------------------------------------------------------------
def _line(tag: str, what: str, err: float, bound: float, yard: float, extra: str = "") -> None:
    print(f"{tag:58s} {what:10s} err {err:.3e}  bound {bound:.3e}  ({err / max(bound, 1e-300):.3f} of it)  cpu fp32 {yard:.3f} of its bound {extra}",
          flush=True)


def _within(family: str, tag: str, what: str, got: torch.Tensor, ref: torch.Tensor, emu: torch.Tensor, bound: torch.Tensor,
            rows: Optional[torch.Tensor] = None) -> None:
    """Every element of `got` (the rows of `rows` where given) within `bound` of the float64 `ref`; prints the comparison's line."""
    got, emu, bound = got.detach().cpu().double(), emu.double(), bound.expand_as(ref)
    if rows is not None:
        got, ref, emu, bound = got[rows], ref[rows], emu[rows], bound[rows]
    if ref.numel() == 0:
        print(f"{tag:58s} {what:10s} no live row", flush=True)
        return
    assert torch.isfinite(got).all(), f"{tag} {what}: non-finite output"
    err = (got - ref).abs()
    share = HC.share(err, bound)
    i = int(share.argmax())
    yard = float(HC.share((emu - ref).abs(), bound).max())
    _line(tag, what, float(err.reshape(-1)[i]), float(bound.reshape(-1)[i]), yard)
    WORST[family] = max(WORST.get(family, 0.0), float(share.reshape(-1)[i]))
    assert yard <= 1.0, f"{tag} {what}: the fp32 emulation itself is at {yard:.3f} of the bound"
    bad = int((err > bound).sum())
    assert bad == 0, f"{tag} {what}: {bad} of {err.numel()} elements beyond the bound, the worst at {float(share.max()):.3f} of it"


def _bits(t: torch.Tensor) -> torch.Tensor:
    return t.view(torch.int32) if t.dtype == F32 else t


def _twice(run):
    """Run a launch twice into fresh sentinel-filled outputs: -> the first result, after asserting the second has the same bits."""
    a, b = run(), run()
    torch.cuda.synchronize()
    for x, y in zip(a, b):
        assert (x is None and y is None) or torch.equal(_bits(x), _bits(y)), "a second launch gave other bits"
    return a


def _sent(shape, dev, dtype=F32) -> torch.Tensor:
    return torch.full(shape, SENTINEL if dtype == F32 else HC.I32_SENTINEL, dtype=dtype, device=dev)


def _untouched(tag: str, buf: torch.Tensor, live: torch.Tensor) -> None:
    """The rows of `buf` outside `live` (the GUARD rows among them) hold the sentinel's bits."""
    dead = torch.ones(buf.shape[0], dtype=torch.bool)
    dead[:live.numel()] = ~live
    fill = torch.full((), SENTINEL if buf.dtype == F32 else HC.I32_SENTINEL, dtype=buf.dtype)
    assert torch.equal(_bits(buf.cpu()[dead]), _bits(fill.expand_as(buf.cpu()[dead]).contiguous())), f"{tag}: a row without work was written"


def _count(counts, dev):
    return None if counts is None else torch.tensor(counts, dtype=torch.int32, device=dev)


def _summary(*families: str) -> None:
    for f in families:
        if f in WORST:
            print(f"  [{f}] worst share of a bound so far: {WORST[f]:.3f}", flush=True)


# ------------------------------------------------------------------------------------------------
# the classifier launches
# ------------------------------------------------------------------------------------------------
def _classify(ops, dev, c, tail=None):
    """One launch of case `c` (HC.classifier_case) into fresh buffers -> (prob, featn or None, mem or None[, boxes_out, deltas_out]).
    `tail` = (layer, hb, boxes_in, with deltas_out, weights, clip): the fused `cascade_stage_tail` instead of `zs_classify`."""
    rows, C1, form, live = c["rows"], c["C1"], c["form"], c["live"]
    prob = _sent((rows + GUARD, C1), dev)
    if c["old"] is not None:
        keep = prob[:rows].cpu()
        keep[live] = c["old"][live]
        prob[:rows] = keep.to(dev)
    featn = _sent((rows + GUARD, 512), dev) if form == "stage0" else None
    mem = _sent((rows + GUARD, C1), dev) if form == "stage0" else None
    ps = c["ps"].to(dev) if form != "middle" else None
    kw = dict(zs_mem=None if c["zs_mem"] is None else c["zs_mem"].to(dev), prop_scores=ps, mem_scores_out=mem, final_inv_stages=c["inv"],
              batch=c["batch"], wide=c["order"] == "wide")
    args = (c["feat"].to(dev), c["zs"].to(dev), prob, form != "stage0", featn, _count(c["counts"], dev), c["R_cap"], C1, HC.TEMP)
    if tail is None:
        ops.zs_classify(*args, **kw)
        return prob, featn, mem
    layer, hb, boxes_in, with_deltas, weights, clip = tail
    boxes_out = _sent((rows + GUARD, 4), dev)
    deltas_out = _sent((rows + GUARD, 4), dev) if with_deltas else None
    ops.cascade_stage_tail(*args, hb, layer, boxes_in, boxes_out, weights, clip, HC.IMG_W, HC.IMG_H, deltas_out=deltas_out, **kw)
    return prob, featn, mem, boxes_out, deltas_out


def _check_classifier(family: str, tag: str, c, prob, featn, mem) -> None:
    rows, live, ref, emu, bound = c["rows"], c["live"], c["ref"], c["emu"], c["bound"]
    _untouched(f"{tag} prob", prob, live)
    _within(family, tag, "prob", prob[:rows], ref["out"], emu["out"], bound["out"], live)
    if c["form"] == "stage0":
        _untouched(f"{tag} featn", featn, live)
        _untouched(f"{tag} mem", mem, live)
        _within(family, tag, "featn", featn[:rows], ref["featn"], emu["featn"], bound["featn"], live)
        _within(family, tag, "mem", mem[:rows], ref["mem"], emu["mem"], bound["mem"], live)
        zero = live & (c["feat"].abs().amax(1) == 0)                        # the all-zero rows: featn = 0 and p = 0.5, exactly
        assert zero.any() or not live.any()
        assert torch.equal(featn[:rows].cpu()[zero], torch.zeros((int(zero.sum()), 512)))
        assert torch.equal(prob[:rows].cpu()[zero], torch.full((int(zero.sum()), c["C1"]), 0.5))
        excluded = live & (c["ps"] >= 1)                                    # p >= 1: the re-score is exactly 0
        assert torch.equal(mem[:rows].cpu()[excluded], torch.zeros((int(excluded.sum()), c["C1"])))


def _classifier_cases(order: str, C1: int):
    table = HC.NARROW_ROWS if order == "narrow" else HC.wide_rows(C1)
    for R_cap, counts, batch in table:
        for form in HC.FORMS:
            yield HC.classifier_case(order, C1, R_cap, counts, batch, form)


def _tag(c, extra: str = "") -> str:
    return f"{c['order']} C1 {c['C1']:4d} R {c['R_cap']:2d} x{c['batch']} count {str(c['counts']):10s} {c.get('form', ''):6s} {extra}"


@gpu
@pytest.mark.parametrize("C1", HC.NARROW_C1)
def test_narrow_classifier(dev, C1):
    """`zs_classify` with C1 <= 24 (one wave per row, four rows per workgroup, the class matrix staged in LDS): the row tables whose
    last workgroup is full, partly live, wholly dead and half beyond the buffer; a batch of three lists with counts 8, 0 and 3; the
    cascade's three forms; the hostile rows and proposal scores of _head_cases."""
    from embodied_object_detection_amd import ops
    for c in _classifier_cases("narrow", C1):
        _check_classifier("narrow classifier", _tag(c), c, *_twice(lambda: _classify(ops, dev, c)))
    _summary("narrow classifier")


@gpu
@pytest.mark.parametrize("C1", HC.WIDE_C1)
def test_wide_classifier(dev, C1):
    """`zs_classify(wide=True)` (32 x 32 tiles on the fp32 matrix cores, K in four quarters): one class tile and one column into the
    second, 32 and 33 columns, 1204; row tiles that are full, one row into the second, partly and wholly dead; a batch of three lists of
    36 rows (counts 36, 0, 5), so that a row tile straddles two lists."""
    from embodied_object_detection_amd import ops
    for c in _classifier_cases("wide", C1):
        _check_classifier("wide classifier", _tag(c), c, *_twice(lambda: _classify(ops, dev, c)))
    _summary("wide classifier")


def _memory_scores(ops, dev, family: str, c) -> None:
    R_cap, C1, live = c["R_cap"], c["C1"], c["live"]

    def run():
        out = _sent((R_cap + GUARD, C1), dev)
        ops.memory_scores(c["featn"].to(dev), c["zs"].to(dev), c["ps"].to(dev), out, _count(c["counts"], dev), R_cap, C1)
        return (out,)
    out, = _twice(run)
    tag = _tag(dict(c, batch=1), "memory_scores")
    _untouched(tag, out, live)
    _within(family, tag, "mem", out[:R_cap], c["ref"]["mem"], c["emu"]["mem"], c["bound"]["mem"], live)
    excluded = live & (c["ps"] >= 1)
    assert torch.equal(out[:R_cap].cpu()[excluded], torch.zeros((int(excluded.sum()), C1)))


@gpu
def test_wide_memory_scores(dev):
    """`memory_scores` with C1 > 24: the wide kernel on rows that are normalised already (its mode 2)."""
    from embodied_object_detection_amd import ops
    for order, C1, R_cap, counts in HC.rescore_table():
        if order == "wide":
            _memory_scores(ops, dev, "wide memory_scores", HC.rescore_case(order, C1, R_cap, counts))
    _summary("wide memory_scores")


@gpu
def test_narrow_memory_scores(dev):
    """`memory_scores` with C1 <= 24 (its own wave-per-row kernel) at 1, 255 and 257 rows with no count, count 0 and R_cap - 1."""
    from embodied_object_detection_amd import ops
    for order, C1, R_cap, counts in HC.rescore_table():
        if order == "narrow":
            _memory_scores(ops, dev, "narrow memory_scores", HC.rescore_case(order, C1, R_cap, counts))
    _summary("narrow memory_scores")


# ------------------------------------------------------------------------------------------------
# the BoxTail
# ------------------------------------------------------------------------------------------------
def _tail_layer(ops, dev, K: int):
    """bbox_pred.2 at width K through a real `ops.Conv` (its packing, its row stride, its bias).  `ops.Conv` takes multiples of 32
    channels only: widths 16 and 1040 are the layer over 32 / 1056 channels, whose columns beyond K hold other weights, handed over
    with `Cin = K` -- a row stride larger than the width, and weights a read beyond `hb_dim` would pick up."""
    w4, bias = HC.tail_layer(K)
    conv = ops.Conv(w4, bias, device=dev, name="bbox_pred.2")
    assert conv.Kpad == w4.shape[1] and conv.Kpad >= K
    return conv if conv.Cin == K else types.SimpleNamespace(w=conv.w, bias=conv.bias, Cin=K, Kpad=conv.Kpad)


@gpu
@pytest.mark.parametrize("order", ("narrow", "wide"))
def test_cascade_stage_tail(dev, order):
    """`cascade_stage_tail`: the classifier outputs bitwise those of `zs_classify` alone; deltas and boxes against float64."""
    from embodied_object_detection_amd import ops
    layers = {K: _tail_layer(ops, dev, K) for K in HC.TAIL_K}
    family = f"{order} BoxTail"
    for o, C1, R_cap, counts, batch, K, with_deltas, clip, form in HC.tail_table():
        if o != order:
            continue
        c = HC.classifier_case(order, C1, R_cap, counts, batch, form)
        t = HC.tail_case(K, c["rows"], HC.FORMS.index(form), clip)
        tail = (layers[K], t["hb"].to(dev), t["boxes"].to(dev), with_deltas, t["weights"], clip)
        prob, featn, mem, boxes, deltas = _twice(lambda: _classify(ops, dev, c, tail))
        alone = _classify(ops, dev, c)
        for a, b in zip((prob, featn, mem), alone):
            assert (a is None and b is None) or torch.equal(_bits(a), _bits(b)), "the fused launch's classifier outputs are not zs_classify's"
        tag = _tag(c, f"K {K} clip {int(clip)}")
        _untouched(f"{tag} boxes", boxes, c["live"])
        _within(family, tag, "boxes", boxes[:c["rows"]], t["box64"], t["box32"], t["b_box"], c["live"])
        if with_deltas:
            _untouched(f"{tag} deltas", deltas, c["live"])
            _within(family, tag, "deltas", deltas[:c["rows"]], t["d64"], t["d32"], t["b_d"], c["live"])
    _summary(family)


# ------------------------------------------------------------------------------------------------
# apply_deltas, cascade_scores
# ------------------------------------------------------------------------------------------------
@gpu
def test_apply_deltas(dev):
    """`apply_deltas` with a row stride of 4 and 8 at 1, 255 and 257 rows (one thread per row, 256 per workgroup), with no count, count 0
    and R_cap - 1, and over a batch of three lists with ragged counts; clip on and off."""
    from embodied_object_detection_amd import ops
    cases = [(R_cap, counts, 1) for R_cap in HC.SMALL_R for counts in (None, (0,), (R_cap - 1,))] + [(255, (255, 0, 17), 3), (257, (3, 257, 256), 3)]
    for ld in (4, 8):
        for i, (R_cap, counts, batch) in enumerate(cases):
            clip = bool((i + ld // 4) % 2)
            c = HC.deltas_case(R_cap, batch, ld, clip)
            live, rows = HC.live_rows(R_cap, counts, batch), R_cap * batch

            def run():
                out = _sent((rows + GUARD, 4), dev)
                ops.apply_deltas(c["d"].to(dev), ld, c["boxes"].to(dev), out, _count(counts, dev), R_cap, c["weights"], clip, HC.IMG_W, HC.IMG_H, batch=batch)
                return (out,)
            out, = _twice(run)
            tag = f"apply_deltas ld {ld} R {R_cap} x{batch} count {counts} clip {int(clip)}"
            _untouched(tag, out, live)
            _within("apply_deltas", tag, "boxes", out[:rows], c["box64"], c["box32"], c["b_box"], live)
    _summary("apply_deltas")


@gpu
def test_cascade_scores(dev):
    """`cascade_scores` in place on [R_cap, 21] at 1, 255 and 257 rows: the live rows fused, the others untouched."""
    from embodied_object_detection_amd import ops
    C1 = 21
    for R_cap in HC.SMALL_R:
        c = HC.fusion_case(R_cap, C1)
        acc, ps = c["acc"], c["ps"]
        for counts in (None, (0,), (R_cap - 1,)):
            live = HC.live_rows(R_cap, counts, 1)

            def run():
                buf = _sent((R_cap + GUARD, C1), dev)
                keep = buf[:R_cap].cpu()
                keep[live] = acc[live]
                buf[:R_cap] = keep.to(dev)
                ops.cascade_scores(buf, ps.to(dev), _count(counts, dev), R_cap, C1, HC.INV3)
                return (buf,)
            buf, = _twice(run)
            tag = f"cascade_scores R {R_cap} count {counts}"
            _untouched(tag, buf, live)
            _within("cascade_scores", tag, "scores", buf[:R_cap], c["ref"], c["emu"], c["bound"], live)
    _summary("cascade_scores")


# ------------------------------------------------------------------------------------------------
# detector_postprocess
# ------------------------------------------------------------------------------------------------
def _postprocess(ops, dev, cap, batch, counts, sx, sy, with_remap, all_dropped=False) -> None:
    boxes, scores, classes, remap, (out_w, out_h) = HC.post_inputs(cap, batch, sx, sy, cap + 7 * batch, all_dropped)

    def run():
        outs = (_sent((batch * cap + GUARD, 4), dev), _sent((batch * cap + GUARD,), dev), _sent((batch * cap + GUARD,), dev, torch.int32),
                _sent((batch * cap + GUARD,), dev, torch.int32), _sent((batch + GUARD,), dev, torch.int32))
        ops.detector_postprocess(boxes.to(dev), scores.to(dev), classes.to(dev), _count(counts, dev), cap, sx, sy, out_w, out_h, *outs,
                                 remap=remap.to(dev) if with_remap else None, batch=batch)
        return outs
    ob, os_, oc, osrc, ocount = (t.cpu() for t in _twice(run))
    tag = f"postprocess cap {cap} x{batch} count {counts} scale ({sx}, {sy}) remap {int(with_remap)}"
    kept = []
    live = torch.zeros(batch * cap, dtype=torch.bool)
    for b in range(batch):
        s = slice(b * cap, (b + 1) * cap)
        rb, rs, rc, rsrc, n = HC.postprocess(boxes[s], scores[s], classes[s], None if counts is None else counts[b], cap, sx, sy, out_w, out_h,
                                             remap[s] if with_remap else None)
        kept.append(n)
        live[b * cap:b * cap + n] = True
        o = b * cap
        assert int(ocount[b]) == n, f"{tag}: scene {b} kept {int(ocount[b])}, the reference {n}"
        assert torch.equal(_bits(ob[o:o + n]), _bits(rb)) and torch.equal(_bits(os_[o:o + n]), _bits(rs)), f"{tag}: boxes or scores differ"
        assert torch.equal(oc[o:o + n], rc) and torch.equal(osrc[o:o + n], rsrc), f"{tag}: classes or sources differ"
    for name, buf in (("boxes", ob), ("scores", os_), ("classes", oc), ("src", osrc)):
        _untouched(f"{tag} {name}", buf, live)
    _untouched(f"{tag} count", ocount, torch.ones(batch, dtype=torch.bool))
    print(f"{tag:90s} kept {kept}: exact", flush=True)
    if all_dropped:
        assert sum(kept) == 0
    return kept


@gpu
def test_detector_postprocess(dev):
    """`detector_postprocess` against the same fp32 arithmetic on the CPU, exactly: boxes, scores, classes, sources, count, order and the
    untouched tail, at 1, 16 and 512 slots (the kernel's limit: one thread per slot), three pairs of scale factors, with no count, count
    0 and cap, with and without `remap`; every box dropped; a batch of three scenes with ragged counts; 513 slots refused."""
    from embodied_object_detection_amd import ops
    from embodied_object_detection_amd._lib import EodError
    some_dropped = some_kept = False
    for sx, sy in HC.POST_SCALES:
        for cap in HC.POST_CAPS:
            for counts in (None, (0,), (cap,)):
                for with_remap in (False, True):
                    n = _postprocess(ops, dev, cap, 1, counts, sx, sy, with_remap)[0]
                    D = 0 if counts == (0,) else cap
                    some_dropped, some_kept = some_dropped or n < D, some_kept or n > 0
        _postprocess(ops, dev, 16, 1, None, sx, sy, True, all_dropped=True)
        _postprocess(ops, dev, 16, 3, (16, 0, 7), sx, sy, True)
        _postprocess(ops, dev, 512, 3, (1, 512, 300), sx, sy, False)
    assert some_dropped and some_kept
    t = torch.zeros((513 * 4,), device=dev)
    i = torch.zeros((513,), dtype=torch.int32, device=dev)
    outs = (_sent((513, 4), dev), _sent((513,), dev), _sent((513,), dev, torch.int32), _sent((513,), dev, torch.int32), _sent((1,), dev, torch.int32))
    with pytest.raises(EodError, match="EOD_ERR_CAPACITY"):
        ops.detector_postprocess(t, t, i, None, 513, 1.0, 1.0, 80.0, 60.0, *outs)
    torch.cuda.synchronize()
    for o in outs:                                                            # refused before any launch: nothing was written
        _untouched("postprocess cap 513", o.cpu(), torch.zeros(0, dtype=torch.bool))


# ------------------------------------------------------------------------------------------------
# mask predictor
# ------------------------------------------------------------------------------------------------
@gpu
def test_mask_predictor(dev):
    """`mask_predictor_sigmoid` (one wave per row, 256 channels per trip, a grid-stride loop over the rows): one lane, one full trip and a
    second trip of the channel loop; units of 4 and 784 rows; the count cutting whole units; the scatter through `out_units` into a
    larger output; 32772 rows, which 8192 workgroups of four waves reach only in a second pass."""
    from embodied_object_detection_amd import ops
    for C, unit_rows, units, count, scatter in HC.mask_table():
        c = HC.mask_case(C, unit_rows, units)
        rows = units * unit_rows
        n_live = units if count is None else count
        place = HC.scatter_units(units) if scatter else torch.arange(units).int()
        out_units = units + 2 if scatter else units
        cnt = None if count is None else torch.tensor([count], dtype=torch.int32, device=dev)

        def run():
            out = _sent((out_units * unit_rows + GUARD,), dev)
            ops.mask_predictor_sigmoid(c["x"].to(dev), c["w"].to(dev), HC.MASK_BIAS, rows, C, cnt, unit_rows, out=out,
                                       out_units=place.to(dev) if scatter else None)
            return (out,)
        out, = _twice(run)
        out = out.cpu()
        src = torch.arange(n_live * unit_rows)                                 # compact row -> its row of the output
        dst = place.long()[src // unit_rows] * unit_rows + src % unit_rows
        live = torch.zeros(out_units * unit_rows, dtype=torch.bool)
        live[dst] = True
        tag = f"mask predictor C {C} unit {unit_rows} x{units} count {count} scatter {int(scatter)}"
        _untouched(tag, out, live)
        _within("mask predictor", tag, "prob", out[dst], c["p64"][src], c["p32"][src], c["b_p"][src])
    _summary("mask predictor")


# ------------------------------------------------------------------------------------------------
# the references' own checks (no GPU)
# ------------------------------------------------------------------------------------------------
def _inside(tag: str, emu: torch.Tensor, ref: torch.Tensor, bound: torch.Tensor) -> float:
    share = float(HC.share((emu.double() - ref).abs(), bound.expand_as(ref)).max()) if ref.numel() else 0.0
    assert share <= 1.0, f"{tag}: the fp32 emulation is at {share:.3f} of the bound"
    return share


def test_fp32_emulation_stays_inside_every_bound():
    """Every bound of _head_cases holds for a CPU fp32 computation in the kernel's own summation order, on EVERY case of the tables (all
    rows, live or not): a bound below that would be a wrong derivation, not a finding about a kernel."""
    worst: Dict[str, float] = {}

    def note(family, share):
        worst[family] = max(worst.get(family, 0.0), share)
    for order, C1, R_cap, counts, batch in HC.classifier_table():
        for form in HC.FORMS:
            c = HC.classifier_case(order, C1, R_cap, counts, batch, form)
            for k in c["bound"]:
                note(f"{order} classifier {k}", _inside(f"{_tag(c)} {k}", c["emu"][k], c["ref"][k], c["bound"][k]))
    for order, C1, R_cap, counts in HC.rescore_table():
        c = HC.rescore_case(order, C1, R_cap, counts)
        for k in ("mem_logit", "mem"):
            note(f"{order} memory_scores {k}", _inside(f"memory_scores {order} {C1} {R_cap} {k}", c["emu"][k], c["ref"][k], c["bound"][k]))
    for order, C1, R_cap, counts, batch, K, with_deltas, clip, form in HC.tail_table():
        t = HC.tail_case(K, R_cap * batch, HC.FORMS.index(form), clip)
        note("BoxTail deltas", _inside(f"tail K {K} rows {R_cap * batch} deltas", t["d32"], t["d64"], t["b_d"]))
        note("BoxTail boxes", _inside(f"tail K {K} rows {R_cap * batch} clip {clip} boxes", t["box32"], t["box64"], t["b_box"]))
    for ld in (4, 8):
        for R_cap, batch in [(r, 1) for r in HC.SMALL_R] + [(255, 3), (257, 3)]:
            for clip in (False, True):
                c = HC.deltas_case(R_cap, batch, ld, clip)
                note("apply_deltas", _inside(f"apply_deltas R {R_cap} x{batch} ld {ld}", c["box32"], c["box64"], c["b_box"]))
    for R_cap in HC.SMALL_R:
        c = HC.fusion_case(R_cap)
        note("cascade_scores", _inside(f"cascade_scores R {R_cap}", c["emu"], c["ref"], c["bound"]))
    for C, unit_rows, units, count, scatter in HC.mask_table():
        c = HC.mask_case(C, unit_rows, units)
        note("mask predictor", _inside(f"mask C {C} unit {unit_rows} x{units}", c["p32"], c["p64"], c["b_p"]))
    for k, v in sorted(worst.items()):
        print(f"fp32 emulation, {k:32s} at most {v:.3f} of its bound")
    # the bounds bite: a dropped channel of a lane (one of 512 products) is far beyond the logit's bound on a plain row
    c = HC.classifier_case("narrow", 21, 64, (50,), 1, "stage0")
    plain = 6                                                                  # kind 6 of feature_rows
    drop = (c["ref"]["featn"][plain, 7] * c["zs"].double()[7]).abs()
    assert float((drop / c["bound"]["logit"][plain]).median()) > 50


def test_references_are_the_oracles():
    """Every float64 reference against the committed oracle's fp32 statement of the same upstream code, at fp32 tolerance."""
    from oracle import model as M
    from oracle import ops as OO
    g = torch.Generator().manual_seed(5)
    R, C1, K = 40, 21, 64
    sd = {}
    p = "roi_heads.box_predictor.0"
    for name, shape in (("roi_heads.box_head.0.fc1", (32, 18)), ("roi_heads.box_head.0.fc2", (32, 32)), (f"{p}.cls_score.linear", (512, 32)),
                        (f"{p}.bbox_pred.0", (K, 32)), (f"{p}.bbox_pred.2", (4, K))):
        sd[f"{name}.weight"] = torch.randn(shape, generator=g) / shape[1] ** 0.5
        sd[f"{name}.bias"] = torch.randn((shape[0],), generator=g) * 0.1
    zs = HC.class_matrix(C1, 0)
    sd[f"{p}.cls_score.zs_weight"] = zs
    pooled = torch.randn((R, 2, 3, 3), generator=g)
    logits, deltas, feat = M.box_head_stage(pooled, sd, 0, M.OracleCfg())
    x = F.relu(F.linear(F.relu(F.linear(pooled.flatten(1), sd["roi_heads.box_head.0.fc1.weight"], sd["roi_heads.box_head.0.fc1.bias"])),
                        sd["roi_heads.box_head.0.fc2.weight"], sd["roi_heads.box_head.0.fc2.bias"]))
    hb = F.relu(F.linear(x, sd[f"{p}.bbox_pred.0.weight"], sd[f"{p}.bbox_pred.0.bias"]))
    # the cascade's scores (oracle/model.py cascade_box_heads): three stages on the same features, then the fusion with the proposal score
    ps = torch.rand((R,), generator=g)
    r0 = HC.classifier(feat, zs, "narrow", F64)
    r2 = HC.classifier(feat, zs, "narrow", F64, old=2 * r0["out"].float(), inv=1.0 / 3, ps=ps)
    torch.testing.assert_close(r0["featn"].float(), M.OracleCfg().norm_temp * F.normalize(feat, p=2, dim=1), rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(r0["logit"].float(), logits, rtol=1e-5, atol=1e-4)
    probs = torch.sigmoid(logits)
    torch.testing.assert_close(r2["out"].float(), ((probs + probs + probs) * (1.0 / 3) * ps[:, None]) ** 0.5, rtol=1e-5, atol=1e-7)
    torch.testing.assert_close(HC.fusion(3 * probs, 1.0 / 3, ps, F64).float(), ((probs + probs + probs) * (1.0 / 3) * ps[:, None]) ** 0.5, rtol=1e-5, atol=1e-7)
    # the memory update's re-score (oracle/memory.py inference_with_proposals): proposals with ps < 1 only, sqrt(sigmoid * ps)
    ps[3], ps[4] = 1.0, 1.5
    rm = HC.classifier(feat, zs, "narrow", F64, ps=ps, zs_mem=zs)
    sel = torch.where(ps < 1)[0]
    sc = (torch.mm(50.0 * F.normalize(feat[sel], p=2, dim=1), zs).sigmoid() * ps[sel, None]) ** 0.5
    torch.testing.assert_close(rm["mem"].float()[sel], sc, rtol=1e-5, atol=1e-7)
    assert float(rm["mem"][3].abs().max()) == 0 and float(rm["mem"][4].abs().max()) == 0
    # bbox_pred.2 and Box2BoxTransform + clip
    d64 = hb.double() @ sd[f"{p}.bbox_pred.2.weight"].double().t() + sd[f"{p}.bbox_pred.2.bias"].double()
    torch.testing.assert_close(d64.float(), deltas, rtol=1e-5, atol=1e-5)
    boxes = HC.hostile_boxes(R, 3)
    d = deltas * 3
    d[0, 2], d[1, 3] = 100.0, 60.0                                          # past the clamp
    for w in HC.CASCADE_WEIGHTS:
        torch.testing.assert_close(HC.box_transform(d, boxes, w, False, HC.IMG_W, HC.IMG_H, F64).float(), OO.apply_deltas(d, boxes, w), rtol=1e-5, atol=1e-3)
        torch.testing.assert_close(HC.box_transform(d, boxes, w, True, HC.IMG_W, HC.IMG_H, F64).float(),
                                   OO.clip_boxes(OO.apply_deltas(d, boxes, w), (int(HC.IMG_H), int(HC.IMG_W))), rtol=1e-5, atol=1e-3)
    # detector_postprocess: scale factors that are fp32 numbers, so that the oracle's multiplication is the reference's
    W, H = HC.POST_IN
    for sx, sy in ((1.0, 1.0), (0.75, 2.5)):
        boxes, scores, classes, _, _ = HC.post_inputs(16, 1, sx, sy, 9)
        out_hw = (int(H * sy), int(W * sx))
        ref = M.detector_postprocess(boxes, scores, classes, torch.rand((16, 1, 28, 28), generator=g), (int(H), int(W)), out_hw, M.OracleCfg())
        rb, rs, rc, rsrc, n = HC.postprocess(boxes, scores, classes, None, 16, sx, sy, float(out_hw[1]), float(out_hw[0]))
        assert 0 < n < 16 and torch.equal(rb, ref["pred_boxes"]) and torch.equal(rs, ref["scores"]) and torch.equal(rc, ref["pred_classes"])
    # the mask predictor: a 1x1 convolution to one channel, then the sigmoid (oracle/model.py mask_head)
    c = HC.mask_case(260, 4, 3)
    x = c["x"].view(3, 2, 2, 260).permute(0, 3, 1, 2).contiguous()
    ref = torch.sigmoid(F.conv2d(x, c["w"].view(1, 260, 1, 1), torch.tensor([HC.MASK_BIAS])))
    torch.testing.assert_close(c["p64"].float().view(3, 1, 2, 2), ref, rtol=1e-5, atol=1e-7)


if __name__ == "__main__":
    sys.exit(pytest.main([__file__, "-s", "-q"] + sys.argv[1:]))
