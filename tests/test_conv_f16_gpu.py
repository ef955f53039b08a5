"""The f16 convolution arithmetic on the GPU: y = epilogue(sum_k half(x)_k * half(w)_k), fp32 accumulate, fp32 output.

Everything is compared with float64 on the CPU.  The reference of a call that gets the f16 family is the operation on the operands
rounded to half (`x.half().double()`, `w.half().double()`): what is left is fp32 accumulation noise, measured with the yardstick of
tests/test_conv_plans_gpu.py (torch's CPU fp32 result on the same rounded operands).  A kernel that rounds to bf16, truncates, or
accumulates in half is far outside it.  The case list of the production plans is that module's recording of the full-size frames.
"""
import copy
import dataclasses
import math
from typing import List

import pytest
import torch
import torch.nn.functional as F

from test_conv_plans_gpu import (SENTINEL, SIZES, Call, _active_units, _ceiling, _cpu_op, _Device, _gn_partials_ok, _inputs, _layer,  # noqa: F401
                                 _plan_in, _rows_call, _single_calls, _unit_counts, dev, recorded)

pytestmark = pytest.mark.gpu

# what make_plan hands back to the fp32 kernel in f16 mode: the 4-channel stem (tap4), in_relu (P7), the fused mask
# tail (out_mode 2) and gated layers (training only)
FP32_LAYERS = {"stem", "p7", "mask_deconv"}


def _stays_fp32(c: Call) -> bool:
    return bool(c.conv.tap4 or c.in_relu or c.fuse or c.gate)


def _rounded(c: Call, inp: dict):
    """The call on operands rounded to half: a copy of the layer with rounded weights, the inputs with a rounded x."""
    conv = copy.copy(c.conv)
    conv.w = c.conv.w.half().float()
    return dataclasses.replace(c, conv=conv), dict(inp, x=inp["x"].half().float())


def _family(c: Call, plan: dict) -> str:
    if plan["wavek"]:
        return f"fp32 wave-K {plan['wavek']} waves"
    if plan["tile"] == 5:
        return "fp32 64x256 fused tail"
    kern = {0: "fp32", 2: "bf16x3", 3: "f16"}[plan["glds"]] + f" {plan['bm']}x{plan['bn']} BK{plan['bk']}"
    if plan["splitk"] == 1:
        return kern
    rows = c.plan_rows if 0 < c.plan_rows < c.M else c.M
    tiles = -(-rows // plan["bm"]) * plan["tiles_n"]
    return f"{kern} split-K ({'slabs, few tiles' if tiles < 256 else 'slabs, mid split'}{', GroupNorm statistics' if plan['gn_fused'] else ''})"


def _check(c: Call, dev, tag: str, seed: int, want_f16=None) -> List[str]:
    """Replays the call alone in f16 mode against fp64 -> what is wrong with it (empty = fine); one line per count is printed."""
    from embodied_object_detection_amd import ops
    bad = []
    for which in ((0, 1) if c.m_count else (0,)):
        counts = _unit_counts(c, which)
        inp = _inputs(c, seed, counts)
        units = _active_units(c, counts)
        d = _Device(c, inp, dev)
        prev = ops.set_conv_math("f16")
        try:
            out, out2, gn_ws = d.launch()
            plan = c.conv.plan()
        finally:
            ops.set_conv_math(prev)
        torch.cuda.synchronize()
        is_f16 = plan["glds"] == 3
        who = f"{c.conv.name} [f16{'' if counts is None else f', counts {counts}'}]"
        if want_f16 is not None and is_f16 != want_f16:
            bad.append(f"{who}: got the {'f16' if is_f16 else 'fp32'} family (plan {plan})")
        if is_f16 and (c.conv.w_half is None or plan["wavek"]):
            bad.append(f"{who}: f16 family without a half weight copy, or on the wave-K kernel")
        rc, rinp = _rounded(c, inp) if is_f16 else (c, inp)
        ref = _cpu_op(rc, rinp, units, torch.float64)
        e32v = (_cpu_op(rc, rinp, units, torch.float32).double() - ref).abs()
        scale = float(ref.abs().mean())
        e32 = (float(e32v.mean()) / scale, float(e32v.max()) / scale)
        ev = (d.values(out, out2, units) - ref).abs()
        e = (float(ev.mean()) / scale, float(ev.max()) / scale)
        print(f"{tag:15s} {c.conv.name[-44:]:44s} M {c.M:7d} K {c.conv.Kpad:5d} Cout {c.conv.Cout:4d} -> {_family(c, plan):56s} "
              f"tiles {plan['tiles_m']}x{plan['tiles_n']} splitk {plan['splitk']}x{plan['cps']}  err/scale mean {e[0]:.2e} max {e[1]:.2e}"
              f"  cpu fp32 mean {e32[0]:.2e} max {e32[1]:.2e}" + ("" if counts is None else f"  counts {counts}"), flush=True)
        if not math.isfinite(e[1]):
            bad.append(f"{who}: non-finite output")
        if e[0] > 2.5 * e32[0]:
            bad.append(f"{who}: mean error {e[0]:.3e} of scale > 2.5 x the CPU fp32 convolution's {e32[0]:.3e} on the same rounded operands")
        if e[1] > 4.0 * e32[1]:
            bad.append(f"{who}: max error {e[1]:.3e} of scale > 4 x the CPU fp32 convolution's {e32[1]:.3e} on the same rounded operands")
        if e[0] > _ceiling(c.conv.Kpad):
            bad.append(f"{who}: mean error {e[0]:.3e} of scale above the ceiling {_ceiling(c.conv.Kpad):.0e}")
        if c.m_count and not d.untouched(out, out2, units):
            bad.append(f"{who}: rows beyond the device-side count were written")
        if c.gn_stats and plan["gn_fused"]:
            rel = _gn_partials_ok(c, out, gn_ws)
            if not rel < 1e-9:
                bad.append(f"{who}: GroupNorm partial sums of the slab reduce differ from the stored values' sums by {rel:.2e}")
    return bad


# ------------------------------------------------------------------------------------------------
# 1. exact rounding, 2. the hard bound, 3. range
# ------------------------------------------------------------------------------------------------
F16_TILES = {83: (3, 64, 64), 84: (4, 256, 64), 93: (3, 64, 32), 94: (4, 256, 32)}      # force_tile -> (tile, bm, bk)


@pytest.mark.parametrize("tile", [0, 83, 84, 93, 94])
@pytest.mark.parametrize("splitk", [0, 3])
def test_f16_kernels_round_exactly_with_every_epilogue(dev, tile, splitk):
    """Each f16 kernel (the planner's choice and each tile forced, BK 64 and 32) with the epilogues the fp32 kernel has, stride 2,
    Cin % 64 != 0, a deconv layer, device-side counts, unit lists, two stacked linear layers and pyramid mode with GroupNorm
    statistics, with and without slabs: the error against fp64 on the rounded operands is fp32 accumulation noise."""
    bad = []
    fk = dict(force_tile=tile, force_splitk=splitk)
    layers = [("res_mode 1 + relu", dict(res_mode=1, relu=True), (128, 192, 3, 1)), ("res_mode 2 (x2 residual)", dict(res_mode=2), (256, 256, 1, 1)),
              ("out_scale", dict(out_scale=0.37, relu=True), (64, 96, 3, 1)), ("stride 2", dict(relu=True), (128, 256, 3, 2)),
              ("stride 2, 1x1", dict(), (256, 512, 1, 2)), ("Cin 96: BK 32 only", dict(relu=True), (96, 80, 3, 1)),
              ("Cin 32, 5x5", dict(), (32, 64, 5, 1))]
    calls = []
    for name, f, (Cin, Cout, k, stride) in layers:
        calls.append(Call(_layer(dev, Cin, Cout, k, stride, seed=len(calls), name=name), 2, 38, 46, **f, **fk))
    calls.append(Call(_layer(dev, 256, 64, seed=10, name="deconv (out_mode 1)", deconv=True), 6, 14, 14, relu=True, **fk))
    calls.append(Call(_layer(dev, 256, 256, 3, seed=11, name="device-side count, 14x14 units"), 40, 14, 14, relu=True, m_count=True,
                      m_unit=196, **fk))
    calls.append(Call(_layer(dev, 1024, 1536, 1, seed=12, name="stacked linear layers (split)"), 320, 1, 1, relu=True, m_count=True,
                      m_unit=1, split_n=512, **fk))
    calls.append(Call(_layer(dev, 1024, 1536, 1, seed=13, name="4 unit lists (m_segments)"), 4 * 80, 1, 1, relu=True, m_count=True,
                      m_unit=1, m_segments=4, split_n=512, **fk))
    shapes = ((40, 52), (20, 26), (10, 13), (5, 7), (3, 4))
    off = [0]
    for h, w in shapes:
        off.append(off[-1] + h * w)
    calls.append(Call(_layer(dev, 256, 256, 3, seed=14, name="pyramid + GroupNorm statistics"), 1, 0, 0, levels=(tuple(off), shapes),
                      gn_stats=True, **fk))
    for i, c in enumerate(calls):
        bad += _check(c, dev, f"tile={tile} sk={splitk}", 9500 + i, want_f16=True)
        plan = c.conv.plan() if tile else _plan_in(c.conv, "f16")
        assert plan["glds"] == 3 and plan["wavek"] == 0, (c.conv.name, plan)
        if tile:
            t, bm, bk = F16_TILES[tile]
            assert (plan["tile"], plan["bm"]) == (t, bm) and plan["bk"] == (bk if c.conv.Cin % 64 == 0 else 32), (c.conv.name, plan)
        if splitk:          # the slabs the forced count leaves once every slab holds whole chunks (K = 256 in 4 chunks of 64: 2 slabs)
            cps = -(-plan["nchunks"] // splitk)
            assert plan["cps"] == cps and plan["splitk"] == -(-plan["nchunks"] // cps) > 1, (c.conv.name, plan)
        if c.gn_stats:
            assert plan["gn_fused"] == int(plan["splitk"] > 1), plan
    assert not bad, "\n".join(bad)


def test_half_weight_copy_is_rne_and_the_kernels_agree_with_and_without_it(dev):
    """eod_conv_half_weights == torch's round-to-nearest-even .half(), bit for bit (ties, overflow to inf, subnormals, NaN); a launch
    that rounds the fp32 weights itself (presplit=False: no copy passed) gives bitwise the launch with the copy."""
    from embodied_object_detection_amd import _lib, ops
    lib = _lib.load()
    g = torch.Generator().manual_seed(3)
    w = torch.randn((96, 320), generator=g)
    w[0, :8] = torch.tensor([1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, 65504.0, 65519.9, 65520.0, -1e6, 2.0 ** -24, 2.0 ** -25])   # ties, range
    w[1, :6] = torch.tensor([2.0 ** -14 - 2.0 ** -25, 3e-6, -7e-8, 2.9e-8, float("inf"), float("nan")])
    wd = w.to(dev)
    out = torch.empty((lib.eod_conv_half_weights_bytes(96, 320),), dtype=torch.uint8, device=dev)
    ops.check(lib.eod_conv_half_weights(wd.data_ptr(), 96, 320, out.data_ptr(), None), "eod_conv_half_weights")
    torch.cuda.synchronize()
    assert torch.equal(out.view(torch.int16).cpu(), w.half().view(torch.int16).reshape(-1))
    for tile in (83, 84, 93, 94):
        conv = _layer(dev, 128, 192, 3, seed=5, name="copy or not")
        x = torch.randn((2, 37, 41, 128), generator=g).to(dev)
        y0 = conv(x, 2, 37, 41, relu=True, force_tile=tile, presplit=False)
        y1 = conv(x, 2, 37, 41, relu=True, force_tile=tile)
        assert conv.w_half is not None and torch.equal(y0, y1), tile


@pytest.mark.parametrize("Cin,k", [(32, 1), (64, 1), (64, 3), (256, 3)])
def test_hard_bound_against_the_unrounded_result(dev, Cin, k):
    """|y - y64| <= (2^-10 + 2^-22) * conv(|x|, |w|) + fp32 noise, element-wise, y64 the fp64 convolution of the UNROUNDED operands:
    two roundings of at most 2^-11 each (operands drawn inside half's normal range, so the rounding error is relative), the noise at
    most one fp32 ulp of the absolute sum per accumulated term.  First principles, no fitted constant; at small K a bf16 rounding
    (2^-9 per operand) breaks it."""
    g = torch.Generator().manual_seed(100 + Cin + k)
    N, H, W, Cout = 2, 33, 47, 96

    def draw(shape, scale):          # magnitudes in [0.25, 1) * scale with random signs: never subnormal as a half
        return (0.25 + 0.75 * torch.rand(shape, generator=g)) * scale * (torch.randint(0, 2, shape, generator=g) * 2 - 1)

    x = draw((N, Cin, H, W), 2.0)
    w = draw((Cout, Cin, k, k), (1.0 / (Cin * k * k)) ** 0.5)
    b = torch.randn((Cout,), generator=g)
    from embodied_object_detection_amd import ops
    conv = ops.Conv(w, b, stride=1, pad=k // 2, device=dev, name="bound")
    y64 = F.conv2d(x.double(), w.double(), b.double(), padding=k // 2)
    mag = F.conv2d(x.double().abs(), w.double().abs(), None, padding=k // 2) + b.double().abs().view(1, -1, 1, 1)
    K = Cin * k * k
    bound = (2.0 ** -10 + 2.0 ** -22) * mag + (K + 2) * 2.0 ** -23 * mag
    xd = x.permute(0, 2, 3, 1).contiguous().to(dev)
    used = []
    for tile in (83, 84, 93, 94, 0):
        prev = ops.set_conv_math("f16")
        try:
            y = conv(xd, N, H, W, force_tile=tile).cpu().permute(0, 3, 1, 2).double()
        finally:
            ops.set_conv_math(prev)
        err = (y - y64).abs()
        worst = float((err / bound).max())
        used.append(worst)
        print(f"hard bound Cin {Cin} k {k} tile {tile}: max |y - y64| / bound = {worst:.3f}, rms error / rms y = "
              f"{float(err.pow(2).mean().sqrt() / y64.pow(2).mean().sqrt()):.2e}", flush=True)
        assert worst <= 1.0, (tile, worst)
    # the rounding is really there: an fp32-class result would sit three orders of magnitude below the bound
    assert min(used) > 0.01, used


def test_range_overflow_subnormals_inf_and_nan(dev):
    """Inputs beyond half's range become inf, half subnormals are kept (not flushed), inf and NaN propagate as IEEE says, 0 * inf = NaN
    included: the positions of inf / NaN equal those of the fp64 reference on `.half()`-rounded operands, the rest agrees."""
    from embodied_object_detection_amd import ops
    g = torch.Generator().manual_seed(77)
    N, H, W, Cin, Cout = 1, 20, 30, 64, 64
    x = torch.randn((N, H, W, Cin), generator=g)
    w = torch.randn((Cout, Cin, 1, 1), generator=g) * 0.125
    x[0, 2, 3, 5] = 70000.0              # > 65504: +inf as a half
    x[0, 4, 1, 9] = -1.0e9               # -inf
    x[0, 6, 6, 0] = 65519.0              # rounds down to 65504: stays finite
    x[0, 8, 2, 7] = float("inf")
    x[0, 9, 9, 9] = float("nan")
    x[0, 11, 4, 1], x[0, 11, 4, 2] = 80000.0, -80000.0     # +inf and -inf in one row: NaN wherever both weights are non-zero
    w[3, 5, 0, 0] = 0.0                  # 0 * inf = NaN at (2, 3) channel 3
    w[7, 1, 0, 0] = 0.0                  # row (11, 4), channel 7: 0 * inf = NaN as well
    x[0, 15] = (torch.arange(W * Cin).view(W, Cin) % 1023 + 1).float() * 2.0 ** -24      # a whole image row of half subnormals (exact)
    x[0, 16] = torch.randn((W, Cin), generator=g) * 2e-6                                  # subnormals that need rounding
    xh, wh = x.half().double().permute(0, 3, 1, 2), w.half().double()
    ref = F.conv2d(xh, wh).permute(0, 2, 3, 1)
    mag = F.conv2d(xh.abs(), wh.abs()).permute(0, 2, 3, 1)      # finite wherever ref is: the yardstick of the fp32 accumulation
    fin = ref.isfinite()
    assert ref.isnan().any() and ref.isinf().any() and ref[0, 15].abs().min() > 0 and mag[fin].isfinite().all()
    conv = ops.Conv(w, None, device=dev, name="range")
    xd = x.to(dev)
    for tile, sk in ((83, 1), (84, 1), (93, 1), (94, 1), (83, 2), (0, 0)):
        prev = ops.set_conv_math("f16")
        try:
            y = conv(xd, N, H, W, force_tile=tile, force_splitk=sk).cpu().double()
        finally:
            ops.set_conv_math(prev)
        assert torch.equal(y.isnan(), ref.isnan()), (tile, sk, int(y.isnan().sum()), int(ref.isnan().sum()))
        assert torch.equal(y.isinf(), ref.isinf()) and torch.equal(y[ref.isinf()], ref[ref.isinf()]), (tile, sk)
        worst = float(((y[fin] - ref[fin]).abs() / (Cin * 2.0 ** -23 * mag[fin])).max())     # one fp32 ulp of the absolute sum per term
        assert worst <= 1.0, (tile, sk, worst)
        sub = y[0, 15:17]
        assert float((sub != 0).double().mean()) > 0.99, (tile, sk)                           # subnormal halves are not flushed to zero
        print(f"range tile {tile} splitk {sk}: {int(y.isnan().sum())} NaN, {int(y.isinf().sum())} inf at the reference's positions; finite "
              f"values within {worst:.3f} of the fp32 accumulation bound; subnormal rows non-zero", flush=True)


# ------------------------------------------------------------------------------------------------
# 4. every production plan
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", list(SIZES))
def test_production_calls_match_fp64_in_f16_mode(dev, recorded, size):
    """Every distinct eod_conv2d call of the full-size frames, replayed in f16 mode with the planner's own choice: the f16 family for
    every layer but the documented fp32 ones, fp32 accumulation noise against fp64 on the rounded operands."""
    bad, fams, fp32_names = [], {}, set()
    for i, c in enumerate(recorded[size]):
        assert c.force_tile == 0 and c.force_splitk == 0
        bad += _check(c, dev, size, 1000 + i, want_f16=not _stays_fp32(c))
        plan = _plan_in(c.conv, "f16")
        fams.setdefault(_family(c, plan), []).append(c.conv.name)
        if plan["glds"] != 3:
            fp32_names.add(c.conv.name)
    for f, names in sorted(fams.items()):
        print(f"{size:15s} f16     {f:70s} {len(names):3d} calls, e.g. {names[0]}")
    assert fp32_names == FP32_LAYERS, f"layers on the fp32 kernel in f16 mode: {sorted(fp32_names)}, documented: {sorted(FP32_LAYERS)}"
    assert any(f.startswith("f16 256x128") for f in fams) and any(f.startswith("f16 64x64") and "split-K" in f for f in fams), sorted(fams)
    assert not any(f.startswith("bf16x3") for f in fams), sorted(fams)
    assert all(set(names) <= FP32_LAYERS for f, names in fams.items() if not f.startswith("f16")), sorted(fams)
    assert not bad, f"{len(bad)} findings:\n" + "\n".join(bad)


def test_batch_of_4_is_bitwise_4_single_image_calls_in_f16_mode(dev, recorded):
    """Tile and split-K are decided on plan_rows: every call of the 960x960 batch of 4 writes bitwise what the four single-scene calls
    write on the same inputs."""
    from embodied_object_detection_amd import ops
    B = SIZES["960x960_batch4"][4]
    bad = []
    prev = ops.set_conv_math("f16")
    try:
        for i, c in enumerate(recorded["960x960_batch4"]):
            counts = _unit_counts(c, 0)
            inp = _inputs(c, 5000 + i, counts)
            d = _Device(c, inp, dev)
            out, out2, _ = d.launch()
            plan = c.conv.plan()
            s_out, s_out2 = d.out_buffers()
            for where, sc, cb in _single_calls(c, B, counts):
                if c.levels is not None:
                    o, _o2, _ws = _Device(sc, {"x": inp["x"][where]}, dev).launch()
                    s_out[where.to(dev)] = o
                elif c.fuse:
                    _Device(sc, inp, dev, share=d).launch(out=s_out, units=where, counts=cb)
                else:
                    rows = slice(where.start * (s_out.shape[0] // c.N), where.stop * (s_out.shape[0] // c.N))
                    _Device(sc, inp, dev, share=d).launch(out=s_out[rows], out2=None if s_out2 is None else s_out2[rows], units=where, counts=cb)
            torch.cuda.synchronize()
            if not (torch.equal(out, s_out) and (out2 is None or torch.equal(out2, s_out2))):
                bad.append(f"{c.conv.name} (M {c.M}, plan {plan}): {int((out != s_out).sum())} values differ from the single-scene calls")
    finally:
        ops.set_conv_math(prev)
    assert not bad, f"{len(bad)} findings:\n" + "\n".join(bad)


# ------------------------------------------------------------------------------------------------
# tile edges
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bm", [64, 256])
def test_row_counts_one_off_a_tile_multiple_f16(dev, bm):
    """M = k * bm - 1 and k * bm + 1 for both tile heights, tile counts of every remainder 1..7 mod 8 (the XCD remap's cases)."""
    bad, rems = [], set()
    cases = [(9, 1), (11, 1), (13, 1), (21, 3), (515, 1)] if bm == 64 else [(257, 1), (259, 1), (261, 1), (263, 1), (265, 3)]
    for k, tn in cases:
        for M in (k * bm - 1, k * bm + 1):
            c = _rows_call(dev, M, 64, (64 if bm == 64 else 128) * tn, k=1, relu=True)
            bad += _check(c, dev, f"bm={bm}", 8000 + M % 997, want_f16=True)
            plan = _plan_in(c.conv, "f16")
            assert plan["glds"] == 3 and plan["bm"] == bm and plan["tiles_m"] == -(-M // bm), (M, plan)
            rems.add(plan["tiles_m"] * plan["tiles_n"] % 8)
    assert rems >= set(range(1, 8)), f"tile counts mod 8 seen: {sorted(rems)}"
    assert not bad, "\n".join(bad)


def test_short_last_slab_f16(dev):
    """K chunks that the slabs do not divide: the last slab is short, by one chunk and by more (BK 64 slabs with a short last one:
    the forced split of the 1024-wide layers in test_f16_kernels_round_exactly_with_every_epilogue)."""
    bad, over_by = [], set()
    for Cin in (64 * 11, 64 * 17, 64 * 19, 32 * 23):
        c = _rows_call(dev, 640, Cin, 64, k=1, relu=True)
        bad += _check(c, dev, f"Cin={Cin}", 9000 + Cin, want_f16=True)
        plan = _plan_in(c.conv, "f16")
        assert plan["glds"] == 3 and plan["bk"] == 32 and plan["nchunks"] == Cin // 32, plan
        assert plan["splitk"] > 1 and (plan["splitk"] - 1) * plan["cps"] < plan["nchunks"] < plan["splitk"] * plan["cps"], plan
        over_by.add(plan["splitk"] * plan["cps"] - plan["nchunks"])
    assert 1 in over_by and max(over_by) > 1, over_by
    assert not bad, "\n".join(bad)
