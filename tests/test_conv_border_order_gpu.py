"""The border-major row order of the mask head's 3x3 convs (csrc/conv_fp32.hip, PIPE 3; force_tile 43).

1. bitwise the pixel-major 64x64 kernel (force_tile 13, one K slab) on random finite inputs, forced and as the planner's own choice,
   into sentinel-filled buffers: rows past the device-side count stay unwritten under both orders;
2. the same cases against float64 with the criteria of test_conv_plans_gpu._check;
3. which order a call gets, seen from outside: an infinite weight under a padding tap is the one input on which the orders differ;
4. calls the order does not take refuse the forcing code and keep the pixel-major kernel's bits.

The shapes are the smallest at which the order or the chunk skip can go wrong: 2 chunks per tap (Cin 64), one and two column
tiles, and ROI counts that leave every region shorter than a tile (order active, nothing skipped), one whole skipping tile next to
a mixed one, two whole skipping tiles per row region, a partial last tile at M, count = capacity and count = 0; a non-square map,
a map without interior; the production shape once at the frame's two ROI counts.  Units past the count hold NaN inputs.
"""
import dataclasses
import math

import pytest
import torch

from _conv_cases import ceiling as _ceiling
from test_conv_plans_gpu import SENTINEL, Call, _active_units, _cpu_op, _Device, _inputs, _layer, dev  # noqa: F401

pytestmark = pytest.mark.gpu

BORDER = 43             # force_tile: the border-major order, or EOD_ERR_BAD_DIMS
GENERIC = 13            # force_tile: conv_igemm_kernel<64,64,32>, pixel-major

# (map h, map w, Cin, Cout, capacity, count)
SMALL = [(14, 14, 64, cout, cap, cnt) for cout in (64, 128)
         for cap, cnt in ((8, 0), (8, 1), (8, 5), (16, 10), (40, 23), (40, 40))]
SMALL += [(6, 9, 64, 64, 40, 23), (3, 3, 64, 64, 40, 30)]
PRODUCTION = [(14, 14, 256, 256, 128, 43), (14, 14, 256, 256, 300, 88)]


def _id(case):
    h, w, cin, cout, cap, cnt = case
    return f"{h}x{w}-{cin}to{cout}-{cnt}of{cap}"


def _call(dev, case, relu=True, **kw) -> Call:
    h, w, cin, cout, cap, _cnt = case
    conv = _layer(dev, cin, cout, k=3, seed=h * w + cout, name=f"border {_id(case)}")
    return Call(conv, cap, h, w, relu=relu, m_count=True, m_unit=h * w, **kw)


def _launch(c: Call, d: _Device, force_tile: int, force_splitk: int):
    cc = dataclasses.replace(c, force_tile=force_tile, force_splitk=force_splitk)
    out, _o2, _ws = _Device(cc, {}, d.dev, share=d).launch()
    plan = c.conv.plan()
    torch.cuda.synchronize()
    assert plan["tile"] == 3 and plan["bm"] == plan["bn"] == 64 and plan["bk"] == 32 and plan["splitk"] == 1 and not plan["wavek"], plan
    return out


def _compare(dev, case, auto_splitk):
    """Forced border order, the planner's choice and force_tile 13 on the same inputs -> findings."""
    c = _call(dev, case)
    counts = [case[5]]
    units = _active_units(c, counts)
    d = _Device(c, _inputs(c, 16000 + case[4] * 50 + case[5], counts), dev)
    old = _launch(c, d, GENERIC, 1)
    new = _launch(c, d, BORDER, 0)
    auto = _launch(c, d, 0, auto_splitk)
    bad = []
    name = c.conv.name
    if not torch.equal(new, old):
        bad.append(f"{name}: {int((new != old).sum())} values differ from the pixel-major kernel's")
    if not torch.equal(auto, new):
        bad.append(f"{name}: the planner's choice differs from the forced code in {int((auto != new).sum())} values")
    for who, out in (("pixel-major", old), ("border-major", new), ("planner's choice", auto)):
        if not d.untouched(out, None, units):
            bad.append(f"{name}: the {who} launch wrote rows past the count")
        if bool((out[units.to(dev)] == SENTINEL).any()) or not bool(torch.isfinite(out[units.to(dev)]).all()):
            bad.append(f"{name}: the {who} launch left rows under the count unwritten or not finite")
    return bad


@pytest.mark.parametrize("case", SMALL, ids=_id)
def test_bitwise_the_pixel_major_kernel(dev, case):
    """(force_splitk 1 on the planner's own call: below 256 tiles the generic plan has slabs, which the order does not take)"""
    bad = _compare(dev, case, auto_splitk=1)
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("case", PRODUCTION, ids=_id)
def test_production_shape_is_the_planners_choice_and_bitwise(dev, case):
    bad = _compare(dev, case, auto_splitk=0)
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("case", SMALL, ids=_id)
def test_matches_fp64(dev, case):
    c = _call(dev, case, force_tile=BORDER)
    counts = [case[5]]
    units = _active_units(c, counts)
    inp = _inputs(c, 17000 + case[4] * 50 + case[5], counts)
    d = _Device(c, inp, dev)
    out, _o2, _ws = d.launch()
    torch.cuda.synchronize()
    assert d.untouched(out, None, units), "rows beyond the device-side count were written"
    if case[5] == 0:
        return
    ref = _cpu_op(c, inp, units, torch.float64)
    e32v = (_cpu_op(c, inp, units, torch.float32).double() - ref).abs()
    scale = float(ref.abs().mean())
    e32 = (float(e32v.mean()) / scale, float(e32v.max()) / scale)
    ev = (d.values(out, None, units) - ref).abs()
    e = (float(ev.mean()) / scale, float(ev.max()) / scale)
    print(f"{c.conv.name}: err/scale mean {e[0]:.2e} max {e[1]:.2e}  cpu fp32 mean {e32[0]:.2e} max {e32[1]:.2e}", flush=True)
    assert math.isfinite(e[1])
    assert e[0] <= 2.5 * e32[0], f"mean error {e[0]:.3e} of scale > 2.5 x the CPU fp32 convolution's {e32[0]:.3e}"
    assert e[1] <= 4.0 * e32[1], f"max error {e[1]:.3e} of scale > 4 x the CPU fp32 convolution's {e32[1]:.3e}"
    assert e[0] <= _ceiling(c.conv.Kpad), f"mean error {e[0]:.3e} of scale above the ceiling {_ceiling(c.conv.Kpad):.0e}"


def _skips_padding_taps(dev, case, force_tile, force_splitk) -> bool:
    """Which order a launch runs, seen from outside: with an infinite weight under tap (0, 0) the pixel-major kernel multiplies it
    with the padding's zeros (NaN) for a top-row pixel, the border-major order leaves the chunk out where the whole tile is top rows
    (the first tile, once count * OW >= 64) -- the one condition under which the orders differ (conv_fp32.hip)."""
    c = _call(dev, case, relu=False)           # (the ReLU's fmaxf would turn the NaN into 0)
    c.conv.w[:, :c.conv.Cin] = float("inf")
    counts = [case[5]]
    d = _Device(c, _inputs(c, 19000, counts), dev)
    cc = dataclasses.replace(c, force_tile=force_tile, force_splitk=force_splitk)
    out, _o2, _ws = _Device(cc, {}, dev, share=d).launch()
    torch.cuda.synchronize()
    top = out[0, 0, 1:case[1] - 1]             # map 0, top row without its corners: logical rows 1 .. OW - 2 of the first tile
    assert bool(torch.isfinite(top).all()) or bool(torch.isnan(top).all()), top
    return bool(torch.isfinite(top).all())


@pytest.mark.parametrize("case,splitk", [((14, 14, 64, 64, 8, 5), 1), (PRODUCTION[0], 0)], ids=["small", "production"])
def test_which_order_a_call_gets(dev, case, splitk):
    """force_tile 13 keeps the pixel-major order, 43 and the planner's own choice run the border-major one."""
    assert not _skips_padding_taps(dev, case, GENERIC, 1)
    assert _skips_padding_taps(dev, case, BORDER, 0)
    assert _skips_padding_taps(dev, case, 0, splitk)


def _ineligible(dev):
    """name -> (call, counts): one call per class the order does not take."""
    k3 = lambda name, stride=1: _layer(dev, 64, 64, k=3, stride=stride, seed=7, name=name)      # noqa: E731
    return {
        "stride 2": (Call(k3("stride 2", 2), 16, 14, 14, relu=True, m_count=True, m_unit=49), [10]),
        "pyramid mode": (Call(k3("pyramid mode"), 1, 0, 0, relu=True, levels=((0, 196, 196 + 63), ((14, 14), (7, 9)))), None),
        "m_segments 2": (Call(k3("m_segments 2"), 16, 14, 14, relu=True, m_count=True, m_unit=196, m_segments=2), [5, 8]),
        "res_mode 1": (Call(k3("res_mode 1"), 16, 14, 14, relu=True, res_mode=1, m_count=True, m_unit=196), [10]),
        "gate": (Call(k3("gate"), 16, 14, 14, gate=True, m_count=True, m_unit=196), [10]),
    }


def test_ineligible_calls_refuse_the_code_and_keep_their_bits(dev):
    from embodied_object_detection_amd._lib import EodError
    bad = []
    for i, (name, (c, counts)) in enumerate(_ineligible(dev).items()):
        d = _Device(c, _inputs(c, 18000 + i, counts), dev)
        with pytest.raises(EodError, match="EOD_ERR_BAD_DIMS"):
            _Device(dataclasses.replace(c, force_tile=BORDER), {}, dev, share=d).launch()
        auto, _o2, _ws = _Device(dataclasses.replace(c, force_splitk=1), {}, dev, share=d).launch()
        old, _o2, _ws = _Device(dataclasses.replace(c, force_tile=GENERIC, force_splitk=1), {}, dev, share=d).launch()
        torch.cuda.synchronize()
        if not torch.equal(auto, old):
            bad.append(f"{name}: {int((auto != old).sum())} values differ from the pixel-major kernel's")
    assert not bad, "\n".join(bad)
