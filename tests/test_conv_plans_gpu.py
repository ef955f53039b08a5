"""Every convolution plan the full-size frames really run, against an fp64 reference, in both arithmetic modes.

The case list is recorded from the model: one frame at each production size with `ops.Conv.__call__` wrapped, every distinct
`eod_conv2d` call kept with the plan the planner gave it (`ops.Conv.plan`, eod_conv2d_plan).  Each call is then replayed alone on
seeded inputs with the planner's own choice (`force_tile = force_splitk = 0`), in fp32 and in bf16x3 arithmetic, and compared with
the same operation in float64 on the CPU; torch's CPU fp32 result of that operation is the yardstick for the error.  One line per
call and mode is printed (`pytest -s`): layer, M, K, Cout -> plan, errors against fp64 next to the CPU fp32 errors.
"""
import math
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Tuple

import pytest
import torch
import torch.nn.functional as F

from _conv_cases import SENTINEL, ceiling as _ceiling, exact_hw as _hw, plan_in as _plan_in

pytestmark = pytest.mark.gpu

MODES = ("fp32", "bf16x3")
# size name -> (H, W, memory grid, cell, scenes in lock-step)
SIZES = {
    "640x640": (640, 640, 200, 0.2, 1),
    "960x960": (960, 960, 512, 0.08, 1),
    "960x960_batch4": (960, 960, 512, 0.08, 4),
    "480x640": (480, 640, 60, 0.5, 1),
}
# layer groups every recorded frame must contain (a refactor that renames layers must not silently empty the case list)
GROUPS = {
    "stem": lambda n: n == "stem",
    "trunk 1x1": lambda n: ".layer" in n and (n.endswith(".conv1") or n.endswith(".conv3")),
    "trunk 3x3": lambda n: ".layer" in n and n.endswith(".conv2"),
    "trunk downsample": lambda n: n.endswith(".downsample"),
    "FPN lateral": lambda n: n.startswith("fpn_lateral"),
    "FPN output": lambda n: n.startswith("fpn_output"),
    "P6": lambda n: n == "p6",
    "P7": lambda n: n == "p7",
    "tower": lambda n: n.startswith("bbox_tower."),
    "agn_hm+bbox_pred": lambda n: n == "agn_hm+bbox_pred",
    "box head fc1": lambda n: n.endswith(".fc1"),
    "box head fc2": lambda n: n.endswith(".fc2"),
    "cls_score+bbox_pred.0": lambda n: n.endswith("cls_score.linear+bbox_pred.0"),
    "mask convs": lambda n: n.startswith("mask_fcn"),
    "mask tail": lambda n: n == "mask_deconv",
}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    from embodied_object_detection_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


# ------------------------------------------------------------------------------------------------
# one eod_conv2d call: what was asked of which layer
# ------------------------------------------------------------------------------------------------
@dataclass
class Call:
    conv: object                      # the layer (ops.Conv): its weights and bias are the call's
    N: int
    H: int
    W: int
    res_mode: int = 0
    relu: bool = False
    in_relu: bool = False
    out_scale: float = 1.0
    gate: bool = False
    split_n: int = 0
    fuse: bool = False                # deconv + ReLU + predictor + sigmoid (out_mode 2)
    out_units: int = 0                # fuse: rows of the probability buffer; > 0 with a unit scatter list, else 0
    levels: Optional[Tuple[Tuple[int, ...], Tuple[Tuple[int, int], ...]]] = None
    gn_stats: bool = False
    gn_groups: int = 32
    plan_rows: int = 0
    m_segments: int = 0
    m_count: bool = False
    m_unit: int = 0
    force_tile: int = 0
    force_splitk: int = 0
    plans: Dict[str, dict] = field(default_factory=dict, compare=False)

    def key(self):
        c = self.conv
        return (c.name, self.N, self.H, self.W, c.Cin, c.Cout, c.KH, c.KW, c.stride, c.pad, c.out_mode, self.res_mode, self.relu,
                self.in_relu, self.out_scale, self.gate, self.split_n, self.fuse, self.out_units, self.levels, self.gn_stats,
                self.gn_groups, self.plan_rows, self.m_segments, self.m_count, self.m_unit, self.force_tile, self.force_splitk)

    @property
    def out_hw(self):
        return self.conv.out_hw(self.H, self.W) if self.levels is None else (0, 0)

    @property
    def M(self):
        return self.levels[0][-1] if self.levels is not None else self.N * self.out_hw[0] * self.out_hw[1]

    def kwargs(self):
        return dict(res_mode=self.res_mode, relu=self.relu, in_relu=self.in_relu, out_scale=self.out_scale, gn_groups=self.gn_groups,
                    plan_rows=self.plan_rows, m_segments=self.m_segments, m_unit=self.m_unit, force_tile=self.force_tile,
                    force_splitk=self.force_splitk, levels=None if self.levels is None else (list(self.levels[0]), list(self.levels[1])))


def _record(run) -> List[Call]:
    """Runs `run()` with ops.Conv.__call__ wrapped (as tools/trunk_layers.py wraps it) -> the distinct calls, in first-seen order."""
    from embodied_object_detection_amd import ops
    orig = ops.Conv.__call__
    seen: Dict[tuple, Call] = {}

    def call(self, x, N, H, W, *, res=None, res_mode=0, relu=False, in_relu=False, out_scale=1.0, m_count=None, m_unit=0, out=None,
             force_tile=0, force_splitk=0, levels=None, fuse=None, presplit=True, plan_rows=0, gn_stats=None, gn_groups=32, split=None,
             m_segments=0, gate=None):
        y = orig(self, x, N, H, W, res=res, res_mode=res_mode, relu=relu, in_relu=in_relu, out_scale=out_scale, m_count=m_count,
                 m_unit=m_unit, out=out, force_tile=force_tile, force_splitk=force_splitk, levels=levels, fuse=fuse, presplit=presplit,
                 plan_rows=plan_rows, gn_stats=gn_stats, gn_groups=gn_groups, split=split, m_segments=m_segments, gate=gate)
        c = Call(self, N, H, W, res_mode=res_mode if res is not None else 0, relu=bool(relu), in_relu=bool(in_relu), out_scale=float(out_scale),
                 gate=gate is not None, split_n=0 if split is None else int(split[0]), fuse=fuse is not None,
                 out_units=int(out.shape[0]) if (fuse is not None and fuse[2] is not None) else 0,
                 levels=None if levels is None else (tuple(int(o) for o in levels[0]), tuple((int(h), int(w)) for h, w in levels[1])),
                 gn_stats=gn_stats is not None, gn_groups=gn_groups, plan_rows=int(plan_rows), m_segments=int(m_segments),
                 m_count=m_count is not None, m_unit=int(m_unit), force_tile=force_tile, force_splitk=force_splitk)
        if c.key() not in seen:
            c.plans = {mode: _plan_in(self, mode) for mode in MODES}
            seen[c.key()] = c
        return y

    ops.Conv.__call__ = call
    try:
        run()
        torch.cuda.synchronize()
    finally:
        ops.Conv.__call__ = orig
    return list(seen.values())


@pytest.fixture(scope="module")
def recorded(dev, synthetic_sd):
    """size name -> the distinct eod_conv2d calls of one frame at that size (the only part that runs the whole model)."""
    from embodied_object_detection_amd import build_model, ops, setup_cfg
    from embodied_object_detection_amd.data.synthetic import SyntheticSequence
    from embodied_object_detection_amd.modeling.lockstep import LockstepScenes
    assert ops.get_conv_math() == "fp32"
    cfg = lambda: setup_cfg(None, ["MODEL.MEMORY_TYPE", "implicit_memory", "MODEL.MAP_FEAT_FUSION", "sum", "MODEL.MAP_FEATURE_WEIGHT", 5])
    out = {}
    for name, (H, W, grid, cell, B) in SIZES.items():
        seqs = [SyntheticSequence(7 + b, H=H, W=W, n_frames=1, map_w=grid, map_h=grid, cell=cell) for b in range(B)]
        if B == 1:
            model = build_model(cfg(), synthetic_sd)
            out[name] = _record(lambda: model([[seqs[0].frame(0)]]))
        else:
            model = LockstepScenes(cfg(), B, synthetic_sd)
            out[name] = _record(lambda: model([[s.frame(0)] for s in seqs]))
        del model
        torch.cuda.empty_cache()
    return out


# ------------------------------------------------------------------------------------------------
# seeded inputs, the operation on the CPU (float64 = reference, float32 = yardstick), the launch
# ------------------------------------------------------------------------------------------------
def _unit_counts(c: Call, which: int) -> Optional[List[int]]:
    """Production-like device-side counts that leave a partly filled last tile: 93 / 256 of 320 ROI slots (scaled to the call's
    capacity); per list of a lock-step batch 93, 256, none and 45 of 320."""
    if not c.m_count:
        return None
    segs = max(1, c.m_segments)
    cap = c.N * c.out_hw[0] * c.out_hw[1] // c.m_unit // segs
    if segs == 1:
        return [max(1, (93, 256)[which] * cap // 320)]
    return [((93, 256, 0, 45, 320, 1, 200, 17)[(s + which) % 8]) * cap // 320 for s in range(segs)]


def _active_units(c: Call, counts) -> torch.Tensor:
    """Indices of the units (images) that hold work under the counts."""
    if counts is None:
        return torch.arange(c.N)
    segs = max(1, c.m_segments)
    per = c.N // segs
    return torch.cat([torch.arange(s * per, s * per + min(counts[s], per)) for s in range(segs)])


def _inputs(c: Call, seed: int, counts) -> dict:
    g = torch.Generator().manual_seed(seed)
    conv = c.conv
    OH, OW = c.out_hw
    if c.levels is not None:
        x = torch.randn((c.M, conv.Cin), generator=g)
    else:
        x = torch.randn((c.N, c.H, c.W, conv.Cin), generator=g)
    inp = {"x": x}
    if c.m_count:
        # a unit is one image (196 rows of a 14x14 ROI, or one row of a linear layer): rows are whole images on both sides
        assert c.levels is None and c.m_unit == OH * OW, (conv.name, c.m_unit, OH, OW)
        idle = torch.ones(c.N, dtype=torch.bool)
        idle[_active_units(c, counts)] = False
        x[idle] = float("nan")             # units without work are not read into anybody's result
        inp["counts"] = torch.tensor(counts, dtype=torch.int32)
    cout = conv.Cout // 4 if conv.out_mode == 1 else conv.Cout
    if c.res_mode == 1:
        inp["res"] = torch.randn((c.M, cout) if c.levels is not None else (c.N, OH, OW, cout), generator=g)
    elif c.res_mode == 2:
        inp["res"] = torch.randn((c.N, OH // 2, OW // 2, cout), generator=g)
    if c.gate:
        inp["gate"] = torch.randn((c.N, OH, OW, cout), generator=g)
    if c.fuse:
        inp["pred_w"] = torch.randn((cout,), generator=g) * (1.0 / cout) ** 0.5
        inp["pred_b"] = 0.25
        if c.out_units:
            inp["units"] = torch.randperm(c.out_units, generator=g)[:c.N].sort().values.to(torch.int32)
    return inp


def _weights(conv, dtype):
    """The layer's weights back in torch's layout (OIHW; [Cin, Cout, 2, 2] of the ConvTranspose2d) and its bias."""
    w = conv.w.cpu()[:, :conv.KH * conv.KW * conv.Cin]
    if conv.out_mode == 1:
        cd = conv.Cout // 4
        w = w.view(2, 2, cd, conv.Cin).permute(3, 2, 0, 1)
    else:
        w = w.view(conv.Cout, conv.KH, conv.KW, conv.Cin).permute(0, 3, 1, 2)
    b = None if conv.bias is None else conv.bias.cpu().to(dtype)
    return w.contiguous().to(dtype), b


def _cpu_op(c: Call, inp: dict, units: torch.Tensor, dtype) -> torch.Tensor:
    """The call's operation in `dtype` on the CPU, for the units that hold work -> every output value, flattened (y, then y2)."""
    conv = c.conv
    w, b = _weights(conv, dtype)
    x = inp["x"].to(dtype)
    if c.in_relu:
        x = x.relu()
    if c.levels is not None:
        off, shapes = c.levels
        v = torch.cat([F.conv2d(x[off[l]:off[l + 1]].view(1, h, w_, conv.Cin).permute(0, 3, 1, 2), w, b, padding=conv.pad)
                       .permute(0, 2, 3, 1).reshape(h * w_, conv.Cout) for l, (h, w_) in enumerate(shapes)])
    else:
        xi = x[units].permute(0, 3, 1, 2)
        if conv.out_mode == 1:
            v = F.conv_transpose2d(xi, w, b, stride=2)
        else:
            v = F.conv2d(xi, w, b, stride=conv.stride, padding=conv.pad)
        v = v.permute(0, 2, 3, 1)
    v = v * c.out_scale
    if c.res_mode == 1:
        v = v + (inp["res"] if c.levels is not None else inp["res"][units]).to(dtype)
    elif c.res_mode == 2:
        v = v + inp["res"][units].to(dtype).repeat_interleave(2, dim=1).repeat_interleave(2, dim=2)
    if c.split_n:
        v = v.reshape(-1, conv.Cout)
        y2 = v[:, c.split_n:]
        return torch.cat([v[:, :c.split_n].reshape(-1), (y2.relu() if c.relu else y2).reshape(-1)])
    if c.relu:
        v = v.relu()
    if c.gate:
        v = torch.where(inp["gate"][units].to(dtype) > 0, v, torch.zeros((), dtype=dtype))
    if c.fuse:
        v = torch.sigmoid((v * inp["pred_w"].to(dtype)).sum(dim=-1) + inp["pred_b"])
    return v.reshape(-1)


class _Device:
    """The call's inputs on the device and its launches."""

    def __init__(self, c: Call, inp: dict, dev, share: Optional["_Device"] = None):
        self.c, self.dev = c, dev
        self.t = share.t if share is not None else {k: v.to(dev) for k, v in inp.items() if isinstance(v, torch.Tensor)}
        self.pred_b = inp.get("pred_b", 0.0)

    def out_buffers(self, n_units=None):
        c, conv = self.c, self.c.conv
        OH, OW = c.out_hw
        n = c.N if n_units is None else n_units
        f = dict(dtype=torch.float32, device=self.dev)
        if c.fuse:
            return torch.full((c.out_units or n, 2 * OH, 2 * OW), SENTINEL, **f), None
        if c.levels is not None:
            return torch.full((c.M, conv.Cout), SENTINEL, **f), None
        if conv.out_mode == 1:
            return torch.full((n, 2 * OH, 2 * OW, conv.Cout // 4), SENTINEL, **f), None
        if c.split_n:
            return torch.full((n * OH * OW, c.split_n), SENTINEL, **f), torch.full((n * OH * OW, conv.Cout - c.split_n), SENTINEL, **f)
        return torch.full((n, OH, OW, conv.Cout), SENTINEL, **f), None

    def launch(self, out=None, out2=None, units=None, counts=None):
        """One eod_conv2d launch; `units` = a slice of the images (a single-image call of a batch), `counts` its own counts."""
        from embodied_object_detection_amd import ops
        c, conv, t = self.c, self.c.conv, self.t
        sl = slice(None) if units is None else units
        n = c.N if units is None else (units.stop - units.start)
        if out is None:
            out, out2 = self.out_buffers(n)
        kw = c.kwargs()
        x = t["x"] if c.levels is not None else t["x"][sl]
        if "res" in t:
            kw["res"] = t["res"] if c.levels is not None else t["res"][sl]
        if "gate" in t:
            kw["gate"] = t["gate"][sl]
        if c.m_count:
            kw["m_count"] = t["counts"] if counts is None else torch.tensor(counts, dtype=torch.int32, device=self.dev)
        if c.fuse:
            kw["fuse"] = (t["pred_w"], self.pred_b, t["units"][sl] if "units" in t else None)
        if c.split_n:
            kw["split"] = (c.split_n, out2)
        gn_ws = None
        if c.gn_stats:
            gn_ws = ops.groupnorm_workspace(kw["levels"][0], self.dev, c.gn_groups)
            kw["gn_stats"] = gn_ws
        y = conv(x, n, c.H, c.W, out=out, **kw)
        assert y.data_ptr() == out.data_ptr()
        return out, out2, gn_ws

    def values(self, out, out2, units: torch.Tensor) -> torch.Tensor:
        """What the launch wrote for the units that hold work, in the order `_cpu_op` returns it."""
        c = self.c
        u = units.to(self.dev)
        if c.fuse:
            rows = self.t["units"].long()[u] if "units" in self.t else u
            return out[rows].reshape(-1).double().cpu()
        if c.levels is not None:
            return out.reshape(-1).double().cpu()
        if c.split_n:
            OH, OW = c.out_hw
            assert OH * OW == 1
            return torch.cat([out[u].reshape(-1), out2[u].reshape(-1)]).double().cpu()
        return out[u].reshape(-1).double().cpu()

    def untouched(self, out, out2, units: torch.Tensor) -> bool:
        """Rows of units without work still hold the sentinel."""
        c = self.c
        idle = torch.ones(out.shape[0], dtype=torch.bool)
        rows = units if not (c.fuse and "units" in self.t) else self.t["units"].long().cpu()[units]
        idle[rows] = False
        idle = idle.to(self.dev)
        ok = bool((out[idle] == SENTINEL).all())
        if out2 is not None:
            ok = ok and bool((out2[idle] == SENTINEL).all())
        return ok


def _gn_partials_ok(c: Call, out: torch.Tensor, gn_ws: torch.Tensor) -> float:
    """The GroupNorm partial sums the slab reduce wrote, against the sums of the very values it stored (32-row chunks per level,
    [chunk][group][sum, sum of squares] in double) -> largest relative difference."""
    from embodied_object_detection_amd import _lib
    off, shapes = c.levels
    G = c.gn_groups
    start = _lib.load().eod_groupnorm_partial_offset(len(shapes), G) // 8
    y = out.double().cpu().view(c.M, G, -1)
    want = []
    for l in range(len(shapes)):
        for r0 in range(off[l], off[l + 1], 32):
            blk = y[r0:min(r0 + 32, off[l + 1])]
            want.append(torch.stack([blk.sum(dim=(0, 2)), (blk * blk).sum(dim=(0, 2))], dim=1))
    want = torch.stack(want)
    got = gn_ws.cpu()[start:start + want.numel()].view_as(want)
    return float(((got - want).abs() / (want.abs() + 1e-30)).max())


def _family(c: Call, plan: dict) -> str:
    """The kernel family a plan belongs to: which kernel, and which branch of the planner split K."""
    if plan["wavek"]:
        return f"fp32 wave-K {plan['wavek']} waves"
    if plan["tile"] == 5:
        return "fp32 64x256 fused tail"
    kern = ("bf16x3" if plan["glds"] == 2 else "fp32") + f" {plan['bm']}x{plan['bn']} BK{plan['bk']}"
    if plan["splitk"] == 1:
        return kern
    rows = c.plan_rows if 0 < c.plan_rows < c.M else c.M
    tiles = -(-rows // plan["bm"]) * plan["tiles_n"]
    how = "slabs, few tiles" if tiles < 256 else "slabs, mid split"
    return f"{kern} split-K ({how}{', GroupNorm statistics' if plan['gn_fused'] else ''})"


def _line(tag, c: Call, plan: dict, e, e32) -> str:
    return (f"{tag:15s} {c.conv.name[-44:]:44s} M {c.M:7d} K {c.conv.Kpad:5d} Cout {c.conv.Cout:4d} -> {_family(c, plan):58s} "
            f"tiles {plan['tiles_m']}x{plan['tiles_n']} splitk {plan['splitk']}x{plan['cps']}  err/scale mean {e[0]:.2e} max {e[1]:.2e}"
            f"  cpu fp32 mean {e32[0]:.2e} max {e32[1]:.2e}")


def _check(c: Call, dev, tag: str, seed: int, expect_plans: Optional[dict] = None, modes=MODES) -> List[str]:
    """Replays the call alone in every mode against fp64 -> the list of what is wrong with it (empty = fine); prints one line per
    mode and count."""
    from embodied_object_detection_amd import ops
    bad = []
    for which in ((0, 1) if c.m_count else (0,)):
        counts = _unit_counts(c, which)
        inp = _inputs(c, seed, counts)
        units = _active_units(c, counts)
        ref = _cpu_op(c, inp, units, torch.float64)
        e32v = (_cpu_op(c, inp, units, torch.float32).double() - ref).abs()
        scale = float(ref.abs().mean())
        e32 = (float(e32v.mean()) / scale, float(e32v.max()) / scale)
        d = _Device(c, inp, dev)
        for mode in modes:
            prev = ops.set_conv_math(mode)
            try:
                out, out2, gn_ws = d.launch()
                plan = c.conv.plan()
            finally:
                ops.set_conv_math(prev)
            torch.cuda.synchronize()
            who = f"{c.conv.name} [{mode}{'' if counts is None else f', counts {counts}'}]"
            # (gn_fused of the recorded plan is the fp32 frame's in both modes: the descriptor it was read from)
            if expect_plans is not None and dict(plan, gn_fused=0) != dict(expect_plans[mode], gn_fused=0):
                bad.append(f"{who}: replayed with plan {plan}, the frame ran {expect_plans[mode]}")
            ev = (d.values(out, out2, units) - ref).abs()
            e = (float(ev.mean()) / scale, float(ev.max()) / scale)
            print(_line(tag, c, plan, e, e32) + ("" if counts is None else f"  counts {counts}"), flush=True)
            if not math.isfinite(e[1]):
                bad.append(f"{who}: non-finite output")
            if e[0] > 2.5 * e32[0]:
                bad.append(f"{who}: mean error {e[0]:.3e} of scale > 2.5 x the CPU fp32 convolution's {e32[0]:.3e}")
            if e[1] > 4.0 * e32[1]:
                bad.append(f"{who}: max error {e[1]:.3e} of scale > 4 x the CPU fp32 convolution's {e32[1]:.3e}")
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
# 1. the production frames
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", list(SIZES))
def test_recording_holds_every_layer_group(recorded, size):
    calls = recorded[size]
    names = [c.conv.name for c in calls]
    for group, pred in GROUPS.items():
        assert any(pred(n) for n in names), f"{size}: no recorded eod_conv2d call of group '{group}'"
    assert sum(1 for n in set(names) if n == "stem" or ".layer" in n) == 53, "ResNet-50 has 53 convolutions"
    # the frame leaves every choice to the planner, and nothing of the training path (gate) runs in it
    assert all(c.force_tile == 0 and c.force_splitk == 0 and not c.gate for c in calls)
    B = SIZES[size][4]
    if B > 1:
        assert all(c.N % B == 0 or c.levels is not None for c in calls)
        assert any(c.m_segments == B for c in calls) and any(c.levels is not None and len(c.levels[1]) == 5 * B for c in calls)
        assert all(c.plan_rows > 0 for c in calls), "a lock-step batch is planned like one image"
    assert any(c.m_count and c.m_unit == 196 for c in calls) and any(c.fuse for c in calls)


@pytest.mark.parametrize("size", list(SIZES))
def test_production_calls_match_fp64_in_both_modes(dev, recorded, size):
    bad = []
    for i, c in enumerate(recorded[size]):
        bad += _check(c, dev, size, 1000 + i, expect_plans=c.plans)
    assert not bad, f"{len(bad)} findings:\n" + "\n".join(bad)


# Families `make_plan` has code for that no force_tile = 0 call can get, whatever its shape: listed with the reason, asserted absent
# (a planner change that makes one reachable has to move it to the required set), and run through force_tile in the supplement.
UNREACHABLE = {
    # make_plan gives the fp32 kernel BK = 32 (measured) unless the call forces 64
    "fp32 64x64 BK64": "BK = 64 is chosen by force_tile 2x only",
    # t128 >= 512 implies t256 >= 256 (ceil(M / 256) >= ceil(M / 128) / 2): the 256x128 kernel always wins the comparison
    "bf16x3 128x128 BK32": "the planner's t128 >= 512 branch is shadowed by t256 >= 256",
}
REQUIRED = {
    "fp32": ["fp32 64x64 BK32", "fp32 wave-K 4 waves", "fp32 wave-K 8 waves", "fp32 64x64 BK32 split-K (slabs, few tiles)",
             "fp32 64x64 BK32 split-K (slabs, mid split, GroupNorm statistics)", "fp32 64x256 fused tail"],
    "bf16x3": ["bf16x3 64x64 BK32", "bf16x3 256x128 BK32", "bf16x3 64x64 BK32 split-K (slabs, few tiles)",
               "bf16x3 64x64 BK32 split-K (slabs, mid split, GroupNorm statistics)", "fp32 64x64 BK32", "fp32 64x256 fused tail"],
}


@pytest.mark.parametrize("mode", MODES)
def test_production_plans_cover_every_kernel_family(recorded, mode):
    """The union of the plans of the recorded frames holds every family the planner can emit in this mode; per size the families
    are printed with the layers that got them."""
    union = set()
    for size, calls in recorded.items():
        fams: Dict[str, List[str]] = {}
        for c in calls:
            fams.setdefault(_family(c, c.plans[mode]), []).append(c.conv.name)
        for f, names in sorted(fams.items()):
            print(f"{size:15s} {mode:7s} {f:70s} {len(names):3d} calls, e.g. {names[0]}")
        union |= set(fams)
    for f in REQUIRED[mode]:
        assert f in union, f"no production call at any size gets the family '{f}' in {mode} mode"
    for f, why in UNREACHABLE.items():
        assert f not in union, f"'{f}' is now reached ({why} no longer holds): require it"
    # the large bf16x3 tile is the planner's own choice for the layers with the most rows at every full size
    if mode == "bf16x3":
        for size, calls in recorded.items():
            assert any(c.plans[mode]["tile"] == 4 for c in calls), size


# ------------------------------------------------------------------------------------------------
# 2. a lock-step batch walks K like a single image
# ------------------------------------------------------------------------------------------------
def _single_calls(c: Call, B: int, counts):
    """The batched call as B calls of one scene each: (rows or units of the scene, that scene's Call, its counts)."""
    if c.levels is not None:
        off, shapes = c.levels
        L = len(shapes) // B
        for b in range(B):
            lv = [l * B + b for l in range(L)]
            soff = [0]
            for l in lv:
                soff.append(soff[-1] + off[l + 1] - off[l])
            rows = torch.cat([torch.arange(off[l], off[l + 1]) for l in lv])
            yield rows, Call(c.conv, 1, 0, 0, relu=c.relu, out_scale=c.out_scale, levels=(tuple(soff), tuple(shapes[l] for l in lv)),
                             gn_stats=c.gn_stats, gn_groups=c.gn_groups), None
        return
    per = c.N // B
    total = None if counts is None else counts[0]
    for b in range(B):
        if counts is None:
            cb = None
        elif c.m_segments == B:
            cb = [counts[b]]
        else:                       # one compact list over all scenes (the mask passes): the scenes' shares follow one another
            cb = [max(0, min(per, total - b * per))]
        yield slice(b * per, (b + 1) * per), Call(c.conv, per, c.H, c.W, res_mode=c.res_mode, relu=c.relu, in_relu=c.in_relu,
                                                  out_scale=c.out_scale, split_n=c.split_n, fuse=c.fuse, out_units=c.out_units,
                                                  m_count=c.m_count, m_unit=c.m_unit), cb


def test_batch_of_4_is_bitwise_4_single_image_calls(dev, recorded):
    """Every call of the 960x960 batch of 4 (N = 4, 20 pyramid levels, 4 unit lists, one compact list), planned like one image as
    recorded, writes bitwise what the four single-scene calls write on the same inputs, in both arithmetic modes."""
    from embodied_object_detection_amd import ops
    B = SIZES["960x960_batch4"][4]
    bad = []
    for i, c in enumerate(recorded["960x960_batch4"]):
        counts = _unit_counts(c, 0)
        inp = _inputs(c, 5000 + i, counts)
        d = _Device(c, inp, dev)
        for mode in MODES:
            prev = ops.set_conv_math(mode)
            try:
                out, out2, _ = d.launch()
                s_out, s_out2 = d.out_buffers()
                for where, sc, cb in _single_calls(c, B, counts):
                    if c.levels is not None:
                        o, _o2, _ws = _Device(sc, {"x": inp["x"][where]}, dev).launch()
                        s_out[where.to(dev)] = o
                    elif c.fuse:         # the scatter rows of the scenes are disjoint: every single call writes the shared buffer
                        _Device(sc, inp, dev, share=d).launch(out=s_out, units=where, counts=cb)
                    else:
                        rows = slice(where.start * (s_out.shape[0] // c.N), where.stop * (s_out.shape[0] // c.N))
                        _Device(sc, inp, dev, share=d).launch(out=s_out[rows], out2=None if s_out2 is None else s_out2[rows], units=where,
                                                              counts=cb)
            finally:
                ops.set_conv_math(prev)
            torch.cuda.synchronize()
            same = torch.equal(out, s_out) and (out2 is None or torch.equal(out2, s_out2))
            if not same:
                n = int((out != s_out).sum())
                bad.append(f"{c.conv.name} [{mode}] (M {c.M}, plan {c.plans[mode]}): {n} values differ from the single-scene calls")
    assert not bad, f"{len(bad)} findings:\n" + "\n".join(bad)


# ------------------------------------------------------------------------------------------------
# 3. edges the production list does not hold but the planner's branch conditions invite
# ------------------------------------------------------------------------------------------------
def _layer(dev, Cin, Cout, k=1, stride=1, seed=0, name="", deconv=False):
    from embodied_object_detection_amd import ops
    g = torch.Generator().manual_seed(seed)
    if deconv:
        w = torch.randn((Cin, Cout, 2, 2), generator=g) * (1.0 / Cin) ** 0.5
        return ops.Conv(w, torch.randn((Cout,), generator=g), device=dev, deconv=True, name=name)
    w = torch.randn((Cout, Cin, k, k), generator=g) * (1.0 / (Cin * k * k)) ** 0.5
    return ops.Conv(w, torch.randn((Cout,), generator=g), stride=stride, pad=k // 2, device=dev, name=name)


def _rows_call(dev, M, Cin, Cout, k=1, name="", **kw) -> Call:
    h, w = _hw(M)
    return Call(_layer(dev, Cin, Cout, k, seed=M % 1000, name=name or f"edge M={M} {Cin}->{Cout} k{k}"), 1, h, w, **kw)


def test_tile_count_thresholds_of_the_planner(dev):
    """Tile counts on both sides of every threshold of make_plan: 255 / 256 / 257 and 1024 / 1025 tiles of 64x64 (fp32: few-tile
    slabs | mid split | none), 255 / 256 tiles of 256x128 (bf16x3: 64x64 | 256x128)."""
    bad = []
    want = {255: "fp32 64x64 BK32 split-K (slabs, few tiles)", 256: "fp32 64x64 BK32", 257: "fp32 64x64 BK32 split-K (slabs, mid split)",
            1024: "fp32 64x64 BK32", 1025: "fp32 64x64 BK32"}
    for tiles, fam in want.items():
        c = _rows_call(dev, tiles * 64, 64, 64, k=3, relu=True)           # K = 576: 18 chunks, the fewest the mid split takes
        bad += _check(c, dev, f"tiles={tiles}", 7000 + tiles, modes=("fp32",))
        plan = _plan_in(c.conv, "fp32")
        assert plan["tiles_m"] * plan["tiles_n"] == tiles and _family(c, plan) == fam, (tiles, plan)
    for t256, tile in ((255, 3), (256, 4)):
        c = _rows_call(dev, t256 * 256, 32, 128, k=3, relu=True)
        bad += _check(c, dev, f"t256={t256}", 7100 + t256, modes=("bf16x3",))
        plan = _plan_in(c.conv, "bf16x3")
        assert plan["glds"] == 2 and plan["tile"] == tile and -(-c.M // 256) == t256, (t256, plan)
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("bm", [32, 64, 128, 256])
def test_row_counts_one_off_a_tile_multiple(dev, bm):
    """M = k * bm + 1 and k * bm - 1 for every tile height in use, with tile counts of every remainder 1..7 mod 8 (the XCD remap's
    remainder cases), one of them above 4 096 tiles.  bm = 128 has no automatic plan (see UNREACHABLE): force_tile 51 / 1."""
    bad, rems = [], set()
    if bm == 32:       # wave-K: few rows, deep K; 32-column tiles
        cases = [(k, 2048 if k in (3, 7, 15) else 1024, 32 * tn, "fp32", 0) for k, tn in ((1, 1), (3, 1), (5, 1), (7, 3), (11, 5), (15, 3))]
    elif bm == 64:
        cases = [(k, 32, 64 * tn, "fp32", 0) for k, tn in ((9, 1), (11, 1), (13, 1), (21, 3), (4103, 1))]
    elif bm == 128:
        cases = [(k, 64, 128 * tn, mode, ft) for k, tn in ((1, 1), (3, 1), (5, 1), (7, 1), (9, 3)) for mode, ft in (("bf16x3", 51), ("fp32", 1))]
    else:
        cases = [(k, 32, 128 * tn, "bf16x3", 0) for k, tn in ((257, 1), (259, 1), (261, 1), (263, 1), (265, 3))]
    for k, Cin, Cout, mode, ft in cases:
        for M in (k * bm - 1, k * bm + 1):
            c = _rows_call(dev, M, Cin, Cout, k=1, relu=True, force_tile=ft)
            bad += _check(c, dev, f"bm={bm}", 8000 + M % 997, modes=(mode,))
            plan = _plan_in(c.conv, mode)
            assert plan["bm"] == bm and plan["tiles_m"] == -(-M // bm), (M, plan)
            rems.add(plan["tiles_m"] * plan["tiles_n"] % 8)
            if bm == 64 and k > 4096:
                assert plan["tiles_m"] * plan["tiles_n"] > 4096
    assert rems >= set(range(1, 8)), f"tile counts mod 8 seen: {sorted(rems)}"
    assert not bad, "\n".join(bad)


def test_short_last_slab(dev):
    """K chunks that the slabs do not divide: the last slab is short, by up to all but one of its chunks' worth."""
    bad, over_by = [], set()
    for nchunks in (11, 17, 19, 23):
        c = _rows_call(dev, 640, 32 * nchunks, 64, k=1, relu=True)
        for mode in MODES:
            bad += _check(c, dev, f"chunks={nchunks}", 9000 + nchunks, modes=(mode,))
            plan = _plan_in(c.conv, mode)
            assert plan["nchunks"] == nchunks and plan["splitk"] > 1 and nchunks % plan["splitk"] != 0, plan
            assert (plan["splitk"] - 1) * plan["cps"] < nchunks < plan["splitk"] * plan["cps"], plan
            over_by.add(plan["splitk"] * plan["cps"] - nchunks)
    assert 1 in over_by and max(over_by) > 1, over_by
    assert not bad, "\n".join(bad)


BF16X3_EPILOGUES = [
    # name, Call fields, layer (Cin, Cout, k, stride)
    ("res_mode 1 + relu", dict(res_mode=1, relu=True), (128, 192, 3, 1)),
    ("res_mode 2 (x2 residual)", dict(res_mode=2), (256, 256, 1, 1)),
    ("out_scale", dict(out_scale=0.37, relu=True), (64, 96, 3, 1)),
    ("stride 2", dict(relu=True), (128, 256, 3, 2)),
    ("stride 2, 1x1", dict(), (256, 512, 1, 2)),
]


@pytest.mark.parametrize("tile", [0, 51, 52, 53, 54])
@pytest.mark.parametrize("splitk", [0, 3])
def test_bf16x3_kernels_with_every_epilogue(dev, tile, splitk):
    """The bf16x3 kernels (planner's choice and each tile forced: 128x128, 128x64, 64x64, 256x128) with the epilogues the fp32 kernel
    has, stride 2, a device-side count, two stacked linear layers, pyramid mode with GroupNorm statistics, with and without slabs."""
    bad = []
    fk = dict(force_tile=tile, force_splitk=splitk)
    calls = []
    for name, f, (Cin, Cout, k, stride) in BF16X3_EPILOGUES:
        calls.append(Call(_layer(dev, Cin, Cout, k, stride, seed=len(calls), name=name), 2, 38, 46, **f, **fk))
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
        bad += _check(c, dev, f"tile={tile} sk={splitk}", 9500 + i, modes=("bf16x3",))
        plan = _plan_in(c.conv, "bf16x3")
        assert plan["glds"] == 2 and (tile == 0 or plan["tile"] == {51: 1, 52: 2, 53: 3, 54: 4}[tile]), (c.conv.name, plan)
        assert splitk == 0 or plan["splitk"] == splitk, (c.conv.name, plan)
        if c.gn_stats:
            assert plan["gn_fused"] == int(plan["splitk"] > 1), plan
    assert not bad, "\n".join(bad)
