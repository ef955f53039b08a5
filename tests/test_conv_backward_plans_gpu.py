"""Every backward convolution launch the full-size training steps really run, against an fp64 reference.

The case list is recorded from the training steps: one step of each production configuration with `ops.ConvBackward.__call__`
wrapped, every distinct call kept (distinct in its ARGUMENTS: layers that share every argument, like the blocks of one ResNet stage,
are one case listed under all their names) with the number of position ranges its weight-gradient launch cuts the positions into,
the plan of its input-gradient convolution and the dX path it took.  Each case is then replayed alone on seeded inputs and weights
in fp32 and in bf16x3 arithmetic and compared with the same operation in float64 on the CPU (`aten.convolution_backward`); torch's
CPU fp32 result of that operation is the yardstick for the error.  One line per case, output and mode is printed (`pytest -s`).

What the code promises and what it does not (so what is compared bitwise and what against fp64 only):
  * dW / db do not read the arithmetic mode: bitwise equal in fp32 and bf16x3.
  * The range reduce adds in range order: every case repeats bitwise through the one shared workspace.
  * The backward of a shared-trunk batch passes no `plan_rows` to its input-gradient convolutions, so dX of image i of an N-image
    call is NOT promised to be bitwise its own N = 1 call (tests/test_detector_training_gpu.py compares the two steps to 1e-5):
    both are compared with fp64, and dW with the fp64 sum over the images.
  * Pyramid mode is compared with per-level convolutions by closeness in the forward tests (test_conv_pyramid_mode_matches_per_
    level_conv), not bitwise: the `levels=` dX is compared with the per-level fp64 gradients, dW / db with their fp64 sum.

The two fallback weight-gradient kernels (`EOD_WGRAD_LDS=0`: 64 x 64 register blocks; with `EOD_WGRAD_RB=0` as well: 32 x 32 tiles)
are selected by environment variables read once at load: one fresh child process per setting replays a handful of production shapes
(this file run as a program).
"""
import math
import os
import subprocess
import sys
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Tuple

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if __name__ == "__main__":
    sys.path[:0] = [ROOT, os.path.dirname(os.path.abspath(__file__))]

from _conv_cases import SENTINEL, ceiling, exact_hw, plan_in    # noqa: E402

pytestmark = pytest.mark.gpu

MODES = ("fp32", "bf16x3")
# configuration -> (H, W, which step, frames that share the trunk pass, config overrides)
FROZEN = ["MODEL.FREEZE_BACKBONE", True, "MODEL.UNFROZEN_LAYERS", ["roi", "map_merge", "proposal_generator"]]
FROZEN_TRUNK = ["MODEL.FREEZE_BACKBONE", True, "MODEL.UNFROZEN_LAYERS", ["roi", "map_merge", "proposal_generator", "fpn_"]]
CONFIGS = {
    "640x640 full": (640, 640, "full", 1, []),
    "640x640 proposals": (640, 640, "proposals", 1, []),
    "640x640 batch2": (640, 640, "full", 2, []),
    "640x640 batch4": (640, 640, "full", 4, []),
    "480x640 full": (480, 640, "full", 1, []),
    "640x640 frozen": (640, 640, "full", 1, FROZEN),                 # the yaml's UNFROZEN_LAYERS: no trunk-half backward at all
    "640x640 frozen trunk": (640, 640, "full", 1, FROZEN_TRUNK),     # the FPN trains, the ResNet does not: laterals with need_dx=False
}
# layer groups a recorded step must contain (a refactor that renames layers must not silently empty the case list)
TRUNK_GROUPS = {
    "stem": lambda n: n == "stem",
    "trunk 1x1": lambda n: ".layer" in n and (n.endswith(".conv1") or n.endswith(".conv3")),
    "trunk 3x3": lambda n: ".layer" in n and n.endswith(".conv2"),
    "trunk downsample": lambda n: n.endswith(".downsample"),
}
FPN_GROUPS = {
    "FPN lateral": lambda n: n.startswith("fpn_lateral"),
    "FPN output": lambda n: n.startswith("fpn_output"),
}
HEAD_GROUPS = {
    "P6": lambda n: n == "p6",
    "P7": lambda n: n == "p7",
    "tower": lambda n: n.startswith("bbox_tower."),
    "agn_hm+bbox_pred": lambda n: n == "agn_hm+bbox_pred",
}
BOX_GROUPS = {
    "box head fc1": lambda n: n.endswith(".fc1"),
    "box head fc2": lambda n: n.endswith(".fc2"),
    "cls_score": lambda n: n.endswith(".cls_score.linear"),
    "bbox_pred.0": lambda n: n.endswith(".bbox_pred.0"),
    "bbox_pred.2": lambda n: n.endswith(".bbox_pred.2"),
}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    from embodied_object_detection_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


# ------------------------------------------------------------------------------------------------
# one ops.ConvBackward call: what was asked of which layer shape
# ------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Case:
    N: int
    H: int
    W: int
    Cin: int                          # of the packed layout (4 for the stem)
    Cout: int
    k: int
    stride: int = 1
    pad: int = 0
    cin_pad: int = 0                  # 4: the stem's tap layout over 3 real channels
    relu: bool = False
    need_dx: bool = True
    res: bool = False                 # dx_res given
    gate: bool = False                # dx_gate given
    levels: Optional[Tuple[Tuple[int, ...], Tuple[Tuple[int, int], ...]]] = None

    @property
    def out_hw(self):
        return ((self.H + 2 * self.pad - self.k) // self.stride + 1, (self.W + 2 * self.pad - self.k) // self.stride + 1)

    @property
    def P(self):
        """Positions the weight gradient sums over."""
        return self.levels[0][-1] if self.levels is not None else self.N * self.out_hw[0] * self.out_hw[1]

    @property
    def K(self):
        return self.k * self.k * self.Cin

    @property
    def path(self):
        """The dX path `ops.ConvBackward` takes for this layer shape."""
        if not self.need_dx:
            return "none"
        if self.pad * 2 != self.k - 1:
            return "gather"
        return "same" if self.stride == 1 else "zero_insert"

    def shape(self):
        if self.levels is not None:
            return "levels " + "+".join(f"{h}x{w}" for h, w in self.levels[1])
        return f"{self.N}x{self.H}x{self.W}"


@dataclass
class Record:
    case: Case
    names: List[str]
    ranges: int
    plans: Dict[str, Optional[dict]] = field(default_factory=dict)     # mode -> the dgrad conv's plan (None: no dgrad conv ran)


def _ranges(c: Case) -> int:
    """Position ranges of the weight-gradient launch, from the workspace it asks for (none: one range)."""
    from embodied_object_detection_amd import _lib
    lib = _lib.load()
    if c.levels is not None:
        nb = lib.eod_conv2d_backward_weights_levels_workspace_bytes(c.P, c.Cin, c.Cout, c.k, c.k)
    else:
        nb = lib.eod_conv2d_backward_weights_workspace_bytes(c.N, c.H, c.W, c.Cin, c.Cout, c.k, c.k, c.pad, c.stride)
    per = (c.Cout * c.K + c.Cout) * 4
    assert nb % per == 0, (c, nb)
    return max(1, nb // per)


def _dgrad_plans(bw, c: Case) -> Dict[str, Optional[dict]]:
    """The plan of the input-gradient convolution's last descriptor in each arithmetic mode (a read-back, nothing is launched)."""
    if c.path not in ("same", "zero_insert"):
        return {m: None for m in MODES}
    return {m: plan_in(bw._dgrad_conv(), m) for m in MODES}


def _record(run) -> List[Record]:
    """Runs `run()` with ops.ConvBackward.__call__ wrapped (that also catches `_pyramid` through `levels=`) -> the distinct calls in
    first-seen order."""
    from embodied_object_detection_amd import ops
    orig = ops.ConvBackward.__call__
    seen: Dict[Case, Record] = {}

    def call(self, x, y, g_out, relu=False, need_dx=True, dx_res=None, dx_gate=None, levels=None):
        out = orig(self, x, y, g_out, relu=relu, need_dx=need_dx, dx_res=dx_res, dx_gate=dx_gate, levels=levels)
        cv = self.conv
        assert cv.KH == cv.KW, cv.name
        lv = None if levels is None else (tuple(int(o) for o in levels[0]), tuple((int(h), int(w)) for h, w in levels[1]))
        N, H, W = (1, 0, 0) if lv is not None else (int(x.shape[0]), int(x.shape[1]), int(x.shape[2]))
        c = Case(N, H, W, cv.Cin, cv.Cout, cv.KH, cv.stride, cv.pad, cin_pad=4 if cv.tap4 else 0, relu=bool(relu), need_dx=bool(need_dx),
                 res=dx_res is not None, gate=dx_gate is not None, levels=lv)
        ran = "none" if out["dx"] is None else "same" if self.same else "zero_insert" if self.zero_insert else "gather"
        assert ran == c.path, (cv.name, ran, c.path)
        if c not in seen:
            seen[c] = Record(c, [], _ranges(c), _dgrad_plans(self, c))
        if cv.name not in seen[c].names:
            seen[c].names.append(cv.name)
        return out

    ops.ConvBackward.__call__ = call
    try:
        run()
        torch.cuda.synchronize()
    finally:
        ops.ConvBackward.__call__ = orig
    return list(seen.values())


def _scene(seed: int, H: int, W: int, dev, n_cells: int = 4000):
    """A synthetic frame as tests/test_detector_training_gpu.py builds its 640x640 one: image, memory table + projection in 16-pixel
    blocks, 24 boxes of 12 .. 245 px with classes."""
    g = torch.Generator().manual_seed(seed)
    img = torch.randint(0, 256, (3, H, W), generator=g, dtype=torch.uint8)
    mem16 = (torch.randn((n_cells, 512), generator=g) * 2).half()
    proj = torch.randint(0, n_cells, (H // 16, W // 16), generator=g).repeat_interleave(16, 0).repeat_interleave(16, 1).contiguous()
    xy = torch.rand((24, 2), generator=g) * torch.tensor([W * 0.8, H * 0.8])
    wh = torch.exp(torch.rand((24, 2), generator=g) * 3.0 + 2.5)
    gt = torch.cat([xy, torch.minimum(xy + wh, torch.tensor([W - 1.0, H - 1.0]))], dim=1).contiguous()
    gc = torch.randint(0, 20, (24,), generator=g)
    return img.to(dev), gt.to(dev), gc.int().to(dev), (mem16.to(dev), proj.int().to(dev))


@pytest.fixture(scope="module")
def recorded(dev, synthetic_sd):
    """configuration -> the distinct ConvBackward calls of one training step (the only part that runs the whole model)."""
    from embodied_object_detection_amd import build_model, ops, setup_cfg
    from embodied_object_detection_amd.modeling.training import Trainer
    assert ops.get_conv_math() == "fp32"
    base = ["MODEL.MEMORY_TYPE", "implicit_memory", "MODEL.MAP_FEAT_FUSION", "sum", "MODEL.MAP_FEATURE_WEIGHT", 5, "SOLVER.BASE_LR", 2e-5,
            "FP16", False]
    trainers: Dict[tuple, object] = {}
    out = {}
    for name, (H, W, kind, B, extra) in CONFIGS.items():
        key = tuple(map(str, extra))
        if key not in trainers:
            sd0 = {k: v.clone() for k, v in synthetic_sd.items()}
            trainers[key] = Trainer(build_model(setup_cfg(None, base + extra), sd0), sd0)
        tr = trainers[key]
        scenes = [_scene(211 + b, H, W, dev) for b in range(B)]
        gen = torch.Generator(device=dev).manual_seed(1)
        if kind == "proposals":
            img, gt, gc, mem = scenes[0]
            run = lambda: tr.step_fn.forward_backward(img, gt, memory=mem)
        elif B == 1:
            img, gt, gc, mem = scenes[0]
            run = lambda: tr.fm.forward_backward(img, gt, gc, memory=mem, generator=gen)
        else:
            run = lambda: tr.fm.forward_backward_batch([s[0] for s in scenes], [s[1] for s in scenes], [s[2] for s in scenes],
                                                       [s[3] for s in scenes], generator=gen)
        out[name] = _record(run)
    del trainers
    torch.cuda.empty_cache()
    return out


# ------------------------------------------------------------------------------------------------
# seeded tensors, the operation on the CPU (float64 = reference, float32 = yardstick), the launches
# ------------------------------------------------------------------------------------------------
def _tensors(c: Case, seed: int) -> dict:
    g = torch.Generator().manual_seed(seed)
    cin = 3 if c.cin_pad else c.Cin
    t = {"w": torch.randn((c.Cout, cin, c.k, c.k), generator=g) * (1.0 / (cin * c.k * c.k)) ** 0.5,
         "b": torch.randn((c.Cout,), generator=g) * 0.1}
    if c.levels is not None:
        xs, gs = (c.P, c.Cin), (c.P, c.Cout)
    else:
        xs, gs = (c.N, c.H, c.W, c.Cin), (c.N,) + c.out_hw + (c.Cout,)
    t["x"] = torch.randn(xs, generator=g)
    if c.cin_pad:
        t["x"][..., cin:] = 0.0           # the preprocessed image's padding channel
    t["g"] = torch.randn(gs, generator=g)
    if c.res:
        t["res"] = torch.randn(xs, generator=g)
    if c.gate:
        t["gate"] = torch.relu(torch.randn(xs, generator=g))      # a ReLU output: zeros and positives
    return t


def _cpu_backward(c: Case, t: dict, dtype, y: Optional[torch.Tensor]) -> dict:
    """The call's operation in `dtype` on the CPU -> dw in the packed layout [Cout, (ky, kx, ci)] (the padded tap layout for the
    4-channel stem), db, dx (None without need_dx).  `y`: the device's own forward output, for the ReLU mask."""
    cin = 3 if c.cin_pad else c.Cin
    w = t["w"].to(dtype)
    g_all = t["g"].to(dtype)
    if c.relu:
        g_all = g_all * (y > 0).to(dtype)
    x_all = t["x"].to(dtype)[..., :cin]
    mask = [c.need_dx, True, True]

    def one(x, g):
        dx, dw, db = torch.ops.aten.convolution_backward(g.permute(0, 3, 1, 2), x.permute(0, 3, 1, 2), w, [c.Cout], [c.stride] * 2, [c.pad] * 2,
                                                         [1, 1], False, [0, 0], 1, mask)
        return (None if dx is None else dx.permute(0, 2, 3, 1)), dw, db

    if c.levels is not None:
        off, shapes = c.levels
        parts = [one(x_all[off[l]:off[l + 1]].view(1, h, w_, cin), g_all[off[l]:off[l + 1]].view(1, h, w_, c.Cout)) for l, (h, w_) in enumerate(shapes)]
        dw, db = sum(p[1] for p in parts), sum(p[2] for p in parts)
        dx = torch.cat([p[0].reshape(-1, cin) for p in parts]) if c.need_dx else None
    else:
        dx, dw, db = one(x_all, g_all)
    dw = dw.permute(0, 2, 3, 1)
    if c.cin_pad:
        dw = torch.nn.functional.pad(dw, (0, c.cin_pad - cin))
    if dx is not None:
        if c.res:
            dx = dx + t["res"].to(dtype)
        if c.gate:
            dx = torch.where(t["gate"] > 0, dx, torch.zeros((), dtype=dtype))
    return dict(dw=dw.reshape(c.Cout, -1), db=db, dx=dx)


class _Replay:
    """One case's layer, tensors on the device and launches."""

    def __init__(self, c: Case, dev, seed: int, tensors: Optional[dict] = None, bw=None):
        """`tensors` / `bw`: given ones instead of seeded tensors and a layer built from them."""
        from embodied_object_detection_amd import ops
        self.c, self.dev = c, dev
        self.t = _tensors(c, seed) if tensors is None else tensors
        self.d = {k: v.to(dev) for k, v in self.t.items() if k not in ("w", "b")}
        self.bw = bw if bw is not None else ops.ConvBackward(self.layer())
        self.y = None
        if c.relu:
            self.y = self.bw.conv(self.d["x"], c.N, c.H, c.W, relu=True,
                                  levels=None if c.levels is None else (list(c.levels[0]), list(c.levels[1])))

    def layer(self, w: Optional[torch.Tensor] = None):
        from embodied_object_detection_amd import ops
        c = self.c
        return ops.Conv(self.t["w"] if w is None else w, self.t["b"], stride=c.stride, pad=c.pad, device=self.dev,
                        cin_pad=c.cin_pad or None, name=f"replay {c.shape()} {c.Cin}->{c.Cout} k{c.k}s{c.stride}")

    def run(self, bw=None) -> dict:
        c, d = self.c, self.d
        return (bw or self.bw)(d["x"], self.y, d["g"], relu=c.relu, need_dx=c.need_dx, dx_res=d.get("res"), dx_gate=d.get("gate"),
                               levels=None if c.levels is None else (list(c.levels[0]), list(c.levels[1])))

    def run_in(self, mode: str, bw=None) -> Tuple[dict, Dict[str, Optional[dict]]]:
        """-> (the outputs in `mode`, the dgrad conv's plan in that mode); the process's mode is put back."""
        from embodied_object_detection_amd import ops
        prev = ops.set_conv_math(mode)
        try:
            out = self.run(bw)
            plan = (bw or self.bw)._dgrad_conv().plan() if self.c.path in ("same", "zero_insert") else None
        finally:
            ops.set_conv_math(prev)
        torch.cuda.synchronize()
        return out, plan


def _errors(got: torch.Tensor, ref: torch.Tensor) -> Tuple[float, float]:
    """(mean, max) of |got - ref| over rms(ref): every element is compared absolutely at the scale of the whole tensor, so an
    element whose reference is tiny is held to the same absolute error as the others, not skipped."""
    e = (got.double().reshape(-1) - ref.reshape(-1)).abs()
    rms = float(ref.double().pow(2).mean().sqrt())
    return float(e.mean()) / rms, float(e.max()) / rms


# Bounds, per output.  Against the CPU fp32 result of the same operation (both measured against fp64): mean error at most MEAN_X
# times, max error at most MAX_X times the CPU's (the forward module's factors); and an absolute cap on mean |err| / rms(ref) that
# does not depend on the CPU's own summation order.  dX is an `eod_conv2d` launch with K = Cout * k * k: the forward module's
# ceiling.  Measured worst (profiles/r07_gpu_tests_conv_backward.log): dX 0.90 x the CPU's mean, 1.09 x its max, 5.2e-7 of rms;
# db 1.24 x / 2.25 x, 4.3e-7.
#
# dW contracts over the P positions, up to 409 600 for the batch of four.  The factors hold for every single-image call but the
# tower (2.58 x the CPU's mean) and fail for the batches: fpn_output3 at N = 4 (25 600 positions in 6 ranges) reaches 3.92 x the
# CPU's mean and layer4.0.downsample at N = 2 4.49 x its max.  That is the kernel's order of summation, not a fault: one fp32
# accumulator adds the `chain` = P / ranges positions of a range in sequence, so its rounding error grows like sqrt(chain) (measured
# mean error / (2^-24 sqrt(chain)): 0.232 at N = 2, chain 2 133, and 0.232 at N = 4, chain 4 267, of that layer), while torch's CPU
# kernel sums in blocks and stays at 1.3e-7 .. 2.3e-7 of rms whatever P is.  So dW / db pass on the LARGER of the CPU yardstick and
# that rounding model: mean <= 0.35, max <= 6.5 times 2^-24 sqrt(chain) (measured worst among the calls that need it: 0.248 and
# 4.49).  One dropped chunk of 32 positions is sqrt(32 / P) of rms, 1.8e-2 at P = 102 400: four orders of magnitude above either.
MEAN_X, MAX_X = 2.5, 4.0
CHAIN_MEAN, CHAIN_MAX = 0.35, 6.5


def _cap(what: str, c: Case, chain: int) -> float:
    """Absolute cap on mean |err| / rms(ref).  dW / db: 3e-6 up to 16 384 positions per range (measured worst: 9.0e-7, fpn_output3 at
    N = 4), 1e-5 beyond (only the entry point without a workspace adds that many in one range)."""
    if what == "dx":
        return ceiling(c.Cout * c.k * c.k)
    return 3e-6 if chain <= 16384 else 1e-5


WORST: Dict[str, list] = {}            # what -> [ratio to the CPU's mean, ratio to its max, mean error, which case]


def _note(what: str, e, e32, who: str):
    w = WORST.setdefault(what, [0.0, "", 0.0, "", 0.0, ""])
    for i, v in ((0, e[0] / max(e32[0], 1e-30)), (2, e[1] / max(e32[1], 1e-30)), (4, e[0])):
        if v > w[i]:
            w[i], w[i + 1] = v, who
    return w


def _compare(c: Case, who: str, mode: str, out: dict, ref: dict, e32: dict, tag: str, what_list=("dw", "db", "dx"),
             ranges: Optional[int] = None) -> List[str]:
    """`ranges`: of the weight-gradient launch that made dW / db (default: what the shape gets with a workspace)."""
    bad = []
    chain = -(-c.P // (ranges or _ranges(c)))
    model = 2.0 ** -24 * math.sqrt(chain)
    for what in what_list:
        if ref[what] is None:
            if out[what] is not None:
                bad.append(f"{who}: a dX came back without need_dx")
            continue
        if out[what] is None or tuple(out[what].shape) != tuple(ref[what].shape):
            bad.append(f"{who}: {what} has shape {None if out[what] is None else tuple(out[what].shape)}, expected {tuple(ref[what].shape)}")
            continue
        e = _errors(out[what].cpu(), ref[what])
        print(f"{tag:22s} {who:58s} {what} [{mode:6s}] err/rms mean {e[0]:.2e} max {e[1]:.2e}   cpu fp32 mean {e32[what][0]:.2e} "
              f"max {e32[what][1]:.2e}", flush=True)
        _note(what, e, e32[what], who)
        if not math.isfinite(e[1]):
            bad.append(f"{who} [{mode}]: non-finite {what}")
        lim = (MEAN_X * e32[what][0], MAX_X * e32[what][1])
        if what != "dx":
            lim = (max(lim[0], CHAIN_MEAN * model), max(lim[1], CHAIN_MAX * model))
        if e[0] > lim[0]:
            bad.append(f"{who} [{mode}]: {what} mean error {e[0]:.3e} of rms > {lim[0]:.3e} (the CPU fp32 result's: {e32[what][0]:.3e})")
        if e[1] > lim[1]:
            bad.append(f"{who} [{mode}]: {what} max error {e[1]:.3e} of rms > {lim[1]:.3e} (the CPU fp32 result's: {e32[what][1]:.3e})")
        if e[0] > _cap(what, c, chain):
            bad.append(f"{who} [{mode}]: {what} mean error {e[0]:.3e} of rms above the cap {_cap(what, c, chain):.0e}")
    return bad


def _who(c: Case, names=()) -> str:
    n = names[0] + (f" (+{len(names) - 1})" if len(names) > 1 else "") if names else ""
    return (f"{n[-30:]:30s} " if names else "") + f"{c.shape()[-24:]} {c.Cin}->{c.Cout} k{c.k}s{c.stride}p{c.pad}"


def _describe(r: Record) -> str:
    c = r.case
    p = r.plans["fp32"]
    pl = "-" if p is None else (f"wave-K {p['wavek']}" if p["wavek"] else f"{p['bm']}x{p['bn']} BK{p['bk']}") + f" splitk {p['splitk']}x{p['cps']}"
    p3 = r.plans["bf16x3"]
    pl3 = "-" if p3 is None else ("bf16x3 " if p3["glds"] == 2 else "fp32 ") + f"{p3['bm']}x{p3['bn']} splitk {p3['splitk']}"
    flags = "".join(f for f, on in (("R", c.relu), ("+res", c.res), ("+gate", c.gate)) if on) or "-"
    return (f"{_who(c, r.names):84s} P {c.P:7d} K {c.K:5d} ranges {r.ranges:2d}  dX {c.path:11s} {flags:9s} dgrad fp32: {pl:30s} "
            f"bf16x3 mode: {pl3}")


def _check(c: Case, dev, tag: str, seed: int, expect: Optional[Record] = None, other: Optional[_Replay] = None, modes=MODES) -> List[str]:
    """Replays the case alone against fp64 in every mode -> the list of what is wrong with it (empty = fine).  With `expect`: the
    replay must get the recorded range count and dgrad plans.  With `other` (a replay of another shape): the case is run twice
    with `other` in between through the shared workspace and must repeat bitwise."""
    bad = []
    who = _who(c, expect.names if expect is not None else ())
    r = _Replay(c, dev, seed)
    y = None if r.y is None else r.y.cpu()
    ref = _cpu_backward(c, r.t, torch.float64, y)
    c32 = _cpu_backward(c, r.t, torch.float32, y)
    e32 = {k: None if ref[k] is None else _errors(c32[k], ref[k]) for k in ref}
    if expect is not None and _ranges(c) != expect.ranges:
        bad.append(f"{who}: replayed with {_ranges(c)} position ranges, the step ran {expect.ranges}")
    first = None
    for mode in modes:
        out, plan = r.run_in(mode)
        if expect is not None and plan != expect.plans[mode]:
            bad.append(f"{who} [{mode}]: dgrad conv replayed with plan {plan}, the step ran {expect.plans[mode]}")
        bad += _compare(c, who, mode, out, ref, e32, tag, ("dw", "db", "dx") if first is None else ("dx",))
        if first is None:
            first = out
            if other is not None:
                other.run()
                again = r.run()
                torch.cuda.synchronize()
                for what in ("dw", "db", "dx"):
                    if first[what] is not None and not torch.equal(first[what], again[what]):
                        bad.append(f"{who}: {what} differs between two runs through the shared workspace "
                                   f"({int((first[what] != again[what]).sum())} elements, {_ranges(c)} ranges)")
        else:
            for what in ("dw", "db"):
                if not torch.equal(first[what], out[what]):
                    bad.append(f"{who}: {what} in {mode} mode is not bitwise the fp32 mode's (the weight-gradient kernels do not read the mode)")
    return bad


# ------------------------------------------------------------------------------------------------
# 1. the production steps
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("config", list(CONFIGS))
def test_recording_holds_every_layer_group(recorded, config):
    recs = recorded[config]
    H, W, kind, B, extra = CONFIGS[config]
    names = [n for r in recs for n in r.names]
    print()
    for r in recs:
        print(f"{config:22s} {_describe(r)}")
    print(f"{config}: {len(recs)} distinct ConvBackward calls of {len(set(names))} layers")
    want = dict(HEAD_GROUPS)
    if kind == "full":
        want.update(BOX_GROUPS)
    if extra is not FROZEN:
        want.update(FPN_GROUPS)
    if not extra:
        want.update(TRUNK_GROUPS)
    for group, pred in want.items():
        assert any(pred(n) for n in names), f"{config}: no recorded ConvBackward call of group '{group}'"
    for group, pred in {**TRUNK_GROUPS, **FPN_GROUPS, **BOX_GROUPS}.items():
        if group not in want:
            assert not any(pred(n) for n in names), f"{config}: group '{group}' runs although nobody reads its gradients"
    # the loader carries no gt_masks and loss_mask is 0 (DetectorTraining): no mask layer has a backward
    assert not any("mask" in n for n in names), [n for n in names if "mask" in n]
    if not extra:
        assert sum(1 for n in set(names) if n == "stem" or ".layer" in n) == 53, "ResNet-50 has 53 convolutions"
        # + 6 FPN convs, P6 / P7, 4 tower convs and the head's output conv, 5 linear layers per cascade stage
        assert len(set(names)) == 53 + 6 + 2 + 5 + (15 if kind == "full" else 0), len(set(names))
        stem = [r for r in recs if "stem" in r.names]
        assert len(stem) == 1 and stem[0].case.cin_pad == 4 and not stem[0].case.need_dx and stem[0].case.N == B
        # the bottleneck shortcuts: conv1's input-gradient launch carries the shortcut's gradient and the ReLU below it
        assert any(r.case.res and r.case.gate and r.names[0].endswith(".conv1") for r in recs)
        assert any(r.case.path == "zero_insert" and r.case.k == 3 for r in recs) and any(r.case.path == "zero_insert" and r.case.k == 1 for r in recs)
        assert all(r.case.N == B for r in recs if any(".layer" in n or n.startswith("fpn_") for n in r.names))
    if extra is FROZEN_TRUNK:
        lat = [r for r in recs if any(n.startswith("fpn_lateral") for n in r.names)]
        assert lat and all(not r.case.need_dx for r in lat)
    # the level-shared layers run in pyramid mode over the five levels; nothing uses the separate ReLU launch (the gates ride on dX)
    lv = [r for r in recs if r.case.levels is not None]
    assert len(lv) == 2 and all(len(r.case.levels[1]) == 5 for r in lv) and not any(r.case.relu for r in recs)
    assert lv[0].case.levels[1][0] == (H // 8, W // 8) and lv[0].case.levels[1][-1] == (-(-H // 128), W // 128)
    # up to the kernels' limit of 64 ranges; the plan of every dgrad conv was read back
    assert (max(r.ranges for r in recs) == 64 if not extra else max(r.ranges for r in recs) >= 22) and min(r.ranges for r in recs) == 1
    assert all((r.plans["fp32"] is None) == (r.case.path in ("none", "gather")) for r in recs)
    assert not any(r.case.path == "gather" for r in recs), "every strided production layer is 'same'-padded: zero insertion"


def _union(recorded) -> List[Tuple[str, Record]]:
    """Every distinct case of all configurations once, under the first configuration that ran it."""
    seen, out = {}, []
    for config, recs in recorded.items():
        for r in recs:
            if r.case not in seen:
                seen[r.case] = r
                out.append((config, r))
            else:
                assert (seen[r.case].ranges, seen[r.case].plans) == (r.ranges, r.plans), (config, r.case)
    return out


def test_production_calls_match_fp64_in_both_modes_and_repeat_bitwise(dev, recorded):
    """Every distinct production call against fp64 (dW, db, dX; fp32 and bf16x3), with the recorded range count and dgrad plan, and
    run twice through the one shared workspace with a call of another shape in between: bitwise the same."""
    cases = _union(recorded)
    print(f"\n{len(cases)} distinct production calls over {len(recorded)} configurations")
    other = _Replay(Case(2, 23, 31, 96, 160, 3, 1, 1), dev, 77)          # 11 ranges of its own in the shared workspace
    assert _ranges(other.c) > 1
    bad = []
    for i, (config, r) in enumerate(cases):
        bad += _check(r.case, dev, config, 1000 + i, expect=r, other=other)
    for what, w in WORST.items():
        print(f"worst {what}: mean {w[0]:.2f} x the CPU fp32 mean ({w[1].strip()}), max {w[2]:.2f} x its max ({w[3].strip()}), "
              f"mean err/rms {w[4]:.2e} ({w[5].strip()})")
    assert not bad, f"{len(bad)} findings:\n" + "\n".join(bad)


def test_f16_arithmetic_stays_refused_for_training():
    from embodied_object_detection_amd import ops
    from embodied_object_detection_amd.modeling.training import Trainer
    prev = ops.set_conv_math("f16")
    try:
        with pytest.raises(ValueError, match="f16"):
            Trainer(None, {})                 # refused before anything of the model is touched
    finally:
        ops.set_conv_math(prev)
    assert ops.get_conv_math() == prev


# ------------------------------------------------------------------------------------------------
# 2. contracts the production calls keep
# ------------------------------------------------------------------------------------------------
def test_batch_gradients_are_the_sum_over_the_images(dev, recorded):
    """The shared-trunk batch of four: dW / db of the N = 4 call against the fp64 SUM of the four images' own gradients, dX of image
    i against that image's own fp64 gradient (no bitwise promise for the backward: see the module's docstring; how many images
    happen to be bitwise their N = 1 call is printed)."""
    recs = recorded["640x640 batch4"]
    pick = {}
    for r in recs:
        if r.case.N == 4:
            for group, pred in {**TRUNK_GROUPS, **FPN_GROUPS}.items():
                if any(pred(n) for n in r.names):
                    pick.setdefault(group, r)
    assert set(pick) == set(TRUNK_GROUPS) | set(FPN_GROUPS), sorted(pick)
    bad = []
    for j, (group, r) in enumerate(pick.items()):
        c = r.case
        one = Case(**{**c.__dict__, "N": 1})
        rp = _Replay(c, dev, 3000 + j)
        out = rp.run()
        torch.cuda.synchronize()
        parts64, parts32, same = [], [], 0
        for i in range(4):
            ti = {k: (v[i:i + 1] if k not in ("w", "b") else v) for k, v in rp.t.items()}
            parts64.append(_cpu_backward(one, ti, torch.float64, None))
            parts32.append(_cpu_backward(one, ti, torch.float32, None))
            if c.need_dx:
                same += int(torch.equal(_Replay(one, dev, 0, tensors=ti, bw=rp.bw).run()["dx"], out["dx"][i:i + 1]))
        ref = dict(dw=sum(p["dw"] for p in parts64), db=sum(p["db"] for p in parts64),
                   dx=torch.cat([p["dx"] for p in parts64]) if c.need_dx else None)
        c32 = dict(dw=sum(p["dw"] for p in parts32), db=sum(p["db"] for p in parts32),
                   dx=torch.cat([p["dx"] for p in parts32]) if c.need_dx else None)
        e32 = {k: None if ref[k] is None else _errors(c32[k], ref[k]) for k in ref}
        bad += _compare(c, _who(c, r.names), "fp32", out, ref, e32, "batch4 vs images")
        if c.need_dx:
            print(f"    {group}: dX of {same} of 4 images is bitwise the image's own N = 1 call")
    assert not bad, "\n".join(bad)


def test_stale_rotated_weights_are_not_used_after_a_weight_update(dev):
    """The dgrad conv keeps rotated weights and, in bf16x3 mode, their bf16 pieces (`w_split`).  After the layer's weights are
    written in place, `ConvBackward.refresh_all` (the trainer's path) and the lazy per-layer refresh at the next call must both
    give bitwise the dX of a layer built freshly from the new weights.  Only the 256x128 bf16x3 kernel reads the pieces (the
    smaller tiles split the fp32 weights as they load them), so the shapes are ones whose dgrad conv gets that tile: fpn_lateral3
    of the batch of four, layer2.0.downsample of the batch of two (zero-inserted) and a pyramid of 33 600 rows."""
    from embodied_object_detection_amd import ops
    lv = ((0, 25600, 32000, 33600), ((160, 160), (80, 80), (40, 40)))
    for j, c in enumerate((Case(4, 80, 80, 512, 256, 1), Case(2, 160, 160, 256, 512, 1, 2, 0), Case(1, 0, 0, 256, 256, 3, 1, 1, levels=lv))):
        for how in ("refresh_all", "lazy"):
            r = _Replay(c, dev, 4000 + j)
            before, plan = r.run_in("bf16x3")
            assert plan["glds"] == 2 and plan["tile"] == 4 and r.bw._flipped.w_split is not None, (c, plan)
            new_w = torch.randn(r.t["w"].shape, generator=torch.Generator().manual_seed(4100 + j)) * 0.05
            packed, _ = ops.pack_conv_weight(new_w)
            r.bw.conv.w.copy_(packed.to(dev))                      # the stepped weights, written in place
            if how == "refresh_all":
                ops.ConvBackward.refresh_all([r.bw])
            after, _ = r.run_in("bf16x3")
            fresh, _ = r.run_in("bf16x3", bw=ops.ConvBackward(r.layer(new_w)))
            assert not torch.equal(before["dx"], after["dx"])
            assert torch.equal(after["dx"], fresh["dx"]), f"{c} after {how}: dX differs from a freshly built layer's " \
                f"({int((after['dx'] != fresh['dx']).sum())} elements): stale rotated weights or bf16x3 pieces"
            assert torch.equal(after["dw"], before["dw"]) and torch.equal(after["db"], before["db"])     # they do not read the weights


def _wgrad_direct(c: Case, d: dict, dw, db, ws, ws_bytes: int):
    """The C entry points on caller-owned buffers (`ops.ConvBackward` allocates its own)."""
    import ctypes as C
    from embodied_object_detection_amd import _lib, ops
    lib = _lib.load()
    if c.levels is not None:
        off, shapes = c.levels
        L = len(shapes)
        _lib.check(lib.eod_conv2d_backward_weights_levels(d["x"].data_ptr(), d["g"].data_ptr(), L, (C.c_int32 * (L + 1))(*off),
                                                          (C.c_int32 * L)(*[h for h, _ in shapes]), (C.c_int32 * L)(*[w for _, w in shapes]),
                                                          c.Cin, c.Cout, c.k, c.k, c.pad, dw.data_ptr(), db.data_ptr(),
                                                          None if ws is None else ws.data_ptr(), ws_bytes, ops._stream()), "wgrad levels")
    elif ws is None:
        _lib.check(lib.eod_conv2d_backward_weights(d["x"].data_ptr(), d["g"].data_ptr(), c.N, c.H, c.W, c.Cin, c.Cout, c.k, c.k, c.pad, c.stride,
                                                   dw.data_ptr(), db.data_ptr(), ops._stream()), "wgrad")
    else:
        _lib.check(lib.eod_conv2d_backward_weights_ws(d["x"].data_ptr(), d["g"].data_ptr(), c.N, c.H, c.W, c.Cin, c.Cout, c.k, c.k, c.pad, c.stride,
                                                      dw.data_ptr(), db.data_ptr(), ws.data_ptr(), ws_bytes, ops._stream()), "wgrad ws")


def _one_per_group(recs: List[Record]) -> Dict[str, Record]:
    """group -> its recorded case with the most positions."""
    pick: Dict[str, Record] = {}
    for r in recs:
        for group, pred in {**TRUNK_GROUPS, **FPN_GROUPS, **HEAD_GROUPS, **BOX_GROUPS}.items():
            if any(pred(n) for n in r.names) and (group not in pick or r.case.P > pick[group].case.P):
                pick[group] = r
    return pick


@pytest.mark.parametrize("config", ["640x640 full", "480x640 full"])
def test_outputs_are_fully_written_and_nothing_else_is(dev, recorded, config):
    """One production case per layer group on caller-owned buffers: dW [Cout, K] and db [Cout] pre-filled with NaN come back without
    one, their guard rows (and dX's) keep the sentinel, the workspace's unused tail keeps its NaN bit for bit and none of it reaches
    dW; the used part of the workspace is written completely (no NaN left: an unwritten range would poison the reduce)."""
    bad = []
    for j, rec in enumerate(_one_per_group(recorded[config]).values()):
        c = rec.case
        who = _who(c, rec.names)
        r = _Replay(c, dev, 5000 + j)
        want = r.run()
        f = dict(dtype=torch.float32, device=dev)
        dw = torch.full((c.Cout + 1, c.K), float("nan"), **f)
        db = torch.full((c.Cout + 32,), float("nan"), **f)
        dw[c.Cout:] = SENTINEL
        db[c.Cout:] = SENTINEL
        per = c.Cout * c.K + c.Cout
        used = rec.ranges * per if rec.ranges > 1 else 0
        ws = torch.full((used + 4096,), float("nan"), **f)
        _wgrad_direct(c, r.d, dw, db, ws, ws.numel() * 4)
        torch.cuda.synchronize()
        if not (torch.equal(dw[:c.Cout], want["dw"]) and torch.equal(db[:c.Cout], want["db"])):
            bad.append(f"{who}: dW / db on NaN-filled buffers and workspace differ from the plain call's (or hold NaN)")
        if not (bool((dw[c.Cout:] == SENTINEL).all()) and bool((db[c.Cout:] == SENTINEL).all())):
            bad.append(f"{who}: the guard row behind dW / db was written")
        if bool(torch.isnan(ws[:used]).any()) or not bool(torch.isnan(ws[used:]).all()):
            bad.append(f"{who}: the workspace's {rec.ranges} partial results are not exactly what was written")
        if c.path in ("same", "zero_insert"):
            g = r.d["g"]
            if c.path == "zero_insert":
                g = torch.zeros((c.N, c.H, c.W, c.Cout), **f)
                g[:, ::c.stride, ::c.stride] = r.d["g"]
            rows = c.P if c.levels is not None else c.N * c.H * c.W
            dx = torch.full((rows + 1, c.Cin), float("nan"), **f)
            dx[rows:] = SENTINEL
            kw = dict(res=r.d.get("res"), res_mode=1 if c.res else 0, gate=r.d.get("gate"), out=dx[:rows].view(want["dx"].shape))
            if c.levels is not None:
                kw["levels"] = (list(c.levels[0]), list(c.levels[1]))
            r.bw._dgrad_conv()(g, c.N, c.H, c.W, **kw)
            torch.cuda.synchronize()
            if not torch.equal(dx[:rows].view(want["dx"].shape), want["dx"]):
                bad.append(f"{who}: dX on a NaN-filled buffer differs from the plain call's (or holds NaN)")
            if not bool((dx[rows:] == SENTINEL).all()):
                bad.append(f"{who}: the guard row behind dX was written")
    assert not bad, "\n".join(bad)


# ------------------------------------------------------------------------------------------------
# 3. edges the production list does not hold but the kernels' index arithmetic invites
# ------------------------------------------------------------------------------------------------
def _run_edges(dev, tag, cases, seed0) -> None:
    bad = []
    other = _Replay(Case(1, 17, 19, 64, 64, 1), dev, 78)
    for i, c in enumerate(cases):
        bad += _check(c, dev, tag, seed0 + i, other=other)
    assert not bad, "\n".join(bad)


def _split(c: Case) -> Tuple[int, int, int]:
    """(chunks of 32 positions, ranges, chunks per range) of the LDS-tiled weight-gradient kernel."""
    chunks = -(-c.P // 32)
    s = _ranges(c)
    return chunks, s, -(-chunks // s)


def test_position_counts_around_a_chunk_multiple(dev):
    """P = 32 k - 1, 32 k, 32 k + 1 (the last chunk of the last range holds 31, 32, 1 positions), single- and multi-range."""
    cases = []
    for P in (31, 32, 33, 32 * 40 - 1, 32 * 40, 32 * 40 + 1, 32 * 257 + 1):
        h, w = exact_hw(P)
        cases.append(Case(1, h, w, 64, 64, 3 if h > 1 else 1, 1, 1 if h > 1 else 0))
    assert [_ranges(c) for c in cases[:3]] == [1, 1, 1] and all(_ranges(c) > 1 for c in cases[3:])
    _run_edges(dev, "P around 32 k", cases, 6000)


def test_few_positions_cap_the_ranges_and_an_empty_last_range_adds_zeros(dev):
    """`cap` = a quarter of the chunks limits the ranges of a small layer; and chunk counts the ranges do not divide leave the last
    ranges EMPTY (`cps * (splits - 1) >= chunks`): they must contribute exact zeros to the reduce."""
    small = [Case(1, 10, 30, 64, 64, 1), Case(1, 16, 16, 32, 64, 3, 1, 1), Case(3, 5, 9, 64, 32, 1)]
    for c, want in zip(small, (2, 2, 1)):
        assert _ranges(c) == want == max(1, _split(c)[0] // 4), (c, _ranges(c))
    empty = [Case(1, 65, 128, 64, 64, 1), Case(1, 52, 160, 32, 32, 3, 1, 1), Case(2, 65, 64, 64, 32, 1)]
    for c in empty:
        chunks, s, cps = _split(c)
        assert s == 64 and cps * (s - 1) >= chunks, (c, chunks, s, cps)
    _run_edges(dev, "ranges", small + empty, 6100)


def test_half_filled_channel_tiles(dev):
    """Cin / Cout of 32, 96 and 160: the 64 x 64 tile's second half is switched off on one or both sides (`g_ok` / `x_ok`, the
    guarded stores), db written by one tile column only."""
    cases = [Case(1, 21, 27, ci, co, k, 1, k // 2) for ci, co, k in ((32, 32, 3), (96, 96, 1), (160, 160, 3), (64, 32, 3), (32, 64, 1), (96, 160, 1),
                                                                     (160, 32, 1), (32, 96, 3))]
    cases.append(Case(1, 0, 0, 96, 32, 3, 1, 1, levels=((0, 21 * 27, 21 * 27 + 11 * 14, 21 * 27 + 11 * 14 + 6 * 7), ((21, 27), (11, 14), (6, 7)))))
    _run_edges(dev, "half tiles", cases, 6200)


def test_image_boundaries_inside_a_chunk(dev):
    """N = 2 and 3 with OH * OW not a multiple of 32: a chunk of 32 positions holds the end of one image and the start of the next,
    whose border taps must not read across; with the ReLU launch (`relu=True`, unused by the production steps) as well."""
    cases = [Case(2, 13, 9, 64, 64, 3, 1, 1), Case(3, 7, 11, 96, 64, 3, 1, 1, relu=True), Case(3, 13, 15, 64, 128, 3, 2, 1),
             Case(2, 9, 7, 32, 64, 5, 1, 2, relu=True), Case(3, 11, 13, 64, 64, 1, res=True, gate=True)]
    assert all((c.out_hw[0] * c.out_hw[1]) % 32 for c in cases)
    _run_edges(dev, "image boundaries", cases, 6300)


def test_stride_2_on_odd_sizes(dev):
    """Stride 2 on odd H and W: 3x3 pad 1 and 1x1 pad 0 (zero-inserted dX: the `up` tensor's last row / column), the 4-channel stem
    forms 7x7 and 5x5 (weight gradient only, padded tap layout), and one layer that is not 'same'-padded (3x3 pad 0: the gather
    kernel `eod_conv2d_backward_input`), with the fused epilogue's arguments on both dX paths."""
    cases = [Case(1, 37, 45, 128, 128, 3, 2, 1), Case(2, 21, 33, 64, 256, 1, 2, 0), Case(1, 37, 45, 64, 96, 3, 2, 1, res=True, gate=True),
             Case(2, 37, 45, 4, 64, 7, 2, 3, cin_pad=4, need_dx=False), Case(1, 51, 39, 4, 64, 5, 2, 2, cin_pad=4, need_dx=False),
             Case(2, 19, 23, 64, 96, 3, 2, 0), Case(1, 19, 23, 32, 64, 3, 2, 0, res=True, gate=True), Case(1, 20, 24, 64, 64, 3, 1, 0)]
    assert [c.path for c in cases] == ["zero_insert"] * 3 + ["none"] * 2 + ["gather"] * 3
    _run_edges(dev, "stride 2 / odd", cases, 6400)


def test_entry_point_without_a_workspace_runs_one_range(dev, recorded):
    """`eod_conv2d_backward_weights` (no workspace: one range over all positions) at production shapes, against fp64."""
    bad = []
    pick = _one_per_group(recorded["640x640 full"])
    recs = [pick[group] for group in ("trunk 1x1", "trunk 3x3", "FPN output", "bbox_pred.0")]
    assert all(r.ranges > 1 for r in recs)
    for j, rec in enumerate(recs):
        c = rec.case
        r = _Replay(c, dev, 6500 + j)
        ref = _cpu_backward(c, r.t, torch.float64, None)
        c32 = _cpu_backward(c, r.t, torch.float32, None)
        e32 = {k: None if ref[k] is None else _errors(c32[k], ref[k]) for k in ref}
        out = dict(dw=torch.full((c.Cout, c.K), float("nan"), device=dev), db=torch.full((c.Cout,), float("nan"), device=dev))
        _wgrad_direct(c, r.d, out["dw"], out["db"], None, 0)
        torch.cuda.synchronize()
        bad += _compare(c, _who(c, rec.names), "fp32", out, ref, e32, "no workspace", ("dw", "db"), ranges=1)
    assert not bad, "\n".join(bad)


# ------------------------------------------------------------------------------------------------
# 4. the fallback weight-gradient kernels: one fresh process per setting
# ------------------------------------------------------------------------------------------------
FALLBACK_CASES = [Case(1, 160, 160, 64, 64, 3, 1, 1), Case(1, 80, 80, 256, 512, 1, 2, 0), Case(2, 40, 40, 256, 256, 3, 1, 1),
                  Case(512, 1, 1, 1024, 32, 1), Case(2, 13, 9, 96, 160, 3, 1, 1), Case(1, 33, 1, 32, 32, 1), Case(1, 8, 29, 64, 64, 1)]


def _fallback_child() -> int:
    """What a child process runs: the weight gradients of FALLBACK_CASES under the EOD_WGRAD_* setting it was started with."""
    from embodied_object_detection_amd import _lib
    _lib.load()
    dev = torch.device("cuda:0")
    tag = "LDS=%s RB=%s" % (os.environ.get("EOD_WGRAD_LDS", "-"), os.environ.get("EOD_WGRAD_RB", "-"))
    per_tile = 32 if os.environ.get("EOD_WGRAD_RB") == "0" else 64
    bad = []
    for i, c in enumerate(FALLBACK_CASES):
        # the range count is the fallback's own (steps of 8 positions, a cap of a 16th of them), not the LDS kernel's
        wgs = -(-c.Cout // per_tile) * -(-c.Cin // per_tile) * c.k * c.k
        want = max(1, min(64, -(-768 // wgs), -(-c.P // 8) // 16))
        if _ranges(c) != want:
            bad.append(f"{_who(c)}: {_ranges(c)} ranges, expected {want} from this setting's own split rule: the setting was not read")
        bad += _check(Case(**{**c.__dict__, "need_dx": False}), dev, tag, 7000 + i, modes=("fp32",))
    for b in bad:
        print("FINDING", b)
    return 1 if bad else 0


def test_fallback_weight_gradient_kernels_in_child_processes():
    """`EOD_WGRAD_LDS=0` (register-blocked 64 x 64 kernel) and `EOD_WGRAD_LDS=0 EOD_WGRAD_RB=0` (32 x 32 kernel): production
    shapes and edge shapes against fp64, one child at a time, stopping at the first that fails.  The children check that their
    setting was read by the range counts: the fallbacks cut 232 positions into one range, the LDS-tiled kernel of this process
    into two."""
    from embodied_object_detection_amd import _lib
    _lib.load()
    assert _ranges(FALLBACK_CASES[-1]) == 2
    for env in ({"EOD_WGRAD_LDS": "0"}, {"EOD_WGRAD_LDS": "0", "EOD_WGRAD_RB": "0"}):
        p = subprocess.run([sys.executable, os.path.abspath(__file__)], env={**os.environ, **env}, cwd=ROOT, timeout=300,
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        print(p.stdout)
        assert p.returncode == 0, f"child with {env} ended with status {p.returncode}:\n{p.stdout[-4000:]}"


if __name__ == "__main__":
    sys.exit(_fallback_child())
