"""Every non-convolution launch the full-size training steps really run, against a float64 reference.

The convolution launches of the training step have their own module (test_conv_backward_plans_gpu.py).  This one records the other
half the same way: one training step of each production configuration (the seven of that module, 960x960, and 640x640 under
`FP16: True`) with the entry points wrapped -- `ops.roi_align`, `ops.roi_align_backward`, `ops.groupnorm_relu`,
`ops.groupnorm_relu_backward`, `ops.MemoryProjectorBackward.__call__`, `ops.memory_gather_pool`, `ops.zs_logits`,
`ops.zs_logits_backward`, `ops.AdamW.nonfinite` and, on the loaded library object, `eod_relu_backward`,
`eod_upsample2_sum_backward`, `eod_maxpool3x3s2_backward` -- every call kept that is distinct in its arguments, the ROIAlign calls with
the real box lists of the cascade's three stages.  Each case is then replayed alone: seeded inputs (or the recorded boxes), the HIP
entry point called as recorded, the same operation in float64 on the CPU written out here; torch's CPU fp32 result of that operation
is printed beside it as the yardstick (`pytest -s`: one line per recorded case, one line per comparison with measured error,
yardstick error and bound).

Bounds come from the arithmetic (U = 2^-24, the number of roundings, the magnitudes they act on) with the head-room factor written
out, or -- where the operation is a long fp32 sum whose order is the kernel's own -- from the rule the convolution module derived:
the larger of a multiple of the CPU fp32 error and the rounding model of a sequential fp32 chain.

The six gaps this closes, by name:
  1. ROIAlign backward, gather form, at R > 64 and C = 256 against float64 including the non-zero cell set
     (test_roi_align_backward_gather_form_*); the rows and sample-tap forms in child processes (EOD_ROI_BWD_ROWS /
     EOD_ROI_BWD_SAMPLES) and at C = 320 (test_roi_align_backward_fallback_forms_*).
  2. GroupNorm + ReLU forward and backward at the recorded five-level pyramids, the backward fed by the fused statistics of the
     tower convolution's slab reduce as well as by the forward's own statistics launch (test_groupnorm_*).
  3. The memory projection's backward at the three production sizes with need_input_grad=False and True, and without a workspace
     (test_memory_projection_backward_*).
  4. The three trunk kernels (up-sample-add, max pool, ReLU backward) at the recorded N, H, W, C including N = 4
     (test_trunk_kernels_*).
  5. zs_logits_backward at the recorded B for 21 and 1204 columns (test_zs_logits_*).
  6. ROIAlign forward on the recorded lists with a derived bound (test_roi_align_forward_*).
"""
import math
import os
import subprocess
import sys
from typing import Dict, List, Optional, Tuple

import numpy as np
import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if __name__ == "__main__":
    sys.path[:0] = [ROOT, os.path.dirname(os.path.abspath(__file__))]

from _launch_cases import (ROI_HEAD, SENTINEL, U, Recorder, RoiRef, fragments_to_rows, hostile_boxes, roi_forward_reference,    # noqa: E402
                           roi_geometry)

pytestmark = pytest.mark.gpu

LVIS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lvis_v1_clip.npy")
FROZEN = ["MODEL.FREEZE_BACKBONE", True, "MODEL.UNFROZEN_LAYERS", ["roi", "map_merge", "proposal_generator"]]
FROZEN_TRUNK = ["MODEL.FREEZE_BACKBONE", True, "MODEL.UNFROZEN_LAYERS", ["roi", "map_merge", "proposal_generator", "fpn_"]]
# configuration -> (H, W, which step, frames that share the trunk pass, config overrides, FP16)
CONFIGS = {
    "640x640 full": (640, 640, "full", 1, [], False),
    "640x640 proposals": (640, 640, "proposals", 1, [], False),
    "640x640 batch2": (640, 640, "full", 2, [], False),
    "640x640 batch4": (640, 640, "full", 4, [], False),
    "480x640 full": (480, 640, "full", 1, [], False),
    "640x640 frozen": (640, 640, "full", 1, FROZEN, False),
    "640x640 frozen trunk": (640, 640, "full", 1, FROZEN_TRUNK, False),
    "960x960 full": (960, 960, "full", 1, [], False),
    "640x640 fp16": (640, 640, "amp", 1, [], True),
}
# families a recorded step must contain (a refactor that renames a call must not silently empty the list)
ROI_FAMILIES = ("roi_align", "roi_align_backward", "zs_logits", "zs_logits_backward")
TOWER_FAMILIES = ("groupnorm_relu", "groupnorm_relu_backward")
MEMORY_FAMILIES = ("memory_gather_pool", "memory_projector_backward")
TRUNK_FAMILIES = ("upsample2_sum_backward", "relu_backward")
ALL_FAMILIES = ROI_FAMILIES + TOWER_FAMILIES + MEMORY_FAMILIES + TRUNK_FAMILIES + ("maxpool3x3s2_backward", "nonfinite")


def _expected_families(config: str) -> set:
    H, W, kind, B, extra, fp16 = CONFIGS[config]
    want = set(TOWER_FAMILIES) | set(MEMORY_FAMILIES)
    if kind != "proposals":
        want |= set(ROI_FAMILIES)
    if extra is not FROZEN:
        want |= set(TRUNK_FAMILIES)              # the FPN's top-down add; the ReLU between P6 and P7 runs in every configuration
    else:
        want |= {"relu_backward"}
    if not extra:
        want |= {"maxpool3x3s2_backward"}
    if fp16:
        want |= {"nonfinite"}
    return want


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    from embodied_object_detection_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def _scene(seed: int, H: int, W: int, dev, n_cells: int = 4000):
    """A synthetic frame as test_conv_backward_plans_gpu.py builds it: image, memory table + projection in 16-pixel blocks, 24 boxes."""
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
def recorded(dev, synthetic_sd) -> Dict[str, Dict[str, Dict[tuple, dict]]]:
    """configuration -> family -> {arguments: payload} of one training step (the only part that runs the whole model).  One model per
    set of overrides, built when first needed and freed before the next."""
    from embodied_object_detection_amd import build_model, ops, setup_cfg
    from embodied_object_detection_amd.modeling.training import AmpTrainer, Trainer, build_trainer
    assert ops.get_conv_math() == "fp32"
    base = ["MODEL.MEMORY_TYPE", "implicit_memory", "MODEL.MAP_FEAT_FUSION", "sum", "MODEL.MAP_FEATURE_WEIGHT", 5, "SOLVER.BASE_LR", 2e-5]
    out = {}
    order = sorted(CONFIGS, key=lambda n: (str(CONFIGS[n][4]), CONFIGS[n][5]))          # configurations of one model side by side
    key, tr = None, None
    for name in order:
        H, W, kind, B, extra, fp16 = CONFIGS[name]
        if key != (str(extra), fp16):
            tr = None
            torch.cuda.empty_cache()
            sd0 = {k: v.clone() for k, v in synthetic_sd.items()}
            tr = build_trainer(build_model(setup_cfg(None, base + ["FP16", fp16] + extra), sd0), sd0)
            assert type(tr) is (AmpTrainer if fp16 else Trainer)
            key = (str(extra), fp16)
        scenes = [_scene(211 + b, H, W, dev) for b in range(B)]
        gen = torch.Generator(device=dev).manual_seed(1)
        img, gt, gc, mem = scenes[0]
        if kind == "proposals":
            run = lambda: tr.step_fn.forward_backward(img, gt, memory=mem)
        elif kind == "amp":
            run = lambda: tr.step(img, gt, memory=mem, gt_classes=gc, generator=gen)           # with the found-inf pass and the optimizer
        elif B == 1:
            run = lambda: tr.fm.forward_backward(img, gt, gc, memory=mem, generator=gen)
        else:
            run = lambda: tr.fm.forward_backward_batch([s[0] for s in scenes], [s[1] for s in scenes], [s[2] for s in scenes],
                                                       [s[3] for s in scenes], generator=gen)
        with Recorder() as rec:
            run()
            torch.cuda.synchronize()
        out[name] = rec.calls
    tr = None
    torch.cuda.empty_cache()
    return {name: out[name] for name in CONFIGS}


def _fmt(family: str, key: tuple, payload: dict) -> str:
    if family == "nonfinite":
        live = [n for n in key if n >= 0]
        return f"{len(live)} tensors, {sum(live)} elements, {sum(1 for n in live if n % 1024)} not a multiple of 1024"
    if family.startswith("groupnorm"):
        off = key[0]
        return f"rows {off[-1]} in levels {[off[i + 1] - off[i] for i in range(len(off) - 1)]} " + " ".join(map(str, key[1:]))
    s = " ".join(str(k) for k in key)
    if "boxes" in payload:
        s += f"  box lists kept: {[tuple(b.shape) for b in payload['boxes']]}"
    return s


def _union(recorded, family: str) -> Dict[tuple, Tuple[str, dict]]:
    """Every distinct call of a family over all configurations, under the first configuration that made it."""
    out: Dict[tuple, Tuple[str, dict]] = {}
    for config, fams in recorded.items():
        for key, payload in fams.get(family, {}).items():
            out.setdefault(key, (config, payload))
    return out


def _line(tag: str, what: str, err: float, yard: float, bound: float, extra: str = "") -> None:
    print(f"{tag:44s} {what:12s} err {err:.3e}  cpu fp32 {yard:.3e}  bound {bound:.3e}  ({err / max(bound, 1e-300):.3f} of it) {extra}", flush=True)


def _worst(err: torch.Tensor, e32: torch.Tensor, bound: torch.Tensor) -> Tuple[float, float, float]:
    """(error, CPU fp32 error, bound) at the element whose error is the largest share of its bound."""
    err, e32, bound = err.detach(), e32.detach(), bound.detach()
    i = int((err / bound.clamp(min=1e-300)).argmax())
    return float(err.reshape(-1)[i]), float(e32.reshape(-1)[i]), float(bound.reshape(-1)[i])


def _rms_errors(got: torch.Tensor, ref: torch.Tensor) -> Tuple[float, float]:
    """(mean, max) of |got - ref| over rms(ref): every element held to the same absolute error at the scale of the whole tensor."""
    e = (got.double().reshape(-1) - ref.double().reshape(-1)).abs()
    rms = float(ref.double().pow(2).mean().sqrt())
    return float(e.mean()) / rms, float(e.max()) / rms


# the convolution modules' factors over the CPU fp32 error (mean, max) and their rounding model of a sequential fp32 chain
MEAN_X, MAX_X = 2.5, 4.0
CHAIN_MEAN, CHAIN_MAX = 0.35, 6.5


# ------------------------------------------------------------------------------------------------
# 1. what the steps launch
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("config", list(CONFIGS))
def test_recording_holds_every_family(recorded, config):
    H, W, kind, B, extra, fp16 = CONFIGS[config]
    fams = recorded[config]
    print()
    for family in ALL_FAMILIES:
        for key, payload in fams.get(family, {}).items():
            print(f"{config:22s} {family:26s} x{payload['n']:<3d} {_fmt(family, key, payload)}")
    want = _expected_families(config)
    for family in want:
        assert fams.get(family), f"{config}: no recorded call of family '{family}'"
    for family in ALL_FAMILIES:
        if family not in want:
            assert not fams.get(family), f"{config}: family '{family}' runs although nothing should need it: {list(fams[family])}"
    h3, w3 = H // 8, W // 8
    off = [0]
    for l in range(5):
        off.append(off[-1] + (-(-H // (8 << l))) * (-(-W // (8 << l))))
    # the tower: four GroupNorm layers forward and backward per frame over the five-level pyramid, statistics by their own launch
    for family in TOWER_FAMILIES:
        keys = list(fams[family])
        assert len(keys) == 1 and keys[0][0] == tuple(off) and keys[0][1:3] == (256, 32), (config, keys)
        assert fams[family][keys[0]]["n"] == 4 * B
    assert list(fams["groupnorm_relu"])[0][4:] == (False, False)
    assert list(fams["memory_projector_backward"]) == [(H, W, 5.0, False)], "the step needs dW / db only"
    assert all(k[:2] == (H, W) and k[3] == 512 for k in fams["memory_gather_pool"])
    if kind != "proposals":
        # three cascade stages per frame, forward and backward, on the same number of sampled rows; real boxes kept
        assert set(fams["roi_align"]) == {k + (False, 1, False) for k in fams["roi_align_backward"]}, (list(fams["roi_align"]), list(fams["roi_align_backward"]))
        for kb, pb in fams["roi_align_backward"].items():
            pf = fams["roi_align"][kb + (False, 1, False)]
            assert kb[:3] == (h3, w3, 256) and kb[4] == 7 and kb[3] > 64 and not kb[5], kb
            assert pf["n"] == pb["n"] and pb["n"] % 3 == 0 and len(pf["boxes"]) == len(pb["boxes"]) == 3
            assert all(torch.equal(a, b) for a, b in zip(pf["boxes"], pb["boxes"])) and not torch.equal(pb["boxes"][0], pb["boxes"][1])
            assert all(b.shape == (kb[3], 4) and bool(torch.isfinite(b).all()) for b in pb["boxes"])
        assert sum(p["n"] for p in fams["roi_align_backward"].values()) == 3 * B
        assert {k[:2] for k in fams["zs_logits"]} == {k[:2] for k in fams["zs_logits_backward"]} == {(k[3], 21) for k in fams["roi_align_backward"]}
        assert sum(p["n"] for p in fams["zs_logits"].values()) == sum(p["n"] for p in fams["zs_logits_backward"].values()) == 3 * B
    if "upsample2_sum_backward" in want:
        assert set(fams["upsample2_sum_backward"]) == {(B, h3 // 2, w3 // 2, 256, 1), (B, h3 // 4, w3 // 4, 256, 1)}
    if "maxpool3x3s2_backward" in want:
        assert list(fams["maxpool3x3s2_backward"]) == [(B, H // 2, W // 2, 64, H // 4, W // 4)]
        assert (B * (H // 2) * (W // 2) * 64,) in fams["relu_backward"], "the stem's ReLU"
    if fp16:
        (kn, pn), = fams["nonfinite"].items()
        assert pn["n"] == 1 and len(kn) > 100 and all(n > 0 for n in kn)


# ------------------------------------------------------------------------------------------------
# 2. ROIAlign
# ------------------------------------------------------------------------------------------------
def _roi_bound(T: torch.Tensor, reach: torch.Tensor, extent: int) -> torch.Tensor:
    """First-order bound on the fp32 error of one ROIAlign sum, element-wise.  A sample coordinate is built from a few fp32 roundings
    at the magnitude of the level's extent E (ulp/2 <= U * 2^ceil(log2 E)), so every tap weight is off by at most ~4 of those, an
    axis weight (g samples) by 4 g, and the product of two axis weights over the g^2 samples by 8 x that rounding: 8 U 2^ceil(log2 E)
    times the sum T of the magnitudes the touched cells / bins hold.  Adding n terms adds at most n U T.  `reach` = n."""
    return ROI_HEAD * U * (8.0 * 2.0 ** math.ceil(math.log2(extent)) + reach) * T


def _guarded(shapes, C: int, dev, pattern: Optional[List[torch.Tensor]] = None):
    """One buffer per level with a guard row of SENTINEL behind it -> (buffers, the [h, w, C] views the kernel is given)."""
    bufs = []
    for l, (h, w) in enumerate(shapes):
        b = torch.full((h * w + 1, C), SENTINEL, dtype=torch.float32, device=dev)
        b[:h * w] = 0.0 if pattern is None else pattern[l].reshape(h * w, C).to(dev)
        bufs.append(b)
    return bufs, [b[:h * w].view(h, w, C) for b, (h, w) in zip(bufs, shapes)]


def _roi_backward_check(tag: str, dev, shapes, C: int, lists: List[torch.Tensor], S: int, seed: int, count: Optional[int] = None,
                        yardstick: bool = True) -> List[str]:
    """The box lists one after the other into ONE gradient buffer pre-filled with a non-zero pattern (the step adds its three stages
    into one buffer), against float64: element-wise within the bound, the non-zero cell set, the guard rows."""
    from embodied_object_detection_amd import ops
    bad = []
    g = torch.Generator().manual_seed(seed)
    pattern = [(torch.randn((h, w, C), generator=g) * 0.25 + 0.5) for h, w in shapes]
    bufs, views = _guarded(shapes, C, dev, pattern)
    ref = [p.double().clone() for p in pattern]
    r32 = [p.clone() for p in pattern]
    bound = [U * ROI_HEAD * p.double().abs() for p in pattern]               # per call one rounding of the sum into the buffer
    touched = [torch.zeros((h, w), dtype=torch.bool) for h, w in shapes]
    for k, boxes in enumerate(lists):
        R_cap = boxes.shape[0]
        R = R_cap if count is None else count
        G = torch.randn((R_cap, S, S, C), generator=g)
        cnt = None if count is None else torch.tensor([count], dtype=torch.int32, device=dev)
        ops.roi_align_backward(views[0], views[1], views[2], shapes[0][0], shapes[0][1], C, boxes.to(dev), cnt, R_cap, S, G.to(dev))
        rr = RoiRef(boxes[:R], S, shapes, torch.float64)
        d, T, n = rr.adjoint(G[:R]), rr.adjoint(G[:R].abs(), indicator=True), rr.reach()
        rr32 = RoiRef(boxes[:R], S, shapes, torch.float32)
        n32 = rr32.reach()              # a tap weight can be exactly 0 at one precision and not at the other: reached = in either
        if yardstick:
            d32 = rr32.adjoint(G[:R])
        for l, (h, w) in enumerate(shapes):
            ref[l] += d[l]
            r32[l] = r32[l] + (d32[l] if yardstick else d[l].float())
            bound[l] = bound[l] + _roi_bound(T[l], n[l][:, :, None], max(h, w)) + U * ROI_HEAD * ref[l].abs()
            touched[l] |= (n[l] > 0) | (n32[l] > 0)
    torch.cuda.synchronize()
    for l, (h, w) in enumerate(shapes):
        got = views[l].cpu()
        err = (got.double() - ref[l]).abs()
        e32 = (r32[l].double() - ref[l]).abs()
        ratio = err / bound[l]
        _line(tag, f"dP{l + 3}", *_worst(err, e32, bound[l]),
              f"largest error {float(err.max()):.2e}, cells reached {int(touched[l].sum())} of {h * w}, cpu fp32 at {float((e32 / bound[l]).max()):.3f} of its bound")
        if not bool((err <= bound[l]).all()):
            i = int(ratio.argmax())
            bad.append(f"{tag}: dP{l + 3} is {float(err.reshape(-1)[i]):.3e} from float64 at flat index {i}, bound {float(bound[l].reshape(-1)[i]):.3e} "
                       f"({int((err > bound[l]).sum())} elements above their bound)")
        # coverage: what the reference moves by more than the bound has moved here, what no ROI reaches keeps the pattern bit for bit
        moved = (ref[l] - pattern[l].double()).abs() > bound[l]
        if bool((moved & (got == pattern[l])).any()):
            bad.append(f"{tag}: {int((moved & (got == pattern[l])).sum())} elements of dP{l + 3} the reference moves were left untouched")
        quiet = ~touched[l]
        if not torch.equal(got[quiet], pattern[l][quiet]):
            bad.append(f"{tag}: {int((got[quiet] != pattern[l][quiet]).any(-1).sum())} cells of dP{l + 3} no ROI reaches were written")
        if not bool((bufs[l][h * w:] == SENTINEL).all()):
            bad.append(f"{tag}: the guard row behind dP{l + 3} was written")
    return bad


def _roi_forward_check(tag: str, dev, shapes, C: int, boxes: torch.Tensor, S: int, seed: int, count: Optional[int] = None) -> List[str]:
    from embodied_object_detection_amd import ops
    bad = []
    g = torch.Generator().manual_seed(seed)
    feats = [torch.randn((h, w, C), generator=g) + 0.5 for h, w in shapes]
    R_cap = boxes.shape[0]
    R = R_cap if count is None else count
    out = torch.full((R_cap + 1, S, S, C), SENTINEL, dtype=torch.float32, device=dev)
    cnt = None if count is None else torch.tensor([count], dtype=torch.int32, device=dev)
    fd = [f.to(dev) for f in feats]
    ops.roi_align(fd[0], fd[1], fd[2], shapes[0][0], shapes[0][1], C, boxes.to(dev), cnt, R_cap, S, out=out[:R_cap])
    torch.cuda.synchronize()
    rr, ref, bound = roi_forward_reference(boxes[:R], S, shapes, feats)      # ROI_HEAD * U * (8 extent + cells a bin touches) * T
    y32 = RoiRef(boxes[:R], S, shapes, torch.float32).forward(feats)
    got = out[:R].cpu()
    err, e32 = (got.double() - ref).abs(), (y32.double() - ref).abs()
    ratio = err / bound.clamp(min=1e-300)
    _line(tag, "pooled", *_worst(err, e32, bound),
          f"largest error {float(err.max()):.2e}, {R} of {R_cap} rows, {sum(1 for x in rr.rois if x is None)} empty, cpu fp32 at {float((e32 / bound.clamp(min=1e-300)).max()):.3f} of its bound")
    if not bool((err <= bound).all()):
        i = int(ratio.argmax())
        bad.append(f"{tag}: pooled value {float(err.reshape(-1)[i]):.3e} from float64 at flat index {i} (ROI {i // (S * S * C)}), bound "
                   f"{float(bound.reshape(-1)[i]):.3e} ({int((err > bound).sum())} elements above their bound)")
    if not bool((out[R:] == SENTINEL).all()):
        bad.append(f"{tag}: rows beyond the count ({R} of {R_cap}) or the guard row were written")
    return bad


def test_roi_reference_is_the_oracles_roi_align():
    """The reference used below (axis matrices at a chosen precision) against autograd through oracle/ops.py's ROIAlignV2 in fp32,
    forward and gradient, on the hostile list (without the boxes inverted along one axis: they have no level in the oracle)."""
    from oracle import ops as OO
    H, W, C, S = 480, 640, 8, 7
    shapes = [(H >> (3 + l), W >> (3 + l)) for l in range(3)]
    boxes = hostile_boxes(H, W, 80, 3)
    boxes = boxes[((boxes[:, 2] - boxes[:, 0]) * (boxes[:, 3] - boxes[:, 1])) >= 0].contiguous()
    assert set(OO.assign_boxes_to_levels(boxes).tolist()) == {0, 1, 2}
    g = torch.Generator().manual_seed(1)
    feats = [torch.randn((1, C, h, w), generator=g).requires_grad_() for h, w in shapes]
    G = torch.randn((boxes.shape[0], C, S, S), generator=g)
    out = OO.roi_pool(feats, boxes, S)
    (out * G).sum().backward()
    rr = RoiRef(boxes, S, shapes, torch.float32)
    f = rr.forward([x[0].permute(1, 2, 0).detach() for x in feats])
    assert float((f.permute(0, 3, 1, 2) - out.detach()).abs().max()) <= 4e-6
    d = rr.adjoint(G.permute(0, 2, 3, 1))
    for l in range(3):
        r = feats[l].grad[0].permute(1, 2, 0)
        assert float((d[l] - r).abs().max()) <= 4e-6 * float(r.abs().max()), l
        assert bool((rr.reach()[l] > 0)[r.abs().sum(-1) > 0].all()), "every cell the oracle's gradient reaches is a reached cell here"


def _roi_cases(recorded) -> List[Tuple[str, tuple, List[torch.Tensor]]]:
    out = []
    for key, (config, payload) in _union(recorded, "roi_align_backward").items():
        out.append((config, key, payload["boxes"]))
    return out


def test_roi_align_backward_gather_form_on_the_recorded_stages(dev, recorded):
    """The shipped gather form at every recorded (pyramid, R): the three stages' real boxes, C = 256, S = 7, into one buffer."""
    cases = _roi_cases(recorded)
    assert {k[:2] for _, k, _ in cases} >= {(80, 80), (60, 80), (120, 120)}, [k for _, k, _ in cases]
    bad = []
    for i, (config, (h3, w3, C, R_cap, S, has_count), lists) in enumerate(cases):
        assert C == 256 and S == 7 and R_cap > 64 and not has_count
        shapes = [(h3, w3), (h3 // 2, w3 // 2), (h3 // 4, w3 // 4)]
        lv = [roi_geometry(b, S)[0].bincount(minlength=3).tolist() for b in lists]
        print(f"\n{config}: R {R_cap}, boxes per level of the stages {lv}")
        bad += _roi_backward_check(f"{config} R {R_cap}", dev, shapes, C, lists, S, 100 + i)
    assert not bad, f"{len(bad)} findings:\n" + "\n".join(bad)


@pytest.mark.parametrize("rows,count", [(65, None), (128, None), (129, None), (536, None), (192, 129)])
def test_roi_align_backward_gather_form_on_hostile_boxes(dev, rows, count):
    """A list built to hurt the footprint filter (see `hostile_boxes`), 65 / 128 / 129 rows so that the passes of 64 boxes end on
    and off a boundary, and a count below R_cap with whole-image boxes behind it that must not be read."""
    H, W = 480, 640
    shapes = [(H >> (3 + l), W >> (3 + l)) for l in range(3)]
    boxes = hostile_boxes(H, W, rows, 7 + rows)
    if count is not None:
        boxes[count:] = torch.tensor([0.0, 0.0, W, H])
    lists = [boxes, boxes.flip(0).contiguous()] if count is None else [boxes]
    bad = _roi_backward_check(f"hostile {rows} rows" + (f" count {count}" if count else ""), dev, shapes, 256, lists, 7, 300 + rows, count=count)
    assert not bad, "\n".join(bad)


def test_roi_align_forward_on_the_recorded_and_hostile_lists(dev, recorded):
    bad = []
    for i, (key, (config, payload)) in enumerate(_union(recorded, "roi_align").items()):
        h3, w3, C, R_cap, S = key[:5]
        assert key[5:] == (False, False, 1, False), key
        shapes = [(h3, w3), (h3 // 2, w3 // 2), (h3 // 4, w3 // 4)]
        for k, boxes in enumerate(payload["boxes"]):
            bad += _roi_forward_check(f"{config} R {R_cap} stage {k}", dev, shapes, C, boxes, S, 400 + 10 * i + k)
    shapes = [(60, 80), (30, 40), (15, 20)]
    bad += _roi_forward_check("hostile 129 rows", dev, shapes, 256, hostile_boxes(480, 640, 129, 136), 7, 470)
    bad += _roi_forward_check("hostile 192 rows count 129", dev, shapes, 256, hostile_boxes(480, 640, 192, 199), 7, 471, count=129)
    assert not bad, f"{len(bad)} findings:\n" + "\n".join(bad)


# ---- the two other backward forms --------------------------------------------------------------
def _atomic_form_ran(dev, shapes, C: int, boxes: torch.Tensor, S: int) -> bool:
    """Which backward form the library runs, seen from outside: with an all-zero dY on a buffer of -0.0 the gather form writes
    nothing (a cell whose sum is zero is skipped), the forms with atomics add +0.0 to every cell they reach and clear its sign."""
    from embodied_object_detection_amd import ops
    d = [torch.full((h, w, C), -0.0, dtype=torch.float32, device=dev) for h, w in shapes]
    ops.roi_align_backward(d[0], d[1], d[2], shapes[0][0], shapes[0][1], C, boxes.to(dev), None, boxes.shape[0], S,
                           torch.zeros((boxes.shape[0], S, S, C), device=dev))
    torch.cuda.synchronize()
    assert all(float(t.abs().max()) == 0.0 for t in d)
    return any(bool((~torch.signbit(t)).any()) for t in d)


def _fallback_cases():
    """(tag, shapes, C, box lists, count): a production-sized hostile list, the 64-box boundary with a count, and a small pyramid."""
    s640 = [(80, 80), (40, 40), (20, 20)]
    s480 = [(60, 80), (30, 40), (15, 20)]
    b = hostile_boxes(480, 640, 192, 21)
    b[129:] = torch.tensor([0.0, 0.0, 640.0, 480.0])
    return [("640x640 R 536", s640, 256, [hostile_boxes(640, 640, 536, 20)], None), ("480x640 R 192 count 129", s480, 256, [b], 129),
            ("480x640 R 65 twice", s480, 256, [hostile_boxes(480, 640, 65, 22)] * 2, None)]


def _fallback_child() -> int:
    """What a child process runs: the cases above under the EOD_ROI_BWD_* setting it was started with."""
    from embodied_object_detection_amd import _lib
    _lib.load()
    dev = torch.device("cuda:0")
    form = "rows" if os.environ.get("EOD_ROI_BWD_ROWS") else "samples" if os.environ.get("EOD_ROI_BWD_SAMPLES") else "gather"
    bad = []
    if not _atomic_form_ran(dev, [(60, 80), (30, 40), (15, 20)], 256, hostile_boxes(480, 640, 65, 22), 7):
        bad.append(f"[{form}] the gather form ran: the setting was not read")
    for i, (tag, shapes, C, lists, count) in enumerate(_fallback_cases()):
        bad += _roi_backward_check(f"[{form}] {tag}", dev, shapes, C, lists, 7, 500 + i, count=count, yardstick=False)
    for b in bad:
        print("FINDING", b)
    return 1 if bad else 0


def test_roi_align_backward_fallback_forms_in_child_processes(dev):
    """`EOD_ROI_BWD_ROWS=1` (footprint rows with atomics) and `EOD_ROI_BWD_SAMPLES=1` (one atomic per sample tap), read once at load:
    one fresh child per setting, one at a time, stopping at the first that fails.  This process runs the gather form."""
    assert not _atomic_form_ran(dev, [(60, 80), (30, 40), (15, 20)], 256, hostile_boxes(480, 640, 65, 22), 7)
    for env in ({"EOD_ROI_BWD_ROWS": "1"}, {"EOD_ROI_BWD_SAMPLES": "1"}):
        p = subprocess.run([sys.executable, os.path.abspath(__file__)], env={**os.environ, **env}, cwd=ROOT, timeout=240,
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        print(p.stdout)
        assert p.returncode == 0, f"child with {env} ended with status {p.returncode}:\n{p.stdout[-4000:]}"


def test_roi_align_backward_rows_form_takes_wide_channels(dev):
    """C = 320 (above the gather form's 256: lane x 4 channels in one pass) reaches the rows form without any variable: its
    second channel pass (`cb` = 256) holds 64 live channels."""
    shapes = [(60, 80), (30, 40), (15, 20)]
    boxes = hostile_boxes(480, 640, 129, 31)
    assert _atomic_form_ran(dev, shapes, 320, boxes, 7)
    bad = _roi_backward_check("C 320 rows form", dev, shapes, 320, [boxes, boxes.flip(0).contiguous()], 7, 600)
    assert not bad, "\n".join(bad)


# ------------------------------------------------------------------------------------------------
# 3. GroupNorm + ReLU, forward and backward, statistics produced both ways
# ------------------------------------------------------------------------------------------------
def _gn_reference(c: torch.Tensor, gamma, beta, off, dy, mask, dtype):
    """F.group_norm per level + the ReLU whose derivative is `mask` (the device's own y > 0: the reference differentiates the
    function the device evaluated; the flips are counted by the caller) -> (pre-activation, dx, dgamma, dbeta)."""
    x = c.detach().to(dtype).clone().requires_grad_()
    gm, bt = gamma.detach().to(dtype).clone().requires_grad_(), beta.detach().to(dtype).clone().requires_grad_()
    pre = []
    for l in range(len(off) - 1):
        xl = x[off[l]:off[l + 1]].t().reshape(1, x.shape[1], -1)
        pre.append(F.group_norm(xl, 32, gm, bt, eps=1e-5)[0].t())
    pre = torch.cat(pre)
    (pre * mask.to(dtype) * dy.to(dtype)).sum().backward()
    return pre.detach(), x.grad, gm.grad, bt.grad


def test_groupnorm_forward_and_backward_at_the_recorded_pyramids(dev, recorded):
    """The tower's GroupNorm(32) + ReLU on the five-level pyramids of 640x640, 480x640 and 960x960.  The input is the output of a
    tower convolution with a bias of four times its spread.  The partial sums come (a) from `groupnorm_relu`'s own statistics launch,
    as the training step runs it, and (b) from the convolution's slab reduce (`gn_stats=`, the inference frames' producer); the
    backward, which recomputes mean and rstd from those sums, is fed from each."""
    from embodied_object_detection_amd import ops
    cases = _union(recorded, "groupnorm_relu_backward")
    assert {k[0][-1] for k in cases} == {8525, 6400, 19189}, list(cases)
    assert {k[0] for k in cases} == {k[0] for k in _union(recorded, "groupnorm_relu")}
    bad = []
    for i, (key, (config, _)) in enumerate(cases.items()):
        off, Cc, groups, eps = list(key[0]), key[1], key[2], key[3]
        H, W = CONFIGS[config][:2]
        shapes = [(-(-H // (8 << l)), -(-W // (8 << l))) for l in range(5)]
        assert [h * w for h, w in shapes] == [off[l + 1] - off[l] for l in range(5)] and Cc == 256 and groups == 32
        g = torch.Generator().manual_seed(700 + i)
        x = torch.randn((off[-1], Cc), generator=g).abs()                      # a post-ReLU activation
        w = torch.randn((Cc, Cc, 3, 3), generator=g) * 0.02
        b = 4.0 + 0.3 * torch.randn((Cc,), generator=g)
        gamma, beta = torch.rand(Cc, generator=g) + 0.5, torch.randn(Cc, generator=g) * 0.3
        dy = torch.randn((off[-1], Cc), generator=g)
        conv = ops.Conv(w, b, pad=1, device=dev, name="tower")
        gd, bd, dyd = gamma.to(dev), beta.to(dev), dy.to(dev)
        ways = {}
        st_own = ops.groupnorm_workspace(off, dev)
        c_own = conv(x.to(dev), 1, 0, 0, levels=(off, shapes))
        assert not conv.gn_fused
        ways["own statistics"] = (c_own, st_own, False)
        st_fused = ops.groupnorm_workspace(off, dev)
        st_fused.fill_(float("nan"))                                           # whatever the fused producer does not write shows
        c_fused = conv(x.to(dev), 1, 0, 0, levels=(off, shapes), gn_stats=st_fused)
        fused = bool(conv.gn_fused)
        print(f"\n{config}: rows {off[-1]}, conv.gn_fused {fused}")
        # 640x640 is the size whose tower plan reduces split-K slabs; the 19 189 rows of 960x960 fill the device without split-K, so no
        # fused producer exists there (printed above)
        if (H, W) == (640, 640):
            assert fused, f"{config}: the tower convolution's plan does not reduce slabs any more: the fused statistics are not tested"
        if fused:
            assert torch.equal(c_fused, c_own)
            ways["fused statistics"] = (c_fused, st_fused, True)
        for way, (c, st, ready) in ways.items():
            tag = f"{config} {way}"
            y = torch.full((off[-1] + 1, Cc), SENTINEL, dtype=torch.float32, device=dev)
            ops.groupnorm_relu(c, gd, bd, off, Cc, st, groups=groups, eps=eps, out=y[:off[-1]], partial_ready=ready)
            dx, dgamma, dbeta = ops.groupnorm_relu_backward(c, y[:off[-1]], dyd, gd, off, Cc, st, groups=groups, eps=eps)
            torch.cuda.synchronize()
            ch, yh = c.cpu(), y[:off[-1]].cpu()
            mask = yh > 0
            pre, rdx, rdg, rdb = _gn_reference(ch, gamma, beta, off, dy, mask, torch.float64)
            p32, xdx, xdg, xdb = _gn_reference(ch, gamma, beta, off, dy, mask, torch.float32)
            # how far the input's mean is from zero in units of its spread: x - mean cancels that many leading digits
            amp = 1.0 + float(ch.double().mean().abs() / ch.double().std())
            assert amp > 3.0, amp
            # forward, element-wise: six roundings (mean and rstd to fp32, the subtraction, two products, the sum), each on a
            # quantity no larger than |gamma| rstd (|x| + |mean|) + |beta|; rstd (|x| + |mean|) <= |xhat| + 2 amp (head-room 2)
            xhat_mag = ((pre - beta.double()) / gamma.double()).abs()
            fb = 2.0 * 6.0 * U * (gamma.double().abs() * (xhat_mag + 2.0 * amp) + beta.double().abs())
            ferr = (yh.double() - pre.clamp(min=0)).abs()
            _line(tag, "y", *_worst(ferr, (p32.clamp(min=0).double() - pre.clamp(min=0)).abs(), fb))
            if not bool((ferr <= fb).all()):
                bad.append(f"{tag}: y is {float(ferr.max()):.3e} from float64, {int((ferr > fb).sum())} elements above their bound")
            # ReLU flips: y > 0 on one side only.  They are discrete and sit at rounding distance from zero -- each is checked for
            # that, none is absorbed into a bound (the backward reference above uses the device's mask)
            flips = mask != (pre > 0)
            print(f"{tag:44s} {int(flips.sum())} ReLU flips of {flips.numel()}, largest |pre-activation| among them "
                  f"{float(pre[flips].abs().max()) if bool(flips.any()) else 0.0:.2e}")
            if not bool((pre[flips].abs() <= fb[flips]).all()) or int(flips.sum()) > flips.numel() // 10000:
                bad.append(f"{tag}: {int(flips.sum())} ReLU flips, not all within the forward bound of zero")
            if not bool((y[off[-1]:] == SENTINEL).all()):
                bad.append(f"{tag}: the guard row behind y was written")
            # backward: errors over the rms of the tensor against the CPU fp32 autograd of the same function, with a floor of
            # 4 U amp (mean) / 32 U amp (max): one rounding of x - mean is U amp of xhat, and dx holds a handful of them
            for what, got, ref, c32 in (("dx", dx, rdx, xdx), ("dgamma", dgamma, rdg, xdg), ("dbeta", dbeta, rdb, xdb)):
                e, e32 = _rms_errors(got.cpu(), ref), _rms_errors(c32, ref)
                lim = (max(MEAN_X * e32[0], 4 * U * amp), max(MAX_X * e32[1], 32 * U * amp))
                _line(tag, what + " mean", e[0], e32[0], lim[0])
                _line(tag, what + " max", e[1], e32[1], lim[1])
                if not (e[0] <= lim[0] and e[1] <= lim[1]):
                    bad.append(f"{tag}: {what} err/rms mean {e[0]:.3e} max {e[1]:.3e} above {lim[0]:.3e} / {lim[1]:.3e} "
                               f"(the CPU fp32 result's: {e32[0]:.3e} / {e32[1]:.3e})")
    assert not bad, f"{len(bad)} findings:\n" + "\n".join(bad)


# ------------------------------------------------------------------------------------------------
# 4. the memory read's backward
# ------------------------------------------------------------------------------------------------
def _proj_ranges() -> int:
    from embodied_object_detection_amd import _lib
    nb = _lib.load().eod_memory_project_backward_weights_workspace_bytes()
    per = 3 * (256 * 512 + 256) * 4
    assert nb % per == 0, nb
    return nb // per


def _wgrad_compare(tag: str, what: str, got, ref, c32, chain: int) -> List[str]:
    """dW / db rule of the convolution module: the larger of a multiple of the CPU fp32 error and the rounding model of one fp32
    accumulator adding `chain` positions in sequence."""
    e, e32 = _rms_errors(got, ref), _rms_errors(c32, ref)
    model = U * math.sqrt(chain)
    lim = (max(MEAN_X * e32[0], CHAIN_MEAN * model), max(MAX_X * e32[1], CHAIN_MAX * model))
    _line(tag, what + " mean", e[0], e32[0], lim[0], f"chain {chain}")
    _line(tag, what + " max", e[1], e32[1], lim[1])
    if not (math.isfinite(e[1]) and e[0] <= lim[0] and e[1] <= lim[1]):
        return [f"{tag}: {what} err/rms mean {e[0]:.3e} max {e[1]:.3e} above {lim[0]:.3e} / {lim[1]:.3e} (cpu fp32 {e32[0]:.3e} / {e32[1]:.3e})"]
    return []


@pytest.mark.parametrize("H,W", [(640, 640), (480, 640), (960, 960)])
def test_memory_projection_backward_at_production_sizes(dev, recorded, H, W):
    """`MemoryProjectorBackward` as the step calls it (need_input_grad=False: dW / db only) and with the input gradients, the pooled
    operand from `ops.memory_gather_pool` with the recorded flags (fragment order; 480x640's level 5 has 300 rows, tile-padded).
    dW / db against a float64 GEMM on the half-rounded pooled values the device itself produced; gE / gE2 by the half-ulp rule of
    test_memory_read_backward_matches_autograd; the entry point without a workspace (one range) against the same reference."""
    import ctypes as C
    from embodied_object_detection_amd import _lib, ops
    lib = _lib.load()
    assert (H, W, 5.0, False) in _union(recorded, "memory_projector_backward")
    pool_keys = [k for k in _union(recorded, "memory_gather_pool") if k[:2] == (H, W)]
    assert pool_keys and all(k[4] for k in pool_keys), pool_keys          # torch_order as the step passes it
    weight, n_cells = 5.0, 4000
    g = torch.Generator().manual_seed(H + W)
    mem16 = (torch.randn((n_cells, 512), generator=g) * 2).half()
    # 4-pixel blocks: E_2 (the 4 x 4 mean) is a table row exactly, so the autograd leaf below is known without a 900 MB gather
    proj4 = torch.randint(0, n_cells, (H // 4, W // 4), generator=g)
    proj = proj4.repeat_interleave(4, 0).repeat_interleave(4, 1).contiguous()
    Ws = [(torch.randn((256, 512, 1, 1), generator=g) * 0.05).requires_grad_() for _ in range(3)]
    bs = [(torch.randn((256,), generator=g) * 0.1).requires_grad_() for _ in range(3)]
    rows = [(H >> (3 + l)) * (W >> (3 + l)) for l in range(3)]
    G = [torch.randn((rows[l], 256), generator=g) for l in range(3)]
    e2 = mem16[proj4].permute(2, 0, 1).unsqueeze(0).float().requires_grad_()
    pooled, cur = [], e2
    for _ in range(3):
        cur = F.avg_pool2d(cur.to(torch.float32), kernel_size=2, stride=2).to(torch.half)
        cur.retain_grad()
        pooled.append(cur)
    loss = 0.0
    for l in range(3):
        Gl = G[l].t().reshape(1, 256, H >> (3 + l), W >> (3 + l))
        loss = loss + (F.conv2d(pooled[l].to(torch.float32), Ws[l], bs[l]) * weight * Gl).sum()
    loss.backward()
    pooled_d = ops.memory_gather_pool(mem16.to(dev), proj.int().to(dev), H, W, torch_order=True)
    got_rows = fragments_to_rows(pooled_d.cpu(), H, W)
    want_rows = [p.detach()[0].permute(1, 2, 0).reshape(-1, 512) for p in pooled]
    assert all(torch.equal(a, b) for a, b in zip(got_rows, want_rows)), "the device's pooled operand is the oracle's cascade"
    bwd = ops.MemoryProjectorBackward([w.detach() for w in Ws], dev)
    grads = [t.contiguous().to(dev) for t in G]
    splits = _proj_ranges()
    assert splits == 8
    bad = []
    ref = [(weight * G[l].double().t() @ want_rows[l].double(), weight * G[l].double().sum(0)) for l in range(3)]
    c32 = [(weight * (G[l].t() @ want_rows[l].float()), weight * G[l].sum(0)) for l in range(3)]
    out_f = bwd(grads, pooled_d, H, W, weight, need_input_grad=False)
    assert set(out_f) == {"dW", "db"}
    out_t = bwd(grads, pooled_d, H, W, weight, need_input_grad=True)
    # without a workspace: one range over all positions, into NaN-filled buffers with a guard row
    dW1 = [torch.full((257, 512), float("nan"), device=dev) for _ in range(3)]
    db1 = [torch.full((256 + 32,), float("nan"), device=dev) for _ in range(3)]
    for t in dW1:
        t[256:] = SENTINEL
    for t in db1:
        t[256:] = SENTINEL
    _lib.check(lib.eod_memory_project_backward_weights(grads[0].data_ptr(), grads[1].data_ptr(), grads[2].data_ptr(), pooled_d.data_ptr(), H, W,
                                                       C.c_float(weight), dW1[0].data_ptr(), db1[0].data_ptr(), dW1[1].data_ptr(), db1[1].data_ptr(),
                                                       dW1[2].data_ptr(), db1[2].data_ptr(), ops._stream()), "eod_memory_project_backward_weights")
    torch.cuda.synchronize()
    for l in range(3):
        steps = -(-rows[l] // 8)
        sps = -(-steps // splits)
        full = sum(1 for z in range(splits) if z * sps < steps)
        print(f"\n{H}x{W} level {l + 3}: {rows[l]} positions = {steps} k-steps, {sps} per range, {full} of {splits} ranges hold positions")
        chain = 8 * -(-sps // 4) + 4 + splits           # a wave's positions in sequence, then the 4 waves and the ranges one by one
        tag = f"{H}x{W} P{l + 3}"
        bad += _wgrad_compare(tag + " dW only", "dW", out_f["dW"][l].cpu(), ref[l][0], c32[l][0], chain)
        bad += _wgrad_compare(tag + " dW only", "db", out_f["db"][l].cpu(), ref[l][1], c32[l][1], chain)
        if not (torch.equal(out_f["dW"][l], out_t["dW"][l]) and torch.equal(out_f["db"][l], out_t["db"][l])):
            bad.append(f"{tag}: dW / db differ between need_input_grad False and True")
        bad += _wgrad_compare(tag + " one range", "dW", dW1[l][:256].cpu(), ref[l][0], c32[l][0], 8 * -(-steps // 4) + 4)
        bad += _wgrad_compare(tag + " one range", "db", db1[l][:256].cpu(), ref[l][1], c32[l][1], 8 * -(-steps // 4) + 4)
        if not (bool((dW1[l][256:] == SENTINEL).all()) and bool((db1[l][256:] == SENTINEL).all())):
            bad.append(f"{tag}: the guard rows behind dW / db were written")
        # the autograd cross-check of the float64 GEMM (fp32, as the existing small-size test compares)
        assert float((Ws[l].grad.reshape(256, 512).double() - ref[l][0]).abs().max()) <= 1e-4 * float(ref[l][0].abs().max())
        ref_g = pooled[l].grad[0].permute(1, 2, 0).reshape(-1, 512).float()
        got_g = out_t["gE"][l].cpu().float()
        tol = 2.0 ** -10 * float(ref_g.abs().max())
        same = float((got_g == ref_g).float().mean())
        _line(tag, "gE", float((got_g - ref_g).abs().max()), 0.0, tol, f"{same:.4f} bit-identical halves")
        if not (bool(((got_g - ref_g).abs() <= tol).all()) and same > 0.99):
            bad.append(f"{tag}: gE {float((got_g - ref_g).abs().max()):.3e} > {tol:.3e} or only {same:.4f} bit-identical")
    ref_g2 = e2.grad[0].permute(1, 2, 0).reshape(-1, 512)
    got_g2 = out_t["gE2"].cpu()
    tol = 2.0 ** -10 * float(ref_g2.abs().max())
    same = float((got_g2 == ref_g2).float().mean())
    _line(f"{H}x{W}", "gE2", float((got_g2 - ref_g2).abs().max()), 0.0, tol, f"{same:.4f} bit-identical")
    if not (bool(((got_g2 - ref_g2).abs() <= tol).all()) and same > 0.99):
        bad.append(f"{H}x{W}: gE2 {float((got_g2 - ref_g2).abs().max()):.3e} > {tol:.3e} or only {same:.4f} bit-identical")
    assert not bad, f"{len(bad)} findings:\n" + "\n".join(bad)


# ------------------------------------------------------------------------------------------------
# 5. the trunk's three small backward kernels
# ------------------------------------------------------------------------------------------------
def test_trunk_kernels_at_the_recorded_sizes(dev, recorded):
    """Up-sample-add, max pool and ReLU backward at every recorded (N, H, W, C), N = 4 included: 26 M elements through grids capped
    at 8192 workgroups.  ReLU backward and the max pool's single-window inputs bitwise; where several gradients add up (the 2 x 2
    block sums of the up-sample, inputs that are the maximum of several windows) float64 and one rounding per addend."""
    import ctypes as C    # noqa: F401
    from embodied_object_detection_amd import _lib, ops
    lib = _lib.load()
    s = ops._stream()
    bad = []
    ups, mps, relus = _union(recorded, "upsample2_sum_backward"), _union(recorded, "maxpool3x3s2_backward"), _union(recorded, "relu_backward")
    assert any(k[0] == 4 for k in ups) and any(k[0] == 4 for k in mps) and {(k[1], k[2]) for k in mps} >= {(320, 320), (240, 320), (480, 480)}
    for i, ((N, h, w, Cc, acc), (config, _)) in enumerate(ups.items()):
        g = torch.Generator().manual_seed(800 + i)
        fine = torch.randn((N, 2 * h, 2 * w, Cc), generator=g)
        base = torch.randn((N, h, w, Cc), generator=g)
        out = torch.full((N * h * w + 1, Cc), SENTINEL, device=dev)
        out[:N * h * w] = base.reshape(-1, Cc).to(dev)
        fd = fine.to(dev)
        _lib.check(lib.eod_upsample2_sum_backward(fd.data_ptr(), out.data_ptr(), N, h, w, Cc, acc, s), "up")
        torch.cuda.synchronize()
        blocks = fine.double().view(N, h, 2, w, 2, Cc)
        ref = blocks.sum(dim=(2, 4)) + (base.double() if acc else 0.0)
        mag = blocks.abs().sum(dim=(2, 4)) + (base.double().abs() if acc else 0.0)
        c32 = fine.view(N, h, 2, w, 2, Cc).sum(dim=(2, 4)) + (base if acc else 0.0)
        err = (out[:N * h * w].cpu().view(N, h, w, Cc).double() - ref).abs()
        bound = (4 + acc) * U * mag
        _line(f"upsample {N}x{h}x{w}x{Cc} acc {acc}", "out", *_worst(err, (c32.double() - ref).abs(), bound))
        if not bool((err <= bound).all()) or not bool((out[N * h * w:] == SENTINEL).all()):
            bad.append(f"upsample {(N, h, w, Cc, acc)}: {int((err > bound).sum())} elements above one rounding per addend, or the guard row written")
    for i, ((N, H, W, Cc, OH, OW), (config, _)) in enumerate(mps.items()):
        g = torch.Generator().manual_seed(820 + i)
        x = (torch.randn((N, Cc, H, W), generator=g) * 2).round().abs()           # a quantised post-ReLU map: every window has ties
        x64 = x.double().requires_grad_()
        y = F.max_pool2d(x64, 3, 2, 1)
        assert tuple(y.shape[2:]) == (OH, OW)
        go = torch.randn(y.shape, generator=g)
        (y * go.double()).sum().backward()
        ref = x64.grad.permute(0, 2, 3, 1)
        x1 = x.double().requires_grad_()
        (F.max_pool2d(x1, 3, 2, 1) * go.double().abs()).sum().backward()
        mag = x1.grad.permute(0, 2, 3, 1)
        x2 = x.double().requires_grad_()
        F.max_pool2d(x2, 3, 2, 1).sum().backward()
        cnt = x2.grad.permute(0, 2, 3, 1)
        xd = x.permute(0, 2, 3, 1).contiguous().to(dev)
        yd = y.detach().float().permute(0, 2, 3, 1).contiguous().to(dev)
        gd = go.permute(0, 2, 3, 1).contiguous().to(dev)
        dx = torch.full((N * H * W + 1, Cc), SENTINEL, device=dev)
        _lib.check(lib.eod_maxpool3x3s2_backward(xd.data_ptr(), yd.data_ptr(), gd.data_ptr(), dx.data_ptr(), N, H, W, Cc, OH, OW, s), "mp")
        torch.cuda.synchronize()
        got = dx[:N * H * W].cpu().view(N, H, W, Cc)
        single = cnt <= 1
        exact = torch.equal(got[single], ref[single].float())
        err = (got.double() - ref).abs()
        bound = cnt * U * mag
        _line(f"maxpool {N}x{H}x{W}x{Cc}", "dx", float(err.max()), 0.0, float(bound.max()),
              f"{int((cnt > 1).sum())} inputs collect several windows (up to {int(cnt.max())}), the others bitwise: {exact}")
        if not exact or not bool((err <= bound).all()) or not bool((dx[N * H * W:] == SENTINEL).all()):
            bad.append(f"maxpool {(N, H, W, Cc)}: single-window inputs bitwise {exact}, {int((err > bound).sum())} sums above their bound, "
                       f"or the guard row written (a tie routed to another maximum shows as both)")
        del x64, x1, x2, y, ref, mag, cnt
    for i, ((n,), (config, _)) in enumerate(relus.items()):
        g = torch.Generator().manual_seed(840 + i)
        gr = torch.randn((n,), generator=g)
        y = torch.relu(torch.randn((n,), generator=g))
        y[::7] = 0.0
        y[3::11] = -0.0
        out = torch.full((n + 4,), SENTINEL, device=dev)
        grd, yd = gr.to(dev), y.to(dev)
        _lib.check(lib.eod_relu_backward(grd.data_ptr(), yd.data_ptr(), out.data_ptr(), n, s), "relu")
        torch.cuda.synchronize()
        ref = gr * (y > 0)
        exact = torch.equal(out[:n].cpu(), ref)
        print(f"relu backward n {n:9d} ({config}): bitwise {exact}")
        if not exact or not bool((out[n:] == SENTINEL).all()):
            bad.append(f"relu backward n {n}: {int((out[:n].cpu() != ref).sum())} elements differ, or the guard was written")
    assert not bad, f"{len(bad)} findings:\n" + "\n".join(bad)


# ------------------------------------------------------------------------------------------------
# 6. the training-mode classifier and its backward
# ------------------------------------------------------------------------------------------------
def _class_matrix(Cn: int) -> torch.Tensor:
    """[512, Cn + 1] as the classifier holds it: unit columns of the LVIS fixture, a zero background column."""
    rows = torch.tensor(np.load(LVIS), dtype=torch.float32)
    w = torch.cat([rows[:Cn].t().contiguous(), torch.zeros((512, 1))], dim=1)
    return F.normalize(w, p=2, dim=0).contiguous()


def test_zs_logits_and_backward_at_the_recorded_rows(dev, recorded):
    """temp * normalize(feat) @ zs at the recorded B (512 sampled rows + ground truth) and `ld`, for 21 columns (as recorded) and the
    LVIS fixture's 1204; d_logits is given with padded rows whose columns beyond C1 hold a sentinel that must not be read."""
    from embodied_object_detection_amd import ops
    fw, bw = _union(recorded, "zs_logits"), _union(recorded, "zs_logits_backward")
    assert fw and bw and all(k[1] == 21 for k in fw)
    bad = []
    for i, (B, C1r, ldr, temp) in enumerate(sorted({(k[0], k[1], k[2], k[3]) for k in fw} | {(k[0], k[1], k[2], k[3]) for k in bw})):
        for C1, ld in ((C1r, ldr), (1204, 1204 + (ldr - C1r)), (1204, 1216)):
            g = torch.Generator().manual_seed(900 + i)
            zs = _class_matrix(C1 - 1)
            feat = torch.randn((B, 512), generator=g) * torch.exp(torch.randn((B, 1), generator=g))       # norms over two decades
            dl = torch.randn((B, ld), generator=g) / C1
            dl[:, C1:] = SENTINEL
            featn = torch.full((B + 1, 512), SENTINEL, device=dev)
            logits = ops.zs_logits(feat.to(dev), zs.to(dev), temp, ld=ld, featn_out=featn[:B])
            d_feat = ops.zs_logits_backward(feat.to(dev), zs.to(dev), dl.to(dev), temp)
            torch.cuda.synchronize()
            tag = f"zs B {B} C1 {C1} ld {ld}"

            def ref_in(dtype):
                f = feat.to(dtype).requires_grad_()
                fn = temp * F.normalize(f, p=2, dim=1)
                lg = fn @ zs.to(dtype)
                (lg * dl[:, :C1].to(dtype)).sum().backward()
                return lg.detach(), fn.detach(), f.grad
            lg, fn, df = ref_in(torch.float64)
            lg32, fn32, df32 = ref_in(torch.float32)
            # logits: 512 products and sums (+ the normalisation's handful), each rounding on at most sum |featn| |zs|
            bnd = (512 + 16) * U * (fn.abs() @ zs.double().abs())
            err = (logits[:, :C1].cpu().double() - lg).abs()
            _line(tag, "logits", *_worst(err, (lg32.double() - lg).abs(), bnd))
            if not bool((err <= bnd).all()):
                bad.append(f"{tag}: logits {float(err.max()):.3e} from float64, {int((err > bnd).sum())} above their bound")
            if ld > C1 and not bool((logits[:, C1:] == 0).all()):
                bad.append(f"{tag}: the padding columns of the logits are not the zeros the wrapper allocated")
            ferr = (featn[:B].cpu().double() - fn).abs()
            fbnd = 2.0 * (512 + 16) / 2 * U * fn.abs()      # relative: the norm is a 512-term sum under a square root (head-room 2)
            _line(tag, "featn", *_worst(ferr, (fn32.double() - fn).abs(), fbnd))
            if not bool((ferr <= fbnd).all()) or not bool((featn[B:] == SENTINEL).all()):
                bad.append(f"{tag}: featn {float(ferr.max()):.3e} from float64 or its guard row written")
            # backward: d featn = temp-free product over C1 columns, then the normalisation's Jacobian (a 512-term dot product)
            A = dl[:, :C1].double().abs() @ zs.double().abs().t()
            unit = (fn / temp).abs()
            scale = temp / feat.double().norm(dim=1, keepdim=True)
            dbnd = 2.0 * (C1 + 512 + 16) * U * scale * (A + unit * (unit * A).sum(dim=1, keepdim=True))
            derr = (d_feat.cpu().double() - df).abs()
            _line(tag, "d_feat", *_worst(derr, (df32.double() - df).abs(), dbnd))
            if not (bool(torch.isfinite(d_feat).all()) and bool((derr <= dbnd).all())):
                bad.append(f"{tag}: d_feat {float(derr.max()):.3e} from float64, {int((derr > dbnd).sum())} above their bound (a read of the "
                           f"sentinel columns beyond C1 shows here)")
    assert not bad, f"{len(bad)} findings:\n" + "\n".join(bad)


# ------------------------------------------------------------------------------------------------
# 7. the loss scaler's found-inf pass
# ------------------------------------------------------------------------------------------------
def test_found_inf_pass_on_the_recorded_gradient_list(dev, recorded):
    """`AdamW.nonfinite` on tensors of the sizes the FP16 step hands it: the flag stays 0 on finite gradients (the largest finite
    values included); one inf or NaN in the first element of the first tensor, the last of the last, and the last of a tensor whose
    size is no multiple of the grid stride each set it.  Values are planted in a copy, the list itself is never changed."""
    from embodied_object_detection_amd import ops
    (sizes, _), = recorded["640x640 fp16"]["nonfinite"].items()
    gen = torch.Generator(device=dev).manual_seed(5)
    grads = [torch.randn((n,), generator=gen, device=dev) for n in sizes]
    grads[1][-1] = 3.4028234e38
    grads[2][0] = -3.4028234e38
    opt = ops.AdamW([{"name": "p", "param": torch.zeros((4,), device=dev), "lr": 1e-3}])
    odd = max((i for i, n in enumerate(sizes) if n % 1024 and n % 4), key=lambda i: sizes[i], default=None)
    if odd is None:
        odd = max((i for i, n in enumerate(sizes) if n % 1024), key=lambda i: sizes[i])
    print(f"\n{len(sizes)} tensors, {sum(sizes)} elements; the odd-sized one: #{odd} with {sizes[odd]} elements")

    def flag_of(lst) -> int:
        flag = torch.zeros((1,), dtype=torch.int32, device=dev)
        opt.nonfinite(lst, flag)
        return int(flag.cpu()[0])

    assert flag_of(grads) == 0, "finite gradients (with +-FLT_MAX among them) set the flag"
    assert flag_of([None, grads[0], None]) == 0
    for which, pos in ((0, 0), (len(sizes) - 1, -1), (odd, -1), (len(sizes) // 2, sizes[len(sizes) // 2] // 2)):
        for bad_value in (float("inf"), float("-inf"), float("nan")):
            lst = list(grads)
            lst[which] = grads[which].clone()
            lst[which][pos] = bad_value
            assert flag_of(lst) == 1, f"{bad_value} at element {pos} of tensor {which} ({sizes[which]} elements) was not found"
    assert flag_of(grads) == 0


if __name__ == "__main__":
    sys.exit(_fallback_child())
