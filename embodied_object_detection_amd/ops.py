"""Thin host wrappers over the C ABI: torch supplies device memory and the stream, nothing else.

Every function enqueues HIP kernels on torch's current stream and returns torch tensors that alias the
buffers the kernels write.  No arithmetic is done with torch ops here.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from ._lib import EodConvDesc, EodDetDesc, EodMemWriteDesc, EodProposalDesc, check


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def _stream() -> int:
    """Raw handle of torch's current stream on the current device.  The private fast path avoids building a Stream object per
    launch (torch.cuda.current_stream() was 45 % of the host time of a frame: ~180 launches)."""
    if _raw_stream is not None:
        return _raw_stream(torch.cuda.current_device())
    return torch.cuda.current_stream().cuda_stream


def _ptr(t: Optional[torch.Tensor]) -> Optional[int]:
    return None if t is None else t.data_ptr()


def _need_cuda(*ts):
    for t in ts:
        if t is not None and not t.is_cuda:
            raise _lib.EodError("HIP product path needs device tensors (no CPU fallback)")


class Workspace:
    """Grow-only scratch buffer per device (split-K slabs, selection scratch)."""

    def __init__(self):
        self.bufs = {}

    def get(self, nbytes: int, device) -> torch.Tensor:
        # one buffer per (device, stream): kernels of different streams may run concurrently
        key = (device.index if isinstance(device, torch.device) else str(device), _stream())
        buf = self.bufs.get(key)
        if buf is None or buf.numel() < nbytes:
            buf = torch.empty(max(int(nbytes), 1 << 20), dtype=torch.uint8, device=device)
            self.bufs[key] = buf
        return buf


_conv_ws = Workspace()


# ----------------------------------------------------------------------------------------------------
# weight preparation (host, once per model build)
# ----------------------------------------------------------------------------------------------------
_CONV_MATH = {"fp32": 0, "bf16x3": 1, "f16": 2}
WGRAD_F16 = 512      # EOD_WGRAD_F16 of include/eod_hip.h: on the stride argument of eod_conv2d_backward_weights_ws


def set_conv_math(mode: str) -> str:
    """Arithmetic of every conv / linear launch from now on (process-wide): "fp32" (fp32 MFMA, default), "bf16x3" (three-way
    bf16 operand split on the bf16 MFMA pipe, fp32 accumulate) or "f16" (operands rounded to half, fp32 accumulate, fp32 outputs:
    inference only; include/eod_hip.h eod_set_conv_math).  Returns the previous mode."""
    if mode not in _CONV_MATH:
        hint = ""
        if str(mode).lower() == "fp16":
            hint = (' ("fp16" / FP16 is the config key of autocast training: modeling.training.build_trainer / AmpTrainer, which choose '
                    'the arithmetic per launch; the process-wide inference arithmetic is "f16")')
        raise ValueError(f"conv math must be one of {sorted(_CONV_MATH)}, got {mode!r}{hint}")
    prev = _lib.load().eod_set_conv_math(_CONV_MATH[mode])
    check(min(prev, 0), "eod_set_conv_math")
    return {v: k for k, v in _CONV_MATH.items()}[prev]


def get_conv_math() -> str:
    return {v: k for k, v in _CONV_MATH.items()}[_lib.load().eod_get_conv_math()]


def fold_bn(w: torch.Tensor, bn_w, bn_b, bn_mean, bn_var, eps: float = 1e-5):
    """FrozenBatchNorm2d folded into the preceding bias-free conv."""
    scale = bn_w / torch.sqrt(bn_var + eps)
    return w * scale.view(-1, 1, 1, 1), bn_b - bn_mean * scale


def pack_conv_weight(w_oihw: torch.Tensor, cin_pad: Optional[int] = None) -> Tuple[torch.Tensor, int]:
    """OIHW -> [Cout, Kpad] with k = (ky, kx, c), c fastest; K padded with zeros to a multiple of 32."""
    O, I, KH, KW = w_oihw.shape
    w = w_oihw.permute(0, 2, 3, 1).contiguous()  # O,KH,KW,I
    if cin_pad is not None and cin_pad != I:
        wp = torch.zeros((O, KH, KW, cin_pad), dtype=w.dtype)
        wp[..., :I] = w
        w = wp
    K = w.shape[1] * w.shape[2] * w.shape[3]
    Kpad = (K + 31) // 32 * 32
    out = torch.zeros((O, Kpad), dtype=torch.float32)
    out[:, :K] = w.reshape(O, K)
    return out.contiguous(), Kpad


class Conv:
    """One prepared conv / linear layer living on the device."""

    def __init__(self, w_oihw: torch.Tensor, bias: Optional[torch.Tensor], stride: int = 1, pad: int = 0,
                 device="cuda", cin_pad: Optional[int] = None, deconv: bool = False, name: str = ""):
        self.name = name
        if deconv:
            # ConvTranspose2d(k=2, s=2) weight [Cin, Cout, 2, 2] -> rows n = (dy*2+dx)*Cout + co, K = Cin
            Cin, Cout, kh, kw = w_oihw.shape
            assert kh == 2 and kw == 2
            w = w_oihw.permute(2, 3, 1, 0).reshape(4 * Cout, Cin, 1, 1).contiguous()
            self.out_mode = 1
            self.KH = self.KW = 1
            self.stride, self.pad = 1, 0
            self.Cin, self.Cout = Cin, 4 * Cout
        else:
            w = w_oihw
            self.out_mode = 0
            self.Cout, cin, self.KH, self.KW = w.shape
            self.Cin = cin_pad or cin
            self.stride, self.pad = stride, pad
        packed, self.Kpad = pack_conv_weight(w, cin_pad)
        self.tap4 = 1 if self.Cin == 4 else 0
        if not self.tap4 and self.Cin % 32 != 0:
            raise ValueError(f"{name}: Cin={self.Cin} must be a multiple of 32 (or 4 for the stem)")
        self.w = packed.to(device)
        self.bias = None if bias is None else bias.detach().to(torch.float32).contiguous().to(device)
        self.desc = EodConvDesc()
        self._lib = _lib.load()
        self.w_split = None     # bf16x3 pieces of the weights, made on first use in that arithmetic mode
        self.w_half = None      # the weights rounded to half, made on first use in f16 mode; dropped wherever w_split is
        self.event_log = None   # bench.py: list that receives (start_event, end_event, event_tag) per launch
        self.event_tag = None   # what the caller wants to know the launch by (no device work: a clone of m_count would be a launch)
        self.lds_reserve = 0    # EodConvDesc.lds_reserve: caps this layer's workgroups per CU (see include/eod_hip.h)
        self.prefetch2 = 0      # EodConvDesc.prefetch2: two chunks of operands in flight (small launches)

    def out_hw(self, H: int, W: int) -> Tuple[int, int]:
        return ((H + 2 * self.pad - self.KH) // self.stride + 1, (W + 2 * self.pad - self.KW) // self.stride + 1)

    def __call__(self, x: torch.Tensor, N: int, H: int, W: int, *, res: Optional[torch.Tensor] = None, res_mode: int = 0,
                 relu: bool = False, in_relu: bool = False, out_scale: float = 1.0, m_count: Optional[torch.Tensor] = None,
                 m_unit: int = 0, out: Optional[torch.Tensor] = None, force_tile: int = 0, force_splitk: int = 0,
                 levels: Optional[Tuple[Sequence[int], Sequence[Tuple[int, int]]]] = None,
                 fuse: Optional[Tuple[torch.Tensor, float, Optional[torch.Tensor]]] = None, presplit: bool = True,
                 plan_rows: int = 0, gn_stats: Optional[torch.Tensor] = None, gn_groups: int = 32,
                 split: Optional[Tuple[int, torch.Tensor]] = None, m_segments: int = 0,
                 gate: Optional[torch.Tensor] = None, math: Optional[str] = None) -> torch.Tensor:
        """`levels=(row_offsets, [(h, w), ...])` runs the layer once over a whole feature pyramid stored as one row list.
        `math` ("fp32" | "bf16x3" | "f16"; None = the process-wide mode of `set_conv_math`): the arithmetic of THIS call
        (EodConvDesc.math) -- the AMP training step runs the backbone's launches in f16 beside fp32 heads this way.
        `split=(n0, out2)`: the layer is two stacked linear layers; columns [0, n0) go to `out` [rows, n0] without the ReLU, columns
        [n0, Cout) to `out2` [rows, Cout - n0] with it (EodConvDesc.split_n).
        `m_segments` = B: the N images are B unit lists back to back, `m_count` holds B counts (EodConvDesc.m_segments).
        `gn_stats` (pyramid mode; the workspace of the `groupnorm_relu` call that follows): when the layer's plan reduces split-K
        slabs, that reduce also writes GroupNorm's partial sums into it and `self.gn_fused` is set (pass it as `partial_ready`).
        `gate` [N,OH,OW,Cout]: the output is zeroed where gate <= 0 (EodConvDesc.gate: a ReLU's backward on the way out).
        `fuse=(pred_w [Cout/4], pred_b, out_units or None)` (deconv layers only): ConvTranspose + ReLU + 1x1 predictor + sigmoid
        in one launch, `out` = [units, 2H, 2W] probabilities (out_mode 2 of include/eod_hip.h)."""
        _need_cuda(x, res, out, gate)
        if fuse is not None:
            if self.out_mode != 1 or out is None:
                raise ValueError("fuse= needs a deconv layer and an explicit probability buffer `out`")
            _need_cuda(fuse[0], fuse[2])
        OH, OW = self.out_hw(H, W) if levels is None else (0, 0)
        if levels is not None and out is None:
            out = torch.empty((levels[0][-1], self.Cout), dtype=torch.float32, device=x.device)
        if out is None:
            if self.out_mode == 1:
                out = torch.empty((N, 2 * OH, 2 * OW, self.Cout // 4), dtype=torch.float32, device=x.device)
            else:
                out = torch.empty((N, OH, OW, self.Cout), dtype=torch.float32, device=x.device)
        d = self.desc
        d.x, d.w, d.bias, d.res, d.y = x.data_ptr(), self.w.data_ptr(), _ptr(self.bias), _ptr(res), out.data_ptr()
        d.m_count, d.m_unit, d.m_segments = _ptr(m_count), m_unit, int(m_segments)
        d.gate = _ptr(gate)
        if math is not None and math not in _CONV_MATH:
            raise ValueError(f"math={math!r}: one of {sorted(_CONV_MATH)} or None")
        d.math = 0 if math is None else _CONV_MATH[math] + 1
        d.N, d.H, d.W, d.Cin, d.OH, d.OW, d.Cout = N, H, W, self.Cin, OH, OW, self.Cout
        d.KH, d.KW, d.stride, d.pad, d.Kpad = self.KH, self.KW, self.stride, self.pad, self.Kpad
        d.relu, d.res_mode, d.in_relu, d.out_mode, d.tap4 = int(relu), res_mode, int(in_relu), self.out_mode, self.tap4
        if fuse is not None:
            d.out_mode, d.fuse_w, d.fuse_b, d.out_units = 2, fuse[0].data_ptr(), float(fuse[1]), _ptr(fuse[2])
        else:
            d.fuse_w, d.fuse_b, d.out_units = None, 0.0, None
        d.force_tile, d.force_splitk, d.out_scale = force_tile, force_splitk, out_scale
        d.plan_rows = plan_rows
        d.lds_reserve = self.lds_reserve
        d.prefetch2 = self.prefetch2
        d.gn_partial, d.gn_groups = None, 0
        self.gn_fused = False
        if split is not None:
            _need_cuda(split[1])
            d.split_n, d.y2 = int(split[0]), split[1].data_ptr()
        else:
            d.split_n, d.y2 = 0, None
        if levels is not None:
            off, shapes = levels
            d.levels = len(shapes)
            for i, o in enumerate(off):
                d.level_off[i] = o
            for i, (h, w) in enumerate(shapes):
                d.level_h[i], d.level_w[i] = h, w
        else:
            d.levels = 0
        mode = math if math is not None else get_conv_math()
        use_split = force_tile // 10 == 5 if force_tile else (mode == "bf16x3")
        if use_split and self.w_split is None and not self.tap4:
            nb = self._lib.eod_conv_split_weights_bytes(self.Cout, self.Kpad)
            self.w_split = torch.empty((nb,), dtype=torch.uint8, device=self.w.device)
            check(self._lib.eod_conv_split_weights_bf16x3(self.w.data_ptr(), self.Cout, self.Kpad, self.w_split.data_ptr(), _stream()),
                  f"eod_conv_split_weights_bf16x3[{self.name}]")
        d.w_split = self.w_split.data_ptr() if (use_split and self.w_split is not None and presplit) else None
        use_half = force_tile // 10 in (8, 9) if force_tile else (mode == "f16")
        if use_half and self.w_half is None and not self.tap4:
            nb = self._lib.eod_conv_half_weights_bytes(self.Cout, self.Kpad)
            self.w_half = torch.empty((nb,), dtype=torch.uint8, device=self.w.device)
            check(self._lib.eod_conv_half_weights(self.w.data_ptr(), self.Cout, self.Kpad, self.w_half.data_ptr(), _stream()),
                  f"eod_conv_half_weights[{self.name}]")
            # the copy is used by every later launch of the layer, on whatever stream (the look-ahead trunk runs beside the frame
            # that made it): finished before anybody can see it.  Once per layer; inside a graph capture it is ordered by the capture.
            if not torch.cuda.is_current_stream_capturing():
                torch.cuda.current_stream(self.w.device).synchronize()
        d.w_half = self.w_half.data_ptr() if (use_half and self.w_half is not None and presplit) else None
        if gn_stats is not None and levels is not None and self._lib.eod_conv2d_gn_fused(C.byref(d)):
            d.gn_partial = gn_stats.data_ptr() + self._lib.eod_groupnorm_partial_offset(len(levels[1]), gn_groups)
            d.gn_groups = gn_groups
            self.gn_fused = True
        d.workspace, d.workspace_bytes = None, 0
        need = self._lib.eod_conv2d_workspace_bytes(C.byref(d))
        if need:
            ws = _conv_ws.get(need, x.device)
            d.workspace, d.workspace_bytes = ws.data_ptr(), ws.numel()
        if self.event_log is not None:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            check(self._lib.eod_conv2d(C.byref(d), _stream()), f"eod_conv2d[{self.name}]")
            e1.record()
            self.event_log.append((e0, e1, self.event_tag))
            return out
        check(self._lib.eod_conv2d(C.byref(d), _stream()), f"eod_conv2d[{self.name}]")
        return out

    def plan(self) -> Dict[str, int]:
        """The plan `eod_conv2d` makes for the descriptor of this layer's last call in the current arithmetic mode (EodConvPlan of
        include/eod_hip.h as a dict): a read-back of the planner, nothing is launched."""
        p = _lib.EodConvPlan()
        check(self._lib.eod_conv2d_plan(C.byref(self.desc), C.byref(p)), f"eod_conv2d_plan[{self.name}]")
        return {n: int(getattr(p, n)) for n, _t in p._fields_}


# ----------------------------------------------------------------------------------------------------
# elementwise / pooling
# ----------------------------------------------------------------------------------------------------
def preprocess_image(img_u8_chw: torch.Tensor, mean: Sequence[float], std: Sequence[float], div: int = 32,
                     out: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, int, int]:
    """`out` (optional): a [1,Hp,Wp,4] slice of a batch buffer to write into."""
    _need_cuda(img_u8_chw)
    assert img_u8_chw.dtype == torch.uint8 and img_u8_chw.dim() == 3 and img_u8_chw.is_contiguous()
    _, H, W = img_u8_chw.shape
    Hp, Wp = (H + div - 1) // div * div, (W + div - 1) // div * div
    if out is None:
        out = torch.empty((1, Hp, Wp, 4), dtype=torch.float32, device=img_u8_chw.device)
    assert out.numel() == Hp * Wp * 4 and out.is_contiguous()
    m = (C.c_float * 3)(*mean)
    s = (C.c_float * 3)(*std)
    check(_lib.load().eod_preprocess_image(img_u8_chw.data_ptr(), out.data_ptr(), H, W, Hp, Wp, m, s, _stream()),
          "eod_preprocess_image")
    return out, Hp, Wp


def maxpool3x3s2(x: torch.Tensor, N: int, H: int, W: int, Cc: int) -> Tuple[torch.Tensor, int, int]:
    OH, OW = (H + 2 - 3) // 2 + 1, (W + 2 - 3) // 2 + 1
    y = torch.empty((N, OH, OW, Cc), dtype=torch.float32, device=x.device)
    check(_lib.load().eod_maxpool3x3s2(x.data_ptr(), y.data_ptr(), N, H, W, Cc, OH, OW, _stream()), "eod_maxpool3x3s2")
    return y, OH, OW


def groupnorm_workspace(level_off: Sequence[int], device, groups: int = 32) -> torch.Tensor:
    lo = (C.c_int32 * len(level_off))(*level_off)
    n = _lib.load().eod_groupnorm_workspace_bytes(lo, len(level_off) - 1, groups)
    return torch.empty(((n + 7) // 8,), dtype=torch.float64, device=device)


def groupnorm_relu(x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, level_off: Sequence[int], Cc: int,
                   stats: torch.Tensor, groups: int = 32, eps: float = 1e-5, out: Optional[torch.Tensor] = None,
                   partial_ready: bool = False) -> torch.Tensor:
    """`partial_ready`: the conv that produced `x` already wrote the partial sums into `stats` (Conv(..., gn_stats=stats))."""
    if out is None:
        out = torch.empty_like(x)
    lo = (C.c_int32 * len(level_off))(*level_off)
    check(_lib.load().eod_groupnorm_relu(x.data_ptr(), out.data_ptr(), gamma.data_ptr(), beta.data_ptr(), lo, len(level_off) - 1,
                                         Cc, groups, eps, stats.data_ptr(), int(partial_ready), _stream()), "eod_groupnorm_relu")
    return out


def groupnorm_relu_backward(x: torch.Tensor, y: torch.Tensor, dy: torch.Tensor, gamma: torch.Tensor, level_off: Sequence[int], Cc: int,
                            fwd_stats: torch.Tensor, groups: int = 32, eps: float = 1e-5):
    """Backward of `groupnorm_relu` (its input `x`, output `y`, the `stats` workspace of that call) -> (dx, dgamma, dbeta)."""
    _need_cuda(x, y, dy, gamma, fwd_stats)
    lo = (C.c_int32 * len(level_off))(*level_off)
    lib = _lib.load()
    ws = torch.empty((lib.eod_groupnorm_backward_workspace_bytes(lo, len(level_off) - 1, Cc) // 8,), dtype=torch.float64, device=x.device)
    dx = torch.empty_like(x)
    dgamma = torch.empty((Cc,), dtype=torch.float32, device=x.device)
    dbeta = torch.empty((Cc,), dtype=torch.float32, device=x.device)
    check(lib.eod_groupnorm_relu_backward(x.data_ptr(), y.data_ptr(), dy.data_ptr(), gamma.data_ptr(), lo, len(level_off) - 1, Cc, groups, eps,
                                          fwd_stats.data_ptr(), ws.data_ptr(), dx.data_ptr(), dgamma.data_ptr(), dbeta.data_ptr(), _stream()),
          "eod_groupnorm_relu_backward")
    return dx, dgamma, dbeta


def mask_predictor_sigmoid(x: torch.Tensor, w: torch.Tensor, bias: float, rows: int, Cc: int, count: Optional[torch.Tensor],
                           unit_rows: int, out: Optional[torch.Tensor] = None, out_units: Optional[torch.Tensor] = None) -> torch.Tensor:
    if out is None:
        out = torch.empty((rows,), dtype=torch.float32, device=x.device)
    check(_lib.load().eod_mask_predictor_sigmoid(x.data_ptr(), w.data_ptr(), bias, out.data_ptr(), rows, Cc, _ptr(count),
                                                 unit_rows, _ptr(out_units), _stream()), "eod_mask_predictor_sigmoid")
    return out


def roi_align(p3, p4, p5, h3: int, w3: int, Cc: int, boxes: torch.Tensor, count: Optional[torch.Tensor], R_cap: int, S: int,
              out: Optional[torch.Tensor] = None, box_rows: Optional[torch.Tensor] = None, batch: int = 1,
              boxes_per_image: int = 0, refine=None) -> torch.Tensor:
    """`batch` > 1: p3..p5 are [batch,h,w,C]; box j is pooled from image j // boxes_per_image (include/eod_hip.h).
    `refine = (deltas, ld, weights, clip, img_w, img_h, boxes_out)`: the ROI boxes are apply_deltas(boxes, deltas), also written to
    `boxes_out` (EodBoxRefine: the cascade's next-stage proposals without their own launch)."""
    if out is None:
        out = torch.empty((R_cap, S, S, Cc), dtype=torch.float32, device=p3.device)
    ref = None
    if refine is not None:
        deltas, ld, (wx, wy, ww, wh), clip, img_w, img_h, boxes_out = refine
        _need_cuda(deltas, boxes_out)
        ref = _lib.EodBoxRefine(deltas.data_ptr(), ld, wx, wy, ww, wh, int(clip), img_w, img_h, boxes_out.data_ptr())
    check(_lib.load().eod_roi_align(p3.data_ptr(), p4.data_ptr(), p5.data_ptr(), h3, w3, Cc, boxes.data_ptr(), _ptr(box_rows),
                                    _ptr(count), R_cap, S, out.data_ptr(), batch, boxes_per_image, None if ref is None else C.byref(ref),
                                    _stream()), "eod_roi_align")
    return out


def roi_align_backward(dp3, dp4, dp5, h3: int, w3: int, Cc: int, boxes: torch.Tensor, count: Optional[torch.Tensor], R_cap: int, S: int,
                       g: torch.Tensor):
    """Adds the pooling's gradient into the pyramid levels' gradients dp3..dp5 ([h,w,C] each, one image); g [R,S,S,C]."""
    _need_cuda(dp3, dp4, dp5, boxes, g)
    assert g.is_contiguous() and tuple(g.shape) == (R_cap, S, S, Cc)
    check(_lib.load().eod_roi_align_backward(dp3.data_ptr(), dp4.data_ptr(), dp5.data_ptr(), h3, w3, Cc, boxes.data_ptr(), _ptr(count),
                                             R_cap, S, g.data_ptr(), _stream()), "eod_roi_align_backward")


def concat_lists(lists: torch.Tensor, counts: torch.Tensor, cap_in: int, id_stride: int, batch: int, out: torch.Tensor,
                 out_count: torch.Tensor):
    """The scene-local index lists of a batch as one list of global indices b * id_stride + lists[b][k] (eod_concat_lists)."""
    check(_lib.load().eod_concat_lists(lists.data_ptr(), counts.data_ptr(), cap_in, id_stride, batch, out.data_ptr(), out_count.data_ptr(),
                                       _stream()), "eod_concat_lists")
    return out, out_count


def unique_rows(rows: torch.Tensor, count: torch.Tensor, K_cap: int, R_cap: int, out_rows: torch.Tensor, out_count: torch.Tensor):
    check(_lib.load().eod_unique_rows(rows.data_ptr(), count.data_ptr(), K_cap, R_cap, out_rows.data_ptr(), out_count.data_ptr(),
                                      _stream()), "eod_unique_rows")


# ----------------------------------------------------------------------------------------------------
# selection
# ----------------------------------------------------------------------------------------------------
class ProposalDecoder:
    """CenterNet.inference on device (centernet.py:603-745)."""

    def __init__(self, level_hw: Sequence[Tuple[int, int]], strides: Sequence[int], scales: Sequence[float], score_thresh: float,
                 pre_nms_topk: int, post_nms_topk: int, nms_thresh: float, cap: int, device, head_stride: int = 5, batch: int = 1):
        """`batch` > 1: B scenes in lock-step; `head_out` is level major over the scenes, the outputs are [B*cap,4] / [B*cap] / [B]."""
        self.lib = _lib.load()
        d = EodProposalDesc()
        off = [0]
        for (h, w) in level_hw:
            off.append(off[-1] + h * w)
        d.levels = len(level_hw)
        for i, o in enumerate(off):
            d.level_off[i] = o
        for i, (h, w) in enumerate(level_hw):
            d.level_w[i] = w
            d.level_stride[i] = strides[i]
            d.level_scale[i] = scales[i]
        d.head_stride = head_stride
        d.score_thresh, d.pre_nms_topk, d.post_nms_topk, d.nms_thresh, d.cap = score_thresh, pre_nms_topk, post_nms_topk, nms_thresh, cap
        nbytes = self.lib.eod_proposals_workspace_bytes(off[-1], d.levels, pre_nms_topk, batch)
        d.batch = batch
        self.ws = torch.empty((nbytes,), dtype=torch.uint8, device=device)
        self.boxes = torch.zeros((batch * cap, 4), dtype=torch.float32, device=device)
        self.scores = torch.zeros((batch * cap,), dtype=torch.float32, device=device)
        self.count = torch.zeros((batch,), dtype=torch.int32, device=device)
        d.out_boxes, d.out_scores, d.out_count = self.boxes.data_ptr(), self.scores.data_ptr(), self.count.data_ptr()
        d.workspace, d.workspace_bytes = self.ws.data_ptr(), nbytes
        self.desc = d
        self.total = off[-1]
        self.level_off = off

    def __call__(self, head_out: torch.Tensor):
        self.desc.head_out = head_out.data_ptr()
        check(self.lib.eod_centernet_proposals(C.byref(self.desc), _stream()), "eod_centernet_proposals")
        return self.boxes, self.scores, self.count


class DetectionSelector:
    """detectron2 fast_rcnn_inference (single image) on device: ONE launch.  `unique=True`: the launch also writes torch.unique of
    the kept proposal rows (`uniq_rows`, `uniq_count`; custom_rcnn.py:875).  `groups=True`: it also groups the detections by
    proposal row -- detections of one row carry the same class-agnostic box: `rep_of[k]` = the first detection of k's group,
    `rep_list` / `rep_count` = the group representatives."""

    def __init__(self, R_cap: int, C1: int, topk: int, device, unique: bool = False, groups: bool = False, batch: int = 1):
        """`batch` > 1: B scenes, one workgroup each; every buffer is B single-scene buffers back to back, indices stay scene-local."""
        self.lib = _lib.load()
        self.R_cap, self.C1, self.topk, self.batch = R_cap, C1, topk, batch
        nbytes = self.lib.eod_detections_workspace_bytes(R_cap, C1)
        if nbytes == 0:
            raise _lib.EodError(f"eod_fast_rcnn_inference: {R_cap} rows x {C1 - 1} classes are not supported (at most 512 rows, 2047 classes)")
        # zeroed: the wide path (more than 24 classes) keeps a histogram here that every call leaves cleared for the next one
        self.ws = torch.zeros((nbytes,), dtype=torch.uint8, device=device)
        B = batch
        self.boxes = torch.zeros((B * topk, 4), dtype=torch.float32, device=device)
        self.scores = torch.zeros((B * topk,), dtype=torch.float32, device=device)
        self.classes = torch.zeros((B * topk,), dtype=torch.int32, device=device)
        self.rows = torch.zeros((B * topk,), dtype=torch.int32, device=device)
        self.count = torch.zeros((B,), dtype=torch.int32, device=device)
        d = EodDetDesc()
        d.R_cap, d.C1, d.topk, d.batch = R_cap, C1, topk, batch
        d.out_boxes, d.out_scores, d.out_classes = self.boxes.data_ptr(), self.scores.data_ptr(), self.classes.data_ptr()
        d.out_rows, d.out_count = self.rows.data_ptr(), self.count.data_ptr()
        d.workspace, d.workspace_bytes = self.ws.data_ptr(), nbytes
        self.uniq_rows = self.uniq_count = None
        if unique:
            self.uniq_rows = torch.zeros((B * R_cap,), dtype=torch.int32, device=device)
            self.uniq_count = torch.zeros((B,), dtype=torch.int32, device=device)
            d.out_unique_rows, d.out_unique_count, d.unique_cap = self.uniq_rows.data_ptr(), self.uniq_count.data_ptr(), R_cap
        self.rep_of = self.rep_list = self.rep_count = None
        if groups:
            self.rep_of = torch.zeros((B * topk,), dtype=torch.int32, device=device)
            self.rep_list = torch.zeros((B * topk,), dtype=torch.int32, device=device)
            self.rep_count = torch.zeros((B,), dtype=torch.int32, device=device)
            d.out_rep_of, d.out_rep_list, d.out_rep_count = self.rep_of.data_ptr(), self.rep_list.data_ptr(), self.rep_count.data_ptr()
        self.desc = d
        # the one-workgroup kernel (at most 24 classes and 8192 slots) can be handed the boxes' suppression matrix: `build_row_matrix`
        self.takes_row_matrix = C1 - 1 <= 24 and R_cap * (C1 - 1) <= 8192
        self.row_matrix = None
        self._matrix_for = None       # arguments of the `build_row_matrix` launch that the next call may use

    def build_row_matrix(self, boxes: torch.Tensor, count: Optional[torch.Tensor], img_w: float, img_h: float, nms_thresh: float):
        """The selection's R x R suppression bit matrix as a launch of its own (several workgroups), on the current stream.  It reads
        the boxes only: enqueued while the scores are still being computed, the matrix is ready before the selection starts.  The
        NEXT call of the selector -- same boxes, count, image size and NMS threshold, anything else is an error -- reads the matrix
        instead of building it, on a stream that is ordered behind this launch.  Same results."""
        if not self.takes_row_matrix:
            raise _lib.EodError("eod_fast_rcnn_inference: the wide selection path builds its suppression matrix itself")
        if self.row_matrix is None:
            self.row_matrix = torch.zeros((self.batch * self.R_cap, (self.R_cap + 63) // 64), dtype=torch.int64, device=self.boxes.device)
            m = EodDetDesc()          # the matrix mode of the entry point: a descriptor of its own
            m.R_cap, m.C1, m.batch, m.row_matrix_out = self.R_cap, self.C1, self.batch, self.row_matrix.data_ptr()
            self._matrix_desc = m
        m = self._matrix_desc
        m.boxes, m.count, m.img_w, m.img_h, m.nms_thresh = boxes.data_ptr(), _ptr(count), img_w, img_h, nms_thresh
        check(self.lib.eod_fast_rcnn_inference(C.byref(m), _stream()), "eod_fast_rcnn_inference (row matrix)")
        self._matrix_for = (boxes.data_ptr(), _ptr(count), float(img_w), float(img_h), float(nms_thresh))
        return self.row_matrix

    def __call__(self, boxes: torch.Tensor, scores: torch.Tensor, count: Optional[torch.Tensor], img_w: float, img_h: float,
                 score_thresh: float, nms_thresh: float):
        d = self.desc
        d.boxes, d.scores, d.count = boxes.data_ptr(), scores.data_ptr(), _ptr(count)
        d.img_w, d.img_h, d.score_thresh, d.nms_thresh = img_w, img_h, score_thresh, nms_thresh
        built, self._matrix_for = self._matrix_for, None
        if built is not None and built != (d.boxes, d.count, float(img_w), float(img_h), float(nms_thresh)):
            raise _lib.EodError("eod_fast_rcnn_inference: the suppression matrix was built for other boxes, count, image size or threshold")
        d.row_matrix = None if built is None else self.row_matrix.data_ptr()
        check(self.lib.eod_fast_rcnn_inference(C.byref(d), _stream()), "eod_fast_rcnn_inference")
        return self.boxes, self.scores, self.classes, self.rows, self.count


ZS_WIDE = 2          # EOD_ZS_WIDE: the flag bit on `accumulate` that asks for the wide-vocabulary classifier kernel
ZS_MAX_C1 = 24       # columns the narrow (LDS-staged) classifier kernel holds
ZS_WIDE_MAX_C1 = 2048


def _zs_refusal(name: str, C1: int, wide: bool) -> str:
    if wide:
        return (f"{name}: {C1 - 1} classes + background exceed the wide classifier kernel's {ZS_WIDE_MAX_C1} columns "
                f"(at most {ZS_WIDE_MAX_C1 - 1} classes on the HIP path)")
    return (f"{name}: {C1 - 1} classes + background do not fit the narrow kernel's LDS-staged class matrix (at most {ZS_MAX_C1 - 1} "
            f"classes); pass wide=True for a RESET_CLS_TESTS / TEST_NUM_CLASSES vocabulary of up to {ZS_WIDE_MAX_C1 - 1} classes")


def zs_classify(feat, zs, prob_acc, accumulate: bool, featn_out, count, R_cap: int, C1: int, temp: float = 50.0, zs_mem=None,
                prop_scores=None, mem_scores_out=None, final_inv_stages: float = 0.0, batch: int = 1, wide: bool = False):
    """`zs_mem` + `prop_scores` + `mem_scores_out`: also the memory update's CLIP re-score (what `memory_scores` computes) in the same
    launch; `final_inv_stages` > 0 (last cascade stage): also the cascade score fusion (what `cascade_scores` does).
    `wide=True` (EOD_ZS_WIDE): vocabularies of 24 to 2047 classes run the matrix-core kernel; up to 23 classes it changes nothing."""
    st = _lib.load().eod_zs_classify(feat.data_ptr(), zs.data_ptr(), prob_acc.data_ptr(), int(bool(accumulate)) | (ZS_WIDE if wide else 0),
                                     _ptr(featn_out), _ptr(count), R_cap, 512, C1, temp, _ptr(zs_mem), _ptr(prop_scores),
                                     _ptr(mem_scores_out), float(final_inv_stages), batch, _stream())
    if st == -5:
        raise _lib.EodError(_zs_refusal("eod_zs_classify", C1, wide))
    check(st, "eod_zs_classify")


def cascade_stage_tail(feat, zs, prob_acc, accumulate: bool, featn_out, count, R_cap: int, C1: int, temp: float, hb, bb2: "Conv", boxes_in,
                       boxes_out, weights, clip: bool, img_w: float, img_h: float, zs_mem=None, prop_scores=None, mem_scores_out=None,
                       final_inv_stages: float = 0.0, deltas_out=None, batch: int = 1, wide: bool = False):
    """`zs_classify` + bbox_pred.2 + apply_deltas of one cascade stage in ONE launch (`eod_cascade_stage_tail`); `bb2` is the stage's
    1024 -> 4 layer (its packed weight rows and bias are read in place).  `wide`: as in `zs_classify`."""
    d = _lib.EodStageTailDesc()
    d.feat, d.zs, d.prob_acc, d.feat_norm_out, d.count = feat.data_ptr(), zs.data_ptr(), prob_acc.data_ptr(), _ptr(featn_out), _ptr(count)
    d.accumulate = int(bool(accumulate)) | (ZS_WIDE if wide else 0)
    d.R_cap, d.D, d.C1, d.temp = R_cap, 512, C1, temp
    d.zs_mem, d.prop_scores, d.mem_scores_out, d.final_inv_stages, d.batch = _ptr(zs_mem), _ptr(prop_scores), _ptr(mem_scores_out), float(final_inv_stages), batch
    d.hb, d.w2, d.b2, d.hb_dim, d.w2_ld = hb.data_ptr(), bb2.w.data_ptr(), bb2.bias.data_ptr(), bb2.Cin, bb2.Kpad
    d.boxes_in, d.boxes_out, d.deltas_out = boxes_in.data_ptr(), boxes_out.data_ptr(), _ptr(deltas_out)
    d.wx, d.wy, d.ww, d.wh = weights
    d.clip, d.img_w, d.img_h = int(clip), img_w, img_h
    st = _lib.load().eod_cascade_stage_tail(C.byref(d), _stream())
    if st == -5:
        raise _lib.EodError(_zs_refusal("eod_cascade_stage_tail", C1, wide))
    check(st, "eod_cascade_stage_tail")


def apply_deltas(deltas, ld: int, boxes, out, count, R_cap: int, weights, clip: bool, img_w: float, img_h: float, batch: int = 1):
    wx, wy, ww, wh = weights
    check(_lib.load().eod_apply_deltas(deltas.data_ptr(), ld, boxes.data_ptr(), out.data_ptr(), _ptr(count), R_cap, wx, wy, ww, wh,
                                       int(clip), img_w, img_h, batch, _stream()), "eod_apply_deltas")


def cascade_scores(prob_acc, prop_scores, count, R_cap: int, C1: int, inv_stages: float):
    check(_lib.load().eod_cascade_scores(prob_acc.data_ptr(), prop_scores.data_ptr(), _ptr(count), R_cap, C1, inv_stages, _stream()),
          "eod_cascade_scores")


def memory_scores(featn, zs, prop_scores, scores_out, count, R_cap: int, C1: int):
    """Dispatches on `C1` by itself: up to 24 columns the wave-per-row kernel, up to 2048 the matrix-core kernel."""
    check(_lib.load().eod_memory_scores(featn.data_ptr(), zs.data_ptr(), prop_scores.data_ptr(), scores_out.data_ptr(), _ptr(count),
                                        R_cap, 512, C1, _stream()), "eod_memory_scores")


def detector_postprocess(boxes, scores, classes, count, cap: int, sx: float, sy: float, out_w: float, out_h: float, ob, os_, oc, osrc,
                         ocount, remap=None, batch: int = 1):
    """`remap` (int32 [cap], optional): osrc[q] = remap[index of the kept detection] -- the detection whose mask stands for it."""
    check(_lib.load().eod_detector_postprocess(boxes.data_ptr(), scores.data_ptr(), classes.data_ptr(), _ptr(count), cap, sx, sy,
                                               out_w, out_h, ob.data_ptr(), os_.data_ptr(), oc.data_ptr(), osrc.data_ptr(),
                                               ocount.data_ptr(), _ptr(remap), batch, _stream()), "eod_detector_postprocess")


def paste_masks(prob, boxes, rows, count, K_cap: int, H: int, W: int, thr: float, out: torch.Tensor, batch: int = 1,
                prob_units: int = 0):
    check(_lib.load().eod_paste_masks(prob.data_ptr(), boxes.data_ptr(), _ptr(rows), _ptr(count), K_cap, H, W, thr, out.data_ptr(),
                                      batch, prob_units, _stream()), "eod_paste_masks")
    return out


# ----------------------------------------------------------------------------------------------------
# spatial memory
# ----------------------------------------------------------------------------------------------------
def unproject_grid_index(depth: torch.Tensor, T: np.ndarray, intr, proj_shift, map_shift, cell: float, map_w: int, map_h: int,
                         order: int = 0, want_xyz: bool = False):
    _need_cuda(depth)
    H, W = depth.shape
    idx = torch.empty((H, W), dtype=torch.int32, device=depth.device)
    xyz = torch.empty((H, W, 3), dtype=torch.float32, device=depth.device) if want_xyz else None
    T16 = (C.c_float * 16)(*np.asarray(T, dtype=np.float32).reshape(-1).tolist())
    ps = (C.c_float * 3)(*np.asarray(proj_shift, dtype=np.float32).tolist())
    ms = (C.c_float * 3)(*np.asarray(map_shift, dtype=np.float32).tolist())
    fx, fy, cx, cy = [float(np.float32(v)) for v in intr]
    check(_lib.load().eod_unproject_grid_index(depth.data_ptr(), H, W, T16, fx, fy, cx, cy, ps, ms, float(np.float32(cell)), map_w,
                                               map_h, order, _ptr(xyz), idx.data_ptr(), _stream()), "eod_unproject_grid_index")
    return (idx, xyz) if want_xyz else idx


def memory_normalize_f16(mem: torch.Tensor, obs: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    N, D = mem.shape
    if out is None:
        out = torch.empty((N, D), dtype=torch.float16, device=mem.device)
    check(_lib.load().eod_memory_normalize_f16(mem.data_ptr(), obs.data_ptr(), out.data_ptr(), N, D, _stream()),
          "eod_memory_normalize_f16")
    return out


def memory_normalize_dirty_f16(mem: torch.Tensor, obs: torch.Tensor, dirty: torch.Tensor, out: torch.Tensor) -> torch.Tensor:
    """a4, incremental: re-normalise the rows flagged in `dirty` (int32 [N]) into the resident fp16 table and clear the flags."""
    N, D = mem.shape
    check(_lib.load().eod_memory_normalize_dirty_f16(mem.data_ptr(), obs.data_ptr(), dirty.data_ptr(), out.data_ptr(), N, D, _stream()),
          "eod_memory_normalize_dirty_f16")
    return out


def pooled_rows(H: int, W: int) -> int:
    """Rows of the pooled buffer: every level padded to whole 32-row operand tiles (include/eod_hip.h eod_memory_gather_pool)."""
    return int(_lib.load().eod_memory_pooled_halves(H, W)) // 512


def memory_gather_pool(mem_f16: torch.Tensor, proj: torch.Tensor, H: int, W: int, out: Optional[torch.Tensor] = None,
                       err: Optional[torch.Tensor] = None, torch_order: bool = False, batch: int = 1) -> torch.Tensor:
    """a8 gather + cascaded pooling -> fp16 pooled rows of the three levels in MFMA operand-fragment order (see the header).
    `batch` > 1: mem_f16 [B,N,D], proj [B,H,W], out [B * pooled_rows, D]."""
    N, D = mem_f16.shape[-2:]
    if out is None:
        out = torch.empty((batch * pooled_rows(H, W), D), dtype=torch.float16, device=mem_f16.device)
    check(_lib.load().eod_memory_gather_pool(mem_f16.data_ptr(), proj.data_ptr(), H, W, D, N, out.data_ptr(), _ptr(err), int(torch_order),
                                             batch, _stream()),
          "eod_memory_gather_pool")
    return out


class MemoryProjector:
    """`map_merge_projection{1,2,3}` + MAP_FEATURE_WEIGHT + fusion (timm.py:174-189) as one launch on the f16 matrix cores."""

    def __init__(self, weights: Sequence[torch.Tensor], biases: Sequence[torch.Tensor], device):
        self.lib = _lib.load()
        ws = [w.detach().to(torch.float32).reshape(256, 512).contiguous().to(device) for w in weights]
        bs = [b.detach().to(torch.float32).contiguous().to(device) for b in biases]
        self.prepared = torch.empty((self.lib.eod_memory_project_weights_bytes(),), dtype=torch.uint8, device=device)
        check(self.lib.eod_memory_project_prepare(ws[0].data_ptr(), bs[0].data_ptr(), ws[1].data_ptr(), bs[1].data_ptr(), ws[2].data_ptr(),
                                                  bs[2].data_ptr(), self.prepared.data_ptr(), _stream()), "eod_memory_project_prepare")
        torch.cuda.current_stream().synchronize()       # ws / bs die with this frame; the prepare kernels must have read them

    def refresh(self, weights: Sequence[torch.Tensor], biases: Sequence[torch.Tensor]):
        """Re-prepare from stepped fp32 masters that live on the device ([256,512] / [256], contiguous, kept alive by the caller)."""
        _need_cuda(*weights, *biases)
        for w, b in zip(weights, biases):
            assert w.dtype == torch.float32 and w.is_contiguous() and w.numel() == 256 * 512 and b.is_contiguous() and b.numel() == 256
        check(self.lib.eod_memory_project_prepare(weights[0].data_ptr(), biases[0].data_ptr(), weights[1].data_ptr(), biases[1].data_ptr(),
                                                  weights[2].data_ptr(), biases[2].data_ptr(), self.prepared.data_ptr(), _stream()),
              "eod_memory_project_prepare")

    def __call__(self, pooled_f16: torch.Tensor, feats: torch.Tensor, H: int, W: int, weight: float, mode: str, batch: int = 1):
        """`batch` > 1: `feats` is level major over the scenes (include/eod_hip.h)."""
        _need_cuda(pooled_f16, feats)
        check(self.lib.eod_memory_project_fuse(pooled_f16.data_ptr(), self.prepared.data_ptr(), feats.data_ptr(), H, W, float(weight),
                                               {"sum": 0, "mem_only": 1}[mode], batch, _stream()), "eod_memory_project_fuse")
        return feats


class MemoryProjectorBackward:
    """Backward of `MemoryProjector` + the cascaded pools (timm.py:142-192): the memory-specific part of the training forward
    (first slice).  `__call__(grads, pooled_f16, H, W, weight)` with `grads` = dL/d(fused P3, P4, P5) as [P_l,256]
    fp32 rows -> dict(dW=[3 x [256,512]], db=[3 x [256]], gE=[3 x half [P_l,512]], gE2=fp32 [(H/4)(W/4),512])."""

    def __init__(self, weights: Sequence[torch.Tensor], device):
        self.lib = _lib.load()
        self.device = device
        # d(pooled) = weight * G . W: a 1x1 convolution whose [Cout=512][K=256] matrix is W^T
        self.convs = [Conv(w.detach().to(torch.float32).reshape(256, 512).t().contiguous().reshape(512, 256, 1, 1), None, device=device,
                           name=f"map_merge_projection{i + 1}^T") for i, w in enumerate(weights)]

    def refresh(self, weights: Sequence[torch.Tensor]) -> None:
        """After an optimizer step on the projections: the W^T convs of the input gradient follow the stepped weights."""
        for c, w in zip(self.convs, weights):
            c.w[:, :256].copy_(w.detach().reshape(256, 512).t())
            c.w_split = None
            c.w_half = None

    def __call__(self, grads: Sequence[torch.Tensor], pooled_f16: torch.Tensor, H: int, W: int, weight: float,
                 need_input_grad: bool = True):
        """`need_input_grad=False`: only dW / db (the training step: the memory table is an input of `forward_model`, loader.py:199-223,
        nothing reads the gradient below the pooled operand -- three dgrad convs and the pool backward, ~50 MB of writes, stay out)."""
        _need_cuda(pooled_f16, *grads)
        dev = self.device
        rows = [(H >> (3 + l)) * (W >> (3 + l)) for l in range(3)]
        for g, r in zip(grads, rows):
            assert tuple(g.shape) == (r, 256) and g.dtype == torch.float32 and g.is_contiguous()
        dW = [torch.empty((256, 512), dtype=torch.float32, device=dev) for _ in range(3)]
        db = [torch.empty((256,), dtype=torch.float32, device=dev) for _ in range(3)]
        ws = _conv_ws.get(self.lib.eod_memory_project_backward_weights_workspace_bytes(), dev)      # the position ranges' partial sums
        check(self.lib.eod_memory_project_backward_weights_ws(grads[0].data_ptr(), grads[1].data_ptr(), grads[2].data_ptr(),
                                                              pooled_f16.data_ptr(), H, W, float(weight), dW[0].data_ptr(), db[0].data_ptr(),
                                                              dW[1].data_ptr(), db[1].data_ptr(), dW[2].data_ptr(), db[2].data_ptr(),
                                                              ws.data_ptr(), ws.numel(), _stream()),
              "eod_memory_project_backward_weights_ws")
        if not need_input_grad:
            return dict(dW=dW, db=db)
        dec = [self.convs[l](grads[l].view(1, H >> (3 + l), W >> (3 + l), 256), 1, H >> (3 + l), W >> (3 + l), out_scale=float(weight))
               .view(rows[l], 512) for l in range(3)]
        gE = [torch.empty((rows[l], 512), dtype=torch.float16, device=dev) for l in range(3)]
        gE2 = torch.empty(((H >> 2) * (W >> 2), 512), dtype=torch.float32, device=dev)
        check(self.lib.eod_memory_pool_backward(dec[0].data_ptr(), dec[1].data_ptr(), dec[2].data_ptr(), H, W, gE[0].data_ptr(),
                                                gE[1].data_ptr(), gE[2].data_ptr(), gE2.data_ptr(), _stream()), "eod_memory_pool_backward")
        return dict(dW=dW, db=db, gE=gE, gE2=gE2, dEc=dec)


class ConvBackward:
    """Backward of a `Conv` layer with bias and optional ReLU (third slice): stride-1 'same' layers (CenterNet
    tower, FPN output convs, mask head convs, the trunk's 1x1 / 3x3 convs), strided ones (P6 / P7, the trunk's down-sampling convs)
    and the weight gradient of the 4-channel stem.  `__call__(x, y, g_out)` with the forward's input `x`
    [N,H,W,Cin], output `y` [N,H,W,Cout] (post-ReLU, only read when `relu`) and dL/dy -> dict(dx, dw [Cout, KH*KW*Cin] in the packed
    layout of `Conv.w`, db).  dx = `eod_conv2d` of the pre-activation gradient with the 180-degree rotated, in/out-transposed
    weights; dw / db = `eod_conv2d_backward_weights`."""

    _workspace: Dict = {}      # per device: partial sums of the position-split weight gradient (stream-ordered reuse)
    # The weight gradients are side outputs of the backward chain (only the optimizer reads them), the input gradients ARE the chain:
    # with `side_stream` every dW / db launch goes to a second stream behind an event of the main one and runs beside the next
    # layers' dgrad convs (the training step is one stream of ~30 us kernels otherwise).  Whoever reads a dW on the main stream calls
    # `join(device)` first -- or does its own small ops inside `on_side(device)`.  Per instance (`ConvBackward(conv, side_stream=True)`):
    # off by default, `modeling.training` switches it on for the layers of its steps.
    _side: Dict = {}           # per device: [stream, event recorded behind the last side launch]

    @classmethod
    def _side_state(cls, dev):
        key = torch.device(dev).index or 0
        st = cls._side.get(key)
        if st is None:
            st = cls._side[key] = [torch.cuda.Stream(device=dev), None]
        return st

    @classmethod
    def join(cls, dev) -> None:
        """The current stream waits for every weight-gradient launch (and `on_side` op) issued so far."""
        st = cls._side.get(torch.device(dev).index or 0)
        if st is not None and st[1] is not None:
            torch.cuda.current_stream(dev).wait_event(st[1])

    @classmethod
    def on_side(cls, dev, enabled: bool = True):
        """Context: torch ops on weight gradients (slices, level sums) ordered on the side stream, behind what is there already."""
        import contextlib
        if not enabled:
            return contextlib.nullcontext()
        st = cls._side_state(dev)

        @contextlib.contextmanager
        def ctx():
            with torch.cuda.stream(st[0]):
                yield
                ev = torch.cuda.Event()
                ev.record(st[0])
                st[1] = ev
        return ctx()

    def __init__(self, conv: "Conv", side_stream: bool = False, math: Optional[str] = None):
        """`math` ("f16" or None = as before): the arithmetic of this layer's backward -- "f16" hands the input-gradient convolution
        (zero-insert form included) `math="f16"` and takes the weight gradient from the f16 kernel (EOD_WGRAD_F16); the 4-channel
        stem's weight gradient and the pyramid-mode weight gradient have no f16 form and stay fp32."""
        if conv.out_mode != 0:
            raise ValueError("ConvBackward covers plain convolutions (no deconv)")
        if math not in (None, "fp32", "f16"):
            raise ValueError(f"ConvBackward(math={math!r}): None, 'fp32' or 'f16'")
        self.math = None if math == "fp32" else math
        self._mk = {} if self.math is None else {"math": self.math}        # what the dgrad conv's call gets on top
        self.side_stream = bool(side_stream)
        # stride-1 'same' layers: dX on the matrix cores (eod_conv2d with rotated weights); anything else: the gather kernel
        self.same = conv.stride == 1 and conv.KH == conv.KW and conv.pad * 2 == conv.KH - 1
        # strided 'same'-padded layers (3x3 s2 p1: P6 / P7 and the trunk's conv2; 1x1 s2: its downsample convs): the gradient is
        # spread onto the input grid with zeros in between and goes through the same rotated-weights conv on the matrix cores
        # (3/4 of the products are zeros, still ~20x faster than the gather kernel: 0.87 ms -> tens of us per layer at 640x640)
        self.zero_insert = conv.stride > 1 and conv.KH == conv.KW and conv.pad * 2 == conv.KH - 1
        self.conv = conv
        self.lib = _lib.load()
        self._flipped = None
        self._flipped_of = None

    def _dgrad_conv(self) -> "Conv":
        # rebuilt when the forward weights have been replaced / updated in place (an optimizer step): keyed by the tensor's version
        key = (self.conv.w.data_ptr(), self.conv.w._version)
        if self._flipped is None or self._flipped_of != key:
            c = self.conv
            K = c.KH * c.KW * c.Cin
            w = c.w[:, :K].reshape(c.Cout, c.KH, c.KW, c.Cin)                       # [co, ky, kx, ci]
            if self._flipped is None:
                wt = w.flip(1, 2).permute(3, 0, 1, 2).contiguous()                 # [ci, co, ky', kx'] = OIHW of the transposed conv
                self._flipped = Conv(wt.cpu(), None, stride=1, pad=c.pad, device=c.w.device, name=c.name + "^T")
            else:
                # the weights were stepped: refresh the packed rows [ci][(ky', kx', co)] on the device, one launch
                check(self.lib.eod_conv_rotate_weights(c.w.data_ptr(), c.Cout, c.KH, c.KW, c.Cin, c.Kpad, self._flipped.w.data_ptr(),
                                                       self._flipped.Kpad, _stream()), "eod_conv_rotate_weights")
                self._flipped.w_split = None
                self._flipped.w_half = None
            self._flipped_of = key
        return self._flipped

    def _pyramid(self, x, y, g_out, relu, need_dx, dx_res, dx_gate, levels):
        """`levels=(row_offsets, [(h, w), ...])`: a level-shared layer over a feature pyramid stored as one row list (x [rows, Cin],
        g_out [rows, Cout]; the forward's `Conv(..., levels=)`): dW / db summed over the levels by ONE weight-gradient launch
        (`eod_conv2d_backward_weights_levels`) and dX by one pyramid-mode launch of the rotated-weights conv."""
        c = self.conv
        if not self.same:
            raise ValueError("pyramid mode covers stride-1 'same' layers")
        off, shapes = levels
        L, rows = len(shapes), int(off[-1])
        assert tuple(x.shape) == (rows, c.Cin) and tuple(g_out.shape) == (rows, c.Cout) and x.is_contiguous() and g_out.is_contiguous()
        g = g_out
        if relu:
            g = torch.empty_like(g_out)
            check(self.lib.eod_relu_backward(g_out.data_ptr(), y.data_ptr(), g.data_ptr(), g.numel(), _stream()), "eod_relu_backward")
        lo = (C.c_int32 * (L + 1))(*off)
        lh = (C.c_int32 * L)(*[h for h, _ in shapes])
        lw = (C.c_int32 * L)(*[w for _, w in shapes])
        K = c.KH * c.KW * c.Cin
        dw = torch.empty((c.Cout, K), dtype=torch.float32, device=x.device)
        db = torch.empty((c.Cout,), dtype=torch.float32, device=x.device)
        need = self.lib.eod_conv2d_backward_weights_levels_workspace_bytes(rows, c.Cin, c.Cout, c.KH, c.KW)
        ws = ConvBackward._workspace.get(x.device)
        if need and (ws is None or ws.numel() * 4 < need):
            ws = ConvBackward._workspace[x.device] = torch.empty(((need + 3) // 4,), dtype=torch.float32, device=x.device)
        check(self.lib.eod_conv2d_backward_weights_levels(x.data_ptr(), g.data_ptr(), L, lo, lh, lw, c.Cin, c.Cout, c.KH, c.KW, c.pad,
                                                          dw.data_ptr(), db.data_ptr(), ws.data_ptr() if need else None,
                                                          ws.numel() * 4 if need else 0, _stream()), "eod_conv2d_backward_weights_levels")
        dx = None
        if need_dx:
            dx = self._dgrad_conv()(g, 1, 0, 0, levels=(off, shapes), res=dx_res, res_mode=1 if dx_res is not None else 0, gate=dx_gate,
                                    **self._mk)
        return dict(dx=dx, dw=dw, db=db)

    @staticmethod
    def refresh_all(bws: Sequence["ConvBackward"]) -> None:
        """After an optimizer step: the rotated weights of every layer in `bws` that has an input-gradient convolution, in
        ceil(n / 24) launches (`eod_conv_rotate_weights_multi`) instead of one launch per layer at its next backward."""
        todo = [bw for bw in bws if bw._flipped is not None]
        for bw in bws:
            bw._flipped_of = None
        if not todo:
            return
        descs = (_lib.EodRotateTensor * len(todo))()
        for d, bw in zip(descs, todo):
            c = bw.conv
            d.w, d.out = c.w.data_ptr(), bw._flipped.w.data_ptr()
            d.Cout, d.KH, d.KW, d.Cin, d.ld_in, d.ld_out = c.Cout, c.KH, c.KW, c.Cin, c.Kpad, bw._flipped.Kpad
        check(_lib.load().eod_conv_rotate_weights_multi(descs, len(todo), _stream()), "eod_conv_rotate_weights_multi")
        for bw in todo:
            bw._flipped.w_split = None
            bw._flipped.w_half = None
            bw._flipped_of = (bw.conv.w.data_ptr(), bw.conv.w._version)

    def __call__(self, x: torch.Tensor, y: Optional[torch.Tensor], g_out: torch.Tensor, relu: bool = False, need_dx: bool = True,
                 dx_res: Optional[torch.Tensor] = None, dx_gate: Optional[torch.Tensor] = None,
                 levels: Optional[Tuple[Sequence[int], Sequence[Tuple[int, int]]]] = None):
        c = self.conv
        _need_cuda(x, y, g_out)
        if levels is not None:
            return self._pyramid(x, y, g_out, relu, need_dx, dx_res, dx_gate, levels)
        if c.tap4 and need_dx:
            raise ValueError("the 4-channel stem has a weight gradient only (its input is the image): pass need_dx=False")
        N, H, W, _ = x.shape
        OH, OW = c.out_hw(H, W)
        assert tuple(g_out.shape) == (N, OH, OW, c.Cout) and x.is_contiguous() and g_out.is_contiguous()
        g = g_out
        if relu:
            g = torch.empty_like(g_out)
            check(self.lib.eod_relu_backward(g_out.data_ptr(), y.data_ptr(), g.data_ptr(), g.numel(), _stream()), "eod_relu_backward")
        K = c.KH * c.KW * c.Cin
        need = self.lib.eod_conv2d_backward_weights_workspace_bytes(N, H, W, c.Cin, c.Cout, c.KH, c.KW, c.pad, c.stride)

        def wgrad():
            dw = torch.empty((c.Cout, K), dtype=torch.float32, device=x.device)
            db = torch.empty((c.Cout,), dtype=torch.float32, device=x.device)
            ws = ConvBackward._workspace.get(x.device)
            if need and (ws is None or ws.numel() * 4 < need):
                ws = ConvBackward._workspace[x.device] = torch.empty(((need + 3) // 4,), dtype=torch.float32, device=x.device)
            stride = c.stride | WGRAD_F16 if (self.math == "f16" and not c.tap4) else c.stride
            check(self.lib.eod_conv2d_backward_weights_ws(x.data_ptr(), g.data_ptr(), N, H, W, c.Cin, c.Cout, c.KH, c.KW, c.pad, stride,
                                                          dw.data_ptr(), db.data_ptr(), ws.data_ptr() if need else None,
                                                          ws.numel() * 4 if need else 0, _stream()), "eod_conv2d_backward_weights_ws")
            return dw, db

        if self.side_stream:
            main = torch.cuda.current_stream(x.device)
            st = ConvBackward._side_state(x.device)
            ready = torch.cuda.Event()
            ready.record(main)                           # x and g (the ReLU-masked gradient included) are complete in main's order here
            st[0].wait_event(ready)
            with torch.cuda.stream(st[0]):
                dw, db = wgrad()
                done = torch.cuda.Event()
                done.record(st[0])
                st[1] = done
            for t in (x, g):
                t.record_stream(st[0])                   # the caching allocator must not hand their memory out before the side launch ran
            dw.record_stream(main)
            db.record_stream(main)
        else:
            dw, db = wgrad()
        # `dx_res` (a second gradient of x: the skip connection's) and `dx_gate` (the ReLU output x came out of: its backward) ride
        # on the input-gradient convolution's epilogue: dx = relu'(dx_gate) * (conv(g) + dx_res) in one launch
        dx = None
        tail = dict(res=dx_res, res_mode=1 if dx_res is not None else 0, gate=dx_gate, **self._mk)
        if need_dx and self.same:
            dx = self._dgrad_conv()(g, N, H, W, **tail)
        elif need_dx and self.zero_insert:
            up = torch.zeros((N, H, W, c.Cout), dtype=torch.float32, device=x.device)
            up[:, ::c.stride, ::c.stride] = g
            dx = self._dgrad_conv()(up, N, H, W, **tail)
        elif need_dx:
            dx = torch.empty_like(x)
            check(self.lib.eod_conv2d_backward_input(g.data_ptr(), c.w.data_ptr(), c.Kpad, N, H, W, c.Cin, c.Cout, c.KH, c.KW, c.pad, c.stride,
                                                     dx.data_ptr(), _stream()), "eod_conv2d_backward_input")
            if dx_res is not None:
                dx = dx + dx_res
            if dx_gate is not None:
                gated = torch.empty_like(dx)
                check(self.lib.eod_relu_backward(dx.data_ptr(), dx_gate.data_ptr(), gated.data_ptr(), dx.numel(), _stream()), "eod_relu_backward")
                dx = gated
        return dict(dx=dx, dw=dw, db=db)


CENTERNET_SOI = ((0, 80), (64, 160), (128, 320), (256, 640), (512, 10000000))      # MODEL.CENTERNET.SOI


def centernet_targets(gt_boxes: torch.Tensor, level_hw: Sequence[Tuple[int, int]], strides: Sequence[int] = (8, 16, 32, 64, 128),
                      sizes_of_interest=CENTERNET_SOI, hm_min_overlap: float = 0.8, min_radius: float = 4.0):
    """CenterNet's target assignment for one image on the device (`eod_centernet_targets`; centernet.py:342-479) ->
    (agn_heatmap [P], reg_targets [P,4], pos_inds int32 [N * levels] of which counts[0] are valid, counts int32 [2] = positives,
    regression rows).  gt_boxes [N,4] float32 on the device."""
    _need_cuda(gt_boxes)
    dev = gt_boxes.device
    d = _lib.EodCenterNetTargetDesc()
    N, L = gt_boxes.shape[0], len(level_hw)
    off = [0]
    for (h, w) in level_hw:
        off.append(off[-1] + h * w)
    P = off[-1]
    d.gt_boxes, d.n_boxes, d.levels = (gt_boxes.data_ptr() if N else None), N, L
    for i, v in enumerate(off):
        d.level_off[i] = v
    for l in range(L):
        d.level_w[l], d.level_stride[l] = level_hw[l][1], strides[l]
        d.soi_lo[l], d.soi_hi[l] = float(sizes_of_interest[l][0]), float(sizes_of_interest[l][1])
    d.hm_min_overlap, d.min_radius = hm_min_overlap, min_radius
    heat = torch.empty((P,), dtype=torch.float32, device=dev)
    reg = torch.empty((P, 4), dtype=torch.float32, device=dev)
    pos = torch.zeros((max(N * L, 1),), dtype=torch.int32, device=dev)
    counts = torch.zeros((2,), dtype=torch.int32, device=dev)
    d.agn_heatmap, d.reg_targets, d.pos_inds, d.counts = heat.data_ptr(), reg.data_ptr(), pos.data_ptr(), counts.data_ptr()
    check(_lib.load().eod_centernet_targets(C.byref(d), _stream()), "eod_centernet_targets")
    return heat, reg, pos, counts


class CenterNetLoss:
    """`CenterNet.losses` of the recurrent configuration on the device with its gradient (`eod_centernet_loss`; centernet.py:241-318:
    agnostic heatmap focal loss + GIoU regression loss).  `__call__(head_out [P, stride], agn_heatmap [P], reg_targets [P,4],
    pos_inds int32 [N], num_pos_avg, reg_norm)` -> (losses [3] = loc, agn_pos, agn_neg on the device, dL/d(head_out)); the two norms are
    the all-reduced counts / world size the reference divides by (the caller reduces them over the ranks)."""

    def __init__(self, level_off: Sequence[int], level_scale: Sequence[float], device, head_stride: int = 8, alpha: float = 0.25,
                 beta: float = 4.0, gamma: float = 2.0, sigmoid_clamp: float = 1e-4, ignore_high_fp: float = 0.85,
                 pos_weight: float = 0.5, neg_weight: float = 0.5, reg_weight: float = 1.0):
        self.lib = _lib.load()
        d = _lib.EodCenterNetLossDesc()
        L = len(level_scale)
        assert len(level_off) == L + 1 and L <= 8
        d.head_stride, d.P, d.levels = head_stride, level_off[-1], L
        for i, v in enumerate(level_off):
            d.level_off[i] = v
        for i, v in enumerate(level_scale):
            d.level_scale[i] = float(v)
        d.hm_focal_alpha, d.hm_focal_beta, d.loss_gamma, d.sigmoid_clamp, d.ignore_high_fp = alpha, beta, gamma, sigmoid_clamp, ignore_high_fp
        d.pos_weight, d.neg_weight, d.reg_weight = pos_weight, neg_weight, reg_weight
        nbytes = self.lib.eod_centernet_loss_workspace_bytes()
        self.ws = torch.empty((nbytes // 8,), dtype=torch.float64, device=device)
        d.workspace, d.workspace_bytes = self.ws.data_ptr(), nbytes
        self.losses = torch.zeros((3,), dtype=torch.float32, device=device)
        d.losses = self.losses.data_ptr()
        self.desc = d

    def __call__(self, head_out: torch.Tensor, agn_heatmap: torch.Tensor, reg_targets: torch.Tensor, pos_inds: torch.Tensor,
                 num_pos_avg: float = 1.0, reg_norm: float = 1.0, out: Optional[torch.Tensor] = None, counts_local: Optional[torch.Tensor] = None,
                 counts_total: Optional[torch.Tensor] = None, world_size: int = 1):
        """`counts_local` / `counts_total` (int32 [2] on the device: `centernet_targets`' counts, the second all-reduced over the
        ranks): the positives' list length and the two normalisers are read on the device -- `pos_inds` is then the capacity-sized
        list and `num_pos_avg` / `reg_norm` are not used; no host round trip between the target assignment and the losses."""
        _need_cuda(head_out, agn_heatmap, reg_targets, pos_inds, out, counts_local, counts_total)
        d = self.desc
        assert tuple(head_out.shape) == (d.P, d.head_stride) and head_out.is_contiguous() and pos_inds.dtype == torch.int32
        assert tuple(reg_targets.shape) == (d.P, 4) and reg_targets.is_contiguous() and agn_heatmap.numel() == d.P
        if out is None:
            out = torch.empty_like(head_out)
        d.head_out, d.agn_heatmap, d.reg_targets = head_out.data_ptr(), agn_heatmap.data_ptr(), reg_targets.data_ptr()
        d.pos_inds, d.n_pos = (pos_inds.data_ptr() if pos_inds.numel() else None), pos_inds.numel()
        d.num_pos_avg, d.reg_norm, d.d_head_out = float(num_pos_avg), float(reg_norm), out.data_ptr()
        d.counts_local, d.counts_total, d.world_size = _ptr(counts_local), _ptr(counts_total), float(world_size)
        check(self.lib.eod_centernet_loss(C.byref(d), _stream()), "eod_centernet_loss")
        return self.losses, out


EOD_LOSS_FED = 1 << 30          # include/eod_hip.h
FED_MAX_C = 2047


def fed_loss_param_bytes(num_classes: int) -> int:
    """EOD_FED_LOSS_PARAM_BYTES of include/eod_hip.h."""
    return (16 + 12 * num_classes + 15) & ~15


class FedLossParams:
    """The federated loss's inputs as `eod_fast_rcnn_loss` reads them (`num_classes | EOD_LOSS_FED`): the parameter block at the head
    of a workspace this object owns.  `num_sample_cats`, `prob` [C] (None = ones: a uniform draw) and `zero_mask_src` [C] (None = no
    IGNORE_ZERO_CATS mask) are written once; `q` is the block's own [C] view, to be refilled in place before every call
    (`draw_q`: q ~ Exp(1), which makes the choice `torch.multinomial(prob, n, replacement=False)`)."""

    def __init__(self, num_classes: int, num_sample_cats: int, prob: Optional[torch.Tensor], zero_mask_src: Optional[torch.Tensor],
                 device):
        C = int(num_classes)
        if not 1 <= C <= FED_MAX_C:
            raise ValueError(f"federated loss: 1 .. {FED_MAX_C} classes, got {C}")
        if int(num_sample_cats) < 0:
            raise ValueError("FED_LOSS_NUM_CAT must not be negative")
        for name, t in (("prob", prob), ("zero_mask_src", zero_mask_src)):
            if t is not None and tuple(t.shape) != (C,):
                raise ValueError(f"federated loss: {name} must have one entry per class ({C}), got {tuple(t.shape)}")
        self.C, self.num_sample_cats, self.device = C, int(num_sample_cats), torch.device(device)
        self.head = fed_loss_param_bytes(C)
        self._rows = 0
        self._host = torch.zeros((self.head // 4,), dtype=torch.float32)
        self._host[:4].view(torch.int32).copy_(torch.tensor([self.num_sample_cats, int(prob is not None), int(zero_mask_src is not None), 0],
                                                            dtype=torch.int32))
        self._host[4:4 + C] = 1.0
        if prob is not None:
            self._host[4 + C:4 + 2 * C] = prob.detach().float().cpu()
        if zero_mask_src is not None:
            self._host[4 + 2 * C:4 + 3 * C] = zero_mask_src.detach().float().cpu()
        self.ws = None
        self.reserve(512)

    def reserve(self, B: int) -> None:
        """Room for the loss's own workspace of B rows behind the block."""
        if self.ws is not None and B <= self._rows:
            return
        n = self.head + int(_lib.load().eod_fast_rcnn_loss_workspace_bytes(B))
        q = None if self.ws is None else self.q.clone()
        self.ws = torch.empty((n // 4,), dtype=torch.float32, device=self.device)
        self.ws[:self.head // 4].copy_(self._host)
        self.q = self.ws[4:4 + self.C]
        if q is not None:
            self.q.copy_(q)
        self._rows = B

    def draw_q(self, generator: Optional[torch.Generator] = None) -> torch.Tensor:
        return self.q.exponential_(1.0, generator=generator)

    def set_q(self, q: torch.Tensor) -> None:
        self.q.copy_(q.to(self.device, torch.float32).view(self.C))


def fast_rcnn_loss(scores: torch.Tensor, deltas: torch.Tensor, proposal_boxes: torch.Tensor, gt_boxes: torch.Tensor,
                   gt_classes: torch.Tensor, num_classes: int, box_weights: Sequence[float], class_weight: Optional[torch.Tensor] = None,
                   smooth_l1_beta: float = 0.0, fed: Optional[FedLossParams] = None):
    """One cascade stage's `DeticFastRCNNOutputLayers.losses` (sigmoid CE + class-agnostic smooth-L1, detic_fast_rcnn.py:157-303) on the
    device -> (losses [2] = loss_cls, loss_box_reg; dL/d(scores) [B, ld]; dL/d(deltas) [B,4]).  gt_classes int32, background = C.

    `fed`: the federated loss (USE_FED_LOSS): the class weight is chosen on the device from `fed`'s block (its `q` as it stands)
    by one more launch in front of the loss, and returned as a fourth value ([C], 0 / 1)."""
    _need_cuda(scores, deltas, proposal_boxes, gt_boxes, gt_classes, class_weight)
    B, ld = scores.shape
    assert scores.is_contiguous() and tuple(deltas.shape) == (B, 4) and deltas.is_contiguous() and gt_classes.dtype == torch.int32
    lib = _lib.load()
    losses = torch.empty((2,), dtype=torch.float32, device=scores.device)
    ds, dd = torch.empty_like(scores), torch.empty_like(deltas)
    wx, wy, ww, wh = box_weights
    if fed is not None:
        if class_weight is not None or fed.C != num_classes:
            raise ValueError("fast_rcnn_loss: `fed` chooses the class weight itself, for its own number of classes")
        fed.reserve(B)
        class_weight = torch.empty((num_classes,), dtype=torch.float32, device=scores.device)
        ws, nbytes, flag = fed.ws, fed.ws.numel() * 4, EOD_LOSS_FED
    else:
        nbytes, flag = lib.eod_fast_rcnn_loss_workspace_bytes(B), 0
        ws = torch.empty((nbytes // 8,), dtype=torch.float64, device=scores.device)
    check(lib.eod_fast_rcnn_loss(scores.data_ptr(), ld, deltas.data_ptr(), proposal_boxes.data_ptr(), gt_boxes.data_ptr(),
                                 gt_classes.data_ptr(), _ptr(class_weight), B, num_classes | flag, wx, wy, ww, wh, smooth_l1_beta,
                                 ds.data_ptr(), dd.data_ptr(), losses.data_ptr(), ws.data_ptr(), nbytes, _stream()), "eod_fast_rcnn_loss")
    if fed is not None:
        return losses, ds, dd, class_weight
    return losses, ds, dd


def fed_loss_weight(gt_classes: torch.Tensor, num_classes: int, q: torch.Tensor, num_sample_cats: int,
                    prob: Optional[torch.Tensor] = None, zero_mask_src: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The federated loss's class weight alone ([C] of 0 / 1) for labels int32 [B] (background = C, -1 = no row) and the caller's
    `q` [C]: the launch lives on `eod_fast_rcnn_loss`, which is run here on zero scores.  Deterministic in its inputs; when fewer
    classes are eligible (not appeared, prob > 0) than are missing, all of them are taken (torch's CPU multinomial raises there)."""
    _need_cuda(gt_classes, q)
    B, dev = int(gt_classes.numel()), gt_classes.device
    fed = FedLossParams(num_classes, num_sample_cats, prob, zero_mask_src, dev)
    fed.set_q(q)
    z = torch.zeros((B, num_classes + 1), dtype=torch.float32, device=dev)
    box = torch.tensor([0.0, 0.0, 1.0, 1.0], device=dev).repeat(B, 1)
    return fast_rcnn_loss(z, torch.zeros((B, 4), device=dev), box, box, gt_classes.to(torch.int32).contiguous(), num_classes,
                          (1.0, 1.0, 1.0, 1.0), fed=fed)[3]


def match_label(boxes: torch.Tensor, gt_boxes: torch.Tensor, gt_classes: torch.Tensor, iou_thresh: float, num_classes: int):
    """detectron2's pairwise_iou + Matcher([iou_thresh], [0, 1]) + the labelling of `_sample_proposals` / `_match_and_label_boxes`
    (called at detic_roi_heads.py:232,115) -> (matched_idx int32 [R], matched_iou [R], classes int32 [R] with background =
    num_classes, matched gt boxes [R,4]).  gt_boxes [G,4] / gt_classes int32 [G]; G may be 0."""
    _need_cuda(boxes, gt_boxes, gt_classes)
    R, G = int(boxes.shape[0]), int(gt_boxes.shape[0])
    assert boxes.is_contiguous() and boxes.dtype == torch.float32 and tuple(boxes.shape) == (R, 4)
    assert gt_boxes.is_contiguous() and gt_boxes.dtype == torch.float32 and gt_classes.dtype == torch.int32 and gt_classes.numel() == G
    dev = boxes.device
    midx = torch.empty((R,), dtype=torch.int32, device=dev)
    miou = torch.empty((R,), dtype=torch.float32, device=dev)
    cls = torch.empty((R,), dtype=torch.int32, device=dev)
    gtb = torch.empty((R, 4), dtype=torch.float32, device=dev)
    check(_lib.load().eod_match_label(boxes.data_ptr(), R, gt_boxes.data_ptr() if G else None, gt_classes.data_ptr() if G else None, G,
                                      float(iou_thresh), num_classes, midx.data_ptr(), miou.data_ptr(), cls.data_ptr(), gtb.data_ptr(),
                                      _stream()), "eod_match_label")
    return midx, miou, cls, gtb


def match_label_proposals(prop_boxes: torch.Tensor, prop_count: torch.Tensor, gt_boxes: torch.Tensor, gt_classes: torch.Tensor,
                          iou_thresh: float, num_classes: int, append_gt: bool = True):
    """`match_label` on a capacity-sized proposal list whose length is on the device, the ground truth appended behind the live rows
    (detectron2's add_ground_truth_to_proposals) -> (all_boxes [cap + G, 4], classes int32 [cap + G] with -1 = no row, matched gt
    boxes): nothing is read back."""
    _need_cuda(prop_boxes, prop_count, gt_boxes, gt_classes)
    cap, G = int(prop_boxes.shape[0]), int(gt_boxes.shape[0])
    assert prop_boxes.is_contiguous() and prop_boxes.dtype == torch.float32 and prop_count.dtype == torch.int32
    assert gt_boxes.is_contiguous() and gt_boxes.dtype == torch.float32 and gt_classes.dtype == torch.int32 and gt_classes.numel() == G
    dev = prop_boxes.device
    R = cap + (G if append_gt else 0)
    allb = torch.empty((R, 4), dtype=torch.float32, device=dev)
    midx = torch.empty((R,), dtype=torch.int32, device=dev)
    miou = torch.empty((R,), dtype=torch.float32, device=dev)
    cls = torch.empty((R,), dtype=torch.int32, device=dev)
    gtb = torch.empty((R, 4), dtype=torch.float32, device=dev)
    check(_lib.load().eod_match_label_proposals(prop_boxes.data_ptr(), prop_count.data_ptr(), cap, gt_boxes.data_ptr() if G else None,
                                                gt_classes.data_ptr() if G else None, G, int(append_gt), float(iou_thresh), num_classes,
                                                allb.data_ptr(), midx.data_ptr(), miou.data_ptr(), cls.data_ptr(), gtb.data_ptr(), _stream()),
          "eod_match_label_proposals")
    return allb, cls, gtb


def sample_proposals(classes: torch.Tensor, keys: torch.Tensor, num_classes: int, batch_size_per_image: int, positive_fraction: float):
    """detectron2's `subsample_labels` as a selection by random keys (include/eod_hip.h) -> (sampled_idx int32 [batch], counts int32
    [2] = foreground rows, rows), both on the device."""
    _need_cuda(classes, keys)
    R = int(classes.numel())
    assert classes.dtype == torch.int32 and keys.dtype == torch.float32 and keys.numel() == R
    idx = torch.zeros((batch_size_per_image,), dtype=torch.int32, device=classes.device)
    counts = torch.zeros((2,), dtype=torch.int32, device=classes.device)
    # the ABI takes the fraction as a float; hand over the mid-point of the bucket of detectron2's `int(batch * fraction)` (a double
    # product) so that the float product truncates to the same count for every fraction (0.7 x 10 is 7 in double and 6.9999999 in float)
    max_pos = int(batch_size_per_image * positive_fraction)
    fraction = min((max_pos + 0.5) / batch_size_per_image, 1.0)
    st = _lib.load().eod_sample_proposals(classes.data_ptr(), keys.data_ptr(), R, num_classes, batch_size_per_image,
                                          float(fraction), idx.data_ptr(), counts.data_ptr(), _stream())
    if st == -5:
        raise _lib.EodError(f"eod_sample_proposals: {R} proposals exceed the sampling kernel's capacity of 8192 rows")
    check(st, "eod_sample_proposals")
    return idx, counts


def zs_logits(feat: torch.Tensor, zs: torch.Tensor, temp: float = 50.0, ld: Optional[int] = None, featn_out: Optional[torch.Tensor] = None):
    """The training-mode scores of DeticFastRCNNOutputLayers.forward: temp * normalize(feat [B,512]) @ zs [512,C1] -> logits [B, ld]."""
    _need_cuda(feat, zs, featn_out)
    B, C1 = int(feat.shape[0]), int(zs.shape[1])
    feat = feat.view(B, 512)
    assert feat.is_contiguous() and zs.is_contiguous() and int(zs.shape[0]) == 512
    ld = C1 if ld is None else ld
    out = torch.zeros((B, ld), dtype=torch.float32, device=feat.device)
    check(_lib.load().eod_zs_logits(feat.data_ptr(), zs.data_ptr(), B, 512, C1, float(temp), out.data_ptr(), ld, _ptr(featn_out),
                                    _stream()), "eod_zs_logits")
    return out


def zs_logits_backward(feat: torch.Tensor, zs: torch.Tensor, d_logits: torch.Tensor, temp: float = 50.0) -> torch.Tensor:
    """d feat [B,512] of `zs_logits` given d_logits [B, ld] (`eod_zs_logits_backward`)."""
    _need_cuda(feat, zs, d_logits)
    B, C1 = int(d_logits.shape[0]), int(zs.shape[1])
    feat = feat.view(B, 512)
    assert feat.is_contiguous() and d_logits.is_contiguous() and d_logits.shape[1] >= C1
    out = torch.empty((B, 512), dtype=torch.float32, device=feat.device)
    check(_lib.load().eod_zs_logits_backward(feat.data_ptr(), zs.data_ptr(), d_logits.data_ptr(), int(d_logits.shape[1]), B, 512, C1,
                                             float(temp), out.data_ptr(), _stream()), "eod_zs_logits_backward")
    return out


class AdamW:
    """`torch.optim.AdamW` (single-tensor form) + detectron2's clip-by-value on the device, one `eod_adamw_step` launch per parameter
    tensor: the optimizer of the reference's training configuration (custom_solver.py:69-72, Base-...recurrent.yaml:68-74).
    `groups`: what `solver.build_param_groups` returns (each with its own `lr`); state = exp_avg / exp_avg_sq per tensor."""

    def __init__(self, groups, betas=(0.9, 0.999), eps: float = 1e-8, weight_decay: float = 1e-2, clip_value: float = 0.0):
        self.groups = groups
        self.betas, self.eps, self.weight_decay, self.clip_value = betas, eps, weight_decay, clip_value
        self.state = [(torch.zeros_like(g["param"]), torch.zeros_like(g["param"])) for g in groups]
        self.steps = [0] * len(groups)
        self.lib = _lib.load()
        # all tensors in ceil(n / 20) launches (`eod_adamw_step_multi`); False: one `eod_adamw_step` launch per tensor (the same
        # arithmetic element for element: tests/test_backward_gpu.py compares the two)
        self.multi_tensor = True
        self._descs = (_lib.EodAdamWTensor * max(len(groups), 1))()

    def state_dict(self) -> Dict:
        """{parameter name: {'step', 'exp_avg', 'exp_avg_sq'}} on the host -- what DetectionCheckpointer stores for the optimizer
        (train_mp3d.py:521-523), keyed by the reference's parameter names instead of torch's positional ids."""
        return {g["name"]: {"step": self.steps[i], "exp_avg": self.state[i][0].cpu(), "exp_avg_sq": self.state[i][1].cpu()}
                for i, g in enumerate(self.groups)}

    def load_state_dict(self, sd: Dict) -> None:
        missing = [g["name"] for g in self.groups if g["name"] not in sd]
        if missing:
            raise KeyError(f"optimizer state without {len(missing)} of this model's parameters (first: {missing[0]})")
        for i, g in enumerate(self.groups):
            e = sd[g["name"]]
            if tuple(e["exp_avg"].shape) != tuple(self.state[i][0].shape):
                raise ValueError(f"optimizer state of {g['name']}: shape {tuple(e['exp_avg'].shape)} != {tuple(self.state[i][0].shape)}")
            self.steps[i] = int(e["step"])
            self.state[i][0].copy_(e["exp_avg"])
            self.state[i][1].copy_(e["exp_avg_sq"])

    def step(self, grads: Sequence[Optional[torch.Tensor]], lr_factor: float = 1.0, inv_scale: Optional[Sequence[float]] = None,
             found_inf: Optional[torch.Tensor] = None):
        """`grads[i]`: gradient of group i's tensor (None: no gradient this iteration, the tensor is skipped as torch does).
        `inv_scale[i]` (0 = off): the gradient is multiplied by it inside the launch, before the fold's chain rule and the clipping
        (a loss scaler's unscale); `found_inf` (device int32 [1]): the launch leaves everything untouched when it is non-zero.  The
        step COUNTS are advanced here either way: a caller that skips takes them back with `rewind(grads)`."""
        if (inv_scale is not None or found_inf is not None) and not self.multi_tensor:
            raise ValueError("inv_scale / found_inf ride on the multi-tensor launch (multi_tensor = True)")
        if self.multi_tensor:
            n = 0
            for i, (g, grad) in enumerate(zip(self.groups, grads)):
                if grad is None:
                    continue
                p = g["param"]
                _need_cuda(p, grad)
                assert p.dtype == torch.float32 and grad.dtype == torch.float32 and p.is_contiguous() and grad.is_contiguous()
                assert grad.shape == p.shape
                self.steps[i] += 1
                d = self._descs[n]
                d.param, d.grad, d.exp_avg, d.exp_avg_sq = p.data_ptr(), grad.data_ptr(), self.state[i][0].data_ptr(), self.state[i][1].data_ptr()
                d.n, d.lr, d.weight_decay, d.step = p.numel(), g["lr"] * lr_factor, g.get("weight_decay", self.weight_decay), self.steps[i]
                fold = g.get("fold")              # (folded weights [rows, ld], per-row scale [rows]): written by the same launch
                if fold is not None:
                    d.folded_out, d.row_scale, d.cols, d.ld_out = fold[0].data_ptr(), fold[1].data_ptr(), p.shape[1], fold[0].stride(0)
                    # `grads[i]` is the gradient of the folded weights: x scale inside the launch (group key "grad_of_folded")
                    d.grad_of_folded = 1 if g.get("grad_of_folded") else 0
                else:
                    d.folded_out, d.row_scale, d.cols, d.ld_out, d.grad_of_folded = None, None, 0, 0, 0
                d.inv_scale = 0.0 if inv_scale is None else float(inv_scale[i])
                d.found_inf = _ptr(found_inf)
                n += 1
            if n:
                check(self.lib.eod_adamw_step_multi(self._descs, n, self.betas[0], self.betas[1], self.eps, self.clip_value, _stream()),
                      "eod_adamw_step_multi")
            return
        for i, (g, grad) in enumerate(zip(self.groups, grads)):
            if grad is None:
                continue
            p = g["param"]
            _need_cuda(p, grad)
            assert p.dtype == torch.float32 and grad.dtype == torch.float32 and p.is_contiguous() and grad.is_contiguous()
            assert grad.shape == p.shape
            self.steps[i] += 1
            m, v = self.state[i]
            if g.get("fold") is not None and g.get("grad_of_folded"):
                grad = grad * g["fold"][1].view(-1, 1)
            check(self.lib.eod_adamw_step(p.data_ptr(), grad.data_ptr(), m.data_ptr(), v.data_ptr(), p.numel(), g["lr"] * lr_factor,
                                          self.betas[0], self.betas[1], self.eps, g.get("weight_decay", self.weight_decay), self.steps[i],
                                          self.clip_value, _stream()), "eod_adamw_step")
            if g.get("fold") is not None:
                g["fold"][0][:, :p.shape[1]].copy_(p * g["fold"][1].view(-1, 1))


    def rewind(self, grads: Sequence[Optional[torch.Tensor]]) -> None:
        """Takes back the step counts of a `step(grads, found_inf=...)` whose launch skipped itself (the flag was set)."""
        for i, grad in enumerate(grads):
            if grad is not None:
                self.steps[i] -= 1

    def nonfinite(self, grads: Sequence[Optional[torch.Tensor]], flag: torch.Tensor) -> None:
        """The loss scaler's found-inf pass: `flag` (device int32 [1], zeroed by the caller) becomes 1 when any element of any
        gradient is inf or NaN -- the check entries of `eod_adamw_step_multi`, ceil(n / 32) launches, nothing read back."""
        live = [g for g in grads if g is not None]
        if not live:
            return
        descs = (_lib.EodAdamWTensor * len(live))()
        for d, g in zip(descs, live):
            _need_cuda(g)
            assert g.dtype == torch.float32 and g.is_contiguous()
            d.grad, d.n, d.found_inf = g.data_ptr(), g.numel(), flag.data_ptr()
        check(self.lib.eod_adamw_step_multi(descs, len(live), self.betas[0], self.betas[1], self.eps, 0.0, _stream()), "eod_adamw_step_multi[check]")


class LossScaler:
    """`torch.amp.GradScaler`'s scale schedule on the host (train_mp3d.py:577-578,628-631): the scale starts at `init_scale`, a step
    whose gradients held an inf / NaN multiplies it by `backoff_factor` (and is skipped by the caller), `growth_interval` clean steps
    in a row multiply it by `growth_factor`.  `state_dict` uses torch's key names, so the two load each other's."""

    def __init__(self, init_scale: float = 65536.0, growth_factor: float = 2.0, backoff_factor: float = 0.5, growth_interval: int = 2000,
                 enabled: bool = True):
        if growth_factor <= 1.0 or not (0.0 < backoff_factor < 1.0):
            raise ValueError("growth_factor > 1 and 0 < backoff_factor < 1 (torch.amp.GradScaler)")
        # fp32 like torch's device scalar: the products below round as `_amp_update_scale_` does
        self._scale = float(np.float32(init_scale))
        self.growth_factor, self.backoff_factor, self.growth_interval = float(growth_factor), float(backoff_factor), int(growth_interval)
        self._growth_tracker = 0
        self.enabled = bool(enabled)
        self.skipped = 0                 # steps skipped so far (reporting)

    def get_scale(self) -> float:
        return self._scale if self.enabled else 1.0

    def update(self, found_inf: bool) -> None:
        """`scaler.update()` after a step whose found-inf pass returned `found_inf` (`_amp_update_scale_`)."""
        if not self.enabled:
            return
        if found_inf:
            self._scale = float(np.float32(self._scale) * np.float32(self.backoff_factor))
            self._growth_tracker = 0
            self.skipped += 1
            return
        self._growth_tracker += 1
        if self._growth_tracker == self.growth_interval:
            with np.errstate(over="ignore"):
                grown = np.float32(self._scale) * np.float32(self.growth_factor)
            if np.isfinite(grown):                      # torch keeps the old scale when the growth would overflow fp32
                self._scale = float(grown)
            self._growth_tracker = 0

    def state_dict(self) -> Dict:
        if not self.enabled:
            return {}
        return {"scale": self._scale, "growth_factor": self.growth_factor, "backoff_factor": self.backoff_factor,
                "growth_interval": self.growth_interval, "_growth_tracker": self._growth_tracker}

    def load_state_dict(self, sd: Dict) -> None:
        if not self.enabled:
            return
        if not sd:
            raise RuntimeError("the loss scaler's state is empty (saved by a disabled scaler)")
        self._scale = float(np.float32(sd["scale"]))
        self.growth_factor, self.backoff_factor = float(sd["growth_factor"]), float(sd["backoff_factor"])
        self.growth_interval, self._growth_tracker = int(sd["growth_interval"]), int(sd["_growth_tracker"])


class MemoryWriter:
    """a16-a19 write path (custom_rcnn.py:681-760) on device."""

    def __init__(self, H: int, W: int, n_cells: int, K_cap: int, R_cap: int, device, mask_thresh: float = 0.5, batch: int = 1):
        """`batch` > 1: B scenes with B independent states; every buffer handed to the call is B single-scene buffers back to back."""
        self.lib = _lib.load()
        nbytes = self.lib.eod_memory_write_workspace_bytes(H, W, 512, n_cells, K_cap, R_cap) * batch
        self.ws = torch.empty((nbytes,), dtype=torch.uint8, device=device)
        check(self.lib.eod_memory_write_init(self.ws.data_ptr(), nbytes, H, W, 512, n_cells, K_cap, R_cap, _stream()), "eod_memory_write_init")
        self.k_out = torch.zeros((batch,), dtype=torch.int32, device=device)
        d = EodMemWriteDesc()
        d.batch = batch
        d.K_cap, d.R_cap, d.H, d.W, d.D, d.n_cells, d.mask_thresh = K_cap, R_cap, H, W, 512, n_cells, mask_thresh
        d.workspace, d.workspace_bytes, d.k_out = self.ws.data_ptr(), nbytes, self.k_out.data_ptr()
        self.desc = d

    def __call__(self, featn, prop_boxes, prop_masks, det_rows, det_count, proj, mem, obs, dirty=None, err=None, snapshot=None):
        """`snapshot` (fp16 [N,512], the table `memory_gather_pool` reads): refreshed in place for every cell whose observation
        count changes (then `dirty` is not written); `dirty` alone: those cells are only marked for `memory_normalize_dirty_f16`."""
        d = self.desc
        d.dirty, d.err_flags, d.snapshot_f16 = _ptr(dirty), _ptr(err), _ptr(snapshot)
        d.featn, d.prop_boxes, d.prop_masks = featn.data_ptr(), prop_boxes.data_ptr(), prop_masks.data_ptr()
        d.det_rows, d.det_count, d.proj, d.mem, d.obs = det_rows.data_ptr(), det_count.data_ptr(), proj.data_ptr(), mem.data_ptr(), obs.data_ptr()
        check(self.lib.eod_memory_write(C.byref(d), _stream()), "eod_memory_write")
        return self.k_out


def semmap_labels(mem: torch.Tensor, obs: torch.Tensor, zs: torch.Tensor, thresh: float) -> torch.Tensor:
    """a20 (custom_rcnn.py:745-756,938-1017): int32 [N] labels, -1 below the observation-intensity threshold."""
    N, D = mem.shape
    labels = torch.empty((N,), dtype=torch.int32, device=mem.device)
    ws = torch.empty((N + 4,), dtype=torch.float32, device=mem.device)
    check(_lib.load().eod_semmap_labels(mem.data_ptr(), obs.data_ptr(), zs.data_ptr(), N, D, zs.shape[1], thresh, labels.data_ptr(),
                                        ws.data_ptr(), _stream()), "eod_semmap_labels")
    return labels


def semmap_query(mem: torch.Tensor, obs: torch.Tensor, zs: torch.Tensor, thresh: float):
    """The map in any vocabulary the heads accept (EOD_SEMMAP_SCORES; `zs` [512, C1], C1 <= 2048, on the fp32 matrix cores):
    (labels int32 [N] as `semmap_labels` defines them, scores float32 [N]: the softmax probability of the cell's argmax class over
    the first C1-1 columns, for every cell, thresholded or not).  `scores` is a view into the call's workspace."""
    N, D = mem.shape
    if zs.dim() != 2 or zs.shape[0] != 512 or not zs.is_contiguous() or zs.dtype != torch.float32:
        raise _lib.EodError(f"semmap_query: class matrix {tuple(zs.shape)} {zs.dtype}: expected contiguous float32 [512, C1]")
    C1 = int(zs.shape[1])
    if C1 > ZS_WIDE_MAX_C1:
        raise _lib.EodError(f"semmap_query: {C1 - 1} classes + background exceed the kernel's {ZS_WIDE_MAX_C1} columns")
    labels = torch.empty((N,), dtype=torch.int32, device=mem.device)
    ws = torch.empty((2 * N + 4,), dtype=torch.float32, device=mem.device)
    check(_lib.load().eod_semmap_labels(mem.data_ptr(), obs.data_ptr(), zs.data_ptr(), N, D | _lib.SEMMAP_SCORES, C1, thresh,
                                        labels.data_ptr(), ws.data_ptr(), _stream()), "eod_semmap_labels")
    return labels, ws[4 + N:]


SEMMAP_LOCATE_MAX_Q, SEMMAP_LOCATE_MAX_K, SEMMAP_LOCATE_MAX_RADIUS = 32, 16, 3


def semmap_locate_workspace(N: int, Q: int, K: int) -> int:
    """Floats of a `semmap_locate` workspace (EOD_SEMMAP_LOCATE_FLOATS): the SCORES call's 4 + 2 N, 32 query indices, prob [Q, N],
    the peak step's candidates [Q, N], peaks and peak_scores [Q, K]."""
    return 4 + 2 * N + 32 + 2 * Q * N + 2 * Q * K


def semmap_locate(mem: torch.Tensor, obs: torch.Tensor, zs: torch.Tensor, classes, thresh: float, cols: Optional[int] = None,
                  radius: int = 1, topk: int = 8, workspace: Optional[torch.Tensor] = None) -> dict:
    """Where on the map the queried classes are (EOD_SEMMAP_LOCATE, then EOD_SEMMAP_PEAKS on the same workspace).  `classes`: Q
    class indices (1 <= Q <= 32, each in [0, C1-2], duplicates allowed), a sequence or an integer tensor.  Returns
      labels int32 [N], scores float32 [N]     what `semmap_query` returns, bit for bit
      prob float32 [Q, N]                      the softmax probability of class q in cell i over the whole vocabulary; 0 where the
                                               threshold labels the cell -1
      peaks int32 [Q, topk], peak_scores       the best local maxima of each map by (prob descending, cell ascending), padded with
                                               (-1, 0.0): cell i = r * cols + c is a peak iff prob > 0 and no cell of its
                                               (2 radius + 1)^2 window, clipped at the edge, has a larger value or an equal value
                                               and a lower index.  `cols=None`: the plain top-k of the positive cells (radius 0).
    Everything but `labels` is a view into the workspace (`workspace`: float32, at least `semmap_locate_workspace(N, Q, topk)`)."""
    N, D = mem.shape
    if zs.dim() != 2 or zs.shape[0] != 512 or not zs.is_contiguous() or zs.dtype != torch.float32:
        raise _lib.EodError(f"semmap_locate: class matrix {tuple(zs.shape)} {zs.dtype}: expected contiguous float32 [512, C1]")
    C1 = int(zs.shape[1])
    if C1 > ZS_WIDE_MAX_C1:
        raise _lib.EodError(f"semmap_locate: {C1 - 1} classes + background exceed the kernel's {ZS_WIDE_MAX_C1} columns")
    if isinstance(classes, torch.Tensor):
        if classes.dim() != 1 or classes.dtype.is_floating_point or classes.dtype == torch.bool:
            raise _lib.EodError(f"semmap_locate: classes {tuple(classes.shape)} {classes.dtype}: expected a 1-d integer tensor")
        classes = classes.tolist()
    classes = [int(c) for c in classes]
    Q, K = len(classes), int(topk)
    if not 1 <= Q <= SEMMAP_LOCATE_MAX_Q:
        raise _lib.EodError(f"semmap_locate: {Q} queried classes; one call takes 1 to {SEMMAP_LOCATE_MAX_Q}")
    bad = [c for c in classes if not 0 <= c <= C1 - 2]
    if bad:
        raise _lib.EodError(f"semmap_locate: class indices {bad} outside [0, {C1 - 2}] (column {C1 - 1} is the background)")
    if not 1 <= K <= SEMMAP_LOCATE_MAX_K:
        raise _lib.EodError(f"semmap_locate: topk {topk} outside 1..{SEMMAP_LOCATE_MAX_K}")
    if cols is None:
        cols, radius = N, 0
    cols, radius = int(cols), int(radius)
    if not 0 <= radius <= SEMMAP_LOCATE_MAX_RADIUS:
        raise _lib.EodError(f"semmap_locate: radius {radius} outside 0..{SEMMAP_LOCATE_MAX_RADIUS}")
    if cols < 1 or N % cols != 0:
        raise _lib.EodError(f"semmap_locate: {N} cells are no whole number of rows of {cols}")
    need = semmap_locate_workspace(N, Q, K)
    if workspace is None:
        workspace = torch.empty((need,), dtype=torch.float32, device=mem.device)
    elif (workspace.dtype != torch.float32 or workspace.dim() != 1 or not workspace.is_contiguous() or workspace.numel() < need
          or workspace.device != mem.device):
        raise _lib.EodError(f"semmap_locate: workspace {tuple(workspace.shape)} {workspace.dtype}: expected {need} contiguous float32 "
                            "on the memory's device")
    ws = workspace
    q0, p0 = 4 + 2 * N, 4 + 2 * N + 32
    ws[q0:q0 + Q].view(torch.int32).copy_(torch.tensor(classes, dtype=torch.int32), non_blocking=False)
    labels = torch.empty((N,), dtype=torch.int32, device=mem.device)
    lib, qbits = _lib.load(), Q << _lib.SEMMAP_Q_SHIFT
    check(lib.eod_semmap_labels(mem.data_ptr(), obs.data_ptr(), zs.data_ptr(), N, D | _lib.SEMMAP_LOCATE | qbits, C1, thresh,
                                labels.data_ptr(), ws.data_ptr(), _stream()), "eod_semmap_labels")
    pbits = _lib.SEMMAP_PEAKS | qbits | (K - 1) << _lib.SEMMAP_K_SHIFT | radius << _lib.SEMMAP_RADIUS_SHIFT
    check(lib.eod_semmap_labels(mem.data_ptr(), obs.data_ptr(), zs.data_ptr(), N, D | pbits, cols, thresh, labels.data_ptr(),
                                ws.data_ptr(), _stream()), "eod_semmap_labels")
    k0 = p0 + 2 * Q * N
    return {"labels": labels, "scores": ws[4 + N:4 + 2 * N], "prob": ws[p0:p0 + Q * N].view(Q, N),
            "peaks": ws[k0:k0 + Q * K].view(torch.int32).view(Q, K), "peak_scores": ws[k0 + Q * K:k0 + 2 * Q * K].view(Q, K)}


PLACE_TOPK_MAX, PLACE_TABLE_LOG2_MIN, PLACE_TABLE_LOG2_MAX, PLACE_TABLE_LOG2 = 8, 4, 12, 12     # EOD_PLACE_* of include/eod_place.h


def place_masks_workspace(K_cap: int, n_cells: int) -> int:
    """int32 words of a `place_masks` workspace (eod_place_masks_workspace_bytes / 4): the overflow list and the four dense
    [n_cells] tables of the overflow kernel.  It does not grow with K_cap * n_cells."""
    if K_cap < 0 or n_cells < 1:
        raise _lib.EodError(f"place_masks_workspace: K_cap {K_cap}, n_cells {n_cells}")
    return int(_lib.load().eod_place_masks_workspace_bytes(int(K_cap), int(n_cells))) // 4


def place_masks(masks: torch.Tensor, proj: torch.Tensor, n_cells: int, count: Optional[torch.Tensor] = None,
                rects: Optional[torch.Tensor] = None, topk: int = 4, exclude_cell: int = -1, table_log2: Optional[int] = None,
                workspace: Optional[torch.Tensor] = None) -> dict:
    """The grid cells under each instance mask (eod_place_masks; the semantics are those of include/eod_place.h).  `masks` [K_cap, H, W] uint8 or
    bool, `proj` [H, W] int32, `count` a device int32 (rows beyond it come back as padding; None: all rows), `rects` int32
    [K_cap, 4] half-open (x0, y0, x1, y1) outside which a mask is not read (None: the image).  Returns int32 tensors, views of
    one buffer: `mask_pixels`, `pixels`, `invalid`, `distinct` [K_cap], `cells` and `cell_pixels` [K_cap, topk] (the cells with
    the most pixels by count descending, cell ascending; padded with -1 / 0).  Pixels whose cell is `exclude_cell` are dropped;
    cells outside [0, n_cells) are counted as `invalid` and never used.  `table_log2` (4..12, None: 12) sizes the kernel's hash
    table and changes nothing in the result; `workspace`: int32, at least `place_masks_workspace(K_cap, n_cells)` words, any
    contents."""
    if not isinstance(masks, torch.Tensor) or masks.dim() != 3 or masks.dtype not in (torch.uint8, torch.bool) or not masks.is_contiguous():
        raise _lib.EodError(f"place_masks: masks {tuple(getattr(masks, 'shape', ()))} {getattr(masks, 'dtype', type(masks))}: "
                            "expected contiguous uint8 or bool [K, H, W]")
    if not masks.is_cuda:
        raise _lib.EodError("place_masks: masks on the host (no CPU fallback)")
    K_cap, H, W = (int(v) for v in masks.shape)
    dev = masks.device
    if (not isinstance(proj, torch.Tensor) or proj.dtype != torch.int32 or tuple(proj.shape) != (H, W) or not proj.is_contiguous()
            or proj.device != dev):
        raise _lib.EodError(f"place_masks: proj {tuple(getattr(proj, 'shape', ()))} {getattr(proj, 'dtype', type(proj))}: expected "
                            f"contiguous int32 [{H}, {W}] on the masks' device")
    n_cells, T, exclude_cell = int(n_cells), int(topk), int(exclude_cell)
    if n_cells < 1:
        raise _lib.EodError(f"place_masks: n_cells {n_cells}")
    if H < 1 or W < 1 or H * W > 2 ** 31 - 5:
        raise _lib.EodError(f"place_masks: image {H} x {W}")
    if not 1 <= T <= PLACE_TOPK_MAX:
        raise _lib.EodError(f"place_masks: topk {topk} outside 1..{PLACE_TOPK_MAX}")
    if not -2 ** 31 <= exclude_cell < 2 ** 31:
        raise _lib.EodError(f"place_masks: exclude_cell {exclude_cell}")
    log2 = PLACE_TABLE_LOG2 if table_log2 is None else int(table_log2)
    if not PLACE_TABLE_LOG2_MIN <= log2 <= PLACE_TABLE_LOG2_MAX:
        raise _lib.EodError(f"place_masks: table_log2 {table_log2} outside {PLACE_TABLE_LOG2_MIN}..{PLACE_TABLE_LOG2_MAX}")
    if count is not None and (not isinstance(count, torch.Tensor) or count.dtype != torch.int32 or count.numel() != 1 or count.device != dev):
        raise _lib.EodError("place_masks: count: expected one int32 on the masks' device")
    if rects is not None and (not isinstance(rects, torch.Tensor) or rects.dtype != torch.int32 or tuple(rects.shape) != (K_cap, 4)
                              or not rects.is_contiguous() or rects.device != dev):
        raise _lib.EodError(f"place_masks: rects: expected contiguous int32 [{K_cap}, 4] on the masks' device")
    need = place_masks_workspace(K_cap, n_cells)
    if workspace is not None and (not isinstance(workspace, torch.Tensor) or workspace.dtype != torch.int32 or workspace.dim() != 1
                                  or not workspace.is_contiguous() or workspace.numel() < need or workspace.device != dev):
        raise _lib.EodError(f"place_masks: workspace: expected {need} contiguous int32 on the masks' device")
    out = torch.empty(((4 + 2 * T) * K_cap,), dtype=torch.int32, device=dev)
    if K_cap > 0:
        if workspace is None:
            workspace = torch.empty((need,), dtype=torch.int32, device=dev)
        check(_lib.load().eod_place_masks(masks.data_ptr(), proj.data_ptr(), _ptr(count), _ptr(rects), K_cap, H, W, n_cells, T,
                                          exclude_cell, log2, out.data_ptr(), workspace.data_ptr(), workspace.numel() * 4, _stream()),
              "eod_place_masks")
    stats = out[:4 * K_cap].view(4, K_cap)
    return {"mask_pixels": stats[0], "pixels": stats[1], "invalid": stats[2], "distinct": stats[3],
            "cells": out[4 * K_cap:(4 + T) * K_cap].view(K_cap, T), "cell_pixels": out[(4 + T) * K_cap:].view(K_cap, T)}


# EOD_REGIONS_* of include/eod_regions.h
REGIONS_Q_MAX, REGIONS_TOPK_MAX, REGIONS_N_MAX, REGIONS_TILE_ROWS, REGIONS_TILE_COLS = 32, 64, 1 << 22, 32, 32


def map_regions_workspace(Q: int, N: int, topk: int) -> int:
    """int32 words of a `map_regions` workspace (eod_map_regions_workspace_bytes / 4): three [Q, N] arrays and Q * topk peak keys."""
    need = int(_lib.load().eod_map_regions_workspace_bytes(int(Q), int(N), int(topk)))
    if need == 0:
        raise _lib.EodError(f"map_regions_workspace: Q {Q}, N {N}, topk {topk}")
    return need // 4


def map_regions(prob: torch.Tensor, cols: int, level: float, connectivity: int = 8, min_cells: int = 1, topk: int = 16,
                workspace: Optional[torch.Tensor] = None) -> dict:
    """The connected regions of each class of a map, ranked by size (eod_map_regions; the semantics are those of
    include/eod_regions.h).  `prob` [Q, N] float32 (the `prob` of `semmap_locate`, or any map), cell i = r * cols + c; the foreground
    of a class is `prob >= level`, two cells are neighbours under `connectivity` 4 or 8 on the grid, a component's label is its
    smallest cell.  Returns `region_labels` int32 [Q, N] (-1: background), `count` and `foreground` int32 [Q], `status` int32 [1]
    (nonzero: a kernel's bounded loop reached its bound; not read here, so nothing synchronises) and, per class for the `topk`
    components of at least `min_cells` cells by (area descending, label ascending), padded with region -1 and zeros: `region`, `area`,
    `peak` int32 [Q, K], `peak_prob` float32 [Q, K], `bbox` int32 [Q, K, 4] (r0, c0, r1, c1 inclusive), `sum_rc` int64 [Q, K, 2],
    `mass_q24` int64 [Q, K].  All but `region_labels` are views of one buffer.  `workspace`: int32, 8-byte aligned, at least
    `map_regions_workspace(Q, N, topk)` words, any contents."""
    if (not isinstance(prob, torch.Tensor) or prob.dim() != 2 or prob.dtype != torch.float32 or not prob.is_contiguous()):
        raise _lib.EodError(f"map_regions: prob {tuple(getattr(prob, 'shape', ()))} {getattr(prob, 'dtype', type(prob))}: expected "
                            "contiguous float32 [Q, N]")
    Q, N = (int(v) for v in prob.shape)
    dev = prob.device
    if not 1 <= Q <= REGIONS_Q_MAX:
        raise _lib.EodError(f"map_regions: prob: Q {Q} outside 1..{REGIONS_Q_MAX}")
    if not 1 <= N <= REGIONS_N_MAX:
        raise _lib.EodError(f"map_regions: prob: N {N} outside 1..{REGIONS_N_MAX}")
    if isinstance(cols, bool) or int(cols) != cols or int(cols) < 1 or N % int(cols) != 0:
        raise _lib.EodError(f"map_regions: cols {cols} does not divide the {N} cells")
    level32 = float(torch.tensor(float(level), dtype=torch.float32))            # what the kernel compares against
    if not 0.0 < level32 <= 1.0:                                                 # a NaN and the infinities fail it
        raise _lib.EodError(f"map_regions: level {level} outside (0, 1]")
    if connectivity not in (4, 8):
        raise _lib.EodError(f"map_regions: connectivity {connectivity}: 4 or 8")
    if int(min_cells) != min_cells or int(min_cells) < 1 or int(min_cells) >= 2 ** 31:
        raise _lib.EodError(f"map_regions: min_cells {min_cells} below 1")
    if int(topk) != topk or not 1 <= int(topk) <= REGIONS_TOPK_MAX:
        raise _lib.EodError(f"map_regions: topk {topk} outside 1..{REGIONS_TOPK_MAX}")
    if not prob.is_cuda:
        raise _lib.EodError("map_regions: prob on the host (no CPU fallback)")
    K = int(topk)
    need = map_regions_workspace(Q, N, K)
    if workspace is not None and (not isinstance(workspace, torch.Tensor) or workspace.dtype != torch.int32 or workspace.dim() != 1
                                  or not workspace.is_contiguous() or workspace.numel() < need or workspace.device != dev
                                  or workspace.data_ptr() % 8 != 0):
        raise _lib.EodError(f"map_regions: workspace: expected {need} contiguous, 8-byte aligned int32 on the map's device")
    if workspace is None:
        workspace = torch.empty((need,), dtype=torch.int32, device=dev)
    labels = torch.empty((Q, N), dtype=torch.int32, device=dev)
    out = torch.empty((2 + 2 * Q + 14 * Q * K,), dtype=torch.int32, device=dev)
    check(_lib.load().eod_map_regions(prob.data_ptr(), Q, N, int(cols), level32, int(connectivity), int(min_cells), K, labels.data_ptr(),
                                      out.data_ptr(), workspace.data_ptr(), workspace.numel() * 4, _stream()), "eod_map_regions")
    b, QK = 2 + 2 * Q, Q * K
    return {"region_labels": labels, "status": out[:1], "count": out[2:2 + Q], "foreground": out[2 + Q:b],
            "region": out[b:b + QK].view(Q, K), "area": out[b + QK:b + 2 * QK].view(Q, K), "peak": out[b + 2 * QK:b + 3 * QK].view(Q, K),
            "peak_prob": out[b + 3 * QK:b + 4 * QK].view(torch.float32).view(Q, K), "bbox": out[b + 4 * QK:b + 8 * QK].view(Q, K, 4),
            "sum_rc": out[b + 8 * QK:b + 12 * QK].view(torch.int64).view(Q, K, 2),
            "mass_q24": out[b + 12 * QK:b + 14 * QK].view(torch.int64).view(Q, K)}


# EOD_INVENTORY_* of include/eod_inventory.h
INVENTORY_B_MAX, INVENTORY_C_MAX, INVENTORY_TOPK_MAX, INVENTORY_N_MAX = 32, 2047, 64, 1 << 22


def map_inventory_workspace(B: int, N: int, C: int, topk: int) -> int:
    """int32 words of a `map_inventory` workspace (eod_map_inventory_workspace_bytes / 4): three [B, N] arrays, B * topk peak keys and
    B * C class keys."""
    need = int(_lib.load().eod_map_inventory_workspace_bytes(int(B), int(N), int(C), int(topk)))
    if need == 0:
        raise _lib.EodError(f"map_inventory_workspace: B {B}, N {N}, C {C}, topk {topk}")
    return need // 4


def map_inventory(labels: torch.Tensor, scores: torch.Tensor, cols: int, num_classes: int, level: float = 0.5, connectivity: int = 8,
                  min_cells: int = 1, topk: int = 16, keep: Optional[torch.Tensor] = None,
                  workspace: Optional[torch.Tensor] = None) -> dict:
    """Every object of a label map, all classes in one call (eod_map_inventory; the semantics are those of
    include/eod_inventory.h).  `labels` int32 and `scores` float32, [N] or [B, N] (what `semmap_query` returns, or any label map),
    cell i = r * cols + c.  A cell is foreground when 0 <= label < `num_classes`, `keep` (uint8 or bool [num_classes], None: every
    class) holds a nonzero for its label and its score is >= `level`; two foreground cells are neighbours under `connectivity` 4 or 8
    on the grid when they carry the same label; an object's label is its smallest cell.  `level = 2 ** -11` lies below any argmax
    probability of a vocabulary of up to 2047 classes (the largest of at most 2048 softmax terms is at least 1 / 2048), so it keeps
    every labelled cell.  Returns `object_labels` int32 (-1: background) in the shape of `labels`, `status` int32 [1] (nonzero: a
    kernel's bounded loop reached its bound; not read here, so nothing synchronises) and, with the leading [B] only for [B, N] maps:
    `count`, `foreground` int32 [B]; for the `topk` objects of at least `min_cells` cells by (area descending, label ascending) over
    all classes, padded with object -1, cls -1 and zeros: `object`, `cls`, `area`, `peak` int32 [B, K], `peak_score` float32 [B, K],
    `bbox` int32 [B, K, 4] (r0, c0, r1, c1 inclusive), `sum_rc` int64 [B, K, 2], `mass_q24` int64 [B, K]; and per class, int32
    [B, num_classes]: `class_objects` (objects of at least `min_cells` cells), `class_cells` (foreground cells, all of them),
    `class_largest` (the label of the class's first object in the same order, -1 for none), `class_largest_area`.  All but
    `object_labels` are views of one buffer.  `workspace`: int32, 8-byte aligned, at least
    `map_inventory_workspace(B, N, num_classes, topk)` words, any contents."""
    def is_map(t, dtype):
        return isinstance(t, torch.Tensor) and t.dim() in (1, 2) and t.dtype == dtype and t.is_contiguous()
    if not is_map(labels, torch.int32):
        raise _lib.EodError(f"map_inventory: labels {tuple(getattr(labels, 'shape', ()))} {getattr(labels, 'dtype', type(labels))}: expected "
                            "contiguous int32 [N] or [B, N]")
    if not is_map(scores, torch.float32) or scores.shape != labels.shape or scores.device != labels.device:
        raise _lib.EodError(f"map_inventory: scores {tuple(getattr(scores, 'shape', ()))} {getattr(scores, 'dtype', type(scores))}: expected "
                            f"contiguous float32 {tuple(labels.shape)} on the labels' device")
    single = labels.dim() == 1
    B, N = (1, int(labels.shape[0])) if single else (int(v) for v in labels.shape)
    dev = labels.device
    if not 1 <= B <= INVENTORY_B_MAX:
        raise _lib.EodError(f"map_inventory: labels: B {B} outside 1..{INVENTORY_B_MAX}")
    if not 1 <= N <= INVENTORY_N_MAX:
        raise _lib.EodError(f"map_inventory: labels: N {N} outside 1..{INVENTORY_N_MAX}")
    if isinstance(cols, bool) or int(cols) != cols or int(cols) < 1 or N % int(cols) != 0:
        raise _lib.EodError(f"map_inventory: cols {cols} does not divide the {N} cells")
    if isinstance(num_classes, bool) or int(num_classes) != num_classes or not 1 <= int(num_classes) <= INVENTORY_C_MAX:
        raise _lib.EodError(f"map_inventory: num_classes {num_classes} outside 1..{INVENTORY_C_MAX}")
    C = int(num_classes)
    level32 = float(torch.tensor(float(level), dtype=torch.float32))            # what the kernel compares against
    if not 0.0 < level32 <= 1.0:                                                 # a NaN and the infinities fail it
        raise _lib.EodError(f"map_inventory: level {level} outside (0, 1]")
    if connectivity not in (4, 8):
        raise _lib.EodError(f"map_inventory: connectivity {connectivity}: 4 or 8")
    if int(min_cells) != min_cells or int(min_cells) < 1 or int(min_cells) >= 2 ** 31:
        raise _lib.EodError(f"map_inventory: min_cells {min_cells} below 1")
    if int(topk) != topk or not 1 <= int(topk) <= INVENTORY_TOPK_MAX:
        raise _lib.EodError(f"map_inventory: topk {topk} outside 1..{INVENTORY_TOPK_MAX}")
    if keep is not None and (not isinstance(keep, torch.Tensor) or keep.dtype not in (torch.uint8, torch.bool) or tuple(keep.shape) != (C,)
                             or not keep.is_contiguous() or keep.device != dev):
        raise _lib.EodError(f"map_inventory: keep {tuple(getattr(keep, 'shape', ()))} {getattr(keep, 'dtype', type(keep))}: expected "
                            f"contiguous uint8 or bool [{C}] on the labels' device")
    K = int(topk)
    need = map_inventory_workspace(B, N, C, K)
    if workspace is not None and (not isinstance(workspace, torch.Tensor) or workspace.dtype != torch.int32 or workspace.dim() != 1
                                  or not workspace.is_contiguous() or workspace.numel() < need or workspace.device != dev
                                  or workspace.data_ptr() % 8 != 0):
        raise _lib.EodError(f"map_inventory: workspace: expected {need} contiguous, 8-byte aligned int32 on the maps' device")
    if not labels.is_cuda:
        raise _lib.EodError("map_inventory: labels on the host (no CPU fallback)")
    if workspace is None:
        workspace = torch.empty((need,), dtype=torch.int32, device=dev)
    object_labels = torch.empty_like(labels)
    out = torch.empty((2 + 2 * B + 15 * B * K + 4 * B * C,), dtype=torch.int32, device=dev)
    check(_lib.load().eod_map_inventory(labels.data_ptr(), scores.data_ptr(), _ptr(keep), B, N, int(cols), C, level32, int(connectivity),
                                        int(min_cells), K, object_labels.data_ptr(), out.data_ptr(), workspace.data_ptr(),
                                        workspace.numel() * 4, _stream()), "eod_map_inventory")
    s, BK, BC = 2 + 2 * B, B * K, B * C
    t = s + 15 * BK
    res = {"count": out[2:2 + B], "foreground": out[2 + B:s],
           "object": out[s:s + BK].view(B, K), "area": out[s + BK:s + 2 * BK].view(B, K), "peak": out[s + 2 * BK:s + 3 * BK].view(B, K),
           "peak_score": out[s + 3 * BK:s + 4 * BK].view(torch.float32).view(B, K), "bbox": out[s + 4 * BK:s + 8 * BK].view(B, K, 4),
           "sum_rc": out[s + 8 * BK:s + 12 * BK].view(torch.int64).view(B, K, 2),
           "mass_q24": out[s + 12 * BK:s + 14 * BK].view(torch.int64).view(B, K), "cls": out[s + 14 * BK:t].view(B, K),
           "class_objects": out[t:t + BC].view(B, C), "class_cells": out[t + BC:t + 2 * BC].view(B, C),
           "class_largest": out[t + 2 * BC:t + 3 * BC].view(B, C), "class_largest_area": out[t + 3 * BC:t + 4 * BC].view(B, C)}
    if single:
        res = {k: v[0] for k, v in res.items()}
    res["object_labels"] = object_labels
    res["status"] = out[:1]
    return res


DESCRIBE_D, DESCRIBE_K_MAX, DESCRIBE_N_MAX, DESCRIBE_C_MAX, DESCRIBE_TOPN_MAX = 512, 64, 1 << 22, 2047, 8


def _describe_what(t) -> str:
    return f"{tuple(getattr(t, 'shape', ()))} {getattr(t, 'dtype', type(t))}"


def describe_pool(mem: torch.Tensor, object_labels: torch.Tensor, objects: torch.Tensor) -> dict:
    """One CLIP-space direction per map object (eod_describe_pool; the semantics are those of include/eod_describe.h).  `mem`
    float32 [N, 512], the memory's sum rows; `object_labels` int32 [N], the `object_labels` of `map_inventory`, a row of the
    `region_labels` of `map_regions` or any other label map; `objects` int32 [K], 1 <= K <= 64, the labels to describe as
    `inv["object"]` holds them (-1 in unused slots).  A cell belongs to the lowest slot that names its label; cells in no slot are
    skipped and their rows are not read.  Returns `sum_q` int64 [K, 512] (the sum over the slot's cells of the normalised row in
    fixed point, truncated at 2^-30), `cells` int32 [K], `embedding` float32 [K, 512] (the unit mean direction; zeros for a slot
    without cells) and `coherence` float32 [K] (the length of the mean of the unit rows: 1 when all cells point the same way).
    Integer atomics only: the same bits on every call, whatever the order of the cells."""
    if not isinstance(mem, torch.Tensor) or mem.dim() != 2 or mem.shape[1] != DESCRIBE_D or mem.dtype != torch.float32 or not mem.is_contiguous():
        raise _lib.EodError(f"describe_pool: mem {_describe_what(mem)}: expected contiguous float32 [N, {DESCRIBE_D}]")
    N = int(mem.shape[0])
    if not 1 <= N <= DESCRIBE_N_MAX:
        raise _lib.EodError(f"describe_pool: mem: N {N} outside 1..{DESCRIBE_N_MAX}")
    if (not isinstance(object_labels, torch.Tensor) or tuple(object_labels.shape) != (N,) or object_labels.dtype != torch.int32
            or not object_labels.is_contiguous() or object_labels.device != mem.device):
        raise _lib.EodError(f"describe_pool: object_labels {_describe_what(object_labels)}: expected contiguous int32 [{N}] on the "
                            "memory's device")
    if (not isinstance(objects, torch.Tensor) or objects.dim() != 1 or objects.dtype != torch.int32 or not objects.is_contiguous()
            or objects.device != mem.device):
        raise _lib.EodError(f"describe_pool: objects {_describe_what(objects)}: expected contiguous int32 [K] on the memory's device")
    K = int(objects.shape[0])
    if not 1 <= K <= DESCRIBE_K_MAX:
        raise _lib.EodError(f"describe_pool: objects: K {K} outside 1..{DESCRIBE_K_MAX}")
    if mem.data_ptr() % 16 != 0:
        raise _lib.EodError("describe_pool: mem is not 16-byte aligned")
    if not mem.is_cuda:
        raise _lib.EodError("describe_pool: mem on the host (no CPU fallback)")
    dev = mem.device
    sum_q = torch.empty((K, DESCRIBE_D), dtype=torch.int64, device=dev)
    cells = torch.empty((K,), dtype=torch.int32, device=dev)
    embedding = torch.empty((K, DESCRIBE_D), dtype=torch.float32, device=dev)
    coherence = torch.empty((K,), dtype=torch.float32, device=dev)
    check(_lib.load().eod_describe_pool(mem.data_ptr(), object_labels.data_ptr(), objects.data_ptr(), N, K, sum_q.data_ptr(),
                                        cells.data_ptr(), embedding.data_ptr(), coherence.data_ptr(), _stream()), "eod_describe_pool")
    return {"sum_q": sum_q, "cells": cells, "embedding": embedding, "coherence": coherence}


def describe_classify(embedding: torch.Tensor, zs: torch.Tensor, topn: int = 5) -> dict:
    """The classes of described objects in any vocabulary (eod_describe_classify): K x C work, no pass over the cells.  `embedding`
    float32 [K, 512], 1 <= K <= 64: what `describe_pool` returned, now or earlier; `zs` float32 [512, C1] as the heads and
    `semmap_query` take it (the last column is the background and never enters; 1 <= C1 - 1 <= 2047); 1 <= `topn` <= min(8, C1 - 1).
    Returns `prob` float32 [K, C1 - 1] (the softmax of 50 * embedding @ zs over the classes), `top_cls` int32 and `top_prob` float32
    [K, topn]: the row's entries by (prob descending, class ascending).  An all-zero embedding row is an empty slot: a prob row of
    zeros, top_cls -1, top_prob 0.  The same bits on every call."""
    if (not isinstance(embedding, torch.Tensor) or embedding.dim() != 2 or embedding.shape[1] != DESCRIBE_D
            or embedding.dtype != torch.float32 or not embedding.is_contiguous()):
        raise _lib.EodError(f"describe_classify: embedding {_describe_what(embedding)}: expected contiguous float32 [K, {DESCRIBE_D}]")
    K = int(embedding.shape[0])
    if not 1 <= K <= DESCRIBE_K_MAX:
        raise _lib.EodError(f"describe_classify: embedding: K {K} outside 1..{DESCRIBE_K_MAX}")
    if (not isinstance(zs, torch.Tensor) or zs.dim() != 2 or zs.shape[0] != DESCRIBE_D or zs.dtype != torch.float32
            or not zs.is_contiguous() or zs.device != embedding.device):
        raise _lib.EodError(f"describe_classify: zs {_describe_what(zs)}: expected contiguous float32 [{DESCRIBE_D}, C1] on the "
                            "embedding's device")
    C = int(zs.shape[1]) - 1
    if not 1 <= C <= DESCRIBE_C_MAX:
        raise _lib.EodError(f"describe_classify: zs: {C} classes beside the background column, outside 1..{DESCRIBE_C_MAX}")
    if isinstance(topn, bool) or int(topn) != topn or not 1 <= int(topn) <= min(DESCRIBE_TOPN_MAX, C):
        raise _lib.EodError(f"describe_classify: topn {topn} outside 1..{min(DESCRIBE_TOPN_MAX, C)}")
    if embedding.data_ptr() % 16 != 0:
        raise _lib.EodError("describe_classify: embedding is not 16-byte aligned")
    if not embedding.is_cuda:
        raise _lib.EodError("describe_classify: embedding on the host (no CPU fallback)")
    dev, T = embedding.device, int(topn)
    prob = torch.empty((K, C), dtype=torch.float32, device=dev)
    top_cls = torch.empty((K, T), dtype=torch.int32, device=dev)
    top_prob = torch.empty((K, T), dtype=torch.float32, device=dev)
    check(_lib.load().eod_describe_classify(embedding.data_ptr(), zs.data_ptr(), K, C + 1, T, prob.data_ptr(), top_cls.data_ptr(),
                                            top_prob.data_ptr(), _stream()), "eod_describe_classify")
    return {"prob": prob, "top_cls": top_cls, "top_prob": top_prob}


RELATIONS_K_MAX, RELATIONS_N_MAX, RELATIONS_DIM_MAX, RELATIONS_RADIUS_MAX, RELATIONS_TOPN_MAX = 64, 1 << 22, 32767, 16, 8
RELATIONS_TILE_ROWS, RELATIONS_TILE_COLS = 32, 32        # the cells one workgroup owns (RL_TR, RL_TC of csrc/relations.hip)


def map_relations(object_labels: torch.Tensor, objects: torch.Tensor, cols: int, radius: int = 2, from_cell: int = -1,
                  topn: int = 4) -> dict:
    """How the objects of a label map stand to each other and to one cell (eod_map_relations; the semantics are those of
    include/eod_relations.h).  `object_labels` int32 [N], cell i = r * cols + c: the `object_labels` of `map_inventory`, a row of the
    `region_labels` of `map_regions` or any other label map; `objects` int32 [K], 1 <= K <= 64, as `inv["object"]` holds them (-1
    in unused slots; a cell belongs to the lowest slot that names its label).  Two cells are within reach when the squared
    distance of their rows and columns is at most `radius` ** 2 (1 <= `radius` <= 16).  Returns, for every ordered pair of slots
    a != b over the cell pairs within reach: `pair_key` int64 [K, K] (the bits of the unsigned minimum of (d2 << 32) | cell of a;
    -1 where no pair is within reach), `min_d2` int32 [K, K] (INT_MAX where none), `closest` int32 [K, K] (the cell of a nearest to
    b, the lowest on ties; -1), `near_cells` int32 [K, K] (cells of a with a cell of b within reach), `edges` int32 [K, K] (cell
    pairs one step apart: the shared border); per slot `cells` int32 [K], `nearest` and `nearest_d2` int32 [K, topn] (the slots
    within reach by (min_d2, slot) ascending, padded with -1 and INT_MAX; 1 <= `topn` <= 8), and for `from_cell` in 0..N-1, over
    all cells of a slot whatever the radius, `from_key` int64 [K], `from_d2` and `from_closest` int32 [K] (INT_MAX and -1 for an
    empty slot and for `from_cell` -1).  Integer atomics only: the same bits on every call."""
    if (not isinstance(object_labels, torch.Tensor) or object_labels.dim() != 1 or object_labels.dtype != torch.int32
            or not object_labels.is_contiguous()):
        raise _lib.EodError(f"map_relations: object_labels {_describe_what(object_labels)}: expected contiguous int32 [N]")
    N = int(object_labels.shape[0])
    if not 1 <= N <= RELATIONS_N_MAX:
        raise _lib.EodError(f"map_relations: object_labels: N {N} outside 1..{RELATIONS_N_MAX}")
    if (not isinstance(objects, torch.Tensor) or objects.dim() != 1 or objects.dtype != torch.int32 or not objects.is_contiguous()
            or objects.device != object_labels.device):
        raise _lib.EodError(f"map_relations: objects {_describe_what(objects)}: expected contiguous int32 [K] on the labels' device")
    K = int(objects.shape[0])
    if not 1 <= K <= RELATIONS_K_MAX:
        raise _lib.EodError(f"map_relations: objects: K {K} outside 1..{RELATIONS_K_MAX}")

    def whole(v):
        return not isinstance(v, bool) and isinstance(v, (int, np.integer))
    if not whole(cols) or int(cols) < 1 or N % int(cols) != 0:
        raise _lib.EodError(f"map_relations: cols {cols} does not divide the {N} cells")
    if int(cols) > RELATIONS_DIM_MAX or N // int(cols) > RELATIONS_DIM_MAX:
        raise _lib.EodError(f"map_relations: cols {cols}: {N // int(cols)} rows x {cols} columns, more than {RELATIONS_DIM_MAX} one way")
    if not whole(radius) or not 1 <= int(radius) <= RELATIONS_RADIUS_MAX:
        raise _lib.EodError(f"map_relations: radius {radius} outside 1..{RELATIONS_RADIUS_MAX}")
    if not whole(from_cell) or not -1 <= int(from_cell) < N:
        raise _lib.EodError(f"map_relations: from_cell {from_cell} outside -1..{N - 1}")
    if not whole(topn) or not 1 <= int(topn) <= RELATIONS_TOPN_MAX:
        raise _lib.EodError(f"map_relations: topn {topn} outside 1..{RELATIONS_TOPN_MAX}")
    if not object_labels.is_cuda:
        raise _lib.EodError("map_relations: object_labels on the host (no CPU fallback)")
    dev, T = object_labels.device, int(topn)
    keys = torch.empty((K * K + K,), dtype=torch.int64, device=dev)               # pair_key, from_key
    out = torch.empty((4 * K * K + 2 * K * T + 3 * K,), dtype=torch.int32, device=dev)
    KK, KT = K * K, K * T
    part = {}
    at = 0
    for name, n, shape in (("min_d2", KK, (K, K)), ("closest", KK, (K, K)), ("near_cells", KK, (K, K)), ("edges", KK, (K, K)),
                           ("cells", K, (K,)), ("nearest", KT, (K, T)), ("nearest_d2", KT, (K, T)), ("from_d2", K, (K,)),
                           ("from_closest", K, (K,))):
        part[name] = out[at:at + n].view(shape)
        at += n
    pair_key, from_key = keys[:KK].view(K, K), keys[KK:]
    check(_lib.load().eod_map_relations(object_labels.data_ptr(), objects.data_ptr(), N, K, int(cols), int(radius), int(from_cell), T,
                                        pair_key.data_ptr(), part["min_d2"].data_ptr(), part["closest"].data_ptr(),
                                        part["near_cells"].data_ptr(), part["edges"].data_ptr(), part["cells"].data_ptr(),
                                        part["nearest"].data_ptr(), part["nearest_d2"].data_ptr(), from_key.data_ptr(),
                                        part["from_d2"].data_ptr(), part["from_closest"].data_ptr(), _stream()), "eod_map_relations")
    return {"pair_key": pair_key, **part, "from_key": from_key}


ROUTE_K_MAX, ROUTE_P_MAX, ROUTE_N_MAX, ROUTE_DIM_MAX, ROUTE_PATH_MAX, ROUTE_SWEEPS_MAX = 64, 64, 1 << 22, 32767, 1024, 1024
ROUTE_COST_ORTH, ROUTE_COST_DIAG = 5, 7                  # a move along a row or column, a diagonal move (sqrt(2) taken as 7 / 5)
ROUTE_TILE_ROWS, ROUTE_TILE_COLS = 32, 32                # the cells one workgroup of a sweep owns (RT_TR, RT_TC of csrc/route.hip)
ROUTE_RESUMES = 8                                        # resumed calls of the model-level `route`, each with twice the sweeps of the last


def map_route_sweeps(rows: int, cols: int) -> int:
    """The default `sweeps` of `map_route`: four times the tile count of the longer side plus four, at most 1024.  A map that is
    reached without detours settles in about one sweep per tile across plus one, so this leaves room for a path that
    winds across the map about four times; a sweep launch in which no tile runs costs about as much as an empty launch."""
    ty, tx = -(-int(rows) // ROUTE_TILE_ROWS), -(-int(cols) // ROUTE_TILE_COLS)
    return min(ROUTE_SWEEPS_MAX, 4 * max(ty, tx) + 4)


def map_route_workspace(N: int, cols: int) -> int:
    """int32 words of a `map_route` workspace (eod_map_route_workspace_bytes / 4): three flags per tile and one byte per cell."""
    need = int(_lib.load().eod_map_route_workspace_bytes(int(N), int(cols)))
    if need == 0:
        raise _lib.EodError(f"map_route_workspace: N {N}, cols {cols}")
    return need // 4


def map_route(object_labels: torch.Tensor, objects: torch.Tensor, cols: int, from_cell: int, passable=None, path_max: int = 256,
              sweeps: Optional[int] = None, resume=None, workspace: Optional[torch.Tensor] = None) -> dict:
    """Shortest paths round the objects of a label map, from `from_cell` to every cell and to each of up to 64 objects
    (eod_map_route; the semantics are those of include/eod_route.h).  `object_labels` int32 [N], cell i = r * cols + c: the
    `object_labels` of `map_inventory` or any other label map; `objects` int32 [K], 1 <= K <= 64, as `inv["object"]` holds them (-1
    in unused slots; a cell belongs to the lowest slot that names its label).  A cell is free when its label is negative, when its
    label is one of `passable` (None, or int32 [P], P <= 64, or a sequence) or when it is `from_cell`; unlabelled cells count as
    free, the optimistic planner's assumption about space the memory does not know.  A move goes to one of the 8 neighbours on the
    grid, the target free and, for a diagonal move, both cells it passes between free too; it costs 5 along a row or column and 7
    diagonally.  Returns `dist` int32 [N] (INT_MAX: blocked or unreached), `parent` int32 [N] (the lowest cell a cheapest path
    enters from; -1), per slot `goal_key` int64 [K] (the bits of the unsigned minimum of (dist << 32) | cell over the reached free
    cells at most one row and one column from a cell of the slot; -1 where none), `goal_cost` (INT_MAX), `goal_cell` (-1), `cells`
    int32 [K], `path` int32 [K, path_max] (from `goal_cell` along `parent` to `from_cell`, then -1), `path_cells` int32 [K],
    `counts` int32 [2] (free cells, reached free cells) and `status` int32 [2]: status[0] bit 0: the `sweeps` (1..1024; None:
    `map_route_sweeps`) ran out before the distances had settled, bit 1: a bounded loop reached its bound; with a nonzero status
    every output but `dist` is void.  `status` is not read here, so nothing synchronises.  `resume`: the dict of an earlier call on
    the same `object_labels`, `passable` and `from_cell`, or its `dist`: the sweeps continue from that `dist`, which is updated in
    place and returned.  `workspace`: int32, 8-byte aligned, at least `map_route_workspace(N, cols)` words, any contents.  Integer
    min and add only: at status 0 the same bits on every call, whatever the sweeps and resumed calls that led there."""
    if (not isinstance(object_labels, torch.Tensor) or object_labels.dim() != 1 or object_labels.dtype != torch.int32
            or not object_labels.is_contiguous()):
        raise _lib.EodError(f"map_route: object_labels {_describe_what(object_labels)}: expected contiguous int32 [N]")
    N = int(object_labels.shape[0])
    if not 1 <= N <= ROUTE_N_MAX:
        raise _lib.EodError(f"map_route: object_labels: N {N} outside 1..{ROUTE_N_MAX}")
    dev = object_labels.device
    if (not isinstance(objects, torch.Tensor) or objects.dim() != 1 or objects.dtype != torch.int32 or not objects.is_contiguous()
            or objects.device != dev):
        raise _lib.EodError(f"map_route: objects {_describe_what(objects)}: expected contiguous int32 [K] on the labels' device")
    K = int(objects.shape[0])
    if not 1 <= K <= ROUTE_K_MAX:
        raise _lib.EodError(f"map_route: objects: K {K} outside 1..{ROUTE_K_MAX}")

    def whole(v):
        return not isinstance(v, bool) and isinstance(v, (int, np.integer))
    if not whole(cols) or int(cols) < 1 or N % int(cols) != 0:
        raise _lib.EodError(f"map_route: cols {cols} does not divide the {N} cells")
    if int(cols) > ROUTE_DIM_MAX or N // int(cols) > ROUTE_DIM_MAX:
        raise _lib.EodError(f"map_route: cols {cols}: {N // int(cols)} rows x {cols} columns, more than {ROUTE_DIM_MAX} one way")
    if not whole(from_cell) or not 0 <= int(from_cell) < N:
        raise _lib.EodError(f"map_route: from_cell {from_cell} outside 0..{N - 1}")
    if passable is not None and not isinstance(passable, torch.Tensor):
        try:
            passable = torch.as_tensor(np.asarray(list(passable), dtype=np.int64).astype(np.int32).reshape(-1), device=dev)
        except (TypeError, ValueError, OverflowError):
            raise _lib.EodError(f"map_route: passable {type(passable).__name__}: expected None, int32 [P] or a sequence of labels") from None
    if passable is not None and (passable.dim() != 1 or passable.dtype != torch.int32 or not passable.is_contiguous()
                                 or passable.device != dev or passable.shape[0] > ROUTE_P_MAX):
        raise _lib.EodError(f"map_route: passable {_describe_what(passable)}: expected contiguous int32 [P], P <= {ROUTE_P_MAX}, on the "
                            "labels' device")
    P = 0 if passable is None else int(passable.shape[0])
    if not whole(path_max) or not 1 <= int(path_max) <= ROUTE_PATH_MAX:
        raise _lib.EodError(f"map_route: path_max {path_max} outside 1..{ROUTE_PATH_MAX}")
    if sweeps is None:
        sweeps = map_route_sweeps(N // int(cols), int(cols))
    if not whole(sweeps) or not 1 <= int(sweeps) <= ROUTE_SWEEPS_MAX:
        raise _lib.EodError(f"map_route: sweeps {sweeps} outside 1..{ROUTE_SWEEPS_MAX}")
    dist = resume["dist"] if isinstance(resume, dict) and "dist" in resume else resume
    if dist is not None and (not isinstance(dist, torch.Tensor) or dist.dtype != torch.int32 or tuple(dist.shape) != (N,)
                             or not dist.is_contiguous() or dist.device != dev):
        raise _lib.EodError(f"map_route: resume {_describe_what(dist)}: expected the dict of an earlier call or its dist, contiguous "
                            f"int32 [{N}] on the labels' device")
    if not object_labels.is_cuda:
        raise _lib.EodError("map_route: object_labels on the host (no CPU fallback)")
    need = map_route_workspace(N, int(cols))
    if workspace is not None and (not isinstance(workspace, torch.Tensor) or workspace.dtype != torch.int32 or workspace.dim() != 1
                                  or not workspace.is_contiguous() or workspace.numel() < need or workspace.device != dev
                                  or workspace.data_ptr() % 8 != 0):
        raise _lib.EodError(f"map_route: workspace: expected {need} contiguous, 8-byte aligned int32 on the labels' device")
    if workspace is None:
        workspace = torch.empty((need,), dtype=torch.int32, device=dev)
    T = int(path_max)
    cont = dist is not None
    if not cont:
        dist = torch.empty((N,), dtype=torch.int32, device=dev)
    parent = torch.empty((N,), dtype=torch.int32, device=dev)
    goal_key = torch.empty((K,), dtype=torch.int64, device=dev)
    out = torch.empty((4 * K + K * T + 4,), dtype=torch.int32, device=dev)
    part = {}
    at = 0
    for name, n, shape in (("goal_cost", K, (K,)), ("goal_cell", K, (K,)), ("cells", K, (K,)), ("path", K * T, (K, T)),
                           ("path_cells", K, (K,)), ("counts", 2, (2,)), ("status", 2, (2,))):
        part[name] = out[at:at + n].view(shape)
        at += n
    check(_lib.load().eod_map_route(object_labels.data_ptr(), objects.data_ptr(), _ptr(passable) if P else None, N, K, P, int(cols),
                                    int(from_cell), T, int(sweeps), 1 if cont else 0, dist.data_ptr(), parent.data_ptr(),
                                    goal_key.data_ptr(), part["goal_cost"].data_ptr(), part["goal_cell"].data_ptr(),
                                    part["cells"].data_ptr(), part["path"].data_ptr(), part["path_cells"].data_ptr(),
                                    part["counts"].data_ptr(), part["status"].data_ptr(), workspace.data_ptr(), workspace.numel() * 4,
                                    _stream()), "eod_map_route")
    return {"dist": dist, "parent": parent, "goal_key": goal_key, **part}


CLEARANCE_K_MAX, CLEARANCE_P_MAX, CLEARANCE_N_MAX, CLEARANCE_DIM_MAX = 64, 64, 1 << 22, 32767
# the rows and columns one workgroup of the row pass owns and the columns it stages either side (CL_TR, CL_CC, CL_HALO of
# csrc/clearance.hip)
CLEARANCE_TILE_ROWS, CLEARANCE_CHUNK_COLS, CLEARANCE_HALO_COLS = 4, 64, 64
CLEARANCE_NONE = 2 ** 31 - 1                             # d2 of a map without a blocked cell


def map_clearance_workspace(N: int, cols: int) -> int:
    """int32 words of a `map_clearance` workspace (eod_map_clearance_workspace_bytes / 4): one byte and one int32 per cell."""
    need = int(_lib.load().eod_map_clearance_workspace_bytes(int(N), int(cols)))
    if need == 0:
        raise _lib.EodError(f"map_clearance_workspace: N {N}, cols {cols}")
    return need // 4


def map_clearance(object_labels: torch.Tensor, objects: torch.Tensor, cols: int, radius2: int = 0, keep_cell: int = -1, passable=None,
                  workspace: Optional[torch.Tensor] = None) -> dict:
    """The exact squared distance from every cell of a label map to the nearest blocked cell, that cell, and the map inflated by a
    body of squared radius `radius2` (eod_map_clearance; the semantics are those of include/eod_clearance.h).  `object_labels`
    int32 [N], cell i = r * cols + c; `objects` int32 [K], 1 <= K <= 64, as `inv["object"]` holds them (-1 in unused slots; a cell
    belongs to the lowest slot that names its label).  A cell is blocked when its label is >= 0 and not one of `passable` (None, or
    int32 [P], P <= 64, or a sequence); `keep_cell` does not change that.  Returns per cell `d2` int32 [N] (0 on a blocked cell,
    INT_MAX when the map has none), `nearest` (the lowest blocked cell at that distance; the cell itself; -1), `owner` (its label;
    -1) and `inflated` (the label map for `map_route` with a body: a free cell with d2 <= radius2 takes its owner's label, unless
    `keep_cell` >= 0 is at most radius2 away from it); per slot `cells`, `territory` (the free cells nearest to the slot),
    `widest_key` int64 [K] (the bits of the unsigned maximum of (d2 << 32) | ~cell over them; 0), `widest_d2` (0) and `widest_cell`
    (-1); `open_key` int64 [1] (the same maximum over all free cells), `counts` int32 [3] (blocked, free, free cells that
    `inflated` changed) and `status` int32 [2] (bit 1 of status[0]: a bounded loop reached its bound), which is not read here, so
    nothing synchronises.  `workspace`: int32, 8-byte aligned, at least `map_clearance_workspace(N, cols)` words, any contents.
    Integer min, max, multiply and add only: the same bits on every call."""
    if (not isinstance(object_labels, torch.Tensor) or object_labels.dim() != 1 or object_labels.dtype != torch.int32
            or not object_labels.is_contiguous()):
        raise _lib.EodError(f"map_clearance: object_labels {_describe_what(object_labels)}: expected contiguous int32 [N]")
    N = int(object_labels.shape[0])
    if not 1 <= N <= CLEARANCE_N_MAX:
        raise _lib.EodError(f"map_clearance: object_labels: N {N} outside 1..{CLEARANCE_N_MAX}")
    dev = object_labels.device
    if (not isinstance(objects, torch.Tensor) or objects.dim() != 1 or objects.dtype != torch.int32 or not objects.is_contiguous()
            or objects.device != dev):
        raise _lib.EodError(f"map_clearance: objects {_describe_what(objects)}: expected contiguous int32 [K] on the labels' device")
    K = int(objects.shape[0])
    if not 1 <= K <= CLEARANCE_K_MAX:
        raise _lib.EodError(f"map_clearance: objects: K {K} outside 1..{CLEARANCE_K_MAX}")

    def whole(v):
        return not isinstance(v, bool) and isinstance(v, (int, np.integer))
    if not whole(cols) or int(cols) < 1 or N % int(cols) != 0:
        raise _lib.EodError(f"map_clearance: cols {cols} does not divide the {N} cells")
    if int(cols) > CLEARANCE_DIM_MAX or N // int(cols) > CLEARANCE_DIM_MAX:
        raise _lib.EodError(f"map_clearance: cols {cols}: {N // int(cols)} rows x {cols} columns, more than {CLEARANCE_DIM_MAX} one way")
    if not whole(radius2) or not 0 <= int(radius2) < CLEARANCE_NONE:
        raise _lib.EodError(f"map_clearance: radius2 {radius2} outside 0..{CLEARANCE_NONE - 1}")
    if not whole(keep_cell) or not -1 <= int(keep_cell) < N:
        raise _lib.EodError(f"map_clearance: keep_cell {keep_cell} outside -1..{N - 1}")
    if passable is not None and not isinstance(passable, torch.Tensor):
        try:
            passable = torch.as_tensor(np.asarray(list(passable), dtype=np.int64).astype(np.int32).reshape(-1), device=dev)
        except (TypeError, ValueError, OverflowError):
            raise _lib.EodError(f"map_clearance: passable {type(passable).__name__}: expected None, int32 [P] or a sequence of "
                                "labels") from None
    if passable is not None and (passable.dim() != 1 or passable.dtype != torch.int32 or not passable.is_contiguous()
                                 or passable.device != dev or passable.shape[0] > CLEARANCE_P_MAX):
        raise _lib.EodError(f"map_clearance: passable {_describe_what(passable)}: expected contiguous int32 [P], P <= "
                            f"{CLEARANCE_P_MAX}, on the labels' device")
    P = 0 if passable is None else int(passable.shape[0])
    if not object_labels.is_cuda:
        raise _lib.EodError("map_clearance: object_labels on the host (no CPU fallback)")
    need = map_clearance_workspace(N, int(cols))
    if workspace is not None and (not isinstance(workspace, torch.Tensor) or workspace.dtype != torch.int32 or workspace.dim() != 1
                                  or not workspace.is_contiguous() or workspace.numel() < need or workspace.device != dev
                                  or workspace.data_ptr() % 8 != 0):
        raise _lib.EodError(f"map_clearance: workspace: expected {need} contiguous, 8-byte aligned int32 on the labels' device")
    if workspace is None:
        workspace = torch.empty((need,), dtype=torch.int32, device=dev)
    per_cell = torch.empty((4, N), dtype=torch.int32, device=dev)
    keys = torch.empty((K + 1,), dtype=torch.int64, device=dev)      # widest_key, open_key
    out = torch.empty((4 * K + 5,), dtype=torch.int32, device=dev)
    part = {}
    at = 0
    for name, n in (("cells", K), ("territory", K), ("widest_d2", K), ("widest_cell", K), ("counts", 3), ("status", 2)):
        part[name] = out[at:at + n]
        at += n
    d2, nearest, owner, inflated = per_cell[0], per_cell[1], per_cell[2], per_cell[3]
    widest_key, open_key = keys[:K], keys[K:]
    check(_lib.load().eod_map_clearance(object_labels.data_ptr(), objects.data_ptr(), _ptr(passable) if P else None, N, K, P, int(cols),
                                        int(radius2), int(keep_cell), d2.data_ptr(), nearest.data_ptr(), owner.data_ptr(),
                                        inflated.data_ptr(), part["cells"].data_ptr(), part["territory"].data_ptr(),
                                        widest_key.data_ptr(), part["widest_d2"].data_ptr(), part["widest_cell"].data_ptr(),
                                        open_key.data_ptr(), part["counts"].data_ptr(), part["status"].data_ptr(),
                                        workspace.data_ptr(), workspace.numel() * 4, _stream()), "eod_map_clearance")
    return {"d2": d2, "nearest": nearest, "owner": owner, "inflated": inflated, "cells": part["cells"],
            "territory": part["territory"], "widest_key": widest_key, "widest_d2": part["widest_d2"],
            "widest_cell": part["widest_cell"], "open_key": open_key, "counts": part["counts"], "status": part["status"]}


SIGHT_K_MAX, SIGHT_P_MAX, SIGHT_S_MAX, SIGHT_N_MAX, SIGHT_DIM_MAX = 64, 64, 64, 1 << 22, 32767
# up to SIGHT_LDS_CELLS cells the walk reads the opacity bit plane from LDS, above it from the workspace; a workgroup of the walk
# owns SIGHT_WORKGROUP consecutive cells and looks from one group of SIGHT_SOURCE_GROUP sources (csrc/sight.hip)
SIGHT_LDS_CELLS, SIGHT_SOURCE_GROUP, SIGHT_WORKGROUP = 131072, 16, 256
SIGHT_UNBOUNDED = 2 ** 31 - 1                            # range2 of a sensor without a range; near_d2 where nothing is seen


def map_sight_workspace(N: int, cols: int) -> int:
    """int32 words of a `map_sight` workspace (eod_map_sight_workspace_bytes / 4): one byte and one bit per cell."""
    need = int(_lib.load().eod_map_sight_workspace_bytes(int(N), int(cols)))
    if need == 0:
        raise _lib.EodError(f"map_sight_workspace: N {N}, cols {cols}")
    return need // 4


def map_sight(object_labels: torch.Tensor, objects: torch.Tensor, cols: int, from_cells, range2: Optional[int] = None, passable=None,
              workspace: Optional[torch.Tensor] = None) -> dict:
    """Which cells of a label map each of up to 64 cells sees, and how much of every object (eod_map_sight; the semantics are those
    of include/eod_sight.h).  `object_labels` int32 [N], cell i = r * cols + c; `objects` int32 [K], 1 <= K <= 64, as
    `inv["object"]` holds them (-1 in unused slots; a cell belongs to the lowest slot that names its label).  A cell is opaque when
    its label is >= 0 and not one of `passable` (None, or int32 [P], P <= 64, or a sequence).  `from_cells`: one int, or a sequence
    or an int32/int64 tensor of 1 <= S <= 64 cells 0..N-1 to look from, negative for an unused source, duplicates allowed; the entry
    point reads them on the host, so a tensor on the device is copied there first (the one synchronisation of this call; a sequence
    or a host tensor costs none).  `range2`: the sensor's range in cells, squared; None is unbounded.  Source s sees cell t when t is
    within the range, no cell of the rounded line from s to t strictly between them is opaque, and no diagonal step of the line
    passes between two opaque cells; the source's own cell is transparent on its own lines, and the line is not symmetric in s and t.
    Returns `seen_mask` int64 [N]: bit s of cell i (`(seen_mask[i] >> s) & 1`; bit 63, source 63, is the sign bit) is set exactly
    when source s is used and sees cell i; per slot `cells`; per (source, slot) `seen_cells` int32 [S, K], `near_key` int64 [S, K]
    (the bits of the unsigned minimum of (d2 << 32) | cell over the seen cells of the slot; all ones), `near_d2` (INT_MAX) and
    `near_cell` (-1), the nearest visible cell of the object; per slot `best_key` int64 [K] (the maximum of (seen_cells << 32) | ~s;
    0), `best_seen` (0) and `best_source` (-1), the source that sees most of the object, the lowest on a tie; `source_counts` int32
    [S, 2] (transparent and opaque cells seen), `counts` int32 [3] (opaque cells, transparent cells, cells anyone sees) and `status`
    int32 [2] (bit 1 of status[0]: a bounded loop reached its bound), which is not read here.  `workspace`: int32, 8-byte aligned,
    at least `map_sight_workspace(N, cols)` words, any contents.  Integer comparisons, additions and atomics only: the same bits on
    every call."""
    if (not isinstance(object_labels, torch.Tensor) or object_labels.dim() != 1 or object_labels.dtype != torch.int32
            or not object_labels.is_contiguous()):
        raise _lib.EodError(f"map_sight: object_labels {_describe_what(object_labels)}: expected contiguous int32 [N]")
    N = int(object_labels.shape[0])
    if not 1 <= N <= SIGHT_N_MAX:
        raise _lib.EodError(f"map_sight: object_labels: N {N} outside 1..{SIGHT_N_MAX}")
    dev = object_labels.device
    if (not isinstance(objects, torch.Tensor) or objects.dim() != 1 or objects.dtype != torch.int32 or not objects.is_contiguous()
            or objects.device != dev):
        raise _lib.EodError(f"map_sight: objects {_describe_what(objects)}: expected contiguous int32 [K] on the labels' device")
    K = int(objects.shape[0])
    if not 1 <= K <= SIGHT_K_MAX:
        raise _lib.EodError(f"map_sight: objects: K {K} outside 1..{SIGHT_K_MAX}")

    def whole(v):
        return not isinstance(v, bool) and isinstance(v, (int, np.integer))
    if not whole(cols) or int(cols) < 1 or N % int(cols) != 0:
        raise _lib.EodError(f"map_sight: cols {cols} does not divide the {N} cells")
    if int(cols) > SIGHT_DIM_MAX or N // int(cols) > SIGHT_DIM_MAX:
        raise _lib.EodError(f"map_sight: cols {cols}: {N // int(cols)} rows x {cols} columns, more than {SIGHT_DIM_MAX} one way")
    if isinstance(from_cells, torch.Tensor):
        if from_cells.dtype not in (torch.int32, torch.int64) or from_cells.dim() > 1 or from_cells.is_meta:
            raise _lib.EodError(f"map_sight: from_cells {_describe_what(from_cells)}: expected int32 or int64 [S] or one cell")
        src = from_cells.detach().cpu().numpy().astype(np.int64).reshape(-1)
    else:
        try:
            seq = [from_cells] if whole(from_cells) else list(from_cells)
            if not all(whole(v) for v in seq):
                raise TypeError
            src = np.asarray(seq, dtype=np.int64).reshape(-1)
        except (TypeError, ValueError, OverflowError):
            raise _lib.EodError(f"map_sight: from_cells {type(from_cells).__name__}: expected one cell, or a sequence or tensor of "
                                "cells") from None
    if not 1 <= src.size <= SIGHT_S_MAX:
        raise _lib.EodError(f"map_sight: from_cells: S {src.size} outside 1..{SIGHT_S_MAX}")
    if src.max() >= N or src.min() < -2 ** 31:
        raise _lib.EodError(f"map_sight: from_cells: {int(src.max() if src.max() >= N else src.min())} is no cell of the {N} (negative: unused)")
    src = np.ascontiguousarray(src.astype(np.int32))
    S = int(src.size)
    if range2 is None:
        range2 = SIGHT_UNBOUNDED
    if not whole(range2) or not 0 <= int(range2) <= SIGHT_UNBOUNDED:
        raise _lib.EodError(f"map_sight: range2 {range2} outside 0..{SIGHT_UNBOUNDED} (None: unbounded)")
    if passable is not None and not isinstance(passable, torch.Tensor):
        try:
            passable = torch.as_tensor(np.asarray(list(passable), dtype=np.int64).astype(np.int32).reshape(-1), device=dev)
        except (TypeError, ValueError, OverflowError):
            raise _lib.EodError(f"map_sight: passable {type(passable).__name__}: expected None, int32 [P] or a sequence of "
                                "labels") from None
    if passable is not None and (passable.dim() != 1 or passable.dtype != torch.int32 or not passable.is_contiguous()
                                 or passable.device != dev or passable.shape[0] > SIGHT_P_MAX):
        raise _lib.EodError(f"map_sight: passable {_describe_what(passable)}: expected contiguous int32 [P], P <= "
                            f"{SIGHT_P_MAX}, on the labels' device")
    P = 0 if passable is None else int(passable.shape[0])
    if not object_labels.is_cuda:
        raise _lib.EodError("map_sight: object_labels on the host (no CPU fallback)")
    need = map_sight_workspace(N, int(cols))
    if workspace is not None and (not isinstance(workspace, torch.Tensor) or workspace.dtype != torch.int32 or workspace.dim() != 1
                                  or not workspace.is_contiguous() or workspace.numel() < need or workspace.device != dev
                                  or workspace.data_ptr() % 8 != 0):
        raise _lib.EodError(f"map_sight: workspace: expected {need} contiguous, 8-byte aligned int32 on the labels' device")
    if workspace is None:
        workspace = torch.empty((need,), dtype=torch.int32, device=dev)
    seen_mask = torch.empty((N,), dtype=torch.int64, device=dev)
    keys = torch.empty((S * K + K,), dtype=torch.int64, device=dev)  # near_key, best_key
    out = torch.empty((3 * S * K + 3 * K + 2 * S + 5,), dtype=torch.int32, device=dev)
    part = {}
    at = 0
    for name, n, shape in (("cells", K, (K,)), ("seen_cells", S * K, (S, K)), ("near_d2", S * K, (S, K)), ("near_cell", S * K, (S, K)),
                           ("best_seen", K, (K,)), ("best_source", K, (K,)), ("source_counts", 2 * S, (S, 2)), ("counts", 3, (3,)),
                           ("status", 2, (2,))):
        part[name] = out[at:at + n].view(shape)
        at += n
    near_key, best_key = keys[:S * K].view(S, K), keys[S * K:]
    check(_lib.load().eod_map_sight(object_labels.data_ptr(), objects.data_ptr(), _ptr(passable) if P else None, src.ctypes.data, N, K,
                                    P, S, int(cols), int(range2), seen_mask.data_ptr(), part["cells"].data_ptr(),
                                    part["seen_cells"].data_ptr(), near_key.data_ptr(), part["near_d2"].data_ptr(),
                                    part["near_cell"].data_ptr(), best_key.data_ptr(), part["best_seen"].data_ptr(),
                                    part["best_source"].data_ptr(), part["source_counts"].data_ptr(), part["counts"].data_ptr(),
                                    part["status"].data_ptr(), workspace.data_ptr(), workspace.numel() * 4, _stream()), "eod_map_sight")
    return {"seen_mask": seen_mask, "cells": part["cells"], "seen_cells": part["seen_cells"], "near_key": near_key,
            "near_d2": part["near_d2"], "near_cell": part["near_cell"], "best_key": best_key, "best_seen": part["best_seen"],
            "best_source": part["best_source"], "source_counts": part["source_counts"], "counts": part["counts"],
            "status": part["status"]}


FRONTIER_P_MAX, FRONTIER_TOPK_MAX, FRONTIER_N_MAX, FRONTIER_DIM_MAX, FRONTIER_PIXELS_MAX = 64, 64, 1 << 22, 32767, 1 << 24
FRONTIER_RANKS = {"area": 0, "behind": 1}                # rank_by: by the frontier's own cells, or by the unknown region behind it
FRONTIER_NO_WAY = 2 ** 31 - 1                            # reach_cost where no cell of the frontier can be reached


def _whole(v) -> bool:
    return not isinstance(v, bool) and isinstance(v, (int, np.integer))


def map_cover(proj_indices: torch.Tensor, last_seen: torch.Tensor, stamp: int, exclude_cell: int = -1) -> torch.Tensor:
    """The record of what the camera covered (eod_map_cover; include/eod_frontier.h): for every pixel of `proj_indices` (int32, any
    shape, contiguous) whose cell c has 0 <= c < N and c != `exclude_cell`, `last_seen[c] = max(last_seen[c], stamp)`, in place.
    `last_seen` is int32 [N], filled with -1 by the caller once; `stamp` >= 0.  Every other pixel is dropped.  One launch, integer
    atomics only: the result depends neither on the order of the pixels nor on that of the frames with one stamp.  Returns
    `last_seen`."""
    if (not isinstance(proj_indices, torch.Tensor) or proj_indices.dtype != torch.int32 or not proj_indices.is_contiguous()):
        raise _lib.EodError(f"map_cover: proj_indices {_describe_what(proj_indices)}: expected contiguous int32")
    if (not isinstance(last_seen, torch.Tensor) or last_seen.dim() != 1 or last_seen.dtype != torch.int32 or not last_seen.is_contiguous()
            or last_seen.device != proj_indices.device):
        raise _lib.EodError(f"map_cover: last_seen {_describe_what(last_seen)}: expected contiguous int32 [N] on the pixels' device")
    P, N = int(proj_indices.numel()), int(last_seen.shape[0])
    if P > FRONTIER_PIXELS_MAX or not 1 <= N <= FRONTIER_N_MAX:
        raise _lib.EodError(f"map_cover: {P} pixels (at most {FRONTIER_PIXELS_MAX}), {N} cells (1..{FRONTIER_N_MAX})")
    if not _whole(stamp) or not 0 <= int(stamp) <= 2 ** 31 - 1:
        raise _lib.EodError(f"map_cover: stamp {stamp} outside 0..{2 ** 31 - 1}")
    if not _whole(exclude_cell) or not -2 ** 31 <= int(exclude_cell) <= 2 ** 31 - 1:
        raise _lib.EodError(f"map_cover: exclude_cell {exclude_cell}: expected an int (-1: none)")
    if not last_seen.is_cuda:
        raise _lib.EodError("map_cover: last_seen on the host (no CPU fallback)")
    check(_lib.load().eod_map_cover(proj_indices.data_ptr() if P else None, P, N, int(stamp), int(exclude_cell), last_seen.data_ptr(),
                                    _stream()), "eod_map_cover")
    return last_seen


def map_frontier_workspace(N: int, cols: int) -> int:
    """int32 words of a `map_frontier` workspace (eod_map_frontier_workspace_bytes / 4)."""
    need = int(_lib.load().eod_map_frontier_workspace_bytes(int(N), int(cols)))
    if need == 0:
        raise _lib.EodError(f"map_frontier_workspace: N {N}, cols {cols}")
    return need // 4


def map_frontier(object_labels: torch.Tensor, last_seen: torch.Tensor, cols: int, since: int = 0, dist: Optional[torch.Tensor] = None,
                 from_cell: int = -1, passable=None, min_cells: int = 2, topk: int = 16, rank_by="behind",
                 workspace: Optional[torch.Tensor] = None) -> dict:
    """Where the known space ends and what lies beyond (eod_map_frontier; the semantics are those of include/eod_frontier.h).
    `object_labels` int32 [N], cell i = r * cols + c; `last_seen` int32 [N], the record of `map_cover`.  A cell is BLOCKED when its
    label is >= 0 and not one of `passable` (None, int32 [P], P <= 64, or a sequence), otherwise OPEN when `last_seen >= since` and
    UNKNOWN when not.  A frontier cell is an OPEN cell with an UNKNOWN 4-neighbour; a frontier an 8-connected component of them; an
    unknown region a 4-connected component of UNKNOWN cells; a label the lowest cell.  Returns per cell `frontier_labels`,
    `unknown_labels` (-1 elsewhere) and `unknown_area` (at a region's label cell its cells, 0 elsewhere), int32 [N]; `count` [1], the
    frontiers of at least `min_cells` cells; for the `topk` (1..64) of them with the largest rank key, in descending order
    (`rank_by` "area" or 0: (area << 32) | ~label; "behind" or 1: (behind_area << 32) | ~label), `frontier` (the label; -1 in a
    padding slot), `area`, `bbox` [K, 4], `sum_rc` int64 [K, 2], `open_edges` (pairs of a frontier cell and an UNKNOWN neighbour),
    `behind_key` int64 with its halves `behind_area` and `behind_label` (the largest unknown region the frontier opens onto; 0 and
    -1), `reach_key` int64 (the minimum of (v << 32) | cell over the frontier's cells with v < INT_MAX; all ones) with its halves
    `reach_cost` (INT_MAX) and `reach_cell` (-1): v is `dist[cell]` with `dist` int32 [N] (the `dist` of `map_route`), otherwise the
    squared distance in cells from `from_cell` (0..N-1), otherwise 0.  `counts` int32 [5]: BLOCKED, OPEN, UNKNOWN cells, frontier
    cells, unknown regions; `status` int32 [2] (bit 1 of status[0]: a bounded loop reached its bound), which is not read here.
    `workspace`: int32, 8-byte aligned, at least `map_frontier_workspace(N, cols)` words, any contents.  Integer comparisons,
    additions and atomics only: the same bits on every call."""
    if (not isinstance(object_labels, torch.Tensor) or object_labels.dim() != 1 or object_labels.dtype != torch.int32
            or not object_labels.is_contiguous()):
        raise _lib.EodError(f"map_frontier: object_labels {_describe_what(object_labels)}: expected contiguous int32 [N]")
    N = int(object_labels.shape[0])
    if not 1 <= N <= FRONTIER_N_MAX:
        raise _lib.EodError(f"map_frontier: object_labels: N {N} outside 1..{FRONTIER_N_MAX}")
    dev = object_labels.device
    if (not isinstance(last_seen, torch.Tensor) or last_seen.shape != object_labels.shape or last_seen.dtype != torch.int32
            or not last_seen.is_contiguous() or last_seen.device != dev):
        raise _lib.EodError(f"map_frontier: last_seen {_describe_what(last_seen)}: expected contiguous int32 [{N}] on the labels' device")
    if dist is not None and (not isinstance(dist, torch.Tensor) or dist.shape != object_labels.shape or dist.dtype != torch.int32
                             or not dist.is_contiguous() or dist.device != dev):
        raise _lib.EodError(f"map_frontier: dist {_describe_what(dist)}: expected None or contiguous int32 [{N}] on the labels' device")
    if not _whole(cols) or int(cols) < 1 or N % int(cols) != 0:
        raise _lib.EodError(f"map_frontier: cols {cols} does not divide the {N} cells")
    if int(cols) > FRONTIER_DIM_MAX or N // int(cols) > FRONTIER_DIM_MAX:
        raise _lib.EodError(f"map_frontier: cols {cols}: {N // int(cols)} rows x {cols} columns, more than {FRONTIER_DIM_MAX} one way")
    if not _whole(since) or not -2 ** 31 <= int(since) <= 2 ** 31 - 1:
        raise _lib.EodError(f"map_frontier: since {since}: expected an int32")
    if from_cell is None:
        from_cell = -1
    if not _whole(from_cell) or not -1 <= int(from_cell) < N:
        raise _lib.EodError(f"map_frontier: from_cell {from_cell} is no cell of the {N} (-1 or None: none)")
    if not _whole(min_cells) or not 1 <= int(min_cells) <= 2 ** 31 - 1:
        raise _lib.EodError(f"map_frontier: min_cells {min_cells}: expected at least 1")
    if not _whole(topk) or not 1 <= int(topk) <= FRONTIER_TOPK_MAX:
        raise _lib.EodError(f"map_frontier: topk {topk} outside 1..{FRONTIER_TOPK_MAX}")
    if isinstance(rank_by, str) and rank_by in FRONTIER_RANKS:
        rank_by = FRONTIER_RANKS[rank_by]
    if not _whole(rank_by) or int(rank_by) not in (0, 1):
        raise _lib.EodError(f"map_frontier: rank_by {rank_by!r}: expected 'area' (0) or 'behind' (1)")
    if passable is not None and not isinstance(passable, torch.Tensor):
        try:
            passable = torch.as_tensor(np.asarray(list(passable), dtype=np.int64).astype(np.int32).reshape(-1), device=dev)
        except (TypeError, ValueError, OverflowError):
            raise _lib.EodError(f"map_frontier: passable {type(passable).__name__}: expected None, int32 [P] or a sequence of "
                                "labels") from None
    if passable is not None and (passable.dim() != 1 or passable.dtype != torch.int32 or not passable.is_contiguous()
                                 or passable.device != dev or passable.shape[0] > FRONTIER_P_MAX):
        raise _lib.EodError(f"map_frontier: passable {_describe_what(passable)}: expected contiguous int32 [P], P <= "
                            f"{FRONTIER_P_MAX}, on the labels' device")
    P = 0 if passable is None else int(passable.shape[0])
    if not object_labels.is_cuda:
        raise _lib.EodError("map_frontier: object_labels on the host (no CPU fallback)")
    need = map_frontier_workspace(N, int(cols))
    if workspace is not None and (not isinstance(workspace, torch.Tensor) or workspace.dtype != torch.int32 or workspace.dim() != 1
                                  or not workspace.is_contiguous() or workspace.numel() < need or workspace.device != dev
                                  or workspace.data_ptr() % 8 != 0):
        raise _lib.EodError(f"map_frontier: workspace: expected {need} contiguous, 8-byte aligned int32 on the labels' device")
    if workspace is None:
        workspace = torch.empty((need,), dtype=torch.int32, device=dev)
    K = int(topk)
    cells = torch.empty((3, N), dtype=torch.int32, device=dev)       # frontier_labels, unknown_labels, unknown_area
    keys = torch.empty((4 * K,), dtype=torch.int64, device=dev)      # sum_rc, behind_key, reach_key
    out = torch.empty((12 * K + 8,), dtype=torch.int32, device=dev)
    part = {}
    at = 0
    for name, n, shape in (("count", 1, (1,)), ("frontier", K, (K,)), ("area", K, (K,)), ("bbox", 4 * K, (K, 4)),
                           ("open_edges", K, (K,)), ("behind_area", K, (K,)), ("behind_label", K, (K,)), ("reach_cost", K, (K,)),
                           ("reach_cell", K, (K,)), ("counts", 5, (5,)), ("status", 2, (2,))):
        part[name] = out[at:at + n].view(shape)
        at += n
    sum_rc, behind_key, reach_key = keys[:2 * K].view(K, 2), keys[2 * K:3 * K], keys[3 * K:]
    check(_lib.load().eod_map_frontier(
        object_labels.data_ptr(), _ptr(passable) if P else None, last_seen.data_ptr(), None if dist is None else dist.data_ptr(), N, P,
        int(cols), int(since), int(from_cell), int(min_cells), K, int(rank_by), cells[0].data_ptr(), cells[1].data_ptr(),
        cells[2].data_ptr(), part["count"].data_ptr(), part["frontier"].data_ptr(), part["area"].data_ptr(), part["bbox"].data_ptr(),
        sum_rc.data_ptr(), part["open_edges"].data_ptr(), behind_key.data_ptr(), part["behind_area"].data_ptr(),
        part["behind_label"].data_ptr(), reach_key.data_ptr(), part["reach_cost"].data_ptr(), part["reach_cell"].data_ptr(),
        part["counts"].data_ptr(), part["status"].data_ptr(), workspace.data_ptr(), workspace.numel() * 4, _stream()), "eod_map_frontier")
    return {"frontier_labels": cells[0], "unknown_labels": cells[1], "unknown_area": cells[2], "count": part["count"],
            "frontier": part["frontier"], "area": part["area"], "bbox": part["bbox"], "sum_rc": sum_rc,
            "open_edges": part["open_edges"], "behind_key": behind_key, "behind_area": part["behind_area"],
            "behind_label": part["behind_label"], "reach_key": reach_key, "reach_cost": part["reach_cost"],
            "reach_cell": part["reach_cell"], "counts": part["counts"], "status": part["status"]}


OBSTACLES_K_MAX, OBSTACLES_TOPK_MAX, OBSTACLES_N_MAX, OBSTACLES_DIM_MAX, OBSTACLES_PIXELS_MAX, OBSTACLES_BAND_MAX = (
    64, 64, 1 << 22, 32767, 1 << 24, 1000000)
OBSTACLES_KINDS = {"unseen": 0, "clear": 1, "obstacle": 2, "object": 3}       # the values of `kind`
HEIGHT_RECORD_INIT = (0, 0, 2 ** 31 - 1, -2 ** 31)                             # hits, band_hits, h_min_mm, h_max_mm of an empty record


def new_height_record(n_cells: int, device) -> torch.Tensor:
    """An empty record for `map_heights`: int32 [4, N], the planes hits, band_hits, h_min_mm, h_max_mm holding 0, 0, INT_MAX,
    INT_MIN."""
    if not _whole(n_cells) or not 1 <= int(n_cells) <= OBSTACLES_N_MAX:
        raise _lib.EodError(f"new_height_record: n_cells {n_cells} outside 1..{OBSTACLES_N_MAX}")
    record = torch.empty((4, int(n_cells)), dtype=torch.int32, device=device)
    for plane, v in enumerate(HEIGHT_RECORD_INIT):
        record[plane].fill_(v)
    return record


def _check_height_record(what: str, record, device=None) -> int:
    if (not isinstance(record, torch.Tensor) or record.dim() != 2 or record.shape[0] != 4 or record.dtype != torch.int32
            or not record.is_contiguous() or (device is not None and record.device != device)):
        raise _lib.EodError(f"{what}: record {_describe_what(record)}: expected contiguous int32 [4, N] (new_height_record)"
                            + (" on the pixels' device" if device is not None else ""))
    N = int(record.shape[1])
    if not 1 <= N <= OBSTACLES_N_MAX:
        raise _lib.EodError(f"{what}: record: N {N} outside 1..{OBSTACLES_N_MAX}")
    return N


def map_heights(proj_indices: torch.Tensor, heights: torch.Tensor, record: torch.Tensor, band_mm=(100, 1500),
                exclude_cell: int = -1) -> torch.Tensor:
    """The per-cell record of the heights the pixels of a frame brought (eod_map_heights; include/eod_obstacles.h), in place.
    `proj_indices` int32, any shape, contiguous: the cell under each pixel.  `heights` float32, contiguous: the world y of each
    pixel in metres, either of the pixels' shape or `xyz` of shape [..., 3] (`unproject_grid_index(..., want_xyz=True)`), whose
    column 1 is then read with stride 3 and without a copy.  A pixel counts when its cell c has 0 <= c < N and c !=
    `exclude_cell` and its height is finite with |y| <= 1000; it then has q = rint(float32(y) * float32(1000)) millimetres and
    does hits[c] += 1, band_hits[c] += (band_mm[0] <= q <= band_mm[1]), h_min_mm[c] = min(.., q), h_max_mm[c] = max(.., q) on the
    planes of `record` int32 [4, N] (`new_height_record`).  `band_mm`: two ints, lo <= hi, within +-1 000 000
    (`RobotFrontEnd.height_band_mm`).  One launch, integer atomics only: the record depends neither on the order of the pixels or of
    the frames nor on how the pixels are split over calls.  Returns `record`."""
    if not isinstance(proj_indices, torch.Tensor) or proj_indices.dtype != torch.int32 or not proj_indices.is_contiguous():
        raise _lib.EodError(f"map_heights: proj_indices {_describe_what(proj_indices)}: expected contiguous int32")
    dev = proj_indices.device
    P = int(proj_indices.numel())
    if (not isinstance(heights, torch.Tensor) or heights.dtype != torch.float32 or not heights.is_contiguous() or heights.device != dev
            or (heights.numel() != P and (heights.dim() < 1 or heights.shape[-1] != 3 or heights.numel() != 3 * P))):
        raise _lib.EodError(f"map_heights: heights {_describe_what(heights)}: expected contiguous float32 with one value a pixel "
                            f"({P}) or xyz [..., 3], on the pixels' device")
    xyz = heights.numel() != P or (P == 0 and heights.dim() >= 1 and heights.shape[-1] == 3)
    N = _check_height_record("map_heights", record, dev)
    if P > OBSTACLES_PIXELS_MAX:
        raise _lib.EodError(f"map_heights: proj_indices: {P} pixels (at most {OBSTACLES_PIXELS_MAX})")
    try:
        lo, hi = band_mm
    except (TypeError, ValueError):
        lo = hi = None
    if not _whole(lo) or not _whole(hi) or not -OBSTACLES_BAND_MAX <= int(lo) <= int(hi) <= OBSTACLES_BAND_MAX:
        raise _lib.EodError(f"map_heights: band_mm {band_mm!r}: expected two ints lo <= hi within +-{OBSTACLES_BAND_MAX}")
    if not _whole(exclude_cell) or not -2 ** 31 <= int(exclude_cell) <= 2 ** 31 - 1:
        raise _lib.EodError(f"map_heights: exclude_cell {exclude_cell}: expected an int (-1: none)")
    if not record.is_cuda:
        raise _lib.EodError("map_heights: record on the host (no CPU fallback)")
    at = (heights.data_ptr() + (4 if xyz else 0)) if P else None
    check(_lib.load().eod_map_heights(proj_indices.data_ptr() if P else None, at, 3 if xyz else 1, P, N, int(lo), int(hi),
                                      int(exclude_cell), record[0].data_ptr(), record[1].data_ptr(), record[2].data_ptr(),
                                      record[3].data_ptr(), _stream()), "eod_map_heights")
    return record


def map_obstacles_workspace(N: int, cols: int) -> int:
    """int32 words of a `map_obstacles` workspace (eod_map_obstacles_workspace_bytes / 4)."""
    need = int(_lib.load().eod_map_obstacles_workspace_bytes(int(N), int(cols)))
    if need == 0:
        raise _lib.EodError(f"map_obstacles_workspace: N {N}, cols {cols}")
    return need // 4


def map_obstacles(record: torch.Tensor, cols: int, object_labels: Optional[torch.Tensor] = None, objects=None, min_hits: int = 4,
                  min_cells: int = 2, topk: int = 16, workspace: Optional[torch.Tensor] = None) -> dict:
    """Which cells something stands in, from the heights alone, merged with the detected objects (eod_map_obstacles; the semantics
    are those of include/eod_obstacles.h).  `record` int32 [4, N] of `map_heights`, cell i = r * cols + c.  A cell's `kind` (uint8
    [N]) is OBJECT 3 where `object_labels` (None or int32 [N]) is >= 0, else OBSTACLE 2 where band_hits >= `min_hits`, else CLEAR 1
    where hits > 0, else UNSEEN 0.  A structure is an 8-connected component of OBSTACLE cells, its label its lowest cell; one of
    fewer than `min_cells` cells is a speck.  Per cell `structure_labels` (specks included, -1 elsewhere) and `merged_labels`
    int32 [N]: the object's label, or the label of a structure that is no speck, or -1: the label map `map_route`,
    `map_clearance`, `map_sight` and `map_frontier` take as it stands.  `count` [1]: the structures of at least `min_cells` cells;
    for the `topk` (1..64) largest, `structure` (the label; -1 in a padding slot), `area`, `bbox` [K, 4], `sum_rc` int64 [K, 2],
    `top_mm` (the highest point, INT_MIN in a padding slot).  Per slot of `objects` (None, int32 [K_obj], K_obj <= 64, or a
    sequence; a cell belongs to the lowest slot that holds its label): `obj_cells`, `obj_seen_cells` (those with hits > 0),
    `obj_top_mm` and `obj_base_mm` over the seen ones (INT_MIN / INT_MAX if none).  `counts` int32 [6]: UNSEEN, CLEAR, OBSTACLE and
    OBJECT cells, structures (specks included), speck cells; `status` int32 [2] (bit 1 of status[0]: a bounded loop reached its
    bound), which is not read here.  `workspace`: int32, 8-byte aligned, at least `map_obstacles_workspace(N, cols)` words, any
    contents.  Integer comparisons, additions and atomics only: the same bits on every call; `record` is not written."""
    N = _check_height_record("map_obstacles", record)
    dev = record.device
    if not _whole(cols) or int(cols) < 1 or N % int(cols) != 0:
        raise _lib.EodError(f"map_obstacles: cols {cols} does not divide the {N} cells")
    if int(cols) > OBSTACLES_DIM_MAX or N // int(cols) > OBSTACLES_DIM_MAX:
        raise _lib.EodError(f"map_obstacles: cols {cols}: {N // int(cols)} rows x {cols} columns, more than {OBSTACLES_DIM_MAX} one way")
    if object_labels is not None and (not isinstance(object_labels, torch.Tensor) or object_labels.shape != (N,)
                                      or object_labels.dtype != torch.int32 or not object_labels.is_contiguous()
                                      or object_labels.device != dev):
        raise _lib.EodError(f"map_obstacles: object_labels {_describe_what(object_labels)}: expected None or contiguous int32 [{N}] on "
                            "the record's device")
    if objects is not None and not isinstance(objects, torch.Tensor):
        try:
            objects = torch.as_tensor(np.asarray(list(objects), dtype=np.int64).astype(np.int32).reshape(-1), device=dev)
        except (TypeError, ValueError, OverflowError):
            raise _lib.EodError(f"map_obstacles: objects {type(objects).__name__}: expected None, int32 [K_obj] or a sequence of "
                                "labels") from None
    if objects is not None and (objects.dim() != 1 or objects.dtype != torch.int32 or not objects.is_contiguous()
                                or objects.device != dev or objects.shape[0] > OBSTACLES_K_MAX):
        raise _lib.EodError(f"map_obstacles: objects {_describe_what(objects)}: expected contiguous int32 [K_obj], K_obj <= "
                            f"{OBSTACLES_K_MAX}, on the record's device")
    for name, v in (("min_hits", min_hits), ("min_cells", min_cells)):
        if not _whole(v) or not 1 <= int(v) <= 2 ** 31 - 1:
            raise _lib.EodError(f"map_obstacles: {name} {v}: expected at least 1")
    if not _whole(topk) or not 1 <= int(topk) <= OBSTACLES_TOPK_MAX:
        raise _lib.EodError(f"map_obstacles: topk {topk} outside 1..{OBSTACLES_TOPK_MAX}")
    if not record.is_cuda:
        raise _lib.EodError("map_obstacles: record on the host (no CPU fallback)")
    need = map_obstacles_workspace(N, int(cols))
    if workspace is not None and (not isinstance(workspace, torch.Tensor) or workspace.dtype != torch.int32 or workspace.dim() != 1
                                  or not workspace.is_contiguous() or workspace.numel() < need or workspace.device != dev
                                  or workspace.data_ptr() % 8 != 0):
        raise _lib.EodError(f"map_obstacles: workspace: expected {need} contiguous, 8-byte aligned int32 on the record's device")
    if workspace is None:
        workspace = torch.empty((need,), dtype=torch.int32, device=dev)
    K, Ko = int(topk), 0 if objects is None else int(objects.shape[0])
    kind = torch.empty((N,), dtype=torch.uint8, device=dev)
    cells = torch.empty((2, N), dtype=torch.int32, device=dev)        # structure_labels, merged_labels
    sum_rc = torch.empty((K, 2), dtype=torch.int64, device=dev)
    out = torch.empty((7 * K + 4 * Ko + 9,), dtype=torch.int32, device=dev)
    part = {}
    at = 0
    for name, n, shape in (("count", 1, (1,)), ("structure", K, (K,)), ("area", K, (K,)), ("bbox", 4 * K, (K, 4)), ("top_mm", K, (K,)),
                           ("obj_cells", Ko, (Ko,)), ("obj_seen_cells", Ko, (Ko,)), ("obj_top_mm", Ko, (Ko,)),
                           ("obj_base_mm", Ko, (Ko,)), ("counts", 6, (6,)), ("status", 2, (2,))):
        part[name] = out[at:at + n].view(shape)
        at += n
    obj = lambda name: part[name].data_ptr() if Ko else None
    check(_lib.load().eod_map_obstacles(
        record[0].data_ptr(), record[1].data_ptr(), record[2].data_ptr(), record[3].data_ptr(), _ptr(object_labels),
        objects.data_ptr() if Ko else None, N, int(cols), Ko, int(min_hits), int(min_cells), K, kind.data_ptr(), cells[0].data_ptr(),
        cells[1].data_ptr(), part["count"].data_ptr(), part["structure"].data_ptr(), part["area"].data_ptr(), part["bbox"].data_ptr(),
        sum_rc.data_ptr(), part["top_mm"].data_ptr(), obj("obj_cells"), obj("obj_seen_cells"), obj("obj_top_mm"), obj("obj_base_mm"),
        part["counts"].data_ptr(), part["status"].data_ptr(), workspace.data_ptr(), workspace.numel() * 4, _stream()), "eod_map_obstacles")
    return {"kind": kind, "structure_labels": cells[0], "merged_labels": cells[1], "count": part["count"],
            "structure": part["structure"], "area": part["area"], "bbox": part["bbox"], "sum_rc": sum_rc, "top_mm": part["top_mm"],
            "obj_cells": part["obj_cells"], "obj_seen_cells": part["obj_seen_cells"], "obj_top_mm": part["obj_top_mm"],
            "obj_base_mm": part["obj_base_mm"], "counts": part["counts"], "status": part["status"]}


ROOMS_K_MAX, ROOMS_P_MAX, ROOMS_TOPK_MAX, ROOMS_N_MAX, ROOMS_DIM_MAX, ROOMS_SWEEPS_MAX = 64, 64, 64, 1 << 22, 32767, 1024
ROOMS_UNASSIGNED = 2 ** 31 - 1                           # grow_dist of a cell that is in no room


def map_rooms_workspace(N: int, cols: int) -> int:
    """int32 words of a `map_rooms` workspace (eod_map_rooms_workspace_bytes / 4)."""
    need = int(_lib.load().eod_map_rooms_workspace_bytes(int(N), int(cols)))
    if need == 0:
        raise _lib.EodError(f"map_rooms_workspace: N {N}, cols {cols}")
    return need // 4


def map_rooms(labels: torch.Tensor, d2: torch.Tensor, cols: int, door_r2: int, min_cells: int = 1, topk: int = 16, objects=None,
              passable=None, known: Optional[torch.Tensor] = None, sweeps: Optional[int] = None,
              workspace: Optional[torch.Tensor] = None) -> dict:
    """The free space of a label map split at its doorways, and the objects by room (eod_map_rooms; the semantics are those of
    include/eod_rooms.h).  `labels` int32 [N], cell i = r * cols + c: `obs["merged_labels"]` of `map_obstacles` or any other label
    map; `d2` int32 [N]: `d2` of `map_clearance` on the same `labels` and `passable` (it is not recomputed here).  A cell is BLOCKED
    when its label is >= 0 and not one of `passable` (None, or int32 [P], P <= 64, or a sequence), VOID when it is not blocked and
    `known` (None or uint8 [N]; `obs["kind"]` fits) is 0 there, FREE otherwise.  A free cell with d2 > `door_r2` is CORE; a
    4-connected region of core cells with at least `min_cells` cells is a room, its label its lowest cell; every free cell goes to
    the room that reaches it at the smallest cost of `map_route`'s moves (the lowest label on a tie).  Returns per cell
    `room_labels` (-1: blocked, void, unassigned) and `grow_dist` int32 [N] (0 on a room's core, INT_MAX where unassigned);
    `count` [1]: the rooms; for the `topk` (1..64) largest by area, `room` (the label; -1 in a padding slot), `area`, `core_area`,
    `bbox` [K, 4], `sum_rc` int64 [K, 2], `widest_key` int64 [K], `widest_d2`, `widest_cell` (the most open cell: where to stand),
    `room_objects`; between ranked rooms `door_edges` [K, K], `door_key` int64 [K, K], `door_d2`, `door_cell` [K, K]
    (`door_cell[a, b]`: the cell of a in the middle of the door to b; -1: none); per slot of `objects` (None, int32 [K_obj],
    K_obj <= 64, or a sequence; a cell belongs to the lowest slot that holds its label) `obj_room_cells` [K_obj, K] (the cells of
    room s beside the object), `obj_room` (the slot with the most; -1) and `obj_room_label`; `counts` int32 [6]: blocked, void,
    free, core cells of rooms, grown cells, unassigned free cells; `status` int32 [2]: status[0] bit 0: the `sweeps` (1..1024;
    None: `map_route_sweeps`) ran out before the keys had settled, bit 1: a bounded loop reached its bound; it is not read here,
    so nothing synchronises.  `workspace`: int32, 8-byte aligned, at least `map_rooms_workspace(N, cols)` words, any contents.
    Integer comparisons, additions and atomics only: at status 0 the same bits on every call."""
    if not isinstance(labels, torch.Tensor) or labels.dim() != 1 or labels.dtype != torch.int32 or not labels.is_contiguous():
        raise _lib.EodError(f"map_rooms: labels {_describe_what(labels)}: expected contiguous int32 [N]")
    N = int(labels.shape[0])
    if not 1 <= N <= ROOMS_N_MAX:
        raise _lib.EodError(f"map_rooms: labels: N {N} outside 1..{ROOMS_N_MAX}")
    dev = labels.device
    if (not isinstance(d2, torch.Tensor) or tuple(d2.shape) != (N,) or d2.dtype != torch.int32 or not d2.is_contiguous()
            or d2.device != dev):
        raise _lib.EodError(f"map_rooms: d2 {_describe_what(d2)}: expected contiguous int32 [{N}] on the labels' device (the d2 of "
                            "map_clearance)")
    if not _whole(cols) or int(cols) < 1 or N % int(cols) != 0:
        raise _lib.EodError(f"map_rooms: cols {cols} does not divide the {N} cells")
    if int(cols) > ROOMS_DIM_MAX or N // int(cols) > ROOMS_DIM_MAX:
        raise _lib.EodError(f"map_rooms: cols {cols}: {N // int(cols)} rows x {cols} columns, more than {ROOMS_DIM_MAX} one way")
    if not _whole(door_r2) or not 0 <= int(door_r2) <= 2 ** 31 - 1:
        raise _lib.EodError(f"map_rooms: door_r2 {door_r2}: expected at least 0 (RobotFrontEnd.door_r2)")
    if not _whole(min_cells) or not 1 <= int(min_cells) <= 2 ** 31 - 1:
        raise _lib.EodError(f"map_rooms: min_cells {min_cells}: expected at least 1")
    if not _whole(topk) or not 1 <= int(topk) <= ROOMS_TOPK_MAX:
        raise _lib.EodError(f"map_rooms: topk {topk} outside 1..{ROOMS_TOPK_MAX}")
    lists = {}
    for name, v, cap in (("objects", objects, ROOMS_K_MAX), ("passable", passable, ROOMS_P_MAX)):
        if v is not None and not isinstance(v, torch.Tensor):
            try:
                v = torch.as_tensor(np.asarray(list(v), dtype=np.int64).astype(np.int32).reshape(-1), device=dev)
            except (TypeError, ValueError, OverflowError):
                raise _lib.EodError(f"map_rooms: {name} {type(v).__name__}: expected None, int32 [n] or a sequence of labels") from None
        if v is not None and (v.dim() != 1 or v.dtype != torch.int32 or not v.is_contiguous() or v.device != dev or v.shape[0] > cap):
            raise _lib.EodError(f"map_rooms: {name} {_describe_what(v)}: expected contiguous int32 [n], n <= {cap}, on the labels' device")
        lists[name] = v
    objects, passable = lists["objects"], lists["passable"]
    if known is not None and (not isinstance(known, torch.Tensor) or tuple(known.shape) != (N,) or known.dtype != torch.uint8
                              or not known.is_contiguous() or known.device != dev):
        raise _lib.EodError(f"map_rooms: known {_describe_what(known)}: expected None or contiguous uint8 [{N}] on the labels' device")
    if sweeps is None:
        sweeps = map_route_sweeps(N // int(cols), int(cols))
    if not _whole(sweeps) or not 1 <= int(sweeps) <= ROOMS_SWEEPS_MAX:
        raise _lib.EodError(f"map_rooms: sweeps {sweeps} outside 1..{ROOMS_SWEEPS_MAX}")
    if not labels.is_cuda:
        raise _lib.EodError("map_rooms: labels on the host (no CPU fallback)")
    need = map_rooms_workspace(N, int(cols))
    if workspace is not None and (not isinstance(workspace, torch.Tensor) or workspace.dtype != torch.int32 or workspace.dim() != 1
                                  or not workspace.is_contiguous() or workspace.numel() < need or workspace.device != dev
                                  or workspace.data_ptr() % 8 != 0):
        raise _lib.EodError(f"map_rooms: workspace: expected {need} contiguous, 8-byte aligned int32 on the labels' device")
    if workspace is None:
        workspace = torch.empty((need,), dtype=torch.int32, device=dev)
    K = int(topk)
    Ko, P = 0 if objects is None else int(objects.shape[0]), 0 if passable is None else int(passable.shape[0])
    cells = torch.empty((2, N), dtype=torch.int32, device=dev)        # room_labels, grow_dist
    wide = torch.empty((3 * K + K * K,), dtype=torch.int64, device=dev)
    sum_rc, widest_key, door_key = wide[:2 * K].view(K, 2), wide[2 * K:3 * K], wide[3 * K:].view(K, K)
    out = torch.empty((10 * K + 3 * K * K + Ko * K + 2 * Ko + 9,), dtype=torch.int32, device=dev)
    part = {}
    at = 0
    for name, n, shape in (("count", 1, (1,)), ("room", K, (K,)), ("area", K, (K,)), ("core_area", K, (K,)), ("bbox", 4 * K, (K, 4)),
                           ("widest_d2", K, (K,)), ("widest_cell", K, (K,)), ("room_objects", K, (K,)), ("door_edges", K * K, (K, K)),
                           ("door_d2", K * K, (K, K)), ("door_cell", K * K, (K, K)), ("obj_room_cells", Ko * K, (Ko, K)),
                           ("obj_room", Ko, (Ko,)), ("obj_room_label", Ko, (Ko,)), ("counts", 6, (6,)), ("status", 2, (2,))):
        part[name] = out[at:at + n].view(shape)
        at += n
    obj = lambda name: part[name].data_ptr() if Ko else None
    check(_lib.load().eod_map_rooms(
        labels.data_ptr(), passable.data_ptr() if P else None, d2.data_ptr(), _ptr(known), objects.data_ptr() if Ko else None, N, P,
        int(cols), Ko, int(door_r2), int(min_cells), K, int(sweeps), cells[0].data_ptr(), cells[1].data_ptr(), part["count"].data_ptr(),
        part["room"].data_ptr(), part["area"].data_ptr(), part["core_area"].data_ptr(), part["bbox"].data_ptr(), sum_rc.data_ptr(),
        widest_key.data_ptr(), part["widest_d2"].data_ptr(), part["widest_cell"].data_ptr(), part["room_objects"].data_ptr(),
        part["door_edges"].data_ptr(), door_key.data_ptr(), part["door_d2"].data_ptr(), part["door_cell"].data_ptr(),
        obj("obj_room_cells"), obj("obj_room"), obj("obj_room_label"), part["counts"].data_ptr(), part["status"].data_ptr(),
        workspace.data_ptr(), workspace.numel() * 4, _stream()), "eod_map_rooms")
    return {"room_labels": cells[0], "grow_dist": cells[1], "count": part["count"], "room": part["room"], "area": part["area"],
            "core_area": part["core_area"], "bbox": part["bbox"], "sum_rc": sum_rc, "widest_key": widest_key,
            "widest_d2": part["widest_d2"], "widest_cell": part["widest_cell"], "room_objects": part["room_objects"],
            "door_edges": part["door_edges"], "door_key": door_key, "door_d2": part["door_d2"], "door_cell": part["door_cell"],
            "obj_room_cells": part["obj_room_cells"], "obj_room": part["obj_room"], "obj_room_label": part["obj_room_label"],
            "counts": part["counts"], "status": part["status"]}
