"""CPU side of test_training_launches_gpu.py: the recorder of the non-convolution entry points and the references of ROIAlign written
out in torch at a chosen precision (float64 = reference, float32 = yardstick).  Nothing here touches a GPU by itself."""
import math
from typing import Dict, List, Sequence, Tuple

import torch

from _conv_cases import SENTINEL    # noqa: F401  (re-exported: one sentinel for the launch modules)

U = 2.0 ** -24                      # fp32 unit round-off


# ------------------------------------------------------------------------------------------------
# recording: which entry point was called with which arguments
# ------------------------------------------------------------------------------------------------
class Recorder:
    """Wraps the Python-level entry points of `ops` and three ctypes-level ones of the loaded library for the duration of a `with`
    block.  `calls[family][key]` = payload of the first call with those arguments (`key`: shapes, counts, flags, which optional
    pointers were given); ROIAlign payloads collect the host copies of the first box lists they met (the cascade's three stages)."""
    KEEP_BOXES = 3

    def __init__(self, inference: bool = False):
        """`inference`: also wrap the entry points only the inference frame calls (tests/_inference_cases.py lists them); without it
        the recorder is the training module's, call for call."""
        self.calls: Dict[str, Dict[tuple, dict]] = {}
        self._undo = []
        self.inference = inference

    def note(self, family: str, key: tuple, **payload) -> dict:
        fam = self.calls.setdefault(family, {})
        if key not in fam:
            fam[key] = dict(payload, n=0)
        fam[key]["n"] += 1
        return fam[key]

    def _patch(self, owner, name: str, make):
        orig = getattr(owner, name)
        setattr(owner, name, make(orig))
        self._undo.append((owner, name, orig))

    def __enter__(self):
        from embodied_object_detection_amd import _lib, ops
        rec = self

        def roi_align(orig):
            def f(p3, p4, p5, h3, w3, Cc, boxes, count, R_cap, S, out=None, box_rows=None, batch=1, boxes_per_image=0, refine=None):
                r = orig(p3, p4, p5, h3, w3, Cc, boxes, count, R_cap, S, out=out, box_rows=box_rows, batch=batch,
                         boxes_per_image=boxes_per_image, refine=refine)
                e = rec.note("roi_align", (int(h3), int(w3), int(Cc), int(R_cap), int(S), count is not None, box_rows is not None, int(batch),
                                           refine is not None), boxes=[])
                if len(e["boxes"]) < rec.KEEP_BOXES and refine is None and box_rows is None:
                    e["boxes"].append(boxes.detach().float().cpu().reshape(-1, 4)[:R_cap].clone())
                return r
            return f

        def roi_align_backward(orig):
            def f(dp3, dp4, dp5, h3, w3, Cc, boxes, count, R_cap, S, g):
                e = rec.note("roi_align_backward", (int(h3), int(w3), int(Cc), int(R_cap), int(S), count is not None), boxes=[])
                if len(e["boxes"]) < rec.KEEP_BOXES:
                    e["boxes"].append(boxes.detach().float().cpu().reshape(-1, 4)[:R_cap].clone())
                return orig(dp3, dp4, dp5, h3, w3, Cc, boxes, count, R_cap, S, g)
            return f

        def groupnorm_relu(orig):
            def f(x, gamma, beta, level_off, Cc, stats, groups=32, eps=1e-5, out=None, partial_ready=False):
                rec.note("groupnorm_relu", (tuple(int(o) for o in level_off), int(Cc), int(groups), float(eps), bool(partial_ready), out is not None))
                return orig(x, gamma, beta, level_off, Cc, stats, groups=groups, eps=eps, out=out, partial_ready=partial_ready)
            return f

        def groupnorm_relu_backward(orig):
            def f(x, y, dy, gamma, level_off, Cc, fwd_stats, groups=32, eps=1e-5):
                rec.note("groupnorm_relu_backward", (tuple(int(o) for o in level_off), int(Cc), int(groups), float(eps)))
                return orig(x, y, dy, gamma, level_off, Cc, fwd_stats, groups=groups, eps=eps)
            return f

        def projector_backward(orig):
            def f(self, grads, pooled_f16, H, W, weight, need_input_grad=True):
                rec.note("memory_projector_backward", (int(H), int(W), float(weight), bool(need_input_grad)))
                return orig(self, grads, pooled_f16, H, W, weight, need_input_grad=need_input_grad)
            return f

        def memory_gather_pool(orig):
            def f(mem_f16, proj, H, W, out=None, err=None, torch_order=False, batch=1):
                rec.note("memory_gather_pool", (int(H), int(W), int(mem_f16.shape[-2]), int(mem_f16.shape[-1]), bool(torch_order), int(batch),
                                                out is not None, err is not None))
                return orig(mem_f16, proj, H, W, out=out, err=err, torch_order=torch_order, batch=batch)
            return f

        def zs_logits(orig):
            def f(feat, zs, temp=50.0, ld=None, featn_out=None):
                r = orig(feat, zs, temp, ld=ld, featn_out=featn_out)
                rec.note("zs_logits", (int(feat.shape[0]), int(zs.shape[1]), int(r.shape[1]), float(temp), featn_out is not None))
                return r
            return f

        def zs_logits_backward(orig):
            def f(feat, zs, d_logits, temp=50.0):
                rec.note("zs_logits_backward", (int(d_logits.shape[0]), int(zs.shape[1]), int(d_logits.shape[1]), float(temp)))
                return orig(feat, zs, d_logits, temp)
            return f

        def nonfinite(orig):
            def f(self, grads, flag):
                rec.note("nonfinite", tuple(-1 if g is None else int(g.numel()) for g in grads))
                return orig(self, grads, flag)
            return f

        for name, make in (("roi_align", roi_align), ("roi_align_backward", roi_align_backward), ("groupnorm_relu", groupnorm_relu),
                           ("groupnorm_relu_backward", groupnorm_relu_backward), ("memory_gather_pool", memory_gather_pool),
                           ("zs_logits", zs_logits), ("zs_logits_backward", zs_logits_backward)):
            self._patch(ops, name, make)
        self._patch(ops.MemoryProjectorBackward, "__call__", projector_backward)
        self._patch(ops.AdamW, "nonfinite", nonfinite)
        if self.inference:
            self._enter_inference(ops)

        # ctypes level: an attribute on the loaded library object shadows the exported function for everybody who goes through it
        lib = _lib.load()

        def relu_backward(orig):
            def f(g, y, out, n, stream):
                rec.note("relu_backward", (int(n),))
                return orig(g, y, out, n, stream)
            return f

        def upsample2_sum_backward(orig):
            def f(g, out, N, h, w, Cc, accumulate, stream):
                rec.note("upsample2_sum_backward", (int(N), int(h), int(w), int(Cc), int(accumulate)))
                return orig(g, out, N, h, w, Cc, accumulate, stream)
            return f

        def maxpool_backward(orig):
            def f(x, y, g, dx, N, H, W, Cc, OH, OW, stream):
                rec.note("maxpool3x3s2_backward", (int(N), int(H), int(W), int(Cc), int(OH), int(OW)))
                return orig(x, y, g, dx, N, H, W, Cc, OH, OW, stream)
            return f

        for name, make in (("eod_relu_backward", relu_backward), ("eod_upsample2_sum_backward", upsample2_sum_backward),
                           ("eod_maxpool3x3s2_backward", maxpool_backward)):
            self._patch(lib, name, make)
        return self

    def _enter_inference(self, ops):
        """The entry points of the inference frame that the training step does not call (or calls with other arguments).  Every key
        is (shapes, capacities, flags, which optional pointers were given, batch); the paste keeps host copies of the first few real
        box / row lists it was given (they are replayed)."""
        rec = self

        def given(*ts):
            return tuple(t is not None for t in ts)

        def host(t, n=None):
            return None if t is None else (t.detach().cpu().clone() if n is None else t.detach().cpu()[:n].clone())

        def preprocess_image(orig):
            def f(img, mean, std, div=32, out=None):
                rec.note("preprocess_image", (int(img.shape[1]), int(img.shape[2]), int(div), out is not None),
                         mean=tuple(float(v) for v in mean), std=tuple(float(v) for v in std))
                return orig(img, mean, std, div=div, out=out)
            return f

        def maxpool3x3s2(orig):
            def f(x, N, H, W, Cc):
                rec.note("maxpool3x3s2", (int(N), int(H), int(W), int(Cc)))
                return orig(x, N, H, W, Cc)
            return f

        def proposals(orig):
            def f(self, head_out):
                d = self.desc
                sizes = tuple(self.level_off[l + 1] - self.level_off[l] for l in range(d.levels))
                rec.note("proposals", (sizes, tuple(int(d.level_w[l]) for l in range(d.levels)), int(d.pre_nms_topk), int(d.post_nms_topk),
                                           int(d.cap), int(d.batch), int(d.head_stride)),
                             strides=tuple(int(d.level_stride[l]) for l in range(d.levels)), scales=tuple(float(d.level_scale[l]) for l in range(d.levels)),
                             score_thresh=float(d.score_thresh), nms_thresh=float(d.nms_thresh))
                return orig(self, head_out)
            return f

        def zs_classify(orig):
            def f(feat, zs, prob_acc, accumulate, featn_out, count, R_cap, C1, temp=50.0, zs_mem=None, prop_scores=None, mem_scores_out=None,
                  final_inv_stages=0.0, batch=1, wide=False):
                rec.note("zs_classify", (int(R_cap), int(C1), bool(accumulate), float(temp), float(final_inv_stages), int(batch), bool(wide))
                         + given(featn_out, count, zs_mem, prop_scores, mem_scores_out))
                return orig(feat, zs, prob_acc, accumulate, featn_out, count, R_cap, C1, temp, zs_mem=zs_mem, prop_scores=prop_scores,
                            mem_scores_out=mem_scores_out, final_inv_stages=final_inv_stages, batch=batch, wide=wide)
            return f

        def cascade_stage_tail(orig):
            def f(feat, zs, prob_acc, accumulate, featn_out, count, R_cap, C1, temp, hb, bb2, boxes_in, boxes_out, weights, clip, img_w, img_h,
                  zs_mem=None, prop_scores=None, mem_scores_out=None, final_inv_stages=0.0, deltas_out=None, batch=1, wide=False):
                rec.note("cascade_stage_tail", (int(R_cap), int(C1), bool(accumulate), float(temp), float(final_inv_stages), int(batch), bool(wide),
                                                tuple(float(w) for w in weights), bool(clip), float(img_w), float(img_h))
                         + given(featn_out, count, zs_mem, prop_scores, mem_scores_out, deltas_out))
                return orig(feat, zs, prob_acc, accumulate, featn_out, count, R_cap, C1, temp, hb, bb2, boxes_in, boxes_out, weights, clip,
                            img_w, img_h, zs_mem=zs_mem, prop_scores=prop_scores, mem_scores_out=mem_scores_out,
                            final_inv_stages=final_inv_stages, deltas_out=deltas_out, batch=batch, wide=wide)
            return f

        def apply_deltas(orig):
            def f(deltas, ld, boxes, out, count, R_cap, weights, clip, img_w, img_h, batch=1):
                rec.note("apply_deltas", (int(ld), int(R_cap), tuple(float(w) for w in weights), bool(clip), float(img_w), float(img_h), int(batch),
                                          count is not None))
                return orig(deltas, ld, boxes, out, count, R_cap, weights, clip, img_w, img_h, batch=batch)
            return f

        def memory_scores(orig):
            def f(featn, zs, prop_scores, scores_out, count, R_cap, C1):
                rec.note("memory_scores", (int(R_cap), int(C1), count is not None))
                return orig(featn, zs, prop_scores, scores_out, count, R_cap, C1)
            return f

        def selector(orig):
            def f(self, boxes, scores, count, img_w, img_h, score_thresh, nms_thresh):
                rec.note("detection_selector", (int(self.R_cap), int(self.C1), int(self.topk), int(self.batch), self.uniq_rows is not None,
                                                self.rep_of is not None, float(img_w), float(img_h), float(score_thresh), float(nms_thresh),
                                                count is not None))
                return orig(self, boxes, scores, count, img_w, img_h, score_thresh, nms_thresh)
            return f

        def mask_predictor_sigmoid(orig):
            def f(x, w, bias, rows, Cc, count, unit_rows, out=None, out_units=None):
                rec.note("mask_predictor_sigmoid", (int(rows), int(Cc), int(unit_rows)) + given(count, out, out_units))
                return orig(x, w, bias, rows, Cc, count, unit_rows, out=out, out_units=out_units)
            return f

        def detector_postprocess(orig):
            def f(boxes, scores, classes, count, cap, sx, sy, out_w, out_h, ob, os_, oc, osrc, ocount, remap=None, batch=1):
                rec.note("detector_postprocess", (int(cap), float(sx), float(sy), float(out_w), float(out_h), remap is not None, int(batch),
                                                  count is not None))
                return orig(boxes, scores, classes, count, cap, sx, sy, out_w, out_h, ob, os_, oc, osrc, ocount, remap=remap, batch=batch)
            return f

        def paste_masks(orig):
            def f(prob, boxes, rows, count, K_cap, H, W, thr, out, batch=1, prob_units=0):
                e = rec.note("paste_masks", (int(K_cap), int(H), int(W), float(thr), int(batch), int(prob_units)) + given(rows, count), lists=[])
                if len(e["lists"]) < rec.KEEP_BOXES:
                    n = batch * K_cap
                    e["lists"].append(dict(boxes=host(boxes.reshape(-1, 4), n), rows=host(rows, n), count=host(count)))
                return orig(prob, boxes, rows, count, K_cap, H, W, thr, out, batch=batch, prob_units=prob_units)
            return f

        def unproject_grid_index(orig):
            def f(depth, T, intr, proj_shift, map_shift, cell, map_w, map_h, order=0, want_xyz=False):
                rec.note("unproject_grid_index", (int(depth.shape[0]), int(depth.shape[1]), int(map_w), int(map_h), int(order), bool(want_xyz)),
                         cell=float(cell), intr=tuple(float(v) for v in intr))
                return orig(depth, T, intr, proj_shift, map_shift, cell, map_w, map_h, order, want_xyz)
            return f

        def memory_normalize_f16(orig):
            def f(mem, obs, out=None):
                rec.note("memory_normalize_f16", (int(mem.shape[0]), int(mem.shape[1]), out is not None))
                return orig(mem, obs, out=out)
            return f

        def memory_normalize_dirty_f16(orig):
            def f(mem, obs, dirty, out):
                rec.note("memory_normalize_dirty_f16", (int(mem.shape[0]), int(mem.shape[1])))
                return orig(mem, obs, dirty, out)
            return f

        def projector(orig):
            def f(self, pooled_f16, feats, H, W, weight, mode, batch=1):
                rec.note("memory_projector", (int(H), int(W), float(weight), str(mode), int(batch)))
                return orig(self, pooled_f16, feats, H, W, weight, mode, batch=batch)
            return f

        def writer(orig):
            def f(self, featn, prop_boxes, prop_masks, det_rows, det_count, proj, mem, obs, dirty=None, err=None, snapshot=None):
                d = self.desc
                rec.note("memory_writer", (int(d.H), int(d.W), int(d.n_cells), int(d.K_cap), int(d.R_cap), int(d.batch), float(d.mask_thresh))
                         + given(dirty, err, snapshot))
                return orig(self, featn, prop_boxes, prop_masks, det_rows, det_count, proj, mem, obs, dirty=dirty, err=err, snapshot=snapshot)
            return f

        def concat_lists(orig):
            def f(lists, counts, cap_in, id_stride, batch, out, out_count):
                rec.note("concat_lists", (int(cap_in), int(id_stride), int(batch)))
                return orig(lists, counts, cap_in, id_stride, batch, out, out_count)
            return f

        def semmap_labels(orig):
            def f(mem, obs, zs, thresh):
                rec.note("semmap_labels", (int(mem.shape[0]), int(mem.shape[1]), int(zs.shape[1]), float(thresh)))
                return orig(mem, obs, zs, thresh)
            return f

        for name, make in (("preprocess_image", preprocess_image), ("maxpool3x3s2", maxpool3x3s2), ("zs_classify", zs_classify),
                           ("cascade_stage_tail", cascade_stage_tail), ("apply_deltas", apply_deltas), ("memory_scores", memory_scores),
                           ("mask_predictor_sigmoid", mask_predictor_sigmoid), ("detector_postprocess", detector_postprocess),
                           ("paste_masks", paste_masks), ("unproject_grid_index", unproject_grid_index),
                           ("memory_normalize_f16", memory_normalize_f16), ("memory_normalize_dirty_f16", memory_normalize_dirty_f16),
                           ("concat_lists", concat_lists), ("semmap_labels", semmap_labels)):
            self._patch(ops, name, make)
        self._patch(ops.ProposalDecoder, "__call__", proposals)
        self._patch(ops.DetectionSelector, "__call__", selector)
        self._patch(ops.MemoryProjector, "__call__", projector)
        self._patch(ops.MemoryWriter, "__call__", writer)

    def __exit__(self, *exc):
        for owner, name, orig in reversed(self._undo):
            setattr(owner, name, orig)
        self._undo = []
        return False


# ------------------------------------------------------------------------------------------------
# ROIAlignV2 (aligned, sampling_ratio 0) over P3..P5 at a chosen precision
# ------------------------------------------------------------------------------------------------
SCALES = (1.0 / 8, 1.0 / 16, 1.0 / 32)


def roi_geometry(boxes: torch.Tensor, S: int):
    """The DISCRETE decisions of the pooler, taken in fp32 as upstream takes them (they are part of the operation, not of its
    rounding): level of every box (`assign_boxes_to_levels`) and its sampling grid (gh, gw) = ceil(roi extent / S) on the fp32
    quotient.  -> (levels int64 [R], gh [R], gw [R]); gh or gw <= 0: the ROI pools zeros and has no gradient."""
    from oracle import ops as OO
    b = boxes.float()
    # a box inverted along one axis has a negative area and no level (NaN); it pools zeros on whatever level: the finest here
    inverted = ((b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])) < 0
    lv = OO.assign_boxes_to_levels(torch.where(inverted[:, None], torch.zeros_like(b), b))
    sc = torch.tensor(SCALES, dtype=torch.float32)[lv]
    bs = b * sc[:, None] - 0.5
    gh = torch.ceil((bs[:, 3] - bs[:, 1]) / S)
    gw = torch.ceil((bs[:, 2] - bs[:, 0]) / S)
    bad = ~(torch.isfinite(gh) & torch.isfinite(gw))
    gh[bad], gw[bad] = 0, 0
    return lv, gh.long(), gw.long()


def _axis(lo, bin_, g: int, S: int, extent: int, dtype) -> torch.Tensor:
    """A [S, extent]: summed bilinear weight of the g samples of every bin on every feature index along one axis, with the
    clamps and the validity rule of torchvision's bilinear_interpolate as oracle/ops.py `_bilinear` states them."""
    ph = torch.arange(S, dtype=dtype)
    i = torch.arange(g, dtype=dtype)
    v = lo + ph[:, None] * bin_ + (i[None, :] + 0.5) * bin_ / g                      # [S, g]
    valid = ~((v < -1.0) | (v > extent))
    v = v.clamp(min=0)
    low = v.to(torch.int64)
    top = low >= extent - 1
    high = torch.where(top, torch.full_like(low, extent - 1), low + 1)
    low = torch.where(top, torch.full_like(low, extent - 1), low)
    v = torch.where(top, low.to(dtype), v)
    l = v - low.to(dtype)
    h = 1.0 - l
    A = torch.zeros((S, extent), dtype=dtype)
    rows = torch.arange(S)[:, None].expand(S, g)
    A.index_put_((rows[valid], low[valid]), h[valid], accumulate=True)
    A.index_put_((rows[valid], high[valid]), l[valid], accumulate=True)
    return A


class RoiRef:
    """ROIAlign of a box list at `dtype`: per ROI the two axis matrices (the bilinear weights of a sample are a product of a y and an
    x weight, and a sample is dropped when EITHER coordinate is out of range, so the double sum over a bin's samples factors
    exactly); `forward` and `adjoint` apply them.  test_roi_reference_is_the_oracles_roi_align ties both to oracle/ops.py."""

    def __init__(self, boxes: torch.Tensor, S: int, shapes: Sequence[Tuple[int, int]], dtype):
        self.S, self.shapes, self.dtype = S, list(shapes), dtype
        self.lv, gh, gw = roi_geometry(boxes, S)
        self.rois = []
        for r in range(boxes.shape[0]):
            l = int(self.lv[r])
            H, W = self.shapes[l]
            if gh[r] <= 0 or gw[r] <= 0:
                self.rois.append(None)
                continue
            # fp32: the oracle's own arithmetic (box * scale - 0.5 in fp32); float64: the same formula on the fp32 boxes, unrounded
            bs = boxes[r].to(dtype) * SCALES[l] - 0.5
            Ay = _axis(bs[1], (bs[3] - bs[1]) / S, int(gh[r]), S, H, dtype)
            Ax = _axis(bs[0], (bs[2] - bs[0]) / S, int(gw[r]), S, W, dtype)
            ys, xs = Ay.any(0).nonzero().flatten(), Ax.any(0).nonzero().flatten()
            if ys.numel() == 0 or xs.numel() == 0:
                self.rois.append(None)
                continue
            y0, y1, x0, x1 = int(ys[0]), int(ys[-1]) + 1, int(xs[0]), int(xs[-1]) + 1
            self.rois.append((l, y0, y1, x0, x1, Ay[:, y0:y1].contiguous(), Ax[:, x0:x1].contiguous(), float(int(gh[r]) * int(gw[r]))))

    def forward(self, feats: Sequence[torch.Tensor], indicator: bool = False) -> torch.Tensor:
        """feats[l] [h, w, C] -> [R, S, S, C].  `indicator`: every non-zero weight counted as 1 and no division by the sample count
        (the sum of the cells a bin touches: the magnitude the bounds are scaled by)."""
        C = feats[0].shape[-1]
        out = torch.zeros((len(self.rois), self.S, self.S, C), dtype=self.dtype)
        for r, roi in enumerate(self.rois):
            if roi is None:
                continue
            l, y0, y1, x0, x1, Ay, Ax, cnt = roi
            if indicator:
                Ay, Ax, cnt = (Ay != 0).to(self.dtype), (Ax != 0).to(self.dtype), 1.0
            out[r] = torch.einsum("py,qx,yxc->pqc", Ay, Ax, feats[l][y0:y1, x0:x1].to(self.dtype)) / cnt
        return out

    def adjoint(self, g: torch.Tensor, indicator: bool = False) -> List[torch.Tensor]:
        """g [R, S, S, C] -> the gradient of every level [h, w, C] (the transpose of `forward`)."""
        C = g.shape[-1]
        d = [torch.zeros((h, w, C), dtype=self.dtype) for h, w in self.shapes]
        for r, roi in enumerate(self.rois):
            if roi is None:
                continue
            l, y0, y1, x0, x1, Ay, Ax, cnt = roi
            if indicator:
                Ay, Ax, cnt = (Ay != 0).to(self.dtype), (Ax != 0).to(self.dtype), 1.0
            d[l][y0:y1, x0:x1] += torch.einsum("py,qx,pqc->yxc", Ay, Ax, g[r].to(self.dtype)) / cnt
        return d

    def reach(self) -> List[torch.Tensor]:
        """Per level [h, w]: how many (ROI, bin) pairs add into the cell."""
        n = [torch.zeros((h, w), dtype=torch.float64) for h, w in self.shapes]
        for roi in self.rois:
            if roi is not None:
                l, y0, y1, x0, x1, Ay, Ax, _ = roi
                n[l][y0:y1, x0:x1] += torch.outer((Ay != 0).sum(0).double(), (Ax != 0).sum(0).double())
        return n


ROI_HEAD = 2.0          # head-room over the first-order bounds of the ROIAlign comparisons


def roi_forward_reference(boxes: torch.Tensor, S: int, shapes: Sequence[Tuple[int, int]], feats: Sequence[torch.Tensor]):
    """ROIAlign of `boxes` over one image's pyramid in float64 -> (RoiRef, pooled [R,S,S,C], element-wise bound on an fp32 kernel's
    error).  The bound is test_training_launches_gpu.py's `_roi_bound` per ROI: 8 U 2^ceil(log2 E) for the roundings of the sample
    coordinates on a level of extent E plus n U for adding the n cells a bin touches, times the sum T of the magnitudes those cells
    hold, times ROI_HEAD."""
    rr = RoiRef(boxes, S, shapes, torch.float64)
    ref, T = rr.forward(feats), rr.forward([f.abs() for f in feats], indicator=True)
    R = boxes.shape[0]
    n = torch.zeros((R, S, S, 1), dtype=torch.float64)
    ext = torch.ones((R, 1, 1, 1), dtype=torch.float64)
    for r, roi in enumerate(rr.rois):
        if roi is not None:
            n[r, :, :, 0] = torch.outer((roi[5] != 0).sum(1).double(), (roi[6] != 0).sum(1).double())
            ext[r] = 2.0 ** math.ceil(math.log2(max(shapes[roi[0]])))
    return rr, ref, ROI_HEAD * U * (8.0 * ext + n) * T


def hostile_boxes(H: int, W: int, rows: int, seed: int) -> torch.Tensor:
    """A box list built to hurt the footprint arithmetic of the ROIAlign kernels on an H x W image: boxes touching and crossing all
    four borders, zero-width / zero-height / inverted boxes, boxes exactly on the level thresholds of `assign_boxes_to_levels`
    (sqrt(area) = 224 and 448: exactly, and within an fp32 rounding of it), boxes of less than one cell of their level, one box over the whole image, and seeded boxes of 6 ..
    400 px for the rest.  Coordinates are off the 1/8-pixel lattice where a sample could land exactly on -1 or on the extent, where
    fp32 and float64 legitimately decide differently whether the sample counts."""
    fx = [[0.0, 0.0, W, H],                                          # the whole image (level 5)
          [0.0, 0.0, 37.3, 41.9], [W - 33.7, 0.0, W, 29.1], [0.0, H - 45.3, 51.7, H], [W - 61.1, H - 57.7, W, H],      # touching the corners
          [-23.3, 50.3, 40.9, 122.7], [W - 48.1, 77.7, W + 31.3, 160.3], [91.3, -19.1, 170.7, 44.3], [203.1, H - 39.3, 290.9, H + 27.7],
          [-150.3, -120.7, 160.9, 170.3], [W - 140.7, H - 170.1, W + 190.3, H + 130.9],                               # crossing two borders
          [-60.3, -44.1, -10.7, -3.3], [W + 12.3, 40.1, W + 90.7, 133.3],                                              # wholly outside
          [120.0, 80.0, 120.0, 160.0], [200.0, 150.0, 260.0, 150.0], [300.0, 300.0, 300.0, 300.0],                    # zero width / height / both
          [180.3, 90.1, 150.7, 140.9], [240.1, 220.3, 300.7, 190.1], [0.0, 0.0, 0.0, 0.0],                             # inverted; the clip's corner
          [32.0, 48.0, 256.0, 272.0], [16.0, 32.0, 464.0, 144.0], [17.1, 33.3, 17.1 + 448.0, 33.3 + 112.0],            # sqrt(area) = 224
          [16.0, 16.0, 464.0, 464.0], [64.0, 40.0, 576.0, 432.0], [61.3, 40.7, 61.3 + 512.0, 40.7 + 392.0],            # sqrt(area) = 448
          [100.3, 100.7, 103.1, 102.9], [301.7, 55.3, 302.9, 61.1], [415.1, 200.3, 421.3, 200.9],                      # less than one cell
          [8.0, 8.0, 16.0, 16.0], [160.0, 160.0, 168.0, 168.0]]                                                       # exactly one cell
    g = torch.Generator().manual_seed(seed)
    n = rows - len(fx)
    assert n >= 0
    ctr = torch.rand((n, 2), generator=g) * torch.tensor([float(W), float(H)])
    half = torch.exp(torch.rand((n, 2), generator=g) * 4.0 + 1.8)
    rnd = torch.cat([ctr - half, ctr + half], dim=1)
    rnd[::3] = torch.stack([rnd[::3, 0].clamp(0, W), rnd[::3, 1].clamp(0, H), rnd[::3, 2].clamp(0, W), rnd[::3, 3].clamp(0, H)], dim=1)
    return torch.cat([torch.tensor(fx, dtype=torch.float32), rnd.float()]).contiguous()


def fragments_to_rows(buf: torch.Tensor, H: int, W: int) -> List[torch.Tensor]:
    """The pooled operand of the memory read ([level][32-row tile][k-step][hi][r][8], every level padded to whole tiles) -> the
    row-major [P_l, 512] rows of the three levels."""
    out, t0 = [], 0
    flat = buf.reshape(-1)
    for s in (8, 16, 32):
        rows = (H // s) * (W // s)
        tiles = (rows + 31) // 32
        blk = flat[t0 * 32 * 512:(t0 + tiles) * 32 * 512].view(tiles, 32, 2, 32, 8)
        out.append(blk.permute(0, 3, 1, 2, 4).reshape(tiles * 32, 512)[:rows])
        t0 += tiles
    return out
