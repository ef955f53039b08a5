"""DeticCascadeROIHeads (inference) on the HIP kernels.

Mirrors `_forward_box/_run_stage/_create_proposals_from_boxes/forward/forward_mask_memory`
(`Detic/detic/modeling/roi_heads/detic_roi_heads.py:88-349`), detectron2's `ROIPooler`(ROIAlignV2),
`FastRCNNConvFCHead`, `MaskRCNNConvUpsampleHead`, `Box2BoxTransform`, `fast_rcnn_inference`,
`DeticFastRCNNOutputLayers.forward/predict_probs` (`detic_fast_rcnn.py:437-466,325-339`) and `ZeroShotClassifier.forward`
(`zero_shot_classifier.py:71-111`).  ROI lists have a fixed capacity and a device-side count; there is no host sync
anywhere in here.
"""
from __future__ import annotations

from typing import Dict, List, Tuple

import torch

from .. import ops
from ..registry import ROI_HEADS_REGISTRY


RESULT_SETS = 3     # detection-list sets: frame t's detection pass may still read set t % 3 while later cascades write the others


class RoiBuffers:
    """The ROI half's persistent activations for B scenes of R proposals, and the batch geometry its launches are told.

    One scene (`lockstep=False`, the heads' own instance): every launch is the plain single-image call -- `batch` 1, no
    `boxes_per_image`, no `m_segments`, no `plan_rows`, ROI lists passed as they are.  Lock-step (`LockstepScenes`, any B >= 1):
    the B scenes' rows back to back, `batch` = B, per-scene counts (`m_segments`), every layer planned like ONE scene while
    `plan_like_single` holds, and the scenes' ROI lists concatenated into one list of global indices (`roi_list`)."""

    def __init__(self, heads: "DeticCascadeROIHeads", B: int, lockstep: bool):
        R, D, dev = heads.R, heads.topk, heads.device
        f32 = dict(dtype=torch.float32, device=dev)
        self.device, self.B, self.R, self.D, self.rows = dev, B, R, D, B * R
        self.lockstep = lockstep
        self.batch, self.m_segments = (B, B) if lockstep else (1, 0)
        # True: every layer is planned like ONE scene (same split-K slabs / wave split, same summation order): each scene's results are
        # bitwise those of its own single-scene run.  False: layers are planned for the rows the batched launch really has (fewer
        # slabs and reduce launches, 64x64 tiles instead of the wave-split kernel on the B x R rows of the FC layers): the same
        # arithmetic in another summation order -- results agree with the single-scene run like two fp32 implementations do
        # (tests/test_fullsize_gpu.py::test_lockstep_planned_for_the_batch_agrees_within_tolerance)
        self.plan_like_single = True
        self.pool7 = torch.empty((B * R, 7, 7, 256), **f32)
        self.h1 = torch.empty((B * R, 1, 1, 1024), **f32)
        self.h2 = torch.empty((B * R, 1, 1, 1024), **f32)
        self.hb = torch.empty((B * R, 1, 1, 1024), **f32)
        self.feat = torch.empty((B * R, 1, 1, 512), **f32)
        self.feat0 = torch.empty((B * R, 1, 1, 512), **f32)        # stage-0 CLIP-space feature = proposals.feat
        self.featn0 = torch.zeros((B * R, 512), **f32)            # 50 * normalize(feat0): what the memory stores
        self.deltas = torch.empty((B * R, 1, 1, 4), **f32)
        self.prob = torch.zeros((B * R, heads.C1), **f32)
        self.boxes = [torch.zeros((B * R, 4), **f32) for _ in range(heads.num_stages + 1)]
        # mask-pass activations (pool, conv ping-pong, deconv output of the two-launch tail).  One scene: one set for both passes,
        # sized for all R proposals, and a second one once the proposal pass runs on its own stream (`proposal_pass_buffers`).
        # Lock-step: a set per pass over the concatenated lists (<= 100 unique memory rows per scene), no deconv output.
        self.Pcap = min(R, 128) if lockstep else R
        if lockstep:
            self.mask_bufs = (torch.empty((B * D, 14, 14, 256), **f32), torch.empty((B * D, 14, 14, 256), **f32), None)
            i32 = dict(dtype=torch.int32, device=dev)
            self.glist_p, self.total_p = torch.zeros((B * R,), **i32), torch.zeros((1,), **i32)
            self.glist_d = [torch.zeros((B * D,), **i32) for _ in range(RESULT_SETS)]
            self.total_d = [torch.zeros((1,), **i32) for _ in range(RESULT_SETS)]
            self._identity = None
        else:
            M = max(R, heads.Dcap)
            self.mask_bufs = (torch.empty((M, 14, 14, 256), **f32), torch.empty((M, 14, 14, 256), **f32),
                              torch.empty((M, 28, 28, 256), **f32))
        self.det_masks = torch.zeros((B * heads.Dcap, 28, 28), **f32)
        self.prop_masks = torch.zeros((B * R, 28, 28), **f32)
        self._prop_bufs = None

    TENSORS = ("pool7", "h1", "h2", "hb", "feat", "feat0", "featn0", "deltas", "prob", "boxes", "det_masks", "prop_masks")

    def expose_on(self, owner) -> None:
        """The tensors under their own names on `owner` (what tests and tools read); again after `set_width`."""
        for name in self.TENSORS:
            setattr(owner, name, getattr(self, name))

    def set_width(self, C1: int) -> None:
        self.prob = torch.zeros((self.rows, C1), dtype=torch.float32, device=self.device)

    def plan_rows(self, rows: int) -> int:
        """EodConvDesc.plan_rows of a layer whose launch holds `rows` rows per scene."""
        return rows if (self.lockstep and self.plan_like_single) else 0

    def per_scene(self, n: int) -> int:
        """`boxes_per_image` / `prob_units` of a launch over buffers that hold `n` entries per scene (0: one image, not used)."""
        return n if self.lockstep else 0

    def proposal_pass_buffers(self):
        """Own activation buffers for the proposal mask pass, so that it can run concurrently with the box cascade / the
        detection pass."""
        if self._prop_bufs is None:
            f32 = dict(dtype=torch.float32, device=self.device)
            n = self.B * self.Pcap
            self._prop_bufs = (torch.empty((n, 14, 14, 256), **f32), torch.empty((n, 14, 14, 256), **f32),
                               None if self.lockstep else torch.empty((n, 28, 28, 256), **f32))
        return self._prop_bufs

    def roi_list(self, lists, counts, cap_in: int, slot: int = None):
        """The ROI list a mask pass runs over -> (rows, count).  One scene: the list as it is (`lists` None: the first `counts[0]`
        boxes).  Lock-step: the scenes' lists concatenated as global indices b * cap_in + lists[b][k], into the proposal list
        (`slot` None) or detection-list set `slot`."""
        if not self.lockstep:
            return lists, counts
        if lists is None:
            if self._identity is None:
                self._identity = torch.arange(cap_in, dtype=torch.int32, device=self.device).repeat(self.B)
            lists = self._identity
        out = (self.glist_p, self.total_p) if slot is None else (self.glist_d[slot], self.total_d[slot])
        return ops.concat_lists(lists, counts, cap_in, cap_in, self.B, out[0], out[1])


@ROI_HEADS_REGISTRY.register()
class DeticCascadeROIHeads:
    def __init__(self, cfg, sd: Dict[str, torch.Tensor], device, prop_cap: int):
        self.device = device
        rb = cfg.MODEL.ROI_BOX_HEAD
        if not (rb.USE_ZEROSHOT_CLS and rb.CLS_AGNOSTIC_BBOX_REG and rb.USE_SIGMOID_CE and rb.MULT_PROPOSAL_SCORE):
            raise NotImplementedError("hot path covers the zero-shot, class-agnostic, sigmoid, mult-proposal-score cascade")
        if rb.NUM_FC != 2 or rb.POOLER_RESOLUTION != 7 or cfg.MODEL.ROI_MASK_HEAD.POOLER_RESOLUTION != 14:
            raise NotImplementedError("unsupported ROI head geometry")
        if not cfg.MODEL.ROI_MASK_HEAD.CLS_AGNOSTIC_MASK or cfg.MODEL.ROI_MASK_HEAD.NUM_CONV != 4:
            raise NotImplementedError("unsupported mask head")
        # the class count is the classifier matrix's (RESET_CLS_TESTS / TEST_NUM_CLASSES swap it before construction, `reset_cls_test`
        # after it), not cfg.MODEL.ROI_HEADS.NUM_CLASSES: utils.py:32-50 sets roi_heads.num_classes the same way
        self.C1 = int(sd["roi_heads.box_predictor.0.cls_score.zs_weight"].shape[1])
        self.num_classes = self.C1 - 1
        if not 1 <= self.num_classes <= ops.ZS_WIDE_MAX_C1 - 1:
            raise NotImplementedError(f"{self.num_classes} classes: the HIP path covers 1 to {ops.ZS_WIDE_MAX_C1 - 1}")
        self.norm_temp = float(rb.NORM_TEMP)
        self.norm_weight = bool(rb.NORM_WEIGHT)
        self.cascade_weights = [tuple(float(v) for v in w) for w in cfg.MODEL.ROI_BOX_CASCADE_HEAD.BBOX_REG_WEIGHTS]
        self.num_stages = len(self.cascade_weights)
        self.score_thresh = float(cfg.MODEL.ROI_HEADS.SCORE_THRESH_TEST)
        self.nms_thresh = float(cfg.MODEL.ROI_HEADS.NMS_THRESH_TEST)
        self.topk = int(cfg.TEST.DETECTIONS_PER_IMAGE)
        self.add_feature_to_prop = bool(rb.ADD_FEATURE_TO_PROP)
        self.R = prop_cap                       # proposal capacity
        self.Dcap = (self.topk + 31) // 32 * 32  # detection capacity for the mask head
        self.stages = []
        for k in range(self.num_stages):
            fc1_w = sd[f"roi_heads.box_head.{k}.fc1.weight"]
            # flatten order: reference (C,7,7) -> ours (7,7,C)
            fc1_w = fc1_w.view(-1, 256, 7, 7).permute(0, 2, 3, 1).reshape(fc1_w.shape[0], -1, 1, 1).contiguous()
            p = f"roi_heads.box_predictor.{k}"
            st = dict(
                fc1=ops.Conv(fc1_w, sd[f"roi_heads.box_head.{k}.fc1.bias"], device=device, name=f"box_head.{k}.fc1"),
                fc2=ops.Conv(sd[f"roi_heads.box_head.{k}.fc2.weight"][:, :, None, None], sd[f"roi_heads.box_head.{k}.fc2.bias"],
                             device=device, name=f"box_head.{k}.fc2"),
                cls=ops.Conv(sd[f"{p}.cls_score.linear.weight"][:, :, None, None], sd[f"{p}.cls_score.linear.bias"], device=device,
                             name=f"box_predictor.{k}.cls_score.linear"),
                bb0=ops.Conv(sd[f"{p}.bbox_pred.0.weight"][:, :, None, None], sd[f"{p}.bbox_pred.0.bias"], device=device,
                             name=f"box_predictor.{k}.bbox_pred.0"),
                bb2=ops.Conv(sd[f"{p}.bbox_pred.2.weight"][:, :, None, None], sd[f"{p}.bbox_pred.2.bias"], device=device,
                             name=f"box_predictor.{k}.bbox_pred.2"),
                zs=sd[f"{p}.cls_score.zs_weight"].contiguous().to(device),
            )
            # cls_score.linear (1024 -> 512, no ReLU) and bbox_pred.0 (1024 -> 1024, ReLU) read the same fc2 output: one GEMM with
            # the weights stacked, two outputs (EodConvDesc.split_n); each output column walks K as in the separate call
            st["cls_bb0"] = ops.Conv(torch.cat([sd[f"{p}.cls_score.linear.weight"], sd[f"{p}.bbox_pred.0.weight"]], dim=0)[:, :, None, None],
                                     torch.cat([sd[f"{p}.cls_score.linear.bias"], sd[f"{p}.bbox_pred.0.bias"]], dim=0), device=device,
                                     name=f"box_predictor.{k}.cls_score.linear+bbox_pred.0")
            assert st["zs"].shape == (512, self.C1), (st["zs"].shape, self.C1)
            self.stages.append(st)
        m = "roi_heads.mask_head"
        self.mask_convs = [ops.Conv(sd[f"{m}.mask_fcn{i}.weight"], sd[f"{m}.mask_fcn{i}.bias"], pad=1, device=device, name=f"mask_fcn{i}")
                           for i in range(1, 5)]
        # EodConvDesc.prefetch2 (two chunks of operands in flight) was built for these launches (~40 / ~90 ROIs leave 2-5 workgroups
        # on a CU) and measured slower at every size (tools/conv_bench.py propmask: 43 ROIs 128 against 121 us, 100 ROIs 254
        # against 229, 300 ROIs 688 against 644; whole frame 273 against 281 frames/s): off; EOD_MASK_PREFETCH2=1 turns it on
        for conv in self.mask_convs:
            conv.prefetch2 = int(__import__("os").environ.get("EOD_MASK_PREFETCH2", "0"))
        self.deconv = ops.Conv(sd[f"{m}.deconv.weight"], sd[f"{m}.deconv.bias"], device=device, deconv=True, name="mask_deconv")
        self.pred_w = sd[f"{m}.predictor.weight"].reshape(-1).contiguous().to(device)
        self.pred_b = float(sd[f"{m}.predictor.bias"].item())
        self.bufs = RoiBuffers(self, 1, lockstep=False)        # the single scene's activations, under the heads' own names too
        self.bufs.expose_on(self)
        # deconv + ReLU + predictor + sigmoid in ONE launch (the [rois,28,28,256] activation never goes to memory); False keeps
        # the two-launch form (used by the tests as the cross-check)
        self.fuse_mask_tail = True
        self.merge_cls_bb0 = True     # False: the two linear layers as two launches (tests: bitwise the same results)
        # classifier tail + bbox_pred.2 + apply_deltas of a stage in one launch (`eod_cascade_stage_tail`); False: three launches
        # (bbox_pred.2 then on the matrix cores: the deltas agree to fp32 summation order, ~1e-7 relative)
        self.fuse_stage_tail = True
        # True: the next stage's ROIAlign applies the deltas on load (EodBoxRefine: one launch less per stage, bitwise the same
        # results).  Measured in the frame (tools/knob_ab.py, same call): 287.1 frames/s against 288.6 with apply_deltas as its own
        # 5 us launch -- every one of the ROIAlign's 12 544 waves redoes the box arithmetic behind a dependent load: off.
        self.fold_deltas = False
        # experiment: the cascade's 21 launches as two captured hipGraphs (stage 0, stages 1-2), replayed (see forward_box).
        # Measured in the frame (tools/knob_ab.py, same call, then as one graph): 286.0 frames/s against 286.1 with stream
        # launches -- the launch boundaries on the GPU are drain + dispatch beside the other streams' kernels, which a graph
        # does not remove, and the host is not the limit: off.
        self.graph_cascade = False
        self._graphs = {}
        # LDS reserve of the DETECTION mask pass's launches (the pass that trails under the frame's / the next frame's latency-bound
        # chains): see EodConvDesc.lds_reserve.  0 = the kernel's natural occupancy.
        self.det_pass_lds_reserve = int(__import__("os").environ.get("EOD_DET_LDS_RESERVE", "0"))
        self.prop_pass_lds_reserve = int(__import__("os").environ.get("EOD_PROP_LDS_RESERVE", "0"))
        self.selectors = [ops.DetectionSelector(self.R, self.C1, self.topk, device, groups=True) for _ in range(RESULT_SETS)]
        self.selector = self.selectors[0]

    def set_classifier(self, zs: torch.Tensor) -> None:
        """`reset_cls_test` on the built heads: `zs` [512, C + 1] (background column included) replaces the three stages' class
        matrices; the score buffer and the selectors follow its width.  Everything else (weights, activations, boxes) stays."""
        zs = zs.to(dtype=torch.float32).contiguous().to(self.device)
        if zs.dim() != 2 or zs.shape[0] != 512 or not 2 <= zs.shape[1] <= ops.ZS_WIDE_MAX_C1:
            raise ValueError(f"classifier matrix {tuple(zs.shape)}: expected [512, C + 1] with 1 <= C <= {ops.ZS_WIDE_MAX_C1 - 1}")
        for st in self.stages:
            st["zs"] = zs
        if zs.shape[1] != self.C1:
            self.C1 = int(zs.shape[1])
            self.num_classes = self.C1 - 1
            self.bufs.set_width(self.C1)
            self.bufs.expose_on(self)
            self.selectors = [ops.DetectionSelector(self.R, self.C1, self.topk, self.device, groups=True) for _ in range(RESULT_SETS)]
            self.selector = self.selectors[0]
        self._graphs = {}

    # ---- cascade box heads ------------------------------------------------------------------------
    def forward_box(self, views: List[torch.Tensor], shapes, prop_boxes: torch.Tensor, prop_scores: torch.Tensor, count: torch.Tensor,
                    image_hw: Tuple[int, int], sel: int = 0, mem_rescore=None, after_stage0=None):
        """`mem_rescore = (zs_weight of the meta-architecture, out [R, C1])`: stage 0's classifier launch also writes the memory
        update's CLIP re-score of the proposals (custom_rcnn.py:838-861).
        `after_stage0` (optional callable): called once stage 0's classifier launch is enqueued, before stages 1-2.  Everything the
        memory side reads (`featn0`, the re-score, the proposal boxes) is final there and no later stage writes it, so the frame's
        critical chain (memory selection -> proposal masks -> memory write) branches off at this point and does not wait for the
        refined boxes, which only the detections need."""
        h3, w3 = shapes[0]
        H, W = image_hw
        R = self.R
        if self.graph_cascade:
            # Experiment (`graph_cascade`): the cascade's 21 launches as TWO hipGraphs per (pyramid set, inputs) combination -- stage 0
            # and stages 1-2, so that `after_stage0` fires between the replays as it does between the launches -- captured on first
            # use and replayed.  Every buffer of the segments is static; the events around them stay outside the graphs.
            key = (views[0].data_ptr(), prop_boxes.data_ptr(), prop_scores.data_ptr(), count.data_ptr(), mem_rescore is not None, H, W)
            gs = self._graphs.get(key)
            if gs is None:
                self._cascade(views, shapes, prop_boxes, prop_scores, count, image_hw, mem_rescore)     # eager once: workspaces exist
                gs = []
                carry = (prop_boxes, None)
                for part in (range(0, 1), range(1, self.num_stages)):
                    g = torch.cuda.CUDAGraph()
                    with torch.cuda.graph(g):
                        carry = self._cascade(views, shapes, prop_boxes, prop_scores, count, image_hw, mem_rescore, part, carry)
                    gs.append(g)
                self._graphs[key] = gs
            gs[0].replay()
            if after_stage0 is not None:
                after_stage0()
            gs[1].replay()
            boxes = self.boxes[self.num_stages]
        else:
            boxes, _ = self._cascade(views, shapes, prop_boxes, prop_scores, count, image_hw, mem_rescore, after_stage0=after_stage0)
        self.last_selector = self.selectors[sel]
        return self.selectors[sel](boxes, self.prob, count, float(W), float(H), self.score_thresh, self.nms_thresh)

    def fuses_mem_rescore(self, zs_mem: torch.Tensor) -> bool:
        """Stage 0's classifier launch writes the memory's CLIP re-score as well only when both class matrices are narrow and
        equally wide (the narrow kernel stages one after the other in the same LDS); otherwise `ops.memory_scores` runs."""
        return self.C1 <= ops.ZS_MAX_C1 and int(zs_mem.shape[1]) == self.C1

    def _cascade(self, views, shapes, prop_boxes, prop_scores, count, image_hw, mem_rescore, part=None, carry=None, after_stage0=None,
                 g: RoiBuffers = None):
        """The cascade stages `part` (default: all three; detic_roi_heads.py:88-175) on the buffers `g` (default: the heads' own single
        scene) -> (the boxes buffer they end on, `pending`), which is also the `carry` a later part starts from; scores land in
        `g.prob`.  `after_stage0`: see `forward_box`."""
        g = g if g is not None else self.bufs
        h3, w3 = shapes[0]
        H, W = image_hw
        R, rows, batch, segs = self.R, g.rows, g.batch, g.m_segments
        bpi, pr = g.per_scene(R), g.plan_rows(R)
        if mem_rescore is not None and not self.fuses_mem_rescore(mem_rescore[0]):
            mem_rescore = None
        # pending (`fold_deltas`): regression weights of the deltas that the next ROIAlign applies to `boxes` on load
        boxes, pending = carry if carry is not None else (prop_boxes, None)
        for k in (part if part is not None else range(self.num_stages)):
            st = self.stages[k]
            # pending: next-stage proposals = apply_deltas(boxes, deltas) clipped to the image (detic_roi_heads.py:314) are computed by
            # the ROIAlign launch itself (EodBoxRefine) and stored to boxes[k] -- one launch less per stage on the frame's chain
            refine = None if pending is None else (g.deltas, 4, pending, True, float(W), float(H), g.boxes[k])
            ops.roi_align(views[0], views[1], views[2], h3, w3, 256, boxes, count, rows, 7, out=g.pool7, batch=batch,
                          boxes_per_image=bpi, refine=refine)
            if pending is not None:
                boxes, pending = g.boxes[k], None
            # the FC layers are ONE GEMM over the scenes' rows, with per-scene counts (EodConvDesc.m_segments)
            st["fc1"](g.pool7, rows, 1, 1, relu=True, m_count=count, m_unit=1, out=g.h1, m_segments=segs, plan_rows=pr)
            st["fc2"](g.h1, rows, 1, 1, relu=True, m_count=count, m_unit=1, out=g.h2, m_segments=segs, plan_rows=pr)
            feat = g.feat0 if k == 0 else g.feat
            if self.merge_cls_bb0:
                st["cls_bb0"](g.h2, rows, 1, 1, relu=True, m_count=count, m_unit=1, out=feat, split=(512, g.hb), m_segments=segs,
                              plan_rows=pr)
            else:
                st["cls"](g.h2, rows, 1, 1, m_count=count, m_unit=1, out=feat, m_segments=segs, plan_rows=pr)
            last = k == self.num_stages - 1
            # the memory update's CLIP re-score rides on stage 0's classifier launch (`fuses_mem_rescore`)
            rescore = mem_rescore if k == 0 else None
            if self.fuse_stage_tail and self.merge_cls_bb0 and not self.fold_deltas:
                # classifier tail + bbox_pred.2 + apply_deltas as ONE launch (two launch boundaries less per stage on the cascade's
                # chain); the last stage's launch also fuses the cascade's scores (detic_roi_heads.py:164-173)
                ops.cascade_stage_tail(feat, st["zs"], g.prob, k > 0, g.featn0 if k == 0 else None, count, R, self.C1, self.norm_temp,
                                       g.hb, st["bb2"], boxes, g.boxes[k + 1], self.cascade_weights[k], not last, float(W), float(H),
                                       zs_mem=rescore[0] if rescore is not None else None,
                                       prop_scores=prop_scores if (last or rescore is not None) else None,
                                       mem_scores_out=rescore[1] if rescore is not None else None,
                                       final_inv_stages=1.0 / self.num_stages if last else 0.0, deltas_out=g.deltas, batch=batch,
                                       wide=True)
                boxes = g.boxes[k + 1]
                if k == 0 and after_stage0 is not None:
                    after_stage0()
                continue
            # the last stage's launch also fuses the cascade's scores: sqrt(mean_k(prob) * proposal score) (detic_roi_heads.py:164-173)
            ops.zs_classify(feat, st["zs"], g.prob, k > 0, g.featn0 if k == 0 else None, count, R, self.C1, self.norm_temp,
                            zs_mem=rescore[0] if rescore is not None else None,
                            prop_scores=prop_scores if (last or rescore is not None) else None,
                            mem_scores_out=rescore[1] if rescore is not None else None,
                            final_inv_stages=1.0 / self.num_stages if last else 0.0, batch=batch, wide=True)
            if k == 0 and after_stage0 is not None:
                after_stage0()      # bbox_pred.2 and apply_deltas of stage 0 feed stage 1 only
            if not self.merge_cls_bb0:
                st["bb0"](g.h2, rows, 1, 1, relu=True, m_count=count, m_unit=1, out=g.hb, m_segments=segs, plan_rows=pr)
            st["bb2"](g.hb, rows, 1, 1, m_count=count, m_unit=1, out=g.deltas, m_segments=segs, plan_rows=pr)
            # next-stage proposals are clipped to the image (detic_roi_heads.py:314); the final boxes are clipped by
            # fast_rcnn_inference itself
            if self.fold_deltas and not last:
                pending = self.cascade_weights[k]
            else:
                ops.apply_deltas(g.deltas, 4, boxes, g.boxes[k + 1], count, R, self.cascade_weights[k], not last, float(W), float(H),
                                 batch=batch)
                boxes = g.boxes[k + 1]
        return boxes, pending

    # ---- mask head ----------------------------------------------------------------------------------
    def forward_mask(self, views, shapes, boxes: torch.Tensor, count: torch.Tensor, cap: int, out: torch.Tensor,
                     rows: torch.Tensor = None, bufs=None, lds_reserve: int = 0, tag=None, g: RoiBuffers = None,
                     boxes_per_image: int = 0):
        """Mask head on `count` ROIs, at most `cap` per scene.  With `rows` (a compact ascending list of box indices) ROI k pools
        `boxes[rows[k]]` and its 28x28 mask is written to `out[rows[k]]`: only the listed boxes are computed, the output layout stays
        per-box.  Lock-step buffers `g`: `rows` / `count` are the scenes' concatenated list (`RoiBuffers.roi_list`) over `boxes`,
        which holds `boxes_per_image` boxes per scene; box j is pooled from image j // boxes_per_image."""
        g = g if g is not None else self.bufs
        h3, w3 = shapes[0]
        mpool, mbuf, mup = bufs if bufs is not None else g.mask_bufs
        if not self.fuse_mask_tail and mup is None:
            raise NotImplementedError("fuse_mask_tail = False: the lock-step buffers hold no deconv output; run the two-launch mask tail "
                                      "on the single-scene model")
        cap, pr = g.B * cap, g.plan_rows(cap * 196)
        ops.roi_align(views[0], views[1], views[2], h3, w3, 256, boxes, count, cap, 14, out=mpool, box_rows=rows, batch=g.batch,
                      boxes_per_image=g.per_scene(boxes_per_image))
        src, dst = mpool, mbuf
        self.deconv.lds_reserve = lds_reserve
        for conv in self.mask_convs:
            conv.lds_reserve = lds_reserve          # occupancy cap of the dense launches (EodConvDesc.lds_reserve)
            conv.event_tag = tag
            conv(src, cap, 14, 14, relu=True, m_count=count, m_unit=196, out=dst, plan_rows=pr)
            src, dst = dst, src
        if self.fuse_mask_tail:
            self.deconv(src, cap, 14, 14, relu=True, m_count=count, m_unit=196, out=out, fuse=(self.pred_w, self.pred_b, rows),
                        plan_rows=pr)
        else:
            self.deconv(src, cap, 14, 14, relu=True, m_count=count, m_unit=196, out=mup, plan_rows=pr)
            ops.mask_predictor_sigmoid(mup, self.pred_w, self.pred_b, cap * 784, 256, count, 784, out=out, out_units=rows)
        return out

    def forward(self, views, shapes, prop_boxes, prop_scores, prop_count, image_hw):
        """-> detections (boxes, scores, classes, rows, count) + det masks; proposals get feat/featn and masks."""
        det = self.forward_box(views, shapes, prop_boxes, prop_scores, prop_count, image_hw)
        det_boxes, det_scores, det_classes, det_rows, det_count = det
        self.forward_mask(views, shapes, det_boxes, det_count, self.topk, self.det_masks)      # forward_with_given_boxes
        return det

    def forward_mask_memory(self, views, shapes, prop_boxes, prop_count, rows: torch.Tensor = None, rows_count: torch.Tensor = None,
                            bufs=None, tag=None, g: RoiBuffers = None, lds_reserve: int = None):
        """`forward_mask_memory` + `mask_rcnn_inference` on ALL proposals (custom_rcnn.py:573-574).

        `rows` / `rows_count`: lazy variant -- only the proposals the memory update will read (custom_rcnn.py:875-880) get a
        mask; every other proposal's mask is dead in the reference (never read after `inference_with_proposals`).  With the
        lock-step buffers `g` they are the scenes' lists (`mem_selector.uniq_rows` / `uniq_count`), concatenated here."""
        g = g if g is not None else self.bufs
        lds = self.prop_pass_lds_reserve if lds_reserve is None else lds_reserve
        if rows is not None:
            rows, rows_count = g.roi_list(rows, rows_count, self.R)
            return self.forward_mask(views, shapes, prop_boxes, rows_count, min(self.R, 128), g.prop_masks, rows=rows, bufs=bufs,
                                     lds_reserve=lds, tag=tag, g=g, boxes_per_image=self.R)
        return self.forward_mask(views, shapes, prop_boxes, prop_count, self.R, g.prop_masks, bufs=bufs, lds_reserve=lds, tag=tag, g=g,
                                 boxes_per_image=self.R)

    # ---- detections: masks, post-processing, paste ----------------------------------------------------
    def detection_masks(self, g: RoiBuffers, views, shapes, sel, slot: int, dedup: bool, lds_reserve: int, tag=None):
        """`forward_with_given_boxes` (detic_roi_heads.py:257): the mask head on the detections `sel` (a `DetectionSelector` after its
        call) of g.B scenes -- once per distinct box when `dedup` (the groups come from the detection selection's launch)."""
        rows, count = g.roi_list(sel.rep_list, sel.rep_count, self.topk, slot) if dedup else g.roi_list(None, sel.count, self.topk, slot)
        return self.forward_mask(views, shapes, sel.boxes, count, self.topk, g.det_masks, rows=rows, lds_reserve=lds_reserve, tag=tag,
                                 g=g, boxes_per_image=self.topk)

    def postprocess_and_paste(self, g: RoiBuffers, sel, post: dict, image_hw, mask_threshold: float, dedup: bool):
        """`detector_postprocess` + paste (custom_rcnn.py:579-580) of g.B scenes' detections into result set `post`, at the input
        size (output size != input size is not used on this path, train_mp3d.py:487-490)."""
        H, W = image_hw
        B, D, dev = g.B, self.topk, self.device
        # this frame's own result tensors, from the caching allocator on the stream that fills them; `materialize` slices them
        post["boxes"] = torch.empty((B * D, 4), dtype=torch.float32, device=dev)
        post["scores"] = torch.empty((B * D,), dtype=torch.float32, device=dev)
        post["classes"] = torch.empty((B * D,), dtype=torch.int32, device=dev)
        post["masks"] = torch.empty((B, D, H, W), dtype=torch.uint8, device=dev)
        ops.detector_postprocess(sel.boxes, sel.scores, sel.classes, sel.count, D, 1.0, 1.0, float(W), float(H), post["boxes"],
                                 post["scores"], post["classes"], post["src"], post["count"], remap=sel.rep_of if dedup else None,
                                 batch=g.batch)
        ops.paste_masks(g.det_masks, post["boxes"], post["src"], post["count"], D, H, W, mask_threshold, post["masks"], batch=g.batch,
                        prob_units=g.per_scene(D))

    def detection_pass(self, g: RoiBuffers, views, shapes, sel, slot: int, post: dict, image_hw, mask_threshold: float, dedup: bool,
                       lds_reserve: int, tag=None):
        """Detection masks, post-processing and paste back to back (the in-order single-scene frame runs the proposal masks between
        the two halves, so they stay callable on their own)."""
        self.detection_masks(g, views, shapes, sel, slot, dedup, lds_reserve, tag)
        self.postprocess_and_paste(g, sel, post, image_hw, mask_threshold, dedup)

