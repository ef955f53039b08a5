"""The non-convolution launches the full-size INFERENCE frames really run: recorded, then replayed alone against references that do
not share the kernels' arithmetic.

test_training_launches_gpu.py holds the non-convolution launches of the training step; this module does the same for the frame
`model([episode])` runs.  A short episode (an empty-memory frame, then two recurrent ones) of every production configuration of
`_inference_cases.CONFIGS` -- 640x640 (the benchmark's headline), 480x640, 640x640 in lock-step of 2 and 4 scenes, 960x960 over a
512x512 grid alone and in lock-step of 4, MAP_FEAT_FUSION mem_only, 1203 LVIS classes -- runs with the entry points wrapped
(`_launch_cases.Recorder(inference=True)`); every call distinct in its arguments is kept, the selection calls with host copies of
the first real lists.  `pytest -s` prints one line per recorded case and one line per comparison.

Replayed here, at the recorded shapes, capacities, flags and `batch`, outputs pre-filled with a sentinel, every launch twice
(bitwise repetition):

  EXACT (decisions on fp32 values; the reference takes the same decisions on the same values, comparison by torch.equal)
  * proposals (`ProposalDecoder`): the 14 hostile heat maps of `_inference_cases.HEAT_CASES` on every recorded pyramid, scenes of a
    lock-step launch carrying different cases, plus one pyramid whose packed slots exceed 4096 (`cn_merge_nms_kernel<8>`; no
    production frame reaches it).  Candidate count, kept count and order exact, scores exact where the heat's bits are known;
    boxes within the decode's roundings.
  * `DetectionSelector` with `unique` / `groups` as recorded, ragged counts over the scenes (0 and R_cap among them) against
    oracle.ops.fast_rcnn_inference_single, torch.unique and a Python restatement of the grouping.
  * `paste_masks`: EVERY pixel of every instance whose float64 probability is further from the threshold than the derived band
    (`_inference_cases.paste_band`) must agree; pixels inside the band are counted, printed and bounded.
  * `memory_gather_pool(torch_order=True)` bit-identical to F.avg_pool2d's order at the recorded sizes and cell counts, five index
    patterns; `memory_normalize_f16` / `_dirty_f16` bit-exact at the recorded cell counts with 0, 1 and all rows dirty.
  * `maxpool3x3s2`, `concat_lists` exact; `unique_rows` bitwise the selector's fused list at R_cap.

  FLOAT64 WITH A DERIVED BOUND
  * `MemoryProjector` at every recorded (H, W, mode, batch): a sentinel-filled row list, every row of the three levels written
    (which is what proves the kernel's workgroup remap is a permutation of the grid), the rows behind P5 untouched.
  * `preprocess_image` at the recorded sizes, in the allocating form and into `out` as recorded.

NOT replayed here (recorded and printed only), but held against float64 with derived bounds (`detector_postprocess`: exactly) at
their own tile and loop edges rather than at the recorded shapes, in test_head_launches_gpu.py: `zs_classify` narrow and wide with
its fused `zs_mem` re-score and `final_inv_stages` fusion (test_narrow_classifier, test_wide_classifier), `cascade_stage_tail`
(test_cascade_stage_tail), `apply_deltas` (test_apply_deltas), `cascade_scores` (test_cascade_scores), `memory_scores`
(test_narrow_memory_scores, test_wide_memory_scores), `mask_predictor_sigmoid` (test_mask_predictor), `detector_postprocess`
(test_detector_postprocess).

NOT replayed here either (recorded and printed only), each held alone in a module of its own, against float64 with derived bounds or
bit for bit, at the sizes where its loops and tiles end rather than at the recorded shapes:
  * `roi_align` with `box_rows` / `refine` / `batch`: test_roi_forms_gpu.py (float64 `RoiRef`; the grid-stride loop's second trip
    at S = 14, both channel trips, NaN / inf / clamped deltas, per-image counts, global index lists over a batch).
  * `MemoryWriter`: test_memory_write_edges_gpu.py (a float64 restatement of the write on scenes without a threshold band: up to
    128 unique instances, the LDS table's overflow, partial and empty blocks, batches, the 4-wave commit); _write_parity.py holds it
    at full size on the frame's own masks.
  * `unproject_grid_index`: test_kernels_gpu.py::test_unproject_grid_index_sizes_and_hostile_depth (bitwise oracle/projector.c past
    the launch's 1 048 576-pixel cap, with non-finite and negative depth) beside test_unproject_grid_index_bit_exact.
  * `semmap_labels`: test_semmap_query_gpu.py (float64, derived bounds).
  * `groupnorm_relu` with `partial_ready=True` (the inference form): at 640 x 640 by the fused-statistics way of
    test_training_launches_gpu.py::test_groupnorm_forward_and_backward_at_the_recorded_pyramids.
Lock-step is recorded in its `launches` kind (modeling/lockstep.py); the `streams` kind (modeling/batched.py) is recorded once and
asserted to make no call the single-scene episode has not made.
"""
import os
import sys
from typing import Dict, Tuple

import numpy as np
import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if __name__ == "__main__":
    sys.path[:0] = [ROOT, os.path.dirname(os.path.abspath(__file__))]

import _inference_cases as IC                                                          # noqa: E402
from _launch_cases import SENTINEL, U, Recorder, fragments_to_rows                     # noqa: E402

gpu = pytest.mark.gpu          # every test below that launches anything carries it; the references' CPU self-checks do not

LVIS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lvis_v1_clip.npy")
BASE = ["MODEL.MEMORY_TYPE", "implicit_memory", "MODEL.MAP_FEAT_FUSION", "sum", "MODEL.MAP_FEATURE_WEIGHT", 5]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    from embodied_object_detection_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def recorded(dev, synthetic_sd) -> Dict[str, Dict[str, Dict[tuple, dict]]]:
    """configuration -> family -> {arguments: payload} of a three-frame episode.  One model per configuration, freed before the next."""
    from embodied_object_detection_amd import build_model, setup_cfg
    from embodied_object_detection_amd.data.synthetic import SyntheticSequence, hip_projector
    from embodied_object_detection_amd.modeling import load_classifier
    from embodied_object_detection_amd.modeling.lockstep import LockstepScenes
    out = {}
    for name, (H, W, grid, cell, B, extra, lvis) in IC.CONFIGS.items():
        sd, opts = synthetic_sd, BASE + extra
        if lvis:
            sd = dict(sd)
            zs = load_classifier(LVIS, 1203)
            for k in range(3):
                sd[f"roi_heads.box_predictor.{k}.cls_score.zs_weight"] = zs.clone()
            opts = opts + ["MODEL.TEST_CLASSIFIERS", f"('{LVIS}',)", "MODEL.TEST_NUM_CLASSES", "[1203]"]
        cfg = setup_cfg(None, opts)
        model = build_model(cfg, sd) if B == 1 else LockstepScenes(cfg, B, sd)
        with Recorder(inference=True) as rec:
            seqs = [SyntheticSequence(60 + b, H=H, W=W, n_frames=3, map_w=grid, map_h=grid, cell=cell, projector=hip_projector()) for b in range(B)]
            eps = [[s.frame(i) for i in range(3)] for s in seqs]
            model([eps[0]] if B == 1 else eps)
            if name == "640x640":
                model.semantic_map()
            torch.cuda.synchronize()
        out[name] = rec.calls
        del model
        torch.cuda.empty_cache()
    return out


def _union(recorded, family: str) -> Dict[tuple, Tuple[str, dict]]:
    """Every distinct call of a family over all configurations, under the first configuration that made it."""
    out: Dict[tuple, Tuple[str, dict]] = {}
    for config, fams in recorded.items():
        for key, payload in fams.get(family, {}).items():
            out.setdefault(key, (config, payload))
    return out


def _twice(run):
    """Run a launch twice into fresh sentinel-filled outputs: -> the first result, after asserting the second has the same bits."""
    a, b = run(), run()
    torch.cuda.synchronize()
    for x, y in zip(a, b):
        assert torch.equal(x.view(torch.uint8) if x.is_floating_point() else x, y.view(torch.uint8) if y.is_floating_point() else y), "a second launch gave other bits"
    return a


def _sent(shape, dtype, dev):
    if dtype == torch.float32:
        return torch.full(shape, SENTINEL, dtype=dtype, device=dev)
    return torch.full(shape, {torch.int32: -77777, torch.uint8: 0xA5, torch.float16: 12345.0}[dtype], dtype=dtype, device=dev)


# ------------------------------------------------------------------------------------------------
# 1. what the frames launch
# ------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("config", list(IC.CONFIGS))
def test_recording_holds_every_family(recorded, config):
    H, W, grid, cell, B, extra, lvis = IC.CONFIGS[config]
    fams = recorded[config]
    print()
    for family in IC.ALL_FAMILIES:
        for key, payload in fams.get(family, {}).items():
            kept = "".join(f"  {k} kept: {len(payload[k])}" for k in ("lists",) if payload.get(k))
            print(f"{config:30s} {family:26s} x{payload['n']:<3d} {' '.join(str(k) for k in key)}{kept}")
    for family in IC.FRAME_FAMILIES:
        assert fams.get(family), f"{config}: no recorded call of family '{family}'"
    assert any(fams.get(f) for f in IC.CLASSIFIER_FAMILIES), f"{config}: the box head's classifier was not recorded"
    if B > 1:
        for family in IC.LOCKSTEP_FAMILIES:
            assert fams.get(family), f"{config}: no recorded call of family '{family}'"
    assert fams.get("memory_normalize_f16") or fams.get("memory_normalize_dirty_f16") or any(k[-1] for k in fams["memory_writer"]), \
        f"{config}: nothing keeps the fp16 table current"
    n_cells = grid * grid
    hw = IC.pyramid_hw(H, W)
    assert {k[:2] for k in fams["preprocess_image"]} == {(H, W)} and {k[1:] for k in fams["maxpool3x3s2"]} == {(H // 2, W // 2, 64)}
    (kp, pp), = fams["proposals"].items()
    assert kp[0] == tuple(h * w for h, w in hw) and kp[1] == tuple(w for _, w in hw) and kp[5] == B and pp["strides"] == IC.STRIDES
    assert {k[:2] for k in fams["memory_gather_pool"]} == {(H, W)} and {k[2] for k in fams["memory_gather_pool"]} == {n_cells}
    assert set(fams["memory_projector"]) == {(H, W, 5.0, "mem_only" if extra else "sum", B)}
    assert {k[:3] + (k[5],) for k in fams["memory_writer"]} == {(H, W, n_cells, B)}
    assert {k[:3] for k in fams["paste_masks"]} == {(300, H, W)} and {k[4] for k in fams["paste_masks"]} == {B}
    sel = fams["detection_selector"]
    assert {k[1] for k in sel} == ({1204, 21} if lvis else {21}) and {k[3] for k in sel} == {B}
    assert any(k[4] for k in sel) and any(k[5] for k in sel), "the memory's selection (unique) and the detections' (groups)"
    assert {k[:2] for k in fams["unproject_grid_index"]} == {(H, W)} and {k[2:4] for k in fams["unproject_grid_index"]} == {(grid, grid)}
    roi = fams["roi_align"]
    assert {k[4] for k in roi} == {7, 14} and any(k[6] for k in roi), "the box head's 7x7 and the mask head's 14x14 over box_rows"
    assert all(k[7] == B for k in roi)
    if config == "640x640":
        assert fams.get("semmap_labels")


@gpu
def test_streams_kind_of_lock_step_makes_no_call_of_its_own(dev, recorded, synthetic_sd):
    """modeling/batched.py (B scene objects on B streams, only the trunk batched): every call it makes, arguments included, is one
    the single-scene 640x640 episode has made -- so the replays of that recording hold it."""
    from embodied_object_detection_amd import setup_cfg
    from embodied_object_detection_amd.data.synthetic import SyntheticSequence, hip_projector
    from embodied_object_detection_amd.modeling.batched import BatchedSequences
    model = BatchedSequences(setup_cfg(None, BASE), 2, synthetic_sd)
    with Recorder(inference=True) as rec:
        seqs = [SyntheticSequence(60 + b, H=640, W=640, n_frames=3, projector=hip_projector()) for b in range(2)]
        model([[s.frame(i) for i in range(3)] for s in seqs])
        torch.cuda.synchronize()
    del model
    torch.cuda.empty_cache()
    single = recorded["640x640"]
    assert set(IC.FRAME_FAMILIES) <= set(rec.calls)
    for family, calls in rec.calls.items():
        extra = set(calls) - set(single.get(family, {}))
        print(f"streams 2 {family:26s} {len(calls)} distinct calls, {len(extra)} not in the single-scene recording")
        assert not extra, f"the streams kind calls '{family}' with arguments no single-scene frame uses: {sorted(extra, key=str)}"


# ------------------------------------------------------------------------------------------------
# 2. proposals
# ------------------------------------------------------------------------------------------------
def _proposal_cases(recorded):
    cases = dict(_union(recorded, "proposals"))
    # a pyramid no frame has: packed slots 5 x 1000 > 4096, the wide merge; the payload of the headline's decoder otherwise
    config, pay = cases[next(iter(cases))]
    key0 = next(iter(cases))
    hw = [(80, 80), (72, 72), (64, 64), (48, 48), (40, 40)]
    cases[(tuple(h * w for h, w in hw), tuple(w for _, w in hw)) + key0[2:5] + (1, key0[6])] = ("packed slots > 4096", pay)
    return cases


@gpu
def test_proposals_on_hostile_heat_maps(dev, recorded):
    from embodied_object_detection_amd import ops
    print()
    bad = []
    for key, (config, pay) in _proposal_cases(recorded).items():
        sizes, widths, pre, post, cap, B, hs = key
        hw = [(n // w, w) for n, w in zip(sizes, widths)]
        dec = ops.ProposalDecoder(hw, pay["strides"], pay["scales"], pay["score_thresh"], pre, post, pay["nms_thresh"], cap, dev, head_stride=hs, batch=B)
        n_cases = len(IC.HEAT_CASES)
        # a lock-step launch carries B cases at once; two launches of it (the single-scene launches have run all fourteen)
        for first in list(range(0, n_cases, B))[:n_cases if B == 1 else 2]:
            names = [IC.HEAT_CASES[(first + b) % n_cases] for b in range(B)]
            logits, heats, regs = [], [], []
            for b, case in enumerate(names):
                lg, ht, regime = IC.hostile_heat(case, sizes, pre, post, seed=100 + first + b)
                logits.append(lg)
                heats.append(ht if ht is not None else [torch.sigmoid(v) for v in lg])
                regs.append(IC.hostile_reg(regime, hw, seed=300 + first + b))
            head = IC.head_rows(logits, regs, hs).to(dev)

            def run():
                dec.boxes.fill_(SENTINEL), dec.scores.fill_(SENTINEL), dec.count.fill_(-77777)
                dec(head)
                return dec.boxes.clone(), dec.scores.clone(), dec.count.clone()
            gb, gs, gc = (t.cpu() for t in _twice(run))
            for b, case in enumerate(names):
                tag = f"{config} / {case}" + (f" / scene {b} of {B}" if B > 1 else "")
                rb, rs, n_cand, n_nms = IC.proposals_reference(heats[b], regs[b], hw, pay["strides"], pay["scales"], pay["score_thresh"], pre, post,
                                                              pay["nms_thresh"])
                n = min(rb.shape[0], cap)
                got_n = int(gc[b])
                ob, os_ = gb[b * cap:(b + 1) * cap], gs[b * cap:(b + 1) * cap]
                line = f"{tag:64s} candidates {n_cand:5d} after NMS {n_nms:5d} kept {rb.shape[0]:5d} (cap {cap}): HIP {got_n}"
                if got_n != n:
                    bad.append(line)
                    print(line + "  <-- COUNT")
                    continue
                # scores: sqrtf of the fp32 sigmoid; exact where the test knows the sigmoid's bits, else within 2 ulp of the CPU's
                s_err = float(((os_[:n].double() - rs[:n].double()).abs() / rs[:n].double()).max()) if n else 0.0
                # boxes: grid -/+ relu(scale * reg) * stride: two roundings of the offset and one of the sum, at their magnitudes
                # order: exact, row for row (a wrong candidate is at least one grid position away).  Scores: the root of the heat is
                # correctly rounded on both sides (`IC.sqrt_rn`; the kernel's sqrtf compiles to the corrected sequence), so where the
                # test knows the heat's bits (the 'cut edge' maps) they are equal; elsewhere the heat is the CPU's sigmoid, which may
                # differ from the device's by an ulp or two of its expf: 4 U relative
                s_bound = 0.0 if case.startswith("cut edge") else 4 * U
                b_bound = 4 * U * (rb[:n].abs().max(dim=1, keepdim=True).values + 1.0) * 2.0
                b_err = (ob[:n].double() - rb[:n].double()).abs()
                order_ok = bool((b_err <= 0.25).all())
                line += f"  score err {s_err:.2e} (bound {s_bound:.2e})  box err {float(b_err.max()) if n else 0.0:.2e} (bound {float(b_bound.max()) if n else 0.0:.2e})"
                print(line)
                if not order_ok:
                    bad.append(f"{tag}: {int((b_err > 0.25).any(dim=1).sum())} of {n} rows are other candidates than the reference's "
                               f"(first at {int((b_err > 0.25).any(dim=1).nonzero()[0])})")
                elif n and (s_err > s_bound or not bool((b_err <= b_bound).all())):
                    bad.append(f"{tag}: scores {s_err:.3e} / boxes {float(b_err.max()):.3e} off the reference")
                if n and not bool((os_[:n - 1] >= os_[1:n]).all()):
                    bad.append(f"{tag}: scores are not descending")
                if not (bool((ob[n:] == SENTINEL).all()) and bool((os_[n:] == SENTINEL).all())):
                    bad.append(f"{tag}: rows behind the count were written")
    assert not bad, "\n".join(bad)


# ------------------------------------------------------------------------------------------------
# 3. detection selection
# ------------------------------------------------------------------------------------------------
@gpu
def test_detection_selection_with_unique_and_groups(dev, recorded):
    from embodied_object_detection_amd import ops
    from oracle import ops as OO
    print()
    bad = []
    for key, (config, pay) in _union(recorded, "detection_selector").items():
        R, C1, topk, B, unique, groups, img_w, img_h, st, nt, has_count = key
        if C1 > 32:
            print(f"{config}: {R} rows x {C1 - 1} classes: the wide selection at this shape is test_vocab_kernels_gpu.py's")
            continue
        sel = ops.DetectionSelector(R, C1, topk, dev, unique=unique, groups=groups, batch=B)
        for ci, case in enumerate(IC.DET_CASES):
            # ragged over the scenes of a batch (0, 1, R_cap among them); a single scene gets the whole list
            counts = [[R, 0, 1, R - 37][(ci + b) % 4] for b in range(B)] if has_count and B > 1 else [R - (37 if ci == 3 and has_count else 0)] * B
            boxes = torch.zeros((B * R, 4))
            scores = torch.zeros((B * R, C1))
            for b in range(B):
                bb, ss = IC.hostile_detections(case, R, C1, img_w, img_h, seed=500 + 10 * ci + b)
                boxes[b * R:(b + 1) * R], scores[b * R:(b + 1) * R] = bb, ss
            cnt = torch.tensor(counts, dtype=torch.int32, device=dev) if has_count else None
            bd, sd = boxes.to(dev), scores.to(dev)
            outs = [sel.boxes, sel.scores, sel.classes, sel.rows, sel.count] + ([sel.uniq_rows, sel.uniq_count] if unique else []) \
                + ([sel.rep_of, sel.rep_list, sel.rep_count] if groups else [])

            def run():
                for t in outs:
                    t.fill_(SENTINEL if t.dtype == torch.float32 else -77777)
                sel(bd, sd, cnt, img_w, img_h, st, nt)
                return [t.clone() for t in outs]
            got = [t.cpu() for t in _twice(run)]
            for b in range(B):
                tag = f"{config} {img_w:.0f}x{img_h:.0f} R {R} topk {topk} batch {B} / {case} / scene {b} count {counts[b]}"
                n_in = counts[b]
                rb, rs, rc, rr = OO.fast_rcnn_inference_single(boxes[b * R:b * R + n_in], scores[b * R:b * R + n_in], (int(img_h), int(img_w)), st, nt, topk)
                n = rb.shape[0]
                gb, gs, gcl, gr = (got[i][b * topk:(b + 1) * topk] for i in range(4))
                print(f"{tag:100s} kept {n:4d}: HIP {int(got[4][b])}")
                if int(got[4][b]) != n:
                    bad.append(f"{tag}: {int(got[4][b])} detections, reference {n}")
                    continue
                ok = torch.equal(gb[:n], rb) and torch.equal(gs[:n], rs) and torch.equal(gcl[:n].long(), rc.long()) and torch.equal(gr[:n].long(), rr.long())
                if not ok:
                    bad.append(f"{tag}: boxes / scores / classes / rows differ from the reference")
                if not (bool((gb[n:] == SENTINEL).all()) and bool((gs[n:] == SENTINEL).all()) and bool((gr[n:] == -77777).all())):
                    bad.append(f"{tag}: slots behind the count were written")
                i = 5
                if unique:
                    u = torch.unique(rr.long())
                    gu = got[i][b * R:(b + 1) * R]
                    if int(got[i + 1][b]) != u.numel() or not torch.equal(gu[:u.numel()].long(), u) or not bool((gu[u.numel():] == -77777).all()):
                        bad.append(f"{tag}: the unique row list differs from torch.unique ({int(got[i + 1][b])} against {u.numel()})")
                    i += 2
                if groups:
                    rep_of, rep_list = IC.group_rows(rr.tolist())
                    g_of, g_list = got[i][b * topk:(b + 1) * topk], got[i + 1][b * topk:(b + 1) * topk]
                    if int(got[i + 2][b]) != len(rep_list) or g_of[:n].tolist() != rep_of or g_list[:len(rep_list)].tolist() != rep_list:
                        bad.append(f"{tag}: the detection-mask groups differ from the restatement")
    assert not bad, "\n".join(bad)


@gpu
def test_unique_rows_is_bitwise_the_selectors_fused_list(dev, recorded):
    from embodied_object_detection_amd import ops
    for key, (config, pay) in _union(recorded, "detection_selector").items():
        R, C1, topk, B, unique = key[:5]
        if not unique or C1 > 32 or B > 1:
            continue
        boxes, scores = IC.hostile_detections("equal scores", R, C1, key[6], key[7], seed=77)
        sel = ops.DetectionSelector(R, C1, topk, dev, unique=True)
        cnt = torch.tensor([R], dtype=torch.int32, device=dev)
        _, _, _, rows, n = sel(boxes.to(dev), scores.to(dev), cnt, key[6], key[7], key[8], key[9])
        out_rows, out_count = _sent((R,), torch.int32, dev), _sent((1,), torch.int32, dev)
        ops.unique_rows(rows, n, topk, R, out_rows, out_count)
        k = int(sel.uniq_count.item())
        assert int(out_count.item()) == k and 0 < k <= R and torch.equal(out_rows[:k], sel.uniq_rows[:k]), config
        assert bool((out_rows[k:] == -77777).all())


# ------------------------------------------------------------------------------------------------
# 4. paste
# ------------------------------------------------------------------------------------------------
def _paste_check(tag, dev, K_cap, H, W, thr, B, units, masks, boxes, rows, counts) -> list:
    """masks [B * units, 28, 28], boxes [B * K_cap, 4], rows [B * K_cap] scene-local or None, counts [B] or None."""
    from embodied_object_detection_amd import ops
    bad = []
    for b in range(B):                                   # every index the launch will follow stays inside the scene's masks
        live = K_cap if counts is None else counts[b]
        assert 0 <= live <= K_cap and masks.shape[0] == B * units and boxes.shape[0] >= B * K_cap
        assert rows is None or bool(((rows[b * K_cap:b * K_cap + live] >= 0) & (rows[b * K_cap:b * K_cap + live] < units)).all())
        assert rows is not None or live <= units
    md, bd = masks.to(dev), boxes[:B * K_cap].contiguous().to(dev)
    rd = None if rows is None else rows.int().to(dev)
    cd = None if counts is None else torch.tensor(counts, dtype=torch.int32, device=dev)

    def run():
        out = _sent((B, K_cap, H, W), torch.uint8, dev)
        ops.paste_masks(md, bd, rd, cd, K_cap, H, W, thr, out, batch=B, prob_units=units if B > 1 else 0)
        return (out,)
    out = _twice(run)[0].cpu()
    decided = in_band = wrong = 0
    widest = 0.0
    for b in range(B):
        live = K_cap if counts is None else counts[b]
        for k in range(live):
            src = b * units + (k if rows is None else int(rows[b * K_cap + k]))
            p = IC.paste_prob(masks[src], boxes[b * K_cap + k], H, W)
            band = IC.paste_band(masks[src])
            widest = max(widest, band)
            sure = (p - thr).abs() > band
            miss = sure & ((p >= thr) != (out[b, k] != 0))
            decided += int(sure.sum())
            in_band += int((~sure).sum())
            if bool(miss.any()):
                wrong += int(miss.sum())
                y, x = (int(v) for v in miss.nonzero()[0])
                bad.append(f"{tag}: scene {b} instance {k} box {[round(float(v), 3) for v in boxes[b * K_cap + k]]}: {int(miss.sum())} pixels decided wrongly, "
                           f"first at (y {y}, x {x}) where the float64 probability is {float(p[y, x]):.6f}")
            if not bool(((out[b, k] == 0) | (out[b, k] == 1)).all()):
                bad.append(f"{tag}: scene {b} instance {k}: bytes other than 0 / 1")
        if not bool((out[b, live:] == 0xA5).all()):
            bad.append(f"{tag}: scene {b}: masks behind the count {live} were written")
    print(f"{tag:70s} pixels decided {decided:11d} wrong {wrong}  inside the band (width {widest:.2e}) {in_band}  ({in_band / max(1, decided + in_band):.2e} of all)")
    # seeded noise masks have |dp| of order 1 per mask pixel: a band of 5e-5 holds ~1e-4 of the pixels of a box at most
    if in_band > 2e-3 * (decided + in_band) + 64:
        bad.append(f"{tag}: {in_band} pixels inside the band: the band does not decide what it should")
    return bad[:12]


@gpu
def test_paste_every_pixel_outside_the_band(dev, recorded):
    print()
    bad = []
    for key, (config, pay) in _union(recorded, "paste_masks").items():
        K_cap, H, W, thr, B, units, has_rows, has_count = key
        units = units if B > 1 else K_cap
        masks = IC.hostile_masks(B * units, seed=9)
        g = torch.Generator().manual_seed(10)
        tag = f"{config} K_cap {K_cap} {H}x{W} batch {B}"
        # the hostile geometry, rows shuffled, ragged counts (0, 1, all, some)
        boxes = torch.cat([IC.hostile_paste_boxes(H, W, K_cap, seed=20 + b) for b in range(B)])
        rows = torch.cat([torch.randperm(units, generator=g)[:K_cap] for _ in range(B)]) if has_rows else None
        counts = ([64, 0, 1, K_cap][:B] if B > 1 else [72]) if has_count else None
        bad += _paste_check(tag + " hostile boxes", dev, K_cap, H, W, thr, B, units, masks, boxes, rows, counts)
        # the frame's own boxes of the recorded lists
        for i, lst in enumerate(pay["lists"][:1]):
            cnt = [min(int(c), 48) for c in lst["count"]] if has_count else None
            if cnt is not None and sum(cnt):              # (without a count the rows behind the frame's own count are not indices)
                bad += _paste_check(tag + f" recorded list {i}", dev, K_cap, H, W, thr, B, units, masks, lst["boxes"], lst["rows"], cnt)
    # K = K_cap on the headline shape, rows absent, no count
    H, W = 640, 640
    bad += _paste_check("640x640 K = K_cap = 300, no rows, no count", dev, 300, H, W, 0.5, 1, 300, IC.hostile_masks(300, 3),
                        IC.hostile_paste_boxes(H, W, 300, seed=4), None, None)
    assert not bad, "\n".join(bad)


def test_reference_square_root_is_correctly_rounded():
    """`IC.sqrt_rn` against numpy's float32 root on every robust heat (numpy's is the IEEE instruction element by element)."""
    x, h = IC.robust_sigmoids()
    assert len(h) > 40000 and bool((np.diff(h) > 0).all())
    assert np.array_equal(IC.sqrt_rn(torch.from_numpy(h)).numpy().view(np.int32), np.sqrt(h).view(np.int32))
    assert np.array_equal(torch.sigmoid(torch.from_numpy(x)).numpy().view(np.int32), h.view(np.int32)), "the CPU's sigmoid on the robust logits"


def test_paste_reference_is_the_oracles_sampler():
    """float64 `paste_prob` against oracle.ops.paste_masks_prob (F.grid_sample in fp32) on the hostile geometry: fp32 close."""
    from oracle import ops as OO
    masks, boxes = IC.hostile_masks(8, 1), IC.hostile_paste_boxes(96, 128, 40, 2)
    ref = OO.paste_masks_prob(masks[torch.arange(40) % 8], boxes, (96, 128))
    for k in range(40):
        if bool(torch.isfinite(ref[k]).all()):
            assert float((IC.paste_prob(masks[k % 8], boxes[k], 96, 128) - ref[k].double()).abs().max()) < 1e-5, k
        else:
            assert float(IC.paste_prob(masks[k % 8], boxes[k], 96, 128).abs().max()) == 0.0          # a zero-width box samples nothing


# ------------------------------------------------------------------------------------------------
# 5. memory read
# ------------------------------------------------------------------------------------------------
@gpu
def test_memory_gather_pool_in_torch_order_is_bit_identical(dev, recorded):
    from embodied_object_detection_amd import ops
    print()
    bad = []
    shapes = sorted({(k[0], k[1], k[2], k[5]) for k in _union(recorded, "memory_gather_pool")})
    for H, W, N, B in shapes:
        g = torch.Generator().manual_seed(7)
        mem = torch.randn((N, 512), generator=g) * 30
        mem[::5] *= 1e-3                                  # wide exponent spread inside the pooling windows
        mem[::7] *= 1e-6                                  # fp16 subnormals
        m16 = torch.stack([mem.half().roll(977 * b, 0) for b in range(B)])       # B tables back to back, every scene its own
        del mem
        md = m16.to(dev)
        # the float64-free reference is an fp16 avg_pool2d on the host: three patterns at 960x960 (3 s each), all five below
        pats = IC.GATHER_PATTERNS if H * W < 500000 else ("distinct", "half", "columns")
        for pi in range(0, len(pats) if B == 1 else 1):
            names = [pats[(pi + b) % len(pats)] for b in range(B)]
            proj = torch.stack([IC.gather_patterns(nm, H, W, N, seed=11 + b) for b, nm in enumerate(names)])
            pd = proj.int().to(dev)
            err = torch.zeros((1,), dtype=torch.int32, device=dev)
            rows = ops.pooled_rows(H, W)

            def run():
                out = _sent((B * rows + 1, 512), torch.float16, dev)
                ops.memory_gather_pool(md if B > 1 else md[0], pd if B > 1 else pd[0], H, W, out=out[:B * rows], err=err, torch_order=True, batch=B)
                return (out,)
            out = _twice(run)[0].cpu()
            for b in (range(B) if H * W < 500000 else sorted({0, B - 1})):
                got = fragments_to_rows(out[b * rows:(b + 1) * rows], H, W)
                ref = IC.pooled_reference(m16[b], proj[b])
                same = [bool(torch.equal(a.view(torch.int16), r.view(torch.int16))) for a, r in zip(got, ref)]
                nd = [int((a.view(torch.int16) != r.view(torch.int16)).sum()) for a, r in zip(got, ref)]
                print(f"gather {H}x{W} over {N} cells batch {B} scene {b} / {names[b]:9s} differing halves per level {nd}")
                if not all(same):
                    bad.append(f"{H}x{W} N {N} batch {B} scene {b} / {names[b]}: {nd} halves differ from F.avg_pool2d's order")
            if int(err.item()) != 0 or not bool((out[B * rows:] == 12345.0).all()):
                bad.append(f"{H}x{W} N {N} batch {B}: error word {int(err.item())} or the guard row written")
    assert not bad, "\n".join(bad)


@gpu
def test_memory_normalize_full_and_dirty_are_bit_exact(dev, recorded):
    from embodied_object_detection_amd import ops
    from oracle import memory as OM
    cells = sorted({k[2] for k in _union(recorded, "memory_gather_pool")})
    assert cells == [40000, 262144]
    for N in cells:
        g = torch.Generator().manual_seed(N)
        mem = torch.randn((N, 512), generator=g) * 20
        mem[::9] *= 1e-6
        obs = torch.randint(0, 5, (N,), generator=g).float()
        ref = OM.create_implicit_memory(mem, obs).half()
        md, od = mem.to(dev), obs.to(dev)
        table = _sent((N + 1, 512), torch.float16, dev)
        ops.memory_normalize_f16(md, od, out=table[:N])
        assert torch.equal(table[:N].cpu().view(torch.int16), ref.view(torch.int16)) and bool((table[N:] == 12345.0).all()), N
        for n_dirty in (0, 1, N):
            stale = _sent((N + 1, 512), torch.float16, dev)
            dirty = torch.zeros((N + 1,), dtype=torch.int32, device=dev)
            dirty[N] = 5                                                             # behind the table: not a flag
            rows = torch.tensor([N - 1][:n_dirty], dtype=torch.int64) if n_dirty <= 1 else torch.arange(N)
            dirty[rows.to(dev)] = 1
            ops.memory_normalize_dirty_f16(md, od, dirty[:N], stale[:N])
            got = stale.cpu()
            assert torch.equal(got[rows].view(torch.int16), ref[rows].view(torch.int16)), (N, n_dirty)
            keep = torch.ones(N + 1, dtype=torch.bool)
            keep[rows] = False
            assert bool((got[keep] == 12345.0).all()), f"{N} cells, {n_dirty} dirty: rows that were not flagged were written"
            assert int(dirty[:N].sum().item()) == 0 and int(dirty[N].item()) == 5


# ------------------------------------------------------------------------------------------------
# 6. memory projection
# ------------------------------------------------------------------------------------------------
@gpu
def test_memory_projector_writes_every_row_once(dev, recorded):
    from embodied_object_detection_amd import ops
    print()
    bad = []
    g = torch.Generator().manual_seed(31)
    Ws = [torch.randn((256, 512), generator=g) * (1.0 / 512) ** 0.5 * 0.05 for _ in range(3)]
    for w in Ws:
        w[7, ::3] *= 1e3
        w[3] *= 1e-4
    bs = [torch.randn((256,), generator=g) * 0.01 for _ in range(3)]
    proj = ops.MemoryProjector([w.reshape(256, 512, 1, 1) for w in Ws], bs, dev)
    for (H, W, weight, mode, B), (config, pay) in _union(recorded, "memory_projector").items():
        for wgt in sorted({weight, 500.0 if mode == "mem_only" else weight}):
            hw = [(H // s, W // s) for s in (8, 16, 32)]
            n_l = [h * w for h, w in hw]
            # fp16-exact pooled operands with a wide exponent spread; an unobserved (all-zero) location in every scene and level
            pooled = [[(torch.randn((n, 512), generator=g) * 8 * torch.exp2(torch.randint(-6, 3, (n, 1), generator=g).float())).half() for n in n_l]
                      for _ in range(B)]
            for b in range(B):
                for l in range(3):
                    pooled[b][l][(5 * b + l) % n_l[l]] = 0
            frag = torch.cat([IC.rows_to_fragments(pooled[b]) for b in range(B)]).contiguous().to(dev)
            assert frag.shape[0] == B * ops.pooled_rows(H, W)
            # the row list, level major over the scenes; "sum" adds into seeded features, "mem_only" must overwrite the sentinel
            res = [[torch.randn((n, 256), generator=g) for n in n_l] for _ in range(B)]
            fill = torch.cat([res[b][l] if mode == "sum" else torch.full((n_l[l], 256), SENTINEL) for l in range(3) for b in range(B)])
            tail = torch.full((B * 64 + 7, 256), SENTINEL)                                # P6 / P7 in the model: not this launch's

            def run():
                buf = torch.cat([fill, tail]).contiguous().to(dev)
                proj(frag, buf, H, W, wgt, mode, batch=B)
                return (buf,)
            buf = _twice(run)[0].cpu()
            off = 0
            worst = (0.0, 0.0, 1.0)
            for l in range(3):
                for b in range(B):
                    got = buf[off:off + n_l[l]].double()
                    p = pooled[b][l].double()
                    dot = p @ Ws[l].double().t()
                    ref = (dot + bs[l].double()) * wgt + (res[b][l].double() if mode == "sum" else 0.0)
                    absdot = p.abs() @ Ws[l].double().abs().t() + bs[l].double().abs()
                    bound = IC.projector_bound(absdot, ref, wgt) + (2 * U * res[b][l].double().abs() if mode == "sum" else 0.0)
                    r32 = ((pooled[b][l].float() @ Ws[l].t() + bs[l]) * wgt + (res[b][l] if mode == "sum" else 0.0)).double()
                    err = (got - ref).abs()
                    i = int((err / bound).argmax())
                    if float((err / bound).reshape(-1)[i]) > worst[0] / worst[2]:
                        worst = (float(err.reshape(-1)[i]), float((r32 - ref).abs().reshape(-1)[i]), float(bound.reshape(-1)[i]))
                    if mode == "mem_only" and bool((buf[off:off + n_l[l]] == SENTINEL).any()):
                        bad.append(f"{config} {H}x{W} {mode} batch {B}: level {l} scene {b}: {int((buf[off:off + n_l[l]] == SENTINEL).any(1).sum())} rows never written")
                    if not bool((err <= bound).all()):
                        rows = (err > bound).any(1).nonzero().flatten()
                        bad.append(f"{config} {H}x{W} {mode} weight {wgt} batch {B}: level {l} scene {b}: {rows.numel()} rows off float64 (first {int(rows[0])}, "
                                   f"last {int(rows[-1])}), worst {float(err.max()):.3e} against bound {float(bound.reshape(-1)[int(err.argmax())]):.3e}")
                    off += n_l[l]
            print(f"{config:30s} projector {H}x{W} {mode:8s} weight {wgt:5.0f} batch {B}  err {worst[0]:.3e}  cpu fp32 {worst[1]:.3e}  bound {worst[2]:.3e} "
                  f"({worst[0] / worst[2]:.3f} of it)")
            if not bool((buf[off:] == SENTINEL).all()):
                bad.append(f"{config} {H}x{W} {mode} batch {B}: rows behind P5 were written")
    assert not bad, "\n".join(bad)


# ------------------------------------------------------------------------------------------------
# 7. the small exact ones
# ------------------------------------------------------------------------------------------------
@gpu
def test_maxpool_preprocess_and_concat_lists_at_recorded_shapes(dev, recorded):
    from embodied_object_detection_amd import ops
    print()
    g = torch.Generator().manual_seed(5)
    for (N, H, W, Cc), (config, _) in _union(recorded, "maxpool3x3s2").items():
        x = torch.randn((N, H, W, Cc), generator=g)
        x[:, 0, :, :], x[:, :, -1, :] = -1e30, 1e30                 # the padding is -inf, not zero: a border of very negative values
        y, OH, OW = ops.maxpool3x3s2(x.to(dev), N, H, W, Cc)
        ref = F.max_pool2d(x.permute(0, 3, 1, 2), 3, 2, 1).permute(0, 2, 3, 1)
        assert (OH, OW) == tuple(ref.shape[1:3]) and torch.equal(y.cpu(), ref), (config, N, H, W)
        print(f"{config:30s} maxpool {N}x{H}x{W}x{Cc} exact")
    for (H, W, div, has_out), (config, pay) in _union(recorded, "preprocess_image").items():
        img = torch.randint(0, 256, (3, H, W), generator=g, dtype=torch.uint8)
        Hp, Wp = -(-H // div) * div, -(-W // div) * div
        buf = _sent((2, Hp, Wp, 4), torch.float32, dev)
        # as recorded: into a slice of a batch buffer (`out`, the lock-step form) or into a tensor the call allocates
        out, hp, wp = ops.preprocess_image(img.to(dev), pay["mean"], pay["std"], div=div, out=buf[0:1] if has_out else None)
        if not has_out:
            assert tuple(out.shape) == (1, Hp, Wp, 4) and bool((buf == SENTINEL).all())
            buf[0:1] = out
        got = buf.cpu()
        mean, std = torch.tensor(pay["mean"], dtype=torch.float64), torch.tensor(pay["std"], dtype=torch.float64)
        ref = (img.permute(1, 2, 0).double() - mean) / std
        err = float((got[0, :H, :W, :3].double() - ref).abs().max())
        bound = 2 * U * float(ref.abs().max()) * 2.0                # a subtraction and a division (or a multiply by 1/std): 2 roundings, x2
        print(f"{config:30s} preprocess {H}x{W} -> {hp}x{wp} {'into out' if has_out else 'allocating'}  err {err:.3e}  bound {bound:.3e}")
        assert (hp, wp) == (Hp, Wp) and err <= bound
        assert bool((got[0, :, :, 3] == 0).all()) and bool((got[0, H:] == 0).all()) and bool((got[0, :, W:] == 0).all()), "pad channel / pad border"
        assert bool((got[1] == SENTINEL).all()), "the neighbouring scene's slice was written"
    for (cap_in, stride, B), (config, _) in _union(recorded, "concat_lists").items():
        counts = [cap_in, 0, 1, cap_in - 3][:B]
        lists = torch.stack([torch.randperm(stride, generator=g)[:cap_in] for _ in range(B)]).int()
        out, out_n = _sent((B * cap_in + 1,), torch.int32, dev), _sent((1,), torch.int32, dev)
        ops.concat_lists(lists.to(dev), torch.tensor(counts, dtype=torch.int32, device=dev), cap_in, stride, B, out[:B * cap_in], out_n)
        ref = torch.cat([lists[b, :counts[b]] + b * stride for b in range(B)])
        assert int(out_n.item()) == ref.numel() and torch.equal(out[:ref.numel()].cpu(), ref) and bool((out[ref.numel():] == -77777).all()), config
        print(f"{config:30s} concat_lists cap {cap_in} stride {stride} batch {B} counts {counts} exact")


if __name__ == "__main__":
    sys.exit(pytest.main([__file__, "-q", "-s", "-m", "gpu"] + sys.argv[1:]))
