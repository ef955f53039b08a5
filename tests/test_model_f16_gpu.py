"""The whole frame in the f16 convolution arithmetic: the schedules and the lock-step batch stay bitwise properties of the model, the
training step refuses the mode, leaving the mode leaves nothing behind -- and the accuracy record: detections of the f16 mode
against the fp32 mode of the same build on the same frames (printed in full with `pytest -s`)."""
import pytest
import torch

from test_fullsize_gpu import _batch_equals_singles, _cfg

pytestmark = pytest.mark.gpu


@pytest.fixture
def f16():
    from embodied_object_detection_amd import ops
    prev = ops.set_conv_math("f16")
    yield
    ops.set_conv_math(prev)


def _frames(H, W, n, grid, cell, seed=0):
    from embodied_object_detection_amd.data.synthetic import SyntheticSequence
    seq = SyntheticSequence(seed, H=H, W=W, n_frames=n, map_w=grid, map_h=grid, cell=cell)
    return [seq.frame(i) for i in range(n)]


def _run(model, frames):
    """One call per frame (the memory persists across calls) -> per frame (boxes, scores, classes, masks), then the memory state."""
    outs = []
    for f in frames:
        inst = model([[f]])[0]["instances"]
        outs.append((inst.pred_boxes.tensor.cpu().clone(), inst.scores.cpu().clone(), inst.pred_classes.cpu().clone(),
                     inst.pred_masks.cpu().clone()))
    return outs, model.implicit_memory.cpu().clone(), model.observations.cpu().clone()


def _same(a, b) -> bool:
    (ra, ma, oa), (rb, mb, ob) = a, b
    return (torch.equal(ma, mb) and torch.equal(oa, ob) and len(ra) == len(rb) and
            all(all(torch.equal(x, y) for x, y in zip(fa, fb)) for fa, fb in zip(ra, rb)))


def test_schedules_are_bitwise_equal_in_f16_mode(synthetic_sd, f16):
    """In order on one stream and pipelined over three: detections, masks and the memory state are bitwise equal, frame after frame."""
    from embodied_object_detection_amd import build_model, ops
    assert ops.get_conv_math() == "f16"
    frames = _frames(128, 160, 4, 24, 0.5)
    got = []
    for overlap in (False, True):
        model = build_model(_cfg(), synthetic_sd)
        model.overlap_branches = overlap
        got.append(_run(model, frames))
    assert _same(got[0], got[1])
    assert sum(len(f[1]) for f in got[0][0]) > 0, "no detections at all: nothing was compared"


@pytest.mark.parametrize("kind", ["launches", "streams"])
def test_lockstep_batch_is_bitwise_its_single_runs_in_f16_mode(synthetic_sd, f16, kind):
    _batch_equals_singles(synthetic_sd, 128, 160, 24, 0.5, 3, 3, kind)


def test_switching_back_to_fp32_reproduces_the_fp32_outputs(synthetic_sd):
    """fp32, then f16, then fp32 again on ONE model: the third run is bitwise the first (no half weights leak into the fp32 kernels),
    the second is not (the mode really changes the arithmetic) and the half copies exist after it."""
    from embodied_object_detection_amd import build_model, ops
    assert ops.get_conv_math() == "fp32"
    frames = _frames(128, 160, 3, 24, 0.5, seed=3)
    model = build_model(_cfg(), synthetic_sd)
    first = _run(model, frames)
    convs = [c for c in model.roi_heads.mask_convs]
    assert all(c.w_half is None for c in convs)
    prev = ops.set_conv_math("f16")
    try:
        second = _run(model, frames)
    finally:
        ops.set_conv_math(prev)
    assert all(c.w_half is not None and c.w_half.numel() == 2 * c.Cout * c.Kpad for c in convs)
    third = _run(model, frames)
    assert _same(first, third)
    assert not _same(first, second)


def test_trainer_refuses_the_mode_on_a_real_model(synthetic_sd):
    from embodied_object_detection_amd import build_model, ops
    from embodied_object_detection_amd.modeling.training import Trainer
    model = build_model(_cfg(FP16=False), synthetic_sd)
    prev = ops.set_conv_math("f16")
    try:
        with pytest.raises(ValueError, match="inference only"):
            Trainer(model, synthetic_sd)
    finally:
        ops.set_conv_math(prev)
    trainer = Trainer(model, synthetic_sd)          # fine in fp32 ...
    prev = ops.set_conv_math("f16")
    try:
        with pytest.raises(ValueError, match="inference only"):   # ... and a step taken after a later switch is refused too
            trainer.optimizer_step()
    finally:
        ops.set_conv_math(prev)


# ------------------------------------------------------------------------------------------------
# the accuracy record
# ------------------------------------------------------------------------------------------------
def _iou(a, b):
    lt = torch.max(a[:, None, :2], b[None, :, :2])
    rb = torch.min(a[:, None, 2:], b[None, :, 2:])
    inter = (rb - lt).clamp(min=0).prod(dim=2)
    area = lambda x: (x[:, 2] - x[:, 0]) * (x[:, 3] - x[:, 1])
    return inter / (area(a)[:, None] + area(b)[None, :] - inter).clamp(min=1e-12)


def _match(ref, got):
    """One-to-one, greedy by IoU, same class, IoU >= 0.9 -> (fraction of the reference matched, box and score differences)."""
    (rb, rs, rc, _), (gb, gs, gc, _) = ref, got
    if len(rb) == 0 or len(gb) == 0:
        return (1.0 if len(rb) == 0 else 0.0), torch.zeros(0), torch.zeros(0)
    iou = _iou(rb.double(), gb.double())
    iou[rc[:, None] != gc[None, :]] = -1.0
    dbox, dscore, used_r, used_g = [], [], set(), set()
    for flat in iou.flatten().argsort(descending=True).tolist():
        i, j = divmod(flat, iou.shape[1])
        if iou[i, j] < 0.9:
            break
        if i in used_r or j in used_g:
            continue
        used_r.add(i)
        used_g.add(j)
        dbox.append(float((rb[i] - gb[j]).abs().max()))
        dscore.append(abs(float(rs[i] - gs[j])))
    return len(used_r) / len(rb), torch.tensor(dbox), torch.tensor(dscore)


def _q(v):
    if len(v) == 0:
        return "-"
    return " / ".join(f"{float(torch.quantile(v.double(), q)):.2e}" for q in (0.5, 0.9, 0.99, 1.0))


@pytest.mark.parametrize("size", ["128x160", "640x640"])
def test_f16_detections_against_the_fp32_mode(synthetic_sd, size):
    """Four frames of one sequence in fp32 and in f16 mode (each from an empty memory, so frame 0 reads identical memory; later frames
    also carry the difference of the memories written).  Floors on frame 0: >= 90 % of the fp32 detections matched one-to-one (same
    class, IoU >= 0.9), median box difference <= 0.5 px, median score difference <= 5e-3; every frame's outputs finite; the full
    distribution is printed (median / 90 % / 99 % / max)."""
    from embodied_object_detection_amd import build_model, ops
    H, W, grid, cell = (128, 160, 24, 0.5) if size == "128x160" else (640, 640, 200, 0.2)
    frames = _frames(H, W, 4, grid, cell, seed=11)
    assert ops.get_conv_math() == "fp32"
    model = build_model(_cfg(), synthetic_sd)
    ref, ref_mem, _ = _run(model, frames)
    prev = ops.set_conv_math("f16")
    try:
        got, got_mem, _ = _run(model, frames)
    finally:
        ops.set_conv_math(prev)
    rows = []
    for t, (r, g) in enumerate(zip(ref, got)):
        assert all(bool(torch.isfinite(x.float()).all()) for x in g[:2]), t
        frac, dbox, dscore = _match(r, g)
        rows.append((frac, dbox, dscore))
        print(f"[f16 vs fp32 {size} frame {t}] fp32 {len(r[1])} detections, f16 {len(g[1])}; matched {frac * 100:.1f} %; box difference px "
              f"(median / 90 % / 99 % / max) {_q(dbox)}; score difference {_q(dscore)}", flush=True)
    assert bool(torch.isfinite(got_mem).all())
    dm = (got_mem - ref_mem).abs()
    print(f"[f16 vs fp32 {size}] memory after 4 frames: max |difference| {float(dm.max()):.3e}, mean {float(dm.mean()):.3e} of mean "
          f"|memory| {float(ref_mem.abs().mean()):.3e}", flush=True)
    frac, dbox, dscore = rows[0]
    assert len(ref[0][1]) > 0
    assert frac >= 0.90, f"frame 0: {frac * 100:.1f} % of the fp32 detections matched"
    assert float(dbox.median()) <= 0.5 and float(dscore.median()) <= 5e-3, (float(dbox.median()), float(dscore.median()))
