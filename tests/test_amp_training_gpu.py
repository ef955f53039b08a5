"""FP16: True end to end (-m gpu): `AmpTrainer` against the fp32 `Trainer` on the same frame, keys and weights; the loss scale never
reaches the heads; a non-finite gradient produced by data skips the step and halves the scale; `trunk_batch` and FREEZE_BACKBONE
under AMP; the training CLI with the shipped configuration's FP16 key, fresh and resumed."""
import json
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BASE = ["MODEL.MEMORY_TYPE", "implicit_memory", "MODEL.MAP_FEAT_FUSION", "sum", "MODEL.MAP_FEATURE_WEIGHT", 5, "SOLVER.BASE_LR", 2e-5]
PROBES = ["backbone.bottom_up.base.conv1.weight", "backbone.bottom_up.base.layer1.0.conv2.weight", "backbone.bottom_up.base.layer2.1.conv1.weight",
          "backbone.bottom_up.base.layer3.2.conv3.weight", "backbone.bottom_up.base.layer4.0.downsample.0.weight",
          "backbone.fpn_lateral4.weight", "backbone.fpn_output3.weight", "backbone.map_merge_projection2.weight", "backbone.top_block.p6.weight",
          "backbone.top_block.p7.weight"]


def _frame(H, W, seed, dev, n_cells=400):
    g = torch.Generator().manual_seed(seed)
    img = torch.randint(0, 256, (3, H, W), generator=g, dtype=torch.uint8).to(dev)
    mem = ((torch.randn((n_cells, 512), generator=g) * 2).half().to(dev), torch.randint(0, n_cells, (H, W), generator=g).int().to(dev))
    s = min(H, W) / 128.0
    gt = (torch.tensor([[10.0, 12.0, 60.0, 70.0], [40.0, 30.0, 150.0, 120.0], [90.0, 8.0, 118.0, 40.0], [5.0, 80.0, 44.0, 124.0]]) * s).to(dev)
    gc = torch.tensor([1, 4, 9, 17]).int().to(dev)
    return img, mem, gt, gc


def _make(synthetic_sd, fp16, extra=()):
    from embodied_object_detection_amd import build_model, setup_cfg
    from embodied_object_detection_amd.modeling.training import build_trainer
    cfg = setup_cfg(None, BASE + ["FP16", fp16] + list(extra))
    sd0 = {k: v.clone() for k, v in synthetic_sd.items()}
    model = build_model(cfg, sd0)
    return model, build_trainer(model, sd0), sd0


def _grads(trainer, frame, dev, seed=1, scale=None, proposals=None, keys=None):
    img, mem, gt, gc = frame
    if scale is not None:
        trainer.step_fn.grad_scale = scale
    kw = dict(generator=torch.Generator(device=dev).manual_seed(seed)) if proposals is None else dict(proposals=proposals, keys=keys)
    losses, grads = trainer.fm.forward_backward(img, gt, gc, memory=mem, **kw)
    torch.cuda.synchronize()
    by_name = {g["name"]: trainer.getters[g["name"]](grads) for g in trainer.groups}
    return {k: float(v) for k, v in losses.items()}, by_name


def test_build_trainer_and_the_scale_never_reaches_the_heads(synthetic_sd):
    """The same AMP step with the scale at 1 and at 65536: every head gradient (tower, output convs, scales, ROI heads) and every loss
    is bitwise the same; the backbone's gradients are 65536 times larger -- exactly where all three products are fp32 (P7), up to the
    half subnormals the unscaled run loses elsewhere -- which the optimizer's launch divides out again."""
    from embodied_object_detection_amd import ops
    from embodied_object_detection_amd.modeling.training import AmpTrainer, Trainer
    dev = torch.device("cuda:0")
    model, trainer, _ = _make(synthetic_sd, True)
    assert type(trainer) is AmpTrainer and trainer.scaler.get_scale() == 65536.0 and ops.get_conv_math() == "fp32"
    assert trainer.step_fn.bb.math == "f16" and trainer.fm.det._bw == {}
    with pytest.raises(NotImplementedError, match="FP16"):
        Trainer(model, {})
    fr = _frame(128, 160, 11, dev)
    _grads(trainer, fr, dev, scale=1.0)                       # settles the exact path for this size
    l1, g1 = _grads(trainer, fr, dev, scale=1.0)
    l2, g2 = _grads(trainer, fr, dev, scale=65536.0)
    assert l1 == l2 and len(l1) == 10
    heads = [n for n in g1 if not n.startswith("backbone.")]
    back = [n for n in g1 if n.startswith("backbone.")]
    assert len(heads) > 40 and len(back) > 60 and [n.startswith("backbone.") for n in g1] == trainer._scaled
    for n in heads:
        assert torch.equal(g1[n], g2[n]), n
    worst = 0.0
    for n in back:
        assert bool(torch.isfinite(g2[n]).all()) and float(g1[n].abs().max()) > 0, n
        if "top_block.p7" in n:
            assert torch.equal(g1[n] * 65536.0, g2[n]), n      # fp32 in all three products: a power of two commutes with every rounding
            continue
        # f16 operands: the unscaled gradients reach into half's subnormals (below 6.1e-5, what the scaler is for), so the two differ
        # by that lost precision and by nothing else
        rel = float((g1[n].double() * 65536.0 - g2[n].double()).norm() / g2[n].double().norm())
        worst = max(worst, rel)
        assert rel < 2e-2, (n, rel)
    print(f"backbone gradients, scale 1 against 65536: worst relative L2 difference {worst:.2e} (half subnormals of the unscaled run)")
    assert all(bw.math is None for bw in trainer.fm.det._bw.values()) and all(bw.math is None for bw in trainer.step_fn._bw.values())


@pytest.mark.parametrize("size", [(128, 160), (640, 640)])
def test_amp_step_against_the_fp32_step(synthetic_sd, size):
    """Ten losses and the probe gradients of one AMP step against the fp32 step on the same frame, keys and weights.  Bound: an
    operand rounded to half carries 2^-11 of relative error, a product of two 2^-10; through a chain of d layers the errors of
    independent roundings add like sqrt(d) on average, and a ReLU that flips at a rounding error moves single elements, so the
    comparison is in the L2 norm: 2^-10 * sqrt(2 * 53) = 1.0e-2 for the deepest probe (the stem: 53 layers forward and back), taken
    with a factor 4 of head room for every probe (8 at 640x640, see below).  The measured figures are printed (profiles/r08_amp_step_and_layers.txt keeps a run)."""
    dev = torch.device("cuda:0")
    H, W = size
    fr = _frame(H, W, 21, dev)
    # both steps on the fp32 step's proposal list and the same sampling keys: a proposal that moves in or out of the list at a
    # rounding error is a different sample, not an arithmetic difference (test_forward_model_training_step_both_halves does the same)
    _, ref, _ = _make(synthetic_sd, False)
    _grads(ref, fr, dev)
    props = ref.fm.last_proposals.clone()
    keys = torch.rand((props.shape[0] + fr[2].shape[0],), generator=torch.Generator().manual_seed(5)).to(dev)
    lr_, gr = _grads(ref, fr, dev, proposals=props, keys=keys)
    del ref
    _, amp, _ = _make(synthetic_sd, True)
    la, ga = _grads(amp, fr, dev, scale=65536.0, proposals=props, keys=keys)
    del amp
    # (640x640: 8 -- P7's gradient is 25 positions behind the ReLU on P6, one flip at a rounding error weighs 1 / 25; measured 5.2e-2)
    bound = (4 if H * W < 640 * 640 else 8) * 2.0 ** -10 * (2 * 53) ** 0.5
    rows = []
    for k in lr_:
        rows.append((k, lr_[k], la[k]))
        assert abs(la[k] - lr_[k]) <= bound * max(abs(lr_[k]), 1e-3), (k, la[k], lr_[k])
    for n in PROBES:
        a, r = ga[n].double() / 65536.0, gr[n].double()
        rel = float((a - r).norm() / r.norm())
        rows.append((n, rel))
        assert rel <= bound, (n, rel)
    # the heads see a pyramid that differs by the backbone's rounding only
    n = "roi_heads.box_head.0.fc1.weight"
    rows.append((n, float((ga[n].double() - gr[n].double()).norm() / gr[n].double().norm())))
    print(f"AMP against fp32 at {H}x{W} (bound {bound:.3e}):")
    for r in rows:
        print("   ", *r)


def _snapshot(trainer):
    bws = list(trainer.step_fn.bb._bw.values())
    return dict(params=[t.clone() for _, t, _ in trainer.entries], m=[s[0].clone() for s in trainer.opt.state],
                v=[s[1].clone() for s in trainer.opt.state], steps=list(trainer.opt.steps),
                folded=[bw.conv.w.clone() for bw in bws], rotated=[bw._flipped.w.clone() for bw in bws if bw._flipped is not None],
                scales=list(trainer.model.proposal_generator.scales), it=trainer.iteration)


def _same(a, b):
    return all(torch.equal(x, y) for k in ("params", "m", "v", "folded", "rotated") for x, y in zip(a[k], b[k])) and \
        a["steps"] == b["steps"] and a["scales"] == b["scales"] and a["it"] == b["it"]


def test_scaler_skips_on_overflow_and_follows_gradscaler(synthetic_sd):
    """Steps with a small growth interval; one of them at a scale that overflows half at the backbone's gradient operands (the
    non-finite values come out of the kernels, nothing is planted): everything the optimizer owns is bitwise unchanged across it,
    the scale is halved; the scale's trajectory is `torch.amp.GradScaler`'s on the same found-inf sequence."""
    from embodied_object_detection_amd import ops
    dev = torch.device("cuda:0")
    _, tr, _ = _make(synthetic_sd, True)
    tr.scaler = ops.LossScaler(growth_interval=2)
    img, mem, gt, gc = _frame(128, 160, 31, dev)
    gen = lambda: torch.Generator(device=dev).manual_seed(4)
    found, scales = [], []
    for i in range(6):
        if i == 3:
            tr.scaler._scale = 2.0 ** 70                      # any gradient above 2^-54 becomes inf as a half operand
        before = _snapshot(tr)
        tr.step(img, gt, memory=mem, gt_classes=gc, generator=gen())
        torch.cuda.synchronize()
        found.append(tr.last_step_skipped)
        if i == 3:
            assert tr.last_step_skipped and _same(before, _snapshot(tr)) and tr.scaler.get_scale() == 2.0 ** 69
            tr.scaler._scale = scales[-1]                     # back to the range the run was in
        else:
            assert not tr.last_step_skipped and not _same(before, _snapshot(tr))
        scales.append(tr.scaler.get_scale())
    assert found == [False, False, False, True, False, False] and tr.scaler.skipped == 1
    assert tr.iteration == 5 and set(tr.opt.steps) == {5}
    # the same found-inf sequence through torch's class (the forced scale of step 3 aside: ratios between consecutive updates)
    ref = torch.amp.GradScaler("cpu", growth_interval=2)
    p = torch.nn.Parameter(torch.zeros(1))
    o = torch.optim.SGD([p], lr=0.0)
    want = []
    for bad in found:
        ref.scale(torch.zeros(()))
        p.grad = torch.tensor([float("inf") if bad else 1.0])
        ref.step(o)
        ref.update()
        want.append((ref.get_scale(), ref._get_growth_tracker()))
    assert scales[:3] == [w[0] for w in want[:3]] == [65536.0, 131072.0, 131072.0]
    assert tr.scaler._growth_tracker == want[-1][1]
    # after the skip the tracker restarted: two clean steps double the scale again
    assert scales[5] == 2 * scales[4] or scales[4] == 2 * scales[3]


def test_loss_falls_over_eight_amp_steps(synthetic_sd):
    dev = torch.device("cuda:0")
    _, tr, _ = _make(synthetic_sd, True)
    _, ref, _ = _make(synthetic_sd, False)
    img, mem, gt, gc = _frame(128, 160, 41, dev)
    tot = {"amp": [], "fp32": []}
    for name, t in (("amp", tr), ("fp32", ref)):
        for i in range(8):
            losses = t.step(img, gt, memory=mem, gt_classes=gc, generator=torch.Generator(device=dev).manual_seed(4))
            tot[name].append(float(sum(losses.values())))
    print("total loss per step:", {k: [round(x, 4) for x in v] for k, v in tot.items()})
    assert tot["amp"][-1] < tot["amp"][0] and tot["fp32"][-1] < tot["fp32"][0]
    assert abs(tot["amp"][-1] - tot["fp32"][-1]) < 0.05 * tot["fp32"][0]
    assert tr.scaler.skipped == 0


def test_trunk_batch_and_freeze_backbone_under_amp(synthetic_sd):
    from embodied_object_detection_amd.modeling.training import AmpTrainer
    dev = torch.device("cuda:0")
    frames = []
    for i in range(2):
        img, mem, gt, gc = _frame(128, 160, 51 + i, dev)
        obs = torch.ones((mem[0].shape[0],))
        frames.append({"image": img.cpu(), "instances": {"gt_boxes": gt.cpu(), "gt_classes": gc.cpu()}, "memory": mem[0].float().cpu(),
                       "observations": obs, "proj_indices": mem[1].cpu()})
    res = {}
    for tb in (1, 2):
        model, tr, _ = _make(synthetic_sd, True)
        tr.trunk_batch = tb
        tr.fm._exact_sizes.add((128, 160))
        total = tr.forward_backward_frames([frames], generator=torch.Generator(device=dev).manual_seed(9))
        res[tb] = ({k: float(v) for k, v in total.items()}, [None if a is None else a.clone() for a in tr._acc], tr)
    assert res[1][0].keys() == res[2][0].keys()
    for k in res[1][0]:
        assert abs(res[1][0][k] - res[2][0][k]) <= 1e-5 * max(1.0, abs(res[1][0][k])), k
    for g, a, b in zip(res[1][2].groups, res[1][1], res[2][1]):
        if a is not None:
            assert float((a - b).norm()) <= 2e-3 * float(a.norm()) + 1e-12, g["name"]      # the order of summation over the frames
    tr = res[2][2]
    tr.optimizer_step()
    assert not tr.last_step_skipped and tr.scaler._growth_tracker == 1
    # FREEZE_BACKBONE: the trunk half's backward is not run, the unfrozen backbone parameters (map_merge) still carry the scale
    model, fz, _ = _make(synthetic_sd, True, ["MODEL.FREEZE_BACKBONE", True, "MODEL.UNFROZEN_LAYERS", ["roi", "map_merge", "proposal_generator"]])
    assert type(fz) is AmpTrainer and fz.step_fn.backward_fpn is False
    assert [g["name"] for g, s in zip(fz.groups, fz._scaled) if s] == [f"backbone.map_merge_projection{i}.{p}" for i in (1, 2, 3) for p in ("weight", "bias")]
    bb = model.backbone
    frozen = [bb.bottom_up.stem.w.clone(), bb.lateral[4].w.clone(), bb.p6.w.clone()]
    moving = [fz.merge_w[0].clone(), model.roi_heads.stages[1]["fc1"].w.clone()]
    img, mem, gt, gc = _frame(128, 160, 61, dev)
    fz.step(img, gt, memory=mem, gt_classes=gc, generator=torch.Generator(device=dev).manual_seed(1))
    torch.cuda.synchronize()
    assert not fz.last_step_skipped
    assert all(torch.equal(a, b) for a, b in zip(frozen, [bb.bottom_up.stem.w, bb.lateral[4].w, bb.p6.w]))
    assert all(not torch.equal(a, b) for a, b in zip(moving, [fz.merge_w[0], model.roi_heads.stages[1]["fc1"].w]))
    # no memory (MEMORY_TYPE ''): the projections have no gradient and are skipped, the step runs
    _, nm, _ = _make(synthetic_sd, True)
    nm.step(img, gt, memory=None, gt_classes=gc, generator=torch.Generator(device=dev).manual_seed(1))
    assert not nm.last_step_skipped


def test_cli_trains_with_fp16_true_and_resumes(tmp_path):
    """`python -m embodied_object_detection_amd.train_mp3d` in a fresh child process with FP16 True (what the shipped yaml says) on
    synthetic episodes: trains, checkpoints the scaler, and a second invocation with --resume continues from it."""
    out = str(tmp_path / "out")
    common = [sys.executable, "-m", "embodied_object_detection_amd.train_mp3d", "--num-gpus", "1", "--synthetic-size", "128", "160",
              "--synthetic-frames", "4"]
    keys = ["FP16", "True", "MODEL.MEMORY_TYPE", "implicit_memory", "MODEL.MAP_FEAT_FUSION", "sum", "MODEL.MAP_FEATURE_WEIGHT", "5",
            "MODEL.TRAIN_DATA_PATH", str(tmp_path / "none"), "MODEL.TEST_DATA_PATH", str(tmp_path / "none"), "OUTPUT_DIR", out,
            "SOLVER.CHECKPOINT_PERIOD", "2", "SOLVER.IMS_PER_BATCH", "1", "TEST.EVAL_PERIOD", "0"]
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run(common + keys + ["SOLVER.MAX_ITER", "3"], env=env, cwd=ROOT, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    ck = torch.load(os.path.join(out, "model_final.pth"), map_location="cpu", weights_only=False)
    assert ck["scaler"]["scale"] == 65536.0 and ck["scaler"]["_growth_tracker"] >= 2 and ck["scaler"]["growth_interval"] == 2000
    r2 = subprocess.run(common + ["--resume"] + keys + ["SOLVER.MAX_ITER", "6"], env=env, cwd=ROOT, capture_output=True, text=True, timeout=900)
    assert r2.returncode == 0, r2.stdout[-3000:] + r2.stderr[-3000:]
    assert "resuming from" in r2.stdout
    ck2 = torch.load(os.path.join(out, "model_final.pth"), map_location="cpu", weights_only=False)
    assert ck2["iteration"] > ck["iteration"] and ck2["scaler"]["_growth_tracker"] > ck["scaler"]["_growth_tracker"]
