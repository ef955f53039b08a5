"""Training on wide vocabularies through the model: the cascade's losses and gradients at 1203 classes against the CPU oracle, without
and with the federated loss (the class weight read back and checked against its restatement), `Trainer` / `AmpTrainer` steps, a batch
of two frames, checkpoints, and the CLI (train, resume, evaluate)."""
import json
import os
import subprocess
import sys

import pytest
import torch

from _fed_loss_ref import fed_loss_weight_ref
from oracle import losses as OL
from oracle import model as M

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LVIS = os.path.join(ROOT, "tests", "golden", "lvis_v1_clip.npy")
FREQ = os.path.join(ROOT, "tests", "golden", "lvis_v1_cat_freq.json")
C = 1203
# the vocabulary of a 1203-class run: the heads' class count and matrix, and the same for the classifier reset the shipped yaml does
VOCAB = ["MODEL.ROI_HEADS.NUM_CLASSES", C, "MODEL.ROI_BOX_HEAD.ZEROSHOT_WEIGHT_PATH", LVIS, "MODEL.TEST_CLASSIFIERS", f"('{LVIS}',)",
         "MODEL.TEST_NUM_CLASSES", f"[{C}]"]
FED = ["MODEL.ROI_BOX_HEAD.USE_FED_LOSS", True, "MODEL.ROI_BOX_HEAD.CAT_FREQ_PATH", FREQ]
BASE = ["MODEL.MEMORY_TYPE", "implicit_memory", "MODEL.MAP_FEAT_FUSION", "sum", "MODEL.MAP_FEATURE_WEIGHT", 5, "SOLVER.BASE_LR", 2e-5]


@pytest.fixture(scope="module")
def lvis_sd():
    from embodied_object_detection_amd.checkpoint import synthetic_state_dict
    return synthetic_state_dict(0, C, LVIS)


def _boxes(g, n_gt, n_rand, W, H):
    xy = torch.rand((n_gt, 2), generator=g) * torch.tensor([W * 0.6, H * 0.6])
    wh = torch.rand((n_gt, 2), generator=g) * torch.tensor([W * 0.3, H * 0.3]) + 12
    gt = torch.cat([xy, xy + wh], dim=1)
    near = (gt.repeat(6, 1) + torch.randn((6 * n_gt, 4), generator=g) * 3).clamp(min=0)
    rxy = torch.rand((n_rand, 2), generator=g) * torch.tensor([W * 0.8, H * 0.8])
    rwh = torch.rand((n_rand, 2), generator=g) * torch.tensor([W * 0.3, H * 0.3]) + 4
    props = torch.cat([near, torch.cat([rxy, rxy + rwh], dim=1)])
    props[:, 0::2] = props[:, 0::2].clamp(max=W)
    props[:, 1::2] = props[:, 1::2].clamp(max=H)
    return gt.contiguous(), props.contiguous()


def _sparse_freq_file(tmp_path):
    """The LVIS counts with every third category at zero images: what IGNORE_ZERO_CATS masks and the federated draw never takes."""
    cats = json.load(open(FREQ))
    for c in cats:
        if c["id"] % 3 == 0:
            c["image_count"] = 0
    p = tmp_path / "sparse_freq.json"
    p.write_text(json.dumps(cats))
    return str(p)


NAMES = [f"roi_heads.box_head.{k}.{n}" for k in range(3) for n in ("fc1", "fc2")] + \
        [f"roi_heads.box_predictor.{k}.{n}" for k in range(3) for n in ("cls_score.linear", "bbox_pred.0", "bbox_pred.2")]


@pytest.mark.parametrize("mode,H,W,batch", [("plain", 128, 160, 96), ("plain", 640, 640, 512), ("fed", 128, 160, 96), ("fed+zero", 128, 160, 96)])
def test_cascade_losses_and_gradients_at_1203_classes_match_the_oracle(lvis_sd, tmp_path, mode, H, W, batch):
    """`DetectorTraining.losses` + `backward` against `oracle.losses.cascade_training_losses` with 1203 classes on the same proposals
    and keys: sampled rows and labels exact, the six losses, the gradients of the 30 head tensors and of P3..P5, within the
    tolerances of tests/test_detector_training_gpu.py.  With the federated loss the class weight of every stage is read back,
    checked against the restatement for the q the trainer drew, and handed to the oracle's loss."""
    from embodied_object_detection_amd import build_model, setup_cfg
    from embodied_object_detection_amd.modeling.fed_loss import load_class_freq
    from embodied_object_detection_amd.modeling.training import DetectorTraining
    dev = torch.device("cuda:0")
    extra = []
    freq_path = FREQ
    if mode != "plain":
        freq_path = _sparse_freq_file(tmp_path) if mode == "fed+zero" else FREQ
        extra = ["MODEL.ROI_BOX_HEAD.USE_FED_LOSS", True, "MODEL.ROI_BOX_HEAD.CAT_FREQ_PATH", freq_path,
                 "MODEL.ROI_BOX_HEAD.IGNORE_ZERO_CATS", mode == "fed+zero"]
    cfg = setup_cfg(None, BASE + VOCAB + ["MODEL.ROI_HEADS.BATCH_SIZE_PER_IMAGE", batch] + extra)
    model = build_model(cfg, lvis_sd)
    assert model.roi_heads.num_classes == C
    det = DetectorTraining(model)
    freq = load_class_freq(freq_path, 0.5)
    ocfg = M.OracleCfg(num_classes=C)

    def run(seed):
        g = torch.Generator().manual_seed(seed)
        gt, props = _boxes(g, 8, 300 if batch < 512 else 1500, float(W), float(H))
        gc = torch.randint(0, C, (8,), generator=g)
        feats = [(torch.randn((1, 256, H >> (3 + l), W >> (3 + l)), generator=g) * 0.5).requires_grad_() for l in range(3)]
        keys = torch.rand((props.shape[0] + gt.shape[0],), generator=g)
        sd = dict(lvis_sd)
        for n in NAMES:
            for s in ("weight", "bias"):
                sd[f"{n}.{s}"] = lvis_sd[f"{n}.{s}"].clone().float().requires_grad_()
        ref, rstages = OL.cascade_training_losses(feats, props, gt, gc, sd, ocfg, (H, W), keys, batch=batch)
        P = [f.detach().permute(0, 2, 3, 1).contiguous().to(dev) for f in feats]
        gen = torch.Generator(device=dev).manual_seed(seed)
        out = det.losses(P, props.to(dev), gt.to(dev), gc.to(dev), (H, W), keys=keys.to(dev), generator=gen)
        grads, dP = det.backward(P)
        torch.cuda.synchronize()
        if mode != "plain":
            gen2 = torch.Generator(device=dev).manual_seed(seed)
            for k in range(3):
                rec = det.last[k]
                q = torch.empty((C,), device=dev).exponential_(1, generator=gen2)          # stage order 0, 1, 2 from the step's generator
                assert torch.equal(rec["fed_q"], q), k
                cw = rec["class_weight"].cpu()
                want = fed_loss_weight_ref(rec["classes"].cpu(), C, q.cpu(), 50, freq, freq if mode == "fed+zero" else None)
                assert torch.equal(cw, want), (k, (cw != want).nonzero().flatten().tolist()[:8])
                assert 40 <= int(cw.sum()) <= 50 and (mode != "fed+zero" or float(cw[2::3].sum()) == 0.0)       # ids 3, 6, ... have no images
                ref[f"loss_cls_stage{k}"] = OL.sigmoid_cross_entropy_loss(rstages[k]["logits"], rstages[k]["classes"], cw)
        else:
            assert all(rec["class_weight"] is None for rec in det.last)
        sum(ref.values()).backward()
        flips = 0
        for k in range(3):
            assert torch.equal(det.last[k]["classes"].cpu().long(), rstages[k]["classes"]), k
            if k == 0:
                assert torch.equal(det.last[0]["boxes"].cpu(), rstages[0]["boxes"])
            assert float((det.last[k]["logits"].cpu() - rstages[k]["logits"].detach()).abs().max()) <= 5e-3, k
            for a in ("h1", "h2", "hb"):
                flips += int(((det.last[k][a].cpu().view(rstages[k][a].shape) > 0) != (rstages[k][a] > 0)).sum())
            for name in (f"loss_cls_stage{k}", f"loss_box_reg_stage{k}"):
                assert abs(float(out[name]) - float(ref[name].detach())) <= 1e-4 * max(abs(float(ref[name].detach())), 1e-3), (name, float(out[name]))

        def check(mine, theirs, what):
            scale = max(float(theirs.abs().max()), 1e-20)
            err = float((mine - theirs).abs().max())
            l2 = float((mine - theirs).norm()) / max(float(theirs.norm()), 1e-20)
            if flips == 0:
                assert err <= 1e-4 * scale, (what, err / scale)
            assert l2 <= 3e-3 * max(flips, 1) and err <= 5e-2 * scale, (what, l2, err / scale, flips)

        for k in range(3):
            st = model.roi_heads.stages[k]
            for conv, n in ((st["fc1"], f"roi_heads.box_head.{k}.fc1"), (st["fc2"], f"roi_heads.box_head.{k}.fc2"),
                            (st["cls"], f"roi_heads.box_predictor.{k}.cls_score.linear"), (st["bb0"], f"roi_heads.box_predictor.{k}.bbox_pred.0"),
                            (st["bb2"], f"roi_heads.box_predictor.{k}.bbox_pred.2")):
                dw, db = grads[conv.name]
                rw = sd[f"{n}.weight"].grad
                if n.endswith("fc1"):
                    rw = rw.view(-1, 256, 7, 7).permute(0, 2, 3, 1).reshape(rw.shape[0], -1)
                check(dw.cpu(), rw, n + ".weight")
                check(db.cpu(), sd[f"{n}.bias"].grad, n + ".bias")
        for l in range(3):
            rg = feats[l].grad[0].permute(1, 2, 0) if feats[l].grad is not None else torch.zeros(tuple(dP[l].shape))
            check(dP[l].cpu(), rg, f"dP{l + 3}")
        return flips

    counts = []
    for seed in range(51, 57):
        counts.append(run(seed))
        if counts[-1] == 0:
            break
    print(f"{mode} {H}x{W}: ReLU flips per seed from 51:", counts)
    assert counts[-1] == 0, counts


def test_zero_cats_alone_is_a_constant_weight_and_bad_files_are_refused(lvis_sd, synthetic_sd, tmp_path):
    from embodied_object_detection_amd import build_model, setup_cfg
    from embodied_object_detection_amd.modeling.training import DetectorTraining
    sparse = _sparse_freq_file(tmp_path)
    model = build_model(setup_cfg(None, BASE + VOCAB + ["MODEL.ROI_BOX_HEAD.IGNORE_ZERO_CATS", True, "MODEL.ROI_BOX_HEAD.CAT_FREQ_PATH", sparse]),
                        lvis_sd)
    det = DetectorTraining(model)
    assert det.fed is None and int(det.class_weight.sum()) == C - C // 3 and float(det.class_weight[2::3].sum()) == 0.0
    # 1203 frequencies for a 20-class head; a file that is not there
    model20 = build_model(setup_cfg(None, BASE + FED), synthetic_sd)
    with pytest.raises(ValueError, match="1203 categories"):
        DetectorTraining(model20)
    model20.cfg.MODEL.ROI_BOX_HEAD.CAT_FREQ_PATH = str(tmp_path / "missing.json")
    with pytest.raises(FileNotFoundError, match="CAT_FREQ_PATH"):
        DetectorTraining(model20)


def _frames(g, n, H=128, W=160, n_cells=400):
    out = []
    for i in range(n):
        xy = torch.rand((4, 2), generator=g) * torch.tensor([W * 0.5, H * 0.5])
        wh = torch.rand((4, 2), generator=g) * 40 + 10
        obs = torch.randint(0, 6, (n_cells,), generator=g).float()
        out.append({"image": torch.randint(0, 256, (3, H, W), generator=g, dtype=torch.uint8),
                    "instances": {"gt_boxes": torch.cat([xy, xy + wh], dim=1), "gt_classes": torch.randint(0, C, (4,), generator=g)},
                    "memory": (torch.randn((n_cells, 512), generator=g) * obs.clamp(min=1)[:, None]).numpy(), "observations": obs.numpy(),
                    "proj_indices": torch.randint(0, n_cells, (H, W, 1), generator=g).numpy(), "sequence_name": f"s{i}", "memory_reset": i == 0})
    return out


def _trainer(lvis_sd, *extra, amp=False):
    from embodied_object_detection_amd import build_model, setup_cfg
    from embodied_object_detection_amd.modeling.training import build_trainer
    cfg = setup_cfg(None, BASE + VOCAB + FED + ["FP16", amp, *extra])
    sd0 = {k: v.clone() for k, v in lvis_sd.items()}
    model = build_model(cfg, sd0)
    return model, build_trainer(model, sd0), sd0


def test_trainer_steps_at_1203_classes_with_the_federated_loss(lvis_sd, tmp_path):
    """Eight iterations on two frames: finite, the total loss falls, and the whole run repeats bit for bit from the same seed; the
    stepped state dict carries the stage predictors' freq_weight and loads back."""
    from embodied_object_detection_amd import checkpoint
    from embodied_object_detection_amd.modeling.fed_loss import FREQ_KEY, load_class_freq
    from embodied_object_detection_amd.modeling.training import Trainer
    dev = torch.device("cuda:0")
    data = [_frames(torch.Generator().manual_seed(9), 2)]

    def run():
        model, trainer, sd0 = _trainer(lvis_sd)
        assert type(trainer) is Trainer and trainer.fm.det.fed is not None and trainer.fm.det.C == C
        gen = torch.Generator(device=dev).manual_seed(21)
        totals = []
        for _ in range(8):
            losses = trainer.forward_backward_frames(data, generator=gen)
            trainer.optimizer_step()
            totals.append(torch.stack([v.float().reshape(()) for v in losses.values()]).sum())
        torch.cuda.synchronize()
        return [float(t) for t in totals], model, trainer, sd0

    a, model, trainer, sd0 = run()
    b = run()[0]
    print("total loss over eight iterations at 1203 classes, federated:", [round(t, 4) for t in a])
    assert all(t == t and abs(t) < 1e6 for t in a) and a[-1] < a[0]
    assert a == b
    cw = trainer.fm.det.last[0]["class_weight"]
    assert tuple(cw.shape) == (C,) and 40 <= int(cw.sum()) <= 50
    stepped = trainer.state_dict(sd0)
    fw = load_class_freq(FREQ, 0.5)
    path = str(tmp_path / "model_0000008.pth")
    checkpoint.save_checkpoint(path, stepped, iteration=trainer.iteration)
    loaded, report = checkpoint.load_checkpoint(path, C, verbose=False)
    assert report == {"missing": [], "shape_mismatch": [], "unexpected": []}
    assert all(torch.equal(loaded[FREQ_KEY.format(k)], fw) for k in range(3))


def test_amp_trainer_steps_at_1203_classes_with_the_federated_loss(lvis_sd):
    from embodied_object_detection_amd.modeling.training import AmpTrainer
    dev = torch.device("cuda:0")
    model, trainer, _ = _trainer(lvis_sd, amp=True)
    assert type(trainer) is AmpTrainer
    data = [_frames(torch.Generator().manual_seed(10), 2)]
    before = model.roi_heads.stages[0]["cls"].w.clone()
    losses = trainer.forward_backward_frames(data, generator=torch.Generator(device=dev).manual_seed(3))
    trainer.optimizer_step()
    torch.cuda.synchronize()
    assert len(losses) == 10 and all(bool(torch.isfinite(v.float()).all()) for v in losses.values())
    assert not torch.equal(before, model.roi_heads.stages[0]["cls"].w)


def test_a_batch_of_two_frames_sums_the_single_frames_at_1203_classes(lvis_sd):
    """`trunk_batch`: two frames through one trunk pass (forward_backward_batch) against frame by frame, the federated draws taken
    from the same generator in the same order -- as tests/test_detector_training_gpu.py states it at 20 classes."""
    dev = torch.device("cuda:0")
    model, trainer, _ = _trainer(lvis_sd)
    data = [_frames(torch.Generator().manual_seed(11), 2)]
    trainer.trunk_batch = 1
    trainer.forward_backward_frames(data, generator=torch.Generator(device=dev).manual_seed(5))       # the size goes onto the exact path
    trainer._acc = None
    runs = {}
    for tb in (1, 2):
        trainer.trunk_batch = tb
        losses = trainer.forward_backward_frames(data, generator=torch.Generator(device=dev).manual_seed(5))
        torch.cuda.synchronize()
        runs[tb] = ({k: float(v) for k, v in losses.items()}, [None if a is None else a.clone() for a in trainer._acc])
        trainer._acc = None
    (la, ga), (lb, gb) = runs[1], runs[2]
    assert set(la) == set(lb) and len(la) == 10
    for k in la:
        assert abs(la[k] - lb[k]) <= 1e-6 * max(abs(la[k]), 1e-3), (k, la[k], lb[k])
    for a, b, g_ in zip(ga, gb, trainer.groups):
        assert (a is None) == (b is None)
        if a is not None:
            assert float((a - b).abs().max()) <= 1e-5 * max(float(a.abs().max()), 1e-12), g_["name"]


def test_cli_trains_resumes_and_evaluates_at_1203_classes(tmp_path):
    """`python -m embodied_object_detection_amd.train_mp3d` in child processes on synthetic episodes with a 1203-class head and the
    federated loss: three iterations fresh, two more with --resume, --eval-only on the result."""
    out = str(tmp_path / "run")
    common = ["--synthetic-scenes", "1", "--synthetic-frames", "4", "--synthetic-size", "128", "160", "FP16", "False",
              "MODEL.MEMORY_TYPE", "implicit_memory", *[str(v) for v in VOCAB], *[str(v) for v in FED],
              "MODEL.TRAIN_DATA_PATH", str(tmp_path / "none"), "MODEL.TEST_DATA_PATH", str(tmp_path / "none"), "OUTPUT_DIR", out,
              "SOLVER.IMS_PER_BATCH", "1", "SOLVER.CHECKPOINT_PERIOD", "2", "TEST.EVAL_PERIOD", "0"]
    cli = [sys.executable, "-m", "embodied_object_detection_amd.train_mp3d"]
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))

    def run(args):
        r = subprocess.run(cli + args, env=env, cwd=ROOT, capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
        return r.stdout

    o = run(common + ["SOLVER.MAX_ITER", "3"])
    assert "[train] 3 iterations" in o, o[-2000:]
    ck = torch.load(os.path.join(out, "model_final.pth"), map_location="cpu", weights_only=False)
    assert tuple(ck["model"]["roi_heads.box_predictor.2.freq_weight"].shape) == (C,)
    assert tuple(ck["model"]["roi_heads.box_predictor.0.cls_score.zs_weight"].shape) == (512, C + 1)
    o = run(["--resume"] + common + ["SOLVER.MAX_ITER", "5"])
    assert "resuming from" in o, o[-2000:]
    ck2 = torch.load(os.path.join(out, "model_final.pth"), map_location="cpu", weights_only=False)
    assert ck2["iteration"] > ck["iteration"] and "roi_heads.box_predictor.0.freq_weight" in ck2["model"]
    o = run(["--eval-only"] + common + ["MODEL.WEIGHTS", os.path.join(out, "model_final.pth")])
    assert "[eval] all: AP" in o, o[-2000:]
