"""FP16: True without a GPU: the loss scaler's schedule against `torch.amp.GradScaler`, its state in a checkpoint, which trainer the
configuration gets, what stays refused, and the host-side checks of the calls the AMP step adds to the C ABI (the per-call arithmetic
of `eod_conv2d`, the f16 flag of the weight gradient, the found-inf pass and the unscale of `eod_adamw_step_multi`)."""
import ctypes as C
import os
import types

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__
    __graft_entry__.build()
    from embodied_object_detection_amd import _lib
    return _lib.load()


def _torch_trajectory(pattern, **kw):
    """(scale, growth tracker) after every `update()` of a real GradScaler driven through `step` by gradients that are finite or not."""
    sc = torch.amp.GradScaler("cpu", **kw)
    p = torch.nn.Parameter(torch.zeros(1))
    opt = torch.optim.SGD([p], lr=0.0)
    out = []
    for bad in pattern:
        sc.scale(torch.zeros(()))                                  # what `scaler.scale(losses)` does first: the lazy scale tensor
        p.grad = torch.tensor([float("inf") if bad else 1.0])
        sc.step(opt)
        sc.update()
        out.append((sc.get_scale(), sc._get_growth_tracker()))
    return sc, out


PATTERNS = {
    "clean": [0] * 12,
    "inf_first": [1, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0],
    "inf_on_growth_step": [0, 0, 1, 0, 0, 0, 0, 0, 1, 1, 0, 0, 0],
    "alternating": [0, 1] * 8,
}


@pytest.mark.parametrize("name", sorted(PATTERNS))
@pytest.mark.parametrize("kw", [dict(growth_interval=3), dict(growth_interval=1, init_scale=4.0), dict(),
                                dict(init_scale=2.0 ** 20, growth_factor=4.0, backoff_factor=0.25, growth_interval=2)])
def test_loss_scaler_follows_torch_gradscaler(name, kw):
    from embodied_object_detection_amd import ops
    pattern = PATTERNS[name]
    ref, want = _torch_trajectory(pattern, **kw)
    ls = ops.LossScaler(**kw)
    got = []
    for bad in pattern:
        ls.update(bool(bad))
        got.append((ls.get_scale(), ls._growth_tracker))
    assert got == want
    assert ls.skipped == sum(pattern)
    # torch's key names, so the two load each other's state
    sd = ls.state_dict()
    assert sd == ref.state_dict()
    other = ops.LossScaler()
    other.load_state_dict(ref.state_dict())
    assert (other.get_scale(), other._growth_tracker, other.growth_interval) == (ls.get_scale(), ls._growth_tracker, ls.growth_interval)
    back = torch.amp.GradScaler("cpu")
    back.load_state_dict(sd)
    assert back.get_scale() == ls.get_scale() and back._get_growth_tracker() == ls._growth_tracker


def test_loss_scaler_default_interval_and_fp32_overflow():
    from embodied_object_detection_amd import ops
    ls = ops.LossScaler()
    assert ls.get_scale() == 65536.0 and ls.growth_interval == 2000
    for _ in range(1999):
        ls.update(False)
    assert ls.get_scale() == 65536.0 and ls._growth_tracker == 1999
    ls.update(False)
    assert ls.get_scale() == 131072.0 and ls._growth_tracker == 0
    big = ops.LossScaler(init_scale=2.0 ** 127, growth_interval=1)
    big.update(False)                                # 2^128 is not an fp32 number: torch keeps the scale
    assert big.get_scale() == 2.0 ** 127
    with pytest.raises(ValueError):
        ops.LossScaler(growth_factor=1.0)
    off = ops.LossScaler(enabled=False)
    off.update(True)
    assert off.get_scale() == 1.0 and off.state_dict() == {}


def test_checkpoint_keeps_the_scaler_state_under_its_own_key(tmp_path):
    from embodied_object_detection_amd import checkpoint, ops
    sd = {"backbone.fpn_output3.bias": torch.arange(4.0)}
    ls = ops.LossScaler(growth_interval=5)
    for bad in (0, 0, 1, 0):
        ls.update(bool(bad))
    path = str(tmp_path / "model_0000003.pth")
    checkpoint.save_checkpoint(path, sd, 3, optimizer=None, scheduler={"last_epoch": 4}, scaler=ls.state_dict())
    obj = torch.load(path, map_location="cpu", weights_only=False)
    assert obj["scaler"] == ls.state_dict() and set(obj) >= {"model", "iteration", "scheduler", "scaler"}
    st = checkpoint.load_training_state(path)
    assert st["scaler"] == ls.state_dict() and st["iteration"] == 3 and st["scheduler"] == {"last_epoch": 4}
    fresh = ops.LossScaler()
    fresh.load_state_dict(st["scaler"])
    assert (fresh.get_scale(), fresh._growth_tracker, fresh.growth_interval) == (32768.0, 1, 5)
    # a file without the key (an fp32 run's, or the reference's own): the resumed scaler starts at the initial scale
    path2 = str(tmp_path / "model_0000004.pth")
    checkpoint.save_checkpoint(path2, sd, 4, scheduler={"last_epoch": 5})
    assert "scaler" not in torch.load(path2, map_location="cpu", weights_only=False)
    assert checkpoint.load_training_state(path2)["scaler"] is None


def test_train_loop_restores_logs_and_saves_the_scaler(tmp_path):
    """`do_train` with a stub trainer that owns a scaler: the state of `resume_state['scaler']` is loaded, the rows carry the scale and
    the skipped steps, the checkpoints the scaler's state."""
    from embodied_object_detection_amd import checkpoint, ops, setup_cfg
    from embodied_object_detection_amd.engine import train_loop

    class StubModel:
        def __init__(self, tr):
            self.tr = tr

        def train(self):
            pass

        def __call__(self, data):
            self.tr.step_fn.grad_scale = self.tr.scaler.get_scale()
            return {"loss": torch.tensor(1.0)}

    class StubTrainer:
        def __init__(self):
            self.scaler = ops.LossScaler(growth_interval=2)
            self.step_fn = types.SimpleNamespace(grad_scale=1.0)
            self.n = 0

        def optimizer_step(self, lr_factor=1.0):
            self.scaler.update(self.n == 1)              # the second iteration overflows
            self.n += 1

        def state_dict(self, base):
            return dict(base)

    cfg = setup_cfg(None, ["SOLVER.MAX_ITER", 6, "SOLVER.CHECKPOINT_PERIOD", 100, "TEST.EVAL_PERIOD", 0])
    tr = StubTrainer()
    rows = train_loop.do_train(cfg, StubModel(tr), tr, iter([[]] * 6), output_dir=str(tmp_path), base_state_dict={"w": torch.zeros(1)})
    assert [r["loss_scale"] for r in rows] == [65536.0, 65536.0, 32768.0, 32768.0, 65536.0, 65536.0]
    assert [r["skipped_steps"] for r in rows] == [0, 1, 1, 1, 1, 1]
    st = checkpoint.load_training_state(os.path.join(str(tmp_path), "model_final.pth"))
    assert st["scaler"] == tr.scaler.state_dict()
    tr2 = StubTrainer()
    train_loop.do_train(cfg, StubModel(tr2), tr2, iter([]), resume_state=st)
    assert tr2.scaler.state_dict() == tr.scaler.state_dict()
    # a state without the key leaves the fresh scaler alone; a trainer without a scaler adds nothing to the rows
    tr3 = StubTrainer()
    train_loop.do_train(cfg, StubModel(tr3), tr3, iter([]), resume_state={k: v for k, v in st.items() if k != "scaler"})
    assert tr3.scaler.get_scale() == 65536.0


def test_build_trainer_follows_the_config_key(monkeypatch):
    from embodied_object_detection_amd.modeling import training
    made = []
    monkeypatch.setattr(training, "AmpTrainer", lambda model, sd: made.append("amp") or "A")
    monkeypatch.setattr(training, "Trainer", lambda model, sd: made.append("fp32") or "T")
    on = types.SimpleNamespace(cfg=types.SimpleNamespace(FP16=True))
    off = types.SimpleNamespace(cfg=types.SimpleNamespace(FP16=False))
    assert training.build_trainer(on, {}) == "A" and training.build_trainer(off, {}) == "T" and made == ["amp", "fp32"]


def test_default_configuration_is_the_shipped_yaml_with_fp16_on():
    """`setup_cfg` without a file is the recurrent yaml, whose FP16 key is True: the training commands run AMP unless told otherwise."""
    from embodied_object_detection_amd import setup_cfg
    assert bool(setup_cfg(None, []).FP16) is True
    assert bool(setup_cfg(None, ["FP16", False]).FP16) is False


def test_direct_trainer_still_refuses_fp16_and_every_trainer_the_process_wide_mode():
    """Host only: both refusals come before anything touches a device."""
    from embodied_object_detection_amd import ops
    from embodied_object_detection_amd.modeling import training
    model = types.SimpleNamespace(cfg=types.SimpleNamespace(FP16=True))
    with pytest.raises(NotImplementedError, match="FP16.*build_trainer"):
        training.Trainer(model, {})
    with pytest.raises(NotImplementedError, match="FP16"):
        training.ProposalTrainer(model, {})
    assert training.AmpTrainer.amp and not training.Trainer.amp and issubclass(training.AmpTrainer, training.Trainer)
    prev = ops.set_conv_math("f16")
    try:
        with pytest.raises(ValueError, match="inference only"):
            training.AmpTrainer(object(), {})
        with pytest.raises(ValueError, match="inference only"):
            training.AmpTrainer.optimizer_step(object())
    finally:
        ops.set_conv_math(prev)
    assert ops.get_conv_math() == prev


def _desc(lib):
    from embodied_object_detection_amd import _lib
    d, p = _lib.EodConvDesc(), _lib.EodConvPlan()
    buf = (C.c_float * 64)()
    a = C.addressof(buf)
    a += (-a) % 16
    d.x = d.w = d.y = a
    d.N, d.H, d.W, d.Cin, d.OH, d.OW, d.Cout, d.KH, d.KW, d.stride, d.pad, d.Kpad = 1, 40, 40, 64, 40, 40, 64, 3, 3, 1, 1, 576
    d.out_scale = 1.0
    return d, p, a, buf


def test_per_call_arithmetic_of_the_planner(lib):
    """EodConvDesc.math: 0 follows the process-wide mode, 1 / 2 / 3 choose fp32 / bf16x3 / f16 for the call whatever the mode is; a
    gated call gets the f16 family only when the CALL asks for f16 (the process-wide inference mode keeps gated launches fp32)."""
    d, p, a, _buf = _desc(lib)
    assert lib.eod_get_conv_math() == 0
    want = {0: 0, 1: 0, 2: 2, 3: 3}
    for m, glds in want.items():
        d.math = m
        assert lib.eod_conv2d_plan(C.byref(d), C.byref(p)) == 0 and p.glds == glds, m
    for m in (-1, 4):
        d.math = m
        assert lib.eod_conv2d_plan(C.byref(d), C.byref(p)) == -1
    prev = lib.eod_set_conv_math(2)
    try:
        d.math = 1                                               # an fp32 call inside the process-wide f16 mode
        assert lib.eod_conv2d_plan(C.byref(d), C.byref(p)) == 0 and p.glds == 0
        d.math, d.gate = 0, a                                    # gated, process-wide f16: fp32 64x64 as before
        assert lib.eod_conv2d_plan(C.byref(d), C.byref(p)) == 0 and (p.glds, p.tile) == (0, 3)
    finally:
        lib.eod_set_conv_math(prev)
    d.math, d.gate, d.res, d.res_mode = 3, a, a, 1               # gated + residual, f16 by the call: the gated f16 64x64 tile
    assert lib.eod_conv2d_plan(C.byref(d), C.byref(p)) == 0 and (p.glds, p.tile, p.bm, p.bn, p.bk, p.wavek) == (3, 3, 64, 64, 32, 0)
    for ft, ok in ((93, True), (83, True), (94, False), (84, False), (53, False)):
        d.force_tile = ft
        assert (lib.eod_conv2d_plan(C.byref(d), C.byref(p)) == 0) == ok, ft
        if ok:
            assert (p.glds, p.tile) == (3, 3)
    d.force_tile, d.math = 93, 0                                 # without the per-call f16 a gated f16 tile stays refused
    assert lib.eod_conv2d_plan(C.byref(d), C.byref(p)) == -1
    d.force_tile, d.math, d.in_relu = 0, 3, 1                    # in_relu (P7) and the stem stay fp32 in every arithmetic
    assert lib.eod_conv2d_plan(C.byref(d), C.byref(p)) == 0 and p.glds == 0
    d.in_relu, d.gate, d.res, d.res_mode = 0, None, None, 0
    d.Cin, d.tap4, d.KH, d.KW, d.pad, d.Kpad, d.stride, d.OH, d.OW = 4, 1, 7, 7, 3, 224, 2, 20, 20
    assert lib.eod_conv2d_plan(C.byref(d), C.byref(p)) == 0 and p.glds == 0


def test_weight_gradient_f16_flag_is_checked_on_the_host(lib):
    from embodied_object_detection_amd import ops
    assert ops.WGRAD_F16 == 512
    a = C.addressof((C.c_float * 64)())
    a += (-a) % 16
    F = ops.WGRAD_F16
    args = (1, 56, 56, 64, 64, 3, 3, 1)
    same = lib.eod_conv2d_backward_weights_workspace_bytes(*args, 1)
    assert same > 0 and lib.eod_conv2d_backward_weights_workspace_bytes(*args, 1 | F) == same       # the same position ranges
    assert lib.eod_conv2d_backward_weights_workspace_bytes(*args, F) == 0                           # stride 0
    assert lib.eod_conv2d_backward_weights_ws(None, a, *args, 1 | F, a, a, None, 0, None) == -4     # EOD_ERR_NULL
    assert lib.eod_conv2d_backward_weights_ws(a, a, 1, 56, 56, 4, 64, 7, 7, 3, 2 | F, a, a, None, 0, None) == -1   # the stem has no f16 form
    assert lib.eod_conv2d_backward_weights_ws(a, a, 1, 56, 56, 48, 64, 3, 3, 1, 1 | F, a, a, None, 0, None) == -1  # Cin % 32
    assert lib.eod_conv2d_backward_weights_ws(a + 4, a, *args, 1 | F, a, a, None, 0, None) == -2    # EOD_ERR_ALIGN
    assert lib.eod_conv2d_backward_weights_ws(a, a, *args, 1 | F, a, a, a, 16, None) == -5          # EOD_ERR_CAPACITY


def test_found_inf_pass_and_unscale_are_checked_on_the_host(lib):
    from embodied_object_detection_amd import _lib
    assert [n for n, _t in _lib.EodAdamWTensor._fields_][-2:] == ["inv_scale", "found_inf"]
    assert [n for n, _t in _lib.EodConvDesc._fields_][-1] == "math"
    a = C.addressof((C.c_float * 64)())
    a += (-a) % 16
    t = (_lib.EodAdamWTensor * 2)()
    for d in t:
        d.grad, d.n, d.found_inf = a, 8, a
    call = lambda n: lib.eod_adamw_step_multi(t, n, 0.9, 0.999, 1e-8, 0.0, None)
    t[1].param = a                                               # check entries and step entries do not mix
    assert call(2) == -1
    t[1].param, t[1].found_inf = None, a + 16                    # one flag per call
    assert call(2) == -1
    t[1].found_inf, t[0].found_inf = None, None                  # a check without a flag
    assert call(2) == -4
    t[0].found_inf = t[1].found_inf = a
    t[1].grad = None
    assert call(2) == -4
    s = (_lib.EodAdamWTensor * 1)()
    s[0].param = s[0].grad = s[0].exp_avg = s[0].exp_avg_sq = a
    s[0].n, s[0].lr, s[0].step, s[0].inv_scale = 8, 1e-3, 1, -1.0
    assert lib.eod_adamw_step_multi(s, 1, 0.9, 0.999, 1e-8, 0.0, None) == -1      # a negative unscale factor
