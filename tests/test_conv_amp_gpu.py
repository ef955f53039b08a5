"""The f16 arithmetic of the AMP training step, launch by launch (-m gpu): every input-gradient and weight-gradient launch the
backbone's backward really makes (recorded from one `AmpTrainer` step at 640x640 and from a two-frame trunk batch) against fp64 on
the half-rounded operands and on the unrounded ones, the planner's choice per layer, run-to-run bitwise weight gradients over the
position splits, the edges of the f16 weight-gradient kernel's index arithmetic (chunks of 64 positions, empty ranges, half-filled
channel tiles, image boundaries inside a chunk), and IEEE behaviour beyond half's range together with the found-inf pass."""
import math

import pytest
import torch

from _conv_cases import exact_hw

pytestmark = pytest.mark.gpu

U16, U32 = 2.0 ** -11, 2.0 ** -24          # unit roundoffs of binary16 and binary32


def _frame(H, W, seed, dev, n_cells=400):
    g = torch.Generator().manual_seed(seed)
    img = torch.randint(0, 256, (3, H, W), generator=g, dtype=torch.uint8).to(dev)
    mem = ((torch.randn((n_cells, 512), generator=g) * 2).half().to(dev), torch.randint(0, n_cells, (H, W), generator=g).int().to(dev))
    s = min(H, W) / 128.0
    gt = (torch.tensor([[10.0, 12.0, 60.0, 70.0], [40.0, 30.0, 150.0, 120.0], [90.0, 8.0, 118.0, 40.0], [5.0, 80.0, 44.0, 124.0]]) * s).to(dev)
    gc = torch.tensor([1, 4, 9, 17]).int().to(dev)
    return img, mem, gt, gc


@pytest.fixture(scope="module")
def recorded(synthetic_sd):
    """One AMP step at 640x640 and one two-frame trunk batch at 256x320 with `ops.ConvBackward.__call__` and `ops.Conv.__call__`
    wrapped: every backward call that differs in its arguments, and every forward / input-gradient launch's plan."""
    from embodied_object_detection_amd import build_model, ops, setup_cfg
    from embodied_object_detection_amd.modeling.training import build_trainer
    dev = torch.device("cuda:0")
    cfg = setup_cfg(None, ["MODEL.MEMORY_TYPE", "implicit_memory", "MODEL.MAP_FEAT_FUSION", "sum", "MODEL.MAP_FEATURE_WEIGHT", 5,
                           "SOLVER.BASE_LR", 2e-5, "FP16", True])
    sd0 = {k: v.clone() for k, v in synthetic_sd.items()}
    model = build_model(cfg, sd0)
    trainer = build_trainer(model, sd0)
    bw_calls, plans = {}, []
    orig_bw, orig_conv = ops.ConvBackward.__call__, ops.Conv.__call__

    def bw_call(self, x, y, g_out, relu=False, need_dx=True, dx_res=None, dx_gate=None, levels=None):
        out = orig_bw(self, x, y, g_out, relu=relu, need_dx=need_dx, dx_res=dx_res, dx_gate=dx_gate, levels=levels)
        c = self.conv
        if levels is None:
            key = (c.Cin, c.Cout, c.KH, c.stride, c.pad, tuple(x.shape), need_dx, dx_res is not None, dx_gate is not None, self.math)
            bw_calls.setdefault(key, c.name)
        return out

    def conv_call(self, x, N, H, W, **kw):
        out = orig_conv(self, x, N, H, W, **kw)
        plans.append((self.name, kw.get("math"), self.plan()["glds"], bool(self.tap4 or kw.get("in_relu")), kw.get("gate") is not None))
        return out

    ops.ConvBackward.__call__, ops.Conv.__call__ = bw_call, conv_call
    try:
        img, mem, gt, gc = _frame(640, 640, 3, dev)
        trainer.step_fn.grad_scale = 1.0
        trainer.fm.forward_backward(img, gt, gc, memory=mem, generator=torch.Generator(device=dev).manual_seed(1))
        fr = [_frame(256, 320, 5 + i, dev) for i in range(2)]
        mems = [f[1] for f in fr]
        trainer.fm.forward_backward_batch([f[0] for f in fr], [f[2] for f in fr], [f[3] for f in fr], mems,
                                          generator=torch.Generator(device=dev).manual_seed(2))
        torch.cuda.synchronize()
    finally:
        ops.ConvBackward.__call__, ops.Conv.__call__ = orig_bw, orig_conv
    return bw_calls, plans


def test_planner_gives_the_backbone_f16_and_the_heads_fp32(recorded):
    _bw, plans = recorded
    backbone = [p for p in plans if p[1] == "f16"]
    heads = [p for p in plans if p[1] is None]
    assert len(backbone) > 150 and len(heads) > 30
    for name, _m, glds, fp32_layer, _gated in backbone:
        assert glds == (0 if fp32_layer else 3), name              # the 4-channel stem is the only fp32 launch of an f16 call here
    assert sum(1 for p in backbone if p[3]) >= 1                   # ... and it was seen
    assert any(p[4] and p[2] == 3 for p in backbone)               # gated input-gradient launches run the gated f16 tile
    for name, _m, glds, _f, _g in heads:
        assert glds == 0, name                                     # tower, heads' GEMMs, P7 (forward and backward): fp32
    assert any("p7" in p[0] for p in heads) and not any("p7" in p[0] for p in backbone)
    assert not any("tower" in p[0] or "roi_heads" in p[0] or "box_" in p[0] for p in backbone)


def _reference(x, g, w, stride, pad, need_dx, dtype=torch.float64):
    """aten.convolution_backward in float64 on NCHW views -> (dX NHWC or None, dW [Cout, KH*KW*Cin], db)."""
    xn, gn = x.permute(0, 3, 1, 2).to(dtype), g.permute(0, 3, 1, 2).to(dtype)
    dx, dw, db = torch.ops.aten.convolution_backward(gn, xn, w.to(dtype), [w.shape[0]], [stride, stride], [pad, pad], [1, 1], False, [0, 0], 1,
                                                     [need_dx, True, True])
    return (dx.permute(0, 2, 3, 1) if need_dx else None), dw.permute(0, 2, 3, 1).reshape(w.shape[0], -1), db


def test_every_backbone_backward_launch_against_fp64(recorded):
    """Against fp64 on the ROUNDED operands only fp32 accumulation is left: n terms summed in fp32 stay within n * 2^-24 of
    conv(|a|, |b|); against fp64 on the unrounded operands the two roundings add (2^-10 + 2^-22) * conv(|a|, |b|)."""
    from embodied_object_detection_amd import ops
    bw_calls, _plans = recorded
    f16_calls = [(k, n) for k, n in bw_calls.items() if k[-1] == "f16"]
    assert len(f16_calls) >= 30
    assert any(k[7] and k[8] for k, _ in f16_calls) and any(k[3] == 2 for k, _ in f16_calls) and any(k[2] == 3 for k, _ in f16_calls)
    dev = torch.device("cuda:0")
    worst = {"dw_r": 0.0, "dx_r": 0.0, "dw_u": 0.0, "dx_u": 0.0, "dw_mean": 0.0, "dx_mean": 0.0}
    half = lambda t: t.half().double()
    for (Cin, Cout, K, stride, pad, xs, need_dx, res, gate, _m), name in f16_calls:
        if Cin == 4:
            continue                                                # the stem: fp32 kernels in every arithmetic (other modules)
        gen = torch.Generator().manual_seed(hash((Cin, Cout, K, stride, xs)) & 0xFFFF)
        N, H, W, _ = xs
        w = torch.randn((Cout, Cin, K, K), generator=gen) / math.sqrt(Cin * K * K)
        conv = ops.Conv(w, torch.zeros(Cout), stride=stride, pad=pad, device=dev, name=name)
        OH, OW = conv.out_hw(H, W)
        x = torch.relu(torch.randn(xs, generator=gen))
        g = torch.randn((N, OH, OW, Cout), generator=gen)
        r = torch.randn(xs, generator=gen) if res else None
        gt_ = torch.relu(torch.randn(xs, generator=gen)) if gate else None
        bw = ops.ConvBackward(conv, math="f16")
        o = bw(x.to(dev), None, g.to(dev), need_dx=need_dx, dx_res=None if r is None else r.to(dev), dx_gate=None if gt_ is None else gt_.to(dev))
        dxr, dwr, dbr = _reference(half(x), half(g), half(w), stride, pad, need_dx)
        dxu, dwu, _ = _reference(x, g, w, stride, pad, need_dx)
        dxa, dwa, _ = _reference(half(x).abs(), half(g).abs(), half(w).abs(), stride, pad, need_dx)
        _, _, db64 = _reference(x, g, w, stride, pad, False)
        n_w, n_x = N * OH * OW, Cout * K * K
        dw = o["dw"].cpu().double()
        e = (dw - dwr).abs()
        assert bool((e <= n_w * U32 * dwa + 1e-30).all()), (name, "dW vs rounded operands")
        assert bool(((dw - dwu).abs() <= (2.0 ** -10 + 2.0 ** -22 + n_w * U32) * dwa * 1.001 + 1e-30).all()), (name, "dW vs unrounded")
        worst["dw_r"] = max(worst["dw_r"], float((e / (n_w * U32 * dwa + 1e-30)).max()))
        worst["dw_u"] = max(worst["dw_u"], float(((dw - dwu).abs() / ((2.0 ** -10 + 2.0 ** -22 + n_w * U32) * dwa + 1e-30)).max()))
        worst["dw_mean"] = max(worst["dw_mean"], float(e.mean() / dwr.abs().mean()))
        assert float(e.mean() / dwr.abs().mean()) < 1e-4, name      # a truncating conversion or a dropped fragment is far above
        # db: the fp32 sum of the UNROUNDED gradient
        assert torch.allclose(o["db"].cpu().double(), db64, rtol=1e-4, atol=1e-4 * float(db64.abs().max())), name
        if need_dx:
            fin = lambda v: torch.where(gt_.double() > 0, v + (r.double() if r is not None else 0.0), torch.zeros((), dtype=torch.float64)) \
                if gate else (v + r.double() if r is not None else v)
            dx = o["dx"].cpu().double()
            e = (dx - fin(dxr)).abs()
            slack = U32 * (dxa + (r.abs().double() if r is not None else 0.0)) * 4
            assert bool((e <= n_x * U32 * dxa + slack + 1e-30).all()), (name, "dX vs rounded operands")
            assert bool(((dx - fin(dxu)).abs() <= (2.0 ** -10 + 2.0 ** -22 + n_x * U32) * dxa * 1.001 + slack + 1e-30).all()), (name, "dX vs unrounded")
            if gate:
                assert bool((dx[gt_ <= 0] == 0).all()), name
            worst["dx_r"] = max(worst["dx_r"], float((e / (n_x * U32 * dxa + slack + 1e-30)).max()))
            worst["dx_mean"] = max(worst["dx_mean"], float(e.mean() / fin(dxr).abs().mean()))
            assert float(e.mean() / fin(dxr).abs().mean()) < 1e-4, name
    print("worst fractions of the bounds / mean relative errors:", {k: round(v, 6) for k, v in worst.items()})


@pytest.mark.parametrize("shape", [(1, 160, 160, 64, 64, 1, 1), (1, 160, 160, 64, 64, 3, 1), (1, 80, 80, 128, 128, 3, 2), (1, 40, 40, 1024, 256, 1, 1),
                                   (2, 20, 20, 2048, 512, 1, 1), (1, 9, 7, 32, 96, 3, 1), (1, 80, 80, 256, 512, 1, 2)])
def test_weight_gradient_is_bitwise_run_to_run_over_the_position_splits(shape):
    from embodied_object_detection_amd import _lib, ops
    N, H, W, Cin, Cout, K, stride = shape
    dev = torch.device("cuda:0")
    lib = _lib.load()
    pad = K // 2
    need = lib.eod_conv2d_backward_weights_workspace_bytes(N, H, W, Cin, Cout, K, K, pad, stride | ops.WGRAD_F16)
    splits = need // ((Cout * K * K * Cin + Cout) * 4) if need else 1
    assert 1 <= splits <= 64
    gen = torch.Generator().manual_seed(7)
    conv = ops.Conv(torch.randn((Cout, Cin, K, K), generator=gen), torch.zeros(Cout), stride=stride, pad=pad, device=dev, name="t")
    OH, OW = conv.out_hw(H, W)
    x, g = torch.randn((N, H, W, Cin), generator=gen).to(dev), torch.randn((N, OH, OW, Cout), generator=gen).to(dev)
    bw = ops.ConvBackward(conv, math="f16")
    a = bw(x, None, g, need_dx=False)
    other = ops.ConvBackward(ops.Conv(torch.randn((64, 64, 3, 3)), None, pad=1, device=dev, name="o"), math="f16")
    other(torch.randn((1, 24, 24, 64), device=dev), None, torch.randn((1, 24, 24, 64), device=dev), need_dx=False)   # the shared workspace in between
    b = bw(x, None, g, need_dx=False)
    assert torch.equal(a["dw"], b["dw"]) and torch.equal(a["db"], b["db"])
    # ... and differs from the fp32 kernel's by the operand rounding only
    c = ops.ConvBackward(conv)(x, None, g, need_dx=False)
    rel = float((a["dw"] - c["dw"]).abs().mean() / c["dw"].abs().mean())
    assert 1e-6 < rel < 2e-3, rel
    assert torch.allclose(a["db"], c["db"], rtol=1e-5, atol=1e-3)
    print(f"splits {splits}: mean |dW_f16 - dW_fp32| / mean |dW_fp32| = {rel:.2e}")


def test_overflow_is_not_clamped_and_the_found_inf_pass_sees_it():
    from embodied_object_detection_amd import ops
    dev = torch.device("cuda:0")
    gen = torch.Generator().manual_seed(3)
    conv = ops.Conv(torch.randn((64, 64, 3, 3), generator=gen) * 0.05, torch.zeros(64), pad=1, device=dev, name="t")
    x = torch.randn((1, 24, 24, 64), generator=gen).to(dev)
    g = torch.randn((1, 24, 24, 64), generator=gen).to(dev)
    bw = ops.ConvBackward(conv, math="f16")
    clean = bw(x, None, g, dx_gate=torch.ones_like(x))
    opt = ops.AdamW([])
    flag = torch.zeros((1,), dtype=torch.int32, device=dev)
    opt.nonfinite([clean["dw"], None, clean["db"], clean["dx"]], flag)
    assert int(flag.cpu()[0]) == 0 and bool(torch.isfinite(clean["dw"]).all())
    g2 = g.clone()
    g2[0, 10, 10, 5] = 70000.0                                   # above 65504: inf as a half operand, not clamped
    hot = bw(x, None, g2, dx_gate=torch.ones_like(x))
    assert not bool(torch.isfinite(hot["dw"][5]).all()) and bool(torch.isfinite(hot["dw"][6]).all())
    assert not bool(torch.isfinite(hot["dx"][0, 9:12, 9:12]).all())
    assert bool(torch.isfinite(hot["db"]).all())                  # db sums the unrounded fp32 gradient
    fp32 = ops.ConvBackward(conv)(x, None, g2)
    assert bool(torch.isfinite(fp32["dw"]).all() and torch.isfinite(fp32["dx"]).all())
    opt.nonfinite([clean["dw"], hot["dw"]], flag)
    assert int(flag.cpu()[0]) == 1
    flag.zero_()
    many = [torch.zeros((33,), device=dev) for _ in range(70)]   # three launches of the table
    opt.nonfinite(many, flag)
    assert int(flag.cpu()[0]) == 0
    many[67][32] = float("nan")
    opt.nonfinite(many, flag)
    assert int(flag.cpu()[0]) == 1


# ------------------------------------------------------------------------------------------------
# edges of the f16 weight-gradient kernel: the fp32 LDS-tiled kernel's frame with chunks of 64 positions
# (tests/test_conv_backward_plans_gpu.py holds the fp32 twins)
# ------------------------------------------------------------------------------------------------
def _f16_split(shape):
    """(chunks of 64 positions, ranges, chunks per range) of an f16 weight-gradient launch; the ranges from the workspace size the
    library asks for."""
    from embodied_object_detection_amd import _lib, ops
    N, H, W, Cin, Cout, K, stride, pad = shape
    need = _lib.load().eod_conv2d_backward_weights_workspace_bytes(N, H, W, Cin, Cout, K, K, pad, stride | ops.WGRAD_F16)
    assert need % ((Cout * K * K * Cin + Cout) * 4) == 0
    ranges = need // ((Cout * K * K * Cin + Cout) * 4) if need else 1
    P = N * ((H + 2 * pad - K) // stride + 1) * ((W + 2 * pad - K) // stride + 1)
    chunks = -(-P // 64)
    return chunks, ranges, -(-chunks // ranges)


def _poison(shape, dev):
    """NaN in the workspace and in the blocks the caching allocator hands out next for dW / db: a range or an element that is not
    written shows as NaN in the result (a stale value of the previous, identical run would not show)."""
    from embodied_object_detection_amd import ops
    _N, _H, _W, Cin, Cout, K, _s, _p = shape
    ws = ops.ConvBackward._workspace.get(dev)
    if ws is not None:
        ws.fill_(float("nan"))
    junk = [torch.full((Cout, K * K * Cin), float("nan"), device=dev), torch.full((Cout,), float("nan"), device=dev)]
    del junk


def _f16_edges(tag, shapes, seed0):
    """Every shape twice with another layer's call in between (the shared workspace): bitwise equal, fully written, dW within
    n_w * 2^-24 * conv(|a|, |b|) of fp64 on the half-rounded operands and within (2^-10 + 2^-22 + n_w * 2^-24) * conv(|a|, |b|) of
    fp64 on the unrounded ones, db = the fp64 sum of the unrounded gradient."""
    from embodied_object_detection_amd import ops
    dev = torch.device("cuda:0")
    half = lambda t: t.half().double()
    other = ops.ConvBackward(ops.Conv(torch.randn((64, 64, 1, 1)), None, device=dev, name="o"), math="f16")
    ox, og = torch.randn((1, 17, 19, 64), device=dev), torch.randn((1, 17, 19, 64), device=dev)
    bad = []
    for i, shape in enumerate(shapes):
        N, H, W, Cin, Cout, K, stride, pad = shape
        gen = torch.Generator().manual_seed(seed0 + i)
        w = torch.randn((Cout, Cin, K, K), generator=gen) / math.sqrt(Cin * K * K)
        conv = ops.Conv(w, torch.zeros(Cout), stride=stride, pad=pad, device=dev, name=f"{tag} {shape}")
        OH, OW = conv.out_hw(H, W)
        x = torch.relu(torch.randn((N, H, W, Cin), generator=gen))
        g = torch.randn((N, OH, OW, Cout), generator=gen)
        xd, gd = x.to(dev), g.to(dev)
        bw = ops.ConvBackward(conv, math="f16")
        bw(xd, None, gd, need_dx=False)                             # sizes the shared workspace for this layer
        _poison(shape, dev)
        a = bw(xd, None, gd, need_dx=False)
        a = {k: a[k].clone() for k in ("dw", "db")}
        other(ox, None, og, need_dx=False)
        _poison(shape, dev)
        b = bw(xd, None, gd, need_dx=False)
        _, dwr, _ = _reference(half(x), half(g), half(w), stride, pad, False)
        _, dwu, db64 = _reference(x, g, w, stride, pad, False)
        _, dwa, _ = _reference(half(x).abs(), half(g).abs(), half(w).abs(), stride, pad, False)
        n_w = N * OH * OW
        dw, db = b["dw"].cpu().double(), b["db"].cpu().double()
        e_r = float(((dw - dwr).abs() / (n_w * U32 * dwa + 1e-30)).max())
        e_u = float(((dw - dwu).abs() / ((2.0 ** -10 + 2.0 ** -22 + n_w * U32) * dwa * 1.001 + 1e-30)).max())
        print(f"{tag} {shape}: split {_f16_split(shape)}, fractions of the bounds: rounded {e_r:.4f}, unrounded {e_u:.4f}")
        if not (torch.equal(a["dw"], b["dw"]) and torch.equal(a["db"], b["db"])):
            bad.append(f"{shape}: two runs differ")
        if not (bool(torch.isfinite(dw).all()) and bool(torch.isfinite(db).all())):
            bad.append(f"{shape}: dW / db not fully written")
        if not bool(((dw - dwr).abs() <= n_w * U32 * dwa + 1e-30).all()):
            bad.append(f"{shape}: dW vs rounded operands, {e_r:.3f} of the bound")
        if not bool(((dw - dwu).abs() <= (2.0 ** -10 + 2.0 ** -22 + n_w * U32) * dwa * 1.001 + 1e-30).all()):
            bad.append(f"{shape}: dW vs unrounded operands, {e_u:.3f} of the bound")
        if not torch.allclose(db, db64, rtol=1e-4, atol=1e-4 * float(db64.abs().max())):
            bad.append(f"{shape}: db")
    assert not bad, "\n".join(bad)


def test_f16_position_counts_around_a_chunk_multiple():
    """P = 64 k - 1, 64 k, 64 k + 1 (the last chunk holds 63, 64, 1 positions), one range and several."""
    shapes = []
    for P in (63, 64, 65, 64 * 20 - 1, 64 * 20, 64 * 20 + 1):
        h, w = exact_hw(P)
        shapes.append((1, h, w, 64, 64, 3, 1, 1) if h > 1 else (1, h, w, 64, 64, 1, 1, 0))
    assert [_f16_split(s)[1] for s in shapes[:3]] == [1, 1, 1]
    # 64 x 64 channels are one tile per tap: 768 workgroups want 86 ranges (3 x 3) or 64 (1 x 1); a quarter of the 40 / 41 chunks of 32
    # positions caps them at 10
    assert [_f16_split(s)[1] for s in shapes[3:]] == [10, 10, 10]
    _f16_edges("P around 64 k", shapes, 7000)


def test_f16_empty_last_ranges_add_zeros():
    """64 ranges over 130 chunks of 64 positions are 3 chunks per range: ranges 44 .. 63 are EMPTY and must contribute exact zeros to
    the reduce (the workspace holds NaN before each run)."""
    shapes = [(1, 65, 128, 64, 64, 1, 1, 0), (1, 52, 160, 32, 32, 3, 1, 1)]
    for s in shapes:
        chunks, ranges, cps = _f16_split(s)
        assert (chunks, ranges, cps) == (130, 64, 3) and -(-chunks // cps) == 44, (s, chunks, ranges, cps)
    _f16_edges("empty ranges", shapes, 7100)


def test_f16_half_filled_channel_tiles():
    """Cin / Cout of 32, 96 and 160: the 64 x 64 tile's second half is switched off on one or both sides (`g_ok` / `x_ok`, the
    guarded stores), db written by one tile column only."""
    shapes = [(1, 21, 27, ci, co, k, 1, k // 2) for ci, co, k in ((32, 32, 3), (96, 96, 1), (160, 160, 3), (64, 32, 3), (32, 96, 3), (160, 32, 1))]
    _f16_edges("half tiles", shapes, 7200)


def test_f16_image_boundaries_inside_a_chunk():
    """N = 2 and 3 with OH * OW not a multiple of 64: a chunk of 64 positions -- and a loader thread's four consecutive ones -- holds
    the end of one image and the start of the next, whose border taps must not read across."""
    shapes = [(2, 13, 9, 64, 64, 3, 1, 1), (3, 7, 11, 96, 64, 3, 1, 1), (3, 13, 15, 64, 128, 3, 2, 1), (2, 9, 7, 32, 64, 5, 1, 2)]
    for N, H, W, _ci, _co, K, stride, pad in shapes:
        assert (((H + 2 * pad - K) // stride + 1) * ((W + 2 * pad - K) // stride + 1)) % 64
    _f16_edges("image boundaries", shapes, 7300)
