"""Place detections on the map (`eod_place_masks`, `ops.place_masks`, `place` on the models): every key of the result against the
exact numpy reference of `_place_cases.py`, with `torch.equal`.

The edge cases are 45 x 37 images (odd: every mask row starts at another alignment) over 19 x 23 = 437 cells, 12 rows of which 10
count; `_place_cases.ROW_NAMES` says what each row holds.  The overflow path is forced with a 16-entry table on the same inputs,
and met with the default table (4096 entries) by one detection over 96 x 96 = 9216 cells of one pixel each.
"""
import numpy as np
import pytest
import torch

import _place_cases as PC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    from embodied_object_detection_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


_EDGE = {}


def edge(dev):
    """The edge cases, built once and left unchanged: host arrays and their device copies."""
    if not _EDGE:
        c = PC.edge_cases()
        _EDGE.update(c, d_masks=torch.from_numpy(c["masks"]).to(dev), d_proj=torch.from_numpy(c["proj"]).to(dev),
                     d_rects=torch.from_numpy(c["rects"]).to(dev), d_count=torch.tensor([PC.COUNT], dtype=torch.int32, device=dev))
    return _EDGE


def check(out, ref, tag=""):
    assert sorted(out) == sorted(PC.KEYS)
    for k in PC.KEYS:
        want = torch.from_numpy(ref[k])
        assert out[k].dtype == torch.int32 and tuple(out[k].shape) == tuple(want.shape), (tag, k)
        assert torch.equal(out[k].cpu(), want), (tag, k, out[k].cpu().tolist(), want.tolist())


def same(a, b, tag=""):
    for k in PC.KEYS:
        assert torch.equal(a[k], b[k]), (tag, k)


@pytest.mark.parametrize("topk", [1, 4, 8])
@pytest.mark.parametrize("with_count", [True, False])
def test_edge_cases(dev, topk, with_count):
    from embodied_object_detection_amd import ops
    c = edge(dev)
    count = c["d_count"] if with_count else None
    out = ops.place_masks(c["d_masks"], c["d_proj"], PC.N_CELLS, count=count, rects=c["d_rects"], topk=topk, exclude_cell=c["exclude_cell"])
    ref = PC.reference(c["masks"], c["proj"], PC.N_CELLS, PC.COUNT if with_count else None, c["rects"], topk, c["exclude_cell"])
    check(out, ref, f"topk {topk} count {with_count}")
    if with_count:                                                               # rows 10 and 11 hold garbage: padding
        assert bool((out["mask_pixels"][10:] == 0).all()) and bool((out["cells"][10:] == -1).all()) and bool((out["cell_pixels"][10:] == 0).all())
    assert int(out["invalid"][9]) == 4 and int(out["invalid"][2]) == 4           # -1, n_cells, INT32_MIN, INT32_MAX under the mask
    assert int(out["distinct"][7]) == 1 and int(out["pixels"][8]) == 0 and int(out["mask_pixels"][8]) > 0
    if topk == 8:
        assert out["cells"][6, :6].tolist() == c["tie_cells"] and out["cells"][6, 6:].tolist() == [-1, -1]


def test_bool_masks_no_rects_no_exclusion(dev):
    from embodied_object_detection_amd import ops
    c = edge(dev)
    ref = PC.reference(c["masks"], c["proj"], PC.N_CELLS, None, None, 4, -1)
    out = ops.place_masks(c["d_masks"] != 0, c["d_proj"], PC.N_CELLS)
    check(out, ref, "bool")
    same(out, ops.place_masks(c["d_masks"], c["d_proj"], PC.N_CELLS), "uint8")
    # a view whose first byte is at an odd address, one row only
    one = c["d_masks"].flatten()[PC.H * PC.W:2 * PC.H * PC.W].view(1, PC.H, PC.W)
    assert one.data_ptr() % 2 == 1
    check(ops.place_masks(one, c["d_proj"], PC.N_CELLS), PC.reference(c["masks"][1:2], c["proj"], PC.N_CELLS), "odd address")
    empty = ops.place_masks(c["d_masks"][:0], c["d_proj"], PC.N_CELLS, topk=3)
    assert empty["cells"].shape == (0, 3) and empty["pixels"].shape == (0,) and empty["cells"].dtype == torch.int32


@pytest.mark.parametrize("topk", [1, 4, 8])
def test_overflow_with_a_sixteen_entry_table(dev, topk):
    """table_log2 = 4: every row with more than a handful of cells goes through the overflow kernel, the full image with 430 of them."""
    from embodied_object_detection_amd import ops
    c = edge(dev)
    ref = PC.reference(c["masks"], c["proj"], PC.N_CELLS, None, c["rects"], topk, c["exclude_cell"])
    assert ref["distinct"][2] >= 300 and int((ref["distinct"] > 16).sum()) >= 5  # more overflowing rows than slots
    kw = dict(rects=c["d_rects"], topk=topk, exclude_cell=c["exclude_cell"])
    small = ops.place_masks(c["d_masks"], c["d_proj"], PC.N_CELLS, table_log2=4, **kw)
    check(small, ref, "table_log2 4")
    for log2 in (5, 8, 12):
        same(small, ops.place_masks(c["d_masks"], c["d_proj"], PC.N_CELLS, table_log2=log2, **kw), f"table_log2 {log2}")


def test_overflow_of_the_default_table(dev):
    """One detection, 96 x 96 pixels, 9216 cells of one pixel each: more than the default table's 4096 entries.  All counts tie, so
    the top T are cells 0 .. T-1."""
    from embodied_object_detection_amd import ops
    assert 1 << ops.PLACE_TABLE_LOG2 < 9216
    proj = torch.arange(9216, dtype=torch.int32, device=dev).view(96, 96)
    masks = torch.ones((1, 96, 96), dtype=torch.uint8, device=dev)
    for T in (1, 8):
        out = ops.place_masks(masks, proj, 9216, topk=T)
        check(out, PC.reference(masks.cpu().numpy(), proj.cpu().numpy(), 9216, topk=T), f"T {T}")
        assert out["cells"][0].tolist() == list(range(T)) and out["cell_pixels"][0].tolist() == [1] * T and int(out["distinct"][0]) == 9216
    # shuffled cells, a few of them twice as heavy
    g = torch.Generator().manual_seed(5)
    p = torch.randperm(9216, generator=g).to(torch.int32)
    p[:40] = p[40:80]
    out = ops.place_masks(masks, p.view(96, 96).to(dev), 9216, topk=8, exclude_cell=int(p[41]))
    check(out, PC.reference(masks.cpu().numpy(), p.view(96, 96).numpy(), 9216, topk=8, exclude_cell=int(p[41])), "shuffled")


def test_determinism_and_workspace(dev):
    from embodied_object_detection_amd import _lib, ops
    c = edge(dev)
    need = ops.place_masks_workspace(PC.K_CAP, PC.N_CELLS)
    assert need == (64 + 12 + 63) // 64 * 64 + 4 * ((PC.N_CELLS + 63) // 64 * 64)
    ws = torch.full((need + 64,), -1, dtype=torch.int32, device=dev)             # 0xFF bytes
    kw = dict(rects=c["d_rects"], topk=8, exclude_cell=c["exclude_cell"])
    for log2 in (4, None):
        ws.fill_(-1)
        a = {k: v.clone() for k, v in ops.place_masks(c["d_masks"], c["d_proj"], PC.N_CELLS, table_log2=log2, workspace=ws, **kw).items()}
        assert bool((ws[need:] == -1).all()), "the call wrote behind its workspace"
        b = ops.place_masks(c["d_masks"], c["d_proj"], PC.N_CELLS, table_log2=log2, workspace=ws, **kw)
        same(a, b, f"table_log2 {log2}")
        check(b, PC.reference(c["masks"], c["proj"], PC.N_CELLS, None, c["rects"], 8, c["exclude_cell"]), f"table_log2 {log2}")
    with pytest.raises(_lib.EodError):
        ops.place_masks(c["d_masks"], c["d_proj"], PC.N_CELLS, workspace=ws[:need - 1])


def test_place_refuses_on_the_host(dev):
    from embodied_object_detection_amd import _lib, ops
    c = edge(dev)
    m, p = c["d_masks"], c["d_proj"]
    ok = dict(masks=m, proj=p, n_cells=PC.N_CELLS)
    bad = [dict(masks=m.to(torch.int32)), dict(masks=m.float()), dict(masks=m[0]), dict(masks=m.cpu()), dict(masks=m[:, :, ::2]),
           dict(masks=m.permute(0, 2, 1)), dict(proj=p.long()), dict(proj=p.float()), dict(proj=p[:, :-1].contiguous()),
           dict(proj=p.t()), dict(proj=p.cpu()), dict(proj=p.view(PC.H, PC.W, 1)), dict(topk=0), dict(topk=9), dict(table_log2=3),
           dict(table_log2=13), dict(n_cells=0), dict(n_cells=-5), dict(count=torch.tensor([3], device=dev)),
           dict(count=torch.tensor([3], dtype=torch.int32)), dict(rects=c["d_rects"][:5]), dict(rects=c["d_rects"].long()),
           dict(rects=c["d_rects"].cpu()), dict(workspace=torch.zeros((ops.place_masks_workspace(PC.K_CAP, PC.N_CELLS),), device=dev)),
           dict(workspace=torch.zeros((ops.place_masks_workspace(PC.K_CAP, PC.N_CELLS) - 1,), dtype=torch.int32, device=dev))]
    for kw in bad:
        args = {**ok, **kw}
        with pytest.raises(_lib.EodError):
            ops.place_masks(args.pop("masks"), args.pop("proj"), args.pop("n_cells"), **args)
    out = ops.place_masks(m, p, PC.N_CELLS, topk=8, table_log2=12, exclude_cell=-1)       # the ends of the ranges are accepted
    assert out["cells"].shape == (PC.K_CAP, 8)


# ---- the models ---------------------------------------------------------------------------------------------------------------
# Seed 0 and 1 of the synthetic sequence (128 x 160 frames, a 24 x 24 map): both give detections whose masks cover map cells.
N_MAP = 24 * 24


def _frames(n, seed=0, H=128, W=160):
    from embodied_object_detection_amd.data.synthetic import SyntheticSequence
    seq = SyntheticSequence(seed, H=H, W=W, n_frames=n, map_w=24, map_h=24, cell=0.5)
    return [seq.frame(i) for i in range(n)]


def _cfg():
    from embodied_object_detection_amd import setup_cfg
    return setup_cfg(None, ["MODEL.MEMORY_TYPE", "implicit_memory", "MODEL.MAP_FEAT_FUSION", "sum", "MODEL.MAP_FEATURE_WEIGHT", 5,
                            "MODEL.MEMORY_CLS_SCORE_THRESH", 0.3])


def _out(model, f):
    o = model([[f]])[0]["instances"]
    return o.pred_boxes.tensor.clone(), o.scores.clone(), o.pred_classes.clone(), o.pred_masks.clone()


def _proj2d(frame):
    return np.asarray(frame["proj_indices"]).reshape(frame["height"], frame["width"]).astype(np.int32)


@pytest.fixture(scope="module")
def single_runs(dev, synthetic_sd):
    """Per seed: the single-scene model after two frames, the second frame's instances and their placement."""
    from embodied_object_detection_amd import build_model
    runs = {}
    for seed in (0, 1):
        model = build_model(_cfg(), synthetic_sd)
        frames = _frames(3, seed)
        model([[frames[0]]])
        inst = model([[frames[1]]])[0]["instances"]
        out = model.place(inst, frames[1]["proj_indices"])
        runs[seed] = dict(model=model, frames=frames, inst=inst, out={k: v.clone() for k, v in out.items()})
    return runs


def test_model_place_equals_the_reference_and_the_op(dev, synthetic_sd, single_runs):
    from embodied_object_detection_amd import _lib, build_model, ops
    placed = 0
    for seed, run in single_runs.items():
        model, frame, inst = run["model"], run["frames"][1], run["inst"]
        assert int(model.implicit_memory.shape[0]) == N_MAP
        proj = _proj2d(frame)
        masks = inst.pred_masks.cpu().numpy()
        ref = PC.reference(masks, proj, N_MAP, topk=4)
        print(f"seed {seed}: {len(inst)} detections, mask pixels {ref['mask_pixels'].tolist()[:12]}, distinct {ref['distinct'].tolist()[:12]}")
        check(run["out"], ref, f"seed {seed}")                                   # the rects cut nothing off the pasted masks
        d_proj = torch.from_numpy(proj).to(dev)
        same(run["out"], ops.place_masks(inst.pred_masks, d_proj, N_MAP, rects=None), f"seed {seed} whole image")
        same(run["out"], model.place(inst, d_proj), "a device tensor")           # [H, W] on the device, as well as [H, W, 1] numpy
        placed += int((run["out"]["pixels"] > 0).sum())
        excl = int(ref["cells"][0, 0]) if len(inst) else -1
        check(model.place(inst, frame["proj_indices"], topk=8, exclude_cell=excl), PC.reference(masks, proj, N_MAP, topk=8, exclude_cell=excl),
              f"seed {seed} topk 8")
    assert placed >= 1, "no detection covers a map cell: pick another seed"
    run = single_runs[0]
    model, frames, inst = run["model"], run["frames"], run["inst"]
    assert not inst.has("pred_cells")
    before = dict(semmap=model.semmap, mem=model.implicit_memory.clone(), obs=model.observations.clone())
    out = model.place(inst, frames[1]["proj_indices"], attach=True)
    assert torch.equal(inst.pred_cells, out["cells"][:, 0]) and torch.equal(inst.pred_cell_pixels, out["cell_pixels"][:, 0])
    assert len(inst.pred_cells) == len(inst)
    assert model.semmap is before["semmap"] and torch.equal(model.implicit_memory, before["mem"]) and torch.equal(model.observations, before["obs"])
    with pytest.raises(_lib.EodError):
        build_model(_cfg(), synthetic_sd).place(inst, frames[1]["proj_indices"])         # no memory yet
    # frame 3 after the queries against a run that never asked
    other = build_model(_cfg(), synthetic_sd)
    for f in frames[:2]:
        other([[f]])
    for a, b in zip(_out(other, frames[2]), _out(model, frames[2])):
        assert torch.equal(a, b)
    assert torch.equal(other.implicit_memory, model.implicit_memory)


def test_lockstep_place_equals_the_single_scene_runs(dev, synthetic_sd, single_runs):
    from embodied_object_detection_amd.modeling.lockstep import LockstepScenes
    ls = LockstepScenes(_cfg(), 2, synthetic_sd)
    outs = ls([list(single_runs[0]["frames"][:2]), list(single_runs[1]["frames"][:2])])
    for b in (0, 1):
        frame = single_runs[b]["frames"][1]
        same(ls.place(b, single_runs[b]["inst"], frame["proj_indices"]), single_runs[b]["out"], f"scene {b}")
        inst = outs[b][1]["instances"]                                           # the batch's own detections of that frame
        check(ls.place(b, inst, frame["proj_indices"]), PC.reference(inst.pred_masks.cpu().numpy(), _proj2d(frame), N_MAP, topk=4), f"scene {b}")
    with pytest.raises(IndexError):
        ls.place(2, single_runs[0]["inst"], single_runs[0]["frames"][1]["proj_indices"])


def test_predictor_place(dev, synthetic_sd):
    from embodied_object_detection_amd.engine.predictor import EmbodiedPredictor
    pred = EmbodiedPredictor(_cfg(), synthetic_sd)
    frames = _frames(2)
    pred.model([[frames[0]]])
    inst = pred.model([[frames[1]]])[0]["instances"]
    out = pred.place(inst, frames[1], topk=3, exclude_cell=5)
    same(out, pred.model.place(inst, frames[1]["proj_indices"], topk=3, exclude_cell=5))
    assert out["cells"].shape == (len(inst), 3)
