"""`roi_align` in the forms only the inference frame uses -- `box_rows` (the mask pooler's gathered list, S = 14), `refine` (the
cascade: deltas applied on load, `boxes_out` written) and `batch` > 1 (one list per image with a count each, or one list of global
indices) -- against the float64 `RoiRef` of tests/_launch_cases.py with the bound of test_training_launches_gpu.py
(`roi_forward_reference`: ROI_HEAD * U * (8 * level extent + cells a bin touches) * sum of the touched magnitudes), and at the sizes
where the kernel's loops take another trip: 172 x 196 = 33 712 (ROI, bin) waves against the launch's 8192 workgroups x 4 waves, so
rows 168 .. 171 are pooled on the grid-stride loop's second trip; C = 512 (two channel trips) and C = 64 (lanes 16 .. 63 idle).

Every output is pre-filled with a sentinel and has a guard row behind it, every launch runs twice from the same state and must
repeat its bits; the images of a batch hold different features.  `pytest -s` prints one line per comparison with the worst fraction
of the bound reached."""
import os
import sys
from typing import List, Sequence

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if __name__ == "__main__":
    sys.path[:0] = [ROOT, os.path.dirname(os.path.abspath(__file__))]

from _launch_cases import SENTINEL, hostile_boxes, roi_forward_reference, roi_geometry      # noqa: E402

pytestmark = pytest.mark.gpu

IMG_H, IMG_W = 480, 640
SHAPES = [(60, 80), (30, 40), (15, 20)]
SCALE_CLAMP = 4.135166556742356            # log(1000 / 16)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    from embodied_object_detection_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def _pyramids(C: int, batch: int, seed: int) -> List[List[torch.Tensor]]:
    """feats[b][l] [h, w, C]: every image its own values and its own offset (an ROI pooled from the wrong image is far off)."""
    g = torch.Generator().manual_seed(seed)
    return [[torch.randn((h, w, C), generator=g) + 0.5 + 0.25 * b for h, w in SHAPES] for b in range(batch)]


def _device_levels(feats, dev) -> List[torch.Tensor]:
    return [torch.stack([f[l] for f in feats]).contiguous().to(dev) for l in range(3)]


def _compare(tag: str, got: torch.Tensor, boxes: torch.Tensor, image_of: Sequence[int], feats, S: int) -> List[str]:
    """got [R,S,S,C] (host) row by row against RoiRef of boxes[r] on the pyramid of image image_of[r].  Rows whose box is not finite
    must be all zero (the kernel's `sane` guard: they pool nothing)."""
    bad = []
    finite = torch.isfinite(boxes).all(1)
    if not bool((got[~finite] == 0).all()):
        bad.append(f"{tag}: a row with a non-finite box is not all zero")
    boxes = torch.where(finite[:, None], boxes, torch.zeros_like(boxes))
    img = torch.as_tensor(list(image_of))
    worst = 0.0
    for b in sorted(set(img.tolist())):
        idx = (img == b).nonzero().flatten()
        rr, ref, bound = roi_forward_reference(boxes[idx], S, SHAPES, feats[b])
        err = (got[idx].double() - ref).abs()
        ratio = err / bound.clamp(min=1e-300)
        worst = max(worst, float(ratio[bound > 0].max()) if bool((bound > 0).any()) else 0.0)
        if not bool((err <= bound).all()):
            i = int(ratio.argmax())
            r = int(idx[i // (S * S * got.shape[-1])])
            bad.append(f"{tag}: image {b} row {r}: {float(err.reshape(-1)[i]):.3e} from float64, bound {float(bound.reshape(-1)[i]):.3e} "
                       f"({int((err > bound).sum())} elements of {int((err > bound).any(-1).any(-1).any(-1).sum())} rows above their bound)")
    lv = roi_geometry(boxes, S)[0].bincount(minlength=3).tolist()
    print(f"{tag:60s} rows {boxes.shape[0]:4d} per level {lv}  worst {worst:.3f} of the bound", flush=True)
    return bad


def _pool(dev, levels, C: int, boxes: torch.Tensor, count, R_cap: int, S: int, **kw):
    """One launch into a sentinel-filled output with a guard row -> the whole buffer on the host."""
    from embodied_object_detection_amd import ops
    out = torch.full((R_cap + 1, S, S, C), SENTINEL, dtype=torch.float32, device=dev)
    ops.roi_align(levels[0], levels[1], levels[2], SHAPES[0][0], SHAPES[0][1], C, boxes, count, R_cap, S, out=out[:R_cap], **kw)
    torch.cuda.synchronize()
    return out.cpu()


def _twice(run):
    a, b = run(), run()
    same = all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(a, b))
    return a, ([] if same else ["the second launch from the same state gave other bits"])


def _i32(v, dev):
    return torch.tensor(v, dtype=torch.int32, device=dev)


# ------------------------------------------------------------------------------------------------
# box_rows, S = 14: the grid-stride loop's second trip
# ------------------------------------------------------------------------------------------------
def test_box_rows_list_beyond_one_trip_of_the_grid(dev):
    S, C, R_cap = 14, 256, 172
    assert 167 * S * S < 8192 * 4 <= 168 * S * S + S * S and R_cap * S * S > 8192 * 4          # rows 168 .. 171: second trip
    boxes = hostile_boxes(IMG_H, IMG_W, 200, 41)
    g = torch.Generator().manual_seed(42)
    rows = torch.cat([torch.randperm(200, generator=g)[:150], torch.randint(0, 200, (R_cap - 150,), generator=g)])
    rows[168:172] = torch.tensor([57, 3, 123, 57])                     # ordinary boxes (one a repeat, one at a border) on the second trip
    assert rows.unique().numel() < R_cap and bool((rows[168:] >= 1).all())
    feats = _pyramids(C, 1, 43)
    lv = [l[0] for l in _device_levels(feats, dev)]
    bd, rd = boxes.to(dev), rows.int().to(dev)
    bad = []
    for count in (R_cap, 129):
        (out,), rep = _twice(lambda: (_pool(dev, lv, C, bd, _i32([count], dev), R_cap, S, box_rows=rd),))
        tag = f"box_rows S 14 R_cap {R_cap} count {count}"
        bad += [f"{tag}: {m}" for m in rep]
        bad += _compare(tag, out[:count], boxes[rows[:count]], [0] * count, feats, S)
        if not bool((out[count:] == SENTINEL).all()):
            bad.append(f"{tag}: rows beyond the count or the guard row were written")
    assert not bad, "\n".join(bad)


# ------------------------------------------------------------------------------------------------
# channel trips
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [512, 64])
def test_channel_trips(dev, C):
    """C = 512: a lane's second trip of `c0 += 256`; C = 64: lanes 16 .. 63 have no channel."""
    S, R = 7, 48
    boxes = hostile_boxes(IMG_H, IMG_W, R, 50 + C)
    feats = _pyramids(C, 1, 51)
    lv = [l[0] for l in _device_levels(feats, dev)]
    (out,), bad = _twice(lambda: (_pool(dev, lv, C, boxes.to(dev), None, R, S),))
    bad += _compare(f"plain S 7 C {C}", out[:R], boxes, [0] * R, feats, S)
    assert bool((out[R:] == SENTINEL).all()), "the guard row was written"
    assert not bad, "\n".join(bad)


# ------------------------------------------------------------------------------------------------
# refine
# ------------------------------------------------------------------------------------------------
def _deltas(boxes: torch.Tensor, ld: int, weights, seed: int, edge_rows: bool) -> torch.Tensor:
    """[R, ld] deltas whose refined boxes move by up to about a box size and change their size by up to e^+-1.5 (they cross borders
    and change level); columns behind the fourth hold a sentinel.  `edge_rows`: row 0 has its dw far above the scale clamp, row 1 is
    all NaN, row 2 has dx = +inf."""
    g = torch.Generator().manual_seed(seed)
    R = boxes.shape[0]
    d = torch.full((R, ld), SENTINEL)
    d[:, :4] = (torch.rand((R, 4), generator=g) * 2 - 1) * torch.tensor([0.8, 0.8, 1.5, 1.5]) * torch.tensor(weights)
    if edge_rows:
        d[0, :4] = torch.tensor([0.1 * weights[0], -0.1 * weights[1], 3.0 * SCALE_CLAMP * weights[2], 0.2 * weights[3]])
        d[1, :4] = float("nan")
        d[2, :4] = torch.tensor([float("inf"), 0.0, 0.0, 0.0])
    return d


def _refined(dev, boxes, deltas, ld, weights, clip, count, R_cap, batch=1):
    """`ops.apply_deltas` of the same inputs into a sentinel-filled list with a guard row -> host.  `R_cap` rows in all: `batch` lists
    of R_cap / batch (eod_apply_deltas takes the capacity of ONE list)."""
    from embodied_object_detection_amd import ops
    assert R_cap % batch == 0 and count.numel() == batch and boxes.shape[0] == R_cap and deltas.shape[0] == R_cap
    out = torch.full((R_cap + 1, 4), SENTINEL, dtype=torch.float32, device=dev)
    ops.apply_deltas(deltas, ld, boxes, out[:R_cap], count, R_cap // batch, weights, clip, float(IMG_W), float(IMG_H), batch=batch)
    torch.cuda.synchronize()
    return out.cpu()


@pytest.mark.parametrize("weights,ld,clip", [((10.0, 10.0, 5.0, 5.0), 4, True), ((30.0, 30.0, 15.0, 15.0), 8, False),
                                              ((10.0, 10.0, 5.0, 5.0), 8, False), ((30.0, 30.0, 15.0, 15.0), 4, True)])
def test_refine_on_load(dev, weights, ld, clip):
    """The ROI's box is apply_deltas(boxes, deltas): `boxes_out` bitwise `ops.apply_deltas` of the same inputs, the pooled rows those
    of `boxes_out`; a row whose refined box is not finite pools zeros."""
    S, C, R_cap, count = 7, 256, 96, 90
    boxes = hostile_boxes(IMG_H, IMG_W, R_cap, 61)
    boxes[:3] = torch.tensor([100.0, 100.0, 140.0, 130.0])              # the edge rows refine an ordinary box
    deltas = _deltas(boxes, ld, weights, 62 + ld, edge_rows=True)
    feats = _pyramids(C, 1, 63)
    lv = [l[0] for l in _device_levels(feats, dev)]
    bd, dd, cnt = boxes.to(dev), deltas.to(dev), _i32([count], dev)

    def run():
        bo = torch.full((R_cap + 1, 4), SENTINEL, dtype=torch.float32, device=dev)
        out = _pool(dev, lv, C, bd, cnt, R_cap, S, refine=(dd, ld, weights, clip, float(IMG_W), float(IMG_H), bo[:R_cap]))
        return out, bo.cpu()

    (out, bo), bad = _twice(run)
    tag = f"refine weights {weights[0]:g} ld {ld} clip {int(clip)}"
    want = _refined(dev, bd, dd, ld, weights, clip, cnt, R_cap)
    assert torch.equal(bo.view(torch.int32), want.view(torch.int32)), f"{tag}: boxes_out is not apply_deltas of the same inputs, bit for bit"
    assert bool((bo[count:] == SENTINEL).all()) and bool((out[count:] == SENTINEL).all()), f"{tag}: rows beyond the count or a guard row were written"
    new = bo[:count]
    # what the inputs are built for
    assert float(new[0, 2] - new[0, 0]) == pytest.approx(min(40.0 * 62.5, IMG_W if clip else 1e9), rel=1e-4), "row 0 sits at the scale clamp"
    assert not bool(torch.isfinite(new[1:3]).all(1).any()) or clip, "rows 1 and 2 are not finite without the clip"
    assert bool((out[1:3] == 0).all()), f"{tag}: the NaN and +inf rows must pool zeros"
    fin = torch.isfinite(new).all(1) & torch.isfinite(boxes[:count]).all(1)
    l0, l1 = roi_geometry(boxes[:count][fin], S)[0], roi_geometry(new[fin], S)[0]
    assert int((l0 != l1).sum()) >= 5, "refined boxes change level"
    assert bool((new[fin][:, 0] < 0).any() or clip) and bool(((new[fin][:, 2] >= IMG_W) | (new[fin][:, 3] >= IMG_H)).any()), "refined boxes cross borders"
    bad += _compare(tag, out[:count], new, [0] * count, feats, S)
    assert not bad, "\n".join(bad)


# ------------------------------------------------------------------------------------------------
# batches
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("refine", [False, True])
def test_segmented_batch(dev, refine):
    """The cascade's form: batch = 3, one list of 43 boxes per image with a count each (43, 0, 17); rows beyond an image's count
    are written neither in `out` nor in `boxes_out`."""
    S, C, B, per = 7, 256, 3, 43
    counts, R_cap = (43, 0, 17), B * per
    weights, ld, clip = (20.0, 20.0, 10.0, 10.0), 4, True
    boxes = hostile_boxes(IMG_H, IMG_W, R_cap, 71)
    boxes = boxes[torch.randperm(R_cap, generator=torch.Generator().manual_seed(72))].contiguous()
    deltas = _deltas(boxes, ld, weights, 73, edge_rows=False)
    feats = _pyramids(C, B, 74)
    lv = _device_levels(feats, dev)
    bd, dd, cnt = boxes.to(dev), deltas.to(dev), _i32(list(counts), dev)

    def run():
        bo = torch.full((R_cap + 1, 4), SENTINEL, dtype=torch.float32, device=dev)
        kw = dict(refine=(dd, ld, weights, clip, float(IMG_W), float(IMG_H), bo[:R_cap])) if refine else {}
        return _pool(dev, lv, C, bd, cnt, R_cap, S, batch=B, boxes_per_image=per, **kw), bo.cpu()

    (out, bo), bad = _twice(run)
    tag = f"segmented batch 3 x 43 counts {counts}" + (" refine" if refine else "")
    live = torch.cat([torch.arange(b * per, b * per + counts[b]) for b in range(B)])
    dead = torch.ones(R_cap + 1, dtype=torch.bool)
    dead[live] = False
    assert bool((out[dead] == SENTINEL).all()), f"{tag}: rows beyond an image's count or the guard row were written"
    used = boxes
    if refine:
        want = _refined(dev, bd, dd, ld, weights, clip, cnt, R_cap, batch=B)
        assert torch.equal(bo.view(torch.int32), want.view(torch.int32)), f"{tag}: boxes_out is not apply_deltas of the same inputs, bit for bit"
        assert bool((bo[dead] == SENTINEL).all()), f"{tag}: boxes_out rows beyond an image's count or its guard row were written"
        used = bo[:R_cap]
    else:
        assert bool((bo == SENTINEL).all())
    bad += _compare(tag, out[live], used[live], (live // per).tolist(), feats, S)
    assert not bad, "\n".join(bad)


def test_box_rows_over_the_images_of_a_batch(dev):
    """The mask pooler's form: one list of global box indices over all images, S = 14; row i pools box rows[i] from image
    rows[i] // boxes_per_image."""
    S, C, B, per = 14, 256, 3, 43
    R_cap, count = 64, 57
    boxes = hostile_boxes(IMG_H, IMG_W, B * per, 81)
    boxes = boxes[torch.randperm(B * per, generator=torch.Generator().manual_seed(82))].contiguous()
    g = torch.Generator().manual_seed(83)
    rows = torch.randint(0, B * per, (R_cap,), generator=g)
    rows[:4] = torch.tensor([0, B * per - 1, per - 1, per])             # the first and last box of the batch, an image boundary
    assert set((rows[:count] // per).tolist()) == {0, 1, 2}
    feats = _pyramids(C, B, 84)
    lv = _device_levels(feats, dev)
    (out,), bad = _twice(lambda: (_pool(dev, lv, C, boxes.to(dev), _i32([count], dev), R_cap, S, box_rows=rows.int().to(dev), batch=B,
                                        boxes_per_image=per),))
    tag = f"box_rows batch 3 S 14 count {count} of {R_cap}"
    assert bool((out[count:] == SENTINEL).all()), f"{tag}: rows beyond the count or the guard row were written"
    bad += _compare(tag, out[:count], boxes[rows[:count]], (rows[:count] // per).tolist(), feats, S)
    assert not bad, "\n".join(bad)
