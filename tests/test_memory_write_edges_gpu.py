"""`MemoryWriter` (mw_cover_kernel, mw_scatter_kernel, mw_commit_kernel of csrc/memory.hip) alone against a float64 restatement of the
write, at the edges no other test reaches: more than 64 unique instances (the second ballot pass of `block_band_candidates`, the
`hit1` mask and `cand_s[64 + i]` of the scatter, `w1` / `wt[lane + 64]` / `inst_rows[kl + 64]` of the commit), the overflow of the
scatter's LDS table, pixel counts that are no multiple of 1024, a block with observed but no sampled pixel, a block with no observed
pixel, cell counts that are no multiple of 64, lists with duplicates / out-of-range rows / a count above the capacity, batches, and
the 4-wave commit.

The scenes and the reference live in _write_cases.py.  They have no threshold band (see there), so NOTHING is excluded from the
comparison: `k_out`, the observation counters, the dirty set and the set of written cells are exact, untouched rows and the guard
rows keep their bits, the snapshot is bitwise the normalisation of the kernel's own memory, and every written value is within

    HEAD * [U * (|mean| + |mem0 + mean|) + cover_max * 2^-33 * max|f|]        (HEAD = 2, U = 2^-24)

of float64: the two fp32 roundings of the commit and the 2^-32 fixed-point shares (a share is off by <= 2^-33, a cell's n sampled
pixels hold <= n * cover_max shares, the sum is divided by n).  Every launch runs twice from the same state and must repeat its
bits.  `pytest -s` prints one line per case with the worst fraction of the bound reached."""
import os
import subprocess
import sys
import types
from typing import Dict, List

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if __name__ == "__main__":
    sys.path[:0] = [ROOT, os.path.dirname(os.path.abspath(__file__))]

import _write_cases as WC                                      # noqa: E402
from _write_cases import R_CAP, SENTINEL                       # noqa: E402

gpu = pytest.mark.gpu          # every test below that launches carries it; the reference's own checks do not
DIRTY_SENTINEL = -7


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    from embodied_object_detection_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


# ------------------------------------------------------------------------------------------------
# the reference's own checks (no GPU)
# ------------------------------------------------------------------------------------------------
def test_write_reference_is_the_oracles_write():
    """The float64 restatement against oracle.ops.paste_masks + oracle.memory.memory_write_sparse (fp32, the upstream order) on a tame
    scene: general-position boxes, continuous masks, no sample within 1e-5 of the threshold."""
    from oracle import memory as OM
    from oracle import ops as OO
    g = torch.Generator().manual_seed(17)
    H, W, N, K = 48, 64, 300, 12
    ctr = torch.rand((R_CAP, 2), generator=g) * torch.tensor([float(W), float(H)])
    size = torch.rand((R_CAP, 2), generator=g) * 30 + 6
    boxes = torch.cat([ctr - size / 2, ctr + size / 2], dim=1)
    masks = torch.rand((R_CAP, 28, 28), generator=g)
    f = torch.randn((R_CAP, 512), generator=g)
    featn = 50 * f / f.norm(dim=1, keepdim=True)
    sc = types.SimpleNamespace(H=H, W=W, boxes=boxes.double().numpy(), masks=masks.double().numpy(), featn=featn)
    proj = torch.randint(0, N, (H, W), generator=g)
    det = torch.randint(0, R_CAP, (K + 4,), generator=g)
    det[3] = det[0]
    mem0, obs0 = torch.randn((N, 512), generator=g), torch.randint(0, 3, (N,), generator=g).float()
    ref = WC.write_reference(sc, det.numpy(), K, 100, proj.numpy(), N, mem0, obs0)
    rows = torch.unique(det[:K])
    assert ref["rows"] == rows.tolist() and ref["k"] == len(rows) < K
    v, inside = WC.paste_values(sc.masks[ref["rows"]], sc.boxes[ref["rows"]], H, W, np.float64)
    assert float(np.abs(v - 0.5)[inside].min()) > 1e-5, "the tame scene has a sample at the threshold"
    pasted = OO.paste_masks(masks[rows], boxes[rows], (H, W), 0.5)
    assert np.array_equal(pasted.reshape(len(rows), -1).numpy(), ref["hits"])
    mean, observed_mem = OM.memory_write_sparse(featn[rows], pasted, proj, N)
    assert torch.equal(observed_mem, ref["written"]) and int(observed_mem.sum()) > 20
    upd = torch.zeros((N, 512))
    upd[observed_mem] = mean
    torch.testing.assert_close((mem0 + upd).double(), ref["mem"], rtol=1e-5, atol=1e-4)
    ou = torch.zeros(N)
    ou[torch.unique(proj)] = 1
    assert torch.equal(obs0 + ou, ref["obs"]) and torch.equal(ou.bool(), ref["dirty"])
    none = WC.write_reference(sc, det.numpy(), 0, 100, proj.numpy(), N, mem0, obs0)
    assert none["k"] == 0 and torch.equal(none["mem"], mem0.double()) and torch.equal(none["obs"], obs0) and not none["dirty"].any()


@pytest.mark.parametrize("name", WC.SCENES)
def test_fp32_sampler_is_float64_on_every_scene(name):
    """The condition the whole module rests on: on these inputs the kernel's sampling arithmetic is exact in fp32, so the mask
    decisions are the float64 ones -- samples exactly at the threshold included."""
    sc = WC.scene(name)
    v32, in32 = WC.paste_values(sc.masks[sc.inst], sc.boxes[sc.inst], sc.H, sc.W, np.float32)
    v64, in64 = WC.paste_values(sc.masks[sc.inst], sc.boxes[sc.inst], sc.H, sc.W, np.float64)
    assert v32.dtype == np.float32 and np.array_equal(v32.astype(np.float64), v64) and np.array_equal(in32, in64)
    assert int(((v64 == 0.5) & in64).sum()) >= 1, "samples exactly at the threshold are part of the scenes"
    assert set(np.unique(sc.boxes[sc.inst][:, 2:] - sc.boxes[sc.inst][:, :2])) <= {8.0, 16.0, 32.0, 64.0}
    assert np.array_equal(sc.boxes * 8, np.round(sc.boxes * 8)) and np.array_equal(sc.masks * 16, np.round(sc.masks * 16))


def test_scenes_run_the_paths_they_are_built_for():
    """From the reference alone, before any launch: what the scenes must contain for the kernels' second halves and edge paths to
    run (block = the 1024 pixels of one workgroup of the cover and scatter passes)."""
    for name in ("dense", "dense2"):
        sc = WC.scene(name)
        rows = [int(sc.inst[i]) for i in sc.order]
        f = WC.scene_facts(sc, rows)
        print(name, f)
        assert f["blocks"] == 6 and max(f["n_cand"]) > 64, "a block with more than 64 band candidates"
        assert any(f["high_hit"]), "a sampled pixel covered by a candidate at position >= 64 of its block's list"
        assert any(o > 0 and r % 8 != 0 for o, r in zip(f["observed"], f["first_rank"])), "the sampling phase crosses a block boundary"
        assert f["observed"][1] == 0, "block 1 has no observed pixel"
        assert 1 <= f["observed"][2] <= 7 and f["sampled"][2] == 0, "block 2 has observed pixels, none of them sampled"
        assert max(f["keys"]) > WC.MW_AGG, "with one cell per pixel a block's table entries overflow the LDS table"
        proj, N = WC.proj_image("pixel", sc.H, sc.W)
        det, cnt = sc.det_list(128, 128, "plain")
        ref = WC.write_reference(sc, det, cnt, 128, proj, N, torch.zeros((N, 512)), torch.zeros(N))
        assert ref["k"] == 128 and (ref["wt"][:, 64:] != 0).any(), "a weight row with an entry at instance index >= 64"
        assert ref["cover_max"] == f["cover_max"] >= 8
    f = WC.scene_facts(WC.scene("tail"), [int(r) for r in WC.scene("tail").inst])
    assert f["blocks"] == 3 and any(r % 8 for r in f["first_rank"]) and max(f["n_cand"]) > 64 and any(f["high_hit"])
    f = WC.scene_facts(WC.scene("partial"), [int(r) for r in WC.scene("partial").inst])
    assert f["blocks"] == 1 and f["n_cand"] == [128] and f["high_hit"] == [True] and f["observed"][0] < 28 * 36


# ------------------------------------------------------------------------------------------------
# launching and checking
# ------------------------------------------------------------------------------------------------
_REF: Dict[tuple, dict] = {}


def _state(N: int, seed: int = 0):
    g = torch.Generator().manual_seed(900 + N + seed)
    return torch.randn((N, 512), generator=g), torch.randint(0, 3, (N,), generator=g).float()


def _case(scene: str, unique: int, K_cap: int, style: str, pattern: str, seed: int = 0) -> dict:
    """Inputs and reference of one single-scene case (computed once).  Pattern 'bad': the blocky image with two indices out of range;
    the reference is that of the hand-clamped image."""
    key = (scene, unique, K_cap, style, pattern, seed)
    if key not in _REF:
        sc = WC.scene(scene)
        proj, N = WC.proj_image("blocky" if pattern == "bad" else pattern, sc.H, sc.W, seed)
        given = proj
        if pattern == "bad":
            given = proj.copy()
            given[0, 0], given[5, 7] = N + 100, -3
            proj = proj.copy()
            proj[0, 0], proj[5, 7] = N - 1, 0
        if unique == 0:
            det, cnt = sc.det_list(7, K_cap, "plain")[0], 0              # valid rows behind a count of zero
        else:
            det, cnt = sc.det_list(unique, K_cap, style)
        mem0, obs0 = _state(N, seed)
        ref = WC.write_reference(sc, det, cnt, K_cap, proj, N, mem0, obs0)
        assert ref["k"] == unique
        _REF[key] = dict(sc=sc, N=N, K_cap=K_cap, proj=given, det=det, cnt=cnt, mem0=mem0, obs0=obs0, ref=ref, bad=pattern == "bad",
                         tag=f"{scene} {sc.H}x{sc.W} K {unique}/{K_cap} {style} {pattern} N {N}")
    return _REF[key]


def _launch(dev, wr, cases: List[dict], form: str) -> dict:
    """One call of the writer on the cases' scenes (one scene, or a batch back to back) from their initial state -> host copies of
    everything the call may write, guard rows included."""
    B, N = len(cases), cases[0]["N"]
    up = lambda ts, dt: torch.stack([torch.as_tensor(t) for t in ts]).to(dt).contiguous().to(dev)      # noqa: E731
    featn = up([c["sc"].featn for c in cases], torch.float32)
    boxes = up([c["sc"].boxes for c in cases], torch.float32)
    masks = up([c["sc"].masks for c in cases], torch.float32)
    det = up([c["det"] for c in cases], torch.int32)
    cnt = torch.tensor([c["cnt"] for c in cases], dtype=torch.int32, device=dev)
    proj = up([c["proj"] for c in cases], torch.int32)
    mem = torch.full((B * N + 1, 512), SENTINEL, dtype=torch.float32)
    obs = torch.full((B * N + 1,), SENTINEL, dtype=torch.float32)
    mem[:B * N], obs[:B * N] = torch.cat([c["mem0"] for c in cases]), torch.cat([c["obs0"] for c in cases])
    mem, obs = mem.to(dev), obs.to(dev)
    dirty = torch.full((B * N + 1,), DIRTY_SENTINEL, dtype=torch.int32, device=dev)
    snap = torch.full((B * N + 1, 512), SENTINEL, dtype=torch.float16, device=dev)
    err = torch.zeros((1,), dtype=torch.int32, device=dev)
    wr.k_out.fill_(-1)
    # the snapshot form is given `dirty` as well: it must not write it
    k = wr(featn, boxes, masks, det, cnt, proj, mem[:B * N], obs[:B * N], dirty=dirty[:B * N], err=err,
           snapshot=snap[:B * N] if form == "snapshot" else None)
    torch.cuda.synchronize()
    return dict(k=k.cpu().clone(), mem=mem.cpu(), obs=obs.cpu(), dirty=dirty.cpu(), snap=snap.cpu(), err=int(err.item()))


def _same_bits(a: dict, b: dict) -> bool:
    return all(torch.equal(a[n], b[n]) for n in ("k", "mem", "obs", "dirty")) and torch.equal(a["snap"].view(torch.int16), b["snap"].view(torch.int16)) \
        and a["err"] == b["err"]


def _scene_of(got: dict, b: int, N: int) -> dict:
    s = slice(b * N, (b + 1) * N)
    return dict(k=got["k"][b:b + 1], mem=got["mem"][s], obs=got["obs"][s], dirty=got["dirty"][s], snap=got["snap"][s])


def _check(c: dict, got: dict, form: str, b: int = 0) -> List[str]:
    """Scene `b` of a launch's results against the case's reference -> what is wrong (empty: nothing); prints the case's line."""
    N, ref, mem0 = c["N"], c["ref"], c["mem0"]
    g = _scene_of(got, b, N)
    bad = []
    if int(g["k"][0]) != ref["k"]:
        bad.append(f"k_out {int(g['k'][0])}, expected {ref['k']}")
    if not torch.equal(g["obs"], ref["obs"]):
        bad.append(f"{int((g['obs'] != ref['obs']).sum())} observation counters differ")
    marked = g["dirty"] == 1
    if form == "dirty":
        if not torch.equal(marked, ref["dirty"]) or not bool((g["dirty"][~marked] == DIRTY_SENTINEL).all()):
            bad.append(f"dirty set: {int(marked.sum())} marked, {int(ref['dirty'].sum())} expected, or an unmarked entry was written")
    elif not bool((g["dirty"] == DIRTY_SENTINEL).all()):
        bad.append("the snapshot form wrote `dirty`")
    w = ref["written"]
    if not torch.equal(g["mem"][~w], mem0[~w]):
        bad.append(f"{int((g['mem'][~w] != mem0[~w]).any(1).sum())} rows of cells without a sampled pixel changed")
    if not bool((g["mem"][w] != mem0[w]).any(1).all()):
        bad.append(f"{int((~(g['mem'][w] != mem0[w]).any(1)).sum())} of {int(w.sum())} cells with sampled pixels were not written")
    err = (g["mem"].double() - ref["mem"]).abs()
    frac = float((err[w] / ref["bound"][w]).max()) if bool(w.any()) else 0.0
    if not bool((err <= ref["bound"]).all()):
        i = int((err - ref["bound"]).argmax())
        bad.append(f"{int((err > ref['bound']).sum())} values beyond the bound; cell {i // 512} channel {i % 512}: {float(err.reshape(-1)[i]):.3e} "
                   f"from float64, bound {float(ref['bound'].reshape(-1)[i]):.3e}")
    if form == "snapshot":
        d = ref["dirty"]
        want = torch.where((g["obs"] > 1)[:, None], g["mem"] / g["obs"][:, None], g["mem"]).half()
        if not torch.equal(g["snap"][d].view(torch.int16), want[d].view(torch.int16)):
            bad.append(f"{int((g['snap'][d] != want[d]).any(1).sum())} snapshot rows are not the normalised memory rows")
        if not bool((g["snap"][~d] == SENTINEL).all()):
            bad.append(f"{int((g['snap'][~d] != SENTINEL).any(1).sum())} snapshot rows of untouched cells were written")
    elif not bool((g["snap"] == SENTINEL).all()):
        bad.append("the dirty form wrote the snapshot")
    if (got["err"] != 0) != c["bad"] and got["k"].numel() == 1:
        bad.append(f"error flags {got['err']} with{'' if c['bad'] else 'out'} an out-of-range index")
    tag = f"{c['tag']} {form}" + (f" scene {b}" if got["k"].numel() > 1 else "")
    print(f"{tag:64s} written {int(w.sum()):5d} dirty {int(ref['dirty'].sum()):5d} cover_max {ref['cover_max']:2d}  worst {frac:.3f} of the bound", flush=True)
    return [f"{tag}: {m}" for m in bad]


def _guards(got: dict) -> List[str]:
    ok = bool((got["mem"][-1] == SENTINEL).all()) and float(got["obs"][-1]) == SENTINEL and int(got["dirty"][-1]) == DIRTY_SENTINEL \
        and bool((got["snap"][-1] == SENTINEL).all())
    return [] if ok else ["a guard row was written"]


def _run(dev, wr, cases: List[dict], form: str) -> List[str]:
    """The launch twice from the same state (bitwise repetition), every scene against its reference, the guards."""
    first, second = _launch(dev, wr, cases, form), _launch(dev, wr, cases, form)
    bad = [] if _same_bits(first, second) else [f"{cases[0]['tag']} {form}: the second launch from the same state gave other bits"]
    for b, c in enumerate(cases):
        bad += _check(c, first, form, b)
    return bad + _guards(first)


def _writer(dev, c: dict, batch: int = 1):
    from embodied_object_detection_amd import ops
    return ops.MemoryWriter(c["sc"].H, c["sc"].W, c["N"], c["K_cap"], R_CAP, dev, mask_thresh=WC.THRESH, batch=batch)


# (scene, unique instances, K_cap, list style, index image, output form)
CASES = [("dense", 1, 128, "hostile", "pixel", "dirty"), ("dense", 63, 128, "over", "pixel", "snapshot"),
         ("dense", 64, 128, "hostile", "pixel", "dirty"), ("dense", 65, 128, "plain", "pixel", "snapshot"),
         ("dense", 127, 128, "hostile", "pixel", "dirty"), ("dense", 128, 128, "over", "pixel", "snapshot"),
         ("dense", 128, 128, "plain", "pixel", "dirty"), ("dense", 128, 128, "over", "one", "snapshot"),
         ("dense", 128, 128, "plain", "blocky", "dirty"), ("dense", 128, 128, "over", "bad", "snapshot"),
         ("dense", 65, 128, "hostile", "bad", "dirty"), ("dense", 100, 100, "over", "pixel", "snapshot"),
         ("dense", 100, 100, "over", "blocky", "dirty"),
         ("tail", 128, 128, "over", "pixel", "dirty"), ("tail", 65, 128, "hostile", "blocky", "snapshot"), ("tail", 128, 128, "plain", "one", "dirty"),
         ("partial", 128, 128, "plain", "pixel", "snapshot"), ("partial", 65, 128, "over", "one", "dirty"),
         ("partial", 64, 128, "hostile", "blocky", "dirty"), ("partial", 127, 128, "hostile", "bad", "snapshot")]


@gpu
@pytest.mark.parametrize("scene,unique,K_cap,style,pattern,form", CASES, ids=[" ".join(str(v) for v in c) for c in CASES])
def test_memory_write_edges(dev, scene, unique, K_cap, style, pattern, form):
    c = _case(scene, unique, K_cap, style, pattern)
    bad = _run(dev, _writer(dev, c), [c], form)
    assert not bad, "\n".join(bad)


@gpu
@pytest.mark.parametrize("form", ["dirty", "snapshot"])
def test_one_writer_on_two_scenes_in_a_row(dev, form):
    """The per-frame tables are left zero: after another scene the writer gives the bits a fresh writer gives."""
    a, b = _case("dense", 128, 128, "over", "pixel"), _case("dense2", 65, 128, "hostile", "pixel", seed=1)
    assert a["N"] == b["N"]
    wr = _writer(dev, a)
    bad = _check(a, _launch(dev, wr, [a], form), form)
    after = _launch(dev, wr, [b], form)
    fresh = _launch(dev, _writer(dev, b), [b], form)
    bad += _check(b, after, form) + _guards(after)
    assert _same_bits(after, fresh), "a writer that has written another scene gives other bits than a fresh one"
    assert not bad, "\n".join(bad)


@gpu
@pytest.mark.parametrize("form", ["dirty", "snapshot"])
def test_batch_of_three_is_three_single_scenes(dev, form):
    """batch = 3 with 0, 128 and 5 unique instances: every scene bitwise its single-scene call; the scene without instances keeps
    memory, counters, snapshot and dirty marks bit for bit."""
    cases = [_case("dense", 0, 128, "plain", "pixel", seed=2), _case("dense", 128, 128, "over", "pixel"), _case("dense2", 5, 128, "hostile", "pixel", seed=1)]
    N = cases[0]["N"]
    bad = _run(dev, _writer(dev, cases[0], batch=3), cases, form)
    both = _launch(dev, _writer(dev, cases[0], batch=3), cases, form)
    for b, c in enumerate(cases):
        single = _scene_of(_launch(dev, _writer(dev, c), [c], form), 0, N)
        inb = _scene_of(both, b, N)
        if not (all(torch.equal(single[n], inb[n]) for n in ("k", "mem", "obs", "dirty")) and torch.equal(single["snap"].view(torch.int16), inb["snap"].view(torch.int16))):
            bad.append(f"scene {b} of the batch differs from its single-scene call")
    idle = _scene_of(both, 0, N)
    assert int(idle["k"][0]) == 0 and torch.equal(idle["mem"], cases[0]["mem0"]) and torch.equal(idle["obs"], cases[0]["obs0"])
    assert bool((idle["snap"] == SENTINEL).all()) and bool((idle["dirty"] == DIRTY_SENTINEL).all())
    assert not bad, "\n".join(bad)


def _child() -> int:
    """What the child process runs: one scene, both forms, under the EOD_MW_COMMIT_WAVES it was started with."""
    from embodied_object_detection_amd import _lib
    _lib.load()
    dev = torch.device("cuda:0")
    c = _case("dense", 128, 128, "over", "pixel")
    bad = _run(dev, _writer(dev, c), [c], "dirty") + _run(dev, _writer(dev, c), [c], "snapshot")
    for m in bad:
        print("FINDING", m)
    return 1 if bad else 0


@gpu
def test_four_wave_commit_in_a_child_process(dev):
    """`EOD_MW_COMMIT_WAVES=4` (mw_commit_kernel<., 4>: 4 waves per 64-cell group, the stride-4 cell masks) is read once at load: one
    fresh child process, after this process's own run of the same scene (16 waves) has passed."""
    c = _case("dense", 128, 128, "over", "pixel")
    bad = _run(dev, _writer(dev, c), [c], "dirty")
    assert not bad, "\n".join(bad)
    p = subprocess.run([sys.executable, os.path.abspath(__file__)], env={**os.environ, "EOD_MW_COMMIT_WAVES": "4"}, cwd=ROOT, timeout=240,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    print(p.stdout)
    assert p.returncode == 0, f"child with EOD_MW_COMMIT_WAVES=4 ended with status {p.returncode}:\n{p.stdout[-4000:]}"


if __name__ == "__main__":
    sys.exit(_child())
