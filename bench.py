#!/usr/bin/env python
"""Headline benchmark: frames/s of the per-frame recurrent inference path on synthetic 640x640 sequences,
MODEL.MEMORY_TYPE implicit_memory, MAP_FEAT_FUSION sum (BASELINE.json metric / configs[2]).

    python bench.py --gpus N --steps K --warmup W
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P bench.py --gpus N ...

A step = one frame through the whole hot path (memory read -> backbone -> proposals -> cascade -> masks x2 ->
post-process -> memory write), inputs (u8 image, int32 proj_indices) already resident in HBM.  One process per GPU,
independent scenes per rank (weak scaling, no data-path collective); after the timed region the ranks exchange their
per-rank detection records with ONE RCCL all-reduce (fixed-shape buffer, each rank fills its slice) for the aggregate
AP50, as the north star asks.  Rank 0 prints one JSON line.

A plain run does what the headline needs and nothing more: set up, warm up, time the K steps, write `--dump-outputs`, print the
line (metric, value, ms_per_step, the static configuration).  `--full` goes on, after the same timed region, with everything
else the line can carry: the untimed replay for the per-frame counts, the rooflines of the dominant kernel and of the HBM-bound
class, the sibling and variant timings (host inputs, enqueue only, mask work as the reference issues it, bf16x3, lock-step,
configs[4] at 960x960, the training iteration), the AP50 collective and the CPU baseline.  The `--no-*` switches trim a `--full` run.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

PEAK_F32_MFMA_TFLOPS = 157.3   # MI355X microarchitecture guide: v_mfma_f32_32x32x2_f32, dense
PEAK_BF16_MFMA_TFLOPS = 2500.0  # same guide: bf16 dense (v_mfma_f32_32x32x16_bf16, 32 cycles per SIMD)
PEAK_HBM_GBPS = 8000.0
EPISODE_LEN = 20               # Detic/SMNet/loader.py: episodes of 20 frames; train_mp3d.py:186 passes one episode per call
DUMP_LIMIT_BYTES = 64 << 20    # --dump-outputs writes at most this much
DUMP_MASK_PIXELS = 32768       # mask pixels sampled per dumped step (shared by the B frames of a --batch step): at the 300
                               # detections a frame can return, 300 x 32768 float32 = 39 MB


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=15, help="untimed frames (clocks and the caching allocator settle in ~10)")
    ap.add_argument("--size", type=int, nargs=2, default=[640, 640], metavar=("H", "W"))
    ap.add_argument("--grid", type=int, nargs=2, default=[200, 200], metavar=("MAP_W", "MAP_H"))
    ap.add_argument("--cell", type=float, default=0.2)
    ap.add_argument("--memory-thresh", type=float, default=0.3, help="MODEL.MEMORY_CLS_SCORE_THRESH (0.0 = worst-case write path)")
    ap.add_argument("--full", action="store_true",
                    help="after the timed steps also measure and check everything beside the headline: per-frame counts (untimed "
                         "replay), rooflines, variants, the AP50 collective, the CPU baseline; the --no-* switches below trim it")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--cpu-budget-s", type=float, default=240.0, help="stop the CPU baseline after this many seconds of frames")
    ap.add_argument("--cpu-frames", type=int, default=20, help="timed CPU frames (SURVEY 8d: >= 20)")
    ap.add_argument("--cpu-warmup", type=int, default=5, help="untimed CPU warm-up frames (SURVEY 8d: 5)")
    ap.add_argument("--no-config5", action="store_true", help="skip variants.config5_960_batch4 (BASELINE configs[4] at full size)")
    ap.add_argument("--no-train-step", action="store_true", help="skip variants.train_step_640 (one training iteration of forward_model)")
    ap.add_argument("--no-kernel-events", action="store_true", help="do not bracket the dominant kernel with events")
    ap.add_argument("--no-variants", dest="variants", action="store_false", help="skip the extra (non-headline) variant timings")
    ap.add_argument("--concurrent-scenes", type=int, default=0, help="with --batch: scenes in flight at once (0 = BatchedSequences decides)")
    ap.add_argument("--lockstep", choices=["launches", "streams"], default="launches",
                    help="with --batch: 'launches' = N = B through every stage, one launch per stage (modeling/lockstep.py); 'streams' = "
                         "B scene objects on their own streams, only the trunk batched (modeling/batched.py)")
    ap.add_argument("--batch", type=int, default=1, help="B independent sequences per GPU in lock-step (BASELINE configs[4]: "
                    "--size 960 960 --grid 512 512 --cell 0.08 --batch 4); a step = B frames")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write the Instances the last timed step returned as DIR/<name>.npy (float32 / float64; "
                         "the masks as a fixed sample of pixel positions + every whole mask's area), for comparing two builds")
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be at least 1 and --warmup at least 0")
    return args


def frame_roofline(H: int, W: int, n_prop: float, n_det: float, sec_per_frame: float, math: str, n_mask_rois: float = None) -> dict:
    """Algorithmic FLOPs of one whole frame (2 x MAC of every conv / linear layer) against the time of a frame.
    `n_mask_rois`: ROIs the mask head really ran on (detections + the proposals the memory update reads, when the proposal masks
    are computed lazily); default = the reference's n_prop + n_det."""
    px = (H // 8) * (W // 8)                                   # P3 positions; P4 = /4, P5 = /16, P6 ~ /64, P7 ~ /256
    lv = px * (1 + 1 / 4 + 1 / 16) + ((H // 64) * (W // 64)) + (-(-H // 128) * -(-W // 128))
    s = H * W / (640.0 * 640.0)
    g = {"resnet50": 66.8 * s, "fpn_p6p7": 13.0 * s, "memory_projections": 2.2 * s,
         "centernet_head": 2.0 * lv * 2304 * (4 * 256 + 5) / 1e9, "cascade_box_heads": 23.8 * n_prop / 256.0,
         "mask_head": 1.028 * (n_prop + n_det if n_mask_rois is None else n_mask_rois)}
    total = sum(g.values())
    ach = total / sec_per_frame / 1e3
    return {"algorithmic_gflop_per_frame": round(total, 1), "by_stage_gflop": {k: round(v, 1) for k, v in g.items()},
            "achieved_tflops": round(ach, 2), "frac_of_fp32_mfma_peak": round(ach / PEAK_F32_MFMA_TFLOPS, 4),
            "note": "every FLOP of the frame over the frame time" + ("" if math == "fp32" else " (bf16x3 arithmetic: algorithmic fp32 FLOPs)")}


def available_cores() -> int:
    """Cores this process may really use: affinity mask and cgroup quota, not the host's total."""
    n = os.cpu_count() or 1
    try:
        n = min(n, len(os.sched_getaffinity(0)))
    except (AttributeError, OSError):
        pass
    for path in ("/sys/fs/cgroup/cpu.max", "/sys/fs/cgroup/cpu/cpu.cfs_quota_us"):
        try:
            with open(path) as fh:
                parts = fh.read().split()
            if path.endswith("cpu.max"):
                if parts[0] != "max":
                    n = min(n, max(1, int(int(parts[0]) / int(parts[1]))))
            else:
                q = int(parts[0])
                if q > 0:
                    with open("/sys/fs/cgroup/cpu/cpu.cfs_period_us") as fh2:
                        n = min(n, max(1, q // int(fh2.read().split()[0])))
        except (OSError, ValueError, IndexError):
            pass
    return max(1, min(n, 32))


def _profile_json(name):
    """The newest committed summary of that name (profiles/r04_*.json, else r03_*, r02_*), with the file it came from."""
    for rnd in ("r04", "r03", "r02"):
        try:
            with open(os.path.join(ROOT, "profiles", f"{rnd}_{name}.json")) as fh:
                d = json.load(fh)
            if isinstance(d, dict):
                d.setdefault("_file", f"profiles/{rnd}_{name}.json")
            return d
        except (OSError, ValueError):
            continue
    return None


def pmc_traffic():
    """HBM bytes per launch of the dominant kernel from the committed rocprofv3 PMC passes (FETCH_SIZE x2 gfx950 correction +
    WRITE_SIZE, separate passes: profiles/r04_dominant_kernel_traffic.json).  PMC counters cannot be read live from here."""
    d = _profile_json("dominant_kernel_traffic")
    try:
        return round(float(d["traffic_bytes_per_launch"]), 1)
    except (TypeError, KeyError, ValueError):
        return None


def hbm_class_probe(model, frames, idx, H, W, n_cells, reps=30, gather_frames=None):
    """The HBM-bound class: memory read = a4 (obs-normalise + fp16 cast) + a8 (gather, cascaded pooling, three 1x1
    projections, x weight, fusion into P3..P5), on the frame's real data, each kernel bracketed by HIP events on the stream it is
    launched on, one stream, `reps` repetitions.  Algorithmic bytes are the reference algorithm's (full-map normalise, U = N):
        4 P + N (512*4 + 4) + 2*256*4 * sum_l h_l w_l + 3*512*256*4
    The build moves far fewer (dirty rows only, distinct rows per tile once); `achieved` = algorithmic bytes / measured time."""
    from embodied_object_detection_amd import ops
    f = frames[idx]
    follow = model.snapshot_follows_write
    model.snapshot_follows_write = False       # this frame's write only MARKS its rows: the stand-alone normalise has work to do
    model.inference_frame(frames[idx - 1], refresh_memory_snapshot=True, materialize=False)
    model.snapshot_follows_write = follow
    torch.cuda.synchronize()
    snap = model._dirty.clone()
    n_dirty = int(snap.sum().item())
    proj = f["proj_indices"]
    shapes, off, feats, views, pooled = model.backbone._plan(H, W, 0)
    names = ("normalize_dirty_f16_kernel", "gather_pool_kernel", "project_fuse_kernel")
    # Each kernel: `batch` back-to-back launches between ONE pair of events, `reps` times; duration = median / batch.  (A pair of
    # events around a single 10-20 us launch adds ~5 us of bracket to it: profiles/r02_mem_bench_rocprof.txt.)  The normalise
    # consumes its dirty flags, so every launch is preceded by the 160 KB copy that restores them and the copies alone are
    # timed the same way and subtracted.
    batch = 20
    blocker = torch.empty((64 << 20,), dtype=torch.float32, device=proj.device)      # 256 MB fill: ~0.2 ms of a busy chip

    def timed(body, pre=None):
        out = []
        for _ in range(reps // 3):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            # ~1 ms of work first, so that the host has queued the whole batch before it starts: streaming fills rather than a
            # spin kernel, which leaves the chip idle long enough for its clocks to drop (in a frame these kernels follow dense work)
            for _f in range(5):
                blocker.fill_(0.0)
            a.record()
            for _i in range(batch):
                if pre is not None:
                    pre()
                if body is not None:
                    body()
            b.record()
            torch.cuda.synchronize()
            out.append(a.elapsed_time(b) * 1e3 / batch)
        return float(np.median(out[2:]))

    restore = lambda: model._dirty.copy_(snap)
    t_restore = timed(None, restore)
    us = [max(0.0, timed(lambda: ops.memory_normalize_dirty_f16(model.implicit_memory, model.observations, model._dirty, model._mem_f16),
                         restore) - t_restore),
          0.0,
          timed(lambda: model.backbone.merge(pooled, feats, H, W, model.backbone.map_feature_weight, "sum"))]
    # the gather's cost depends on the frame's index image (how many distinct cells a 16x16 pixel quadrant and a 4x4 block see:
    # 14.7-20.1 us over the frames of the synthetic scene, tools/gather_by_frame.py): mean over frames spread over the timed region
    gf = [i for i in (gather_frames or [idx]) if 0 <= i < len(frames)]
    per_frame = {i: timed(lambda p_=frames[i]["proj_indices"]: ops.memory_gather_pool(model._mem_f16, p_, H, W, out=pooled, err=model._err))
                 for i in gf}
    us[1] = float(np.mean(list(per_frame.values())))
    restore()
    ops.memory_normalize_dirty_f16(model.implicit_memory, model.observations, model._dirty, model._mem_f16)
    model._dirty_pending = False
    # The product path (TEST_TYPE default / episodic) has no normalise launch: the memory write refreshes the snapshot rows of the
    # cells it touches (EodMemWriteDesc.snapshot_f16).  Its cost = the same write replayed with and without the snapshot.
    standalone_a4 = us[0]
    folded = None
    if getattr(model, "_last_write", None) is not None and (follow if follow is not None else model.test_type in ("default", "episodic")):
        keep = (model.implicit_memory.clone(), model.observations.clone(), model._mem_f16.clone())
        pb, pm, rows_, cnt_, pj = model._last_write
        wr = model._writer
        scratch = torch.zeros_like(model._dirty)
        w_mark = lambda: wr(model.roi_heads.featn0, pb, pm, rows_, cnt_, pj, model.implicit_memory, model.observations, dirty=scratch)
        w_snap = lambda: wr(model.roi_heads.featn0, pb, pm, rows_, cnt_, pj, model.implicit_memory, model.observations,
                            snapshot=model._mem_f16)
        t_mark = [timed(w_mark) for _ in range(2)]
        t_snap = [timed(w_snap) for _ in range(2)]
        folded = max(0.0, min(t_snap) - min(t_mark))
        model.implicit_memory.copy_(keep[0]); model.observations.copy_(keep[1]); model._mem_f16.copy_(keep[2])
        us[0] = folded
        names = ("snapshot rows inside eod_memory_write (mw_obs_snapshot_kernel - mw_obs_kernel)",) + names[1:]
    rows = sum(h * w for (h, w) in shapes[:3])
    # ---- memory read + fusion (a4 + a8): SURVEY 8(d) bytes = 4 P + U (512*4 + 4) + 2*256*4 * sum h_l w_l + 3*512*256*4 ----------------
    fixed = 4 * H * W + 2 * 256 * 4 * rows + 3 * 512 * 256 * 4
    alg_full = fixed + n_cells * (512 * 4 + 4)          # U = N: the reference's full-map clone + divide + cast of every frame
    alg_u = fixed + n_dirty * (512 * 4 + 4)             # U = the cells this frame really touches
    # a4: the stand-alone incremental normalise on the frame's rows (an upper bound of what the write-through snapshot adds to
    # the memory write; `folded` = the replayed-write difference is reported beside it)
    us_read = [standalone_a4, us[1], us[2]]
    tot = sum(us_read)
    traffic = None
    try:
        if (H, W, n_cells) == (640, 640, 40000):        # the committed PMC passes were taken on this configuration
            traffic = round(float(_profile_json("hbm_class_traffic")["traffic_bytes_total_x2_reads"]), 1)
    except (TypeError, KeyError, ValueError):
        pass

    def rate(nbytes, t_us):
        g = nbytes / (t_us * 1e-6) / 1e9
        return {"bytes": int(nbytes), "achieved": round(g, 1), "frac": round(g / PEAK_HBM_GBPS, 4)}

    by_def = {"reference_algorithm_U_eq_N": rate(alg_full, tot), "frame_measured_U": rate(alg_u, tot)}
    if traffic:
        by_def["counter_traffic"] = rate(traffic, tot)

    # ---- memory write (a16-a19): SURVEY 8(d) bytes = 4 P + K 784*4 + K 512*4 + (P_obs / 8) 4 + 2 U' 512*4 + 2*4 U_frame ---------------
    write = None
    unproj = None
    try:
        pb, pm, rows_, cnt_, pj = model._last_write
        keep = (model.implicit_memory.clone(), model.observations.clone(), model._mem_f16.clone())
        wr = model._writer
        scratch = torch.zeros_like(model._dirty)
        wr(model.roi_heads.featn0, pb, pm, rows_, cnt_, pj, model.implicit_memory, model.observations, dirty=scratch)
        torch.cuda.synchronize()
        K = int(wr.k_out.item())
        u_written = int((model.implicit_memory != keep[0]).any(dim=1).sum().item())
        u_frame = int(scratch.sum().item())
        # observed pixels: the union of the K pasted instance masks (the product's paste kernel; counted with torch after the timed region)
        urows = torch.unique(rows_[:int(cnt_.item())].long())
        pasted = torch.zeros((max(K, 1), H, W), dtype=torch.uint8, device=pb.device)
        if K:
            ops.paste_masks(pm, pb[urows].contiguous(), urows.to(torch.int32).contiguous(), torch.tensor([K], dtype=torch.int32, device=pb.device),
                            K, H, W, 0.5, pasted)
        p_obs = int(pasted[:K].any(dim=0).sum().item())
        del pasted
        t_write = timed(lambda: wr(model.roi_heads.featn0, pb, pm, rows_, cnt_, pj, model.implicit_memory, model.observations,
                                   snapshot=model._mem_f16))
        model.implicit_memory.copy_(keep[0]); model.observations.copy_(keep[1]); model._mem_f16.copy_(keep[2])
        w_bytes = 4 * H * W + K * 784 * 4 + K * 512 * 4 + (p_obs // 8) * 4 + 2 * u_written * 512 * 4 + 2 * 4 * u_frame
        write = dict(rate(w_bytes, t_write), us=round(t_write, 2), launches=3, memory_instances=K, observed_pixels=p_obs,
                     sampled_pixels=p_obs // 8 + (1 if p_obs % 8 else 0), written_cells=u_written, cells_hit=u_frame,
                     note="eod_memory_write (cover + scatter + commit, incl. the fp16 snapshot rows), 20 back-to-back launches of the "
                          "frame's own write between one pair of events")
        # ---- un-projection (a1 + a2): 4 P read + 4 P write + 64 B ----------------------------------------------------------------------
        from embodied_object_detection_amd.data.synthetic import intrinsics_from_vfov, transform3d
        depth = torch.rand((H, W), device=pb.device) * 5 + 1
        T = transform3d((10.0, 1.5, 10.0, 0.3, 3.14159265))
        intr = intrinsics_from_vfov(W, H)
        side = int(round(n_cells ** 0.5))
        t_un = timed(lambda: ops.unproject_grid_index(depth, T, intr, (0.0, 0.0, 0.0), (-5.0, 0.0, -5.0), 0.2, side, max(1, n_cells // side)))
        unproj = dict(rate(8 * H * W + 64, t_un), us=round(t_un, 2), note="eod_unproject_grid_index (depth -> world xyz -> cell index)")
    except Exception as e:      # diagnostics only
        log(f"write / un-projection probe failed: {e!r}")
    head = by_def["frame_measured_U"]
    return {"bound": "hbm", "class": "memory read + fusion (a4 + a8)",
            "kernels": {"normalize_dirty_f16_kernel (stand-alone a4 on the frame's rows)": round(us_read[0], 2),
                        "gather_pool_kernel (F.avg_pool2d summation order)" if model.backbone.pool_in_torch_order else "gather_pool_kernel":
                            round(us_read[1], 2),
                        "project_fuse_kernel": round(us_read[2], 2)},
            "achieved": head["achieved"], "peak": PEAK_HBM_GBPS, "unit": "GB/s", "frac": head["frac"], "algorithmic_bytes": head["bytes"],
            "traffic": traffic, "avg_us_total": round(tot, 2), "by_definition": by_def,
            "a4_folded_into_the_write_us": None if folded is None else round(folded, 2),
            "gather_pool_us_by_frame": {str(k): round(v, 2) for k, v in per_frame.items()},
            "dirty_rows_this_frame": n_dirty, "memory_cells": n_cells,
            "memory_write_a16_a19": write, "unprojection_a1_a2": unproj,
            "note": "HIP events around %d back-to-back launches of each kernel on one stream, after the timed region (median of %d "
                    "batches, / %d).  `achieved` / `frac` use SURVEY 8(d)'s byte formula with U = the cells this frame touches; "
                    "by_definition also gives the reference algorithm's bytes (U = N: its full-map clone + divide + cast of every "
                    "frame, which this build does not perform) and the PMC counter traffic of the same three kernels over the same "
                    "time.  At this size the class is three launch-latency-sized kernels, not a bandwidth problem"
                    % (batch, reps // 3 - 2, batch)}


def log(msg):
    print(f"[bench {time.strftime('%H:%M:%S')}] {msg}", file=sys.stderr, flush=True)


def instances_arrays(inst, n_px: int, prefix: str = "") -> dict:
    """One frame's Instances, as its caller receives them, as host float arrays: pred_boxes [D, 4], scores [D], pred_classes [D].
    pred_masks (bool [D, H, W]: 491 MB as floats at 300 detections of 640x640) is stored as pred_masks_sample [D, n_px], every
    mask at the same n_px pixel positions (flattened y * W + x, ascending) drawn without replacement by
    np.random.default_rng(0), and pred_masks_area [D], the pixel count of every whole mask."""
    H, W = inst.image_size
    m = inst.pred_masks.reshape(len(inst), H * W)
    pos = np.sort(np.random.default_rng(0).choice(H * W, size=min(n_px, H * W), replace=False))
    return {prefix + "pred_boxes": inst.pred_boxes.tensor.float().cpu().numpy(),
            prefix + "scores": inst.scores.float().cpu().numpy(),
            prefix + "pred_classes": inst.pred_classes.float().cpu().numpy(),
            prefix + "pred_masks_sample": m[:, torch.from_numpy(pos).to(m.device)].float().cpu().numpy(),
            prefix + "pred_masks_area": m.sum(dim=1).double().cpu().numpy()}


def write_dump(out_dir: str, arrays: dict) -> None:
    total = sum(a.nbytes for a in arrays.values())
    if total > DUMP_LIMIT_BYTES:
        raise RuntimeError(f"--dump-outputs: {total} bytes of outputs, the limit is {DUMP_LIMIT_BYTES}")
    os.makedirs(out_dir, exist_ok=True)
    for name, a in arrays.items():
        assert a.dtype in (np.float32, np.float64), (name, a.dtype)
        np.save(os.path.join(out_dir, name + ".npy"), a)
    log(f"--dump-outputs: {len(arrays)} arrays, {total} bytes -> {out_dir}")


def cpu_baseline(sd, frames, args, budget_s):
    """The CPU oracle (a port: the reference's own CPU mode cannot run) timed on the host cores, SURVEY §8(d)
    protocol scaled to a bounded sample: warm-up frame(s) first (not timed: the first frame has an empty memory and cold
    allocators), then timed frames of the same recurrent sequence until `--cpu-frames` frames or the `--cpu-budget-s` budget,
    MEDIAN ms/frame -> frames/s, and the per-stage breakdown (mean seconds per timed frame)."""
    from oracle import memory as OM
    from oracle import model as M
    torch.set_num_threads(available_cores())
    log(f'cpu baseline on {torch.get_num_threads()} threads')
    ocfg = M.OracleCfg(memory_cls_score_thresh=args.memory_thresh, map_feature_weight=5.0)
    oracle = OM.RecurrentOracle(sd, ocfg)
    n_warm = max(1, min(args.cpu_warmup, len(frames) - 1))
    t0 = time.perf_counter()
    times = []
    for i, f in enumerate(frames):
        if i == n_warm:
            oracle.timings = {}
        t = time.perf_counter()
        oracle.step(f, i, frames)
        dt = time.perf_counter() - t
        log(f'cpu baseline frame {i}{" (warm-up)" if i < n_warm else ""}: {dt:.1f} s')
        if i >= n_warm:
            times.append(dt)
        if len(times) >= args.cpu_frames or (times and time.perf_counter() - t0 > budget_s):
            break
    n = len(times)
    med = float(np.median(times))
    stages = {k: round(v / n, 3) for k, v in (oracle.timings or {}).items()}
    model_name = ""
    try:
        with open("/proc/cpuinfo") as fh:
            for line in fh:
                if line.startswith("model name"):
                    model_name = line.split(":", 1)[1].strip()
                    break
    except OSError:
        pass
    return {"value": round(1.0 / med, 5), "unit": "frames/s", "cores": torch.get_num_threads(), "kind": "port",
            "sample": f"{n} consecutive timed frame(s) of the same synthetic recurrent sequence after {n_warm} warm-up frame(s), "
                      f"median {med * 1e3:.0f} ms/frame (min {min(times) * 1e3:.0f}, max {max(times) * 1e3:.0f}); oracle/ torch fp32; "
                      f"stopped by {'the frame count' if n >= args.cpu_frames else f'the {budget_s:.0f} s budget'} "
                      f"(SURVEY 8d's protocol: 5 warm-up + >= 20 timed frames)",
            "median_ms_per_frame": round(med * 1e3, 1), "timed_frames": n, "warmup_frames": n_warm,
            "per_stage_s_per_frame": stages, "cpu_model": model_name,
            "cores_note": f"{torch.get_num_threads()} threads = this job's CPU share (affinity / cgroup quota, capped at 32) of the "
                          f"host's {os.cpu_count()} logical cores"}


def relaunch_under_torchrun(args) -> int:
    """`python bench.py --gpus N` (N > 1) without a launcher: start N fresh one-GPU worker processes through
    `torch.distributed.run` BEFORE this process has touched the GPU, and return their exit code.  Refuses (non-zero) when the
    node does not have N devices -- never silently runs one rank and reports n_gpus: 1."""
    import socket
    import subprocess
    n_dev = torch.cuda.device_count()          # counting devices does not initialise the GPU
    if n_dev < args.gpus and os.environ.get("EOD_BENCH_ONE_DEVICE") != "1":
        print(f"[bench] --gpus {args.gpus} requested but only {n_dev} device(s) are visible", file=sys.stderr)
        return 2
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    log("no RANK in the environment: launching " + " ".join(cmd))
    return subprocess.call(cmd)


def run_batched(H, W, map_w, map_h, cell, B, warmup, steps, lockstep="launches", memory_thresh=0.3, concurrent_scenes=0, sd=None,
                dump_outputs=None) -> dict:
    """configs[4]: B sequences per GPU in lock-step, a step = B frames through the boundary -> the line's fields (single rank)."""
    from embodied_object_detection_amd import setup_cfg
    from embodied_object_detection_amd.checkpoint import synthetic_state_dict
    from embodied_object_detection_amd.data.synthetic import SyntheticSequence
    from embodied_object_detection_amd.modeling.batched import BatchedSequences
    torch.cuda.set_device(0)
    dev = torch.device("cuda:0")
    cfg = setup_cfg(None, ["MODEL.MEMORY_TYPE", "implicit_memory", "MODEL.MAP_FEAT_FUSION", "sum", "MODEL.MAP_FEATURE_WEIGHT", 5,
                           "MODEL.MEMORY_CLS_SCORE_THRESH", memory_thresh, "MODEL.DEVICE", "cuda:0"])
    sd = sd if sd is not None else synthetic_state_dict(0)
    if lockstep == "launches":
        from embodied_object_detection_amd.modeling.lockstep import LockstepScenes
        model = LockstepScenes(cfg, B, sd)
        how = (f"N = {B} through every stage of the frame: one launch per stage for all scenes (trunk, memory read, tower, proposal "
               f"decoding, cascade, selections, both mask passes over the concatenated ROI lists, memory write of the {B} states, paste)")
    else:
        model = BatchedSequences(cfg, B, sd, concurrent_scenes=concurrent_scenes)
        how = (f"the memory-independent trunk + FPN top-down run once per step with N = {B}, the scenes continue on their own streams "
               f"({len(set(id(s_) for s_ in model.streams))} in flight)")
    n = warmup + steps
    eps = []
    for b in range(B):
        seq = SyntheticSequence(100 + b, H=H, W=W, n_frames=n, map_w=map_w, map_h=map_h, cell=cell)
        fr = []
        for i in range(n):
            f = seq.frame(i)
            f["image"] = f["image"].to(dev)
            f["proj_indices"] = torch.from_numpy(f["proj_indices"][..., 0]).to(dev)
            fr.append(f)
        eps.append(fr)
    torch.cuda.synchronize()
    log(f"{B} x {n} frames of {H}x{W} resident")
    model([e[:warmup] for e in eps])
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    outs = model([e[warmup:] for e in eps])
    torch.cuda.synchronize()
    el = time.perf_counter() - t0
    nd = float(np.mean([len(o["instances"]) for ob in outs for o in ob]))
    if dump_outputs:         # the last timed step = the last frame of each of the B scenes
        arrays = {}
        for b, ob in enumerate(outs):
            arrays.update(instances_arrays(ob[-1]["instances"], DUMP_MASK_PIXELS // B, prefix=f"scene{b}_"))
        write_dump(dump_outputs, arrays)
    del model, eps, outs
    torch.cuda.empty_cache()
    return {
        "metric": f"frames/sec ({H}x{W}, implicit_memory, {B} sequences batched per GPU)", "value": round(steps * B / el, 3),
        "unit": "frames/s", "n_gpus": 1, "steps": steps, "warmup": warmup, "ms_per_step": round(el / steps * 1e3, 3),
        "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "f32", "data": "synthetic",
        "config": {"workload": f"BASELINE.json configs[4]: {B} independent sequences in lock-step per GPU, {H}x{W}, memory grid "
                               f"{map_w}x{map_h} @ {cell} m; a step = {B} frames through the boundary (Instances materialised); "
                               + how, "batch": B, "lockstep": lockstep, "detections_per_frame_mean": round(nd, 1)}}


def bench_batched(args):
    H, W = args.size
    map_w, map_h = args.grid
    print(json.dumps(run_batched(H, W, map_w, map_h, args.cell, args.batch, args.warmup, args.steps, args.lockstep, args.memory_thresh,
                                 args.concurrent_scenes, dump_outputs=args.dump_outputs)), flush=True)


def config5_variant(sd, memory_thresh: float) -> dict:
    """BASELINE.json configs[4] at full size inside the default run: 4 sequences in lock-step at 960x960 with a 512x512 memory grid
    (N = 262 144 cells), and the HBM-bound class (memory read + fusion) measured on a single 960x960 scene, where
    the full-map byte count is 581 MB and the class is no longer launch-sized."""
    from embodied_object_detection_amd import build_model, setup_cfg
    from embodied_object_detection_amd.data.synthetic import SyntheticSequence
    H = W = 960
    map_w = map_h = 512
    cell = 0.08
    line = run_batched(H, W, map_w, map_h, cell, 4, warmup=4, steps=12, sd=sd, memory_thresh=memory_thresh)
    out = {"value": line["value"], "unit": "frames/s", "ms_per_step": line["ms_per_step"], "steps": line["steps"], "warmup": line["warmup"],
           "batch": 4, "detections_per_frame_mean": line["config"]["detections_per_frame_mean"],
           "note": "BASELINE.json configs[4]: LockstepScenes(cfg, 4) at 960x960, memory grid 512x512 @ 0.08 m; a step = 4 frames through "
                   "the boundary (Instances materialised), N = 4 through every stage; `python bench.py --size 960 960 --grid 512 512 "
                   "--cell 0.08 --batch 4` is the same measurement as its own line"}
    try:
        dev = torch.device("cuda:0")
        cfg = setup_cfg(None, ["MODEL.MEMORY_TYPE", "implicit_memory", "MODEL.MAP_FEAT_FUSION", "sum", "MODEL.MAP_FEATURE_WEIGHT", 5,
                               "MODEL.MEMORY_CLS_SCORE_THRESH", memory_thresh, "MODEL.DEVICE", "cuda:0"])
        model = build_model(cfg, sd)
        seq = SyntheticSequence(7, H=H, W=W, n_frames=10, map_w=map_w, map_h=map_h, cell=cell)
        frames = []
        for i in range(10):
            f = seq.frame(i)
            f["image"] = f["image"].to(dev)
            f["proj_indices"] = torch.from_numpy(f["proj_indices"][..., 0]).to(dev)
            frames.append(f)
        model([frames[:6]])
        t0 = time.perf_counter()
        model([frames[:6]])
        torch.cuda.synchronize()
        out["single_sequence_frames_per_s"] = round(6 / (time.perf_counter() - t0), 2)
        probe = hbm_class_probe(model, frames, 7, H, W, seq.n_cells, reps=15, gather_frames=[6, 8])
        out["roofline_hbm"] = {k: probe[k] for k in ("bound", "class", "kernels", "achieved", "peak", "unit", "frac", "algorithmic_bytes",
                                                     "avg_us_total", "by_definition", "dirty_rows_this_frame", "memory_cells",
                                                     "memory_write_a16_a19")}
        del model, frames
        torch.cuda.empty_cache()
    except Exception as e:      # diagnostics only
        log(f"config5 hbm probe failed: {e!r}")
    return out


def train_step_variant(sd, freeze_backbone: bool = False) -> dict:
    """One training iteration of `forward_model` (custom_rcnn.py:584-679 + the optimizer step, train_mp3d.py:609-633) at 640x640:
    `Trainer.step` on one frame with 24 ground-truth boxes -- both halves forward and backward, train-mode proposals at the yaml's
    4000 / 2000, 512 sampled ROI rows per cascade stage, AdamW over all 126 parameter tensors.  FLOPs: 2 x MAC of every conv / linear
    layer forward, twice that again for the backward (input gradient + weight gradient)."""
    from embodied_object_detection_amd import build_model, setup_cfg
    from embodied_object_detection_amd.modeling.training import Trainer
    H = W = 640
    dev = torch.device("cuda:0")
    opts = ["MODEL.MEMORY_TYPE", "implicit_memory", "MODEL.MAP_FEAT_FUSION", "sum", "MODEL.MAP_FEATURE_WEIGHT", 5, "MODEL.DEVICE", "cuda:0",
            "FP16", False]
    if freeze_backbone:      # the shipped fine-tuning yaml's list (Detic_..._mp3d_recurrent.yaml:18-19)
        opts += ["MODEL.FREEZE_BACKBONE", True, "MODEL.UNFROZEN_LAYERS", ["roi", "map_merge", "proposal_generator"]]
    cfg = setup_cfg(None, opts)
    sd = {k: v.clone() for k, v in sd.items()}
    model = build_model(cfg, sd)
    trainer = Trainer(model, sd)
    g = torch.Generator().manual_seed(0)
    n_cells = 200 * 200
    img = torch.randint(0, 256, (3, H, W), generator=g, dtype=torch.uint8).to(dev)
    mem16 = (torch.randn((n_cells, 512), generator=g) * 2).half().to(dev)
    proj = torch.randint(0, n_cells, (H, W), generator=g).int().to(dev)
    xy = torch.rand((24, 2), generator=g) * torch.tensor([W * 0.6, H * 0.6])
    wh = torch.rand((24, 2), generator=g) * torch.tensor([W * 0.35, H * 0.35]) + 8
    gt = torch.cat([xy, xy + wh], dim=1).to(dev)
    kw = dict(gt_classes=torch.randint(0, 20, (24,), generator=g).int().to(dev), generator=torch.Generator(device=dev).manual_seed(0))
    torch.cuda.empty_cache()
    warm, steps = 4, 10
    first = None
    for _ in range(warm):
        out = trainer.step(img, gt, memory=(mem16, proj), **kw)
        first = first if first is not None else sum(float(v) for v in out.values())
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        out = trainer.step(img, gt, memory=(mem16, proj), **kw)
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / steps
    last = sum(float(v) for v in out.values())
    per_iter = []
    for _ in range(4):                                          # diagnostics: one iteration at a time, synchronised
        t1 = time.perf_counter()
        trainer.step(img, gt, memory=(mem16, proj), **kw)
        torch.cuda.synchronize()
        per_iter.append(round((time.perf_counter() - t1) * 1e3, 2))
    rows = [int(r["boxes"].shape[0]) for r in trainer.fm.det.last]
    fr = frame_roofline(H, W, float(np.mean(rows)), 0.0, 1.0, "fp32", n_mask_rois=0.0)["by_stage_gflop"]
    fwd = sum(fr.values())
    res = {"value": round(1.0 / dt, 3), "unit": "training iterations/s", "ms_per_step": round(dt * 1e3, 2), "steps": steps, "warmup": warm,
           "dtype": "f32", "proposals": int(trainer.fm.last_proposals.shape[0]), "proposal_list_sizes": [trainer.fm.pre, trainer.fm.post],
           "roi_rows_per_stage": rows, "gt_boxes": 24, "forward_gflop": round(fwd, 1), "algorithmic_gflop_per_iteration": round(3 * fwd, 1),
           "achieved_tflops": round(3 * fwd / dt / 1e3, 2), "frac_of_fp32_mfma_peak": round(3 * fwd / dt / 1e3 / PEAK_F32_MFMA_TFLOPS, 4),
           "total_loss_first_last": [round(first, 4), round(last, 4)], "synchronised_iterations_ms": per_iter,
           "stepped_tensors": len(trainer.groups),
           "note": "Trainer.step: forward_model forward + backward + AdamW on one 640x640 frame, parameters stepped in the "
                   "layers the inference path runs; FP16: False (the yaml's autocast / GradScaler path is refused, not emulated)"}
    if freeze_backbone:
        # the trunk half's backward is not run: forward of everything + backward of the heads only
        res["note"] += ("; MODEL.FREEZE_BACKBONE True, UNFROZEN_LAYERS ['roi', 'map_merge', 'proposal_generator']: nobody reads the trunk "
                        "half's gradients, its backward is skipped (the GFLOP fields count the full backward and do not apply)")
        for k in ("algorithmic_gflop_per_iteration", "achieved_tflops", "frac_of_fp32_mfma_peak"):
            res.pop(k)
    del trainer, model
    torch.cuda.empty_cache()
    return res


def main():
    args = parse()
    if args.batch > 1:
        if args.gpus != 1:
            print("[bench] --batch is a single-GPU line", file=sys.stderr)
            sys.exit(2)
        return bench_batched(args)
    if args.gpus > 1 and "RANK" not in os.environ:
        sys.exit(relaunch_under_torchrun(args))
    rank = int(os.environ.get("RANK", 0))
    local_rank = int(os.environ.get("LOCAL_RANK", 0))
    world = int(os.environ.get("WORLD_SIZE", 1))
    distributed = world > 1
    if args.gpus != world:
        print(f"[bench] --gpus {args.gpus} != WORLD_SIZE {world}: refusing to report a mislabelled run", file=sys.stderr)
        sys.exit(2)
    # rehearsal knobs for a one-GPU box: EOD_BENCH_ONE_DEVICE=1 puts every rank on cuda:0, EOD_BENCH_BACKEND=gloo replaces RCCL
    # (RCCL refuses two ranks on one device).  The driver's real runs use neither.
    if os.environ.get("EOD_BENCH_ONE_DEVICE") == "1":
        local_rank = 0
    backend = os.environ.get("EOD_BENCH_BACKEND", "nccl")
    torch.cuda.set_device(local_rank)
    dev = torch.device(f"cuda:{local_rank}")
    if distributed:
        import torch.distributed as dist
        if backend == "nccl":
            dist.init_process_group(backend="nccl", device_id=dev)
        else:
            dist.init_process_group(backend=backend)

    from embodied_object_detection_amd import build_model, ops, setup_cfg
    from embodied_object_detection_amd.checkpoint import synthetic_state_dict
    from embodied_object_detection_amd.data.synthetic import SyntheticSequence
    from embodied_object_detection_amd.engine.eval_loop import (KIND_DET, KIND_GT, RecordBuffer, evaluate_gathered, gather_records,
                                                                 gt_to_coco_xyxy)

    H, W = args.size
    map_w, map_h = args.grid
    cfg = setup_cfg(None, ["MODEL.MEMORY_TYPE", "implicit_memory", "MODEL.MAP_FEAT_FUSION", "sum", "MODEL.MAP_FEATURE_WEIGHT", 5,
                           "MODEL.MEMORY_CLS_SCORE_THRESH", args.memory_thresh, "MODEL.DEVICE", f"cuda:{local_rank}"])
    sd = synthetic_state_dict(0)
    model = build_model(cfg, sd)
    log('model built')

    headline_math = ops.get_conv_math()          # "fp32" unless EOD_CONV_MATH=bf16x3 is exported
    # one frame more than is processed: in the enqueue-only variant the model starts the NEXT frame's memory-independent
    # bottom-up pass during a step, so the last timed step needs a next frame for the region to hold exactly `steps` trunks
    # (the look-ahead window reaches up to four frames beyond the current one: with four spare frames its fill is the same at
    # both ends of the timed region, which then holds the trunks of exactly `steps` frames)
    n_proc = args.steps + args.warmup
    n_frames = n_proc + 4
    seq = SyntheticSequence(rank, H=H, W=W, n_frames=n_frames, map_w=map_w, map_h=map_h, cell=args.cell,
                            projector=None)
    host_frames = [seq.frame(i) for i in range(n_frames)]
    # inputs resident in HBM before the timed region
    frames = []
    for f in host_frames:
        g = dict(f)
        g["image"] = f["image"].to(dev)
        g["proj_indices"] = torch.from_numpy(f["proj_indices"][..., 0]).to(dev)
        frames.append(g)
    torch.cuda.synchronize()
    log(f'{n_frames} frames resident on device')

    # dominant-kernel instrumentation: events around every mask-head 3x3 conv launch (fp32 MFMA implicit GEMM)
    ev = []

    def barrier():
        if distributed:
            dist.barrier()

    def run_boundary(fr, lo, hi, keep_last=None):
        """The reference's call shape (train_mp3d.py:186): `model([episode])` with episodes of 20 frames, `Instances`
        (boxes, scores, classes, bool masks) materialised for every frame.  `keep_last`: a list that receives the last frame's."""
        n = 0
        for e0 in range(lo, hi, EPISODE_LEN):
            outs = model([fr[e0:min(hi, e0 + EPISODE_LEN)]])
            n += len(outs)
            assert all(o["instances"].pred_masks.dtype == torch.bool for o in outs)
            if keep_last is not None:
                keep_last[:] = [outs[-1]["instances"]]
        return n

    def run_enqueue(fr, lo, hi):
        """Round-1 headline form: frames enqueued back to back, results left in the device buffers (no Instances)."""
        for i in range(lo, hi):
            if fr[i]["memory_reset"]:
                model.reset_memory(seq.n_cells)      # custom_rcnn.py:470-479
            model.inference_frame(fr[i], refresh_memory_snapshot=True, materialize=False,
                                  next_frame=fr[i + 1:i + 5] or None)          # the look-ahead window sees the frames that follow
        return hi - lo

    def timed_pass(run, fr, what):
        """W untimed + exactly K timed steps, barrier + synchronize on both sides, MAX over ranks."""
        run(fr, 0, args.warmup)
        torch.cuda.synchronize()
        barrier()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        n = run(fr, args.warmup, args.warmup + args.steps)
        host = time.perf_counter() - t0
        torch.cuda.synchronize()
        barrier()
        torch.cuda.synchronize()
        el = time.perf_counter() - t0
        assert n == args.steps
        if distributed:
            t = torch.tensor([el], dtype=torch.float64, device=dev)
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            el = float(t.item())
        hp = model.host_profile
        fr = max(hp["frames"], 1)
        log(f'{what}: {el:.3f} s for {args.steps} frames ({args.steps * world / el:.1f} frames/s), host side {host / args.steps * 1e3:.2f} ms/frame'
            f' [forward(): enqueue {hp["enqueue_s"] / fr * 1e3:.2f}, materialise {hp["materialize_s"] / fr * 1e3:.2f} of which waiting '
            f'{hp["wait_s"] / fr * 1e3:.2f} ms/frame]')
        for k_ in hp:
            hp[k_] = 0
        return el

    def as_variant(el, note, **extra):
        v = {"value": round(args.steps * world / el, 3), "unit": "frames/s", "ms_per_step": round(el / args.steps * 1e3, 3)}
        v.update(extra)
        v["note"] = note
        return v

    # ---- headline: through the boundary, inputs resident in HBM -------------------------------------------------------------
    # The timed region carries NO device-side instrumentation launches: HIP events around the mask-conv launches only (tagged
    # (pass, frame) on the host); the frames' counters come from an untimed replay of the same frames below.  A plain run records
    # the same events and only --full reads them: the timed region is the same launches, event records included, in both.
    if not args.no_kernel_events:
        for conv in model.roi_heads.mask_convs:
            conv.event_log = ev
    model.stats_log = None
    run_boundary(frames, 0, min(args.warmup, 4))       # allocator / clocks
    torch.cuda.synchronize()
    ev.clear()
    # the events of the warm-up frames are dropped inside timed_pass's caller below: remember where the timed ones start
    ev_mark = []

    last_timed = []         # --dump-outputs: the Instances of the last timed step

    def run_boundary_marked(fr, lo, hi):
        if lo == args.warmup:
            ev_mark.append(len(ev))
            return run_boundary(fr, lo, hi, keep_last=last_timed if args.dump_outputs else None)
        return run_boundary(fr, lo, hi)

    elapsed = timed_pass(run_boundary_marked, frames, "boundary, resident inputs")
    if args.dump_outputs:
        write_dump(args.dump_outputs, instances_arrays(last_timed.pop(), DUMP_MASK_PIXELS, prefix=f"rank{rank}_" if distributed else ""))
    ev = ev[ev_mark[0]:] if ev_mark else ev
    for conv in model.roi_heads.mask_convs:
        conv.event_log = None

    lazy = bool(model.lazy_proposal_masks)
    dedup = bool(model.dedup_detection_masks)
    total_frames = args.steps * world

    def headline_line(mask_counts, frame_counts):
        """The result line of a plain run; --full passes the per-frame means of its replay's counters and adds its own keys."""
        return {
            "metric": "frames/sec (640x640, implicit_memory); frames/sec/GPU = value / n_gpus",
            "value": round(total_frames / elapsed, 3), "unit": "frames/s", "n_gpus": world, "steps": args.steps,
            "warmup": args.warmup, "ms_per_step": round(elapsed / args.steps * 1e3, 3), "higher_is_better": True,
            "scaling": "weak", "vs_baseline": None,
            "dtype": "f32" if headline_math == "fp32" else "f32 emulated as 3 x bf16 on the bf16 MFMA pipe, fp32 accumulate", "data": "synthetic",
            "config": {"workload": f"recurrent per-frame inference, MEMORY_TYPE implicit_memory, MAP_FEAT_FUSION sum, "
                                   f"{H}x{W} synthetic sequence, memory grid {map_w}x{map_h} @ {args.cell} m, one scene per GPU "
                                   f"(BASELINE.json configs[2]/[3]); proposal masks "
                                   + ("computed only for the <=100 proposals the memory update reads (outputs bitwise identical to the "
                                      "reference's 256-proposal pass, reported by --full as variants.all_256_proposal_masks)" if lazy else
                                      "computed for all 256 proposals as the reference does")
                                   + ("; detection masks computed once per distinct class-agnostic box (detections of one proposal share "
                                      "it; bitwise identical to one ROI per detection, reported by --full as variants.one_mask_roi_per_detection)"
                                      if dedup else "; one mask-head ROI per detection"),
                       **mask_counts,
                       "image": f"{H}x{W}", "memory_cells": map_w * map_h, "weights": "random-init (synthetic_state_dict seed 0)",
                       "memory_cls_score_thresh": args.memory_thresh,
                       "schedule": ("five HIP streams per scene inside model([episode]): main chain (memory read + fusion, tower, proposal "
                                    "decoding, proposal masks), side (box cascade, detection and memory selection, memory write), "
                                    "look-ahead (the next frame's memory-independent ResNet trunk), detection (detection mask pass + "
                                    "post-process + paste, may trail under the next frame), caller; Instances are sliced out two frames "
                                    "behind the enqueue; every step does one frame's full work, results bitwise equal to one stream"
                                    if model.overlap_branches else "one HIP stream"),
                       **frame_counts},
            "boundary": "model([episode of <=20 frame dicts]) -> [{'instances': Instances(pred_boxes, scores, pred_classes i64, "
                        "pred_masks bool [D,H,W])}] per frame (train_mp3d.py:186, custom_rcnn.py:537-546); inputs resident in HBM",
            "full": args.full,
        }

    if not args.full:
        if rank == 0:
            print(json.dumps(headline_line({}, {})), flush=True)
        if distributed:
            dist.barrier()
            dist.destroy_process_group()
        return

    # ---- --full: everything below is beside the headline --------------------------------------------------------------------------
    # replay (untimed): the same frames from the same reset state give the same counters (every kernel is deterministic)
    run_boundary(frames, 0, args.warmup)
    model.stats_log = []
    run_boundary(frames, args.warmup, args.warmup + args.steps)
    torch.cuda.synchronize()
    counts = model.stats_log or []
    model.stats_log = None
    assert len(counts) == args.steps, (len(counts), args.steps)

    # ---- the dominant kernel without a concurrent stream (short extra pass, not part of `value`) --------------------------------
    ev_excl = []
    excl_counts = []
    if ev and model.overlap_branches:
        model.overlap_branches = False
        run_enqueue(frames, 0, min(args.warmup, 2))
        for conv in model.roi_heads.mask_convs:
            conv.event_log = ev_excl
        model.stats_log = []
        run_enqueue(frames, args.warmup, min(n_proc, args.warmup + 8))
        torch.cuda.synchronize()
        excl_counts = model.stats_log
        model.stats_log = None
        for conv in model.roi_heads.mask_convs:
            conv.event_log = None
        model.overlap_branches = True

    # ---- siblings and variants (reported beside, never as `value`) ----------------------------------------------------------------
    variants = {}
    boundary_host = None
    if args.variants:
        tv = timed_pass(run_boundary, host_frames, "boundary, host inputs")
        boundary_host = as_variant(tv, "same call, but every frame dict carries HOST buffers as the reference's loader hands them over "
                                       "(u8 CHW torch tensor, np.int32 [H,W,1] proj_indices, pageable memory): PCIe-inclusive rate")
        tv = timed_pass(run_enqueue, frames, "enqueue only")
        variants["enqueue_only"] = as_variant(tv, "round-1 headline form: model.inference_frame(materialize=False) back to back, next "
                                                  "frame hinted across the whole run, results left in device buffers (no Instances, "
                                                  "no per-frame host wait)")

        model.lazy_proposal_masks = False
        tv = timed_pass(run_boundary, frames, "reference-faithful proposal masks")
        variants["all_256_proposal_masks"] = as_variant(tv, "reference-faithful work: the mask head also runs on the proposals whose "
                                                            "masks nothing reads (custom_rcnn.py:573 computes all 256, :875-880 reads "
                                                            "<= 100); outputs bitwise identical to the headline")
        model.lazy_proposal_masks = True

        model.dedup_detection_masks = False
        tv = timed_pass(run_boundary, frames, "one mask-head ROI per detection")
        variants["one_mask_roi_per_detection"] = as_variant(tv, "reference-faithful work on the detection side: the mask head runs on every "
                                                                "one of the <=300 detections although detections of one proposal share "
                                                                "one class-agnostic box and hence one mask (detic_roi_heads.py:214-221,257); "
                                                                "outputs bitwise identical to the headline")
        model.lazy_proposal_masks = False
        tv = timed_pass(run_boundary, frames, "reference-faithful mask work (256 proposals + every detection)")
        variants["reference_faithful_mask_work"] = as_variant(tv, "both of the above: 256 proposal masks + one ROI per detection, the mask "
                                                                  "head's work exactly as the reference issues it; outputs bitwise identical")
        model.lazy_proposal_masks = True
        model.dedup_detection_masks = True

        # the same frame with the two mask passes one after the other (the detection pass may start only when the proposal masks
        # are done): the dominant kernel's launches then share the chip with the look-ahead trunk only -- what its in-frame
        # fraction is when the schedule does not overlap it with itself
        if not args.no_kernel_events:
            ev3, mark3 = [], []
            for conv in model.roi_heads.mask_convs:
                conv.event_log = ev3
            model.detection_pass_after = "proposal_masks"

            def run_seq(fr, lo, hi):
                if lo == args.warmup:
                    mark3.append(len(ev3))
                return run_boundary(fr, lo, hi)

            tv = timed_pass(run_seq, frames, "mask passes one after the other")
            model.detection_pass_after = "cascade"
            for conv in model.roi_heads.mask_convs:
                conv.event_log = None
            ev3 = ev3[mark3[0]:] if mark3 else ev3
            v = as_variant(tv, "detection_pass_after = 'proposal_masks': the detection mask pass waits for the proposal-mask pass instead of "
                               "running beside it; bitwise the same results (tests/test_model_gpu.py)")
            if ev3:
                order3 = {f: i for i, f in enumerate(sorted({t[1] for (_s, _e, t) in ev3}))}
                fl3 = [2.0 * int(counts[min(order3[t[1]], len(counts) - 1)][4 if t[0] == "det" else 3].item()) * 196 * 256 * 2304
                       for (_s, _e, t) in ev3]
                d3 = [s_.elapsed_time(e_) for (s_, e_, _c) in ev3]
                a3 = sum(fl3) / (sum(d3) * 1e-3) / 1e12
                v["mask_conv"] = {"achieved_tflops": round(a3, 3), "frac_of_fp32_mfma_peak": round(a3 / PEAK_F32_MFMA_TFLOPS, 4),
                                  "avg_launch_ms": round(sum(d3) / len(d3), 4), "launches": len(d3)}
            variants["mask_passes_one_after_the_other"] = v

        # worst-case memory write path: MEMORY_CLS_SCORE_THRESH 0.0 keeps up to 100 memory instances per frame
        thr0 = model.cls_score_thresh
        model.cls_score_thresh = 0.0
        model.stats_log = []
        tv = timed_pass(run_boundary, frames, "memory thresh 0")
        ks = [int(c[2].item()) for c in model.stats_log[-args.steps:]]
        model.stats_log = None
        model.cls_score_thresh = thr0
        variants["memory_cls_score_thresh_0"] = as_variant(tv, "MODEL.MEMORY_CLS_SCORE_THRESH 0.0: worst-case memory write path",
                                                           memory_instances_per_frame_mean=round(float(np.mean(ks)), 1))

        # fp32 emulated on the bf16 matrix cores (three-way operand split, six MFMAs per term set, fp32 accumulate): same
        # parity tests, 16/6 of the fp32-MFMA arithmetic ceiling.  Opt-in (EOD_CONV_MATH=bf16x3 / ops.set_conv_math).
        if ops.get_conv_math() == "fp32":
            prev_math = ops.set_conv_math("bf16x3")
            ev2 = []
            if not args.no_kernel_events:
                for conv in model.roi_heads.mask_convs:
                    conv.event_log = ev2
            mark2 = []

            def run_b3(fr, lo, hi):
                if lo == args.warmup:
                    mark2.append(len(ev2))
                return run_boundary(fr, lo, hi)

            tv = timed_pass(run_b3, frames, "bf16x3")
            ev2 = ev2[mark2[0]:] if mark2 else ev2
            for conv in model.roi_heads.mask_convs:
                conv.event_log = None
            ops.set_conv_math(prev_math)
            v = as_variant(tv, "every eligible conv/linear on the bf16 MFMA pipe with fp32 operands split into three bf16 pieces "
                               "(6 MFMAs per K=16 step, fp32 accumulate); passes the same parity tests; error vs an fp64 conv "
                               "within 2x of the fp32-MFMA kernel's (tests/test_kernels_gpu.py::test_conv_bf16x3_accuracy)")
            if ev2:
                durs = [s_.elapsed_time(e_) for (s_, e_, _c) in ev2]
                # same frames, same counters as the headline pass (the selection decisions agree in both arithmetic modes on this
                # sequence to within a few ROIs; the figure is an average over 8 x steps launches)
                order2 = {f: i for i, f in enumerate(sorted({t[1] for (_s, _e, t) in ev2}))}
                fl = [2.0 * int(counts[min(order2[t[1]], len(counts) - 1)][4 if t[0] == "det" else 3].item()) * 196 * 256 * 2304
                      for (_s, _e, t) in ev2]
                ach = sum(fl) / (sum(durs) * 1e-3) / 1e12
                v["mask_conv"] = {"kernel": "conv_bf16x3_w8_kernel (256x128 tile, 8 waves)", "achieved_fp32_equivalent_tflops": round(ach, 3),
                                  "avg_launch_ms": round(sum(durs) / len(durs), 4),
                                  "frac_of_bf16_dense_peak_algorithmic": round(ach / PEAK_BF16_MFMA_TFLOPS, 4),
                                  "frac_of_bf16_dense_peak_issued": round(6.0 * ach / PEAK_BF16_MFMA_TFLOPS, 4),
                                  "vs_fp32_mfma_peak": round(ach / PEAK_F32_MFMA_TFLOPS, 4)}
            variants["bf16x3_split_mfma"] = v

        # two independent sequences per GPU in lock-step (scenes are independent: `train_mp3d.py --scenes-in-lockstep 2`): the
        # latency-bound chains of one scene run beside the dense passes of the other
        if not distributed:
            from embodied_object_detection_amd.modeling.lockstep import LockstepScenes
            try:
                for nb, key in ((2, "two_sequences_in_lockstep"), (4, "four_sequences_in_lockstep")):
                    group = LockstepScenes(cfg, nb, sd)
                    eps = [frames[:n_proc]]
                    for extra in range(1, nb):
                        seq2 = SyntheticSequence(1000 * extra + rank, H=H, W=W, n_frames=n_proc, map_w=map_w, map_h=map_h, cell=args.cell)
                        fr2 = []
                        for i in range(n_proc):
                            f = seq2.frame(i)
                            f["image"] = f["image"].to(dev)
                            f["proj_indices"] = torch.from_numpy(f["proj_indices"][..., 0]).to(dev)
                            fr2.append(f)
                        eps.append(fr2)
                    part = args.steps // 2
                    cut = lambda lo, hi: [e[lo:hi] for e in eps]
                    for e0 in range(0, args.warmup, EPISODE_LEN):
                        group(cut(e0, min(args.warmup, e0 + EPISODE_LEN)))
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    n2 = 0
                    for e0 in range(args.warmup, args.warmup + part, EPISODE_LEN):
                        o2 = group(cut(e0, min(args.warmup + part, e0 + EPISODE_LEN)))
                        n2 += sum(len(o) for o in o2)
                    torch.cuda.synchronize()
                    el2 = time.perf_counter() - t0
                    log(f"{nb} sequences in lock-step: {el2:.3f} s for {n2} frames ({n2 / el2:.1f} frames/s)")
                    variants[key] = {
                        "value": round(n2 / el2, 3), "unit": "frames/s", "ms_per_step": round(el2 / max(n2, 1) * 1e3, 3),
                        "note": f"LockstepScenes(cfg, {nb}): {nb} independent scenes per GPU, {part} steps of {nb} frames, through the boundary "
                                f"(Instances materialised), episodes of 20; N = {nb} through every stage of the frame (one launch per stage "
                                "for all scenes), every scene keeps its own memory; per-scene results bitwise those of a single-scene run "
                                "(tests/test_fullsize_gpu.py)"}
                    del group, eps
                    torch.cuda.empty_cache()
            except Exception as e:      # never lose the headline to a variant
                log(f"lock-step variant failed: {e!r}")
            if (H, W) == (640, 640) and not args.no_config5:
                try:
                    variants["config5_960_batch4"] = config5_variant(sd, args.memory_thresh)
                    log(f"config5 960x960 batch of 4: {variants['config5_960_batch4']['value']} frames/s")
                except Exception as e:
                    log(f"config5 variant failed: {e!r}")
            if (H, W) == (640, 640) and not args.no_train_step:
                try:
                    variants["train_step_640"] = train_step_variant(sd)
                    log(f"training iteration at 640x640: {variants['train_step_640']['ms_per_step']} ms")
                    variants["train_step_640_frozen_backbone"] = train_step_variant(sd, freeze_backbone=True)
                    log(f"training iteration at 640x640, frozen backbone: {variants['train_step_640_frozen_backbone']['ms_per_step']} ms")
                except Exception as e:
                    log(f"train-step variant failed: {e!r}")

    roofline_hbm = None
    if rank == 0:
        try:
            spread = sorted({args.warmup + int(args.steps * q) for q in (0.1, 0.3, 0.5, 0.7, 0.9)})
            roofline_hbm = hbm_class_probe(model, frames, args.warmup + 2, H, W, seq.n_cells, gather_frames=spread)
            log(f"hbm class: {roofline_hbm['kernels']} -> {roofline_hbm['achieved']} GB/s ({roofline_hbm['frac']})")
        except Exception as e:      # never lose the headline to the probe
            log(f"hbm probe failed: {e!r}")

    # ---- detection records -> one all-reduce -> AP50 (the eval collective of the north star) --------------------
    rec = RecordBuffer(max_rows=4 * 108)
    for j, i in enumerate(range(args.warmup, n_proc)):
        if j % max(1, args.steps // 4) == 0 and j // max(1, args.steps // 4) < 4:
            inst = model.inference_frame(frames[i], refresh_memory_snapshot=True, materialize=True)["instances"]
            n = min(len(inst), 100)
            b, sc, cl = inst.pred_boxes.tensor[:n].cpu().numpy(), inst.scores[:n].cpu().numpy(), inst.pred_classes[:n].cpu().numpy()
            for q in range(n):
                rec.add([KIND_DET, rank, j, float(cl[q]), float(sc[q]), *b[q].tolist(), 0])
            gt = host_frames[i]["instances"]
            gb = gt_to_coco_xyxy(gt["gt_boxes"])
            for q, c in enumerate(gt["gt_classes"].tolist()):
                rec.add([KIND_GT, rank, j, float(c), 0.0, *gb[q].tolist(), 0])
    torch.cuda.synchronize()
    t_ar = time.perf_counter()
    buf = gather_records(rec, rank, world, dev)          # ONE all_reduce(SUM) over RCCL when world > 1
    t_ar = time.perf_counter() - t_ar
    ap = evaluate_gathered(buf, 20)["all"] if rank == 0 else None

    # ---- dominant kernel roofline ----------------------------------------------------------------------------------
    roofline = None
    if ev:
        # (start, end, (pass, frame)) recorded by ops.Conv around every mask_fcn launch of the timed region; the ROI count of a
        # launch = the frame's detection count ("det") or the proposals its memory update reads ("prop"), from the replay
        def rows_of(events, cnts):
            order = {f: i for i, f in enumerate(sorted({t[1] for (_s, _e, t) in events}))}
            out = []
            for (_s, _e, t) in events:
                c = cnts[min(order[t[1]], len(cnts) - 1)]
                out.append(int(c[4].item()) if t[0] == "det" else (int(c[3].item()) if t[0] == "prop" else int(c[0].item())))
            return out
        durs = [s.elapsed_time(e) for (s, e, _c) in ev]
        rows = rows_of(ev, counts)
        flops = [2.0 * r * 196 * 256 * 2304 for r in rows]
        tot_ms = sum(durs)
        b3 = headline_math == "bf16x3"
        peak = PEAK_BF16_MFMA_TFLOPS if b3 else PEAK_F32_MFMA_TFLOPS
        kname = ("conv_bf16x3_w8_kernel 256x128 (bf16 MFMA, 3-way operand split: 6 issued MFMA flops per algorithmic flop)" if b3
                 else "conv_igemm_kernel<64,64,BK=32>") + " (mask_fcn 3x3 implicit GEMM, M=rois*196, N=256, K=2304)"
        roofline = {"bound": "mfma", "kernel": kname,
                    "achieved": round(sum(flops) / (tot_ms * 1e-3) / 1e12, 3), "peak": peak, "unit": "TFLOP/s",
                    "frac": round(sum(flops) / (tot_ms * 1e-3) / 1e12 / peak, 4), "traffic": None if b3 else pmc_traffic(),
                    "launches": len(durs), "avg_launch_ms": round(tot_ms / len(durs), 4),
                    "algorithmic_flop_per_launch": round(sum(flops) / len(flops), 1),
                    "note": "events on the launch stream around every mask-conv launch of the timed region (detection pass and "
                            "proposal-mask pass, ROI counts in config): in the default schedule these launches run concurrently with each "
                            "other and with the look-ahead trunk, so a launch's duration includes sharing the chip; "
                            "exclusive_launches is the kernel with the chip to itself"}
        prof = None if b3 else _profile_json("dominant_kernel_rocprof")
        if prof:
            # committed `rocprofv3 --kernel-trace` of this same command, per grid shape: 3676 workgroups = the detection pass's
            # launch capacity (300 ROIs), 1568 = the proposal-mask pass's (128); the live events above must agree with their mean
            by_wg = {s_["workgroups"]: s_ for s_ in prof.get("shapes", [])}
            sel = [by_wg[w_] for w_ in (3676, 1568) if w_ in by_wg]
            if sel:
                n_ = sum(s_["launches"] for s_ in sel)
                tags_ = [t_[0] for (_s, _e, t_) in ev]
                mean_flop = {3676: [f_ for f_, g_ in zip(flops, tags_) if g_ == "det"], 1568: [f_ for f_, g_ in zip(flops, tags_) if g_ != "det"]}
                # this run's mean FLOPs per launch of each pass over the committed trace's mean kernel duration of that launch shape
                fl_ = sum((sum(mean_flop[s_["workgroups"]]) / max(1, len(mean_flop[s_["workgroups"]]))) * s_["launches"] for s_ in sel)
                us_ = sum(s_["avg_us"] * s_["launches"] for s_ in sel)
                roofline["rocprof"] = {"file": prof.get("_file"),
                                       "avg_launch_ms": round(us_ / n_ * 1e-3, 4),
                                       "achieved": round(fl_ / (us_ * 1e-6) / 1e12, 3), "frac": round(fl_ / (us_ * 1e-6) / 1e12 / peak, 4),
                                       "by_workgroups": {str(s_["workgroups"]): {"launches": s_["launches"], "avg_us": s_["avg_us"],
                                                                                 "min_us": s_["min_us"]} for s_ in sel},
                                       "note": "rocprofv3 --kernel-trace of this command: a kernel's duration from its first wave to its "
                                               "last; the event brackets above also contain the launch's wait for workgroup slots beside "
                                               "the other streams' kernels (the detection pass runs at normal priority under three "
                                               "high-priority chains), which is why they are ~15 % longer"}
        if ev_excl:
            d2 = [s_.elapsed_time(e_) for (s_, e_, _c) in ev_excl]
            f2 = [2.0 * r_ * 196 * 256 * 2304 for r_ in rows_of(ev_excl, excl_counts)]
            ach = sum(f2) / (sum(d2) * 1e-3) / 1e12
            by_pass = {}
            tags2 = [t_[0] for (_s, _e, t_) in ev_excl]
            for name, want in (("detection_pass", ("det",)), ("proposal_mask_pass", ("prop", "prop_all"))):
                dd = [t_ for t_, g_ in zip(d2, tags2) if g_ in want]
                ff = [f_ for f_, g_ in zip(f2, tags2) if g_ in want]
                if dd:
                    a_ = sum(ff) / (sum(dd) * 1e-3) / 1e12
                    by_pass[name] = {"launches": len(dd), "rois_mean": round(sum(ff) / len(ff) / (2.0 * 196 * 256 * 2304), 1),
                                     "avg_launch_ms": round(sum(dd) / len(dd), 4), "achieved": round(a_, 3), "frac": round(a_ / peak, 4)}
            roofline["exclusive_launches"] = {"achieved": round(ach, 3), "frac": round(ach / peak, 4), "launches": len(d2),
                                              "avg_launch_ms": round(sum(d2) / len(d2), 4), "by_pass": by_pass,
                                              "note": "same kernel, same inputs, measured in a short extra pass on ONE stream "
                                                      "(model.overlap_branches = False) after the timed region: in the timed "
                                                      "region every launch shares the chip with the second stream's box cascade / "
                                                      "memory write"}

    result = None
    if rank == 0:
        pc = [int(c[0].item()) for c in counts]
        dc = [int(c[1].item()) for c in counts]
        mk = [int(c[2].item()) for c in counts]
        uq = [int(c[3].item()) for c in counts]
        dm = [int(c[4].item()) for c in counts]
        result = headline_line(
            {"detection_mask_rois_per_frame_mean": round(float(np.mean(dm)), 1),
             "proposal_masks_per_frame_mean": round(float(np.mean(uq)), 1) if lazy else round(float(np.mean(pc)), 1)},
            {"proposals_per_frame_mean": round(float(np.mean(pc)), 1), "detections_per_frame_mean": round(float(np.mean(dc)), 1),
             "memory_instances_per_frame_mean": round(float(np.mean(mk)), 1)})
        result.update({
            "boundary_host_inputs": boundary_host,
            "roofline": roofline,
            "roofline_hbm": roofline_hbm,
            "frame_roofline": frame_roofline(H, W, float(np.mean(pc)), float(np.mean(dc)), elapsed / args.steps, headline_math,
                                             n_mask_rois=(float(np.mean(uq)) if lazy else float(np.mean(pc))) + float(np.mean(dm))),
            "variants": variants,
            "eval_allreduce_ms": round(t_ar * 1e3, 3),
            "ap50_synthetic": None if ap is None else round(ap["AP50"], 3),
        })
    if rank == 0 and world == 1 and not args.no_cpu_baseline:   # reported at N=1 only (bench contract)
        result["cpu_baseline"] = cpu_baseline(sd, host_frames[:args.cpu_warmup + args.cpu_frames], args, args.cpu_budget_s)
    if rank == 0:
        print(json.dumps(result), flush=True)
    if distributed:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
