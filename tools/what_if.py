#!/usr/bin/env python
"""What would the frame rate be if a piece of background work were free?  Same loop as tools/knob_ab.py (60 resident 640x640 frames
through the boundary), with the look-ahead trunk's launches removed after the warm-up episode (the pyramid sets keep the values an
earlier frame left in them: the rest of the frame works on a valid pyramid of another frame).  A diagnostic for DESIGN §9 (how much
of the frame's period is the trunk's), not a benchmark.

    python tools/what_if.py
"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from embodied_object_detection_amd import build_model, setup_cfg
from embodied_object_detection_amd.checkpoint import synthetic_state_dict
from embodied_object_detection_amd.data.synthetic import SyntheticSequence

dev = torch.device("cuda:0")
cfg = setup_cfg(None, ["MODEL.MEMORY_TYPE", "implicit_memory", "MODEL.MAP_FEAT_FUSION", "sum", "MODEL.MAP_FEATURE_WEIGHT", 5,
                       "MODEL.MEMORY_CLS_SCORE_THRESH", 0.3, "MODEL.DEVICE", "cuda:0"])
sd = synthetic_state_dict(0)
N = 60
seq = SyntheticSequence(0, H=640, W=640, n_frames=N, map_w=200, map_h=200, cell=0.2)
frames = []
for i in range(N):
    f = seq.frame(i)
    f["image"] = f["image"].to(dev)
    f["proj_indices"] = torch.from_numpy(f["proj_indices"][..., 0]).to(dev)
    frames.append(f)


def rate(model):
    out = []
    for _ in range(3):
        t = time.perf_counter()
        model([frames[20:40]])
        model([frames[40:60]])
        torch.cuda.synchronize()
        out.append(40 / (time.perf_counter() - t))
    return out


model = build_model(cfg, sd)
model([frames[:20]])
torch.cuda.synchronize()
print("as shipped                         ", " ".join(f"{v:6.1f}" for v in rate(model)), "frames/s")

bu, bb = model.backbone.bottom_up, model.backbone
real = (bu.forward, bb.top_down)
kept = {}


def fake_forward(x, Hp, Wp, N=1):
    key = (Hp, Wp, N)
    if key not in kept:
        kept[key] = real[0](x, Hp, Wp, N=N) if N != 1 else real[0](x, Hp, Wp)
    return kept[key]


tdb = {}


def fake_top_down(c, N=1, views=None, planned=False):
    if views is not None:
        return views[:3]              # the set keeps an earlier frame's P3..P5
    if N not in tdb:
        tdb[N] = real[1](c, N, planned=planned)
    return tdb[N]


bu.forward, bb.top_down = fake_forward, fake_top_down
model([frames[:20]])
torch.cuda.synchronize()
print("look-ahead trunk + top-down removed", " ".join(f"{v:6.1f}" for v in rate(model)), "frames/s   (the three P3..P5 copies per frame remain)")
bu.forward, bb.top_down = real
