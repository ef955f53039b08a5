"""MI355X-native per-frame recurrent inference path of the embodied object detector.

Public surface (mirrors what `Detic/train_mp3d.py --eval-only` touches):
    setup_cfg / get_cfg            config (yacs-compatible CfgNode, `_BASE_`, KEY VALUE overrides)
    build_model(cfg[, state_dict]) registries + CustomRCNNRecurrent on the HIP kernels
    model([[frame, ...]])          -> [{"instances": Instances}, ...]
The arithmetic lives in libeod_hip.so (hand-written gfx950 kernels behind the C ABI of include/eod_hip.h).
"""
# The schedule uses up to ~8 streams of one priority (4 per model + one per scene of a BatchedSequences).  The HIP runtime maps the
# streams of a priority onto its hardware queues round-robin, and two streams that share a hardware queue run strictly one after
# the other (tools/experiments/chain_contention.hip).  How many queues a process may open is the host's decision -- a card's queue
# slots are shared by every process on it -- so the package leaves the runtime's environment alone: with fewer queues than streams
# the schedule computes the same results with less overlap.

from .config import CfgNode, get_cfg, setup_cfg  # noqa: F401
from .registry import (BACKBONE_REGISTRY, META_ARCH_REGISTRY, PROPOSAL_GENERATOR_REGISTRY, ROI_HEADS_REGISTRY,  # noqa: F401
                       build_model)
from .structures import Boxes, Instances  # noqa: F401

__version__ = "0.1.0"
