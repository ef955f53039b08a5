"""A restatement of the federated loss's class choice (`get_fed_loss_inds`, detic/modeling/utils.py:16-28, with the draw written out
as torch.multinomial defines it: the largest prob / q for q ~ Exp(1)) -> the 0 / 1 class weight `fed_loss_weight_kernel` must produce.
tests/test_vocab_training_cpu.py checks it against torch.multinomial itself; the GPU tests check the kernel against it."""
import torch


def fed_loss_weight_ref(gt_classes: torch.Tensor, C: int, q: torch.Tensor, num_sample_cats: int, prob=None, zero_mask_src=None):
    gt = gt_classes.long().cpu()
    appeared = torch.unique(gt[gt >= 0])                       # the background label C counts (torch.unique(gt_classes))
    fg = appeared[appeared < C]
    w = torch.zeros(C)
    w[fg] = 1.0
    need = int(num_sample_cats) - int(appeared.numel())
    if need > 0:
        p = torch.ones(C) if prob is None else prob.detach().float().cpu().clone()
        eligible = p > 0
        eligible[fg] = False
        key = p / q.detach().float().cpu()                     # IEEE fp32 division
        key[~eligible] = -1.0
        order = torch.argsort(-key, stable=True)               # descending, ties to the lower class index
        drawn = order[:need]
        w[drawn[eligible[drawn]]] = 1.0                        # fewer eligible classes than asked for: all of them
    if zero_mask_src is not None:
        w = w * (zero_mask_src.detach().float().cpu() > 1e-4).float()
    return w
