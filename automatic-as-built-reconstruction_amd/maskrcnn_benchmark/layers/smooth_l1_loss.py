"""reference: maskrcnn_benchmark/layers/smooth_l1_loss.py:34-52 -- `smooth_l1_loss` with the reference's signature on the
library's list-form kernels (include/aabr_hip.h aabr_smooth_l1_forward / _backward), with autograd.

Yaw mode 'Diff' (and 'Diff_<w>', whose weight the reference parses and never applies) is the plain smooth L1 on all 7
columns.  'SinDiff' raises ValueError: RPNLossComputation passes a tensor as `anchor` (rpn/loss_3d.py:238-241) and the
mode reads `anchor.bbox3d` (smooth_l1_loss.py:27), so it never runs in the reference's RPN loss.  ENABLE_SYMEETRIC_CORNER
is False there (its other branch stops in a debugger) and has no counterpart."""
import torch

import _hip
from _hip import check, ptr, stream
from rpn_glue import parse_yaw_loss_mode


class _SmoothL1(torch.autograd.Function):
    @staticmethod
    def forward(ctx, input, target, beta, divisor):
        lib = _hip.load()
        x = input.contiguous()
        t = target.detach().float().contiguous()
        out = torch.empty((), dtype=torch.float32, device=x.device)
        scr = _hip.workspace("smooth_l1", int(lib.aabr_smooth_l1_scratch_floats()), torch.float32, x.device)
        check(lib.aabr_smooth_l1_forward(ptr(x), ptr(t), x.numel(), int(x.dtype == torch.bfloat16), float(beta),
                                         float(divisor), ptr(out), ptr(scr), stream()))
        ctx.save_for_backward(x, t)
        ctx.beta, ctx.divisor = beta, divisor
        return out

    @staticmethod
    def backward(ctx, g):
        x, t = ctx.saved_tensors
        grad = torch.empty_like(x)
        check(_hip.load().aabr_smooth_l1_backward(ptr(x), ptr(t), x.numel(), int(x.dtype == torch.bfloat16),
                                                  float(ctx.beta), float(ctx.divisor), ptr(g.float().contiguous()),
                                                  ptr(grad), stream()))
        gt = -grad.float() if ctx.needs_input_grad[1] else None
        return grad, gt, None, None


def smooth_l1_loss(input, target, anchor, beta=1. / 9, size_average=True, yaw_loss_mode='Diff'):
    """very similar to the smooth_l1_loss from pytorch, but with the extra beta parameter: input / target / anchor [n, 7]
    (input fp32 or bf16, on the device); the mean over the n x 7 terms (size_average) or their sum, a 0-dim fp32 tensor"""
    assert input.shape[0] == target.shape[0] == anchor.shape[0]
    assert input.shape[1] == target.shape[1] == anchor.shape[1] == 7
    parse_yaw_loss_mode(yaw_loss_mode)
    if input.dtype not in (torch.float32, torch.bfloat16):
        raise TypeError("smooth_l1_loss: input must be float32 or bfloat16")
    _hip.require_gpu(input)
    n = input.numel()
    return _SmoothL1.apply(input, target, float(beta), float(n) if size_average else 1.0)
