# -*- coding: utf-8 -*-
"""Classifier tail on the kernel pack (hip/head.h).

* ``pool_fc(x, fc)`` — global average pool + ``nn.Linear`` as ONE forward
  launch (``head_fwd``) and, in training, one backward call (``head_bwd``:
  a dx kernel and a dw/db reduce).  Opt-in: ``FEDTORCH_FUSED_HEAD=1``.
* ``MetricAccumulator`` — cross-entropy sum, top-1 / top-5 counts and the
  sample count of a validation pass, added up on the device by one
  ``ce_topk_accum`` launch per batch and read back ONCE.  The validation
  loops (trainings/eval.py, trainings/eval_centered.py) use it with
  ``FEDTORCH_FUSED_METRICS=1``.

Both default OFF; per-call and in-bench figures: profiles/head_notes.md.

Numerics.  The fused head reads x / weight / bias in their own dtypes,
accumulates in fp32 and returns **fp32 logits**.  Under bf16 autocast the
stock path rounds the pooled vector and the logits to bf16 and returns bf16
logits, so with the flag on the loss sees un-rounded logits (and
``logits.dtype`` differs).  Without autocast (fp32 model) both return fp32.

Metric rules (the kernel and the torch fallback implement the same three):
per sample, in fp32 from the stored logit values z and the target t,

    loss = log(sum_j exp(z_j - max z)) - (z_t - max z)
    rank = #{j : z_j > z_t} + #{j < t : z_j == z_t}
    the sample is a top-k hit  iff  rank < k

i.e. among equal logits the LOWER class index wins.  A sample whose target
is outside [0, K) — ``ignore_index`` -100 included — is skipped entirely: it
adds nothing, not even to n.  (The stock per-batch path counts such a sample
in the batch size and as a miss.)
"""
import os

import torch
import torch.nn as nn
import torch.nn.functional as F
from torch.autograd.function import once_differentiable

from fedtorch_amd import ops

_HEAD_ENABLED = os.environ.get('FEDTORCH_FUSED_HEAD', '0') == '1'
_METRICS_ENABLED = os.environ.get('FEDTORCH_FUSED_METRICS', '0') == '1'

MAX_C = 1024
MAX_K = 1024
_FLOATS = (torch.bfloat16, torch.float32)


def _kernels_active(t):
    return t.is_cuda and ops.hip_available() and not ops.FORCE_EAGER


# --------------------------------------------------------------------------
# pool + FC
# --------------------------------------------------------------------------
class _PoolFCFn(torch.autograd.Function):
    """logits = mean_hw(x) @ weight^T + bias over head_fwd / head_bwd."""

    @staticmethod
    def forward(ctx, x, weight, bias):
        b = bias if bias is not None else torch.empty(0, device=x.device)
        logits, pooled = ops._C.head_fwd(x, weight, b)
        ctx.save_for_backward(pooled, weight, b)
        ctx.hw = (x.size(2), x.size(3))
        ctx.x_bf16 = x.dtype == torch.bfloat16
        ctx.has_bias = bias is not None
        return logits

    @staticmethod
    @once_differentiable
    def backward(ctx, dlogits):
        pooled, weight, b = ctx.saved_tensors
        need_dx, need_dw, need_db = ctx.needs_input_grad
        if dlogits.dtype != torch.float32:
            dlogits = dlogits.float()
        dx, dw, db = ops._C.head_bwd(
            dlogits.contiguous(), pooled, weight, b, ctx.hw[0], ctx.hw[1],
            ctx.x_bf16, bool(need_dx))
        return (dx if need_dx else None, dw if need_dw else None,
                db if (need_db and ctx.has_bias) else None)


def head_eligible(x, fc):
    """the fused head applies to this (feature map, linear layer) pair"""
    if not (_HEAD_ENABLED and isinstance(x, torch.Tensor)
            and isinstance(fc, nn.Linear) and _kernels_active(x)):
        return False
    if x.dim() != 4 or x.dtype not in _FLOATS or x.numel() == 0:
        return False
    C, K = fc.in_features, fc.out_features
    if x.size(1) != C or C % 8 or not 8 <= C <= MAX_C or not 1 <= K <= MAX_K:
        return False
    if not x.is_contiguous(memory_format=torch.channels_last):
        return False
    w, b = fc.weight, fc.bias
    if w.device != x.device or w.dtype not in _FLOATS \
            or not w.is_contiguous():
        return False
    if b is not None and (b.device != x.device or b.dtype not in _FLOATS
                          or not b.is_contiguous()):
        return False
    # the kernels use 16-byte loads along C
    return x.data_ptr() % 16 == 0 and w.data_ptr() % 16 == 0


def pool_fc(x, fc, pool=None):
    """``fc(pool(x).flatten(1))`` with ``pool`` a global average pool
    (``F.adaptive_avg_pool2d(x, 1)`` when no module is given).  With
    FEDTORCH_FUSED_HEAD=1 and an eligible pair (GPU, 4-D channels_last
    bf16/fp32 x, nn.Linear with C % 8 == 0, 8 <= C <= 1024, K <= 1024) it is
    one head_fwd launch, in training and eval, with and without grad; the
    result is then fp32 whatever autocast says (module docstring)."""
    if _HEAD_ENABLED and head_eligible(x, fc):
        return _PoolFCFn.apply(x, fc.weight, fc.bias)
    pooled = pool(x) if pool is not None else F.adaptive_avg_pool2d(x, 1)
    return fc(pooled.flatten(1))


# --------------------------------------------------------------------------
# loss / top-k accumulator
# --------------------------------------------------------------------------
class MetricAccumulator(object):
    """(loss_sum, top1_count, top5_count, n) of every ``update`` since the
    last ``reset``, kept in a float64 [4] tensor on ``device``.  ``update``
    never synchronises; ``result`` is the one device->host read."""

    def __init__(self, device):
        self.device = torch.device(device)
        self.acc = torch.zeros(4, dtype=torch.float64, device=self.device)

    def update(self, logits, target):
        if _kernels_active(logits):
            z = logits.detach()
            if z.dtype not in _FLOATS:
                z = z.float()
            ops._C.ce_topk_accum(z.contiguous(), target.contiguous(),
                                 self.acc)
        else:
            self.acc += _metrics_torch(logits.detach(), target)

    def result(self):
        loss_sum, top1, top5, n = self.acc.tolist()
        return loss_sum, int(top1), int(top5), int(n)

    def reset(self):
        self.acc.zero_()


def _metrics_torch(logits, target):
    """the module docstring's three formulas in torch ops (CPU, or a GPU
    without the extension); float64 [4] on logits' device, no host sync"""
    z = logits.float()
    K = z.size(1)
    valid = (target >= 0) & (target < K)
    t = target.clamp(0, K - 1).view(-1, 1)
    m = z.max(dim=1, keepdim=True).values
    zt = z.gather(1, t)
    loss = torch.log(torch.exp(z - m).sum(dim=1)) - (zt - m).squeeze(1)
    j = torch.arange(K, device=z.device).view(1, -1)
    rank = ((z > zt) | ((z == zt) & (j < t))).sum(dim=1)
    zero = torch.zeros((), dtype=torch.float64, device=z.device)
    return torch.stack([
        torch.where(valid, loss.double(), zero).sum(),
        ((rank < 1) & valid).sum().double(),
        ((rank < 5) & valid).sum().double(),
        valid.sum().double()])


# --------------------------------------------------------------------------
# validation-loop glue
# --------------------------------------------------------------------------
def metrics_eligible(args, criterion, metrics):
    """the validation pass may accumulate its metrics on the device: plain
    mean-reduced nn.CrossEntropyLoss, classification arch, top-1[/top-5]"""
    return (_METRICS_ENABLED
            and type(criterion) is nn.CrossEntropyLoss
            and criterion.reduction == 'mean'
            and criterion.weight is None
            and getattr(criterion, 'label_smoothing', 0.0) == 0.0
            and criterion.ignore_index == -100
            and getattr(args, 'arch', None) != 'rnn'
            and tuple(metrics) in ((1,), (1, 5)))


def batch_eligible(output, target):
    if not (isinstance(output, torch.Tensor) and output.dim() == 2
            and output.is_floating_point() and target.dim() == 1
            and target.dtype == torch.int64
            and target.size(0) == output.size(0)
            and target.device == output.device):
        return False
    return not (_kernels_active(output) and output.size(1) > MAX_K)


def fill_meters(tracker, macc, metrics):
    """the single read-back: leave in the losses / top1 / top5 meters what
    the per-batch updates would have (sum += mean * batch, count += batch)"""
    loss_sum, top1, top5, n = macc.result()
    if n == 0:
        return tracker
    pairs = [('losses', loss_sum), ('top1', 100.0 * top1)]
    if len(metrics) == 2:
        pairs.append(('top5', 100.0 * top5))
    for name, s in pairs:
        meter = tracker[name]
        meter.sum += s
        meter.count += n
        meter.avg = meter.sum / meter.count
        meter.val = meter.avg
    return tracker
