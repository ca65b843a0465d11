# -*- coding: utf-8 -*-
"""Single-layer GRU sequence on the kernel pack (hip/gru.h).

``gru_seq(gru, x, h0)`` has the contract of ``gru(x, h0)`` for a
``batch_first`` ``nn.GRU``.  Opt-in: ``FEDTORCH_FUSED_GRU=1``.  An eligible
call (``gru_eligible``) is

* one ``F.linear`` for the input projection of all T steps
  (``gx = x W_ih^T + b_ih``, with its library autograd),
* ONE ``gru_fwd`` launch for the T sequential steps, and in training ONE
  ``gru_bwd`` launch for the reverse sweep, plus two deterministic library
  reductions outside the sequential chain
  (``dW_hh = dgh^T @ h_prev``, ``db_hh = sum dgh``).

Every other call -- the flag off, a CPU tensor, a GRU the kernels do not
cover -- is exactly ``gru(x, h0)``.  Default OFF; timings against the library
path: profiles/gru_notes.md.

Numerics.  The fused path computes ``gx`` in fp32 with autocast disabled,
reads ``weight_hh`` / ``bias_hh`` in their own dtype (bf16 or fp32),
accumulates in fp32 and returns **fp32** ``out`` and ``h_n`` whatever
autocast says.  Under bf16 autocast the stock path returns bf16 ``out`` /
``h_n`` (and rounds the recurrent products to bf16), so with the flag on the
decoder and the carried hidden state see un-rounded values and the dtypes
differ.  Without autocast (fp32 model) both paths return fp32.  The
gradients of ``weight_hh`` / ``bias_hh`` are reduced in fp32 and cast with
round-to-nearest-even to the parameters' dtypes.
"""
import os

import torch
import torch.nn as nn
import torch.nn.functional as F
from torch.autograd.function import once_differentiable

from fedtorch_amd import ops

_GRU_ENABLED = os.environ.get('FEDTORCH_FUSED_GRU', '0') == '1'

MAX_H = 64
_FLOATS = (torch.bfloat16, torch.float32)


def _kernels_active(t):
    return t.is_cuda and ops.hip_available() and not ops.FORCE_EAGER


class _GRUSeqFn(torch.autograd.Function):
    """out[:, t] = GRU cell(gx[:, t], out[:, t-1]) over gru_fwd / gru_bwd;
    gx [B, T, 3H] fp32, h0 [B, H] fp32."""

    @staticmethod
    def forward(ctx, gx, w_hh, b_hh, h0, need):
        out, gates = ops._C.gru_fwd(gx, w_hh, b_hh, h0, need)
        if need:
            ctx.save_for_backward(out, gates, w_hh, h0)
            ctx.b_dtype = b_hh.dtype
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, dout):
        out, gates, w_hh, h0 = ctx.saved_tensors
        need_dw, need_db = ctx.needs_input_grad[1:3]
        if dout.dtype != torch.float32:
            dout = dout.float()
        dgx, dgh, dh0 = ops._C.gru_bwd(dout.contiguous(), out, gates, w_hh,
                                       h0)
        dw = db = None
        if need_dw:
            dw = hh_weight_grad(dgh, out, h0).to(w_hh.dtype)
        if need_db:
            db = hh_bias_grad(dgh).to(ctx.b_dtype)
        return dgx, dw, db, dh0, None


def hh_weight_grad(dgh, out, h0):
    """dW_hh [3H, H] = dgh^T @ h_prev with h_prev = (h0, out[:, :-1]): one
    deterministic fp32 library GEMM outside the sequential chain"""
    H = out.size(2)
    h_prev = torch.cat((h0.unsqueeze(1), out[:, :-1]), dim=1)
    return dgh.view(-1, 3 * H).t() @ h_prev.view(-1, H)


def hh_bias_grad(dgh):
    """db_hh [3H] = sum of dgh over batch and time"""
    return dgh.sum((0, 1))


def gru_eligible(gru, x, h0):
    """the fused sequence kernels apply to this (GRU, input, hidden) call"""
    if not (_GRU_ENABLED and isinstance(x, torch.Tensor)
            and isinstance(h0, torch.Tensor) and isinstance(gru, nn.GRU)
            and _kernels_active(x)):
        return False
    if gru.num_layers != 1 or gru.bidirectional or not gru.batch_first \
            or not gru.bias or getattr(gru, 'proj_size', 0) != 0:
        return False
    H = gru.hidden_size
    if not 1 <= H <= MAX_H:
        return False
    for p in (gru.weight_ih_l0, gru.weight_hh_l0, gru.bias_ih_l0,
              gru.bias_hh_l0):
        if p.device != x.device or p.dtype not in _FLOATS \
                or not p.is_contiguous():
            return False
    if x.dim() != 3 or not x.is_floating_point() or x.numel() == 0 \
            or x.size(2) != gru.input_size:
        return False
    return (h0.device == x.device and h0.is_floating_point()
            and tuple(h0.shape) == (1, x.size(0), H))


def gru_seq(gru, x, h0):
    """``gru(x, h0)`` -> ``(out [B, T, H], h_n [1, B, H])``.  With
    FEDTORCH_FUSED_GRU=1 and an eligible call (GPU, one unidirectional
    batch_first layer with biases, hidden_size <= 64, bf16/fp32 contiguous
    parameters, x [B, T, I], h0 [1, B, H]) the T steps are one gru_fwd
    launch, in training and eval; ``out`` and ``h_n = out[:, -1]`` are then
    fp32 whatever autocast says (module docstring)."""
    if not (_GRU_ENABLED and gru_eligible(gru, x, h0)):
        return gru(x, h0)
    with torch.autocast(device_type='cuda', enabled=False):
        gx = F.linear(x.float(), gru.weight_ih_l0.float(),
                      gru.bias_ih_l0.float())
        args = (gx.contiguous(), gru.weight_hh_l0, gru.bias_hh_l0,
                h0[0].float().contiguous())
        # the gates are stored only where a backward can follow
        need = torch.is_grad_enabled() and any(t.requires_grad for t in args)
        out = _GRUSeqFn.apply(*args, need)
    return out, out[:, -1].unsqueeze(0)
