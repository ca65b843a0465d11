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

Hidden sizes 65..128 (``gru_wide_eligible``) take the same route over
``gru_wide_fwd`` / ``gru_wide_bwd`` (hip/gru_wide.h: W_hh resident in
registers instead of LDS) when ``FEDTORCH_FUSED_GRU_WIDE=1`` is set as well.

Hidden sizes 129..256 (``gru_stream_eligible``) take it over
``gru_stream_fwd`` / ``gru_stream_bwd`` (hip/gru_stream.h: W_hh is too large
for one workgroup's registers or LDS there, so every step streams it from
global memory -- L2 after the first step -- into the MFMA B fragments) when
``FEDTORCH_FUSED_GRU_STREAM=1`` is set on top of ``FEDTORCH_FUSED_GRU=1``.
Within each 16-deep block of the recurrent sums these kernels add in another
order than the two above; results are deterministic all the same.

Every other call -- the flag off, a CPU tensor, a GRU the kernels do not
cover (hidden_size > 256 among them) -- is exactly ``gru(x, h0)``.  All
flags default OFF; timings against the library path: profiles/gru_notes.md.
The token path below stops at hidden size 128.

Token input (``gru_tok_seq(encoder, gru, tok, h0)``, third opt-in
``FEDTORCH_FUSED_GRU_TOKENS=1`` on top of the flags above, default OFF).  When
the layer's input is ``encoder(tok)`` for a plain ``nn.Embedding``,
``gx[b, t]`` is one of the V rows of ``P = E W_ih^T + b_ih``.  An eligible
call (``gru_tok_eligible``) is one ``addmm`` over V rows (library autograd:
``dE``, ``dW_ih``, ``db_ih`` from ``dP``), ONE ``gru_tok_fwd`` /
``gru_tok_wide_fwd`` launch that gathers ``P[tok]`` inside the sequence
kernel, and in training the unchanged ``gru_bwd`` / ``gru_wide_bwd`` plus ONE
``gru_tok_grads`` launch for ``dP``, ``dW_hh`` and ``db_hh`` (hip/gru_tok.h).
``emb``, ``gx`` and the concatenated ``h_prev`` are never materialised.  A
token outside ``[0, V)`` -- on which ``nn.Embedding`` faults -- reads
``gx = 0`` and contributes nothing to ``dP``: the launchers never read ``tok``
on the host.  An infinite ``dgx`` element turns its column of the whole
16-row vocabulary tile of ``dP`` into NaN (0 * inf in the one-hot product).

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
# second opt-in on top of the first: hidden sizes MAX_H + 1 .. MAX_H_WIDE
_GRU_WIDE_ENABLED = os.environ.get('FEDTORCH_FUSED_GRU_WIDE', '0') == '1'
# opt-in on top of the first: hidden sizes MAX_H_WIDE + 1 .. MAX_H_STREAM
_GRU_STREAM_ENABLED = os.environ.get('FEDTORCH_FUSED_GRU_STREAM', '0') == '1'
# third opt-in on top of those: token input through the [V, 3H] table
_GRU_TOK_ENABLED = os.environ.get('FEDTORCH_FUSED_GRU_TOKENS', '0') == '1'

MAX_H = 64
MAX_H_WIDE = 128
MAX_H_STREAM = 256
_FLOATS = (torch.bfloat16, torch.float32)


def _kernels_active(t):
    return t.is_cuda and ops.hip_available() and not ops.FORCE_EAGER


def _seq_forward(ctx, fwd, gx, w_hh, b_hh, h0, need):
    out, gates = fwd(gx, w_hh, b_hh, h0, need)
    if need:
        ctx.save_for_backward(out, gates, w_hh, h0)
        ctx.b_dtype = b_hh.dtype
    return out


def _seq_backward(ctx, bwd, dout):
    out, gates, w_hh, h0 = ctx.saved_tensors
    need_dw, need_db = ctx.needs_input_grad[1:3]
    if dout.dtype != torch.float32:
        dout = dout.float()
    dgx, dgh, dh0 = bwd(dout.contiguous(), out, gates, w_hh, h0)
    dw = db = None
    if need_dw:
        dw = hh_weight_grad(dgh, out, h0).to(w_hh.dtype)
    if need_db:
        db = hh_bias_grad(dgh).to(ctx.b_dtype)
    return dgx, dw, db, dh0, None


class _GRUSeqFn(torch.autograd.Function):
    """out[:, t] = GRU cell(gx[:, t], out[:, t-1]) over gru_fwd / gru_bwd;
    gx [B, T, 3H] fp32, h0 [B, H] fp32."""

    @staticmethod
    def forward(ctx, gx, w_hh, b_hh, h0, need):
        return _seq_forward(ctx, ops._C.gru_fwd, gx, w_hh, b_hh, h0, need)

    @staticmethod
    @once_differentiable
    def backward(ctx, dout):
        return _seq_backward(ctx, ops._C.gru_bwd, dout)


class _GRUWideSeqFn(torch.autograd.Function):
    """the same over gru_wide_fwd / gru_wide_bwd (65 <= H <= 128)"""

    @staticmethod
    def forward(ctx, gx, w_hh, b_hh, h0, need):
        return _seq_forward(ctx, ops._C.gru_wide_fwd, gx, w_hh, b_hh, h0,
                            need)

    @staticmethod
    @once_differentiable
    def backward(ctx, dout):
        return _seq_backward(ctx, ops._C.gru_wide_bwd, dout)


class _GRUStreamSeqFn(torch.autograd.Function):
    """the same over gru_stream_fwd / gru_stream_bwd (129 <= H <= 256)"""

    @staticmethod
    def forward(ctx, gx, w_hh, b_hh, h0, need):
        return _seq_forward(ctx, ops._C.gru_stream_fwd, gx, w_hh, b_hh, h0,
                            need)

    @staticmethod
    @once_differentiable
    def backward(ctx, dout):
        return _seq_backward(ctx, ops._C.gru_stream_bwd, dout)


def _tok_forward(ctx, fwd, P, tok, w_hh, b_hh, h0, need):
    out, gates = fwd(P, tok, w_hh, b_hh, h0, need)
    if need:
        ctx.save_for_backward(out, gates, w_hh, h0, tok)
        ctx.vocab = P.size(0)
        ctx.b_dtype = b_hh.dtype
    return out


def _tok_backward(ctx, bwd, dout):
    out, gates, w_hh, h0, tok = ctx.saved_tensors
    if dout.dtype != torch.float32:
        dout = dout.float()
    dgx, dgh, dh0 = bwd(dout.contiguous(), out, gates, w_hh, h0)
    dP, dw, db = ops._C.gru_tok_grads(dgx, dgh, out, h0, tok, ctx.vocab)
    return dP, None, dw.to(w_hh.dtype), db.to(ctx.b_dtype), dh0, None


class _GRUTokSeqFn(torch.autograd.Function):
    """_GRUSeqFn with gx[b, t] = P[tok[b, t]]: P [V, 3H] fp32, tok [B, T]
    int64; backward is gru_bwd, then gru_tok_grads for dP, dW_hh, db_hh"""

    @staticmethod
    def forward(ctx, P, tok, w_hh, b_hh, h0, need):
        return _tok_forward(ctx, ops._C.gru_tok_fwd, P, tok, w_hh, b_hh, h0,
                            need)

    @staticmethod
    @once_differentiable
    def backward(ctx, dout):
        return _tok_backward(ctx, ops._C.gru_bwd, dout)


class _GRUTokWideSeqFn(torch.autograd.Function):
    """the same over gru_tok_wide_fwd / gru_wide_bwd (65 <= H <= 128)"""

    @staticmethod
    def forward(ctx, P, tok, w_hh, b_hh, h0, need):
        return _tok_forward(ctx, ops._C.gru_tok_wide_fwd, P, tok, w_hh, b_hh,
                            h0, need)

    @staticmethod
    @once_differentiable
    def backward(ctx, dout):
        return _tok_backward(ctx, ops._C.gru_wide_bwd, dout)


def hh_weight_grad(dgh, out, h0):
    """dW_hh [3H, H] = dgh^T @ h_prev with h_prev = (h0, out[:, :-1]): one
    deterministic fp32 library GEMM outside the sequential chain"""
    H = out.size(2)
    h_prev = torch.cat((h0.unsqueeze(1), out[:, :-1]), dim=1)
    return dgh.view(-1, 3 * H).t() @ h_prev.view(-1, H)


def hh_bias_grad(dgh):
    """db_hh [3H] = sum of dgh over batch and time"""
    return dgh.sum((0, 1))


def _gru_covered(gru, x, h0, h_min, h_max):
    """the flag is on and the GRU and hidden state are ones the sequence
    kernels serve, with h_min <= hidden_size <= h_max, for an input tensor
    ``x`` (floats [B, T, I] or tokens [B, T]) whose device decides"""
    if not (_GRU_ENABLED and isinstance(x, torch.Tensor)
            and isinstance(h0, torch.Tensor) and isinstance(gru, nn.GRU)
            and _kernels_active(x)):
        return False
    if gru.num_layers != 1 or gru.bidirectional or not gru.batch_first \
            or not gru.bias or getattr(gru, 'proj_size', 0) != 0:
        return False
    H = gru.hidden_size
    if not h_min <= H <= h_max:
        return False
    for p in (gru.weight_ih_l0, gru.weight_hh_l0, gru.bias_ih_l0,
              gru.bias_hh_l0):
        if p.device != x.device or p.dtype not in _FLOATS \
                or not p.is_contiguous():
            return False
    return (x.dim() >= 1 and h0.device == x.device
            and h0.is_floating_point()
            and tuple(h0.shape) == (1, x.size(0), H))


def _covered(gru, x, h0, h_min, h_max):
    """the flag is on and the (GRU, input, hidden) call is one the sequence
    kernels serve, with h_min <= hidden_size <= h_max"""
    if not _gru_covered(gru, x, h0, h_min, h_max):
        return False
    return (x.dim() == 3 and x.is_floating_point() and x.numel() > 0
            and x.size(2) == gru.input_size)


def gru_eligible(gru, x, h0):
    """the fused sequence kernels apply to this (GRU, input, hidden) call"""
    return _covered(gru, x, h0, 1, MAX_H)


def gru_wide_eligible(gru, x, h0):
    """the register-resident kernels (MAX_H < hidden_size <= MAX_H_WIDE)
    apply to this call: the conditions of ``gru_eligible`` with that range,
    and FEDTORCH_FUSED_GRU_WIDE=1 on top of FEDTORCH_FUSED_GRU=1"""
    return _GRU_WIDE_ENABLED and _covered(gru, x, h0, MAX_H + 1, MAX_H_WIDE)


def gru_stream_eligible(gru, x, h0):
    """the streamed-weight kernels (MAX_H_WIDE < hidden_size <= MAX_H_STREAM)
    apply to this call: the conditions of ``gru_eligible`` with that range,
    and FEDTORCH_FUSED_GRU_STREAM=1 on top of FEDTORCH_FUSED_GRU=1"""
    return _GRU_STREAM_ENABLED and _covered(gru, x, h0, MAX_H_WIDE + 1,
                                            MAX_H_STREAM)


def gru_seq(gru, x, h0):
    """``gru(x, h0)`` -> ``(out [B, T, H], h_n [1, B, H])``.  With
    FEDTORCH_FUSED_GRU=1 and an eligible call (GPU, one unidirectional
    batch_first layer with biases, hidden_size <= 64, bf16/fp32 contiguous
    parameters, x [B, T, I], h0 [1, B, H]) the T steps are one gru_fwd
    launch, in training and eval; ``out`` and ``h_n = out[:, -1]`` are then
    fp32 whatever autocast says (module docstring).  With
    FEDTORCH_FUSED_GRU_WIDE=1 as well, 65 <= hidden_size <= 128 takes the
    same route over gru_wide_fwd / gru_wide_bwd, and with
    FEDTORCH_FUSED_GRU_STREAM=1 129 <= hidden_size <= 256 takes it over
    gru_stream_fwd / gru_stream_bwd."""
    if gru_eligible(gru, x, h0):
        fn = _GRUSeqFn
    elif gru_wide_eligible(gru, x, h0):
        fn = _GRUWideSeqFn
    elif gru_stream_eligible(gru, x, h0):
        fn = _GRUStreamSeqFn
    else:
        return gru(x, h0)
    with torch.autocast(device_type='cuda', enabled=False):
        gx = F.linear(x.float(), gru.weight_ih_l0.float(),
                      gru.bias_ih_l0.float())
        args = (gx.contiguous(), gru.weight_hh_l0, gru.bias_hh_l0,
                h0[0].float().contiguous())
        # the gates are stored only where a backward can follow
        need = torch.is_grad_enabled() and any(t.requires_grad for t in args)
        out = fn.apply(*args, need)
    return out, out[:, -1].unsqueeze(0)


def _tok_fn(gru, tok, h0):
    """the autograd function of the token path for this GRU, or None"""
    if not _GRU_TOK_ENABLED:
        return None
    if _gru_covered(gru, tok, h0, 1, MAX_H):
        return _GRUTokSeqFn
    if _GRU_WIDE_ENABLED and _gru_covered(gru, tok, h0, MAX_H + 1,
                                          MAX_H_WIDE):
        return _GRUTokWideSeqFn
    return None


def gru_tok_eligible(encoder, gru, tok, h0):
    """the token path applies to ``gru(encoder(tok), h0)``:
    FEDTORCH_FUSED_GRU_TOKENS=1 on top of the conditions of ``gru_eligible``
    / ``gru_wide_eligible`` for the GRU and h0; ``tok`` a non-empty int64
    [B, T] tensor on the GPU; ``encoder`` a plain ``nn.Embedding`` (no
    padding_idx, max_norm, sparse or scale_grad_by_freq) with a contiguous
    fp32 / bf16 weight on that device and embedding_dim == gru.input_size"""
    if _tok_fn(gru, tok, h0) is None:
        return False
    if tok.dtype != torch.int64 or tok.dim() != 2 or tok.numel() == 0:
        return False
    if type(encoder) is not nn.Embedding or encoder.padding_idx is not None \
            or encoder.max_norm is not None or encoder.sparse \
            or encoder.scale_grad_by_freq:
        return False
    E = encoder.weight
    return (E.device == tok.device and E.dtype in _FLOATS
            and E.is_contiguous()
            and encoder.embedding_dim == gru.input_size)


def gru_tok_seq(encoder, gru, tok, h0):
    """``gru(encoder(tok), h0)`` -> ``(out [B, T, H], h_n [1, B, H])``.  An
    eligible call (``gru_tok_eligible``) never builds ``encoder(tok)`` or
    ``gx``: one addmm makes the table P = E W_ih^T + b_ih [V, 3H], one
    gru_tok_fwd / gru_tok_wide_fwd launch runs the T steps on P[tok], and
    backward is gru_bwd / gru_wide_bwd plus one gru_tok_grads launch; ``out``
    and ``h_n`` are fp32 as in ``gru_seq``.  A token outside [0, V) reads
    gx = 0 there (module docstring).  Anything else is
    ``gru_seq(gru, encoder(tok), h0)``."""
    if not gru_tok_eligible(encoder, gru, tok, h0):
        return gru_seq(gru, encoder(tok), h0)
    fn = _tok_fn(gru, tok, h0)
    with torch.autocast(device_type='cuda', enabled=False):
        P = torch.addmm(gru.bias_ih_l0.float(), encoder.weight.float(),
                        gru.weight_ih_l0.float().t())
        args = (P, tok.contiguous(), gru.weight_hh_l0, gru.bias_hh_l0,
                h0[0].float().contiguous())
        # the gates are stored only where a backward can follow
        need = torch.is_grad_enabled() and any(t.requires_grad for t in args)
        out = fn.apply(*args, need)
    return out, out[:, -1].unsqueeze(0)
