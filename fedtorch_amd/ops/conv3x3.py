# -*- coding: utf-8 -*-
"""NHWC 3x3 convolution modules on the MFMA kernel pack.

Routing lives in three small functions: `_mfma_stride` (is this a shape
the kernels cover), `_kernels_active` (GPU, extension, eager not forced)
and `_bwd_plan` (which dx / dw path a body conv's backward takes).

Default GPU training path for the CIFAR ResNet body convs (Co == Ci,
(Co, W) in {(16,32), (32,16), (64,8)}) and the stride-2 transitions:

* forward: `hip/convfwd.h` conv3x3_bn_fwd_k — direct implicit GEMM with
  a fused BN-stats epilogue (the following BN skips its stats pass via
  the `_ft_bn_part` handoff) — 5.1-6.6 us/call;
* backward-data: conv3x3_dgrad_k (the forward's mirror) — 5.0-6.7 us
  vs MIOpen's 23-24;
* weight gradient: MFMA wrw v2 (`hip/convwrw2.h`, main kernel + one
  reduce/cast/scatter kernel over few, long supertile streams) for the
  channel counts in FEDTORCH_WRW2_C; per-call figures against
  MIOpen-incl-wrappers in profiles/wrw2_notes.md;
* deferred BN backward (opt-in): the BN's elementwise dx pass runs
  inside the dgrad staging, handed off through a data_ptr-keyed side
  table (python tensor attrs do not survive the autograd engine's
  rewrapping);
* stride-2 transition backward (opt-in, FEDTORCH_MFMA_S2_BWD=1):
  `hip/convs2bwd.h` conv3x3s2_dgrad_k (parity-class implicit GEMM) and
  conv3x3s2_wrw_k (column-parity-split staging) replace the one combined
  MIOpen call of _Conv3x3S2BNFn.backward — 20.7 vs 30.0 us (16->32) and
  22.5 vs 22.0 us (32->64) of device time per conv; not resolved in the
  flagship bench, hence off by default (profiles/s2bwd_notes.md);
* eval-mode forward (default, FEDTORCH_MFMA_EVAL=1): under model.eval() +
  no_grad `conv_bn_act` runs conv + BN [+ add] + ReLU as ONE
  conv3x3_bn_act_fwd launch (the running-stats BN folded into the conv
  epilogue) — ResNet-20 forward 0.43-0.52 vs 2.60 ms at N=256
  (profiles/eval_notes.md).

Anything else falls back to stock F.conv2d autograd.  Per-call evidence:
profiles/r02_bench_notes.md; kernel details: hip/README.md.
"""
import os

import torch
import torch.nn as nn
import torch.nn.functional as F

from fedtorch_amd import ops

_CL = torch.channels_last
# what the kernels are built for (the instance table of hip/ops.hip): the
# body convs as (C, W) with Co == Ci at stride 1, the transitions as
# (Ci, W_in) with Co == 2 Ci at stride 2
_SHAPES = {(64, 8), (32, 16), (16, 32)}
_S2_SHAPES = {(16, 32), (32, 16)}
# Default OFF: the kernel is numerically exact (test_conv3x3_wrw_*) but at
# CIFAR sizes it measured 27-79 us/call vs MIOpen's 22-33 us (the LDS-staged
# tile pipeline is latency-bound at these tiny K-tiles; see
# profiles/r01_bench_notes.md "MFMA wrw" entry).  FEDTORCH_MFMA_WRW=1
# re-enables for experimentation.
_ENABLED = os.environ.get('FEDTORCH_MFMA_WRW', '0') == '1'
# MFMA direct conv FORWARD with fused BN-stats epilogue (hip/convfwd.h):
# 5.1-6.6 us/call vs MIOpen's solver stack AND the following BN's stats
# pass dies (its partials come out of the conv epilogue).  Default ON.
_FWD_ENABLED = os.environ.get('FEDTORCH_MFMA_FWD', '1') == '1'
# MFMA wrw v2 (hip/convwrw2.h): transposed-LDS staging + alignbit tap
# shifts, two launches per call (main + final).  FEDTORCH_WRW2=1 forces it
# for every body conv whatever FEDTORCH_WRW2_C says.
_WRW2_ENABLED = os.environ.get('FEDTORCH_WRW2', '0') == '1'
# per-shape wrw2: the channel counts whose wrw runs on the v2 kernel; the
# default holds exactly those that beat MIOpen-incl-wrappers per call
# (profiles/wrw2_notes.md).  Empty string = all body wrw on the library.
_WRW2_DEFAULT_C = '16,32,64'
_WRW2_SHAPES = set(
    int(c) for c in
    os.environ.get('FEDTORCH_WRW2_C', _WRW2_DEFAULT_C).split(',')
    if c.strip())
# MFMA direct conv backward-data (hip/convfwd.h conv3x3_dgrad_k): the fwd
# kernel's mirror, 5.0-6.7 us/call vs MIOpen's 23-24.  Default ON.
_DGRAD_ENABLED = os.environ.get('FEDTORCH_MFMA_DGRAD', '1') == '1'
# Deferred BN backward (hip/convfwd.h TRF path): the BN's elementwise dx
# pass runs inside the conv dgrad staging (which also writes the
# transformed dy for the wrw consumer) — the bnh_bwd_dx kernel leaves the
# hot path.  Handshake: _FusedBNFunction.backward registers
# (xbn, z, coefs, relu) under its outgoing grad tensor's data_ptr; the
# producing conv's backward pops it (python tensor attrs do not survive
# the autograd engine's rewrapping, a data_ptr-keyed side table does).
# MEASURED A WASH at the flagship config (174.0k vs 174.7k samples/s):
# the killed bnh_bwd_dx pass (~145 us/step) is consumed by the coef/mask
# side kernels + the 2 extra tensors the transform stages; default OFF,
# capability kept (tests pin deferred == eager gradients).
_BNDEFER_ENABLED = os.environ.get('FEDTORCH_BN_DEFER', '0') == '1'
# MFMA backward of the two 3x3/stride-2 transition convs
# (hip/convs2bwd.h): parity-class dgrad + parity-plane wrw replace the one
# combined MIOpen call in _Conv3x3S2BNFn.backward.  Opt-in
# (FEDTORCH_MFMA_S2_BWD=1); per-call and in-bench figures in
# profiles/s2bwd_notes.md.
_S2BWD_ENABLED = os.environ.get('FEDTORCH_MFMA_S2_BWD', '0') == '1'
# Eval-mode forward on the kernel pack (model.eval() + no_grad): every
# conv3x3 + BN [+ add] + ReLU group is ONE conv3x3_bn_act_fwd launch (the
# running-stats BN is a per-channel affine on the conv accumulators,
# hip/convfwd.h), the stem / downsample BNs run bn_fwd_eval
# (hip/batchnorm.h).  Default and figures: profiles/eval_notes.md.
_EVAL_DEFAULT = '1'
_EVAL_ENABLED = os.environ.get('FEDTORCH_MFMA_EVAL', _EVAL_DEFAULT) == '1'
_BNBWD_TAGS = {}


def bn_defer_active():
    return _DGRAD_ENABLED and _BNDEFER_ENABLED and not ops.FORCE_EAGER


def register_bn_defer(grad, xbn, z, coefs, relu, dres=None):
    _BNBWD_TAGS[grad.data_ptr()] = (xbn, z, coefs, relu, dres)


def _pop_bn_tag(dy):
    """(channels_last dy, its deferred-BN tag or None).  The tag is popped
    by the INCOMING tensor's ptr before the contiguous() copy could change
    it, then again by the copy's (a missed tag would silently skip the BN
    backward transform)."""
    tag = _BNBWD_TAGS.pop(dy.data_ptr(), None) if _BNBWD_TAGS else None
    dy = dy.contiguous(memory_format=_CL)
    if tag is None and _BNBWD_TAGS:
        tag = _BNBWD_TAGS.pop(dy.data_ptr(), None)
    return dy, tag


_EMPTY = {}


def _empty(dev):
    e = _EMPTY.get(dev)
    if e is None:
        e = _EMPTY[dev] = torch.empty(0, device=dev)
    return e


def _kernels_active(x):
    """the one runtime gate of every kernel route: a GPU tensor, the
    extension built, eager not forced"""
    return x.is_cuda and ops.hip_available() and not ops.FORCE_EAGER


def _mfma_stride(conv, x, v1_rows=False):
    """1 / 2 when `conv` on `x` is a shape the MFMA conv kernels cover, else
    0.  Shape, dtype and layout only, so it holds on CPU tensors too; the
    flags and `_kernels_active` are the caller's.  The stride-1 kernels
    tile H by 8 rows; wrw v1 (`v1_rows`) by its 32-position K-tile."""
    if not (x.dim() == 4 and conv.bias is None and conv.padding == (1, 1)
            and x.dtype == torch.bfloat16
            and x.is_contiguous(memory_format=_CL)):
        return 0
    Ci, Co, H, W = conv.in_channels, conv.out_channels, x.shape[2], x.shape[3]
    if conv.stride == (1, 1) and Co == Ci and (Ci, W) in _SHAPES:
        return int(H % (32 // W if v1_rows else 8) == 0)
    if (conv.stride == (2, 2) and Co == 2 * Ci and (Ci, W) in _S2_SHAPES
            and H % 16 == 0):
        return 2
    return 0


def _kernel_weight(w):
    """w as the kernels read it, bf16 channels_last, or None"""
    wb = w if w.dtype == torch.bfloat16 else \
        w.bfloat16().contiguous(memory_format=_CL)
    return wb if wb.is_contiguous(memory_format=_CL) else None


def _lib_backward(dy, x, weight, stride, want_dx, want_dw):
    """(dx, dw) of a 3x3/p1 conv from ONE aten.convolution_backward call,
    None for the one not wanted"""
    dx, dw, _ = torch.ops.aten.convolution_backward(
        dy, x, weight, None, [stride, stride], [1, 1], [1, 1], False, [0, 0],
        1, [want_dx, want_dw, False])
    return dx, dw


def _bwd_plan(C, tagged):
    """(dx path, dw path, combined) of a body conv's backward, from the
    module flags and the channel count.  dx: 'dgrad' | 'lib', with a live
    deferred-BN tag always 'dgrad_bn' (the BN already SKIPPED its dx pass;
    ignoring the tag would treat dz as dy_conv silently).  dw: 'wrw2' |
    'wrw' (v1, never on a tag's dy_conv) | 'lib'.  combined: both on the
    library, which is ONE call (dgrad+wrw split into two was ~0.2 ms/step
    slower over the 19 body convs)."""
    wrw2 = _WRW2_ENABLED or C in _WRW2_SHAPES
    if tagged:
        return 'dgrad_bn', 'wrw2' if wrw2 else 'lib', False
    dx = 'dgrad' if _DGRAD_ENABLED else 'lib'
    dw = 'wrw2' if wrw2 else 'wrw' if _ENABLED else 'lib'
    return dx, dw, dx == dw == 'lib'


class _Conv3x3BNFn(torch.autograd.Function):
    """y, part = conv3x3(x, w) with the BN-stats partials [grid, Co, 2]
    produced by the conv epilogue (consumed by bn_fwd_train_part so the
    following BN skips its stats pass).  Backward: dx and dw each by the
    path `_bwd_plan` names."""

    @staticmethod
    def forward(ctx, x, weight):
        grid = x.shape[0] * (x.shape[2] // 8) * \
            (2 if weight.shape[0] == 64 else 1)
        part = torch.empty(grid, weight.shape[0], 2, device=x.device)
        e = _empty(x.device)
        y = ops._C.conv3x3_bn_fwd(x, weight, part, e, e, e, False)
        ctx.save_for_backward(x, weight)
        ctx.mark_non_differentiable(part)
        # without this the engine materializes a ZERO gradient for `part`
        # every backward: 18 fill kernels/step (~60 us) in the profile
        ctx.set_materialize_grads(False)
        return y, part

    @staticmethod
    def backward(ctx, dy, _dpart):
        x, weight = ctx.saved_tensors
        dy, tag = _pop_bn_tag(dy)
        need_dx = bool(ctx.needs_input_grad[0])
        dx_path, dw_path, combined = _bwd_plan(weight.shape[0],
                                               tag is not None)
        if combined:
            return _lib_backward(dy, x, weight, 1, need_dx, True)
        dx = None
        if dx_path == 'dgrad_bn':
            # dy is dz here; the kernel also hands back dy_conv for the wrw
            xbn, z, coefs, relu, dres = tag
            dx, dy = ops._C.conv3x3_dgrad_bn(
                dy, weight, xbn, z if z is not None else xbn, coefs, relu,
                dres if dres is not None else _empty(dy.device))
            if not need_dx:
                dx = None
        elif need_dx and dx_path == 'dgrad':
            dx = ops._C.conv3x3_dgrad(dy, weight)
        elif need_dx:
            dx = _lib_backward(dy, x, weight, 1, True, False)[0]
        if dw_path == 'wrw2':
            dw = ops._C.conv3x3_wrw2(dy, x)
        elif dw_path == 'wrw':
            dw = ops._C.conv3x3_wrw(dy, x)
        else:
            dw = _lib_backward(dy, x, weight, 1, False, True)[1]
        return dx, dw


class _Conv3x3S2BNFn(torch.autograd.Function):
    """stride-2 transition conv (16->32, 32->64) with the fused BN-stats
    epilogue; backward = ONE combined MIOpen call (these run once per
    step each — the fwd CK solver + the following BN's stats pass are
    the pool), or with _S2BWD_ENABLED the conv3x3s2_dgrad /
    conv3x3s2_wrw kernels (hip/convs2bwd.h)."""

    @staticmethod
    def forward(ctx, x, weight):
        H_out = x.shape[2] // 2
        grid = x.shape[0] * (H_out // 8) * (weight.shape[0] // 32)
        part = torch.empty(grid, weight.shape[0], 2, device=x.device)
        y = ops._C.conv3x3s2_bn_fwd(x, weight, part)
        ctx.save_for_backward(x, weight)
        ctx.mark_non_differentiable(part)
        ctx.set_materialize_grads(False)
        return y, part

    @staticmethod
    def backward(ctx, dy, _dpart):
        x, weight = ctx.saved_tensors
        dy, tag = _pop_bn_tag(dy)
        need_dx = bool(ctx.needs_input_grad[0])
        if tag is not None:
            # a deferred BN backward landed on the stride-2 conv (no TRF
            # kernel here): materialize dy_conv = A*mask(dz) + B + D*x_bn
            # eagerly (2 transition convs per step) and fill dres
            xbn, z, coefs, relu, dres = tag
            C = dy.shape[1]
            g = dy
            if relu and z is not None:
                g = dy * (z > 0)
            if dres is not None:
                dres.copy_(g)
            A = coefs[0].view(1, C, 1, 1)
            B = coefs[1].view(1, C, 1, 1)
            D = coefs[2].view(1, C, 1, 1)
            dy = (g.float() * A + B + D * xbn.float()).bfloat16() \
                .contiguous(memory_format=_CL)
        if _S2BWD_ENABLED and _kernels_active(dy):
            dx = ops._C.conv3x3s2_dgrad(dy, weight) if need_dx else None
            dw = ops._C.conv3x3s2_wrw(dy, x)
            return dx, dw
        return _lib_backward(dy, x, weight, 2, need_dx, True)


class _Conv3x3Fn(torch.autograd.Function):
    """stock forward; backward with the wrw v1 weight gradient (opt-in
    FEDTORCH_MFMA_WRW, taken only when the fused forward did not apply)"""

    @staticmethod
    def forward(ctx, x, weight):
        y = F.conv2d(x, weight, None, (1, 1), (1, 1))
        ctx.save_for_backward(x, weight)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, weight = ctx.saved_tensors
        dy = dy.contiguous(memory_format=_CL)
        dx = _lib_backward(dy, x, weight, 1, True, False)[0] \
            if ctx.needs_input_grad[0] else None
        dw = ops._C.conv3x3_wrw(dy, x)
        return dx, dw


class _Conv1x1S2Fn(torch.autograd.Function):
    """1x1 stride-2 downsample conv as three library GEMMs over the
    even-subsampled input (the ResNet transition shortcut): MIOpen's CK
    solvers for this shape carry batched-GEMM + wrapper kernels; a plain
    hipBLASLt GEMM over the strided slice is smaller and simpler.
    y[p, co] = sum_ci x_even[p, ci] w[co, ci]."""

    @staticmethod
    def forward(ctx, x, weight):
        N, Ci, H, W = x.shape
        Co = weight.shape[0]
        xe = x[:, :, ::2, ::2].contiguous(memory_format=_CL)
        wm = weight.reshape(Co, Ci)
        # channels_last [N,C,H,W] -> NHWC rows: permute view, flatten
        xr = xe.permute(0, 2, 3, 1).reshape(-1, Ci)
        y = (xr @ wm.t()).reshape(N, H // 2, W // 2, Co) \
            .permute(0, 3, 1, 2).contiguous(memory_format=_CL)
        ctx.save_for_backward(xe, weight)
        ctx.in_shape = (N, Ci, H, W)
        return y

    @staticmethod
    def backward(ctx, dy):
        xe, weight = ctx.saved_tensors
        N, Ci, H, W = ctx.in_shape
        Co = weight.shape[0]
        dy = dy.contiguous(memory_format=_CL)
        dyr = dy.permute(0, 2, 3, 1).reshape(-1, Co)
        dx = None
        if ctx.needs_input_grad[0]:
            dxe = (dyr @ weight.reshape(Co, Ci)) \
                .reshape(N, H // 2, W // 2, Ci).permute(0, 3, 1, 2)
            dx = torch.zeros(N, Ci, H, W, dtype=dy.dtype, device=dy.device
                             ).contiguous(memory_format=_CL)
            dx[:, :, ::2, ::2] = dxe
        xr = xe.permute(0, 2, 3, 1).reshape(-1, Ci)
        dw = (dyr.t() @ xr).reshape(Co, Ci, 1, 1) \
            .contiguous(memory_format=_CL)
        return dx, dw


_CONV1X1_GEMM = os.environ.get('FEDTORCH_CONV1X1_GEMM', '0') == '1'


class NhwcConv1x1S2(nn.Conv2d):
    """Drop-in 1x1/stride-2 bias-free Conv2d (the ResNet downsample
    shortcut).  The GEMM path (default OFF) measured SLOWER in-bench
    (160.0k vs 177.0k flagship): the K=16384 reduction wrw GEMM and the
    strided dx scatter cost more than MIOpen's CK solvers here."""

    def forward(self, x):
        w = self.weight
        use = (_CONV1X1_GEMM
               and self.training and x.is_cuda and x.dim() == 4
               and self.bias is None and self.stride == (2, 2)
               and self.kernel_size == (1, 1)
               and x.dtype == torch.bfloat16
               and x.is_contiguous(memory_format=_CL)
               and not ops.FORCE_EAGER)
        if use:
            wb = w if w.dtype == torch.bfloat16 else w.bfloat16()
            return _Conv1x1S2Fn.apply(x, wb)
        return F.conv2d(x, w, self.bias, self.stride, self.padding,
                        self.dilation, self.groups)


class NhwcConv3x3(nn.Conv2d):
    """Drop-in 3x3/p1 bias-free Conv2d (stride 1 or 2) with the stock
    Conv2d's state_dict layout.  In training, on a bf16 channels_last GPU
    input of a shape `_mfma_stride` accepts, the forward is the MFMA kernel
    with the BN-stats epilogue and the backward is `_Conv3x3BNFn` /
    `_Conv3x3S2BNFn`'s; the eval-mode launch is `conv_bn_act`'s.  Anything
    else is exactly F.conv2d."""

    def forward(self, x):
        w = self.weight
        if self.training and _kernels_active(x):
            stride = _mfma_stride(self, x) if _FWD_ENABLED else 0
            wb = _kernel_weight(w) if stride else None
            if wb is not None:
                fn = _Conv3x3BNFn if stride == 1 else _Conv3x3S2BNFn
                y, part = fn.apply(x, wb)
                y._ft_bn_part = part  # consumed by FusedBatchNorm2d
                return y
            # wrw v1 (opt-in) under the stock forward, on its own conditions
            if (_ENABLED and torch.is_grad_enabled()
                    and w.dtype == torch.bfloat16
                    and w.is_contiguous(memory_format=_CL)
                    and _mfma_stride(self, x, v1_rows=True) == 1):
                return _Conv3x3Fn.apply(x, w)
        return F.conv2d(x, w, self.bias, self.stride, self.padding,
                        self.dilation, self.groups)


def eval_active(x):
    """the eval-mode kernel path applies to this call (the module's own
    `not self.training` is checked by the caller, first)"""
    return (_EVAL_ENABLED and not torch.is_grad_enabled()
            and _kernels_active(x))


def bn_eval_ok(bn):
    """an eval BN the kernels can fold: affine + tracked fp32 buffers"""
    return (bn.affine and bn.track_running_stats
            and bn.running_mean is not None and bn.running_var is not None
            and bn.weight is not None and bn.bias is not None
            and bn.weight.dtype == torch.float32
            and bn.running_mean.dtype == torch.float32)


def conv_bn_act(conv, bn_mod, x, res=None):
    """``bn_mod(conv(x))`` / ``bn_mod(conv(x), res)`` for a conv followed by
    a BNReLU / BNAddReLU.  In eval under no_grad, with an eligible
    NhwcConv3x3 and a FusedBatchNorm2d inside `bn_mod`, the whole group is
    one conv3x3_bn_act_fwd launch; anything else is exactly the two module
    calls."""
    if _EVAL_ENABLED and not conv.training and not bn_mod.training \
            and eval_active(x):
        from fedtorch_amd.ops.batchnorm import (
            BNAddReLU, BNReLU, FusedBatchNorm2d)
        bn = getattr(bn_mod, 'bn', None)
        has_res = isinstance(bn_mod, BNAddReLU)
        stride = 0
        if (isinstance(conv, NhwcConv3x3) and isinstance(bn, FusedBatchNorm2d)
                and (has_res or isinstance(bn_mod, BNReLU))
                and has_res == (res is not None) and bn_eval_ok(bn)
                and (res is None or res.dtype == torch.bfloat16)):
            stride = _mfma_stride(conv, x)
        wb = _kernel_weight(conv.weight) if stride else None
        if wb is not None:
            rc = res.contiguous(memory_format=_CL) if has_res \
                else _empty(x.device)
            return ops._C.conv3x3_bn_act_fwd(
                x, wb, bn.weight, bn.bias, bn.running_mean,
                bn.running_var, float(bn.eps), True, rc, stride)
    y = conv(x)
    return bn_mod(y) if res is None else bn_mod(y, res)
