# -*- coding: utf-8 -*-
"""Case generators and float64 references for the classifier-tail kernels
(hip/head.h), shared by tests/test_gpu_head.py (GPU) and
tests/test_head_cpu.py (no GPU).  Imports torch only.

References, written out from the formulas in float64:

  head_fwd   pooled[n,c] = sum_hw x[n,c,h,w] / HW
             logits[n,k] = sum_c pooled[n,c] w[k,c] + b[k]
  head_bwd   dx[n,c,h,w] = sum_k dl[n,k] w[k,c] / HW   (same for every pixel)
             dw[k,c] = sum_n dl[n,k] pooled[n,c],  db[k] = sum_n dl[n,k]
  ce_topk    per sample, from the STORED logit values z (bf16 values are
             widened first) and the target t:
               loss = log(sum_j exp(z_j - max z)) - (z_t - max z)
               rank = #{j : z_j > z_t} + #{j < t : z_j == z_t}
               top-k hit iff rank < k
             a target outside [0, K) skips the sample entirely.

Exact cases use small integers (and eighths for dlogits) with a power-of-two
H*W, so every sum the kernels can form, in any order, is an fp32 number; the
builders assert that before they return, so building all cases without a GPU
proves the reference alone meets the precondition.

Tolerances of the random companions: an fp32 sum of L terms, in any order,
with or without fma, is within (L - 1) u sum|terms| of the exact sum to first
order; the test allows (L + 2) u sum|terms|, with sum|terms| in float64.
  pooled   L = HW   (HW - 1 adds and one division)
  logits   L = HW + C + 1   (the pooled chain, C products, C adds with bias)
  dx       L = K + 1        (K products/adds and one division)
  dw       L = N            db: L = N
and half an ulp of the output dtype where the kernel rounds to bf16.

Loss bound (per sample, summed over the batch): (2K + 32) u max(1, loss_i),
from <= 2 ulp each for expf and logf, a K-term fp32 sum and the roundings of
z - max and of the final subtraction."""
import zlib
from types import SimpleNamespace

import torch
import torch.nn as nn

F64 = torch.float64
EXACT = float(2 ** 24)      # integers below this are exact in fp32
U = 2.0 ** -24              # fp32 unit roundoff
DTYPES = {'bf16': torch.bfloat16, 'fp32': torch.float32}

# (N, C, H, W, K)
FWD_EXACT_FULL = [(1, 8, 1, 1, 1), (3, 16, 2, 2, 5), (3, 64, 8, 8, 10)]
FWD_EXACT_REST = [(2, 256, 4, 4, 62), (1, 1024, 2, 2, 100),
                  (5, 64, 8, 8, 1000)]
FWD_RANDOM = [(2, 24, 5, 7, 7), (3, 64, 8, 8, 10)]
BWD_N = [1, 3, 64, 257]
# (C, H, W, K) of the backward cases; N comes from BWD_N
BWD_SHAPES = [(64, 8, 8, 10), (24, 2, 2, 7)]
CE_K = [1, 5, 10, 62, 1000]
CE_N = [1, 3, 64, 257]
CE_DIST = [(1.0, 0.0), (4.0, 0.0), (4.0, 100.0)]


def gen(*key):
    """CPU generator seeded by the case's name (stable across runs)"""
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


def ints(g, lo, hi, *shape):
    """float64 tensor of uniform integers in [lo, hi]"""
    return torch.randint(lo, hi + 1, shape, generator=g).to(F64)


def is_pow2(n):
    return n >= 1 and (n & (n - 1)) == 0


def fp32_exact(t):
    """every entry of the float64 tensor is an fp32 number"""
    return torch.equal(t.float().double(), t)


def bf16_exact(t):
    return torch.equal(t.bfloat16().double(), t)


def half_ulp(v64, dtype):
    """half an ulp of `dtype` in the binade of |v| (0 for fp32 outputs: the
    fp32 rounding is inside the (L + 2) u bound)"""
    if dtype == torch.float32:
        return torch.zeros_like(v64)
    _m, e = torch.frexp(v64.abs())          # |v| = m * 2^e, m in [0.5, 1)
    return torch.where(v64 == 0, torch.zeros_like(v64),
                       torch.ldexp(torch.ones_like(v64), e - 9))


# --------------------------------------------------------------------------
# float64 references
# --------------------------------------------------------------------------
def ref_fwd(x, w, b):
    """x [N,C,H,W], w [K,C], b [K] or None, all float64"""
    pooled = x.sum(dim=(2, 3)) / (x.size(2) * x.size(3))
    logits = pooled @ w.t()
    if b is not None:
        logits = logits + b
    return logits, pooled


def ref_bwd(dl, pooled, w, H, W):
    """-> dx [N,C,H,W], dw [K,C], db [K] (float64)"""
    g = (dl @ w) / (H * W)
    dx = g[:, :, None, None].expand(-1, -1, H, W)
    return dx, dl.t() @ pooled, dl.sum(dim=0)


def ref_metrics_per_sample(z, t):
    """z: [N, K] of any float dtype (its stored values are used), t: int64
    [N] -> (loss [N] float64, rank [N] int64, valid [N] bool)"""
    z = z.detach().cpu().to(F64)
    t = t.detach().cpu()
    K = z.size(1)
    valid = (t >= 0) & (t < K)
    tc = t.clamp(0, K - 1).view(-1, 1)
    m = z.max(dim=1, keepdim=True).values
    zt = z.gather(1, tc)
    loss = torch.log(torch.exp(z - m).sum(dim=1)) - (zt - m).squeeze(1)
    j = torch.arange(K).view(1, -1)
    rank = ((z > zt) | ((z == zt) & (j < tc))).sum(dim=1)
    return loss, rank, valid


def ref_metrics(z, t):
    """-> (loss_sum float, top1 int, top5 int, n int, loss_bound float)"""
    loss, rank, valid = ref_metrics_per_sample(z, t)
    K = z.size(1)
    lv = loss[valid]
    bound = ((2 * K + 32) * U * lv.clamp(min=1.0)).sum().item()
    return (lv.sum().item(), int(((rank < 1) & valid).sum()),
            int(((rank < 5) & valid).sum()), int(valid.sum()), bound)


def tie_free(z, t):
    """no valid sample's target logit equals another logit of its row"""
    z = z.detach().cpu().to(F64)
    t = t.detach().cpu()
    K = z.size(1)
    valid = (t >= 0) & (t < K)
    zt = z.gather(1, t.clamp(0, K - 1).view(-1, 1))
    return bool((((z == zt).sum(dim=1) == 1) | ~valid).all())


# --------------------------------------------------------------------------
# forward cases
# --------------------------------------------------------------------------
def fwd_exact_case(shape, bias=True):
    """integer x in [-4, 4], w in [-3, 3], b in [-3, 3], power-of-two HW"""
    N, C, H, W, K = shape
    g = gen('fwd_exact', shape, bias)
    x = ints(g, -4, 4, N, C, H, W)
    w = ints(g, -3, 3, K, C)
    b = ints(g, -3, 3, K) if bias else None
    HW = H * W
    assert is_pow2(HW)
    # every partial sum of the pool is an integer below 2^24, the pooled
    # values and the products are multiples of 1/HW below 2^24 / HW
    assert x.abs().sum(dim=(2, 3)).max().item() < EXACT
    logits, pooled = ref_fwd(x, w, b)
    absum = (pooled.abs() @ w.abs().t()).max().item() + 3.0
    assert absum * HW < EXACT
    assert bf16_exact(x) and bf16_exact(w) and (b is None or bf16_exact(b))
    assert fp32_exact(pooled) and fp32_exact(logits)
    return x, w, b, logits, pooled


def fwd_random_case(shape, xdt, wdt, bdt):
    """randn inputs rounded to their dtypes first, so the reference reads
    the same values as the kernel; -> x, w, b, logits, pooled, tol_logits,
    tol_pooled (float64)"""
    N, C, H, W, K = shape
    g = gen('fwd_random', shape)
    x = torch.randn(N, C, H, W, generator=g).to(xdt).to(F64)
    w = (torch.randn(K, C, generator=g) * 0.5).to(wdt).to(F64)
    b = torch.randn(K, generator=g).to(bdt).to(F64)
    logits, pooled = ref_fwd(x, w, b)
    HW = H * W
    ap = x.abs().sum(dim=(2, 3)) / HW
    tol_p = (HW + 2) * U * ap
    tol_l = (HW + C + 1 + 2) * U * (ap @ w.abs().t() + b.abs())
    return x, w, b, logits, pooled, tol_l, tol_p


def to_dev(x64, dtype, device, channels_last=False):
    t = x64.to(dtype).to(device)
    if channels_last:
        t = t.contiguous(memory_format=torch.channels_last)
    return t


# --------------------------------------------------------------------------
# backward cases
# --------------------------------------------------------------------------
def bwd_exact_case(N, shape):
    """dlogits from {-2..2}/8, pooled from an exact forward, integer w"""
    C, H, W, K = shape
    g = gen('bwd_exact', N, shape)
    x, w, b, _logits, pooled = fwd_exact_case((N, C, H, W, K))
    dl = ints(g, -2, 2, N, K) / 8
    HW = H * W
    # dx: multiples of 1/(8 HW); dw: multiples of 1/(8 HW); db: of 1/8
    assert (dl.abs() @ w.abs()).max().item() * 8 * HW < EXACT
    assert (dl.abs().t() @ pooled.abs()).max().item() * 8 * HW < EXACT
    assert dl.abs().sum(dim=0).max().item() * 8 < EXACT
    dx, dw, db = ref_bwd(dl, pooled, w, H, W)
    assert fp32_exact(dx) and fp32_exact(dw) and fp32_exact(db)
    return dl, pooled, w, b, dx, dw, db


def bwd_random_case(N, shape, wdt):
    C, H, W, K = shape
    g = gen('bwd_random', N, shape)
    dl = (torch.randn(N, K, generator=g) * 0.1).float().to(F64)
    pooled = torch.randn(N, C, generator=g).float().to(F64)
    w = (torch.randn(K, C, generator=g) * 0.5).to(wdt).to(F64)
    dx, dw, db = ref_bwd(dl, pooled, w, H, W)
    HW = H * W
    tol_dx = ((K + 1 + 2) * U * (dl.abs() @ w.abs()) / HW)[
        :, :, None, None].expand(-1, -1, H, W)
    tol_dw = (N + 2) * U * (dl.abs().t() @ pooled.abs())
    tol_db = (N + 2) * U * dl.abs().sum(dim=0)
    return dl, pooled, w, dx, dw, db, tol_dx, tol_dw, tol_db


# --------------------------------------------------------------------------
# metric cases
# --------------------------------------------------------------------------
def metric_case(K, N, s, o, dtype):
    """logits randn * s + o rounded to `dtype`, uniform targets"""
    g = gen('metric', K, N, s, o, str(dtype))
    z = (torch.randn(N, K, generator=g) * s + o).to(dtype)
    t = torch.randint(0, K, (N,), generator=g)
    return z, t


def tie_row_case(K=10):
    """every class with all-equal logits: rank == t, so top-1 iff t == 0
    and top-5 iff t < 5"""
    z = torch.full((K, K), 1.5)
    return z, torch.arange(K)


def mixed_target_case(K=10, N=9):
    """valid targets with ignore_index / out-of-range ones in between"""
    z, t = metric_case(K, N, 1.0, 0.0, torch.float32)
    t[1], t[4], t[7] = -100, K, -1
    return z, t


# --------------------------------------------------------------------------
# validation-pass pieces
# --------------------------------------------------------------------------
class TinyMLP(nn.Module):
    """fp32 classifier without BatchNorm; `noise` as the framework's MLP"""

    def __init__(self, d_in=12, hidden=16, num_classes=10):
        super().__init__()
        self.noise = None
        self.num_classes = num_classes
        self.body = nn.Sequential(nn.Linear(d_in, hidden), nn.Tanh(),
                                  nn.Linear(hidden, num_classes))

    def forward(self, x):
        return self.body(x.reshape(x.size(0), -1))


def val_setup(on_cuda, d_in=12, num_classes=10, sizes=(8, 8, 5, 1)):
    """seeded model, the list loader (batches of `sizes`) and args"""
    torch.manual_seed(11)
    model = TinyMLP(d_in, 16, num_classes)
    g = gen('val_loader', d_in, num_classes, sizes)
    loader = [(torch.randn(n, d_in, generator=g),
               torch.randint(0, num_classes, (n,), generator=g))
              for n in sizes]
    args = SimpleNamespace(arch='mlp', data='synthetic',
                           graph=SimpleNamespace(on_cuda=on_cuda),
                           channels_last=False)
    if on_cuda:
        model = model.cuda()
    return model, loader, args
