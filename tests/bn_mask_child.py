# -*- coding: utf-8 -*-
"""Child process of test_gpu_batchnorm.py::test_bn_fwd_mask_child_process.
FT_BNH_MASK=1 (read once per process by bn_fwd_train) makes the bf16
channels_last forward return the ReLU bitmask: N*H*W*C/8 bytes, bit (e & 7)
of byte (e >> 3) set where output element e (flat NHWC index) is > 0.
Checks the mask against the packed y > 0 and bn_bwd with the mask against
bn_bwd with y.  Exit status 0 = all checks passed."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

import fedtorch_amd.ops as ops  # noqa: E402

import bn_cases as bc  # noqa: E402

DEV = 'cuda'
CL = torch.channels_last
FLAGS = (True, True, True, True)
# one channel group, the body's 64 channels over a ragged row count, and
# C = 256 (32 groups)
CASES = (('cl', 'bf16', 8, 1, 1, 257), ('cl', 'bf16', 64, 3, 5, 7),
         ('cl', 'bf16', 256, 4, 16, 16))


def act(t):
    return t.bfloat16().to(DEV).contiguous(memory_format=CL)


def f32(t):
    return t.float().to(DEV)


def main():
    assert os.environ.get('FT_BNH_MASK') == '1'
    for case in CASES:
        i, r, _E = bc.fwd_case(case, FLAGS)
        x = act(i['x'])
        y, sm, siv, mask = ops._C.bn_fwd_train(
            x, f32(i['w']), f32(i['b']), f32(i['rm0']), f32(i['rv0']),
            i['eps'], i['mom'], True, act(i['res']))
        where = 'mask %s' % bc.case_id(case)
        assert mask.dtype == torch.uint8 and mask.dim() == 1, where
        assert mask.numel() * 8 == x.numel(), '%s: %d bytes' % (
            where, mask.numel())
        yc = y.float().cpu()
        want = bc.pack_mask(yc)
        assert torch.equal(mask.cpu(), want), '%s != packed y > 0' % where
        # the reference decides every sign with margin (asserted by the
        # case), so the mask is also the reference's
        assert torch.equal(want, bc.pack_mask(r['f'])), where + ' vs f64'
        assert 0 < (yc > 0).sum().item() < yc.numel()
        b = bc.bwd_inputs(case)
        dy = act(b['dy'])
        with_y = ops._C.bn_bwd(dy, x, y, torch.empty(0, device=DEV,
                                                     dtype=torch.uint8),
                               sm, siv, f32(i['w']), True, True)
        with_m = ops._C.bn_bwd(dy, x, torch.empty(0, device=DEV), mask, sm,
                               siv, f32(i['w']), True, True)
        for k, (u, v) in enumerate(zip(with_y, with_m)):
            assert torch.isfinite(u.float()).all().item(), where
            assert torch.equal(u.cpu(), v.cpu()), \
                '%s: bn_bwd output %d differs between y and mask' % (where, k)
        print('%s ok (%d bytes)' % (where, mask.numel()))
    torch.cuda.synchronize()


if __name__ == '__main__':
    main()
