# -*- coding: utf-8 -*-
"""FEDTORCH_MFMA_S2_BWD is opt-in and inert off the GPU: on CPU tensors the
stride-2 NhwcConv3x3 stays stock Conv2d whatever the flag says."""
import torch
import torch.nn as nn

from fedtorch_amd.ops import conv3x3 as c3


def test_s2_bwd_flag_defaults_off():
    assert hasattr(c3, '_S2BWD_ENABLED')
    assert c3._S2BWD_ENABLED is False


def test_s2_bwd_flag_is_inert_on_cpu():
    old = c3._S2BWD_ENABLED
    c3._S2BWD_ENABLED = True
    try:
        for Ci, Wi in ((16, 32), (32, 16)):
            torch.manual_seed(5)
            m = c3.NhwcConv3x3(Ci, 2 * Ci, 3, stride=2, padding=1,
                               bias=False).to(memory_format=c3._CL)
            ref = nn.Conv2d(Ci, 2 * Ci, 3, stride=2, padding=1,
                            bias=False).to(memory_format=c3._CL)
            ref.load_state_dict(m.state_dict())
            m.train()
            ref.train()
            x = torch.randn(2, Ci, Wi, Wi).to(memory_format=c3._CL)
            xa = x.clone().requires_grad_(True)
            xb = x.clone().requires_grad_(True)
            ya, yb = m(xa), ref(xb)
            ya.square().mean().backward()
            yb.square().mean().backward()
            assert torch.equal(ya, yb)
            assert torch.equal(xa.grad, xb.grad)
            assert torch.equal(m.weight.grad, ref.weight.grad)
    finally:
        c3._S2BWD_ENABLED = old
