"""`fused_conv` on CombineCLIPVisualV4 (encoders.py): the seven 3x3 convolutions as ops.conv3x3 launches with `multiply_fusion_1..3` in
their epilogues and amax_out chained, against the float64 evaluation of the same module; the torch GPU run of the same module
(`fused_conv=False`) is the yardstick: e_fused <= 8 e_torch, relative L2 and worst element.  The fusion on its own: synthetic stage
maps, visual map and text vector - no producer, no ViT.  Channel counts the kernel takes: 64 -> 64, 64 + 32 -> 64 three times, 64 -> 64."""
import copy

import numpy as np
import pytest
import torch

from tests import conv3x3_ref as R
from thesis_clip_nerf_amd import encoders as E
from thesis_clip_nerf_amd import ops

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
HALF = (16, 24)
TINY_FUSION = dict(clip_channels=(16, 32, 32, 64), text_dim=64, widths=(64, 32, 32), up3_filters=16)      # as tests/test_feature_fusion_cpu.py
FUSABLE = dict(clip_channels=(32, 32, 32, 64), text_dim=64, widths=(64, 64, 64), up3_filters=64)


def fusion(fused_conv, **kw):
    torch.manual_seed(7)
    kw = {**FUSABLE, **kw}
    return E.CombineCLIPVisualV4(use_dense=True, activation='elu', half_size=HALF, visual_channels=32, fused_tail=False, fused_conv=fused_conv,
                                 **kw)


def inputs(channels=(32, 32, 32, 64), n=2):
    g = torch.Generator().manual_seed(8)
    r = lambda *s: torch.randn(*s, generator=g)
    c1, c2, c3, c4 = channels
    clip = (r(n, 64), r(n, c1, 7, 9), r(n, c2, 5, 5), r(n, c3, 3, 4), r(n, c4, 2, 2))
    return clip, r(n, 32, *HALF), r(n, 64)


def to(x, device=None, dtype=None):
    if isinstance(x, tuple):
        return tuple(to(t, device, dtype) for t in x)
    return x.to(device=device, dtype=dtype)


@pytest.fixture
def calls(monkeypatch):
    """Counts the mvnerf_conv3x3_nhwc launches (every one goes through ops.conv3x3)."""
    seen = []
    real = ops.conv3x3

    def counted(*args, **kw):
        seen.append(args[3])
        return real(*args, **kw)
    monkeypatch.setattr(ops, 'conv3x3', counted)
    return seen


def test_fused_conv_against_the_float64_module(calls):
    clip, visual, text = inputs()
    mod = fusion(False)
    with torch.no_grad():
        ref = copy.deepcopy(mod).double()(to(clip, dtype=torch.float64), visual.double(), text.double()).numpy()
        mod = mod.to(DEV)
        args = (to(clip, DEV), visual.to(DEV), text.to(DEV))
        plain = mod(*args).cpu().numpy()
        assert not calls
        mod.fused_conv = True
        fused = mod(*args)
        assert len(calls) == 7 and fused.shape == (2, 256, 2 * HALF[0], 2 * HALF[1])
        again = mod(*args)
    assert torch.equal(fused, again)
    e_t, e_f = R.errors(plain, ref), R.errors(fused.cpu().numpy(), ref)
    print(f'fused_conv: rel L2 {e_f[0]:.3g} = {e_f[0] / e_t[0]:.2f} x torch ({e_t[0]:.3g}), worst {e_f[1]:.3g} = {e_f[1] / e_t[1]:.2f} x torch ({e_t[1]:.3g})')
    assert e_f[0] <= R.BAR * e_t[0] and e_f[1] <= R.BAR * e_t[1], (e_f, e_t)


def test_auto_with_a_gradient_runs_torch_and_backpropagates(calls):
    clip, visual, text = inputs()
    mod = fusion('auto').to(DEV)                                  # its parameters require a gradient
    out = mod(to(clip, DEV), visual.to(DEV), text.to(DEV))
    out.square().mean().backward()
    assert not calls and all(p.grad is not None and p.grad.abs().sum() > 0 for p in mod.parameters())
    with torch.no_grad():
        fused = mod(to(clip, DEV), visual.to(DEV), text.to(DEV))
    assert len(calls) == 7 and R.rel_l2(fused.cpu().numpy(), out.detach().cpu().numpy()) < 1e-5
    mod.fused_conv = True
    with pytest.raises(RuntimeError, match='no backward'):
        mod(to(clip, DEV), visual.to(DEV), text.to(DEV))


def test_rejected_channel_counts_run_torch_under_auto_and_raise_under_true(calls):
    """TINY_FUSION: 64 + 32 -> 32, 32 -> 32, 32 + 32 -> 32, 32 + 16 -> 16, 16 -> 16 are not the kernel's; only its first convolution
    (64 -> 64) is."""
    clip, visual, text = inputs((16, 32, 32, 64))
    args = (to(clip, DEV), visual.to(DEV), text.to(DEV))
    mod = fusion(False, **TINY_FUSION).to(DEV)
    with torch.no_grad():
        plain = mod(*args)
        mod.fused_conv = 'auto'
        auto = mod(*args)
        assert calls == [64] and R.rel_l2(auto.cpu().numpy(), plain.cpu().numpy()) < 1e-5
        mod.fused_conv = True
        with pytest.raises(ValueError, match='not one the HIP pass takes'):
            mod(*args)


def test_a_weight_changed_in_place_is_packed_again(calls):
    clip, visual, text = inputs()
    args = (to(clip, DEV), visual.to(DEV), text.to(DEV))
    mod = fusion(True).to(DEV)
    with torch.no_grad():
        first = mod(*args)
        packed = mod.conv._mvnerf_packed[1]
        assert mod(*args) is not None and mod.conv._mvnerf_packed[1] is packed            # cached per parameter version
        mod.conv.weight.mul_(-1.5)
        mod.up_3.double_conv.conv_2.weight.add_(0.01)
        second = mod(*args)
        assert mod.conv._mvnerf_packed[1] is not packed and not torch.equal(first, second)
        mod.fused_conv = False
        plain = mod(*args)
    assert R.rel_l2(second.cpu().numpy(), plain.cpu().numpy()) < 1e-5
    assert len(calls) == 21
