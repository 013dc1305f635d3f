"""mvnerf_fuse_upsample2x_bwd without a GPU: every rejected argument returns its error before any launch; the checks of
ops.fuse_upsample2x_bwd; the `fused_backward` switch of the two combine modules."""
import ctypes

import pytest
import torch

from thesis_clip_nerf_amd import _lib, encoders as E, ops


def test_argument_checks_come_before_any_launch():
    lib = _lib.lib()
    one, odd = ctypes.c_void_p(256), ctypes.c_void_p(260)
    base = dict(g=one, a=one, b=one, weight=one, N=1, h=4, w=4, Ca=16, Cb=16, act=0, da=one, db=one, g_low=one, stream=None)
    call = lambda **kw: lib.mvnerf_fuse_upsample2x_bwd(*{**base, **kw}.values())
    assert call(g=None) == -1 and b'null pointer (g)' in lib.mvnerf_last_error()
    assert call(weight=None) == -1 and b'null pointer (weight)' in lib.mvnerf_last_error()
    assert call(da=None, db=None, g_low=None) == -1 and b'no output wanted' in lib.mvnerf_last_error()
    assert call(N=0) == -1 and call(h=0) == -1 and call(w=0) == -1 and call(N=-1) == -1 and call(h=-3) == -1 and call(w=-2) == -1
    assert call(Ca=24) == -2 and b'Ca=24' in lib.mvnerf_last_error()
    assert call(Ca=0) == -2 and call(Cb=8) == -2 and call(Cb=40) == -2 and b'Cb=40' in lib.mvnerf_last_error()
    assert call(Ca=256, Cb=272) == -2 and b'Ca+Cb=528' in lib.mvnerf_last_error()
    assert call(act=3) == -2 and b'act=3' in lib.mvnerf_last_error() and call(act=-1) == -2
    for name in ('g', 'a', 'b', 'weight', 'da', 'db', 'g_low'):
        assert call(**{name: odd}) == -3 and f'{name} must be 16-byte aligned'.encode() in lib.mvnerf_last_error(), name
    # act' reads the input of every half it differentiates; the identity reads neither
    assert call(act=1, a=None) == -1 and b'null pointer (a)' in lib.mvnerf_last_error()
    assert call(act=2, b=None) == -1 and b'null pointer (b)' in lib.mvnerf_last_error()
    assert lib.mvnerf_abi_version() == 1


def test_ops_wrapper_checks():
    g, a, b, wt = torch.zeros(1, 8, 8, 256), torch.zeros(1, 4, 4, 16), torch.zeros(1, 4, 4, 16), torch.zeros(32, 256)
    with pytest.raises(ValueError, match='HIP device'):
        ops.fuse_upsample2x_bwd(g, a, b, wt, None)
    with pytest.raises(ValueError, match='expected a torch.Tensor'):
        ops.fuse_upsample2x_bwd(g, None, b, wt, None)


def test_fused_backward_switch_validation():
    v0 = E.CombineCLIPVisualV0((8, 8))
    v4 = E.CombineCLIPVisualV4(use_dense=True, activation='elu', half_size=(8, 8), clip_channels=(16, 32, 64, 128), text_dim=32,
                               widths=(64, 32, 16), up3_filters=16, visual_channels=16)
    for module in (v0, v4):
        assert module.fused_backward is False
        module.fused_backward = True
        assert module.fused_backward is True
        for bad in ('auto', 1, 0, None, 'yes'):
            with pytest.raises(ValueError, match='fused_backward'):
                module.fused_backward = bad
    with pytest.raises(ValueError, match='fused_backward'):
        E.CombineCLIPVisualV0((8, 8), fused_backward='auto')
    with pytest.raises(ValueError, match='fused_backward'):
        E.CombineCLIPVisualV4(half_size=(8, 8), fused_backward='auto')
    assert E.CombineCLIPVisualV0((8, 8), fused_tail='auto', fused_backward=True).fused_backward is True
    assert E.FeatureProducer((32, 48)).combine_clip_visual.fused_backward is False


def test_on_the_cpu_the_switch_changes_nothing():
    """No GPU tensor in the call: 'auto' stays torch with or without `fused_backward`, the same bits and gradients; fused_tail=True
    keeps its "no backward" error; a bad `fused_tail` keeps its message."""
    torch.manual_seed(5)
    tail = E.CombineCLIPVisualV0((4, 6), 16, 16, fused_tail='auto')
    clip, vis = torch.randn(1, 16, 7, 7), torch.randn(1, 16, 4, 6, requires_grad=True)
    out = tail(clip, vis)
    out.square().mean().backward()
    want = (out.detach().clone(), vis.grad.clone(), tail.conv.weight.grad.clone())
    vis.grad = None
    tail.zero_grad()
    tail.fused_backward = True
    out = tail(clip, vis)
    out.square().mean().backward()
    assert torch.equal(out, want[0]) and torch.equal(vis.grad, want[1]) and torch.equal(tail.conv.weight.grad, want[2])
    for switch in (False, True):
        tail.fused_backward = switch
        tail.fused_tail = True
        with pytest.raises(RuntimeError, match='no backward'):
            tail(clip, vis)
        tail.fused_tail = 'sometimes'
        with pytest.raises(ValueError, match="fused_tail: 'sometimes'"):
            tail(clip, vis)
        tail.fused_tail = 'auto'
