"""`fused_vit` on TransformerBlock / VisionTransformer / VisionTransformerEncoder / VisualFeatures / LanguageFeatureProducer
(encoders.py): each transformer block as seven HIP launches - ops.bn_apply (running statistics), ops.linear (q, k, v at once),
ops.attention, ops.linear (+ inputs), ops.layer_norm, ops.linear (gelu), ops.linear (+ inputs) - against the float64 evaluation of the
same module; the torch GPU run of the same module is the yardstick: e_fused <= 8 e_torch, relative L2 and worst element.  Sizes are the
smallest the kernels take: embed 64 with 4 heads of 16, 36 and 25 tokens (72 and 75 rows: two row tiles of 32 and a partial third)."""
import copy
import hashlib

import pytest
import torch

from tests import conv3x3_ref as R
from thesis_clip_nerf_amd import encoders as E
from thesis_clip_nerf_amd import ops

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
SIZE = (32, 48)
VIT64 = dict(transformer_image_size=(32, 48), patch_size=8, embed_dim=64, num_heads=4, hooks=(1, 2, 3, 4), features=(32, 64, 96, 128))
TINY_VIT = dict(transformer_image_size=(32, 32), patch_size=16, embed_dim=32, num_heads=4, hooks=(1, 2, 3, 4), features=(32, 64, 96, 128))
TINY_FUSION = dict(clip_channels=(16, 32, 32, 64), text_dim=64, widths=(64, 32, 32), up3_filters=16)
NAMES = ('conv3x3', 'bn_finalize', 'bn_apply', 'linear', 'attention', 'layer_norm')
BLOCK = {'conv3x3': 0, 'bn_finalize': 0, 'bn_apply': 1, 'linear': 4, 'attention': 1, 'layer_norm': 1}      # 7 launches


# under 'auto' the passes measured slower than torch at the reference's shape stay torch (encoders.VIT_AUTO_TORCH_PASSES)
AUTO_BLOCK = {**BLOCK, 'linear': sum(p.startswith('linear') and p not in E.VIT_AUTO_TORCH_PASSES for p in E.VIT_PASSES),
              'attention': int('attention' not in E.VIT_AUTO_TORCH_PASSES), 'layer_norm': int('layer_norm' not in E.VIT_AUTO_TORCH_PASSES)}


def blocks(k, per_block=BLOCK, **more):
    return {name: k * per_block[name] + more.get(name, 0) for name in NAMES}


@pytest.fixture
def calls(monkeypatch):
    """Counts the launches by wrapper."""
    seen = dict.fromkeys(NAMES, 0)
    for name in seen:
        def counted(*args, _real=getattr(ops, name), _name=name, **kw):
            seen[_name] += 1
            return _real(*args, **kw)
        monkeypatch.setattr(ops, name, counted)
    return seen


def randomise(module, seed=9):
    """gamma and beta away from Keras' 1 and 0, running statistics away from 0 and 1, biases away from 0: the defaults would hide a dropped
    bias, a wrong gamma or batch statistics in place of the running ones."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for m in module.modules():
            if isinstance(m, (torch.nn.BatchNorm2d, torch.nn.BatchNorm1d, torch.nn.LayerNorm)):
                m.weight.copy_(1 + 0.3 * torch.randn(m.weight.shape, generator=g))
                m.bias.copy_(0.3 * torch.randn(m.bias.shape, generator=g))
                if isinstance(m, torch.nn.BatchNorm1d):
                    m.running_mean.copy_(0.3 * torch.randn(m.running_mean.shape, generator=g))
                    m.running_var.copy_(0.5 + torch.rand(m.running_var.shape, generator=g))
            elif isinstance(m, (torch.nn.Conv2d, torch.nn.Linear)) and m.bias is not None:
                m.bias.copy_(0.2 * torch.randn(m.bias.shape, generator=g))
    return module


def deterministic_torch():
    """torch's own switch for the parts that stay torch (tests/test_gpu_fused_visual.py has the reason)."""
    return torch.backends.cudnn.flags(enabled=True, benchmark=False, deterministic=True)


def as_list(out):
    return list(out) if isinstance(out, (list, tuple)) else [out]


def check(module, x, calls, expected, **switches):
    """float64 on the CPU, torch float32 on the GPU, fused on the GPU -> the two error pairs, per output."""
    module = randomise(module).requires_grad_(False).eval()
    with torch.no_grad():
        ref = [t.numpy() for t in as_list(copy.deepcopy(module).double()(x.double()))]
        module = module.to(DEV)
        xd = x.to(DEV)
        with deterministic_torch():
            plain = [t.cpu().numpy() for t in as_list(module(xd))]
            assert not any(calls.values())
            for name, value in switches.items():
                setattr(module, name, value)
            fused = as_list(module(xd))
            assert calls == expected, calls
            again = as_list(module(xd))
    for i, (f, a, p, r) in enumerate(zip(fused, again, plain, ref)):
        assert f.shape == r.shape and torch.equal(f, a)                          # deterministic
        e_t, e_f = R.errors(p, r), R.errors(f.cpu().numpy(), r)
        print(f'{type(module).__name__}[{i}] {switches}: rel L2 {e_f[0]:.3g} = {e_f[0] / e_t[0]:.2f} x torch ({e_t[0]:.3g}), '
              f'worst {e_f[1]:.3g} = {e_f[1] / e_t[1]:.2f} x torch ({e_t[1]:.3g})')
        assert e_f[0] <= R.BAR * e_t[0] and e_f[1] <= R.BAR * e_t[1], (e_f, e_t)


def images(n):
    return torch.rand(n, *SIZE, 3, generator=torch.Generator().manual_seed(8))


def test_transformer_block_against_the_float64_module(calls):
    torch.manual_seed(7)
    x = torch.randn(2, 36, 64, generator=torch.Generator().manual_seed(3))
    check(E.TransformerBlock(4, 64), x, calls, blocks(1), fused_vit=True)


def test_transformer_block_under_auto_against_the_float64_module(calls):
    """'auto' mixes HIP and torch passes inside the block; an amax word is handed on only between two HIP passes."""
    assert set(E.VIT_AUTO_TORCH_PASSES) <= set(E.VIT_PASSES)
    torch.manual_seed(7)
    x = torch.randn(2, 36, 64, generator=torch.Generator().manual_seed(3))
    check(E.TransformerBlock(4, 64), x, calls, blocks(1, AUTO_BLOCK), fused_vit='auto')


def test_vision_transformer_against_the_float64_module(calls):
    torch.manual_seed(7)
    vit = E.VisionTransformer(img_size=(40, 56), patch_size=8, embed_dim=64, num_heads=4, hooks=(1, 2, 3, 4))
    x = torch.rand(2, 3, 40, 56, generator=torch.Generator().manual_seed(4))
    check(vit, x, calls, blocks(4), fused_vit=True)


@pytest.mark.parametrize('with_conv', [False, True], ids=['vit', 'vit_and_conv'])
def test_visual_features_against_the_float64_module(calls, with_conv):
    torch.manual_seed(7)
    expected = blocks(4, conv3x3=12, bn_finalize=6, bn_apply=6) if with_conv else blocks(4)
    switches = dict(fused_vit=True, fused_conv=True) if with_conv else dict(fused_vit=True)
    check(E.VisualFeatures(256, SIZE, **VIT64), images(3), calls, expected, **switches)


def test_fallbacks_auto_runs_torch_and_true_raises(calls):
    torch.manual_seed(7)
    x = torch.randn(2, 36, 64, device=DEV)
    blk = randomise(E.TransformerBlock(4, 64, fused_vit='auto')).to(DEV).eval()          # its parameters require a gradient
    out = blk(x)
    out.square().mean().backward()
    assert not any(calls.values()) and blk.dense_0.weight.grad is not None
    with torch.no_grad():
        fused = blk(x)
    assert calls == blocks(1, AUTO_BLOCK) and R.rel_l2(fused.cpu().numpy(), out.detach().cpu().numpy()) < 1e-5
    blk.fused_vit = True
    with pytest.raises(RuntimeError, match='no backward'):
        blk(x)
    blk.requires_grad_(False).train()                                                    # batch statistics, running ones updated: torch
    before = blk.layer_norm_1.running_mean.clone()
    with pytest.raises(ValueError, match='training mode'):
        blk(x)
    blk.fused_vit = 'auto'
    blk(x)
    assert calls == blocks(1, AUTO_BLOCK) and not torch.equal(blk.layer_norm_1.running_mean, before)
    small = E.TransformerBlock(4, 32, fused_vit='auto').to(DEV).requires_grad_(False).eval()      # embed 32, d = 8
    small(torch.randn(2, 5, 32, device=DEV))
    assert calls == blocks(1, AUTO_BLOCK)
    small.fused_vit = True
    with pytest.raises(ValueError, match='multiples of 64'):
        small(torch.randn(2, 5, 32, device=DEV))


def test_packed_weights_follow_a_parameter_update(calls):
    torch.manual_seed(7)
    blk = randomise(E.TransformerBlock(4, 64, fused_vit=True)).to(DEV).requires_grad_(False).eval()
    x = torch.randn(1, 9, 64, device=DEV)
    first = blk(x)
    packed = blk.dense_1.__dict__['_mvnerf_packed'][1]
    assert torch.equal(blk(x), first) and blk.dense_1.__dict__['_mvnerf_packed'][1] is packed         # cached
    with torch.no_grad():
        blk.dense_1.weight.mul_(2.0)
        blk.attention.v.bias.add_(1.0)
    second = blk(x)
    blk.fused_vit = False
    assert not torch.equal(second, first) and R.rel_l2(second.cpu().numpy(), blk(x).cpu().numpy()) < 1e-5


def digest(t):
    return hashlib.sha256(t.cpu().numpy().tobytes()).hexdigest()


def test_the_switch_off_is_the_default_path_bit_for_bit(calls):
    x = images(2).to(DEV)

    def features(**kw):
        torch.manual_seed(0)
        return randomise(E.VisualFeatures(256, SIZE, **VIT64, **kw)).to(DEV).requires_grad_(False).eval()
    with torch.no_grad(), deterministic_torch():
        base = digest(features()(x))
        assert digest(features(fused_vit=False)(x)) == base
        vf = features(fused_vit='auto')
        vf.fused_vit = False
        assert digest(vf(x)) == base and not any(calls.values())


def test_producer_with_fused_vit_runs_and_repeats(calls):
    def producer(**kw):
        torch.manual_seed(0)
        return randomise(E.LanguageFeatureProducer(SIZE, n_features=256, clip_pyramid=E.SyntheticCLIPPyramid((16, 32, 32, 64), (8, 4, 2, 1), 64),
                                                   clip_text=E.SyntheticCLIPText(embed_dim=64), combine_kw=TINY_FUSION, **VIT64, **kw)).to(DEV)
    tokens = torch.from_numpy(E.tokenize(['pick up the red block'])).to(DEV)
    x = images(2).to(DEV)
    with deterministic_torch():
        plain = producer()(x, tokens=tokens)
        assert not any(calls.values())
        prod = producer(fused_vit=True)
        fused = prod(x, tokens=tokens)
        assert calls == blocks(4)
        assert fused.shape == (2, *SIZE, 256) and fused.is_contiguous() and torch.isfinite(fused).all()
        assert torch.equal(prod(x, tokens=tokens), fused)
    assert R.rel_l2(fused.cpu().numpy(), plain.cpu().numpy()) < 1e-4
    with pytest.raises(ValueError, match='multiples of 64'):                      # the tiny configuration of the other tests: embed 32
        E.LanguageFeatureProducer(SIZE, n_features=256, clip_pyramid=E.SyntheticCLIPPyramid((16, 32, 32, 64), (8, 4, 2, 1), 64),
                                  clip_text=E.SyntheticCLIPText(embed_dim=64), combine_kw=TINY_FUSION, fused_vit=True, **TINY_VIT).to(DEV)(
            x, tokens=tokens)
