"""`fused_conv` on Block / ConvolutionalEncoder / VisionTransformerEncoder / VisualFeatures and `fused_visual` on
LanguageFeatureProducer (encoders.py): the stride-1 3x3 convolutions as ops.conv3x3 launches (bias, relu in front, tile statistics) and
the blocks' batch-statistics normalisation as ops.bn_finalize + ops.bn_apply, against the float64 evaluation of the same module; the
torch GPU run of the same module is the yardstick: e_fused <= 8 e_torch, relative L2 and worst element.  Sizes are the smallest the
kernel takes: 64 -> 128 -> 128 channels at 16 x 24 in the conv encoder, 32 / 64 / 96 / 128 -> 256 on 8 x 8 ... 1 x 1 maps and
1024 -> 256 -> 128 at 16 x 16 in the ViT decoder."""
import copy
import hashlib
import json
import os

import pytest
import torch

from tests import conv3x3_ref as R
from thesis_clip_nerf_amd import encoders as E
from thesis_clip_nerf_amd import ops

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
SIZE = (32, 48)
TINY_VIT = dict(transformer_image_size=(32, 32), patch_size=16, embed_dim=32, num_heads=4, hooks=(1, 2, 3, 4), features=(32, 64, 96, 128))
TINY_FUSION = dict(clip_channels=(16, 32, 32, 64), text_dim=64, widths=(64, 32, 32), up3_filters=16)


@pytest.fixture
def calls(monkeypatch):
    """Counts the launches by wrapper."""
    seen = {'conv3x3': 0, 'bn_finalize': 0, 'bn_apply': 0}
    for name in seen:
        def counted(*args, _real=getattr(ops, name), _name=name, **kw):
            seen[_name] += 1
            return _real(*args, **kw)
        monkeypatch.setattr(ops, name, counted)
    return seen


def images(nchw=False, size=SIZE):
    x = torch.rand(2, *size, 3, generator=torch.Generator().manual_seed(8))
    return x.permute(0, 3, 1, 2).contiguous() if nchw else x


def randomise_norms(module, seed=9):
    """gamma and beta away from Keras' 1 and 0, biases away from 0: the defaults would hide a dropped bias or a wrong gamma."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for m in module.modules():
            if isinstance(m, (torch.nn.BatchNorm2d, torch.nn.BatchNorm1d)):
                m.weight.copy_(1 + 0.3 * torch.randn(m.weight.shape, generator=g))
                m.bias.copy_(0.3 * torch.randn(m.bias.shape, generator=g))
            elif isinstance(m, torch.nn.Conv2d) and m.bias is not None:
                m.bias.copy_(0.2 * torch.randn(m.bias.shape, generator=g))
    return module


def deterministic_torch():
    """torch's own switch for the parts that stay torch: without it the library's stride-2 3x3 convolution of `post_process_4` (2 x 2
    -> 1 x 1 at this size) differs by 1.2e-7 between two plain torch runs on the same input, before any HIP pass of this package has run;
    the passes themselves repeat bit for bit on equal inputs (tests/test_gpu_bn_conv.py)."""
    return torch.backends.cudnn.flags(enabled=True, benchmark=False, deterministic=True)


def check(module, x, calls, expected):
    """float64 on the CPU, torch float32 on the GPU, fused on the GPU -> the two error pairs.  All GPU runs are under torch's
    deterministic switch: it pins the library's choice of convolution algorithm, so the yardstick's error, the fused run's error (fixed
    summation orders) and with them the recorded ratios repeat from run to run - the ViT decoder's worst-element ratio,
    7.4 of the 8 allowed, is a fixed number for these seeded weights and inputs, not a draw."""
    module = randomise_norms(module).requires_grad_(False).eval()
    with torch.no_grad():
        ref = copy.deepcopy(module).double()(x.double()).numpy()
        module = module.to(DEV)
        xd = x.to(DEV)
        with deterministic_torch():
            plain = module(xd).cpu().numpy()
            assert not any(calls.values())
            module.fused_conv = True
            fused = module(xd)
            assert calls == expected, calls
            again = module(xd)
    assert fused.shape == ref.shape and torch.equal(fused, again)                 # deterministic
    e_t, e_f = R.errors(plain, ref), R.errors(fused.cpu().numpy(), ref)
    print(f'{type(module).__name__}: rel L2 {e_f[0]:.3g} = {e_f[0] / e_t[0]:.2f} x torch ({e_t[0]:.3g}), '
          f'worst {e_f[1]:.3g} = {e_f[1] / e_t[1]:.2f} x torch ({e_t[1]:.3g})')
    assert e_f[0] <= R.BAR * e_t[0] and e_f[1] <= R.BAR * e_t[1], (e_f, e_t)


def test_convolutional_encoder_against_the_float64_module(calls):
    torch.manual_seed(7)
    check(E.ConvolutionalEncoder(256), images(nchw=True), calls, {'conv3x3': 6, 'bn_finalize': 6, 'bn_apply': 6})


def test_vision_transformer_encoder_against_the_float64_module(calls):
    torch.manual_seed(7)
    kw = {k: v for k, v in TINY_VIT.items() if k != 'transformer_image_size'}
    check(E.VisionTransformerEncoder(img_size=(32, 32), n_features=256, **kw), images(nchw=True, size=(32, 32)), calls,
          {'conv3x3': 6, 'bn_finalize': 0, 'bn_apply': 0})


def test_auto_leaves_the_small_decode_convolutions_to_torch(calls):
    """8 x 8 ... 1 x 1 maps of two images are 8 workgroups each, under the 48 from which the kernel was measured faster: under 'auto' only
    the two `output_conv` convolutions (2 x 1 x 4 and 2 x 1 x 2 workgroups, but never measured slower) are launches."""
    assert E.conv3x3_auto_pays(3, 28, 28, 256) and not E.conv3x3_auto_pays(3, 14, 14, 256) and not E.conv3x3_auto_pays(3, 7, 7, 256)
    torch.manual_seed(7)
    kw = {k: v for k, v in TINY_VIT.items() if k != 'transformer_image_size'}
    enc = E.VisionTransformerEncoder(img_size=(32, 32), n_features=256, **kw).requires_grad_(False).eval().to(DEV)
    x = images(nchw=True, size=(32, 32)).to(DEV)
    with torch.no_grad():
        plain = enc(x)
        enc.fused_conv = 'auto'
        auto = enc(x)
    assert calls['conv3x3'] == 2 and R.rel_l2(auto.cpu().numpy(), plain.cpu().numpy()) < 1e-5


def test_visual_features_against_the_float64_module(calls):
    torch.manual_seed(7)
    check(E.VisualFeatures(256, SIZE, **TINY_VIT), images(), calls, {'conv3x3': 12, 'bn_finalize': 6, 'bn_apply': 6})


def test_auto_runs_torch_under_gradients_and_for_channel_counts_the_kernel_does_not_take(calls):
    torch.manual_seed(7)
    enc = E.ConvolutionalEncoder(256, fused_conv='auto').to(DEV)                  # its parameters require a gradient
    x = images(nchw=True).to(DEV)
    out = enc(x)
    out.square().mean().backward()
    assert not any(calls.values()) and enc.conv_features[4].conv_1.weight.grad is not None
    with torch.no_grad():
        fused = enc(x)
    assert calls['conv3x3'] == 6 and R.rel_l2(fused.cpu().numpy(), out.detach().cpu().numpy()) < 1e-5
    enc.fused_conv = True
    with pytest.raises(RuntimeError, match='no backward'):
        enc(x)
    small = E.ConvolutionalEncoder(64, stem=16, fused_conv='auto').to(DEV).requires_grad_(False)      # 16 -> 32 -> 32 channels
    with torch.no_grad():
        small(x)
        assert calls['conv3x3'] == 6
        small.fused_conv = True
        with pytest.raises(ValueError, match='not one the HIP pass takes'):
            small(x)


def tiny_producer(**kw):
    torch.manual_seed(0)
    return randomise_norms(E.LanguageFeatureProducer(SIZE, n_features=256, clip_pyramid=E.SyntheticCLIPPyramid((16, 32, 32, 64), (8, 4, 2, 1), 64),
                                                     clip_text=E.SyntheticCLIPText(embed_dim=64), combine_kw=TINY_FUSION, **TINY_VIT, **kw)).to(DEV)


def test_producer_with_fused_visual_runs_and_is_deterministic(calls):
    tokens = torch.from_numpy(E.tokenize(['pick up the red block'])).to(DEV)
    x = images().to(DEV)
    plain = tiny_producer()(x, tokens=tokens)
    assert not any(calls.values())
    prod = tiny_producer(fused_visual=True)
    with deterministic_torch():
        fused = prod(x, tokens=tokens)
        assert calls == {'conv3x3': 12, 'bn_finalize': 6, 'bn_apply': 6}
        assert fused.shape == (2, *SIZE, 256) and fused.is_contiguous() and torch.isfinite(fused).all()
        assert torch.equal(prod(x, tokens=tokens), fused)
    assert R.rel_l2(fused.cpu().numpy(), plain.cpu().numpy()) < 1e-4


def default_producer_digests(encoders):
    """sha256 of the tiny producer's output with the defaults and with the fusion's `fused_conv='auto'`, built from `encoders` (this
    package's module, or the parent commit's when the golden record is made) under torch's deterministic switch."""
    tokens = torch.from_numpy(encoders.tokenize(['pick up the red block'])).to(DEV)
    x = images().to(DEV)
    out = {}
    with deterministic_torch():
        for key, kw in (('default', {}), ('fused_conv_auto', {'fused_conv': 'auto'})):
            torch.manual_seed(0)
            prod = randomise_norms(encoders.LanguageFeatureProducer(
                SIZE, n_features=256, clip_pyramid=encoders.SyntheticCLIPPyramid((16, 32, 32, 64), (8, 4, 2, 1), 64),
                clip_text=encoders.SyntheticCLIPText(embed_dim=64), combine_kw=TINY_FUSION, **TINY_VIT, **kw)).to(DEV)
            out[key] = hashlib.sha256(prod(x, tokens=tokens).cpu().numpy().tobytes()).hexdigest()
    return out


def test_the_default_producer_hashes_as_it_did_before_the_switch_existed(calls, golden_dir):
    """tests/golden/producer_default_hash.json holds the digests of :func:`default_producer_digests` recorded on an MI355X with the
    encoders.py of the commit before `fused_visual` / `fused_conv` on the visual encoders existed: with the defaults nothing changed."""
    with open(os.path.join(golden_dir, 'producer_default_hash.json')) as f:
        golden = json.load(f)
    got = default_producer_digests(E)
    assert got == {k: golden[k] for k in got}, (got, golden)
    assert not calls['bn_finalize'] and not calls['bn_apply']


def test_the_switch_off_is_the_default_path_bit_for_bit(calls):
    """`fused_visual` left out, False, and 'auto' with the switch forced off again: the same bits, and no launch."""
    tokens = torch.from_numpy(E.tokenize(['pick up the red block'])).to(DEV)
    x = images().to(DEV)
    digest = lambda t: hashlib.sha256(t.cpu().numpy().tobytes()).hexdigest()
    with deterministic_torch():
        base = digest(tiny_producer()(x, tokens=tokens))
        assert digest(tiny_producer(fused_visual=False)(x, tokens=tokens)) == base
        prod = tiny_producer(fused_visual='auto')
        prod.visual_features.fused_conv = False
        assert digest(prod(x, tokens=tokens)) == base and not any(calls.values())
