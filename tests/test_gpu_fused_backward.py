"""`fused_backward` on Block / ConvolutionalEncoder / VisionTransformerEncoder / VisualFeatures (encoders.py): under
`fused_conv` and gradients the stride-1 3x3 convolutions run as encoders.Conv3x3BiasFunction - the fused forward launch, ops.conv3x3_wgrad
and the data gradient through the transposed pack - and the batch-statistics normalisation, skip and relu as torch.  The gradients of
`out.square().mean()` with respect to the input and every parameter are compared with the float64 CPU autograd of a deep copy; the
yardstick is the plain torch GPU float32 backward of the same module: e_fused <= 8 e_torch on the relative L2 of every tensor.  The
biases of the six block convolutions sit in front of a batch-statistics normalisation: their true gradient is zero and a ratio of
rounding noise means nothing, so exactly those are left out (and the attentions' key biases, see `check`).  Sizes as tests/test_gpu_fused_visual.py."""
import copy

import numpy as np
import pytest
import torch

from tests import conv3x3_ref as R
from tests.test_gpu_fused_visual import SIZE, TINY_VIT, deterministic_torch, images, randomise_norms
from thesis_clip_nerf_amd import encoders as E
from thesis_clip_nerf_amd import ops

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
NAMES = ('conv3x3', 'conv3x3_wgrad', 'bn_finalize', 'bn_apply')


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


def gradients(module, x):
    """-> {name: gradient} of out.square().mean() for the input ('input') and every parameter, as float64 arrays."""
    module.zero_grad(set_to_none=True)
    x = x.detach().clone().requires_grad_(True)
    module(x).square().mean().backward()
    got = {n: p.grad.detach().double().cpu().numpy() for n, p in module.named_parameters() if p.grad is not None}
    got['input'] = x.grad.detach().double().cpu().numpy()
    return got


def check(module, x, calls, expected, zero_bias_names, repeatable=lambda name: True):
    """`repeatable`: the tensors whose gradient must repeat bit for bit - every gradient the HIP passes and torch's deterministic
    kernels alone decide.  torch's bilinear up-sampling backward adds with atomics, so whatever lies upstream of an `_up` / `_resize`
    in the backward differs between two runs of plain torch as well (the test prints both lists); those are held to the bar in both runs.
    `zero_bias_names` are the parameters whose true gradient is zero: next to them, the key bias of every attention (a shift of all
    keys by one vector adds a constant to a query's logits, which the softmax removes) is left out for the same reason."""
    module = randomise_norms(module)
    ref = gradients(copy.deepcopy(module).double(), x.double())
    module = module.to(DEV)
    xd = x.to(DEV)
    with deterministic_torch():
        plain = gradients(module, xd)
        assert not any(calls.values())
        plain_again = gradients(module, xd)
        module.fused_conv, module.fused_backward = True, True
        fused = gradients(module, xd)
        assert calls == expected, calls
        again = gradients(module, xd)
    assert fused.keys() == ref.keys() == plain.keys()
    print('torch differs between two runs in:', sorted(n for n in plain if not np.array_equal(plain[n], plain_again[n])))
    print('fused differs between two runs in:', sorted(n for n in fused if not np.array_equal(fused[n], again[n])))
    for n in fused:
        if repeatable(n):
            assert np.array_equal(fused[n], again[n]), f'two runs differ in {n}'
    top = max(np.linalg.norm(ref[n]) for n in ref if n != 'input')
    excluded = {n for n in ref if n != 'input' and np.linalg.norm(ref[n]) < 1e-6 * top}
    assert excluded == set(zero_bias_names) | {n for n in ref if n.endswith('attention.k.bias')}, excluded
    worst = (0.0, None)
    for n in ref:
        if n in excluded:
            continue
        e_t = R.rel_l2(plain[n], ref[n])
        for run in (fused, again):
            e_f = R.rel_l2(run[n], ref[n])
            worst = max(worst, (e_f / e_t, n))
            assert e_f <= R.BAR * e_t, (n, e_f, e_t)
        print(f'{n}: rel L2 {e_f:.3g} = {e_f / e_t:.2f} x torch ({e_t:.3g})')
    print(f'{type(module).__name__}: largest ratio {worst[0]:.2f} ({worst[1]})')


BLOCK_BIASES = [f'conv_features.{b}.conv_{c}.bias' for b in (3, 4, 5) for c in (1, 2)]


def test_convolutional_encoder_gradients_against_the_float64_module(calls):
    """Six convolutions forward, six weight gradients, six data gradients (the first block's input comes from the trained stem)."""
    torch.manual_seed(7)
    check(E.ConvolutionalEncoder(256), images(nchw=True), calls, {'conv3x3': 12, 'conv3x3_wgrad': 6, 'bn_finalize': 0, 'bn_apply': 0},
          BLOCK_BIASES)


def test_vision_transformer_encoder_gradients_against_the_float64_module(calls):
    """Four `conv_decode` and two `output_conv` forward and weight gradients; the data gradient is a launch for 64, 128, 1024 and 256
    input channels and torch's for 32 and 96."""
    torch.manual_seed(7)
    kw = {k: v for k, v in TINY_VIT.items() if k != 'transformer_image_size'}
    check(E.VisionTransformerEncoder(img_size=(32, 32), n_features=256, **kw), images(nchw=True, size=(32, 32)), calls,
          {'conv3x3': 10, 'conv3x3_wgrad': 6, 'bn_finalize': 0, 'bn_apply': 0}, [], lambda name: name.startswith('output_conv'))


def test_visual_features_gradients_against_the_float64_module(calls):
    torch.manual_seed(7)
    check(E.VisualFeatures(256, SIZE, **TINY_VIT), images(), calls, {'conv3x3': 22, 'conv3x3_wgrad': 12, 'bn_finalize': 0, 'bn_apply': 0},
          ['conv_features.' + n for n in BLOCK_BIASES], lambda name: name.startswith('conv_features'))


def test_the_switch_leaves_every_other_case_as_it_was(calls):
    torch.manual_seed(7)
    enc = E.ConvolutionalEncoder(256, fused_conv='auto', fused_backward=True).to(DEV)
    x = images(nchw=True).to(DEV)
    with torch.no_grad():                                    # nothing needs a gradient: the inference passes, statistics and all
        enc(x)
    assert calls == {'conv3x3': 6, 'conv3x3_wgrad': 0, 'bn_finalize': 6, 'bn_apply': 6}
    enc.fused_backward = False                               # gradients without the switch: torch under 'auto', the error under True
    enc(x).square().mean().backward()
    assert calls == {'conv3x3': 6, 'conv3x3_wgrad': 0, 'bn_finalize': 6, 'bn_apply': 6}
    enc.fused_conv = True
    with pytest.raises(RuntimeError, match='no backward'):
        enc(x)
    enc.fused_conv, enc.fused_backward = False, True         # the switch alone does nothing
    enc(x).square().mean().backward()
    assert calls == {'conv3x3': 6, 'conv3x3_wgrad': 0, 'bn_finalize': 6, 'bn_apply': 6}
    small = E.ConvolutionalEncoder(64, stem=16, fused_conv='auto', fused_backward=True).to(DEV)      # 16 -> 32 -> 32: not the kernel's
    small(x).square().mean().backward()
    assert calls['conv3x3_wgrad'] == 0
    small.fused_conv = True
    with pytest.raises(ValueError, match='not one the HIP pass takes'):
        small(x)


def test_train_step_trains_a_producer_through_the_hip_backward(calls):
    from thesis_clip_nerf_amd import MVVNeRFRenderer
    from thesis_clip_nerf_amd.synthetic import make_scene
    tiny = dict(transformer_image_size=(32, 32), patch_size=16, embed_dim=32, num_heads=4, hooks=(1, 2, 3, 4), features=(4, 8, 16, 32))
    sc = make_scene(seed=85, batch=1, n_views=2, height=16, width=24, n_rays=32, bias_scale=0.05)
    y = np.random.default_rng(4).random((1, 32, 3)).astype(np.float32)
    inputs = tuple(sc[k] for k in ['rays_o', 'rays_d', 'images', 'intrinsics', 'extrinsics_inv'])
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    for kw, hip in ((dict(), False), (dict(fused_conv='auto', fused_backward=True), True)):
        torch.manual_seed(0)
        prod = E.FeatureProducer(original_image_size=(16, 24), **tiny, **kw).to(DEV)
        m = MVVNeRFRenderer(32, 32, n_views=2, batch_size=1, near=sc['near'], far=sc['far'], device=DEV, feature_encoder=prod)
        m.set_weights(sc['coarse'], sc['fine'])
        opt, sched = E.make_encoder_optimizer(prod, target_lr=1e-3, warmup_steps=1)
        m.compile(learning_rate=0.0, encoder_optimizer=opt)
        sched.step()                                         # past the warm-up's lr(0) = 0
        before = [p.detach().clone() for p in prod.trainable_parameters()]
        for name in calls:
            calls[name] = 0
        out = m.train_step((inputs, y), u_coarse=dev(sc['u_coarse']), u_fine=dev(sc['u_fine']), stop_fine_z=True)
        torch.cuda.synchronize()
        assert np.isfinite(float(out['loss']))
        assert any(not torch.equal(a, b) for a, b in zip(before, prod.trainable_parameters()))
        if hip:            # the six block convolutions and the two of output_conv, forward, weight and data gradient; conv_decode is too small
            assert calls == {'conv3x3': 16, 'conv3x3_wgrad': 8, 'bn_finalize': 0, 'bn_apply': 0}, calls
            assert all(torch.isfinite(p.grad).all() for p in prod.trainable_parameters() if p.grad is not None)
        else:
            assert not any(calls.values()), calls
