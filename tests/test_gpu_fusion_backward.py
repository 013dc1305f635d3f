"""Training through the language fusion on the GPU: encoders.Conv3x3ActFunction - the frozen two-source 3x3 convolution
with its activation and `mul`, HIP in both directions - against the float64 references of tests/fusion_bwd_ref.py at the project's bar
e64 <= 8 e32 (e32: torch's float32 CPU autograd of the same case), with exact impulse and power-of-two properties and a launch census;
`fused_backward` on CombineCLIPVisualV4 against the float64 twin of the module with a synthetic visual-features leaf (the yardstick is
the module's own torch float32 backward on the GPU); one `train_step` through encoders.FeatureProducerV4; the six checkpoint files into
LanguageNeRF.load_backbone; the train_nerf command line with a resume.  The tiny torch ViT runs in the train_step test and the command
line test only."""
import copy
import json
import os

import numpy as np
import pytest
import torch

from tests import conv3x3_ref as R
from tests import fusion_bwd_ref as G
from tests.test_gpu_fused_visual import deterministic_torch
from thesis_clip_nerf_amd import encoders as E
from thesis_clip_nerf_amd import ops

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
TINY_VISUAL = dict(transformer_image_size=(32, 32), patch_size=16, embed_dim=32, num_heads=4, hooks=(1, 2, 3, 4), features=(4, 8, 16, 32))
FUSION = dict(clip_channels=(32, 32, 32, 32), text_dim=64, widths=(64, 64, 64), up3_filters=64)
SIZES = [(1, 3, 5), (1, 16, 16), (1, 17, 33), (2, 19, 35)]
CHANNELS = [(64, 32, 64), (64, 0, 64)]


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def nchw(a, grad=False):
    return None if a is None else dev(a).permute(0, 3, 1, 2).requires_grad_(grad)


def nhwc(t):
    return t.detach().permute(0, 2, 3, 1).contiguous().cpu().numpy()


def frozen_conv(wt):
    conv = E.SameConv2d(wt.shape[2], wt.shape[3], 3, bias=False).to(DEV)
    E.load_conv(conv, wt, None)
    return conv.requires_grad_(False)


@pytest.fixture()
def calls(monkeypatch):
    seen = []
    for name in ('conv3x3', 'act_gate', 'absmax', 'conv3x3_wgrad', 'conv3x3_pack'):
        real = getattr(ops, name)
        monkeypatch.setattr(ops, name, lambda *a, _real=real, _name=name, **kw: (seen.append(_name), _real(*a, **kw))[1])
    return seen


def run_function(conv, a, b, mul, act, g, switch=True, b_grad=True):
    at, bt = nchw(a, True), nchw(b, b_grad)
    mul4 = None if mul is None else dev(mul)[:, :, None, None]
    out, top = E.conv3x3_act(conv, at, bt, act, switch, mul4, fused_backward=True)
    out.backward(nchw(g))
    return out, top, at, bt


def check_bar(name, got, ref, yard):
    err = R.errors(got, ref)
    print(f'{name}: e64 = {err[0]:.3g}, {err[1]:.3g}; e32 = {yard[0]:.3g}, {yard[1]:.3g}; ratios {err[0] / yard[0]:.2f}, {err[1] / yard[1]:.2f}')
    assert G.within_bar(err, yard), (name, err, yard)


_refs = {}


def reference(shape, kind, act):
    """(inputs, float64 (da, db), float32 CPU yardstick errors) of one case, computed once."""
    key = (shape, kind, act)
    if key not in _refs:
        a, b, wt, mul, g = G.two_source_inputs(shape, kind)
        ref = G.two_source_grads_ref(a, b, wt, mul, act, g)
        cpu32 = G.torch_two_source_grads(a, b, wt, mul, act, g, torch.float32)
        yard = [R.errors(c, r) for c, r in zip(cpu32, ref) if r is not None]
        _refs[key] = ((a, b, wt, mul, g), ref, yard)
    return _refs[key]


@pytest.mark.parametrize('kind', ['none', 'with_zero'])
@pytest.mark.parametrize('act', G.ACTS)
@pytest.mark.parametrize('channels', CHANNELS, ids=str)
@pytest.mark.parametrize('size', SIZES, ids=str)
def test_function_gradients_against_float64(size, channels, act, kind, calls):
    shape = (*size, *channels)
    (a, b, wt, mul, g), ref, yard = reference(shape, kind, act)
    conv = frozen_conv(wt)
    out, top, at, bt = run_function(conv, a, b, mul, act, g)
    want = R.conv_ref(a, b, wt, act, mul)
    assert R.rel_l2(nhwc(out), want) < 1e-6 and float(top) == float(out.detach().abs().max())
    assert 'act_gate' in calls and conv.weight.grad is None
    check_bar(f'{shape} {act} {kind} da', nhwc(at.grad), ref[0], yard[0])
    if b is not None:
        check_bar(f'{shape} {act} {kind} db', nhwc(bt.grad), ref[1], yard[1])
    if kind == 'with_zero':                                   # channels under mul == 0 carry nothing back; d is exactly zero there
        d = ops.act_gate(dev(g), out.detach().permute(0, 2, 3, 1).contiguous(), dev(mul), act)
        assert not d[..., ::3].contiguous().view(torch.int32).any()


def test_two_backward_launches_per_convolution_and_no_absmax(calls):
    (a, b, wt, mul, g), _, _ = reference((2, 19, 35, 64, 32, 64), 'with_zero', 'elu')
    conv = frozen_conv(wt)
    at, bt = nchw(a, True), nchw(b, False)                    # the CLIP map needs no gradient
    out, _ = E.conv3x3_act(conv, at, bt, 'elu', 'auto', dev(mul)[:, :, None, None], fused_backward=True)
    assert calls.count('conv3x3') == 1 and 'act_gate' not in calls
    del calls[:]
    out.backward(nchw(g))
    assert calls == ['act_gate', 'conv3x3_pack', 'conv3x3'], calls          # the `a` rows packed once ...
    assert bt.grad is None and at.grad.shape == at.shape
    first = at.grad.clone()
    at.grad = None
    out, _ = E.conv3x3_act(conv, at, bt, 'elu', 'auto', dev(mul)[:, :, None, None], fused_backward=True)
    del calls[:]
    out.backward(nchw(g))
    assert calls == ['act_gate', 'conv3x3'], calls                          # ... and cached: two launches, no absmax
    assert torch.equal(at.grad, first)                                      # and the same bits
    # 64 + 32: the `b` rows do not fit the kernel (32 % 64), so db is torch's; da stays the launch
    at, bt = nchw(a, True), nchw(b, True)
    out, _ = E.conv3x3_act(conv, at, bt, 'elu', True, dev(mul)[:, :, None, None], fused_backward=True)
    del calls[:]
    out.backward(nchw(g))
    assert calls == ['act_gate', 'conv3x3'] and bt.grad is not None and torch.equal(at.grad, first)
    assert E.conv3x3_rows_dgrad_fusable(conv, 0, 64) and not E.conv3x3_rows_dgrad_fusable(conv, 64, 96)


def test_impulse_gradients_are_the_gated_flipped_stamp():
    """g is 1 at one (pixel, co) per image - corners, both sides of a tile seam - weights small integers / 8, relu, no mul:
    da[py + dy - 1, px + dx - 1, ci] = W[dy, dx, ci, co] where the forward's out is positive at the pixel, zero otherwise; bit for bit."""
    h, w, ca, cb, cout = 19, 35, 64, 32, 64
    rng = np.random.default_rng(22)
    wt = rng.integers(-8, 9, (3, 3, ca + cb, cout)).astype(np.float32) / 8
    places = [(0, 0), (h - 1, w - 1), (0, w - 1), (15, 15), (16, 16), (15, 16), (9, 31), (9, 32)]
    a = rng.integers(-4, 5, (len(places), h, w, ca)).astype(np.float32) / 4
    b = rng.integers(-4, 5, (len(places), h, w, cb)).astype(np.float32) / 4
    conv = frozen_conv(wt)
    g = np.zeros((len(places), h, w, cout), np.float32)
    picks = []
    for i, (py, px) in enumerate(places):
        co = int(rng.integers(0, cout))
        g[i, py, px, co] = 1.0
        picks.append(co)
    out, _, at, bt = run_function(conv, a, b, None, 'relu', g)
    fwd = nhwc(out)
    assert np.array_equal(fwd, R.conv_ref(a, b, wt, 'relu').astype(np.float32))           # small integers: the forward is exact
    want = np.zeros((len(places), h, w, ca + cb), np.float32)
    opened = 0
    for i, ((py, px), co) in enumerate(zip(places, picks)):
        if fwd[i, py, px, co] > 0:
            opened += 1
            for dy in range(3):
                for dx in range(3):
                    y, x = py + dy - 1, px + dx - 1
                    if 0 <= y < h and 0 <= x < w:
                        want[i, y, x] = wt[dy, dx, :, co]
    assert 0 < opened < len(places)                                                        # both sides of the gate are on trial
    assert np.array_equal(nhwc(at.grad), want[..., :ca]) and np.array_equal(nhwc(bt.grad), want[..., ca:])


@pytest.mark.parametrize('act', G.ACTS)
def test_scaling_g_by_powers_of_two_scales_the_gradients_bit_for_bit(act):
    (a, b, wt, mul, g), _, _ = reference((2, 19, 35, 64, 0, 64), 'with_zero', act)
    conv = frozen_conv(wt)
    base = run_function(conv, a, None, mul, act, g)[2].grad
    for k in (-7, 5):
        scaled = run_function(conv, a, None, mul, act, np.ldexp(g, k))[2].grad
        assert torch.equal(scaled, torch.ldexp(base, torch.tensor(k, device=DEV)))


def test_trained_weights_or_mul_are_not_this_paths_case(calls):
    (a, b, wt, mul, g), _, _ = reference((1, 3, 5, 64, 32, 64), 'with_zero', 'relu')
    conv = frozen_conv(wt).requires_grad_(True)
    at, bt = nchw(a, True), nchw(b, False)
    with pytest.raises(ValueError, match='freeze'):
        E.conv3x3_act(conv, at, bt, 'relu', True, None, fused_backward=True)
    out, top = E.conv3x3_act(conv, at, bt, 'relu', 'auto', None, fused_backward=True)        # 'auto': torch, and the weight learns
    assert top is None and not calls
    out.square().mean().backward()
    assert conv.weight.grad is not None and at.grad is not None
    conv.requires_grad_(False)
    mul4 = dev(mul)[:, :, None, None].requires_grad_(True)
    with pytest.raises(ValueError, match='freeze'):
        E.conv3x3_act(conv, at, bt, 'relu', True, mul4, fused_backward=True)
    assert E.conv3x3_act(conv, at, bt, 'relu', 'auto', mul4, fused_backward=True)[1] is None and not calls
    with pytest.raises(RuntimeError, match='no backward'):                                   # without the switch: as before
        E.conv3x3_act(conv, at, bt, 'relu', True, None)


# ---- the module ---------------------------------------------------------------------------------------------------------------------------
def fusion_inputs(visual_channels, device, dtype, n=2):
    gen = torch.Generator().manual_seed(5)
    r = lambda *s: torch.randn(*s, generator=gen).to(device=device, dtype=dtype)
    clip = (r(n, 64), r(n, 32, 8, 12), r(n, 32, 4, 6), r(n, 32, 2, 3), r(n, 32, 1, 2))
    return clip, r(n, visual_channels, 16, 24), r(n, 64)


def visual_gradient(module, device, dtype, visual_channels):
    clip, visual, text = fusion_inputs(visual_channels, device, dtype)
    visual.requires_grad_(True)
    out = module(clip, visual, text)
    out.square().mean().backward()
    return out.detach(), visual.grad.detach().double().cpu().numpy()


@pytest.mark.parametrize('visual_channels', [32, 64])
@pytest.mark.parametrize('use_dense,activation', [(False, 'relu'), (True, 'elu'), (False, 'elu'), (True, 'relu')])
def test_combine_clip_visual_v4_gradient_against_the_float64_twin(use_dense, activation, visual_channels, calls):
    torch.manual_seed(11)
    mod = E.CombineCLIPVisualV4(use_dense=use_dense, activation=activation, half_size=(16, 24), visual_channels=visual_channels,
                                fused_tail=False, **FUSION).requires_grad_(False)
    ref = visual_gradient(copy.deepcopy(mod).double(), 'cpu', torch.float64, visual_channels)[1]
    mod = mod.to(DEV)
    with deterministic_torch():
        out_plain, plain = visual_gradient(mod, DEV, torch.float32, visual_channels)
        assert not calls
        mod.fused_conv, mod.fused_backward = 'auto', True
        assert all(u.fused_backward is True for u in (mod.up_1, mod.up_2, mod.up_3))
        out_fused, fused = visual_gradient(mod, DEV, torch.float32, visual_channels)
        # forward: conv, up_1 (2) as inference launches, up_2 and up_3 (4) through the Function; backward: 4 gates, 4 data gradients
        assert calls.count('act_gate') == 4 and calls.count('conv3x3') == 7 + 4 and 'conv3x3_wgrad' not in calls, calls
        assert all(p.grad is None for p in mod.parameters())
        # the switches off again: today's path, bit for bit - with gradients, and without (where only `fused_conv` decides)
        mod.fused_conv, mod.fused_backward = False, False
        out_again, again = visual_gradient(mod, DEV, torch.float32, visual_channels)
        assert torch.equal(out_again, out_plain)
        mod.fused_conv = 'auto'
        clip, visual, text = fusion_inputs(visual_channels, DEV, torch.float32)
        with torch.no_grad():
            inference = mod(clip, visual, text)
            mod.fused_backward = True
            assert torch.equal(mod(clip, visual, text), inference)
    assert R.rel_l2(out_fused.cpu().numpy(), out_plain.cpu().numpy()) < 1e-5
    e_t, e_f = R.errors(plain, ref), R.errors(fused, ref)
    print(f'use_dense={use_dense} {activation} C={visual_channels}: fused {e_f[0]:.3g}, {e_f[1]:.3g}; torch {e_t[0]:.3g}, {e_t[1]:.3g}; '
          f'ratios {e_f[0] / e_t[0]:.2f}, {e_f[1] / e_t[1]:.2f}')
    assert G.within_bar(e_f, e_t), (e_f, e_t)


# ---- the producer inside train_step, the files, the loop -------------------------------------------------------------------------------
def tiny_producer(**kw):
    pyramid = E.SyntheticCLIPPyramid(FUSION['clip_channels'], ((8, 8), (4, 4), (2, 2), (1, 1)), FUSION['text_dim'])
    return E.FeatureProducerV4((32, 32), n_features=32, clip_pyramid=pyramid, combine_kw=FUSION, **TINY_VISUAL, **kw)


def test_train_step_trains_the_visual_encoder_through_the_fusion(calls):
    from oracle import mvnerf_torch as T
    from thesis_clip_nerf_amd import MVVNeRFRenderer
    from thesis_clip_nerf_amd.synthetic import make_scene
    sc = make_scene(seed=86, batch=1, n_views=2, height=32, width=32, n_rays=32, bias_scale=0.05)
    y = np.random.default_rng(4).random((1, 32, 3)).astype(np.float32)
    torch.manual_seed(0)
    prod = tiny_producer(fused_conv='auto', fused_backward=True).to(DEV)
    twin = copy.deepcopy(prod).double().cpu()
    fusion_before = {k: v.clone() for k, v in prod.combine_clip_visual.state_dict().items()}
    m = MVVNeRFRenderer(32, 32, n_views=2, batch_size=1, near=sc['near'], far=sc['far'], device=DEV, feature_encoder=prod)
    m.set_weights(sc['coarse'], sc['fine'])
    opt, sched = E.make_encoder_optimizer(prod, target_lr=1e-3, warmup_steps=1)
    m.compile(learning_rate=0.0, encoder_optimizer=opt)
    inputs = tuple(sc[k] for k in ['rays_o', 'rays_d', 'images', 'intrinsics', 'extrinsics_inv'])
    before = [p.detach().clone() for p in prod.trainable_parameters()]
    u = dict(u_coarse=dev(sc['u_coarse']), u_fine=dev(sc['u_fine']), stop_fine_z=True)
    m.train_step((inputs, y), **u)                                        # lr(0) = 0: gradients only
    torch.cuda.synchronize()
    assert calls.count('act_gate') == 4, calls                            # up_2 and up_3, two convolutions each
    got = {n: p.grad.double().cpu().clone() for n, p in prod.named_parameters() if p.grad is not None}
    assert not any(n.startswith('combine_clip_visual') for n in got)
    t = lambda k: torch.as_tensor(sc[k]).double()
    imgs = t('images')
    feats = twin(imgs.reshape(2, 32, 32, 3)).reshape(1, 2, 32, 32, 256)
    out = T.render_call(t('coarse'), t('fine'), t('rays_o'), t('rays_d'), imgs, t('intrinsics'), t('extrinsics_inv'), feats,
                        sc['near'], sc['far'], sc['n_samples'], t('u_coarse'), t('u_fine'), stop_fine_z=True)
    yy = torch.as_tensor(y).double()
    (((yy - out[0]) ** 2).mean() + ((yy - out[2]) ** 2).mean()).backward()
    checked, worst = 0, (0.0, None)
    for n, p in twin.named_parameters():
        if p.grad is None or n not in got or p.grad.norm() == 0:
            continue
        ref = p.grad.clamp(-1.0, 1.0)                                      # train_step clips by value before the optimizer step
        if ref.norm() < 1e-7:                                              # a bias in front of a batch-statistics norm: exactly zero
            assert got[n].norm() < 1e-5, (n, float(got[n].norm()))
            continue
        rel = float((got[n] - ref).norm() / ref.norm())
        worst = max(worst, (rel, n))
        assert rel < 2e-2, (n, rel)
        checked += 1
    print(f'{checked} encoder gradients, largest relative L2 {worst[0]:.3g} ({worst[1]})')
    assert checked >= 20
    assert all(torch.equal(a, b) for a, b in zip(before, prod.trainable_parameters()))
    sched.step()                                                          # past the warm-up's lr(0) = 0
    m.train_step((inputs, y), **u)
    assert any(not torch.equal(a, b) for a, b in zip(before, prod.trainable_parameters()))
    after = prod.combine_clip_visual.state_dict()
    assert all(torch.equal(after[k], v) for k, v in fusion_before.items())


def test_six_files_reach_the_language_model_bit_for_bit(tmp_path):
    from thesis_clip_nerf_amd import MVVNeRFRenderer
    from thesis_clip_nerf_amd._lib import NET_PARAMS
    from thesis_clip_nerf_amd.lmvnerf import LanguageNeRF
    from thesis_clip_nerf_amd.synthetic import glorot_net
    torch.manual_seed(3)
    rng = np.random.default_rng(3)
    src = MVVNeRFRenderer(32, 32, n_views=1, batch_size=1, device=DEV, feature_encoder=tiny_producer().to(DEV))
    src.set_weights(glorot_net(rng, bias_scale=0.05), glorot_net(rng, bias_scale=0.05))
    path = str(tmp_path / 'model_final')
    src.store(path)
    assert len(os.listdir(tmp_path)) == 4                                  # the default writes the four MLP files
    dst = MVVNeRFRenderer(32, 32, n_views=1, batch_size=1, device=DEV, feature_encoder=tiny_producer().to(DEV))
    kept = {k: v.clone() for k, v in dst.feature_encoder.state_dict().items()}
    assert dst.load(path, encoders=True) is False
    assert all(torch.equal(v, kept[k]) for k, v in dst.feature_encoder.state_dict().items())
    src.store(path, encoders=True)
    assert len(os.listdir(tmp_path)) == 6
    assert dst.load(path, encoders=True) is True
    assert torch.equal(dst.coarse_net, src.coarse_net) and torch.equal(dst.fine_net, src.fine_net)
    want = src.feature_encoder.state_dict()
    assert all(torch.equal(v, want[k]) for k, v in dst.feature_encoder.state_dict().items())
    pyramid = E.SyntheticCLIPPyramid(FUSION['clip_channels'], ((8, 8), (4, 4), (2, 2), (1, 1)), FUSION['text_dim'])
    producer = E.LanguageFeatureProducer((32, 32), n_features=32, clip_pyramid=pyramid, clip_text=E.SyntheticCLIPText(embed_dim=64),
                                         combine_kw=dict(FUSION, use_dense=False, activation='relu'), **TINY_VISUAL).to(DEV)
    model = LanguageNeRF(np.zeros(NET_PARAMS, dtype=np.float32), n_points_train=4, n_views=1, batch_size=1, device=DEV)
    assert model.load_backbone(path, verbose=False, producer=producer) is True
    assert torch.equal(model.trunk_net.detach(), src.fine_net)
    for name in ('visual_features', 'combine_clip_visual'):
        ours, theirs = getattr(producer, name).state_dict(), getattr(src.feature_encoder, name).state_dict()
        assert ours.keys() == theirs.keys() and all(torch.equal(ours[k], theirs[k]) for k in ours)


def test_train_nerf_with_the_v4_encoder_and_a_resume(tmp_path, capsys):
    from thesis_clip_nerf_amd import train_nerf
    run = str(tmp_path / 'run')
    argv = ['--model-path', run, '--eval-after', '1', '--n-rays', '64', '--size', '32', '--encoder', 'v4', '--tiny-encoder', '--fused-conv',
            '--fused-backward']
    np.random.seed(0)
    torch.manual_seed(0)
    train_nerf.main(argv + ['--epochs', '2'])
    first = capsys.readouterr().out
    assert 'New model initialized' in first and 'Epoch 2/2' in first
    files = sorted(f for f in os.listdir(run) if f.endswith('.pt'))
    assert files == sorted(f'model_final_{n}.pt' for n in ('coarse_embedding', 'coarse_readout', 'fine_embedding', 'fine_readout',
                                                           'visual_features', 'combine_clip_visual'))
    assert sorted(os.listdir(f'{run}/valid')) == ['valid-0.ppm', 'valid-1.ppm', 'valid-2.ppm']
    torch.manual_seed(0)                                                  # the fusion is frozen: its file holds the initial weights
    fresh = train_nerf.make_feature_encoder('v4', (32, 32), tiny=True)
    saved = torch.load(f'{run}/model_final_combine_clip_visual.pt', weights_only=True)
    init = fresh.combine_clip_visual.state_dict()
    assert saved.keys() == init.keys() and all(torch.equal(saved[k], init[k].cpu()) for k in saved)
    train_nerf.main(argv + ['--epochs', '3'])
    second = capsys.readouterr().out
    assert 'Model loaded from checkpoint.' in second and 'Epoch 3/3' in second and 'Epoch 2/3' not in second
    with open(f'{run}/training_progress.json') as f:
        assert json.load(f) == {'epoch': 3}
    assert os.path.exists(f'{run}/valid/valid-3.ppm')
