"""`fused_backward` on CombineCLIPVisualV0 / CombineCLIPVisualV4 (encoders.py): under `fused_tail` and gradients the tail
runs as encoders.FuseUpsample2xFunction - the fused forward launch and one ops.fuse_upsample2x_bwd launch.  Gradients are compared with
float64 (tests/feature_tail_bwd_ref.py for the Function, the float64 CPU autograd of a deep copy for the modules); the yardstick is the
plain torch GPU float32 backward of the same tail or module: e_fused <= 8 e_torch, as relative L2 and as worst element."""
import copy

import numpy as np
import pytest
import torch

from tests import feature_fusion_ref as R
from tests import feature_tail_bwd_ref as B
from thesis_clip_nerf_amd import encoders as E
from thesis_clip_nerf_amd import ops

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
NAMES = ('fuse_upsample2x', 'fuse_upsample2x_bwd', 'gemm_tn')
TINY_FUSION = dict(clip_channels=(16, 32, 32, 64), text_dim=64, widths=(64, 32, 32), up3_filters=16)


@pytest.fixture
def calls(monkeypatch):
    """Counts the launches by wrapper; 'needs' holds the (need_a, need_b, need_g_low) of every backward launch."""
    seen = dict.fromkeys(NAMES, 0)
    seen['needs'] = []
    for name in NAMES:
        def counted(*args, _real=getattr(ops, name), _name=name, **kw):
            seen[_name] += 1
            if _name == 'fuse_upsample2x_bwd':
                seen['needs'].append((bool(kw.get('need_a', True)), bool(kw.get('need_b', True)), bool(kw.get('need_g_low', False))))
            return _real(*args, **kw)
        monkeypatch.setattr(ops, name, counted)
    return seen


def counts(calls):
    return tuple(calls[n] for n in NAMES)


def dev(x):
    return torch.from_numpy(np.array(x)).to(DEV)


def function_grads(shape, requires=(True, True, True), fused=True):
    """Gradients of sum(out * g) through the Function (or the torch tail) on the GPU -> dict(da, db, dw) of NHWC / (Cin, 256) arrays."""
    a, b, weight, g, _, _ = B.case(shape)
    ta, tb = (dev(t).permute(0, 3, 1, 2).requires_grad_(r) for t, r in zip((a, b), requires))
    conv = E.SameConv2d(weight.shape[0], 256, 1, bias=False).to(DEV)
    with torch.no_grad():
        conv.weight.copy_(dev(weight).t().reshape(conv.weight.shape))
    conv.weight.requires_grad_(requires[2])
    out = E.conv_fusion_tail(ta, tb, conv, shape[5], 'backward' if fused else False)
    assert out.shape == (a.shape[0], 256, 2 * a.shape[1], 2 * a.shape[2]) and out.dtype == torch.float32
    out.backward(dev(g).permute(0, 3, 1, 2))
    nhwc = lambda t: None if t.grad is None else t.grad.permute(0, 2, 3, 1).cpu().numpy()
    dw = None if conv.weight.grad is None else conv.weight.grad.reshape(256, -1).t().cpu().numpy()
    return dict(da=nhwc(ta), db=nhwc(tb), dw=dw), out.detach()


# 198 pixels: the weight gradient through torch's matmul; 128 pixels x 32 channels: through ops.gemm_tn
@pytest.mark.parametrize('shape', [(2, 9, 11, 128, 256), (1, 8, 16, 16, 16)], ids=str)
@pytest.mark.parametrize('act', [None, 'relu', 'elu'], ids=str)
def test_function_gradients_against_float64(shape, act, calls):
    shape = shape + (act,)
    a, b, weight, g, ref, _ = B.case(shape)
    plain, out_plain = function_grads(shape, fused=False)
    assert counts(calls) == (0, 0, 0)
    fused, out = function_grads(shape)
    uses_gemm = (shape[0] * shape[1] * shape[2]) % 8 == 0 and (shape[3] + shape[4]) % 32 == 0
    assert counts(calls) == (1, 1, int(uses_gemm)) and calls['needs'] == [(True, True, True)]
    assert torch.equal(out, ops.fuse_upsample2x(dev(a), dev(b), dev(weight), act).permute(0, 3, 1, 2))       # the unchanged forward launch
    B.assert_at_bar(fused, ref, B.errors(plain, ref), f'Function {shape}')
    again, _ = function_grads(shape)
    for name in ('da', 'db') + (('dw',) if uses_gemm else ()):
        assert np.array_equal(fused[name].view(np.uint32), again[name].view(np.uint32)), name


def test_only_what_needs_a_gradient_is_computed(calls):
    shape = (1, 8, 16, 16, 16, 'elu')
    full, _ = function_grads(shape)
    for requires in ((False, True, False), (True, False, False), (False, False, True), (True, True, False)):
        calls['needs'].clear()
        got, _ = function_grads(shape, requires)
        assert calls['needs'] == [requires]                                  # a frozen weight asks for no g_low, a frozen input is not computed
        for name, need in zip(('da', 'db', 'dw'), requires):
            assert (got[name] is not None) == need
            if need:
                assert np.array_equal(got[name].view(np.uint32), full[name].view(np.uint32)), (requires, name)
    assert calls['gemm_tn'] == 2                                             # the all-gradients run and the weight-only run


def module_gradients(module, inputs, wrt):
    """-> {name: gradient} of out.square().mean() for inputs[wrt] ('input') and every parameter, as float64 arrays."""
    module.zero_grad(set_to_none=True)
    inputs = list(inputs)
    inputs[wrt] = inputs[wrt].detach().clone().requires_grad_(True)
    module(*inputs).square().mean().backward()
    got = {n: p.grad.detach().double().cpu().numpy() for n, p in module.named_parameters() if p.grad is not None}
    got['input'] = inputs[wrt].grad.detach().double().cpu().numpy()
    return got


def check_module(module, inputs, wrt, calls, tail_weight):
    to = lambda f: [tuple(f(u) for u in t) if isinstance(t, tuple) else f(t) for t in inputs]
    ref = module_gradients(copy.deepcopy(module).double(), to(lambda t: t.double()), wrt)
    module = module.to(DEV)
    on_gpu = to(lambda t: t.to(DEV))
    module.fused_tail = False
    plain = module_gradients(module, on_gpu, wrt)
    assert counts(calls) == (0, 0, 0)
    module.fused_tail, module.fused_backward = 'auto', True
    fused = module_gradients(module, on_gpu, wrt)
    assert calls['fuse_upsample2x'] == 1 and calls['fuse_upsample2x_bwd'] == 1 and calls['needs'][-1][2] is True
    assert fused.keys() == ref.keys() == plain.keys()
    for n in ref:
        e_t = (R.rel_l2(plain[n], ref[n]), R.worst(plain[n], ref[n]))
        e_f = (R.rel_l2(fused[n], ref[n]), R.worst(fused[n], ref[n]))
        print(f'{n}: {e_f[0]:.3g} / {e_f[1]:.3g} = {e_f[0] / e_t[0]:.2f} / {e_f[1] / e_t[1]:.2f} x torch ({e_t[0]:.3g} / {e_t[1]:.3g})')
        assert e_f[0] <= B.BAR * e_t[0] and e_f[1] <= B.BAR * e_t[1], (n, e_f, e_t)
    # frozen, as the reference trains it: no g_low, and the input's gradient keeps its bits
    tail_weight.requires_grad_(False)
    frozen = module_gradients(module, on_gpu, wrt)
    assert calls['needs'][-1][2] is False and tail_weight.grad is None
    return fused, frozen


def test_combine_clip_visual_v0_against_the_float64_module(calls):
    torch.manual_seed(11)
    module = E.CombineCLIPVisualV0((8, 12), 16, 32)
    gen = torch.Generator().manual_seed(12)
    inputs = (torch.randn(2, 16, 7, 7, generator=gen), torch.randn(2, 32, 8, 12, generator=gen))
    fused, frozen = check_module(module, inputs, 1, calls, module.conv.weight)
    assert calls['needs'] == [(False, True, True), (False, True, False)]         # the CLIP map has no gradient: db only
    assert np.array_equal(fused['input'], frozen['input'])


def test_combine_clip_visual_v4_against_the_float64_module(calls):
    torch.manual_seed(13)
    module = E.CombineCLIPVisualV4(use_dense=True, activation='elu', half_size=(8, 16), visual_channels=32, **TINY_FUSION)
    gen = torch.Generator().manual_seed(14)
    rn = lambda *s: torch.randn(*s, generator=gen)
    clip = (rn(2, 64), rn(2, 16, 4, 4), rn(2, 32, 2, 2), rn(2, 32, 2, 2), rn(2, 64, 1, 1))
    check_module(module, (clip, rn(2, 32, 8, 16), rn(2, 64)), 1, calls, module.conv_fusion_3.conv.weight)
    assert calls['needs'] == [(True, True, True), (True, True, False)]


def test_the_switch_leaves_every_other_case_as_it_was(calls):
    torch.manual_seed(15)
    tail = E.CombineCLIPVisualV0((8, 12), 16, 32, fused_tail='auto', fused_backward=True).to(DEV)
    clip, vis = torch.randn(1, 16, 7, 7, device=DEV), torch.randn(1, 32, 8, 12, device=DEV)
    with torch.no_grad():                                    # nothing needs a gradient: the inference launch
        want = tail(clip, vis)
    assert counts(calls) == (1, 0, 0)
    tail.requires_grad_(False)                               # frozen weight, inputs without gradients: still the inference launch
    assert torch.equal(tail(clip, vis), want) and counts(calls) == (2, 0, 0)
    tail.requires_grad_(True)
    out16 = tail(clip, vis, out_dtype=torch.bfloat16)        # bf16 under gradients: torch, as before (fp32; the caller casts)
    assert counts(calls) == (2, 0, 0) and out16.dtype == torch.float32 and out16.requires_grad
    tail.fused_tail = True
    with pytest.raises(RuntimeError, match='no backward'):
        tail(clip, vis, out_dtype=torch.bfloat16)
    tail.fused_backward = False                              # gradients without the switch: the error under True, torch under 'auto'
    with pytest.raises(RuntimeError, match='no backward'):
        tail(clip, vis)
    tail.fused_tail = 'auto'
    tail(clip, vis).square().mean().backward()
    assert counts(calls) == (2, 0, 0)
    tail.fused_tail, tail.fused_backward = False, True       # the switch alone does nothing
    tail(clip, vis).square().mean().backward()
    assert counts(calls) == (2, 0, 0)
    tail.fused_tail = True                                   # and with both on, True runs where it raised
    got = tail(clip, vis)
    assert torch.equal(got, want) and got.requires_grad
    got.square().mean().backward()
    assert counts(calls) == (3, 1, 0)                        # (96 pixels x 48 channels: the weight gradient through torch's matmul)


def test_train_step_trains_a_producer_through_the_tail_backward(calls):
    from thesis_clip_nerf_amd import MVVNeRFRenderer
    from thesis_clip_nerf_amd.synthetic import make_scene
    tiny = dict(transformer_image_size=(32, 32), patch_size=16, embed_dim=32, num_heads=4, hooks=(1, 2, 3, 4), features=(4, 8, 16, 32))
    sc = make_scene(seed=85, batch=1, n_views=2, height=16, width=24, n_rays=32, bias_scale=0.05)
    y = np.random.default_rng(4).random((1, 32, 3)).astype(np.float32)
    inputs = tuple(sc[k] for k in ['rays_o', 'rays_d', 'images', 'intrinsics', 'extrinsics_inv'])
    torch.manual_seed(0)
    prod = E.FeatureProducer(original_image_size=(16, 24), **tiny).to(DEV)
    prod.combine_clip_visual.requires_grad_(False)           # not in trainable_parameters(): frozen, as the reference trains
    prod.combine_clip_visual.fused_tail, prod.combine_clip_visual.fused_backward = 'auto', True
    m = MVVNeRFRenderer(32, 32, n_views=2, batch_size=1, near=sc['near'], far=sc['far'], device=DEV, feature_encoder=prod)
    m.set_weights(sc['coarse'], sc['fine'])
    opt, sched = E.make_encoder_optimizer(prod, target_lr=1e-3, warmup_steps=1)
    m.compile(learning_rate=0.0, encoder_optimizer=opt)
    sched.step()                                             # past the warm-up's lr(0) = 0
    before = [p.detach().clone() for p in prod.trainable_parameters()]
    out = m.train_step((inputs, y), u_coarse=dev(sc['u_coarse']), u_fine=dev(sc['u_fine']), stop_fine_z=True)
    torch.cuda.synchronize()
    assert np.isfinite(float(out['loss']))
    assert counts(calls) == (1, 1, 0) and calls['needs'] == [(False, True, False)]          # one forward and one backward tail launch
    names = {id(p): n for n, p in prod.named_parameters()}
    unchanged = [names[id(p)] for p, old in zip(prod.trainable_parameters(), before) if torch.equal(p, old)]
    assert not unchanged, unchanged
    assert all(torch.isfinite(p.grad).all() for p in prod.trainable_parameters() if p.grad is not None)
