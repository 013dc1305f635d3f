"""LanguageNeRF.compile(fused_step=True): the training step up to the optimiser as one C call (csrc/language_api.hip), and the kernels it
adds (mvnerf_pose_query_jvp, mvnerf_landscape_loss, mvnerf_cosine_loss), on the GPU.

Kernels: the bars of tests/test_language_math_cpu.py (the host build of the same source) unchanged - float64 autograd, 1e-5 for the JVP,
8 x the float32 evaluation's error for the losses - with NaN-prefilled outputs and guard rows, pad rows left alone, two runs the same bits.

The whole step, against oracle/lmvnerf_torch in float64 (train_losses; its pieces for the cross-entropy landscape), with the bars of
tests/test_gpu_language_fused_tail.py::test_language_train_step_with_fused_tail_matches_restatement unchanged (prediction and landscape
1e-4, cosine losses 5e-3, every variable |g - ref| < 3e-2 |ref| + 1e-6), and for every variable at most 4 x the error of the path it
replaces (fused_tail=True, autograd) + 1e-6, the factor of tests/test_gpu_grasp_tail_train.py.  Each loss term alone through the loss
weights; the step through ctypes alone; the captured graph; the flag.

The scenes follow the seed rule of the test whose bars these are (language_case(50 + n_views, ...)).  The bars against float64 are bars on
the trunk's fp32 passes as much as on the step: on another scene (seed 102 at V=1, B=2, np=3, quaternion) the autograd path and the fused step
agree with each other (grad_loss_t 0.300240 / 0.300237, every variable's error within 1 %) and both sit 5.5e-3 from float64's 0.294715, over the
5e-3 bar, with the second-order gradients of that term 3.1 % off; the 4 x rule against the path it replaces held on that scene too."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from oracle import lmvnerf_torch as L
from oracle import mvnerf_torch as T
from tests import test_language_math_cpu as H
from tests.test_gpu_language_fused_tail import language_case, t64
from tests.test_oracle_lmvnerf import keras_weights
from tests.test_pose_math_cpu import F32
from thesis_clip_nerf_amd import _lib, ops
from thesis_clip_nerf_amd import lmvnerf as M

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
NAN = float('nan')


@pytest.fixture(scope='module')
def cpu():
    lib = H.build('cpu_language', 'libmvnerf_language_cpu.so')
    lib.pose = H.build('cpu_pose', 'libmvnerf_pose_cpu.so')
    return lib


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


# ---- kernels ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('representation', ['quaternion', '6d'])
@pytest.mark.parametrize('p,n_scenes,pad', [(1, 1, 0), (5, 2, 7), (53, 1, 0)])          # P n5 = 42, 210, 2226: no multiple of 64
def test_pose_query_jvp_kernel(cpu, representation, p, n_scenes, pad):
    rep, rd, offsets, t, r, c_t, c_r = H.jvp_case(representation, 100 + p, p=p)
    n5 = offsets.shape[0]
    n, ld = p * n5, p * n5 + pad
    ref = H.jvp_ref(representation, offsets, t, r, c_t, c_r)
    host = H.host_jvp(cpu, rep, offsets, r, c_t, c_r)
    runs = []
    for _ in range(2):
        # one guard scene in front of and behind the n_scenes the kernel owns
        bufs = [torch.full((n_scenes + 2, ld, 3), NAN, device=DEV) for _ in range(2)]
        ops.pose_query_jvp(dev(r), dev(offsets), dev(c_t), dev(c_r), n_scenes=n_scenes, ld=ld, out=tuple(b[1:-1] for b in bufs))
        torch.cuda.synchronize()
        runs.append([b.cpu().numpy() for b in bufs])
    for k, (got, again) in enumerate(zip(*runs)):
        assert np.isnan(got[0]).all() and np.isnan(got[-1]).all()                      # guard scenes
        assert np.isnan(got[1:-1, n:]).all()                                           # pad rows left alone
        np.testing.assert_array_equal(got[1:-1, :n], again[1:-1, :n])
        for b in range(n_scenes):
            (l2, mx), = H.jvp_errors([got[1 + b, :n]], [ref[k]])
            assert l2 < 1e-5 and mx < 4e-5, (k, b, l2, mx)
        print(f'{representation} P={p}: max |gpu - host| {np.abs(got[1, :n] - host[k]).max():.3e}')


def guarded(shape):
    """A NaN-prefilled buffer with one guard row in front and behind; returns (whole, inner view)."""
    whole = torch.full((shape[0] + 2,) + tuple(shape[1:]), NAN, device=DEV)
    return whole, whole[1:-1]


def gpu_landscape(y, label, kind, weight):
    whole, g = guarded(y.shape)
    loss = torch.full((3,), NAN, device=DEV)
    y_d, label_d = dev(y), dev(label)
    rc = _lib.lib().mvnerf_landscape_loss(ops._p(y_d), ops._p(label_d), y.shape[0], y.shape[1], kind, weight, ops._p(g), ops._p(loss[1:]),
                                          None)
    assert rc == 0
    torch.cuda.synchronize()
    assert torch.isnan(whole[0]).all() and torch.isnan(whole[-1]).all() and torch.isnan(loss[0]) and torch.isnan(loss[2])
    return float(loss[1]), g.cpu().numpy().astype(np.float64)


def gpu_cosine(x, label, scale):
    whole, g = guarded(x.shape)
    loss = torch.full((3,), NAN, device=DEV)
    x_d, label_d = dev(x), dev(label)
    rc = _lib.lib().mvnerf_cosine_loss(ops._p(x_d), ops._p(label_d), x.shape[0], x.shape[1], scale, ops._p(g), ops._p(loss[1:]), None)
    assert rc == 0
    torch.cuda.synchronize()
    assert torch.isnan(whole[0]).all() and torch.isnan(whole[-1]).all() and torch.isnan(loss[0]) and torch.isnan(loss[2])
    return float(loss[1]), g.cpu().numpy().astype(np.float64)


@pytest.mark.parametrize('kind', [0, 1])
@pytest.mark.parametrize('b,n_p', [(1, 1), (2, 3), (7, 5), (300, 8)])                   # 300 rows: more than the workgroup's 256 threads
def test_landscape_loss_kernel(kind, b, n_p):
    y, label = H.landscape_case(b + n_p, b, n_p)
    if b == 7:
        y[0, 0] = 40.0
        label[1, 0] = 0.0
    value, g = gpu_landscape(y, label, kind, 0.7)
    ok_v, ok_g = H.check_loss(f'landscape kind={kind} B={b} np={n_p}', value, g, H.landscape_total, y, label, (kind, 0.7))
    assert ok_v and ok_g
    value2, g2 = gpu_landscape(y, label, kind, 0.7)
    assert value2 == value and np.array_equal(g, g2)


@pytest.mark.parametrize('dim', [3, 4, 6])
@pytest.mark.parametrize('rows', [1, 6, 300])
def test_cosine_loss_kernel(dim, rows):
    x, label = H.cosine_case(10 * dim + rows, rows, dim)
    if rows == 6:
        x[2] = (1e-8 * np.arange(1, dim + 1)).astype(F32)                               # below the 1e-12 clamp
    value, g = gpu_cosine(x, label, 2.0)
    ok_v, ok_g = H.check_loss(f'cosine dim={dim} rows={rows}', value, g, H.cosine_total, x, label, (2.0,))
    assert ok_v and ok_g
    value2, g2 = gpu_cosine(x, label, 2.0)
    assert value2 == value and np.array_equal(g, g2)


# ---- the whole step ---------------------------------------------------------------------------------------------------------------------------
CASES = {'v1b1p1_6d': (1, 1, 1, '6d'),                     # one pose: M = 1, 42 query rows
         'v1b2p3_q': (1, 2, 3, 'quaternion'),              # 252 query rows: a ragged tile; M = 6 is no multiple of 8
         'v2b2p3_6d': (2, 2, 3, '6d'),                     # two views: every scene's 126 rows padded to 128
         'v1b1p8_q': (1, 1, 8, 'quaternion')}              # M = 8: the batched GEMMs without pad rows
LOSSES = {'kl_divergence': (M.kl_divergence, True), 'cross_entropy': (M.categorical_crossentropy_from_logits, False)}


def case(name):
    n_views, batch, n_points, representation = CASES[name]
    # the seed rule of the test whose bars these are (tests/test_gpu_language_fused_tail.py: language_case(50 + n_views, ...))
    return language_case(50 + n_views, n_views, batch, n_points, representation)


def grad_of(model, k):
    ro = model.grasp_readout
    if k.startswith('ds'):
        lin = ro.activation_downscale[int(k[2])]
    elif k.startswith('comb'):
        lin = ro.combined_activation_downscale
    elif k.startswith('out'):
        lin = ro.output_layer
    else:
        blk = ro.block_0 if k.startswith('b0') else ro.block_1
        lin = {'l0': blk.layer_0, 'l1': blk.layer_1, 'sc': blk.shortcut}[k.split('.')[1]]
    g = lin.weight.grad.T if k.endswith('.k') else lin.bias.grad
    assert g is not None, k
    return g.detach().double().cpu().numpy().copy()


@functools.lru_cache(maxsize=None)
def reference(name):
    """float64, once per case: oracle train_losses (kl_divergence after the softmax) and, from the oracle's pieces, the cross-entropy of the
    same landscape prediction; the gradient of every term alone w.r.t. every read-out variable."""
    n_views, batch, n_points, representation = CASES[name]
    sc, inputs, labels, model = case(name)
    w = {k: v.detach().double().cpu().clone().requires_grad_(True) for k, v in keras_weights(model.grasp_readout).items()}
    net = T.unflatten_net(t64(sc['fine']))
    checks = torch.as_tensor(L.transforms_to_check(7))
    inp, lab = [t64(a) for a in inputs], [t64(a) for a in labels]
    _, kl, loss_t, loss_r, pred = L.train_losses(w, net, inp, lab, checks, n_points, t64(sc['features']), representation)
    y = L.call(w, net, L.compute_matrices(inp[0], inp[1], representation), checks, n_points, inp[4], t64(sc['features']), inp[5], inp[6])
    ce = -(lab[0] * torch.log_softmax(y, -1)).sum(-1).mean()
    keys = list(w)
    def grads(scalar):
        gs = torch.autograd.grad(scalar, [w[k] for k in keys], retain_graph=True, allow_unused=True)
        return {k: (np.zeros(tuple(w[k].shape)) if g is None else g.numpy()) for k, g in zip(keys, gs)}
    terms = {'kl_divergence': grads(kl.sum()), 'cross_entropy': grads(ce), 't': grads(loss_t), 'r': grads(loss_r)}
    values = {'kl_divergence': float(kl.detach().mean()), 'cross_entropy': float(ce.detach()), 't': float(loss_t.detach()),
              'r': float(loss_r.detach()), 'pred': pred.detach().numpy()}
    return keys, terms, values


def reference_grads(name, loss, weights=(1.0, 1.0, 1.0)):
    keys, terms, values = reference(name)
    times = CASES[name][1] if loss == 'kl_divergence' else 1            # the (B,) total is summed: the scalar cosine losses enter B times
    return {k: weights[0] * terms[loss][k] + times * (weights[1] * terms['t'][k] + weights[2] * terms['r'][k]) for k in keys}, values


def run_step(model, sc, inputs, labels, loss, **flags):
    fn, softmax = LOSSES[loss]
    model.softmax_before_loss = softmax
    model.compile(loss=fn, **flags)
    out, pred = model.loss_and_grads((inputs, labels), sc['features'])
    torch.cuda.synchronize()
    keys = list(keras_weights(model.grasp_readout))
    return {k: float(v) for k, v in out.items()}, pred.cpu().numpy(), {k: grad_of(model, k) for k in keys}


@pytest.mark.parametrize('loss', list(LOSSES))
@pytest.mark.parametrize('name', list(CASES))
def test_fused_step_matches_float64_and_the_path_it_replaces(name, loss):
    sc, inputs, labels, model = case(name)
    ref, values = reference_grads(name, loss)
    out_old, _, g_old = run_step(model, sc, inputs, labels, loss, fused_tail=True, fused_step=False)
    out, pred, g_new = run_step(model, sc, inputs, labels, loss, fused_step=True)
    assert model.fused_step is True
    assert pred.shape == values['pred'].shape
    print(f'{name} {loss}: losses fused {out}, autograd {out_old}, float64 ' + str({k: v for k, v in values.items() if k != 'pred'}))
    top = max(1.0, float(np.abs(values['pred']).max()))
    scalars = [('prediction', float(np.abs(pred - values['pred']).max()), 1e-4 * top),
               ('pred', abs(out['pred'] - float(values['pred'].mean())), 1e-4 * top),
               ('landscape_loss', abs(out['landscape_loss'] - values[loss]), 1e-4 * max(1.0, abs(values[loss]))),
               ('grad_loss_t', abs(out['grad_loss_t'] - values['t']), 5e-3), ('grad_loss_r', abs(out['grad_loss_r'] - values['r']), 5e-3)]
    worst, failed = 0.0, [(k, e, bar) for k, e, bar in scalars if not e < bar]
    for k, r in ref.items():
        e_new, e_old, nr = np.linalg.norm(g_new[k] - r), np.linalg.norm(g_old[k] - r), np.linalg.norm(r)
        worst = max(worst, e_new)
        print(f'{name} {loss} {k}: |g - ref| fused_step {e_new:.3e}, autograd + fused_tail {e_old:.3e}, |ref| {nr:.3e}')
        if not (e_new < 3e-2 * nr + 1e-6 and e_new <= 4.0 * e_old + 1e-6):
            failed.append((k, e_new, e_old, nr))
    assert not failed, failed
    assert worst > 0.0


@pytest.mark.parametrize('name,loss', [('v1b2p3_q', 'kl_divergence'), ('v2b2p3_6d', 'cross_entropy')])
@pytest.mark.parametrize('weights', [(1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0)])
def test_each_loss_term_alone_matches_float64(name, loss, weights):
    """One term at a time: a contribution dropped from the step cannot hide under a larger one."""
    sc, inputs, labels, model = case(name)
    ref, _ = reference_grads(name, loss, weights)
    _, _, g = run_step(model, sc, inputs, labels, loss, fused_step=True, loss_weights=weights)
    _, _, g_old = run_step(model, sc, inputs, labels, loss, fused_tail=True, fused_step=False, loss_weights=weights)
    failed, total = [], 0.0
    for k, r in ref.items():
        e, e_old, nr = np.linalg.norm(g[k] - r), np.linalg.norm(g_old[k] - r), np.linalg.norm(r)
        total += nr
        print(f'{name} {loss} w={weights} {k}: |g - ref| {e:.3e} (autograd path {e_old:.3e}), |ref| {nr:.3e}')
        if not e < 3e-2 * nr + 1e-6:
            failed.append((k, e, nr))
    assert not failed, failed
    assert total > 0.0


def ctypes_step(lib, model, fs, state, inputs_dev, labels_dev, kind):
    """mvnerf_language_loss_and_grads filled field by field from raw pointers - nothing of ops.language_call."""
    ro = model.grasp_readout
    b0, b1, out = ro.block_0, ro.block_1, ro.output_layer
    fs['w4'].copy_(torch.stack([lin.weight.detach() for lin in ro.activation_downscale]))
    fs['b4'].copy_(torch.stack([lin.bias.detach() for lin in ro.activation_downscale]))
    c = _lib.LanguageCall()
    images, features, intrinsics, extrinsics_inv = state.geo
    c.images, c.features, c.intrinsics, c.extrinsics_inv = (t.data_ptr() for t in state.geo)
    c.B, c.V, c.H, c.W = images.shape[:4]
    c.packed_net, c.split, c.bwd_streams = state.packed.data_ptr(), state.packed_split.data_ptr(), state.bwd_streams.data_ptr()
    c.head_w4, c.head_b4 = fs['w4'].data_ptr(), fs['b4'].data_ptr()
    c.head_wc, c.head_bc = ro.combined_activation_downscale.weight.data_ptr(), ro.combined_activation_downscale.bias.data_ptr()
    for i, t in enumerate((b0.layer_0.weight, b0.layer_0.bias, b0.layer_1.weight, b0.layer_1.bias, b0.shortcut.weight, b1.layer_0.weight,
                           b1.layer_0.bias, b1.layer_1.weight, b1.layer_1.bias, out.weight, out.bias)):
        c.tail_w[i] = t.data_ptr()
    c.offsets = model.transforms_to_check.data_ptr()
    c.rep, c.np, c.n5 = (0 if model.rotations.shape[-1] == 4 else 1), model.n_points_train, model.n_transforms_to_check
    c.t_landscape, c.rot_landscape, c.t_grad, c.rot_grad = (t.data_ptr() for t in inputs_dev[:4])
    c.label_landscape, c.label_grad_t, c.label_grad_r = (t.data_ptr() for t in labels_dev)
    c.loss_kind, c.w_land, c.w_t, c.w_r = kind, 1.0, 1.0, 1.0
    c.grads, c.prediction, c.scalars = fs['grads'].data_ptr(), fs['prediction'].data_ptr(), fs['scalars'].data_ptr()
    c.workspace, c.workspace_bytes = fs['workspace'].data_ptr(), fs['workspace'].numel()
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert lib.mvnerf_language_loss_and_grads(ctypes.byref(c), stream) == 0, lib.mvnerf_last_error()


@pytest.mark.parametrize('name', ['v1b2p3_q', 'v1b1p1_6d'])
def test_step_through_ctypes_alone_reproduces_the_python_path(name):
    """Three steps, optimiser included, at V = 1 (no unordered sum anywhere): the same bits."""
    lib = _lib.lib()
    n_views, batch, n_points, representation = CASES[name]
    sc, inputs, labels, model = case(name)
    twin = case(name)[3]
    model.compile(learning_rate=1e-3, fused_step=True)
    opt = torch.optim.Adam(twin.grasp_readout.parameters(), lr=1e-3, eps=1e-7)
    n5 = twin.n_transforms_to_check
    layout, total = ops.language_grad_layout(n5)
    assert total == lib.mvnerf_language_grad_floats(n5)
    h, w = sc['images'].shape[2:4]
    need = lib.mvnerf_language_workspace_bytes(batch, n_views, h, w, n_points, n5)
    fs = {'w4': torch.empty(4, 64, 128, device=DEV), 'b4': torch.empty(4, 64, device=DEV), 'grads': torch.full((total,), NAN, device=DEV),
          'prediction': torch.full((batch, n_points), NAN, device=DEV), 'scalars': torch.full((4,), NAN, device=DEV),
          'workspace': torch.full((need // 4,), NAN, device=DEV).view(torch.uint8)}          # NaN: the step relies on nothing it did not write
    ro = twin.grasp_readout
    b0, b1 = ro.block_0, ro.block_1
    views = {'wc': ro.combined_activation_downscale.weight, 'bc': ro.combined_activation_downscale.bias, 'w0': b0.layer_0.weight,
             'b0': b0.layer_0.bias, 'w1': b0.layer_1.weight, 'b1': b0.layer_1.bias, 'ws': b0.shortcut.weight, 'w0b': b1.layer_0.weight,
             'b0b': b1.layer_0.bias, 'w1b': b1.layer_1.weight, 'b1b': b1.layer_1.bias, 'w_out': ro.output_layer.weight,
             'b_out': ro.output_layer.bias}
    rng = np.random.default_rng(3)
    for step in range(3):
        moved = tuple((a + 0.02 * rng.standard_normal(a.shape)).astype(np.float32) for a in inputs[:4]) + tuple(inputs[4:])
        out = model.train_step((moved, labels), sc['features'])
        state = twin.trunk_state(moved, sc['features'])
        ctypes_step(lib, twin, fs, state, [dev(a) for a in moved[:4]], [dev(a) for a in labels], 0)
        flat = fs['grads']
        def view(n):
            o, shape = layout[n]
            return flat[o:o + int(np.prod(shape))].view(shape)
        for n, prm in views.items():
            prm.grad = view(n).clone()
        for k, lin in enumerate(ro.activation_downscale):
            lin.weight.grad, lin.bias.grad = view('w4')[k].clone(), view('b4')[k].clone()
        for prm in ro.parameters():
            prm.grad.clamp_(-1.0, 1.0)
        opt.step()
        torch.cuda.synchronize()
        got = fs['scalars'].cpu().numpy()
        want = np.array([float(out[k]) for k in ('landscape_loss', 'grad_loss_t', 'grad_loss_r', 'pred')], np.float32)
        np.testing.assert_array_equal(got, want)
        assert np.isfinite(got).all()
        for (n, a), (_, b) in zip(model.grasp_readout.named_parameters(), twin.grasp_readout.named_parameters()):
            assert torch.equal(a, b), (step, n)


@pytest.mark.parametrize('name,exact', [('v1b2p3_q', True), ('v2b2p3_6d', False)])
def test_fused_step_graph_replay_matches_eager(name, exact):
    """compile(graph=True, fused_step=True): two eager steps, one capture, replays - against a twin stepping eagerly on the same changing
    inputs at learning rate 0.  V = 1: the same bits; V > 1 (mvnerf_query_vjp's view sum uses atomics): 1e-5, as the fused-tail replay test."""
    steps = 5
    sc, inputs, labels, eager = case(name)
    graphed = case(name)[3]
    rng = np.random.default_rng(7)
    datas = [((*[(a + 0.05 * rng.standard_normal(a.shape)).astype(np.float32) for a in inputs[:4]], *inputs[4:]), labels) for _ in range(steps)]
    eager.compile(learning_rate=0.0, fused_step=True)
    graphed.compile(learning_rate=0.0, graph=True, fused_step=True)
    seen = []
    for step, data in enumerate(datas):
        out_e = eager.train_step(data, sc['features'])
        out_g = graphed.train_step(data, sc['features'])
        for k in out_e:
            a, b = float(out_e[k]), float(out_g[k])
            assert np.isfinite(a) and (a == b if exact else abs(a - b) < 1e-5 * max(1.0, abs(a))), (step, k, a, b)
        seen.append(float(out_g['grad_loss_t']))
    assert graphed._graph is not None
    assert min(abs(a - b) for a, b in zip(seen[2:], seen[3:])) > 1e-4, seen               # replays follow the staged inputs
    graphed.compile(learning_rate=0.0, graph=True, fused_step=False)                      # changing the flag drops the captured graph
    assert graphed._graph is None and graphed.fused_step is False


def test_fused_step_off_gives_the_bits_it_gave_before():
    name = 'v1b2p3_q'
    sc, inputs, labels, untouched = case(name)
    toggled = case(name)[3]
    assert untouched.fused_step is False
    before = run_step(untouched, sc, inputs, labels, 'kl_divergence')
    run_step(toggled, sc, inputs, labels, 'kl_divergence', fused_step=True)
    after = run_step(toggled, sc, inputs, labels, 'kl_divergence', fused_step=False)
    assert before[0] == after[0]
    np.testing.assert_array_equal(before[1], after[1])
    for k in before[2]:
        np.testing.assert_array_equal(before[2][k], after[2][k])
