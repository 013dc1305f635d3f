"""GraspReadout.fused_tail / LanguageNeRF.compile(fused_tail=True): the per-pose layers of the read-out as fused HIP passes
(csrc/grasp_tail.hip, csrc/grasp_tail_train.hip) inside the module, the training step, its captured graph and inference, on the GPU.

(a) holds the fused path to the rule of tests/test_gpu_grasp_tail_train.py with the unfused path (today's default) as the yardstick: both
are measured against the module in float64 on the CPU, the fused path may have 4x the unfused path's relative L2 error (floor 2e-6), capped
at 1e-5 for the prediction and first gradients and 1e-4 for the gradients of a loss on d prediction / d acts.  (b)-(d) restate the cases
and bars of tests/test_gpu_query.py's training-step tests with the flag on."""
import copy

import numpy as np
import pytest
import torch

from oracle import mvnerf_torch as T
from tests import grasp_tail_ref as R
from thesis_clip_nerf_amd.synthetic import make_scene

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
FACTOR, FLOOR, CAP1, CAP2 = 4.0, 2e-6, 1e-5, 1e-4


def check(name, err_fused, err_unfused, cap):
    bar = min(max(FACTOR * err_unfused, FLOOR), cap)
    print(f'{name}: unfused {err_unfused:.3e}, fused {err_fused:.3e}, bar {bar:.3e}')
    assert err_fused <= bar, (name, err_fused, err_unfused, bar)


def readout_quantities(ro, acts, probe):
    """prediction, first gradients of pred.sum() w.r.t. acts and every parameter, and the gradients of <d pred / d acts, probe> w.r.t.
    every parameter (None where the graph does not reach one)."""
    a = acts.detach().clone().requires_grad_(True)
    params = list(ro.parameters())
    pred = ro(a)
    first = torch.autograd.grad(pred.sum(), [a] + params, create_graph=True)
    second = torch.autograd.grad((first[0] * probe).sum(), params, allow_unused=True)
    return pred.detach(), [g.detach() for g in first], second


@pytest.mark.parametrize('n_p', [5, 8])                    # M = 10 rows: a ragged tile, the _gtn products; M = 16: mvnerf_gemm_tn_batched
def test_grasp_readout_fused_tail_against_float64(n_p):
    ro = R.make_readout(42, 3).to(DEV)
    ro64 = copy.deepcopy(ro).double().cpu()
    g = torch.Generator().manual_seed(n_p)
    acts = torch.randn((4, 2, n_p, 42, 128), generator=g) * 0.7
    probe = torch.randn((4, 2, n_p, 42, 128), generator=g)
    ref = readout_quantities(ro64, acts.double(), probe.double())
    names = [n for n, _ in ro.named_parameters()]
    got = {}
    for fused in (False, True):
        ro.fused_tail = fused
        got[fused] = readout_quantities(ro, acts.to(DEV), probe.to(DEV))
    torch.cuda.synchronize()
    assert got[True][0].shape == (2, n_p)
    check(f'np={n_p} prediction', R.rel(got[True][0], ref[0]), R.rel(got[False][0], ref[0]), CAP1)
    for n, gf, gu, r in zip(['acts'] + names, got[True][1], got[False][1], ref[1]):
        check(f'np={n_p} d_{n}', R.rel(gf, r), R.rel(gu, r), CAP1)
    nonzero = 0
    for n, gf, gu, r in zip(names, got[True][2], got[False][2], ref[2]):
        if r is None or float(r.abs().max()) == 0.0:        # the output bias and block_1's last bias: identically zero
            assert gf is None or float(gf.abs().max()) == 0.0, n
            continue
        nonzero += 1
        check(f'np={n_p} dd_{n}', R.rel(gf, r), R.rel(gu, r), CAP2)
    assert nonzero == len(names) - 2


# ---- the training step (the helper of tests/test_gpu_query.py, restated) --------------------------------------------------------------------
def t64(a):
    return torch.as_tensor(np.asarray(a)).to(torch.float64)


def language_case(seed, n_views, batch, n_points, representation):
    from thesis_clip_nerf_amd.lmvnerf import LanguageNeRF
    sc = make_scene(seed=seed, batch=batch, n_views=n_views, height=16, width=20, n_rays=4, bias_scale=0.05)
    rng = np.random.default_rng(seed)
    rot_dim = 4 if representation == 'quaternion' else 6

    def poses():
        t = (np.array([0.0, 0.0, 0.8]) + 0.1 * rng.standard_normal((batch, n_points, 3))).astype(np.float32)
        r = rng.standard_normal((batch, n_points, rot_dim)).astype(np.float32)
        if representation == 'quaternion':
            r /= np.linalg.norm(r, axis=-1, keepdims=True)
        return t, r
    t1, r1 = poses()
    t2, r2 = poses()
    lab0 = rng.random((batch, n_points)).astype(np.float32)
    lab0 /= lab0.sum(-1, keepdims=True)
    labels = (lab0, rng.standard_normal((batch, n_points, 3)).astype(np.float32),
              rng.standard_normal((batch, n_points, rot_dim)).astype(np.float32))
    inputs = (t1, r1, t2, r2, sc['images'], sc['intrinsics'], sc['extrinsics_inv'])
    torch.manual_seed(seed)
    model = LanguageNeRF(sc['fine'], n_points_train=n_points, n_views=n_views, batch_size=batch,
                         rotation_representation=representation, softmax_before_loss=True, device=DEV)
    return sc, inputs, labels, model


@pytest.mark.parametrize('n_views,batch,representation', [(1, 1, '6d'), (2, 2, 'quaternion')])
def test_language_train_step_with_fused_tail_matches_restatement(n_views, batch, representation):
    from oracle import lmvnerf_torch as L
    from tests.test_oracle_lmvnerf import keras_weights
    n_points = 3
    sc, inputs, labels, model = language_case(50 + n_views, n_views, batch, n_points, representation)
    model.compile(fused_tail=True)
    assert model.grasp_readout.fused_tail is True
    out, pred = model.loss_and_grads((inputs, labels), sc['features'])
    torch.cuda.synchronize()
    w = {k: v.detach().double().cpu().clone().requires_grad_(True) for k, v in keras_weights(model.grasp_readout).items()}
    net = T.unflatten_net(t64(sc['fine']))
    checks = torch.as_tensor(L.transforms_to_check(7))
    loss, landscape, loss_t, loss_r, pred_ref = L.train_losses(w, net, [t64(a) for a in inputs], [t64(a) for a in labels], checks,
                                                               n_points, t64(sc['features']), representation)
    loss.sum().backward()
    assert np.abs(pred.cpu().numpy() - pred_ref.detach().numpy()).max() < 1e-4 * max(1.0, float(pred_ref.detach().abs().max()))
    assert abs(float(out['landscape_loss']) - float(landscape.detach().mean())) < 1e-4 * max(1.0, abs(float(landscape.detach().mean())))
    assert abs(float(out['grad_loss_t']) - float(loss_t.detach())) < 5e-3
    assert abs(float(out['grad_loss_r']) - float(loss_r.detach())) < 5e-3
    worst = 0.0
    for k, ref in w.items():                  # oracle name -> module parameter (Keras kernels are the transposed weights)
        if k.startswith('ds'):
            lin = model.grasp_readout.activation_downscale[int(k[2])]
        elif k.startswith('comb'):
            lin = model.grasp_readout.combined_activation_downscale
        elif k.startswith('out'):
            lin = model.grasp_readout.output_layer
        else:
            blk = model.grasp_readout.block_0 if k.startswith('b0') else model.grasp_readout.block_1
            lin = {'l0': blk.layer_0, 'l1': blk.layer_1, 'sc': blk.shortcut}[k.split('.')[1]]
        grad = lin.weight.grad.T if k.endswith('.k') else lin.bias.grad
        assert grad is not None, k
        g = grad.double().cpu().numpy()
        r = ref.grad.numpy()
        e = np.linalg.norm(g - r)
        worst = max(worst, e)
        print(f'{k}: |g - ref| {e:.3e}, |ref| {np.linalg.norm(r):.3e}')
        assert e < 3e-2 * np.linalg.norm(r) + 1e-6, (k, e, np.linalg.norm(r))
    assert worst > 0.0


def test_fused_tail_graph_replay_matches_eager():
    """compile(graph=True, fused_tail=True): two eager steps, one capture, replays - against a twin stepping eagerly with the same flag on
    the same changing inputs at learning rate 0 (the weights stand still: every step's losses agree to fp32 rounding)."""
    n_points, steps = 3, 5
    sc, inputs, labels, _ = language_case(70, 2, 2, n_points, '6d')
    rng = np.random.default_rng(7)
    datas = [((*[(a + 0.05 * rng.standard_normal(a.shape)).astype(np.float32) for a in inputs[:4]], *inputs[4:]), labels) for _ in range(steps)]
    eager, graphed = (language_case(70, 2, 2, n_points, '6d')[3] for _ in range(2))
    eager.compile(learning_rate=0.0, fused_tail=True)
    graphed.compile(learning_rate=0.0, graph=True, fused_tail=True)
    assert eager.grasp_readout.fused_tail and graphed.grasp_readout.fused_tail
    seen = []
    for step, data in enumerate(datas):
        out_e = eager.train_step(data, sc['features'])
        out_g = graphed.train_step(data, sc['features'])
        for k in out_e:
            assert abs(float(out_e[k]) - float(out_g[k])) < 1e-5 * max(1.0, abs(float(out_e[k]))), (step, k, float(out_e[k]), float(out_g[k]))
        seen.append(float(out_g['grad_loss_t']))
    assert graphed._graph is not None
    assert min(abs(a - b) for a, b in zip(seen[2:], seen[3:])) > 2e-3, seen           # replays follow the staged inputs
    graphed.compile(learning_rate=0.0, graph=True, fused_tail=False)                  # changing the flag drops the captured graph
    assert graphed._graph is None and graphed.grasp_readout.fused_tail is False


def test_infer_with_fused_tail_returns_the_unfused_scores():
    sc, inputs, labels, model = language_case(60, 1, 1, 2, '6d')
    model.set_pose(inputs[0], inputs[1])
    transforms = model.compute_matrices().detach()
    scores = {}
    for fused in (False, True):
        model.compile(fused_tail=fused)
        scores[fused] = model.infer(inputs, transforms, 2, sc['features'])
    torch.cuda.synchronize()
    assert scores[True].shape == (1, 2) and torch.isfinite(scores[True]).all()
    diff, top = (scores[True] - scores[False]).abs().max().item(), scores[False].abs().max().item()
    print(f'infer: max |fused - unfused| {diff:.3e}, max |score| {top:.3e}')
    assert diff < 1e-4 * max(1.0, top)
