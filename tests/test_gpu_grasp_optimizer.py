"""The grasp-pose optimiser on the GPU (thesis_clip_nerf_amd/grasp_optimizer.py, csrc/pose_ops.hip): the three pose kernels against
float64, the whole step's gradient d(-sum success)/d(t, rot) against float64 autograd through the oracle restatement
(oracle/lmvnerf_torch.call), and compute_results end to end.  Bars for the whole step are test_gpu_query.py's: the trunk's positional
encoding has gain pi * 2^9, so fp32 first derivatives agree to ~1e-3 relative and a relu flip can move a single row."""
import numpy as np
import pytest
import torch

from oracle import lmvnerf_torch as L
from oracle import mvnerf_torch as T
from tests.test_pose_math_cpu import REPS, post_process_ref, query_ref, random_poses
from thesis_clip_nerf_amd import ops
from thesis_clip_nerf_amd.encoders import KerasAdam as TorchKerasAdam
from thesis_clip_nerf_amd.grasp_optimizer import DNGFOptimizer, KerasAdam, best_grasps, compute_results, optimize_pose
from thesis_clip_nerf_amd.lmvnerf import LanguageNeRF
from thesis_clip_nerf_amd.synthetic import make_scene

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
F32 = np.float32
BOUNDS = ((-0.15, 0.15), (-0.15, 0.15), (-0.1, 0.1))       # around the synthetic scenes' look-at centre


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def t64(a):
    return torch.as_tensor(np.asarray(a)).to(torch.float64)


def grasp_case(seed, n_images, n_views, representation, n_poses, clip_translation=True):
    sc = make_scene(seed=seed, batch=1, n_views=n_images, height=16, width=20, n_rays=4, bias_scale=0.05)
    torch.manual_seed(seed)
    model = LanguageNeRF(sc['fine'], n_views=n_views, rotation_representation=representation, device=DEV)
    opt = DNGFOptimizer(model, BOUNDS, n_initial_guesses=n_poses, n_images=n_images, clip_translation=clip_translation,
                        rotation_representation=representation)
    inputs = [dev(sc['images']), dev(sc['intrinsics']), dev(sc['extrinsics_inv'])]
    return sc, model, opt, inputs, dev(sc['features'])


@pytest.mark.parametrize('representation', ['quaternion', '6d'])
def test_pose_query_points_match_float64_and_the_matrix_path(representation):
    _, model, opt, _, _ = grasp_case(1, 3, 1, representation, 37)
    rep, rd = REPS[representation]
    t, r = random_poses(np.random.default_rng(2), 37, rd)
    offsets = model.transforms_to_check
    n = 37 * offsets.shape[0]
    points, dirs = ops.pose_query_points(dev(t), dev(r), offsets, n_scenes=3)
    torch.cuda.synchronize()
    ref_p, ref_d = query_ref(t64(t), t64(r), representation, offsets.cpu().numpy())
    for b in range(3):
        assert torch.equal(points[b], points[0]) and torch.equal(dirs[b], dirs[0])      # B identical copies
    got_p, got_d = points[0].cpu().numpy(), dirs[0].cpu().numpy()
    assert np.abs(got_p - ref_p.numpy()).max() < 1e-6 * np.abs(ref_p.numpy()).max()
    assert np.abs(got_d - ref_d.numpy()).max() < 1e-6 * np.abs(ref_d.numpy()).max()
    # the same order and values as LanguageNeRF._query_points on the tiled compute_matrices (grasp_optimizer.py:96-98)
    opt.set_initial_guesses([t[None], r[None]])
    mp, md = model._query_points(opt.compute_matrices().expand(3, -1, -1, -1))
    assert mp.shape == (3, n, 3)
    assert (mp - points).abs().max().item() < 2e-6 and (md - dirs).abs().max().item() < 2e-6
    # rows past P * n5 of a padded scene are left alone
    pad_p, pad_d = (torch.full((2, n + 14, 3), 7.0, device=DEV) for _ in range(2))
    ops.pose_query_points(dev(t), dev(r), offsets, n_scenes=2, ld=n + 14, out=(pad_p, pad_d))
    assert torch.equal(pad_p[:, :n], points[:2]) and torch.equal(pad_d[:, :n], dirs[:2])
    assert (pad_p[:, n:] == 7.0).all() and (pad_d[:, n:] == 7.0).all()


@pytest.mark.parametrize('representation', ['quaternion', '6d'])
@pytest.mark.parametrize('n_scenes,pad', [(1, 0), (3, 0), (2, 10)])
def test_pose_query_vjp_matches_float64_and_is_deterministic(representation, n_scenes, pad):
    rep, rd = REPS[representation]
    rng = np.random.default_rng(3 + n_scenes + rep)
    offsets = dev(L.transforms_to_check(7).astype(F32))
    p, n5 = 37, 42
    t, r = random_poses(rng, p, rd)
    ld = p * n5 + pad
    dp = rng.standard_normal((n_scenes, ld, 3)).astype(F32)
    dd = rng.standard_normal((n_scenes, ld, 3)).astype(F32)
    d_t, d_r = ops.pose_query_vjp(dev(r), offsets, dev(dp), dev(dd), scale=-1.0)
    d_t2, d_r2 = ops.pose_query_vjp(dev(r), offsets, dev(dp), dev(dd), scale=-1.0)
    torch.cuda.synchronize()
    assert torch.equal(d_t, d_t2) and torch.equal(d_r, d_r2)
    tt, rr = t64(t).requires_grad_(True), t64(r).requires_grad_(True)
    pts, drs = query_ref(tt, rr, representation, offsets.cpu().numpy())
    loss = -sum((t64(dp[b, :p * n5]) * pts).sum() + (t64(dd[b, :p * n5]) * drs).sum() for b in range(n_scenes))
    g_t, g_r = torch.autograd.grad(loss, (tt, rr))
    for got, ref in ((d_t, g_t), (d_r, g_r)):
        got, ref = got.cpu().numpy(), ref.numpy()
        assert np.linalg.norm(got - ref) / np.linalg.norm(ref) < 1e-5


@pytest.mark.parametrize('representation', ['quaternion', '6d'])
def test_pose_adam_step_matches_keras_closed_form(representation):
    rep, rd = REPS[representation]
    rng = np.random.default_rng(11 + rep)
    p = 300
    lr, decay = (0.05, 0.04), (0.9, 0.09)
    bounds = np.array(BOUNDS)
    t, r = random_poses(rng, p, rd)
    t0, r0 = post_process_ref(t64(t), t64(r), representation, bounds, True)
    t, r = dev(t0.numpy().astype(F32)), dev(r0.numpy().astype(F32))
    m_t, v_t, m_r, v_r = (torch.zeros_like(a) for a in (t, t, r, r))
    counters, flags = torch.zeros((2, p), dtype=torch.int32, device=DEV), torch.zeros(2, dtype=torch.int32, device=DEV)
    cfg = ops.pose_adam_config(lr0=lr, decay=decay, clip_translation=True, bounds=bounds)
    tv, rv = t0.clone().requires_grad_(True), r0.clone().requires_grad_(True)
    opts = [TorchKerasAdam([tv], lr=lr[0], eps=1e-7), TorchKerasAdam([rv], lr=lr[1], eps=1e-7)]
    ks = [0, 0]
    for phase in [(1, 0)] * 5 + [(0, 1)] * 5 + [(1, 1)] * 3:
        flags[0].fill_(phase[0])
        flags[1].fill_(phase[1])
        g_t = (1.5 * rng.standard_normal((p, 3))).astype(F32)
        g_r = (1.5 * rng.standard_normal((p, rd))).astype(F32)
        ops.pose_adam_step(cfg, flags, counters, dev(g_t), dev(g_r), m_t, v_t, m_r, v_r, t, r)
        for i, (var, g) in enumerate(((tv, g_t), (rv, g_r))):
            if phase[i]:
                ks[i] += 1
                opts[i].param_groups[0]['lr'] = lr[i] * decay[i] ** (ks[i] - 1)
                var.grad = t64(np.clip(g, -1.0, 1.0))
                opts[i].step()
        with torch.no_grad():
            a, b = post_process_ref(tv, rv, representation, bounds, True)
            tv.copy_(a)
            rv.copy_(b)
        c = counters.cpu().numpy()
        assert (c[0] == ks[0]).all() and (c[1] == ks[1]).all()          # only the trained variable's counter advances
        assert np.abs(t.cpu().numpy() - tv.detach().numpy()).max() < 1e-6
        assert np.abs(r.cpu().numpy() - rv.detach().numpy()).max() < 1e-6


def rel(got, ref):
    return float(np.linalg.norm(got - ref) / max(np.linalg.norm(ref), 1e-30))


def check_close(got, ref, name):
    """test_gpu_query.py's bars: relative L2 < 3e-2 and median per-pose relative error < 3e-3."""
    rows = np.linalg.norm((got - ref).reshape(-1, ref.shape[-1]), axis=-1) / np.maximum(
        np.linalg.norm(ref.reshape(-1, ref.shape[-1]), axis=-1), 1e-30)
    assert rel(got, ref) < 3e-2, (name, rel(got, ref))
    assert np.median(rows) < 3e-3, (name, float(np.median(rows)))


@pytest.mark.parametrize('representation', ['quaternion', '6d'])
@pytest.mark.parametrize('n_images,n_views', [(1, 1), (3, 1), (2, 2)])
def test_step_gradient_matches_float64_autograd(representation, n_images, n_views):
    from tests.test_oracle_lmvnerf import keras_weights
    p = 37
    sc, model, opt, inputs, feats = grasp_case(20 + n_images + n_views, n_images, n_views, representation, p)
    rng = np.random.default_rng(21)
    rd = REPS[representation][1]
    t = rng.uniform(np.array(BOUNDS)[:, 0], np.array(BOUNDS)[:, 1], (1, p, 3)).astype(F32)
    r = rng.standard_normal((1, p, rd)).astype(F32)
    if rd == 4:
        r /= np.linalg.norm(r, axis=-1, keepdims=True)
    opt.set_initial_guesses([t, r])
    opt.compile()
    opt.bind(inputs, feats)
    success, g_t, g_r = opt.success_and_gradients()
    torch.cuda.synchronize()
    b = n_images // n_views
    w = {k: v.detach().double().cpu() for k, v in keras_weights(model.grasp_readout).items()}
    net = T.unflatten_net(t64(sc['fine']))
    grp = lambda a: t64(a).reshape((b, n_views) + a.shape[2:])
    tt, rr = t64(t).requires_grad_(True), t64(r).requires_grad_(True)
    mats = L.compute_matrices(tt, rr, representation).expand(b, -1, -1, -1)
    ref = L.call(w, net, mats, torch.as_tensor(L.transforms_to_check(7)), p, grp(sc['images']), grp(sc['features']), grp(sc['intrinsics']),
                 grp(sc['extrinsics_inv']))
    rg_t, rg_r = torch.autograd.grad(-ref.sum(), (tt, rr))
    s_ref = ref.detach().numpy()
    assert success.shape == (b, p)
    assert np.abs(success.cpu().numpy() - s_ref).max() < 1e-4 * max(1.0, np.abs(s_ref).max())
    check_close(g_t.cpu().numpy(), rg_t[0].numpy(), 'd_t')
    check_close(g_r.cpu().numpy(), rg_r[0].numpy(), 'd_rot')
    # the summed success of compute_current_grasp_success is the same forward
    cur = opt.compute_current_grasp_success(inputs, feats)
    assert cur.shape == (p, 1)
    assert torch.equal(cur[:, 0], success.sum(0))


def _poses_ok(grasps, bounds):
    t = grasps[:, :3, 3]
    b = np.array(bounds, dtype=F32)
    assert (t >= b[:, 0]).all() and (t <= b[:, 1]).all()
    np.testing.assert_allclose(np.linalg.norm(grasps[:, :3, 0], axis=-1), 1.0, atol=1e-5)
    np.testing.assert_allclose(np.linalg.norm(grasps[:, :3, 1], axis=-1), 1.0, atol=1e-5)


@pytest.mark.parametrize('representation', ['quaternion', '6d'])
def test_compute_results_structure_bounds_and_reproducibility(representation):
    p, steps = 256, 3
    _, _, opt, inputs, feats = grasp_case(40, 3, 1, representation, p)
    kw = dict(n_optimization_steps=steps, init_lr_t=0.05, decay_t=0.9, init_lr_r=0.05, decay_r=0.09)
    out = compute_results(opt, inputs, feats, True, rng=np.random.default_rng(0), **kw)
    losses_t, losses_r, grasps_t, grasps_r, duration, all_poses = out
    assert losses_t.shape == (p,) and losses_r.shape == (p,)
    assert grasps_t.shape == (p, 4, 4) and grasps_r.shape == (p, 4, 4)
    assert duration > 0.0
    assert len(all_poses) == 1 + 2 * (steps + 1)
    for g in (grasps_t, grasps_r, *all_poses[1:]):
        _poses_ok(g, BOUNDS)
    assert np.isfinite(losses_t).all() and np.isfinite(losses_r).all()
    assert not np.array_equal(grasps_t[:, :3, 3], all_poses[0][:, :3, 3])             # the t phase moved the translations ...
    np.testing.assert_allclose(grasps_t[:, :3, :3], all_poses[0][:, :3, :3], atol=1e-6)  # ... and not the rotations (renormalised only)
    np.testing.assert_array_equal(grasps_r[:, :3, 3], grasps_t[:, :3, 3])              # the r phase leaves t alone
    c = opt._counters.cpu().numpy()
    assert (c == steps).all()
    again = compute_results(opt, inputs, feats, False, rng=np.random.default_rng(0), **kw)
    for a, b in zip(out[:4], again[:4]):
        np.testing.assert_array_equal(a, b)
    assert again[5] == []
    idx, best, best_l = best_grasps(losses_r, grasps_r)
    assert list(idx) == list(np.argsort(losses_r)[-5:]) and best.shape == (5, 4, 4)
    assert (np.diff(best_l) >= 0).all()
    # a list of step counts continues the same optimisers; sync trains both variables in one phase
    out_l = compute_results(opt, inputs, feats, False, rng=np.random.default_rng(0), **dict(kw, n_optimization_steps=[1, 2]))
    assert (opt._counters.cpu().numpy() == 3).all() and out_l[0].shape == (p,)
    compute_results(opt, inputs, feats, False, rng=np.random.default_rng(0), sync=True, **kw)
    assert (opt._counters.cpu().numpy() == steps).all()


def test_graph_replay_equals_eager():
    """compile(graph=True): two eager steps, one capture, replays - for both phases (the phase is a device-side flag) against an eager
    twin on the same seed.  The replay runs the same kernels on the same data, so the results are the same bits."""
    p, steps = 256, 4
    _, _, eager, inputs, feats = grasp_case(50, 3, 1, '6d', p)
    _, _, graphed, _, _ = grasp_case(50, 3, 1, '6d', p)
    graphed.compile(graph=True)
    kw = dict(n_optimization_steps=steps, init_lr_t=0.05, decay_t=0.9, init_lr_r=0.05, decay_r=0.09)
    out_e = compute_results(eager, inputs, feats, True, rng=np.random.default_rng(1), **kw)
    out_g = compute_results(graphed, inputs, feats, True, rng=np.random.default_rng(1), **kw)
    assert graphed._graph is not None and eager._graph is None
    for a, b in zip(out_e[:4], out_g[:4]):
        np.testing.assert_array_equal(a, b)
    for a, b in zip(out_e[5], out_g[5]):
        np.testing.assert_array_equal(a, b)
    # a second compute_results on the same inputs keeps the captured step (the packed weights are refreshed in place)
    graph = graphed._graph
    again = compute_results(graphed, inputs, feats, False, rng=np.random.default_rng(1), **kw)
    assert graphed._graph is graph
    for a, b in zip(out_e[:4], again[:4]):
        np.testing.assert_array_equal(a, b)


def test_small_steps_raise_success():
    p = 256
    _, _, opt, inputs, feats = grasp_case(60, 3, 1, 'quaternion', p, clip_translation=False)
    opt.compile(optimizer=KerasAdam(2e-4, 1.0))
    t, r = opt.generate_initial_guesses(workspace_bounds=BOUNDS, rng=np.random.default_rng(2))
    opt.set_initial_guesses([t, r])
    before = opt.compute_current_grasp_success(inputs, feats).cpu().numpy()[:, 0]
    _, after, _, _ = optimize_pose(opt, inputs, feats, [True, False], n_optimization_steps=3)
    assert after.mean() >= before.mean(), (before.mean(), after.mean())
    assert (opt._counters.cpu().numpy()[0] == 3).all() and (opt._counters.cpu().numpy()[1] == 0).all()
