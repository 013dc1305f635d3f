"""DNGFOptimizer(compute_dtype='bf16') on the GPU: the explicit, graph and fused modes against each other at the bars of
tests/test_gpu_grasp_step.py, against the float64 step within twice the error of the torch-CPU emulation of the bf16 path
(tests/trunk_vjp_bf16_ref.py), a three-step compute_results run, and mvnerf_grasp_opt_step_bf16 through ctypes alone."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import mvnerf_torch as T
from tests import trunk_vjp_bf16_ref as B
from tests.test_gpu_grasp_optimizer import BOUNDS, DEV, _poses_ok, check_close, dev, rel
from tests.test_gpu_grasp_step import float64_step, random_guesses
from tests.test_pose_math_cpu import REPS
from thesis_clip_nerf_amd import _lib
from thesis_clip_nerf_amd.grasp_optimizer import DNGFOptimizer, KerasAdam, compute_results
from thesis_clip_nerf_amd.lmvnerf import LanguageNeRF
from thesis_clip_nerf_amd.synthetic import make_scene

pytestmark = pytest.mark.gpu


def grasp_case_bf16(seed, n_images, n_views, representation, n_poses):
    """tests/test_gpu_grasp_optimizer.grasp_case with compute_dtype='bf16'."""
    sc = make_scene(seed=seed, batch=1, n_views=n_images, height=16, width=20, n_rays=4, bias_scale=0.05)
    torch.manual_seed(seed)
    model = LanguageNeRF(sc['fine'], n_views=n_views, rotation_representation=representation, device=DEV)
    opt = DNGFOptimizer(model, BOUNDS, n_initial_guesses=n_poses, n_images=n_images, clip_translation=True,
                        rotation_representation=representation, compute_dtype='bf16')
    return sc, model, opt, [dev(sc['images']), dev(sc['intrinsics']), dev(sc['extrinsics_inv'])], dev(sc['features'])


@pytest.mark.parametrize('representation,n_images,n_views', [('quaternion', 3, 1), ('6d', 2, 2), ('quaternion', 3, 3)])
def test_bf16_step_modes_agree_and_stay_within_twice_the_emulation_error(representation, n_images, n_views, monkeypatch):
    p = 37
    sc, model, opt, inputs, feats = grasp_case_bf16(70 + n_images, n_images, n_views, representation, p)
    t, r = random_guesses(p, REPS[representation][1], seed=5)
    opt.set_initial_guesses([t, r])
    opt.compile()
    opt.bind(inputs, feats)
    s_x, g_t, g_r = opt.success_and_gradients()
    s_x, gt_x, gr_x = s_x.cpu().numpy(), g_t.cpu().numpy(), g_r.cpu().numpy()
    opt.compile(fused=True)
    s_f, g_t, g_r = opt.success_and_gradients()
    torch.cuda.synchronize()
    s_f, gt_f, gr_f = s_f.cpu().numpy(), g_t.cpu().numpy(), g_r.cpu().numpy()
    assert opt._bound['fused']['nets16'] is not None
    assert np.abs(s_f - s_x).max() < 1e-4 * max(1.0, np.abs(s_x).max())
    check_close(gt_f, gt_x, 'd_t')
    check_close(gr_f, gr_x, 'd_rot')
    # against float64, with the error of the emulated bf16 path as the yardstick
    s_ref, rt_ref, rr_ref = float64_step(sc, model, t, r, representation, n_images, n_views, p)
    monkeypatch.setattr(T, 'mv_embedding', B.emulated_mv_embedding)
    s_em, rt_em, rr_em = float64_step(sc, model, t, r, representation, n_images, n_views, p)
    for name, got, em, ref in (('success', s_f, s_em, s_ref), ('g_t', gt_f, rt_em, rt_ref), ('g_rot', gr_f, rr_em, rr_ref)):
        e_k, e_emul = rel(got, ref), rel(em, ref)
        print(f'{representation} {n_images}/{n_views} {name}: e_kernel = {e_k:.3e}, e_emul = {e_emul:.3e}, ratio {e_k / e_emul:.2f}')
        assert e_k <= 2 * e_emul, name


@pytest.mark.parametrize('fused', [False, True])
def test_bf16_graph_replay_equals_eager(fused):
    p, steps = 64, 4
    _, _, eager, inputs, feats = grasp_case_bf16(50, 3, 1, '6d', p)
    _, _, graphed, _, _ = grasp_case_bf16(50, 3, 1, '6d', p)
    eager.compile(fused=fused)
    graphed.compile(graph=True, fused=fused)
    kw = dict(n_optimization_steps=steps, init_lr_t=0.05, decay_t=0.9, init_lr_r=0.05, decay_r=0.09)
    out_e = compute_results(eager, inputs, feats, True, rng=np.random.default_rng(1), **kw)
    out_g = compute_results(graphed, inputs, feats, True, rng=np.random.default_rng(1), **kw)
    assert graphed._graph is not None and eager._graph is None
    for a, b in zip(out_e[:4], out_g[:4]):
        np.testing.assert_array_equal(a, b)
    for a, b in zip(out_e[5], out_g[5]):
        np.testing.assert_array_equal(a, b)


def test_bf16_compute_results_structure_bounds_and_reproducibility():
    p, steps = 128, 3
    _, _, opt, inputs, feats = grasp_case_bf16(40, 3, 1, 'quaternion', p)
    opt.compile(fused=True)
    kw = dict(n_optimization_steps=steps, init_lr_t=0.05, decay_t=0.9, init_lr_r=0.05, decay_r=0.09)
    out = compute_results(opt, inputs, feats, True, rng=np.random.default_rng(0), **kw)
    losses_t, losses_r, grasps_t, grasps_r, duration, all_poses = out
    assert opt._fused is True and opt.compute_dtype == 'bf16'
    assert losses_t.shape == (p,) and losses_r.shape == (p,) and grasps_t.shape == (p, 4, 4) and grasps_r.shape == (p, 4, 4)
    assert duration > 0.0 and len(all_poses) == 1 + 2 * (steps + 1)
    for g in (grasps_t, grasps_r, *all_poses[1:]):
        _poses_ok(g, BOUNDS)
    assert np.isfinite(losses_t).all() and np.isfinite(losses_r).all()
    assert not np.array_equal(grasps_t[:, :3, 3], all_poses[0][:, :3, 3])
    np.testing.assert_array_equal(grasps_r[:, :3, 3], grasps_t[:, :3, 3])
    assert (opt._counters.cpu().numpy() == steps).all()
    again = compute_results(opt, inputs, feats, False, rng=np.random.default_rng(0), **kw)
    for a, b in zip(out[:4], again[:4]):
        np.testing.assert_array_equal(a, b)


def test_c_abi_bf16_grasp_step_through_ctypes():
    """One mvnerf_grasp_opt_step_bf16 on the bound buffers of a second optimiser equals optimize_pose of the first."""
    p = 37
    lr, decay = (0.05, 0.05), (0.9, 0.09)
    pair = []
    for _ in range(2):
        _, _, opt, inputs, feats = grasp_case_bf16(83, 3, 1, 'quaternion', p)
        opt.compile(optimizer=[KerasAdam(lr[0], decay[0]), KerasAdam(lr[1], decay[1])], fused=True)
        opt.set_initial_guesses(list(random_guesses(p, 4, seed=8)))
        opt.bind(inputs, feats)
        pair.append((opt, inputs, feats))
    (a, inputs, feats), (b, _, _) = pair
    a.optimize_pose(inputs, feats, [True, True])
    lib = _lib.lib()
    ptr = lambda x: ctypes.c_void_p(x.data_ptr())
    fs, st = b._fused_state(), b._bound['state']
    b.set_train_config([True, True])
    need = lib.mvnerf_grasp_workspace_bytes_bf16(3, 1, p, 42)
    assert fs['ws'].numel() == need and need < lib.mvnerf_grasp_workspace_bytes(3, 1, p, 42)
    step = lambda: lib.mvnerf_grasp_opt_step_bf16(ctypes.byref(fs['call']), ptr(st.packed16), ptr(st.bwd16), ctypes.byref(b._adam_cfg), ptr(b._flags),
                                                  ptr(b._counters), ptr(b._m_t), ptr(b._v_t), ptr(b._m_r), ptr(b._v_r), None)
    fs['call'].workspace_bytes = need - 1
    assert step() == -1 and b'workspace' in lib.mvnerf_last_error()
    fs['call'].workspace_bytes = need
    assert step() == 0, lib.mvnerf_last_error()
    torch.cuda.synchronize()
    assert torch.equal(a.translations, b.translations) and torch.equal(a.rotations, b.rotations)
    assert torch.equal(a._bound['fused']['success'], fs['success']) and (b._counters == 1).all()
