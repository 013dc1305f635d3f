"""The grasp-pose optimisation step behind the C ABI (csrc/grasp_api.hip) on the GPU: `DNGFOptimizer.compile(fused=True)` against float64
autograd through the oracle restatement with tests/test_gpu_grasp_optimizer.py's bars, against the torch path on the same state,
compute_results end to end (eager and graph replay), and the same step driven through ctypes alone."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import lmvnerf_torch as L
from oracle import mvnerf_torch as T
from tests.test_gpu_grasp_optimizer import BOUNDS, DEV, F32, _poses_ok, check_close, dev, grasp_case, t64
from tests.test_pose_math_cpu import REPS
from thesis_clip_nerf_amd import _lib
from thesis_clip_nerf_amd.grasp_optimizer import DNGFOptimizer, KerasAdam, best_grasps, compute_results
from thesis_clip_nerf_amd.lmvnerf import LanguageNeRF
from thesis_clip_nerf_amd.synthetic import make_scene

pytestmark = pytest.mark.gpu


def random_guesses(p, rd, seed=21):
    rng = np.random.default_rng(seed)
    t = rng.uniform(np.array(BOUNDS)[:, 0], np.array(BOUNDS)[:, 1], (1, p, 3)).astype(F32)
    r = rng.standard_normal((1, p, rd)).astype(F32)
    if rd == 4:
        r /= np.linalg.norm(r, axis=-1, keepdims=True)
    return t, r


def small_offsets_case(seed, n_images, n_views, representation, n_poses, n_5d_poses):
    """grasp_case with another number of gripper offsets, and read-out biases that are not zero."""
    sc = make_scene(seed=seed, batch=1, n_views=n_images, height=16, width=20, n_rays=4, bias_scale=0.05)
    torch.manual_seed(seed)
    model = LanguageNeRF(sc['fine'], n_views=n_views, n_5d_poses=n_5d_poses, rotation_representation=representation, device=DEV)
    with torch.no_grad():
        ro = model.grasp_readout
        for lin in (ro.block_0.layer_0, ro.block_0.layer_1, ro.block_1.layer_0, ro.block_1.layer_1, ro.output_layer):
            lin.bias.normal_(0.0, 0.05)
    opt = DNGFOptimizer(model, BOUNDS, n_initial_guesses=n_poses, n_images=n_images, clip_translation=True, rotation_representation=representation)
    return sc, model, opt, [dev(sc['images']), dev(sc['intrinsics']), dev(sc['extrinsics_inv'])], dev(sc['features'])


def float64_step(sc, model, t, r, representation, n_images, n_views, p, n_5d_poses=7):
    from tests.test_oracle_lmvnerf import keras_weights
    b = n_images // n_views
    w = {k: v.detach().double().cpu() for k, v in keras_weights(model.grasp_readout).items()}
    net = T.unflatten_net(t64(sc['fine']))
    grp = lambda a: t64(a).reshape((b, n_views) + a.shape[2:])
    tt, rr = t64(t).requires_grad_(True), t64(r).requires_grad_(True)
    mats = L.compute_matrices(tt, rr, representation).expand(b, -1, -1, -1)
    ref = L.call(w, net, mats, torch.as_tensor(L.transforms_to_check(n_5d_poses)), p, grp(sc['images']), grp(sc['features']),
                 grp(sc['intrinsics']), grp(sc['extrinsics_inv']))
    rg_t, rg_r = torch.autograd.grad(-ref.sum(), (tt, rr))
    return ref.detach().numpy(), rg_t[0].numpy(), rg_r[0].numpy()


def check_fused_step(sc, model, opt, inputs, feats, representation, n_images, n_views, p, n_5d_poses=7):
    t, r = random_guesses(p, REPS[representation][1])
    opt.set_initial_guesses([t, r])
    opt.compile(fused=True)
    opt.bind(inputs, feats)
    success, g_t, g_r = opt.success_and_gradients()
    torch.cuda.synchronize()
    s_ref, rg_t, rg_r = float64_step(sc, model, t, r, representation, n_images, n_views, p, n_5d_poses)
    b = n_images // n_views
    assert success.shape == (b, p)
    err = np.abs(success.cpu().numpy() - s_ref).max()
    print(f'{representation} {n_images}/{n_views} n5={6 * n_5d_poses}: |success - f64| = {err:.3e} of {np.abs(s_ref).max():.3e}')
    assert err < 1e-4 * max(1.0, np.abs(s_ref).max())
    check_close(g_t.cpu().numpy(), rg_t, 'd_t')
    check_close(g_r.cpu().numpy(), rg_r, 'd_rot')
    cur = opt.compute_current_grasp_success(inputs, feats)
    assert cur.shape == (p, 1)
    assert torch.equal(cur[:, 0], success.sum(0))
    return success, g_t.clone(), g_r.clone()


@pytest.mark.parametrize('representation', ['quaternion', '6d'])
@pytest.mark.parametrize('n_images,n_views', [(1, 1), (3, 1), (2, 2)])
def test_fused_step_gradient_matches_float64_autograd(representation, n_images, n_views):
    p = 37
    sc, model, opt, inputs, feats = grasp_case(20 + n_images + n_views, n_images, n_views, representation, p)
    check_fused_step(sc, model, opt, inputs, feats, representation, n_images, n_views, p)


def test_fused_step_with_eighteen_offsets_matches_float64_autograd():
    p = 37
    sc, model, opt, inputs, feats = small_offsets_case(31, 2, 2, 'quaternion', p, 3)
    assert model.n_transforms_to_check == 18
    check_fused_step(sc, model, opt, inputs, feats, 'quaternion', 2, 2, p, n_5d_poses=3)


@pytest.mark.parametrize('representation', ['quaternion', '6d'])
@pytest.mark.parametrize('n_images,n_views', [(3, 1), (2, 2)])
def test_fused_step_matches_the_torch_path_on_the_same_state(representation, n_images, n_views):
    p = 37
    _, _, opt, inputs, feats = grasp_case(70 + n_images, n_images, n_views, representation, p)
    t, r = random_guesses(p, REPS[representation][1], seed=5)
    opt.set_initial_guesses([t, r])
    opt.compile()
    opt.bind(inputs, feats)
    s_torch, g_t, g_r = opt.success_and_gradients()
    s_torch, gt_torch, gr_torch = s_torch.cpu().numpy(), g_t.cpu().numpy(), g_r.cpu().numpy()
    opt.compile(fused=True)
    s_fused, g_t, g_r = opt.success_and_gradients()
    torch.cuda.synchronize()
    assert np.abs(s_fused.cpu().numpy() - s_torch).max() < 1e-4 * max(1.0, np.abs(s_torch).max())
    check_close(g_t.cpu().numpy(), gt_torch, 'd_t')
    check_close(g_r.cpu().numpy(), gr_torch, 'd_rot')
    opt.compile(fused=False)                                  # and back: the torch path is untouched by the fused buffers
    s_again, g_t, g_r = opt.success_and_gradients()
    assert np.array_equal(s_again.cpu().numpy(), s_torch) and np.array_equal(g_t.cpu().numpy(), gt_torch)


@pytest.mark.parametrize('representation', ['quaternion', '6d'])
def test_fused_compute_results_structure_bounds_and_reproducibility(representation):
    p, steps = 256, 3
    _, _, opt, inputs, feats = grasp_case(40, 3, 1, representation, p)
    opt.compile(fused=True)
    kw = dict(n_optimization_steps=steps, init_lr_t=0.05, decay_t=0.9, init_lr_r=0.05, decay_r=0.09)
    out = compute_results(opt, inputs, feats, True, rng=np.random.default_rng(0), **kw)
    assert opt._fused is True                                 # the compile inside compute_results keeps the mode
    losses_t, losses_r, grasps_t, grasps_r, duration, all_poses = out
    assert losses_t.shape == (p,) and losses_r.shape == (p,)
    assert grasps_t.shape == (p, 4, 4) and grasps_r.shape == (p, 4, 4)
    assert duration > 0.0
    assert len(all_poses) == 1 + 2 * (steps + 1)
    for g in (grasps_t, grasps_r, *all_poses[1:]):
        _poses_ok(g, BOUNDS)
    assert np.isfinite(losses_t).all() and np.isfinite(losses_r).all()
    assert not np.array_equal(grasps_t[:, :3, 3], all_poses[0][:, :3, 3])
    np.testing.assert_allclose(grasps_t[:, :3, :3], all_poses[0][:, :3, :3], atol=1e-6)
    np.testing.assert_array_equal(grasps_r[:, :3, 3], grasps_t[:, :3, 3])
    assert (opt._counters.cpu().numpy() == steps).all()
    again = compute_results(opt, inputs, feats, False, rng=np.random.default_rng(0), **kw)
    for a, b in zip(out[:4], again[:4]):
        np.testing.assert_array_equal(a, b)
    assert again[5] == []
    idx, best, best_l = best_grasps(losses_r, grasps_r)
    assert list(idx) == list(np.argsort(losses_r)[-5:]) and best.shape == (5, 4, 4)
    assert (np.diff(best_l) >= 0).all()
    out_l = compute_results(opt, inputs, feats, False, rng=np.random.default_rng(0), **dict(kw, n_optimization_steps=[1, 2]))
    assert (opt._counters.cpu().numpy() == 3).all() and out_l[0].shape == (p,)
    compute_results(opt, inputs, feats, False, rng=np.random.default_rng(0), sync=True, **kw)
    assert (opt._counters.cpu().numpy() == steps).all()


def test_fused_graph_replay_equals_fused_eager():
    p, steps = 256, 4
    _, _, eager, inputs, feats = grasp_case(50, 3, 1, '6d', p)
    _, _, graphed, _, _ = grasp_case(50, 3, 1, '6d', p)
    eager.compile(fused=True)
    graphed.compile(graph=True, fused=True)
    kw = dict(n_optimization_steps=steps, init_lr_t=0.05, decay_t=0.9, init_lr_r=0.05, decay_r=0.09)
    out_e = compute_results(eager, inputs, feats, True, rng=np.random.default_rng(1), **kw)
    out_g = compute_results(graphed, inputs, feats, True, rng=np.random.default_rng(1), **kw)
    assert graphed._graph is not None and eager._graph is None
    for a, b in zip(out_e[:4], out_g[:4]):
        np.testing.assert_array_equal(a, b)
    for a, b in zip(out_e[5], out_g[5]):
        np.testing.assert_array_equal(a, b)
    graph = graphed._graph
    again = compute_results(graphed, inputs, feats, False, rng=np.random.default_rng(1), **kw)
    assert graphed._graph is graph                            # re-binding the same tensors re-packs in place and keeps the capture
    for a, b in zip(out_e[:4], again[:4]):
        np.testing.assert_array_equal(a, b)
    graphed.compile(fused=False)                              # changing the mode drops it
    assert graphed._graph is None


# ---- the step through ctypes alone: torch allocates device buffers and nothing else ---------------------------------------------------------
def drive_with_ctypes_only(tensors, rep, p, b, v, h, w, n5, lr, decay, bounds, phases):
    """tensors: float32 device tensors - the scene, trunk_net, the read-out's weights, offsets and the initial t, rot.  Packs every weight
    image, fills a mvnerf_grasp_call and takes one mvnerf_grasp_opt_step per entry of `phases`.  Returns (t, rot, counters, success)."""
    lib = _lib.lib()
    ptr = lambda x: None if x is None else ctypes.c_void_p(x.data_ptr())
    f32 = lambda *s: torch.zeros(s, dtype=torch.float32, device=DEV)

    def ok(rc):
        assert rc == 0, lib.mvnerf_last_error().decode()

    packed_net, bwd = f32(lib.mvnerf_packed_net_floats()), f32(15 * 16384)
    split = torch.zeros(lib.mvnerf_packed_net_split_bytes(), dtype=torch.uint8, device=DEV)
    ok(lib.mvnerf_pack_net(ptr(tensors['trunk_net']), ptr(packed_net), None))
    ok(lib.mvnerf_pack_net_split(ptr(tensors['trunk_net']), ptr(split), None))
    ok(lib.mvnerf_pack_bwd_streams(ptr(tensors['trunk_net']), ptr(bwd), None))
    head = f32(lib.mvnerf_grasp_head_packed_floats())
    ok(lib.mvnerf_grasp_head_pack(ptr(tensors['w4']), ptr(tensors['wc']), ptr(head), None))
    tail = f32(lib.mvnerf_grasp_tail_packed_floats(n5))
    ok(lib.mvnerf_grasp_tail_pack(*(ptr(tensors[k]) for k in ('w0', 'b0', 'w1', 'b1', 'ws', 'w0b', 'b0b', 'w1b', 'b1b', 'w_out', 'b_out')), n5,
                                  ptr(tail), None))
    rd = (4, 6)[rep]
    t, rot = tensors['t'].clone(), tensors['rot'].clone()
    success, g_t, g_r = f32(b, p), f32(p, 3), f32(p, rd)
    m_t, v_t, m_r, v_r = f32(p, 3), f32(p, 3), f32(p, rd), f32(p, rd)
    counters, flags = torch.zeros((2, p), dtype=torch.int32, device=DEV), torch.zeros(2, dtype=torch.int32, device=DEV)
    need = lib.mvnerf_grasp_workspace_bytes(b, v, p, n5)
    ws = torch.full((need // 4,), float('nan'), dtype=torch.float32, device=DEV).view(torch.uint8)      # any content: production hands in torch.empty
    assert ws.numel() == need and ws.data_ptr() % 256 == 0
    c = _lib.GraspCall()
    for name, x in (('images', tensors['images']), ('features', tensors['features']), ('intrinsics', tensors['intrinsics']),
                    ('extrinsics_inv', tensors['extrinsics_inv']), ('packed_net', packed_net), ('split', split), ('bwd_streams', bwd),
                    ('head_packed', head), ('head_b4', tensors['b4']), ('head_bc', tensors['bc']), ('tail_packed', tail),
                    ('offsets', tensors['offsets']), ('t', t), ('rot', rot), ('success', success), ('g_t', g_t), ('g_rot', g_r), ('workspace', ws)):
        setattr(c, name, x.data_ptr())
    c.B, c.V, c.H, c.W, c.rep, c.P, c.n5 = b, v, h, w, rep, p, n5
    cfg = _lib.PoseAdamConfig()
    cfg.lr0[0], cfg.lr0[1], cfg.decay[0], cfg.decay[1] = lr[0], lr[1], decay[0], decay[1]
    cfg.beta1, cfg.beta2, cfg.eps, cfg.clip, cfg.clip_translation = 0.9, 0.999, 1e-7, 1.0, 1
    for i in range(3):
        cfg.lo[i], cfg.hi[i] = bounds[i][0], bounds[i][1]
    step = lambda: lib.mvnerf_grasp_opt_step(ctypes.byref(c), ctypes.byref(cfg), ptr(flags), ptr(counters), ptr(m_t), ptr(v_t), ptr(m_r),
                                             ptr(v_r), None)
    c.workspace_bytes = need - 1                              # a workspace that is too small is refused before anything runs
    assert step() == -1 and b'workspace' in lib.mvnerf_last_error()
    c.workspace_bytes = need
    for phase in phases:
        flags.copy_(torch.tensor(phase, dtype=torch.int32))  # the phase switches on the device
        ok(step())
    torch.cuda.synchronize()
    return t, rot, counters, success


@pytest.mark.parametrize('representation,n_images,n_views', [('quaternion', 3, 1), ('6d', 2, 2)])
def test_c_abi_grasp_step_through_ctypes_only(representation, n_images, n_views):
    p = 37
    sc, model, opt, inputs, feats = grasp_case(80 + n_images, n_images, n_views, representation, p)
    rep, rd = REPS[representation]
    t0, r0 = random_guesses(p, rd, seed=8)
    lr, decay = (0.05, 0.05), (0.9, 0.09)
    phases = [(1, 0)] * 3 + [(0, 1)] * 3
    # the fused optimiser from the same initial guesses
    opt.compile(optimizer=[KerasAdam(lr[0], decay[0]), KerasAdam(lr[1], decay[1])], fused=True)
    opt.set_initial_guesses([t0, r0])
    opt.bind(inputs, feats)
    for phase in phases:
        opt.optimize_pose(inputs, feats, [bool(f) for f in phase])
    torch.cuda.synchronize()
    # the same through ctypes
    b = n_images // n_views
    ro = model.grasp_readout
    f = lambda x: x.detach().to(DEV, torch.float32).contiguous()
    grp = lambda x: x.reshape((b, n_views) + tuple(x.shape[2:])).contiguous()
    tensors = dict(images=grp(inputs[0]), intrinsics=grp(inputs[1]), extrinsics_inv=grp(inputs[2]), features=grp(feats),
                   trunk_net=f(model.trunk_net), offsets=f(model.transforms_to_check),
                   w4=f(torch.stack([lin.weight for lin in ro.activation_downscale])), b4=f(torch.stack([lin.bias for lin in ro.activation_downscale])),
                   wc=f(ro.combined_activation_downscale.weight), bc=f(ro.combined_activation_downscale.bias),
                   w0=f(ro.block_0.layer_0.weight), b0=f(ro.block_0.layer_0.bias), w1=f(ro.block_0.layer_1.weight), b1=f(ro.block_0.layer_1.bias),
                   ws=f(ro.block_0.shortcut.weight), w0b=f(ro.block_1.layer_0.weight), b0b=f(ro.block_1.layer_0.bias),
                   w1b=f(ro.block_1.layer_1.weight), b1b=f(ro.block_1.layer_1.bias), w_out=f(ro.output_layer.weight), b_out=f(ro.output_layer.bias),
                   t=dev(t0[0]), rot=dev(r0[0]))
    h, w = inputs[0].shape[-3], inputs[0].shape[-2]
    t, rot, counters, success = drive_with_ctypes_only(tensors, rep, p, b, n_views, h, w, model.n_transforms_to_check, lr, decay, BOUNDS, phases)
    assert torch.equal(t, opt.translations[0]) and torch.equal(rot, opt.rotations[0])
    assert torch.equal(counters, opt._counters) and (counters == 3).all()
    assert torch.equal(success, opt._bound['fused']['success'])
    assert not torch.equal(t, dev(t0[0])) and not torch.equal(rot, dev(r0[0]))      # the steps moved both variables
