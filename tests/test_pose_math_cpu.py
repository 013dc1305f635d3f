"""The per-pose math of the grasp-pose optimiser (thesis_clip_nerf_amd/csrc/mvnerf_pose.h, the source pose_ops.hip compiles), built for
the host by tests/cpu_pose/Makefile and checked against float64 torch autograd and the Keras Adam closed form; the host side of
DNGFOptimizer (initial guesses, shape checks) and the argument validation of the new C entry points - no GPU here."""
import ctypes
import os
import subprocess
import types

import numpy as np
import pytest
import torch

from oracle import lmvnerf_torch as L
from thesis_clip_nerf_amd import _lib
from thesis_clip_nerf_amd.encoders import KerasAdam as TorchKerasAdam
from thesis_clip_nerf_amd.grasp_optimizer import DNGFOptimizer, KerasAdam, euler_xyz_to_matrix
from thesis_clip_nerf_amd.lmvnerf import grasp_offsets

HERE = os.path.dirname(os.path.abspath(__file__))
F32 = np.float32
REPS = {'quaternion': (0, 4), '6d': (1, 6)}


@pytest.fixture(scope='module')
def cpu():
    d = os.path.join(HERE, 'cpu_pose')
    subprocess.run(['make', '-C', d], check=True, capture_output=True)
    return ctypes.CDLL(os.path.join(d, 'libmvnerf_pose_cpu.so'))


def ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def random_poses(rng, p, rd):
    t = rng.uniform(-0.5, 0.5, (p, 3)).astype(F32)
    r = rng.standard_normal((p, rd)).astype(F32)
    if rd == 4:
        r *= rng.uniform(0.5, 2.0, (p, 1)).astype(F32)          # non-unit quaternions: tfg uses q as given
    return t, r


def query_ref(t, r, representation, offsets):
    """compute_matrices (oracle restatement) then LanguageNeRF._query_points in float64 -> points, dirs (P*n5, 3)."""
    m = L.compute_matrices(t[None], r[None], representation)[0]
    rot, tr = m[:, :3, :3], m[:, :3, 3]
    off = torch.as_tensor(offsets, dtype=torch.float64)
    pts = torch.einsum('pik,ok->poi', rot, off[:, :3, 3]) + tr[:, None]
    drs = torch.einsum('pik,ok->poi', rot, off[:, :3, 2])
    return pts.reshape(-1, 3), drs.reshape(-1, 3)


def rel_max(got, ref):
    return float(np.abs(got - ref).max() / np.abs(ref).max())


@pytest.mark.parametrize('representation', ['quaternion', '6d'])
def test_query_points_match_float64(cpu, representation):
    rep, rd = REPS[representation]
    rng = np.random.default_rng(1 + rep)
    offsets = grasp_offsets(7)
    p, n5 = 97, offsets.shape[0]
    t, r = random_poses(rng, p, rd)
    pts, drs = np.empty((p * n5, 3), F32), np.empty((p * n5, 3), F32)
    cpu.mp_query_points(ptr(t), ptr(r), rep, ptr(offsets), p, n5, ptr(pts), ptr(drs))
    rp, rdr = query_ref(torch.as_tensor(t, dtype=torch.float64), torch.as_tensor(r, dtype=torch.float64), representation, offsets)
    assert rel_max(pts, rp.numpy()) < 1e-6
    assert rel_max(drs, rdr.numpy()) < 1e-6


@pytest.mark.parametrize('representation', ['quaternion', '6d'])
@pytest.mark.parametrize('n_scenes', [1, 3])
def test_query_vjp_matches_float64_autograd(cpu, representation, n_scenes):
    rep, rd = REPS[representation]
    rng = np.random.default_rng(10 * n_scenes + rep)
    offsets = grasp_offsets(7)
    p, n5 = 53, offsets.shape[0]
    t, r = random_poses(rng, p, rd)
    dp = rng.standard_normal((n_scenes, p * n5, 3)).astype(F32)
    dd = rng.standard_normal((n_scenes, p * n5, 3)).astype(F32)
    d_t, d_r = np.empty((p, 3), F32), np.empty((p, rd), F32)
    cpu.mp_query_vjp(ptr(r), rep, ptr(offsets), ptr(dp), ptr(dd), p, n5, n_scenes, ctypes.c_float(-1.0), ptr(d_t), ptr(d_r))
    t64 = torch.as_tensor(t, dtype=torch.float64).requires_grad_(True)
    r64 = torch.as_tensor(r, dtype=torch.float64).requires_grad_(True)
    pts, drs = query_ref(t64, r64, representation, offsets)
    loss = -sum(((torch.as_tensor(dp[b], dtype=torch.float64) * pts).sum() + (torch.as_tensor(dd[b], dtype=torch.float64) * drs).sum())
                for b in range(n_scenes))
    g_t, g_r = torch.autograd.grad(loss, (t64, r64))
    for got, ref in ((d_t, g_t.numpy()), (d_r, g_r.numpy())):
        assert np.linalg.norm(got - ref) / np.linalg.norm(ref) < 1e-5
        assert np.abs(got - ref).max() < 1e-5 * np.abs(ref).max() * 4


def post_process_ref(t, r, representation, bounds, clip_translation):
    if clip_translation:
        t = torch.minimum(torch.maximum(t, torch.as_tensor(bounds[:, 0])), torch.as_tensor(bounds[:, 1]))
    if representation == 'quaternion':
        r = r / r.norm(dim=-1, keepdim=True)
    else:
        r = torch.cat([r[..., :3] / r[..., :3].norm(dim=-1, keepdim=True), r[..., 3:] / r[..., 3:].norm(dim=-1, keepdim=True)], -1)
    return t, r


@pytest.mark.parametrize('representation', ['quaternion', '6d'])
@pytest.mark.parametrize('lr,decay', [((0.05, 0.05), (0.9, 0.09)), ((0.02, 0.03), (1.0, 1.0))])
def test_adam_steps_match_keras_closed_form(cpu, representation, lr, decay):
    """20 steps with the phase flags toggled: t only, rot only, both, t only - each variable's Keras iteration counter advances only when
    it trains; lr_k = lr0 decay^(k-1) (ExponentialDecay, decay_steps=1); clip-by-value 1; post_process after every step."""
    rep, rd = REPS[representation]
    rng = np.random.default_rng(5 + rep)
    p = 41
    bounds = np.array([[-0.2, 0.2], [-0.3, 0.1], [0.0, 0.25]])
    t, r = random_poses(rng, p, rd)
    t0, r0 = post_process_ref(torch.as_tensor(t, dtype=torch.float64), torch.as_tensor(r, dtype=torch.float64), representation, bounds, True)
    t, r = t0.numpy().astype(F32), r0.numpy().astype(F32)
    m_t, v_t, m_r, v_r = (np.zeros_like(a) for a in (t, t, r, r))
    counters = np.zeros((2, p), np.int32)
    cfg = np.array([lr[0], lr[1], decay[0], decay[1], 0.9, 0.999, 1e-7, 1.0, *bounds[:, 0], *bounds[:, 1]], F32)
    # float64 twin: encoders.KerasAdam (Keras' update form), one optimiser per variable, rate set to the decayed value before each step
    tv, rv = t.astype(np.float64), r.astype(np.float64)
    tv = torch.tensor(tv, requires_grad=True)
    rv = torch.tensor(rv, requires_grad=True)
    opts = [TorchKerasAdam([tv], lr=lr[0], eps=1e-7), TorchKerasAdam([rv], lr=lr[1], eps=1e-7)]
    ks = [0, 0]
    phases = [(1, 0)] * 6 + [(0, 1)] * 6 + [(1, 1)] * 4 + [(1, 0)] * 4
    for flags in phases:
        g_t = (1.5 * rng.standard_normal((p, 3))).astype(F32)               # some entries beyond the clip
        g_r = (1.5 * rng.standard_normal((p, rd))).astype(F32)
        fl = np.array(flags, np.int32)
        cpu.mp_adam_step(ptr(cfg), 1, rep, p, ptr(fl), ptr(counters), ptr(g_t), ptr(g_r), ptr(m_t), ptr(v_t), ptr(m_r), ptr(v_r), ptr(t),
                         ptr(r))
        for i, (var, g) in enumerate(((tv, g_t), (rv, g_r))):
            if flags[i]:
                ks[i] += 1
                opts[i].param_groups[0]['lr'] = lr[i] * decay[i] ** (ks[i] - 1)
                var.grad = torch.as_tensor(np.clip(g, -1.0, 1.0), dtype=torch.float64)
                opts[i].step()
        with torch.no_grad():
            a, b = post_process_ref(tv, rv, representation, bounds, True)
            tv.copy_(a)
            rv.copy_(b)
        np.testing.assert_array_equal(counters[0], ks[0])
        np.testing.assert_array_equal(counters[1], ks[1])
        assert np.abs(t - tv.detach().numpy()).max() < 1e-6
        assert np.abs(r - rv.detach().numpy()).max() < 1e-6
    assert ks == [14, 10]
    assert (t >= bounds[:, 0].astype(F32)).all() and (t <= bounds[:, 1].astype(F32)).all()


# ---- host side of DNGFOptimizer ---------------------------------------------------------------------------------------------------------
def stub_grasper(n_views=1):
    return types.SimpleNamespace(n_views=n_views, device_=torch.device('cpu'), n_transforms_to_check=42)


@pytest.mark.parametrize('representation', ['quaternion', '6d'])
def test_initial_guesses_bounds_units_and_seed(representation):
    bounds = ((0.35, 0.85), (-0.25, 0.25), (0.0, 0.2))
    opt = DNGFOptimizer(stub_grasper(), bounds, n_initial_guesses=500, n_images=3, rotation_representation=representation)
    t, r = opt.generate_initial_guesses(rng=np.random.default_rng(4))
    rd = REPS[representation][1]
    assert t.shape == (1, 500, 3) and r.shape == (1, 500, rd)
    b = np.array(bounds)
    assert (t >= b[:, 0]).all() and (t <= b[:, 1]).all()
    halves = [r] if rd == 4 else [r[..., :3], r[..., 3:]]
    for h in halves:
        np.testing.assert_allclose(np.linalg.norm(h, axis=-1), 1.0, atol=1e-12)
    t2, r2 = opt.generate_initial_guesses(rng=np.random.default_rng(4))
    np.testing.assert_array_equal(t, t2)
    np.testing.assert_array_equal(r, r2)
    t3, _ = opt.generate_initial_guesses(rng=np.random.default_rng(5))
    assert not np.array_equal(t, t3)
    tb, rb = opt.generate_initial_guesses(rng=np.random.default_rng(4), batch_size=2, n_initial_guesses=7)
    assert tb.shape == (2, 7, 3) and rb.shape == (2, 7, rd)


@pytest.mark.parametrize('representation', ['quaternion', '6d'])
def test_initial_guesses_follow_scipy_from_euler(representation):
    Rotation = pytest.importorskip('scipy.spatial.transform').Rotation
    opt = DNGFOptimizer(stub_grasper(), ((0, 1), (0, 1), (0, 1)), n_initial_guesses=300, rotation_representation=representation)
    # the draws are t then rpy per pose, as Affine.random's two np.random.uniform calls (transform.py:32-55)
    draws = np.random.default_rng(9).uniform(np.r_[np.zeros(3), np.zeros(3)], np.r_[np.ones(3), np.full(3, 2 * np.pi)], (300, 6))
    t, r = opt.generate_initial_guesses(rng=np.random.default_rng(9))
    np.testing.assert_array_equal(t[0], draws[:, :3])
    rot = Rotation.from_euler('xyz', draws[:, 3:])
    np.testing.assert_allclose(euler_xyz_to_matrix(draws[:, 3:]), rot.as_matrix(), rtol=0, atol=1e-12)
    if representation == 'quaternion':
        np.testing.assert_allclose(r[0], rot.as_quat(), rtol=0, atol=1e-12)           # same sign as scipy's composition
    else:
        m = rot.as_matrix()
        np.testing.assert_allclose(r[0], np.concatenate([m[:, :, 0], m[:, :, 1]], -1), rtol=0, atol=1e-12)


def test_set_initial_guesses_checks_shapes_and_scene_grouping():
    opt = DNGFOptimizer(stub_grasper(), ((0, 1), (0, 1), (0, 1)), n_initial_guesses=5, n_images=3, rotation_representation='6d')
    assert opt.batch_size == 3
    opt.set_initial_guesses([np.zeros((1, 5, 3)), np.ones((1, 5, 6))])
    assert float(opt.rotations.sum()) == 30.0
    with pytest.raises(ValueError):
        opt.set_initial_guesses([np.zeros((1, 5, 3)), np.ones((1, 5, 4))])
    with pytest.raises(ValueError):
        opt.set_initial_guesses([np.zeros((1, 4, 3)), np.ones((1, 4, 6))])
    with pytest.raises(ValueError):
        opt.set_initial_guesses([np.zeros((1, 5, 3))])
    assert DNGFOptimizer(stub_grasper(2), ((0, 1), (0, 1), (0, 1)), n_images=4).batch_size == 2
    with pytest.raises(ValueError):
        DNGFOptimizer(stub_grasper(2), ((0, 1), (0, 1), (0, 1)), n_images=3)
    with pytest.raises(ValueError):
        DNGFOptimizer(stub_grasper(), ((0, 1), (0, 1), (0, 1)), rotation_representation='euler')
    with pytest.raises(ValueError):
        opt.compile(optimizer=[KerasAdam(0.1), KerasAdam(0.1, beta_1=0.8)])


def test_argument_validation_of_pose_entry_points():
    lib = _lib.lib()
    one, odd = ctypes.c_void_p(16), ctypes.c_void_p(18)
    qp = lambda t, rep, p, n5, b, ld: lib.mvnerf_pose_query_points(t, one, rep, one, p, n5, b, ld, one, one, None)
    assert qp(None, 0, 4, 42, 1, 168) == -1
    assert b'null' in lib.mvnerf_last_error()
    assert qp(one, 0, 0, 42, 1, 168) == -1                    # P = 0
    assert qp(one, 2, 4, 42, 1, 168) == -2                    # no such representation
    assert qp(one, 1, 4, 42, 1, 167) == -2                    # ld < P * n5
    assert qp(odd, 1, 4, 42, 1, 168) == -3
    vj = lambda rot, rep, b, ld, d_t: lib.mvnerf_pose_query_vjp(rot, rep, one, one, one, 4, 42, b, ld, -1.0, d_t, one, None)
    assert vj(one, 0, 1, 168, None) == -1
    assert vj(one, 0, 0, 168, one) == -1                      # B = 0
    assert vj(one, 3, 1, 168, one) == -2
    assert vj(one, 0, 2, 100, one) == -2
    assert vj(odd, 0, 1, 168, one) == -3
    cfg = _lib.PoseAdamConfig()
    ad = lambda c, rep, p, flags: lib.mvnerf_pose_adam_step(c, rep, p, flags, *([one] * 10), None)
    assert ad(None, 0, 4, one) == -1
    assert ad(ctypes.byref(cfg), 0, 4, None) == -1
    assert ad(ctypes.byref(cfg), 0, -1, one) == -1
    assert ad(ctypes.byref(cfg), 5, 4, one) == -2
    assert ad(ctypes.byref(cfg), 1, 4, odd) == -3
