"""The scalar math of the LanguageNeRF training step's new HIP passes, built for the host by tests/cpu_language/Makefile from the source
the kernels compile (thesis_clip_nerf_amd/csrc/mvnerf_pose.h: the pose JVP; mvnerf_language.h: the losses) - no GPU here.

Bars.  The pose JVP: float64 autograd of the restated pose map, relative 1e-5 as tests/test_pose_math_cpu.py holds the host VJP to; and
<c, VJP(d)> = <JVP(c), d> against that host VJP to 1e-4 of the sum of the terms' magnitudes.  The losses and their cotangents: the error
against float64 autograd of lmvnerf.py's torch losses is at most FACTOR = 8 times the error of the same torch code evaluated in float32
(the rule of tests/test_gpu_field_backward.py); for a scalar the bar is never below one ulp of the value (tests/test_gpu_ray_backward.py).
Four deliberately wrong terms (tests/cpu_language/language_cpu.cpp) show that each bar catches a wrong formula."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

from tests.test_pose_math_cpu import F32, REPS, ptr, query_ref, random_poses
from thesis_clip_nerf_amd import lmvnerf as M
from thesis_clip_nerf_amd.lmvnerf import grasp_offsets

HERE = os.path.dirname(os.path.abspath(__file__))
FACTOR = 8.0


def build(name, so):
    d = os.path.join(HERE, name)
    subprocess.run(['make', '-C', d], check=True, capture_output=True)
    return ctypes.CDLL(os.path.join(d, so))


@pytest.fixture(scope='module')
def cpu():
    lib = build('cpu_language', 'libmvnerf_language_cpu.so')
    lib.pose = build('cpu_pose', 'libmvnerf_pose_cpu.so')
    return lib


# ---- the pose JVP -----------------------------------------------------------------------------------------------------------------------------
def jvp_case(representation, seed, p=53):
    rep, rd = REPS[representation]
    rng = np.random.default_rng(seed)
    offsets = grasp_offsets(7)
    t, r = random_poses(rng, p, rd)
    c_t = rng.standard_normal((p, 3)).astype(F32)
    c_r = rng.standard_normal((p, rd)).astype(F32)
    return rep, rd, offsets, t, r, c_t, c_r


def host_jvp(cpu, rep, offsets, r, c_t, c_r, wrong=0):
    p, n5 = r.shape[0], offsets.shape[0]
    tp, td = np.empty((p * n5, 3), F32), np.empty((p * n5, 3), F32)
    cpu.ml_pose_jvp(ptr(r), rep, ptr(offsets), ptr(c_t), ptr(c_r), p, n5, ptr(tp), ptr(td), wrong)
    return tp, td


def jvp_ref(representation, offsets, t, r, c_t, c_r):
    """float64 forward-mode derivative of (t, r) -> query_ref along (c_t, c_r)."""
    d = lambda a: torch.as_tensor(a, dtype=torch.float64)
    fn = lambda tt, rr: query_ref(tt, rr, representation, offsets)
    _, (tp, td) = torch.autograd.functional.jvp(fn, (d(t), d(r)), (d(c_t), d(c_r)))
    return tp.numpy(), td.numpy()


def jvp_errors(got, ref):
    return [(np.linalg.norm(g - r) / np.linalg.norm(r), np.abs(g - r).max() / np.abs(r).max()) for g, r in zip(got, ref)]


@pytest.mark.parametrize('representation', ['quaternion', '6d'])
def test_pose_jvp_matches_float64_autograd(cpu, representation):
    rep, rd, offsets, t, r, c_t, c_r = jvp_case(representation, 20 + REPS[representation][0])
    got = host_jvp(cpu, rep, offsets, r, c_t, c_r)
    ref = jvp_ref(representation, offsets, t, r, c_t, c_r)
    for l2, mx in jvp_errors(got, ref):
        print(f'{representation}: l2 {l2:.3e} max {mx:.3e}')
        assert l2 < 1e-5 and mx < 4e-5


@pytest.mark.parametrize('representation', ['quaternion', '6d'])
@pytest.mark.parametrize('n_scenes', [1, 3])
def test_pose_jvp_is_the_adjoint_of_the_host_vjp(cpu, representation, n_scenes):
    rep, rd, offsets, t, r, c_t, c_r = jvp_case(representation, 30 + n_scenes, p=41)
    p, n5 = r.shape[0], offsets.shape[0]
    rng = np.random.default_rng(n_scenes)
    dp = rng.standard_normal((n_scenes, p * n5, 3)).astype(F32)
    dd = rng.standard_normal((n_scenes, p * n5, 3)).astype(F32)
    d_t, d_r = np.empty((p, 3), F32), np.empty((p, rd), F32)
    cpu.pose.mp_query_vjp(ptr(r), rep, ptr(offsets), ptr(dp), ptr(dd), p, n5, n_scenes, ctypes.c_float(1.0), ptr(d_t), ptr(d_r))
    tp, td = host_jvp(cpu, rep, offsets, r, c_t, c_r)
    f64 = np.float64
    left = [c_t.astype(f64) * d_t, c_r.astype(f64) * d_r]
    right = [tp.astype(f64)[None] * dp, td.astype(f64)[None] * dd]                     # the JVP is the same for every scene
    lhs, rhs = sum(a.sum() for a in left), sum(a.sum() for a in right)
    scale = sum(np.abs(a).sum() for a in left + right)
    print(f'{representation} B={n_scenes}: <c, VJP d> {lhs:.6e}  <JVP c, d> {rhs:.6e}  sum|terms| {scale:.3e}')
    assert abs(lhs - rhs) <= 1e-4 * scale


@pytest.mark.parametrize('representation,wrong', [('6d', 1), ('quaternion', 2)])
def test_pose_jvp_bar_catches_a_wrong_term(cpu, representation, wrong):
    rep, rd, offsets, t, r, c_t, c_r = jvp_case(representation, 40 + wrong)
    ref = jvp_ref(representation, offsets, t, r, c_t, c_r)
    assert all(l2 < 1e-5 for l2, _ in jvp_errors(host_jvp(cpu, rep, offsets, r, c_t, c_r), ref))
    errs = jvp_errors(host_jvp(cpu, rep, offsets, r, c_t, c_r, wrong), ref)
    print(representation, wrong, errs)
    assert max(l2 for l2, _ in errs) > 1e-5


# ---- the losses -------------------------------------------------------------------------------------------------------------------------------
def landscape_total(y, label, kind, weight):
    """(reported loss, weight * the total lmvnerf.py differentiates) in y's dtype."""
    if kind == 0:
        per = M.kl_divergence(label, torch.softmax(y, -1))
        return per.mean(), weight * per.sum()
    ce = M.categorical_crossentropy_from_logits(label, y)
    return ce, weight * ce


def cosine_total(x, label, scale):
    if x.shape[-1] == 6:
        loss = M.cosine_similarity_loss(label[..., :3], x[..., :3]) + M.cosine_similarity_loss(label[..., 3:], x[..., 3:])
    else:
        loss = M.cosine_similarity_loss(label, x)
    return loss, scale * loss


def torch_eval(fn, x, label, extra, dtype):
    xx = torch.as_tensor(x).to(dtype).requires_grad_(True)
    value, total = fn(xx, torch.as_tensor(label).to(dtype), *extra)
    g, = torch.autograd.grad(total, xx)
    return float(value.detach()), g.double().numpy()


def check_loss(name, got_value, got_g, fn, x, label, extra):
    v64, g64 = torch_eval(fn, x, label, extra, torch.float64)
    v32, g32 = torch_eval(fn, x, label, extra, torch.float32)
    ulp = float(np.spacing(np.float32(abs(v64))))
    e64v, e32v = abs(got_value - v64), abs(v32 - v64)
    e64g, e32g = np.linalg.norm(got_g - g64), np.linalg.norm(g32 - g64)
    print(f'{name}: value e64 {e64v:.3e} e32 {e32v:.3e} ulp {ulp:.3e}; cotangent e64 {e64g:.3e} e32 {e32g:.3e} |ref| {np.linalg.norm(g64):.3e}')
    return e64v <= max(FACTOR * e32v, ulp), e64g <= FACTOR * e32g


def host_landscape(cpu, y, label, kind, weight, wrong=0):
    g, loss = np.empty_like(y), np.empty(1, F32)
    cpu.ml_landscape(ptr(y), ptr(label), y.shape[0], y.shape[1], kind, ctypes.c_float(weight), ptr(g), ptr(loss), wrong)
    return float(loss[0]), g.astype(np.float64)


def host_cosine(cpu, x, label, scale, wrong=0):
    g, loss = np.empty_like(x), np.empty(1, F32)
    cpu.ml_cosine(ptr(x), ptr(label), ctypes.c_long(x.size // x.shape[-1]), x.shape[-1], ctypes.c_float(scale), ptr(g), ptr(loss), wrong)
    return float(loss[0]), g.astype(np.float64)


def landscape_case(seed, b, n_p):
    rng = np.random.default_rng(seed)
    y = (2.0 * rng.standard_normal((b, n_p))).astype(F32)
    label = rng.random((b, n_p)).astype(F32)
    label /= label.sum(-1, keepdims=True)
    return y, label


@pytest.mark.parametrize('kind', [0, 1])
@pytest.mark.parametrize('b,n_p', [(1, 1), (2, 3), (7, 5), (300, 8)])
def test_landscape_loss_and_cotangent(cpu, kind, b, n_p):
    y, label = landscape_case(b + n_p, b, n_p)
    if b == 7:
        y[0, 0] = 40.0                   # the other softmax entries of this row fall below the 1e-7 clip: no derivative through them
        label[1, 0] = 0.0                # a label below the clip
    weight = 0.7
    value, g = host_landscape(cpu, y, label, kind, weight)
    ok_v, ok_g = check_loss(f'landscape kind={kind} B={b} np={n_p}', value, g, landscape_total, y, label, (kind, weight))
    assert ok_v and ok_g


def cosine_case(seed, rows, dim):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((rows, dim)).astype(F32) * rng.uniform(0.01, 30.0, (rows, 1)).astype(F32)
    label = rng.standard_normal((rows, dim)).astype(F32)
    return x, label


@pytest.mark.parametrize('dim', [3, 4, 6])
@pytest.mark.parametrize('rows', [1, 6, 300])
def test_cosine_loss_and_cotangent(cpu, dim, rows):
    x, label = cosine_case(10 * dim + rows, rows, dim)
    value, g = host_cosine(cpu, x, label, 2.0)
    ok_v, ok_g = check_loss(f'cosine dim={dim} rows={rows}', value, g, cosine_total, x, label, (2.0,))
    assert ok_v and ok_g


@pytest.mark.parametrize('dim', [3, 4, 6])
def test_cosine_loss_below_the_clamp(cpu, dim):
    """A row whose squared norm is below 1e-12: the clamp holds the scale at 1e6 and passes no derivative."""
    x, label = cosine_case(dim, 5, dim)
    x[2] = (1e-8 * np.arange(1, dim + 1)).astype(F32)
    value, g = host_cosine(cpu, x, label, 1.0)
    ok_v, ok_g = check_loss(f'cosine below the clamp dim={dim}', value, g, cosine_total, x, label, (1.0,))
    assert ok_v and ok_g
    assert np.abs(g[2]).max() > 1e4           # u(label) * 1e6 / rows


def test_loss_bars_catch_wrong_terms(cpu):
    x, label = cosine_case(3, 6, 3)
    assert check_loss('cosine', *host_cosine(cpu, x, label, 1.0), cosine_total, x, label, (1.0,))[1]
    assert not check_loss('cosine without its projection', *host_cosine(cpu, x, label, 1.0, 1), cosine_total, x, label, (1.0,))[1]
    y, lab = landscape_case(4, 2, 3)
    assert check_loss('kl', *host_landscape(cpu, y, lab, 0, 1.0), landscape_total, y, lab, (0, 1.0))[1]
    assert not check_loss('kl without the softmax Jacobian', *host_landscape(cpu, y, lab, 0, 1.0, 1), landscape_total, y, lab, (0, 1.0))[1]
