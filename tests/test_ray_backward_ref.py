"""The stand-alone ray-side references (oracle/ray_backward_ref.py) without a GPU: against torch float64 autograd, against the NumPy
oracle's float32 forward, and the sensitivity of the GPU tests' bar - every planted wrong term (`mutant=`) must be rejected by `check`
on at least one case of the input set tests/test_gpu_ray_backward.py runs the kernels on."""
import functools

import numpy as np
import pytest
import torch

from oracle import mvnerf_oracle as O
from oracle import mvnerf_torch as T
from oracle import ray_backward_ref as R

F32 = np.float32
DECISIONS = ('above', 'below', 'den_live', 'unit_sum', 'fine_rank')


def t64(a):
    return torch.tensor(np.asarray(a), dtype=torch.float64)


# ---- against autograd -----------------------------------------------------------------------------------------
@pytest.mark.parametrize('scale', R.SIGMA_SCALES)
@pytest.mark.parametrize('s', R.COMPOSITE_S)
def test_composite_bwd_ref_matches_autograd(s, scale):
    inp = R.composite_inputs(s, 5, scale)
    for which in R.COTANGENT_SETS[:3]:
        g_rgb, g_d, g_w, _ = R.cotangents(inp, which)
        tz = t64(inp['z']).requires_grad_(True)
        tr = t64(inp['rgbs']).requires_grad_(True)
        rgb, depth, w = T.volumetric_render(tz, tr[..., 3], tr[..., :3])
        loss = (rgb * t64(g_rgb)).sum()
        if g_d is not None:
            loss = loss + (depth * t64(g_d)).sum()
        if g_w is not None:
            loss = loss + (w * t64(g_w)).sum()
        loss.backward()
        d_rgbs, d_z = R.composite_bwd_ref(inp['z'], inp['rgbs'], g_rgb, g_d, g_w, np.float64)
        for got, want in ((d_rgbs, tr.grad.numpy()), (d_z, tz.grad.numpy())):
            assert np.abs(want).max() > 0
            assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max(), (which, np.abs(got - want).max() / np.abs(want).max())
        fwd = R.composite_ref(inp['z'], inp['rgbs'], np.float64)
        for got, want in zip(fwd, (rgb, depth, w)):
            assert np.abs(got - want.detach().numpy()).max() <= 1e-14


@pytest.mark.parametrize('q7', [O.Q7_ZERO, O.Q7_CLAMP])
def test_resample_bwd_ref_matches_autograd_where_the_decisions_agree(q7):
    """float64 forward values, the float32 forward's decisions, on the rays where the float64 forward decides the same."""
    inp = R.resample_inputs(301, seed=1, edge_u=False)
    f32 = R.resample_forward_f32(inp['z'], inp['weights'], inp['u_fine'], q7)
    f64 = R.resample_forward(inp['z'], inp['weights'], inp['u_fine'], q7, np.float64)
    agree = np.ones(301, bool)
    for k in DECISIONS:
        agree &= (f32[k] == f64[k]).reshape(301, -1).all(axis=1)
    left_out = 1.0 - agree.mean()
    print(f'q7={q7}: {left_out:.1%} of the rays left out')
    assert left_out <= 0.05, left_out
    got = R.resample_bwd_ref(dict(f64, **{k: f32[k] for k in DECISIONS}), inp['u_fine'], inp['d_z_all'], q7, np.float64)

    tw = t64(inp['weights']).requires_grad_(True)
    tz = t64(inp['z'])
    zf = T.sample_pdf(0.5 * (tz[..., 1:] + tz[..., :-1]), tw[..., 1:-1], t64(inp['u_fine']), q7_zero=(q7 == O.Q7_ZERO))
    z_all = torch.sort(torch.cat([tz, zf], -1), dim=-1, stable=True).values
    assert np.abs(z_all.detach().numpy() - f64['z_all']).max() < 1e-10       # sum orders differ, 1 / den amplifies
    (z_all * t64(inp['d_z_all'])).sum().backward()
    want = tw.grad.numpy()
    err = np.abs(got - want)[agree].max() / np.abs(want[agree]).max()
    print(f'q7={q7}: {err:.2e} of the maximum')
    assert err <= 1e-9, err
    assert not got[:, 0].any() and not got[:, -1].any()


def test_mse_grad_ref_matches_autograd():
    rng = np.random.default_rng(2)
    pred, label = rng.standard_normal((2, 24, 3))
    tp = t64(pred).requires_grad_(True)
    loss = ((tp - t64(label)) ** 2).mean()
    loss.backward()
    d_pred, got = R.mse_grad_ref(pred, label, np.float64)
    assert abs(got - loss.item()) < 1e-15 and np.abs(d_pred - tp.grad.numpy()).max() < 1e-16
    d32, l32 = R.mse_grad_ref(pred.astype(F32), label.astype(F32), F32)
    assert d32.dtype == F32 and l32.dtype == F32
    # one wave: the butterfly's tree and one add onto the buffer
    a, b = pred.astype(F32).ravel()[:63], label.astype(F32).ravel()[:63]
    assert abs(float(R.mse_loss_f32_accumulated(a, b, 0.25)) - 0.25 - R.mse_grad_ref(a, b)[1]) < 2e-7
    assert R.mse_loss_f32_accumulated(a, a, 0.25) == F32(0.25)


# ---- against the float32 oracle ----------------------------------------------------------------------------------
@pytest.mark.parametrize('q7', [O.Q7_ZERO, O.Q7_CLAMP])
def test_resample_forward_f32_is_the_oracle(q7):
    inp = R.resample_inputs(301)
    fwd = R.resample_forward_f32(inp['z'], inp['weights'], inp['u_fine'], q7)
    z_all, z_fine, above, below = O.hierarchical_depths(inp['z'], inp['weights'], inp['u_fine'], q7, return_indices=True)
    for k, want in (('z_all', z_all), ('z_fine', z_fine), ('above', above), ('below', below)):
        assert np.array_equal(fwd[k], want), k
    # the intermediates the oracle does not return reproduce what it does return
    again = R.resample_forward(inp['z'], inp['weights'], inp['u_fine'], q7, F32)
    for k in ('z_all', 'z_fine', 'above', 'below', 'fine_rank', 'bins', 'pdf', 'cdf', 'wsum', 'unit_sum', 'den_live'):
        assert np.array_equal(fwd[k], again[k]), k
    assert np.array_equal(np.take_along_axis(fwd['z_all'], fwd['fine_rank'].astype(np.int64), -1), fwd['z_fine'])
    # what the input set is there for
    assert list(np.nonzero(fwd['unit_sum'])[0]) == [4, 5] and fwd['pdf'][5].any() and not fwd['pdf'][4].any()
    assert (fwd['above'] >= 63).any() and not fwd['den_live'].all()
    assert (fwd['z_fine'][0, 0] == inp['z'][0, :2]).all()                         # an importance sample on two coarse depths
    assert fwd['z_fine'][1, 5] in inp['z'][1, 20:44] and 0 < inp['u_fine'][1, 5] < 1   # ... and one with a live gradient on one
    assert len(set(fwd['z_fine'][0, 8:16])) == 1                                  # tied importance samples
    assert len(set(fwd['below'][3])) <= 3                                         # the surface ray: one bin takes nearly all


# ---- the float32 run, yardstick of the GPU bars --------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def composite_refs(s, n, scale, which):
    return R.composite_bwd_refs(R.composite_inputs(s, n, scale), which)


@functools.lru_cache(maxsize=None)
def resample_refs(n, q7):
    return R.resample_bwd_refs(R.resample_inputs(n), q7)


def e32(ref64, ref32):
    out = []
    for k, r64 in ref64.items():
        m = np.abs(r64).max()
        if m > 0:
            out.append(max(np.abs(ref32[k] - r64).max() / m, np.linalg.norm(ref32[k] - r64) / np.linalg.norm(r64)))
    return max(out)


def test_float32_runs_sit_at_rounding_level():
    """Array-level e32 (max and L2) over the whole input set: what FACTOR multiplies (DESIGN.md section 8 has the table)."""
    worst = {}
    for s in R.COMPOSITE_S:
        for scale in R.SIGMA_SCALES:
            worst['composite_bwd', s, scale] = max(e32(*composite_refs(s, n, scale, which)) for n in R.COMPOSITE_RAYS
                                                   for which in R.COTANGENT_SETS[:3])
    for q7 in (O.Q7_ZERO, O.Q7_CLAMP):
        worst['resample_bwd', q7] = max(e32(*resample_refs(n, q7)[1:]) for n in R.RESAMPLE_RAYS)
    for k, v in worst.items():
        print(k, f'{v:.2e}')
        assert 0 < v < 1e-6, (k, v)
    r64, r32 = composite_refs(64, 5, 30.0, 'all')
    assert R.check('self', r32, r64, r32) == 1.0


# ---- mutants -------------------------------------------------------------------------------------------------
def rejected(tag, got, ref64, ref32):
    try:
        R.check(tag, got, ref64, ref32)
    except AssertionError:
        return True
    return False


@pytest.mark.parametrize('mutant', R.COMPOSITE_MUTANTS)
def test_check_rejects_composite_bwd_mutants(mutant):
    hits = []
    for s in R.COMPOSITE_S:
        for n in R.COMPOSITE_RAYS:
            for scale in R.SIGMA_SCALES:
                inp = R.composite_inputs(s, n, scale)
                for which in R.COTANGENT_SETS[:3]:
                    _, bad = R.composite_bwd_refs(inp, which, mutant=mutant)
                    if rejected(mutant, bad, *composite_refs(s, n, scale, which)):
                        hits.append((s, n, scale, which))
    print(mutant, len(hits), 'cases reject it, first', hits[:3])
    assert hits, mutant
    if mutant in ('no_eps', 'suffix_by_difference'):        # invisible below saturation: what the two dense regimes are there for
        assert all(scale > 30.0 for _, _, scale, _ in hits)


@pytest.mark.parametrize('mutant', [m for m in R.RESAMPLE_MUTANTS if m != 'const_gets_dca'])
def test_check_rejects_resample_bwd_mutants(mutant):
    hits = []
    for n in R.RESAMPLE_RAYS:
        for q7 in (O.Q7_ZERO, O.Q7_CLAMP):
            fwd, r64, r32 = resample_refs(n, q7)
            _, _, bad = R.resample_bwd_refs(R.resample_inputs(n), q7, mutant=mutant, fwd=fwd)
            if rejected(mutant, bad, r64, r32):
                hits.append((n, q7))
    print(mutant, 'rejected on', hits)
    assert hits, mutant


def test_the_q7_zero_constant_never_has_a_cdf_gradient_to_receive():
    """Mutant 6 of the list, `const_gets_dca` (the out-of-range gather's constant 0 receives d cdf_a), changes no bit on any input
    the forward can produce, so no bar can reject it, and this test asserts why instead.  The constant is gathered when above == 63,
    where cdf_a = 0 and cdf_b = cdf_62, the sequential sum of all pdf = s / sum(s): 1 up to rounding, or exactly 0 under unit_sum.
    den_raw = -cdf_62 <= 0 is below 1e-5f, den_live is false, k2 is not formed and d cdf_a = -k2 is exactly zero.  Only a pdf whose
    rounding errors sum past 1 (entries above 2^24) could make cdf_62 negative; the same cancellation would leave the float32 run
    of `dot` without a correct digit, and with it the bar."""
    seen = 0
    for n in R.RESAMPLE_RAYS:
        inp = R.resample_inputs(n)
        fwd, r64, r32 = resample_refs(n, O.Q7_ZERO)
        a_const = fwd['above'] >= 63
        seen += int(a_const.sum())
        assert not (a_const & fwd['den_live']).any()
        _, _, same = R.resample_bwd_refs(inp, O.Q7_ZERO, mutant='const_gets_dca', fwd=fwd)
        assert np.array_equal(same['d_weights'], r32['d_weights'])
    assert seen > 300                            # the nextafter(1, 0) column and the unit_sum rays
