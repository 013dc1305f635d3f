"""The ray-side kernels of the training step, each on its own against the stand-alone references of oracle/ray_backward_ref.py:
`mse_grad_kernel`, `composite_bwd_kernel<1|2>`, `resample_bwd_kernel` (csrc/train_ops.hip), `composite_kernel<1..4>` and the
`fine_rank` output of `resample_kernel` (csrc/ray_ops.hip).

Bar (`R.check`): for every output array, e64 = |got - ref64| must not exceed FACTOR * e32 in the L2 norm, in the maximum relative to
the array's maximum and for the worst ray relative to that ray's own maximum; e32 is the float32 run of the same NumPy reference
against its float64 run, computed here, from the reference alone.  FACTOR = 8 as in tests/test_gpu_field_backward.py; these kernels
are plain fp32 and differ from the float32 run in summation order only, so ratios near 1 are what to expect (printed with -s,
DESIGN.md section 8 keeps the largest per case).  Where ref64 is exactly zero the kernel's value must be exactly zero.  The
resampling backward is compared on the float32 forward's own decisions (`R.resample_forward_f32`, which the forward test holds the
kernel to), so no ray is left out.

Every output buffer belongs to the test (the C ABI is called through `ops._lib`), is four rays longer than n_rays and holds the NaN
pattern 0x7FC00000 before the call: an element the kernel does not write shows as NaN, a row past n_rays it writes shows as a changed
pattern.  tests/test_ray_backward_ref.py asserts, without a GPU, that this bar rejects each of ten planted wrong terms on these inputs.
"""
import functools

import numpy as np
import pytest
import torch

from oracle import mvnerf_oracle as O
from oracle import ray_backward_ref as R
from thesis_clip_nerf_amd import ops

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
F32 = np.float32
GUARD = 4
Q7_MODES = (O.Q7_ZERO, O.Q7_CLAMP)


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def poisoned(*shape, dtype=torch.float32):
    return torch.full(shape, R.NAN_PATTERN, dtype=torch.int32, device=DEV).view(dtype)


def result(buf, n):
    """Rows [0, n) of an output buffer as float64 (int32 stays), after asserting that the guard rows kept the pattern."""
    torch.cuda.synchronize()
    assert buf.shape[0] == n + GUARD
    assert bool((buf[n:].view(torch.int32) == R.NAN_PATTERN).all()), 'rows past n_rays were written'
    out = buf[:n].cpu().numpy()
    return out.astype(np.float64) if out.dtype == F32 else out


def call(name, *args):
    with torch.cuda.device(DEV):
        rc = getattr(ops._lib.lib(), name)(*args, ops._stream(torch.empty(0, device=DEV)))
    ops._lib.check(rc, name)


# ---- composite_bwd -------------------------------------------------------------------------------------------
def composite_bwd(inp, which):
    g_rgb, g_d, g_w, want_dz = R.cotangents(inp, which)
    n, s = inp['z'].shape
    args = [dev(a) for a in (inp['z'], inp['rgbs'], g_rgb, g_d, g_w)]
    d_rgbs = poisoned(n + GUARD, s, 4)
    d_z = poisoned(n + GUARD, s) if want_dz else None
    call('mvnerf_composite_bwd', *(ops._p(a) for a in args), n, s, ops._p(d_rgbs), ops._p(d_z))
    got = dict(d_rgbs=result(d_rgbs, n))
    if want_dz:
        got['d_z'] = result(d_z, n)
    return got


@pytest.mark.parametrize('scale', R.SIGMA_SCALES)
@pytest.mark.parametrize('n_rays', R.COMPOSITE_RAYS)
@pytest.mark.parametrize('s', R.COMPOSITE_S)
def test_composite_bwd_matches_float64_reference(s, n_rays, scale):
    """All three cotangents; d_rgb only with d_z requested (the fine call of the step: d_depth = d_weights = NULL); d_rgb and
    d_weights without d_z (the coarse call); zero cotangents, where every output is exactly zero."""
    inp = R.composite_inputs(s, n_rays, scale)
    worst = 0.0
    for which in R.COTANGENT_SETS:
        ref64, ref32 = R.composite_bwd_refs(inp, which)
        got = composite_bwd(inp, which)
        assert set(got) == set(ref64)
        if which == 'zero':
            assert not any(np.count_nonzero(v) for v in ref64.values())
        worst = max(worst, R.check(f'composite_bwd S={s} n={n_rays} sigma~{scale:g} {which}:', got, ref64, ref32))
    print(f'RATIO composite_bwd S={s} n={n_rays} sigma~{scale:g}: {worst:.2f}')


def test_composite_bwd_refuses_192_samples():
    inp = R.composite_inputs(192, 2, 30.0)
    with pytest.raises(ValueError, match=r'mvnerf_composite_bwd: S=192.*\(code -2\)'):
        ops.composite_bwd(dev(inp['z']), dev(inp['rgbs']), dev(inp['d_rgb']))


# ---- composite forward ---------------------------------------------------------------------------------------
@pytest.mark.parametrize('scale', R.SIGMA_SCALES)
@pytest.mark.parametrize('s', (64, 128, 192, 256))
def test_composite_matches_float64_reference(s, scale):
    n = 131                                                      # 33 workgroups, the last one ragged
    inp = R.composite_inputs(s, n, scale)
    rgb, depth, weights = poisoned(n + GUARD, 3), poisoned(n + GUARD), poisoned(n + GUARD, s)
    z, rgbs = dev(inp['z']), dev(inp['rgbs'])
    call('mvnerf_composite', ops._p(z), ops._p(rgbs), n, s, ops._p(rgb), ops._p(depth), ops._p(weights))
    got = dict(rgb=result(rgb, n), depth=result(depth, n), weights=result(weights, n))
    names = ('rgb', 'depth', 'weights')
    ref64 = dict(zip(names, R.composite_ref(inp['z'], inp['rgbs'], np.float64)))
    ref32 = dict(zip(names, R.composite_ref(inp['z'], inp['rgbs'], F32)))
    worst = R.check(f'composite S={s} sigma~{scale:g}:', got, ref64, ref32)
    print(f'RATIO composite S={s} sigma~{scale:g}: {worst:.2f}')
    assert got['weights'].sum(axis=1).max() <= 1 + 1e-6 and got['weights'].min() >= 0


# ---- resample: the rank, then the backward ------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def resample_case(n_rays, q7):
    inp = R.resample_inputs(n_rays)
    return (inp,) + R.resample_bwd_refs(inp, q7)


@functools.lru_cache(maxsize=None)
def resample_forward(n_rays, q7):
    inp = resample_case(n_rays, q7)[0]
    n = n_rays
    z_all, z_fine = poisoned(n + GUARD, 128), poisoned(n + GUARD, 64)
    above, below, rank = (poisoned(n + GUARD, 64, dtype=torch.int32) for _ in range(3))
    args = [dev(inp[k]) for k in ('z', 'weights', 'u_fine')]
    call('mvnerf_resample', *(ops._p(a) for a in args), n, 64, int(q7), *(ops._p(b) for b in (z_all, z_fine, above, below, rank)))
    return dict(z_all=result(z_all, n), z_fine=result(z_fine, n), above=result(above, n), below=result(below, n),
                fine_rank=result(rank, n), rank_dev=rank[:n])


@pytest.mark.parametrize('q7', Q7_MODES)
@pytest.mark.parametrize('n_rays', R.RESAMPLE_RAYS)
def test_resample_rank_is_the_stable_sort_rank(n_rays, q7):
    """Ties among the importance samples (eight equal u) and between an importance sample and coarse depths (ray 0: u = 0 with
    z_0 = z_1; ray 1: a u chosen to land on a coarse depth) are ordered coarse first, then by index."""
    inp, fwd, _, _ = resample_case(n_rays, q7)
    got = resample_forward(n_rays, q7)
    for k in ('above', 'below', 'z_fine', 'z_all'):               # the float32 forward the backward's reference stands on
        assert np.array_equal(got[k], fwd[k]), k
    assert np.array_equal(got['fine_rank'], R.stable_rank(inp['z'], got['z_fine'].astype(F32)))
    assert np.array_equal(got['fine_rank'], fwd['fine_rank'])
    assert np.array_equal(np.take_along_axis(got['z_all'], got['fine_rank'].astype(np.int64), -1), got['z_fine'])
    assert (got['z_fine'][0, 0] == inp['z'][0, :2]).all() and list(got['fine_rank'][0, 8:16]) == list(range(got['fine_rank'][0, 8], got['fine_rank'][0, 8] + 8))


@pytest.mark.parametrize('q7', Q7_MODES)
@pytest.mark.parametrize('n_rays', R.RESAMPLE_RAYS)
def test_resample_bwd_matches_float64_reference_on_the_float32_forward(n_rays, q7):
    inp, fwd, ref64, ref32 = resample_case(n_rays, q7)
    rank = resample_forward(n_rays, q7)['rank_dev']               # the kernel's own, as in the step
    d_w = poisoned(n_rays + GUARD, 64)
    args = [dev(inp[k]) for k in ('z', 'weights', 'u_fine')] + [rank, dev(inp['d_z_all'])]
    call('mvnerf_resample_bwd', *(ops._p(a) for a in args), n_rays, 64, int(q7), ops._p(d_w))
    got = dict(d_weights=result(d_w, n_rays))
    worst = R.check(f'resample_bwd n={n_rays} q7={q7}:', got, ref64, ref32)
    print(f'RATIO resample_bwd n={n_rays} q7={q7}: {worst:.2f}')
    assert not got['d_weights'][:, 0].any() and not got['d_weights'][:, -1].any()        # probs = weights[1:-1]


# ---- mse_grad -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', (1, 63, 3 * 24, 3 * 4096 + 1))
def test_mse_grad_and_the_loss_it_adds(n):
    """d_pred bit-equal to the float32 restatement (the same two multiplications).  The loss is added into a buffer that held 0.25:
    one atomic per wave, in no fixed order, so the float32 restatement's error is the largest over eight orders of those adds."""
    rng = np.random.default_rng(n)
    pred, label = rng.standard_normal((2, n)).astype(F32)
    d_pred = poisoned(n + GUARD)
    loss = torch.full((1,), 0.25, device=DEV)
    p_dev, l_dev = dev(pred), dev(label)
    call('mvnerf_mse_grad', ops._p(p_dev), ops._p(l_dev), n, ops._p(d_pred), ops._p(loss))
    assert np.array_equal(result(d_pred, n).astype(F32), R.mse_grad_ref(pred, label, F32)[0])
    got = float(loss.cpu()[0])
    want = 0.25 + float(R.mse_grad_ref(pred, label, np.float64)[1])
    waves = -(-n // 64)
    orders = [None, range(waves - 1, -1, -1)] + [np.random.default_rng(k).permutation(waves) for k in range(6)]
    e32 = max(abs(float(R.mse_loss_f32_accumulated(pred, label, 0.25, order)) - want) for order in orders)
    ulp = float(np.spacing(F32(want)))
    e64 = abs(got - want)
    print(f'RATIO mse_grad n={n}: e64 {e64:.3e}  e32 {e32:.3e}  ulp {ulp:.3e}  e64/max(e32, ulp/8) {e64 / max(e32, ulp / R.FACTOR):.2f}')
    assert e64 <= max(R.FACTOR * e32, ulp), (e64, e32, ulp)

    d_same = poisoned(n + GUARD)
    call('mvnerf_mse_grad', ops._p(p_dev), ops._p(p_dev), n, ops._p(d_same), ops._p(loss))
    assert not result(d_same, n).any()
    assert float(loss.cpu()[0]) == got                             # pred == label adds nothing
