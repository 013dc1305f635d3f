"""oracle/query_ref.py on the CPU: the frozen-decision reference of the query map is the derivative of the free-running float64 twin
wherever the two take the same decisions, the input sets of tests/test_gpu_query_grade.py meet that file's conditions, and its bar
rejects every planted error (the bar function and the inputs are imported from the GPU test, not copied)."""
import functools

import numpy as np
import pytest
import torch

from oracle import mvnerf_torch as T
from oracle import query_ref as Q
from tests import test_gpu_query_grade as G

N_CASES = len(G.CASES)
SCATTERED = [i for i, c in enumerate(G.CASES) if c[3]]


def t64(a):
    return torch.as_tensor(np.asarray(a)).to(torch.float64)


@functools.lru_cache(maxsize=None)
def own(i):
    """Case i with the masks of the reference's own float32 forward, and the float64 / float32 derivatives under them."""
    c = G.case_inputs(i)
    ref = c['ref']
    rows32 = ref.rows(torch.float32)
    masks = ref.masks_from_rows(rows32)
    out = dict(c, rows32=rows32, masks=masks, keep=~ref.near_zero_points(rows32))
    for tier, kw in G.TIERS.items():
        for bits, dt in G.DTYPES.items():
            out['jvp' + tier, bits] = ref.jvp(c['tp'], c['td'], masks, dt, **kw)
            out['vjp' + tier, bits] = ref.vjp(c['g'], masks, dt, **kw)
    return out


def arrays(kind, got, c, tier=''):
    """The GPU test's arrays of one product and one tier, with `got` in the kernel's place."""
    ref = {(tier, bits): c[kind + tier, bits] for bits in G.DTYPES}
    return (G.jvp_arrays if kind == 'jvp' else G.vjp_arrays)(got, ref, (tier,))


@pytest.mark.parametrize('i', range(N_CASES), ids=G.IDS)
def test_frozen_reference_is_the_derivative_of_the_free_float64_twin(i):
    """Masks and cells from the float32 forward; on the points where the free float64 run of oracle/mvnerf_torch.query_acts takes the
    same decisions, J t and J^T g agree to 1e-12 of the tensor's largest entry.  The share of points where they differ is <= 2 %."""
    c = own(i)
    ref, sc = c['ref'], c['sc']
    net = T.unflatten_net(t64(sc['fine']))
    geo = (t64(sc['images']), t64(sc['features']), t64(sc['intrinsics']), t64(sc['extrinsics_inv']))

    def free(points, dirs):
        return torch.stack(T.query_acts(net, points, dirs, *geo), 0)
    x = (t64(c['points']), t64(c['dirs']))
    acts_free, jt_free = torch.autograd.functional.jvp(free, x, (t64(c['tp']), t64(c['td'])))
    _, (dp_free, dd_free) = torch.autograd.functional.vjp(free, x, t64(c['g']))
    # the decisions of the free float64 run
    pix64, _ = T.compute_pixel_in_image_mv(x[0][:, :, None, :], geo[2], geo[3])
    pix64 = pix64[:, :, :, 0].numpy()                                                               # (B,V,N,2)
    hi = np.array([ref.W - 2, ref.H - 2], np.float64)
    cell64 = np.clip(np.floor(pix64), 0, hi)
    u64 = pix64 - cell64
    pass64 = (u64 >= 0) & (u64 <= 1) & (np.abs(pix64) < 1e6)
    differ = (cell64 != ref.cell).any(-1) | (pass64 != ref.pass_xy).any(-1)
    # behind the camera the twin divides by the double 1e-8, the kernels by fl32(1e-8): a different function unless the clip swallows it
    differ |= ~ref.pass_q2 & ref.pass_clip.any(-1)
    differ = differ.any(1)                                                                          # (B,N)
    rows64 = ref.rows(torch.float64)
    for name in Q.VIEW_MASKS + Q.FUSED_MASKS:
        flip = ((c['rows32'][name] > 0) != (rows64[name] > 0)).any(-1)
        differ |= flip.reshape(ref.B, ref.V, ref.N).any(1) if name in Q.VIEW_MASKS else flip.reshape(ref.B, ref.N)
    print(f'{G.IDS[i]}: float32 and float64 decisions differ on {differ.mean():.4f} of the points')
    assert differ.mean() <= 0.02, differ.mean()
    same = ~differ
    acts64, _ = ref.forward(torch.float64, c['masks'])
    for name, got, want in (('acts', acts64, acts_free.numpy()), ('J t', c['jvp', 64], jt_free.numpy())):
        err = np.abs(got - want)[:, same].max() / np.abs(want).max()
        print(f'{G.IDS[i]}: {name} {err:.2e}')
        assert err < 1e-12, (name, err)
    for name, got, want in (('d_points', c['vjp', 64][0], dp_free.numpy()), ('d_dirs', c['vjp', 64][1], dd_free.numpy())):
        err = np.abs(got - want)[same].max() / np.abs(want).max()
        print(f'{G.IDS[i]}: {name} {err:.2e}')
        assert err < 1e-12, (name, err)


@pytest.mark.parametrize('i', range(N_CASES), ids=G.IDS)
def test_inputs_of_the_gpu_test_meet_its_conditions(i):
    """At most 1/4 of a case's points have a float32 pre-activation within 2e-5 * max(1, max |slot|) of zero; the plain cases keep every
    point in front of the cameras, the scattered ones reach the closed clamps."""
    c = own(i)
    ref = c['ref']
    left_out = 1.0 - c['keep'].mean()
    outside, behind = ref.outside_image().mean(), ref.behind_or_clipped().mean()
    print(f'{G.IDS[i]}: left out {left_out:.3f}, (view, point) pairs outside the image {outside:.2f}, behind the camera or clipped {behind:.2f}')
    assert left_out <= G.MAX_LEFT_OUT, left_out
    if i in SCATTERED:
        assert outside >= 0.6 and behind >= 0.05, (outside, behind)
    else:
        assert 0.1 <= outside <= 0.5 and behind == 0, (outside, behind)


def test_float32_yardstick_table():
    """The figures behind the GPU test's bars (printed): what float32 arithmetic costs on the frozen algebra.  They
    sit far below the 3e-3 / 3e-2 of tests/test_gpu_query.check_close - two digits of room that file's bars cannot see into."""
    for i in range(N_CASES):
        c = own(i)
        for kind in ('jvp', 'vjp'):
            keep = c['keep'] if kind == 'jvp' else None
            for tier in G.TIERS:
                for name, _, r64, r32 in arrays(kind, c[kind + tier, 32], c, tier):
                    l2, mx = Q.errors(r32, r64, keep)
                    print(f'{G.IDS[i]} {name:15s} e32 L2 {l2:.2e} max {mx:.2e}')
                    assert l2 < 3e-4 and mx < 3e-3, (i, name, l2, mx)


def expected_identity(mutant, ref):
    """The inputs on which a planted error cannot show, by construction."""
    if mutant == 'inv_v_twice':
        return ref.V == 1                                      # 1 / V = 1
    if mutant == 'clamp_open_behind_camera':
        return bool(ref.pass_clip.all() and ref.pass_q2.all())   # no point behind a camera or at the clip: the clamp is never closed
    return False


@pytest.mark.parametrize('mutant', sorted(Q.MUTANTS))
def test_bar_of_the_gpu_test_rejects_planted_errors(mutant):
    """Each planted error, computed in float32 on every input set of the GPU test, is over the bar in at least one array of each product
    it concerns - except on inputs where it is the identity by construction, which is asserted instead."""
    shown = 0
    for i in range(N_CASES):
        c = own(i)
        ref = c['ref']
        for kind in ('jvp', 'vjp'):
            if Q.MUTANTS[mutant] not in (kind, 'both'):
                continue
            if kind == 'jvp':
                got, keep = ref.jvp(c['tp'], c['td'], c['masks'], torch.float32, mutant), c['keep']
                same = np.array_equal(got, c['jvp', 32])
            else:
                got, keep = ref.vjp(c['g'], c['masks'], torch.float32, mutant), None
                same = all(np.array_equal(a, b) for a, b in zip(got, c['vjp', 32]))
            if expected_identity(mutant, ref):
                assert same, (mutant, i, kind)
                continue
            bad, _ = G.bar(f'{mutant} {G.IDS[i]} {kind}:', arrays(kind, got, c), keep)
            assert bad, (mutant, i, kind)
            shown += 1
    assert shown >= 2, mutant


def test_bar_of_the_gpu_test_accepts_the_float32_run_itself():
    for i in range(N_CASES):
        c = own(i)
        for kind in ('jvp', 'vjp'):
            for tier in G.TIERS:
                bad, worst = G.bar(f'float32 {G.IDS[i]} {kind}:', arrays(kind, c[kind + tier, 32], c, tier), c['keep'] if kind == 'jvp' else None)
                assert not bad and worst == 1.0


def test_second_tier_sees_what_the_rounded_pe_argument_hides():
    """The view mean scaled by 1 + 3e-5: below the first tier's bar (e32 there is 3-6e-5, the rounded argument of the positional
    encoding), over the second tier's, where sin / cos are taken at the fp32 arguments on both sides."""
    for i in range(N_CASES):
        c = own(i)
        ref = c['ref']
        for tier, kw in G.TIERS.items():
            got = ref.jvp(c['tp'], c['td'], c['masks'], torch.float32, 'view_mean_scaled', eps=3e-5, **kw)
            bad, _ = G.bar(f'1 + 3e-5 {G.IDS[i]} jvp:', arrays('jvp', got, c, tier), c['keep'])
            assert bool(bad) == (tier == '@arg32'), (i, tier, bad)


def test_closed_clamps_leave_the_pe_path_alone():
    """The points the GPU test's closed-clamp case selects: with both pass flags off, removing the gather changes nothing in d_points."""
    c = own(4)
    ref = c['ref']
    closed = ~ref.pass_xy.any(-1)[:, 0]
    assert ref.V == 1 and closed.sum() >= 8 and (~closed).sum() >= 8
    full, cut = c['vjp', 64], ref.vjp(c['g'], c['masks'], torch.float64, gather=False)
    assert np.array_equal(full[0][closed], cut[0][closed]) and np.array_equal(full[1], cut[1])
    assert np.abs(full[0][~closed] - cut[0][~closed]).max() > 1e-3 * np.abs(full[0]).max()
