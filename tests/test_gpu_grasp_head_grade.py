"""The four kernels of csrc/grasp_head.hip (fwd, vjp<true>, vjp<false>, vjp_bwd) called directly through ops.grasp_head_*, every one of
their ten per-point buffers against the float64 closed forms of tests/grasp_head_ref.py.

Frozen decisions: elu'' jumps at 0 and the kernels decide from the sign of their stored c and y, so the float64 closed forms are evaluated
on the masks of the kernel's c and y (the device tests/test_gpu_field_backward.py uses with the stash); those masks may differ from the
float64 run's own only where a pre-activation is below 1e-5 in magnitude, which is asserted.

Bars: the rule of tests/test_gpu_grasp_tail_train.py, nothing fitted to the kernel.  The yardstick is the same closed forms in plain fp32
torch on the device, on the same inputs, against float64 on the yardstick's own decisions; a kernel figure (relative L2 and worst row, per
64-column block) may be at most FACTOR = 4 times the yardstick's (floor 2e-6) and stays under CAP1 = 1e-5 for c, y, g_v, q, g_u, g_acts and
under CAP2 = 1e-4 for out_gy, r, m, p - the constants that file takes from tests/test_gpu_grasp_head.py.  Each triple is printed first."""
import functools

import pytest
import torch

from tests import grasp_head_ref as R
from tests.grasp_head_ref import NEAR, WEIGHT_SEED, seed_of
from thesis_clip_nerf_amd import lmvnerf as L
from thesis_clip_nerf_amd import ops

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
FACTOR, FLOOR, CAP1, CAP2 = 4.0, 2e-6, 1e-5, 1e-4
# one valid lane and 31 shadows of row 0; a second wave with one valid lane; a second workgroup that is one wave with one valid lane and
# three waves that return; whole tiles only, workgroup 2 with one live wave
SIZES = (1, 33, 129, 160)
SENTINEL = -12345.0
GUARD = 40                                                    # guard rows in front of and behind every buffer (more than a tile)
SHAPES = dict(c=256, y=64, g_v=64, q=256, g_u=256, out_gy=64, r=256, m=64, p=256)


def check(name, err_hip, err_torch, cap):
    bar = min(max(FACTOR * err_torch, FLOOR), cap)
    print(f'{name}: torch fp32 {err_torch:.3e}, hip {err_hip:.3e}, bar {bar:.3e}, ratio {err_hip / max(err_torch, 1e-300):.2f}')
    assert err_hip <= bar, (name, err_hip, err_torch, bar)


def guarded(n, cols, fill, planes=1):
    """(planes x n rows of cols floats, laid out with n as given) inside a larger allocation with GUARD rows on both sides; the guards hold
    `fill`, the rows too -> (whole allocation, view)."""
    big = torch.full((GUARD + planes * n + GUARD, cols), fill, device=DEV)
    view = big[GUARD:GUARD + planes * n]
    return big, (view.view(planes, n, cols) if planes > 1 else view)


def fenced(x):
    """A copy of the input x with NaN rows in front of and behind it: rows past N hold NaN."""
    planes = x.shape[0] if x.dim() == 3 else 1
    big, view = guarded(x.shape[-2], x.shape[-1], float('nan'), planes)
    view.copy_(x)
    return view


def guards_hold(big):
    return bool((big[:GUARD] == SENTINEL).all()) and bool((big[-GUARD:] == SENTINEL).all())


def run_passes(n, acts, g_y, t, w32, packed):
    """The three passes into sentinel-filled guarded outputs, inputs fenced with NaN -> (buffers, allocations)."""
    bigs, out = {}, {}
    for name, cols in SHAPES.items():
        bigs[name], out[name] = guarded(n, cols, SENTINEL)
    for name in ('g_acts', 'g_acts_only'):
        bigs[name], out[name] = guarded(n, 128, SENTINEL, planes=4)
    ops.grasp_head_fwd(acts, packed, w32['b4'], w32['bc'], out=(out['c'], out['y']))
    c_in, y_in = fenced(out['c']), fenced(out['y'])
    ops.grasp_head_vjp(g_y, c_in, y_in, packed, out=(out['g_v'], out['q'], out['g_u'], out['g_acts']))
    ops.grasp_head_vjp_acts(g_y, c_in, y_in, packed, out=out['g_acts_only'])
    ops.grasp_head_vjp_bwd(t, g_y, c_in, y_in, fenced(out['q']), packed, out=(out['out_gy'], out['r'], out['m'], out['p']))
    torch.cuda.synchronize()
    return out, bigs


@functools.lru_cache(maxsize=None)
def case(n):
    """Inputs, the kernels' buffers (two runs), the float64 closed forms on the kernels' decisions and the fp32 yardstick with its own
    float64 counterpart: computed once per size, shared by the tests, never modified."""
    acts, g_y, t = R.inputs(n, seed_of(n))
    w = R.weights(WEIGHT_SEED)
    w64, w32 = R.to(w, torch.float64), R.to(w, torch.float32, DEV)
    a64, g64, t64 = acts.double(), g_y.double(), t.double()
    ad, gd, td = fenced(acts.to(DEV)), fenced(g_y.to(DEV)), fenced(t.to(DEV))
    packed = ops.grasp_head_pack(w32['w4'], w32['wc'])
    runs = [run_passes(n, ad, gd, td, w32, packed) for _ in range(2)]
    plain = ops.grasp_head_fwd(ad, packed, w32['b4'], w32['bc'])                                       # the wrappers' own outputs
    plain += ops.grasp_head_vjp(gd, plain[0], plain[1], packed)
    plain += ops.grasp_head_vjp_bwd(td, gd, plain[0], plain[1], plain[3], packed)
    got = runs[0][0]

    def closed64(pos_c, pos_y):
        return {**R.first_buffers(a64, w64, g64, pos_c, pos_y), **R.second_buffers(a64, w64, g64, t64, pos_c, pos_y)}

    kernel_masks = (got['c'].cpu() > 0, got['y'].cpu() > 0)
    ref = closed64(*kernel_masks)
    yard_masks = R.own_masks(ad, w32)
    yard = {**R.first_buffers(ad, w32, gd, *yard_masks), **R.second_buffers(ad, w32, gd, td, *yard_masks)}
    yard_ref = closed64(yard_masks[0].cpu(), yard_masks[1].cpu())
    torch.cuda.synchronize()
    return dict(runs=runs, plain=plain, ref=ref, yard=yard, yard_ref=yard_ref, kernel_masks=kernel_masks, own=R.own_masks(a64, w64),
                pre=R.pre_activations(a64, w64))


@pytest.mark.parametrize('n', SIZES)
def test_kernel_decisions_differ_from_float64_only_next_to_zero(n):
    c = case(n)
    differ = 0
    for mine, theirs, pre in zip(c['kernel_masks'], c['own'], c['pre']):
        d = mine != theirs
        differ += int(d.sum())
        assert bool((pre[d].abs() < NEAR).all())
    print(f'N={n}: {differ} of {n * 320} decisions differ from the float64 run')


@pytest.mark.parametrize('n', SIZES)
def test_every_buffer_matches_the_float64_closed_forms(n):
    c = case(n)
    got, ref, yard, yard_ref = c['runs'][0][0], c['ref'], c['yard'], c['yard_ref']
    for name in R.FIRST + R.SECOND:
        cap = CAP1 if name in R.FIRST else CAP2
        assert got[name].shape == ref[name].shape and bool(torch.isfinite(got[name]).all()), name
        for (label, g), (_, r), (_, yd), (_, yr) in zip(R.blocks_of(name, got[name]), R.blocks_of(name, ref[name]),
                                                        R.blocks_of(name, yard[name]), R.blocks_of(name, yard_ref[name])):
            check(f'N={n} {label} L2', R.rel(g, r), R.rel(yd, yr), cap)
            check(f'N={n} {label} worst row', R.worst_row(g, r), R.worst_row(yd, yr), cap)


@pytest.mark.parametrize('n', SIZES)
def test_frozen_read_out_form_equals_the_full_pass_bit_for_bit(n):
    c = case(n)
    for out, _ in c['runs']:
        assert torch.equal(out['g_acts_only'], out['g_acts'])


@pytest.mark.parametrize('n', SIZES)
def test_out_keyword_gives_the_bits_of_the_wrappers_own_outputs(n):
    c = case(n)
    out = c['runs'][0][0]
    assert len(c['plain']) == len(R.FIRST + R.SECOND)
    for name, plain in zip(R.FIRST + R.SECOND, c['plain']):
        assert torch.equal(out[name], plain), name


@pytest.mark.parametrize('n', SIZES)
def test_rows_past_n_stay_untouched(n):
    c = case(n)
    for out, bigs in c['runs']:
        for name, big in bigs.items():
            assert guards_hold(big), name                      # the last tile's lanes shadow row N - 1 and must not store
            assert big.shape[0] == 2 * GUARD + (4 * n if name.startswith('g_acts') else n)
            assert bool(torch.isfinite(out[name]).all()), name     # and no valid row took in a NaN from past N


@pytest.mark.parametrize('n', SIZES)
def test_two_runs_give_the_same_bits(n):
    c = case(n)
    (first, _), (second, _) = c['runs']
    for name in first:
        assert torch.equal(first[name], second[name]), name     # p in particular: written, reloaded and rewritten by its own lane


def test_out_keyword_checks_shapes():
    n = 33
    w32 = R.to(R.weights(WEIGHT_SEED), torch.float32, DEV)
    packed = ops.grasp_head_pack(w32['w4'], w32['wc'])
    z = lambda *shape: torch.zeros(shape, device=DEV)
    with pytest.raises(ValueError, match='out y'):
        ops.grasp_head_fwd(z(4, n, 128), packed, w32['b4'], w32['bc'], out=(z(n, 256), z(n + 1, 64)))
    with pytest.raises(ValueError, match='out'):
        ops.grasp_head_vjp(z(n, 64), z(n, 256), z(n, 64), packed, out=(z(n, 64), z(n, 256), z(n, 256)))
    with pytest.raises(ValueError, match='out p'):
        ops.grasp_head_vjp_bwd(z(4, n, 128), z(n, 64), z(n, 256), z(n, 64), z(n, 256), packed, out=(z(n, 64), z(n, 256), z(n, 64), z(n, 128)))


def test_head_fn_at_a_ragged_multiple_of_eight():
    """_HeadFn at N = 136: a multiple of 8 with a ragged last tile, so the weight gradients of _HeadVJP take mvnerf_gemm_tn_batched at two
    splits (N = 41 of tests/test_gpu_grasp_head.py is the torch fallback; 96 and 1536 are whole tiles).  Value, first and second gradients
    against float64 autograd, each tensor under the yardstick rule with torch fp32 autograd of the same layers on the device as yardstick.
    No float64 pre-activation of this seed lies within 1e-5 of zero (tests/test_grasp_head_ref.py), so both runs take the same branches."""
    n = 136
    assert ops.gemm_tn_ok(n, 64, 128) and n % 32 != 0
    acts, g_y, t = R.inputs(n, seed_of(n))
    w = R.weights(WEIGHT_SEED)
    w64, w32 = R.to(w, torch.float64), R.to(w, torch.float32, DEV)
    assert R.near_zero(acts.double(), w64, NEAR)[0] == 0
    y64, first64, second64 = R.autograd_reference(acts.double(), w64, g_y.double(), t.double())
    ad, gd, td = acts.to(DEV), g_y.to(DEV), t.to(DEV)
    y32, first32, second32 = R.autograd_reference(ad, w32, gd, td)
    y, first, second = R.autograd_reference(ad, w32, gd, td, fn=lambda *a: L._HeadFn.apply(*a))
    torch.cuda.synchronize()
    check('N=136 value', R.rel(y, y64), R.rel(y32, y64), CAP1)
    for name, g, g32, g64 in zip(('d acts', 'd w4', 'd b4', 'd wc', 'd bc'), first, first32, first64):
        assert g.shape == g64.shape and bool(torch.isfinite(g).all()), name
        check(f'N=136 {name}', R.rel(g, g64), R.rel(g32, g64), CAP1)
    for name, g, g32, g64 in zip(('dd w4', 'dd b4', 'dd wc', 'dd bc', 'dd g_y'), second, second32, second64):
        assert g.shape == g64.shape and bool(torch.isfinite(g).all()), name
        check(f'N=136 {name}', R.rel(g, g64), R.rel(g32, g64), CAP2)
