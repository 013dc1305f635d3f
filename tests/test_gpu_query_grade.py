"""mvnerf_query_jvp and mvnerf_query_vjp through the C ABI against the frozen-decision float64 reference (oracle/query_ref.py).

tests/test_gpu_query.py compares the two kernels with a free-running float64 twin, whose relu branches and bilinear cells may
differ from the kernel's; its bars (relative L2 3e-2, median per-point error 3e-3) have to cover a flipped row.  Here every decision
is data: the relu masks of the 12 hidden layers come from the stash the kernel itself reads, the bilinear cell and the pass flags of
the clamps from the NumPy fp32 geometry chain that tests/test_gpu_parity.py holds bit-equal to the kernels'.  The float64 run of the
reference then shares every branch with the kernel and the comparison sits at rounding level.

Bar, per output array (t_acts[k], d_points, d_dirs) and for two measures - the tensor-relative L2 and the maximum over points of the
per-point relative error: e64 <= 8 * e32, where e64 is the kernel against the float64 run and e32 the float32 run of the SAME frozen
algebra against the float64 run on the same inputs.  8 = 2^-21 / 2^-24 is the project's factor.  The bar
is computed here from the reference alone; nothing in it is fitted to what the kernels give.  Every figure is printed before it is
asserted (run with -s); DESIGN.md section 10 records them.

Two tiers, same bar.  e32 of the true derivative is 3-6e-5, and nearly all of it is ONE systematic term that the kernels share with
any float32 run: the positional encoding takes sin / cos of the fp32-ROUNDED argument (about 1e3 rad at the top octave, half an ulp
of it is 3e-5 rad), which the derivative passes on at relative size.  Against that term a kernel error of 1e-4 would still pass.  So
every comparison is made a second time ('@arg32') against the derivative of the map with sin / cos taken AT those fp32 arguments
(QueryRef at_arg32: the arguments are those of the NumPy fp32 chain, bit-equal to the kernels'; their tangent is unchanged).  That map
is what the kernels differentiate, the systematic term is gone from both e64 and e32, and e32 drops to 3-5e-7 (L2): plain fp32
rounding of sums of 128 to 379 products.  The kernels' arithmetic is fp32 throughout (fp32 MFMA, ~1.5 ulp sincos), so the same factor
applies.

VJP: the reference takes its masks from the very stash the kernel reads (once written by the fp32-MFMA forward, once by the split
kernel training uses), so no point is left out.  JVP: the kernel keeps no stash; its primal takes an exact sincos per octave where the
stash forward takes double-angle steps, so the two primals differ in the last bits.  The masks come from the fp32-MFMA stash of the
same points, and a point is left out of the rounding-level assertions if any of its stashed pre-activations lies within
2e-5 * max(1, max |slot|) of zero (the project's primal-agreement bar); at most 1/4 of a case's points may be left out (asserted
here, and beforehand on the CPU in tests/test_query_ref.py), and those points still meet the old bound of test_gpu_query.check_close.

Every buffer a pass reads without having written it would show: stash, scratch and workspace are filled with NaN first, and the
outputs are views into larger NaN-filled buffers whose guard floats on both sides must stay untouched.
"""
import functools

import numpy as np
import pytest
import torch

from oracle import field_backward_ref as R
from oracle import query_ref as Q
from tests.test_gpu_query import check_close, make_query
from thesis_clip_nerf_amd import ops

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
FACTOR = 8.0
GUARD = 64                       # floats on either side of an output (keeps its 16-byte alignment)
MAX_LEFT_OUT = 0.25
HW = (16, 20)
# (B, V, N, noise on the points, seed)
CASES = [(1, 1, 33, 0.0, 211),       # ragged: one valid row in the second tile
         (1, 1, 160, 0.0, 212),      # five tiles, two workgroups, the last one partial
         (2, 2, 64, 0.0, 213),       # batch boundary, per-scene cameras
         (1, 3, 96, 0.0, 214),       # 1 / V is not a power of two
         (1, 1, 64, 0.6, 215),       # scattered: most pairs outside the image, some behind the camera or at the +-1e6 clip
         (2, 2, 32, 0.6, 216)]
IDS = [f'B{b}V{v}N{n}' + ('scattered' if s else '') for b, v, n, s, _ in CASES]
PATHS = ('mfma', 'split')
TIERS = {'': {}, '@arg32': {'at_arg32': True}}          # suffix of the array's name -> arguments of the reference
DTYPES = {64: torch.float64, 32: torch.float32}


@functools.lru_cache(maxsize=None)
def case_inputs(i):
    """Scene, points, tangents, cotangents and the reference object of case i (host only: tests/test_query_ref.py uses the same)."""
    b, v, n, noise, seed = CASES[i]
    sc, points, dirs = make_query(seed, v, n, b, HW)
    rng = np.random.default_rng(seed + 1)
    if noise:
        points = (points + noise * rng.standard_normal(points.shape)).astype(np.float32)
    tp = rng.standard_normal(points.shape).astype(np.float32)
    td = rng.standard_normal(dirs.shape).astype(np.float32)
    g = rng.standard_normal((4, b, n, 128)).astype(np.float32)
    ref = Q.QueryRef(sc['fine'], sc['images'], sc['features'], sc['intrinsics'], sc['extrinsics_inv'], points, dirs)
    return dict(sc=sc, points=points, dirs=dirs, tp=tp, td=td, g=g, ref=ref)


def bar(tag, arrays, keep=None):
    """arrays: [(name, got, ref64, ref32)].  Prints e64, e32 and their ratio per array and measure, returns (the list of measures
    over the bar, the largest ratio)."""
    bad, worst = [], 0.0
    for name, got, r64, r32 in arrays:
        for kind, e64, e32 in zip(('L2', 'max'), Q.errors(got, r64, keep), Q.errors(r32, r64, keep)):
            ratio = e64 / e32 if e32 > 0 else (0.0 if e64 == 0 else np.inf)
            print(f'{tag} {name:15s} {kind:3s}: e64 {e64:.3e}  e32 {e32:.3e}  e64/e32 {ratio:.2f}')
            worst = max(worst, ratio)
            if not e64 <= FACTOR * e32:
                bad.append((name, kind, e64, e32, ratio))
    print(f'{tag} largest e64/e32: {worst:.2f}')
    return bad, worst


def vjp_arrays(got, ref, tiers=TIERS):
    """The arrays the VJP's bar is applied to; ref[tier, bits] = (d_points, d_dirs)."""
    return [(name + tier, got[k], ref[tier, 64][k], ref[tier, 32][k]) for tier in tiers for k, name in enumerate(('d_points', 'd_dirs'))]


def jvp_arrays(got, ref, tiers=TIERS):
    """The arrays the JVP's bar is applied to; ref[tier, bits] = t_acts (4,B,N,128)."""
    return [(f't_acts[{k}]{tier}', got[k], ref[tier, 64][k], ref[tier, 32][k]) for tier in tiers for k in range(4)]


def transpose_residual(g, t_acts, d_points, d_dirs, tp, td, scale, keep):
    """max over the kept points n of |<g_n, (J t)_n> - <(J^T g)_n, t_n>| / scale_n (all float64)."""
    lhs = (np.asarray(g, np.float64) * t_acts).sum((0, 3))
    rhs = (d_points * np.asarray(tp, np.float64)).sum(-1) + (d_dirs * np.asarray(td, np.float64)).sum(-1)
    return float((np.abs(lhs - rhs) / scale)[keep].max())


def transpose_scale(g, t_acts64, d_points64, d_dirs64, tp, td):
    """sum of |products| of both sides of the identity, per point, from the float64 reference: what the rounding of either side scales with."""
    return (np.abs(np.asarray(g, np.float64) * t_acts64).sum((0, 3)) + np.abs(d_points64 * tp).sum(-1) + np.abs(d_dirs64 * td).sum(-1))


# ---- device side ----------------------------------------------------------------------------------------------------------------
def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def poisoned(n_bytes):
    """n_bytes of device memory holding the quiet-NaN pattern 0x7FC00000 in every float."""
    assert n_bytes % 4 == 0
    return torch.full((n_bytes // 4,), 0x7FC00000, dtype=torch.int32, device=DEV).view(torch.uint8)


class Guarded:
    """An output of `shape` as a view into a NaN-filled buffer with GUARD floats on either side."""

    def __init__(self, shape):
        n = int(np.prod(shape))
        self.buf = poisoned(4 * (n + 2 * GUARD)).view(torch.float32)
        self.out = self.buf[GUARD:GUARD + n].view(shape)

    def read(self):
        assert torch.isnan(self.buf[:GUARD]).all() and torch.isnan(self.buf[-GUARD:]).all(), 'guard floats written'
        assert torch.isfinite(self.out).all()
        return self.out.cpu().numpy().astype(np.float64)


@functools.lru_cache(maxsize=None)
def device_case(i):
    """Case i on the device: both forwards into NaN-filled stashes, decoded on the host."""
    b, v, n, _, _ = CASES[i]
    c = case_inputs(i)
    d = {k: dev(c['sc'][k]) for k in ('images', 'features', 'intrinsics', 'extrinsics_inv', 'fine')}
    geo = (d['images'], d['features'], d['intrinsics'], d['extrinsics_inv'])
    pts, dirs = dev(c['points']), dev(c['dirs'])
    packed, split, streams = ops.pack_net(d['fine']), ops.pack_net_split(d['fine']), ops.pack_bwd_streams(d['fine'])
    stash, rows = {}, {}
    for path in PATHS:
        buf = poisoned(ops.stash_bytes(b, v, n, 1))
        out = ops.query_stash(pts, dirs, *geo, packed, stash=buf, packed_split=split if path == 'split' else None)
        assert out.data_ptr() == buf.data_ptr()
        torch.cuda.synchronize()
        stash[path] = buf
        rows[path] = R.decode_stash(buf.view(torch.float32).cpu().numpy(), b, v, n, 1)
        for name in Q.VIEW_MASKS + Q.FUSED_MASKS:
            assert np.isfinite(rows[path][name]).all(), (path, name)
    return dict(geo=geo, pts=pts, dirs=dirs, packed=packed, streams=streams, stash=stash, rows=rows)


def run_vjp(i, path, g):
    b, v, n, _, _ = CASES[i]
    dc = device_case(i)
    dp, dd = Guarded((b, n, 3)), Guarded((b, n, 3))
    scratch = poisoned(int(ops._lib.lib().mvnerf_query_vjp_scratch_bytes(b, v, n)))
    g = g.contiguous()
    with torch.cuda.device(DEV):
        rc = ops._lib.lib().mvnerf_query_vjp(ops._p(dc['pts']), ops._p(dc['dirs']), *[ops._p(a) for a in dc['geo']], ops._p(dc['streams']),
                                             ops._p(dc['stash'][path]), ops._p(g), b, v, n, HW[0], HW[1], ops._p(scratch), ops._p(dp.out),
                                             ops._p(dd.out), ops._stream(dc['pts']))
    ops._lib.check(rc, 'query_vjp')
    torch.cuda.synchronize()
    return dp, dd


def run_jvp(i, tp, td):
    b, v, n, _, _ = CASES[i]
    dc = device_case(i)
    t_acts = Guarded((4, b, n, 128))
    ws = poisoned(int(ops._lib.lib().mvnerf_query_workspace_bytes(b, v, n)))
    tp, td = tp.contiguous(), td.contiguous()
    with torch.cuda.device(DEV):
        rc = ops._lib.lib().mvnerf_query_jvp(ops._p(dc['pts']), ops._p(dc['dirs']), ops._p(tp), ops._p(td), *[ops._p(a) for a in dc['geo']],
                                             ops._p(dc['packed']), b, v, n, HW[0], HW[1], None, ops._p(t_acts.out), ops._p(ws),
                                             ops._stream(dc['pts']))
    ops._lib.check(rc, 'query_jvp')
    torch.cuda.synchronize()
    return t_acts


@functools.lru_cache(maxsize=None)
def vjp_reference(i, path):
    c, ref = case_inputs(i), case_inputs(i)['ref']
    masks = ref.masks_from_rows(device_case(i)['rows'][path])
    return {(tier, bits): ref.vjp(c['g'], masks, dtype, **kw) for tier, kw in TIERS.items() for bits, dtype in DTYPES.items()}


@functools.lru_cache(maxsize=None)
def jvp_reference(i):
    c, ref = case_inputs(i), case_inputs(i)['ref']
    rows = device_case(i)['rows']['mfma']
    masks = ref.masks_from_rows(rows)
    out = {(tier, bits): ref.jvp(c['tp'], c['td'], masks, dtype, **kw) for tier, kw in TIERS.items() for bits, dtype in DTYPES.items()}
    out['keep'] = ~ref.near_zero_points(rows)
    return out


@functools.lru_cache(maxsize=None)
def kernel_vjp(i, path):
    dp, dd = run_vjp(i, path, dev(case_inputs(i)['g']))
    return dp.read(), dd.read()


@functools.lru_cache(maxsize=None)
def kernel_jvp(i):
    c = case_inputs(i)
    return run_jvp(i, dev(c['tp']), dev(c['td'])).read()


# ---- rounding-level comparisons -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('path', PATHS)
@pytest.mark.parametrize('i', range(len(CASES)), ids=IDS)
def test_query_vjp_matches_float64_reference_on_its_own_stash(i, path):
    got, ref = kernel_vjp(i, path), vjp_reference(i, path)
    bad, _ = bar(f'vjp {IDS[i]} {path}:', vjp_arrays(got, ref))
    assert not bad, bad


@pytest.mark.parametrize('i', range(len(CASES)), ids=IDS)
def test_query_jvp_matches_float64_reference_with_stash_masks(i):
    got, ref = kernel_jvp(i), jvp_reference(i)
    keep = ref['keep']
    left_out = 1.0 - keep.mean()
    print(f'jvp {IDS[i]}: share of points left out {left_out:.3f}')
    assert left_out <= MAX_LEFT_OUT, left_out
    bad, _ = bar(f'jvp {IDS[i]}:', jvp_arrays(got, ref), keep)
    assert not bad, bad
    if (~keep).any():
        for k in range(4):
            check_close(got[k][~keep], ref['', 64][k][~keep], f'left-out t_acts[{k}]')


@pytest.mark.parametrize('i', range(len(CASES)), ids=IDS)
def test_query_jvp_is_the_transpose_of_vjp_point_by_point(i):
    """J is block-diagonal per point, so <g_n, (J t)_n> = <(J^T g)_n, t_n> for every point n (outside the JVP's left-out set).  The
    residual is taken relative to the sum of the absolute products of both sides (what either side's rounding scales with, from the
    float64 reference); its maximum over the points must not exceed 8 times the same figure between the two float32 references."""
    c = case_inputs(i)
    keep = jvp_reference(i)['keep']
    j, v = ({bits: r['', bits] for bits in DTYPES} for r in (jvp_reference(i), vjp_reference(i, 'mfma')))
    scale = transpose_scale(c['g'], j[64], *v[64], c['tp'], c['td'])
    assert (scale[keep] > 0).all()
    r32 = transpose_residual(c['g'], j[32], *v[32], c['tp'], c['td'], scale, keep)
    r64 = transpose_residual(c['g'], j[64], *v[64], c['tp'], c['td'], scale, keep)
    got = transpose_residual(c['g'], kernel_jvp(i), *kernel_vjp(i, 'mfma'), c['tp'], c['td'], scale, keep)
    print(f'transpose {IDS[i]}: kernels {got:.3e}  float32 references {r32:.3e}  ratio {got / r32:.2f}  (float64 references {r64:.1e})')
    assert r64 < 1e-12, r64
    assert got <= FACTOR * r32, (got, r32)


def test_query_vjp_of_a_point_with_all_clamps_closed_is_the_pe_path_alone():
    """V = 1, scattered: where both coordinates' pass flags are off nothing flows through the gather, and d_points is the positional
    encoding's part alone - the reference with the gather removed, same bar."""
    i = 4
    c, ref = case_inputs(i), case_inputs(i)['ref']
    closed = ~ref.pass_xy.any(-1)[:, 0]                                          # (B,N)
    assert closed.sum() >= 8, closed.sum()
    masks = ref.masks_from_rows(device_case(i)['rows']['mfma'])
    cut = {(tier, bits): ref.vjp(c['g'], masks, dtype, gather=False, **kw) for tier, kw in TIERS.items() for bits, dtype in DTYPES.items()}
    bad, _ = bar('vjp closed clamps:', vjp_arrays(kernel_vjp(i, 'mfma'), cut), closed)
    assert not bad, bad


# ---- exact properties -------------------------------------------------------------------------------------------------------------
def test_zero_tangent_and_zero_cotangent_give_exactly_zero():
    for i in (1, 2):
        c = case_inputs(i)
        t_acts = run_jvp(i, torch.zeros_like(dev(c['tp'])), torch.zeros_like(dev(c['td']))).read()
        assert not np.count_nonzero(t_acts), i
        for out in run_vjp(i, 'mfma', torch.zeros_like(dev(c['g']))):
            assert not np.count_nonzero(out.read()), i


@pytest.mark.parametrize('i', [1, 3], ids=[IDS[1], IDS[3]])
def test_query_jvp_is_homogeneous_under_powers_of_two(i):
    """J (2^k t) = 2^k J t bit for bit: the tangent path is linear in t and a power of two commutes with every rounding in it."""
    c = case_inputs(i)
    tp, td = dev(c['tp']), dev(c['td'])
    base = run_jvp(i, tp, td).read()
    assert np.abs(base).max() > 0
    for k in (10, -10):
        assert np.array_equal(run_jvp(i, tp * 2.0 ** k, td * 2.0 ** k).read(), base * 2.0 ** k), k


@pytest.mark.parametrize('i', [1, 2], ids=[IDS[1], IDS[2]])
def test_query_vjp_is_equivariant_under_powers_of_two(i):
    """Multiplying g_acts by 2^k multiplies d_points and d_dirs by 2^k: bit for bit at V = 1; with more views the per-point sum over the
    views is accumulated with fp32 atomics, order-dependent in the last bit (the bar of test_gpu_train's field-backward twin)."""
    g = dev(case_inputs(i)['g'])
    base = [o.read() for o in run_vjp(i, 'mfma', g)]
    assert all(np.abs(a).max() > 0 for a in base)
    for k in (10, -10):
        for a, o in zip(base, run_vjp(i, 'mfma', g * 2.0 ** k)):
            if CASES[i][1] == 1:
                assert np.array_equal(o.read(), a * 2.0 ** k), k
            else:
                assert np.abs(o.read() - a * 2.0 ** k).max() <= 1e-5 * np.abs(a * 2.0 ** k).max(), k


def test_repeated_runs_are_bit_identical_with_one_view():
    i = 1
    c = case_inputs(i)
    first = run_jvp(i, dev(c['tp']), dev(c['td'])).read()
    assert np.array_equal(first, kernel_jvp(i))
    again = [o.read() for o in run_vjp(i, 'mfma', dev(c['g']))]
    for a, b in zip(again, kernel_vjp(i, 'mfma')):
        assert np.array_equal(a, b)
