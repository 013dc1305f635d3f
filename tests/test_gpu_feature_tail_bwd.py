"""mvnerf_fuse_upsample2x_bwd (csrc/feature_tail_bwd.hip) through ops.fuse_upsample2x_bwd, against the float64 reference
of tests/feature_tail_bwd_ref.py.

Bar: the kernel's error against float64 may be at most 8 x the error e32 of torch's float32 CPU autograd of the same tail, as relative
L2 and as worst element over largest magnitude, for da, db and g_low each.  Then what makes a fused pass go wrong without being
inaccurate: writes outside the outputs, elements left unwritten, the need flags, exact small-integer data, the adjoint identity with
the forward kernel, the closed form of an impulse at corners, edges and tile seams, power-of-two scaling, the relu mask at zero, the
footprint of a NaN, offsets beyond 2^31 elements and run-to-run determinism."""
import itertools

import numpy as np
import pytest
import torch

from tests import feature_tail_bwd_ref as B
from thesis_clip_nerf_amd import ops

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
GUARD = 2                                          # guard rows (of w x C elements) in front of and behind every output
GUARD_WORD = 0x7FA5A5A5                            # a NaN no arithmetic produces
FILLS = (0x00000000, 0x7FC00000, 0x3F800000)
NAMES = ('da', 'db', 'g_low')


def dev(x):
    return torch.from_numpy(np.array(x)).to(DEV)                      # (a copy: the cached cases are read-only)


def guarded(shape, fill):
    """An output of `shape` (N, h, w, C) filled with the word `fill`, between guard rows -> (whole int32 buffer, the output as float32)."""
    n, h, w, c = shape
    row = w * c
    buf = torch.full(((n * h + 2 * GUARD) * row,), GUARD_WORD, dtype=torch.int32, device=DEV)
    body = buf[GUARD * row:buf.numel() - GUARD * row]
    body.fill_(fill if fill < 2 ** 31 else fill - 2 ** 32)
    return buf, body.view(torch.float32).view(n, h, w, c)


def guards_kept(buf, shape):
    row = shape[2] * shape[3]
    return bool((buf[:GUARD * row] == GUARD_WORD).all() and (buf[buf.numel() - GUARD * row:] == GUARD_WORD).all())


def run(g, a, b, weight, act, fill=0x7FC00000, needs=(True, True, True)):
    """One call into filled, guarded outputs -> {name: tensor | None}; asserts that the guards kept their word."""
    n, h, w, ca = a.shape
    shapes = ((n, h, w, ca), (n, h, w, b.shape[3]), (n, h, w, 256))
    bufs = [guarded(s, fill) if need else (None, None) for s, need in zip(shapes, needs)]
    got = ops.fuse_upsample2x_bwd(g, a, b, weight, act, *needs, out=tuple(o for _, o in bufs))
    torch.cuda.synchronize()
    for (buf, out), result, shape, need in zip(bufs, got, shapes, needs):
        assert (result is None) == (not need)
        if need:
            assert result.data_ptr() == out.data_ptr() and guards_kept(buf, shape), 'wrote outside an output'
    return dict(zip(NAMES, got))


def bits(t):
    return t.view(torch.int32)


_runs = {}


def kernel_runs(shape):
    """One run per fill word and shape, shared by the tests below."""
    if shape not in _runs:
        a, b, weight, g, _, _ = B.case(shape)
        args = [dev(t) for t in (g, a, b, weight)]
        _runs[shape] = [run(*args, shape[5], fill=fill) for fill in FILLS]
    return _runs[shape]


@pytest.mark.parametrize('shape', B.SHAPES, ids=str)
def test_against_the_float64_reference(shape):
    _, _, _, _, ref, e32 = B.case(shape)
    got = {k: v.cpu().numpy() for k, v in kernel_runs(shape)[1].items()}
    assert all(np.isfinite(v).all() for v in got.values()), 'left elements unwritten'
    B.assert_at_bar(got, ref, e32, f'kernel {shape}')


@pytest.mark.parametrize('shape', B.SHAPES, ids=str)
def test_results_do_not_depend_on_what_the_outputs_held(shape):
    first, *others = kernel_runs(shape)
    for other in others:
        for name in NAMES:
            assert torch.equal(bits(first[name]), bits(other[name])), name


@pytest.mark.parametrize('shape', [(2, 9, 11, 128, 256, 'elu'), (1, 17, 33, 32, 16, None), (1, 1, 1, 16, 16, 'relu')], ids=str)
def test_every_combination_of_need_flags(shape):
    a, b, weight, g, _, _ = B.case(shape)
    args = [dev(t) for t in (g, a, b, weight)]
    full = kernel_runs(shape)[0]
    for needs in itertools.product((True, False), repeat=3):
        if not any(needs):
            with pytest.raises(ValueError, match='nothing asked for'):
                ops.fuse_upsample2x_bwd(*args, shape[5], False, False, False)
            continue
        got = run(*args, shape[5], needs=needs)
        for name, need in zip(NAMES, needs):
            assert (got[name] is not None) == need
            if need:
                assert torch.equal(bits(got[name]), bits(full[name])), (needs, name)
    # a buffer that is handed over but not asked for is not touched
    spare = [torch.full_like(full[name], 7.0) for name in NAMES]
    got = ops.fuse_upsample2x_bwd(*args, shape[5], False, True, False, out=tuple(spare))
    assert got[0] is None and got[2] is None and got[1].data_ptr() == spare[1].data_ptr()
    assert bool((spare[0] == 7.0).all() and (spare[2] == 7.0).all()) and torch.equal(bits(got[1]), bits(full['db']))


def test_small_integers_are_exact_and_the_adjoint_identity_holds():
    a, b, weight, g = B.integer_case()
    ref = B.tail_bwd_ref(g, a, b, weight, None)
    got = {k: v.cpu().numpy() for k, v in run(dev(g), dev(a), dev(b), dev(weight), None).items()}
    for name in NAMES:
        assert np.array_equal(got[name].astype(np.float64), ref[name]), name
    assert 100 < max(np.abs(ref['da']).max(), np.abs(ref['db']).max()) < 200
    # <out, g> = <a, da> + <b, db> with the forward kernel's out (the identity: the tail is linear in [a | b]), exactly, in float64
    out = ops.fuse_upsample2x(dev(a), dev(b), dev(weight), None).cpu().numpy().astype(np.float64)
    left = float((out * g.astype(np.float64)).sum())
    right = float((a.astype(np.float64) * got['da']).sum() + (b.astype(np.float64) * got['db']).sum())
    assert left == right and left != 0.0


def test_impulses_at_corners_edges_seams_and_inside():
    """A unit impulse in g, a weight of small integers / 8, the identity: da | db is {9, 3, 3, 1} / 16 of the weight's column at the <= 4
    low pixels the output pixel reads (the folded values at the border), zero elsewhere, bit for bit.  9 x 19 low pixels: two tiles
    each way; the seams are low rows 7 | 8 and low columns 15 | 16."""
    h, w, ca, cb = 9, 19, 16, 32
    rng = np.random.default_rng(3)
    weight = rng.integers(-8, 9, (ca + cb, 256)).astype(np.float32) / 8
    places = [(0, 0), (0, 2 * w - 1), (2 * h - 1, 0), (2 * h - 1, 2 * w - 1), (0, 9), (2 * h - 1, 20), (7, 0), (8, 2 * w - 1),
              (15, 31), (16, 32), (15, 32), (16, 31), (14, 30), (17, 33), (5, 9)]
    cs = [int(c) for c in rng.integers(0, 256, len(places))]
    cs[0], cs[1] = 0, 255
    g = np.zeros((len(places), 2 * h, 2 * w, 256), np.float32)
    for n, ((py, px), c) in enumerate(zip(places, cs)):
        g[n, py, px, c] = 1.0
    zeros = lambda c: torch.zeros(len(places), h, w, c, device=DEV)
    got = {k: v.cpu().numpy() for k, v in run(dev(g), zeros(ca), zeros(cb), dev(weight), None).items()}
    uy, ux = B.upsample_matrix(h), B.upsample_matrix(w)
    for n, ((py, px), c) in enumerate(zip(places, cs)):
        spread = (uy[py][:, None] * ux[px][None, :]).astype(np.float32)                      # sixteenths
        assert 1 <= np.count_nonzero(spread) <= 4 and spread.sum() == 1.0
        want = spread[:, :, None] * weight[None, None, :, c]
        assert np.array_equal(got['da'][n], want[..., :ca]) and np.array_equal(got['db'][n], want[..., ca:]), (py, px, c)
        low = np.zeros((h, w, 256), np.float32)
        low[:, :, c] = spread
        assert np.array_equal(got['g_low'][n], low), (py, px, c)


def test_power_of_two_scaling_is_bit_exact():
    shape = (1, 9, 11, 128, 256, 'elu')
    a, b, weight, g, _, _ = B.case(shape)
    args = [dev(t) for t in (a, b, weight)]
    base = kernel_runs(shape)[0]
    for j in (-3, 5):
        scaled = run(dev(g * np.float32(2.0 ** j)), *args, 'elu')
        for name in NAMES:
            assert torch.equal(bits(scaled[name]), bits(base[name] * 2.0 ** j)), (j, name)
    zero = run(torch.zeros_like(dev(g)), *args, 'elu')
    assert not any(bool(zero[name].any()) for name in NAMES)                                 # all-zero g gives zeros


def test_relu_masks_at_minus_one_and_both_zeros():
    shape = (1, 9, 17, 16, 32, 'relu')
    _, _, weight, g, _, _ = B.case(shape)
    values = np.float32([-1.0, -0.0, 0.0])
    a = np.resize(values, (1, 9, 17, 16)).astype(np.float32)
    b = np.resize(values[::-1], (1, 9, 17, 32)).astype(np.float32)
    got = run(dev(g), dev(a), dev(b), dev(weight), 'relu')
    assert not bool(got['da'].any()) and not bool(got['db'].any()) and bool(got['g_low'].any())
    nan_g = run(torch.full_like(dev(g), float('nan')), dev(a), dev(b), dev(weight), 'relu')   # a masked element is 0 whatever d is
    assert not bool(nan_g['da'].any()) and not bool(nan_g['db'].any())


@pytest.mark.parametrize('act', [None, 'elu'], ids=str)
def test_a_nan_reaches_exactly_the_low_pixels_it_feeds(act):
    shape = (1, 9, 19, 16, 32, act)
    a, b, weight, g, _, _ = B.case(shape)
    places = [(0, 0), (17, 37), (0, 11), (15, 31), (16, 32), (6, 9)]
    many = np.repeat(g, len(places), 0)
    cs = [0, 255, 17, 100, 101, 200]
    for n, ((py, px), c) in enumerate(zip(places, cs)):
        many[n, py, px, c] = np.nan
    rep = lambda t: dev(np.repeat(t, len(places), 0))
    got = {k: v.cpu().numpy() for k, v in run(dev(many), rep(a), rep(b), dev(weight), act).items()}
    uy, ux = B.upsample_matrix(9), B.upsample_matrix(19)
    for n, ((py, px), c) in enumerate(zip(places, cs)):
        fed = (uy[py][:, None] * ux[px][None, :]) != 0
        assert 1 <= fed.sum() <= 4
        for name in ('da', 'db'):
            bad = ~np.isfinite(got[name][n])
            assert np.array_equal(bad, np.broadcast_to(fed[:, :, None], bad.shape)), (py, px, name)      # every k of those pixels, nothing else
        bad = ~np.isfinite(got['g_low'][n])
        want = np.zeros_like(bad)
        want[:, :, c] = fed
        assert np.array_equal(bad, want), (py, px)


def test_offsets_beyond_two_to_the_31_elements():
    """g of 4100 x 2048 x 256 = 2^31 + 2.3e6 elements (8.6 GB of zeros) with impulses at its very end: the last low pixel receives them."""
    h, w, ca, cb = 2050, 1024, 16, 16
    g = torch.zeros(1, 2 * h, 2 * w, 256, device=DEV)
    assert g.numel() > 2 ** 31
    g[0, 2 * h - 1, 2 * w - 1, 255] = 1.0
    g[0, 2 * h - 2, 2 * w - 2, 3] = 16.0
    weight = torch.arange((ca + cb) * 256, device=DEV, dtype=torch.float32).reshape(ca + cb, 256) % 17 - 8
    zeros = lambda c: torch.zeros(1, h, w, c, device=DEV)
    da, db, _ = ops.fuse_upsample2x_bwd(g, zeros(ca), zeros(cb), weight, None)
    dx = torch.cat([da, db], -1)
    want = torch.zeros(2, 2, ca + cb, device=DEV)
    want[1, 1] = weight[:, 255] + 9.0 * weight[:, 3]
    want[1, 0] = want[0, 1] = 3.0 * weight[:, 3]
    want[0, 0] = weight[:, 3]
    assert torch.equal(dx[0, h - 2:, w - 2:], want)
    assert float(dx.abs().sum()) == float(want.abs().sum())                                   # small integers: exact, and nothing elsewhere


def test_two_runs_give_the_same_bits():
    shape = (2, 9, 11, 128, 256, 'elu')
    a, b, weight, g, _, _ = B.case(shape)
    args = [dev(t) for t in (g, a, b, weight)]
    first, again = run(*args, 'elu'), run(*args, 'elu')
    for name in NAMES:
        assert torch.equal(bits(first[name]), bits(again[name])), name


def test_wrapper_checks_its_arguments():
    a, b, weight, g, _, _ = (B.case((1, 3, 17, 128, 256, 'elu')))
    g, a, b, weight = (dev(t) for t in (g, a, b, weight))
    assert [t.shape for t in ops.fuse_upsample2x_bwd(g, a, b, weight, 'identity', need_g_low=True)] == [a.shape, b.shape, (1, 3, 17, 256)]
    with pytest.raises(ValueError):
        ops.fuse_upsample2x_bwd(g, a, b, weight, 'gelu')
    with pytest.raises(ValueError):
        ops.fuse_upsample2x_bwd(g[:, :5], a, b, weight, None)
    with pytest.raises(ValueError):
        ops.fuse_upsample2x_bwd(g, a, b[:, :2], weight, None)
    with pytest.raises(ValueError):
        ops.fuse_upsample2x_bwd(g, a, b, weight[:, :128].contiguous(), None)
    with pytest.raises(ValueError):
        ops.fuse_upsample2x_bwd(g, a, b, weight, None, out=(None, None))
    with pytest.raises(ValueError):
        ops.fuse_upsample2x_bwd(g, a, b, weight, None, out=(torch.empty_like(b), None, None))
    with pytest.raises(ValueError, match='Ca=24'):
        z = torch.zeros(1, 3, 4, 24, device=DEV)
        ops.fuse_upsample2x_bwd(torch.zeros(1, 6, 8, 256, device=DEV), z, z, torch.zeros(48, 256, device=DEV), None)
