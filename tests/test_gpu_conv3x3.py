"""mvnerf_conv3x3_nhwc (csrc/conv3x3.hip) - the bias-free 'same' 3x3 convolution over [a | b] with activation, per-image channel
multiplier and amax_out in one launch, fp32 grade on the fp16 matrix pipe - against the float64 reference of tests/conv3x3_ref.py.

Bar: the kernel's error against float64 is at most 8 x the error e32 of the float32 yardstick run of the
same case, for the relative L2 and separately for the worst element over the largest magnitude.

Shapes (N, h, w, Ca, Cb, Cout): (1,1,1,32,0,64) every tap but the centre is padding; (2,3,5,32,32,64) smaller than a tile, two sources,
two images; (1,4,4,2048,0,64) K = 18432; and from the kernel's tile constants kCvTile = 16 pixels, kCvCout = 64 channels, kCvChunk = 32:
(3,19,35,32,64,128) = 2 x 3 pixel tiles with 3-pixel last tiles, two channel tiles, three images, and (3,33,17,64,0,128) with 1-pixel
last tiles (a channel tile cannot be partial: Cout % 64 == 0 is the accepted set); the first of them again with a x 1e3 and b x 1e-3.
A tile belongs to one image (the image index is decoded from the block index, pixel tiles fastest), so with N = 3 the block index runs
over image boundaries inside a channel tile; the impulse test puts a stamp on the last pixel of one image and the first of the next.
Then what a fused pass gets wrong without being inaccurate: writes outside `out`, unwritten elements, the exact stamp of an impulse
at corners, edges, tile seams and image boundaries, power-of-two covariance (what the in-kernel scale buys), amax_out, the NaN and zero
rules, and run-to-run determinism."""
import numpy as np
import pytest
import torch

from tests import conv3x3_ref as R
from thesis_clip_nerf_amd import ops

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
GUARD = 2                       # guard rows (of w x Cout elements) in front of and behind `out`

CASES = [(s, 1.0, 1.0) for s in R.SHAPES] + [(R.TILED_TWO, 1e3, 1e-3)]


def dev(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def hwio(wt):
    return ops.conv3x3_pack(dev(wt))


def run_guarded(a, b, packed, cout, act, mul=None, **kw):
    """The call into a NaN-filled `out` between guard rows; asserts that the guards are untouched."""
    n, h, w, _ = a.shape
    row = w * cout
    buf = torch.full(((n * h + 2 * GUARD) * row,), float('nan'), dtype=torch.float32, device=DEV)
    out = buf[GUARD * row:-GUARD * row].view(n, h, w, cout)
    got = ops.conv3x3(a, b, packed, cout, act, mul=mul, out=out, **kw)
    assert got.data_ptr() == out.data_ptr()
    torch.cuda.synchronize()
    assert bool(torch.isnan(buf[:GUARD * row]).all() and torch.isnan(buf[-GUARD * row:]).all()), 'wrote outside out'
    return out


_dev_inputs = {}


def device_inputs(case):
    if case not in _dev_inputs:
        shape, sa, sb = case
        a, b, wt, mul = R.inputs(shape, 0, sa, sb)
        _dev_inputs[case] = (dev(a), dev(b), hwio(wt), dev(mul))
    return _dev_inputs[case]


@pytest.mark.parametrize('with_mul', [False, True], ids=['plain', 'mul'])
@pytest.mark.parametrize('act', R.ACTS, ids=str)
@pytest.mark.parametrize('case', CASES, ids=str)
def test_against_the_float64_reference(case, act, with_mul):
    shape, sa, sb = case
    a, b, wt, mul = R.inputs(shape, 0, sa, sb)
    ref = R.conv_ref(a, b, wt, act, mul if with_mul else None)
    e32_l2, e32_worst = R.e32(shape, act, with_mul, 0, sa, sb)
    da, db, packed, dmul = device_inputs(case)
    out = run_guarded(da, db, packed, shape[5], act, dmul if with_mul else None)
    assert torch.isfinite(out).all(), 'left elements unwritten'
    e_l2, e_worst = R.errors(out.cpu().numpy(), ref)
    print(f'{case} {act} mul={with_mul}: rel L2 {e_l2:.3g} = {e_l2 / e32_l2:.2f} x e32 ({e32_l2:.3g}), '
          f'worst {e_worst:.3g} = {e_worst / e32_worst:.2f} x e32 ({e32_worst:.3g})')
    assert e_l2 <= R.BAR * e32_l2, (e_l2, e32_l2)
    assert e_worst <= R.BAR * e32_worst, (e_worst, e32_worst)


def test_impulse_stamp_is_exact_at_corners_edges_seams_and_image_boundaries():
    """One input channel 1 at one pixel per image, weights small integers / 8: the output is the 3 x 3 stamp of weight rows around that
    pixel (out[py + 1 - dy, px + 1 - dx] = W[dy, dx, k]), cut off at the borders, nothing in any other image - bit for bit.  Tiles are
    16 x 16: seams between rows 15 | 16 and columns 15 | 16, 31 | 32."""
    h, w, ca, cb, cout = 19, 35, 32, 32, 128
    rng = np.random.default_rng(5)
    wt = rng.integers(-8, 9, (3, 3, ca + cb, cout)).astype(np.float32) / 8
    places = [(0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1), (0, 9), (h - 1, 20), (7, 0), (8, w - 1),            # corners, edges
              (15, 15), (16, 16), (15, 16), (16, 15), (15, 31), (16, 32), (3, 31), (3, 32), (15, 5), (16, 5),       # both sides of every seam
              (h - 1, w - 1), (0, 0), (9, 20)]                    # the last pixel of image n, the first of image n + 1; one well inside
    n = len(places)
    ks = [int(k) for k in rng.integers(0, ca + cb, n)]
    ks[0], ks[1], ks[2] = 0, ca + cb - 1, ca
    a = np.zeros((n, h, w, ca), np.float32)
    b = np.zeros((n, h, w, cb), np.float32)
    want = np.zeros((n, h, w, cout), np.float32)
    for i, ((py, px), k) in enumerate(zip(places, ks)):
        (a if k < ca else b)[i, py, px, k if k < ca else k - ca] = 1.0
        for dy in range(3):
            for dx in range(3):
                y, x = py + 1 - dy, px + 1 - dx
                if 0 <= y < h and 0 <= x < w:
                    want[i, y, x] = wt[dy, dx, k]
    out = run_guarded(dev(a), dev(b), hwio(wt), cout, None)
    got = out.cpu().numpy()
    for i, place in enumerate(places):
        assert np.array_equal(got[i].view(np.int32) & 0x7fffffff, want[i].view(np.int32) & 0x7fffffff) and np.array_equal(got[i], want[i]), \
            (place, ks[i])


@pytest.mark.parametrize('act', [None, 'relu'], ids=str)
@pytest.mark.parametrize('power', [40, -40])
@pytest.mark.parametrize('shape', [R.SMALL_TWO, R.TILED_TWO], ids=str)
def test_power_of_two_covariance(shape, power, act):
    """a and b times 2^p (amax recomputed) give the output times 2^p, bit for bit: the scales are derived inside the kernel."""
    da, db, packed, dmul = device_inputs((shape, 1.0, 1.0))
    base = ops.conv3x3(da, db, packed, shape[5], act, mul=dmul)
    f = float(2.0 ** power)
    scaled = run_guarded(da * f, db * f, packed, shape[5], act, dmul)
    assert torch.isfinite(scaled).all() and float(base.abs().max()) > 0
    assert torch.equal((base * f).view(torch.int32), scaled.view(torch.int32))


def test_amax_out_is_the_output_maximum_and_a_loose_amax_in_meets_the_bar():
    case = (R.TILED_TWO, 1.0, 1.0)
    shape = case[0]
    a, b, wt, mul = R.inputs(shape)
    da, db, packed, dmul = device_inputs(case)
    top = torch.full((1,), 7.0, device=DEV)                      # (the wrapper zeroes it)
    out = ops.conv3x3(da, db, packed, shape[5], 'elu', mul=dmul, amax_out=top)
    assert torch.equal(top.view(torch.int32), out.abs().max().reshape(1).view(torch.int32))
    loose = run_guarded(da, db, packed, shape[5], 'elu', dmul, amax_a=ops.absmax(da) * 1.5, amax_b=ops.absmax(db) * 1.5)
    ref = R.conv_ref(a, b, wt, 'elu', mul)
    e32_l2, e32_worst = R.e32(shape, 'elu', True)
    e_l2, e_worst = R.errors(loose.cpu().numpy(), ref)
    print(f'amax x 1.5: rel L2 {e_l2 / e32_l2:.2f} x e32, worst {e_worst / e32_worst:.2f} x e32')
    assert e_l2 <= R.BAR * e32_l2 and e_worst <= R.BAR * e32_worst


def test_absmax_and_the_nan_and_zero_rules():
    shape = R.SMALL_TWO
    da, db, packed, dmul = device_inputs((shape, 1.0, 1.0))
    assert torch.equal(ops.absmax(da).view(torch.int32), da.abs().max().reshape(1).view(torch.int32))
    big = torch.randn(3, 7, 11, 13, device=DEV)
    big[1, 2, 3, 4] = -77.5
    assert float(ops.absmax(big)) == 77.5
    bad = da.clone()
    bad[1, 2, 3, 7] = float('nan')
    assert torch.isnan(ops.absmax(bad)).all()
    top = torch.zeros(1, device=DEV)
    out = run_guarded(bad, db, packed, shape[5], 'relu', dmul, amax_out=top)
    assert torch.isnan(out).all() and torch.isnan(top).all()                   # a loud failure, and it reaches the next launch's amax
    for act in R.ACTS:
        zero = run_guarded(torch.zeros_like(da), torch.zeros_like(db), packed, shape[5], act, dmul, amax_out=top)
        assert bool((zero == 0).all()) and float(top) == 0.0                   # mul * act(0)


def test_two_runs_and_two_packs_give_identical_bits():
    case = (R.TILED_TWO, 1.0, 1.0)
    shape = case[0]
    a, b, wt, mul = R.inputs(shape)
    da, db, packed, dmul = device_inputs(case)
    again = hwio(wt)
    assert again.data_ptr() != packed.data_ptr() and torch.equal(again, packed)
    first = ops.conv3x3(da, db, packed, shape[5], 'elu', mul=dmul)
    second = ops.conv3x3(da, db, again, shape[5], 'elu', mul=dmul)
    assert torch.equal(first.view(torch.int32), second.view(torch.int32))
    single = ops.conv3x3(da[1:2].contiguous(), db[1:2].contiguous(), packed, shape[5], 'elu', mul=dmul[1:2].contiguous(),
                         amax_a=ops.absmax(da), amax_b=ops.absmax(db))
    assert torch.equal(single[0], first[1])                                    # images of a batch do not see each other


def test_wrappers_check_their_arguments():
    da, db, packed, dmul = device_inputs((R.SMALL_TWO, 1.0, 1.0))
    with pytest.raises(ValueError):
        ops.conv3x3(da, db, packed, 64, 'gelu')
    with pytest.raises(ValueError):
        ops.conv3x3(da, db[:, :2], packed, 64, None)
    with pytest.raises(ValueError):
        ops.conv3x3(da, None, packed, 64, None)                                # the stream is the (3,3,64,64) kernel's
    with pytest.raises(ValueError):
        ops.conv3x3(da, db, packed, 128, None)
    with pytest.raises(ValueError):
        ops.conv3x3(da, db, packed, 64, None, mul=dmul[:, :32].contiguous())
    with pytest.raises(ValueError, match='cin=48'):
        ops.conv3x3_pack(torch.zeros(3, 3, 48, 64, device=DEV))
    with pytest.raises(ValueError, match='cout=32'):
        ops.conv3x3_pack(torch.zeros(3, 3, 32, 32, device=DEV))
