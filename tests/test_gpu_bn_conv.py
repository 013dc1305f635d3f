"""mvnerf_conv3x3_nhwc_ex (bias, act_in, tile statistics; csrc/conv3x3.hip), mvnerf_bn_finalize and mvnerf_bn_apply_nhwc
(csrc/batchnorm.hip) against the float64 references of tests/bn_ref.py.

Bar: e64 <= 8 e32, relative L2 and worst element over the largest magnitude, e32 the float32 torch CPU run of the same case.
Shapes (N, h, w, Ca, Cout) from the kernel's tile constants (16 x 16 pixels, 64 channels): (1,1,1,32,64) one pixel, every tap but the
centre is padding; (2,19,35,64,128) 2 x 3 pixel tiles with 3-pixel last tiles, two channel tiles, two images; (3,33,17,128,128) 1-pixel
last tiles, three images.  The normalisation needs two values per channel (torch's yardstick refuses one), so its first shape is
(1,2,3,32,64).  Then the exact properties: impulse + bias, relu in front of an all-negative source, the statistics of a constant map,
the pixel counts through a map of known mean, in-place apply, amax_out, determinism, and the wrappers' argument checks."""
import numpy as np
import pytest
import torch

from tests import bn_ref as B
from tests import conv3x3_ref as R
from thesis_clip_nerf_amd import ops

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
GUARD = 2


def dev(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def run_guarded(a, packed, cout, act=None, **kw):
    """ops.conv3x3 into a NaN-filled `out` between guard rows; asserts that the guards are untouched.  -> what ops.conv3x3 returns."""
    n, h, w, _ = a.shape
    row = w * cout
    buf = torch.full(((n * h + 2 * GUARD) * row,), float('nan'), dtype=torch.float32, device=DEV)
    out = buf[GUARD * row:-GUARD * row].view(n, h, w, cout)
    got = ops.conv3x3(a, None, packed, cout, act, out=out, **kw)
    torch.cuda.synchronize()
    assert bool(torch.isnan(buf[:GUARD * row]).all() and torch.isnan(buf[-GUARD * row:]).all()), 'wrote outside out'
    assert (got[0] if isinstance(got, tuple) else got).data_ptr() == out.data_ptr()
    return got


_dev = {}


def device_case(shape):
    if shape not in _dev:
        d = B.inputs(shape)
        _dev[shape] = {k: dev(v) for k, v in d.items()} | {'packed': ops.conv3x3_pack(dev(d['wt']))}
    return _dev[shape]


@pytest.mark.parametrize('act_in', B.ACT_INS, ids=str)
@pytest.mark.parametrize('shape', B.SHAPES, ids=str)
def test_bias_and_act_in_against_the_float64_reference(shape, act_in):
    _, ref, e32 = B.conv_case(shape, act_in)
    g = device_case(shape)
    out = run_guarded(g['x'], g['packed'], shape[4], bias=g['bias'], act_in=act_in)
    assert torch.isfinite(out).all(), 'left elements unwritten'
    ok, (e, _) = B.passes(out.cpu().numpy(), ref, e32)
    print(f'{shape} act_in={act_in}: rel L2 {e[0]:.3g} = {e[0] / e32[0]:.2f} x e32, worst {e[1]:.3g} = {e[1] / e32[1]:.2f} x e32')
    assert ok, (e, e32)
    again, stats = run_guarded(g['x'], g['packed'], shape[4], bias=g['bias'], act_in=act_in, stats=True)
    assert torch.equal(out.view(torch.int32), again.view(torch.int32))          # two runs, and the statistics change nothing that is written
    assert torch.isfinite(stats).all()


def test_impulse_with_bias_is_stamp_plus_bias_bit_for_bit():
    h, w, ca, cout = 19, 35, 64, 128
    rng = np.random.default_rng(5)
    wt = rng.integers(-8, 9, (3, 3, ca, cout)).astype(np.float32) / 8
    bias = rng.integers(-16, 17, cout).astype(np.float32) / 4
    places = [(0, 0), (h - 1, w - 1), (15, 15), (16, 16), (15, 31), (16, 32), (9, 20)]
    ks = [int(k) for k in rng.integers(0, ca, len(places))]
    a = np.zeros((len(places), h, w, ca), np.float32)
    want = np.broadcast_to(bias, (len(places), h, w, cout)).copy()
    for i, ((py, px), k) in enumerate(zip(places, ks)):
        a[i, py, px, k] = 1.0
        for dy in range(3):
            for dx in range(3):
                y, x = py + 1 - dy, px + 1 - dx
                if 0 <= y < h and 0 <= x < w:
                    want[i, y, x] = wt[dy, dx, k] + bias
    out = run_guarded(dev(a), ops.conv3x3_pack(dev(wt)), cout, bias=dev(bias))
    assert np.array_equal(out.cpu().numpy(), want)


@pytest.mark.parametrize('act', R.ACTS, ids=str)
def test_relu_in_front_of_an_all_negative_source_leaves_act_of_bias(act):
    shape = B.SHAPES[1]
    g = device_case(shape)
    neg = -g['x'].abs() - 0.25
    out, stats = run_guarded(neg, g['packed'], shape[4], act, bias=g['bias'], act_in='relu', stats=True)
    want = {None: lambda v: v, 'relu': torch.relu, 'elu': torch.nn.functional.elu}[act](g['bias'].double()).float()
    if act == 'elu':                                                            # expm1f on the device against torch's: a rounding apart
        assert torch.allclose(out, want.expand_as(out), rtol=3e-7, atol=0) and bool((out == out[0, 0, 0]).all())
        want = out[0, 0, 0]
    else:
        assert torch.equal(out, want.expand_as(out))
    # a constant map: every tile's mean is the constant and its M2 is zero, exactly
    n, h, w, _, cout = shape
    st = stats.view(cout // 64, n * 2 * 3, 2, 64)
    assert torch.equal(st[:, :, 0], want.view(cout // 64, 1, 64).expand(-1, n * 2 * 3, -1)) and not bool(st[:, :, 1].any())
    mean, rstd = ops.bn_finalize(stats, n, h, w, cout, B.EPS)
    assert torch.equal(mean, want) and torch.equal(rstd, torch.full_like(rstd, float(np.float32(1 / np.sqrt(B.EPS)))))


def test_tile_pixel_counts_through_a_map_of_known_mean():
    """Centre-tap identity weights copy channel co % Ca of the source: the source is the pixel's column index, so every channel's mean is
    (w - 1) / 2 and its variance (w^2 - 1) / 12 - if and only if every tile enters with its real pixels (the counts sum to N h w)."""
    for n, h, w, ca, cout in B.BN_SHAPES:
        wt = np.zeros((3, 3, ca, cout), np.float32)
        wt[1, 1, np.arange(cout) % ca, np.arange(cout)] = 1.0
        ramp = np.broadcast_to(np.arange(w, dtype=np.float32)[None, None, :, None], (n, h, w, ca)).copy()
        out, stats = ops.conv3x3(dev(ramp), None, ops.conv3x3_pack(dev(wt)), cout, None, stats=True)
        assert np.array_equal(out.cpu().numpy(), np.broadcast_to(ramp[..., :1], (n, h, w, cout)))
        mean, rstd = ops.bn_finalize(stats, n, h, w, cout, B.EPS)
        assert torch.equal(mean, torch.full_like(mean, (w - 1) / 2)), (n, h, w)
        assert torch.allclose(rstd, torch.full_like(rstd, float(1 / np.sqrt((w * w - 1) / 12 + B.EPS))), rtol=1e-6, atol=0)


def gpu_pipeline(g, shape, skip, act_in=None, act=None, eps=B.EPS, in_place=True):
    n, h, w, _, cout = shape
    y, stats = run_guarded(g['x'], g['packed'], cout, act, bias=g['bias'], act_in=act_in, stats=True)
    mean, rstd = ops.bn_finalize(stats, n, h, w, cout, eps)
    top = torch.full((1,), 7.0, device=DEV)
    out = ops.bn_apply(y, mean, rstd, g['gamma'], g['beta'], skip=g['skip'] if skip else None, act='relu', out=y if in_place else None,
                       amax_out=top)
    return out, top, mean, rstd


@pytest.mark.parametrize('skip', [False, True], ids=['plain', 'skip'])
@pytest.mark.parametrize('shape', B.BN_SHAPES, ids=str)
def test_convolution_statistics_and_apply_against_the_float64_pipeline(shape, skip):
    d, ref, e32 = B.pipeline_case(shape, skip)
    g = device_case(shape)
    out, top, mean, rstd = gpu_pipeline(g, shape, skip)
    assert torch.isfinite(out).all()
    ok, (e, _) = B.passes(out.cpu().numpy(), ref, e32)
    print(f'{shape} skip={skip}: rel L2 {e[0]:.3g} = {e[0] / e32[0]:.2f} x e32, worst {e[1]:.3g} = {e[1] / e32[1]:.2f} x e32')
    assert ok, (e, e32)
    y64 = B.conv_bias_ref(d['x'], d['wt'], d['bias'])
    assert np.allclose(mean.cpu().numpy(), y64.mean((0, 1, 2)), rtol=1e-5, atol=1e-6)
    assert np.allclose(rstd.cpu().numpy(), 1 / np.sqrt(y64.var((0, 1, 2)) + B.EPS), rtol=1e-5)
    # in place == out of place, amax_out == max |out|, two runs the same bits
    apart, top2, _, _ = gpu_pipeline(g, shape, skip, in_place=False)
    assert torch.equal(out.view(torch.int32), apart.view(torch.int32))
    assert torch.equal(top.view(torch.int32), out.abs().max().reshape(1).view(torch.int32)) and torch.equal(top, top2)


def test_channels_with_a_mean_of_1e3_sigma_meet_the_bar():
    """A bias of +-1e3 x the output's sigma on three channels of four: what a raw fp32 sum of squares cannot survive."""
    shape = B.SHAPES[1]
    d = B.inputs(shape)
    sigma = float(B.conv_bias_ref(d['x'], d['wt'], None).std())
    c = np.arange(shape[4])
    d['bias'] = np.where(c % 4 == 0, d['bias'], 1e3 * sigma * np.where(c % 2 == 0, 1.0, -1.0)).astype(np.float32)
    ref = B.pipeline_ref(d, True)
    e32 = R.errors(B.pipeline_torch(d, torch.float32, True), ref)
    g = {k: dev(v) for k, v in d.items()} | {'packed': device_case(shape)['packed']}
    out, _, _, rstd = gpu_pipeline(g, shape, True)
    ok, (e, _) = B.passes(out.cpu().numpy(), ref, e32)
    print(f'|mean|/sigma = 1e3: rel L2 {e[0]:.3g} = {e[0] / e32[0]:.2f} x e32, worst {e[1]:.3g} = {e[1] / e32[1]:.2f} x e32')
    assert ok, (e, e32)
    assert B.passes(B.restated(d, True), ref, e32)[0]


def test_a_nan_bound_reaches_the_statistics_and_the_output():
    shape = B.BN_SHAPES[0]
    g = device_case(shape)
    bad = g['x'].clone()
    bad[0, 1, 2, 5] = float('nan')
    out, top, mean, _ = gpu_pipeline(dict(g, x=bad), shape, True)
    assert torch.isnan(out).all() and torch.isnan(mean).all() and torch.isnan(top).all()


def test_wrappers_check_their_arguments():
    shape = B.BN_SHAPES[0]
    g = device_case(shape)
    n, h, w, _, cout = shape
    call = lambda **kw: ops.conv3x3(g['x'], None, g['packed'], cout, None, **kw)
    with pytest.raises(ValueError, match='bias'):
        call(bias=g['bias'][:32].contiguous())
    with pytest.raises(ValueError, match='act_in'):
        call(act_in='gelu')
    with pytest.raises(ValueError, match='act_in'):
        call(act_in=3)
    with pytest.raises(ValueError, match='stats'):
        call(stats=torch.zeros(64, device=DEV))
    with pytest.raises(ValueError, match='bias'):
        call(bias=g['bias'].double())
    y, stats = call(bias=g['bias'], stats=True)
    with pytest.raises(ValueError, match='stats'):
        ops.bn_finalize(stats, n, h + 16, w, cout)
    with pytest.raises(ValueError, match='eps'):
        ops.bn_finalize(stats, n, h, w, cout, eps=-1.0)
    mean, rstd = ops.bn_finalize(stats, n, h, w, cout)
    with pytest.raises(ValueError, match='gamma'):
        ops.bn_apply(y, mean, rstd, g['gamma'][:32].contiguous(), g['beta'])
    with pytest.raises(ValueError, match='skip'):
        ops.bn_apply(y, mean, rstd, g['gamma'], g['beta'], skip=g['skip'][:, :1].contiguous())
    with pytest.raises(ValueError, match='act'):
        ops.bn_apply(y, mean, rstd, g['gamma'], g['beta'], act='elu')
