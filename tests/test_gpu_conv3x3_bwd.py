"""The backward of the biased 3x3 convolution on the GPU (csrc/conv3x3_bwd.hip, ops.conv3x3_wgrad, ops.conv3x3_pack_transposed,
encoders.Conv3x3BiasFunction) against the float64 references of tests/conv3x3_bwd_ref.py.

Bar: the error against float64 is at most 8 x the error e32 of the float32 torch CPU autograd run of the same case, for the relative L2
and separately for the worst element over the largest magnitude.  Shapes (N, h, w, Cin, Cout): smaller than a tile with two images; 2 x 3
tiles with 3-pixel last tiles and two channel tiles both ways; 1-pixel last tiles with four input chunks; 16 pixels of 256 channels;
and, from the slab constant, 45 tiles = two full slabs and a ragged third.  Then what such a pass gets wrong without being inaccurate:
writes outside its buffers, a dependence on what the workspace held (three fills), exact integer sums, the exact place of an impulse at
corners, edges, tile seams and image boundaries, power-of-two covariance, the relu / zero / NaN rules."""
import numpy as np
import pytest
import torch

from tests import conv3x3_bwd_ref as B
from tests import conv3x3_ref as R
from thesis_clip_nerf_amd import encoders as E
from thesis_clip_nerf_amd import ops

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
GUARD = 64                                          # guard floats around every buffer
GUARD_WORD = 0x7FA5A5A5                             # (as int32)
FILLS = [0x00000000, 0x7FC00000, 0x3F800000]        # the fill protocol: zeros, NaN, ones


def dev(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def test_the_slab_constant_is_the_librarys():
    from thesis_clip_nerf_amd import _lib
    assert ops.CONV3X3_WGRAD_SLAB_PIXELS == _lib.lib().mvnerf_conv3x3_wgrad_slab_pixels() == B.SLAB_PIXELS


def wgrad_filled(x, g, act_in=None, want_bias=True, **kw):
    """ops.conv3x3_wgrad three times, outputs and workspace between guard words and filled with each of FILLS before the call: asserts
    that the guards keep their word and that the three results are the same bits; -> (dw, dbias) arrays."""
    n, h, w, cin = x.shape
    cout = g.shape[3]
    nw, nws = 9 * cin * cout, ops.conv3x3_wgrad_workspace_bytes(n, h, w, cin, cout) // 4
    sizes = [nw, cout, nws]
    buf = torch.empty(sum(sizes) + 4 * GUARD, dtype=torch.int32, device=DEV)
    views, guards, at = [], [], 0
    for size in sizes:
        guards.append(buf[at:at + GUARD])
        views.append(buf[at + GUARD:at + GUARD + size])
        at += GUARD + size
    guards.append(buf[at:at + GUARD])
    results = []
    for fill in FILLS:
        buf.fill_(GUARD_WORD)
        for v in views:
            v.fill_(fill)
        dw, db = views[0].view(torch.float32).view(3, 3, cin, cout), views[1].view(torch.float32)
        got = ops.conv3x3_wgrad(x, g, act_in, want_bias=want_bias, workspace=views[2].view(torch.uint8), out=(dw, db) if want_bias else dw, **kw)
        torch.cuda.synchronize()
        assert (got[0] if want_bias else got).data_ptr() == dw.data_ptr()
        assert all(bool((q == GUARD_WORD).all()) for q in guards), 'wrote outside its buffers'
        if not want_bias:
            assert bool((views[1] == fill).all()), 'dbias written without want_bias'
        results.append((views[0].cpu().numpy().copy(), views[1].cpu().numpy().copy()))
    for r in results[1:]:
        assert np.array_equal(r[0], results[0][0]) and (not want_bias or np.array_equal(r[1], results[0][1])), 'depends on what the buffers held'
    return results[0][0].view(np.float32).reshape(3, 3, cin, cout), results[0][1].view(np.float32)


def check_bar(name, got, ref, yard):
    ok, ratios = B.within_bar(got, ref, yard)
    print(f'{name}: {ratios[0]:.2f} / {ratios[1]:.2f} x e32 ({yard[0]:.3g}, {yard[1]:.3g})')
    assert ok, (name, ratios, yard)


@pytest.mark.parametrize('act_in', B.ACTS, ids=str)
@pytest.mark.parametrize('shape', B.GPU_SHAPES, ids=str)
def test_weight_and_bias_gradient_against_the_float64_reference(shape, act_in):
    x, g, wt, bias = B.case(shape)
    yard = B.e32(shape, act_in)
    dw, db = wgrad_filled(dev(x), dev(g), act_in)
    assert np.isfinite(dw).all() and np.isfinite(db).all()
    check_bar(f'{shape} {act_in} dw', dw, B.dw_ref(x, g, act_in), yard['dw'])
    check_bar(f'{shape} {act_in} dbias', db, B.dbias_ref(g), yard['dbias'])


def test_half_zero_and_tiny_gradients_stay_inside_the_bar():
    for shape, kw in (((3, 33, 17, 64, 64), dict(mask_g=True)), ((1, 16, 16, 32, 64), dict(scale_g=1e-6))):
        x, g, wt, bias = B.case(shape, **kw)
        dw, db = wgrad_filled(dev(x), dev(g), 'relu')
        yard = B.e32(shape, 'relu', **kw)
        check_bar(f'{shape} {kw} dw', dw, B.dw_ref(x, g, 'relu'), yard['dw'])
        check_bar(f'{shape} {kw} dbias', db, B.dbias_ref(g), yard['dbias'])


def int_ref(x, g):
    xp = np.pad(x.astype(np.int64), ((0, 0), (1, 1), (1, 1), (0, 0)))
    n, h, w, cin = x.shape
    dw = np.zeros((3, 3, cin, g.shape[3]), np.int64)
    for dy in range(3):
        for dx in range(3):
            dw[dy, dx] = np.einsum('nijc,nijo->co', xp[:, dy:dy + h, dx:dx + w], g.astype(np.int64))
    return dw.astype(np.float32), g.astype(np.int64).sum((0, 1, 2)).astype(np.float32)


@pytest.mark.parametrize('shape', [(1, 1, 1, 32, 64), (1, 2, 3, 32, 64), (2, 17, 33, 32, 64)], ids=str)
def test_small_integers_are_summed_exactly(shape):
    """|x|, |g| <= 8: every piece, product and partial sum is an integer below 2^24 - the result is the integer sum, bit for bit.  The
    last shape crosses a tile seam both ways."""
    n, h, w, cin, cout = shape
    rng = np.random.default_rng(3)
    x = rng.integers(-8, 9, (n, h, w, cin)).astype(np.float32)
    g = rng.integers(-8, 9, (n, h, w, cout)).astype(np.float32)
    want_dw, want_db = int_ref(x, g)
    dw, db = wgrad_filled(dev(x), dev(g))
    assert np.array_equal(dw, want_dw) and np.array_equal(db, want_db)
    for k in (7, -5):                               # x -> 2^k x scales dw by 2^k bit for bit (the scale follows the amax)
        dwk, dbk = wgrad_filled(dev(np.ldexp(x, k)), dev(g))
        assert np.array_equal(dwk, np.ldexp(want_dw, k)) and np.array_equal(dbk, want_db)
    # relu in front of an all-negative x: no weight gradient, the bias gradient untouched
    dwn, dbn = wgrad_filled(dev(-np.abs(x) - 1), dev(g), 'relu')
    assert not dwn.any() and np.array_equal(dbn, want_db)


def test_random_values_scale_by_powers_of_two_bit_for_bit():
    x, g, wt, bias = B.case(B.TILED)
    dw, db = wgrad_filled(dev(x), dev(g), 'relu')
    dwk, dbk = wgrad_filled(dev(np.ldexp(x, 9)), dev(np.ldexp(g, -13)), 'relu')
    assert np.array_equal(dwk, np.ldexp(dw, -4)) and np.array_equal(dbk, np.ldexp(db, -13))


def test_impulses_land_on_exactly_one_tap_or_nowhere():
    """x is 1 at one (pixel P, channel ci) and g is 1 at one (pixel Q, channel co) per image: dw[dy, dx, ci, co] = 1 where
    P = Q + (dy - 1, dx - 1) and nothing else, bit for bit.  Tiles are 16 x 16; each image has its own (ci, co), so an image that saw its
    neighbour would show."""
    h, w, cin, cout = 19, 35, 32, 64
    pairs = [((0, 0), (0, 0)), ((0, 0), (1, 1)), ((1, 1), (0, 0)), ((0, w - 1), (1, w - 2)), ((h - 1, 0), (h - 2, 1)),       # corners
             ((h - 1, w - 1), (h - 1, w - 1)), ((h - 1, w - 1), (h - 2, w - 2)), ((0, 9), (0, 10)), ((7, 0), (8, 0)),        # edges
             ((15, 15), (16, 16)), ((16, 16), (15, 15)), ((15, 16), (16, 15)), ((16, 31), (15, 32)), ((3, 32), (3, 31)),     # across the seams
             ((7, 5), (8, 5)), ((8, 20), (7, 21)),                                                                          # across the stage seam
             ((0, 0), (h - 1, w - 1)), ((5, 5), (5, 8)), ((h - 1, 3), (0, 3)), ((4, w - 1), (5, 0))]                         # too far apart: nothing
    n = len(pairs)
    x = np.zeros((n, h, w, cin), np.float32)
    g = np.zeros((n, h, w, cout), np.float32)
    want = np.zeros((3, 3, cin, cout), np.float32)
    for i, (p, q) in enumerate(pairs):
        ci, co = i, 2 * i + 1
        x[i, p[0], p[1], ci] = 1.0
        g[i, q[0], q[1], co] = 1.0
        dy, dx = p[0] - q[0] + 1, p[1] - q[1] + 1
        if 0 <= dy < 3 and 0 <= dx < 3:
            want[dy, dx, ci, co] = 1.0
    assert want.sum() == n - 4
    dw, db = wgrad_filled(dev(x), dev(g))
    assert np.array_equal(dw, want)
    # the last pixel of one image against the first of the next, same channels: nothing may cross
    x2, g2 = np.zeros((2, h, w, cin), np.float32), np.zeros((2, h, w, cout), np.float32)
    x2[0, h - 1, w - 1, 0] = 1.0
    g2[1, 0, 0, 0] = 1.0
    dw2, _ = wgrad_filled(dev(x2), dev(g2))
    assert not dw2.any()


def test_the_amax_rules():
    shape = B.TILED
    x, g, wt, bias = B.case(shape)
    dx_, dg_ = dev(x), dev(g)
    one = lambda v: torch.tensor([v], dtype=torch.float32, device=DEV)
    dw, db = wgrad_filled(dx_, dg_, amax_x=one(0.0))
    assert not dw.any() and np.array_equal(db, wgrad_filled(dx_, dg_)[1])
    dw, db = wgrad_filled(dx_, dg_, amax_g=one(0.0))
    assert not dw.any() and not db.any()
    for kw in (dict(amax_x=one(float('nan'))), dict(amax_g=one(float('inf')))):
        dw, db = wgrad_filled(dx_, dg_, **kw)
        assert np.isnan(dw).all() and np.isnan(db).all()
    # a loose bound (x 1000 on both) costs bits of the pieces, not the grade
    dw, db = wgrad_filled(dx_, dg_, 'elu', amax_x=one(1000 * float(np.abs(x).max())), amax_g=one(1000 * float(np.abs(g).max())))
    yard = B.e32(shape, 'elu')
    check_bar('loose dw', dw, B.dw_ref(x, g, 'elu'), yard['dw'])
    check_bar('loose dbias', db, B.dbias_ref(g), yard['dbias'])


def test_argument_checks_raise_before_any_launch():
    x, g = torch.zeros((1, 4, 4, 32), device=DEV), torch.zeros((1, 4, 4, 64), device=DEV)
    need = ops.conv3x3_wgrad_workspace_bytes(1, 4, 4, 32, 64)
    ws = torch.empty(need + 16, dtype=torch.uint8, device=DEV)
    bad = [dict(x=x[0]), dict(g=g[:, :3]), dict(x=torch.zeros((1, 4, 4, 48), device=DEV)), dict(g=torch.zeros((1, 4, 4, 32), device=DEV)),
           dict(act_in=3), dict(act_in=-1), dict(act_in='gelu'), dict(workspace=ws[:need - 16]), dict(workspace=ws[4:need + 4]),
           dict(workspace=ws.view(torch.float32)[:need // 4]), dict(out=torch.zeros((3, 3, 64, 32), device=DEV)),
           dict(want_bias=True, out=(torch.zeros((3, 3, 32, 64), device=DEV), torch.zeros(32, device=DEV))), dict(x=x.cpu()), dict(x=x.double())]
    for kw in bad:
        args = dict(x=x, g=g)
        args.update(kw)
        with pytest.raises(ValueError):
            ops.conv3x3_wgrad(**args)
    with pytest.raises(ValueError):
        ops.conv3x3_pack_transposed(torch.zeros((3, 3, 32, 64), device=DEV))          # the transposed kernel has 32 outputs
    with pytest.raises(ValueError):
        ops.conv3x3_wgrad_workspace_bytes(1, 0, 4, 32, 64)


# ---- the data gradient: the forward kernel on the flipped, transposed pack ------------------------------------------------------------------
DGRAD_SHAPES = [B.TILED, B.WIDE_IN, B.DEEP]


@pytest.mark.parametrize('shape', DGRAD_SHAPES, ids=str)
def test_data_gradient_through_the_transposed_pack(shape):
    x, g, wt, bias = B.case(shape)
    packed_t = ops.conv3x3_pack_transposed(dev(wt))
    raw = ops.conv3x3(dev(g), None, packed_t, shape[3], 0)
    for act_in in B.ACTS:
        got = E.conv3x3_act_grad(raw.permute(0, 3, 1, 2), dev(x).permute(0, 3, 1, 2), act_in).permute(0, 2, 3, 1)
        check_bar(f'{shape} {act_in} dx', got.cpu().numpy(), B.dx_ref(x, g, wt, act_in), B.e32(shape, act_in)['dx'])


def test_data_gradient_of_an_impulse_is_the_flipped_stamp():
    """g is 1 at one (pixel, co) per image, weights small integers / 8: dx[py + dy - 1, px + dx - 1, ci] = W[dy, dx, ci, co], cut off at
    the borders - bit for bit (the forward's stamp is out[py + 1 - dy, ..]: this one is its mirror image)."""
    h, w, cin, cout = 19, 35, 64, 64
    rng = np.random.default_rng(6)
    wt = rng.integers(-8, 9, (3, 3, cin, cout)).astype(np.float32) / 8
    places = [(0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1), (15, 15), (16, 16), (15, 32), (9, 20)]
    g = np.zeros((len(places), h, w, cout), np.float32)
    want = np.zeros((len(places), h, w, cin), np.float32)
    for i, (py, px) in enumerate(places):
        co = int(rng.integers(0, cout))
        g[i, py, px, co] = 1.0
        for dy in range(3):
            for dx in range(3):
                y, xx = py + dy - 1, px + dx - 1
                if 0 <= y < h and 0 <= xx < w:
                    want[i, y, xx] = wt[dy, dx, :, co]
    got = ops.conv3x3(dev(g), None, ops.conv3x3_pack_transposed(dev(wt)), cin, 0).cpu().numpy()
    assert np.array_equal(got, want)


# ---- the autograd Function --------------------------------------------------------------------------------------------------------------------
def make_conv(wt, bias):
    conv = E.SameConv2d(wt.shape[2], wt.shape[3], 3, bias=bias is not None).to(DEV)
    E.load_conv(conv, wt, bias)
    return conv


@pytest.fixture()
def calls(monkeypatch):
    seen = []
    for name in ('conv3x3', 'conv3x3_wgrad', 'conv3x3_pack', 'absmax'):
        real = getattr(ops, name)
        monkeypatch.setattr(ops, name, lambda *a, _real=real, _name=name, **kw: (seen.append(_name), _real(*a, **kw))[1])
    return seen


@pytest.mark.parametrize('act_in', B.ACTS, ids=str)
def test_function_gradients_against_float64(act_in):
    shape = B.TILED
    x, g, wt, bias = B.case(shape)
    conv = make_conv(wt, bias)
    xt = dev(x).permute(0, 3, 1, 2).requires_grad_(True)
    out, top = E.conv3x3_bias(conv, xt, act_in, True, None, True)
    ref_out = R.conv_ref(R.activation(x.astype(np.float64), act_in), None, wt) + bias.astype(np.float64)
    assert R.rel_l2(out.detach().permute(0, 2, 3, 1).cpu().numpy(), ref_out) < 1e-6 and float(top) == float(out.detach().abs().max())
    out.backward(dev(g).permute(0, 3, 1, 2))
    yard = B.e32(shape, act_in)
    check_bar('x.grad', xt.grad.permute(0, 2, 3, 1).cpu().numpy(), B.dx_ref(x, g, wt, act_in), yard['dx'])
    check_bar('weight.grad', conv.weight.grad.permute(2, 3, 1, 0).cpu().numpy(), B.dw_ref(x, g, act_in), yard['dw'])
    check_bar('bias.grad', conv.bias.grad.cpu().numpy(), B.dbias_ref(g), yard['dbias'])


def test_function_skips_the_data_gradient_of_an_input_that_needs_none(calls):
    x, g, wt, bias = B.case(B.TILED)
    conv = make_conv(wt, bias)
    for needs in (True, False):
        xt = dev(x).permute(0, 3, 1, 2).requires_grad_(needs)
        out, _ = E.conv3x3_bias(conv, xt, 'relu', 'auto', None, True)
        del calls[:]
        out.backward(dev(g).permute(0, 3, 1, 2))
        assert calls.count('conv3x3_wgrad') == 1 and calls.count('conv3x3') == int(needs), calls
        assert (xt.grad is not None) == needs


def test_function_without_a_bias_and_with_96_inputs_takes_the_torch_data_gradient(calls):
    """96 -> 256 (the second `conv_decode`): the forward and the weight gradient are HIP, the data gradient is torch's."""
    shape = (3, 9, 11, 96, 256)
    x, g, wt, bias = B.case(shape)
    conv = make_conv(wt, None)
    assert E.conv3x3_fusable(conv, 96, bias=True) and not E.conv3x3_dgrad_fusable(conv)
    xt = dev(x).permute(0, 3, 1, 2).requires_grad_(True)
    out, _ = E.conv3x3_bias(conv, xt, None, 'auto', None, True)
    assert calls.count('conv3x3') == 1
    del calls[:]
    out.backward(dev(g).permute(0, 3, 1, 2))
    assert calls.count('conv3x3_wgrad') == 1 and calls.count('conv3x3') == 0, calls
    yard = B.e32(shape, None)
    check_bar('weight.grad', conv.weight.grad.permute(2, 3, 1, 0).cpu().numpy(), B.dw_ref(x, g, None), yard['dw'])
    assert R.rel_l2(xt.grad.permute(0, 2, 3, 1).cpu().numpy(), B.dx_ref(x, g, wt, None)) < 1e-5


def test_the_transposed_pack_follows_the_parameter():
    x, g, wt, bias = B.case(B.DEEP)
    conv = make_conv(wt, bias)
    first = E._packed_conv3x3_t(conv)
    assert E._packed_conv3x3_t(conv) is first
    with torch.no_grad():
        conv.weight.mul_(2.0)
    second = E._packed_conv3x3_t(conv)
    assert second is not first and not torch.equal(second, first)
    E.load_conv(conv, wt, bias)
    assert torch.equal(E._packed_conv3x3_t(conv), first)
