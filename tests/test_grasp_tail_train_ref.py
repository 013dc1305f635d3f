"""The closed forms the training kernels of the per-pose read-out are built against (tests/grasp_tail_ref.py, include/mvnerf_hip.h) against
float64 torch.autograd.grad(..., create_graph=True) on the five lines of the tail: every buffer-derived quantity - g_x, the eleven first-order
weight gradients, and the gradients of phi = <t, g_x> with respect to g_s, x and the eleven weights - to a relative L2 of 1e-12, and the
second-order gradients of b1' and b_out exactly zero.  Each of a set of planted wrong terms must break that bar: the comparison can see them.
No GPU."""
import pytest
import torch

from tests import grasp_tail_ref as R

BAR = 1e-12
SHAPES = [(1, 42, True), (5, 7, True), (37, 42, True), (64, 18, True), (70, 1, False)]


def case(m, n5, use_bias):
    ro = R.make_readout(n5, 100 + n5, use_bias=use_bias)
    w = R.weights(ro, torch.float64, 'cpu')
    x, g_s, t = (v.double() for v in R.inputs(m, n5, 7 * m + n5))
    return w, x, g_s, t


def errors(w, x, g_s, t, mutate=None):
    """name -> relative L2 error of the closed form against autograd, for every quantity."""
    s, first, second = R.autograd_reference(x, g_s, t, w)
    fb, sb = R.first_backward(x, g_s, w, mutate=mutate), R.second_backward(x, g_s, t, w, mutate=mutate)
    out = {'g_x': R.rel(fb['g_x'], first['x']), 'out_gs': R.rel(sb['out_gs'], second['g_s']), 'out_x': R.rel(sb['out_x'], second['x'])}
    for n in R.WEIGHTS:
        if w[n] is None:
            continue
        out['d_' + n] = R.rel(fb['grads'][n], first[n])
        if n in ('b1b', 'b_out'):
            assert float(second[n].abs().max()) == 0.0
            out['dd_' + n] = float(sb['grads'][n].abs().max())              # identically zero: the absolute value
        else:
            out['dd_' + n] = R.rel(sb['grads'][n], second[n])
    return out


@pytest.mark.parametrize('m,n5,use_bias', SHAPES)
def test_closed_forms_match_float64_autograd(m, n5, use_bias):
    w, x, g_s, t = case(m, n5, use_bias)
    s, first, _ = R.autograd_reference(x, g_s, t, w)
    assert float(first['x'].norm(dim=1).min()) > 0.0                         # no row wholly behind the final relu
    assert torch.equal(R.tail(x, w), s)
    errs = errors(w, x, g_s, t)
    for name, e in errs.items():
        print(f'M={m} n5={n5} {name}: {e:.3e}')
    assert errs['dd_b1b'] == 0.0 and (not use_bias or errs['dd_b_out'] == 0.0)
    for name, e in errs.items():
        assert e <= BAR, (name, e)


@pytest.mark.parametrize('m,n5,use_bias', SHAPES)
def test_buffers_reproduce_the_gradients(m, n5, use_bias):
    """cot, act, ex, cot2, tan, dex are what the weight gradients are made of: the documented products of the returned buffers give the
    returned gradients (the same expressions, to 1e-14), so a kernel that matches the buffers matches the gradients."""
    w, x, g_s, t = case(m, n5, use_bias)
    fb, sb = R.first_backward(x, g_s, w), R.second_backward(x, g_s, t, w)
    cot, act, ex, cot2, tan, dex = fb['cot'], fb['act'], fb['ex'], sb['cot2'], sb['tan'], sb['dex']
    assert cot.shape == (m, 320) and act.shape == (m, 320) and cot2.shape == (m, 256) and tan.shape == (m, 320)
    assert ex.shape == dex.shape == x.shape and sb['out_gs'].shape == (m,) and sb['out_x'].shape == x.shape
    g_h0, g_x1, g_h1, g_x2 = cot[:, :128], cot[:, 128:192], cot[:, 192:256], cot[:, 256:]
    p_h0, p_x1, p_h1 = cot2[:, :128], cot2[:, 128:192], cot2[:, 192:]
    f, s2 = fb['grads'], sb['grads']
    same = lambda a, b: R.rel(a, b) <= 1e-14                                   # the same expression on a column block of the buffer
    assert same(f['w0'], g_h0.T @ ex) and same(f['w1'], g_x1.T @ act[:, :128]) and same(f['ws'], g_x1.T @ x)
    assert same(f['w0b'], g_h1.T @ act[:, 128:192]) and same(f['w1b'], g_x2.T @ act[:, 192:256])
    assert same(torch.cat([f['b0'], f['b1'], f['b0b'], f['b1b']]), cot.sum(0)) and same(f['w_out'][0], act[:, 256:].sum(0))
    assert same(s2['w0'], g_h0.T @ dex + p_h0.T @ ex) and same(s2['ws'], g_x1.T @ t + p_x1.T @ x)
    assert same(s2['w1'], g_x1.T @ tan[:, :128] + p_x1.T @ act[:, :128])
    assert same(s2['w0b'], g_h1.T @ tan[:, 128:192] + p_h1.T @ act[:, 128:192]) and same(s2['w1b'], g_x2.T @ tan[:, 192:256])
    assert same(torch.cat([s2['b0'], s2['b1'], s2['b0b']]), cot2.sum(0)) and same(s2['w_out'][0], tan[:, 256:].sum(0))


@pytest.mark.parametrize('mutate', R.MUTATIONS)
def test_planted_errors_break_the_bar(mutate):
    w, x, g_s, t = case(37, 42, True)
    errs = errors(w, x, g_s, t, mutate=mutate)
    worst = max(errs, key=errs.get)
    print(f'{mutate}: worst {worst} {errs[worst]:.3e}')
    assert errs[worst] > 1e3 * BAR, (mutate, worst, errs[worst])
