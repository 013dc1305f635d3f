"""The read-out's optimiser without a GPU: the host build of csrc/mvnerf_adam.h (tests/cpu_language_adam) bit for bit
against the NumPy restatement of tests/language_adam_ref.py, the restatement against float64 under a bar counted from its roundings,
planted defects against that same bar, and the segment map against ops.language_grad_layout."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from tests import language_adam_ref as A
from thesis_clip_nerf_amd import ops

HERE = os.path.dirname(os.path.abspath(__file__))
F32 = np.float32
STEPS = (1, 2, 10, 1000, 10 ** 6)
N = 3 * 4096


@pytest.fixture(scope='module')
def cpu():
    d = os.path.join(HERE, 'cpu_language_adam')
    subprocess.run(['make', '-C', d], check=True, capture_output=True)
    lib = ctypes.CDLL(os.path.join(d, 'libmvnerf_language_adam_cpu.so'))
    lib.adam_cpu_rate.restype, lib.adam_cpu_rate.argtypes = ctypes.c_float, [ctypes.c_float] * 3 + [ctypes.c_longlong]
    lib.adam_cpu_power.restype, lib.adam_cpu_power.argtypes = ctypes.c_double, [ctypes.c_double, ctypes.c_longlong]
    lib.adam_cpu_update.restype = None
    lib.adam_cpu_update.argtypes = [ctypes.c_void_p] * 4 + [ctypes.c_long] + [ctypes.c_float] * 5
    lib.adam_cpu_head_stack.restype = ctypes.c_long
    lib.adam_cpu_entry.restype = ctypes.c_char_p
    lib.adam_cpu_entry.argtypes = [ctypes.c_int, ctypes.c_int] + [ctypes.c_void_p] * 4
    lib.adam_cpu_segments.restype, lib.adam_cpu_segments.argtypes = None, [ctypes.c_int] + [ctypes.c_void_p] * 3
    return lib


def ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def inputs(seed, n=N):
    """p, g, m, v (float32), in thirds of g: |g| above the clip, ordinary, and |g| <= 1e-7 on moments as small, where eps decides."""
    rng = np.random.default_rng(seed)
    k = n // 3
    sign = lambda size: rng.choice([-1.0, 1.0], size)
    g = np.concatenate([sign(k) * rng.uniform(1.0, 50.0, k), 0.3 * rng.standard_normal(k), sign(n - 2 * k) * rng.uniform(1e-9, 1e-7, n - 2 * k)])
    m = np.concatenate([rng.standard_normal(k), 0.1 * rng.standard_normal(k), 1e-8 * rng.standard_normal(n - 2 * k)])
    v = np.concatenate([rng.uniform(0.0, 2.0, k), rng.uniform(0.0, 0.1, k), rng.uniform(0.0, 1e-14, n - 2 * k)])
    p = 0.5 * rng.standard_normal(n)
    return tuple(a.astype(F32) for a in (p, g, m, v))


def host_update(cpu, p, g, m, v, lr_t, hyper):
    p, m, v = p.copy(), m.copy(), v.copy()
    c = A.f32_constants(hyper)
    cpu.adam_cpu_update(ptr(p), ptr(g), ptr(m), ptr(v), p.size, lr_t, c['beta1'], c['beta2'], c['eps'], c['clip'])
    return p, m, v


@pytest.mark.parametrize('clip', (1.0, 0.0))
@pytest.mark.parametrize('t', STEPS)
def test_host_build_matches_the_numpy_restatement_bit_for_bit(cpu, t, clip):
    hyper = dict(A.HYPER, clip=clip)
    c = A.f32_constants(hyper)
    p, g, m, v = inputs(t)
    g[5], g[N // 3 + 5] = np.nan, np.inf                               # fminf / fmaxf: a NaN gives way to the bound, as in the kernel
    want_p, want_m, want_v, want_rate = A.update32(p, g, m, v, t, **hyper)
    rate = F32(cpu.adam_cpu_rate(c['lr'], c['beta1'], c['beta2'], t))
    assert rate.tobytes() == want_rate.tobytes(), (t, float(rate), float(want_rate))
    for beta in (c['beta1'], c['beta2']):
        assert cpu.adam_cpu_power(float(beta), t) == A.power(float(beta), t)
    got = host_update(cpu, p, g, m, v, rate, hyper)
    for name, a, b in zip('pmv', got, (want_p, want_m, want_v)):
        assert a.dtype == b.dtype and a.tobytes() == b.tobytes(), (name, t)
    if clip > 0:
        assert got[1][5] == c['beta1'] * m[5] + (F32(1) - c['beta1']) * F32(-clip)      # the NaN became -clip, as fmaxf(NaN, -clip) does
    else:
        assert np.isnan(got[0][5]) and np.isnan(got[1][5]) and np.isnan(got[2][5])


def test_rate_is_the_closed_form_and_starts_where_keras_does():
    """Against pow in float64: 1 ulp of float32 and the two roundings' worth of double error; t = 1: sqrt(1 - b2) / (1 - b1) * lr."""
    for t in STEPS + (3, 7, 12345):
        got, want = float(A.rate32(1e-3, 0.9, 0.999, t)), A.rate64(1e-3, 0.9, 0.999, t)
        assert abs(got - want) <= 2.0 ** -24 * want * (1 + 1e-6), t
    assert float(A.rate32(1e-3, 0.9, 0.999, 10 ** 6)) == float(F32(1e-3))


def errors(ref, got):
    return {k: np.abs(np.asarray(got[k], np.float64) - ref[k]) for k in 'pmv'}


def over(err, bar):
    return {k: int((~(err[k] <= bar[k])).sum()) for k in 'pmv'}


@pytest.mark.parametrize('t', STEPS)
def test_restatement_is_inside_the_bar(t):
    """The bar, per element, from the roundings of float32 (u = 2^-24) against exact arithmetic on the same inputs and constants; the
    float64 reference's own error is 2^-29 of that.  With a = b1 m, b = (1 - b1) g_c and M = |a| + |b| (M stands in for |m'|: a and b may
    cancel, their rounding errors do not):
      m' = fl(fl(a) + fl(fl(1 - b1) g_c))        1 rounding on a, 2 on b, 1 on the sum <= M            |dm| <= 3 u M       bar 4 u M
      v' = fl(fl(b2 v) + fl(fl(fl(1 - b2) g_c) g_c))   1 + 3 + 1, every term >= 0                        |dv| <= 4 u v'      bar 5 u v'
      s  = fl(sqrt(v'))                          half of v's 4 u, + 1                                   3 u s
      d  = fl(s + eps)                           s <= d                                                 4 u d
      n  = fl(lr_t m')                           lr_t rounded to float32 (1), m' (3 u M), the product (1)   5 u lr_t M
      q  = fl(n / d)                             5 + 4 + 1                                              10 u lr_t M / d
      p' = fl(p - q)                             + u |p - q| <= u (|p| + lr_t M / d)                    u (|p| + 11 lr_t M / d)
    bar for p': u (|p| + 12 lr_t M / d): one rounding of slack each for the terms of second order; every bar + a few 2^-149 for results
    in the subnormal range.  lr_t, M and d are the float64 reference's."""
    p, g, m, v = inputs(100 + t % 97)
    ref = A.update64(p, g, m, v, t, **A.HYPER)
    got = dict(zip('pmv', A.update32(p, g, m, v, t, **A.HYPER)[:3]))
    err, bar = errors(ref, got), A.bars(ref)
    for k in 'pmv':
        print(f't={t} {k}: worst |f32 - f64| / bar = {float((err[k] / bar[k]).max()):.3f}')
    assert over(err, bar) == dict(p=0, m=0, v=0)
    third = N // 3
    assert (np.abs(g[:third]) > 1.0).all() and (np.abs(g[2 * third:]) <= 1e-7).all()
    assert (np.sqrt(ref['v'][2 * third:]) < 10 * 1e-7).all()             # the third where eps decides the denominator


@pytest.mark.parametrize('defect', A.DEFECTS)
def test_planted_defects_exceed_the_bar(defect):
    """At the second update (t = 2: both bias corrections far from 1) every misreading of the formula leaves the bar somewhere."""
    t = 2
    p, g, m, v = inputs(7)
    ref = A.update64(p, g, m, v, t, **A.HYPER)
    bar = A.bars(ref)
    good = over(errors(ref, dict(zip('pmv', A.update32(p, g, m, v, t, **A.HYPER)[:3]))), bar)
    assert good == dict(p=0, m=0, v=0)
    bad = over(errors(ref, dict(zip('pmv', A.update32(p, g, m, v, t, **A.HYPER, defect=defect)[:3]))), bar)
    print(defect, bad)
    assert bad['p'] > 0, defect
    third = N // 3
    if defect in ('torch_eps', 'eps_under_root'):                       # seen where eps decides
        e = errors(ref, dict(zip('pmv', A.update32(p, g, m, v, t, **A.HYPER, defect=defect)[:3])))
        assert (~(e['p'][2 * third:] <= bar['p'][2 * third:])).any()
    if defect in ('clip_after_moments', 'unclipped_moments'):
        assert bad['m'] > 0 and bad['v'] > 0


@pytest.mark.parametrize('n5', (1, 7))
@pytest.mark.parametrize('defect', (None,) + A.LAYOUT_DEFECTS)
def test_whole_update_through_the_flat_layout(n5, defect):
    """21 variables, flat moments: the restated step is inside the bar for every variable and for the stacked head images; the tail_w[]
    order used as the flat order, or a skipped head mirror, is not."""
    variables = A.random_variables(n5, 11 + n5)
    total = A.layout(n5)[1]
    rng = np.random.default_rng(n5)
    grads = (0.5 * rng.standard_normal(total)).astype(F32)
    m, v = (0.05 * rng.standard_normal(total)).astype(F32), rng.uniform(0.0, 0.05, total).astype(F32)
    ref_vars, ref_m, ref_v, bar = A.step64(variables, grads, m, v, 4, n5)
    new, m2, v2, image, counter = A.step32(variables, grads, m, v, 4, n5, defect=defect)
    assert counter == 5
    bad = {k: int((~(np.abs(new[k].astype(np.float64) - ref_vars[k]) <= bar['p'][k])).sum()) for k in new}
    bad['image'] = sum(int((~(np.abs(img.astype(np.float64) - ref_vars[k]) <= bar['p'][k])).sum()) for img, k in zip(image, ('w4', 'b4')))
    assert int((~(np.abs(m2 - ref_m) <= bar['m'])).sum()) == 0 and int((~(np.abs(v2 - ref_v) <= bar['v'])).sum()) == 0
    if defect is None:
        assert not any(bad.values()), bad
    elif defect == 'tail_order':
        assert bad['w1b'] > 0 and bad['b0b'] > 0 and bad['w0b'] == 0 and bad['image'] == 0, bad
    else:
        assert bad['image'] > 0 and all(n == 0 for k, n in bad.items() if k != 'image'), bad


@pytest.mark.parametrize('n5', (1, 7, 42))
def test_segment_map_is_the_gradient_layout(cpu, n5):
    layout, total = ops.language_grad_layout(n5)
    assert cpu.adam_cpu_entries() == len(layout) == 15 and cpu.adam_cpu_segment_count() == 21
    assert cpu.adam_cpu_head_stack() == 4 * 64 * 128 + 4 * 64
    tail_index = {name: i for i, name in enumerate(A.TAIL_ORDER)}
    head_var = {'w4': -1, 'b4': -2, 'wc': -3, 'bc': -4}
    expect = []                                                          # (begin, var, part) of the 21 variables
    for e, (name, (offset, shape)) in enumerate(layout.items()):
        off, floats, var, parts = (ctypes.c_long(), ctypes.c_long(), ctypes.c_int(), ctypes.c_int())
        got = cpu.adam_cpu_entry(n5, e, ctypes.byref(off), ctypes.byref(floats), ctypes.byref(var), ctypes.byref(parts))
        assert got.decode() == name and off.value == offset and floats.value == int(np.prod(shape)), name
        assert var.value == (head_var[name] if name in head_var else tail_index[name]), name
        assert parts.value == (4 if name in ('w4', 'b4') else 1)
        each = floats.value // parts.value
        expect += [(offset + k * each, var.value, k) for k in range(parts.value)]
    begin, var, part = np.zeros(22, np.int64), np.zeros(21, np.int32), np.zeros(21, np.int32)
    cpu.adam_cpu_segments(n5, ptr(begin), ptr(var), ptr(part))
    assert [(int(b), int(x), int(k)) for b, x, k in zip(begin[:21], var, part)] == expect
    assert begin[21] == total == ops._lib.lib().mvnerf_language_grad_floats(n5) and total % 2 == 1
    assert (np.diff(begin) > 0).all()
    # the flat order is not the order of tail_w[]: block_1's weights come before its biases
    assert [v for v in var if v >= 0] == [0, 1, 2, 3, 4, 5, 7, 6, 8, 9, 10]
