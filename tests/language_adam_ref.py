"""References of the read-out's optimiser (csrc/mvnerf_adam.h, csrc/language_opt.hip): optimize() = clip-by-value, then tf.keras Adam,

    g_c = clip(g, -c, c);  m' = b1 m + (1 - b1) g_c;  v' = b2 v + (1 - b2) g_c^2;  p' = p - lr_t m' / (sqrt(v') + eps),
    lr_t = lr sqrt(1 - b2^t) / (1 - b1^t),  t = completed updates + 1.

`update64` is that formula in float64 (`**` for the powers) on the float32 constants the kernel is given.  `update32` restates the kernel
operation for operation in NumPy float32, one rounding each, with `rate32` forming lr_t in double from b^t by square-and-multiply (lowest
bit first) - the bits csrc/mvnerf_adam.h must give.  `defect=` plants one wrong reading of the formula or of the layout.  `bars` gives the
elementwise bound on |float32 restatement - float64| that tests/test_language_adam_cpu.py derives.

The whole update acts on the 21 variables through the flat layout of the gradient (`ops.language_grad_layout`): `flat_names` lists its
entries, `to_flat` / `from_flat` move a dict of variables in and out of it.
"""
import numpy as np

F32 = np.float32
U = 2.0 ** -24                                                     # unit round-off of float32
TINY = 2.0 ** -149                                                 # its smallest subnormal
HYPER = dict(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-7, clip=1.0)  # train_language.py:65-67 with Keras's defaults, optimize()'s bound
DEFECTS = ('torch_eps', 'eps_under_root', 'clip_after_moments', 'unclipped_moments', 'no_bias_correction', 't_not_t_plus_1', 'betas_swapped',
           'v_with_g')
LAYOUT_DEFECTS = ('tail_order', 'no_mirror')
TAIL_ORDER = ('w0', 'b0', 'w1', 'b1', 'ws', 'w0b', 'b0b', 'w1b', 'b1b', 'w_out', 'b_out')     # mvnerf_language_call.tail_w[]


def f32_constants(hyper):
    return {k: F32(v) for k, v in hyper.items()}


# ---- the rate ---------------------------------------------------------------------------------------------------------------------------
def power(beta, t):
    """beta ** t for a Python float and t >= 0 by square-and-multiply, lowest bit of t first: r = the product of beta^(2^k) over set bits."""
    r, s, t = 1.0, float(beta), int(t)
    while t > 0:
        if t & 1:
            r = r * s
        s = s * s
        t >>= 1
    return r


def rate32(lr, beta1, beta2, t):
    """lr_t as csrc/mvnerf_adam.h::adam_rate forms it: doubles throughout (of the float32 constants), one rounding to float32."""
    with np.errstate(all='ignore'):
        up = np.sqrt(np.float64(1.0) - np.float64(power(float(F32(beta2)), t)))
        down = np.float64(1.0) - np.float64(power(float(F32(beta1)), t))
        return F32(np.float64(float(F32(lr))) * up / down)


def rate64(lr, beta1, beta2, t):
    b1, b2 = float(F32(beta1)), float(F32(beta2))
    return float(F32(lr)) * np.sqrt(1.0 - b2 ** t) / (1.0 - b1 ** t)


# ---- one array of elements --------------------------------------------------------------------------------------------------------------
def update64(p, g, m, v, t, lr, beta1, beta2, eps, clip):
    """float64, from the formula -> dict p, m, v (new values) and lr_t, M = |b1 m| + |(1 - b1) g_c|, d = sqrt(v') + eps for `bars`."""
    c = f32_constants(dict(lr=lr, beta1=beta1, beta2=beta2, eps=eps, clip=clip))
    b1, b2, e, cl = (float(c[k]) for k in ('beta1', 'beta2', 'eps', 'clip'))
    p, g, m, v = (np.asarray(a, np.float64) for a in (p, g, m, v))
    gc = np.clip(g, -cl, cl) if cl > 0 else g
    m2 = b1 * m + (1.0 - b1) * gc
    v2 = b2 * v + (1.0 - b2) * gc * gc
    lr_t = rate64(lr, beta1, beta2, t)
    d = np.sqrt(v2) + e
    return dict(p=p - lr_t * m2 / d, m=m2, v=v2, lr_t=lr_t, M=np.abs(b1 * m) + np.abs((1.0 - b1) * gc), d=d, p0=np.abs(p))


def bars(ref):
    """Elementwise bounds on |float32 - float64| for m', v', p' (tests/test_language_adam_cpu.py::test_restatement_is_inside_the_bar has
    the count of roundings they come from)."""
    q = ref['lr_t'] * ref['M'] / ref['d']
    return dict(m=4 * U * ref['M'] + 4 * TINY, v=5 * U * ref['v'] + 5 * TINY, p=U * (ref['p0'] + 12 * q) + 12 * TINY)


def update32(p, g, m, v, t, lr, beta1, beta2, eps, clip, defect=None, lr_t=None):
    """The kernel's arithmetic on float32 arrays, one NumPy operation per rounding -> (p', m', v', lr_t).  defect: one of DEFECTS."""
    assert defect is None or defect in DEFECTS, defect
    c = f32_constants(dict(lr=lr, beta1=beta1, beta2=beta2, eps=eps, clip=clip))
    lr, b1, b2, e, cl = (c[k] for k in ('lr', 'beta1', 'beta2', 'eps', 'clip'))
    if defect == 'betas_swapped':
        b1, b2 = b2, b1
    p, g, m, v = (np.asarray(a, F32) for a in (p, g, m, v))
    if lr_t is None:
        lr_t = lr if defect == 'no_bias_correction' else rate32(lr, b1, b2, t - 1 if defect == 't_not_t_plus_1' else t)
    lr_t = F32(lr_t)
    one = F32(1.0)
    clipped = lambda x: np.fmin(np.fmax(x, -cl), cl) if cl > 0 else x            # fminf(fmaxf(.)): a NaN gives way to the bound
    with np.errstate(all='ignore'):
        gm = g if defect in ('clip_after_moments', 'unclipped_moments') else clipped(g)
        m2 = b1 * m + (one - b1) * gm
        second = (one - b2) * gm
        if defect != 'v_with_g':
            second = second * gm
        v2 = b2 * v + second
        m_used = clipped(m2) if defect == 'clip_after_moments' else m2
        if defect == 'torch_eps':        # torch.optim.Adam: step lr / (1 - b1^t), denominator sqrt(v) / sqrt(1 - b2^t) + eps
            bc1 = F32(1.0 - power(float(b1), t))
            bc2s = F32(np.sqrt(1.0 - power(float(b2), t)))
            p2 = p - (lr / bc1) * m_used / (np.sqrt(v2) / bc2s + e)
        elif defect == 'eps_under_root':
            p2 = p - lr_t * m_used / np.sqrt(v2 + e)
        else:
            p2 = p - lr_t * m_used / (np.sqrt(v2) + e)
    for a in (p2, m2, v2):
        assert a.dtype == F32
    return p2, m2, v2, lr_t


# ---- the 21 variables through the flat layout ----------------------------------------------------------------------------------------------
def layout(n5):
    from thesis_clip_nerf_amd import ops
    return ops.language_grad_layout(n5)


def flat_names(n5, order=None):
    """The entries of the flat layout in order (order='tail': the head's four, then the tail in the order of tail_w[] - the planted defect)."""
    names = list(layout(n5)[0])
    return names if order is None else names[:4] + list(TAIL_ORDER)


def to_flat(variables, n5, dtype, order=None):
    lay, total = layout(n5)
    flat = np.concatenate([np.asarray(variables[k], dtype).reshape(-1) for k in flat_names(n5, order)])
    assert flat.size == total
    return flat


def from_flat(flat, n5, order=None):
    lay, total = layout(n5)
    out, at = {}, 0
    for k in flat_names(n5, order):
        shape = lay[k][1]
        n = int(np.prod(shape))
        out[k] = flat[at:at + n].reshape(shape).copy()
        at += n
    return out


def random_variables(n5, seed, scale=0.1):
    rng = np.random.default_rng(seed)
    return {k: (scale * rng.standard_normal(shape)).astype(F32) for k, (_, shape) in layout(n5)[0].items()}


def step32(variables, grads, m, v, counter, n5, hyper=HYPER, defect=None):
    """One mvnerf_language_apply_gradients restated: variables {name: array} (w4 (4, 64, 128), b4 (4, 64) standing for the four layers),
    grads / m / v flat, counter = completed updates -> (variables', m', v', (w4 image, b4 image), counter + 1).  defect: any of DEFECTS,
    or of LAYOUT_DEFECTS: 'tail_order' lays the variables out in the order of tail_w[], 'no_mirror' leaves the stacked images alone."""
    order = 'tail' if defect == 'tail_order' else None
    p2, m2, v2, _ = update32(to_flat(variables, n5, F32, order), grads, m, v, counter + 1, **hyper,
                             defect=None if defect in LAYOUT_DEFECTS else defect)
    new = from_flat(p2, n5, order)
    image = (variables['w4'].copy(), variables['b4'].copy()) if defect == 'no_mirror' else (new['w4'].copy(), new['b4'].copy())
    return new, m2, v2, image, counter + 1


def step64(variables, grads, m, v, counter, n5, hyper=HYPER):
    """The same update in float64 -> (variables', m', v', bars: dict p (as variables), m, v)."""
    ref = update64(to_flat(variables, n5, np.float64), grads, m, v, counter + 1, **hyper)
    b = bars(ref)
    return from_flat(ref['p'], n5), ref['m'], ref['v'], dict(p=from_flat(b['p'], n5), m=b['m'], v=b['v'])
