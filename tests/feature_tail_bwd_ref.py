"""References of the backward pass of the producers' tail (csrc/feature_tail_bwd.hip, csrc/mvnerf_feature_tail.h), written
from the forward's definition in tests/feature_fusion_ref.py and not by calling thesis_clip_nerf_amd:

* :func:`tail_bwd_ref` - float64: the up-sampling as the matrix of :func:`feature_fusion_ref._axis_taps`, its transpose applied to g, the
  1x1 convolution's transpose, act'.  `mistake=` plants one wrong reading, for the test that each of them is far above the bar.
* :func:`tail_bwd_f32` - the NumPy float32 restatement of the header: coefficients with the fold, rows first then columns from +0 in
  ascending order, one rounding per operation, act'.  The host build of the header must equal it bit for bit.
* the shapes, inputs and the bar of the GPU tests, shared with their CPU companion (tests/test_feature_tail_bwd_cpu.py)."""
import numpy as np

from tests import feature_fusion_ref as R

TILE_H, TILE_W = 8, 16                  # csrc/mvnerf_feature_tail.h: kFtbTileH, kFtbTileW
# (N, h, w, Ca, Cb, act): the forward's shapes, exactly one 8 x 16 tile, two tiles and one pixel each way
SHAPES = list(R.TAIL_SHAPES) + [(1, 8, 16, 16, 16, 'elu'), (1, 17, 33, 32, 16, None)]
INTEGER_SHAPE = (1, 9, 17, 16, 16, None)
DEFECT_SHAPE = (1, 9, 11, 128, 128, 'elu')          # Ca + Cb = 256 (W for W^T keeps its shape), Ca = Cb (da for db keeps its shape)
BAR = R.TAIL_BAR                          # e64 of the code under test <= BAR x e64 of torch's float32 CPU autograd of the same tail
ARRAYS = ('da', 'db', 'g_low', 'dw')


def cotangent(shape, seed=0):
    """Seeded unit-normal g = dL/dout (N, 2h, 2w, 256), float32."""
    n, h, w, ca, cb, _ = shape
    rng = np.random.default_rng([seed + 1000, n, h, w, ca, cb])
    return rng.standard_normal((n, 2 * h, 2 * w, 256)).astype(np.float32)


def integer_case(shape=INTEGER_SHAPE, seed=0):
    """a, b in [-3, 3], W in [-8, 8] / 8, g in [-4, 4], all integers: every sum of the pass is exact in fp32."""
    n, h, w, ca, cb, _ = shape
    rng = np.random.default_rng([seed + 2000, n, h, w, ca, cb])
    a = rng.integers(-3, 4, (n, h, w, ca)).astype(np.float32)
    b = rng.integers(-3, 4, (n, h, w, cb)).astype(np.float32)
    weight = (rng.integers(-8, 9, (ca + cb, 256)) / 8.0).astype(np.float32)
    g = rng.integers(-4, 5, (n, 2 * h, 2 * w, 256)).astype(np.float32)
    return a, b, weight, g


# ---- float64 ----------------------------------------------------------------------------------------------------------------------------
def upsample_matrix(n_in, mistake=None):
    """U (2 n_in, n_in) float64 with out = U @ low along one axis, from the forward's taps."""
    i0, i1, lam = R._axis_taps(n_in, 2 * n_in, align_corners=mistake == 'align_corners')
    if mistake == 'quarter_swapped':
        lam = np.where((lam > 0) & (lam < 1), 1.0 - lam, lam)
    u = np.zeros((2 * n_in, n_in))
    o = np.arange(2 * n_in)
    if mistake == 'border_dropped':                 # the taps that clamp are left out instead of folded onto the border sample
        src = (o + 0.5) / 2 - 0.5
        lo = np.floor(src).astype(np.int64)
        frac = src - lo
        for k, wgt in ((lo, 1.0 - frac), (lo + 1, frac)):
            ok = (k >= 0) & (k < n_in)
            np.add.at(u, (o[ok], k[ok]), wgt[ok])
        return u
    np.add.at(u, (o, i0), 1.0 - lam)
    np.add.at(u, (o, i1), lam)
    return u


def act_grad(x, d, name, mistake=None):
    if mistake == 'no_act_grad':
        return d
    if mistake == 'relu_for_elu' and name == 'elu':
        name = 'relu'
    if name is None:
        return d
    if name == 'relu':
        return np.where(x >= 0 if mistake == 'mask_ge' else x > 0, d, 0.0)
    if name == 'elu':
        if mistake == 'exp_everywhere':
            return d * np.exp(x)
        return np.where(x > 0, d, d * np.exp(np.minimum(x, 0.0)))
    raise ValueError(name)


def tail_bwd_ref(g, a, b, weight, act, mistake=None):
    """-> dict(da, db, g_low, dw) in float64: the gradients of sum(out * g) for out = feature_fusion_ref.tail_ref(a, b, weight, act)."""
    g, a, b, weight = (np.asarray(t, dtype=np.float64) for t in (g, a, b, weight))
    ca = a.shape[3]
    x = np.concatenate([a, b], -1)
    uy, ux = upsample_matrix(a.shape[1], mistake), upsample_matrix(a.shape[2], mistake)
    g_low = np.einsum('Yy,Xx,nYXc->nyxc', uy, ux, g, optimize=True)
    w_used = weight[::-1] if mistake == 'reversed_weight' else weight
    d_pre = g_low @ (w_used if mistake == 'w_not_transposed' else w_used.T)
    dx = act_grad(x, d_pre, act, mistake)
    da, db = dx[..., :ca], dx[..., ca:]
    if mistake == 'swapped':
        da, db = db, da
    dw = R.activation(x, act).reshape(-1, x.shape[3]).T @ g_low.reshape(-1, 256)
    return dict(da=da, db=db, g_low=g_low, dw=dw)


MISTAKES = ('border_dropped', 'align_corners', 'quarter_swapped', 'no_act_grad', 'relu_for_elu', 'exp_everywhere', 'mask_ge',
            'w_not_transposed', 'swapped', 'reversed_weight')


# ---- the float32 restatement of csrc/mvnerf_feature_tail.h --------------------------------------------------------------------------------
def coef(o, l, n):
    """ftb_coef: the weight with which output index o of an axis of n low samples reads low index l, float32."""
    t0 = (o - 1) >> 1
    l0, l1 = max(t0, 0), min(t0 + 1, n - 1)
    w0, w1 = (np.float32(0.75), np.float32(0.25)) if o & 1 else (np.float32(0.25), np.float32(0.75))
    c = np.float32(0.0)
    if l0 == l:
        c = np.float32(c + w0)
    if l1 == l:
        c = np.float32(c + w1)
    return c


def taps(l, n):
    """ftb_taps: [(output index, coefficient)] of low index l, ascending; only the outputs that exist."""
    return [(o, coef(o, l, n)) for o in range(2 * l - 1, 2 * l + 3) if 0 <= o < 2 * n]


def adjoint_f32(g):
    """g (N, 2h, 2w, C) float32 -> g_low (N, h, w, C) float32 in the header's order: rows first, then columns, each from +0, ascending."""
    g = np.asarray(g, dtype=np.float32)
    n, h2, w2, c = g.shape
    h, w = h2 // 2, w2 // 2
    rows = np.zeros((n, h, w2, c), np.float32)
    for y in range(h):
        acc = np.zeros((n, w2, c), np.float32)
        for o, cf in taps(y, h):
            acc = acc + g[:, o] * cf
        rows[:, y] = acc
    out = np.zeros((n, h, w, c), np.float32)
    for x in range(w):
        acc = np.zeros((n, h, c), np.float32)
        for o, cf in taps(x, w):
            acc = acc + rows[:, :, o] * cf
        out[:, :, x] = acc
    return out


def act_grad_f32(x, d, name):
    """ftb_act_grad in float32 (np.exp for expf: within an ulp of the C library's)."""
    x, d = np.asarray(x, np.float32), np.asarray(d, np.float32)
    if name is None:
        return d
    if name == 'relu':
        return np.where(x > 0, d, np.float32(0.0))
    with np.errstate(over='ignore', invalid='ignore'):
        return np.where(x > 0, d, d * np.exp(np.minimum(x, np.float32(0.0))))


def tail_bwd_f32(g, a, b, weight, act):
    """The pass in float32 throughout (the product by NumPy's matmul, whose order is not the kernel's) -> dict(da, db, g_low, dw)."""
    a, b, weight = (np.asarray(t, np.float32) for t in (a, b, weight))
    x = np.concatenate([a, b], -1)
    g_low = adjoint_f32(g)
    dx = act_grad_f32(x, g_low @ weight.T, act)
    dw = R.activation(x, act).astype(np.float32).reshape(-1, x.shape[3]).T @ g_low.reshape(-1, 256)
    return dict(da=dx[..., :a.shape[3]], db=dx[..., a.shape[3]:], g_low=g_low, dw=dw)


# ---- the yardstick: torch autograd of the torch tail --------------------------------------------------------------------------------------
def torch_tail_grads(g, a, b, weight, act, dtype, device='cpu'):
    """Autograd of cat -> act -> 1x1 conv -> interpolate (the tail the fused pass replaces) in `dtype` -> dict(da, db, g_low, dw) arrays."""
    import torch
    import torch.nn.functional as F
    ta, tb, tw, tg = (torch.from_numpy(np.array(t)).to(dtype).to(device) for t in (a, b, weight, g))     # (a copy: the cached cases are read-only)
    ta.requires_grad_(True), tb.requires_grad_(True), tw.requires_grad_(True)
    x = torch.cat([ta, tb], -1).permute(0, 3, 1, 2)
    x = {None: lambda t: t, 'relu': F.relu, 'elu': F.elu}[act](x)
    y = F.conv2d(x, tw.t().reshape(tw.shape[1], tw.shape[0], 1, 1))
    y.retain_grad()
    out = F.interpolate(y, scale_factor=2, mode='bilinear', align_corners=False)
    out.backward(tg.permute(0, 3, 1, 2))
    host = lambda t: t.detach().cpu().numpy()
    return dict(da=host(ta.grad), db=host(tb.grad), g_low=host(y.grad.permute(0, 2, 3, 1)), dw=host(tw.grad))


def errors(got, ref):
    """{array: (relative L2, worst element over largest magnitude)} of the arrays `got` holds."""
    return {k: (R.rel_l2(got[k], ref[k]), R.worst(got[k], ref[k])) for k in got if got[k] is not None}


_cases = {}


def case(shape, seed=0):
    """(a, b, weight, g, float64 reference, errors of torch's float32 CPU autograd), computed once per shape and never changed."""
    key = (tuple(shape), seed)
    if key not in _cases:
        import torch
        a, b, weight = R.tail_inputs(shape, seed)
        g = cotangent(shape, seed)
        ref = tail_bwd_ref(g, a, b, weight, shape[5])
        e32 = errors(torch_tail_grads(g, a, b, weight, shape[5], torch.float32), ref)
        for t in (a, b, weight, g, *ref.values()):
            t.setflags(write=False)
        _cases[key] = (a, b, weight, g, ref, e32)
    return _cases[key]


def assert_at_bar(got, ref, e32, what, names=None, bar=BAR, report=None):
    """Every array of `got` (or `names`) within bar x the float32 yardstick, as relative L2 and as worst element.  Prints the figures
    first; report: a dict that receives {array: (ratio L2, ratio worst)}."""
    e64 = errors({k: got[k] for k in (names or got)}, ref)
    for k, (l2, wst) in e64.items():
        ratios = (l2 / e32[k][0], wst / e32[k][1])
        print(f'{what} {k}: e64 {l2:.3e} / {wst:.3e}, e32 {e32[k][0]:.3e} / {e32[k][1]:.3e}, ratios {ratios[0]:.2f} / {ratios[1]:.2f}')
        if report is not None:
            report[k] = ratios
    for k, (l2, wst) in e64.items():
        assert l2 <= bar * e32[k][0], (what, k, 'relative L2', l2, e32[k][0])
        assert wst <= bar * e32[k][1], (what, k, 'worst element', wst, e32[k][1])
