"""References of the backward through a frozen 3x3 convolution of the language fusion (csrc/act_gate.hip, csrc/mvnerf_act_gate.h,
encoders.Conv3x3ActFunction), shared by tests/test_act_gate_cpu.py and the GPU modules.  Written from the definition and not
by calling the package.  For out = mul * act(y), y = conv3x3_same([a | b], W), NHWC maps, mul (N, C), and g = dL/dout:

    d  = g * mul * act'(y)                     relu'(y) = [y > 0],  elu'(y) = 1 for y > 0, exp(y) otherwise (1 at y == 0)
    da = conv3x3_same(d, W'[:, :, :, :Ca])     W'[dy,dx,co,ci] = W[2-dy,2-dx,ci,co];  db from the rows Ca: of W

* :func:`gate_ref` - d in float64 from y itself.
* :func:`forward32` - `out` as the convolution's epilogue writes it: float32 act(y), then one float32 multiplication.
* :func:`gate_np` - a NumPy restatement of mvnerf_act_gate.h's arithmetic: d from `out` and `mul` alone in float32, one rounding per
  operation, no division.  `defect=` plants one wrong reading.
* :func:`torch_gate` - the yardstick: torch CPU autograd of act(y) * mul in a given dtype.
* :func:`two_source_grads_ref` - (da, db) in float64."""
import numpy as np

from tests import conv3x3_bwd_ref as B
from tests import conv3x3_ref as R

BAR = R.BAR
ACTS = ['relu', 'elu']
ACT_CODES = {None: 0, 'relu': 1, 'elu': 2}
MUL_KINDS = ['none', 'positive', 'mixed', 'with_zero']
# (N, h, w, C): one quad; two images smaller than a block; more than one block per image (19 * 35 * 64 / 4 quads), odd sizes; three images
GATE_SHAPES = [(1, 1, 1, 4), (2, 3, 5, 32), (2, 19, 35, 64), (3, 16, 16, 128)]
DEFECTS = ['mask_ignores_mul_sign', 'mul_forgotten', 'mul_twice', 'relu_passes_at_zero', 'elu_branch_from_out', 'mul_per_pixel']


def gate_inputs(shape, mul_kind, seed=0):
    """Seeded g, y (N,h,w,C) unit normals - about one y in eight an exact zero - and mul (N,C) | None of the kind; float32."""
    n, h, w, c = shape
    rng = np.random.default_rng([seed, 22, *shape, MUL_KINDS.index(mul_kind)])
    g = rng.standard_normal(shape).astype(np.float32)
    y = rng.standard_normal(shape).astype(np.float32)
    y[rng.random(shape) < 0.125] = 0.0
    mul = None
    if mul_kind != 'none':
        mul = (0.25 + rng.random((n, c)) * 1.5).astype(np.float32)
        if mul_kind in ('mixed', 'with_zero'):
            mul = mul * np.where(rng.random((n, c)) < 0.5, -1, 1).astype(np.float32)
        if mul_kind == 'with_zero':
            mul[:, ::3] = 0.0
    return g, y, mul


def _rows(mul, shape):
    """mul (N,C) | None -> broadcastable over (N,h,w,C); None means 1."""
    return np.ones((1, 1, 1, 1), np.float32) if mul is None else np.asarray(mul)[:, None, None, :]


def gate_ref(g, y, mul, act):
    g, y = np.asarray(g, np.float64), np.asarray(y, np.float64)
    return g * _rows(mul, y.shape).astype(np.float64) * B.act_grad(y, act)


def forward32(y, mul, act):
    y = np.asarray(y, np.float32)
    return (R.activation(y, act).astype(np.float32) * _rows(mul, y.shape).astype(np.float32)).astype(np.float32)


def gate_np(g, out, mul, act, defect=None):
    """mvnerf_act_gate.h act_gate_one over whole arrays, float32 throughout."""
    g, out = np.asarray(g, np.float32), np.asarray(out, np.float32)
    m = np.broadcast_to(_rows(mul, out.shape).astype(np.float32), out.shape)
    if defect == 'mul_per_pixel' and mul is not None:             # the row of mul taken from the pixel index, not the image index
        n, h, w, c = out.shape
        m = np.asarray(mul, np.float32)[np.arange(n * h * w) % n].reshape(n, h, w, c)
    positive = ((out > 0) & (m > 0)) | ((out < 0) & (m < 0))
    if defect == 'mask_ignores_mul_sign':
        positive = out > 0
    if defect == 'relu_passes_at_zero' and act == 'relu':
        positive = ((out >= 0) & (m > 0)) | ((out <= 0) & (m < 0))
    if defect == 'elu_branch_from_out' and act == 'elu':
        positive = out >= 0
    straight = (g * m).astype(np.float32)
    if defect == 'mul_twice':
        straight = (straight * m).astype(np.float32)
    if act is None:
        d = straight
    elif act == 'relu':
        d = np.where(positive, straight, np.float32(0))
    else:
        slope = (out + (np.float32(1) if defect == 'mul_forgotten' else m)).astype(np.float32)
        d = np.where(positive, straight, (g * slope).astype(np.float32))
    return np.where(m == 0, np.float32(0), d).astype(np.float32)


def torch_gate(g, y, mul, act, dtype):
    """torch CPU autograd of sum(g * act(y) * mul) with respect to y in `dtype` -> array."""
    import torch
    import torch.nn.functional as F
    t = lambda v: torch.from_numpy(np.ascontiguousarray(v)).to(dtype)
    yt = t(y).requires_grad_(True)
    out = {None: lambda v: v, 'relu': F.relu, 'elu': F.elu}[act](yt)
    if mul is not None:
        out = out * t(mul)[:, None, None, :]
    out.backward(t(g))
    return yt.grad.numpy()


_e32 = {}


def gate_e32(shape, mul_kind, act, seed=0):
    """(relative L2, worst element) of torch's float32 autograd against :func:`gate_ref`, once per case."""
    import torch
    key = (tuple(shape), mul_kind, act, seed)
    if key not in _e32:
        g, y, mul = gate_inputs(shape, mul_kind, seed)
        _e32[key] = R.errors(torch_gate(g, y, mul, act, torch.float32), gate_ref(g, y, mul, act))
    return _e32[key]


def within_bar(err, yard, bar=BAR):
    return all(e <= bar * y for e, y in zip(err, yard))


# ---- the two-source convolution ------------------------------------------------------------------------------------------------------------
def two_source_inputs(shape, mul_kind, seed=0):
    """conv3x3_ref.inputs of (N,h,w,Ca,Cb,Cout) with the mul of `mul_kind` and a cotangent g (N,h,w,Cout); float32."""
    n, h, w, ca, cb, cout = shape
    a, b, wt, _ = R.inputs(shape, seed)
    rng = np.random.default_rng([seed, 23, *shape, MUL_KINDS.index(mul_kind)])
    g = rng.standard_normal((n, h, w, cout)).astype(np.float32)
    mul = None
    if mul_kind != 'none':
        mul = (0.25 + rng.random((n, cout)) * 1.5).astype(np.float32)
        if mul_kind in ('mixed', 'with_zero'):
            mul = mul * np.where(rng.random((n, cout)) < 0.5, -1, 1).astype(np.float32)
        if mul_kind == 'with_zero':
            mul[:, ::3] = 0.0
    return a, b, wt, mul, g


def two_source_grads_ref(a, b, wt, mul, act, g):
    """(da, db | None) of sum(g * mul * act(conv3x3_same([a | b], W))) in float64."""
    ca = a.shape[3]
    d = gate_ref(g, R.conv_ref(a, b, wt), mul, act)
    wt = np.asarray(wt, np.float64)
    da = B.dx_ref(a, d, wt[:, :, :ca])
    db = None if b is None else B.dx_ref(b, d, wt[:, :, ca:])
    return da, db


def torch_two_source_grads(a, b, wt, mul, act, g, dtype):
    """torch CPU autograd of the same sum in `dtype` -> (da, db | None) NHWC arrays."""
    import torch
    import torch.nn.functional as F
    t = lambda v: torch.from_numpy(np.ascontiguousarray(v)).to(dtype)
    at = t(a).permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    bt = None if b is None else t(b).permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    y = F.conv2d(at if bt is None else torch.cat([at, bt], 1), t(wt).permute(3, 2, 0, 1), padding=1)
    out = {None: lambda v: v, 'relu': F.relu, 'elu': F.elu}[act](y)
    if mul is not None:
        out = out * t(mul)[:, :, None, None]
    out.backward(t(g).permute(0, 3, 1, 2))
    nhwc = lambda v: None if v is None else v.grad.permute(0, 2, 3, 1).contiguous().numpy()
    return nhwc(at), nhwc(bt)
