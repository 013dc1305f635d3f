"""References of the fused 3x3 convolution (csrc/conv3x3.hip, csrc/mvnerf_conv.h), shared by tests/test_conv3x3_cpu.py and
tests/test_gpu_conv3x3.py; written from the formula and not by calling the package:

    y[n,i,j,co] = mul[n,co] * act( sum_{dy,dx} sum_c X[n,i+dy-1,j+dx-1,c] W[dy,dx,c,co] ),  X = [a | b], taps outside the image 0

* :func:`conv_ref` - the formula in float64, NHWC, HWIO kernel.
* :func:`split_conv` - a NumPy restatement of the kernel's arithmetic: power-of-two scales from amax, two fp16 pieces per operand, three
  products, fp32 accumulation per (32-channel chunk, tap) in the kernel's order, the rescale at the a -> b boundary.  `defect=` plants one
  wrong reading, for the test that the bar can tell each of them.
* :func:`e32` - the yardstick: the error against float64 of torch's float32 CPU run of the same case; for K >= 4096 the larger of that
  and of a float32 k-ordered fma-free chain (the order of the exact-fp32 MFMA kernels): torch's CPU blocking is an accident the bar must
  not depend on."""
import numpy as np

# kernel tile constants (csrc/conv3x3.hip: kCvTile, kCvCout, kCvChunk)
TILE, COUT_TILE, CHUNK = 16, 64, 32
BAR = 8.0

# (N, h, w, Ca, Cb, Cout)
ONE_PIXEL = (1, 1, 1, 32, 0, 64)                 # every tap but the centre is padding
SMALL_TWO = (2, 3, 5, 32, 32, 64)                # smaller than a tile both ways, two sources, two images
LONG_K = (1, 4, 4, 2048, 0, 64)                  # K = 18432, the reference's longest
# from the tile constants: 19 = 16 + 3 rows, 35 = 2 * 16 + 3 columns, 128 = 2 * 64 channels (a channel tile cannot be partial: Cout % 64
# == 0 is the accepted set), N = 3; the second has one source and a single-column last tile
TILED_TWO = (3, TILE + 3, 2 * TILE + 3, 32, 64, 2 * COUT_TILE)
TILED_ONE = (3, 2 * TILE + 1, TILE + 1, 64, 0, 2 * COUT_TILE)
SHAPES = [ONE_PIXEL, SMALL_TWO, LONG_K, TILED_TWO, TILED_ONE]
ACTS = [None, 'relu', 'elu']


def inputs(shape, seed=0, scale_a=1.0, scale_b=1.0):
    """Seeded a (N,h,w,Ca), b (N,h,w,Cb) | None unit normals times the scales, a Glorot-uniform HWIO kernel, mul (N,Cout); float32."""
    n, h, w, ca, cb, cout = shape
    rng = np.random.default_rng([seed, *shape])
    a = (rng.standard_normal((n, h, w, ca)) * scale_a).astype(np.float32)
    b = (rng.standard_normal((n, h, w, cb)) * scale_b).astype(np.float32) if cb else None
    lim = np.sqrt(6.0 / (9 * (ca + cb) + 9 * cout))
    wt = rng.uniform(-lim, lim, (3, 3, ca + cb, cout)).astype(np.float32)
    mul = rng.standard_normal((n, cout)).astype(np.float32)
    return a, b, wt, mul


def activation(x, name):
    if name is None:
        return x
    if name == 'relu':
        return np.maximum(x, 0)
    if name == 'elu':
        return np.where(x > 0, x, np.expm1(np.minimum(x, 0)))
    raise ValueError(name)


def _cat(a, b):
    return a if b is None else np.concatenate([a, b], -1)


def _padded(x, mode='constant'):
    return np.pad(x, ((0, 0), (1, 1), (1, 1), (0, 0)), mode=mode)


def conv_ref(a, b, wt, act=None, mul=None):
    x = _padded(_cat(a, b).astype(np.float64))
    wt = np.asarray(wt, np.float64)
    n, h, w = a.shape[:3]
    y = np.zeros((n, h, w, wt.shape[3]))
    for dy in range(3):
        for dx in range(3):
            y += x[:, dy:dy + h, dx:dx + w] @ wt[dy, dx]
    y = activation(y, act)
    return y if mul is None else y * np.asarray(mul, np.float64)[:, None, None, :]


def rel_l2(x, ref):
    x, ref = np.asarray(x, np.float64), np.asarray(ref, np.float64)
    return float(np.linalg.norm((x - ref).ravel()) / np.linalg.norm(ref.ravel()))


def worst(x, ref):
    x, ref = np.asarray(x, np.float64), np.asarray(ref, np.float64)
    return float(np.abs(x - ref).max() / np.abs(ref).max())


def errors(x, ref):
    return rel_l2(x, ref), worst(x, ref)


def torch_conv(a, b, wt, act, mul, dtype):
    """The torch path the kernel replaces (cat -> pad -> conv2d -> activation -> multiply) on the CPU in `dtype` -> NHWC array."""
    import torch
    import torch.nn.functional as F
    t = lambda v: torch.from_numpy(np.ascontiguousarray(v)).to(dtype)
    x = F.pad(t(_cat(a, b)).permute(0, 3, 1, 2), (1, 1, 1, 1))
    y = F.conv2d(x, t(wt).permute(3, 2, 0, 1))
    y = {None: lambda v: v, 'relu': F.relu, 'elu': F.elu}[act](y)
    if mul is not None:
        y = y * t(mul)[:, :, None, None]
    return y.permute(0, 2, 3, 1).contiguous().numpy()


def chain32(a, b, wt, act, mul):
    """float32, one rounding per product and per sum, k in order (tap, channel): the exact-fp32 MFMA's chain."""
    x = _padded(_cat(a, b).astype(np.float32))
    n, h, w = a.shape[:3]
    acc = np.zeros((n, h, w, wt.shape[3]), np.float32)
    for dy in range(3):
        for dx in range(3):
            xs = x[:, dy:dy + h, dx:dx + w]
            for k in range(xs.shape[3]):
                acc = acc + xs[..., k:k + 1] * wt[dy, dx, k]
    y = activation(acc, act).astype(np.float32)
    return y if mul is None else y * mul[:, None, None, :]


_e32 = {}


def e32(shape, act, with_mul, seed=0, scale_a=1.0, scale_b=1.0):
    """(relative L2, worst element) of the float32 yardstick run against :func:`conv_ref`, once per case."""
    key = (tuple(shape), act, with_mul, seed, scale_a, scale_b)
    if key not in _e32:
        import torch
        a, b, wt, mul = inputs(shape, seed, scale_a, scale_b)
        mul = mul if with_mul else None
        ref = conv_ref(a, b, wt, act, mul)
        err = errors(torch_conv(a, b, wt, act, mul, torch.float32), ref)
        if 9 * (shape[3] + shape[4]) >= 4096:
            err = tuple(max(p, q) for p, q in zip(err, errors(chain32(a, b, wt, act, mul), ref)))
        _e32[key] = err
    return _e32[key]


# ---- the kernel's arithmetic ------------------------------------------------------------------------------------------------------------
def scale_exp(amax):
    """mvnerf_conv.h conv_scale_exp: e with amax * 2^e in [2^8, 2^9), 0 for amax == 0; subnormals counted from their leading bit."""
    amax = np.float32(abs(amax))
    if amax == 0:
        return 0
    return 8 - (int(np.frexp(np.float64(amax))[1]) - 1)


def cut_weight(wt, ew):
    tw = np.ldexp(np.asarray(wt, np.float32), ew).astype(np.float32)
    a0 = tw.astype(np.float16)
    a1 = (tw - a0.astype(np.float32)).astype(np.float16)
    a0s = (a0.astype(np.float32) * np.float32(1 / 64)).astype(np.float16)
    return a0, a1, a0s


def cut_act(x, ex):
    with np.errstate(over='ignore', invalid='ignore'):
        tx = np.ldexp(np.asarray(x, np.float32), ex).astype(np.float32)
        b0 = tx.astype(np.float16)
        b1 = (np.float32(64) * (tx - b0.astype(np.float32))).astype(np.float16)
    return b0, b1


def split_conv(a, b, wt, act=None, mul=None, amax_a=None, amax_b=None, defect=None):
    """The kernel's arithmetic in NumPy -> float32 (N,h,w,Cout).  The three products of one (chunk, tap) are summed in float64 (exact
    for fp16 factors) and rounded into the fp32 accumulator; the MFMA truncates inside that sum, so the kernel sits a little above this."""
    if defect == 'ab_swapped' and b is not None:
        a, b, amax_a, amax_b = b, a, amax_b, amax_a
    if defect == 'taps_transposed':
        wt = np.ascontiguousarray(np.swapaxes(wt, 0, 1))
    if defect == 'taps_flipped':
        wt = np.ascontiguousarray(wt[::-1, ::-1])
    n, h, w, ca = a.shape
    cb = 0 if b is None else b.shape[3]
    cout = wt.shape[3]
    ea = scale_exp(np.abs(a).max() if amax_a is None else amax_a)
    eb = 0 if b is None else scale_exp(np.abs(b).max() if amax_b is None else amax_b)
    ew = scale_exp(np.abs(wt).max())
    a0, a1, a0s = (p.astype(np.float64) for p in cut_weight(wt, ew))
    pad = 'edge' if defect == 'clamp_padding' else 'constant'
    pieces = [tuple(_padded(p.astype(np.float64), pad) for p in cut_act(a, ea))]
    if b is not None:
        pieces.append(tuple(_padded(p.astype(np.float64), pad) for p in cut_act(b, eb)))
    acc = np.zeros((n, h, w, cout), np.float32)
    for c in range((ca + cb) // CHUNK):
        src, c0 = (0, c * CHUNK) if c * CHUNK < ca else (1, c * CHUNK - ca)
        if src == 1 and c0 == 0 and ea != eb and defect != 'no_rescale':
            acc = np.ldexp(acc, eb - ea).astype(np.float32)
        b0, b1 = (p[..., c0:c0 + CHUNK] for p in pieces[src])
        ks = slice(c * CHUNK, (c + 1) * CHUNK)
        for dy in range(3):
            for dx in range(3):
                x0, x1 = b0[:, dy:dy + h, dx:dx + w], b1[:, dy:dy + h, dx:dx + w]
                s = x0 @ a0[dy, dx, ks]
                if defect != 'drop_a0s_b1':
                    s = s + x1 @ a0s[dy, dx, ks]
                if defect != 'drop_a1_b0':
                    s = s + x0 @ a1[dy, dx, ks]
                acc = (acc.astype(np.float64) + s).astype(np.float32)
    undo = -((0 if defect == 'weight_scale_kept' else ew) + (eb if b is not None else ea))
    with np.errstate(over='ignore'):
        y = np.ldexp(acc, undo).astype(np.float32)
    m = None if mul is None else np.asarray(mul, np.float32)[:, None, None, :]
    if defect == 'act_after_mul' and m is not None:
        return activation(y * m, act).astype(np.float32)
    y = activation(y, 'relu' if defect == 'relu_for_elu' and act == 'elu' else act).astype(np.float32)
    return y if m is None else y * m


DEFECTS = ['drop_a1_b0', 'drop_a0s_b1', 'weight_scale_kept', 'clamp_padding', 'taps_transposed', 'taps_flipped', 'ab_swapped',
           'act_after_mul', 'relu_for_elu']          # ('no_rescale' has its own case: sources of 1e3 and 1e-3)
