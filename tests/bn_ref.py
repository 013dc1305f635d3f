"""References of the biased 3x3 convolution with a source activation and of the batch-statistics normalisation behind it
(csrc/conv3x3.hip mvnerf_conv3x3_nhwc_ex, csrc/batchnorm.hip), shared by tests/test_bn_conv_cpu.py and the GPU tests; written from the
formulas (layers.py:7-34 of the reference's Block), not by calling the package.  The convolution is tests/conv3x3_ref.py's.

    s = conv3x3_same(act_in(x), W) + bias          (zero padding AFTER act_in)
    y = act(s)
    out = relu( (y - mean_c) / sqrt(var_c + eps) * gamma_c + beta_c (+ skip) ),  mean, BIASED var over all N h w pixels of channel c

* :func:`conv_bias_ref`, :func:`bn_ref`, :func:`pipeline_ref` - float64.
* :func:`conv_bias_torch`, :func:`bn_torch`, :func:`pipeline_torch` - the torch path the passes replace, on the CPU in a dtype; in float32
  it is the yardstick e32, in float64 it checks the references.
* :func:`restated` - the passes' arithmetic in NumPy float32 (per-tile mean then M2 about it, Chan's combine in double, subtract-first
  apply), with `defect=` planting one wrong reading each.
* :func:`passes` - THE assertion of every test here: e64 <= 8 e32 on the relative L2 and on the worst element over the largest magnitude.
"""
import numpy as np

from tests import conv3x3_ref as R

TILE, COUT_TILE = R.TILE, R.COUT_TILE
BAR = R.BAR
EPS = 1e-3                                          # Keras BatchNormalization's default

# (N, h, w, Ca, Cout): one pixel; 2 x 3 pixel tiles with 3-pixel last tiles and two channel tiles; 1-pixel last tiles, three images
SHAPES = [(1, 1, 1, 32, 64), (2, TILE + 3, 2 * TILE + 3, 64, 2 * COUT_TILE), (3, 2 * TILE + 1, TILE + 1, 128, 2 * COUT_TILE)]
BN_SHAPES = [(1, 2, 3, 32, 64)] + SHAPES[1:]       # (torch's batch norm refuses one value per channel: the yardstick needs two pixels)
ACT_INS = [None, 'relu', 'elu']


def inputs(shape, seed=0, const=None):
    """x (N,h,w,Ca) unit normal (or the constant), Glorot-uniform HWIO kernel, bias, gamma, beta (Cout), skip (N,h,w,Cout); float32."""
    n, h, w, ca, cout = shape
    rng = np.random.default_rng([seed, *shape])
    x = rng.standard_normal((n, h, w, ca)).astype(np.float32)
    if const is not None:
        x = np.full_like(x, const)
    lim = np.sqrt(6.0 / (9 * ca + 9 * cout))
    wt = rng.uniform(-lim, lim, (3, 3, ca, cout)).astype(np.float32)
    bias = (0.5 * rng.standard_normal(cout)).astype(np.float32)
    gamma = (1.0 + 0.3 * rng.standard_normal(cout)).astype(np.float32)
    beta = (0.3 * rng.standard_normal(cout)).astype(np.float32)
    skip = rng.standard_normal((n, h, w, cout)).astype(np.float32)
    return dict(x=x, wt=wt, bias=bias, gamma=gamma, beta=beta, skip=skip)


def offset_map(shape, ratio=1e3, seed=0):
    """A convolution output (N,h,w,Cout) float32 whose channels have sigma = 1 and a mean of 0 (every fourth) or +-ratio x sigma."""
    n, h, w, _, cout = shape
    rng = np.random.default_rng([seed, 77, *shape])
    mean = np.where(np.arange(cout) % 4 == 0, 0.0, ratio * np.where(np.arange(cout) % 2 == 0, 1.0, -1.0))
    return (rng.standard_normal((n, h, w, cout)) + mean).astype(np.float32)


# ---- float64 ------------------------------------------------------------------------------------------------------------------------------
def conv_bias_ref(x, wt, bias, act_in=None, act=None):
    s = R.conv_ref(R.activation(np.asarray(x, np.float64), act_in), None, wt)
    return R.activation(s if bias is None else s + np.asarray(bias, np.float64), act)


def bn_ref(y, gamma, beta, skip=None, eps=EPS, relu=True):
    y = np.asarray(y, np.float64)
    mean, var = y.mean((0, 1, 2)), y.var((0, 1, 2))
    out = (y - mean) / np.sqrt(var + eps) * np.asarray(gamma, np.float64) + np.asarray(beta, np.float64)
    if skip is not None:
        out = out + np.asarray(skip, np.float64)
    return np.maximum(out, 0) if relu else out


def pipeline_ref(d, skip=True, act_in=None, act=None, eps=EPS):
    return bn_ref(conv_bias_ref(d['x'], d['wt'], d['bias'], act_in, act), d['gamma'], d['beta'], d['skip'] if skip else None, eps)


# ---- torch on the CPU ---------------------------------------------------------------------------------------------------------------------
def _t(v, dtype):
    import torch
    return torch.from_numpy(np.ascontiguousarray(v)).to(dtype)


def conv_bias_torch(x, wt, bias, act_in, act, dtype):
    import torch.nn.functional as F
    fn = {None: lambda v: v, 'relu': F.relu, 'elu': F.elu}
    xin = F.pad(fn[act_in](_t(x, dtype).permute(0, 3, 1, 2)), (1, 1, 1, 1))
    y = fn[act](F.conv2d(xin, _t(wt, dtype).permute(3, 2, 0, 1), None if bias is None else _t(bias, dtype)))
    return y.permute(0, 2, 3, 1).contiguous().numpy()


def bn_torch(y, gamma, beta, skip, dtype, eps=EPS, relu=True):
    import torch.nn.functional as F
    out = F.batch_norm(_t(y, dtype).permute(0, 3, 1, 2), None, None, _t(gamma, dtype), _t(beta, dtype), True, 0.0, eps)
    if skip is not None:
        out = out + _t(skip, dtype).permute(0, 3, 1, 2)
    out = F.relu(out) if relu else out
    return out.permute(0, 2, 3, 1).contiguous().numpy()


def pipeline_torch(d, dtype, skip=True, act_in=None, act=None, eps=EPS):
    y = conv_bias_torch(d['x'], d['wt'], d['bias'], act_in, act, dtype)
    return bn_torch(y, d['gamma'], d['beta'], d['skip'] if skip else None, dtype, eps)


def two_pass32(y, gamma, beta, skip=None, eps=EPS, relu=True):
    """A second float32 yardstick: the textbook two-pass normalisation, every operation rounded to float32 (pairwise NumPy sums)."""
    y = np.asarray(y, np.float32)
    n = np.float32(y.shape[0] * y.shape[1] * y.shape[2])
    mean = (y.sum((0, 1, 2), dtype=np.float32) / n).astype(np.float32)
    dev = y - mean
    var = ((dev * dev).sum((0, 1, 2), dtype=np.float32) / n).astype(np.float32)
    out = dev / np.sqrt(var + np.float32(eps)) * gamma + beta
    if skip is not None:
        out = out + skip
    return np.maximum(out, 0) if relu else out


_cache = {}


def cached(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def conv_case(shape, act_in, act=None):
    """(inputs, float64 reference, e32) of the biased convolution, once per case."""
    def make():
        import torch
        d = inputs(shape)
        ref = conv_bias_ref(d['x'], d['wt'], d['bias'], act_in, act)
        return d, ref, R.errors(conv_bias_torch(d['x'], d['wt'], d['bias'], act_in, act, torch.float32), ref)
    return cached(('conv', tuple(shape), act_in, act), make)


def pipeline_case(shape, skip=True, act_in=None, act=None, const=None, eps=EPS):
    """(inputs, float64 reference, e32) of convolution -> normalisation -> (skip) -> relu, once per case."""
    def make():
        import torch
        d = inputs(shape, const=const)
        ref = pipeline_ref(d, skip, act_in, act, eps)
        return d, ref, R.errors(pipeline_torch(d, torch.float32, skip, act_in, act, eps), ref)
    return cached(('pipe', tuple(shape), skip, act_in, act, const, eps), make)


def passes(out, ref, e32):
    """e64 <= 8 e32, relative L2 and worst element -> (bool, figures)."""
    e = R.errors(out, ref)
    return bool(e[0] <= BAR * e32[0] and e[1] <= BAR * e32[1]), (e, e32)


# ---- the passes' arithmetic ----------------------------------------------------------------------------------------------------------------
def tile_stats(y):
    """y (N,h,w,C) float32 -> per tile [n, ty, tx]: (count, mean (C,), M2 (C,)) as the kernel forms them: mean = ref + sum(y - ref) / k with
    ref the tile's first pixel, then M2 about that mean; float32 (NumPy's summation order, not the kernel's)."""
    n, h, w, _ = y.shape
    out = []
    for i in range(n):
        for y0 in range(0, h, TILE):
            for x0 in range(0, w, TILE):
                t = y[i, y0:y0 + TILE, x0:x0 + TILE].reshape(-1, y.shape[3])
                k = np.float32(t.shape[0])
                ref = t[0]
                mean = (ref + (t - ref).sum(0, dtype=np.float32) / k).astype(np.float32)
                dev = t - mean
                out.append((float(k), mean, (dev * dev).sum(0, dtype=np.float32)))
    return out


def chan_combine(parts):
    count, mean, m2 = 0.0, 0.0, 0.0
    for k, mu, q in parts:
        mu, q = mu.astype(np.float64), q.astype(np.float64)
        if count == 0.0:
            count, mean, m2 = k, mu, q
            continue
        total, delta = count + k, mu - mean
        mean, m2 = mean + delta * (k / total), m2 + q + delta * delta * (count * k / total)
        count = total
    return count, mean, m2


DEFECTS = ['raw_sums', 'unbiased', 'padding_counted', 'bias_after_act', 'act_in_pad_nonzero', 'skip_after_relu', 'eps_dropped', 'per_image']


def restated_conv(d, act_in=None, act=None, defect=None, extend=False):
    """The kernel's convolution at fp32 grade: the float64 sum rounded once, then bias and activation in float32.  extend: on the canvas
    of whole 16 x 16 tiles, the input zero beyond the image (what the accumulators of an edge tile's padding pixels hold)."""
    x = R.activation(d['x'].astype(np.float64), act_in)
    n, h, w, _ = x.shape
    if extend:
        x = np.pad(x, ((0, 0), (0, -h % TILE), (0, -w % TILE), (0, 0)))
    if defect == 'act_in_pad_nonzero':                 # the taps outside the image read the activated edge pixel instead of zero
        xp = np.pad(x, ((0, 0), (1, 1), (1, 1), (0, 0)), mode='edge')
        s = sum(xp[:, dy:dy + h, dx:dx + w] @ d['wt'][dy, dx].astype(np.float64) for dy in range(3) for dx in range(3))
    else:
        s = R.conv_ref(x, None, d['wt'])
    s = s.astype(np.float32)
    if defect == 'bias_after_act':
        return (R.activation(s, act) + d['bias']).astype(np.float32)
    return R.activation(s + d['bias'], act).astype(np.float32)


def restated_bn(y, gamma, beta, skip=None, eps=EPS, defect=None, y_extended=None):
    n, h, w, c = y.shape
    if defect == 'raw_sums':                            # E[y^2] - E[y]^2 from raw float32 sums
        k = np.float32(n * h * w)
        mean = (y.sum((0, 1, 2), dtype=np.float32) / k).astype(np.float32)
        var = ((y * y).sum((0, 1, 2), dtype=np.float32) / k - mean * mean).astype(np.float64)
        mean = mean.astype(np.float64)[None]
        var = var[None]
    else:
        groups = [y[i:i + 1] for i in range(n)] if defect == 'per_image' else [y_extended if defect == 'padding_counted' else y]
        mean, var = [], []
        for g in groups:
            count, mu, m2 = chan_combine(tile_stats(g))
            mean.append(mu)
            var.append(m2 / (count - 1 if defect == 'unbiased' else count))
        mean, var = np.stack(mean), np.stack(var)
    with np.errstate(invalid='ignore', divide='ignore'):          # (raw sums can leave a negative variance)
        rstd = (1.0 / np.sqrt(var + (0.0 if defect == 'eps_dropped' else eps))).astype(np.float32)
    mean = mean.astype(np.float32)
    if mean.shape[0] == 1:
        mean, rstd = mean[0], rstd[0]
    else:
        mean, rstd = mean[:, None, None, :], rstd[:, None, None, :]
    with np.errstate(invalid='ignore', over='ignore'):
        t = (((y - mean).astype(np.float32) * rstd).astype(np.float32) * gamma).astype(np.float32) + beta
        if skip is not None and defect != 'skip_after_relu':
            t = t + skip
        t = np.maximum(t, 0).astype(np.float32)
        if skip is not None and defect == 'skip_after_relu':
            t = t + skip
    return t.astype(np.float32)


def restated(d, skip=True, act_in=None, act=None, eps=EPS, defect=None):
    y = restated_conv(d, act_in, act, defect)
    ext = restated_conv(d, act_in, act, defect, extend=True) if defect == 'padding_counted' else None
    return restated_bn(y, d['gamma'], d['beta'], d['skip'] if skip else None, eps, defect, ext)
