"""References of the transformer-block passes (csrc/token_linear.hip, csrc/attention.hip, csrc/mvnerf_vit.h), shared by
tests/test_vit_cpu.py, tests/test_gpu_vit_ops.py and tests/test_gpu_fused_vit.py; written from the Keras semantics of the reference's
`TransformerBlock` (layers.py:72-95) and not by calling the package:

    x  = BatchNormalization(inputs)  over the embedding axis, inference mode: (x - moving_mean) / sqrt(moving_var + 1e-3) * gamma + beta
    x  = inputs + MultiHeadAttention(x, x):  softmax(q k^T / sqrt(d)) v per head, biased q / k / v / out projections
    x  = LayerNormalization(x), eps 1e-3, biased variance
    out = inputs + Dense(gelu(Dense(x))):  the exact-erf gelu; the second residual adds the block INPUT (layers.py:94)

* float64 NumPy: :func:`dense_ref`, :func:`layer_norm_ref`, :func:`bn_eval_ref`, :func:`attention_ref`, :func:`block` (dtype float64).
* :func:`split_linear` - a NumPy restatement of the GEMM kernel's arithmetic with tests/conv3x3_ref.py's `scale_exp`, `cut_weight` and
  `cut_act` in chunks of 32; :func:`layer_norm_walk` - the LayerNorm kernel's order in float32; :func:`block` with `restated=True` - the
  block on these.  `defect=` plants one wrong reading, for the test that the bar can tell each of them.
* the torch functions the passes replace, in a dtype of choice: the float32 CPU run is the yardstick e32, the float64 run checks the
  references."""
import math

import numpy as np

from tests.conv3x3_ref import BAR, cut_act, cut_weight, errors, rel_l2, scale_exp, worst  # noqa: F401

CHUNK = 32
ROW_TILE, COUT_TILE = 32, 64            # csrc/token_linear.hip: kTlRows, kTlCout
LN_LANES = 64                           # csrc/mvnerf_vit.h: kVitLnLanes
LN_EPS = BN_EPS = 1e-3                  # Keras defaults
MAX_TOKENS = 256                        # csrc/attention.hip: kAtMaxKeys

_erf = np.vectorize(math.erf, otypes=[np.float64])
_tanh_gelu = lambda x: 0.5 * x * (1 + np.tanh(np.sqrt(2 / np.pi) * (x + 0.044715 * x ** 3)))


def gelu_ref(x):
    x = np.asarray(x, np.float64)
    return 0.5 * x * (1.0 + _erf(x / np.sqrt(2.0)))


def gelu32(x):
    """mvnerf_vit.h vit_gelu, one float32 rounding per written operation (erf taken in double and rounded)."""
    x = np.asarray(x, np.float32)
    t = x * np.float32(0.70710678118654752440)
    e = np.float32(1) + _erf(t.astype(np.float64)).astype(np.float32)
    return (x * np.float32(0.5)) * e


def dense_ref(x, w, bias=None, act=None, residual=None):
    """x (..., K), w (N, K): the Keras kernel transposed, as torch stores it."""
    y = np.asarray(x, np.float64) @ np.asarray(w, np.float64).T
    if bias is not None:
        y = y + np.asarray(bias, np.float64)
    if act == 'gelu':
        y = gelu_ref(y)
    if residual is not None:
        y = y + np.asarray(residual, np.float64)
    return y


def layer_norm_ref(x, gamma, beta, eps=LN_EPS, unbiased=False):
    x = np.asarray(x, np.float64)
    mean = x.mean(-1, keepdims=True)
    var = ((x - mean) ** 2).sum(-1, keepdims=True) / (x.shape[-1] - (1 if unbiased else 0))
    return (x - mean) / np.sqrt(var + eps) * np.asarray(gamma, np.float64) + np.asarray(beta, np.float64)


def bn_eval_ref(x, gamma, beta, mean, var, eps=BN_EPS):
    x, gamma, beta, mean, var = (np.asarray(t, np.float64) for t in (x, gamma, beta, mean, var))
    return (x - mean) / np.sqrt(var + eps) * gamma + beta


def attention_ref(qkv, scale=None, softmax_axis=-1):
    """qkv (B, n, 3, heads, d) -> (B, n, heads d)."""
    qkv = np.asarray(qkv, np.float64)
    b, n, _, h, d = qkv.shape
    q, k, v = (qkv[:, :, i].transpose(0, 2, 1, 3) for i in range(3))                # (B, heads, n, d)
    s = q @ k.transpose(0, 1, 3, 2) * (d ** -0.5 if scale is None else scale)
    s = s - s.max(softmax_axis, keepdims=True)
    p = np.exp(s)
    p = p / p.sum(softmax_axis, keepdims=True)
    return (p @ v).transpose(0, 2, 1, 3).reshape(b, n, h * d)


# ---- the kernels' arithmetic ------------------------------------------------------------------------------------------------------------
def split_linear(x, w, bias=None, act=None, residual=None, amax_x=None, defect=None):
    """mvnerf_linear_tokens in NumPy -> float32 (..., N).  The three products of one chunk of 32 are summed in float64 (exact for fp16
    factors) and rounded into the fp32 accumulator; the MFMA truncates inside that sum, so the kernel sits a little above this."""
    x, w = np.asarray(x, np.float32), np.asarray(w, np.float32)
    lead, k = x.shape[:-1], x.shape[-1]
    x = x.reshape(-1, k)
    ex = scale_exp(np.abs(x).max() if amax_x is None else amax_x)
    ew = scale_exp(np.abs(w).max())
    a0, a1, a0s = (p.astype(np.float64) for p in cut_weight(w, ew))
    b0, b1 = (p.astype(np.float64) for p in cut_act(x, ex))
    acc = np.zeros((x.shape[0], w.shape[0]), np.float32)
    for c in range(0, k, CHUNK):
        ks = slice(c, c + CHUNK)
        s = b0[:, ks] @ a0[:, ks].T + b1[:, ks] @ a0s[:, ks].T
        if defect != 'drop_a1_b0':
            s = s + b0[:, ks] @ a1[:, ks].T
        acc = (acc.astype(np.float64) + s).astype(np.float32)
    y = np.ldexp(acc, -((0 if defect == 'weight_scale_kept' else ew) + ex)).astype(np.float32)
    if bias is not None:
        y = y + np.asarray(bias, np.float32)
    if act == 'gelu':
        y = gelu32(y)
    y = y.reshape(*lead, -1)
    return y if residual is None else y + np.asarray(residual, np.float32)


def _walk_sum(terms):
    """(rows, C) float32 terms -> the row sums in the LayerNorm kernel's order: lane l of 64 adds the elements of its quads l, l + 64, ...
    in order, then an xor butterfly over the lanes."""
    rows, c = terms.shape
    quads = c // 4
    lanes = np.zeros((rows, LN_LANES), np.float32)
    for first in range(0, quads, LN_LANES):
        live = min(LN_LANES, quads - first)
        for e in range(4):
            lanes[:, :live] = lanes[:, :live] + terms[:, 4 * first + e:4 * (first + live):4]
    idx = np.arange(LN_LANES)
    for bit in range(6):
        lanes = lanes + lanes[:, idx ^ (1 << bit)]
    return lanes[:, :1]


def layer_norm_walk(x, gamma, beta, eps=LN_EPS):
    """mvnerf_layer_norm_tokens in NumPy, float32, bit for bit."""
    x = np.asarray(x, np.float32)
    lead, c = x.shape[:-1], x.shape[-1]
    x = x.reshape(-1, c)
    ref = x[:, :1]
    mean = ref + _walk_sum(x - ref) / np.float32(c)
    d = x - mean
    var = _walk_sum(d * d) / np.float32(c)
    rstd = np.float32(1) / np.sqrt(var + np.float32(eps))
    out = ((x - mean) * rstd) * np.asarray(gamma, np.float32) + np.asarray(beta, np.float32)
    return out.reshape(*lead, c)


# ---- the block --------------------------------------------------------------------------------------------------------------------------
BLOCK_DEFECTS = ['tanh_gelu', 'scale_1_over_d', 'softmax_over_queries', 'unbiased_ln_variance', 'eps_dropped', 'second_residual_adds_x',
                 'batch_statistics', 'v_bias_dropped', 'drop_a1_b0', 'weight_scale_kept']


def block_params(embed, heads, mlp_ratio=4, seed=0):
    """Seeded parameters of one block away from Keras' initial values: Glorot-uniform kernels in torch's (out, in) layout, biases of
    0.2 sigma, gamma 1 + 0.3 sigma, beta 0.3 sigma, moving mean 0.3 sigma, moving variance in [0.5, 1.5]; float32."""
    rng = np.random.default_rng([seed, embed, heads])
    f = lambda a: a.astype(np.float32)

    def dense(k, n):
        lim = np.sqrt(6.0 / (k + n))
        return f(rng.uniform(-lim, lim, (n, k))), f(0.2 * rng.standard_normal(n))
    p = {'heads': heads}
    p['bn_gamma'], p['bn_beta'] = f(1 + 0.3 * rng.standard_normal(embed)), f(0.3 * rng.standard_normal(embed))
    p['bn_mean'], p['bn_var'] = f(0.3 * rng.standard_normal(embed)), f(rng.uniform(0.5, 1.5, embed))
    for name in 'qkvo':
        p['w' + name], p['b' + name] = dense(embed, embed)
    p['ln_gamma'], p['ln_beta'] = f(1 + 0.3 * rng.standard_normal(embed)), f(0.3 * rng.standard_normal(embed))
    p['w0'], p['b0'] = dense(embed, embed * mlp_ratio)
    p['w1'], p['b1'] = dense(embed * mlp_ratio, embed)
    return p


def block(inputs, p, restated=False, defect=None):
    """One TransformerBlock on (B, n, embed): float64 from the formulas, or (`restated`) float32 on the kernels' arithmetic - the GEMMs
    through :func:`split_linear` with every amax the maximum of the tensor, the LayerNorm through :func:`layer_norm_walk`."""
    dt = np.float32 if restated else np.float64
    inputs = np.asarray(inputs, dt)
    b, n, e = inputs.shape
    h = p['heads']
    d = e // h
    g = lambda name: np.asarray(p[name], dt)
    gemm_defect = defect if defect in ('drop_a1_b0', 'weight_scale_kept') else None
    lin = (lambda x, w, bias, **kw: split_linear(x, w, bias, defect=gemm_defect, **kw)) if restated else dense_ref
    if defect == 'batch_statistics':
        mean, var = inputs.mean((0, 1)), inputs.var((0, 1))
    else:
        mean, var = g('bn_mean'), g('bn_var')
    x = (((inputs - mean) * (1 / np.sqrt(var.astype(np.float64) + BN_EPS)).astype(dt)) * g('bn_gamma') + g('bn_beta')).astype(dt)
    bv = np.zeros_like(p['bv']) if defect == 'v_bias_dropped' else p['bv']
    qkv = lin(x, np.concatenate([p['wq'], p['wk'], p['wv']], 0), np.concatenate([p['bq'], p['bk'], bv], 0)).reshape(b, n, 3, h, d)
    att = attention_ref(qkv, 1.0 / d if defect == 'scale_1_over_d' else None, -2 if defect == 'softmax_over_queries' else -1).astype(dt)
    x = lin(att, p['wo'], p['bo'], residual=inputs)
    eps = 0.0 if defect == 'eps_dropped' else LN_EPS
    if restated and defect != 'unbiased_ln_variance':
        x = layer_norm_walk(x, p['ln_gamma'], p['ln_beta'], eps)
    else:
        x = layer_norm_ref(x, p['ln_gamma'], p['ln_beta'], eps, unbiased=defect == 'unbiased_ln_variance').astype(dt)
    if defect == 'tanh_gelu':
        hidden = _tanh_gelu(lin(x, p['w0'], p['b0']).astype(np.float64)).astype(dt)
    else:
        hidden = lin(x, p['w0'], p['b0'], act='gelu')
    return lin(hidden, p['w1'], p['b1'], residual=x if defect == 'second_residual_adds_x' else inputs)


def load_block(blk, p):
    """The parameters of :func:`block_params` into an encoders.TransformerBlock, in place."""
    import torch
    t = lambda name: torch.from_numpy(p[name])
    with torch.no_grad():
        bn = blk.layer_norm_1
        bn.weight.copy_(t('bn_gamma')), bn.bias.copy_(t('bn_beta')), bn.running_mean.copy_(t('bn_mean')), bn.running_var.copy_(t('bn_var'))
        for name, lin in (('q', blk.attention.q), ('k', blk.attention.k), ('v', blk.attention.v), ('o', blk.attention.o),
                          ('0', blk.dense_0), ('1', blk.dense_1)):
            lin.weight.copy_(t('w' + name)), lin.bias.copy_(t('b' + name))
        blk.layer_norm_2.weight.copy_(t('ln_gamma')), blk.layer_norm_2.bias.copy_(t('ln_beta'))
    return blk


# ---- the torch functions the passes replace, on the CPU in `dtype` ------------------------------------------------------------------------
def _t(a, dtype):
    import torch
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dtype)


def torch_linear(x, w, bias, act, residual, dtype):
    import torch.nn.functional as F
    y = F.linear(_t(x, dtype), _t(w, dtype), _t(bias, dtype))
    if act == 'gelu':
        y = F.gelu(y)
    if residual is not None:
        y = y + _t(residual, dtype)
    return y.numpy()


def torch_layer_norm(x, gamma, beta, eps, dtype):
    import torch.nn.functional as F
    return F.layer_norm(_t(x, dtype), (x.shape[-1],), _t(gamma, dtype), _t(beta, dtype), eps).numpy()


def torch_attention(qkv, dtype, scale=None):
    import torch.nn.functional as F
    b, n, _, h, d = qkv.shape
    q, k, v = (_t(qkv[:, :, i], dtype).transpose(1, 2) for i in range(3))
    return F.scaled_dot_product_attention(q, k, v, scale=scale).transpose(1, 2).reshape(b, n, h * d).numpy()


def linear_inputs(m, k, n, seed=0):
    """Seeded unit-normal x (m, k), Glorot-uniform w (n, k), bias, residual (m, n); float32."""
    rng = np.random.default_rng([seed, m, k, n])
    lim = np.sqrt(6.0 / (k + n))
    f = lambda a: a.astype(np.float32)
    return f(rng.standard_normal((m, k))), f(rng.uniform(-lim, lim, (n, k))), f(0.2 * rng.standard_normal(n)), f(rng.standard_normal((m, n)))
