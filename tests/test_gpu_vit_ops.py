"""ops.linear / ops.layer_norm / ops.attention (csrc/token_linear.hip, csrc/attention.hip) on the GPU against the float64 references of
tests/vit_ref.py.  The bar is e64 <= 8 e32, relative L2 and worst element, e32 being torch's float32 CPU run of the same case.  Every
output lies NaN-filled between NaN guard rows that must stay NaN, every case runs twice and must repeat bit for bit.  Shapes: the row
tile is 32 and the channel tile 64, so 37 = one tile + 5 rows, 69 = two tiles + 5, 133 = four tiles + 5; K = 160 ends on a short slab
(128 + 32), K = 3072 is the reference's longest; attention runs 16 keys per block and 64 queries per workgroup, so n = 5, 70, 197, 256."""
import numpy as np
import pytest
import torch

from tests import vit_ref as V
from thesis_clip_nerf_amd import ops

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
GUARD = 3
LINEAR_SHAPES = [(1, 32, 64), (37, 96, 128), (69, 64, 64), (133, 160, 192), (5, 3072, 64)]
EPILOGUES = [None, 'gelu', 'residual']


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def guarded(rows, cols):
    """-> (buffer, view): `rows` NaN rows of `cols` between GUARD NaN rows on each side."""
    buf = torch.full((rows + 2 * GUARD, cols), float('nan'), dtype=torch.float32, device=DEV)
    return buf, buf[GUARD:GUARD + rows]


def twice(run, rows, cols):
    """Runs `run(out)` into two guarded buffers -> the output as an array; the guards stay NaN, the runs agree bit for bit."""
    outs = []
    for _ in range(2):
        buf, out = guarded(rows, cols)
        run(out)
        assert torch.isnan(buf[:GUARD]).all() and torch.isnan(buf[GUARD + rows:]).all()
        outs.append(out)
    assert torch.equal(outs[0].view(torch.int32), outs[1].view(torch.int32))            # (the bits: a NaN fill repeats too)
    return outs[0]


def assert_bar(got, ref, e32, what):
    e64 = V.errors(got, ref)
    print(f'{what}: rel L2 {e64[0]:.3g} = {e64[0] / e32[0]:.2f} x e32, worst {e64[1]:.3g} = {e64[1] / e32[1]:.2f} x e32')
    assert e64[0] <= V.BAR * e32[0] and e64[1] <= V.BAR * e32[1], (what, e64, e32)


def run_linear(x, w, bias, act, res, amax_x=None, amax_out=None):
    packed = ops.linear_pack(dev(w))
    xd, bd, rd = dev(x), dev(bias), dev(res)
    return twice(lambda out: ops.linear(xd, packed, w.shape[0], bias=bd, act=act, residual=rd, amax_x=amax_x, out=out, amax_out=amax_out),
                 x.shape[0], w.shape[0])


# ---- linear -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('epi', EPILOGUES, ids=str)
@pytest.mark.parametrize('shape', LINEAR_SHAPES, ids=str)
def test_linear_against_float64(shape, epi):
    x, w, bias, res = V.linear_inputs(*shape)
    act, res = ('gelu' if epi == 'gelu' else None), (res if epi == 'residual' else None)
    ref = V.dense_ref(x, w, bias, act, res)
    e32 = V.errors(V.torch_linear(x, w, bias, act, res, torch.float32), ref)
    top = torch.empty(1, device=DEV)
    got = run_linear(x, w, bias, act, res, amax_out=top)
    assert torch.isfinite(got).all() and float(top) == float(got.abs().max())
    assert_bar(got.cpu().numpy(), ref, e32, f'linear {shape} {epi}')


def test_linear_with_one_element_far_above_the_rest():
    x, w, bias, res = V.linear_inputs(37, 96, 128, seed=1)
    x[11, 40] = np.float32(2.0 ** 10) * np.abs(x).max()
    ref = V.dense_ref(x, w, bias)
    e32 = V.errors(V.torch_linear(x, w, bias, None, None, torch.float32), ref)
    assert_bar(run_linear(x, w, bias, None, None).cpu().numpy(), ref, e32, 'linear, one element at 2^10')


def test_linear_exact_properties():
    m, k, n = 37, 96, 128
    x, w, bias, res = V.linear_inputs(m, k, n, seed=2)
    # a one-hot row times weights of 11 significant bits: that weight column, bit for bit
    w11 = w.astype(np.float16).astype(np.float32)
    hot = np.zeros((m, k), np.float32)
    cols = (np.arange(m) * 7) % k
    hot[np.arange(m), cols] = 1.0
    assert np.array_equal(run_linear(hot, w11, None, None, None).cpu().numpy(), w11[:, cols].T)
    # x -> 2^k x without a bias scales out, bit for bit
    base = run_linear(x, w, None, None, None)
    for p in (5, -3):
        assert torch.equal(run_linear(x * np.float32(2.0 ** p), w, None, None, None), base * 2.0 ** p)
    # a zero bound is an all-zero source: epi(bias); a NaN bound poisons the output and its maximum
    zero, top = torch.zeros(1, device=DEV), torch.empty(1, device=DEV)
    nothing = np.zeros_like(x)
    assert np.array_equal(run_linear(nothing, w, bias, None, None, amax_x=zero).cpu().numpy(), np.broadcast_to(bias, (m, n)))
    assert np.array_equal(run_linear(nothing, w, bias, None, res, amax_x=zero).cpu().numpy(), bias + res)
    assert V.worst(run_linear(nothing, w, bias, 'gelu', None, amax_x=zero).cpu().numpy(), np.broadcast_to(V.gelu_ref(bias), (m, n))) < 1e-6
    bad = torch.full((1,), float('nan'), device=DEV)
    assert torch.isnan(run_linear(x, w, bias, None, None, amax_x=bad, amax_out=top)).all() and torch.isnan(top).all()


def test_linear_tail_rows_are_predicated():
    """Rows 0..36 of the M = 133 run equal the M = 37 run on the same rows under the same amax word."""
    x, w, bias, res = V.linear_inputs(133, 160, 192)
    amax = ops.absmax(dev(x))
    full = run_linear(x, w, bias, 'gelu', None, amax_x=amax)
    part = run_linear(x[:37], w, bias, 'gelu', None, amax_x=amax)
    assert torch.equal(full[:37], part)


# ---- layer_norm ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('offset', [0.0, 1e3], ids=['centred', 'mean_1e3_sigma'])
@pytest.mark.parametrize('shape', [(1, 32), (5, 64), (70, 768)], ids=str)
def test_layer_norm_against_float64(shape, offset):
    rng = np.random.default_rng([7, *shape])
    x = (rng.standard_normal(shape) + offset).astype(np.float32)
    gamma, beta = ((1 + 0.3 * rng.standard_normal(shape[1])).astype(np.float32), (0.3 * rng.standard_normal(shape[1])).astype(np.float32))
    ref = V.layer_norm_ref(x, gamma, beta)
    e32 = V.errors(V.torch_layer_norm(x, gamma, beta, V.LN_EPS, torch.float32), ref)
    xd, gd, bd, top = dev(x), dev(gamma), dev(beta), torch.empty(1, device=DEV)
    got = twice(lambda out: ops.layer_norm(xd, gd, bd, V.LN_EPS, out=out, amax_out=top), *shape)
    assert float(top) == float(got.abs().max())
    assert_bar(got.cpu().numpy(), ref, e32, f'layer_norm {shape} offset {offset}')
    assert np.array_equal(got.cpu().numpy(), V.layer_norm_walk(x, gamma, beta))          # the stated order, bit for bit
    inplace = xd.clone()
    assert ops.layer_norm(inplace, gd, bd, V.LN_EPS, out=inplace) is inplace and torch.equal(inplace, got)
    const = torch.full(shape, 3.7, device=DEV)
    assert torch.equal(ops.layer_norm(const, gd, bd, V.LN_EPS), bd.expand(shape))      # a constant row gives beta


# ---- attention ----------------------------------------------------------------------------------------------------------------------------
def run_attention(qkv, amax_out=None):
    """qkv (B, n, 3, heads, d) array, on the device followed by NaN guard tokens: an unmasked padded key would show."""
    b, n, _, h, d = qkv.shape
    buf = torch.full((b * n + 16, 3 * h * d), float('nan'), dtype=torch.float32, device=DEV)
    buf[:b * n] = dev(qkv.reshape(b * n, 3 * h * d))
    view = buf[:b * n].view(b, n, 3, h, d)
    return twice(lambda out: ops.attention(view, out=out.view(b, n, h * d), amax_out=amax_out), b * n, h * d).view(b, n, h * d)


@pytest.mark.parametrize('logits', [None, 60.0], ids=['unit', 'logits_60'])
@pytest.mark.parametrize('shape', [(2, 4, 5, 16), (1, 2, 70, 32), (1, 3, 197, 64), (1, 1, 256, 64)], ids=str)
def test_attention_against_float64(shape, logits):
    b, h, n, d = shape
    qkv = np.random.default_rng([8, *shape]).standard_normal((b, n, 3, h, d)).astype(np.float32)
    if logits:
        s = np.einsum('bihd,bjhd->bhij', qkv[:, :, 0].astype(np.float64), qkv[:, :, 1].astype(np.float64)) * d ** -0.5
        qkv[:, :, :2] *= np.float32(np.sqrt(logits / np.abs(s).max()))
    ref = V.attention_ref(qkv)
    e32 = V.errors(V.torch_attention(qkv, torch.float32), ref)
    top = torch.empty(1, device=DEV)
    got = run_attention(qkv, top)
    assert torch.isfinite(got).all() and float(top) == float(got.abs().max())
    assert_bar(got.cpu().numpy(), ref, e32, f'attention {shape} logits {logits}')


def test_attention_exact_properties():
    rng = np.random.default_rng(9)
    one = rng.standard_normal((1, 1, 3, 1, 16)).astype(np.float32)                  # one token: the softmax is 1, out == v
    assert np.array_equal(run_attention(one).cpu().numpy(), one[:, :, 2].reshape(1, 1, 16))
    n, j = 37, 21                                                                   # one dominant key: logit gap 32 * 32 / 4 = 256
    qkv = np.zeros((1, n, 3, 1, 16), np.float32)
    qkv[:, :, 0, 0, 0] = 32.0
    qkv[:, j, 1, 0, 0] = 32.0
    qkv[:, :, 2] = rng.standard_normal((1, n, 1, 16))
    assert np.array_equal(run_attention(qkv).cpu().numpy(), np.broadcast_to(qkv[:, j, 2], (1, n, 16)))


def test_wrappers_reject_what_the_kernels_do_not_take():
    x = torch.zeros(4, 32, device=DEV)
    packed = ops.linear_pack(torch.zeros(64, 32, device=DEV))
    with pytest.raises(ValueError, match='shape'):
        ops.linear(torch.zeros(4, 64, device=DEV), ops.linear_pack(torch.zeros(64, 64, device=DEV)), 128)
    with pytest.raises(ValueError, match='do not go together'):
        ops.linear(x, packed, 64, act='gelu', residual=torch.zeros(4, 64, device=DEV))
    with pytest.raises(ValueError, match='multiple of 32'):
        ops.linear_pack(torch.zeros(64, 40, device=DEV))
    with pytest.raises(ValueError, match='multiple of 4'):
        ops.layer_norm(torch.zeros(4, 30, device=DEV), torch.zeros(30, device=DEV), torch.zeros(30, device=DEV))
    with pytest.raises(ValueError, match='head dimension'):
        ops.attention(torch.zeros(1, 5, 3, 4, 8, device=DEV))
    with pytest.raises(ValueError, match='at most 256'):
        ops.attention(torch.zeros(1, 257, 3, 1, 16, device=DEV))
