"""The transformer-block passes without a GPU: the float64 references of tests/vit_ref.py against the torch modules in double; the host
build of csrc/mvnerf_vit.h (tests/cpu_vit) bit for bit against the NumPy restatement where that is defined (the operand cut, the
LayerNorm walk, the epilogue's additions) and at the GPU tests' bar e64 <= 8 e32 otherwise (gelu, a softmax row), e32 being torch's
float32 CPU run of the same case; the restated GEMM and the restated block at that bar; planted defects against the same assertion; the
argument checks of the new entry points and wrappers; the module switches.  The kernels themselves are tests/test_gpu_vit_ops.py and
tests/test_gpu_fused_vit.py."""
import copy
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import vit_ref as V
from thesis_clip_nerf_amd import _lib
from thesis_clip_nerf_amd import encoders as E
from thesis_clip_nerf_amd import ops

HERE = os.path.dirname(os.path.abspath(__file__))
LINEAR_SHAPES = [(1, 32, 64), (37, 96, 128), (133, 160, 192), (5, 3072, 64)]
EPILOGUES = [None, 'gelu', 'residual']
TINY_VIT = dict(transformer_image_size=(32, 32), patch_size=16, embed_dim=32, num_heads=4, hooks=(1, 2, 3, 4), features=(32, 64, 96, 128))


@pytest.fixture(scope='module')
def cpu():
    d = os.path.join(HERE, 'cpu_vit')
    subprocess.run(['make', '-C', d], check=True, capture_output=True)
    lib = ctypes.CDLL(os.path.join(d, 'libmvnerf_vit_cpu.so'))
    p, i, n = ctypes.c_void_p, ctypes.c_int, ctypes.c_long
    lib.vit_cpu_scale_exp.argtypes = [ctypes.c_float]
    lib.vit_cpu_cut_act.argtypes = [p, n, i, p, p]
    lib.vit_cpu_cut_weight.argtypes = [p, n, i, p, p, p]
    lib.vit_cpu_gelu.argtypes = [p, n, p]
    lib.vit_cpu_linear_epi.argtypes = [p, p, p, n, i, i, p]
    lib.vit_cpu_layer_norm.argtypes = [p, p, p, n, i, ctypes.c_float, p]
    lib.vit_cpu_softmax_row.argtypes = [p, i, p]
    return lib


def ptr(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def meets_bar(got, ref, e32):
    e64 = V.errors(got, ref)
    return e64[0] <= V.BAR * e32[0] and e64[1] <= V.BAR * e32[1]


# ---- the references against torch in double ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('epi', EPILOGUES, ids=str)
@pytest.mark.parametrize('shape', LINEAR_SHAPES[:3], ids=str)
def test_dense_reference_against_float64_torch(shape, epi):
    x, w, bias, res = V.linear_inputs(*shape)
    act, res = ('gelu' if epi == 'gelu' else None), (res if epi == 'residual' else None)
    assert V.worst(V.torch_linear(x, w, bias, act, res, torch.float64), V.dense_ref(x, w, bias, act, res)) <= 1e-12


def test_norm_and_attention_references_against_float64_torch():
    rng = np.random.default_rng(3)
    x = rng.standard_normal((5, 7, 64))
    gamma, beta, mean, var = rng.standard_normal(64), rng.standard_normal(64), rng.standard_normal(64), rng.uniform(0.5, 1.5, 64)
    assert V.worst(V.torch_layer_norm(x, gamma, beta, V.LN_EPS, torch.float64), V.layer_norm_ref(x, gamma, beta)) <= 1e-12
    t = lambda a: torch.from_numpy(a)
    bn = F.batch_norm(t(x).transpose(1, 2), t(mean), t(var), t(gamma), t(beta), False, 0.0, V.BN_EPS).transpose(1, 2).numpy()
    assert V.worst(bn, V.bn_eval_ref(x, gamma, beta, mean, var)) <= 1e-12
    qkv = rng.standard_normal((2, 37, 3, 4, 16))
    assert V.worst(V.torch_attention(qkv, torch.float64), V.attention_ref(qkv)) <= 1e-12


@pytest.mark.parametrize('embed,heads,tokens', [(64, 4, 36), (128, 2, 19)], ids=str)
def test_block_reference_against_the_float64_module(embed, heads, tokens):
    p = V.block_params(embed, heads)
    x = np.random.default_rng(5).standard_normal((2, tokens, embed))
    blk = V.load_block(E.TransformerBlock(heads, embed), p).double().eval()
    with torch.no_grad():
        got = blk(torch.from_numpy(x)).numpy()
    assert V.worst(got, V.block(x, p)) <= 1e-12


# ---- the host build, bit for bit --------------------------------------------------------------------------------------------------------
def test_host_cut_is_the_numpy_cut(cpu):
    rng = np.random.default_rng(1)
    x = (rng.standard_normal(4096) * np.exp(rng.uniform(-12, 0, 4096))).astype(np.float32)
    x[:4] = [0.0, -0.0, 1.0, -1.0]
    tiny = (x * np.float32(1e-30) * np.float32(1e-9)).astype(np.float32)           # the maximum is a subnormal number
    assert 0 < np.abs(tiny).max() < np.finfo(np.float32).tiny
    for v, amax in ((x, float(np.abs(x).max())), (x, 7e4), (tiny, float(np.abs(tiny).max()))):      # upper bounds: nothing overflows
        e = V.scale_exp(amax)
        assert cpu.vit_cpu_scale_exp(amax) == e
        b0, b1 = np.zeros(v.size, np.uint16), np.zeros(v.size, np.uint16)
        cpu.vit_cpu_cut_act(ptr(v), v.size, e, ptr(b0), ptr(b1))
        r0, r1 = V.cut_act(v, e)
        assert np.array_equal(b0, r0.view(np.uint16)) and np.array_equal(b1, r1.view(np.uint16))
        a = [np.zeros(v.size, np.uint16) for _ in range(3)]
        cpu.vit_cpu_cut_weight(ptr(v), v.size, e, *map(ptr, a))
        for got, want in zip(a, V.cut_weight(v, e)):
            assert np.array_equal(got, want.view(np.uint16))


@pytest.mark.parametrize('shape', [(1, 32), (5, 64), (70, 768), (3, 260)], ids=str)
def test_host_layer_norm_is_the_numpy_walk(cpu, shape):
    rng = np.random.default_rng([2, *shape])
    x = rng.standard_normal(shape).astype(np.float32)
    gamma, beta = (rng.standard_normal(shape[1]).astype(np.float32) for _ in range(2))
    out = np.full_like(x, np.nan)
    cpu.vit_cpu_layer_norm(ptr(x), ptr(gamma), ptr(beta), shape[0], shape[1], V.LN_EPS, ptr(out))
    assert np.array_equal(out, V.layer_norm_walk(x, gamma, beta))
    const = np.full(shape, np.float32(3.7))
    cpu.vit_cpu_layer_norm(ptr(const), ptr(gamma), ptr(beta), shape[0], shape[1], V.LN_EPS, ptr(out))
    assert np.array_equal(out, np.broadcast_to(beta, shape))                       # a constant row gives beta


def test_host_epilogue_adds_in_the_stated_order(cpu):
    s, w, bias, res = V.linear_inputs(9, 32, 64)
    s = res * np.float32(3)
    out = np.full_like(s, np.nan)
    cpu.vit_cpu_linear_epi(ptr(s), ptr(bias), None, 9, 64, 0, ptr(out))
    assert np.array_equal(out, s + bias)
    cpu.vit_cpu_linear_epi(ptr(s), ptr(bias), ptr(res), 9, 64, 2, ptr(out))
    assert np.array_equal(out, (s + bias) + res)
    cpu.vit_cpu_linear_epi(ptr(s), None, None, 9, 64, 0, ptr(out))
    assert np.array_equal(out, s)


# ---- the host build at the bar ----------------------------------------------------------------------------------------------------------
def test_host_gelu_meets_the_bar(cpu):
    x = np.concatenate([np.linspace(-9, 9, 4001), np.random.default_rng(0).standard_normal(4000) * 3]).astype(np.float32)
    out = np.full_like(x, np.nan)
    cpu.vit_cpu_gelu(ptr(x), x.size, ptr(out))
    ref = V.gelu_ref(x)
    e32 = V.errors(F.gelu(torch.from_numpy(x)).numpy(), ref)
    assert meets_bar(out, ref, e32), (V.errors(out, ref), e32)
    assert meets_bar(V.gelu32(x), ref, e32)
    assert not meets_bar(V._tanh_gelu(x.astype(np.float64)), ref, e32)


@pytest.mark.parametrize('n,spread', [(1, 1.0), (5, 1.0), (197, 3.0), (256, 60.0)], ids=str)
def test_host_softmax_row_meets_the_bar(cpu, n, spread):
    rng = np.random.default_rng([4, n])
    rows = (rng.standard_normal((8, n)) * spread).astype(np.float32)
    out = np.full_like(rows, np.nan)
    for r in range(rows.shape[0]):
        cpu.vit_cpu_softmax_row(ptr(rows[r]), n, ptr(out[r]))
    s = rows.astype(np.float64)
    ref = np.exp(s - s.max(-1, keepdims=True))
    ref /= ref.sum(-1, keepdims=True)
    e32 = V.errors(torch.softmax(torch.from_numpy(rows), -1).numpy(), ref)
    if n == 1:
        assert np.array_equal(out, np.ones_like(out))
    else:
        assert meets_bar(out, ref, e32), (V.errors(out, ref), e32)


# ---- the restated arithmetic at the bar, and what the bar can tell -------------------------------------------------------------------------
@pytest.mark.parametrize('epi', EPILOGUES, ids=str)
@pytest.mark.parametrize('shape', LINEAR_SHAPES, ids=str)
def test_restated_gemm_meets_the_bar(shape, epi):
    x, w, bias, res = V.linear_inputs(*shape)
    act, res = ('gelu' if epi == 'gelu' else None), (res if epi == 'residual' else None)
    ref = V.dense_ref(x, w, bias, act, res)
    e32 = V.errors(V.torch_linear(x, w, bias, act, res, torch.float32), ref)
    got = V.split_linear(x, w, bias, act, res)
    print(shape, epi, [g / e for g, e in zip(V.errors(got, ref), e32)])
    assert meets_bar(got, ref, e32)
    for defect in ('drop_a1_b0', 'weight_scale_kept'):
        assert not meets_bar(V.split_linear(x, w, bias, act, res, defect=defect), ref, e32), defect


@pytest.fixture(scope='module')
def block_case():
    p = V.block_params(64, 4)
    x = np.random.default_rng(6).standard_normal((2, 36, 64)).astype(np.float32)
    ref = V.block(x, p)
    blk = V.load_block(E.TransformerBlock(4, 64), p).eval()
    with torch.no_grad():
        e32 = V.errors(blk(torch.from_numpy(x)).numpy(), ref)
    return p, x, ref, e32


def test_restated_block_meets_the_bar(block_case):
    p, x, ref, e32 = block_case
    got = V.block(x, p, restated=True)
    print([g / e for g, e in zip(V.errors(got, ref), e32)])
    assert got.dtype == np.float32 and meets_bar(got, ref, e32), (V.errors(got, ref), e32)


@pytest.mark.parametrize('defect', V.BLOCK_DEFECTS)
def test_the_bar_tells_a_planted_defect(block_case, defect):
    p, x, ref, e32 = block_case
    assert not meets_bar(V.block(x, p, restated=True, defect=defect), ref, e32), defect


# ---- argument checks ----------------------------------------------------------------------------------------------------------------------
def test_entry_points_check_their_arguments_before_any_launch():
    lib = _lib.lib()
    one, odd = ctypes.c_void_p(16), ctypes.c_void_p(20)
    assert lib.mvnerf_linear_packed_bytes(768, 2304) == 256 + (2304 // 16) * (768 // 32) * 3 * 1024
    assert lib.mvnerf_linear_packed_bytes(48, 64) == 0 and lib.mvnerf_linear_packed_bytes(32, 96) == 0
    assert lib.mvnerf_linear_pack(None, 32, 64, one, None) == -1
    assert lib.mvnerf_linear_pack(one, 40, 64, one, None) == -2
    assert lib.mvnerf_linear_pack(one, 32, 64, odd, None) == -3
    lin = lambda x=one, amax=one, packed=one, bias=None, res=None, m=5, k=32, n=64, epi=0, out=one, top=None: \
        lib.mvnerf_linear_tokens(x, amax, packed, bias, res, m, k, n, epi, out, top, None)
    assert lin(x=None) == -1 and lin(amax=None) == -1 and lin(m=0) == -1
    assert lin(epi=2) == -1 and b'residual' in lib.mvnerf_last_error()
    assert lin(res=one, epi=1) == -1
    assert lin(k=48) == -2 and lin(n=96) == -2 and lin(epi=3) == -2
    assert lin(x=odd) == -3 and lin(bias=odd) == -3 and lin(out=odd) == -3 and lin(amax=ctypes.c_void_p(18)) == -3
    ln = lambda x=one, g=one, b=one, m=3, c=64, eps=1e-3, out=one: lib.mvnerf_layer_norm_tokens(x, g, b, m, c, eps, out, None, None)
    assert ln(g=None) == -1 and ln(m=0) == -1 and ln(eps=-1.0) == -1
    assert ln(c=66) == -2 and ln(out=odd) == -3
    at = lambda qkv=one, b=1, n=197, h=12, d=64, scale=0.125, out=one: lib.mvnerf_attention_tokens(qkv, b, n, h, d, scale, out, None, None)
    assert at(qkv=None) == -1 and at(n=0) == -1 and at(scale=float('nan')) == -1
    assert at(d=8) == -2 and at(d=48) == -2 and at(n=257) == -2 and at(out=odd) == -3


def test_wrappers_check_before_any_launch():
    x = torch.zeros(5, 32)
    packed = torch.zeros(256 + 4 * 3 * 1024, dtype=torch.uint8)
    with pytest.raises(ValueError, match='HIP device'):
        ops.linear(x, packed, 64)
    with pytest.raises(ValueError, match='HIP device'):
        ops.linear_pack(torch.zeros(64, 32))
    with pytest.raises(ValueError, match='multiple of 32'):
        ops.linear_packed_bytes(40, 64)
    assert ops.linear_packed_bytes(32, 64) == packed.numel()
    with pytest.raises(ValueError, match='HIP device'):
        ops.layer_norm(x, torch.ones(32), torch.zeros(32))
    with pytest.raises(ValueError, match='HIP device'):
        ops.attention(torch.zeros(1, 5, 3, 2, 16))
    with pytest.raises(ValueError, match='torch.Tensor'):
        ops.attention(None)


# ---- the switches ---------------------------------------------------------------------------------------------------------------------------
def test_fused_vit_defaults_to_off_and_rejects_other_values():
    vf = E.VisualFeatures(256, (32, 48), **TINY_VIT)
    blocks = [b for seq in vf.vision_transformer.vit.transformer_blocks for b in seq]
    assert vf.fused_vit is False and vf.vision_transformer.fused_vit is False and all(b.fused_vit is False for b in blocks)
    vf.fused_vit = 'auto'
    assert vf.vision_transformer.vit.fused_vit == 'auto' and all(b.fused_vit == 'auto' for b in blocks) and vf.fused_conv is False
    for bad in (1, 'on', None):
        with pytest.raises(ValueError, match='fused_vit'):
            vf.fused_vit = bad
        with pytest.raises(ValueError, match='fused_vit'):
            E.TransformerBlock(4, 64, fused_vit=bad)
    prod = E.LanguageFeatureProducer((32, 48), n_features=256, clip_pyramid=E.SyntheticCLIPPyramid((16, 32, 32, 64), (8, 4, 2, 1), 64),
                                     clip_text=E.SyntheticCLIPText(embed_dim=64), fused_vit='auto',
                                     combine_kw=dict(clip_channels=(16, 32, 32, 64), text_dim=64, widths=(64, 32, 32), up3_filters=16), **TINY_VIT)
    assert prod.visual_features.fused_vit == 'auto' and prod.visual_features.fused_conv is False


def test_fused_vit_true_raises_in_training_mode_and_under_gradients_and_auto_runs_torch():
    torch.manual_seed(0)
    blk = E.TransformerBlock(4, 64)
    x = torch.randn(2, 9, 64)
    plain = blk.eval()(x)
    blk.fused_vit = 'auto'                                   # CPU tensors, parameters with gradients: torch, the same bits
    assert torch.equal(blk(x), plain)
    blk.fused_vit = True
    with pytest.raises(RuntimeError, match='no backward'):
        blk(x)
    blk.requires_grad_(False).train()
    with torch.no_grad():
        with pytest.raises(ValueError, match='training mode'):
            blk(x)
        blk.fused_vit = 'auto'
        blk(x)                                               # batch statistics, through torch
        small = E.TransformerBlock(4, 32, fused_vit=True).requires_grad_(False).eval()
        with pytest.raises(ValueError, match='multiples of 64'):
            small(torch.randn(1, 5, 32))
        with pytest.raises(ValueError, match='HIP device'):  # everything fits, but there is no CPU path
            blk.eval()
            blk.fused_vit = True
            blk(x)


def test_loaders_drop_the_packed_caches():
    blk = E.TransformerBlock(4, 64)
    for m in (blk.dense_0, blk.attention, blk.layer_norm_1):
        m.__dict__['_mvnerf_packed'] = ('stale', None)
    p = V.block_params(64, 4)
    E.load_dense(blk.dense_0, p['w0'].T, p['b0'])
    E.load_batchnorm(blk.layer_norm_1, p['bn_gamma'], p['bn_beta'], p['bn_mean'], p['bn_var'])
    k3 = lambda w: w.T.reshape(64, 4, 16)
    E.load_mha(blk.attention, k3(p['wq']), p['bq'].reshape(4, 16), k3(p['wk']), p['bk'].reshape(4, 16), k3(p['wv']), p['bv'].reshape(4, 16),
               p['wo'].T.reshape(4, 16, 64), p['bo'])
    assert all('_mvnerf_packed' not in m.__dict__ for m in (blk.dense_0, blk.attention, blk.layer_norm_1, blk.attention.q))
    assert E._loads(blk.dense_0, blk.attention.q, blk.attention) == (1, 1, 1)
    clone = copy.deepcopy(blk)
    assert E._param_key(clone.dense_0.weight) != E._param_key(blk.dense_0.weight)
