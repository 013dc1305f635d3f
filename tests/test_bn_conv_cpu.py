"""The biased 3x3 convolution with a source activation and the batch-statistics normalisation behind it, without a GPU: the float64
references of tests/bn_ref.py against torch in float64; the host build of csrc/mvnerf_conv.h's statistics (tests/cpu_bn: tile mean and
M2 in the kernel's order, Chan's combine in double, the subtract-first apply) against float64 at the GPU tests' bar e64 <= 8 e32, e32
being torch's float32 CPU F.batch_norm(training=True) on the same case - also where channels have |mean| / sigma = 1e3; the yardstick
itself on that case; planted defects against the same assertion; the argument checks of the new entry points; the module switches.
The kernels themselves are tests/test_gpu_bn_conv.py and tests/test_gpu_fused_visual.py."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

from tests import bn_ref as B
from tests import conv3x3_ref as R
from thesis_clip_nerf_amd import _lib
from thesis_clip_nerf_amd import encoders as E
from thesis_clip_nerf_amd import ops

HERE = os.path.dirname(os.path.abspath(__file__))
TILED = B.SHAPES[1]
TINY_VIT = dict(transformer_image_size=(32, 32), patch_size=16, embed_dim=32, num_heads=4, hooks=(1, 2, 3, 4), features=(32, 64, 96, 128))


@pytest.fixture(scope='module')
def cpu():
    d = os.path.join(HERE, 'cpu_bn')
    subprocess.run(['make', '-C', d], check=True, capture_output=True)
    lib = ctypes.CDLL(os.path.join(d, 'libmvnerf_bn_cpu.so'))
    lib.bn_cpu_finalize.argtypes = [ctypes.c_void_p] + [ctypes.c_int] * 4 + [ctypes.c_double, ctypes.c_void_p, ctypes.c_void_p]
    lib.bn_cpu_apply.argtypes = [ctypes.c_void_p] * 6 + [ctypes.c_long, ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
    lib.bn_cpu_tile_stats.argtypes = [ctypes.c_void_p] + [ctypes.c_int] * 4 + [ctypes.c_void_p]
    lib.bn_cpu_act_in.argtypes = [ctypes.c_void_p, ctypes.c_long, ctypes.c_int, ctypes.c_void_p]
    lib.bn_cpu_bias_act.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_long, ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
    return lib


def ptr(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def host_stats(cpu, y):
    n, h, w, c = y.shape
    tiles = n * -(-h // B.TILE) * -(-w // B.TILE)
    stats = np.full(tiles * (c // 64) * 128, np.nan, np.float32)
    cpu.bn_cpu_tile_stats(ptr(y), n, h, w, c, ptr(stats))
    return stats


def host_bn(cpu, y, gamma, beta, skip, eps=B.EPS, relu=True):
    """tile statistics -> finalize -> apply, all through the host build."""
    y = np.ascontiguousarray(y, np.float32)
    n, h, w, c = y.shape
    stats = host_stats(cpu, y)
    mean, rstd = np.zeros(c, np.float32), np.zeros(c, np.float32)
    cpu.bn_cpu_finalize(ptr(stats), n, h, w, c, eps, ptr(mean), ptr(rstd))
    out = np.full_like(y, np.nan)
    cpu.bn_cpu_apply(ptr(y), ptr(mean), ptr(rstd), ptr(gamma), ptr(beta), ptr(skip), n * h * w, c, int(relu), ptr(out))
    return out, mean, rstd, stats


@pytest.mark.parametrize('shape', B.SHAPES, ids=str)
def test_references_against_float64_torch(shape):
    d = B.inputs(shape)
    for act_in in B.ACT_INS:
        ref = B.conv_bias_ref(d['x'], d['wt'], d['bias'], act_in)
        assert R.worst(B.conv_bias_torch(d['x'], d['wt'], d['bias'], act_in, None, torch.float64), ref) <= 1e-12


@pytest.mark.parametrize('shape', B.BN_SHAPES, ids=str)
def test_pipeline_reference_against_float64_torch(shape):
    d = B.inputs(shape)
    for skip in (False, True):
        ref = B.pipeline_ref(d, skip)
        assert ref.shape == (*shape[:3], shape[4])
        assert R.worst(B.pipeline_torch(d, torch.float64, skip), ref) <= 1e-11


@pytest.mark.parametrize('skip', [False, True], ids=['plain', 'skip'])
@pytest.mark.parametrize('shape', B.BN_SHAPES, ids=str)
def test_host_statistics_and_apply_meet_the_bar(cpu, shape, skip):
    """The normalisation alone, on the float32 convolution output of the case: the same map goes to the host build, to float64 and to
    torch's float32 F.batch_norm(training=True)."""
    d = B.inputs(shape)
    y = B.conv_bias_ref(d['x'], d['wt'], d['bias']).astype(np.float32)
    sk = d['skip'] if skip else None
    ref = B.bn_ref(y, d['gamma'], d['beta'], sk)
    e32 = R.errors(B.bn_torch(y, d['gamma'], d['beta'], sk, torch.float32), ref)
    out, mean, rstd, _ = host_bn(cpu, y, d['gamma'], d['beta'], sk)
    ok, (e, _) = B.passes(out, ref, e32)
    print(f'{shape} skip={skip}: rel L2 {e[0]:.3g} (e32 {e32[0]:.3g}), worst {e[1]:.3g} (e32 {e32[1]:.3g})')
    assert ok, (e, e32)
    y64 = y.astype(np.float64)
    assert np.allclose(mean, y64.mean((0, 1, 2)), rtol=1e-6, atol=1e-6)
    assert np.allclose(rstd, 1 / np.sqrt(y64.var((0, 1, 2)) + B.EPS), rtol=1e-6)


def test_the_yardstick_at_mean_over_sigma_1e3_is_sound():
    """Checked before the case below was fixed: at |mean| / sigma = 1e3 torch's float32 batch norm is no worse than 8 x a textbook
    float32 two-pass (it is not broken there), and it sits far above float32's 6e-8: the mean's own rounding, 1e3 x 2^-24 of a sigma,
    sets a floor that no float32 pass gets under, so 8 e32 is within reach of one (measured: torch 4.7e-5, the two-pass 3.3e-4, the
    host build of the passes 1.2e-5) while a cancelling variance (e64 of order 1) is far outside it."""
    y = B.offset_map(TILED)
    d = B.inputs(TILED)
    ref = B.bn_ref(y, d['gamma'], d['beta'], d['skip'])
    e_torch = R.errors(B.bn_torch(y, d['gamma'], d['beta'], d['skip'], torch.float32), ref)
    e_two = R.errors(B.two_pass32(y, d['gamma'], d['beta'], d['skip']), ref)
    print(f'|mean|/sigma = 1e3: torch float32 {e_torch}, two-pass float32 {e_two}')
    for a, b in zip(e_torch, e_two):
        assert a <= B.BAR * b
        assert 1e-6 < a < 1e-3


def test_host_statistics_at_mean_over_sigma_1e3(cpu):
    y = B.offset_map(TILED)
    d = B.inputs(TILED)
    ref = B.bn_ref(y, d['gamma'], d['beta'], d['skip'])
    e32 = R.errors(B.bn_torch(y, d['gamma'], d['beta'], d['skip'], torch.float32), ref)
    out, _, rstd, _ = host_bn(cpu, y, d['gamma'], d['beta'], d['skip'])
    ok, (e, _) = B.passes(out, ref, e32)
    print(f'|mean|/sigma = 1e3: rel L2 {e[0]:.3g} (e32 {e32[0]:.3g}), worst {e[1]:.3g} (e32 {e32[1]:.3g})')
    assert ok, (e, e32)
    assert np.allclose(rstd, 1 / np.sqrt(y.astype(np.float64).var((0, 1, 2)) + B.EPS), rtol=1e-5)
    # and the restatement the planted defects are cut from
    assert B.passes(B.restated_bn(y, d['gamma'], d['beta'], d['skip']), ref, e32)[0]
    assert not B.passes(B.restated_bn(y, d['gamma'], d['beta'], d['skip'], defect='raw_sums'), ref, e32)[0]


def test_host_tile_statistics_exact_properties(cpu):
    n, h, w, c = 2, 19, 35, 64
    const = np.full((n, h, w, c), np.float32(0.1)) * np.arange(1, c + 1, dtype=np.float32)
    stats = host_stats(cpu, const).reshape(-1, 2, 64)
    assert np.array_equal(stats[:, 0], np.broadcast_to(const[0, 0, 0], stats[:, 0].shape)) and not stats[:, 1].any()
    # the counts: a map equal to the pixel's column index has mean (w - 1) / 2 only if every tile is weighted by its real pixels
    ramp = np.broadcast_to(np.arange(w, dtype=np.float32)[None, None, :, None], (n, h, w, c)).copy()
    out, mean, rstd, _ = host_bn(cpu, ramp, np.ones(c, np.float32), np.zeros(c, np.float32), None)
    assert np.array_equal(mean, np.full(c, (w - 1) / 2, np.float32))
    assert np.allclose(rstd, 1 / np.sqrt((w * w - 1) / 12 + B.EPS), rtol=1e-6)


def test_host_act_in_and_bias(cpu):
    x = np.concatenate([np.linspace(-30, 30, 2001), [0.0, -0.0, 1e-30, -1e-30]]).astype(np.float32)
    for code, name in enumerate(B.ACT_INS):
        got = np.zeros_like(x)
        cpu.bn_cpu_act_in(ptr(x), x.size, code, ptr(got))
        want = R.activation(x.astype(np.float64), name)
        assert np.allclose(got, want, rtol=3e-7, atol=0) and bool((np.abs(got) <= np.abs(x)).all())        # the amax bound stays a bound
        assert got[2001] == 0 and got[2002] == 0                                                            # act_in(0) == 0: padding stays zero
    s = np.linspace(-2, 2, 64 * 5, dtype=np.float32).reshape(5, 64)
    bias = np.linspace(-1, 1, 64, dtype=np.float32)
    got = np.zeros_like(s)
    cpu.bn_cpu_bias_act(ptr(s), ptr(bias), 5, 64, 1, ptr(got))
    assert np.array_equal(got, np.maximum(s + bias, 0))                       # the bias first, then the activation


CONFIGS = {                       # the case each defect is planted in: (skip, act_in, act, const)
    'unbiased': (True, None, None, None), 'padding_counted': (True, None, None, None), 'skip_after_relu': (True, None, None, None),
    'eps_dropped': (True, None, None, None), 'per_image': (True, None, None, None), 'bias_after_act': (False, None, 'elu', None),
    'act_in_pad_nonzero': (False, 'elu', None, -1.0),
}


def test_restated_arithmetic_meets_the_bar_in_every_configuration():
    for skip, act_in, act, const in sorted(set(CONFIGS.values()), key=str):
        d, ref, e32 = B.pipeline_case(TILED, skip, act_in, act, const)
        ok, figures = B.passes(B.restated(d, skip, act_in, act), ref, e32)
        assert ok, ((skip, act_in, act, const), figures)


@pytest.mark.parametrize('defect', [x for x in B.DEFECTS if x != 'raw_sums'])       # ('raw_sums' is planted in the |mean| / sigma = 1e3 case)
def test_planted_defects_fail_the_bar(defect):
    skip, act_in, act, const = CONFIGS[defect]
    d, ref, e32 = B.pipeline_case(TILED, skip, act_in, act, const)
    ok, (e, _) = B.passes(B.restated(d, skip, act_in, act, defect=defect), ref, e32)
    print(f'{defect}: rel L2 {e[0] / max(e32[0], 1e-300):.3g} x e32, worst {e[1] / max(e32[1], 1e-300):.3g} x e32')
    assert not ok, (defect, e, e32)


def test_entry_points_check_their_arguments_before_any_launch():
    lib = _lib.lib()
    one, odd = ctypes.c_void_p(16), ctypes.c_void_p(20)
    assert lib.mvnerf_conv3x3_stats_bytes(2, 19, 35, 128) == 2 * 2 * 3 * 2 * 128 * 4
    assert lib.mvnerf_conv3x3_stats_bytes(1, 1, 1, 64) == 512 and lib.mvnerf_conv3x3_stats_bytes(1, 16, 17, 96) == 0
    assert lib.mvnerf_conv3x3_stats_bytes(0, 4, 4, 64) == 0
    ex = lambda bias=None, act_in=0, stats=None, ca=32, cout=64, a=one: lib.mvnerf_conv3x3_nhwc_ex(
        a, ca, one, None, 0, None, one, 1, 4, 4, cout, 0, None, one, None, bias, act_in, stats, None)
    assert ex(act_in=3) == -2 and b'act_in=3' in lib.mvnerf_last_error()
    assert ex(act_in=-1) == -2
    assert ex(bias=odd) == -3 and b'bias' in lib.mvnerf_last_error()
    assert ex(stats=odd) == -3 and b'stats' in lib.mvnerf_last_error()
    assert ex(bias=one, ca=48) == -2 and ex(bias=one, cout=32) == -2
    assert ex(bias=one, a=None) == -1 and b'mvnerf_conv3x3_nhwc_ex' in lib.mvnerf_last_error()
    fin = lambda stats=one, n=1, cout=64, eps=1e-3, mean=one, rstd=one: lib.mvnerf_bn_finalize(stats, n, 4, 4, cout, eps, mean, rstd, None)
    assert fin(stats=None) == -1 and fin(mean=None) == -1 and fin(n=0) == -1
    assert fin(cout=96) == -2 and fin(eps=-1.0) == -1 and fin(eps=float('nan')) == -1 and fin(stats=odd) == -3
    app = lambda y=one, skip=None, pixels=8, c=64, act=1, out=one, gamma=one: lib.mvnerf_bn_apply_nhwc(
        y, one, one, gamma, one, skip, pixels, c, act, out, None, None)
    assert app(y=None) == -1 and app(out=None) == -1 and app(gamma=None) == -1 and app(pixels=0) == -1
    assert app(c=6) == -2 and app(act=2) == -2 and b'act=2' in lib.mvnerf_last_error()
    assert app(skip=odd) == -3 and b'skip' in lib.mvnerf_last_error() and app(y=odd) == -3


def test_ops_wrappers_refuse_host_tensors_and_bad_arguments():
    a, packed = torch.zeros(1, 4, 4, 32), torch.zeros(10, dtype=torch.uint8)
    with pytest.raises(ValueError, match='HIP device'):
        ops.conv3x3(a, None, packed, 64, None, bias=torch.zeros(64), act_in='relu', stats=True)
    with pytest.raises(ValueError, match='HIP device'):
        ops.bn_finalize(torch.zeros(128), 1, 4, 4, 64)
    with pytest.raises(ValueError, match='HIP device'):
        ops.bn_apply(torch.zeros(1, 4, 4, 64), *[torch.zeros(64)] * 4)
    with pytest.raises(ValueError, match='cout=96'):
        ops.conv3x3_stats_bytes(1, 4, 4, 96)
    assert ops.conv3x3_stats_bytes(3, 33, 17, 128) == 3 * 3 * 2 * 2 * 128 * 4


def test_module_switches_on_the_cpu():
    torch.manual_seed(3)
    images = torch.rand(2, 32, 48, 3)
    with pytest.raises(ValueError, match='fused_conv'):
        E.Block(64, 128, fused_conv='yes')
    with pytest.raises(ValueError, match='fused_conv'):
        E.VisualFeatures(256, (32, 48), fused_conv=1.5, **TINY_VIT)
    for almost in (1, 0):                                                  # 1 == True, but it is not the switch: the code asks `is True`
        with pytest.raises(ValueError, match='fused_conv'):
            E.VisualFeatures(256, (32, 48), fused_conv=almost, **TINY_VIT)
        with pytest.raises(ValueError, match='fused_conv'):
            E.Block(64, 128).fused_conv = almost
    vis = E.VisualFeatures(256, (32, 48), **TINY_VIT)
    assert vis.fused_conv is False and vis.conv_features.fused_conv is False and vis.vision_transformer.fused_conv is False
    with torch.no_grad():
        plain = vis(images)
        vis.fused_conv = 'auto'                                        # CPU tensors: the torch path, the same bits
        assert all(b.fused_conv == 'auto' for b in vis.conv_features.conv_features[3:]) and vis.vision_transformer.fused_conv == 'auto'
        assert torch.equal(vis(images), plain)
        vis.fused_conv = True
        with pytest.raises(ValueError, match='HIP device'):
            vis(images)
        with pytest.raises(ValueError, match='HIP device'):
            vis.conv_features(images.permute(0, 3, 1, 2))
        with pytest.raises(ValueError, match='HIP device'):
            vis.vision_transformer(torch.rand(2, 3, 32, 32))
    vis.fused_conv = True
    with pytest.raises(RuntimeError, match='no backward'):               # parameters that need a gradient
        vis.conv_features(images.permute(0, 3, 1, 2))
    producer = E.LanguageFeatureProducer((32, 48), fused_visual='auto', **TINY_VIT)
    assert producer.visual_features.fused_conv == 'auto' and producer.combine_clip_visual.fused_conv is False
    assert E.LanguageFeatureProducer((32, 48), fused_conv='auto', **TINY_VIT).visual_features.fused_conv is False
    assert E.FeatureProducer((32, 48), **TINY_VIT).visual_features.fused_conv is False
