"""The fused 3x3 convolution without a GPU: the float64 reference of tests/conv3x3_ref.py against torch, the host build of
csrc/mvnerf_conv.h (tests/cpu_conv) bit for bit against the NumPy restatement, the restated arithmetic against the GPU test's bar at
every shape and at input scales 2^-40, 1, 2^40, planted defects against that same bar, the argument checks of the new entry points, the
ABI, and the `fused_conv` switch of the encoder modules.  The kernel itself is tests/test_gpu_conv3x3.py."""
import ctypes
import inspect
import os
import subprocess

import numpy as np
import pytest
import torch

from tests import conv3x3_ref as R
from thesis_clip_nerf_amd import _lib
from thesis_clip_nerf_amd import encoders as E
from thesis_clip_nerf_amd import ops

HERE = os.path.dirname(os.path.abspath(__file__))
SCALES = [2.0 ** -40, 1.0, 2.0 ** 40]
TINY_FUSION = dict(clip_channels=(16, 32, 32, 64), text_dim=64, widths=(64, 32, 32), up3_filters=16)      # as tests/test_feature_fusion_cpu.py


@pytest.fixture(scope='module')
def cpu():
    d = os.path.join(HERE, 'cpu_conv')
    subprocess.run(['make', '-C', d], check=True, capture_output=True)
    return ctypes.CDLL(os.path.join(d, 'libmvnerf_conv_cpu.so'))


def ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


@pytest.mark.parametrize('shape', R.SHAPES, ids=str)
def test_reference_against_float64_torch(shape):
    a, b, wt, mul = R.inputs(shape)
    for act in R.ACTS:
        ref = R.conv_ref(a, b, wt, act, mul)
        got = R.torch_conv(a, b, wt, act, mul, torch.float64)
        assert ref.shape == (shape[0], shape[1], shape[2], shape[5])
        assert R.rel_l2(got, ref) <= 1e-12 and R.worst(got, ref) <= 1e-12


def _special_values():
    rng = np.random.default_rng(1)
    tiny, huge = np.float32(1.4e-45), np.finfo(np.float32).max
    pows = np.ldexp(np.float32(1), np.arange(-149, 128)).astype(np.float32)
    ends = np.array([256.0, np.nextafter(np.float32(512), np.float32(0)), 512.0, np.nextafter(np.float32(256), np.float32(0))], np.float32)
    rnd = (rng.standard_normal(4000) * np.exp(rng.uniform(-30, 30, 4000))).astype(np.float32)
    return np.concatenate([rnd, pows, -pows, ends, -ends, [0.0, -0.0, tiny, -tiny, huge, -huge, np.finfo(np.float32).tiny]]).astype(np.float32)


def test_host_build_matches_the_numpy_restatement_bit_for_bit(cpu):
    x = _special_values()
    n = x.size
    cpu.conv_cpu_scale_exp.argtypes = [ctypes.c_float]
    for v in x:
        e = cpu.conv_cpu_scale_exp(float(v))
        assert e == R.scale_exp(v), v
        if v != 0:
            assert 256.0 <= np.ldexp(np.float64(abs(v)), e) < 512.0, v
    assert cpu.conv_cpu_scale_exp(0.0) == 0 and R.scale_exp(np.float32(1.4e-45)) == 157 and R.scale_exp(np.finfo(np.float32).max) == -119
    cpu.conv_cpu_amax_finite.argtypes = [ctypes.c_float]
    assert cpu.conv_cpu_amax_finite(3.0e38) == 1 and cpu.conv_cpu_amax_finite(float('inf')) == 0 and cpu.conv_cpu_amax_finite(float('nan')) == 0
    # the fp16 rounding itself (NumPy's astype is round-to-nearest-even with subnormals), on the values and on what the cuts feed it
    h, back = np.zeros(n, np.uint16), np.zeros(n, np.float32)
    with np.errstate(over='ignore'):
        want = x.astype(np.float16)
    cpu.conv_cpu_rn16(ptr(x), ctypes.c_long(n), ptr(h), ptr(back))
    assert np.array_equal(h, want.view(np.uint16)) and np.array_equal(back.view(np.uint32), want.astype(np.float32).view(np.uint32))
    # the pieces, under the exponent of every magnitude class: the tensor's own maximum, 1.5 x it, and a far larger one
    for amax in (np.abs(x[:4000]).max(), np.float32(1.0), np.float32(2.0 ** 60), np.float32(2.0 ** -100), np.float32(1.4e-45)):
        e = R.scale_exp(amax)
        sel = x[np.abs(x) <= amax]
        a0, a1, a0s = (np.zeros(sel.size, np.uint16) for _ in range(3))
        cpu.conv_cpu_cut_weight(ptr(sel), ctypes.c_long(sel.size), e, ptr(a0), ptr(a1), ptr(a0s))
        for got, ref in zip((a0, a1, a0s), R.cut_weight(sel, e)):
            assert np.array_equal(got, ref.view(np.uint16)), amax
        b0, b1 = (np.zeros(sel.size, np.uint16) for _ in range(2))
        cpu.conv_cpu_cut_act(ptr(sel), ctypes.c_long(sel.size), e, ptr(b0), ptr(b1))
        for got, ref in zip((b0, b1), R.cut_act(sel, e)):
            assert np.array_equal(got, ref.view(np.uint16)), amax
        assert np.isfinite(R.cut_act(sel, e)[0].astype(np.float32)).all()             # normalised: nothing finite overflows fp16


@pytest.mark.parametrize('scale', SCALES, ids=['2^-40', '1', '2^40'])
@pytest.mark.parametrize('shape', R.SHAPES, ids=str)
def test_restated_arithmetic_meets_the_gpu_bar(shape, scale):
    a, b, wt, mul = R.inputs(shape, 0, scale, scale)
    for act in (None, 'elu'):
        ref = R.conv_ref(a, b, wt, act, mul)
        e32_l2, e32_worst = R.e32(shape, act, True, 0, scale, scale)
        e_l2, e_worst = R.errors(R.split_conv(a, b, wt, act, mul), ref)
        print(f'{shape} x {scale:g} {act}: rel L2 {e_l2 / e32_l2:.2f} x e32, worst {e_worst / e32_worst:.2f} x e32')
        assert e_l2 <= R.BAR * e32_l2 and e_worst <= R.BAR * e32_worst, (e_l2, e32_l2, e_worst, e32_worst)


def _fails_the_bar(got, ref, e32):
    e_l2, e_worst = R.errors(got, ref)
    return not (e_l2 <= R.BAR * e32[0] and e_worst <= R.BAR * e32[1])


@pytest.mark.parametrize('shape', R.SHAPES, ids=str)
def test_planted_defects_fail_the_same_assertion(shape):
    """Each wrong reading misses `e <= 8 e32`.  Where a defect is no defect - no second source to swap, taps of a 1 x 1 image that are
    all padding but the centre - the case is left out by construction, not by tolerance."""
    a, b, wt, mul = R.inputs(shape)
    ref = R.conv_ref(a, b, wt, 'elu', mul)
    e32 = R.e32(shape, 'elu', True)
    assert not _fails_the_bar(R.split_conv(a, b, wt, 'elu', mul), ref, e32)
    one_pixel = shape[1] == 1 and shape[2] == 1
    for defect in R.DEFECTS:
        if (defect == 'ab_swapped' and b is None) or (one_pixel and defect in ('clamp_padding', 'taps_transposed', 'taps_flipped')):
            continue
        assert _fails_the_bar(R.split_conv(a, b, wt, 'elu', mul, defect=defect), ref, e32), defect


def test_missing_rescale_between_sources_of_1e3_and_1e_3_fails_the_bar():
    shape = R.SMALL_TWO
    a, b, wt, mul = R.inputs(shape, 0, 1e3, 1e-3)
    ref = R.conv_ref(a, b, wt, None, mul)
    e32 = R.e32(shape, None, True, 0, 1e3, 1e-3)
    assert not _fails_the_bar(R.split_conv(a, b, wt, None, mul), ref, e32)
    assert _fails_the_bar(R.split_conv(a, b, wt, None, mul, defect='no_rescale'), ref, e32)
    # the fixed v / 64 scale of the MLP kernels loses the remainder piece of small inputs: what the per-tensor scale is for
    x = (np.random.default_rng(0).standard_normal(4096) * 1e-3).astype(np.float32)
    b0 = (x / 64).astype(np.float16).astype(np.float32)
    b1 = (x - 64 * b0).astype(np.float16).astype(np.float32)
    fixed = np.abs((64 * b0 + b1).astype(np.float64) - x).max() / np.abs(x).max()
    p0, p1 = (p.astype(np.float64) for p in R.cut_act(x, R.scale_exp(np.abs(x).max())))
    ours = np.abs(np.ldexp(p0 + p1 / 64, -R.scale_exp(np.abs(x).max())) - x).max() / np.abs(x).max()
    assert ours < 2.0 ** -21 and fixed > 20 * ours, (fixed, ours)


def test_entry_points_validate_their_arguments_without_a_gpu():
    lib = _lib.lib()
    one, odd = ctypes.c_void_p(16), ctypes.c_void_p(20)
    assert lib.mvnerf_conv3x3_packed_bytes(2048, 1024) == 256 + 9 * 2048 * 1024 * 6
    assert lib.mvnerf_conv3x3_packed_bytes(48, 64) == 0 and lib.mvnerf_conv3x3_packed_bytes(32, 32) == 0 and lib.mvnerf_conv3x3_packed_bytes(0, 64) == 0

    def call(a=one, ca=32, ma=one, b=None, cb=0, mb=None, packed=one, n=1, h=4, w=4, cout=64, act=2, mul=None, out=one, top=None):
        return lib.mvnerf_conv3x3_nhwc(a, ca, ma, b, cb, mb, packed, n, h, w, cout, act, mul, out, top, None)
    for kw, name in ((dict(a=None), b'(a)'), (dict(ma=None), b'(amax_a)'), (dict(packed=None), b'(packed)'), (dict(out=None), b'(out)')):
        assert call(**kw) == -1 and b'null pointer' in lib.mvnerf_last_error() and name in lib.mvnerf_last_error()
    assert call(b=one) == -1 and call(cb=32) == -1 and call(b=one, cb=32) == -1 and b'go together' in lib.mvnerf_last_error()
    for kw in (dict(n=0), dict(h=0), dict(w=-1)):
        assert call(**kw) == -1
    assert call(ca=48) == -2 and b'Ca=48' in lib.mvnerf_last_error()
    assert call(ca=0) == -2 and call(b=one, cb=16, mb=one) == -2 and b'Cb=16' in lib.mvnerf_last_error()
    assert call(cout=32) == -2 and b'Cout=32' in lib.mvnerf_last_error() and call(cout=96) == -2
    assert call(act=3) == -2 and b'act=3' in lib.mvnerf_last_error() and call(act=-1) == -2
    assert call(n=70000, h=70000, w=4) == -2
    for kw, name in ((dict(a=odd), b'a must'), (dict(packed=odd), b'packed must'), (dict(mul=odd), b'mul must'), (dict(out=odd), b'out must'),
                     (dict(b=odd, cb=32, mb=one), b'b must')):
        assert call(**kw) == -3 and name in lib.mvnerf_last_error()
    assert call(ma=ctypes.c_void_p(18)) == -3 and call(top=ctypes.c_void_p(18)) == -3
    assert call(ca=48, a=odd) == -2                                                      # the shape is checked before the alignment
    assert lib.mvnerf_conv3x3_pack(None, 32, 64, one, None) == -1 and lib.mvnerf_conv3x3_pack(one, 48, 64, one, None) == -2
    assert lib.mvnerf_conv3x3_pack(one, 32, 64, odd, None) == -3
    assert lib.mvnerf_absmax_f32(None, 4, one, None) == -1 and lib.mvnerf_absmax_f32(one, 0, one, None) == -1
    assert lib.mvnerf_absmax_f32(ctypes.c_void_p(18), 4, one, None) == -3


def test_new_symbols_are_in_the_header_and_the_library():
    header = open(_lib.HEADER_PATH).read()
    for name in ('mvnerf_conv3x3_packed_bytes', 'mvnerf_conv3x3_pack', 'mvnerf_absmax_f32', 'mvnerf_conv3x3_nhwc'):
        assert name + '(' in header and name in _lib.SIGNATURES and hasattr(_lib.lib(), name)


def test_ops_wrappers_have_no_cpu_path_and_check_first():
    z = torch.zeros
    with pytest.raises(ValueError, match='no CPU path'):
        ops.absmax(z(4))
    with pytest.raises(ValueError, match='no CPU path'):
        ops.conv3x3_pack(z(3, 3, 32, 64))
    with pytest.raises(ValueError, match='no CPU path'):
        ops.conv3x3(z(1, 2, 2, 32), None, z(8, dtype=torch.uint8), 64, 'elu')
    with pytest.raises(ValueError, match='cin=48'):
        ops.conv3x3_packed_bytes(48, 64)
    assert ops.conv3x3_packed_bytes(32, 64) == 256 + 9 * 32 * 64 * 6


def _tiny_fusion(**kw):
    torch.manual_seed(3)
    return E.CombineCLIPVisualV4(use_dense=True, activation='elu', half_size=(8, 8), visual_channels=32, fused_tail=False, **TINY_FUSION, **kw)


def _tiny_inputs():
    g = torch.Generator().manual_seed(4)
    r = lambda *s: torch.randn(*s, generator=g)
    return (r(1, 64), r(1, 16, 4, 4), r(1, 32, 2, 2), r(1, 32, 2, 2), r(1, 64, 1, 1)), r(1, 32, 8, 8), r(1, 64)


def test_fused_conv_defaults_to_false_and_true_needs_no_gradient():
    assert E.DoubleConv(32, 64).fused_conv is False and E.Up((4, 4), 32, 32, 64).fused_conv is False
    mod = _tiny_fusion()
    assert mod.fused_conv is False and mod.up_1.fused_conv is False and mod.up_3.double_conv.fused_conv is False
    assert inspect.signature(E.LanguageFeatureProducer.__init__).parameters['fused_conv'].default is False
    assert inspect.signature(E.CombineCLIPVisualV4.__init__).parameters['fused_conv'].default is False
    mod.fused_conv = 'auto'
    assert mod.up_2.double_conv.fused_conv == 'auto'
    with pytest.raises(ValueError):
        mod.fused_conv = 'yes'
    clip, visual, text = _tiny_inputs()
    mod.fused_conv = True
    with pytest.raises(RuntimeError, match='no backward'):
        mod(clip, visual, text)                                                  # the parameters require a gradient
    with torch.no_grad(), pytest.raises(ValueError, match='not one the HIP pass takes'):          # 64 + 32 -> 32 channels: no silent torch run
        E.conv3x3_act(mod.up_1.double_conv.conv_1, torch.zeros(1, 64, 2, 2), torch.zeros(1, 32, 2, 2), 'elu', True)
    with torch.no_grad():
        got, amax = E.conv3x3_act(mod.up_1.double_conv.conv_1, torch.ones(1, 64, 2, 2), torch.ones(1, 32, 2, 2), 'elu', 'auto')
    assert amax is None and got.shape == (1, 32, 2, 2)
    dc = E.DoubleConv(32, 64, 'elu', fused_conv=True)
    with torch.no_grad(), pytest.raises(ValueError, match='no CPU path'):
        dc(torch.zeros(1, 32, 4, 4))
    assert E.conv3x3_fusable(dc.conv_1, 32) and E.conv3x3_fusable(dc.conv_2, 32, 32) and not E.conv3x3_fusable(dc.conv_1, 16, 16)
    assert not E.conv3x3_fusable(E.SameConv2d(32, 64, 3), 32) and not E.conv3x3_fusable(E.SameConv2d(32, 64, 1, bias=False), 32)


def test_default_forward_is_the_fused_conv_false_forward_bit_for_bit():
    clip, visual, text = _tiny_inputs()
    default, spelled, auto = _tiny_fusion(), _tiny_fusion(fused_conv=False), _tiny_fusion(fused_conv='auto')
    with torch.no_grad():
        want = default(clip, visual, text)
        assert torch.equal(want, spelled(clip, visual, text))
        assert torch.equal(want, auto(clip, visual, text))                      # 'auto' on the CPU is the torch chain
    out = auto(clip, visual, text)                                               # ... and so it is when a gradient is needed
    out.square().mean().backward()
    assert torch.equal(out.detach(), want) and all(p.grad is not None for p in auto.parameters())


def test_train_language_has_the_flag():
    from thesis_clip_nerf_amd import train_language as T
    with pytest.raises(SystemExit):
        T.main(['--fused-conv'])                                                 # only meaningful with --encoder v4
