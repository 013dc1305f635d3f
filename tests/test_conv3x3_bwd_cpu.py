"""The backward of the fused 3x3 convolution without a GPU: the float64 references of tests/conv3x3_bwd_ref.py against torch double
autograd, the host build of the weight-gradient part of csrc/mvnerf_conv.h (tests/cpu_conv_bwd) bit for bit against the NumPy restatement,
the restated arithmetic against the GPU tests' bar, planted defects against that same bar, the argument checks of the new entry points
and the `fused_backward` switch of the encoder modules.  The kernel itself is tests/test_gpu_conv3x3_bwd.py."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

from tests import conv3x3_bwd_ref as B
from tests import conv3x3_ref as R
from thesis_clip_nerf_amd import _lib
from thesis_clip_nerf_amd import encoders as E
from thesis_clip_nerf_amd import ops

HERE = os.path.dirname(os.path.abspath(__file__))
TINY_VIT = dict(transformer_image_size=(32, 32), patch_size=16, embed_dim=32, num_heads=4, hooks=(1, 2, 3, 4), features=(32, 64, 96, 128))
# (shape, keyword arguments of B.case): the accuracy bar is asserted where N h w >= 30
BAR_CASES = [(B.SMALL, {}), (B.TILED, {}), ((3, 33, 17, 64, 64), dict(mask_g=True)), ((1, 16, 16, 32, 64), dict(scale_g=1e-6))]
ONE_PIXEL = (1, 1, 1, 32, 64)
TWO_SLABS = (2, 33, 49, 32, 64)                    # 2 x 3 x 4 = 24 tiles: one full slab and a ragged one of 8


@pytest.fixture(scope='module')
def cpu():
    d = os.path.join(HERE, 'cpu_conv_bwd')
    subprocess.run(['make', '-C', d], check=True, capture_output=True)
    return ctypes.CDLL(os.path.join(d, 'libmvnerf_conv_bwd_cpu.so'))


def ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


@pytest.mark.parametrize('act_in', B.ACTS, ids=str)
@pytest.mark.parametrize('shape', [ONE_PIXEL, B.SMALL, B.TILED], ids=str)
def test_references_against_float64_torch_autograd(shape, act_in):
    x, g, wt, bias = B.case(shape)
    got = B.torch_grads(x, g, wt, bias, act_in, torch.float64)
    ref = (B.dx_ref(x, g, wt, act_in), B.dw_ref(x, g, act_in), B.dbias_ref(g))
    for a, b in zip(got, ref):
        assert a.shape == b.shape and R.rel_l2(a, b) <= 1e-12 and R.worst(a, b) <= 1e-12


def test_host_build_matches_the_numpy_restatement_bit_for_bit(cpu):
    rng = np.random.default_rng(2)
    v = (rng.standard_normal(6000) * np.exp(rng.uniform(-12, 12, 6000))).astype(np.float32)
    v = np.concatenate([v, [0.0, -0.0, 1.0, -1.0, 255.9, -511.9], np.ldexp(np.float32(1), np.arange(-30, 30)).astype(np.float32)]).astype(np.float32)
    n = v.size
    for e in (-20, -3, 0, 5, 17):
        a0, a1, a0s = (np.zeros(n, np.uint16) for _ in range(3))
        cpu.conv_bwd_cpu_cut_g(ptr(v), ctypes.c_long(n), e, ptr(a0), ptr(a1), ptr(a0s))
        with np.errstate(over='ignore', invalid='ignore'):
            want = R.cut_weight(v, e)
        for got, w in zip((a0, a1, a0s), want):
            assert np.array_equal(got, w.view(np.uint16))
        for code, name in enumerate(B.ACTS):
            b0, b1 = np.zeros(n, np.uint16), np.zeros(n, np.uint16)
            cpu.conv_bwd_cpu_cut_x(ptr(v), ctypes.c_long(n), code, e, ptr(b0), ptr(b1))
            acted = np.zeros(n, np.float32)                               # (expm1f of the C library, within an ulp of NumPy's)
            cpu.conv_bwd_cpu_act(ptr(v), ctypes.c_long(n), code, ptr(acted))
            assert np.allclose(acted, R.activation(v, name), rtol=3e-7, atol=0) and (name == 'elu' or np.array_equal(acted, R.activation(v, name)))
            want = R.cut_act(acted, e)
            finite = np.isfinite(want[0].astype(np.float32))             # (beyond the fp16 range the remainder is inf - inf)
            for got, w in zip((b0, b1), want):
                assert np.array_equal(got[finite], w.view(np.uint16)[finite])
    # the slab geometry and the finish
    cpu.conv_bwd_cpu_tiles.restype = cpu.conv_bwd_cpu_slabs.restype = ctypes.c_long
    assert cpu.conv_bwd_cpu_slab_pixels() == B.SLAB_PIXELS == ops.CONV3X3_WGRAD_SLAB_PIXELS
    for n_, h, w in ((1, 1, 1), (2, 19, 35), (3, 33, 65), (3, 240, 320)):
        tiles = B.tiles_of(n_, h, w)
        assert cpu.conv_bwd_cpu_tiles(n_, h, w) == len(tiles) and cpu.conv_bwd_cpu_slabs(n_, h, w) == -(-len(tiles) // B.SLAB_TILES)
    for f in (cpu.conv_bwd_cpu_finish, cpu.conv_bwd_cpu_dbias_finish):
        f.restype, f.argtypes = ctypes.c_float, [ctypes.c_double, ctypes.c_float, ctypes.c_float]
    total = 123456.789
    assert cpu.conv_bwd_cpu_finish(total, 3.0, 0.01) == np.float32(np.ldexp(total, -(R.scale_exp(3.0) + R.scale_exp(0.01))))
    assert cpu.conv_bwd_cpu_finish(total, 0.0, 1.0) == 0.0 and cpu.conv_bwd_cpu_finish(total, 1.0, 0.0) == 0.0
    assert np.isnan(cpu.conv_bwd_cpu_finish(total, float('nan'), 1.0)) and np.isnan(cpu.conv_bwd_cpu_finish(total, 1.0, float('inf')))
    assert cpu.conv_bwd_cpu_dbias_finish(total, 0.0, 1.0) == np.float32(total) and cpu.conv_bwd_cpu_dbias_finish(total, 1.0, 0.0) == 0.0
    assert np.isnan(cpu.conv_bwd_cpu_dbias_finish(total, float('inf'), 1.0))


def restated(shape, act_in, kw, defect=None):
    """-> [(name, got, ref, yardstick)] of the restated weight, bias and (where the channel counts allow) data gradient."""
    x, g, wt, bias = B.case(shape, **kw)
    yard = B.e32(shape, act_in, **kw)
    wd = defect if defect in B.WGRAD_DEFECTS else None
    dw, db = B.split_wgrad(x, g, act_in, defect=wd)
    out = [('dw', dw, B.dw_ref(x, g, act_in), yard['dw']), ('dbias', db, B.dbias_ref(g), yard['dbias'])]
    if shape[3] % 64 == 0 and shape[4] % 32 == 0:
        dd = defect if defect in B.DGRAD_DEFECTS else None
        out.append(('dx', B.split_dgrad(x, g, wt, act_in, defect=dd), B.dx_ref(x, g, wt, act_in), yard['dx']))
    return out


@pytest.mark.parametrize('act_in', B.ACTS, ids=str)
@pytest.mark.parametrize('case', BAR_CASES, ids=str)
def test_restated_arithmetic_is_inside_the_bar(case, act_in):
    shape, kw = case
    assert shape[0] * shape[1] * shape[2] >= B.MIN_PIXELS
    for name, got, ref, yard in restated(shape, act_in, kw):
        ok, ratios = B.within_bar(got, ref, yard)
        print(f'{shape} {kw} {act_in} {name}: {ratios[0]:.2f} / {ratios[1]:.2f} x e32')
        assert ok, (name, ratios)


def test_one_pixel_is_one_product_and_is_reported_not_asserted():
    """A one-pixel sum is a single product that float32 rounds once: the ratio to e32 says nothing (DESIGN.md 18 has the figure); the
    GPU file's exact tests cover the shape.  What holds: the error is of the size of one float32 rounding."""
    for name, got, ref, yard in restated(ONE_PIXEL, None, {}):
        err = R.errors(got, ref)
        print(f'{ONE_PIXEL} {name}: {err[0] / yard[0] if yard[0] else 0:.2f} / {err[1] / yard[1] if yard[1] else 0:.2f} x e32')
        assert err[0] < 2.0 ** -22 and err[1] < 2.0 ** -22


def defect_shows(defect):
    """Whether the planted defect fails the assertion of test_restated_arithmetic_is_inside_the_bar on at least one of its cases (plus,
    for what only more than one slab can show, the two-slab shape)."""
    for shape, kw in BAR_CASES + [(TWO_SLABS, {})]:
        for act_in in ('elu', 'relu'):
            for name, got, ref, yard in restated(shape, act_in, kw, defect):
                if not B.within_bar(got, ref, yard)[0]:
                    return True
    return False


def test_the_clean_restatement_passes_on_the_two_slab_shape_too():
    for name, got, ref, yard in restated(TWO_SLABS, 'elu', {}):
        assert B.within_bar(got, ref, yard)[0], name


@pytest.mark.parametrize('defect', B.WGRAD_DEFECTS + B.DGRAD_DEFECTS)
def test_planted_defects_fail_the_bar(defect):
    assert defect_shows(defect), defect


def test_argument_checks_come_before_any_launch():
    lib = _lib.lib()
    one, odd = ctypes.c_void_p(256), ctypes.c_void_p(260)
    assert lib.mvnerf_conv3x3_wgrad_slab_pixels() == ops.CONV3X3_WGRAD_SLAB_PIXELS
    wb = lib.mvnerf_conv3x3_wgrad_workspace_bytes
    assert wb(2, 19, 35, 64, 128) == 1 * (9 * 64 * 128 + 128) * 4 and wb(3, 33, 65, 32, 64) == 3 * (9 * 32 * 64 + 64) * 4
    assert wb(1, 4, 4, 48, 64) == 0 and wb(1, 4, 4, 32, 32) == 0 and wb(0, 4, 4, 32, 64) == 0 and wb(1, 4, -1, 32, 64) == 0
    base = dict(x=one, amax_x=one, act_in=0, g=one, amax_g=one, N=1, h=4, w=4, Cin=32, Cout=64, dw=one, dbias=None, ws=one, stream=None)
    call = lambda **kw: lib.mvnerf_conv3x3_wgrad_nhwc(*{**base, **kw}.values())
    assert call(x=None) == -1 and b'null pointer (x)' in lib.mvnerf_last_error()
    assert call(ws=None) == -1 and call(amax_g=None) == -1 and call(dw=None) == -1
    assert call(h=0) == -1
    assert call(Cin=48) == -2 and b'Cin=48' in lib.mvnerf_last_error()
    assert call(Cin=16) == -2 and call(Cout=32) == -2 and call(Cout=96) == -2
    assert call(act_in=3) == -2 and call(act_in=-1) == -2 and b'act_in=-1' in lib.mvnerf_last_error()
    assert call(ws=odd) == -3 and b'workspace' in lib.mvnerf_last_error()
    assert call(x=odd) == -3 and call(g=odd) == -3 and call(dw=odd) == -3 and call(dbias=odd) == -3
    assert call(amax_x=ctypes.c_void_p(258)) == -3
    assert lib.mvnerf_abi_version() == 1
    # the Python wrappers: ValueError, and no CPU path
    with pytest.raises(ValueError, match='HIP device'):
        ops.conv3x3_wgrad(torch.zeros(1, 4, 4, 32), torch.zeros(1, 4, 4, 64))
    with pytest.raises(ValueError):
        ops.conv3x3_wgrad_workspace_bytes(1, 4, 4, 32, 48)
    with pytest.raises(ValueError, match='HIP device'):
        ops.conv3x3_pack_transposed(torch.zeros(3, 3, 64, 64))


def test_fused_backward_switch():
    vf = E.VisualFeatures(256, (32, 48), **TINY_VIT)
    blocks = [m for m in vf.modules() if isinstance(m, E.Block)]
    assert len(blocks) == 3 and vf.fused_backward is False and vf.conv_features.fused_backward is False
    assert vf.vision_transformer.fused_backward is False and not any(b.fused_backward for b in blocks)
    vf.fused_backward = True
    assert vf.conv_features.fused_backward is True and vf.vision_transformer.fused_backward is True and all(b.fused_backward is True for b in blocks)
    assert vf.fused_conv is False                                          # a switch of its own
    vf.fused_backward = False
    assert not any(b.fused_backward for b in blocks)
    for bad in (1, 0, 'auto', None, 'yes'):
        for module in (vf, vf.conv_features, vf.vision_transformer, blocks[0]):
            with pytest.raises(ValueError, match='fused_backward'):
                module.fused_backward = bad
        with pytest.raises(ValueError, match='fused_backward'):
            E.VisualFeatures(256, (32, 48), fused_backward=bad, **TINY_VIT)
    on = E.VisualFeatures(256, (32, 48), fused_conv='auto', fused_backward=True, **TINY_VIT)
    assert all(b.fused_backward is True and b.fused_conv == 'auto' for b in on.modules() if isinstance(b, E.Block))
    assert E.ConvolutionalEncoder(256, fused_backward=True).conv_features[4].fused_backward is True
    assert E.Block(64, 128, fused_backward=True).fused_backward is True
    prod = E.FeatureProducer((32, 48), fused_conv='auto', fused_backward=True, **TINY_VIT)
    assert prod.visual_features.fused_backward is True and E.FeatureProducer((32, 48), **TINY_VIT).visual_features.fused_backward is False
    assert E.LanguageFeatureProducer((32, 48), **TINY_VIT).visual_features.fused_backward is False


def test_on_the_cpu_the_switch_changes_nothing():
    """No GPU tensor in the call: 'auto' stays torch with or without `fused_backward`, the same bits, gradients and all."""
    torch.manual_seed(3)
    enc = E.ConvolutionalEncoder(256, fused_conv='auto')
    x = torch.rand(1, 3, 16, 16, generator=torch.Generator().manual_seed(1))
    enc(x).square().mean().backward()
    want = [p.grad.clone() for p in enc.parameters()]
    enc.zero_grad()
    enc.fused_backward = True
    enc(x).square().mean().backward()
    assert all(torch.equal(a, p.grad) for a, p in zip(want, enc.parameters()))
    assert E.conv3x3_dgrad_fusable(enc.conv_features[3].conv_1) and not E.conv3x3_dgrad_fusable(E.SameConv2d(96, 256, 3))
