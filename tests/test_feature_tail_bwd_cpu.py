"""The backward of the producers' tail without a GPU: the float64 reference against torch double autograd, the host
build of csrc/mvnerf_feature_tail.h (tests/cpu_feature_tail_bwd) bit for bit against the NumPy restatement, the restatement against the
GPU tests' bar, the tiling's index arithmetic exhaustively, and planted defects against that same bar.  The kernel itself is
tests/test_gpu_feature_tail_bwd.py."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

from tests import feature_fusion_ref as R
from tests import feature_tail_bwd_ref as B

HERE = os.path.dirname(os.path.abspath(__file__))
ACTS = (None, 'relu', 'elu')


@pytest.fixture(scope='module')
def cpu():
    d = os.path.join(HERE, 'cpu_feature_tail_bwd')
    subprocess.run(['make', '-C', d], check=True, capture_output=True)
    lib = ctypes.CDLL(os.path.join(d, 'libmvnerf_feature_tail_bwd_cpu.so'))
    lib.ftb_cpu_coef.restype, lib.ftb_cpu_coef.argtypes = ctypes.c_float, [ctypes.c_int] * 3
    lib.ftb_cpu_tiles.restype = lib.ftb_cpu_adjoint.restype = lib.ftb_cpu_epilogue.restype = ctypes.c_long
    lib.ftb_cpu_adjoint.argtypes = [ctypes.c_void_p] + [ctypes.c_int] * 3 + [ctypes.c_void_p] * 2
    lib.ftb_cpu_epilogue.argtypes = [ctypes.c_int] * 5 + [ctypes.c_void_p]
    lib.ftb_cpu_act_grad.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_long, ctypes.c_int, ctypes.c_void_p]
    lib.ftb_cpu_taps.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
    return lib


def ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


@pytest.mark.parametrize('act', ACTS, ids=str)
@pytest.mark.parametrize('shape', [(2, 9, 11, 32, 48), (1, 1, 1, 16, 16), (1, 3, 17, 16, 32), (1, 17, 2, 32, 16)], ids=str)
def test_float64_reference_against_torch_double_autograd(shape, act):
    shape = shape + (act,)
    a, b, weight = R.tail_inputs(shape)
    g = B.cotangent(shape)
    ref = B.tail_bwd_ref(g, a, b, weight, act)
    want = B.torch_tail_grads(g, a, b, weight, act, torch.float64)
    for name in B.ARRAYS:
        assert R.worst(ref[name], want[name]) < 1e-12 and R.rel_l2(ref[name], want[name]) < 1e-12, name


def test_host_build_coefficients_and_fold(cpu):
    assert (cpu.ftb_cpu_tile_h(), cpu.ftb_cpu_tile_w()) == (B.TILE_H, B.TILE_W)
    for n in range(1, 13):
        u = B.upsample_matrix(n)                                     # the forward's own matrix: the coefficients are its entries
        for o in range(2 * n):
            for l in range(n):
                got = cpu.ftb_cpu_coef(o, l, n)
                assert got == B.coef(o, l, n) == u[o, l], (n, o, l)
        assert np.all(u.sum(1) == 1.0)
        for l in range(n):
            c, on = np.zeros(4, np.float32), np.zeros(4, np.int32)
            first = cpu.ftb_cpu_taps(l, n, ptr(c), ptr(on))
            want = B.taps(l, n)
            assert first == 2 * l - 1 and [(first + t, c[t]) for t in range(4) if on[t]] == want
            assert all(cf > 0 for _, cf in want) and np.all(c[on == 0] == 0)
            # the terms are all of the column: nothing else of the forward's matrix lands on l
            assert sorted(o for o, _ in want) == sorted(np.nonzero(u[:, l])[0].tolist())
    # the fold: 1/4 + 3/4 on the border sample, and both outputs of a one-sample axis
    assert cpu.ftb_cpu_coef(0, 0, 5) == 1.0 and cpu.ftb_cpu_coef(9, 4, 5) == 1.0
    assert cpu.ftb_cpu_coef(0, 0, 1) == 1.0 and cpu.ftb_cpu_coef(1, 0, 1) == 1.0
    assert [cpu.ftb_cpu_coef(o, 2, 5) for o in range(3, 7)] == [0.25, 0.75, 0.75, 0.25]


@pytest.mark.parametrize('hw', [(1, 1), (1, 5), (3, 17), (9, 11), (17, 33), (8, 16)], ids=str)
def test_host_build_adjoint_bit_for_bit(cpu, hw):
    h, w = hw
    n = 2
    rng = np.random.default_rng([7, h, w])
    g = (rng.standard_normal((n, 2 * h, 2 * w, 256)) * np.exp2(rng.integers(-8, 8, (n, 2 * h, 2 * w, 256)))).astype(np.float32)
    got, writes = np.full((n, h, w, 256), np.nan, np.float32), np.zeros((n, h, w), np.int32)
    assert cpu.ftb_cpu_adjoint(ptr(g), n, h, w, ptr(got), ptr(writes)) == 0
    assert np.all(writes == 1)
    want = B.adjoint_f32(g)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    # and it is the adjoint: within float32 rounding of the float64 matrix form
    ref = np.einsum('Yy,Xx,nYXc->nyxc', B.upsample_matrix(h), B.upsample_matrix(w), g.astype(np.float64))
    assert R.worst(got, ref) < 2.0 ** -21


def test_host_build_act_grad(cpu):
    rng = np.random.default_rng(11)
    x = np.concatenate([rng.standard_normal(4096).astype(np.float32), np.float32([0.0, -0.0, -1.0, 1.0, -100.0, 100.0, -1e-30])])
    d = np.concatenate([rng.standard_normal(4096).astype(np.float32), np.float32([3.0, 3.0, 3.0, 3.0, 3.0, 3.0, 3.0])])
    for code, name in enumerate(ACTS):
        got = np.zeros_like(x)
        cpu.ftb_cpu_act_grad(ptr(x), ptr(d), x.size, code, ptr(got))
        want = B.act_grad_f32(x, d, name)
        if name == 'elu':                                        # (expf of the C library, within an ulp of NumPy's)
            assert np.allclose(got, want, rtol=3e-7, atol=0) and np.array_equal(got[x > 0], d[x > 0])
        else:
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    relu = np.zeros_like(x)
    cpu.ftb_cpu_act_grad(ptr(x), ptr(np.full_like(x, np.nan)), x.size, 1, ptr(relu))
    assert np.all(relu[x <= 0] == 0) and np.all(np.isnan(relu[x > 0]))          # a masked element is 0 whatever d is


def test_index_arithmetic_exhaustively(cpu):
    """All h, w in 1..40, two images: the gather writes every low pixel exactly once and reads g only inside it; the epilogue stores
    every low pixel exactly once per channel, inside da / db, at the pixel the accumulator register holds."""
    n = 2
    for h in range(1, 41):
        for w in range(1, 41):
            assert cpu.ftb_cpu_tiles(n, h, w) == n * -(-h // B.TILE_H) * -(-w // B.TILE_W)
            writes = np.zeros((n, h, w), np.int32)
            assert cpu.ftb_cpu_adjoint(None, n, h, w, None, ptr(writes)) == 0, (h, w)
            assert np.all(writes == 1), (h, w)
            for c, k in ((16, 0), (48, 47)):
                stores = np.zeros((n, h, w), np.int32)
                assert cpu.ftb_cpu_epilogue(n, h, w, c, k, ptr(stores)) == 0, (h, w, c, k)
                assert np.all(stores == 1), (h, w, c, k)


@pytest.mark.parametrize('shape', B.SHAPES, ids=str)
def test_restated_arithmetic_is_inside_the_bar(shape):
    a, b, weight, g, ref, e32 = B.case(shape)
    B.assert_at_bar(B.tail_bwd_f32(g, a, b, weight, shape[5]), ref, e32, f'restated {shape}')


def test_integer_case_is_exact_in_float32():
    a, b, weight, g = B.integer_case()
    ref = B.tail_bwd_ref(g, a, b, weight, None)
    got = B.tail_bwd_f32(g, a, b, weight, None)
    want32 = B.torch_tail_grads(g, a, b, weight, None, torch.float32)
    for name in ('da', 'db', 'g_low'):
        assert np.array_equal(got[name].astype(np.float64), ref[name]) and np.array_equal(want32[name].astype(np.float64), ref[name]), name
    assert 100 < max(np.abs(ref['da']).max(), np.abs(ref['db']).max()) < 2 ** 24


def defect_case(act):
    """The defect shape's inputs with every fourth element of a and b an exact zero (what tells x > 0 from x >= 0)."""
    shape = B.DEFECT_SHAPE[:5] + (act,)
    a, b, weight = R.tail_inputs(shape)
    a, b = a.copy(), b.copy()
    a.reshape(-1)[::4] = 0.0
    b.reshape(-1)[1::4] = 0.0
    g = B.cotangent(shape)
    ref = B.tail_bwd_ref(g, a, b, weight, act)
    e32 = B.errors(B.torch_tail_grads(g, a, b, weight, act, torch.float32), ref)
    return a, b, weight, g, ref, e32


@pytest.mark.parametrize('act', ('relu', 'elu'))
def test_the_clean_restatement_passes_on_the_defect_case(act):
    a, b, weight, g, ref, e32 = defect_case(act)
    B.assert_at_bar(B.tail_bwd_f32(g, a, b, weight, act), ref, e32, f'defect case {act}', names=('da', 'db', 'g_low'))


@pytest.mark.parametrize('mistake', B.MISTAKES)
def test_planted_defects_fail_the_bar(mistake):
    assert len(B.MISTAKES) >= 10
    act = 'relu' if mistake == 'mask_ge' else 'elu'
    a, b, weight, g, ref, e32 = defect_case(act)
    wrong = {k: v.astype(np.float32) for k, v in B.tail_bwd_ref(g, a, b, weight, act, mistake=mistake).items()}
    with pytest.raises(AssertionError):
        B.assert_at_bar(wrong, ref, e32, f'{mistake}', names=('da', 'db', 'g_low'))
