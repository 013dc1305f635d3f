"""The range guard of the fp16 two-piece field kernel, as far as it can be checked without a GPU: the new C symbols and their
argument validation, the two limits against NumPy's float16, the policy function, and the float64 range reference against the oracle."""
import ctypes
import itertools
import os
import re

import numpy as np
import pytest

from oracle import mvnerf_oracle as O
from thesis_clip_nerf_amd import _lib, range_policy as rp
from thesis_clip_nerf_amd.synthetic import make_scene

from tests.range_ref import operand_max, trunk64

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ['mvnerf_field_eval_split_ex', 'mvnerf_field_eval_stash_split_ex', 'mvnerf_render_fwd_split_ex', 'mvnerf_net_range']


def header_text():
    return open(os.path.join(ROOT, 'include', 'mvnerf_hip.h')).read()


def header_constant(name):
    m = re.search(r'#define\s+%s\s+([0-9.eE+-]+)f\b' % name, header_text())
    assert m, name
    return float(m.group(1))


def test_new_symbols_in_header_ctypes_table_and_library():
    code = re.sub(r'/\*.*?\*/', '', header_text(), flags=re.S)
    lib = _lib.lib()
    for name in NEW:
        assert re.search(r'\b%s\s*\(' % name, code), name
        assert name in _lib.SIGNATURES, name
        assert hasattr(lib, name), name
    for name in ('mvnerf_field_eval_split', 'mvnerf_field_eval_stash_split', 'mvnerf_render_fwd_split'):
        # the same arguments with `int which, float* range_status` in front of the stream
        old, new = _lib.SIGNATURES[name][1], _lib.SIGNATURES[name + '_ex'][1]
        assert new == old[:-1] + [ctypes.c_int, ctypes.c_void_p] + old[-1:], name
    assert header_constant('MVNERF_F16X3_MAX_WEIGHT') == _lib.F16X3_MAX_WEIGHT
    assert header_constant('MVNERF_F16X3_MAX_ACT') == _lib.F16X3_MAX_ACT


def test_ex_entry_points_validate_their_arguments_without_a_device():
    lib = _lib.lib()
    one, odd2, odd20 = ctypes.c_void_p(16), ctypes.c_void_p(18), ctypes.c_void_p(20)
    ins = [one] * 10
    dims = (1, 1, 4, 64, 8, 8)
    outs = [one, None, None, None, None, None, one]                     # rgbs, tap_idx, pix, embedding, acts x2, workspace

    def fe(ins=ins, outs=outs, which=-1, status=None):
        return lib.mvnerf_field_eval_split_ex(*ins, *dims, *outs, which, status, None)

    assert fe(ins=[None] + [one] * 9) == -1 and b'null' in lib.mvnerf_last_error()
    assert fe(which=7) == -1 and b'which=7' in lib.mvnerf_last_error()
    assert fe(which=-2) == -1 and b'which=-2' in lib.mvnerf_last_error()
    assert fe(status=odd2) == -3 and b'range_status' in lib.mvnerf_last_error()
    assert fe(ins=[one] * 4 + [odd20] + [one] * 5, status=odd2) == -3 and b'features' in lib.mvnerf_last_error()   # the older alignments first

    def st(ins=ins, which=-1, status=None, stash=one):
        return lib.mvnerf_field_eval_stash_split_ex(*ins, *dims, one, stash, one, which, status, None)

    assert st(stash=None) == -1 and b'null' in lib.mvnerf_last_error()
    assert st(which=7) == -1 and b'which=7' in lib.mvnerf_last_error()
    assert st(status=odd2) == -3

    def rf(which=-1, status=None, u=one):
        return lib.mvnerf_render_fwd_split_ex(*([one] * 10), u, one, 1, 1, 4, 64, 8, 8, 0.3, 1.3, 0, one, one, one, one, one, None, 0,
                                              which, status, None)

    assert rf(u=None) == -1 and b'null' in lib.mvnerf_last_error()
    assert rf(which=7) == -1 and b'which=7' in lib.mvnerf_last_error()
    assert rf(status=odd2) == -3 and b'range_status' in lib.mvnerf_last_error()

    assert lib.mvnerf_net_range(None, one, None) == -1 and b'null' in lib.mvnerf_last_error()
    assert lib.mvnerf_net_range(one, odd2, None) == -3


def test_float16_pins_the_two_limits():
    """rn16 overflows to infinity from 65520 upward: float16(64 w) is finite exactly for |w| < 1023.75, float16(v / 64) exactly
    for v < 4193280; the header's constants are those thresholds, slightly conservative."""
    w_exact, a_exact = 65520.0 / 64.0, 65520.0 * 64.0
    assert (w_exact, a_exact) == (1023.75, 4193280.0)
    with np.errstate(over='ignore'):
        for exact, cut in ((w_exact, lambda v: np.float16(np.float32(64.0) * v)), (a_exact, lambda v: np.float16(v / np.float32(64.0)))):
            at = np.float32(exact)
            under = np.nextafter(at, np.float32(0.0))
            assert np.isinf(cut(at)) and np.isinf(cut(-at)) and np.isinf(cut(np.nextafter(at, np.float32(np.inf))))
            assert np.isfinite(cut(under)) and np.isfinite(cut(-under))
            grid = np.linspace(0.0, 2.0 * exact, 4001, dtype=np.float32)
            assert np.array_equal(np.isfinite(cut(grid)), grid < at)
    for name, exact in (('MVNERF_F16X3_MAX_WEIGHT', w_exact), ('MVNERF_F16X3_MAX_ACT', a_exact)):
        c = header_constant(name)
        assert 0.999 * exact <= c <= exact, (name, c)


def test_policy_truth_table():
    w_lim, a_lim = rp.limits()
    assert (w_lim, a_lim) == (_lib.F16X3_MAX_WEIGHT, _lib.F16X3_MAX_ACT)
    assert rp.limits(training=True) == (w_lim, w_lim)
    values = {'none': None, 'in': 1.0, 'nan': float('nan'), 'inf': float('inf')}
    for policy, kernel, training in itertools.product(rp.POLICIES, ('split_f16', 'split_bf16', 'mfma_f32'), (False, True)):
        a_edge = w_lim if training else a_lim
        w_cases = dict(values, edge=w_lim, under=float(np.nextafter(np.float32(w_lim), np.float32(0))))
        a_cases = dict(values, edge=a_edge, under=float(np.nextafter(np.float32(a_edge), np.float32(0))))
        for (wn, w), (an, a) in itertools.product(w_cases.items(), a_cases.items()):
            ok = wn in ('none', 'in', 'under') and an in ('none', 'in', 'under')
            assert rp.in_range(w, a, training) == ok, (wn, an, training)
            if policy == 'off' or kernel != 'split_f16' or ok:
                want = rp.RUN
            elif policy == 'raise' or training:
                want = rp.RAISE
            else:
                want = rp.FALLBACK
            assert rp.decide(policy, kernel, w, a, training) == want, (policy, kernel, training, wn, an)
    # a pre-activation of 2000 passes the forward's limit and fails the backward's
    assert rp.decide('fallback', 'split_f16', 1.0, 2000.0) == rp.RUN
    assert rp.decide('fallback', 'split_f16', 1.0, 2000.0, training=True) == rp.RAISE
    assert '1023' in rp.describe(1.0, 2000.0, training=True) and '2000' in rp.describe(1.0, 2000.0, training=True)
    assert '4.19e+06' in rp.describe(None, 5e6) and 'weight' in rp.describe(2000.0, None)
    with pytest.raises(ValueError):
        rp.decide('sometimes', 'split_f16', 1.0, 1.0)


@pytest.mark.parametrize('views', [1, 3])
def test_range_reference_against_the_oracle(views):
    """range_ref.trunk64's eight activations against the oracle's complete_output, at the oracle's precision: fp32 dot products of up to
    K = 379 terms through 13 layers, so |difference| <= 13 * 379 * 2^-24 * max |x| (each layer's worst-case rounding, added up)."""
    sc = make_scene(seed=5, n_views=views, height=8, width=8, n_rays=6, bias_scale=0.1)
    rng = np.random.default_rng(0)
    z = np.sort(rng.uniform(0.3, 1.3, (1, 6, 64)).astype(np.float32), -1)
    t = trunk64(sc['coarse'], sc['rays_o'], sc['rays_d'], z, sc['images'], sc['features'], sc['intrinsics'], sc['extrinsics_inv'])
    net = O.unflatten_net(sc['coarse'])
    norm_images = (sc['images'] * np.float32(2.0) - np.float32(1.0)).astype(np.float32)
    world = O.points_on_rays(sc['rays_o'], sc['rays_d'], z)
    pix, cam = O.compute_pixel_in_image_mv(world, sc['intrinsics'], sc['extrinsics_inv'])
    feat = O.get_projection_features_mv(norm_images, sc['features'], pix)
    cdir = O.world_to_camera_direction_vector_mv(sc['rays_d'], sc['extrinsics_inv'])
    cdir = np.broadcast_to(cdir[:, :, :, None, :], cam.shape[:-1] + (3,))
    outs = O.mv_embedding(net, cam[..., :3].reshape(views, 6, 64, 3), cdir.reshape(views, 6, 64, 3), feat.reshape(views, 6, 64, -1), views,
                          complete_output=True)
    assert len(outs) == len(t['x']) == 8
    for got, ref in zip(t['x'], outs):
        bound = 13 * 379 * 2.0 ** -24 * float(np.abs(ref).max())
        assert got.shape == ref.shape and float(np.abs(got - ref).max()) <= bound
    # the operand set: the table form leaves the gathered features out, and nothing else
    assert operand_max(t, table=True) <= operand_max(t, table=False)
    big = dict(t, feat=t['feat'] * 1e3)
    assert operand_max(big, table=False) == pytest.approx(float(np.abs(big['feat']).max()))
    assert operand_max(big, table=True) == operand_max(t, table=True)
