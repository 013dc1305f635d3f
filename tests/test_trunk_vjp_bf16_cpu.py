"""The bf16 trunk VJP without a GPU: the float64 references of tests/trunk_vjp_bf16_ref.py against float64 autograd, planted defects
against the bars the GPU tests use (tests/test_gpu_trunk_vjp_bf16.py), the relu-bit layout of include/mvnerf_hip.h restated, the argument
checks of the new entry points, compute_dtype validation and the double-backward error."""
import ctypes
import types

import numpy as np
import pytest
import torch

from oracle import field_bf16_ref as R
from oracle import mvnerf_oracle as O
from tests import trunk_vjp_bf16_ref as B
from thesis_clip_nerf_amd import _lib, ops
from thesis_clip_nerf_amd.synthetic import make_scene

E_ARG, E_SHAPE, E_ALIGN = -1, -2, -3
NEW = ['mvnerf_relu_bits_bytes', 'mvnerf_bwd_streams_bf16_bytes', 'mvnerf_pack_bwd_streams_bf16', 'mvnerf_query_stash_bf16',
       'mvnerf_trunk_vjp_bf16', 'mvnerf_query_vjp_bf16_scratch_bytes', 'mvnerf_query_vjp_bf16', 'mvnerf_grasp_workspace_bytes_bf16',
       'mvnerf_grasp_success_bf16', 'mvnerf_grasp_success_and_gradients_bf16', 'mvnerf_grasp_opt_step_bf16']
_case = {}


def case(views, n=40):
    """A Glorot net (make_scene's), x0 (views, n, 128) and cotangents (4, n, 128); the float64 forward's acts and bits."""
    if (views, n) not in _case:
        net = O.unflatten_net(make_scene(seed=3, height=8, width=8, n_rays=4, bias_scale=0.1)['fine'])
        rng = np.random.default_rng(10 + views)
        x0 = rng.standard_normal((views, n, 128))
        g_acts = rng.standard_normal((4, n, 128)).astype(np.float32)
        _, bits = B.forward64(net, x0)
        _case[views, n] = (net, x0, g_acts, bits)
    return _case[views, n]


@pytest.mark.parametrize('views', [1, 2, 3])
def test_chain_reference_equals_float64_autograd_of_the_bf16_weight_trunk(views):
    net, x0, g_acts, bits = case(views)
    ref = B.chain(net, g_acts, bits, views)
    auto = B.autograd64(net, x0, g_acts)
    err = np.abs(ref - auto).max() / np.abs(auto).max()
    print(f'V={views}: max |R - autograd| / max |autograd| = {err:.2e}')
    assert ref.shape == (views, 40, 128) and err < 1e-12


@pytest.mark.parametrize('views', [1, 3])
def test_emulation_is_close_and_planted_defects_fail_the_chain_bar(views):
    """The GPU bar is e_k <= 2 e_q with e_q = relL2(R_q - R): every planted defect in the emulation must miss it."""
    net, _, g_acts, bits = case(views)
    ref = B.chain(net, g_acts, bits, views)
    e_q = B.rel_l2(B.chain(net, g_acts, bits, views, quantize=True), ref)
    print(f'V={views}: e_q = {e_q:.3e}')
    assert 1e-4 < e_q < 1e-2                                 # bf16 operands: 2^-9 per rounding, averaged over 128-term sums
    for defect in B.DEFECTS:
        if defect == 'no_1_over_v' and views == 1:
            continue
        e_d = B.rel_l2(B.chain(net, g_acts, bits, views, quantize=True, defect=defect), ref)
        print(f'  {defect}: e = {e_d:.3e} = {e_d / e_q:.1f} e_q')
        assert e_d > 2 * e_q, defect


def test_block_reference_holds_the_emulation_and_refuses_block_level_defects():
    """block_bwd_ref at R.check's 16 * 2^-24 bar: the emulated block (same roundings) passes, fp32-sized noise passes, a block with a
    missing mask, swapped masks, a dropped residual or W in place of W^T does not."""
    net, _, g_acts, bits = case(1)
    g, blk = g_acts[3], net['blocks'][5]
    bits_h, bits_x = bits[6 + 5], bits[6 + 4]
    ref, und, flip = B.block_bwd_ref(g, blk, bits_h, bits_x)
    good = B._block(g.astype(np.float64), blk, bits_h, bits_x, True, None)
    fig = R.check(good, ref, und, flip, 'emulated block')
    assert fig['worst'] == 0.0
    noisy = good * (1 + 2.0 ** -24 * np.random.default_rng(0).uniform(-1, 1, good.shape))
    R.check(noisy, ref, und, flip, 'emulated block with fp32 noise')
    for defect in ('no_mask', 'swap_masks', 'no_residual', 'w_not_transposed'):
        bad = B._block(g.astype(np.float64), blk, bits_h, bits_x, True, defect)
        with pytest.raises(AssertionError):
            R.check(bad, ref, und, flip, defect)
    # one bf16 step on an undecided element is inside its window, on a decided one it is not
    assert und.mean() < 0.01


def test_torch_emulation_backward_equals_the_numpy_emulation():
    """Bf16 straight-through Functions: the torch block's input gradient is R_q's block, given the forward's own masks."""
    net, x0, g_acts, _ = case(1)
    blk = net['blocks'][4]
    x = torch.from_numpy(x0[0]).requires_grad_(True)
    w1, b1, w2, b2 = (torch.from_numpy(np.asarray(t, np.float64)) for t in blk)
    y = B.emulated_block(x, w1, b1, w2, b2)
    g = g_acts[2].astype(np.float64)
    y.backward(torch.from_numpy(g))
    xq = R.q(np.maximum(x0[0], 0))
    hid = xq @ R.q(blk[0]) + np.asarray(blk[1], np.float64)
    want = B._block(g, blk, hid > 0, x0[0] > 0, True, None)
    np.testing.assert_allclose(x.grad.numpy(), want, rtol=0, atol=1e-12 * np.abs(want).max())


# ---- the bit layout ------------------------------------------------------------------------------------------------------------------
def pack_by_the_header(on, b, v, n):
    """include/mvnerf_hip.h restated with loops: on (b, 6 v + 6, n, 128) bool -> the uint8 buffer."""
    n_tiles = -(-b * n // 32)
    words = np.zeros(((v + 1) * n_tiles, 6, 64), np.uint64)
    tiles_per_b = n_tiles // b if v > 1 else None
    for tile in range(n_tiles):
        for j in range(32):
            flat = tile * 32 + j
            if flat >= b * n:
                continue
            bb, i = divmod(flat, n)
            for slot in range(6):
                for vv in range(v + 1):                       # vv == v: the fused tensors
                    k = tile - bb * tiles_per_b if v > 1 else None
                    row = n_tiles * v + tile if vv == v else ((bb * v + vv) * tiles_per_b + k if v > 1 else tile)
                    feats = on[bb, 6 * vv + slot, i]
                    for h in range(2):
                        w = 0
                        for nb in range(4):
                            for r in range(16):
                                if feats[32 * nb + 8 * (r // 4) + 4 * h + r % 4]:
                                    w |= 1 << (16 * nb + r)
                        words[row, slot, 32 * h + j] = w
    return torch.from_numpy(words.view(np.uint8).reshape(-1))


@pytest.mark.parametrize('b,v,n', [(1, 1, 40), (2, 1, 40), (2, 2, 64), (1, 3, 32)])
def test_unpack_relu_bits_follows_the_documented_layout(b, v, n):
    on = np.random.default_rng(b + v + n).random((b, 6 * v + 6, n, 128)) < 0.5
    buf = pack_by_the_header(on, b, v, n)
    assert buf.numel() == _lib.lib().mvnerf_relu_bits_bytes(b, v, n)
    got = ops.unpack_relu_bits(buf, b, v, n)
    assert got.dtype == torch.bool and tuple(got.shape) == on.shape
    np.testing.assert_array_equal(got.numpy(), on)


# ---- the C ABI -----------------------------------------------------------------------------------------------------------------------
def test_new_entry_points_are_exported_sized_and_leave_the_abi_version():
    lib = _lib.lib()
    for name in NEW:
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
    assert lib.mvnerf_abi_version() == 1
    assert lib.mvnerf_bwd_streams_bf16_bytes() == 12 * 128 * 128 * 2
    # 1 bit where the fp32 stash keeps 4 bytes, for 6 of its 7 tensors per view and fused
    assert lib.mvnerf_relu_bits_bytes(1, 1, 32) == 12 * 512 and lib.mvnerf_relu_bits_bytes(2, 3, 64) == 4 * (6 * 3 + 6) * 512
    assert lib.mvnerf_relu_bits_bytes(1, 1, 40) == 2 * 12 * 512
    assert lib.mvnerf_relu_bits_bytes(0, 1, 32) == 0 and lib.mvnerf_query_vjp_bf16_scratch_bytes(1, 0, 32) == 0
    assert lib.mvnerf_query_vjp_bf16_scratch_bytes(2, 3, 64) == 4 * 3 * 128 * 32 * 4
    assert lib.mvnerf_grasp_workspace_bytes_bf16(1, 1, 0, 42) == 0
    assert 0 < lib.mvnerf_grasp_workspace_bytes_bf16(1, 1, 37, 42) < lib.mvnerf_grasp_workspace_bytes(1, 1, 37, 42)


def test_query_entry_points_validate_their_arguments():
    lib = _lib.lib()
    one, odd = ctypes.c_void_p(256), ctypes.c_void_p(260)
    err = lib.mvnerf_last_error
    assert lib.mvnerf_pack_bwd_streams_bf16(None, one, None) == E_ARG and b'mvnerf_pack_bwd_streams_bf16' in err()
    assert lib.mvnerf_pack_bwd_streams_bf16(one, odd, None) == E_ALIGN

    def stash(ptrs=None, sizes=(1, 1, 32, 8, 8), outs=None):
        return lib.mvnerf_query_stash_bf16(*(ptrs or [one] * 8), *sizes, *(outs or [one] * 3), None)
    assert stash(ptrs=[one] * 7 + [None]) == E_ARG and b'mvnerf_query_stash_bf16' in err()
    assert stash(outs=[one, None, one]) == E_ARG
    for sizes in ((0, 1, 32, 8, 8), (1, 0, 32, 8, 8), (1, 1, 0, 8, 8), (1, 1, 32, 1, 8)):
        assert stash(sizes=sizes) == E_ARG, sizes
    assert stash(sizes=(1, 2, 40, 8, 8)) == E_SHAPE and b'multiple of 32' in err()
    assert stash(sizes=(1, 1, 40, 8, 8), ptrs=[one, one, one, odd] + [one] * 4) == E_ALIGN
    assert stash(outs=[one, odd, one]) == E_ALIGN

    def trunk(ptrs=None, sizes=(1, 1, 32), out=one):
        return lib.mvnerf_trunk_vjp_bf16(*(ptrs or [one] * 3), *sizes, out, None)
    assert trunk(ptrs=[one, None, one]) == E_ARG and b'mvnerf_trunk_vjp_bf16' in err()
    assert trunk(out=None) == E_ARG
    assert trunk(sizes=(1, 1, 0)) == E_ARG
    assert trunk(sizes=(2, 3, 48)) == E_SHAPE
    assert trunk(sizes=(1, 1, 1 << 24)) == E_SHAPE and b'tiles' in err()
    assert trunk(ptrs=[odd, one, one]) == E_ALIGN and trunk(out=odd) == E_ALIGN

    def vjp(ptrs=None, sizes=(1, 1, 32, 8, 8), outs=None):
        return lib.mvnerf_query_vjp_bf16(*(ptrs or [one] * 10), *sizes, *(outs or [one] * 3), None)
    assert vjp(ptrs=[one] * 7 + [None, one, one]) == E_ARG and b'mvnerf_query_vjp_bf16' in err()
    assert vjp(outs=[one, one, None]) == E_ARG
    assert vjp(sizes=(1, 1, 32, 8, 1)) == E_ARG
    assert vjp(sizes=(1, 3, 33, 8, 8)) == E_SHAPE
    assert vjp(ptrs=[one] * 8 + [odd, one]) == E_ALIGN and vjp(outs=[odd, one, one]) == E_ALIGN


def filled_call():
    c = _lib.GraspCall()
    for name, kind in _lib.GraspCall._fields_:
        if kind is ctypes.c_void_p:
            setattr(c, name, 256)
    c.B, c.V, c.H, c.W, c.rep, c.P, c.n5 = 1, 1, 8, 8, 0, 37, 42
    c.workspace_bytes = _lib.lib().mvnerf_grasp_workspace_bytes_bf16(1, 1, 37, 42)
    return c


@pytest.mark.parametrize('entry', ['mvnerf_grasp_success_bf16', 'mvnerf_grasp_success_and_gradients_bf16', 'mvnerf_grasp_opt_step_bf16'])
def test_bf16_step_entry_points_validate_their_arguments(entry):
    lib = _lib.lib()
    fn = getattr(lib, entry)
    cfg = _lib.PoseAdamConfig()
    one, odd = ctypes.c_void_p(256), ctypes.c_void_p(264)
    extra = [ctypes.byref(cfg)] + [one] * 6 if entry == 'mvnerf_grasp_opt_step_bf16' else []
    call = lambda c, p16=one, b16=one: fn(ctypes.byref(c) if c is not None else None, p16, b16, *extra, None)
    name = entry.encode()
    assert call(None) == E_ARG and name in lib.mvnerf_last_error()
    assert call(filled_call(), p16=None) == E_ARG and b'packed16' in lib.mvnerf_last_error()
    assert call(filled_call(), b16=None) == E_ARG
    assert call(filled_call(), p16=odd) == E_ALIGN and call(filled_call(), b16=odd) == E_ALIGN
    for field in ('features', 'bwd_streams', 'tail_packed', 't', 'workspace'):
        c = filled_call()
        setattr(c, field, None)
        assert call(c) == E_ARG, field
    c = filled_call()
    c.P = 0
    assert call(c) == E_ARG and b'P=' in lib.mvnerf_last_error()
    c = filled_call()
    c.workspace_bytes -= 1
    assert call(c) == E_ARG and b'mvnerf_grasp_workspace_bytes_bf16' in lib.mvnerf_last_error()
    if entry == 'mvnerf_grasp_opt_step_bf16':
        assert fn(ctypes.byref(filled_call()), one, one, None, one, one, one, one, one, one, None) == E_ARG


# ---- Python --------------------------------------------------------------------------------------------------------------------------
def test_compute_dtype_is_validated_before_anything_runs():
    from thesis_clip_nerf_amd.grasp_optimizer import DNGFOptimizer
    from thesis_clip_nerf_amd.lmvnerf import TrunkState

    class Grasper:
        n_views, device_ = 1, torch.device('cpu')

    assert DNGFOptimizer(Grasper(), n_initial_guesses=4, n_images=1).compute_dtype == 'f32'
    assert DNGFOptimizer(Grasper(), n_initial_guesses=4, n_images=1, compute_dtype='bf16').compute_dtype == 'bf16'
    for bad in ('fp16', 'f16', None, torch.bfloat16):
        with pytest.raises(ValueError, match='compute_dtype'):
            DNGFOptimizer(Grasper(), n_initial_guesses=4, n_images=1, compute_dtype=bad)
        with pytest.raises(ValueError, match='compute_dtype'):
            TrunkState(None, None, None, None, None, compute_dtype=bad)


def test_the_second_derivative_of_a_bf16_state_is_refused():
    from thesis_clip_nerf_amd.lmvnerf import _TrunkVJP
    ctx = types.SimpleNamespace(state=types.SimpleNamespace(compute_dtype='bf16'), points=torch.zeros(1, 1, 3), dirs=torch.zeros(1, 1, 3))
    with pytest.raises(RuntimeError, match='no bf16 form'):
        _TrunkVJP.backward(ctx, torch.zeros(1, 1, 3), torch.zeros(1, 1, 3))
