"""The grasp-pose optimisation step behind the C ABI (csrc/grasp_api.hip, csrc/grasp_tail.hip, mvnerf_grasp_head_vjp_acts): the symbols
are exported and listed in the ctypes table, the Python mirror of mvnerf_grasp_call has the header's layout, and every entry point refuses
bad arguments with the documented code before it touches a device - no GPU here, as tests/test_abi.py does for the older symbols."""
import ctypes

import pytest

from thesis_clip_nerf_amd import _lib

NEW = ['mvnerf_grasp_tail_packed_floats', 'mvnerf_grasp_tail_pack', 'mvnerf_grasp_tail_fwd', 'mvnerf_grasp_tail_vjp', 'mvnerf_grasp_head_vjp_acts',
       'mvnerf_grasp_workspace_bytes', 'mvnerf_grasp_success', 'mvnerf_grasp_success_and_gradients', 'mvnerf_grasp_opt_step']
E_ARG, E_SHAPE, E_ALIGN = -1, -2, -3


def test_new_entry_points_are_exported_and_in_the_table():
    lib = _lib.lib()
    for name in NEW:
        assert name in _lib.SIGNATURES, name
        assert hasattr(lib, name), name
    assert lib.mvnerf_abi_version() == 1


def test_packed_tail_and_workspace_sizes():
    lib = _lib.lib()
    assert lib.mvnerf_grasp_tail_packed_floats(42) >= 2688 * 192 + 128 * 64 + 2 * 64 * 64 + 64
    assert lib.mvnerf_grasp_tail_packed_floats(1) >= 64 * 192 + 128 * 64 + 2 * 64 * 64 + 64
    assert lib.mvnerf_grasp_tail_packed_floats(0) == 0
    assert lib.mvnerf_grasp_workspace_bytes(1, 1, 0, 42) == 0 and lib.mvnerf_grasp_workspace_bytes(1, 1, 32, 0) == 0
    small = lib.mvnerf_grasp_workspace_bytes(1, 1, 37, 42)
    # at least the tensors the header lists: stash, acts, c, y, g_x, g_acts (per point) and the tail stash (per pose)
    n = 37 * 42
    assert small >= lib.mvnerf_stash_bytes(1, 1, n, 1) + n * (512 + 256 + 64 + 64 + 512) * 4 + 37 * 320 * 4
    assert small < lib.mvnerf_grasp_workspace_bytes(3, 1, 37, 42)
    # V > 1 pads every scene to whole 32-point tiles
    assert lib.mvnerf_grasp_workspace_bytes(1, 2, 37, 42) >= lib.mvnerf_stash_bytes(1, 2, (n + 31) // 32 * 32, 1)


def test_grasp_call_mirror_has_the_header_layout():
    c = _lib.GraspCall()
    # include/mvnerf_hip.h (LP64): 4 pointers, 4 ints, 8 pointers, 3 ints (+ 4 bytes of padding), 6 pointers, size_t
    assert ctypes.sizeof(c) == 4 * 8 + 4 * 4 + 8 * 8 + 3 * 4 + 4 + 6 * 8 + 8
    assert _lib.GraspCall.P.offset == 4 * 8 + 4 * 4 + 8 * 8 + 4 and _lib.GraspCall.t.offset == 4 * 8 + 4 * 4 + 8 * 8 + 16
    assert [n for n, _ in _lib.GraspCall._fields_] == [
        'images', 'features', 'intrinsics', 'extrinsics_inv', 'B', 'V', 'H', 'W', 'packed_net', 'split', 'bwd_streams', 'head_packed', 'head_b4',
        'head_bc', 'tail_packed', 'offsets', 'rep', 'P', 'n5', 't', 'rot', 'success', 'g_t', 'g_rot', 'workspace', 'workspace_bytes']


def test_tail_and_head_entry_points_validate_their_arguments():
    lib = _lib.lib()
    one, odd = ctypes.c_void_p(256), ctypes.c_void_p(260)
    w = [one] * 10
    assert lib.mvnerf_grasp_tail_pack(*w, None, 42, None, None) == E_ARG and b'mvnerf_grasp_tail_pack' in lib.mvnerf_last_error()
    assert lib.mvnerf_grasp_tail_pack(None, *w[1:], None, 42, one, None) == E_ARG
    assert lib.mvnerf_grasp_tail_pack(*w, None, 0, one, None) == E_ARG and b'n5=0' in lib.mvnerf_last_error()
    assert lib.mvnerf_grasp_tail_pack(*w, None, 42, odd, None) == E_ALIGN
    assert lib.mvnerf_grasp_tail_fwd(None, one, 32, 42, one, None, None) == E_ARG and b'mvnerf_grasp_tail_fwd' in lib.mvnerf_last_error()
    assert lib.mvnerf_grasp_tail_fwd(one, one, 0, 42, one, None, None) == E_ARG and b'M=0' in lib.mvnerf_last_error()
    assert lib.mvnerf_grasp_tail_fwd(one, one, 32, 0, one, None, None) == E_ARG
    assert lib.mvnerf_grasp_tail_fwd(odd, one, 32, 42, one, None, None) == E_ALIGN
    assert lib.mvnerf_grasp_tail_fwd(one, one, 32, 42, one, odd, None) == E_ALIGN              # the optional stash
    assert lib.mvnerf_grasp_tail_vjp(one, None, None, one, 32, 42, one, None) == E_ARG and b'mvnerf_grasp_tail_vjp' in lib.mvnerf_last_error()
    assert lib.mvnerf_grasp_tail_vjp(one, None, one, one, 32, -1, one, None) == E_ARG
    assert lib.mvnerf_grasp_tail_vjp(one, None, one, one, 32, 42, odd, None) == E_ALIGN
    assert lib.mvnerf_grasp_head_vjp_acts(one, one, one, one, 32, None, None) == E_ARG and b'mvnerf_grasp_head_vjp_acts' in lib.mvnerf_last_error()
    assert lib.mvnerf_grasp_head_vjp_acts(one, one, one, one, 0, one, None) == E_ARG
    assert lib.mvnerf_grasp_head_vjp_acts(one, one, one, one, 32, odd, None) == E_ALIGN
    # the existing entry still refuses NULL outputs
    assert lib.mvnerf_grasp_head_vjp(one, one, one, one, 32, None, None, None, one, None) == E_ARG


def filled_call():
    c = _lib.GraspCall()
    for name, kind in _lib.GraspCall._fields_:
        if kind is ctypes.c_void_p:
            setattr(c, name, 256)
    c.B, c.V, c.H, c.W, c.rep, c.P, c.n5 = 1, 1, 8, 8, 0, 37, 42
    c.workspace_bytes = _lib.lib().mvnerf_grasp_workspace_bytes(1, 1, 37, 42)
    return c


@pytest.mark.parametrize('entry', ['mvnerf_grasp_success', 'mvnerf_grasp_success_and_gradients', 'mvnerf_grasp_opt_step'])
def test_step_entry_points_validate_their_struct(entry):
    lib = _lib.lib()
    fn = getattr(lib, entry)
    cfg = _lib.PoseAdamConfig()
    one = ctypes.c_void_p(256)
    extra = [ctypes.byref(cfg)] + [one] * 6 if entry == 'mvnerf_grasp_opt_step' else []
    call = lambda c: fn(ctypes.byref(c) if c is not None else None, *extra, None)
    name = entry.encode()
    assert call(None) == E_ARG and name in lib.mvnerf_last_error()
    assert call(_lib.GraspCall()) == E_ARG and b'null pointer' in lib.mvnerf_last_error() and name in lib.mvnerf_last_error()
    for field in ('features', 'split', 'tail_packed', 'offsets', 't', 'success', 'workspace'):
        c = filled_call()
        setattr(c, field, None)
        assert call(c) == E_ARG, field
    for field, bad in (('P', 0), ('P', -3), ('n5', 0), ('n5', -1), ('B', 0), ('H', 1)):
        c = filled_call()
        setattr(c, field, bad)
        assert call(c) == E_ARG and (field + '=').encode() in lib.mvnerf_last_error(), field
    for rep in (-1, 2):
        c = filled_call()
        c.rep = rep
        assert call(c) == E_SHAPE and b'rep=' in lib.mvnerf_last_error() and name in lib.mvnerf_last_error()
    for field, bad in (('features', 260), ('tail_packed', 264), ('head_packed', 260), ('t', 258), ('workspace', 16)):
        c = filled_call()
        setattr(c, field, bad)
        assert call(c) == E_ALIGN and name in lib.mvnerf_last_error(), field
    c = filled_call()
    c.workspace_bytes -= 1
    assert call(c) == E_ARG and b'workspace' in lib.mvnerf_last_error() and name in lib.mvnerf_last_error()
    if entry != 'mvnerf_grasp_success':                      # the gradients' outputs are needed from stage 5 on
        c = filled_call()
        c.g_rot = None
        assert call(c) == E_ARG and b'g_rot' in lib.mvnerf_last_error()
    if entry == 'mvnerf_grasp_opt_step':
        c = filled_call()
        assert fn(ctypes.byref(c), None, one, one, one, one, one, one, None) == E_ARG and b'mvnerf_grasp_opt_step' in lib.mvnerf_last_error()
        assert fn(ctypes.byref(c), ctypes.byref(cfg), one, None, one, one, one, one, None) == E_ARG


def test_compile_rejects_a_fused_flag_that_is_not_a_bool():
    torch = pytest.importorskip('torch')
    from thesis_clip_nerf_amd.grasp_optimizer import DNGFOptimizer

    class Grasper:                       # compile() reads nothing of the model
        n_views, device_ = 1, torch.device('cpu')

    opt = DNGFOptimizer(Grasper(), n_initial_guesses=4, n_images=1)
    for bad in ('x', 1, 0, 'True'):
        with pytest.raises(ValueError, match='fused'):
            opt.compile(fused=bad)
    assert opt._fused is False
    opt.compile(fused=True)
    assert opt._fused is True
    opt.compile()                                            # None keeps the mode (compute_results compiles again)
    assert opt._fused is True
    opt._graph = object()
    opt.compile(fused=False)                                 # changing it drops a captured graph
    assert opt._fused is False and opt._graph is None
