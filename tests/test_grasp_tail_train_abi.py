"""The training passes of the per-pose read-out behind the C ABI (csrc/grasp_tail_train.hip) and LanguageNeRF.compile(fused_tail=...): the
symbols are exported and listed in the ctypes table, the entry points refuse bad arguments with the documented code and name themselves
before they touch a device, and the flag is validated - no GPU here, as tests/test_grasp_step_abi.py does for the frozen-weight tail."""
import ctypes

import pytest

from thesis_clip_nerf_amd import _lib

NEW = ['mvnerf_grasp_tail_vjp_train', 'mvnerf_grasp_tail_vjp_bwd']
E_ARG, E_ALIGN = -1, -3


def test_new_entry_points_are_exported_and_in_the_table():
    lib = _lib.lib()
    for name in NEW:
        assert name in _lib.SIGNATURES, name
        assert hasattr(lib, name), name
    assert len(_lib.SIGNATURES['mvnerf_grasp_tail_vjp_train'][1]) == 11 and len(_lib.SIGNATURES['mvnerf_grasp_tail_vjp_bwd'][1]) == 14
    assert lib.mvnerf_abi_version() == 1


def test_vjp_train_validates_its_arguments():
    lib = _lib.lib()
    fn, name = lib.mvnerf_grasp_tail_vjp_train, b'mvnerf_grasp_tail_vjp_train'
    one, odd, odd4 = ctypes.c_void_p(256), ctypes.c_void_p(260), ctypes.c_void_p(258)
    good = [one, None, one, one, 32, 42, one, one, one, one, None]       # x, g_s, stash, packed, M, n5, g_x, cot, act, ex, stream
    for i in (0, 2, 3, 6, 7, 8, 9):                                           # every pointer but g_s
        args = list(good)
        args[i] = None
        assert fn(*args) == E_ARG and name in lib.mvnerf_last_error() and b'null pointer' in lib.mvnerf_last_error(), i
    for m, n5, word in ((0, 42, b'M=0'), (-5, 42, b'M=-5'), ((1 << 24) + 1, 42, b'M='), (32, 0, b'n5=0'), (32, -1, b'n5=-1'), (32, 4097, b'n5=4097')):
        args = list(good)
        args[4], args[5] = m, n5
        assert fn(*args) == E_ARG and name in lib.mvnerf_last_error() and word in lib.mvnerf_last_error(), (m, n5)
    for i in (0, 2, 3, 6, 7, 8, 9):
        args = list(good)
        args[i] = odd
        assert fn(*args) == E_ALIGN and name in lib.mvnerf_last_error(), i
    args = list(good)
    args[1] = odd4                                                            # g_s: 4-byte alignment
    assert fn(*args) == E_ALIGN and name in lib.mvnerf_last_error()


def test_vjp_bwd_validates_its_arguments():
    lib = _lib.lib()
    fn, name = lib.mvnerf_grasp_tail_vjp_bwd, b'mvnerf_grasp_tail_vjp_bwd'
    one, odd, odd4 = ctypes.c_void_p(256), ctypes.c_void_p(260), ctypes.c_void_p(258)
    # x, t_x, g_s, stash, cot, packed, M, n5, out_gs, out_x, cot2, tan, dex, stream
    good = [one, one, None, one, one, one, 32, 42, one, None, one, one, one, None]
    for i in (0, 1, 3, 4, 5, 8, 10, 11, 12):                                  # every pointer but g_s and out_x
        args = list(good)
        args[i] = None
        assert fn(*args) == E_ARG and name in lib.mvnerf_last_error() and b'null pointer' in lib.mvnerf_last_error(), i
    for m, n5, word in ((0, 42, b'M=0'), (32, 0, b'n5=0'), (32, -1, b'n5=-1'), ((1 << 24) + 1, 1, b'M='), (32, 4097, b'n5=4097')):
        args = list(good)
        args[6], args[7] = m, n5
        assert fn(*args) == E_ARG and name in lib.mvnerf_last_error() and word in lib.mvnerf_last_error(), (m, n5)
    for i in (0, 1, 3, 4, 5, 9, 10, 11, 12):                                  # the optional out_x included
        args = list(good)
        args[i] = odd
        assert fn(*args) == E_ALIGN and name in lib.mvnerf_last_error(), i
    for i in (2, 8):                                                          # g_s, out_gs: 4 bytes
        args = list(good)
        args[i] = odd4
        assert fn(*args) == E_ALIGN, i


def test_compile_validates_and_applies_the_fused_tail_flag():
    torch = pytest.importorskip('torch')
    import numpy as np
    from thesis_clip_nerf_amd.lmvnerf import GraspReadout, LanguageNeRF

    assert GraspReadout.fused_tail is False and GraspReadout.fused_head is True          # the defaults
    model = LanguageNeRF(np.zeros(_lib.NET_PARAMS, np.float32), n_points_train=2, n_5d_poses=3, device='cpu')
    assert model.grasp_readout.fused_tail is False
    for bad in ('x', 1, 0, 'True', 1.0):
        with pytest.raises(ValueError, match='fused_tail'):
            model.compile(fused_tail=bad)
    assert model.grasp_readout.fused_tail is False and model.optimizer is None           # a refused call changes nothing
    model.compile(fused_tail=True)
    assert model.grasp_readout.fused_tail is True
    model.compile()                                                                      # None keeps the setting
    assert model.grasp_readout.fused_tail is True
    model._graph, model._g_calls = object(), 5
    model.compile(fused_tail=False)                                                      # a change drops a captured graph
    assert model.grasp_readout.fused_tail is False and model._graph is None and model._g_calls == 0
    assert GraspReadout.fused_tail is False                                              # the class default is untouched


def test_fused_tail_is_not_taken_off_the_gpu():
    """With the flag set, a CPU input still runs today's torch layers: the fused tail is for CUDA fp32 tensors only."""
    torch = pytest.importorskip('torch')
    from thesis_clip_nerf_amd.lmvnerf import GraspReadout

    torch.manual_seed(3)
    ro = GraspReadout(2)
    ro.fused_head = False
    acts = [torch.randn(1, 3, 2, 128) for _ in range(4)]
    want = ro(acts)
    ro.fused_tail = True
    assert torch.equal(ro(acts), want)
