"""The LanguageNeRF training step with its optimiser behind the C ABI (csrc/language_opt.hip): the symbols are in the header, the ctypes
table and the library, the Python mirror of mvnerf_language_adam has the header's layout, both entry points refuse bad arguments with the
documented code and a message naming the field before they touch a device, and LanguageNeRF.compile handles fused_optimizer - no GPU
here.  Conventions of tests/test_language_step_abi.py."""
import ctypes
import re

import numpy as np
import pytest

from tests.test_language_step_abi import E_ALIGN, E_ARG, filled_call
from thesis_clip_nerf_amd import _lib

NEW = ['mvnerf_language_apply_gradients', 'mvnerf_language_train_step']
FIELDS = ['head_w', 'head_b', 'head_wc', 'head_bc', 'tail_w', 'head_w4', 'head_b4', 'm', 'v', 'step', 'lr', 'beta1', 'beta2', 'eps', 'clip']
ARRAYS = {'head_w': 4, 'head_b': 4, 'tail_w': 11}


def test_new_entry_points_are_in_the_header_the_table_and_the_library():
    lib = _lib.lib()
    header = open(_lib.HEADER_PATH).read()
    for name in NEW:
        assert re.search(r'\b' + name + r'\(', header), name
        assert name in _lib.SIGNATURES, name
        assert hasattr(lib, name), name
    assert 'typedef struct mvnerf_language_adam' in header
    assert lib.mvnerf_abi_version() == 1                         # additive
    assert lib.mvnerf_language_workspace_bytes(2, 1, 16, 20, 3, 42) == filled_call().workspace_bytes


def test_language_adam_mirror_has_the_header_layout():
    header = open(_lib.HEADER_PATH).read()
    body = header[header.index('typedef struct mvnerf_language_adam {'):header.index('} mvnerf_language_adam;')]
    body = re.sub(r'/\*.*?\*/', '', body, flags=re.S)
    declared, counts = [], {}
    for stmt in body.split('{', 1)[1].split(';'):
        names = re.sub(r'^\s*(const\s+)?(float|void|int|long long|size_t)\s*\*?', '', stmt.strip())
        for n in names.split(','):
            if n.strip():
                size = re.search(r'\[(\d+)\]', n)
                name = re.sub(r'[\s\*]|\[\d+\]', '', n)
                declared.append(name)
                if size:
                    counts[name] = int(size.group(1))
    assert declared == FIELDS and counts == ARRAYS
    a = _lib.LanguageAdam
    assert [n for n, _ in a._fields_] == FIELDS
    # LP64: 4 + 4 + 2 + 11 + 5 pointers, 5 floats (+ 4 bytes of padding)
    assert ctypes.sizeof(a) == 26 * 8 + 5 * 4 + 4
    assert a.head_w.offset == 0 and a.head_b.offset == 32 and a.head_wc.offset == 64 and a.tail_w.offset == 80 and a.tail_w.size == 88
    assert a.head_w4.offset == 168 and a.m.offset == 184 and a.step.offset == 200 and a.lr.offset == 208 and a.clip.offset == 224


def filled_adam():
    a = _lib.LanguageAdam()
    for name, n in ARRAYS.items():
        for i in range(n):
            getattr(a, name)[i] = 256
    for name in ('head_wc', 'head_bc', 'head_w4', 'head_b4', 'm', 'v', 'step'):
        setattr(a, name, 256)
    a.lr, a.beta1, a.beta2, a.eps, a.clip = 1e-3, 0.9, 0.999, 1e-7, 1.0
    return a


ENTRY_POINTS = [('mvnerf_language_apply_gradients', False), ('mvnerf_language_train_step', True)]


@pytest.mark.parametrize('name,whole', ENTRY_POINTS)
def test_entry_points_validate_the_adam_struct(name, whole):
    lib = _lib.lib()
    fn = getattr(lib, name)
    ref = lambda x: ctypes.byref(x) if x is not None else None
    call = lambda c, a: fn(ref(c), ref(a), None)
    said = lambda text: text.encode() in lib.mvnerf_last_error()
    assert call(None, filled_adam()) == E_ARG and said(name) and said('null call')
    assert call(filled_call(), None) == E_ARG and said(name) and said('null adam')
    c = filled_call()
    c.grads = None
    assert call(c, filled_adam()) == E_ARG and said('grads')
    for bad in (0, 5000):
        c = filled_call()
        c.n5 = bad
        assert call(c, filled_adam()) == E_ARG and said(f'n5={bad}')
    for field in ('head_wc', 'head_bc', 'head_w4', 'head_b4', 'm', 'v', 'step'):
        a = filled_adam()
        setattr(a, field, None)
        assert call(filled_call(), a) == E_ARG and said('null pointer') and said(f'({field})'), field
        a = filled_adam()
        setattr(a, field, 258)
        assert call(filled_call(), a) == E_ALIGN and said(f'{field} must be'), field
    a = filled_adam()
    a.step = 260                                                 # a 64-bit word
    assert call(filled_call(), a) == E_ALIGN and said('step must be 8-byte aligned')
    for field, n in ARRAYS.items():
        for i in range(n):
            a = filled_adam()
            getattr(a, field)[i] = None
            assert call(filled_call(), a) == E_ARG and said(f'{field}[{i}]'), (field, i)
            a = filled_adam()
            getattr(a, field)[i] = 257
            assert call(filled_call(), a) == E_ALIGN and said(f'{field}[{i}]'), (field, i)
    for field, bad, shown in (('lr', -1e-3, 'lr=-0.001'), ('lr', float('nan'), 'lr=nan'), ('beta1', 1.0, 'beta1=1'), ('beta1', -0.5, 'beta1=-0.5'),
                              ('beta2', 1.5, 'beta2=1.5'), ('beta2', float('nan'), 'beta2=nan'), ('eps', -1e-7, 'eps=-1e-07')):
        a = filled_adam()
        setattr(a, field, bad)
        assert call(filled_call(), a) == E_ARG and said(shown), (field, lib.mvnerf_last_error())
    c = filled_call()
    c.grads = 258
    assert call(c, filled_adam()) == E_ALIGN and said('grads')


def test_apply_reads_only_grads_and_n5_of_the_call():
    """mvnerf_language_apply_gradients on an otherwise empty call gets as far as a bad adam struct; the whole step checks the call too."""
    lib = _lib.lib()
    c = _lib.LanguageCall()
    c.grads, c.n5 = 256, 7
    a = filled_adam()
    a.eps = -1.0
    assert lib.mvnerf_language_apply_gradients(ctypes.byref(c), ctypes.byref(a), None) == E_ARG and b'eps=-1' in lib.mvnerf_last_error()
    assert lib.mvnerf_language_train_step(ctypes.byref(c), ctypes.byref(filled_adam()), None) == E_ARG
    msg = lib.mvnerf_last_error()
    assert b'mvnerf_language_loss_and_grads' in msg and b'null pointer' in msg


def test_train_step_wants_the_calls_own_weight_pointers():
    lib = _lib.lib()
    step = lambda c, a: lib.mvnerf_language_train_step(ctypes.byref(c), ctypes.byref(a), None)
    said = lambda text: text.encode() in lib.mvnerf_last_error()
    for field in ('head_w4', 'head_b4', 'head_wc', 'head_bc'):
        a = filled_adam()
        setattr(a, field, 512)
        assert step(filled_call(), a) == E_ARG and said('mvnerf_language_train_step') and said(f'adam->{field} is not call->{field}'), field
    for i in range(11):
        a = filled_adam()
        a.tail_w[i] = 512
        assert step(filled_call(), a) == E_ARG and said(f'adam->tail_w[{i}] is not call->tail_w[{i}]'), i
    c = filled_call()                                            # the call's own checks come before the comparison and before any launch
    c.rep = 2
    assert step(c, filled_adam()) == -2 and said('rep=2')
    c = filled_call()
    c.workspace_bytes -= 1
    assert step(c, filled_adam()) == E_ARG and said('mvnerf_language_workspace_bytes')


def test_compile_takes_fused_optimizer_without_a_device():
    torch = pytest.importorskip('torch')
    from thesis_clip_nerf_amd import ops
    from thesis_clip_nerf_amd.lmvnerf import LanguageNeRF
    model = LanguageNeRF(np.zeros(_lib.NET_PARAMS, np.float32), n_points_train=2, device='cpu')
    assert model.fused_optimizer is False
    for bad in ('x', 1, 0):
        with pytest.raises(ValueError, match='fused_optimizer'):
            model.compile(fused_optimizer=bad)
        with pytest.raises(ValueError, match='fused_optimizer'):
            model.set_fused_optimizer(bad)
    with pytest.raises(ValueError, match='fused_optimizer'):     # needs the fused step
        model.compile(fused_optimizer=True)
    with pytest.raises(ValueError, match='fused_optimizer'):
        model.compile(fused_optimizer=True, fused_step=False)
    assert model.fused_optimizer is False and model.fused_step is False and model.optimizer is None
    own = torch.optim.SGD(model.grasp_readout.parameters(), lr=0.1)
    with pytest.raises(ValueError, match='fused_optimizer'):     # and is its own optimizer
        model.compile(fused_optimizer=True, fused_step=True, optimizer=own)
    assert model.fused_step is False                             # a refused compile() changes nothing
    with pytest.raises(RuntimeError, match='fused_optimizer'):
        model.optimizer_steps()
    model.compile(fused_step=True, fused_optimizer=True, learning_rate=3e-4)
    assert model.fused_optimizer is True and model.fused_step is True and model.optimizer is None
    total = ops.language_grad_layout(model.n_transforms_to_check)[1]
    state = model._opt
    assert state['m'].shape == (total,) and state['v'].shape == (total,) and state['step'].dtype == torch.int64
    assert not state['m'].any() and not state['v'].any() and model.optimizer_steps() == 0 and state['lr'] == 3e-4
    model.compile()                                              # None keeps the flag; compile() starts new moments
    assert model.fused_optimizer is True and model._opt is not state and model.optimizer is None
    with pytest.raises(ValueError, match='fused_optimizer'):     # the step cannot leave while the optimizer needs it
        model.set_fused_step(False)
    with pytest.raises(ValueError, match='fused_optimizer'):
        model.compile(fused_step=False)
    assert [k for k, _ in model.grasp_readout.named_parameters()] == [k for k in model.grasp_readout.state_dict()]
    assert all(isinstance(p, torch.nn.Parameter) for p in model.grasp_readout.parameters())
    model._graph = object()
    model.set_fused_optimizer(False)                             # a change drops a captured graph and puts torch's Adam back
    assert model.fused_optimizer is False and model._graph is None and model._opt is None
    assert isinstance(model.optimizer, torch.optim.Adam) and model.optimizer.param_groups[0]['lr'] == 1e-4
    model._graph = object()
    model.set_fused_optimizer(False)                             # no change: nothing dropped
    assert model._graph is not None
    model.compile(fused_optimizer=False, fused_step=False)
    assert model.fused_step is False and isinstance(model.optimizer, torch.optim.Adam)
