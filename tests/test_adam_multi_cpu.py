"""The multi-tensor optimiser step without a GPU: the host build of csrc/mvnerf_adam.h's warmup_rate, multi_plan and
multi_find (tests/cpu_adam_multi) bit for bit against the NumPy restatements of tests/adam_multi_ref.py, a whole restated step inside
language_adam_ref.bars per element, and planted defects against that bar or against bit-equality.  No kernel uses this code yet."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from tests import adam_multi_ref as R
from tests import language_adam_ref as A

HERE = os.path.dirname(os.path.abspath(__file__))
F32 = np.float32
C = R.CHUNK
# every length class of the kernel, empty entries first, last and adjacent
LENGTHS = (0, 1, 3, 0, 0, 4, C - 1, C, C + 1, 2 * C + 5, 0)
NO_GRAD = (7,)                                                      # the full-chunk tensor has no gradient
HYPER = dict(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-7, clip=1.0)
DIV_FIRST_CASES = ((0.006948058493435383, 24, 13), (0.0022889229003340006, 112, 34), (0.0008216166170313954, 176, 49))


@pytest.fixture(scope='module')
def cpu():
    d = os.path.join(HERE, 'cpu_adam_multi')
    subprocess.run(['make', '-C', d], check=True, capture_output=True)
    lib = ctypes.CDLL(os.path.join(d, 'libmvnerf_adam_multi_cpu.so'))
    lib.multi_cpu_chunk.restype = ctypes.c_longlong
    lib.multi_cpu_warmup_rate.restype = ctypes.c_float
    lib.multi_cpu_warmup_rate.argtypes = [ctypes.c_float, ctypes.c_double, ctypes.c_double, ctypes.c_longlong]
    lib.multi_cpu_plan.restype, lib.multi_cpu_plan.argtypes = ctypes.c_longlong, [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]
    lib.multi_cpu_find.restype, lib.multi_cpu_find.argtypes = ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong]
    lib.multi_cpu_step.restype = None
    lib.multi_cpu_step.argtypes = ([ctypes.c_void_p] * 6 + [ctypes.c_int, ctypes.c_void_p, ctypes.c_float, ctypes.c_double, ctypes.c_double] +
                                   [ctypes.c_float] * 4)
    return lib


def bits(x):
    return np.asarray(x, F32).tobytes()


SCHEDULES = [((2, 3), range(0, 6)),
             ((10000, 450000), (0, 1, 2, 3, 9999, 10000, 10001, 10002, 449999, 450000, 450001, 450002)),
             ((0, -1), (0, 1, 2, 10 ** 6))]


@pytest.mark.parametrize('shape,steps', SCHEDULES)
def test_host_warmup_rate_matches_the_float64_restatement_bit_for_bit(cpu, shape, steps):
    warm, after = shape
    for target in (1e-5, 1e-3, 0.3):
        for step in steps:
            got, want = F32(cpu.multi_cpu_warmup_rate(target, warm, after, step)), R.warmup32(target, warm, after, step)
            assert bits(got) == bits(want), (target, shape, step, float(got), float(want))
    t = F32(1e-5)
    rate = lambda step: F32(cpu.multi_cpu_warmup_rate(t, warm, after, step))
    if warm > 0:
        assert rate(0) == 0.0                                       # Keras reads the schedule at `iterations`: the first update has rate 0
        assert rate(warm) == t and rate(warm + 1) == t              # target * warm / warm, then the plateau
        assert 0 < rate(1) < t
    else:
        assert rate(0) == t                                         # warm <= 0: no warm-up
    if after >= 0:
        assert rate(after) == t and bits(rate(after + 1)) == bits(F32(np.float64(t) * 0.1)) and rate(after + 2) == rate(after + 1)
    else:
        assert rate(10 ** 9) == t                                   # after < 0: the rate never drops


def test_warmup_rate_is_the_reference_schedule():
    """nerf_utils.WarmupScheduler (float32, step / warm * target) and encoders.warmup_lr_lambda (double factor times the rate): the same
    schedule up to their own roundings - 2 ulp of float32."""
    from thesis_clip_nerf_amd.encoders import warmup_lr_lambda
    from thesis_clip_nerf_amd.nerf_utils import WarmupScheduler
    ref, lam = WarmupScheduler(1e-5, 10, 20), warmup_lr_lambda(10, 20)
    for step in range(25):
        want = float(R.warmup32(1e-5, 10, 20, step))
        assert abs(want - ref(step)) <= 2 * 2.0 ** -24 * 1e-5 and abs(want - 1e-5 * lam(step)) <= 2 * 2.0 ** -24 * 1e-5, step


def test_plan_and_find_against_searchsorted(cpu):
    assert cpu.multi_cpu_chunk() == C
    rng = np.random.default_rng(0)
    pool = (0, 1, 3, 4, C - 1, C, C + 1, 2 * C + 5)
    lists = [LENGTHS, (0, 0, 0, 5), (5, 0, 0, 0), (0,), (1,), (0, 0)] + [tuple(rng.choice(pool, rng.integers(1, 12))) for _ in range(40)]
    for lengths in lists:
        n = np.asarray(lengths, np.int64)
        first = np.full(n.size + 1, -7, np.int64)
        total = cpu.multi_cpu_plan(n.ctypes.data, n.size, first.ctypes.data)
        want = R.plan(lengths)
        assert (first == want).all() and total == want[-1] == sum(-(-int(k) // C) for k in lengths), lengths
        for chunk in range(int(total)):                             # exhaustively: every chunk belongs to a tensor that has it
            t = cpu.multi_cpu_find(first.ctypes.data, n.size, chunk)
            assert t == R.find(want, chunk), (lengths, chunk)
            assert n[t] > 0 and first[t] <= chunk < first[t + 1] and (chunk - first[t]) * C < n[t], (lengths, chunk, t)


def pointers(arrays):
    return (ctypes.c_void_p * len(arrays))(*[None if a is None else a.ctypes.data for a in arrays])


def host_step(cpu, tensors, counter, hyper, warm, after):
    out = [dict(p=t['p'].copy(), g=t['g'], m=t['m'].copy(), v=t['v'].copy()) for t in tensors]
    n = np.asarray([t['p'].size for t in out], np.int64)
    first = R.plan(n)
    step = np.asarray([counter], np.int64)
    c = A.f32_constants(hyper)
    cpu.multi_cpu_step(pointers([t['p'] for t in out]), pointers([t['g'] for t in out]), pointers([t['m'] for t in out]),
                       pointers([t['v'] for t in out]), n.ctypes.data, first.ctypes.data, n.size, step.ctypes.data, c['lr'], warm, after,
                       c['beta1'], c['beta2'], c['eps'], c['clip'])
    return out, int(step[0])


def same_bits(a, b):
    return all(bits(x[k]) == bits(y[k]) for x, y in zip(a, b) for k in 'pmv')


@pytest.mark.parametrize('counter', (0, 1, 2, 3, 4, 5))
def test_whole_step_host_build_restatement_and_bar(cpu, counter):
    """(warm, after) = (2, 3): rate 0, half, full, full, a tenth, a tenth.  Host build == restatement bit for bit; the restatement inside
    language_adam_ref.bars of the float64 step per element; the tensor without a gradient and the counter as they should be."""
    tensors = R.random_tensors(LENGTHS, 31 + counter, NO_GRAD)
    got, after_step = host_step(cpu, tensors, counter, HYPER, 2, 3)
    want, want_step = R.step32(tensors, counter, HYPER, 2, 3)
    assert after_step == want_step == counter + 1
    assert same_bits(got, want)
    ref = R.step64(tensors, counter, HYPER, 2, 3)
    for i, (r, w, t) in enumerate(zip(ref, want, tensors)):
        if r is None:
            assert i in NO_GRAD and all(bits(w[k]) == bits(t[k]) for k in 'pmv')
        else:
            assert R.outside(r, w) == 0, (i, LENGTHS[i])
    if counter == 0:                                                # the warm-up's first update: moments move, variables do not
        assert all(bits(w['p']) == bits(t['p']) for w, t in zip(want, tensors))
        assert any(bits(w['m']) != bits(t['m']) for w, t in zip(want, tensors))


@pytest.mark.parametrize('defect', R.DEFECTS)
def test_planted_defects_leave_the_bar_or_break_bit_equality(defect):
    assert len(R.DEFECTS) >= 8
    warm, after, hyper = 2, 3, HYPER
    # a counter at which the defect shows: inside the warm-up, at the drop, or anywhere
    counter = {'schedule_after_increment': 1, 'bias_at_step': 2, 'drop_at_after': 3}.get(defect, 2)
    if defect == 'div_first':
        # t * s / warm and t * (s / warm) both round once more to float32 and agree at most steps; three (target, warm, step) at which
        # the last bit differs, found by search (about 3 in a million of random ones do)
        for target, w, s in DIV_FIRST_CASES:
            assert bits(R.warmup32(target, w, -1, s)) != bits(R.warmup32(target, w, -1, s, defect)), (target, w, s)
        (target, warm, counter), after = DIV_FIRST_CASES[1], -1        # one where the corrected rate differs too
        hyper = dict(HYPER, lr=target)
    tensors = R.random_tensors(LENGTHS, 77, NO_GRAD)
    good, _ = R.step32(tensors, counter, hyper, warm, after)
    bad, _ = R.step32(tensors, counter, hyper, warm, after, defect=defect)
    assert not same_bits(good, bad), defect
    ref = R.step64(tensors, counter, hyper, warm, after)
    with_grad = [(r, g, b) for r, g, b in zip(ref, good, bad) if r is not None]
    assert sum(R.outside(r, g) for r, g, _ in with_grad) == 0
    over = sum(R.outside(r, b) for r, _, b in with_grad)
    print(defect, 'counter', counter, 'elements outside the bar:', over)
    if defect == 'null_grad_zeros':                                 # seen on the tensor the step must leave alone
        i = NO_GRAD[0]
        assert bits(good[i]['m']) == bits(tensors[i]['m']) and bits(bad[i]['m']) != bits(tensors[i]['m'])
        assert bits(bad[i]['p']) != bits(tensors[i]['p'])
    elif defect == 'div_first':                                     # one bit of the rate: bit-equality sees it, the bar need not
        assert bits(R.rates(hyper, warm, after, counter)[1]) != bits(R.rates(hyper, warm, after, counter, defect)[1])
    else:
        assert over > 0, defect
    if defect == 'empty_not_skipped':                               # the chunk lands on the empty entry in front: its owner is not updated
        assert bits(bad[5]['p']) == bits(tensors[5]['p']) and bits(good[5]['p']) != bits(tensors[5]['p'])
    if defect == 'tail_twice':                                      # only partial chunks: the full-chunk tensors are as they should be
        assert bits(bad[8]['p'][:C]) == bits(good[8]['p'][:C]) and bits(bad[8]['p'][C:]) != bits(good[8]['p'][C:])
