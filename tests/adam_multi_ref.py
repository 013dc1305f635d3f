"""References of the multi-tensor optimiser step (csrc/mvnerf_adam.h: warmup_rate, multi_plan, multi_find - host/device code that no
kernel uses yet):

    lr_s = warmup_rate(lr, warm, after, step)        the schedule at the counter BEFORE its increment, in double, rounded to float once
    lr_t = adam_rate(lr_s, b1, b2, step + 1)         tests/language_adam_ref.rate32
    per element of every tensor with a gradient: language_adam_ref.update32 (clip, m, v, p), the tensor found chunk by chunk.

`warmup32` restates the schedule in NumPy float64, `plan` / `find` the chunk prefix and the lookup through numpy.searchsorted, `step32`
the whole step chunk by chunk as the kernel walks it, `step64` the same update in float64 with language_adam_ref.bars per element.
`defect=` plants one wrong reading (DEFECTS).  A tensor is a dict p, g (None: no gradient), m, v of equally long float32 arrays.
"""
import numpy as np

from tests import language_adam_ref as A

F32 = np.float32
CHUNK = 4096
DEFECTS = ('schedule_after_increment', 'bias_at_step', 'drop_at_after', 'div_first', 'tail_twice', 'empty_not_skipped', 'null_grad_zeros',
           'neighbour_first_chunk')


def warmup32(target, warm, after, step, defect=None):
    """csrc/mvnerf_adam.h::warmup_rate: float64 on the float32 target, one rounding to float32."""
    t, s, warm, after = np.float64(F32(target)), np.float64(int(step)), np.float64(warm), np.float64(after)
    if warm > 0 and s <= warm:
        return F32(t * (s / warm)) if defect == 'div_first' else F32(t * s / warm)
    keeps = s < after if defect == 'drop_at_after' else s <= after
    if after < 0 or keeps:
        return F32(target)
    return F32(t * np.float64(0.1))


def plan(lengths, chunk=CHUNK):
    """-> first_chunk (len + 1) int64: the prefix of ceil(n / chunk)."""
    n = np.asarray(lengths, np.int64)
    return np.concatenate([[0], np.cumsum(-(-n // chunk))]).astype(np.int64)


def find(first_chunk, chunk):
    """The last t < count with first_chunk[t] <= chunk."""
    return int(np.searchsorted(first_chunk[:-1], chunk, side='right')) - 1


def rates(hyper, warm, after, counter, defect=None):
    """(lr_s, lr_t) of the update that finds `counter` completed ones."""
    lr_s = warmup32(hyper['lr'], warm, after, counter + 1 if defect == 'schedule_after_increment' else counter, defect)
    with np.errstate(all='ignore'):
        lr_t = A.rate32(lr_s, hyper['beta1'], hyper['beta2'], counter if defect == 'bias_at_step' else counter + 1)
    return lr_s, lr_t


def step32(tensors, counter, hyper, warm, after, defect=None, chunk=CHUNK):
    """One multi-tensor step restated -> (tensors', counter + 1)."""
    assert defect is None or defect in DEFECTS, defect
    out = [dict(p=t['p'].copy(), g=t['g'], m=t['m'].copy(), v=t['v'].copy()) for t in tensors]
    first = plan([t['p'].size for t in tensors], chunk)
    _, lr_t = rates(hyper, warm, after, counter, defect)
    kw = dict(lr=hyper['lr'], beta1=hyper['beta1'], beta2=hyper['beta2'], eps=hyper['eps'], clip=hyper['clip'], lr_t=lr_t)

    def update(t, at, n):
        x = out[t]
        g = x['g']
        if g is None:
            if defect != 'null_grad_zeros':
                return
            g = np.zeros(x['p'].size, F32)
        sl = slice(at, at + n)
        if x['p'][sl].size:
            x['p'][sl], x['m'][sl], x['v'][sl], _ = A.update32(x['p'][sl], g[sl], x['m'][sl], x['v'][sl], counter + 1, **kw)

    for c in range(int(first[-1])):
        t = find(first, c)
        if defect == 'empty_not_skipped':
            t = int(np.searchsorted(first[:-1], first[t], side='left'))       # the first of a run of equal entries: an empty one
        base = first[max(t - 1, 0)] if defect == 'neighbour_first_chunk' else first[t]
        at = int(c - base) * chunk
        n = max(0, min(chunk, out[t]['p'].size - at))
        update(t, at, n)
        if defect == 'tail_twice' and 0 < n < chunk:
            update(t, at, n)
    return out, counter + 1


def step64(tensors, counter, hyper, warm, after):
    """The same step in float64 on the float32 constants and the float32 schedule rate -> per tensor None (no gradient) or
    dict p, m, v (float64) and bar (language_adam_ref.bars)."""
    lr_s, _ = rates(hyper, warm, after, counter)
    out = []
    for t in tensors:
        if t['g'] is None:
            out.append(None)
            continue
        with np.errstate(all='ignore'):
            ref = A.update64(t['p'], t['g'], t['m'], t['v'], counter + 1, lr_s, hyper['beta1'], hyper['beta2'], hyper['eps'], hyper['clip'])
        out.append(dict(p=ref['p'], m=ref['m'], v=ref['v'], bar=A.bars(ref)))
    return out


def outside(ref, got):
    """Elements of one tensor outside the bar, summed over p, m, v."""
    return sum(int((~(np.abs(np.asarray(got[k], np.float64) - ref[k]) <= ref['bar'][k])).sum()) for k in 'pmv')


def random_tensors(lengths, seed, no_grad=()):
    """p, g, m, v per length; g in thirds as tests/test_language_adam_cpu.py's inputs (above the clip, ordinary, where eps decides)."""
    rng = np.random.default_rng(seed)
    out = []
    for i, n in enumerate(lengths):
        kind = rng.integers(0, 3, n)
        sign = rng.choice([-1.0, 1.0], n)
        g = np.where(kind == 0, sign * rng.uniform(1.0, 50.0, n), np.where(kind == 1, 0.3 * rng.standard_normal(n), sign * rng.uniform(1e-9, 1e-7, n)))
        m = np.where(kind == 0, rng.standard_normal(n), np.where(kind == 1, 0.1 * rng.standard_normal(n), 1e-8 * rng.standard_normal(n)))
        v = np.where(kind == 0, rng.uniform(0.0, 2.0, n), np.where(kind == 1, rng.uniform(0.0, 0.1, n), rng.uniform(0.0, 1e-14, n)))
        p = 0.5 * rng.standard_normal(n)
        out.append(dict(p=p.astype(F32), g=None if i in no_grad else g.astype(F32), m=m.astype(F32), v=v.astype(F32)))
    return out
