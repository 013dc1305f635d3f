"""The per-pose part of GraspReadout with trainable weights as HIP passes (csrc/grasp_tail_train.hip; lmvnerf._TailFn / _TailVJP), on the GPU.

The rule is that of tests/test_gpu_grasp_tail.py: the yardstick is the path training ran before these kernels - the same five lines as plain
torch fp32 tensors with torch.autograd.grad on the same device and inputs - measured here against the float64 result on the CPU; a kernel
quantity may have at most 4x the yardstick's relative L2 error (2e-6 where that is larger) and in any case stays below 1e-5 for the value,
g_x and the first-order weight gradients (that file's cap) and below 1e-4 for out_gs, out_x and the second-order weight gradients (the
head's second-derivative bar, tests/test_gpu_grasp_head.py).  Each pair of figures is printed before it is asserted."""
import functools

import pytest
import torch

from tests import grasp_tail_ref as R
from thesis_clip_nerf_amd import ops
from thesis_clip_nerf_amd.lmvnerf import _TailFn, _TailVJP

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
FACTOR, FLOOR, CAP1, CAP2 = 4.0, 2e-6, 1e-5, 1e-4
ZERO2 = ('b1b', 'b_out')                         # second-order gradients that are identically zero
# (M, n5, use_bias): one row; a ragged tile and the _gtn path; full tiles and the batched-GEMM path; one offset and no output bias; 257 row
# tiles x 6 offsets: gy = min(512 / 257, 2) = 1, so every wave of the wide kernels walks two offsets (0, 4 and 1, 5)
SHAPES = [(1, 42, True), (37, 42, True), (64, 18, True), (70, 1, False), (8224, 6, True)]


def check(name, err_hip, err_torch, cap):
    bar = min(max(FACTOR * err_torch, FLOOR), cap)
    print(f'{name}: torch fp32 {err_torch:.3e}, hip {err_hip:.3e}, bar {bar:.3e}')
    assert err_hip <= bar, (name, err_hip, err_torch, bar)


@functools.lru_cache(maxsize=None)
def case(m, n5, use_bias):
    """Inputs, float64 references (autograd and the closed forms' buffers) on the CPU and the fp32 yardsticks on the device: computed once
    per shape, shared by the tests, never modified."""
    ro = R.make_readout(n5, 100 + n5, use_bias=use_bias)
    x, g_s, t = R.inputs(m, n5, 7 * m + n5)
    w64 = R.weights(ro, torch.float64, 'cpu')
    ref = R.autograd_reference(x.double(), g_s.double(), t.double(), w64)
    assert float(ref[1]['x'].norm(dim=1).min()) > 0.0                          # no row wholly behind the final relu
    buf64 = (R.first_backward(x.double(), g_s.double(), w64), R.second_backward(x.double(), g_s.double(), t.double(), w64))
    w32 = R.weights(ro, torch.float32, DEV)
    xd, gd, td = x.to(DEV), g_s.to(DEV), t.to(DEV)
    yard = R.autograd_reference(xd, gd, td, w32)
    ybuf = (R.first_backward(xd, gd, w32), R.second_backward(xd, gd, td, w32))
    return dict(w32=w32, x=xd, g_s=gd, t=td, ref=ref, yard=yard, buf64=buf64, ybuf=ybuf)


def weight_list(w32, requires_grad):
    return [None if w32[n] is None else w32[n].detach().clone().requires_grad_(requires_grad) for n in R.WEIGHTS]


def pack(w):
    return ops.grasp_tail_pack((w['w0'], w['b0'], w['w1'], w['b1'], w['ws']), (w['w0b'], w['b0b'], w['w1b'], w['b1b']), (w['w_out'], w['b_out']))


@pytest.mark.parametrize('m,n5,use_bias', SHAPES)
def test_tail_fn_matches_float64_within_the_torch_paths_error(m, n5, use_bias):
    c = case(m, n5, use_bias)
    s64, first64, second64 = c['ref']
    s32, first32, second32 = c['yard']
    wl = weight_list(c['w32'], True)
    names = [n for n, w in zip(R.WEIGHTS, wl) if w is not None]
    live = [w for w in wl if w is not None]
    x = c['x'].clone().requires_grad_(True)
    g_s = c['g_s'].clone().requires_grad_(True)
    s = _TailFn.apply(x, *wl)
    first = torch.autograd.grad((s * g_s).sum(), [x] + live, create_graph=True)
    second = torch.autograd.grad((first[0] * c['t']).sum(), [g_s, x] + live, allow_unused=True)
    torch.cuda.synchronize()
    tag = f'M={m} n5={n5}'
    assert s.shape == (m,) and first[0].shape == (m, 64 * n5)
    check(tag + ' value', R.rel(s, s64), R.rel(s32, s64), CAP1)
    for n, g in zip(['x'] + names, first):
        assert g.shape == first64[n].shape and torch.isfinite(g).all(), n
        check(f'{tag} d_{n}', R.rel(g, first64[n]), R.rel(first32[n], first64[n]), CAP1)
    for n, g in zip(['g_s', 'x'] + names, second):
        if n in ZERO2:
            assert float(second64[n].abs().max()) == 0.0
            assert g is None or float(g.abs().max()) == 0.0, n                  # identically zero: exactly zero or None
            continue
        assert g is not None and g.shape == second64[n].shape and torch.isfinite(g).all(), n
        check(f'{tag} dd_{n}', R.rel(g, second64[n]), R.rel(second32[n], second64[n]), CAP2)


@pytest.mark.parametrize('m,n5,use_bias', SHAPES)
def test_kernel_buffers_match_the_closed_forms(m, n5, use_bias):
    c = case(m, n5, use_bias)
    fb64, sb64 = c['buf64']
    fb32, sb32 = c['ybuf']
    packed = pack(c['w32'])
    x, g_s, t = c['x'], c['g_s'], c['t']
    _, stash = ops.grasp_tail_fwd(x, packed)
    g_x, cot, act, ex = ops.grasp_tail_vjp_train(x, stash, packed, g_s=g_s)
    assert torch.equal(g_x, ops.grasp_tail_vjp(x, stash, packed, g_s=g_s))     # the frozen-weight VJP's bits
    ones = ops.grasp_tail_vjp_train(x, stash, packed)                          # g_s = NULL: ones
    assert torch.equal(ones[0], ops.grasp_tail_vjp(x, stash, packed))
    assert torch.equal(ones[1], ops.grasp_tail_vjp_train(x, stash, packed, g_s=torch.ones_like(g_s))[1])
    out_gs, out_x, cot2, tan, dex = ops.grasp_tail_vjp_bwd(x, t, stash, cot, packed, g_s=g_s)
    skipped = ops.grasp_tail_vjp_bwd(x, t, stash, cot, packed, g_s=g_s, want_x=False)
    torch.cuda.synchronize()
    assert skipped[1] is None and all(torch.equal(a, b) for a, b in zip(skipped[:1] + skipped[2:], (out_gs, cot2, tan, dex)))
    tag = f'M={m} n5={n5}'
    blocks320 = (('h0', 0, 128), ('x1', 128, 192), ('h1', 192, 256), ('x2', 256, 320))
    for name, got, cap, blocks in (('cot', cot, CAP1, blocks320), ('act', act, CAP1, blocks320), ('ex', ex, CAP1, None),
                                   ('cot2', cot2, CAP2, blocks320[:3]), ('tan', tan, CAP2, blocks320), ('dex', dex, CAP2, None),
                                   ('out_gs', out_gs, CAP2, None), ('out_x', out_x, CAP2, None)):
        r64, r32 = (fb64, fb32) if name in fb64 else (sb64, sb32)
        assert got.shape == r64[name].shape and torch.isfinite(got).all(), name
        for bname, lo, hi in blocks or (('', 0, None),):
            check(f'{tag} {name}{"." + bname if bname else ""}', R.rel(got[..., lo:hi], r64[name][..., lo:hi]),
                  R.rel(r32[name][..., lo:hi], r64[name][..., lo:hi]), cap)


def test_training_passes_are_deterministic_and_rows_past_m_do_not_leak():
    n5, m, rows = 42, 37, 64
    ro = R.make_readout(n5, 9)
    packed = pack(R.weights(ro, torch.float32, DEV))
    x, g_s, t = R.inputs(rows, n5, 11)
    xd, gd, td = x.to(DEV), g_s.to(DEV), t.to(DEV)
    _, good_stash = ops.grasp_tail_fwd(xd[:m].contiguous(), packed)
    stash = torch.full((rows, ops.TAIL_STASH), float('nan'), device=DEV)
    stash[:m] = good_stash
    _, good_cot, _, _ = ops.grasp_tail_vjp_train(xd[:m], stash[:m], packed, g_s=gd[:m])
    cot_in = torch.full((rows, ops.TAIL_COT), float('nan'), device=DEV)
    cot_in[:m] = good_cot
    for v in (xd, td, gd):
        v[m:] = float('nan')
    sentinel = -12345.0
    full = lambda *shape: torch.full(shape, sentinel, device=DEV)
    runs = []
    for _ in range(2):
        first = (full(rows, 64 * n5), full(rows, ops.TAIL_COT), full(rows, ops.TAIL_ACT), full(rows, 64 * n5))
        second = (full(rows), full(rows, 64 * n5), full(rows, ops.TAIL_COT2), full(rows, ops.TAIL_TAN), full(rows, 64 * n5))
        ops.grasp_tail_vjp_train(xd[:m], stash[:m], packed, g_s=gd[:m], out=tuple(v[:m] for v in first))
        ops.grasp_tail_vjp_bwd(xd[:m], td[:m], stash[:m], cot_in[:m], packed, g_s=gd[:m], out=tuple(v[:m] for v in second))
        runs.append(first + second)
    torch.cuda.synchronize()
    for a, b in zip(*runs):
        assert torch.equal(a, b)                                                 # the same bits from run to run
    for v in runs[0]:
        assert torch.isfinite(v[:m]).all()
        assert (v[m:] == sentinel).all()                                         # untouched
    assert torch.equal(runs[0][1][:m], good_cot)


def test_cotangent_on_a_weight_gradient_is_refused():
    c = case(64, 18, True)
    wl = weight_list(c['w32'], True)
    packed = pack(c['w32'])
    x = c['x'].clone().requires_grad_(True)
    _, stash = ops.grasp_tail_fwd(c['x'], packed)
    outs = _TailVJP.apply(c['g_s'].clone().requires_grad_(True), x, stash, packed, *wl)
    assert len(outs) == 12
    with pytest.raises(NotImplementedError, match='_TailVJP'):
        torch.autograd.grad(outs[1].sum(), wl[0])
    with pytest.raises(NotImplementedError, match='_TailVJP'):
        torch.autograd.grad((outs[0] * c['t']).sum() + outs[5].sum(), x)


def test_train_wrappers_check_shapes():
    ro = R.make_readout(2, 1)
    packed = pack(R.weights(ro, torch.float32, DEV))
    z = lambda *shape: torch.zeros(shape, device=DEV)
    x = z(5, 128)
    with pytest.raises(ValueError, match='stash'):
        ops.grasp_tail_vjp_train(x, z(4, ops.TAIL_STASH), packed)
    with pytest.raises(ValueError, match='g_s'):
        ops.grasp_tail_vjp_train(x, z(5, ops.TAIL_STASH), packed, g_s=z(4))
    with pytest.raises(ValueError, match='t_x'):
        ops.grasp_tail_vjp_bwd(x, z(5, 64), z(5, ops.TAIL_STASH), z(5, ops.TAIL_COT), packed)
    with pytest.raises(ValueError, match='cot'):
        ops.grasp_tail_vjp_bwd(x, z(5, 128), z(5, ops.TAIL_STASH), z(5, 256), packed)
    with pytest.raises(ValueError, match='packed'):
        ops.grasp_tail_vjp_bwd(z(5, 192), z(5, 192), z(5, ops.TAIL_STASH), z(5, ops.TAIL_COT), packed)
