"""The per-pose part of GraspReadout as HIP kernels (csrc/grasp_tail.hip) and the g_acts-only head VJP, on the GPU.

Value and VJP of the tail are held against a float64 restatement of delta_ngf/layers.py:24-28, 39-41.  The bar is not a chosen number: the
yardstick is the path the optimiser ran before these kernels - the same five lines as torch fp32 modules with torch.autograd.grad, on the
same device and inputs - measured here against the same float64 result; the kernels may have at most 4x its relative L2 error (2e-6 where
that is larger: the head's value bar, tests/test_gpu_grasp_head.py, a floor for M = 1 where the yardstick's error is one number), and in any
case stay below 1e-5, the head's first-derivative bar.  Each pair of figures is printed before it is asserted."""
import numpy as np
import pytest
import torch

from thesis_clip_nerf_amd import ops
from thesis_clip_nerf_amd.lmvnerf import GraspReadout

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
FACTOR, FLOOR, CAP = 4.0, 2e-6, 1e-5


def make_readout(n5, seed, use_bias=True):
    """GraspReadout's own initialisation (_he_normal_ weights) with N(0, 0.05^2) biases on the per-pose layers."""
    torch.manual_seed(seed)
    ro = GraspReadout(n5, use_bias=use_bias)
    with torch.no_grad():
        for lin in (ro.block_0.layer_0, ro.block_0.layer_1, ro.block_1.layer_0, ro.block_1.layer_1, ro.output_layer):
            if lin.bias is not None:
                lin.bias.normal_(0.0, 0.05)
    return ro


def weights(ro, dtype, device):
    f = lambda t: None if t is None else t.detach().to(device=device, dtype=dtype).contiguous()
    b0, b1, out = ro.block_0, ro.block_1, ro.output_layer
    return dict(w0=f(b0.layer_0.weight), b0=f(b0.layer_0.bias), w1=f(b0.layer_1.weight), b1=f(b0.layer_1.bias), ws=f(b0.shortcut.weight),
                w0b=f(b1.layer_0.weight), b0b=f(b1.layer_0.bias), w1b=f(b1.layer_1.weight), b1b=f(b1.layer_1.bias), w_out=f(out.weight),
                b_out=f(out.bias))


def tail(x, w):
    """delta_ngf/layers.py:24-28, 39-41 in the dtype of its arguments: x (M, K) -> success (M)."""
    elu = torch.nn.functional.elu
    h0 = elu(x) @ w['w0'].T + w['b0']
    x1 = x @ w['ws'].T + elu(h0) @ w['w1'].T + w['b1']
    h1 = elu(x1) @ w['w0b'].T + w['b0b']
    x2 = x1 + elu(h1) @ w['w1b'].T + w['b1b']
    s = torch.relu(x2) @ w['w_out'][0]
    return s if w['b_out'] is None else s + w['b_out'][0]


def value_and_vjp(x, w, g_s):
    x = x.detach().requires_grad_(True)
    s = tail(x, w)
    (g_x,) = torch.autograd.grad(s.sum() if g_s is None else (s * g_s).sum(), x)
    return s.detach(), g_x


def pack(ro):
    w = weights(ro, torch.float32, DEV)
    return ops.grasp_tail_pack((w['w0'], w['b0'], w['w1'], w['b1'], w['ws']), (w['w0b'], w['b0b'], w['w1b'], w['b1b']), (w['w_out'], w['b_out']))


def rel(got, ref):
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    return float((got - ref).norm() / max(float(ref.norm()), 1e-300))


def inputs(m, n5, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.nn.functional.elu(torch.randn((m, 64 * n5), generator=g, dtype=torch.float64)).float()
    g_s = torch.randn(m, generator=g, dtype=torch.float64).float()
    return x, g_s


def check(name, err_hip, err_torch):
    bar = min(max(FACTOR * err_torch, FLOOR), CAP)
    print(f'{name}: torch fp32 {err_torch:.3e}, hip {err_hip:.3e}, bar {bar:.3e}')
    assert err_hip <= bar, (name, err_hip, err_torch, bar)


@pytest.mark.parametrize('with_cotangent', [True, False])
@pytest.mark.parametrize('m,n5', [(1, 42), (37, 42), (256, 18), (12288, 42)])
def test_tail_value_and_vjp_match_float64_within_the_torch_paths_error(m, n5, with_cotangent):
    ro = make_readout(n5, 100 + n5)
    x, g_s = inputs(m, n5, 7 * m + n5)
    if not with_cotangent:
        g_s = None
    s64, g64 = value_and_vjp(x.double(), weights(ro, torch.float64, 'cpu'), None if g_s is None else g_s.double())
    assert float(g64.norm(dim=1).min()) > 0.0                                  # no row wholly behind the final relu
    xd, gd = x.to(DEV), None if g_s is None else g_s.to(DEV)
    s32, g32 = value_and_vjp(xd, weights(ro, torch.float32, DEV), gd)            # the yardstick: torch fp32 on the same device
    packed = pack(ro)
    success, stash = ops.grasp_tail_fwd(xd, packed)
    g_x = ops.grasp_tail_vjp(xd, stash, packed, g_s=gd)
    only = ops.grasp_tail_fwd(xd, packed, stash=False)
    torch.cuda.synchronize()
    assert success.shape == (m,) and stash.shape == (m, ops.TAIL_STASH) and g_x.shape == (m, 64 * n5)
    assert torch.isfinite(success).all() and torch.isfinite(g_x).all()
    assert torch.equal(only, success)                                            # value-only is the same forward
    tag = f'M={m} n5={n5} g_s={"random" if with_cotangent else "NULL"}'
    check(tag + ' value', rel(success, s64), rel(s32, s64))
    check(tag + ' vjp', rel(g_x, g64), rel(g32, g64))


def test_tail_without_output_bias_and_with_one_offset():
    ro = make_readout(1, 5, use_bias=False)
    x, g_s = inputs(70, 1, 3)
    s64, g64 = value_and_vjp(x.double(), weights(ro, torch.float64, 'cpu'), g_s.double())
    xd, gd = x.to(DEV), g_s.to(DEV)
    s32, g32 = value_and_vjp(xd, weights(ro, torch.float32, DEV), gd)
    packed = pack(ro)
    success, stash = ops.grasp_tail_fwd(xd, packed)
    g_x = ops.grasp_tail_vjp(xd, stash, packed, g_s=gd)
    torch.cuda.synchronize()
    check('M=70 n5=1 no bias value', rel(success, s64), rel(s32, s64))
    check('M=70 n5=1 no bias vjp', rel(g_x, g64), rel(g32, g64))


def test_tail_is_deterministic_and_rows_past_m_do_not_leak():
    n5, m, rows = 42, 37, 64
    ro = make_readout(n5, 9)
    packed = pack(ro)
    x, g_s = inputs(rows, n5, 11)
    x[m:] = float('nan')
    xd, gd = x.to(DEV), g_s.to(DEV)
    sentinel = -12345.0
    outs = []
    for _ in range(2):
        success = torch.full((rows,), sentinel, device=DEV)
        stash = torch.full((rows, ops.TAIL_STASH), sentinel, device=DEV)
        g_x = torch.full((rows, 64 * n5), sentinel, device=DEV)
        ops.grasp_tail_fwd(xd[:m], packed, stash=stash[:m], out=success[:m])
        ops.grasp_tail_vjp(xd[:m], stash[:m], packed, g_s=gd[:m], out=g_x[:m])
        outs.append((success, stash, g_x))
    torch.cuda.synchronize()
    for a, b in zip(*outs):
        assert torch.equal(a, b)                                                 # the same bits from run to run
    success, stash, g_x = outs[0]
    for t in (success, stash, g_x):
        assert torch.isfinite(t[:m]).all()
        assert (t[m:] == sentinel).all()                                         # untouched
    s64, g64 = value_and_vjp(x[:m].double(), weights(ro, torch.float64, 'cpu'), g_s[:m].double())
    s32, g32 = value_and_vjp(xd[:m], weights(ro, torch.float32, DEV), gd[:m])
    check('M=37 of 64 value', rel(success[:m], s64), rel(s32, s64))
    check('M=37 of 64 vjp', rel(g_x[:m], g64), rel(g32, g64))


def test_tail_wrappers_check_shapes():
    ro = make_readout(2, 1)
    packed = pack(ro)
    x = torch.zeros((5, 128), device=DEV)
    with pytest.raises(ValueError, match='x'):
        ops.grasp_tail_fwd(torch.zeros((5, 100), device=DEV), packed)
    with pytest.raises(ValueError, match='packed'):
        ops.grasp_tail_fwd(torch.zeros((5, 192), device=DEV), packed)
    with pytest.raises(ValueError, match='stash'):
        ops.grasp_tail_vjp(x, torch.zeros((4, ops.TAIL_STASH), device=DEV), packed)
    with pytest.raises(ValueError, match='g_s'):
        ops.grasp_tail_vjp(x, torch.zeros((5, ops.TAIL_STASH), device=DEV), packed, g_s=torch.zeros(4, device=DEV))


@pytest.mark.parametrize('n', [32, 1554, 64512])
def test_head_vjp_acts_is_bit_identical_to_the_full_head_vjp(n):
    g = torch.Generator().manual_seed(n)
    rnd = lambda *s, scale=1.0: (scale * torch.randn(s, generator=g)).to(DEV)
    w4, wc, b4, bc = rnd(4, 64, 128, scale=0.12), rnd(64, 256, scale=0.1), rnd(4, 64, scale=0.05), rnd(64, scale=0.05)
    packed = ops.grasp_head_pack(w4, wc)
    c, y = ops.grasp_head_fwd(rnd(4, n, 128), packed, b4, bc)
    g_y = rnd(n, 64)
    full = ops.grasp_head_vjp(g_y, c, y, packed)[3]
    acts_only = ops.grasp_head_vjp_acts(g_y, c, y, packed)
    torch.cuda.synchronize()
    assert acts_only.shape == (4, n, 128) and torch.isfinite(acts_only).all()
    assert torch.equal(acts_only, full)
