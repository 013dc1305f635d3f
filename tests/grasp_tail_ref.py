"""The per-pose part of GraspReadout (delta_ngf/layers.py:24-28, 39-41) and the closed forms of its first backward and of the derivative of
that backward, as plain torch functions in the dtype of their arguments: what csrc/grasp_tail_train.hip is specified by
(include/mvnerf_hip.h).  A helper for the tests, not a conftest.

E = elu, E'(v) = 1 for v > 0 else e^v, E''(v) = 0 for v > 0 else e^v, H = [x2 > 0], K = 64 n5.  `mutate` names one deliberately wrong term
(tests/test_grasp_tail_train_ref.py shows that the comparison against autograd sees each of them)."""
import torch

WEIGHTS = ('w0', 'b0', 'w1', 'b1', 'ws', 'w0b', 'b0b', 'w1b', 'b1b', 'w_out', 'b_out')
MUTATIONS = ('drop_e2_h1', 'e1_for_e2_x1', 'drop_shortcut_out_x', 'swap_w0b_w1b', 'drop_gx2_from_gx1', 'forget_h', 'drop_e2_x')


def make_readout(n5, seed, use_bias=True):
    """GraspReadout's own initialisation (_he_normal_ weights) with N(0, 0.05^2) biases on the per-pose layers."""
    from thesis_clip_nerf_amd.lmvnerf import GraspReadout
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


def inputs(m, n5, seed):
    """x = elu(randn) (the head's output is an elu), g_s, t_x: float32 values on the CPU."""
    g = torch.Generator().manual_seed(seed)
    x = torch.nn.functional.elu(torch.randn((m, 64 * n5), generator=g, dtype=torch.float64)).float()
    g_s = torch.randn(m, generator=g, dtype=torch.float64).float()
    t_x = torch.randn((m, 64 * n5), generator=g, dtype=torch.float64).float()
    return x, g_s, t_x


def tail(x, w):
    """x (M, K) -> success (M)."""
    elu = torch.nn.functional.elu
    h0 = elu(x) @ w['w0'].T + w['b0']
    x1 = x @ w['ws'].T + elu(h0) @ w['w1'].T + w['b1']
    h1 = elu(x1) @ w['w0b'].T + w['b0b']
    x2 = x1 + elu(h1) @ w['w1b'].T + w['b1b']
    s = torch.relu(x2) @ w['w_out'][0]
    return s if w['b_out'] is None else s + w['b_out'][0]


def stash_of(x, w):
    """[h0 | x1 | h1 | x2] (M, 320), as mvnerf_grasp_tail_fwd writes it."""
    elu = torch.nn.functional.elu
    h0 = elu(x) @ w['w0'].T + w['b0']
    x1 = x @ w['ws'].T + elu(h0) @ w['w1'].T + w['b1']
    h1 = elu(x1) @ w['w0b'].T + w['b0b']
    x2 = x1 + elu(h1) @ w['w1b'].T + w['b1b']
    return torch.cat([h0, x1, h1, x2], 1)


def d1(v):
    return torch.where(v > 0, torch.ones_like(v), torch.exp(v))


def d2(v):
    return torch.where(v > 0, torch.zeros_like(v), torch.exp(v))


def first_backward(x, g_s, w, mutate=None):
    """mvnerf_grasp_tail_vjp_train and the weight gradients made of its buffers -> dict(g_x, cot, act, ex, grads={name: tensor})."""
    elu = torch.nn.functional.elu
    st = stash_of(x, w)
    h0, x1, h1, x2 = st[:, :128], st[:, 128:192], st[:, 192:256], st[:, 256:]
    wo = w['w_out'][0]
    hm = (x2 > 0).to(x.dtype)
    if mutate == 'forget_h':
        hm = torch.ones_like(hm)
    g_x2 = g_s[:, None] * wo * hm
    w0b, w1b = (w['w1b'], w['w0b']) if mutate == 'swap_w0b_w1b' else (w['w0b'], w['w1b'])
    g_h1 = (g_x2 @ w1b) * d1(h1)
    g_x1 = (g_h1 @ w0b) * d1(x1)
    if mutate != 'drop_gx2_from_gx1':
        g_x1 = g_x2 + g_x1
    g_h0 = (g_x1 @ w['w1']) * d1(h0)
    g_x = (g_h0 @ w['w0']) * d1(x) + g_x1 @ w['ws']
    ex, e0, e1, e2 = elu(x), elu(h0), elu(x1), elu(h1)
    r2 = g_s[:, None] * torch.relu(x2)
    cot = torch.cat([g_h0, g_x1, g_h1, g_x2], 1)
    act = torch.cat([e0, e1, e2, r2], 1)
    grads = dict(w0=g_h0.T @ ex, b0=g_h0.sum(0), w1=g_x1.T @ e0, b1=g_x1.sum(0), ws=g_x1.T @ x, w0b=g_h1.T @ e1, b0b=g_h1.sum(0),
                 w1b=g_x2.T @ e2, b1b=g_x2.sum(0), w_out=r2.sum(0)[None], b_out=g_s.sum()[None])
    return dict(g_x=g_x, cot=cot, act=act, ex=ex, grads=grads)


def second_backward(x, g_s, t, w, mutate=None):
    """mvnerf_grasp_tail_vjp_bwd and the weight gradients of phi = <t, g_x> made of its buffers ->
    dict(out_gs, out_x, cot2, tan, dex, grads={name: tensor})."""
    elu = torch.nn.functional.elu
    fb = first_backward(x, g_s, w)
    st = stash_of(x, w)
    h0, x1, h1, x2 = st[:, :128], st[:, 128:192], st[:, 192:256], st[:, 256:]
    g_h0, g_x1, g_h1, g_x2 = fb['cot'][:, :128], fb['cot'][:, 128:192], fb['cot'][:, 192:256], fb['cot'][:, 256:]
    wo = w['w_out'][0]
    hm = (x2 > 0).to(x.dtype)
    if mutate == 'forget_h':
        hm = torch.ones_like(hm)
    w0b, w1b = (w['w1b'], w['w0b']) if mutate == 'swap_w0b_w1b' else (w['w0b'], w['w1b'])
    # tangents forward
    da0 = d1(x) * t
    dh0 = da0 @ w['w0'].T
    de0 = d1(h0) * dh0
    dx1 = t @ w['ws'].T + de0 @ w['w1'].T
    da1 = d1(x1) * dx1
    dh1 = da1 @ w0b.T
    de1 = d1(h1) * dh1
    dx2 = dx1 + de1 @ w1b.T
    # second-order cotangents backward
    te1, ta1, te0, ta0 = g_x2 @ w1b, g_h1 @ w0b, g_x1 @ w['w1'], g_h0 @ w['w0']
    p_h1 = d2(h1) * dh1 * te1
    if mutate == 'drop_e2_h1':
        p_h1 = torch.zeros_like(p_h1)
    p_x1 = d1(x1) * (p_h1 @ w0b) + (d1(x1) if mutate == 'e1_for_e2_x1' else d2(x1)) * dx1 * ta1
    p_h0 = d1(h0) * (p_x1 @ w['w1']) + d2(h0) * dh0 * te0
    out_gs = (hm * dx2) @ wo
    out_x = d1(x) * (p_h0 @ w['w0'])
    if mutate != 'drop_e2_x':
        out_x = out_x + d2(x) * t * ta0
    if mutate != 'drop_shortcut_out_x':
        out_x = out_x + p_x1 @ w['ws']
    tg = g_s[:, None] * hm * dx2
    ex, e0, e1 = elu(x), elu(h0), elu(x1)
    cot2 = torch.cat([p_h0, p_x1, p_h1], 1)
    tan = torch.cat([de0, da1, de1, tg], 1)
    grads = dict(w0=g_h0.T @ da0 + p_h0.T @ ex, b0=p_h0.sum(0), w1=g_x1.T @ de0 + p_x1.T @ e0, b1=p_x1.sum(0), ws=g_x1.T @ t + p_x1.T @ x,
                 w0b=g_h1.T @ da1 + p_h1.T @ e1, b0b=p_h1.sum(0), w1b=g_x2.T @ de1, b1b=torch.zeros_like(w['b1b']), w_out=tg.sum(0)[None],
                 b_out=torch.zeros(1, dtype=x.dtype, device=x.device))
    return dict(out_gs=out_gs, out_x=out_x, cot2=cot2, tan=tan, dex=da0, grads=grads)


def autograd_reference(x, g_s, t, w):
    """The same quantities from torch.autograd on `tail` (create_graph=True for the second tape) -> (s, first, second): first = dict(x=g_x,
    **weight gradients) of (s . g_s).sum(), second = dict(g_s, x, **weights) of phi = (g_x . t).sum(); identically-zero entries are zeros."""
    names = [n for n in WEIGHTS if w[n] is not None]
    wl = {n: (None if w[n] is None else w[n].detach().clone().requires_grad_(True)) for n in WEIGHTS}
    xr, gr = x.detach().clone().requires_grad_(True), g_s.detach().clone().requires_grad_(True)
    s = tail(xr, wl)
    got = torch.autograd.grad((s * gr).sum(), [xr] + [wl[n] for n in names], create_graph=True)
    first = dict(zip(['x'] + names, got))
    phi = (first['x'] * t).sum()
    got2 = torch.autograd.grad(phi, [gr, xr] + [wl[n] for n in names], allow_unused=True)
    second = {}
    for n, ref, g in zip(['g_s', 'x'] + names, [gr, xr] + [wl[n] for n in names], got2):
        second[n] = torch.zeros_like(ref) if g is None else g
    return s.detach(), {k: v.detach() for k, v in first.items()}, {k: v.detach() for k, v in second.items()}


def rel(got, ref):
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    return float((got - ref).norm() / max(float(ref.norm()), 1e-300))
