"""The per-point part of GraspReadout (delta_ngf/layers.py:8-42: four Dense(128 -> 64) + elu, concatenation, Dense(256 -> 64) + elu) and the
closed forms of its first backward and of the derivative of that backward, as plain torch functions in the dtype of their arguments: what
csrc/grasp_head.hip is specified by (the formulas at the top of that file).  A helper for the tests, not a conftest.

  u_k = W_k a_k + b_k,  c = [elu(u_k)],  v = W_c c + b_c,  y = elu(v)
  first  : g_v = g_y . E'(v);  q_k = W_c[:,k]^T g_v;  g_u_k = q_k . E'(u_k);  g_a_k = W_k^T g_u_k
  second : s_k = W_k T_k;  r_k = s_k . E'(u_k);  z = sum_k W_c[:,k] r_k;  out_gy = z . E'(v);  m = z . g_y . E''(v);
           w_k = W_c[:,k]^T m;  p_k = s_k . q_k . E''(u_k) + w_k . E'(u_k)

E'(x) = 1 for x > 0 else e^x, E''(x) = 0 for x > 0 else e^x.  E'' jumps at 0, and the kernels decide from the sign of the stored output, so
the closed forms take the two decisions as boolean masks (`pos_c` = [c > 0] (N, 256), `pos_y` = [y > 0] (N, 64)): a reference run passes
its own (`own_masks`), a comparison with a kernel passes the masks of the kernel's c and y, and both then differentiate the same branch.
`mutant` names one deliberately wrong term (tests/test_grasp_head_ref.py shows that each of them moves a buffer past its bar)."""
import torch

FIRST = ('c', 'y', 'g_v', 'q', 'g_u', 'g_acts')
SECOND = ('out_gy', 'r', 'm', 'p')
MUTANTS = ('p_drop_first', 'p_drop_second', 'm_e1_for_e2', 'r_drop_e1', 'swap_wc_blocks', 'gv_drop_e1')
ACT_SCALE, W4_SCALE, SMALL_SCALE = 0.7, 0.12, 0.1          # the scales of tests/test_gpu_grasp_head.py
WEIGHT_SEED = 5
NEAR = 1e-5                                                   # two runs' decisions may differ only where |pre-activation| is below this


def seed_of(n):
    """The input seed of size n, shared by the CPU and the GPU tests.  With these seeds and WEIGHT_SEED no float64 pre-activation lies
    below NEAR in magnitude at N = 1, 33, 129, 160 or 136 (tests/test_grasp_head_ref.py asserts at most 0.1 %)."""
    return 1000 + n


def inputs(n, seed):
    """acts (4, n, 128), g_y (n, 64), t (4, n, 128) = dL/d(g_acts): float32 values on the CPU."""
    g = torch.Generator().manual_seed(seed)
    acts = torch.randn((4, n, 128), generator=g) * ACT_SCALE
    g_y = torch.randn((n, 64), generator=g)
    t = torch.randn((4, n, 128), generator=g)
    return acts, g_y, t


def weights(seed):
    """dict(w4 (4,64,128), b4 (4,64), wc (64,256), bc (64,)): float32 values on the CPU, torch [out, in] layout."""
    g = torch.Generator().manual_seed(seed)
    return dict(w4=torch.randn((4, 64, 128), generator=g) * W4_SCALE, b4=torch.randn((4, 64), generator=g) * SMALL_SCALE,
                wc=torch.randn((64, 256), generator=g) * SMALL_SCALE, bc=torch.randn((64,), generator=g) * SMALL_SCALE)


def to(w, dtype, device='cpu'):
    return {k: v.detach().to(device=device, dtype=dtype).contiguous() for k, v in w.items()}


def head(acts, w4, b4, wc, bc):
    elu = torch.nn.functional.elu
    return elu(torch.cat([elu(acts[k] @ w4[k].t() + b4[k]) for k in range(4)], -1) @ wc.t() + bc)


def pre_activations(acts, w):
    """u (N, 256) = [u_1 | .. | u_4] and v (N, 64) in the dtype of the arguments."""
    u = torch.cat([acts[k] @ w['w4'][k].t() + w['b4'][k] for k in range(4)], -1)
    v = torch.nn.functional.elu(u) @ w['wc'].t() + w['bc']
    return u, v


def own_masks(acts, w):
    u, v = pre_activations(acts, w)
    return u > 0, v > 0


def near_zero(acts, w, tol=1e-5):
    """(count, total) of the pre-activations u_k, v with magnitude below tol: the only places where two runs' masks may disagree."""
    u, v = pre_activations(acts, w)
    return int((u.abs() < tol).sum() + (v.abs() < tol).sum()), u.numel() + v.numel()


def _elu(x, pos):
    return torch.where(pos, x, torch.expm1(x))


def _d1(x, pos):
    return torch.where(pos, torch.ones_like(x), torch.exp(x))


def _d2(x, pos):
    return torch.where(pos, torch.zeros_like(x), torch.exp(x))


def _wc_of(w, mutant):
    wc = w['wc']
    if mutant == 'swap_wc_blocks':                            # the column block of k = 1 and of k + 1 change places (q and w read it)
        wc = torch.cat([wc[:, :64], wc[:, 128:192], wc[:, 64:128], wc[:, 192:]], 1)
    return wc


def first_buffers(acts, w, g_y, pos_c, pos_y, mutant=None):
    """-> dict(c (N,256), y (N,64), g_v (N,64), q (N,256), g_u (N,256), g_acts (4,N,128)) and the pre-activations u, v."""
    u = torch.cat([acts[k] @ w['w4'][k].t() + w['b4'][k] for k in range(4)], -1)
    c = _elu(u, pos_c)
    v = c @ w['wc'].t() + w['bc']
    y = _elu(v, pos_y)
    g_v = g_y if mutant == 'gv_drop_e1' else g_y * _d1(v, pos_y)
    q = g_v @ _wc_of(w, mutant)
    g_u = q * _d1(u, pos_c)
    g_acts = torch.stack([g_u[:, 64 * k:64 * k + 64] @ w['w4'][k] for k in range(4)])
    return dict(c=c, y=y, g_v=g_v, q=q, g_u=g_u, g_acts=g_acts, u=u, v=v)


def second_buffers(acts, w, g_y, t, pos_c, pos_y, mutant=None):
    """-> dict(s (N,256), r (N,256), z (N,64), out_gy (N,64), m (N,64), w (N,256), p (N,256))."""
    fb = first_buffers(acts, w, g_y, pos_c, pos_y, mutant=mutant)
    u, v, q = fb['u'], fb['v'], fb['q']
    s = torch.cat([t[k] @ w['w4'][k].t() for k in range(4)], -1)
    r = s if mutant == 'r_drop_e1' else s * _d1(u, pos_c)
    z = r @ w['wc'].t()
    out_gy = z * _d1(v, pos_y)
    m = z * g_y * (_d1(v, pos_y) if mutant == 'm_e1_for_e2' else _d2(v, pos_y))
    wk = m @ _wc_of(w, mutant)
    first, second = s * q * _d2(u, pos_c), wk * _d1(u, pos_c)
    p = second if mutant == 'p_drop_first' else first if mutant == 'p_drop_second' else first + second
    return dict(s=s, r=r, z=z, out_gy=out_gy, m=m, w=wk, p=p)


def first_grads(fb, acts):
    """The first gradients of <y, g_y> made of the first pass's buffers -> (d acts, d w4, d b4, d wc, d bc)."""
    g_u = fb['g_u']
    d_w4 = torch.stack([g_u[:, 64 * k:64 * k + 64].t() @ acts[k] for k in range(4)])
    return fb['g_acts'], d_w4, g_u.sum(0).reshape(4, 64), fb['g_v'].t() @ fb['c'], fb['g_v'].sum(0)


def second_grads(fb, sb, acts, t):
    """The gradients of <g_acts, T> made of both passes' buffers -> (dd w4, dd b4, dd wc, dd bc, dd g_y)."""
    g_u, p = fb['g_u'], sb['p']
    dd_w4 = torch.stack([g_u[:, 64 * k:64 * k + 64].t() @ t[k] + p[:, 64 * k:64 * k + 64].t() @ acts[k] for k in range(4)])
    return dd_w4, p.sum(0).reshape(4, 64), fb['g_v'].t() @ sb['r'] + sb['m'].t() @ fb['c'], sb['m'].sum(0), sb['out_gy']


def autograd_reference(acts, w, g_y, t, fn=head):
    """torch.autograd on `fn` in the dtype and on the device of the arguments -> (y, first, second): first = the gradients of <y, g_y>
    w.r.t. (acts, w4, b4, wc, bc) (create_graph=True), second = the gradients of <d/d acts, t> w.r.t. (w4, b4, wc, bc, g_y): the
    quantities tests/test_gpu_grasp_head.py forms."""
    a_, w4_, b4_, wc_, bc_, gy_ = (x.detach().clone().requires_grad_(True) for x in (acts, w['w4'], w['b4'], w['wc'], w['bc'], g_y))
    y = fn(a_, w4_, b4_, wc_, bc_)
    first = torch.autograd.grad((y * gy_).sum(), [a_, w4_, b4_, wc_, bc_], create_graph=True)
    second = torch.autograd.grad((first[0] * t).sum(), [w4_, b4_, wc_, bc_, gy_])
    return y.detach(), tuple(x.detach() for x in first), tuple(x.detach() for x in second)


def autograd_buffers(acts, w, g_y, t):
    """The ten per-point buffers from torch.autograd alone, the backward taken in stages so that q is a tensor of the second tape:
    g_v = d l1 / d v, q = d l1 / d c, g_u = d l1 / d u, g_acts = d l1 / d acts; with l2 = <g_acts, t>: out_gy = d l2 / d g_y,
    r = d l2 / d q, m = d l2 / d v, p = d l2 / d u."""
    elu, grad = torch.nn.functional.elu, torch.autograd.grad
    a_, gy_ = acts.detach().clone().requires_grad_(True), g_y.detach().clone().requires_grad_(True)
    u = torch.cat([a_[k] @ w['w4'][k].t() + w['b4'][k] for k in range(4)], -1)
    c = elu(u)
    v = c @ w['wc'].t() + w['bc']
    y = elu(v)
    g_v, = grad((y * gy_).sum(), v, create_graph=True)
    q, = grad(v, c, grad_outputs=g_v, create_graph=True)
    g_u, = grad(c, u, grad_outputs=q, create_graph=True)
    g_acts, = grad(u, a_, grad_outputs=g_u, create_graph=True)
    out_gy, r, m, p = grad((g_acts * t).sum(), [gy_, q, v, u])
    out = dict(c=c, y=y, g_v=g_v, q=q, g_u=g_u, g_acts=g_acts, out_gy=out_gy, r=r, m=m, p=p)
    return {k: x.detach() for k, x in out.items()}


def blocks_of(name, x):
    """The pieces of a buffer that are compared separately: the four 64-column blocks of the 256-wide buffers (one per Dense(128 -> 64)),
    the four (N, 128) planes of g_acts, the whole of the 64-wide ones -> [(label, (rows, cols) tensor)]."""
    if name == 'g_acts':
        return [(f'{name}[{k}]', x[k]) for k in range(4)]
    if x.shape[-1] == 256:
        return [(f'{name}[:, {64 * k}:{64 * k + 64}]', x[:, 64 * k:64 * k + 64]) for k in range(4)]
    return [(name, x)]


def rel(got, ref):
    """Relative L2 error."""
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    return float((got - ref).norm() / max(float(ref.norm()), 1e-300))


def worst_row(got, ref):
    """The largest row-wise L2 error over the largest row norm of the reference (2-D arguments)."""
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    return float((got - ref).norm(dim=-1).max() / max(float(ref.norm(dim=-1).max()), 1e-300))
