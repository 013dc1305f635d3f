"""float64 references for the bf16 trunk VJP (csrc/query_bf16.hip).  TEST INFRASTRUCTURE ONLY (NumPy, torch on the CPU).

The kernel walks the six ResNet blocks backwards.  Per block, with g = dL/d(block output), W1, W2 the bf16-rounded kernels and
bits(.) = [fp32 pre-activation > 0] as the forward wrote them:

    g_rh = bf16(g) W2^T ;  g_hid = g_rh o bits(h) ;  g_x = g + (bf16(g_hid) W1^T) o bits(x)          (fp32 accumulate, fp32 residual)

* `block_bwd_ref`  one block from the kernel's own fp32 cotangent, in the style of oracle/field_bf16_ref.block_ref: bf16(g) is decided
                   exactly, the one rounding in the middle, bf16(g_hid), gets the undecided window -> (ref, U, flip) for R.check;
* `chain(..., quantize=False)` = R    exact given the bits and the bf16 weights: no operand is rounded.  Equals float64 autograd of the
                   bf16-weight trunk when the bits come from that trunk's forward (`forward64`);
* `chain(..., quantize=True)`  = R_q  every B operand rounded to bf16, everything else float64: what the kernel computes up to fp32
                   accumulation and rare rounding flips.  `defect=` plants one of DEFECTS into it;
* `emulated_block`, `emulated_mv_embedding`   torch-CPU emulation of the whole bf16 path for end-to-end comparisons: hidden-layer
                   operands rounded to bf16 with straight-through Functions in the forward (value) and in the backward (cotangent),
                   layer 0 rounded in the forward only.

Bits are ordered as ops.unpack_relu_bits returns them: per view x0, h1, x1, h2, x2, h3, then mean, h4, x4, h5, x5, h6.
"""
from __future__ import annotations

import numpy as np
import torch

from oracle import field_bf16_ref as R

F64 = np.float64
DEFECTS = ('no_mask', 'swap_masks', 'no_residual', 'w_not_transposed', 'no_1_over_v', 'slot_late')


def rel_l2(a, b):
    a, b = np.asarray(a, F64), np.asarray(b, F64)
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


def _wq(blk):
    w1, _, w2, _ = blk
    return R.q(w1), R.q(w2)


# --------------------------------------------------------------------------------------------------------------------------
# one block from the kernel's own cotangent
# --------------------------------------------------------------------------------------------------------------------------
def block_bwd_ref(g, blk, bits_h, bits_x, c=R.C_WINDOW):
    """g (N,128) fp32: the cotangent the kernel was given (so bf16(g) is decided exactly); blk = (W1, b1, W2, b2); bits_h, bits_x
    (N,128) bool.  -> ref (N,128) float64, U (N,128) bool, flip (N,128): a kernel whose fp32 g_hid lies in the same bf16 rounding cell
    as the float64 one rounds it to the identical value; only elements within c * 2^-24 * mag of a rounding boundary may differ, by one
    bf16 step each, and `flip` is the most that can move an output."""
    w1q, w2q = _wq(blk)
    g = np.asarray(g, F64)
    a = R.q(g)
    g_hid = (a @ w2q.T) * bits_h
    mag = np.abs(a) @ np.abs(w2q.T)
    und = bits_h & (R.boundary_distance(g_hid) <= c * R.EPS * mag)
    flip = ((und * R.bf16_ulp(g_hid)) @ np.abs(w1q.T)) * bits_x
    ref = g + (R.q(g_hid) @ w1q.T) * bits_x
    return ref, und, flip


# --------------------------------------------------------------------------------------------------------------------------
# the chain
# --------------------------------------------------------------------------------------------------------------------------
def _block(g, blk, bits_h, bits_x, quantize, defect):
    w1q, w2q = _wq(blk)
    rnd = R.q if quantize else (lambda t: t)
    if defect == 'no_mask':
        bits_h = np.ones_like(bits_h)
    if defect == 'swap_masks':
        bits_h, bits_x = bits_x, bits_h
    t2, t1 = (w2q, w1q) if defect == 'w_not_transposed' else (w2q.T, w1q.T)
    g_hid = (rnd(g) @ t2) * bits_h
    d = (rnd(g_hid) @ t1) * bits_x
    return d if defect == 'no_residual' else g + d


def chain(net, g_acts, bits, views, quantize=False, defect=None):
    """g_acts (4,N,128): cotangents of the view mean, u1, u2, u3; bits (6 views + 6, N, 128) bool -> g0 (views, N, 128) float64 =
    dL/d(layer-0 output) of every view.  The cotangents of u3, u2, u1 and the mean enter where those tensors are produced; the mean's
    cotangent goes to each view as g / views."""
    assert defect is None or defect in DEFECTS
    g_acts, bits = np.asarray(g_acts, F64), np.asarray(bits, bool)
    fused = bits[6 * views:]
    g = g_acts[3]
    late = None
    for bi in (5, 4, 3):
        m = bi - 3
        g = _block(g, net['blocks'][bi], fused[2 * m + 1], fused[2 * m], quantize, defect)
        if late is not None:
            g, late = g + late, None
        if defect == 'slot_late':
            late = g_acts[m]
        else:
            g = g + g_acts[m]
    if defect != 'no_1_over_v':
        g = g / views
        late = None if late is None else late / views
    out = []
    for v in range(views):
        gv, pend = g, late
        for bi in (2, 1, 0):
            b = bits[6 * v:6 * v + 6]
            gv = _block(gv, net['blocks'][bi], b[2 * bi + 1], b[2 * bi], quantize, defect)
            if pend is not None:
                gv, pend = gv + pend, None
        out.append(gv)
    return np.stack(out)


def forward64(net, x0):
    """The bf16-weight trunk from x0 (views, N, 128) in float64, no activation rounding -> (acts (4,N,128), bits (6 views + 6, N, 128))."""
    x0 = np.asarray(x0, F64)
    bits, outs = [], []
    for x in x0:
        for bi in range(3):
            x, b = _fwd_block(x, net['blocks'][bi])
            bits += b
        outs.append(x)
    x = sum(outs) / len(outs)
    acts = [x]
    for bi in range(3, 6):
        x, b = _fwd_block(x, net['blocks'][bi])
        bits += b
        acts.append(x)
    return np.stack(acts), np.stack(bits)


def _fwd_block(x, blk):
    w1q, w2q = _wq(blk)
    hid = np.maximum(x, 0) @ w1q + np.asarray(blk[1], F64)
    return x + np.maximum(hid, 0) @ w2q + np.asarray(blk[3], F64), [x > 0, hid > 0]


def autograd64(net, x0, g_acts):
    """d(sum g_acts . acts)/d x0 of `forward64` by torch autograd in float64 -> (views, N, 128)."""
    t = lambda a: torch.from_numpy(np.asarray(a, F64))
    x0 = t(x0).requires_grad_(True)
    blocks = [(t(R.q(b[0])), t(b[1]), t(R.q(b[2])), t(b[3])) for b in net['blocks']]

    def block(x, blk):
        return x + torch.relu(torch.relu(x) @ blk[0] + blk[1]) @ blk[2] + blk[3]
    outs = []
    for x in x0:
        for bi in range(3):
            x = block(x, blocks[bi])
        outs.append(x)
    x = sum(outs) / len(outs)
    acts = [x]
    for bi in range(3, 6):
        x = block(x, blocks[bi])
        acts.append(x)
    (torch.stack(acts) * t(g_acts)).sum().backward()
    return x0.grad.numpy()


# --------------------------------------------------------------------------------------------------------------------------
# torch-CPU emulation of the bf16 path, for end-to-end comparisons against a float64 step
# --------------------------------------------------------------------------------------------------------------------------
def _q_torch(x):
    return x.to(torch.float32).to(torch.bfloat16).to(x.dtype)


class _RoundValue(torch.autograd.Function):
    """bf16(x) in the forward, identity in the backward (straight-through)."""

    @staticmethod
    def forward(ctx, x):
        return _q_torch(x)

    @staticmethod
    def backward(ctx, g):
        return g


class _RoundCotangent(torch.autograd.Function):
    """identity in the forward, bf16(g) in the backward: the B operand of the backward's products."""

    @staticmethod
    def forward(ctx, x):
        return x.clone()

    @staticmethod
    def backward(ctx, g):
        return _q_torch(g)


def emulated_block(x, w1, b1, w2, b2):
    """One ResNet block as the bf16 kernels compute it, float64 torch tensors: x + bf16(relu(hid)) bf16(W2) + b2 with
    hid = bf16(relu(x)) bf16(W1) + b1; in the backward the cotangent is rounded where the kernel rounds its B operands (in front of
    each transposed product), the masks are the forward's, the residual path is unrounded."""
    w1q, w2q = _q_torch(w1), _q_torch(w2)
    hid = _RoundCotangent.apply(_RoundValue.apply(torch.relu(x)) @ w1q) + b1
    return x + _RoundCotangent.apply(_RoundValue.apply(torch.relu(hid)) @ w2q) + b2


class _Layer0(torch.autograd.Function):
    """Layer 0 as the bf16 path runs it: the forward on the rounded operands (field_eval_bf16.hip), the backward through the unrounded
    fp32 weights (field_dz_kernel)."""

    @staticmethod
    def forward(ctx, x, w, xq, wq):
        ctx.save_for_backward(w)
        return xq @ wq

    @staticmethod
    def backward(ctx, g):
        (w,) = ctx.saved_tensors
        return g @ w.T, None, None, None


def emulated_mv_embedding(net, cam_xyz, cam_dir, feat, n_views, complete_output=False):
    """oracle/mvnerf_torch.mv_embedding with the bf16 path's roundings: layer 0 takes bf16 PE(xyz), image colours, features and weight
    rows (the PE(dir) seed stays fp32-grade) in the forward only; the six blocks are `emulated_block`."""
    from oracle import mvnerf_torch as T
    pe_xyz, pe_dir = T.position_encoding(cam_xyz), T.position_encoding(cam_dir)
    x = torch.cat([pe_xyz, pe_dir, feat], -1)
    n_pe = pe_xyz.shape[-1]
    keep = slice(n_pe, n_pe + pe_dir.shape[-1])
    xq, wq = _q_torch(x.detach()), _q_torch(net['W0'])
    xq[..., keep], wq[keep] = x.detach()[..., keep], net['W0'][keep]
    outs = [_Layer0.apply(x, net['W0'], xq, wq) + net['b0']]
    for blk in net['blocks'][:3]:
        outs.append(emulated_block(outs[-1], *blk))
    pre = outs[-1].reshape(outs[-1].shape[0] // n_views, n_views, *outs[-1].shape[1:])
    outs.append(pre.sum(1) / n_views)
    for blk in net['blocks'][3:]:
        outs.append(emulated_block(outs[-1], *blk))
    return outs if complete_output else outs[-1]
