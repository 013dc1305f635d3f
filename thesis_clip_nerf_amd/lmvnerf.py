"""`LanguageNeRF` on the HIP trunk (reference: src/lib/lmvnerf/model_v4.py).

The reference's language/grasp model re-uses the NeRF trunk (`fine_embedding`, frozen) as a feature field on points
derived from grasp poses, puts a small `GraspReadout` MLP on its four fused activations and trains ONLY that read-out
with a loss on the prediction and a loss on d prediction / d pose (nested GradientTape, model_v4.py:277-322).  Here:

* the trunk is `TrunkField`: forward = `mvnerf_field_eval_stash` on the query points (activations read back from the
  stash), backward = `mvnerf_query_vjp`, and the backward of THAT backward w.r.t. its cotangent = `mvnerf_query_jvp`
  (the trunk is linear in nothing but the cotangent, so the double-backward the second tape needs is a JVP);
* `GraspReadout`'s per-point layers are fused HIP passes (`_HeadFn`, csrc/grasp_head.hip) and so, with `fused_tail`, are its
  per-pose blocks (`_TailFn`, csrc/grasp_tail.hip + grasp_tail_train.hip; off by default: torch + gemm_ops); the pose algebra
  and the losses are ordinary torch (small, and torch's autograd supplies their double-backward); the CLIP / ViT / conv
  encoders are outside the hot path: `combined_features` is an input.

Names and argument meaning follow the reference (`_call`, `compute_matrices`, `set_pose`, `train_step`, `infer`).
"""
from __future__ import annotations

import math
import os
import warnings

import numpy as np
import torch
from torch import nn

from . import ops, range_policy

N_FUSED = 4
COMPUTE_DTYPES = ('f32', 'bf16')


# ---- the trunk as an autograd function ----------------------------------------------------------------------
class TrunkState:
    """Everything the trunk needs besides the query points: source views, cameras, packed weights."""

    def __init__(self, images, features, intrinsics, extrinsics_inv, net_keras, compute_dtype='f32', weight_images=None):
        """weight_images: (packed, packed_split, bwd_streams) of `net_keras` kept by the caller (LanguageNeRF's trunk cache); None packs
        them here."""
        if compute_dtype not in COMPUTE_DTYPES:
            raise ValueError(f"compute_dtype must be 'f32' or 'bf16', got {compute_dtype!r}")
        self.compute_dtype = compute_dtype
        self.geo = (images.contiguous(), features.contiguous(), intrinsics.contiguous(), extrinsics_inv.contiguous())
        if weight_images is not None:
            self.packed, self.packed_split, self.bwd_streams = weight_images
        else:
            self.packed = ops.pack_net(net_keras)
            self.packed_split = ops.pack_net_split(net_keras)      # value pass on the split-bf16 kernel (fp32-grade)
            self.bwd_streams = ops.pack_bwd_streams(net_keras)
        self.n_views = images.shape[1]
        if compute_dtype == 'bf16':                                # the hidden layers on the bf16 MFMA, forward and VJP
            self.packed16 = ops.pack_net_bf16(net_keras)
            self.bwd16 = ops.pack_bwd_streams_bf16(net_keras)


def _pad32(t, n_pad):
    return t if n_pad == 0 else torch.cat([t, t[:, -1:].expand(-1, n_pad, -1)], 1).contiguous()


class _TrunkVJP(torch.autograd.Function):
    """(g_acts) -> (d_points, d_dirs) = J^T g_acts; differentiable w.r.t. g_acts: its backward is J c."""

    @staticmethod
    def forward(ctx, g_acts, points, dirs, state, stash):
        ctx.state, ctx.points, ctx.dirs = state, points, dirs
        if state.compute_dtype == 'bf16':               # stash: the relu bits of query_stash_bf16
            return ops.query_vjp_bf16(points, dirs, *state.geo, state.bwd_streams, state.bwd16, stash, g_acts.contiguous())
        return ops.query_vjp(points, dirs, *state.geo, state.bwd_streams, stash, g_acts.contiguous())

    @staticmethod
    def backward(ctx, c_points, c_dirs):
        st = ctx.state
        if st.compute_dtype == 'bf16':
            raise RuntimeError("the trunk's second derivative (the JVP behind the gradient of a gradient) has no bf16 form: "
                               "build the TrunkState with compute_dtype='f32' for losses on d prediction / d pose")
        zero = torch.zeros_like(ctx.points)
        c_points = zero if c_points is None else c_points.contiguous()
        c_dirs = zero if c_dirs is None else c_dirs.contiguous()
        t_acts = ops.query_jvp(ctx.points, ctx.dirs, c_points, c_dirs, *st.geo, st.packed)
        return t_acts, None, None, None, None          # second derivatives w.r.t. the poses are not propagated


class TrunkField(torch.autograd.Function):
    """points, dirs (B,N,3) -> acts (4,B,N,128) = (view mean, u1, u2, u3) of the frozen trunk (layers.py:364-377)."""

    @staticmethod
    def forward(ctx, points, dirs, state):
        b, n, _ = points.shape
        pad = (-n) % 32 if state.n_views > 1 else 0     # the multi-view training kernels want whole 32-point tiles per scene
        p, d = _pad32(points.detach().contiguous(), pad), _pad32(dirs.detach().contiguous(), pad)
        if state.compute_dtype == 'bf16':
            acts, stash = ops.query_stash_bf16(p, d, *state.geo, state.packed, state.packed16)          # rows, and relu bits for the VJP
        else:
            stash = ops.query_stash(p, d, *state.geo, state.packed, packed_split=state.packed_split)
            acts = ops.stash_fused_acts(stash, b, state.n_views, n + pad)   # tile layout -> (4, b, n + pad, 128) rows
        ctx.state, ctx.stash, ctx.pad, ctx.n = state, stash, pad, n
        ctx.save_for_backward(p, d)
        return acts[:, :, :n].contiguous() if pad else acts

    @staticmethod
    def backward(ctx, g_acts):
        p, d = ctx.saved_tensors
        if ctx.pad:
            g_acts = torch.cat([g_acts, g_acts.new_zeros(4, g_acts.shape[1], ctx.pad, 128)], 2)
        d_points, d_dirs = _TrunkVJP.apply(g_acts, p, d, ctx.state, ctx.stash)
        return d_points[:, :ctx.n], d_dirs[:, :ctx.n], None


# ---- GraspReadout (delta_ngf/layers.py:8-42) ----------------------------------------------------------------
def _skinny(m, n, k):
    """Products mvnerf_gemm_nt takes over from the library GEMM: every shape it accepts.  On the GraspReadout's shapes the library picks
    poor kernels - 4 to 36 workgroups for the weight gradients (64 x 128 outputs over K = 64 512 rows: 245 us) and for the 2688-input block
    (1536 x 128 over K = 2688), 16 x 16 tiles for 64 512 x 128 x 64 (590 us) - see profiles/r02_language_step_trace.md."""
    return ops.gemm_nt_ok(m, n, k) and k >= 64


def _mm_nt_raw(a, bt):
    if a.is_cuda and a.dtype == torch.float32 and bt.dtype == torch.float32 and _skinny(a.shape[0], bt.shape[0], a.shape[1]):
        return ops.gemm_nt(a.contiguous(), bt.contiguous())
    return a @ bt.t()


def _tn_skinny(m, n, k):
    return ops.gemm_tn_ok(m, n, k) and m >= 64


class _MatmulNT(torch.autograd.Function):
    """a (M,K) @ bt (N,K)^T with the skinny products on mvnerf_gemm_nt.  The backward is built from this function and _MatmulTN again, so
    the second derivatives LanguageNeRF.train_step takes (model_v4.py:290-322) choose their kernels the same way (a large forward
    product has a skinny weight gradient)."""

    @staticmethod
    def forward(ctx, a, bt):
        ctx.save_for_backward(a, bt)
        return _mm_nt_raw(a, bt)

    @staticmethod
    def backward(ctx, g):
        a, bt = ctx.saved_tensors
        ga = _MatmulNT.apply(g, bt.t()) if ctx.needs_input_grad[0] else None               # g (M,N) @ bt (N,K): bt^T is a small copy
        gbt = _MatmulTN.apply(g, a) if ctx.needs_input_grad[1] else None                   # g^T (N,M) @ a (M,K), operands as they lie
        return ga, gbt


class _MatmulTN(torch.autograd.Function):
    """g (M,N)^T @ a (M,K) -> (N,K): a weight gradient, without transposed copies of the M-row operands (mvnerf_gemm_tn)."""

    @staticmethod
    def forward(ctx, g, a):
        ctx.save_for_backward(g, a)
        if g.is_cuda and g.dtype == torch.float32 and a.dtype == torch.float32 and _tn_skinny(g.shape[0], g.shape[1], a.shape[1]):
            return ops.gemm_tn(g.contiguous(), a.contiguous())
        return g.t() @ a

    @staticmethod
    def backward(ctx, c):
        g, a = ctx.saved_tensors
        gg = _MatmulNT.apply(a, c) if ctx.needs_input_grad[0] else None                    # a (M,K) @ c (N,K)^T -> (M,N)
        ga = _MatmulNT.apply(g, c.t()) if ctx.needs_input_grad[1] else None                # g (M,N) @ c (N,K) -> (M,K): c^T is a small copy
        return gg, ga


class _LinearNT(torch.autograd.Function):
    """x (M,K) @ w (N,K)^T + b with the bias added in the GEMM's epilogue (mvnerf_gemm_nt_bias: one launch instead of two).  The backward is
    _MatmulNT / _MatmulTN and a column sum, so it can be differentiated again like the unfused form."""

    @staticmethod
    def forward(ctx, a, w, b):
        ctx.save_for_backward(a, w)
        return ops.gemm_nt(a.contiguous(), w.contiguous(), bias=b.contiguous())

    @staticmethod
    def backward(ctx, g):
        a, w = ctx.saved_tensors
        ga = _MatmulNT.apply(g, w.t()) if ctx.needs_input_grad[0] else None
        if (ctx.needs_input_grad[1] and ctx.needs_input_grad[2] and not torch.is_grad_enabled() and g.is_cuda and g.dtype == torch.float32
                and _tn_skinny(g.shape[0], g.shape[1], a.shape[1])):
            # the last backward of a step (nothing differentiates it again): weight and bias gradient from one pass over g
            gw, gb = (t[0] for t in ops.gemm_tn_batched(g.contiguous()[None], a.contiguous()[None], colsum_of=1))
            return ga, gw, gb
        gw = _MatmulTN.apply(g, a) if ctx.needs_input_grad[1] else None
        gb = g.sum(0) if ctx.needs_input_grad[2] else None
        return ga, gw, gb


def _mm_nt(a, bt):
    """a @ bt^T through _MatmulNT on the GPU (fp32), plain torch otherwise."""
    if a.is_cuda and a.dtype == torch.float32 and bt.dtype == torch.float32:
        return _MatmulNT.apply(a, bt)
    return a @ bt.t()


def _wide_linear(lin, x):
    """nn.Linear through _mm_nt (value, input / weight gradients and their derivatives)."""
    if not x.is_cuda:
        return lin(x)
    x2 = x.reshape(-1, lin.in_features)
    if lin.bias is not None and x2.dtype == torch.float32 and _skinny(x2.shape[0], lin.out_features, lin.in_features):
        y = _LinearNT.apply(x2, lin.weight, lin.bias)
    else:
        y = _mm_nt(x2, lin.weight)
        if lin.bias is not None:
            y = y + lin.bias
    return y.reshape(*x.shape[:-1], lin.out_features)


# ---- the per-point part of the read-out as fused HIP passes (csrc/grasp_head.hip) ----------------------------------------------------
def _gtn(g, a):
    """g (M,N)^T @ a (M,K) -> (N,K) on mvnerf_gemm_tn where it takes the shape (M = the number of query points)."""
    if _tn_skinny(g.shape[0], g.shape[1], a.shape[1]):
        return ops.gemm_tn(g.contiguous(), a.contiguous())
    return g.t() @ a


def _batched_ok(g_u):
    return g_u.is_cuda and g_u.dtype == torch.float32 and g_u.shape[0] % 8 == 0 and g_u.is_contiguous()


def _col_blocks(x):
    """(M, 4 * 64) -> the four (M, 64) column blocks as a (4, M, 64) view (strides 64, 256, 1): what mvnerf_gemm_tn_batched reads in place."""
    return x.view(x.shape[0], 4, 64).permute(1, 0, 2)


class _HeadVJP(torch.autograd.Function):
    """The vector-Jacobian product of the fused head as a differentiable function of its cotangent and of the weights: forward =
    mvnerf_grasp_head_vjp (+ the weight gradients as skinny GEMMs), backward = mvnerf_grasp_head_vjp_bwd - what the nested tape of
    LanguageNeRF.train_step needs (model_v4.py:290-322).  The activations' own second derivative is not formed (they depend on the pose
    only, which is not trained); cotangents on the weight-gradient outputs are refused."""

    @staticmethod
    def forward(ctx, g_y, acts, c, y, w4, b4, wc, bc, packed):
        g_y = g_y.contiguous()
        g_v, q, g_u, g_acts = ops.grasp_head_vjp(g_y, c, y, packed)
        if _batched_ok(g_u):
            # the five weight gradients and their bias gradients: two launches (+ fixed-order reduces), the column blocks of g_u read where they lie
            d_w4, d_b4 = ops.gemm_tn_batched(_col_blocks(g_u), acts, colsum_of=1)
            d_wc, d_bc = (t[0] for t in ops.gemm_tn_batched(g_v[None], c[None], colsum_of=1))
        else:
            d_wc, d_bc = _gtn(g_v, c), g_v.sum(0)
            d_w4 = torch.stack([_gtn(g_u[:, 64 * k:64 * k + 64], acts[k]) for k in range(4)])
            d_b4 = g_u.sum(0).reshape(4, 64)
        ctx.save_for_backward(g_y, acts, c, y, q, g_v, g_u, packed)
        ctx.set_materialize_grads(False)
        return g_acts, d_w4, d_b4, d_wc, d_bc

    @staticmethod
    def backward(ctx, t_acts, *weight_cotangents):
        if any(t is not None for t in weight_cotangents):
            raise NotImplementedError('_HeadVJP: derivatives of the weight gradients are not built (LanguageNeRF.train_step does not take them)')
        if t_acts is None:
            return (None,) * 9
        g_y, acts, c, y, q, g_v, g_u, packed = ctx.saved_tensors
        out_gy, r, m, p_ = ops.grasp_head_vjp_bwd(t_acts.contiguous(), g_y, c, y, q, packed)
        if _batched_ok(g_u):
            d_w4, d_b4 = ops.gemm_tn_batched(_col_blocks(g_u), t_acts.contiguous(), g2=_col_blocks(p_), a2=acts, colsum_of=2)
            d_wc, d_bc = (t[0] for t in ops.gemm_tn_batched(g_v[None], r[None], g2=m[None], a2=c[None], colsum_of=2))
        else:
            d_w4 = torch.stack([_gtn(g_u[:, 64 * k:64 * k + 64], t_acts[k]) + _gtn(p_[:, 64 * k:64 * k + 64], acts[k]) for k in range(4)])
            d_b4 = p_.sum(0).reshape(4, 64)
            d_wc = _gtn(g_v, r) + _gtn(m, c)
            d_bc = m.sum(0)
        return out_gy, None, None, None, d_w4, d_b4, d_wc, d_bc, None


class _HeadFn(torch.autograd.Function):
    """acts (4,N,128) -> (N,64): four Dense(128 -> 64) + elu, concatenation, Dense(256 -> 64) + elu in ONE launch (mvnerf_grasp_head_fwd);
    its backward is _HeadVJP, itself differentiable."""

    @staticmethod
    def forward(ctx, acts, w4, b4, wc, bc):
        acts, w4, b4, wc, bc = (t.contiguous() for t in (acts, w4, b4, wc, bc))
        packed = ops.grasp_head_pack(w4, wc)
        c, y = ops.grasp_head_fwd(acts, packed, b4, bc)
        ctx.save_for_backward(acts, c, y, w4, b4, wc, bc, packed)
        return y

    @staticmethod
    def backward(ctx, g_y):
        acts, c, y, w4, b4, wc, bc, packed = ctx.saved_tensors
        return _HeadVJP.apply(g_y, acts, c, y, w4, b4, wc, bc, packed)


# ---- the per-pose part of the read-out as fused HIP passes (csrc/grasp_tail.hip, csrc/grasp_tail_train.hip) ---------------------------
def _tn1(g, a, g2=None, a2=None, colsum_of=0):
    """One weight gradient g^T a (+ g2^T a2) [and the column sums of g / g2] on mvnerf_gemm_tn_batched: the operands may be column blocks
    of the kernels' (M, 320) / (M, 256) buffers, read where they lie."""
    r = ops.gemm_tn_batched(g[None], a[None], g2=None if g2 is None else g2[None], a2=None if a2 is None else a2[None], colsum_of=colsum_of)
    return (r[0][0], r[1][0]) if colsum_of else r[0]


def _pair(x, lo):
    """Columns lo .. lo + 128 of x (M, F) as a (2, M, 64) view: the two 64 x 64 layers of block_1 as one batch of two."""
    return x[:, lo:lo + 128].unflatten(1, (2, 64)).permute(1, 0, 2)


class _TailVJP(torch.autograd.Function):
    """The vector-Jacobian product of the fused tail as a differentiable function of its cotangent, of x and of the weights: forward =
    mvnerf_grasp_tail_vjp_train (+ the weight gradients as skinny TN products of its buffers), backward = mvnerf_grasp_tail_vjp_bwd - what
    the nested tape of LanguageNeRF.train_step needs (model_v4.py:290-322).  Unlike the head's, the input's cotangent is returned: x is
    the head's output and the head is trained.  Cotangents on the weight-gradient outputs are refused."""

    @staticmethod
    def forward(ctx, g_s, x, stash, packed, w0, b0, w1, b1, ws, w0b, b0b, w1b, b1b, w_out, b_out):
        g_s = g_s.contiguous()
        g_x, cot, act, ex = ops.grasp_tail_vjp_train(x, stash, packed, g_s=g_s)
        if _batched_ok(cot):
            d_w0, d_b0 = _tn1(cot[:, :128], ex, colsum_of=1)
            d_ws, d_b1 = _tn1(cot[:, 128:192], x, colsum_of=1)
            d_w1 = _tn1(cot[:, 128:192], act[:, :128])
            (d_w0b, d_w1b), (d_b0b, d_b1b) = ops.gemm_tn_batched(_pair(cot, 192), _pair(act, 128), colsum_of=1)
        else:
            g_h0, g_x1, g_h1, g_x2 = cot[:, :128], cot[:, 128:192], cot[:, 192:256], cot[:, 256:]
            d_w0, d_ws, d_w1 = _gtn(g_h0, ex), _gtn(g_x1, x), _gtn(g_x1, act[:, :128])
            d_w0b, d_w1b = _gtn(g_h1, act[:, 128:192]), _gtn(g_x2, act[:, 192:256])
            d_b0, d_b1, d_b0b, d_b1b = cot.sum(0).split([128, 64, 64, 64])
        d_wout = act[:, 256:].sum(0).reshape(w_out.shape)
        d_bout = g_s.sum().reshape(1) if b_out is not None else None
        ctx.save_for_backward(g_s, x, stash, packed, cot, act, ex)
        ctx.wout_shape = w_out.shape
        ctx.set_materialize_grads(False)
        return g_x, d_w0, d_b0, d_w1, d_b1, d_ws, d_w0b, d_b0b, d_w1b, d_b1b, d_wout, d_bout

    @staticmethod
    def backward(ctx, t_x, *weight_cotangents):
        if any(t is not None for t in weight_cotangents):
            raise NotImplementedError('_TailVJP: derivatives of the weight gradients are not built (LanguageNeRF.train_step does not take them)')
        if t_x is None:
            return (None,) * 15
        g_s, x, stash, packed, cot, act, ex = ctx.saved_tensors
        t_x = t_x.contiguous()
        out_gs, out_x, cot2, tan, dex = ops.grasp_tail_vjp_bwd(x, t_x, stash, cot, packed, g_s=g_s, want_x=ctx.needs_input_grad[1])
        g_h0, g_x1, g_h1, g_x2 = cot[:, :128], cot[:, 128:192], cot[:, 192:256], cot[:, 256:]
        p_h0, p_x1, p_h1 = cot2[:, :128], cot2[:, 128:192], cot2[:, 192:]
        if _batched_ok(cot):
            d_w0, d_b0 = _tn1(g_h0, dex, p_h0, ex, colsum_of=2)
            d_ws, d_b1 = _tn1(g_x1, t_x, p_x1, x, colsum_of=2)
            d_w1 = _tn1(g_x1, tan[:, :128], p_x1, act[:, :128])
            d_w0b, d_b0b = _tn1(g_h1, tan[:, 128:192], p_h1, act[:, 128:192], colsum_of=2)
            d_w1b = _tn1(g_x2, tan[:, 192:256])
        else:
            d_w0 = _gtn(g_h0, dex) + _gtn(p_h0, ex)
            d_ws = _gtn(g_x1, t_x) + _gtn(p_x1, x)
            d_w1 = _gtn(g_x1, tan[:, :128]) + _gtn(p_x1, act[:, :128])
            d_w0b = _gtn(g_h1, tan[:, 128:192]) + _gtn(p_h1, act[:, 128:192])
            d_w1b = _gtn(g_x2, tan[:, 192:256])
            d_b0, d_b1, d_b0b = cot2.sum(0).split([128, 64, 64])
        d_wout = tan[:, 256:].sum(0).reshape(ctx.wout_shape)
        # b1' and b_out enter the first backward through the relu's mask only: their second-order gradients are identically zero (None)
        return out_gs, out_x, None, None, d_w0, d_b0, d_w1, d_b1, d_ws, d_w0b, d_b0b, d_w1b, None, d_wout, None


class _TailFn(torch.autograd.Function):
    """x (M, 64 n5) -> success (M,): Dense(64 n5 -> 128) + elu, the two elu ResNet blocks and relu-Dense(64 -> 1) in ONE launch
    (mvnerf_grasp_tail_fwd on the weights packed by mvnerf_grasp_tail_pack); its backward is _TailVJP, itself differentiable."""

    @staticmethod
    def forward(ctx, x2d, w0, b0, w1, b1, ws, w0b, b0b, w1b, b1b, w_out, b_out):
        x2d, w0, b0, w1, b1, ws, w0b, b0b, w1b, b1b, w_out = (t.contiguous() for t in (x2d, w0, b0, w1, b1, ws, w0b, b0b, w1b, b1b, w_out))
        packed = ops.grasp_tail_pack((w0, b0, w1, b1, ws), (w0b, b0b, w1b, b1b), (w_out, b_out))
        if not any(ctx.needs_input_grad):                  # no gradient can be asked for: the value only, no stash
            return ops.grasp_tail_fwd(x2d, packed, stash=False)
        s, stash = ops.grasp_tail_fwd(x2d, packed)
        ctx.save_for_backward(x2d, stash, packed, w0, b0, w1, b1, ws, w0b, b0b, w1b, b1b, w_out, b_out)
        return s

    @staticmethod
    def backward(ctx, g_s):
        return _TailVJP.apply(g_s, *ctx.saved_tensors)


def _he_normal_(w):
    fan_in = w.shape[1]
    nn.init.trunc_normal_(w, std=math.sqrt(2.0 / fan_in) / 0.87962566103423978, a=-2 * math.sqrt(2.0 / fan_in) / 0.87962566103423978,
                          b=2 * math.sqrt(2.0 / fan_in) / 0.87962566103423978)


class ResNetMLPBlock(nn.Module):
    """layers.py:262-298 with activation='elu' (the pre-activation form: act -> Dense -> act -> Dense, + shortcut)."""

    def __init__(self, in_size, hidden_size, output_size, transform_shortcut=False):
        super().__init__()
        self.layer_0 = nn.Linear(in_size, hidden_size)
        self.layer_1 = nn.Linear(hidden_size, output_size)
        self.shortcut = nn.Linear(in_size, output_size, bias=False) if transform_shortcut else None
        for lin in (self.layer_0, self.layer_1) + ((self.shortcut,) if self.shortcut is not None else ()):
            _he_normal_(lin.weight)
            if lin.bias is not None:
                nn.init.zeros_(lin.bias)

    def forward(self, x):
        r = _wide_linear(self.layer_1, nn.functional.elu(_wide_linear(self.layer_0, nn.functional.elu(x))))
        return (_wide_linear(self.shortcut, x) if self.shortcut is not None else x) + r


class GraspReadout(nn.Module):
    def __init__(self, n_offsets, use_bias=True):
        super().__init__()
        self.activation_downscale = nn.ModuleList([nn.Linear(128, 64) for _ in range(N_FUSED)])
        self.combined_activation_downscale = nn.Linear(4 * 64, 64)
        self.block_0 = ResNetMLPBlock(n_offsets * 64, 128, 64, transform_shortcut=True)
        self.block_1 = ResNetMLPBlock(64, 64, 64)
        self.output_layer = nn.Linear(64, 1, bias=use_bias)
        for lin in self.activation_downscale:
            _he_normal_(lin.weight)
            nn.init.zeros_(lin.bias)
        nn.init.xavier_uniform_(self.combined_activation_downscale.weight)      # Keras default glorot_uniform
        nn.init.zeros_(self.combined_activation_downscale.bias)
        _he_normal_(self.output_layer.weight)
        if self.output_layer.bias is not None:
            nn.init.zeros_(self.output_layer.bias)

    fused_head = True      # the per-point layers as fused HIP passes (csrc/grasp_head.hip); False: Linear by Linear (torch + gemm_ops)
    fused_tail = False     # the per-pose layers as fused HIP passes (csrc/grasp_tail.hip, grasp_tail_train.hip); False: torch + gemm_ops

    def forward(self, acts):
        """acts: 4 x (B, np, n5, 128), or the same stacked as one (4, B, np, n5, 128) tensor -> (B, np)."""
        stacked = acts if isinstance(acts, torch.Tensor) else None
        first = acts[0]
        b, n_p, n5 = first.shape[0], first.shape[1], first.shape[2]
        if self.fused_head and first.is_cuda and first.dtype == torch.float32:
            a = (stacked if stacked is not None else torch.stack(list(acts))).reshape(N_FUSED, -1, 128)
            w4 = torch.stack([lin.weight for lin in self.activation_downscale])
            b4 = torch.stack([lin.bias for lin in self.activation_downscale])
            x = _HeadFn.apply(a, w4, b4, self.combined_activation_downscale.weight, self.combined_activation_downscale.bias)
            x = x.reshape(b, n_p, n5 * 64)                                       # 'b np n5 d -> b np (n5 d)'
        else:
            acts = list(acts.unbind(0)) if stacked is not None else acts
            ds = [nn.functional.elu(_wide_linear(lin, a)) for lin, a in zip(self.activation_downscale, acts)]
            x = nn.functional.elu(_wide_linear(self.combined_activation_downscale, torch.cat(ds, -1)))
            x = x.reshape(x.shape[0], x.shape[1], -1)                            # 'b np n5 d -> b np (n5 d)'
        if self.fused_tail and x.is_cuda and x.dtype == torch.float32:
            b0, b1, out = self.block_0, self.block_1, self.output_layer
            weights = (b0.layer_0.weight, b0.layer_0.bias, b0.layer_1.weight, b0.layer_1.bias, b0.shortcut.weight, b1.layer_0.weight,
                       b1.layer_0.bias, b1.layer_1.weight, b1.layer_1.bias, out.weight, out.bias)
            x2d = x.reshape(-1, x.shape[-1])
            if torch.is_grad_enabled():
                return _TailFn.apply(x2d, *weights).reshape(x.shape[:-1])
            packed = ops.grasp_tail_pack(*(tuple(t.detach().contiguous() for t in w) for w in (weights[:5], weights[5:9])),
                                         (out.weight.detach().contiguous(), None if out.bias is None else out.bias.detach()))
            return ops.grasp_tail_fwd(x2d.contiguous(), packed, stash=False).reshape(x.shape[:-1])
        x = self.block_1(self.block_0(x))
        return self.output_layer(torch.relu(x))[..., 0]


# ---- pose algebra (model_v4.py:67-101, 192-206) -------------------------------------------------------------
def _rot_y(angle):
    c, s = math.cos(angle), math.sin(angle)
    return np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]])


def grasp_offsets(n_5d_poses=7):
    """`transforms_to_check`: 6 gripper-part bases x n_5d_poses steps along the local z axis -> (6*n_5d_poses, 4, 4).
    (Affine(rotation=[0, +-pi/2, 0]) is scipy's extrinsic 'xyz' Euler = a rotation about y.)"""
    bx, by, bz = 0.02, 0.015, 0.0125
    step = (bx - 0.005) / ((n_5d_poses - 1) / 2)

    def affine(t, ry=0.0):
        m = np.eye(4)
        m[:3, :3] = _rot_y(ry)
        m[:3, 3] = t
        return m
    bases = [affine([0, by, 0]), affine([0, -by, 0]), affine([-bx, by, bz], math.pi / 2), affine([bx, by, bz], -math.pi / 2),
             affine([-bx, -by, bz], math.pi / 2), affine([bx, -by, bz], -math.pi / 2)]
    c = int((n_5d_poses - 1) / 2)
    steps = [affine([0.0, 0.0, i * step]) for i in range(-c, c + 1)]
    return np.array([b @ t for b in bases for t in steps], dtype=np.float32)


def rotation_from_quaternion(q):
    """tensorflow_graphics rotation_matrix_3d.from_quaternion (x, y, z, w; the input is used as given, not normalised)."""
    x, y, z, w = q.unbind(-1)
    tx, ty, tz = 2 * x, 2 * y, 2 * z
    twx, twy, twz = tx * w, ty * w, tz * w
    txx, txy, txz = tx * x, ty * x, tz * x
    tyy, tyz, tzz = ty * y, tz * y, tz * z
    m = torch.stack([1 - (tyy + tzz), txy - twz, txz + twy,
                     txy + twz, 1 - (txx + tzz), tyz - twx,
                     txz - twy, tyz + twx, 1 - (txx + tyy)], -1)
    return m.reshape(q.shape[:-1] + (3, 3))


def rotation_from_6d(r6):
    """model_v4.py:196-204: both halves normalised (not orthogonalised), third column their cross product."""
    r1 = r6[..., :3] / r6[..., :3].norm(dim=-1, keepdim=True)
    r2 = r6[..., 3:] / r6[..., 3:].norm(dim=-1, keepdim=True)
    r3 = torch.linalg.cross(r1, r2)
    return torch.stack([r1, r2, r3], -1)


def t_m_to_h_matrix(translations, rot):
    top = torch.cat([rot, translations[..., None]], -1)
    # (0,0,0,1) built on the device: a host constant would be an H2D copy, which a graph capture refuses
    last = torch.cat([torch.zeros_like(translations), torch.ones_like(translations[..., :1])], -1)[..., None, :]
    return torch.cat([top, last], -2)


def cosine_similarity_loss(y_true, y_pred):
    """tf.keras.losses.CosineSimilarity(axis=-1): -mean(sum(l2n(y_true) * l2n(y_pred)))."""
    def l2n(x):
        return x * torch.rsqrt(torch.clamp((x * x).sum(-1, keepdim=True), min=1e-12))
    return -(l2n(y_true) * l2n(y_pred)).sum(-1).mean()


def kl_divergence(y_true, y_pred):
    """tf.keras.losses.KLDivergence(reduction=NONE): per batch element, inputs clipped to [1e-7, 1]."""
    y_true = torch.clamp(y_true, 1e-7, 1.0)
    y_pred = torch.clamp(y_pred, 1e-7, 1.0)
    return (y_true * torch.log(y_true / y_pred)).sum(-1)


def categorical_crossentropy_from_logits(y_true, y_pred):
    """tf.keras.losses.CategoricalCrossentropy(from_logits=True) (train_language.py:56-57): -sum(y_true * log_softmax(logits)) over the
    last axis, mean over the batch (SUM_OVER_BATCH_SIZE)."""
    return -(y_true * torch.log_softmax(y_pred, -1)).sum(-1).mean()


# ---- checkpoint files (model_v4.py:132-174) -----------------------------------------------------------------
_BACKBONE_FILES = ('fine_embedding', 'fine_readout')        # what MVVNeRFRenderer.store writes for the fine MLP (model._SUBMODELS)


def store_trunk(path, trunk_net):
    """Write a flat Keras-order MLP (247 300 floats) as `{path}_fine_embedding.pt` / `{path}_fine_readout.pt`, the two fine-MLP files of
    MVVNeRFRenderer.store, so either model's `load_backbone` / `load` reads them."""
    flat = torch.as_tensor(trunk_net, dtype=torch.float32).reshape(-1).detach().cpu()
    n_emb = flat.numel() - (128 * 4 + 4)          # model._EMB_PARAMS: the trunk; the rest is the (unused here) colour read-out
    for name, t in zip(_BACKBONE_FILES, (flat[:n_emb], flat[n_emb:])):
        torch.save(t.clone(), f'{path}_{name}.pt')


def _quaternion_pose_map(offsets):
    """rotation_from_quaternion is a quadratic form in q = (x, y, z, w): R_ik = delta_ik + sum_ab q_a q_b A[ab, ik].  Folded with the gripper
    offsets, the query points and directions of ALL offsets are one product of the 16 pair products q_a q_b with a constant matrix:
        points[o, i] = off_t[o, i] + t_i + sum_ab q_a q_b (A[ab, i, :] . off_t[o]),     dirs[o, i] = off_z[o, i] + sum_ab q_a q_b (A[ab, i, :] . off_z[o])
    -> (16, 2 * n5 * 3) float32: columns [points (o, i) | dirs (o, i)].  Same polynomial as the reference's expression tree
    (tensorflow_graphics from_quaternion, then transforms @ offsets: model_v4.py:67-101, 222-226), different summation order."""
    a = np.zeros((4, 4, 3, 3))
    x, y, z, w = 0, 1, 2, 3
    def add(i, k, terms):
        for (p, q, c) in terms:
            a[p, q, i, k] += c
    add(0, 0, [(y, y, -2), (z, z, -2)]); add(0, 1, [(x, y, 2), (z, w, -2)]); add(0, 2, [(x, z, 2), (y, w, 2)])
    add(1, 0, [(x, y, 2), (z, w, 2)]); add(1, 1, [(x, x, -2), (z, z, -2)]); add(1, 2, [(y, z, 2), (x, w, -2)])
    add(2, 0, [(x, z, 2), (y, w, -2)]); add(2, 1, [(y, z, 2), (x, w, 2)]); add(2, 2, [(x, x, -2), (y, y, -2)])
    off_t, off_z = offsets[:, :3, 3].astype(np.float64), offsets[:, :3, 2].astype(np.float64)          # (n5, 3)
    pts = np.einsum('pqik,ok->pqoi', a, off_t).reshape(16, -1)
    drs = np.einsum('pqik,ok->pqoi', a, off_z).reshape(16, -1)
    return np.concatenate([pts, drs], 1).astype(np.float32)


class LanguageNeRF(nn.Module):
    """model_v4.py:37-330 without the encoders: `trunk_net` is the frozen fine_embedding (+ unused read-out) in the flat
    Keras order of MVVNeRFRenderer.fine_net; `combined_features` is passed in."""

    def __init__(self, trunk_net, n_points_train=5, n_views=1, n_5d_poses=7, batch_size=1, rotation_representation='quaternion',
                 softmax_before_loss=False, device='cuda:0'):
        super().__init__()
        if rotation_representation not in ('quaternion', '6d'):
            raise ValueError('Unknown rotation representation: ' + rotation_representation)
        self.device_ = torch.device(device)
        self.n_views, self.n_points_train, self.batch_size = n_views, n_points_train, batch_size
        self.rotation_representation = rotation_representation
        self.softmax_before_loss = softmax_before_loss
        self.register_buffer('trunk_net', torch.as_tensor(trunk_net, dtype=torch.float32).reshape(-1).clone())
        self.register_buffer('transforms_to_check', torch.from_numpy(grasp_offsets(n_5d_poses)))      # (n5,4,4)
        self.n_transforms_to_check = self.transforms_to_check.shape[0]
        self.register_buffer('_pose_map', torch.from_numpy(_quaternion_pose_map(self.transforms_to_check.numpy())))   # (16, 2 n5 3)
        self.grasp_readout = GraspReadout(self.n_transforms_to_check, use_bias=True)
        self.translations = nn.Parameter(torch.zeros(batch_size, n_points_train, 3))
        rot_dim = 4 if rotation_representation == 'quaternion' else 6
        self.rotations = nn.Parameter(torch.zeros(batch_size, n_points_train, rot_dim))
        self.pose_variables = [self.translations, self.rotations]
        self.loss = kl_divergence if softmax_before_loss else None
        self.optimizer = None
        self._graph_mode, self._graph, self._g_static, self._g_out, self._g_calls = False, None, None, None, 0
        self.fused_step, self.loss_weights, self._fs = False, (1.0, 1.0, 1.0), None
        self.fused_optimizer, self._opt, self._learning_rate, self._trunk_images = False, None, 1e-4, None
        self.to(self.device_)

    # -- reference API --
    def compile(self, optimizer=None, loss=None, learning_rate=1e-4, graph=False, fused_tail=None, fused_step=None, loss_weights=None,
                fused_optimizer=None):
        """graph=True: `train_step` is captured ONCE as a HIP graph (torch.cuda.CUDAGraph) and replayed: the step is ~740 launches of
        3-500 us that the host cannot issue as fast as the GPU runs them - 6.6 ms per replay against 8-10.7 ms eager at the cfg3 shape
        (profiles/r02_language_step_graph.md).  The graph fixes shapes and addresses:
        inputs are staged into the buffers `graph_inputs()` returns (a producer that writes `combined_features` there in place skips the
        copy), the optimizer is this method's own Adam (capturable).  The first two steps run eagerly (they load every kernel and size
        the allocator pools), the third is captured.
        fused_tail: True / False runs the read-out's per-pose layers as fused HIP passes (GraspReadout.fused_tail) or layer by layer through
        torch; None keeps the current setting.  A captured graph is dropped either way (compile() always starts a new one).
        fused_step: True makes `loss_and_grads` one call of mvnerf_language_loss_and_grads (csrc/language_api.hip: both passes, the pose
        algebra, the losses and every weight gradient as HIP launches on the current stream, no autograd graph); the parameters' `.grad` are
        views into its flat gradient, the optimizer and `graph=True` work as before.  False is the autograd path; None keeps the setting.
        loss_weights: (landscape, grad_t, grad_r) factors of the three losses in the total that is differentiated (the reference: 1, 1, 1;
        the returned losses stay unweighted); None keeps the setting.
        fused_optimizer: True makes `train_step` one call of mvnerf_language_train_step (csrc/language_opt.hip): the head gather, the
        fused step and clip + Keras Adam on the parameters where they live, with the bias-corrected rate formed on the device from a step
        counter - in eager mode and under graph=True, whose captured graph then holds no torch optimizer.  It needs fused_step=True and
        optimizer=None; `model.optimizer` is None in this mode, `optimizer_steps()` reads the counter, the moments and the counter start
        at zero at every compile(), and the trunk's weight images are kept across steps (`invalidate_trunk`).  The update is Keras's,
        p - lr_t m / (sqrt(v) + eps), not torch.optim.Adam's (eps elsewhere).  False is the torch optimizer; None keeps it."""
        for name, flag in (('fused_step', fused_step), ('fused_optimizer', fused_optimizer)):
            if flag is not None and not isinstance(flag, bool):
                raise ValueError(f'{name} must be True or False (compile: or None to keep the setting), got {flag!r}')
        if self.fused_optimizer if fused_optimizer is None else fused_optimizer:
            if not (self.fused_step if fused_step is None else fused_step):
                raise ValueError('fused_optimizer=True needs fused_step=True: the update reads the flat gradient of the C step')
            if optimizer is not None:
                raise ValueError('fused_optimizer=True is its own Adam inside the C call; pass learning_rate instead of an optimizer')
        if fused_optimizer is not None and fused_optimizer != self.fused_optimizer:
            self.fused_optimizer, self._trunk_images = fused_optimizer, None       # the optimizer itself is built below, once
        if fused_tail is not None:
            self.set_fused_tail(fused_tail)
        if fused_step is not None:
            self.set_fused_step(fused_step)
        if loss_weights is not None:
            if len(loss_weights) != 3:
                raise ValueError(f'loss_weights: (landscape, grad_t, grad_r), got {loss_weights!r}')
            self.loss_weights = tuple(float(x) for x in loss_weights)
        if graph and optimizer is not None:
            raise ValueError('graph=True builds its own capturable Adam; pass learning_rate instead of an optimizer')
        self._learning_rate = float(learning_rate)
        if self.fused_optimizer:
            self.optimizer, self._opt = None, self._adam_state(learning_rate)
        else:
            self._opt = None
            self.optimizer = optimizer or torch.optim.Adam(self.grasp_readout.parameters(), lr=learning_rate, eps=1e-7, capturable=bool(graph))
        if loss is not None:
            self.loss = loss
        self._graph_mode, self._graph, self._g_static, self._g_out, self._g_calls = bool(graph), None, None, None, 0

    def set_fused_tail(self, fused_tail):
        """GraspReadout.fused_tail on this model's read-out without touching the optimizer; a change drops a captured step (the next
        train_step runs its two eager steps and captures again)."""
        if not isinstance(fused_tail, bool):
            raise ValueError(f'fused_tail must be True or False (compile: or None to keep the setting), got {fused_tail!r}')
        if fused_tail != self.grasp_readout.fused_tail:
            self.grasp_readout.fused_tail = fused_tail
            self._graph, self._g_out, self._g_calls = None, None, 0

    def set_fused_step(self, fused_step):
        """The step up to the optimizer as one C call (compile(fused_step=...)) without touching the optimizer; a change drops a captured
        step, like set_fused_tail."""
        if not isinstance(fused_step, bool):
            raise ValueError(f'fused_step must be True or False (compile: or None to keep the setting), got {fused_step!r}')
        if not fused_step and self.fused_optimizer:
            raise ValueError('fused_optimizer is on and needs fused_step=True; switch it off first (set_fused_optimizer(False))')
        if fused_step != self.fused_step:
            self.fused_step = fused_step
            self._graph, self._g_out, self._g_calls = None, None, 0

    def set_fused_optimizer(self, fused_optimizer, learning_rate=None):
        """The optimizer inside the C call (compile(fused_optimizer=...)).  Switching it on needs fused_step and starts new moments and a
        new step counter at `learning_rate` (None: the last compile()'s); switching it off puts torch's Adam back at that rate.  A change
        drops a captured step, like set_fused_step."""
        if not isinstance(fused_optimizer, bool):
            raise ValueError(f'fused_optimizer must be True or False (compile: or None to keep the setting), got {fused_optimizer!r}')
        if fused_optimizer and not self.fused_step:
            raise ValueError('fused_optimizer=True needs fused_step=True: the update reads the flat gradient of the C step')
        if fused_optimizer == self.fused_optimizer:
            return
        lr = self._learning_rate if learning_rate is None else float(learning_rate)
        self.fused_optimizer, self._trunk_images = fused_optimizer, None
        if fused_optimizer:
            self.optimizer, self._opt = None, self._adam_state(lr)
        else:
            self._opt = None
            self.optimizer = torch.optim.Adam(self.grasp_readout.parameters(), lr=lr, eps=1e-7, capturable=self._graph_mode)
        self._graph, self._g_out, self._g_calls = None, None, 0

    def _adam_state(self, learning_rate):
        """Zero moments in the layout of the flat gradient and a zero step counter, on the model's device."""
        total = ops.language_grad_layout(self.n_transforms_to_check)[1]
        dev = self.device_
        return {'m': torch.zeros(total, dtype=torch.float32, device=dev), 'v': torch.zeros(total, dtype=torch.float32, device=dev),
                'step': torch.zeros(1, dtype=torch.int64, device=dev), 'lr': float(learning_rate)}

    def optimizer_steps(self):
        """Completed updates of the fused optimizer: one host read of its device counter, on demand only."""
        if not self.fused_optimizer:
            raise RuntimeError('optimizer_steps() reads the counter of compile(fused_optimizer=True)')
        return int(self._opt['step'].item())

    def invalidate_trunk(self):
        """For a caller that wrote `trunk_net` through a raw pointer (no version bump) under fused_optimizer: the next step packs the
        trunk's weight images again, into the buffers it has (a captured graph stays valid)."""
        if self._trunk_images is not None:
            self._trunk_images['key'] = None

    # -- checkpoints (model_v4.py:132-174): torch.save'd tensors, one file per sub-model, load() -> False when a file is missing --
    # The reference also writes and reads `{path}_visual_features` / `{path}_combine_clip_visual`; here the feature map is an input
    # (DESIGN.md 7), so those files are neither written nor read.  Loading copies IN PLACE into `trunk_net` and the read-out parameters:
    # the Adam state, a captured training graph and DNGFOptimizer's bound views all hold those tensors.
    def load_backbone(self, path, verbose=True, producer=None):
        """The frozen trunk from `{path}_fine_embedding.pt` + `{path}_fine_readout.pt` (MVVNeRFRenderer.store's fine MLP) -> True, or
        False (nothing changed) if either file is missing.
        producer: a LanguageFeatureProducer (anything with `visual_features` and `combine_clip_visual`) - then
        `{path}_visual_features.pt` and `{path}_combine_clip_visual.pt`, as `MVVNeRFRenderer.store(path, encoders=True)` wrote them, are
        loaded into it as well (model_v4.py:132-152); False (nothing changed) if either is missing, ValueError naming the first key
        that does not match."""
        from .model import ENCODER_SUBMODELS, check_state_dict
        files = [f'{path}_{name}.pt' for name in _BACKBONE_FILES]
        encoder_files = [f'{path}_{name}.pt' for name in ENCODER_SUBMODELS] if producer is not None else []
        for f in files + encoder_files:
            if not os.path.exists(f):
                if verbose:
                    print(f'{f} does not exist')
                return False
        flat = torch.cat([torch.load(f, weights_only=True).reshape(-1) for f in files])
        if flat.numel() != self.trunk_net.numel():
            raise ValueError(f'{path}: {flat.numel()} backbone parameters, expected {self.trunk_net.numel()}')
        states = [torch.load(f, weights_only=True) for f in encoder_files]
        for name, state, f in zip(ENCODER_SUBMODELS, states, encoder_files):
            check_state_dict(getattr(producer, name), state, f)
        for name, state in zip(ENCODER_SUBMODELS, states):
            getattr(producer, name).load_state_dict(state)
        with torch.no_grad():
            self.trunk_net.copy_(flat)
        if self.trunk_net.is_cuda:
            # the query kernels read the same packed_split image as the render passes: its fp16 two-piece form is only correct for
            # |w| < 1023 (include/mvnerf_hip.h, MVNERF_F16X3_MAX_WEIGHT); checked once per load, one host read
            max_w = float(ops.net_range(self.trunk_net.detach())[0])
            if not range_policy.below(max_w, range_policy.limits()[0]):
                warnings.warn(f'{path}: backbone ' + range_policy.describe(max_w, None), RuntimeWarning, stacklevel=2)
        return True

    def store(self, path):
        """`{path}_fine_embedding.pt`, `{path}_fine_readout.pt` (the trunk) and `{path}_grasp_readout.pt` (the GraspReadout state dict)."""
        store_trunk(path, self.trunk_net)
        torch.save({k: v.detach().cpu().clone() for k, v in self.grasp_readout.state_dict().items()}, f'{path}_grasp_readout.pt')

    def load(self, path):
        """load_backbone + the read-out -> True, or False (nothing changed) if any of the three files is missing."""
        readout_file = f'{path}_grasp_readout.pt'
        if not all(os.path.exists(f'{path}_{name}.pt') for name in _BACKBONE_FILES):
            print(f'backbone models at {path} do not exist')
            return False
        if not os.path.exists(readout_file):
            print(f'{readout_file} does not exist')
            return False
        state = torch.load(readout_file, weights_only=True)
        own = self.grasp_readout.state_dict()
        if set(state) != set(own) or any(state[k].shape != own[k].shape for k in own):
            raise ValueError(f'{readout_file}: the GraspReadout variables do not match this model')
        self.load_backbone(path, verbose=False)
        with torch.no_grad():
            for k, t in own.items():                 # state_dict() tensors share the parameters' storage
                t.copy_(state[k])
        return True

    def set_pose(self, translations, rotations):
        with torch.no_grad():
            self.translations.copy_(torch.as_tensor(translations, dtype=torch.float32))
            self.rotations.copy_(torch.as_tensor(rotations, dtype=torch.float32))

    def compute_matrices(self):
        rot = (rotation_from_quaternion(self.rotations) if self.rotation_representation == 'quaternion'
               else rotation_from_6d(self.rotations))
        return t_m_to_h_matrix(self.translations, rot)

    def trunk_state(self, inputs, batched_features, compute_dtype='f32'):
        """inputs[4:7] = src_images (B,V,H,W,3), src_intrinsics (B,V,4,4), src_extrinsics_inv (B,V,4,4) (model_v4.py:209-213)."""
        dev = self.device_
        f32 = lambda t: torch.as_tensor(t, dtype=torch.float32).to(dev)
        images = self._trunk_weight_images() if self.fused_optimizer and compute_dtype == 'f32' else None
        return TrunkState(f32(inputs[4]), f32(batched_features), f32(inputs[5]), f32(inputs[6]), self.trunk_net, compute_dtype, images)

    def _trunk_weight_images(self):
        """(packed, packed_split, bwd_streams) of the frozen trunk, kept while (trunk_net.data_ptr(), trunk_net._version) is unchanged
        (load_backbone / load copy in place: a new version); packed again INTO the same buffers otherwise, so that a captured step,
        which holds their addresses, reads the new trunk."""
        net = self.trunk_net
        key = (net.data_ptr(), net._version)
        kept = self._trunk_images
        if kept is None:
            kept = self._trunk_images = {'key': key, 'images': (ops.pack_net(net), ops.pack_net_split(net), ops.pack_bwd_streams(net))}
        elif kept['key'] != key:
            for old, new in zip(kept['images'], (ops.pack_net(net), ops.pack_net_split(net), ops.pack_bwd_streams(net))):
                old.copy_(new)
            kept['key'] = key
        return kept['images']

    def _query_points(self, transforms):
        """poses = transforms @ offsets (model_v4.py:222-226) reduced to what is used of them: points = the poses' translations, dirs =
        their z axes.  With affine offsets (last row 0 0 0 1) that is R t_o + t and R z_o - two (B np 3, 3) x (3, n5) products instead of
        B np n5 batched 4 x 4 products, for which the library GEMM takes 590 us (16 x 16 tiles over 64 512 batches)."""
        rot, trans = transforms[..., :3, :3], transforms[..., :3, 3]
        off_t, off_z = self.transforms_to_check[:, :3, 3], self.transforms_to_check[:, :3, 2]      # (n5, 3)
        points = torch.einsum('bpik,ok->bpoi', rot, off_t) + trans[:, :, None, :]
        dirs = torch.einsum('bpik,ok->bpoi', rot, off_z)
        b = transforms.shape[0]
        return points.reshape(b, -1, 3), dirs.reshape(b, -1, 3)                                     # query order (np, n5)

    def _query_points_from_pose(self, translations, rotations):
        """compute_matrices + _query_points for the quaternion representation in four launches instead of about thirty (and as many again
        in each of the two backward passes): q (x) q, one (B np, 16) x (16, 6 n5) product, the offsets' constant, the translation."""
        b, n_p = rotations.shape[:2]
        n5 = self.n_transforms_to_check
        qq = (rotations[..., :, None] * rotations[..., None, :]).reshape(b * n_p, 16)
        both = (qq @ self._pose_map).reshape(b, n_p, 2, n5, 3)
        off_t, off_z = self.transforms_to_check[:, :3, 3], self.transforms_to_check[:, :3, 2]
        points = both[:, :, 0] + off_t + translations[:, :, None, :]
        dirs = both[:, :, 1] + off_z
        return points.reshape(b, -1, 3), dirs.reshape(b, -1, 3)

    def _call(self, inputs, transforms, n_points, batched_features, state=None):
        """model_v4.py:211-265: poses = transforms @ offsets; points = their translations, directions = their z axes;
        trunk -> fused activations (b, np, n5, 128) x 4 -> GraspReadout -> (B, np)."""
        state = state or self.trunk_state(inputs, batched_features)
        if transforms is None:                           # the training step: straight from the pose variables (quaternion representation)
            points, dirs = self._query_points_from_pose(self.translations, self.rotations)
            b = self.translations.shape[0]
        else:
            points, dirs = self._query_points(transforms)
            b = transforms.shape[0]
        acts = TrunkField.apply(points, dirs, state)                                     # (4, B, np*n5, 128)
        acts = acts.reshape(N_FUSED, b, n_points, self.n_transforms_to_check, 128)
        return self.grasp_readout(acts)

    def infer(self, inputs, transforms, n_points_infer, batched_features, compute_dtype='f32'):
        """model_v4.py:208-209.  compute_dtype='bf16' evaluates the trunk on the bf16 MFMA kernel (gradients in bf16: TrunkState(compute_dtype='bf16'))."""
        transforms = torch.as_tensor(transforms, dtype=torch.float32).to(self.device_)
        with torch.no_grad():
            if compute_dtype == 'f32':
                return self._call(inputs, transforms, n_points_infer, batched_features)
            if compute_dtype != 'bf16':
                raise ValueError("compute_dtype must be 'f32' or 'bf16'")
            f32 = lambda t: torch.as_tensor(t, dtype=torch.float32).to(self.device_).contiguous()
            geo = (f32(inputs[4]), f32(batched_features), f32(inputs[5]), f32(inputs[6]))
            packed, packed16 = self._infer_nets16()
            b = transforms.shape[0]
            points, dirs = (t.contiguous() for t in self._query_points(transforms))
            z = torch.zeros(b, points.shape[1], 1, dtype=torch.float32, device=self.device_)
            _, acts = ops.field_eval_bf16(points, dirs, z, *geo, packed, packed16, return_fused_acts=True)
            acts = acts.reshape(N_FUSED, b, n_points_infer, self.n_transforms_to_check, 128)
            return self.grasp_readout(list(acts.unbind(0)))

    def _infer_nets16(self):
        """The two weight images infer(compute_dtype='bf16') reads, packed once per value of trunk_net (its storage and version counter)."""
        key = (self.trunk_net.data_ptr(), self.trunk_net._version)
        cached = getattr(self, '_nets16_cache', None)
        if cached is None or cached[0] != key:
            cached = (key, ops.pack_net(self.trunk_net), ops.pack_net_bf16(self.trunk_net))
            object.__setattr__(self, '_nets16_cache', cached)
        return cached[1], cached[2]

    def loss_and_grads(self, data, combined_features):
        """The body of train_step (model_v4.py:277-318) up to the optimizer: returns (dict of losses, prediction)."""
        if self.fused_step:
            return self._loss_and_grads_fused(data, combined_features)
        inputs, labels = data
        dev = self.device_
        lab = [torch.as_tensor(l, dtype=torch.float32).to(dev) for l in labels]
        state = self.trunk_state(inputs, combined_features)
        self.set_pose(inputs[0], inputs[1])
        fast = self.rotation_representation == 'quaternion'
        y_pred = self._call(inputs, None if fast else self.compute_matrices(), self.n_points_train, combined_features, state)
        if self.softmax_before_loss:
            y_pred = torch.softmax(y_pred, -1)
        landscape_loss = self.loss(lab[0], y_pred)
        self.set_pose(inputs[2], inputs[3])
        prediction = self._call(inputs, None if fast else self.compute_matrices(), self.n_points_train, combined_features, state)
        grads = torch.autograd.grad(prediction.sum(), self.pose_variables, create_graph=True)
        loss_t = cosine_similarity_loss(lab[1], grads[0])
        if self.rotation_representation == 'quaternion':
            loss_r = cosine_similarity_loss(lab[2], grads[1])
        else:
            loss_r = cosine_similarity_loss(lab[2][..., :3], grads[1][..., :3]) + cosine_similarity_loss(lab[2][..., 3:], grads[1][..., 3:])
        if self.loss_weights == (1.0, 1.0, 1.0):
            loss = loss_t + loss_r + landscape_loss
        else:
            w_land, w_t, w_r = self.loss_weights
            loss = w_t * loss_t + w_r * loss_r + w_land * landscape_loss
        for prm in self.grasp_readout.parameters():
            prm.grad = None
        loss.sum().backward(inputs=list(self.grasp_readout.parameters()))
        return {'landscape_loss': landscape_loss.detach().mean(), 'grad_loss_t': loss_t.detach(), 'grad_loss_r': loss_r.detach(),
                'pred': prediction.detach().mean()}, prediction.detach()

    # -- the same body as one C call (compile(fused_step=True); csrc/language_api.hip) --
    def _readout_tensors(self):
        """The read-out's parameters in the order of mvnerf_language_call: the four per-activation layers, then (wc, bc), then the tail's 11."""
        ro = self.grasp_readout
        b0, b1, out = ro.block_0, ro.block_1, ro.output_layer
        tail = {'w0': b0.layer_0.weight, 'b0': b0.layer_0.bias, 'w1': b0.layer_1.weight, 'b1': b0.layer_1.bias, 'ws': b0.shortcut.weight,
                'w0b': b1.layer_0.weight, 'b0b': b1.layer_0.bias, 'w1b': b1.layer_1.weight, 'b1b': b1.layer_1.bias, 'w_out': out.weight,
                'b_out': out.bias}
        return list(ro.activation_downscale), ro.combined_activation_downscale, tail

    def _fused_buffers(self, key):
        """Everything the C step writes, allocated once per shape: the flat gradient (the parameters' `.grad` are views into it), the
        prediction, the four scalars, the landscape poses, the stacked head weights and the workspace."""
        if self._fs is not None and self._fs['key'] == key:
            return self._fs
        b, v, h, w, n_p, n5, rd = key
        dev = self.device_
        layout, total = ops.language_grad_layout(n5)
        f32 = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)
        grads = torch.zeros(total, dtype=torch.float32, device=dev)
        view = lambda name: grads[layout[name][0]:layout[name][0] + int(np.prod(layout[name][1]))].view(layout[name][1])
        heads, comb, tail = self._readout_tensors()
        grad_views = [(comb.weight, view('wc')), (comb.bias, view('bc'))]
        grad_views += [(lin.weight, view('w4')[k]) for k, lin in enumerate(heads)] + [(lin.bias, view('b4')[k]) for k, lin in enumerate(heads)]
        grad_views += [(prm, view(name)) for name, prm in tail.items()]
        self._fs = {'key': key, 'grads': grads, 'grad_views': grad_views, 'prediction': f32(b, n_p), 'scalars': f32(4), 't_l': f32(b, n_p, 3),
                    'r_l': f32(b, n_p, rd), 'w4': f32(4, 64, 128), 'b4': f32(4, 64),
                    'workspace': torch.empty(ops.language_workspace_bytes(b, v, h, w, n_p, n5), dtype=torch.uint8, device=dev)}
        return self._fs

    def _fused_call(self, data, combined_features, stack_heads):
        """The filled mvnerf_language_call of one step -> (call, its buffers, the tensor whose device and stream the call runs on).
        stack_heads: gather the four per-activation layers into the stacked images here (mvnerf_language_train_step does it itself)."""
        if self.loss is kl_divergence and self.softmax_before_loss:
            kind = 'kl_divergence'
        elif self.loss is categorical_crossentropy_from_logits and not self.softmax_before_loss:
            kind = 'cross_entropy'
        else:
            raise ValueError('fused_step: the C step knows kl_divergence after a softmax and categorical_crossentropy_from_logits without one '
                             '(train_language.select_loss); use fused_step=False for another loss')
        if self.grasp_readout.output_layer.bias is None:
            raise ValueError('fused_step: the read-out needs its output bias')
        inputs, labels = data
        dev = self.device_
        lab = [torch.as_tensor(l, dtype=torch.float32).to(dev).contiguous() for l in labels]
        state = self.trunk_state(inputs, combined_features)
        images, features = state.geo[0], state.geo[1]
        b, v, h, w = images.shape[:4]
        n_p, n5, rd = self.n_points_train, self.n_transforms_to_check, self.rotations.shape[-1]
        fs = self._fused_buffers((b, v, h, w, n_p, n5, rd))
        heads, comb, tail = self._readout_tensors()
        with torch.no_grad():
            fs['t_l'].copy_(torch.as_tensor(inputs[0], dtype=torch.float32), non_blocking=True)
            fs['r_l'].copy_(torch.as_tensor(inputs[1], dtype=torch.float32), non_blocking=True)
            if stack_heads:
                torch.stack([lin.weight.detach() for lin in heads], out=fs['w4'])
                torch.stack([lin.bias.detach() for lin in heads], out=fs['b4'])
        self.set_pose(inputs[2], inputs[3])
        call = ops.language_call(*state.geo, state.packed, state.packed_split, state.bwd_streams,
                                 (fs['w4'], fs['b4'], comb.weight.detach(), comb.bias.detach()), [t.detach() for t in tail.values()],
                                 self.transforms_to_check, (fs['t_l'], fs['r_l'], self.translations.detach(), self.rotations.detach()), lab, kind,
                                 self.loss_weights, fs['grads'], fs['prediction'], fs['scalars'], fs['workspace'])
        return call, fs, features

    def _loss_and_grads_fused(self, data, combined_features):
        call, fs, features = self._fused_call(data, combined_features, True)
        ops.language_loss_and_grads(call, features)
        for prm, g in fs['grad_views']:
            prm.grad = g
        s = fs['scalars'].clone()
        return {'landscape_loss': s[0], 'grad_loss_t': s[1], 'grad_loss_r': s[2], 'pred': s[3]}, fs['prediction'].clone()

    def _train_step_fused(self, data, combined_features):
        """compile(fused_optimizer=True): the whole step, update included, as one call of mvnerf_language_train_step."""
        call, fs, features = self._fused_call(data, combined_features, False)
        heads, comb, tail = self._readout_tensors()
        opt = self._opt
        adam = ops.language_adam_state([lin.weight.detach() for lin in heads], [lin.bias.detach() for lin in heads], comb.weight.detach(),
                                       comb.bias.detach(), [t.detach() for t in tail.values()], fs['w4'], fs['b4'], opt['m'], opt['v'],
                                       opt['step'], opt['lr'])
        ops.language_train_step(call, adam, features)
        for prm, g in fs['grad_views']:
            prm.grad = g
        s = fs['scalars'].clone()
        return {'landscape_loss': s[0], 'grad_loss_t': s[1], 'grad_loss_r': s[2], 'pred': s[3]}

    def _clip_and_step(self):
        for prm in self.grasp_readout.parameters():                      # optimize(): clip-by-value 1.0, then Adam
            if prm.grad is not None:
                prm.grad.clamp_(-1.0, 1.0)
        self.optimizer.step()

    def train_step(self, data, combined_features):
        if self.optimizer is None and not self.fused_optimizer:
            self.compile()
        if self._graph_mode:
            return self._train_step_graphed(data, combined_features)
        return self._step(data, combined_features)

    def _step(self, data, combined_features):
        if self.fused_optimizer:
            return self._train_step_fused(data, combined_features)
        out, _ = self.loss_and_grads(data, combined_features)
        self._clip_and_step()
        return out

    # -- the step as one HIP graph (compile(graph=True)) --
    _GRAPH_INPUTS = ('translations_landscape', 'rotations_landscape', 'translations_grad', 'rotations_grad', 'src_images', 'src_intrinsics',
                     'src_extrinsics_inv', 'combined_features', 'label_landscape', 'label_grad_t', 'label_grad_r')

    def graph_inputs(self):
        """name -> the device buffer the captured step reads (None before the first step)."""
        return None if self._g_static is None else dict(zip(self._GRAPH_INPUTS, self._g_static))

    def bind_graph_inputs(self, data, combined_features):
        """Make the caller's own device tensors (fp32, contiguous) the buffers of the captured step: whatever they hold at the time of a
        `train_step` is what that step reads, nothing is copied (2.5 GB of features at the cfg3 shape).  Before the capture only."""
        if self._graph is not None:
            raise RuntimeError('the step is already captured; call compile(graph=True) again first')
        inputs, labels = data
        flat = [*inputs[:7], combined_features, *labels]
        for name, t in zip(self._GRAPH_INPUTS, flat):
            if not (isinstance(t, torch.Tensor) and t.device == self.device_ and t.dtype == torch.float32 and t.is_contiguous()):
                raise ValueError(f'{name}: bind_graph_inputs wants contiguous float32 tensors on {self.device_}')
        self._g_static = flat

    def _stage(self, data, combined_features):
        inputs, labels = data
        flat = [torch.as_tensor(x, dtype=torch.float32) for x in (*inputs[:7], combined_features, *labels)]
        if self._g_static is None:
            self._g_static = [torch.empty(t.shape, dtype=torch.float32, device=self.device_) for t in flat]
        for t, s in zip(flat, self._g_static):
            if t.shape != s.shape:
                raise ValueError(f'compile(graph=True) fixed the input shapes at the first step: got {tuple(t.shape)}, captured '
                                 f'{tuple(s.shape)}; call compile(graph=True) again for a new shape')
            if not (t.device == s.device and t.data_ptr() == s.data_ptr()):
                s.copy_(t, non_blocking=True)
        st = self._g_static
        return (tuple(st[:7]), tuple(st[8:])), st[7]

    def _train_step_graphed(self, data, combined_features):
        data_s, feats = self._stage(data, combined_features)
        if self._g_calls < 2:
            self._g_calls += 1
            side = torch.cuda.Stream(self.device_)
            side.wait_stream(torch.cuda.current_stream(self.device_))
            with torch.cuda.stream(side):
                out = self._step(data_s, feats)
            torch.cuda.current_stream(self.device_).wait_stream(side)
            return out
        if self._graph is None:
            torch.cuda.synchronize(self.device_)
            for prm in self.grasp_readout.parameters():
                prm.grad = None
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                out = self._step(data_s, feats)
            self._graph, self._g_out = graph, out
        elif self.fused_optimizer:
            self._trunk_weight_images()                  # the captured step holds the kept images: packed again in place if the trunk changed
        self._graph.replay()
        return {k: v.clone() for k, v in self._g_out.items()}
