"""Reference of the trunk's query map (points, dirs) -> (view mean, u1, u2, u3) with every decision frozen.  TEST INFRASTRUCTURE ONLY.

The map the query kernels differentiate (mvnerf_query_jvp, mvnerf_query_vjp; oracle/mvnerf_torch.query_acts is its free-running
twin) is piecewise smooth: its pieces are cut by
  * the relu of 12 hidden layers - six pre-activations per view (x0 h1 x1 h2 x2 h3) and six fused ones (mean h4 x4 h5 x5 h6),
  * the bilinear cell (x0, y0) of every (view, point),
  * the pass flags of the clamps, per coordinate: ux in [0, 1] and |pxr| <= 1e6 (one flag, `pass`: the kernels test both in one
    condition, query_ops.hip / train_ops.hip field_dz_kernel), and q2 >= 1e-8.
This module takes all of them as DATA: the relu masks from a decoded stash (oracle/field_backward_ref.decode_stash with S = 1) or
from a forward of its own, the cell and the flags from the NumPy fp32 oracle's geometry chain, which tests/test_gpu_parity.py
holds bit-equal to the kernels' pixel coordinates and taps.  With the decisions frozen the map is smooth (affine layers between
fixed masks, sin / cos, one division), so a float64 run shares every branch with the kernel and a comparison can sit at
rounding level; a float32 run of the SAME algebra measures what plain fp32 arithmetic costs on the same data - the yardstick the
GPU tests scale their bars with (tests/test_gpu_query_grade.py).

Frozen algebra at `dtype`:
    cam = E [p; 1], q = K cam, den = q2 where q2 >= 1e-8 else the constant fl32(1e-8)
    pxr = q0 / den ; ax = pxr - x0 where `pass_x` else the constant the fp32 chain produced (0 or 1) ; same for y
    feat = ay (bot - top) + top, top = ax (tr - tl) + tl, bot = ax (br - bl) + bl        (tfa interpolate_bilinear's form)
    x_in = [PE(cam xyz) | PE(E [d; 1]) | feat], PE argument = coordinate * fl32(pi 2^k) formed at `dtype`
    layer: relu(x) is x * mask.

`mutant=` plants one of the errors of MUTANTS into the derivative (the value of the map never changes): what a wrong kernel would
compute, for tests/test_query_ref.py to show that the GPU test's bar rejects it.
"""
from __future__ import annotations

import numpy as np
import torch

from . import mvnerf_oracle as O
from . import mvnerf_torch as T
from .field_backward_ref import FUSED_SLOTS, N_HIDDEN, VIEW_SLOTS

F32 = np.float32
VIEW_MASKS = VIEW_SLOTS[:6]            # x0 h1 x1 h2 x2 h3: the relu inputs of the three per-view blocks
FUSED_MASKS = FUSED_SLOTS[:6]          # mean h4 x4 h5 x5 h6
DELTA = 2e-5                           # the project's primal-agreement bar (tests/test_gpu_query.py), relative to max(1, max |slot|)

# name -> which product shows it ('jvp', 'vjp' or 'both')
MUTANTS = {
    'rgb_tangent_dropped': 'both',
    'y_lerp_tangent_dropped': 'both',
    'pxr_tq2_dropped': 'both',
    'clamp_open_outside_image': 'both',
    'clamp_open_behind_camera': 'both',
    'view_mean_scaled': 'both',
    'top_octave_tangent_dropped': 'both',
    'cos_derivative_sign': 'both',
    'dir_tangent_gets_translation': 'jvp',
    'inv_v_twice': 'both',
    'd_dirs_missing_view': 'both',
}


def _only_value(x):
    return x.detach()


def _negated_tangent(x):
    return 2.0 * x.detach() - x


class QueryRef:
    """One set of query points in one scene: the frozen decisions of the geometry, and the map at any dtype."""

    def __init__(self, net_flat, images, features, intrinsics, extrinsics_inv, points, dirs):
        self.net_flat = np.asarray(net_flat, F32)
        self.images, self.features = np.asarray(images, F32), np.asarray(features, F32)
        self.k4, self.einv = np.asarray(intrinsics, F32), np.asarray(extrinsics_inv, F32)
        self.points, self.dirs = np.asarray(points, F32), np.asarray(dirs, F32)
        self.B, self.V, self.H, self.W, _ = self.images.shape
        self.N = self.points.shape[1]
        assert self.points.shape == self.dirs.shape == (self.B, self.N, 3)
        # the fp32 geometry chain, operation for operation what query_ops.hip:116-129 and pixel_from_cam / bilinear_taps do
        p = self.points[:, None]
        e, k = self.einv[:, :, None], self.k4[:, :, None]
        c = O._matvec4(e, p[..., 0], p[..., 1], p[..., 2], F32(1.0))
        q = O._matvec4(k, c[0], c[1], c[2], c[3])
        den = np.maximum(q[2], F32(1e-8))
        raw = np.stack([(q[0] / den).astype(F32), (q[1] / den).astype(F32)], -1)                 # (B,V,N,2)
        pix = np.clip(raw, F32(-1e6), F32(1e6))
        x0, y0, ax, ay = O.bilinear_taps(pix, self.H, self.W)
        cell = np.stack([x0, y0], -1)
        u = (pix - cell.astype(F32)).astype(F32)                                                # unclamped lerp factors
        self.cell = cell.astype(np.int64)
        self.alpha32 = np.stack([ax, ay], -1)
        self.pass_clip = (raw >= F32(-1e6)) & (raw <= F32(1e6))
        self.pass_xy = (u >= 0) & (u <= 1) & self.pass_clip
        self.pass_q2 = q[2] >= F32(1e-8)
        self.raw32, self.q2_32 = raw, q[2]
        # the fp32 arguments of the two positional encodings (O.position_encoding: coordinate * fl32(pi 2^k), one rounding)
        freq = (F32(np.pi) * np.power(F32(2.0), np.arange(T.N_FREQ, dtype=F32))).astype(F32)
        cdir = O.world_to_camera_direction_vector_mv(self.dirs, self.einv)
        self.arg32_xyz = (np.stack(c[:3], -1)[..., None] * freq).astype(F32)                    # (B,V,N,3,10)
        self.arg32_dir = (cdir[..., None] * freq).astype(F32)

    # ---- shares of the decisions, for the tests' conditions on their inputs ------------------------------------------------
    def outside_image(self):
        """(B,V,N): either coordinate's clamp closed."""
        return ~self.pass_xy.all(-1)

    def behind_or_clipped(self):
        """(B,V,N): behind the camera (q2 < 1e-8) or at the +-1e6 clip."""
        return ~self.pass_q2 | (np.abs(self.raw32) > F32(1e6)).any(-1)

    # ---- masks -------------------------------------------------------------------------------------------------------------
    def masks_from_rows(self, rows):
        """{slot: (rows, 128)} as decode_stash(stash, B, V, N, 1) gives it (or self.rows(dtype)) -> boolean relu masks."""
        m = {}
        for name in VIEW_MASKS:
            m[name] = torch.as_tensor(np.asarray(rows[name]) > 0).reshape(self.B, self.V, self.N, N_HIDDEN)
        for name in FUSED_MASKS:
            m[name] = torch.as_tensor(np.asarray(rows[name]) > 0).reshape(self.B, self.N, N_HIDDEN)
        return m

    def near_zero_points(self, rows, delta=DELTA):
        """(B,N) bool: points with a pre-activation of any of the 12 relu inputs within delta * max(1, max |slot|) of zero - where
        two forwards that agree to the project's primal bar may still take different relu branches."""
        out = np.zeros((self.B, self.N), bool)
        for name in VIEW_MASKS + FUSED_MASKS:
            a = np.asarray(rows[name], np.float64)
            near = (np.abs(a) <= delta * max(1.0, float(np.abs(a).max()))).any(-1)
            out |= near.reshape(self.B, self.V, self.N).any(1) if name in VIEW_MASKS else near.reshape(self.B, self.N)
        return out

    # ---- the map -----------------------------------------------------------------------------------------------------------
    def _fn(self, dtype, masks, mutant=None, gather=True, record=None, at_arg32=False, eps=1e-3):
        """f(points, dirs, w) -> (4,B,N,128) at `dtype`; w is the homogeneous coordinate of the direction (Q3: the constant 1).
        masks None: free-running relu.  record: dict that receives the pre-activations (detached NumPy, stash row order).
        at_arg32: sin / cos are taken AT the fp32-rounded arguments of the fp32 chain (exact constants at any dtype) while the
        argument's tangent stays d(coordinate) * fl32(pi 2^k) - see the module docstring.  eps: size of 'view_mean_scaled'."""
        assert mutant is None or mutant in MUTANTS, mutant
        B, V, N, H, W = self.B, self.V, self.N, self.H, self.W

        def t(a):
            return torch.as_tensor(np.asarray(a)).to(dtype)
        net = T.unflatten_net(t(self.net_flat))
        E, K = t(self.einv)[:, :, None], t(self.k4)[:, :, None]                                  # (B,V,1,4,4)
        grid = torch.cat([t(self.images) * 2.0 - 1.0, t(self.features)], -1).reshape(B * V * H * W, -1)
        base = torch.arange(B * V).reshape(B, V, 1) * (H * W) + torch.as_tensor(self.cell[..., 1] * W + self.cell[..., 0])
        tl, tr, bl, br = grid[base], grid[base + 1], grid[base + W], grid[base + W + 1]          # (B,V,N,259)
        cell = t(self.cell)
        alpha32 = t(self.alpha32)
        pass_xy, pass_q2, pass_clip = torch.as_tensor(self.pass_xy), torch.as_tensor(self.pass_q2), torch.as_tensor(self.pass_clip)
        den_const = torch.tensor(float(F32(1e-8)), dtype=dtype)
        freq = t(F32(np.pi)) * (2.0 ** torch.arange(T.N_FREQ, dtype=dtype))

        def pe(pos, drop_top, arg32):
            arg = pos[..., None] * freq
            if at_arg32:
                arg = t(arg32) + (arg - _only_value(arg))
            if drop_top:
                arg = torch.cat([arg[..., :-1], _only_value(arg[..., -1:])], -1)
            c = torch.cos(arg)
            if mutant == 'cos_derivative_sign':
                c = _negated_tangent(c)
            return torch.stack([torch.sin(arg), c], -1).reshape(*pos.shape[:-1], -1)

        def relu(x, name):
            if record is not None:
                record[name] = x.detach().numpy().reshape(-1, N_HIDDEN)
            return x * (masks[name].to(dtype) if masks is not None else (x > 0).to(dtype))

        def block(x, blk, name_x, name_h):
            w1, b1, w2, b2 = blk
            r = relu(x, name_x) @ w1 + b1
            return x + (relu(r, name_h) @ w2 + b2)

        def f(points, dirs, w):
            p = points[:, None]                                                                  # (B,1,N,3)
            cam = [((E[..., r, 0] * p[..., 0] + E[..., r, 1] * p[..., 1]) + E[..., r, 2] * p[..., 2]) + E[..., r, 3] for r in range(4)]
            q = [((K[..., r, 0] * cam[0] + K[..., r, 1] * cam[1]) + K[..., r, 2] * cam[2]) + K[..., r, 3] * cam[3] for r in range(3)]
            closed = den_const + (q[2] - _only_value(q[2])) if mutant == 'clamp_open_behind_camera' else den_const
            den = torch.where(pass_q2, q[2], closed)
            if mutant == 'pxr_tq2_dropped':
                den = _only_value(den)
            a = torch.stack([q[0] / den, q[1] / den], -1) - cell
            closed = alpha32
            if mutant == 'clamp_open_outside_image':                 # the [0, 1] clamp of the lerp factor, inside the +-1e6 clip
                closed = torch.where(pass_clip, alpha32 + (a - _only_value(a)), alpha32)
            if mutant == 'clamp_open_behind_camera':                 # the +-1e6 clip, where points behind the camera end up
                closed = torch.where(pass_clip, alpha32, alpha32 + (a - _only_value(a)))
            a = torch.where(pass_xy, a, closed)
            ax, ay = a[..., 0:1], a[..., 1:2]
            if mutant == 'y_lerp_tangent_dropped':
                ay = _only_value(ay)
            top = ax * (tr - tl) + tl
            bot = ax * (br - bl) + bl
            feat = ay * (bot - top) + top
            if mutant == 'rgb_tangent_dropped':
                feat = torch.cat([_only_value(feat[..., :3]), feat[..., 3:]], -1)
            if not gather:
                feat = _only_value(feat)
            d = dirs[:, None]
            if mutant == 'd_dirs_missing_view':
                d = torch.cat([d.expand(B, V, N, 3)[:, :-1], _only_value(d)], 1)
            cdir = torch.stack([((E[..., r, 0] * d[..., 0] + E[..., r, 1] * d[..., 1]) + E[..., r, 2] * d[..., 2]) + E[..., r, 3] * w
                                for r in range(3)], -1)
            x_in = torch.cat([pe(torch.stack(cam[:3], -1), mutant == 'top_octave_tangent_dropped', self.arg32_xyz),
                              pe(cdir, False, self.arg32_dir), feat], -1)
            if record is not None:
                record['x_in'] = x_in.detach().numpy().reshape(-1, x_in.shape[-1])
            x = x_in @ net['W0'] + net['b0']                                                     # (B,V,N,128)
            for bi in range(3):
                x = block(x, net['blocks'][bi], VIEW_MASKS[2 * bi], VIEW_MASKS[2 * bi + 1])
            if mutant == 'inv_v_twice':
                x = _only_value(x) * (1.0 - 1.0 / V) + x / V
            x = x.sum(1) / V
            if mutant == 'view_mean_scaled':
                x = x * (1.0 + eps)
            outs = [x]
            for bi in range(3, 6):
                outs.append(block(outs[-1], net['blocks'][bi], FUSED_MASKS[2 * (bi - 3)], FUSED_MASKS[2 * (bi - 3) + 1]))
            if record is not None:
                record['x6'] = outs[-1].detach().numpy().reshape(-1, N_HIDDEN)
            return torch.stack(outs, 0)
        return f, t

    def forward(self, dtype=torch.float64, masks=None):
        """-> (acts (4,B,N,128), x_in (B*V*N, 379) the layer-0 input, rows (b, v, n)), NumPy at `dtype`."""
        rec = {}
        f, t = self._fn(dtype, masks, record=rec)
        with torch.no_grad():
            acts = f(t(self.points), t(self.dirs), torch.ones((), dtype=dtype))
        return acts.numpy(), rec['x_in']

    def rows(self, dtype=torch.float32):
        """Pre-activations of a free-running forward at `dtype` on the frozen geometry, named and ordered as decode_stash's."""
        rec = {}
        f, t = self._fn(dtype, None, record=rec)
        with torch.no_grad():
            f(t(self.points), t(self.dirs), torch.ones((), dtype=dtype))
        rec.pop('x_in')
        return rec

    def jvp(self, t_points, t_dirs, masks, dtype=torch.float64, mutant=None, gather=True, **kw):
        """J [t_points; t_dirs] -> (4,B,N,128) float64 NumPy (computed at `dtype`)."""
        f, t = self._fn(dtype, masks, mutant, gather, **kw)
        t_w = 1.0 if mutant == 'dir_tangent_gets_translation' else 0.0
        _, out = torch.autograd.functional.jvp(f, (t(self.points), t(self.dirs), torch.ones((), dtype=dtype)),
                                               (t(t_points), t(t_dirs), torch.full((), t_w, dtype=dtype)))
        return out.numpy().astype(np.float64)

    def vjp(self, g_acts, masks, dtype=torch.float64, mutant=None, gather=True, **kw):
        """J^T g_acts -> (d_points, d_dirs), each (B,N,3) float64 NumPy (computed at `dtype`)."""
        f, t = self._fn(dtype, masks, mutant, gather, **kw)
        one = torch.ones((), dtype=dtype)
        _, (dp, dd) = torch.autograd.functional.vjp(lambda p, d: f(p, d, one), (t(self.points), t(self.dirs)), t(g_acts))
        return dp.numpy().astype(np.float64), dd.numpy().astype(np.float64)


# ---- the measures of the GPU test's bar ----------------------------------------------------------------------------------------
def errors(got, ref, keep=None):
    """(tensor-relative L2, maximum over points of the per-point relative error) of got against ref; the last axis is the point's
    vector, keep (bool over the leading axes) selects the points."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    if keep is not None:
        got, ref = got[keep], ref[keep]
    got, ref = got.reshape(-1, ref.shape[-1]), ref.reshape(-1, ref.shape[-1])
    l2 = np.linalg.norm(got - ref) / max(np.linalg.norm(ref), 1e-300)
    rows = np.linalg.norm(got - ref, axis=-1) / np.maximum(np.linalg.norm(ref, axis=-1), 1e-300)
    return float(l2), float(rows.max())
