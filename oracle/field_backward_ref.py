"""Stand-alone reference of the field backward pass (mvnerf_field_backward).  TEST INFRASTRUCTURE ONLY.

Given the stash of a training forward, the backward is a LINEAR map of the cotangent `d_rgbs` with fixed relu masks.  This
module restates that map as explicit matrix algebra in NumPy, at float64 or float32, taking activations AND masks from the
decoded stash - the kernel's real input - instead of from a twin's forward.  A float64 run is therefore a reference that
shares every relu decision with the kernel (no branch flips), so a comparison can sit at rounding level; a float32 run of
the same algebra measures what plain fp32 arithmetic costs on the same data, which is the yardstick the GPU tests scale
their bars with (tests/test_gpu_field_backward.py).

Layout of the stash (csrc/api.hip, mvnerf_stash_bytes): 7 per-view slots `x0 h1 x1 h2 x2 h3 x3` over V * n_tiles tiles, then
7 fused slots `mean h4 x4 h5 x5 h6 x6` over n_tiles tiles, every slot in tile layout [tile][128 features][32 samples] with
n_tiles = ceil(B*R*S / 32).  Per-view rows are ordered (b, v, r, s).  The per-view `x3` slot is in the layout but never written.
"""
from __future__ import annotations

import numpy as np
import torch

from . import mvnerf_oracle as O
from . import mvnerf_torch as T

VIEW_SLOTS = ('x0', 'h1', 'x1', 'h2', 'x2', 'h3', 'x3')
FUSED_SLOTS = ('mean', 'h4', 'x4', 'h5', 'x5', 'h6', 'x6')
N_HIDDEN = 128
N_IN = 379
NET_PARAMS = 247300


def stash_floats(b, v, r, s):
    tiles = (b * r * s + 31) // 32
    return (7 * v + 7) * tiles * 4096


def _tl_to_rows(slot, n_rows):
    tiles = slot.size // 4096
    return slot.reshape(tiles, N_HIDDEN, 32).transpose(0, 2, 1).reshape(tiles * 32, N_HIDDEN)[:n_rows]


def _rows_to_tl(rows, tiles, fill):
    out = np.full((tiles * 32, N_HIDDEN), fill, dtype=rows.dtype)
    out[:rows.shape[0]] = rows
    return out.reshape(tiles, 32, N_HIDDEN).transpose(0, 2, 1).reshape(-1)


def decode_stash(stash, b, v, r, s):
    """Flat stash (any float dtype, stash_floats(b, v, r, s) elements) -> {slot name: (rows, 128) row-major}.
    Per-view slots have b*v*r*s rows, fused slots b*r*s.  With one view `x3` is the fused `mean` slot (nothing writes the
    per-view one); with more views it is returned as stored."""
    stash = np.asarray(stash).reshape(-1)
    total = b * r * s
    tiles = (total + 31) // 32
    assert stash.size == stash_floats(b, v, r, s), (stash.size, stash_floats(b, v, r, s))
    assert v == 1 or (r * s) % 32 == 0, 'tiles must not straddle views'
    vslot, fslot = v * tiles * 4096, tiles * 4096
    rows = {}
    for k, name in enumerate(VIEW_SLOTS):
        rows[name] = _tl_to_rows(stash[k * vslot:(k + 1) * vslot], v * total)
    for k, name in enumerate(FUSED_SLOTS):
        rows[name] = _tl_to_rows(stash[7 * vslot + k * fslot:7 * vslot + (k + 1) * fslot], total)
    if v == 1:
        rows['x3'] = rows['mean']
    return rows


def encode_stash(rows, b, v, r, s, fill=np.nan):
    """Inverse of decode_stash on the rows a forward writes: the per-view `x3` slot and the rows past b*r*s of a ragged last
    tile hold `fill`."""
    total = b * r * s
    tiles = (total + 31) // 32
    dtype = rows['x0'].dtype
    parts = []
    for name in VIEW_SLOTS:
        src = rows[name] if name != 'x3' else np.empty((0, N_HIDDEN), dtype)
        parts.append(_rows_to_tl(np.asarray(src, dtype), v * tiles, fill))
    for name in FUSED_SLOTS:
        parts.append(_rows_to_tl(np.asarray(rows[name], dtype), tiles, fill))
    return np.concatenate(parts)


def net_sections():
    """The 28 variables of one MLP as (name, lo, hi) spans of the flat Keras-order buffer (O.unflatten_net's order)."""
    out, pos = [], 0

    def take(name, n):
        nonlocal pos
        out.append((name, pos, pos + n))
        pos += n

    take('W0', N_IN * N_HIDDEN)
    take('b0', N_HIDDEN)
    for k in range(6):
        take(f'blk{k}.W1', N_HIDDEN * N_HIDDEN)
        take(f'blk{k}.b1', N_HIDDEN)
        take(f'blk{k}.W2', N_HIDDEN * N_HIDDEN)
        take(f'blk{k}.b2', N_HIDDEN)
    take('Wr', N_HIDDEN * 4)
    take('br', 4)
    assert pos == NET_PARAMS
    return out


def field_backward_ref(net_flat, stash_rows, rgbs, d_rgbs, x_in, V, dtype=np.float64):
    """The backward of one field pass as matrix algebra at `dtype` (float64 or float32).

    net_flat: the 247 300 Keras-order variables; stash_rows: decode_stash(...); rgbs, d_rgbs: (B,R,S,4) forward output and its
    cotangent; x_in: (B*V*R*S, 379) layer-0 input, rows (b, v, r, s).
    Returns (grad (247300,), g0 (B*V*R*S, 128) = dL/d(layer-0 output), c0 = g0 W0^T (B*V*R*S, 379) = dL/d(x_in))."""
    dt = np.dtype(dtype)
    net = {k: (v if k == 'blocks' else np.asarray(v, dt)) for k, v in O.unflatten_net(np.asarray(net_flat, np.float32)).items()}
    net['blocks'] = [tuple(np.asarray(a, dt) for a in blk) for blk in net['blocks']]
    a = {k: np.asarray(v, dt) for k, v in stash_rows.items()}
    B = rgbs.shape[0]
    y = np.asarray(rgbs, dt).reshape(-1, 4)
    dy = np.asarray(d_rgbs, dt).reshape(-1, 4)
    total = y.shape[0]
    x_in = np.asarray(x_in, dt)
    assert x_in.shape == (V * total, N_IN) and a['x6'].shape == (total, N_HIDDEN)
    one = dt.type(1)

    def relu(t):
        return np.maximum(t, dt.type(0))

    # read-out: rgb = sigmoid(o[:3]), sigma = softplus(o[3]); softplus' = sigmoid(o) = 1 - exp(-softplus(o))
    d_o = np.empty_like(dy)
    d_o[:, :3] = dy[:, :3] * y[:, :3] * (one - y[:, :3])
    d_o[:, 3] = dy[:, 3] * (one - np.exp(-y[:, 3]))
    grads = {'Wr': relu(a['x6']).T @ d_o, 'br': d_o.sum(0)}
    g = (d_o @ net['Wr'].T) * (a['x6'] > 0)
    blocks = [None] * 6
    inputs = ('x0', 'x1', 'x2', 'mean', 'x4', 'x5')
    hiddens = ('h1', 'h2', 'h3', 'h4', 'h5', 'h6')
    for bi in range(5, -1, -1):
        if bi == 2 and V > 1:                               # backward of the mean over views: g / V to every view, rows (b, v, r, s)
            g = g.reshape(B, 1, total // B, N_HIDDEN) / dt.type(V)
            g = np.broadcast_to(g, (B, V, total // B, N_HIDDEN)).reshape(V * total, N_HIDDEN)
        w1, _, w2, _ = net['blocks'][bi]
        x, h = a[inputs[bi]], a[hiddens[bi]]
        dw2, db2 = relu(h).T @ g, g.sum(0)
        gh = (g @ w2.T) * (h > 0)
        dw1, db1 = relu(x).T @ gh, gh.sum(0)
        g = g + (gh @ w1.T) * (x > 0)
        blocks[bi] = (dw1, db1, dw2, db2)
    grads['W0'], grads['b0'] = x_in.T @ g, g.sum(0)
    flat = [grads['W0'].reshape(-1), grads['b0']]
    for blk in blocks:
        flat += [blk[0].reshape(-1), blk[1], blk[2].reshape(-1), blk[3]]
    flat += [grads['Wr'].reshape(-1), grads['br']]
    grad = np.concatenate(flat).astype(dt)
    assert grad.size == NET_PARAMS
    return grad, g, g @ net['W0'].T


# ---- the layer-0 input: NumPy fp32 (the oracle's op sequence) and differentiable torch (either dtype) ---------------------------
def layer0_input_f32(rays_o, rays_d, z, images, features, intrinsics, extrinsics_inv):
    """x_in (B*V*R*S, 379) = [PE(cam xyz) | PE(cam dir) | 2 rgb - 1 | features] with the NumPy oracle's fp32 arithmetic."""
    f32 = np.float32
    world = O.points_on_rays(rays_o, rays_d, z)
    pix, cam = O.compute_pixel_in_image_mv(world, intrinsics, extrinsics_inv)
    feat = O.get_projection_features_mv((images * f32(2) - f32(1)).astype(f32), features, pix)
    cdir = O.world_to_camera_direction_vector_mv(rays_d, extrinsics_inv)
    cdir = np.broadcast_to(cdir[:, :, :, None, :], cam.shape[:-1] + (3,))
    x = np.concatenate([O.position_encoding(cam[..., :3]), O.position_encoding(cdir), feat], -1)
    return x.reshape(-1, N_IN)


def layer0_input_torch(rays_o, rays_d, z, images, features, intrinsics, extrinsics_inv):
    """The same input from the differentiable twin's functions (torch tensors of one dtype) -> (x_in (B*V*R*S, 379),
    pixel coordinates (B,V,R,S,2)); gradients flow to z and features."""
    b, v, h, w, _ = images.shape
    r, s = z.shape[1:3]
    world = T.points_on_rays(rays_o, rays_d, z)
    pix, cam = T.compute_pixel_in_image_mv(world, intrinsics, extrinsics_inv)
    grid = torch.cat([images * 2.0 - 1.0, features], -1).reshape(b * v, h, w, -1)
    feat = T.interpolate_bilinear_xy(grid, pix.reshape(b * v, r * s, 2)).reshape(b, v, r, s, -1)
    cdir = T.world_to_camera_direction_vector_mv(rays_d, extrinsics_inv)[:, :, :, None, :].expand(b, v, r, s, 3)
    x = torch.cat([T.position_encoding(cam[..., :3]), T.position_encoding(cdir), feat], -1)
    return x.reshape(b * v * r * s, N_IN), pix


def input_grads(c0, rays_o, rays_d, z, images, features, intrinsics, extrinsics_inv, dtype=torch.float64):
    """d_z (B,R,S) and d_features (B,V,H,W,256) by autograd of sum(x_in(z, features) * c0) at `dtype`, plus the pixel
    coordinates (B,V,R,S,2) of that run and x_in itself (all NumPy).  c0: the cotangent of x_in, a function that makes it from
    x_in (one forward for field_backward_ref and for this), or None (forward only)."""
    def t(arr):
        return torch.as_tensor(np.asarray(arr)).to(dtype)
    zt = t(z).clone().requires_grad_(True)
    ft = t(features).clone().requires_grad_(True)
    x, pix = layer0_input_torch(t(rays_o), t(rays_d), zt, t(images), ft, t(intrinsics), t(extrinsics_inv))
    if c0 is None:
        return None, None, pix.detach().numpy(), x.detach().numpy()
    if callable(c0):
        c0 = c0(x.detach().numpy())
    (x * t(c0)).sum().backward()
    return zt.grad.numpy(), ft.grad.numpy(), pix.detach().numpy(), x.detach().numpy()
