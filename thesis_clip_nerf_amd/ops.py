"""Torch-tensor front end of the C ABI (include/mvnerf_hip.h).

PyTorch is used only for device memory and streams: every function checks device / dtype /
contiguity, allocates outputs with ``torch.empty`` and passes raw pointers plus the current HIP
stream to libmvnerf_hip.so.  Shape errors raise ``ValueError`` (like the reference's TensorSpec
mismatches), HIP failures ``RuntimeError``.
"""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from . import _lib
from ._lib import F16X3_MAX_ACT, F16X3_MAX_WEIGHT, NET_PARAMS, Q7_CLAMP, Q7_ZERO  # noqa: F401


def _chk(t, name, dtype=torch.float32, shape=None):
    if not isinstance(t, torch.Tensor):
        raise ValueError(f'{name}: expected a torch.Tensor, got {type(t).__name__}')
    if not t.is_cuda:
        raise ValueError(f'{name}: must live on a HIP device (got {t.device}); there is no CPU path')
    if t.dtype != dtype:
        raise ValueError(f'{name}: dtype {t.dtype}, expected {dtype}')
    if not t.is_contiguous():
        raise ValueError(f'{name}: must be contiguous')
    if shape is not None:
        if len(shape) != t.dim() or any(s is not None and s != d for s, d in zip(shape, t.shape)):
            raise ValueError(f'{name}: shape {tuple(t.shape)}, expected {tuple(shape)}')
    return t


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _stream(t):
    return ctypes.c_void_p(torch.cuda.current_stream(t.device).cuda_stream)


def _scene(images, features, intrinsics, extrinsics_inv, b=None, features_dtype=torch.float32):
    """The source views of a field pass: images (B,V,H,W,3), features (B,V,H,W,256), intrinsics and extrinsics_inv (B,V,4,4)
    -> (b, v, h, w).  b: the batch size the caller's rays or points have already fixed."""
    _chk(images, 'images', shape=(b, None, None, None, 3))
    b, v, h, w, _ = images.shape
    _chk(features, 'features', dtype=features_dtype, shape=(b, v, h, w, 256))
    _chk(intrinsics, 'intrinsics', shape=(b, v, 4, 4))
    _chk(extrinsics_inv, 'extrinsics_inv', shape=(b, v, 4, 4))
    return b, v, h, w


def packed_net_floats():
    return int(_lib.lib().mvnerf_packed_net_floats())


def pack_net(net_keras):
    """Keras-order flat MLP (247 300 floats) -> MFMA operand image (mvnerf_pack_net)."""
    _chk(net_keras, 'net_keras', shape=(NET_PARAMS,))
    out = torch.empty(packed_net_floats(), dtype=torch.float32, device=net_keras.device)
    with torch.cuda.device(net_keras.device):
        _lib.check(_lib.lib().mvnerf_pack_net(_p(net_keras), _p(out), _stream(net_keras)), 'pack_net')
    return out


def get_rays_device(m3x3, origin, device, u=None, v=None, width=0, height=0, normalize=True, return_f64=False):
    """mvnerf_get_rays.  m3x3 = E[:3,:3] @ inv(K[:3,:3]) and origin = E[:3,3] are host float64."""
    m = np.ascontiguousarray(m3x3, dtype=np.float64).reshape(9)
    o = np.ascontiguousarray(origin, dtype=np.float64).reshape(3)
    if u is None:
        n = int(width) * int(height)
    else:
        _chk(u, 'u')
        _chk(v, 'v', shape=tuple(u.shape))
        n = u.numel()
    device = torch.device(device)
    rays_o = torch.empty((n, 3), dtype=torch.float32, device=device)
    rays_d = torch.empty((n, 3), dtype=torch.float32, device=device)
    d64 = torch.empty((n, 3), dtype=torch.float64, device=device) if return_f64 else None
    with torch.cuda.device(device):
        rc = _lib.lib().mvnerf_get_rays(m.ctypes.data_as(ctypes.c_void_p), o.ctypes.data_as(ctypes.c_void_p), _p(u),
                                        _p(v), n, int(width), int(bool(normalize)), _p(rays_o), _p(rays_d), _p(d64),
                                        _stream(rays_o))
    _lib.check(rc, 'get_rays')
    return (rays_o, rays_d, d64) if return_f64 else (rays_o, rays_d)


def stratified_depths(u, near, far):
    """u (..., S) uniforms -> z (..., S) (mvnerf_stratified_depths)."""
    _chk(u, 'u')
    s = u.shape[-1]
    z = torch.empty_like(u)
    with torch.cuda.device(u.device):
        rc = _lib.lib().mvnerf_stratified_depths(_p(u), u.numel() // s, s, float(near), float(far), _p(z), _stream(u))
    _lib.check(rc, 'stratified_depths')
    return z


def texel_table_pays(n_rays_per_scene, n_samples, h, w):
    """Host-side rule for building a texel table for ONE field pass: the table costs H*W rows of the 256->128
    product per view, the direct form R*S rows; the factor 2 covers the table's own launch and traffic."""
    return n_rays_per_scene * n_samples >= 2 * h * w


def _auto_texel_tables(texel_tables, bvhw, n_rays_per_scene, n_samples, device):
    """The texel_tables argument of the render_fwd* functions: 'auto' -> a (2,B,V,H,W,128) tensor to build when
    texel_table_pays(), else None; None or a tensor is handed back."""
    if not isinstance(texel_tables, str):
        return texel_tables
    if texel_tables != 'auto':
        raise ValueError(f"texel_tables: {texel_tables!r}, expected None, 'auto' or a tensor")
    if not texel_table_pays(n_rays_per_scene, n_samples, bvhw[2], bvhw[3]):
        return None
    return torch.empty((2,) + tuple(bvhw) + (128,), dtype=torch.float32, device=device)


def project_texels(features, packed_net, out=None):
    """mvnerf_project_texels: features (B,V,H,W,256), one net's packed image -> table (B,V,H,W,128)
    (W0[123:379]^T features per texel, accumulator order) for field_eval(..., texel_table=table)."""
    _chk(features, 'features', shape=(None, None, None, None, 256))
    b, v, h, w, _ = features.shape
    _chk(packed_net, 'packed_net', shape=(packed_net_floats(),))
    if out is None:
        out = torch.empty((b, v, h, w, 128), dtype=torch.float32, device=features.device)
    else:
        _chk(out, 'texel_table', shape=(b, v, h, w, 128))
    with torch.cuda.device(features.device):
        rc = _lib.lib().mvnerf_project_texels(_p(features), _p(packed_net), b, v, h, w, _p(out), _stream(features))
    _lib.check(rc, 'project_texels')
    return out


def project_texels2(features, packed_a, packed_b, out=None):
    """mvnerf_project_texels2: both nets' tables (2,B,V,H,W,128) [a | b] from one read of the feature maps."""
    _chk(features, 'features', shape=(None, None, None, None, 256))
    b, v, h, w, _ = features.shape
    _chk(packed_a, 'packed_a', shape=(packed_net_floats(),))
    _chk(packed_b, 'packed_b', shape=(packed_net_floats(),))
    if out is None:
        out = torch.empty((2, b, v, h, w, 128), dtype=torch.float32, device=features.device)
    else:
        _chk(out, 'texel_tables', shape=(2, b, v, h, w, 128))
    with torch.cuda.device(features.device):
        rc = _lib.lib().mvnerf_project_texels2(_p(features), _p(packed_a), _p(packed_b), b, v, h, w, _p(out[0]), _p(out[1]),
                                               _stream(features))
    _lib.check(rc, 'project_texels2')
    return out


def _field_pass(what, fn, rays_o, rays_d, z, scene, packed_net, second=None, texel_table=None, table_arg=True, wide=True,
                features_dtype=torch.float32, return_taps=False, return_pix=False, return_embedding=False, complete_output=False,
                return_fused_acts=False, extra=()):
    """The checks, output allocation, C call and result tuple of field_eval / field_eval_split / field_eval_bf16.
    fn: the entry point; second: (tensor, name, bytes) of the weight stream it takes behind packed_net; table_arg: it takes a
    texel_table; wide: it has the pix and per-view outputs (the bf16 entry points do not); extra: what an _ex entry point takes
    in front of the stream."""
    _chk(rays_o, 'rays_o', shape=(None, None, 3))
    b, r, _ = rays_o.shape
    _chk(rays_d, 'rays_d', shape=(b, r, 3))
    _chk(z, 'z', shape=(b, r, None))
    s = z.shape[2]
    _, v, h, w = _scene(*scene, b=b, features_dtype=features_dtype)
    _chk(packed_net, 'packed_net', shape=(packed_net_floats(),))
    if second is not None:
        _chk(second[0], second[1], dtype=torch.uint8, shape=(second[2],))
    if texel_table is not None:
        _chk(texel_table, 'texel_table', shape=(b, v, h, w, 128))
    dev = rays_o.device
    rgbs = torch.empty((b, r, s, 4), dtype=torch.float32, device=dev)
    taps = torch.empty((b, v, r, s, 4), dtype=torch.int32, device=dev) if return_taps else None
    pix = torch.empty((b, v, r, s, 2), dtype=torch.float32, device=dev) if return_pix else None
    emb = torch.empty((b, r, s, 128), dtype=torch.float32, device=dev) if return_embedding else None
    acts_v = torch.empty((4, b * v, r, s, 128), dtype=torch.float32, device=dev) if complete_output else None
    acts_f = torch.empty((4, b, r, s, 128), dtype=torch.float32, device=dev) if complete_output or return_fused_acts else None
    ws = torch.empty(int(_lib.lib().mvnerf_field_workspace_bytes(b, v, r)), dtype=torch.uint8, device=dev)
    ins = [rays_o, rays_d, z, scene[0], scene[1]] + ([texel_table] if table_arg else []) + [scene[2], scene[3], packed_net]
    outs = [rgbs, taps, pix, emb, acts_v, acts_f] if wide else [rgbs, taps, emb, acts_f]
    with torch.cuda.device(dev):
        rc = fn(*map(_p, ins + ([] if second is None else [second[0]])), b, v, r, s, h, w, *map(_p, outs + [ws]), *extra, _stream(rays_o))
    _lib.check(rc, what)
    out = (rgbs,)
    if return_taps:
        out += (taps,)
    if return_pix:
        out += (pix,)
    if return_embedding:
        out += (emb,)
    if complete_output:               # the reference's `outputs` list (layers.py:364-377): 4 per-view + 4 fused
        out += (list(acts_v.unbind(0)) + list(acts_f.unbind(0)),)
    if return_fused_acts:
        out += (acts_f,)
    return out if len(out) > 1 else rgbs


def field_eval(rays_o, rays_d, z, images, features, intrinsics, extrinsics_inv, packed_net, return_taps=False,
               return_pix=False, return_embedding=False, complete_output=False, texel_table=None):
    """mvnerf_field_eval: -> rgbs (B,R,S,4) [+ tap_idx (B,V,R,S,4) int32] [+ pix (B,V,R,S,2)] [+ embedding (B,R,S,128)].
    texel_table: project_texels(features, packed_net) of the SAME net -> mvnerf_field_eval_table."""
    fn = _lib.lib().mvnerf_field_eval if texel_table is None else _lib.lib().mvnerf_field_eval_table
    return _field_pass('field_eval', fn, rays_o, rays_d, z, (images, features, intrinsics, extrinsics_inv), packed_net,
                       texel_table=texel_table, table_arg=texel_table is not None, return_taps=return_taps, return_pix=return_pix,
                       return_embedding=return_embedding, complete_output=complete_output)


def query_field(points, dirs, images, features, intrinsics, extrinsics_inv, packed_net, complete_output=False):
    """Trunk as a field on arbitrary points (lmvnerf/model_v4.py:217-262 use of fine_embedding):
    points, dirs (B,N,3) -> rgbs (B,N,4) and either the embedding (B,N,128) or, with complete_output, the
    list of 8 activations [x0,f1,f2,f3 (B*V,N,128) | mean,u1,u2,u3 (B,N,128)]."""
    _chk(points, 'points', shape=(None, None, 3))
    z = torch.zeros(tuple(points.shape[:2]) + (1,), dtype=torch.float32, device=points.device)   # p = o + 0*d = o
    res = field_eval(points, dirs, z, images, features, intrinsics, extrinsics_inv, packed_net,
                     return_embedding=not complete_output, complete_output=complete_output)
    rgbs, extra = res[0], res[1]
    if complete_output:
        return rgbs[:, :, 0], [a[:, :, 0] for a in extra]
    return rgbs[:, :, 0], extra[:, :, 0]


def composite(z, rgbs, return_weights=True):
    """mvnerf_composite: z (...,S), rgbs (...,S,4) -> rgb (...,3), depth (...), weights (...,S)."""
    _chk(z, 'z')
    s = z.shape[-1]
    _chk(rgbs, 'rgbs', shape=tuple(z.shape) + (4,))
    lead = tuple(z.shape[:-1])
    n = z.numel() // s
    rgb = torch.empty(lead + (3,), dtype=torch.float32, device=z.device)
    depth = torch.empty(lead, dtype=torch.float32, device=z.device)
    weights = torch.empty_like(z) if return_weights else None
    with torch.cuda.device(z.device):
        rc = _lib.lib().mvnerf_composite(_p(z), _p(rgbs), n, s, _p(rgb), _p(depth), _p(weights), _stream(z))
    _lib.check(rc, 'composite')
    return rgb, depth, weights


def resample(z, weights, u_fine, q7_mode=Q7_ZERO, return_aux=False, return_rank=False):
    """mvnerf_resample: -> z_all (...,2S) [+ z_fine, above, below] [+ fine_rank]."""
    _chk(z, 'z')
    s = z.shape[-1]
    _chk(weights, 'weights', shape=tuple(z.shape))
    _chk(u_fine, 'u_fine', shape=tuple(z.shape))
    n = z.numel() // s
    z_all = torch.empty(tuple(z.shape[:-1]) + (2 * s,), dtype=torch.float32, device=z.device)
    z_fine = torch.empty_like(z) if return_aux else None
    above = torch.empty(z.shape, dtype=torch.int32, device=z.device) if return_aux else None
    below = torch.empty(z.shape, dtype=torch.int32, device=z.device) if return_aux else None
    rank = torch.empty(z.shape, dtype=torch.int32, device=z.device) if return_rank else None
    with torch.cuda.device(z.device):
        rc = _lib.lib().mvnerf_resample(_p(z), _p(weights), _p(u_fine), n, s, int(q7_mode), _p(z_all), _p(z_fine),
                                        _p(above), _p(below), _p(rank), _stream(z))
    _lib.check(rc, 'resample')
    out = (z_all, z_fine, above, below) if return_aux else (z_all,)
    if return_rank:
        out += (rank,)
    return out if len(out) > 1 else z_all


def resample_bwd(z, weights, u_fine, fine_rank, d_z_all, q7_mode=Q7_ZERO):
    """Backward of resample w.r.t. the coarse weights: -> d_weights (..., S)."""
    _chk(z, 'z')
    s = z.shape[-1]
    _chk(weights, 'weights', shape=tuple(z.shape))
    _chk(u_fine, 'u_fine', shape=tuple(z.shape))
    _chk(fine_rank, 'fine_rank', dtype=torch.int32, shape=tuple(z.shape))
    _chk(d_z_all, 'd_z_all', shape=tuple(z.shape[:-1]) + (2 * s,))
    out = torch.empty_like(z)
    with torch.cuda.device(z.device):
        rc = _lib.lib().mvnerf_resample_bwd(_p(z), _p(weights), _p(u_fine), _p(fine_rank), _p(d_z_all), z.numel() // s, s,
                                            int(q7_mode), _p(out), _stream(z))
    _lib.check(rc, 'resample_bwd')
    return out


def render_workspace_bytes(b, v, r, s):
    return int(_lib.lib().mvnerf_render_workspace_bytes(int(b), int(v), int(r), int(s)))


def render_fwd(rays_o, rays_d, images, features, intrinsics, extrinsics_inv, packed_coarse, packed_fine, u_coarse,
               u_fine, near, far, q7_mode=Q7_ZERO, workspace=None, out=None, texel_tables=None, tables_ready=False, split=None,
               kernel=None, range_status=None):
    """mvnerf_render_fwd = MVVNeRFRenderer._call (model_v0.py:113-184) -> (rgb, depth, fine_rgb, fine_depth).
    split: (pack_net_split(coarse), pack_net_split(fine)) -> mvnerf_render_fwd_split (fp32-grade Dense layers on the bf16 MFMA).
    kernel, range_status (split path only): see field_eval_split; range_status here is TWO floats (coarse pass, fine pass).
    texel_tables: None = gather raw features; 'auto' = allocate and build when texel_table_pays(); or a float32
    tensor (2,B,V,H,W,128) [coarse net | fine net], built by this call unless tables_ready."""
    _chk(rays_o, 'rays_o', shape=(None, None, 3))
    b, r, _ = rays_o.shape
    _chk(rays_d, 'rays_d', shape=(b, r, 3))
    _, v, h, w = _scene(images, features, intrinsics, extrinsics_inv, b=b)
    _chk(u_coarse, 'u_coarse', shape=(b, r, None))
    s = u_coarse.shape[2]
    _chk(u_fine, 'u_fine', shape=(b, r, s))
    _chk(packed_coarse, 'packed_coarse', shape=(packed_net_floats(),))
    _chk(packed_fine, 'packed_fine', shape=(packed_net_floats(),))
    dev = rays_o.device
    need = render_workspace_bytes(b, v, r, s)
    if workspace is None:
        workspace = torch.empty(need, dtype=torch.uint8, device=dev)
    else:
        _chk(workspace, 'workspace', dtype=torch.uint8)
        if workspace.numel() < need:
            raise ValueError(f'workspace: {workspace.numel()} bytes, need {need}')
    if out is None:
        out = (torch.empty((b, r, 3), dtype=torch.float32, device=dev), torch.empty((b, r), dtype=torch.float32, device=dev),
               torch.empty((b, r, 3), dtype=torch.float32, device=dev), torch.empty((b, r), dtype=torch.float32, device=dev))
    rgb, depth, fine_rgb, fine_depth = out
    if isinstance(texel_tables, str):
        tables_ready = False
    texel_tables = _auto_texel_tables(texel_tables, (b, v, h, w), r, s, dev)
    if texel_tables is not None:
        _chk(texel_tables, 'texel_tables', shape=(2, b, v, h, w, 128))
    with torch.cuda.device(dev):
        if split is None:
            if kernel is not None or range_status is not None:
                raise ValueError('kernel / range_status belong to the split path: pass split=')
            rc = _lib.lib().mvnerf_render_fwd(_p(rays_o), _p(rays_d), _p(images), _p(features), _p(intrinsics),
                                              _p(extrinsics_inv), _p(packed_coarse), _p(packed_fine), _p(u_coarse),
                                              _p(u_fine), b, v, r, s, h, w, float(near), float(far), int(q7_mode), _p(rgb),
                                              _p(depth), _p(fine_rgb), _p(fine_depth), _p(workspace), _p(texel_tables),
                                              int(bool(tables_ready)), _stream(rays_o))
        else:
            nbytes = int(_lib.lib().mvnerf_packed_net_split_bytes())
            _chk(split[0], 'split_coarse', dtype=torch.uint8, shape=(nbytes,))
            _chk(split[1], 'split_fine', dtype=torch.uint8, shape=(nbytes,))
            ex = _split_ex_args(kernel, range_status, 2)
            if ex is not None:
                rc = _lib.lib().mvnerf_render_fwd_split_ex(_p(rays_o), _p(rays_d), _p(images), _p(features), _p(intrinsics),
                                                           _p(extrinsics_inv), _p(packed_coarse), _p(packed_fine), _p(split[0]), _p(split[1]),
                                                           _p(u_coarse), _p(u_fine), b, v, r, s, h, w, float(near), float(far),
                                                           int(q7_mode), _p(rgb), _p(depth), _p(fine_rgb), _p(fine_depth), _p(workspace),
                                                           _p(texel_tables), int(bool(tables_ready)), *ex, _stream(rays_o))
                _lib.check(rc, 'render_fwd')
                return rgb, depth, fine_rgb, fine_depth
            rc = _lib.lib().mvnerf_render_fwd_split(_p(rays_o), _p(rays_d), _p(images), _p(features), _p(intrinsics),
                                                    _p(extrinsics_inv), _p(packed_coarse), _p(packed_fine), _p(split[0]), _p(split[1]),
                                                    _p(u_coarse), _p(u_fine), b, v, r, s, h, w, float(near), float(far),
                                                    int(q7_mode), _p(rgb), _p(depth), _p(fine_rgb), _p(fine_depth), _p(workspace),
                                                    _p(texel_tables), int(bool(tables_ready)), _stream(rays_o))
    _lib.check(rc, 'render_fwd')
    return rgb, depth, fine_rgb, fine_depth


# ---- op-level (unfused) operators: one per reference function ---------------------------------------
def points_on_rays(rays_o, rays_d, z):
    """o + z*d: rays (...,3), z (...,S) -> (...,S,3)."""
    _chk(rays_o, 'rays_o')
    _chk(rays_d, 'rays_d', shape=tuple(rays_o.shape))
    _chk(z, 'z', shape=tuple(rays_o.shape[:-1]) + (None,))
    s = z.shape[-1]
    out = torch.empty(tuple(z.shape) + (3,), dtype=torch.float32, device=z.device)
    with torch.cuda.device(z.device):
        rc = _lib.lib().mvnerf_points_on_rays(_p(rays_o), _p(rays_d), _p(z), z.numel() // s, s, _p(out), _stream(z))
    _lib.check(rc, 'points_on_rays')
    return out


def project_points(world, intrinsics, extrinsics_inv):
    """compute_pixel_in_image_mv: world (B,...,3) -> pix (B,V,...,2), cam (B,V,...,4)."""
    _chk(world, 'world')
    b = world.shape[0]
    _chk(intrinsics, 'intrinsics', shape=(b, None, 4, 4))
    v = intrinsics.shape[1]
    _chk(extrinsics_inv, 'extrinsics_inv', shape=(b, v, 4, 4))
    mid = tuple(world.shape[1:-1])
    n = world.numel() // (3 * b)
    pix = torch.empty((b, v) + mid + (2,), dtype=torch.float32, device=world.device)
    cam = torch.empty((b, v) + mid + (4,), dtype=torch.float32, device=world.device)
    with torch.cuda.device(world.device):
        rc = _lib.lib().mvnerf_project_points(_p(world), _p(intrinsics), _p(extrinsics_inv), b, v, n, _p(pix), _p(cam),
                                              _stream(world))
    _lib.check(rc, 'project_points')
    return pix, cam


def camera_directions(dirs, extrinsics_inv):
    """world_to_camera_direction_vector_mv: dirs (B,R,3) -> (B,V,R,3)."""
    _chk(dirs, 'dirs', shape=(None, None, 3))
    b, r, _ = dirs.shape
    _chk(extrinsics_inv, 'extrinsics_inv', shape=(b, None, 4, 4))
    v = extrinsics_inv.shape[1]
    out = torch.empty((b, v, r, 3), dtype=torch.float32, device=dirs.device)
    with torch.cuda.device(dirs.device):
        rc = _lib.lib().mvnerf_camera_directions(_p(dirs), _p(extrinsics_inv), b, v, r, _p(out), _stream(dirs))
    _lib.check(rc, 'camera_directions')
    return out


def position_encoding(position, n_freq=10, pos_encoding_freq=np.pi):
    """position (...,D) -> (..., D*2*n_freq), layout (d, k, {sin,cos})."""
    _chk(position, 'position')
    out = torch.empty(tuple(position.shape[:-1]) + (position.shape[-1] * 2 * n_freq,), dtype=torch.float32,
                      device=position.device)
    with torch.cuda.device(position.device):
        rc = _lib.lib().mvnerf_position_encoding(_p(position), position.numel(), int(n_freq),
                                                 float(np.float32(pos_encoding_freq)), _p(out), _stream(position))
    _lib.check(rc, 'position_encoding')
    return out


def bilinear_gather(images, features, pixel_locations, return_taps=False):
    """images (N,H,W,3), features (N,H,W,256), pixel_locations (N,Q,2) -> (N,Q,259) [+ taps (N,Q,4)]."""
    _chk(images, 'images', shape=(None, None, None, 3))
    n, h, w, _ = images.shape
    _chk(features, 'features', shape=(n, h, w, 256))
    _chk(pixel_locations, 'pixel_locations', shape=(n, None, 2))
    q = pixel_locations.shape[1]
    out = torch.empty((n, q, 259), dtype=torch.float32, device=images.device)
    taps = torch.empty((n, q, 4), dtype=torch.int32, device=images.device) if return_taps else None
    with torch.cuda.device(images.device):
        rc = _lib.lib().mvnerf_bilinear_gather(_p(images), _p(features), _p(pixel_locations), n, q, h, w, _p(out),
                                               _p(taps), _stream(images))
    _lib.check(rc, 'bilinear_gather')
    return (out, taps) if return_taps else out


def sigma_to_alpha(sigma, dists):
    _chk(sigma, 'sigma')
    _chk(dists, 'dists', shape=tuple(sigma.shape))
    out = torch.empty_like(sigma)
    with torch.cuda.device(sigma.device):
        rc = _lib.lib().mvnerf_sigma_to_alpha(_p(sigma), _p(dists), sigma.numel(), _p(out), _stream(sigma))
    _lib.check(rc, 'sigma_to_alpha')
    return out


def sample_pdf(bins, weights, u, q7_mode=Q7_ZERO, return_indices=False):
    """bins (...,63), weights (...,62), u (...,64) -> samples (...,64) [+ above, below int32]."""
    _chk(bins, 'bins')
    lead = tuple(bins.shape[:-1])
    _chk(weights, 'weights', shape=lead + (None,))
    _chk(u, 'u', shape=lead + (None,))
    n = bins.numel() // bins.shape[-1]
    samples = torch.empty_like(u)
    above = torch.empty(u.shape, dtype=torch.int32, device=u.device) if return_indices else None
    below = torch.empty(u.shape, dtype=torch.int32, device=u.device) if return_indices else None
    if weights.shape[-1] != bins.shape[-1] - 1:
        raise ValueError(f'weights: last dim {weights.shape[-1]}, expected {bins.shape[-1] - 1}')
    with torch.cuda.device(u.device):
        rc = _lib.lib().mvnerf_sample_pdf(_p(bins), _p(weights), _p(u), n, bins.shape[-1], u.shape[-1], int(q7_mode),
                                          _p(samples), _p(above), _p(below), _stream(u))
    _lib.check(rc, 'sample_pdf')
    return (samples, above, below) if return_indices else samples


def readout(embedding, wr, br):
    """RenderReadout: embedding (...,128), wr (128,4), br (4,) -> rgbs (...,4)."""
    _chk(embedding, 'embedding', shape=tuple(embedding.shape[:-1]) + (128,))
    _chk(wr, 'wr', shape=(128, 4))
    _chk(br, 'br', shape=(4,))
    out = torch.empty(tuple(embedding.shape[:-1]) + (4,), dtype=torch.float32, device=embedding.device)
    with torch.cuda.device(embedding.device):
        rc = _lib.lib().mvnerf_readout(_p(embedding), _p(wr), _p(br), embedding.numel() // 128, _p(out), _stream(embedding))
    _lib.check(rc, 'readout')
    return out


def finish_view(rgb, depth):
    """render_view epilogue: rgb (n,3), depth (n) -> (rgb8 (n,3) uint8, depth8 (n) uint8)."""
    _chk(depth, 'depth')
    n = depth.numel()
    _chk(rgb, 'rgb', shape=tuple(depth.shape) + (3,))
    rgb8 = torch.empty(rgb.shape, dtype=torch.uint8, device=rgb.device)
    depth8 = torch.empty(depth.shape, dtype=torch.uint8, device=rgb.device)
    scratch = torch.empty(2, dtype=torch.float32, device=rgb.device)
    with torch.cuda.device(rgb.device):
        rc = _lib.lib().mvnerf_finish_view(_p(rgb), _p(depth), n, _p(scratch), _p(rgb8), _p(depth8), _stream(rgb))
    _lib.check(rc, 'finish_view')
    return rgb8, depth8


# ---- training step (model_v0.py:186-197): forward with stash, loss gradient, backward, Adam ---------------
def stash_bytes(b, v, r, s):
    return int(_lib.lib().mvnerf_stash_bytes(int(b), int(v), int(r), int(s)))


def field_eval_stash(rays_o, rays_d, z, images, features, intrinsics, extrinsics_inv, packed_net, stash=None, texel_table=None,
                     packed_split=None, kernel=None, range_status=None):
    """Training-mode field pass: -> (rgbs (B,R,S,4), stash uint8 tensor with the trunk pre-activations).
    packed_split: pack_net_split(net) -> the split-bf16 kernel (mvnerf_field_eval_stash_split), same stash.
    kernel, range_status (with packed_split): as field_eval_split -> mvnerf_field_eval_stash_split_ex."""
    _chk(rays_o, 'rays_o', shape=(None, None, 3))
    b, r, _ = rays_o.shape
    _chk(rays_d, 'rays_d', shape=(b, r, 3))
    _chk(z, 'z', shape=(b, r, None))
    s = z.shape[2]
    _, v, h, w = _scene(images, features, intrinsics, extrinsics_inv, b=b)
    _chk(packed_net, 'packed_net', shape=(packed_net_floats(),))
    dev = rays_o.device
    need = stash_bytes(b, v, r, s)
    if stash is None or stash.numel() < need:
        stash = torch.empty(need, dtype=torch.uint8, device=dev)
    rgbs = torch.empty((b, r, s, 4), dtype=torch.float32, device=dev)
    ws = torch.empty(int(_lib.lib().mvnerf_field_workspace_bytes(b, v, r)), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        if texel_table is not None:
            _chk(texel_table, 'texel_table', shape=(b, v, h, w, 128))
        if packed_split is None:
            if kernel is not None or range_status is not None:
                raise ValueError('kernel / range_status belong to the split path: pass packed_split=')
            rc = _lib.lib().mvnerf_field_eval_stash(_p(rays_o), _p(rays_d), _p(z), _p(images), _p(features), _p(texel_table),
                                                    _p(intrinsics), _p(extrinsics_inv), _p(packed_net), b, v, r, s, h, w, _p(rgbs),
                                                    _p(stash), _p(ws), _stream(rays_o))
        else:
            _chk(packed_split, 'packed_split', dtype=torch.uint8, shape=(int(_lib.lib().mvnerf_packed_net_split_bytes()),))
            ex = _split_ex_args(kernel, range_status, 1)
            if ex is not None:
                rc = _lib.lib().mvnerf_field_eval_stash_split_ex(_p(rays_o), _p(rays_d), _p(z), _p(images), _p(features), _p(texel_table),
                                                                 _p(intrinsics), _p(extrinsics_inv), _p(packed_net), _p(packed_split), b, v, r,
                                                                 s, h, w, _p(rgbs), _p(stash), _p(ws), *ex, _stream(rays_o))
                _lib.check(rc, 'field_eval_stash')
                return rgbs, stash
            rc = _lib.lib().mvnerf_field_eval_stash_split(_p(rays_o), _p(rays_d), _p(z), _p(images), _p(features), _p(texel_table),
                                                          _p(intrinsics), _p(extrinsics_inv), _p(packed_net), _p(packed_split), b, v, r, s,
                                                          h, w, _p(rgbs), _p(stash), _p(ws), _stream(rays_o))
    _lib.check(rc, 'field_eval_stash')
    return rgbs, stash


def pack_bwd_streams(net_keras):
    _chk(net_keras, 'net_keras', shape=(NET_PARAMS,))
    out = torch.empty(15 * 16384, dtype=torch.float32, device=net_keras.device)
    with torch.cuda.device(net_keras.device):
        _lib.check(_lib.lib().mvnerf_pack_bwd_streams(_p(net_keras), _p(out), _stream(net_keras)), 'pack_bwd_streams')
    return out


def mse_grad(pred, label, loss):
    """d pred of Keras MeanSquaredError; adds the loss value into the 1-element device tensor `loss`."""
    _chk(pred, 'pred')
    _chk(label, 'label', shape=tuple(pred.shape))
    _chk(loss, 'loss', shape=(1,))
    d = torch.empty_like(pred)
    with torch.cuda.device(pred.device):
        _lib.check(_lib.lib().mvnerf_mse_grad(_p(pred), _p(label), pred.numel(), _p(d), _p(loss), _stream(pred)), 'mse_grad')
    return d


def composite_bwd(z, rgbs, d_rgb, d_depth=None, d_weights=None, return_dz=False):
    """volumetric_render backward w.r.t. the per-sample (r,g,b,sigma): -> d_rgbs (...,S,4) [+ d_z (...,S)]."""
    _chk(z, 'z')
    s = z.shape[-1]
    lead = tuple(z.shape[:-1])
    _chk(rgbs, 'rgbs', shape=tuple(z.shape) + (4,))
    _chk(d_rgb, 'd_rgb', shape=lead + (3,))
    if d_depth is not None:
        _chk(d_depth, 'd_depth', shape=lead)
    if d_weights is not None:
        _chk(d_weights, 'd_weights', shape=tuple(z.shape))
    out = torch.empty_like(rgbs)
    d_z = torch.empty_like(z) if return_dz else None
    with torch.cuda.device(z.device):
        rc = _lib.lib().mvnerf_composite_bwd(_p(z), _p(rgbs), _p(d_rgb), _p(d_depth), _p(d_weights), z.numel() // s, s,
                                             _p(out), _p(d_z), _stream(z))
    _lib.check(rc, 'composite_bwd')
    return (out, d_z) if return_dz else out


def field_backward(rays_o, rays_d, z, images, features, intrinsics, extrinsics_inv, net_keras, bwd_streams, stash, rgbs,
                   d_rgbs, grad, scratch=None, d_z=None, d_features=None, texel_table=None, texel_grad=None):
    """Accumulate dL/d(net variables) of one field_eval_stash call into `grad` (247300 floats, Keras order);
    d_z (optional, (B,R,S)) is incremented by the gradient through the sample positions, d_features (optional,
    (B,V,H,W,256)) by the gradient w.r.t. the source feature maps.  texel_table (optional): project_texels of the same
    net; used for the feature rows' part of d_z, and - with the scratch texel_grad (B,V,H,W,128) - for d_features (the cotangents are
    scattered onto the 128-channel table gradient and W0 is applied once per texel; mvnerf_field_backward_table)."""
    b, r, s = z.shape
    _, v, h, w, _ = images.shape
    _chk(net_keras, 'net_keras', shape=(NET_PARAMS,))
    _chk(bwd_streams, 'bwd_streams', shape=(15 * 16384,))
    if d_z is not None:
        _chk(d_z, 'd_z', shape=(b, r, s))
    _chk(rgbs, 'rgbs', shape=(b, r, s, 4))
    _chk(d_rgbs, 'd_rgbs', shape=(b, r, s, 4))
    _chk(grad, 'grad', shape=(NET_PARAMS,))
    if d_features is not None:
        _chk(d_features, 'd_features', shape=(b, v, h, w, 256))
    need = int(_lib.lib().mvnerf_field_backward_scratch_bytes(b, v, r, s))
    if scratch is None or scratch.numel() < need:
        scratch = torch.empty(need, dtype=torch.uint8, device=z.device)
    if texel_table is not None:
        _chk(texel_table, 'texel_table', shape=(b, v, h, w, 128))
    if texel_grad is not None:
        _chk(texel_grad, 'texel_grad', shape=(b, v, h, w, 128))
    with torch.cuda.device(z.device):
        rc = _lib.lib().mvnerf_field_backward_table(_p(rays_o), _p(rays_d), _p(z), _p(images), _p(features), _p(texel_table),
                                                    _p(texel_grad), _p(intrinsics), _p(extrinsics_inv), _p(net_keras), _p(bwd_streams), _p(stash),
                                                    _p(rgbs), _p(d_rgbs), b, v, r, s, h, w, _p(scratch), _p(grad), _p(d_z),
                                                    _p(d_features), _stream(z))
    _lib.check(rc, 'field_backward')
    return scratch


# ---- the per-point part of GraspReadout as fused passes (csrc/grasp_head.hip; delta_ngf/layers.py:8-42, lmvnerf/model_v4.py:261-322) ----
def grasp_head_pack(w4, wc):
    """The four Dense(128 -> 64) kernels w4 (4,64,128) and the Dense(256 -> 64) kernel wc (64,256), torch [out, in] layout -> MFMA operand image."""
    _chk(w4, 'w4', shape=(4, 64, 128))
    _chk(wc, 'wc', shape=(64, 256))
    out = torch.empty(int(_lib.lib().mvnerf_grasp_head_packed_floats()), dtype=torch.float32, device=w4.device)
    with torch.cuda.device(w4.device):
        _lib.check(_lib.lib().mvnerf_grasp_head_pack(_p(w4), _p(wc), _p(out), _stream(w4)), 'grasp_head_pack')
    return out


def _head_out(out, specs, dev):
    """The output tensors of a head pass: fresh ones, or the caller's `out` tuple checked against specs = ((name, shape), ...) in order."""
    if out is None:
        return tuple(torch.empty(shape, dtype=torch.float32, device=dev) for _, shape in specs)
    if len(out) != len(specs):
        raise ValueError(f'out: {len(out)} tensors, expected {len(specs)} ({", ".join(nm for nm, _ in specs)})')
    return tuple(_chk(t, 'out ' + nm, shape=shape) for t, (nm, shape) in zip(out, specs))


def grasp_head_fwd(acts, packed, b4, bc, out=None):
    """acts (4,N,128) -> c (N,256) = [elu(W_k a_k + b_k)], y (N,64) = elu(W_c c + b_c).  out: (c, y) to write into."""
    _chk(acts, 'acts', shape=(4, None, 128))
    n = acts.shape[1]
    _chk(packed, 'packed', shape=(int(_lib.lib().mvnerf_grasp_head_packed_floats()),))
    _chk(b4, 'b4', shape=(4, 64))
    _chk(bc, 'bc', shape=(64,))
    c, y = _head_out(out, (('c', (n, 256)), ('y', (n, 64))), acts.device)
    with torch.cuda.device(acts.device):
        _lib.check(_lib.lib().mvnerf_grasp_head_fwd(_p(acts), _p(packed), _p(b4), _p(bc), n, _p(c), _p(y), _stream(acts)), 'grasp_head_fwd')
    return c, y


def grasp_head_vjp(g_y, c, y, packed, out=None):
    """g_y (N,64) -> g_v (N,64), q (N,256), g_u (N,256), g_acts (4,N,128).  out: the four tensors to write into."""
    _chk(g_y, 'g_y', shape=(None, 64))
    n = g_y.shape[0]
    _chk(c, 'c', shape=(n, 256))
    _chk(y, 'y', shape=(n, 64))
    _chk(packed, 'packed', shape=(int(_lib.lib().mvnerf_grasp_head_packed_floats()),))
    dev = g_y.device
    g_v, q, g_u, g_acts = _head_out(out, (('g_v', (n, 64)), ('q', (n, 256)), ('g_u', (n, 256)), ('g_acts', (4, n, 128))), dev)
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().mvnerf_grasp_head_vjp(_p(g_y), _p(c), _p(y), _p(packed), n, _p(g_v), _p(q), _p(g_u), _p(g_acts), _stream(g_y)),
                   'grasp_head_vjp')
    return g_v, q, g_u, g_acts


def grasp_head_vjp_acts(g_y, c, y, packed, out=None):
    """mvnerf_grasp_head_vjp_acts: g_y (N,64) -> g_acts (4,N,128) only (a frozen read-out), bit-identical to grasp_head_vjp(...)[3]."""
    _chk(g_y, 'g_y', shape=(None, 64))
    n = g_y.shape[0]
    _chk(c, 'c', shape=(n, 256))
    _chk(y, 'y', shape=(n, 64))
    _chk(packed, 'packed', shape=(int(_lib.lib().mvnerf_grasp_head_packed_floats()),))
    g_acts = torch.empty((4, n, 128), dtype=torch.float32, device=g_y.device) if out is None else _chk(out, 'out', shape=(4, n, 128))
    with torch.cuda.device(g_y.device):
        _lib.check(_lib.lib().mvnerf_grasp_head_vjp_acts(_p(g_y), _p(c), _p(y), _p(packed), n, _p(g_acts), _stream(g_y)), 'grasp_head_vjp_acts')
    return g_acts


def grasp_head_vjp_bwd(t_acts, g_y, c, y, q, packed, out=None):
    """t_acts (4,N,128) = dL/d(g_acts) -> out_gy (N,64) = dL/d(g_y), r (N,256), m (N,64), p (N,256) (see include/mvnerf_hip.h).
    out: the four tensors to write into."""
    _chk(t_acts, 't_acts', shape=(4, None, 128))
    n = t_acts.shape[1]
    _chk(g_y, 'g_y', shape=(n, 64))
    _chk(c, 'c', shape=(n, 256))
    _chk(y, 'y', shape=(n, 64))
    _chk(q, 'q', shape=(n, 256))
    _chk(packed, 'packed', shape=(int(_lib.lib().mvnerf_grasp_head_packed_floats()),))
    dev = t_acts.device
    out_gy, r, m, p_ = _head_out(out, (('out_gy', (n, 64)), ('r', (n, 256)), ('m', (n, 64)), ('p', (n, 256))), dev)
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().mvnerf_grasp_head_vjp_bwd(_p(t_acts), _p(g_y), _p(c), _p(y), _p(q), _p(packed), n, _p(out_gy), _p(r), _p(m),
                                                        _p(p_), _stream(t_acts)), 'grasp_head_vjp_bwd')
    return out_gy, r, m, p_


# ---- the per-pose part of GraspReadout with frozen weights (csrc/grasp_tail.hip; delta_ngf/layers.py:24-28, 39-41) -------------------------
TAIL_STASH = 320          # floats per row: the pre-activations h0 (128) | x1 | h1 | x2 (64 each)


def grasp_tail_packed_floats(n5):
    return int(_lib.lib().mvnerf_grasp_tail_packed_floats(int(n5)))


def grasp_tail_pack(block_0, block_1, output_layer, out=None):
    """The weights of GraspReadout's block_0 = (layer_0.weight (128, K), layer_0.bias, layer_1.weight (64, 128), layer_1.bias, shortcut.weight
    (64, K)), block_1 = (layer_0.weight (64, 64), layer_0.bias, layer_1.weight (64, 64), layer_1.bias) and output_layer = (weight (1, 64) or
    (64,), bias (1,) or None), torch [out, in] layout, K = 64 n5 -> the kernels' operand image.  out: a packed buffer to refill in place."""
    w0, b0, w1, b1, ws = block_0
    w0b, b0b, w1b, b1b = block_1
    w_out, b_out = output_layer
    _chk(w0, 'block_0.layer_0.weight', shape=(128, None))
    k = w0.shape[1]
    if k <= 0 or k % 64 != 0:
        raise ValueError(f'block_0.layer_0.weight: {k} inputs, expected a multiple of 64 (n5 offsets x 64)')
    n5 = k // 64
    for t, name, shape in ((b0, 'block_0.layer_0.bias', (128,)), (w1, 'block_0.layer_1.weight', (64, 128)), (b1, 'block_0.layer_1.bias', (64,)),
                           (ws, 'block_0.shortcut.weight', (64, k)), (w0b, 'block_1.layer_0.weight', (64, 64)), (b0b, 'block_1.layer_0.bias', (64,)),
                           (w1b, 'block_1.layer_1.weight', (64, 64)), (b1b, 'block_1.layer_1.bias', (64,))):
        _chk(t, name, shape=shape)
    _chk(w_out, 'output_layer.weight')
    if w_out.numel() != 64:
        raise ValueError(f'output_layer.weight: shape {tuple(w_out.shape)}, expected (1, 64)')
    if b_out is not None:
        _chk(b_out, 'output_layer.bias', shape=(1,))
    n = grasp_tail_packed_floats(n5)
    packed = torch.empty(n, dtype=torch.float32, device=w0.device) if out is None else _chk(out, 'out', shape=(n,))
    with torch.cuda.device(w0.device):
        rc = _lib.lib().mvnerf_grasp_tail_pack(_p(w0), _p(b0), _p(w1), _p(b1), _p(ws), _p(w0b), _p(b0b), _p(w1b), _p(b1b), _p(w_out), _p(b_out),
                                               n5, _p(packed), _stream(w0))
    _lib.check(rc, 'grasp_tail_pack')
    return packed


def _tail_shapes(x, packed):
    _chk(x, 'x', shape=(None, None))
    m, k = x.shape
    if m <= 0 or k <= 0 or k % 64 != 0:
        raise ValueError(f'x: shape {tuple(x.shape)}, expected (M >= 1, 64 n5)')
    _chk(packed, 'packed', shape=(grasp_tail_packed_floats(k // 64),))
    return m, k // 64


def grasp_tail_fwd(x, packed, stash=True, out=None):
    """mvnerf_grasp_tail_fwd: x (M, 64 n5) -> success (M,) [, stash (M, 320) for grasp_tail_vjp].  stash: True allocates one, False / None
    runs the value only, a tensor is written in place; out: a success tensor to write into."""
    m, n5 = _tail_shapes(x, packed)
    success = torch.empty(m, dtype=torch.float32, device=x.device) if out is None else _chk(out, 'out', shape=(m,))
    if stash is True:
        stash = torch.empty((m, TAIL_STASH), dtype=torch.float32, device=x.device)
    elif stash is False:
        stash = None
    if stash is not None:
        _chk(stash, 'stash', shape=(m, TAIL_STASH))
    with torch.cuda.device(x.device):
        _lib.check(_lib.lib().mvnerf_grasp_tail_fwd(_p(x), _p(packed), m, n5, _p(success), _p(stash), _stream(x)), 'grasp_tail_fwd')
    return success if stash is None else (success, stash)


def grasp_tail_vjp(x, stash, packed, g_s=None, out=None):
    """mvnerf_grasp_tail_vjp: cotangent g_s (M,) of success (None: ones) -> g_x (M, 64 n5)."""
    m, n5 = _tail_shapes(x, packed)
    _chk(stash, 'stash', shape=(m, TAIL_STASH))
    if g_s is not None:
        _chk(g_s, 'g_s', shape=(m,))
    g_x = torch.empty_like(x) if out is None else _chk(out, 'out', shape=(m, 64 * n5))
    with torch.cuda.device(x.device):
        _lib.check(_lib.lib().mvnerf_grasp_tail_vjp(_p(x), _p(g_s), _p(stash), _p(packed), m, n5, _p(g_x), _stream(x)), 'grasp_tail_vjp')
    return g_x


TAIL_COT, TAIL_ACT, TAIL_COT2, TAIL_TAN = 320, 320, 256, 320          # floats per row of the training passes' buffers (include/mvnerf_hip.h)


def grasp_tail_vjp_train(x, stash, packed, g_s=None, out=None):
    """mvnerf_grasp_tail_vjp_train: the tail's first backward with trainable weights.  g_s (M,) or None (ones) -> g_x (M, 64 n5) (the bits
    of grasp_tail_vjp), cot (M, 320) = [g_h0 | g_x1 | g_h1 | g_x2], act (M, 320) = [E(h0) | E(x1) | E(h1) | g_s relu(x2)], ex (M, 64 n5) = E(x).
    out: the four tensors to write into."""
    m, n5 = _tail_shapes(x, packed)
    _chk(stash, 'stash', shape=(m, TAIL_STASH))
    if g_s is not None:
        _chk(g_s, 'g_s', shape=(m,))
    dev = x.device
    if out is None:
        g_x, ex = torch.empty_like(x), torch.empty_like(x)
        cot = torch.empty((m, TAIL_COT), dtype=torch.float32, device=dev)
        act = torch.empty((m, TAIL_ACT), dtype=torch.float32, device=dev)
    else:                                                    # (g_x, cot, act, ex) to write into
        g_x, cot, act, ex = out
        for t, name, cols in ((g_x, 'out g_x', 64 * n5), (cot, 'out cot', TAIL_COT), (act, 'out act', TAIL_ACT), (ex, 'out ex', 64 * n5)):
            _chk(t, name, shape=(m, cols))
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().mvnerf_grasp_tail_vjp_train(_p(x), _p(g_s), _p(stash), _p(packed), m, n5, _p(g_x), _p(cot), _p(act), _p(ex), _stream(x)),
                   'grasp_tail_vjp_train')
    return g_x, cot, act, ex


def grasp_tail_vjp_bwd(x, t_x, stash, cot, packed, g_s=None, want_x=True, out=None):
    """mvnerf_grasp_tail_vjp_bwd: t_x (M, 64 n5) = dL/d(g_x) -> out_gs (M,) = dL/d(g_s), out_x (M, 64 n5) = dL/dx (None with want_x=False),
    cot2 (M, 256) = [pi_h0 | pi_x1 | pi_h1], tan (M, 320) = [de0 | da1 | de1 | g_s H dx2], dex (M, 64 n5) = E'(x) t (see include/mvnerf_hip.h)."""
    m, n5 = _tail_shapes(x, packed)
    _chk(t_x, 't_x', shape=(m, 64 * n5))
    _chk(stash, 'stash', shape=(m, TAIL_STASH))
    _chk(cot, 'cot', shape=(m, TAIL_COT))
    if g_s is not None:
        _chk(g_s, 'g_s', shape=(m,))
    dev = x.device
    if out is None:
        out_gs = torch.empty(m, dtype=torch.float32, device=dev)
        out_x = torch.empty_like(x) if want_x else None
        cot2 = torch.empty((m, TAIL_COT2), dtype=torch.float32, device=dev)
        tan = torch.empty((m, TAIL_TAN), dtype=torch.float32, device=dev)
        dex = torch.empty_like(x)
    else:                                                    # (out_gs, out_x or None, cot2, tan, dex) to write into
        out_gs, out_x, cot2, tan, dex = out
        _chk(out_gs, 'out out_gs', shape=(m,))
        for t, name, cols in ((out_x, 'out out_x', 64 * n5), (cot2, 'out cot2', TAIL_COT2), (tan, 'out tan', TAIL_TAN), (dex, 'out dex', 64 * n5)):
            if t is not None or name != 'out out_x':
                _chk(t, name, shape=(m, cols))
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().mvnerf_grasp_tail_vjp_bwd(_p(x), _p(t_x), _p(g_s), _p(stash), _p(cot), _p(packed), m, n5, _p(out_gs), _p(out_x),
                                                        _p(cot2), _p(tan), _p(dex), _stream(x)), 'grasp_tail_vjp_bwd')
    return out_gs, out_x, cot2, tan, dex


# ---- one grasp-pose optimisation step behind the C ABI (csrc/grasp_api.hip; lmvnerf/grasp_optimizer.py:158-184) ------------------------------
def grasp_workspace_bytes(b, v, p, n5, bf16=False):
    fn = _lib.lib().mvnerf_grasp_workspace_bytes_bf16 if bf16 else _lib.lib().mvnerf_grasp_workspace_bytes
    return int(fn(int(b), int(v), int(p), int(n5)))


def _nets16(nets16):
    """(packed16, bwd16) of the _bf16 grasp entry points -> their two pointer arguments."""
    packed16, bwd16 = nets16
    _chk(packed16, 'packed16', dtype=torch.uint8, shape=(int(_lib.lib().mvnerf_packed_net_bf16_bytes()),))
    _chk(bwd16, 'bwd16', dtype=torch.uint8, shape=(int(_lib.lib().mvnerf_bwd_streams_bf16_bytes()),))
    return _p(packed16), _p(bwd16)


def grasp_call(images, features, intrinsics, extrinsics_inv, packed_net, split, bwd_streams, head_packed, head_b4, head_bc, tail_packed, offsets,
               t, rot, success, g_t, g_rot, workspace):
    """Fill a mvnerf_grasp_call (include/mvnerf_hip.h) from device tensors after checking shapes; the caller keeps the tensors alive."""
    b, v, h, w = _scene(images, features, intrinsics, extrinsics_inv)
    _chk(packed_net, 'packed_net', shape=(packed_net_floats(),))
    _chk(split, 'split', dtype=torch.uint8, shape=(int(_lib.lib().mvnerf_packed_net_split_bytes()),))
    _chk(bwd_streams, 'bwd_streams', shape=(15 * 16384,))
    _chk(head_packed, 'head_packed', shape=(int(_lib.lib().mvnerf_grasp_head_packed_floats()),))
    _chk(head_b4, 'head_b4', shape=(4, 64))
    _chk(head_bc, 'head_bc', shape=(64,))
    _chk(offsets, 'offsets', shape=(None, 4, 4))
    n5 = offsets.shape[0]
    _chk(tail_packed, 'tail_packed', shape=(grasp_tail_packed_floats(n5),))
    p, rep, rd = _pose_shapes(t, rot)
    _chk(success, 'success', shape=(b, p))
    _chk(g_t, 'g_t', shape=(p, 3))
    _chk(g_rot, 'g_rot', shape=(p, rd))
    _chk(workspace, 'workspace', dtype=torch.uint8)
    c = _lib.GraspCall()
    for name, x in (('images', images), ('features', features), ('intrinsics', intrinsics), ('extrinsics_inv', extrinsics_inv),
                    ('packed_net', packed_net), ('split', split), ('bwd_streams', bwd_streams), ('head_packed', head_packed),
                    ('head_b4', head_b4), ('head_bc', head_bc), ('tail_packed', tail_packed), ('offsets', offsets), ('t', t), ('rot', rot),
                    ('success', success), ('g_t', g_t), ('g_rot', g_rot), ('workspace', workspace)):
        setattr(c, name, x.data_ptr())
    c.B, c.V, c.H, c.W = b, v, h, w
    c.rep, c.P, c.n5 = rep, p, n5
    c.workspace_bytes = workspace.numel()
    return c


def grasp_success(call, stream_of, nets16=None):
    """mvnerf_grasp_success: stages 1-4 on a filled grasp_call -> its success (B, P).  nets16 = (packed16, bwd16): mvnerf_grasp_success_bf16,
    the trunk on the bf16 MFMA (workspace: grasp_workspace_bytes(..., bf16=True)); likewise for the two functions below."""
    with torch.cuda.device(stream_of.device):
        if nets16 is None:
            rc = _lib.lib().mvnerf_grasp_success(ctypes.byref(call), _stream(stream_of))
        else:
            rc = _lib.lib().mvnerf_grasp_success_bf16(ctypes.byref(call), *_nets16(nets16), _stream(stream_of))
    _lib.check(rc, 'grasp_success')


def grasp_success_and_gradients(call, stream_of, nets16=None):
    """mvnerf_grasp_success_and_gradients: stages 1-7 -> success, g_t, g_rot of the call."""
    with torch.cuda.device(stream_of.device):
        if nets16 is None:
            rc = _lib.lib().mvnerf_grasp_success_and_gradients(ctypes.byref(call), _stream(stream_of))
        else:
            rc = _lib.lib().mvnerf_grasp_success_and_gradients_bf16(ctypes.byref(call), *_nets16(nets16), _stream(stream_of))
    _lib.check(rc, 'grasp_success_and_gradients')


def grasp_opt_step(call, cfg, train_flags, counters, m_t, v_t, m_r, v_r, stream_of, nets16=None):
    """mvnerf_grasp_opt_step: stages 1-8, in place on the call's t, rot and on the Adam state (arguments as pose_adam_step)."""
    p, rd = call.P, (4, 6)[call.rep]
    _chk(train_flags, 'train_flags', dtype=torch.int32, shape=(2,))
    _chk(counters, 'counters', dtype=torch.int32, shape=(2, p))
    for x, n, width in ((m_t, 'm_t', 3), (v_t, 'v_t', 3), (m_r, 'm_r', rd), (v_r, 'v_r', rd)):
        _chk(x, n)
        if x.numel() != width * p:
            raise ValueError(f'{n}: {x.numel()} floats, expected {width * p}')
    with torch.cuda.device(stream_of.device):
        moments = (_p(train_flags), _p(counters), _p(m_t), _p(v_t), _p(m_r), _p(v_r), _stream(stream_of))
        if nets16 is None:
            rc = _lib.lib().mvnerf_grasp_opt_step(ctypes.byref(call), ctypes.byref(cfg), *moments)
        else:
            rc = _lib.lib().mvnerf_grasp_opt_step_bf16(ctypes.byref(call), *_nets16(nets16), ctypes.byref(cfg), *moments)
    _lib.check(rc, 'grasp_opt_step')


def train_workspace_bytes(b, v, r, s, h, w, use_tables, want_d_features):
    return int(_lib.lib().mvnerf_train_workspace_bytes(int(b), int(v), int(r), int(s), int(h), int(w), int(bool(use_tables)),
                                                       int(bool(want_d_features))))


def train_call(rays_o, rays_d, images, features, intrinsics, extrinsics_inv, u_coarse, u_fine, labels, near, far, nets, packed, split,
               bwd_streams, loss, grad, outputs, workspace, q7_mode=Q7_ZERO, stop_fine_z=False, use_tables=False, d_features=None):
    """Fill a mvnerf_train_call (include/mvnerf_hip.h) from device tensors after checking shapes; the caller keeps the tensors alive.
    nets / packed / split / bwd_streams: (coarse, fine) pairs (split may be None: fp32-MFMA forward); outputs: (rgb, depth, fine_rgb,
    fine_depth); grad: (2 x 247300,) [coarse | fine]; workspace: uint8 tensor of train_workspace_bytes(...)."""
    _chk(rays_o, 'rays_o', shape=(None, None, 3))
    b, r, _ = rays_o.shape
    _chk(rays_d, 'rays_d', shape=(b, r, 3))
    _, v, h, w = _scene(images, features, intrinsics, extrinsics_inv, b=b)
    _chk(u_coarse, 'u_coarse', shape=(b, r, None))
    s = u_coarse.shape[2]
    _chk(u_fine, 'u_fine', shape=(b, r, s))
    _chk(labels, 'labels', shape=(b, r, 3))
    for k in range(2):
        _chk(nets[k], 'net', shape=(NET_PARAMS,))
        _chk(packed[k], 'packed', shape=(packed_net_floats(),))
        _chk(bwd_streams[k], 'bwd_streams', shape=(15 * 16384,))
        if split is not None:
            _chk(split[k], 'split', dtype=torch.uint8, shape=(int(_lib.lib().mvnerf_packed_net_split_bytes()),))
    _chk(loss, 'loss', shape=(1,))
    _chk(grad, 'grad', shape=(2 * NET_PARAMS,))
    rgb, depth, fine_rgb, fine_depth = outputs
    _chk(rgb, 'rgb', shape=(b, r, 3))
    _chk(depth, 'depth', shape=(b, r))
    _chk(fine_rgb, 'fine_rgb', shape=(b, r, 3))
    _chk(fine_depth, 'fine_depth', shape=(b, r))
    if d_features is not None:
        _chk(d_features, 'd_features', shape=(b, v, h, w, 256))
    _chk(workspace, 'workspace', dtype=torch.uint8)
    c = _lib.TrainCall()
    for name, t in (('rays_o', rays_o), ('rays_d', rays_d), ('images', images), ('features', features), ('intrinsics', intrinsics),
                    ('extrinsics_inv', extrinsics_inv), ('u_coarse', u_coarse), ('u_fine', u_fine), ('labels', labels),
                    ('net_coarse', nets[0]), ('net_fine', nets[1]), ('packed_coarse', packed[0]), ('packed_fine', packed[1]),
                    ('split_coarse', None if split is None else split[0]), ('split_fine', None if split is None else split[1]),
                    ('bwd_streams_coarse', bwd_streams[0]), ('bwd_streams_fine', bwd_streams[1]), ('loss', loss), ('grad', grad),
                    ('rgb', rgb), ('depth', depth), ('fine_rgb', fine_rgb), ('fine_depth', fine_depth), ('d_features', d_features),
                    ('workspace', workspace)):
        setattr(c, name, None if t is None else t.data_ptr())
    c.B, c.V, c.R, c.S, c.H, c.W = b, v, r, s, h, w
    c.near_, c.far_ = float(near), float(far)
    c.q7_mode, c.stop_fine_z, c.use_texel_tables = int(q7_mode), int(bool(stop_fine_z)), int(bool(use_tables))
    c.workspace_bytes = workspace.numel()
    return c


def adam_state(m, v, lr_t, beta1=0.9, beta2=0.999, eps=1e-7, clip=1.0, update_mask=None, repack=True):
    _chk(m, 'm', shape=(2 * NET_PARAMS,))
    _chk(v, 'v', shape=(2 * NET_PARAMS,))
    if update_mask is not None:
        _chk(update_mask, 'update_mask', dtype=torch.uint8, shape=(2 * NET_PARAMS,))
    a = _lib.AdamState()
    a.m, a.v, a.update_mask = m.data_ptr(), v.data_ptr(), None if update_mask is None else update_mask.data_ptr()
    a.lr_t, a.beta1, a.beta2, a.eps, a.clip = float(lr_t), float(beta1), float(beta2), float(eps), float(clip)
    a.repack = int(bool(repack))
    return a


def loss_and_grads(call, stream_of):
    """mvnerf_loss_and_grads: MVVNeRFRenderer.train_step's tape (model_v0.py:190-194) on a filled train_call."""
    with torch.cuda.device(stream_of.device):
        _lib.check(_lib.lib().mvnerf_loss_and_grads(ctypes.byref(call), _stream(stream_of)), 'loss_and_grads')


def apply_gradients(call, adam, stream_of):
    """mvnerf_apply_gradients: optimize() (nerf_utils.py:8-12) - clip-by-value, Adam, re-pack."""
    with torch.cuda.device(stream_of.device):
        _lib.check(_lib.lib().mvnerf_apply_gradients(ctypes.byref(call), ctypes.byref(adam), _stream(stream_of)), 'apply_gradients')


def train_step_c(call, adam, stream_of):
    """mvnerf_train_step: the two above in one C call."""
    with torch.cuda.device(stream_of.device):
        _lib.check(_lib.lib().mvnerf_train_step(ctypes.byref(call), ctypes.byref(adam), _stream(stream_of)), 'train_step')


def gemm_nt_ok(m, n, k):
    """Shapes mvnerf_gemm_nt takes."""
    return m > 0 and n > 0 and k > 0 and m % 32 == 0 and n % 64 == 0 and k % 8 == 0


def _gemm_scratch(scratch, need, dev):
    """The split-K partial buffer of a GEMM call: a fresh one of `need` bytes (None for 0), or the caller's, which must hold that many."""
    if scratch is None:
        return torch.empty(need, dtype=torch.uint8, device=dev) if need else None
    if not isinstance(scratch, torch.Tensor) or not scratch.is_cuda or not scratch.is_contiguous():
        raise ValueError('scratch: needs a contiguous device tensor')
    if scratch.numel() * scratch.element_size() < need:
        raise ValueError(f'scratch: {scratch.numel() * scratch.element_size()} bytes, this shape needs {need}')
    return scratch


def gemm_nt(a, bt, bias=None, out=None, scratch=None):
    """mvnerf_gemm_nt / mvnerf_gemm_nt_bias: a (M,K) @ bt (N,K)^T [+ bias (N,)] -> (M,N), fp32, deterministic (K split into ranges whose
    partials are added in order).  out: the (M,N) tensor to write into; scratch: at least mvnerf_gemm_nt_scratch_bytes(M,N,K) bytes."""
    m, k = a.shape
    n = bt.shape[0]
    _chk(a, 'a', shape=(m, k))
    _chk(bt, 'bt', shape=(n, k))
    if bias is not None:
        _chk(bias, 'bias', shape=(n,))
    out = torch.empty((m, n), dtype=torch.float32, device=a.device) if out is None else _chk(out, 'out', shape=(m, n))
    scratch = _gemm_scratch(scratch, int(_lib.lib().mvnerf_gemm_nt_scratch_bytes(m, n, k)), a.device)
    with torch.cuda.device(a.device):
        if bias is None:
            rc = _lib.lib().mvnerf_gemm_nt(_p(a), _p(bt), _p(out), m, n, k, _p(scratch), _stream(a))
        else:
            rc = _lib.lib().mvnerf_gemm_nt_bias(_p(a), _p(bt), _p(bias), _p(out), m, n, k, _p(scratch), _stream(a))
    _lib.check(rc, 'gemm_nt')
    return out


def gemm_tn_ok(m, n, k):
    """Shapes mvnerf_gemm_tn takes."""
    return m > 0 and n > 0 and k > 0 and m % 8 == 0 and n % 32 == 0 and k % 64 == 0


def gemm_tn(g, a, out=None, scratch=None):
    """mvnerf_gemm_tn: g (M,N)^T @ a (M,K) -> (N,K), fp32, deterministic; no transposed copies.  out: the (N,K) tensor to write into;
    scratch: at least mvnerf_gemm_tn_scratch_bytes(M,N,K) bytes."""
    m, n = g.shape
    k = a.shape[1]
    _chk(g, 'g', shape=(m, n))
    _chk(a, 'a', shape=(m, k))
    out = torch.empty((n, k), dtype=torch.float32, device=a.device) if out is None else _chk(out, 'out', shape=(n, k))
    scratch = _gemm_scratch(scratch, int(_lib.lib().mvnerf_gemm_tn_scratch_bytes(m, n, k)), a.device)
    with torch.cuda.device(a.device):
        rc = _lib.lib().mvnerf_gemm_tn(_p(g), _p(a), _p(out), m, n, k, _p(scratch), _stream(a))
    _lib.check(rc, 'gemm_tn')
    return out


def gemm_tn_batched(g, a, g2=None, a2=None, colsum_of=0, out=None, scratch=None):
    """mvnerf_gemm_tn_batched: out[b] = g[b]^T @ a[b] (+ g2[b]^T @ a2[b]) for a batch of weight gradients that share their M rows, and the
    column sums of g (colsum_of=1) or g2 (=2) from the same pass.  g, g2: (batch, M, N) views whose last dimension is contiguous - e.g.
    `x.view(M, batch, N).permute(1, 0, 2)` for the column blocks of one (M, batch * N) matrix: no copies are made; a, a2: (batch, M, K).
    -> (batch, N, K) [, (batch, N)].  out: the (batch, N, K) tensor to write into, with column sums the pair (out, colsum); scratch: at
    least mvnerf_gemm_tn_batched_scratch_bytes(M, N, K, batch, colsum_of != 0) bytes."""
    def strides(t, name):
        if t.dim() != 3 or t.stride(2) != 1 or t.dtype != torch.float32 or not t.is_cuda:
            raise ValueError(f'{name}: needs a float32 device tensor (batch, M, cols) with contiguous rows')
        return t.stride(0), t.stride(1)
    batch, m, n = g.shape
    k = a.shape[2]
    if tuple(a.shape[:2]) != (batch, m):
        raise ValueError(f'a: {tuple(a.shape)} does not match g {tuple(g.shape)}')
    q = _lib.GemmTnBatch()
    q.g, q.a = _p(g), _p(a)
    (q.g_batch_stride, q.ldg), (q.a_batch_stride, q.lda) = strides(g, 'g'), strides(a, 'a')
    if g2 is not None:
        if tuple(g2.shape) != tuple(g.shape) or tuple(a2.shape) != tuple(a.shape):
            raise ValueError('g2 / a2 must have the shapes of g / a')
        q.g2, q.a2 = _p(g2), _p(a2)
        (q.g2_batch_stride, q.ldg2), (q.a2_batch_stride, q.lda2) = strides(g2, 'g2'), strides(a2, 'a2')
    q.colsum_of = int(colsum_of)
    if out is None:
        out = torch.empty((batch, n, k), dtype=torch.float32, device=a.device)
        colsum = torch.empty((batch, n), dtype=torch.float32, device=a.device) if colsum_of else None
    else:
        out, colsum = out if colsum_of else (out, None)
        _chk(out, 'out', shape=(batch, n, k))
        if colsum_of:
            _chk(colsum, 'out colsum', shape=(batch, n))
    scratch = _gemm_scratch(scratch, int(_lib.lib().mvnerf_gemm_tn_batched_scratch_bytes(m, n, k, batch, int(bool(colsum_of)))), a.device)
    with torch.cuda.device(a.device):
        rc = _lib.lib().mvnerf_gemm_tn_batched(ctypes.byref(q), _p(out), _p(colsum), m, n, k, batch, _p(scratch), _stream(a))
    _lib.check(rc, 'gemm_tn_batched')
    return (out, colsum) if colsum_of else out


SPLIT_KERNELS = {'split_f16': 0, 'split_bf16': 1, 'split_bf16_32x32x16': 2}


def set_split_kernel(name):
    """mvnerf_set_split_kernel: which kernel runs the split field passes of this process - 'split_f16' (default: two fp16 pieces per
    operand, three MFMAs per product block), 'split_bf16' (exact three-piece bf16 cut, six MFMAs) or 'split_bf16_32x32x16' (round 2's
    kernel).  Returns the previous name.  The environment variable MVNERF_SPLIT_MFMA overrides it at every launch."""
    if name not in SPLIT_KERNELS:
        raise ValueError(f'split kernel must be one of {sorted(SPLIT_KERNELS)}, got {name!r}')
    prev = int(_lib.lib().mvnerf_set_split_kernel(SPLIT_KERNELS[name]))
    return {v: k for k, v in SPLIT_KERNELS.items()}[prev]


def _split_ex_args(kernel, range_status, n_status):
    """(which, range_status pointer) of an _ex entry point, or None when both keywords are left alone (the plain entry point runs)."""
    if kernel is None and range_status is None:
        return None
    if kernel is not None and kernel not in SPLIT_KERNELS:
        raise ValueError(f'kernel must be None or one of {sorted(SPLIT_KERNELS)}, got {kernel!r}')
    if range_status is not None:
        _chk(range_status, 'range_status', shape=(n_status,))
    return (-1 if kernel is None else SPLIT_KERNELS[kernel], _p(range_status))


def net_range(net_keras, out=None):
    """mvnerf_net_range: -> device tensor [max |w| over the weights pack_net_split cuts (W0, the 12 hidden kernels), max |.| over all
    variables]; NaN stays NaN.  Compare [0] with F16X3_MAX_WEIGHT.  No host synchronisation here."""
    _chk(net_keras, 'net_keras', shape=(NET_PARAMS,))
    if out is None:
        out = torch.empty(2, dtype=torch.float32, device=net_keras.device)
    _chk(out, 'out', shape=(2,))
    with torch.cuda.device(net_keras.device):
        _lib.check(_lib.lib().mvnerf_net_range(_p(net_keras), _p(out), _stream(net_keras)), 'net_range')
    return out


def set_deterministic(on=True):
    """mvnerf_set_deterministic.  Weight gradients are ALWAYS summed in a fixed order since round 2 (stored per-workgroup partials +
    a parallel fixed-order reduction turned out faster than fp32 atomics); the call is kept for its callers, records the flag and
    returns the previous value."""
    return bool(_lib.lib().mvnerf_set_deterministic(int(bool(on))))


def adam_clip(param, grad, m, v, lr_t, beta1=0.9, beta2=0.999, eps=1e-7, clip=1.0, update_mask=None):
    """optimize() (nerf_utils.py:8-12): clip-by-value then Adam, in place on `param`, `m`, `v`."""
    _chk(param, 'param')
    for t, n in ((grad, 'grad'), (m, 'm'), (v, 'v')):
        _chk(t, n, shape=tuple(param.shape))
    if update_mask is not None:
        _chk(update_mask, 'update_mask', dtype=torch.uint8, shape=tuple(param.shape))
    with torch.cuda.device(param.device):
        rc = _lib.lib().mvnerf_adam_clip(_p(param), _p(grad), _p(m), _p(v), param.numel(), float(lr_t), float(beta1),
                                         float(beta2), float(eps), float(clip), _p(update_mask), _stream(param))
    _lib.check(rc, 'adam_clip')


# ---- bf16 variant of the field pass (configs 3 / 5) ---------------------------------------------------------
def pack_net_bf16(net_keras):
    """Keras-order fp32 MLP -> bf16 MFMA operand stream (uint8 tensor of mvnerf_packed_net_bf16_bytes())."""
    _chk(net_keras, 'net_keras', shape=(NET_PARAMS,))
    out = torch.empty(int(_lib.lib().mvnerf_packed_net_bf16_bytes()), dtype=torch.uint8, device=net_keras.device)
    with torch.cuda.device(net_keras.device):
        _lib.check(_lib.lib().mvnerf_pack_net_bf16(_p(net_keras), _p(out), _stream(net_keras)), 'pack_net_bf16')
    return out


def project_texels_bf16(features, packed16, out=None, packed16_b=None):
    """mvnerf_project_texels_bf16: the texel table of one net on the bf16 MFMA (fp32 table, same layout as project_texels);
    with packed16_b both nets' tables (2,B,V,H,W,128) from one read of the feature maps.
    features: fp32, or bfloat16 (B,V,H,W,256) -> mvnerf_project_texels_bf16maps (half the bytes of the pass)."""
    maps16 = isinstance(features, torch.Tensor) and features.dtype == torch.bfloat16
    _chk(features, 'features', dtype=torch.bfloat16 if maps16 else torch.float32, shape=(None, None, None, None, 256))
    b, v, h, w, _ = features.shape
    nbytes = int(_lib.lib().mvnerf_packed_net_bf16_bytes())
    _chk(packed16, 'packed16', dtype=torch.uint8, shape=(nbytes,))
    shape = (b, v, h, w, 128) if packed16_b is None else (2, b, v, h, w, 128)
    if packed16_b is not None:
        _chk(packed16_b, 'packed16_b', dtype=torch.uint8, shape=(nbytes,))
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=features.device)
    else:
        _chk(out, 'texel_table', shape=shape)
    t0, t1 = (out, None) if packed16_b is None else (out[0], out[1])
    with torch.cuda.device(features.device):
        fn = _lib.lib().mvnerf_project_texels_bf16maps if maps16 else _lib.lib().mvnerf_project_texels_bf16
        rc = fn(_p(features), _p(packed16), _p(packed16_b), b, v, h, w, _p(t0), _p(t1), _stream(features))
    _lib.check(rc, 'project_texels_bf16')
    return out


def field_eval_bf16(rays_o, rays_d, z, images, features, intrinsics, extrinsics_inv, packed_net, packed16, return_taps=False,
                    return_embedding=False, return_fused_acts=False, texel_table=None):
    """mvnerf_field_eval_bf16: as field_eval with the Dense layers on the bf16 MFMA path.
    return_fused_acts: + (4,B,R,S,128) = view mean and the three fusion blocks (complete_output[4:]).
    features: fp32, or bfloat16 (B,V,H,W,256) -> mvnerf_field_eval_bf16maps (the gather reads bf16 texel rows)."""
    maps16 = isinstance(features, torch.Tensor) and features.dtype == torch.bfloat16
    fn = _lib.lib().mvnerf_field_eval_bf16maps if maps16 else _lib.lib().mvnerf_field_eval_bf16
    return _field_pass('field_eval_bf16', fn, rays_o, rays_d, z, (images, features, intrinsics, extrinsics_inv), packed_net,
                       second=(packed16, 'packed16', int(_lib.lib().mvnerf_packed_net_bf16_bytes())), texel_table=texel_table, wide=False,
                       features_dtype=torch.bfloat16 if maps16 else torch.float32, return_taps=return_taps,
                       return_embedding=return_embedding, return_fused_acts=return_fused_acts)


def _render_two_pass(field, build_tables, features, u_coarse, u_fine, near, far, q7_mode, texel_tables):
    """`_call` (model_v0.py:113-184) as two field passes around the fp32 sampling, compositing and resampling.
    field(z, k, texel_table) -> rgbs of net k (0 coarse, 1 fine); build_tables(out) fills and returns both nets' tables."""
    tab_c = tab_f = None
    b, r, s = u_coarse.shape
    texel_tables = _auto_texel_tables(texel_tables, tuple(features.shape[:4]), r, s, features.device)
    if texel_tables is not None:
        tab_c, tab_f = build_tables(texel_tables).unbind(0)
    z = stratified_depths(u_coarse, near, far)
    rgbs_c = field(z, 0, tab_c)
    rgb, depth, w = composite(z, rgbs_c)
    z_all = resample(z, w, u_fine, q7_mode)
    rgbs_f = field(z_all, 1, tab_f)
    fine_rgb, fine_depth, _ = composite(z_all, rgbs_f, return_weights=False)
    return rgb, depth, fine_rgb, fine_depth


def render_fwd_bf16(rays_o, rays_d, images, features, intrinsics, extrinsics_inv, packed_coarse, packed_fine, packed16_coarse,
                    packed16_fine, u_coarse, u_fine, near, far, q7_mode=Q7_ZERO, texel_tables='auto'):
    """`_call` with both field passes on the bf16 path (sampling, compositing and resampling stay fp32).
    texel_tables: 'auto' (build the two fp32 tables when texel_table_pays), None, or a (2,B,V,H,W,128) tensor to fill."""
    geo = (images, features, intrinsics, extrinsics_inv)
    nets, nets16 = (packed_coarse, packed_fine), (packed16_coarse, packed16_fine)
    return _render_two_pass(lambda z, k, tab: field_eval_bf16(rays_o, rays_d, z, *geo, nets[k], nets16[k], texel_table=tab),
                            lambda out: project_texels_bf16(features, packed16_coarse, out=out, packed16_b=packed16_fine),
                            features, u_coarse, u_fine, near, far, q7_mode, texel_tables)


# ---- fp32-grade field pass on the bf16 matrix pipe (three-piece operand split, csrc/field_eval_split.hip) ------------------
def pack_net_split(net_keras):
    """Keras-order fp32 MLP -> three-piece bf16 operand stream (uint8 tensor of mvnerf_packed_net_split_bytes())."""
    _chk(net_keras, 'net_keras', shape=(NET_PARAMS,))
    out = torch.empty(int(_lib.lib().mvnerf_packed_net_split_bytes()), dtype=torch.uint8, device=net_keras.device)
    with torch.cuda.device(net_keras.device):
        _lib.check(_lib.lib().mvnerf_pack_net_split(_p(net_keras), _p(out), _stream(net_keras)), 'pack_net_split')
    return out


def field_eval_split(rays_o, rays_d, z, images, features, intrinsics, extrinsics_inv, packed_net, packed_split, return_taps=False,
                     return_pix=False, return_embedding=False, complete_output=False, texel_table=None, kernel=None, range_status=None):
    """mvnerf_field_eval_split: field_eval (same outputs, same fp32 bar) with the Dense layers as split-bf16 MFMA products.
    texel_table: project_texels(features, packed_net) of the same net (fp32).
    kernel: None (the process-wide choice, set_split_kernel) or a SPLIT_KERNELS name for this call only.
    range_status: None, or one device float the caller has zeroed: the 'split_f16' kernel then runs range-guarded and max-accumulates
    the largest |activation| it cuts into fp16 pieces (compare with F16X3_MAX_ACT; reading it is the caller's synchronisation).
    With both left at None the plain entry point runs; otherwise mvnerf_field_eval_split_ex."""
    ex = _split_ex_args(kernel, range_status, 1)
    fn = _lib.lib().mvnerf_field_eval_split if ex is None else _lib.lib().mvnerf_field_eval_split_ex
    return _field_pass('field_eval_split', fn, rays_o, rays_d, z, (images, features, intrinsics, extrinsics_inv),
                       packed_net, second=(packed_split, 'packed_split', int(_lib.lib().mvnerf_packed_net_split_bytes())),
                       texel_table=texel_table, return_taps=return_taps, return_pix=return_pix, return_embedding=return_embedding,
                       complete_output=complete_output, extra=ex or ())


def render_fwd_split(rays_o, rays_d, images, features, intrinsics, extrinsics_inv, packed_coarse, packed_fine, split_coarse,
                     split_fine, u_coarse, u_fine, near, far, q7_mode=Q7_ZERO, texel_tables='auto'):
    """`_call` (model_v0.py:113-184) with both field passes on the split-bf16 kernel (fp32-grade products, 1e-4 bar).
    texel_tables: 'auto' (build the two fp32 tables when texel_table_pays), None, or a (2,B,V,H,W,128) tensor to fill."""
    geo = (images, features, intrinsics, extrinsics_inv)
    nets, splits = (packed_coarse, packed_fine), (split_coarse, split_fine)
    return _render_two_pass(lambda z, k, tab: field_eval_split(rays_o, rays_d, z, *geo, nets[k], splits[k], texel_table=tab),
                            lambda out: project_texels2(features, packed_coarse, packed_fine, out=out),
                            features, u_coarse, u_fine, near, far, q7_mode, texel_tables)


# ---- the trunk as a differentiable field on query points (lmvnerf/model_v4.py:208-265) -------------
def _query_shapes(points, dirs, images, features, intrinsics, extrinsics_inv):
    _chk(points, 'points', shape=(None, None, 3))
    b, n, _ = points.shape
    _chk(dirs, 'dirs', shape=(b, n, 3))
    _, v, h, w = _scene(images, features, intrinsics, extrinsics_inv, b=b)
    return b, v, n, h, w


def query_jvp(points, dirs, t_points, t_dirs, images, features, intrinsics, extrinsics_inv, packed_net, return_primal=False):
    """mvnerf_query_jvp: tangents (B,N,3) of the query points / directions -> tangents (4,B,N,128) of the four fused
    activations (view mean, u1, u2, u3) [+ the activations themselves]."""
    b, v, n, h, w = _query_shapes(points, dirs, images, features, intrinsics, extrinsics_inv)
    _chk(t_points, 't_points', shape=(b, n, 3))
    _chk(t_dirs, 't_dirs', shape=(b, n, 3))
    _chk(packed_net, 'packed_net', shape=(packed_net_floats(),))
    dev = points.device
    t_acts = torch.empty((4, b, n, 128), dtype=torch.float32, device=dev)
    acts = torch.empty((4, b, n, 128), dtype=torch.float32, device=dev) if return_primal else None
    ws = torch.empty(int(_lib.lib().mvnerf_query_workspace_bytes(b, v, n)), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        rc = _lib.lib().mvnerf_query_jvp(_p(points), _p(dirs), _p(t_points), _p(t_dirs), _p(images), _p(features), _p(intrinsics),
                                         _p(extrinsics_inv), _p(packed_net), b, v, n, h, w, _p(acts), _p(t_acts), _p(ws),
                                         _stream(points))
    _lib.check(rc, 'query_jvp')
    return (t_acts, acts) if return_primal else t_acts


def query_stash(points, dirs, images, features, intrinsics, extrinsics_inv, packed_net, stash=None, packed_split=None):
    """Forward of the trunk on query points with the pre-activations kept for query_vjp (field_eval_stash, S = 1, z = 0);
    packed_split: run it on the split-bf16 kernel."""
    z = torch.zeros(tuple(points.shape[:2]) + (1,), dtype=torch.float32, device=points.device)
    return field_eval_stash(points, dirs, z, images, features, intrinsics, extrinsics_inv, packed_net, stash, packed_split=packed_split)[1]


def stash_fused_acts(stash, b, v, n):
    """mvnerf_stash_fused_acts: the four fused activations of a query stash (query_stash on (b, n) points, v views) as (4, b, n, 128)."""
    _chk(stash, 'stash', dtype=torch.uint8)
    if stash.numel() < stash_bytes(b, v, n, 1):
        raise ValueError(f'stash: {stash.numel()} bytes, need {stash_bytes(b, v, n, 1)}')
    acts = torch.empty((4, b, n, 128), dtype=torch.float32, device=stash.device)
    with torch.cuda.device(stash.device):
        rc = _lib.lib().mvnerf_stash_fused_acts(_p(stash), b, v, n, _p(acts), _stream(stash))
    _lib.check(rc, 'stash_fused_acts')
    return acts


def query_vjp(points, dirs, images, features, intrinsics, extrinsics_inv, bwd_streams, stash, g_acts):
    """mvnerf_query_vjp: cotangents (4,B,N,128) of the four fused activations -> (d_points, d_dirs), each (B,N,3)."""
    b, v, n, h, w = _query_shapes(points, dirs, images, features, intrinsics, extrinsics_inv)
    _chk(g_acts, 'g_acts', shape=(4, b, n, 128))
    _chk(bwd_streams, 'bwd_streams', shape=(15 * 16384,))
    _chk(stash, 'stash', dtype=torch.uint8)
    if stash.numel() < stash_bytes(b, v, n, 1):
        raise ValueError(f'stash: {stash.numel()} bytes, need {stash_bytes(b, v, n, 1)}')
    dev = points.device
    d_points = torch.empty((b, n, 3), dtype=torch.float32, device=dev)
    d_dirs = torch.empty((b, n, 3), dtype=torch.float32, device=dev)
    scratch = torch.empty(int(_lib.lib().mvnerf_query_vjp_scratch_bytes(b, v, n)), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        rc = _lib.lib().mvnerf_query_vjp(_p(points), _p(dirs), _p(images), _p(features), _p(intrinsics), _p(extrinsics_inv),
                                         _p(bwd_streams), _p(stash), _p(g_acts), b, v, n, h, w, _p(scratch), _p(d_points),
                                         _p(d_dirs), _stream(points))
    _lib.check(rc, 'query_vjp')
    return d_points, d_dirs


# ---- the same field on the bf16 matrix pipe: relu bits instead of a stash, one backward launch (csrc/query_bf16.hip) ----
def relu_bits_bytes(b, v, n):
    return int(_lib.lib().mvnerf_relu_bits_bytes(b, v, n))


def pack_bwd_streams_bf16(net_keras):
    """mvnerf_pack_bwd_streams_bf16: the twelve hidden kernels transposed and rounded to bf16, in the order the backward walk reads them
    (uint8 tensor of mvnerf_bwd_streams_bf16_bytes())."""
    _chk(net_keras, 'net_keras', shape=(NET_PARAMS,))
    out = torch.empty(int(_lib.lib().mvnerf_bwd_streams_bf16_bytes()), dtype=torch.uint8, device=net_keras.device)
    with torch.cuda.device(net_keras.device):
        _lib.check(_lib.lib().mvnerf_pack_bwd_streams_bf16(_p(net_keras), _p(out), _stream(net_keras)), 'pack_bwd_streams_bf16')
    return out


def _chk_bytes(t, name, nbytes):
    _chk(t, name, dtype=torch.uint8)
    if t.numel() < nbytes:
        raise ValueError(f'{name}: {t.numel()} bytes, need {nbytes}')
    return t


def query_stash_bf16(points, dirs, images, features, intrinsics, extrinsics_inv, packed_net, packed16, relu_bits=None):
    """mvnerf_query_stash_bf16: the trunk on query points with its hidden layers on the bf16 MFMA -> (acts (4,B,N,128) = view mean, u1, u2,
    u3; relu_bits: one bit per pre-activation, what trunk_vjp_bf16 / query_vjp_bf16 need of this forward)."""
    b, v, n, h, w = _query_shapes(points, dirs, images, features, intrinsics, extrinsics_inv)
    _chk(packed_net, 'packed_net', shape=(packed_net_floats(),))
    _chk(packed16, 'packed16', dtype=torch.uint8, shape=(int(_lib.lib().mvnerf_packed_net_bf16_bytes()),))
    dev = points.device
    if relu_bits is None:
        relu_bits = torch.empty(relu_bits_bytes(b, v, n), dtype=torch.uint8, device=dev)
    else:
        _chk_bytes(relu_bits, 'relu_bits', relu_bits_bytes(b, v, n))
    acts = torch.empty((4, b, n, 128), dtype=torch.float32, device=dev)
    ws = torch.empty(int(_lib.lib().mvnerf_query_workspace_bytes(b, v, n)), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        rc = _lib.lib().mvnerf_query_stash_bf16(_p(points), _p(dirs), _p(images), _p(features), _p(intrinsics), _p(extrinsics_inv),
                                                _p(packed_net), _p(packed16), b, v, n, h, w, _p(acts), _p(relu_bits), _p(ws), _stream(points))
    _lib.check(rc, 'query_stash_bf16')
    return acts, relu_bits


def unpack_relu_bits(bits, b, v, n):
    """relu_bits of query_stash_bf16 on (b, n) points, v views -> bool (b, 6 v + 6, n, 128) in feature order: per view x0, h1, x1, h2, x2,
    h3, then mean, h4, x4, h5, x5, h6 (the layout: include/mvnerf_hip.h).  For tests; any device."""
    if bits.dtype != torch.uint8 or bits.numel() < (-(-b * n // 32)) * (v + 1) * 6 * 512:
        raise ValueError('bits: expected the uint8 tensor of query_stash_bf16 for these sizes')
    if v > 1 and n % 32:
        raise ValueError(f'n = {n} must be a multiple of 32 when v > 1')
    n_tiles = -(-b * n // 32)
    words = bits[:n_tiles * (v + 1) * 6 * 512].view(torch.int64).reshape(-1, 6, 2, 32)              # [tile][slot][h][j]
    k = torch.arange(64, device=bits.device)
    on = ((words[..., None] >> k) & 1).bool().reshape(-1, 6, 2, 32, 4, 4, 4)                          # ... [nb][q][c]: bit 16 nb + 4 q + c
    rows = on.permute(0, 1, 3, 4, 5, 2, 6).reshape(-1, 6, 32, 128)                                    # feature 32 nb + 8 q + 4 h + c
    view, fused = rows[:n_tiles * v], rows[n_tiles * v:]
    if v == 1:                                             # tiles run over the flat b * n points
        flat = lambda t: t.permute(1, 0, 2, 3).reshape(6, -1, 128)[:, :b * n].reshape(6, b, n, 128).permute(1, 0, 2, 3)
        return torch.cat([flat(view), flat(fused)], 1).contiguous()
    view = view.reshape(b, v, n // 32, 6, 32, 128).permute(0, 1, 3, 2, 4, 5).reshape(b, v * 6, n, 128)
    fused = fused.reshape(b, n // 32, 6, 32, 128).permute(0, 2, 1, 3, 4).reshape(b, 6, n, 128)
    return torch.cat([view, fused], 1).contiguous()


def trunk_vjp_bf16(bwd16, relu_bits, g_acts, v):
    """mvnerf_trunk_vjp_bf16: cotangents (4,B,N,128) -> g0 (view tiles, 128, 32) = dL/d(layer-0 output) in tile layout: the twelve
    hidden layers' backward as one launch on the bf16 MFMA."""
    _chk(g_acts, 'g_acts', shape=(4, None, None, 128))
    _, b, n, _ = g_acts.shape
    _chk(bwd16, 'bwd16', dtype=torch.uint8, shape=(int(_lib.lib().mvnerf_bwd_streams_bf16_bytes()),))
    _chk_bytes(relu_bits, 'relu_bits', relu_bits_bytes(b, v, n))
    g0 = torch.empty((-(-b * n // 32) * v, 128, 32), dtype=torch.float32, device=g_acts.device)
    with torch.cuda.device(g_acts.device):
        rc = _lib.lib().mvnerf_trunk_vjp_bf16(_p(bwd16), _p(relu_bits), _p(g_acts), b, v, n, _p(g0), _stream(g_acts))
    _lib.check(rc, 'trunk_vjp_bf16')
    return g0


def query_vjp_bf16(points, dirs, images, features, intrinsics, extrinsics_inv, bwd_streams, bwd16, relu_bits, g_acts):
    """mvnerf_query_vjp_bf16: cotangents (4,B,N,128) -> (d_points, d_dirs), each (B,N,3): trunk_vjp_bf16, then the fp32 layer-0 pass of
    query_vjp (bwd_streams: pack_bwd_streams, its layer-0 slabs)."""
    b, v, n, h, w = _query_shapes(points, dirs, images, features, intrinsics, extrinsics_inv)
    _chk(g_acts, 'g_acts', shape=(4, b, n, 128))
    _chk(bwd_streams, 'bwd_streams', shape=(15 * 16384,))
    _chk(bwd16, 'bwd16', dtype=torch.uint8, shape=(int(_lib.lib().mvnerf_bwd_streams_bf16_bytes()),))
    _chk_bytes(relu_bits, 'relu_bits', relu_bits_bytes(b, v, n))
    dev = points.device
    d_points = torch.empty((b, n, 3), dtype=torch.float32, device=dev)
    d_dirs = torch.empty((b, n, 3), dtype=torch.float32, device=dev)
    scratch = torch.empty(int(_lib.lib().mvnerf_query_vjp_bf16_scratch_bytes(b, v, n)), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        rc = _lib.lib().mvnerf_query_vjp_bf16(_p(points), _p(dirs), _p(images), _p(features), _p(intrinsics), _p(extrinsics_inv),
                                              _p(bwd_streams), _p(bwd16), _p(relu_bits), _p(g_acts), b, v, n, h, w, _p(scratch),
                                              _p(d_points), _p(d_dirs), _stream(points))
    _lib.check(rc, 'query_vjp_bf16')
    return d_points, d_dirs


# ---- the grasp-pose optimiser's pose side (csrc/pose_ops.hip; lmvnerf/grasp_optimizer.py:113-184, utils/optimization.py:40-69) ---------
POSE_REPS = {4: 0, 6: 1}          # rotation width -> rep (0 quaternion x y z w, 1 6d)


def _rot_shape(rot):
    _chk(rot, 'rot')
    if rot.dim() not in (2, 3) or rot.shape[-1] not in POSE_REPS or (rot.dim() == 3 and rot.shape[0] != 1):
        raise ValueError(f'rot: shape {tuple(rot.shape)}, expected (P, 4|6) or (1, P, 4|6)')
    return rot.shape[-2], POSE_REPS[rot.shape[-1]], rot.shape[-1]


def _pose_shapes(t, rot):
    _chk(t, 't')
    _chk(rot, 'rot')
    if t.dim() not in (2, 3) or t.shape[-1] != 3 or (t.dim() == 3 and t.shape[0] != 1):
        raise ValueError(f't: shape {tuple(t.shape)}, expected (P, 3) or (1, P, 3)')
    p = t.shape[-2]
    if rot.dim() != t.dim() or rot.shape[-1] not in POSE_REPS or rot.numel() != p * rot.shape[-1]:
        raise ValueError(f'rot: shape {tuple(rot.shape)}, expected (P, 4) or (P, 6) with P = {p}')
    return p, POSE_REPS[rot.shape[-1]], rot.shape[-1]


def pose_query_points(t, rot, offsets, n_scenes=1, ld=None, out=None):
    """mvnerf_pose_query_points: poses -> (points, dirs), each (n_scenes, ld, 3), rows p * n5 + o (ld defaults to P * n5; rows past P * n5
    are not written).  out: a (points, dirs) pair to write into."""
    p, rep, _ = _pose_shapes(t, rot)
    _chk(offsets, 'offsets', shape=(None, 4, 4))
    n5 = offsets.shape[0]
    ld = p * n5 if ld is None else int(ld)
    if out is None:
        out = tuple(torch.empty((n_scenes, ld, 3), dtype=torch.float32, device=t.device) for _ in range(2))
    points, dirs = out
    _chk(points, 'points', shape=(n_scenes, ld, 3))
    _chk(dirs, 'dirs', shape=(n_scenes, ld, 3))
    with torch.cuda.device(t.device):
        rc = _lib.lib().mvnerf_pose_query_points(_p(t), _p(rot), rep, _p(offsets), p, n5, int(n_scenes), ld, _p(points), _p(dirs), _stream(t))
    _lib.check(rc, 'pose_query_points')
    return points, dirs


def pose_query_vjp(rot, offsets, d_points, d_dirs, scale=1.0, out=None):
    """mvnerf_pose_query_vjp: (d_points, d_dirs) (B, ld, 3) -> scale * (d_t (P, 3), d_rot (P, 4|6)), fixed-order sums."""
    p, rep, rd = _rot_shape(rot)
    _chk(offsets, 'offsets', shape=(None, 4, 4))
    n5 = offsets.shape[0]
    _chk(d_points, 'd_points', shape=(None, None, 3))
    b, ld, _ = d_points.shape
    _chk(d_dirs, 'd_dirs', shape=(b, ld, 3))
    if out is None:
        out = (torch.empty((p, 3), dtype=torch.float32, device=rot.device), torch.empty((p, rd), dtype=torch.float32, device=rot.device))
    d_t, d_rot = out
    _chk(d_t, 'd_t', shape=(p, 3))
    _chk(d_rot, 'd_rot', shape=(p, rd))
    with torch.cuda.device(rot.device):
        rc = _lib.lib().mvnerf_pose_query_vjp(_p(rot), rep, _p(offsets), _p(d_points), _p(d_dirs), p, n5, b, ld, float(scale), _p(d_t),
                                              _p(d_rot), _stream(rot))
    _lib.check(rc, 'pose_query_vjp')
    return d_t, d_rot


def pose_query_jvp(rot, offsets, c_t, c_rot, n_scenes=1, ld=None, out=None):
    """mvnerf_pose_query_jvp: tangents (c_t (P, 3), c_rot (P, 4|6)) of the poses -> (t_points, t_dirs), each (n_scenes, ld, 3), rows
    p * n5 + o (rows past P * n5 are not written).  out: a (t_points, t_dirs) pair to write into."""
    p, rep, rd = _rot_shape(rot)
    _chk(offsets, 'offsets', shape=(None, 4, 4))
    n5 = offsets.shape[0]
    _chk(c_t, 'c_t', shape=(p, 3))
    _chk(c_rot, 'c_rot', shape=(p, rd))
    ld = p * n5 if ld is None else int(ld)
    if out is None:
        out = tuple(torch.empty((n_scenes, ld, 3), dtype=torch.float32, device=rot.device) for _ in range(2))
    t_points, t_dirs = out
    _chk(t_points, 't_points', shape=(n_scenes, ld, 3))
    _chk(t_dirs, 't_dirs', shape=(n_scenes, ld, 3))
    with torch.cuda.device(rot.device):
        rc = _lib.lib().mvnerf_pose_query_jvp(_p(rot), rep, _p(offsets), _p(c_t), _p(c_rot), p, n5, int(n_scenes), ld, _p(t_points), _p(t_dirs),
                                              _stream(rot))
    _lib.check(rc, 'pose_query_jvp')
    return t_points, t_dirs


# ---- the LanguageNeRF training step behind the C ABI (csrc/language_ops.hip, language_api.hip; lmvnerf/model_v4.py:277-318) ----------------
LANGUAGE_LOSSES = {'kl_divergence': 0, 'cross_entropy': 1}


def landscape_loss(y, label, kind, weight=1.0):
    """mvnerf_landscape_loss: predicted success y (B, np) against label -> (loss (1,) = the mean over the batch, g_y (B, np))."""
    _chk(y, 'y', shape=(None, None))
    b, n_p = y.shape
    _chk(label, 'label', shape=(b, n_p))
    g_y = torch.empty_like(y)
    loss = torch.empty(1, dtype=torch.float32, device=y.device)
    with torch.cuda.device(y.device):
        rc = _lib.lib().mvnerf_landscape_loss(_p(y), _p(label), b, n_p, LANGUAGE_LOSSES[kind], float(weight), _p(g_y), _p(loss), _stream(y))
    _lib.check(rc, 'landscape_loss')
    return loss, g_y


def cosine_loss(x, label, scale=1.0):
    """mvnerf_cosine_loss: x, label (..., 3|4|6) (6: the two 3-halves separately, added) -> (loss (1,), g_x = scale * d loss / d x)."""
    _chk(x, 'x')
    dim = x.shape[-1]
    _chk(label, 'label', shape=tuple(x.shape))
    g_x = torch.empty_like(x)
    loss = torch.empty(1, dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        rc = _lib.lib().mvnerf_cosine_loss(_p(x), _p(label), x.numel() // max(dim, 1), dim, float(scale), _p(g_x), _p(loss), _stream(x))
    _lib.check(rc, 'cosine_loss')
    return loss, g_x


def language_grad_layout(n5):
    """name -> (offset, shape) of every read-out variable inside the flat gradient of mvnerf_language_loss_and_grads (include/mvnerf_hip.h)."""
    k = 64 * n5
    shapes = (('w4', (4, 64, 128)), ('b4', (4, 64)), ('wc', (64, 256)), ('bc', (64,)), ('w0', (128, k)), ('b0', (128,)), ('w1', (64, 128)),
              ('b1', (64,)), ('ws', (64, k)), ('w0b', (64, 64)), ('w1b', (64, 64)), ('b0b', (64,)), ('b1b', (64,)), ('w_out', (1, 64)),
              ('b_out', (1,)))
    layout, at = {}, 0
    for name, shape in shapes:
        layout[name] = (at, shape)
        at += int(np.prod(shape))
    if at != int(_lib.lib().mvnerf_language_grad_floats(int(n5))):
        raise RuntimeError('language_grad_layout disagrees with mvnerf_language_grad_floats')
    return layout, at


def language_workspace_bytes(b, v, h, w, n_p, n5):
    return int(_lib.lib().mvnerf_language_workspace_bytes(int(b), int(v), int(h), int(w), int(n_p), int(n5)))


_TAIL_ORDER = ('w0', 'b0', 'w1', 'b1', 'ws', 'w0b', 'b0b', 'w1b', 'b1b', 'w_out', 'b_out')


def language_call(images, features, intrinsics, extrinsics_inv, packed_net, split, bwd_streams, head, tail, offsets, poses, labels, loss_kind,
                  loss_weights, grads, prediction, scalars, workspace):
    """Fill a mvnerf_language_call (include/mvnerf_hip.h) from device tensors after checking shapes; the caller keeps the tensors alive.
    head = (w4 (4,64,128), b4 (4,64), wc (64,256), bc (64,)); tail = the 11 tensors of grasp_tail_pack in its order; poses = (t_landscape,
    rot_landscape, t_grad, rot_grad), each (B, np, .); labels = (landscape (B, np), grad_t (B, np, 3), grad_r (B, np, 4|6))."""
    b, v, h, w = _scene(images, features, intrinsics, extrinsics_inv)
    _chk(packed_net, 'packed_net', shape=(packed_net_floats(),))
    _chk(split, 'split', dtype=torch.uint8, shape=(int(_lib.lib().mvnerf_packed_net_split_bytes()),))
    _chk(bwd_streams, 'bwd_streams', shape=(15 * 16384,))
    _chk(offsets, 'offsets', shape=(None, 4, 4))
    n5 = offsets.shape[0]
    k = 64 * n5
    for t, name, shape in zip(head, ('w4', 'b4', 'wc', 'bc'), ((4, 64, 128), (4, 64), (64, 256), (64,))):
        _chk(t, 'head ' + name, shape=shape)
    tail_shapes = ((128, k), (128,), (64, 128), (64,), (64, k), (64, 64), (64,), (64, 64), (64,), None, (1,))
    if len(tail) != 11:
        raise ValueError('tail: the 11 tensors of grasp_tail_pack')
    for t, name, shape in zip(tail, _TAIL_ORDER, tail_shapes):
        _chk(t, 'tail ' + name, shape=shape)
    if tail[9].numel() != 64:
        raise ValueError(f'tail w_out: shape {tuple(tail[9].shape)}, expected (1, 64)')
    t_l, r_l, t_g, r_g = poses
    _chk(t_l, 't_landscape', shape=(b, None, 3))
    n_p = t_l.shape[1]
    rd = r_l.shape[-1]
    if rd not in POSE_REPS:
        raise ValueError(f'rot_landscape: shape {tuple(r_l.shape)}, expected (B, np, 4|6)')
    _chk(r_l, 'rot_landscape', shape=(b, n_p, rd))
    _chk(t_g, 't_grad', shape=(b, n_p, 3))
    _chk(r_g, 'rot_grad', shape=(b, n_p, rd))
    _chk(labels[0], 'label_landscape', shape=(b, n_p))
    _chk(labels[1], 'label_grad_t', shape=(b, n_p, 3))
    _chk(labels[2], 'label_grad_r', shape=(b, n_p, rd))
    _chk(grads, 'grads', shape=(int(_lib.lib().mvnerf_language_grad_floats(n5)),))
    _chk(prediction, 'prediction', shape=(b, n_p))
    _chk(scalars, 'scalars', shape=(4,))
    _chk(workspace, 'workspace', dtype=torch.uint8)
    c = _lib.LanguageCall()
    for name, x in (('images', images), ('features', features), ('intrinsics', intrinsics), ('extrinsics_inv', extrinsics_inv),
                    ('packed_net', packed_net), ('split', split), ('bwd_streams', bwd_streams), ('head_w4', head[0]), ('head_b4', head[1]),
                    ('head_wc', head[2]), ('head_bc', head[3]), ('offsets', offsets), ('t_landscape', t_l), ('rot_landscape', r_l),
                    ('t_grad', t_g), ('rot_grad', r_g), ('label_landscape', labels[0]), ('label_grad_t', labels[1]),
                    ('label_grad_r', labels[2]), ('grads', grads), ('prediction', prediction), ('scalars', scalars), ('workspace', workspace)):
        setattr(c, name, x.data_ptr())
    for i, t in enumerate(tail):
        c.tail_w[i] = t.data_ptr()
    c.B, c.V, c.H, c.W = b, v, h, w
    c.rep, c.np, c.n5 = POSE_REPS[rd], n_p, n5
    c.loss_kind = LANGUAGE_LOSSES[loss_kind] if isinstance(loss_kind, str) else int(loss_kind)
    c.w_land, c.w_t, c.w_r = (float(x) for x in loss_weights)
    c.workspace_bytes = workspace.numel()
    return c


def language_loss_and_grads(call, stream_of):
    """mvnerf_language_loss_and_grads on a filled language_call -> its grads, prediction, scalars."""
    with torch.cuda.device(stream_of.device):
        _lib.check(_lib.lib().mvnerf_language_loss_and_grads(ctypes.byref(call), _stream(stream_of)), 'language_loss_and_grads')


def language_adam_state(head_w, head_b, head_wc, head_bc, tail, w4, b4, m, v, step, lr, beta1=0.9, beta2=0.999, eps=1e-7, clip=1.0):
    """Fill a mvnerf_language_adam (include/mvnerf_hip.h) from device tensors; the caller keeps them alive.  head_w / head_b: the four
    activation_downscale weights (64, 128) / biases (64,), the variables themselves; tail: the 11 tensors of language_call's `tail`; w4,
    b4: the stacked images language_call's `head` holds; m, v: flat, the size and layout of the gradient; step: one int64 on the device
    (completed updates).  lr is the plain rate: the bias correction is formed on the device from `step`."""
    if len(head_w) != 4 or len(head_b) != 4:
        raise ValueError('head_w, head_b: the four activation_downscale layers')
    for k in range(4):
        _chk(head_w[k], f'head_w[{k}]', shape=(64, 128))
        _chk(head_b[k], f'head_b[{k}]', shape=(64,))
    _chk(head_wc, 'head_wc', shape=(64, 256))
    _chk(head_bc, 'head_bc', shape=(64,))
    if len(tail) != 11:
        raise ValueError('tail: the 11 tensors of grasp_tail_pack')
    n5 = tail[0].shape[-1] // 64 if isinstance(tail[0], torch.Tensor) and tail[0].dim() == 2 else 0
    k = 64 * n5
    for t, name, shape in zip(tail, _TAIL_ORDER, ((128, k), (128,), (64, 128), (64,), (64, k), (64, 64), (64,), (64, 64), (64,), None, (1,))):
        _chk(t, 'tail ' + name, shape=shape)
    if n5 < 1 or tail[9].numel() != 64:
        raise ValueError(f'tail: w0 {tuple(tail[0].shape)}, w_out {tuple(tail[9].shape)}, expected (128, 64 n5) and (1, 64)')
    _chk(w4, 'w4', shape=(4, 64, 128))
    _chk(b4, 'b4', shape=(4, 64))
    total = int(_lib.lib().mvnerf_language_grad_floats(n5))
    _chk(m, 'm', shape=(total,))
    _chk(v, 'v', shape=(total,))
    _chk(step, 'step', dtype=torch.int64, shape=(1,))
    a = _lib.LanguageAdam()
    for i in range(4):
        a.head_w[i], a.head_b[i] = head_w[i].data_ptr(), head_b[i].data_ptr()
    for i, t in enumerate(tail):
        a.tail_w[i] = t.data_ptr()
    for name, x in (('head_wc', head_wc), ('head_bc', head_bc), ('head_w4', w4), ('head_b4', b4), ('m', m), ('v', v), ('step', step)):
        setattr(a, name, x.data_ptr())
    a.lr, a.beta1, a.beta2, a.eps, a.clip = float(lr), float(beta1), float(beta2), float(eps), float(clip)
    return a


def language_apply_gradients(call, adam, stream_of):
    """mvnerf_language_apply_gradients: clip + Keras Adam from call's grads on the variables of `adam`, in place; its step counter rises by one."""
    with torch.cuda.device(stream_of.device):
        _lib.check(_lib.lib().mvnerf_language_apply_gradients(ctypes.byref(call), ctypes.byref(adam), _stream(stream_of)), 'language_apply_gradients')


def language_train_step(call, adam, stream_of):
    """mvnerf_language_train_step: head gather, mvnerf_language_loss_and_grads, mvnerf_language_apply_gradients - LanguageNeRF.train_step."""
    with torch.cuda.device(stream_of.device):
        _lib.check(_lib.lib().mvnerf_language_train_step(ctypes.byref(call), ctypes.byref(adam), _stream(stream_of)), 'language_train_step')


def pose_adam_config(lr0=(0.09, 0.09), decay=(1.0, 1.0), beta1=0.9, beta2=0.999, eps=1e-7, clip=1.0, clip_translation=False, bounds=None):
    """mvnerf_pose_adam_config: lr0 / decay per variable (translations, rotations); bounds (3, 2) = workspace_bounds."""
    bounds = np.zeros((3, 2)) if bounds is None else np.asarray(bounds, dtype=np.float64).reshape(3, 2)
    c = _lib.PoseAdamConfig()
    c.lr0[0], c.lr0[1] = float(lr0[0]), float(lr0[1])
    c.decay[0], c.decay[1] = float(decay[0]), float(decay[1])
    c.beta1, c.beta2, c.eps, c.clip = float(beta1), float(beta2), float(eps), float(clip)
    c.clip_translation = int(bool(clip_translation))
    for i in range(3):
        c.lo[i], c.hi[i] = float(bounds[i, 0]), float(bounds[i, 1])
    return c


def pose_adam_step(cfg, train_flags, counters, g_t, g_rot, m_t, v_t, m_r, v_r, t, rot):
    """mvnerf_pose_adam_step: clip, Keras Adam with the decayed rate from the device-side counters (2, P) int32 of the variables that
    train_flags (2,) int32 marks, post_process; in place on t, rot, m_*, v_*, counters."""
    p, rep, rd = _pose_shapes(t, rot)
    _chk(train_flags, 'train_flags', dtype=torch.int32, shape=(2,))
    _chk(counters, 'counters', dtype=torch.int32, shape=(2, p))
    for x, n in ((g_t, 'g_t'), (m_t, 'm_t'), (v_t, 'v_t')):
        _chk(x, n)
        if x.numel() != 3 * p:
            raise ValueError(f'{n}: {x.numel()} floats, expected {3 * p}')
    for x, n in ((g_rot, 'g_rot'), (m_r, 'm_r'), (v_r, 'v_r')):
        _chk(x, n)
        if x.numel() != rd * p:
            raise ValueError(f'{n}: {x.numel()} floats, expected {rd * p}')
    with torch.cuda.device(t.device):
        rc = _lib.lib().mvnerf_pose_adam_step(ctypes.byref(cfg), rep, p, _p(train_flags), _p(counters), _p(g_t), _p(g_rot), _p(m_t),
                                              _p(v_t), _p(m_r), _p(v_r), _p(t), _p(rot), _stream(t))
    _lib.check(rc, 'pose_adam_step')


FUSE_ACTIVATIONS = {None: 0, 'identity': 0, 'relu': 1, 'elu': 2}


def fuse_upsample2x(a, b, weight, act, out_dtype=torch.float32, out=None):
    """mvnerf_fuse_upsample2x: a (N,h,w,Ca), b (N,h,w,Cb) fp32 NHWC, weight (Ca+Cb,256) (the Keras 1x1 kernel as stored) ->
    bilinear_x2(act([a | b]) . weight) as (N,2h,2w,256) NHWC in fp32 or bf16; act: 0 | 'identity', 1 | 'relu', 2 | 'elu'."""
    _chk(a, 'a', shape=(None, None, None, None))
    n, h, w, ca = a.shape
    _chk(b, 'b', shape=(n, h, w, None))
    cb = b.shape[3]
    _chk(weight, 'weight', shape=(ca + cb, 256))
    if out_dtype not in (torch.float32, torch.bfloat16):
        raise ValueError(f'out_dtype: {out_dtype}, expected torch.float32 or torch.bfloat16')
    if not isinstance(act, int):
        if act not in FUSE_ACTIVATIONS:
            raise ValueError(f'act: {act!r}, expected one of {list(FUSE_ACTIVATIONS)} or 0, 1, 2')
        act = FUSE_ACTIVATIONS[act]
    if out is None:
        out = torch.empty((n, 2 * h, 2 * w, 256), dtype=out_dtype, device=a.device)
    else:
        _chk(out, 'out', dtype=out_dtype, shape=(n, 2 * h, 2 * w, 256))
    with torch.cuda.device(a.device):
        rc = _lib.lib().mvnerf_fuse_upsample2x(_p(a), _p(b), _p(weight), n, h, w, ca, cb, int(act), _p(out),
                                               int(out_dtype == torch.bfloat16), _stream(a))
    _lib.check(rc, 'fuse_upsample2x')
    return out


def fuse_upsample2x_bwd(g, a, b, weight, act, need_a=True, need_b=True, need_g_low=False, out=None):
    """mvnerf_fuse_upsample2x_bwd: g = dL/dout (N,2h,2w,256) fp32 NHWC and the forward's a, b, weight, act -> (da | None, db | None,
    g_low | None): the gradients of a (N,h,w,Ca) and b (N,h,w,Cb), and the adjoint of the up-sampling g_low (N,h,w,256) that a weight
    gradient needs (dW = act([a | b])^T . g_low).  Only what the need flags ask for is computed.  out: None, or a (da, db, g_low) triple
    of buffers to write (None where not needed).  One launch, no atomics, no workspace."""
    _chk(a, 'a', shape=(None, None, None, None))
    n, h, w, ca = a.shape
    _chk(b, 'b', shape=(n, h, w, None))
    cb = b.shape[3]
    _chk(weight, 'weight', shape=(ca + cb, 256))
    _chk(g, 'g', shape=(n, 2 * h, 2 * w, 256))
    if not isinstance(act, int):
        if act not in FUSE_ACTIVATIONS:
            raise ValueError(f'act: {act!r}, expected one of {list(FUSE_ACTIVATIONS)} or 0, 1, 2')
        act = FUSE_ACTIVATIONS[act]
    needs = (bool(need_a), bool(need_b), bool(need_g_low))
    if not any(needs):
        raise ValueError('fuse_upsample2x_bwd: nothing asked for (need_a, need_b and need_g_low are all False)')
    shapes = ((n, h, w, ca), (n, h, w, cb), (n, h, w, 256))
    names = ('da', 'db', 'g_low')
    if out is None:
        out = (None, None, None)
    elif len(out) != 3:
        raise ValueError(f'out: expected a (da, db, g_low) triple, got {len(out)} entries')
    bufs = []
    for need, buf, shape, name in zip(needs, out, shapes, names):
        if not need:
            bufs.append(None)
        elif buf is None:
            bufs.append(torch.empty(shape, dtype=torch.float32, device=a.device))
        else:
            bufs.append(_chk(buf, f'out[{name}]', shape=shape))
    with torch.cuda.device(a.device):
        rc = _lib.lib().mvnerf_fuse_upsample2x_bwd(_p(g), _p(a), _p(b), _p(weight), n, h, w, ca, cb, int(act), _p(bufs[0]), _p(bufs[1]),
                                                   _p(bufs[2]), _stream(a))
    _lib.check(rc, 'fuse_upsample2x_bwd')
    return tuple(bufs)


def absmax(x, out=None):
    """mvnerf_absmax_f32: max |x| of a contiguous fp32 tensor as one device float (shape (1,)); a NaN in x gives a NaN.  No host read."""
    _chk(x, 'x')
    if x.numel() == 0:
        raise ValueError('x: empty tensor')
    if out is None:
        out = torch.empty(1, dtype=torch.float32, device=x.device)
    else:
        _chk(out, 'out', shape=(1,))
    with torch.cuda.device(x.device):
        rc = _lib.lib().mvnerf_absmax_f32(_p(x), x.numel(), _p(out), _stream(x))
    _lib.check(rc, 'absmax')
    return out


def conv3x3_packed_bytes(cin, cout):
    """Bytes of the packed stream of a (3,3,cin,cout) kernel (cin a multiple of 32, cout a multiple of 64; ValueError otherwise)."""
    n = _lib.lib().mvnerf_conv3x3_packed_bytes(int(cin), int(cout))
    if n == 0:
        raise ValueError(f'conv3x3: cin={cin} cout={cout} (cin a multiple of 32, cout a multiple of 64)')
    return n


def conv3x3_pack(w_hwio, out=None):
    """mvnerf_conv3x3_pack: w_hwio (3,3,cin,cout) fp32, the Keras kernel as stored -> the packed fp16-piece stream (uint8 tensor) that
    :func:`conv3x3` reads; max |w| and the scale are found on the device."""
    _chk(w_hwio, 'w_hwio', shape=(3, 3, None, None))
    cin, cout = w_hwio.shape[2:]
    nbytes = conv3x3_packed_bytes(cin, cout)
    if out is None:
        out = torch.empty(nbytes, dtype=torch.uint8, device=w_hwio.device)
    else:
        _chk(out, 'out', dtype=torch.uint8, shape=(nbytes,))
    with torch.cuda.device(w_hwio.device):
        rc = _lib.lib().mvnerf_conv3x3_pack(_p(w_hwio), cin, cout, _p(out), _stream(w_hwio))
    _lib.check(rc, 'conv3x3_pack')
    return out


def conv3x3(a, b, packed, cout, act, mul=None, amax_a=None, amax_b=None, out=None, amax_out=None, bias=None, act_in=None, stats=None):
    """mvnerf_conv3x3_nhwc: out (N,h,w,cout) = mul[n,co] * act(conv3x3_same([a | b], W)), bias-free, stride 1, zero padding.
    a (N,h,w,Ca), b (N,h,w,Cb) or None: fp32 NHWC; packed: :func:`conv3x3_pack` of the (3,3,Ca+Cb,cout) kernel; act: 0 | 'identity',
    1 | 'relu', 2 | 'elu'; mul (N,cout) or None.  amax_a / amax_b: device floats (1,) bounding |a| / |b| (computed with :func:`absmax`
    when missing); amax_out: a (1,) device float that receives max |out| (zeroed here).
    With any of the next three the call is mvnerf_conv3x3_nhwc_ex: bias (cout,) joins the sum before act; act_in (as act) is applied to
    the elements of a and b as they are read - |act_in(x)| <= |x|, so amax_a / amax_b of the plain maps stay valid, and the padding is
    zero after it; stats: True, or a float32 tensor of :func:`conv3x3_stats_bytes` / 4 elements, receives the per-tile (mean, M2) of what
    is written for :func:`bn_finalize` - the return value is then (out, stats)."""
    _chk(a, 'a', shape=(None, None, None, None))
    n, h, w, ca = a.shape
    cb = 0
    if b is not None:
        _chk(b, 'b', shape=(n, h, w, None))
        cb = b.shape[3]
    if not isinstance(act, int):
        if act not in FUSE_ACTIVATIONS:
            raise ValueError(f'act: {act!r}, expected one of {list(FUSE_ACTIVATIONS)} or 0, 1, 2')
        act = FUSE_ACTIVATIONS[act]
    if act_in is not None and not isinstance(act_in, int):
        if act_in not in FUSE_ACTIVATIONS:
            raise ValueError(f'act_in: {act_in!r}, expected one of {list(FUSE_ACTIVATIONS)} or 0, 1, 2')
        act_in = FUSE_ACTIVATIONS[act_in]
    act_in = int(act_in or 0)
    if not 0 <= act_in <= 2:
        raise ValueError(f'act_in: {act_in}, expected 0, 1 or 2')
    _chk(packed, 'packed', dtype=torch.uint8, shape=(conv3x3_packed_bytes(ca + cb, cout),))
    if mul is not None:
        _chk(mul, 'mul', shape=(n, cout))
    if bias is not None:
        _chk(bias, 'bias', shape=(cout,))
    if stats is True:
        stats = torch.empty(conv3x3_stats_bytes(n, h, w, cout) // 4, dtype=torch.float32, device=a.device)
    elif stats is not None and stats is not False:
        _chk(stats, 'stats', shape=(conv3x3_stats_bytes(n, h, w, cout) // 4,))
    else:
        stats = None
    if amax_a is None:
        amax_a = absmax(a)
    else:
        _chk(amax_a, 'amax_a', shape=(1,))
    if b is not None:
        if amax_b is None:
            amax_b = absmax(b)
        else:
            _chk(amax_b, 'amax_b', shape=(1,))
    elif amax_b is not None:
        raise ValueError('amax_b given without b')
    if out is None:
        out = torch.empty((n, h, w, cout), dtype=torch.float32, device=a.device)
    else:
        _chk(out, 'out', shape=(n, h, w, cout))
    if amax_out is not None:
        _chk(amax_out, 'amax_out', shape=(1,))
        amax_out.zero_()
    with torch.cuda.device(a.device):
        if bias is None and not act_in and stats is None:
            rc = _lib.lib().mvnerf_conv3x3_nhwc(_p(a), ca, _p(amax_a), _p(b), cb, _p(amax_b), _p(packed), n, h, w, int(cout), int(act), _p(mul),
                                                _p(out), _p(amax_out), _stream(a))
        else:
            rc = _lib.lib().mvnerf_conv3x3_nhwc_ex(_p(a), ca, _p(amax_a), _p(b), cb, _p(amax_b), _p(packed), n, h, w, int(cout), int(act),
                                                   _p(mul), _p(out), _p(amax_out), _p(bias), act_in, _p(stats), _stream(a))
    _lib.check(rc, 'conv3x3')
    return out if stats is None else (out, stats)


def conv3x3_stats_bytes(n, h, w, cout):
    """Bytes of the tile-statistics buffer of a (n,h,w,cout) convolution output (mvnerf_conv3x3_stats_bytes; ValueError when cout is not
    a multiple of 64 or a size is not positive)."""
    nbytes = _lib.lib().mvnerf_conv3x3_stats_bytes(int(n), int(h), int(w), int(cout))
    if nbytes == 0:
        raise ValueError(f'conv3x3 stats: n={n} h={h} w={w} cout={cout} (positive sizes, cout a multiple of 64)')
    return nbytes


# ---- backward of the biased 3x3 convolution (csrc/conv3x3_bwd.hip) ---------------------------------------------------------
CONV3X3_WGRAD_SLAB_PIXELS = 4096       # mvnerf_conv3x3_wgrad_slab_pixels(): 16 tiles of 16 x 16 pixels per slab of the reduction


def conv3x3_pack_transposed(w_hwio, out=None):
    """The packed stream of the data gradient's kernel W'[dy,dx,co,ci] = W[2-dy,2-dx,ci,co] of w_hwio (3,3,cin,cout): flipped and
    transposed on the device, then :func:`conv3x3_pack`.  `conv3x3(g, None, packed, cin, 0)` is then dL/d(act_in(x)) of
    y = conv3x3_same(act_in(x), W).  Needs cout a multiple of 32 and cin a multiple of 64 (ValueError otherwise)."""
    _chk(w_hwio, 'w_hwio', shape=(3, 3, None, None))
    return conv3x3_pack(w_hwio.flip(0, 1).transpose(2, 3).contiguous(), out=out)


def conv3x3_wgrad_workspace_bytes(n, h, w, cin, cout):
    """Bytes of the workspace of :func:`conv3x3_wgrad` (mvnerf_conv3x3_wgrad_workspace_bytes; ValueError for a shape it does not take)."""
    nbytes = _lib.lib().mvnerf_conv3x3_wgrad_workspace_bytes(int(n), int(h), int(w), int(cin), int(cout))
    if nbytes == 0:
        raise ValueError(f'conv3x3_wgrad: n={n} h={h} w={w} cin={cin} cout={cout} (positive sizes, cin a multiple of 32, cout a multiple of 64)')
    return nbytes


def conv3x3_wgrad(x, g, act_in=None, amax_x=None, amax_g=None, want_bias=False, workspace=None, out=None):
    """mvnerf_conv3x3_wgrad_nhwc: dw (3,3,cin,cout) HWIO = sum over the pixels of act_in(x) shifted by the tap times g, for
    y = conv3x3_same(act_in(x), W) + bias and g = dL/dy; with want_bias also dbias (cout,) = sum g, and the return value is (dw, dbias).
    x (N,h,w,cin), g (N,h,w,cout): fp32 NHWC.  act_in: None | 0 | 'identity', 1 | 'relu', 2 | 'elu'.  amax_x / amax_g: device floats (1,)
    bounding |x| / |g| (computed with :func:`absmax` when missing).  workspace: a uint8 tensor of at least
    :func:`conv3x3_wgrad_workspace_bytes` bytes, 16-byte aligned (allocated when missing); out: dw, or (dw, dbias) with want_bias."""
    _chk(x, 'x', shape=(None, None, None, None))
    n, h, w, cin = x.shape
    _chk(g, 'g', shape=(n, h, w, None))
    cout = g.shape[3]
    if act_in is not None and not isinstance(act_in, int):
        if act_in not in FUSE_ACTIVATIONS:
            raise ValueError(f'act_in: {act_in!r}, expected one of {list(FUSE_ACTIVATIONS)} or 0, 1, 2')
        act_in = FUSE_ACTIVATIONS[act_in]
    act_in = int(act_in or 0)
    if not 0 <= act_in <= 2:
        raise ValueError(f'act_in: {act_in}, expected 0, 1 or 2')
    nbytes = conv3x3_wgrad_workspace_bytes(n, h, w, cin, cout)
    if workspace is None:
        workspace = torch.empty(nbytes, dtype=torch.uint8, device=x.device)
    else:
        _chk(workspace, 'workspace', dtype=torch.uint8, shape=(None,))
        if workspace.numel() < nbytes:
            raise ValueError(f'workspace: {workspace.numel()} bytes, expected at least {nbytes}')
        if workspace.data_ptr() % 16:
            raise ValueError('workspace: must be 16-byte aligned')
    dw, dbias = (out if want_bias else (out, None)) if out is not None else (None, None)
    if dw is None:
        dw = torch.empty((3, 3, cin, cout), dtype=torch.float32, device=x.device)
    else:
        _chk(dw, 'out (dw)', shape=(3, 3, cin, cout))
    if want_bias:
        if dbias is None:
            dbias = torch.empty(cout, dtype=torch.float32, device=x.device)
        else:
            _chk(dbias, 'out (dbias)', shape=(cout,))
    for t, name in ((dw, 'out (dw)'), (dbias, 'out (dbias)'), (x, 'x'), (g, 'g')):
        if t is not None and t.data_ptr() % 16:
            raise ValueError(f'{name}: must be 16-byte aligned')
    if amax_x is None:
        amax_x = absmax(x)
    else:
        _chk(amax_x, 'amax_x', shape=(1,))
    if amax_g is None:
        amax_g = absmax(g)
    else:
        _chk(amax_g, 'amax_g', shape=(1,))
    with torch.cuda.device(x.device):
        rc = _lib.lib().mvnerf_conv3x3_wgrad_nhwc(_p(x), _p(amax_x), act_in, _p(g), _p(amax_g), n, h, w, cin, cout, _p(dw), _p(dbias),
                                                  _p(workspace), _stream(x))
    _lib.check(rc, 'conv3x3_wgrad')
    return (dw, dbias) if want_bias else dw


# ---- backward through a frozen 3x3 convolution of the language fusion (csrc/act_gate.hip) -----------------------------------
ACT_GATE_MAX_IMAGES = 65535


def act_gate(g, out, mul, act, out_d=None, amax_out=None):
    """mvnerf_act_gate_nhwc: d = g * mul * act'(y) for out = act(y) * mul as :func:`conv3x3` wrote it, from `out` and `mul` alone:
    where act(y) > 0 (out and mul of one sign) d = g * mul; else 0 for relu and g * (out + mul) for elu; mul == 0 gives exact zeros.
    g, out (N,h,w,C) fp32 NHWC with C a multiple of 4; mul (N,C) or None (= 1); act: 0 | 'identity', 1 | 'relu', 2 | 'elu'.
    out_d: like g, may be g itself (in place); allocated when missing.  amax_out: a (1,) device float that receives max |d| (zeroed
    here; a NaN in d gives a NaN) - the `amax_a` of the data-gradient convolution that reads d.  Every argument is checked by name
    before anything reaches the GPU."""
    if not isinstance(act, int):
        if act not in FUSE_ACTIVATIONS:
            raise ValueError(f'act: {act!r}, expected one of {list(FUSE_ACTIVATIONS)} or 0, 1, 2')
        act = FUSE_ACTIVATIONS[act]
    if isinstance(act, bool) or not 0 <= act <= 2:
        raise ValueError(f'act: {act!r}, expected 0, 1 or 2')
    for t, name in ((g, 'g'), (out, 'out')):
        if not isinstance(t, torch.Tensor):
            raise ValueError(f'{name}: expected a torch.Tensor, got {type(t).__name__}')
    if g.dim() != 4 or g.numel() == 0:
        raise ValueError(f'g: shape {tuple(g.shape)}, expected (N, h, w, C) with at least one element')
    n, h, w, c = g.shape
    if c % 4:
        raise ValueError(f'g: {c} channels, expected a multiple of 4')
    if n > ACT_GATE_MAX_IMAGES or n * h * w > 0x7fffffff:
        raise ValueError(f'g: shape {tuple(g.shape)}, expected at most {ACT_GATE_MAX_IMAGES} images and 2^31 - 1 pixels')
    if tuple(out.shape) != (n, h, w, c):
        raise ValueError(f'out: shape {tuple(out.shape)}, expected {(n, h, w, c)}')
    if mul is not None and (not isinstance(mul, torch.Tensor) or tuple(mul.shape) != (n, c)):
        raise ValueError(f'mul: shape {tuple(mul.shape) if isinstance(mul, torch.Tensor) else type(mul).__name__}, expected {(n, c)} or None')
    if out_d is not None and (not isinstance(out_d, torch.Tensor) or tuple(out_d.shape) != (n, h, w, c)):
        raise ValueError(f'out_d: shape {tuple(out_d.shape) if isinstance(out_d, torch.Tensor) else type(out_d).__name__}, expected {(n, h, w, c)}')
    _chk(g, 'g')
    _chk(out, 'out')
    if mul is not None:
        _chk(mul, 'mul')
    if out_d is None:
        out_d = torch.empty_like(g)
    else:
        _chk(out_d, 'out_d')
    for t, name in ((g, 'g'), (out, 'out'), (mul, 'mul'), (out_d, 'out_d')):
        if t is not None and t.data_ptr() % 16:
            raise ValueError(f'{name}: must be 16-byte aligned')
        if t is not None and t.device != g.device:
            raise ValueError(f'{name}: on {t.device}, expected {g.device}')
    if amax_out is not None:
        _chk(amax_out, 'amax_out', shape=(1,))
        amax_out.zero_()
    with torch.cuda.device(g.device):
        rc = _lib.lib().mvnerf_act_gate_nhwc(_p(g), _p(out), _p(mul), act, n, h * w, c, _p(out_d), _p(amax_out), _stream(g))
    _lib.check(rc, 'act_gate')
    return out_d


def bn_finalize(stats, n, h, w, cout, eps=1e-3, out=None):
    """mvnerf_bn_finalize: the tile statistics of :func:`conv3x3` over an (n,h,w,cout) output -> (mean, rstd), each (cout,), rstd =
    1 / sqrt(biased variance + eps) over all n h w pixels.  out: a (2, cout) tensor to write them into.  No host read."""
    _chk(stats, 'stats', shape=(conv3x3_stats_bytes(n, h, w, cout) // 4,))
    eps = float(eps)
    if not eps >= 0.0:
        raise ValueError(f'eps: {eps}, expected a non-negative number')
    if out is None:
        out = torch.empty((2, cout), dtype=torch.float32, device=stats.device)
    else:
        _chk(out, 'out', shape=(2, cout))
    with torch.cuda.device(stats.device):
        rc = _lib.lib().mvnerf_bn_finalize(_p(stats), int(n), int(h), int(w), int(cout), eps, _p(out[0]), _p(out[1]), _stream(stats))
    _lib.check(rc, 'bn_finalize')
    return out[0], out[1]


def bn_apply(y, mean, rstd, gamma, beta, skip=None, act=None, out=None, amax_out=None, amax_zeroed=False):
    """mvnerf_bn_apply_nhwc: act(((y - mean) * rstd) * gamma + beta (+ skip)) over y (..., C) fp32, channels last; mean, rstd, gamma,
    beta (C,); skip like y or None; act: 0 | 'identity' | None, 1 | 'relu'.  out may be y (in place).  amax_out: a (1,) device float that
    receives max |out| (zeroed here, unless amax_zeroed says that the caller has done that: several words in one fill)."""
    _chk(y, 'y')
    if y.dim() < 2 or y.numel() == 0:
        raise ValueError(f'y: shape {tuple(y.shape)}, expected (..., C) with at least one pixel')
    c = y.shape[-1]
    if c % 4:
        raise ValueError(f'y: {c} channels, expected a multiple of 4')
    for t, name in ((mean, 'mean'), (rstd, 'rstd'), (gamma, 'gamma'), (beta, 'beta')):
        _chk(t, name, shape=(c,))
    if skip is not None:
        _chk(skip, 'skip', shape=tuple(y.shape))
    if not isinstance(act, int):
        if act not in (None, 'identity', 'relu'):
            raise ValueError(f"act: {act!r}, expected None, 'identity', 'relu' or 0, 1")
        act = int(act == 'relu')
    if act not in (0, 1):
        raise ValueError(f'act: {act}, expected 0 or 1')
    if out is None:
        out = torch.empty_like(y)
    else:
        _chk(out, 'out', shape=tuple(y.shape))
    if amax_out is not None:
        _chk(amax_out, 'amax_out', shape=(1,))
        if not amax_zeroed:
            amax_out.zero_()
    with torch.cuda.device(y.device):
        rc = _lib.lib().mvnerf_bn_apply_nhwc(_p(y), _p(mean), _p(rstd), _p(gamma), _p(beta), _p(skip), y.numel() // c, c, act, _p(out),
                                             _p(amax_out), _stream(y))
    _lib.check(rc, 'bn_apply')
    return out


# ---- the transformer blocks of the ViT (csrc/token_linear.hip, csrc/attention.hip) ----------------------------------------
LINEAR_EPILOGUES = {None: 0, 'gelu': 1}
ATTENTION_MAX_TOKENS = 256
ATTENTION_HEAD_DIMS = (16, 32, 64)


def linear_packed_bytes(k, n):
    """Bytes of the packed stream of an (n, k) Dense weight (k a multiple of 32, n a multiple of 64; ValueError otherwise)."""
    nbytes = _lib.lib().mvnerf_linear_packed_bytes(int(k), int(n))
    if nbytes == 0:
        raise ValueError(f'linear: K={k} N={n} (K a multiple of 32, N a multiple of 64)')
    return nbytes


def linear_pack(weight, out=None):
    """mvnerf_linear_pack: weight (N, K) fp32, torch's Linear layout -> the packed fp16-piece stream (uint8 tensor) that :func:`linear`
    reads; max |w| and the scale are found on the device."""
    _chk(weight, 'weight', shape=(None, None))
    n, k = weight.shape
    nbytes = linear_packed_bytes(k, n)
    if out is None:
        out = torch.empty(nbytes, dtype=torch.uint8, device=weight.device)
    else:
        _chk(out, 'out', dtype=torch.uint8, shape=(nbytes,))
    with torch.cuda.device(weight.device):
        rc = _lib.lib().mvnerf_linear_pack(_p(weight), k, n, _p(out), _stream(weight))
    _lib.check(rc, 'linear_pack')
    return out


def linear(x, packed, n, bias=None, act=None, residual=None, amax_x=None, out=None, amax_out=None, amax_zeroed=False):
    """mvnerf_linear_tokens: out (..., n) = epi(x (..., K) . W^T + bias) over fp32 token rows; packed: :func:`linear_pack` of the (n, K)
    weight; bias (n,) or None; act: None | 'gelu' (exact erf); residual like out or None, added after the bias (not together with
    act).  amax_x: a device float (1,) bounding |x| (computed with :func:`absmax` when missing); amax_out: a (1,) device float that
    receives max |out| (zeroed here; amax_zeroed=True says that the caller has zeroed it, as :func:`bn_apply` takes it).  Any number of
    rows; K a multiple of 32, n a multiple of 64."""
    _chk(x, 'x')
    if x.dim() < 2 or x.numel() == 0:
        raise ValueError(f'x: shape {tuple(x.shape)}, expected (..., K) with at least one row')
    k = x.shape[-1]
    m = x.numel() // k
    n = int(n)
    _chk(packed, 'packed', dtype=torch.uint8, shape=(linear_packed_bytes(k, n),))
    if act not in LINEAR_EPILOGUES:
        raise ValueError(f"act: {act!r}, expected None or 'gelu'")
    if act is not None and residual is not None:
        raise ValueError('act and residual do not go together: the epilogue is the bias, then gelu OR the residual')
    shape = (*x.shape[:-1], n)
    if bias is not None:
        _chk(bias, 'bias', shape=(n,))
    if residual is not None:
        _chk(residual, 'residual', shape=shape)
    if amax_x is None:
        amax_x = absmax(x)
    else:
        _chk(amax_x, 'amax_x', shape=(1,))
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=x.device)
    else:
        _chk(out, 'out', shape=shape)
        if out.data_ptr() == x.data_ptr():
            raise ValueError('out: must not be x (a tile reads whole rows of x while others write)')
    if amax_out is not None:
        _chk(amax_out, 'amax_out', shape=(1,))
        if not amax_zeroed:
            amax_out.zero_()
    epi = 2 if residual is not None else LINEAR_EPILOGUES[act]
    with torch.cuda.device(x.device):
        rc = _lib.lib().mvnerf_linear_tokens(_p(x), _p(amax_x), _p(packed), _p(bias), _p(residual), m, k, n, epi, _p(out), _p(amax_out),
                                             _stream(x))
    _lib.check(rc, 'linear')
    return out


def layer_norm(x, gamma, beta, eps=1e-3, out=None, amax_out=None, amax_zeroed=False):
    """mvnerf_layer_norm_tokens: ((x - mean) * rstd) * gamma + beta per row of x (..., C) fp32 with the biased variance; gamma, beta (C,).
    out may be x (in place).  amax_out: a (1,) device float that receives max |out| (zeroed here).  C a multiple of 4."""
    _chk(x, 'x')
    if x.dim() < 2 or x.numel() == 0:
        raise ValueError(f'x: shape {tuple(x.shape)}, expected (..., C) with at least one row')
    c = x.shape[-1]
    if c % 4:
        raise ValueError(f'x: {c} channels, expected a multiple of 4')
    _chk(gamma, 'gamma', shape=(c,))
    _chk(beta, 'beta', shape=(c,))
    eps = float(eps)
    if not eps >= 0.0:
        raise ValueError(f'eps: {eps}, expected a non-negative number')
    if out is None:
        out = torch.empty_like(x)
    else:
        _chk(out, 'out', shape=tuple(x.shape))
    if amax_out is not None:
        _chk(amax_out, 'amax_out', shape=(1,))
        if not amax_zeroed:
            amax_out.zero_()
    with torch.cuda.device(x.device):
        rc = _lib.lib().mvnerf_layer_norm_tokens(_p(x), _p(gamma), _p(beta), x.numel() // c, c, eps, _p(out), _p(amax_out), _stream(x))
    _lib.check(rc, 'layer_norm')
    return out


def attention(qkv, scale=None, out=None, amax_out=None, amax_zeroed=False):
    """mvnerf_attention_tokens: qkv (B, n, 3, heads, d) fp32, the QKV Dense layer's output as it lies -> (B, n, heads * d) =
    softmax(q k^T * scale) v per image and head, fp32 throughout; scale defaults to 1 / sqrt(d).  d in ATTENTION_HEAD_DIMS and
    n <= ATTENTION_MAX_TOKENS.  amax_out: a (1,) device float that receives max |out| (zeroed here)."""
    _chk(qkv, 'qkv', shape=(None, None, 3, None, None))
    b, n, _, heads, d = qkv.shape
    if qkv.numel() == 0:
        raise ValueError(f'qkv: shape {tuple(qkv.shape)}, expected at least one token and one head')
    if d not in ATTENTION_HEAD_DIMS:
        raise ValueError(f'qkv: head dimension {d}, expected one of {ATTENTION_HEAD_DIMS}')
    if n > ATTENTION_MAX_TOKENS:
        raise ValueError(f'qkv: {n} tokens, at most {ATTENTION_MAX_TOKENS} (the logits of a query stay in registers)')
    scale = float(d) ** -0.5 if scale is None else float(scale)
    if not np.isfinite(scale):
        raise ValueError(f'scale: {scale}, expected a finite number')
    if out is None:
        out = torch.empty((b, n, heads * d), dtype=torch.float32, device=qkv.device)
    else:
        _chk(out, 'out', shape=(b, n, heads * d))
    if amax_out is not None:
        _chk(amax_out, 'amax_out', shape=(1,))
        if not amax_zeroed:
            amax_out.zero_()
    with torch.cuda.device(qkv.device):
        rc = _lib.lib().mvnerf_attention_tokens(_p(qkv), b, n, heads, d, scale, _p(out), _p(amax_out), _stream(qkv))
    _lib.check(rc, 'attention')
    return out
