"""float64 reference for the range status of the guarded fp16 field kernel (include/mvnerf_hip.h, mvnerf_field_eval_split_ex).

The geometry (projection, bilinear gather, the arguments of the positional encoding) is the NumPy oracle's fp32 restatement - those
values ARE fp32 in the kernel too - and the trunk behind it is evaluated in float64 from a Keras-order net.  `operand_max` returns
the largest |v| over exactly what the kernel cuts into fp16 activation pieces:
  * PE(cam xyz) and the gathered rgb (both forms; PE(cam dir) is not cut: it enters through the fp32 per-ray seed);
  * the 256 gathered features (direct form only: the texel-table form adds their fp32 products to the accumulators);
  * relu(x) and relu(h) in front of the 12 hidden Dense layers, per view and fused (the read-out runs on the vector ALU: not cut).
"""
import numpy as np

from oracle import mvnerf_oracle as O


def trunk64(net_flat, rays_o, rays_d, z, images, features, k4, einv):
    """-> dict: 'pe_rgb' (B*V,R,S,63), 'feat' (B*V,R,S,256), 'x' = the 8 complete_output activations and 'h' = the 6 hidden
    pre-activations, all float64."""
    net = O.unflatten_net(net_flat)
    b, v = images.shape[:2]
    r, s = z.shape[1:3]
    norm_images = (images.astype(np.float32) * np.float32(2.0) - np.float32(1.0)).astype(np.float32)
    world = O.points_on_rays(rays_o, rays_d, z)
    pix, cam = O.compute_pixel_in_image_mv(world, k4, einv)
    feat = O.get_projection_features_mv(norm_images, features, pix).reshape(b * v, r, s, -1)
    cdir = O.world_to_camera_direction_vector_mv(rays_d, einv)
    cdir = np.broadcast_to(cdir[:, :, :, None, :], cam.shape[:-1] + (3,)).reshape(b * v, r, s, 3)
    pe_xyz = O.position_encoding(cam[..., :3].reshape(b * v, r, s, 3)).astype(np.float64)
    pe_dir = O.position_encoding(cdir).astype(np.float64)
    f64 = lambda a: np.asarray(a, np.float64)
    x = np.concatenate([pe_xyz, pe_dir, f64(feat)], -1) @ f64(net['W0']) + f64(net['b0'])
    xs, hs = [x], []

    def block(x, blk):
        w1, b1, w2, b2 = map(f64, blk)
        h = np.maximum(x, 0) @ w1 + b1
        hs.append(h)
        return x + np.maximum(h, 0) @ w2 + b2

    for blk in net['blocks'][:3]:
        xs.append(block(xs[-1], blk))
    xs.append(xs[-1].reshape(b, v, r, s, 128).mean(1))
    for blk in net['blocks'][3:]:
        xs.append(block(xs[-1], blk))
    return {'pe_rgb': np.concatenate([pe_xyz, f64(feat[..., :3])], -1), 'feat': f64(feat[..., 3:]), 'x': xs, 'h': hs}


def operand_max(t, table):
    """The range status the guarded kernel must report for trunk64's result `t`; table: the texel-table form."""
    inputs = [t['x'][k] for k in (0, 1, 2, 4, 5, 6)] + t['h']          # x3 (k = 3) only enters the view mean; x6 (k = 7) the read-out
    m = max(float(np.maximum(a, 0).max()) for a in inputs)
    m = max(m, float(np.abs(t['pe_rgb']).max()))
    if not table:
        m = max(m, float(np.abs(t['feat']).max()))
    return m


def stash_relu_max(t):
    """max relu over the 13 pre-activation tensors the training forward stashes (x0..x2, h1..h3, mean, h4..h6, x4..x6 less x6's
    consumer): the operands of the hidden layers."""
    inputs = [t['x'][k] for k in (0, 1, 2, 4, 5, 6)] + t['h']
    return max(float(np.maximum(a, 0).max()) for a in inputs)
