"""The stand-alone field-backward reference (oracle/field_backward_ref.py) against torch autograd, without a GPU.

The float64 torch twin's trunk is run with `complete_output`, its pre-activations are packed into a stash-shaped array (the
encoder), decoded back (the decoder the GPU tests use on the kernel's stash), and fed to field_backward_ref; every variable's
gradient, d_z and d_features must match autograd of sum(rgbs * d_rgbs) through T.field_eval to 1e-10 relative L2 - both sides
are float64 doing the same sums."""
import numpy as np
import pytest
import torch

from oracle import field_backward_ref as R
from oracle import mvnerf_torch as T
from thesis_clip_nerf_amd.synthetic import make_scene

GEO = ('rays_o', 'rays_d', 'images', 'features', 'intrinsics', 'extrinsics_inv')


def _twin_forward(sc, z, views):
    """float64 twin: layer-0 input, the 13 pre-activations of the trunk as rows, rgbs."""
    t = {k: torch.as_tensor(sc[k]).double() for k in GEO}
    net = T.unflatten_net(torch.as_tensor(sc['fine']).double())
    x_in, _ = R.layer0_input_torch(t['rays_o'], t['rays_d'], torch.as_tensor(z).double(), t['images'], t['features'], t['intrinsics'],
                                   t['extrinsics_inv'])
    b, r, s = z.shape
    # the twin's trunk with complete_output: [x0, x1, x2, x3, mean, x4, x5, x6]
    world = T.points_on_rays(t['rays_o'], t['rays_d'], torch.as_tensor(z).double())
    pix, cam = T.compute_pixel_in_image_mv(world, t['intrinsics'], t['extrinsics_inv'])
    grid = torch.cat([t['images'] * 2.0 - 1.0, t['features']], -1).reshape(b * views, 16, 16, -1)
    feat = T.interpolate_bilinear_xy(grid, pix.reshape(b * views, r * s, 2)).reshape(b * views, r, s, -1)
    cdir = T.world_to_camera_direction_vector_mv(t['rays_d'], t['extrinsics_inv'])[:, :, :, None, :].expand(b, views, r, s, 3)
    outs = T.mv_embedding(net, cam[..., :3].reshape(b * views, r, s, 3), cdir.reshape(b * views, r, s, 3), feat, views, complete_output=True)
    assert (outs[0].reshape(-1, 128) - (x_in @ net['W0'] + net['b0'])).abs().max() < 1e-12      # x_in is the input of that trunk
    ins = outs[:3] + outs[4:7]                                # the inputs of the six blocks
    hid = [torch.relu(xk) @ blk[0] + blk[1] for xk, blk in zip(ins, net['blocks'])]    # the expression resnet_block evaluates
    names = dict(x0=outs[0], x1=outs[1], x2=outs[2], x3=outs[3], mean=outs[4], x4=outs[5], x5=outs[6], x6=outs[7],
                 h1=hid[0], h2=hid[1], h3=hid[2], h4=hid[3], h5=hid[4], h6=hid[5])
    rows = {k: v.reshape(-1, 128).numpy() for k, v in names.items()}
    rgb, sigma = T.render_readout(net, outs[7])
    return x_in.numpy(), rows, torch.cat([rgb, sigma[..., None]], -1).numpy()


@pytest.mark.parametrize('views', [1, 2])
def test_reference_matches_autograd_of_the_float64_twin(views):
    sc = make_scene(seed=200 + views, batch=1, n_views=views, height=16, width=16, n_rays=24, n_samples=64, bias_scale=0.05)
    b, r, s = 1, 24, 64
    _, z = T.sample_along_ray(torch.as_tensor(sc['rays_o']).double(), torch.as_tensor(sc['rays_d']).double(), sc['near'], sc['far'], s,
                              torch.as_tensor(sc['u_coarse']).double())
    z = z.numpy()
    x_in, rows, rgbs = _twin_forward(sc, z, views)
    d_rgbs = np.random.default_rng(7).standard_normal(rgbs.shape)

    # encoder / decoder round trip through the stash layout
    stash = R.encode_stash(rows, b, views, r, s)
    assert stash.size == R.stash_floats(b, views, r, s) and stash.dtype == np.float64
    back = R.decode_stash(stash, b, views, r, s)
    for name in R.VIEW_SLOTS + R.FUSED_SLOTS:
        if name == 'x3' and views > 1:
            assert np.isnan(back[name]).all()                # in the layout, written by nobody
        elif name == 'x3':
            assert np.array_equal(back[name], rows['mean'])
        else:
            assert np.array_equal(back[name], rows[name]), name

    grad, g0, c0 = R.field_backward_ref(sc['fine'], back, rgbs, d_rgbs, x_in, views, np.float64)
    d_z, d_feat, _, x_again = R.input_grads(c0, *(sc[k] for k in GEO[:2]), z, *(sc[k] for k in GEO[2:]), dtype=torch.float64)
    assert np.array_equal(x_again, x_in)

    # autograd through the twin's own field pass
    t = {k: torch.as_tensor(sc[k]).double() for k in GEO}
    flat = torch.as_tensor(sc['fine']).double().requires_grad_(True)
    zt = torch.as_tensor(z).requires_grad_(True)
    ft = t['features'].clone().requires_grad_(True)
    rgb, sigma = T.field_eval(T.unflatten_net(flat), t['rays_o'], t['rays_d'], zt, t['images'], ft, t['intrinsics'], t['extrinsics_inv'])
    out = torch.cat([rgb, sigma[..., None]], -1)
    assert np.abs(out.detach().numpy() - rgbs).max() < 1e-12
    (out * torch.as_tensor(d_rgbs)).sum().backward()
    want = flat.grad.numpy()

    def rel(a, w):
        return np.linalg.norm(a - w) / np.linalg.norm(w)
    for name, lo, hi in R.net_sections():
        assert np.linalg.norm(want[lo:hi]) > 0, name
        assert rel(grad[lo:hi], want[lo:hi]) < 1e-10, (name, rel(grad[lo:hi], want[lo:hi]))
    assert rel(d_z, zt.grad.numpy()) < 1e-10
    assert rel(d_feat, ft.grad.numpy()) < 1e-10
    assert g0.shape == (views * r * s, 128) and c0.shape == (views * r * s, 379)


def test_float32_run_of_the_reference_is_at_fp32_rounding_level():
    """The float32 run is the yardstick of the GPU tests' bars: the same algebra, so it sits a few 1e-7 from the float64 run."""
    sc = make_scene(seed=201, batch=1, n_views=1, height=16, width=16, n_rays=24, n_samples=64, bias_scale=0.05)
    _, z = T.sample_along_ray(torch.as_tensor(sc['rays_o']).double(), torch.as_tensor(sc['rays_d']).double(), sc['near'], sc['far'], 64,
                              torch.as_tensor(sc['u_coarse']).double())
    x_in, rows, rgbs = _twin_forward(sc, z.numpy(), 1)
    rows32 = {k: v.astype(np.float32) for k, v in rows.items()}          # one set of masks for both runs
    d_rgbs = np.random.default_rng(7).standard_normal(rgbs.shape).astype(np.float32)
    g64, _, _ = R.field_backward_ref(sc['fine'], rows32, rgbs.astype(np.float32), d_rgbs, x_in.astype(np.float32), 1, np.float64)
    g32, _, _ = R.field_backward_ref(sc['fine'], rows32, rgbs.astype(np.float32), d_rgbs, x_in.astype(np.float32), 1, np.float32)
    assert g32.dtype == np.float32 and g64.dtype == np.float64
    for name, lo, hi in R.net_sections():
        e = np.linalg.norm(g32[lo:hi] - g64[lo:hi]) / np.linalg.norm(g64[lo:hi])
        assert 0 < e < 5e-6, (name, e)


def test_layer0_input_of_the_numpy_oracle_matches_the_twin():
    sc = make_scene(seed=202, batch=2, n_views=2, height=16, width=16, n_rays=5, n_samples=32, bias_scale=0.05)
    from oracle import mvnerf_oracle as O
    _, z = O.sample_along_ray(sc['rays_o'], sc['rays_d'], sc['near'], sc['far'], 32, sc['u_coarse'])
    x32 = R.layer0_input_f32(sc['rays_o'], sc['rays_d'], z, *(sc[k] for k in GEO[2:]))
    _, _, pix, x64 = R.input_grads(None, sc['rays_o'], sc['rays_d'], z, *(sc[k] for k in GEO[2:]), dtype=torch.float64)
    assert x32.shape == x64.shape == (2 * 2 * 5 * 32, 379) and pix.shape == (2, 2, 5, 32, 2)
    # positional encoding of octave 9 has an argument gain of pi * 2^9 on an fp32 coordinate: ~1e-4; the other rows are at 1e-6
    assert np.abs(x32 - x64).max() < 1e-3 and np.abs(x32[:, 120:] - x64[:, 120:]).max() < 2e-5
