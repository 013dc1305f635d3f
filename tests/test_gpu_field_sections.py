"""The sections of the split16 field kernels between their MFMA runs (csrc/field_eval_split16_impl.h): the tile front end has a
wave-uniform path for S % 32 == 0 (a tile lies inside one ray: scalar index arithmetic, scalar loads of the ray and of the view's
matrices) beside the per-lane path for every other S, the first Dense layer of a ResNet block takes its bias row as the C operand of
its first MFMAs, and the weight ring keeps its slots as rotating scalar state.  Per-sample arithmetic is the same on both front-end
paths, so they must agree bit for bit; every shape is held to the per-sample bars of tests/test_gpu_split.py."""
import numpy as np
import pytest
import torch

from oracle import mvnerf_oracle as O
from thesis_clip_nerf_amd import ops
from thesis_clip_nerf_amd.synthetic import make_scene

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
KEYS = ['rays_o', 'rays_d', 'images', 'features', 'intrinsics', 'extrinsics_inv', 'fine']


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def depths(seed, b, r, s):
    return np.sort(np.random.default_rng(seed).uniform(0.3, 1.3, (b, r, s)).astype(np.float32), -1)


@pytest.fixture
def split_kernel():
    prev = []

    def choose(name):
        prev.append(ops.set_split_kernel(name))
    yield choose
    if prev:
        ops.set_split_kernel(prev[0])


@pytest.mark.parametrize('table', [False, True])
@pytest.mark.parametrize('gemm', ['split_f16', 'split_bf16'])
def test_uniform_front_end_equals_per_lane_front_end_bit_for_bit(gemm, table, split_kernel):
    """R = 24 rays of S = 64 (a tile inside one ray: the uniform path) against the same samples as 96 rays of S = 16, every ray
    repeated four times with a quarter of its depths (a tile holds two rays: the per-lane path)."""
    split_kernel(gemm)
    sc = make_scene(seed=21, height=16, width=16, n_views=1, n_rays=24, bias_scale=0.1)
    d = {k: dev(sc[k]) for k in KEYS}
    z = dev(depths(5, 1, 24, 64))
    packed, split = ops.pack_net(d['fine']), ops.pack_net_split(d['fine'])
    tab = ops.project_texels(d['features'], packed) if table else None
    maps = (d['images'], d['features'], d['intrinsics'], d['extrinsics_inv'], packed, split)
    whole = ops.field_eval_split(d['rays_o'], d['rays_d'], z, *maps, texel_table=tab)
    quarters = ops.field_eval_split(d['rays_o'].repeat_interleave(4, dim=1).contiguous(), d['rays_d'].repeat_interleave(4, dim=1).contiguous(),
                                    z.reshape(1, 96, 16).contiguous(), *maps, texel_table=tab)
    torch.cuda.synchronize()
    assert whole.shape == (1, 24, 64, 4) and quarters.shape == (1, 96, 16, 4)
    assert whole.abs().max().item() > 0
    np.testing.assert_array_equal(quarters.reshape(1, 24, 64, 4).cpu().numpy(), whole.cpu().numpy())


# (batch, rays, samples): the scene index changes between tiles and the last workgroup has idle waves; three tiles per ray; S no
# multiple of 32 (the per-lane path) with 5 * 40 = 200 samples, so that the last tile is partial
EDGE_SHAPES = [(2, 5, 32), (1, 5, 96), (1, 5, 40)]


@pytest.mark.parametrize('table', [False, True])
@pytest.mark.parametrize('batch,rays,s', EDGE_SHAPES)
def test_front_end_edges_match_oracle(batch, rays, s, table):
    sc = make_scene(seed=31 + s, batch=batch, height=16, width=16, n_views=1, n_rays=rays, bias_scale=0.1)
    d = {k: dev(sc[k]) for k in KEYS}
    z = depths(7, batch, rays, s)
    rgb_ref, sig_ref, taps_ref = O.field_eval(O.unflatten_net(sc['fine']), sc['rays_o'], sc['rays_d'], z, sc['images'], sc['features'],
                                              sc['intrinsics'], sc['extrinsics_inv'], return_taps=True)
    packed, split = ops.pack_net(d['fine']), ops.pack_net_split(d['fine'])
    tab = ops.project_texels(d['features'], packed) if table else None
    args = (d['rays_o'], d['rays_d'], dev(z), d['images'], d['features'], d['intrinsics'], d['extrinsics_inv'], packed, split)
    plain = ops.field_eval_split(*args, texel_table=tab)                                   # the render variant
    rgbs, taps = ops.field_eval_split(*args, return_taps=True, texel_table=tab)            # the variant with the optional outputs
    torch.cuda.synchronize()
    np.testing.assert_array_equal(taps.cpu().numpy(), taps_ref)
    for name, out in (('plain', plain), ('taps', rgbs)):
        got = out.cpu().numpy()
        e_rgb, e_sig = np.abs(got[..., :3] - rgb_ref).max(), np.abs(got[..., 3] - sig_ref).max()
        print(f'B={batch} R={rays} S={s} table={table} {name}: max|rgb - oracle| {e_rgb:.2e}, max|sigma - oracle| {e_sig:.2e}')
        assert e_rgb < 5e-6 and e_sig < 2e-5 * max(1.0, np.abs(sig_ref).max()), (name, e_rgb, e_sig)
    assert torch.equal(plain, rgbs)                                                         # same arithmetic in both variants


@pytest.mark.parametrize('table', [False, True])
def test_two_views_match_oracle(table):
    sc = make_scene(seed=41, height=16, width=16, n_views=2, n_rays=8, bias_scale=0.1)
    d = {k: dev(sc[k]) for k in KEYS}
    z = depths(9, 1, 8, 32)
    rgb_ref, sig_ref, taps_ref = O.field_eval(O.unflatten_net(sc['fine']), sc['rays_o'], sc['rays_d'], z, sc['images'], sc['features'],
                                              sc['intrinsics'], sc['extrinsics_inv'], return_taps=True)
    packed, split = ops.pack_net(d['fine']), ops.pack_net_split(d['fine'])
    tab = ops.project_texels(d['features'], packed) if table else None
    args = (d['rays_o'], d['rays_d'], dev(z), d['images'], d['features'], d['intrinsics'], d['extrinsics_inv'], packed, split)
    plain = ops.field_eval_split(*args, texel_table=tab)
    rgbs, taps = ops.field_eval_split(*args, return_taps=True, texel_table=tab)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(taps.cpu().numpy(), taps_ref)
    for out in (plain, rgbs):
        got = out.cpu().numpy()
        e_rgb, e_sig = np.abs(got[..., :3] - rgb_ref).max(), np.abs(got[..., 3] - sig_ref).max()
        assert e_rgb < 5e-6 and e_sig < 2e-5 * max(1.0, np.abs(sig_ref).max()), (e_rgb, e_sig)


@pytest.mark.parametrize('table', [False, True])
def test_training_forward_stash_matches_fp32_stash(table):
    """kStash at R = 8, S = 32: per-sample outputs and the 13 written pre-activation slots against the fp32-MFMA kernel's
    (the bars of tests/test_gpu_split.py), and the outputs against the inference variant of the same kernel."""
    sc = make_scene(seed=43, height=16, width=16, n_views=1, n_rays=8, bias_scale=0.05)
    d = {k: dev(sc[k]) for k in KEYS}
    z = dev(depths(11, 1, 8, 32))
    packed, split = ops.pack_net(d['fine']), ops.pack_net_split(d['fine'])
    tab = ops.project_texels(d['features'], packed) if table else None
    args = (d['rays_o'], d['rays_d'], z, d['images'], d['features'], d['intrinsics'], d['extrinsics_inv'], packed)
    rgbs32, stash32 = ops.field_eval_stash(*args, texel_table=tab)
    rgbs, stash = ops.field_eval_stash(*args, texel_table=tab, packed_split=split)
    infer = ops.field_eval_split(*args, split, texel_table=tab)
    torch.cuda.synchronize()
    n = ops.stash_bytes(1, 1, 8, 32) // 4
    slot = (8 * 32 // 32) * 4096                                                 # floats per per-view slot
    keep = torch.ones(n, dtype=torch.bool, device=DEV)
    keep[6 * slot:7 * slot] = False                                              # per-view slot 6 (x3) is written by neither kernel
    a, b = stash.view(torch.float32)[:n][keep], stash32.view(torch.float32)[:n][keep]
    assert (rgbs - rgbs32).abs().max().item() < 1e-5
    assert (a - b).abs().max().item() < 2e-5 * max(1.0, b.abs().max().item())
    assert torch.equal(rgbs, infer)
