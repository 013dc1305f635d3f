"""The plain single-view inference variants of the split16 field kernels form the layer-0 seed rows b0 + W0_dir^T PE(cam dir) of
their own rays in the kernel prologue (csrc/field_eval_split16_impl.h, kSeedHere; the row itself: dir_seed_row,
csrc/mvnerf_field_common.h) instead of reading what a dir_bias_kernel launch left.  The variant with the optional outputs still takes
its rows from that launch - the same routine, so the two must agree bit for bit - and every shape is held to the per-sample oracle
bars of tests/test_gpu_field_sections.py."""
import functools

import numpy as np
import pytest
import torch

from oracle import mvnerf_oracle as O
from thesis_clip_nerf_amd import ops
from thesis_clip_nerf_amd.synthetic import make_scene

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
KEYS = ['rays_o', 'rays_d', 'images', 'features', 'intrinsics', 'extrinsics_inv', 'fine']

# (batch, rays, samples): a group is 8 tiles = 256 consecutive samples, a workgroup forms the rows of every ray its groups touch
#   (2, 5, 32)    one group, the scene changes between tiles, six idle waves shadow the last tile
#   (1, 5, 96)    three tiles per ray, rays straddle the two groups (a row formed by two workgroups)
#   (1, 5, 40)    the per-lane front end, 200 samples: the last tile is partial, the last group's end is clamped
#   (1, 600, 128) 300 groups on a persistent grid of one workgroup per compute unit: workgroups own two groups
SHAPES = [(2, 5, 32), (1, 5, 96), (1, 5, 40), (1, 600, 128)]


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@functools.lru_cache(maxsize=None)
def case(batch, rays, s):
    """Scene, depths and the oracle's per-sample outputs of one shape: computed once, read by every test of the shape."""
    sc = make_scene(seed=51 + s, batch=batch, height=16, width=16, n_views=1, n_rays=rays, bias_scale=0.1)
    z = np.sort(np.random.default_rng(13).uniform(0.3, 1.3, (batch, rays, s)).astype(np.float32), -1)
    rgb_ref, sig_ref = O.field_eval(O.unflatten_net(sc['fine']), sc['rays_o'], sc['rays_d'], z, sc['images'], sc['features'],
                                    sc['intrinsics'], sc['extrinsics_inv'])
    for a in (z, rgb_ref, sig_ref):
        a.setflags(write=False)
    return sc, z, rgb_ref, sig_ref


def device_args(batch, rays, s, table):
    """-> the arguments of a call with the fine net, the same with the coarse net in its place (other seed rows), the fine net's table."""
    sc, z, _, _ = case(batch, rays, s)
    d = {k: dev(sc[k]) for k in KEYS + ['coarse']}
    packed, split = ops.pack_net(d['fine']), ops.pack_net_split(d['fine'])
    tab = ops.project_texels(d['features'], packed) if table else None
    geo = (d['rays_o'], d['rays_d'], dev(z.copy()), d['images'], d['features'], d['intrinsics'], d['extrinsics_inv'])
    return geo + (packed, split), geo + (ops.pack_net(d['coarse']), ops.pack_net_split(d['coarse'])), tab


def plain_after_other_rows(args, other, tab, **kw):
    """The plain call under test.  Its seed rows live in a workspace the wrapper allocates uninitialised per call, so a block the
    allocator hands out again could still hold the right rows of an earlier call.  A call of the same shape with ANOTHER net goes first
    (the same allocations in the same order, so its freed workspace is what the next call gets, now holding the wrong rows), and the
    rows of a third call with the standalone seed kernel, right ones again, are not there yet."""
    decoy_kw = dict(kw, range_status=torch.zeros_like(kw['range_status'])) if 'range_status' in kw else kw
    decoy = ops.field_eval_split(*other, texel_table=tab, **decoy_kw)
    torch.cuda.synchronize()
    del decoy
    return ops.field_eval_split(*args, texel_table=tab, **kw)


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
@pytest.mark.parametrize('batch,rays,s', SHAPES)
def test_rows_formed_in_the_launch_equal_the_seed_kernels(batch, rays, s, gemm, table, split_kernel):
    split_kernel(gemm)
    _, _, rgb_ref, sig_ref = case(batch, rays, s)
    args, other, tab = device_args(batch, rays, s, table)
    plain = plain_after_other_rows(args, other, tab)                                   # seed rows formed in the launch
    with_taps = ops.field_eval_split(*args, return_taps=True, texel_table=tab)[0]      # seed rows from dir_bias_kernel
    torch.cuda.synchronize()
    got = plain.cpu().numpy()
    e_rgb, e_sig = np.abs(got[..., :3] - rgb_ref).max(), np.abs(got[..., 3] - sig_ref).max()
    print(f'B={batch} R={rays} S={s} {gemm} table={table}: max|rgb - oracle| {e_rgb:.2e}, max|sigma - oracle| {e_sig:.2e}')
    assert torch.equal(plain, with_taps)
    assert e_rgb < 5e-6 and e_sig < 2e-5 * max(1.0, np.abs(sig_ref).max()), (e_rgb, e_sig)


@pytest.mark.parametrize('table', [False, True])
def test_range_guarded_launch_forms_the_same_rows(table):
    batch, rays, s = 1, 5, 96
    _, _, rgb_ref, sig_ref = case(batch, rays, s)
    args, other, tab = device_args(batch, rays, s, table)
    status = torch.zeros(1, dtype=torch.float32, device=DEV)
    guarded = plain_after_other_rows(args, other, tab, kernel='split_f16', range_status=status)
    with_taps = ops.field_eval_split(*args, return_taps=True, texel_table=tab, kernel='split_f16')[0]
    torch.cuda.synchronize()
    got = guarded.cpu().numpy()
    e_rgb, e_sig = np.abs(got[..., :3] - rgb_ref).max(), np.abs(got[..., 3] - sig_ref).max()
    print(f'guarded B={batch} R={rays} S={s} table={table}: max|rgb - oracle| {e_rgb:.2e}, max|sigma - oracle| {e_sig:.2e}')
    assert 0.0 < float(status[0]) < ops.F16X3_MAX_ACT
    assert torch.equal(guarded, with_taps)
    assert e_rgb < 5e-6 and e_sig < 2e-5 * max(1.0, np.abs(sig_ref).max()), (e_rgb, e_sig)
