"""One sample front end, several kernels: the kernels on the 32x32 lane mapping (field_eval.hip, field_eval_split.hip, field_eval_bf16.hip)
share the routines of csrc/mvnerf_field_common.h, the 16x16x32 kernels (field_eval_split16_impl.h) keep a front end of their own.  Projection
and taps are the same fp32 operations everywhere (the parity contract of mvnerf_math.h), so the tap indices and pixels they report are equal
element for element - GPU results against GPU results, no tolerance."""
import numpy as np
import pytest
import torch

from thesis_clip_nerf_amd import ops
from thesis_clip_nerf_amd.synthetic import make_scene

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


@pytest.mark.parametrize('batch,n_views,n_rays,s', [(2, 2, 5, 40), (1, 1, 3, 32)])
def test_tap_idx_and_pix_agree_across_field_kernels(batch, n_views, n_rays, s):
    """(2, 2, 5, 40): 12 whole tiles and one of 16 samples, tiles that straddle rays and the two scenes; (1, 1, 3, 32): one ray per tile."""
    sc = make_scene(seed=90 + n_views, batch=batch, n_views=n_views, height=16, width=16, n_rays=n_rays, n_samples=s, bias_scale=0.05)
    d = {k: torch.from_numpy(np.ascontiguousarray(sc[k])).to(DEV)
         for k in ('rays_o', 'rays_d', 'images', 'features', 'intrinsics', 'extrinsics_inv', 'fine', 'u_coarse')}
    z = ops.stratified_depths(d['u_coarse'], sc['near'], sc['far'])
    args = (d['rays_o'], d['rays_d'], z, d['images'], d['features'], d['intrinsics'], d['extrinsics_inv'])
    packed, split, packed16 = ops.pack_net(d['fine']), ops.pack_net_split(d['fine']), ops.pack_net_bf16(d['fine'])
    table = ops.project_texels(d['features'], packed)

    _, taps_ref, pix_ref = ops.field_eval(*args, packed, return_taps=True, return_pix=True)
    assert taps_ref.shape == (batch, n_views, n_rays, s, 4) and pix_ref.shape == (batch, n_views, n_rays, s, 2)
    _, taps, pix = ops.field_eval(*args, packed, return_taps=True, return_pix=True, texel_table=table)
    assert torch.equal(taps, taps_ref) and torch.equal(pix, pix_ref), 'field_eval, texel table'
    for kernel in ('split_f16', 'split_bf16', 'split_bf16_32x32x16'):
        for tab in (None, table):
            _, taps, pix = ops.field_eval_split(*args, packed, split, return_taps=True, return_pix=True, texel_table=tab, kernel=kernel)
            where = f'field_eval_split {kernel}, {"direct" if tab is None else "texel table"}'
            assert torch.equal(taps, taps_ref), where
            assert torch.equal(pix, pix_ref), where
    _, taps = ops.field_eval_bf16(*args, packed, packed16, return_taps=True)
    assert torch.equal(taps, taps_ref), 'field_eval_bf16, direct'
