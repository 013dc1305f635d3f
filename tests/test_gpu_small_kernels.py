"""The small kernels around the two field launches of a render step.

project_texels_kernel (csrc/field_eval.hip) projects two nets either from one staged copy of 32 feature rows (workgroups of 8 waves)
or, while that would leave compute units without a workgroup, as one 4-wave workgroup per (32 texels, net): the same MFMA sequence
per wave, so both tables must equal the single-net tables bit for bit on either side of the threshold.

resample_kernel (csrc/ray_ops.hip) counts the rank of each depth in the (value, index) order with wave-wide compare masks, and
sample_pdf_core lets one lane run the sequential cdf sum: every decision (above, below, the rank) and every value must stay the
oracle's, ties included."""
import numpy as np
import pytest
import torch

from oracle import mvnerf_oracle as O
from thesis_clip_nerf_amd import ops
from thesis_clip_nerf_amd.synthetic import make_scene

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
F32 = np.float32


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


# 5 x 7: 35 texels, a partial second block; 64 x 64: the benchmark's 128 blocks; 128 x 128: 512 blocks
@pytest.mark.parametrize('height,width,form', [(5, 7, 'split'), (64, 64, 'split'), (128, 128, 'shared')])
def test_project_texels2_equals_the_single_net_tables(height, width, form):
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    blocks = (height * width + 31) // 32
    assert (blocks < cus) == (form == 'split'), (blocks, cus)          # the case lies on the side of the threshold it is meant for
    sc = make_scene(seed=3, height=16, width=16, n_views=1, n_rays=4, bias_scale=0.1)
    features = torch.randn((1, 1, height, width, 256), generator=torch.Generator(DEV).manual_seed(height), device=DEV)
    a, b = ops.pack_net(dev(sc['coarse'])), ops.pack_net(dev(sc['fine']))
    both = ops.project_texels2(features, a, b)
    one_a, one_b = ops.project_texels(features, a), ops.project_texels(features, b)
    torch.cuda.synchronize()
    assert both.shape == (2, 1, 1, height, width, 128) and one_a.abs().max().item() > 0 and not torch.equal(one_a, one_b)
    np.testing.assert_array_equal(both[0].cpu().numpy(), one_a.cpu().numpy())
    np.testing.assert_array_equal(both[1].cpu().numpy(), one_b.cpu().numpy())


def stable_rank(z, z_fine):
    """Position of importance sample i in the ascending (value, index) order of [coarse | fine]."""
    order = np.argsort(np.concatenate([z, z_fine], axis=-1), axis=-1, kind='stable')
    pos = np.empty_like(order)
    np.put_along_axis(pos, order, np.broadcast_to(np.arange(order.shape[-1]), order.shape), axis=-1)
    return pos[..., z.shape[-1]:].astype(np.int32)


def resample_inputs():
    rng = np.random.default_rng(17)
    n = 8
    _, z = O.sample_along_ray(np.zeros((1, n, 3), F32), np.ones((1, n, 3), F32), 0.3, 1.3, 64, rng.random((1, n, 64), dtype=F32))
    z = np.ascontiguousarray(z, dtype=F32)
    w = (rng.random((1, n, 64), dtype=F32) ** 3).astype(F32)
    u = rng.random((1, n, 64), dtype=F32)
    z[0, 0, 1] = z[0, 0, 0]                          # ray 0: bins_0 = z_0 = z_1, and u = 0 draws bins_0: a fine depth equal to two coarse ones
    u[0, 0, 0] = 0.0
    z[0, 1, 10:13] = z[0, 1, 10]                     # ray 1: a coarse depth three times
    u[0, 2, 8:16] = u[0, 2, 8]                       # ray 2: eight equal fine depths
    w[0, 3] = 0.0                                    # ray 3: all-zero weights (a uniform pdf through the + 1e-5)
    w[0, 4] = F32(-1e-5)                             # ray 4: weights + 1e-5 == 0 in every bin: w_sum == 0, every cdf entry 0
    u[0, 5, 0] = 1.0                                 # ray 5: u = 1 passes every cdf entry
    u[0, 5, 1] = np.nextafter(F32(1), F32(0))
    return z, w, u


@pytest.mark.parametrize('q7', [O.Q7_ZERO, O.Q7_CLAMP])
def test_resample_decisions_and_rank_with_ties(q7):
    z, w, u = resample_inputs()
    ref_all, ref_fine, ref_above, ref_below = O.hierarchical_depths(z, w, u, q7, return_indices=True)
    z_all, z_fine, above, below, rank = [t.cpu().numpy() for t in ops.resample(dev(z), dev(w), dev(u), q7, return_aux=True, return_rank=True)]
    # the inputs do what they are meant to
    assert (ref_fine[0, 0, 0] == z[0, 0, :2]).all() and (ref_fine[0, 2, 8:16] == ref_fine[0, 2, 8]).all()
    assert (np.abs((w[0, 4, 1:-1] + F32(1e-5))).sum() == 0) and (ref_above[0, 4] == 63).all()
    assert ref_above[0, 5, 0] == 63
    np.testing.assert_array_equal(above, ref_above)
    np.testing.assert_array_equal(below, ref_below)
    np.testing.assert_array_equal(z_fine, ref_fine)
    np.testing.assert_array_equal(z_all, ref_all)
    np.testing.assert_array_equal(rank, stable_rank(z, ref_fine))
    np.testing.assert_array_equal(np.take_along_axis(z_all, rank.astype(np.int64), -1), z_fine)
    assert list(rank[0, 2, 8:16]) == list(range(rank[0, 2, 8], rank[0, 2, 8] + 8))
