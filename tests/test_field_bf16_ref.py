"""oracle/field_bf16_ref.py without a GPU: the block-local float64 references and their one assertion (`check`) against the fp32 NumPy
restatement of the bf16 field pass (O.mv_embedding(emulate_bf16=True)), which stands in for the kernels here.

* the checker passes on the restatement: six blocks, layer 0 (direct and texel-table form), read-out (bf16 and fp32), texel table;
* the checker is sensitive: five mutations of the restated block, each a defect that shifts results by 1e-3 ... 1e-4 and passes
  every bar of tests/test_gpu_bf16.py, make `check` fail;
* bf16_ulp / boundary_distance against torch.bfloat16 casts."""
import numpy as np
import pytest
import torch

from oracle import field_bf16_ref as R
from oracle import mvnerf_oracle as O
from thesis_clip_nerf_amd.synthetic import make_scene

F32 = np.float32
GEO = ('images', 'features', 'intrinsics', 'extrinsics_inv')
SCENES = {'v1_24x24': dict(seed=61, n_views=1, height=24, width=24, n_rays=40, s=64),
          'v2_9x13': dict(seed=5, n_views=2, height=9, width=13, n_rays=17, s=33)}
_cache = {}


def restated(name):
    """The scene, its fine net and the fp32 restatement's activations [x0, f1, f2, f3, mean, u1, u2, u3] as rows; computed once."""
    if name in _cache:
        return _cache[name]
    cfg = dict(SCENES[name])
    s = cfg.pop('s')
    sc = make_scene(bias_scale=0.1, **cfg)
    v, r = cfg['n_views'], cfg['n_rays']
    net = O.unflatten_net(sc['fine'])
    z = np.sort(np.random.default_rng(0).uniform(0.3, 1.3, (1, r, s)).astype(F32), -1)
    world = O.points_on_rays(sc['rays_o'], sc['rays_d'], z)
    pix, cam = O.compute_pixel_in_image_mv(world, sc['intrinsics'], sc['extrinsics_inv'])
    norm_images = (sc['images'].astype(F32) * F32(2) - F32(1)).astype(F32)
    feat = O.get_projection_features_mv(norm_images, sc['features'], pix)
    cdir = O.world_to_camera_direction_vector_mv(sc['rays_d'], sc['extrinsics_inv'])
    cdir = np.broadcast_to(cdir[:, :, :, None, :], cam.shape[:-1] + (3,))
    xyz = cam[..., :3].reshape(v, r, s, 3)
    acts = O.mv_embedding(net, xyz, cdir.reshape(v, r, s, 3), feat.reshape(v, r, s, -1), v, complete_output=True, emulate_bf16=True)
    acts = [a.reshape(-1, 128) for a in acts]
    # the texel-table form of layer 0: bf16 PE / rgb rows on the seed, plus an fp32 lerp of the rows of a bf16-product table
    table = (O.bf16_round(sc['features']) @ O.bf16_round(net['W0'][123:])).astype(F32)                 # (1,V,H,W,128)
    h, w = table.shape[2:4]
    lerp = O.interpolate_bilinear_xy(table.reshape(v, h, w, 128), pix.reshape(v, r * s, 2)).reshape(-1, 128)
    small = np.concatenate([O.position_encoding(xyz), feat.reshape(v, r, s, -1)[..., :3]], -1).reshape(-1, 63)
    w_small = np.concatenate([net['W0'][:60], net['W0'][120:123]], 0)
    seed = (O.position_encoding(cdir.reshape(v, r, s, 3)).reshape(-1, 60) @ net['W0'][60:120] + net['b0']).astype(F32)
    x0_table = ((O.bf16_round(small) @ O.bf16_round(w_small) + seed).astype(F32) + lerp).astype(F32)
    _cache[name] = dict(sc=sc, net=net, z=z, acts=acts, table=table, x0_table=x0_table)
    return _cache[name]


@pytest.mark.parametrize('name', list(SCENES))
def test_check_passes_on_the_restated_blocks(name):
    d = restated(name)
    for k, blk in zip((0, 1, 2, 4, 5, 6), d['net']['blocks']):
        R.check(d['acts'][k + 1], *R.block_ref(d['acts'][k], blk), f'{name} block {k}')


@pytest.mark.parametrize('name', list(SCENES))
def test_check_passes_on_the_restated_layer0_readout_and_table(name):
    d = restated(name)
    sc, net = d['sc'], d['net']
    args = (net, sc['rays_o'], sc['rays_d'], d['z']) + tuple(sc[k] for k in GEO)
    R.check(d['acts'][0], *R.layer0_ref(*args, pe_direct=None, fused_lerp=False), f'{name} layer 0 direct')
    R.check(d['x0_table'], *R.layer0_ref(*args, table=d['table'], pe_direct=None), f'{name} layer 0 table')
    emb = d['acts'][7]
    for rounded in (True, False):
        rgb, sigma = O.render_readout(net, emb, emulate_bf16=rounded)
        R.check(np.concatenate([rgb, sigma[:, None]], -1), R.readout_ref(emb, net, rounded), name=f'{name} read-out bf16={rounded}')
    R.check(d['table'].reshape(-1, 128), R.table_ref(sc['features'], net['W0']).reshape(-1, 128), name=f'{name} table')


def test_kernel_pe_restates_the_position_encoding():
    """sincos_f32 restated in NumPy against numpy's own fp32 sin / cos at the project's bar (test_sincos_matches_oracle_pe), and the
    double-angle octaves within the x16 error growth that field_eval.hip:124-126 states."""
    x = np.random.default_rng(1).uniform(-1.5, 1.5, (4096, 3)).astype(F32)
    ref = O.position_encoding(x)
    assert np.abs(R.kernel_pe(x, direct=range(10)) - ref).max() < 4e-7
    for direct in ((0, 5), (0, 5, 8)):
        assert np.abs(R.kernel_pe(x, direct) - ref).max() < 16 * 4e-7


def test_table_rows_inverts_the_accumulator_order():
    feat = np.arange(128)
    stored = np.empty(128, np.int64)
    for h in range(2):
        for nb in range(4):
            for qq in range(4):
                for c in range(4):
                    stored[64 * h + 16 * nb + 4 * qq + c] = 32 * nb + 8 * qq + 4 * h + c
    np.testing.assert_array_equal(R.table_rows(stored[None])[0], feat)


# ---- sensitivity: mutations of the restated block ----------------------------------------------------------------------------
def bf16_truncate(a):
    return (np.ascontiguousarray(a, dtype=F32).view(np.uint32) & np.uint32(0xFFFF0000)).view(F32).reshape(np.shape(a))


def bf16_half_up(a):
    """add half a step to the magnitude and truncate: differs from nearest-even only on exact ties"""
    u = np.ascontiguousarray(a, dtype=F32).view(np.uint32).astype(np.uint64)
    return (((u + 0x8000) >> 16) << 16).astype(np.uint32).view(F32).reshape(np.shape(a))


def block_restated(x, blk, rnd_w=O.bf16_round, rnd_hid=O.bf16_round, zero_k=None, bias_after_relu=False, no_residual=None):
    """O.resnet_block(rnd=bf16_round) in fp32 with one defect switched on."""
    w1, b1, w2, b2 = blk
    if zero_k is not None:
        w1 = w1.copy()
        w1[zero_k] = 0
    hid = (O.bf16_round(np.maximum(x, 0)) @ rnd_w(w1)).astype(F32)
    act = (np.maximum(hid, 0) + b1).astype(F32) if bias_after_relu else np.maximum((hid + b1).astype(F32), 0)
    res = x.copy()
    if no_residual is not None:
        res[:, no_residual] = 0
    return (res + (rnd_hid(act) @ rnd_w(w2) + b2).astype(F32)).astype(F32)


MUTATIONS = {'weights truncated': dict(rnd_w=bf16_truncate),
             'k-row 77 of W1 zeroed': dict(zero_k=77),
             'b1 after the relu': dict(bias_after_relu=True),
             'residual dropped for 16 features': dict(no_residual=slice(48, 64))}


@pytest.mark.parametrize('k', [0, 5])
def test_check_fails_on_each_mutation(k):
    d = restated('v1_24x24')
    x, blk = d['acts'][k], d['net']['blocks'][k if k < 3 else k - 1]
    ref = R.block_ref(x, blk)
    R.check(block_restated(x, blk), *ref, f'block {k} unmutated')
    for name, kw in MUTATIONS.items():
        with pytest.raises(AssertionError):
            R.check(block_restated(x, blk, **kw), *ref, f'block {k} {name}')


def test_check_fails_on_round_half_up_of_relu_hid():
    """Half-up differs from nearest-even only on exact ties, which a real block meets in 2^-16 of its elements - and a tie is inside
    every window.  What catches it is the over-bar cap: on a block whose first GEMM is exact (dyadic x and W1: products are multiples
    of 2^-21 and sums of |products| stay below 2^3, so fp32 and float64 agree bit for bit in any order), ties are frequent enough to count: the
    nearest-even block matches the reference on every tie, the half-up block is one bf16 step off on half of them."""
    d = restated('v1_24x24')
    rng = np.random.default_rng(3)
    x = (rng.integers(-256, 257, (4096, 128)) / 256.0).astype(F32)                      # multiples of 2^-8, |x| <= 1: bf16 values
    k = rng.choice(np.r_[64:256, 256:512:2, 512:1024:4], (128, 128))                              # 8 significant bits: bf16 values as well
    w1 = (rng.choice([-1.0, 1.0], (128, 128)) * k / 8192.0).astype(F32)                 # multiples of 2^-13, 1/128 <= |w| < 1/8
    assert np.array_equal(O.bf16_round(x), x) and np.array_equal(O.bf16_round(w1), w1)
    assert (np.maximum(x, 0) @ np.abs(w1)).max() < 8.0
    _, _, w2, b2 = d['net']['blocks'][0]
    blk = (w1, np.zeros(128, F32), w2, b2)
    ref, und, flip = R.block_ref(x, blk)
    ties = (R.boundary_distance(np.maximum(x, 0).astype(np.float64) @ w1.astype(np.float64)) == 0) & und
    assert 0.04 < ties.any(1).mean() < 0.20, ties.any(1).mean()
    R.check(block_restated(x, blk), ref, und, flip, 'exact block, nearest even')
    with pytest.raises(AssertionError, match='over-bar share'):
        R.check(block_restated(x, blk, rnd_hid=bf16_half_up), ref, und, flip, 'exact block, half up')


# ---- helpers -----------------------------------------------------------------------------------------------------------------
def _bf16(x):
    return torch.from_numpy(np.asarray(x, np.float64)).to(torch.float32).to(torch.bfloat16).to(torch.float64).numpy()


def _sweep():
    """bf16 values across the exponent range - powers of two, ordinary cells, subnormals, zero - as (value, next value up)."""
    lows = []
    for e in (-133, -132, -130, -127, -126, -125, -60, -8, -1, 0, 1, 7, 100, 126):
        base = 2.0 ** max(e, -126)
        step = 2.0 ** (max(e, -126) - 7)
        for m in ((0, 1, 77, 127) if e >= -126 else (0,)):
            lows.append((base + m * step) if e >= -126 else 2.0 ** e)
    lows.append(0.0)
    return np.array(lows)


def test_bf16_ulp_is_the_spacing_of_torch_bfloat16():
    lo = _sweep()
    assert np.array_equal(_bf16(lo), lo)                                                # the sweep holds bf16 values
    u = R.bf16_ulp(lo)
    assert np.array_equal(_bf16(lo + u), lo + u)                                        # lo + ulp is the next bf16 value ...
    for frac in (0.26, 0.49):
        assert np.array_equal(_bf16(lo + frac * u), lo)                                 # ... nothing representable lies between
    for frac in (0.51, 0.74):
        assert np.array_equal(_bf16(lo + frac * u), lo + u)
    assert np.array_equal(R.bf16_ulp(-lo), u)
    assert np.array_equal(R.bf16_ulp(lo + 0.3 * u), u)
    assert np.array_equal(R.q(lo + 0.3 * u), lo) and np.array_equal(R.q(lo + 0.7 * u), lo + u)


def test_boundary_distance_is_where_the_torch_bfloat16_cast_changes():
    lo = _sweep()
    u = R.bf16_ulp(lo)
    for frac in (0.0, 0.1, 0.25, 0.4, 0.6, 0.75, 0.9):
        for sign in (1.0, -1.0):
            x = sign * (lo + frac * u)
            d = R.boundary_distance(x)
            assert (d > 0).all()
            here = _bf16(x)
            for step in (-0.98, 0.98):                                                  # inside the cell: the same bf16 value
                assert np.array_equal(_bf16(x + step * d), here), (frac, sign, step)
            moved = (_bf16(x + 1.02 * d) != here) | (_bf16(x - 1.02 * d) != here)       # just past the nearest boundary: another one
            assert moved.all(), (frac, sign, x[~moved])
    assert np.array_equal(R.boundary_distance(lo + 0.5 * u), np.zeros_like(lo))
    pow2 = np.array([2.0 ** -60, 1.0, 2.0, 2.0 ** 100])
    np.testing.assert_array_equal(R.boundary_distance(pow2), R.bf16_ulp(pow2) / 4)      # the narrower cell below is the nearer one
