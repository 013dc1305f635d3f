"""oracle/field_f32_ref.py on the CPU: the float64 section references of the fp32-grade forward kernels are right, their bars are met
by a faithful emulation of the default kernel's arithmetic, and planted defects exceed them.  The GPU module that holds the kernels
themselves to the same references and bars is not in the suite yet (DESIGN.md 4.0c has its measured figures and the reason).

  1. The references agree with the NumPy fp32 oracle (O.mv_embedding(complete_output=True), O.render_readout) within the seq32
     yardstick - a reference that is wrong (a row order, a weight slice, the view mean, the table order) fails here.
  2. `emulate_f16x3` (exact piece products, float64 sums) passes the hidden and the layer-0 bar at scale 1; at the 2^-12 scale of the
     GPU sweep it EXCEEDS the pure relative bar and stays under bar + `f16_floor`: the sweep reaches the regime, the floor is right.
  3. Planted defects, all emulated in NumPy, each exceed their bar (figures in units of 2^-24 max |ref| are printed).

NOT detectable at these bars, by the same emulation (test_defects_below_the_bars prints the figures): activation pieces converted by
truncation instead of round-to-nearest (about 2.4 x 2^-24 max |ref| on a hidden Dense), and PE octaves 8 and 9 formed by doubling from
octave 5 instead of an accurate sin / cos at octave 8 (about 5 on layer 0) - both sit inside the fp32 noise the bars allow."""
import functools

import numpy as np
import pytest

from oracle import field_f32_ref as R
from oracle import mvnerf_oracle as O
from thesis_clip_nerf_amd.synthetic import make_scene

F32, F64 = np.float32, np.float64
GEO = ('images', 'features', 'intrinsics', 'extrinsics_inv')
SHAPES = [(1, 1, 1), (1, 17, 33), (1, 40, 64), (3, 17, 33)]          # (views, rays, samples): the shapes of the GPU measurement


@functools.lru_cache(maxsize=None)
def scene(views, n_rays, s):
    """The scenes of tests/test_gpu_bf16_grade.py (24x24 maps, bias_scale 0.1, z sorted uniform in [0.3, 1.3]) with the oracle's eight
    complete_output activations; computed once per shape."""
    sc = make_scene(seed=61 + views, n_views=views, height=24, width=24, n_rays=n_rays, bias_scale=0.1)
    sc['z'] = np.sort(np.random.default_rng(0).uniform(0.3, 1.3, (1, n_rays, s)).astype(F32), -1)
    net = O.unflatten_net(sc['fine'])
    world = O.points_on_rays(sc['rays_o'], sc['rays_d'], sc['z'])
    pix, cam = O.compute_pixel_in_image_mv(world, sc['intrinsics'], sc['extrinsics_inv'])
    feat = O.get_projection_features_mv((sc['images'] * F32(2) - F32(1)).astype(F32), sc['features'], pix)
    cdir = O.world_to_camera_direction_vector_mv(sc['rays_d'], sc['extrinsics_inv'])
    cdir = np.broadcast_to(cdir[:, :, :, None, :], cam.shape[:-1] + (3,))
    flat = lambda a: a.reshape(views, n_rays, s, a.shape[-1])                      # B = 1: (B*V, R, S, .)
    sc['acts'] = [a.reshape(-1, 128) for a in O.mv_embedding(net, flat(cam[..., :3]), flat(cdir), flat(feat), views, complete_output=True)]
    sc['net'] = net
    return sc


def parts(sc, **kw):
    return R.layer0_parts(sc['net'], sc['rays_o'], sc['rays_d'], sc['z'], *(sc[k] for k in GEO), **kw)


def over(got, ref, bar):
    """Worst |got - ref| as a share of the bar (> 1: the check fails) and in units of 2^-24 max |ref|."""
    err = np.abs(np.asarray(got, F64) - ref)
    return float((err / bar).max()), float(err.max() / (R.EPS * np.abs(ref).max()))


# ---- 1. the references against the fp32 oracle -------------------------------------------------------------------------------------
@pytest.mark.parametrize('views,n_rays,s', SHAPES)
def test_references_agree_with_the_fp32_oracle(views, n_rays, s):
    sc = scene(views, n_rays, s)
    net, acts = sc['net'], sc['acts']
    name = f'V={views} {n_rays}x{s}'
    # layer 0: both accurate-octave sets, direct and table form (the table: float64 product rounded to fp32, as a kernel would hold it),
    # against the oracle's x0 at the direct form's bar - the oracle's own K = 379 fp32 sum is what seq32 measures
    p = parts(sc)
    bar, _ = R.layer0_bar(R.layer0_from_parts(*p), *p)
    table = R.table_ref(sc['features'], net['W0']).astype(F32)
    for direct in ((0, 5), (0, 5, 8)):
        R.check(acts[0], R.layer0_from_parts(*parts(sc, pe_direct=direct)), bar, f'{name} layer 0 direct, octaves {direct}')
        R.check(acts[0], R.layer0_from_parts(*parts(sc, pe_direct=direct, table=table)), bar, f'{name} layer 0 table, octaves {direct}')
    for k, blk in zip((0, 1, 2, 4, 5, 6), net['blocks']):
        ref = R.block_ref(acts[k], blk)
        R.check(acts[k + 1], ref, R.bar16(ref), f'{name} block {k}')
    mean, bar = R.view_mean_ref(acts[3].reshape(views, -1, 128))
    R.check(acts[4], mean, bar, f'{name} view mean')
    if views == 1:
        assert np.array_equal(acts[4], acts[3])
    rgb, sigma = O.render_readout(net, acts[7])
    ref, bar, _ = R.readout_bars(acts[7], net)
    R.check(np.concatenate([rgb, sigma[:, None]], -1), ref, bar, f'{name} read-out')


def test_decode_stash_and_table_rows_are_the_reused_ones():
    """The module re-exports, it does not copy."""
    from oracle import field_backward_ref, field_bf16_ref
    assert R.decode_stash is field_backward_ref.decode_stash and R.table_rows is field_bf16_ref.table_rows
    assert R.kernel_pe is field_bf16_ref.kernel_pe and R.readout_ref is field_bf16_ref.readout_ref


# ---- 2. the emulation of the fp16 form: passes at scale 1, meets the floor below ----------------------------------------------------
def hidden_problem(k=0):
    """Block 0's first Dense of the fine net on the oracle's x0 (seed 62, V = 1, 17 x 33), inputs and bias scaled by 2^-k."""
    sc = scene(1, 17, 33)
    w1, b1 = sc['net']['blocks'][0][:2]
    x = (sc['acts'][0] * F32(2.0 ** -k)).astype(F32)
    b1 = (b1 * F32(2.0 ** -k)).astype(F32)
    return x, w1, b1, R.dense_ref(x, w1, b1)


@pytest.mark.parametrize('k', [0, 6, 12])
def test_emulated_f16x3_hidden_dense_passes_at_scale_1_and_meets_the_floor_below(k):
    x, w1, b1, ref = hidden_problem(k)
    a = np.maximum(x, 0)
    got = R.emulate_f16x3(a, w1) + b1.astype(F64)
    bar, floor = R.bar16(ref), R.f16_floor(a, w1)
    share, units = over(got, ref, bar)
    share_floor, _ = over(got, ref, bar + floor)
    print(f'hidden Dense, scale 2^-{k}: max |act| {np.abs(x).max():.3g}, worst {units:.1f} x 2^-24 max |ref|, share of bar + floor {share_floor:.3f}, '
          f'max |err| {np.abs(got - ref).max():.2e}, max floor {floor.max():.2e}')
    assert share_floor <= 1.0
    if k == 0:
        assert share <= 1.0                      # scale 1: the pure relative bar holds
    if k == 12:
        assert share > 1.0                       # the sweep reaches the regime where it cannot


@pytest.mark.parametrize('k', [0, 12])
@pytest.mark.parametrize('table', [False, True])
def test_emulated_f16x3_layer0_passes_at_scale_1_and_meets_the_floor_below(table, k):
    sc = scene(1, 17, 33)
    net = O.unflatten_net(R.scale_net(sc['fine'], k))
    tab = R.table_ref(sc['features'], net['W0']).astype(F32) if table else None
    seed, inp, w, extra = R.layer0_parts(net, sc['rays_o'], sc['rays_d'], sc['z'], *(sc[g] for g in GEO), table=tab, pe_direct=(0, 5, 8))
    ref = R.layer0_from_parts(seed, inp, w, extra)
    got = seed + R.emulate_f16x3(inp, w) + extra
    bar = R.bar16(ref) if table else R.layer0_bar(ref, seed, inp, w)[0]
    share, units = over(got, ref, bar)
    share_floor, _ = over(got, ref, bar + R.f16_floor(inp, w))
    print(f'layer 0 table={table}, scale 2^-{k}: worst {units:.1f} x 2^-24 max |ref|, share of the bar {share:.3f}, of bar + floor {share_floor:.3f}')
    assert share_floor <= 1.0
    if k == 0:
        assert share <= 1.0


def test_scale_net_is_exactly_homogeneous():
    """net_k's float64 trunk is 2^-k times net_0's: only W0, b0 and the hidden biases are scaled."""
    sc = scene(1, 17, 33)
    x = {}
    for k in (0, 12):
        net = O.unflatten_net(R.scale_net(sc['fine'], k))
        x[k] = R.block_ref(R.block_ref(R.layer0_from_parts(*R.layer0_parts(net, sc['rays_o'], sc['rays_d'], sc['z'], *(sc[g] for g in GEO))).astype(F32),
                                       net['blocks'][0]).astype(F32), net['blocks'][1])
        assert np.array_equal(net['Wr'], sc['net']['Wr']) and np.array_equal(net['blocks'][3][0], sc['net']['blocks'][3][0])
    assert np.array_equal(x[12] * 2.0 ** 12, x[0])


# ---- 3. planted defects ---------------------------------------------------------------------------------------------------------------
def test_a_dropped_piece_product_in_one_k_step_of_a_hidden_dense_exceeds_the_bar():
    """A1 B0 left out in one k-step (32 inputs) on one 16-feature row block."""
    x, w1, b1, ref = hidden_problem()
    got = R.emulate_f16x3(np.maximum(x, 0), w1, drop=('A1B0', slice(32, 64), slice(16, 32))) + b1.astype(F64)
    share, units = over(got, ref, R.bar16(ref))
    print(f'A1 B0 dropped in one hidden k-step: {units:.0f} x 2^-24 max |ref|')
    assert share > 4.0


@pytest.mark.parametrize('term', ['A1B0', 'A0sB1'])
def test_a_dropped_piece_product_in_one_feature_k_step_of_layer0_exceeds_the_bar(term):
    sc = scene(1, 17, 33)
    seed, inp, w, extra = parts(sc, pe_direct=(0, 5, 8))
    ref = R.layer0_from_parts(seed, inp, w, extra)
    got = seed + R.emulate_f16x3(inp, w, drop=(term, slice(63 + 32, 63 + 64), slice(16, 32)))
    share, units = over(got, ref, R.layer0_bar(ref, seed, inp, w)[0])
    print(f'{term} dropped in one feature k-step of layer 0: {units:.0f} x 2^-24 max |ref|')
    assert share > 4.0


def test_flushed_fp16_subnormals_exceed_the_bar():
    x, w1, b1, ref = hidden_problem()
    got = R.emulate_f16x3(np.maximum(x, 0), w1, flush=True) + b1.astype(F64)
    share, units = over(got, ref, R.bar16(ref))
    print(f'fp16 subnormal pieces flushed: {units:.0f} x 2^-24 max |ref|')
    assert share > 4.0


def test_a_view_left_out_of_the_mean_exceeds_the_bar():
    sc = scene(3, 17, 33)
    xv = sc['acts'][3].reshape(3, -1, 128)
    mean, bar = R.view_mean_ref(xv)
    assert (np.abs(xv[:2].astype(F64).mean(0) - mean) > bar).mean() > 0.9
    assert (np.abs(xv.astype(F64).sum(0) / 2 - mean) > bar).mean() > 0.9          # divided by the wrong count
    with pytest.raises(AssertionError):
        R.check(xv[:2].astype(F64).mean(0), mean, bar, 'mean of two of three views')


def test_readout_defects_exceed_the_bars():
    """No relu in front of the read-out; one of the four lane groups' partial sums lost (the 16x16x32 kernels: lane group g holds
    features 16 rb + 4 g + {0..3})."""
    sc = scene(1, 17, 33)
    net, emb = sc['net'], sc['acts'][7]
    act = lambda o: np.concatenate([1.0 / (1.0 + np.exp(-o[:, :3])), np.logaddexp(0.0, o[:, 3:])], -1)
    wr, br = net['Wr'].astype(F64), net['br'].astype(F64)
    R.check_readout(act(np.maximum(emb.astype(F64), 0) @ wr + br), emb, net, 'faithful read-out')
    with pytest.raises(AssertionError):
        R.check_readout(act(emb.astype(F64) @ wr + br), emb, net, 'read-out without the relu')
    lost = (np.arange(128) % 16) // 4 == 2
    with pytest.raises(AssertionError):
        R.check_readout(act(np.maximum(emb.astype(F64), 0)[:, ~lost] @ wr[~lost] + br), emb, net, 'read-out less one lane group')
    with pytest.raises(AssertionError):                                            # the bias forgotten
        R.check_readout(act(np.maximum(emb.astype(F64), 0) @ wr), emb, net, 'read-out without the bias')


def test_the_neighbouring_rays_seed_exceeds_the_bar():
    sc = scene(1, 17, 33)
    p = parts(sc)
    ref = R.layer0_from_parts(*p)
    share, units = over(R.layer0_from_parts(*parts(sc, ray_shift=1)), ref, R.layer0_bar(ref, *p)[0])
    print(f'seed of the neighbouring ray: {units:.0f} x 2^-24 max |ref|')
    assert share > 4.0


def test_a_table_lerp_with_exchanged_factors_exceeds_the_bar():
    sc = scene(1, 17, 33)
    table = R.table_ref(sc['features'], sc['net']['W0']).astype(F32)
    ref = R.layer0_from_parts(*parts(sc, table=table))
    share, units = over(R.layer0_from_parts(*parts(sc, table=table, swap_lerp=True)), ref, R.bar16(ref))
    print(f'table lerp with ax and ay exchanged: {units:.0f} x 2^-24 max |ref|')
    assert share > 4.0


def test_a_wrong_texel_table_exceeds_the_bar():
    """A table in accumulator order read as if in feature order; a table from W0 rows shifted by one."""
    sc = scene(1, 17, 33)
    w0 = sc['net']['W0']
    ref = R.table_ref(sc['features'], w0).reshape(-1, 128)
    assert not np.array_equal(R.table_rows(ref), ref)
    with pytest.raises(AssertionError):
        R.check(R.table_rows(ref), ref, R.bar16(ref), 'table in the wrong order')
    with pytest.raises(AssertionError):
        R.check((sc['features'].astype(F64) @ w0[122:378].astype(F64)).reshape(-1, 128), ref, R.bar16(ref), 'table of shifted rows')


def rz16(x):
    """fp32 -> fp16 by truncation (round toward zero)."""
    h = x.astype(np.float16)
    return np.where(np.abs(h.astype(F32)) > np.abs(x), np.nextafter(h, np.float16(0)), h)


def test_defects_below_the_bars():
    """Recorded, not detected: both figures sit inside the fp32 noise that the bars allow (module docstring)."""
    x, w1, b1, ref = hidden_problem()
    a = np.maximum(x, 0)
    a0, a0s, a1, _, _ = R.split_weight(w1)
    b0 = rz16((a * F32(1 / 64)).astype(F32))
    b1p = rz16((a - F32(64) * b0.astype(F32)).astype(F32))
    f = lambda t: t.astype(F64)
    got = f(b1p) @ f(a0s) + f(b0) @ f(a1) + f(b0) @ f(a0) + b1.astype(F64)
    share, units = over(got, ref, R.bar16(ref))
    print(f'activation pieces by truncation: {units:.1f} x 2^-24 max |ref| (share of the bar {share:.2f})')
    assert share < 1.0
    sc = scene(1, 17, 33)
    p = parts(sc, pe_direct=(0, 5, 8))
    ref = R.layer0_from_parts(*p)
    share, units = over(R.layer0_from_parts(*parts(sc, pe_direct=(0, 5))), ref, R.layer0_bar(ref, *p)[0])
    print(f'PE octaves 8 and 9 by doubling from 5: {units:.1f} x 2^-24 max |ref| (share of the bar {share:.2f})')
    assert share < 1.0
