"""Range guard of the fp16 two-piece field kernel on the GPU: the status of the guarded kernel against a float64 reference
(tests/range_ref.py) wherever the maximum sits, bit-identical results with and without the guard, idle waves and accumulation, the
stash form, mvnerf_net_range, the per-call kernel choice, and the model's fallback / raise policies."""
import functools
import os
import warnings

import numpy as np
import pytest
import torch

from tests import range_ref as RR
from thesis_clip_nerf_amd import MVVNeRFRenderer, _lib, ops, render_view, train_nerf
from thesis_clip_nerf_amd.synthetic import make_scene, pinhole

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
PINNED = bool(os.environ.get('MVNERF_SPLIT_MFMA'))          # the variable pins ONE kernel for every call
needs_choice = pytest.mark.skipif(PINNED, reason='MVNERF_SPLIT_MFMA pins one kernel for every call: nothing to compare')

# Keras-order offsets (W0[379,128] b0 | 6 x (W1 b1 W2 b2) | Wr br)
B0, BLOCKS, BLOCK, WR = 379 * 128, 379 * 128 + 128, 2 * (128 * 128 + 128), 379 * 128 + 128 + 6 * 2 * (128 * 128 + 128)
W1, B1, W2, B2 = 0, 128 * 128, 128 * 128 + 128, 2 * 128 * 128 + 128
SCENE_KEYS = ['rays_o', 'rays_d', 'images', 'features', 'intrinsics', 'extrinsics_inv']


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def block(bi):
    return BLOCKS + bi * BLOCK


def planted(case, views, boost, n_rays=21, s=64):
    """Scene, net and depths with the largest cut activation where `case` puts it."""
    sc = make_scene(seed=40 + views, n_views=views, height=8, width=8, n_rays=n_rays, bias_scale=0.1)
    net = sc['coarse'].copy()
    feats = sc['features']
    if case == 'features':
        feats = (feats * np.float32(boost)).astype(np.float32)
    elif case == 'b0':
        net[B0 + 5] = boost
    elif case == 'hidden':                  # a per-view block's hidden layer alone: its second kernel is zero, so neither the residual
        net[block(1) + B1 + 7] = boost      # stream nor the output shows it
        net[block(1) + W2:block(1) + B2] = 0.0
    elif case == 'b2':                      # a fused block's output
        net[block(4) + B2 + 3] = boost
    else:
        assert case == 'none'
    rng = np.random.default_rng(7)
    z = np.sort(rng.uniform(0.3, 1.3, (1, n_rays, s)).astype(np.float32), -1)
    return dict(sc, features=feats), net, z


@functools.lru_cache(maxsize=None)
def reference(case, views, n_rays=21, s=64):
    """trunk64 of the boost-1e3 problem, computed once and shared."""
    sc, net, z = planted(case, views, 1e3, n_rays, s)
    return RR.trunk64(net, sc['rays_o'], sc['rays_d'], z, sc['images'], sc['features'], sc['intrinsics'], sc['extrinsics_inv'])


def device_problem(sc, net, z, table):
    d = [dev(sc[k]) for k in SCENE_KEYS]
    netd = dev(net)
    packed, split = ops.pack_net(netd), ops.pack_net_split(netd)
    tab = ops.project_texels(d[3], packed) if table else None
    return (d[0], d[1], dev(z), *d[2:], packed), split, tab


CASES = [(c, t) for t in (False, True) for c in ('features', 'b0', 'hidden', 'b2') if not (t and c == 'features')]


@needs_choice
@pytest.mark.parametrize('views', [1, 3])
@pytest.mark.parametrize('case,table', CASES)
def test_status_against_float64_reference(case, table, views):
    """R = 21: 42 tiles - five full workgroups and a partial one.  Boost 1e3: the status is the reference's maximum to the project's
    fp32 parity bar (1e-4, relative) and the guard changes no result bit.  Boost 5e6: the status says out of range."""
    sc, net, z = planted(case, views, 1e3)
    args, split, tab = device_problem(sc, net, z, table)
    status = torch.zeros(1, dtype=torch.float32, device=DEV)
    rgbs_g, emb_g = ops.field_eval_split(*args, split, return_embedding=True, texel_table=tab, kernel='split_f16', range_status=status)
    rgbs, emb = ops.field_eval_split(*args, split, return_embedding=True, texel_table=tab, kernel='split_f16')
    ref = RR.operand_max(reference(case, views), table)
    got = status.item()
    print(f'{case} table={table} V={views}: status {got!r} reference {ref!r} rel {abs(got - ref) / ref:.2e}')
    assert 900.0 < ref < _lib.F16X3_MAX_ACT
    assert abs(got - ref) <= 1e-4 * ref
    assert torch.equal(rgbs_g, rgbs) and torch.equal(emb_g, emb)

    sc, net, z = planted(case, views, 5e6)
    args, split, tab = device_problem(sc, net, z, table)
    status.zero_()
    ops.field_eval_split(*args, split, texel_table=tab, kernel='split_f16', range_status=status)
    got = status.item()
    print(f'{case} table={table} V={views}: status at boost 5e6 {got!r}')
    assert not np.isfinite(got) or got >= _lib.F16X3_MAX_ACT


@needs_choice
@pytest.mark.parametrize('table', [False, True])
@pytest.mark.parametrize('n_rays,s', [(3, 64), (3, 40)])
def test_idle_waves_partial_tile_and_accumulation(n_rays, s, table):
    """R = 3, S = 64: six tiles - one workgroup, two of its eight waves idle.  S = 40: 120 samples, the last tile a quarter empty (the
    per-lane path).  The status float sits between NaN guard floats; a preset above the true maximum stays."""
    sc, net, z = planted('b0', 1, 1e3, n_rays, s)
    args, split, tab = device_problem(sc, net, z, table)
    ref = RR.operand_max(reference('b0', 1, n_rays, s), table)
    buf = torch.tensor([float('nan'), 0.0, float('nan')], dtype=torch.float32, device=DEV)
    rgbs_g = ops.field_eval_split(*args, split, texel_table=tab, kernel='split_f16', range_status=buf[1:2])
    rgbs = ops.field_eval_split(*args, split, texel_table=tab, kernel='split_f16')
    got = buf.cpu().numpy()
    assert np.isnan(got[0]) and np.isnan(got[2])
    assert abs(got[1] - ref) <= 1e-4 * ref
    assert torch.equal(rgbs_g, rgbs)
    first = float(got[1])
    ops.field_eval_split(*args, split, texel_table=tab, kernel='split_f16', range_status=buf[1:2])     # accumulates: same maximum again
    assert buf[1].item() == first
    buf[1] = 4.0 * first
    ops.field_eval_split(*args, split, texel_table=tab, kernel='split_f16', range_status=buf[1:2])
    got = buf.cpu().numpy()
    assert got[1] == np.float32(4.0 * first) and np.isnan(got[0]) and np.isnan(got[2])
    # the kernels with the full range leave the status alone
    buf[1] = 0.0
    ops.field_eval_split(*args, split, texel_table=tab, kernel='split_bf16', range_status=buf[1:2])
    ops.field_eval_split(*args, split, texel_table=tab, kernel='split_bf16_32x32x16', range_status=buf[1:2])
    assert buf[1].item() == 0.0


@needs_choice
@pytest.mark.parametrize('views', [1, 3])
@pytest.mark.parametrize('table', [False, True])
def test_stash_form_status_is_the_stash_maximum(table, views):
    """The stash holds the very fp32 values that are cut: with the maximum planted in a hidden layer the status equals
    relu(stash).max() exactly, and the guarded stash is the unguarded one bit for bit."""
    sc, net, z = planted('hidden', views, 1e3)
    args, split, tab = device_problem(sc, net, z, table)
    status = torch.zeros(1, dtype=torch.float32, device=DEV)
    rgbs_g, stash_g = ops.field_eval_stash(*args, texel_table=tab, packed_split=split, kernel='split_f16', range_status=status)
    rgbs, stash = ops.field_eval_stash(*args, texel_table=tab, packed_split=split, kernel='split_f16')
    n = ops.stash_bytes(1, views, 21, 64) // 4
    slot = views * (21 * 64 // 32) * 4096
    keep = torch.ones(n, dtype=torch.bool, device=DEV)
    keep[6 * slot:7 * slot] = False                       # per-view slot 6 (x3) is not written
    a, b = stash_g.view(torch.float32)[:n][keep], stash.view(torch.float32)[:n][keep]
    assert torch.equal(a, b) and torch.equal(rgbs_g, rgbs)
    assert status.item() == a.clamp_min(0).max().item()
    ref = RR.stash_relu_max(reference('hidden', views))
    assert abs(status.item() - ref) <= 1e-4 * ref


def test_net_range_matches_numpy():
    base = make_scene(seed=3, height=8, width=8, n_rays=4, bias_scale=0.1)['fine']
    cut = np.zeros(base.size, dtype=bool)
    cut[:B0] = True
    for bi in range(6):
        cut[block(bi) + W1:block(bi) + B1] = True
        cut[block(bi) + W2:block(bi) + B2] = True
    assert cut.sum() == 379 * 128 + 12 * 128 * 128
    spots = {'pe row': 3 * 128 + 7, 'feature row': (123 + 10) * 128 + 5, 'last hidden': block(5) + B2 - 1, 'bias': B0, 'read-out': WR + 1}
    assert [bool(cut[i]) for i in spots.values()] == [True, True, True, False, False]
    out = ops.net_range(dev(base)).cpu().numpy()
    assert out[0] == np.abs(base[cut]).max() and out[1] == np.abs(base).max()
    for name, i in spots.items():
        for val in (2000.0, -2000.0):
            net = base.copy()
            net[i] = val
            out = ops.net_range(dev(net)).cpu().numpy()
            assert out[0] == np.abs(net[cut]).max() and out[1] == np.abs(net).max() == 2000.0, name
            assert (out[0] == 2000.0) == bool(cut[i]), name
        net[i] = np.nan
        out = ops.net_range(dev(net)).cpu().numpy()
        assert np.isnan(out[1]) and np.isnan(out[0]) == bool(cut[i]), name
        net[i] = np.inf
        out = ops.net_range(dev(net)).cpu().numpy()
        assert np.isinf(out[1]) and np.isinf(out[0]) == bool(cut[i]), name


def current_split_kernel():
    prev = ops.set_split_kernel('split_f16')
    ops.set_split_kernel(prev)
    return prev


@needs_choice
def test_per_call_choice_overrides_and_leaves_the_process_wide_value():
    sc, net, z = planted('none', 1, 1.0)
    args, split, tab = device_problem(sc, net, z, True)
    runs = {'field': lambda **kw: (ops.field_eval_split(*args, split, texel_table=tab, **kw),),
            'stash': lambda **kw: (ops.field_eval_stash(*args, texel_table=tab, packed_split=split, **kw)[0],)}
    sr = make_scene(seed=9, height=8, width=8, n_rays=32, bias_scale=0.1)
    d = {k: dev(sr[k]) for k in SCENE_KEYS + ['u_coarse', 'u_fine', 'coarse', 'fine']}
    pk = (ops.pack_net(d['coarse']), ops.pack_net(d['fine']))
    sp = (ops.pack_net_split(d['coarse']), ops.pack_net_split(d['fine']))
    runs['render'] = lambda **kw: ops.render_fwd(*[d[k] for k in SCENE_KEYS], *pk, d['u_coarse'], d['u_fine'], 0.3, 1.3, split=sp, **kw)
    for name, run in runs.items():
        want = {}
        for k in ('split_f16', 'split_bf16'):
            ops.set_split_kernel(k)
            want[k] = run()
        assert not all(torch.equal(a, b) for a, b in zip(want['split_f16'], want['split_bf16'])), name      # really two kernels
        for process_wide, per_call in (('split_bf16', 'split_f16'), ('split_f16', 'split_bf16')):
            ops.set_split_kernel(process_wide)
            got = run(kernel=per_call)
            assert all(torch.equal(a, b) for a, b in zip(got, want[per_call])), (name, per_call)
            assert current_split_kernel() == process_wide
    with pytest.raises(ValueError):
        runs['field'](kernel='tf32')


@needs_choice
def test_two_models_keep_their_own_kernels():
    sc = make_scene(seed=71, height=8, width=8, n_rays=32, bias_scale=0.05)
    inputs = tuple(sc[k] for k in ['rays_o', 'rays_d', 'images', 'intrinsics', 'extrinsics_inv'])
    u = dict(u_coarse=dev(sc['u_coarse']), u_fine=dev(sc['u_fine']))
    d = {k: dev(sc[k]) for k in SCENE_KEYS + ['coarse', 'fine']}
    pk = (ops.pack_net(d['coarse']), ops.pack_net(d['fine']))
    sp = (ops.pack_net_split(d['coarse']), ops.pack_net_split(d['fine']))
    models, want = {}, {}
    for gemm in ('split_f16', 'split_bf16'):
        models[gemm] = MVVNeRFRenderer(32, 32, n_views=1, near=sc['near'], far=sc['far'], device=DEV, f32_gemm=gemm)
        models[gemm].set_weights(sc['coarse'], sc['fine'])
        ops.set_split_kernel(gemm)                                    # the reference bits: the process-wide path
        want[gemm] = ops.render_fwd(*[d[k] for k in SCENE_KEYS], *pk, u['u_coarse'], u['u_fine'], sc['near'], sc['far'], split=sp,
                                    texel_tables='auto')         # as `_call` chooses
    ops.set_split_kernel('split_bf16_32x32x16')
    for _ in range(2):
        for gemm, m in models.items():
            got = m._call(inputs, 32, 1, sc['features'], **u)
            assert all(torch.equal(a, b) for a, b in zip(got, want[gemm])), gemm
            assert current_split_kernel() == 'split_bf16_32x32x16'


@needs_choice
def test_model_falls_back_or_raises_on_out_of_range_weights():
    sc = make_scene(seed=72, height=8, width=8, n_rays=32, bias_scale=0.05)
    fine = sc['fine'].copy()
    fine[block(0) + W1 + 5] = 2000.0
    inputs = tuple(sc[k] for k in ['rays_o', 'rays_d', 'images', 'intrinsics', 'extrinsics_inv'])
    u = dict(u_coarse=dev(sc['u_coarse']), u_fine=dev(sc['u_fine']))

    def model(**kw):
        m = MVVNeRFRenderer(32, 32, n_views=1, near=sc['near'], far=sc['far'], device=DEV, **kw)
        m.set_weights(sc['coarse'], fine)
        return m

    want = model(f32_gemm='split_bf16')._call(inputs, 32, 1, sc['features'], **u)
    m = model()
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter('always')
        got = m._call(inputs, 32, 1, sc['features'], **u)
        again = m._call(inputs, 32, 1, sc['features'], **u)
    assert [w.category for w in caught] == [RuntimeWarning] and '2000' in str(caught[0].message)
    assert all(torch.equal(a, b) for a, b in zip(got, want)) and all(torch.equal(a, b) for a, b in zip(again, want))
    assert m.range_report()['fine']['max_weight'] == 2000.0 and not m.range_report()['in_range']
    with pytest.raises(FloatingPointError, match='1023'):
        model(range_policy='raise')._call(inputs, 32, 1, sc['features'], **u)
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        model(range_policy='off')._call(inputs, 32, 1, sc['features'], **u)           # nobody looks
    with pytest.raises(ValueError):
        model(range_policy='sometimes')


def view_problem(boost=None):
    sc = make_scene(seed=73, height=8, width=8, bias_scale=0.05)
    rng = np.random.default_rng(1)
    colors = [rng.integers(0, 256, (8, 8, 3), dtype=np.uint8)]
    nets = [sc['coarse'].copy(), sc['fine'].copy()]
    if boost is not None:
        for n in nets:
            n[B0 + 5] = boost
    kw = dict(src_colors=colors,
              src_camera_configs=[{'pose': np.linalg.inv(sc['extrinsics_inv'][0, 0].astype(np.float64)), 'intrinsics': pinhole(8, 8).reshape(9)}],
              tgt_camera_config={'pose': sc['tgt_pose'][0], 'intrinsics': sc['tgt_intrinsics'].reshape(9)},
              combined_features=dev(sc['features']), chunk=24)              # 64 rays: chunks of 24, 24 and 16

    def model(**mk):
        m = MVVNeRFRenderer(64, 64, n_views=1, near=sc['near'], far=sc['far'], device=DEV, **mk)
        m.set_weights(*nets)
        return m

    gen = lambda: torch.Generator(device=DEV).manual_seed(5)
    return sc, nets, colors, kw, model, gen


@needs_choice
def test_render_view_range_check_falls_back_out_of_range():
    sc, nets, colors, kw, model, gen = view_problem(boost=5e6)
    want = render_view(model(f32_gemm='split_bf16'), generator=gen(), **kw)
    with pytest.warns(RuntimeWarning, match='split_bf16'):
        got = render_view(model(), generator=gen(), range_check=True, **kw)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    with pytest.raises(FloatingPointError, match='4.19e'):
        render_view(model(range_policy='raise'), generator=gen(), range_check=True, **kw)


@needs_choice
def test_render_view_range_check_in_range_matches_reference():
    sc, nets, colors, kw, model, gen = view_problem()
    want = render_view(model(), generator=gen(), **kw)
    m = model()
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        got = render_view(m, generator=gen(), range_check=True, **kw)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    rep = m.range_report()
    assert rep['in_range']
    # the reference: the frame's own depths (the op-level chain on the same uniforms, drawn chunk by chunk as render_view draws them)
    g, uc, uf = gen(), [], []
    for n in (24, 24, 16):
        uc.append(torch.rand((1, n, 64), dtype=torch.float32, device=DEV, generator=g))
        uf.append(torch.rand((1, n, 64), dtype=torch.float32, device=DEV, generator=g))
    uc, uf = torch.cat(uc, 1), torch.cat(uf, 1)
    pose = np.asarray(kw['tgt_camera_config']['pose'], dtype=np.float64)
    rays_o, rays_d = ops.get_rays_device(pose[:3, :3] @ np.linalg.inv(sc['tgt_intrinsics'][:3, :3]), pose[:3, 3], DEV, width=8, height=8)
    images = np.array([[colors[0] / 255.0]]).astype(np.float32)
    k4 = np.array([[np.asarray(m_) for m_ in [np.eye(4)]]], dtype=np.float32)
    k4[0, 0, :3, :3] = pinhole(8, 8)
    einv = np.linalg.inv(kw['src_camera_configs'][0]['pose'])[None, None].astype(np.float32)
    geo = (dev(images), dev(sc['features']), dev(k4), dev(einv))
    pc, pf = m.packed()
    z = ops.stratified_depths(uc, sc['near'], sc['far'])
    rgbs_c = ops.field_eval_split(rays_o[None], rays_d[None], z, *geo, pc, m.packed_split()[0], kernel='split_f16')
    z_all = ops.resample(z, ops.composite(z, rgbs_c)[2], uf)
    for name, net, zz in (('coarse', nets[0], z), ('fine', nets[1], z_all)):
        t = RR.trunk64(net, rays_o[None].cpu().numpy(), rays_d[None].cpu().numpy(), zz.cpu().numpy(), images, sc['features'], k4, einv)
        ref = RR.operand_max(t, table=True)                           # a frame in chunks runs the texel-table form
        print(f'{name}: report {rep[name]["max_activation"]!r} reference {ref!r}')
        assert abs(rep[name]['max_activation'] - ref) <= 1e-4 * ref


@needs_choice
def test_check_range_flags_what_only_the_backward_cannot_take():
    sc = make_scene(seed=74, height=8, width=8, n_rays=32, bias_scale=0.05)
    coarse = sc['coarse'].copy()
    coarse[block(1) + B1 + 7] = 2000.0
    coarse[block(1) + W2:block(1) + B2] = 0.0
    m = MVVNeRFRenderer(32, 32, n_views=1, near=sc['near'], far=sc['far'], device=DEV)
    m.set_weights(coarse, sc['fine'])
    inputs = tuple(sc[k] for k in ['rays_o', 'rays_d', 'images', 'intrinsics', 'extrinsics_inv'])
    u = dict(u_coarse=dev(sc['u_coarse']), u_fine=dev(sc['u_fine']))
    rep = m.check_range(inputs, sc['features'], training=True, **u)
    assert not rep['in_range'] and rep['limit'] == _lib.F16X3_MAX_WEIGHT and '1023' in rep['message']
    assert 2000.0 <= rep['coarse']['max_activation'] < 2100.0 and rep['fine']['max_activation'] < 1023.0
    assert m.check_range(inputs, sc['features'], training=False, **u)['in_range']          # the forward allows it
    with pytest.raises(FloatingPointError, match='1023'):
        train_nerf.check_training_range(m, (inputs, sc['features']))
    fine_model = MVVNeRFRenderer(32, 32, n_views=1, near=sc['near'], far=sc['far'], device=DEV)
    fine_model.set_weights(sc['coarse'], sc['fine'])
    assert train_nerf.check_training_range(fine_model, (inputs, sc['features']))['in_range']


def test_load_backbone_warns_about_out_of_range_weights(tmp_path):
    from thesis_clip_nerf_amd.lmvnerf import LanguageNeRF
    sc = make_scene(seed=75, height=8, width=8, n_rays=4, bias_scale=0.05)
    fine = sc['fine'].copy()
    renderer = MVVNeRFRenderer(4, 4, n_views=1, device=DEV)
    model = LanguageNeRF(sc['coarse'], n_views=1, device=DEV)
    renderer.set_weights(sc['coarse'], fine)
    renderer.store(str(tmp_path / 'ok'))
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        assert model.load_backbone(str(tmp_path / 'ok'))
    fine[block(3) + W2 + 9] = -2000.0
    renderer.set_weights(sc['coarse'], fine)
    renderer.store(str(tmp_path / 'big'))
    with pytest.warns(RuntimeWarning, match='1023'):
        assert model.load_backbone(str(tmp_path / 'big'))
    assert torch.equal(model.trunk_net.detach(), dev(fine))
