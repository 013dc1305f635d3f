"""The bf16 field kernels at rounding-level bars (oracle/field_bf16_ref.py): every block is recomputed in float64 FROM THE KERNEL'S OWN
INPUT of that block, the one rounding that cannot be shared (bf16(relu(hid))) is bounded by an undecided window, and `R.check` holds
|got - ref| to 16 * 2^-24 * max |ref| (+ the flip bound of undecided elements only).  tests/test_gpu_bf16.py keeps the end-to-end bars.

  a. fusion blocks 4, 5, 6 and the read-out of all four kernel variants, from return_fused_acts of one launch;
  b. layer 0 and the per-view blocks 0, 1, 2 at V = 1 through knock-out nets (a block with W2 = b2 = 0 is an exact identity);
  c. the view mean at V = 2, 3 against single-view launches; the fusion half of the multi-view instantiations;
  d. project_texels_bf16 (one / two nets, fp32 / bf16 maps) against q(features) @ q(W0[123:379]);
  e. the packed bf16 streams hold round-to-nearest-even weights.
MVNERF_BF16_KERNEL = segments | layers pins the kernel of a call (test_bf16_layer_ring_kernel_agrees_with_the_segment_ring_kernel)."""
import os
import re

import numpy as np
import pytest
import torch

from oracle import field_bf16_ref as R
from oracle import mvnerf_oracle as O
from thesis_clip_nerf_amd import ops
from thesis_clip_nerf_amd.synthetic import make_scene

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
GEO = ('images', 'features', 'intrinsics', 'extrinsics_inv')
SHAPES = [(1, 1), (17, 33), (40, 64)]          # a single sample; ragged wave tile and ragged workgroup group; ten whole tiles
# kernel variant -> (MVNERF_BF16_KERNEL, table form, views).  `layers` sends V > 1 to the layer-ring kernel too.
VARIANTS = {'segment-direct': ('segments', False, 1), 'segment-table': ('segments', True, 1),
            'layer-table-v1': ('layers', True, 1), 'layer-table-v3': ('layers', True, 3)}
PE_DIRECT = {'segments': (0, 5), 'layers': (0, 5, 8)}      # the octaves with an accurate sin / cos (R.kernel_pe)
_scenes = {}


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def scene(views, n_rays, s):
    """24x24 maps, bias_scale 0.1 (inside the rounding-level bars); computed once per shape."""
    key = (views, n_rays, s)
    if key not in _scenes:
        sc = make_scene(seed=61 + views, n_views=views, height=24, width=24, n_rays=n_rays, bias_scale=0.1)
        sc['z'] = np.sort(np.random.default_rng(0).uniform(0.3, 1.3, (1, n_rays, s)).astype(np.float32), -1)
        sc['dev'] = {k: dev(sc[k]) for k in ('rays_o', 'rays_d', 'z') + GEO}
        _scenes[key] = sc
    return _scenes[key]


def launch(monkeypatch, kernel, sc, flat, table=None, view=None):
    """One field_eval_bf16 call with the kernel pinned.  table: None (direct gather), 'f32' (project_texels) or 'bf16'
    (project_texels_bf16), rebuilt from `flat`; view: that view's slices only (a single-view launch).
    -> rgbs (N,4), fused acts (4,N,128) [view mean, u1, u2, u3], the table in feature order or None."""
    d = sc['dev']
    geo = [d[k] if view is None else d[k][:, view:view + 1].contiguous() for k in GEO]
    net = dev(flat)
    packed, packed16 = ops.pack_net(net), ops.pack_net_bf16(net)
    tab = None
    if table == 'f32':
        tab = ops.project_texels(geo[1], packed)
    elif table == 'bf16':
        tab = ops.project_texels_bf16(geo[1], packed16)
    monkeypatch.setenv('MVNERF_BF16_KERNEL', kernel)
    rgbs, fused = ops.field_eval_bf16(d['rays_o'], d['rays_d'], d['z'], *geo, packed, packed16, return_fused_acts=True, texel_table=tab)
    torch.cuda.synchronize()
    return (rgbs.cpu().numpy().reshape(-1, 4), fused.cpu().numpy().reshape(4, -1, 128),
            None if tab is None else R.table_rows(tab.cpu().numpy()))


def check_fusion_half(name, kernel, net, rgbs, fused, rows=slice(None)):
    """Blocks 4, 5, 6 from the kernel's own view mean, u1, u2; the read-out from its own u3 (bf16 in the segment kernel, fp32 in the
    layer-ring kernel) at the bars of the existing layer-ring read-out assertion."""
    for k in range(3):
        R.check(fused[k + 1][rows], *R.block_ref(fused[k][rows], net['blocks'][3 + k]), f'{name} block {4 + k}')
    ref = R.readout_ref(fused[3][rows], net, rounded=kernel == 'segments')
    e_rgb = np.abs(rgbs[rows][:, :3] - ref[:, :3]).max()
    e_sig, top = np.abs(rgbs[rows][:, 3] - ref[:, 3]).max(), max(1.0, float(ref[:, 3].max()))
    print(f'{name} read-out: max |rgb - ref| {e_rgb:.2e}, max |sigma - ref| {e_sig:.2e} (max sigma {top:.3g})')
    assert e_rgb < 2e-6 and e_sig < 1e-5 * top


# ---- a. fusion blocks and read-out, full net ------------------------------------------------------------------------------------
@pytest.mark.parametrize('n_rays,s', SHAPES)
@pytest.mark.parametrize('variant', list(VARIANTS))
def test_fusion_blocks_and_readout(variant, n_rays, s, monkeypatch):
    kernel, table, views = VARIANTS[variant]
    sc = scene(views, n_rays, s)
    rgbs, fused, _ = launch(monkeypatch, kernel, sc, sc['fine'], 'f32' if table else None)
    check_fusion_half(f'{variant} {n_rays}x{s}', kernel, O.unflatten_net(sc['fine']), rgbs, fused)


@pytest.mark.parametrize('variant', list(VARIANTS))
def test_fusion_blocks_and_readout_in_a_second_tile_group(variant, monkeypatch):
    """Both kernels are persistent: launch_field_eval_bf16 / launch_field_eval_bf16x start min(n_groups, CUs) workgroups of 8 waves x 32
    samples, and workgroup w takes tile groups w, w + grid, ...  So with more than 256 * CUs samples the first workgroups run a second
    group (ring positions wrap, the weights stay in flight across the tile boundary): 4 * CUs + 1 rays of 64 samples are 256 * CUs + 64
    samples, one ragged group more than the grid.  Only the first and the last 2048 rows are recomputed in float64."""
    kernel, table, views = VARIANTS[variant]
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    sc = scene(views, 4 * cus + 1, 64)
    rgbs, fused, _ = launch(monkeypatch, kernel, sc, sc['fine'], 'f32' if table else None)
    n = rgbs.shape[0]
    assert n == 256 * cus + 64 and np.isfinite(fused).all() and np.isfinite(rgbs).all()
    check_fusion_half(f'{variant} second group', kernel, O.unflatten_net(sc['fine']), rgbs, fused, np.r_[0:2048, n - 2048:n])


# ---- b. layer 0 and the per-view blocks through knock-out nets, V = 1 -----------------------------------------------------------
BLOCKS_AT = O.N_IN * O.N_HIDDEN + O.N_HIDDEN                     # Keras order: W0 b0 | 6 x (W1 b1 W2 b2) | Wr br
BLOCK_STRIDE = 2 * (O.N_HIDDEN * O.N_HIDDEN + O.N_HIDDEN)


def knock_out(flat, blocks):
    """W2 = 0 and b2 = 0 make a block an exact identity: r = 0 and x + 0 = x."""
    out = flat.copy()
    for i in blocks:
        at = BLOCKS_AT + i * BLOCK_STRIDE + BLOCK_STRIDE // 2
        out[at:at + BLOCK_STRIDE // 2] = 0
    return out


@pytest.mark.parametrize('n_rays,s', SHAPES)
@pytest.mark.parametrize('kernel,table', [('segments', None), ('segments', 'f32'), ('segments', 'bf16'), ('layers', 'f32'), ('layers', 'bf16')])
def test_layer0_and_per_view_blocks_by_knock_out_nets(kernel, table, n_rays, s, monkeypatch):
    """net A (blocks 0, 1, 2 knocked out): view mean = x0; B (1, 2): block0(x0); C (2): block1(f1); D: block2(f2).  x0 is held to
    layer0_ref, every block to block_ref from the PREVIOUS launch's view mean - its own input, since launches repeat bit for bit."""
    sc = scene(1, n_rays, s)
    net = O.unflatten_net(sc['fine'])
    name = f'{kernel} table={table} {n_rays}x{s}'
    prev = None
    for tag, out in (('A', (0, 1, 2)), ('B', (1, 2)), ('C', (2,)), ('D', ())):
        flat = knock_out(sc['fine'], out)
        _, fused, tab = launch(monkeypatch, kernel, sc, flat, table)
        _, again, _ = launch(monkeypatch, kernel, sc, flat, table)
        m = fused[0]
        assert np.array_equal(m, again[0]), tag                             # values, not bit patterns: -0 == +0
        if prev is None:
            ref = R.layer0_ref(net, sc['rays_o'], sc['rays_d'], sc['z'], *(sc[k] for k in GEO), table=tab, pe_direct=PE_DIRECT[kernel])
            R.check(m, *ref, f'{name} layer 0')
        else:
            blk = 'ABCD'.index(tag) - 1
            R.check(m, *R.block_ref(prev, net['blocks'][blk]), f'{name} block {blk}')
        prev = m


# ---- c. the view mean ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('views', [2, 3])
@pytest.mark.parametrize('kernel,table', [('segments', None), ('segments', 'f32'), ('layers', 'f32')])
def test_view_mean_against_single_view_launches(kernel, table, views, monkeypatch):
    """The V-view launch's view mean against the float64 mean of V single-view launches (view v's slices of images, features,
    intrinsics and extrinsics_inv) at the fp32 bar: with net A that is the mean of x0, with the whole net (D) the mean of the per-view
    half - the instantiations may differ in summation order only.  The fusion half of the multi-view launch is checked as in (a)."""
    sc = scene(views, 17, 33)
    net = O.unflatten_net(sc['fine'])
    name = f'{kernel} table={table} V={views}'
    for tag, out in (('A', (0, 1, 2)), ('D', ())):
        flat = knock_out(sc['fine'], out)
        rgbs, fused, _ = launch(monkeypatch, kernel, sc, flat, table)
        singles = [launch(monkeypatch, kernel, sc, flat, table, view=v)[1][0].astype(np.float64) for v in range(views)]
        R.check(fused[0], sum(singles) / views, name=f'{name} net {tag} view mean')
    check_fusion_half(name, kernel, net, rgbs, fused)


# ---- d. project_texels_bf16 ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('maps', ['f32', 'bf16'])
def test_project_texels_bf16_against_float64(maps):
    """2 views of 10 x 14: 280 texels, 8 workgroups of 32 and a ragged one.  Inputs are given and the arithmetic is exact bf16 products
    with fp32 accumulation: nothing is undecided, the bar has no window."""
    sc = make_scene(seed=13, n_views=2, height=10, width=14, n_rays=4)
    feats = dev(sc['features'])
    if maps == 'bf16':
        feats = feats.to(torch.bfloat16).contiguous()
    given = feats.float().cpu().numpy()
    p16 = {k: ops.pack_net_bf16(dev(sc[k])) for k in ('coarse', 'fine')}
    one = {k: ops.project_texels_bf16(feats, p16[k]) for k in p16}
    pair = ops.project_texels_bf16(feats, p16['coarse'], packed16_b=p16['fine'])
    torch.cuda.synchronize()
    for i, k in enumerate(('coarse', 'fine')):
        ref = R.table_ref(given, O.unflatten_net(sc[k])['W0']).reshape(-1, 128)
        R.check(R.table_rows(one[k].cpu().numpy()).reshape(-1, 128), ref, name=f'project_texels_bf16 maps={maps} {k}, one net')
        R.check(R.table_rows(pair[i].cpu().numpy()).reshape(-1, 128), ref, name=f'project_texels_bf16 maps={maps} {k}, two nets')


# ---- e. the packed streams -------------------------------------------------------------------------------------------------------
def _constants(path):
    """The `constexpr int NAME = EXPR` of a kernel source, evaluated in order."""
    ns = {}
    with open(path) as f:
        text = f.read()
    for stmt in re.findall(r'constexpr int ([^;{]+);', text):
        for part in stmt.split(','):
            m = re.fullmatch(r'\s*(\w+)\s*=\s*([\w\s+*/()-]+)', part)
            if m:
                try:
                    ns[m[1]] = int(eval(m[2], {'__builtins__': {}}, ns))
                except (NameError, SyntaxError, TypeError):
                    pass
    return ns


def test_packed_streams_hold_nearest_even_weights():
    """pack_net_bf16 = the segment stream, then the layer-ring stream; a chunk is 1 KiB = 64 lanes x 8 bf16.
    field_eval_bf16.hip: kW16Chunks = 80 (layer 0: 16 PE / rgb + 64 feature chunks) + 12 x 32 (hidden layers) + 16 (read-out: 8 + 8 of
    padding) = 480 chunks, carrying W0 rows 0..59 and 120..378, the twelve 128 x 128 kernels and Wr;
    field_eval_bf16x.hip: kXChunks = 13 positions x 32 chunks = 416, carrying W0 rows 0..59 and 120..122 and the twelve kernels.
    Everything else is zero padding, so the sorted stream must equal the sorted q(w) of those weights plus that many zeros - a
    truncating or half-up converter, a dropped or a duplicated row all change the multiset."""
    csrc = os.path.join(os.path.dirname(ops.__file__), 'csrc')
    seg, ring = _constants(os.path.join(csrc, 'field_eval_bf16.hip')), _constants(os.path.join(csrc, 'field_eval_bf16x.hip'))
    assert (seg['kW16Chunks'], seg['kW16ChunkElems'], ring['kXChunks']) == (480, 512, 416)
    sc = make_scene(seed=2, height=8, width=8, n_rays=4, bias_scale=0.1)
    net = O.unflatten_net(sc['fine'])
    stream = ops.pack_net_bf16(dev(sc['fine'])).view(torch.bfloat16).float().cpu().numpy()
    n_seg, n_ring = seg['kW16Chunks'] * 512, ring['kXChunks'] * 512
    assert stream.size == n_seg + n_ring
    hidden = [blk[i].reshape(-1) for blk in net['blocks'] for i in (0, 2)]
    carried = {'segment': [net['W0'][:60].reshape(-1), net['W0'][120:].reshape(-1), net['Wr'].reshape(-1)] + hidden,
               'layer-ring': [net['W0'][:60].reshape(-1), net['W0'][120:123].reshape(-1)] + hidden}
    for name, got in (('segment', stream[:n_seg]), ('layer-ring', stream[n_seg:])):
        w = np.concatenate(carried[name])
        assert (w != 0).all() and got.size >= w.size
        want = np.concatenate([O.bf16_round(w), np.zeros(got.size - w.size, np.float32)])
        print(f'{name} stream: {got.size} values, {w.size} weights, {got.size - w.size} of padding')
        np.testing.assert_array_equal(np.sort(got), np.sort(want))
