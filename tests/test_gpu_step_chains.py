"""The multi-launch C entry points - mvnerf_render_fwd[_split[_ex]] (csrc/api.hip), mvnerf_loss_and_grads / mvnerf_train_step
(csrc/train_api.hip), mvnerf_grasp_success / _success_and_gradients / _opt_step and the _bf16 step (csrc/grasp_api.hip) - against their
parts run by hand on test-owned buffers (tests/step_chains.py), on poisoned workspaces.

Every case runs the step three times on identical inputs.  Before each run the workspace (exactly `*_workspace_bytes`, with 4 KiB
behind it) and every output buffer (with four guard rows) hold one fill word in every 32-bit word: 0x00000000, 0x7FC00000 (NaN),
0x3F800000 (1.0f).  Asserted (step_chains.check_protocol): every output element is written and finite; guard rows and the workspace
tail keep the word; every ORDER-FIXED output has the same bits under the three fills and the bits of the chain, which runs once on
NaN-filled buffers of its own.  No order-fixed output has a tolerance.

Order-fixed is everything the steps return except, from the code:
  * `loss`: one fp32 atomic per wave in mse_grad_kernel;
  * `d_features`: fp32 atomics in field_dz_kernel (direct path) and texel_scatter_kernel (table path);
  * at V >= 3 only, what depends on the view sum of d_z (the coarse gradient with stop_fine_z = 0) or of d_points / d_dirs (grasp
    gradients): at V <= 2 such a sum has two terms on a zeroed word and commutes exactly.  The V = 3 training case here runs with
    stop_fine_z = 1, no grasp case has V > 2.  (For d_z this became true with this module: its first run found `grad` of the
    (1, 2, 7), stop_fine_z = 0 cases differing between fills, because the two views added their shares onto the compositing term that
    composite_bwd had already stored there - three terms, order-dependent.  mvnerf_loss_and_grads now lets the views add onto zeros
    and adds that term behind them)
Weight gradients are summed in a fixed order (per-workgroup partials, reduce_partials_kernel), so `grad` is order-fixed in every case.

The two order-free outputs have bars that come from references alone:
  * loss: |step - want64| <= max(8 e32, ulp), want64 and e32 built as tests/test_gpu_ray_backward.py::test_mse_grad_and_the_loss_it_adds
    builds them (R.mse_grad_ref, R.mse_loss_f32_accumulated over eight orders of the waves' adds) from the CHAIN's rgb, fine_rgb and
    the labels - images that the assertion above makes bit-equal to the step's;
  * d_features: oracle/field_backward_ref.py on the CHAIN's two stashes and cotangents as tests/test_gpu_field_backward.py::reference
    applies it: ref64 = fine + coarse, e32 = |ref32 fine + ref32 coarse - ref64|, |step - ref64| <= 8 e32 in relative L2 and in the
    worst element over the largest, exactly zero where ref64 is exactly zero; 8 is that file's FACTOR with its derivation.
Both are printed per case (run with -s); DESIGN.md section 8.1 keeps the largest.

Nothing here patches an allocator or fills a buffer it does not own; the largest allocation is the training step's gradient pair."""
import functools

import numpy as np
import pytest
import torch

from oracle import field_backward_ref as FB
from oracle import lmvnerf_torch as L
from oracle import ray_backward_ref as R
from tests import step_chains as C
from tests.test_gpu_grasp_optimizer import BOUNDS
from tests.test_pose_math_cpu import REPS
from thesis_clip_nerf_amd import ops
from thesis_clip_nerf_amd.synthetic import make_scene

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
F32 = np.float32
H, W, S = 16, 20, 64
GEO = ('rays_o', 'rays_d', 'images', 'features', 'intrinsics', 'extrinsics_inv')
FACTOR = 8.0                                               # tests/test_gpu_field_backward.py's, with its derivation


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@pytest.fixture
def split_kernel():
    prev = []

    def choose(name):
        prev.append(ops.set_split_kernel(name))
    yield choose
    if prev:
        ops.set_split_kernel(prev[0])


def chain_run(fn):
    """The chain, once, on NaN-filled buffers of its own; their guards are checked too."""
    fill = C.Fill(C.NAN_WORD, DEV)
    out = fn(fill)
    torch.cuda.synchronize()
    fill.assert_guards()
    return out


@functools.lru_cache(maxsize=None)
def scene(b, v, r):
    sc = make_scene(seed=700 + 100 * b + 10 * v + r, batch=b, n_views=v, height=H, width=W, n_rays=r, bias_scale=0.05)
    d = {k: dev(sc[k]) for k in GEO + ('u_coarse', 'u_fine')}
    nets = (dev(sc['coarse']), dev(sc['fine']))
    d.update(B=b, V=v, R=r, S=S, H=H, W=W, near=float(sc['near']), far=float(sc['far']), q7=ops.Q7_ZERO, sc=sc, nets=nets,
             packed=tuple(ops.pack_net(n) for n in nets), split=tuple(ops.pack_net_split(n) for n in nets),
             bwd=tuple(ops.pack_bwd_streams(n) for n in nets),
             labels=dev(np.random.default_rng(b + v + r).random((b, r, 3)).astype(F32)))
    torch.cuda.synchronize()
    return d


# ---- render ----------------------------------------------------------------------------------------------------------------------------------
RENDER_KINDS = {'fp32': ('fp32', None), 'split_f16': ('split', 'split_f16'), 'split_bf16': ('split', 'split_bf16'), 'ex': ('ex', None)}
RENDER_CASES = ([((2, 1, 5), kind, tables) for kind in RENDER_KINDS for tables in (None, 'built', 'ready')] +
                [(shape, 'split_f16', tables) for shape in ((1, 2, 7), (1, 3, 3)) for tables in (None, 'built')])


@pytest.mark.parametrize('shape,kind,tables', RENDER_CASES)
def test_render_step_equals_its_parts_under_every_fill(shape, kind, tables, split_kernel):
    """(2, 1, 5): 10 rays - a ragged 4-ray workgroup of the scans, the scene boundary inside a tile group; (1, 2, 7), (1, 3, 3): the
    view mean, 1 / V not a power of two.  `ex`: the f16x3 kernel chosen per call with a two-float range status, compared too."""
    d = scene(*shape)
    entry, process_wide = RENDER_KINDS[kind]
    if process_wide:
        split_kernel(process_wide)
    which = ops.SPLIT_KERNELS['split_f16'] if entry == 'ex' else -1
    if tables == 'ready':
        tables = ops.project_texels2(d['features'], *d['packed'])
    status = lambda fill: fill((2,), name='range status', init=torch.zeros(2, device=DEV)) if entry == 'ex' else None
    runs = C.run_fills(lambda fill: C.render_step(fill, d, entry, tables, which, status(fill)), DEV, torch.cuda.synchronize)
    want = chain_run(lambda fill: C.render_chain(fill, d, entry, tables, which, status(fill)))
    C.check_protocol(runs, want)
    print(f'render {shape} {kind} tables={tables if isinstance(tables, str) or tables is None else "ready"}: three fills and the chain agree '
          f'bit for bit on {sorted(want)}')


# ---- training --------------------------------------------------------------------------------------------------------------------------------
def check_loss(tag, runs, want, d):
    rgb, fine, label = (t.cpu().numpy() for t in (want['rgb'], want['fine_rgb'], d['labels']))
    want64 = float(R.mse_grad_ref(rgb, label, np.float64)[1]) + float(R.mse_grad_ref(fine, label, np.float64)[1])
    waves = -(-rgb.size // 64)
    orders = [None, range(waves - 1, -1, -1)] + [np.random.default_rng(k).permutation(waves) for k in range(6)]
    e32 = max(abs(float(R.mse_loss_f32_accumulated(fine, label, R.mse_loss_f32_accumulated(rgb, label, 0.0, order), order)) - want64)
              for order in orders)
    ulp = float(np.spacing(F32(want64)))
    worst = 0.0
    for word, out in runs:
        e64 = abs(float(out['loss'].cpu()[0]) - want64)
        worst = max(worst, e64 / max(e32, ulp / R.FACTOR))
        print(f'RATIO {tag} loss fill {word:#010x}: e64 {e64:.3e}  e32 {e32:.3e}  ulp {ulp:.3e}  e64/max(e32, ulp/8) {e64 / max(e32, ulp / R.FACTOR):.2f}')
        assert e64 <= max(R.FACTOR * e32, ulp), (tag, word, e64, e32, ulp)
    return worst


def d_features_refs(d, k, z, stash, rgbs, d_rgbs, s):
    """float64 and float32 d_features of one field pass (net k) from its own stash, as tests/test_gpu_field_backward.py::reference."""
    b, v, r = d['B'], d['V'], d['R']
    sc = d['sc']
    net = sc[('coarse', 'fine')[k]]
    geo = (sc['rays_o'], sc['rays_d'], z.cpu().numpy()) + tuple(sc[key] for key in GEO[2:])
    rows = FB.decode_stash(stash.view(torch.float32).cpu().numpy(), b, v, r, s)
    rgbs, d_rgbs = rgbs.cpu().numpy(), d_rgbs.cpu().numpy()
    c0_64 = lambda x_in: FB.field_backward_ref(net, rows, rgbs, d_rgbs, x_in, v, np.float64)[2]
    df64 = FB.input_grads(c0_64, *geo, dtype=torch.float64)[1]
    c0_32 = FB.field_backward_ref(net, rows, rgbs, d_rgbs, FB.layer0_input_f32(*geo), v, np.float32)[2]
    df32 = FB.input_grads(c0_32, *geo, dtype=torch.float32)[1]
    return df64.astype(np.float64), df32.astype(np.float64)

def check_d_features(tag, runs, aux, d):
    f64, f32 = d_features_refs(d, 1, aux['z_all'], aux['stash_f'], aux['rgbs_f'], aux['d_rgbs_f'], 2 * S)
    c64, c32 = d_features_refs(d, 0, aux['z'], aux['stash_c'], aux['rgbs_c'], aux['d_rgbs_c'], S)
    ref64 = f64 + c64
    err32 = np.abs(f32 + c32 - ref64)
    n, m = np.linalg.norm(ref64), np.abs(ref64).max()
    assert n > 0
    worst = 0.0
    for word, out in runs:
        g = out['d_features'].cpu().numpy().astype(np.float64)
        assert not np.count_nonzero(g[ref64 == 0]), (tag, word, 'not exactly zero where the reference is')
        for kind, e64, e32 in (('L2', np.linalg.norm(g - ref64) / n, np.linalg.norm(err32) / n), ('max', np.abs(g - ref64).max() / m, err32.max() / m)):
            ratio = e64 / e32 if e32 > 0 else np.inf
            worst = max(worst, ratio)
            print(f'RATIO {tag} d_features fill {word:#010x} {kind}: e64 {e64:.3e}  e32 {e32:.3e}  e64/e32 {ratio:.2f}')
            assert e64 <= FACTOR * e32, (tag, word, kind, e64, e32)
    return worst


def run_train_case(shape, use_split, stop, tables, want_df):
    d = scene(*shape)
    tag = f'train {shape} split={int(use_split)} stop={int(stop)} tables={int(tables)} d_features={int(want_df)}'

    def step(fill):
        c, out, _ = C.train_call(fill, d, use_split, stop, tables, want_df)
        ops.loss_and_grads(c, d['rays_o'])
        return out
    runs = C.run_fills(step, DEV, torch.cuda.synchronize)
    want, aux = chain_run(lambda fill: C.train_chain(fill, d, use_split, stop, tables, want_df))
    C.check_protocol(runs, want, order_free=('loss', 'd_features'))
    print(f'{tag}: three fills and the chain agree bit for bit on {sorted(set(want) - {"loss", "d_features"})}')
    check_loss(tag, runs, want, d)
    if want_df:
        check_d_features(tag, runs, aux, d)


@pytest.mark.parametrize('want_df', [False, True])
@pytest.mark.parametrize('tables', [False, True])
@pytest.mark.parametrize('stop', [False, True])
@pytest.mark.parametrize('shape', [(2, 1, 5), (1, 2, 7)])
def test_loss_and_grads_equals_its_parts_under_every_fill(shape, stop, tables, want_df, split_kernel):
    """All eight wirings of carve_train; bwd_scratch, field_ws and texel_grad are shared by the fine and the coarse call in the step
    and separate in the chain."""
    split_kernel('split_f16')
    run_train_case(shape, True, stop, tables, want_df)


def test_loss_and_grads_on_the_fp32_mfma_forward_equals_its_parts(split_kernel):
    """split_coarse = split_fine = NULL: mvnerf_field_eval_stash instead of mvnerf_field_eval_stash_split."""
    run_train_case((2, 1, 5), False, False, True, True)


def test_loss_and_grads_with_three_views_equals_its_parts(split_kernel):
    """V = 3 with the fine depths held constant: no view sum of d_z enters the coarse gradient, so all but loss and d_features stays
    order-fixed."""
    split_kernel('split_f16')
    run_train_case((1, 3, 3), True, True, True, True)


def test_train_step_equals_loss_and_grads_then_apply_gradients(split_kernel):
    """mvnerf_train_step from zero moments with every 7th entry of update_mask off: the nets, m, v and the three re-packed weight images
    of each net are bit-equal to the chain followed by adam_clip twice and the re-packs."""
    split_kernel('split_f16')
    base = scene(2, 1, 5)
    mask = torch.ones(2 * C.NP, dtype=torch.uint8, device=DEV)
    mask[::7] = 0
    adam = dict(lr_t=float(F32(1e-3 * np.sqrt(1 - 0.999) / (1 - 0.9))), beta1=0.9, beta2=0.999, eps=1e-7, clip=1.0, update_mask=mask)
    state_names = [f'{kind}{k}' for kind in ('nets', 'packed', 'split', 'bwd') for k in range(2)] + ['m', 'v']

    def state(fill):
        """The in/out state of one run: copies of the variables and their weight images, zero moments; guard rows behind each."""
        d = dict(base)
        for kind in ('nets', 'packed', 'bwd'):
            d[kind] = tuple(fill(t.shape, name=kind, init=t) for t in base[kind])
        d['split'] = tuple(fill(t.numel(), name='split', init=t) for t in base['split'])
        zeros = torch.zeros(2 * C.NP, device=DEV)
        return d, fill((2 * C.NP,), name='m', init=zeros), fill((2 * C.NP,), name='v', init=zeros)

    def outputs(out, d, m, v):
        out.update({f'{kind}{k}': d[kind][k] for kind in ('nets', 'packed', 'split', 'bwd') for k in range(2)}, m=m, v=v)
        return out

    def step(fill):
        d, m, v = state(fill)
        c, out, _ = C.train_call(fill, d, True, False, True, False)
        ops.train_step_c(c, ops.adam_state(m, v, adam['lr_t'], adam['beta1'], adam['beta2'], adam['eps'], adam['clip'], mask, repack=True), d['rays_o'])
        return outputs(out, d, m, v)

    def chain(fill):
        d, m, v = state(fill)
        out, _ = C.train_chain(fill, d, True, False, True, False)
        C.apply_chain(d, out['grad'], m, v, adam)
        return outputs(out, d, m, v)
    runs = C.run_fills(step, DEV, torch.cuda.synchronize)
    want = chain_run(chain)
    C.check_protocol(runs, want, order_free=('loss',))
    check_loss('train_step (2, 1, 5)', runs, want, base)
    nets = torch.cat(base['nets'])
    got = torch.cat([runs[0][1]['nets0'], runs[0][1]['nets1']])
    assert torch.equal(got[::7], nets[::7]) and not torch.equal(got, nets)          # masked entries stay, the others moved
    assert not torch.equal(runs[0][1]['packed1'], base['packed'][1]) and not torch.equal(runs[0][1]['split0'], base['split'][0])
    print(f'train_step (2, 1, 5): three fills and the chain agree bit for bit on {sorted(set(want) - {"loss"})}; state {state_names}')


# ---- grasp -----------------------------------------------------------------------------------------------------------------------------------
PHASES = ((1, 0), (0, 1), (1, 1))
GRASP_SHAPES = [(1, 1, 1, 42),          # M = 1
                (3, 1, 5, 42),          # 210 rows a scene: a ragged 32-row tile, three scenes unpadded
                (1, 2, 5, 42),          # ld = 224 > 210: pad rows
                (2, 2, 3, 18)]          # ld = 64 > 54: pad rows, one tail call per scene


@functools.lru_cache(maxsize=None)
def grasp_scene(b, v, p, n5, representation):
    sc = make_scene(seed=900 + 100 * b + 10 * v + p, batch=b, n_views=v, height=H, width=W, n_rays=4, bias_scale=0.05)
    rep, rd = REPS[representation]
    rng = np.random.default_rng(n5 + p)
    f = lambda scale, *shape: dev((scale * rng.standard_normal(shape)).astype(F32))
    k = 64 * n5
    net = dev(sc['fine'])
    w4, wc = f(0.1, 4, 64, 128), f(0.08, 64, 256)
    tail = ops.grasp_tail_pack((f(k ** -0.5, 128, k), f(0.05, 128), f(0.1, 64, 128), f(0.05, 64), f(k ** -0.5, 64, k)),
                               (f(0.15, 64, 64), f(0.05, 64), f(0.15, 64, 64), f(0.05, 64)), (f(0.2, 1, 64), f(0.05, 1)))
    t = rng.uniform(np.array(BOUNDS)[:, 0], np.array(BOUNDS)[:, 1], (p, 3)).astype(F32)
    rot = rng.standard_normal((p, rd)).astype(F32)
    if rd == 4:
        rot /= np.linalg.norm(rot, axis=-1, keepdims=True)
    d = dict(B=b, V=v, P=p, n5=n5, H=H, W=W, rep=rep, images=dev(sc['images']), features=dev(sc['features']), intrinsics=dev(sc['intrinsics']),
             extrinsics_inv=dev(sc['extrinsics_inv']), packed=ops.pack_net(net), split=ops.pack_net_split(net), bwd=ops.pack_bwd_streams(net),
             packed16=ops.pack_net_bf16(net), bwd16=ops.pack_bwd_streams_bf16(net), head=ops.grasp_head_pack(w4, wc), b4=f(0.05, 4, 64),
             bc=f(0.05, 64), tail=tail, offsets=dev(L.transforms_to_check(n5 // 6).astype(F32)), t=dev(t), rot=dev(rot),
             cfg=ops.pose_adam_config(lr0=(0.05, 0.05), decay=(0.9, 0.09), clip_translation=True, bounds=BOUNDS))
    assert d['offsets'].shape == (n5, 4, 4)
    torch.cuda.synchronize()
    return d


def grasp_state(fill, d, with_adam):
    p, rd = d['P'], d['rot'].shape[-1]
    state = dict(t=fill((p, 3), name='t', init=d['t']), rot=fill((p, rd), name='rot', init=d['rot']))
    if not with_adam:
        return state, None
    z = lambda *shape: torch.zeros(shape, device=DEV)
    adam = dict(cfg=d['cfg'], flags=torch.zeros(2, dtype=torch.int32, device=DEV),
                counters=fill((2, p), dtype=torch.int32, name='counters', init=torch.zeros((2, p), dtype=torch.int32, device=DEV)),
                m_t=fill((p, 3), name='m_t', init=z(p, 3)), v_t=fill((p, 3), name='v_t', init=z(p, 3)),
                m_r=fill((p, rd), name='m_r', init=z(p, rd)), v_r=fill((p, rd), name='v_r', init=z(p, rd)))
    return state, adam


def run_grasp_case(shape, representation, entry, bf16):
    d = grasp_scene(*shape, representation)
    opt = entry == 'opt_step'

    def drive(one):
        """one(fill, state, adam) -> outputs of one call; an optimiser case takes one step per phase, each on freshly filled buffers."""
        def run(fill):
            state, adam = grasp_state(fill, d, opt)
            if not opt:
                return one(fill, state, None)
            out = {}
            for i, phase in enumerate(PHASES):
                adam['flags'].copy_(torch.tensor(phase, dtype=torch.int32))
                out.update({f'{k}@{i}': v for k, v in one(fill, state, adam).items()})
            out.update(t=state['t'], rot=state['rot'], **{k: adam[k] for k in ('counters', 'm_t', 'v_t', 'm_r', 'v_r')})
            return out
        return run
    runs = C.run_fills(drive(lambda fill, state, adam: C.grasp_step(fill, d, state, entry, bf16, adam)), DEV, torch.cuda.synchronize)
    want = chain_run(drive(lambda fill, state, adam: C.grasp_chain(fill, d, state, entry != 'success', bf16, adam)))
    C.check_protocol(runs, want)
    if opt:
        assert not torch.equal(want['t'], d['t']) and not torch.equal(want['rot'], d['rot']) and bool((want['counters'] == 2).all())
    print(f'grasp{"_bf16" if bf16 else ""} {shape} {representation} {entry}: three fills and the chain agree bit for bit on {sorted(want)}')


@pytest.mark.parametrize('entry', ['success', 'success_and_gradients', 'opt_step'])
@pytest.mark.parametrize('representation', ['quaternion', '6d'])
@pytest.mark.parametrize('shape', GRASP_SHAPES)
def test_grasp_step_equals_its_parts_under_every_fill(shape, representation, entry, split_kernel):
    split_kernel('split_f16')
    run_grasp_case(shape, representation, entry, False)


@pytest.mark.parametrize('representation', ['quaternion', '6d'])
@pytest.mark.parametrize('shape', [(3, 1, 5, 42), (1, 2, 5, 42)])
def test_grasp_bf16_step_equals_its_parts_under_every_fill(shape, representation):
    """Relu bits in the stash's place, the bf16 workspace size."""
    run_grasp_case(shape, representation, 'opt_step', True)
