"""The bf16 trunk VJP on the GPU (csrc/query_bf16.hip, the relu bits of csrc/field_eval_bf16.hip) against the float64
references of tests/trunk_vjp_bf16_ref.py.  Small shapes: one tile (N = 32), a partial tile (N = 40, V = 1), two scenes of two tiles
(N = 64, B = 2), V in {1, 2, 3}, 16 x 20 sources.

  1. relu bits that can be observed directly: mean, x4, x5 against acts > 0 of the same launch; x0, x1, x2 through knock-out nets (V = 1);
  2. bits of the hidden pre-activations against float64 W1_bf16 bf16(relu(x_observed)) + b1 outside a 16 * 2^-24 window;
  3. single-block launches against block_bwd_ref at R.check's bar;
  4. all blocks knocked out, V = 2, 3: every view's g0 is the fp32 sum of the four cotangents over V, exactly;
  5. the whole chain: relL2(g0 - R) <= 2 relL2(R_q - R);
  6. mvnerf_query_vjp_bf16 = mvnerf_query_vjp's layer-0 pass on the same g0, bit for bit (V = 1);
  7. zero cotangent, scaling by 2, guard rows, two runs;
  8. TrunkField / _TrunkVJP on a bf16 TrunkState through autograd; LanguageNeRF.infer packs its bf16 images once."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import field_bf16_ref as R
from oracle import mvnerf_oracle as O
from tests import trunk_vjp_bf16_ref as B
from tests.test_gpu_bf16_grade import knock_out
from tests.test_gpu_query import DEV, dev, make_query
from thesis_clip_nerf_amd import _lib, ops

pytestmark = pytest.mark.gpu
GEO = ('images', 'features', 'intrinsics', 'extrinsics_inv')
SHAPES = [(1, 32, 1), (1, 40, 1), (1, 64, 2), (2, 64, 2), (3, 32, 1)]          # (views, points per scene, scenes)
_cases, _fwd = {}, {}


def case(views, n, batch):
    key = (views, n, batch)
    if key not in _cases:
        sc, points, dirs = make_query(40 + views, views, n, batch)
        g_acts = np.random.default_rng(views + n).standard_normal((4, batch, n, 128)).astype(np.float32)
        _cases[key] = dict(sc=sc, net=O.unflatten_net(sc['fine']), points=dev(points), dirs=dev(dirs), geo=[dev(sc[k]) for k in GEO],
                           g_acts=g_acts, v=views, n=n, b=batch)
    return _cases[key]


def forward(c, flat=None, tag='full'):
    """query_stash_bf16 with the case's net or a knock-out of it -> acts (4, B N, 128) numpy, bits (6 V + 6, B N, 128) bool numpy,
    the device bit buffer and the device weight images.  Once per (case, net)."""
    key = (c['v'], c['n'], c['b'], tag)
    if key not in _fwd:
        net = dev(c['sc']['fine'] if flat is None else flat)
        packed, packed16, bwd16 = ops.pack_net(net), ops.pack_net_bf16(net), ops.pack_bwd_streams_bf16(net)
        acts, bits = ops.query_stash_bf16(c['points'], c['dirs'], *c['geo'], packed, packed16)
        on = ops.unpack_relu_bits(bits, c['b'], c['v'], c['n'])
        torch.cuda.synchronize()
        rows = c['b'] * c['n']
        _fwd[key] = dict(acts=acts.cpu().numpy().reshape(4, rows, 128), on=on.permute(1, 0, 2, 3).reshape(-1, rows, 128).cpu().numpy(),
                         bits=bits, bwd16=bwd16, net=net)
    return _fwd[key]


def g0_rows(g0, c):
    """g0 (view tiles, 128, 32) -> (V, B N, 128) rows, and the padding rows of a last partial tile (V = 1)."""
    v, n, b = c['v'], c['n'], c['b']
    t = g0.cpu().numpy()
    if v == 1:
        rows = t.transpose(0, 2, 1).reshape(-1, 128)
        return rows[None, :b * n], rows[b * n:]
    rows = t.reshape(b, v, n // 32, 128, 32).transpose(1, 0, 2, 4, 3).reshape(v, b * n, 128)
    return rows, rows[:, :0]


def trunk_vjp(c, f, g_acts):
    g0 = ops.trunk_vjp_bf16(f['bwd16'], f['bits'], dev(g_acts), c['v'])
    torch.cuda.synchronize()
    return g0


# ---- 1. bits that can be observed ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('views,n,batch', SHAPES)
def test_bits_of_mean_x4_x5_equal_the_sign_of_the_activations_of_the_same_launch(views, n, batch):
    c = case(views, n, batch)
    f = forward(c)
    fused = f['on'][6 * views:]
    for slot, k in ((0, 0), (2, 1), (4, 2)):
        np.testing.assert_array_equal(fused[slot], f['acts'][k] > 0, err_msg=f'fused slot {slot}')
    assert 0.2 < fused.mean() < 0.8


@pytest.mark.parametrize('n,batch', [(32, 1), (40, 1), (64, 2)])
def test_bits_of_x0_x1_x2_through_knock_out_nets(n, batch):
    """A block with W2 = b2 = 0 is an exact identity, so with blocks k.. 2 knocked out the view mean IS x_k (V = 1)."""
    c = case(1, n, batch)
    for tag, out, slots in (('A', (0, 1, 2), (0, 2, 4)), ('B', (1, 2), (2, 4)), ('C', (2,), (4,))):
        f = forward(c, knock_out(c['sc']['fine'], out), tag)
        for slot in slots:
            np.testing.assert_array_equal(f['on'][slot], f['acts'][0] > 0, err_msg=f'net {tag} per-view slot {slot}')


# ---- 2. bits of the hidden pre-activations ------------------------------------------------------------------------------------------
def hidden_bits_check(name, on_h, x_obs, blk):
    w1q, a = R.q(blk[0]), R.q(np.maximum(x_obs, 0))
    b1 = np.asarray(blk[1], np.float64)
    h_ref = a @ w1q + b1
    decided = np.abs(h_ref) > 16 * R.EPS * (np.abs(a) @ np.abs(w1q) + np.abs(b1))
    wrong = int((on_h != (h_ref > 0))[decided].sum())
    print(f'{name}: {on_h.size} bits, undecided {int((~decided).sum())}, wrong among the decided {wrong}')
    assert wrong == 0, name
    return int((~decided).sum()), on_h.size


@pytest.mark.parametrize('views,n,batch', SHAPES)
def test_hidden_bits_of_the_fusion_blocks(views, n, batch):
    c = case(views, n, batch)
    f = forward(c)
    fused = f['on'][6 * views:]
    und = [hidden_bits_check(f'h{4 + k}', fused[2 * k + 1], f['acts'][k], c['net']['blocks'][3 + k]) for k in range(3)]
    assert sum(u for u, _ in und) <= max(1, int(1e-4 * sum(s for _, s in und)))


@pytest.mark.parametrize('n,batch', [(32, 1), (40, 1), (64, 2)])
def test_hidden_bits_of_the_per_view_blocks_through_knock_out_nets(n, batch):
    c = case(1, n, batch)
    und = []
    for k, (tag, out) in enumerate((('A', (0, 1, 2)), ('B', (1, 2)), ('C', (2,)))):
        f = forward(c, knock_out(c['sc']['fine'], out), tag)          # the mean is x_k, and block k's first Dense is untouched
        und.append(hidden_bits_check(f'h{k + 1}', f['on'][2 * k + 1], f['acts'][0], c['net']['blocks'][k]))
    assert sum(u for u, _ in und) <= max(1, int(1e-4 * sum(s for _, s in und)))


# ---- 3. single-block launches -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('block', range(6))
def test_single_block_against_the_block_reference(block):
    """Every block but one knocked out: the others pass g on exactly (0 products, g + 0), so with only u3's cotangent given g0 is that
    block's backward of it, with the bits of that launch.  Every launch is held on its own to R.check's element-wise assertions
    (|got - ref| <= bar + flip everywhere, <= bar on rows without an undecided element, bar = 16 * 2^-24 * max |ref| of that launch).
    R.check's two caps are shares of rows, so they are taken over the three launches of a block together (200 rows, each launch
    divided by its own max |ref| so that its rows keep their bar): the share of undecided rows is a property of the reference alone -
    a cotangent has both signs, so |g_hid| is small against sum |g| |w| more often than a forward's hid, and 9 - 17 % of a block's
    200 rows hold an element inside the c = 2 window (6 - 28 % of a single launch's) - which 32 rows cannot resolve against the
    20 % cap."""
    got, refs, unds, flips = [], [], [], []
    for n, batch in ((32, 1), (40, 1), (64, 2)):
        c = case(1, n, batch)
        flat = knock_out(c['sc']['fine'], [k for k in range(6) if k != block])
        f = forward(c, flat, f'only{block}')
        g = np.zeros_like(c['g_acts'])
        g[3] = c['g_acts'][3]
        rows, pad = g0_rows(trunk_vjp(c, f, g), c)
        assert not pad.any()                                  # the last tile's padding carries a zero cotangent
        on = f['on']
        bits_x, bits_h = (on[2 * block], on[2 * block + 1]) if block < 3 else (on[6 + 2 * (block - 3)], on[6 + 2 * (block - 3) + 1])
        ref, und, flip = B.block_bwd_ref(g[3].reshape(-1, 128), O.unflatten_net(flat)['blocks'][block], bits_h, bits_x)
        scale = np.abs(ref).max()
        err, bar, decided = np.abs(rows[0] - ref), R.BAR_ULPS * R.EPS * scale, ~und.any(1)
        print(f'block {block} N={n} B={batch}: undecided rows {int((~decided).sum())} of {len(ref)}, worst decided row '
              f'{err[decided].max() / (R.EPS * scale):.2f} x 2^-24 scale, worst row {err.max() / (R.EPS * scale):.1f}')
        assert np.isfinite(rows).all() and (err <= bar + flip).all() and (err[decided] <= bar).all(), (n, batch)
        got.append(rows[0] / scale), refs.append(ref / scale), unds.append(und), flips.append(flip / scale)
    R.check(np.concatenate(got), np.concatenate(refs), np.concatenate(unds), np.concatenate(flips), f'block {block} backward, 200 rows')


# ---- 4. views -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('views,n,batch', [(2, 64, 2), (3, 32, 1), (2, 32, 1)])
def test_every_view_gets_the_summed_cotangent_over_v_exactly(views, n, batch):
    """All blocks knocked out: g0 of each view = (((g_u3 + g_u2) + g_u1) + g_mean) / V in fp32 - the cotangents enter in the order of
    mvnerf_query_vjp, the division mirrors the forward's mean."""
    c = case(views, n, batch)
    f = forward(c, knock_out(c['sc']['fine'], range(6)), 'none')
    g = c['g_acts'].reshape(4, -1, 128)
    want = (((g[3] + g[2]) + g[1]) + g[0]) / np.float32(views)
    assert want.dtype == np.float32
    rows, _ = g0_rows(trunk_vjp(c, f, c['g_acts']), c)
    for v in range(views):
        np.testing.assert_array_equal(rows[v], want, err_msg=f'view {v}')


# ---- 5. the whole chain -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('views,n,batch', SHAPES)
def test_whole_chain_within_twice_the_operand_rounding_error(views, n, batch):
    c = case(views, n, batch)
    f = forward(c)
    rows, _ = g0_rows(trunk_vjp(c, f, c['g_acts']), c)
    g = c['g_acts'].reshape(4, -1, 128)
    ref = B.chain(c['net'], g, f['on'], views)
    e_q = B.rel_l2(B.chain(c['net'], g, f['on'], views, quantize=True), ref)
    e_k = B.rel_l2(rows, ref)
    print(f'V={views} N={n} B={batch}: e_k = {e_k:.3e}, e_q = {e_q:.3e}, e_k / e_q = {e_k / e_q:.3f}')
    assert np.isfinite(rows).all() and e_k <= 2 * e_q


# ---- 6. composition -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n,batch', [(32, 1), (40, 1), (64, 2)])
def test_query_vjp_bf16_is_the_fp32_layer0_pass_on_the_same_g0(n, batch):
    c = case(1, n, batch)
    f = forward(c)
    g_acts = dev(c['g_acts'])
    bwd = ops.pack_bwd_streams(f['net'])
    d_points, d_dirs = ops.query_vjp_bf16(c['points'], c['dirs'], *c['geo'], bwd, f['bwd16'], f['bits'], g_acts)
    rows, _ = g0_rows(ops.trunk_vjp_bf16(f['bwd16'], f['bits'], g_acts, 1), c)
    # the existing entry point with the hidden slabs zeroed (every block passes its cotangent on) and g0 given as u3's cotangent
    bwd0 = bwd.clone()
    bwd0[:12 * 16384] = 0
    cot = np.zeros_like(c['g_acts'])
    cot[3] = rows[0].reshape(batch, n, 128)
    stash = ops.query_stash(c['points'], c['dirs'], *c['geo'], ops.pack_net(f['net']))
    want_p, want_d = ops.query_vjp(c['points'], c['dirs'], *c['geo'], bwd0, stash, dev(cot))
    torch.cuda.synchronize()
    assert torch.isfinite(d_points).all() and d_points.abs().max() > 0
    assert torch.equal(d_points, want_p) and torch.equal(d_dirs, want_d)


# ---- 7. properties ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('views,n,batch', [(1, 40, 1), (3, 32, 1), (2, 64, 2)])
def test_zero_cotangent_scaling_and_repeatability(views, n, batch):
    c = case(views, n, batch)
    f = forward(c)
    g0 = trunk_vjp(c, f, c['g_acts'])
    assert not trunk_vjp(c, f, np.zeros_like(c['g_acts'])).any()
    assert torch.equal(trunk_vjp(c, f, 2 * c['g_acts']), 2 * g0)
    assert torch.equal(trunk_vjp(c, f, c['g_acts']), g0)
    if views == 1:                                                # (for V > 1 the layer-0 pass sums the views with atomics)
        bwd = ops.pack_bwd_streams(f['net'])
        one = ops.query_vjp_bf16(c['points'], c['dirs'], *c['geo'], bwd, f['bwd16'], f['bits'], dev(c['g_acts']))
        two = ops.query_vjp_bf16(c['points'], c['dirs'], *c['geo'], bwd, f['bwd16'], f['bits'], dev(2 * c['g_acts']))
        assert torch.equal(two[0], 2 * one[0]) and torch.equal(two[1], 2 * one[1])


@pytest.mark.parametrize('views,n,batch', [(1, 40, 1), (2, 64, 2)])
def test_outputs_stay_between_their_guard_rows(views, n, batch):
    """Every output pre-filled with NaN between guard rows: the kernels write all of it and nothing else."""
    c = case(views, n, batch)
    f = forward(c)
    lib = _lib.lib()
    ptr = lambda t, off=0: ctypes.c_void_p(t.data_ptr() + off)
    guard = 4096                                                  # bytes in front of and behind each output

    def guarded(nbytes):
        buf = torch.full((nbytes + 2 * guard,), 0xA5, dtype=torch.uint8, device=DEV)
        buf[guard:guard + nbytes].view(torch.float32).fill_(float('nan'))
        return buf

    def inside(buf, nbytes):
        assert (buf[:guard] == 0xA5).all() and (buf[guard + nbytes:] == 0xA5).all()
        return buf[guard:guard + nbytes].view(torch.float32)

    g_acts = dev(c['g_acts'])
    n_g0 = lib.mvnerf_query_vjp_bf16_scratch_bytes(batch, views, n)
    g0 = guarded(n_g0)
    assert lib.mvnerf_trunk_vjp_bf16(ptr(f['bwd16']), ptr(f['bits']), ptr(g_acts), batch, views, n, ptr(g0, guard), None) == 0
    torch.cuda.synchronize()
    assert torch.isfinite(inside(g0, n_g0)).all()
    assert torch.equal(inside(g0, n_g0), trunk_vjp(c, f, c['g_acts']).reshape(-1))
    # the forward's two outputs
    n_bits, n_acts = lib.mvnerf_relu_bits_bytes(batch, views, n), 4 * batch * n * 128 * 4
    bits, acts = guarded(n_bits), guarded(n_acts)
    ws = torch.empty(lib.mvnerf_query_workspace_bytes(batch, views, n), dtype=torch.uint8, device=DEV)
    packed, packed16 = ops.pack_net(f['net']), ops.pack_net_bf16(f['net'])
    rc = lib.mvnerf_query_stash_bf16(ptr(c['points']), ptr(c['dirs']), *(ptr(t) for t in c['geo']), ptr(packed), ptr(packed16), batch, views, n,
                                     c['geo'][0].shape[2], c['geo'][0].shape[3], ptr(acts, guard), ptr(bits, guard), ptr(ws), None)
    assert rc == 0, lib.mvnerf_last_error()
    torch.cuda.synchronize()
    assert torch.isfinite(inside(acts, n_acts)).all()
    assert torch.equal(inside(bits, n_bits).view(torch.uint8), f['bits'][:n_bits])
    # d_points, d_dirs
    n_d = batch * n * 3 * 4
    d_points, d_dirs = guarded(n_d), guarded(n_d)
    scratch = torch.empty(n_g0, dtype=torch.uint8, device=DEV)
    bwd = ops.pack_bwd_streams(f['net'])
    rc = lib.mvnerf_query_vjp_bf16(ptr(c['points']), ptr(c['dirs']), *(ptr(t) for t in c['geo']), ptr(bwd), ptr(f['bwd16']), ptr(f['bits']),
                                   ptr(g_acts), batch, views, n, c['geo'][0].shape[2], c['geo'][0].shape[3], ptr(scratch), ptr(d_points, guard),
                                   ptr(d_dirs, guard), None)
    assert rc == 0, lib.mvnerf_last_error()
    torch.cuda.synchronize()
    assert torch.isfinite(inside(d_points, n_d)).all() and torch.isfinite(inside(d_dirs, n_d)).all()


# ---- 8. the autograd dispatch --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('views,n,batch', [(1, 40, 1), (2, 40, 2), (3, 32, 1)])
def test_trunk_field_with_a_bf16_state_runs_the_bf16_entry_points(views, n, batch):
    """TrunkField.apply / .backward() on a TrunkState(compute_dtype='bf16') against ops.query_stash_bf16 / ops.query_vjp_bf16 on the same
    points - padded by hand to whole tiles where V > 1 and N % 32 != 0, as TrunkField pads them (last point repeated, zero cotangent)."""
    from thesis_clip_nerf_amd.lmvnerf import TrunkField, TrunkState
    sc, points, dirs = make_query(60 + views, views, n, batch)
    net = dev(sc['fine'])
    state = TrunkState(*(dev(sc[k]) for k in GEO), net, compute_dtype='bf16')
    assert state.compute_dtype == 'bf16' and state.packed16.dtype == torch.uint8 and state.bwd16.dtype == torch.uint8
    p, d = dev(points).requires_grad_(True), dev(dirs).requires_grad_(True)
    g = dev(np.random.default_rng(views).standard_normal((4, batch, n, 128)).astype(np.float32))
    acts = TrunkField.apply(p, d, state)
    (acts * g).sum().backward()
    pad = (-n) % 32 if views > 1 else 0
    rep = lambda t: torch.cat([t, t[:, -1:].expand(-1, pad, -1)], 1).contiguous() if pad else t
    pp, dd = rep(p.detach()), rep(d.detach())
    gg = torch.cat([g, g.new_zeros(4, batch, pad, 128)], 2).contiguous() if pad else g
    want_acts, bits = ops.query_stash_bf16(pp, dd, *state.geo, state.packed, state.packed16)
    want_p, want_d = ops.query_vjp_bf16(pp, dd, *state.geo, state.bwd_streams, state.bwd16, bits, gg)
    torch.cuda.synchronize()
    assert acts.shape == (4, batch, n, 128) and torch.equal(acts, want_acts[:, :, :n])
    assert p.grad.shape == (batch, n, 3) and p.grad.abs().max() > 0
    if views == 1:
        assert torch.equal(p.grad, want_p) and torch.equal(d.grad, want_d)
    else:                                                       # the layer-0 pass sums the views with atomics: the order of V addends
        for got, want in ((p.grad, want_p[:, :n]), (d.grad, want_d[:, :n])):
            assert (got - want).abs().max() <= 4 * 2.0 ** -24 * want.abs().max()
    with pytest.raises(RuntimeError, match='no bf16 form'):     # the gradient of the gradient stays fp32
        g2 = g.clone().requires_grad_(True)
        d_points, _ = torch.autograd.grad((TrunkField.apply(p, d, state) * g2).sum(), (p, d), create_graph=True)
        d_points.sum().backward()


def test_infer_in_bf16_packs_its_weight_images_once():
    from thesis_clip_nerf_amd.lmvnerf import LanguageNeRF
    sc, _, _ = make_query(70, 1, 32, 1)
    model = LanguageNeRF(sc['fine'], n_views=1, device=DEV)
    inputs = (None, None, None, None, sc['images'], sc['intrinsics'], sc['extrinsics_inv'])
    transforms = torch.eye(4).repeat(1, 3, 1, 1)
    one = model.infer(inputs, transforms, 3, sc['features'], compute_dtype='bf16')
    first = model._infer_nets16()
    two = model.infer(inputs, transforms, 3, sc['features'], compute_dtype='bf16')
    assert one.shape == (1, 3) and torch.equal(one, two)
    assert all(a is b for a, b in zip(first, model._infer_nets16()))
    with torch.no_grad():
        model.trunk_net.mul_(0.5)                             # new weights: new images
    assert model._infer_nets16()[1] is not first[1]
    assert not torch.equal(model.infer(inputs, transforms, 3, sc['features'], compute_dtype='bf16'), one)
