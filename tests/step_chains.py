"""The multi-launch C entry points restated as their parts, and the fill protocol they are held to (tests/test_gpu_step_chains.py;
tests/test_step_protocol_cpu.py shows on CPU tensors that the protocol sees what it is for).

The protocol.  A step is a function `step(fill) -> {name: tensor}` that takes EVERY buffer it writes - its workspace and its outputs -
from `fill` (a `Fill`: every 32-bit word of such a buffer holds one fill word; an output has GUARD extra rows behind it, a workspace
TAIL_BYTES).  `run_fills` runs it once per word of FILL_WORDS and asserts after each run that the guard words kept the word;
`check_protocol` then asserts, in this order and with the cause in the message,
  1. that no output element holds the fill word under every fill (never written),
  2. that every order-fixed output has the same bits under the three fills (a difference: the step reads memory it did not write; if
     the zero fill alone gives the bits of the parts, it adds into memory it did not zero),
  3. that every output is finite,
  4. that every order-fixed output has the bits of `want`, the chain of the step's parts.
Nothing here carries a tolerance: order-free outputs (`order_free`) are only held to 1 and 3, their bars belong to the caller.

The chains.  `render_chain`, `train_chain` + `apply_chain` and `grasp_chain` run, in the order of the C source (csrc/api.hip
`render_fwd`, csrc/train_api.hip `mvnerf_loss_and_grads` / `mvnerf_apply_gradients`, csrc/grasp_api.hip `run`), the public entry
points the steps are made of.  They call the C ABI through `ops._lib` (as tests/test_gpu_ray_backward.py::call does) rather than the
`ops` wrappers: most wrappers allocate their own outputs and scratch with torch.empty, and here every buffer a launch writes belongs
to the caller and comes from `fill` - own rgbs, own stash, own field workspace per pass, where the step shares one.
"""
import ctypes

import numpy as np
import torch

from thesis_clip_nerf_amd import ops

NAN_WORD = 0x7FC00000                                    # the suite's quiet-NaN pattern
FILL_WORDS = (0x00000000, NAN_WORD, 0x3F800000)          # zeros (hides a sum into an un-zeroed buffer), NaN, 1.0f (a plausible value)
GUARD = 4                                                # extra rows behind an output buffer
TAIL_BYTES = 4096                                        # behind a workspace
NP = ops.NET_PARAMS


# ---- fill, guard, bit-compare: any device -------------------------------------------------------------------------------------------------
def filled(nbytes_or_shape, word, device='cpu', dtype=torch.float32):
    """A buffer whose every 32-bit word is `word`, with its guard.  An int is a workspace of that many bytes (uint8, TAIL_BYTES behind
    it), a shape an output tensor of a 4-byte dtype (GUARD more rows along the first axis).  -> (buffer, whole): `whole` is the int32
    allocation the buffer is the front of."""
    if isinstance(nbytes_or_shape, (int, np.integer)):
        nbytes = int(nbytes_or_shape)
        assert nbytes >= 0 and nbytes % 4 == 0, nbytes
        whole = torch.full(((nbytes + TAIL_BYTES) // 4,), word, dtype=torch.int32, device=device)
        return whole.view(torch.uint8)[:nbytes], whole
    shape = tuple(int(s) for s in nbytes_or_shape)
    assert torch.empty(0, dtype=dtype).element_size() == 4, dtype
    whole = torch.full((shape[0] + GUARD,) + shape[1:], word, dtype=torch.int32, device=device)
    return whole.view(dtype)[:shape[0]], whole


def guard_words(buf, whole):
    """The words of `whole` behind `buf`."""
    return whole.reshape(-1)[buf.numel() * buf.element_size() // 4:]


def assert_guard(buf, whole, word, name='buffer'):
    bad = int((guard_words(buf, whole) != word).sum())
    assert bad == 0, f'{name}: {bad} guard words behind it no longer hold {word:#010x}: the step wrote past the end of {name}'


class Fill:
    """Hands out buffers filled with one word and remembers them for `assert_guards`.  init: values to copy into the buffer (an in/out
    state such as Adam moments: the guard keeps the word)."""

    def __init__(self, word, device):
        self.word, self.device, self.owned = word, device, []

    def __call__(self, nbytes_or_shape, dtype=torch.float32, name=None, init=None):
        buf, whole = filled(nbytes_or_shape, self.word, self.device, dtype)
        if init is not None:
            buf.copy_(init.reshape(buf.shape))
        self.owned.append((name or f'buffer {len(self.owned)}', buf, whole))
        return buf

    def assert_guards(self):
        for name, buf, whole in self.owned:
            assert_guard(buf, whole, self.word, name)


def bits(t):
    """A tensor's 32-bit words."""
    t = t.contiguous()
    return t if t.dtype == torch.int32 else t.view(torch.int32)


def run_fills(step, device, sync=None):
    """step(fill) -> {name: tensor}, once per fill word on fresh buffers.  -> [(word, {name: clone})]"""
    runs = []
    for word in FILL_WORDS:
        fill = Fill(word, device)
        out = step(fill)
        if sync is not None:
            sync()
        fill.assert_guards()
        runs.append((word, {k: v.detach().clone() for k, v in out.items()}))
    return runs


def check_protocol(runs, want=None, order_free=()):
    """Assertions 1-4 of the module docstring on the result of run_fills.  want: {name: tensor} of the chain (every order-fixed name)."""
    names = list(runs[0][1])
    for name in names:
        unwritten = None
        for word, out in runs:
            m = bits(out[name]) == word
            unwritten = m if unwritten is None else unwritten & m
        n = int(unwritten.sum())
        assert n == 0, f'{name}: {n} of {unwritten.numel()} elements hold the fill word under every fill: never written'
    fixed = [n for n in names if n not in order_free]
    zero_run = runs[0][1]
    for name in fixed:
        differ = [f'{word:#010x}' for word, out in runs[1:] if not torch.equal(bits(out[name]), bits(zero_run[name]))]
        if differ:
            if want is not None and torch.equal(bits(zero_run[name]), bits(want[name])):
                cause = 'right under the zero fill alone: the step adds into memory it did not zero'
            else:
                cause = 'the step reads memory it did not write'
            raise AssertionError(f'{name}: fills {", ".join(differ)} give other bits than fill 0x00000000 - {cause}')
    for word, out in runs:
        for name in names:
            if out[name].is_floating_point():
                assert bool(torch.isfinite(out[name]).all()), f'{name}: not finite under fill {word:#010x}'
    if want is not None:
        for name in fixed:
            got, ref = bits(zero_run[name]), bits(want[name])
            assert got.shape == ref.shape, (name, got.shape, ref.shape)
            n = int((got != ref).sum())
            assert n == 0, f'{name}: {n} of {got.numel()} elements differ from the chain of the parts'


# ---- the C ABI on caller-owned buffers -------------------------------------------------------------------------------------------------------
def call(name, *args):
    """A C entry point on the current stream: tensors go as their pointers, everything else as it is."""
    tensors = [a for a in args if isinstance(a, torch.Tensor)]
    conv = [ctypes.c_void_p(a.data_ptr()) if isinstance(a, torch.Tensor) else a for a in args]
    with torch.cuda.device(tensors[0].device):
        rc = getattr(ops._lib.lib(), name)(*conv, ops._stream(tensors[0]))
    ops._lib.check(rc, name)


def size(name, *dims):
    return int(getattr(ops._lib.lib(), name)(*dims))


# ---- render ----------------------------------------------------------------------------------------------------------------------------------
def field_pass(fill, d, kind, z, table, packed, split, s, which=-1, status=None):
    """The plain field pass of a render step of `kind` ('fp32', 'split', 'ex') on depths z (B, R, s) -> rgbs (B, R, s, 4)."""
    b, v, r, h, w = (d[k] for k in 'BVRHW')
    rgbs = fill((b, r, s, 4), name='rgbs')
    ws = fill(size('mvnerf_field_workspace_bytes', b, v, r), name='field workspace')
    geo = (d['rays_o'], d['rays_d'], z, d['images'], d['features'])
    cams = (d['intrinsics'], d['extrinsics_inv'])
    outs = (rgbs, None, None, None, None, None, ws)
    if kind == 'fp32':
        if table is None:
            call('mvnerf_field_eval', *geo, *cams, packed, b, v, r, s, h, w, *outs)
        else:
            call('mvnerf_field_eval_table', *geo, table, *cams, packed, b, v, r, s, h, w, *outs)
    elif kind == 'split':
        call('mvnerf_field_eval_split', *geo, table, *cams, packed, split, b, v, r, s, h, w, *outs)
    else:
        call('mvnerf_field_eval_split_ex', *geo, table, *cams, packed, split, b, v, r, s, h, w, *outs, which, status)
    return rgbs


def render_chain(fill, d, kind, tables, which=-1, status=None):
    """render_fwd of csrc/api.hip.  tables: None, 'built' (project_texels2 runs first, into a buffer of the chain's) or a ready
    (2, B, V, H, W, 128) tensor.  status: the two range-status floats of the _ex entry point (coarse, fine)."""
    b, v, r, s, h, w = (d[k] for k in 'BVRSHW')
    n = b * r
    out = {}
    if isinstance(tables, str):
        tab = fill((2, b, v, h, w, 128), name='texel tables')
        call('mvnerf_project_texels2', d['features'], d['packed'][0], d['packed'][1], b, v, h, w, tab[0], tab[1])
        out['tables'] = tab
    else:
        tab = tables
    tab_c, tab_f = (None, None) if tab is None else (tab[0], tab[1])
    z = fill((b, r, s), name='z')
    call('mvnerf_stratified_depths', d['u_coarse'], n, s, d['near'], d['far'], z)
    rgbs_c = field_pass(fill, d, kind, z, tab_c, d['packed'][0], d['split'][0], s, which, None if status is None else status[0:1])
    rgb, depth, weights = fill((b, r, 3), name='rgb'), fill((b, r), name='depth'), fill((b, r, s), name='weights')
    call('mvnerf_composite', z, rgbs_c, n, s, rgb, depth, weights)
    z_all = fill((b, r, 2 * s), name='z_all')
    call('mvnerf_resample', z, weights, d['u_fine'], n, s, d['q7'], z_all, None, None, None, None)
    rgbs_f = field_pass(fill, d, kind, z_all, tab_f, d['packed'][1], d['split'][1], 2 * s, which, None if status is None else status[1:2])
    fine_rgb, fine_depth = fill((b, r, 3), name='fine_rgb'), fill((b, r), name='fine_depth')
    call('mvnerf_composite', z_all, rgbs_f, n, 2 * s, fine_rgb, fine_depth, None)
    out.update(rgb=rgb, depth=depth, fine_rgb=fine_rgb, fine_depth=fine_depth)
    if status is not None:
        out['status'] = status
    return out


def render_step(fill, d, kind, tables, which=-1, status=None):
    """The step itself: mvnerf_render_fwd / _split / _split_ex on a filled workspace of exactly mvnerf_render_workspace_bytes."""
    b, v, r, s, h, w = (d[k] for k in 'BVRSHW')
    out = {}
    ready = 0
    if isinstance(tables, str):
        tab = out['tables'] = fill((2, b, v, h, w, 128), name='texel tables')
    else:
        tab, ready = tables, int(tables is not None)
    ws = fill(size('mvnerf_render_workspace_bytes', b, v, r, s), name='workspace')
    rgb, depth, fine_rgb, fine_depth = fill((b, r, 3), name='rgb'), fill((b, r), name='depth'), fill((b, r, 3), name='fine_rgb'), fill((b, r), name='fine_depth')
    front = (d['rays_o'], d['rays_d'], d['images'], d['features'], d['intrinsics'], d['extrinsics_inv'], d['packed'][0], d['packed'][1])
    back = (d['u_coarse'], d['u_fine'], b, v, r, s, h, w, d['near'], d['far'], d['q7'], rgb, depth, fine_rgb, fine_depth, ws, tab, ready)
    if kind == 'fp32':
        call('mvnerf_render_fwd', *front, *back)
    elif kind == 'split':
        call('mvnerf_render_fwd_split', *front, d['split'][0], d['split'][1], *back)
    else:
        call('mvnerf_render_fwd_split_ex', *front, d['split'][0], d['split'][1], *back, which, status)
        out['status'] = status
    out.update(rgb=rgb, depth=depth, fine_rgb=fine_rgb, fine_depth=fine_depth)
    return out


# ---- training --------------------------------------------------------------------------------------------------------------------------------
def train_chain(fill, d, use_split, stop_fine_z, use_tables, want_d_features):
    """mvnerf_loss_and_grads line by line.  -> (outputs, aux): aux keeps what the d_features reference needs (depths, the two stashes,
    rgbs and their cotangents)."""
    b, v, r, s, h, w = (d[k] for k in 'BVRSHW')
    n = b * r
    geo = (d['rays_o'], d['rays_d'])
    src = (d['images'], d['features'])
    cams = (d['intrinsics'], d['extrinsics_inv'])
    tab_c = tab_f = None
    if use_tables:
        tab = fill((2, b, v, h, w, 128), name='texel tables')
        call('mvnerf_project_texels2', d['features'], d['packed'][0], d['packed'][1], b, v, h, w, tab[0], tab[1])
        tab_c, tab_f = tab[0], tab[1]

    def forward(z, table, k, ss):
        rgbs = fill((b, r, ss, 4), name='rgbs')
        stash = fill(size('mvnerf_stash_bytes', b, v, r, ss), name='stash')
        ws = fill(size('mvnerf_field_workspace_bytes', b, v, r), name='field workspace')
        if use_split:
            call('mvnerf_field_eval_stash_split', *geo, z, *src, table, *cams, d['packed'][k], d['split'][k], b, v, r, ss, h, w, rgbs, stash, ws)
        else:
            call('mvnerf_field_eval_stash', *geo, z, *src, table, *cams, d['packed'][k], b, v, r, ss, h, w, rgbs, stash, ws)
        return rgbs, stash

    z = fill((b, r, s), name='z')
    call('mvnerf_stratified_depths', d['u_coarse'], n, s, d['near'], d['far'], z)
    rgbs_c, stash_c = forward(z, tab_c, 0, s)
    rgb, depth, weights = fill((b, r, 3), name='rgb'), fill((b, r), name='depth'), fill((b, r, s), name='weights')
    call('mvnerf_composite', z, rgbs_c, n, s, rgb, depth, weights)
    z_all, rank = fill((b, r, 2 * s), name='z_all'), fill((b, r, s), dtype=torch.int32, name='rank')
    call('mvnerf_resample', z, weights, d['u_fine'], n, s, d['q7'], z_all, None, None, None, rank)
    rgbs_f, stash_f = forward(z_all, tab_f, 1, 2 * s)
    fine_rgb, fine_depth = fill((b, r, 3), name='fine_rgb'), fill((b, r), name='fine_depth')
    call('mvnerf_composite', z_all, rgbs_f, n, 2 * s, fine_rgb, fine_depth, None)
    loss = fill((1,), name='loss')
    loss.zero_()
    d_rgb, d_fine = fill((b, r, 3), name='d_rgb'), fill((b, r, 3), name='d_fine')
    call('mvnerf_mse_grad', rgb, d['labels'], n * 3, d_rgb, loss)
    call('mvnerf_mse_grad', fine_rgb, d['labels'], n * 3, d_fine, loss)
    grad = fill((2 * NP,), name='grad')
    grad.zero_()
    d_feat = None
    if want_d_features:
        d_feat = fill((b, v, h, w, 256), name='d_features')
        d_feat.zero_()
    d_rgbs_f = fill((b, r, 2 * s, 4), name='d_rgbs_f')
    d_z_all = None if stop_fine_z else fill((b, r, 2 * s), name='d_z_all')
    # V > 1: the step keeps the compositing term of dL/dz apart, lets the views add onto zeros (two such adds commute exactly) and
    # adds the term behind them; the add is done by hand in torch, one fp32 add per element as in the step
    dz_composite = fill((b, r, 2 * s), name='dz_composite') if v > 1 and not stop_fine_z else d_z_all
    call('mvnerf_composite_bwd', z_all, rgbs_f, d_fine, None, None, n, 2 * s, d_rgbs_f, dz_composite)
    if dz_composite is not d_z_all:
        d_z_all.zero_()

    def backward(zz, table, k, ss, stash, rgbs, d_rgbs, d_z):
        scratch = fill(size('mvnerf_field_backward_scratch_bytes', b, v, r, ss), name='backward scratch')
        texel_grad = fill((b, v, h, w, 128), name='texel_grad') if use_tables and want_d_features else None
        call('mvnerf_field_backward_table', *geo, zz, *src, table, texel_grad, *cams, d['nets'][k], d['bwd'][k], stash, rgbs, d_rgbs,
             b, v, r, ss, h, w, scratch, grad[k * NP:], d_z, d_feat)

    backward(z_all, tab_f, 1, 2 * s, stash_f, rgbs_f, d_rgbs_f, d_z_all)
    d_w = None
    if not stop_fine_z:
        if dz_composite is not d_z_all:
            d_z_all.add_(dz_composite)
        d_w = fill((b, r, s), name='d_w')
        call('mvnerf_resample_bwd', z, weights, d['u_fine'], rank, d_z_all, n, s, d['q7'], d_w)
    d_rgbs_c = fill((b, r, s, 4), name='d_rgbs_c')
    call('mvnerf_composite_bwd', z, rgbs_c, d_rgb, None, d_w, n, s, d_rgbs_c, None)
    backward(z, tab_c, 0, s, stash_c, rgbs_c, d_rgbs_c, None)
    out = dict(loss=loss, grad=grad, rgb=rgb, depth=depth, fine_rgb=fine_rgb, fine_depth=fine_depth)
    if want_d_features:
        out['d_features'] = d_feat
    aux = dict(z=z, z_all=z_all, stash_c=stash_c, stash_f=stash_f, rgbs_c=rgbs_c, rgbs_f=rgbs_f, d_rgbs_c=d_rgbs_c, d_rgbs_f=d_rgbs_f)
    return out, aux


def apply_chain(d, grad, m, v, adam):
    """mvnerf_apply_gradients: adam_clip on both nets, then the three weight images of each re-packed from the new variables; in
    place on d['nets'], m, v, d['packed'], d['split'], d['bwd'].  adam: dict lr_t, beta1, beta2, eps, clip, update_mask (or None)."""
    for k in range(2):
        mask = None if adam['update_mask'] is None else adam['update_mask'][k * NP:]
        call('mvnerf_adam_clip', d['nets'][k], grad[k * NP:], m[k * NP:], v[k * NP:], NP, adam['lr_t'], adam['beta1'], adam['beta2'],
             adam['eps'], adam['clip'], mask)
    for k in range(2):
        call('mvnerf_pack_net', d['nets'][k], d['packed'][k])
        if d['split'] is not None:
            call('mvnerf_pack_net_split', d['nets'][k], d['split'][k])
        call('mvnerf_pack_bwd_streams', d['nets'][k], d['bwd'][k])


def train_call(fill, d, use_split, stop_fine_z, use_tables, want_d_features):
    """A mvnerf_train_call on filled outputs and a filled workspace of exactly mvnerf_train_workspace_bytes.  -> (call, outputs, keep)"""
    b, v, r, s, h, w = (d[k] for k in 'BVRSHW')
    ws = fill(size('mvnerf_train_workspace_bytes', b, v, r, s, h, w, int(use_tables), int(want_d_features)), name='workspace')
    loss, grad = fill((1,), name='loss'), fill((2 * NP,), name='grad')
    outs = (fill((b, r, 3), name='rgb'), fill((b, r), name='depth'), fill((b, r, 3), name='fine_rgb'), fill((b, r), name='fine_depth'))
    d_feat = fill((b, v, h, w, 256), name='d_features') if want_d_features else None
    c = ops.train_call(d['rays_o'], d['rays_d'], d['images'], d['features'], d['intrinsics'], d['extrinsics_inv'], d['u_coarse'], d['u_fine'],
                       d['labels'], d['near'], d['far'], d['nets'], d['packed'], d['split'] if use_split else None, d['bwd'], loss, grad, outs, ws,
                       q7_mode=d['q7'], stop_fine_z=stop_fine_z, use_tables=use_tables, d_features=d_feat)
    assert c.workspace_bytes == ws.numel()
    out = dict(loss=loss, grad=grad, rgb=outs[0], depth=outs[1], fine_rgb=outs[2], fine_depth=outs[3])
    if want_d_features:
        out['d_features'] = d_feat
    return c, out, (ws, d)


# ---- grasp -----------------------------------------------------------------------------------------------------------------------------------
def grasp_ld(v, n):
    return n if v == 1 else -(-n // 32) * 32


def grasp_chain(fill, d, state, want_grads, bf16=False, adam=None):
    """Stages 1-8 of grasp_api.hip::run and the optimiser step behind it, on the poses in state['t'], state['rot'].

    The fp32 trunk stage is the internal pose_rows_trunk (csrc/mvnerf_api.h), which has no entry point of its own; it is two public
    ones called back to back, mvnerf_field_eval_stash_split on S = 1 and z = 0 (texel_table NULL) and mvnerf_stash_fused_acts, and
    those two are called here with the same arguments: the same kernels on the same operands, so the bits must agree.
    adam: dict cfg, flags, counters, m_t, v_t, m_r, v_r (stage 8, in place on them and on the poses)."""
    b, v, p, n5, h, w, rep = (d[k] for k in ('B', 'V', 'P', 'n5', 'H', 'W', 'rep'))
    n = p * n5
    ld = grasp_ld(v, n)
    rows = b * ld
    padded = ld > n
    t, rot = state['t'], state['rot']
    scene = (d['images'], d['features'], d['intrinsics'], d['extrinsics_inv'])
    points, dirs = fill((b, ld, 3), name='points'), fill((b, ld, 3), name='dirs')
    call('mvnerf_pose_query_points', t, rot, rep, d['offsets'], p, n5, b, ld, points, dirs)
    if padded:                                              # rows n .. ld of every scene repeat row n - 1 (pad_rows_kernel)
        points[:, n:] = points[:, n - 1:n]
        dirs[:, n:] = dirs[:, n - 1:n]
    acts = fill((4, rows, 128), name='acts')
    if bf16:
        stash = fill(size('mvnerf_relu_bits_bytes', b, v, ld), name='relu bits')
        ws = fill(size('mvnerf_query_workspace_bytes', b, v, ld), name='query workspace')
        call('mvnerf_query_stash_bf16', points, dirs, *scene, d['packed'], d['packed16'], b, v, ld, h, w, acts, stash, ws)
    else:
        z = fill((b, ld), name='z')
        z.zero_()
        rgbs = fill((b, ld, 4), name='rgbs')
        stash = fill(size('mvnerf_stash_bytes', b, v, ld, 1), name='stash')
        ws = fill(size('mvnerf_field_workspace_bytes', b, v, ld), name='field workspace')
        call('mvnerf_field_eval_stash_split', points, dirs, z, d['images'], d['features'], None, d['intrinsics'], d['extrinsics_inv'], d['packed'],
             d['split'], b, v, ld, 1, h, w, rgbs, stash, ws)
        call('mvnerf_stash_fused_acts', stash, b, v, ld, acts)
    c, y = fill((rows, 256), name='c'), fill((rows, 64), name='y')
    call('mvnerf_grasp_head_fwd', acts, d['head'], d['b4'], d['bc'], rows, c, y)
    success = fill((b, p), name='success')
    tail_stash = fill((b * p, ops.TAIL_STASH), name='tail stash') if want_grads else None
    scenes = range(b) if padded else range(1)               # padded scenes are ld * 64 floats apart: one tail call per scene
    m_call = p if padded else b * p
    y_of = lambda k: y.reshape(-1)[k * ld * 64:]
    for k in scenes:
        call('mvnerf_grasp_tail_fwd', y_of(k), d['tail'], m_call, n5, success.reshape(-1)[k * p:], None if tail_stash is None else tail_stash[k * p:])
    out = dict(success=success)
    if not want_grads:
        return out
    g_x = fill((rows, 64), name='g_x')
    if padded:
        g_x.view(b, ld, 64)[:, n:] = 0.0
    for k in scenes:
        call('mvnerf_grasp_tail_vjp', y_of(k), None, tail_stash[k * p:], d['tail'], m_call, n5, g_x.reshape(-1)[k * ld * 64:])
    g_acts = fill((4, rows, 128), name='g_acts')
    call('mvnerf_grasp_head_vjp_acts', g_x, c, y, d['head'], rows, g_acts)
    d_points, d_dirs = fill((b, ld, 3), name='d_points'), fill((b, ld, 3), name='d_dirs')
    if bf16:
        scratch = fill(size('mvnerf_query_vjp_bf16_scratch_bytes', b, v, ld), name='vjp scratch')
        call('mvnerf_query_vjp_bf16', points, dirs, *scene, d['bwd'], d['bwd16'], stash, g_acts, b, v, ld, h, w, scratch, d_points, d_dirs)
    else:
        scratch = fill(size('mvnerf_query_vjp_scratch_bytes', b, v, ld), name='vjp scratch')
        call('mvnerf_query_vjp', points, dirs, *scene, d['bwd'], stash, g_acts, b, v, ld, h, w, scratch, d_points, d_dirs)
    g_t, g_rot = fill((p, 3), name='g_t'), fill((p, rot.shape[-1]), name='g_rot')
    call('mvnerf_pose_query_vjp', rot, rep, d['offsets'], d_points, d_dirs, p, n5, b, ld, -1.0, g_t, g_rot)
    out.update(g_t=g_t, g_rot=g_rot)
    if adam is not None:
        call('mvnerf_pose_adam_step', ctypes.byref(adam['cfg']), rep, p, adam['flags'], adam['counters'], g_t, g_rot, adam['m_t'], adam['v_t'],
             adam['m_r'], adam['v_r'], t, rot)
    return out


def grasp_step(fill, d, state, entry, bf16=False, adam=None):
    """The step itself: `entry` in ('success', 'success_and_gradients', 'opt_step') on a filled workspace of exactly
    mvnerf_grasp_workspace_bytes[_bf16] and filled success / gradient buffers."""
    b, v, p, n5 = (d[k] for k in ('B', 'V', 'P', 'n5'))
    t, rot = state['t'], state['rot']
    ws = fill(size('mvnerf_grasp_workspace_bytes_bf16' if bf16 else 'mvnerf_grasp_workspace_bytes', b, v, p, n5), name='workspace')
    success, g_t, g_rot = fill((b, p), name='success'), fill((p, 3), name='g_t'), fill((p, rot.shape[-1]), name='g_rot')
    c = ops.grasp_call(d['images'], d['features'], d['intrinsics'], d['extrinsics_inv'], d['packed'], d['split'], d['bwd'], d['head'], d['b4'],
                       d['bc'], d['tail'], d['offsets'], t, rot, success, g_t, g_rot, ws)
    assert c.workspace_bytes == ws.numel()
    nets16 = (d['packed16'], d['bwd16']) if bf16 else None
    if entry == 'success':
        ops.grasp_success(c, t, nets16=nets16)
        return dict(success=success)
    if entry == 'success_and_gradients':
        ops.grasp_success_and_gradients(c, t, nets16=nets16)
    else:
        ops.grasp_opt_step(c, adam['cfg'], adam['flags'], adam['counters'], adam['m_t'], adam['v_t'], adam['m_r'], adam['v_r'], t, nets16=nets16)
    return dict(success=success, g_t=g_t, g_rot=g_rot)
