"""Stand-alone references for the ray-side kernels of the training step.  TEST INFRASTRUCTURE ONLY.

`mse_grad -> composite_bwd (fine) -> ... -> resample_bwd -> composite_bwd (coarse)` (csrc/train_ops.hip) and the forward kernels
they differentiate (`composite_kernel<P>`, `resample_kernel`, csrc/ray_ops.hip), restated in NumPy with a `dtype` argument: the
float64 run is the reference, the float32 run of the SAME algebra is the yardstick of the bar (`check`).  No torch in the arithmetic.

The resampling backward is split the way tests/test_gpu_field_backward.py splits the field backward: the forward's float32 `pdf`,
`cdf`, `bins` and every decision taken on them (`above`, `below`, `den_live`, `unit_sum`, `fine_rank`, the Q7-zero constant) come
from `resample_forward_f32`, which the kernel reproduces bit for bit; given those, the backward is a fixed linear map of `d_z_all`,
and its float64 evaluation has no branch to flip and no 1/den^2 amplification of forward rounding.

`mutant=` arguments exist for tests/test_ray_backward_ref.py only: each one plants a wrong term, and that test asserts that `check`
rejects it on the input set of tests/test_gpu_ray_backward.py (`composite_inputs`, `resample_inputs`, shared from here).
"""
from __future__ import annotations

import numpy as np

from oracle import mvnerf_oracle as O

F32 = np.float32
FACTOR = 8.0                     # the factor tests/test_gpu_field_backward.py uses; never fitted to a kernel
NAN_PATTERN = 0x7FC00000         # the quiet NaN the GPU tests fill every output buffer with

COMPOSITE_MUTANTS = ('no_q6_fold', 'no_relu_mask', 'no_eps', 'inclusive_suffix', 'suffix_by_difference')
RESAMPLE_MUTANTS = ('no_k2_in_dcb', 'const_gets_dca', 'dot_with_unit_sum', 'd_weights_off_by_one', 'last_writer_wins',
                    'unstable_rank')


# ------------------------------------------------------------------------------------------------------------
# volumetric_render (model_v0.py:89-100) and its backward
# ------------------------------------------------------------------------------------------------------------
def _composite_terms(z, rgbs, dtype):
    one = np.dtype(dtype).type(1.0)
    z = np.asarray(z).astype(dtype)
    c = np.asarray(rgbs).astype(dtype)
    sigma = c[..., 3]
    dist = z[..., 1:] - z[..., :-1]
    dist = np.concatenate([dist, dist[..., -1:]], axis=-1)                      # Q6: the last interval twice
    alpha = one - np.exp(-dist * np.maximum(sigma, one * 0))
    t = (one - alpha) + np.dtype(dtype).type(1e-10)
    incl = np.cumprod(t, axis=-1, dtype=dtype)
    trans = np.concatenate([np.ones_like(incl[..., :1]), incl[..., :-1]], axis=-1)   # exclusive
    return z, c, sigma, dist, alpha, t, trans, alpha * trans


def composite_ref(z, rgbs, dtype=np.float64):
    """z (...,S), rgbs (...,S,4) -> rgb (...,3), depth (...), weights (...,S); any S >= 2."""
    z, c, _, _, _, _, _, w = _composite_terms(z, rgbs, dtype)
    return (w[..., None] * c[..., :3]).sum(axis=-2, dtype=dtype), (w * z).sum(axis=-1, dtype=dtype), w


def composite_bwd_ref(z, rgbs, d_rgb, d_depth=None, d_weights=None, dtype=np.float64, mutant=None):
    """The formulas in the comment above composite_bwd_kernel: q_i = gR.c_i + gD z_i + gW_i, dL/dalpha_i = q_i T_i - (sum_{k>i}
    q_k w_k) / t_i with t_i = 1 - alpha_i + 1e-10, dL/dsigma_i = dL/dalpha_i delta_i (1 - alpha_i) [sigma_i > 0], dL/dc_i = w_i gR;
    dL/d delta_i = dL/dalpha_i sigma_i (1 - alpha_i) [sigma_i > 0], the duplicate last interval folded into the one before it, and
    dL/dz_k = dd_{k-1} - dd_k + w_k gD.  None cotangents are zero.  -> d_rgbs (...,S,4), d_z (...,S)."""
    assert mutant is None or mutant in COMPOSITE_MUTANTS, mutant
    z, c, sigma, dist, alpha, t, trans, w = _composite_terms(z, rgbs, dtype)
    zero, one = np.dtype(dtype).type(0.0), np.dtype(dtype).type(1.0)
    g_rgb = np.asarray(d_rgb).astype(dtype)
    g_d = np.zeros(z.shape[:-1], dtype) if d_depth is None else np.asarray(d_depth).astype(dtype)
    q = (c[..., :3] * g_rgb[..., None, :]).sum(axis=-1, dtype=dtype) + g_d[..., None] * z
    if d_weights is not None:
        q = q + np.asarray(d_weights).astype(dtype)
    qw = q * w
    incl_suffix = np.cumsum(qw[..., ::-1], axis=-1, dtype=dtype)[..., ::-1]        # sum_{k >= i}
    suffix = np.concatenate([incl_suffix[..., 1:], np.zeros_like(qw[..., :1])], axis=-1)
    if mutant == 'inclusive_suffix':
        suffix = incl_suffix
    if mutant == 'suffix_by_difference':         # what composite_bwd_kernel did until these tests: no digit of a t_i times smaller tail
        suffix = incl_suffix - qw
    pos = (one - alpha) if mutant == 'no_relu_mask' else np.where(sigma > zero, one - alpha, zero)
    with np.errstate(divide='ignore', invalid='ignore'):                          # the no_eps mutant divides by zero
        dalpha = q * trans - suffix / ((one - alpha) if mutant == 'no_eps' else t)
        dd = dalpha * sigma * pos
        d_rgbs = np.concatenate([w[..., None] * g_rgb[..., None, :], (dalpha * dist * pos)[..., None]], axis=-1)
    if mutant != 'no_q6_fold':
        dd[..., -2] = dd[..., -2] + dd[..., -1]
    dd[..., -1] = zero
    prev = np.concatenate([np.zeros_like(dd[..., :1]), dd[..., :-1]], axis=-1)
    d_z = (prev - dd) + w * g_d[..., None]
    assert d_rgbs.dtype == np.dtype(dtype) and d_z.dtype == np.dtype(dtype)
    return d_rgbs, d_z


# ------------------------------------------------------------------------------------------------------------
# sample_pdf + sort-merge (nerf_utils.py:143-176, model_v0.py:150-156) and the backward w.r.t. the coarse weights
# ------------------------------------------------------------------------------------------------------------
def stable_rank(z, z_fine, reverse_ties=False):
    """Position of importance sample i inside sort([coarse | fine]); ties keep the concatenation's order (coarse first, then by
    index), which is what resample_kernel's rank count does.  reverse_ties: the opposite order on ties (a mutant)."""
    both = np.concatenate([z, z_fine], axis=-1)
    n = both.shape[-1]
    if reverse_ties:
        order = (n - 1) - np.argsort(both[..., ::-1], axis=-1, kind='stable')
    else:
        order = np.argsort(both, axis=-1, kind='stable')
    pos = np.empty_like(order)
    np.put_along_axis(pos, order, np.broadcast_to(np.arange(n), order.shape), axis=-1)
    return pos[..., z.shape[-1]:].astype(np.int32)


def resample_forward(z, weights, u_fine, q7_mode, dtype):
    """The forward in `dtype`, the op sequence of oracle.sample_pdf (sequential sums): values and decisions."""
    ty = np.dtype(dtype).type
    z, w, u = (np.asarray(a).astype(dtype) for a in (z, weights, u_fine))
    bins = ty(0.5) * (z[..., 1:] + z[..., :-1])
    eps = ty(F32(1e-5) if np.dtype(dtype) == np.float32 else 1e-5)               # the float32 kernel's 1e-5f / the twin's 1e-5
    stable = w[..., 1:-1] + eps
    wsum = np.cumsum(stable, axis=-1, dtype=dtype)[..., -1:]
    unit_sum = np.abs(wsum) == 0
    wsum = np.where(unit_sum, np.ones_like(wsum), wsum)
    pdf = stable / wsum
    cdf = np.cumsum(pdf, axis=-1, dtype=dtype)
    cdf = np.concatenate([np.zeros_like(cdf[..., :1]), cdf], axis=-1)
    nb = bins.shape[-1]
    above = (u[..., :, None] >= cdf[..., None, :]).sum(axis=-1).astype(np.int32)
    below = np.clip(above - 1, 0, nb - 1).astype(np.int32)
    fwd = dict(z=z, bins=bins, pdf=pdf, cdf=cdf, wsum=wsum[..., 0], unit_sum=unit_sum[..., 0], above=above, below=below)
    cdf_a, cdf_b, bins_a, bins_b = _gathers(fwd, q7_mode)
    den_raw = cdf_a - cdf_b
    fwd['den_live'] = ~(den_raw < eps)
    den = np.where(fwd['den_live'], den_raw, np.ones_like(den_raw))
    fwd['z_fine'] = bins_b + ((u - cdf_b) / den) * (bins_a - bins_b)
    fwd['z_all'] = np.sort(np.concatenate([z, fwd['z_fine']], axis=-1), axis=-1)
    fwd['fine_rank'] = stable_rank(z, fwd['z_fine'])
    return fwd


def _gathers(fwd, q7_mode):
    nb = fwd['bins'].shape[-1]
    ia = np.minimum(fwd['above'], nb - 1).astype(np.int64)
    a_const = (fwd['above'] >= nb) & (q7_mode == O.Q7_ZERO)                     # the gathered value is the constant 0
    take = np.take_along_axis
    cdf_a = np.where(a_const, np.zeros_like(fwd['cdf'][..., :1]), take(fwd['cdf'], ia, axis=-1))
    bins_a = np.where(a_const, np.zeros_like(fwd['bins'][..., :1]), take(fwd['bins'], ia, axis=-1))
    ib = fwd['below'].astype(np.int64)
    return cdf_a, take(fwd['cdf'], ib, axis=-1), bins_a, take(fwd['bins'], ib, axis=-1)


def resample_forward_f32(z, weights, u_fine, q7_mode):
    """What resample_kernel computes, in its float32: `z_all`, `z_fine`, `above`, `below` from oracle.hierarchical_depths, the
    intermediates (`bins`, `pdf`, `cdf`, `wsum` - 1 where `unit_sum` -, `den_live`) by the same sequential float32 sums, and
    `fine_rank` from a stable sort of [coarse | fine]."""
    z, weights, u_fine = (np.ascontiguousarray(a, dtype=F32) for a in (z, weights, u_fine))
    fwd = resample_forward(z, weights, u_fine, q7_mode, F32)
    z_all, z_fine, above, below = O.hierarchical_depths(z, weights, u_fine, q7_mode, return_indices=True)
    fwd.update(z_all=z_all, z_fine=z_fine, above=above.astype(np.int32), below=below.astype(np.int32))
    fwd['fine_rank'] = stable_rank(z, z_fine)
    assert all(fwd[k].dtype == F32 for k in ('bins', 'pdf', 'cdf', 'wsum', 'z_fine', 'z_all'))
    return fwd


def resample_bwd_ref(fwd, u_fine, d_z_all, q7_mode, dtype=np.float64, mutant=None):
    """The linear map of resample_bwd_kernel in `dtype` on the values of `fwd` (float32 ones from resample_forward_f32, or float64
    ones from resample_forward for the check against autograd), every decision taken from `fwd`.  -> d_weights (...,S)."""
    assert mutant is None or mutant in RESAMPLE_MUTANTS, mutant
    vals = {k: (np.asarray(v).astype(dtype) if np.asarray(v).dtype.kind == 'f' else np.asarray(v)) for k, v in fwd.items()}
    u = np.asarray(u_fine).astype(dtype)
    g_all = np.asarray(d_z_all).astype(dtype)
    zero = np.dtype(dtype).type(0.0)
    nb = vals['bins'].shape[-1]
    lead = u.shape[:-1]
    cdf_a, cdf_b, bins_a, bins_b = _gathers(vals, q7_mode)
    a_const = (vals['above'] >= nb) & (q7_mode == O.Q7_ZERO)
    live = vals['den_live']
    den = np.where(live, cdf_a - cdf_b, np.ones_like(cdf_a))
    rank = stable_rank(fwd['z'], fwd['z_fine'], reverse_ties=True) if mutant == 'unstable_rank' else vals['fine_rank']
    dzf = np.take_along_axis(g_all, rank.astype(np.int64), axis=-1)
    dt = dzf * (bins_a - bins_b)
    k2 = np.where(live, dt * (u - cdf_b) / (den * den), zero)
    dca = -k2
    dcb = -dt / den + (zero if mutant == 'no_k2_in_dcb' else k2)
    if mutant != 'const_gets_dca':
        dca = np.where(a_const, zero, dca)
    ia = np.minimum(vals['above'], nb - 1).astype(np.int64)
    ib = vals['below'].astype(np.int64)
    # scatter-add into d cdf in the kernel's order: lane after lane, `above` then `below`
    idx = np.stack([ia, ib], axis=-1).reshape(-1, 2 * u.shape[-1])
    add = np.stack([dca, dcb], axis=-1).reshape(idx.shape)
    dcdf = np.zeros((idx.shape[0], nb), dtype)
    rows = np.arange(idx.shape[0])
    if mutant == 'last_writer_wins':
        skip = np.stack([a_const, np.zeros_like(a_const)], axis=-1).reshape(idx.shape)
        for s in range(idx.shape[1]):
            keep = ~skip[:, s]
            dcdf[rows[keep], idx[keep, s]] = add[keep, s]
    else:
        np.add.at(dcdf, (rows[:, None], idx), add)
    # cdf_j = sum_{k<j} pdf_k -> d pdf_k = sum_{j>k} d cdf_j ; pdf_k = s_k / wsum -> d s_k = (d pdf_k - sum_m d pdf_m pdf_m) / wsum
    dpdf = np.cumsum(dcdf[:, :0:-1], axis=-1, dtype=dtype)[:, ::-1]
    pdf = vals['pdf'].reshape(dpdf.shape)
    dot = (dpdf * pdf).sum(axis=-1, dtype=dtype)
    if mutant != 'dot_with_unit_sum':
        dot = np.where(vals['unit_sum'].reshape(-1), zero, dot)                  # wsum is the constant 1 there
    ds = (dpdf - dot[:, None]) / vals['wsum'].reshape(-1, 1)
    pad = np.zeros((ds.shape[0], 1), dtype)
    out = np.concatenate([ds, pad, pad] if mutant == 'd_weights_off_by_one' else [pad, ds, pad], axis=-1)   # probs = weights[1:-1]
    assert out.dtype == np.dtype(dtype)
    return out.reshape(lead + (nb + 1,))


# ------------------------------------------------------------------------------------------------------------
# Keras MeanSquaredError and its gradient
# ------------------------------------------------------------------------------------------------------------
def mse_grad_ref(pred, label, dtype=np.float64):
    """-> d_pred = 2 (pred - label) (1 / n), loss = sum (pred - label)^2 (1 / n): mse_grad_kernel's op sequence per element (in
    float32 `1 / n` is the rounded reciprocal the launcher passes); the loss is a plain sum in `dtype`."""
    ty = np.dtype(dtype).type
    d = np.asarray(pred).astype(dtype) - np.asarray(label).astype(dtype)
    inv_n = ty(1.0) / ty(d.size)
    return (ty(2.0) * d) * inv_n, ((d * d) * inv_n).sum(dtype=dtype)


def mse_loss_f32_accumulated(pred, label, start, order=None):
    """The float32 value mse_grad_kernel leaves in a loss buffer that held `start`: every 64 consecutive elements are one wave,
    summed by the xor butterfly (a balanced tree), and each wave's non-zero total is added to the buffer with one atomic.  The
    hardware fixes no order for those adds; `order` is a permutation of the waves (default: ascending)."""
    d = (np.asarray(pred, F32) - np.asarray(label, F32)).ravel()
    inv_n = F32(1.0) / F32(d.size)
    sq = np.zeros(-(-d.size // 64) * 64, F32)
    sq[:d.size] = (d * d) * inv_n
    v = sq.reshape(-1, 64)
    for off in (32, 16, 8, 4, 2, 1):
        v = v[:, :off] + v[:, off:2 * off]
    acc = F32(start)
    for k in (range(v.shape[0]) if order is None else order):
        if v[k, 0] != 0:
            acc = F32(acc + v[k, 0])
    return acc


# ------------------------------------------------------------------------------------------------------------
# the bar
# ------------------------------------------------------------------------------------------------------------
def check(tag, got, ref64, ref32, factor=FACTOR):
    """got, ref64, ref32: dicts name -> array whose first axis is the ray.  For every array, with e64 = |got - ref64| and e32 =
    |ref32 - ref64| (ref32 = the float32 run of the same reference), asserts e64 <= factor * e32 in three measures - L2 over the
    array, max over the array relative to the array's maximum, and the worst ray's max relative to that ray's own reference maximum
    (against the worst ray of the float32 run) -, that `got` is finite, and that it is exactly zero wherever ref64 is exactly zero.
    Prints every figure first; returns the largest e64 / e32."""
    bad, worst = [], 0.0
    for name, r64 in ref64.items():
        r64 = np.asarray(r64, np.float64)
        n = r64.shape[0]
        r64 = r64.reshape(n, -1)
        g = np.asarray(got[name], np.float64).reshape(r64.shape)
        r32 = np.asarray(ref32[name], np.float64).reshape(r64.shape)
        if not np.isfinite(g).all():
            bad.append((name, 'not finite'))
            continue
        if np.count_nonzero(g[r64 == 0]):
            bad.append((name, 'not exactly zero where the reference is', int(np.count_nonzero(g[r64 == 0]))))
        m = np.abs(r64).max()
        if m == 0:
            print(f'{tag} {name:10s} reference is zero')
            continue
        d64, d32 = np.abs(g - r64), np.abs(r32 - r64)
        nrm = np.linalg.norm(r64)
        ray_m = np.abs(r64).max(axis=1)
        live = ray_m > 0
        with np.errstate(over='ignore'):                                         # a ray whose own maximum is subnormal
            measures = [('L2', np.linalg.norm(d64) / nrm, np.linalg.norm(d32) / nrm), ('max', d64.max() / m, d32.max() / m),
                        ('ray', (d64.max(axis=1)[live] / ray_m[live]).max(), (d32.max(axis=1)[live] / ray_m[live]).max())]
        for kind, e64, e32 in measures:
            ratio = e64 / e32 if e32 > 0 else (0.0 if e64 == 0 else np.inf)
            print(f'{tag} {name:10s} {kind:3s}: e64 {e64:.3e}  e32 {e32:.3e}  e64/e32 {ratio:.2f}')
            worst = max(worst, ratio)
            if not e64 <= factor * e32:
                bad.append((name, kind, e64, e32, ratio))
    print(f'{tag} largest e64/e32: {worst:.2f}')
    assert not bad, (tag, bad)
    return worst


# ------------------------------------------------------------------------------------------------------------
# the input set of tests/test_gpu_ray_backward.py (the mutant test of tests/test_ray_backward_ref.py runs on the same)
# ------------------------------------------------------------------------------------------------------------
COMPOSITE_S = (64, 128)
COMPOSITE_RAYS = (1, 5, 1027)                 # a lone wave, a ragged workgroup, many workgroups
SIGMA_SCALES = (30.0, 3e3, 3e5)               # alpha <= 0.35 / saturating / opaque within one sample
COTANGENT_SETS = ('all', 'fine', 'coarse', 'zero')
RESAMPLE_RAYS = (1, 5, 301)


def composite_inputs(s, n_rays, scale, seed=0):
    """z (n,S) ascending float32 in [0.3, 1.3], rgbs (n,S,4) with sigma = scale * U(-0.1, 1) (about a tenth negative), and the three
    cotangents.  Ray 0 has two equal depths and its first five depths at 0 (importance samples outside [near, far] under Q7 zero);
    ray 1 (where there is one) has no positive density."""
    rng = np.random.default_rng([seed, s, n_rays, int(scale)])
    z = np.sort(rng.uniform(0.3, 1.3, (n_rays, s)), axis=-1).astype(F32)
    rgbs = rng.random((n_rays, s, 4)).astype(F32)
    rgbs[..., 3] = ((rng.random((n_rays, s)) * 1.1 - 0.1) * scale).astype(F32)
    z[0, :5] = 0.0
    z[0, s // 3 + 1] = z[0, s // 3]
    if n_rays > 1:
        rgbs[1, :, 3] = -np.abs(rgbs[1, :, 3])
        rgbs[1, ::7, 3] = 0.0
    return dict(z=z, rgbs=rgbs, d_rgb=rng.standard_normal((n_rays, 3)).astype(F32),
                d_depth=rng.standard_normal(n_rays).astype(F32), d_weights=rng.standard_normal((n_rays, s)).astype(F32))


def cotangents(inp, which):
    """-> (d_rgb, d_depth, d_weights, want_dz): 'fine' and 'coarse' are the two calls of the training step."""
    if which == 'all':
        return inp['d_rgb'], inp['d_depth'], inp['d_weights'], True
    if which == 'fine':
        return inp['d_rgb'], None, None, True
    if which == 'coarse':
        return inp['d_rgb'], None, inp['d_weights'], False
    assert which == 'zero'
    return np.zeros_like(inp['d_rgb']), np.zeros_like(inp['d_depth']), np.zeros_like(inp['d_weights']), True


def composite_bwd_refs(inp, which, mutant=None):
    """-> (ref64, ref32) dicts for `check`; `mutant` plants a wrong term in the float32 run (returned in place of ref32)."""
    g_rgb, g_d, g_w, want_dz = cotangents(inp, which)
    out = []
    for dtype, mut in ((np.float64, None), (F32, mutant)):
        d_rgbs, d_z = composite_bwd_ref(inp['z'], inp['rgbs'], g_rgb, g_d, g_w, dtype, mutant=mut)
        out.append(dict(d_rgbs=d_rgbs, d_z=d_z) if want_dz else dict(d_rgbs=d_rgbs))
    return out


def unit_sum_pair():
    """Two float32 weights w_lo, w_hi with fl(w_lo + 1e-5f) = -fl(w_hi + 1e-5f) != 0."""
    eps = F32(1e-5)
    w_hi = F32(0.25)
    target = -F32(w_hi + eps)
    w_lo = F32(target - eps)
    for _ in range(8):
        if F32(w_lo + eps) == target:
            return w_lo, w_hi
        w_lo = np.nextafter(w_lo, F32(0) if F32(w_lo + eps) < target else F32(-1), dtype=F32)
    raise AssertionError('no float32 weight cancels 0.25 + 1e-5f')


def _u_landing_on(z_ray, w_ray, targets):
    """A float32 u whose importance sample is exactly one of `targets` (coarse depths of that ray), by bisection over the bit
    patterns of u: a tie between an importance sample with a live gradient and a coarse depth, which only a stable rank orders."""
    def z_fine(bits):
        uu = np.array([[[bits]]], np.int32).view(F32)
        bins = (F32(0.5) * (z_ray[1:] + z_ray[:-1]).astype(F32)).astype(F32)
        return O.sample_pdf(bins[None, None], w_ray[None, None, 1:-1], uu)[0, 0, 0]
    for target in targets:
        lo, hi = 0, int(np.array(1.0, F32).view(np.int32)) - 1              # u in [0, 1)
        while hi - lo > 1:
            mid = (lo + hi) // 2
            lo, hi = (mid, hi) if z_fine(mid) < target else (lo, mid)
        if z_fine(hi) == target:
            return np.array(hi, np.int32).view(F32)
    raise AssertionError('no u lands on a coarse depth')


def resample_inputs(n_rays, seed=0, edge_u=True):
    """z, weights, u_fine (n,64) float32 and d_z_all (n,128).  Rays by index, as far as n_rays goes: 0 weights random^4, eight
    equal u, z_0 = z_1 (so the u = 0 sample lands exactly on two coarse depths); 1 all-zero weights, and u_5 chosen so that its
    importance sample equals a coarse depth; 2 zero from index 10 on; 3 a
    one-bin surface; 4 weights = -1e-5f exactly (wsum == 0: unit_sum); 5 weights + 1e-5f = (a, 0, ..., 0, -a): unit_sum with a
    non-zero pdf, the only place where skipping `dot` matters; every seventh ray after that has z_0 = z_1 again.  Column 0 of u is
    0; with edge_u column 1 is nextafter(1, 0) (the Q7 edge)."""
    rng = np.random.default_rng([seed, n_rays])
    u_c = rng.random((1, n_rays, 64)).astype(F32)
    _, z = O.sample_along_ray(np.zeros((1, n_rays, 3), F32), np.ones((1, n_rays, 3), F32), 0.3, 1.3, 64, u_c)
    z = z[0].copy()
    w = (rng.random((n_rays, 64)) ** 4).astype(F32)
    u = rng.random((n_rays, 64)).astype(F32)
    u[:, 0] = 0.0
    if edge_u:
        u[:, 1] = np.nextafter(F32(1), F32(0), dtype=F32)
    u[0, 8:16] = u[0, 8]
    z[0::7, 1] = z[0::7, 0]
    if n_rays > 1:
        w[1] = 0.0
        u[1, 5] = _u_landing_on(z[1], w[1], z[1, 20:44])
    if n_rays > 2:
        w[2, 10:] = 0.0
    if n_rays > 3:
        w[3] = 0.0
        w[3, 37] = 1.0
    if n_rays > 4:
        w[4] = -F32(1e-5)
    if n_rays > 5:
        w[5] = -F32(1e-5)
        w[5, 62], w[5, 1] = unit_sum_pair()
    return dict(z=z, weights=w, u_fine=u, d_z_all=rng.standard_normal((n_rays, 128)).astype(F32))


def resample_bwd_refs(inp, q7_mode, mutant=None, fwd=None):
    """-> (fwd, ref64, ref32) on the float32 forward values; `mutant` as in composite_bwd_refs."""
    fwd = resample_forward_f32(inp['z'], inp['weights'], inp['u_fine'], q7_mode) if fwd is None else fwd
    r64 = resample_bwd_ref(fwd, inp['u_fine'], inp['d_z_all'], q7_mode, np.float64)
    r32 = resample_bwd_ref(fwd, inp['u_fine'], inp['d_z_all'], q7_mode, F32, mutant=mutant)
    return fwd, dict(d_weights=r64), dict(d_weights=r32)
