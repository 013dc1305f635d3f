"""Block-local float64 references for the four fp32-grade forward field kernels.  TEST INFRASTRUCTURE ONLY (NumPy).

The kernels: fp32 MFMA (csrc/field_eval.hip), two fp16 pieces / three products (csrc/field_eval_split16_impl.h, MVS16_F16 = 1, and its
range-guarded copy), the exact bf16 cut on 16x16x32 (same file, MVS16_F16 = 0) and on 32x32x16 (csrc/field_eval_split.hip).  Every
reference starts from the kernel's OWN fp32 input of that section (`dense_ref`, `block_ref`, `view_mean_ref`, `readout_ref`,
`table_ref`) or from the oracle's bit-exact fp32 geometry (`layer0_ref`), so a comparison isolates one section's arithmetic.  Nothing
is rounded to 16 bits in a reference - unlike oracle/field_bf16_ref.py there are no undecided sets: every bar is elementwise, no row
is exempt and no share is capped.

Bars ("what holds the fp32-grade forward kernels"):
  * hidden Dense, ResNet block, texel table, layer 0 in table form: 16 * 2^-24 * max |ref| (`bar16`, the bar of
    tests/test_gpu_split.py::test_products_of_the_three_fp32_grade_kernels_against_float64);
  * layer 0, direct form (K = 379): max(bar16, 2 x the worst element of `seq32` against the same reference) and rel-L2 <= 2 x
    seq32's (`layer0_bar`): seq32 is the longest legitimate fp32 rounding chain, the factor 2 covers other summation orders;
  * view mean: (V + 2) * 2^-24 * max_v |x_v| per element (V - 1 additions and a division), bit-equal at V = 1;
  * read-out: `readout_bars`;
  * the fp16 form below scale 1: the section's bar + `f16_floor` (`block_floor` for a whole block).

`emulate_f16x3` restates the three-piece fp16 product (exact piece products, float64 sums) for the CPU tests
(tests/test_field_f32_ref.py), which plant defects into it and show that each exceeds its bar.
"""
from __future__ import annotations

import numpy as np

from oracle import mvnerf_oracle as O
from oracle.field_backward_ref import decode_stash, net_sections                                            # noqa: F401  (re-exported)
from oracle.field_bf16_ref import _lerp64, _lerp_fma, _taps, kernel_pe, readout_ref, sincos_f32, table_rows  # noqa: F401

F16, F32, F64 = np.float16, np.float32, np.float64
EPS = 2.0 ** -24
BAR_ULPS = 16.0
PE_DIRECT = {'mfma_f32': (0, 5), 'split_bf16_32x32x16': (0, 5),           # mvnerf_field_common.h pe_cam_xyz
             'split_f16': (0, 5, 8), 'split_bf16': (0, 5, 8)}             # field_eval_split16_impl.h: sincos_f32 at a0, 32 a0, 256 a0
F16_MIN_NORMAL = 2.0 ** -14


def _relu(x):
    return np.maximum(x, 0.0)


# --------------------------------------------------------------------------------------------------------------------------
# the two-piece fp16 representation (csrc/field_eval_split16_impl.h, MVS16_F16 = 1; tests/test_f16_split_math.py pins its claims)
# --------------------------------------------------------------------------------------------------------------------------
def split_weight(w):
    """tw = 64 w: A0 = rn16(tw), A1 = rn16(tw - A0), A0s = A0 / 64 -> A0, A0s, A1 (fp16), the fp32 remainder and tw."""
    tw = (w * F32(64)).astype(F32)
    a0 = tw.astype(F16)
    r = (tw - a0.astype(F32)).astype(F32)
    a1 = r.astype(F16)
    a0s = (a0.astype(F32) * F32(1 / 64)).astype(F16)
    return a0, a0s, a1, r, tw


def split_activation(v):
    """tv = v / 64: B0 = rn16(tv), B1 = rn16(v - 64 B0) -> B0, B1 (fp16), the fp32 remainder and tv."""
    tv = (v * F32(1 / 64)).astype(F32)
    b0 = tv.astype(F16)
    r64 = (v - F32(64) * b0.astype(F32)).astype(F32)           # what v_fma_mix_f32(B0, -64, v) returns
    b1 = r64.astype(F16)
    return b0, b1, r64, tv


def _flush16(p):
    """fp16 subnormals to zero (a matrix pipe that did not honour them)."""
    return np.where(np.abs(p.astype(F64)) < F16_MIN_NORMAL, F16(0), p)


def emulate_f16x3(v, w, drop=None, flush=False):
    """v (N,K) fp32 activations, w (K,M) fp32 weights -> (N,M) float64: sum_k A0s B1 + A1 B0 + A0 B0 with exact piece products and
    float64 sums (the representation alone: no fp32 accumulation noise).
    drop = (term, k range, column range), term in 'A0sB1' | 'A1B0' | 'A0B0': that product left out there (a planted defect);
    flush: subnormal fp16 pieces read as zero (a planted defect)."""
    v, w = np.asarray(v, F32), np.asarray(w, F32)
    a0, a0s, a1, _, _ = split_weight(w)
    b0, b1, _, _ = split_activation(v)
    if flush:
        a0, a0s, a1, b0, b1 = (_flush16(t) for t in (a0, a0s, a1, b0, b1))
    terms = {'A0sB1': (a0s, b1), 'A1B0': (a1, b0), 'A0B0': (a0, b0)}
    out = np.zeros((v.shape[0], w.shape[1]), F64)
    for name, (a, b) in terms.items():
        a = a.astype(F64)
        if drop is not None and drop[0] == name:
            a = a.copy()
            a[drop[1], drop[2]] = 0.0
        out += b.astype(F64) @ a
    assert drop is None or drop[0] in terms
    return out


def f16_floor(v, w):
    """The absolute floor of the fp16 form per output element (N,M): 2^-25 sum_k |W_kj| (B1 = rn16(v - 64 B0) is subnormal for
    |v| < 1/4: absolute error <= 2^-25 per activation) + 2^-31 sum_k |v_k| (A1 subnormal for |w| < 2^-8: <= 2^-31 per weight).
    The two operand floors of tests/test_f16_split_math.py."""
    return 2.0 ** -25 * np.abs(np.asarray(w, F64)).sum(0)[None, :] + 2.0 ** -31 * np.abs(np.asarray(v, F64)).sum(1)[:, None]


# --------------------------------------------------------------------------------------------------------------------------
# hidden layers
# --------------------------------------------------------------------------------------------------------------------------
def dense_ref(x, w, b, relu_in=True, residual=None):
    """[residual +] (relu(x) if relu_in else x) @ w + b in float64 from the kernel's own fp32 x (N,K)."""
    a = np.asarray(x, F64)
    out = (_relu(a) if relu_in else a) @ np.asarray(w, F64) + np.asarray(b, F64)
    return out if residual is None else out + np.asarray(residual, F64)


def block_ref(x, blk):
    """x + relu(relu(x) W1 + b1) W2 + b2 in float64 from the kernel's own block input x (N,128); blk = (W1, b1, W2, b2)."""
    w1, b1, w2, b2 = blk
    return dense_ref(dense_ref(x, w1, b1), w2, b2, residual=x)


def block_floor(x, blk):
    """`f16_floor` of a whole block as seen at its output: the first Dense's floor through |W2| (relu is 1-Lipschitz) plus the
    second Dense's own."""
    w1, b1, w2, _ = blk
    hid = dense_ref(x, w1, b1)
    return f16_floor(_relu(np.asarray(x, F64)), w1) @ np.abs(np.asarray(w2, F64)) + f16_floor(_relu(hid), w2)


def scale_net(flat, k):
    """net_k of the scale sweep: W0, b0 and every hidden bias times 2^-k, the hidden kernels, Wr and br untouched.  relu and the
    residual sums are positively homogeneous, so every trunk activation of net_k is exactly 2^-k times that of net_0 in exact
    arithmetic - and bit for bit in fp32 while nothing is subnormal."""
    out = np.array(flat, F32, copy=True)
    for name, lo, hi in net_sections():
        if name in ('W0', 'b0') or name.endswith(('.b1', '.b2')):
            out[lo:hi] = (out[lo:hi] * F32(2.0 ** -k)).astype(F32)
    return out


def view_mean_ref(x_views):
    """x_views (V,N,128) fp32: the per-view block outputs -> (float64 mean (N,128), bar (N,128) = (V + 2) 2^-24 max_v |x_v|)."""
    x = np.asarray(x_views, F64)
    return x.mean(0), (x.shape[0] + 2) * EPS * np.abs(x).max(0)


def table_ref(features, w0):
    """project_texels / project_texels2: features (..., 256) @ W0[123:379] in float64 -> (..., 128) in the feature order of O."""
    return np.asarray(features, F64) @ np.asarray(w0, F64)[123:379]


# --------------------------------------------------------------------------------------------------------------------------
# layer 0
# --------------------------------------------------------------------------------------------------------------------------
def layer0_parts(net, rays_o, rays_d, z, images, features, intrinsics, extrinsics_inv, table=None, pe_direct=(0, 5), ray_shift=0,
                 swap_lerp=False):
    """The pieces of layer 0, rows ordered (b, v, r, s) -> seed (N,128) float64, inp (N,K) fp32, w (K,128) fp32, extra (N,128) float64.
      * geometry: the oracle's bit-exact fp32 chain (points_on_rays, compute_pixel_in_image_mv, world_to_camera_direction_vector_mv);
      * seed = b0 + W0[60:120]^T PE(cam dir), PE by sincos_f32 at every octave (dir_seed_row), float64 sums;
      * inp = [PE(cam xyz) with the kernel's accurate octaves `pe_direct` | rgb by the oracle's lerp (bit-exact with bilerp) | direct
        form only: the 256 features by the kernels' FMA lerp], w the matching rows of W0;
      * extra: table form only - the float64 lerp of the kernel's own table rows (`table` (B,V,H,W,128) in feature order).
    ray_shift, swap_lerp: planted defects (the seed of the ray `ray_shift` further on; ax and ay exchanged in the table lerp)."""
    b, v, h, w, _ = images.shape
    r, s = z.shape[1:3]
    n = b * v * r * s
    w0 = np.asarray(net['W0'], F32)
    world = O.points_on_rays(rays_o, rays_d, z)
    pix, cam = O.compute_pixel_in_image_mv(world, intrinsics, extrinsics_inv)
    cdir = O.world_to_camera_direction_vector_mv(rays_d, extrinsics_inv)                      # (B,V,R,3)
    seed = kernel_pe(cdir, direct=range(O.N_FREQ)).astype(F64) @ w0[60:120].astype(F64) + np.asarray(net['b0'], F64)
    seed = np.roll(seed, -ray_shift, 2) if ray_shift else seed
    seed = np.broadcast_to(seed[:, :, :, None, :], (b, v, r, s, 128)).reshape(n, 128)
    pe = kernel_pe(cam[..., :3].reshape(n, 3), pe_direct)
    norm_images = (images.astype(F32) * F32(2.0) - F32(1.0)).astype(F32)
    pixq = pix.reshape(b * v, r * s, 2)
    rgb = O.interpolate_bilinear_xy(norm_images.reshape(b * v, h, w, 3), pixq).reshape(n, 3)
    if table is None:
        feat = _lerp_fma(*_taps(features.astype(F32).reshape(b * v, h, w, -1), pixq)).reshape(n, -1)
        return seed, np.concatenate([pe, rgb, feat], -1).astype(F32), np.concatenate([w0[:60], w0[120:]], 0), np.zeros((n, 128))
    tl, tr, bl, br, ax, ay = _taps(np.asarray(table, F32).reshape(b * v, h, w, 128), pixq)
    extra = _lerp64(tl, tr, bl, br, ay, ax) if swap_lerp else _lerp64(tl, tr, bl, br, ax, ay)
    return seed, np.concatenate([pe, rgb], -1).astype(F32), np.concatenate([w0[:60], w0[120:123]], 0), extra.reshape(n, 128)


def layer0_from_parts(seed, inp, w, extra):
    return seed + np.asarray(inp, F64) @ np.asarray(w, F64) + extra


def layer0_ref(net, rays_o, rays_d, z, images, features, intrinsics, extrinsics_inv, table=None, pe_direct=(0, 5)):
    """x0 (N,128) float64 of the direct form (table None) or the texel-table form: see `layer0_parts`."""
    return layer0_from_parts(*layer0_parts(net, rays_o, rays_d, z, images, features, intrinsics, extrinsics_inv, table, pe_direct))


def seq32(seed, inp, w):
    """The yardstick: fp32 accumulation in K order from the fp32 seed, one fused product at a time (acc = fl32(acc + inp_k W_k)) -
    the longest legitimate fp32 rounding chain of the sum.  -> (N,M) fp32."""
    inp, w = np.asarray(inp, F64), np.asarray(w, F64)
    acc = np.asarray(seed, F64).astype(F32)
    for k in range(inp.shape[1]):
        acc = (acc.astype(F64) + inp[:, k:k + 1] * w[k][None, :]).astype(F32)
    return acc


def bar16(ref):
    return BAR_ULPS * EPS * float(np.abs(ref).max())


def rel_l2(got, ref):
    ref = np.asarray(ref, F64)
    return float(np.linalg.norm(np.asarray(got, F64) - ref) / max(np.linalg.norm(ref), 1e-300))


def layer0_bar(ref, seed, inp, w, extra=0.0):
    """The direct form's bar: (max(bar16, 2 x worst element of seq32 against `ref`), 2 x seq32's rel-L2)."""
    yard = seq32(seed, inp, w).astype(F64) + extra
    return max(bar16(ref), 2.0 * float(np.abs(yard - ref).max())), 2.0 * rel_l2(yard, ref)


# --------------------------------------------------------------------------------------------------------------------------
# read-out
# --------------------------------------------------------------------------------------------------------------------------
def readout_bars(emb, net):
    """From the kernel's own embedding (N,128) fp32 -> ref (N,4) float64 [rgb | sigma], elementwise bar (N,4), rel-L2 caps (whole
    (N,4) output, rgb columns, sigma column).
    d_o = 36 * 2^-24 * (sum_k |a_k Wr_kj| + |br_j|) per row: 32 FMAs, 2 shuffle adds, the bias, one to spare; sigmoid' <= 1/4 and
    softplus' <= 1, plus the helper bars of tests/test_device_math_cpu.py::test_readout_activations (1.5e-7 absolute for sigmoid,
    5e-7 relative for softplus).  The rel-L2 caps are 8 x those of the fp32 oracle read-out (O.render_readout) on the same embedding,
    8 being the project's yardstick factor (tests/vit_ref.py)."""
    ref = readout_ref(emb, net, rounded=False)
    a = _relu(np.asarray(emb, F64))
    d_o = 36.0 * EPS * (a @ np.abs(np.asarray(net['Wr'], F64)) + np.abs(np.asarray(net['br'], F64)))
    bar = np.concatenate([0.25 * d_o[:, :3] + 1.5e-7, d_o[:, 3:] + 5e-7 * ref[:, 3:]], -1)
    rgb32, sig32 = O.render_readout(net, np.asarray(emb, F32))
    yard = np.concatenate([rgb32, sig32[:, None]], -1)
    return ref, bar, (8.0 * rel_l2(yard, ref), 8.0 * rel_l2(rgb32, ref[:, :3]), 8.0 * rel_l2(sig32, ref[:, 3]))


COLUMN_CAP_ROWS = 32          # one wave tile


def check_readout(rgbs, emb, net, name):
    """rgbs (N,4) of a kernel against `readout_bars` of its own embedding; prints, asserts, returns the figures.
    The rel-L2 cap is a statistic of the output tensor: it is taken over the whole (N,4) output at every shape, and over the rgb
    columns and the sigma column separately from one tile of rows on.  Below that a column's yardstick is the rounding of a handful
    of values - a single-sample launch leaves ONE sigma, whose fp32 yardstick came out between 9e-10 and 1.8e-7 relative on the GPU
    while the kernels' softplus sits at 1e-8 .. 6e-7 (its helper bar is 5e-7 relative) - and says nothing about the kernel."""
    ref, bar, (cap, cap_rgb, cap_sig) = readout_bars(emb, net)
    rgbs = np.asarray(rgbs, F64)
    err = np.abs(rgbs - ref)
    l2, l2_rgb, l2_sig = rel_l2(rgbs, ref), rel_l2(rgbs[:, :3], ref[:, :3]), rel_l2(rgbs[:, 3], ref[:, 3])
    fig = dict(name=name, rgb=float(err[:, :3].max()), sigma=float(err[:, 3].max()), share=float((err / bar).max()), l2=l2, cap=cap,
               l2_rgb=l2_rgb, l2_sigma=l2_sig, cap_rgb=cap_rgb, cap_sigma=cap_sig)
    print(f'{name}: max |rgb - ref| {fig["rgb"]:.2e}, max |sigma - ref| {fig["sigma"]:.2e}, worst share of the bar {fig["share"]:.3f}, '
          f'rel-L2 {l2:.2e} (cap {cap:.2e}), rgb {l2_rgb:.2e} (cap {cap_rgb:.2e}), sigma {l2_sig:.2e} (cap {cap_sig:.2e})')
    assert np.isfinite(rgbs).all(), name
    assert (err <= bar).all(), (name, 'elementwise', fig['share'])
    assert l2 <= cap, (name, 'rel-L2', l2, cap)
    if len(ref) >= COLUMN_CAP_ROWS:
        assert l2_rgb <= cap_rgb and l2_sig <= cap_sig, (name, 'rel-L2 per column', l2_rgb, cap_rgb, l2_sig, cap_sig)
    return fig


# --------------------------------------------------------------------------------------------------------------------------
# the assertion
# --------------------------------------------------------------------------------------------------------------------------
def check(got, ref, bar, name, l2_cap=None):
    """|got - ref| <= bar elementwise (bar: a number or an array that broadcasts), every element finite, rel-L2 <= l2_cap when given.
    Prints the worst element in units of 2^-24 max |ref| and the rel-L2, then asserts; returns the figures."""
    got, ref = np.asarray(got, F64), np.asarray(ref, F64)
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    scale = float(np.abs(ref).max())
    unit = EPS * scale if scale else EPS
    err = np.abs(got - ref)
    fig = dict(name=name, rows=len(ref), scale=scale, worst=float(err.max() / unit), l2=rel_l2(got, ref),
               share=float((err / np.maximum(bar, 1e-300)).max()))
    print(f'{name}: rows {fig["rows"]} max |ref| {scale:.3g} worst {fig["worst"]:.2f} x 2^-24 max |ref|, rel-L2 {fig["l2"]:.2e}, '
          f'worst share of the bar {fig["share"]:.3f}')
    assert np.isfinite(got).all(), name
    assert (err <= bar).all(), (name, 'elementwise', fig['worst'], fig['share'])
    assert l2_cap is None or fig['l2'] <= l2_cap, (name, 'rel-L2', fig['l2'], l2_cap)
    return fig
