"""float64 references with BOUNDED rounding decisions for the bf16 field kernels.  TEST INFRASTRUCTURE ONLY (NumPy).

The bf16 field pass (csrc/field_eval_bf16.hip: the segment-ring kernel, direct and texel-table form; csrc/field_eval_bf16x.hip: the
layer-ring kernel; project_texels_bf16_kernel) rounds Dense inputs to bfloat16 and accumulates in fp32.  An end-to-end reference
cannot share those rounding decisions - one flipped rounding costs a whole bf16 step - so every reference here is BLOCK-LOCAL:

* it starts from the kernel's own fp32 input of that block (`block_ref`, `readout_ref`, `table_ref`), so the rounding of the input is
  decided exactly, or from the oracle's bit-exact fp32 geometry (`layer0_ref`);
* the one rounding inside a block that cannot be shared, bf16(relu(hid)), is BOUNDED: a kernel whose fp32 `hid` lies in the same
  bf16 rounding cell as the float64 `hid` rounds to the identical value.  Only elements whose float64 value lies within
  c * 2^-24 * mag of a rounding boundary (mag = sum of |products| + |bias|, the scale of an fp32 dot product's error) can differ, and
  then by one bf16 step.  Those elements are the UNDECIDED SET `U`; `flip` is the largest effect they can have on each output.

`check` is the one assertion: |got - ref| <= bar + flip elementwise, <= bar on rows without an undecided element, with caps on the
share of undecided and over-bar rows so that the windows cannot hide a failure.  bar = 16 * 2^-24 * max |ref| is the bar of
tests/test_gpu_split.py::test_products_of_the_three_fp32_grade_kernels_against_float64.
"""
from __future__ import annotations

import numpy as np

from oracle import mvnerf_oracle as O

F32 = np.float32
F64 = np.float64
EPS = 2.0 ** -24
BAR_ULPS = 16.0
C_WINDOW = 2                                  # the c of the undecided window ("rounding-level bars")
DECIDED_SHARE_CAP = {2: 0.80, 4: 0.75, 8: 0.60}
OVER_BAR_SHARE_CAP = 0.01
PE_WINDOW = 4e-7                              # tests/test_device_math_cpu.py::test_sincos_matches_oracle_pe
_MIN_EXP = -126                               # bf16 shares fp32's exponent range; below 2^-126 the spacing stays 2^-133


# --------------------------------------------------------------------------------------------------------------------------
# helpers
# --------------------------------------------------------------------------------------------------------------------------
def bf16_ulp(x):
    """Spacing of bfloat16 at |x| (8 significant bits): 2^(floor(log2 |x|) - 7), 2^-133 in the subnormal range and at 0."""
    ax = np.abs(np.asarray(x, F64))
    _, e = np.frexp(ax)                                             # |x| = m 2^e, m in [0.5, 1)
    return np.ldexp(1.0, np.where(ax > 0, np.maximum(e - 1, _MIN_EXP), _MIN_EXP) - 7)


def boundary_distance(x):
    """Distance of a float64 value to the nearest bf16 ROUNDING BOUNDARY - the midpoint between two neighbouring bf16 values.
    Just above a power of two the cell below is half as wide, so its midpoint (lo - u/4) can be the nearer one."""
    ax = np.abs(np.asarray(x, F64))
    u = bf16_ulp(ax)
    lo = np.floor(ax / u) * u
    d = np.abs(ax - (lo + 0.5 * u))
    m, _ = np.frexp(lo)
    pow2 = (m == 0.5) & (lo > 2.0 ** _MIN_EXP)
    return np.where(pow2, np.minimum(d, ax - lo + 0.25 * u), d)


def q(x):
    """Round to bfloat16 (nearest even), returned as float64.  The value goes through fp32 first (O.bf16_round takes fp32): exact for
    the fp32 arrays this module rounds (activations, weights); for a float64 `hid` the two-step rounding can differ from a direct one
    only within 2^-24 |hid| of a boundary, which is inside every undecided window used here."""
    return O.bf16_round(np.asarray(x, F64).astype(F32)).astype(F64)


def _relu(x):
    return np.maximum(x, 0.0)


# --------------------------------------------------------------------------------------------------------------------------
# one ResNet block from the kernel's own input
# --------------------------------------------------------------------------------------------------------------------------
def block_ref(x, blk, c=C_WINDOW):
    """x (N,128) fp32: the kernel's own block input (so q(relu(x)) is decided exactly); blk = (W1, b1, W2, b2).
    hid = q(relu(x)) @ q(W1) + b1 ; ref = x + q(relu(hid)) @ q(W2) + b2, all float64 (biases and the residual are fp32 in the
    kernels: dense128_bf16 / bias_acc, layer_x).  -> ref (N,128), U (N,128) bool, flip (N,128)."""
    w1, b1, w2, b2 = (np.asarray(t, F64) for t in blk)
    x = np.asarray(x, F64)
    a, w1q, w2q = q(_relu(x)), q(w1), q(w2)
    hid = a @ w1q + b1
    mag = np.abs(a) @ np.abs(w1q) + np.abs(b1)
    und = (hid > 0) & (boundary_distance(hid) <= c * EPS * mag)
    flip = (und * bf16_ulp(hid)) @ np.abs(w2q)
    ref = x + q(_relu(hid)) @ w2q + b2
    return ref, und, flip


# --------------------------------------------------------------------------------------------------------------------------
# layer 0
# --------------------------------------------------------------------------------------------------------------------------
def _fma(a, b, c):
    """fmaf restated: the product of two fp32 is exact in float64; the sum is rounded to float64 and then to fp32 (a double rounding
    that differs from the single one in ~2^-29 of the cases, by one fp32 ulp - inside the windows below)."""
    return (np.asarray(a, F64) * np.asarray(b, F64) + np.asarray(c, F64)).astype(F32)


def sincos_f32(x):
    """mvnerf_math.h sincos_f32 / sincos_reduced (|x| < 1e5) operation by operation in fp32."""
    x = np.asarray(x, F32)
    assert np.all(np.abs(x) < 100000.0)
    j = np.rint((x * F32(0.636619747)).astype(F32)).astype(F32)
    r = _fma(j, F32(-1.57079601e+00), x)
    r = _fma(j, F32(-3.13916473e-07), r)
    r = _fma(j, F32(-5.39030253e-15), r)
    k = j.astype(np.int64)
    s2 = (r * r).astype(F32)
    ps = np.full_like(s2, F32(2.86567956e-6))
    for coef in (-1.98559923e-4, 8.33338592e-3, -1.66666672e-1):
        ps = _fma(ps, s2, F32(coef))
    sn = _fma(ps, (r * s2).astype(F32), r)
    pc = np.full_like(s2, F32(2.44677067e-5))
    for coef in (-1.38877297e-3, 4.16666567e-2, -5.00000000e-1):
        pc = _fma(pc, s2, F32(coef))
    cs = _fma(pc, s2, F32(1.0))
    s = np.where(k & 1, cs, sn)
    cc = np.where(k & 1, sn, cs)
    s = np.where(k & 2, -s, s)
    cc = np.where((k + 1) & 2, -cc, cc)
    return s.astype(F32), cc.astype(F32)


def kernel_pe(position, direct=(0, 5)):
    """PE(cam xyz) as the field kernels form it, layout (d, k, {sin, cos}) of O.position_encoding: a0 = x * fl32(pi); octave k in
    `direct` is sincos_f32(a0 * 2^k) (2^k a0 == fl32(x * fl32(pi 2^k)) exactly), every other octave the double-angle step of the one
    below (s' = 2 s c, c' = fma(-2 s, s, 1)).  direct = (0, 5): field_eval_bf16.hip:413-429; (0, 5, 8): field_eval_bf16x.hip:336-381
    (lane groups 0..2 hold octaves 0..7, group 3 octaves 8, 9 from an accurate sin/cos at 256 a0); range(10): dir_bias_kernel."""
    a0 = (np.asarray(position, F32) * F32(3.14159274101257324)).astype(F32)
    out = np.empty(a0.shape + (O.N_FREQ, 2), F32)
    sk = ck = None
    for k in range(O.N_FREQ):
        if k in direct:
            sk, ck = sincos_f32((a0 * F32(1 << k)).astype(F32))
        else:
            s2 = (sk + sk).astype(F32)
            cn = _fma(-s2, sk, F32(1.0))
            sk = (s2 * ck).astype(F32)
            ck = cn
        out[..., k, 0], out[..., k, 1] = sk, ck
    return out.reshape(*a0.shape[:-1], -1)


def _taps(grid, pix):
    """The four fp32 taps and lerp factors of O.interpolate_bilinear_xy: grid (N,H,W,C), pix (N,Q,2) -> tl, tr, bl, br (N,Q,C), ax, ay."""
    n, h, w, ch = grid.shape
    x0, y0, ax, ay = O.bilinear_taps(pix, h, w)
    flat = grid.reshape(n * h * w, ch)
    idx = O.tap_linear_indices(x0, y0, np.arange(n, dtype=np.int64)[:, None], h, w)
    return [flat[idx[..., i]] for i in range(4)] + [ax[..., None], ay[..., None]]


def _lerp_fma(tl, tr, bl, br, ax, ay):
    """The gathers' lerp: top = fma(ax, tr - tl, tl), bot = fma(ax, br - bl, bl), out = fma(ay, bot - top, top)
    (field_eval_bf16.hip:473-475 and :538-540, field_eval_bf16x.hip:435-437)."""
    top = _fma(ax, (tr - tl).astype(F32), tl)
    bot = _fma(ax, (br - bl).astype(F32), bl)
    return _fma(ay, (bot - top).astype(F32), top)


def _lerp64(tl, tr, bl, br, ax, ay):
    tl, tr, bl, br, ax, ay = (np.asarray(t, F64) for t in (tl, tr, bl, br, ax, ay))
    top = ax * (tr - tl) + tl
    bot = ax * (br - bl) + bl
    return ay * (bot - top) + top


def layer0_ref(net, rays_o, rays_d, z, images, features, intrinsics, extrinsics_inv, table=None, pe_direct=(0, 5), fused_lerp=True):
    """Layer 0 (x0, rows ordered (b, v, r, s)) of the direct form (table None) or the texel-table form (table (B,V,H,W,128): the
    kernel's own input table, in the feature order of O - see `table_rows`).

    Geometry is the oracle's fp32 chain (points_on_rays, compute_pixel_in_image_mv, world_to_camera_direction_vector_mv, bilinear_taps:
    bit-exact with the kernels, test_field_eval_matches_oracle / test_geometry_chain_bit_exact).  Rounding sites mirrored, with the
    source lines that document them:
      * seed b0 + W0[60:120]^T PE(cam dir): fp32, never rounded to bf16 (field_eval.hip:287-312 dir_bias_kernel, sincos_f32 at every
        octave; field_eval_bf16.hip:399 / field_eval_bf16x.hip:331-335 load it into the accumulators);
      * PE(cam xyz): `kernel_pe` with the kernel's accurate octaves `pe_direct`, rounded to bf16 (field_eval_bf16.hip:430-437,
        field_eval_bf16x.hip:383-394); pe_direct=None takes O.position_encoding (the NumPy restatement);
      * rgb: bilerp of 2 img - 1 without FMA (mvnerf_math.h:126-130, bit-exact with O), rounded to bf16 with PE (same lines);
      * direct form: features lerped in fp32 with FMAs and rounded ONCE to bf16 (field_eval_bf16.hip:536-545); fused_lerp=False takes
        the oracle's lerp without FMA (the NumPy restatement);
      * table form: the feature part is an fp32 FMA lerp of table rows added to the fp32 accumulators, no bf16 rounding
        (field_eval_bf16.hip:470-488, field_eval_bf16x.hip:432-450): float64 lerp of the fp32 taps here;
      * weights W0[0:60], W0[120:379] rounded to bf16 (pack_net_bf16_kernel / pack_net_bf16x_kernel); fp32 accumulation.
    Undecided windows: PE(xyz) 4e-7 absolute (the sincos_f32 bar, test_sincos_matches_oracle_pe), rgb and lerped features one fp32 ulp
    (test_bilerp_bit_exact; the restated FMA's double rounding).  -> ref (N,128), U (N,K) bool over the rounded inputs, flip (N,128)."""
    b, v, h, w, _ = images.shape
    r, s = z.shape[1:3]
    n = b * v * r * s
    w0 = np.asarray(net['W0'], F64)
    world = O.points_on_rays(rays_o, rays_d, z)
    pix, cam = O.compute_pixel_in_image_mv(world, intrinsics, extrinsics_inv)
    cdir = O.world_to_camera_direction_vector_mv(rays_d, extrinsics_inv)                      # (B,V,R,3)
    pe_dir = kernel_pe(cdir, direct=range(O.N_FREQ)).astype(F64)
    seed = pe_dir @ w0[60:120] + np.asarray(net['b0'], F64)                                    # (B,V,R,128)
    seed = np.broadcast_to(seed[:, :, :, None, :], (b, v, r, s, 128)).reshape(n, 128)
    xyz = cam[..., :3].reshape(n, 3)
    pe = (O.position_encoding(xyz) if pe_direct is None else kernel_pe(xyz, pe_direct)).astype(F64)
    norm_images = (images.astype(F32) * F32(2.0) - F32(1.0)).astype(F32)
    pixq = pix.reshape(b * v, r * s, 2)
    rgb = O.interpolate_bilinear_xy(norm_images.reshape(b * v, h, w, 3), pixq).reshape(n, 3).astype(F64)
    cols = [pe, rgb]
    wins = [np.full(pe.shape, PE_WINDOW), 2 * EPS * np.abs(rgb)]
    rows = [w0[:60], w0[120:123]]
    extra = 0.0
    if table is None:
        taps = _taps(features.astype(F32).reshape(b * v, h, w, -1), pixq)
        feat = (_lerp_fma(*taps) if fused_lerp else O.interpolate_bilinear_xy(features.astype(F32).reshape(b * v, h, w, -1), pixq))
        feat = feat.reshape(n, -1).astype(F64)
        cols.append(feat)
        wins.append(2 * EPS * np.abs(feat))
        rows.append(w0[123:])
    else:
        extra = _lerp64(*_taps(np.asarray(table, F32).reshape(b * v, h, w, 128), pixq)).reshape(n, 128)
    inp, win, wq = np.concatenate(cols, -1), np.concatenate(wins, -1), q(np.concatenate(rows, 0))
    und = boundary_distance(inp) <= win
    flip = (und * bf16_ulp(inp)) @ np.abs(wq)
    ref = seed + q(inp) @ wq + extra
    return ref, und, flip


# --------------------------------------------------------------------------------------------------------------------------
# read-out and texel table: the input is given, nothing is undecided
# --------------------------------------------------------------------------------------------------------------------------
def readout_ref(emb, net, rounded):
    """Read-out from the kernel's own embedding (N,128) fp32 -> (N,4) float64 [sigmoid(o[:3]) | softplus(o[3])].
    rounded=True: relu(emb) and Wr rounded to bf16 (the segment kernel's MFMA read-out, field_eval_bf16.hip:602-615);
    False: both fp32 (the layer-ring kernel's vector-ALU read-out, field_eval_bf16x.hip:517-541).  br is fp32 in both."""
    a, wr = _relu(np.asarray(emb, F64)), np.asarray(net['Wr'], F64)
    if rounded:
        a, wr = q(a), q(wr)
    o = a @ wr + np.asarray(net['br'], F64)
    return np.concatenate([1.0 / (1.0 + np.exp(-o[:, :3])), np.logaddexp(0.0, o[:, 3:])], -1)


def table_ref(features, w0):
    """project_texels_bf16: q(features) @ q(W0[123:379]) in float64, (..., 256) -> (..., 128) in the feature order of O."""
    return q(features) @ q(np.asarray(w0)[123:379])


def table_rows(table):
    """A kernel texel table (..., 128) is stored in the 32x32 accumulator order [h][nb][q][c] = feature 32 nb + 8 q + 4 h + c
    (field_eval_bf16.hip:209-217: out = table + 128 t + 64 h + 16 nb, f32x4 number q holds accumulator registers 4q..4q+3 =
    output rows 8 q + 4 h + {0..3} of block nb) -> the same table in feature order."""
    t = np.asarray(table)
    return t.reshape(*t.shape[:-1], 2, 4, 4, 4).swapaxes(-4, -3).swapaxes(-3, -2).reshape(t.shape)


# --------------------------------------------------------------------------------------------------------------------------
# the assertion
# --------------------------------------------------------------------------------------------------------------------------
def check(got, ref, U=None, flip=None, name='', c=C_WINDOW):
    """|got - ref| <= bar + flip elementwise (no row exempt); <= bar on decided rows (no element in U); share of decided rows >= the
    cap of c (0.80 at c = 2); share of rows with any element over bar <= 1 % - from 100 rows on exactly these shares, below that one
    row may be undecided or over the bar (inside its window).  bar = 16 * 2^-24 * max |ref|.  Prints its figures, then asserts;
    returns them."""
    got, ref = np.asarray(got, F64), np.asarray(ref, F64)
    assert got.shape == ref.shape and got.ndim == 2, (got.shape, ref.shape)
    scale = float(np.abs(ref).max())
    bar = BAR_ULPS * EPS * scale
    err = np.abs(got - ref)
    und_rows = np.zeros(len(ref), bool) if U is None else np.asarray(U).any(1)
    flip = np.zeros_like(ref) if flip is None else flip
    over_rows = (err > bar).any(1)
    fig = dict(name=name, rows=len(ref), scale=scale, decided_share=float(1.0 - und_rows.mean()),
               worst_decided=float(err[~und_rows].max() / (EPS * scale)) if (~und_rows).any() else 0.0,
               worst=float(err.max() / (EPS * scale)), over_bar_share=float(over_rows.mean()),
               over_bar_outside_window=int((over_rows & ~und_rows).sum()), max_flip=float(flip.max() / scale) if scale else 0.0)
    print(f'{name}: rows {fig["rows"]} scale {scale:.3g} decided {fig["decided_share"]:.4f} worst decided row {fig["worst_decided"]:.2f} '
          f'x 2^-24 scale, worst row {fig["worst"]:.1f}, rows over bar {fig["over_bar_share"]:.4f} ({fig["over_bar_outside_window"]} decided), '
          f'max flip {fig["max_flip"]:.2e} scale (c = {c})')
    assert np.isfinite(got).all(), name
    assert (err <= bar + flip).all(), (name, 'elementwise', float((err - flip).max() / (EPS * scale)))
    assert (err[~und_rows] <= bar).all(), (name, 'decided rows', fig['worst_decided'])
    # the caps as row counts: a share of n rows cannot be finer than one row, so one row is always allowed (a single-sample launch)
    n = len(ref)
    assert und_rows.sum() <= max(1, int((1.0 - DECIDED_SHARE_CAP[c]) * n + 1e-9)), (name, 'decided share', fig['decided_share'])
    assert over_rows.sum() <= max(1, int(OVER_BAR_SHARE_CAP * n + 1e-9)), (name, 'over-bar share', fig['over_bar_share'])
    return fig
