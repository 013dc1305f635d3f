"""mvnerf_fuse_upsample2x (csrc/feature_tail.hip) - act([a | b]) . weight, x2 bilinear, NHWC fp32 / bf16 in one launch - against the
float64 reference of tests/feature_fusion_ref.py.

Bar: the kernel's error against float64 may be at most 8 x the error e32 of the float32 torch run of the same tail
(computed on the CPU here), for the relative L2 and separately for the worst element; e32 is 0.8-3.4e-7 and 0.2-1.8e-6 at these shapes.
Then what makes a fused pass go wrong without being inaccurate: writes outside `out`, elements left unwritten, the bf16 rounding, the
closed form of the up-sampling at corners, edges and tile seams, signed zeros, and run-to-run determinism."""
import numpy as np
import pytest
import torch

from tests import feature_fusion_ref as R
from thesis_clip_nerf_amd import ops

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
GUARD = 2                       # guard rows (of 2w x 256 elements) in front of and behind `out`


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def run_guarded(a, b, weight, act, dtype):
    """The fused call into a NaN-filled `out` between guard rows -> (out, the guards are untouched)."""
    n, h, w, _ = a.shape
    row = 2 * w * 256
    buf = torch.full(((n * 2 * h + 2 * GUARD) * row,), float('nan'), dtype=dtype, device=DEV)
    out = buf[GUARD * row:-GUARD * row].view(n, 2 * h, 2 * w, 256)
    got = ops.fuse_upsample2x(a, b, weight, act, out_dtype=dtype, out=out)
    assert got.data_ptr() == out.data_ptr()
    torch.cuda.synchronize()
    guards_nan = bool(torch.isnan(buf[:GUARD * row]).all() and torch.isnan(buf[-GUARD * row:]).all())
    return out, guards_nan


_runs = {}


def fused(shape):
    """One fp32 and one bf16 run per shape, shared by the tests below."""
    if shape not in _runs:
        a, b, weight = map(dev, R.tail_inputs(shape))
        _runs[shape] = {dtype: run_guarded(a, b, weight, shape[5], dtype) for dtype in (torch.float32, torch.bfloat16)}
    return _runs[shape]


@pytest.mark.parametrize('shape', R.TAIL_SHAPES, ids=str)
def test_against_the_float64_reference(shape):
    a, b, weight = R.tail_inputs(shape)
    ref = R.tail_ref(a, b, weight, shape[5])
    e32_l2, e32_worst = R.float32_tail_error(shape)
    out, guards_nan = fused(shape)[torch.float32]
    assert guards_nan, 'wrote outside out'
    assert torch.isfinite(out).all(), 'left elements unwritten'
    got = out.cpu().numpy()
    e_l2, e_worst = R.rel_l2(got, ref), R.worst(got, ref)
    print(f'{shape}: rel L2 {e_l2:.3g} (float32 torch {e32_l2:.3g}), worst element {e_worst:.3g} (float32 torch {e32_worst:.3g})')
    assert e_l2 <= R.TAIL_BAR * e32_l2, (e_l2, e32_l2)
    assert e_worst <= R.TAIL_BAR * e32_worst, (e_worst, e32_worst)


@pytest.mark.parametrize('shape', R.TAIL_SHAPES, ids=str)
def test_bf16_output_is_the_rounded_fp32_output(shape):
    runs = fused(shape)
    out16, guards_nan = runs[torch.bfloat16]
    assert guards_nan, 'wrote outside out'
    assert torch.isfinite(out16.float()).all(), 'left elements unwritten'
    want = runs[torch.float32][0].to(torch.bfloat16)
    assert torch.equal(out16.view(torch.int16), want.view(torch.int16))


def _closed_form(h, w, py, px, row):
    """Up-sampling of a map that is `row` (256,) at low pixel (py, px) and 0 elsewhere, with the clamped taps folded: exact in fp32
    for a row of small integers / 8."""
    def taps(n_low, p):
        wts = np.zeros(2 * n_low)
        for Y in range(2 * n_low):
            i0 = (Y - 1) >> 1
            for i, wt in ((i0, 0.75 if Y % 2 else 0.25), (i0 + 1, 0.25 if Y % 2 else 0.75)):
                if min(max(i, 0), n_low - 1) == p:
                    wts[Y] += wt
        return wts
    return (taps(h, py)[:, None, None] * taps(w, px)[None, :, None] * row[None, None, :]).astype(np.float32)


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16], ids=['fp32', 'bf16'])
def test_identity_is_exact_at_corners_edges_seams_and_inside(dtype):
    """One input channel set to 1 at one low-resolution pixel, a weight of small integers / 8: the output is {9, 3, 3, 1} / 16 of that
    weight row around the pixel (folded where the taps clamp), bit for bit.  9 x 19 low pixels: two tiles each way."""
    h, w, ca, cb = 9, 19, 16, 32
    rng = np.random.default_rng(3)
    weight = rng.integers(-8, 9, (ca + cb, 256)).astype(np.float32) / 8
    # corners, a pixel on each edge, interior pixels at the tile seams (low row 6 and low column 14 belong to two tiles), one well inside
    places = [(0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1), (0, 7), (h - 1, 9), (4, 0), (3, w - 1), (5, 13), (6, 14), (5, 14), (6, 13), (2, 4)]
    a = np.zeros((len(places), h, w, ca), np.float32)
    b = np.zeros((len(places), h, w, cb), np.float32)
    ks = [int(k) for k in rng.integers(0, ca + cb, len(places))]
    ks[0], ks[1] = 0, ca + cb - 1
    for n, ((py, px), k) in enumerate(zip(places, ks)):
        (a if k < ca else b)[n, py, px, k if k < ca else k - ca] = 1.0
    out, guards_nan = run_guarded(dev(a), dev(b), dev(weight), None, dtype)
    assert guards_nan
    for n, ((py, px), k) in enumerate(zip(places, ks)):
        want = torch.from_numpy(_closed_form(h, w, py, px, weight[k])).to(dtype)      # multiples of 1/128 below 16: exact in bf16 too
        assert torch.equal(out[n].cpu(), want), (py, px, k)
        assert float(want.float().sum()) == pytest.approx(4.0 * float(weight[k].sum()))      # the taps of one low pixel sum to 4


@pytest.mark.parametrize('act', [None, 'relu', 'elu'])
def test_zero_weight_gives_positive_zeros(act):
    a, b, _ = R.tail_inputs((1, 9, 17, 16, 16, act))
    for dtype, bits in ((torch.float32, torch.int32), (torch.bfloat16, torch.int16)):
        out, guards_nan = run_guarded(dev(a), dev(b), torch.zeros(32, 256, device=DEV), act, dtype)
        assert guards_nan and not out.view(bits).any()                                   # +0.0 everywhere: no sign bit either


def test_identical_images_give_identical_halves_and_runs_repeat():
    shape = (2, 9, 11, 128, 256, 'elu')
    a, b, weight = R.tail_inputs(shape)
    a[1], b[1] = a[0], b[0]
    first = ops.fuse_upsample2x(dev(a), dev(b), dev(weight), 'elu')
    assert torch.equal(first[0], first[1])
    again = ops.fuse_upsample2x(dev(a), dev(b), dev(weight), 'elu')
    assert torch.equal(first.view(torch.int32), again.view(torch.int32))
    single = ops.fuse_upsample2x(dev(a[:1]), dev(b[:1]), dev(weight), 2)                 # the integer code of 'elu'
    assert torch.equal(single[0], first[0])


def test_wrapper_checks_its_arguments():
    a, b, weight = map(dev, R.tail_inputs((1, 3, 4, 16, 32, None)))
    assert ops.fuse_upsample2x(a, b, weight, 'identity').shape == (1, 6, 8, 256)
    with pytest.raises(ValueError):
        ops.fuse_upsample2x(a, b, weight, 'gelu')
    with pytest.raises(ValueError):
        ops.fuse_upsample2x(a, b[:, :2], weight, None)
    with pytest.raises(ValueError):
        ops.fuse_upsample2x(a, b, weight[:, :128].contiguous(), None)
    with pytest.raises(ValueError):
        ops.fuse_upsample2x(a, b, weight, None, out_dtype=torch.float16)
    with pytest.raises(ValueError):
        ops.fuse_upsample2x(a, b, weight, None, out=torch.empty(1, 6, 8, 256, dtype=torch.bfloat16, device=DEV))
    with pytest.raises(ValueError, match='Ca=24'):
        ops.fuse_upsample2x(torch.zeros(1, 3, 4, 24, device=DEV), torch.zeros(1, 3, 4, 24, device=DEV), weight, None)
